// BatchNorm backward folded through the 1x1 convolution in front of it (ResNet identity bottleneck: conv3 -> bn3).
//
// With yc = y2 * W^T (W = w[co][ci], y2 the 4x narrower conv input), g the masked output gradient and the BN
// backward dx = A g + B yc + K (per-channel A, B, K: bn_bwd_finalize's coef), everything the backward needs is
// a function of the small products P = g^T y2 [Co][Ci], S = y2^T y2 [Ci][Ci] and s = sum_p y2 [Ci]:
//   sum_p g yc [co]   = sum_ci w[co][ci] P[co][ci]                         (the BN-backward reduce)
//   dW[co][ci]        = A_co P[co][ci] + B_co sum_cj w[co][cj] S[cj][ci] + K_co s[ci]
//   d y2              = g (A (.) W) + y2 Gm + kv,   Gm[cj][ci] = sum_co B_co w[co][cj] w[co][ci],
//                                                    kv[ci]    = sum_co K_co w[co][ci]
// so neither the BN input yc nor dx (both [M][Co]) is read or written by the backward.  The two kernels here
// are the per-channel glue: bn_fold_sums (before bn_bwd_finalize) and bn_fold_coef (after it).  All sums fp32
// (the reduce's cancellation sum g (yc - mean) in double).
#include "ddl_common.h"
#include "ddl_ops.h"

namespace ddl {
namespace {

constexpr int FT = 32;    // output tile of the small products
constexpr int BKG = 128;  // reduction rows staged per step: Gm (over Co; each step is one round of global-load
constexpr int BKW = 64;   // latency, so few deep steps) and dW (over Ci)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// blocks [0, cb): one wave per output channel co -> sums[0][co] = sum g, sums[1][co] = sum g (yc - mean)
// blocks [cb, ..): s[ci] += the column sums of y2 from the partial rows of a bn_stats sweep (s zeroed by the
// caller; kSumSplit blocks share the rows of 64 columns, each thread a handful of independent loads)
constexpr int kSumSplit = 8;
__global__ __launch_bounds__(256) void bn_fold_sums_kernel(const bf16_t* __restrict__ w, long ldw,
                                                            const float* __restrict__ P,
                                                            const float* __restrict__ wsg,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ wsy, int rows,
                                                            float* __restrict__ sums, float* __restrict__ s, int Co,
                                                            int Ci, int cb) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((int)blockIdx.x < cb) {
    const int co = blockIdx.x * 4 + wv;
    if (co >= Co) return;
    double dot = 0.0;
    for (int ci = lane; ci < Ci; ci += 64) dot += (double)bf2f(w[(long)co * ldw + ci]) * (double)P[(long)co * Ci + ci];
    double sg = lane < kBnShards ? (double)wsg[(long)lane * 2 * Co + co] : 0.0;
    dot = wave_sum(dot);
    sg = wave_sum(sg);
    if (lane == 0) {
      sums[co] = (float)sg;
      sums[Co + co] = (float)(dot - (double)mean[co] * sg);
    }
  } else {
    __shared__ float red[4][64];
    const int sb = (int)blockIdx.x - cb;
    const int ci = (sb / kSumSplit) * 64 + lane;
    float a = 0.f;
    if (ci < Ci) {
#pragma unroll 8
      for (int r = (sb % kSumSplit) * 4 + wv; r < rows; r += 4 * kSumSplit) a += wsy[(long)r * 2 * Ci + ci];
    }
    red[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && ci < Ci) atomicAdd(s + ci, (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
  }
}

// blocks [0, nG): a 32x32 tile of Gm (bf16);  [nG, nG + nW): a 32x32 tile of dW (+=) and of the scaled
// weights WA = bf16(A (.) W) ([Co][Ci]) and their transpose WAt ([Ci][Co]).  The Gm blocks of the first tile row
// (m0 = 0) also form kv for their 32 columns from the weight rows they stage anyway.
__global__ __launch_bounds__(256) void bn_fold_coef_kernel(const bf16_t* __restrict__ w, long ldw,
                                                            const float* __restrict__ P,
                                                            const float* __restrict__ S,
                                                            const float* __restrict__ s,
                                                            const float* __restrict__ coef, bf16_t* __restrict__ WA,
                                                            bf16_t* __restrict__ WAt, bf16_t* __restrict__ Gm,
                                                            float* __restrict__ kv, float* __restrict__ dW, long lddw,
                                                            int Co, int Ci) {
  __shared__ float As[BKG][FT + 1], Bs[BKG][FT + 1];
  const int tc = Ci / FT;
  const int nG = tc * tc, nW = (Co / FT) * tc;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // outputs (ty + 8 i, tx), i < 4
  const float* cA = coef;
  const float* cB = coef + Co;
  const float* cK = coef + 2 * Co;
  int b = blockIdx.x;
  if (b >= nG + nW) return;
  const bool gm = b < nG;
  if (!gm) b -= nG;
  const int m0 = (b / tc) * FT, n0 = (b % tc) * FT;
  const int Kd = gm ? Co : Ci;
  const int bk = gm ? BKG : BKW;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float kvp = 0.f;  // this thread's rows of sum_co K_co w[co][n0 + tx]
  for (int k0 = 0; k0 < Kd; k0 += bk) {
    if (gm) {  // As[k][m] = B_co w[co][m0 + m], Bs[k][n] = w[co][n0 + n], co = k0 + k
#pragma unroll
      for (int i = 0; i < BKG / 8; ++i) {
        const int r = ty + 8 * i;
        const long row = (long)(k0 + r) * ldw;
        As[r][tx] = cB[k0 + r] * bf2f(w[row + m0 + tx]);
        const float wn = bf2f(w[row + n0 + tx]);
        Bs[r][tx] = wn;
        kvp = fmaf(cK[k0 + r], wn, kvp);
      }
    } else {  // As[k][m] = w[m0 + m][k0 + k] (loaded along k), Bs[k][n] = S[k0 + k][n0 + n]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < BKW / 32; ++h)
          As[tx + 32 * h][ty + 8 * i] = bf2f(w[(long)(m0 + ty + 8 * i) * ldw + k0 + tx + 32 * h]);
#pragma unroll
      for (int i = 0; i < BKW / 8; ++i) Bs[ty + 8 * i][tx] = S[(long)(k0 + ty + 8 * i) * Ci + n0 + tx];
    }
    __syncthreads();
#pragma unroll 16
    for (int k = 0; k < bk; ++k) {
      const float bv = Bs[k][tx];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(As[k][ty + 8 * i], bv, acc[i]);
    }
    __syncthreads();
  }
  if (gm && m0 == 0) {  // block-uniform; the K loop ended with a barrier, As is free
    As[ty][tx] = kvp;
    __syncthreads();
    if (ty == 0) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) a += As[j][tx];
      kv[n0 + tx] = a;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, n = n0 + tx;
    if (gm) {
      Gm[(long)m * Ci + n] = f2bf(acc[i]);
    } else {
      const bf16_t wa = f2bf(cA[m] * bf2f(w[(long)m * ldw + n]));
      WA[(long)m * Ci + n] = wa;
      WAt[(long)n * Co + m] = wa;
      dW[(long)m * lddw + n] += cA[m] * P[(long)m * Ci + n] + cB[m] * acc[i] + cK[m] * s[n];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Forward side of the fold: conv3 is 1x1, so bn3's batch statistics follow from the narrow tensor alone,
//   sum_p yc[p][co] = w_co . s,   sum_p yc[p][co]^2 = w_co^T S w_co,   S = y2^T y2, s = sum_p y2
// and conv3's output is never written: gram_colsum reads y2 once for S and s (which the folded backward needs
// anyway), bn_fold_fwd_stats turns them into the [shard][2][Co] sums bn_finalize takes.

// One 32-KB tile of y2 rows per step: TP rows of CI channels, staged row-major in LDS (rows padded by 16 B: the
// 4-row x 16-column blocks of the transposed reads then fall on distinct banks) and consumed on both MFMA
// sides through ds_read_b64_tr_b16 — the fragment addressing of ddl_gemm_kernel.h's row-contiguous operands.
template <int CI>
struct GramCfg {
  static constexpr int TP = CI == 64 ? 256 : (CI == 128 ? 128 : 64);
  static constexpr int ROWB = CI * 2 + 16;
  static constexpr int CH = CI / 8;      // 16-B chunks per row
  static constexpr int PPP = 256 / CH;   // rows per load pass of the workgroup
  static constexpr int V = TP / PPP;     // 16-B loads per thread per tile
  static constexpr int RB = CI / 16;     // 16-row blocks of S
  static constexpr int P = CI / 64;      // 64-column panels of S, one workgroup each
  static_assert(V == 8 && TP % 32 == 0 && PPP * CI * 4 <= TP * ROWB, "gram tile shape");
};

// fragment of channels c0 + (lane & 15), tile rows 32 kk + 8 (lane >> 4) + j
template <int ROWB>
__device__ __forceinline__ bf16x8 gram_frag(const char* lds, int kk, int c0, int lane) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int k1 = kk * 32 + 8 * g + q;
  const int off = k1 * ROWB + (c0 + 4 * p) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DDL_LDS s16x4*)(lds + off));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DDL_LDS s16x4*)(lds + off + 4 * ROWB));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// workgroup (chunk, panel): rows [chunk * rows_per_wg, +rows_per_wg) of y2, columns [64 panel, +64) of S, wave w
// the 16 columns 64 panel + 16 w of every row block.  fp32 accumulators over the workgroup's rows, then one
// atomic per element into the zeroed S; the panel-0 workgroups also sum the columns of the rows they load.
// Two levels: the MFMA chain restarts from zero every tile and its result is added to the running total with a
// round-to-nearest VALU add — a long MFMA accumulation chain on an all-positive sum drifts (measured: chains of
// 32 k-steps 1.5x the error of chains of 16).
template <int CI>
__global__ __launch_bounds__(256) void gram_colsum_kernel(const bf16_t* __restrict__ y2, long ld, int M,
                                                           int rows_per_wg, float* __restrict__ S,
                                                           float* __restrict__ s) {
  using G = GramCfg<CI>;
  __shared__ __attribute__((aligned(16))) char tile[G::TP * G::ROWB];
  const int panel = (int)blockIdx.x % G::P, chunk = (int)blockIdx.x / G::P;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ch = threadIdx.x % G::CH, pr = threadIdx.x / G::CH;
  const int r0 = chunk * rows_per_wg;
  const int r1 = min(M, r0 + rows_per_wg);
  const int cb = (panel * 4 + w) * 16;
  f32x4 tot[G::RB];
#pragma unroll
  for (int i = 0; i < G::RB; ++i) tot[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;
  uint4 reg[G::V];
  auto load = [&](int t0) {  // rows past the workgroup's range load zeros: they add nothing to S or s
#pragma unroll
    for (int v = 0; v < G::V; ++v) {
      const int row = t0 + pr + v * G::PPP;
      reg[v] = row < r1 ? *reinterpret_cast<const uint4*>(y2 + (long)row * ld + ch * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  load(r0);
  for (int t0 = r0; t0 < r1; t0 += G::TP) {
    __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
    for (int v = 0; v < G::V; ++v)
      *reinterpret_cast<uint4*>(tile + (pr + v * G::PPP) * G::ROWB + ch * 16) = reg[v];
    if (panel == 0) {
#pragma unroll
      for (int v = 0; v < G::V; ++v) {
        const uint32_t wv[4] = {reg[v].x, reg[v].y, reg[v].z, reg[v].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          cs[2 * q] += __uint_as_float(wv[q] << 16);
          cs[2 * q + 1] += __uint_as_float(wv[q] & 0xffff0000u);
        }
      }
    }
    __syncthreads();
    if (t0 + G::TP < r1) load(t0 + G::TP);  // the next tile's loads fly under this tile's MFMAs
    f32x4 acc[G::RB];
#pragma unroll
    for (int i = 0; i < G::RB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int kk = 0; kk < G::TP / 32; ++kk) {
      const bf16x8 b = gram_frag<G::ROWB>(tile, kk, cb, lane);
#pragma unroll
      for (int i = 0; i < G::RB; ++i) acc[i] = mfma16x16x32(gram_frag<G::ROWB>(tile, kk, 16 * i, lane), b, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < G::RB; ++i) tot[i] += acc[i];
  }
  // tot[i][e] = S[16 i + 4 (lane >> 4) + e][cb + (lane & 15)]
#pragma unroll
  for (int i = 0; i < G::RB; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      atomicAdd(S + (long)(16 * i + 4 * (lane >> 4) + e) * CI + cb + (lane & 15), tot[i][e]);
  if (panel == 0) {  // block-uniform
    __syncthreads();
    float* red = reinterpret_cast<float*>(tile);  // [PPP][CI]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pr * CI + ch * 8 + e] = cs[e];
    __syncthreads();
    if ((int)threadIdx.x < CI) {
      double a = 0.0;
      for (int j = 0; j < G::PPP; ++j) a += (double)red[j * CI + threadIdx.x];
      atomicAdd(s + threadIdx.x, (float)a);
    }
  }
}

// One wave per output channel co: mean = w_co . s_bar, var = w_co^T (S / M - s_bar s_bar^T) w_co with
// s_bar = s / M.  y2 is post-ReLU, so S is dominated by the outer product of its mean: the covariance is
// centred element by element and the quadratic form summed in double.  Writes sum = M mean and
// sumsq = M (var + mean^2) to shard row 0 of the zeroed [kBnShards][2][Co] workspace (bn_finalize's input).
// S passes through LDS FST rows at a time, shared by the block's four channels.
constexpr int FST = 32;
__global__ __launch_bounds__(256) void bn_fold_fwd_stats_kernel(const bf16_t* __restrict__ w, long ldw,
                                                                 const float* __restrict__ S,
                                                                 const float* __restrict__ s, long M,
                                                                 float* __restrict__ ws, int Co, int Ci) {
  __shared__ float Ssh[FST][256];
  __shared__ double wsh[4][256];
  __shared__ double sb[256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int co = (int)blockIdx.x * 4 + wv;
  const int cor = min(co, Co - 1);
  const double invM = 1.0 / (double)M;
  for (int ci = lane; ci < Ci; ci += 64) wsh[wv][ci] = (double)bf2f(w[(long)cor * ldw + ci]);
  for (int ci = threadIdx.x; ci < Ci; ci += 256) sb[ci] = (double)s[ci] * invM;
  double q[4] = {0.0, 0.0, 0.0, 0.0};  // column cj = lane + 64 t of C w_co
  for (int ci0 = 0; ci0 < Ci; ci0 += FST) {
    __syncthreads();  // wsh / sb written; the previous rows of S consumed
    for (int idx = threadIdx.x * 4; idx < FST * Ci; idx += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(S + (long)ci0 * Ci + idx);
      *reinterpret_cast<float4*>(&Ssh[idx / Ci][idx % Ci]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cj = lane + 64 * t;
      if (cj < Ci) {
        const double sj = sb[cj];
        double inner = 0.0;
#pragma unroll 8
        for (int r = 0; r < FST; ++r) inner += wsh[wv][ci0 + r] * ((double)Ssh[r][cj] * invM - sb[ci0 + r] * sj);
        q[t] += inner;
      }
    }
  }
  double mean = 0.0, var = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cj = lane + 64 * t;
    if (cj < Ci) {
      mean += wsh[wv][cj] * sb[cj];
      var += wsh[wv][cj] * q[t];
    }
  }
  mean = wave_sum(mean);
  var = wave_sum(var);
  if (var < 0.0) var = 0.0;
  if (lane == 0 && co < Co) {
    ws[co] = (float)((double)M * mean);
    ws[Co + co] = (float)((double)M * (var + mean * mean));
  }
}

}  // namespace

int gram_colsum(const void* y2, long ld, long M, int Ci, float* S, float* s, int cus, hipStream_t st) {
  if ((Ci != 64 && Ci != 128 && Ci != 256) || M <= 0 || M >= (1L << 30) || ld % 8) return (int)hipErrorInvalidValue;
  // rows per workgroup: at least 8 Ci (the Ci x 64 fp32 atomics of a workgroup stay under a quarter of the bytes
  // it reads) and 1024 (few atomic adds per element: each rounds against the running total), more where that
  // would make over two workgroups per CU; whole tiles
  const int P = Ci / 64, tp = Ci == 64 ? 256 : (Ci == 128 ? 128 : 64);
  long rows = std::max<long>(std::max(1024, 8 * Ci), (M + 2 * cus / P - 1) / std::max(1, 2 * cus / P));
  rows = (rows + tp - 1) / tp * tp;
  const int chunks = (int)((M + rows - 1) / rows);
  const dim3 grid((unsigned)(chunks * P));
  const bf16_t* y = (const bf16_t*)y2;
  switch (Ci) {
    case 64: hipLaunchKernelGGL(gram_colsum_kernel<64>, grid, dim3(256), 0, st, y, ld, (int)M, (int)rows, S, s); break;
    case 128: hipLaunchKernelGGL(gram_colsum_kernel<128>, grid, dim3(256), 0, st, y, ld, (int)M, (int)rows, S, s); break;
    default: hipLaunchKernelGGL(gram_colsum_kernel<256>, grid, dim3(256), 0, st, y, ld, (int)M, (int)rows, S, s); break;
  }
  return (int)hipGetLastError();
}

int bn_fold_fwd_stats(const void* w, long ldw, const float* S, const float* s, long M, float* ws, int Co, int Ci,
                      hipStream_t st) {
  if (Ci % FST || Ci > 256 || Ci % 4 || Co <= 0 || M <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_fold_fwd_stats_kernel, dim3((Co + 3) / 4), dim3(256), 0, st, (const bf16_t*)w, ldw, S, s, M, ws,
                     Co, Ci);
  return (int)hipGetLastError();
}

int bn_fold_sums(const void* w, long ldw, const float* P, const float* wsg, const float* mean, const float* wsy,
                 int rows, float* sums, float* s, int Co, int Ci, hipStream_t st) {
  const int cb = (Co + 3) / 4;
  // rows == 0: s is already complete (gram_colsum formed it in the forward), only the per-channel blocks run
  const int sblocks = rows > 0 ? kSumSplit * ((Ci + 63) / 64) : 0;
  hipLaunchKernelGGL(bn_fold_sums_kernel, dim3(cb + sblocks), dim3(256), 0, st, (const bf16_t*)w, ldw, P, wsg,
                     mean, wsy, rows, sums, s, Co, Ci, cb);
  return (int)hipGetLastError();
}

int bn_fold_coef(const void* w, long ldw, const float* P, const float* S, const float* s, const float* coef, void* WA,
                 void* WAt, void* Gm, float* kv, float* dW, long lddw, int Co, int Ci, hipStream_t st) {
  if (Co % BKG || Ci % BKW) return (int)hipErrorInvalidValue;
  const int tc = Ci / FT;
  const int blocks = tc * tc + (Co / FT) * tc;
  hipLaunchKernelGGL(bn_fold_coef_kernel, dim3(blocks), dim3(256), 0, st, (const bf16_t*)w, ldw, P, S, s, coef,
                     (bf16_t*)WA, (bf16_t*)WAt, (bf16_t*)Gm, kv, dW, lddw, Co, Ci);
  return (int)hipGetLastError();
}

namespace {

// kv from the ROUNDED matrices the two data-gradient GEMMs read.  The BN's dx has zero column sums, so
// sum_p d y2 = (sum_p g) WA + s Gm + M kv = 0 fixes kv; evaluated with the bf16 WA and Gm it cancels their rounding,
// which otherwise leaves sum_p d y2 off by (sum_p g) dWA + s dGm — a per-channel offset that grows with M.  A BN
// behind d y2 removes it again (conv3 of a bottleneck: bn2's backward); where d y2 IS the block-input gradient
// (the projection shortcut) it would reach the parameters below.  64 columns per block, the Co + Ci rows split over
// the block's 16 waves (a column's Co + Ci loads are latency-bound in one thread), double sums.
constexpr int KVW = 16;
__global__ __launch_bounds__(64 * KVW) void bn_fold_kv_kernel(const bf16_t* __restrict__ WA, const bf16_t* __restrict__ Gm,
                                                               const float* __restrict__ sg, const float* __restrict__ s,
                                                               double inv_m, float* __restrict__ kv, int Co, int Ci) {
  __shared__ double red[KVW][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int ci = blockIdx.x * 64 + tx;
  double a = 0.0;
  if (ci < Ci) {
#pragma unroll 4
    for (int co = ty; co < Co; co += KVW) a += (double)sg[co] * (double)bf2f(WA[(long)co * Ci + ci]);
#pragma unroll 4
    for (int cj = ty; cj < Ci; cj += KVW) a += (double)s[cj] * (double)bf2f(Gm[(long)cj * Ci + ci]);
  }
  red[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && ci < Ci) {
#pragma unroll
    for (int j = 1; j < KVW; ++j) a += red[j][tx];
    kv[ci] = (float)(-a * inv_m);
  }
}

}  // namespace

int bn_fold_kv(const void* WA, const void* Gm, const float* sg, const float* s, long M, float* kv, int Co, int Ci,
               hipStream_t st) {
  if (Co <= 0 || Ci <= 0 || M <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_fold_kv_kernel, dim3((Ci + 63) / 64), dim3(64 * KVW), 0, st, (const bf16_t*)WA, (const bf16_t*)Gm, sg,
                     s, 1.0 / (double)M, kv, Co, Ci);
  return (int)hipGetLastError();
}

}  // namespace ddl
