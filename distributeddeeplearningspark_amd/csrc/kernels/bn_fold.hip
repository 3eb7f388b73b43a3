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

}  // namespace

int bn_fold_sums(const void* w, long ldw, const float* P, const float* wsg, const float* mean, const float* wsy,
                 int rows, float* sums, float* s, int Co, int Ci, hipStream_t st) {
  const int cb = (Co + 3) / 4;
  hipLaunchKernelGGL(bn_fold_sums_kernel, dim3(cb + kSumSplit * ((Ci + 63) / 64)), dim3(256), 0, st, (const bf16_t*)w, ldw, P, wsg,
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

}  // namespace ddl
