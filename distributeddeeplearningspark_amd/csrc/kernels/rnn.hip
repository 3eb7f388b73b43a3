// Persistent recurrent kernels (Keras-2 GRU reset_after=False, LSTM and SimpleRNN), fp32 like the
// reference's Keras models (GRU(128) / LSTM(128) over 25 steps).  The generic
// kernels take the activation / recurrent activation as ActCodes (ddl_act.h); the
// register-resident fast path below serves the Keras defaults (tanh + hard_sigmoid).
//
// The input projection x W + b of ALL time steps is one GEMM done before the kernel; the
// kernel then owns BB batch rows for the whole sequence: h (and c) stay in LDS across the
// T steps, every step reads U (fp32, L2/L1-resident) column-per-thread (coalesced) and the
// hidden state as an LDS broadcast.  Post-activation gates, the hidden / cell sequences
// are saved for the backward.
// Backward (BPTT) runs the same persistent structure in reverse time, propagating dh (and dc)
// with U^T columns per thread; it emits the pre-activation gate gradients of every step so
// that dW, dU, db and dx are plain GEMMs / reductions afterwards.
//
// Directed instantiations (DIR = true; go_backwards / Bidirectional, RnnDir in ddl_ops.h): the workgroup takes its
// direction from blockIdx.y, picks that direction's pointers out of the table and maps processing step s to memory
// time index t = rev ? T-1-s : s.  Saved tensors stay in memory time order; a reverse direction keeps the state
// after step t in slot t (slot T = zero state), so the previous state is slot t + rev and the next one t + 1 - rev.
// With DIR = false every direction value below is a compile-time constant and the code is the forward-only one.
//
// Masked instantiations (MASK = true, directed only; Keras Masking / Embedding(mask_zero)): RnnDir::mask is a uint8
// [B][T] array in memory time order, read at t = time(s) and shared by the directions.  A masked step carries h (and
// c) over in the element-wise state update and writes the carried state to the "next" slots and to y; backward it
// emits zero gate gradients and hands dh (dc) on unchanged.  Contractions and barriers are those of MASK = false,
// and with MASK = false no mask code is generated.
//
// Dropout instantiations (DROP = true, directed only, never with REP or the fused input projection; Keras
// recurrent_dropout, implementation = 1): RnnDir::rdp[d] holds the direction's fp32 multipliers [G][B][H], constant over
// the steps.  Gate g contracts h * rdp[g] (the GRU candidate r * h * rdp[2]); the element-wise updates keep the unmasked
// h.  The generic kernels stage the workgroup's rows of the masks in LDS once (forward) or apply them per gate to the
// U^T contractions (backward).  The register-resident kernels run one batch row per workgroup and fold the row's mask
// into the U registers as they are loaded, (h * m) U = h (diag(m) U): step loop, barriers and prefetch are untouched.
// Input dropout never reaches these kernels (masked projection up front: rnn_drop_x / rnn_drop_dx below); the
// parameter-gradient kernel has a DROP variant tiled per gate.  With DROP = false no dropout code is generated.
#include <type_traits>

#include "ddl_act.h"

namespace ddl {
namespace {

constexpr int BB = 4;  // batch rows per workgroup

struct NoDir {};
template <bool DIR>
using DirArg = std::conditional_t<DIR, RnnDir, NoDir>;      // trailing argument of the generic kernels
template <bool DIR>
using RegArg = std::conditional_t<DIR, RnnDir, RnnRep>;     // ... of the register-resident kernels

// Direction state of a workgroup and the index expressions that depend on it.  row = batch row, s = processing
// step, t = time(s) its memory time index.  With DIR = false they are literally the forward-only expressions.
template <bool DIR>
struct DirOf {
  int rev = 0, yoff = 0, ldy = 0, yproc = 0;
  float dscale = 1.f;
  __device__ __forceinline__ void load(const DirArg<DIR>& a, int d) {
    if constexpr (DIR) {
      rev = a.rev[d]; yoff = a.yoff[d]; ldy = a.ldy; yproc = a.yproc[d]; dscale = a.dscale;
    }
  }
  __device__ __forceinline__ int time(int s, int T) const {
    if constexpr (DIR) return rev ? T - 1 - s : s;
    else return s;
  }
  // slot of hs / cs [row][T+1] holding the zero state, the state before step t and the state after it
  __device__ __forceinline__ long zero_slot(long row, int T) const {
    if constexpr (DIR) return row * (T + 1) + (rev ? T : 0);
    else return row * (T + 1);
  }
  __device__ __forceinline__ long prev_slot(long row, int T, int t) const {
    if constexpr (DIR) return row * (T + 1) + t + rev;
    else return row * (T + 1) + t;
  }
  __device__ __forceinline__ long next_slot(long row, int T, int t) const {
    if constexpr (DIR) return row * (T + 1) + t + 1 - rev;
    else return row * (T + 1) + t + 1;
  }
  // element col of a y / dy sequence row (H wide when undirected) and of a last-state row
  __device__ __forceinline__ long yseq(long row, int T, int s, int t, int H, int col) const {
    if constexpr (DIR) return (row * T + (yproc ? s : t)) * ldy + yoff + col;
    else return (row * T + t) * H + col;
  }
  __device__ __forceinline__ long ylast(long row, int H, int col) const {
    if constexpr (DIR) return row * ldy + yoff + col;
    else return row * H + col;
  }
  __device__ __forceinline__ float dyv(float v) const {
    if constexpr (DIR) return dscale * v;
    else return v;
  }
};

__device__ __forceinline__ float hsig(float x) { return fminf(fmaxf(0.2f * x + 0.5f, 0.f), 1.f); }
__device__ __forceinline__ float hsig_d(float y) { return (y > 0.f && y < 1.f) ? 0.2f : 0.f; }

// ----------------------------------------------------------------------------- forward
template <int CELL, bool DIR = false, bool MASK = false, bool DROP = false>  // 0 = GRU (gates z, r, h), 1 = LSTM (gates i, f, c, o), 2 = SimpleRNN (h)
__global__ __launch_bounds__(512) void rnn_fwd_kernel(const float* __restrict__ xw, const float* __restrict__ U,
                                                      float* __restrict__ hs, float* __restrict__ cs,
                                                      float* __restrict__ gates, float* __restrict__ y, int B, int T,
                                                      int H, int rs, int act, int ract, const DirArg<DIR> dr) {
  static_assert(DIR || !MASK, "masked recurrences run as directed launches");
  static_assert(DIR || !DROP, "recurrences with dropout masks run as directed launches");
  constexpr int G = CELL == 0 ? 3 : (CELL == 1 ? 4 : 1);
  extern __shared__ float sm[];
  const int GH = G * H;
  DirOf<DIR> dz;
  if constexpr (DIR) {
    const int d = blockIdx.y;
    xw = dr.xw[d]; U = dr.U[d]; hs = dr.hs[d]; cs = dr.cs[d]; gates = dr.gates[d]; y = dr.y[d];
    dz.load(dr, d);
  }
  float* h = sm;              // [BB][H]
  float* c = h + BB * H;      // [BB][H]   (LSTM) / r*h (GRU)
  float* gb = c + BB * H;     // [BB][GH]  gate values of the current step
  float* rd = gb + BB * GH;   // [G][BB][H] recurrent dropout multipliers of the workgroup's rows (DROP only)
  const int b0 = blockIdx.x * BB;
  const int nb = min(BB, B - b0);
  if constexpr (DROP) {
    const float* rdp = dr.rdp[blockIdx.y];
    for (int i = threadIdx.x; i < G * BB * H; i += blockDim.x) {
      const int g = i / (BB * H), q = i - g * BB * H, r = q / H, k = q - r * H;
      rd[i] = r < nb ? rdp[((long)g * B + b0 + r) * H + k] : 0.f;
    }
  }
  for (int i = threadIdx.x; i < BB * H; i += blockDim.x) h[i] = c[i] = 0.f;
  for (int i = threadIdx.x; i < nb * H; i += blockDim.x) {
    const int r = i / H, k = i - r * H;
    hs[dz.zero_slot((long)(b0 + r), T) * H + k] = 0.f;
    if (CELL == 1) cs[dz.zero_slot((long)(b0 + r), T) * H + k] = 0.f;
  }
  __syncthreads();
  for (int s = 0; s < T; ++s) {
    const int t = dz.time(s, T);  // memory time index of processing step s
    // gate pre-activations x W + h U (GRU: only z, r here; the candidate needs r * h first)
    const int jend = CELL == 0 ? 2 * H : GH;
    for (int j = threadIdx.x; j < jend; j += blockDim.x) {
      float acc[BB];
#pragma unroll
      for (int r = 0; r < BB; ++r) acc[r] = r < nb ? xw[((long)(b0 + r) * T + t) * GH + j] : 0.f;
      if constexpr (DROP) {
        const float* rg = rd + (j / H) * BB * H;  // the masks of column j's gate
        for (int k = 0; k < H; ++k) {
          const float u = U[(long)k * GH + j];
#pragma unroll
          for (int r = 0; r < BB; ++r) acc[r] += h[r * H + k] * rg[r * H + k] * u;
        }
      } else {
        for (int k = 0; k < H; ++k) {
          const float u = U[(long)k * GH + j];
#pragma unroll
          for (int r = 0; r < BB; ++r) acc[r] += h[r * H + k] * u;
        }
      }
      // LSTM candidate and SimpleRNN use the activation, every other gate the recurrent one
      const bool main_act = CELL == 2 || (CELL == 1 && j >= 2 * H && j < 3 * H);
#pragma unroll
      for (int r = 0; r < BB; ++r) gb[r * GH + j] = act_f(main_act ? act : ract, acc[r]);
    }
    __syncthreads();
    if (CELL == 0) {
      for (int i = threadIdx.x; i < BB * H; i += blockDim.x) {
        const int r = i / H, k = i - r * H;
        c[i] = gb[r * GH + H + k] * h[i];  // r * h
        if constexpr (DROP) c[i] *= rd[2 * BB * H + i];  // read only by the candidate's contraction
      }
      __syncthreads();
      for (int j = 2 * H + threadIdx.x; j < GH; j += blockDim.x) {
        float acc[BB];
#pragma unroll
        for (int r = 0; r < BB; ++r) acc[r] = r < nb ? xw[((long)(b0 + r) * T + t) * GH + j] : 0.f;
        for (int k = 0; k < H; ++k) {
          const float u = U[(long)k * GH + j];
#pragma unroll
          for (int r = 0; r < BB; ++r) acc[r] += c[r * H + k] * u;
        }
#pragma unroll
        for (int r = 0; r < BB; ++r) gb[r * GH + j] = act_f(act, acc[r]);
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < nb * H; i += blockDim.x) {
      const int r = i / H, k = i - r * H;
      const float* g = gb + r * GH;
      // A masked step carries the state over.  The mask selects the gate values (z = 1; i = 0, f = 1), not the
      // result, so the arithmetic is the unmasked kernel's: 1 * h + 0 * hh is h exactly.
      bool data = true;
      if constexpr (MASK) data = dr.mask[(long)(b0 + r) * T + t] != 0;
      float hn;
      if (CELL == 2) {
        hn = data ? g[k] : h[i];
      } else if (CELL == 0) {
        const float z = data ? g[k] : 1.f, hh = g[2 * H + k];
        hn = z * h[i] + (1.f - z) * hh;
      } else {
        const float cn = (data ? g[H + k] : 1.f) * c[i] + (data ? g[k] : 0.f) * g[2 * H + k];
        c[i] = cn;
        hn = data ? g[3 * H + k] * act_f(act, cn) : h[i];
        cs[dz.next_slot((long)(b0 + r), T, t) * H + k] = cn;
      }
      h[i] = hn;
      hs[dz.next_slot((long)(b0 + r), T, t) * H + k] = hn;
      if (rs) y[dz.yseq((long)(b0 + r), T, s, t, H, k)] = hn;
      else if (s == T - 1) y[dz.ylast((long)(b0 + r), H, k)] = hn;
    }
    for (int i = threadIdx.x; i < nb * GH; i += blockDim.x) {
      const int r = i / GH, j = i - r * GH;
      gates[((long)(b0 + r) * T + t) * GH + j] = gb[r * GH + j];
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------- backward
// UT = U^T [GH][H]; dgates [B][T][GH] = d(pre-activation)
template <int CELL, bool DIR = false, bool MASK = false, bool DROP = false>
__global__ __launch_bounds__(512) void rnn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ UT,
                                                      const float* __restrict__ hs, const float* __restrict__ cs,
                                                      const float* __restrict__ gates, float* __restrict__ dgates,
                                                      int B, int T, int H, int rs, int act, int ract,
                                                      const DirArg<DIR> dr) {
  static_assert(DIR || !MASK, "masked recurrences run as directed launches");
  static_assert(DIR || !DROP, "recurrences with dropout masks run as directed launches");
  constexpr int G = CELL == 0 ? 3 : (CELL == 1 ? 4 : 1);
  extern __shared__ float sm[];
  const int GH = G * H;
  DirOf<DIR> dz;
  const float* rdp = nullptr;  // [G][B][H] (DROP only)
  if constexpr (DROP) rdp = dr.rdp[blockIdx.y];
  if constexpr (DIR) {
    const int d = blockIdx.y;
    dy = dr.dy[d]; UT = dr.UT[d]; hs = dr.hs[d]; cs = dr.cs[d]; gates = dr.gates[d]; dgates = dr.dgates[d];
    dz.load(dr, d);
  }
  float* dh = sm;            // [BB][H] running dh (into h_t)
  float* aux = dh + BB * H;  // [BB][H] GRU: dh*z direct part; LSTM: running dc
  float* dp = aux + BB * H;  // [BB][GH] pre-activation gradients of the step
  const int b0 = blockIdx.x * BB;
  const int nb = min(BB, B - b0);
  for (int i = threadIdx.x; i < BB * H; i += blockDim.x) dh[i] = aux[i] = 0.f;
  for (int i = threadIdx.x; i < BB * GH; i += blockDim.x) dp[i] = 0.f;
  __syncthreads();
  for (int s = T - 1; s >= 0; --s) {
    const int t = dz.time(s, T);  // memory time index of processing step s
    for (int i = threadIdx.x; i < nb * H; i += blockDim.x) {
      const int r = i / H, k = i - r * H;
      const long row = (long)(b0 + r);
      float d = dh[i];
      if (rs) d += dz.dyv(dy[dz.yseq(row, T, s, t, H, k)]);
      else if (s == T - 1) d += dz.dyv(dy[dz.ylast(row, H, k)]);
      const float* g = gates + (row * T + t) * GH;
      const float hp = hs[dz.prev_slot(row, T, t) * H + k];
      float* p = dp + r * GH;
      if constexpr (MASK) {
        if (!dr.mask[row * T + t]) {  // masked step: zero gate gradients, dh (and dc, in aux) pass through
          for (int q = 0; q < G; ++q) p[q * H + k] = 0.f;
          dh[i] = d;  // this thread's own element: read again only by itself, in the last phase
          if (CELL == 0) aux[i] = 0.f;
          continue;
        }
      }
      if (CELL == 2) {
        p[k] = d * act_d(act, g[k]);
      } else if (CELL == 0) {
        const float z = g[k], hh = g[2 * H + k];
        p[k] = d * (hp - hh) * act_d(ract, z);
        p[2 * H + k] = d * (1.f - z) * act_d(act, hh);
        aux[i] = d * z;
      } else {
        const float gi = g[k], gf = g[H + k], gg = g[2 * H + k], go = g[3 * H + k];
        const float cn = cs[dz.next_slot(row, T, t) * H + k], cp = cs[dz.prev_slot(row, T, t) * H + k];
        const float tc = act_f(act, cn);
        const float dc = aux[i] + d * go * act_d(act, tc);
        p[k] = dc * gg * act_d(ract, gi);
        p[H + k] = dc * cp * act_d(ract, gf);
        p[2 * H + k] = dc * gi * act_d(act, gg);
        p[3 * H + k] = d * tc * act_d(ract, go);
        aux[i] = dc * gf;
      }
    }
    __syncthreads();
    if (CELL == 0) {  // d(r*h) = dp_h Uh^T -> dr, and the r-path contribution to dh_{t-1}
      for (int i = threadIdx.x; i < nb * H; i += blockDim.x) {
        const int r = i / H, k = i - r * H;
        const long row = (long)(b0 + r);
        const float* p = dp + r * GH;
        float drh = 0.f;
        for (int j = 0; j < H; ++j) drh += p[2 * H + j] * UT[(long)(2 * H + j) * H + k];
        if constexpr (DROP) drh *= rdp[((long)2 * B + row) * H + k];  // d(r*h) through (r * h * rdp[2]) Uh
        const float hp = hs[dz.prev_slot(row, T, t) * H + k];
        const float rg = gates[(row * T + t) * GH + H + k];
        if constexpr (MASK) {
          if (!dr.mask[row * T + t]) continue;  // dr stays the zero written above
        }
        dp[r * GH + H + k] = drh * hp * act_d(ract, rg);
        aux[i] += drh * rg;
      }
      __syncthreads();
    }
    // dh_{t-1} = direct + dp[:, gates feeding from h] U^T
    const int jend = CELL == 0 ? 2 * H : GH;
    for (int i = threadIdx.x; i < nb * H; i += blockDim.x) {
      const int r = i / H, k = i - r * H;
      const float* p = dp + r * GH;
      float s = CELL == 0 ? aux[i] : 0.f;
      if constexpr (MASK) {
        if (!dr.mask[(long)(b0 + r) * T + t]) s = dh[i];  // the carried dh; every p[j] of the row is zero
      }
      if constexpr (DROP) {  // gate g's contraction read h * rdp[g]
        for (int g = 0; g * H < jend; ++g) {
          float sg = 0.f;
          for (int j = g * H; j < (g + 1) * H; ++j) sg += p[j] * UT[(long)j * H + k];
          s += sg * rdp[((long)g * B + b0 + r) * H + k];
        }
      } else {
        for (int j = 0; j < jend; ++j) s += p[j] * UT[(long)j * H + k];
      }
      dh[i] = s;
    }
    for (int i = threadIdx.x; i < nb * GH; i += blockDim.x) {
      const int r = i / GH, j = i - r * GH;
      dgates[((long)(b0 + r) * T + t) * GH + j] = dp[r * GH + j];
    }
    __syncthreads();
  }
}


// =============================================================================================
// Register-resident fast path (H = 64 / 128, the reference's GRU(128) / LSTM(128)).
//
// The generic kernels above stream U from L2 on every step (latency-bound: ~3 ms per GRU step
// at B=32).  Here each workgroup pins the WHOLE recurrent matrix in VGPRs for the sequence:
//  forward : thread (j, kh) holds U[kh*64 .. kh*64+63][j]  (KS = H/64 lane-adjacent k-splits,
//            reduced with one xor-shuffle), so NT = G*H*KS threads (768 GRU / 1024 LSTM);
//  backward: thread (k, js) holds U[k][js*64 .. js*64+63]  (row chunk, contiguous loads),
//            JSP = pow2(G*H/64) lane-adjacent chunks reduced with xor-shuffles.
// h / (r*h) / gate-gradient rows live in LDS with 64-float chunks padded to 68 floats, so the
// lanes of a wave that read different chunks hit different banks.
// Every per-step global input is prefetched one step ahead into registers (its latency hides
// behind the current step's contractions); the input projection x W + b is computed in-kernel
// for narrow inputs (I <= 8: the reference's 25x1 load series), so a step is a pure chain of
// LDS contractions and barriers.  Element-wise phases map one (row, unit) element per thread.
// =============================================================================================
constexpr int CH = 64;       // k / j chunk held in registers
constexpr int CP = CH + 4;   // padded LDS chunk stride (floats)
constexpr int IMAX = 8;      // widest input fused into the kernels
constexpr int RNN_BB_FWD = 1, RNN_BB_BWD = 1;  // default rows per workgroup (H = 128), measured

__device__ __forceinline__ int cpos(int col) { return (col / CH) * CP + (col % CH); }

// lane ^ 1 / lane ^ 2 / ... partner value by DPP (VALU) instead of ds_bpermute (an LDS round trip
// on the recurrence's critical path): quad_perm within 4 lanes, row_ror / row_mirror patterns beyond
template <int O>
__device__ __forceinline__ float xor_lane(float v) {
  const int iv = __builtin_bit_cast(int, v);
  if constexpr (O == 1) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(iv, 0xB1, 0xf, 0xf, false));
  else if constexpr (O == 2) return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(iv, 0x4E, 0xf, 0xf, false));
  else return __shfl_xor(v, O, 64);
}
// partner-quad value inside each 8-lane group (row_half_mirror): lane i reads lane 7 - i, i.e. a lane
// of the OTHER quad — equal to lane ^ 4 whenever the values are uniform within quads, as they are
// after the xor 1 / xor 2 steps of a sum reduction
__device__ __forceinline__ float other_quad(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));
}

// The waitcnt pass treats the values loaded before a loop as possibly still in flight inside it and
// then waits, in every iteration, for whatever vector loads are outstanding at their first use (the
// next step's prefetch).  One real s_waitcnt vmcnt(0) before the loop (a builtin the pass models,
// unlike an asm string) retires them once.  gfx9 encoding: vmcnt 0, expcnt 7, lgkmcnt 15.
__device__ __forceinline__ void retire_vm_loads() { __builtin_amdgcn_s_waitcnt(0x0F70); }

template <int CELL, int H>
constexpr int fwd_threads() { return (CELL == 0 ? 3 : 4) * H * (H / 64); }
template <int CELL, int H>
constexpr int bwd_threads() { return H * (((CELL == 0 ? 3 : 4) * H / 64) <= 4 ? 4 : 8); }

// REP: replica-batched (RnnRep): the workgroup's replica is b0 / rp.B; W / U / bias come from its table
// entries and x from its resident shard at mini-batch (*rp.ctr % rp.nbr[r]) — outputs stay global-row indexed.
// DIR: directed (RnnDir): blockIdx.y is the direction; xw / W / bias / U / hs / cs / gates / y come from its table entry.
// MASK: masked steps (RnnDir::mask) carry the state over; the byte of the element this thread owns in the state
// update is prefetched with the step's inputs.
// DROP: recurrent dropout (RnnDir::rdp) at one batch row per workgroup: the row's multipliers of column j's gate scale
// the thread's U slice once, in the prologue.
template <int CELL, int H, int BB_, bool FUSE, bool REP = false, bool DIR = false, bool MASK = false, bool DROP = false>
__global__ __launch_bounds__((fwd_threads<CELL, H>())) void rnn_fwd_reg_kernel(
    const float* __restrict__ xw, const float* __restrict__ x, const float* __restrict__ W,
    const float* __restrict__ bias, int I, const float* __restrict__ U, float* __restrict__ hs,
    float* __restrict__ cs, float* __restrict__ gates, float* __restrict__ y, int B, int T, int rs,
    const RegArg<DIR> rp) {
  static_assert(!(REP && DIR), "replica batching is forward-only");
  static_assert(DIR || !MASK, "masked recurrences run as directed launches");
  static_assert(!DROP || (DIR && !FUSE && BB_ == 1), "dropout: directed, projection precomputed, one row per workgroup");
  constexpr int G = CELL == 0 ? 3 : 4;
  constexpr int GH = G * H;
  constexpr int KS = H / CH;
  constexpr int HC = KS * CP;  // padded row length of h / c
  constexpr int NT = fwd_threads<CELL, H>();  // == blockDim.x (the launcher's block size)
  __shared__ __attribute__((aligned(16))) float h[BB_][HC];
  __shared__ __attribute__((aligned(16))) float c[BB_][HC];  // LSTM cell state / GRU r*h
  __shared__ float gb[BB_][GH];
  const int tid = threadIdx.x;
  const int j = tid / KS, kh = tid % KS;
  const int b0 = blockIdx.x * BB_;
  const int nb = min(BB_, B - b0);
  long xrow0 = b0;  // input row of the workgroup's first batch row
  if constexpr (REP) {
    const int r = b0 / rp.B;
    U = rp.U[r];
    W = rp.W[r];
    bias = rp.b[r];
    x = rp.x[r];
    xrow0 = (long)(*rp.ctr % rp.nbr[r]) * rp.B + (b0 - r * rp.B);
  }
  DirOf<DIR> dz;
  if constexpr (DIR) {
    const int d = blockIdx.y;
    xw = rp.xw[d]; W = rp.W[d]; bias = rp.b[d]; U = rp.U[d];
    hs = rp.hs[d]; cs = rp.cs[d]; gates = rp.gates[d]; y = rp.y[d];
    dz.load(rp, d);
  }
  float u[CH];
  if constexpr (DROP) {  // (h * m) U = h (diag(m) U): b0 is the workgroup's only row, j / H its gate
    // Sixteen U elements and their multipliers per round trip: the 64 strided U loads at once already fill the
    // register budget with their addresses (LSTM(128): 1024 threads, 128 VGPRs) and would spill beside the mask's.
    const float* m = rp.rdp[blockIdx.y] + ((long)(j / H) * B + b0) * H + kh * CH;
#pragma unroll
    for (int i0 = 0; i0 < CH; i0 += 16) {
      float mv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        u[i0 + i] = U[(long)(kh * CH + i0 + i) * GH + j];
        mv[i] = m[i0 + i];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        u[i0 + i] *= mv[i];
        asm volatile("" : "+v"(u[i0 + i]));  // the product exists here: U element and multiplier are not both kept
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) u[i] = U[(long)(kh * CH + i) * GH + j];
  }
  float wv[IMAX], bv = 0.f;  // input-projection column j (fused path); wv[i] = 0 past the input width
#pragma unroll
  for (int i = 0; i < IMAX; ++i) wv[i] = (FUSE && i < I) ? W[(long)i * GH + j] : 0.f;
  if (FUSE && bias) bv = bias[j];
  // Step t's inputs are fetched one step ahead and contracted only when used, so their latency hides
  // behind a whole step.  The x row address is workgroup-uniform: an opaque zero offset keeps the loads
  // on the vector path (a scalar load is counted by lgkmcnt, which every LDS barrier drains), and the
  // loads are unconditional at clamped indices (a runtime-guarded load per element makes the compiler
  // branch and wait per element); padded inputs meet wv = 0.
  int zoff;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zoff));
  auto fetch_x = [&](int s, float (&xr)[BB_][IMAX]) {
    const int tc = min(max(dz.time(s, T), 0), T - 1);  // processing step -> memory time index first, then the clamp
#pragma unroll
    for (int r = 0; r < BB_; ++r) {
      const long bt = (xrow0 + min(r, nb - 1)) * T + tc;
      if constexpr (!FUSE) {
        xr[r][0] = xw[bt * GH + j];
      } else {
#pragma unroll
        for (int i = 0; i < IMAX; ++i) xr[r][i] = x[bt * I + min(i, I - 1) + zoff];
      }
    }
  };
  auto proj = [&](const float (&xr)[BB_][IMAX], float* xv) {
#pragma unroll
    for (int r = 0; r < BB_; ++r) {
      if constexpr (!FUSE) {
        xv[r] = xr[r][0];
      } else {
        float a = bv;
#pragma unroll
        for (int i = 0; i < IMAX; ++i) a += xr[r][i] * wv[i];
        xv[r] = a;
      }
    }
  };
  for (int i = tid; i < BB_ * HC; i += NT) (&h[0][0])[i] = (&c[0][0])[i] = 0.f;
  // element owned in the state-update phase
  const int er = tid / H, ek = tid - er * H;
  const bool eown = er < nb;
  const long erow = b0 + er;
  if (eown) {
    hs[dz.zero_slot(erow, T) * H + ek] = 0.f;
    if (CELL == 1) cs[dz.zero_slot(erow, T) * H + ek] = 0.f;
  }
  // mask byte of this thread's state element at step s: clamped and unconditional like fetch_x, and issued before
  // the step's x loads, so the wait for those covers it
  const long mrow = (b0 + min(er, nb - 1)) * (long)T;
  auto fetch_m = [&](int s) -> unsigned {
    if constexpr (MASK) return rp.mask[mrow + min(max(dz.time(s, T), 0), T - 1) + zoff];
    else return 1u;
  };
  unsigned mcur = fetch_m(0);
  float xr[BB_][IMAX], xv[BB_];
  fetch_x(0, xr);
  proj(xr, xv);
  retire_vm_loads();
  __syncthreads();
  auto contract = [&](float (*src)[HC], float* acc) {
#pragma unroll
    for (int r = 0; r < BB_; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < CH; i += 4) {
#pragma unroll
      for (int r = 0; r < BB_; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(&src[r][kh * CP + i]);
        acc[r] += v.x * u[i] + v.y * u[i + 1] + v.z * u[i + 2] + v.w * u[i + 3];
      }
    }
    if (KS == 2) {
#pragma unroll
      for (int r = 0; r < BB_; ++r) acc[r] += xor_lane<1>(acc[r]);
    }
  };
  for (int s = 0; s < T; ++s) {
    const int t = dz.time(s, T);  // memory time index of processing step s
    const unsigned mnext = fetch_m(s + 1);
    fetch_x(s + 1, xr);  // the next step's inputs (consumed at the end of this step)
    float acc[BB_];
    if (CELL == 1 || j < 2 * H) {  // wave-uniform: 2H columns span whole waves
      contract(h, acc);
      if (kh == 0) {
        const bool is_tanh = CELL == 1 && j >= 2 * H && j < 3 * H;
#pragma unroll
        for (int r = 0; r < BB_; ++r) gb[r][j] = is_tanh ? tanhf(acc[r] + xv[r]) : hsig(acc[r] + xv[r]);
      }
    }
    lds_barrier();
    if (CELL == 0) {
      for (int i = tid; i < BB_ * H; i += NT) {
        const int r = i / H, k = i - r * H;
        c[r][cpos(k)] = gb[r][H + k] * h[r][cpos(k)];
      }
      lds_barrier();
      if (j >= 2 * H) {
        contract(c, acc);
        if (kh == 0) {
#pragma unroll
          for (int r = 0; r < BB_; ++r) gb[r][j] = tanhf(acc[r] + xv[r]);
        }
      }
      lds_barrier();
    }
    // next step's projection before this step's stores: its wait then covers the loads issued at the
    // top of the step and the PREVIOUS step's stores (a whole step old), never the stores below
    float xnext[BB_];
    proj(xr, xnext);
#pragma unroll
    for (int r = 0; r < BB_; ++r) asm volatile("" ::"v"(xnext[r]) : "memory");  // computed here, not sunk past the stores
    if constexpr (MASK) asm volatile("" ::"v"(mnext) : "memory");
    if (eown) {
      // A masked step carries the state over.  The mask selects the gate values (z = 1; i = 0, f = 1), not the
      // result, so the arithmetic is the unmasked kernel's: 1 * h + 0 * hh is h exactly.
      const bool data = !MASK || mcur != 0;
      float hn;
      if (CELL == 0) {
        const float z = data ? gb[er][ek] : 1.f, hh = gb[er][2 * H + ek];
        hn = z * h[er][cpos(ek)] + (1.f - z) * hh;
      } else {
        const float cn = (data ? gb[er][H + ek] : 1.f) * c[er][cpos(ek)] +
                         (data ? gb[er][ek] : 0.f) * gb[er][2 * H + ek];
        c[er][cpos(ek)] = cn;
        hn = data ? gb[er][3 * H + ek] * tanhf(cn) : h[er][cpos(ek)];
        cs[dz.next_slot(erow, T, t) * H + ek] = cn;
      }
      h[er][cpos(ek)] = hn;
      hs[dz.next_slot(erow, T, t) * H + ek] = hn;
      if (rs) y[dz.yseq(erow, T, s, t, H, ek)] = hn;
      else if (s == T - 1) y[dz.ylast(erow, H, ek)] = hn;
    }
    for (int i = tid; i < nb * GH; i += NT) {
      const int r = i / GH, jj = i - r * GH;
      gates[((long)(b0 + r) * T + t) * GH + jj] = gb[r][jj];
    }
#pragma unroll
    for (int r = 0; r < BB_; ++r) xv[r] = xnext[r];
    mcur = mnext;
    lds_barrier();
  }
}

// MASK: a masked step (RnnDir::mask, its byte prefetched with the step's saved activations) writes zero gate
// gradients and hands dh on through the direct-part row (GRU: aux, LSTM: the otherwise unused hpl); dc stays in aux.
// DROP: as forward, the row's multipliers fold into the U registers: thread (k, js) scales its chunk, which lies inside
// one gate (H is a multiple of 64), by rdp[gate][row][k].
template <int CELL, int H, int BB_, bool REP = false, bool DIR = false, bool MASK = false, bool DROP = false>
__global__ __launch_bounds__((bwd_threads<CELL, H>())) void rnn_bwd_reg_kernel(
    const float* __restrict__ dy, const float* __restrict__ U, const float* __restrict__ hs,
    const float* __restrict__ cs, const float* __restrict__ gates, float* __restrict__ dgates, int B, int T, int rs,
    const RegArg<DIR> rp) {
  static_assert(!(REP && DIR), "replica batching is forward-only");
  static_assert(DIR || !MASK, "masked recurrences run as directed launches");
  static_assert(!DROP || (DIR && BB_ == 1 && H % CH == 0), "dropout: directed, one row per workgroup");
  constexpr int G = CELL == 0 ? 3 : 4;
  constexpr int GH = G * H;
  constexpr int JS = GH / CH;                            // column chunks
  constexpr int JSP = JS <= 4 ? 4 : 8;                   // lanes per k (power of two)
  constexpr int ZR = CELL == 0 ? 2 * H / CH : JS;        // chunks feeding dh directly
  constexpr int NT = bwd_threads<CELL, H>();            // == blockDim.x
  __shared__ __attribute__((aligned(16))) float p[BB_][JS * CP];  // pre-activation gradients
  __shared__ float dh[BB_][H];
  __shared__ float aux[BB_][H];  // GRU: d*z direct part; LSTM: running dc
  __shared__ float hpl[BB_][H];  // GRU: h_{t-1} and r of the step, staged for the dr phase
  __shared__ float rgl[BB_][H];
  const int tid = threadIdx.x;
  const int k = tid / JSP, js = tid % JSP;
  const bool active = js < JS;
  const int b0 = blockIdx.x * BB_;
  const int nb = min(BB_, B - b0);
  if constexpr (REP) U = rp.U[b0 / rp.B];
  DirOf<DIR> dz;
  if constexpr (DIR) {
    const int d = blockIdx.y;
    dy = rp.dy[d]; U = rp.U[d]; hs = rp.hs[d]; cs = rp.cs[d]; gates = rp.gates[d]; dgates = rp.dgates[d];
    dz.load(rp, d);
  }
  float u[CH];
#pragma unroll
  for (int i = 0; i < CH; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(&U[(long)k * GH + min(js, JS - 1) * CH + i]);  // idle: unused
    u[i] = v.x; u[i + 1] = v.y; u[i + 2] = v.z; u[i + 3] = v.w;
  }
  if constexpr (DROP) {
    const int g = min(js, JS - 1) * CH / H;  // the gate of this thread's column chunk
    const float m = rp.rdp[blockIdx.y][((long)g * B + b0) * H + k];
#pragma unroll
    for (int i = 0; i < CH; ++i) u[i] *= m;
  }
  for (int i = tid; i < BB_ * H; i += NT) (&dh[0][0])[i] = (&aux[0][0])[i] = 0.f;
  if constexpr (MASK && CELL == 1) {  // rows past the batch are never written
    for (int i = tid; i < BB_ * H; i += NT) (&hpl[0][0])[i] = 0.f;
  }
  for (int i = tid; i < BB_ * JS * CP; i += NT) (&p[0][0])[i] = 0.f;
  // element owned in the element-wise phase, and its prefetched inputs
  const int er = tid / H, ek = tid - er * H;
  const bool eown = er < nb;
  const long erow = b0 + er;
  struct In { float d, g0, g1, g2, g3, hp, cn, cp; };
  unsigned mcur = 1, mnxt = 1;  // mask bytes of the current and the prefetched step (MASK only)
  auto load_in = [&](int s, In& v, unsigned& m) {
    if (!eown || s < 0) return;  // the guard is on the processing step; every index below is then in range
    const int t = dz.time(s, T);
    if constexpr (MASK) m = rp.mask[erow * T + t];
    v.d = rs ? dz.dyv(dy[dz.yseq(erow, T, s, t, H, ek)]) : (s == T - 1 ? dz.dyv(dy[dz.ylast(erow, H, ek)]) : 0.f);
    const float* g = gates + (erow * T + t) * GH;
    v.g0 = g[ek]; v.g1 = g[H + ek]; v.g2 = g[2 * H + ek];
    if (CELL == 1) {
      v.g3 = g[3 * H + ek];
      v.cn = cs[dz.next_slot(erow, T, t) * H + ek];
      v.cp = cs[dz.prev_slot(erow, T, t) * H + ek];
    } else {
      v.hp = hs[dz.prev_slot(erow, T, t) * H + ek];
    }
  };
  In cur{}, nxt{};
  load_in(T - 1, cur, mcur);
  retire_vm_loads();
  __syncthreads();
  auto contract = [&](bool use, float* acc) {
#pragma unroll
    for (int r = 0; r < BB_; ++r) acc[r] = 0.f;
    // every lane computes (no divergence inside the unrolled dot); lanes whose chunk is not
    // part of this contraction drop their partial before the shuffle reduction
    const int jc = min(js, JS - 1);
#pragma unroll
    for (int i = 0; i < CH; i += 4) {
#pragma unroll
      for (int r = 0; r < BB_; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(&p[r][jc * CP + i]);
        acc[r] += v.x * u[i] + v.y * u[i + 1] + v.z * u[i + 2] + v.w * u[i + 3];
      }
      if ((i & 15) == 12) __builtin_amdgcn_sched_barrier(0);  // bound the LDS loads in flight
    }
#pragma unroll
    for (int r = 0; r < BB_; ++r) {
      acc[r] = use ? acc[r] : 0.f;
      acc[r] += xor_lane<1>(acc[r]);
      acc[r] += xor_lane<2>(acc[r]);
      if constexpr (JSP == 8) acc[r] += other_quad(acc[r]);
    }
  };
  for (int s = T - 1; s >= 0; --s) {
    const int t = dz.time(s, T);  // memory time index of processing step s
    load_in(s - 1, nxt, mnxt);  // prefetch the previous step's saved activations
    if (eown) {
      const float d = dh[er][ek] + cur.d;
      const bool data = !MASK || mcur != 0;  // a masked step: zero gate gradients, dh (and dc) pass through
      float* pr = p[er];
      if (CELL == 0) {
        const float z = cur.g0, hh = cur.g2;
        pr[cpos(ek)] = data ? d * (cur.hp - hh) * hsig_d(z) : 0.f;
        pr[cpos(2 * H + ek)] = data ? d * (1.f - z) * (1.f - hh * hh) : 0.f;
        aux[er][ek] = data ? d * z : d;
        hpl[er][ek] = cur.hp;
        rgl[er][ek] = cur.g1;
      } else {
        const float gi = cur.g0, gf = cur.g1, gg = cur.g2, go = cur.g3;
        const float tc = tanhf(cur.cn);
        const float dc = aux[er][ek] + d * go * (1.f - tc * tc);
        pr[cpos(ek)] = data ? dc * gg * hsig_d(gi) : 0.f;
        pr[cpos(H + ek)] = data ? dc * cur.cp * hsig_d(gf) : 0.f;
        pr[cpos(2 * H + ek)] = data ? dc * gi * (1.f - gg * gg) : 0.f;
        pr[cpos(3 * H + ek)] = data ? d * tc * hsig_d(go) : 0.f;
        if (data) aux[er][ek] = dc * gf;  // a masked step leaves the running dc as it is
        if constexpr (MASK) hpl[er][ek] = data ? 0.f : d;  // the carried dh, added in phase 1
      }
    }
    lds_barrier();
    // GRU: phase 0 = d(r*h) = dp_h Uh^T -> dr and the r-path part of dh_{t-1}; phase 1 = dh_{t-1}.
    // One call site for the contraction (keeps a single register-resident copy of U).
#pragma unroll 1
    for (int ph = CELL == 0 ? 0 : 1; ph < 2; ++ph) {
      float acc[BB_];
      contract(active && (ph == 0 ? js >= ZR : js < ZR), acc);
      if (js == 0) {
        if (ph == 0) {
#pragma unroll
          for (int r = 0; r < BB_; ++r) {
            const float rg = rgl[r][k];
            p[r][cpos(H + k)] = acc[r] * hpl[r][k] * hsig_d(rg);
            aux[r][k] += acc[r] * rg;
          }
        } else {
#pragma unroll
          for (int r = 0; r < BB_; ++r) dh[r][k] = (CELL == 0 ? aux[r][k] : (MASK ? hpl[r][k] : 0.f)) + acc[r];
        }
      }
      if (ph == 0) lds_barrier();
    }
    for (int i = tid; i < nb * GH; i += NT) {
      const int r = i / GH, jj = i - r * GH;
      dgates[((long)(b0 + r) * T + t) * GH + jj] = p[r][cpos(jj)];
    }
    cur = nxt;
    if constexpr (MASK) mcur = mnxt;
    lds_barrier();
  }
}

// Parameter gradients of a recurrent layer in ONE launch, accumulated (fp32 atomics) straight
// into the gradient arena:  rows m < H      : gU[m][j] += sum_bt A(bt,m,j) dg[bt][j]
//                           rows H <= m < H+I: gW[m-H][j] += sum_bt x[bt][m-H] dg[bt][j]
//                           row m = H+I      : gb[j] += sum_bt dg[bt][j]
// with A = h_{t-1}[m] (GRU candidate columns: r[m] * h_{t-1}[m]).  Tile 64(m) x 64(j) over a
// chunk of PG_BT (b,t) rows staged in LDS; 256 threads x 4x4 outputs.
constexpr int PG_BT = 128;

struct DropMasks {
  const float* dp;   // [G][B][I] input multipliers or null
  const float* rdp;  // [G][B][H] recurrent multipliers or null
};
template <bool DROP>
using DropArg = std::conditional_t<DROP, DropMasks, NoDir>;

// REV: saved tensors of a reverse-direction recurrence, h_{t-1} in slot t + 1
// DROP: the A rows carry gate g's dropout multipliers (h_{t-1} * rdp[g], x * dp[g]), so a j tile stays inside one
// gate: blockIdx.y = gate * ceil(H / 64) + tile of the gate's H columns (any H, GRU included).
template <int CELL, bool REV = false, bool DROP = false>
__global__ __launch_bounds__(256) void rnn_param_grad_kernel(const float* __restrict__ dg, const float* __restrict__ hs,
                                                             const float* __restrict__ gates,
                                                             const float* __restrict__ x, float* __restrict__ gU,
                                                             float* __restrict__ gW, float* __restrict__ gb, int B,
                                                             int T, int H, int I, const DropArg<DROP> dm) {
  constexpr int G = CELL == 0 ? 3 : (CELL == 1 ? 4 : 1);
  const int GH = G * H;
  const int M = H + I + (gb ? 1 : 0);
  const long BT = (long)B * T;
  const int m0 = blockIdx.x * 64;
  int j0 = blockIdx.y * 64, jend = GH, gate = 0;  // columns [j0, min(j0 + 64, jend)) of dg
  if constexpr (DROP) {
    const int tiles = (H + 63) / 64;
    gate = blockIdx.y / tiles;
    j0 = gate * H + (blockIdx.y - gate * tiles) * 64;
    jend = (gate + 1) * H;
  }
  const long bt0 = (long)blockIdx.z * PG_BT;
  const int nbt = (int)min((long)PG_BT, BT - bt0);
  __shared__ float As[PG_BT][64 + 1];
  __shared__ float Ds[PG_BT][64 + 1];
  const bool cand = CELL == 0 && (DROP ? gate == 2 : j0 >= 2 * H);  // not DROP: 2H is a multiple of 64
  // fill: thread owns column c and rows q = q0, q0+4, ...; (b, t) advance incrementally
  // (a runtime-T division per element would dominate the kernel)
  const int c = threadIdx.x & 63, q0 = threadIdx.x >> 6;
  long b = (bt0 + q0) / T, t = (bt0 + q0) - b * T;
  for (int q = q0; q < nbt; q += 4, t += 4) {
    while (t >= T) { t -= T; ++b; }
    const long bt = bt0 + q;
    const int m = m0 + c;
    float a = 0.f;
    if (m < H) {
      a = hs[(b * (T + 1) + t + (REV ? 1 : 0)) * H + m];
      if (cand) a *= gates[bt * GH + H + m];
      if constexpr (DROP) {
        if (dm.rdp) a *= dm.rdp[((long)gate * B + b) * H + m];
      }
    } else if (m < H + I) {
      a = x[bt * I + (m - H)];
      if constexpr (DROP) {
        if (dm.dp) a *= dm.dp[((long)gate * B + b) * I + (m - H)];
      }
    } else if (m < M) {
      a = 1.f;
    }
    As[q][c] = a;
    const int jj = j0 + c;
    Ds[q][c] = jj < jend ? dg[bt * GH + jj] : 0.f;
  }
  __syncthreads();
  const int tm = (threadIdx.x / 16) * 4, tj = (threadIdx.x % 16) * 4;
  float acc[4][4] = {};
  for (int q = 0; q < nbt; ++q) {
    float a[4], d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = As[q][tm + i]; d[i] = Ds[q][tj + i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int l = 0; l < 4; ++l) acc[i][l] += a[i] * d[l];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tm + i;
    if (m >= M) continue;
    float* dst = m < H ? gU + (long)m * GH : (m < H + I ? gW + (long)(m - H) * GH : gb);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int jj = j0 + tj + l;
      if (jj < jend) atomicAdd(dst + jj, acc[i][l]);
    }
  }
}

template <int CELL, int H, int BB_>
int launch_fwd_reg(const float* xw, const float* x, const float* W, const float* b, int I, const float* U, float* hs,
                   float* cs, float* gates, float* y, int B, int T, int rs, hipStream_t s) {
  constexpr int G = CELL == 0 ? 3 : 4;
  static_assert(BB_ * H <= fwd_threads<CELL, H>(), "one state element per thread");
  if (!xw && (I < 1 || I > IMAX)) return (int)hipErrorInvalidValue;
  const dim3 grid((B + BB_ - 1) / BB_);
  const RnnRep none{};
  if (xw)
    hipLaunchKernelGGL((rnn_fwd_reg_kernel<CELL, H, BB_, false>), grid, dim3(G * H * (H / CH)), 0, s, xw, x, W, b, I,
                       U, hs, cs, gates, y, B, T, rs, none);
  else
    hipLaunchKernelGGL((rnn_fwd_reg_kernel<CELL, H, BB_, true>), grid, dim3(G * H * (H / CH)), 0, s, xw, x, W, b, I,
                       U, hs, cs, gates, y, B, T, rs, none);
  return (int)hipGetLastError();
}

template <int CELL, int H, int BB_>
int launch_bwd_reg(const float* dy, const float* U, const float* hs, const float* cs, const float* gates,
                   float* dgates, int B, int T, int rs, hipStream_t s) {
  static_assert(BB_ * H <= bwd_threads<CELL, H>(), "one state element per thread");
  const dim3 grid((B + BB_ - 1) / BB_);
  const RnnRep none{};
  hipLaunchKernelGGL((rnn_bwd_reg_kernel<CELL, H, BB_>), grid, dim3(bwd_threads<CELL, H>()), 0, s, dy, U, hs, cs,
                     gates, dgates, B, T, rs, none);
  return (int)hipGetLastError();
}

// directed launches: grid.y = direction, everything per direction comes from the table (MASK: d.mask is set;
// DROP: d.rdp is set in every direction and the projection d.xw is given)
template <int CELL, int H, int BB_, bool MASK, bool DROP>
int launch_fwd_reg_dir(const RnnDir& d, int ndir, const float* x, int I, int B, int T, int rs, hipStream_t s) {
  const bool fuse = !d.xw[0];
  if (fuse && (DROP || I < 1 || I > IMAX)) return (int)hipErrorInvalidValue;
  const dim3 grid((B + BB_ - 1) / BB_, ndir), block(fwd_threads<CELL, H>());
  const float* const np = nullptr;
  float* const nq = nullptr;
  if constexpr (!DROP) {
    if (fuse) {
      hipLaunchKernelGGL((rnn_fwd_reg_kernel<CELL, H, BB_, true, false, true, MASK>), grid, block, 0, s, np, x, np, np,
                         I, np, nq, nq, nq, nq, B, T, rs, d);
      return (int)hipGetLastError();
    }
  }
  hipLaunchKernelGGL((rnn_fwd_reg_kernel<CELL, H, BB_, false, false, true, MASK, DROP>), grid, block, 0, s, np, x, np,
                     np, I, np, nq, nq, nq, nq, B, T, rs, d);
  return (int)hipGetLastError();
}

template <int CELL, int H, int BB_, bool MASK, bool DROP>
int launch_bwd_reg_dir(const RnnDir& d, int ndir, int B, int T, int rs, hipStream_t s) {
  const dim3 grid((B + BB_ - 1) / BB_, ndir);
  const float* const np = nullptr;
  hipLaunchKernelGGL((rnn_bwd_reg_kernel<CELL, H, BB_, false, true, MASK, DROP>), grid, dim3(bwd_threads<CELL, H>()), 0,
                     s, np, np, np, np, np, (float*)nullptr, B, T, rs, d);
  return (int)hipGetLastError();
}

// dynamic LDS of the generic kernels: h, c / aux and the gate rows of BB batch rows; forward DROP: plus the staged masks.
// Past the 64 KB a launch gets by default the kernel is granted the larger size; 160 KB is the CU's LDS.
constexpr size_t kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;
template <typename K>
int grant_lds(K kernel, size_t lds) {
  if (lds <= kLdsDefault) return 0;
  if (lds > kLdsMax) return (int)hipErrorInvalidValue;
  return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
}

template <int CELL, bool MASK, bool DROP>
int launch_fwd_gen_dir(const RnnDir& d, const dim3 grid, int threads, size_t lds, int B, int T, int H, int rs, int act,
                       int ract, hipStream_t s) {
  const float* const np = nullptr;
  float* const nq = nullptr;
  if constexpr (DROP) {
    if (const int e = grant_lds(rnn_fwd_kernel<CELL, true, MASK, DROP>, lds)) return e;
  }
  hipLaunchKernelGGL((rnn_fwd_kernel<CELL, true, MASK, DROP>), grid, dim3(threads), lds, s, np, np, nq, nq, nq, nq, B, T,
                     H, rs, act, ract, d);
  return (int)hipGetLastError();
}

template <bool MASK, bool DROP>
int launch_fwd_dir(int cell, const RnnDir& d, int ndir, const float* x, int I, int B, int T, int H, int rs, int act,
                   int ract, hipStream_t s) {
  const bool reg = rnn_reg_path(cell, H, act, ract);
  constexpr int BB128 = DROP ? 1 : RNN_BB_FWD, BB64 = DROP ? 1 : 2;  // DROP: one row per workgroup (mask folded into U)
  if (reg && H == 128)
    return cell == 0 ? launch_fwd_reg_dir<0, 128, BB128, MASK, DROP>(d, ndir, x, I, B, T, rs, s)
                     : launch_fwd_reg_dir<1, 128, BB128, MASK, DROP>(d, ndir, x, I, B, T, rs, s);
  if (reg && H == 64)
    return cell == 0 ? launch_fwd_reg_dir<0, 64, BB64, MASK, DROP>(d, ndir, x, I, B, T, rs, s)
                     : launch_fwd_reg_dir<1, 64, BB64, MASK, DROP>(d, ndir, x, I, B, T, rs, s);
  if (!d.xw[0]) return (int)hipErrorInvalidValue;  // generic kernels need the projection precomputed
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  const size_t lds = sizeof(float) * (2 * BB * H + (DROP ? 2 : 1) * BB * G * H);
  const int threads = std::min(512, ((G * H + 63) / 64) * 64);
  const dim3 grid((B + BB - 1) / BB, ndir);
  if (cell == 0) return launch_fwd_gen_dir<0, MASK, DROP>(d, grid, threads, lds, B, T, H, rs, act, ract, s);
  if (cell == 1) return launch_fwd_gen_dir<1, MASK, DROP>(d, grid, threads, lds, B, T, H, rs, act, ract, s);
  return launch_fwd_gen_dir<2, MASK, DROP>(d, grid, threads, lds, B, T, H, rs, act, ract, s);
}

template <bool MASK, bool DROP>
int launch_bwd_dir(int cell, const RnnDir& d, int ndir, int B, int T, int H, int rs, int act, int ract,
                   hipStream_t s) {
  const bool reg = rnn_reg_path(cell, H, act, ract);
  constexpr int BB128 = DROP ? 1 : RNN_BB_BWD, BB64 = DROP ? 1 : 2;
  if (reg && H == 128)
    return cell == 0 ? launch_bwd_reg_dir<0, 128, BB128, MASK, DROP>(d, ndir, B, T, rs, s)
                     : launch_bwd_reg_dir<1, 128, BB128, MASK, DROP>(d, ndir, B, T, rs, s);
  if (reg && H == 64)
    return cell == 0 ? launch_bwd_reg_dir<0, 64, BB64, MASK, DROP>(d, ndir, B, T, rs, s)
                     : launch_bwd_reg_dir<1, 64, BB64, MASK, DROP>(d, ndir, B, T, rs, s);
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  const size_t lds = sizeof(float) * (2 * BB * H + BB * G * H);
  const int threads = std::min(512, ((G * H + 63) / 64) * 64);
  const dim3 grid((B + BB - 1) / BB, ndir);
  const float* const np = nullptr;
  if (cell == 0)
    hipLaunchKernelGGL((rnn_bwd_kernel<0, true, MASK, DROP>), grid, dim3(threads), lds, s, np, np, np, np, np,
                       (float*)nullptr, B, T, H, rs, act, ract, d);
  else if (cell == 1)
    hipLaunchKernelGGL((rnn_bwd_kernel<1, true, MASK, DROP>), grid, dim3(threads), lds, s, np, np, np, np, np,
                       (float*)nullptr, B, T, H, rs, act, ract, d);
  else
    hipLaunchKernelGGL((rnn_bwd_kernel<2, true, MASK, DROP>), grid, dim3(threads), lds, s, np, np, np, np, np,
                       (float*)nullptr, B, T, H, rs, act, ract, d);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void bidir_merge_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          float* __restrict__ out, long n, float scale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = scale * (a[i] + b[i]);
}

// Step masks (Keras Masking / Embedding(mask_zero)).  One wave per (b, t) row of x [rows][F]:
// mask = any_f(x != mask_value); y (nullable) = x * mask.
__global__ __launch_bounds__(256) void mask_from_features_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 unsigned char* __restrict__ mask, long rows, int F,
                                                                 float mask_value) {
  const int lane = threadIdx.x & 63;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {  // wave-uniform
    const float* xr = x + row * F;
    bool any = false;
    for (int f = lane; f < F; f += 64) any |= xr[f] != mask_value;
    const bool data = __any(any);
    if (lane == 0) mask[row] = data ? 1 : 0;
    if (y) {
      for (int f = lane; f < F; f += 64) y[row * F + f] = data ? xr[f] : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void mask_apply_kernel(const float* __restrict__ in,
                                                         const unsigned char* __restrict__ mask,
                                                         float* __restrict__ out, long rows, int F) {
  const long n = rows * F;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = mask[i / F] ? in[i] : 0.f;
}

// Input dropout (Keras dropout on a recurrent layer): xm [G][B T][I] = x [B T][I] * dp [G][B][I], the G masked
// copies the per-gate projection GEMMs read
__global__ __launch_bounds__(256) void rnn_drop_x_kernel(const float* __restrict__ x, const float* __restrict__ dp,
                                                         float* __restrict__ xm, int G, int B, int T, int I) {
  const long per = (long)B * T * I, n = G * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long g = i / per, q = i - g * per, b = q / ((long)T * I);
    xm[i] = x[q] * dp[(g * B + b) * I + q % I];
  }
}

// ... and its gradient: dx [B T][I] (+)= sum_g t [G][B T][I] * dp [G][B][I]
__global__ __launch_bounds__(256) void rnn_drop_dx_kernel(const float* __restrict__ t, const float* __restrict__ dp,
                                                          float* __restrict__ dx, int G, int B, int T, int I,
                                                          int accumulate) {
  const long per = (long)B * T * I;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < per; q += (long)gridDim.x * 256) {
    const long b = q / ((long)T * I);
    const int i = (int)(q % I);
    float a = accumulate ? dx[q] : 0.f;
    for (int g = 0; g < G; ++g) a += t[g * per + q] * dp[((long)g * B + b) * I + i];
    dx[q] = a;
  }
}

__global__ __launch_bounds__(256) void mask_from_ids_kernel(const long* __restrict__ ids,
                                                            unsigned char* __restrict__ mask, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) mask[i] = ids[i] != 0;
}

}  // namespace

bool rnn_fast_path(int H) { return H == 128 || H == 64; }
bool rnn_fuses_input(int H, int I) { return rnn_fast_path(H) && I <= IMAX; }
bool rnn_reg_path(int cell, int H, int act, int ract) {
  return (cell == 0 || cell == 1) && rnn_fast_path(H) && act == ACT_C_TANH && ract == ACT_C_HARD_SIGMOID;
}


int rnn_fwd(int cell, const float* xw, const float* x, const float* W, const float* b, int I, const float* U,
            float* hs, float* cs, float* gates, float* y, int B, int T, int H, int rs, int act, int ract,
            hipStream_t s) {
  const bool reg = rnn_reg_path(cell, H, act, ract);
  if (reg && H == 128)  // one batch row per workgroup: more CUs busy, less VALU per step (latency-bound)
    return cell == 0 ? launch_fwd_reg<0, 128, RNN_BB_FWD>(xw, x, W, b, I, U, hs, cs, gates, y, B, T, rs, s)
                     : launch_fwd_reg<1, 128, RNN_BB_FWD>(xw, x, W, b, I, U, hs, cs, gates, y, B, T, rs, s);
  if (reg && H == 64)
    return cell == 0 ? launch_fwd_reg<0, 64, 2>(xw, x, W, b, I, U, hs, cs, gates, y, B, T, rs, s)
                     : launch_fwd_reg<1, 64, 2>(xw, x, W, b, I, U, hs, cs, gates, y, B, T, rs, s);
  if (!xw) return (int)hipErrorInvalidValue;  // generic kernels need the projection precomputed
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  const size_t lds = sizeof(float) * (2 * BB * H + BB * G * H);
  const int threads = std::min(512, ((G * H + 63) / 64) * 64);
  const dim3 grid((B + BB - 1) / BB);
  if (cell == 0)
    hipLaunchKernelGGL(rnn_fwd_kernel<0>, grid, dim3(threads), lds, s, xw, U, hs, cs, gates, y, B, T, H, rs, act, ract, NoDir{});
  else if (cell == 1)
    hipLaunchKernelGGL(rnn_fwd_kernel<1>, grid, dim3(threads), lds, s, xw, U, hs, cs, gates, y, B, T, H, rs, act, ract, NoDir{});
  else
    hipLaunchKernelGGL(rnn_fwd_kernel<2>, grid, dim3(threads), lds, s, xw, U, hs, cs, gates, y, B, T, H, rs, act, ract, NoDir{});
  return (int)hipGetLastError();
}

bool rnn_bwd_uses_ut(int H) { return !rnn_fast_path(H); }

int rnn_param_grad(int cell, const float* dg, const float* hs, const float* gates, const float* x, float* gU,
                   float* gW, float* gb, int B, int T, int H, int I, hipStream_t s, int rev) {
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  if (cell == 0 && (2 * H) % 64) return (int)hipErrorInvalidValue;  // candidate columns start on a tile
  const int M = H + I + (gb ? 1 : 0);
  const long BT = (long)B * T;
  const dim3 grid((M + 63) / 64, (G * H + 63) / 64, (unsigned)((BT + PG_BT - 1) / PG_BT));
  const NoDir nd{};
  if (rev) {
    if (cell == 0)
      hipLaunchKernelGGL((rnn_param_grad_kernel<0, true>), grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
    else if (cell == 1)
      hipLaunchKernelGGL((rnn_param_grad_kernel<1, true>), grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
    else
      hipLaunchKernelGGL((rnn_param_grad_kernel<2, true>), grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
    return (int)hipGetLastError();
  }
  if (cell == 0)
    hipLaunchKernelGGL(rnn_param_grad_kernel<0>, grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
  else if (cell == 1)
    hipLaunchKernelGGL(rnn_param_grad_kernel<1>, grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
  else
    hipLaunchKernelGGL(rnn_param_grad_kernel<2>, grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, nd);
  return (int)hipGetLastError();
}

namespace {
template <int CELL, bool REV>
void launch_param_grad_drop(const dim3 grid, hipStream_t s, const float* dg, const float* hs, const float* gates,
                            const float* x, float* gU, float* gW, float* gb, int B, int T, int H, int I,
                            const DropMasks dm) {
  hipLaunchKernelGGL((rnn_param_grad_kernel<CELL, REV, true>), grid, dim3(256), 0, s, dg, hs, gates, x, gU, gW, gb, B, T,
                     H, I, dm);
}
}  // namespace

int rnn_param_grad_drop(int cell, const float* dg, const float* hs, const float* gates, const float* x, const float* dp,
                        const float* rdp, float* gU, float* gW, float* gb, int B, int T, int H, int I, hipStream_t s,
                        int rev) {
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  const int M = H + I + (gb ? 1 : 0);
  const long BT = (long)B * T;
  const dim3 grid((M + 63) / 64, G * ((H + 63) / 64), (unsigned)((BT + PG_BT - 1) / PG_BT));  // j tiles per gate
  const DropMasks dm{dp, rdp};
  if (cell == 0)
    rev ? launch_param_grad_drop<0, true>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm)
        : launch_param_grad_drop<0, false>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm);
  else if (cell == 1)
    rev ? launch_param_grad_drop<1, true>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm)
        : launch_param_grad_drop<1, false>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm);
  else
    rev ? launch_param_grad_drop<2, true>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm)
        : launch_param_grad_drop<2, false>(grid, s, dg, hs, gates, x, gU, gW, gb, B, T, H, I, dm);
  return (int)hipGetLastError();
}

int rnn_drop_x(const float* x, const float* dp, float* xm, int G, int B, int T, int I, hipStream_t s) {
  const long n = (long)G * B * T * I;
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(rnn_drop_x_kernel, dim3(blocks), dim3(256), 0, s, x, dp, xm, G, B, T, I);
  return (int)hipGetLastError();
}

int rnn_drop_dx(const float* t, const float* dp, float* dx, int G, int B, int T, int I, int accumulate, hipStream_t s) {
  const long n = (long)B * T * I;
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(rnn_drop_dx_kernel, dim3(blocks), dim3(256), 0, s, t, dp, dx, G, B, T, I, accumulate);
  return (int)hipGetLastError();
}

int rnn_bwd(int cell, const float* dy, const float* U, const float* UT, const float* hs, const float* cs,
            const float* gates, float* dgates, int B, int T, int H, int rs, int act, int ract, hipStream_t s) {
  const bool reg = rnn_reg_path(cell, H, act, ract);
  if (reg && H == 128)
    return cell == 0 ? launch_bwd_reg<0, 128, RNN_BB_BWD>(dy, U, hs, cs, gates, dgates, B, T, rs, s)
                     : launch_bwd_reg<1, 128, RNN_BB_BWD>(dy, U, hs, cs, gates, dgates, B, T, rs, s);
  if (reg && H == 64)
    return cell == 0 ? launch_bwd_reg<0, 64, 2>(dy, U, hs, cs, gates, dgates, B, T, rs, s)
                     : launch_bwd_reg<1, 64, 2>(dy, U, hs, cs, gates, dgates, B, T, rs, s);
  const int G = cell == 0 ? 3 : (cell == 1 ? 4 : 1);
  const size_t lds = sizeof(float) * (2 * BB * H + BB * G * H);
  const int threads = std::min(512, ((G * H + 63) / 64) * 64);
  const dim3 grid((B + BB - 1) / BB);
  if (cell == 0)
    hipLaunchKernelGGL(rnn_bwd_kernel<0>, grid, dim3(threads), lds, s, dy, UT, hs, cs, gates, dgates, B, T, H, rs, act,
                       ract, NoDir{});
  else if (cell == 1)
    hipLaunchKernelGGL(rnn_bwd_kernel<1>, grid, dim3(threads), lds, s, dy, UT, hs, cs, gates, dgates, B, T, H, rs, act,
                       ract, NoDir{});
  else
    hipLaunchKernelGGL(rnn_bwd_kernel<2>, grid, dim3(threads), lds, s, dy, UT, hs, cs, gates, dgates, B, T, H, rs, act,
                       ract, NoDir{});
  return (int)hipGetLastError();
}

int rnn_fwd_dir(int cell, const RnnDir& d, int ndir, const float* x, int I, int B, int T, int H, int rs, int act,
                int ract, hipStream_t s) {
  if (ndir < 1 || ndir > 2 || (ndir == 2 && !d.xw[0] != !d.xw[1])) return (int)hipErrorInvalidValue;
  if (ndir == 2 && !d.rdp[0] != !d.rdp[1]) return (int)hipErrorInvalidValue;
  if (d.rdp[0])
    return d.mask ? launch_fwd_dir<true, true>(cell, d, ndir, x, I, B, T, H, rs, act, ract, s)
                  : launch_fwd_dir<false, true>(cell, d, ndir, x, I, B, T, H, rs, act, ract, s);
  return d.mask ? launch_fwd_dir<true, false>(cell, d, ndir, x, I, B, T, H, rs, act, ract, s)
                : launch_fwd_dir<false, false>(cell, d, ndir, x, I, B, T, H, rs, act, ract, s);
}

int rnn_bwd_dir(int cell, const RnnDir& d, int ndir, int B, int T, int H, int rs, int act, int ract, hipStream_t s) {
  if (ndir < 1 || ndir > 2 || (ndir == 2 && !d.rdp[0] != !d.rdp[1])) return (int)hipErrorInvalidValue;
  if (d.rdp[0])
    return d.mask ? launch_bwd_dir<true, true>(cell, d, ndir, B, T, H, rs, act, ract, s)
                  : launch_bwd_dir<false, true>(cell, d, ndir, B, T, H, rs, act, ract, s);
  return d.mask ? launch_bwd_dir<true, false>(cell, d, ndir, B, T, H, rs, act, ract, s)
                : launch_bwd_dir<false, false>(cell, d, ndir, B, T, H, rs, act, ract, s);
}

int bidir_merge(const float* a, const float* b, float* out, long n, float scale, hipStream_t s) {
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(bidir_merge_kernel, dim3(blocks), dim3(256), 0, s, a, b, out, n, scale);
  return (int)hipGetLastError();
}

int mask_from_features(const float* x, float* y, unsigned char* mask, long rows, int F, float mask_value,
                       hipStream_t s) {
  if (rows <= 0) return 0;
  if (F < 1) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<long>((rows + 3) / 4, 4096);
  hipLaunchKernelGGL(mask_from_features_kernel, dim3(blocks), dim3(256), 0, s, x, y, mask, rows, F, mask_value);
  return (int)hipGetLastError();
}

int mask_apply(const float* in, const unsigned char* mask, float* out, long rows, int F, hipStream_t s) {
  if (rows <= 0) return 0;
  if (F < 1) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)std::min<long>((rows * F + 255) / 256, 4096);
  hipLaunchKernelGGL(mask_apply_kernel, dim3(blocks), dim3(256), 0, s, in, mask, out, rows, F);
  return (int)hipGetLastError();
}

int mask_from_ids(const long* ids, unsigned char* mask, long n, hipStream_t s) {
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(mask_from_ids_kernel, dim3(blocks), dim3(256), 0, s, ids, mask, n);
  return (int)hipGetLastError();
}

// =============================================================================================
// Replica-batched training step (RnnRep / OptRep, ddl_ops.h; parallel/replica_batch.py).
// The reference runs its dist-keras workers as separate Keras models, num_processes per executor
// (ddl_nyiso_aztk.py:51-55, 206-218); on one MI355X the R co-located replicas of RNN(H) -> Dense(K)
// with an MSE loss are ONE launch per phase: the recurrences of all R x B batch rows run side by side
// (each workgroup reads its replica's U / W from the pointer table), the Dense head + loss + its
// backward is one workgroup per replica, and the parameter gradients and optimizer sweep take the
// replica from blockIdx.z / blockIdx.y.  Gradients are written (not accumulated), so no step zeroes them.
// =============================================================================================
namespace {

constexpr int kRepMaxB = 64, kRepMaxK = 8;

// One workgroup per replica: y = h Wd^T + bd, loss = mean (y - t)^2 over B K (Keras / ops.loss.mse),
// dy = 2 (y - t) / (B K); gWd = dy^T h, gbd = colsum dy, dh = dy Wd; history[ctr] = loss; Adam tick.
template <int H>
__global__ __launch_bounds__(256) void dense_mse_rep_kernel(const float* __restrict__ hlast, float* __restrict__ dh,
                                                            const RnnRep rp, const OptRep op) {
  const int r = blockIdx.x, B = rp.B, K = rp.K, tid = threadIdx.x;
  __shared__ float hsm[kRepMaxB][H + 1];
  __shared__ float dys[kRepMaxB][kRepMaxK];
  __shared__ float red[256];
  const float* hb = hlast + (long)r * B * H;
  for (int i = tid; i < B * H; i += 256) hsm[i / H][i % H] = hb[i];
  const int ctr = *rp.ctr;
  const bool live = ctr < rp.steps[r];  // ragged shards: an exhausted replica computes but does not step
  const float* tgt = rp.y[r] + (long)(ctr % rp.nbr[r]) * B * K;
  const float* Wd = rp.Wd[r];
  const float* bd = rp.bd[r];
  __syncthreads();
  const float sc = 2.f / (float)(B * K);
  float se = 0.f;
  for (int q = tid; q < B * K; q += 256) {
    const int b = q / K, o = q - b * K;
    float a = bd ? bd[o] : 0.f;
    const float* w = Wd + (long)o * H;
#pragma unroll 8
    for (int i = 0; i < H; ++i) a += hsm[b][i] * w[i];
    const float e = a - tgt[q];
    se += e * e;
    dys[b][o] = sc * e;
  }
  red[tid] = se;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    rp.live[r] = live ? 1 : 0;  // read by the optimizer sweep of this step
    if (live) {
      rp.hist[r][ctr] = red[0] / (float)(B * K);
      if (op.t[r]) op.t[r][0] += 1.f;  // Adam's device step counter (read by the optimizer sweep below)
    }
  }
  // gWd[o][i] = sum_b dy[b][o] h[b][i];  gbd[o] = sum_b dy[b][o]
  for (int q = tid; q < K * H; q += 256) {
    const int o = q / H, i = q - o * H;
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dys[b][o] * hsm[b][i];
    rp.gWd[r][q] = a;
  }
  if (rp.gbd[r] && tid < K) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dys[b][tid];
    rp.gbd[r][tid] = a;
  }
  // dh[b][i] = sum_o dy[b][o] Wd[o][i]  (the recurrent backward's dy at the last step)
  float* dhb = dh + (long)r * B * H;
  for (int q = tid; q < B * H; q += 256) {
    const int b = q / H, i = q - b * H;
    float a = 0.f;
    for (int o = 0; o < K; ++o) a += dys[b][o] * Wd[(long)o * H + i];
    dhb[q] = a;
  }
}

// Recurrent parameter gradients: rows m < H gU, H <= m < H + I gW, m = H + I gb (as rnn_param_grad).
// blockIdx.z = replica * S + slice: a workgroup sums PG_BT-row chunks [slice, slice + S, ...) of its
// replica's B T rows.  S = 1 (deterministic mode): one writer per output, plain stores in row order;
// S > 1: fp32 atomics into gradients the optimizer sweep of the previous step left zeroed.
template <int CELL>
__global__ __launch_bounds__(256) void rnn_param_grad_rep_kernel(const float* __restrict__ dg, const float* __restrict__ hs,
                                                                 const float* __restrict__ gates, const RnnRep rp,
                                                                 int T, int H, int I, int S) {
  constexpr int G = CELL == 0 ? 3 : (CELL == 1 ? 4 : 1);
  const int GH = G * H, r = blockIdx.z / S, slice = blockIdx.z - r * S, B = rp.B;
  const bool has_b = rp.gb[r] != nullptr;
  const int M = H + I + (has_b ? 1 : 0);
  const long BT = (long)B * T, row0 = (long)r * B;  // global batch row of the replica's row 0
  const long xrow0 = (long)(*rp.ctr % rp.nbr[r]) * B;  // shard row of its mini-batch
  const float* x = rp.x[r];
  const int m0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  __shared__ float As[PG_BT][64 + 1];
  __shared__ float Ds[PG_BT][64 + 1];
  const bool cand = CELL == 0 && j0 >= 2 * H;
  const int c = threadIdx.x & 63, q0 = threadIdx.x >> 6;
  const int tm = (threadIdx.x / 16) * 4, tj = (threadIdx.x % 16) * 4;
  float acc[4][4] = {};
  for (long bt0 = (long)slice * PG_BT; bt0 < BT; bt0 += (long)S * PG_BT) {
    const int nbt = (int)min((long)PG_BT, BT - bt0);
    long b = (bt0 + q0) / T, t = (bt0 + q0) - b * T;
    for (int q = q0; q < nbt; q += 4, t += 4) {
      while (t >= T) { t -= T; ++b; }
      const long gbt = (row0 + b) * T + t;  // global (row, step)
      const int m = m0 + c;
      float a = 0.f;
      if (m < H) {
        a = hs[((row0 + b) * (T + 1) + t) * H + m];
        if (cand) a *= gates[gbt * GH + H + m];
      } else if (m < H + I) {
        a = x[((xrow0 + b) * T + t) * I + (m - H)];
      } else if (m < M) {
        a = 1.f;
      }
      As[q][c] = a;
      const int jj = j0 + c;
      Ds[q][c] = jj < GH ? dg[gbt * GH + jj] : 0.f;
    }
    __syncthreads();
    for (int q = 0; q < nbt; ++q) {
      float a[4], d[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[q][tm + i]; d[i] = Ds[q][tj + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[i][l] += a[i] * d[l];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tm + i;
    if (m >= M) continue;
    float* dst = m < H ? rp.gU[r] + (long)m * GH : (m < H + I ? rp.gW[r] + (long)(m - H) * GH : rp.gb[r]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int jj = j0 + tj + l;
      if (jj < GH) {
        if (S == 1) dst[jj] = acc[i][l];
        else atomicAdd(dst + jj, acc[i][l]);
      }
    }
  }
}

// Optimizer sweep over the R replica arenas (blockIdx.y = replica), Keras semantics as the per-replica
// kernels (optim.hip): OPT 0 SGD (+momentum p1), 1 Adagrad, 2 Adam (b1 = p1, b2 = p2, amode as adam_step).
// zero_g: leave the gradients zeroed for the next step's atomic parameter-gradient slices.  Block (0, 0)
// advances the shared step counter (no block of this kernel reads it: the live flags come from the head kernel).
// A dead replica (ragged shard exhausted) keeps its parameters and state; its gradients are still zeroed.
template <int OPT>
__global__ __launch_bounds__(256) void opt_rep_kernel(const OptRep op, long n4, float lr, float p1, float p2, float eps,
                                                      float wd, int amode, int* ctr, const int* __restrict__ live,
                                                      int zero_g) {
  const int r = blockIdx.y;
  if (!live[r]) {
    if (zero_g) {
      float4* g = const_cast<float4*>(reinterpret_cast<const float4*>(op.g[r]));
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
        g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ctr += 1;
    return;
  }
  float4* w = reinterpret_cast<float4*>(op.w[r]);
  float4* g = const_cast<float4*>(reinterpret_cast<const float4*>(op.g[r]));
  float4* s1 = reinterpret_cast<float4*>(op.s1[r]);
  float4* s2 = reinterpret_cast<float4*>(op.s2[r]);
  float bc1 = 1.f, bc2 = 1.f;
  if constexpr (OPT == 2) {
    const float t = op.t[r][0];
    bc1 = 1.f - powf(p1, t);
    bc2 = 1.f - powf(p2, t);
  }
  const float sbc2 = sqrtf(bc2);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 p = w[i], d = g[i];
    float4 a = s1 ? s1[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = (OPT == 2) ? s2[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float *pp = &p.x, *dd = &d.x, *aa = &a.x, *vv = &v.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (OPT == 0) {
        float gg = dd[k] + wd * pp[k];
        if (s1) {
          aa[k] = p1 * aa[k] + gg;
          gg = aa[k];
        }
        pp[k] -= lr * gg;
      } else if constexpr (OPT == 1) {
        const float gg = dd[k] + wd * pp[k];
        aa[k] += gg * gg;
        pp[k] -= lr * gg / (sqrtf(aa[k]) + eps);
      } else {
        float gg = dd[k];
        if (amode & 1) pp[k] *= (1.f - lr * wd);
        else gg += wd * pp[k];
        aa[k] = p1 * aa[k] + (1.f - p1) * gg;
        vv[k] = p2 * vv[k] + (1.f - p2) * gg * gg;
        if (amode & 2) pp[k] -= lr * (sbc2 / bc1) * aa[k] / (sqrtf(vv[k]) + eps);
        else pp[k] -= lr * (aa[k] / bc1) / (sqrtf(vv[k]) / sbc2 + eps);
      }
    }
    w[i] = p;
    if (s1) s1[i] = a;
    if constexpr (OPT == 2) s2[i] = v;
    if (zero_g) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *ctr += 1;
}

template <int CELL, int H>
int rep_step(const RnnRep& rp, int R, int T, int I, float* hs, float* cs, float* gates, float* hlast, float* dh,
             float* dgates, const OptRep& op, long n, int opt, float lr, float p1, float p2, float eps, float wd,
             int amode, hipStream_t s) {
  constexpr int G = CELL == 0 ? 3 : 4;
  constexpr int BBF = H == 128 ? RNN_BB_FWD : 2, BBB = H == 128 ? RNN_BB_BWD : 2;
  const int RB = R * rp.B;
  hipLaunchKernelGGL((rnn_fwd_reg_kernel<CELL, H, BBF, true, true>), dim3((RB + BBF - 1) / BBF),
                     dim3(fwd_threads<CELL, H>()), 0, s, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, I, (const float*)nullptr, hs, cs, gates, hlast, RB,
                     T, 0, rp);
  hipLaunchKernelGGL((dense_mse_rep_kernel<H>), dim3(R), dim3(256), 0, s, hlast, dh, rp, op);
  hipLaunchKernelGGL((rnn_bwd_reg_kernel<CELL, H, BBB, true>), dim3((RB + BBB - 1) / BBB), dim3(bwd_threads<CELL, H>()),
                     0, s, dh, (const float*)nullptr, hs, cs, gates, dgates, RB, T, 0, rp);
  const int M = H + I + 1;
  // row slices of the parameter gradients (atomics); deterministic mode: one ordered writer per output
  const int S = deterministic() ? 1 : (int)std::max<long>(1, ((long)rp.B * T + PG_BT - 1) / PG_BT);
  hipLaunchKernelGGL((rnn_param_grad_rep_kernel<CELL>), dim3((M + 63) / 64, (G * H + 63) / 64, R * S), dim3(256), 0,
                     s, dgates, hs, gates, rp, T, H, I, S);
  const long n4 = n / 4;
  const dim3 og((unsigned)std::min<long>((n4 + 255) / 256, 1024), R);
  const int zg = S > 1;
  if (opt == 0)
    hipLaunchKernelGGL(opt_rep_kernel<0>, og, dim3(256), 0, s, op, n4, lr, p1, p2, eps, wd, amode, rp.ctr, rp.live,
                       zg);
  else if (opt == 1)
    hipLaunchKernelGGL(opt_rep_kernel<1>, og, dim3(256), 0, s, op, n4, lr, p1, p2, eps, wd, amode, rp.ctr, rp.live,
                       zg);
  else
    hipLaunchKernelGGL(opt_rep_kernel<2>, og, dim3(256), 0, s, op, n4, lr, p1, p2, eps, wd, amode, rp.ctr, rp.live,
                       zg);
  return (int)hipGetLastError();
}

}  // namespace

bool rnn_replica_ok(int cell, int H, int I, int K, int B) {
  return (cell == 0 || cell == 1) && (H == 128 || (H == 64 && B % 2 == 0)) && I >= 1 && I <= IMAX && K >= 1 &&
         K <= kRepMaxK && B >= 1 && B <= kRepMaxB;
}

int rnn_replica_step(int cell, const RnnRep& rp, int R, int T, int H, int I, float* hs, float* cs, float* gates,
                     float* hlast, float* dh, float* dgates, const OptRep& op, long n, int opt, float lr, float p1,
                     float p2, float eps, float wd, int amode, hipStream_t s) {
  if (!rnn_replica_ok(cell, H, I, rp.K, rp.B) || R < 1 || R > kMaxRnnRep || n % 4 || opt < 0 || opt > 2 || !rp.live)
    return (int)hipErrorInvalidValue;
  for (int r = 0; r < R; ++r)
    if (rp.nbr[r] < 1) return (int)hipErrorInvalidValue;
  if (cell == 0)
    return H == 128 ? rep_step<0, 128>(rp, R, T, I, hs, cs, gates, hlast, dh, dgates, op, n, opt, lr, p1, p2, eps, wd, amode, s)
                    : rep_step<0, 64>(rp, R, T, I, hs, cs, gates, hlast, dh, dgates, op, n, opt, lr, p1, p2, eps, wd, amode, s);
  return H == 128 ? rep_step<1, 128>(rp, R, T, I, hs, cs, gates, hlast, dh, dgates, op, n, opt, lr, p1, p2, eps, wd, amode, s)
                  : rep_step<1, 64>(rp, R, T, I, hs, cs, gates, hlast, dh, dgates, op, n, opt, lr, p1, p2, eps, wd, amode, s);
}

}  // namespace ddl
