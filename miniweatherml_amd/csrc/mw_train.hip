// =====================================================================================================
// mw_train.hip -- native training of the ponni 5 -> 10 -> 4 surrogate (the reference's Keras notebooks,
// experiments/supercell_kessler_surrogate/jupyter_notebooks/kessler_singlecell_train_example.ipynb and kessler_netcdf_to_numpy.ipynb):
// Dense(10) -> LeakyReLU(0.1) -> Dense(4), loss mse, Nadam, fit(batch_size, shuffle=True).  DESIGN.md section 13.
//
// k_surrogate_train: ONE workgroup (256 threads = 4 waves) per model, the epoch's batches loop inside.  A batch is cut into chunks of
// 256 samples, one per thread.  Per chunk every thread runs its sample's forward and backward pass on the VALU (weights in LDS) and
// writes two 16-float rows into its wave's LDS slice:
//   A = [x0..x4, 1, h0..h9]                 (features of the sample: layer-1 inputs, the bias input, the hidden activations)
//   D = [dpre0..dpre9, r0..r3, sum r^2, sum |r|]   (r = y - t; dpre = leaky'(pre) * W2 r; unscaled: times 2 / (4 B) below)
// and the wave adds A^T D over its 64 samples on the matrix cores: 16 x v_mfma_f32_16x16x4_f32 with the samples as the reduction axis
// (lane (g, c) feeds A[sample 4j+g][c] and D[sample 4j+g][c]; the 16x16 result has row = feature, column = delta).  Every gradient is
// a block of that tile: dW1 = rows 0-4 x cols 0-9, db1 = row 5 x cols 0-9, db2 = row 5 x cols 10-13, dW2 = rows 6-15 x cols 10-13, and
// row 5 x cols 14 / 15 are the batch's sums of r^2 and |r|.  At the end of a batch the four waves' tiles are added in wave order through
// LDS; tile entry e (= register e >> 6 of lane e & 63) belongs to thread e, which keeps that parameter and its two Nadam moments in
// registers for the whole epoch and writes the updated weight back to LDS.  The reduction order is fixed: bit-identical run to run, and
// a model's result does not depend on the other workgroups.
//
// The STENCIL model (9 -> 10 -> 4, NIN = 9): A = [x(9), 1, h(10)] is 20 rows, so the wave accumulates TWO 16x16 tiles over the same D:
//   P = [x0..x8, 1]^T D : dW1 = rows 0-8 x cols 0-9, db1 = row 9 x cols 0-9, db2 = row 9 x cols 10-13, the two sums = row 9 x cols 14 / 15
//   Q = [h0..h8, 0, h9]^T D : dW2 = rows 0-8 and 10 x cols 10-13 (h9 sits in row 10 so that no Q entry shares a thread with a live P entry)
// 32 MFMAs per 64-sample chunk, 146 live entries, still one per thread: thread e owns entry e of P if that is live, else entry e of Q.
// (A 32x32x2 tile would hold all 20 rows at once, but 16 accumulator registers per lane with 1024 entries over 256 threads breaks "entry
// e belongs to thread e", and its 32 columns would be half empty; two 16x16 tiles cost 4 more accumulator registers and 8 KiB less LDS.)
// The single-cell instantiation (NIN = 5) is the code above, unchanged in every operation.
//
// WEIGHTED (k_surrogate_train<NIN, true>, mw_surrogate_train_epoch_w): Keras' sample_weight.  The sample's weight
// comes with its x and t through the same permuted index (one more 4-byte gather, prefetched with the others) and multiplies its whole D
// row -- the ten dpre, the four r, sum r^2 and sum |r| -- so that the tile is sum_i w_i A_i^T D_i; A, the MFMAs, the tile sum, the 0.5 / B
// factor and Nadam are the code of the unweighted instantiation, which has no weight in its Sample, no load and no multiply.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_common.h"
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace mw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the permutations (restated in miniweatherml_amd/surrogate_train.py; the tests replay them) ----
__host__ __device__ __forceinline__ uint64_t sm64(uint64_t z) {         // splitmix64 (include/mw_cdna4.h, "Substitutions")
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {        // round function: a 32-bit integer hash (lowbias32)
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
static constexpr uint64_t TAG_PRESHUFFLE = ~0ull;                        // stream tags: epoch e uses tag e

struct Feistel { uint32_t k[4]; uint32_t mask; int h; long long n; };
// The permutation of [0, n) for the stream (a, tag): base = sm64(sm64(a) ^ tag), round key r = high word of sm64(base + r); the domain is
// 4^h >= n (h >= 1), x = (L << h) | R, four rounds (L, R) <- (R, L ^ (mix32(R ^ k_r) & mask)), then cycle-walking until the value is < n.
__host__ __device__ inline Feistel make_feistel(uint64_t a, uint64_t tag, long long n) {
  Feistel F;
  const uint64_t base = sm64(sm64(a) ^ tag);
  for (int r = 0; r < 4; r++) F.k[r] = (uint32_t)(sm64(base + (uint64_t)r) >> 32);
  int h = 1;
  while (h < 32 && (1ll << (2 * h)) < n) h++;
  F.h = h; F.mask = (uint32_t)((1ull << h) - 1); F.n = n;
  return F;
}
__device__ __forceinline__ long long feistel_index(const Feistel &F, long long p) {
  uint64_t x = (uint64_t)p;
  do {
    uint32_t L = (uint32_t)(x >> F.h), R = (uint32_t)x & F.mask;
#pragma unroll
    for (int r = 0; r < 4; r++) { const uint32_t t = L ^ (mix32(R ^ F.k[r]) & F.mask); L = R; R = t; }
    x = ((uint64_t)L << F.h) | R;
  } while (x >= (uint64_t)F.n);
  return (long long)x;
}

// ---- the batch routine (shared by the trainer and the test aid) ----
constexpr int TPB = 256;
template <int NIN> constexpr int npar() { return NIN * 10 + 10 + 40 + 4; }      // 104 | 144
struct SetRef { const float *x, *y; long long n; };
struct Identity { __device__ long long operator()(long long p) const { return p; } };
struct Shuffled { Feistel F; __device__ long long operator()(long long p) const { return feistel_index(F, p); } };
template <int NIN, bool WEIGHTED> struct Sample { float v[NIN + 4 + (WEIGHTED ? 1 : 0)]; };    // x0..x(NIN-1), t0..t3, then the weight

template <int NIN> struct Smem;
template <> struct Smem<5> {
  float W[104];                                                         // the current parameters
  float A[TPB][16], D[TPB][16];                                         // one chunk's rows, wave w owns rows 64 w .. 64 w + 63
  float G[4][TPB];                                                      // the waves' gradient tiles
};
template <> struct Smem<9> {
  float W[144];
  float A[TPB][12], H[TPB][12], D[TPB][16];                             // A = [x0..x8, 1, 0, 0], H = [h0..h8, 0, h9, 0]
  float G[4][2][TPB];                                                   // the waves' tiles P and Q
};

// sample at batch position c + threadIdx.x (zero beyond the batch); wt (n,): the samples' weights, read by the WEIGHTED instantiation alone
template <int NIN, bool WEIGHTED, class Pos>
__device__ __forceinline__ void fetch(const SetRef &S, const float *wt, const Pos &pos, long long first, int B, int c, Sample<NIN, WEIGHTED> &s) {
  const int i = c + (int)threadIdx.x;
  const bool ok = i < B;
  const long long idx = ok ? pos(first + i) : 0;
#pragma unroll
  for (int f = 0; f < NIN; f++) s.v[f] = ok ? S.x[f * S.n + idx] : 0.f;
#pragma unroll
  for (int o = 0; o < 4; o++) s.v[NIN + o] = ok ? S.y[o * S.n + idx] : 0.f;
  if constexpr (WEIGHTED) s.v[NIN + 4] = ok ? wt[idx] : 0.f;
}

template <bool WEIGHTED>
__device__ __forceinline__ void sample_rows(const float *W, const Sample<5, WEIGHTED> &s, bool ok, float *a, float *d) {
  const float *W1 = W, *b1 = W + 50, *W2 = W + 60, *b2 = W + 100;
  float pre[10], h[10], r[4];
#pragma unroll
  for (int u = 0; u < 10; u++) {
    float acc = b1[u];
#pragma unroll
    for (int i = 0; i < 5; i++) acc = fmaf(s.v[i], W1[i * 10 + u], acc);
    pre[u] = acc;
    h[u] = acc > 0.f ? acc : 0.1f * acc;
  }
  float sq = 0.f, ab = 0.f;
#pragma unroll
  for (int n = 0; n < 4; n++) {
    float acc = b2[n];
#pragma unroll
    for (int u = 0; u < 10; u++) acc = fmaf(h[u], W2[u * 4 + n], acc);
    r[n] = acc - s.v[5 + n];
    sq = fmaf(r[n], r[n], sq);
    ab += fabsf(r[n]);
  }
  f32x4 A[4], D[4];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    float av, dv;
    if (i < 5) av = s.v[i]; else if (i == 5) av = 1.f; else av = h[i - 6];
    if (i < 10) {
      float acc = 0.f;
#pragma unroll
      for (int n = 0; n < 4; n++) acc = fmaf(W2[i * 4 + n], r[n], acc);
      dv = pre[i] > 0.f ? acc : 0.1f * acc;                              // leaky_relu'(pre): 1 above 0, else the slope
    } else if (i < 14) dv = r[i - 10];
    else dv = (i == 14) ? sq : ab;
    if constexpr (WEIGHTED) dv *= s.v[9];                                 // the whole D row times the sample's weight; A is untouched
    A[i >> 2][i & 3] = ok ? av : 0.f;
    D[i >> 2][i & 3] = ok ? dv : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) { ((f32x4 *)a)[q] = A[q]; ((f32x4 *)d)[q] = D[q]; }
}

// the stencil model's rows: a = [x0..x8, 1, 0, 0], hrow = [h0..h8, 0, h9, 0] (12 floats each), d as above
template <bool WEIGHTED>
__device__ __forceinline__ void sample_rows(const float *W, const Sample<9, WEIGHTED> &s, bool ok, float *a, float *hrow, float *d) {
  const float *W1 = W, *b1 = W + 90, *W2 = W + 100, *b2 = W + 140;
  float pre[10], h[10], r[4];
#pragma unroll
  for (int u = 0; u < 10; u++) {
    float acc = b1[u];
#pragma unroll
    for (int i = 0; i < 9; i++) acc = fmaf(s.v[i], W1[i * 10 + u], acc);
    pre[u] = acc;
    h[u] = acc > 0.f ? acc : 0.1f * acc;
  }
  float sq = 0.f, ab = 0.f;
#pragma unroll
  for (int n = 0; n < 4; n++) {
    float acc = b2[n];
#pragma unroll
    for (int u = 0; u < 10; u++) acc = fmaf(h[u], W2[u * 4 + n], acc);
    r[n] = acc - s.v[9 + n];
    sq = fmaf(r[n], r[n], sq);
    ab += fabsf(r[n]);
  }
  f32x4 A[3], H[3], D[4];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const float av = i < 9 ? s.v[i] : i == 9 ? 1.f : 0.f;
    const float hv = i < 9 ? h[i] : i == 10 ? h[9] : 0.f;
    A[i >> 2][i & 3] = ok ? av : 0.f;
    H[i >> 2][i & 3] = ok ? hv : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    float dv;
    if (i < 10) {
      float acc = 0.f;
#pragma unroll
      for (int n = 0; n < 4; n++) acc = fmaf(W2[i * 4 + n], r[n], acc);
      dv = pre[i] > 0.f ? acc : 0.1f * acc;
    } else if (i < 14) dv = r[i - 10];
    else dv = (i == 14) ? sq : ab;
    if constexpr (WEIGHTED) dv *= s.v[13];
    D[i >> 2][i & 3] = ok ? dv : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 3; q++) { ((f32x4 *)a)[q] = A[q]; ((f32x4 *)hrow)[q] = H[q]; }
#pragma unroll
  for (int q = 0; q < 4; q++) ((f32x4 *)d)[q] = D[q];
}

// LDS rows written by other lanes of the SAME wave become visible (no workgroup barrier needed: a wave reads only its own slice)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Raw gradient tile entry threadIdx.x of one batch (sum over its samples of A^T D, waves added in order 0..3).  On entry `pf` holds this
// thread's sample of the batch's first chunk; on exit the sample of the NEXT batch's first chunk (next_B > 0), fetched while this batch's
// last chunk computes.  Ends with the tile in sm.G (read after a workgroup barrier); the caller barriers before the next call.
template <bool WEIGHTED, class Pos>
__device__ float batch_tile(Smem<5> &sm, const SetRef &S, const float *wt, const Pos &pos, long long first, int B, long long next_first, int next_B,
                            Sample<5, WEIGHTED> &pf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < B; c0 += TPB) {
    const Sample<5, WEIGHTED> cur = pf;
    if (c0 + TPB < B) fetch(S, wt, pos, first, B, c0 + TPB, pf);
    else if (next_B > 0) fetch(S, wt, pos, next_first, next_B, 0, pf);
    sample_rows(sm.W, cur, c0 + tid < B, sm.A[tid], sm.D[tid]);
    wave_sync();
    const float *Aw = sm.A[wave * 64], *Dw = sm.D[wave * 64];
#pragma unroll
    for (int j = 0; j < 16; j++)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Aw[(4 * j + g) * 16 + c], Dw[(4 * j + g) * 16 + c], acc, 0, 0, 0);
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < 4; r++) sm.G[wave][r * 64 + lane] = acc[r];
  __syncthreads();
  return ((sm.G[0][tid] + sm.G[1][tid]) + sm.G[2][tid]) + sm.G[3][tid];
}

// The stencil model's: the tiles P and Q (see the header), the thread's own entry taken from the tile `which` (0 = P, 1 = Q).
template <bool WEIGHTED, class Pos>
__device__ float batch_tile(Smem<9> &sm, const SetRef &S, const float *wt, const Pos &pos, long long first, int B, long long next_first, int next_B,
                            Sample<9, WEIGHTED> &pf, int which) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  f32x4 accP = {0.f, 0.f, 0.f, 0.f}, accQ = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < B; c0 += TPB) {
    const Sample<9, WEIGHTED> cur = pf;
    if (c0 + TPB < B) fetch(S, wt, pos, first, B, c0 + TPB, pf);
    else if (next_B > 0) fetch(S, wt, pos, next_first, next_B, 0, pf);
    sample_rows(sm.W, cur, c0 + tid < B, sm.A[tid], sm.H[tid], sm.D[tid]);
    wave_sync();
    const float *Aw = sm.A[wave * 64], *Hw = sm.H[wave * 64], *Dw = sm.D[wave * 64];
    const int ca = c < 12 ? c : 11;                                     // columns 12..15 of A and H do not exist: zero rows of the tiles
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const float dv = Dw[(4 * j + g) * 16 + c], av = Aw[(4 * j + g) * 12 + ca], hv = Hw[(4 * j + g) * 12 + ca];
      accP = __builtin_amdgcn_mfma_f32_16x16x4f32(c < 12 ? av : 0.f, dv, accP, 0, 0, 0);
      accQ = __builtin_amdgcn_mfma_f32_16x16x4f32(c < 12 ? hv : 0.f, dv, accQ, 0, 0, 0);
    }
    wave_sync();
  }
#pragma unroll
  for (int r = 0; r < 4; r++) { sm.G[wave][0][r * 64 + lane] = accP[r]; sm.G[wave][1][r * 64 + lane] = accQ[r]; }
  __syncthreads();
  return ((sm.G[0][which][tid] + sm.G[1][which][tid]) + sm.G[2][which][tid]) + sm.G[3][which][tid];
}

// tile entry e (register e >> 6, lane e & 63: row 4 (lane >> 4) + reg, column lane & 15) -> parameter index, or -1 / -2 (sum r^2) / -3 (sum |r|)
__device__ __forceinline__ int param_of_entry(int e) {
  const int lane = e & 63, row = 4 * (lane >> 4) + (e >> 6), col = lane & 15;
  if (row < 5 && col < 10) return row * 10 + col;                       // W1 (5,10)
  if (row == 5 && col < 10) return 50 + col;                            // b1
  if (row == 5 && col < 14) return 100 + col - 10;                      // b2
  if (row >= 6 && col >= 10 && col < 14) return 60 + (row - 6) * 4 + col - 10;   // W2 (10,4)
  if (row == 5) return col == 14 ? -2 : -3;
  return -1;
}

// the stencil model's: sets `which` (the tile the entry is read from)
__device__ __forceinline__ int param_of_entry9(int e, int &which) {
  const int lane = e & 63, row = 4 * (lane >> 4) + (e >> 6), col = lane & 15;
  which = 0;
  if (row < 9 && col < 10) return row * 10 + col;                       // P: W1 (9,10)
  if (row == 9 && col < 10) return 90 + col;                            // P: b1
  if (row == 9 && col < 14) return 140 + col - 10;                      // P: b2
  if (row == 9) return col == 14 ? -2 : -3;
  which = 1;
  if (col >= 10 && col < 14 && (row < 9 || row == 10)) return 100 + (row < 9 ? row : 9) * 4 + col - 10;   // Q: W2 (10,4), h9 in row 10
  return -1;
}

struct TrainArgs {
  SetRef S; int B; int epoch; uint64_t seed;
  float *params, *m1, *m2; const float *table; double *stats;
  float beta1, beta2, eps;
  const float *wt;                                                      // (n,) sample weights: the WEIGHTED instantiations' (last: the others' layout stays)
};

template <int NIN, bool WEIGHTED>
__global__ __launch_bounds__(TPB) void k_surrogate_train(TrainArgs a) {
  constexpr int NPAR = npar<NIN>();
  __shared__ Smem<NIN> sm;
  const int tid = threadIdx.x, model = blockIdx.x;
  int which = 0;
  const int p = NIN == 5 ? param_of_entry(tid) : param_of_entry9(tid, which);
  float w = 0.f, m = 0.f, v = 0.f;
  if (p >= 0) {
    w = a.params[model * NPAR + p]; m = a.m1[model * NPAR + p]; v = a.m2[model * NPAR + p];
    sm.W[p] = w;
  }
  const Shuffled pos{make_feistel(a.seed + (uint64_t)model, (uint64_t)a.epoch, a.S.n)};
  const long long n = a.S.n, steps = (n + a.B - 1) / a.B;
  Sample<NIN, WEIGHTED> pf;
  fetch(a.S, a.wt, pos, 0, (int)std::min<long long>(a.B, n), 0, pf);
  double sq = 0.0, ab = 0.0;
  __syncthreads();
  for (long long s = 0; s < steps; s++) {
    const long long first = s * a.B;
    const int B = (int)std::min<long long>(a.B, n - first);
    const long long nf = first + B;
    const int nB = (int)std::min<long long>(a.B, n - nf);
    float gsum;
    if constexpr (NIN == 5) gsum = batch_tile(sm, a.S, a.wt, pos, first, B, nf, nB > 0 ? nB : 0, pf);
    else gsum = batch_tile(sm, a.S, a.wt, pos, first, B, nf, nB > 0 ? nB : 0, pf, which);
    if (p >= 0) {                                                       // Nadam (TF 2.x Keras), scalars from the host table
      const float cg = a.table[3 * s], cm = a.table[3 * s + 1], bc2 = a.table[3 * s + 2];
      const float gr = gsum * (0.5f / (float)B);                        // d mean((y - t)^2) = 2 r / (4 B)
      m = a.beta1 * m + (1.f - a.beta1) * gr;
      v = a.beta2 * v + (1.f - a.beta2) * gr * gr;
      w -= (cg * gr + cm * m) / (sqrtf(v / bc2) + a.eps);
      sm.W[p] = w;
    } else if (p == -2) sq += (double)gsum;
    else if (p == -3) ab += (double)gsum;
    __syncthreads();
  }
  if (p >= 0) { a.params[model * NPAR + p] = w; a.m1[model * NPAR + p] = m; a.m2[model * NPAR + p] = v; }
  else if (p == -2) a.stats[2 * model] = sq;
  else if (p == -3) a.stats[2 * model + 1] = ab;
}

template <int NIN, bool WEIGHTED>
__global__ __launch_bounds__(TPB) void k_surrogate_grad(const float *__restrict__ params, SetRef S, int B, float *__restrict__ grad,
                                                        float *__restrict__ loss, const float *__restrict__ wt) {
  __shared__ Smem<NIN> sm;
  int which = 0;
  const int tid = threadIdx.x, p = NIN == 5 ? param_of_entry(tid) : param_of_entry9(tid, which);
  if (p >= 0) sm.W[p] = params[p];
  Sample<NIN, WEIGHTED> pf;
  fetch(S, wt, Identity(), 0, B, 0, pf);
  __syncthreads();
  float gsum;
  if constexpr (NIN == 5) gsum = batch_tile(sm, S, wt, Identity(), 0, B, 0, 0, pf);
  else gsum = batch_tile(sm, S, wt, Identity(), 0, B, 0, 0, pf, which);
  if (p >= 0) grad[p] = gsum * (0.5f / (float)B);
  else if (p == -2) loss[0] = gsum / (4.f * (float)B);
}

// ---- data preparation: pre-shuffle, split, scaling, feature-major sets ----
struct PrepArgs {
  long long n, n_train, n_val; Feistel F; const float *raw_in, *raw_out;
  double in_min[9], in_rng[9], out_min[4], out_rng[4];
  float *x[3], *y[3];
};
// TEND: the labels of the tendency form -- the sample's change, fp64 difference of the two fp32 records, scaled by the table of the changes
template <int NIN, bool TEND>
__global__ __launch_bounds__(TPB) void k_surrogate_prepare(PrepArgs a) {
#pragma clang fp contract(off)
  const long long stride = (long long)gridDim.x * TPB;
  for (long long p = (long long)blockIdx.x * TPB + threadIdx.x; p < a.n; p += stride) {
    const long long src = feistel_index(a.F, p);
    const int set = p < a.n_train ? 0 : p < a.n_train + a.n_val ? 1 : 2;
    const long long q = set == 0 ? p : set == 1 ? p - a.n_train : p - a.n_train - a.n_val;
    const long long len = set == 0 ? a.n_train : set == 1 ? a.n_val : a.n - a.n_train - a.n_val;
#pragma unroll
    for (int f = 0; f < NIN; f++) a.x[set][f * len + q] = (float)(((double)a.raw_in[src * NIN + f] - a.in_min[f]) / a.in_rng[f]);
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const int base = o == 0 ? 0 : o + 1;                                  // temp, rho_v, rho_c, rho_r among the inputs
      if (TEND) a.y[set][o * len + q] = (float)((((double)a.raw_out[src * 4 + o] - (double)a.raw_in[src * NIN + base]) - a.out_min[o]) / a.out_rng[o]);
      else      a.y[set][o * len + q] = (float)(((double)a.raw_out[src * 4 + o] - a.out_min[o]) / a.out_rng[o]);
    }
  }
}

// one fp32 value per sample through k_surrogate_prepare's pre-shuffle and split (the samples' weights, their file index)
struct ColArgs { long long n, n_train, n_val; Feistel F; const float *col; float *out[3]; };
__global__ __launch_bounds__(TPB) void k_surrogate_prepare_column(ColArgs a) {
  const long long stride = (long long)gridDim.x * TPB;
  for (long long p = (long long)blockIdx.x * TPB + threadIdx.x; p < a.n; p += stride) {
    const long long src = feistel_index(a.F, p);
    const int set = p < a.n_train ? 0 : p < a.n_train + a.n_val ? 1 : 2;
    const long long q = set == 0 ? p : set == 1 ? p - a.n_train : p - a.n_train - a.n_val;
    a.out[set][q] = a.col[src];
  }
}

// ---- error sums of predictions (validation loss, test metrics) ----
// WEIGHTED: every sum term times (double)w_i, the two maxima over the samples with w_i > 0 (a zero-weight sample does not exist); with
// w = 1 the bits of the unweighted instantiation (the terms d (d w), w |d|, w d, w |t| are the unweighted ones times an exact 1).
constexpr int ERR_BLOCKS = 128, NSTAT = 24;
template <bool WEIGHTED>
__global__ __launch_bounds__(TPB) void k_surrogate_sums(long long n, const float *__restrict__ pred, const float *__restrict__ y,
                                                          double *__restrict__ partial, const float *__restrict__ wt) {
  __shared__ double red[NSTAT][TPB];
  const int tid = threadIdx.x, set = blockIdx.y;
  double acc[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = 0.0;
  const float *ps = pred + (long long)set * 4 * n;
  for (long long i = (long long)blockIdx.x * TPB + tid; i < n; i += (long long)ERR_BLOCKS * TPB) {
#pragma unroll
    for (int o = 0; o < 4; o++) {
      const double t = y[o * n + i], d = t - (double)ps[o * n + i];
      if constexpr (WEIGHTED) {
        const double w = (double)wt[i], dw = d * w;
        acc[6 * o] += d * dw; acc[6 * o + 1] += w * fabs(d); acc[6 * o + 2] += w * d; acc[6 * o + 3] += w * fabs(t);
        if (w > 0.0) { acc[6 * o + 4] = fmax(acc[6 * o + 4], fabs(d)); acc[6 * o + 5] = fmax(acc[6 * o + 5], fabs(t)); }
      } else {
        acc[6 * o] += d * d; acc[6 * o + 1] += fabs(d); acc[6 * o + 2] += d; acc[6 * o + 3] += fabs(t);
        acc[6 * o + 4] = fmax(acc[6 * o + 4], fabs(d)); acc[6 * o + 5] = fmax(acc[6 * o + 5], fabs(t));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NSTAT; k++) red[k][tid] = acc[k];
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int k = 0; k < NSTAT; k++) red[k][tid] = (k % 6 >= 4) ? fmax(red[k][tid], red[k][tid + s]) : red[k][tid] + red[k][tid + s];
    __syncthreads();
  }
  if (tid < NSTAT) partial[((long long)set * ERR_BLOCKS + blockIdx.x) * NSTAT + tid] = red[tid][0];
}
__global__ __launch_bounds__(64) void k_surrogate_sums_final(int nsets, const double *__restrict__ partial, double *__restrict__ out) {
  const int k = threadIdx.x % NSTAT, set = blockIdx.x * (64 / NSTAT) + threadIdx.x / NSTAT;
  if (threadIdx.x >= (64 / NSTAT) * NSTAT || set >= nsets) return;
  double s = 0.0;
  for (int b = 0; b < ERR_BLOCKS; b++) {
    const double q = partial[((long long)set * ERR_BLOCKS + b) * NSTAT + k];
    s = (k % 6 >= 4) ? fmax(s, q) : s + q;
  }
  out[set * NSTAT + k] = s;
}

} // namespace mw

using namespace mw;

extern "C" {

static int check_n_in(int n_in, const char *who) {
  if (n_in != 5 && n_in != 9) MW_FAIL(std::string(who) + ": n_in must be 5 (single cell) or 9 (stencil), got " + std::to_string(n_in));
  return 0;
}

int mw_surrogate_prepare_form(int form, int n_in, long long n, const float *raw_in, const float *raw_out, const double *scl_in,
                              const double *scl_out, unsigned long long seed, long long n_train, long long n_val, float *train_x,
                              float *train_y, float *val_x, float *val_y, float *test_x, float *test_y, void *stream) {
  if (form != MW_FORM_STATE && form != MW_FORM_TENDENCY)
    MW_FAIL("surrogate_prepare: form must be MW_FORM_STATE (0) or MW_FORM_TENDENCY (1), got " + std::to_string(form));
  if (check_n_in(n_in, "surrogate_prepare")) return 1;
  if (!raw_in || !raw_out || !scl_in || !scl_out || !train_x || !train_y || !val_x || !val_y || !test_x || !test_y)
    MW_FAIL("surrogate_prepare: null argument");
  if (n < 3 || n_train < 1 || n_val < 1 || n - n_train - n_val < 1) MW_FAIL("surrogate_prepare: every set needs at least one sample");
  PrepArgs a;
  memset(&a, 0, sizeof(a));
  for (int f = 0; f < n_in; f++) { a.in_min[f] = scl_in[2 * f]; a.in_rng[f] = scl_in[2 * f + 1] - scl_in[2 * f]; }
  for (int o = 0; o < 4; o++) { a.out_min[o] = scl_out[2 * o]; a.out_rng[o] = scl_out[2 * o + 1] - scl_out[2 * o]; }
  for (int f = 0; f < n_in; f++) if (!(a.in_rng[f] > 0)) MW_FAIL("surrogate_prepare: input " + std::to_string(f) + " has max <= min");
  for (int o = 0; o < 4; o++) if (!(a.out_rng[o] > 0)) MW_FAIL("surrogate_prepare: output " + std::to_string(o) + " has max <= min");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  a.n = n; a.n_train = n_train; a.n_val = n_val; a.F = make_feistel(seed, TAG_PRESHUFFLE, n);
  a.raw_in = raw_in; a.raw_out = raw_out;
  a.x[0] = train_x; a.y[0] = train_y; a.x[1] = val_x; a.y[1] = val_y; a.x[2] = test_x; a.y[2] = test_y;
  const long long blocks = std::max(1ll, std::min((n + TPB - 1) / TPB, 256ll * 16));
  const dim3 grid((unsigned)blocks), tpb(TPB);
  hipStream_t st = (hipStream_t)stream;
  if (form == MW_FORM_TENDENCY) {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_prepare<5, true>), grid, tpb, 0, st, a);
    else           hipLaunchKernelGGL((k_surrogate_prepare<9, true>), grid, tpb, 0, st, a);
  } else {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_prepare<5, false>), grid, tpb, 0, st, a);
    else           hipLaunchKernelGGL((k_surrogate_prepare<9, false>), grid, tpb, 0, st, a);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_surrogate_prepare_column(long long n, const float *col, unsigned long long seed, long long n_train, long long n_val, float *train_c,
                                float *val_c, float *test_c, void *stream) {
  if (!col || !train_c || !val_c || !test_c) MW_FAIL("surrogate_prepare_column: null argument");
  if (n < 3 || n_train < 1 || n_val < 1 || n - n_train - n_val < 1) MW_FAIL("surrogate_prepare_column: every set needs at least one sample");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  ColArgs a;
  a.n = n; a.n_train = n_train; a.n_val = n_val; a.F = make_feistel(seed, TAG_PRESHUFFLE, n);
  a.col = col; a.out[0] = train_c; a.out[1] = val_c; a.out[2] = test_c;
  const long long blocks = std::max(1ll, std::min((n + TPB - 1) / TPB, 256ll * 16));
  hipLaunchKernelGGL(k_surrogate_prepare_column, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, a);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_surrogate_prepare_v2(int n_in, long long n, const float *raw_in, const float *raw_out, const double *scl_in, const double *scl_out,
                            unsigned long long seed, long long n_train, long long n_val, float *train_x, float *train_y, float *val_x,
                            float *val_y, float *test_x, float *test_y, void *stream) {
  return mw_surrogate_prepare_form(MW_FORM_STATE, n_in, n, raw_in, raw_out, scl_in, scl_out, seed, n_train, n_val, train_x, train_y, val_x, val_y,
                                   test_x, test_y, stream);
}

int mw_surrogate_prepare(long long n, const float *raw_in, const float *raw_out, const double *scl_in, const double *scl_out,
                         unsigned long long seed, long long n_train, long long n_val, float *train_x, float *train_y, float *val_x,
                         float *val_y, float *test_x, float *test_y, void *stream) {
  return mw_surrogate_prepare_v2(5, n, raw_in, raw_out, scl_in, scl_out, seed, n_train, n_val, train_x, train_y, val_x, val_y, test_x, test_y,
                                 stream);
}

// the epoch of mw_surrogate_train_epoch_v2 (wt == nullptr) and of mw_surrogate_train_epoch_w
static int train_epoch(int n_in, int models, const float *x, const float *y, const float *wt, bool weighted, long long n, int batch, int epoch,
                       unsigned long long seed, float *params, float *m1, float *m2, const float *table, float beta1, float beta2, float eps,
                       double *stats, void *stream) {
  if (check_n_in(n_in, "surrogate_train_epoch")) return 1;
  if (!x || !y || !params || !m1 || !m2 || !table || !stats) MW_FAIL("surrogate_train_epoch: null argument");
  if (weighted && !wt) MW_FAIL("surrogate_train_epoch: null weights (the unweighted epoch is mw_surrogate_train_epoch_v2)");
  if (models < 1 || models > MW_SURROGATE_MAX_MODELS) MW_FAIL("surrogate_train_epoch: models must be in [1, " + std::to_string(MW_SURROGATE_MAX_MODELS) + "]");
  if (batch < 1 || batch > MW_SURROGATE_MAX_BATCH) MW_FAIL("surrogate_train_epoch: batch must be in [1, " + std::to_string(MW_SURROGATE_MAX_BATCH) + "]");
  if (n < 1 || epoch < 0) MW_FAIL("surrogate_train_epoch: n must be >= 1 and epoch >= 0");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  TrainArgs a;
  a.S = SetRef{x, y, n}; a.B = batch; a.epoch = epoch; a.seed = seed;
  a.params = params; a.m1 = m1; a.m2 = m2; a.table = table; a.stats = stats;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wt = wt;
  const dim3 grid((unsigned)models), tpb(TPB);
  hipStream_t st = (hipStream_t)stream;
  if (weighted) {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_train<5, true>), grid, tpb, 0, st, a);
    else           hipLaunchKernelGGL((k_surrogate_train<9, true>), grid, tpb, 0, st, a);
  } else {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_train<5, false>), grid, tpb, 0, st, a);
    else           hipLaunchKernelGGL((k_surrogate_train<9, false>), grid, tpb, 0, st, a);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_surrogate_train_epoch_v2(int n_in, int models, const float *x, const float *y, long long n, int batch, int epoch,
                                unsigned long long seed, float *params, float *m1, float *m2, const float *table, float beta1, float beta2,
                                float eps, double *stats, void *stream) {
  return train_epoch(n_in, models, x, y, nullptr, false, n, batch, epoch, seed, params, m1, m2, table, beta1, beta2, eps, stats, stream);
}

int mw_surrogate_train_epoch_w(int n_in, int models, const float *x, const float *y, const float *w, long long n, int batch, int epoch,
                               unsigned long long seed, float *params, float *m1, float *m2, const float *table, float beta1, float beta2,
                               float eps, double *stats, void *stream) {
  return train_epoch(n_in, models, x, y, w, true, n, batch, epoch, seed, params, m1, m2, table, beta1, beta2, eps, stats, stream);
}

int mw_surrogate_train_epoch(int models, const float *x, const float *y, long long n, int batch, int epoch, unsigned long long seed,
                             float *params, float *m1, float *m2, const float *table, float beta1, float beta2, float eps, double *stats,
                             void *stream) {
  return mw_surrogate_train_epoch_v2(5, models, x, y, n, batch, epoch, seed, params, m1, m2, table, beta1, beta2, eps, stats, stream);
}

static int batch_grad(int n_in, const float *params, const float *x, const float *y, const float *wt, bool weighted, int batch, float *grad,
                      float *loss, void *stream) {
  if (check_n_in(n_in, "surrogate_batch_grad")) return 1;
  if (!params || !x || !y || !grad || !loss) MW_FAIL("surrogate_batch_grad: null argument");
  if (weighted && !wt) MW_FAIL("surrogate_batch_grad: null weights (the unweighted gradient is mw_surrogate_batch_grad_v2)");
  if (batch < 1 || batch > MW_SURROGATE_MAX_BATCH) MW_FAIL("surrogate_batch_grad: batch must be in [1, " + std::to_string(MW_SURROGATE_MAX_BATCH) + "]");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const SetRef S{x, y, (long long)batch};
  hipStream_t st = (hipStream_t)stream;
  if (weighted) {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_grad<5, true>), dim3(1), dim3(TPB), 0, st, params, S, batch, grad, loss, wt);
    else           hipLaunchKernelGGL((k_surrogate_grad<9, true>), dim3(1), dim3(TPB), 0, st, params, S, batch, grad, loss, wt);
  } else {
    if (n_in == 5) hipLaunchKernelGGL((k_surrogate_grad<5, false>), dim3(1), dim3(TPB), 0, st, params, S, batch, grad, loss, wt);
    else           hipLaunchKernelGGL((k_surrogate_grad<9, false>), dim3(1), dim3(TPB), 0, st, params, S, batch, grad, loss, wt);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_surrogate_batch_grad_v2(int n_in, const float *params, const float *x, const float *y, int batch, float *grad, float *loss,
                               void *stream) {
  return batch_grad(n_in, params, x, y, nullptr, false, batch, grad, loss, stream);
}

int mw_surrogate_batch_grad_w(int n_in, const float *params, const float *x, const float *y, const float *w, int batch, float *grad,
                              float *loss, void *stream) {
  return batch_grad(n_in, params, x, y, w, true, batch, grad, loss, stream);
}

int mw_surrogate_batch_grad(const float *params, const float *x, const float *y, int batch, float *grad, float *loss, void *stream) {
  return mw_surrogate_batch_grad_v2(5, params, x, y, batch, grad, loss, stream);
}

long long mw_surrogate_errors_workspace_bytes(int nsets) { return nsets < 1 ? 0 : (long long)nsets * ERR_BLOCKS * NSTAT * (long long)sizeof(double); }

static int errors(long long n, int nsets, const float *pred, const float *y, const float *wt, bool weighted, void *workspace, double *out,
                  void *stream) {
  if (!pred || !y || !workspace || !out || (weighted && !wt)) MW_FAIL("surrogate_errors: null argument");
  if (n < 1 || nsets < 1 || nsets > 65535) MW_FAIL("surrogate_errors: n must be >= 1 and nsets in [1, 65535]");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const dim3 grid(ERR_BLOCKS, (unsigned)nsets);
  if (weighted) hipLaunchKernelGGL(k_surrogate_sums<true>, grid, dim3(TPB), 0, (hipStream_t)stream, n, pred, y, (double *)workspace, wt);
  else          hipLaunchKernelGGL(k_surrogate_sums<false>, grid, dim3(TPB), 0, (hipStream_t)stream, n, pred, y, (double *)workspace, wt);
  MW_LAUNCH_CHECK();
  const int per = 64 / NSTAT;
  hipLaunchKernelGGL(k_surrogate_sums_final, dim3((unsigned)((nsets + per - 1) / per)), dim3(64), 0, (hipStream_t)stream, nsets,
                     (const double *)workspace, out);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_surrogate_errors(long long n, int nsets, const float *pred, const float *y, void *workspace, double *out, void *stream) {
  return errors(n, nsets, pred, y, nullptr, false, workspace, out, stream);
}

int mw_surrogate_errors_weighted(long long n, int nsets, const float *pred, const float *y, const float *w, void *workspace, double *out,
                                 void *stream) {
  return errors(n, nsets, pred, y, w, true, workspace, out, stream);
}

} // extern "C"
