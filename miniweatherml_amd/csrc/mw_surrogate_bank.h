// =====================================================================================================
// mw_surrogate_bank.h -- what the units that score a bank of surrogate models share (mw_surrogate_bank.hip: mw_surrogate_eval and the
// handle; mw_surrogate_eval_domain.hip: the domain-split form): the statistics of one difference, the lane tree, the class ballot, the
// block's tail, and the handle itself.  Only inline functions, templates and plain structs: every kernel is emitted from one unit.
// =====================================================================================================
#pragma once
#include "mw_mlp_net.h"
#include <vector>

namespace mw {

constexpr int EVAL_G5 = 6, EVAL_G9 = 4;    // models per pass, single-cell / stencil: 16 accumulator registers per model + the persistence row's 16,
                                           // the largest groups that leave two waves per SIMD
constexpr int EVAL_MAX_BLOCKS = 1024;      // grid.x: grid-stride beyond 4 blocks per CU
constexpr int EVAL_ROW = 32;               // doubles per model: [class 2][field 4][statistic 4]

struct EvalFields { const double *in[5], *truth[4]; };
struct EvalAcc { double s[2][4]; };        // [class][sum d, sum |d|, sum d^2, max |d|]

// one cell of one field: d joins the sums of the cell's class (adding +0.0 elsewhere leaves a sum's bits alone)
__device__ __forceinline__ void eval_add(EvalAcc &a, double pred, double truth, bool inactive, bool active) {
#pragma clang fp contract(off)
  const double d = pred - truth;
  const double d0 = inactive ? d : 0.0, d1 = active ? d : 0.0;
  a.s[0][0] += d0; a.s[0][1] += fabs(d0); a.s[0][2] += d0 * d0; a.s[0][3] = eval_max(a.s[0][3], fabs(d0));
  a.s[1][0] += d1; a.s[1][1] += fabs(d1); a.s[1][2] += d1 * d1; a.s[1][3] = eval_max(a.s[1][3], fabs(d1));
}
__device__ __forceinline__ void eval_zero(EvalAcc &a) {
#pragma unroll
  for (int i = 0; i < 8; i++) a.s[i >> 2][i & 3] = 0.0;
}
// fixed xor tree over LANES neighbouring lanes; every lane ends with the result
template <int LANES> __device__ __forceinline__ double eval_lane_tree(double v, bool is_max) {
#pragma unroll
  for (int off = LANES / 2; off > 0; off >>= 1) { const double o = __shfl_xor(v, off, 64); v = is_max ? eval_max(v, o) : v + o; }
  return v;
}
// the class of the wave's 16 cells from the four lane groups' flags: bit c of the result = some group of cell c raised its flag
__device__ __forceinline__ bool eval_cell_active(bool flag, int cidx) {
  unsigned long long b = __ballot(flag);
  b |= b >> 32; b |= b >> 16;
  return (b >> cidx) & 1ull;
}

// the tail of both MFMA kernels: lanes -> groups of 16 -> the block's waves -> this block's row of partial sums
template <int G>
__device__ __forceinline__ void eval_block_store(EvalAcc (&acc)[G], EvalAcc &accp, long long nact, int cnt, int m0, int models,
                                                 double *__restrict__ partial, long long *__restrict__ cpartial) {
  __shared__ double red[4][4][(G + 1) * 8];
  __shared__ long long wcount[4];
  const int lane = threadIdx.x & 63, g = lane >> 4, cidx = lane & 15, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j <= G; j++) {
    EvalAcc &a = j < G ? acc[j < G ? j : 0] : accp;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const double v = eval_lane_tree<16>(a.s[i >> 2][i & 3], (i & 3) == 3);
      if (cidx == 0) red[wv][g][j * 8 + i] = v;
    }
  }
  if (lane == 0) wcount[wv] = nact;
  __syncthreads();
  for (int e = threadIdx.x; e < (G + 1) * EVAL_ROW; e += 256) {
    const int j = e >> 5, r = e & 31, c = r >> 4, v = (r >> 2) & 3, s = r & 3;
    if (j < G ? j >= cnt : blockIdx.y != 0) continue;              // the persistence row leaves from the first group's blocks
    double q = red[0][v][j * 8 + c * 4 + s];
#pragma unroll
    for (int w = 1; w < 4; w++) { const double o = red[w][v][j * 8 + c * 4 + s]; q = s == 3 ? eval_max(q, o) : q + o; }
    const int row = j < G ? m0 + j : models;
    partial[((long long)blockIdx.x * (models + 1) + row) * EVAL_ROW + r] = q;
  }
  if (threadIdx.x == 0 && blockIdx.y == 0) cpartial[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

template <int G>
__device__ __forceinline__ void eval_load_models(EvalModel (&sm)[G], const EvalModel *__restrict__ bank, int m0, int cnt) {
  const unsigned *src = (const unsigned *)(bank + m0);
  unsigned *dst = (unsigned *)sm;
  for (int i = threadIdx.x; i < cnt * (int)(sizeof(EvalModel) / 4); i += 256) dst[i] = src[i];
  __syncthreads();
}

} // namespace mw

struct mw_surrogate_bank_s {
  int n_in, models;
  mw::EvalModel *images;          // DEVICE (models): the MFMA kernels' form
  mw::StencilRef *refs;           // DEVICE (models): the strict kernel's form (n_in 5: the first 50 of W1, 5 of the scaling rows)
  double *partial;            // DEVICE (blocks, models + 1, 32), grown on demand
  long long partial_blocks;
  long long *cpartial;        // DEVICE (EVAL_MAX_BLOCKS)
  std::vector<int> forms;     // HOST (models): MW_FORM_* per model, as the images and refs carry it
  bool any_tendency;          // some model is of the tendency form: the kernels' ANYT
  // the domain-split evaluation (mw_surrogate_eval_domain.hip); all null until mw_surrogate_bank_set_domain
  double *dom_box;            // DEVICE (models, 5, 2): [lo, hi] per IN5 field
  double *dom_partial;        // DEVICE (blocks, models, 2, 64), grown on demand
  long long dom_partial_blocks;
  long long *dom_cpartial;    // DEVICE (EVAL_MAX_BLOCKS, models, 4)
};

// launches the first kernel where the condition holds, else the second (a kernel template's two instantiations, each in parentheses)
#define MW_LAUNCH_ANYT(cond, KT, KF, ...) do { if (cond) hipLaunchKernelGGL(KT, __VA_ARGS__); else hipLaunchKernelGGL(KF, __VA_ARGS__); } while (0)
