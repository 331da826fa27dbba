// =====================================================================================================
// mw_surrogate_bank.h -- what the units that score a bank of surrogate models share (mw_surrogate_bank.hip: mw_surrogate_eval and the
// handle; mw_surrogate_eval_domain.hip: the domain-split form): the statistics of one difference, the lane tree, the class ballot, the
// block's tail, the walks around the cell (tile load, raw stencil sweep, strict gathers and tails), the entry points' set-up, and the
// handle itself.  Only inline functions, templates, macros and plain structs: every kernel is emitted from one unit.
// =====================================================================================================
#pragma once
#include "mw_mlp_net.h"
#include <algorithm>
#include <string>
#include <vector>

namespace mw {

constexpr int EVAL_G5 = 6, EVAL_G9 = 4;    // models per pass, single-cell / stencil: 16 accumulator registers per model + the persistence row's 16,
                                           // the largest groups that leave two waves per SIMD
constexpr int EVAL_MAX_BLOCKS = 1024;      // grid.x: grid-stride beyond 4 blocks per CU
constexpr int EVAL_ROW = 32;               // doubles per model: [class 2][field 4][statistic 4]
constexpr int EVAL_TILES = 4, EVAL_U = 4;  // tiles per wave and pass of the single-cell kernels, levels per pass of the stencil sweeps

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

// ---- the walks around the cell that the MFMA kernels share.  MACROS, expanded in place, for MW_STRICT_CELL's reason:
// whatever reorders these kernels' statements on their way through the optimiser changes their code, and a function does -- the carry
// step's three assignments as an inline function gave seven kernels another instruction stream.  The arguments are the caller's own
// arrays, lvalues and expressions; an element offset (top, idx) is the caller's, in its own layout. ----
// a dense eval tile: per cell field g, the lane group's in_s and field g of the truth (u: the macro's own)
#define MW_EVAL_TILE_LOAD(TILES, xin, xs, xt, in_g, in_s, tr_g, t0, cidx, ncells)                                               \
  _Pragma("unroll")                                                                                                             \
  for (int u = 0; u < TILES; u++) {                                                                                             \
    const long long cell = ((t0) + u) * 16 + (cidx);                                                                            \
    const bool ok = cell < (ncells);                                                                                            \
    (xin)[u] = ok ? (in_g)[cell] : 0.0;                                                                                         \
    (xs)[u]  = ok ? (in_s)[cell] : 0.0;                                                                                         \
    (xt)[u]  = ok ? (tr_g)[cell] : 0.0;                                                                                         \
  }
// the class of a cell (of a dense tile or a sweep level): active where some output field moved (gather_micro_statistics.h:61-74),
// neither where the lane holds no cell
#define MW_EVAL_CELL_CLASS(ina, inn, ok, truth, before, cidx)                                                                   \
  {                                                                                                                             \
    const bool act_ = eval_cell_active((ok) && fabs((truth) - (before)) > 1.e-10, cidx);                                        \
    (ina) = (ok) && act_; (inn) = (ok) && !act_;                                                                                \
  }
// The RAW stencil sweep of a kernel that loops over models: a lane carries the level above of its own field and its group's latest rho_r
// unscaled (above, rr: zero so far), and every model scales them with its own tables.  The chunk's top -- `top`: level min(nz - 1, k_hi + 1)
#define MW_SWEEP_TOP(above, rr, in_g, rho_r, top, ok, g, k_hi)                                                                  \
  if (ok) {                                                                                                                     \
    (above) = (in_g)[top];                                                                                                      \
    if ((g) == (((k_hi) & 1) ^ 1)) (rr) = (rho_r)[top];                                                                         \
  }
// level k at idx: field g, rho_r in group k & 1, and the level's own value of the field output g replaces (group 0: temp, which it holds;
// unused, and so not loaded, in a kernel that runs no tendency model)
#define MW_SWEEP_LEVEL(xin, xrr, xs, in_g, rho_r, in_s, idx, lv, g, k)                                                          \
  {                                                                                                                             \
    (xin) = (lv) ? (in_g)[idx] : 0.0;                                                                                           \
    (xrr) = ((lv) && (g) == ((k) & 1)) ? (rho_r)[idx] : 0.0;                                                                    \
    (xs)  = ((lv) && (g) != 0) ? (in_s)[idx] : (xin);                                                                           \
  }
// level k joins what the lane carries: xrr becomes the group's latest rho_r, xab the level above; level k is level k - 1's level above
#define MW_SWEEP_CARRY(g, k, xin, xrr, xab, rr, above)                                                                          \
  {                                                                                                                             \
    if ((g) == ((k) & 1)) (rr) = (xrr);                                                                                         \
    (xrr) = (rr); (xab) = (above); (above) = (xin);                                                                             \
  }

// ---- the strict kernels' gathers: the nine features of MW_STRICT_CELL (NIN == 5: the last four stay zero), returned BY VALUE (filled
// through a reference, the column gather changed the registers of k_members_apply_strict<9> and k_committee_apply_strict<9>) ----
struct StrictIn { double v[9]; };
// thread = cell c of level-major fields: the level above is level min(nz - 1, k + 1) of the same column
template <int NIN>
__device__ __forceinline__ StrictIn strict_cell_inputs(const double *const (&f)[5], long long c, int nz, long long ncol) {
  const long long k = c / ncol;
  const long long ca = (k + 1 < nz) ? c + ncol : c;
  StrictIn I = {{f[0][c], f[1][c], f[2][c], f[3][c], f[4][c], 0.0, 0.0, 0.0, 0.0}};
  if (NIN == 9) { I.v[5] = f[0][ca]; I.v[6] = f[2][ca]; I.v[7] = f[3][ca]; I.v[8] = f[4][ca]; }
  return I;
}
// thread = column, swept top-down and in place: ab carries temp, rho_v, rho_c, rho_r of the level above AS THEY WERE (top: the column's
// top level is its own level above)
template <int NIN, typename T>
__device__ __forceinline__ StrictIn strict_column_inputs(double (&ab)[4], T *const (&f)[5], long long c, bool top) {
  StrictIn I = {{f[0][c], f[1][c], f[2][c], f[3][c], f[4][c], 0.0, 0.0, 0.0, 0.0}};
  double *in = I.v;
  if (top) { ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4]; }
  if (NIN == 9) { in[5] = ab[0]; in[6] = ab[1]; in[7] = ab[2]; in[8] = ab[3]; }
  ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4];
  return I;
}

// The double part of a strict eval kernel's tail, in two halves: the kernel's counts go to LDS between them, ahead of its barrier (as one
// function behind the counts, k_surrogate_eval_domain_strict<5, true> took two more AGPRs).  Before the barrier: number r =
// [class][field][statistic] of the thread's ROW doubles goes down the 64-lane tree into the wave's row of `red`.
template <int ROW, typename ACC>
__device__ __forceinline__ void eval_strict_trees(const ACC (&acc)[4], double (&red)[4][ROW]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < ROW; r++) {
    const double q = eval_lane_tree<64>(acc[(r >> 2) & 3].s[r >> 4][r & 3], (r & 3) == 3);
    if (lane == 0) red[wv][r] = q;
  }
}
// after it: thread r joins the four waves in order and stores the block's number r to row[r]
template <int ROW>
__device__ __forceinline__ void eval_strict_row_store(const double (&red)[4][ROW], double *__restrict__ row) {
  if (threadIdx.x < ROW) {
    const int r = threadIdx.x;
    double q = red[0][r];
#pragma unroll
    for (int w = 1; w < 4; w++) q = (r & 3) == 3 ? eval_max(q, red[w][r]) : q + red[w][r];
    row[r] = q;
  }
}

// number e of a final kernel's `out`: the blocks' partial rows (len doubles each) in block order; every fourth statistic is a maximum.
// (The bounds test is in here: with it in the kernel the loop's exit test came out inverted.)
__device__ __forceinline__ void eval_final_store(int nblocks, int len, int e, const double *__restrict__ partial, double *__restrict__ out) {
  if (e < len) {
    double q = 0.0;
    for (int b = 0; b < nblocks; b++) {
      const double o = partial[(long long)b * len + e];
      q = (e & 3) == 3 ? eval_max(q, o) : q + o;
    }
    out[e] = q;
  }
}

template <int G>
__device__ __forceinline__ void eval_load_models(EvalModel (&sm)[G], const EvalModel *__restrict__ bank, int m0, int cnt) {
  const unsigned *src = (const unsigned *)(bank + m0);
  unsigned *dst = (unsigned *)sm;
  for (int i = threadIdx.x; i < cnt * (int)(sizeof(EvalModel) / 4); i += 256) dst[i] = src[i];
  __syncthreads();
}

// ---- host set-up that mw_surrogate_eval and mw_surrogate_eval_domain share ----
// the entry points' argument checks, in the caller's name `who`, and the kernels' field table
inline int eval_fields(const char *who, EvalFields &F, mw_surrogate_bank_t b, int nz, long long ncol, const double *const *in5,
                       const double *const *truth4, const double *out, const long long *counts) {
  if (!b || !in5 || !truth4 || !out || !counts) MW_FAIL(std::string(who) + ": null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL(std::string(who) + ": nz and ncol must be >= 1");
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL(std::string(who) + ": null field"); F.in[i] = in5[i]; }
  for (int i = 0; i < 4; i++) { if (!truth4[i]) MW_FAIL(std::string(who) + ": null field"); F.truth[i] = truth4[i]; }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");      // (a handle exists only with a device)
  return 0;
}

// grid.x from the shape alone (a model's partial sums do not depend on how many models share the call), and the stencil sweep's z chunks
struct EvalGrid { long long blocks; int zc, nchunks; };
inline EvalGrid eval_grid(int n_in, int nz, long long ncol) {
  const long long ncells = (long long)nz * ncol;
  EvalGrid g;
  g.zc = mw_mlp_stencil_chunk(nz, ncol); g.nchunks = (nz + g.zc - 1) / g.zc;
  if (mlp_strict()) g.blocks = (ncells + 255) / 256;
  else if (n_in == 5) g.blocks = (((ncells + 15) / 16 + EVAL_TILES - 1) / EVAL_TILES + 3) / 4;
  else g.blocks = (((ncol + 15) / 16) * g.nchunks + 3) / 4;
  g.blocks = std::max<long long>(1, std::min<long long>(g.blocks, EVAL_MAX_BLOCKS));
  return g;
}

// a device buffer of `per_block` doubles per block of grid.x, grown on demand: `have` is the blocks it holds
inline int eval_grow(double *&buf, long long &have, long long blocks, size_t per_block) {
  if (blocks <= have) return 0;
  (void)hipFree(buf); buf = nullptr; have = 0;
  MW_HIP(hipMalloc(&buf, sizeof(double) * (size_t)blocks * per_block));
  have = blocks;
  return 0;
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
