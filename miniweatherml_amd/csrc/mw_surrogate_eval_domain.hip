// =====================================================================================================
// mw_surrogate_eval_domain.hip -- mw_surrogate_eval with every model's errors SPLIT by whether the cell lies inside or outside that model's
// training box: per model, for the prediction and for the persistence baseline, the statistics of eval_add in four
// classes, side {inside, outside} x {inactive, active}.  A cell is outside for model m iff some tested value x fails lo <= x && x <= hi
// against m's row of the box (mw_member_domain's rule: NaN is outside, a bound is inside); the tested values are the cell's five inputs
// and, for a bank of width 9, temp and the three water fields of the level above against the same rows (the top level is its own level
// above: mw_member_sample_mask_domain's `above` rule).
//
// The kernels are mw_surrogate_bank.hip's three with the same tile walk, per-lane loop order, lane trees, wave and block order -- so with a
// box nothing leaves, a model's inside rows are mw_surrogate_eval's bits.  What differs:
//   - the side of a cell per model: every lane tests the raw values it holds anyway against the model's rows, read from LDS next to the
//     model's image; one ballot folded as in eval_cell_active gives the cell's bit.  The state is read once per pass as before.
//   - a model's accumulators are 16 doubles per lane, not 8, and the persistence baseline is per model too (the sides are per model), so it
//     no longer rides along with the predictions: the NET = false instantiation of each MFMA kernel scores `before` for DOM_GP5 / DOM_GP9 models per
//     pass without a network, and carries the integer counts.  The strict kernel gives both kinds a grid row of their own.
//   - counts are ballots: per block the active cells and, per model and class, the outside cells; the final kernel derives the inside ones.
// No floating-point atomics; nothing is written to the fields.
// =====================================================================================================
#include "mw_surrogate_bank.h"
#include <algorithm>
#include <cmath>
#include <string>

using namespace mw;

namespace mw {

// models per pass: predictions of the single-cell / stencil kernel, persistence rows of either -- the largest groups that leave two waves
// per SIMD without a spill (32 accumulator registers per model and kind; DESIGN.md 13.12 has the table)
constexpr int DOM_G5 = 4, DOM_G9 = 2, DOM_GP5 = 5, DOM_GP9 = 4;
constexpr int DOM_ROW = 64;                // doubles per (model, kind): [side 2][class 2][field 4][statistic 4]

struct DomAcc { double s[4][4]; };         // [side * 2 + class][sum d, sum |d|, sum d^2, max |d|]

// eval_add with the side: d joins the sums of the cell's (side, class); the other three receive +0.0
__device__ __forceinline__ void dom_add(DomAcc &a, double pred, double truth, bool inactive, bool active, bool outside) {
#pragma clang fp contract(off)
  const double d = pred - truth;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const bool mine = ((c >> 1) ? outside : !outside) && ((c & 1) ? active : inactive);
    const double dc = mine ? d : 0.0;
    a.s[c][0] += dc; a.s[c][1] += fabs(dc); a.s[c][2] += dc * dc; a.s[c][3] = eval_max(a.s[c][3], fabs(dc));
  }
}
__device__ __forceinline__ void dom_zero(DomAcc &a) {
#pragma unroll
  for (int i = 0; i < 16; i++) a.s[i >> 2][i & 3] = 0.0;
}
// mw_member_domain's test of one value against one row
__device__ __forceinline__ bool dom_fails(double x, double lo, double hi) { return !(lo <= x && x <= hi); }

// the boxes of a block's models into LDS (the caller's barrier follows)
template <int G> __device__ __forceinline__ void dom_load_boxes(double (&sbox)[G][5][2], const double *__restrict__ box, int m0, int cnt) {
  for (int i = threadIdx.x; i < cnt * 10; i += 256) (&sbox[0][0][0])[i] = box[(long long)m0 * 10 + i];
}

// the tail of both MFMA kernels (eval_block_store's scheme): lanes -> groups of 16 -> the block's waves -> this block's rows.
// nout[j][c]: this lane's outside cells of model j and class c, nact: its active cells (both only where COUNTS; group 0 counts, a lane
// sees far fewer than 2^32 cells).
template <int G, bool COUNTS>
__device__ __forceinline__ void dom_block_store(DomAcc (&acc)[G], const unsigned (&nout)[G][2], unsigned nact, int cnt, int m0, int models,
                                                int kind, double *__restrict__ partial, long long *__restrict__ cpartial) {
  __shared__ double red[4][4][G * 16];
  __shared__ long long wcount[4][1 + 2 * G];
  const int lane = threadIdx.x & 63, g = lane >> 4, cidx = lane & 15, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < G; j++) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const double v = eval_lane_tree<16>(acc[j].s[i >> 2][i & 3], (i & 3) == 3);
      if (cidx == 0) red[wv][g][j * 16 + i] = v;
    }
  }
  if (COUNTS) {
#pragma unroll
    for (int e = 0; e < 1 + 2 * G; e++) {
      long long q = e == 0 ? nact : nout[e == 0 ? 0 : (e - 1) >> 1][(e - 1) & 1];
      for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
      if (lane == 0) wcount[wv][e] = q;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < G * DOM_ROW; e += 256) {
    const int j = e >> 6, r = e & 63, c = r >> 4, v = (r >> 2) & 3, s = r & 3;
    if (j >= cnt) continue;
    double q = red[0][v][j * 16 + c * 4 + s];
#pragma unroll
    for (int w = 1; w < 4; w++) { const double o = red[w][v][j * 16 + c * 4 + s]; q = s == 3 ? eval_max(q, o) : q + o; }
    partial[(((long long)blockIdx.x * models + (m0 + j)) * 2 + kind) * DOM_ROW + r] = q;
  }
  if (COUNTS && (int)threadIdx.x < 1 + 2 * G) {
    const int e = threadIdx.x;
    const long long q = wcount[0][e] + wcount[1][e] + wcount[2][e] + wcount[3][e];
    long long *row = cpartial + (long long)blockIdx.x * (1 + 2 * models);
    if (e == 0) { if (blockIdx.y == 0) row[0] = q; }
    else if ((e - 1) >> 1 < cnt) row[1 + 2 * m0 + (e - 1)] = q;
  }
}

// k_surrogate_eval's tiles.  NET: the predictions of G models (kind 0); else `before` as the prediction of G models (kind 1) and the counts.
// Group g of a cell holds in[g] and in_s (rho_r in group 0, else in[g + 1]): together the cell's five inputs.
template <int G, int TILES, bool ANYT, bool NET>
__global__ __launch_bounds__(256) void k_surrogate_eval_domain(const EvalModel *__restrict__ bank, const double *__restrict__ box, int models,
                                                               long long ncells, EvalFields F, double *__restrict__ partial,
                                                               long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[NET ? G : 1];
  __shared__ double sbox[G][5][2];
  const int m0 = blockIdx.y * G, cnt = min(G, models - m0);
  dom_load_boxes<G>(sbox, box, m0, cnt);
  if constexpr (NET) eval_load_models<G>(sm, bank, m0, cnt); else __syncthreads();
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const int rs = g == 0 ? 4 : g + 1;                                       // the box row of in_s
  const double *in_g = F.in[g], *in_s = F.in[rs], *tr_g = F.truth[g];
  Net5 N;
  DomAcc acc[G];
#pragma unroll
  for (int j = 0; j < G; j++) dom_zero(acc[j]);
  unsigned nact = 0, nout[G][2];
#pragma unroll
  for (int j = 0; j < G; j++) nout[j][0] = nout[j][1] = 0;
  const long long ntiles = (ncells + 15) / 16;
  for (long long t0 = wave * TILES; t0 < ntiles; t0 += nwaves * TILES) {
    double xin[TILES], xs[TILES], xt[TILES];
    bool ina[TILES], inn[TILES];
    MW_EVAL_TILE_LOAD(TILES, xin, xs, xt, in_g, in_s, tr_g, t0, cidx, ncells)
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const bool ok = (t0 + u) * 16 + cidx < ncells;
      const double before = g == 0 ? xin[u] : xs[u];
      MW_EVAL_CELL_CLASS(ina[u], inn[u], ok, xt[u], before, cidx)
      if (!NET) nact += (ina[u] && g == 0) ? 1u : 0u;
    }
#pragma unroll
    for (int j = 0; j < G; j++) {
      if (j < cnt) {                                                                          // (block-uniform)
        if constexpr (NET) net5_ops(N, sm[j], lane, g);
        const double lo0 = sbox[j][g][0], hi0 = sbox[j][g][1], lo1 = sbox[j][rs][0], hi1 = sbox[j][rs][1];
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const bool ok = ina[u] || inn[u];
          const bool outside = eval_cell_active(ok && (dom_fails(xin[u], lo0, hi0) || dom_fails(xs[u], lo1, hi1)), cidx);
          double y;
          if constexpr (NET) y = net5_cell_form<ANYT>(N, g, xin[u], xs[u], ANYT ? sm[j].form : MW_FORM_STATE);
          else {
            y = g == 0 ? xin[u] : xs[u];
            nout[j][0] += (inn[u] && outside && g == 0) ? 1u : 0u;
            nout[j][1] += (ina[u] && outside && g == 0) ? 1u : 0u;
          }
          dom_add(acc[j], y, xt[u], inn[u], ina[u], outside);
        }
      }
    }
  }
  dom_block_store<G, !NET>(acc, nout, nact, cnt, m0, models, NET ? 0 : 1, partial, cpartial);
}

// k_surrogate_eval_stencil's sweep.  At level k group g holds field g of level k (xin) and of the level above (xab: an input of the network
// for groups 0, 2, 3 -- temp, water_vapor, cloud_liquid), and of groups 0 / 1 the one with g == (k & 1) holds rho_r of level k, the other
// rho_r of the level above (xrr): the nine inputs, each tested against the row of its IN5 field.
template <int G, int U, bool ANYT, bool NET>
__global__ __launch_bounds__(256) void k_surrogate_eval_domain_stencil(const EvalModel *__restrict__ bank, const double *__restrict__ box, int models,
                                                                       int nz, long long ncol, int zc, int nchunks, EvalFields F,
                                                                       double *__restrict__ partial, long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[NET ? G : 1];
  __shared__ double sbox[G][5][2];
  const int m0 = blockIdx.y * G, cnt = min(G, models - m0);
  dom_load_boxes<G>(sbox, box, m0, cnt);
  if constexpr (NET) eval_load_models<G>(sm, bank, m0, cnt); else __syncthreads();
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = F.in[g], *in_s = F.in[g == 0 ? 0 : g + 1], *rho_r = F.in[4], *tr_g = F.truth[g];
  Net9 N;
  DomAcc acc[G];
#pragma unroll
  for (int j = 0; j < G; j++) dom_zero(acc[j]);
  unsigned nact = 0, nout[G][2];
#pragma unroll
  for (int j = 0; j < G; j++) nout[j][0] = nout[j][1] = 0;
  const long long items = ((ncol + 15) / 16) * nchunks;                   // (16-column tile, z chunk): k_mlp_stencil's wave index
  for (long long item = wave; item < items; item += nwaves) {
    const int chunk = (int)(item % nchunks);
    const long long col = (item / nchunks) * 16 + cidx;
    const bool ok = col < ncol;
    const int k_lo = chunk * zc, k_hi = min(nz, k_lo + zc) - 1, k_top = min(nz - 1, k_hi + 1);
    double above = 0.0, rr = 0.0;                                         // raw: the level above of this lane's field, this group's latest rho_r
    MW_SWEEP_TOP(above, rr, in_g, rho_r, (long long)k_top * ncol + col, ok, g, k_hi)
    for (int k0 = k_hi; k0 >= k_lo; k0 -= U) {
      double xin[U], xab[U], xrr[U], xs[U], xt[U];
      bool ina[U], inn[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        const bool lv = ok && k >= k_lo;
        const long long idx = (long long)k * ncol + col;
        MW_SWEEP_LEVEL(xin[u], xrr[u], xs[u], in_g, rho_r, in_s, idx, lv, g, k)
        xt[u]  = lv ? tr_g[idx] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        const bool lv = ok && k >= k_lo;
        if (k >= k_lo) MW_SWEEP_CARRY(g, k, xin[u], xrr[u], xab[u], rr, above)        // (wave-uniform)
        else xab[u] = 0.0;
        MW_EVAL_CELL_CLASS(ina[u], inn[u], lv, xt[u], xs[u], cidx)
        if (!NET) nact += (ina[u] && g == 0) ? 1u : 0u;
      }
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (j < cnt) {                                                    // (block-uniform)
          if constexpr (NET) net9_ops(N, sm[j], lane, g);
          const double lo0 = sbox[j][g][0], hi0 = sbox[j][g][1], lo4 = sbox[j][4][0], hi4 = sbox[j][4][1];
#pragma unroll
          for (int u = 0; u < U; u++) {
            const int k = k0 - u;
            if (k >= k_lo) {                                              // (wave-uniform)
              const bool lv = ina[u] || inn[u];
              const bool bad = dom_fails(xin[u], lo0, hi0) || (g != 1 && dom_fails(xab[u], lo0, hi0)) || (g < 2 && dom_fails(xrr[u], lo4, hi4));
              const bool outside = eval_cell_active(lv && bad, cidx);
              double y;
              if constexpr (NET) {
                const f32x4 d1 = net9_layer1(N, k, net9_b0(N, xin[u]), net9_above(N, xab[u]), net9_b2(N, g, k, xrr[u]));
                y = net_out_form<ANYT>(N, g, d1, ANYT ? sm[j].form : MW_FORM_STATE, xs[u]);
              } else {
                y = xs[u];
                nout[j][0] += (inn[u] && outside && g == 0) ? 1u : 0u;
                nout[j][1] += (ina[u] && outside && g == 0) ? 1u : 0u;
              }
              dom_add(acc[j], y, xt[u], inn[u], ina[u], outside);
            }
          }
        }
      }
    }
  }
  dom_block_store<G, !NET>(acc, nout, nact, cnt, m0, models, NET ? 0 : 1, partial, cpartial);
}

// STRICT form: k_surrogate_eval_strict's thread = cell; grid row y = (model y >> 1, kind y & 1).  The persistence rows carry the counts.
template <int NIN, bool ANYT>
__global__ __launch_bounds__(256) void k_surrogate_eval_domain_strict(const StencilRef *__restrict__ bank, const double *__restrict__ box, int models,
                                                                      int nz, long long ncol, EvalFields F, double *__restrict__ partial,
                                                                      long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ double red[4][DOM_ROW];
  __shared__ long long wcount[4][3];
  __shared__ double sbox[5][2];
  __shared__ StencilRef P;                                                // (from LDS: as scalar operands the 144 weights do not fit the SGPRs)
  const int m = blockIdx.y >> 1, kind = blockIdx.y & 1;
  for (int i = threadIdx.x; i < (int)(sizeof(StencilRef) / 4); i += 256) ((unsigned *)&P)[i] = ((const unsigned *)(bank + m))[i];
  if (threadIdx.x < 10) (&sbox[0][0])[threadIdx.x] = box[(long long)m * 10 + threadIdx.x];
  __syncthreads();
  const long long n = (long long)nz * ncol;
  DomAcc acc[4];
#pragma unroll
  for (int v = 0; v < 4; v++) dom_zero(acc[v]);
  long long nact = 0, nout0 = 0, nout1 = 0;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const StrictIn I = strict_cell_inputs<NIN>(F.in, c, nz, ncol);
    const double *in = I.v;
    const double before[4] = {in[0], in[2], in[3], in[4]};
    const double tr[4] = {F.truth[0][c], F.truth[1][c], F.truth[2][c], F.truth[3][c]};
    bool act = false, outside = false;
#pragma unroll
    for (int v = 0; v < 4; v++) act = act || fabs(tr[v] - before[v]) > 1.e-10;
#pragma unroll
    for (int f = 0; f < 5; f++) outside = outside || dom_fails(in[f], sbox[f][0], sbox[f][1]);
    if (NIN == 9) {
      outside = outside || dom_fails(in[5], sbox[0][0], sbox[0][1]) || dom_fails(in[6], sbox[2][0], sbox[2][1]) ||
                dom_fails(in[7], sbox[3][0], sbox[3][1]) || dom_fails(in[8], sbox[4][0], sbox[4][1]);
    }
    double pred[4] = {before[0], before[1], before[2], before[3]};
    if (kind == 0) {                                                      // (block-uniform)
      MW_STRICT_CELL_FORM(NIN, P, in, ANYT && P.form != MW_FORM_STATE, pred[0], pred[1], pred[2], pred[3])
    }
#pragma unroll
    for (int v = 0; v < 4; v++) dom_add(acc[v], pred[v], tr[v], !act, act, outside);
    nact += act ? 1 : 0;
    nout0 += (outside && !act) ? 1 : 0;
    nout1 += (outside && act) ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  eval_strict_trees<DOM_ROW>(acc, red);
  for (int off = 32; off > 0; off >>= 1) {
    nact += __shfl_xor(nact, off, 64); nout0 += __shfl_xor(nout0, off, 64); nout1 += __shfl_xor(nout1, off, 64);
  }
  if (lane == 0) { wcount[wv][0] = nact; wcount[wv][1] = nout0; wcount[wv][2] = nout1; }
  __syncthreads();
  eval_strict_row_store<DOM_ROW>(red, partial + (((long long)blockIdx.x * models + m) * 2 + kind) * DOM_ROW);
  if (kind == 1 && threadIdx.x < 3) {
    const int e = threadIdx.x;
    const long long q = wcount[0][e] + wcount[1][e] + wcount[2][e] + wcount[3][e];
    long long *row = cpartial + (long long)blockIdx.x * (1 + 2 * models);
    if (e == 0) { if (m == 0) row[0] = q; }
    else row[2 * m + e] = q;
  }
}

// the blocks' partial rows in block order (k_surrogate_eval_final's scheme): one thread per number of `out`; the inside counts are what the
// outside ones leave of the class
__global__ __launch_bounds__(256) void k_surrogate_eval_domain_final(int nblocks, int models, long long ncells, const double *__restrict__ partial,
                                                                     const long long *__restrict__ cpartial, double *__restrict__ out,
                                                                     long long *__restrict__ counts) {
  const int e = blockIdx.x * 256 + threadIdx.x, len = models * 2 * DOM_ROW;
  eval_final_store(nblocks, len, e, partial, out);
  if (e < models * 2) {
    const int m = e >> 1, c = e & 1, w = 1 + 2 * models;
    long long a = 0, o = 0;
    for (int b = 0; b < nblocks; b++) { a += cpartial[(long long)b * w]; o += cpartial[(long long)b * w + 1 + e]; }
    counts[m * 4 + 2 + c] = o;
    counts[m * 4 + c] = (c ? a : ncells - a) - o;
  }
}

} // namespace mw

extern "C" int mw_surrogate_bank_set_domain(mw_surrogate_bank_t b, const double *box) {
  if (!b || !box) MW_FAIL("surrogate_bank_set_domain: null pointer");
  for (int m = 0; m < b->models; m++)
    for (int f = 0; f < 5; f++) {
      const double lo = box[(m * 5 + f) * 2], hi = box[(m * 5 + f) * 2 + 1];
      if (!(lo <= hi)) MW_FAIL("surrogate_bank_set_domain: the box of model " + std::to_string(m) + ", field " + std::to_string(f) +
                               ", is not lo <= hi (NaN is refused, +-inf is allowed)");
    }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  MW_HIP(hipDeviceSynchronize());                                         // a call that reads the boxes being replaced has finished
  if (!b->dom_cpartial) MW_HIP(hipMalloc(&b->dom_cpartial, sizeof(long long) * EVAL_MAX_BLOCKS * (size_t)(1 + 2 * b->models)));
  double *dbox = b->dom_box;
  if (!dbox) MW_HIP(hipMalloc(&dbox, sizeof(double) * 10 * (size_t)b->models));
  const hipError_t e = hipMemcpy(dbox, box, sizeof(double) * 10 * (size_t)b->models, hipMemcpyHostToDevice);
  if (e != hipSuccess) { if (!b->dom_box) (void)hipFree(dbox); MW_FAIL(std::string("surrogate_bank_set_domain: ") + hipGetErrorString(e)); }
  b->dom_box = dbox;
  MW_HIP(hipDeviceSynchronize());
  return 0;
}

extern "C" int mw_surrogate_eval_domain_group(mw_surrogate_bank_t b) {
  if (!b) { mw::set_error("surrogate_eval_domain_group: null handle"); return 0; }
  return b->n_in == 5 ? DOM_G5 : DOM_G9;
}

extern "C" int mw_surrogate_eval_domain(mw_surrogate_bank_t b, int nz, long long ncol, const double *const *in5, const double *const *truth4,
                                        double *out, long long *counts, void *stream) {
  EvalFields F;
  if (eval_fields("surrogate_eval_domain", F, b, nz, ncol, in5, truth4, out, counts)) return 1;
  if (!b->dom_box) MW_FAIL("surrogate_eval_domain: the bank has no boxes (mw_surrogate_bank_set_domain comes first)");
  hipStream_t st = (hipStream_t)stream;
  const long long ncells = (long long)nz * ncol;
  const int models = b->models;
  constexpr int TILES = EVAL_TILES, U = EVAL_U;
  const auto [blocks, zc, nchunks] = eval_grid(b->n_in, nz, ncol);        // mw_surrogate_eval's grid.x
  if (eval_grow(b->dom_partial, b->dom_partial_blocks, blocks, (size_t)models * 2 * DOM_ROW)) return 1;
  const double *box = b->dom_box;
  if (mlp_strict()) {
    const dim3 grid((unsigned)blocks, (unsigned)(2 * models));
    if (b->n_in == 5) MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_domain_strict<5, true>), (k_surrogate_eval_domain_strict<5, false>), grid, dim3(256), 0, st, b->refs, box, models, nz, ncol, F, b->dom_partial, b->dom_cpartial);
    else              MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_domain_strict<9, true>), (k_surrogate_eval_domain_strict<9, false>), grid, dim3(256), 0, st, b->refs, box, models, nz, ncol, F, b->dom_partial, b->dom_cpartial);
    MW_LAUNCH_CHECK();
  } else {
    const int G = b->n_in == 5 ? DOM_G5 : DOM_G9;
    const int GP = b->n_in == 5 ? DOM_GP5 : DOM_GP9;
    const dim3 grid((unsigned)blocks, (unsigned)((models + G - 1) / G)), gridp((unsigned)blocks, (unsigned)((models + GP - 1) / GP));
    if (b->n_in == 5) {
      MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_domain<DOM_G5, TILES, true, true>), (k_surrogate_eval_domain<DOM_G5, TILES, false, true>), grid, dim3(256), 0, st, b->images, box, models, ncells, F,
                   b->dom_partial, b->dom_cpartial);
      MW_LAUNCH_CHECK();
      hipLaunchKernelGGL((k_surrogate_eval_domain<DOM_GP5, TILES, false, false>), gridp, dim3(256), 0, st, b->images, box, models, ncells, F, b->dom_partial, b->dom_cpartial);
    } else {
      MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_domain_stencil<DOM_G9, U, true, true>), (k_surrogate_eval_domain_stencil<DOM_G9, U, false, true>), grid, dim3(256), 0, st, b->images, box, models, nz, ncol,
                   zc, nchunks, F, b->dom_partial, b->dom_cpartial);
      MW_LAUNCH_CHECK();
      hipLaunchKernelGGL((k_surrogate_eval_domain_stencil<DOM_GP9, U, false, false>), gridp, dim3(256), 0, st, b->images, box, models, nz, ncol, zc, nchunks, F, b->dom_partial,
                         b->dom_cpartial);
    }
    MW_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_surrogate_eval_domain_final, dim3((unsigned)((models * 2 * DOM_ROW + 255) / 256)), dim3(256), 0, st, (int)blocks, models, ncells,
                     (const double *)b->dom_partial, (const long long *)b->dom_cpartial, out, counts);
  MW_LAUNCH_CHECK();
  return 0;
}
