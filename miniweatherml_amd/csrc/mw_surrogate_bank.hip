// =====================================================================================================
// mw_surrogate_bank.hip -- a BANK of surrogate models on the device and the kernels that run many models over one state: in-loop
// evaluation against Kessler (mw_surrogate_eval), rollout as ensemble members (mw_surrogate_members_apply), the committee mean and spread
// (mw_surrogate_committee_apply) and its score (mw_committee_score).  A cell's arithmetic is mw_mlp_net.h's, the one definition the
// forward kernels of mw_mlp.hip call too: a model's prediction here has the bits those kernels store.
// =====================================================================================================
#include "mw_surrogate_bank.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

using namespace mw;

// =====================================================================================================
// IN-LOOP EVALUATION of a bank of models (mw_surrogate_eval): while Kessler runs the simulation, every candidate network is scored
// against what Kessler did to the state -- sum d, sum |d|, sum d^2, max |d| of d = prediction - truth per output field, separately for
// the inactive / active cells of StatisticsGatherer::is_active (gather_micro_statistics.h:61-74), plus the persistence baseline
// (prediction = input).  No prediction reaches memory.
//
// k_surrogate_eval / k_surrogate_eval_stencil are k_mlp's / k_mlp_stencil's tiles with a loop over a group of G models inside: a wave
// loads its inputs once, takes each model's A operands, biases and scaling constants from LDS and keeps 8 fp64 sums per model in
// registers (lane group g ends up holding output g, so a lane needs field g of the truth and the input field that output g replaces:
// the latter is one more load for groups 1..3, of a line another group of the same wave fetches anyway).  The class flag of a cell is
// the OR over its four lane groups: one ballot, folded by two shifts.  Per cell the arithmetic is the forward kernels' own -- the same
// functions (the reciprocal ranges come from the same device division) -- so a prediction has the bits those kernels store.
// Reduction: per lane in loop order, an xor tree over the 16 lanes of a group, the block's four waves in order, then
// k_surrogate_eval_final over the blocks in order -- no floating-point atomics.  grid.x depends on the shape alone and grid.y carries the
// groups of models, so a model's row does not depend on the size of the bank or on its place in it.
// ANYT (every kernel of this unit that runs a model): the bank holds a model of the TENDENCY form.  Then a model's form (EvalModel::form /
// StencilRef::form, uniform over the wave) picks the epilogue per model; a bank of state models alone runs the instantiation without the
// branch, which is the code these kernels had before there were two forms.  The base of the tendency form is the field output g replaces,
// which the eval kernels load anyway (`before`).
// =====================================================================================================
namespace mw {

__global__ __launch_bounds__(64) void k_surrogate_bank_recip(EvalModel *bank, int n_in) {
  if ((int)threadIdx.x < n_in) bank[blockIdx.x].in_irng[threadIdx.x] = 1.0 / bank[blockIdx.x].in_irng[threadIdx.x];   // k_mlp's `1.0 / P.in_rng[g]`
}

template <int G, int TILES, bool ANYT>
__global__ __launch_bounds__(256) void k_surrogate_eval(const EvalModel *__restrict__ bank, int models, long long ncells, EvalFields F,
                                                        double *__restrict__ partial, long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[G];
  const int m0 = blockIdx.y * G, cnt = min(G, models - m0);
  eval_load_models<G>(sm, bank, m0, cnt);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = F.in[g], *in_s = F.in[g == 0 ? 4 : g + 1], *tr_g = F.truth[g];     // in_s: rho_r for the network (group 0), else the field output g replaces
  Net5 N;                                  // (ahead of the accumulators: the order of a kernel's locals is the order in which the optimiser promotes
                                           // them to registers, and this one keeps the accumulators' registers where they were before the cell was shared)
  EvalAcc acc[G], accp;
#pragma unroll
  for (int j = 0; j < G; j++) eval_zero(acc[j]);
  eval_zero(accp);
  long long nact = 0;
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
      nact += __popcll(__ballot(ina[u] && g == 0));
      eval_add(accp, before, xt[u], inn[u], ina[u]);
    }
#pragma unroll
    for (int j = 0; j < G; j++) {
      if (j < cnt) {                                                                          // (block-uniform)
        net5_ops(N, sm[j], lane, g);
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const double y = net5_cell_form<ANYT>(N, g, xin[u], xs[u], ANYT ? sm[j].form : MW_FORM_STATE);
          eval_add(acc[j], y, xt[u], inn[u], ina[u]);
        }
      }
    }
  }
  eval_block_store<G>(acc, accp, nact, cnt, m0, models, partial, cpartial);
}

// k_mlp_stencil's sweep (a wave owns 16 columns x one z chunk at a time, top-down) with the models inside.  What that kernel carries from
// level to level as scaled floats -- the level above, the two groups' rho_r -- is carried RAW here and scaled per model with the same
// expressions: the scaling tables are the models' own.
template <int G, int U, bool ANYT>
__global__ __launch_bounds__(256) void k_surrogate_eval_stencil(const EvalModel *__restrict__ bank, int models, int nz, long long ncol, int zc,
                                                                int nchunks, EvalFields F, double *__restrict__ partial,
                                                                long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[G];
  const int m0 = blockIdx.y * G, cnt = min(G, models - m0);
  eval_load_models<G>(sm, bank, m0, cnt);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = F.in[g], *in_s = F.in[g == 0 ? 0 : g + 1], *rho_r = F.in[4], *tr_g = F.truth[g];
  Net9 N;                                                                 // (ahead of the accumulators, as in k_surrogate_eval)
  EvalAcc acc[G], accp;
#pragma unroll
  for (int j = 0; j < G; j++) eval_zero(acc[j]);
  eval_zero(accp);
  long long nact = 0;
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
        MW_EVAL_CELL_CLASS(ina[u], inn[u], lv, xt[u], xs[u], cidx)
        nact += __popcll(__ballot(ina[u] && g == 0));
        eval_add(accp, xs[u], xt[u], inn[u], ina[u]);
      }
#pragma unroll
      for (int j = 0; j < G; j++) {
        if (j < cnt) {                                                    // (block-uniform)
          net9_ops(N, sm[j], lane, g);
#pragma unroll
          for (int u = 0; u < U; u++) {
            const int k = k0 - u;
            if (k >= k_lo) {                                              // (wave-uniform)
              const f32x4 d1 = net9_layer1(N, k, net9_b0(N, xin[u]), net9_above(N, xab[u]), net9_b2(N, g, k, xrr[u]));
              const double y = net_out_form<ANYT>(N, g, d1, ANYT ? sm[j].form : MW_FORM_STATE, xs[u]);
              eval_add(acc[j], y, xt[u], inn[u], ina[u]);
            }
          }
        }
      }
    }
  }
  eval_block_store<G>(acc, accp, nact, cnt, m0, models, partial, cpartial);
}

// STRICT form: thread = cell with k_mlp_strict's / k_mlp_stencil_strict's expressions (index order, no contraction, the quotient form of the
// scaling), grid row y = one model (row `models`: persistence); the reduction scheme is the MFMA kernels'.
template <int NIN, bool ANYT>
__global__ __launch_bounds__(256) void k_surrogate_eval_strict(const StencilRef *__restrict__ bank, int models, int nz, long long ncol, EvalFields F,
                                                               double *__restrict__ partial, long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ double red[4][EVAL_ROW];
  __shared__ long long wcount[4];
  __shared__ StencilRef P;                                                // (from LDS: as scalar operands the 144 weights do not fit the SGPRs)
  const int m = blockIdx.y;
  for (int i = threadIdx.x; i < (int)(sizeof(StencilRef) / 4); i += 256) ((unsigned *)&P)[i] = ((const unsigned *)(bank + min(m, models - 1)))[i];
  __syncthreads();
  const long long n = (long long)nz * ncol;
  EvalAcc acc[4];
#pragma unroll
  for (int v = 0; v < 4; v++) eval_zero(acc[v]);
  long long nact = 0;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const StrictIn I = strict_cell_inputs<NIN>(F.in, c, nz, ncol);
    const double *in = I.v;
    const double before[4] = {in[0], in[2], in[3], in[4]};
    const double tr[4] = {F.truth[0][c], F.truth[1][c], F.truth[2][c], F.truth[3][c]};
    bool act = false;
#pragma unroll
    for (int v = 0; v < 4; v++) act = act || fabs(tr[v] - before[v]) > 1.e-10;
    double pred[4] = {before[0], before[1], before[2], before[3]};
    if (m < models) {                                                     // (block-uniform)
      MW_STRICT_CELL_FORM(NIN, P, in, ANYT && P.form != MW_FORM_STATE, pred[0], pred[1], pred[2], pred[3])
    }
#pragma unroll
    for (int v = 0; v < 4; v++) eval_add(acc[v], pred[v], tr[v], !act, act);
    nact += act ? 1 : 0;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  eval_strict_trees<EVAL_ROW>(acc, red);
  for (int off = 32; off > 0; off >>= 1) nact += __shfl_xor(nact, off, 64);
  if (lane == 0) wcount[wv] = nact;
  __syncthreads();
  eval_strict_row_store<EVAL_ROW>(red, partial + ((long long)blockIdx.x * (models + 1) + m) * EVAL_ROW);
  if (threadIdx.x == 0 && m == models) cpartial[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

// the blocks' partial rows in block order (k_surrogate_sums_final's scheme): one thread per number of `out`
__global__ __launch_bounds__(256) void k_surrogate_eval_final(int nblocks, int rows, long long ncells, const double *__restrict__ partial,
                                                              const long long *__restrict__ cpartial, double *__restrict__ out,
                                                              long long *__restrict__ counts) {
  const int e = blockIdx.x * 256 + threadIdx.x, len = rows * EVAL_ROW;
  eval_final_store(nblocks, len, e, partial, out);
  if (e == 0) {
    long long a = 0;
    for (int b = 0; b < nblocks; b++) a += cpartial[b];
    counts[0] = ncells - a; counts[1] = a;
  }
}

} // namespace mw


extern "C" void mw_surrogate_bank_destroy(mw_surrogate_bank_t b) {
  if (!b) return;
  (void)hipFree(b->images); (void)hipFree(b->refs); (void)hipFree(b->partial); (void)hipFree(b->cpartial);
  (void)hipFree(b->dom_box); (void)hipFree(b->dom_partial); (void)hipFree(b->dom_cpartial);
  delete b;
}

extern "C" int mw_surrogate_bank_create_forms(mw_surrogate_bank_t *out, int n_in, int models, const float *params, const double *scl_in,
                                              const double *scl_out, const int *forms) {
  if (!out) MW_FAIL("surrogate_bank_create: null pointer");
  *out = nullptr;
  if (n_in != 5 && n_in != 9) MW_FAIL("surrogate_bank_create: n_in must be 5 (single cell) or 9 (stencil), got " + std::to_string(n_in));
  if (models < 1 || models > MW_SURROGATE_MAX_MODELS) MW_FAIL("surrogate_bank_create: models must be in [1, " + std::to_string(MW_SURROGATE_MAX_MODELS) + "], got " + std::to_string(models));
  if (!params || !scl_in || !scl_out) MW_FAIL("surrogate_bank_create: null pointer");
  for (int m = 0; m < models; m++) {
    for (int i = 0; i < n_in; i++) if (scl_in[(m * n_in + i) * 2 + 1] == scl_in[(m * n_in + i) * 2])
      MW_FAIL("surrogate_bank_create: model " + std::to_string(m) + ", input scaling row " + std::to_string(i) + " has max == min");
    for (int i = 0; i < 4; i++) if (scl_out[(m * 4 + i) * 2 + 1] == scl_out[(m * 4 + i) * 2])
      MW_FAIL("surrogate_bank_create: model " + std::to_string(m) + ", output scaling row " + std::to_string(i) + " has max == min");
  }
  if (forms) for (int m = 0; m < models; m++) if (forms[m] != MW_FORM_STATE && forms[m] != MW_FORM_TENDENCY)
    MW_FAIL("surrogate_bank_create: model " + std::to_string(m) + ": form must be MW_FORM_STATE (0) or MW_FORM_TENDENCY (1), got " + std::to_string(forms[m]));
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const int npar = 10 * n_in + 54;
  std::vector<EvalModel> img((size_t)models);
  std::vector<StencilRef> ref((size_t)models);
  for (int m = 0; m < models; m++) {
    const float *W1 = params + (size_t)m * npar, *b1 = W1 + 10 * n_in, *W2 = b1 + 10, *b2 = W2 + 40;
    const double *si = scl_in + (size_t)m * n_in * 2, *so = scl_out + (size_t)m * 4 * 2;
    EvalModel &E = img[m];
    memset(&E, 0, sizeof(E));
    if (n_in == 5) net_dense_layer1_images(E.a1, W1, 5);
    else           net_stencil_layer1_images(E.a1, W1);
    net_layer2_images(E.c1, E.a2, E.c2, b1, W2, b2);
    fill_scaling(n_in, si, so, E.in_min, E.in_irng, E.out_min, E.out_rng);      // in_irng: the range; k_surrogate_bank_recip inverts it below
    E.form = forms ? forms[m] : MW_FORM_STATE;
    fill_ref(ref[m], n_in, W1, b1, W2, b2, si, so, E.form);
  }
  mw_surrogate_bank_t b = new mw_surrogate_bank_s();
  b->forms.assign((size_t)models, MW_FORM_STATE);
  if (forms) b->forms.assign(forms, forms + models);
  b->any_tendency = std::find(b->forms.begin(), b->forms.end(), (int)MW_FORM_TENDENCY) != b->forms.end();
  b->n_in = n_in; b->models = models; b->images = nullptr; b->refs = nullptr; b->partial = nullptr; b->partial_blocks = 0; b->cpartial = nullptr;
  b->dom_box = nullptr; b->dom_partial = nullptr; b->dom_partial_blocks = 0; b->dom_cpartial = nullptr;
  hipError_t e = hipMalloc(&b->images, sizeof(EvalModel) * (size_t)models);
  if (e == hipSuccess) e = hipMalloc(&b->refs, sizeof(StencilRef) * (size_t)models);
  if (e == hipSuccess) e = hipMalloc(&b->cpartial, sizeof(long long) * EVAL_MAX_BLOCKS);
  if (e == hipSuccess) e = hipMemcpy(b->images, img.data(), sizeof(EvalModel) * (size_t)models, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(b->refs, ref.data(), sizeof(StencilRef) * (size_t)models, hipMemcpyHostToDevice);
  if (e == hipSuccess) { hipLaunchKernelGGL(k_surrogate_bank_recip, dim3((unsigned)models), dim3(64), 0, 0, b->images, n_in); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { mw_surrogate_bank_destroy(b); MW_FAIL(std::string("surrogate_bank_create: ") + hipGetErrorString(e)); }
  *out = b;
  return 0;
}

extern "C" int mw_surrogate_bank_create(mw_surrogate_bank_t *out, int n_in, int models, const float *params, const double *scl_in,
                                        const double *scl_out) {
  return mw_surrogate_bank_create_forms(out, n_in, models, params, scl_in, scl_out, nullptr);
}

extern "C" int mw_surrogate_bank_form(mw_surrogate_bank_t b, int model) {
  if (!b) { mw::set_error("surrogate_bank_form: null handle"); return -1; }
  if (model < 0 || model >= b->models) { mw::set_error("surrogate_bank_form: model " + std::to_string(model) + " is outside the bank's [0, " + std::to_string(b->models) + ")"); return -1; }
  return b->forms[(size_t)model];
}

extern "C" int mw_surrogate_eval_group(mw_surrogate_bank_t b) {
  if (!b) { mw::set_error("surrogate_eval_group: null handle"); return 0; }
  return b->n_in == 5 ? EVAL_G5 : EVAL_G9;
}

extern "C" int mw_surrogate_eval(mw_surrogate_bank_t b, int nz, long long ncol, const double *const *in5, const double *const *truth4,
                                 double *out, long long *counts, void *stream) {
  EvalFields F;
  if (eval_fields("surrogate_eval", F, b, nz, ncol, in5, truth4, out, counts)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long ncells = (long long)nz * ncol;
  const int models = b->models, rows = models + 1;
  constexpr int TILES = EVAL_TILES, U = EVAL_U;
  const auto [blocks, zc, nchunks] = eval_grid(b->n_in, nz, ncol);
  if (eval_grow(b->partial, b->partial_blocks, blocks, (size_t)rows * EVAL_ROW)) return 1;
  if (mlp_strict()) {
    const dim3 grid((unsigned)blocks, (unsigned)rows);
    if (b->n_in == 5) MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_strict<5, true>), (k_surrogate_eval_strict<5, false>), grid, dim3(256), 0, st, b->refs, models, nz, ncol, F, b->partial, b->cpartial);
    else              MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_strict<9, true>), (k_surrogate_eval_strict<9, false>), grid, dim3(256), 0, st, b->refs, models, nz, ncol, F, b->partial, b->cpartial);
  } else {
    const int G = b->n_in == 5 ? EVAL_G5 : EVAL_G9;
    const dim3 grid((unsigned)blocks, (unsigned)((models + G - 1) / G));
    if (b->n_in == 5) MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval<EVAL_G5, TILES, true>), (k_surrogate_eval<EVAL_G5, TILES, false>), grid, dim3(256), 0, st, b->images, models, ncells, F, b->partial,
                                   b->cpartial);
    else              MW_LAUNCH_IF(b->any_tendency, (k_surrogate_eval_stencil<EVAL_G9, U, true>), (k_surrogate_eval_stencil<EVAL_G9, U, false>), grid, dim3(256), 0, st, b->images, models, nz, ncol, zc, nchunks, F,
                                   b->partial, b->cpartial);
  }
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_surrogate_eval_final, dim3((unsigned)((rows * EVAL_ROW + 255) / 256)), dim3(256), 0, st, (int)blocks, rows, ncells,
                     (const double *)b->partial, (const long long *)b->cpartial, out, counts);
  MW_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// ROLLOUT of a bank's models as ensemble members (mw_surrogate_members_apply): model j replaces temp and the three water fields of member
// members[j] of the coupler's member-fastest arrays (cell c, member e at c * nens + e) IN PLACE, from that member's own values.
//
// k_members_apply / k_members_apply_stencil are k_mlp's / k_mlp_stencil's tiles on that layout: the 16 cells of a tile belong to ONE
// member (the A operands are one model's), a wave owns (a group of tiles, one model), and the waves of a workgroup take consecutive models
// of the SAME cells -- their strided accesses touch the same lines, which so come from HBM once and from L1 / L2 afterwards (the idea of
// the dycore's members-in-one-workgroup launches).  A model's operands, biases and scaling are read from the bank's image in LDS, as in
// k_surrogate_eval, and a cell's arithmetic is the forward kernels' (mw_mlp_net.h): the same bits.
// In place: a single-cell tile is loaded whole before its MFMAs, which join all its lanes, so no store precedes a load of its cells.  The
// stencil wave sweeps its columns top-down in ONE chunk and carries the level above in registers (k_mlp_stencil's own scheme): level k is
// loaded before level k is stored, and nobody else reads it -- the result is the out-of-place one without a copy of any level.
// =====================================================================================================
namespace mw {

constexpr int APPLY_MAX_MEMBERS = 32;      // members a call can address (the dycore steps at most MW_ROLLOUT_MAX_MEMBERS = 30)
constexpr int APPLY_MAX_BLOCKS = 256 * 16; // grid.x: grid-stride beyond 16 blocks per CU
struct ApplyMap { int member[APPLY_MAX_MEMBERS]; };
struct ApplyFields { double *f[5]; };      // temp, density_dry, water_vapor, cloud_liquid, precip_liquid (density_dry is only read)

// wave -> (model, tile slot) of a workgroup: mpb models per workgroup (1, 2 or 4), 4 / mpb tile slots
__host__ __device__ __forceinline__ int apply_mpb(int models) { return models >= 3 ? 4 : models; }
__device__ __forceinline__ void apply_slot(int models, int &j, int &slot, int &slots) {
  const int mpb = apply_mpb(models), wv = threadIdx.x >> 6;
  slots = 4 / mpb;
  j = blockIdx.y * mpb + (wv % mpb);
  slot = wv / mpb;
}

// ANYT and a model of the tendency form: lane group g > 0 also loads the field its output replaces -- the one it stores to -- in the register
// that only group 0 uses for rho_r (stencil: one more register per level), with the tile's other loads and ahead of its stores.
template <int TILES, bool ANYT>
__global__ __launch_bounds__(256) void k_members_apply(const EvalModel *__restrict__ bank, int models, ApplyMap map, long long ncells, int nens,
                                                       ApplyFields F) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[4];
  const int mpb = apply_mpb(models), m0 = blockIdx.y * mpb, cnt = min(mpb, models - m0);
  eval_load_models<4>(sm, bank, m0, cnt);
  int j, slot, slots;
  apply_slot(models, j, slot, slots);
  if (j >= models) return;                                                // (wave-uniform, after the barrier)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const int e = map.member[j];
  const int form = ANYT ? sm[j - m0].form : MW_FORM_STATE;               // (wave-uniform)
  const bool tend = ANYT && form != MW_FORM_STATE;
  const bool loadb = tend && !MW_TENDENCY_ROTATE_APPLY;                         // the base of groups 1..3 by a load (else, tend: by the rotate)
  const double *in_g = F.f[g], *rho_r = F.f[(loadb && g != 0) ? g + 1 : 4];  // (loadb: group g > 0 reads its base here)
  double *out_g = F.f[g == 0 ? 0 : g + 1];
  Net5 N;
  net5_ops(N, sm[j - m0], lane, g);
  const long long ntiles = (ncells + 15) / 16;
  for (long long t0 = ((long long)blockIdx.x * slots + slot) * TILES; t0 < ntiles; t0 += (long long)gridDim.x * slots * TILES) {
    double xin[TILES], xin4[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      const bool ok = cell < ncells;
      xin[u]  = ok ? in_g[cell * nens + e] : N.imin;
      xin4[u] = (ok && (loadb || g == 0)) ? rho_r[cell * nens + e] : N.imin4;
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      if (tend && !loadb) xin4[u] = net5_rotate_base(g, xin[u], xin4[u]);    // (wave-uniform: every lane calls it)
      const double y = net5_cell_form<ANYT>(N, g, xin[u], xin4[u], form);
      if (cell < ncells) out_g[cell * nens + e] = y;
    }
  }
}

// k_mlp_stencil's sweep with one chunk per column: a wave owns 16 columns of one member, all nz levels
template <int U, bool ANYT>
__global__ __launch_bounds__(256) void k_members_apply_stencil(const EvalModel *__restrict__ bank, int models, ApplyMap map, int nz, long long ncol,
                                                               int nens, ApplyFields F) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[4];
  const int mpb = apply_mpb(models), m0 = blockIdx.y * mpb, cnt = min(mpb, models - m0);
  eval_load_models<4>(sm, bank, m0, cnt);
  int j, slot, slots;
  apply_slot(models, j, slot, slots);
  if (j >= models) return;                                                // (wave-uniform, after the barrier)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const int e = map.member[j];
  const int form = ANYT ? sm[j - m0].form : MW_FORM_STATE;               // (wave-uniform)
  const bool tend = ANYT && form != MW_FORM_STATE;
  const double *in_g = F.f[g], *rho_r = F.f[4];
  double *out_g = F.f[g == 0 ? 0 : g + 1];
  Net9 N;
  net9_ops(N, sm[j - m0], lane, g);
  const long long ntiles = (ncol + 15) / 16, lev = ncol * nens;           // lev: doubles from level k to level k + 1
  for (long long t = (long long)blockIdx.x * slots + slot; t < ntiles; t += (long long)gridDim.x * slots) {
    const long long col = t * 16 + cidx;
    const bool ok = col < ncol;
    const long long base = col * nens + e;
    const int k_hi = nz - 1;
    float above = 0.f;                    // the model top is its own level above
    double rr_raw = N.rmin;
    if (ok) {
      above = net9_above(N, in_g[(long long)k_hi * lev + base]);
      if (g == ((k_hi & 1) ^ 1)) rr_raw = rho_r[(long long)k_hi * lev + base];
    }
    for (int k0 = k_hi; k0 >= 0; k0 -= U) {
      double xin[U], xrr[U], xs[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        const bool lv = ok && k >= 0;
        xin[u] = lv ? in_g[(long long)k * lev + base] : N.imin;
        xrr[u] = (lv && g == (k & 1)) ? rho_r[(long long)k * lev + base] : N.rmin;
        if (ANYT) xs[u] = (lv && tend && g != 0) ? out_g[(long long)k * lev + base] : xin[u];      // level k's own value of the field output g replaces
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        if (k >= 0) {                                                     // (wave-uniform)
          if (g == (k & 1)) rr_raw = xrr[u];
          const f32x4 d1 = net9_layer1(N, k, net9_b0(N, xin[u]), above, net9_b2(N, g, k, rr_raw));
          above = net9_above(N, xin[u]);                                  // level k is level k - 1's level above
          const double y = net_out_form<ANYT>(N, g, d1, form, ANYT ? xs[u] : 0.0);
          if (ok) out_g[(long long)k * lev + base] = y;
        }
      }
    }
  }
}

// STRICT form: thread = one column of one member, swept top-down with the level above in registers (in place for the same reason);
// k_mlp_strict's / k_mlp_stencil_strict's expressions, grid row y = one model, its weights from LDS as in k_surrogate_eval_strict.
template <int NIN, bool ANYT>
__global__ __launch_bounds__(256) void k_members_apply_strict(const StencilRef *__restrict__ bank, ApplyMap map, int nz, long long ncol, int nens,
                                                              ApplyFields F) {
#pragma clang fp contract(off)
  __shared__ StencilRef P;
  for (int i = threadIdx.x; i < (int)(sizeof(StencilRef) / 4); i += 256) ((unsigned *)&P)[i] = ((const unsigned *)(bank + blockIdx.y))[i];
  __syncthreads();
  const int e = map.member[blockIdx.y];
  const long long lev = ncol * nens;
  for (long long col = (long long)blockIdx.x * 256 + threadIdx.x; col < ncol; col += (long long)gridDim.x * 256) {
    const long long base = col * nens + e;
    double ab[4];                                                         // temp, rho_v, rho_c, rho_r of level min(nz - 1, k + 1) as they were
    for (int k = nz - 1; k >= 0; k--) {
      const long long c = (long long)k * lev + base;
      const StrictIn I = strict_column_inputs<NIN>(ab, F.f, c, k == nz - 1);
      const double *in = I.v;
      MW_STRICT_CELL_FORM(NIN, P, in, ANYT && P.form != MW_FORM_STATE, F.f[0][c], F.f[2][c], F.f[3][c], F.f[4][c])
    }
  }
}

} // namespace mw

extern "C" int mw_surrogate_members_apply(mw_surrogate_bank_t b, const int *members, int nz, long long ncol, int nens, double *const *fields5,
                                          void *stream) {
  if (!b || !members || !fields5) MW_FAIL("surrogate_members_apply: null pointer");
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL("surrogate_members_apply: nz, ncol and nens must be >= 1");
  const int models = b->models;
  if (models > APPLY_MAX_MEMBERS) MW_FAIL("surrogate_members_apply: the bank has " + std::to_string(models) + " models, at most " +
                                          std::to_string(APPLY_MAX_MEMBERS) + " can be members of one call");
  ApplyMap map;
  memset(&map, 0, sizeof(map));
  for (int j = 0; j < models; j++) {
    if (members[j] < 0 || members[j] >= nens) MW_FAIL("surrogate_members_apply: member " + std::to_string(members[j]) + " of model " + std::to_string(j) +
                                                      " is outside [0, " + std::to_string(nens) + ")");
    for (int i = 0; i < j; i++) if (members[i] == members[j]) MW_FAIL("surrogate_members_apply: member " + std::to_string(members[j]) + " is given to two models");
    map.member[j] = members[j];
  }
  ApplyFields F;
  for (int i = 0; i < 5; i++) { if (!fields5[i]) MW_FAIL("surrogate_members_apply: null field"); F.f[i] = fields5[i]; }
  if ((double)nz * (double)ncol * (double)nens > 9.0e18) MW_FAIL("surrogate_members_apply: the fields are too large");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long ncells = (long long)nz * ncol;
  if (mlp_strict()) {
    const long long blocks = std::max<long long>(1, std::min<long long>((ncol + 255) / 256, APPLY_MAX_BLOCKS));
    const dim3 grid((unsigned)blocks, (unsigned)models);
    if (b->n_in == 5) MW_LAUNCH_IF(b->any_tendency, (k_members_apply_strict<5, true>), (k_members_apply_strict<5, false>), grid, dim3(256), 0, st, b->refs, map, nz, ncol, nens, F);
    else              MW_LAUNCH_IF(b->any_tendency, (k_members_apply_strict<9, true>), (k_members_apply_strict<9, false>), grid, dim3(256), 0, st, b->refs, map, nz, ncol, nens, F);
    MW_LAUNCH_CHECK();
    return 0;
  }
  constexpr int TILES = 4, U = 4;
  const int mpb = apply_mpb(models), slots = 4 / mpb;
  const unsigned gy = (unsigned)((models + mpb - 1) / mpb);
  if (b->n_in == 5) {
    const long long groups = ((ncells + 15) / 16 + TILES - 1) / TILES;
    const long long blocks = std::max<long long>(1, std::min<long long>((groups + slots - 1) / slots, APPLY_MAX_BLOCKS));
    MW_LAUNCH_IF(b->any_tendency, (k_members_apply<TILES, true>), (k_members_apply<TILES, false>), dim3((unsigned)blocks, gy), dim3(256), 0, st, b->images, models, map, ncells, nens, F);
  } else {
    const long long tiles = (ncol + 15) / 16;
    const long long blocks = std::max<long long>(1, std::min<long long>((tiles + slots - 1) / slots, APPLY_MAX_BLOCKS));
    MW_LAUNCH_IF(b->any_tendency, (k_members_apply_stencil<U, true>), (k_members_apply_stencil<U, false>), dim3((unsigned)blocks, gy), dim3(256), 0, st, b->images, models, map, nz, ncol, nens, F);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// COMMITTEE of a bank's models (mw_surrogate_committee_apply): the mean of n <= MW_COMMITTEE_MAX_MODELS selected models and their spread,
// one pass over the state whatever n is.  For a cell and an output field, y_j is what the forward kernels store for model sel[j] (per
// model scaling, un-scaling and clip included); mean = (((y_0 + y_1) + y_2) + ...) / (double)n in the order of sel, range = hi - lo with the
// NaN-propagating extrema of eval_max.  All n models sit in LDS once per workgroup (16 x sizeof(EvalModel) = 33,280 B) and the loop over
// models is INSIDE the cell / level loop: a lane keeps sum, hi, lo of its (cell, field) in registers.
//
// k_committee_apply / k_committee_apply_stencil are k_members_apply's / k_members_apply_stencil's tiles on one member of the member-fastest
// layout, with the models inside as in k_surrogate_eval*: what the stencil kernel carries from level to level is carried RAW and scaled per
// model.  A tile (stencil: a level of the wave's columns) is loaded whole before it is stored and nobody else reads it, so an output may be
// its own input field.
// =====================================================================================================
namespace mw {

constexpr int COMMITTEE_MAX = MW_COMMITTEE_MAX_MODELS;
struct CommitteeSel { int n; int model[COMMITTEE_MAX]; };
struct CommitteeFields { const double *in[5]; double *out[4]; double *range[4]; };   // range[*]: all null or all set

template <typename T>
__device__ __forceinline__ void committee_load(T *sm, const T *__restrict__ bank, const CommitteeSel &S) {
  constexpr int W = (int)(sizeof(T) / 4);
  for (int i = threadIdx.x; i < S.n * W; i += 256) ((unsigned *)sm)[i] = ((const unsigned *)(bank + S.model[i / W]))[i % W];
  __syncthreads();
}

// ANYT (some selected model is of the tendency form): the base is loaded once per cell, raw, for all models (k_members_apply's scheme)
template <int TILES, bool ANYT>
__global__ __launch_bounds__(256) void k_committee_apply(const EvalModel *__restrict__ bank, CommitteeSel S, int member, long long ncells, int nens,
                                                         CommitteeFields F) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[COMMITTEE_MAX];
  committee_load(sm, bank, S);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = F.in[g], *rho_r = F.in[(ANYT && g != 0) ? g + 1 : 4];   // (ANYT: group g > 0 reads its base here)
  double *out_g = F.out[g], *rng_g = F.range[g];
  const double dn = (double)S.n;
  const long long ntiles = (ncells + 15) / 16;
  for (long long t0 = wave * TILES; t0 < ntiles; t0 += nwaves * TILES) {
    double xin[TILES], xin4[TILES], sum[TILES], hi[TILES], lo[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      const bool ok = cell < ncells;
      xin[u]  = ok ? in_g[cell * nens + member] : 0.0;
      xin4[u] = (ok && (ANYT || g == 0)) ? rho_r[cell * nens + member] : 0.0;
      sum[u] = hi[u] = lo[u] = 0.0;
    }
    for (int j = 0; j < S.n; j++) {
      Net5 N;
      net5_ops(N, sm[j], lane, g);
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const double y = net5_cell_form<ANYT>(N, g, xin[u], xin4[u], ANYT ? sm[j].form : MW_FORM_STATE);
        sum[u] = j == 0 ? y : sum[u] + y;                                   // (the first addend as it is: a committee of one keeps its bits)
        hi[u]  = j == 0 ? y : eval_max(hi[u], y);
        lo[u]  = j == 0 ? y : eval_min(lo[u], y);
      }
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      if (cell < ncells) {
        out_g[cell * nens + member] = sum[u] / dn;
        if (rng_g) rng_g[cell * nens + member] = hi[u] - lo[u];
      }
    }
  }
}

// k_members_apply_stencil's sweep (a wave owns 16 columns of the member, all nz levels, top-down) with the models inside
template <int U, bool ANYT>
__global__ __launch_bounds__(256) void k_committee_apply_stencil(const EvalModel *__restrict__ bank, CommitteeSel S, int member, int nz, long long ncol,
                                                                 int nens, CommitteeFields F) {
#pragma clang fp contract(off)
  __shared__ EvalModel sm[COMMITTEE_MAX];
  committee_load(sm, bank, S);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = F.in[g], *rho_r = F.in[4], *in_s = F.in[g == 0 ? 0 : g + 1];
  double *out_g = F.out[g], *rng_g = F.range[g];
  const double dn = (double)S.n;
  const long long ntiles = (ncol + 15) / 16, lev = ncol * nens;           // lev: doubles from level k to level k + 1
  for (long long t = wave; t < ntiles; t += nwaves) {
    const long long col = t * 16 + cidx;
    const bool ok = col < ncol;
    const long long base = col * nens + member;
    const int k_hi = nz - 1;
    double above = 0.0, rr = 0.0;                                         // raw: the level above of this lane's field, this group's latest rho_r
    MW_SWEEP_TOP(above, rr, in_g, rho_r, (long long)k_hi * lev + base, ok, g, k_hi)      // the model top is its own level above
    for (int k0 = k_hi; k0 >= 0; k0 -= U) {
      double xin[U], xab[U], xrr[U], xs[U], sum[U], hi[U], lo[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        const bool lv = ok && k >= 0;
        MW_SWEEP_LEVEL(xin[u], xrr[u], xs[u], in_g, rho_r, in_s, (long long)k * lev + base, lv, g, k)
        sum[u] = hi[u] = lo[u] = 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        if (k >= 0) MW_SWEEP_CARRY(g, k, xin[u], xrr[u], xab[u], rr, above)           // (wave-uniform)
        else xab[u] = 0.0;
      }
      for (int j = 0; j < S.n; j++) {
        Net9 N;
        net9_ops(N, sm[j], lane, g);
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int k = k0 - u;
          if (k >= 0) {                                                   // (wave-uniform)
            const f32x4 d1 = net9_layer1(N, k, net9_b0(N, xin[u]), net9_above(N, xab[u]), net9_b2(N, g, k, xrr[u]));
            const double y = net_out_form<ANYT>(N, g, d1, ANYT ? sm[j].form : MW_FORM_STATE, ANYT ? xs[u] : 0.0);
            sum[u] = j == 0 ? y : sum[u] + y;
            hi[u]  = j == 0 ? y : eval_max(hi[u], y);
            lo[u]  = j == 0 ? y : eval_min(lo[u], y);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = k0 - u;
        if (ok && k >= 0) {
          out_g[(long long)k * lev + base] = sum[u] / dn;
          if (rng_g) rng_g[(long long)k * lev + base] = hi[u] - lo[u];
        }
      }
    }
  }
}

// STRICT form: thread = one column of the member, swept top-down with the level above in registers (k_members_apply_strict), the models
// inside the level loop, their weights from LDS; k_mlp_strict's / k_mlp_stencil_strict's expressions.
template <int NIN, bool ANYT>
__global__ __launch_bounds__(256) void k_committee_apply_strict(const StencilRef *__restrict__ bank, CommitteeSel S, int member, int nz, long long ncol,
                                                                int nens, CommitteeFields F) {
#pragma clang fp contract(off)
  __shared__ StencilRef sm[COMMITTEE_MAX];
  committee_load(sm, bank, S);
  const long long lev = ncol * nens;
  const double dn = (double)S.n;
  for (long long col = (long long)blockIdx.x * 256 + threadIdx.x; col < ncol; col += (long long)gridDim.x * 256) {
    const long long base = col * nens + member;
    double ab[4];                                                         // temp, rho_v, rho_c, rho_r of level min(nz - 1, k + 1) as they were
    for (int k = nz - 1; k >= 0; k--) {
      const long long c = (long long)k * lev + base;
      const StrictIn I = strict_column_inputs<NIN>(ab, F.in, c, k == nz - 1);
      const double *in = I.v;
      double sum[4], hi[4], lo[4];
      for (int j = 0; j < S.n; j++) {
        double p[4];
        MW_STRICT_CELL_FORM(NIN, sm[j], in, ANYT && sm[j].form != MW_FORM_STATE, p[0], p[1], p[2], p[3])
#pragma unroll
        for (int v = 0; v < 4; v++) {
          sum[v] = j == 0 ? p[v] : sum[v] + p[v];
          hi[v]  = j == 0 ? p[v] : eval_max(hi[v], p[v]);
          lo[v]  = j == 0 ? p[v] : eval_min(lo[v], p[v]);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; v++) {
        F.out[v][c] = sum[v] / dn;
        if (F.range[v]) F.range[v][c] = hi[v] - lo[v];
      }
    }
  }
}

// ---- scoring a committee (mw_committee_score): d = pred - truth and r = range per class and field ----
constexpr int SCORE_STATS = 7;                       // sum d, sum |d|, sum d^2, max |d|, sum r, sum r^2, sum r |d|
constexpr int SCORE_ROW = 2 * 4 * SCORE_STATS;       // doubles of a result: [class][field][statistic]
constexpr int SCORE_CNT = 9;                         // int64 per block: active cells, then covered [class][field]
constexpr int SCORE_MAX_BLOCKS = 1024;
struct ScoreFields { const double *in[5], *truth[4], *pred[4], *range[4]; };

__global__ __launch_bounds__(256) void k_committee_score(long long n, ScoreFields F, double *__restrict__ partial, long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ double red[4][SCORE_ROW];
  __shared__ long long cred[4][SCORE_CNT];
  double acc[2][4][SCORE_STATS];
  long long cnt[SCORE_CNT];
#pragma unroll
  for (int i = 0; i < SCORE_ROW; i++) (&acc[0][0][0])[i] = 0.0;
#pragma unroll
  for (int i = 0; i < SCORE_CNT; i++) cnt[i] = 0;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const double before[4] = {F.in[0][c], F.in[2][c], F.in[3][c], F.in[4][c]};
    double tr[4];
    bool act = false;
#pragma unroll
    for (int v = 0; v < 4; v++) { tr[v] = F.truth[v][c]; act = act || fabs(tr[v] - before[v]) > 1.e-10; }      // gather_micro_statistics.h:61-74
    cnt[0] += act ? 1 : 0;
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const double d = F.pred[v][c] - tr[v], r = F.range[v][c];
      const bool cov = fabs(d) <= r;
#pragma unroll
      for (int cl = 0; cl < 2; cl++) {                                     // adding +0.0 to the other class leaves its bits alone (eval_add)
        const bool in = cl == (act ? 1 : 0);
        const double dc = in ? d : 0.0, rc = in ? r : 0.0, ad = fabs(dc);
        double *a = acc[cl][v];
        a[0] += dc; a[1] += ad; a[2] += dc * dc; a[3] = eval_max(a[3], ad);
        a[4] += rc; a[5] += rc * rc; a[6] += rc * ad;
        cnt[1 + cl * 4 + v] += (in && cov) ? 1 : 0;
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < SCORE_ROW; i++) {
    const double q = eval_lane_tree<64>((&acc[0][0][0])[i], i % SCORE_STATS == 3);
    if (lane == 0) red[wv][i] = q;
  }
#pragma unroll
  for (int i = 0; i < SCORE_CNT; i++) {
    long long q = cnt[i];
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) cred[wv][i] = q;
  }
  __syncthreads();
  if (threadIdx.x < SCORE_ROW) {
    const int i = threadIdx.x;
    double q = red[0][i];
#pragma unroll
    for (int w = 1; w < 4; w++) q = i % SCORE_STATS == 3 ? eval_max(q, red[w][i]) : q + red[w][i];
    partial[(long long)blockIdx.x * SCORE_ROW + i] = q;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 64 + SCORE_CNT) {
    const int i = threadIdx.x - 64;
    cpartial[(long long)blockIdx.x * SCORE_CNT + i] = cred[0][i] + cred[1][i] + cred[2][i] + cred[3][i];
  }
}

// the blocks' partial rows in block order (k_surrogate_eval_final's scheme)
__global__ __launch_bounds__(64) void k_committee_score_final(int nblocks, long long n, const double *__restrict__ partial,
                                                              const long long *__restrict__ cpartial, double *__restrict__ out,
                                                              long long *__restrict__ counts) {
  const int e = threadIdx.x;
  if (e < SCORE_ROW) {
    double q = 0.0;
    for (int b = 0; b < nblocks; b++) {
      const double o = partial[(long long)b * SCORE_ROW + e];
      q = e % SCORE_STATS == 3 ? eval_max(q, o) : q + o;
    }
    out[e] = q;
  }
  if (e < SCORE_CNT) {
    long long a = 0;
    for (int b = 0; b < nblocks; b++) a += cpartial[(long long)b * SCORE_CNT + e];
    if (e == 0) { counts[0] = n - a; counts[1] = a; }
    else counts[1 + e] = a;
  }
}

} // namespace mw

static bool committee_overlap(const double *a, const double *b, long long n) { return a < b + n && b < a + n; }

extern "C" int mw_surrogate_committee_apply(mw_surrogate_bank_t b, int n_sel, const int *sel, int member, int nz, long long ncol, int nens,
                                            const double *const *in5, double *const *out4, double *const *range4, void *stream) {
  if (!b || !sel || !in5 || !out4) MW_FAIL("surrogate_committee_apply: null pointer");
  if (n_sel < 1 || n_sel > MW_COMMITTEE_MAX_MODELS) MW_FAIL("surrogate_committee_apply: a committee has 1 to " + std::to_string(MW_COMMITTEE_MAX_MODELS) +
                                                            " models, got " + std::to_string(n_sel));
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL("surrogate_committee_apply: nz, ncol and nens must be >= 1");
  if (member < 0 || member >= nens) MW_FAIL("surrogate_committee_apply: member " + std::to_string(member) + " is outside [0, " + std::to_string(nens) + ")");
  CommitteeSel S;
  memset(&S, 0, sizeof(S));
  S.n = n_sel;
  for (int j = 0; j < n_sel; j++) {
    if (sel[j] < 0 || sel[j] >= b->models) MW_FAIL("surrogate_committee_apply: model " + std::to_string(sel[j]) + " is outside the bank's [0, " +
                                                   std::to_string(b->models) + ")");
    for (int i = 0; i < j; i++) if (sel[i] == sel[j]) MW_FAIL("surrogate_committee_apply: model " + std::to_string(sel[j]) + " is given twice");
    S.model[j] = sel[j];
  }
  if ((double)nz * (double)ncol * (double)nens > 9.0e18) MW_FAIL("surrogate_committee_apply: the fields are too large");
  const long long total = (long long)nz * ncol * nens;
  CommitteeFields F;
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL("surrogate_committee_apply: null field"); F.in[i] = in5[i]; }
  for (int v = 0; v < 4; v++) { if (!out4[v]) MW_FAIL("surrogate_committee_apply: null field"); F.out[v] = out4[v]; F.range[v] = nullptr; }
  if (range4) for (int v = 0; v < 4; v++) { if (!range4[v]) MW_FAIL("surrogate_committee_apply: null field"); F.range[v] = range4[v]; }
  // an output is its own input field (in place) or overlaps no input; outputs and ranges overlap nothing else
  const int own[4] = {0, 2, 3, 4};
  for (int v = 0; v < 4; v++) {
    for (int i = 0; i < 5; i++) {
      if (!(F.out[v] == F.in[i] && i == own[v]) && committee_overlap(F.out[v], F.in[i], total)) MW_FAIL("surrogate_committee_apply: an output must be its own input field (in place) or overlap no input");
      if (F.range[v] && committee_overlap(F.range[v], F.in[i], total)) MW_FAIL("surrogate_committee_apply: a range field must not overlap an input");
    }
    for (int w = 0; w < 4; w++) {
      if (w != v && committee_overlap(F.out[v], F.out[w], total)) MW_FAIL("surrogate_committee_apply: the outputs must not overlap each other");
      if (F.range[v] && committee_overlap(F.range[v], F.out[w], total)) MW_FAIL("surrogate_committee_apply: a range field must not overlap an output");
      if (F.range[v] && w != v && committee_overlap(F.range[v], F.range[w], total)) MW_FAIL("surrogate_committee_apply: the range fields must not overlap each other");
    }
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long ncells = (long long)nz * ncol;
  bool anyt = false;                                                       // ANYT of this call: a selected model of the tendency form
  for (int j = 0; j < n_sel; j++) anyt = anyt || b->forms[(size_t)sel[j]] != MW_FORM_STATE;
  if (mlp_strict()) {
    const long long blocks = std::max<long long>(1, std::min<long long>((ncol + 255) / 256, APPLY_MAX_BLOCKS));
    if (b->n_in == 5) MW_LAUNCH_IF(anyt, (k_committee_apply_strict<5, true>), (k_committee_apply_strict<5, false>), dim3((unsigned)blocks), dim3(256), 0, st, b->refs, S, member, nz, ncol, nens, F);
    else              MW_LAUNCH_IF(anyt, (k_committee_apply_strict<9, true>), (k_committee_apply_strict<9, false>), dim3((unsigned)blocks), dim3(256), 0, st, b->refs, S, member, nz, ncol, nens, F);
    MW_LAUNCH_CHECK();
    return 0;
  }
  constexpr int TILES = 4, U = 4;
  if (b->n_in == 5) {
    const long long groups = ((ncells + 15) / 16 + TILES - 1) / TILES;
    const long long blocks = std::max<long long>(1, std::min<long long>((groups + 3) / 4, APPLY_MAX_BLOCKS));
    MW_LAUNCH_IF(anyt, (k_committee_apply<TILES, true>), (k_committee_apply<TILES, false>), dim3((unsigned)blocks), dim3(256), 0, st, b->images, S, member, ncells, nens, F);
  } else {
    const long long tiles = (ncol + 15) / 16;
    const long long blocks = std::max<long long>(1, std::min<long long>((tiles + 3) / 4, APPLY_MAX_BLOCKS));
    MW_LAUNCH_IF(anyt, (k_committee_apply_stencil<U, true>), (k_committee_apply_stencil<U, false>), dim3((unsigned)blocks), dim3(256), 0, st, b->images, S, member, nz, ncol, nens, F);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

static long long committee_score_blocks(int nz, long long ncol) {
  if (nz < 1 || ncol < 1 || (double)nz * (double)ncol > 9.0e18) return 0;
  return std::max<long long>(1, std::min<long long>(((long long)nz * ncol + 255) / 256, SCORE_MAX_BLOCKS));
}

extern "C" long long mw_committee_score_workspace_bytes(int nz, long long ncol) {
  return committee_score_blocks(nz, ncol) * (long long)(SCORE_ROW * sizeof(double) + SCORE_CNT * sizeof(long long));
}

extern "C" int mw_committee_score(int nz, long long ncol, const double *const *in5, const double *const *truth4, const double *const *pred4,
                                  const double *const *range4, void *workspace, double *out, long long *counts, void *stream) {
  if (!in5 || !truth4 || !pred4 || !range4 || !workspace || !out || !counts) MW_FAIL("committee_score: null pointer");
  const long long blocks = committee_score_blocks(nz, ncol);
  if (blocks < 1) MW_FAIL("committee_score: nz and ncol must be >= 1");
  ScoreFields F;
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL("committee_score: null field"); F.in[i] = in5[i]; }
  for (int v = 0; v < 4; v++) {
    if (!truth4[v] || !pred4[v] || !range4[v]) MW_FAIL("committee_score: null field");
    F.truth[v] = truth4[v]; F.pred[v] = pred4[v]; F.range[v] = range4[v];
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)nz * ncol;
  double *partial = (double *)workspace;
  long long *cpartial = (long long *)(partial + blocks * SCORE_ROW);
  hipLaunchKernelGGL(k_committee_score, dim3((unsigned)blocks), dim3(256), 0, st, n, F, partial, cpartial);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_committee_score_final, dim3(1), dim3(64), 0, st, (int)blocks, n, (const double *)partial, (const long long *)cpartial, out, counts);
  MW_LAUNCH_CHECK();
  return 0;
}
