// =====================================================================================================
// mw_stack_eval.hip -- a GROUP of dense surrogate stacks (mw_mlp_stack.h) scored against the truth fields in the running simulation:
// mw_surrogate_eval's 32 numbers per stack ([inactive, active][field][sum d, sum |d|, sum d^2, max |d|], d = prediction - truth), the
// persistence row and the class counts, in one call for 1 .. 32 stacks of any mix of shapes, widths and forms (mw_stack_group_eval).
// No prediction reaches memory and nothing is written to the nine fields.  DESIGN.md 13.21.
//
// k_stack_eval<N9, ANYT>: one launch per list of the group (n_in = 5: flat 16-cell tiles, four per pass; n_in = 9: 16 columns top-down,
// four levels per pass, the level above carried raw -- k_stack_members' two walks at contiguous addresses).  A 256-thread workgroup holds
// mpb = 4, 2 or 1 consecutive stacks' images in dynamic LDS and a wave scores ONE stack, so its accumulators are one EvalAcc (16 VGPRs)
// for its lane group's field.  The waves of a workgroup work on the same cells at the same time: the nine fields' lines come from HBM
// once per workgroup.  Per cell a lane loads three values: field g for the network, field g of the truth, and in_s -- rho_r in group 0
// (the network's fifth feature), else the input field that output g replaces (the class flag).  The prediction is stack_cells', the
// function k_stack_members calls: the bits mw_mlp_stack_forward stores out of place.
//
// A ROW DOES NOT DEPEND ON THE GROUP.  Every block has four tile slots whatever mpb is: slot s of block b walks the items (tile quads;
// column tiles) (4 b + s) + i * 4 gridDim.x, and grid.x is a function of (nz, ncol) alone.  With mpb = 1 the four waves take one slot
// each; with mpb = 2 (4) a wave takes its two (all four) slots one after the other.  Behind each slot the wave sends its sums down
// eval_lane_tree<16> into red[stack][slot] and zeroes them; the block's tail joins slots 0..3 in order and stores the block's row; the
// final kernel joins the blocks in order.  No floating-point atomics, eval_max (NaN-propagating) for every maximum.
//
// k_stack_eval_persist: the persistence row (prediction = input) and the count of active cells, once per call, on the flat walk with the
// same slot deal and tail -- it keeps 16 more accumulator registers and the count ballots out of the MFMA kernel.
// k_stack_eval_strict (mw_mlp_set_strict(1)): thread = cell, grid row y = stack, k_mlp_stack_strict's index-order loops on the parameters
// as they came; the tail is the strict bank kernels' (eval_strict_trees / eval_strict_row_store).
// =====================================================================================================
#include "mw_mlp_stack.h"
#include "mw_surrogate_bank.h"                                      // EvalAcc, eval_add, the lane tree, the class ballot, the strict tails, eval_final_store
#include <cstring>
#include <string>

namespace mw {

constexpr int SE_TILES = 4;                                         // tiles (n_in = 9: levels) per wave and pass
constexpr int SE_SLOTS = 4;                                         // tile slots of a block, whatever mpb is

// one slot's sums of one wave: lanes -> groups of 16 -> red[slot][group][8]; the accumulators start the next slot from zero
__device__ __forceinline__ void stack_eval_slot_store(EvalAcc &acc, double (&red)[SE_SLOTS][4][8], int slot, int g, int cidx) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const double v = eval_lane_tree<16>(acc.s[i >> 2][i & 3], (i & 3) == 3);
    if (cidx == 0) red[slot][g][i] = v;
  }
  eval_zero(acc);
}
// number r = [class][field][statistic] of a block's row: the four slots in order
__device__ __forceinline__ double stack_eval_slot_join(const double (&red)[SE_SLOTS][4][8], int r) {
  const int c = r >> 4, v = (r >> 2) & 3, s = r & 3;
  double q = red[0][v][c * 4 + s];
#pragma unroll
  for (int sl = 1; sl < SE_SLOTS; sl++) { const double o = red[sl][v][c * 4 + s]; q = s == 3 ? eval_max(q, o) : q + o; }
  return q;
}

// rows: the list's rows (n_in = 5 or 9 alone), `models` of them.  partial: (gridDim.x, models, 32), the list's own.  ANYT: the list holds
// a stack of the tendency form (then a wave's form picks the epilogue, wave-uniformly).
template <bool N9, bool ANYT>
__global__ __launch_bounds__(256, 2) void k_stack_eval(const StackRow *__restrict__ rows, const float *__restrict__ imgs, int models, int mpb, int nz,
                                                    long long ncol, EvalFields F, double *__restrict__ partial) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ double red[4][SE_SLOTS][4][8];                               // [stack of the block][slot][lane group][class, statistic]
  const int m0 = blockIdx.y * mpb, cnt = min(mpb, models - m0);
  const int lo = rows[m0].img_off, hi = rows[m0 + cnt - 1].img_off + rows[m0 + cnt - 1].P.nimg + MW_STACK_PAD;
  for (int i = threadIdx.x; i < hi - lo; i += 256) lds[i] = imgs[lo + i];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lg = mpb >> 1;                         // mpb = 1, 2, 4: its logarithm
  const int jl = __builtin_amdgcn_readfirstlane(wv & (mpb - 1));          // the wave's stack of the block
  const int s0 = __builtin_amdgcn_readfirstlane((wv >> lg) << lg);        // its first slot; it takes mpb of them
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  if (jl < cnt) {                                                         // (wave-uniform; an idle wave waits at the barrier below)
    const StackRow *R = rows + m0 + jl;
    const StackP *P = &R->P;
    const float *img = lds + (R->img_off - lo);
    const bool tend = ANYT && R->form != MW_FORM_STATE;
    const double *in_g = F.in[g], *in_s = F.in[g == 0 ? 4 : g + 1], *tr_g = F.truth[g];
    const StackLane S = stack_lane<N9>(P, g);
    constexpr int TILES = SE_TILES;
    EvalAcc acc;
    eval_zero(acc);
    for (int slot = s0; slot < s0 + mpb; slot++) {
      if (!N9) {
        const long long ncells = (long long)nz * ncol;
        const long long nquads = ((ncells + 15) / 16 + TILES - 1) / TILES;
        for (long long q = (long long)blockIdx.x * SE_SLOTS + slot; q < nquads; q += (long long)gridDim.x * SE_SLOTS) {
          double x0[TILES], xs[TILES], xt[TILES], x1[TILES], x2[TILES], y[TILES];
          int cls[TILES];                                                 // 0: no cell, 1: inactive, 2: active (a lane's word: masks would crowd the SGPRs)
#pragma unroll
          for (int u = 0; u < TILES; u++) {
            const long long cell = (q * TILES + u) * 16 + cidx;
            const bool ok = cell < ncells;
            x0[u] = ok ? in_g[cell] : S.imin0;
            xs[u] = ok ? in_s[cell] : S.imin1;
            xt[u] = ok ? tr_g[cell] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < TILES; u++) {
            const bool ok = (q * TILES + u) * 16 + cidx < ncells;
            const double before = g == 0 ? x0[u] : xs[u];
            bool ina, inn;
            MW_EVAL_CELL_CLASS(ina, inn, ok, xt[u], before, cidx)
            cls[u] = ina ? 2 : inn ? 1 : 0;
            x1[u] = g == 0 ? xs[u] : S.imin1;
            x2[u] = S.imin2;
          }
          stack_cells<TILES, false>(y, P, img, S, tend, lane, g, x0, x1, x2);
#pragma unroll
          for (int u = 0; u < TILES; u++) eval_add(acc, y[u], xt[u], cls[u] == 1, cls[u] == 2);
        }
      } else {
        const int ntiles = (int)((ncol + 15) / 16);                       // (the host refuses more column tiles than an int holds)
        for (int t = blockIdx.x * SE_SLOTS + slot; t < ntiles; t += gridDim.x * SE_SLOTS) {
          const long long col = (long long)t * 16 + cidx;
          const bool ok = col < ncol;
          double carry = 0.0;                                             // raw, of the pass before's lowest level: what this lane's feature 4 + g (group 0: 8) is one level down
          for (int k0 = nz - 1; k0 >= 0; k0 -= TILES) {
            double x0[TILES], xs[TILES], xt[TILES], c[TILES], x1[TILES], x2[TILES], y[TILES];
            int cls[TILES];
#pragma unroll
            for (int u = 0; u < TILES; u++) {                             // tile u: level k0 - u
              const int k = k0 - u;
              const bool lv = ok && k >= 0;
              const long long idx = (long long)k * ncol + col;
              x0[u] = lv ? in_g[idx] : S.imin0;
              xs[u] = lv ? in_s[idx] : S.imin1;
              xt[u] = lv ? tr_g[idx] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < TILES; u++) {
              const bool lv = ok && k0 - u >= 0;
              const double before = g == 0 ? x0[u] : xs[u];
              bool ina, inn;
              MW_EVAL_CELL_CLASS(ina, inn, lv, xt[u], before, cidx)
              cls[u] = ina ? 2 : inn ? 1 : 0;
              const double t0 = __shfl(x0[u], (lane + 48) & 63, 64);      // group 1: temp of its level from group 0 (lane - 16)
              c[u] = g == 0 ? xs[u] : g == 1 ? t0 : x0[u];
            }
#pragma unroll
            for (int u = 0; u < TILES; u++) {
              const double above = u == 0 ? (k0 == nz - 1 ? c[0] : carry) : c[u > 0 ? u - 1 : 0];      // the model top is its own level above
              x1[u] = g == 0 ? xs[u] : above;
              x2[u] = g == 0 ? above : S.imin2;
            }
            carry = c[TILES - 1];
            stack_cells<TILES, true>(y, P, img, S, tend, lane, g, x0, x1, x2);
#pragma unroll
            for (int u = 0; u < TILES; u++) eval_add(acc, y[u], xt[u], cls[u] == 1, cls[u] == 2);
          }
        }
      }
      stack_eval_slot_store(acc, red[jl], slot, g, cidx);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < cnt * EVAL_ROW) {
    const int j = threadIdx.x >> 5, r = threadIdx.x & 31;
    partial[((long long)blockIdx.x * models + m0 + j) * EVAL_ROW + r] = stack_eval_slot_join(red[j], r);
  }
}

// the persistence row and the active cells: the flat walk, wave w = slot w.  partial: (gridDim.x, 32); cpartial: (gridDim.x)
__global__ __launch_bounds__(256) void k_stack_eval_persist(long long ncells, EvalFields F, double *__restrict__ partial, long long *__restrict__ cpartial) {
#pragma clang fp contract(off)
  __shared__ double red[SE_SLOTS][4][8];
  __shared__ long long wcount[SE_SLOTS];
  constexpr int TILES = SE_TILES;
  const int lane = threadIdx.x & 63, slot = threadIdx.x >> 6;
  const int g = lane >> 4, cidx = lane & 15;
  const double *in_b = F.in[g == 0 ? 0 : g + 1], *tr_g = F.truth[g];      // the input field that output g replaces
  EvalAcc acc;
  eval_zero(acc);
  long long nact = 0;
  const long long nquads = ((ncells + 15) / 16 + TILES - 1) / TILES;
  for (long long q = (long long)blockIdx.x * SE_SLOTS + slot; q < nquads; q += (long long)gridDim.x * SE_SLOTS) {
    double xb[TILES], xt[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (q * TILES + u) * 16 + cidx;
      const bool ok = cell < ncells;
      xb[u] = ok ? in_b[cell] : 0.0;
      xt[u] = ok ? tr_g[cell] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const bool ok = (q * TILES + u) * 16 + cidx < ncells;
      bool ina, inn;
      MW_EVAL_CELL_CLASS(ina, inn, ok, xt[u], xb[u], cidx)
      nact += __popcll(__ballot(ina && g == 0));
      eval_add(acc, xb[u], xt[u], inn, ina);
    }
  }
  stack_eval_slot_store(acc, red, slot, g, cidx);
  if (lane == 0) wcount[slot] = nact;
  __syncthreads();
  if (threadIdx.x < EVAL_ROW) partial[(long long)blockIdx.x * EVAL_ROW + threadIdx.x] = stack_eval_slot_join(red, threadIdx.x);
  if (threadIdx.x == 0) cpartial[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

// STRICT form: thread = cell, grid row y = one stack of the group (any n_in; the table's order); k_mlp_stack_strict's expressions on the
// parameters as they came.  partial: (gridDim.x, gridDim.y, 32)
__global__ __launch_bounds__(256) void k_stack_eval_strict(const StackRow *__restrict__ rows, const float *__restrict__ params, int nz, long long ncol,
                                                           EvalFields F, double *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[4][EVAL_ROW];
  const StackRow *R = rows + blockIdx.y;
  const StackP &P = R->P;
  const float *par = params + R->par_off;
  const bool tend = R->form != MW_FORM_STATE;
  const long long ncells = (long long)nz * ncol;
  EvalAcc acc[4];
#pragma unroll
  for (int v = 0; v < 4; v++) eval_zero(acc[v]);
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < ncells; c += (long long)gridDim.x * 256) {
    const long long ca = (P.n_in == 9 && c + ncol < ncells) ? c + ncol : c;
    const double in[9] = {F.in[0][c], F.in[1][c], F.in[2][c], F.in[3][c], F.in[4][c], F.in[0][ca], F.in[2][ca], F.in[3][ca], F.in[4][ca]};
    const double before[4] = {in[0], in[2], in[3], in[4]};
    const double tr[4] = {F.truth[0][c], F.truth[1][c], F.truth[2][c], F.truth[3][c]};
    bool act = false;
#pragma unroll
    for (int v = 0; v < 4; v++) act = act || fabs(tr[v] - before[v]) > 1.e-10;
    float x[MW_STACK_MAX_WIDTH], h[MW_STACK_MAX_WIDTH];
    for (int i = 0; i < P.n_in; i++) x[i] = (float)((in[i] - P.in_min[i]) / P.in_rng[i]);
    for (int l = 0; l < P.nl; l++) {
      const int n = P.width[l], no = P.width[l + 1];
      const float *W = par + P.woff[l], *b = par + P.bwoff[l];
      for (int o = 0; o < no; o++) {
        float a = 0.f;
        for (int i = 0; i < n; i++) a += x[i] * W[i * no + o];
        a = a + b[o];
        h[o] = (l < P.nl - 1) ? (a > 0.f ? a : P.slope[l] * a) : a;
      }
      for (int o = 0; o < no; o++) x[o] = h[o];
    }
    double pred[4];
    if (tend) {
      pred[0] =           in[0] + (x[0] * P.out_rng[0] + P.out_min[0]);
      pred[1] = fmax(0.0, in[2] + (x[1] * P.out_rng[1] + P.out_min[1]));
      pred[2] = fmax(0.0, in[3] + (x[2] * P.out_rng[2] + P.out_min[2]));
      pred[3] = fmax(0.0, in[4] + (x[3] * P.out_rng[3] + P.out_min[3]));
    } else {
      pred[0] =           x[0] * P.out_rng[0] + P.out_min[0];
      pred[1] = fmax(0.0, x[1] * P.out_rng[1] + P.out_min[1]);
      pred[2] = fmax(0.0, x[2] * P.out_rng[2] + P.out_min[2]);
      pred[3] = fmax(0.0, x[3] * P.out_rng[3] + P.out_min[3]);
    }
#pragma unroll
    for (int v = 0; v < 4; v++) eval_add(acc[v], pred[v], tr[v], !act, act);
  }
  eval_strict_trees<EVAL_ROW>(acc, red);
  __syncthreads();
  eval_strict_row_store<EVAL_ROW>(red, partial + ((long long)blockIdx.x * gridDim.y + blockIdx.y) * EVAL_ROW);
}

// What the final kernel joins: grid row y = one region of partial rows -- (nblocks, rows, 32) doubles whose local row lr is row
// target[row0 + lr] of `out` (persistence: row n) -- in block order, one thread per number of `out`.
struct StackEvalRegion { const double *partial; int nblocks, rows, row0; };
struct StackEvalFinal { StackEvalRegion reg[3]; StackMap target; int n; };

__global__ __launch_bounds__(256) void k_stack_eval_final(StackEvalFinal A, long long ncells, const long long *__restrict__ cpartial,
                                                          double *__restrict__ out, long long *__restrict__ counts) {
  const StackEvalRegion R = A.reg[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x, len = R.rows * EVAL_ROW;
  if (e < len) {
    const int lr = e >> 5;
    const int row = blockIdx.y == 2 ? A.n : A.target.member[R.row0 + lr];
    eval_final_store(R.nblocks, len, e, R.partial, out + (long long)(row - lr) * EVAL_ROW);
  }
  if (blockIdx.y == 2 && e == 0) {
    long long a = 0;
    for (int b = 0; b < R.nblocks; b++) a += cpartial[b];
    counts[0] = ncells - a; counts[1] = a;
  }
}

// grid.x of the three walks from the shape alone: a row does not depend on the group.  false: the shape is out of range
struct StackEvalGrid { long long flat, cols, strict; };
static bool stack_eval_grid(StackEvalGrid &G, int nz, long long ncol) {
  if (nz < 1 || ncol < 1 || (double)nz * (double)ncol >= 9.0e18) return false;
  const long long ctiles = (ncol + 15) / 16;
  if (ctiles > 0x7fffffffll - SE_SLOTS * EVAL_MAX_BLOCKS) return false;   // (the stencil walk counts column tiles in an int)
  const long long ncells = (long long)nz * ncol;
  const long long nquads = ((ncells + 15) / 16 + SE_TILES - 1) / SE_TILES;
  auto clamp = [](long long b) { return std::max<long long>(1, std::min<long long>(b, EVAL_MAX_BLOCKS)); };
  G.flat = clamp((nquads + SE_SLOTS - 1) / SE_SLOTS);
  G.cols = clamp((ctiles + SE_SLOTS - 1) / SE_SLOTS);
  G.strict = clamp((ncells + 255) / 256);
  return true;
}
// doubles of the stacks' partial rows (either form of the kernels), then (flat, 32) for persistence, then `flat` int64 counts
static long long stack_eval_rows_doubles(const mw_stack_group_s *g, const StackEvalGrid &G) {
  const long long fast = G.flat * g->elist[0].n + G.cols * g->elist[1].n, strict = G.strict * g->n;
  return std::max(fast, strict) * EVAL_ROW;
}

} // namespace mw

using namespace mw;

extern "C" long long mw_stack_group_eval_workspace_bytes(mw_stack_group_t g, int nz, long long ncol) {
  StackEvalGrid G;
  if (!g || !stack_eval_grid(G, nz, ncol)) return 0;
  return (long long)sizeof(double) * (stack_eval_rows_doubles(g, G) + G.flat * EVAL_ROW) + (long long)sizeof(long long) * G.flat;
}

extern "C" int mw_stack_group_eval(mw_stack_group_t g, int nz, long long ncol, const double *const *in5, const double *const *truth4, double *out,
                                   long long *counts, void *workspace, void *stream) {
  if (!g) MW_FAIL("stack_group_eval: null handle");
  if (!in5 || !truth4 || !out || !counts || !workspace) MW_FAIL("stack_group_eval: null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL("stack_group_eval: nz and ncol must be >= 1");
  EvalFields F;
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL("stack_group_eval: null field"); F.in[i] = in5[i]; }
  for (int i = 0; i < 4; i++) { if (!truth4[i]) MW_FAIL("stack_group_eval: null field"); F.truth[i] = truth4[i]; }
  StackEvalGrid G;
  if (!stack_eval_grid(G, nz, ncol)) MW_FAIL("stack_group_eval: the fields are too large");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long ncells = (long long)nz * ncol;
  double *rowsp = (double *)workspace, *pers = rowsp + stack_eval_rows_doubles(g, G);
  long long *cpartial = (long long *)(pers + G.flat * EVAL_ROW);
  StackEvalFinal A;
  memset(&A, 0, sizeof(A));
  A.n = g->n;
  for (int j = 0; j < g->n; j++) A.target.member[g->row_of[j]] = j;        // row r of the table is stack j of the caller
  A.reg[2] = {pers, (int)G.flat, 1, 0};
  if (mlp_strict()) {
    hipLaunchKernelGGL(k_stack_eval_strict, dim3((unsigned)G.strict, (unsigned)g->n), dim3(256), 0, st, g->rows, g->params, nz, ncol, F, rowsp);
    MW_LAUNCH_CHECK();
    A.reg[0] = {rowsp, (int)G.strict, g->n, 0};
  } else {
    double *part = rowsp;
    for (int pass = 0; pass < 2; pass++) {
      const StackList &L = g->elist[pass];
      if (L.n < 1) continue;
      if (L.lds > MW_STACK_GROUP_LDS - MW_STACK_EVAL_RED) MW_FAIL("stack_group_eval: a stack's image exceeds the kernel's LDS");      // (no shape mw_mlp_stack_create accepts does)
      const long long blocks = pass == 0 ? G.flat : G.cols;
      const dim3 grid((unsigned)blocks, (unsigned)((L.n + L.mpb - 1) / L.mpb));
      if (pass == 0) MW_LAUNCH_IF(L.anyt, (k_stack_eval<false, true>), (k_stack_eval<false, false>), grid, dim3(256), L.lds, st, g->rows + L.r0, g->imgs, L.n, L.mpb, nz, ncol, F, part);
      else           MW_LAUNCH_IF(L.anyt, (k_stack_eval<true, true>), (k_stack_eval<true, false>), grid, dim3(256), L.lds, st, g->rows + L.r0, g->imgs, L.n, L.mpb, nz, ncol, F, part);
      MW_LAUNCH_CHECK();
      A.reg[pass] = {part, (int)blocks, L.n, L.r0};
      part += blocks * L.n * EVAL_ROW;
    }
  }
  hipLaunchKernelGGL(k_stack_eval_persist, dim3((unsigned)G.flat), dim3(256), 0, st, ncells, F, pers, cpartial);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_stack_eval_final, dim3((unsigned)((g->n * EVAL_ROW + 255) / 256), 3), dim3(256), 0, st, A, ncells, (const long long *)cpartial, out, counts);
  MW_LAUNCH_CHECK();
  return 0;
}
