// =====================================================================================================
// mw_stack_committee.hip -- a COMMITTEE of dense surrogate stacks (mw_mlp_stack.h): the mean of 1 .. 16 selected stacks of a group and
// their range on one ensemble member of the member-fastest arrays (mw_stack_group_committee_apply; mw_surrogate_committee_apply's
// semantics for stacks of any shape, width and form).  DESIGN.md 13.22.
//
// For a cell and an output field, y_j is what mw_mlp_stack_forward stores for stack sel[j] (stack_cells: its own scaling, base and clip
// BEFORE combining); mean = (((y_0 + y_1) + y_2) + ...) / (double)n in the order of sel, the first addend as it is; range = hi - lo with
// the NaN-propagating extrema of eval_max / eval_min.  A committee of one returns its stack's bits and range 0.
//
// CHUNKS.  A stack's image is up to 57,408 B, so the models cannot all sit in LDS as the fixed committee's do.  The host splits sel
// greedily, in listed order, into chunks: the longest run of consecutive stacks whose images + MW_STACK_PAD fit MW_STACK_GROUP_LDS bytes
// of dynamic LDS together.  One launch per chunk, in order, on the caller's stream.  A 256-thread workgroup fills LDS once with its
// chunk's images (each behind the one before, wherever it lies in the group's buffer); the loop over the chunk's stacks is INSIDE the
// tile loop: a wave keeps the raw features of its tiles in registers, reads each stack's StackP row through a wave-uniform index and calls
// stack_cells once per stack, and keeps sum, hi, lo of its (cell, field) in three doubles per tile.  One pass over the state serves
// every stack of the chunk.  Between launches the partial (sum, hi, lo) x 4 fields travel in the caller's workspace, 12 planes of the
// member's cells (contiguous, not member-fastest): the first chunk starts from its first y, a middle chunk loads, combines and stores,
// only the last divides and writes out4 / range4.  The sum is sequential in the order of sel, so the chunking does not show in the bits,
// and nothing touches the state before the last launch.  first / last are run-time, wave-uniform flags.
//
// The two walks are k_stack_members': n_in = 5 flat 16-cell tiles at cell * nens + member; n_in = 9 a wave owns 16 columns, top-down,
// the four tiles of a pass are consecutive levels, the level above carried RAW from tile to tile and from pass to pass and scaled per
// stack where it is used, group 1's temp by the lane move.  A level is stored after every load of its pass and nobody else reads the
// member's columns: in place and out of place give the same bits with no copy.  Only vector loads and stores, no atomics.
// k_stack_committee_strict<NIN> (mw_mlp_set_strict(1)): thread = cell (n_in = 5) or column of the member, top-down (n_in = 9);
// k_mlp_stack_strict's index-order loops on the parameters as they came, the stacks in listed order, no chunks and no workspace.
// =====================================================================================================
#include "mw_mlp_stack.h"

namespace mw {

template <bool N9, bool ANYT>
__global__ __launch_bounds__(256, 2) void k_stack_committee(const StackRow *__restrict__ rows, const float *__restrict__ imgs, StackChunk C, double dn,
                                                         int member, int nz, long long ncol, int nens, StackCommitteeFields F,
                                                         double *__restrict__ ws) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int j = 0; j < C.n; j++) {
    const StackRow *R = rows + C.row[j];
    const int len = R->P.nimg + MW_STACK_PAD;                             // (the group keeps the pad behind every image)
    const float *src = imgs + R->img_off;
    float *dst = lds + C.lds_off[j];
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const bool first = C.first != 0, last = C.last != 0;
  const double *in_g = F.in[g], *rho_r = F.in[4];
  double *out_g = F.out[g], *rng_g = F.range[g];
  const long long ncells = (long long)nz * ncol;
  double *ws_g = ws + 3 * g * ncells;                                     // (never dereferenced in a one-chunk committee)
  constexpr int TILES = SC_TILES;
  if (!N9) {
    const long long ntiles = (ncells + 15) / 16;
    for (long long t0 = ((long long)blockIdx.x * 4 + wv) * TILES; t0 < ntiles; t0 += (long long)gridDim.x * 4 * TILES) {
      double x0[TILES], x1[TILES], x2[TILES], y[TILES];
      CommitteeAcc a[TILES];
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const long long cell = (t0 + u) * 16 + cidx;
        const bool ok = cell < ncells;
        x0[u] = ok ? in_g[cell * nens + member] : 0.0;
        x1[u] = (ok && g == 0) ? rho_r[cell * nens + member] : 0.0;
        x2[u] = 0.0;
        a[u].sum = (ok && !first) ? ws_g[cell] : 0.0;
        a[u].hi  = (ok && !first) ? ws_g[ncells + cell] : 0.0;
        a[u].lo  = (ok && !first) ? ws_g[2 * ncells + cell] : 0.0;
      }
      for (int j = 0; j < C.n; j++) {
        const StackRow *R = rows + C.row[j];
        const StackLane S = stack_lane<false>(&R->P, g);
        stack_cells<TILES, false>(y, &R->P, lds + C.lds_off[j], S, ANYT && R->form != MW_FORM_STATE, lane, g, x0, x1, x2);
#pragma unroll
        for (int u = 0; u < TILES; u++) acc_add(a[u], y[u], first && j == 0);
      }
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const long long cell = (t0 + u) * 16 + cidx;
        if (cell < ncells) {
          if (last) {
            out_g[cell * nens + member] = a[u].sum / dn;
            if (rng_g) rng_g[cell * nens + member] = a[u].hi - a[u].lo;
          } else {
            ws_g[cell] = a[u].sum; ws_g[ncells + cell] = a[u].hi; ws_g[2 * ncells + cell] = a[u].lo;
          }
        }
      }
    }
  } else {
    const int ntiles = (int)((ncol + 15) / 16);                           // (the host refuses more column tiles than an int holds)
    const long long lev = ncol * nens;                                    // doubles from level k to level k + 1
    for (int t = blockIdx.x * 4 + wv; t < ntiles; t += gridDim.x * 4) {
      const long long col = (long long)t * 16 + cidx;
      const bool ok = col < ncol;
      const long long at = col * nens + member;
      double carry = 0.0;                                                 // raw, of the pass before's lowest level: what this lane's feature 4 + g (group 0: 8) is one level down
      for (int k0 = nz - 1; k0 >= 0; k0 -= TILES) {
        double x0[TILES], xr[TILES], c[TILES], x1[TILES], x2[TILES], y[TILES];
        CommitteeAcc a[TILES];
#pragma unroll
        for (int u = 0; u < TILES; u++) {                                 // tile u: level k0 - u
          const int k = k0 - u;
          const bool lv = ok && k >= 0;
          const long long cell = (long long)k * ncol + col;
          x0[u] = lv ? in_g[(long long)k * lev + at] : 0.0;
          xr[u] = (lv && g == 0) ? rho_r[(long long)k * lev + at] : 0.0;
          a[u].sum = (lv && !first) ? ws_g[cell] : 0.0;
          a[u].hi  = (lv && !first) ? ws_g[ncells + cell] : 0.0;
          a[u].lo  = (lv && !first) ? ws_g[2 * ncells + cell] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const double t0 = __shfl(x0[u], (lane + 48) & 63, 64);          // group 1: temp of its level from group 0 (lane - 16)
          c[u] = g == 0 ? xr[u] : g == 1 ? t0 : x0[u];
        }
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const double above = u == 0 ? (k0 == nz - 1 ? c[0] : carry) : c[u > 0 ? u - 1 : 0];      // the model top is its own level above
          x1[u] = g == 0 ? xr[u] : above;
          x2[u] = g == 0 ? above : 0.0;
        }
        carry = c[TILES - 1];
        for (int j = 0; j < C.n; j++) {
          const StackRow *R = rows + C.row[j];
          const StackLane S = stack_lane<true>(&R->P, g);
          stack_cells<TILES, true>(y, &R->P, lds + C.lds_off[j], S, ANYT && R->form != MW_FORM_STATE, lane, g, x0, x1, x2);
#pragma unroll
          for (int u = 0; u < TILES; u++) acc_add(a[u], y[u], first && j == 0);
        }
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const int k = k0 - u;
          if (ok && k >= 0) {
            const long long cell = (long long)k * ncol + col;
            if (last) {
              out_g[(long long)k * lev + at] = a[u].sum / dn;
              if (rng_g) rng_g[(long long)k * lev + at] = a[u].hi - a[u].lo;
            } else {
              ws_g[cell] = a[u].sum; ws_g[ncells + cell] = a[u].hi; ws_g[2 * ncells + cell] = a[u].lo;
            }
          }
        }
      }
    }
  }
}


// STRICT form.  NIN = 5: thread = one cell of the member; NIN = 9: thread = one column of the member, swept top-down with temp, rho_v,
// rho_c, rho_r of the level above AS THEY WERE in registers.  items: the member's cells / columns.
template <int NIN>
__global__ __launch_bounds__(256) void k_stack_committee_strict(const StackRow *__restrict__ rows, const float *__restrict__ params, StackSel S, int member,
                                                                int nz, long long ncol, int nens, StackCommitteeFields F) {
#pragma clang fp contract(off)
  const long long lev = ncol * nens, items = NIN == 5 ? (long long)nz * ncol : ncol;
  const double dn = (double)S.n;
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
    const long long at = it * nens + member;
    double ab[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = NIN == 5 ? 0 : nz - 1; k >= 0; k--) {
      const long long c = NIN == 5 ? at : (long long)k * lev + at;
      double in[9] = {F.in[0][c], F.in[1][c], F.in[2][c], F.in[3][c], F.in[4][c], 0.0, 0.0, 0.0, 0.0};
      if (NIN == 9) {
        if (k == nz - 1) { ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4]; }      // the column's top level is its own level above
        in[5] = ab[0]; in[6] = ab[1]; in[7] = ab[2]; in[8] = ab[3];
        ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4];
      }
      CommitteeAcc a[4];
      for (int j = 0; j < S.n; j++) {
        const StackRow *R = rows + S.row[j];
        double p[4];
        stack_strict_cell(R, params + R->par_off, in, p);
#pragma unroll
        for (int v = 0; v < 4; v++) acc_add(a[v], p[v], j == 0);
      }
#pragma unroll
      for (int v = 0; v < 4; v++) {
        F.out[v][c] = a[v].sum / dn;
        if (F.range[v]) F.range[v][c] = a[v].hi - a[v].lo;
      }
    }
  }
}


} // namespace mw

using namespace mw;

// Chunk c of a planned committee in the fast form, on `st`: what mw_stack_group_committee_apply launches for it.  mw_stack_guard.hip
// sends the chunks before its own last launch through here, so they are these kernels unchanged.
int mw::stack_committee_launch(const mw_stack_group_s *g, const StackCommitteePlan &Q, int c, int member, int nz, long long ncol, int nens,
                               const StackCommitteeFields &F, double *workspace, hipStream_t st) {
  const long long ncells = (long long)nz * ncol;
  const long long items = Q.n_in == 5 ? ((ncells + 15) / 16 + SC_TILES - 1) / SC_TILES : (ncol + 15) / 16;      // tile groups / column tiles
  const long long blocks = std::max<long long>(1, std::min<long long>((items + 3) / 4, SC_MAX_BLOCKS));
  const double dn = (double)Q.sel.n;
  const dim3 grid((unsigned)blocks);
  if (Q.n_in == 5) MW_LAUNCH_IF(Q.anyt, (k_stack_committee<false, true>), (k_stack_committee<false, false>), grid, dim3(256), Q.lds[c], st, g->rows, g->imgs, Q.chunk[c], dn, member, nz, ncol, nens, F, workspace);
  else             MW_LAUNCH_IF(Q.anyt, (k_stack_committee<true, true>), (k_stack_committee<true, false>), grid, dim3(256), Q.lds[c], st, g->rows, g->imgs, Q.chunk[c], dn, member, nz, ncol, nens, F, workspace);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_stack_group_committee_workspace_bytes(mw_stack_group_t g, int n_sel, const int *sel, int nz, long long ncol, long long *bytes) {
  if (!bytes) MW_FAIL("stack_group_committee_workspace_bytes: null pointer");
  *bytes = 0;
  StackCommitteePlan Q;
  const std::string err = stack_committee_plan(Q, g, n_sel, sel, "stack_group_committee_workspace_bytes");
  if (!err.empty()) MW_FAIL(err);
  if (nz < 1 || ncol < 1) MW_FAIL("stack_group_committee_workspace_bytes: nz and ncol must be >= 1");
  if ((double)nz * (double)ncol * 96.0 > 9.0e18) MW_FAIL("stack_group_committee_workspace_bytes: the fields are too large");
  if (Q.nchunks > 1 && !mlp_strict()) *bytes = 96ll * nz * ncol;            // (sum, hi, lo) x 4 fields in fp64 per cell of the member
  return 0;
}

extern "C" int mw_stack_group_committee_apply(mw_stack_group_t g, int n_sel, const int *sel, int member, int nz, long long ncol, int nens,
                                              const double *const *in5, double *const *out4, double *const *range4, void *workspace,
                                              long long workspace_bytes, void *stream) {
  if (!g) MW_FAIL("stack_group_committee_apply: null handle");
  if (!sel || !in5 || !out4) MW_FAIL("stack_group_committee_apply: null pointer");
  StackCommitteePlan Q;
  const std::string err = stack_committee_plan(Q, g, n_sel, sel, "stack_group_committee_apply");
  if (!err.empty()) MW_FAIL(err);
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL("stack_group_committee_apply: nz, ncol and nens must be >= 1");
  if (member < 0 || member >= nens) MW_FAIL("stack_group_committee_apply: member " + std::to_string(member) + " is outside [0, " + std::to_string(nens) + ")");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18 || (double)nz * (double)ncol * 96.0 > 9.0e18) MW_FAIL("stack_group_committee_apply: the fields are too large");
  if ((ncol + 15) / 16 > 0x7fffffffll - 4 * SC_MAX_BLOCKS) MW_FAIL("stack_group_committee_apply: more column tiles than an int holds");
  const long long total = (long long)nz * ncol * nens, ncells = (long long)nz * ncol;
  StackCommitteeFields F;
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL("stack_group_committee_apply: null field"); F.in[i] = in5[i]; }
  for (int v = 0; v < 4; v++) { if (!out4[v]) MW_FAIL("stack_group_committee_apply: null field"); F.out[v] = out4[v]; F.range[v] = nullptr; }
  if (range4) for (int v = 0; v < 4; v++) { if (!range4[v]) MW_FAIL("stack_group_committee_apply: null field"); F.range[v] = range4[v]; }
  // an output is its own input field (in place) or overlaps no input; outputs and ranges overlap nothing else
  const int own[4] = {0, 2, 3, 4};
  for (int v = 0; v < 4; v++) {
    for (int i = 0; i < 5; i++) {
      if (!(F.out[v] == F.in[i] && i == own[v]) && sc_overlap(F.out[v], total, F.in[i], total)) MW_FAIL("stack_group_committee_apply: an output must be its own input field (in place) or overlap no input");
      if (F.range[v] && sc_overlap(F.range[v], total, F.in[i], total)) MW_FAIL("stack_group_committee_apply: a range field must not overlap an input");
    }
    for (int w = 0; w < 4; w++) {
      if (w != v && sc_overlap(F.out[v], total, F.out[w], total)) MW_FAIL("stack_group_committee_apply: the outputs must not overlap each other");
      if (F.range[v] && sc_overlap(F.range[v], total, F.out[w], total)) MW_FAIL("stack_group_committee_apply: a range field must not overlap an output");
      if (F.range[v] && w != v && sc_overlap(F.range[v], total, F.range[w], total)) MW_FAIL("stack_group_committee_apply: the range fields must not overlap each other");
    }
  }
  const bool strict = mlp_strict() != 0;
  const long long need = (Q.nchunks > 1 && !strict) ? 96ll * ncells : 0;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) MW_FAIL("stack_group_committee_apply: a committee of " + std::to_string(Q.nchunks) + " chunks needs a workspace of " +
                                                      std::to_string(need) + " bytes, got " + std::to_string(workspace ? workspace_bytes : 0));
    const double *wsd = (const double *)workspace;
    for (int i = 0; i < 5; i++) if (sc_overlap(wsd, 12 * ncells, F.in[i], total)) MW_FAIL("stack_group_committee_apply: the workspace must not overlap a field");
    for (int v = 0; v < 4; v++)
      if (sc_overlap(wsd, 12 * ncells, F.out[v], total) || (F.range[v] && sc_overlap(wsd, 12 * ncells, F.range[v], total)))
        MW_FAIL("stack_group_committee_apply: the workspace must not overlap a field");
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  if (strict) {
    const long long items = Q.n_in == 5 ? ncells : ncol;
    const long long blocks = std::max<long long>(1, std::min<long long>((items + 255) / 256, SC_MAX_BLOCKS));
    if (Q.n_in == 5) hipLaunchKernelGGL(k_stack_committee_strict<5>, dim3((unsigned)blocks), dim3(256), 0, st, g->rows, g->params, Q.sel, member, nz, ncol, nens, F);
    else             hipLaunchKernelGGL(k_stack_committee_strict<9>, dim3((unsigned)blocks), dim3(256), 0, st, g->rows, g->params, Q.sel, member, nz, ncol, nens, F);
    MW_LAUNCH_CHECK();
    return 0;
  }
  for (int c = 0; c < Q.nchunks; c++)
    if (stack_committee_launch(g, Q, c, member, nz, ncol, nens, F, (double *)workspace, st)) return 1;
  return 0;
}
