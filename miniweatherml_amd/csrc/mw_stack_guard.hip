// =====================================================================================================
// mw_stack_guard.hip -- the GUARDED committee of dense stacks (mw_stack_group_committee_guard_flag): the mean of a
// selection of a group's stacks on one ensemble member, out of place, and IN THE SAME LAUNCH the member's column flags and their count
// by mw_committee_guard_flags' rule (13.7) -- a column goes to Kessler when at some level some field has !(range <= thr) or a mean that
// is not finite.  The composed form writes the range (32 B per cell) and reads mean and range again (64 B) in a launch of its own; here
// the decision is taken on the registers that hold sum, hi and lo, and the range is stored only for a caller who asks for it.
//
// k_stack_committee_guard<N9, ANYT> is the LAST launch of the committee: mw_stack_committee.hip's 256 threads, LDS fill of the chunk's
// images, StackChunk, first / last workspace protocol and stack_cells<4, N9> call per stack.  The chunks before the last are
// k_stack_committee's own launches (stack_committee_launch), which leave (sum, hi, lo) x 4 in the workspace planes at cell = k * ncol +
// col whichever walk wrote them.  The walk here is always the COLUMN walk, for n_in = 5 too -- a flat 16-cell tile owns no column: a
// wave owns 16 columns top-down, lane (g, cidx) field g of column 16 t + cidx, four consecutive levels per pass.  n_in = 9 carries the
// level above raw from tile to tile and pass to pass and moves temp from group 0 to group 1; n_in = 5 is that walk without the level
// above (x1 = rho_r in group 0, x2 = 0, no carry, no lane move).  A cell's bits do not depend on the walk.
// Per lane ONE integer `bad`, ORed over the column's levels with the flags kernel's expression (| on integers, no branch: NaN flags, a
// range equal to its threshold does not).  Behind the last level one ballot: column cidx is flagged iff bit cidx, 16 + cidx, 32 + cidx
// or 48 + cidx is set.  Group 0's lanes store the member's flag byte of their column (a vector byte store of 0 or 1), lane 0 adds the
// popcount of the folded 16-bit mask to both count words (integer atomicAdd, skipped when zero: any order, the same numbers).
// k_stack_committee_guard_strict<NIN> (mw_mlp_set_strict(1)): thread = column of the member for both widths, top-down,
// stack_strict_cell with the stacks in listed order; the byte store by the thread, a ballot popcount per wave.  No chunks, no workspace.
// Only vector loads and stores and integer atomics.
// =====================================================================================================
#include "mw_mlp_stack.h"

namespace mw {

struct StackGuardOut { double thr[4]; unsigned char *flags; unsigned long long *counts; };

// the flags kernel's test of one (cell, field): 1 flags.  (k_committee_guard_flags' spelling)
__device__ __forceinline__ int guard_bad(double range, double thr, double mean) {
  return (int)!(range <= thr) | (int)!(fabs(mean) <= 1.7976931348623157e308);
}

template <bool N9, bool ANYT>
__global__ __launch_bounds__(256, 2) void k_stack_committee_guard(const StackRow *__restrict__ rows, const float *__restrict__ imgs, StackChunk C, double dn,
                                                                  int member, int nz, long long ncol, int nens, StackCommitteeFields F,
                                                                  StackGuardOut G, const double *__restrict__ ws) {
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
  const bool first = C.first != 0;                                        // (this launch is the last one: it divides and writes out)
  const double *in_g = F.in[g], *rho_r = F.in[4];
  double *out_g = F.out[g], *rng_g = F.range[g];
  const double thr = G.thr[g];
  const long long ncells = (long long)nz * ncol;
  const double *ws_g = ws + 3 * g * ncells;                               // (never dereferenced in a one-chunk committee)
  constexpr int TILES = SC_TILES;
  const int ntiles = (int)((ncol + 15) / 16);                             // (the host refuses more column tiles than an int holds)
  const long long lev = ncol * nens;                                      // doubles from level k to level k + 1
  for (int t = blockIdx.x * 4 + wv; t < ntiles; t += gridDim.x * 4) {
    const long long col = (long long)t * 16 + cidx;
    const bool ok = col < ncol;
    const long long at = col * nens + member;
    double carry = 0.0;                                                   // n_in = 9: raw, of the pass before's lowest level
    int bad = 0;
    for (int k0 = nz - 1; k0 >= 0; k0 -= TILES) {
      double x0[TILES], xr[TILES], x1[TILES], x2[TILES], y[TILES];
      CommitteeAcc a[TILES];
#pragma unroll
      for (int u = 0; u < TILES; u++) {                                   // tile u: level k0 - u
        const int k = k0 - u;
        const bool lv = ok && k >= 0;
        const long long cell = (long long)k * ncol + col;
        x0[u] = lv ? in_g[(long long)k * lev + at] : 0.0;
        xr[u] = (lv && g == 0) ? rho_r[(long long)k * lev + at] : 0.0;
        a[u].sum = (lv && !first) ? ws_g[cell] : 0.0;
        a[u].hi  = (lv && !first) ? ws_g[ncells + cell] : 0.0;
        a[u].lo  = (lv && !first) ? ws_g[2 * ncells + cell] : 0.0;
      }
      if (N9) {
        double c[TILES];
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
      } else {
#pragma unroll
        for (int u = 0; u < TILES; u++) { x1[u] = xr[u]; x2[u] = 0.0; }   // (xr is 0 outside group 0)
      }
      for (int j = 0; j < C.n; j++) {
        const StackRow *R = rows + C.row[j];
        const StackLane S = stack_lane<N9>(&R->P, g);
        stack_cells<TILES, N9>(y, &R->P, lds + C.lds_off[j], S, ANYT && R->form != MW_FORM_STATE, lane, g, x0, x1, x2);
#pragma unroll
        for (int u = 0; u < TILES; u++) acc_add(a[u], y[u], first && j == 0);
      }
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const int k = k0 - u;
        const bool lv = ok && k >= 0;
        const double mean = a[u].sum / dn, range = a[u].hi - a[u].lo;
        bad |= guard_bad(range, thr, mean) & (int)lv;                     // (a level above the top, a column past the edge: never)
        if (lv) {
          out_g[(long long)k * lev + at] = mean;
          if (rng_g) rng_g[(long long)k * lev + at] = range;
        }
      }
    }
    const unsigned long long b = __ballot(bad != 0);                      // (t is wave-uniform: all 64 lanes are here)
    const long long left = ncol - (long long)t * 16;
    const unsigned int valid = left >= 16 ? 0xffffu : ((1u << (int)left) - 1u);
    const unsigned int m16 = (unsigned int)((b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffull) & valid;
    if (g == 0 && ok) G.flags[at] = (unsigned char)((m16 >> cidx) & 1u);
    if (lane == 0 && m16) {
      const unsigned long long q = (unsigned long long)__popc(m16);
      atomicAdd(G.counts, q);
      atomicAdd(G.counts + 1, q);
    }
  }
}

// STRICT form: thread = one column of the member for both widths, top-down (NIN = 9: temp, rho_v, rho_c, rho_r of the level above AS
// THEY WERE in registers).  A wave's 64 columns are consecutive and its loop bound is wave-uniform, so the ballot sees every lane.
template <int NIN>
__global__ __launch_bounds__(256) void k_stack_committee_guard_strict(const StackRow *__restrict__ rows, const float *__restrict__ params, StackSel S,
                                                                      int member, int nz, long long ncol, int nens, StackCommitteeFields F,
                                                                      StackGuardOut G) {
#pragma clang fp contract(off)
  const long long lev = ncol * nens;
  const double dn = (double)S.n;
  const int lane = threadIdx.x & 63;
  for (long long c0 = (long long)blockIdx.x * 256 + (threadIdx.x - lane); c0 < ncol; c0 += (long long)gridDim.x * 256) {
    const long long col = c0 + lane, at = col * nens + member;
    int bad = 0;
    if (col < ncol) {
      double ab[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = nz - 1; k >= 0; k--) {
        const long long c = (long long)k * lev + at;
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
          const double mean = a[v].sum / dn, range = a[v].hi - a[v].lo;
          bad |= guard_bad(range, G.thr[v], mean);
          F.out[v][c] = mean;
          if (F.range[v]) F.range[v][c] = range;
        }
      }
      G.flags[at] = (unsigned char)(bad != 0);
    }
    const unsigned long long b = __ballot(bad != 0);
    if (lane == 0 && b) {
      const unsigned long long q = (unsigned long long)__popcll(b);
      atomicAdd(G.counts, q);
      atomicAdd(G.counts + 1, q);
    }
  }
}

} // namespace mw

using namespace mw;

extern "C" int mw_stack_group_committee_guard_flag(mw_stack_group_t g, int n_sel, const int *sel, int member, int nz, long long ncol, int nens,
                                                   const double *const *in5, double *const *mean4, double *const *range4, const double *thr4,
                                                   unsigned char *flags, long long *counts, void *workspace, long long workspace_bytes,
                                                   void *stream) {
  const std::string who = "stack_group_committee_guard_flag";
  if (!sel || !in5 || !mean4 || !thr4 || !flags || !counts) MW_FAIL(who + ": null pointer");
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL(who + ": nz, ncol and nens must be >= 1");
  if (member < 0 || member >= nens) MW_FAIL(who + ": member " + std::to_string(member) + " is outside [0, " + std::to_string(nens) + ")");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18 || (double)nz * (double)ncol * 96.0 > 9.0e18) MW_FAIL(who + ": the fields are too large");
  if ((ncol + 15) / 16 > 0x7fffffffll - 4 * SC_MAX_BLOCKS) MW_FAIL(who + ": more column tiles than an int holds");
  const long long total = (long long)nz * ncol * nens, ncells = (long long)nz * ncol;
  StackCommitteeFields F;
  StackGuardOut G;
  for (int i = 0; i < 5; i++) { if (!in5[i]) MW_FAIL(who + ": null field"); F.in[i] = in5[i]; }
  for (int v = 0; v < 4; v++) { if (!mean4[v]) MW_FAIL(who + ": null field"); F.out[v] = mean4[v]; F.range[v] = nullptr; }
  if (range4) for (int v = 0; v < 4; v++) { if (!range4[v]) MW_FAIL(who + ": null field"); F.range[v] = range4[v]; }
  for (int v = 0; v < 4; v++) {
    if (!(thr4[v] >= 0.0)) MW_FAIL(who + ": threshold " + std::to_string(v) + " is negative or NaN (+inf: the field never flags by size)");
    G.thr[v] = thr4[v];
  }
  // the mean is never the state (Kessler needs it on the flagged columns): means and ranges overlap no input and not each other
  for (int v = 0; v < 4; v++) {
    for (int i = 0; i < 5; i++) {
      if (sc_overlap(F.out[v], total, F.in[i], total)) MW_FAIL(who + ": a mean field must overlap no input (in place is refused: Kessler reads the state on the flagged columns)");
      if (F.range[v] && sc_overlap(F.range[v], total, F.in[i], total)) MW_FAIL(who + ": a range field must not overlap an input");
    }
    for (int w = 0; w < 4; w++) {
      if (w != v && sc_overlap(F.out[v], total, F.out[w], total)) MW_FAIL(who + ": the mean fields must not overlap each other");
      if (F.range[v] && sc_overlap(F.range[v], total, F.out[w], total)) MW_FAIL(who + ": a range field must not overlap a mean field");
      if (F.range[v] && w != v && sc_overlap(F.range[v], total, F.range[w], total)) MW_FAIL(who + ": the range fields must not overlap each other");
    }
  }
  StackCommitteePlan Q;
  const std::string err = stack_committee_plan(Q, g, n_sel, sel, who);
  if (!err.empty()) MW_FAIL(err);
  const bool strict = mlp_strict() != 0;
  const long long need = (Q.nchunks > 1 && !strict) ? 96ll * ncells : 0;
  if (need > 0) {
    if (!workspace || workspace_bytes < need) MW_FAIL(who + ": a committee of " + std::to_string(Q.nchunks) + " chunks needs a workspace of " +
                                                      std::to_string(need) + " bytes, got " + std::to_string(workspace ? workspace_bytes : 0));
    const double *wsd = (const double *)workspace;
    for (int i = 0; i < 5; i++) if (sc_overlap(wsd, 12 * ncells, F.in[i], total)) MW_FAIL(who + ": the workspace must not overlap a field");
    for (int v = 0; v < 4; v++)
      if (sc_overlap(wsd, 12 * ncells, F.out[v], total) || (F.range[v] && sc_overlap(wsd, 12 * ncells, F.range[v], total)))
        MW_FAIL(who + ": the workspace must not overlap a field");
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  G.flags = flags; G.counts = (unsigned long long *)counts;
  MW_HIP(hipMemsetAsync(counts, 0, 8, st));                                 // counts[0]: this call's count; counts[1] goes on accumulating
  if (strict) {
    const long long blocks = std::max<long long>(1, std::min<long long>((ncol + 255) / 256, SC_MAX_BLOCKS));
    if (Q.n_in == 5) hipLaunchKernelGGL(k_stack_committee_guard_strict<5>, dim3((unsigned)blocks), dim3(256), 0, st, g->rows, g->params, Q.sel, member, nz, ncol, nens, F, G);
    else             hipLaunchKernelGGL(k_stack_committee_guard_strict<9>, dim3((unsigned)blocks), dim3(256), 0, st, g->rows, g->params, Q.sel, member, nz, ncol, nens, F, G);
    MW_LAUNCH_CHECK();
    return 0;
  }
  const int c = Q.nchunks - 1;
  for (int b = 0; b < c; b++)                                               // the chunks before the last: k_stack_committee's launches as they are
    if (stack_committee_launch(g, Q, b, member, nz, ncol, nens, F, (double *)workspace, st)) return 1;
  const long long blocks = std::max<long long>(1, std::min<long long>(((ncol + 15) / 16 + 3) / 4, SC_MAX_BLOCKS));
  const dim3 grid((unsigned)blocks);
  const double dn = (double)n_sel;
  if (Q.n_in == 5) MW_LAUNCH_IF(Q.anyt, (k_stack_committee_guard<false, true>), (k_stack_committee_guard<false, false>), grid, dim3(256), Q.lds[c], st, g->rows, g->imgs, Q.chunk[c], dn, member, nz, ncol, nens, F, G, (const double *)workspace);
  else             MW_LAUNCH_IF(Q.anyt, (k_stack_committee_guard<true, true>), (k_stack_committee_guard<true, false>), grid, dim3(256), Q.lds[c], st, g->rows, g->imgs, Q.chunk[c], dn, member, nz, ncol, nens, F, G, (const double *)workspace);
  MW_LAUNCH_CHECK();
  return 0;
}
