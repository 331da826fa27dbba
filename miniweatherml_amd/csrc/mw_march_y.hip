// =====================================================================================================
// mw_march_y.hip -- launchers of the y-face marching kernels of mw_march.h (k_y_state, k_y_all, k_y_tracers): launch code only.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include "mw_march.h"

// rows per chunk of k_y_state / k_y_all, decided once per handle (threads: of one member's launch)
static int y_chunk(mw_dycore_s *d, const DyP &p, long long threads) {
  return d->chunk_y ? d->chunk_y : (d->chunk_y = balanced_chunk(d, p.ny, (threads + 63) / 64, d->o.chunk_y, 5000, 2, 5.0, (threads + 255) / 256 < 96));
}

// conv != nullptr: the slab S is still empty -- the kernel converts the coupler's fields on the way and fills it (k_y_state<true>)
// edges: only the two MW_Y_EDGE-row strips at the block's south / north end (pipelined multi-rank schedule, on stream st); a block too
// short to split (see launch_y_all) takes all its rows here
int launch_y_state(mw_dycore_s *d, const double *S, int par, const CouplerPtrs *conv, bool edges, hipStream_t st) {
  if (d->p.sim2d) return 0;
  if (!st) st = d->stream;
  ProfScope ps(d, 5, st);
  if (conv && d->member_major) {
    // D1 inside the launch, member-major handle: ONE launch over the fused lanes (k_y_state<.., MM>): unit-stride reads of the
    // coupler's arrays, outputs into the members' arrays.  The folded configuration is decided on a member's view (nens = 1 there).
    const View v0 = view(d, 0);
    const DyP &p = d->p;
    const long long threads = (long long)p.nz * p.nx * p.nens;
    const long long mthreads = (long long)p.nz * p.nx;                                   // one member's: the chunk rule of the per-member launches
    int chunk = y_chunk(d, p, mthreads);
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)((p.ny + chunk - 1) / chunk));
    const MemberOff mo = member_off(d);
    const YMember mm = {v0.p.sJ, v0.p.sK, v0.p.sV, v0.slab, v0.p.fyJ, v0.p.fyK, v0.m[1], v0.p.nC, v0.tend, p.nx, mo.per, mo.n, mo.sh};
    double *Sw = const_cast<double *>(S);
    const int K = marching_config(d, v0.p);
    if (d->mm_direct && d->o.mm_conv) {      // the members of the same cells in one workgroup (k_y_state<.., MM = 2>)
      grid.x = (unsigned)((mthreads + 64 * (4 / mo.n) - 1) / (64 * (4 / mo.n)));
#define MW_YSM2(K_) { if (d->ord == 3) MW_YSM2O(K_, 3); else MW_YSM2O(K_, 5); }
#define MW_YSM2O(K_, O_) MW_KLAUNCH((k_y_state<true, K_, O_, 2>), grid, dim3(256), 0, d->stream, v0.p, S, d->M[par][1], d->UP[par][1], d->tendY, chunk, *conv, Sw, mm)
      if (K == 1) MW_YSM2(1) else if (K == 2) MW_YSM2(2) else MW_YSM2(0)
#undef MW_YSM2
#undef MW_YSM2O
      MW_LAUNCH_CHECK();
      return 0;
    }
#define MW_YSM(K_, O_) MW_KLAUNCH((k_y_state<true, K_, O_, 1>), grid, dim3(256), 0, d->stream, p, S, d->M[par][1], d->UP[par][1], d->tendY, chunk, *conv, Sw, mm)
    if (d->ord == 3) { if (K == 1) MW_YSM(1, 3); else if (K == 2) MW_YSM(2, 3); else MW_YSM(0, 3); }
    else             { if (K == 1) MW_YSM(1, 5); else if (K == 2) MW_YSM(2, 5); else MW_YSM(0, 5); }
#undef MW_YSM
    MW_LAUNCH_CHECK();
    return 0;
  }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    long long threads = (long long)p.nz * p.nx * p.nens;
    // measured on 400x400x100 (625 wave columns): 8 x 50 rows for k_y_state, 14 x 29 for k_y_tracers (-5 % / -2 % vs. 32-row chunks)
    int chunk = y_chunk(d, p, threads);
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)((p.ny + chunk - 1) / chunk));
    if (edges && p.ny >= 4 * MW_Y_EDGE) { chunk = -MW_Y_EDGE; grid.y = 2u; }      // (k_y_state: chunk < 0 = the two edge strips)
    double *MY = d->M[par][1] + e * v.m[1]; unsigned char *UY = d->UP[par][1] + e * v.m[1];
#define MW_YS(CONV_, K_, O_, cp, sw) MW_KLAUNCH((k_y_state<CONV_, K_, O_>), grid, dim3(256), 0, st, p, v.S(S), MY, UY, d->tendY + e * v.tend, chunk, cp, sw, YMember())
#define MW_YS_K(K_) { if (d->ord == 3) { if (conv) MW_YS(true, K_, 3, *conv, Sw); else MW_YS(false, K_, 3, CouplerPtrs(), nullptr); } \
                      else             { if (conv) MW_YS(true, K_, 5, *conv, Sw); else MW_YS(false, K_, 5, CouplerPtrs(), nullptr); } }
    double *Sw = const_cast<double *>(v.S(S));
    switch (marching_config(d, p)) { case 1: MW_YS_K(1) break; case 2: MW_YS_K(2) break; default: MW_YS_K(0) break; }
#undef MW_YS_K
#undef MW_YS
    MW_LAUNCH_CHECK();
  }
  return 0;
}

// part: 0 = all rows; 1 = the rows whose chunks read no halo row (all of them with the row wrap), 2 = the two edge strips of
// MW_Y_EDGE rows (short chunks: their launch runs between the exchange and k_xz_state, with a quarter of the wavefronts)
int launch_y_all(mw_dycore_s *d, const double *S, const CouplerPtrs *conv, int part, hipStream_t st) {
  if (!st) st = d->stream;
  ProfScope ps(d, 5, st);
  // the cells the pipelined schedule converted up front (time_step): the converting launch leaves them alone (see k_y_all)
  const int pre_lo = (conv && part == 1) ? d->pre_lo : 0, pre_hi = (conv && part == 1) ? d->pre_hi : 0;
  int fy_skip = 0;                                              // (set below where the inner launch shares its first / last face with the edge strips' launch)
  if (conv && d->member_major) {                                // mm_direct: all members in one launch, the members of the same cells in one workgroup
    const View v = view(d, 0);
    const DyP &p = v.p;
    if (!d->mm_direct || marching_config(d, p) == 0) MW_FAIL("internal: the converting k_y_all of a member-major handle exists for 2 or 4 members of a folded configuration only");
    const MemberOff mo = member_off(d);
    const long long mthreads = (long long)p.nz * p.nx;
    int chunk = y_chunk(d, p, mthreads);
    dim3 grid((unsigned)((mthreads + 64 * (4 / mo.n) - 1) / (64 * (4 / mo.n))), (unsigned)((p.ny + chunk - 1) / chunk));
    int row0 = 0, row_end = p.ny;
    if (part == 1 && !p.wrap_y) {                               // (pipelined schedule: the inner rows; the edge strips come from the slab later)
      const int n = (int)grid.y;
      row0 = MW_Y_EDGE; row_end = p.ny - MW_Y_EDGE; chunk = (row_end - row0 + n - 1) / n; grid.y = (unsigned)((row_end - row0 + chunk - 1) / chunk);
      fy_skip = 3;
    }
#define MW_YAM(K_, O_, T_) MW_KLAUNCH((k_y_all<true, K_, O_, T_, true>), grid, dim3(256), 0, st, p, S, d->FY, d->tendY, chunk, *conv, const_cast<double *>(S), mo, row0, chunk, row_end, pre_lo, pre_hi, fy_skip)
#define MW_YAM_O(K_, T_) { if (d->ord == 3) MW_YAM(K_, 3, T_); else MW_YAM(K_, 5, T_); }
    if (marching_config(d, p) == 1) MW_YAM_O(1, 3) else MW_YAM_O(2, 1)
#undef MW_YAM_O
#undef MW_YAM
    MW_LAUNCH_CHECK();
    return 0;
  }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    long long threads = (long long)p.nz * p.nx * p.nens;
    int chunk = y_chunk(d, p, threads);
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)((p.ny + chunk - 1) / chunk));
    int row0 = 0, rstride = chunk, row_end = p.ny;
    if (part) {
      const int n = (int)grid.y;
      const bool edges = !p.wrap_y;                             // the first / last rows read halo rows of the slab
      const bool split = p.ny >= 4 * MW_Y_EDGE;                 // (an inner chunk reads up to 3 rows beyond its own: MW_Y_EDGE >= 3)
      if (part == 1) {
        if (edges) { if (!split) continue; row0 = MW_Y_EDGE; row_end = p.ny - MW_Y_EDGE; chunk = (row_end - row0 + n - 1) / n; rstride = chunk;
                     grid.y = (unsigned)((row_end - row0 + chunk - 1) / chunk); fy_skip = 3; }
      } else {
        if (!edges) continue;
        if (split) { chunk = MW_Y_EDGE; rstride = p.ny - MW_Y_EDGE; grid.y = 2u; }
      }
    }
#define MW_YA(C_, K_, O_, T_) MW_KLAUNCH((k_y_all<C_, K_, O_, T_>), grid, dim3(256), 0, st, p, v.S(S), d->FY + e * v.f[1], d->tendY + e * v.tend, chunk, \
                                         conv ? *conv : CouplerPtrs(), const_cast<double *>(v.S(S)), MemberOff(), row0, rstride, row_end, pre_lo, pre_hi, fy_skip)
#define MW_YA_O(K_, T_) { if (conv) { if (d->ord == 3) MW_YA(true, K_, 3, T_); else MW_YA(true, K_, 5, T_); } \
                          else      { if (d->ord == 3) MW_YA(false, K_, 3, T_); else MW_YA(false, K_, 5, T_); } }
    const int K = marching_config(d, p);
    if (K == 1) MW_YA_O(1, 3)
    else if (K == 2) MW_YA_O(2, 1)
    else if (p.nt == 1) MW_YA_O(0, 1)
    else if (p.nt == 2) MW_YA_O(0, 2)
    else MW_YA_O(0, 3)
#undef MW_YA_O
#undef MW_YA
    MW_LAUNCH_CHECK();
  }
  return 0;
}

int launch_y_tracers(mw_dycore_s *d, const double *S, int par, hipStream_t st, bool edges) {
  if (d->p.sim2d) return 0;
  ProfScope ps(d, 6, st);
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    long long threads = (long long)p.nz * p.nx * p.nens;
    int chunk = d->chunk_yt ? d->chunk_yt : (d->chunk_yt = balanced_chunk(d, p.ny, (threads + 63) / 64, d->o.chunk_yt, 8400, 3, 5.0, (threads + 255) / 256 < 96));
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)((p.ny + chunk - 1) / chunk));
    if (edges && p.ny >= 4 * MW_Y_EDGE) { chunk = -MW_Y_EDGE; grid.y = 2u; }      // (k_y_tracers: chunk < 0 = the two edge strips)
    double *FY = d->FY + e * v.f[1];
    for (int t0 = 0; t0 < p.nt; t0 += 4) {
      int cnt = std::min(4, p.nt - t0);
      const double *M = d->M[par][1] + e * v.m[1]; const unsigned char *U = d->UP[par][1] + e * v.m[1];
#define MW_YT(T_) { if (d->ord == 3) MW_KLAUNCH((k_y_tracers<T_, 3>), grid, dim3(256), 0, st, p, v.S(S), FY, M, U, chunk, t0); \
                    else             MW_KLAUNCH((k_y_tracers<T_, 5>), grid, dim3(256), 0, st, p, v.S(S), FY, M, U, chunk, t0); }
      switch (cnt) { case 1: MW_YT(1) break; case 2: MW_YT(2) break; case 3: MW_YT(3) break; default: MW_YT(4) break; }
#undef MW_YT
      MW_LAUNCH_CHECK();
    }
  }
  return 0;
}
