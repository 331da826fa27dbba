// =====================================================================================================
// mw_march_tracers.hip -- launchers of the tracer-stage marching kernels of mw_march.h (k_xz_tracers, k_tracer_update, k_tracers_fused + k_tracer_patch): launch code only.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include "mw_march.h"

template <int T, bool N1>
static void launch_xz_tracers_t(mw_dycore_s *d, const double *S, dim3 grid, int chunk, int tiles_x, int t0, int par, double dt, int rows4,
                                hipStream_t st) {
  MW_KLAUNCH((k_xz_tracers<T, N1>), grid, dim3(256), 0, st, d->p, S, d->FX, d->FY, d->FZ, d->M[par][0], d->M[par][2], d->UP[par][0],
                     d->UP[par][2], dt, chunk, tiles_x, t0, rows4);
}

// tracer x/z fluxes + FCT (dt = the stage's dt, like k_fct)
int launch_xz_tracers(mw_dycore_s *d, const double *S, int par, double dt, hipStream_t st) {
  const DyP &p = d->p;
  ProfScope ps(d, 7, st);
  dim3 grid; int chunk, tiles_x;
  if (xz_grid(d, p, grid, chunk, tiles_x)) return 1;
  const int rows4 = p.ny >= 4 ? 1 : 0;                         // block = 4 rows of one x tile (shares the FY rows)
  if (rows4) grid.x = (unsigned)(((p.ny + 3) / 4) * tiles_x);
  for (int t0 = 0; t0 < p.nt; t0 += 4) {
    int cnt = std::min(4, p.nt - t0);
    if (p.nens == 1) {
      switch (cnt) { case 1: launch_xz_tracers_t<1, true>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     case 2: launch_xz_tracers_t<2, true>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     case 3: launch_xz_tracers_t<3, true>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     default: launch_xz_tracers_t<4, true>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break; }
    } else {
      switch (cnt) { case 1: launch_xz_tracers_t<1, false>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     case 2: launch_xz_tracers_t<2, false>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     case 3: launch_xz_tracers_t<3, false>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break;
                     default: launch_xz_tracers_t<4, false>(d, S, grid, chunk, tiles_x, t0, par, dt, rows4, st); break; }
    }
    MW_LAUNCH_CHECK();
  }
  return 0;
}

template <int STAGE, int MODE>
int launch_tracer_update(mw_dycore_s *d, const double *Sstar, const double *Sn, double *Sout, double dt_dyn, const CouplerPtrs &c,
                                hipStream_t st) {
  ProfScope ps(d, 2, st);
  const DyP &p = d->p;
  dim3 grid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz);
  MW_KLAUNCH((k_tracer_update<STAGE, MODE>), grid, dim3(256), 0, st, p, Sstar, Sn, Sout, d->FX, d->FY, d->FZ, dt_dyn, c);
  MW_LAUNCH_CHECK();
  return 0;
}

template <int STAGE, int MODE, int T, bool N1, int K, int ORD = 5, int VS = 0>
static void launch_tracers_fused_t(mw_dycore_s *d, const View &v, const double *S, const double *Sn, double *Sout, dim3 grid, int chunk, int tiles_x, int par,
                                   double dt, double dt_dyn, const CouplerPtrs &c, int rows4, hipStream_t st, int vap_slot) {
  const int e = v.e;
  // (VS, option lean_stores: where the previous fused launch's word lies, seen from this launch's -- the two alternate; see the kernel)
  const int prev_word = !d->o.lean_stores ? 0 : (d->fused_launches & 1) ? 2 : 1;
  MW_KLAUNCH((k_tracers_fused<STAGE, MODE, T, N1, K, ORD, false, VS>), grid, dim3(256), 0, st, v.p, v.S(S), v.S(Sn), v.S(Sout), d->FY + e * v.f[1],
                     d->M[par][0] + e * v.m[0], d->M[par][2] + e * v.m[2], d->UP[par][0] + e * v.m[0], d->UP[par][2] + e * v.m[2],
                     d->FX + e * v.f[0], d->FZ + e * v.f[2], d->flags + e * v.cells, d->dirty + (d->fused_launches & 1), dt, dt_dyn, c, chunk, tiles_x, rows4, MemberOff(),
                     VS ? d->dirty + MW_VREDO_RING : nullptr, VS ? vap_slot + 8 * prev_word : 0);
}
// x/z tracer fluxes + FCT + update in one kernel, then the (normally empty) y-face correction
template <int STAGE, int MODE>
int launch_tracers_fused(mw_dycore_s *d, const double *S, const double *Sn, double *Sout, int par, double dt, double dt_dyn,
                                const CouplerPtrs &c, hipStream_t st, int vap_slot) {
  {
    ProfScope ps(d, 7, st);
    bool direct = false;
    if constexpr (STAGE == 3 && MODE == 1) direct = d->mm_direct;
    if constexpr (STAGE == 3 && MODE == 1) if (direct) {            // all members in one launch (MemberOff): workgroup = nens members x 4 / nens rows of a tile
      const View v = view(d, 0);
      const DyP &p = v.p;
      const MemberOff mo = member_off(d);
      const int U = 64 - 2 * ((d->ord - 1) / 2 + 1), tiles_x = (p.nx + U - 1) / U, rpb = 4 / mo.n;
      const long long waves = (long long)p.ny * tiles_x;
      const int chunk = d->chunk_f ? d->chunk_f : (d->chunk_f = balanced_chunk(d, p.nz, waves, d->o.chunk_f, 10000, 2, 4.5, true));
      dim3 grid((unsigned)(((p.ny + rpb - 1) / rpb) * tiles_x), (unsigned)((p.nz + chunk - 1) / chunk));
#define MW_FUSED_MT(TT) case TT: MW_FUSED_MTK(TT, 0) break;
#define MW_FUSED_MTK(TT, K_) { if (d->ord == 3) MW_FUSED_MTO(TT, K_, 3); else MW_FUSED_MTO(TT, K_, 5); }
#define MW_FUSED_MTO(TT, K_, O_) MW_KLAUNCH((k_tracers_fused<3, 1, TT, true, K_, O_, true>), grid, dim3(256), 0, st, p, S, Sn, Sout, d->FY, d->M[par][0], d->M[par][2], \
                                 d->UP[par][0], d->UP[par][2], d->FX, d->FZ, d->flags, d->dirty + (d->fused_launches & 1), dt, dt_dyn, c, chunk, tiles_x, 0, mo, nullptr, 0)
      if (marching_config(d, p) == 1) MW_FUSED_MTK(3, 1)
      else switch (p.nt) { MW_FUSED_MT(1) MW_FUSED_MT(2) MW_FUSED_MT(3) MW_FUSED_MT(4) default: MW_FAIL("fused tracer stage needs 1..4 tracers"); }
#undef MW_FUSED_MT
#undef MW_FUSED_MTK
#undef MW_FUSED_MTO
      MW_LAUNCH_CHECK();
    }
    for (int e = 0; e < (direct ? 0 : n_views(d)); e++) {
      const View v = view(d, e);
      const DyP &p = v.p;
      const int U = p.nens == 1 ? 64 - 2 * ((d->ord - 1) / 2 + 1) : 64 - 4 * p.nens;   // hs + 1 / 2 halo cells per side (k_tracers_fused)
      const int tiles_x = (p.nx * p.nens + U - 1) / U;
      const int rows4 = (p.ny >= 4 && d->o.tf_rows4) ? 1 : 0;   // (workgroup = 4 rows of one x tile: the rows' shared y faces meet in L1; option tf_rows4 = 0: 4 x tiles of one row, A/B)
      const long long waves = (long long)p.ny * tiles_x;
      const int chunk = d->chunk_f ? d->chunk_f : (d->chunk_f = balanced_chunk(d, p.nz, waves, d->o.chunk_f, 10000, 2, 4.5, true));
      dim3 grid(rows4 ? (unsigned)(((p.ny + 3) / 4) * tiles_x) : (unsigned)((waves + 3) / 4), (unsigned)((p.nz + chunk - 1) / chunk));
#define MW_FUSED_ARGS d, v, S, Sn, Sout, grid, chunk, tiles_x, par, dt, dt_dyn, c, rows4, st, vap_slot
#define MW_FUSED_CASE(TT) \
      case TT: if (p.nens != 1)     launch_tracers_fused_t<STAGE, MODE, TT, false, 0>(MW_FUSED_ARGS); \
               else if (d->ord == 3) launch_tracers_fused_t<STAGE, MODE, TT, true, 0, 3>(MW_FUSED_ARGS); \
               else                  launch_tracers_fused_t<STAGE, MODE, TT, true, 0>(MW_FUSED_ARGS); break;
      const int K = marching_config(d, p);
      if (K == 1 && vap_slot >= 0) {                               // the vapour was advanced by k_xz_state<.., VAP>: cloud and rain here, or the redo
        launch_tracers_fused_t<STAGE, MODE, 3, true, 1, 5, 1>(MW_FUSED_ARGS); }
      else if (K == 1) { if (d->ord == 3) launch_tracers_fused_t<STAGE, MODE, 3, true, 1, 3>(MW_FUSED_ARGS); else launch_tracers_fused_t<STAGE, MODE, 3, true, 1>(MW_FUSED_ARGS); }
      else if (K == 2) { if (d->ord == 3) launch_tracers_fused_t<STAGE, MODE, 1, true, 2, 3>(MW_FUSED_ARGS); else launch_tracers_fused_t<STAGE, MODE, 1, true, 2>(MW_FUSED_ARGS); }
      else switch (p.nt) { MW_FUSED_CASE(1) MW_FUSED_CASE(2) MW_FUSED_CASE(3) MW_FUSED_CASE(4) default: MW_FAIL("fused tracer stage needs 1..4 tracers"); }
#undef MW_FUSED_CASE
#undef MW_FUSED_ARGS
      MW_LAUNCH_CHECK();
    }
  }
  const DyP &p = d->p;
  if (!p.sim2d && p.pos_mask && !d->o.debug_no_patch) {   // (the switch exists for the negative control in tests/)
    ProfScope ps(d, 1, st);
    for (int e = 0; e < n_views(d); e++) {
      const View v = view(d, e);
      const DyP &q = v.p;
      // (member-major: every member's launch reads the same `dirty` word; only the last one may clear the next stage's word)
      unsigned int *next = (e == n_views(d) - 1) ? d->dirty + ((d->fused_launches + 1) & 1) : d->dirty + 2;
      MW_KLAUNCH((k_tracer_patch<STAGE, MODE>), plane_grid((long long)q.ny * ((q.nx * q.nens + MW_PATCH_CELLS - 1) / MW_PATCH_CELLS), q.nz), dim3(256), 0, st, q,
                         v.S(Sout), d->flags + e * v.cells, d->FX + e * v.f[0], d->FZ + e * v.f[2], dt_dyn, c, d->dirty + (d->fused_launches & 1), next);
      MW_LAUNCH_CHECK();
    }
  } else if (!p.sim2d && p.pos_mask) {                          // (negative-control switch) nobody else clears the next word
    (void)hipMemsetAsync(d->dirty + ((d->fused_launches + 1) & 1), 0, sizeof(unsigned int), st);
  }
  d->fused_launches++;
  return 0;
}

// the four (STAGE, MODE) of an SSPRK3 cycle (rk_stage_march / rk_stage_pipe in mw_march_sched.hip)
template int launch_tracer_update<1, 0>(mw_dycore_s *, const double *, const double *, double *, double, const CouplerPtrs &, hipStream_t);
template int launch_tracers_fused<1, 0>(mw_dycore_s *, const double *, const double *, double *, int, double, double, const CouplerPtrs &, hipStream_t, int);
template int launch_tracer_update<2, 0>(mw_dycore_s *, const double *, const double *, double *, double, const CouplerPtrs &, hipStream_t);
template int launch_tracers_fused<2, 0>(mw_dycore_s *, const double *, const double *, double *, int, double, double, const CouplerPtrs &, hipStream_t, int);
template int launch_tracer_update<3, 0>(mw_dycore_s *, const double *, const double *, double *, double, const CouplerPtrs &, hipStream_t);
template int launch_tracers_fused<3, 0>(mw_dycore_s *, const double *, const double *, double *, int, double, double, const CouplerPtrs &, hipStream_t, int);
template int launch_tracer_update<3, 1>(mw_dycore_s *, const double *, const double *, double *, double, const CouplerPtrs &, hipStream_t);
template int launch_tracers_fused<3, 1>(mw_dycore_s *, const double *, const double *, double *, int, double, double, const CouplerPtrs &, hipStream_t, int);
