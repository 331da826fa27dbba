// =====================================================================================================
// mw_march_xz.hip -- launcher of the x/z state marching kernel of mw_march.h (k_xz_state): launch code only.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include "mw_march.h"

int xz_grid(mw_dycore_s *d, const DyP &p, dim3 &grid, int &chunk, int &tiles_x) {
  int U = xz_cells_per_wave(p.nens, d->ord);
  if (U < 4) MW_FAIL("nens too large for the 64-lane x tiling (need nens <= 30)");
  tiles_x = (p.nx * p.nens + U - 1) / U;
  long long waves = (long long)p.ny * tiles_x;
  if (!d->chunk_z) {
    // k_xz_state: equal chunks, enough of them for ~5 rounds of 2 waves/SIMD over the 1024 SIMDs (measured on 400x400x100:
    // 4 x 25 levels beats 32,32,32,4 by 4 %)
    d->chunk_z = balanced_chunk(d, p.nz, waves, d->o.chunk_z, 10000, 2, 2.5, true);
    // k_xz_state<.., HPL = 1> keeps (chunk + 2) rows of 64 bytes in dynamic LDS: stay well inside the 64 KB a workgroup may have
    d->chunk_z = std::min(d->chunk_z, 900);
  }
  chunk = d->chunk_z;
  grid = dim3((unsigned)((waves + 3) / 4), (unsigned)((p.nz + chunk - 1) / chunk));
  return 0;
}

template <int STAGE, int MODE>
int launch_xz_state(mw_dycore_s *d, const double *S, const double *Sn, double *Sout, double dt_stage, double dt_dyn, int par,
                           const CouplerPtrs &c, int vap_slot) {
  ProfScope ps(d, 0);
  if constexpr (STAGE == 3 && MODE == 1) {
    if (d->mm_direct) {                                         // all members in one launch: workgroup = the nens members of 4 / nens tiles
      const View v = view(d, 0);
      const DyP &p = v.p;
      dim3 grid; int chunk, tiles_x;
      if (xz_grid(d, p, grid, chunk, tiles_x)) return 1;
      const MemberOff mo = member_off(d);
      const int wpb = 4 / mo.n;
      grid.x = (unsigned)(((long long)p.ny * tiles_x + wpb - 1) / wpb);
      // one background table per wave here: (chunk + 2) x 256 B of dynamic LDS on top of the kernel's ~20.5 KB of static LDS must fit
      // the 64 KB a workgroup may have -- shorter chunks for this launch when nz is large and the chunk rule asks for one long chunk
      { const int cap = (65536 - 21504) / 256 - 2;               // 170 levels
        if (chunk > cap) { chunk = cap; grid.y = (unsigned)((p.nz + chunk - 1) / chunk); } }
      const size_t lds = (size_t)(chunk + 2) * 64 * 4;
#define MW_XZ_MT(K_) { if (d->ord == 3) MW_XZ_MTO(K_, 3); else MW_XZ_MTO(K_, 5); }
#define MW_XZ_MTO(K_, O_) MW_KLAUNCH((k_xz_state<3, true, 1, 1, K_, O_, true>), grid, dim3(256), lds, d->stream, p, S, Sn, Sout, d->M[par][0], d->M[par][2], \
                                        d->UP[par][0], d->UP[par][2], d->tendY, dt_stage, dt_dyn, chunk, tiles_x, c.u, c.v, c.w, mo, XzVap())
      if (marching_config(d, p) == 1) MW_XZ_MT(1) else MW_XZ_MT(0)
#undef MW_XZ_MT
#undef MW_XZ_MTO
      MW_LAUNCH_CHECK();
      return 0;
    }
  }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    dim3 grid; int chunk, tiles_x;
    if (xz_grid(d, p, grid, chunk, tiles_x)) return 1;
    double *MX = d->M[par][0] + e * v.m[0], *MZ = d->M[par][2] + e * v.m[2], *tY = d->tendY + e * v.tend;
    unsigned char *UX = d->UP[par][0] + e * v.m[0], *UZ = d->UP[par][2] + e * v.m[2];
    // nens == 1 (also: one member of a member-major handle): the per-level background values come through LDS
    // (k_xz_state<.., HPL = 1>; dynamic LDS = the chunk's rows)
#define MW_XZ(N1_, HPL_, K_, O_, lds) MW_KLAUNCH((k_xz_state<STAGE, N1_, MODE, HPL_, K_, O_>), grid, dim3(256), (lds), d->stream, p, v.S(S), v.S(Sn), v.S(Sout), \
                                                 MX, MZ, UX, UZ, tY, dt_stage, dt_dyn, chunk, tiles_x, c.u, c.v, c.w, MemberOff(), XzVap())
#define MW_XZ_K(K_) { if (d->ord == 3) MW_XZ(true, 1, K_, 3, hpl_bytes); else MW_XZ(true, 1, K_, 5, hpl_bytes); }
    const size_t hpl_bytes = (size_t)(chunk + 2) * 64;
    if (vap_slot >= 0) {
      // the water vapour rides along (rk_stage_march decided: K = 1, nens == 1, WENO-5, behind k_y_all): its per-thread carries behind the table rows
      XzVap va = {d->FY + (long long)5 * p.fyV, c.tr[0], c.rho_d, c.temp, d->dirty + MW_VREDO_RING + vap_slot, d->o.lean_stores ? 1 : 0};
      const size_t lds = hpl_bytes + (size_t)(5 + 5) * 256 * sizeof(double);   // (five carry slots + the five slots of the window ring)
#define MW_XZ_VAP() MW_KLAUNCH((k_xz_state<STAGE, true, MODE, 1, 1, 5, false, true>), grid, dim3(256), lds, d->stream, p, v.S(S), v.S(Sn), v.S(Sout), \
                               MX, MZ, UX, UZ, tY, dt_stage, dt_dyn, chunk, tiles_x, c.u, c.v, c.w, MemberOff(), va)
      MW_XZ_VAP();
      // (test aid debug_vapour_redo: the stage's word set by hand, so that the tracer stage redoes a vapour that needs no redo)
      if (d->o.debug_vapour_redo) MW_HIP(hipMemsetAsync(d->dirty + MW_VREDO_RING + vap_slot, 0xFF, sizeof(unsigned int), d->stream));
      // (lean stores with maps: the launch above may have left out what a redo reads -- the replay launch stores it when the stage's word is set)
      if (va.lean && p.zq != nullptr && p.zero_skip) { MW_LAUNCH_CHECK(); va.lean = 2; MW_XZ_VAP(); }
#undef MW_XZ_VAP
    } else
    if (p.nens == 1) {
      switch (marching_config(d, p)) { case 1: MW_XZ_K(1) break; case 2: MW_XZ_K(2) break; default: MW_XZ_K(0) break; }
    } else MW_XZ(false, 0, 0, 5, 0);                          // (the fused-layout form for nens > 1: WENO-5 only, see time_step)
#undef MW_XZ_K
#undef MW_XZ
    MW_LAUNCH_CHECK();
  }
  return 0;
}

// the four (STAGE, MODE) of an SSPRK3 cycle (rk_stage_march / rk_stage_pipe in mw_march_sched.hip)
template int launch_xz_state<1, 0>(mw_dycore_s *, const double *, const double *, double *, double, double, int, const CouplerPtrs &, int);
template int launch_xz_state<2, 0>(mw_dycore_s *, const double *, const double *, double *, double, double, int, const CouplerPtrs &, int);
template int launch_xz_state<3, 0>(mw_dycore_s *, const double *, const double *, double *, double, double, int, const CouplerPtrs &, int);
template int launch_xz_state<3, 1>(mw_dycore_s *, const double *, const double *, double *, double, double, int, const CouplerPtrs &, int);
