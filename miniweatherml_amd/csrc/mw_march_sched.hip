// =====================================================================================================
// mw_march_sched.hip -- the schedules of an RK stage on the marching kernels (one stream, two streams, pipelined), the zero-row maps and the
// coupler <-> slab conversion passes.  The one unit that compiles the non-template kernels of mw_march.h.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#define MW_MARCH_SCHED_KERNELS
#include "mw_march.h"
#include <cstring>

// ---------------------------------------------------------------------------------------------------------------------
// One RK stage on the production path, as two pipelines on two HIP streams:
//   state stream  (the handle's stream): halo(state vars) -> k_y_state -> k_xz_state        [fp64-VALU bound]
//   tracer stream (side stream)        : halo(tracers) -> k_y_tracers -> k_tracers_fused -> k_tracer_patch                 [fp64-VALU bound too]
// The state variables of stage s+1 depend only on the state variables of stage s, so the state pipeline runs ahead
// while the tracer pipeline of stage s fills the memory system beside it.  Hand-offs: the tracer kernels need the
// mass fluxes / selectors / new density of their stage (event ev_state); the state pipeline may not run more than
// one stage ahead because the M/UP buffers are double-buffered and the four slabs rotate (event ev_tr of stage s-2).
// ---------------------------------------------------------------------------------------------------------------------
static void zero_rows_stage(mw_dycore_s *d, int stage);
static void zero_rows_conv(mw_dycore_s *d, const double *S, bool done, hipStream_t st);
static int zero_rows_build(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st, bool first_cycle);
static bool zero_rows_ok(const mw_dycore_s *d);
static int zero_rows_local(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st);
static int zero_rows_merge(mw_dycore_s *d, hipStream_t st, bool first_cycle);
// Option zero_verify (test aid): the maps' claims against the data, on stream `st`, in front of the launches that rely on them.
//   what = 0: in front of the stage's tracer kernel -- the stage's input slab against Qs / QYs, the destination (slab Sout, or the coupler's
//             arrays in the last stage of a time step) against the "holds zeros already" map the kernel was handed;
//   what = 1: in front of the converting y launch -- the slab it fills against zqk.
// Uses the parameter block as the next launch will see it (zero_rows_stage / zero_rows_conv have run).  Counters: mw_debug_zero_violations.
static int zero_rows_verify(mw_dycore_s *d, int what, const double *Sin, const double *Sout, bool dst_coupler, const CouplerPtrs &c, hipStream_t st) {
  if (!d->o.zero_verify || !d->zr_on) return 0;
  if (!d->zviol) { MW_HIP(hipMalloc(&d->zviol, 4 * sizeof(unsigned long long))); MW_HIP(hipMemsetAsync(d->zviol, 0, 4 * sizeof(unsigned long long), st)); }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    if (what == 0 && !p.zq) continue;
    if (what == 1 && !p.zqk) continue;
    const unsigned vmask = (marching_config(d, p) == 1) ? 0x6u : 0xFu;
    const long long nrow = (long long)p.nz * p.ny;
    const bool dstc = what == 0 && dst_coupler && p.zqc != nullptr;
    const double *dst = (what == 0 && !dst_coupler && p.zqp) ? v.S(Sout) : nullptr;
    MW_KLAUNCH(k_zero_verify, dim3((unsigned)((nrow + 3) / 4)), dim3(256), 0, st, p, c, what == 0 ? v.S(Sin) : nullptr, dst, dstc ? 1 : 0,
               what == 1 ? v.S(Sin) : nullptr, d->zr_msz, vmask, d->zviol);
    MW_LAUNCH_CHECK();
  }
  return 0;
}
template <int STAGE, int MODE>
static int rk_stage_march(mw_dycore_s *d, double *Sin, const double *Sn, double *Sout, double dt_stage, double dt_dyn,
                          const CouplerPtrs &c) {
  const long long gs = d->gstage++;
  const int par = (int)(gs & 1), slot = (int)(gs & 7);
  hipStream_t ss = d->stream, ts = d->overlap ? d->tstream : d->stream;
  const int T = d->p.nt;
  zero_rows_stage(d, STAGE);
  ProfScope stage_scope(d, 8, ss);                            // one-stream schedule: first launch to last launch of the stage
  if (d->overlap && gs >= 2) MW_HIP(hipStreamWaitEvent(ss, d->ev_tr[(gs - 2) & 7], 0));
  // ---- state pipeline
  if (halo_fill(d, Sin, 0, 5, ss, 0, true)) return 1;
  const bool conv = (STAGE == 1) && d->conv_pending;            // first stage of the step: D1 + D2 inside k_y_state
  d->conv_pending = false;
  // (the converting launch of a member-major handle exists in the members-in-one-workgroup form of the folded configurations only)
  const bool mm_conv_ok = d->mm_direct && d->o.mm_conv && marching_config(d, view(d, 0).p) != 0;
  const bool yall = y_all_ok(d) && !(conv && ((d->member_major && !mm_conv_ok) || !d->o.y_all_conv));   // y faces of state variables and tracers in one launch
  if (STAGE == 1) { if (conv) zero_rows_conv(d, Sin, false, ss); else zero_rows_forget(d, Sin); }   // (what is known about the rows of the slab that is about to be written)
  if (STAGE == 3 && MODE == 0) zero_rows_forget(d, Sout);
  // The water vapour rides along in k_xz_state (option vapour_state): the folded supercell configuration with nens == 1 and WENO-5 on this schedule's
  // one-stream form, behind k_y_all (the vapour's y fluxes are complete before the x/z launch starts) and in front of the fused tracer stage.
  const bool vap = yall && d->o.vapour_state && d->fused && !d->overlap && !d->member_major && d->p.nens == 1 && d->ord == 5 && marching_config(d, d->p) == 1;
  const int vap_slot = vap ? slot : -1;
  {
  if (conv && zero_rows_verify(d, 1, Sin, nullptr, false, c, ss)) return 1;
  if (yall) { if (halo_fill(d, Sin, 5, T, ts, 1, true) || launch_y_all(d, Sin, conv ? &c : nullptr)) return 1; }
  else if (launch_y_state(d, Sin, par, conv ? &c : nullptr)) return 1;             // y faces: m_upw, selector, y tendencies
  if (STAGE == 1 && conv) zero_rows_conv(d, Sin, true, ss);
  if (vap) {
    // (the word of stage gs is cleared by the tracer kernel of stage gs - 1 when that stage ran this form too; otherwise here)
    if (d->vap_last_gs != gs - 1) MW_HIP(hipMemsetAsync(d->dirty + MW_VREDO_RING + slot, 0, sizeof(unsigned int), ss));
    d->vap_last_gs = gs; d->vap_used = true;
  }
  if (launch_xz_state<STAGE, MODE>(d, Sin, Sn, Sout, dt_stage, dt_dyn, par, c, vap_slot)) return 1;   // x,z faces + finished state variables (+ the vapour)
  }
  if (STAGE == 1 && d->member_major && !d->overlap) {           // the members' maps, from the slab the y launch has just completed
    if (zero_rows_build(d, Sin, c, false, ss, d->first_cycle)) return 1;
    zero_rows_stage(d, 1);
  }
  // ---- tracer pipeline.  Its halo fill (and, on several ranks, its strip exchange over RCCL) only needs the tracer values of the
  // previous stage, which this stream produced itself: it is issued BEFORE the wait for this stage's state kernels and so
  // runs beside them; the state stream's exchange for stage s+1 in turn runs beside this stage's tracer kernels.
  // (Measured, round 3 -- profiles/r03_ab_two_stream_yt_beside_xz.txt: letting k_y_tracers start right behind k_y_state, BESIDE
  //  k_xz_state (an HBM-bound launch beside a VALU-bound one), stretches both and leaves the step where it was: 5.62-5.74 ms against
  //  5.51-5.70 on one stream.  The step as a whole moves 26 GB at 4.8 TB/s: there is no idle HBM time for a second kernel to use.)
  if (!yall && halo_fill(d, Sin, 5, T, ts, 1, true)) return 1;
  if (d->overlap) { MW_HIP(hipEventRecord(d->ev_state[slot], ss)); MW_HIP(hipStreamWaitEvent(ts, d->ev_state[slot], 0)); }
  if (!yall && launch_y_tracers(d, Sin, par, ts)) return 1;                   // tracer fluxes (public arrays)
  if (d->fused) {
    if (zero_rows_verify(d, 0, Sin, Sout, MODE == 1, c, ts)) return 1;
    if (launch_tracers_fused<STAGE, MODE>(d, Sin, Sn, Sout, par, dt_stage, dt_dyn, c, ts, vap_slot)) return 1;   // x/z fluxes + D10 + D11/D12 (+ D13)
  } else {
    if (launch_xz_tracers(d, Sin, par, dt_stage, ts)) return 1;               // x/z fluxes + D10 (FCT)
    if (launch_tracer_update<STAGE, MODE>(d, Sin, Sn, Sout, dt_dyn, c, ts)) return 1;
  }
  if (d->overlap) MW_HIP(hipEventRecord(d->ev_tr[slot], ts));
  return 0;
}
// ---------------------------------------------------------------------------------------------------------------------
// One RK stage of a block of a decomposed domain, PIPELINED schedule (the default with a neighbour exchange when k_y_all applies):
// one compute stream, and the strip exchange of a stage on the side stream BESIDE interior work that does not need it:
//   compute : k_y_all(chunks without halo rows) | wait | k_y_all(first + last chunk) -> k_xz_state -> k_tracers_fused (+ patch)
//   exchange:   [strips of this stage's input ]         after k_xz_state: state strips of the NEXT stage's input (beside
//                                                       k_tracers_fused); after k_tracers_fused: its tracer strips (beside the next
//                                                       stage's interior k_y_all)
// The y marching kernel reads no x halo at all and y halo rows only in its first and last chunk, so six of eight chunks start at
// once.  The first stage of a cycle exchanges all variables at its start (its input comes from the conversion pass / the previous
// cycle).  Compared with the two-stream schedule of rk_stage_march (each pipeline hides the other's exchange behind whole kernels)
// this one keeps k_y_all -- 5 % of the step -- and needs less machinery; the transfer must fit beside ~0.3-0.5 ms of kernels.
// ---------------------------------------------------------------------------------------------------------------------
template <int STAGE, int MODE>
static int rk_stage_pipe(mw_dycore_s *d, double *Sin, const double *Sn, double *Sout, double dt_stage, double dt_dyn, const CouplerPtrs &c) {
  const long long gs = d->gstage++;
  const int par = (int)(gs & 1);
  hipStream_t ss = d->stream, xs = d->tstream;
  const int T = d->p.nt;
  ProfScope stage_scope(d, 8, ss);
  const bool conv = (STAGE == 1) && d->conv_pending;            // the inner rows come from the coupler's arrays (see time_step)
  d->conv_pending = false;
  // (round 4: the two edge strips of the y launch run on the EXCHANGE stream right behind the unpack kernels -- beside the inner rows on
  //  the compute stream -- instead of behind them: a launch of 2 x 157 workgroups no longer sits alone between k_y_all and k_xz_state)
  const bool edge_side = !d->o.pipe_edge_inline;
  // (round 5: the edge strips of the NEXT stage's y launch are SPLIT by what they wait for.  Their state part -- y tendencies of the edge
  //  rows, k_y_state -- only needs the state strips, which travel beside this stage's tracer kernel: it runs right behind them, and
  //  k_xz_state of the next stage waits for nothing else.  Their tracer part -- the tracer y fluxes of the edge faces, k_y_tracers, which
  //  only the next stage's TRACER kernel reads -- runs behind the tracer strips and has the next stage's inner y rows AND its k_xz_state
  //  to hide behind.  Before, k_xz_state waited for the whole tracer chain (pack, group, unpack, edge launch: 0.3-0.4 ms of idle compute
  //  stream per stage in the rocprofv3 timeline of the self-loop transport).  pipe_split_edges = 0: one k_y_all edge launch
  //  behind the tracer strips, as in rounds 3-4.)
  const bool split_edges = edge_side && d->o.pipe_split_edges;
  const int par_next = (int)((gs + 1) & 1);
  // (round 5, first stage with the split edge strips: LOCAL zero-row maps on the compute stream in front of the y launches, the state strips
  //  and the tracer strips as two exchanges -- k_xz_state waits for the first only -- and the neighbours' maps merged in behind them; before,
  //  this stage's y launch ran without maps, 664 against 476 us, in front of one 609 us exchange chain for all eight variables)
  bool maps_early = false;
  // (every rank must take the same branch here -- it posts a different number and size of exchanges -- so the size test looks at the
  //  SMALLEST block of the decomposition, as zero_rows_ok does: blocks of 15 and 16 rows (ny_glob = 31 on two y ranks) would otherwise
  //  straddle the threshold and post mismatched send / receive groups)
  const long long ny_min_blk = d->g.ny_glob / std::max(1, d->p.nproc_y);
  if (!d->pipe_ready && STAGE == 1 && split_edges && d->o.pipe_maps_early && !d->p.wrap_y && ny_min_blk >= 4 * MW_Y_EDGE && zero_rows_ok(d)) {   // (a y-decomposed block with real edge strips)
    maps_early = true;
    // the local maps on the exchange stream: from the coupler's arrays they only need the step's inputs and run BESIDE the strip conversion
    // on the compute stream (first sub-cycle); from the slab they wait for it like everything else
    const bool beside = conv && d->first_cycle && d->entry_marked;
    MW_HIP(hipEventRecord(d->ev_pipe[0], ss));
    MW_HIP(hipStreamWaitEvent(xs, beside ? d->ev_pipe[6] : d->ev_pipe[0], 0));
    if (zero_rows_local(d, Sin, c, conv, xs)) return 1;
    MW_HIP(hipEventRecord(d->ev_pipe[5], xs));
    MW_HIP(hipStreamWaitEvent(ss, d->ev_pipe[5], 0));         // the stage's inner y rows read them
    if (beside) MW_HIP(hipStreamWaitEvent(xs, d->ev_pipe[0], 0));
    if (halo_fill(d, Sin, 0, 5, xs, 0, true)) return 1;
    if (launch_y_state(d, Sin, par, nullptr, true, xs)) return 1;
    MW_HIP(hipEventRecord(d->ev_pipe[2], xs));
    if (halo_fill(d, Sin, 5, T, xs, 1, true)) return 1;
    if (launch_y_tracers(d, Sin, par, xs, true)) return 1;
    MW_HIP(hipEventRecord(d->ev_pipe[3], xs));
    d->pipe_edge_done = true;
    if (zero_rows_merge(d, xs, d->first_cycle)) return 1;
    if (d->zr_on) MW_HIP(hipEventRecord(d->ev_pipe[4], xs));
    zero_rows_stage(d, 1);                                      // the local maps, for this stage's inner y rows
    if (conv) zero_rows_conv(d, Sin, false, ss); else zero_rows_forget(d, Sin);
  } else
  if (!d->pipe_ready) {                                       // this stage's input has not been exchanged yet
    MW_HIP(hipEventRecord(d->ev_pipe[0], ss)); MW_HIP(hipStreamWaitEvent(xs, d->ev_pipe[0], 0));
    if (halo_fill(d, Sin, 0, -1, xs, 0, true)) return 1;
    if (edge_side && launch_y_all(d, Sin, nullptr, 2, xs)) return 1;
    MW_HIP(hipEventRecord(d->ev_pipe[2], xs));
    MW_HIP(hipEventRecord(d->ev_pipe[3], xs));
    d->pipe_edge_done = edge_side;
    if (STAGE == 1) {                                           // the sub-cycle's zero-row maps, behind the strips: needed by the tracer kernel only
      if (zero_rows_build(d, Sin, c, conv, xs, d->first_cycle)) return 1;
      if (conv) zero_rows_conv(d, Sin, true, xs); else zero_rows_forget(d, Sin);
      if (d->zr_on) MW_HIP(hipEventRecord(d->ev_pipe[4], xs));
    }
  }
  if (STAGE != 1) zero_rows_stage(d, STAGE);                    // (stage 1 without the early maps: its y launches run BESIDE the map build -- the maps are handed over in front of the tracer kernel)
  if (STAGE == 3 && MODE == 0) zero_rows_forget(d, Sout);
  d->pipe_ready = false;
  if (conv && zero_rows_verify(d, 1, Sin, nullptr, false, c, ss)) return 1;
  if (launch_y_all(d, Sin, conv ? &c : nullptr, 1)) return 1;  // rows whose chunks read no halo row
  { ProfScope wait_scope(d, 10, ss);                           // (profile class 10: how long the compute stream sits in this wait)
    MW_HIP(hipStreamWaitEvent(ss, d->ev_pipe[2], 0)); }        // state strips (+ the edge rows' y tendencies) of this stage's input
  if (!d->pipe_edge_done && launch_y_all(d, Sin, nullptr, 2)) return 1;   // first and last chunk
  d->pipe_edge_done = false;
  if (launch_xz_state<STAGE, MODE>(d, Sin, Sn, Sout, dt_stage, dt_dyn, par, c)) return 1;
  const bool early = (STAGE < 3);                             // the next stage of this cycle reads Sout
  if (early) {
    MW_HIP(hipEventRecord(d->ev_pipe[0], ss)); MW_HIP(hipStreamWaitEvent(xs, d->ev_pipe[0], 0));
    if (halo_fill(d, Sout, 0, 5, xs, 0, true)) return 1;      // state strips, beside the tracer stage
    if (split_edges) {
      if (launch_y_state(d, Sout, par_next, nullptr, true, xs)) return 1;   // ... and the state part of the NEXT stage's edge strips right behind them
      MW_HIP(hipEventRecord(d->ev_pipe[2], xs));
    }
  }
  { ProfScope wait_scope(d, 11, ss);                           // (profile class 11)
    MW_HIP(hipStreamWaitEvent(ss, d->ev_pipe[3], 0)); }        // tracer strips + the edge faces' tracer fluxes of this stage's input
  if (STAGE == 1 && d->zr_on) {
    MW_HIP(hipStreamWaitEvent(ss, d->ev_pipe[4], 0)); zero_rows_stage(d, 1);
    if (maps_early && conv) zero_rows_conv(d, Sin, true, ss);     // (the slab's row map changes BEHIND the converting launch that reads it)
  }
  if (zero_rows_verify(d, 0, Sin, Sout, MODE == 1, c, ss)) return 1;
  if (launch_tracers_fused<STAGE, MODE>(d, Sin, Sn, Sout, par, dt_stage, dt_dyn, c, ss)) return 1;
  if (early) {
    MW_HIP(hipEventRecord(d->ev_pipe[1], ss)); MW_HIP(hipStreamWaitEvent(xs, d->ev_pipe[1], 0));
    if (halo_fill(d, Sout, 5, T, xs, 1, true)) return 1;      // tracer strips, beside the next stage's interior y chunks (and, split, its k_xz_state)
    if (split_edges) { if (launch_y_tracers(d, Sout, par_next, xs, true)) return 1; }                    // the tracer part of the next stage's edge strips
    else if (edge_side) { zero_rows_stage(d, STAGE + 1); if (launch_y_all(d, Sout, nullptr, 2, xs)) return 1; }   // ... or both parts in one launch (the NEXT stage's maps)
    if (!split_edges) MW_HIP(hipEventRecord(d->ev_pipe[2], xs));
    MW_HIP(hipEventRecord(d->ev_pipe[3], xs));
    d->pipe_ready = true; d->pipe_edge_done = edge_side;
  }
  return 0;
}
// Zero-row maps (mw_march.h: k_zero_rows).  Which handles: nens == 1, fused tracer stage, x and y periodic; one rank on the one-stream
// schedule, or the blocks of a decomposed domain on the pipelined schedule.  The ranks of a decomposed domain exchange maps, so all of
// them must decide alike: the size test looks at the smallest block of the decomposition, not at this rank's.
static bool zero_rows_ok(const mw_dycore_s *d) {
  const DyP &p = d->p;
  // (nens > 1: the member-major layout on one rank -- every member has its own maps and the per-member launches read them; the launches
  //  that hold all members of a tile in one workgroup run without)
  if (!(d->o.zero_skip && d->o.zero_rows && d->fused && (p.nens == 1 || (d->member_major && !d->xchg)) && p.nt >= 1 && p.nt <= 4 && !p.sim2d &&
        p.nz >= 2 && p.bc_x == MW_BC_PERIODIC && p.bc_y == MW_BC_PERIODIC)) return false;
  const long long nx_min = d->g.nx_glob / std::max(1, p.nproc_x), ny_min = d->g.ny_glob / std::max(1, p.nproc_y);
  if (ny_min < MW_ZR_HALO || nx_min < 2 * MW_ZR_HALO) return false;   // (a tracer must not cross a whole block in one sub-cycle)
  if (!d->xchg) return !d->overlap && !d->pipe;
  return d->pipe != 0;
}
// ... built at the start of a sub-cycle from its input on stream `st`: the coupler's arrays while the conversion is still pending (it
// happens inside the first y launch), slab S0 otherwise.  Blocks of a decomposed domain: + the neighbours' maps (see k_zero_merge).
static int zero_rows_build(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st, bool first_cycle) {
  d->zr_on = zero_rows_ok(d);
  if (!d->zr_on) return 0;
  DyP &p = d->p;
  const int ld = p.ny + 2 * MW_ZR_HALO;
  const long long msz = (long long)p.nz * ld;
  const bool ex_x = d->xchg && p.nproc_x > 1, ex_y = d->xchg && p.nproc_y > 1;
  const long long nrow = (long long)p.nz * p.ny, nedge = (long long)p.nz * MW_ZR_HALO;
  const long long dWE = (nrow + 1) / 2, dSN = (nedge + 1) / 2;   // message lengths in doubles (the transport's unit)
  if (!d->zr || d->zr_msz != msz) {
    if (d->zr) { MW_HIP(hipDeviceSynchronize()); (void)hipFree(d->zr); d->zr = nullptr; }
    if (d->zrx) { (void)hipFree(d->zrx); d->zrx = nullptr; }
    if (hipMalloc(&d->zr, (2 * MW_ZR_MAPS + 3) * (size_t)msz * sizeof(unsigned) * (size_t)p.nens) != hipSuccess) {   // per member: two sets + MC + the two q^n slabs' maps
      (void)hipGetLastError(); d->zr = nullptr; d->zr_on = false;
      if (d->xchg) MW_FAIL("zero-row maps: out of device memory");   // (a decomposed block: the other ranks are about to exchange maps -- an error, not a fall-back)
      return 0; }
    d->zr_msz = msz; d->zr_prev_ok = false; d->kz_buf[0] = d->kz_buf[1] = nullptr;
  }
  if (d->member_major) {                                        // one map set per member, from the member's slab (the caller runs this behind the first y launch)
    d->zr_cur ^= 1;
    d->zr_prev_use = d->zr_prev_ok && d->o.zero_stores;
    const long long mstride = (2 * MW_ZR_MAPS + 3) * msz;
    const int K = marching_config(d, view(d, 0).p);
    const unsigned vmask = (K == 1) ? 0x6u : 0xFu;
    ProfScope ps(d, 4, st);
    for (int e = 0; e < n_views(d); e++) {
      const View v = view(d, e);
      DyP q = v.p; q.zq_ld = ld;
      unsigned *zr = d->zr + e * mstride + (long long)d->zr_cur * MW_ZR_MAPS * msz;
      MW_KLAUNCH(k_zero_rows<true>, dim3((unsigned)((nrow + 3) / 4)), dim3(256), 0, st, q, c, v.S(S0), zr, vmask, ld, MW_ZR_HALO, 1, nullptr);
      MW_KLAUNCH(k_zero_dilate, dim3((unsigned)((p.ny + 63) / 64), (unsigned)((p.nz + 15) / 16)), dim3(256), 0, st, q, zr, msz, 0);
    }
    MW_LAUNCH_CHECK();
    return 0;
  }
  d->zr_cur ^= 1;                                               // build into the other set; the one of the sub-cycle before stays readable
  d->zr_prev_use = d->zr_prev_ok && d->o.zero_stores;
  unsigned *const zr = d->zr + (long long)d->zr_cur * MW_ZR_MAPS * msz;
  if ((ex_x || ex_y) && !d->zrx) {
    if (hipMalloc(&d->zrx, (size_t)(3 * dWE + 4 * dSN) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); MW_FAIL("zero-row maps: out of device memory"); }
    // (a failure here is an error, not a fall-back: the other ranks are about to exchange maps)
  }
  p.zq_ld = ld;
  const int K = marching_config(d, p);
  const unsigned vmask = (K == 1) ? 0x6u : 0xFu;                // = tracer_may_vanish<K>
  ProfScope ps(d, 4, st);
  const dim3 g((unsigned)((nrow + 3) / 4));
  const bool local = !ex_x && !ex_y;
  unsigned *own = local ? zr : (unsigned *)d->zrx;
  const int ldo = local ? ld : p.ny, offo = local ? MW_ZR_HALO : 0;
  if (from_coupler) MW_KLAUNCH(k_zero_rows<false>, g, dim3(256), 0, st, p, c, S0, own, vmask, ldo, offo, local ? 1 : 0, nullptr);
  else              MW_KLAUNCH(k_zero_rows<true>, g, dim3(256), 0, st, p, c, S0, own, vmask, ldo, offo, local ? 1 : 0, nullptr);
  MW_LAUNCH_CHECK();
  if (!local) {
    double *rW = d->zrx + dWE, *rE = d->zrx + 2 * dWE, *sS = d->zrx + 3 * dWE, *sN = sS + dSN, *rS = sN + dSN, *rN = rS + dSN;
    if (ex_x && d->xchg(d->xchg_ctx, d->zrx, d->zrx, nullptr, nullptr, rW, rE, nullptr, nullptr, dWE, 0, st)) MW_FAIL("zero-row maps: exchange callback failed");
    MW_KLAUNCH(k_zero_merge, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, p, own, ex_x ? (const unsigned *)rW : nullptr, (const unsigned *)rE, zr,
               ex_y ? (unsigned *)sS : nullptr, (unsigned *)sN);
    MW_LAUNCH_CHECK();
    if (ex_y) {
      if (d->xchg(d->xchg_ctx, nullptr, nullptr, sS, sN, nullptr, nullptr, rS, rN, 0, dSN, st)) MW_FAIL("zero-row maps: exchange callback failed");
      MW_KLAUNCH(k_zero_halo, dim3((unsigned)((nedge + 255) / 256)), dim3(256), 0, st, p, zr, (const unsigned *)rS, (const unsigned *)rN);
      MW_LAUNCH_CHECK();
    }
  }
  // the first sub-cycle's M0 doubles as "which rows of the coupler's tracer arrays are zero" until the last sub-cycle's D13 (map MC)
  if (first_cycle) MW_HIP(hipMemcpyAsync(d->zr + 2 * MW_ZR_MAPS * msz, zr, (size_t)msz * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  MW_KLAUNCH(k_zero_dilate, dim3((unsigned)((p.ny + 63) / 64), (unsigned)((p.nz + 15) / 16)), dim3(256), 0, st, p, zr, msz, 0);
  MW_LAUNCH_CHECK();
  return 0;
}
// The same in two halves for the first stage of the pipelined schedule (round 5, profiles/r05_selfloop_timeline_maps.txt): LOCAL maps on the
// compute stream in front of the stage's y launches -- the y kernel reads no x halo, its inner rows only the block's own rows; the rows
// beyond a decomposed y edge count as "may be non-zero", and FNs as "store" -- ...
static int zero_rows_local(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st) {
  d->zr_on = zero_rows_ok(d);
  if (!d->zr_on) return 0;
  DyP &p = d->p;
  const int ld = p.ny + 2 * MW_ZR_HALO;
  const long long msz = (long long)p.nz * ld;
  const bool ex_x = d->xchg && p.nproc_x > 1, ex_y = d->xchg && p.nproc_y > 1;
  const long long nrow = (long long)p.nz * p.ny, nedge = (long long)p.nz * MW_ZR_HALO;
  const long long dWE = (nrow + 1) / 2, dSN = (nedge + 1) / 2;
  if (!d->zr || d->zr_msz != msz) {
    if (d->zr) { MW_HIP(hipDeviceSynchronize()); (void)hipFree(d->zr); d->zr = nullptr; }
    if (d->zrx) { (void)hipFree(d->zrx); d->zrx = nullptr; }
    if (hipMalloc(&d->zr, (2 * MW_ZR_MAPS + 3) * (size_t)msz * sizeof(unsigned) * (size_t)p.nens) != hipSuccess) {
      (void)hipGetLastError(); d->zr = nullptr; d->zr_on = false;
      if (d->xchg) MW_FAIL("zero-row maps: out of device memory");   // (as in zero_rows_build: the neighbours still post their map exchanges)
      return 0; }
    d->zr_msz = msz; d->zr_prev_ok = false; d->kz_buf[0] = d->kz_buf[1] = nullptr;
  }
  if (!d->zrx && hipMalloc(&d->zrx, (size_t)(3 * dWE + 4 * dSN) * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); MW_FAIL("zero-row maps: out of device memory"); }
  d->zr_cur ^= 1;
  d->zr_prev_use = d->zr_prev_ok && d->o.zero_stores;
  unsigned *const zr = d->zr + (long long)d->zr_cur * MW_ZR_MAPS * msz;
  p.zq_ld = ld;
  const unsigned vmask = (marching_config(d, p) == 1) ? 0x6u : 0xFu;
  ProfScope ps(d, 4, st);
  const dim3 g((unsigned)((nrow + 3) / 4));
  const int wrap = ex_y ? 2 : 1;
  if (from_coupler) MW_KLAUNCH(k_zero_rows<false>, g, dim3(256), 0, st, p, c, S0, zr, vmask, ld, MW_ZR_HALO, wrap, (unsigned *)d->zrx);
  else              MW_KLAUNCH(k_zero_rows<true>, g, dim3(256), 0, st, p, c, S0, zr, vmask, ld, MW_ZR_HALO, wrap, (unsigned *)d->zrx);
  MW_KLAUNCH(k_zero_dilate, dim3((unsigned)((p.ny + 63) / 64), (unsigned)((p.nz + 15) / 16)), dim3(256), 0, st, p, zr, msz, (ex_x || ex_y) ? 1 : 0);
  MW_LAUNCH_CHECK();
  return 0;
}
// ... and the neighbours' maps merged in on the exchange stream, for the tracer kernel and everything after it.  (The y launches of the first
// stage may read either version of a word while this runs: both describe their rows correctly, the merged one only knows more.)
static int zero_rows_merge(mw_dycore_s *d, hipStream_t st, bool first_cycle) {
  if (!d->zr_on) return 0;
  DyP &p = d->p;
  const long long msz = d->zr_msz;
  const bool ex_x = d->xchg && p.nproc_x > 1, ex_y = d->xchg && p.nproc_y > 1;
  const long long nrow = (long long)p.nz * p.ny, nedge = (long long)p.nz * MW_ZR_HALO;
  const long long dWE = (nrow + 1) / 2, dSN = (nedge + 1) / 2;
  unsigned *const zr = d->zr + (long long)d->zr_cur * MW_ZR_MAPS * msz;
  ProfScope ps(d, 4, st);
  if (ex_x || ex_y) {
    double *rW = d->zrx + dWE, *rE = d->zrx + 2 * dWE, *sS = d->zrx + 3 * dWE, *sN = sS + dSN, *rS = sN + dSN, *rN = rS + dSN;
    if (ex_x && d->xchg(d->xchg_ctx, d->zrx, d->zrx, nullptr, nullptr, rW, rE, nullptr, nullptr, dWE, 0, st)) MW_FAIL("zero-row maps: exchange callback failed");
    MW_KLAUNCH(k_zero_merge, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, st, p, (const unsigned *)d->zrx, ex_x ? (const unsigned *)rW : nullptr, (const unsigned *)rE, zr,
               ex_y ? (unsigned *)sS : nullptr, (unsigned *)sN);
    MW_LAUNCH_CHECK();
    if (ex_y) {
      if (d->xchg(d->xchg_ctx, nullptr, nullptr, sS, sN, nullptr, nullptr, rS, rN, 0, dSN, st)) MW_FAIL("zero-row maps: exchange callback failed");
      MW_KLAUNCH(k_zero_halo, dim3((unsigned)((nedge + 255) / 256)), dim3(256), 0, st, p, zr, (const unsigned *)rS, (const unsigned *)rN);
      MW_LAUNCH_CHECK();
    }
  }
  if (first_cycle) MW_HIP(hipMemcpyAsync(d->zr + 2 * MW_ZR_MAPS * msz, zr, (size_t)msz * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  if (ex_x || ex_y) { MW_KLAUNCH(k_zero_dilate, dim3((unsigned)((p.ny + 63) / 64), (unsigned)((p.nz + 15) / 16)), dim3(256), 0, st, p, zr, msz, 0); MW_LAUNCH_CHECK(); }
  return 0;
}
// ... and handed to the kernels of RK stage `stage` (1..3) through the parameter block
static void zero_rows_stage(mw_dycore_s *d, int stage) {
  DyP &p = d->p;
  p.zqk = nullptr;
  if (!d->zr_on || stage < 1) { p.zq = p.zqp = p.zqc = nullptr; p.zq_ld = 0; return; }
  const long long set = (long long)MW_ZR_MAPS * d->zr_msz;
  p.zq = d->zr + d->zr_cur * set + (long long)stage * d->zr_msz;
  p.zqp = (d->zr_prev_use && stage <= 2) ? d->zr + (d->zr_cur ^ 1) * set + (long long)stage * d->zr_msz : nullptr;   // (S1, S2: the slab of stage s is always the same one)
  p.zqc = (d->o.zero_stores && !d->member_major) ? d->zr + 2 * set : nullptr;      // (member-major: the coupler's arrays are written by launches that read no maps)
  // (member-major: these are member 0's; view() moves them on to its member)
  p.zq_ld = p.ny + 2 * MW_ZR_HALO;
}
// The converting y launch (first stage of a time step, conversion inside k_y_all) writes slab S: before it, hand over what is known about S's
// rows (written by the last conversion into S, untouched since); after it (`done`), S's rows are zero exactly where the coupler's are: map MC.
static void zero_rows_conv(mw_dycore_s *d, const double *S, bool done, hipStream_t st) {
  const long long msz = d->zr_msz;
  int sl = (d->kz_buf[0] == S) ? 0 : (d->kz_buf[1] == S) ? 1 : -1;
  if (!done) { d->p.zqk = (sl >= 0 && d->zr_on && d->o.zero_stores) ? d->zr + (2 * MW_ZR_MAPS + 1 + sl) * msz : nullptr; return; }
  d->p.zqk = nullptr;
  if (!d->zr_on) { if (sl >= 0) d->kz_buf[sl] = nullptr; return; }
  if (sl < 0) {                                                 // a free slot, else the one of a slab that is not one of the two q^n slabs any more
    const double *other = (S == d->S0) ? d->S3 : d->S0;
    sl = (d->kz_buf[0] == nullptr) ? 0 : (d->kz_buf[1] == nullptr) ? 1 : (d->kz_buf[0] != other) ? 0 : 1;
  }
  (void)hipMemcpyAsync(d->zr + (2 * MW_ZR_MAPS + 1 + sl) * msz, d->zr + 2 * MW_ZR_MAPS * msz, (size_t)msz * sizeof(unsigned), hipMemcpyDeviceToDevice, st);
  d->kz_buf[sl] = S;
}
void zero_rows_forget(mw_dycore_s *d, const double *S) {   // slab S is about to be written by something that keeps no map
  for (int i = 0; i < 2; i++) if (!S || d->kz_buf[i] == S) d->kz_buf[i] = nullptr;
}
// One SSPRK3 sub-cycle.  Slabs: Q[0] = q^n, Q[1..3] scratch; on return the new q^n is in Q[3] (caller rotates).
int rk_cycle_march(mw_dycore_s *d, double **Q, double dt_dyn, bool last, const CouplerPtrs &c) {
  const double dt2 = (1.0 / 4.0) * dt_dyn, dt3 = (2.0 / 3.0) * dt_dyn;
  d->zr_on = false;
  if (!d->pipe && !d->member_major && zero_rows_build(d, Q[0], c, d->conv_pending, d->stream, d->first_cycle)) return 1;   // (pipelined schedule: inside its first stage, on the exchange stream; member-major: behind the first y launch, from the slab)
  if (d->pipe) {                                              // blocks of a decomposed domain, pipelined schedule
    d->pipe_ready = false; d->pipe_edge_done = false;
    if (rk_stage_pipe<1, 0>(d, Q[0], Q[0], Q[1], dt_dyn, dt_dyn, c)) return 1;
    if (rk_stage_pipe<2, 0>(d, Q[1], Q[0], Q[2], dt2, dt_dyn, c)) return 1;
    const bool pass13p = d->member_major && !d->mm_direct;
    if (last && !pass13p) { if (rk_stage_pipe<3, 1>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }
    else                  { if (rk_stage_pipe<3, 0>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }
    if (last && pass13p) {
      ProfScope ps(d, 4, d->stream);
      const View v = view(d, 0);
      const MemberStrides ms = {v.p.sJ, v.p.sK, v.p.sV, v.slab};
      MW_KLAUNCH(k_member_to_coupler, plane_grid((long long)d->p.ny * d->p.nx * d->p.nens, d->p.nz), dim3(256), 0, d->stream, d->p, Q[3], c, ms);
      MW_LAUNCH_CHECK();
    }
    d->flux_src = Q[2]; d->flux_dt = dt3;
    d->zr_prev_ok = d->zr_on; d->zr_on = false; zero_rows_stage(d, 0);
    return 0;
  }
  if (rk_stage_march<1, 0>(d, Q[0], Q[0], Q[1], dt_dyn, dt_dyn, c)) return 1;                        // stage 1 (:119-132)
  if (rk_stage_march<2, 0>(d, Q[1], Q[0], Q[2], dt2, dt_dyn, c)) return 1;                           // stage 2 (:136-153)
  const bool pass13 = d->member_major && !d->mm_direct;        // D13 as a pass over the result slab
  if (last && !pass13) { if (rk_stage_march<3, 1>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }   // stage 3 (:157-174) + :178
  else                 { if (rk_stage_march<3, 0>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }
  if (last && pass13) {                              // D13 (:178) as one coalesced pass over the result slab
    hipStream_t ts = d->overlap ? d->tstream : d->stream;     // the tracer pipeline finishes the stage
    ProfScope ps(d, 4, ts);
    const View v = view(d, 0);
    const MemberStrides ms = {v.p.sJ, v.p.sK, v.p.sV, v.slab};
    MW_KLAUNCH(k_member_to_coupler, plane_grid((long long)d->p.ny * d->p.nx * d->p.nens, d->p.nz), dim3(256), 0, ts, d->p, Q[3], c, ms);
    MW_LAUNCH_CHECK();
    if (d->overlap) MW_HIP(hipEventRecord(d->ev_tr[(d->gstage - 1) & 7], ts));     // the step's join waits for this event
  }
  d->flux_src = Q[2]; d->flux_dt = dt3;
  d->zr_prev_ok = d->zr_on; d->zr_on = false; zero_rows_stage(d, 0);
  return 0;
}

// D1 + D2 as a pass of its own in front of the first sub-cycle (mw_dycore_time_step): cells with j < ylo, j >= yhi or within HX cells of the
// block's west / east edge (ylo >= ny: all cells); strips: launch over those strip cells only (see k_coupler_to_state_fast)
int launch_coupler_to_slab(mw_dycore_s *d, const CouplerPtrs &c, int ylo, int yhi, bool strips) {
  const DyP &p = d->p;
  const dim3 cgrid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz);
  if (d->member_major) {      // one coalesced pass in the coupler's order (see k_coupler_to_member)
    const View v = view(d, 0);
    const MemberStrides ms = {v.p.sJ, v.p.sK, v.p.sV, v.slab};
    MW_KLAUNCH(k_coupler_to_member, cgrid, dim3(256), 0, d->stream, p, c, d->S0, ms, ylo, yhi);
  } else {
    const long long nstrip = (long long)(ylo + p.ny - yhi) * p.nx * p.nens + (long long)(yhi - ylo) * 2 * p.HX * p.nens;
    const bool s = strips && p.nx > 2 * p.HX && nstrip > 0;
    MW_KLAUNCH(k_coupler_to_state_fast, s ? plane_grid(nstrip, p.nz) : cgrid, dim3(256), 0, d->stream, p, c, d->S0, ylo, yhi, s ? 1 : 0);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" {
// Test aid: the zero-row maps of the last sub-cycle, on the host (include/mw_cdna4.h).
long long mw_debug_zero_maps(mw_dycore_t d, unsigned int *out_host, long long cap_words, int *dims2) {
  if (!d) return 0;
  if (!d->zr || !d->zr_prev_ok || d->member_major) return 0;    // (zr_prev_ok: the last sub-cycle ran with maps; member-major handles keep one set per member)
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  const long long n = (long long)MW_ZR_MAPS * d->zr_msz;
  if (dims2) { dims2[0] = d->p.nz; dims2[1] = d->p.ny + 2 * MW_ZR_HALO; }
  if (out_host && cap_words > 0)
    (void)hipMemcpy(out_host, d->zr + (long long)d->zr_cur * n, (size_t)std::min(n, cap_words) * sizeof(unsigned), hipMemcpyDeviceToHost);
  return n;
}
// Test aid: the four violation counters of option zero_verify (k_zero_verify, mw_march.h) since the handle was created; -1: the option
// never ran.  out4: [0] input row non-zero under a clear Qs word, [1] ... under a clear QYs word, [2] a destination row the tracer kernel
// was told holds zeros does not, [3] likewise a row of the slab the converting y launch fills.
long long mw_debug_zero_violations(mw_dycore_t d, unsigned long long *out4) {
  if (!d || !d->zviol) return -1;
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  unsigned long long h[4] = {0, 0, 0, 0};
  if (hipMemcpy(h, d->zviol, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (out4) for (int i = 0; i < 4; i++) out4[i] = h[i];
  return (long long)(h[0] + h[1] + h[2] + h[3]);
}
// Test aid: the fused tracer stage's per-cell flag bytes as its last launch left them (bits 2v / 2v + 1: tracer v's south / north face was
// scaled by this cell), index (k * ny + j) * nx * nens + x.  Returns the number of cells; copies at most `cap` bytes to out_host.
long long mw_debug_tracer_flags(mw_dycore_t d, unsigned char *out_host, long long cap) {
  if (!d || !d->flags) return -1;
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  const long long n = (long long)d->p.nC;
  if (out_host && cap > 0 && hipMemcpy(out_host, d->flags, (size_t)std::min(n, cap), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}
// Test aid: how many RK stages of the last time step redid their water vapour in the tracer stage's three-tracer form because a cell failed the
// limiter test in k_xz_state's vapour form (or option debug_vapour_redo set the word); 0 also when no stage ran the vapour form.  -1: null handle.
long long mw_debug_vapour_redo(mw_dycore_t d) {
  if (!d || !d->dirty) return -1;
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  unsigned int n = 0;
  if (hipMemcpy(&n, d->dirty + MW_VREDO_RING + 8, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
} // extern "C"
