// =====================================================================================================
// mw_march_sched.hip -- the schedules of an RK stage on the marching kernels (one stream, two streams, pipelined) and the coupler <-> slab
// conversion passes.  The one unit that compiles the non-template kernels of mw_march.h.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#define MW_MARCH_SCHED_KERNELS
#include "mw_march.h"

// ---------------------------------------------------------------------------------------------------------------------
// One RK stage on the production path, as two pipelines on two HIP streams:
//   state stream  (the handle's stream): halo(state vars) -> k_y_state -> k_xz_state        [fp64-VALU bound]
//   tracer stream (side stream)        : halo(tracers) -> k_y_tracers -> k_tracers_fused -> k_tracer_patch                 [fp64-VALU bound too]
// The state variables of stage s+1 depend only on the state variables of stage s, so the state pipeline runs ahead
// while the tracer pipeline of stage s fills the memory system beside it.  Hand-offs: the tracer kernels need the
// mass fluxes / selectors / new density of their stage (event ev_state); the state pipeline may not run more than
// one stage ahead because the M/UP buffers are double-buffered and the four slabs rotate (event ev_tr of stage s-2).
// ---------------------------------------------------------------------------------------------------------------------
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
    if (d->zr.on) MW_HIP(hipEventRecord(d->ev_pipe[4], xs));
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
      if (d->zr.on) MW_HIP(hipEventRecord(d->ev_pipe[4], xs));
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
  if (STAGE == 1 && d->zr.on) {
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
template <int STAGE, int MODE>   // one RK stage on the handle's schedule
static int rk_stage(mw_dycore_s *d, double *Sin, const double *Sn, double *Sout, double dt_stage, double dt_dyn, const CouplerPtrs &c) {
  return d->pipe ? rk_stage_pipe<STAGE, MODE>(d, Sin, Sn, Sout, dt_stage, dt_dyn, c) : rk_stage_march<STAGE, MODE>(d, Sin, Sn, Sout, dt_stage, dt_dyn, c);
}
// One SSPRK3 sub-cycle.  Slabs: Q[0] = q^n, Q[1..3] scratch; on return the new q^n is in Q[3] (caller rotates).
int rk_cycle_march(mw_dycore_s *d, double **Q, double dt_dyn, bool last, const CouplerPtrs &c) {
  const double dt2 = (1.0 / 4.0) * dt_dyn, dt3 = (2.0 / 3.0) * dt_dyn;
  d->zr.on = false;
  if (d->pipe) { d->pipe_ready = false; d->pipe_edge_done = false; }   // blocks of a decomposed domain, pipelined schedule
  if (!d->pipe && !d->member_major && zero_rows_build(d, Q[0], c, d->conv_pending, d->stream, d->first_cycle)) return 1;   // (pipelined schedule: inside its first stage, on the exchange stream; member-major: behind the first y launch, from the slab)
  if (rk_stage<1, 0>(d, Q[0], Q[0], Q[1], dt_dyn, dt_dyn, c)) return 1;                        // stage 1 (:119-132)
  if (rk_stage<2, 0>(d, Q[1], Q[0], Q[2], dt2, dt_dyn, c)) return 1;                           // stage 2 (:136-153)
  const bool pass13 = d->member_major && !d->mm_direct;        // D13 as a pass over the result slab
  if (last && !pass13) { if (rk_stage<3, 1>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }   // stage 3 (:157-174) + :178
  else                 { if (rk_stage<3, 0>(d, Q[2], Q[0], Q[3], dt3, dt_dyn, c)) return 1; }
  if (last && pass13) {                              // D13 (:178) as one coalesced pass over the result slab
    hipStream_t ts = d->overlap ? d->tstream : d->stream;     // the tracer pipeline finishes the stage (the pipelined schedule has none: overlap == 0)
    ProfScope ps(d, 4, ts);
    const View v = view(d, 0);
    const MemberStrides ms = {v.p.sJ, v.p.sK, v.p.sV, v.slab};
    MW_KLAUNCH(k_member_to_coupler, plane_grid((long long)d->p.ny * d->p.nx * d->p.nens, d->p.nz), dim3(256), 0, ts, d->p, Q[3], c, ms);
    MW_LAUNCH_CHECK();
    if (d->overlap) MW_HIP(hipEventRecord(d->ev_tr[(d->gstage - 1) & 7], ts));     // the step's join waits for this event
  }
  d->flux_src = Q[2]; d->flux_dt = dt3;
  zero_rows_end_cycle(d);
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
// Test aid of option lean_stores: NaN / 0xFF over everything k_xz_state<.., VAP> may leave out -- both parities of MX, MZ, UPX, UPZ and the rho' and
// pressure slots of the slab that takes the last stage's result when the next time step runs one sub-cycle (S3).  All of it is scratch between
// time steps: the faces are rewritten by every stage that reads them, and a time step starts from the coupler's arrays.
int mw_debug_poison_handoff(mw_dycore_t d) {
  if (!d || !d->S3) MW_FAIL("mw_debug_poison_handoff: null handle");
  const DyP &p = d->p;
  const size_t fn[3] = {(size_t)p.fxV, (size_t)p.fyV, (size_t)p.fzV};
  for (int b = 0; b < 2; b++) for (int a = 0; a < 3; a += 2) {
    MW_HIP(hipMemsetAsync(d->M[b][a], 0xFF, fn[a] * sizeof(double), d->stream));
    MW_HIP(hipMemsetAsync(d->UP[b][a], 0xFF, fn[a], d->stream));
  }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    for (int l : {(int)idR, (int)idT}) MW_HIP(hipMemsetAsync(v.S(d->S3) + (long long)l * v.p.sV, 0xFF, (size_t)v.p.sV * sizeof(double), d->stream));
  }
  if (d->tstream) { MW_HIP(hipStreamSynchronize(d->stream)); }   // (the tracer stream of the two-stream schedule reads the faces too)
  return 0;
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
