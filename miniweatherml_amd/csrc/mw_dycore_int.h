// =====================================================================================================
// mw_dycore_int.h -- what the units of the dycore share on the HOST side (exported nowhere): the handle, its options, the member
// views, the launch registry and the functions that cross unit boundaries.
//
//   mw_dycore.hip          general-path kernels and their launchers, handle, options, C ABI, time_step's decisions
//   mw_march_y.hip         launchers of k_y_state / k_y_all / k_y_tracers                      }
//   mw_march_xz.hip        launchers of k_xz_state                                             }  the kernels' text is in mw_march.h;
//   mw_march_tracers.hip   launchers of k_xz_tracers / k_tracer_update / k_tracers_fused       }  these units hold launch code only
//   mw_march_sched.hip     the three schedules of an RK stage, conversion passes               }
//   mw_zero_rows.hip       the zero-row maps: their kernels (text there too) and host side (interface: mw_zero_rows.h)
//   mw_dycore_init.hip     the four initial states and the temperature perturbations
//   mw_dycore_aids.hip     calibration launchers (mw_calib.h) and test aids
//
// One definition per kernel: without relocatable device code every unit is a code object of its own, and a kernel that two units
// instantiate (or a non-template kernel in a header that two units include) is emitted twice.  So every kernel family is launched from
// exactly one unit; the non-template kernels of mw_march.h are compiled by mw_march_sched.hip alone (MW_MARCH_SCHED_KERNELS), and the zero-row
// kernels are defined in mw_zero_rows.hip, not in a header.
// =====================================================================================================
#pragma once
#include "mw_common.h"
#include "mw_zero_rows.h"
#include <string>
#include <vector>
#include <algorithm>

#pragma GCC visibility push(hidden)      // nothing below is part of the library's ABI

// Every kernel launch of the dycore goes through MW_KLAUNCH: besides launching it notes the kernel's host function in a process-wide
// registry (defined in mw_dycore.hip), so that a test session can ask which INSTANTIATIONS of the dispatcher's kernels its oracle comparisons
// really exercised (mw_debug_launched_kernels; tests/conftest.py checks them against the list of everything compiled into the library).
// Host-side only: one uncontended mutex and a set insert per launch, nothing in the kernels.
namespace mw { void note_launch(const void *fn); }
#define MW_KLAUNCH(kern, ...) do { mw::note_launch((const void *)&kern); hipLaunchKernelGGL(kern, __VA_ARGS__); } while (0)

using namespace mw;

// Run-time options of a handle (mw_dycore_set_option / mw_dycore_get_option; rounds 1-4 read MW_* environment variables per launch
// instead -- process-global, untyped and racy under threads).  Typed integers, read where the schedule of a time step is decided.
struct DyOpts {
  int overlap = -1;            // two-stream schedule (state | tracer pipelines): -1 = automatic (with a transport installed), 0 / 1 forced
  int pipe = 1;                // with a transport: the pipelined one-stream schedule (rk_stage_pipe) where k_y_all applies
  int pipe_edge_inline = 0;    // ... its two edge strips of the y launch on the compute stream instead of the exchange stream
  int pipe_convert = 1;        // ... D1 of the inner rows inside the first k_y_all<true>
  int pipe_split_edges = 1;    // ... the next stage's edge strips split into a state part (behind the state strips) and a tracer part
  int spec = 1;                // folded configurations of the marching kernels (Cf<1>, Cf<2>)
  int wrap = 1;                // index wrap instead of halo cells in a periodic direction owned by one rank
  int y_all = 1, y_all_conv = 1;      // y faces of all variables in one launch; ... also the converting first stage
  int member_major = 1, mm_direct = 1, mm_conv = 1;   // nens > 1: member-major arrays; D13 / D1 inside the members-in-one-workgroup launches
  int fused_convert = 1, fused_convert_mm = 1;        // D1 inside the first y launch (one rank, periodic x and y)
  int chunk_y = 0, chunk_yt = 0, chunk_z = 0, chunk_f = 0;   // cells per chunk of the marching kernels (0 = the chunk model)
  int chunk_model = 1;
  int tf_rows4 = 1;            // tracer stage: workgroup = 4 rows of one x tile (0: 4 tiles of one row)
  int zero_skip = 1;           // wave-uniform short-cut for tracers that are exactly zero over a wavefront's stencil (bit-neutral; 0: A/B)
  int zero_rows = 1;           // ... and the zero-row maps on top of it: rows of a tracer that are known to be zero are not loaded (mw_zero_rows.h)
  int pipe_maps_early = 1;     // pipelined schedule, first stage: local zero-row maps in front of its y launches, two strip exchanges (0: one exchange, maps beside the y launch; A/B)
  int zero_stores = 1;         // ... and zeros are not stored over rows that hold zeros already (the coupler's arrays, slabs S1 / S2; 0: A/B)
  int zero_verify = 0;         // test aid: check the maps' claims against the data in front of every launch that relies on them (k_zero_verify; mw_debug_zero_violations)
  int rccl_lanes = 0, rccl_two_comms = -1;            // built-in RCCL transport: side streams (1 | 2), a communicator per lane (0 | 1); 0 / -1 = the
                                                      // process default (MW_RCCL_LANES); read when mw_dycore_use_rccl* installs the transport
  int rccl_prio = 1;           // ... its side streams at the highest stream priority (0: default priority; A/B)
  int rccl_inline = 1;         // ... the send / receive group on the caller's stream instead of a side stream of the transport's own
  int xchg_fuzz = 0;           // test aid: seeded random delays (spin kernels) around the built-in transport's sends / receives
  int debug_no_patch = 0;      // test aid: the y-face correction pass of the fused tracer stage is not launched (the negative control of the FCT tests)
  int vapour_state = 1;        // folded supercell configuration, nens == 1, WENO-5, one-stream schedule behind k_y_all: the water vapour is advanced by k_xz_state (0: by the tracer stage; A/B)
  int debug_vapour_redo = 0;   // test aid: every stage's redo word is set by hand -- the tracer stage recomputes the vapour in its three-tracer form
  int lean_stores = 1;         // with vapour_state and maps: k_xz_state does not store the faces (and, last stage, the slab slots) that only FULL iterations of the tracer stage read where the row map says lean, a replay launch stores them when the vapour is redone; all-lean tracer waves leave their zero flag bytes out while the buffer is known to be zero (0: everything is stored; A/B)
};

struct mw_dycore_s {
  mw_grid_t g;
  DyOpts o;
  unsigned char pos[MW_MAX_TRACERS], adds[MW_MAX_TRACERS];
  DyP p;
  bool strides_ok = true;                    // fill_params: every stride of DyP fits its Stride32
  int ord = 5;                               // WENO order (3, 7, 9: the reference's -DMW_ORD builds; they run on the general kernels)
  int hxw = HXc, hzw = HZc;                  // halo widths of the slabs: hs + 1 in x / y, hs in z (3 / 2 up to order 5)
  double etime = 0;
  int strict = 0;
  int last_march = 0;                        // the last time_step ran on the marching kernels (mw_dycore_schedule)
  std::string path;                          // what the dispatcher chose for the last time_step, spelled out (mw_dycore_path)
  // ---- slabs, face arrays, background
  double *S0 = nullptr, *S1 = nullptr, *S2 = nullptr, *S3 = nullptr;   // q^n and three stage slabs (rotated, never aliased)
  int member_major = 0;                      // production path with nens > 1: the handle's arrays hold one member after the other (View)
  int mm_direct = 0;                         // member-major: D13 written from the last stage's kernels (MemberOff: 2 or 4 members per workgroup), no k_member_to_coupler pass
  double *M[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};          // upwind mass flux of every x/y/z face,
  unsigned char *UP[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // upwind selector; double-buffered by stage parity
  double *tendY = nullptr;                   // (5,nz,ny,nx,nens) y part of the state tendencies
  double *FX = nullptr, *FY = nullptr, *FZ = nullptr;
  const double *flux_src = nullptr; double flux_dt = 0; // stage input + dt of the last stage (state fluxes on demand)
  int chunk_y = 0, chunk_yt = 0, chunk_z = 0, chunk_f = 0;
  double *hy_dev = nullptr;                  // hyc | hytc | hye | hyte | p0c | ihytc | p0e | ihyte | packed rows (see DyP::hypk)
  std::vector<double> hy_host;               // same packing (the last four are derived in upload_background)
  double *imm = nullptr;
  // ---- streams, events and where a time step stands
  hipStream_t stream;
  hipStream_t tstream = nullptr;             // tracer pipeline (runs one stage behind / beside the state pipeline); the pipelined schedule's exchange stream
  hipEvent_t ev_state[8] = {nullptr}, ev_tr[8] = {nullptr}, ev_misc = nullptr;
  long long gstage = 0;                      // global stage counter (event ring index, buffer parity)
  int overlap = 1;                           // two-stream schedule (state | tracer pipelines)
  bool conv_pending = false;                 // time_step: the coupler -> slab conversion is still to be done by stage 1's y launch
  bool first_cycle = false;                  // the running sub-cycle is the time step's first
  // ---- pipelined schedule
  int pipe = 0;                              // blocks of a decomposed domain: pipelined one-stream schedule (rk_stage_pipe)
  bool pipe_ready = false;                   // ... the next stage's input strips are already on their way (event ev_pipe[2])
  bool pipe_edge_done = false;               // ... and its two edge strips of the y launch were issued behind them on the exchange stream
  int pre_lo = 0, pre_hi = 0;                // ... rows outside [pre_lo, pre_hi) (and the W / E strip columns) were converted up front
  // [0], [1]: compute -> exchange stream; [2]: state strips + state edge rows ready; [3]: tracer strips + tracer edge faces ready; [4]: zero-row
  // maps ready; [5]: the block's local zero-row maps ready (exchange -> compute stream); [6]: time_step entered (the coupler's arrays are ready)
  hipEvent_t ev_pipe[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool entry_marked = false;                 // ev_pipe[6] was recorded at this time step's entry
  // ---- fused tracer stage, vapour redo, zero-row maps
  int fused = 0;                             // 1: fused tracer stage (k_tracers_fused + k_tracer_patch)
  unsigned long long fused_launches = 0;
  unsigned char *flags = nullptr;            // fused tracer stage: per-cell "a y face of this cell was FCT-scaled" bits
  unsigned int *dirty = nullptr;             // [0], [1]: "a y face was scaled in this / the next fused tracer launch"; [2]: scratch; [MW_VREDO_RING ..+7]: "a vapour cell of stage gs & 7 failed the limiter test"; [MW_VREDO_RING + 8]: stages of this time step that took the redo
  long long vap_last_gs = -2;                // the last stage (gstage) that advanced the water vapour in k_xz_state (option vapour_state)
  bool vap_used = false;                     // some stage since the last reset of the redo counter did
  ZeroRows zr;                               // zero-row maps (mw_zero_rows.h); touched by mw_zero_rows.hip and, reading `on`, the schedules
  // ---- parked column increments
  double *pinc = nullptr; bool pinc_on = false; double *pinc_fields[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // parked column increments (mw_nudge_to_column_deferred) and the five arrays they belong to
  unsigned long long pinc_lazy = 0, pinc_eager = 0;             // how often parked increments rode on the conversion / were applied by a pass
  // ---- halo exchange
  mw_exchange_fn xchg = nullptr; void *xchg_ctx = nullptr;
  void (*xchg_free)(void *) = nullptr;       // set when the handle owns xchg_ctx (the built-in RCCL transport, mw_rccl.cpp)
  double *bufs[2][8] = {{nullptr}, {nullptr}};   // [group: 0 state (or all), 1 tracers][sW sE sS sN rW rE rS rN]
  long long nWE1 = 0, nSN1 = 0;                  // per variable
  // ---- profiling
  int prof = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[12];      // kernel classes 0..7; 8 = one whole RK stage (all its launches); 9 = one whole time_step; 10 / 11 = the compute stream's waits for the state / tracer strips (pipelined schedule)
  size_t ev_used[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an L2).  Padding the blocks-per-plane count to a
// multiple of 8 puts the block that owns tile (j,i) of level k+1 on the SAME XCD as the block of level k, so the z-neighbour
// face/cell reads of the plane kernels hit that XCD's L2 instead of going out to the Infinity Cache / HBM.
static inline dim3 plane_grid(long long per_plane, int nk, int nzdim = 1) {
  unsigned nb = (unsigned)((per_plane + 255) / 256);
  nb = (nb + 7u) & ~7u;
  return dim3(nb, (unsigned)nk, (unsigned)nzdim);
}

struct ProfScope {
  mw_dycore_s *d; int which; size_t idx; bool on; hipStream_t st;
  ProfScope(mw_dycore_s *d_, int w, hipStream_t st_ = nullptr) : d(d_), which(w), idx(0), on((d_->prof == 1 && w != 9) || (d_->prof == 2 && (w == 0 || w == 8)) || (d_->prof == 3 && w == 9)), st(st_ ? st_ : d_->stream) {
    if (!on) return;
    if (d->ev_used[which] == d->ev[which].size()) {
      hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b); d->ev[which].push_back({a, b});
    }
    idx = d->ev_used[which]++;
    (void)hipEventRecord(d->ev[which][idx].first, st);
  }
  ~ProfScope() { if (on) (void)hipEventRecord(d->ev[which][idx].second, st); }
};

// ---------------------------------------------------------------------------------------------------------------------
// Member-major mode (production path, nens > 1).  With the coupler's member-fastest layout the x stencil of a wave cannot use
// the DPP lane shifts (x neighbours are nens lanes apart) and the marching kernels fall back to neighbour loads + ds_bpermute:
// k_xz_state is 36 % slower per cell at nens = 4.  The handle's INTERNAL arrays (slabs, tendY, M/UP, FY, side arrays, flags) are
// ours to lay out, so with nens > 1 they hold one member after the other and every production kernel is launched once per member
// in its nens = 1 form (View: the member's parameter block and base pointers); only the coupler-side accesses -- conversion in,
// D13 out, immersed proportion -- are strided (DyP::cst / ce, cpl() in mw_common.h).  The general kernels keep the fused layout in
// the same allocations (a handle runs one path or the other within a time_step; get_fluxes transposes the retained stage input).
// ---------------------------------------------------------------------------------------------------------------------
struct View {
  DyP p;
  long long slab, tend, m[3], f[3], cells;          // member e's offsets = e * these (doubles; UP / flags: bytes = the same counts)
  int e;
  template <class T> T *S(T *base) const { return base ? base + e * slab : base; }
};
int n_views(const mw_dycore_s *d);
View view(const mw_dycore_s *d, int e);
MemberOff member_off(const mw_dycore_s *d);

#define MW_VREDO_RING 4                                        // first word of the vapour redo ring in mw_dycore_s::dirty (8 words + the counter)
#define MW_DIRTY_WORDS 16
#define MW_Y_EDGE 4                                            // rows of an edge strip of the pipelined schedule (>= 4: the converting inner launch requests coupler rows up to row_end + 3 < ny)

// ---- mw_dycore.hip
void fill_params(mw_dycore_s *d);
int upload_background(mw_dycore_s *d);
int make_coupler_ptrs(mw_dycore_s *d, const double *rho_d, const double *u, const double *v, const double *w, const double *temp, double *const *tracers, CouplerPtrs &c);
int halo_fill(mw_dycore_s *d, double *Sbase, int v0 = 0, int nv = -1, hipStream_t st = nullptr, int grp = 0, bool skip_z = false);
int balanced_chunk(const mw_dycore_s *d, int nz, long long base_waves, int forced, long long target, int bpc, double o, bool model);
int device_cus();
int marching_config(const mw_dycore_s *d, const DyP &p);
bool y_all_ok(const mw_dycore_s *d);
// ---- mw_march_y.hip
int launch_y_state(mw_dycore_s *d, const double *S, int par, const CouplerPtrs *conv = nullptr, bool edges = false, hipStream_t st = nullptr);
int launch_y_all(mw_dycore_s *d, const double *S, const CouplerPtrs *conv, int part = 0, hipStream_t st = nullptr);
int launch_y_tracers(mw_dycore_s *d, const double *S, int par, hipStream_t st, bool edges = false);
// ---- mw_march_xz.hip, mw_march_tracers.hip: instantiated there for the four (STAGE, MODE) of an SSPRK3 cycle -- (1, 0), (2, 0), (3, 0), (3, 1)
int xz_grid(mw_dycore_s *d, const DyP &p, dim3 &grid, int &chunk, int &tiles_x);
template <int STAGE, int MODE>
int launch_xz_state(mw_dycore_s *d, const double *S, const double *Sn, double *Sout, double dt_stage, double dt_dyn, int par, const CouplerPtrs &c, int vap_slot = -1);
// (vap_slot >= 0, both launchers: the stage advances the water vapour in k_xz_state -- rk_stage_march decides -- and this is its word of the redo ring)
int launch_xz_tracers(mw_dycore_s *d, const double *S, int par, double dt, hipStream_t st);
template <int STAGE, int MODE>
int launch_tracer_update(mw_dycore_s *d, const double *Sstar, const double *Sn, double *Sout, double dt_dyn, const CouplerPtrs &c, hipStream_t st);
template <int STAGE, int MODE>
int launch_tracers_fused(mw_dycore_s *d, const double *S, const double *Sn, double *Sout, int par, double dt, double dt_dyn, const CouplerPtrs &c, hipStream_t st, int vap_slot = -1);
// ---- mw_march_sched.hip
int rk_cycle_march(mw_dycore_s *d, double **Q, double dt_dyn, bool last, const CouplerPtrs &c);
int launch_coupler_to_slab(mw_dycore_s *d, const CouplerPtrs &c, int ylo, int yhi, bool strips);

#pragma GCC visibility pop
