/* =====================================================================================================
 * mw_cdna4.h -- C ABI of the MI355X-native (gfx950 / CDNA4) miniWeatherML hot path.
 *
 * One shared library, libmw_cdna4.so (miniweatherml_amd/csrc), exports exactly the symbols declared
 * here.  Plain pointers and sizes only; no C++ or torch types.  All field pointers are DEVICE pointers
 * (hipMalloc'd / torch.cuda tensors) unless a parameter is documented as "host".  All arithmetic is IEEE
 * fp64 except the MLP (fp32 inside, fp64 at the boundary).  Array layout everywhere: C row-major, last
 * index fastest, coupler fields (nz,ny,nx,nens)  -- reference: model/core/coupler.h:323-330.
 *
 * Every entry point returns 0 on success, non-zero on failure; mw_last_error() then returns the message
 * (replaces the reference's endrun()/yakl_throw abort, model/main_header.h:66-68).  A missing GPU, a
 * failed kernel launch or an unsupported option is an ERROR -- there is no CPU fallback in this library.
 *
 * Each function cites the reference interface it replaces (paths relative to the reference repo root).
 * ===================================================================================================== */
#ifndef MW_CDNA4_H
#define MW_CDNA4_H

#ifdef __cplusplus
extern "C" {
#endif

#define MW_NUM_STATE 5          /* dynamics_euler_stratified_wenofv.h:31 */
#define MW_MAX_TRACERS 16

/* test cases, dynamics_euler_stratified_wenofv.h:41-44 */
enum { MW_DATA_THERMAL = 0, MW_DATA_SUPERCELL = 1, MW_DATA_CITY = 2, MW_DATA_BUILDING = 3 };
/* boundary conditions, dynamics_euler_stratified_wenofv.h:46-48 */
enum { MW_BC_PERIODIC = 0, MW_BC_OPEN = 1, MW_BC_WALL = 2 };

/* Everything the dycore pulls out of core::Coupler getters and options
 * (coupler.h:219-278 geometry getters; options set/read at dynamics_euler_stratified_wenofv.h:211-226,
 * 1227-1249,1300,1312,1332-1335). */
typedef struct {
  int nz, ny, nx, nens, num_tracers;          /* local sizes: coupler.get_nz/ny/nx/nens/num_tracers            */
  long long nx_glob, ny_glob, i_beg, j_beg;   /* coupler.get_nx_glob/ny_glob/i_beg/j_beg                       */
  double xlen, ylen, zlen;                    /* coupler.get_xlen/ylen/zlen ; dx = xlen/nx_glob etc.           */
  int px, py, nproc_x, nproc_y;               /* coupler.get_px/py/nproc_x/nproc_y                             */
  int neigh[9];                               /* coupler.get_neighbor_rankid_matrix(), [y][x] row-major 3x3    */
  int bc_x, bc_y, bc_z;                       /* options "bc_x","bc_y","bc_z"                                  */
  int use_immersed, enable_gravity;           /* options "use_immersed_boundaries","enable_gravity"            */
  int idWV;                                   /* option "idWV": index of the tracer named water_vapor          */
  double R_d, R_v, cp_d, cp_v, p0, grav, gamma_d, kappa_d, C0, earthrot, latitude;   /* real options           */
} mw_grid_t;

typedef struct mw_dycore_s *mw_dycore_t;      /* opaque: module-private persistent state (hy_dens_*, flags,     */
                                              /* etime, workspace) -- the reference keeps it in the module      */
                                              /* object, dynamics_euler_stratified_wenofv.h:51-66               */

const char *mw_last_error(void);
int  mw_device_count(void);                   /* >0 iff a HIP device is usable                                  */

/* ---- decomposition + constants (host only) -------------------------------------------------------- */
/* core::Coupler::distribute_mpi_and_allocate_coupled_state, coupler.h:110-214 (factorisation :133-140,
 * index ranges :147-153, neighbour matrix :169-179).  Fills nx,ny,nx_glob,ny_glob,i_beg,j_beg,px,py,
 * nproc_x,nproc_y,neigh of *g; leaves the rest untouched. */
int  mw_decompose(int nranks, int myrank, long long nx_glob, long long ny_glob, mw_grid_t *g);
/* Physical constants exactly as Microphysics_Kessler::init then Dynamics::init leave them in the coupler
 * options: microphysics_kessler.h:29-41,86-95 ; dynamics_euler_stratified_wenofv.h:1227-1249. */
int  mw_default_constants(mw_grid_t *g);
/* Dynamics_Euler_Stratified_WenoFV::compute_time_step, dynamics_euler_stratified_wenofv.h:70-77 */
double mw_dycore_compute_time_step(const mw_grid_t *g);

/* ---- dycore --------------------------------------------------------------------------------------- */
/* Allocates the device workspace (two halo'd prognostic slabs + six flux arrays, reused across calls --
 * the reference re-allocates them every call/cycle/stage, :97-98,:112-115,:260-265).  `stream` is a
 * hipStream_t (NULL = default stream); all work of this handle is ordered on it.
 * tracer_positive / tracer_adds_mass: host arrays [num_tracers], Coupler::get_tracer_info (:1285-1293).
 * Fails (before any large allocation) when one variable of the block's halo'd slab has 2^31 or more elements (16 GB): the kernels keep
 * their strides in 32 bits, and four slabs of such variables would not fit the GPU anyway. */
int  mw_dycore_create(mw_dycore_t *h, const mw_grid_t *g, const unsigned char *tracer_positive,
                      const unsigned char *tracer_adds_mass, void *stream);
void mw_dycore_destroy(mw_dycore_t h);

/* Dynamics_Euler_Stratified_WenoFV::init, :1197-1683 (file output :1659 excluded).  Builds the hydrostatic
 * background + immersed_proportion for `init_data` (MW_DATA_*), sets bc_x/bc_y/bc_z/use_immersed/latitude as
 * the reference does, and writes the initial COUPLER fields (density_dry,uvel,vvel,wvel,temp,tracers[T]). */
int  mw_dycore_init(mw_dycore_t h, int init_data, double *density_dry, double *uvel, double *vvel, double *wvel,
                    double *temp, double *const *tracers /* host array of T device ptrs */);
/* For callers that build their own initial state: set the persistent background directly.
 * hy_*: HOST arrays (nz,nens) / (nz+1,nens); immersed_proportion: DEVICE (nz,ny,nx,nens) or NULL (= zeros). */
int  mw_dycore_set_background(mw_dycore_t h, const double *hy_dens_cells, const double *hy_dens_theta_cells,
                              const double *hy_dens_edges, const double *hy_dens_theta_edges,
                              const double *immersed_proportion);
/* Copies the background to HOST arrays (any may be NULL).  Registered in the coupler by the reference at
 * :1663-1668 (cells) ; edges are module members :53-54. */
int  mw_dycore_get_background(mw_dycore_t h, double *hy_dens_cells, double *hy_dens_theta_cells,
                              double *hy_dens_edges, double *hy_dens_theta_edges);
/* DEVICE pointer of immersed_proportion (nz,ny,nx,nens), registered by the reference at :1313. */
double *mw_dycore_immersed_proportion(mw_dycore_t h);
/* Current grid/options of the handle (bc_*, use_immersed, latitude may have been set by mw_dycore_init). */
int  mw_dycore_get_grid(mw_dycore_t h, mw_grid_t *g);
/* coupler options "bc_x","bc_y","bc_z" (read at :588-590, :846-848); mw_dycore_init sets them like :1332-1334. */
int  mw_dycore_set_bc(mw_dycore_t h, int bc_x, int bc_y, int bc_z);
/* Kernel path.  0 (default): production path (shared reconstruction, marching kernels, state fluxes never
 * materialised; re-associated WENO and series pressure).  1: "strict": the general flux-materialising kernels in the
 * reference's exact operation order with FMA contraction off (diagnostic / parity proof; also env MW_STRICT=1 at
 * create).  2: the general flux-materialising kernels with the fast arithmetic (A/B of the two kernel structures). */
int  mw_dycore_set_strict(mw_dycore_t h, int strict);
/* Run-time options of a handle (no reference counterpart: the reference's variants are compile-time).  They replace the MW_* environment
 * switches of rounds 1-4: typed integers stored in the handle, read when the schedule of a time step is decided; no entry point of this
 * library reads the environment per call (the two process defaults left: MW_STRICT=1 at mw_dycore_create, MW_RCCL_LANES for the
 * built-in transport).  Schedule: "overlap" (-1 automatic | 0 | 1: the two-stream schedule), "pipe" (1: the pipelined schedule of a
 * decomposed block), "pipe_edge_inline", "pipe_convert", "pipe_split_edges", "pipe_maps_early".  Kernel forms: "spec" (folded configurations), "wrap" (index wrap on one
 * rank), "y_all", "y_all_conv", "member_major", "mm_direct", "mm_conv", "fused_convert", "fused_convert_mm", "fused_tracers", "tf_rows4", "zero_skip" (the
 * marching kernels skip the reconstructions of a tracer that is exactly zero over a wavefront's whole stencil: bit-neutral, 1 by default),
 * "zero_rows" (on top of it: per sub-cycle a map of the x rows in which a tracer can be non-zero -- scanned from the input, grown by the three
 * cells per direction an RK stage can move it, OR-ed with the neighbour blocks' maps on a decomposed domain -- lets the fused tracer
 * kernel neither load nor compute rows of cloud / rain that are zero; same results, 1 by default), "zero_stores" (... nor store zeros over
 * rows that hold zeros already: the coupler's own arrays, the stage slabs; 1 by default), "zero_verify" (a test aid, 0 by default: every
 * claim of the maps is checked against the data in front of the launch that relies on it -- mw_debug_zero_violations).
 * Launch shapes: "chunk_y", "chunk_yt", "chunk_z", "chunk_f" (cells per chunk, 0 = the chunk model), "chunk_model".  Built-in transport
 * (read when mw_dycore_use_rccl / _self installs it): "rccl_lanes" (0 = process default | 1 | 2), "rccl_two_comms" (-1 | 0 | 1), "rccl_prio" (1: side streams at the highest priority), "rccl_inline" (1: the group runs on the caller's stream, no side stream),
 * "xchg_fuzz" (seed of random delays around the sends / receives; a test aid), "debug_no_patch" (a test aid: the y-face correction pass of the
 * fused tracer stage is not launched -- the negative control of the FCT tests).  "vapour_state" (default 1; the folded supercell configuration
 * with one member and WENO-5 on the one-stream schedule behind k_y_all, ignored elsewhere: the water vapour is advanced by the x/z state kernel and the
 * tracer stage works on cloud and rain only; a stage in which a vapour cell fails the limiter test is redone by the three-tracer tracer stage;
 * results are bit for bit those of 0), "debug_vapour_redo" (a test aid: every stage takes that redo), "lean_stores" (default 1; with
 * "vapour_state" and the zero-row maps: the x/z state kernel does not store the face fluxes and selectors -- last stage: nor the result slab's
 * density and pressure slots -- that only the tracer stage's full iterations read where the maps say lean, a replay launch stores them when the
 * vapour is redone, and all-lean tracer waves leave their zero flag bytes out while the buffer is known to hold zeros; results are bit for bit
 * those of 0).  Unknown keys and out-of-range values are errors.  (The
 * experiment builds of rounds 4-5 -- the fused x-y-z state kernel, the balanced launch lists, the timing hooks -- left the tree in round 6.) */
int  mw_dycore_set_option(mw_dycore_t h, const char *key, long long value);
int  mw_dycore_get_option(mw_dycore_t h, const char *key, long long *value);
/* Optional parts this build of the library contains: always 0 (there are none any more; kept in the ABI). */
int  mw_build_flags(void);
/* WENO order, the reference's compile-time -DMW_ORD (dynamics_euler_stratified_wenofv.h:24-29; 3 in build/machines/aws/aws_a100_gpu.env:21):
 * 5 (default), 3, 7 or 9.  Call before mw_dycore_init (the supercell initial data uses `ord` GLL points, :1725-1886).  Orders 3, 7
 * and 9 run on the general flux-materialising kernels; 7 and 9 (WenoLimiter<7> / <9>, hs = 3 / 4) re-allocate the handle's slabs
 * with 4- / 5-cell x, y halos and 3 / 4 z levels and exchange strips of that depth. */
int  mw_dycore_set_order(mw_dycore_t h, int ord);

/* Dynamics_Euler_Stratified_WenoFV::time_step(coupler, dt_phys), :81-198: convert-in, ncycles x SSPRK3,
 * convert-out, etime += dt_phys.  Fields are updated in place.  Asynchronous on the handle's stream. */
int  mw_dycore_time_step(mw_dycore_t h, double *density_dry, double *uvel, double *vvel, double *wvel, double *temp,
                         double *const *tracers /* host array of T device ptrs */, double dt_phys);
/* One compute_tendencies(state(coupler fields), dt) as the first RK stage sees it, :204-552: fills the six
 * public flux arrays and writes state_tend (5,nz,ny,nx,nens) / tracers_tend (T,nz,ny,nx,nens) (DEVICE, may be
 * NULL).  Test/diagnostic entry; the fields are not modified. */
int  mw_dycore_compute_tendencies(mw_dycore_t h, const double *density_dry, const double *uvel, const double *vvel,
                                  const double *wvel, const double *temp, double *const *tracers, double dt,
                                  double *state_tend, double *tracers_tend);
/* The six persistent flux arrays the reference registers "so the user has access", :1671-1676:
 * out[0..2] = state_flux_x,y,z (5,nz[+1],ny[+1],nx[+1],nens); out[3..5] = tracers_flux_x,y,z (T,...). DEVICE. */
int  mw_dycore_get_fluxes(mw_dycore_t h, double **out6);
double mw_dycore_get_etime(mw_dycore_t h);   /* member etime, :55 */
/* Name + total time (ms) of this handle's kernels measured with hipEvents on the handle's stream since the
 * last reset (enabled by mw_dycore_profile(h,1); mw_dycore_profile(h,2) times class 0 only -- two events per launch of the
 * dominant kernel instead of two around every kernel, whose markers cost about 2 % of the step); which: 0 x/z flux stencil + state update (k_xz_state; k_flux on the
 * general path), 1 fct (general path) / y-face correction pass of the fused tracer stage, 2 update (general path; tracer update
 * of the unfused production path), 3 halo, 4 convert, 5 y stencil state, 6 y stencil tracers, 7 x/z tracer stage (fused:
 * fluxes + FCT + update), 8 one whole RK stage of the production path (first to last launch on the handle's stream; also
 * recorded by mw_dycore_profile(h,2)), 9 one whole mw_dycore_time_step (the only class of mw_dycore_profile(h,3): two events per time step
 * instead of twelve -- the per-stage pairs of mode 2 cost 1.5 % of the step they time), 10 / 11 (mode 1, pipelined schedule of a decomposed
 * block): the time the compute stream sits waiting for the stage's state strips / tracer strips -- what the exchange costs on the critical path. */
/* Which schedule the last mw_dycore_time_step chose: 0 one stream, 1 two streams (state | tracer pipelines), 2 pipelined one-stream
 * schedule of a decomposed block; + 4: y faces of all variables in one launch (k_y_all); + 8: general (flux-materialising) kernels. */
int  mw_dycore_schedule(mw_dycore_t h);
/* The same decision spelled out (valid until the handle's next call): "march | general-strict | general-fast", the WENO order, and on the
 * marching kernels the folded configuration (K0 | K1 | K2), the internal layout (nens1 | fused_members | member_major | mm_direct), the
 * schedule (one_stream | two_stream | pipe), y_all | y_split, where D1 happened (conv_in_y | conv_pipe | conv_pass), tracers_fused |
 * tracers_unfused, 2d | 3d, "transport" with a halo exchange installed.  The tests log it with every parity comparison and assert at
 * session end that every combination the dispatcher can produce was compared (tests/conftest.py). */
const char *mw_dycore_path(mw_dycore_t h);
int  mw_dycore_profile(mw_dycore_t h, int enable);
int  mw_dycore_profile_get(mw_dycore_t h, int which, double *total_ms, long long *launches);

/* Diagnostic: weno::WenoLimiter<5>::compute_limited_coefs + coefs_to_gll_lower<5,2> (WenoLimiter.h:68-93, TransformMatrices.h:1132-1144)
 * on n caller-supplied 5-cell stencils (DEVICE (n,5)) -> the two edge values (DEVICE (n,2)); strict = 1: the reference's operation
 * order with contraction off, 0: the production arithmetic (mw_weno.h). */
int  mw_weno5_edges(long long n, const double *stencils, double *edges, int strict, void *stream);
/* Diagnostic: out[i] = pow(x[i], y[i]) as the kernels that keep the reference's operation order compute it (strict path, init,
 * D1 / D13 passes): glibc's algorithm and tables (csrc/mw_glibc_pow.h), i.e. the bits of the host libm's pow that the reference
 * built with the YAKL serial backend gets (dynamics_euler_stratified_wenofv.h:401, :1935, :2009).  main_path (device, n bytes,
 * may be NULL): 1 where the restated main path applied, 0 where the device library's pow was used (arguments the dycore never
 * produces: x <= 0 or subnormal, |y| < 2^-65 or >= 2^63, over- / underflowing results). */
int  mw_strict_pow(long long n, const double *x, const double *y, double *out, unsigned char *main_path, void *stream);

/* Measurement aid (no reference counterpart): copies n doubles with this library's access shape (8 B per lane).  A launch
 * moves exactly 8n bytes each way, which calibrates rocprofv3's FETCH_SIZE / WRITE_SIZE counters (tools/calib_pmc.py). */
int  mw_calib_copy(const double *in, double *out, long long n, void *stream);

/* Calibration (no reference counterpart; SURVEY.md 8(d) asks for a measured fp64 ceiling).  mw_calib_fma64: independent v_fma_f64
 * chains, `waves_per_simd` (1..8) wavefronts per SIMD on every CU for about `seconds`; out5 (HOST) = wave-instructions per second,
 * kernel ms, shader clock GHz during the run (0 if the part's two counters tick alike), wave-instructions issued, CUs.
 * mw_calib_stage_arith: the arithmetic of one RK stage and nothing else -- per cell 24 WENO-5 reconstructions + 3 Riemann solves + the
 * passive fluxes (the production arithmetic) on register windows fed from `tab`, DEVICE (nlev >= 6, 8, 64) doubles that stay in L2
 * (variables rho', u, v, w, (rho theta)', q_v, q_c, q_r of a 64-cell row; smooth or rough data as the caller likes), `levels` cells per
 * thread, 256-thread workgroups, two per CU (k_xz_state's shape and register budget).  active_tracers = 3: all 24 reconstructions; 1: cloud and rain
 * exactly zero, which the production kernels do not reconstruct (option zero_skip): 18 per cell, the floor of a stage on a cloud-free state.  bg4 (HOST): hy_dens, hy_dens_theta, C0
 * hy_dens_theta^gamma, 1 / hy_dens_theta of the level.  sink: DEVICE, mw_calib_stage_arith_threads(cells, levels) doubles.  out3
 * (HOST): ms of the timed launch, cells processed, workgroups.  No stage of that many cells can take less on this chip. */
int  mw_calib_fma64(int waves_per_simd, double seconds, double *out5, void *stream);
long long mw_calib_stage_arith_threads(long long cells, int levels);
int  mw_calib_stage_arith(const double *tab, int nlev, long long cells, int levels, int active_tracers, const double *bg4, double *sink, double *out3, void *stream);
/* Test aid: occupies `stream` for about `usec` microseconds (delay fuzz of the exchange tests). */
int  mw_debug_spin(long long usec, void *stream);
/* Test aid: the names (as the code object spells them -- mangled; newline-separated) of the dycore kernels this PROCESS has launched since
 * the last reset; every instantiation of the dispatcher's kernel templates has its own.  Returns the bytes needed (terminator included)
 * and writes at most `cap`; reset != 0 clears the registry.  (tests/conftest.py: instantiation coverage of the parity comparisons.) */
long long mw_debug_launched_kernels(char *buf, long long cap, int reset);
/* Test aid: the zero-row maps of the handle's LAST sub-cycle, copied to HOST memory after a stream synchronise: ten maps of
 * nz * (ny + 18) 32-bit words each -- M0, Q1..Q3, FN1..FN3, QY1..QY3; word of (level k, row j) at [k * (ny + 18) + j + 9], bit v = tracer v.
 * Returns the number of words (0: the last time step ran without maps), writes at most cap_words; dims2 = {nz, ny + 18}. */
long long mw_debug_zero_maps(mw_dycore_t h, unsigned int *out_host, long long cap_words, int *dims2);
/* Test aid: option "zero_verify" = 1 makes every time step check the zero-row maps' claims against the data, right in front of the launches
 * that rely on them (k_zero_verify): [0] / [1] a tracer that can vanish is non-zero in a row of a stage's input although the map of the fused
 * tracer kernel / of the y kernel says it cannot be; [2] / [3] a destination row whose store of zeros is about to be skipped (slab S1 / S2,
 * the coupler's arrays / the slab the converting y launch fills) is not all zero.  Returns the sum of the four counters since the handle was
 * created (out4, may be NULL: the four), -1 when the option never ran.  No reference counterpart. */
long long mw_debug_zero_violations(mw_dycore_t h, unsigned long long *out4);
/* Test aid: how many RK stages of the last time step redid their water vapour in the tracer stage's three-tracer form (option "vapour_state":
 * a cell failed the limiter test in the x/z state kernel, or "debug_vapour_redo" asked for it); 0 when no stage ran the vapour form, -1 for a
 * null handle.  No reference counterpart. */
long long mw_debug_vapour_redo(mw_dycore_t h);
/* Test aid: the fused tracer stage's per-cell flag bytes ("this cell scaled its south / north face of tracer v": bits 2v / 2v + 1) as the
 * last launch left them, index (k * ny + j) * nx * nens + x; at most cap bytes go to out_host (host memory).  Returns the number of cells,
 * -1 on error.  No reference counterpart. */
long long mw_debug_tracer_flags(mw_dycore_t h, unsigned char *out_host, long long cap);
/* Test aid of option "lean_stores": fills what the x/z state kernel hands to the tracer stage with values no reader survives -- both parities
 * of the x and z mass-flux arrays with NaN and of their selector bytes with 0xFF, and the density and pressure slots of the slab that the last
 * stage of the next time step writes (one sub-cycle) with NaN.  A reader that consumes an entry the kernel left out turns its result into
 * NaN.  Returns 0, 1 on error.  No reference counterpart. */
int  mw_debug_poison_handoff(mw_dycore_t h);

/* modules::perturb_temperature(coupler, thermal=true, random=false), perturb_temperature.h:41-66 */
int  mw_perturb_temperature(const mw_grid_t *g, double *temp, void *stream);
/* the random = true branch, perturb_temperature.h:25-39 (applied BEFORE the thermal, as there): +-3 K uniform noise on the lowest
 * nz/4 levels, fading linearly; one draw per (level, column) from the key myrank*nz*nx*ny*nens + k*ncol + i.  yakl::Random is
 * unavailable: the key goes through the splitmix64 finaliser ("Substitutions"). */
int  mw_perturb_temperature_random(const mw_grid_t *g, double *temp, void *stream);

/* ---- multi-GPU halo exchange ---------------------------------------------------------------------- */
/* halo_exchange, :574-747 (MPI_Isend/Irecv W/E/S/N, tags 0-3).  The native design ships a 3-cell halo once
 * per RK stage and reconstructs the neighbour's edge values locally, which makes edge_exchange (:830-1003)
 * unnecessary (bitwise identical: reconstruction is a pure function of the 5-cell stencil).
 * The callback receives DEVICE buffers packed as (V,nz,ny,3,nens) [W/E] and (V,nz,3,nx,nens) [S/N] and must
 * deliver sendW to the west neighbour's recvE etc., ordered on `stream`.  NULL => single-rank periodic wrap. */
/* Posting plan of one exchange (host only; single source of truth for mw_rccl.cpp and for the CPU gloo tests):
 * peers[4] = west, east, south, north rank (neigh(1,0), neigh(1,2), neigh(0,1), neigh(2,1), :651-655);
 * send_order[4] / recv_order[4] = directions (0 W, 1 E, 2 S, 3 N) in posting order.  Messages between one pair of
 * ranks match in FIFO order, so when west == east (two ranks in x) or south == north the receives are posted E,W / N,S
 * against sends W,E / S,N: the peer's first send (its W strip) is my E halo.  active[4]: direction takes part
 * (more than one rank in that direction and, for S/N, a 3-D run). */
int  mw_exchange_plan(const mw_grid_t *g, int *peers, int *send_order, int *recv_order, int *active);
typedef int (*mw_exchange_fn)(void *ctx, const double *sendW, const double *sendE, const double *sendS,
                              const double *sendN, double *recvW, double *recvE, double *recvS, double *recvN,
                              long long nWE, long long nSN, void *stream);
int  mw_dycore_set_exchange(mw_dycore_t h, mw_exchange_fn fn, void *ctx);
/* Built-in exchange over RCCL point-to-point (ncclSend/ncclRecv in one group on a side stream).
 * unique_id: the 128-byte ncclUniqueId created on rank 0 (mw_rccl_unique_id) and broadcast by the host. */
int  mw_rccl_unique_id(unsigned char *id128);
int  mw_dycore_use_rccl(mw_dycore_t h, const unsigned char *id128, int nranks, int myrank);
/* Test transport (no reference counterpart): ONE rank plays every rank of the handle's nproc_x x nproc_y rank grid -- a 1-rank
 * communicator, every active direction's peer is this rank itself (sends W,E,S,N matched FIFO by receives E,W,N,S), i.e. the messages a
 * block exchanges with neighbours that hold the same data.  For a periodic domain tiled from copies of one block the handle's result
 * equals the one-rank run of that block bit for bit, with the real send / receive groups, side streams and event pairs of
 * halo_exchange's replacement in flight beside compute on one GPU.  mw_dycore_rccl_allreduce_sum on such a handle multiplies by the
 * number of blocks (identical contributions; exact), mw_dycore_rccl_bcast is the identity. */
int  mw_dycore_use_rccl_self(mw_dycore_t h);
/* RCCL is resolved at run time from the librccl ALREADY mapped in the process (a PyTorch host: torch's own, the one behind
 * torch.distributed's "nccl" backend), else from the loader's search path -- never two RCCLs in one process.  Returns the
 * path it came from ("" when none is available) and, optionally, its version code (ncclGetVersion). */
const char *mw_rccl_library_path(int *version);
/* ncclCommCount / ncclCommUserRank of the installed transport's communicator, and its number of lanes (side streams): what a
 * multi-GPU run reports as evidence that RCCL connected all ranks.  Error if the handle's transport is not the built-in RCCL one. */
int  mw_dycore_rccl_info(mw_dycore_t h, int *comm_ranks, int *comm_rank, int *lanes);
/* The other two collectives of a decomposed run, on the handle's communicator, for hosts without torch.distributed / MPI:
 * MPI_Allreduce(SUM) of sponge_layer.h:53-63 / column_nudging.h:89-99 -- pass this function as the mw_allreduce_fn of mw_sponge_layer /
 * mw_column_average / mw_nudge_to_column with ctx = the dycore handle -- and MPI_Bcast(root) of horizontal_sponge.h:72-77.  DEVICE
 * buffers, in place, ordered on `stream`. */
int  mw_dycore_rccl_allreduce_sum(void *dycore_handle, double *buf, long long n, void *stream);
int  mw_dycore_rccl_bcast(mw_dycore_t h, double *buf, long long n, int root, void *stream);
/* Diagnostic: one rank sends 4 strips of n doubles to itself through the exchange's own ncclGroup / side stream / event
 * sequence and compares; 0 = RCCL initialises on this box and the ordering against `stream` holds. */
int  mw_rccl_selftest(long long n, void *stream);
/* What the last mw_rccl_selftest drove: 10 x the number of exchange lanes (side stream + event pair each; one per pipeline of the
 * two-stream schedule) + the number of communicators behind them: 21 = two lanes on one communicator (default), 22 = a communicator
 * per lane (split with ncclCommSplit).  mw_rccl_selftest_config chooses the form of the following self-tests of this process: lanes
 * 1 | 2 (0 = back to the process default, MW_RCCL_LANES = "1" | "2" | "2x2"), two_comms 0 | 1. */
int  mw_rccl_selftest_lanes(void);
int  mw_rccl_selftest_config(int lanes, int two_comms);

/* ---- Kessler microphysics ------------------------------------------------------------------------- */
/* Microphysics_Kessler::time_step(coupler, dt), microphysics_kessler.h:99-162 + kessler() :234-339.
 * (nz,ncol) views of water_vapor, cloud_liquid, precip_liquid, density_dry(const), temp; precl (ncol).
 * rainsplit is taken from THIS rank's minval exactly like the reference (:276-279).  workspace: DEVICE scratch
 * of mw_kessler_workspace_bytes(nz,ncol) bytes.  rainsplit_out: optional HOST int (forces a stream sync). */
long long mw_kessler_workspace_bytes(int nz, long long ncol);
int  mw_kessler_time_step(int nz, long long ncol, double dz, double dt, double *rho_v, double *rho_c, double *rho_r,
                          const double *rho_d, double *temp, double *precl, void *workspace, int *rainsplit_out,
                          void *stream);
/* 1: the STRICT Kessler path -- the reference's formulas in the reference's operation order (theta form, IEEE divisions, no
 * contraction) with glibc's pow and exp (csrc/mw_glibc_pow.h): the bits microphysics_kessler.h:99-162, :234-339 produces on a glibc
 * host (YAKL serial backend).  0 (default): the production kernels (1e-12 from it).  Process-wide, like the module's constants. */
int  mw_kessler_set_strict(int strict);
/* Host only, no device needed: the z-chunk length of the rainsplit == 1 sweep for nz levels and `columns` kernel columns (ncol, or
 * ncol * nens for the teacher).  It is nz (one chunk) or one of 25, 20, 16, 12, 10, 8, 5, 4 below nz, so a column is cut into at most
 * nz / 4 + 1 chunks -- the bound the flux_top rows of the two workspace formulas rest on. */
int  mw_kessler_chunk(int nz, long long columns);
/* Test aid, per calling thread like mw_kessler_set_strict: replaces that rule in mw_kessler_time_step and mw_kessler_members_teacher.
 * 0 restores the rule; one of 4, 5, 8, 10, 12, 16, 20, 25 is used where it is < nz (else the column is one chunk); any value >= 1024
 * forces one chunk.  Anything else is an error: a chunk below 4 would overrun the flux_top rows.  The results do not depend on it. */
int  mw_kessler_debug_set_chunk(int chunk);

/* ponni::load_h5_weights<N>(file, group, dataset), microphysics_kessler_ponni.h:103-107: one 32-bit float dataset of an HDF5 file
 * (the Keras weight file `keras_weights_h5`: "/dense_6/dense_6" "kernel:0" (5,10), "bias:0" (10), "/dense_7/dense_7" ...), read by a
 * dependency-free HOST reader (old-style groups, contiguous / compact little-endian float data; anything else is refused).
 * out == NULL: shape query.  dims: up to 8 extents, ndims: rank.  capacity: number of floats `out` holds. */
int  mw_h5_read_f32(const char *file, const char *group, const char *dataset, float *out, long long capacity, long long *dims, int *ndims);

/* mean(a - b) over n DEVICE doubles -- the surrogate module's "Relative diff" prints, microphysics_kessler_ponni.h:266-269
 * (yakl::intrinsics::sum(a - b) / size there).  Deterministic order.  workspace1024: DEVICE scratch of 1024 doubles; mean_out: HOST. */
int  mw_mean_diff(long long n, const double *a, const double *b, double *workspace1024, double *mean_out, void *stream);

/* Diagnostic (no reference counterpart): the Kessler module's own log (fn 0), exp (1), sqrt (2) and reciprocal (3) -- short
 * forms for positive finite arguments, see mw_kessler.hip -- on n caller-supplied DEVICE doubles. */
int  mw_kessler_math_probe(long long n, const double *x, double *y, int fn, void *stream);

/* ---- sponge layer + column nudging (the two remaining per-step modules of the supercell loop) ---- */
/* Sums `buf` (DEVICE, n doubles) in place over all ranks, ordered on `stream` -- MPI_Allreduce(SUM) in the reference
 * (sponge_layer.h:53-63, column_nudging.h:89-99).  Pass NULL on a single rank. */
typedef int (*mw_allreduce_fn)(void *ctx, double *buf, long long n, void *stream);
/* DEVICE scratch size for the three calls below (num_fields = 5 + T for the sponge, 5 for the nudger). */
long long mw_column_workspace_bytes(const mw_grid_t *g, int num_fields);
/* modules::sponge_layer(coupler, dt, time_scale = 60), sponge_layer.h:8-77: relax the top 10 levels of every field to the
 * horizontal mean (w to zero).  fields: HOST array of num_fields DEVICE pointers in the reference's MultiField order
 * (density_dry, uvel, vvel, wvel, temp, tracers...).  Horizontal sums are deterministic (no atomics). */
/* 1: the horizontal sums of mw_sponge_layer / mw_column_average / mw_nudge_to_column are added in the reference's SERIAL order
 * (j, then i: sponge_layer.h:44-51, column_nudging.h:80-87 on the YAKL serial backend) by one thread per (field, level, member), which
 * makes the two modules bit-identical to that backend; 0 (default): deterministic fixed-slice tree sums.  Process-wide. */
int  mw_column_set_strict(int strict);
int  mw_sponge_layer(const mw_grid_t *g, double *const *fields, int num_fields, double dt, double time_scale, void *workspace,
                     mw_allreduce_fn allreduce, void *ctx, void *stream);
/* ColumnNudger::get_column_average, column_nudging.h:69-106: state5 = density_dry, uvel, vvel, temp, water_vapor;
 * column_out: DEVICE (5,nz,nens).  set_column (:15-36) is this call on the initial state. */
int  mw_column_average(const mw_grid_t *g, const double *const *state5, double *column_out, void *workspace,
                       mw_allreduce_fn allreduce, void *ctx, void *stream);
/* ColumnNudger::nudge_to_column(coupler, dt), :39-66: state += dt (column - column_average(state)) / 900. */
int  mw_nudge_to_column(const mw_grid_t *g, double *const *state5, const double *column, double dt, void *workspace,
                        mw_allreduce_fn allreduce, void *ctx, void *stream);
/* The same, DEFERRED (round 6; no reference counterpart -- the reference's nudge_to_column is two passes): the horizontal sums are taken and the
 * increments dt (column - average) / 900 are PARKED in the dycore handle instead of being added by a second pass over the five fields.  The
 * handle's next mw_dycore_time_step adds them while its conversion loads the coupler's arrays (the same rounded addition: results are bit for
 * bit those of mw_nudge_to_column), on the one-rank production path of the supercell configuration; any other path, and
 * mw_dycore_compute_tendencies, applies them with a pass first.  Between this call and that time step the five arrays do NOT hold the nudged
 * values: whoever reads them must call mw_dycore_flush_pending first (the Coupler mirrors do so inside DataManager::get).  The grid is the
 * handle's; sums and increments are ordered on the handle's stream.  state5: density_dry, uvel, vvel, temp, water_vapor -- the arrays later
 * handed to mw_dycore_time_step. */
int  mw_nudge_to_column_deferred(mw_dycore_t h, double *const *state5, const double *column, double dt, void *workspace,
                                 mw_allreduce_fn allreduce, void *ctx);
/* Applies parked increments now (a no-op when there are none). */
int  mw_dycore_flush_pending(mw_dycore_t h);
/* 1 while increments are parked; out2 (may be NULL): how often parked increments rode on a conversion / were applied by a pass, since create. */
int  mw_dycore_pending(mw_dycore_t h, unsigned long long *out2);

/* ---- ponni surrogate MLP -------------------------------------------------------------------------- */
/* NN block of custom_modules::Microphysics_Kessler::time_step,
 * experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:176-202
 * (ponni::Matvec,Bias,Relu(0.1),Matvec,Bias ; model.forward_batch_parallel :189), fused with the min-max
 * input scaling :182-186 and output un-scaling + clip :198-201.  W1 (5,10), b1 (10), W2 (10,4), b2 (4):
 * HOST fp32, Keras (in,out) layout; scl_in (5,2), scl_out (4,2): HOST fp64 [min,max] rows. */
int  mw_mlp_forward(long long ncells, const double *temp, const double *rho_d, const double *rho_v,
                    const double *rho_c, const double *rho_r, const float *W1, const float *b1, const float *W2,
                    const float *b2, const double *scl_in, const double *scl_out, double *temp_out,
                    double *rho_v_out, double *rho_c_out, double *rho_r_out, void *stream);
/* 1: the strict form -- thread per cell, fp32 accumulation in index order, no contraction (the order in which the layers are defined,
 * microphysics_kessler_ponni.h:103-110); 0 (default): the MFMA kernels (the same products summed in the matrix cores' order). */
int  mw_mlp_set_strict(int strict);

/* The STENCIL model 9 -> 10 -> 4 on the coupler's fields: the network the sample files are written for.  Features 0..4 are the cell's
 * (temp, rho_d, rho_v, rho_c, rho_r); features 5..8 are (temp, rho_v, rho_c, rho_r) of level min(nz - 1, k + 1) of the same column and
 * ensemble member -- DataGenerator::generate_samples_stencil's inputs(:, 0:5, 0) and inputs(:, 0:4, 1),
 * experiments/supercell_kessler_surrogate/custom_modules/generate_micro_surrogate_data.h:139-156; the layers, the scaling and the
 * un-scaling + clip are mw_mlp_forward's (microphysics_kessler_ponni.h:103-110, :182-186, :198-201).  Fields: DEVICE fp64, level-major
 * (cell (k, col) at k * ncol + col, ncol = ny * nx * nens).  W1 (9,10), b1 (10), W2 (10,4), b2 (4): HOST fp32, Keras layout; scl_in
 * (9,2), scl_out (4,2): HOST fp64 [min,max] rows.  The four outputs must not overlap any input (level k + 1 is an input of level k):
 * overlap is an error.  Honours mw_mlp_set_strict: 0 = MFMA tiles, a wave sweeps 16 columns top-down and carries the level above in
 * registers, every input read once plus one level per z chunk; 1 = thread per cell, index order, no contraction. */
int  mw_mlp_stencil_forward(int nz, long long ncol, const double *temp, const double *rho_d, const double *rho_v, const double *rho_c,
                            const double *rho_r, const float *W1, const float *b1, const float *W2, const float *b2,
                            const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out, double *rho_c_out,
                            double *rho_r_out, void *stream);
/* The number of levels of one z chunk that mw_mlp_stencil_forward's MFMA kernel uses for (nz, ncol) (nz: a single chunk). */
int  mw_mlp_stencil_chunk(int nz, long long ncol);

/* The two OUTPUT FORMS of a surrogate model.  MW_FORM_STATE: the network's output is the new state, y = (double)o * rng + min, the water
 * fields then max(0, y) -- mw_mlp_forward / mw_mlp_stencil_forward, the reference's form.  MW_FORM_TENDENCY: the output is the CHANGE, and
 * it is added in fp64 to the cell's own temp, rho_v, rho_c, rho_r (input features 0, 2, 3, 4 of the cell's own level, for the stencil
 * model too; no reference counterpart):
 *   d_j = (double)o_j * (max_j - min_j) + min_j          scl_out rows: [min, max] of (after - before)
 *   y_0 = base_0 + d_0 ,  y_j = fmax(0.0, base_j + d_j)  j = 1, 2, 3; fp64, no contraction, this association
 * The input scaling, both layers, the activation and the order of the fp32 sums are mw_mlp_forward's.  The two functions take the
 * arguments of mw_mlp_forward / mw_mlp_stencil_forward behind `form` and honour mw_mlp_set_strict; form 0 writes the bits of those
 * functions (which call these), any other value than the two is an error.  HBM traffic stays 72 B per cell: lane group g > 0 of the MFMA
 * kernels reads its base from a line that another group of the same wave loads in the same iteration. */
#define MW_FORM_STATE 0
#define MW_FORM_TENDENCY 1
int  mw_mlp_forward_form(int form, long long ncells, const double *temp, const double *rho_d, const double *rho_v,
                         const double *rho_c, const double *rho_r, const float *W1, const float *b1, const float *W2,
                         const float *b2, const double *scl_in, const double *scl_out, double *temp_out,
                         double *rho_v_out, double *rho_c_out, double *rho_r_out, void *stream);
int  mw_mlp_stencil_forward_form(int form, int nz, long long ncol, const double *temp, const double *rho_d, const double *rho_v,
                                 const double *rho_c, const double *rho_r, const float *W1, const float *b1, const float *W2, const float *b2,
                                 const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out, double *rho_c_out,
                                 double *rho_r_out, void *stream);

/* ponni's own surface: ponni::Inference<...>::forward_batch_parallel(float2d in(num_in, batch)) -> float2d
 * (num_out, batch), experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h:40-45,103-110,189, for a stack
 * of ponni::Matvec<float> (kind 0: weights (n_in, n_out) in Keras order, y = x W), ponni::Bias<float> (kind 1) and ponni::Relu<float>(n,
 * negative_slope) (kind 2) layers.  layers / params: HOST memory (params = all weights back to back, `offset` in floats); in / out:
 * DEVICE fp32, batch fastest.  The surrogate's stacks (5 -> 10 -> 4 and 9 -> 10 -> 4) run on the MFMA tiles, any other stack of up to 10 layers, widths
 * <= 32 and 960 parameters on a thread-per-element kernel; a size mismatch between consecutive layers is an error (Inference::validate). */
typedef struct { int kind, n_in, n_out; float negative_slope; int offset; } mw_ponni_layer_t;
int  mw_ponni_forward(const mw_ponni_layer_t *layers, int nlayers, const float *params, int nparams, long long batch,
                      const float *in, float *out, void *stream);

/* ---- file output ------------------------------------------------------------ */
/* A minimal netCDF *classic* writer (mw_netcdf.cpp): the reference writes through PnetCDF with NC_CLOBBER | NC_64BIT_DATA,
 * i.e. the CDF-5 on-disk format, dims x,y,z (+ unlimited t), double variables, no attributes
 * (dynamics_euler_stratified_wenofv.h:2106-2131, time_averager.h:104-120).  format: 5 = CDF-5 (the reference's), 2 = CDF-2
 * (64-bit offset; same structure with 32-bit sizes -- readable by readers that predate CDF-5).  header_align / var_align are
 * PnetCDF's nc_header_align_size / nc_var_align_size hints (:2103-2104: 1048576 each; <= 0: 512 / 4).  All HOST calls.
 * Sharing: the creating rank runs create..enddef; after that any process on the node may mw_nc_open the file and write
 * disjoint hyperslabs (pwrite); the main rank publishes the record count with mw_nc_set_numrecs. */
typedef struct mw_nc_s *mw_nc_t;
int  mw_nc_create(mw_nc_t *nc, const char *path, int format, long long header_align, long long var_align);   /* nc.create        */
int  mw_nc_def_dim(mw_nc_t nc, const char *name, long long len, int *dimid);          /* create_dim; len 0 = create_unlim_dim   */
int  mw_nc_def_var(mw_nc_t nc, const char *name, int ndims, const int *dimids, int *varid);   /* create_var<real>               */
/* nc_type 4 = int, 5 = float, 6 = double (the surrogate sample files hold floats and one int, generate_micro_surrogate_data.h) */
int  mw_nc_def_var_typed(mw_nc_t nc, const char *name, int nc_type, int ndims, const int *dimids, int *varid);
int  mw_nc_enddef(mw_nc_t nc);                                                         /* nc.enddef: lays out + writes header    */
int  mw_nc_open(mw_nc_t *nc, const char *path);                                        /* nc.open (read-write)                   */
int  mw_nc_inq_varid(mw_nc_t nc, const char *name, int *varid);
int  mw_nc_inq_dimlen(mw_nc_t nc, const char *name, long long *len);                   /* get_dim_size; record dim: # records    */
int  mw_nc_put_vara_double(mw_nc_t nc, int varid, const long long *start, const long long *count, const double *host_data);
int  mw_nc_put_vara(mw_nc_t nc, int varid, const long long *start, const long long *count, const void *host_data);   /* variable's own type */
int  mw_nc_set_numrecs(mw_nc_t nc, long long numrecs);
/* Reads back (HOST, the variable's own type, C order): records [rec_start, rec_start + rec_count) of a record variable in full, record axis
 * first, or the whole of a fixed-size variable (rec_start 0, rec_count ignored) -- the reads of the training notebooks' input step
 * (kessler_netcdf_to_numpy.ipynb: nc.variables['inputs'][:], ['outputs'][:], ['time_step_size']) for the files DataGenerator writes. */
/* nc.inq_var: nc_type (4 int, 5 float, 6 double), rank, extents (up to 8; the record dimension's extent is the number of records) and
 * whether the variable's first dimension is the record dimension. */
int  mw_nc_inq_var(mw_nc_t nc, int varid, int *nc_type, int *ndims, long long *shape8, int *is_record);
int  mw_nc_get_var(mw_nc_t nc, int varid, long long rec_start, long long rec_count, void *host_data);
int  mw_nc_close(mw_nc_t nc);
/* The body of Dynamics_Euler_Stratified_WenoFV::output's variable loop, :2176-2185 (and Time_Averager::finalize's,
 * time_averager.h:131-136): ensemble member 0 of the DEVICE field (nz,ny,nx,nens) -> host -> this rank's hyperslab
 * {record, 0, j_beg, i_beg} x {1, nz, ny, nx} of variable varid (record < 0: a variable without the t dimension). */
int  mw_output_put_field(mw_nc_t nc, int varid, long long record, const mw_grid_t *g, const double *field, void *stream);

/* ---- simple_city custom modules ------------------------------------------- */
/* fields6 / avg6: HOST arrays of 6 DEVICE pointers: density_dry, uvel, vvel, wvel, temp, water_vapor. */
/* custom_modules::Horizontal_Sponge::init, horizontal_sponge.h:54-61: column (6,nz,nens) DEVICE = cell (k,0,0,iens) of this
 * rank; the reference takes the main rank's and MPI_Bcast's it (:73-78) -- the host broadcasts `column` from rank 0. */
int  mw_horizontal_sponge_column(const mw_grid_t *g, const double *const *fields6, double *column, void *stream);
/* Horizontal_Sponge::apply(coupler, dt, x1, x2, y1, y2), :101-192: cosine-weighted relaxation of the 6 fields to the stored
 * column within sponge_cells of the enabled domain edges (only on the ranks that own the edge). */
int  mw_horizontal_sponge_apply(const mw_grid_t *g, double *const *fields6, const double *column, int sponge_cells,
                                double time_scale, double dt, int x1, int x2, int y1, int y2, void *stream);
/* custom_modules::Time_Averager::accumulate, time_averager.h:37-78: avg = inertia*avg + (1-inertia)*field with
 * inertia = etime/(etime+dt); the caller advances its etime by dt afterwards (:77). */
int  mw_time_average_accumulate(const mw_grid_t *g, const double *const *fields6, double *const *avg6, double etime, double dt,
                                void *stream);

/* ---- surrogate workflow statistics ----------------------------------------- */
/* custom_modules::StatisticsGatherer::gather_micro_statistics, experiments/supercell_kessler_surrogate/custom_modules/
 * gather_micro_statistics.h:19-58: number of cells (ensemble member 0) whose temp / water_vapor / cloud_liquid /
 * precip_liquid changed by more than 1e-10 across the microphysics call (is_active, :61-74).  in4 / out4: HOST arrays of 4
 * DEVICE pointers (temp, water_vapor, cloud_liquid, precip_liquid) before / after; mask: optional DEVICE (nz,ny,nx) bytes
 * (the `active` array, :40-52); *count: the sum the reference adds to `numer` (:56).  Integer, hence exact. */
int  mw_micro_active_count(const mw_grid_t *g, const double *const *in4, const double *const *out4, unsigned char *mask,
                           long long *count, void *stream);
/* custom_modules::DataGenerator::generate_samples_stencil, .../generate_micro_surrogate_data.h:35-153, device parts.
 * mw_micro_sample_mask: mask[k,j,i] (DEVICE bytes) = u01(key0 + k*ny*nx + j*nx + i) < (is_active ? thr_active : thr_inactive),
 * :83-101; key0 = (seed + myrank)*nz*ny*nx as in the reference; u01 = splitmix64 (yakl::Random is not available).
 * mw_micro_gather_samples: for the n cell indices `cells` (DEVICE int64, k*ny*nx + j*nx + i, member 0) fills inputs (n,5,2) and
 * outputs (n,4) (DEVICE fp32) exactly as :139-156 (inputs: temp, density_dry, water_vapor, cloud_liquid, precip_liquid at k;
 * slot 1 as assigned there at min(nz-1,k+1); outputs: temp, water_vapor, cloud_liquid, precip_liquid after micro). */
int  mw_micro_sample_mask(const mw_grid_t *g, const double *const *in4, const double *const *out4, unsigned long long key0,
                          double thr_active, double thr_inactive, unsigned char *mask, void *stream);
int  mw_micro_gather_samples(const mw_grid_t *g, const double *rho_d, const double *const *in4, const double *const *out4,
                             const long long *cells, long long n, float *inputs, float *outputs, void *stream);

/* ---- surrogate training (experiments/supercell_kessler_surrogate/jupyter_notebooks) --------------------------------------- */
/* The notebooks' fit of the single-cell model, natively (csrc/mw_train.hip).  Sets are feature-major fp32 DEVICE
 * arrays, x (5, n) and y (4, n), batch fastest -- mw_ponni_forward's layout.  Parameters: (models, 104) fp32 DEVICE, per model W1 (5,10),
 * b1 (10), W2 (10,4), b2 (4) in Keras order (the order of miniweatherml_amd/data/kessler_surrogate_weights.txt); moments the same shape.
 * Permutations: a 4-round Feistel network on the smallest square power-of-two domain >= n, cycle-walked into [0, n), round keys from
 * splitmix64 -- the exact definition is the Python restatement miniweatherml_amd/surrogate_train.py (feistel_permutation). */
#define MW_SURROGATE_MAX_BATCH 8192
#define MW_SURROGATE_MAX_MODELS 256
/* kessler_netcdf_to_numpy.ipynb (np.random.shuffle of the samples) + kessler_singlecell_train_example.ipynb (min-max scaling, test_split,
 * then Keras' validation_split tail): sample p of the permutation of seed (tag 2^64 - 1) goes to position p of [train | val | test], scaled
 * as (float)(((double)v - min) / (max - min)) -- the strict inference's expression.  raw_in (n, 5), raw_out (n, 4): DEVICE fp32 (slot 0
 * of DataGenerator's inputs); scl_in (5, 2), scl_out (4, 2): HOST [min, max] rows; n_train + n_val + n_test = n. */
int  mw_surrogate_prepare(long long n, const float *raw_in, const float *raw_out, const double *scl_in, const double *scl_out,
                          unsigned long long seed, long long n_train, long long n_val, float *train_x, float *train_y, float *val_x,
                          float *val_y, float *test_x, float *test_y, void *stream);
/* One epoch of model.fit(epochs, batch_size, shuffle=True) with Nadam (kessler_singlecell_train_example.ipynb, the compile / fit cells) for
 * `models` models in ONE launch, one workgroup per model: model m visits the training set in the order of the permutation of (seed + m,
 * epoch) in batches of `batch` (the last one partial), and takes one Nadam step per batch.  table: HOST-computed per-step scalars of this
 * epoch's steps, 3 fp32 each (lr (1 - mu_t) / (1 - prod mu), lr mu_t+1 / (1 - prod mu * mu_t+1), 1 - beta2^t), ceil(n / batch) rows,
 * DEVICE.  stats (models, 2) fp64 DEVICE: sum over the epoch's samples of sum_outputs (y - t)^2 and of sum_outputs |y - t|, each sample with
 * the weights of its batch (Keras' running `loss` and `mean_absolute_error` = these / (4 n)). */
int  mw_surrogate_train_epoch(int models, const float *x, const float *y, long long n, int batch, int epoch, unsigned long long seed,
                              float *params, float *m1, float *m2, const float *table, float beta1, float beta2, float eps, double *stats,
                              void *stream);
/* Test aid: loss (1 fp32) and gradient (104 fp32, the parameters' order) of the mean squared error of ONE batch of `batch` samples x (5,
 * batch), y (4, batch), at params (104); all DEVICE.  The trainer's own batch routine, in a one-workgroup launch. */
int  mw_surrogate_batch_grad(const float *params, const float *x, const float *y, int batch, float *grad, float *loss, void *stream);
/* Error sums of `nsets` predictions pred (nsets, 4, n) against y (4, n), all DEVICE fp32 -- model.evaluate / the notebook's test metrics
 * cell.  out (nsets, 24) fp64 DEVICE: per output v at [6 v ...]: sum (y - p)^2, sum |y - p|, sum (y - p), sum |y|, max |y - p|, max |y|.
 * Fixed reduction order (run-to-run identical).  workspace: DEVICE, mw_surrogate_errors_workspace_bytes(nsets). */
/* The same three for n_in = 5 (the functions above) or n_in = 9, the stencil model: raw_in (n, 9) in the feature order of
 * mw_mlp_stencil_forward, x (9, n), scl_in (9, 2), parameters and gradient (144): W1 (9,10), b1 (10), W2 (10,4), b2 (4). */
int  mw_surrogate_prepare_v2(int n_in, long long n, const float *raw_in, const float *raw_out, const double *scl_in, const double *scl_out,
                             unsigned long long seed, long long n_train, long long n_val, float *train_x, float *train_y, float *val_x,
                             float *val_y, float *test_x, float *test_y, void *stream);
int  mw_surrogate_train_epoch_v2(int n_in, int models, const float *x, const float *y, long long n, int batch, int epoch,
                                 unsigned long long seed, float *params, float *m1, float *m2, const float *table, float beta1, float beta2,
                                 float eps, double *stats, void *stream);
int  mw_surrogate_batch_grad_v2(int n_in, const float *params, const float *x, const float *y, int batch, float *grad, float *loss,
                                void *stream);
/* mw_surrogate_prepare_v2 with the labels of an output form (MW_FORM_*).  Form 1: y = the scaled CHANGE of the sample,
 *   (float)((((double)raw_out[j] - (double)raw_in[base(j)]) - min_j) / (max_j - min_j))      base(j) = 0, 2, 3, 4
 * with scl_out rows [min, max] of (after - before); the x sets are those of _v2.  Form 0 writes the bits of _v2 in every array.  The
 * sample records are fp32: a change below the fp32 spacing of the value (temperature: 3e-5 K at 300 K) arrives as 0 in the label.  The
 * epoch, batch-gradient and error-sum functions work in scaled label space and serve both forms as they are. */
int  mw_surrogate_prepare_form(int form, int n_in, long long n, const float *raw_in, const float *raw_out, const double *scl_in,
                               const double *scl_out, unsigned long long seed, long long n_train, long long n_val, float *train_x,
                               float *train_y, float *val_x, float *val_y, float *test_x, float *test_y, void *stream);
long long mw_surrogate_errors_workspace_bytes(int nsets);
int  mw_surrogate_errors(long long n, int nsets, const float *pred, const float *y, void *workspace, double *out, void *stream);
/* Weighted training: Keras' fit(sample_weight=...) under the default sum_over_batch_size reduction.  None of
 * these kernels inspects a weight: finite, non-negative and not all zero are the host's checks (surrogate_train.check_weights).  A NaN
 * weight gives NaN sums, which is what 0 * NaN gives anyway.
 * mw_surrogate_prepare_column: ONE fp32 value per sample, col (n,) DEVICE, through the pre-shuffle and split of mw_surrogate_prepare_form
 * with the same seed, n_train and n_val: col[perm[p]] goes to position p of [train_c | val_c | test_c], bits unchanged.  The trainer sends
 * the samples' weights through it, and the index of each sample's file (a float: exact below 2^24 files; not checked here). */
int  mw_surrogate_prepare_column(long long n, const float *col, unsigned long long seed, long long n_train, long long n_val, float *train_c,
                                 float *val_c, float *test_c, void *stream);
/* mw_surrogate_train_epoch_v2 with sample weights w (n,) fp32 DEVICE, laid out like a row of y (null: refused, the unweighted epoch is
 * _v2).  The loss of a batch of B samples is sum_i w_i mean_o((y_io - t_io)^2) / B -- the divisor is the batch size, not the sum of the
 * weights, and the weights are used as given.  stats (models, 2): sum w sum_o (y - t)^2 and sum w sum_o |y - t| over the epoch (Keras'
 * running `loss`, and mean_absolute_error as a weighted_metrics entry, = these / (4 n)).  With w = 1 the bits of _v2 in every output. */
int  mw_surrogate_train_epoch_w(int n_in, int models, const float *x, const float *y, const float *w, long long n, int batch, int epoch,
                                unsigned long long seed, float *params, float *m1, float *m2, const float *table, float beta1, float beta2,
                                float eps, double *stats, void *stream);
/* Test aid: mw_surrogate_batch_grad_v2 of the weighted batch routine, w (batch,) DEVICE: the gradient of the loss above, and
 * loss[0] = sum_i w_i sum_o r_io^2 / (4 batch). */
int  mw_surrogate_batch_grad_w(int n_in, const float *params, const float *x, const float *y, const float *w, int batch, float *grad,
                               float *loss, void *stream);
/* mw_surrogate_errors with sample weights w (n,) fp32 DEVICE shared by the sets: the same 24 numbers per set, the same reduction order
 * and workspace, every term of the four sums times (double)w_i, both maxima over the samples with w_i > 0 only (a sample of weight zero
 * does not exist for this call; no such sample at all: maxima 0).  With w = 1 the bits of mw_surrogate_errors; with the indicator of
 * a group of samples, the unweighted numbers of that group. */
int  mw_surrogate_errors_weighted(long long n, int nsets, const float *pred, const float *y, const float *w, void *workspace, double *out,
                                  void *stream);

/* ---- surrogate evaluation in the model loop ------------------------------------------------------------- */
/* A bank of `models` candidate networks of ONE width, scored against what the microphysics really did to a state: the four `Relative diff`
 * prints of microphysics_kessler_ponni.h:266-269 for many models at once, split by output field and by the active / inactive classes of
 * StatisticsGatherer::is_active (gather_micro_statistics.h:61-74), in one pass over the state per group of models and without writing
 * a prediction to memory.  The handle uploads the models' MFMA operand images and scaling tables once.
 * n_in 5 (single cell) or 9 (stencil); params HOST (models, 104 | 144) fp32 in the weights.txt order (W1, b1, W2, b2); scl_in HOST
 * (models, n_in, 2), scl_out HOST (models, 4, 2) fp64 [min,max] rows -- PER MODEL, so that models of different training runs can sit in
 * one bank.  1 <= models <= MW_SURROGATE_MAX_MODELS.  A scaling row with max == min is an error. */
typedef struct mw_surrogate_bank_s *mw_surrogate_bank_t;
int  mw_surrogate_bank_create(mw_surrogate_bank_t *b, int n_in, int models, const float *params, const double *scl_in,
                              const double *scl_out);
/* The same with an output form per model (MW_FORM_*): forms HOST (models), NULL = all MW_FORM_STATE, which is what
 * mw_surrogate_bank_create passes.  A bank may hold both forms, as it holds models with different scaling tables; mw_surrogate_eval,
 * mw_surrogate_members_apply and mw_surrogate_committee_apply then give, per model, the bits of mw_mlp_forward_form /
 * mw_mlp_stencil_forward_form with that model's form (a mixed committee's mean is still the mean of its models' outputs).  Any other
 * value is an error.  mw_surrogate_bank_form: model's form, -1 (and the error text) for a null handle or a model outside the bank. */
int  mw_surrogate_bank_create_forms(mw_surrogate_bank_t *b, int n_in, int models, const float *params, const double *scl_in,
                                    const double *scl_out, const int *forms);
int  mw_surrogate_bank_form(mw_surrogate_bank_t b, int model);
void mw_surrogate_bank_destroy(mw_surrogate_bank_t b);
/* G: the number of models the MFMA kernels evaluate per pass over the state (more models: ceil(models / G) passes in one launch). */
int  mw_surrogate_eval_group(mw_surrogate_bank_t b);
/* in5: HOST array of 5 DEVICE fp64 fields before the microphysics call (temp, density_dry, water_vapor, cloud_liquid, precip_liquid),
 * level-major (nz, ncol); truth4: the 4 fields after it (temp, water_vapor, cloud_liquid, precip_liquid).
 * out: DEVICE fp64 (models + 1, 2, 4, 4) = [model][class][field][statistic]: class 0 = inactive, 1 = active (any of the four
 * |after - before| > 1e-10); statistics sum d, sum |d|, sum d^2, max |d| of d = prediction - truth over the cells of the class.  Row
 * `models` is the persistence baseline (prediction = the input field).  counts: DEVICE int64 [2], the cells per class.
 * Model m's prediction is bit for bit what mw_mlp_forward / mw_mlp_stencil_forward write for its weights and scaling (mw_mlp_set_strict is
 * honoured); the reduction order is fixed and independent of the number of models and of a model's position in the bank.  Nothing is
 * written to in5 / truth4.  Asynchronous on `stream`; one call at a time per bank (the handle owns the partial sums' workspace, which
 * grows -- synchronising -- when a call needs more). */
int  mw_surrogate_eval(mw_surrogate_bank_t b, int nz, long long ncol, const double *const *in5, const double *const *truth4,
                       double *out, long long *counts, void *stream);
/* mw_surrogate_eval with every model's errors split by whether the cell lies INSIDE or OUTSIDE that model's training box:
 * how much of a model's one-step error comes from extrapolation.
 * mw_surrogate_bank_set_domain: box HOST (models, 5, 2) fp64 [lo, hi] per model and in5 field (mw_member_domain's layout and rule: lo <= hi,
 * NaN refused, +-inf allowed), uploaded into a table the handle owns; synchronises, as mw_surrogate_bank_create does; a later call
 * replaces the boxes.
 * A cell is outside for model m iff some tested value x fails lo <= x && x <= hi against m's row of x's field: NaN is outside, a value
 * equal to a bound is inside (-0.0 against lo = 0.0 too, +-inf against an infinite bound too).  Tested: the cell's five inputs and, for a
 * bank of width 9, temp, water_vapor, cloud_liquid and precip_liquid of the level above (at the top level the cell itself) against the
 * same rows.
 * mw_surrogate_eval_domain_group: the number of models whose predictions the MFMA kernels score per pass over the state.
 * mw_surrogate_eval_domain: in5, truth4, the classes and the statistics are mw_surrogate_eval's.  out: DEVICE fp64 (models, 2, 2, 2, 4, 4)
 * = [model][0 prediction | 1 persistence][0 inside | 1 outside][0 inactive | 1 active][field][statistic]; the persistence rows are per
 * model because the sides are.  counts: DEVICE int64 (models, 2, 2) = [model][side][class].  The tile walk and the reduction order are
 * mw_surrogate_eval's: with a box no cell leaves, a model's inside rows are that call's bits, and a model's rows depend neither on the
 * size of the bank, nor on its place in it, nor on the other models' boxes.  A class without cells holds +0.0; NaN reaches the sums and
 * the maximum of its own class alone.  mw_mlp_set_strict is honoured; nothing is written to in5 / truth4.  Asynchronous on `stream`; one
 * call at a time per bank (the handle's workspace grows as mw_surrogate_eval's does).  Refused with nothing launched and out / counts
 * untouched: a null pointer, nz or ncol below 1, a null field, a bank without boxes. */
int  mw_surrogate_bank_set_domain(mw_surrogate_bank_t b, const double *box);
int  mw_surrogate_eval_domain_group(mw_surrogate_bank_t b);
int  mw_surrogate_eval_domain(mw_surrogate_bank_t b, int nz, long long ncol, const double *const *in5, const double *const *truth4,
                              double *out, long long *counts, void *stream);

/* ---- surrogate rollout: candidate models as ensemble members beside Kessler ------------------------------ */
/* No reference counterpart (the reference runs one network per simulation, microphysics_kessler_ponni.h:273-276 un-commented).  The
 * coupler's arrays are member-fastest: cell c (level-major, c = k * ncol + col with ncol = ny * nx columns PER MEMBER), member e at
 * c * nens + e.  MW_ROLLOUT_MAX_MEMBERS: the most members the dycore steps in one call (its 64-lane x tiling). */
#define MW_ROLLOUT_MAX_MEMBERS 30
/* Member `member` of nf (<= MW_MAX_TRACERS) member-fastest DEVICE fp64 fields of n cells x nens members to / from contiguous arrays of n
 * doubles.  fields / out / in: HOST arrays of nf DEVICE pointers.  The rollout steps Kessler on member 0 ALONE with this pair:
 * mw_kessler_time_step takes its rain sub-cycle count from the minimum over all the columns it is given, so a candidate member with absurd
 * rain would change how the truth member is integrated. */
int  mw_member_extract(long long n, int nens, int member, int nf, const double *const *fields, double *const *out, void *stream);
int  mw_member_insert(long long n, int nens, int member, int nf, const double *const *in, double *const *fields, void *stream);
/* Model j of the bank replaces temp, water_vapor, cloud_liquid and precip_liquid of member members[j] IN PLACE with what mw_mlp_forward
 * (n_in 5) / mw_mlp_stencil_forward (n_in 9) would write for its weights from that member's own five fields before the call: the same
 * bits, mw_mlp_set_strict honoured.  fields5: HOST array of 5 DEVICE pointers (temp, density_dry, water_vapor, cloud_liquid,
 * precip_liquid), each (nz, ncol, nens); members: HOST array of the bank's `models` distinct member indices in [0, nens).  density_dry
 * and every member not listed are not written.  One launch for all models of the bank (at most 32): a 16-cell MFMA tile holds cells of
 * one member, the waves of a workgroup take consecutive models of the same cells.  The stencil model reads level k + 1 for level k: a
 * wave (strict: a thread) sweeps its columns top-down in one chunk and carries the level above in registers, so the result is the
 * out-of-place one and no workspace is needed.  Asynchronous on `stream`. */
int  mw_surrogate_members_apply(mw_surrogate_bank_t b, const int *members, int nz, long long ncol, int nens, double *const *fields5,
                                void *stream);
/* A COMMITTEE: the mean of n_sel (1 .. MW_COMMITTEE_MAX_MODELS) distinct models sel[0 .. n_sel) of one bank, and their spread, in one pass
 * over the state whatever n_sel is (the selected models sit in LDS once per workgroup: 16 x 2,080 B).  For every cell and output field,
 * y_j is bit for bit what mw_mlp_forward (n_in 5) / mw_mlp_stencil_forward (n_in 9) writes for model sel[j] -- per-model scaling and the
 * max(0, .) clamp of the three water fields included, mw_mlp_set_strict honoured -- and
 *   out   = (((y_0 + y_1) + y_2) + ...) / (double)n_sel      fp64, in the order of sel, no contraction, a true division
 *   range = hi - lo                                          hi / lo: the largest / smallest y_j, NaN if any y_j is
 * so a committee of one returns its model's own bits, and a NaN in any member makes both NaN at that cell and field alone.
 * in5: HOST array of 5 DEVICE pointers (temp, density_dry, water_vapor, cloud_liquid, precip_liquid); out4, range4 (optional: NULL):
 * HOST arrays of 4 DEVICE pointers (temp, water_vapor, cloud_liquid, precip_liquid); all member-fastest (nz, ncol, nens), and only the
 * elements of `member` are read and written (nens = 1, member = 0: plain contiguous fields).  out4[f] is either the matching input field
 * (in place) or overlaps no input; range4 overlaps nothing; anything else is refused.  The stencil kernels sweep a column top-down and
 * carry the level above raw in registers, so in place and out of place give the same bits without a workspace.  density_dry and the other
 * members are never written.  Asynchronous on `stream`. */
#define MW_COMMITTEE_MAX_MODELS 16
int  mw_surrogate_committee_apply(mw_surrogate_bank_t b, int n_sel, const int *sel, int member, int nz, long long ncol, int nens,
                                  const double *const *in5, double *const *out4, double *const *range4, void *stream);
/* Scores a committee on contiguous (nz, ncol) DEVICE fields: with d = pred4 - truth4 and r = range4, per class (0 inactive, 1 active, as
 * mw_surrogate_eval decides it from in5 and truth4) and field, out (DEVICE fp64 (2, 4, 7)) receives sum d, sum |d|, sum d^2, max |d|
 * (the statistics of an mw_surrogate_eval row), sum r, sum r^2, sum r |d|.  counts: DEVICE int64 [10] = the cells per class [2], then the
 * cells with |d| <= r per class and field (2, 4).  NaN reaches the sums and the maximum (and is never covered).  One fixed reduction
 * order, no floating-point atomics.  workspace: DEVICE, mw_committee_score_workspace_bytes(nz, ncol) bytes (0: arguments out of range).
 * Asynchronous on `stream`. */
long long mw_committee_score_workspace_bytes(int nz, long long ncol);
int  mw_committee_score(int nz, long long ncol, const double *const *in5, const double *const *truth4, const double *const *pred4,
                        const double *const *range4, void *workspace, double *out, long long *counts, void *stream);
/* How far every member has moved from member 0, and the member's own totals, for nf (<= MW_MAX_TRACERS) member-fastest DEVICE fp64 fields
 * of n cells x nens (<= 256) members.  fields: HOST array of nf DEVICE pointers.  out: DEVICE fp64 (nens, nf, 7) = sum d, sum |d|,
 * sum d^2, max |d| of d = member - member 0 over the cells, then sum x, min x, max x of the member itself; nonfinite: DEVICE int64
 * (nens, nf), the member's NaN or inf elements.  NaN reaches the sums AND the extrema.  Every element is loaded once; no floating-point
 * atomics, one fixed reduction order (run-to-run identical).  workspace: DEVICE, mw_member_divergence_workspace_bytes(n, nens, nf) bytes
 * (0: arguments out of range).  Asynchronous on `stream`. */
long long mw_member_divergence_workspace_bytes(long long n, int nens, int nf);
int  mw_member_divergence(long long n, int nens, int nf, const double *const *fields, void *workspace, double *out, long long *nonfinite,
                          void *stream);

/* ---- surface rain of every member from its column water budget -------------------------- */
/* The tracers are densities and in Kessler water leaves a column only through the ground, so what a microphysics step removes from a
 * column's water is that member's surface precipitation -- also for a member that a network steps, which emits no precl.
 * mw_member_column_water: w (DEVICE fp64 (ncol, nens)) of element t = col * nens + e is
 *   w[t] = dz * sum_{k = 0 .. nz-1} ((rho_v + rho_c) + rho_r)[(k * ncol + col) * nens + e]              kg / m^2
 * with exactly that association: k ascending in ONE fp64 accumulator that starts from +0.0, no contraction, dz applied once at the end,
 * no atomics -- a host loop over k reproduces the bits.  water3: HOST array of 3 DEVICE pointers (water_vapor, cloud_liquid,
 * precip_liquid), member-fastest (nz, ncol, nens), never written.  One thread per t walks the levels at stride ncol * nens, so the loads
 * are coalesced whatever nens is.  A NaN or inf of a cell reaches its own w[t] alone.
 * mw_member_surface_rain: the same sweep on the state AFTER the step, fused with the finish.  For a member e in `members`,
 *   precl[t] = (w_before[t] - W_after[t]) / (1000.0 * dt)                                                m of water / s
 * (1000: rhoqr of microphysics_kessler.h:247; the unit of Kessler's own precl).  The sign is kept: a step that creates water shows a
 * negative rate.  Then, for a member e in `accum` (any set; usually all members), rain_total[t] = rain_total[t] + dt * precl[t] with
 * whatever precl[t] holds NOW -- so a member in accum alone accumulates the precl another module wrote (Kessler's own, for the Kessler
 * member).  Elements of members in neither list are neither read nor written.  members / accum: HOST arrays of nm / na (0 .. nens)
 * distinct indices in [0, nens), nens <= 64; w_before, precl, rain_total: DEVICE fp64 (ncol, nens); w_before may be NULL when nm = 0,
 * rain_total when na = 0.  With a top level that holds rain the identity does not hold for Kessler itself (its top-cell formula, :294,
 * does not telescope).  Refused, with nothing launched: null pointers, nz or ncol < 1, nens outside [1, 64], members out of range or
 * repeated, dz or dt not positive and finite.  Both asynchronous on `stream`. */
int  mw_member_column_water(int nz, long long ncol, int nens, const double *const *water3, double dz, double *w, void *stream);
int  mw_member_surface_rain(int nz, long long ncol, int nens, int nm, const int *members, int na, const int *accum,
                            const double *const *water3, double dz, double dt, const double *w_before, double *precl, double *rain_total,
                            void *stream);
/* The water fixer: mw_member_surface_rain that also acts.  members, accum, w_before, precl, rain_total, dz, dt: as
 * above.  fixed: HOST array of nfix (0 .. nens) distinct members, every one of them in `members`.  For element t = col * nens + e of a
 * fixed member, with W_b = w_before[t] and W_a = mw_member_column_water of the state given (same order):
 *   W_a or W_b not finite, or W_a > W_b with W_b < 0:  SKIPPED -- counted, the state untouched, precl as mw_member_surface_rain's;
 *   W_b >= 0 and W_a - W_b > tolerance * W_b:           FIXED -- s = W_b / W_a (one fp64 division), every level's water_vapor,
 *     cloud_liquid and precip_liquid becomes q * s (one fp64 product each, no contraction, ordinary stores), W' is the column water of
 *     the STORED products in the same order (a later mw_member_column_water returns W' to the bit), precl[t] = (W_b - W') / (1000 dt),
 *     and the column's excess is W_a - W_b, kg / m^2;
 *   otherwise exactly mw_member_surface_rain's bits, and nothing of the state is written.
 * With non-negative fields and no underflow |W' - W_b| <= (nz + 4) * 2^-52 * W_b.  Only the three water fields are written: this is
 * a mass fixer, no latent heat is exchanged, temp and density_dry are not arguments.  water3: HOST array of 3 DEVICE pointers to three
 * different arrays.  counts: DEVICE int64 (nens, 2) = fixed columns, skipped columns of every member; stats: DEVICE fp64 (nens, 2) = sum and
 * maximum of the excess over the member's fixed columns (0 for a member not in `fixed`); both SET.  excess: NULL, or DEVICE fp64
 * (ncol, nens) that receives every element's excess, +0.0 where nothing was fixed (every member).  Reduction: a block of 256 consecutive
 * elements folds each member's lanes in ascending order; for each member thread l of 256 folds the blocks l, l + 256, ... in ascending
 * order, then the 256 results are folded in ascending l -- no atomics, no memset, run-to-run identical.  workspace: DEVICE,
 * mw_member_water_fix_workspace_bytes(ncol, nens) bytes (0: arguments out of range).  Refused, with nothing launched: what
 * mw_member_surface_rain refuses, a fixed member outside `members`, a tolerance that is negative or not finite, null workspace, counts
 * or stats.  Asynchronous on `stream`. */
long long mw_member_water_fix_workspace_bytes(long long ncol, int nens);
int  mw_member_water_fix(int nz, long long ncol, int nens, int nm, const int *members, int na, const int *accum, int nfix,
                         const int *fixed, double tolerance, double *const *water3, double dz, double dt, const double *w_before,
                         double *precl, double *rain_total, void *workspace, long long *counts, double *stats, double *excess,
                         void *stream);
/* The latent-heat closure.  In a Kessler step temp changes only by the vapour that condenses or evaporates in the cell,
 * so temp_after - temp_before = (lv / cp_d) * (rho_v_before - rho_v_after) / rho_d per cell; a network writes temp and water_vapor as two
 * unrelated outputs.  All fields DEVICE fp64, member-fastest (nz, ncol, nens).  members: HOST array of nm (0 .. nens) distinct DIAGNOSED
 * members; closed: HOST array of nclosed distinct members, every one of them in `members`.  Per cell i = (k * ncol + col) * nens + e of a
 * diagnosed member e, in fp64, no contraction, every operation rounded once:
 *   C   = lv / cp_d                                              (one division, on the host)
 *   T_c = temp_before[i] + C * ((rho_v_before[i] - rho_v[i]) / rho_d[i])
 *   r   = temp[i] - T_c                                          (the residual, K)
 *   r not finite (any of the five values NaN or inf, or rho_d == 0):  SKIPPED -- counted, temp untouched, left out of every sum;
 *   e in `closed` and |r| > tolerance (strict):                       CLOSED -- temp[i] = T_c, an ordinary store, counted;
 *   otherwise nothing is written.
 * Only temp is written, and only in closed members.  Statistics of every diagnosed member over its cells with finite r, r BEFORE closing:
 * counts: DEVICE int64 (nens, 2) = closed cells, skipped cells; stats: DEVICE fp64 (nens, 6) = sum r, sum |r|, sum r^2, max |r|, sum H,
 * max |H|, where H[t] = ((cp_d * dz) / dt) * (sum over k of rho_d * r), W / m^2, is the spurious heating of column t = col * nens + e (k
 * ascending in one accumulator from +0.0; the scale, made on the host, applied once); both SET, zeros for a member not diagnosed.  heating:
 * NULL, or DEVICE fp64 (ncol, nens) that receives H, +0.0 for members not diagnosed.  Order of the sums: a column's cells in ascending k from
 * +0.0; a block of 256 consecutive plane elements folds each member's lanes in ascending order from +0.0; for each member thread l of 256
 * folds the blocks l, l + 256, ... in ascending order from +0.0, then the 256 results are folded in ascending l -- no atomics, no memset,
 * run-to-run identical.  before2: HOST array of 2 DEVICE pointers, temp_before and rho_v_before, read only at elements of diagnosed members.
 * workspace: DEVICE, mw_member_heat_closure_workspace_bytes(ncol, nens) bytes (0: arguments out of range).  Refused, with nothing launched:
 * what mw_member_surface_rain refuses, a closed member outside `members`, a tolerance that is negative or not finite, lv or cp_d not
 * positive and finite, null workspace, counts or stats, temp equal to any of the four arrays that are only read.  Asynchronous on `stream`. */
long long mw_member_heat_closure_workspace_bytes(long long ncol, int nens);
int  mw_member_heat_closure(int nz, long long ncol, int nens, int nm, const int *members, int nclosed, const int *closed,
                            double tolerance, double lv, double cp_d, double dz, double dt,
                            double *temp, const double *rho_d, const double *rho_v,
                            const double *const *before2 /* temp_before, rho_v_before */,
                            void *workspace, long long *counts, double *stats, double *heating /* or NULL */, void *stream);
/* The contingency table of nf (1 .. 4) member-fastest DEVICE fp64 fields (ncol, nens) against member 0, the observation.  Field f has
 * nt[f] (1 .. 8) thresholds, finite and strictly ascending: thresholds is a HOST (nf, 8) fp64 array whose row f holds them first (the
 * rest is not read); nt: HOST.  An event is x >= thr.  counts: DEVICE int64 (nf, 8, nens, 5) = hits (member and member 0 both have the
 * event), misses (member 0 alone), false alarms (the member alone), correct negatives, non-finite -- a column where the member's or
 * member 0's value is NaN or inf (x - x != 0) counts as non-finite only, so the five sum to ncol for every field, threshold j < nt[f]
 * and member; rows j >= nt[f] are zeros.  Integer sums: any order gives the same numbers.  workspace: DEVICE,
 * mw_member_rain_table_workspace_bytes(ncol, nens, nf) bytes (0: arguments out of range; nens <= 64).  Asynchronous on `stream`. */
long long mw_member_rain_table_workspace_bytes(long long ncol, int nens, int nf);
int  mw_member_rain_table(long long ncol, int nens, int nf, const double *const *fields, const int *nt, const double *thresholds,
                          void *workspace, long long *counts, void *stream);

/* ---- harvesting Kessler labels on the rollout members' own states ---------------------------------------- */
/* The teacher: what Kessler would do to the state of the listed members, each member ALONE, out of place.  A member-fastest field
 * (nz, ncol, nens) is a (nz, ncol * nens) array of columns col * nens + e, so the production kernels' column walk is as coalesced on all
 * members at once as it is on one; every column lowers the rain sub-cycle count of its own member only (nens words in the workspace,
 * integer atomicMin on the bit pattern, no floating-point atomics).  fields5: HOST array of 5 DEVICE pointers (temp, density_dry,
 * water_vapor, cloud_liquid, precip_liquid), never written; out4: HOST array of 4 DEVICE pointers of the same (nz, ncol, nens) shape
 * that receive temp, water_vapor, cloud_liquid, precip_liquid after Kessler (densities) of the nm members in `members` (HOST, distinct,
 * in [0, nens), nens <= 64) -- for such a member the bits mw_kessler_time_step leaves when it is given that member's columns alone.
 * Elements of members not listed are NOT written; precl is not produced.  A member's count comes from one decision function
 * (mw_kessler_teacher_rainsplit below): a member whose state asks for more than max_rainsplit (1 .. 1024) sub-cycles, or whose rain
 * CFL step is not a positive finite number (a member with inf or NaN rain: 0), is SKIPPED: not computed, not written, count 0.  rainsplit_out: optional HOST
 * array of nm counts (0 = skipped; forces a stream synchronisation); without it the call is asynchronous on `stream` and may be repeated
 * on one workspace (DEVICE, mw_kessler_members_teacher_workspace_bytes bytes; 0: arguments out of range).
 * The production form only: mw_kessler_set_strict is not consulted (the labels end as fp32 samples). */
long long mw_kessler_members_teacher_workspace_bytes(int nz, long long ncol, int nens);
int  mw_kessler_members_teacher(int nz, long long ncol, int nens, int nm, const int *members, double dz, double dt, int max_rainsplit,
                                const double *const *fields5, double *const *out4, int *rainsplit_out, void *workspace, void *stream);
/* Host only: the teacher's decision function on a member's minimum rain CFL step dt_max -- ceil(dt / dt_max) if dt_max is finite,
 * > 0 and the quotient is in [1, cap], else 0.  Decided in floating point before any conversion to int. */
int  mw_kessler_teacher_rainsplit(double dt, double dt_max, int cap);

/* ---- guarded committee: Kessler takes the columns where the committee's models disagree ------------------ */
/* Three passes that, between an out-of-place mw_surrogate_committee_apply and the state, make the member "the committee's mean where its
 * models agree, Kessler where they do not" (DESIGN.md 13.7).  All member-fastest (nz, ncol, nens), all asynchronous on `stream`.
 * mw_committee_guard_flags: column col of `member` is flagged iff, at some level k and for some field f of temp, water_vapor,
 * cloud_liquid, precip_liquid, !(range4[f] <= thr4[f]) or mean4[f] is not finite -- so a NaN range flags, a range EQUAL to its threshold
 * does not, and thr4[f] = +inf means that field never flags by size.  mean4 / range4: HOST arrays of 4 DEVICE pointers (what
 * committee_apply wrote); thr4: HOST, 4 thresholds >= 0 (negative or NaN: refused).  flags: DEVICE bytes (ncol, nens), byte
 * col * nens + member receives 0 or 1 for every column of `member`, no other byte is touched.  counts: DEVICE int64 [2]; [0] is SET to
 * this call's number of flagged columns, [1] is INCREASED by it (integer atomics: run-to-run identical).  One pass over the member's
 * 64 bytes per cell. */
int  mw_committee_guard_flags(int nz, long long ncol, int nens, int member, const double *const *mean4, const double *const *range4,
                              const double *thr4, unsigned char *flags, long long *counts, void *stream);
/* mw_kessler_members_teacher with "column col * nens + e takes part iff flags[col * nens + e] != 0" in place of the member list: for
 * the flagged columns F of a member, in ascending order, out4 receives the bits mw_kessler_time_step leaves when it is given those
 * columns alone as contiguous (nz, |F|) fields -- the rain sub-cycle count is the minimum over F only, decided by
 * mw_kessler_teacher_rainsplit.  A member whose count is 0 (more than max_rainsplit sub-cycles, or inf / NaN rain or fall speed in a
 * FLAGGED column) is skipped: nothing of it is written.  Elements of unflagged columns of out4 are never written; fields5 is never
 * written; precl is not produced.  rainsplit_out: optional HOST array of nens counts (a member without a flagged column: 1; forces a
 * stream synchronisation).  The same workspace layout, start-of-call memset and repeatability as the members teacher.  A wavefront
 * without a flagged lane leaves after one byte load per lane. */
long long mw_kessler_columns_teacher_workspace_bytes(int nz, long long ncol, int nens);
int  mw_kessler_columns_teacher(int nz, long long ncol, int nens, const unsigned char *flags, double dz, double dt, int max_rainsplit,
                                const double *const *fields5, double *const *out4, int *rainsplit_out, void *workspace, void *stream);
/* dst[f][c * nens + e] = src[f][c * nens + e] for the n cells c, the nm members e in `members` (HOST, distinct, nens <= 64) and the nf
 * (<= MW_MAX_TRACERS) fields: the commit of a scratch result into the state.  Elements of other members are not touched. */
int  mw_members_copy(long long n, int nens, int nm, const int *members, int nf, const double *const *src, double *const *dst, void *stream);
/* DataGenerator's sampler on the member layout, between the listed members' own fields5 and their teacher values teacher4 (as above).
 * mw_member_sample_mask: mask (DEVICE bytes, (nz, ncol, nens)) of element t = (k * ncol + col) * nens + e is 1 if e is listed,
 * u01(key0 + t) < (active ? thr_active : thr_inactive) with u01 and `active` as mw_micro_sample_mask has them (any of the four
 * |teacher - input| > 1e-10), and all fourteen values of the element's sample record are finite AS fp32 (a trainer refuses a file that
 * holds one that is not); 0 otherwise, and 0 for every member not listed.
 * mw_member_gather_samples: mw_micro_gather_samples' records -- inputs (n, 5, 2), outputs (n, 4), DEVICE fp32 -- for the n flat element
 * indices `elems` (DEVICE int64) into the member layout; the level above is min(nz - 1, k + 1) of the same column and member, slot (4, 1)
 * is 0.  An index outside the fields gives a record of zeros.  Both asynchronous on `stream`. */
int  mw_member_sample_mask(int nz, long long ncol, int nens, int nm, const int *members, const double *const *fields5,
                           const double *const *teacher4, unsigned long long key0, double thr_active, double thr_inactive,
                           unsigned char *mask, void *stream);
int  mw_member_gather_samples(int nz, long long ncol, int nens, const double *const *fields5, const double *const *teacher4,
                              const long long *elems, long long n, float *inputs, float *outputs, void *stream);

/* ---- training-domain guard: which cells of a member lie outside the box its model was trained in --------- */
/* One read of the five input fields in5 (temp, density_dry, water_vapor, cloud_liquid, precip_liquid: HOST array of 5 DEVICE pointers,
 * member-fastest (nz, ncol, nens), never written) of the nm (1 .. 32) listed members (HOST, distinct, in [0, nens), nens <= 64)
 * against box, a HOST (nm, 5, 2) fp64 array of [lo, hi] per listed member and field (lo <= hi; NaN refused, +-inf allowed; it travels in
 * the kernel arguments, hence nm <= 32).  A value x of field f is BELOW iff x < lo, ABOVE iff x > hi, NAN iff x != x, else inside: x
 * equal to a bound, +-inf against an infinite bound and -0.0 against lo = 0.0 are inside.  A column of a member is OUTSIDE iff some
 * level and field of it holds a below, above or nan value.
 * counts: DEVICE int64 (nm, 16), SET by the call (a memset in stream order, then integer adds): word 3 f + c the cells of field f in
 * class c (0 below, 1 above, 2 nan), word 15 the member's outside columns.
 * flags / slots / flag_counts: all three may be NULL (report only).  slots: HOST, nm entries; for a member with slots[j] >= 0 the byte
 * col * nens + member of flags (DEVICE, (ncol, nens)) becomes 1 for every outside column and is never set to 0, and
 * flag_counts[2 slots[j]] and [2 slots[j] + 1] (DEVICE int64, the layout of mw_committee_guard_flags' counts, one pair per slot) are
 * both INCREASED by the number of that member's bytes this call turned from 0 to 1 -- so after mw_committee_guard_flags on the same
 * member the pair holds the union.  Bytes of unlisted members and of members with slots[j] < 0 are not touched.
 * Asynchronous on `stream`, no allocation, no host synchronisation, integer atomics only: every result is independent of order and
 * run-to-run identical.  Refused, with nothing launched: null in5, counts, box or members; nz or ncol < 1; nens outside [1, 64]; nm
 * outside [1, 32]; a repeated or out-of-range member; a bad box; a slots[j] >= 0 with flags or flag_counts NULL.  40 bytes per cell of
 * the listed members. */
int  mw_member_domain(int nz, long long ncol, int nens, int nm, const int *members, const double *box, const double *const *in5,
                      long long *counts, unsigned char *flags, const int *slots, long long *flag_counts, void *stream);

/* ---- harvest outside the training box: the member sampler with a third class --------------------------- */
/* mw_member_sample_mask with the classes OUTSIDE, ACTIVE, INACTIVE, element t = (k * ncol + col) * nens + e as there.
 * members: HOST, nm (1 .. 32) distinct members in [0, nens), nens <= 64.  box: HOST (nm, 5, 2) fp64 [lo, hi] per listed member and
 * fields5 field (mw_member_domain's layout and rule: lo <= hi, NaN refused, +-inf allowed).  above: HOST, nm ints; non-zero: the
 * member's model reads the level above (a stencil model), and the four values of that level are tested too.  thr: HOST (nm, 3) fp64 in
 * [0, 1], the rates of the classes outside, active, inactive.  Box, thresholds and bits travel in the kernel arguments (3.5 KB).
 * An element of listed member members[j] is ELIGIBLE iff all fourteen values of its sample record -- the five inputs at t, the four of
 * temp, water_vapor, cloud_liquid, precip_liquid at `up` (t + ncol * nens, or t itself at the top level), the four teacher values -- are
 * finite AS fp32 (mw_member_sample_mask's test).  An eligible element is OUTSIDE iff some fields5[f][t] is < lo or > hi of box[j][f],
 * or, with above[j], some fields5[f][up], f in {0, 2, 3, 4}, against the same row (a value equal to a bound and -0.0 against lo = 0.0
 * are inside); otherwise ACTIVE iff any of the four |teacher - input| > 1e-10, else INACTIVE.
 * counts: DEVICE int64 (nm, 6), SET by the call (a memset in stream order, then integer adds): the eligible elements outside, active,
 * inactive, then the taken ones in the same order.  An element is taken iff it is eligible and u01(key0 + t) < thr[j][class].
 * mask: DEVICE bytes (nz, ncol, nens), 1 for a taken element, 0 for every other, unlisted members included; NULL: count only, nothing
 * but counts is written.
 * Asynchronous on `stream`, no allocation, no host synchronisation, integer atomics only: every result is independent of order and
 * run-to-run identical.  Refused, with nothing launched and nothing written: mw_member_sample_mask's refusals (mask apart), a bad box,
 * a threshold that is NaN or outside [0, 1], counts NULL.  13 eight-byte loads per element of the listed members. */
int  mw_member_sample_mask_domain(int nz, long long ncol, int nens, int nm, const int *members, const double *box, const int *above,
                                  const double *const *fields5, const double *const *teacher4, unsigned long long key0, const double *thr,
                                  unsigned char *mask, long long *counts, void *stream);

/* ---- DataManager validators ---------------------------------------------------------------------------- */
/* core::DataManager::validate / validate_nan / validate_inf / validate_pos (model/core/DataManager.h:385-483) -- the reference's only
 * built-in health check: it copies an entry to the host and loops over it.  Here ONE device pass over the entry's `n` elements
 * (DEVICE pointer): out6[0..2] = number of NaN / inf / negative elements, out6[3..5] = the lowest flat ("global") index of each
 * kind, i.e. the first one the reference's loop reports, or -1.  The caller decides which of the three apply (negative values only
 * matter for entries registered `positive`, :469) and whether to die (die_on_failed_check).  Synchronises the stream. */
int  mw_validate_f64(const double *field, long long n, long long *out6, void *stream);
int  mw_validate_f32(const float *field, long long n, long long *out6, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MW_CDNA4_H */
