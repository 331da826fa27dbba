// =====================================================================================================
// mw_dycore_aids.hip -- calibration launchers (kernels: mw_calib.h) and test aids.  Nothing here runs in a time step.
// (unit map and the one-definition rule: mw_dycore_int.h)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include "mw_march.h"
#include "mw_calib.h"      // calibration kernels: fp64 FMA ceiling, the arithmetic floor of a stage (WENO + Riemann on registers)

namespace mw {

// Diagnostic: the device WENO-5 routines on caller-supplied stencils (unit test of the core arithmetic against the golden vectors)
__global__ __launch_bounds__(256) void k_weno5_edges(const double *__restrict__ st, double *__restrict__ out, long long n, int strict) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const double *s = st + t * 5;
  double l, r;
  if (strict) weno5_edges_strict(s[0], s[1], s[2], s[3], s[4], l, r);
  else        weno5_edges_fast(s[0], s[1], s[2], s[3], s[4], l, r);
  out[t * 2] = l; out[t * 2 + 1] = r;
}

// Diagnostic: the strict path's pow (mw_glibc_pow.h) on caller-supplied arguments; main[i] = 1 where the restated main path applied
__global__ __launch_bounds__(256) void k_strict_pow(const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ out,
                                                    unsigned char *__restrict__ main_path, long long n) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  double r;
  const bool m = glibc_pow_main(x[t], y[t], &r);
  out[t] = m ? r : pow(x[t], y[t]);
  if (main_path) main_path[t] = m ? 1 : 0;
}

} // namespace mw

extern "C" {

int mw_weno5_edges(long long n, const double *stencils, double *edges, int strict, void *stream) {
  if (n < 1 || !stencils || !edges) MW_FAIL("weno5_edges: bad argument");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  MW_KLAUNCH(k_weno5_edges, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stencils, edges, n, strict);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_strict_pow(long long n, const double *x, const double *y, double *out, unsigned char *main_path, void *stream) {
  if (n < 1 || !x || !y || !out) MW_FAIL("strict_pow: bad argument");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  MW_KLAUNCH(k_strict_pow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, out, main_path, n);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_calib_copy(const double *in, double *out, long long n, void *stream) {
  if (!in || !out || n < 1) MW_FAIL("mw_calib_copy: bad arguments");
  MW_KLAUNCH(k_calib_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n);
  MW_LAUNCH_CHECK();
  return 0;
}

// ---- calibration (mw_calib.h) --------------------------------------------------------------------------------------------
// Sustained v_fma_f64 issue rate with `waves_per_simd` wavefronts per SIMD on every CU, for about `seconds` (a short run sizes the
// long one).  out5 (HOST): wave-instructions per second, kernel milliseconds, shader clock in GHz during the run (the kernel's cycle
// counter over its 100 MHz real-time counter; 0 when the two counters run at the same rate on this part), wave-instructions issued, CUs.
int mw_calib_fma64(int waves_per_simd, double seconds, double *out5, void *stream) {
  if (waves_per_simd < 1 || waves_per_simd > 8 || !(seconds > 0) || seconds > 20 || !out5) MW_FAIL("mw_calib_fma64: waves_per_simd in 1..8, seconds in (0, 20]");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const int cus = device_cus();
  if (cus < 1) MW_FAIL("mw_calib_fma64: cannot read the device's CU count");
  double *sink = nullptr; long long *clk = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
  MW_HIP(hipMalloc(&sink, 8)); MW_HIP(hipMalloc(&clk, 16));
  MW_HIP(hipEventCreate(&e0)); MW_HIP(hipEventCreate(&e1));
  const dim3 grid((unsigned)(cus * waves_per_simd));            // 256 threads = one wave per SIMD; waves_per_simd workgroups per CU
  auto run = [&](long long trips, float &ms) -> int {
    MW_HIP(hipEventRecord(e0, st));
    MW_KLAUNCH(k_calib_fma64, grid, dim3(256), 0, st, trips, 1.0, sink, clk);
    MW_LAUNCH_CHECK();
    MW_HIP(hipEventRecord(e1, st));
    MW_HIP(hipEventSynchronize(e1));
    MW_HIP(hipEventElapsedTime(&ms, e0, e1));
    return 0;
  };
  float ms = 0;
  long long trips = 20000;
  int rc = run(trips, ms) || run(trips, ms);                     // (the first launch also loads the code object)
  if (!rc) { trips = std::max(1000ll, (long long)(trips * (seconds * 1e3 / std::max(1e-3f, ms)))); rc = run(trips, ms); }
  long long h[2] = {0, 0};
  if (!rc && hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost) != hipSuccess) { set_error("mw_calib_fma64: download failed"); rc = 1; }
  (void)hipFree(sink); (void)hipFree(clk); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (rc) return 1;
  const double winstr = (double)trips * 64.0 * (double)grid.x * 4.0;
  out5[0] = winstr / (ms * 1e-3); out5[1] = ms;
  out5[2] = (h[1] > 0 && h[0] != h[1]) ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
  out5[3] = winstr; out5[4] = cus;
  return 0;
}

// The arithmetic floor of one RK stage: `cells` cell-stages (24 reconstructions + 3 Riemann solves + the passive fluxes each, the
// production arithmetic of mw_weno.h / mw_march.h) on register windows fed from `tab` -- DEVICE (nlev, 8, 64) doubles, a few KB that
// stay in L2 -- in workgroups of 256 threads, two per CU, `levels` cells per thread (k_xz_state's shape).  bg4 (HOST): hyr, hyt, p0,
// 1/hyt of the level.  sink: DEVICE, one double per thread (mw_calib_stage_arith_threads).  out3 (HOST): milliseconds, cells processed,
// workgroups.  The table decides smooth or rough data; the time is what a stage of that many cells cannot beat on this chip.
long long mw_calib_stage_arith_threads(long long cells, int levels) {
  if (cells < 1 || levels < 1) return 0;
  const long long thr = (cells + levels - 1) / levels;
  return ((thr + 255) / 256) * 256;
}
int mw_calib_stage_arith(const double *tab, int nlev, long long cells, int levels, int active_tracers, const double *bg4, double *sink, double *out3, void *stream) {
  if (!tab || nlev < 6 || cells < 1 || levels < 1 || !bg4 || !sink || !out3) MW_FAIL("mw_calib_stage_arith: bad argument (nlev >= 6)");
  if (active_tracers != 1 && active_tracers != 3) MW_FAIL("mw_calib_stage_arith: active_tracers must be 3 (24 reconstructions per cell) or 1 (cloud and rain zero: 18)");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long thr = mw_calib_stage_arith_threads(cells, levels);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MW_HIP(hipEventCreate(&e0)); MW_HIP(hipEventCreate(&e1));
  float ms = 0; int rc = 0;
  for (int rep = 0; rep < 2 && !rc; rep++) {                     // (the second launch is the measurement)
    if (hipEventRecord(e0, st) != hipSuccess) rc = 1;
    if (active_tracers == 3) MW_KLAUNCH((k_calib_stage_arith<8>), dim3((unsigned)(thr / 256)), dim3(256), 0, st, tab, nlev, levels, bg4[0], bg4[1], bg4[2], bg4[3], sink);
    else                     MW_KLAUNCH((k_calib_stage_arith<6>), dim3((unsigned)(thr / 256)), dim3(256), 0, st, tab, nlev, levels, bg4[0], bg4[1], bg4[2], bg4[3], sink);
    if (hipGetLastError() != hipSuccess || hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
        hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = 1;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (rc) MW_FAIL("mw_calib_stage_arith: launch or timing failed");
  out3[0] = ms; out3[1] = (double)(thr * levels); out3[2] = (double)(thr / 256);
  return 0;
}
// Test aid: occupies `stream` for about `usec` microseconds (one wavefront polling the 100 MHz counter).
int mw_debug_spin(long long usec, void *stream) { return launch_spin(usec, (hipStream_t)stream); }

} // extern "C"
