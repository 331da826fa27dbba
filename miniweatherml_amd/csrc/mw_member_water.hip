// =====================================================================================================
// mw_member_water.hip -- every member's column water budget (no reference counterpart).  mw_member_column_water is the budget before
// the step, mw_member_surface_rain the finish after it: a listed member's precl is what the step took out of its column
// (DESIGN.md 13.8).  mw_member_water_fix is mw_member_surface_rain that also acts: a listed member's column that holds more water than
// before the step is scaled back to what it held, and the step's precl is the budget of the state left behind (13.15).
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_member.h"

namespace mw {

struct WaterFields { const double *v, *c, *r; };
struct FixFields { double *v, *c, *r; };
constexpr int WATER_AHEAD = 4;             // levels whose loads are issued ahead of their adds

// dz * sum over k of ((v + c) + r)[k * plane + t]: one fp64 accumulator from +0.0, k ascending, no contraction.  Thread t is one (column,
// member) of the plane, so a wavefront's loads of a level are 64 consecutive doubles per field whatever nens is.  The twelve loads of
// WATER_AHEAD levels are issued before the first add; the adds keep the order of k.
// SCALE: every value times s first, twelve ordinary stores, and the stored products are what is summed.
template <bool SCALE, class Fields>
__device__ __forceinline__ double column_walk(int nz, long long plane, long long t, const Fields &F, double s, double dz) {
#pragma clang fp contract(off)
  double acc = 0.0;
  int k = 0;
  for (; k + WATER_AHEAD <= nz; k += WATER_AHEAD) {
    double v[WATER_AHEAD], c[WATER_AHEAD], r[WATER_AHEAD];
#pragma unroll
    for (int j = 0; j < WATER_AHEAD; j++) {
      const long long i = (long long)(k + j) * plane + t;
      v[j] = F.v[i]; c[j] = F.c[i]; r[j] = F.r[i];
    }
#pragma unroll
    for (int j = 0; j < WATER_AHEAD; j++) {
      if constexpr (SCALE) {
        const long long i = (long long)(k + j) * plane + t;
        v[j] = v[j] * s; c[j] = c[j] * s; r[j] = r[j] * s;
        F.v[i] = v[j]; F.c[i] = c[j]; F.r[i] = r[j];
      }
      acc = acc + ((v[j] + c[j]) + r[j]);
    }
  }
  for (; k < nz; k++) {
    const long long i = (long long)k * plane + t;
    double v = F.v[i], c = F.c[i], r = F.r[i];
    if constexpr (SCALE) {
      v = v * s; c = c * s; r = r * s;
      F.v[i] = v; F.c[i] = c; F.r[i] = r;
    }
    acc = acc + ((v + c) + r);
  }
  return dz * acc;
}

__device__ __forceinline__ double column_water(int nz, long long plane, long long t, const WaterFields &F, double dz) {
  return column_walk<false>(nz, plane, t, F, 1.0, dz);
}

// the walk that scales the column by s: column_water of the state left behind returns this to the bit
__device__ __forceinline__ double column_water_scale(int nz, long long plane, long long t, const FixFields &F, double s, double dz) {
  return column_walk<true>(nz, plane, t, F, s, dz);
}

// The finish of element t: a listed member's (`mine`) precl is what the step took out of its column, signed; a member of `accum`
// (`sums`) adds dt * (whatever precl holds now) to its total.  per_rate = 1000.0 * dt: kg / m^2 to m of water per second.
__device__ __forceinline__ void member_rain_finish(bool mine, bool sums, long long t, double w_before, double w_after, double per_rate, double dt,
                                                   double *__restrict__ precl, double *__restrict__ rain_total) {
#pragma clang fp contract(off)
  double p;
  if (mine) {
    p = (w_before - w_after) / per_rate;
    precl[t] = p;
  } else {
    p = precl[t];
  }
  if (sums) rain_total[t] = rain_total[t] + dt * p;
}

__global__ __launch_bounds__(256) void k_member_column_water(int nz, long long plane, WaterFields F, double dz, double *__restrict__ w) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < plane) w[t] = column_water(nz, plane, t, F, dz);
}

// The same sweep on the state after the step, and the finish.  Elements of members in neither set are not read or written.
__global__ __launch_bounds__(256) void k_member_surface_rain(int nz, long long plane, int nens, unsigned long long listed, unsigned long long accum,
                                                             WaterFields F, double dz, double dt, double per_rate,
                                                             const double *__restrict__ w_before, double *__restrict__ precl,
                                                             double *__restrict__ rain_total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= plane) return;
  const int e = (int)(t % nens);
  const bool mine = (listed >> e) & 1ull, sums = (accum >> e) & 1ull;
  if (!mine && !sums) return;
  double wb = 0.0, wa = 0.0;
  if (mine) { wb = w_before[t]; wa = column_water(nz, plane, t, F, dz); }
  member_rain_finish(mine, sums, t, wb, wa, per_rate, dt, precl, rain_total);
}

// ---- mw_member_water_fix ------------------------------------------------------------------------------------------------------------
constexpr int FIX_COUNTS = 2, FIX_STATS = 2;   // per block and member: fixed columns, skipped columns (int64 bits), sum of excess, max of excess
constexpr unsigned FIX_MAX = 1u << 1;      // (statistic 1 is a maximum)
constexpr int FIX_FIXED = 1, FIX_SKIPPED = 2;

// k_member_surface_rain with the remedy.  Thread t is one (column, member) of the plane and first sweeps its column as
// column_water does.  A member of `fixed` whose column holds more water than before the step (W_a - W_b > tolerance * W_b, W_b >= 0)
// sweeps it a second time with s = W_b / W_a (column_water_scale).  The second sweep is behind a ballot: a wavefront with no column to
// fix does not enter it.  Statistics: every lane's flag and excess go to LDS, and the block's rows and k_member_rows_final follow
// (mw_member.h); a block with nothing fixed or skipped writes rows of zeros.
__global__ __launch_bounds__(256) void k_member_water_fix(int nz, long long plane, int nens, unsigned long long listed, unsigned long long accum,
                                                          unsigned long long fixed, double tolerance, FixFields F, double dz, double dt,
                                                          double per_rate, const double *__restrict__ w_before, double *__restrict__ precl,
                                                          double *__restrict__ rain_total, double *__restrict__ partial,
                                                          double *__restrict__ excess) {
#pragma clang fp contract(off)
  __shared__ double ex[256];
  __shared__ int what[256];
  const int l = threadIdx.x;
  const long long t = (long long)blockIdx.x * 256 + l;
  const int e = (int)(t % nens);
  const bool in = t < plane;
  const bool mine = in && ((listed >> e) & 1ull), sums = in && ((accum >> e) & 1ull);
  double wb = 0.0, wa = 0.0, over = 0.0;
  int flag = 0;
  if (mine) {
    const WaterFields R = {F.v, F.c, F.r};
    wb = w_before[t];
    wa = column_water(nz, plane, t, R, dz);
    if ((fixed >> e) & 1ull) {
      const double d = wa - wb;
      if (wa - wa != 0.0 || wb - wb != 0.0) flag = FIX_SKIPPED;                // NaN or inf: the budget's own bits show it
      else if (wa > wb && wb < 0.0) flag = FIX_SKIPPED;                        // no scale of a negative total is a remedy
      else if (wb >= 0.0 && d > tolerance * wb) { flag = FIX_FIXED; over = d; }
    }
  }
  if (__ballot(flag == FIX_FIXED)) {                                          // wavefront-uniform: only a wavefront with a column to fix sweeps again
    if (flag == FIX_FIXED) wa = column_water_scale(nz, plane, t, F, wb / wa, dz);      // W': what column_water now returns for this column
  }
  if (mine || sums) member_rain_finish(mine, sums, t, wb, wa, per_rate, dt, precl, rain_total);
  if (excess && in) excess[t] = over;
  ex[l] = over;
  what[l] = flag;
  member_rows_fold<FIX_COUNTS, FIX_STATS, FIX_MAX>(nens, flag, partial, [&](int j, int s) { return what[j] == s + 1 ? 1 : 0; },
                                                   [&](int j, int) { return ex[j]; });
}

static int water_fields(const char *who, int nz, long long ncol, int nens, const double *const *water3, double dz, WaterFields *F) {
  if (!water3) MW_FAIL(std::string(who) + ": null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL(std::string(who) + ": nz and ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL(std::string(who) + ": nens must be in [1, 64]");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18) MW_FAIL(std::string(who) + ": the fields are too large");
  if (!positive_finite(dz)) MW_FAIL(std::string(who) + ": dz must be positive and finite");
  for (int f = 0; f < 3; f++) if (!water3[f]) MW_FAIL(std::string(who) + ": null field");
  F->v = water3[0]; F->c = water3[1]; F->r = water3[2];
  return 0;
}

} // namespace mw

using namespace mw;

extern "C" int mw_member_column_water(int nz, long long ncol, int nens, const double *const *water3, double dz, double *w, void *stream) {
  WaterFields F;
  if (water_fields("member_column_water", nz, ncol, nens, water3, dz, &F)) return 1;
  if (!w) MW_FAIL("member_column_water: null pointer");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long plane = ncol * nens;
  hipLaunchKernelGGL(k_member_column_water, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nz, plane, F, dz, w);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_member_surface_rain(int nz, long long ncol, int nens, int nm, const int *members, int na, const int *accum,
                                      const double *const *water3, double dz, double dt, const double *w_before, double *precl,
                                      double *rain_total, void *stream) {
  WaterFields F;
  if (water_fields("member_surface_rain", nz, ncol, nens, water3, dz, &F)) return 1;
  if (!positive_finite(dt)) MW_FAIL("member_surface_rain: dt must be positive and finite");
  unsigned long long listed = 0, sums = 0;
  if (member_bits("member_surface_rain", "members", nens, nm, members, &listed)) return 1;
  if (member_bits("member_surface_rain", "accum", nens, na, accum, &sums)) return 1;
  if (!precl || (nm > 0 && !w_before) || (na > 0 && !rain_total)) MW_FAIL("member_surface_rain: null pointer");
  if (nm == 0 && na == 0) return 0;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long plane = ncol * nens;
  hipLaunchKernelGGL(k_member_surface_rain, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nz, plane, nens, listed, sums, F,
                     dz, dt, 1000.0 * dt, w_before, precl, rain_total);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" long long mw_member_water_fix_workspace_bytes(long long ncol, int nens) {
  if (ncol < 1 || nens < 1 || nens > 64 || !member_counts_fit((double)ncol * (double)nens, 256.0)) return 0;
  return member_plane_blocks(ncol, nens) * nens * (FIX_COUNTS + FIX_STATS) * 8;
}

extern "C" int mw_member_water_fix(int nz, long long ncol, int nens, int nm, const int *members, int na, const int *accum, int nfix,
                                   const int *fixed, double tolerance, double *const *water3, double dz, double dt, const double *w_before,
                                   double *precl, double *rain_total, void *workspace, long long *counts, double *stats, double *excess,
                                   void *stream) {
  const char *who = "member_water_fix";
  WaterFields R;
  if (water_fields(who, nz, ncol, nens, water3, dz, &R)) return 1;
  if (!positive_finite(dt)) MW_FAIL("member_water_fix: dt must be positive and finite");
  if (!finite_nonnegative(tolerance)) MW_FAIL("member_water_fix: tolerance must be finite and >= 0");
  unsigned long long listed = 0, sums = 0, fix = 0;
  if (member_bits(who, "members", nens, nm, members, &listed)) return 1;
  if (member_bits(who, "accum", nens, na, accum, &sums)) return 1;
  if (member_bits(who, "fixed", nens, nfix, fixed, &fix)) return 1;
  if (member_subset(who, "fixed", "members", fix, listed, nens)) return 1;
  if (!precl || (nm > 0 && !w_before) || (na > 0 && !rain_total) || !workspace || !counts || !stats) MW_FAIL("member_water_fix: null pointer");
  if (water3[0] == water3[1] || water3[0] == water3[2] || water3[1] == water3[2]) MW_FAIL("member_water_fix: the three water fields must be three arrays");
  if (member_plane_limit(who, ncol, nens)) return 1;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const FixFields F = {water3[0], water3[1], water3[2]};
  hipStream_t st = (hipStream_t)stream;
  const long long plane = ncol * nens, blocks = member_plane_blocks(ncol, nens);
  hipLaunchKernelGGL(k_member_water_fix, dim3((unsigned)blocks), dim3(256), 0, st, nz, plane, nens, listed, sums, fix, tolerance, F, dz, dt,
                     1000.0 * dt, w_before, precl, rain_total, (double *)workspace, excess);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_member_rows_final<FIX_COUNTS, FIX_STATS, FIX_MAX>), dim3((unsigned)nens), dim3(256), 0, st, blocks, nens,
                     (const double *)workspace, counts, stats);
  MW_LAUNCH_CHECK();
  return 0;
}
