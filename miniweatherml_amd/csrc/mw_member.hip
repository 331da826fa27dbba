// =====================================================================================================
// mw_member.hip -- passes over the coupler's member-fastest arrays (cell c, ensemble member e at c * nens + e) that treat the members
// differently: one member out to contiguous arrays and back (mw_member_extract / mw_member_insert: the rollout's Kessler member is stepped
// alone), and how far every member has moved from member 0 (mw_member_divergence).  No reference counterpart: the reference's ensemble
// members never meet.  mw_member_sample_mask / mw_member_gather_samples are DataGenerator's sampler (k_sample_mask / k_gather_samples of
// mw_output.hip, which see member 0 only) on the member layout, between a member's own state and its Kessler teacher values.
// mw_committee_guard_flags / mw_members_copy are the guarded committee's two passes that are not Kessler's: which columns
// of a member go to Kessler, and the commit of the scratch result into the state.  mw_member_column_water / mw_member_surface_rain /
// mw_member_rain_table are every member's surface rain from its column water budget and its contingency table.
// mw_member_domain counts the cells of the listed members that lie outside the box their models were trained in, and flags their columns
// for the guarded committee's Kessler pass.  mw_member_sample_mask_domain is the member sampler with a third class, the
// cells outside the member's box, and the counts of every class that fix its rate.  mw_member_water_fix is
// mw_member_surface_rain that also acts: a listed member's column that holds more water than before the step is scaled back to what it
// held, and the step's precl is the budget of the state left behind.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_common.h"
#include "mw_sample_key.h"
#include <algorithm>
#include <string>

namespace mw {

struct MemberFields { double *f[MW_MAX_TRACERS]; };

// thread = cell, grid row y = field: member `e` of the fused array <-> element i of the contiguous one
template <bool INSERT>
__global__ __launch_bounds__(256) void k_member_copy(long long n, int nens, int e, MemberFields fused, MemberFields flat) {
  double *a = fused.f[blockIdx.y], *b = flat.f[blockIdx.y];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if (INSERT) a[i * nens + e] = b[i];
    else b[i] = a[i * nens + e];
  }
}

// ---- mw_member_divergence -----------------------------------------------------------------------------------------------------------
constexpr int DIV_STATS = 7;               // sum d, sum |d|, sum d^2, max |d|, sum x, min x, max x
constexpr int DIV_ROW = 8;                 // ... and the non-finite count (as int64 bits) in the workspace rows
constexpr int DIV_MAX_BLOCKS = 512;        // grid.x: grid-stride beyond two blocks per CU (grid.y carries the fields)

// the larger / smaller of two values, NaN if either is (mw_mlp_net.h: eval_max)
__device__ __forceinline__ double div_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double div_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double div_join(int s, double a, double b) { return (s == 3 || s == 6) ? div_max(a, b) : s == 5 ? div_min(a, b) : a + b; }

// A workgroup reads nens * C consecutive doubles per iteration, C = 256 / nens whole cells: lane l holds member l % nens of cell l / nens,
// always the same member, and the cell's member-0 value is in its own or the line before (L1).  Reduction: per lane in loop order, the
// C lanes of a member in lane order, then k_member_divergence_final over the blocks in block order -- no atomics, one fixed order.
__global__ __launch_bounds__(256) void k_member_divergence(long long n, int nens, MemberFields F, double *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[256][DIV_STATS];
  __shared__ long long cnt[256];
  const double *x = F.f[blockIdx.y];
  const int C = 256 / nens, l = threadIdx.x, e = l % nens, cl = l / nens;
  const bool lane_on = cl < C;
  double sd = 0.0, sa = 0.0, s2 = 0.0, md = 0.0, sx = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  long long bad = 0;
#pragma unroll 4
  for (long long c0 = (long long)blockIdx.x * C; c0 < n; c0 += (long long)gridDim.x * C) {
    const long long c = c0 + cl;
    if (lane_on && c < n) {
      const double v = x[c * nens + e], v0 = x[c * nens];
      const double d = v - v0;
      sd += d; sa += fabs(d); s2 += d * d; md = div_max(md, fabs(d));
      sx += v; mn = div_min(mn, v); mx = div_max(mx, v);
      bad += (v - v != 0.0) ? 1 : 0;                                       // NaN or inf
    }
  }
  red[l][0] = sd; red[l][1] = sa; red[l][2] = s2; red[l][3] = md; red[l][4] = sx; red[l][5] = mn; red[l][6] = mx;
  cnt[l] = bad;
  __syncthreads();
  for (int t = l; t < nens * DIV_ROW; t += 256) {
    const int m = t / DIV_ROW, s = t % DIV_ROW;
    double *row = partial + (((long long)blockIdx.x * gridDim.y + blockIdx.y) * nens + m) * DIV_ROW;
    if (s == DIV_STATS) {
      long long q = 0;
      for (int c = 0; c < C; c++) q += cnt[c * nens + m];
      ((long long *)row)[s] = q;
    } else {
      double q = red[m][s];
      for (int c = 1; c < C; c++) q = div_join(s, q, red[c * nens + m][s]);
      row[s] = q;
    }
  }
}

// thread = one number of `out` / `nonfinite`: the blocks' rows in block order
__global__ __launch_bounds__(256) void k_member_divergence_final(int nblocks, int nf, int nens, const double *__restrict__ partial,
                                                                 double *__restrict__ out, long long *__restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nf * nens * DIV_ROW) return;
  const int s = t % DIV_ROW, m = (t / DIV_ROW) % nens, f = t / (DIV_ROW * nens);
  const long long stride = (long long)nf * nens * DIV_ROW;
  const double *p = partial + ((long long)f * nens + m) * DIV_ROW + s;
  if (s == DIV_STATS) {
    long long q = 0;
    for (int b = 0; b < nblocks; b++) q += ((const long long *)p)[b * stride];
    nonfinite[(long long)m * nf + f] = q;
  } else {
    double q = p[0];
    for (int b = 1; b < nblocks; b++) q = div_join(s, q, p[b * stride]);
    out[((long long)m * nf + f) * DIV_STATS + s] = q;
  }
}

static long long divergence_blocks(long long n, int nens) {
  const long long C = 256 / nens;
  return std::max<long long>(1, std::min<long long>((n + C - 1) / C, DIV_MAX_BLOCKS));
}

// ---- mw_member_sample_mask / mw_member_gather_samples --------------------------------------------------------------------------------
struct MemberSample { const double *in[5]; const double *teach[4]; };       // temp, density_dry, vapor, cloud, rain | temp, vapor, cloud, rain

__device__ __forceinline__ bool f32_finite(double x) { const float f = (float)x; return f - f == 0.0f; }

// thread = flat element t = (k * ncol + col) * nens + e.  A listed member's element is taken if its draw u01(key0 + t) is below the
// threshold of its class (active: any of the four |teacher - input| > 1e-10, StatisticsGatherer::is_active) AND all fourteen values of its
// sample record -- the five inputs, the four of the level above, the four teacher values -- are finite as fp32.
__global__ __launch_bounds__(256) void k_member_sample_mask(MemberSample f, long long n, long long plane, int nens, unsigned long long listed,
                                                            unsigned long long key0, double thr_active, double thr_inactive,
                                                            unsigned char *__restrict__ mask) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int e = (int)(t % nens);
  if (!((listed >> e) & 1ull)) { mask[t] = 0; return; }
  const long long up = (t + plane < n) ? t + plane : t;                     // level min(nz - 1, k + 1) of the same column and member
  const int before[4] = {0, 2, 3, 4};                                       // the input that teacher value v replaces
  bool act = false, fin = f32_finite(f.in[1][t]);
  for (int v = 0; v < 4; v++) {
    const double a = f.in[before[v]][t], b = f.teach[v][t];
    act = act || (fabs(b - a) > 1.e-10);
    fin = fin && f32_finite(a) && f32_finite(b) && f32_finite(f.in[before[v]][up]);
  }
  const double thresh = act ? thr_active : thr_inactive;
  mask[t] = (fin && u01_from_key(key0 + (unsigned long long)t) < thresh) ? 1 : 0;
}

// k_gather_samples' records (n, 5, 2) / (n, 4) fp32 for flat element indices of the member layout
__global__ __launch_bounds__(256) void k_member_gather_samples(MemberSample f, const long long *__restrict__ elems, long long n, long long nelem,
                                                               long long plane, float *__restrict__ inputs, float *__restrict__ outputs) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const long long c = elems[s];
  float *in = inputs + s * 10, *out = outputs + s * 4;
  if (c < 0 || c >= nelem) {                                                // (an index outside the fields: a record of zeros, no load)
    for (int v = 0; v < 10; v++) in[v] = 0.0f;
    for (int v = 0; v < 4; v++) out[v] = 0.0f;
    return;
  }
  const long long up = (c + plane < nelem) ? c + plane : c;
  in[0] = (float)f.in[0][c];  in[2] = (float)f.in[1][c];  in[4] = (float)f.in[2][c];
  in[6] = (float)f.in[3][c];  in[8] = (float)f.in[4][c];
  in[1] = (float)f.in[0][up]; in[3] = (float)f.in[2][up]; in[5] = (float)f.in[3][up];
  in[7] = (float)f.in[4][up]; in[9] = 0.0f;
  for (int v = 0; v < 4; v++) out[v] = (float)f.teach[v][c];
}

// ---- mw_committee_guard_flags / mw_members_copy ---------------------------------------------------------------------------------------
struct GuardFields { const double *mean[4], *range[4]; double thr[4]; };

// A workgroup takes 64 consecutive columns of the member; lane l of each of its four wavefronts holds column 64 * block + l, and wavefront
// g the levels g, g + 4, ...  The member's elements of a level are nens doubles apart, so a wavefront's load touches the same 64-byte
// lines whichever way threads are laid over columns (a line holds 8 / nens of them, every line of the level for nens <= 8): the lines
// cannot be fewer.  An iteration loads the eight values of TWO levels into registers before it tests any of them, and the tests are
// joined with | on integers, not ||: with short-circuit tests every load waits for the test before it (one 8-byte load in flight per
// lane, and a lane that has flagged stops reading).  So a wavefront has sixteen loads in flight, a block four times that.  The OR over
// levels is order-free; the count is a popcount of the block's 64-bit mask and one integer atomicAdd per word.
__global__ __launch_bounds__(256) void k_committee_guard_flags(int nz, long long ncol, int nens, int member, GuardFields G,
                                                               unsigned char *__restrict__ flags, unsigned long long *__restrict__ counts) {
  __shared__ unsigned long long masks[4];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long c = (long long)blockIdx.x * 64 + lane;
  int bad = 0;
  if (c < ncol) {
    const long long plane = ncol * nens, base = c * nens + member;
    for (int k = g; k < nz; k += 8) {
      const long long idx0 = (long long)k * plane + base;
      const long long idx1 = (long long)(k + 4 < nz ? k + 4 : k) * plane + base;       // past the top: level k again, which an OR may see twice
      double r[8], m[8];
#pragma unroll
      for (int f = 0; f < 4; f++) { r[f] = G.range[f][idx0]; m[f] = G.mean[f][idx0]; r[4 + f] = G.range[f][idx1]; m[4 + f] = G.mean[f][idx1]; }
#pragma unroll
      for (int f = 0; f < 8; f++)                                                       // NaN flags; a range equal to its threshold does not
        bad |= (int)!(r[f] <= G.thr[f & 3]) | (int)!(fabs(m[f]) <= 1.7976931348623157e308);
    }
  }
  const bool flag = bad != 0;
  const unsigned long long mine = __ballot(flag);
  if (lane == 0) masks[g] = mine;
  __syncthreads();
  if (g != 0) return;
  const unsigned long long all = masks[0] | masks[1] | masks[2] | masks[3];
  if (c < ncol) flags[c * nens + member] = (unsigned char)((all >> lane) & 1ull);
  if (lane == 0 && all) {
    const unsigned long long q = (unsigned long long)__popcll(all);
    atomicAdd(counts, q);
    atomicAdd(counts + 1, q);
  }
}

// thread = flat element t = cell * nens + e, grid row y = field: the listed members' elements from src to dst
__global__ __launch_bounds__(256) void k_members_copy(long long total, int nens, unsigned long long listed, MemberFields src, MemberFields dst) {
  const double *a = src.f[blockIdx.y];
  double *b = dst.f[blockIdx.y];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256)
    if ((listed >> (int)(t % nens)) & 1ull) b[t] = a[t];
}

// ---- mw_member_column_water / mw_member_surface_rain ------------------------------------------------------------------------------------
struct WaterFields { const double *v, *c, *r; };
constexpr int WATER_AHEAD = 4;             // levels whose loads are issued ahead of their adds

// dz * sum over k of ((v + c) + r)[k * plane + t]: one fp64 accumulator from +0.0, k ascending, no contraction.  Thread t is one (column,
// member) of the plane, so a wavefront's loads of a level are 64 consecutive doubles per field whatever nens is.  The twelve loads of
// WATER_AHEAD levels are issued before the first add; the adds keep the order of k.
__device__ __forceinline__ double column_water(int nz, long long plane, long long t, const WaterFields &F, double dz) {
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
    for (int j = 0; j < WATER_AHEAD; j++) acc = acc + ((v[j] + c[j]) + r[j]);
  }
  for (; k < nz; k++) {
    const long long i = (long long)k * plane + t;
    acc = acc + ((F.v[i] + F.c[i]) + F.r[i]);
  }
  return dz * acc;
}

__global__ __launch_bounds__(256) void k_member_column_water(int nz, long long plane, WaterFields F, double dz, double *__restrict__ w) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < plane) w[t] = column_water(nz, plane, t, F, dz);
}

// The same sweep on the state after the step, and the finish: a listed member's precl is what the step took out of its column, signed;
// a member of `accum` adds dt * (whatever precl holds now) to its total.  Elements of members in neither set are not read or written.
__global__ __launch_bounds__(256) void k_member_surface_rain(int nz, long long plane, int nens, unsigned long long listed, unsigned long long accum,
                                                             WaterFields F, double dz, double dt, double per_rate,
                                                             const double *__restrict__ w_before, double *__restrict__ precl,
                                                             double *__restrict__ rain_total) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= plane) return;
  const int e = (int)(t % nens);
  const bool mine = (listed >> e) & 1ull, sums = (accum >> e) & 1ull;
  if (!mine && !sums) return;
  double p;
  if (mine) {
    p = (w_before[t] - column_water(nz, plane, t, F, dz)) / per_rate;       // per_rate = 1000.0 * dt: kg / m^2 to m of water per second
    precl[t] = p;
  } else {
    p = precl[t];
  }
  if (sums) rain_total[t] = rain_total[t] + dt * p;
}

// ---- mw_member_water_fix ------------------------------------------------------------------------------------------------------------
struct FixFields { double *v, *c, *r; };
constexpr int FIX_ROW = 4;                 // per block and member: fixed columns, skipped columns (int64 bits), sum of excess, max of excess
constexpr int FIX_FIXED = 1, FIX_SKIPPED = 2;

// k_member_surface_rain with the remedy.  Thread t is one (column, member) of the plane and first sweeps its column as
// column_water does.  A member of `fixed` whose column holds more water than before the step (W_a - W_b > tolerance * W_b, W_b >= 0)
// sweeps it a second time: the twelve loads of WATER_AHEAD levels, each value times s = W_b / W_a, twelve ordinary stores, and the stored
// products summed in column_water's order, so that column_water of the state left behind is W' to the bit.  The second sweep is behind a
// ballot: a wavefront with no column to fix does not enter it.  Statistics: every lane's flags and excess go to LDS; a block with nothing
// fixed or skipped writes rows of zeros, any other folds, for member m and each of the four numbers, the lanes of m in ascending lane
// order (one thread per number).  k_member_water_fix_final then folds the blocks' rows.  No atomics, no memset, one fixed order.
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
    if (flag == FIX_FIXED) {
      const double s = wb / wa;
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
          const long long i = (long long)(k + j) * plane + t;
          v[j] = v[j] * s; c[j] = c[j] * s; r[j] = r[j] * s;
          F.v[i] = v[j]; F.c[i] = c[j]; F.r[i] = r[j];
          acc = acc + ((v[j] + c[j]) + r[j]);
        }
      }
      for (; k < nz; k++) {
        const long long i = (long long)k * plane + t;
        const double v = F.v[i] * s, c = F.c[i] * s, r = F.r[i] * s;
        F.v[i] = v; F.c[i] = c; F.r[i] = r;
        acc = acc + ((v + c) + r);
      }
      wa = dz * acc;                                                           // W': what column_water now returns for this column
    }
  }
  if (mine || sums) {
    double p;
    if (mine) {
      p = (wb - wa) / per_rate;
      precl[t] = p;
    } else {
      p = precl[t];
    }
    if (sums) rain_total[t] = rain_total[t] + dt * p;
  }
  if (excess && in) excess[t] = over;
  ex[l] = over;
  what[l] = flag;
  if (!__syncthreads_or(flag)) {                                               // nothing fixed or skipped in this block: what the fold below would give
    if (l < nens * FIX_ROW) partial[(long long)blockIdx.x * nens * FIX_ROW + l] = 0.0;     // (+0.0 is the int64 0 too)
    return;
  }
  if (l < nens * FIX_ROW) {
    const int m = l / FIX_ROW, s = l % FIX_ROW;
    const int first = (int)(((long long)m - (long long)(((long long)blockIdx.x * 256) % nens) + nens) % nens);      // the block's first lane of member m
    double *row = partial + ((long long)blockIdx.x * nens + m) * FIX_ROW;
    if (s < 2) {
      long long q = 0;
      for (int j = first; j < 256; j += nens) q += (what[j] == s + 1) ? 1 : 0;
      ((long long *)row)[s] = q;
    } else {
      double q = 0.0;
      for (int j = first; j < 256; j += nens) q = (s == 2) ? q + ex[j] : (ex[j] > q ? ex[j] : q);
      row[s] = q;
    }
  }
}

// block m = member m; thread l folds the rows of the blocks l, l + 256, ... in ascending order, then threads 0 .. 3 fold the 256 partial
// results of one number each in ascending l.  counts (nens, 2) = fixed, skipped; stats (nens, 2) = sum, max of the excess.
__global__ __launch_bounds__(256) void k_member_water_fix_final(long long nblocks, int nens, const double *__restrict__ partial,
                                                                long long *__restrict__ counts, double *__restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double red[256][2];
  __shared__ long long cnt[256][2];
  const int m = blockIdx.x, l = threadIdx.x;
  long long nf = 0, ns = 0;
  double sum = 0.0, mx = 0.0;
  for (long long b = l; b < nblocks; b += 256) {
    const double *row = partial + (b * nens + m) * FIX_ROW;
    nf += ((const long long *)row)[0]; ns += ((const long long *)row)[1];
    sum = sum + row[2]; mx = row[3] > mx ? row[3] : mx;
  }
  cnt[l][0] = nf; cnt[l][1] = ns; red[l][0] = sum; red[l][1] = mx;
  __syncthreads();
  if (l < 2) {
    long long q = 0;
    for (int j = 0; j < 256; j++) q += cnt[j][l];
    counts[m * 2 + l] = q;
  } else if (l < 4) {
    double q = red[0][l - 2];
    for (int j = 1; j < 256; j++) q = (l == 2) ? q + red[j][0] : (red[j][1] > q ? red[j][1] : q);
    stats[m * 2 + (l - 2)] = q;
  }
}

static long long water_fix_blocks(long long ncol, int nens) { return (ncol * nens + 255) / 256; }

// ---- mw_member_rain_table -----------------------------------------------------------------------------------------------------------
constexpr int RAIN_MAX_FIELDS = 4, RAIN_MAX_THR = 8;
constexpr int RAIN_OUT = 5;                // hits, misses, false alarms, correct negatives, non-finite
constexpr int RAIN_ROW = 3 * RAIN_MAX_THR + 2;   // per lane: hits, misses, false alarms per threshold, then non-finite and finite columns
constexpr int RAIN_MAX_BLOCKS = 512;

struct RainFields { const double *f[RAIN_MAX_FIELDS]; int nt[RAIN_MAX_FIELDS]; double thr[RAIN_MAX_FIELDS][RAIN_MAX_THR]; };

// k_member_divergence's layout: a workgroup reads nens * C consecutive doubles per iteration, lane l always member l % nens.  The counts
// are integers: per lane, then the C lanes of a member, then k_member_rain_table_final over the blocks -- any order gives the same numbers.
__global__ __launch_bounds__(256) void k_member_rain_table(long long n, int nens, RainFields R, long long *__restrict__ partial) {
  __shared__ int red[256][RAIN_ROW + 1];                                    // (+ 1: rows on different banks)
  const int fi = blockIdx.y, nt = R.nt[fi];
  const double *x = R.f[fi];
  const int C = 256 / nens, l = threadIdx.x, e = l % nens, cl = l / nens;
  int cnt[RAIN_ROW];
#pragma unroll
  for (int s = 0; s < RAIN_ROW; s++) cnt[s] = 0;
  for (long long c0 = (long long)blockIdx.x * C; c0 < n; c0 += (long long)gridDim.x * C) {
    const long long c = c0 + cl;
    if (cl < C && c < n) {
      const double v = x[c * nens + e], v0 = x[c * nens];
      const bool fin = (v - v == 0.0) && (v0 - v0 == 0.0);                  // a NaN or inf of the member or of member 0 takes the column out
      cnt[3 * RAIN_MAX_THR] += fin ? 0 : 1;
      cnt[3 * RAIN_MAX_THR + 1] += fin ? 1 : 0;
#pragma unroll
      for (int j = 0; j < RAIN_MAX_THR; j++) {
        const bool on = fin && j < nt, fc = v >= R.thr[fi][j], ob = v0 >= R.thr[fi][j];
        cnt[3 * j] += (on && fc && ob) ? 1 : 0;
        cnt[3 * j + 1] += (on && !fc && ob) ? 1 : 0;
        cnt[3 * j + 2] += (on && fc && !ob) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < RAIN_ROW; s++) red[l][s] = cnt[s];
  __syncthreads();
  for (int t = l; t < nens * RAIN_ROW; t += 256) {
    const int m = t / RAIN_ROW, s = t % RAIN_ROW;
    long long q = 0;
    for (int c = 0; c < C; c++) q += red[c * nens + m][s];
    partial[(((long long)blockIdx.x * gridDim.y + fi) * nens + m) * RAIN_ROW + s] = q;
  }
}

// thread = one (field, threshold, member): the blocks' rows summed, the correct negatives as what is left of the finite columns
__global__ __launch_bounds__(256) void k_member_rain_table_final(int nblocks, int nf, int nens, RainFields R, const long long *__restrict__ partial,
                                                                 long long *__restrict__ counts) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nf * RAIN_MAX_THR * nens) return;
  const int m = t % nens, j = (t / nens) % RAIN_MAX_THR, f = t / (nens * RAIN_MAX_THR);
  long long q[5] = {0, 0, 0, 0, 0};                                         // hits, misses, false alarms, non-finite, finite
  if (j < R.nt[f]) {
    const long long stride = (long long)nf * nens * RAIN_ROW;
    const long long *p = partial + ((long long)f * nens + m) * RAIN_ROW;
    for (int b = 0; b < nblocks; b++) {
      const long long *row = p + b * stride;
      q[0] += row[3 * j]; q[1] += row[3 * j + 1]; q[2] += row[3 * j + 2]; q[3] += row[3 * RAIN_MAX_THR]; q[4] += row[3 * RAIN_MAX_THR + 1];
    }
  }
  long long *out = counts + (long long)t * RAIN_OUT;
  out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[4] - q[0] - q[1] - q[2]; out[4] = q[3];
}

static long long rain_table_blocks(long long n, int nens) {
  const long long C = 256 / nens;
  return std::max<long long>(1, std::min<long long>((n + C - 1) / C, RAIN_MAX_BLOCKS));
}

// ---- mw_member_domain ---------------------------------------------------------------------------------------------------------------
constexpr int DOMAIN_MAX_MEMBERS = 32;     // the boxes travel in the kernel arguments: 32 x 80 bytes
constexpr int DOMAIN_WORDS = 16;           // per listed member: 3 f + c (c: below, above, nan) for the five fields, word 15 the outside columns
constexpr int DOMAIN_ROW = DOMAIN_WORDS + 1;   // ... and, in LDS only, the flag bytes this block turned from 0 to 1

struct DomainArgs {
  const double *in[5];
  double box[DOMAIN_MAX_MEMBERS][5][2];    // [listed member][field][lo, hi]
  int slot[DOMAIN_MAX_MEMBERS];            // < 0: the member's flag bytes are not touched
  signed char listed_at[64];               // member e is box / slot / counts row listed_at[e], -1: not listed
};

// A workgroup takes 64 consecutive elements t = col * nens + e of the (ncol, nens) plane, lane l of each of its four wavefronts element
// 64 * block + l (k_member_column_water's layout: a wavefront's load of a level is 64 consecutive doubles per field whatever nens is),
// and wavefront g the levels g, g + 4, ... (k_committee_guard_flags' split: at nens = 1 a 400 x 400 plane is 2,500 wavefronts, a quarter
// of what the chip holds; the split makes them 10,000).  An iteration issues the ten loads of TWO levels before the first test; the
// second level past the top is level k again with its counts masked by `on`.  The tests are joined with | on integers (see above).
// Counts: fifteen registers per lane, then LDS integer adds into the block's row of the lane's member (zero words skipped), then one
// global atomicAdd per non-zero word and block.  The OR over the four wavefronts' levels goes through ballots as in the flags kernel;
// wavefront 0 then owns the element's flag byte, so its read-test-write needs no atomic.  Integer adds only: any order, the same numbers.
__global__ __launch_bounds__(256) void k_member_domain(int nz, long long plane, int nens, int nm, DomainArgs A,
                                                       unsigned long long *__restrict__ counts, unsigned char *__restrict__ flags,
                                                       unsigned long long *__restrict__ flag_counts) {
  __shared__ unsigned long long masks[4];
  __shared__ unsigned int rows[DOMAIN_MAX_MEMBERS * DOMAIN_ROW];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long t = (long long)blockIdx.x * 64 + lane;
  for (int w = threadIdx.x; w < nm * DOMAIN_ROW; w += 256) rows[w] = 0u;
  __syncthreads();
  const int j = t < plane ? (int)A.listed_at[(int)(t % nens)] : -1;
  int bad = 0;
  if (j >= 0) {
    double lo[5], hi[5];
#pragma unroll
    for (int f = 0; f < 5; f++) { lo[f] = A.box[j][f][0]; hi[f] = A.box[j][f][1]; }
    int cnt[15];
#pragma unroll
    for (int w = 0; w < 15; w++) cnt[w] = 0;
    for (int k = g; k < nz; k += 8) {
      const int on = k + 4 < nz ? 1 : 0;
      const long long idx0 = (long long)k * plane + t;
      const long long idx1 = (long long)(on ? k + 4 : k) * plane + t;
      double x[10];
#pragma unroll
      for (int f = 0; f < 5; f++) { x[f] = A.in[f][idx0]; x[5 + f] = A.in[f][idx1]; }
      __builtin_amdgcn_sched_barrier(0);                                    // (left alone the scheduler tests after two loads: four in flight)
#pragma unroll
      for (int f = 0; f < 5; f++) {
        const int b0 = (int)(x[f] < lo[f]), a0 = (int)(x[f] > hi[f]), n0 = (int)(x[f] != x[f]);
        const int b1 = (int)(x[5 + f] < lo[f]) & on, a1 = (int)(x[5 + f] > hi[f]) & on, n1 = (int)(x[5 + f] != x[5 + f]) & on;
        cnt[3 * f] += b0 + b1; cnt[3 * f + 1] += a0 + a1; cnt[3 * f + 2] += n0 + n1;
        bad |= b0 | a0 | n0 | b1 | a1 | n1;
      }
    }
#pragma unroll
    for (int w = 0; w < 15; w++)
      if (cnt[w]) atomicAdd(&rows[j * DOMAIN_ROW + w], (unsigned int)cnt[w]);
  }
  const unsigned long long mine = __ballot(bad != 0);
  if (lane == 0) masks[g] = mine;
  __syncthreads();
  if (g == 0) {
    const unsigned long long all = masks[0] | masks[1] | masks[2] | masks[3];
    if (j >= 0 && ((all >> lane) & 1ull)) {
      atomicAdd(&rows[j * DOMAIN_ROW + 15], 1u);
      if (A.slot[j] >= 0) {
        const unsigned char old = flags[t];
        if (old != 1) flags[t] = 1;
        if (old == 0) atomicAdd(&rows[j * DOMAIN_ROW + DOMAIN_WORDS], 1u);
      }
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nm * DOMAIN_ROW; w += 256) {
    const unsigned int q = rows[w];
    if (!q) continue;
    const int m = w / DOMAIN_ROW, s = w % DOMAIN_ROW;
    if (s < DOMAIN_WORDS) {
      atomicAdd(counts + m * DOMAIN_WORDS + s, (unsigned long long)q);
    } else {
      atomicAdd(flag_counts + 2 * A.slot[m], (unsigned long long)q);
      atomicAdd(flag_counts + 2 * A.slot[m] + 1, (unsigned long long)q);
    }
  }
}

// ---- mw_member_sample_mask_domain ---------------------------------------------------------------------------------------------------
constexpr int SAMPLE_CLASSES = 3;          // outside the member's box, active, inactive
constexpr int SAMPLE_WORDS = 2 * SAMPLE_CLASSES;   // per listed member: eligible per class, then taken per class

struct SampleDomainArgs {
  const double *in[5], *teach[4];
  double box[DOMAIN_MAX_MEMBERS][5][2];    // [listed member][field][lo, hi]
  double thr[DOMAIN_MAX_MEMBERS][SAMPLE_CLASSES];
  unsigned int above;                      // bit j: listed member j's model reads the level above, whose four values are tested too
  signed char listed_at[64];               // member e is box / thr / counts row listed_at[e], -1: not listed
};
// 72 + 2560 + 768 + 4 (+ 4 padding) + 64 = 3472 bytes, and 48 of scalars and pointers beside it: under the 4 KB of kernel arguments
static_assert(sizeof(SampleDomainArgs) + 48 <= 4096, "SampleDomainArgs no longer fits the kernel arguments: upload it instead");

// lane = flat element t = (k * ncol + col) * nens + e, as in k_member_sample_mask, with a third class in front of its two: an eligible
// element (all fourteen values of its record finite as fp32) is OUTSIDE if one of its five inputs -- with the member's `above` bit also one
// of the four values of the level above -- is below lo or above hi of the member's box; otherwise active or inactive as before.  The
// thirteen loads are issued before the first test, and the tests are joined with | and & on integers (k_member_domain).  Counts: six
// ballots per wavefront (eligible and taken per class), one ballot per listed member for its lanes, popcounts in lanes 0 .. 5 and LDS
// integer adds into the block's row of that member; then one global atomicAdd per non-zero word and block.  The grid is capped
// (SAMPLE_MAX_BLOCKS) and a block strides over the elements: with one block per 256 elements a 400 x 400 x 100 x 8 state issues 18 million
// global atomics onto 36 words, which cost five times the loads.  Integer adds only: any order, the same numbers.
constexpr int SAMPLE_MAX_BLOCKS = 256 * 16;

__global__ __launch_bounds__(256) void k_member_sample_mask_domain(SampleDomainArgs A, long long n, long long plane, int nens, int nm,
                                                                   unsigned long long key0, unsigned char *__restrict__ mask,
                                                                   unsigned long long *__restrict__ counts) {
  __shared__ unsigned int rows[DOMAIN_MAX_MEMBERS * SAMPLE_WORDS];
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x; w < nm * SAMPLE_WORDS; w += 256) rows[w] = 0u;
  __syncthreads();
  for (long long first = (long long)blockIdx.x * 256; first < n; first += (long long)gridDim.x * 256) {     // (block-uniform: the ballots see whole wavefronts)
    const long long t = first + threadIdx.x;
    const int j = t < n ? (int)A.listed_at[(int)(t % nens)] : -1;
    int cls = -1, take = 0;                                                 // cls < 0: not eligible (or not listed, or past the end)
    if (j >= 0) {
      const long long up = (t + plane < n) ? t + plane : t;                 // level min(nz - 1, k + 1) of the same column and member
      const int before[4] = {0, 2, 3, 4};                                   // the input that teacher value v replaces
      double x[5], u[4], b[4], lo[5], hi[5];
#pragma unroll
      for (int f = 0; f < 5; f++) { x[f] = A.in[f][t]; lo[f] = A.box[j][f][0]; hi[f] = A.box[j][f][1]; }
#pragma unroll
      for (int v = 0; v < 4; v++) { u[v] = A.in[before[v]][up]; b[v] = A.teach[v][t]; }
      __builtin_amdgcn_sched_barrier(0);
      const int ab = (int)((A.above >> j) & 1u);
      int fin = (int)f32_finite(x[1]), act = 0, out = 0;
#pragma unroll
      for (int f = 0; f < 5; f++) out |= (int)(x[f] < lo[f]) | (int)(x[f] > hi[f]);
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const double a = x[before[v]];
        act |= (int)(fabs(b[v] - a) > 1.e-10);
        fin &= (int)f32_finite(a) & (int)f32_finite(b[v]) & (int)f32_finite(u[v]);
        out |= ((int)(u[v] < lo[before[v]]) | (int)(u[v] > hi[before[v]])) & ab;
      }
      if (fin) {
        cls = out ? 0 : act ? 1 : 2;
        take = (int)(u01_from_key(key0 + (unsigned long long)t) < A.thr[j][cls]);
      }
    }
    if (mask && t < n) mask[t] = (unsigned char)take;
    const unsigned long long e0 = __ballot(cls == 0), e1 = __ballot(cls == 1), e2 = __ballot(cls == 2);
    const unsigned long long t0 = __ballot(take && cls == 0), t1 = __ballot(take && cls == 1), t2 = __ballot(take && cls == 2);
    const unsigned long long mine = lane == 0 ? e0 : lane == 1 ? e1 : lane == 2 ? e2 : lane == 3 ? t0 : lane == 4 ? t1 : t2;
    if (e0 | e1 | e2) {
      for (int jj = 0; jj < nm; jj++) {
        const unsigned long long lanes = __ballot(j == jj);
        if (lane < SAMPLE_WORDS) {
          const unsigned int q = (unsigned int)__popcll(mine & lanes);
          if (q) atomicAdd(&rows[jj * SAMPLE_WORDS + lane], q);
        }
      }
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nm * SAMPLE_WORDS; w += 256) {
    const unsigned int q = rows[w];
    if (q) atomicAdd(counts + w, (unsigned long long)q);
  }
}

} // namespace mw

using namespace mw;

static int member_copy(bool insert, long long n, int nens, int member, int nf, double *const *fused, double *const *flat, void *stream) {
  const char *who = insert ? "member_insert" : "member_extract";
  if (!fused || !flat) MW_FAIL(std::string(who) + ": null pointer");
  if (n < 1 || nens < 1) MW_FAIL(std::string(who) + ": n and nens must be >= 1");
  if (member < 0 || member >= nens) MW_FAIL(std::string(who) + ": member " + std::to_string(member) + " is outside [0, " + std::to_string(nens) + ")");
  if (nf < 1 || nf > MW_MAX_TRACERS) MW_FAIL(std::string(who) + ": nf must be in [1, " + std::to_string(MW_MAX_TRACERS) + "]");
  MemberFields A, B;
  for (int f = 0; f < MW_MAX_TRACERS; f++) { A.f[f] = nullptr; B.f[f] = nullptr; }
  for (int f = 0; f < nf; f++) {
    if (!fused[f] || !flat[f]) MW_FAIL(std::string(who) + ": null field");
    A.f[f] = fused[f]; B.f[f] = flat[f];
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long blocks = std::max<long long>(1, std::min<long long>((n + 255) / 256, 256 * 16));
  if (insert) hipLaunchKernelGGL(k_member_copy<true>, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, (hipStream_t)stream, n, nens, member, A, B);
  else        hipLaunchKernelGGL(k_member_copy<false>, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, (hipStream_t)stream, n, nens, member, A, B);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_member_extract(long long n, int nens, int member, int nf, const double *const *fields, double *const *out, void *stream) {
  return member_copy(false, n, nens, member, nf, (double *const *)fields, out, stream);
}

extern "C" int mw_member_insert(long long n, int nens, int member, int nf, const double *const *in, double *const *fields, void *stream) {
  return member_copy(true, n, nens, member, nf, fields, (double *const *)in, stream);
}

extern "C" long long mw_member_divergence_workspace_bytes(long long n, int nens, int nf) {
  if (n < 1 || nens < 1 || nens > 256 || nf < 1 || nf > MW_MAX_TRACERS) return 0;
  return divergence_blocks(n, nens) * nf * nens * DIV_ROW * 8;
}

extern "C" int mw_member_divergence(long long n, int nens, int nf, const double *const *fields, void *workspace, double *out,
                                    long long *nonfinite, void *stream) {
  if (!fields || !workspace || !out || !nonfinite) MW_FAIL("member_divergence: null pointer");
  if (n < 1) MW_FAIL("member_divergence: n must be >= 1");
  if (nens < 1 || nens > 256) MW_FAIL("member_divergence: nens must be in [1, 256]");
  if (nf < 1 || nf > MW_MAX_TRACERS) MW_FAIL("member_divergence: nf must be in [1, " + std::to_string(MW_MAX_TRACERS) + "]");
  MemberFields F;
  for (int f = 0; f < MW_MAX_TRACERS; f++) F.f[f] = nullptr;
  for (int f = 0; f < nf; f++) { if (!fields[f]) MW_FAIL("member_divergence: null field"); F.f[f] = (double *)fields[f]; }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = divergence_blocks(n, nens);
  hipLaunchKernelGGL(k_member_divergence, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, st, n, nens, F, (double *)workspace);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_member_divergence_final, dim3((unsigned)((nf * nens * DIV_ROW + 255) / 256)), dim3(256), 0, st, (int)blocks, nf, nens,
                     (const double *)workspace, out, nonfinite);
  MW_LAUNCH_CHECK();
  return 0;
}

static int member_sample_fields(const char *who, int nz, long long ncol, int nens, const double *const *fields5, const double *const *teacher4,
                                MemberSample *f) {
  if (!fields5 || !teacher4) MW_FAIL(std::string(who) + ": null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL(std::string(who) + ": nz and ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL(std::string(who) + ": nens must be in [1, 64]");
  for (int v = 0; v < 5; v++) { if (!fields5[v]) MW_FAIL(std::string(who) + ": null field"); f->in[v] = fields5[v]; }
  for (int v = 0; v < 4; v++) { if (!teacher4[v]) MW_FAIL(std::string(who) + ": null field"); f->teach[v] = teacher4[v]; }
  return 0;
}

extern "C" int mw_member_sample_mask(int nz, long long ncol, int nens, int nm, const int *members, const double *const *fields5,
                                     const double *const *teacher4, unsigned long long key0, double thr_active, double thr_inactive,
                                     unsigned char *mask, void *stream) {
  MemberSample f;
  if (member_sample_fields("member_sample_mask", nz, ncol, nens, fields5, teacher4, &f)) return 1;
  if (!members || !mask) MW_FAIL("member_sample_mask: null pointer");
  if (nm < 1 || nm > nens) MW_FAIL("member_sample_mask: nm must be in [1, nens]");
  unsigned long long listed = 0;
  for (int j = 0; j < nm; j++) {
    const int e = members[j];
    if (e < 0 || e >= nens) MW_FAIL("member_sample_mask: member " + std::to_string(e) + " is outside [0, " + std::to_string(nens) + ")");
    if ((listed >> e) & 1ull) MW_FAIL("member_sample_mask: member " + std::to_string(e) + " is listed twice");
    listed |= 1ull << e;
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long plane = ncol * nens, n = plane * nz;
  hipLaunchKernelGGL(k_member_sample_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, n, plane, nens, listed, key0,
                     thr_active, thr_inactive, mask);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_member_sample_mask_domain(int nz, long long ncol, int nens, int nm, const int *members, const double *box, const int *above,
                                            const double *const *fields5, const double *const *teacher4, unsigned long long key0,
                                            const double *thr, unsigned char *mask, long long *counts, void *stream) {
  MemberSample f;
  if (member_sample_fields("member_sample_mask_domain", nz, ncol, nens, fields5, teacher4, &f)) return 1;
  if (!members || !box || !above || !thr) MW_FAIL("member_sample_mask_domain: null pointer");
  if (!counts) MW_FAIL("member_sample_mask_domain: null pointer (counts; the mask alone may be null: count only)");
  if (nm < 1 || nm > DOMAIN_MAX_MEMBERS) MW_FAIL("member_sample_mask_domain: nm must be in [1, " + std::to_string(DOMAIN_MAX_MEMBERS) + "]");
  if ((double)nz * (double)ncol * (double)nens > 256.0 * 2147483647.0) MW_FAIL("member_sample_mask_domain: the fields are too large");   // (a block's LDS counters are 32-bit)
  SampleDomainArgs A;
  for (int v = 0; v < 5; v++) A.in[v] = f.in[v];
  for (int v = 0; v < 4; v++) A.teach[v] = f.teach[v];
  A.above = 0u;
  for (int e = 0; e < 64; e++) A.listed_at[e] = -1;
  for (int j = 0; j < DOMAIN_MAX_MEMBERS; j++) {
    for (int c = 0; c < SAMPLE_CLASSES; c++) A.thr[j][c] = 0.0;
    for (int v = 0; v < 5; v++) { A.box[j][v][0] = -__builtin_inf(); A.box[j][v][1] = __builtin_inf(); }
  }
  for (int j = 0; j < nm; j++) {
    const int e = members[j];
    if (e < 0 || e >= nens) MW_FAIL("member_sample_mask_domain: member " + std::to_string(e) + " is outside [0, " + std::to_string(nens) + ")");
    if (A.listed_at[e] >= 0) MW_FAIL("member_sample_mask_domain: member " + std::to_string(e) + " is listed twice");
    A.listed_at[e] = (signed char)j;
    for (int v = 0; v < 5; v++) {
      const double lo = box[(j * 5 + v) * 2], hi = box[(j * 5 + v) * 2 + 1];
      if (!(lo <= hi)) MW_FAIL("member_sample_mask_domain: the box of member " + std::to_string(e) + ", field " + std::to_string(v) +
                               ", is not lo <= hi (NaN is refused, +-inf is allowed)");
      A.box[j][v][0] = lo; A.box[j][v][1] = hi;
    }
    for (int c = 0; c < SAMPLE_CLASSES; c++) {
      const double x = thr[j * SAMPLE_CLASSES + c];
      if (!(x >= 0.0 && x <= 1.0)) MW_FAIL("member_sample_mask_domain: threshold " + std::to_string(c) + " of member " + std::to_string(e) +
                                           " is NaN or outside [0, 1]");
      A.thr[j][c] = x;
    }
    if (above[j]) A.above |= 1u << j;
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long plane = ncol * nens, n = plane * nz;
  MW_HIP(hipMemsetAsync(counts, 0, (size_t)nm * SAMPLE_WORDS * 8, st));     // counts is SET: the adds start from zero
  const long long blocks = std::min<long long>((n + 255) / 256, SAMPLE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_member_sample_mask_domain, dim3((unsigned)blocks), dim3(256), 0, st, A, n, plane, nens, nm, key0, mask,
                     (unsigned long long *)counts);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_member_gather_samples(int nz, long long ncol, int nens, const double *const *fields5, const double *const *teacher4,
                                        const long long *elems, long long n, float *inputs, float *outputs, void *stream) {
  MemberSample f;
  if (member_sample_fields("member_gather_samples", nz, ncol, nens, fields5, teacher4, &f)) return 1;
  if (n < 0) MW_FAIL("member_gather_samples: n must be >= 0");
  if (n == 0) return 0;
  if (!elems || !inputs || !outputs) MW_FAIL("member_gather_samples: null pointer");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long plane = ncol * nens;
  hipLaunchKernelGGL(k_member_gather_samples, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, elems, n, plane * nz, plane,
                     inputs, outputs);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_committee_guard_flags(int nz, long long ncol, int nens, int member, const double *const *mean4, const double *const *range4,
                                        const double *thr4, unsigned char *flags, long long *counts, void *stream) {
  if (!mean4 || !range4 || !thr4 || !flags || !counts) MW_FAIL("committee_guard_flags: null pointer");
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL("committee_guard_flags: nz, ncol and nens must be >= 1");
  if (member < 0 || member >= nens) MW_FAIL("committee_guard_flags: member " + std::to_string(member) + " is outside [0, " + std::to_string(nens) + ")");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18) MW_FAIL("committee_guard_flags: the fields are too large");
  GuardFields G;
  for (int f = 0; f < 4; f++) {
    if (!mean4[f] || !range4[f]) MW_FAIL("committee_guard_flags: null field");
    if (!(thr4[f] >= 0.0)) MW_FAIL("committee_guard_flags: threshold " + std::to_string(f) + " is negative or NaN (+inf: the field never flags by size)");
    G.mean[f] = mean4[f]; G.range[f] = range4[f]; G.thr[f] = thr4[f];
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  MW_HIP(hipMemsetAsync(counts, 0, 8, st));                                 // counts[0]: this call's count; counts[1] goes on accumulating
  hipLaunchKernelGGL(k_committee_guard_flags, dim3((unsigned)((ncol + 63) / 64)), dim3(256), 0, st, nz, ncol, nens, member, G, flags,
                     (unsigned long long *)counts);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_members_copy(long long n, int nens, int nm, const int *members, int nf, const double *const *src, double *const *dst,
                               void *stream) {
  if (!members || !src || !dst) MW_FAIL("members_copy: null pointer");
  if (n < 1) MW_FAIL("members_copy: n must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("members_copy: nens must be in [1, 64]");
  if (nm < 1 || nm > nens) MW_FAIL("members_copy: nm must be in [1, nens]");
  if (nf < 1 || nf > MW_MAX_TRACERS) MW_FAIL("members_copy: nf must be in [1, " + std::to_string(MW_MAX_TRACERS) + "]");
  if ((double)n * (double)nens > 9.0e18) MW_FAIL("members_copy: the fields are too large");
  unsigned long long listed = 0;
  for (int j = 0; j < nm; j++) {
    const int e = members[j];
    if (e < 0 || e >= nens) MW_FAIL("members_copy: member " + std::to_string(e) + " is outside [0, " + std::to_string(nens) + ")");
    if ((listed >> e) & 1ull) MW_FAIL("members_copy: member " + std::to_string(e) + " is listed twice");
    listed |= 1ull << e;
  }
  MemberFields A, B;
  for (int f = 0; f < MW_MAX_TRACERS; f++) { A.f[f] = nullptr; B.f[f] = nullptr; }
  for (int f = 0; f < nf; f++) {
    if (!src[f] || !dst[f]) MW_FAIL("members_copy: null field");
    A.f[f] = (double *)src[f]; B.f[f] = dst[f];
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long total = n * nens;
  const long long blocks = std::max<long long>(1, std::min<long long>((total + 255) / 256, 256 * 16));
  hipLaunchKernelGGL(k_members_copy, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, (hipStream_t)stream, total, nens, listed, A, B);
  MW_LAUNCH_CHECK();
  return 0;
}

static bool positive_finite(double x) { return x > 0.0 && x - x == 0.0; }

// the bit set of a member list: distinct indices in [0, nens), nens <= 64
static int member_bits(const char *who, const char *what, int nens, int n, const int *list, unsigned long long *bits) {
  if (n < 0 || n > nens) MW_FAIL(std::string(who) + ": " + what + " holds " + std::to_string(n) + " members, not 0 to nens");
  if (n > 0 && !list) MW_FAIL(std::string(who) + ": null pointer");
  *bits = 0;
  for (int j = 0; j < n; j++) {
    const int e = list[j];
    if (e < 0 || e >= nens) MW_FAIL(std::string(who) + ": member " + std::to_string(e) + " is outside [0, " + std::to_string(nens) + ")");
    if ((*bits >> e) & 1ull) MW_FAIL(std::string(who) + ": member " + std::to_string(e) + " is listed twice in " + what);
    *bits |= 1ull << e;
  }
  return 0;
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
  if (ncol < 1 || nens < 1 || nens > 64 || (double)ncol * (double)nens > 256.0 * 2147483647.0) return 0;
  return water_fix_blocks(ncol, nens) * nens * FIX_ROW * 8;
}

extern "C" int mw_member_water_fix(int nz, long long ncol, int nens, int nm, const int *members, int na, const int *accum, int nfix,
                                   const int *fixed, double tolerance, double *const *water3, double dz, double dt, const double *w_before,
                                   double *precl, double *rain_total, void *workspace, long long *counts, double *stats, double *excess,
                                   void *stream) {
  WaterFields R;
  if (water_fields("member_water_fix", nz, ncol, nens, water3, dz, &R)) return 1;
  if (!positive_finite(dt)) MW_FAIL("member_water_fix: dt must be positive and finite");
  if (!(tolerance >= 0.0 && tolerance - tolerance == 0.0)) MW_FAIL("member_water_fix: tolerance must be finite and >= 0");
  unsigned long long listed = 0, sums = 0, fix = 0;
  if (member_bits("member_water_fix", "members", nens, nm, members, &listed)) return 1;
  if (member_bits("member_water_fix", "accum", nens, na, accum, &sums)) return 1;
  if (member_bits("member_water_fix", "fixed", nens, nfix, fixed, &fix)) return 1;
  for (int e = 0; e < nens; e++)
    if (((fix & ~listed) >> e) & 1ull) MW_FAIL("member_water_fix: member " + std::to_string(e) + " is in fixed but not in members (a fixed member is a budget member)");
  if (!precl || (nm > 0 && !w_before) || (na > 0 && !rain_total) || !workspace || !counts || !stats) MW_FAIL("member_water_fix: null pointer");
  if (water3[0] == water3[1] || water3[0] == water3[2] || water3[1] == water3[2]) MW_FAIL("member_water_fix: the three water fields must be three arrays");
  if ((double)ncol * (double)nens > 256.0 * 2147483647.0) MW_FAIL("member_water_fix: the fields are too large");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const FixFields F = {water3[0], water3[1], water3[2]};
  hipStream_t st = (hipStream_t)stream;
  const long long plane = ncol * nens, blocks = water_fix_blocks(ncol, nens);
  hipLaunchKernelGGL(k_member_water_fix, dim3((unsigned)blocks), dim3(256), 0, st, nz, plane, nens, listed, sums, fix, tolerance, F, dz, dt,
                     1000.0 * dt, w_before, precl, rain_total, (double *)workspace, excess);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_member_water_fix_final, dim3((unsigned)nens), dim3(256), 0, st, blocks, nens, (const double *)workspace, counts, stats);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" long long mw_member_rain_table_workspace_bytes(long long ncol, int nens, int nf) {
  if (ncol < 1 || nens < 1 || nens > 64 || nf < 1 || nf > RAIN_MAX_FIELDS) return 0;
  return rain_table_blocks(ncol, nens) * nf * nens * RAIN_ROW * 8;
}

extern "C" int mw_member_rain_table(long long ncol, int nens, int nf, const double *const *fields, const int *nt, const double *thresholds,
                                    void *workspace, long long *counts, void *stream) {
  if (!fields || !nt || !thresholds || !workspace || !counts) MW_FAIL("member_rain_table: null pointer");
  if (ncol < 1) MW_FAIL("member_rain_table: ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("member_rain_table: nens must be in [1, 64]");
  if (nf < 1 || nf > RAIN_MAX_FIELDS) MW_FAIL("member_rain_table: nf must be in [1, " + std::to_string(RAIN_MAX_FIELDS) + "]");
  if ((double)ncol * (double)nens > 9.0e18) MW_FAIL("member_rain_table: the fields are too large");
  RainFields R;
  for (int f = 0; f < RAIN_MAX_FIELDS; f++) {
    R.f[f] = nullptr; R.nt[f] = 0;
    for (int j = 0; j < RAIN_MAX_THR; j++) R.thr[f][j] = 0.0;
  }
  for (int f = 0; f < nf; f++) {
    if (!fields[f]) MW_FAIL("member_rain_table: null field");
    if (nt[f] < 1 || nt[f] > RAIN_MAX_THR) MW_FAIL("member_rain_table: a field has 1 to " + std::to_string(RAIN_MAX_THR) + " thresholds, field " +
                                                   std::to_string(f) + " has " + std::to_string(nt[f]));
    R.f[f] = fields[f]; R.nt[f] = nt[f];
    for (int j = 0; j < nt[f]; j++) {
      const double thr = thresholds[f * RAIN_MAX_THR + j];
      if (thr - thr != 0.0) MW_FAIL("member_rain_table: threshold " + std::to_string(j) + " of field " + std::to_string(f) + " is not finite");
      if (j > 0 && !(thr > R.thr[f][j - 1])) MW_FAIL("member_rain_table: the thresholds of field " + std::to_string(f) + " are not strictly ascending");
      R.thr[f][j] = thr;
    }
  }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = rain_table_blocks(ncol, nens);
  hipLaunchKernelGGL(k_member_rain_table, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, st, ncol, nens, R, (long long *)workspace);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_member_rain_table_final, dim3((unsigned)((nf * RAIN_MAX_THR * nens + 255) / 256)), dim3(256), 0, st, (int)blocks, nf, nens, R,
                     (const long long *)workspace, counts);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_member_domain(int nz, long long ncol, int nens, int nm, const int *members, const double *box, const double *const *in5,
                                long long *counts, unsigned char *flags, const int *slots, long long *flag_counts, void *stream) {
  if (!in5 || !counts || !box || !members) MW_FAIL("member_domain: null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL("member_domain: nz and ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("member_domain: nens must be in [1, 64]");
  if (nm < 1 || nm > DOMAIN_MAX_MEMBERS) MW_FAIL("member_domain: nm must be in [1, " + std::to_string(DOMAIN_MAX_MEMBERS) + "]");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18 || (double)ncol * (double)nens > 64.0 * 2147483647.0)
    MW_FAIL("member_domain: the fields are too large");
  DomainArgs A;
  for (int e = 0; e < 64; e++) A.listed_at[e] = -1;
  for (int j = 0; j < DOMAIN_MAX_MEMBERS; j++) {
    A.slot[j] = -1;
    for (int f = 0; f < 5; f++) { A.box[j][f][0] = -__builtin_inf(); A.box[j][f][1] = __builtin_inf(); }
  }
  for (int j = 0; j < nm; j++) {
    const int e = members[j];
    if (e < 0 || e >= nens) MW_FAIL("member_domain: member " + std::to_string(e) + " is outside [0, " + std::to_string(nens) + ")");
    if (A.listed_at[e] >= 0) MW_FAIL("member_domain: member " + std::to_string(e) + " is listed twice");
    A.listed_at[e] = (signed char)j;
    for (int f = 0; f < 5; f++) {
      const double lo = box[(j * 5 + f) * 2], hi = box[(j * 5 + f) * 2 + 1];
      if (!(lo <= hi)) MW_FAIL("member_domain: the box of member " + std::to_string(e) + ", field " + std::to_string(f) +
                               ", is not lo <= hi (NaN is refused, +-inf is allowed)");
      A.box[j][f][0] = lo; A.box[j][f][1] = hi;
    }
    if (slots && slots[j] >= 0) {
      if (!flags || !flag_counts) MW_FAIL("member_domain: member " + std::to_string(e) + " has a slot, but flags or flag_counts is null");
      A.slot[j] = slots[j];
    }
  }
  for (int f = 0; f < 5; f++) { if (!in5[f]) MW_FAIL("member_domain: null field"); A.in[f] = in5[f]; }
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long plane = ncol * nens;
  MW_HIP(hipMemsetAsync(counts, 0, (size_t)nm * DOMAIN_WORDS * 8, st));     // counts is SET: the adds start from zero
  hipLaunchKernelGGL(k_member_domain, dim3((unsigned)((plane + 63) / 64)), dim3(256), 0, st, nz, plane, nens, nm, A, (unsigned long long *)counts,
                     flags, (unsigned long long *)flag_counts);
  MW_LAUNCH_CHECK();
  return 0;
}
