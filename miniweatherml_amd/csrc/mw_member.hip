// =====================================================================================================
// mw_member.hip -- the plumbing and the scores of the coupler's member-fastest arrays (cell c, ensemble member e at c * nens + e; no
// reference counterpart: the reference's ensemble members never meet).  One member out to contiguous arrays and back (mw_member_extract /
// mw_member_insert: the rollout's Kessler member is stepped alone), the listed members from one set of arrays to another (mw_members_copy:
// the guarded committee's commit), how far every member has moved from member 0 (mw_member_divergence, 13.3) and every
// member's rain contingency table against member 0 (mw_member_rain_table, 13.8).  The other member units: DESIGN.md 13.17.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_member.h"
#include <algorithm>

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

// thread = flat element t = cell * nens + e, grid row y = field: the listed members' elements from src to dst
__global__ __launch_bounds__(256) void k_members_copy(long long total, int nens, unsigned long long listed, MemberFields src, MemberFields dst) {
  const double *a = src.f[blockIdx.y];
  double *b = dst.f[blockIdx.y];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256)
    if ((listed >> (int)(t % nens)) & 1ull) b[t] = a[t];
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

// grid.x of the C = 256 / nens lane layout: a block per C cells, capped (the kernels stride)
static long long member_lane_blocks(long long n, int nens, int cap) {
  const long long C = 256 / nens;
  return std::max<long long>(1, std::min<long long>((n + C - 1) / C, cap));
}

// nf fields of `a` (and of `b`, unless B is null) into kernel arguments
static int member_fields(const char *who, int nf, double *const *a, double *const *b, MemberFields *A, MemberFields *B) {
  for (int f = 0; f < MW_MAX_TRACERS; f++) { A->f[f] = nullptr; if (B) B->f[f] = nullptr; }
  for (int f = 0; f < nf; f++) {
    if (!a[f] || (B && !b[f])) MW_FAIL(std::string(who) + ": null field");
    A->f[f] = a[f];
    if (B) B->f[f] = b[f];
  }
  return 0;
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
  if (member_fields(who, nf, fused, flat, &A, &B)) return 1;
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

extern "C" int mw_members_copy(long long n, int nens, int nm, const int *members, int nf, const double *const *src, double *const *dst,
                               void *stream) {
  if (!members || !src || !dst) MW_FAIL("members_copy: null pointer");
  if (n < 1) MW_FAIL("members_copy: n must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("members_copy: nens must be in [1, 64]");
  if (nm < 1 || nm > nens) MW_FAIL("members_copy: nm must be in [1, nens]");
  if (nf < 1 || nf > MW_MAX_TRACERS) MW_FAIL("members_copy: nf must be in [1, " + std::to_string(MW_MAX_TRACERS) + "]");
  if ((double)n * (double)nens > 9.0e18) MW_FAIL("members_copy: the fields are too large");
  unsigned long long listed = 0;
  if (member_bits("members_copy", "members", nens, nm, members, &listed)) return 1;
  MemberFields A, B;
  if (member_fields("members_copy", nf, (double *const *)src, dst, &A, &B)) return 1;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long total = n * nens;
  const long long blocks = std::max<long long>(1, std::min<long long>((total + 255) / 256, 256 * 16));
  hipLaunchKernelGGL(k_members_copy, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, (hipStream_t)stream, total, nens, listed, A, B);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" long long mw_member_divergence_workspace_bytes(long long n, int nens, int nf) {
  if (n < 1 || nens < 1 || nens > 256 || nf < 1 || nf > MW_MAX_TRACERS) return 0;
  return member_lane_blocks(n, nens, DIV_MAX_BLOCKS) * nf * nens * DIV_ROW * 8;
}

extern "C" int mw_member_divergence(long long n, int nens, int nf, const double *const *fields, void *workspace, double *out,
                                    long long *nonfinite, void *stream) {
  if (!fields || !workspace || !out || !nonfinite) MW_FAIL("member_divergence: null pointer");
  if (n < 1) MW_FAIL("member_divergence: n must be >= 1");
  if (nens < 1 || nens > 256) MW_FAIL("member_divergence: nens must be in [1, 256]");
  if (nf < 1 || nf > MW_MAX_TRACERS) MW_FAIL("member_divergence: nf must be in [1, " + std::to_string(MW_MAX_TRACERS) + "]");
  MemberFields F;
  if (member_fields("member_divergence", nf, (double *const *)fields, nullptr, &F, nullptr)) return 1;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = member_lane_blocks(n, nens, DIV_MAX_BLOCKS);
  hipLaunchKernelGGL(k_member_divergence, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, st, n, nens, F, (double *)workspace);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_member_divergence_final, dim3((unsigned)((nf * nens * DIV_ROW + 255) / 256)), dim3(256), 0, st, (int)blocks, nf, nens,
                     (const double *)workspace, out, nonfinite);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" long long mw_member_rain_table_workspace_bytes(long long ncol, int nens, int nf) {
  if (ncol < 1 || nens < 1 || nens > 64 || nf < 1 || nf > RAIN_MAX_FIELDS) return 0;
  return member_lane_blocks(ncol, nens, RAIN_MAX_BLOCKS) * nf * nens * RAIN_ROW * 8;
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
  const long long blocks = member_lane_blocks(ncol, nens, RAIN_MAX_BLOCKS);
  hipLaunchKernelGGL(k_member_rain_table, dim3((unsigned)blocks, (unsigned)nf), dim3(256), 0, st, ncol, nens, R, (long long *)workspace);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_member_rain_table_final, dim3((unsigned)((nf * RAIN_MAX_THR * nens + 255) / 256)), dim3(256), 0, st, (int)blocks, nf, nens, R,
                     (const long long *)workspace, counts);
  MW_LAUNCH_CHECK();
  return 0;
}
