// =====================================================================================================
// mw_member.hip -- passes over the coupler's member-fastest arrays (cell c, ensemble member e at c * nens + e) that treat the members
// differently: one member out to contiguous arrays and back (mw_member_extract / mw_member_insert: the rollout's Kessler member is stepped
// alone), and how far every member has moved from member 0 (mw_member_divergence).  No reference counterpart: the reference's ensemble
// members never meet.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_common.h"
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

// the larger / smaller of two values, NaN if either is (mw_mlp.hip: eval_max)
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
