// =====================================================================================================
// mw_member.h -- what the member units (mw_member.hip, mw_member_sample.hip, mw_member_guard.hip, mw_member_water.hip, mw_member_heat.hip;
// map: DESIGN.md 13.17) and mw_kessler.hip's member teacher share.  Host: the one parser of a member list, the subset rule, the scalar
// checks, the 32-bit counter limit and the box rows of the two domain calls.  Device: the two-stage block-row reduction of the water
// fixer and the latent-heat closure.  What a single unit uses stays in that unit.
// =====================================================================================================
#pragma once
#include "mw_common.h"
#include <string>

namespace mw {

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static bool positive_finite(double x) { return x > 0.0 && x - x == 0.0; }
static bool finite_nonnegative(double x) { return x >= 0.0 && x - x == 0.0; }          // (a tolerance)

// the bit set of a member list: distinct indices in [0, nens), nens <= 64.  A caller that needs a member checks its n first.
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

// every member of `sub` is one of `of`: a fixed member is a budget member, a closed member a diagnosed one
static int member_subset(const char *who, const char *sub, const char *of, unsigned long long bits_sub, unsigned long long bits_of, int nens) {
  for (int e = 0; e < nens; e++)
    if (((bits_sub & ~bits_of) >> e) & 1ull) MW_FAIL(std::string(who) + ": member " + std::to_string(e) + " is in " + sub + " but not in " + of);
  return 0;
}

// a block of `lanes` elements counts them in 32-bit LDS words
static bool member_counts_fit(double elements, double lanes) { return elements <= lanes * 2147483647.0; }
static long long member_plane_blocks(long long ncol, int nens) { return (ncol * nens + 255) / 256; }
static int member_plane_limit(const char *who, long long ncol, int nens) {
  if (!member_counts_fit((double)ncol * (double)nens, 256.0)) MW_FAIL(std::string(who) + ": the fields are too large");
  return 0;
}

constexpr int DOMAIN_MAX_MEMBERS = 32;     // the boxes travel in the kernel arguments: 32 x 80 bytes

// the list and the boxes of the two domain calls: listed_at[e] = j for members[j] = e, -1 for every other member; dst[j] = box row j
// ([field][lo, hi], lo <= hi), (-inf, +inf) for the rows past nm
static int member_boxes(const char *who, int nens, int nm, const int *members, const double *box, signed char *listed_at,
                        double (*dst)[5][2]) {
  unsigned long long bits;
  if (member_bits(who, "members", nens, nm, members, &bits)) return 1;
  for (int e = 0; e < 64; e++) listed_at[e] = -1;
  for (int j = 0; j < DOMAIN_MAX_MEMBERS; j++)
    for (int f = 0; f < 5; f++) { dst[j][f][0] = -__builtin_inf(); dst[j][f][1] = __builtin_inf(); }
  for (int j = 0; j < nm; j++) {
    listed_at[members[j]] = (signed char)j;
    for (int f = 0; f < 5; f++) {
      const double lo = box[(j * 5 + f) * 2], hi = box[(j * 5 + f) * 2 + 1];
      if (!(lo <= hi)) MW_FAIL(std::string(who) + ": the box of member " + std::to_string(members[j]) + ", field " + std::to_string(f) +
                               ", is not lo <= hi (NaN is refused, +-inf is allowed)");
      dst[j][f][0] = lo; dst[j][f][1] = hi;
    }
  }
  return 0;
}

// ---- device: the block rows ---------------------------------------------------------------------------------------------------------
// A kernel of one thread per plane element t = col * nens + e leaves, per lane, NCOUNT integers and NSTAT doubles in LDS.  Stage one
// (member_rows_fold, the kernel's last act: it holds the barrier) writes the block's rows partial[block][member][NCOUNT int64 bits |
// NSTAT doubles]: for member m and each number, one thread folds the lanes of m in ascending lane order from `first`, the block's first
// lane of member m; a block where no lane says `any` writes the rows of zeros the fold would give (+0.0 is the int64 0 too).  Stage
// two (k_member_rows_final) is one block per member: thread l folds the rows of the blocks l, l + 256, ... in ascending order, then one
// thread per number folds the 256 partial results in ascending l.  A sum starts from +0.0 (the last from red[0]) and is q + x; a
// maximum (bit c of MAXMASK: statistic c) is x > q ? x : q from +0.0.  No atomics, no memset, no contraction: one fixed order.
template <int NCOUNT, int NSTAT, unsigned MAXMASK, class CountAt, class StatAt>
__device__ __forceinline__ void member_rows_fold(int nens, int any, double *__restrict__ partial, CountAt count_at, StatAt stat_at) {
#pragma clang fp contract(off)
  constexpr int ROW = NCOUNT + NSTAT;
  const int l = threadIdx.x, words = nens * ROW;
  if (!__syncthreads_or(any)) {
    for (int w = l; w < words; w += 256) partial[(long long)blockIdx.x * words + w] = 0.0;
    return;
  }
  const int shift = (int)(((long long)blockIdx.x * 256) % nens);
  for (int w = l; w < words; w += 256) {
    const int m = w / ROW, s = w % ROW;
    const int first = (m - shift + nens) % nens;
    double *row = partial + ((long long)blockIdx.x * nens + m) * ROW;
    if (s < NCOUNT) {
      long long n = 0;
      for (int j = first; j < 256; j += nens) n += count_at(j, s);
      ((long long *)row)[s] = n;
    } else {
      const int c = s - NCOUNT;
      const bool is_max = (MAXMASK >> c) & 1u;
      double q = 0.0;
      for (int j = first; j < 256; j += nens) { const double x = stat_at(j, c); q = is_max ? (x > q ? x : q) : q + x; }
      row[s] = q;
    }
  }
}

// counts (nens, NCOUNT), stats (nens, NSTAT); grid = nens blocks of 256.  A template: each instance is launched from one unit.
template <int NCOUNT, int NSTAT, unsigned MAXMASK>
__global__ __launch_bounds__(256) void k_member_rows_final(long long nblocks, int nens, const double *__restrict__ partial,
                                                           long long *__restrict__ counts, double *__restrict__ stats) {
#pragma clang fp contract(off)
  constexpr int ROW = NCOUNT + NSTAT;
  __shared__ double red[256][NSTAT];
  __shared__ long long cnt[256][NCOUNT];
  const int m = blockIdx.x, l = threadIdx.x;
  long long n[NCOUNT] = {};
  double v[NSTAT] = {};
  for (long long b = l; b < nblocks; b += 256) {
    const double *row = partial + (b * nens + m) * ROW;
#pragma unroll
    for (int s = 0; s < NCOUNT; s++) n[s] += ((const long long *)row)[s];
#pragma unroll
    for (int c = 0; c < NSTAT; c++) v[c] = ((MAXMASK >> c) & 1u) ? (row[NCOUNT + c] > v[c] ? row[NCOUNT + c] : v[c]) : v[c] + row[NCOUNT + c];
  }
#pragma unroll
  for (int s = 0; s < NCOUNT; s++) cnt[l][s] = n[s];
#pragma unroll
  for (int c = 0; c < NSTAT; c++) red[l][c] = v[c];
  __syncthreads();
  if (l < NCOUNT) {
    long long q = 0;
    for (int j = 0; j < 256; j++) q += cnt[j][l];
    counts[m * NCOUNT + l] = q;
  } else if (l < ROW) {
    const int c = l - NCOUNT;
    const bool is_max = (MAXMASK >> c) & 1u;
    double x = red[0][c];
    for (int j = 1; j < 256; j++) x = is_max ? (red[j][c] > x ? red[j][c] : x) : x + red[j][c];
    stats[m * NSTAT + c] = x;
  }
}

} // namespace mw
