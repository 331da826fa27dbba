// =====================================================================================================
// mw_member_guard.hip -- the two four-wavefront, level-split kernels that write the flag bytes of the guarded committee's Kessler pass
// (no reference counterpart).  mw_committee_guard_flags: which columns of a member go to Kessler because its models disagree
// (DESIGN.md 13.7).  mw_member_domain: the cells of the listed members outside the box their models were trained in, counted, and
// their columns flagged (13.10).
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_member.h"

namespace mw {

// ---- mw_committee_guard_flags -------------------------------------------------------------------------------------------------------
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

// ---- mw_member_domain ---------------------------------------------------------------------------------------------------------------
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

} // namespace mw

using namespace mw;

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

extern "C" int mw_member_domain(int nz, long long ncol, int nens, int nm, const int *members, const double *box, const double *const *in5,
                                long long *counts, unsigned char *flags, const int *slots, long long *flag_counts, void *stream) {
  if (!in5 || !counts || !box || !members) MW_FAIL("member_domain: null pointer");
  if (nz < 1 || ncol < 1) MW_FAIL("member_domain: nz and ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("member_domain: nens must be in [1, 64]");
  if (nm < 1 || nm > DOMAIN_MAX_MEMBERS) MW_FAIL("member_domain: nm must be in [1, " + std::to_string(DOMAIN_MAX_MEMBERS) + "]");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18 || !member_counts_fit((double)ncol * (double)nens, 64.0))
    MW_FAIL("member_domain: the fields are too large");
  DomainArgs A;
  if (member_boxes("member_domain", nens, nm, members, box, A.listed_at, A.box)) return 1;
  for (int j = 0; j < DOMAIN_MAX_MEMBERS; j++) A.slot[j] = -1;
  for (int j = 0; j < nm; j++) {
    if (slots && slots[j] >= 0) {
      if (!flags || !flag_counts) MW_FAIL("member_domain: member " + std::to_string(members[j]) + " has a slot, but flags or flag_counts is null");
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
