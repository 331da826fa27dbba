// =====================================================================================================
// mw_member_sample.hip -- DataGenerator's sampler (k_sample_mask / k_gather_samples of mw_output.hip, which see member 0 only) on the
// member layout, between a member's own state and its Kessler teacher values: mw_member_sample_mask / mw_member_gather_samples
// (DESIGN.md 13.4), and mw_member_sample_mask_domain, the sampler with a third class, the cells outside the member's training box, and
// the counts of every class that fix its rate (13.11).  No reference counterpart.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_member.h"
#include "mw_sample_key.h"
#include <algorithm>

namespace mw {

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
  if (member_bits("member_sample_mask", "members", nens, nm, members, &listed)) return 1;
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
  if (!member_counts_fit((double)nz * (double)ncol * (double)nens, 256.0)) MW_FAIL("member_sample_mask_domain: the fields are too large");
  SampleDomainArgs A;
  for (int v = 0; v < 5; v++) A.in[v] = f.in[v];
  for (int v = 0; v < 4; v++) A.teach[v] = f.teach[v];
  if (member_boxes("member_sample_mask_domain", nens, nm, members, box, A.listed_at, A.box)) return 1;
  A.above = 0u;
  for (int j = 0; j < DOMAIN_MAX_MEMBERS; j++)
    for (int c = 0; c < SAMPLE_CLASSES; c++) A.thr[j][c] = 0.0;
  for (int j = 0; j < nm; j++) {
    for (int c = 0; c < SAMPLE_CLASSES; c++) {
      const double x = thr[j * SAMPLE_CLASSES + c];
      if (!(x >= 0.0 && x <= 1.0)) MW_FAIL("member_sample_mask_domain: threshold " + std::to_string(c) + " of member " + std::to_string(members[j]) +
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
