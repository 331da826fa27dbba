// =====================================================================================================
// mw_member_heat.hip -- the latent-heat closure of the rollout's members (no reference counterpart).  In a Kessler step the
// only thing that changes a cell's temp is the vapour that leaves or enters it, so temp_after - temp_before = (lv / cp_d) *
// (rho_v_before - rho_v_after) / rho_d in every cell.  mw_member_heat_closure measures how far a member's step is from that (the residual,
// K, and the spurious heating of a column, W / m^2) and, for the members listed as closed, makes temp the diagnosed quantity of the member's
// own vapour change.  One of the five member units: the list parser, the scalar checks and the block-row reduction
// are mw_member.h's, shared with the water fixer.
// =====================================================================================================
#include "../../include/mw_cdna4.h"
#include "mw_member.h"

namespace mw {

struct HeatFields { double *temp; const double *rho_d, *rho_v, *temp_b, *rho_v_b; };
constexpr int HEAT_AHEAD = 4;              // levels whose loads are issued ahead of their arithmetic
constexpr int HEAT_COUNTS = 2;             // per block and member: closed cells, skipped cells (int64 bits), then
constexpr int HEAT_STATS = 6;              // sum r, sum |r|, sum r^2, max |r|, sum H, max |H|
constexpr unsigned HEAT_MAX = (1u << 3) | (1u << 5);      // (statistics 3 and 5 are maxima)

// one cell of a diagnosed lane; every operation is rounded once (contraction is off), so numpy restates it bit for bit
struct HeatLane {
  double sr, sa, s2, mx, h;
  int nclosed, nskipped;
};

__device__ __forceinline__ void heat_cell(HeatLane &q, double C, double tolerance, bool closes, double ta, double rd, double rva, double tb,
                                          double rvb, double *__restrict__ temp_at) {
#pragma clang fp contract(off)
  const double tc = tb + C * ((rvb - rva) / rd);
  const double r = ta - tc;
  if (r - r != 0.0) {                                                          // NaN or inf in any of the five, or rho_d == 0: skipped
    q.nskipped++;
    return;
  }
  const double a = fabs(r);
  q.sr = q.sr + r;
  q.sa = q.sa + a;
  q.s2 = q.s2 + r * r;
  q.mx = a > q.mx ? a : q.mx;
  q.h = q.h + rd * r;
  if (closes && a > tolerance) {
    *temp_at = tc;
    q.nclosed++;
  }
}

// k_member_surface_rain's mapping: thread t is one (column, member) of the plane, so a wavefront's loads of a level are 64 consecutive
// doubles per field whatever nens is; a wavefront with no diagnosed lane takes no load at all (its lanes' branch is empty).  The twenty
// loads of HEAT_AHEAD levels are issued before the first of their cells is worked on; the cells keep the order of k.  A lane's sums start
// from +0.0 and run over k ascending; H = scale * (sum over k of rho_d * r), the scale applied once.  Every lane's numbers go to LDS, and
// the block's rows and k_member_rows_final follow (mw_member.h); a block with no diagnosed lane writes rows of zeros.
__global__ __launch_bounds__(256) void k_member_heat_closure(int nz, long long plane, int nens, unsigned long long listed, unsigned long long closed,
                                                             double tolerance, double C, double scale, HeatFields F,
                                                             double *__restrict__ partial, double *__restrict__ heating) {
#pragma clang fp contract(off)
  __shared__ double red[256][HEAT_STATS];
  __shared__ int cnt[256][2];
  const int l = threadIdx.x;
  const long long t = (long long)blockIdx.x * 256 + l;
  const int e = (int)(t % nens);
  const bool in = t < plane;
  const bool mine = in && ((listed >> e) & 1ull);
  HeatLane q = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0};
  double H = 0.0;
  if (mine) {
    const bool closes = (closed >> e) & 1ull;
    int k = 0;
    for (; k + HEAT_AHEAD <= nz; k += HEAT_AHEAD) {
      double ta[HEAT_AHEAD], rd[HEAT_AHEAD], rva[HEAT_AHEAD], tb[HEAT_AHEAD], rvb[HEAT_AHEAD];
#pragma unroll
      for (int j = 0; j < HEAT_AHEAD; j++) {
        const long long i = (long long)(k + j) * plane + t;
        ta[j] = F.temp[i]; rd[j] = F.rho_d[i]; rva[j] = F.rho_v[i]; tb[j] = F.temp_b[i]; rvb[j] = F.rho_v_b[i];
      }
#pragma unroll
      for (int j = 0; j < HEAT_AHEAD; j++)
        heat_cell(q, C, tolerance, closes, ta[j], rd[j], rva[j], tb[j], rvb[j], F.temp + ((long long)(k + j) * plane + t));
    }
    for (; k < nz; k++) {
      const long long i = (long long)k * plane + t;
      heat_cell(q, C, tolerance, closes, F.temp[i], F.rho_d[i], F.rho_v[i], F.temp_b[i], F.rho_v_b[i], F.temp + i);
    }
    H = scale * q.h;
  }
  if (heating && in) heating[t] = H;
  const double aH = fabs(H);
  red[l][0] = q.sr; red[l][1] = q.sa; red[l][2] = q.s2; red[l][3] = q.mx; red[l][4] = H; red[l][5] = aH;
  cnt[l][0] = q.nclosed; cnt[l][1] = q.nskipped;
  member_rows_fold<HEAT_COUNTS, HEAT_STATS, HEAT_MAX>(nens, mine ? 1 : 0, partial, [&](int j, int s) { return cnt[j][s]; },
                                                      [&](int j, int c) { return red[j][c]; });
}

} // namespace mw

using namespace mw;

extern "C" long long mw_member_heat_closure_workspace_bytes(long long ncol, int nens) {
  if (ncol < 1 || nens < 1 || nens > 64 || !member_counts_fit((double)ncol * (double)nens, 256.0)) return 0;
  return member_plane_blocks(ncol, nens) * nens * (HEAT_COUNTS + HEAT_STATS) * 8;
}

extern "C" int mw_member_heat_closure(int nz, long long ncol, int nens, int nm, const int *members, int nclosed, const int *closed,
                                      double tolerance, double lv, double cp_d, double dz, double dt, double *temp, const double *rho_d,
                                      const double *rho_v, const double *const *before2, void *workspace, long long *counts, double *stats,
                                      double *heating, void *stream) {
  if (nz < 1 || ncol < 1) MW_FAIL("member_heat_closure: nz and ncol must be >= 1");
  if (nens < 1 || nens > 64) MW_FAIL("member_heat_closure: nens must be in [1, 64]");
  if ((double)nz * (double)ncol * (double)nens > 9.0e18) MW_FAIL("member_heat_closure: the fields are too large");
  if (!positive_finite(dz)) MW_FAIL("member_heat_closure: dz must be positive and finite");
  if (!positive_finite(dt)) MW_FAIL("member_heat_closure: dt must be positive and finite");
  if (!finite_nonnegative(tolerance)) MW_FAIL("member_heat_closure: tolerance must be finite and >= 0");
  if (!positive_finite(lv) || !positive_finite(cp_d)) MW_FAIL("member_heat_closure: lv and cp_d must be positive and finite");
  unsigned long long listed = 0, closes = 0;
  if (member_bits("member_heat_closure", "members", nens, nm, members, &listed)) return 1;
  if (member_bits("member_heat_closure", "closed", nens, nclosed, closed, &closes)) return 1;
  if (member_subset("member_heat_closure", "closed", "members", closes, listed, nens)) return 1;
  if (!temp || !rho_d || !rho_v || !before2 || !workspace || !counts || !stats) MW_FAIL("member_heat_closure: null pointer");
  if (!before2[0] || !before2[1]) MW_FAIL("member_heat_closure: null field");
  if (temp == rho_d || temp == rho_v || temp == before2[0] || temp == before2[1]) MW_FAIL("member_heat_closure: temp must not be one of the arrays that are only read");
  if (member_plane_limit("member_heat_closure", ncol, nens)) return 1;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const HeatFields F = {temp, rho_d, rho_v, before2[0], before2[1]};
  hipStream_t st = (hipStream_t)stream;
  const long long plane = ncol * nens, blocks = member_plane_blocks(ncol, nens);
  hipLaunchKernelGGL(k_member_heat_closure, dim3((unsigned)blocks), dim3(256), 0, st, nz, plane, nens, listed, closes, tolerance, lv / cp_d,
                     cp_d * dz / dt, F, (double *)workspace, heating);
  MW_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_member_rows_final<HEAT_COUNTS, HEAT_STATS, HEAT_MAX>), dim3((unsigned)nens), dim3(256), 0, st, blocks, nens,
                     (const double *)workspace, counts, stats);
  MW_LAUNCH_CHECK();
  return 0;
}
