// =====================================================================================================
// mw_stack_members.hip -- a GROUP of dense surrogate stacks (mw_mlp_stack.h) rolled out as ensemble members: stack j replaces temp and the
// three water fields of member members[j] of the coupler's member-fastest arrays (cell c, member e at c * nens + e) IN PLACE, from that
// member's own values (mw_stack_group_members_apply; mw_surrogate_members_apply's semantics for stacks of any shape).  DESIGN.md 13.20.
//
// The group packs, at creation, its stacks' MFMA images (each followed by MW_STACK_PAD zero floats), their StackP rows and their
// parameters as they came into device buffers of its own; a call allocates and copies nothing.  The stacks are held as two lists, n_in = 5
// and n_in = 9, each in the order given: the two walks differ (flat tiles of 16 cells; 16 columns top-down), so a call launches one kernel
// per list that is not empty.
//
// k_stack_members: the waves of a 256-thread workgroup are dealt to (stack, tile slot) as apply_slot does in mw_surrogate_bank.hip -- mpb
// = 4, 2 or 1 consecutive stacks of the list per workgroup, 4 / mpb tile slots -- so that the waves of a workgroup work on the SAME cells
// of neighbouring members: a line of the member-fastest array fetched for one stack is a cache hit for the others.  mpb is the largest for
// which the images (+ pad) of every workgroup's stacks fit MW_STACK_GROUP_LDS bytes of dynamic LDS together.  A wave reads its StackP row
// wave-uniformly from the device table and its image from LDS; the one barrier is behind the LDS fill.
// A cell's arithmetic is k_mlp_stack's, expression for expression (net_scaled, stack_dense's bias-then-ki order, leaky_slope, the
// un-scaling, net5_rotate_base, the clip) under the same contraction setting: a member holds the bits mw_mlp_stack_forward stores for it.
//   n_in = 5: k_mlp_stack's tiles at address cell * nens + e; a tile is loaded whole before its MFMAs, so in place is safe.
//   n_in = 9: a wave owns 16 columns of one member and walks them top-down, four consecutive levels per pass (the four tiles of a pass, so
//     one LDS read of an A operand still feeds four MFMAs).  All loads of a pass precede its stores.  The level above tile u is tile
//     u - 1's RAW values, already in registers; above the pass's top tile: carried raw from the pass before; the model top is its own
//     level above.  Carried values are scaled where they are used.  Lane group 1 holds density_dry but needs temp of the level above: it
//     takes temp of its level from group 0 by a lane move (no second load) and carries it.  Nobody else reads a member's columns, so no
//     level is copied and nothing is refused for overlap.
//   tendency form: the base of groups 1..3 by the rotate of the level's own values, which are loaded before its stores.
// k_stack_members_strict (mw_mlp_set_strict(1)): thread = one column of one member, grid.y = stack, top-down with the level above as it
// was in registers, k_mlp_stack_strict's index-order loops on the parameters as they came.
// =====================================================================================================
#include "mw_mlp_stack.h"
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace mw {

struct StackFields { double *f[5]; };                               // temp, density_dry, water_vapor, cloud_liquid, precip_liquid (density_dry is only read)

constexpr int SM_TILES = 4;
constexpr long long SM_MAX_BLOCKS = 256 * 8;                        // grid.x: grid-stride beyond 8 blocks per CU (every block fills its LDS once)

// rows: the list's rows (n_in = 5 or 9 alone), `models` of them; map.member[j]: the member of row j.  ANYT: the list holds a stack of the
// tendency form (then a wave's form picks the epilogue, wave-uniformly).
template <bool N9, bool ANYT>
__global__ __launch_bounds__(256, 2) void k_stack_members(const StackRow *__restrict__ rows, const float *__restrict__ imgs, int models, int mpb,
                                                       StackMap map, int nz, long long ncol, int nens, StackFields F) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int m0 = blockIdx.y * mpb, cnt = min(mpb, models - m0);
  const int lo = rows[m0].img_off, hi = rows[m0 + cnt - 1].img_off + rows[m0 + cnt - 1].P.nimg + MW_STACK_PAD;
  for (int i = threadIdx.x; i < hi - lo; i += 256) lds[i] = imgs[lo + i];
  __syncthreads();
  const int wv = threadIdx.x >> 6, lg = mpb >> 1;                         // mpb = 1, 2, 4: its logarithm
  const int slots = 4 >> lg, slot = __builtin_amdgcn_readfirstlane(wv >> lg);
  const int j = __builtin_amdgcn_readfirstlane(m0 + (wv & (mpb - 1)));
  if (j >= models) return;                                                // (wave-uniform, after the barrier)
  const StackRow *R = rows + j;
  const StackP *P = &R->P;
  const float *img = lds + (R->img_off - lo);
  const bool tend = ANYT && R->form != MW_FORM_STATE;
  const int e = map.member[j];
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const double *in_g = F.f[g], *rho_r = F.f[4];
  double *out_g = F.f[g == 0 ? 0 : g + 1];
  const int f1 = (N9 || g == 0) ? 4 + g : 4;
  StackLane S;
  S.imin0 = P->in_min[g]; S.irng0 = 1.0 / P->in_rng[g]; S.imin1 = P->in_min[f1]; S.irng1 = 1.0 / P->in_rng[f1];
  S.imin2 = N9 ? P->in_min[8] : 0.0; S.irng2 = N9 ? 1.0 / P->in_rng[8] : 1.0;
  S.omin = P->out_min[g]; S.orng = P->out_rng[g];
  constexpr int TILES = SM_TILES;
  if (!N9) {
    const long long ncells = (long long)nz * ncol;
    const long long ntiles = (ncells + 15) / 16;
    for (long long t0 = ((long long)blockIdx.x * slots + slot) * TILES; t0 < ntiles; t0 += (long long)gridDim.x * slots * TILES) {
      double x0[TILES], x1[TILES], x2[TILES], y[TILES];
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const long long cell = (t0 + u) * 16 + cidx;
        const bool ok = cell < ncells;
        x0[u] = ok ? in_g[cell * nens + e] : S.imin0;
        x1[u] = (ok && g == 0) ? rho_r[cell * nens + e] : S.imin1;
        x2[u] = S.imin2;
      }
      stack_cells<TILES, false>(y, P, img, S, tend, lane, g, x0, x1, x2);
#pragma unroll
      for (int u = 0; u < TILES; u++) {
        const long long cell = (t0 + u) * 16 + cidx;
        if (cell < ncells) out_g[cell * nens + e] = y[u];
      }
    }
  } else {
    const int ntiles = (int)((ncol + 15) / 16);                           // (the host refuses more column tiles than an int holds)
    const long long lev = ncol * nens;                                    // doubles from level k to level k + 1
    for (int t = blockIdx.x * slots + slot; t < ntiles; t += gridDim.x * slots) {
      const long long col = (long long)t * 16 + cidx;
      const bool ok = col < ncol;
      const long long top = (long long)(nz - 1) * lev + (col * (unsigned)nens + (unsigned)e);      // the column's top level in this member
      const double *pg = in_g + top, *pr = rho_r + top;                   // per lane, walking down by lev per level (never read below level 0)
      double *po = out_g + top;
      double carry = 0.0;                                                 // raw, of the pass before's lowest level: what this lane's feature 4 + g (group 0: 8) is one level down
      for (int k0 = nz - 1; k0 >= 0; k0 -= TILES, pg -= TILES * lev, pr -= TILES * lev, po -= TILES * lev) {
        double x0[TILES], xr[TILES], c[TILES], x1[TILES], x2[TILES], y[TILES];
#pragma unroll
        for (int u = 0; u < TILES; u++) {                                 // tile u: level k0 - u
          const int k = k0 - u;
          const bool lv = ok && k >= 0;
          x0[u] = lv ? pg[-u * lev] : S.imin0;
          xr[u] = (lv && g == 0) ? pr[-u * lev] : S.imin1;
        }
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const double t0 = __shfl(x0[u], (lane + 48) & 63, 64);          // group 1: temp of its level from group 0 (lane - 16)
          c[u] = g == 0 ? xr[u] : g == 1 ? t0 : x0[u];
        }
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const double above = u == 0 ? (k0 == nz - 1 ? c[0] : carry) : c[u > 0 ? u - 1 : 0];      // the model top is its own level above
          x1[u] = g == 0 ? xr[u] : above;
          x2[u] = g == 0 ? above : S.imin2;
        }
        carry = c[TILES - 1];
        stack_cells<TILES, true>(y, P, img, S, tend, lane, g, x0, x1, x2);
#pragma unroll
        for (int u = 0; u < TILES; u++) {
          const int k = k0 - u;
          if (ok && k >= 0) po[-u * lev] = y[u];
        }
      }
    }
  }
}

// STRICT form: thread = one column of one member, grid row y = one stack of the group (any n_in), swept top-down with temp, rho_v,
// rho_c, rho_r of the level above AS THEY WERE in registers; k_mlp_stack_strict's expressions on the parameters as they came.
__global__ __launch_bounds__(256) void k_stack_members_strict(const StackRow *__restrict__ rows, const float *__restrict__ params, StackMap map, int nz,
                                                              long long ncol, int nens, StackFields F) {
#pragma clang fp contract(off)
  const StackRow *R = rows + blockIdx.y;
  const StackP &P = R->P;
  const float *par = params + R->par_off;
  const bool tend = R->form != MW_FORM_STATE;
  const int e = map.member[blockIdx.y];
  const long long lev = ncol * nens;
  for (long long col = (long long)blockIdx.x * 256 + threadIdx.x; col < ncol; col += (long long)gridDim.x * 256) {
    const long long at = col * nens + e;
    double ab[4];
    for (int k = nz - 1; k >= 0; k--) {
      const long long c = (long long)k * lev + at;
      double in[9] = {F.f[0][c], F.f[1][c], F.f[2][c], F.f[3][c], F.f[4][c], 0.0, 0.0, 0.0, 0.0};
      if (k == nz - 1) { ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4]; }      // the column's top level is its own level above
      in[5] = ab[0]; in[6] = ab[1]; in[7] = ab[2]; in[8] = ab[3];
      ab[0] = in[0]; ab[1] = in[2]; ab[2] = in[3]; ab[3] = in[4];
      float x[MW_STACK_MAX_WIDTH], h[MW_STACK_MAX_WIDTH];
      for (int i = 0; i < P.n_in; i++) x[i] = (float)((in[i] - P.in_min[i]) / P.in_rng[i]);
      for (int l = 0; l < P.nl; l++) {
        const int n = P.width[l], no = P.width[l + 1];
        const float *W = par + P.woff[l], *b = par + P.bwoff[l];
        for (int o = 0; o < no; o++) {
          float acc = 0.f;
          for (int i = 0; i < n; i++) acc += x[i] * W[i * no + o];
          acc = acc + b[o];
          h[o] = (l < P.nl - 1) ? (acc > 0.f ? acc : P.slope[l] * acc) : acc;
        }
        for (int o = 0; o < no; o++) x[o] = h[o];
      }
      if (tend) {
        F.f[0][c] =           in[0] + (x[0] * P.out_rng[0] + P.out_min[0]);
        F.f[2][c] = fmax(0.0, in[2] + (x[1] * P.out_rng[1] + P.out_min[1]));
        F.f[3][c] = fmax(0.0, in[3] + (x[2] * P.out_rng[2] + P.out_min[2]));
        F.f[4][c] = fmax(0.0, in[4] + (x[3] * P.out_rng[3] + P.out_min[3]));
      } else {
        F.f[0][c] =           x[0] * P.out_rng[0] + P.out_min[0];
        F.f[2][c] = fmax(0.0, x[1] * P.out_rng[1] + P.out_min[1]);
        F.f[3][c] = fmax(0.0, x[2] * P.out_rng[2] + P.out_min[2]);
        F.f[4][c] = fmax(0.0, x[3] * P.out_rng[3] + P.out_min[3]);
      }
    }
  }
}

} // namespace mw

using namespace mw;

extern "C" void mw_stack_group_destroy(mw_stack_group_t g) {
  if (!g) return;
  (void)hipFree(g->rows); (void)hipFree(g->imgs); (void)hipFree(g->params);
  delete g;
}

extern "C" int mw_stack_group_create(mw_stack_group_t *out, int n, const mw_mlp_stack_t *stacks) {
  if (!out) MW_FAIL("stack_group_create: null pointer");
  *out = nullptr;
  if (n < 1 || n > MW_STACK_GROUP_MAX) MW_FAIL("stack_group_create: a group holds 1 to " + std::to_string(MW_STACK_GROUP_MAX) + " stacks, got " + std::to_string(n));
  if (!stacks) MW_FAIL("stack_group_create: null pointer");
  for (int j = 0; j < n; j++) if (!stacks[j]) MW_FAIL("stack_group_create: stack " + std::to_string(j) + " is a null handle");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  mw_stack_group_t g = new mw_stack_group_s();
  g->n = n; g->rows = nullptr; g->imgs = nullptr; g->params = nullptr; g->any_tendency = false;
  std::vector<StackRow> rows;
  std::vector<int> src;                                                   // the stack of a row
  for (int pass = 0; pass < 2; pass++) {
    StackList &L = g->list[pass];
    L.r0 = (int)rows.size(); L.anyt = false;
    for (int j = 0; j < n; j++) {
      if ((stacks[j]->P.n_in == 9) != (pass == 1)) continue;
      StackRow R;
      memset(&R, 0, sizeof(R));
      R.P = stacks[j]->P; R.form = stacks[j]->form;
      L.anyt = L.anyt || R.form != MW_FORM_STATE;
      g->row_of[j] = (int)rows.size();
      rows.push_back(R); src.push_back(j);
    }
    L.n = (int)rows.size() - L.r0;
    g->any_tendency = g->any_tendency || L.anyt;
  }
  size_t nimg = 0, npar = 0;
  for (StackRow &R : rows) {
    R.img_off = (int)nimg; R.par_off = (int)npar;
    g->form_of[&R - rows.data()] = R.form; g->nimg_of[&R - rows.data()] = R.P.nimg;
    nimg += (size_t)R.P.nimg + MW_STACK_PAD;
    npar += (size_t)(R.P.bwoff[R.P.nl - 1] + 4);
  }
  for (int pass = 0; pass < 2; pass++) {
    stack_list_plan(g->list[pass], rows);
    g->elist[pass] = g->list[pass];
    stack_list_plan(g->elist[pass], rows, MW_STACK_GROUP_LDS - MW_STACK_EVAL_RED);
  }
  hipError_t e = hipMalloc(&g->rows, sizeof(StackRow) * rows.size());
  if (e == hipSuccess) e = hipMalloc(&g->imgs, sizeof(float) * nimg);
  if (e == hipSuccess) e = hipMalloc(&g->params, sizeof(float) * npar);
  if (e == hipSuccess) e = hipMemset(g->imgs, 0, sizeof(float) * nimg);      // the pads
  if (e == hipSuccess) e = hipMemcpy(g->rows, rows.data(), sizeof(StackRow) * rows.size(), hipMemcpyHostToDevice);
  for (size_t r = 0; r < rows.size() && e == hipSuccess; r++) {
    const mw_mlp_stack_t s = stacks[src[r]];
    e = hipMemcpy(g->imgs + rows[r].img_off, s->img, sizeof(float) * (size_t)rows[r].P.nimg, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(g->params + rows[r].par_off, s->params, sizeof(float) * (size_t)(rows[r].P.bwoff[rows[r].P.nl - 1] + 4), hipMemcpyDeviceToDevice);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { mw_stack_group_destroy(g); MW_FAIL(std::string("stack_group_create: ") + hipGetErrorString(e)); }
  *out = g;
  return 0;
}

extern "C" int mw_stack_group_members_apply(mw_stack_group_t g, const int *members, int nz, long long ncol, int nens, double *const *fields5, void *stream) {
  if (!g) MW_FAIL("stack_group_members_apply: null handle");
  if (!members || !fields5) MW_FAIL("stack_group_members_apply: null pointer");
  if (nz < 1 || ncol < 1 || nens < 1) MW_FAIL("stack_group_members_apply: nz, ncol and nens must be >= 1");
  StackMap map;                                                           // by row
  memset(&map, 0, sizeof(map));
  for (int j = 0; j < g->n; j++) {
    if (members[j] < 0 || members[j] >= nens) MW_FAIL("stack_group_members_apply: member " + std::to_string(members[j]) + " of stack " + std::to_string(j) +
                                                      " is outside [0, " + std::to_string(nens) + ")");
    for (int i = 0; i < j; i++) if (members[i] == members[j]) MW_FAIL("stack_group_members_apply: member " + std::to_string(members[j]) + " is given to two stacks");
    map.member[g->row_of[j]] = members[j];
  }
  StackFields F;
  for (int i = 0; i < 5; i++) { if (!fields5[i]) MW_FAIL("stack_group_members_apply: null field"); F.f[i] = fields5[i]; }
  if ((double)nz * (double)ncol * (double)nens > 9.0e18 || (ncol + 15) / 16 > 0x7fffffffll - 4 * SM_MAX_BLOCKS)      // (the stencil walk counts column tiles in an int)
    MW_FAIL("stack_group_members_apply: the fields are too large");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  hipStream_t st = (hipStream_t)stream;
  if (mlp_strict()) {
    const long long blocks = std::max<long long>(1, std::min<long long>((ncol + 255) / 256, SM_MAX_BLOCKS));
    hipLaunchKernelGGL(k_stack_members_strict, dim3((unsigned)blocks, (unsigned)g->n), dim3(256), 0, st, g->rows, g->params, map, nz, ncol, nens, F);
    MW_LAUNCH_CHECK();
    return 0;
  }
  const long long ncells = (long long)nz * ncol;
  for (int pass = 0; pass < 2; pass++) {
    const StackList &L = g->list[pass];
    if (L.n < 1) continue;
    if (L.lds > MW_STACK_GROUP_LDS) MW_FAIL("stack_group_members_apply: a stack's image exceeds the kernel's LDS");      // (no shape mw_mlp_stack_create accepts does)
    const int slots = 4 / L.mpb;
    const long long items = pass == 0 ? ((ncells + 15) / 16 + SM_TILES - 1) / SM_TILES : (ncol + 15) / 16;      // tile groups / column tiles
    const long long blocks = std::max<long long>(1, std::min<long long>((items + slots - 1) / slots, SM_MAX_BLOCKS));
    const dim3 grid((unsigned)blocks, (unsigned)((L.n + L.mpb - 1) / L.mpb));
    StackMap lm;                                                          // the list's own rows first
    memset(&lm, 0, sizeof(lm));
    for (int j = 0; j < L.n; j++) lm.member[j] = map.member[L.r0 + j];
    if (pass == 0) MW_LAUNCH_IF(L.anyt, (k_stack_members<false, true>), (k_stack_members<false, false>), grid, dim3(256), L.lds, st, g->rows + L.r0, g->imgs, L.n, L.mpb, lm, nz, ncol, nens, F);
    else           MW_LAUNCH_IF(L.anyt, (k_stack_members<true, true>), (k_stack_members<true, false>), grid, dim3(256), L.lds, st, g->rows + L.r0, g->imgs, L.n, L.mpb, lm, nz, ncol, nens, F);
    MW_LAUNCH_CHECK();
  }
  return 0;
}
