// =====================================================================================================
// mw_mlp_stack.hip -- a dense surrogate stack n_in -> H1 -> ... -> HL -> 4 of any width (1..64) and depth (1..4) on the coupler's fp64
// fields, as one fused MFMA kernel on gfx950: scale (fp64) -> L x (Dense, leaky ReLU with the layer's slope) -> Dense(4) -> un-scale,
// base of the tendency form, clip (fp64).  The scaling, un-scaling and clip are mw_mlp_forward_form's (mw_mlp_net.h: net_scaled, the
// association of net_out / net_out_tendency); the features of n_in = 9 are mw_mlp_stencil_forward's.  DESIGN.md 13.18.
//
// Tile layout (v_mfma_f32_16x16x4_f32, fp32 operands and accumulation): 16 cells on the N axis (column = lane & 15), units on the M axis
// in blocks of 16, the K axis (lane >> 4 = group g) carries four inputs of the layer per MFMA.  MFMA ki of a layer contracts inputs
// 4 ki + g, g = 0..3 -- for the first layer the features (group g loads field g; group 0 also rho_r; n_in = 9: feature 4 + g from
// groups 0..3 and feature 8 from group 0), for every later layer the units of the layer before.
//
// Chaining without lane movement: D holds row 4 g + j in register j of group g.  Unit u of a layer is placed at row
//   rho(u) = 4 (u % 4) + (u % 16) / 4     of unit block u / 16,
// so register j of group g of block m is unit 16 m + 4 j + g = 4 (4 m + j) + g: exactly k-slot g of MFMA ki = 4 m + j of the next layer,
// whose A operand therefore holds W[4 ki + g'][unit at row r] in lane (r, g').  The units fill register 0 of all groups first: a layer
// H_in -> H_out costs ceil(H_in / 4) * ceil(H_out / 16) MFMAs per tile.  Padded units and padded inputs carry zero weights and zero bias.
// The same rule places output n of the last Dense(4) at row 4 n: lane group n holds it in register 0 and stores 16 contiguous doubles.
//
// The A-operand images and the bias rows (C initialisers) are built on the host once per model (stack_images), uploaded once and owned
// by the handle; every workgroup copies them to LDS once and then walks tiles grid-stride, TILES 16-cell tiles per wave at a time, so
// that one LDS read of an A operand feeds TILES MFMAs.
// =====================================================================================================
#include "mw_mlp_stack.h"                                          // StackP, leaky_slope, stack_dense, stack_images, the handle
#include <cmath>
#include <string>
#include <vector>
#include <algorithm>

namespace mw {

// N9: the nine features of the stencil model (features 5..8 from level min(nz - 1, k + 1): plain loads of cell + ncol, which the wave
// that owns that level loads too -- L2 hits).  TEND: the tendency form; the base of groups 1..3 comes by k_mlp's rotate.
template <int TILES, bool N9, bool TEND>
__global__ __launch_bounds__(256, 2) void k_mlp_stack(StackP P, const float *__restrict__ img, long long ncells, long long ncol,
                                                   const double *__restrict__ temp, const double *__restrict__ rho_d,
                                                   const double *__restrict__ rho_v, const double *__restrict__ rho_c,
                                                   const double *__restrict__ rho_r, double *__restrict__ o_temp, double *__restrict__ o_rv,
                                                   double *__restrict__ o_rc, double *__restrict__ o_rr) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  for (int i = threadIdx.x; i < P.nimg + MW_STACK_PAD; i += 256) lds[i] = i < P.nimg ? img[i] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = (g == 0) ? temp : (g == 1) ? rho_d : (g == 2) ? rho_v : rho_c;
  const double *in_1 = (!N9 || g == 0) ? rho_r : (g == 1) ? temp : (g == 2) ? rho_v : rho_c;      // feature 4 + g: rho_r of the cell; N9: temp, rho_v, rho_c above
  double *out_g = (g == 0) ? o_temp : (g == 1) ? o_rv : (g == 2) ? o_rc : o_rr;
  const bool has1 = N9 || g == 0, has2 = N9 && g == 0;                    // this lane carries feature 4 + g / feature 8
  const int f1 = has1 ? 4 + g : 4;
  const double imin0 = P.in_min[g], irng0 = 1.0 / P.in_rng[g], imin1 = P.in_min[f1], irng1 = 1.0 / P.in_rng[f1];
  const double imin2 = N9 ? P.in_min[8] : 0.0, irng2 = N9 ? 1.0 / P.in_rng[8] : 1.0;
  const double omin = P.out_min[g], orng = P.out_rng[g];
  const int last = P.nl - 1;
  const long long ntiles = (ncells + 15) / 16;
  for (long long t0 = wave * TILES; t0 < ntiles; t0 += nwaves * TILES) {
    double x0[TILES], x1[TILES], x2[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      const bool ok = cell < ncells;
      const long long above = (N9 && cell + ncol < ncells) ? cell + ncol : cell;                   // level min(nz - 1, k + 1), same column
      x0[u] = ok ? in_g[cell] : imin0;
      x1[u] = (ok && has1) ? in_1[g == 0 ? cell : above] : imin1;
      x2[u] = (ok && has2) ? rho_r[above] : imin2;
    }
    f32x4 a[MW_STACK_UB][TILES];
    double base[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      a[0][u] = (f32x4){net_scaled(x0[u], imin0, irng0), has1 ? net_scaled(x1[u], imin1, irng1) : 0.f, has2 ? net_scaled(x2[u], imin2, irng2) : 0.f, 0.f};
      if (TEND) { const double b = net5_rotate_base(g, x0[u], x1[u]); base[u] = g == 0 ? x0[u] : b; }
    }
    for (int l = 0; l < last; l++) {                                      // the hidden layers
      f32x4 d[MW_STACK_UB][TILES];
      const int nob = P.nob[l];
      const float slope = P.slope[l];
      stack_dense<TILES, MW_STACK_UB>(d, a, lds + P.aoff[l], lds + P.boff[l], P.nk[l], nob, lane, g);
#pragma unroll
      for (int ob = 0; ob < MW_STACK_UB; ob++) {
        if (ob < nob) {
#pragma unroll
          for (int u = 0; u < TILES; u++)
#pragma unroll
            for (int r = 0; r < 4; r++) a[ob][u][r] = leaky_slope(d[ob][u][r], slope);
        }
      }
    }
    f32x4 o[1][TILES];                                                    // Dense(4): output g in register 0 of group g
    stack_dense<TILES, 1>(o, a, lds + P.aoff[last], lds + P.boff[last], P.nk[last], 1, lane, g);
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      double y = (double)o[0][u][0] * orng + omin;
      if (TEND) y = base[u] + y;
      if (g != 0) y = fmax(0.0, y);
      if (cell < ncells) out_g[cell] = y;
    }
  }
}

// STRICT form (mw_mlp_set_strict(1)): thread = cell, the weights as they came, every layer a plain fp32 loop in index order (acc = 0;
// acc += x[i] * W[i][o]; then + b; then the activation), no contraction, the quotient form of the scaling (MW_STRICT_CELL).
template <bool TEND>
__global__ __launch_bounds__(256) void k_mlp_stack_strict(StackP P, const float *__restrict__ params, long long ncells, long long ncol,
                                                          const double *__restrict__ temp, const double *__restrict__ rho_d,
                                                          const double *__restrict__ rho_v, const double *__restrict__ rho_c,
                                                          const double *__restrict__ rho_r, double *__restrict__ temp_out,
                                                          double *__restrict__ rho_v_out, double *__restrict__ rho_c_out,
                                                          double *__restrict__ rho_r_out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  const long long ca = (P.n_in == 9 && c + ncol < ncells) ? c + ncol : c;
  const double in[9] = {temp[c], rho_d[c], rho_v[c], rho_c[c], rho_r[c], temp[ca], rho_v[ca], rho_c[ca], rho_r[ca]};
  float x[MW_STACK_MAX_WIDTH], h[MW_STACK_MAX_WIDTH];
  for (int i = 0; i < P.n_in; i++) x[i] = (float)((in[i] - P.in_min[i]) / P.in_rng[i]);
  for (int l = 0; l < P.nl; l++) {
    const int n = P.width[l], no = P.width[l + 1];
    const float *W = params + P.woff[l], *b = params + P.bwoff[l];
    for (int o = 0; o < no; o++) {
      float acc = 0.f;
      for (int i = 0; i < n; i++) acc += x[i] * W[i * no + o];
      acc = acc + b[o];
      h[o] = (l < P.nl - 1) ? (acc > 0.f ? acc : P.slope[l] * acc) : acc;
    }
    for (int o = 0; o < no; o++) x[o] = h[o];
  }
  if (TEND) {
    temp_out[c]  =           in[0] + (x[0] * P.out_rng[0] + P.out_min[0]);
    rho_v_out[c] = fmax(0.0, in[2] + (x[1] * P.out_rng[1] + P.out_min[1]));
    rho_c_out[c] = fmax(0.0, in[3] + (x[2] * P.out_rng[2] + P.out_min[2]));
    rho_r_out[c] = fmax(0.0, in[4] + (x[3] * P.out_rng[3] + P.out_min[3]));
  } else {
    temp_out[c]  =           x[0] * P.out_rng[0] + P.out_min[0];
    rho_v_out[c] = fmax(0.0, x[1] * P.out_rng[1] + P.out_min[1]);
    rho_c_out[c] = fmax(0.0, x[2] * P.out_rng[2] + P.out_min[2]);
    rho_r_out[c] = fmax(0.0, x[3] * P.out_rng[3] + P.out_min[3]);
  }
}

} // namespace mw

using namespace mw;

extern "C" void mw_mlp_stack_destroy(mw_mlp_stack_t s) {
  if (!s) return;
  (void)hipFree(s->img); (void)hipFree(s->params);
  delete s;
}

extern "C" int mw_mlp_stack_create(mw_mlp_stack_t *out, int n_in, int nhidden, const int *widths, const float *slopes, const float *params,
                                   long long nparams, const double *scl_in, const double *scl_out, int form) {
  if (!out) MW_FAIL("mlp_stack_create: null pointer");
  *out = nullptr;
  long long need = 0;
  if (stack_shape_check("mlp_stack_create", n_in, nhidden, widths, slopes, !params || !scl_in || !scl_out, &need)) return 1;
  if (nparams != need)
    MW_FAIL("mlp_stack_create: this shape has " + std::to_string(need) + " parameters, nparams is " + std::to_string(nparams));
  for (int i = 0; i < n_in; i++) if (scl_in[2 * i + 1] == scl_in[2 * i]) MW_FAIL("mlp_stack_create: input scaling row " + std::to_string(i) + " has max == min");
  for (int i = 0; i < 4; i++) if (scl_out[2 * i + 1] == scl_out[2 * i]) MW_FAIL("mlp_stack_create: output scaling row " + std::to_string(i) + " has max == min");
  if (form != MW_FORM_STATE && form != MW_FORM_TENDENCY)
    MW_FAIL("mlp_stack_create: form must be MW_FORM_STATE (0) or MW_FORM_TENDENCY (1), got " + std::to_string(form));
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");

  mw_mlp_stack_t s = new mw_mlp_stack_s();
  StackP &P = s->P;
  memset(&P, 0, sizeof(P));
  s->form = form; s->img = nullptr; s->params = nullptr;
  P.n_in = n_in; P.nl = nhidden + 1;
  P.width[0] = n_in;
  for (int l = 0; l < nhidden; l++) { P.width[l + 1] = widths[l]; P.slope[l] = slopes[l]; }
  P.width[P.nl] = 4;
  std::vector<float> img;
  int off = 0;
  for (int l = 0; l < P.nl; l++) {
    const int n_i = P.width[l], n_o = P.width[l + 1];
    P.woff[l] = off; P.bwoff[l] = off + n_i * n_o;
    P.nk[l] = (n_i + 3) / 4; P.nob[l] = (n_o + 15) / 16;
    stack_images(img, params + P.woff[l], params + P.bwoff[l], n_i, n_o, P.aoff[l], P.boff[l]);
    off += (n_i + 1) * n_o;
  }
  P.nimg = (int)img.size();
  fill_scaling(n_in, scl_in, scl_out, P.in_min, P.in_rng, P.out_min, P.out_rng);
  hipError_t e = hipMalloc(&s->img, sizeof(float) * img.size());
  if (e == hipSuccess) e = hipMalloc(&s->params, sizeof(float) * (size_t)nparams);
  if (e == hipSuccess) e = hipMemcpy(s->img, img.data(), sizeof(float) * img.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->params, params, sizeof(float) * (size_t)nparams, hipMemcpyHostToDevice);
  if (e != hipSuccess) { mw_mlp_stack_destroy(s); MW_FAIL(std::string("mlp_stack_create: ") + hipGetErrorString(e)); }
  *out = s;
  return 0;
}

// tiles per wave and iteration (DESIGN.md 13.18 has the resource row); grid: enough waves for the tiles, at most STACK_BLOCKS_PER_CU
// workgroups per CU, each of which fills its LDS once and walks the rest grid-stride
static constexpr int STACK_TILES = 4;
static constexpr long long STACK_MAX_BLOCKS = 256 * 8;

extern "C" int mw_mlp_stack_forward(mw_mlp_stack_t s, int nz, long long ncol, const double *temp, const double *rho_d, const double *rho_v,
                                    const double *rho_c, const double *rho_r, double *temp_out, double *rho_v_out, double *rho_c_out,
                                    double *rho_r_out, void *stream) {
  if (!s) MW_FAIL("mlp_stack_forward: null handle");
  if (nz < 1 || ncol < 1) MW_FAIL("mlp_stack_forward: nz and ncol must be >= 1");
  if (!temp || !rho_d || !rho_v || !rho_c || !rho_r || !temp_out || !rho_v_out || !rho_c_out || !rho_r_out) MW_FAIL("mlp_stack_forward: null pointer");
  const StackP &P = s->P;
  const long long ncells = (long long)nz * ncol;
  const bool n9 = P.n_in == 9, tend = s->form == MW_FORM_TENDENCY;
  if (n9)
    for (const double *o : {temp_out, rho_v_out, rho_c_out, rho_r_out})
      for (const double *i : {temp, rho_d, rho_v, rho_c, rho_r})
        if (o < i + ncells && i < o + ncells) MW_FAIL("mlp_stack_forward: with n_in = 9 the outputs must not overlap the inputs (level k + 1 is an input of level k)");
  hipStream_t st = (hipStream_t)stream;
  if (mlp_strict()) {
    const long long blocks = (ncells + 255) / 256;
    if (blocks > 0x7fffffffll) MW_FAIL("mlp_stack_forward: grid too large");
    MW_LAUNCH_IF(tend, (k_mlp_stack_strict<true>), (k_mlp_stack_strict<false>), dim3((unsigned)blocks), dim3(256), 0, st, P, s->params, ncells, ncol, temp, rho_d,
                 rho_v, rho_c, rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out);
    MW_LAUNCH_CHECK();
    return 0;
  }
  const long long waves = ((ncells + 15) / 16 + STACK_TILES - 1) / STACK_TILES;
  const long long blocks = std::max<long long>(1, std::min<long long>((waves + 3) / 4, STACK_MAX_BLOCKS));
  const size_t lds = sizeof(float) * (size_t)(P.nimg + MW_STACK_PAD);
#define MW_STACK_LAUNCH(N9, TEND)                                                                                                       \
  hipLaunchKernelGGL((k_mlp_stack<STACK_TILES, N9, TEND>), dim3((unsigned)blocks), dim3(256), lds, st, P, s->img, ncells, ncol, temp, rho_d, rho_v, rho_c, \
                     rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out)
  if (n9) { if (tend) MW_STACK_LAUNCH(true, true); else MW_STACK_LAUNCH(true, false); }
  else    { if (tend) MW_STACK_LAUNCH(false, true); else MW_STACK_LAUNCH(false, false); }
#undef MW_STACK_LAUNCH
  MW_LAUNCH_CHECK();
  return 0;
}
