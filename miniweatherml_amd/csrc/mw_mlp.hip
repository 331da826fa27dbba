// =====================================================================================================
// mw_mlp.hip -- the ponni 5 -> 10 -> 4 surrogate MLP as a batched MFMA GEMM on gfx950
// reference call sites: experiments/supercell_kessler_surrogate/custom_modules/microphysics_kessler_ponni.h
//   :103-110 (Matvec, Bias, Relu(negative_slope 0.1), Matvec, Bias), :180-187 (input scaling -> float),
//   :189 (forward_batch_parallel), :196-201 (un-scaling, clip >= 0).
//
// One fused kernel: scale (fp64) -> layer 1 -> leaky ReLU -> layer 2 -> un-scale + clip (fp64), 72 B of HBM
// traffic per cell and nothing else.  Matrix work rides v_mfma_f32_16x16x4_f32 (exact f32 fma chain):
//   tile = 16 cells on the N (column = lane & 15) axis; the K axis (lane >> 4 = "group" g) carries input features.
//   Layer 1: D1[16 x 16cells] = W1p^T[16 x 8] * X[8 x 16cells] + b1p      (2 MFMAs, K = 5 padded to 8)
//   Layer 2: D2[16 x 16cells] = W2p^T[16 x 12] * H[12 x 16cells] + b2p    (3 MFMAs, K = 10 padded to 12)
// The C/D layout (row = 4*g + reg) is used as the next B operand WITHOUT any lane movement: hidden unit u is
// placed at row rho(u) with rho(u) % 4 < 3, so register j of group g *is* k-slot g of MFMA j.  Output n is
// placed at row 4n, so lane group n holds output n in register 0 and stores 16 contiguous doubles.
// Inputs are fetched the same way: lane group g reads feature g's array (128 contiguous bytes per group).
//
// This unit: the forward kernels (k_mlp*, k_mlp_f32, k_ponni_generic, k_mlp_stencil*) and the host builders of the operand images.  The
// network's cell itself is mw_mlp_net.h's; the kernels that run a BANK of models on it are mw_surrogate_bank.hip's.
// =====================================================================================================
#include "mw_mlp_net.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

namespace mw {

// TILES 16-cell tiles per wave per iteration.  TEND: the tendency form (mw_mlp_net.h: net_out_tendency) -- a template parameter and not
// a branch on P.form, so that the state form's instantiation is the code it always was.  Lane group g > 0 then needs the field its output
// replaces (rho_v, rho_c, rho_r), which another group of the wave loads in the same iteration: one more 8-byte load per lane, in the
// register that only group 0 uses for rho_r, issued with the iteration's other loads and ahead of its stores.
template <int TILES, bool TEND>
__global__ __launch_bounds__(256) void k_mlp(MlpP P, long long ncells, const double *__restrict__ temp,
                                             const double *__restrict__ rho_d, const double *__restrict__ rho_v,
                                             const double *__restrict__ rho_c, const double *__restrict__ rho_r,
                                             double *__restrict__ o_temp, double *__restrict__ o_rv,
                                             double *__restrict__ o_rc, double *__restrict__ o_rr) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  // per-lane constants
  const double *in_g = (g == 0) ? temp : (g == 1) ? rho_d : (g == 2) ? rho_v : rho_c;
  double *out_g = (g == 0) ? o_temp : (g == 1) ? o_rv : (g == 2) ? o_rc : o_rr;
  constexpr bool LOADB = TEND && !MW_TENDENCY_ROTATE_FORWARD;                    // the base of groups 1..3 by a load (else, TEND: by the rotate)
  const double *in_s = (!LOADB || g == 0) ? rho_r : (g == 1) ? rho_v : (g == 2) ? rho_c : rho_r;     // group 0: rho_r for the network; else the base
  Net5 N;
  net5_ops(N, P, lane, g);
  const long long ntiles = (ncells + 15) / 16;
  for (long long t0 = wave * TILES; t0 < ntiles; t0 += nwaves * TILES) {
    double xin[TILES], xin4[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      long long cell = (t0 + u) * 16 + cidx;
      bool ok = cell < ncells;
      xin[u]  = ok ? in_g[cell] : N.imin;
      xin4[u] = (ok && (LOADB || g == 0)) ? in_s[cell] : N.imin4;
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      long long cell = (t0 + u) * 16 + cidx;
      if (TEND && !LOADB) xin4[u] = net5_rotate_base(g, xin[u], xin4[u]);
      const double y = net5_cell_form<TEND>(N, g, xin[u], xin4[u], MW_FORM_TENDENCY);
      if (cell < ncells) out_g[cell] = y;
    }
  }
}

// The same with 16-byte accesses: a lane owns the cell PAIR (2c, 2c+1) of a 32-cell span, loaded / stored as one double2 -- every
// lane group then moves 256 contiguous bytes per instruction and the wave issues half as many memory instructions.  The even
// cells of the span form one MFMA tile, the odd cells the next (a tile is any 16 cells).  ncells must be a multiple of 32 here;
// the launcher hands the remainder to k_mlp.
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <int PAIRS, bool TEND>
__global__ __launch_bounds__(256) void k_mlp_x2(MlpP P, long long ncells, const double *__restrict__ temp,
                                                const double *__restrict__ rho_d, const double *__restrict__ rho_v,
                                                const double *__restrict__ rho_c, const double *__restrict__ rho_r,
                                                double *__restrict__ o_temp, double *__restrict__ o_rv,
                                                double *__restrict__ o_rc, double *__restrict__ o_rr) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const double *in_g = (g == 0) ? temp : (g == 1) ? rho_d : (g == 2) ? rho_v : rho_c;
  double *out_g = (g == 0) ? o_temp : (g == 1) ? o_rv : (g == 2) ? o_rc : o_rr;
  constexpr bool LOADB = TEND && !MW_TENDENCY_ROTATE_FORWARD;                    // (as in k_mlp)
  const double *in_s = (!LOADB || g == 0) ? rho_r : (g == 1) ? rho_v : (g == 2) ? rho_c : rho_r;
  Net5 N;
  net5_ops(N, P, lane, g);
  const long long nspans = ncells / 32;
  for (long long s0 = wave * PAIRS; s0 < nspans; s0 += nwaves * PAIRS) {
    f64x2 xin[PAIRS], xin4[PAIRS];
#pragma unroll
    for (int u = 0; u < PAIRS; u++) {
      const long long cell = min(s0 + u, nspans - 1) * 32 + 2 * cidx;          // (clamped: the tail spans are recomputed, not stored)
      xin[u] = *(const f64x2 *)(in_g + cell);
      xin4[u] = (LOADB || g == 0) ? *(const f64x2 *)(in_s + cell) : (f64x2){N.imin4, N.imin4};
    }
#pragma unroll
    for (int u = 0; u < PAIRS; u++) {
      f64x2 y2;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (TEND && !LOADB) xin4[u][h] = net5_rotate_base(g, xin[u][h], xin4[u][h]);
        y2[h] = net5_cell_form<TEND>(N, g, xin[u][h], xin4[u][h], MW_FORM_TENDENCY);
      }
      if (s0 + u < nspans) *(f64x2 *)(out_g + (s0 + u) * 32 + 2 * cidx) = y2;
    }
  }
}


// ponni::Inference::forward_batch_parallel for the surrogate's stack on fp32 arrays in ponni's own layout -- in (5, batch), out (4, batch),
// batch fastest (microphysics_kessler_ponni.h:176-189: ponni_in(feature, iglob)) -- with the same MFMA tiles as k_mlp: lane group g
// reads feature g's row (64 contiguous bytes per group and tile), output n leaves from group n.  The activation slope is an argument
// (ponni::Relu<float>(n, negative_slope), :105).  NM1 = 3: the 9 -> 10 -> 4 stack of the stencil model, K = 9 padded to 12 (group 0 also
// reads feature 8; one more layer-1 MFMA, everything else the same).
template <int TILES, int NM1>
__global__ __launch_bounds__(256) void k_mlp_f32(MlpP P, float slope, long long batch, const float *__restrict__ in, float *__restrict__ out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * 256) >> 6;
  const float *in_g = in + (long long)g * batch, *in_4 = in + (NM1 == 3 ? 4 + g : 4) * batch, *in_8 = in + 8 * batch;
  float *out_g = out + (long long)g * batch;
  const float a10 = P.a1[0][lane], a11 = P.a1[1][lane], a12 = P.a1[2][lane];
  const float a20 = P.a2[0][lane], a21 = P.a2[1][lane], a22 = P.a2[2][lane];
  const f32x4 c1 = {P.c1[g][0], P.c1[g][1], P.c1[g][2], P.c1[g][3]};
  const f32x4 c2 = {P.c2[g], 0.f, 0.f, 0.f};
  const NetOut N = {a20, a21, a22, c2, 0.0, 1.0};                         // (layer 2 alone: ponni's arrays are the network's own, unscaled)
  const long long ntiles = (batch + 15) / 16;
  for (long long t0 = wave * TILES; t0 < ntiles; t0 += nwaves * TILES) {
    float x0[TILES], x4[TILES], x8[TILES];
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      const bool ok = cell < batch;
      x0[u] = ok ? in_g[cell] : 0.f;
      x4[u] = (ok && (NM1 == 3 || g == 0)) ? in_4[cell] : 0.f;
      if (NM1 == 3) x8[u] = (ok && g == 0) ? in_8[cell] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < TILES; u++) {
      const long long cell = (t0 + u) * 16 + cidx;
      f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a10, x0[u], c1, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a11, x4[u], d1, 0, 0, 0);
      if (NM1 == 3) d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a12, x8[u], d1, 0, 0, 0);
      const float h0 = d1[0] > 0.f ? d1[0] : slope * d1[0], h1 = d1[1] > 0.f ? d1[1] : slope * d1[1], h2 = d1[2] > 0.f ? d1[2] : slope * d1[2];
      const f32x4 d2 = net_layer2(N, h0, h1, h2);
      if (cell < batch) out_g[cell] = d2[0];
    }
  }
}

// Any other stack of ponni layers (Matvec / Bias / Relu), and the strict form of the surrogate's: thread = one batch element, every
// layer a plain fp32 loop in index order (Matvec: acc = 0; acc += x[i] * W[i][o] for i = 0 .. n_in - 1), no contraction.
#define MW_PONNI_MAX_LAYERS 10                                  // (microphysics_kessler_ponni.h:32)
#define MW_PONNI_MAX_WIDTH 32
#define MW_PONNI_MAX_PARAMS 960
struct PonniStack { int nlayers; int kind[MW_PONNI_MAX_LAYERS], n_in[MW_PONNI_MAX_LAYERS], n_out[MW_PONNI_MAX_LAYERS], off[MW_PONNI_MAX_LAYERS];
                    float slope[MW_PONNI_MAX_LAYERS]; float params[MW_PONNI_MAX_PARAMS]; };
__global__ __launch_bounds__(256) void k_ponni_generic(PonniStack P, long long batch, const float *__restrict__ in, float *__restrict__ out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= batch) return;
  float a[MW_PONNI_MAX_WIDTH], b[MW_PONNI_MAX_WIDTH];
  int n = P.n_in[0];
  for (int i = 0; i < n; i++) a[i] = in[(long long)i * batch + c];
  for (int l = 0; l < P.nlayers; l++) {
    const float *w = P.params + P.off[l];
    if (P.kind[l] == 0) {                                        // Matvec: weights (n_in, n_out), y = x W
      for (int o = 0; o < P.n_out[l]; o++) { float acc = 0.f; for (int i = 0; i < n; i++) acc += a[i] * w[i * P.n_out[l] + o]; b[o] = acc; }
      n = P.n_out[l];
      for (int o = 0; o < n; o++) a[o] = b[o];
    } else if (P.kind[l] == 1) { for (int o = 0; o < n; o++) a[o] = a[o] + w[o]; }
    else { const float sl = P.slope[l]; for (int o = 0; o < n; o++) a[o] = a[o] > 0.f ? a[o] : sl * a[o]; }
  }
  for (int o = 0; o < n; o++) out[(long long)o * batch + c] = a[o];
}

} // namespace mw

using namespace mw;

// STRICT form (mw_mlp_set_strict(1)): thread = cell, the index-order loops of MW_STRICT_CELL -- bit-identical to the CPU restatement.
// (The MFMA kernels sum the same products in the matrix cores' order: 1e-5 on the fp32 outputs.)
template <bool TEND>
__global__ __launch_bounds__(256) void k_mlp_strict(MlpRef P, long long n, const double *__restrict__ temp, const double *__restrict__ rho_d,
                                                    const double *__restrict__ rho_v, const double *__restrict__ rho_c, const double *__restrict__ rho_r,
                                                    double *__restrict__ temp_out, double *__restrict__ rho_v_out, double *__restrict__ rho_c_out,
                                                    double *__restrict__ rho_r_out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const double in[5] = {temp[c], rho_d[c], rho_v[c], rho_c[c], rho_r[c]};
  MW_STRICT_CELL_FORM(5, P, in, TEND, temp_out[c], rho_v_out[c], rho_c_out[c], rho_r_out[c])
}

// The MFMA operand images (see the header of this file): A operands per lane, C initialisers = the biases.
static int hidden_at(int row) {                                 // the hidden unit u at D1 row rho(u) = (u / 3) * 4 + u % 3 (row % 4 < 3), or -1
  for (int u = 0; u < 10; u++) if ((u / 3) * 4 + (u % 3) == row) return u;
  return -1;
}
void mw::net_dense_layer1_images(float (*a1)[64], const float *W1, int n_in) {
  for (int lane = 0; lane < 64; lane++) {
    const int u = hidden_at(lane & 15), g = lane >> 4;
    for (int m = 0; m < 3; m++) { const int in = 4 * m + g; a1[m][lane] = (u >= 0 && in < n_in) ? W1[in * 10 + u] : 0.f; }
  }
}
void mw::net_stencil_layer1_images(float (*a1)[64], const float *W1) {
  const int above_of_group[4] = {5, -1, 6, 7};
  for (int lane = 0; lane < 64; lane++) {
    const int u = hidden_at(lane & 15), g = lane >> 4;
    a1[0][lane] = u < 0 ? 0.f : W1[g * 10 + u];
    a1[1][lane] = u < 0 || above_of_group[g] < 0 ? 0.f : W1[above_of_group[g] * 10 + u];
    a1[2][lane] = u < 0 ? 0.f : g == 0 ? W1[4 * 10 + u] : g == 1 ? W1[8 * 10 + u] : 0.f;      // even k: group 0 holds level k, group 1 level k + 1
    a1[3][lane] = u < 0 ? 0.f : g == 0 ? W1[8 * 10 + u] : g == 1 ? W1[4 * 10 + u] : 0.f;      // odd k: the other way round
  }
}
void mw::net_layer2_images(float (&c1)[4][4], float (&a2)[3][64], float (&c2)[4], const float *b1, const float *W2, const float *b2) {
  for (int lane = 0; lane < 64; lane++) {
    const int o = lane & 15, g = lane >> 4, n = (o % 4 == 0) ? o / 4 : -1;                    // output n lives at row 4n
    for (int j = 0; j < 3; j++) { const int uk = hidden_at(4 * g + j); a2[j][lane] = (n >= 0 && uk >= 0) ? W2[uk * 4 + n] : 0.f; }   // k-slot g of MFMA j is hidden row 4g + j
  }
  for (int g = 0; g < 4; g++) {
    for (int r = 0; r < 4; r++) { const int u = hidden_at(4 * g + r); c1[g][r] = (u >= 0) ? b1[u] : 0.f; }
    c2[g] = b2[g];
  }
}

static thread_local int g_mlp_strict = 0;        // per calling thread: a rank harness with one host thread per rank may use different modes side by side
extern "C" int mw_mlp_set_strict(int strict) { g_mlp_strict = strict ? 1 : 0; return 0; }
int mw::mlp_strict() { return g_mlp_strict; }

static bool form_known(int form) { return form == MW_FORM_STATE || form == MW_FORM_TENDENCY; }

extern "C" int mw_mlp_forward_form(int form, long long ncells, const double *temp, const double *rho_d, const double *rho_v, const double *rho_c,
                                   const double *rho_r, const float *W1, const float *b1, const float *W2, const float *b2,
                                   const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out,
                                   double *rho_c_out, double *rho_r_out, void *stream) {
  if (!form_known(form)) MW_FAIL("mlp: form must be MW_FORM_STATE (0) or MW_FORM_TENDENCY (1), got " + std::to_string(form));
  const bool tend = form == MW_FORM_TENDENCY;
  if (ncells < 1) MW_FAIL("mlp: ncells must be >= 1");
  if (!temp || !rho_d || !rho_v || !rho_c || !rho_r || !W1 || !b1 || !W2 || !b2 || !scl_in || !scl_out || !temp_out ||
      !rho_v_out || !rho_c_out || !rho_r_out) MW_FAIL("mlp: null pointer");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  if (g_mlp_strict) {
    MlpRef R;
    fill_ref(R, 5, W1, b1, W2, b2, scl_in, scl_out, form);
    MW_LAUNCH_IF(tend, (k_mlp_strict<true>), (k_mlp_strict<false>), dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R, ncells, temp, rho_d, rho_v, rho_c,
                       rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out);
    MW_LAUNCH_CHECK();
    return 0;
  }
  MlpP P;          // operand images built per call (cheap: 104 weights)
  net_dense_layer1_images(P.a1, W1, 5);
  net_layer2_images(P.c1, P.a2, P.c2, b1, W2, b2);
  fill_scaling(5, scl_in, scl_out, P.in_min, P.in_rng, P.out_min, P.out_rng);
  P.form = form;
  constexpr int TILES = 4, PAIRS = 2;
  // bulk: spans of 32 cells with 16-byte accesses (needs 16-byte aligned arrays); remainder (and unaligned callers): k_mlp
  bool aligned = true;
  for (const void *q : {(const void *)temp, (const void *)rho_d, (const void *)rho_v, (const void *)rho_c, (const void *)rho_r, (const void *)temp_out,
                        (const void *)rho_v_out, (const void *)rho_c_out, (const void *)rho_r_out}) aligned = aligned && (((size_t)q & 15) == 0);
  const long long bulk = aligned ? (ncells / 32) * 32 : 0;
  if (bulk > 0) {
    long long waves_needed = (bulk / 32 + PAIRS - 1) / PAIRS;
    long long blocks = (waves_needed + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;                   // grid-stride beyond 16 blocks per CU
    MW_LAUNCH_IF(tend, (k_mlp_x2<PAIRS, true>), (k_mlp_x2<PAIRS, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, bulk, temp, rho_d, rho_v, rho_c,
                       rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out);
    MW_LAUNCH_CHECK();
  }
  const long long rest = ncells - bulk;
  if (rest > 0) {
    long long ntiles = (rest + 15) / 16;
    long long waves_needed = (ntiles + TILES - 1) / TILES;
    long long blocks = (waves_needed + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    MW_LAUNCH_IF(tend, (k_mlp<TILES, true>), (k_mlp<TILES, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, rest, temp + bulk, rho_d + bulk, rho_v + bulk,
                       rho_c + bulk, rho_r + bulk, temp_out + bulk, rho_v_out + bulk, rho_c_out + bulk, rho_r_out + bulk);
    MW_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int mw_mlp_forward(long long ncells, const double *temp, const double *rho_d, const double *rho_v, const double *rho_c,
                              const double *rho_r, const float *W1, const float *b1, const float *W2, const float *b2,
                              const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out,
                              double *rho_c_out, double *rho_r_out, void *stream) {
  return mw_mlp_forward_form(MW_FORM_STATE, ncells, temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, temp_out, rho_v_out,
                             rho_c_out, rho_r_out, stream);
}

// ponni::Inference<...>::forward_batch_parallel (microphysics_kessler_ponni.h:189) for a stack of ponni layers on fp32 device arrays in
// ponni's layout: in (n_in of the first layer, batch), out (n_out of the last, batch), batch fastest.  layers / params: HOST memory
// (params = the layers' weights back to back: a Matvec's (n_in, n_out) kernel in Keras order, a Bias's vector; offsets in floats).
// The surrogate's stacks Matvec(5 or 9,10), Bias(10), Relu(10), Matvec(10,4), Bias(4) run on the MFMA tiles; any other stack that fits
// the limits (MW_PONNI_MAX_*), and every stack under mw_mlp_set_strict(1), on the thread-per-element kernel (index order, no contraction).
extern "C" int mw_ponni_forward(const mw_ponni_layer_t *layers, int nlayers, const float *params, int nparams, long long batch,
                                const float *in, float *out, void *stream) {
  if (!layers || nlayers < 1 || !params || nparams < 0 || !in || !out) MW_FAIL("ponni_forward: null argument");
  if (batch < 1) MW_FAIL("ponni_forward: batch must be >= 1");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  if (nlayers > MW_PONNI_MAX_LAYERS) MW_FAIL("ponni_forward: more than " + std::to_string(MW_PONNI_MAX_LAYERS) + " layers");
  if (nparams > MW_PONNI_MAX_PARAMS) MW_FAIL("ponni_forward: more than " + std::to_string(MW_PONNI_MAX_PARAMS) + " parameters");
  // Inference::validate(): every layer's input size is its predecessor's output size, parameters inside the buffer
  int width = layers[0].n_in;
  for (int l = 0; l < nlayers; l++) {
    const mw_ponni_layer_t &L = layers[l];
    if (L.kind < 0 || L.kind > 2) MW_FAIL("ponni_forward: unknown layer kind");
    if (L.n_in != width) MW_FAIL("ponni_forward: layer " + std::to_string(l) + " expects " + std::to_string(L.n_in) + " inputs but its predecessor provides " + std::to_string(width));
    if (L.kind != 0 && L.n_out != L.n_in) MW_FAIL("ponni_forward: Bias / Relu layers keep the size");
    if (L.n_in < 1 || L.n_out < 1 || L.n_in > MW_PONNI_MAX_WIDTH || L.n_out > MW_PONNI_MAX_WIDTH) MW_FAIL("ponni_forward: layer width outside [1, " + std::to_string(MW_PONNI_MAX_WIDTH) + "]");
    const long long need = L.kind == 0 ? (long long)L.n_in * L.n_out : L.kind == 1 ? L.n_out : 0;
    if (need && (L.offset < 0 || L.offset + need > nparams)) MW_FAIL("ponni_forward: layer parameters outside the buffer");
    width = L.n_out;
  }
  hipStream_t st = (hipStream_t)stream;
  const int n_in = layers[0].n_in;
  const bool surrogate = nlayers == 5 && layers[0].kind == 0 && (n_in == 5 || n_in == 9) && layers[0].n_out == 10 && layers[1].kind == 1 &&
                         layers[2].kind == 2 && layers[3].kind == 0 && layers[3].n_out == 4 && layers[4].kind == 1;
  if (surrogate && !g_mlp_strict) {
    MlpP P;
    memset(&P, 0, sizeof(P));                                   // (no scaling: ponni's arrays are the network's own inputs and outputs)
    net_dense_layer1_images(P.a1, params + layers[0].offset, n_in);
    net_layer2_images(P.c1, P.a2, P.c2, params + layers[1].offset, params + layers[3].offset, params + layers[4].offset);
    constexpr int TILES = 4;
    long long blocks = (((batch + 15) / 16 + TILES - 1) / TILES + 3) / 4;
    blocks = std::max<long long>(1, std::min<long long>(blocks, 256 * 16));
    if (n_in == 5) hipLaunchKernelGGL((k_mlp_f32<TILES, 2>), dim3((unsigned)blocks), dim3(256), 0, st, P, layers[2].negative_slope, batch, in, out);
    else           hipLaunchKernelGGL((k_mlp_f32<TILES, 3>), dim3((unsigned)blocks), dim3(256), 0, st, P, layers[2].negative_slope, batch, in, out);
    MW_LAUNCH_CHECK();
    return 0;
  }
  PonniStack S;
  memset(&S, 0, sizeof(S));
  S.nlayers = nlayers;
  for (int l = 0; l < nlayers; l++) { S.kind[l] = layers[l].kind; S.n_in[l] = layers[l].n_in; S.n_out[l] = layers[l].n_out; S.off[l] = layers[l].offset; S.slope[l] = layers[l].negative_slope; }
  memcpy(S.params, params, sizeof(float) * (size_t)nparams);
  hipLaunchKernelGGL(k_ponni_generic, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, S, batch, in, out);
  MW_LAUNCH_CHECK();
  return 0;
}

// =====================================================================================================
// The STENCIL model 9 -> 10 -> 4 on the coupler's fields (level-major: cell (k, col) at k * ncol + col).  Features 0..4 are the cell's
// (temp, rho_d, rho_v, rho_c, rho_r), features 5..8 are (temp, rho_v, rho_c, rho_r) of level min(nz - 1, k + 1) of the same column:
// DataGenerator::generate_samples_stencil's inputs(:, :, 0) and inputs(0..3, 1) (generate_micro_surrogate_data.h:139-156).
//
// k_mlp_stencil: k_mlp's tiles with layer 1 as K = 9 padded to 12 (three MFMAs), one wave per (16-column tile, z chunk), the levels swept
// TOP-DOWN so that the level-above operand is what the previous iteration loaded -- every input is read once (plus one level per chunk):
//   MFMA 0, k-slot g : feature g of level k (group g loads field g, as in k_mlp)
//   MFMA 1, k-slot g : the SAME lane's value of level k + 1, scaled as feature 5 / - / 6 / 7 (group 1 holds rho_d, which has no
//                      level-above feature: its A operand is zero) -- carried in a register, no lane movement
//   MFMA 2           : rho_r of levels k and k + 1.  Group (k & 1) loads rho_r of level k, so group 0 always holds the last even level
//                      and group 1 the last odd one; the A operand (W1 rows 4 and 8) swaps its two groups with the parity of k.
// Layer 2, un-scaling and clip are k_mlp's.  The outputs must not alias the inputs (level k + 1 is an input of level k, and a chunk's
// first level-above is computed by another wave).
// =====================================================================================================
namespace mw {

template <int U, bool TEND>
__global__ __launch_bounds__(256) void k_mlp_stencil(StencilP P, int nz, long long ncol, int zc, int nchunks,
                                                     const double *__restrict__ temp, const double *__restrict__ rho_d,
                                                     const double *__restrict__ rho_v, const double *__restrict__ rho_c,
                                                     const double *__restrict__ rho_r, double *__restrict__ o_temp,
                                                     double *__restrict__ o_rv, double *__restrict__ o_rc, double *__restrict__ o_rr) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cidx = lane & 15;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long ntiles = (ncol + 15) / 16;
  if (wave >= ntiles * nchunks) return;                                   // (wave-uniform)
  const int chunk = (int)(wave % nchunks);
  const long long col = (wave / nchunks) * 16 + cidx;
  const bool ok = col < ncol;
  const int k_lo = chunk * zc, k_hi = min(nz, k_lo + zc) - 1, k_top = min(nz - 1, k_hi + 1);
  const double *in_g = (g == 0) ? temp : (g == 1) ? rho_d : (g == 2) ? rho_v : rho_c;
  double *out_g = (g == 0) ? o_temp : (g == 1) ? o_rv : (g == 2) ? o_rc : o_rr;
  const double *in_s = (g == 1) ? rho_v : (g == 2) ? rho_c : rho_r;       // TEND: the field output g replaces (group 0 holds its own, temp)
  Net9 N;
  net9_ops(N, P, lane, g);
  // the level above the chunk's top (the top level itself at the model top): the one level a chunk reads twice
  float above = 0.f, rr_s = 0.f;          // rr_s: this group's latest rho_r, scaled as feature 4 when it is level k and as feature 8 when k + 1
  double rr_raw = N.rmin;
  if (ok) {
    above = net9_above(N, in_g[(long long)k_top * ncol + col]);
    if (g == ((k_hi & 1) ^ 1)) rr_raw = rho_r[(long long)k_top * ncol + col];
  }
  for (int k0 = k_hi; k0 >= k_lo; k0 -= U) {
    double xin[U], xrr[U], xs[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = k0 - u;
      const bool lv = ok && k >= k_lo;
      xin[u] = lv ? in_g[(long long)k * ncol + col] : N.imin;
      xrr[u] = (lv && g == (k & 1)) ? rho_r[(long long)k * ncol + col] : N.rmin;
      if (TEND) xs[u] = (lv && g != 0) ? in_s[(long long)k * ncol + col] : xin[u];                  // level k's own value, not the carried level above
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = k0 - u;
      if (k >= k_lo) {                                                    // (wave-uniform)
        if (g == (k & 1)) rr_raw = xrr[u];                                // this group holds rho_r of level k, the other one of level k + 1
        const f32x4 d1 = net9_layer1(N, k, net9_b0(N, xin[u]), above, net9_b2(N, g, k, rr_raw));
        above = net9_above(N, xin[u]);                                    // level k is level k - 1's level above
        const double y = net_out_form<TEND>(N, g, d1, MW_FORM_TENDENCY, TEND ? xs[u] : 0.0);
        if (ok) out_g[(long long)k * ncol + col] = y;
      }
    }
  }
}

// STRICT form: thread = cell, MW_STRICT_CELL with nine features.
template <bool TEND>
__global__ __launch_bounds__(256) void k_mlp_stencil_strict(StencilRef P, int nz, long long ncol, const double *__restrict__ temp,
                                                            const double *__restrict__ rho_d, const double *__restrict__ rho_v,
                                                            const double *__restrict__ rho_c, const double *__restrict__ rho_r,
                                                            double *__restrict__ temp_out, double *__restrict__ rho_v_out,
                                                            double *__restrict__ rho_c_out, double *__restrict__ rho_r_out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= (long long)nz * ncol) return;
  const long long k = c / ncol;
  const long long ca = (k + 1 < nz) ? c + ncol : c;                       // level min(nz - 1, k + 1), same column
  const double in[9] = {temp[c], rho_d[c], rho_v[c], rho_c[c], rho_r[c], temp[ca], rho_v[ca], rho_c[ca], rho_r[ca]};
  MW_STRICT_CELL_FORM(9, P, in, TEND, temp_out[c], rho_v_out[c], rho_c_out[c], rho_r_out[c])
}

} // namespace mw

// z chunks of the production kernel: a wave owns (16 columns, zc levels).  One chunk per column unless the tiles alone leave the chip
// short of waves; then as many chunks as bring ntiles * nchunks to STENCIL_WAVES, but never shorter than STENCIL_MIN_ZC levels (a chunk
// re-reads one level of four fields: 4 / (9 zc) of its input).
static constexpr long long STENCIL_WAVES = 256 * 4 * 8 * 2;      // 256 CUs x 4 SIMDs x 8 wave slots, twice over
static constexpr int STENCIL_MIN_ZC = 8;
extern "C" int mw_mlp_stencil_chunk(int nz, long long ncol) {
  if (nz < 1 || ncol < 1) return 0;
  const long long ntiles = (ncol + 15) / 16;
  long long want = (STENCIL_WAVES + ntiles - 1) / ntiles;
  want = std::max<long long>(1, std::min<long long>(want, (nz + STENCIL_MIN_ZC - 1) / STENCIL_MIN_ZC));
  return (int)((nz + want - 1) / want);
}

extern "C" int mw_mlp_stencil_forward_form(int form, int nz, long long ncol, const double *temp, const double *rho_d, const double *rho_v,
                                           const double *rho_c, const double *rho_r, const float *W1, const float *b1, const float *W2,
                                           const float *b2, const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out,
                                           double *rho_c_out, double *rho_r_out, void *stream) {
  if (!form_known(form)) MW_FAIL("mlp_stencil: form must be MW_FORM_STATE (0) or MW_FORM_TENDENCY (1), got " + std::to_string(form));
  const bool tend = form == MW_FORM_TENDENCY;
  if (nz < 1 || ncol < 1) MW_FAIL("mlp_stencil: nz and ncol must be >= 1");
  if (!temp || !rho_d || !rho_v || !rho_c || !rho_r || !W1 || !b1 || !W2 || !b2 || !scl_in || !scl_out || !temp_out ||
      !rho_v_out || !rho_c_out || !rho_r_out) MW_FAIL("mlp_stencil: null pointer");
  const long long ncells = (long long)nz * ncol;
  for (const double *o : {temp_out, rho_v_out, rho_c_out, rho_r_out})
    for (const double *i : {temp, rho_d, rho_v, rho_c, rho_r})
      if (o < i + ncells && i < o + ncells) MW_FAIL("mlp_stencil: the outputs must not overlap the inputs (level k + 1 is an input of level k)");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  if (g_mlp_strict) {
    StencilRef R;
    fill_ref(R, 9, W1, b1, W2, b2, scl_in, scl_out, form);
    MW_LAUNCH_IF(tend, (k_mlp_stencil_strict<true>), (k_mlp_stencil_strict<false>), dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R, nz, ncol, temp, rho_d,
                       rho_v, rho_c, rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out);
    MW_LAUNCH_CHECK();
    return 0;
  }
  StencilP P;
  net_stencil_layer1_images(P.a1, W1);
  net_layer2_images(P.c1, P.a2, P.c2, b1, W2, b2);
  fill_scaling(9, scl_in, scl_out, P.in_min, P.in_rng, P.out_min, P.out_rng);
  P.form = form;
  const int zc = mw_mlp_stencil_chunk(nz, ncol), nchunks = (nz + zc - 1) / zc;
  const long long waves = ((ncol + 15) / 16) * nchunks, blocks = (waves + 3) / 4;
  if (blocks > 0x7fffffffll) MW_FAIL("mlp_stencil: grid too large");
  MW_LAUNCH_IF(tend, (k_mlp_stencil<4, true>), (k_mlp_stencil<4, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P, nz, ncol, zc, nchunks, temp, rho_d, rho_v,
                     rho_c, rho_r, temp_out, rho_v_out, rho_c_out, rho_r_out);
  MW_LAUNCH_CHECK();
  return 0;
}

extern "C" int mw_mlp_stencil_forward(int nz, long long ncol, const double *temp, const double *rho_d, const double *rho_v,
                                      const double *rho_c, const double *rho_r, const float *W1, const float *b1, const float *W2,
                                      const float *b2, const double *scl_in, const double *scl_out, double *temp_out, double *rho_v_out,
                                      double *rho_c_out, double *rho_r_out, void *stream) {
  return mw_mlp_stencil_forward_form(MW_FORM_STATE, nz, ncol, temp, rho_d, rho_v, rho_c, rho_r, W1, b1, W2, b2, scl_in, scl_out, temp_out,
                                     rho_v_out, rho_c_out, rho_r_out, stream);
}
