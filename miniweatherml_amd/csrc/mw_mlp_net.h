// =====================================================================================================
// mw_mlp_net.h -- the surrogate network's cell, defined ONCE for every kernel that evaluates it (mw_mlp.hip: the forward kernels;
// mw_surrogate_bank.hip: eval, members-apply, committee), the images those kernels read, and what the two units share on the host.
//
// MFMA form (the header of mw_mlp.hip has the tile layout): a lane's operands are a Net5 / Net9, filled by net5_ops / net9_ops from any
// model image; net5_cell is the single-cell network, net9_layer1 + net_out the stencil one.  Strict form: MW_STRICT_CELL, thread = cell,
// index order, the quotient form of the scaling.  What the project promises about these kernels -- a committee of one keeps the model's
// bits, eval scores the bits the forward kernels store, strict equals the CPU restatement -- rests on there being one definition.
// Only templates, inline functions and a macro live here: every kernel is emitted from exactly one unit.
// =====================================================================================================
#pragma once
#include "../../include/mw_cdna4.h"
#include "mw_common.h"
#include <cstring>

// (in the global namespace, as k_mlp_strict is: the kernel's symbol carries its argument types)
struct MlpRef { float W1[50], b1[10], W2[40], b2[4]; double in_min[5], in_rng[5], out_min[4], out_rng[4]; int form; };

namespace mw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- model images (layouts are the kernels' argument / LDS layouts) ----
struct MlpP {
  float a1[3][64];      // layer-1 A operand per MFMA m, per lane (m = 2: only the 9-input stack's feature 8)
  float c1[4][4];       // layer-1 C init (bias) [g][reg]
  float a2[3][64];      // layer-2 A operand per MFMA j, per lane
  float c2[4];          // layer-2 C init for reg 0 of group g (bias of output g)
  double in_min[5], in_rng[5];     // scl_in(:,0), scl_in(:,1)-scl_in(:,0)
  double out_min[4], out_rng[4];
  int form;                        // MW_FORM_STATE / MW_FORM_TENDENCY: what the un-scaled output is (net_out / net_out_tendency)
};
struct StencilP {
  float a1[4][64];      // layer-1 A operands: [0] cell features 0..3, [1] level-above features by group, [2] / [3] rho_r rows for even / odd k
  float c1[4][4];
  float a2[3][64];
  float c2[4];
  double in_min[9], in_rng[9];
  double out_min[4], out_rng[4];
  int form;
};
struct EvalModel {                         // one model of a bank as the MFMA kernels read it from LDS
  float a1[4][64];                         // n_in 5: MlpP::a1[0..1]; n_in 9: StencilP::a1[0..3]
  float a2[3][64];
  float c1[4][4];
  float c2[4];
  double in_min[9], in_irng[9];            // in_irng: uploaded as the range, inverted on the device by k_surrogate_bank_recip
  double out_min[4], out_rng[4];
  int form;                                // per model: a bank may hold both forms, as it holds models with different scaling tables
};
// the strict kernels' form: the weights as they are (MlpRef: above, outside the namespace)
struct StencilRef { float W1[90], b1[10], W2[40], b2[4]; double in_min[9], in_rng[9], out_min[4], out_rng[4]; int form; };

// ---- host side (defined in mw_mlp.hip) ----
// the MFMA operand images: layer 1 of the dense form (feature 4m + g in k-slot g of MFMA m: 5 inputs, or ponni's 9), layer 1 of the
// stencil sweep, and layer 2 with both biases, each written straight into the image's arrays (a1: its first 3 / all 4 rows)
void net_dense_layer1_images(float (*a1)[64], const float *W1, int n_in);
void net_stencil_layer1_images(float (*a1)[64], const float *W1);
void net_layer2_images(float (&c1)[4][4], float (&a2)[3][64], float (&c2)[4], const float *b1, const float *W2, const float *b2);
int mlp_strict();     // mw_mlp_set_strict's flag of the calling thread

// scl_in (n_in, 2), scl_out (4, 2) -> minimum and range; rows n_in .. NI - 1 of a wider table: minimum 0, range 1
template <int NI>
inline void fill_scaling(int n_in, const double *scl_in, const double *scl_out, double (&in_min)[NI], double (&in_rng)[NI], double (&out_min)[4],
                         double (&out_rng)[4]) {
  for (int i = 0; i < NI; i++) { in_min[i] = i < n_in ? scl_in[i * 2] : 0.0; in_rng[i] = i < n_in ? scl_in[i * 2 + 1] - scl_in[i * 2] : 1.0; }
  for (int i = 0; i < 4; i++) { out_min[i] = scl_out[i * 2]; out_rng[i] = scl_out[i * 2 + 1] - scl_out[i * 2]; }
}
// a strict kernel's table (MlpRef / StencilRef) of a model with n_in inputs: the weights as they are; what a narrower model leaves is zero
template <typename R>
inline void fill_ref(R &ref, int n_in, const float *W1, const float *b1, const float *W2, const float *b2, const double *scl_in, const double *scl_out,
                     int form = MW_FORM_STATE) {
  memset(&ref, 0, sizeof(ref));
  ref.form = form;
  memcpy(ref.W1, W1, sizeof(float) * 10 * n_in); memcpy(ref.b1, b1, sizeof(ref.b1)); memcpy(ref.W2, W2, sizeof(ref.W2)); memcpy(ref.b2, b2, sizeof(ref.b2));
  fill_scaling(n_in, scl_in, scl_out, ref.in_min, ref.in_rng, ref.out_min, ref.out_rng);
}
// launches the first kernel where the condition holds, else the second (a kernel template's two instantiations, each in parentheses):
// TEND of the forward kernels, ANYT of the bank's
#define MW_LAUNCH_IF(cond, KT, KF, ...) do { if (cond) hipLaunchKernelGGL(KT, __VA_ARGS__); else hipLaunchKernelGGL(KF, __VA_ARGS__); } while (0)

// the larger / smaller of two values, NaN if either is: a diverged model must not show a finite extremum (fmax / fmin would drop the NaN)
__device__ __forceinline__ double eval_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double eval_min(double a, double b) { return (b < a || b != b) ? b : a; }

// ---- the MFMA cell ----
__device__ __forceinline__ float leaky(float x) { return x > 0.f ? x : 0.1f * x; }                  // Relu(negative_slope = 0.1), :105

// min-max scaling as a multiply by the reciprocal range (the quotient is cast to fp32 right after: the <= 1 ulp fp64 difference is
// invisible at 24 bits except on exact rounding ties); fp64 math, stored as float (microphysics_kessler_ponni.h:182-186)
__device__ __forceinline__ float net_scaled(double x, double mn, double irng) {
#pragma clang fp contract(off)
  return (float)((x - mn) * irng);
}
// the reciprocal range of input row i: a division here, except in the bank's images, which hold that division's result
template <typename P> __device__ __forceinline__ double net_irng(const P &M, int i) { return 1.0 / M.in_rng[i]; }
__device__ __forceinline__ double net_irng(const EvalModel &M, int i) { return M.in_irng[i]; }

// A lane's operands of one model: filled once per (model, lane) by net5_ops / net9_ops from a model image -- the kernel-argument MlpP /
// StencilP, or the bank's EvalModel in LDS -- in the order the kernels have always loaded them (the order is part of their code).
struct NetOut { float a20, a21, a22; f32x4 c2; double omin, orng; };                                 // layer 2 and the un-scaling of lane group g
struct Net5 : NetOut { float a10, a11; f32x4 c1; double imin, irng, imin4, irng4; };                 // + single cell, layer 1: feature g, and rho_r (group 0)
struct Net9 : NetOut { float a10, a11, a12e, a12o; f32x4 c1;                                         // + stencil sweep, layer 1: feature g, its level
                       double imin, irng, amin, arng, rmin, rrng, ramin, rarng; };                   //   above, rho_r as feature 4 / 8

template <typename P> __device__ __forceinline__ void net5_ops(Net5 &n, const P &M, int lane, int g) {
  n.imin = M.in_min[g]; n.irng = net_irng(M, g); n.imin4 = M.in_min[4]; n.irng4 = net_irng(M, 4);
  n.omin = M.out_min[g]; n.orng = M.out_rng[g];
  n.a10 = M.a1[0][lane]; n.a11 = M.a1[1][lane];
  n.a20 = M.a2[0][lane]; n.a21 = M.a2[1][lane]; n.a22 = M.a2[2][lane];
  n.c1 = (f32x4){M.c1[g][0], M.c1[g][1], M.c1[g][2], M.c1[g][3]};
  n.c2 = (f32x4){M.c2[g], 0.f, 0.f, 0.f};
}
template <typename P> __device__ __forceinline__ void net9_ops(Net9 &n, const P &M, int lane, int g) {
  const int fa3 = (g == 3) ? 7 : 1, fa2 = (g == 2) ? 6 : fa3;             // the feature this lane's field is one level down: 5, -, 6, 7 (group 1
  const int fa = (g == 0) ? 5 : fa2;                                      // has none and takes row 1; its A operand is zero)
  n.imin = M.in_min[g]; n.irng = net_irng(M, g); n.amin = M.in_min[fa]; n.arng = net_irng(M, fa);
  n.rmin = M.in_min[4]; n.rrng = net_irng(M, 4); n.ramin = M.in_min[8]; n.rarng = net_irng(M, 8);
  n.omin = M.out_min[g]; n.orng = M.out_rng[g];
  n.a10 = M.a1[0][lane]; n.a11 = M.a1[1][lane]; n.a12e = M.a1[2][lane]; n.a12o = M.a1[3][lane];
  n.a20 = M.a2[0][lane]; n.a21 = M.a2[1][lane]; n.a22 = M.a2[2][lane];
  n.c1 = (f32x4){M.c1[g][0], M.c1[g][1], M.c1[g][2], M.c1[g][3]};
  n.c2 = (f32x4){M.c2[g], 0.f, 0.f, 0.f};
}

// the three layer-2 MFMAs of a C init and three hidden rows: k-slot g of MFMA j is register j of group g
__device__ __forceinline__ f32x4 net_layer2(const NetOut &n, float h0, float h1, float h2) {
  f32x4 d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(n.a20, h0, n.c2, 0, 0, 0);
  d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(n.a21, h1, d2, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(n.a22, h2, d2, 0, 0, 0);
}
// leaky ReLU, layer 2, un-scaling and clip: what lane group g stores for its output (:105-110, :198-201)
__device__ __forceinline__ double net_out(const NetOut &n, int g, f32x4 d1) {
#pragma clang fp contract(off)
  const f32x4 d2 = net_layer2(n, leaky(d1[0]), leaky(d1[1]), leaky(d1[2]));
  double y = (double)d2[0] * n.orng + n.omin;
  if (g != 0) y = fmax(0.0, y);
  return y;
}
// the TENDENCY form of the same: the un-scaled output is the change d of output g, added in fp64 to `base`, the cell's own value of the
// field that output g replaces (temp, rho_v, rho_c, rho_r: input features 0, 2, 3, 4 of the cell's own level), then the clip.  This
// association, no contraction: y = base + ((double)o * rng + min).
__device__ __forceinline__ double net_out_tendency(const NetOut &n, int g, f32x4 d1, double base) {
#pragma clang fp contract(off)
  const f32x4 d2 = net_layer2(n, leaky(d1[0]), leaky(d1[1]), leaky(d1[2]));
  const double d = (double)d2[0] * n.orng + n.omin;
  double y = base + d;
  if (g != 0) y = fmax(0.0, y);
  return y;
}
// either, by a wave-uniform flag (TEND: a compile-time switch that leaves the state form's code as it is where it is false)
template <bool TEND> __device__ __forceinline__ double net_out_form(const NetOut &n, int g, f32x4 d1, int form, double base) {
  if (TEND && form != MW_FORM_STATE) return net_out_tendency(n, g, d1, base);
  return net_out(n, g, d1);
}
// How the single-cell MFMA kernels bring the base to lane groups 1..3.  0: one more 8-byte load per lane, of a line that
// another group of the wave loads in the same iteration.  1: a 16-lane rotate of what the wave holds already -- group g's base is group
// g + 1's own field (rho_v, rho_c) and group 3's is group 0's rho_r: lane l takes it from lane (l + 16) & 63, no memory instruction.
// Measured (13.9): the rotate is the faster one in the forward kernels k_mlp / k_mlp_x2, the load in k_members_apply; the same bits.
#ifndef MW_TENDENCY_ROTATE_FORWARD
#define MW_TENDENCY_ROTATE_FORWARD 1
#endif
#ifndef MW_TENDENCY_ROTATE_APPLY
#define MW_TENDENCY_ROTATE_APPLY 0
#endif
// x4 of a tendency cell by the rotate: group 0 keeps rho_r, the others receive their base (every lane of the wave must call it)
__device__ __forceinline__ double net5_rotate_base(int g, double x, double x4) {
  const double got = __shfl(g == 0 ? x4 : x, (int)((threadIdx.x + 16) & 63), 64);
  return g == 0 ? x4 : got;
}
// layer 1 of the single-cell network on raw inputs: x = field g, x4 = rho_r (used by group 0)
__device__ __forceinline__ f32x4 net5_layer1(const Net5 &n, int g, double x, double x4) {
  const float b0 = net_scaled(x, n.imin, n.irng);
  const float b1 = (g == 0) ? net_scaled(x4, n.imin4, n.irng4) : 0.f;
  f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(n.a10, b0, n.c1, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(n.a11, b1, d1, 0, 0, 0);
}
// the single-cell network: the state form, and either form.  x4 is rho_r in group 0 alone, so in the other groups the same register
// carries the group's base field (rho_v, rho_c, rho_r): group 0's base is x itself.
__device__ __forceinline__ double net5_cell(const Net5 &n, int g, double x, double x4) { return net_out(n, g, net5_layer1(n, g, x, x4)); }
template <bool TEND> __device__ __forceinline__ double net5_cell_form(const Net5 &n, int g, double x, double x4, int form) {
  return net_out_form<TEND>(n, g, net5_layer1(n, g, x, x4), form, g == 0 ? x : x4);
}
// the stencil sweep's operands of level k from raw values: field g of level k, of the level above, and this group's latest rho_r -- of
// level k (feature 4) in group k & 1, of level k + 1 (feature 8) in the other of groups 0 / 1
__device__ __forceinline__ float net9_b0(const Net9 &n, double x) { return net_scaled(x, n.imin, n.irng); }
__device__ __forceinline__ float net9_above(const Net9 &n, double x) { return net_scaled(x, n.amin, n.arng); }
__device__ __forceinline__ float net9_b2(const Net9 &n, int g, int k, double rr) {
  return (g < 2) ? (g == (k & 1) ? net_scaled(rr, n.rmin, n.rrng) : net_scaled(rr, n.ramin, n.rarng)) : 0.f;
}
// layer 1 of the stencil sweep from scaled operands (a kernel that serves one model carries `above` scaled, one that loops over models
// carries it raw and scales it per model: the same expressions either way); net_out finishes the cell
__device__ __forceinline__ f32x4 net9_layer1(const Net9 &n, int k, float b0, float above, float b2) {
  f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(n.a10, b0, n.c1, 0, 0, 0);
  d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(n.a11, above, d1, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32((k & 1) ? n.a12o : n.a12e, b2, d1, 0, 0, 0);
}

// ---- the strict cell: plain fp32 loops in INDEX ORDER, no contraction -- the order in which the layers are defined (Matvec, Bias, Relu,
// Matvec, Bias; microphysics_kessler_ponni.h:103-110) and in which the CPU restatement accumulates: bit-identical to it.
//   NIN: 5 or 9; R: an MlpRef / StencilRef lvalue (kernel argument or LDS); in: the features, double[>= NIN]; y0..y3: the four destinations,
//   written directly (temp as it is, the three water fields clipped at 0).  TEND (MW_STRICT_CELL_FORM): a condition, constant or
//   uniform; where it holds, y = in[base] + (o * rng + min) in fp64 with base = 0, 2, 3, 4, the same clip.  MW_STRICT_CELL is the state form.
// A macro and not a function on purpose.  A function takes R by reference, and the table of a kernel that gets it as an ARGUMENT then
// stays an addressable copy until the call is inlined; the optimiser splits that copy into its 156 scalars before it can see that they
// are kernel-argument loads (k_mlp_stencil_strict: 164 SGPR spills, occupancy 8 -> 7; every other strict kernel scheduled differently).
// Expanded in place, the cell is the text the kernels always had, and their code stays what it was. ----
#define MW_STRICT_CELL_FORM(NIN, R, in, TEND, y0, y1, y2, y3)                                                                   \
  {                                                                                                                             \
    _Pragma("clang fp contract(off)")                                                                                           \
    float x_[NIN], h_[10], o_[4];                                                                                               \
    _Pragma("unroll")                                                                                                           \
    for (int i_ = 0; i_ < NIN; i_++) x_[i_] = (float)(((in)[i_] - (R).in_min[i_]) / (R).in_rng[i_]);   /* :182-186 (fp64, stored to float) */ \
    _Pragma("unroll")                                                                                                           \
    for (int o = 0; o < 10; o++) {                                                                                              \
      float acc = 0.f;                                                                                                          \
      _Pragma("unroll")                                                                                                         \
      for (int i_ = 0; i_ < NIN; i_++) acc += x_[i_] * (R).W1[i_ * 10 + o];                                                     \
      acc = acc + (R).b1[o];                                                                                                    \
      h_[o] = acc > 0.f ? acc : 0.1f * acc;                                                                                     \
    }                                                                                                                           \
    _Pragma("unroll")                                                                                                           \
    for (int o = 0; o < 4; o++) {                                                                                               \
      float acc = 0.f;                                                                                                          \
      _Pragma("unroll")                                                                                                         \
      for (int i_ = 0; i_ < 10; i_++) acc += h_[i_] * (R).W2[i_ * 4 + o];                                                       \
      o_[o] = acc + (R).b2[o];                                                                                                  \
    }                                                                                                                           \
    if (TEND) {                                 /* the tendency form: the cell's own temp, rho_v, rho_c, rho_r + the un-scaled change */ \
      (y0) =           (in)[0] + (o_[0] * (R).out_rng[0] + (R).out_min[0]);                                                     \
      (y1) = fmax(0.0, (in)[2] + (o_[1] * (R).out_rng[1] + (R).out_min[1]));                                                    \
      (y2) = fmax(0.0, (in)[3] + (o_[2] * (R).out_rng[2] + (R).out_min[2]));                                                    \
      (y3) = fmax(0.0, (in)[4] + (o_[3] * (R).out_rng[3] + (R).out_min[3]));                                                    \
    } else {                                                                                                                    \
      (y0) =           o_[0] * (R).out_rng[0] + (R).out_min[0];                                        /* :198-201 */           \
      (y1) = fmax(0.0, o_[1] * (R).out_rng[1] + (R).out_min[1]);                                                                \
      (y2) = fmax(0.0, o_[2] * (R).out_rng[2] + (R).out_min[2]);                                                                \
      (y3) = fmax(0.0, o_[3] * (R).out_rng[3] + (R).out_min[3]);                                                                \
    }                                                                                                                           \
  }
#define MW_STRICT_CELL(NIN, R, in, y0, y1, y2, y3) MW_STRICT_CELL_FORM(NIN, R, in, false, y0, y1, y2, y3)

} // namespace mw
