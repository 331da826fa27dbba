// =====================================================================================================
// mw_train_stack.hip -- native training of a dense surrogate stack n_in -> H1 -> ... -> HL -> 4 (the shapes mw_mlp_stack_create accepts):
// loss mse, Keras-Nadam, fit(batch_size, shuffle=True), optional sample weights -- the semantics of mw_train.hip for the fixed models.
// DESIGN.md section 13.19.
//
// k_stack_train: ONE workgroup (256 threads = 4 waves) per model, the epoch's batches loop inside, one launch per epoch.  The parameters
// sit in LDS for the whole epoch, ONE copy in Keras order (W (in, out) row-major with a padded row stride S = 4 * odd, then the biases):
// the forward pass reads it as W[k][u], the backward pass as W[u][k]; with S = 4 * odd the 16 units x 4 k-slots of a transposed read
// fall into 64 different banks.  Cells of the padding are never read: every operand read is guarded by the layer's real widths, and a
// unit or an input that does not exist contributes an exact zero.  So nothing that is padding has a gradient, a moment or a file entry.
//
// Every step of a batch of B samples has two phases on v_mfma_f32_16x16x4_f32 (fp32 operands and accumulation):
//
// Phase A (samples on the N axis).  A wave takes tiles of 16 samples (tile = wave, wave + 4, ...).  Forward with the chaining rule of
// mw_mlp_stack.hip: unit u of a layer at row 4 (u % 4) + (u % 16) / 4 of block u / 16, so that register j of lane group g of block m
// holds unit 16 m + 4 j + g = k-slot g of MFMA 4 m + j of the next layer: the D registers are the next B operands, no lane movement, the
// activations travel from layer to layer in registers (of a finished layer the wave keeps one bit per unit, "pre > 0").  r = out - t (times the sample's weight in the weighted instantiation), then back:
// delta_l = leaky'(pre_l) * (W_{l+1} delta_{l+1}) by the same rule with the roles of inputs and units exchanged (act > 0 <=> pre > 0,
// because a slope is >= 0).  The wave writes each sample's row into the model's workspace (global, sample-major, RS floats per sample):
//   [X block (16) | act_1 .. act_L (16 per unit block) | delta_1 .. delta_L (the same) | delta_out (16)]
// Position 4 g + j of a block holds unit 4 j + g of it -- the D layout as it is, so a lane stores its four registers as ONE 16-byte
// vector and a sample's block is 64 contiguous bytes.  The X block carries a constant 1 at feature n_in (the ones column), delta_out
// carries sum_o r_o^2 and sum_o |r_o| of the sample (times its weight) at the positions of the non-existent output units 4 and 8.
// A sample beyond a partial batch writes a row of zeros (its x, its ones entry, its activations and its r are zeroed).
//
// Phase B (samples on the K axis), after one workgroup barrier.  dW_l = a_{l-1}^T delta_l is a set of 16 x 16 tiles.  A "tile row" is one
// input block of a layer with ALL its output blocks (the A operand is loaded once per four samples and feeds up to four MFMAs); the
// bias gradients of a layer are row n_in of the tile row [X block]^T delta_l (for the first layer that is the weights' own tile row),
// and the two sums ride in the last layer's.  Tile rows are dealt to the four waves round-robin; a wave reduces its tiles over the whole
// batch in sample order, so the order is fixed, there is no cross-wave sum, and a model's bits do not depend on the launch, on the
// number of models or on the CU.  The lane that holds a tile entry owns that parameter: it reads the two Nadam moments from the global
// arrays, runs k_surrogate_train's fp32 expressions, writes the moments back and the new weight to LDS.  A second barrier ends the step.
//
// LDS: the largest shape 9 -> 64 -> 64 -> 64 -> 64 -> 4 needs its 136 shape words + 14,260 floats + LDS_PAD = 61,680 B (dynamic, below the 64 KB every kernel here
// stays under); the moments (two more copies) stay in global memory, read and written once per step.
// =====================================================================================================
#include "mw_mlp_net.h"
#include "mw_feistel.h"
#include "mw_stack_shape.h"
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <algorithm>

namespace mw {
namespace stk {

constexpr int TPB = 256;
constexpr int MAXROWS = 1 + MW_STACK_MAX_HIDDEN * (MW_STACK_UB + 1);      // the first layer's tile row; per later Dense four input blocks and the ones row
constexpr int MAX_LDS_BYTES = 64 * 1024;
// floats behind the parameters in LDS: an operand read of a lane whose unit or k-slot does not exist is issued all the same (dense_fwd);
// it reaches at most 14 rows and 14 floats past the layer, rows of at most 68 floats
constexpr int LDS_PAD = 15 * (MW_STACK_MAX_WIDTH + 4) + 4;

struct Row { int l, ib, acol, ones; };                                   // Dense l, input block ib (-1: the ones row alone), workspace column of its A block
struct Shape {                                                            // 32-bit words only: the kernels read it word by word (Tab)
  int n_in, nh;                                                           // nh hidden layers: Dense 0 .. nh
  int width[MW_STACK_DENSE + 1];                                          // n_in, H1 .. HL, 4
  float slope[MW_STACK_MAX_HIDDEN];
  int lw[MW_STACK_DENSE], lb[MW_STACK_DENSE], S[MW_STACK_DENSE];          // LDS (floats): W_l, b_l, the row stride of W_l
  int gw[MW_STACK_DENSE], gb[MW_STACK_DENSE];                             // the flat Keras vector: W_l, b_l
  int acol[MW_STACK_MAX_HIDDEN], dcol[MW_STACK_DENSE];                    // workspace columns: act of hidden layer l, delta of Dense l
  int RS, nparams, nlds, nrows;
  Row rows[MAXROWS];
};
constexpr int SHAPE_WORDS = (int)((sizeof(Shape) / 4 + 3) / 4 * 4);        // the shape's copy at the head of LDS, the parameters behind it
// The shape as the device functions see it: its words in LDS, each read where it is used and made wave-uniform.  The kernel argument
// itself would be loop-invariant: the compiler then keeps every word, every offset and every lane mask derived from them in scalar
// registers across the step, tile and layer loops, far more than there are.  A volatile LDS word is read again instead (a layer reads
// about ten per 16-sample tile, beside its 16 to 256 MFMAs).
struct Tab {
  const volatile int *w;
  __device__ __forceinline__ int i(int off) const { return __builtin_amdgcn_readfirstlane(w[off]); }
  __device__ __forceinline__ float f(int off) const { return __int_as_float(i(off)); }
};
#define TI(field, idx) T.i((int)(offsetof(Shape, field) / 4) + (idx))
#define TROW(t, member) T.i((int)((offsetof(Shape, rows) + offsetof(Row, member)) / 4) + 4 * (t))
struct SetRef { const float *x, *y; long long n; };
struct Identity { __device__ long long operator()(long long p) const { return p; } };
struct Shuffled { Feistel F; __device__ long long operator()(long long p) const { return feistel_index(F, p); } };

__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// d[ob] += sum_k A(k, unit) b(k) with the units at their chained rows (lane row r holds unit 16 ob + 4 (r % 4) + r / 4) and k = 4 ki + g
// the lane's k-slot.  Unrolled over the largest layer and guarded by wave-uniform conditions, so that every register index is a constant.
// What a lane reads for a unit or a k-slot that does not exist is a finite number -- another row's weights, or a cell of the row padding
// or of LDS_PAD, which the kernels fill with zeros and never write again.  The A operand of a unit that does not exist is that number
// times the lane's 0.f (oku: 1.f or 0.f per unit block; a multiply, because 16 lane masks per layer cost the kernel its scalar registers):
// an exact zero.  A k-slot that does not exist needs no guard: its B operand is an exact zero (a padded input, a padded unit's
// activation or delta).
// For the same reason the k axis is guarded per block of 16 (four MFMAs) only: up to three MFMAs of a block add exact zeros.
// dense_fwd: A(k, unit) = W[k][unit], k over the n_i inputs (KB blocks of KJ MFMAs at most).  The pointer walks down the rows; the unit
// block is an immediate offset.
template <int KB, int KJ>
__device__ __forceinline__ void dense_fwd(f32x4 (&d)[MW_STACK_UB], const f32x4 (&b)[MW_STACK_UB], const float *W, int S, int n_i, int n_o, int r, int g) {
  const int nkb = (n_i + 15) >> 4, nob = (n_o + 15) >> 4, up = 4 * (r & 3) + (r >> 2);
  const float *p = W + g * S + up;
  float oku[MW_STACK_UB];
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) oku[ob] = 16 * ob + up < n_o ? 1.f : 0.f;
#pragma unroll
  for (int kb = 0; kb < KB; kb++) {
    if (kb < nkb) {
#pragma unroll
      for (int j = 0; j < KJ; j++) {
#pragma unroll
        for (int ob = 0; ob < MW_STACK_UB; ob++)
          if (ob < nob) d[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(oku[ob] * p[16 * ob], b[kb][j], d[ob], 0, 0, 0);
        p += 4 * S;
      }
    }
  }
}
// dense_bwd: A(k, unit) = W[unit][k], k over the n_o outputs of the same Dense, the units its n_i inputs.  One pointer per unit block; the
// k step is an immediate offset (k-slots from n_o on lie in the row padding, then in the next row).
__device__ __forceinline__ void dense_bwd(f32x4 (&d)[MW_STACK_UB], const f32x4 (&b)[MW_STACK_UB], const float *W, int S, int n_i, int n_o, int r, int g) {
  const int nkb = (n_o + 15) >> 4, nob = (n_i + 15) >> 4, up = 4 * (r & 3) + (r >> 2);
  const float *q[MW_STACK_UB];
  float oku[MW_STACK_UB];
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) { q[ob] = W + (16 * ob + up) * S + g; oku[ob] = 16 * ob + up < n_i ? 1.f : 0.f; }
#pragma unroll
  for (int kb = 0; kb < MW_STACK_UB; kb++) {
    if (kb < nkb) {
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int ob = 0; ob < MW_STACK_UB; ob++)
          if (ob < nob) d[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(oku[ob] * q[ob][16 * kb + 4 * j], b[kb][j], d[ob], 0, 0, 0);
    }
  }
}

// the block's four registers of one sample as one 16-byte vector (zeros for a sample beyond the batch)
__device__ __forceinline__ void put(float *row, int col, int g, bool ok, f32x4 v) { *(f32x4 *)(row + col + 4 * g) = ok ? v : zero4(); }

// bias of Dense l as the C operand: register j of group g of block ob is unit 16 ob + 4 j + g (b: padded with zeros to whole blocks)
__device__ __forceinline__ void bias_init(f32x4 (&d)[MW_STACK_UB], const float *b, int n_o, int g) {
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) {
    d[ob] = zero4();
    if (16 * ob < n_o) {
#pragma unroll
      for (int j = 0; j < 4; j++) d[ob][j] = b[16 * ob + 4 * j + g];
    }
  }
}

// hidden layer l (Dense l, then the leaky ReLU): cur -> the layer's activations, stored into the sample's row; bit 16 l + 4 ob + j of
// mask keeps "pre > 0" of register j of block ob, which is all the backward pass needs of the layer
template <int KB, int KJ, bool STORE = true>
__device__ __forceinline__ void hidden_forward(const Tab &T, const float *lds, int l, f32x4 (&cur)[MW_STACK_UB], uint64_t &mask, float *row, bool ok,
                                               int c, int g) {
  const int n_i = TI(width, l), n_o = TI(width, l + 1);
  const float slope = T.f((int)(offsetof(Shape, slope) / 4) + l);
  f32x4 d[MW_STACK_UB];
  bias_init(d, lds + TI(lb, l), n_o, g);
  dense_fwd<KB, KJ>(d, cur, lds + TI(lw, l), TI(S, l), n_i, n_o, c, g);
  const int acol = STORE ? TI(acol, l) : 0;
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool pos = d[ob][j] > 0.f;
      cur[ob][j] = pos ? d[ob][j] : slope * d[ob][j];
      mask |= (uint64_t)pos << (16 * l + 4 * ob + j);
    }
    if (STORE && 16 * ob < n_o) put(row, acol + 16 * ob, g, ok, cur[ob]);
  }
}

// delta of hidden layer l from the delta behind it (dcur: of Dense l + 1's outputs), stored; becomes dcur
__device__ __forceinline__ void hidden_backward(const Tab &T, const float *lds, int l, f32x4 (&dcur)[MW_STACK_UB], uint64_t mask, float *row, int c,
                                                int g) {
  const int n_i = TI(width, l + 1), n_o = TI(width, l + 2), dcol = TI(dcol, l);
  const float slope = T.f((int)(offsetof(Shape, slope) / 4) + l);
  f32x4 d[MW_STACK_UB];
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) d[ob] = zero4();
  dense_bwd(d, dcur, lds + TI(lw, l + 1), TI(S, l + 1), n_i, n_o, c, g);
#pragma unroll
  for (int ob = 0; ob < MW_STACK_UB; ob++) {
#pragma unroll
    for (int j = 0; j < 4; j++) d[ob][j] = ((mask >> (16 * l + 4 * ob + j)) & 1) ? d[ob][j] : slope * d[ob][j];
    if (16 * ob < n_i) put(row, dcol + 16 * ob, g, true, d[ob]);       // (a masked sample's r is zero, so its deltas are)
    dcur[ob] = d[ob];
  }
}

// Phase A of one batch: the samples at positions first .. first + B - 1 of `pos`, rows 0 .. 16 ceil(B / 16) - 1 of the workspace
template <bool WEIGHTED, class Pos>
__device__ __forceinline__ void phase_a(const Tab &T, const float *lds, const SetRef &S, const float *wt, const Pos &pos, long long first, int B,
                                        float *ws) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
  const int ntiles = (B + 15) >> 4;
  for (int tile = wave; tile < ntiles; tile += TPB / 64) {
    const int i = 16 * tile + c, nh = TI(nh, 0), n_in = TI(n_in, 0);
    const bool ok = i < B;
    const long long idx = ok ? pos(first + i) : 0;
    f32x4 x = zero4();
    x[0] = ok ? S.x[g * S.n + idx] : 0.f;                                 // feature 4 j + g in register j
    if (ok && 4 + g < n_in) x[1] = S.x[(4 + g) * S.n + idx];
    if (ok && 8 + g < n_in) x[2] = S.x[(8 + g) * S.n + idx];
    const float t = ok ? S.y[g * S.n + idx] : 0.f;
    float *row = ws + (size_t)i * TI(RS, 0);
    f32x4 xs = x;                                                         // the stored X block: the ones column at feature n_in (5: j 1, g 1; 9: j 2, g 1)
    if (g == (n_in & 3)) { if (n_in == 5) xs[1] = 1.f; else xs[2] = 1.f; }
    put(row, 0, g, ok, xs);

    f32x4 cur[MW_STACK_UB];
    uint64_t mask = 0;
    cur[0] = x;
#pragma unroll
    for (int ob = 1; ob < MW_STACK_UB; ob++) cur[ob] = zero4();
    hidden_forward<1, 3>(T, lds, 0, cur, mask, row, ok, c, g);
#pragma unroll 1
    for (int l = 1; l < nh; l++) hidden_forward<MW_STACK_UB, 4>(T, lds, l, cur, mask, row, ok, c, g);
    f32x4 o[MW_STACK_UB];                                                 // Dense(4): output g in register 0 of group g
    bias_init(o, lds + TI(lb, nh), 4, g);
    dense_fwd<MW_STACK_UB, 4>(o, cur, lds + TI(lw, nh), TI(S, nh), TI(width, nh), 4, c, g);
    const float r = o[0][0] - t;
    float sq = r * r, ab = fabsf(r);                                      // over the four outputs: (g0 + g1) + (g2 + g3) in every lane
    sq += __shfl_xor(sq, 16, 64); ab += __shfl_xor(ab, 16, 64);
    sq += __shfl_xor(sq, 32, 64); ab += __shfl_xor(ab, 32, 64);
    float dr = r;
    if constexpr (WEIGHTED) { const float w = ok ? wt[idx] : 0.f; dr *= w; sq *= w; ab *= w; }
    if (!ok) { dr = 0.f; sq = 0.f; ab = 0.f; }
    put(row, TI(dcol, nh), g, true, (f32x4){dr, g == 0 ? sq : 0.f, g == 0 ? ab : 0.f, 0.f});

    f32x4 dcur[MW_STACK_UB];
    dcur[0] = (f32x4){dr, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ob = 1; ob < MW_STACK_UB; ob++) dcur[ob] = zero4();
#pragma unroll 1
    for (int l = nh - 1; l >= 0; l--) hidden_backward(T, lds, l, dcur, mask, row, c, g);
  }
}

// Phase B of one batch: every tile entry that is a parameter goes to apply(global index, LDS index, raw sum over the batch), the two
// sums to stat(0 | 1, sum).  Raw: the gradient of mean((y - t)^2) is the sum times 0.5 / B.
template <class Apply, class Stat>
__device__ __forceinline__ void phase_b(const Tab &T, const float *ws, int B, Apply &&apply, Stat &&stat) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
  const int ksteps = ((B + 15) >> 4) * 4;
  const int RS = TI(RS, 0), nrows = TI(nrows, 0), n_in = TI(n_in, 0), nh = TI(nh, 0);
  const size_t step = (size_t)4 * RS;
  for (int t = wave; t < nrows; t += TPB / 64) {
    const Row R{TROW(t, l), TROW(t, ib), TROW(t, acol), TROW(t, ones)};
    const int l = R.l, n_i = TI(width, l), n_o = TI(width, l + 1), nob = (n_o + 15) >> 4;
    f32x4 acc[MW_STACK_UB];
#pragma unroll
    for (int ob = 0; ob < MW_STACK_UB; ob++) acc[ob] = zero4();
    const float *pa = ws + (size_t)g * RS + R.acol + c, *pd = ws + (size_t)g * RS + TI(dcol, l) + c;
#pragma unroll 16
    for (int ks = 0; ks < ksteps; ks++) {                                  // samples 4 ks + g: in order, the reduction order of every entry
      const float a = pa[ks * step];
#pragma unroll
      for (int ob = 0; ob < MW_STACK_UB; ob++)
        if (ob < nob) acc[ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pd[ks * step + 16 * ob], acc[ob], 0, 0, 0);
    }
    const int ocol = 4 * (c & 3) + (c >> 2);                               // the unit at column position c of a block
    const int gw = TI(gw, l), gb = TI(gb, l), lw = TI(lw, l), lb = TI(lb, l), S = TI(S, l);
#pragma unroll
    for (int ob = 0; ob < MW_STACK_UB; ob++) {
      if (ob < nob) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int f = 4 * j + g, iu = 16 * (R.ib > 0 ? R.ib : 0) + f, o = 16 * ob + ocol;    // row position 4 g + j holds unit 4 j + g
          if (o < n_o) {
            if (R.ib >= 0 && iu < n_i) apply(gw + iu * n_o + o, lw + iu * S + o, acc[ob][j]);
            else if (R.ones && f == n_in) apply(gb + o, lb + o, acc[ob][j]);
          } else if (R.ones && l == nh && f == n_in && (o == 4 || o == 8)) stat(o == 8, acc[ob][j]);
        }
      }
    }
  }
}

// The head of a kernel: the shape's words to the head of LDS, zeros behind them (the row padding and LDS_PAD stay zero for good), a
// barrier, then the parameters at their places.  Returns the table; the parameters' image starts SHAPE_WORDS floats into `smem`.
__device__ __forceinline__ Tab load_params(const Shape &K, float *smem, const float *params) {
  const int *kw = (const int *)&K;
  for (int e = threadIdx.x; e < SHAPE_WORDS; e += TPB) ((int *)smem)[e] = e < (int)(sizeof(Shape) / 4) ? kw[e] : 0;
  float *lds = smem + SHAPE_WORDS;
  for (int e = threadIdx.x; e < K.nlds + LDS_PAD; e += TPB) lds[e] = 0.f;
  __syncthreads();
  const Tab T{(const volatile int *)smem};
  const int nh = TI(nh, 0);
  for (int l = 0; l <= nh; l++) {
    const int n_i = TI(width, l), n_o = TI(width, l + 1), lw = TI(lw, l), lb = TI(lb, l), S = TI(S, l), gw = TI(gw, l), gb = TI(gb, l);
    for (int e = threadIdx.x; e < n_i * n_o; e += TPB) lds[lw + (e / n_o) * S + e % n_o] = params[gw + e];
    for (int e = threadIdx.x; e < n_o; e += TPB) lds[lb + e] = params[gb + e];
  }
  return T;
}
__device__ __forceinline__ void store_params(const Tab &T, const float *lds, float *params) {
  const int nh = TI(nh, 0);
  for (int l = 0; l <= nh; l++) {
    const int n_i = TI(width, l), n_o = TI(width, l + 1), lw = TI(lw, l), lb = TI(lb, l), S = TI(S, l), gw = TI(gw, l), gb = TI(gb, l);
    for (int e = threadIdx.x; e < n_i * n_o; e += TPB) params[gw + e] = lds[lw + (e / n_o) * S + e % n_o];
    for (int e = threadIdx.x; e < n_o; e += TPB) params[gb + e] = lds[lb + e];
  }
}

struct TrainArgs {
  SetRef S; const float *wt; int B; int epoch; uint64_t seed;
  float *params, *m1, *m2; const float *table; double *stats;
  float beta1, beta2, eps;
  float *ws; long long ws_model;                                          // the workspace, floats per model
};

} // namespace stk

template <bool WEIGHTED>
__global__ __launch_bounds__(stk::TPB) void k_stack_train(stk::Shape K, stk::TrainArgs a) {
  using namespace stk;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *lds = smem + SHAPE_WORDS;
  const int model = blockIdx.x;
  float *params = a.params + (size_t)model * K.nparams, *m1 = a.m1 + (size_t)model * K.nparams, *m2 = a.m2 + (size_t)model * K.nparams;
  float *ws = a.ws + (size_t)model * a.ws_model;
  const Tab T = load_params(K, smem, params);
  const Shuffled pos{make_feistel(a.seed + (uint64_t)model, (uint64_t)a.epoch, a.S.n)};
  const long long n = a.S.n, steps = (n + a.B - 1) / a.B;
  double sq = 0.0, ab = 0.0;
  int role = 0;                                                           // bit 0 / 1: this lane owns sum r^2 / sum |r| (the deal is the same every step)
  __syncthreads();
  for (long long s = 0; s < steps; s++) {
    const long long first = s * a.B;
    const int B = (int)std::min<long long>(a.B, n - first);
    phase_a<WEIGHTED>(T, lds, a.S, a.wt, pos, first, B, ws);
    __syncthreads();                                                      // the rows of all four waves are written
    const float cg = a.table[3 * s], cm = a.table[3 * s + 1], bc2 = a.table[3 * s + 2];
    const float scale = 0.5f / (float)B;                                  // d mean((y - t)^2) = 2 r / (4 B)
    phase_b(T, ws, B,
            [&](int gp, int lp, float gsum) {                             // Nadam (TF 2.x Keras): k_surrogate_train's expressions
              float w = lds[lp], m = m1[gp], v = m2[gp];
              const float gr = gsum * scale;
              m = a.beta1 * m + (1.f - a.beta1) * gr;
              v = a.beta2 * v + (1.f - a.beta2) * gr * gr;
              w -= (cg * gr + cm * m) / (sqrtf(v / bc2) + a.eps);
              m1[gp] = m; m2[gp] = v; lds[lp] = w;
            },
            [&](int which, float gsum) { if (which) { ab += (double)gsum; role |= 2; } else { sq += (double)gsum; role |= 1; } });
    __syncthreads();                                                      // the new weights are in LDS, the rows are free again
  }
  store_params(T, lds, params);
  if (role & 1) a.stats[2 * model] = sq;
  if (role & 2) a.stats[2 * model + 1] = ab;
}

// the forward pass alone on a set x (n_in, n) -> out (4, n), scaled label space: the trainer's validation and test predictions (the
// generic layer kernel of mw_ponni_forward stops at 32 units and 10 layers).  Tiles of 16 samples, grid-stride; the layers are Phase A's.
__global__ __launch_bounds__(stk::TPB) void k_stack_predict(stk::Shape K, const float *params, long long n, const float *x, float *out) {
  using namespace stk;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *lds = smem + SHAPE_WORDS;
  const Tab T = load_params(K, smem, params);
  __syncthreads();
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15, nh = TI(nh, 0), n_in = TI(n_in, 0);
  const long long ntiles = (n + 15) >> 4, wave = ((long long)blockIdx.x * TPB + threadIdx.x) >> 6, nwaves = (long long)gridDim.x * (TPB / 64);
  for (long long tile = wave; tile < ntiles; tile += nwaves) {
    const long long i = 16 * tile + c;
    const bool ok = i < n;
    f32x4 cur[MW_STACK_UB];
    uint64_t mask = 0;
#pragma unroll
    for (int ob = 0; ob < MW_STACK_UB; ob++) cur[ob] = zero4();
    cur[0][0] = ok ? x[g * n + i] : 0.f;
    if (ok && 4 + g < n_in) cur[0][1] = x[(4 + g) * n + i];
    if (ok && 8 + g < n_in) cur[0][2] = x[(8 + g) * n + i];
    hidden_forward<1, 3, false>(T, lds, 0, cur, mask, nullptr, ok, c, g);
#pragma unroll 1
    for (int l = 1; l < nh; l++) hidden_forward<MW_STACK_UB, 4, false>(T, lds, l, cur, mask, nullptr, ok, c, g);
    f32x4 o[MW_STACK_UB];
    bias_init(o, lds + TI(lb, nh), 4, g);
    dense_fwd<MW_STACK_UB, 4>(o, cur, lds + TI(lw, nh), TI(S, nh), TI(width, nh), 4, c, g);
    if (ok) out[g * n + i] = o[0][0];
  }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(stk::TPB) void k_stack_grad(stk::Shape K, const float *params, stk::SetRef S, const float *wt, int B, float *grad,
                                                         float *loss, float *ws) {
  using namespace stk;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *lds = smem + SHAPE_WORDS;
  const Tab T = load_params(K, smem, params);
  __syncthreads();
  phase_a<WEIGHTED>(T, lds, S, wt, Identity(), 0, B, ws);
  __syncthreads();
  const float scale = 0.5f / (float)B;
  phase_b(T, ws, B, [&](int gp, int lp, float gsum) { grad[gp] = gsum * scale; },
          [&](int which, float gsum) { if (!which) loss[0] = gsum / (4.f * (float)B); });
}

namespace stk {

// the shape's tables: LDS layout, workspace row, the deal of tile rows (host)
static int make_shape(const char *who, int n_in, int nhidden, const int *widths, const float *slopes, bool other_null, Shape &T) {
  long long need = 0;
  if (stack_shape_check(who, n_in, nhidden, widths, slopes, other_null, &need)) return 1;
  memset(&T, 0, sizeof(T));
  T.n_in = n_in; T.nh = nhidden; T.nparams = (int)need;
  T.width[0] = n_in;
  for (int l = 0; l < nhidden; l++) { T.width[l + 1] = widths[l]; T.slope[l] = slopes[l]; }
  T.width[nhidden + 1] = 4;
  int gp = 0, q = 0;
  for (int l = 0; l <= nhidden; l++) {
    const int n_i = T.width[l], n_o = T.width[l + 1];
    T.gw[l] = gp; T.gb[l] = gp + n_i * n_o; gp += (n_i + 1) * n_o;
    T.S[l] = 4 * (((n_o + 3) / 4) | 1);                                   // the smallest 4 * odd >= n_o
    T.lw[l] = q; q += n_i * T.S[l];
  }
  for (int l = 0; l <= nhidden; l++) { T.lb[l] = q; q += 16 * ((T.width[l + 1] + 15) / 16); }   // whole blocks: bias_init reads them unguarded
  T.nlds = q;
  if ((long long)(SHAPE_WORDS + q + LDS_PAD) * (long long)sizeof(float) > MAX_LDS_BYTES)
    MW_FAIL(std::string(who) + ": this shape needs " + std::to_string((SHAPE_WORDS + q + LDS_PAD) * sizeof(float)) + " B of LDS for its parameters, more than " + std::to_string(MAX_LDS_BYTES));
  int col = 16;
  for (int l = 0; l < nhidden; l++) { T.acol[l] = col; col += 16 * ((widths[l] + 15) / 16); }
  for (int l = 0; l < nhidden; l++) { T.dcol[l] = col; col += 16 * ((widths[l] + 15) / 16); }
  T.dcol[nhidden] = col; col += 16;
  T.RS = col;
  int nr = 0;
  T.rows[nr++] = Row{0, 0, 0, 1};
  for (int l = 1; l <= nhidden; l++) {
    for (int ib = 0; ib < (T.width[l] + 15) / 16; ib++) T.rows[nr++] = Row{l, ib, T.acol[l - 1] + 16 * ib, 0};
    T.rows[nr++] = Row{l, -1, 0, 1};
  }
  T.nrows = nr;
  return 0;
}

static long long ws_floats(const Shape &T, int batch) { return (long long)((batch + 15) / 16 * 16) * T.RS; }

} // namespace stk
} // namespace mw

using namespace mw;

extern "C" {

long long mw_stack_train_workspace_bytes(int n_in, int nhidden, const int *widths, int models, int batch) {
  static const float zeros[MW_STACK_MAX_HIDDEN] = {0.f, 0.f, 0.f, 0.f};
  stk::Shape T;
  if (stk::make_shape("stack_train_workspace_bytes", n_in, nhidden, widths, zeros, false, T)) return -1;
  if (models < 1 || models > MW_SURROGATE_MAX_MODELS || batch < 1 || batch > MW_SURROGATE_MAX_BATCH) {
    set_error("stack_train_workspace_bytes: models must be in [1, " + std::to_string(MW_SURROGATE_MAX_MODELS) + "] and batch in [1, " +
              std::to_string(MW_SURROGATE_MAX_BATCH) + "]");
    return -1;
  }
  return (long long)models * stk::ws_floats(T, batch) * (long long)sizeof(float);
}

int mw_stack_train_epoch(int n_in, int nhidden, const int *widths, const float *slopes, int models, const float *x, const float *y, const float *w,
                         long long n, int batch, int epoch, unsigned long long seed, float *params, float *m1, float *m2, const float *table,
                         float beta1, float beta2, float eps, double *stats, void *workspace, void *stream) {
  stk::Shape T;
  if (stk::make_shape("stack_train_epoch", n_in, nhidden, widths, slopes, !x || !y || !params || !m1 || !m2 || !table || !stats || !workspace, T)) return 1;
  if (models < 1 || models > MW_SURROGATE_MAX_MODELS) MW_FAIL("stack_train_epoch: models must be in [1, " + std::to_string(MW_SURROGATE_MAX_MODELS) + "]");
  if (batch < 1 || batch > MW_SURROGATE_MAX_BATCH) MW_FAIL("stack_train_epoch: batch must be in [1, " + std::to_string(MW_SURROGATE_MAX_BATCH) + "]");
  if (n < 1 || epoch < 0) MW_FAIL("stack_train_epoch: n must be >= 1 and epoch >= 0");
  if ((uintptr_t)workspace & 15) MW_FAIL("stack_train_epoch: the workspace must be 16-byte aligned");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  stk::TrainArgs a;
  a.S = stk::SetRef{x, y, n}; a.wt = w; a.B = batch; a.epoch = epoch; a.seed = seed;
  a.params = params; a.m1 = m1; a.m2 = m2; a.table = table; a.stats = stats;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.ws = (float *)workspace; a.ws_model = stk::ws_floats(T, batch);
  const size_t lds = sizeof(float) * (size_t)(stk::SHAPE_WORDS + T.nlds + stk::LDS_PAD);
  MW_LAUNCH_IF(w != nullptr, (k_stack_train<true>), (k_stack_train<false>), dim3((unsigned)models), dim3(stk::TPB), lds, (hipStream_t)stream, T, a);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_stack_batch_grad(int n_in, int nhidden, const int *widths, const float *slopes, const float *params, const float *x, const float *y,
                        const float *w, int batch, float *grad, float *loss, void *workspace, void *stream) {
  stk::Shape T;
  if (stk::make_shape("stack_batch_grad", n_in, nhidden, widths, slopes, !params || !x || !y || !grad || !loss || !workspace, T)) return 1;
  if (batch < 1 || batch > MW_SURROGATE_MAX_BATCH) MW_FAIL("stack_batch_grad: batch must be in [1, " + std::to_string(MW_SURROGATE_MAX_BATCH) + "]");
  if ((uintptr_t)workspace & 15) MW_FAIL("stack_batch_grad: the workspace must be 16-byte aligned");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const stk::SetRef S{x, y, (long long)batch};
  const size_t lds = sizeof(float) * (size_t)(stk::SHAPE_WORDS + T.nlds + stk::LDS_PAD);
  MW_LAUNCH_IF(w != nullptr, (k_stack_grad<true>), (k_stack_grad<false>), dim3(1), dim3(stk::TPB), lds, (hipStream_t)stream, T, params, S, w, batch, grad,
               loss, (float *)workspace);
  MW_LAUNCH_CHECK();
  return 0;
}

int mw_stack_predict(int n_in, int nhidden, const int *widths, const float *slopes, const float *params, long long n, const float *x, float *out,
                     void *stream) {
  stk::Shape T;
  if (stk::make_shape("stack_predict", n_in, nhidden, widths, slopes, !params || !x || !out, T)) return 1;
  if (n < 1) MW_FAIL("stack_predict: n must be >= 1");
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  const long long blocks = std::max<long long>(1, std::min<long long>(((n + 15) / 16 + 3) / 4, 1024));
  hipLaunchKernelGGL(k_stack_predict, dim3((unsigned)blocks), dim3(stk::TPB), sizeof(float) * (size_t)(stk::SHAPE_WORDS + T.nlds + stk::LDS_PAD), (hipStream_t)stream, T,
                     params, n, x, out);
  MW_LAUNCH_CHECK();
  return 0;
}

} // extern "C"
