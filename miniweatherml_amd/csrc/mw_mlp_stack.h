// =====================================================================================================
// mw_mlp_stack.h -- what the units that run a dense surrogate stack share (mw_mlp_stack.hip: the handle and mw_mlp_stack_forward on
// level-major fields; mw_stack_members.hip: groups of stacks as ensemble members on the member-fastest layout): the kernels' parameter
// struct, the leaky ReLU, one Dense layer of MFMA tiles from LDS images, the host's image builder and the handle itself.  Only inline
// functions, templates and plain structs: every kernel is emitted from one unit.  The tile layout is described in mw_mlp_stack.hip.
// =====================================================================================================
#pragma once
#include "mw_mlp_net.h"
#include "mw_stack_shape.h"                                         // the shape limits (MW_STACK_*) and their check
#include <vector>

#define MW_STACK_PAD (64 * (MW_STACK_UB - 1))                      // floats behind the image in LDS: a layer with fewer unit blocks reads (and drops) up to here

namespace mw {

// what both kernels take by value; the MFMA kernel reads the layer tables (nk, nob, aoff, boff: of the image), the strict one the
// widths and the offsets of W and b in the parameters as they came
struct StackP {
  int n_in, nl;                                                    // nl Dense layers: the hidden ones and Dense(4)
  int nk[MW_STACK_DENSE], nob[MW_STACK_DENSE];                     // MFMAs along K = ceil(H_in / 4), unit blocks = ceil(H_out / 16)
  int aoff[MW_STACK_DENSE], boff[MW_STACK_DENSE];                  // float offsets in the image: A operands [ki][ob][lane], bias [ob][row]
  int width[MW_STACK_DENSE + 1], woff[MW_STACK_DENSE], bwoff[MW_STACK_DENSE];
  float slope[MW_STACK_DENSE];
  int nimg;
  double in_min[9], in_rng[9], out_min[4], out_rng[4];
};

__device__ __forceinline__ float leaky_slope(float x, float slope) {
#pragma clang fp contract(off)
  return x > 0.f ? x : slope * x;
}

// One Dense layer of TILES tiles from LDS images: d[ob][u] = bias, then nk * nob A operands, each feeding TILES MFMAs.  The loops are
// unrolled over the largest model and guarded by wave-uniform conditions, so that every register index is a constant; NOB = 1 is the
// last layer (one unit block, no guard).  The A operands of a K step are read ahead of its MFMAs, all MW_STACK_UB of them: a layer with
// fewer blocks reads the next step's (or the pad) and drops them.
template <int TILES, int NOB>
__device__ __forceinline__ void stack_dense(f32x4 (&d)[NOB][TILES], const f32x4 (&a)[MW_STACK_UB][TILES], const float *A, const float *B, int nk, int nob,
                                            int lane, int g) {
#pragma unroll
  for (int ob = 0; ob < NOB; ob++) {
    if (NOB == 1 || ob < nob) {
      const f32x4 c = *(const f32x4 *)(B + ob * 16 + 4 * g);
#pragma unroll
      for (int u = 0; u < TILES; u++) d[ob][u] = c;
    }
  }
#pragma unroll
  for (int ki = 0; ki < MW_STACK_MAX_WIDTH / 4; ki++) {
    if (ki < nk) {
      float w[NOB];
#pragma unroll
      for (int ob = 0; ob < NOB; ob++) w[ob] = A[(ki * nob + ob) * 64 + lane];
#pragma unroll
      for (int ob = 0; ob < NOB; ob++) {
        if (NOB == 1 || ob < nob) {
#pragma unroll
          for (int u = 0; u < TILES; u++) d[ob][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ob], a[ki / 4][u][ki % 4], d[ob][u], 0, 0, 0);
        }
      }
    }
  }
}

// The image of one Dense layer n_i -> n_o (W (n_i, n_o) in Keras order, b (n_o)): A operands [ki][ob][lane], then the bias [ob][row].
// Lane (r, g') of MFMA ki holds W[4 ki + g'][u] for the unit u of block ob at row r; zero where the input or the unit does not exist.
static void stack_images(std::vector<float> &img, const float *W, const float *b, int n_i, int n_o, int &aoff, int &boff) {
  const int nk = (n_i + 3) / 4, nob = (n_o + 15) / 16;
  auto unit_at = [](int ob, int r) { return 16 * ob + 4 * (r % 4) + r / 4; };
  aoff = (int)img.size();
  for (int ki = 0; ki < nk; ki++)
    for (int ob = 0; ob < nob; ob++)
      for (int lane = 0; lane < 64; lane++) {
        const int in = 4 * ki + (lane >> 4), u = unit_at(ob, lane & 15);
        img.push_back((in < n_i && u < n_o) ? W[in * n_o + u] : 0.f);
      }
  boff = (int)img.size();
  for (int ob = 0; ob < nob; ob++)
    for (int r = 0; r < 16; r++) { const int u = unit_at(ob, r); img.push_back(u < n_o ? b[u] : 0.f); }
}

} // namespace mw

struct mw_mlp_stack_s {
  mw::StackP P;
  int form;
  float *img, *params;                                                    // DEVICE: the MFMA image, the parameters as they came
};
