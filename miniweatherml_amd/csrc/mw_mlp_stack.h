// =====================================================================================================
// mw_mlp_stack.h -- what the units that run a dense surrogate stack share (mw_mlp_stack.hip: the handle and mw_mlp_stack_forward on
// level-major fields; mw_stack_members.hip: groups of stacks as ensemble members on the member-fastest layout; mw_stack_eval.hip: groups
// of stacks scored against the truth fields; mw_stack_committee.hip: the mean and range of a selection of a group's stacks;
// mw_stack_guard.hip: that mean with the guard's column flags): the kernels' parameter struct, the leaky ReLU, one Dense layer of MFMA tiles from LDS
// images, the cell of a group's kernels (stack_cells), the host's image builder, the group's lists, the handles and a committee's plan.  Only inline
// functions, templates and plain structs: every kernel is emitted from one unit.  The tile layout is described in mw_mlp_stack.hip.
// =====================================================================================================
#pragma once
#include "mw_mlp_net.h"
#include "mw_stack_shape.h"                                         // the shape limits (MW_STACK_*) and their check
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#define MW_STACK_PAD (64 * (MW_STACK_UB - 1))                      // floats behind the image in LDS: a layer with fewer unit blocks reads (and drops) up to here
#define MW_STACK_EVAL_RED 4096                                     // bytes of static LDS of k_stack_eval's tail: red[stack 4][slot 4][group 4][8] doubles

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

// ---- what the units that run a GROUP of stacks share (mw_stack_members.hip: rollout members; mw_stack_eval.hip: the scorer) ----
#define MW_STACK_GROUP_MAX 32                                       // stacks of a group = members a call can address
#define MW_STACK_GROUP_LDS 65536                                    // bytes of dynamic LDS a workgroup's images may take together

struct StackRow { StackP P; int form, img_off, par_off, pad_; };   // img_off / par_off: floats, in the group's packed images / parameters
struct StackMap { int member[MW_STACK_GROUP_MAX]; };

// a lane's scaling constants of one stack: feature g, feature f1 (4 + g, or 4), feature 8, output g
struct StackLane { double imin0, irng0, imin1, irng1, imin2, irng2, omin, orng; };

// TILES tiles of one stack from raw features: x0 = feature g, x1 = feature 4 + g (n_in = 5: rho_r in group 0), x2 = feature 8 (group 0
// of n_in = 9).  k_mlp_stack's statements between its loads and its stores; every lane of the wave calls it (the rotate).
template <int TILES, bool N9>
__device__ __forceinline__ void stack_cells(double (&y)[TILES], const StackP *P, const float *img, const StackLane &S, bool tend, int lane, int g,
                                            const double (&x0)[TILES], const double (&x1)[TILES], const double (&x2)[TILES]) {
#pragma clang fp contract(off)
  const bool has1 = N9 || g == 0, has2 = N9 && g == 0;
  const int last = P->nl - 1;
  f32x4 a[MW_STACK_UB][TILES];
  double base[TILES];
#pragma unroll
  for (int u = 0; u < TILES; u++) {
    a[0][u] = (f32x4){net_scaled(x0[u], S.imin0, S.irng0), has1 ? net_scaled(x1[u], S.imin1, S.irng1) : 0.f, has2 ? net_scaled(x2[u], S.imin2, S.irng2) : 0.f, 0.f};
    base[u] = 0.0;
    if (tend) { const double b = net5_rotate_base(g, x0[u], x1[u]); base[u] = g == 0 ? x0[u] : b; }      // (wave-uniform)
  }
  for (int l = 0; l < last; l++) {                                        // the hidden layers
    f32x4 d[MW_STACK_UB][TILES];
    const int nob = P->nob[l];
    const float slope = P->slope[l];
    stack_dense<TILES, MW_STACK_UB>(d, a, img + P->aoff[l], img + P->boff[l], P->nk[l], nob, lane, g);
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
  f32x4 o[1][TILES];                                                      // Dense(4): output g in register 0 of group g
  stack_dense<TILES, 1>(o, a, img + P->aoff[last], img + P->boff[last], P->nk[last], 1, lane, g);
#pragma unroll
  for (int u = 0; u < TILES; u++) {
    double v = (double)o[0][u][0] * S.orng + S.omin;
    if (tend) v = base[u] + v;
    if (g != 0) v = fmax(0.0, v);
    y[u] = v;
  }
}

// the scaling constants of lane group g of one stack (the divisions are k_mlp_stack's)
template <bool N9>
__device__ __forceinline__ StackLane stack_lane(const StackP *P, int g) {
  const int f1 = (N9 || g == 0) ? 4 + g : 4;
  StackLane S;
  S.imin0 = P->in_min[g]; S.irng0 = 1.0 / P->in_rng[g]; S.imin1 = P->in_min[f1]; S.irng1 = 1.0 / P->in_rng[f1];
  S.imin2 = N9 ? P->in_min[8] : 0.0; S.irng2 = N9 ? 1.0 / P->in_rng[8] : 1.0;
  S.omin = P->out_min[g]; S.orng = P->out_rng[g];
  return S;
}

// one list of the group: rows [r0, r0 + n) of the table
struct StackList {
  int r0, n, mpb;
  size_t lds;                                                             // bytes of dynamic LDS: the largest workgroup's images + pads
  bool anyt;
};

// the largest mpb of 4, 2, 1 (at most apply_slot's rule for n stacks) for which every workgroup's images + pads fit `budget` bytes
inline void stack_list_plan(StackList &L, const std::vector<StackRow> &rows, size_t budget = MW_STACK_GROUP_LDS) {
  L.mpb = 1; L.lds = 0;
  if (L.n < 1) return;
  for (int mpb = L.n >= 3 ? 4 : L.n; mpb >= 1; mpb /= 2) {
    size_t worst = 0;
    for (int m0 = 0; m0 < L.n; m0 += mpb) {
      size_t bytes = 0;
      for (int j = m0; j < std::min(L.n, m0 + mpb); j++) bytes += sizeof(float) * (size_t)(rows[(size_t)(L.r0 + j)].P.nimg + MW_STACK_PAD);
      worst = std::max(worst, bytes);
    }
    L.mpb = mpb; L.lds = worst;
    if (worst <= budget) return;
  }
}

} // namespace mw

struct mw_mlp_stack_s {
  mw::StackP P;
  int form;
  float *img, *params;                                                    // DEVICE: the MFMA image, the parameters as they came
};

struct mw_stack_group_s {
  int n;
  mw::StackRow *rows;                   // DEVICE (n): the n_in = 5 list, then the n_in = 9 list
  float *imgs, *params;                 // DEVICE: the images, each with its pad behind it, and the parameters as they came, in row order
  mw::StackList list[2];                // n_in = 5, n_in = 9
  mw::StackList elist[2];               // the same lists as mw_stack_group_eval plans them (its tail takes MW_STACK_EVAL_RED bytes of the LDS)
  int row_of[MW_STACK_GROUP_MAX];       // HOST: the row of stack j (the order given at creation)
  int form_of[MW_STACK_GROUP_MAX], nimg_of[MW_STACK_GROUP_MAX];      // HOST, by row: its form and the floats of its image (what a committee's chunks are planned from)
  bool any_tendency;
};

// ---- what the units that run a COMMITTEE of a group's stacks share (mw_stack_committee.hip: mean and range; mw_stack_guard.hip: the
// guarded committee's last launch) ----
namespace mw {

constexpr int SC_MAX = MW_COMMITTEE_MAX_MODELS;
constexpr int SC_TILES = 4;                                         // tiles (n_in = 9: levels) per wave and pass
constexpr long long SC_MAX_BLOCKS = 256 * 4;                        // grid.x: grid-stride beyond 4 blocks per CU (every block fills its LDS once)

struct StackChunk { int n, first, last; int row[SC_MAX], lds_off[SC_MAX]; };   // rows of the group's table, floats from the LDS base
struct StackSel { int n; int row[SC_MAX]; };
struct StackCommitteeFields { const double *in[5]; double *out[4]; double *range[4]; };      // range[*]: all null or all set

// what a lane carries of its (cell, field) across the stacks of a chunk, and across chunks through the workspace: plane (3 g + q) of
// `cells` doubles, q = sum, hi, lo
struct CommitteeAcc { double sum, hi, lo; };

__device__ __forceinline__ void acc_add(CommitteeAcc &a, double y, bool init) {
#pragma clang fp contract(off)
  a.sum = init ? y : a.sum + y;                                     // (the first addend as it is: a committee of one keeps its bits)
  a.hi  = init ? y : eval_max(a.hi, y);
  a.lo  = init ? y : eval_min(a.lo, y);
}

// k_mlp_stack_strict's expressions for one cell of one stack: in[9] raw (n_in = 5: the first five), p[4] the four outputs
__device__ __forceinline__ void stack_strict_cell(const StackRow *R, const float *par, const double (&in)[9], double (&p)[4]) {
#pragma clang fp contract(off)
  const StackP &P = R->P;
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
  if (R->form != MW_FORM_STATE) {
    p[0] =           in[0] + (x[0] * P.out_rng[0] + P.out_min[0]);
    p[1] = fmax(0.0, in[2] + (x[1] * P.out_rng[1] + P.out_min[1]));
    p[2] = fmax(0.0, in[3] + (x[2] * P.out_rng[2] + P.out_min[2]));
    p[3] = fmax(0.0, in[4] + (x[3] * P.out_rng[3] + P.out_min[3]));
  } else {
    p[0] =           x[0] * P.out_rng[0] + P.out_min[0];
    p[1] = fmax(0.0, x[1] * P.out_rng[1] + P.out_min[1]);
    p[2] = fmax(0.0, x[2] * P.out_rng[2] + P.out_min[2]);
    p[3] = fmax(0.0, x[3] * P.out_rng[3] + P.out_min[3]);
  }
}

// The checked selection: the rows of sel in the group's table and the greedy chunks of the fast form, from the group's host mirror of
// its rows (n_in by list, form_of, nimg_of).  Returns an error text, or empty.
struct StackCommitteePlan { StackSel sel; int n_in; bool anyt; int nchunks; StackChunk chunk[SC_MAX]; size_t lds[SC_MAX]; };

static std::string stack_committee_plan(StackCommitteePlan &Q, const mw_stack_group_s *g, int n_sel, const int *sel, const std::string &w) {
  if (!g) return w + ": null handle";
  if (!sel) return w + ": null pointer";
  if (n_sel < 1 || n_sel > SC_MAX) return w + ": a committee has 1 to " + std::to_string(SC_MAX) + " stacks, got " + std::to_string(n_sel);
  memset(&Q, 0, sizeof(Q));
  Q.sel.n = n_sel;
  size_t used = 0;
  for (int j = 0; j < n_sel; j++) {
    if (sel[j] < 0 || sel[j] >= g->n) return w + ": stack " + std::to_string(sel[j]) + " is outside the group's [0, " + std::to_string(g->n) + ")";
    for (int i = 0; i < j; i++) if (sel[i] == sel[j]) return w + ": stack " + std::to_string(sel[j]) + " is given twice";
    const int r = g->row_of[sel[j]], n_in = r >= g->list[1].r0 ? 9 : 5;    // (the n_in = 5 list comes first in the table)
    if (j > 0 && n_in != Q.n_in) return w + ": stacks " + std::to_string(sel[0]) + " and " + std::to_string(sel[j]) + " differ in n_in: a committee has one";
    Q.n_in = n_in;
    Q.sel.row[j] = r;
    Q.anyt = Q.anyt || g->form_of[r] != MW_FORM_STATE;
    const size_t bytes = sizeof(float) * (size_t)(g->nimg_of[r] + MW_STACK_PAD);
    if (bytes > MW_STACK_GROUP_LDS) return w + ": a stack's image exceeds the kernel's LDS";      // (no shape mw_mlp_stack_create accepts does)
    if (Q.nchunks == 0 || used + bytes > MW_STACK_GROUP_LDS) { Q.nchunks++; used = 0; }      // greedy, in listed order
    StackChunk &C = Q.chunk[Q.nchunks - 1];
    C.row[C.n] = r; C.lds_off[C.n] = (int)(used / sizeof(float)); C.n++;
    used += bytes;
    Q.lds[Q.nchunks - 1] = used;
  }
  Q.chunk[0].first = 1; Q.chunk[Q.nchunks - 1].last = 1;
  return std::string();
}

// chunk c of the plan in the fast form (mw_stack_committee.hip, where k_stack_committee is emitted); 0, or 1 with the error text set
int stack_committee_launch(const mw_stack_group_s *g, const StackCommitteePlan &Q, int c, int member, int nz, long long ncol, int nens,
                           const StackCommitteeFields &F, double *workspace, hipStream_t st);

static bool sc_overlap(const double *a, long long na, const double *b, long long nb) { return a < b + nb && b < a + na; }

} // namespace mw
