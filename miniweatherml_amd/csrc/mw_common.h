// Shared by every unit of libmw_cdna4.so: error reporting (no CPU fallbacks live here), and the device-visible types, constants and
// pressure / pow helpers of the dycore that kernels in several of its units need (mw_dycore.hip, mw_march.h, mw_calib.h, mw_dycore_init.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mw_cdna4.h"
#include "mw_glibc_pow.h"
#include <string>
#include <cstdio>

namespace mw {

void set_error(const std::string &msg);           // defined in mw_host.cpp

#define MW_HIP(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e__ = (call);                                                                           \
    if (e__ != hipSuccess) {                                                                           \
      char b__[512];                                                                                   \
      snprintf(b__, sizeof(b__), "%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
      mw::set_error(b__);                                                                              \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

#define MW_FAIL(msg)                                                                                   \
  do { mw::set_error(std::string(__FILE__) + ":" + std::to_string(__LINE__) + ": " + (msg)); return 1; } while (0)

#define MW_LAUNCH_CHECK() MW_HIP(hipGetLastError())

} // namespace mw

// ---- dycore: what its kernels share ---------------------------------------------------------------------------------------
namespace mw {

enum { idR = 0, idU = 1, idV = 2, idW = 3, idT = 4 };
static constexpr int HXc = 3;     // x/y halo: 2 for the stencil + 1 so that the neighbour's edge value is rebuilt locally
static constexpr int HZc = 2;     // z halo: z faces at the domain boundary use the edge-value BC rule, not ghost cells

// A row / level / variable stride in elements.  It fits 32 bits on any handle that fits the GPU (one variable of a slab with 2^31 doubles is 16 GB,
// and a handle keeps 4 slabs of >= 6 variables; strides_fit() refuses anything else at create), and every use is a
// product with a 32-bit index: held as an int that converts to long long, `(long long)idx * stride` is a 32 x 32 -> 64 multiply (s_mul_i32 +
// s_mul_hi_i32) instead of the 64 x 64 one (7 scalar instructions) -- the marching kernels derive a dozen such offsets from the level index in
// every iteration (no SGPRs to keep them), and at two waves per SIMD a wave's scalar instructions delay its own vector ones.  No int arithmetic can
// overflow through it: the only way out is the conversion.
struct Stride32 {
  int v;
  __host__ __device__ __forceinline__ operator long long() const { return (long long)v; }
  __host__ __device__ __forceinline__ Stride32 &operator=(long long x) { v = (int)x; return *this; }
};

struct DyP {                      // kernel parameter block (by value)
  int nz, ny, nx, nens, nt, V;
  int HX, HY, HZ;
  int NXE;                        // (nx+2HX)*nens
  Stride32 sJ, sK, sV;            // row / level / variable strides of the prognostic slabs
  Stride32 nC;                    // nz*ny*nx*nens
  Stride32 fxJ, fxK, fxV, fyJ, fyK, fyV, fzJ, fzK, fzV;   // flux strides
  int sim2d, bc_x, bc_y, bc_z, px, py, nproc_x, nproc_y;
  int v0;                         // halo/pack kernels: index of the first variable of the group being processed
  int cst, ce;                    // coupler-side stride / member offset (1, 0; member-major mode: nens, member) -- see cpl() below
  int wrap_x, wrap_y;             // production path, periodic direction owned by one rank: the marching kernels wrap their x / row index
                                  // instead of reading halo cells, and that halo is not filled
  int enable_gravity, use_immersed, idWV;
  int zero_skip;                  // marching kernels: skip the reconstructions of a tracer that is exactly zero over a wavefront's stencil (mw_march.h)
  // zero-row map of the current RK stage (mw_zero_rows.h), nullptr = none: one word per (level, row), bit v = "tracer v may be
  // non-zero in what iterations k-3 .. k of the row's marching wave touch"; word of (k, j) at [k * zq_ld + j + HY]
  const unsigned *zq;
  const unsigned *zqk;            // ... the converting y launch: the rows of the slab it writes that hold zeros already
  const unsigned *zqp, *zqc;      // ... "the row an iteration stores to holds zeros already": the previous sub-cycle's map of this stage / the coupler's rows (mw_zero_rows.h)
  int zq_ld;
  int zq_xper;                    // this rank owns the periodic x direction (bc_x periodic, x not decomposed): the maps' x segments grow and are looked up round
                                  // the seam.  NOT wrap_x: with option wrap = 0 the kernels read halo cells instead of wrapping their index, and the halo fill
                                  // puts the far edge's cells there -- a tracer crosses the seam either way
  // parked column increments (mw_nudge_to_column_deferred): inc[(l * nz + k) * nens + e] for l = density_dry, uvel, vvel, temp, water_vapor, added to
  // the coupler's values while the converting y launch loads them; nullptr = none
  const double *pinc;
  unsigned pos_mask, mass_mask;
  double dx, dy, dz, rdx, rdy, rdz, C0, gamma, grav, fcor, R_d, R_v;
  const double *hyc, *hytc, *hye, *hyte;       // device (nz,nens) / (nz+1,nens)
  const double *p0c, *p0e, *ihytc, *ihyte;     // C0*hyt^gamma and 1/hyt at cells / edges (fast pressure path)
  const double *imm;                           // device (nz,ny,nx,nens)
  const double *hypk;                          // the eight profile values of level k packed as rows of 8: (hyc, hytc, p0c, ihytc, hye, hyte,
                                               // p0e, ihyte)[(k*nens+e)*8 + f], nz+1 rows: one pointer instead of eight in the hot kernels
  double bn[11];                               // binomial series coefficients C(gamma, n), n = 0..10
  int bn_default;                              // bn[] equals the literal table for gamma = 1003/716 bit for bit (the usual case)
  int an_default;                              // likewise C(1/gamma, n) of the conversion's inverse series (mw_march.h)
};

struct CouplerPtrs {
  double *rho_d, *u, *v, *w, *temp;
  double *tr[MW_MAX_TRACERS];
};

// Index into a COUPLER-layout array (nz,ny,nx,nens) from an index `ci` of the handle's internal cell numbering.  Normally the two
// coincide (cst = 1, ce = 0).  Member-major mode (nens > 1, production path): the handle's arrays hold one member after the other and
// every kernel runs its nens = 1 form on member ce; the coupler's arrays keep their member-fastest layout: cst = nens doubles apart.
__device__ __forceinline__ long long cpl(const DyP &p, long long ci) { return ci * p.cst + p.ce; }
// Periodic direction owned by one rank (DyP::wrap_x / wrap_y): the interior index that a halo index stands for.
__device__ __forceinline__ int wrap_xq(const DyP &p, int q, int NXI) { return p.wrap_x ? (q < 0 ? q + NXI : (q >= NXI ? q - NXI : q)) : q; }
__device__ __forceinline__ int wrap_row(const DyP &p, int j) { return p.wrap_y ? (j < 0 ? j + p.ny : (j >= p.ny ? j - p.ny : j)) : j; }

// Compile-time configuration of the marching kernels (mw_march.h).  The run-time switches of DyP that are wave-uniform and fixed
// for a whole run cost SGPRs (the marching kernels have none to spare: every SGPR spilled to a VGPR lane comes back as a
// v_readlane, a VALU instruction) and selects (v_cndmask pairs per double).  K = 0 keeps every switch at run time (any
// configuration).  K = 1 / 2 are the shipped experiments' configurations with the switches folded:
//   both: nens == 1 (or one member of a member-major handle), 3-D, periodic x and y (any rank count: the index wrap stays a
//         run-time switch), wall in z, no Coriolis term (latitude is forced to 0 at init, :1249), the default gamma (series
//         coefficients as literals), every tracer positive and mass-adding with water vapour first (idWV == 0);
//   K = 1 (supercell_example, supercell_kessler_surrogate, community_benchmark): gravity on, no immersed boundaries, the three
//         Kessler tracers;
//   K = 2 (simple_city): immersed boundaries, gravity off, water vapour only.
// marching_config() (mw_dycore.hip) decides; anything else runs K = 0.
template <int K> struct Cf {
  static constexpr bool spec = (K != 0);
  static __device__ __forceinline__ bool x_periodic(const DyP &p) { return spec || p.bc_x == MW_BC_PERIODIC; }
  static __device__ __forceinline__ bool y_periodic(const DyP &p) { return spec || p.bc_y == MW_BC_PERIODIC; }
  static __device__ __forceinline__ bool z_wall(const DyP &p) { return spec || p.bc_z == MW_BC_WALL; }
  static __device__ __forceinline__ bool sim2d(const DyP &p) { return !spec && p.sim2d; }
  static __device__ __forceinline__ bool immersed(const DyP &p) { return K == 2 || (!spec && p.use_immersed); }
  static __device__ __forceinline__ bool gravity(const DyP &p) { return K == 1 || (!spec && p.enable_gravity); }
  static __device__ __forceinline__ bool coriolis(const DyP &p) { return !spec; }
  static __device__ __forceinline__ bool bn_default(const DyP &p) { return spec || p.bn_default; }
  static __device__ __forceinline__ bool an_default(const DyP &p) { return spec || p.an_default; }
  static __device__ __forceinline__ bool positive(const DyP &p, int t) { return spec || ((p.pos_mask >> t) & 1u); }
  static __device__ __forceinline__ bool adds_mass(const DyP &p, int t) { return spec || ((p.mass_mask >> t) & 1u); }
  static __device__ __forceinline__ bool is_wv(const DyP &p, int t) { return spec ? (t == 0) : (t == p.idWV); }
  static __device__ __forceinline__ int ntr(const DyP &p) { return K == 1 ? 3 : K == 2 ? 1 : p.nt; }   // K = 1: the three Kessler tracers; K = 2: water vapour
};

// -----------------------------------------------------------------------------------------------------
// pow(x, gamma): strict = device libm pow; fast = same for now (kept separate so it can be specialised)
// -----------------------------------------------------------------------------------------------------
// pow of the kernels that keep the reference's operation order (general path: strict and fast arithmetic; init; D1 / D13 passes):
// the bits of the host's glibc (mw_glibc_pow.h), so that the strict path equals the CPU oracle bit for bit.  Arguments outside the
// restated main path -- nothing the dycore produces -- take the device library's pow.
__device__ __forceinline__ double pow_ref(double x, double y) {
  double r;
  if (__builtin_expect(glibc_pow_main(x, y, &r), 1)) return r;
  return pow(x, y);
}
__device__ __forceinline__ double exp_ref(double x) {       // likewise exp (the thermal initial state's saturation vapour pressure, :1139)
  double r;
  if (__builtin_expect(glibc_exp_main(x, &r), 1)) return r;
  return exp(x);
}
__device__ __forceinline__ double cos_ref(double x) {       // likewise cos (the cosine bells of the initial states, :1131, perturb_temperature.h:63)
  double r;
  if (__builtin_expect(glibc_cos_main(x, &r), 1)) return r;
  return cos(x);
}
template <bool STRICT> __device__ __forceinline__ double pow_gamma(double x, double g) { return pow_ref(x, g); }

// p = C0 (hyt + e)^gamma for the fast path.  The Riemann solver needs two of these per face (6 per cell and stage,
// :401,:426,:457); the device-libm pow costs ~230 fp64-VALU instructions.  Writing (hyt + e)^gamma =
// hyt^gamma (1 + delta)^gamma with delta = e/hyt (|delta| is a few per cent: e is the reconstructed PERTURBATION of
// rho*theta) turns it into p0(k) * sum_n C(gamma,n) delta^n: 10 FMAs; truncation |C(gamma,11)| 0.05^11 ~ 1e-17 for
// |delta| <= 0.05.  Larger perturbations take the generic pow (per-lane branch).
// out of line on purpose: the libm pow body (~230 instructions, ~60 VGPRs) would otherwise be inlined twice per Riemann solve
// into kernels that sit at the register limit; it only runs for |(rho theta)'| > 5 % of the hydrostatic value.
__device__ __attribute__((noinline)) double pressure_pow(double C0, double x, double gamma) { return C0 * pow(x, gamma); }

// C(gamma, n), n = 1..10, for the default gamma = cp_d/(cp_d - R_d) = 1003/716 (the long-double recurrence of fill_params, as
// hex literals).  Literal operands are materialised by scalar moves where they are used; the same numbers read from the
// parameter block stay resident in 22 SGPRs for the whole kernel -- and the marching kernels already spill SGPRs to VGPR lanes.
__device__ __forceinline__ double pressure_series_default(double dl) {
#pragma clang fp contract(fast)
  double acc = 0x1.d587239f51368p-10;
  acc = acc * dl + -0x1.34ef19ee96d45p-9;
  acc = acc * dl + 0x1.a553bdf108378p-9;
  acc = acc * dl + -0x1.2cfe340a81e1p-8;
  acc = acc * dl + 0x1.ca1dc2cec496fp-8;
  acc = acc * dl + -0x1.7dda38e0cc64cp-7;
  acc = acc * dl + 0x1.6f48bfb7e5329p-6;
  acc = acc * dl + -0x1.cb58863e4dd29p-5;
  acc = acc * dl + 0x1.1f7e1e502b562p-2;
  acc = acc * dl + 0x1.669d5185016e2p+0;
  return acc;
}
static const double BN_DEFAULT[11] = {1.0, 0x1.669d5185016e2p+0, 0x1.1f7e1e502b562p-2, -0x1.cb58863e4dd29p-5, 0x1.6f48bfb7e5329p-6,
                                      -0x1.7dda38e0cc64cp-7, 0x1.ca1dc2cec496fp-8, -0x1.2cfe340a81e1p-8, 0x1.a553bdf108378p-9,
                                      -0x1.34ef19ee96d45p-9, 0x1.d587239f51368p-10};

template <int K = 0>
__device__ __forceinline__ double pressure_fast(const DyP &p, double e, double hyt, double p0, double ihyt) {
#pragma clang fp contract(fast)
  double dl = e * ihyt;
  if (fabs(dl) <= 0.05 && Cf<K>::bn_default(p)) return p0 + p0 * (pressure_series_default(dl) * dl);
  return pressure_pow(p.C0, hyt + e, p.gamma);                  // large perturbation, or a non-default gamma
}
// The two sides of a face at once (the Riemann solver needs both, :401): the same two Horner chains as pressure_series_default,
// as three-address v_fma_f64 interleaved in ONE asm statement.  Left to the compiler, the chain of a polynomial whose coefficients
// it keeps in registers becomes v_mov_b64 (coefficient -> accumulator) + v_fmac_f64 (two-address) per step -- nine extra VALU
// instructions per evaluation, four evaluations per level in k_xz_state (seen in round 2's gfx950 code, tools/isa_histogram.py) --
// inside one divergent block per side.  Here: two independent dependency chains in one block, no moves.  (The coefficients are
// "v" operands: twenty VGPRs for the whole kernel.  The single evaluations of D1 / D13 keep the compiler's form: k_tracers_fused
// <3, 1> has no registers for them.)
__device__ __forceinline__ void pressure_series_pair(double dlL, double dlR, double &sL, double &sR) {
  double aL, aR;
  asm("v_fma_f64 %0, %4, %2, %5\n\tv_fma_f64 %1, %4, %3, %5\n\t"
      "v_fma_f64 %0, %0, %2, %6\n\tv_fma_f64 %1, %1, %3, %6\n\t"
      "v_fma_f64 %0, %0, %2, %7\n\tv_fma_f64 %1, %1, %3, %7\n\t"
      "v_fma_f64 %0, %0, %2, %8\n\tv_fma_f64 %1, %1, %3, %8\n\t"
      "v_fma_f64 %0, %0, %2, %9\n\tv_fma_f64 %1, %1, %3, %9\n\t"
      "v_fma_f64 %0, %0, %2, %10\n\tv_fma_f64 %1, %1, %3, %10\n\t"
      "v_fma_f64 %0, %0, %2, %11\n\tv_fma_f64 %1, %1, %3, %11\n\t"
      "v_fma_f64 %0, %0, %2, %12\n\tv_fma_f64 %1, %1, %3, %12\n\t"
      "v_fma_f64 %0, %0, %2, %13\n\tv_fma_f64 %1, %1, %3, %13"
      : "=&v"(aL), "=&v"(aR)
      : "v"(dlL), "v"(dlR), "v"(0x1.d587239f51368p-10), "v"(-0x1.34ef19ee96d45p-9), "v"(0x1.a553bdf108378p-9), "v"(-0x1.2cfe340a81e1p-8),
        "v"(0x1.ca1dc2cec496fp-8), "v"(-0x1.7dda38e0cc64cp-7), "v"(0x1.6f48bfb7e5329p-6), "v"(-0x1.cb58863e4dd29p-5),
        "v"(0x1.1f7e1e502b562p-2), "v"(0x1.669d5185016e2p+0));
  sL = aL; sR = aR;
}
template <int K = 0>
__device__ __forceinline__ void pressure_fast_pair(const DyP &p, double eL, double eR, double hyt, double p0, double ihyt, double &pL, double &pR) {
#pragma clang fp contract(fast)
  const double dL = eL * ihyt, dR = eR * ihyt;
  if (__builtin_expect(fabs(dL) <= 0.05 && fabs(dR) <= 0.05 && Cf<K>::bn_default(p), 1)) {
    double sL, sR;
    pressure_series_pair(dL, dR, sL, sR);
    pL = p0 + p0 * (sL * dL);
    pR = p0 + p0 * (sR * dR);
  } else {                                                      // a large perturbation on either side, or a non-default gamma
    pL = pressure_fast<K>(p, eL, hyt, p0, ihyt);
    pR = pressure_fast<K>(p, eR, hyt, p0, ihyt);
  }
}

// the member-to-member strides of a member-major handle, for the kernels that hold the members of a tile in one workgroup (mw_march.h)
struct MemberOff {
  long long slab, tend, mx, my, mz, fx, fy, fz, cells, per;    // doubles (selectors / flags: bytes) from member e to member e + 1
  long long zq;                                                // ... and words, for the members' zero-row maps
  int n, sh;                                                   // members per workgroup (2 or 4) and log2 of it
};

} // namespace mw
