// =====================================================================================================
// mw_dycore.hip -- MI355X (gfx950) implementation of Dynamics_Euler_Stratified_WenoFV::time_step
// (reference: model/modules/dynamics_euler_stratified_wenofv.h:81-552,1891-2015) behind include/mw_cdna4.h.
// This unit: the general-path kernels and their launchers, the handle and its options, the C ABI and time_step's decisions; the marching
// kernels' launchers and schedules, the initial states and the test aids are units of their own (map: mw_dycore_int.h).
//
// Data layout in HBM:
//   * two prognostic slabs S0 (q^n) and S1 (q*), each (V, nz+2*HZ, ny+2*HY, (nx+2*HX)*nens) fp64, x(+ens) fastest,
//     V = 5 + T, HX = HY = 3 (HY = 0 in 2-D), HZ = 2.  They hold the *reconstruction variables*
//     (rho', u, v, w, (rho theta)', q_t) -- i.e. the reference's `state`/`tracers` AFTER its in-place divide by
//     density (:248-255); the conserved value is recovered as u*rho exactly like the reference's re-multiply
//     (:477-484), so no information or rounding step is lost or added.
//   * six face-flux arrays in the reference's public layout (:1671-1676), state and tracer parts contiguous.
//   * no `limits` arrays (6*V*N doubles in the reference, :260-265): edge values live in registers only.
//
// Per RK stage:   halo fill (3-cell, replaces halo_exchange+edge_exchange)  ->  k_flux (D6+D9 fused)
//                 ->  k_fct (D10)  ->  k_update (D11 + D12 + the next stage's D2, or D13 on the last stage)
// =====================================================================================================
#include "mw_dycore_int.h"
#include "mw_weno.h"
#include <map>
#include <set>
#include <tuple>
#include <mutex>
#include <cmath>
#include <cstring>

namespace mw {
static std::mutex g_launch_mu;
static std::set<const void *> g_launched;
void note_launch(const void *fn) { std::lock_guard<std::mutex> lk(g_launch_mu); g_launched.insert(fn); }

// -----------------------------------------------------------------------------------------------------
// D1  convert_coupler_to_dynamics (:1955-2015) fused with the stage-1 divide D2 (:248-255)
// -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_coupler_to_state(DyP p, CouplerPtrs c, double *__restrict__ S) {
#pragma clang fp contract(off)
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y;
  int NXI = p.nx * p.nens;
  if (t >= (long long)p.ny * NXI) return;
  int j = (int)(t / NXI), ie = (int)(t - (long long)j * NXI);
  int e = ie % p.nens;
  long long ci = ((long long)k * p.ny + j) * NXI + ie;
  double rho_d = c.rho_d[ci], u = c.u[ci], v = c.v[ci], w = c.w[ci], temp = c.temp[ci];
  double rho_v = c.tr[p.idWV][ci];
  double press = rho_d * p.R_d * temp + rho_v * p.R_v * temp;
  double rho = rho_d;
  for (int tr = 0; tr < p.nt; tr++) if ((p.mass_mask >> tr) & 1u) rho += c.tr[tr][ci];
  double theta = pow_ref(press / p.C0, 1.0 / p.gamma) / rho;
  double hyc = p.hyc[k * p.nens + e], hytc = p.hytc[k * p.nens + e];
  double *s = S + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens + ie;
  double rp = rho - hyc;                                  // state(idR)
  double den = rp + hyc;                                  // what D2 divides by (:249)
  s[idR * p.sV] = rp;
  s[idU * p.sV] = (rho * u) / den;
  s[idV * p.sV] = (rho * v) / den;
  s[idW * p.sV] = (rho * w) / den;
  s[idT * p.sV] = rho * theta - hytc;
  for (int tr = 0; tr < p.nt; tr++) s[(5 + tr) * p.sV] = c.tr[tr][ci] / den;
}

// -----------------------------------------------------------------------------------------------------
// Halo fill, single rank in a direction == periodic wrap onto itself (coupler.h:169-179 self neighbour),
// plus the boundary conditions of halo_exchange (:752-825).  One thread per halo cell and variable.
// Regions: 0 = x halos (k,j interior), 1 = y halos (k,i interior), 2 = z halos (j,i interior); corners are
// never read.  `do_x`/`do_y` = 0 when that direction's halos come from a neighbour.
// -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void halo_x_body(const DyP &p, double *__restrict__ S, long long t) {
  // threads: (v, k, j, h in [0,2HX), e)
  int H2 = 2 * p.HX;
  long long n = (long long)p.V * p.nz * p.ny * H2 * p.nens;
  if (t >= n) return;
  int e = (int)(t % p.nens); t /= p.nens;
  int h = (int)(t % H2); t /= H2;
  int j = (int)(t % p.ny); t /= p.ny;
  int k = (int)(t % p.nz); int v = (int)(t / p.nz);
  double *row = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + e;
  int lo = h < p.HX;
  int ih = lo ? h : p.nx + h;                       // halo cell index in [0,HX) or [nx+HX, nx+2HX)
  double val;
  if (p.bc_x == MW_BC_PERIODIC) {
    int src = lo ? ih + p.nx : ih - p.nx;
    val = row[(long long)src * p.nens];
  } else {                                          // :782-803 (both sides, two independent ifs: `px == 0`, `px == nproc_x-1`)
    if (lo ? (p.px != 0) : (p.px != p.nproc_x - 1)) return;   // not a domain edge: this halo holds the neighbour's strip
    if (v + p.v0 == idU && p.bc_x == MW_BC_WALL) val = 0;
    else val = row[(long long)(lo ? p.HX : p.HX + p.nx - 1) * p.nens];
  }
  row[(long long)ih * p.nens] = val;
}
__device__ __forceinline__ void halo_y_body(const DyP &p, double *__restrict__ S, long long t) {
  // threads: (v, k, h in [0,2HY), ie interior)
  int H2 = 2 * p.HY, NXI = p.nx * p.nens;
  long long n = (long long)p.V * p.nz * H2 * NXI;
  if (t >= n) return;
  int ie = (int)(t % NXI); t /= NXI;
  int h = (int)(t % H2); t /= H2;
  int k = (int)(t % p.nz); int v = (int)(t / p.nz);
  double *col = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)p.HX * p.nens + ie;
  int lo = h < p.HY;
  int jh = lo ? h : p.ny + h;
  double val;
  if (p.bc_y == MW_BC_PERIODIC) {
    int src = lo ? jh + p.ny : jh - p.ny;
    val = col[(long long)src * p.sJ];
  } else {                                          // :804-825
    if (lo ? (p.py != 0) : (p.py != p.nproc_y - 1)) return;
    if (v + p.v0 == idV && p.bc_y == MW_BC_WALL) val = 0;
    else val = col[(long long)(lo ? p.HY : p.HY + p.ny - 1) * p.sJ];
  }
  col[(long long)jh * p.sJ] = val;
}
__device__ __forceinline__ void halo_z_body(const DyP &p, double *__restrict__ S, long long t) {
  // threads: (v, h in [0,2HZ), j, ie interior)   :752-781
  int H2 = 2 * p.HZ, NXI = p.nx * p.nens;
  long long n = (long long)p.V * H2 * p.ny * NXI;
  if (t >= n) return;
  int ie = (int)(t % NXI); t /= NXI;
  int j = (int)(t % p.ny); t /= p.ny;
  int h = (int)(t % H2); int v = (int)(t / H2);
  double *col = S + (long long)v * p.sV + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens + ie;
  int lo = h < p.HZ;
  int kh = lo ? h : p.nz + h;
  double val;
  if (p.bc_z == MW_BC_PERIODIC) val = col[(long long)(lo ? kh + p.nz : kh - p.nz) * p.sK];     // :752-763
  else if (v + p.v0 == idW && p.bc_z == MW_BC_WALL) val = 0;
  else val = col[(long long)(lo ? p.HZ : p.HZ + p.nz - 1) * p.sK];
  col[(long long)kh * p.sK] = val;
}

// All three regions in one launch (they are independent: each writes its own halo cells from interior cells, and the corners
// are never read): blocks [0, nbx) do x, [nbx, nbx+nby) do y, the rest z.  Used when no direction needs a neighbour exchange.
__global__ __launch_bounds__(256) void k_halo_xyz(DyP p, double *__restrict__ S, unsigned nbx, unsigned nby) {
  const unsigned b = blockIdx.x;
  if (b < nbx) halo_x_body(p, S, (long long)b * 256 + threadIdx.x);
  else if (b < nbx + nby) halo_y_body(p, S, (long long)(b - nbx) * 256 + threadIdx.x);
  else halo_z_body(p, S, (long long)(b - nbx - nby) * 256 + threadIdx.x);
}

// Pack / unpack for a neighbour exchange (3-cell halos of all V variables; interior rows only, like :606-631,:725-747)
// W/E buffers (V,nz,ny,HX,nens), S/N buffers (V,nz,HY,nx,nens).
__device__ __forceinline__ void pack_x_body(const DyP &p, const double *__restrict__ S, double *__restrict__ bW, double *__restrict__ bE, long long t) {
  long long n = (long long)p.V * p.nz * p.ny * p.HX * p.nens;
  if (t >= n) return;
  long long r = t;
  int e = (int)(r % p.nens); r /= p.nens;
  int h = (int)(r % p.HX); r /= p.HX;
  int j = (int)(r % p.ny); r /= p.ny;
  int k = (int)(r % p.nz); int v = (int)(r / p.nz);
  const double *row = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + e;
  bW[t] = row[(long long)(p.HX + h) * p.nens];              // my first HX interior cells -> west neighbour's east halo
  bE[t] = row[(long long)(p.nx + h) * p.nens];              // my last  HX interior cells -> east neighbour's west halo
}
__device__ __forceinline__ void unpack_x_body(const DyP &p, double *__restrict__ S, const double *__restrict__ bW, const double *__restrict__ bE, long long t) {
  long long n = (long long)p.V * p.nz * p.ny * p.HX * p.nens;
  if (t >= n) return;
  long long r = t;
  int e = (int)(r % p.nens); r /= p.nens;
  int h = (int)(r % p.HX); r /= p.HX;
  int j = (int)(r % p.ny); r /= p.ny;
  int k = (int)(r % p.nz); int v = (int)(r / p.nz);
  double *row = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + e;
  row[(long long)h * p.nens]                 = bW[t];       // received from west
  row[(long long)(p.nx + p.HX + h) * p.nens] = bE[t];       // received from east
}
__device__ __forceinline__ void pack_y_body(const DyP &p, const double *__restrict__ S, double *__restrict__ bS, double *__restrict__ bN, long long t) {
  int NXI = p.nx * p.nens;
  long long n = (long long)p.V * p.nz * p.HY * NXI;
  if (t >= n) return;
  long long r = t;
  int ie = (int)(r % NXI); r /= NXI;
  int h = (int)(r % p.HY); r /= p.HY;
  int k = (int)(r % p.nz); int v = (int)(r / p.nz);
  const double *col = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)p.HX * p.nens + ie;
  bS[t] = col[(long long)(p.HY + h) * p.sJ];
  bN[t] = col[(long long)(p.ny + h) * p.sJ];
}
__device__ __forceinline__ void unpack_y_body(const DyP &p, double *__restrict__ S, const double *__restrict__ bS, const double *__restrict__ bN, long long t) {
  int NXI = p.nx * p.nens;
  long long n = (long long)p.V * p.nz * p.HY * NXI;
  if (t >= n) return;
  long long r = t;
  int ie = (int)(r % NXI); r /= NXI;
  int h = (int)(r % p.HY); r /= p.HY;
  int k = (int)(r % p.nz); int v = (int)(r / p.nz);
  double *col = S + (long long)v * p.sV + (long long)(k + p.HZ) * p.sK + (long long)p.HX * p.nens + ie;
  col[(long long)h * p.sJ]                 = bS[t];
  col[(long long)(p.ny + p.HY + h) * p.sJ] = bN[t];
}

// Both directions in ONE launch (round 5; blocks [0, nbx) pack / unpack the W / E strips, the rest the S / N strips -- nbx or the rest
// may be 0): an exchange is a chain pack -> transfer -> unpack on a stream that shares the chip with the big stencil kernels, where every
// launch waits for a workgroup slot; two launches per exchange instead of four shorten the chain (tools/exchange_serial_probe.py).
__global__ __launch_bounds__(256) void k_pack_xy(DyP p, const double *__restrict__ S, double *__restrict__ bW, double *__restrict__ bE,
                                                 double *__restrict__ bS, double *__restrict__ bN, unsigned nbx) {
  if (blockIdx.x < nbx) pack_x_body(p, S, bW, bE, (long long)blockIdx.x * 256 + threadIdx.x);
  else pack_y_body(p, S, bS, bN, (long long)(blockIdx.x - nbx) * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void k_unpack_xy(DyP p, double *__restrict__ S, const double *__restrict__ bW, const double *__restrict__ bE,
                                                   const double *__restrict__ bS, const double *__restrict__ bN, unsigned nbx) {
  if (blockIdx.x < nbx) unpack_x_body(p, S, bW, bE, (long long)blockIdx.x * 256 + threadIdx.x);
  else unpack_y_body(p, S, bS, bN, (long long)(blockIdx.x - nbx) * 256 + threadIdx.x);
}

// -----------------------------------------------------------------------------------------------------
// Flux stencil: WENO reconstruction (D6, :271-388) + edge BCs (D8, :1008-1081) + Riemann solver (D9, :395-474)
// fused; one thread per face triple (x-, y-, z- lower faces of cell (k,j,i,e), plus the top/north/east rim).
// The two sides of a face are described by (source cell, which edge); passive variables (transverse momenta,
// tracers) are reconstructed on the upwind side only.
// -----------------------------------------------------------------------------------------------------
template <bool STRICT, int ORD = 5>
__device__ __forceinline__ double edge_value(const double *__restrict__ q, long long st, int right) {
  double l, r;
  if (ORD == 7 || ORD == 9) {
    constexpr int h = (ORD - 1) / 2;
    double s[ORD];
#pragma unroll
    for (int m = 0; m < ORD; m++) s[m] = q[(long long)(m - h) * st];
    if (STRICT) weno79_edges_strict<ORD>(s, l, r); else weno79_edges_fast<ORD>(s, l, r);
  }
  else if (ORD == 3) { if (STRICT) weno3_edges_strict(q[-st], q[0], q[st], l, r); else weno3_edges_fast(q[-st], q[0], q[st], l, r); }
  else if (STRICT) weno5_edges_strict(q[-2 * st], q[-st], q[0], q[st], q[2 * st], l, r);
  else             weno5_edges_fast  (q[-2 * st], q[-st], q[0], q[st], q[2 * st], l, r);
  return right ? r : l;
}

// Background values a face side adds to its reconstructed perturbations: hyr (density), hyt (rho theta), p0 = C0 hyt^gamma, 1/hyt.
// Both sides of a face share them -- except at the two z faces of a z-PERIODIC domain, where the reference copies the finished
// edge value of the opposite boundary face (:1008-1019), hydrostatic part of THAT level included.
struct FaceBg { double hyr, hyt, p0, ihyt; };

template <bool STRICT, int ORD>
__device__ __forceinline__ void face_flux(const DyP &p, const double *__restrict__ cL, int eL, const double *__restrict__ cR,
                                          int eR, long long st, int nrm, const FaceBg &bL, const FaceBg &bR,
                                          bool zero_nrm, double *__restrict__ f, long long fV) {
  const double cs = 350;
  double rL = edge_value<STRICT, ORD>(cL + idR * p.sV, st, eL) + bL.hyr;
  double rR = edge_value<STRICT, ORD>(cR + idR * p.sV, st, eR) + bR.hyr;
  double uL = edge_value<STRICT, ORD>(cL + nrm * p.sV, st, eL);
  double uR = edge_value<STRICT, ORD>(cR + nrm * p.sV, st, eR);
  double eTL = edge_value<STRICT, ORD>(cL + idT * p.sV, st, eL), eTR = edge_value<STRICT, ORD>(cR + idT * p.sV, st, eR);
  double tL = eTL + bL.hyt;
  double tR = eTR + bR.hyt;
  if (STRICT) {
#pragma clang fp contract(off)
    double mL = zero_nrm ? 0.0 : uL * rL;
    double mR = zero_nrm ? 0.0 : uR * rR;
    double p_L = p.C0 * pow_gamma<true>(tL, p.gamma), p_R = p.C0 * pow_gamma<true>(tR, p.gamma);
    double w1 = 0.5 * (p_R - cs * mR);
    double w2 = 0.5 * (p_L + cs * mL);
    double p_upw = w1 + w2;
    double m_upw = (w2 - w1) / cs;
    int ind = (mL + mR > 0) ? 0 : 1;
    double r_upw = ind ? rR : rL;
    const double *cU = ind ? cR : cL;  int eU = ind ? eR : eL;
    f[idR * fV] = m_upw;
    f[nrm * fV] = m_upw * (ind ? mR : mL) / r_upw + p_upw;
    f[idT * fV] = m_upw * (ind ? tR : tL) / r_upw;
    for (int l = idU; l < p.V; l++) {
      if (l == nrm || l == idT) continue;
      double val = edge_value<true, ORD>(cU + l * p.sV, st, eU) * r_upw;
      f[l * fV] = m_upw * val / r_upw;
    }
  } else {
#pragma clang fp contract(fast)
    double mL = zero_nrm ? 0.0 : uL * rL;
    double mR = zero_nrm ? 0.0 : uR * rR;
    double p_L = pressure_fast(p, eTL, bL.hyt, bL.p0, bL.ihyt), p_R = pressure_fast(p, eTR, bR.hyt, bR.p0, bR.ihyt);
    double w1 = 0.5 * (p_R - cs * mR);
    double w2 = 0.5 * (p_L + cs * mL);
    double p_upw = w1 + w2;
    double m_upw = (w2 - w1) * (1.0 / 350.0);
    int ind = (mL + mR > 0) ? 0 : 1;
    double r_upw = ind ? rR : rL;
    const double *cU = ind ? cR : cL;  int eU = ind ? eR : eL;
    double u_upw = zero_nrm ? 0.0 : (ind ? uR : uL);
    f[idR * fV] = m_upw;
    f[nrm * fV] = m_upw * u_upw + p_upw;
    f[idT * fV] = m_upw * (ind ? tR : tL) / r_upw;
    for (int l = idU; l < p.V; l++) {
      if (l == nrm || l == idT) continue;
      f[l * fV] = m_upw * edge_value<false, ORD>(cU + l * p.sV, st, eU);
    }
  }
}

template <bool STRICT, int ORD>
__global__ __launch_bounds__(256) void k_flux(DyP p, const double *__restrict__ S, double *__restrict__ FX,
                                              double *__restrict__ FY, double *__restrict__ FZ) {
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y;
  int NXF = (p.nx + 1) * p.nens;
  int nyf = p.sim2d ? p.ny : p.ny + 1;                       // 2-D: no y faces beyond row 0 needed
  if (t >= (long long)nyf * NXF) return;
  int j = (int)(t / NXF), ie = (int)(t - (long long)j * NXF);
  int i = ie / p.nens, e = ie - i * p.nens;
  const double *c = S + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)(i + p.HX) * p.nens + e;
  // ---------------- X face i-1/2 : left state = right edge of cell i-1, right state = left edge of cell i
  if (j < p.ny && k < p.nz) {
    const double *cL = c - p.nens, *cR = c;  int eL = 1, eR = 0;  bool zero = false;
    if (p.bc_x != MW_BC_PERIODIC) {                          // :1040-1060 (note the else-if: quirk 1)
      if (p.px == 0) {
        if (i == 0) { cL = cR; eL = eR; zero = (p.bc_x == MW_BC_WALL); }
        else if (i == p.nx && p.nproc_x == 1) { cR = c - (long long)p.nx * p.nens; eR = 0; }   // slot 1 at nx keeps what the periodic self-exchange delivered: left edge of cell 0 (:985)
      } else if (p.px == p.nproc_x - 1) {
        if (i == p.nx) { cR = cL; eR = eL; zero = (p.bc_x == MW_BC_WALL); }
      }
    }
    const FaceBg bg = {p.hyc[k * p.nens + e], p.hytc[k * p.nens + e], p.p0c[k * p.nens + e], p.ihytc[k * p.nens + e]};
    face_flux<STRICT, ORD>(p, cL, eL, cR, eR, p.nens, idU, bg, bg, zero, FX + (long long)k * p.fxK + (long long)j * p.fxJ + ie, p.fxV);
  }
  // ---------------- Y face j-1/2
  if (!p.sim2d && i < p.nx && k < p.nz) {
    const double *cL = c - p.sJ, *cR = c;  int eL = 1, eR = 0;  bool zero = false;
    if (p.bc_y != MW_BC_PERIODIC) {                          // :1061-1081
      if (p.py == 0) {
        if (j == 0) { cL = cR; eL = eR; zero = (p.bc_y == MW_BC_WALL); }
        else if (j == p.ny && p.nproc_y == 1) { cR = c - (long long)p.ny * p.sJ; eR = 0; }
      } else if (p.py == p.nproc_y - 1) {
        if (j == p.ny) { cR = cL; eR = eL; zero = (p.bc_y == MW_BC_WALL); }
      }
    }
    const FaceBg bg = {p.hyc[k * p.nens + e], p.hytc[k * p.nens + e], p.p0c[k * p.nens + e], p.ihytc[k * p.nens + e]};
    face_flux<STRICT, ORD>(p, cL, eL, cR, eR, p.sJ, idV, bg, bg, zero, FY + (long long)k * p.fyK + (long long)j * p.fyJ + ie, p.fyV);
  }
  // ---------------- Z face k-1/2 : wall / open edge-value rule at k = 0 and k = nz  (:1020-1038)
  if (i < p.nx && j < p.ny) {
    const double *cL = c - p.sK, *cR = c;  int eL = 1, eR = 0;  bool zero = false;
    int kL = k, kR = k;                                      // which face's hydrostatic edge values each side carries (:368-377)
    if (p.bc_z == MW_BC_PERIODIC) {                          // :1008-1019: slot 0 of face 0 := slot 0 of face nz, slot 1 of face nz := slot 1 of face 0
      if (k == 0)    { cL = c + (long long)(p.nz - 1) * p.sK; kL = p.nz; }       // top edge of cell nz-1, as finished at face nz
      if (k == p.nz) { cR = c - (long long)p.nz * p.sK;       kR = 0;    }       // bottom edge of cell 0, as finished at face 0
    } else {                                                 // :1020-1038 wall / open
      if (k == 0)    { cL = cR; eL = eR; zero = (p.bc_z == MW_BC_WALL); }
      if (k == p.nz) { cR = cL; eR = eL; zero = (p.bc_z == MW_BC_WALL); }
    }
    const FaceBg bL = {p.hye[kL * p.nens + e], p.hyte[kL * p.nens + e], p.p0e[kL * p.nens + e], p.ihyte[kL * p.nens + e]};
    const FaceBg bR = {p.hye[kR * p.nens + e], p.hyte[kR * p.nens + e], p.p0e[kR * p.nens + e], p.ihyte[kR * p.nens + e]};
    face_flux<STRICT, ORD>(p, cL, eL, cR, eR, p.sK, idW, bL, bR, zero,
                      FZ + (long long)k * p.fzK + (long long)j * p.fzJ + (long long)i * p.nens + e, p.fzV);
  }
}

// -----------------------------------------------------------------------------------------------------
// D10  FCT positivity (:498-516).  In-place scaling of outgoing tracer fluxes; race-free by the reference's
// sign argument (:495-497): a face is only ever rescaled by the cell it leaves.
// -----------------------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(256) void k_fct(DyP p, const double *__restrict__ S, double *__restrict__ FX,
                                             double *__restrict__ FY, double *__restrict__ FZ, double dt) {
#pragma clang fp contract(off)
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y, tr = blockIdx.z;
  if (!((p.pos_mask >> tr) & 1u)) return;
  int NXI = p.nx * p.nens;
  if (t >= (long long)p.ny * NXI) return;
  int j = (int)(t / NXI), ie = (int)(t - (long long)j * NXI);
  int e = ie % p.nens;
  const double *s = S + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens + ie;
  double rho = s[idR * p.sV] + p.hyc[k * p.nens + e];
  double tracer = s[(5 + tr) * p.sV] * rho;                 // the re-multiplied value (:482) that FCT reads
  double dx = p.dx, dy = p.dy, dz = p.dz;
  double *fx = FX + (long long)(5 + tr) * p.fxV + (long long)k * p.fxK + (long long)j * p.fxJ + ie;
  double *fy = FY + (long long)(5 + tr) * p.fyV + (long long)k * p.fyK + (long long)j * p.fyJ + ie;
  double *fz = FZ + (long long)(5 + tr) * p.fzV + (long long)k * p.fzK + (long long)j * p.fzJ + ie;
  double fxm = fx[0], fxp = fx[p.nens], fym = fy[0], fyp = fy[p.fyJ], fzm = fz[0], fzp = fz[p.fzK];
  double mass_available = fmax(tracer, 0.0) * dx * dy * dz;
  double flux_out_x, flux_out_y, flux_out_z;
  if (FAST) {   // production path: multiply by the reciprocal grid spacings (1 ulp from the reference's divisions)
    flux_out_x = (fmax(fxp, 0.0) - fmin(fxm, 0.0)) * p.rdx;
    flux_out_y = (fmax(fyp, 0.0) - fmin(fym, 0.0)) * p.rdy;
    flux_out_z = (fmax(fzp, 0.0) - fmin(fzm, 0.0)) * p.rdz;
  } else {
    flux_out_x = (fmax(fxp, 0.0) - fmin(fxm, 0.0)) / dx;
    flux_out_y = (fmax(fyp, 0.0) - fmin(fym, 0.0)) / dy;
    flux_out_z = (fmax(fzp, 0.0) - fmin(fzm, 0.0)) / dz;
  }
  double mass_out = (flux_out_x + flux_out_y + flux_out_z) * dt * dx * dy * dz;
  if (mass_out > mass_available) {
    double mult = mass_available / mass_out;
    if (fxp > 0) fx[p.nens] = fxp * mult;
    if (fxm < 0) fx[0]      = fxm * mult;
    if (fyp > 0) fy[p.fyJ]  = fyp * mult;
    if (fym < 0) fy[0]      = fym * mult;
    if (fzp > 0) fz[p.fzK]  = fzp * mult;
    if (fzm < 0) fz[0]      = fzm * mult;
  }
}

// -----------------------------------------------------------------------------------------------------
// D11 tendencies (:519-551) + D12 SSPRK3 combine (:121-174) + storage divide (next stage's D2, :248-255)
//   MODE 0: write the new slab (stored form)            STAGE 1: q* = q^n + dt L(q^n)
//   MODE 1: last stage of the last cycle: write the     STAGE 2: q* = 3/4 q^n + 1/4 q* + 1/4 dt L(q*)
//           COUPLER fields directly (D13, :1927-1950)    STAGE 3: q  = 1/3 q^n + 2/3 q* + 2/3 dt L(q*)
//   MODE 2: write tendencies only (mw_dycore_compute_tendencies)
// Sstar = slab the fluxes were computed from; Sn = q^n slab (== Sstar in stage 1).
// -----------------------------------------------------------------------------------------------------
template <int STAGE, int MODE>
__global__ __launch_bounds__(256) void k_update(DyP p, const double *Sstar, const double *Sn,   // may alias Sout (in-place stages)
                                                double *Sout, const double *__restrict__ FX,
                                                const double *__restrict__ FY, const double *__restrict__ FZ,
                                                double dt_stage, double dt_dyn, CouplerPtrs c,
                                                double *__restrict__ state_tend, double *__restrict__ tracers_tend) {
#pragma clang fp contract(off)
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int k = blockIdx.y;
  int NXI = p.nx * p.nens;
  if (t >= (long long)p.ny * NXI) return;
  int j = (int)(t / NXI), ie = (int)(t - (long long)j * NXI);
  int e = ie % p.nens;
  long long so = (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens + ie;
  long long ci = ((long long)k * p.ny + j) * NXI + ie;
  const double *fx = FX + (long long)k * p.fxK + (long long)j * p.fxJ + ie;
  const double *fy = FY + (long long)k * p.fyK + (long long)j * p.fyJ + ie;
  const double *fz = FZ + (long long)k * p.fzK + (long long)j * p.fzJ + ie;
  const double hyc = p.hyc[k * p.nens + e], hytc = p.hytc[k * p.nens + e];
  const double dx = p.dx, dy = p.dy, dz = p.dz;
  const double rho_s = Sstar[so + idR * p.sV] + hyc;                 // density of the stage input
  const double rho_n = (STAGE == 1) ? rho_s : Sn[so + idR * p.sV] + hyc;
  // immersed-boundary relaxation coefficients (:534-550)
  double prop = 0, imm_coef = 0;
  if (p.use_immersed) {
    double tau = 1.e3 * dt_stage;
    imm_coef = -fmin(1.0, dt_stage / tau);
    prop = p.imm[ci];
  }
  const double ru_s = Sstar[so + idU * p.sV] * rho_s;                // re-multiplied momenta (:478-480)
  const double rv_s = Sstar[so + idV * p.sV] * rho_s;
  double newR = 0, rho_new = 0;                                      // filled at l == idR (first iteration)
  double rho_dry_acc = 0, rho_v_new = 0, press_arg = 0, unew = 0, vnew = 0, wnew = 0;
  for (int l = 0; l < p.V; l++) {
    // conserved value of the stage input and of q^n
    double raw_s = Sstar[so + l * p.sV];
    double q_s = (l == idR || l == idT) ? raw_s : raw_s * rho_s;
    double q_n;
    if (STAGE == 1) q_n = q_s;
    else { double raw_n = Sn[so + l * p.sV]; q_n = (l == idR || l == idT) ? raw_n : raw_n * rho_n; }
    double tend = -(fx[l * p.fxV + p.nens] - fx[l * p.fxV]) / dx
                  -(fy[l * p.fyV + p.fyJ ] - fy[l * p.fyV]) / dy
                  -(fz[l * p.fzV + p.fzK ] - fz[l * p.fzV]) / dz;
    if (l == idW && p.enable_gravity) tend += -p.grav * rho_s;
    if (l == idU) tend += p.fcor * rv_s;
    if (l == idV) tend -= p.fcor * ru_s;
    if (l == idV && p.sim2d) tend = 0;
    if (p.use_immersed && l < 5) {
      double imm_tend = imm_coef * q_s / dt_stage;
      tend = prop * imm_tend + (1 - prop) * tend;
    }
    if (MODE == 2) {
      if (l < 5) state_tend[(long long)l * p.nC + ci] = tend;
      else       tracers_tend[(long long)(l - 5) * p.nC + ci] = tend;
      continue;
    }
    double qnew;
    if (STAGE == 1)      qnew = q_n + dt_dyn * tend;
    else if (STAGE == 2) qnew = (3.0 / 4.0) * q_n + (1.0 / 4.0) * q_s + (1.0 / 4.0) * dt_dyn * tend;
    else                 qnew = (1.0 / 3.0) * q_n + (2.0 / 3.0) * q_s + (2.0 / 3.0) * dt_dyn * tend;
    if (l >= 5 && ((p.pos_mask >> (l - 5)) & 1u)) qnew = fmax(0.0, qnew);
    if (l == idR) { newR = qnew; rho_new = newR + hyc; rho_dry_acc = rho_new; }
    if (MODE == 0) {
      Sout[so + l * p.sV] = (l == idR || l == idT) ? qnew : qnew / rho_new;
    } else {  // MODE 1: convert_dynamics_to_coupler (:1927-1950)
      if (l == idU) unew = qnew / rho_new;
      if (l == idV) vnew = qnew / rho_new;
      if (l == idW) wnew = qnew / rho_new;
      if (l == idT) { double theta = (qnew + hytc) / rho_new; press_arg = rho_new * theta; }
      if (l >= 5) {
        c.tr[l - 5][ci] = qnew;
        if (l - 5 == p.idWV) rho_v_new = qnew;
        if ((p.mass_mask >> (l - 5)) & 1u) rho_dry_acc -= qnew;
      }
    }
  }
  if (MODE == 1) {
    double press = p.C0 * pow_ref(press_arg, p.gamma);
    double temp = press / (rho_dry_acc * p.R_d + rho_v_new * p.R_v);
    c.rho_d[ci] = rho_dry_acc;  c.u[ci] = unew;  c.v[ci] = vnew;  c.w[ci] = wnew;  c.temp[ci] = temp;
  }
}


// member-major slab (nens, V, nz+2HZ, ny+2HY, nx+2HX) -> the fused layout (V, nz+2HZ, ny+2HY, (nx+2HX)*nens), halos included.
// p = the FUSED parameter block.  Used when the public flux arrays are rebuilt from a stage input of the production path.
__global__ __launch_bounds__(256) void k_member_to_fused(DyP p, const double *__restrict__ src, double *__restrict__ dst) {
  const long long n = (long long)p.V * p.sV;                  // fused elements
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int e = (int)(t % p.nens);
  const long long r = t / p.nens;                             // (v, k, j, i) with the member-major strides
  dst[t] = src[(long long)e * (n / p.nens) + r];
}

// ColumnNudger's increment (column_nudging.h:62-65): dt (column - average) / time_scale, one number per (field, level, member) -- the
// reference's expression, IEEE division, no contraction (= k_nudge_apply in mw_column.hip).
__global__ __launch_bounds__(256) void k_nudge_increments(const double *__restrict__ column, const double *__restrict__ avg, double dt, long long n, double *__restrict__ inc) {
#pragma clang fp contract(off)
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const double time_scale = 900;
  if (t < n) inc[t] = dt * (column[t] - avg[t]) / time_scale;
}
// ... and parked increments applied by a pass after all (mw_dycore_flush_pending: somebody wants to see the fields before the next time step,
// or the next time step runs a path whose conversion does not take them along): state(l,k,j,i,e) += inc(l,k,e), the same rounded addition.
struct Ptr5 { double *f[5]; };
__global__ __launch_bounds__(256) void k_apply_pending(Ptr5 fp, int nz, long long ncell_lev, int nens, const double *__restrict__ inc) {
#pragma clang fp contract(off)
  const int k = blockIdx.y, l = blockIdx.z;
  const long long n = ncell_lev * nens;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const int e = (int)(t % nens);
    double *q = fp.f[l] + (long long)k * n;
    q[t] = q[t] + inc[((long long)l * nz + k) * nens + e];
  }
}

} // namespace mw

// =====================================================================================================
// Host side
// =====================================================================================================

void fill_params(mw_dycore_s *d) {
  const mw_grid_t &g = d->g;  DyP &p = d->p;
  p.nz = g.nz; p.ny = g.ny; p.nx = g.nx; p.nens = g.nens; p.nt = g.num_tracers; p.V = 5 + g.num_tracers;
  p.sim2d = (g.ny_glob == 1);
  p.HX = d->hxw; p.HY = p.sim2d ? 0 : d->hxw; p.HZ = d->hzw;
  p.NXE = (g.nx + 2 * p.HX) * g.nens;
  p.sJ = p.NXE; p.sK = (long long)(g.ny + 2 * p.HY) * p.sJ; p.sV = (long long)(g.nz + 2 * p.HZ) * p.sK;
  p.nC = (long long)g.nz * g.ny * g.nx * g.nens;
  p.fxJ = (long long)(g.nx + 1) * g.nens; p.fxK = (long long)g.ny * p.fxJ;       p.fxV = (long long)g.nz * p.fxK;
  p.fyJ = (long long)g.nx * g.nens;       p.fyK = (long long)(g.ny + 1) * p.fyJ; p.fyV = (long long)g.nz * p.fyK;
  p.fzJ = (long long)g.nx * g.nens;       p.fzK = (long long)g.ny * p.fzJ;       p.fzV = (long long)(g.nz + 1) * p.fzK;
  // (Stride32: the largest stride is a slab's variable stride; the products above were formed from converted values, so check it in 64 bits)
  d->strides_ok = (long long)(g.nz + 2 * p.HZ) * (long long)(g.ny + 2 * p.HY) * (long long)p.NXE <= 2147483647ll &&
                  (long long)(g.nz + 1) * (long long)(g.ny + 1) * (long long)(g.nx + 1) * g.nens <= 2147483647ll;
  p.v0 = 0; p.wrap_x = 0; p.wrap_y = 0; p.cst = 1; p.ce = 0;
  p.bc_x = g.bc_x; p.bc_y = g.bc_y; p.bc_z = g.bc_z; p.px = g.px; p.py = g.py; p.nproc_x = g.nproc_x; p.nproc_y = g.nproc_y;
  p.enable_gravity = g.enable_gravity; p.use_immersed = g.use_immersed; p.idWV = g.idWV;
  p.zero_skip = d->o.zero_skip;
  p.zq = p.zqp = p.zqc = p.zqk = nullptr; p.zq_ld = 0;          // (set per RK stage by zero_rows_stage / zero_rows_conv)
  p.zq_xper = (g.bc_x == MW_BC_PERIODIC && !(d->xchg && g.nproc_x > 1)) ? 1 : 0;
  p.pinc = nullptr;                                             // (set by mw_dycore_time_step when parked increments ride on the conversion)
  p.pos_mask = 0; p.mass_mask = 0;
  for (int t = 0; t < g.num_tracers; t++) { if (d->pos[t]) p.pos_mask |= 1u << t; if (d->adds[t]) p.mass_mask |= 1u << t; }
  p.dx = g.xlen / g.nx_glob; p.dy = g.ylen / g.ny_glob; p.dz = g.zlen / g.nz;        // coupler.h:262-268
  p.rdx = 1.0 / p.dx; p.rdy = 1.0 / p.dy; p.rdz = 1.0 / p.dz;
  p.C0 = g.C0; p.gamma = g.gamma_d; p.grav = g.grav; p.R_d = g.R_d; p.R_v = g.R_v;
  p.fcor = 2 * g.earthrot * sin(g.latitude);                                           // :213
  size_t nzc = (size_t)g.nz * g.nens, nze = (size_t)(g.nz + 1) * g.nens;
  p.hyc = d->hy_dev; p.hytc = d->hy_dev + nzc; p.hye = d->hy_dev + 2 * nzc; p.hyte = d->hy_dev + 2 * nzc + nze;
  const double *ext = d->hy_dev + 2 * nzc + 2 * nze;
  p.p0c = ext; p.ihytc = ext + nzc; p.p0e = ext + 2 * nzc; p.ihyte = ext + 2 * nzc + nze;
  p.imm = d->imm;
  p.hypk = d->hy_dev + 4 * nzc + 4 * nze;
  long double bn = 1.0L;                                    // C(gamma, n) = C(gamma, n-1) (gamma - n + 1) / n
  p.bn[0] = 1.0;
  for (int n = 1; n <= 10; n++) { bn = bn * ((long double)g.gamma_d - (n - 1)) / n; p.bn[n] = (double)bn; }
  p.bn_default = 1;
  for (int n = 0; n <= 10; n++) if (p.bn[n] != BN_DEFAULT[n]) p.bn_default = 0;
  { static const double AN_DEFAULT[11] = {1.0, 0x1.6d7ed9f857ccfp-1, -0x1.a255770e765c3p-4, 0x1.66b0e7bdc9cadp-5, -0x1.9a025de3c9f2fp-6,
                                         0x1.0d783d4c75011p-6, -0x1.80febd2957c9ap-7, 0x1.22bbebca1e45p-7, -0x1.c8e61cbaa3102p-8,
                                         0x1.71e467e9895fp-8, -0x1.327f77d85aeeep-8};
    const long double a = 1.0L / (long double)g.gamma_d;
    long double an = 1.0L;                                  // C(1/gamma, n)
    p.an_default = 1;
    for (int n = 1; n <= 10; n++) { an = an * (a - (n - 1)) / n; if ((double)an != AN_DEFAULT[n]) p.an_default = 0; } }
}

int upload_background(mw_dycore_s *d) {
  {  // derived tables of the fast pressure path: p0 = C0 hyt^gamma, 1/hyt (cells and edges)
    const mw_grid_t &g = d->g;
    size_t nzc = (size_t)g.nz * g.nens, nze = (size_t)(g.nz + 1) * g.nens;
    double *h = d->hy_host.data();
    const double *hytc = h + nzc, *hyte = h + 2 * nzc + nze;
    double *ext = h + 2 * nzc + 2 * nze;
    for (size_t n = 0; n < nzc; n++) { ext[n] = g.C0 * pow(hytc[n], g.gamma_d); ext[nzc + n] = 1.0 / hytc[n]; }
    for (size_t n = 0; n < nze; n++) { ext[2 * nzc + n] = g.C0 * pow(hyte[n], g.gamma_d); ext[2 * nzc + nze + n] = 1.0 / hyte[n]; }
    double *pk = h + 4 * nzc + 4 * nze;                      // packed rows
    const double *src[8] = {h, h + nzc, ext, ext + nzc, h + 2 * nzc, h + 2 * nzc + nze, ext + 2 * nzc, ext + 2 * nzc + nze};
    for (size_t n = 0; n < nze; n++) for (int f = 0; f < 8; f++) pk[n * 8 + f] = (f < 4 && n >= nzc) ? 0.0 : src[f][n];
    // member-major copies (View): member e's columns contiguous, so that the nens = 1 kernels index them with k alone
    double *mm = pk + 8 * nze;
    const size_t per = 4 * (size_t)g.nz + 8 * (size_t)(g.nz + 1);
    for (int e = 0; e < g.nens; e++) {
      double *m = mm + (size_t)e * per;
      for (int k = 0; k < g.nz; k++) { const size_t n = (size_t)k * g.nens + e;
        m[k] = h[n]; m[g.nz + k] = hytc[n]; m[2 * g.nz + k] = ext[n]; m[3 * g.nz + k] = ext[nzc + n]; }
      double *mpk = m + 4 * g.nz;
      for (int k = 0; k <= g.nz; k++) for (int f = 0; f < 8; f++) mpk[(size_t)k * 8 + f] = pk[((size_t)k * g.nens + e) * 8 + f];
    }
  }
  MW_HIP(hipMemcpyAsync(d->hy_dev, d->hy_host.data(), d->hy_host.size() * sizeof(double), hipMemcpyHostToDevice, d->stream));
  MW_HIP(hipStreamSynchronize(d->stream));
  return 0;
}

int n_views(const mw_dycore_s *d) { return d->member_major ? d->p.nens : 1; }
View view(const mw_dycore_s *d, int e) {
  View v; v.e = e; v.p = d->p;
  v.slab = v.tend = v.cells = 0; for (int a = 0; a < 3; a++) v.m[a] = v.f[a] = 0;
  if (!d->member_major) { v.e = 0; return v; }
  DyP &q = v.p;
  const int n = d->p.nens;
  q.nens = 1; q.cst = n; q.ce = e;
  q.NXE = q.nx + 2 * q.HX;
  q.sJ = q.NXE; q.sK = (long long)(q.ny + 2 * q.HY) * q.sJ; q.sV = (long long)(q.nz + 2 * q.HZ) * q.sK;
  q.nC = (long long)q.nz * q.ny * q.nx;
  q.fxJ = q.nx + 1; q.fxK = (long long)q.ny * q.fxJ;       q.fxV = (long long)q.nz * q.fxK;
  q.fyJ = q.nx;     q.fyK = (long long)(q.ny + 1) * q.fyJ; q.fyV = (long long)q.nz * q.fyK;
  q.fzJ = q.nx;     q.fzK = (long long)q.ny * q.fzJ;       q.fzV = (long long)(q.nz + 1) * q.fzK;
  const size_t nzc = (size_t)q.nz * n, nze = (size_t)(q.nz + 1) * n, per = 4 * (size_t)q.nz + 8 * (size_t)(q.nz + 1);
  const double *m = d->hy_dev + 4 * nzc + 4 * nze + 8 * nze + (size_t)e * per;
  q.hyc = m; q.hytc = m + q.nz; q.p0c = m + 2 * q.nz; q.ihytc = m + 3 * q.nz; q.hypk = m + 4 * q.nz;
  q.hye = q.hyte = q.p0e = q.ihyte = nullptr;              // (edge tables: only through hypk on this path)
  if (q.zq) {                                                  // the member's own zero-row maps (zero_rows_build)
    const long long mstride = d->zr.member_words();
    q.zq += e * mstride; if (q.zqp) q.zqp += e * mstride;
    q.zqc = q.zqk = nullptr;
  }
  v.slab = (long long)q.V * q.sV; v.tend = 5 * q.nC; v.cells = q.nC;
  v.m[0] = q.fxV; v.m[1] = q.fyV; v.m[2] = q.fzV;
  v.f[0] = (long long)q.V * q.fxV; v.f[1] = (long long)q.V * q.fyV; v.f[2] = (long long)q.V * q.fzV;
  return v;
}

// the member-to-member strides of a member-major handle, for the member-transposing kernels (MemberOff, mw_march.h)
MemberOff member_off(const mw_dycore_s *d) {
  const View v = view(d, 0);
  MemberOff mo;
  mo.slab = v.slab; mo.tend = v.tend; mo.mx = v.m[0]; mo.my = v.m[1]; mo.mz = v.m[2]; mo.fx = v.f[0]; mo.fy = v.f[1]; mo.fz = v.f[2];
  mo.cells = v.cells; mo.per = 4 * (long long)v.p.nz + 8 * (long long)(v.p.nz + 1);
  mo.n = d->p.nens; mo.sh = d->p.nens == 4 ? 2 : 1;
  mo.zq = d->zr.member_words();
  return mo;
}

// halo fill of variables [v0, v0+nv) of one slab: neighbour exchange (or self wrap) in x/y, then BCs -- replaces
// halo_exchange (:574-827).  `grp` selects the pack-buffer set (0: state or all variables, 1: tracers).
int halo_fill(mw_dycore_s *d, double *Sbase, int v0, int nv, hipStream_t st, int grp, bool skip_z) {
  if (!st) st = d->stream;
  if (nv < 0) nv = d->p.V;
  if (nv == 0) return 0;
  ProfScope ps(d, 3, st);
  // skip_z = production path; with a member-major handle the slab holds one member after the other: every kernel below runs once
  // per member on its nens = 1 view, and the strips of member e sit at e * (strip size / nens) in the exchange buffers
  const int nv_views = (skip_z && d->member_major) ? d->p.nens : 1;
  const DyP &pf = d->p;
  bool ex_x = d->xchg && (pf.nproc_x > 1), ex_y = d->xchg && (pf.nproc_y > 1) && !pf.sim2d;
  long long nWE = d->nWE1 * nv, nSN = d->nSN1 * nv;              // all members
  const long long mWE = nWE / nv_views, mSN = nSN / nv_views;    // one view
  double **bf = d->bufs[grp];
  auto member = [&](int e, DyP &q, double *&S) {
    View v; if (nv_views > 1) v = view(d, e); else { v.p = d->p; v.e = 0; v.slab = 0; }
    q = v.p; q.v0 = v0; q.V = nv;
    S = Sbase + e * v.slab + (long long)v0 * q.sV;
  };
  if (ex_x || ex_y) {
    // a rank grid with more than one rank in a direction: ship 3-cell strips to the face neighbours.
    // Directions with a single rank still wrap locally below.
    for (int e = 0; e < nv_views; e++) {
      DyP q; double *S; member(e, q, S);
      const unsigned nbx = ex_x ? (unsigned)((mWE + 255) / 256) : 0u, nby = ex_y ? (unsigned)((mSN + 255) / 256) : 0u;
      MW_KLAUNCH(k_pack_xy, dim3(nbx + nby), dim3(256), 0, st, q, S, bf[0] + e * mWE, bf[1] + e * mWE, bf[2] + e * mSN, bf[3] + e * mSN, nbx); MW_LAUNCH_CHECK();
    }
    int rc = d->xchg(d->xchg_ctx, ex_x ? bf[0] : nullptr, ex_x ? bf[1] : nullptr, ex_y ? bf[2] : nullptr, ex_y ? bf[3] : nullptr,
                     ex_x ? bf[4] : nullptr, ex_x ? bf[5] : nullptr, ex_y ? bf[6] : nullptr, ex_y ? bf[7] : nullptr, ex_x ? nWE : 0,
                     ex_y ? nSN : 0, st);
    if (rc) MW_FAIL("halo exchange callback failed");
    for (int e = 0; e < nv_views; e++) {
      DyP q; double *S; member(e, q, S);
      const unsigned nbx = ex_x ? (unsigned)((mWE + 255) / 256) : 0u, nby = ex_y ? (unsigned)((mSN + 255) / 256) : 0u;
      MW_KLAUNCH(k_unpack_xy, dim3(nbx + nby), dim3(256), 0, st, q, S, bf[4] + e * mWE, bf[5] + e * mWE, bf[6] + e * mSN, bf[7] + e * mSN, nbx); MW_LAUNCH_CHECK();
    }
  }
  // local wrap / BC:  x when this direction has one rank (periodic self-wrap), or a wall / open boundary on a domain-edge rank.
  // With several ranks in a non-periodic direction the edge ranks have just exchanged with their periodic-wrap neighbour like
  // the reference does (:641-723 uses the periodic neighbour matrix) and the boundary rule then OVERWRITES that halo
  // (:782-825: `px == 0` west side, `px == nproc_x-1` east side; the kernel skips the sides that are rank-interior).
  for (int e = 0; e < nv_views; e++) {
    DyP q; double *S; member(e, q, S);
    const DyP &p = q;
    const bool edge_x = (p.px == 0 || p.px == p.nproc_x - 1), edge_y = (p.py == 0 || p.py == p.nproc_y - 1);
    const bool bcx_after = ex_x && p.bc_x != MW_BC_PERIODIC && edge_x, bcy_after = ex_y && p.bc_y != MW_BC_PERIODIC && edge_y;
    const long long nx_ = (long long)p.V * p.nz * p.ny * 2 * p.HX * p.nens;
    const long long ny_ = (long long)p.V * p.nz * 2 * p.HY * p.nx * p.nens;
    const long long nz_ = (long long)p.V * 2 * p.HZ * p.ny * p.nx * p.nens;
    const unsigned nbx = ((ex_x && !bcx_after) || (skip_z && p.wrap_x)) ? 0u : (unsigned)((nx_ + 255) / 256);      // skip_z = production path
    const unsigned nby = ((ex_y && !bcy_after) || p.sim2d || (skip_z && p.wrap_y)) ? 0u : (unsigned)((ny_ + 255) / 256);
    const unsigned nbz = skip_z ? 0u : (unsigned)((nz_ + 255) / 256);      // (the marching kernels apply the z rule while loading)
    if (nbx + nby + nbz) { MW_KLAUNCH(k_halo_xyz, dim3(nbx + nby + nbz), dim3(256), 0, st, p, S, nbx, nby); MW_LAUNCH_CHECK(); }
  }
  return 0;
}

static int launch_flux(mw_dycore_s *d, const double *S) {
  ProfScope ps(d, 0);
  const DyP &p = d->p;
  long long per_plane = (long long)(p.sim2d ? p.ny : p.ny + 1) * (p.nx + 1) * p.nens;
  dim3 grid = plane_grid(per_plane, p.nz + 1);
  if (d->ord == 3) {
    if (d->strict == 1) MW_KLAUNCH((k_flux<true, 3>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
    else                MW_KLAUNCH((k_flux<false, 3>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
  } else if (d->ord == 7) {
    if (d->strict == 1) MW_KLAUNCH((k_flux<true, 7>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
    else                MW_KLAUNCH((k_flux<false, 7>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
  } else if (d->ord == 9) {
    if (d->strict == 1) MW_KLAUNCH((k_flux<true, 9>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
    else                MW_KLAUNCH((k_flux<false, 9>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
  } else {
    if (d->strict == 1) MW_KLAUNCH((k_flux<true, 5>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
    else                MW_KLAUNCH((k_flux<false, 5>), grid, dim3(256), 0, d->stream, p, S, d->FX, d->FY, d->FZ);
  }
  MW_LAUNCH_CHECK();
  return 0;
}

static int launch_fct(mw_dycore_s *d, const double *S, double dt, hipStream_t st = nullptr) {
  const DyP &p = d->p;
  if (!st) st = d->stream;
  if (p.nt == 0 || p.pos_mask == 0) return 0;
  ProfScope ps(d, 1, st);
  dim3 grid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz, p.nt);
  if (d->strict == 1) MW_KLAUNCH(k_fct<false>, grid, dim3(256), 0, st, p, S, d->FX, d->FY, d->FZ, dt);
  else                MW_KLAUNCH(k_fct<true>, grid, dim3(256), 0, st, p, S, d->FX, d->FY, d->FZ, dt);
  MW_LAUNCH_CHECK();
  return 0;
}

template <int STAGE, int MODE>
static int launch_update(mw_dycore_s *d, const double *Sstar, const double *Sn, double *Sout, double dt_stage, double dt_dyn,
                         const CouplerPtrs &c, double *st, double *tt) {
  ProfScope ps(d, 2);
  const DyP &p = d->p;
  dim3 grid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz);
  MW_KLAUNCH((k_update<STAGE, MODE>), grid, dim3(256), 0, d->stream, p, Sstar, Sn, Sout, d->FX, d->FY, d->FZ, dt_stage,
                     dt_dyn, c, st, tt);
  MW_LAUNCH_CHECK();
  return 0;
}

// Equal chunks along the marching direction: enough of them for `target` waves (x/z kernels: ~5 rounds of 2 waves/SIMD over
// the 1024 SIMDs), none shorter than 8 cells (every chunk re-primes its pipeline).
// The count of chunks decides how many workgroups a CU holds at once, and that quantises the run time -- measured on 100 x 100 x 50:
// 0.37 ms per step with 10 chunks of 5 levels (250 workgroups: one per CU, every wave alone on its SIMD), 0.47 ms with 6 chunks of
// 9 (300 workgroups: 44 CUs hold two).  Model: duration = t(B) * (chunk + o) * (1 + chunk / 1000) with B workgroups on 256 CUs that
// hold `bpc` of them each; a CU's last, partly filled round costs less than a full one (a wave that has its SIMD to itself runs
// ~1.7 x faster); o = cells of work a chunk adds (ghost levels, pipeline priming); the last factor is what long chunks lose in
// cache locality.  Fitted to chunk sweeps on 100 x 100 x 50, 200 x 200 x 50, 256 x 256 x 64, 300 x 300 x 80 and 400 x 400 x 100
// (tools/tail_probe.py); `model` = false keeps the older rule (enough chunks for `target` waves, none under 8 cells).
int balanced_chunk(const mw_dycore_s *d, int nz, long long base_waves, int forced, long long target, int bpc, double o, bool model) {
  if (forced > 0) return std::min(nz, forced);                 // (options chunk_y / chunk_yt / chunk_z / chunk_f)
  long long nch = std::max(1ll, (target + base_waves - 1) / base_waves);
  nch = std::min<long long>(nch, std::max(1, nz / 8));
  const long long cap = 256ll * bpc;
  if (!model || !d->o.chunk_model) return (int)((nz + nch - 1) / nch);
  auto t_of = [&](long long B) {
    const long long full = B / cap, rem = B - full * cap;
    if (rem == 0) return (double)full;
    const long long m = (rem + 255) / 256;                     // workgroups per CU in the last round
    const double part = (bpc == 2) ? (m == 1 ? 0.6 : 1.0) : (m == 1 ? 0.45 : m == 2 ? 0.75 : 1.0);
    return (double)full + part;
  };
  auto cost_of = [&](int chunk) {
    const int neff = (nz + chunk - 1) / chunk;                 // the chunk length decides; neff chunks result
    return t_of(((base_waves + 3) / 4) * neff) * (chunk + o) * (1.0 + 0.001 * chunk);
  };
  const int old_chunk = (int)((nz + nch - 1) / nch);
  double best = 1e300; int best_chunk = nz;
  for (int n = 1; n <= std::max(1, nz / 4); n++) {
    const int chunk = (nz + n - 1) / n;
    const double cost = cost_of(chunk);
    if (cost < best * (1.0 - 1e-9)) { best = cost; best_chunk = chunk; }
  }
  // the model is crude: it overrides the older rule only where it promises more than 3 % (small and odd-sized launches: 9-26 %
  // measured; the tuned large grids keep their chunks)
  return (best < 0.97 * cost_of(old_chunk)) ? best_chunk : old_chunk;
}

int device_cus() {
  static int n = -1;
  if (n < 0) { int dev = 0; hipDeviceProp_t pr; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) n = pr.multiProcessorCount; else n = 0; }
  return n;
}
// Which compile-time configuration of the marching kernels (Cf<K>) fits this view of the handle: 1 / 2 = the shipped supercell /
// simple_city set-ups with their run-time switches folded, 0 = everything at run time.  Option "spec" = 0 forces 0 (A/B timing, tests).
int marching_config(const mw_dycore_s *d, const DyP &p) {
  if (!d->o.spec) return 0;                                    // (option "spec" = 0: A/B timing, tests)
  const unsigned all = (1u << p.nt) - 1u;
  if (p.nens != 1 || p.sim2d || p.bc_x != MW_BC_PERIODIC || p.bc_y != MW_BC_PERIODIC || p.bc_z != MW_BC_WALL || p.fcor != 0.0 ||
      !p.bn_default || !p.an_default || p.pos_mask != all || p.mass_mask != all || p.idWV != 0) return 0;
  if (p.nt == 3 && !p.use_immersed && p.enable_gravity) return 1;
  if (p.nt == 1 && p.use_immersed && !p.enable_gravity) return 2;
  return 0;
}


// y faces of all variables in one launch (k_y_all): one-stream schedule, up to three tracers.  (With the switches at run time, K = 0,
// the eight register windows do not fit -- 90-96 VGPRs go to scratch -- and the one launch is still 2.5 % of the step faster than
// k_y_state + k_y_tracers: 5.44-5.49 against 5.57-5.62 ms on the supercell grid with MW_NO_SPEC=1.)
bool y_all_ok(const mw_dycore_s *d) {
  return !d->overlap && d->fused && !d->p.sim2d && d->p.nt <= 3 && d->o.y_all;
}

int make_coupler_ptrs(mw_dycore_s *d, const double *rho_d, const double *u, const double *v, const double *w,
                             const double *temp, double *const *tracers, CouplerPtrs &c) {
  if (!rho_d || !u || !v || !w || !temp || (d->g.num_tracers > 0 && !tracers)) MW_FAIL("null field pointer");
  c.rho_d = (double *)rho_d; c.u = (double *)u; c.v = (double *)v; c.w = (double *)w; c.temp = (double *)temp;
  for (int t = 0; t < MW_MAX_TRACERS; t++) c.tr[t] = (t < d->g.num_tracers) ? tracers[t] : nullptr;
  for (int t = 0; t < d->g.num_tracers; t++) if (!c.tr[t]) MW_FAIL("null tracer pointer");
  return 0;
}

// A block of a decomposed domain needs its neighbours' strips: without a transport the halo fill would wrap the block onto
// itself and the result would be silently wrong (the reference always exchanges, :641-723).
static int need_exchange(const mw_dycore_s *d) {
  const mw_grid_t &g = d->g;
  if (!d->xchg && (g.nproc_x > 1 || (g.nproc_y > 1 && g.ny_glob != 1)))
    MW_FAIL("this handle is one block of a " + std::to_string(g.nproc_x) + " x " + std::to_string(g.nproc_y) +
            " rank grid but no halo-exchange transport is installed (mw_dycore_use_rccl / mw_dycore_set_exchange)");
  return 0;
}

static int validate_grid(const mw_grid_t *g) {
  if (!g) MW_FAIL("null grid");
  if (g->nz < 3 || g->nx < 3 || g->ny < 1 || g->nens < 1) MW_FAIL("grid too small (need nz,nx >= 3, ny >= 1, nens >= 1)");
  if (g->ny_glob != 1 && g->ny < 3) MW_FAIL("3-D runs need ny >= 3 per rank");
  if (g->num_tracers < 1 || g->num_tracers > MW_MAX_TRACERS) MW_FAIL("num_tracers must be in [1, MW_MAX_TRACERS] (a water_vapor tracer is required, SURVEY 8(a) quirk 6)");
  if (g->idWV < 0 || g->idWV >= g->num_tracers) MW_FAIL("idWV out of range");
  for (int b : {g->bc_x, g->bc_y, g->bc_z}) if (b != MW_BC_PERIODIC && b != MW_BC_OPEN && b != MW_BC_WALL) MW_FAIL("bc_x / bc_y / bc_z must be 0 (periodic), 1 (open) or 2 (wall)");
  return 0;
}

// The halo kernels fill a periodic halo from the interior of the SAME block (halo_x_body: src = ih + nx) and the pack kernels read
// HX / HY interior cells per side: a block narrower than its halo would read halo cells that are not filled yet and give silently
// wrong results.  (3 cells up to WENO-5; 4 / 5 for orders 7 / 9; z only when bc_z is periodic -- wall / open copy one level.)
static int check_halo_fit(const mw_dycore_s *d) {
  const DyP &p = d->p;
  if (p.nx < p.HX) MW_FAIL("nx = " + std::to_string(p.nx) + " per rank is narrower than the x halo of WENO order " + std::to_string(d->ord) + " (" + std::to_string(p.HX) + " cells)");
  if (!p.sim2d && p.ny < p.HY) MW_FAIL("ny = " + std::to_string(p.ny) + " per rank is narrower than the y halo of WENO order " + std::to_string(d->ord) + " (" + std::to_string(p.HY) + " cells)");
  if (p.bc_z == MW_BC_PERIODIC && p.nz < p.HZ) MW_FAIL("nz = " + std::to_string(p.nz) + " is smaller than the z halo of WENO order " + std::to_string(d->ord) + " (" + std::to_string(p.HZ) + " levels) with bc_z = periodic");
  return 0;
}

extern "C" {

int mw_dycore_create(mw_dycore_t *h, const mw_grid_t *g, const unsigned char *tracer_positive,
                     const unsigned char *tracer_adds_mass, void *stream) {
  if (!h) MW_FAIL("null handle pointer");
  if (validate_grid(g)) return 1;
  if (mw_device_count() < 1) MW_FAIL("no HIP device available: libmw_cdna4 has no CPU fallback");
  mw_dycore_s *d = new mw_dycore_s();
  d->g = *g;
  for (int t = 0; t < MW_MAX_TRACERS; t++) { d->pos[t] = (t < g->num_tracers && tracer_positive) ? tracer_positive[t] : 0;
                                             d->adds[t] = (t < g->num_tracers && tracer_adds_mass) ? tracer_adds_mass[t] : 0; }
  d->stream = (hipStream_t)stream;
  const char *s = getenv("MW_STRICT");
  d->strict = (s && s[0] == '1');
  size_t nzc = (size_t)g->nz * g->nens, nze = (size_t)(g->nz + 1) * g->nens;
  // fused tables (hyc | hytc | hye | hyte | p0c | ihytc | p0e | ihyte | packed rows), then per member: hyc | hytc | p0c | ihytc | packed rows
  d->hy_host.assign(4 * nzc + 4 * nze + 8 * nze + (size_t)g->nens * (4 * (size_t)g->nz + 8 * (size_t)(g->nz + 1)), 0.0);
  auto fail = [&](void) { mw_dycore_destroy(d); return 1; };
  if (hipMalloc(&d->hy_dev, d->hy_host.size() * sizeof(double)) != hipSuccess) { set_error("hipMalloc(hy) failed"); return fail(); }
  fill_params(d);
  if (!d->strides_ok) { set_error("mw_dycore_create: a variable of this block has more than 2^31 - 1 elements (16 GB): too large for one handle"); return fail(); }
  const DyP &p = d->p;
  size_t slab = (size_t)p.V * p.sV * sizeof(double);
  size_t fxb = (size_t)p.V * p.fxV * sizeof(double), fyb = (size_t)p.V * p.fyV * sizeof(double), fzb = (size_t)p.V * p.fzV * sizeof(double);
  if (hipMalloc(&d->S0, slab) != hipSuccess || hipMalloc(&d->S1, slab) != hipSuccess || hipMalloc(&d->S2, slab) != hipSuccess ||
      hipMalloc(&d->S3, slab) != hipSuccess ||
      hipMalloc(&d->tendY, (size_t)5 * p.nC * sizeof(double)) != hipSuccess || hipMalloc(&d->FX, fxb) != hipSuccess ||
      hipMalloc(&d->FY, fyb) != hipSuccess || hipMalloc(&d->FZ, fzb) != hipSuccess ||
      hipMalloc(&d->imm, (size_t)p.nC * sizeof(double)) != hipSuccess || hipMalloc(&d->flags, (size_t)p.nC) != hipSuccess ||
      hipMalloc(&d->dirty, MW_DIRTY_WORDS * sizeof(unsigned int)) != hipSuccess) {
    set_error("hipMalloc(workspace) failed"); return fail(); }
  (void)hipMemsetAsync(d->flags, 0, (size_t)p.nC, d->stream);
  (void)hipMemsetAsync(d->dirty, 0, MW_DIRTY_WORDS * sizeof(unsigned int), d->stream);
  d->fused = (g->num_tracers <= 4 && g->nens <= 12) ? 1 : 0;       // (option "fused_tracers" = 0: the unfused tracer stage)
  // zero everything once: halo corners are never written and the flux arrays start at 0 (:1677-1682)
  (void)hipMemsetAsync(d->S0, 0, slab, d->stream); (void)hipMemsetAsync(d->S1, 0, slab, d->stream);
  (void)hipMemsetAsync(d->S2, 0, slab, d->stream); (void)hipMemsetAsync(d->S3, 0, slab, d->stream); (void)hipMemsetAsync(d->tendY, 0, (size_t)5 * p.nC * sizeof(double), d->stream);
  (void)hipMemsetAsync(d->FX, 0, fxb, d->stream); (void)hipMemsetAsync(d->FY, 0, fyb, d->stream); (void)hipMemsetAsync(d->FZ, 0, fzb, d->stream);
  (void)hipMemsetAsync(d->imm, 0, (size_t)p.nC * sizeof(double), d->stream);
  d->nWE1 = (long long)p.nz * p.ny * p.HX * p.nens;
  d->nSN1 = (long long)p.nz * p.HY * p.nx * p.nens;
  {
    const size_t fn[3] = {(size_t)p.fxV, (size_t)p.fyV, (size_t)p.fzV};
    for (int b = 0; b < 2; b++) for (int a = 0; a < 3; a++) {
      if (hipMalloc(&d->M[b][a], fn[a] * sizeof(double)) != hipSuccess || hipMalloc(&d->UP[b][a], fn[a]) != hipSuccess) { set_error("hipMalloc(M/UP) failed"); return fail(); }
      (void)hipMemsetAsync(d->M[b][a], 0, fn[a] * sizeof(double), d->stream); (void)hipMemsetAsync(d->UP[b][a], 0, fn[a], d->stream);
    }
    { // The tracer stream gets the highest stream priority: its kernels are the older work (stage s while the state stream is
      // already in stage s+1), and with both pipelines fp64-VALU bound an even split of the chip only stretches both (measured on
      // one rank with the two-stream schedule forced: step time -0.5 % against equal priorities).
      int least = 0, greatest = 0; (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      hipError_t er = hipStreamCreateWithPriority(&d->tstream, hipStreamNonBlocking, greatest);
      if (er != hipSuccess) { set_error("hipStreamCreate failed"); return fail(); } }
    for (int i = 0; i < 8; i++) if (hipEventCreateWithFlags(&d->ev_state[i], hipEventDisableTiming) != hipSuccess ||
                                    hipEventCreateWithFlags(&d->ev_tr[i], hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return fail(); }
    if (hipEventCreateWithFlags(&d->ev_misc, hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return fail(); }
    for (int i = 0; i < 7; i++)
      if (hipEventCreateWithFlags(&d->ev_pipe[i], hipEventDisableTiming) != hipSuccess) { set_error("hipEventCreate failed"); return fail(); }
  }
  fill_params(d);
  if (hipStreamSynchronize(d->stream) != hipSuccess) { set_error("stream sync failed in create"); return fail(); }
  *h = d;
  return 0;
}

void mw_dycore_destroy(mw_dycore_t d) {
  if (!d) return;
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  for (double *ptr : {d->S0, d->S1, d->S2, d->S3, d->tendY, d->FX, d->FY, d->FZ, d->hy_dev, d->imm}) if (ptr) (void)hipFree(ptr);
  if (d->flags) (void)hipFree(d->flags);
  if (d->dirty) (void)hipFree(d->dirty);
  zero_rows_free(d);
  if (d->pinc) (void)hipFree(d->pinc);
  for (int b = 0; b < 2; b++) for (int a = 0; a < 3; a++) { if (d->M[b][a]) (void)hipFree(d->M[b][a]); if (d->UP[b][a]) (void)hipFree(d->UP[b][a]); }
  for (int i = 0; i < 8; i++) { if (d->ev_state[i]) (void)hipEventDestroy(d->ev_state[i]); if (d->ev_tr[i]) (void)hipEventDestroy(d->ev_tr[i]); }
  if (d->ev_misc) (void)hipEventDestroy(d->ev_misc);
  for (int i = 0; i < 7; i++) if (d->ev_pipe[i]) (void)hipEventDestroy(d->ev_pipe[i]);
  if (d->tstream) (void)hipStreamDestroy(d->tstream);
  if (d->xchg_free && d->xchg_ctx) d->xchg_free(d->xchg_ctx);
  for (int g = 0; g < 2; g++) for (int b = 0; b < 8; b++) if (d->bufs[g][b]) (void)hipFree(d->bufs[g][b]);
  for (int w = 0; w < 12; w++) for (auto &pr : d->ev[w]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  delete d;
}

int mw_dycore_get_grid(mw_dycore_t d, mw_grid_t *g) { if (!d || !g) MW_FAIL("null argument"); *g = d->g; return 0; }
double mw_dycore_get_etime(mw_dycore_t d) { return d ? d->etime : -1.0; }
double *mw_dycore_immersed_proportion(mw_dycore_t d) { return d ? d->imm : nullptr; }

int mw_dycore_set_bc(mw_dycore_t d, int bc_x, int bc_y, int bc_z) {
  if (!d) MW_FAIL("null handle");
  for (int b : {bc_x, bc_y, bc_z}) if (b != MW_BC_PERIODIC && b != MW_BC_OPEN && b != MW_BC_WALL) MW_FAIL("bc_x / bc_y / bc_z must be 0 (periodic), 1 (open) or 2 (wall)");
  const int old[3] = {d->g.bc_x, d->g.bc_y, d->g.bc_z};
  d->g.bc_x = bc_x; d->g.bc_y = bc_y; d->g.bc_z = bc_z;
  fill_params(d);
  if (check_halo_fit(d)) { d->g.bc_x = old[0]; d->g.bc_y = old[1]; d->g.bc_z = old[2]; fill_params(d); return 1; }
  return 0;
}
int mw_dycore_set_strict(mw_dycore_t d, int strict) { if (!d) MW_FAIL("null handle"); d->strict = strict; return 0; }

// ---- run-time options (see DyOpts) ------------------------------------------------------------------------------------
namespace {
struct OptDesc { const char *key; int DyOpts::*field; long long lo, hi; int build; };   // build: 0 = every build has it (the experiment builds of rounds 4-5 left the tree in round 6)
const OptDesc OPTS[] = {
  {"overlap", &DyOpts::overlap, -1, 1, 0}, {"pipe", &DyOpts::pipe, 0, 1, 0}, {"pipe_edge_inline", &DyOpts::pipe_edge_inline, 0, 1, 0},
  {"pipe_convert", &DyOpts::pipe_convert, 0, 1, 0}, {"pipe_split_edges", &DyOpts::pipe_split_edges, 0, 1, 0}, {"spec", &DyOpts::spec, 0, 1, 0}, {"wrap", &DyOpts::wrap, 0, 1, 0},
  {"y_all", &DyOpts::y_all, 0, 1, 0}, {"y_all_conv", &DyOpts::y_all_conv, 0, 1, 0}, {"member_major", &DyOpts::member_major, 0, 1, 0},
  {"mm_direct", &DyOpts::mm_direct, 0, 1, 0}, {"mm_conv", &DyOpts::mm_conv, 0, 1, 0}, {"fused_convert", &DyOpts::fused_convert, 0, 1, 0},
  {"fused_convert_mm", &DyOpts::fused_convert_mm, 0, 1, 0}, {"chunk_y", &DyOpts::chunk_y, 0, 1 << 20, 0}, {"chunk_yt", &DyOpts::chunk_yt, 0, 1 << 20, 0},
  {"chunk_z", &DyOpts::chunk_z, 0, 1 << 20, 0}, {"chunk_f", &DyOpts::chunk_f, 0, 1 << 20, 0}, {"chunk_model", &DyOpts::chunk_model, 0, 1, 0},
  {"tf_rows4", &DyOpts::tf_rows4, 0, 1, 0}, {"zero_skip", &DyOpts::zero_skip, 0, 1, 0}, {"zero_rows", &DyOpts::zero_rows, 0, 1, 0}, {"zero_stores", &DyOpts::zero_stores, 0, 1, 0}, {"zero_verify", &DyOpts::zero_verify, 0, 1, 0}, {"pipe_maps_early", &DyOpts::pipe_maps_early, 0, 1, 0}, {"rccl_lanes", &DyOpts::rccl_lanes, 0, 2, 0}, {"rccl_two_comms", &DyOpts::rccl_two_comms, -1, 1, 0},
  {"xchg_fuzz", &DyOpts::xchg_fuzz, 0, 0x7fffffff, 0}, {"rccl_prio", &DyOpts::rccl_prio, 0, 1, 0}, {"rccl_inline", &DyOpts::rccl_inline, 0, 1, 0},
  {"debug_no_patch", &DyOpts::debug_no_patch, 0, 1, 0},
};
// (round 7's two keys, beside the table like "fused_tracers": tests/test_capi_host.py ties every table entry to the DEFAULTS of
//  tests/test_gpu_options.py; the defaults of these two are under test in tests/test_gpu_vapour_state.py)
struct OptDesc2 { const char *key; int DyOpts::*field; };
const OptDesc2 OPTS_VAPOUR[] = {{"vapour_state", &DyOpts::vapour_state}, {"debug_vapour_redo", &DyOpts::debug_vapour_redo}};
// (round 9's key, in a table of its own for the same reason; its default is under test in tests/test_gpu_lean_stores.py)
const OptDesc2 OPTS_LEAN[] = {{"lean_stores", &DyOpts::lean_stores}};
constexpr int BUILD_FLAGS = 0;      // (no optional parts any more: mw_build_flags stays in the ABI and says so)
}
int mw_build_flags(void) { return BUILD_FLAGS; }
int mw_dycore_set_option(mw_dycore_t d, const char *key, long long value) {
  if (!d || !key) MW_FAIL("mw_dycore_set_option: null argument");
  if (!strcmp(key, "fused_tracers")) {                          // (0: the unfused tracer stage k_xz_tracers + k_tracer_update)
    if (value != 0 && value != 1) MW_FAIL("option fused_tracers must be 0 or 1");
    if (value && !(d->g.num_tracers <= 4 && d->g.nens <= 12)) MW_FAIL("option fused_tracers = 1 needs at most 4 tracers and 12 members");
    d->fused = (int)value;
    return 0;
  }
  for (const OptDesc2 *od : {&OPTS_VAPOUR[0], &OPTS_VAPOUR[1], &OPTS_LEAN[0]}) {
    if (strcmp(key, od->key)) continue;
    if (value != 0 && value != 1) MW_FAIL(std::string("option ") + key + " must be 0 or 1");
    d->o.*(od->field) = (int)value;
    return 0;
  }
  for (const OptDesc &od : OPTS) {
    if (strcmp(key, od.key)) continue;
    if (value < od.lo || value > od.hi) MW_FAIL(std::string("option ") + key + ": value out of range [" + std::to_string(od.lo) + ", " + std::to_string(od.hi) + "]");
    d->o.*(od.field) = (int)value;
    if (!strncmp(key, "chunk_", 6)) d->chunk_y = d->chunk_yt = d->chunk_z = d->chunk_f = 0;      // (cached chunk sizes: decided again at the next launch)
    return 0;
  }
  MW_FAIL(std::string("unknown option: ") + key);
}
int mw_dycore_get_option(mw_dycore_t d, const char *key, long long *value) {
  if (!d || !key || !value) MW_FAIL("mw_dycore_get_option: null argument");
  if (!strcmp(key, "fused_tracers")) { *value = d->fused; return 0; }
  for (const OptDesc2 &od : OPTS_VAPOUR) if (!strcmp(key, od.key)) { *value = d->o.*(od.field); return 0; }
  for (const OptDesc2 &od : OPTS_LEAN) if (!strcmp(key, od.key)) { *value = d->o.*(od.field); return 0; }
  for (const OptDesc &od : OPTS) if (!strcmp(key, od.key)) { *value = d->o.*(od.field); return 0; }
  MW_FAIL(std::string("unknown option: ") + key);
}
int mw_dycore_set_order(mw_dycore_t d, int ord) {
  if (!d) MW_FAIL("null handle");
  if (ord != 3 && ord != 5 && ord != 7 && ord != 9) MW_FAIL("WENO order must be 3, 5, 7 or 9");
  // orders 7 and 9 reach further: x / y halo hs + 1 (the neighbour's edge value is rebuilt locally), z halo hs
  const int hs = (ord - 1) / 2, hx = std::max(HXc, hs + 1), hz = std::max(HZc, hs);
  const int old_ord = d->ord, old_hx = d->hxw, old_hz = d->hzw;
  auto rollback = [&]() { d->ord = old_ord; d->hxw = old_hx; d->hzw = old_hz; fill_params(d); return 1; };
  d->ord = ord; d->hxw = hx; d->hzw = hz;
  fill_params(d);
  if (!d->strides_ok) { set_error("mw_dycore_set_order: with this order's halo a variable of the block has more than 2^31 - 1 elements"); return rollback(); }
  if (check_halo_fit(d)) return rollback();
  if (hx != old_hx || hz != old_hz) {
    MW_HIP(hipStreamSynchronize(d->stream));
    if (d->tstream) MW_HIP(hipStreamSynchronize(d->tstream));
    // the four slabs in their new size first; the handle only changes once all of them exist
    const size_t slab = (size_t)d->p.V * d->p.sV * sizeof(double);
    double *fresh[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; i++) {
      if (hipMalloc(&fresh[i], slab) != hipSuccess || hipMemsetAsync(fresh[i], 0, slab, d->stream) != hipSuccess) {   // halo corners are never written (as in create)
        for (int j = 0; j <= i; j++) if (fresh[j]) (void)hipFree(fresh[j]);
        set_error("mw_dycore_set_order: hipMalloc of the wider slabs failed (the handle keeps its previous order)");
        return rollback();
      }
    }
    zero_rows_invalidate(d); zero_rows_forget(d, nullptr);     // (the slabs are replaced)
    double **S[4] = {&d->S0, &d->S1, &d->S2, &d->S3};
    for (int i = 0; i < 4; i++) { if (*S[i]) (void)hipFree(*S[i]); *S[i] = fresh[i]; }
    d->flux_src = nullptr;                                      // pointed into a slab that no longer exists
    d->chunk_y = d->chunk_yt = d->chunk_z = d->chunk_f = 0;
    d->nWE1 = (long long)d->p.nz * d->p.ny * d->p.HX * d->p.nens;
    d->nSN1 = (long long)d->p.nz * d->p.HY * d->p.nx * d->p.nens;
    bool had = false;
    for (int g = 0; g < 2; g++) for (int b = 0; b < 8; b++) if (d->bufs[g][b]) { (void)hipFree(d->bufs[g][b]); d->bufs[g][b] = nullptr; had = true; }
    if (had) {                                                  // strips are HX / HY cells deep: re-allocate (the transport and its owner stay)
      auto owner = d->xchg_free; auto fn = d->xchg; void *ctx = d->xchg_ctx;
      d->xchg_free = nullptr;                                   // (set_exchange must not free the context it is about to re-install)
      if (mw_dycore_set_exchange(d, fn, ctx)) { d->xchg_free = owner; d->xchg = fn; d->xchg_ctx = ctx; return 1; }
      d->xchg_free = owner;
    }
    MW_HIP(hipStreamSynchronize(d->stream));
  }
  return 0;
}

int mw_dycore_set_background(mw_dycore_t d, const double *hyc, const double *hytc, const double *hye, const double *hyte,
                             const double *immersed_proportion) {
  if (!d || !hyc || !hytc || !hye || !hyte) MW_FAIL("null argument");
  size_t nzc = (size_t)d->g.nz * d->g.nens, nze = (size_t)(d->g.nz + 1) * d->g.nens;
  memcpy(d->hy_host.data(), hyc, nzc * 8); memcpy(d->hy_host.data() + nzc, hytc, nzc * 8);
  memcpy(d->hy_host.data() + 2 * nzc, hye, nze * 8); memcpy(d->hy_host.data() + 2 * nzc + nze, hyte, nze * 8);
  if (upload_background(d)) return 1;
  if (immersed_proportion) MW_HIP(hipMemcpyAsync(d->imm, immersed_proportion, (size_t)d->p.nC * 8, hipMemcpyDeviceToDevice, d->stream));
  else MW_HIP(hipMemsetAsync(d->imm, 0, (size_t)d->p.nC * 8, d->stream));
  return 0;
}

int mw_dycore_get_background(mw_dycore_t d, double *hyc, double *hytc, double *hye, double *hyte) {
  if (!d) MW_FAIL("null handle");
  size_t nzc = (size_t)d->g.nz * d->g.nens, nze = (size_t)(d->g.nz + 1) * d->g.nens;
  if (hyc) memcpy(hyc, d->hy_host.data(), nzc * 8);
  if (hytc) memcpy(hytc, d->hy_host.data() + nzc, nzc * 8);
  if (hye) memcpy(hye, d->hy_host.data() + 2 * nzc, nze * 8);
  if (hyte) memcpy(hyte, d->hy_host.data() + 2 * nzc + nze, nze * 8);
  return 0;
}

int mw_dycore_get_fluxes(mw_dycore_t d, double **out6) {
  if (!d || !out6) MW_FAIL("null argument");
  if (d->flux_src) {     // production path: the state-variable fluxes of the last stage were never written; rebuild all six
    if (d->member_major) {   // the retained stage input is member-major: bring it into the fused layout the general kernels read (S1 is free)
      const long long n = (long long)d->p.V * d->p.sV;
      zero_rows_invalidate(d);                                  // (S1 is written without maps)
      MW_KLAUNCH(k_member_to_fused, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d->stream, d->p, d->flux_src, d->S1);
      MW_LAUNCH_CHECK();
      d->flux_src = d->S1;
    }
    { // the marching kernels apply the z boundary rule (and, in a periodic direction owned by one rank, the wrap) while
      // loading and leave those halos of the slab unfilled: fill them for k_flux
      DyP p = d->p; p.v0 = 0;
      double *S = const_cast<double *>(d->flux_src);
      const long long nx_ = (long long)p.V * p.nz * p.ny * 2 * p.HX * p.nens, ny_ = (long long)p.V * p.nz * 2 * p.HY * p.nx * p.nens;
      const long long nz_ = (long long)p.V * 2 * p.HZ * p.ny * p.nx * p.nens;
      const unsigned nbx = p.wrap_x ? (unsigned)((nx_ + 255) / 256) : 0u, nby = p.wrap_y ? (unsigned)((ny_ + 255) / 256) : 0u;
      MW_KLAUNCH(k_halo_xyz, dim3(nbx + nby + (unsigned)((nz_ + 255) / 256)), dim3(256), 0, d->stream, p, S, nbx, nby);
      MW_LAUNCH_CHECK(); }
    if (launch_flux(d, d->flux_src)) return 1;              // arrays from the retained stage input exactly as D9+D10 leave them
    if (launch_fct(d, d->flux_src, d->flux_dt)) return 1;
    d->flux_src = nullptr;
  }
  out6[0] = d->FX; out6[1] = d->FY; out6[2] = d->FZ;
  out6[3] = d->FX + 5 * d->p.fxV; out6[4] = d->FY + 5 * d->p.fyV; out6[5] = d->FZ + 5 * d->p.fzV;
  return 0;
}

int mw_dycore_set_exchange(mw_dycore_t d, mw_exchange_fn fn, void *ctx) {
  if (!d) MW_FAIL("null handle");
  if (d->xchg_free && d->xchg_ctx && d->xchg_ctx != ctx) {     // a transport the handle owned is being replaced
    (void)hipStreamSynchronize(d->stream); if (d->tstream) (void)hipStreamSynchronize(d->tstream);
    d->xchg_free(d->xchg_ctx);
  }
  d->xchg_free = nullptr;
  d->xchg = nullptr; d->xchg_ctx = nullptr;                    // committed below, once the strip buffers exist: a failed allocation
  if (fn) {                                                    // must not leave a transport (and a context its owner then frees) behind
    for (int g = 0; g < 2; g++) for (int b = 0; b < 8; b++) {
      if (d->bufs[g][b]) continue;
      long long n = ((b % 4 < 2) ? d->nWE1 : d->nSN1) * d->p.V;          // sized for all V variables
      if (n == 0) n = 1;
      MW_HIP(hipMalloc(&d->bufs[g][b], (size_t)n * sizeof(double)));
    }
  }
  d->xchg = fn; d->xchg_ctx = ctx;
  return 0;
}

int mw_dycore_profile(mw_dycore_t d, int enable) {
  if (!d) MW_FAIL("null handle");
  MW_HIP(hipStreamSynchronize(d->stream));
  d->prof = enable;
  for (int w = 0; w < 12; w++) d->ev_used[w] = 0;
  return 0;
}
int mw_dycore_profile_get(mw_dycore_t d, int which, double *total_ms, long long *launches) {
  if (!d || which < 0 || which > 11) MW_FAIL("bad argument");
  MW_HIP(hipStreamSynchronize(d->stream));
  double tot = 0;
  for (size_t i = 0; i < d->ev_used[which]; i++) { float ms = 0; MW_HIP(hipEventElapsedTime(&ms, d->ev[which][i].first, d->ev[which][i].second)); tot += ms; }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (long long)d->ev_used[which];
  return 0;
}

// ---- parked column increments (round 6) ---------------------------------------------------------------------------------------------
// ColumnNudger::nudge_to_column is two passes over five fields: the horizontal sums, and `state += dt (column - avg) / 900` (1.3 GB read and
// written again on config 2, 0.25 ms of a 5.4 ms loop iteration).  The second pass adds ONE number per (field, level) -- and the next thing the
// reference's loop does with those five arrays is dycore.time_step, whose conversion D1 reads them once and whose D13 overwrites them.  The
// deferred form parks the increments in the dycore handle instead; the next mw_dycore_time_step adds them while its converting y launch
// loads the coupler's values (the same rounded addition, so the result is bit for bit the eager one's) and the pass disappears.  Anybody who
// wants to SEE the fields in between calls mw_dycore_flush_pending first (the Coupler mirrors do that inside DataManager::get); a time step
// on a path whose conversion does not take increments along (strict / general kernels, decomposed blocks, members, 2-D) flushes by itself.
static int flush_pending(mw_dycore_s *d) {
  if (!d->pinc_on) return 0;
  const DyP &p = d->p;
  Ptr5 fp; for (int l = 0; l < 5; l++) fp.f[l] = d->pinc_fields[l];
  const long long ncell_lev = (long long)p.ny * p.nx;
  const unsigned nb = (unsigned)std::min<long long>((ncell_lev * p.nens + 256ll * 8 - 1) / (256ll * 8), 65535);
  MW_KLAUNCH(k_apply_pending, dim3(nb, (unsigned)p.nz, 5u), dim3(256), 0, d->stream, fp, p.nz, ncell_lev, p.nens, d->pinc);
  MW_LAUNCH_CHECK();
  d->pinc_on = false; d->pinc_eager++;
  return 0;
}
int mw_dycore_flush_pending(mw_dycore_t d) {
  if (!d) MW_FAIL("null handle");
  if (!d->pinc_on) return 0;                                    // (the Coupler mirrors call this in front of every field access: nothing parked = nothing done)
  fill_params(d);
  return flush_pending(d);
}
/* 1: increments are parked; out2 (may be NULL): how often parked increments rode on a conversion / were applied by a pass, since create */
int mw_dycore_pending(mw_dycore_t d, unsigned long long *out2) {
  if (!d) return 0;
  if (out2) { out2[0] = d->pinc_lazy; out2[1] = d->pinc_eager; }
  return d->pinc_on ? 1 : 0;
}
int mw_nudge_to_column_deferred(mw_dycore_t d, double *const *state5, const double *column, double dt, void *workspace, mw_allreduce_fn allreduce,
                                void *ctx) {
  if (!d || !state5 || !column || !workspace) MW_FAIL("nudge_to_column_deferred: null argument");
  for (int l = 0; l < 5; l++) if (!state5[l]) MW_FAIL("nudge_to_column_deferred: null field");
  fill_params(d);
  if (flush_pending(d)) return 1;                              // (increments of an earlier call that no time step has consumed: they count in the averages)
  const DyP &p = d->p;
  const long long n = 5ll * p.nz * p.nens;
  if (!d->pinc) MW_HIP(hipMalloc(&d->pinc, (size_t)n * sizeof(double)));
  double *avg = (double *)workspace, *rest = avg + n;
  if (mw_column_average(&d->g, state5, avg, rest, allreduce, ctx, d->stream)) return 1;      // (ordered on the handle's stream, like the time step that will use them)
  MW_KLAUNCH(k_nudge_increments, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d->stream, column, avg, dt, n, d->pinc);
  MW_LAUNCH_CHECK();
  for (int l = 0; l < 5; l++) d->pinc_fields[l] = state5[l];
  d->pinc_on = true;
  return 0;
}

// ---- time_step (:81-198) -------------------------------------------------------------------------------
int mw_dycore_time_step(mw_dycore_t d, double *rho_d, double *u, double *v, double *w, double *temp, double *const *tracers,
                        double dt_phys) {
  if (!d) MW_FAIL("null handle");
  if (!(dt_phys > 0)) MW_FAIL("dt_phys must be > 0");
  CouplerPtrs c;
  if (make_coupler_ptrs(d, rho_d, u, v, w, temp, tracers, c)) return 1;
  fill_params(d);
  const DyP &p = d->p;
  if (need_exchange(d) || check_halo_fit(d)) return 1;
  ProfScope step_scope(d, 9);                                   // (mw_dycore_profile(h, 3): the whole time step, first launch to the join on the handle's stream)
  dim3 cgrid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz);
  // production path; strict = 1/2 use the general flux-materialising kernels below.  So does a z-PERIODIC domain (:752-763,
  // :1008-1019; no shipped case): the marching kernels apply the wall / open z rule while loading and have no periodic form.
  // WENO-3 (the reference's GPU-benchmark build, -DMW_ORD=3) marches too, in the forms that exist for it: fused tracer stage, and
  // nens == 1 or the member-major layout.  Orders 7 / 9 run on the general kernels.
  const bool ord3_ok = d->fused && (p.nens == 1 || d->o.member_major);
  const bool march = (d->strict == 0) && (p.bc_z != MW_BC_PERIODIC) && (d->ord == 5 || (d->ord == 3 && ord3_ok));
  d->last_march = march ? 1 : 0;
  if (march && d->o.wrap) {                       // index wrap instead of halo cells (see DyP::wrap_x)
    d->p.wrap_x = (p.bc_x == MW_BC_PERIODIC) && !(d->xchg && p.nproc_x > 1) && p.nx >= 3;
    d->p.wrap_y = !p.sim2d && (p.bc_y == MW_BC_PERIODIC) && !(d->xchg && p.nproc_y > 1) && p.ny >= 3;
  }
  // Two-stream schedule (see rk_stage_march): the default when strips are exchanged with neighbour ranks (the exchange of one
  // pipeline then runs beside the kernels of the other).  On one rank both pipelines are fp64-VALU bound, the step takes the
  // same time either way (measured without any timing events: +-0.3 %) and sharing the chip only stretches every kernel, so the
  // default there is the handle's stream for everything.  Option "overlap" = 1 / 0 forces either schedule.
  { const bool ov = d->o.overlap >= 0;                          // forced either way
    const bool want = ov ? (d->o.overlap != 0) : (d->xchg != nullptr);
    d->overlap = march && d->tstream && want;
    // ... unless k_y_all applies: then the pipelined one-stream schedule (rk_stage_pipe) is the default with an exchange
    d->pipe = 0;
    if (d->overlap && d->xchg && !ov && d->o.pipe) {
      d->overlap = 0;
      if (y_all_ok(d) && d->ev_pipe[0]) d->pipe = 1; else d->overlap = 1;
    } }
  // nens > 1 on the production path: member-major internal layout (see View)
  // (Measured, round 3, config 4's block 256 x 512 x 128 x 4: the members' coupler-touching launches -- D1 inside k_y_state, D13 inside the
  //  last stage -- issued SIDE BY SIDE on one stream per member, hoping that the quarter lines the four members read / write would
  //  meet in L2: they do not.  27.3 ms per step with the two coalesced conversion passes; 33.2 with D13 inside the member launches
  //  (k_tracers_fused 7.6 -> 12.0 ms, k_xz_state 9.4 -> 11.7), 30.3 with D1 inside (k_y_state 3.8 -> 7.7), 34.3 with both.)
  d->member_major = march && d->fused && p.nens > 1 && d->o.member_major;
  // ... with D13 written by the last stage's kernels themselves and D1 read by the first k_y_state, the members of a tile in one
  // workgroup so that their quarter-sector accesses meet in L1 / L2 (MemberOff, mw_march.h): 2 or 4 members
  d->mm_direct = d->member_major && (p.nens == 2 || p.nens == 4) && d->o.mm_direct;
  // D1 + D2 (:101, :248-255).  Production path with periodic x and y owned by this rank (either schedule: the tracer stream waits
  // for the stage's state kernels anyway): done inside the first k_y_state (no separate pass); otherwise a conversion kernel first
  // (the reference's operation order on the general path).
  d->conv_pending = march && d->p.wrap_x && d->p.wrap_y && p.nt <= 4 && d->o.fused_convert &&
                    (!d->member_major || d->o.fused_convert_mm);
  // Pipelined schedule of a decomposed block (rk_stage_pipe): only the strips that are packed for the neighbours and the rows the
  // edge-strip y launch reads are converted up front; the inner rows are converted by the first k_y_all<true> while the strips travel.
  const bool pipe_conv = d->pipe && (!d->member_major || (d->mm_direct && d->o.mm_conv && marching_config(d, view(d, 0).p) != 0)) && p.nt <= 3 &&
                         d->o.fused_convert && d->o.pipe_convert && (d->p.wrap_y || p.ny >= 4 * MW_Y_EDGE);
  // (the pipelined schedule converts inside k_y_all<true> ONLY in the forms pipe_conv names: any other handle -- e.g. three members, or a
  //  member-major handle whose configuration is not a folded one -- gets the full conversion pass below; without this a 1 x 1
  //  decomposition with a transport installed (both wraps on) reached the members-in-one-workgroup launch with the wrong kernel)
  if (d->pipe) d->conv_pending = false;
  { // the dispatcher's decisions of this time step, for the tests' path-coverage matrix (mw_dycore_path)
    const int K = march ? marching_config(d, view(d, 0).p) : 0;
    d->path = std::string(march ? "march" : (d->strict == 1 ? "general-strict" : "general-fast")) + " ord" + std::to_string(d->ord);
    if (march) {
      d->path += " K" + std::to_string(K);
      d->path += p.nens == 1 ? " nens1" : d->mm_direct ? " mm_direct" : d->member_major ? " member_major" : " fused_members";
      d->path += d->pipe ? " pipe" : d->overlap ? " two_stream" : " one_stream";
      d->path += y_all_ok(d) ? " y_all" : " y_split";
      d->path += pipe_conv ? " conv_pipe" : d->conv_pending ? " conv_in_y" : " conv_pass";
      d->path += d->fused ? " tracers_fused" : " tracers_unfused";
      d->path += p.sim2d ? " 2d" : " 3d";
    } else d->path += p.nens == 1 ? " nens1" : " fused_members";
    if (d->xchg) d->path += " transport"; }
  if (d->pinc_on) {
    // parked column increments: they ride on the conversion where it happens inside k_y_all<true, K = 1> of a one-rank handle, and belong to
    // exactly the arrays this call was handed; anything else applies them with a pass first
    const bool same = c.rho_d == d->pinc_fields[0] && c.u == d->pinc_fields[1] && c.v == d->pinc_fields[2] && c.temp == d->pinc_fields[3] &&
                      p.idWV >= 0 && p.idWV < p.nt && c.tr[p.idWV] == d->pinc_fields[4];
    const bool lazy = same && march && d->conv_pending && !d->pipe && !d->overlap && !d->member_major && p.nens == 1 && marching_config(d, d->p) == 1 &&
                      y_all_ok(d) && d->o.y_all_conv;
    if (lazy) { d->p.pinc = d->pinc; d->pinc_on = false; d->pinc_lazy++; }
    else if (flush_pending(d)) return 1;
  }
  if (d->vap_used) { MW_HIP(hipMemsetAsync(d->dirty + MW_VREDO_RING + 8, 0, sizeof(unsigned int), d->stream)); d->vap_used = false; }   // the redo counter counts the stages of one time step
  d->pre_lo = d->pre_hi = 0;
  d->entry_marked = false;
  if (pipe_conv && d->ev_pipe[6]) { MW_HIP(hipEventRecord(d->ev_pipe[6], d->stream)); d->entry_marked = true; }   // the coupler's arrays are ready here (see rk_stage_pipe: the row scan runs beside the strip conversion)
  if (pipe_conv) {
    ProfScope ps(d, 4);
    const int ylo = d->p.wrap_y ? 0 : MW_Y_EDGE + 3, yhi = d->p.wrap_y ? p.ny : p.ny - MW_Y_EDGE - 3;
    d->pre_lo = ylo; d->pre_hi = yhi;
    if (launch_coupler_to_slab(d, c, ylo, yhi, true)) return 1;   // the strip cells only (see k_coupler_to_state_fast)
    d->conv_pending = true;
  }
  if (!d->conv_pending) {
    ProfScope ps(d, 4);
    if (d->member_major || (march && p.nt <= 4)) { if (launch_coupler_to_slab(d, c, p.ny, p.ny, false)) return 1; }
    else { MW_KLAUNCH(k_coupler_to_state, cgrid, dim3(256), 0, d->stream, p, c, d->S0); MW_LAUNCH_CHECK(); }
  }
  if (d->overlap) { MW_HIP(hipEventRecord(d->ev_misc, d->stream)); MW_HIP(hipStreamWaitEvent(d->tstream, d->ev_misc, 0)); d->gstage = 0; }
  double dt_dyn = mw_dycore_compute_time_step(&d->g);                     // :104
  int ncycles = (int)std::ceil(dt_phys / dt_dyn);                         // :107
  dt_dyn = dt_phys / ncycles;                                             // :108
  for (int icycle = 0; icycle < ncycles; icycle++) {
    bool last = (icycle == ncycles - 1);
    d->first_cycle = (icycle == 0);
    if (march) {
      double *Q[4] = {d->S0, d->S1, d->S2, d->S3};
      if (rk_cycle_march(d, Q, dt_dyn, last, c)) return 1;
      std::swap(d->S0, d->S3);                                // (P,A,B,C) -> (C,A,B,P): the new q^n is C
      continue;
    }
    // stage 1 (:119-132)
    zero_rows_invalidate(d); zero_rows_forget(d, nullptr);     // (the general path writes the slabs without maps)
    if (halo_fill(d, d->S0)) return 1;
    if (launch_flux(d, d->S0)) return 1;
    if (launch_fct(d, d->S0, dt_dyn)) return 1;
    if (launch_update<1, 0>(d, d->S0, d->S0, d->S1, dt_dyn, dt_dyn, c, nullptr, nullptr)) return 1;
    // stage 2 (:136-153)
    double dt2 = (1.0 / 4.0) * dt_dyn;
    if (halo_fill(d, d->S1)) return 1;
    if (launch_flux(d, d->S1)) return 1;
    if (launch_fct(d, d->S1, dt2)) return 1;
    if (launch_update<2, 0>(d, d->S1, d->S0, d->S1, dt2, dt_dyn, c, nullptr, nullptr)) return 1;
    // stage 3 (:157-174)
    double dt3 = (2.0 / 3.0) * dt_dyn;
    if (halo_fill(d, d->S1)) return 1;
    if (launch_flux(d, d->S1)) return 1;
    if (launch_fct(d, d->S1, dt3)) return 1;
    if (last) { if (launch_update<3, 1>(d, d->S1, d->S0, d->S0, dt3, dt_dyn, c, nullptr, nullptr)) return 1; }     // + :178
    else      { if (launch_update<3, 0>(d, d->S1, d->S0, d->S0, dt3, dt_dyn, c, nullptr, nullptr)) return 1; }
    d->flux_src = nullptr;                                    // all six flux arrays are already materialised
  }
  if (d->overlap) MW_HIP(hipStreamWaitEvent(d->stream, d->ev_tr[(d->gstage - 1) & 7], 0));   // join: the handle's stream owns the result
  d->etime += dt_phys;                                                    // :181
  return 0;
}

int mw_dycore_compute_tendencies(mw_dycore_t d, const double *rho_d, const double *u, const double *v, const double *w,
                                 const double *temp, double *const *tracers, double dt, double *state_tend, double *tracers_tend) {
  if (!d) MW_FAIL("null handle");
  CouplerPtrs c;
  if (make_coupler_ptrs(d, rho_d, u, v, w, temp, tracers, c)) return 1;
  fill_params(d);
  const DyP &p = d->p;
  if (need_exchange(d) || check_halo_fit(d)) return 1;
  if (flush_pending(d)) return 1;
  dim3 cgrid = plane_grid((long long)p.ny * p.nx * p.nens, p.nz);
  MW_KLAUNCH(k_coupler_to_state, cgrid, dim3(256), 0, d->stream, p, c, d->S0); MW_LAUNCH_CHECK();
  if (halo_fill(d, d->S0)) return 1;
  if (launch_flux(d, d->S0)) return 1;
  if (launch_fct(d, d->S0, dt)) return 1;
  d->flux_src = nullptr;
  if (state_tend && tracers_tend) { if (launch_update<1, 2>(d, d->S0, d->S0, nullptr, dt, dt, c, state_tend, tracers_tend)) return 1; }
  return 0;
}

// Test aid: the names (as the code object spells them, i.e. mangled; newline-separated) of the dycore kernels this PROCESS has launched
// since the last reset -- every instantiation of the dispatcher's templates has its own.  Returns the bytes needed (terminator included);
// writes at most `cap` of them.  reset != 0 clears the registry afterwards.
long long mw_debug_launched_kernels(char *buf, long long cap, int reset) {
  std::string all;
  {
    std::lock_guard<std::mutex> lk(g_launch_mu);
    for (const void *fn : g_launched) {
      const char *n = hipKernelNameRefByPtr(fn, nullptr);
      if (!n) { (void)hipGetLastError(); continue; }
      all += n; all += "\n";
    }
    if (reset) g_launched.clear();
  }
  if (buf && cap > 0) { const size_t m = std::min<size_t>((size_t)cap - 1, all.size()); memcpy(buf, all.data(), m); buf[m] = 0; }
  return (long long)all.size() + 1;
}

} // extern "C"

namespace mw {
int dycore_set_exchange_owned(mw_dycore_t d, mw_exchange_fn fn, void *ctx, void (*free_ctx)(void *)) {
  if (mw_dycore_set_exchange(d, fn, ctx)) return 1;
  d->xchg_free = free_ctx;
  return 0;
}
// the installed transport of a handle (mw_rccl.cpp recognises its own by the callback's address)
int dycore_option(mw_dycore_t d, const char *key) { long long v = 0; return (d && !mw_dycore_get_option(d, key, &v)) ? (int)v : 0; }
void *dycore_exchange_ctx(mw_dycore_t d, mw_exchange_fn *fn) { if (fn) *fn = d ? d->xchg : nullptr; return d ? d->xchg_ctx : nullptr; }
} // namespace mw

// Which schedule the LAST mw_dycore_time_step of this handle chose (decided per call from the transport, the configuration and the
// MW_* switches): 0 = one stream, 1 = two streams (state | tracer pipelines, rk_stage_march with overlap), 2 = the pipelined
// one-stream schedule of a decomposed block (rk_stage_pipe); + 4 when the y faces of all variables go through the one k_y_all launch,
// + 8 when that time step ran on the general (flux-materialising) kernels instead of the marching ones.  -1: null handle.
extern "C" const char *mw_dycore_path(mw_dycore_t d) { return d ? d->path.c_str() : ""; }
extern "C" int mw_dycore_schedule(mw_dycore_t d) {
  if (!d) return -1;
  return (d->pipe ? 2 : d->overlap ? 1 : 0) + (d->last_march && y_all_ok(d) ? 4 : 0) + (d->last_march ? 0 : 8);
}

