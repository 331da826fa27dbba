// =====================================================================================================
// mw_zero_rows.hip -- the zero-row maps: their five kernels, compiled here alone, and their host side -- which handles run with maps, how a
// sub-cycle's maps are built and reach the kernels' parameter block, the two test aids.  (What the maps are: mw_zero_rows.h)
// =====================================================================================================
#include "mw_dycore_int.h"

namespace mw {
// k_zero_rows: wave = one x row (k, j).  SLAB: the tracers of slab S (later sub-cycles of a step, or after a conversion pass); else the
// coupler's arrays.  vmask: the tracers that can vanish -- the others are flagged non-zero without being read.  ldo / offo: layout of
// `out` (compact [k][ny] for k_zero_merge, or the map's own); wrap: also write the row's periodic images into the map's halo rows.
template <bool SLAB>
// (wrap == 2: the halo rows are marked "may be non-zero" instead -- the LOCAL maps of a decomposed block, used by the first stage's y launches
//  before the neighbours' maps have arrived; out2: a second, compact [k][ny] copy for k_zero_merge)
__global__ __launch_bounds__(256) void k_zero_rows(DyP p, CouplerPtrs c, const double *__restrict__ S, unsigned *__restrict__ out, unsigned vmask,
                                                   int ldo, int offo, int wrap, unsigned *__restrict__ out2) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)p.nz * p.ny) return;
  const int k = (int)(row / p.ny), j = (int)(row - (long long)k * p.ny), lane = threadIdx.x & 63;
  const int NXI = p.nx * p.nens;
  // (all tracers' values of eight 64-cell pieces are requested before the first one is tested: the kernel is a latency-bound stream otherwise)
  const double *src[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int vv = min(v, p.nt - 1);
    src[v] = SLAB ? S + (long long)(5 + vv) * p.sV + (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens
                  : c.tr[vv] + ((long long)k * p.ny + j) * NXI;
  }
  const unsigned scan = vmask & ((1u << min(p.nt, 4)) - 1u);
  bool nz[4] = {false, false, false, false};
  unsigned segb = 0;                                              // this lane's part of the segment bits (+ the edge flags)
  const bool xwrap = p.zq_xper != 0;                             // (one rank owns periodic x -- whether the kernels wrap their index or read filled halo cells)
  for (int base = 0; base < NXI; base += 512) {
    double a[4][8];
#pragma unroll
    for (int v = 0; v < 4; v++) {
      if (!((scan >> v) & 1u)) continue;                        // (wave-uniform)
#pragma unroll
      for (int u = 0; u < 8; u++) { const int ie = base + u * 64 + lane; a[v][u] = src[v][min(ie, NXI - 1)]; }
    }
    bool cellnz[8] = {false, false, false, false, false, false, false, false};
#pragma unroll
    for (int v = 0; v < 4; v++) {
      if (!((scan >> v) & 1u)) continue;
#pragma unroll
      for (int u = 0; u < 8; u++) { const bool b = (a[v][u] != 0.0); nz[v] = nz[v] || b; cellnz[u] = cellnz[u] || b; }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      if (!cellnz[u]) continue;
      const int ie = min(base + u * 64 + lane, NXI - 1);
      segb |= zr_seg_mask(ie - MW_ZR_HALO, ie + MW_ZR_HALO, NXI, xwrap);
      if (!xwrap && ie - MW_ZR_HALO < 0) segb |= MW_ZR_TOUCH_W;
      if (!xwrap && ie + MW_ZR_HALO >= NXI) segb |= MW_ZR_TOUCH_E;
    }
  }
  for (int off = 32; off > 0; off >>= 1) segb |= (unsigned)__shfl_xor((int)segb, off, 64);
  unsigned word = ((1u << min(p.nt, 4)) - 1u) & ~vmask;           // the tracers that cannot vanish
#pragma unroll
  for (int v = 0; v < 4; v++) if (((scan >> v) & 1u) && __any(nz[v])) word |= 1u << v;
  word |= segb;                                                  // (with the two edge flags when x is decomposed: k_zero_merge of the neighbours reads them; nobody else looks at bits 30, 31)
  if (lane == 0) {
    unsigned *o = out + (long long)k * ldo + offo;
    o[j] = word;
    if (wrap && j < MW_ZR_HALO) o[p.ny + j] = (wrap == 2) ? ~0u : word;
    if (wrap && j >= p.ny - MW_ZR_HALO) o[j - p.ny] = (wrap == 2) ? ~0u : word;
    if (out2) out2[(long long)k * p.ny + j] = word;
  }
}
// Decomposed block: M = own rows (compact) OR the west / east neighbours' (rW / rE, nullptr: x is not decomposed); the merged rows next
// to the south / north edge are packed for those neighbours (sS / sN, nullptr: y is not decomposed -- the halo rows are then the block's
// own periodic images).
__global__ __launch_bounds__(256) void k_zero_merge(DyP p, const unsigned *__restrict__ own, const unsigned *__restrict__ rW, const unsigned *__restrict__ rE,
                                                    unsigned *__restrict__ M, unsigned *__restrict__ sS, unsigned *__restrict__ sN) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)p.nz * p.ny) return;
  const int k = (int)(t / p.ny), j = (int)(t - (long long)k * p.ny);
  unsigned wd = own[t];
  if (rW) {
    // the neighbours' rows: their row bits as before (coarse, but a superset -- the y kernel's store decision looks at them); of their
    // segments only what can cross the shared edge within a sub-cycle: a grown set that touches the neighbour's edge reaches my first / last 9 cells
    const unsigned w = rW[t], e = rE[t];
    const int NXI = p.nx * p.nens;
    wd |= (w | e) & MW_ZR_ROWBITS;
    if (w & MW_ZR_TOUCH_E) wd |= zr_seg_mask(0, MW_ZR_HALO - 1, NXI, false);
    if (e & MW_ZR_TOUCH_W) wd |= zr_seg_mask(NXI - MW_ZR_HALO, NXI - 1, NXI, false);
  }
  unsigned *o = M + (long long)k * p.zq_ld + MW_ZR_HALO;
  o[j] = wd;
  if (sS) {
    if (j < MW_ZR_HALO) sS[k * MW_ZR_HALO + j] = wd;
    if (j >= p.ny - MW_ZR_HALO) sN[k * MW_ZR_HALO + j - (p.ny - MW_ZR_HALO)] = wd;
  } else {
    if (j < MW_ZR_HALO) o[p.ny + j] = wd;
    if (j >= p.ny - MW_ZR_HALO) o[j - p.ny] = wd;
  }
}
// ... and the rows beyond the y edges from what the south / north neighbours packed (their northernmost / southernmost rows)
__global__ __launch_bounds__(256) void k_zero_halo(DyP p, unsigned *__restrict__ M, const unsigned *__restrict__ rS, const unsigned *__restrict__ rN) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= p.nz * MW_ZR_HALO) return;
  const int k = t / MW_ZR_HALO, h = t - k * MW_ZR_HALO;
  unsigned *o = M + (long long)k * p.zq_ld + MW_ZR_HALO;
  o[h - MW_ZR_HALO] = rS[t];
  o[p.ny + h] = rN[t];
}
// M0 -> Q1, Q2, Q3, FN1..3 and QY1..3 (a set's layout: mw_zero_rows.h), separably through LDS: rows first (three radii), then levels.
// (fn_ones: FNs = "store" everywhere -- the local maps of a decomposed block cannot know what the neighbours make the tracer kernel read)
__global__ __launch_bounds__(256) void k_zero_dilate(DyP p, unsigned *__restrict__ M, long long msz, int fn_ones) {
  constexpr int TK = 16, TJ = 64, R = MW_ZR_HALO, LO = R + MW_ZR_BEFORE + 1, HI = R + MW_ZR_AFTER + 1, EK = TK + LO + HI, EJ = TJ + 2 * R;
  __shared__ unsigned a[EK][EJ];
  __shared__ unsigned b[3][EK][TJ];
  const int k0 = blockIdx.y * TK, j0 = blockIdx.x * TJ, tid = threadIdx.x;
  for (int t = tid; t < EK * EJ; t += 256) {
    const int kk = t / EJ, jj = t - kk * EJ;
    const int k = min(max(k0 + kk - LO, 0), p.nz - 1);
    const int j = j0 + jj - R;                                   // -9 .. ny+8 are rows of the map; beyond (the last tile's overhang): nobody's
    a[kk][jj] = (j < p.ny + R) ? M[(long long)k * p.zq_ld + j + MW_ZR_HALO] : 0u;
  }
  __syncthreads();
  for (int t = tid; t < EK * TJ; t += 256) {
    const int kk = t / TJ, jj = t - kk * TJ, cc = jj + R;
    unsigned o = a[kk][cc];
#pragma unroll
    for (int r = 1; r <= R; r++) {
      o |= a[kk][cc - r] | a[kk][cc + r];
      if (r % MW_ZR_REACH == 0) b[r / MW_ZR_REACH - 1][kk][jj] = o;
    }
  }
  __syncthreads();
  for (int t = tid; t < TK * TJ; t += 256) {
    const int kk = t / TJ, jj = t - kk * TJ, k = k0 + kk, j = j0 + jj;
    if (k >= p.nz || j >= p.ny) continue;
#pragma unroll
    for (int m = 0; m < 3; m++) {
      const int r = MW_ZR_REACH * (m + 1);
      const int ry = MW_ZR_REACH * m;
      unsigned o = 0, fn = 0, qy = 0;
      for (int dd = -r - MW_ZR_BEFORE - 1; dd <= r + MW_ZR_AFTER + 1; dd++) {
        const unsigned v = b[m][kk + LO + dd][jj];
        fn |= v;
        if (dd >= -r - MW_ZR_BEFORE && dd <= r + MW_ZR_AFTER) o |= v;
        if (dd >= -ry && dd <= ry) qy |= v;
      }
      M[(long long)(m + 1) * msz + (long long)k * p.zq_ld + j + MW_ZR_HALO] = o;
      M[(long long)(m + 4) * msz + (long long)k * p.zq_ld + j + MW_ZR_HALO] = fn_ones ? ~0u : fn;
      M[(long long)(m + 7) * msz + (long long)k * p.zq_ld + j + MW_ZR_HALO] = qy;
    }
  }
}

// Test aid (option zero_verify, any build): the CLAIMS the maps make, checked against the data right in front of the launches that rely on
// them.  wave = one x row (k, j) of the block; viol[] counts rows:
//   [0] a tracer that can vanish is non-zero in row (k, j) of the stage's INPUT slab although Qs[k'][j] is clear for one of the iterations
//       k' = k-3 .. k+2 (clamped) of the row's tracer wave that touch level k  (k_tracers_fused would not have loaded it);
//   [1] ... although QYs[k][j'] is clear for one of the rows j' = j-3 .. j+3 whose y-marching iteration touches row j  (k_y_all);
//   [2] a destination row whose store of zeros the tracer kernel is about to SKIP (its storing iteration is lean and the map handed over as
//       "the destination holds zeros already" is clear -- zqp: slab S1 / S2; zqc: the coupler's arrays) is NOT all zero: a non-zero value
//       would be left standing;
//   [3] likewise a row of the slab that the converting y launch is about to skip (zqk).
// dst == nullptr / the map pointers == nullptr: that claim is not made in this launch and not checked.
__global__ __launch_bounds__(256) void k_zero_verify(DyP p, CouplerPtrs c, const double *__restrict__ Sin, const double *__restrict__ Sdst, int dst_coupler,
                                                     const double *__restrict__ Skz, long long msz, unsigned vmask, unsigned long long *__restrict__ viol) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)p.nz * p.ny) return;
  const int k = (int)(row / p.ny), j = (int)(row - (long long)k * p.ny), lane = threadIdx.x & 63;
  const int NXI = p.nx * p.nens;
  const unsigned scan = vmask & ((1u << min(p.nt, 4)) - 1u);
  unsigned in_nz = 0, dst_nz = 0, kz_nz = 0;
  unsigned in_sg = 0, dst_sg = 0, kz_sg = 0;                      // ... and the x segments (exact: no growth) that hold a non-zero cell
  const long long so = (long long)(k + p.HZ) * p.sK + (long long)(j + p.HY) * p.sJ + (long long)p.HX * p.nens;
  const long long ci = ((long long)k * p.ny + j) * NXI;
  for (int v = 0; v < 4; v++) {
    if (!((scan >> v) & 1u)) continue;
    bool a = false, b = false, e = false;
    for (int ie = lane; ie < NXI; ie += 64) {
      const unsigned sg = zr_seg_mask(ie, ie, NXI, false);
      if (Sin && Sin[(long long)(5 + v) * p.sV + so + ie] != 0.0) { a = true; in_sg |= sg; }
      if (Sdst && !dst_coupler && Sdst[(long long)(5 + v) * p.sV + so + ie] != 0.0) { b = true; dst_sg |= sg; }
      if (dst_coupler && c.tr[v][cpl(p, ci + ie)] != 0.0) { b = true; dst_sg |= sg; }
      if (Skz && Skz[(long long)(5 + v) * p.sV + so + ie] != 0.0) { e = true; kz_sg |= sg; }
    }
    if (__any(a)) in_nz |= 1u << v;
    if (__any(b)) dst_nz |= 1u << v;
    if (__any(e)) kz_nz |= 1u << v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    in_sg |= (unsigned)__shfl_xor((int)in_sg, off, 64); dst_sg |= (unsigned)__shfl_xor((int)dst_sg, off, 64); kz_sg |= (unsigned)__shfl_xor((int)kz_sg, off, 64);
  }
  // (a segment's claim is a claim about its cells: checked with the same rules as the row bits, the segment bits beside them)
  in_nz |= in_sg; dst_nz |= dst_sg; kz_nz |= kz_sg;
  if (lane != 0) return;
  const long long ld = p.zq_ld;
  if (p.zq && in_nz) {
    bool bad0 = false, bad1 = false;
    for (int kk = max(k - 3, 0); kk <= min(k + 2, p.nz - 1); kk++) bad0 = bad0 || ((in_nz & ~p.zq[(long long)kk * ld + j + MW_ZR_HALO]) != 0u);
    const unsigned *qy = p.zq + 6 * msz;
    // (the derived maps hold the block's own rows only -- the kernels index them behind wrap_row: rows beyond a decomposed y edge belong to
    //  the neighbour's maps and are not checked here)
    for (int dj = -MW_ZR_REACH; dj <= MW_ZR_REACH; dj++) {
      const int jj = wrap_row(p, j + dj);
      if (jj >= 0 && jj < p.ny) bad1 = bad1 || ((in_nz & ~qy[(long long)k * ld + jj + MW_ZR_HALO]) != 0u);
    }
    if (bad0) atomicAdd(&viol[0], 1ull);
    if (bad1) atomicAdd(&viol[1], 1ull);
  }
  // (the store of level k is skipped by the iteration k + 2 of the row's wave -- word min(k + 2, nz - 1) -- when that iteration is LEAN and
  //  the destination's map is clear; the converting y launch skips row j when the iteration that converts it, j - 3, is lean and zqk is clear)
  if (dst_nz && p.zq) {
    const unsigned *m = dst_coupler ? p.zqc : p.zqp;
    const int kq = min(k + 2, p.nz - 1);
    if (m && (dst_nz & ~p.zq[(long long)kq * ld + j + MW_ZR_HALO] & ~m[(long long)(dst_coupler ? k : kq) * ld + j + MW_ZR_HALO])) atomicAdd(&viol[2], 1ull);
  }
  if (kz_nz && p.zqk && p.zq) {
    const unsigned *qy = p.zq + 6 * msz;
    const int jl = wrap_row(p, j - MW_ZR_REACH);                 // the iteration that converts row j; beyond a decomposed edge: never lean
    if (jl >= 0 && jl < p.ny && (kz_nz & ~qy[(long long)k * ld + jl + MW_ZR_HALO] & ~p.zqk[(long long)k * ld + j + MW_ZR_HALO])) atomicAdd(&viol[3], 1ull);
  }
}
} // namespace mw

// Which handles: nens == 1, fused tracer stage, x and y periodic; one rank on the one-stream schedule, or the blocks of a decomposed domain
// on the pipelined schedule.  The ranks of a decomposed domain exchange maps, so all of them must decide alike: the size test looks at the
// smallest block of the decomposition, not at this rank's.
bool zero_rows_ok(const mw_dycore_s *d) {
  const DyP &p = d->p;
  // (nens > 1: the member-major layout on one rank -- every member has its own maps and the per-member launches read them; the launches
  //  that hold all members of a tile in one workgroup run without)
  if (!(d->o.zero_skip && d->o.zero_rows && d->fused && (p.nens == 1 || (d->member_major && !d->xchg)) && p.nt >= 1 && p.nt <= 4 && !p.sim2d &&
        p.nz >= 2 && p.bc_x == MW_BC_PERIODIC && p.bc_y == MW_BC_PERIODIC)) return false;
  const long long nx_min = d->g.nx_glob / std::max(1, p.nproc_x), ny_min = d->g.ny_glob / std::max(1, p.nproc_y);
  if (ny_min < MW_ZR_HALO || nx_min < 2 * MW_ZR_HALO) return false;   // (a tracer must not cross a whole block in one sub-cycle)
  if (!d->xchg) return !d->overlap && !d->pipe;
  return d->pipe != 0;
}
static bool zr_decomposed(const mw_dycore_s *d) { return d->xchg && (d->p.nproc_x > 1 || d->p.nproc_y > 1); }

// ---- the four pieces of a build.  Every launch, copy and callback call goes to stream `st`.
// 1: decide (ZeroRows::on), make sure the allocations fit this block (message buffers: for a decomposed block, or `msg_always`), turn to the other
// set.  Out of device memory: one rank runs the sub-cycle without maps; with a transport it is an error -- the other ranks are about to exchange maps.
static int zr_begin(mw_dycore_s *d, bool msg_always) {
  ZeroRows &z = d->zr;
  DyP &p = d->p;
  if (!(z.on = zero_rows_ok(d))) return 0;
  p.zq_ld = p.ny + 2 * MW_ZR_HALO;                              // (the map kernels read it; the map pointers: zero_rows_stage)
  const long long msz = (long long)p.nz * p.zq_ld;
  if (!z.maps || z.msz != msz) {
    if (z.maps) { MW_HIP(hipDeviceSynchronize()); (void)hipFree(z.maps); z.maps = nullptr; }
    if (z.msg) { (void)hipFree(z.msg); z.msg = nullptr; }
    z.msz = msz; z.prev_ok = false; z.conv_slab[0] = z.conv_slab[1] = nullptr;
    if (hipMalloc(&z.maps, (size_t)z.member_words() * sizeof(unsigned) * (size_t)p.nens) != hipSuccess) {
      (void)hipGetLastError(); z.maps = nullptr; z.on = false;
      if (d->xchg) MW_FAIL("zero-row maps: out of device memory");
      return 0; }
  }
  const ZeroRows::Msg m = z.slices(p.nz, p.ny);
  if ((msg_always || zr_decomposed(d)) && !z.msg && hipMalloc(&z.msg, (size_t)(3 * m.dWE + 4 * m.dSN) * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError(); MW_FAIL("zero-row maps: out of device memory"); }
  z.cur ^= 1;
  z.prev_use = z.prev_ok && d->o.zero_stores;
  return 0;
}
// 2: M0 of block (or member) q from its input -- the coupler's arrays, or slab S.  out / ldo / offo / wrap / out2: see k_zero_rows
static void zr_scan(const mw_dycore_s *d, const DyP &q, const CouplerPtrs &c, const double *S, bool from_coupler, hipStream_t st, unsigned *out, int ldo, int offo, int wrap, unsigned *out2) {
  const dim3 g((unsigned)(((long long)q.nz * q.ny + 3) / 4));
  const unsigned vmask = zr_vanish_mask(marching_config(d, q));
  if (from_coupler) MW_KLAUNCH(k_zero_rows<false>, g, dim3(256), 0, st, q, c, S, out, vmask, ldo, offo, wrap, out2);
  else              MW_KLAUNCH(k_zero_rows<true>, g, dim3(256), 0, st, q, c, S, out, vmask, ldo, offo, wrap, out2);
}
// 3, a decomposed block: its compact copy to the west / east neighbours, theirs OR-ed into M0 of set `zr`, the merged edge rows to the
// south / north neighbours, theirs into the halo rows
static int zr_exchange_merge(mw_dycore_s *d, unsigned *zr, hipStream_t st) {
  const DyP &p = d->p;
  const bool ex_x = d->xchg && p.nproc_x > 1, ex_y = d->xchg && p.nproc_y > 1;
  const ZeroRows::Msg m = d->zr.slices(p.nz, p.ny);
  if (ex_x && d->xchg(d->xchg_ctx, m.own, m.own, nullptr, nullptr, m.rW, m.rE, nullptr, nullptr, m.dWE, 0, st)) MW_FAIL("zero-row maps: exchange callback failed");
  MW_KLAUNCH(k_zero_merge, dim3((unsigned)(((long long)p.nz * p.ny + 255) / 256)), dim3(256), 0, st, p, (const unsigned *)m.own, ex_x ? (const unsigned *)m.rW : nullptr, (const unsigned *)m.rE, zr,
             ex_y ? (unsigned *)m.sS : nullptr, (unsigned *)m.sN);
  MW_LAUNCH_CHECK();
  if (!ex_y) return 0;
  if (d->xchg(d->xchg_ctx, nullptr, nullptr, m.sS, m.sN, nullptr, nullptr, m.rS, m.rN, 0, m.dSN, st)) MW_FAIL("zero-row maps: exchange callback failed");
  MW_KLAUNCH(k_zero_halo, dim3((unsigned)(((long long)p.nz * MW_ZR_HALO + 255) / 256)), dim3(256), 0, st, p, zr, (const unsigned *)m.rS, (const unsigned *)m.rN);
  MW_LAUNCH_CHECK();
  return 0;
}
// 4: the first sub-cycle's M0 doubles as "which rows of the coupler's tracer arrays are zero" until the last sub-cycle's D13 (map MC); then
// (`fn_ones` >= 0) the nine derived maps of the set
static int zr_finish(mw_dycore_s *d, const DyP &q, unsigned *zr, hipStream_t st, bool to_mc, int fn_ones) {
  if (to_mc) MW_HIP(hipMemcpyAsync(d->zr.mc(), zr, (size_t)d->zr.msz * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  if (fn_ones >= 0) MW_KLAUNCH(k_zero_dilate, dim3((unsigned)((q.ny + 63) / 64), (unsigned)((q.nz + 15) / 16)), dim3(256), 0, st, q, zr, d->zr.msz, fn_ones);
  MW_LAUNCH_CHECK();
  return 0;
}

// ---- what the schedules call: the maps of a sub-cycle from its input, the coupler's arrays while the conversion is still pending or slab S0.
// All at once (one-stream schedule: at the start of the sub-cycle; pipelined schedule without the early maps: behind the strips).  A decomposed
// block scans into the compact copy and gets its M0 from the merge; any other scans straight into the map, periodic images included.
// Member-major handles (the caller runs this behind the first y launch): one set per member, from the member's slab, no MC.
int zero_rows_build(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st, bool first_cycle) {
  if (zr_begin(d, false)) return 1;
  const ZeroRows &z = d->zr;
  if (!z.on) return 0;
  const DyP &p = d->p;
  ProfScope ps(d, 4, st);
  if (d->member_major) {
    for (int e = 0; e < n_views(d); e++) {
      const View v = view(d, e);
      zr_scan(d, v.p, c, v.S(S0), false, st, z.set(z.cur, e), p.zq_ld, MW_ZR_HALO, 1, nullptr);
      if (zr_finish(d, v.p, z.set(z.cur, e), st, false, 0)) return 1;
    }
    return 0;
  }
  const bool dec = zr_decomposed(d);
  zr_scan(d, p, c, S0, from_coupler, st, dec ? (unsigned *)z.msg : z.set(z.cur), dec ? p.ny : p.zq_ld, dec ? 0 : MW_ZR_HALO, dec ? 0 : 1, nullptr);
  MW_LAUNCH_CHECK();
  if (dec && zr_exchange_merge(d, z.set(z.cur), st)) return 1;
  return zr_finish(d, p, z.set(z.cur), st, first_cycle, 0);
}
// The same in two halves for the first stage of the pipelined schedule (round 5, profiles/r05_selfloop_timeline_maps.txt).  LOCAL maps in front
// of the stage's y launches -- the y kernel reads no x halo, its inner rows only the block's own rows; the rows beyond a decomposed y edge
// count as "may be non-zero", and FNs as "store" --, scanned straight into the map with the compact copy for the merge beside it ...
int zero_rows_local(mw_dycore_s *d, const double *S0, const CouplerPtrs &c, bool from_coupler, hipStream_t st) {
  if (zr_begin(d, true)) return 1;
  const ZeroRows &z = d->zr;
  if (!z.on) return 0;
  const DyP &p = d->p;
  ProfScope ps(d, 4, st);
  zr_scan(d, p, c, S0, from_coupler, st, z.set(z.cur), p.zq_ld, MW_ZR_HALO, (d->xchg && p.nproc_y > 1) ? 2 : 1, (unsigned *)z.msg);
  return zr_finish(d, p, z.set(z.cur), st, false, zr_decomposed(d) ? 1 : 0);
}
// ... and the neighbours' maps merged in on the exchange stream, for the tracer kernel and everything after it.  (The y launches of the first
// stage may read either version of a word while this runs: both describe their rows correctly, the merged one only knows more.)
int zero_rows_merge(mw_dycore_s *d, hipStream_t st, bool first_cycle) {
  const ZeroRows &z = d->zr;
  if (!z.on) return 0;
  ProfScope ps(d, 4, st);
  const bool dec = zr_decomposed(d);                            // (otherwise the local maps are complete: only MC is left to do)
  if (dec && zr_exchange_merge(d, z.set(z.cur), st)) return 1;
  return zr_finish(d, d->p, z.set(z.cur), st, first_cycle, dec ? 0 : -1);
}

// ---- the maps on their way to the kernels
// The maps of RK stage `stage` (1..3) into the parameter block; stage 0 or a sub-cycle without maps: none
void zero_rows_stage(mw_dycore_s *d, int stage) {
  const ZeroRows &z = d->zr;
  DyP &p = d->p;
  p.zqk = nullptr;
  if (!z.on || stage < 1) { p.zq = p.zqp = p.zqc = nullptr; p.zq_ld = 0; return; }
  p.zq = z.set(z.cur) + (long long)stage * z.msz;
  p.zqp = (z.prev_use && stage <= 2) ? z.set(z.cur ^ 1) + (long long)stage * z.msz : nullptr;   // (S1, S2: the slab of stage s is always the same one)
  p.zqc = (d->o.zero_stores && !d->member_major) ? z.mc() : nullptr;      // (member-major: the coupler's arrays are written by launches that read no maps)
  // (member-major: these are member 0's; view() moves them on to its member)
  p.zq_ld = p.ny + 2 * MW_ZR_HALO;
}
void zero_rows_end_cycle(mw_dycore_s *d) { d->zr.prev_ok = d->zr.on; d->zr.on = false; zero_rows_stage(d, 0); }   // the maps become "the previous sub-cycle's"
// The converting y launch (first stage of a time step, conversion inside k_y_all) writes slab S: before it, hand over what is known about S's
// rows (written by the last conversion into S, untouched since); after it (`done`), S's rows are zero exactly where the coupler's are: map MC.
void zero_rows_conv(mw_dycore_s *d, const double *S, bool done, hipStream_t st) {
  ZeroRows &z = d->zr;
  int sl = (z.conv_slab[0] == S) ? 0 : (z.conv_slab[1] == S) ? 1 : -1;
  if (!done) { d->p.zqk = (sl >= 0 && z.on && d->o.zero_stores) ? z.conv_map(sl) : nullptr; return; }
  d->p.zqk = nullptr;
  if (!z.on) { if (sl >= 0) z.conv_slab[sl] = nullptr; return; }
  if (sl < 0) {                                                 // a free slot, else the one of a slab that is not one of the two q^n slabs any more
    const double *other = (S == d->S0) ? d->S3 : d->S0;
    sl = (z.conv_slab[0] == nullptr) ? 0 : (z.conv_slab[1] == nullptr) ? 1 : (z.conv_slab[0] != other) ? 0 : 1;
  }
  (void)hipMemcpyAsync(z.conv_map(sl), z.mc(), (size_t)z.msz * sizeof(unsigned), hipMemcpyDeviceToDevice, st);
  z.conv_slab[sl] = S;
}
void zero_rows_forget(mw_dycore_s *d, const double *S) {   // slab S (nullptr: any) is about to be written by something that keeps no map
  for (int i = 0; i < 2; i++) if (!S || d->zr.conv_slab[i] == S) d->zr.conv_slab[i] = nullptr;
}
void zero_rows_invalidate(mw_dycore_s *d) { d->zr.prev_ok = false; }   // slabs S1 / S2 are about to be written without maps, or replaced
void zero_rows_free(mw_dycore_s *d) {
  for (void *ptr : {(void *)d->zr.maps, (void *)d->zr.msg, (void *)d->zr.viol}) if (ptr) (void)hipFree(ptr);
  d->zr = ZeroRows();
}

// Option zero_verify (test aid): the maps' claims against the data, on stream `st`, in front of the launches that rely on them.
//   what = 0: in front of the stage's tracer kernel -- the stage's input slab against Qs / QYs, the destination (slab Sout, or the coupler's
//             arrays in the last stage of a time step) against the "holds zeros already" map the kernel was handed;
//   what = 1: in front of the converting y launch -- the slab it fills against zqk.
// Uses the parameter block as the next launch will see it (zero_rows_stage / zero_rows_conv have run).  Counters: mw_debug_zero_violations.
int zero_rows_verify(mw_dycore_s *d, int what, const double *Sin, const double *Sout, bool dst_coupler, const CouplerPtrs &c, hipStream_t st) {
  ZeroRows &z = d->zr;
  if (!d->o.zero_verify || !z.on) return 0;
  if (!z.viol) { MW_HIP(hipMalloc(&z.viol, 4 * sizeof(unsigned long long))); MW_HIP(hipMemsetAsync(z.viol, 0, 4 * sizeof(unsigned long long), st)); }
  for (int e = 0; e < n_views(d); e++) {
    const View v = view(d, e);
    const DyP &p = v.p;
    if (what == 0 && !p.zq) continue;
    if (what == 1 && !p.zqk) continue;
    const long long nrow = (long long)p.nz * p.ny;
    const bool dstc = what == 0 && dst_coupler && p.zqc != nullptr;
    const double *dst = (what == 0 && !dst_coupler && p.zqp) ? v.S(Sout) : nullptr;
    MW_KLAUNCH(k_zero_verify, dim3((unsigned)((nrow + 3) / 4)), dim3(256), 0, st, p, c, what == 0 ? v.S(Sin) : nullptr, dst, dstc ? 1 : 0,
               what == 1 ? v.S(Sin) : nullptr, z.msz, zr_vanish_mask(marching_config(d, p)), z.viol);
    MW_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" {
// Test aid: the zero-row maps of the last sub-cycle, on the host (include/mw_cdna4.h).
long long mw_debug_zero_maps(mw_dycore_t d, unsigned int *out_host, long long cap_words, int *dims2) {
  if (!d) return 0;
  const ZeroRows &z = d->zr;
  if (!z.maps || !z.prev_ok || d->member_major) return 0;       // (prev_ok: the last sub-cycle ran with maps; member-major handles keep one set per member)
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  const long long n = (long long)MW_ZR_MAPS * z.msz;
  if (dims2) { dims2[0] = d->p.nz; dims2[1] = d->p.ny + 2 * MW_ZR_HALO; }
  if (out_host && cap_words > 0)
    (void)hipMemcpy(out_host, z.set(z.cur), (size_t)std::min(n, cap_words) * sizeof(unsigned), hipMemcpyDeviceToHost);
  return n;
}
// Test aid: the four violation counters of option zero_verify (k_zero_verify) since the handle was created; -1: the option
// never ran.  out4: [0] input row non-zero under a clear Qs word, [1] ... under a clear QYs word, [2] a destination row the tracer kernel
// was told holds zeros does not, [3] likewise a row of the slab the converting y launch fills.
long long mw_debug_zero_violations(mw_dycore_t d, unsigned long long *out4) {
  if (!d || !d->zr.viol) return -1;
  (void)hipStreamSynchronize(d->stream);
  if (d->tstream) (void)hipStreamSynchronize(d->tstream);
  unsigned long long h[4] = {0, 0, 0, 0};
  if (hipMemcpy(h, d->zr.viol, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (out4) for (int i = 0; i < 4; i++) out4[i] = h[i];
  return (long long)(h[0] + h[1] + h[2] + h[3]);
}
} // extern "C"
