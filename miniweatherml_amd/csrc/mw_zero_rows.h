// =====================================================================================================
// mw_zero_rows.h -- the zero-row maps: what the marching kernels (mw_march.h) and the maps' own unit (mw_zero_rows.hip: the five k_zero_*
// kernels and all host code) share -- the constants and word layout of a map, the segment helpers, the handle's state and the host interface.
// =====================================================================================================
#pragma once
#include "mw_common.h"

namespace mw {

// ---------------------------------------------------------------------------------------------------------------
// Zero-row maps (round 5).  Cloud water and rain are exactly zero over most of a supercell domain (all of it at the start), and after
// the zero short-cut (MW_ZERO_SKIP) the fused tracer kernel is bound by the HBM traffic of values that are all zero.  The maps let it
// not issue those loads at all:
//   M0[k][j], bit v : tracer v is non-zero somewhere in the x row (k, j) of the sub-cycle's input q^n   (k_zero_rows: one pass over the
//                     tracers that can vanish, 16 bytes per cell of the ~500 a stage moves)
//   Qs[k][j], bit v : (s = 1, 2, 3) tracer v may be non-zero in something that iterations k-3 .. k of row j's marching wave touch in RK
//                     stage s: the OR of M0 over rows j-3s .. j+3s (periodic) and levels k-3s-5 .. k+3s+1 (clamped)  (k_zero_dilate)
// One RK stage moves a tracer by at most 3 cells per direction (cell (k, j) is updated from the faces j, j+1 / k, k+1, whose upwind
// WENO-5 stencils reach rows j-3 .. j+3 / levels k-3 .. k+3; an FCT multiplier only scales a flux, the y-face correction of
// k_tracer_patch is a difference of scaled and unscaled flux, and every stage adds q^n's own row), and a flux of zeros is zero: a row
// that is non-zero in the input of stage s (its output, its y fluxes) lies within 3(s-1) (3s) rows and levels of a non-zero row of q^n.
// Iteration k of k_tracers_fused reads input levels k-2 .. k+3, y fluxes of levels k-1 .. k+1 and q^n of levels k-2 .. k+2, and its
// carries come from the three iterations before (input levels from k-5, y fluxes from k-5): with Qs[k][j]'s bit clear all of that is
// exactly zero, and so is the tracer's new value.  The maps are a SUPERSET of the non-zero rows -- a set bit costs the loads, nothing
// else -- and results equal the run without them (tests/: bitwise up to the sign of a zero; a skipped value enters as +0.0).
// (Which handles run with maps: zero_rows_ok in mw_zero_rows.hip.)
// ---------------------------------------------------------------------------------------------------------------
#define MW_ZR_REACH 3
#define MW_ZR_HALO (3 * MW_ZR_REACH)                              // rows a tracer can travel in one sub-cycle = halo rows of the maps
// x SEGMENTS (round 6).  A storm covers a fifth of the x rows but a fourteenth of the 58-cell tiles a marching wave works on (bench.py:
// storm.extent), so a word also says WHERE in its row something can be:
//   bits 0 .. 3   tracer v may be non-zero somewhere in the row (as before; the y kernel's store decision, the tests)
//   bits 4 .. 29  segment s of the row -- cells [s L, (s + 1) L), L = ceil(NXI / 26) -- may hold a non-zero value of a tracer that can vanish.
//                 Set at SCAN time for every segment within MW_ZR_HALO = 9 cells of a non-zero cell (what a whole sub-cycle can move it in
//                 x; periodic when one rank owns the direction), so that the row / level growth of k_zero_dilate -- a plain OR of words --
//                 carries the segments along.  A wave is lean when the segments its lanes (halo lanes and patch cells included) overlap are clear.
//   bits 30, 31   (the compact copy a block sends to its west / east neighbours only) the grown set touches the block's west / east edge:
//                 the neighbour then sets the segments of its first / last 9 cells (k_zero_merge).
// Per cell the invariants are the old ones -- "bit clear => the cell is zero" -- so the zero-store rules hold cell by cell whatever the tiling.
#define MW_ZR_SEGS 26
#define MW_ZR_SEG_SHIFT 4
#define MW_ZR_ROWBITS 0xFu
#define MW_ZR_TOUCH_W 0x40000000u
#define MW_ZR_TOUCH_E 0x80000000u
__host__ __device__ __forceinline__ int zr_seg_len(int NXI) { return (NXI + MW_ZR_SEGS - 1) / MW_ZR_SEGS; }
// segment bits (in place: shifted) of the cells [a, b], 0 <= a <= b < NXI
__host__ __device__ __forceinline__ unsigned zr_seg_span(int a, int b, int L) { return ((2u << (b / L)) - (1u << (a / L))) << MW_ZR_SEG_SHIFT; }
// ... of the cells [lo, hi] of a row of NXI cells (lo may be < 0, hi >= NXI): periodic images when `wrap`, else clamped into the row
__host__ __device__ __forceinline__ unsigned zr_seg_mask(int lo, int hi, int NXI, bool wrap) {
  const int L = zr_seg_len(NXI);
  if (hi - lo + 1 >= NXI) return zr_seg_span(0, NXI - 1, L);
  if (!wrap) return zr_seg_span(max(lo, 0), min(hi, NXI - 1), L);
  if (lo < 0) return zr_seg_span(lo + NXI, NXI - 1, L) | zr_seg_span(0, hi, L);
  if (hi >= NXI) return zr_seg_span(lo, NXI - 1, L) | zr_seg_span(0, hi - NXI, L);
  return zr_seg_span(lo, hi, L);
}
// Map layout: word of (k, j) at [k * zq_ld + j + MW_ZR_HALO], zq_ld = ny + 2 MW_ZR_HALO (j = -9 .. ny+8: the rows beyond the block's
// south / north edge -- its own rows again when it owns the periodic y direction, the neighbours' rows otherwise).
// Blocks of a decomposed domain (pipelined schedule): a row's x halo holds the west / east neighbour's cells and its tracer can come
// from there, so M0 is OR-ed with the neighbours' M0 of the same row (k_zero_merge; whole rows: coarse, but a superset), and the rows
// beyond the y edges come from the south / north neighbours' merged maps -- two small messages per sub-cycle through the handle's
// halo transport, on the exchange stream beside the stage's y and x/z kernels.
// A SET of maps is M0 and the nine that k_zero_dilate derives from it, msz = nz * zq_ld words each, Q_s at M + s * msz:
//   FNs[k][j] at M + (3 + s) * msz = the OR of Qs[k-1 .. k+1][j]: "row j's tracer kernel may load its y fluxes of level k" (its iteration k'
//   reads level k'-1, clamped into the chunk: k' = k-1, k or k+1) -- k_y_all does not store the fluxes of a face whose two rows are clear.
#define MW_ZR_BEFORE 5                                            // levels below: the three iterations whose carries an iteration inherits
#define MW_ZR_AFTER 1                                             // levels above: the y fluxes of level k+1 (chunk ends clamp k-1 upwards)
//   QYs[k][j] at M + (6 + s) * msz = M0 dilated by 3s rows and 3(s-1) levels = the input of stage s, three more rows either way: what
//   iteration j of k_y_all's wave at level k touches (the window of face j, the row that enters it, the edge value carried from j-1).
#define MW_ZR_MAPS 10                                             // maps per set -- M0, Q1..Q3, FN1..FN3, QY1..QY3
// Zeros are not stored over zeros either (DyP::zqc / zqp / zqk, host side: zero_rows_stage / zero_rows_conv):
//   MC (zqc) = M0 of the time step's FIRST sub-cycle = which rows of the coupler's own tracer arrays are zero (nothing writes them before the
//   last sub-cycle's D13): a lean iteration of the last stage does not store there;
//   the PREVIOUS sub-cycle's Qs (zqp; s = 1, 2 -- slabs S1 and S2 always take the output of stages 1 and 2): level k of a row is stored by
//   iteration k+2, in the lean form (zeros) exactly when Qs[k+2][j] was clear -- for every x tile of the row alike, the form follows from the
//   row's word alone -- so where the previous Qs is clear the slab row holds zeros already and a lean iteration leaves it alone.  The host
//   hands the previous maps over only when the previous sub-cycle ran with maps and nothing else has written the slabs since.

// Tracers that can be identically zero over large parts of a domain (see the zero short-cut of k_tracers_fused): everything but the
// water vapour of the supercell set-ups; simple_city's vapour IS zero (its only tracer); with the switches at run time: all of them.
// (DyP::zero_skip = the handle's option zero_skip: 0 switches the short-cut off at run time -- the bitwise A/B of tests/ and tools/)
template <int K> __device__ __forceinline__ bool tracer_may_vanish(const DyP &p, int v) { return p.zero_skip && (K == 1 ? v != 0 : true); }
// ... as the mask the map kernels scan, for the marching configuration K (marching_config) of a handle that runs with maps
inline unsigned zr_vanish_mask(int K) { return (K == 1) ? 0x6u : 0xFu; }

} // namespace mw

// ---- host side (mw_zero_rows.hip) -------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)      // nothing below is part of the library's ABI
struct mw_dycore_s;

// The handle's zero-row state (mw_dycore_s::zr).  One allocation holds, per member (nens == 1: one member), two SETS of MW_ZR_MAPS maps --
// double-buffered by sub-cycle --, then map MC, then the two conversion maps: 2 * MW_ZR_MAPS + 3 maps of `msz` words.
struct ZeroRows {
  unsigned *maps = nullptr;                  // the map allocation described above (nullptr: no sub-cycle has run with maps yet)
  long long msz = 0;                         // words per map: nz * (ny + 2 * MW_ZR_HALO), of the block size `maps` was allocated for
  double *msg = nullptr;                     // message buffers of a decomposed block's map exchange, in doubles (the transport's unit): see slices()
  bool on = false;                           // the running sub-cycle has maps (zero_rows_ok, and the allocation succeeded)
  int cur = 0;                               // set `cur` belongs to the running sub-cycle, set `cur ^ 1` to the one before
  bool prev_ok = false;                      // set `cur ^ 1` describes what slabs S1 / S2 hold now: the sub-cycle before ran with maps and nothing else has written the slabs since
  bool prev_use = false;                     // prev_ok held when this sub-cycle's maps were built and option zero_stores is on: set `cur ^ 1` is handed to its kernels (DyP::zqp)
  const double *conv_slab[2] = {nullptr, nullptr};   // the two slabs that take turns as q^n: slab conv_slab[i]'s rows are zero where conversion map i says so (the last conversion into it left them zero, nothing has written it since); nullptr: slot free
  unsigned long long *viol = nullptr;        // option zero_verify: the four violation counters of k_zero_verify (nullptr: the option never ran)

  long long member_words() const { return (2 * MW_ZR_MAPS + 3) * msz; }    // from one member's maps to the next member's
  unsigned *set(int which, int e = 0) const { return maps + e * member_words() + (long long)which * MW_ZR_MAPS * msz; }   // M0 of set `which` (cur, cur ^ 1) of member e
  unsigned *mc() const { return maps + 2 * MW_ZR_MAPS * msz; }             // map MC
  unsigned *conv_map(int slot) const { return mc() + (1 + slot) * msz; }   // the map that goes with conv_slab[slot]
  // The slices of `msg` for a block of nz x ny rows: the block's own compact [k][ny] map (sent west and east) and what the west / east
  // neighbours sent, dWE doubles each; the merged edge rows packed for the south / north neighbours and what those sent, dSN doubles each.
  struct Msg { long long dWE, dSN; double *own, *rW, *rE, *sS, *sN, *rS, *rN; };
  Msg slices(int nz, int ny) const {
    const long long w = ((long long)nz * ny + 1) / 2, s = ((long long)nz * MW_ZR_HALO + 1) / 2;
    return {w, s, msg, msg + w, msg + 2 * w, msg + 3 * w, msg + 3 * w + s, msg + 3 * w + 2 * s, msg + 3 * w + 3 * s};
  }
};

// The unit's functions (what each does: at its definition) -- which handles run with maps; a sub-cycle's maps all at once or as a local
// and a merge half; the maps of a stage into the parameter block, the sub-cycle's end; what is known about the rows of a slab; test aid; destroy
bool zero_rows_ok(const mw_dycore_s *d);
int zero_rows_build(mw_dycore_s *d, const double *S0, const mw::CouplerPtrs &c, bool from_coupler, hipStream_t st, bool first_cycle);
int zero_rows_local(mw_dycore_s *d, const double *S0, const mw::CouplerPtrs &c, bool from_coupler, hipStream_t st);
int zero_rows_merge(mw_dycore_s *d, hipStream_t st, bool first_cycle);
void zero_rows_stage(mw_dycore_s *d, int stage);
void zero_rows_end_cycle(mw_dycore_s *d);
void zero_rows_conv(mw_dycore_s *d, const double *S, bool done, hipStream_t st);
void zero_rows_forget(mw_dycore_s *d, const double *S);
void zero_rows_invalidate(mw_dycore_s *d);
int zero_rows_verify(mw_dycore_s *d, int what, const double *Sin, const double *Sout, bool dst_coupler, const mw::CouplerPtrs &c, hipStream_t st);
void zero_rows_free(mw_dycore_s *d);
#pragma GCC visibility pop
