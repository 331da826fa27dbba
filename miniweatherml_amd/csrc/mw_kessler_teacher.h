// =====================================================================================================
// mw_kessler_teacher.h -- how many rain sub-cycles the Kessler teacher (mw_kessler_members_teacher) runs on one ensemble member.
// One definition for the kernels and for the host (the call's rainsplit_out and mw_kessler_teacher_rainsplit, which the CPU tests pin):
// the count sizes a loop on the device, so it is decided in floating point BEFORE anything is converted to int.  A member whose own
// state asks for more than `cap` sub-cycles, or whose rain CFL step is not a positive finite number (the CFL pass gives 0 for a member
// with non-finite rain or fall speed; whatever else a diverged state may leave in the word), gets 0 = "skipped": it is not computed and costs
// nothing.
// =====================================================================================================
#ifndef MW_KESSLER_TEACHER_H
#define MW_KESSLER_TEACHER_H

#if defined(__HIPCC__)
#define MW_TEACHER_HD __host__ __device__
#else
#define MW_TEACHER_HD
#endif

namespace mw {

// dt_max_bits: the bit pattern of the member's minimum rain CFL step (what the integer atomicMin of the CFL pass leaves), capped at dt.
// -> ceil(dt / dt_max) if dt_max is finite, > 0 and the quotient is in [1, cap]; 0 otherwise.
MW_TEACHER_HD inline int kessler_teacher_rainsplit(double dt, unsigned long long dt_max_bits, int cap) {
  double dt_max;
  __builtin_memcpy(&dt_max, &dt_max_bits, 8);
  if (!(dt_max > 0.0) || !(dt_max <= 1.7976931348623157e308)) return 0;      // 0, negative, NaN, +inf
  const double q = __builtin_ceil(dt / dt_max);                               // a denormal dt_max: inf or huge, refused below
  if (!(q >= 1.0) || !(q <= (double)cap)) return 0;
  return (int)q;                                                              // 1 .. cap: exact
}

// The member's word as the kernels and the host read it: no column of the member lowered it (the word still holds the all-ones
// pattern the call starts from, which is above every double's) -> dt, the value every harmless column stands for.
MW_TEACHER_HD inline unsigned long long kessler_teacher_word(unsigned long long word, double dt) {
  unsigned long long dt_bits;
  __builtin_memcpy(&dt_bits, &dt, 8);
  return word < dt_bits ? word : dt_bits;                                     // dt > 0: positive doubles order like their bit patterns
}

} // namespace mw
#endif
