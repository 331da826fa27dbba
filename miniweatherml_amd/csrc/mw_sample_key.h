// mw_sample_key.h -- the draw of the sample masks (k_sample_mask in mw_output.hip, k_member_sample_mask in mw_member.hip): one
// definition, so that a cell's key gives the same number in both.
#ifndef MW_SAMPLE_KEY_H
#define MW_SAMPLE_KEY_H
namespace mw {
// splitmix64's finaliser of the key, its top 53 bits as a double in [0, 1)
__device__ __forceinline__ double u01_from_key(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
} // namespace mw
#endif
