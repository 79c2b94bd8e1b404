// Stochastic rounding of fp32 to bf16 and its counter-based generator: one definition for the
// kernels (csrc/zs_kernels.hip), the host entry points zs_sr_keys / zs_sr_bits and stand-alone host
// programs (tools/sr_host_check.cpp).  Plain C++; under hipcc every function is host and device.
// DESIGN.md §4, "Stochastic rounding of bf16 moments", states the definition.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ZS_SR_FN __host__ __device__ __forceinline__
#else
#define ZS_SR_FN inline
#endif

namespace zs_sr {

// lowbias32 (an avalanching 32-bit integer hash: two multiplies, three xor-shifts)
ZS_SR_FN uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// The two keys of one launch: a function of the optimizer's seed and the torch step of the part.
// (The added constant keeps key1 from being lowbias32(key0) when both high words are 0: element
// 0 would then draw key1 ^ key1 = 0 at every step.)
ZS_SR_FN void keys(uint64_t seed, uint64_t t, uint32_t* k0, uint32_t* k1) {
  *k0 = lowbias32(uint32_t(t) ^ uint32_t(seed));
  *k1 = lowbias32((*k0 ^ uint32_t(seed >> 32) ^ uint32_t(t >> 32)) + 0x9E3779B9u);
}

// 32 random bits of element e of the shard's moment array: exp_avg rounds with the low 16,
// exp_avg_sq with the high 16.
// One hash round per element (two 32-bit multiplies): the index's high word and key0 go in
// before it, key1 on after it.
ZS_SR_FN uint32_t bits(uint64_t e, uint32_t k0, uint32_t k1) {
  return lowbias32(uint32_t(e) ^ k0 ^ (uint32_t(e >> 32) * 0x9E3779B9u)) ^ k1;
}

// The keys of the parameter's draw in a master-free launch (zs_adamset_run_psr), from the launch's
// keys: r16p = bits(e, kp0, kp1) & 0xFFFF.  Each goes through a hash round of its own, so the draw
// is independent of the m and v halves of bits(e, k0, k1) of the same element.
ZS_SR_FN void pkeys(uint32_t k0, uint32_t k1, uint32_t* kp0, uint32_t* kp1) {
  *kp0 = lowbias32(k0 ^ 0x85EBCA6Bu);
  *kp1 = lowbias32(k1 + 0xC2B2AE35u);
}

// fp32 bits u -> bf16 code, r16 in [0, 65535].  Sign-magnitude: away from zero with probability
// low16(u) / 65536, exact when low16(u) == 0; a carry out of the largest finite value is Inf (a
// finite u + 0xFFFF stays below 2^32, and Inf + r16 keeps its high half).  A NaN takes `nan_code`,
// the round-to-nearest conversion's result, instead.
ZS_SR_FN uint16_t round_bf16(uint32_t u, uint32_t r16, uint16_t nan_code) {
  const bool nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
  return nan ? nan_code : uint16_t((u + r16) >> 16);
}

// the host's round-to-nearest-even of a NaN: quiet, payload's high bits kept
ZS_SR_FN uint16_t nan_bf16(uint32_t u) { return uint16_t((u >> 16) | 0x40u); }

}  // namespace zs_sr
