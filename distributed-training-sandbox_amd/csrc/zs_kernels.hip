// CDNA4 (gfx950) kernels of the ZeRO step and the C entry points that launch them: segment copy
// (pack / unpack), the fused optimizer update (one vector and one scalar kernel, instantiated over
// the element rules: Adam, Adam with bf16 moments rounded to nearest or stochastically, Adam over
// master-free bf16 parameters rounded stochastically, SGD), the
// gradient sum of squares and clip coefficient, scale, accumulate, convert, the fp8 row quantizer
// and gather, and the flag kernels.
//
// The copy and update kernels are HBM-bound streaming kernels (no MFMA, no LDS): 64-wide waves,
// 256-thread workgroups, 16-byte-per-lane coalesced accesses, a grid of 128 workgroups per CU (16x
// the 8 resident; 1024 per CU for the split-master update) that strides over fixed-size chunks of
// a segment table.  A workgroup finds the segment of its chunk with a forward scan from the
// previous one (chunks are visited in increasing order), so the lookup is a couple of scalar loads,
// not a per-chunk binary search (the update bisects once, for its first chunk).  The update issues
// all of a full chunk's loads (20 for the split-master Adam) before its first wait and addresses
// them from scalar bases, which keeps its headline instance, adam_segments_kernel<AdamRule<false>,
// unsigned short, false, true, true, false, float> (bf16 gradients, split master, loads first), at
// 79 VGPRs and 106 SGPRs: 6 waves per SIMD, no scratch.
//
// Tables (segment pointers + chunk prefix sums) are uploaded once per set and reused every step:
// the step itself only launches kernels (no host sync), so it can be captured into a hipGraph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "zs_common.h"
#include "zs_sr.h"

namespace {

constexpr int kThreads = 256;
// segment copy: U 16-byte accesses in flight per lane, a workgroup step moves 256 * 16 * U bytes
constexpr int kCopyUnrollDefault = 4;
constexpr int64_t copy_chunk_bytes(int u) { return int64_t(kThreads) * 16 * u; }
// float4 groups per thread: 2 (2048-element chunks); 4 (4096) for the split master, whose 26 B/elem
// stream has one fp32 array fewer per group (+1 % measured with the predicated body, which has one
// group's loads in flight at a time: profiles/r01_adam_split_master.log).  update_full_chunk has all
// G groups' loads in flight at once: 5 G loads, 14 G raw registers per lane for the split master.
constexpr int adam_groups(bool split) { return split ? 4 : 2; }
constexpr int64_t adam_chunk(bool split) { return int64_t(kThreads) * 4 * adam_groups(split); }

int grid_cap() {
  static int cap = 0;
  if (cap == 0) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    }
    // 128 workgroups per CU (16x the resident 8): the best of 32/64/128/512/one-per-chunk for the
    // Adam and copy kernels at C4 scale (profiles/r01_adam_variants2.log)
    cap = cus * 128;
  }
  return cap;
}

// Kernel pointers live in the global address space; a plain pointer loaded from a table would
// lower to flat_load/flat_store (which also count in lgkmcnt and complete out of order).
#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
using gptr = __attribute__((address_space(1))) T*;
#else
template <typename T>
using gptr = T*;
#endif
template <typename T>
__device__ __forceinline__ gptr<T> glob(T* p) {
  return (gptr<T>)p;
}

// Streaming accesses carry the non-temporal hint (global_load/store ... nt): nothing these kernels
// touch is re-read while it could still be cached, and at C4 scale (86 GB per Adam launch) the hint
// measured +4-6 % over plain accesses, loads and stores alike (profiles/r01_adam_variants2.log).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint4 nt_ld16(const void* p) {
  const u32x4 v = __builtin_nontemporal_load((gptr<const u32x4>)p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_st16(void* p, uint4 x) {
  const u32x4 v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, (gptr<u32x4>)p);
}
__device__ __forceinline__ uint2 nt_ld8(const void* p) {
  const u32x2 v = __builtin_nontemporal_load((gptr<const u32x2>)p);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void nt_st8(void* p, uint2 x) {
  const u32x2 v = {x.x, x.y};
  __builtin_nontemporal_store(v, (gptr<u32x2>)p);
}
// the same accesses with the cache policy chosen at compile time (NT: non-temporal hint)
template <bool NT>
__device__ __forceinline__ uint4 ld16(const void* p) {
  if constexpr (NT) return nt_ld16(p);
  else return *(gptr<const uint4>)p;
}
template <bool NT>
__device__ __forceinline__ void st16(void* p, uint4 x) {
  if constexpr (NT) nt_st16(p, x);
  else *(gptr<uint4>)p = x;
}
template <bool NT>
__device__ __forceinline__ uint2 ld8(const void* p) {
  if constexpr (NT) return nt_ld8(p);
  else return *(gptr<const uint2>)p;
}
template <bool NT>
__device__ __forceinline__ void st8(void* p, uint2 x) {
  if constexpr (NT) nt_st8(p, x);
  else *(gptr<uint2>)p = x;
}
// Above this many bytes a buffer cannot sit in the 256 MB MALL (Infinity Cache): the in-place scale
// and the conversions take the non-temporal policy there and the default policy below, where the
// buffer was usually just written (an all-reduce, a backward) and is read next (the collective).
constexpr int64_t kMallBytes = int64_t(256) << 20;

// ----------------------------------------------------------------------------------------------
// segment copy
// ----------------------------------------------------------------------------------------------
struct CopySeg {
  const unsigned char* src;  // nullptr = zero fill
  unsigned char* dst;
  int64_t nbytes;
  int64_t vec;  // 1 if src and dst are 16-byte aligned (or src is null and dst aligned)
};

// Cache policy by size (NT) as zs_scale / zs_convert: non-temporal when the set moves more than the
// MALL holds (a C4 pack group, a checkpoint), the default policy below (a 64 MB overlap bucket, read
// next by its collective); `zs_tune("copy_nt")` forces either.
// One chunk [b0, b1) of one segment, by the whole workgroup.
template <int U, bool NT>
__device__ __forceinline__ void copy_chunk(const unsigned char* s_src, unsigned char* s_dst, bool vec,
                                           int64_t b0, int64_t b1) {
  const gptr<const unsigned char> src = glob(s_src);
  const gptr<unsigned char> dst = glob(s_dst);
  if (vec) {
    uint4 val[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // all loads first: U x 16 B in flight per lane
      const int64_t off = b0 + (int64_t(u) * kThreads + threadIdx.x) * 16;
      val[u] = make_uint4(0, 0, 0, 0);
      if (s_src && off + 16 <= b1) val[u] = ld16<NT>(s_src + off);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = b0 + (int64_t(u) * kThreads + threadIdx.x) * 16;
      if (off + 16 <= b1) {
        st16<NT>(s_dst + off, val[u]);
      } else if (off < b1) {
        for (int64_t b = off; b < b1; ++b) dst[b] = s_src ? src[b] : 0;
      }
    }
  } else {
    for (int64_t b = b0 + threadIdx.x; b < b1; b += kThreads) dst[b] = s_src ? src[b] : 0;
  }
}

template <int U, bool NT>
__global__ __launch_bounds__(kThreads) void copy_segments_kernel(
    const CopySeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks) {
  constexpr int64_t kChunk = copy_chunk_bytes(U);
  int64_t seg = 0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;  // uniform forward scan
    const CopySeg s = segs[seg];
    const int64_t b0 = (c - chunk_prefix[seg]) * kChunk;
    copy_chunk<U, NT>(s.src, s.dst, s.vec != 0, b0, min(b0 + kChunk, s.nbytes));
  }
}

// The same copy with up to kDirectMax segments passed BY VALUE in the kernel arguments: no
// descriptor table to allocate and upload, so a set whose pointers change every call (backward's
// fresh gradients into their arena slots) costs one launch and nothing else.
constexpr int kDirectMax = 64;
struct DirectSet {
  const unsigned char* src[kDirectMax];  // nullptr = zero fill
  unsigned char* dst[kDirectMax];
  int64_t nbytes[kDirectMax];
  int64_t prefix[kDirectMax + 1];  // chunk prefix over the segments
  uint64_t vec_mask;               // bit i: segment i is 16-byte aligned on both sides
  int n;
};

template <int U, bool NT>
__global__ __launch_bounds__(kThreads) void copy_direct_kernel(const DirectSet set) {
  constexpr int64_t kChunk = copy_chunk_bytes(U);
  const int64_t total = set.prefix[set.n];
  int seg = 0;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    while (set.prefix[seg + 1] <= c) ++seg;  // uniform forward scan
    const int64_t b0 = (c - set.prefix[seg]) * kChunk;
    copy_chunk<U, NT>(set.src[seg], set.dst[seg], (set.vec_mask >> seg) & 1, b0,
                      min(b0 + kChunk, set.nbytes[seg]));
  }
}

// ----------------------------------------------------------------------------------------------
// fused optimizer update: one chunk-streaming skeleton, three element rules (Adam, SGD, Lion)
// ----------------------------------------------------------------------------------------------
struct AdamSeg {
  const void* g;
  const float* master;
  float* master_out;
  unsigned short* p_out;
  float* m;
  float* v;
  float* vmax;
  float* carry;
  int64_t n;
};

__device__ __forceinline__ float bf16_to_f32(unsigned short h) {
  return __uint_as_float(uint32_t(h) << 16);
}

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  // round-to-nearest-even; NaN stays NaN (plain cast lowers to v_cvt_pk_bf16_f32 on gfx950)
  __bf16 h = static_cast<__bf16>(f);
  unsigned short r;
  __builtin_memcpy(&r, &h, 2);
  return r;
}

// Split master (ZS_BF16_SPLIT): the fp32 master's bits u live as hi = RNE-bf16(u) — the bf16 param
// itself — and the int16 residual lo = u - (hi << 16), so u = (hi << 16) + sext(lo).  The one
// residual int16 cannot hold, +0x8000 (an exact tie rounded down to an even hi), is stored as
// 0x7FFF: that master moves 1 ulp toward zero and its bf16 param stays the same.
__device__ __forceinline__ float join_master(uint32_t hi, uint32_t lo) {
  return __uint_as_float((hi << 16) + uint32_t(int32_t(int16_t(uint16_t(lo)))));
}
__device__ __forceinline__ uint32_t master_residual(float p, uint32_t hi) {
  const uint32_t d = __float_as_uint(p) - (hi << 16);
  return d == 0x8000u ? 0x7FFFu : (d & 0xFFFFu);
}

// The four elements of one lane access and back: fp32 in 16 bytes, bf16 in 8, and the split
// master's hi and lo words (8 bytes each).  Callers name a packed value before they form the
// address it goes to where the code did so before: the order of the two shows in the schedule.
__device__ __forceinline__ void unpack4(const uint4& q, float* f) {
  f[0] = __uint_as_float(q.x), f[1] = __uint_as_float(q.y);
  f[2] = __uint_as_float(q.z), f[3] = __uint_as_float(q.w);
}
__device__ __forceinline__ uint4 pack4(const float* f) {
  return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                    __float_as_uint(f[3]));
}
__device__ __forceinline__ void unpack_bf16x4(const uint2& d, float* f) {
  f[0] = __uint_as_float(d.x << 16), f[1] = __uint_as_float(d.x & 0xffff0000u);
  f[2] = __uint_as_float(d.y << 16), f[3] = __uint_as_float(d.y & 0xffff0000u);
}
__device__ __forceinline__ uint2 pack_bf16x4(const float* f) {
  uint2 r;
  r.x = uint32_t(f32_to_bf16(f[0])) | (uint32_t(f32_to_bf16(f[1])) << 16);
  r.y = uint32_t(f32_to_bf16(f[2])) | (uint32_t(f32_to_bf16(f[3])) << 16);
  return r;
}
__device__ __forceinline__ void join_master4(const uint2& h, const uint2& l, float* p) {
  p[0] = join_master(h.x & 0xFFFFu, l.x), p[1] = join_master(h.x >> 16, l.x >> 16);
  p[2] = join_master(h.y & 0xFFFFu, l.y), p[3] = join_master(h.y >> 16, l.y >> 16);
}
// four masters as their bf16 params h and residuals l, 16 bits each, and four such in 8 bytes
__device__ __forceinline__ void split_master4(const float* p, uint32_t* h, uint32_t* l) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    h[j] = f32_to_bf16(p[j]);
    l[j] = master_residual(p[j], h[j]);
  }
}
__device__ __forceinline__ uint2 pack_u16x4(const uint32_t* h) {
  return make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
}

// The gradient both rules start from (HPT: HP or SgdHP, which name these fields alike): the ZeRO-1
// carry, the averaging, CLIP and maximize, one fp32 operation each.  The coupled weight decay that
// follows, fma(wd, p, g), stands in each rule: read here, p is loaded a block earlier than it was.
//
// CLIP (zs_adamset_run_clipped, zs_sgdset_run with a coefficient): the averaged gradient times the
// global-norm clip coefficient (clip_grad_norm_'s `g.mul_(clip_coef_clamped)`), one IEEE multiply
// before maximize / weight decay; `coef` is uniform (a scalar register) and unused otherwise.
template <bool CARRY, bool CLIP, typename HPT>
__device__ __forceinline__ float prep_grad(float gsum, float& carry, const HPT& hp, float coef) {
#pragma clang fp contract(off)
  float s = gsum;
  if constexpr (CARRY) s = s + hp.carry_mul * carry;  // ZeRO-1: Σ G + (ws-1)·A_{t-1}
  // zero1.py:84 / zero2.py:111 `grad / ws`; a power-of-two divisor is an exact reciprocal multiply
  float g = hp.div_pow2 ? s * hp.inv_div : s / hp.grad_div;
  if constexpr (CARRY) carry = g;
  if constexpr (CLIP) g = g * coef;
  if (hp.maximize) g = -g;
  return g;
}

// An element rule gives the skeleton below its hyperparameter struct (Hyper), which of a
// segment's state arrays an instance reads and writes (kM: m, kV: v, kX: vmax) and the update of
// one element, elem<CARRY, CLIP>(gsum, p, m, v, vmax, carry, hp, coef); state it does not touch is
// passed as a dummy.  kGradOffset2: see update_full_chunk.

// Rule::Stats: what a lane carries through the bodies of one chunk beside the update -- nothing
// (NoStats), or AdamStatsRule's two running sums.
struct NoStats {};
struct LaneStats {
  float d = 0.0f, w = 0.0f;
};

// lerp_w / lerp_hi: ATen's lerp (Lerp.h) with weight w = 1-beta1 is self + w*(end-self) for
// |w| < 0.5 and end - (end-self)*(1-w) otherwise; make_hp holds the fma's coefficient (w, or w-1 in
// one fp32 subtraction) and which operand it adds to, so the choice is uniform.
struct HP {
  float lerp_w, beta2, omb2, neg_step, bc2_sqrt, eps, wd, decay_mul, grad_div, inv_div, carry_mul;
  int div_pow2, maximize, lerp_hi;
};

template <bool AMS>
struct AdamRule {
  using Hyper = HP;
  static constexpr bool kM = true, kV = true, kX = AMS, kGradOffset2 = true;
  static constexpr bool kPsr = false;  // AdamPsrRule: no master, the bf16 parameter in place
  static constexpr bool kEma = false;  // AdamEmaRule: the vmax stream is an EMA of the stored master
  static constexpr bool kStats = false;  // AdamStatsRule: per-chunk sums of (p1 - p0)^2 and p1^2
  using Stats = NoStats;

  // One element of torch.optim.Adam's single-tensor update (adam.py:394-547), one fp32 operation
  // per operation of torch's CPU kernels: lerp = fma(w, end-self, self) or fma(w-1, end-self, end)
  // (ATen Lerp.h, by |w| < 0.5), exp_avg_sq.mul_(b2).addcmul_(g,g,1-b2) = fma((1-b2)*g, g, v*b2),
  // max_exp_avg_sq = maximum (NaN in either operand stays), denom = sqrt(v)/bc2_sqrt + eps,
  // param.addcdiv_(m, denom, -step_size) = p + (-step_size*m)/denom.  Only explicit fmaf() fuse;
  // sqrt and '/' are IEEE correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt).  m, v and
  // vmax equal live torch bit for bit; p stays within 0.5 ulp + 6 * 2^-24 * |update| of the exact
  // step, like torch's own p, whose vectorized CPU sqrt is not correctly rounded.
  template <bool CARRY, bool CLIP>
  static __device__ __forceinline__ void elem(float gsum, float& p, float& m, float& v,
                                              float& vmax, float& carry, const HP& hp,
                                              float coef) {
#pragma clang fp contract(off)
    float g = prep_grad<CARRY, CLIP>(gsum, carry, hp, coef);
    if (hp.wd != 0.0f) g = fmaf(hp.wd, p, g);  // grad.add(param, alpha=wd)
    p = p * hp.decay_mul;  // AdamW: param.mul_(1 - lr*wd); 1.0 otherwise
    m = fmaf(hp.lerp_w, g - m, hp.lerp_hi ? g : m);
    v = fmaf(hp.omb2 * g, g, v * hp.beta2);
    float vv = v;
    if constexpr (AMS) {
      vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: fmaxf would drop a NaN
      vv = vmax;
    }
    const float denom = sqrtf(vv) / hp.bc2_sqrt + hp.eps;
    p = p + (hp.neg_step * m) / denom;
  }
};

// Stochastic rounding of bf16 moments (zs_adamset_run_sr).  SrBf16 as ST names the stochastic
// instances: 16-bit m and v like `unsigned short`, stored through zs_sr::round_bf16 with 16 bits of
// zs_sr::bits(e, k0, k1) each, e = the element's index in the shard's m array (its address less
// m_base, in elements).  The keys and m_base ride behind Adam's HP, so no other instance sees them.
struct SrBf16 {
  unsigned short bits;
};
struct SrHP : HP {
  uint32_t k0, k1;
  uint64_t m_base;
};
struct AdamSrRule : AdamRule<false> {
  using Hyper = SrHP;
};
template <typename ST>
inline constexpr bool kStochastic = std::is_same_v<ST, SrBf16>;

// index of a segment's element 0 in the shard's m array (uniform: scalar registers)
template <typename HPT>
__device__ __forceinline__ uint64_t sr_seg_index(const float* m, const HPT& hp) {
  return (uint64_t(reinterpret_cast<uintptr_t>(m)) - hp.m_base) >> 1;
}
// zs_sr::bits(eu + off, k0, k1) for a uniform eu and a per-lane off: the high word of the sum is
// eu's or one more, so its multiply and the xor with k0 stay scalar and a lane selects
// (HPT: SrHP or LionSrHP, which name k0, k1 and m_base alike)
template <typename HPT>
__device__ __forceinline__ uint32_t sr_bits_at(uint64_t eu, uint32_t off, const HPT& hp) {
  const uint32_t lo0 = uint32_t(eu), hi = uint32_t(eu >> 32);
  const uint32_t lo = lo0 + off;
  const uint32_t ka = hp.k0 ^ (hi * 0x9E3779B9u), kb = hp.k0 ^ ((hi + 1u) * 0x9E3779B9u);
  return zs_sr::lowbias32(lo ^ (lo < lo0 ? kb : ka)) ^ hp.k1;
}
// zs_sr::round_bf16(u, r16, zs_sr::nan_bf16(u)) with the code left in the word's high half: one
// add, and a NaN (quiet, its payload's high bits kept) selected over it; two such words pack in
// one operation.  sr_narrow: m and v of one element, one draw for both.
__device__ __forceinline__ uint32_t sr_word(float x, uint32_t r16) {
  const uint32_t u = __float_as_uint(x);
  return x != x ? (u | 0x00400000u) : u + r16;
}
__device__ __forceinline__ void sr_narrow(float m, float v, uint32_t r, uint32_t& mw, uint32_t& vw) {
  mw = sr_word(m, r & 0xFFFFu);
  vw = sr_word(v, r >> 16);
}
__device__ __forceinline__ uint32_t sr_pack2(uint32_t w0, uint32_t w1) {
  return (w0 >> 16) | (w1 & 0xFFFF0000u);
}
// Four elements from index eu + off on, packed for one 8-byte store each.  HPT: the instance's
// Hyper (SrHP wherever this is reached).
template <typename HPT>
__device__ __forceinline__ void sr_pack_bf16x4(const float* mp, const float* vp, uint64_t eu,
                                               uint32_t off, const HPT& hp, uint2& mr, uint2& vr) {
  uint32_t mw[4], vw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sr_narrow(mp[j], vp[j], sr_bits_at(eu, off + j, hp), mw[j], vw[j]);
  mr = make_uint2(sr_pack2(mw[0], mw[1]), sr_pack2(mw[2], mw[3]));
  vr = make_uint2(sr_pack2(vw[0], vw[1]), sr_pack2(vw[2], vw[3]));
}
// The same for a rule whose only 16-bit state is m (LionSrRule): the low half of each element's
// draw, the one Adam's exp_avg takes; the high half is not used.
template <typename HPT>
__device__ __forceinline__ uint2 sr_pack_m_bf16x4(const float* mp, uint64_t eu, uint32_t off,
                                                  const HPT& hp) {
  uint32_t mw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) mw[j] = sr_word(mp[j], sr_bits_at(eu, off + j, hp) & 0xFFFFu);
  return make_uint2(sr_pack2(mw[0], mw[1]), sr_pack2(mw[2], mw[3]));
}

// Master-free bf16 parameters (zs_adamset_run_psr over a ZS_BF16_SR set; DESIGN.md §4, "Master-free
// bf16 parameters").  AdamPsrRule names the instances: the third storage mode beside SPLIT and the
// fp32 master.  A segment's `master` is the bf16 parameter, read, widened (exact), run through the
// unchanged fp32 rule and stored in place through p_out with zs_sr::round_bf16 and the low 16 bits
// of zs_sr::bits(e, kp0, kp1), (kp0, kp1) = zs_sr::pkeys(k0, k1) derived on the host; there is no
// master_out and no residual.  The geometry (groups, chunk, alignment) is the split master's, so
// such an instance has SPLIT set.  e counts elements of the m array as ST stores it (fp32 or bf16).
struct PsrHP : SrHP {
  uint32_t kp0, kp1;
};
struct AdamPsrRule : AdamRule<false> {
  using Hyper = PsrHP;
  static constexpr bool kPsr = true;
};
template <typename ST>
__device__ __forceinline__ uint64_t psr_seg_index(const float* m, const PsrHP& hp) {
  return (uint64_t(reinterpret_cast<uintptr_t>(m)) - hp.m_base) >> (sizeof(ST) == 2 ? 1 : 2);
}
// sr_bits_at under the parameter's keys, its low 16 bits: the index's high word stays scalar
__device__ __forceinline__ uint32_t psr_r16_at(uint64_t eu, uint32_t off, const PsrHP& hp) {
  const uint32_t lo0 = uint32_t(eu), hi = uint32_t(eu >> 32);
  const uint32_t lo = lo0 + off;
  const uint32_t ka = hp.kp0 ^ (hi * 0x9E3779B9u), kb = hp.kp0 ^ ((hi + 1u) * 0x9E3779B9u);
  return (zs_sr::lowbias32(lo ^ (lo < lo0 ? kb : ka)) ^ hp.kp1) & 0xFFFFu;
}
// four parameters from index eu + off on as their stochastically rounded bf16 codes, 8 bytes
__device__ __forceinline__ uint2 psr_pack_bf16x4(const float* pp, uint64_t eu, uint32_t off,
                                                 const PsrHP& hp) {
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = sr_word(pp[j], psr_r16_at(eu, off + j, hp));
  return make_uint2(sr_pack2(w[0], w[1]), sr_pack2(w[2], w[3]));
}

// Sharded EMA of the master weights (zs_adamset_run_ema; DESIGN.md §4, "Sharded EMA").  AdamEmaRule
// names the instances: the unchanged amsgrad-free fp32 rule, with the segment's `vmax` column as the
// EMA array -- the stream slot amsgrad uses, so kX is set and elem leaves the value alone.  After the
// storage step the skeleton calls ema(stored, e, hp): e = lerp(e, stored, w), ATen's lerp like
// exp_avg's, where `stored` is the fp32 master as memory now holds it (for the split master the
// re-joined (hi << 16) + sext(lo), 1 ulp off the computed value at an exact tie).  ema_w / ema_hi:
// the fma's coefficient and which operand it adds to, made on the host like lerp_w / lerp_hi.
struct EmaHP : HP {
  float ema_w;
  int ema_hi;
};
struct AdamEmaRule : AdamRule<false> {
  using Hyper = EmaHP;
  static constexpr bool kX = true, kEma = true;
  static __device__ __forceinline__ void ema(float stored, float& e, const EmaHP& hp) {
#pragma clang fp contract(off)
    e = fmaf(hp.ema_w, stored - e, hp.ema_hi ? stored : e);
  }
};

// Per-parameter update and weight norms (zs_adamset_run_stats; DESIGN.md §4, "Per-parameter update
// and weight norms").  AdamStatsRule names the instances: the unchanged amsgrad-free fp32 rule, whose
// bodies keep the master as loaded (p0) and, right after the storage step, add per element
//   d = p1 - p0 (one fp32 subtraction), accd = fmaf(d, d, accd), accw = fmaf(p1, p1, accw)
// with p1 the fp32 master as stored (the split master: the re-joined words, as AdamEmaRule::ema
// sees it).  A lane's two sums cover its elements of one chunk, in the order the body visits them;
// stats_store widens them to double, sums the wave's 64 lanes (block_sum's first stage) and lane 0
// stores the pair with plain stores: one slot per wave per chunk, so the four waves of a workgroup
// stay independent (no LDS, no barrier, no atomics).  The slot of a chunk: off[entry] +
// 4 * (chunk in entry) + wave, off the table's per-entry offsets (vec_off in the vector kernel,
// sca_off in the scalar one); plane 0 (sum d^2) at planes, plane 1 (sum p1^2) nslots doubles on.
struct StatsHP : HP {
  double* planes;
  int64_t nslots;
  const int64_t* vec_off;
  const int64_t* sca_off;
};
struct AdamStatsRule : AdamRule<false> {
  using Hyper = StatsHP;
  using Stats = LaneStats;
  static constexpr bool kStats = true;
  static __device__ __forceinline__ void stat(float p0, float p1, LaneStats& a) {
#pragma clang fp contract(off)
    const float d = p1 - p0;
    a.d = fmaf(d, d, a.d);
    a.w = fmaf(p1, p1, a.w);
  }
};
// The wave's sums of one chunk into its slot (every lane of the wave arrives here).
__device__ __forceinline__ void stats_store(const LaneStats& a, const StatsHP& hp, int64_t slot) {
  double d = double(a.d), w = double(a.w);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    d += __shfl_down(d, o, 64);
    w += __shfl_down(w, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    glob(hp.planes)[slot] = d;
    glob(hp.planes)[hp.nslots + slot] = w;
  }
}

// torch.optim.SGD over the same tables: field `m` of a segment is the momentum buffer (MOM: the
// set has one), `v` and `vmax` are unused.  Without MOM no state array is touched.
struct SgdHP {
  float neg_lr, momentum, omd, wd, grad_div, inv_div, carry_mul;
  int div_pow2, nesterov, maximize, first;
};

template <bool MOM>
struct SgdRule {
  using Hyper = SgdHP;
  static constexpr bool kM = MOM, kV = false, kX = false, kGradOffset2 = false;
  static constexpr bool kPsr = false;
  static constexpr bool kEma = false;
  static constexpr bool kStats = false;
  using Stats = NoStats;

  // One element of torch.optim.SGD's single-tensor update (sgd.py _single_tensor_sgd), in the
  // rounding order of torch's CPU kernels: add(x, alpha=a) = fma(a, x, self), so
  // grad.add(param, alpha=wd) = fma(wd, p, g), buf.mul_(momentum).add_(grad, alpha=1-dampening) =
  // fma(1-dampening, g, buf*momentum), grad.add(buf, alpha=momentum) = fma(momentum, buf, g) and
  // param.add_(grad, alpha=-lr) = fma(-lr, g, p).  Only explicit fmaf() fuse.  `first`: the buffer
  // does not exist yet and becomes the gradient.
  template <bool CARRY, bool CLIP>
  static __device__ __forceinline__ void elem(float gsum, float& p, float& buf, float&, float&,
                                              float& carry, const SgdHP& hp, float coef) {
#pragma clang fp contract(off)
    float g = prep_grad<CARRY, CLIP>(gsum, carry, hp, coef);
    if (hp.wd != 0.0f) g = fmaf(hp.wd, p, g);  // grad.add(param, alpha=wd)
    if constexpr (MOM) {
      buf = hp.first ? g : fmaf(hp.omd, g, buf * hp.momentum);
      g = hp.nesterov ? fmaf(hp.momentum, buf, g) : buf;
    }
    p = fmaf(hp.neg_lr, g, p);
  }
};

// Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") over the same tables:
// field `m` of a segment is exp_avg, the one moment; `v` and `vmax` are unused.  No bias correction,
// so nothing in the struct depends on the step count.  LionSrHP: the keys and m_base of the
// stochastically rounded bf16 momentum ride behind it, as SrHP's behind HP.
struct LionHP {
  float beta1, omb1, beta2, omb2, neg_lr, decay_mul, grad_div, inv_div, carry_mul;
  int div_pow2, maximize;
};
struct LionSrHP : LionHP {
  uint32_t k0, k1;
  uint64_t m_base;
};

template <typename HPT>
struct LionRuleT {
  using Hyper = HPT;
  static constexpr bool kM = true, kV = false, kX = false, kGradOffset2 = false;
  static constexpr bool kPsr = false;
  static constexpr bool kEma = false;
  static constexpr bool kStats = false;
  using Stats = NoStats;

  // One element of zero_amd.optim.Lion's step, in the rounding order of torch's CPU kernels:
  // p.mul_(1 - lr*wd); c = m.mul(b1).add_(g, alpha=1-b1) = fma(1-b1, g, m*b1); u = sign(c) (torch's:
  // +-0 -> +0, NaN -> 0); p.add_(u, alpha=-lr) = fma(-lr, u, p); m.mul_(b2).add_(g, alpha=1-b2) =
  // fma(1-b2, g, m*b2).  Only explicit fmaf() fuse.
  template <bool CARRY, bool CLIP>
  static __device__ __forceinline__ void elem(float gsum, float& p, float& m, float&, float&,
                                              float& carry, const HPT& hp, float coef) {
#pragma clang fp contract(off)
    const float g = prep_grad<CARRY, CLIP>(gsum, carry, hp, coef);
    p = p * hp.decay_mul;
    const float c = fmaf(hp.omb1, g, m * hp.beta1);
    const float u = (c > 0.0f ? 1.0f : 0.0f) - (c < 0.0f ? 1.0f : 0.0f);
    p = fmaf(hp.neg_lr, u, p);
    m = fmaf(hp.omb2, g, m * hp.beta2);
  }
};
template <bool>
using LionRule = LionRuleT<LionHP>;
template <bool>
using LionSrRule = LionRuleT<LionSrHP>;

template <typename GT>
__device__ __forceinline__ float load_g1(const void* g, int64_t i) {
  if constexpr (sizeof(GT) == 4) return glob(static_cast<const float*>(g))[i];
  else return bf16_to_f32(glob(static_cast<const unsigned short*>(g))[i]);
}

// The clip coefficient of a CLIP instance: one uniform load per workgroup (the pointer is a kernel
// argument, the load a scalar one), kept in a scalar register; 1 (unused) otherwise.
template <bool CLIP>
__device__ __forceinline__ float clip_coef(const float* __restrict__ coef_ptr) {
  if constexpr (CLIP) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(*coef_ptr)));
#else
    return *coef_ptr;
#endif
  } else {
    return 1.0f;
  }
}

__device__ __forceinline__ float4 ld4(const float* p, int64_t i) {
  const uint4 r = nt_ld16(p + i);
  return make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z),
                     __uint_as_float(r.w));
}
__device__ __forceinline__ void st4(float* p, int64_t i, float4 x) {
  nt_st16(p + i, make_uint4(__float_as_uint(x.x), __float_as_uint(x.y), __float_as_uint(x.z),
                            __float_as_uint(x.w)));
}

template <typename GT>
__device__ __forceinline__ float4 load_g4(const void* g, int64_t i) {
  if constexpr (sizeof(GT) == 4) {
    return ld4(static_cast<const float*>(g), i);
  } else {
    const uint2 r = nt_ld8(static_cast<const unsigned short*>(g) + i);
    float4 f;
    unpack_bf16x4(r, reinterpret_cast<float*>(&f));
    return f;
  }
}

// A stream of a full chunk is addressed as a uniform base in scalar registers, one 32-bit per-lane
// byte offset shared by all streams of that width, and an immediate: no access has a 64-bit
// address pair of its own in vector registers.  The immediate reaches -4096..4095 bytes, so a
// stream gets the base chunk start + 4096 B (groups at -4096 and 0 for fp32, -4096 .. 2048 for
// bf16) and, for fp32 groups 2 and 3, a second one 8192 B on.
template <typename T>
__device__ __forceinline__ T* lane_ptr(T* base, uint32_t lane_off, int imm) {
  return (T*)((gptr<char>)(char*)base + lane_off + imm);
}
// a pointer the compiler keeps as it is, in scalar registers (or it would fold the bases of a
// stream into one and carry the difference in per-access vector adds)
template <typename T>
__device__ __forceinline__ T* scalar_base(T* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(p));
#endif
  return p;
}
// the bases of one stream of a chunk that starts at p, and group u's access through them
template <typename T, int G>
struct ChunkStream {
  static constexpr int kBytes = int(kThreads * 4 * sizeof(T));  // per group
  static constexpr int kPer = 8192 / kBytes;                    // groups per base
  T* base[(G + kPer - 1) / kPer];
  __device__ __forceinline__ explicit ChunkStream(T* p) {
#pragma unroll
    for (int k = 0; k < (G + kPer - 1) / kPer; ++k)
      base[k] = scalar_base(reinterpret_cast<T*>((char*)p + 4096 + 8192 * k));
  }
  __device__ __forceinline__ T* at(int u, uint32_t lane_off) const {
    return lane_ptr(base[u / kPer], lane_off, (u % kPer) * kBytes - 4096);
  }
};
// in the place of a stream that a rule does not have (SGD: v, vmax): no bases, no registers
struct NoStream {
  __device__ __forceinline__ explicit NoStream(const void*) {}
};

// One full chunk [e0, e0 + adam_chunk) of a segment, no per-lane predicate; HASG (the segment has a
// gradient) is resolved by the caller, once per chunk.  First loop: every load of the chunk (g,
// hi/lo or master, m, v, vmax, carry; 20 for the split-master Adam's G = 4) goes into raw registers
// before anything depends on one.  Second loop: unpack, the rule's elem and the stores, group by
// group.  ST: the element type of m and v in memory, float or unsigned short (bf16 moments: 8 bytes
// per lane per access through the 16-bit streams, widened before the rule and rounded to nearest
// even after it — SrBf16: stochastically, sr_pack_bf16x4; the rule itself and the parameter it
// leaves see fp32 moments only).  Rule::kPsr (AdamPsrRule, with SPLIT): the parameter is the one
// 16-bit stream `hi` / `pb`, read, widened and stored back through psr_pack_bf16x4; no `lo`.
template <typename Rule, typename GT, bool CARRY, bool SPLIT, bool HASG, bool CLIP,
          typename ST = float>
__device__ __forceinline__ void update_full_chunk(const AdamSeg& s, int64_t e0,
                                                  const typename Rule::Hyper& hp, float coef,
                                                  typename Rule::Stats& acc) {
  constexpr int G = adam_groups(SPLIT);
  constexpr bool G32 = sizeof(GT) == 4;
  constexpr bool S16 = sizeof(ST) == 2;
  constexpr bool PSR = Rule::kPsr;
  static_assert(!S16 || (Rule::kM && !Rule::kX && !CARRY),
                "bf16 state: m (and Adam's v), no amsgrad, no carry");
  static_assert(!PSR || (SPLIT && !Rule::kX && !CARRY),
                "master-free: the split master's geometry, no amsgrad, no carry");
  uint32_t o4 = threadIdx.x * 16u;                   // lane byte offset in an fp32 stream
  uint32_t o2 = threadIdx.x * 8u;                    // ... in a bf16 stream
#if defined(__HIP_DEVICE_COMPILE__)
  // Opaque per chunk: hoisted out of the chunk loop, the offsets' zero-extensions would end up in
  // another block than the accesses, which then fall back to a 64-bit vector address each.
  asm volatile("" : "+v"(o4), "+v"(o2));
#endif
  typedef ChunkStream<float, G> S4;
  typedef ChunkStream<unsigned short, G> S2;
  typedef std::conditional_t<Rule::kV && !S16, S4, NoStream> SV;  // v and its running maximum vmax
  typedef std::conditional_t<S16, NoStream, S4> SM;                // m as fp32
  typedef std::conditional_t<S16, S2, NoStream> SH;                // m as bf16
  typedef std::conditional_t<S16 && Rule::kV, S2, NoStream> SHV;   // v as bf16 (Lion: none)
  const S4 gf(HASG && G32 ? (float*)s.g + e0 : nullptr), pm(SPLIT ? nullptr : (float*)s.master + e0);
  const S4 po(SPLIT ? nullptr : s.master_out + e0);
  const SM sm(Rule::kM ? s.m + e0 : nullptr);
  const SV sv(s.v + e0), sx(Rule::kX ? s.vmax + e0 : nullptr);
  const S4 sc(CARRY ? s.carry + e0 : nullptr);
  const S2 gh(HASG && !G32 ? (unsigned short*)s.g + e0 : nullptr);
  const S2 hi(SPLIT ? (unsigned short*)s.master + e0 : nullptr);
  const S2 lo(SPLIT && !PSR ? (unsigned short*)s.master_out + e0 : nullptr), pb(s.p_out + e0);
  const SH mh((unsigned short*)s.m + e0);
  const SHV vh((unsigned short*)s.v + e0);
  uint4 gq[G], pq[G], mq[G], vq[G], xq[G], cq[G];
  uint2 gd[G], hd[G], ld[G], md[G], vd[G];
  // kGradOffset2 (Adam), fp32 gradients over the split master (G = 4): the gradient's groups 2 and
  // 3 through the first base and a second lane offset 8 KiB on — one vector register instead of a
  // second pair of scalar ones, which this instance (five fp32 streams of two bases each under
  // amsgrad) has not
  constexpr bool GOFF2 = Rule::kGradOffset2 && HASG && G32 && SPLIT;
  uint32_t o4g = o4 + 8192u;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (GOFF2) asm volatile("" : "+v"(o4g));
#endif
#pragma unroll
  for (int u = 0; u < G; ++u) {
    if constexpr (HASG) {
      if constexpr (GOFF2)
        gq[u] = nt_ld16(u < S4::kPer ? gf.at(u, o4)
                                     : lane_ptr(gf.base[0], o4g, (u % S4::kPer) * S4::kBytes - 4096));
      else if constexpr (G32) gq[u] = nt_ld16(gf.at(u, o4));
      else gd[u] = nt_ld8(gh.at(u, o2));
    }
    if constexpr (SPLIT) {
      hd[u] = nt_ld8(hi.at(u, o2));
      if constexpr (!PSR) ld[u] = nt_ld8(lo.at(u, o2));
    } else {
      pq[u] = nt_ld16(pm.at(u, o4));
    }
    if constexpr (S16) {
      md[u] = nt_ld8(mh.at(u, o2));
      if constexpr (Rule::kV) vd[u] = nt_ld8(vh.at(u, o2));
    } else {
      if constexpr (Rule::kM) mq[u] = nt_ld16(sm.at(u, o4));
      if constexpr (Rule::kV) vq[u] = nt_ld16(sv.at(u, o4));
    }
    if constexpr (Rule::kX) xq[u] = nt_ld16(sx.at(u, o4));
    if constexpr (CARRY) cq[u] = nt_ld16(sc.at(u, o4));
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    float gp[4] = {0.f, 0.f, 0.f, 0.f}, pp[4];
    if constexpr (HASG && G32) unpack4(gq[u], gp);
    else if constexpr (HASG) unpack_bf16x4(gd[u], gp);
    if constexpr (PSR) unpack_bf16x4(hd[u], pp);
    else if constexpr (SPLIT) join_master4(hd[u], ld[u], pp);
    else unpack4(pq[u], pp);
    float mp[4] = {0.f, 0.f, 0.f, 0.f}, vp[4] = {0.f, 0.f, 0.f, 0.f};
    float xp[4] = {0.f, 0.f, 0.f, 0.f}, cp[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (S16) {
      unpack_bf16x4(md[u], mp);
      if constexpr (Rule::kV) unpack_bf16x4(vd[u], vp);
    } else {
      if constexpr (Rule::kM) unpack4(mq[u], mp);
      if constexpr (Rule::kV) unpack4(vq[u], vp);
    }
    if constexpr (Rule::kX) unpack4(xq[u], xp);
    if constexpr (CARRY) unpack4(cq[u], cp);
    float p0[4] = {0.f, 0.f, 0.f, 0.f};  // the master as loaded (kStats)
    if constexpr (Rule::kStats) {
#pragma unroll
      for (int j = 0; j < 4; ++j) p0[j] = pp[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      Rule::template elem<CARRY, CLIP>(gp[j], pp[j], mp[j], vp[j], xp[j], cp[j], hp, coef);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(o4), "+v"(o2));  // as above, for the block the stores are in
#endif
    if constexpr (PSR) {
      const uint2 r = psr_pack_bf16x4(pp, psr_seg_index<ST>(s.m, hp) + uint64_t(e0),
                                      (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp);
      nt_st8(pb.at(u, o2), r);
    } else if constexpr (SPLIT) {
      uint32_t h[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // split_master4, in place: through the call 16 instances
        h[j] = f32_to_bf16(pp[j]);   // of this body schedule differently
        l[j] = master_residual(pp[j], h[j]);
      }
      nt_st8(pb.at(u, o2), pack_u16x4(h));
      nt_st8(lo.at(u, o2), pack_u16x4(l));
      if constexpr (Rule::kEma) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Rule::ema(join_master(h[j], l[j]), xp[j], hp);
      }
      if constexpr (Rule::kStats) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Rule::stat(p0[j], join_master(h[j], l[j]), acc);
      }
    } else {
      if (s.master_out) nt_st16(po.at(u, o4), pack4(pp));
      if (s.p_out) {
        const uint2 r = pack_bf16x4(pp);
        nt_st8(pb.at(u, o2), r);
      }
      if constexpr (Rule::kEma) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Rule::ema(pp[j], xp[j], hp);
      }
      if constexpr (Rule::kStats) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Rule::stat(p0[j], pp[j], acc);
      }
    }
    if constexpr (S16 && !Rule::kV) {  // a 16-bit m alone (Lion): no v stream at all
      uint2 mr;
      if constexpr (kStochastic<ST>)
        mr = sr_pack_m_bf16x4(mp, sr_seg_index(s.m, hp) + uint64_t(e0),
                              (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp);
      else
        mr = pack_bf16x4(mp);
      nt_st8(mh.at(u, o2), mr);
    } else if constexpr (kStochastic<ST>) {
      uint2 mr, vr;
      // (one uniform index per chunk: the group's offset rides in the lane's part, an immediate)
      sr_pack_bf16x4(mp, vp, sr_seg_index(s.m, hp) + uint64_t(e0),
                     (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp, mr, vr);
      nt_st8(mh.at(u, o2), mr);
      nt_st8(vh.at(u, o2), vr);
    } else if constexpr (S16) {
      const uint2 mr = pack_bf16x4(mp), vr = pack_bf16x4(vp);
      nt_st8(mh.at(u, o2), mr);
      nt_st8(vh.at(u, o2), vr);
    } else {
      if constexpr (Rule::kM) nt_st16(sm.at(u, o4), pack4(mp));
      if constexpr (Rule::kV) nt_st16(sv.at(u, o4), pack4(vp));
    }
    if constexpr (Rule::kX) nt_st16(sx.at(u, o4), pack4(xp));
    if constexpr (CARRY) nt_st16(sc.at(u, o4), pack4(cp));
  }
}

// The per-lane predicated body: G float4 groups from element e0 of a segment, each group under its
// own `i < s.n`.  The branches keep each group's loads and their waits in a block of their own, so
// a wave has one group's loads in flight at a time.  ST as in update_full_chunk.
template <typename Rule, typename GT, bool CARRY, bool SPLIT, int G, bool CLIP,
          typename ST = float>
__device__ __forceinline__ void update_pred_groups(const AdamSeg& s, int64_t e0,
                                                   const typename Rule::Hyper& hp, float coef,
                                                   typename Rule::Stats& acc) {
  constexpr bool S16 = sizeof(ST) == 2;
  constexpr bool PSR = Rule::kPsr;
  static_assert(!S16 || (Rule::kM && !Rule::kX && !CARRY),
                "bf16 state: m (and Adam's v), no amsgrad, no carry");
  static_assert(!PSR || (SPLIT && !Rule::kX && !CARRY),
                "master-free: the split master's geometry, no amsgrad, no carry");
  float4 g4[G], p4[G], m4[G], v4[G];
  float4 x4[G], c4[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    const int64_t i = e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
    if (i < s.n) {
      g4[u] = s.g ? load_g4<GT>(s.g, i) : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (PSR) {
        const uint2 h = nt_ld8(reinterpret_cast<const unsigned short*>(s.master) + i);
        unpack_bf16x4(h, reinterpret_cast<float*>(&p4[u]));
      } else if constexpr (SPLIT) {
        const uint2 h = nt_ld8(reinterpret_cast<const unsigned short*>(s.master) + i);
        const uint2 l = nt_ld8(reinterpret_cast<const unsigned short*>(s.master_out) + i);
        join_master4(h, l, reinterpret_cast<float*>(&p4[u]));
      } else {
        p4[u] = ld4(s.master, i);
      }
      if constexpr (S16) {
        const uint2 mr = nt_ld8(reinterpret_cast<const unsigned short*>(s.m) + i);
        if constexpr (Rule::kV) {
          const uint2 vr = nt_ld8(reinterpret_cast<const unsigned short*>(s.v) + i);
          unpack_bf16x4(mr, reinterpret_cast<float*>(&m4[u]));
          unpack_bf16x4(vr, reinterpret_cast<float*>(&v4[u]));
        } else {  // a 16-bit m alone (Lion)
          unpack_bf16x4(mr, reinterpret_cast<float*>(&m4[u]));
        }
      } else {
        if constexpr (Rule::kM) m4[u] = ld4(s.m, i);
        if constexpr (Rule::kV) v4[u] = ld4(s.v, i);
      }
      if constexpr (Rule::kX) x4[u] = ld4(s.vmax, i);
      if constexpr (CARRY) c4[u] = ld4(s.carry, i);
    }
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    const int64_t i = e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
    if (i < s.n) {
      float* gp = reinterpret_cast<float*>(&g4[u]);
      float* pp = reinterpret_cast<float*>(&p4[u]);
      float* mp = reinterpret_cast<float*>(&m4[u]);
      float* vp = reinterpret_cast<float*>(&v4[u]);
      float* xp = reinterpret_cast<float*>(&x4[u]);
      float* cp = reinterpret_cast<float*>(&c4[u]);
      float p0[4] = {0.f, 0.f, 0.f, 0.f};  // the master as loaded (kStats)
      if constexpr (Rule::kStats) {
#pragma unroll
        for (int j = 0; j < 4; ++j) p0[j] = pp[j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mv = Rule::kM ? mp[j] : 0.0f;
        float vv = Rule::kV ? vp[j] : 0.0f;
        float xv = Rule::kX ? xp[j] : 0.0f;
        float cv = CARRY ? cp[j] : 0.0f;
        Rule::template elem<CARRY, CLIP>(gp[j], pp[j], mv, vv, xv, cv, hp, coef);
        if constexpr (Rule::kM) mp[j] = mv;
        if constexpr (Rule::kV) vp[j] = vv;
        if constexpr (Rule::kX) xp[j] = xv;
        if constexpr (CARRY) cp[j] = cv;
      }
      if constexpr (PSR) {
        const uint2 r = psr_pack_bf16x4(pp, psr_seg_index<ST>(s.m, hp) + uint64_t(e0),
                                        (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp);
        nt_st8(s.p_out + i, r);
      } else if constexpr (SPLIT) {
        uint32_t h[4], l[4];
        split_master4(pp, h, l);
        nt_st8(s.p_out + i, pack_u16x4(h));
        nt_st8(reinterpret_cast<unsigned short*>(s.master_out) + i, pack_u16x4(l));
        if constexpr (Rule::kEma) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Rule::ema(join_master(h[j], l[j]), xp[j], hp);
        }
        if constexpr (Rule::kStats) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Rule::stat(p0[j], join_master(h[j], l[j]), acc);
        }
      } else {
        if (s.master_out) st4(s.master_out, i, p4[u]);
        if (s.p_out) {
          const uint2 r = pack_bf16x4(pp);
          nt_st8(s.p_out + i, r);
        }
        if constexpr (Rule::kEma) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Rule::ema(pp[j], xp[j], hp);
        }
        if constexpr (Rule::kStats) {
#pragma unroll
          for (int j = 0; j < 4; ++j) Rule::stat(p0[j], pp[j], acc);
        }
      }
      if constexpr (S16 && !Rule::kV) {  // a 16-bit m alone (Lion)
        uint2 mr;
        if constexpr (kStochastic<ST>)
          mr = sr_pack_m_bf16x4(mp, sr_seg_index(s.m, hp) + uint64_t(e0),
                                (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp);
        else
          mr = pack_bf16x4(mp);
        nt_st8(reinterpret_cast<unsigned short*>(s.m) + i, mr);
      } else if constexpr (kStochastic<ST>) {
        uint2 mr, vr;
        sr_pack_bf16x4(mp, vp, sr_seg_index(s.m, hp) + uint64_t(e0),
                       (uint32_t(u) * kThreads + threadIdx.x) * 4u, hp, mr, vr);
        nt_st8(reinterpret_cast<unsigned short*>(s.m) + i, mr);
        nt_st8(reinterpret_cast<unsigned short*>(s.v) + i, vr);
      } else if constexpr (S16) {
        const uint2 mr = pack_bf16x4(mp), vr = pack_bf16x4(vp);
        nt_st8(reinterpret_cast<unsigned short*>(s.m) + i, mr);
        nt_st8(reinterpret_cast<unsigned short*>(s.v) + i, vr);
      } else {
        if constexpr (Rule::kM) st4(s.m, i, m4[u]);
        if constexpr (Rule::kV) st4(s.v, i, v4[u]);
      }
      if constexpr (Rule::kX) st4(s.vmax, i, x4[u]);
      if constexpr (CARRY) st4(s.carry, i, c4[u]);
    }
  }
}

// The kernels: one vector and one scalar kernel, instantiated per element rule.  The chunk loop, the
// routing of a chunk and the scalar body stand in the kernel itself and not in a function: behind a
// function of their own they compile to other code than they did (the return block moves and with
// it what the loop hoists, and sinking stops at the call), and `make asm` must show the kernels
// unchanged.  A kernel template over the rule is the same text instantiated per rule, so one text
// serves Adam, Adam with stochastically rounded bf16 moments and SGD.  Both keep the name they had
// when Adam was the only rule (the roofline label, the profiles and the ABI test key on it), so an
// SGD launch shows under a profiler as adam_segments_kernel<SgdRule<true>, ...> -- like AdamSeg and
// zs_adamset, which carry SGD sets too.  CLIP instances exist without the carry only.
// GUARD (zs_adamset_run_guarded, zs_adamset_run_sr_guarded; with CLIP, the Adam families): a NaN
// coefficient -- zs_clip_coef_guarded's mark of a non-finite gradient norm -- ends the workgroup
// right after the coefficient's scalar load, so the skipped step changes nothing in memory.  The
// coefficient is uniform (clip_coef's readfirstlane): one scalar compare and branch.
//
// Vector kernel: every segment 16-B aligned (8-B for bf16 arrays) with n % 4 == 0 (the host
// splits tails off into the scalar table).  adam_groups() float4 groups per thread, lane-contiguous
// (16 B per lane per access), so each wave instruction touches one contiguous 1 KiB (f32) /
// 512 B (bf16) run.  LOADS_FIRST (the default): a full chunk, all but the last of a segment, goes
// through update_full_chunk and the partial one through the predicated body a group at a time (it
// is one chunk per segment, and a group at a time it stays out of the kernel's register budget).
// !LOADS_FIRST (`zs_tune("adam_loads_first", 0)`): every chunk through the predicated body, all
// groups unrolled -- the kernel as it was before update_full_chunk, kept for A/B runs.
// ST = unsigned short (zs_adamset_create_ex with ZS_BF16 state): m and v are bf16 arrays, 8-B
// aligned like the other 16-bit ones; the chunk geometry is the fp32-state instance's.  ST = SrBf16
// (zs_adamset_run_sr, over AdamSrRule, whose Hyper carries the keys and m_base): the same arrays,
// stored with stochastic rounding.  Rule = AdamPsrRule (zs_adamset_run_psr, a ZS_BF16_SR set;
// SPLIT names its geometry): no master, the bf16 parameter in place, any of the three ST.
// Rule = AdamEmaRule (zs_adamset_run_ema; fp32 moments, no carry): the vmax stream is an EMA of the
// master, moved by Rule::ema right after the storage step of each body, on the value as stored.
// Rule = AdamStatsRule (zs_adamset_run_stats; fp32 moments, no carry): each body also adds the
// element's (stored - loaded)^2 and stored^2 to the lane's Rule::Stats, which stats_store sums per
// wave into the chunk's slots once the chunk is done.
template <typename Rule, typename GT, bool CARRY, bool SPLIT, bool LOADS_FIRST, bool CLIP,
          typename ST = float, bool GUARD = false>
__global__ __launch_bounds__(kThreads) void adam_segments_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, typename Rule::Hyper hp, const float* __restrict__ coef_ptr) {
  static_assert(!(CLIP && CARRY), "the clip coefficient is not defined under the ZeRO-1 carry");
  static_assert(CLIP || !GUARD, "the guard tests the clip coefficient");
  const float coef = clip_coef<CLIP>(coef_ptr);
  if constexpr (GUARD) {
    if (coef != coef) return;  // uniform: the step is skipped, nothing is loaded or stored
  }
  int64_t seg = 0;
  if constexpr (LOADS_FIRST) {
    int64_t hi = nseg;
    while (hi - seg > 1) {
      const int64_t mid = (seg + hi) >> 1;
      if (chunk_prefix[mid] <= int64_t(blockIdx.x)) seg = mid;
      else hi = mid;
    }
  }
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const AdamSeg s = segs[seg];
    constexpr int G = adam_groups(SPLIT);
    const int64_t e0 = (c - chunk_prefix[seg]) * adam_chunk(SPLIT);
    typename Rule::Stats acc;  // kStats: this lane's sums over the chunk, +0 at its start
    if constexpr (LOADS_FIRST) {
      if (e0 + adam_chunk(SPLIT) <= s.n) {  // uniform per workgroup
        if (s.g) update_full_chunk<Rule, GT, CARRY, SPLIT, true, CLIP, ST>(s, e0, hp, coef, acc);
        else update_full_chunk<Rule, GT, CARRY, SPLIT, false, CLIP, ST>(s, e0, hp, coef, acc);
      } else {
#pragma unroll 1
        for (int u = 0; u < G && e0 + int64_t(u) * kThreads * 4 < s.n; ++u)
          update_pred_groups<Rule, GT, CARRY, SPLIT, 1, CLIP, ST>(
              s, e0 + int64_t(u) * kThreads * 4, hp, coef, acc);
      }
    } else {
      update_pred_groups<Rule, GT, CARRY, SPLIT, G, CLIP, ST>(s, e0, hp, coef, acc);
    }
    if constexpr (Rule::kStats)
      stats_store(acc, hp, hp.vec_off[seg] + 4 * (c - chunk_prefix[seg]) + (threadIdx.x >> 6));
  }
}

// Scalar kernel: one element per lane, 256-element chunks.  m and v as ST stores them: stochastic
// (one draw for both, the chunk's uniform index i0 plus the lane), bf16 to nearest, or the rule's
// own fp32 arrays.
template <typename Rule, typename GT, bool CARRY, bool SPLIT, bool CLIP, typename ST = float,
          bool GUARD = false>
__global__ __launch_bounds__(kThreads) void adam_scalar_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, typename Rule::Hyper hp, const float* __restrict__ coef_ptr) {
  static_assert(!(CLIP && CARRY), "the clip coefficient is not defined under the ZeRO-1 carry");
  static_assert(CLIP || !GUARD, "the guard tests the clip coefficient");
  const float coef = clip_coef<CLIP>(coef_ptr);
  if constexpr (GUARD) {
    if (coef != coef) return;  // uniform: the step is skipped, nothing is loaded or stored
  }
  constexpr bool S16 = sizeof(ST) == 2;
  constexpr bool PSR = Rule::kPsr;
  static_assert(!S16 || (Rule::kM && !Rule::kX && !CARRY),
                "bf16 state: m (and Adam's v), no amsgrad, no carry");
  static_assert(!PSR || (SPLIT && !Rule::kX && !CARRY),
                "master-free: the split master's geometry, no amsgrad, no carry");
  int64_t seg = 0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const AdamSeg s = segs[seg];
    const int64_t i0 = (c - chunk_prefix[seg]) * kThreads;  // uniform
    const int64_t i = i0 + threadIdx.x;
    typename Rule::Stats acc;  // kStats: a lane past n adds nothing and still joins the wave's sum
    if (i < s.n) {
      float gs = s.g ? load_g1<GT>(s.g, i) : 0.0f;
      const gptr<unsigned short> lo = glob(reinterpret_cast<unsigned short*>(s.master_out));
      float p;
      if constexpr (PSR)
        p = bf16_to_f32(glob(reinterpret_cast<const unsigned short*>(s.master))[i]);
      else
        p = SPLIT ? join_master(glob(reinterpret_cast<const unsigned short*>(s.master))[i], lo[i])
                  : glob(s.master)[i];
      const gptr<unsigned short> mb = glob(reinterpret_cast<unsigned short*>(s.m));
      const gptr<unsigned short> vb = glob(reinterpret_cast<unsigned short*>(s.v));
      float m = 0.0f, v = 0.0f, vm = 0.0f;
      if constexpr (S16) {
        m = bf16_to_f32(mb[i]);
        if constexpr (Rule::kV) v = bf16_to_f32(vb[i]);
      } else {
        if constexpr (Rule::kM) m = glob(s.m)[i];
        if constexpr (Rule::kV) v = glob(s.v)[i];
      }
      if constexpr (Rule::kX) vm = glob(s.vmax)[i];
      float cr = CARRY ? glob(s.carry)[i] : 0.0f;
      const float p0 = p;  // the master as loaded (kStats)
      Rule::template elem<CARRY, CLIP>(gs, p, m, v, vm, cr, hp, coef);
      if constexpr (PSR) {
        const uint32_t r16 = psr_r16_at(psr_seg_index<ST>(s.m, hp) + uint64_t(i0), threadIdx.x, hp);
        glob(s.p_out)[i] = (unsigned short)(sr_word(p, r16) >> 16);
      } else if constexpr (SPLIT) {
        const unsigned short h = f32_to_bf16(p);
        glob(s.p_out)[i] = h;
        const uint32_t l = master_residual(p, h);
        lo[i] = (unsigned short)l;
        if constexpr (Rule::kEma) Rule::ema(join_master(h, l), vm, hp);
        if constexpr (Rule::kStats) Rule::stat(p0, join_master(h, l), acc);
      } else {
        if (s.master_out) glob(s.master_out)[i] = p;
        if (s.p_out) glob(s.p_out)[i] = f32_to_bf16(p);
        if constexpr (Rule::kEma) Rule::ema(p, vm, hp);
        if constexpr (Rule::kStats) Rule::stat(p0, p, acc);
      }
      if constexpr (S16 && !Rule::kV) {  // a 16-bit m alone (Lion)
        if constexpr (kStochastic<ST>) {
          const uint32_t r = sr_bits_at(sr_seg_index(s.m, hp) + uint64_t(i0), threadIdx.x, hp);
          mb[i] = (unsigned short)(sr_word(m, r & 0xFFFFu) >> 16);
        } else {
          mb[i] = f32_to_bf16(m);
        }
      } else if constexpr (kStochastic<ST>) {
        uint32_t mh, vh;
        sr_narrow(m, v, sr_bits_at(sr_seg_index(s.m, hp) + uint64_t(i0), threadIdx.x, hp), mh, vh);
        mb[i] = (unsigned short)(mh >> 16);
        vb[i] = (unsigned short)(vh >> 16);
      } else if constexpr (S16) {
        mb[i] = f32_to_bf16(m);
        vb[i] = f32_to_bf16(v);
      } else {
        if constexpr (Rule::kM) glob(s.m)[i] = m;
        if constexpr (Rule::kV) glob(s.v)[i] = v;
      }
      if constexpr (Rule::kX) glob(s.vmax)[i] = vm;
      if constexpr (CARRY) glob(s.carry)[i] = cr;
    }
    if constexpr (Rule::kStats)
      stats_store(acc, hp, hp.sca_off[seg] + 4 * (c - chunk_prefix[seg]) + (threadIdx.x >> 6));
  }
}

// ----------------------------------------------------------------------------------------------
// gradient sum of squares over an Adam set (global-norm clipping, clip_grad_norm_'s norm)
// ----------------------------------------------------------------------------------------------
// One read-only pass over the gradients a set is bound to, driven by the set's own tables: the
// vector table in the Adam's chunks (16 B fp32 / 8 B bf16 per lane per access, all of a chunk's
// loads before its first use), the scalar table in 256-element chunks.  fp32 arithmetic covers one
// lane's terms of one chunk (fmaf(g, g, acc): 4 * adam_groups() terms, 16 for a split-master set
// and 8 otherwise; 1 in the scalar table); everything above is double: a lane's total over its
// chunks, the wave (shuffles), the 4 waves (LDS) and one partial per workgroup, a plain store.  No
// atomics.  The grid is the number of partials, fixed when the set is created: min(chunks, cap)
// per table, workgroup b summing chunks b, b + grid, ... — neither zs_tune nor the device enters,
// so the sum has the same bits on every run.
constexpr int64_t kSqnormVecPartials = 8192, kSqnormScaPartials = 1024;

// Sum over the workgroup in a fixed order; the result is valid in every thread.
__device__ __forceinline__ double block_sum(double x) {
  __shared__ double wave_sum[kThreads / 64];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// NT: the loads' cache policy (zs_tune "sqnorm_nt")
template <typename GT, bool SPLIT, bool NT>
__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, double* __restrict__ partials) {
  constexpr int G = adam_groups(SPLIT);
  constexpr bool G32 = sizeof(GT) == 4;
  int64_t seg = 0, hi = nseg;
  while (hi - seg > 1) {  // the segment of the first chunk, as adam_segments_kernel
    const int64_t mid = (seg + hi) >> 1;
    if (chunk_prefix[mid] <= int64_t(blockIdx.x)) seg = mid;
    else hi = mid;
  }
  double total = 0.0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const GT* g = static_cast<const GT*>(segs[seg].g);
    const int64_t n = segs[seg].n;
    if (!g) continue;  // no gradient: nothing read (uniform per workgroup)
    const int64_t e0 = (c - chunk_prefix[seg]) * adam_chunk(SPLIT);
    uint4 r[G];  // bf16: x, y hold the four elements
    if (e0 + adam_chunk(SPLIT) <= n) {
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const GT* p = g + e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
        if constexpr (G32) {
          r[u] = ld16<NT>(p);
        } else {
          const uint2 d = ld8<NT>(p);
          r[u] = make_uint4(d.x, d.y, 0u, 0u);
        }
      }
    } else {  // the segment's last chunk: groups past n contribute +0
#pragma unroll
      for (int u = 0; u < G; ++u) {
        const int64_t i = e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
        r[u] = make_uint4(0u, 0u, 0u, 0u);
        if (i < n) {
          if constexpr (G32) {
            r[u] = ld16<NT>(g + i);
          } else {
            const uint2 d = ld8<NT>(g + i);
            r[u] = make_uint4(d.x, d.y, 0u, 0u);
          }
        }
      }
    }
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < G; ++u) {
      float x[4];
      if constexpr (G32) unpack4(r[u], x);
      else unpack_bf16x4(make_uint2(r[u].x, r[u].y), x);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(x[j], x[j], acc);
    }
    total += double(acc);
  }
  const double b = block_sum(total);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

template <typename GT>
__global__ __launch_bounds__(kThreads) void grad_sqnorm_scalar_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, double* __restrict__ partials) {
  int64_t seg = 0;
  double total = 0.0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const void* g = segs[seg].g;
    const int64_t n = segs[seg].n;
    if (!g) continue;
    const int64_t i = (c - chunk_prefix[seg]) * kThreads + threadIdx.x;
    if (i < n) {
      const float x = load_g1<GT>(g, i);
      total += double(fmaf(x, x, 0.0f));
    }
  }
  const double b = block_sum(total);
  if (threadIdx.x == 0) partials[blockIdx.x] = b;
}

// n double partials -> the fp32 rounding of their double sum: one workgroup, thread t summing
// partials t, t + 256, ... in order, then block_sum.
__global__ __launch_bounds__(kThreads) void sqnorm_reduce_kernel(
    const double* __restrict__ partials, int64_t n, float* __restrict__ sumsq) {
  double t = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) t += partials[i];
  const double b = block_sum(t);
  if (threadIdx.x == 0) *sumsq = float(b);
}

// ----------------------------------------------------------------------------------------------
// the same pass keyed by segment (per-parameter gradient norms)
// ----------------------------------------------------------------------------------------------
// grad_sqnorm_kernel's reads and arithmetic with another reduction shape: a table entry (the vector
// or the scalar part of one input segment) has slots = min(its chunks, cap) partials of its own,
// and the workgroup of slot j sums chunks j, j + slots, ... of that entry alone.  slot_prefix
// (entries + 1) maps a workgroup to (entry, j); slot_out[entry] is where the entry's slots start
// in the set's partials (input order; a segment's vector part, then its scalar part).  An entry's
// slot count and every slot's value depend on that segment alone: neither its neighbours, the
// device nor zs_tune enter.  An entry without a gradient is not read: its slots get +0.0.
constexpr int64_t kSqnormSegVecSlots = 128, kSqnormSegScaSlots = 16;

// grad_sqnorm_kernel's chunk body (kept apart from it, so that the instances of that kernel stay
// the parent's instruction for instruction): one lane's fp32 sum of squares over the chunk at
// element e0 of a vector-table segment (g, n) — all of the chunk's loads, then fmaf(x, x, acc) over
// its 4 * adam_groups() terms; groups past n contribute +0.  NT: the loads' cache policy
template <typename GT, bool SPLIT, bool NT>
__device__ __forceinline__ float chunk_sumsq(const GT* __restrict__ g, int64_t n, int64_t e0) {
  constexpr int G = adam_groups(SPLIT);
  constexpr bool G32 = sizeof(GT) == 4;
  uint4 r[G];  // bf16: x, y hold the four elements
  if (e0 + adam_chunk(SPLIT) <= n) {
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const GT* p = g + e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
      if constexpr (G32) {
        r[u] = ld16<NT>(p);
      } else {
        const uint2 d = ld8<NT>(p);
        r[u] = make_uint4(d.x, d.y, 0u, 0u);
      }
    }
  } else {  // the segment's last chunk: groups past n contribute +0
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int64_t i = e0 + (int64_t(u) * kThreads + threadIdx.x) * 4;
      r[u] = make_uint4(0u, 0u, 0u, 0u);
      if (i < n) {
        if constexpr (G32) {
          r[u] = ld16<NT>(g + i);
        } else {
          const uint2 d = ld8<NT>(g + i);
          r[u] = make_uint4(d.x, d.y, 0u, 0u);
        }
      }
    }
  }
  float acc = 0.0f;
#pragma unroll
  for (int u = 0; u < G; ++u) {
    float x[4];
    if constexpr (G32) unpack4(r[u], x);
    else unpack_bf16x4(make_uint2(r[u].x, r[u].y), x);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(x[j], x[j], acc);
  }
  return acc;
}

// the entry of workgroup b: slot_prefix[entry] <= b < slot_prefix[entry + 1]
__device__ __forceinline__ int64_t slot_entry(const int64_t* __restrict__ slot_prefix,
                                              int64_t nent, int64_t b) {
  int64_t e = 0, hi = nent;
  while (hi - e > 1) {
    const int64_t mid = (e + hi) >> 1;
    if (slot_prefix[mid] <= b) e = mid;
    else hi = mid;
  }
  return e;
}

template <typename GT, bool SPLIT, bool NT>
__global__ __launch_bounds__(kThreads) void grad_sqnorm_segs_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ slot_prefix,
    const int64_t* __restrict__ slot_out, int64_t nent, double* __restrict__ partials) {
  const int64_t e = slot_entry(slot_prefix, nent, blockIdx.x);
  const int64_t j = int64_t(blockIdx.x) - slot_prefix[e];
  const int64_t slots = slot_prefix[e + 1] - slot_prefix[e];
  const GT* g = static_cast<const GT*>(segs[e].g);
  const int64_t n = segs[e].n;
  double total = 0.0;
  if (g) {  // (uniform per workgroup)
    const int64_t chunks = (n + adam_chunk(SPLIT) - 1) / adam_chunk(SPLIT);
    for (int64_t c = j; c < chunks; c += slots)
      total += double(chunk_sumsq<GT, SPLIT, NT>(g, n, c * adam_chunk(SPLIT)));
  }
  const double b = block_sum(total);
  if (threadIdx.x == 0) partials[slot_out[e] + j] = b;
}

template <typename GT>
__global__ __launch_bounds__(kThreads) void grad_sqnorm_segs_scalar_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ slot_prefix,
    const int64_t* __restrict__ slot_out, int64_t nent, double* __restrict__ partials) {
  const int64_t e = slot_entry(slot_prefix, nent, blockIdx.x);
  const int64_t j = int64_t(blockIdx.x) - slot_prefix[e];
  const int64_t slots = slot_prefix[e + 1] - slot_prefix[e];
  const void* g = segs[e].g;
  const int64_t n = segs[e].n;
  double total = 0.0;
  if (g) {
    const int64_t chunks = (n + kThreads - 1) / kThreads;
    for (int64_t c = j; c < chunks; c += slots) {
      const int64_t i = c * kThreads + threadIdx.x;
      if (i < n) {
        const float x = load_g1<GT>(g, i);
        total += double(fmaf(x, x, 0.0f));
      }
    }
  }
  const double b = block_sum(total);
  if (threadIdx.x == 0) partials[slot_out[e] + j] = b;
}

// Per-parameter sums over a CSR of slot ranges: workgroup i adds parameter i's ranges
// row_ptr[i] .. row_ptr[i + 1] in that order, thread t taking slots t, t + 256, ... of each range
// into one running double, then block_sum; out[i] is the fp32 rounding.  No range: +0.0.
__global__ __launch_bounds__(kThreads) void sqnorm_reduce_params_kernel(
    const double* __restrict__ partials, const int64_t* __restrict__ row_ptr,
    const int64_t* __restrict__ slot_lo, const int64_t* __restrict__ slot_n,
    float* __restrict__ out) {
  double t = 0.0;
  for (int64_t r = row_ptr[blockIdx.x]; r < row_ptr[blockIdx.x + 1]; ++r) {
    const double* p = partials + slot_lo[r];
    for (int64_t i = threadIdx.x; i < slot_n[r]; i += kThreads) t += p[i];
  }
  const double b = block_sum(t);
  if (threadIdx.x == 0) out[blockIdx.x] = float(b);
}

// clip_coef_kernel's norm line per element: norms[i] = float(sqrt(double(sumsq[i])) / grad_div)
__global__ __launch_bounds__(kThreads) void param_norms_kernel(const float* __restrict__ sumsq,
                                                               int64_t n, double grad_div,
                                                               float* __restrict__ norms) {
#pragma clang fp contract(off)
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * kThreads)
    norms[i] = float(sqrt(double(sumsq[i])) / grad_div);
}

// zs_update_norms: parameter i of sums3 = [sum d^2 | sum p1^2 | touched], n floats each.  A step
// that measured nothing for i -- the coefficient is NaN (the guarded update skipped the step) or no
// rank has a range for i -- gives the update norm +0.0 and leaves the weight norm as it is.
__global__ __launch_bounds__(kThreads) void update_norms_kernel(
    const float* __restrict__ sums3, int64_t n, const float* __restrict__ coef,
    float* __restrict__ update_norms, float* __restrict__ weight_norms) {
#pragma clang fp contract(off)
  bool skipped = false;
  if (coef) {
    const float c = *coef;
    skipped = c != c;
  }
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * kThreads) {
    if (skipped || sums3[2 * n + i] == 0.0f) {
      update_norms[i] = 0.0f;
    } else {
      update_norms[i] = float(sqrt(double(sums3[i])));
      weight_norms[i] = float(sqrt(double(sums3[n + i])));
    }
  }
}

// clip_grad_norm_'s coefficient (error_if_nonfinite=False): norm = sqrt(sumsq) / grad_div in
// double, rounded once; coef = min(1, max_norm / (norm + 1e-6)) in fp32, a NaN norm giving a NaN
// coefficient as torch's clamp does.  One lane.
__global__ __launch_bounds__(64) void clip_coef_kernel(const float* __restrict__ sumsq,
                                                       double grad_div, float max_norm,
                                                       float* __restrict__ out2) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  const float norm = float(sqrt(double(*sumsq)) / grad_div);
  const float c = max_norm / (norm + 1e-6f);
  out2[0] = norm;
  out2[1] = c > 1.0f ? 1.0f : c;
}

// clip_coef_kernel plus the skip decision (zs_clip_coef_guarded), on the same lane: a norm that is
// not finite -- NaN or inf, from any non-finite gradient element or from a sum of squares beyond
// fp32 -- gives the quiet NaN 0x7FC00000 as the coefficient, which the GUARD update instances take
// as "skip this step", and counts one skipped step (a plain load, add and store: the launches of a
// stream are ordered).  A finite norm gives clip_coef_kernel's bits, and then the coefficient is
// never NaN: max_norm is finite or inf and >= 0 and norm + 1e-6f > 0, so the quotient is a
// number >= 0 or inf and the clamp a number in [0, 1].  NaN therefore means "skipped" and nothing
// else.
__global__ __launch_bounds__(64) void clip_coef_guarded_kernel(
    const float* __restrict__ sumsq, double grad_div, float max_norm, float* __restrict__ out2,
    unsigned long long* __restrict__ skipped) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  const float norm = float(sqrt(double(*sumsq)) / grad_div);
  const float c = max_norm / (norm + 1e-6f);
  out2[0] = norm;
  if ((__float_as_uint(norm) & 0x7F800000u) == 0x7F800000u) {  // NaN or inf
    out2[1] = __uint_as_float(0x7FC00000u);
    *skipped = *skipped + 1ull;
  } else {
    out2[1] = c > 1.0f ? 1.0f : c;
  }
}

// ----------------------------------------------------------------------------------------------
// in-place scale: x /= div (DDP's `param.grad /= world_size`, ddp.py:45-47)
// ----------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float to_f32(T x) {
  if constexpr (sizeof(T) == 4) return x;
  else return bf16_to_f32(x);
}
template <typename T>
__device__ __forceinline__ T from_f32(float x) {
  if constexpr (sizeof(T) == 4) return x;
  else return f32_to_bf16(x);
}

// In place, kScaleU 16-B accesses per lane in flight: a wave step covers kScaleU contiguous 1 KiB
// blocks (lane l of block u at 16-B chunk 64u + l), every load issued before the first store;
// grid-stride over wave steps; the tail (n % elements per step) by block 0.  Cache policy by size
// (NT): a DDP bucket (64 MiB) is scaled right after the all-reduce wrote it, while it is still in
// the 256 MB MALL — default policy; a buffer larger than the MALL cannot be there, so its loads
// and stores carry the non-temporal hint (kMallBytes; `zs_tune("scale_nt")` forces either).
// (Round 2's one access in flight per lane measured 0.61 of 8 TB/s on a 4 GiB buffer.)
// fp32: IEEE division (x / div), or an exact reciprocal multiply when div is a power of two;
// bf16: the same in fp32, rounded to bf16 (RNE) — torch's div_ on a bf16 tensor.
constexpr int kScaleU = 4;

template <typename T, bool NT>
__global__ __launch_bounds__(kThreads) void scale_kernel(T* __restrict__ x, int64_t n, float div,
                                                         float inv, int pow2) {
#pragma clang fp contract(off)
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t kSpan = int64_t(64) * V * kScaleU;  // elements per wave step
  const gptr<T> gx = glob(x);
  const int64_t steps = n / kSpan;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = int64_t(gridDim.x) * (kThreads / 64);
  auto op = [&](float f) { return pow2 ? f * inv : f / div; };
  for (int64_t w = int64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); w < steps;
       w += nwaves) {
    T* base = x + w * kSpan + int64_t(lane) * V;
    uint4 raw[kScaleU];
#pragma unroll
    for (int u = 0; u < kScaleU; ++u) raw[u] = ld16<NT>(base + u * 64 * V);
#pragma unroll
    for (int u = 0; u < kScaleU; ++u) {
      T* e = reinterpret_cast<T*>(&raw[u]);
#pragma unroll
      for (int j = 0; j < V; ++j) e[j] = from_f32<T>(op(to_f32<T>(e[j])));
      st16<NT>(base + u * 64 * V, raw[u]);
    }
  }
  if (blockIdx.x == 0) {
    for (int64_t i = steps * kSpan + threadIdx.x; i < n; i += kThreads)
      gx[i] = from_f32<T>(op(to_f32<T>(gx[i])));
  }
}

// ----------------------------------------------------------------------------------------------
// accumulate: dst += src (ZeRO-3 update mode's gradient accumulation: a later micro-batch's
// reduce-scattered chunks, in a staging buffer, added to the grad chunk arena)
// ----------------------------------------------------------------------------------------------
// The shape of scale_kernel with a second read stream: a wave step covers kAccU contiguous 1 KiB
// blocks of each buffer (lane l of block u at 16-B chunk 64u + l), all 2 kAccU loads issued before
// the first store; grid-stride over wave steps; the tail (n % elements per step) by block 0.
// 3 x element size bytes per element (dst read, src read, dst written); no atomics, LDS or scratch.
// fp32: one IEEE add; bf16: both operands widened exactly, one fp32 add, one RNE to bf16 (NaN stays
// NaN) — torch's add_ on a tensor of that dtype, i.e. what AccumulateGrad does to p.grad.
// Cache policy by size (NT) over the bytes touched, as zs_scale; `zs_tune("accumulate_nt")`
// forces either.
constexpr int kAccU = 4;

template <typename T, bool NT>
__global__ __launch_bounds__(kThreads) void accumulate_kernel(T* dst, const T* src, int64_t n) {
#pragma clang fp contract(off)
  constexpr int V = 16 / sizeof(T);
  constexpr int64_t kSpan = int64_t(64) * V * kAccU;  // elements per wave step
  const int64_t steps = n / kSpan;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = int64_t(gridDim.x) * (kThreads / 64);
  for (int64_t w = int64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); w < steps;
       w += nwaves) {
    const int64_t off = w * kSpan + int64_t(lane) * V;
    T* d = dst + off;
    const T* s = src + off;
    uint4 a[kAccU], b[kAccU];
#pragma unroll
    for (int u = 0; u < kAccU; ++u) a[u] = ld16<NT>(d + u * 64 * V);
#pragma unroll
    for (int u = 0; u < kAccU; ++u) b[u] = ld16<NT>(s + u * 64 * V);
#pragma unroll
    for (int u = 0; u < kAccU; ++u) {
      T* x = reinterpret_cast<T*>(&a[u]);
      const T* y = reinterpret_cast<const T*>(&b[u]);
#pragma unroll
      for (int j = 0; j < V; ++j) x[j] = from_f32<T>(to_f32<T>(x[j]) + to_f32<T>(y[j]));
      st16<NT>(d + u * 64 * V, a[u]);
    }
  }
  if (blockIdx.x == 0) {
    const gptr<T> gd = glob(dst);
    const gptr<const T> gs = glob(src);
    for (int64_t i = steps * kSpan + threadIdx.x; i < n; i += kThreads)
      gd[i] = from_f32<T>(to_f32<T>(gd[i]) + to_f32<T>(gs[i]));
  }
}

// ----------------------------------------------------------------------------------------------
// widening accumulate: fp32 dst = bf16 a + bf16 src (FIRST), or fp32 dst += bf16 src
// (accumulation_dtype=torch.float32: later micro-batches' bf16 chunks summed in an fp32 arena)
// ----------------------------------------------------------------------------------------------
// Mixed widths, so the wave-dense pattern of convert_kernel below and not accumulate_kernel's
// lane-contiguous 16 B on every stream: a wave step covers kWidenSpan elements in kWidenU blocks of
// 256; in block u lane l handles elements [256u + 4l, +4) — one 16-B fp32 access and one 8-B bf16
// access per stream, every wave instruction one contiguous 1 KiB (fp32) or 512 B (bf16) span.  All
// of a step's loads (2 kWidenU) are issued before its first store; grid-stride over wave steps; the
// n % kWidenSpan tail by block 0.  FIRST: 2 + 2 B read, 4 B written per element; otherwise 4 + 2 B
// read, 4 B written.  No atomics, LDS or scratch.  Widening is exact (bits << 16), then one IEEE
// fp32 add per element: a NaN stays a NaN, Inf + -Inf is NaN, denormals are kept.
// Cache policy by size (NT) over the bytes touched, under `zs_tune("accumulate_nt")` as zs_accumulate.
constexpr int kWidenU = 4;
constexpr int64_t kWidenSpan = 256 * kWidenU;

__device__ __forceinline__ void widen4(const uint2& h, float (&f)[4]) {
  f[0] = __uint_as_float(h.x << 16), f[1] = __uint_as_float(h.x & 0xffff0000u);
  f[2] = __uint_as_float(h.y << 16), f[3] = __uint_as_float(h.y & 0xffff0000u);
}

template <bool FIRST, bool NT>
__global__ __launch_bounds__(kThreads) void accumulate_widen_kernel(float* dst,
                                                                    const unsigned short* a,
                                                                    const unsigned short* src,
                                                                    int64_t n) {
#pragma clang fp contract(off)
  const int64_t steps = n / kWidenSpan;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = int64_t(gridDim.x) * (kThreads / 64);
  for (int64_t w = int64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); w < steps;
       w += nwaves) {
    const int64_t base = w * kWidenSpan + 4 * lane;
    float* d = dst + base;
    const unsigned short* s = src + base;
    uint4 x4[kWidenU];
    uint2 x2[kWidenU], y2[kWidenU];
#pragma unroll
    for (int u = 0; u < kWidenU; ++u) {
      if constexpr (FIRST) x2[u] = ld8<NT>(a + base + 256 * u);
      else x4[u] = ld16<NT>(d + 256 * u);
    }
#pragma unroll
    for (int u = 0; u < kWidenU; ++u) y2[u] = ld8<NT>(s + 256 * u);
#pragma unroll
    for (int u = 0; u < kWidenU; ++u) {
      float x[4], y[4];
      if constexpr (FIRST) widen4(x2[u], x);
      else unpack4(x4[u], x);
      widen4(y2[u], y);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = x[j] + y[j];
      st16<NT>(d + 256 * u, pack4(x));
    }
  }
  if (blockIdx.x == 0) {
    const gptr<float> gd = glob(dst);
    const gptr<const unsigned short> ga = glob(a), gs = glob(src);
    for (int64_t i = steps * kWidenSpan + threadIdx.x; i < n; i += kThreads)
      gd[i] = (FIRST ? bf16_to_f32(ga[i]) : gd[i]) + bf16_to_f32(gs[i]);
  }
}

// ----------------------------------------------------------------------------------------------
// fp32 <-> bf16 conversion (the bf16 gradient exchange of fp32-parameter models)
// ----------------------------------------------------------------------------------------------
// Wave-dense accesses: a wave step covers kConvSpan elements in kConvU blocks of 256; in block u
// lane l converts elements [256u + 4l, +4) — one 16-B fp32 access and one 8-B bf16 access per
// block, so every wave instruction touches one contiguous 1 KiB (fp32) or 512 B (bf16) span.
// (Round 2's lane-contiguous 8 elements per lane gave each fp32 instruction a 32-B lane stride —
// half-dense — and measured 0.58 of 8 TB/s bf16 -> fp32, profiles/r03_kernels_table.json.)
// All kConvU loads are issued before the first store; grid-stride over wave steps; the n % kConvSpan
// tail by block 0.  Cache policy by size (NT), as zs_scale: non-temporal when source and destination
// together are larger than the MALL, the default policy below (a bucket's grads just written by
// backward, the bf16 bucket read next by the collective); `zs_tune("convert_nt")` forces either.
// Round 4 A/B on placed buffers (profiles/r04_policy_ab.json): 64 MiB fp32 side, bf16 -> fp32 0.80
// default vs 0.72 non-temporal (fp32 -> bf16 0.83 / 0.85); 256 MiB and above non-temporal wins
// (0.84 / 0.74 fp32 -> bf16, 0.75 / 0.72 bf16 -> fp32).
// fp32 -> bf16 rounds to nearest even (v_cvt_pk_bf16_f32), NaN stays NaN; bf16 -> fp32 is exact.
constexpr int kConvU = 4;
constexpr int64_t kConvSpan = 256 * kConvU;

template <bool TO_BF16, bool NT>
__global__ __launch_bounds__(kThreads) void convert_kernel(const void* __restrict__ src,
                                                           void* __restrict__ dst, int64_t n) {
  const int64_t steps = n / kConvSpan;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = int64_t(gridDim.x) * (kThreads / 64);
  for (int64_t w = int64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6); w < steps;
       w += nwaves) {
    const int64_t base = w * kConvSpan + 4 * lane;
    if constexpr (TO_BF16) {
      const float* s = static_cast<const float*>(src) + base;
      float4 a[kConvU];
#pragma unroll
      for (int u = 0; u < kConvU; ++u) {
        const uint4 r = ld16<NT>(s + 256 * u);
        a[u] = make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z),
                           __uint_as_float(r.w));
      }
      unsigned short* d = static_cast<unsigned short*>(dst) + base;
#pragma unroll
      for (int u = 0; u < kConvU; ++u) {
        const uint32_t lo = uint32_t(f32_to_bf16(a[u].x)) | (uint32_t(f32_to_bf16(a[u].y)) << 16);
        const uint32_t hi = uint32_t(f32_to_bf16(a[u].z)) | (uint32_t(f32_to_bf16(a[u].w)) << 16);
        st8<NT>(d + 256 * u, make_uint2(lo, hi));
      }
    } else {
      const unsigned short* s = static_cast<const unsigned short*>(src) + base;
      uint2 h[kConvU];
#pragma unroll
      for (int u = 0; u < kConvU; ++u) h[u] = ld8<NT>(s + 256 * u);
      float* d = static_cast<float*>(dst) + base;
#pragma unroll
      for (int u = 0; u < kConvU; ++u)
        st16<NT>(d + 256 * u, make_uint4(h[u].x << 16, h[u].x & 0xffff0000u, h[u].y << 16,
                                         h[u].y & 0xffff0000u));
    }
  }
  if (blockIdx.x == 0) {
    for (int64_t i = steps * kConvSpan + threadIdx.x; i < n; i += kThreads) {
      if constexpr (TO_BF16)
        glob(static_cast<unsigned short*>(dst))[i] = f32_to_bf16(glob(static_cast<const float*>(src))[i]);
      else
        glob(static_cast<float*>(dst))[i] = bf16_to_f32(glob(static_cast<const unsigned short*>(src))[i]);
    }
  }
}

// scalar variant for unaligned buffers
template <bool TO_BF16>
__global__ __launch_bounds__(kThreads) void convert_scalar_kernel(const void* __restrict__ src,
                                                                  void* __restrict__ dst, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * kThreads) {
    if constexpr (TO_BF16)
      glob(static_cast<unsigned short*>(dst))[i] = f32_to_bf16(glob(static_cast<const float*>(src))[i]);
    else
      glob(static_cast<float*>(dst))[i] = bf16_to_f32(glob(static_cast<const unsigned short*>(src))[i]);
  }
}

// ----------------------------------------------------------------------------------------------
// row-wise fp8 (OCP E4M3) quantise / dequantise for the low-precision parameter all-gather
// ----------------------------------------------------------------------------------------------
constexpr float kE4M3Max = 448.0f;

__device__ __forceinline__ uint32_t e4m3x4(float a, float b, float c, float d) {
  // v_cvt_pk_fp8_f32: round to nearest even, OCP E4M3 on gfx950 (no saturation: from 480 on, and
  // for NaN, the NaN code); finite inputs stay below the tie at 464 (qscaled)
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return uint32_t(w);
}
// Degenerate rows (DESIGN.md §4 "fp8 rows: the contract").  A row whose amax (the max of |x| over
// its non-NaN elements; fmaxf drops NaN) lies below 2^-116 is scaled as though amax were 2^-116:
// 448 / amax would overflow to +inf from amax < 448 / FLT_MAX ~ 1.32e-36 on, and 0 * inf is NaN;
// with the floor inv <= 1.75 * 2^124 stays finite and scale stays normal.  Rows at or above the
// floor keep their bits.
constexpr float kAmaxFloor = 0x1p-116f;
__device__ __forceinline__ float q_inv(float amax) {
  return amax > 0.0f ? kE4M3Max / fmaxf(amax, kAmaxFloor) : 1.0f;
}
__device__ __forceinline__ float q_scale(float amax) {
  return amax > 0.0f ? fmaxf(amax, kAmaxFloor) / kE4M3Max : 1.0f;
}
// The scaled value handed to the conversion, unclamped.  |x| <= amax and both the division and
// the product are correctly rounded, so a finite |x * inv| is at most 448 * (1 + 2^-23), and
// v_cvt_pk_fp8_f32 rounds everything up to the tie at 464 to 448 (RNE, ties to even).  A NaN
// product (a NaN element, or +-Inf times the inv = 0 of a row that holds an Inf) it stores as
// the E4M3 NaN code 0xFF whatever the NaN's sign.  The clamp that used to stand here,
// v_med3_f32(x * inv, 448, -448), answers a NaN operand with the minimum of the three: it stored
// a NaN as 0xFE, which came back as the finite value -amax.
__device__ __forceinline__ float qscaled(float x, float inv) {
#pragma clang fp contract(off)
  return x * inv;
}

// Block-per-row fallback for any row length and alignment (scalar accesses): amax by wave
// shuffles + a 4-entry LDS exchange, then the row is re-read (L2-resident) and converted.
template <typename T>
__global__ __launch_bounds__(kThreads) void fp8_quantize_rows_kernel(
    const T* __restrict__ src, unsigned char* __restrict__ dst, float* __restrict__ scales,
    int64_t rows, int64_t row_len) {
#pragma clang fp contract(off)
  __shared__ float red[kThreads / 64];
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const gptr<const T> x = glob(src + r * row_len);
    const gptr<unsigned char> q = glob(dst + r * row_len);
    float amax = 0.0f;
    for (int64_t i = threadIdx.x; i < row_len; i += kThreads) amax = fmaxf(amax, fabsf(to_f32<T>(x[i])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    const float inv = q_inv(amax);
    if (threadIdx.x == 0) glob(scales)[r] = q_scale(amax);
    for (int64_t i = threadIdx.x; i < row_len; i += kThreads) {
      const float c = qscaled(to_f32<T>(x[i]), inv);
      q[i] = (unsigned char)(__builtin_amdgcn_cvt_pk_fp8_f32(c, c, 0, false) & 0xff);
    }
  }
}

// Wave-per-row variant (the vector path): each 64-lane wave owns rows r = 4*block + wave (grid
// stride), reads the row as lane-contiguous 16-byte chunks (one wave instruction = 1 KiB), reduces
// amax with wave shuffles only (no LDS, no block barrier), and converts.  NREG > 0: the row's
// chunks stay in registers between the two passes (rows of at most 64 * NREG chunks: NREG = 8, 16
// or 32, i.e. up to 16384 bf16 / 8192 fp32 elements — every row of the C5 set) — one read of the
// row, all of its loads in flight at once; NREG == 0 (longer rows): both passes stream the row in
// batches of 8 loads in flight per lane, the second from L2 / MALL where it is still cached.  Same
// arithmetic, same bits as the block-per-row kernel: amax = max|x|, inv = 448/amax,
// e4m3(RNE(x*inv)), scale = amax/448 (q_inv, q_scale, qscaled above).
// One row, one wave (lane = threadIdx.x & 63): x -> q (row_len elements), *scale.
template <typename T, int NREG>
__device__ __forceinline__ void fp8_quantize_row(const T* __restrict__ src_row,
                                                 unsigned char* __restrict__ dst_row,
                                                 float* __restrict__ scale, int64_t row_len,
                                                 int lane) {
#pragma clang fp contract(off)
  constexpr int E = 16 / int(sizeof(T));  // elements per 16-byte chunk
  constexpr int R = NREG > 0 ? NREG : 8;  // chunks in flight per lane
  auto unpack = [](const uint4& raw, float* v) {
    if constexpr (sizeof(T) == 2) {
      const unsigned short* h = reinterpret_cast<const unsigned short*>(&raw);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32(h[j]);
    } else {
      v[0] = __uint_as_float(raw.x); v[1] = __uint_as_float(raw.y);
      v[2] = __uint_as_float(raw.z); v[3] = __uint_as_float(raw.w);
    }
  };
  const gptr<const T> x = glob(src_row);
  const gptr<unsigned char> q = glob(dst_row);
  auto load = [&](int64_t i) {
    if (i >= row_len) return make_uint4(0, 0, 0, 0);
    if constexpr (NREG > 0) return nt_ld16(x + i);  // read once
    else return *reinterpret_cast<gptr<const uint4>>(x + i);  // read again in pass 2
  };
  float amax = 0.0f;
  uint4 keep[R];
  for (int64_t b0 = 0; b0 < row_len; b0 += int64_t(64) * R * E) {  // NREG > 0: one batch
#pragma unroll
    for (int u = 0; u < R; ++u) keep[u] = load(b0 + (int64_t(u) * 64 + lane) * E);
#pragma unroll
    for (int u = 0; u < R; ++u) {
      float v[E];
      unpack(keep[u], v);
#pragma unroll
      for (int j = 0; j < E; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  const float inv = q_inv(amax);
  if (lane == 0) *glob(scale) = q_scale(amax);
  auto emit = [&](int64_t i, const uint4& raw) {
    float v[E];
    unpack(raw, v);
    if constexpr (sizeof(T) == 2) {
      uint2 out;
      out.x = e4m3x4(qscaled(v[0], inv), qscaled(v[1], inv), qscaled(v[2], inv), qscaled(v[3], inv));
      out.y = e4m3x4(qscaled(v[4], inv), qscaled(v[5], inv), qscaled(v[6], inv), qscaled(v[7], inv));
      nt_st8(q + i, out);
    } else {
      *reinterpret_cast<gptr<uint32_t>>(q + i) =
          e4m3x4(qscaled(v[0], inv), qscaled(v[1], inv), qscaled(v[2], inv), qscaled(v[3], inv));
    }
  };
  if constexpr (NREG > 0) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int64_t i = (int64_t(u) * 64 + lane) * E;
      if (i < row_len) emit(i, keep[u]);
    }
  } else {
    for (int64_t b0 = 0; b0 < row_len; b0 += int64_t(64) * R * E) {
#pragma unroll
      for (int u = 0; u < R; ++u) keep[u] = load(b0 + (int64_t(u) * 64 + lane) * E);
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int64_t i = b0 + (int64_t(u) * 64 + lane) * E;
        if (i < row_len) emit(i, keep[u]);
      }
    }
  }
}

template <typename T, int NREG>
__global__ __launch_bounds__(kThreads) void fp8_quantize_rows_wave_kernel(
    const T* __restrict__ src, unsigned char* __restrict__ dst, float* __restrict__ scales,
    int64_t rows, int64_t row_len) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = kThreads / 64;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  for (int64_t r = int64_t(blockIdx.x) * wpb + wave; r < rows; r += int64_t(gridDim.x) * wpb)
    fp8_quantize_row<T, NREG>(src + r * row_len, dst + r * row_len, scales + r, row_len, lane);
}

// A gather group's matrices in one launch (zs_fp8_quantize_rowset): global row g (one wave each,
// grid-stride, so g only grows and the matrix lookup is a forward scan) of matrix m, local row
// lr = g - prefix[m]; rows [rows[m], cs[m]) are the chunk's padding: q = 0, scale = 1.  The table
// travels in the kernel arguments (constant, uniform: scalar loads).
constexpr int kSetMax = 16;
struct QSet {
  const void* src[kSetMax];
  unsigned char* q[kSetMax];
  float* sc[kSetMax];
  int64_t rows[kSetMax], row_len[kSetMax], prefix[kSetMax + 1];  // prefix over cs
  int n;
};

template <typename T, int NREG>
__global__ __launch_bounds__(kThreads) void fp8_quantize_rowset_kernel(const QSet set) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = kThreads / 64;
  const int64_t total = set.prefix[set.n];
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // uniform: scalar math
  int m = 0;
  for (int64_t g = int64_t(blockIdx.x) * wpb + wave; g < total; g += int64_t(gridDim.x) * wpb) {
    while (set.prefix[m + 1] <= g) ++m;
    const int64_t lr = g - set.prefix[m], len = set.row_len[m];
    unsigned char* qrow = set.q[m] + lr * len;
    if (lr < set.rows[m]) {
      fp8_quantize_row<T, NREG>(static_cast<const T*>(set.src[m]) + lr * len, qrow, set.sc[m] + lr,
                                len, lane);
    } else {  // padding row of the chunk
      for (int64_t i = int64_t(lane) * 8; i < len; i += 64 * 8) nt_st8(qrow + i, make_uint2(0, 0));
      if (lane == 0) *glob(set.sc[m] + lr) = 1.0f;
    }
  }
}

// Dequantise (round 4): one wave walks whole rows.  The rows of a set of matrices are numbered
// over the set (a single matrix for zs_fp8_dequantize_rows; every matrix of a gather group, rank by
// rank, for zs_fp8_dequantize_gathered), and each wave takes rows g, g + nwaves, ... — so the matrix
// index only grows (uniform forward scan) and the row's rank, local row, scale and source /
// destination pointers are worked out ONCE per row, in scalar registers (one 32-bit division per
// row, none per access).  The wave then walks the row in batches of kDqU accesses per lane: 8-B fp8
// loads (512 B per wave instruction, dense) and 16-B bf16 stores (1 KiB, dense) for bf16 output,
// 4 B -> 16 B for fp32.  The loads of the NEXT batch — in the same row or the wave's next row — are
// issued before the stores of the current one, so on gfx950, whose vmcnt counts loads and stores
// together, waiting for a batch's data never waits for the previous batch's stores: each wave keeps
// one batch of loads and one of stores in flight throughout.
constexpr int kDqU = 4;  // default accesses in flight per lane (zs_tune "dq_unroll": 4 / 8 / 16;
                         // 4 measured best at ws = 1 and ws = 8, profiles/r04_dq_ab.json)

struct DqSet {
  const unsigned char* q;
  const float* sc;
  int64_t q_rank, sc_rank;  // per-rank strides of the gathered q (bytes) and scales (elements)
  int64_t q_off[kSetMax], sc_off[kSetMax], cs[kSetMax], row_len[kSetMax];
  int64_t prefix[kSetMax + 1];  // prefix over ws * cs[m] full rows
  void* dst[kSetMax];
  int n;
};

template <typename T>
struct DqRow {
  const unsigned char* q;
  T* y;
  float sc;
  int64_t len;
};

template <typename T, int U>
__device__ __forceinline__ void fp8_dq_load(const DqRow<T>& r, int64_t b0, int lane, uint2* raw) {
  constexpr int E = sizeof(T) == 2 ? 8 : 4;
  const gptr<const unsigned char> q = glob(r.q);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = b0 + (int64_t(u) * 64 + lane) * E;
    raw[u] = make_uint2(0, 0);
    if (i < r.len) {
      if constexpr (E == 8) raw[u] = nt_ld8(q + i);
      else raw[u].x = __builtin_nontemporal_load(reinterpret_cast<gptr<const uint32_t>>(q + i));
    }
  }
}

template <typename T, int U, bool NT>
__device__ __forceinline__ void fp8_dq_store(const DqRow<T>& r, int64_t b0, int lane,
                                             const uint2* raw) {
#pragma clang fp contract(off)
  constexpr int E = sizeof(T) == 2 ? 8 : 4;
  const gptr<T> y = glob(r.y);
  const float sc = r.sc;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = b0 + (int64_t(u) * 64 + lane) * E;
    if (i >= r.len) continue;
    const int lo = int(raw[u].x), hi = int(raw[u].y);
    const float a0 = __builtin_amdgcn_cvt_f32_fp8(lo, 0) * sc, a1 = __builtin_amdgcn_cvt_f32_fp8(lo, 1) * sc;
    const float a2 = __builtin_amdgcn_cvt_f32_fp8(lo, 2) * sc, a3 = __builtin_amdgcn_cvt_f32_fp8(lo, 3) * sc;
    if constexpr (E == 8) {
      const float b0_ = __builtin_amdgcn_cvt_f32_fp8(hi, 0) * sc, b1 = __builtin_amdgcn_cvt_f32_fp8(hi, 1) * sc;
      const float b2 = __builtin_amdgcn_cvt_f32_fp8(hi, 2) * sc, b3 = __builtin_amdgcn_cvt_f32_fp8(hi, 3) * sc;
      auto pk = [](float a, float b) { return uint32_t(f32_to_bf16(a)) | (uint32_t(f32_to_bf16(b)) << 16); };
      const uint4 v = make_uint4(pk(a0, a1), pk(a2, a3), pk(b0_, b1), pk(b2, b3));
      if constexpr (NT) nt_st16(y + i, v);
      else *reinterpret_cast<gptr<uint4>>(y + i) = v;
    } else {
      if constexpr (NT) st4(reinterpret_cast<float*>(r.y + i), 0, make_float4(a0, a1, a2, a3));
      else *reinterpret_cast<gptr<float4>>(y + i) = make_float4(a0, a1, a2, a3);
    }
  }
}

template <typename T, int U, bool NT>
__global__ __launch_bounds__(kThreads) void fp8_dequantize_gathered_kernel(const DqSet set) {
  constexpr int64_t B = int64_t(64) * (sizeof(T) == 2 ? 8 : 4) * U;  // elements per batch
  const int lane = threadIdx.x & 63;
  const int64_t total = set.prefix[set.n];
  const int64_t nwaves = int64_t(gridDim.x) * (kThreads / 64);
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // uniform: scalar math
  int m = 0;
  // row g of the set -> its pointers and scale (uniform; the host checks ws * cs[m] < 2^31)
  auto row_at = [&](int64_t g, DqRow<T>& r) {
    while (set.prefix[m + 1] <= g) ++m;
    const uint32_t R = uint32_t(g - set.prefix[m]), cs = uint32_t(set.cs[m]);
    const uint32_t rk = R / cs, lr = R - rk * cs;
    r.len = set.row_len[m];
    r.sc = glob(set.sc)[int64_t(rk) * set.sc_rank + set.sc_off[m] + lr];
    r.q = set.q + int64_t(rk) * set.q_rank + set.q_off[m] + int64_t(lr) * r.len;
    r.y = static_cast<T*>(set.dst[m]) + int64_t(R) * r.len;
  };
  int64_t g = int64_t(blockIdx.x) * (kThreads / 64) + wave;
  if (g >= total) return;
  DqRow<T> cur;
  row_at(g, cur);
  int64_t b0 = 0;
  uint2 raw[U];
  fp8_dq_load<T, U>(cur, b0, lane, raw);
  while (true) {
    DqRow<T> nxt = cur;
    int64_t nb0 = b0 + B;
    bool more = true;
    if (nb0 >= cur.len) {  // the wave's next row
      g += nwaves;
      more = g < total;
      if (more) row_at(g, nxt);
      nb0 = 0;
    }
    uint2 nraw[U];
    if (more) fp8_dq_load<T, U>(nxt, nb0, lane, nraw);  // next batch's loads before this one's stores
    fp8_dq_store<T, U, NT>(cur, b0, lane, raw);
    if (!more) break;
    cur = nxt;
    b0 = nb0;
#pragma unroll
    for (int u = 0; u < U; ++u) raw[u] = nraw[u];
  }
}

// Scalar fallback for any row length and alignment: grid-stride over elements.
template <typename T>
__global__ __launch_bounds__(kThreads) void fp8_dequantize_rows_kernel(
    const unsigned char* __restrict__ src, const float* __restrict__ scales, T* __restrict__ dst,
    int64_t n, int64_t row_len) {
#pragma clang fp contract(off)
  const gptr<const unsigned char> q = glob(src);
  const gptr<T> y = glob(dst);
  const int64_t stride = int64_t(gridDim.x) * kThreads;
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const float v = __builtin_amdgcn_cvt_f32_fp8(int(q[i]), 0) * glob(scales)[i / row_len];
    y[i] = from_f32<T>(v);
  }
}

inline bool aligned(uint64_t p, uint64_t a) { return p % a == 0; }

// Diagnostic tuning knobs of the dequantise kernel (zs_tune; defaults are the measured best):
// accesses in flight per lane, non-temporal stores, and a cap of workgroups per CU (0 = one wave
// per row up to the usual grid cap; k > 0 = at most k workgroups per CU, each wave walking several
// rows with the next row's loads issued before the current row's stores).
struct DqTune {
  int unroll = kDqU;
  int nt_store = 1;
  int wg_per_cu = 0;
};
DqTune& dq_tune() {
  static DqTune t;
  return t;
}

// Adam grid (zs_tune "adam_wg_per_cu", diagnostic A/B): 0 = the kernel's default, k = at most k
// workgroups per CU striding over the chunks.  The default is grid_cap()'s 128 per CU, and 1024
// per CU for the loads-first vector kernel of the split master: at C4 size 1024-2048 per CU
// measured 2.5 % under 128 and 2.2 % under one workgroup per chunk
// (profiles/r07_adam_ab_grid.json); the predicated kernel gains half of that from the grid, and
// the fp32-master instance 0.4 %, short of the 1 % that tells a gain from noise
// (profiles/r07_adam_ab_fp32_master.json), so both keep 128
constexpr int kAdamWgPerCu = 128, kAdamLoadsFirstWgPerCu = 1024;
int& adam_wg_per_cu() {
  static int v = 0;
  return v;
}
// Full chunks' issue order (zs_tune "adam_loads_first", diagnostic A/B): 1 = update_full_chunk (all
// of a chunk's loads before its first wait), 0 = every chunk through the predicated body that
// partial chunks take
int& adam_loads_first() {
  static int v = 1;
  return v;
}
// Cache policy of the gradient sum-of-squares pass (zs_tune "sqnorm_nt", diagnostic A/B): 1 =
// non-temporal loads, 0 = the default policy.  The sum's bits do not depend on it.
int& sqnorm_nt() {
  static int v = 1;
  return v;
}
int64_t adam_grid_cap(int default_per_cu) {
  const int k = adam_wg_per_cu();
  return int64_t(grid_cap() / 128) * (k > 0 ? k : default_per_cu);
}

// zs_scale's / zs_convert's / zs_copyset_run's cache policy: -1 by size (kMallBytes), 0 default
// policy, 1 non-temporal
int& scale_nt_mode() {
  static int mode = -1;
  return mode;
}
int& convert_nt_mode() {
  static int mode = -1;
  return mode;
}
int& copy_nt_mode() {
  static int mode = -1;
  return mode;
}
int& accumulate_nt_mode() {
  static int mode = -1;
  return mode;
}

int dq_grid(int64_t rows) {
  int64_t cap = grid_cap();
  const int per_cu = dq_tune().wg_per_cu;
  if (per_cu > 0) cap = std::max<int64_t>(1, cap / 128 * per_cu);
  return int(std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, cap)));
}

template <typename T>
void launch_dequantize_t(const DqSet& set, int grid, hipStream_t st) {
  const DqTune& t = dq_tune();
#define ZS_DQ(U, NT) hipLaunchKernelGGL((fp8_dequantize_gathered_kernel<T, U, NT>), dim3(grid), dim3(kThreads), 0, st, set)
  if (t.nt_store) {
    switch (t.unroll) { case 4: ZS_DQ(4, true); break; case 16: ZS_DQ(16, true); break; default: ZS_DQ(8, true); }
  } else {
    switch (t.unroll) { case 4: ZS_DQ(4, false); break; case 16: ZS_DQ(16, false); break; default: ZS_DQ(8, false); }
  }
#undef ZS_DQ
}

void launch_dequantize(const DqSet& set, int dst_dtype, int grid, hipStream_t st) {
  if (dst_dtype == ZS_F32) launch_dequantize_t<float>(set, grid, st);
  else launch_dequantize_t<unsigned short>(set, grid, st);
}

}  // namespace

struct zs_copyset {
  CopySeg* d_segs = nullptr;
  int64_t* d_prefix = nullptr;
  int64_t nseg = 0, total_chunks = 0;
  int64_t bytes = 0;                // copied per run (read + write: 2x this)
  int unroll = kCopyUnrollDefault;  // 16-B accesses in flight per lane (chunk = 4 KiB * unroll)
};

// ZERO_AMD_COPY_UNROLL (diagnostic A/B): 2, 4 (default) or 8 accesses in flight per lane.
static int copy_unroll() {
  static int u = 0;
  if (u == 0) {
    const char* e = std::getenv("ZERO_AMD_COPY_UNROLL");
    const int v = e ? std::atoi(e) : kCopyUnrollDefault;
    u = (v == 2 || v == 4 || v == 8) ? v : kCopyUnrollDefault;
  }
  return u;
}

struct zs_adamset {
  // vector table (aligned, n % 4 == 0) and scalar table (tails, unaligned segments)
  AdamSeg* d_vec = nullptr;
  int64_t* d_vec_prefix = nullptr;
  AdamSeg* d_sca = nullptr;
  int64_t* d_sca_prefix = nullptr;
  int64_t nvec = 0, vec_chunks = 0, nsca = 0, sca_chunks = 0, elems = 0, bytes = 0;
  // zs_adamset_grad_sqnorm: partials (= workgroups) of the vector and of the scalar table
  int64_t sq_vec = 0, sq_sca = 0;
  // zs_adamset_grad_sqnorm_segs: per table, entries + 1 slot prefixes followed by each entry's
  // first slot in the set's partials (one upload); the slots of each table; seg_off (inputs + 1)
  int64_t* d_vec_slots = nullptr;
  int64_t* d_sca_slots = nullptr;
  int64_t sqs_vec = 0, sqs_sca = 0;
  std::vector<int64_t> seg_off;
  // zs_adamset_run_stats: 4 slots per chunk of either table, by input segment (vector part, then
  // scalar part); each table entry's first slot (un_vec, then un_sca), on the device from the first
  // such run on (d_un_off: nvec + nsca offsets); un_seg_off (inputs + 1)
  std::vector<int64_t> un_off, un_seg_off;
  mutable int64_t* d_un_off = nullptr;
  int g_dtype = ZS_F32, p_dtype = ZS_BF16, has_carry = 0, has_vmax = 0;
  // zs_sgdset_create: an SGD set (field m is the momentum buffer, has_mom: it has one)
  int sgd = 0, has_mom = 0;
  // zs_lionset_create: a Lion set (field m is exp_avg, fp32 or bf16 by state_dtype; no v)
  int lion = 0;
  // zs_adamset_create_ex: the element type of m and v, ZS_F32 or ZS_BF16
  int state_dtype = ZS_F32;
  // zs_adamset_set_grads: which input segment each table entry came from (the scalar entries with
  // their byte offset into that input's gradient), the gradient each input is bound to now, its
  // elements, whether it has a vector part (then its gradient must keep the vector alignment), and
  // the algorithmic bytes of one run without any gradient read
  int32_t* d_vec_in = nullptr;
  int32_t* d_sca_in = nullptr;
  int64_t* d_sca_goff = nullptr;
  std::vector<uint64_t> in_g;
  std::vector<int64_t> in_n;
  std::vector<unsigned char> in_vec;
  int64_t bytes_no_g = 0;
  // zs_adamset_run_sr: the lowest m address of the inputs (~0: none) and whether they all share
  // its parity (an element index is a whole number of bf16 elements from m_base)
  uint64_t m_lowest = ~uint64_t(0);
  int m_one_parity = 1;
  // zs_adamset_run_psr over fp32 moments: whether all inputs' m share m_lowest's low two bits
  int m_one_mod4 = 1;
  // zs_adamset_set_state_rounding: a ZS_BF16_SR set's bf16 moments round stochastically
  int state_sr = 0;
};

// ZS_BF16_SR (master-free) sets have the split master's geometry: 16-bit parameter stream, 4 groups
static bool split_geometry(const zs_adamset* as) {
  return as->p_dtype == ZS_BF16_SPLIT || as->p_dtype == ZS_BF16_SR;
}

namespace {
// zs_adamset_set_grads: new gradient pointers for inputs [k0, k0 + n) of a set, in the kernel
// arguments (no upload, no host synchronisation), patched into the device tables in stream order.
constexpr int kGradPatchMax = 224;
struct GradPatch {
  uint64_t g[kGradPatchMax];
  int64_t k0;
  int n;
};

__global__ __launch_bounds__(kThreads) void adam_patch_grads_kernel(
    AdamSeg* __restrict__ vec, const int32_t* __restrict__ vec_in, int64_t nvec,
    AdamSeg* __restrict__ sca, const int32_t* __restrict__ sca_in,
    const int64_t* __restrict__ sca_goff, int64_t nsca, const GradPatch p) {
  for (int64_t j = int64_t(blockIdx.x) * kThreads + threadIdx.x; j < nvec + nsca;
       j += int64_t(gridDim.x) * kThreads) {
    if (j < nvec) {
      const int64_t k = int64_t(vec_in[j]) - p.k0;
      if (k >= 0 && k < p.n) glob(&vec[j].g)[0] = reinterpret_cast<const void*>(p.g[k]);
    } else {
      const int64_t t = j - nvec;
      const int64_t k = int64_t(sca_in[t]) - p.k0;
      if (k >= 0 && k < p.n) {
        const uint64_t g = p.g[k];
        glob(&sca[t].g)[0] = reinterpret_cast<const void*>(g ? g + uint64_t(sca_goff[t]) : 0);
      }
    }
  }
}
}  // namespace

// zs_adam_step's one-range tables: [vector segment, tail segment], prefixes {0, vch, 0, sch}.
struct AdamTables {
  AdamSeg seg[2];
  int64_t prefix[4];
};

__global__ void write_tables_kernel(AdamTables* __restrict__ d, AdamTables t) { *d = t; }

// Table uploads run on a private non-blocking stream per device, so creating a set never
// synchronises with the legacy null stream (which may hold kernels waiting on collectives).
static hipStream_t upload_stream() {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
  streams[dev] = st;
  return st;
}

template <typename T>
static int upload(const std::vector<T>& h, T** d) {
  *d = nullptr;
  if (h.empty()) return ZS_OK;
  hipStream_t st = upload_stream();
  if (!st) return zs::fail(ZS_ERR_HIP, "table upload: no upload stream");
  ZS_HIP(hipMalloc(reinterpret_cast<void**>(d), h.size() * sizeof(T)));
  hipError_t e = hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(*d);
    *d = nullptr;
    return zs::fail(ZS_ERR_HIP, "table upload failed: %s", hipGetErrorString(e));
  }
  return ZS_OK;
}

// HP's and SgdHP's `grad / grad_div`: a power-of-two divisor is an exact reciprocal multiply
template <typename HPT>
static void set_grad_div(HPT* hp, float grad_div) {
  int exp2 = 0;
  hp->grad_div = grad_div;
  hp->div_pow2 = std::frexp(double(grad_div), &exp2) == 0.5 ? 1 : 0;
  hp->inv_div = float(1.0 / double(grad_div));
}

static HP make_hp(const zs_adam_hparams* h) {
  HP hp;
  const float w = h->one_minus_beta1;
  hp.lerp_hi = std::fabs(w) < 0.5f ? 0 : 1;  // a NaN weight takes the high form, as in ATen
  hp.lerp_w = hp.lerp_hi ? w - 1.0f : w;
  hp.beta2 = h->beta2;
  hp.omb2 = h->one_minus_beta2;
  hp.neg_step = h->neg_step_size;
  hp.bc2_sqrt = h->bc2_sqrt;
  hp.eps = h->eps;
  hp.wd = h->weight_decay;
  hp.decay_mul = h->decay_mul;
  hp.carry_mul = h->carry_mul;
  set_grad_div(&hp, h->grad_div);
  hp.maximize = h->maximize;
  return hp;
}

// A family of update kernels: its rule as a function of the one rule flag (amsgrad / momentum
// buffer), the type m and v are stored as, and whether instances with the flag set or with the
// ZeRO-1 carry exist at all.  16-bit moments have neither: set_create refuses their vmax and carry
// and adam_run their amsgrad, so the flag and the carry select nothing there.
template <template <bool> class RuleOf, typename ST, bool VARIANTS, bool GUARDED = false>
struct UpdateFamily {
  template <bool FLAG>
  using Rule = RuleOf<FLAG>;
  using State = ST;
  using Hyper = typename RuleOf<false>::Hyper;
  static constexpr bool kVariants = VARIANTS;
  static constexpr bool kGuard = GUARDED;  // GUARD instances of its CLIP kernels exist
};
template <bool>
using AdamSrRuleOf = AdamSrRule;
using AdamFamily = UpdateFamily<AdamRule, float, true, true>;
using AdamBf16Family = UpdateFamily<AdamRule, unsigned short, false, true>;  // zs_adamset_create_ex
using AdamSrFamily = UpdateFamily<AdamSrRuleOf, SrBf16, false, true>;        // zs_adamset_run_sr
using SgdFamily = UpdateFamily<SgdRule, float, true>;
// zs_lionset_run: fp32 momentum (with the carry instances; the rule has no flag), bf16 momentum to
// nearest, bf16 momentum rounded stochastically
using LionFamily = UpdateFamily<LionRule, float, true, true>;
using LionBf16Family = UpdateFamily<LionRule, unsigned short, false, true>;
using LionSrFamily = UpdateFamily<LionSrRule, SrBf16, false, true>;
template <bool>
using AdamPsrRuleOf = AdamPsrRule;
// zs_adamset_run_psr: the master-free instances, by how m and v are stored
using AdamPsrFamily = UpdateFamily<AdamPsrRuleOf, float, false, true>;
using AdamPsrBf16Family = UpdateFamily<AdamPsrRuleOf, unsigned short, false, true>;
using AdamPsrSrFamily = UpdateFamily<AdamPsrRuleOf, SrBf16, false, true>;
template <bool>
using AdamEmaRuleOf = AdamEmaRule;
// zs_adamset_run_ema: fp32 moments, no carry; every (gradient dtype, master storage) pair
using AdamEmaFamily = UpdateFamily<AdamEmaRuleOf, float, false, true>;
template <bool>
using AdamStatsRuleOf = AdamStatsRule;
// zs_adamset_run_stats: the same pairs, 24 vector + 12 scalar instances
using AdamStatsFamily = UpdateFamily<AdamStatsRuleOf, float, false, true>;

struct UpdateTable {  // a segment array with its chunk prefix
  const AdamSeg* segs;
  const int64_t* prefix;
  int64_t nseg, chunks;
};
static UpdateTable vec_table(const zs_adamset* as) {
  return {as->d_vec, as->d_vec_prefix, as->nvec, as->vec_chunks};
}
static UpdateTable sca_table(const zs_adamset* as) {
  return {as->d_sca, as->d_sca_prefix, as->nsca, as->sca_chunks};
}

// The tail of a segment from element nv on, n elements: what the vector kernel leaves to the scalar
// one.  gsz, msz, ssz: bytes per element of g, of master / master_out and of m / v / vmax.
static AdamSeg seg_tail(const AdamSeg& d, int64_t nv, int64_t n, int64_t gsz, int64_t msz,
                        int64_t ssz) {
  auto adv = [nv](auto* p, int64_t es) {
    using P = decltype(p);
    return p ? reinterpret_cast<P>(reinterpret_cast<uintptr_t>(p) + uintptr_t(nv * es)) : p;
  };
  return {adv(d.g, gsz),  adv(d.master, msz), adv(d.master_out, msz), adv(d.p_out, 2),
          adv(d.m, ssz),  adv(d.v, ssz),      adv(d.vmax, ssz),       adv(d.carry, 4),
          n};
}

// a run-time flag as a compile-time one: fn(std::true_type) or fn(std::false_type)
template <typename Fn>
static void with_flag(bool b, Fn&& fn) {
  if (b) fn(std::true_type{});
  else fn(std::false_type{});
}

// Vector table (aligned, n % 4 == 0) then scalar table (tails, unaligned); the instance of family
// F is picked by clip (a coefficient is given), split master, grad dtype, the rule's flag and
// carry, and with CLIP by guard (the guarded runs of the Adam families).  No instance has the
// carry with CLIP (the run paths refuse a set with one) or with fp32 gradients over the split
// master (set_create refuses one), and none is named here that F has not.
template <typename F>
static int launch_update_tables(const UpdateTable& vec, const UpdateTable& sca, int g_dtype,
                                bool split, bool flag, bool carry, const typename F::Hyper& hp,
                                const float* coef, hipStream_t st, bool guard = false) {
  using ST = typename F::State;
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  auto table = [&](const UpdateTable& t, auto is_vec, auto lf, int64_t cap) {
    const dim3 grid(int(std::min<int64_t>(t.chunks, cap)));
    with_flag(coef != nullptr, [&](auto clip) {
      with_flag(split, [&](auto s) {
        with_flag(g_dtype == ZS_F32, [&](auto g32) {
          using GT = std::conditional_t<decltype(g32)::value, float, unsigned short>;
          constexpr bool CLIP = decltype(clip)::value, S = decltype(s)::value;
          auto launch = [&](auto f, auto c) {
            using Rule = typename F::template Rule<decltype(f)::value>;
            constexpr bool C = decltype(c)::value;
            auto go = [&](auto gd) {
              constexpr bool GD = decltype(gd)::value;
              // the master-free families exist over the split geometry only (run_set passes it)
              if constexpr (Rule::kPsr && !S)
                return;
              else if constexpr (decltype(is_vec)::value)
                hipLaunchKernelGGL(
                    (adam_segments_kernel<Rule, GT, C, S, decltype(lf)::value, CLIP, ST, GD>), grid,
                    dim3(kThreads), 0, st, t.segs, t.prefix, t.nseg, t.chunks, hp, coef);
              else
                hipLaunchKernelGGL((adam_scalar_kernel<Rule, GT, C, S, CLIP, ST, GD>), grid,
                                   dim3(kThreads), 0, st, t.segs, t.prefix, t.nseg, t.chunks, hp,
                                   coef);
            };
            // GUARD: with CLIP, without the carry, the Adam families only (the callers refuse the
            // rest), so SGD gets no such instance
            if constexpr (CLIP && !C && F::kGuard) with_flag(guard, go);
            else go(no);
          };
          if constexpr (!F::kVariants) {
            launch(no, no);
          } else {
            if constexpr (!CLIP && !(decltype(g32)::value && S)) {
              if (carry) return with_flag(flag, [&](auto f) { launch(f, yes); });
            }
            with_flag(flag, [&](auto f) { launch(f, no); });
          }
        });
      });
    });
  };
  if (vec.chunks) {
    const bool lf = adam_loads_first() != 0;
    const int64_t cap =
        adam_grid_cap(lf && split ? kAdamLoadsFirstWgPerCu : kAdamWgPerCu);
    if (lf) table(vec, yes, yes, cap);
    else table(vec, yes, no, cap);
    ZS_HIP(hipGetLastError());
  }
  if (sca.chunks) {
    table(sca, no, no, adam_grid_cap(kAdamWgPerCu));
    ZS_HIP(hipGetLastError());
  }
  return ZS_OK;
}

// One run of a set's two tables through family F (flag: amsgrad / momentum).  The callers have
// refused a clipped run of a set with the carry.
template <typename F>
static int run_set(const zs_adamset* as, bool flag, const typename F::Hyper& hp, const float* coef,
                   uintptr_t stream, bool guard = false) {
  return launch_update_tables<F>(vec_table(as), sca_table(as), as->g_dtype, split_geometry(as),
                                 flag, as->has_carry != 0, hp, coef,
                                 reinterpret_cast<hipStream_t>(stream), guard);
}

extern "C" {

int zs_copyset_create(const uint64_t* src, const uint64_t* dst, const int64_t* nbytes, int64_t n,
                      zs_copyset** out) {
  ZS_REQUIRE(out != nullptr, "zs_copyset_create: out is NULL");
  *out = nullptr;
  ZS_REQUIRE(n >= 0, "zs_copyset_create: n < 0");
  ZS_REQUIRE(n == 0 || (src && dst && nbytes), "zs_copyset_create: NULL table");
  std::vector<CopySeg> segs;
  std::vector<int64_t> prefix(1, 0);
  int64_t bytes = 0;
  const int unroll = copy_unroll();
  const int64_t chunk = copy_chunk_bytes(unroll);
  for (int64_t i = 0; i < n; ++i) {
    ZS_REQUIRE(nbytes[i] >= 0, "zs_copyset_create: nbytes[%lld] < 0", (long long)i);
    if (nbytes[i] == 0) continue;
    ZS_REQUIRE(dst[i] != 0, "zs_copyset_create: dst[%lld] is NULL", (long long)i);
    CopySeg s;
    s.src = reinterpret_cast<const unsigned char*>(src[i]);
    s.dst = reinterpret_cast<unsigned char*>(dst[i]);
    s.nbytes = nbytes[i];
    s.vec = aligned(src[i], 16) && aligned(dst[i], 16) ? 1 : 0;
    segs.push_back(s);
    bytes += nbytes[i];
    prefix.push_back(prefix.back() + (nbytes[i] + chunk - 1) / chunk);
  }
  zs_copyset* cs = new (std::nothrow) zs_copyset();
  if (!cs) return zs::fail(ZS_ERR_NOMEM, "zs_copyset_create: out of memory");
  cs->nseg = int64_t(segs.size());
  cs->total_chunks = prefix.back();
  cs->bytes = bytes;
  cs->unroll = unroll;
  int rc = upload(segs, &cs->d_segs);
  if (rc == ZS_OK) rc = upload(prefix, &cs->d_prefix);
  if (rc != ZS_OK) {
    zs_copyset_destroy(cs);
    return rc;
  }
  *out = cs;
  return ZS_OK;
}

int zs_copyset_run(const zs_copyset* cs, uintptr_t stream) {
  ZS_REQUIRE(cs != nullptr, "zs_copyset_run: NULL set");
  if (cs->total_chunks == 0) return ZS_OK;
  const int grid = int(std::min<int64_t>(cs->total_chunks, grid_cap()));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int force = copy_nt_mode();
  const bool nt = force < 0 ? 2 * cs->bytes > kMallBytes : force == 1;
#define ZS_COPY(U, NT) hipLaunchKernelGGL((copy_segments_kernel<U, NT>), dim3(grid), dim3(kThreads), 0, st, \
                                          cs->d_segs, cs->d_prefix, cs->nseg, cs->total_chunks)
  if (nt) {
    switch (cs->unroll) { case 8: ZS_COPY(8, true); break; case 2: ZS_COPY(2, true); break; default: ZS_COPY(4, true); }
  } else {
    switch (cs->unroll) { case 8: ZS_COPY(8, false); break; case 2: ZS_COPY(2, false); break; default: ZS_COPY(4, false); }
  }
#undef ZS_COPY
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_copyset_destroy(zs_copyset* cs) {
  if (!cs) return ZS_OK;
  if (cs->d_segs) (void)hipFree(cs->d_segs);
  if (cs->d_prefix) (void)hipFree(cs->d_prefix);
  delete cs;
  return ZS_OK;
}

int zs_copy_direct(int64_t n, const uint64_t* src, const uint64_t* dst, const int64_t* nbytes,
                   uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_copy_direct: n < 0");
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(src && dst && nbytes, "zs_copy_direct: NULL table");
  int64_t total_bytes = 0;
  for (int64_t i = 0; i < n; ++i) {
    ZS_REQUIRE(nbytes[i] >= 0, "zs_copy_direct: nbytes[%lld] < 0", (long long)i);
    ZS_REQUIRE(nbytes[i] == 0 || dst[i] != 0, "zs_copy_direct: dst[%lld] is NULL", (long long)i);
    total_bytes += nbytes[i];
  }
  const int force = copy_nt_mode();
  const bool nt = force < 0 ? 2 * total_bytes > kMallBytes : force == 1;
  constexpr int U = kCopyUnrollDefault;
  const int64_t chunk = copy_chunk_bytes(U);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int64_t i0 = 0; i0 < n;) {  // launches of up to kDirectMax non-empty segments
    DirectSet set{};
    int k = 0;
    for (; i0 < n && k < kDirectMax; ++i0) {
      if (nbytes[i0] == 0) continue;
      set.src[k] = reinterpret_cast<const unsigned char*>(src[i0]);
      set.dst[k] = reinterpret_cast<unsigned char*>(dst[i0]);
      set.nbytes[k] = nbytes[i0];
      set.prefix[k + 1] = set.prefix[k] + (nbytes[i0] + chunk - 1) / chunk;
      if (aligned(src[i0], 16) && aligned(dst[i0], 16)) set.vec_mask |= uint64_t(1) << k;
      ++k;
    }
    set.n = k;
    if (k == 0) break;
    for (int j = k; j < kDirectMax; ++j) set.prefix[j + 1] = set.prefix[k];
    const int grid = int(std::min<int64_t>(set.prefix[k], grid_cap()));
    if (nt) hipLaunchKernelGGL((copy_direct_kernel<U, true>), dim3(grid), dim3(kThreads), 0, st, set);
    else hipLaunchKernelGGL((copy_direct_kernel<U, false>), dim3(grid), dim3(kThreads), 0, st, set);
    ZS_HIP(hipGetLastError());
  }
  return ZS_OK;
}

int zs_scale(void* x, int64_t n, int dtype, double div, uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_scale: n < 0");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_scale: bad dtype %d", dtype);
  ZS_REQUIRE(div != 0.0, "zs_scale: div == 0");
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(x != nullptr && aligned(reinterpret_cast<uint64_t>(x), 16),
             "zs_scale: x must be non-NULL and 16-byte aligned");
  // the reciprocal shortcut only where it is exact in fp32: div itself an fp32 power of two whose
  // reciprocal is one as well (2^-128 and below have inf there, and x * inf is not x / div)
  int e = 0;
  const float fdiv = float(div), inv = float(1.0 / div);
  const bool exact = double(fdiv) == div && std::frexp(div, &e) == 0.5 && std::isfinite(inv) &&
                     inv != 0.0f;
  const int pow2 = exact ? 1 : 0;
  const int64_t span = int64_t(64) * kScaleU * (dtype == ZS_F32 ? 4 : 8);  // elements per wave step
  const int64_t blocks = std::max<int64_t>(1, (n / span + 3) / 4);
  const int grid = int(std::min<int64_t>(blocks, grid_cap()));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int force = scale_nt_mode();
  const bool nt = force < 0 ? n * (dtype == ZS_F32 ? 4 : 2) > kMallBytes : force == 1;
#define ZS_SCALE(T, NT) hipLaunchKernelGGL((scale_kernel<T, NT>), dim3(grid), dim3(kThreads), 0, st, \
                                           static_cast<T*>(x), n, fdiv, inv, pow2)
  if (dtype == ZS_F32) {
    if (nt) ZS_SCALE(float, true); else ZS_SCALE(float, false);
  } else {
    if (nt) ZS_SCALE(unsigned short, true); else ZS_SCALE(unsigned short, false);
  }
#undef ZS_SCALE
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_accumulate(void* dst, const void* src, int64_t n, int dtype, uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_accumulate: n < 0");
  ZS_REQUIRE(dtype == ZS_F32 || dtype == ZS_BF16, "zs_accumulate: bad dtype %d", dtype);
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(dst != nullptr && src != nullptr, "zs_accumulate: NULL buffer");
  ZS_REQUIRE(aligned(reinterpret_cast<uint64_t>(dst), 16) &&
                 aligned(reinterpret_cast<uint64_t>(src), 16),
             "zs_accumulate: dst and src must be 16-byte aligned");
  const int64_t es = dtype == ZS_F32 ? 4 : 2;
  const int64_t span = int64_t(64) * kAccU * (16 / es);  // elements per wave step
  const int64_t blocks = std::max<int64_t>(1, (n / span + 3) / 4);
  const int grid = int(std::min<int64_t>(blocks, grid_cap()));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int force = accumulate_nt_mode();
  const bool nt = force < 0 ? 3 * n * es > kMallBytes : force == 1;  // by the bytes touched
#define ZS_ACC(T, NT) hipLaunchKernelGGL((accumulate_kernel<T, NT>), dim3(grid), dim3(kThreads), 0, st, \
                                         static_cast<T*>(dst), static_cast<const T*>(src), n)
  if (dtype == ZS_F32) {
    if (nt) ZS_ACC(float, true); else ZS_ACC(float, false);
  } else {
    if (nt) ZS_ACC(unsigned short, true); else ZS_ACC(unsigned short, false);
  }
#undef ZS_ACC
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_accumulate_widen(float* dst, const void* a_bf16, const void* src_bf16, int64_t n,
                        uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_accumulate_widen: n < 0");
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(dst != nullptr && src_bf16 != nullptr, "zs_accumulate_widen: NULL buffer");
  ZS_REQUIRE(aligned(reinterpret_cast<uint64_t>(dst), 16),
             "zs_accumulate_widen: dst must be 16-byte aligned");
  ZS_REQUIRE(aligned(reinterpret_cast<uint64_t>(a_bf16), 8) &&
                 aligned(reinterpret_cast<uint64_t>(src_bf16), 8),
             "zs_accumulate_widen: a and src must be 8-byte aligned");
  const bool first = a_bf16 != nullptr;
  const int64_t blocks = std::max<int64_t>(1, (n / kWidenSpan + 3) / 4);
  const int grid = int(std::min<int64_t>(blocks, grid_cap()));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int force = accumulate_nt_mode();
  const bool nt = force < 0 ? n * (first ? 8 : 10) > kMallBytes : force == 1;  // bytes touched
  const unsigned short* a = static_cast<const unsigned short*>(a_bf16);
  const unsigned short* s = static_cast<const unsigned short*>(src_bf16);
#define ZS_ACCW(F, NT) hipLaunchKernelGGL((accumulate_widen_kernel<F, NT>), dim3(grid), dim3(kThreads), 0, st, \
                                          dst, a, s, n)
  if (first) {
    if (nt) ZS_ACCW(true, true); else ZS_ACCW(true, false);
  } else {
    if (nt) ZS_ACCW(false, true); else ZS_ACCW(false, false);
  }
#undef ZS_ACCW
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n,
               uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_convert: n < 0");
  ZS_REQUIRE((src_dtype == ZS_F32 && dst_dtype == ZS_BF16) ||
                 (src_dtype == ZS_BF16 && dst_dtype == ZS_F32),
             "zs_convert: only fp32 <-> bf16 (got %d -> %d)", src_dtype, dst_dtype);
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(src && dst, "zs_convert: NULL buffer");
  const bool to_bf16 = src_dtype == ZS_F32;
  const bool vec = aligned(uint64_t(src), 16) && aligned(uint64_t(dst), 16);
  // vector path: one wave per kConvSpan-element step (4 waves per workgroup)
  const int64_t work = vec ? std::max<int64_t>(1, (n / kConvSpan + 3) / 4) : (n + kThreads - 1) / kThreads;
  const int grid = int(std::min<int64_t>(work, grid_cap()));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec) {
    const int force = convert_nt_mode();
    const bool nt = force < 0 ? n * 6 > kMallBytes : force == 1;  // by both sides' bytes
#define ZS_CONV(B, NT) hipLaunchKernelGGL((convert_kernel<B, NT>), dim3(grid), dim3(kThreads), 0, st, src, dst, n)
    if (to_bf16) {
      if (nt) ZS_CONV(true, true); else ZS_CONV(true, false);
    } else {
      if (nt) ZS_CONV(false, true); else ZS_CONV(false, false);
    }
#undef ZS_CONV
  } else {
    if (to_bf16) hipLaunchKernelGGL(convert_scalar_kernel<true>, dim3(grid), dim3(kThreads), 0, st, src, dst, n);
    else hipLaunchKernelGGL(convert_scalar_kernel<false>, dim3(grid), dim3(kThreads), 0, st, src, dst, n);
  }
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_fp8_quantize_rows(const void* src, int src_dtype, void* dst, float* scales, int64_t rows,
                         int64_t row_len, uintptr_t stream) {
  ZS_REQUIRE(rows >= 0 && row_len >= 0, "zs_fp8_quantize_rows: negative size");
  ZS_REQUIRE(src_dtype == ZS_F32 || src_dtype == ZS_BF16, "zs_fp8_quantize_rows: bad dtype %d",
             src_dtype);
  if (rows == 0 || row_len == 0) return ZS_OK;
  ZS_REQUIRE(src && dst && scales, "zs_fp8_quantize_rows: NULL buffer");
  const bool vec = row_len % 8 == 0 && aligned(uint64_t(src), 16) && aligned(uint64_t(dst), 8);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned char* q = static_cast<unsigned char*>(dst);
  if (vec) {  // wave per row, 4 rows per workgroup
    const int grid = int(std::min<int64_t>((rows + 3) / 4, grid_cap()));
    // 16-B chunks per lane the row needs: the smallest register-resident variant that holds it
    const int64_t chunks = (row_len + 64 * (src_dtype == ZS_F32 ? 4 : 8) - 1) / (64 * (src_dtype == ZS_F32 ? 4 : 8));
    const int nreg = chunks <= 8 ? 8 : chunks <= 16 ? 16 : chunks <= 32 ? 32 : 0;
#define ZS_Q(T, N, X) hipLaunchKernelGGL((fp8_quantize_rows_wave_kernel<T, N>), dim3(grid), dim3(kThreads), 0, st, X, q, scales, rows, row_len)
#define ZS_QSEL(T, X) \
    switch (nreg) { case 8: ZS_Q(T, 8, X); break; case 16: ZS_Q(T, 16, X); break; \
                    case 32: ZS_Q(T, 32, X); break; default: ZS_Q(T, 0, X); }
    if (src_dtype == ZS_F32) {
      const float* x = static_cast<const float*>(src);
      ZS_QSEL(float, x)
    } else {
      const unsigned short* x = static_cast<const unsigned short*>(src);
      ZS_QSEL(unsigned short, x)
    }
#undef ZS_QSEL
#undef ZS_Q
  } else {  // any row length / alignment: block per row, scalar accesses
    const int grid = int(std::min<int64_t>(rows, grid_cap()));
    if (src_dtype == ZS_F32)
      hipLaunchKernelGGL((fp8_quantize_rows_kernel<float>), dim3(grid), dim3(kThreads), 0, st, static_cast<const float*>(src), q, scales, rows, row_len);
    else
      hipLaunchKernelGGL((fp8_quantize_rows_kernel<unsigned short>), dim3(grid), dim3(kThreads), 0, st, static_cast<const unsigned short*>(src), q, scales, rows, row_len);
  }
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_fp8_dequantize_rows(const void* src, const float* scales, void* dst, int dst_dtype,
                           int64_t rows, int64_t row_len, uintptr_t stream) {
  ZS_REQUIRE(rows >= 0 && row_len >= 0, "zs_fp8_dequantize_rows: negative size");
  ZS_REQUIRE(dst_dtype == ZS_F32 || dst_dtype == ZS_BF16, "zs_fp8_dequantize_rows: bad dtype %d",
             dst_dtype);
  if (rows == 0 || row_len == 0) return ZS_OK;
  ZS_REQUIRE(src && dst && scales, "zs_fp8_dequantize_rows: NULL buffer");
  const int64_t n = rows * row_len;
  const bool vec = row_len % 8 == 0 && aligned(uint64_t(src), 8) && aligned(uint64_t(dst), 16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned char* q = static_cast<const unsigned char*>(src);
  if (vec) {  // the gathered kernel over one matrix of one rank: one wave per row
    ZS_REQUIRE(rows < (int64_t(1) << 31), "zs_fp8_dequantize_rows: %lld rows (max 2^31 - 1)",
               (long long)rows);
    DqSet set{};
    set.q = q;
    set.sc = scales;
    set.n = 1;
    set.cs[0] = rows;
    set.row_len[0] = row_len;
    set.dst[0] = dst;
    set.prefix[0] = 0;
    for (int k = 1; k <= kSetMax; ++k) set.prefix[k] = rows;
    const int grid = dq_grid(rows);
    launch_dequantize(set, dst_dtype, grid, st);
  } else {
    const int grid = int(std::min<int64_t>(std::max<int64_t>(1, (n + kThreads - 1) / kThreads), grid_cap()));
    if (dst_dtype == ZS_F32)
      hipLaunchKernelGGL((fp8_dequantize_rows_kernel<float>), dim3(grid), dim3(kThreads), 0, st, q, scales, static_cast<float*>(dst), n, row_len);
    else
      hipLaunchKernelGGL((fp8_dequantize_rows_kernel<unsigned short>), dim3(grid), dim3(kThreads), 0, st, q, scales, static_cast<unsigned short*>(dst), n, row_len);
  }
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_fp8_quantize_rowset(int64_t n, const uint64_t* src, const uint64_t* q, const uint64_t* scales,
                           const int64_t* rows, const int64_t* cs, const int64_t* row_len,
                           int src_dtype, uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_fp8_quantize_rowset: n < 0");
  ZS_REQUIRE(src_dtype == ZS_F32 || src_dtype == ZS_BF16, "zs_fp8_quantize_rowset: bad dtype %d",
             src_dtype);
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(src && q && scales && rows && cs && row_len, "zs_fp8_quantize_rowset: NULL table");
  const int E = src_dtype == ZS_F32 ? 4 : 8;
  for (int64_t m = 0; m < n; ++m) {
    ZS_REQUIRE(rows[m] >= 0 && cs[m] >= rows[m] && row_len[m] > 0 && row_len[m] % 8 == 0,
               "zs_fp8_quantize_rowset: matrix %lld: rows %lld, cs %lld, row_len %lld (needs "
               "0 <= rows <= cs, row_len a positive multiple of 8)", (long long)m,
               (long long)rows[m], (long long)cs[m], (long long)row_len[m]);
    ZS_REQUIRE((rows[m] == 0 || (src[m] && aligned(src[m], 16))) && (cs[m] == 0 || (q[m] &&
               aligned(q[m], 8) && scales[m] && aligned(scales[m], 4))),
               "zs_fp8_quantize_rowset: matrix %lld: src must be 16-B and q 8-B aligned",
               (long long)m);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // one launch per register class (8 / 16 / 32 resident chunks per lane, or streamed) and per
  // kSetMax matrices: a long-row matrix does not push the others into its low-occupancy variant
  auto nreg_of = [&](int64_t len) {
    const int64_t chunks = (len + 64 * E - 1) / (64 * E);
    return chunks <= 8 ? 8 : chunks <= 16 ? 16 : chunks <= 32 ? 32 : 0;
  };
  for (int cls : {8, 16, 32, 0}) {
    std::vector<int64_t> ms;
    for (int64_t m = 0; m < n; ++m)
      if (nreg_of(row_len[m]) == cls && cs[m] > 0) ms.push_back(m);
    for (size_t k0 = 0; k0 < ms.size(); k0 += kSetMax) {
      QSet set{};
      set.n = int(std::min<size_t>(kSetMax, ms.size() - k0));
      set.prefix[0] = 0;
      for (int k = 0; k < set.n; ++k) {
        const int64_t m = ms[k0 + k];
        set.src[k] = reinterpret_cast<const void*>(src[m]);
        set.q[k] = reinterpret_cast<unsigned char*>(q[m]);
        set.sc[k] = reinterpret_cast<float*>(scales[m]);
        set.rows[k] = rows[m];
        set.row_len[k] = row_len[m];
        set.prefix[k + 1] = set.prefix[k] + cs[m];
      }
      for (int k = set.n; k < kSetMax; ++k) set.prefix[k + 1] = set.prefix[set.n];
      const int64_t total = set.prefix[set.n];
      const int grid = int(std::min<int64_t>((total + 3) / 4, grid_cap()));
#define ZS_QS(T, N) hipLaunchKernelGGL((fp8_quantize_rowset_kernel<T, N>), dim3(grid), dim3(kThreads), 0, st, set)
#define ZS_QSSEL(T) \
      switch (cls) { case 8: ZS_QS(T, 8); break; case 16: ZS_QS(T, 16); break; \
                     case 32: ZS_QS(T, 32); break; default: ZS_QS(T, 0); }
      if (src_dtype == ZS_F32) { ZS_QSSEL(float) } else { ZS_QSSEL(unsigned short) }
#undef ZS_QSSEL
#undef ZS_QS
      ZS_HIP(hipGetLastError());
    }
  }
  return ZS_OK;
}

int zs_fp8_dequantize_gathered(int64_t n, const void* q, const float* scales, int ws,
                               int64_t q_rank_bytes, int64_t sc_rank_elems, const int64_t* q_off,
                               const int64_t* sc_off, const int64_t* cs, const int64_t* row_len,
                               const uint64_t* dst, int dst_dtype, uintptr_t stream) {
  ZS_REQUIRE(n >= 0 && ws >= 1, "zs_fp8_dequantize_gathered: n %lld, ws %d", (long long)n, ws);
  ZS_REQUIRE(dst_dtype == ZS_F32 || dst_dtype == ZS_BF16,
             "zs_fp8_dequantize_gathered: bad dtype %d", dst_dtype);
  if (n == 0) return ZS_OK;
  ZS_REQUIRE(q && scales && q_off && sc_off && cs && row_len && dst,
             "zs_fp8_dequantize_gathered: NULL buffer or table");
  ZS_REQUIRE(aligned(uint64_t(q), 8) && aligned(uint64_t(scales), 4) && q_rank_bytes % 8 == 0 &&
                 q_rank_bytes >= 0 && sc_rank_elems >= 0,
             "zs_fp8_dequantize_gathered: q must be 8-B aligned with an 8-B multiple rank stride");
  for (int64_t m = 0; m < n; ++m)
    ZS_REQUIRE(cs[m] >= 0 && row_len[m] > 0 && row_len[m] % 8 == 0 && q_off[m] % 8 == 0 &&
                   q_off[m] >= 0 && sc_off[m] >= 0 && (cs[m] == 0 || (dst[m] && aligned(dst[m], 16))),
               "zs_fp8_dequantize_gathered: matrix %lld: cs %lld, row_len %lld, q_off %lld (needs "
               "row_len and q_off multiples of 8, dst 16-B aligned)", (long long)m,
               (long long)cs[m], (long long)row_len[m], (long long)q_off[m]);
  for (int64_t m = 0; m < n; ++m)  // the kernel's row arithmetic is 32-bit
    ZS_REQUIRE(int64_t(ws) * cs[m] < (int64_t(1) << 31),
               "zs_fp8_dequantize_gathered: matrix %lld too large (%lld rows x %d ranks)",
               (long long)m, (long long)cs[m], ws);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  for (int64_t m0 = 0; m0 < n; m0 += kSetMax) {
    DqSet set{};
    set.q = static_cast<const unsigned char*>(q);
    set.sc = scales;
    set.q_rank = q_rank_bytes;
    set.sc_rank = sc_rank_elems;
    set.n = int(std::min<int64_t>(kSetMax, n - m0));
    set.prefix[0] = 0;
    for (int k = 0; k < set.n; ++k) {
      const int64_t m = m0 + k;
      set.q_off[k] = q_off[m];
      set.sc_off[k] = sc_off[m];
      set.cs[k] = cs[m];
      set.row_len[k] = row_len[m];
      set.dst[k] = reinterpret_cast<void*>(dst[m]);
      set.prefix[k + 1] = set.prefix[k] + int64_t(ws) * cs[m];
    }
    for (int k = set.n; k < kSetMax; ++k) set.prefix[k + 1] = set.prefix[set.n];
    const int64_t total = set.prefix[set.n];
    if (total == 0) continue;
    const int grid = dq_grid(total);
    launch_dequantize(set, dst_dtype, grid, st);
    ZS_HIP(hipGetLastError());
  }
  return ZS_OK;
}

int zs_adam_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                         int decoupled, int amsgrad, int maximize, int64_t step, double grad_div,
                         double carry_mul, zs_adam_hparams* hp) {
  ZS_REQUIRE(hp != nullptr, "zs_adam_hparams_init: hp is NULL");
  ZS_REQUIRE(step >= 1, "zs_adam_hparams_init: step must be >= 1");
  ZS_REQUIRE(grad_div > 0.0, "zs_adam_hparams_init: grad_div must be > 0");
  // adam.py:508-515 (non-capturable): Python-float (double) scalars.
  const double t = double(step);
  const double bc1 = 1.0 - std::pow(beta1, t);
  const double bc2 = 1.0 - std::pow(beta2, t);
  hp->one_minus_beta1 = float(1.0 - beta1);
  hp->beta2 = float(beta2);
  hp->one_minus_beta2 = float(1.0 - beta2);
  hp->neg_step_size = float(-(lr / bc1));
  hp->bc2_sqrt = float(std::pow(bc2, 0.5));
  hp->eps = float(eps);
  hp->weight_decay = decoupled ? 0.0f : float(weight_decay);
  hp->decay_mul = decoupled ? float(1.0 - lr * weight_decay) : 1.0f;
  hp->grad_div = float(grad_div);
  hp->carry_mul = float(carry_mul);
  hp->amsgrad = amsgrad ? 1 : 0;
  hp->maximize = maximize ? 1 : 0;
  return ZS_OK;
}

// zs_adamset_create (sgd = false), zs_sgdset_create (sgd = true: field m is the momentum buffer,
// on all segments or on none; v and vmax must be 0) and zs_lionset_create (lion = true: m on every
// segment, v and vmax 0); `fn` names the entry point in messages.
// state_dtype: the element type of m and v (ZS_BF16: zs_adamset_create_ex's bf16 moments, Lion's
// bf16 momentum).
static int set_create(const char* fn, bool sgd, const zs_adam_seg* in, int64_t n, int g_dtype,
                      int p_dtype, int state_dtype, zs_adamset** out, bool lion = false) {
  ZS_REQUIRE(out != nullptr, "%s: out is NULL", fn);
  *out = nullptr;
  ZS_REQUIRE(n >= 0 && (n == 0 || in), "%s: bad table", fn);
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "%s: bad g_dtype %d", fn, g_dtype);
  const bool psr = p_dtype == ZS_BF16_SR;  // master-free: zs_adamset_run_psr
  ZS_REQUIRE(p_dtype == ZS_BF16 || p_dtype == ZS_BF16_SPLIT || (psr && !sgd && !lion),
             "%s: p_dtype must be ZS_BF16 or ZS_BF16_SPLIT%s (got %d)", fn,
             sgd || lion ? "" : " or ZS_BF16_SR", p_dtype);
  ZS_REQUIRE(state_dtype == ZS_F32 || (state_dtype == ZS_BF16 && !sgd),
             "%s: state_dtype must be ZS_F32 or ZS_BF16 (got %d)", fn, state_dtype);
  const bool split = p_dtype == ZS_BF16_SPLIT;
  const bool geo = split || psr;      // 16-bit parameter stream, the split master's chunks
  const int64_t msz = geo ? 2 : 4;    // bytes per element of master / master_out
  const int64_t ssz = state_dtype == ZS_BF16 ? 2 : 4;  // ... of m, v (and vmax)
  const int64_t gsz = g_dtype == ZS_F32 ? 4 : 2;
  ZS_REQUIRE(n < (int64_t(1) << 31), "%s: %lld segments (max 2^31 - 1)", fn,
             (long long)n);
  std::vector<AdamSeg> vec, sca;
  std::vector<int64_t> vpre(1, 0), spre(1, 0);
  std::vector<int32_t> vec_in, sca_in;
  std::vector<int64_t> sca_goff;
  std::vector<uint64_t> in_g(size_t(n), 0);
  std::vector<int64_t> in_n(size_t(n), 0);
  std::vector<unsigned char> in_vec(size_t(n), 0);
  int carry_state = -1, vmax_state = -1, mom_state = -1, m_one_parity = 1, m_one_mod4 = 1;
  uint64_t m_lowest = ~uint64_t(0);
  int64_t elems = 0, bytes = 0, bytes_no_g = 0;
  for (int64_t i = 0; i < n; ++i) {
    const zs_adam_seg& s = in[i];
    ZS_REQUIRE(s.n >= 0, "%s: seg %lld n < 0", fn, (long long)i);
    in_g[size_t(i)] = s.g;
    in_n[size_t(i)] = s.n;
    if (s.n == 0) continue;
    if (sgd) {
      ZS_REQUIRE(s.master, "%s: seg %lld missing master", fn, (long long)i);
      ZS_REQUIRE(!s.v && !s.vmax, "%s: seg %lld: v and vmax must be 0 in an SGD set", fn,
                 (long long)i);
      const int b = s.m ? 1 : 0;
      ZS_REQUIRE(mom_state < 0 || mom_state == b,
                 "%s: m (the momentum buffer) must be set on all segments or none", fn);
      mom_state = b;
    } else if (lion) {
      ZS_REQUIRE(s.master && s.m, "%s: seg %lld missing master/m", fn, (long long)i);
      ZS_REQUIRE(!s.v && !s.vmax, "%s: seg %lld: v and vmax must be 0 in a Lion set", fn,
                 (long long)i);
    } else {
      ZS_REQUIRE(s.master && s.m && s.v, "%s: seg %lld missing master/m/v", fn, (long long)i);
    }
    ZS_REQUIRE(!split || (s.master_out && s.p_out),
               "%s: seg %lld: a split master needs master_out (residual) and p_out", fn,
               (long long)i);
    ZS_REQUIRE(!psr || (s.p_out == s.master && !s.master_out && !s.vmax && !s.carry),
               "%s: seg %lld: a ZS_BF16_SR set takes master = p_out (the bf16 param, updated in "
               "place) and no master_out, vmax or carry", fn, (long long)i);
    // fp32 gradients over a split master: ZeRO-3's fp32 accumulation arena; ZeRO-1 (the carry)
    // never has such a set, so no CARRY instance of it exists
    ZS_REQUIRE(!(split && g_dtype == ZS_F32 && s.carry),
               "%s: seg %lld: a ZS_BF16_SPLIT set with fp32 grads takes no carry", fn,
               (long long)i);
    ZS_REQUIRE(ssz == 4 || (!s.vmax && !s.carry),
               "%s: seg %lld: a set with ZS_BF16 state takes no vmax (amsgrad) and no carry", fn,
               (long long)i);
    const int c = s.carry ? 1 : 0;
    ZS_REQUIRE(carry_state < 0 || carry_state == c,
               "%s: carry must be set on all segments or none", fn);
    carry_state = c;
    const int x = s.vmax ? 1 : 0;
    ZS_REQUIRE(vmax_state < 0 || vmax_state == x,
               "%s: vmax must be set on all segments or none", fn);
    vmax_state = x;
    AdamSeg d;
    d.g = reinterpret_cast<const void*>(s.g);
    d.master = reinterpret_cast<const float*>(s.master);
    d.master_out = reinterpret_cast<float*>(s.master_out);
    d.p_out = reinterpret_cast<unsigned short*>(s.p_out);
    d.m = reinterpret_cast<float*>(s.m);
    d.v = reinterpret_cast<float*>(s.v);
    d.vmax = reinterpret_cast<float*>(s.vmax);
    d.carry = reinterpret_cast<float*>(s.carry);
    const bool ok = aligned(s.g, uint64_t(gsz) * 4) && aligned(s.master, uint64_t(msz) * 4) &&
                    aligned(s.master_out, uint64_t(msz) * 4) && aligned(s.p_out, 8) &&
                    aligned(s.m, uint64_t(ssz) * 4) && aligned(s.v, uint64_t(ssz) * 4) &&
                    aligned(s.vmax, uint64_t(ssz) * 4) && aligned(s.carry, 16);
    const int64_t nv = ok ? (s.n & ~int64_t(3)) : 0;
    if (nv) {
      d.n = nv;
      vec.push_back(d);
      vec_in.push_back(int32_t(i));
      in_vec[size_t(i)] = 1;
      vpre.push_back(vpre.back() + (nv + adam_chunk(geo) - 1) / adam_chunk(geo));
    }
    if (nv < s.n) {  // tail (or the whole unaligned segment) through the scalar kernel
      const AdamSeg t = seg_tail(d, nv, s.n - nv, gsz, msz, ssz);
      sca.push_back(t);
      sca_in.push_back(int32_t(i));
      sca_goff.push_back(nv * gsz);
      spre.push_back(spre.back() + (t.n + kThreads - 1) / kThreads);
    }
    if (m_lowest != ~uint64_t(0) && ((s.m ^ m_lowest) & 1)) m_one_parity = 0;
    if (m_lowest != ~uint64_t(0) && ((s.m ^ m_lowest) & 3)) m_one_mod4 = 0;
    m_lowest = std::min<uint64_t>(m_lowest, s.m);
    elems += s.n;
    int64_t b = msz /*master*/ + (sgd    ? (s.m ? 8 : 0) /*buffer*/
                                  : lion ? 2 * ssz /*m*/
                                         : 2 * ssz /*m*/ + 2 * ssz /*v*/);
    if (s.master_out) b += split ? 4 /*residual read + write*/ : 4;
    if (s.p_out) b += 2;
    if (s.vmax) b += 2 * ssz;
    if (s.carry) b += 8;
    bytes_no_g += b * s.n;
    bytes += (b + (s.g ? gsz : 0)) * s.n;
  }
  zs_adamset* as = new (std::nothrow) zs_adamset();
  if (!as) return zs::fail(ZS_ERR_NOMEM, "%s: out of memory", fn);
  as->nvec = int64_t(vec.size());
  as->vec_chunks = vpre.back();
  as->nsca = int64_t(sca.size());
  as->sca_chunks = spre.back();
  as->sq_vec = std::min(as->vec_chunks, kSqnormVecPartials);
  as->sq_sca = std::min(as->sca_chunks, kSqnormScaPartials);
  // the segmented pass: slots per entry from the entry's own chunks, laid out by input segment
  // (vector part, then scalar part)
  std::vector<int64_t> seg_off(size_t(n) + 1, 0);
  std::vector<int64_t> vslots(2 * vec.size() + 1, 0), sslots(2 * sca.size() + 1, 0);
  for (size_t e = 0; e < vec.size(); ++e) {
    const int64_t k = std::min(vpre[e + 1] - vpre[e], kSqnormSegVecSlots);
    vslots[e + 1] = vslots[e] + k;
    seg_off[size_t(vec_in[e]) + 1] += k;
  }
  for (size_t e = 0; e < sca.size(); ++e) {
    const int64_t k = std::min(spre[e + 1] - spre[e], kSqnormSegScaSlots);
    sslots[e + 1] = sslots[e] + k;
    seg_off[size_t(sca_in[e]) + 1] += k;
  }
  for (size_t i = 0; i < size_t(n); ++i) seg_off[i + 1] += seg_off[i];
  for (size_t e = 0; e < vec.size(); ++e)
    vslots[vec.size() + 1 + e] = seg_off[size_t(vec_in[e])];
  for (size_t e = 0; e < sca.size(); ++e)  // behind the segment's vector slots, if it has any
    sslots[sca.size() + 1 + e] = seg_off[size_t(sca_in[e]) + 1] - (sslots[e + 1] - sslots[e]);
  as->sqs_vec = vslots[vec.size()];
  as->sqs_sca = sslots[sca.size()];
  as->seg_off = std::move(seg_off);
  // the update-norm slots: 4 per chunk (one per wave), laid out the same way
  std::vector<int64_t> un_seg(size_t(n) + 1, 0), un_off(vec.size() + sca.size(), 0);
  for (size_t e = 0; e < vec.size(); ++e) un_seg[size_t(vec_in[e]) + 1] += 4 * (vpre[e + 1] - vpre[e]);
  for (size_t e = 0; e < sca.size(); ++e) un_seg[size_t(sca_in[e]) + 1] += 4 * (spre[e + 1] - spre[e]);
  for (size_t i = 0; i < size_t(n); ++i) un_seg[i + 1] += un_seg[i];
  for (size_t e = 0; e < vec.size(); ++e) un_off[e] = un_seg[size_t(vec_in[e])];
  for (size_t e = 0; e < sca.size(); ++e)
    un_off[vec.size() + e] = un_seg[size_t(sca_in[e]) + 1] - 4 * (spre[e + 1] - spre[e]);
  as->un_off = std::move(un_off);
  as->un_seg_off = std::move(un_seg);
  as->elems = elems;
  as->bytes = bytes;
  as->g_dtype = g_dtype;
  as->p_dtype = p_dtype;
  as->has_carry = carry_state > 0 ? 1 : 0;
  as->has_vmax = vmax_state > 0 ? 1 : 0;
  as->sgd = sgd ? 1 : 0;
  as->has_mom = mom_state > 0 ? 1 : 0;
  as->lion = lion ? 1 : 0;
  as->state_dtype = state_dtype;
  as->in_g = std::move(in_g);
  as->in_n = std::move(in_n);
  as->in_vec = std::move(in_vec);
  as->bytes_no_g = bytes_no_g;
  as->m_lowest = m_lowest;
  as->m_one_parity = m_one_parity;
  as->m_one_mod4 = m_one_mod4;
  int rc = ZS_OK;
  if (as->nvec) {
    rc = upload(vec, &as->d_vec);
    if (rc == ZS_OK) rc = upload(vpre, &as->d_vec_prefix);
    if (rc == ZS_OK) rc = upload(vec_in, &as->d_vec_in);
    if (rc == ZS_OK) rc = upload(vslots, &as->d_vec_slots);
  }
  if (rc == ZS_OK && as->nsca) {
    rc = upload(sca, &as->d_sca);
    if (rc == ZS_OK) rc = upload(spre, &as->d_sca_prefix);
    if (rc == ZS_OK) rc = upload(sca_in, &as->d_sca_in);
    if (rc == ZS_OK) rc = upload(sca_goff, &as->d_sca_goff);
    if (rc == ZS_OK) rc = upload(sslots, &as->d_sca_slots);
  }
  if (rc != ZS_OK) {
    zs_adamset_destroy(as);
    return rc;
  }
  *out = as;
  return ZS_OK;
}

int zs_adamset_create(const zs_adam_seg* in, int64_t n, int g_dtype, int p_dtype,
                      zs_adamset** out) {
  return set_create("zs_adamset_create", false, in, n, g_dtype, p_dtype, ZS_F32, out);
}

int zs_adamset_create_ex(const zs_adam_seg* in, int64_t n, int g_dtype, int p_dtype,
                         int state_dtype, zs_adamset** out) {
  return set_create("zs_adamset_create_ex", false, in, n, g_dtype, p_dtype, state_dtype, out);
}

int zs_sgdset_create(const zs_adam_seg* in, int64_t n, int g_dtype, int p_dtype,
                     zs_adamset** out) {
  return set_create("zs_sgdset_create", true, in, n, g_dtype, p_dtype, ZS_F32, out);
}

int zs_sgd_hparams_init(double lr, double momentum, double dampening, double weight_decay,
                        int nesterov, int maximize, int first, double grad_div, double carry_mul,
                        zs_sgd_hparams* hp) {
  ZS_REQUIRE(hp != nullptr, "zs_sgd_hparams_init: hp is NULL");
  ZS_REQUIRE(grad_div > 0.0, "zs_sgd_hparams_init: grad_div must be > 0");
  // sgd.py SGD.__init__'s rules
  ZS_REQUIRE(lr >= 0.0, "zs_sgd_hparams_init: invalid learning rate %g", lr);
  ZS_REQUIRE(momentum >= 0.0, "zs_sgd_hparams_init: invalid momentum %g", momentum);
  ZS_REQUIRE(weight_decay >= 0.0, "zs_sgd_hparams_init: invalid weight_decay %g", weight_decay);
  ZS_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0),
             "zs_sgd_hparams_init: Nesterov momentum requires a momentum and zero dampening");
  hp->neg_lr = float(-lr);
  hp->momentum = float(momentum);
  hp->one_minus_dampening = float(1.0 - dampening);
  hp->weight_decay = float(weight_decay);
  hp->grad_div = float(grad_div);
  hp->carry_mul = float(carry_mul);
  hp->nesterov = nesterov ? 1 : 0;
  hp->maximize = maximize ? 1 : 0;
  hp->first = first ? 1 : 0;
  return ZS_OK;
}

int zs_sgdset_run(const zs_adamset* as, const zs_sgd_hparams* h, const float* coef,
                  uintptr_t stream) {
  ZS_REQUIRE(as && h, "zs_sgdset_run: NULL argument");
  ZS_REQUIRE(!as->lion, "zs_sgdset_run: the set was made by zs_lionset_create (use zs_lionset_run)");
  ZS_REQUIRE(as->sgd, "zs_sgdset_run: the set was made by zs_adamset_create (use zs_adamset_run)");
  // a struct filled by hand gets zs_sgd_hparams_init's rules too (-0.0f is lr = 0)
  ZS_REQUIRE(h->neg_lr <= 0.0f, "zs_sgdset_run: negative learning rate");
  ZS_REQUIRE(h->momentum >= 0.0f, "zs_sgdset_run: invalid momentum %g", double(h->momentum));
  ZS_REQUIRE(h->weight_decay >= 0.0f, "zs_sgdset_run: invalid weight_decay %g",
             double(h->weight_decay));
  ZS_REQUIRE(h->grad_div > 0.0f, "zs_sgdset_run: grad_div must be > 0");
  ZS_REQUIRE(!h->nesterov || (h->momentum > 0.0f && h->one_minus_dampening == 1.0f),
             "zs_sgdset_run: Nesterov momentum requires a momentum and zero dampening");
  ZS_REQUIRE(h->momentum == 0.0f || as->has_mom || (as->nvec + as->nsca) == 0,
             "zs_sgdset_run: momentum %g on a set without momentum buffers", double(h->momentum));
  ZS_REQUIRE(!coef || !as->has_carry,
             "zs_sgdset_run: a set with the ZeRO-1 carry cannot be clipped");
  SgdHP hp;
  hp.neg_lr = h->neg_lr;
  hp.momentum = h->momentum;
  hp.omd = h->one_minus_dampening;
  hp.wd = h->weight_decay;
  hp.carry_mul = h->carry_mul;
  set_grad_div(&hp, h->grad_div);
  hp.nesterov = h->nesterov ? 1 : 0;
  hp.maximize = h->maximize ? 1 : 0;
  hp.first = h->first ? 1 : 0;
  // torch with momentum == 0 never makes a buffer: a set that has one leaves it alone then
  return run_set<SgdFamily>(as, as->has_mom != 0 && h->momentum != 0.0f, hp, coef, stream);
}

int zs_lionset_create(const zs_adam_seg* in, int64_t n, int g_dtype, int p_dtype, int state_dtype,
                      zs_adamset** out) {
  return set_create("zs_lionset_create", false, in, n, g_dtype, p_dtype, state_dtype, out, true);
}

int zs_lion_hparams_init(double lr, double beta1, double beta2, double weight_decay, int maximize,
                         double grad_div, double carry_mul, zs_lion_hparams* hp) {
  ZS_REQUIRE(hp != nullptr, "zs_lion_hparams_init: hp is NULL");
  ZS_REQUIRE(grad_div > 0.0, "zs_lion_hparams_init: grad_div must be > 0");
  // zero_amd.optim.Lion.__init__'s rules
  ZS_REQUIRE(lr >= 0.0, "zs_lion_hparams_init: invalid learning rate %g", lr);
  ZS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "zs_lion_hparams_init: invalid beta1 %g", beta1);
  ZS_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "zs_lion_hparams_init: invalid beta2 %g", beta2);
  ZS_REQUIRE(weight_decay >= 0.0, "zs_lion_hparams_init: invalid weight_decay %g", weight_decay);
  hp->neg_lr = float(-lr);
  hp->beta1 = float(beta1);
  hp->one_minus_beta1 = float(1.0 - beta1);
  hp->beta2 = float(beta2);
  hp->one_minus_beta2 = float(1.0 - beta2);
  hp->decay_mul = weight_decay != 0.0 ? float(1.0 - lr * weight_decay) : 1.0f;
  hp->grad_div = float(grad_div);
  hp->carry_mul = float(carry_mul);
  hp->maximize = maximize ? 1 : 0;
  return ZS_OK;
}

int zs_lionset_run(const zs_adamset* as, const zs_lion_hparams* h, const float* coef, int guard,
                   uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream) {
  const char* fn = "zs_lionset_run";
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(as->lion, "%s: the set was not made by zs_lionset_create", fn);
  ZS_REQUIRE(!guard || coef, "%s: the guard tests the clip coefficient, which is NULL", fn);
  // a struct filled by hand gets zs_lion_hparams_init's rules too (-0.0f is lr = 0)
  ZS_REQUIRE(h->neg_lr <= 0.0f, "%s: negative learning rate", fn);
  ZS_REQUIRE(h->beta1 >= 0.0f && h->beta1 <= 1.0f && h->beta2 >= 0.0f && h->beta2 <= 1.0f,
             "%s: invalid betas (%g, %g)", fn, double(h->beta1), double(h->beta2));
  ZS_REQUIRE(h->grad_div > 0.0f, "%s: grad_div must be > 0", fn);
  ZS_REQUIRE(!coef || !as->has_carry, "%s: a set with the ZeRO-1 carry cannot be clipped", fn);
  LionSrHP hp;
  hp.beta1 = h->beta1;
  hp.omb1 = h->one_minus_beta1;
  hp.beta2 = h->beta2;
  hp.omb2 = h->one_minus_beta2;
  hp.neg_lr = h->neg_lr;
  hp.decay_mul = h->decay_mul;
  hp.carry_mul = h->carry_mul;
  set_grad_div(&hp, h->grad_div);
  hp.maximize = h->maximize ? 1 : 0;
  hp.k0 = key0;
  hp.k1 = key1;
  hp.m_base = m_base;
  const bool g = guard != 0;
  if (as->state_dtype != ZS_BF16)
    return run_set<LionFamily>(as, false, static_cast<const LionHP&>(hp), coef, stream, g);
  if (!as->state_sr)
    return run_set<LionBf16Family>(as, false, static_cast<const LionHP&>(hp), coef, stream, g);
  if (as->nvec + as->nsca) {  // every element's index: its m address less m_base, in elements
    ZS_REQUIRE(as->m_lowest >= m_base, "%s: a segment's m lies below m_base (%#llx < %#llx)", fn,
               (unsigned long long)as->m_lowest, (unsigned long long)m_base);
    ZS_REQUIRE(as->m_one_parity && ((as->m_lowest - m_base) & 1) == 0,
               "%s: a segment's m lies at an odd byte distance from m_base", fn);
  }
  return run_set<LionSrFamily>(as, false, hp, coef, stream, g);
}

// The three Adam entry points (`fn`: the one called, in messages).  need_coef: zs_adamset_run_clipped
// requires its coefficient; sr: zs_adamset_run_sr's m_base and keys, over a set with bf16 moments.
struct SrArgs {
  uint64_t m_base;
  uint32_t k0, k1;
};
static int adam_run(const char* fn, const zs_adamset* as, const zs_adam_hparams* h, bool need_coef,
                    const float* coef, const SrArgs* sr, uintptr_t stream, bool guard = false) {
  ZS_REQUIRE(as && h && (coef || !need_coef), "%s: NULL argument", fn);
  ZS_REQUIRE(!as->lion, "%s: the set was made by zs_lionset_create (use zs_lionset_run)", fn);
  ZS_REQUIRE(!guard || !as->sgd, "%s: the guarded update is Adam's (the set was made by "
             "zs_sgdset_create)", fn);
  ZS_REQUIRE(!sr || (!as->sgd && as->state_dtype == ZS_BF16),
             "%s: stochastic rounding needs an Adam set with ZS_BF16 state (zs_adamset_create_ex)",
             fn);
  ZS_REQUIRE(!as->sgd, "%s: the set was made by zs_sgdset_create (use zs_sgdset_run)", fn);
  ZS_REQUIRE(as->p_dtype != ZS_BF16_SR, "%s: a ZS_BF16_SR set runs through zs_adamset_run_psr", fn);
  ZS_REQUIRE(!coef || !as->has_carry, "%s: a set with the ZeRO-1 carry cannot be clipped", fn);
  const bool ams = h->amsgrad != 0;
  const bool bf16_state = as->state_dtype == ZS_BF16;
  ZS_REQUIRE(!ams || !bf16_state, "%s: a set with ZS_BF16 state has no amsgrad", fn);
  ZS_REQUIRE(!ams || as->has_vmax || (as->nvec + as->nsca) == 0, "%s: amsgrad needs vmax segments",
             fn);
  if (!sr) {
    if (bf16_state) return run_set<AdamBf16Family>(as, false, make_hp(h), coef, stream, guard);
    return run_set<AdamFamily>(as, ams, make_hp(h), coef, stream, guard);
  }
  if (as->nvec + as->nsca) {  // every element's index: its m address less m_base, in elements
    ZS_REQUIRE(as->m_lowest >= sr->m_base, "%s: a segment's m lies below m_base (%#llx < %#llx)", fn,
               (unsigned long long)as->m_lowest, (unsigned long long)sr->m_base);
    ZS_REQUIRE(as->m_one_parity && ((as->m_lowest - sr->m_base) & 1) == 0,
               "%s: a segment's m lies at an odd byte distance from m_base", fn);
  }
  SrHP hp;
  static_cast<HP&>(hp) = make_hp(h);
  hp.k0 = sr->k0;
  hp.k1 = sr->k1;
  hp.m_base = sr->m_base;
  return run_set<AdamSrFamily>(as, false, hp, coef, stream, guard);
}

int zs_adamset_run(const zs_adamset* as, const zs_adam_hparams* h, uintptr_t stream) {
  return adam_run("zs_adamset_run", as, h, false, nullptr, nullptr, stream);
}

int zs_adamset_run_clipped(const zs_adamset* as, const zs_adam_hparams* h, const float* coef,
                           uintptr_t stream) {
  return adam_run("zs_adamset_run_clipped", as, h, true, coef, nullptr, stream);
}

int zs_adamset_run_sr(const zs_adamset* as, const zs_adam_hparams* h, const float* coef,
                      uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream) {
  const SrArgs sr = {m_base, key0, key1};
  return adam_run("zs_adamset_run_sr", as, h, false, coef, &sr, stream);
}

int zs_adamset_run_guarded(const zs_adamset* as, const zs_adam_hparams* h, const float* coef,
                           uintptr_t stream) {
  return adam_run("zs_adamset_run_guarded", as, h, true, coef, nullptr, stream, true);
}

int zs_adamset_run_sr_guarded(const zs_adamset* as, const zs_adam_hparams* h, const float* coef,
                              uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream) {
  const SrArgs sr = {m_base, key0, key1};
  return adam_run("zs_adamset_run_sr_guarded", as, h, true, coef, &sr, stream, true);
}

int zs_adamset_run_psr(const zs_adamset* as, const zs_adam_hparams* h, const float* coef, int guard,
                       uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream) {
  const char* fn = "zs_adamset_run_psr";
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(as->p_dtype == ZS_BF16_SR && !as->sgd && !as->lion,
             "%s: the set was not made with p_dtype ZS_BF16_SR (zs_adamset_create_ex)", fn);
  ZS_REQUIRE(!guard || coef, "%s: the guard tests the clip coefficient, which is NULL", fn);
  ZS_REQUIRE(h->amsgrad == 0, "%s: a ZS_BF16_SR set has no amsgrad", fn);
  const bool bf16_state = as->state_dtype == ZS_BF16;
  if (as->nvec + as->nsca) {  // every element's index: its m address less m_base, in elements
    ZS_REQUIRE(as->m_lowest >= m_base, "%s: a segment's m lies below m_base (%#llx < %#llx)", fn,
               (unsigned long long)as->m_lowest, (unsigned long long)m_base);
    const uint64_t mask = bf16_state ? 1 : 3;
    ZS_REQUIRE((bf16_state ? as->m_one_parity : as->m_one_mod4) &&
                   ((as->m_lowest - m_base) & mask) == 0,
               "%s: a segment's m is not a whole number of elements from m_base", fn);
  }
  PsrHP hp;
  static_cast<HP&>(hp) = make_hp(h);
  hp.k0 = key0;
  hp.k1 = key1;
  hp.m_base = m_base;
  zs_sr::pkeys(key0, key1, &hp.kp0, &hp.kp1);
  if (!bf16_state) return run_set<AdamPsrFamily>(as, false, hp, coef, stream, guard != 0);
  if (!as->state_sr) return run_set<AdamPsrBf16Family>(as, false, hp, coef, stream, guard != 0);
  return run_set<AdamPsrSrFamily>(as, false, hp, coef, stream, guard != 0);
}

int zs_adamset_run_ema(const zs_adamset* as, const zs_adam_hparams* h, const float* coef, int guard,
                       float ema_weight, uintptr_t stream) {
  const char* fn = "zs_adamset_run_ema";
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(!as->sgd, "%s: the EMA rides on Adam's update (the set was made by zs_sgdset_create)",
             fn);
  ZS_REQUIRE(!as->lion, "%s: the EMA rides on Adam's update (the set was made by "
             "zs_lionset_create)", fn);
  ZS_REQUIRE(as->state_dtype == ZS_F32, "%s: a set with ZS_BF16 state has no EMA column", fn);
  ZS_REQUIRE(as->p_dtype != ZS_BF16_SR, "%s: a ZS_BF16_SR set has no master to average", fn);
  ZS_REQUIRE(!as->has_carry, "%s: a set with the ZeRO-1 carry has no EMA instances", fn);
  ZS_REQUIRE(as->has_vmax || (as->nvec + as->nsca) == 0,
             "%s: the EMA array is the segments' vmax column, which this set lacks", fn);
  ZS_REQUIRE(h->amsgrad == 0, "%s: amsgrad and the EMA share the vmax column", fn);
  ZS_REQUIRE(!guard || coef, "%s: the guard tests the clip coefficient, which is NULL", fn);
  ZS_REQUIRE(ema_weight >= 0.0f && ema_weight <= 1.0f,  // false for a NaN
             "%s: ema_weight must lie in [0, 1]", fn);
  EmaHP hp;
  static_cast<HP&>(hp) = make_hp(h);
  hp.ema_hi = ema_weight < 0.5f ? 0 : 1;  // ATen's lerp, as make_hp for exp_avg
  hp.ema_w = hp.ema_hi ? ema_weight - 1.0f : ema_weight;
  return run_set<AdamEmaFamily>(as, false, hp, coef, stream, guard != 0);
}

int zs_adamset_update_norm_slots(const zs_adamset* as, int64_t* n, int64_t* seg_off) {
  ZS_REQUIRE(as && n && seg_off, "zs_adamset_update_norm_slots: NULL argument");
  *n = as->un_seg_off.back();
  std::copy(as->un_seg_off.begin(), as->un_seg_off.end(), seg_off);
  return ZS_OK;
}

int zs_adamset_run_stats(const zs_adamset* as, const zs_adam_hparams* h, const float* coef,
                         int guard, double* partials, uintptr_t stream) {
  const char* fn = "zs_adamset_run_stats";
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(!as->sgd, "%s: the norms ride on Adam's update (the set was made by zs_sgdset_create)",
             fn);
  ZS_REQUIRE(!as->lion, "%s: the norms ride on Adam's update (the set was made by "
             "zs_lionset_create)", fn);
  ZS_REQUIRE(as->state_dtype == ZS_F32, "%s: a set with ZS_BF16 state has no stats instances", fn);
  ZS_REQUIRE(as->p_dtype != ZS_BF16_SR, "%s: a ZS_BF16_SR set has no master to measure", fn);
  ZS_REQUIRE(!as->has_carry, "%s: a set with the ZeRO-1 carry has no stats instances", fn);
  ZS_REQUIRE(!as->has_vmax, "%s: a set with the vmax column (amsgrad, EMA) has no stats instances",
             fn);
  ZS_REQUIRE(h->amsgrad == 0, "%s: amsgrad has no stats instances", fn);
  ZS_REQUIRE(!guard || coef, "%s: the guard tests the clip coefficient, which is NULL", fn);
  const int64_t nslots = as->un_seg_off.back();
  ZS_REQUIRE(partials != nullptr || nslots == 0, "%s: partials is NULL", fn);
  if (nslots && !as->d_un_off) {  // first use: the per-entry slot offsets
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!as->d_un_off) {
      const int rc = upload(as->un_off, &as->d_un_off);
      if (rc != ZS_OK) return rc;
    }
  }
  StatsHP hp;
  static_cast<HP&>(hp) = make_hp(h);
  hp.planes = partials;
  hp.nslots = nslots;
  hp.vec_off = as->d_un_off;
  hp.sca_off = as->d_un_off ? as->d_un_off + as->nvec : nullptr;
  return run_set<AdamStatsFamily>(as, false, hp, coef, stream, guard != 0);
}

int zs_update_norms(const float* sums3, int64_t n_params, const float* coef, float* update_norms,
                    float* weight_norms, uintptr_t stream) {
  ZS_REQUIRE(n_params >= 0 && (n_params == 0 || (sums3 && update_norms && weight_norms)),
             "zs_update_norms: %lld parameters at NULL", (long long)n_params);
  if (n_params == 0) return ZS_OK;
  const int grid = int(std::min<int64_t>((n_params + kThreads - 1) / kThreads, 1024));
  hipLaunchKernelGGL(update_norms_kernel, dim3(grid), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), sums3, n_params, coef, update_norms,
                     weight_norms);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_adamset_set_state_rounding(zs_adamset* as, int stochastic) {
  ZS_REQUIRE(as != nullptr, "zs_adamset_set_state_rounding: NULL set");
  ZS_REQUIRE((as->p_dtype == ZS_BF16_SR || as->lion) && as->state_dtype == ZS_BF16,
             "zs_adamset_set_state_rounding: a ZS_BF16_SR set or a Lion set, with ZS_BF16 state "
             "only (other sets choose by entry point: zs_adamset_run / zs_adamset_run_sr)");
  as->state_sr = stochastic ? 1 : 0;
  return ZS_OK;
}

int zs_adamset_sqnorm_partials(const zs_adamset* as, int64_t* n) {
  ZS_REQUIRE(as && n, "zs_adamset_sqnorm_partials: NULL argument");
  *n = as->sq_vec + as->sq_sca;
  return ZS_OK;
}

int zs_adamset_grad_sqnorm(const zs_adamset* as, double* partials, uintptr_t stream) {
  ZS_REQUIRE(as != nullptr, "zs_adamset_grad_sqnorm: NULL set");
  ZS_REQUIRE(partials != nullptr || as->sq_vec + as->sq_sca == 0,
             "zs_adamset_grad_sqnorm: partials is NULL");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool f32 = as->g_dtype == ZS_F32, split = split_geometry(as);
  if (as->sq_vec) {
#define ZS_SQ(GT, S, NT)                                                                      \
  hipLaunchKernelGGL((grad_sqnorm_kernel<GT, S, NT>), dim3(int(as->sq_vec)), dim3(kThreads), 0, \
                     st, as->d_vec, as->d_vec_prefix, as->nvec, as->vec_chunks, partials)
    if (sqnorm_nt()) {
      if (f32 && split) ZS_SQ(float, true, true);
      else if (f32) ZS_SQ(float, false, true);
      else if (split) ZS_SQ(unsigned short, true, true);
      else ZS_SQ(unsigned short, false, true);
    } else {
      if (f32 && split) ZS_SQ(float, true, false);
      else if (f32) ZS_SQ(float, false, false);
      else if (split) ZS_SQ(unsigned short, true, false);
      else ZS_SQ(unsigned short, false, false);
    }
#undef ZS_SQ
    ZS_HIP(hipGetLastError());
  }
  if (as->sq_sca) {
    if (f32)
      hipLaunchKernelGGL(grad_sqnorm_scalar_kernel<float>, dim3(int(as->sq_sca)), dim3(kThreads),
                         0, st, as->d_sca, as->d_sca_prefix, as->nsca, as->sca_chunks,
                         partials + as->sq_vec);
    else
      hipLaunchKernelGGL(grad_sqnorm_scalar_kernel<unsigned short>, dim3(int(as->sq_sca)),
                         dim3(kThreads), 0, st, as->d_sca, as->d_sca_prefix, as->nsca,
                         as->sca_chunks, partials + as->sq_vec);
    ZS_HIP(hipGetLastError());
  }
  return ZS_OK;
}

int zs_sqnorm_reduce(const double* partials, int64_t n, float* sumsq, uintptr_t stream) {
  ZS_REQUIRE(sumsq != nullptr, "zs_sqnorm_reduce: sumsq is NULL");
  ZS_REQUIRE(n >= 0 && (n == 0 || partials), "zs_sqnorm_reduce: %lld partials at NULL",
             (long long)n);
  hipLaunchKernelGGL(sqnorm_reduce_kernel, dim3(1), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), partials, n, sumsq);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_adamset_sqnorm_seg_partials(const zs_adamset* as, int64_t* n, int64_t* seg_off) {
  ZS_REQUIRE(as && n && seg_off, "zs_adamset_sqnorm_seg_partials: NULL argument");
  *n = as->sqs_vec + as->sqs_sca;
  std::copy(as->seg_off.begin(), as->seg_off.end(), seg_off);
  return ZS_OK;
}

int zs_adamset_grad_sqnorm_segs(const zs_adamset* as, double* partials, uintptr_t stream) {
  ZS_REQUIRE(as != nullptr, "zs_adamset_grad_sqnorm_segs: NULL set");
  ZS_REQUIRE(partials != nullptr || as->sqs_vec + as->sqs_sca == 0,
             "zs_adamset_grad_sqnorm_segs: partials is NULL");
  ZS_REQUIRE(as->sqs_vec < (int64_t(1) << 31) && as->sqs_sca < (int64_t(1) << 31),
             "zs_adamset_grad_sqnorm_segs: more than 2^31 - 1 slots in one table");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool f32 = as->g_dtype == ZS_F32, split = split_geometry(as);
  if (as->sqs_vec) {
#define ZS_SQ(GT, S, NT)                                                                   \
  hipLaunchKernelGGL((grad_sqnorm_segs_kernel<GT, S, NT>), dim3(int(as->sqs_vec)),         \
                     dim3(kThreads), 0, st, as->d_vec, as->d_vec_slots,                    \
                     as->d_vec_slots + as->nvec + 1, as->nvec, partials)
    if (sqnorm_nt()) {
      if (f32 && split) ZS_SQ(float, true, true);
      else if (f32) ZS_SQ(float, false, true);
      else if (split) ZS_SQ(unsigned short, true, true);
      else ZS_SQ(unsigned short, false, true);
    } else {
      if (f32 && split) ZS_SQ(float, true, false);
      else if (f32) ZS_SQ(float, false, false);
      else if (split) ZS_SQ(unsigned short, true, false);
      else ZS_SQ(unsigned short, false, false);
    }
#undef ZS_SQ
    ZS_HIP(hipGetLastError());
  }
  if (as->sqs_sca) {
    if (f32)
      hipLaunchKernelGGL(grad_sqnorm_segs_scalar_kernel<float>, dim3(int(as->sqs_sca)),
                         dim3(kThreads), 0, st, as->d_sca, as->d_sca_slots,
                         as->d_sca_slots + as->nsca + 1, as->nsca, partials);
    else
      hipLaunchKernelGGL(grad_sqnorm_segs_scalar_kernel<unsigned short>, dim3(int(as->sqs_sca)),
                         dim3(kThreads), 0, st, as->d_sca, as->d_sca_slots,
                         as->d_sca_slots + as->nsca + 1, as->nsca, partials);
    ZS_HIP(hipGetLastError());
  }
  return ZS_OK;
}

int zs_sqnorm_reduce_params(const double* partials, const int64_t* row_ptr, const int64_t* slot_lo,
                            const int64_t* slot_n, int64_t n_params, float* out,
                            uintptr_t stream) {
  ZS_REQUIRE(n_params >= 0 && n_params < (int64_t(1) << 31),
             "zs_sqnorm_reduce_params: %lld parameters", (long long)n_params);
  // (partials, slot_lo and slot_n may be NULL when no parameter has a range)
  ZS_REQUIRE(row_ptr && out, "zs_sqnorm_reduce_params: NULL argument");
  if (n_params == 0) return ZS_OK;
  hipLaunchKernelGGL(sqnorm_reduce_params_kernel, dim3(int(n_params)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), partials, row_ptr, slot_lo, slot_n,
                     out);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_param_norms(const float* sumsq_vec, int64_t n, double grad_div, float* norms,
                   uintptr_t stream) {
  ZS_REQUIRE(n >= 0 && (n == 0 || (sumsq_vec && norms)), "zs_param_norms: %lld elements at NULL",
             (long long)n);
  ZS_REQUIRE(grad_div > 0.0, "zs_param_norms: grad_div must be > 0");
  if (n == 0) return ZS_OK;
  const int grid = int(std::min<int64_t>((n + kThreads - 1) / kThreads, 1024));
  hipLaunchKernelGGL(param_norms_kernel, dim3(grid), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), sumsq_vec, n, grad_div, norms);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_clip_coef(const float* sumsq, double grad_div, double max_norm, float* out2,
                 uintptr_t stream) {
  ZS_REQUIRE(sumsq && out2, "zs_clip_coef: NULL argument");
  ZS_REQUIRE(grad_div > 0.0, "zs_clip_coef: grad_div must be > 0");
  ZS_REQUIRE(max_norm >= 0.0, "zs_clip_coef: max_norm must be >= 0 (infinity allowed), not NaN");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), sumsq, grad_div, float(max_norm), out2);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int zs_clip_coef_guarded(const float* sumsq, double grad_div, double max_norm, float* out2,
                         uint64_t* skipped, uintptr_t stream) {
  ZS_REQUIRE(sumsq && out2 && skipped, "zs_clip_coef_guarded: NULL argument");
  ZS_REQUIRE(grad_div > 0.0, "zs_clip_coef_guarded: grad_div must be > 0");
  ZS_REQUIRE(max_norm >= 0.0,
             "zs_clip_coef_guarded: max_norm must be >= 0 (infinity allowed), not NaN");
  hipLaunchKernelGGL(clip_coef_guarded_kernel, dim3(1), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), sumsq, grad_div, float(max_norm), out2,
                     reinterpret_cast<unsigned long long*>(skipped));
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

// zs_adam_step: one contiguous range through the same kernels.  Its two one-entry tables
// (vector part + tail) are written on the caller's stream by a one-thread kernel into a
// stream-ordered allocation, so the call neither synchronises nor keeps state between calls.
int zs_adam_step_ex(float* p, uint16_t* p_bf16, const void* g, int g_dtype, float* m, float* v,
                    int64_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int decoupled, int64_t step, double grad_div, float* carry,
                    double carry_mul, uintptr_t stream) {
  ZS_REQUIRE(n >= 0, "zs_adam_step_ex: n < 0");
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "zs_adam_step_ex: bad g_dtype %d", g_dtype);
  ZS_REQUIRE(n == 0 || (p && m && v), "zs_adam_step_ex: p, m and v must be non-NULL");
  zs_adam_hparams h;
  int rc = zs_adam_hparams_init(lr, beta1, beta2, eps, weight_decay, decoupled, 0, 0, step,
                                grad_div, carry_mul, &h);
  if (rc != ZS_OK) return rc;
  if (n == 0) return ZS_OK;
  const int64_t gsz = g_dtype == ZS_F32 ? 4 : 2;
  const uint64_t up = reinterpret_cast<uint64_t>(p), ug = reinterpret_cast<uint64_t>(g);
  const uint64_t ub = reinterpret_cast<uint64_t>(p_bf16), um = reinterpret_cast<uint64_t>(m);
  const uint64_t uv = reinterpret_cast<uint64_t>(v), uc = reinterpret_cast<uint64_t>(carry);
  const bool ok = aligned(ug, uint64_t(gsz) * 4) && aligned(up, 16) && aligned(ub, 8) &&
                  aligned(um, 16) && aligned(uv, 16) && aligned(uc, 16);
  const int64_t nv = ok ? (n & ~int64_t(3)) : 0;
  AdamTables t;
  AdamSeg& a = t.seg[0];
  a.g = g;
  a.master = p;
  a.master_out = p;
  a.p_out = reinterpret_cast<unsigned short*>(p_bf16);
  a.m = m;
  a.v = v;
  a.vmax = nullptr;
  a.carry = carry;
  a.n = nv;
  t.seg[1] = seg_tail(a, nv, n - nv, gsz, 4, 4);
  const int64_t vch = (nv + adam_chunk(false) - 1) / adam_chunk(false);
  const int64_t sch = (n - nv + kThreads - 1) / kThreads;
  t.prefix[0] = 0;
  t.prefix[1] = vch;
  t.prefix[2] = 0;
  t.prefix[3] = sch;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  AdamTables* d = nullptr;
  ZS_HIP(hipMallocAsync(reinterpret_cast<void**>(&d), sizeof(AdamTables), st));
  hipLaunchKernelGGL(write_tables_kernel, dim3(1), dim3(1), 0, st, d, t);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    rc = launch_update_tables<AdamFamily>({d->seg, d->prefix, 1, vch},
                                          {d->seg + 1, d->prefix + 2, 1, sch}, g_dtype, false, false,
                                          carry != nullptr, make_hp(&h), nullptr, st);
  }
  const hipError_t ef = hipFreeAsync(d, st);  // after the launches, in stream order
  if (e != hipSuccess)
    return zs::fail(ZS_ERR_HIP, "zs_adam_step_ex: table kernel: %s", hipGetErrorString(e));
  if (rc != ZS_OK) return rc;
  ZS_HIP(ef);
  return ZS_OK;
}

// SURVEY.md §8(b)'s literal signature: float scalars and grad_scale = 1/ws.  The divisor is the
// integer nearest to 1/grad_scale when that is within float(1/ws)'s rounding (2^-24 relative) —
// the world size, so the update divides as zero1.py:84 `p.grad /= ws` does — else 1/grad_scale;
// the scalars are widened to double before torch's bias-correction arithmetic.  carry is read and
// rewritten (A_{t-1} -> A_t) although the reference signature spells it const.
int zs_adam_step(float* p, uint16_t* p_bf16, const void* g, int g_dtype, float* m, float* v,
                 int64_t n, float lr, float b1, float b2, float eps, float wd, int decoupled,
                 int64_t step, float grad_scale, float* carry, float carry_scale,
                 uintptr_t stream) {
  ZS_REQUIRE(grad_scale > 0.0f && std::isfinite(grad_scale), "zs_adam_step: grad_scale must be > 0");
  const double r = 1.0 / double(grad_scale), k = std::nearbyint(r);
  const double div = (k >= 1.0 && std::fabs(r - k) <= 1e-6 * k) ? k : r;
  return zs_adam_step_ex(p, p_bf16, g, g_dtype, m, v, n, lr, b1, b2, eps, wd, decoupled, step, div,
                         carry, carry_scale, stream);
}

int zs_adamset_set_grads(zs_adamset* as, int64_t n, const uint64_t* g, uintptr_t stream) {
  ZS_REQUIRE(as != nullptr, "zs_adamset_set_grads: NULL set");
  ZS_REQUIRE(n == int64_t(as->in_g.size()),
             "zs_adamset_set_grads: %lld gradients for a set of %lld segments", (long long)n,
             (long long)as->in_g.size());
  ZS_REQUIRE(n == 0 || g != nullptr, "zs_adamset_set_grads: NULL table");
  const uint64_t galign = as->g_dtype == ZS_F32 ? 16 : 8;
  int64_t lo = n, hi = -1, g_elems = 0;
  for (int64_t i = 0; i < n; ++i) {
    // the set's vector / scalar split was made on the create-time alignment: a gradient of an
    // input with a vector part must keep it (torch allocations are 512-B aligned)
    ZS_REQUIRE(!as->in_vec[size_t(i)] || aligned(g[i], galign),
               "zs_adamset_set_grads: g[%lld] = %#llx is not %llu-byte aligned", (long long)i,
               (unsigned long long)g[i], (unsigned long long)galign);
    if (g[i] != as->in_g[size_t(i)]) {
      lo = std::min(lo, i);
      hi = i;
    }
    if (g[i]) g_elems += as->in_n[size_t(i)];
  }
  if (hi < lo) return ZS_OK;  // bound to these gradients already: nothing to launch
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t nseg = as->nvec + as->nsca;
  const int grid = int(std::max<int64_t>(1, std::min<int64_t>((nseg + kThreads - 1) / kThreads, 64)));
  for (int64_t k0 = lo; k0 <= hi; k0 += kGradPatchMax) {
    GradPatch p{};
    p.k0 = k0;
    p.n = int(std::min<int64_t>(kGradPatchMax, hi + 1 - k0));
    for (int k = 0; k < p.n; ++k) p.g[k] = g[k0 + k];
    if (nseg)
      hipLaunchKernelGGL(adam_patch_grads_kernel, dim3(grid), dim3(kThreads), 0, st, as->d_vec,
                         as->d_vec_in, as->nvec, as->d_sca, as->d_sca_in, as->d_sca_goff, as->nsca,
                         p);
    ZS_HIP(hipGetLastError());
  }
  std::copy(g, g + n, as->in_g.begin());
  const int64_t gsz = as->g_dtype == ZS_F32 ? 4 : 2;
  as->bytes = as->bytes_no_g + gsz * g_elems;
  return ZS_OK;
}

int zs_adamset_destroy(zs_adamset* as) {
  if (!as) return ZS_OK;
  if (as->d_vec) (void)hipFree(as->d_vec);
  if (as->d_vec_prefix) (void)hipFree(as->d_vec_prefix);
  if (as->d_sca) (void)hipFree(as->d_sca);
  if (as->d_sca_prefix) (void)hipFree(as->d_sca_prefix);
  if (as->d_vec_in) (void)hipFree(as->d_vec_in);
  if (as->d_sca_in) (void)hipFree(as->d_sca_in);
  if (as->d_sca_goff) (void)hipFree(as->d_sca_goff);
  if (as->d_vec_slots) (void)hipFree(as->d_vec_slots);
  if (as->d_sca_slots) (void)hipFree(as->d_sca_slots);
  if (as->d_un_off) (void)hipFree(as->d_un_off);
  delete as;
  return ZS_OK;
}

int zs_adamset_stats(const zs_adamset* as, int64_t* elems, int64_t* bytes) {
  ZS_REQUIRE(as && elems && bytes, "zs_adamset_stats: NULL argument");
  *elems = as->elems;
  *bytes = as->bytes;
  return ZS_OK;
}

}  // extern "C"

// A stream-flag record (zs_comm.cpp zs_sync_record): one wave whose lane 0 stores the epoch with a
// system-scope release (a vector store: global_store … sc0 sc1).  In stream order like any launch
// (the dispatch waits for the stream's earlier work, whose writes its end-of-kernel release made
// visible), so the word reaches `value` only after everything recorded before it — what
// hipStreamWriteValue64 does, without the runtime's stream-operation command: on this stack that
// command costs a HIP runtime thread ~20 us of CPU per record (profiles/r06_z3_thr_*.json: 1.5 ms
// of the simulated ws = 8 C5 iteration's 102 records), a kernel launch does not.
template <bool kFence>
__global__ __launch_bounds__(64) void flag_write_kernel(uint64_t* flag, uint64_t value) {
  // kFence: a system-scope release (an L2 write-back first); without it a relaxed store straight
  // to memory (sc0 sc1) — the stream's earlier kernels made their writes visible at their own end
  if (threadIdx.x == 0) {
    if (kFence)
      __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    else
      __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// A stream-flag wait as one wave that polls the word with s_sleep between loads (zs_tune
// "sync_wait_kernel" 1).  hipStreamWaitValue64 on this stack is a runtime kernel
// (__amd_rocclr_streamOpsWait) spinning without pause: a side stream waiting for the compute stream
// keeps it busy for milliseconds beside the compute stream's GEMMs (profiles/r06_sm3_sim8 kernel
// stats).  Gives up after ~2^24 polls (about a minute) rather than hold the GPU forever, and then
// stores 1 into `timed_out` (a pinned host word): the next sync call on the host fails loudly
// (zs_comm.cpp flag_wait_check) instead of the lost ordering passing silently.
__global__ __launch_bounds__(64) void flag_wait_kernel(const uint64_t* flag, uint64_t value,
                                                       uint32_t* timed_out) {
  if (threadIdx.x == 0) {
    uint32_t i = 0;
    for (; i < (1u << 24); ++i) {
      if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= value) break;
      __builtin_amdgcn_s_sleep(64);
    }
    if (i == (1u << 24) && timed_out != nullptr)
      __hip_atomic_store(timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

namespace zs {
int& sync_write_kernel() {  // zs_tune("sync_write_kernel"): 1 = flag_write_kernel, 0 = hipStreamWriteValue64
  static int v = 1;
  return v;
}
int& sync_write_fence() {  // zs_tune("sync_write_fence"): 1 = release store, 0 = relaxed store
  static int v = 1;
  return v;
}
int& sync_wait_kernel() {  // zs_tune("sync_wait_kernel"): 1 = flag_wait_kernel, 0 = hipStreamWaitValue64
  static int v = 1;
  return v;
}

hipError_t flag_write(uint64_t* flag, uint64_t value, hipStream_t st) {
  if (sync_write_fence())
    hipLaunchKernelGGL(flag_write_kernel<true>, dim3(1), dim3(64), 0, st, flag, value);
  else
    hipLaunchKernelGGL(flag_write_kernel<false>, dim3(1), dim3(64), 0, st, flag, value);
  return hipGetLastError();
}

// the pinned host word flag_wait_kernel marks on a timeout (nullptr when pinned memory is refused)
uint32_t* wait_timeout_word() {
  static uint32_t* w = [] {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocPortable | hipHostMallocMapped) !=
        hipSuccess) {
      (void)hipGetLastError();
      return static_cast<uint32_t*>(nullptr);
    }
    *static_cast<volatile uint32_t*>(p) = 0;
    return static_cast<uint32_t*>(p);
  }();
  return w;
}

hipError_t flag_wait_launch(const uint64_t* flag, uint64_t value, hipStream_t st) {
  hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, st, flag, value, wait_timeout_word());
  return hipGetLastError();
}
}  // namespace zs

extern "C" {

int zs_tune(const char* key, int64_t value, int64_t* previous) {
  ZS_REQUIRE(key != nullptr, "zs_tune: key is NULL");
  int* slot = nullptr;
  bool ok = false;
  if (std::strcmp(key, "dq_unroll") == 0) {
    slot = &dq_tune().unroll;
    ok = value == 4 || value == 8 || value == 16;
  } else if (std::strcmp(key, "dq_nt_store") == 0) {
    slot = &dq_tune().nt_store;
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "dq_wg_per_cu") == 0) {
    slot = &dq_tune().wg_per_cu;
    ok = value >= 0 && value <= 128;
  } else if (std::strcmp(key, "scale_nt") == 0) {
    slot = &scale_nt_mode();
    ok = value >= -1 && value <= 1;
  } else if (std::strcmp(key, "convert_nt") == 0) {
    slot = &convert_nt_mode();
    ok = value >= -1 && value <= 1;
  } else if (std::strcmp(key, "copy_nt") == 0) {
    slot = &copy_nt_mode();
    ok = value >= -1 && value <= 1;
  } else if (std::strcmp(key, "accumulate_nt") == 0) {
    slot = &accumulate_nt_mode();
    ok = value >= -1 && value <= 1;
  } else if (std::strcmp(key, "adam_wg_per_cu") == 0) {
    slot = &adam_wg_per_cu();
    ok = value >= 0 && value <= 1024;
  } else if (std::strcmp(key, "adam_loads_first") == 0) {
    slot = &adam_loads_first();
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "sqnorm_nt") == 0) {
    slot = &sqnorm_nt();
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "sync_host_flags") == 0) {
    slot = &zs::sync_host_flags();
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "sync_write_kernel") == 0) {
    slot = &zs::sync_write_kernel();
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "sync_write_fence") == 0) {
    slot = &zs::sync_write_fence();
    ok = value == 0 || value == 1;
  } else if (std::strcmp(key, "sync_wait_kernel") == 0) {
    slot = &zs::sync_wait_kernel();
    ok = value == 0 || value == 1;
  } else {
    return zs::fail(ZS_ERR_INVALID, "zs_tune: unknown key '%s'", key);
  }
  ZS_REQUIRE(ok, "zs_tune: value %lld out of range for '%s'", (long long)value, key);
  if (previous) *previous = *slot;
  *slot = int(value);
  return ZS_OK;
}

int zs_device_alloc(int64_t bytes, void** out) {
  ZS_REQUIRE(out != nullptr, "zs_device_alloc: out is NULL");
  ZS_REQUIRE(bytes > 0, "zs_device_alloc: bytes must be > 0 (got %lld)", (long long)bytes);
  *out = nullptr;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, size_t(bytes));
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();  // clear the sticky-looking error state of the runtime
    return zs::fail(ZS_ERR_NOMEM, "zs_device_alloc: %lld bytes: out of device memory",
                    (long long)bytes);
  }
  ZS_HIP(e);
  *out = p;
  return ZS_OK;
}

}  // extern "C"

namespace {
// Chunked allocations (zs_device_alloc_chunked): the physical handles behind each reserved range.
struct ChunkedAlloc {
  size_t bytes = 0;
  std::vector<hipMemGenericAllocationHandle_t> handles;
};
std::mutex g_chunked_mu;
std::map<void*, ChunkedAlloc> g_chunked;

void chunked_release(void* p, ChunkedAlloc& a) {  // (every chunk of a live range is mapped)
  (void)hipMemUnmap(p, a.bytes);
  for (auto h : a.handles) (void)hipMemRelease(h);
  (void)hipMemAddressFree(p, a.bytes);
}
}  // namespace

extern "C" {

int zs_device_alloc_chunked(int64_t bytes, int64_t chunk_bytes, void** out) {
  ZS_REQUIRE(out != nullptr, "zs_device_alloc_chunked: out is NULL");
  ZS_REQUIRE(bytes > 0 && chunk_bytes > 0, "zs_device_alloc_chunked: bytes and chunk_bytes must be > 0");
  *out = nullptr;
  int dev = 0;
  ZS_HIP(hipGetDevice(&dev));
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = dev;
  size_t gran = 0;
  ZS_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
  ZS_REQUIRE(gran > 0 && size_t(chunk_bytes) % gran == 0,
             "zs_device_alloc_chunked: chunk_bytes %lld is not a multiple of the granularity %zu",
             (long long)chunk_bytes, gran);
  const size_t chunk = size_t(chunk_bytes);
  const size_t total = (size_t(bytes) + chunk - 1) / chunk * chunk;
  ChunkedAlloc a;
  a.bytes = total;
  void* p = nullptr;
  hipError_t e = hipMemAddressReserve(&p, total, 0, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return zs::fail(ZS_ERR_HIP, "zs_device_alloc_chunked: hipMemAddressReserve(%zu): %s", total,
                    hipGetErrorString(e));
  }
  for (size_t off = 0; off < total && e == hipSuccess; off += chunk) {
    hipMemGenericAllocationHandle_t h;
    e = hipMemCreate(&h, chunk, &prop, 0);
    if (e != hipSuccess) break;
    e = hipMemMap(static_cast<char*>(p) + off, chunk, 0, h, 0);
    if (e != hipSuccess) {
      (void)hipMemRelease(h);
      break;
    }
    a.handles.push_back(h);
  }
  if (e == hipSuccess) {
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    e = hipMemSetAccess(p, total, &acc, 1);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    const size_t n = a.handles.size();
    if (n) (void)hipMemUnmap(p, n * chunk);
    for (auto h : a.handles) (void)hipMemRelease(h);
    (void)hipMemAddressFree(p, total);
    (void)hipGetLastError();
    return zs::fail(e == hipErrorOutOfMemory ? ZS_ERR_NOMEM : ZS_ERR_HIP,
                    "zs_device_alloc_chunked: %lld bytes in %lld-byte chunks: %s", (long long)bytes,
                    (long long)chunk_bytes, hipGetErrorString(e));
  }
  {
    std::lock_guard<std::mutex> lk(g_chunked_mu);
    g_chunked[p] = std::move(a);
  }
  *out = p;
  return ZS_OK;
}

int zs_device_free(void* p) {
  if (p == nullptr) return ZS_OK;
  {
    std::unique_lock<std::mutex> lk(g_chunked_mu);
    auto it = g_chunked.find(p);
    if (it != g_chunked.end()) {
      ChunkedAlloc a = std::move(it->second);
      g_chunked.erase(it);
      lk.unlock();
      // hipFree waits for the device; an unmap does not: no queued work may still use the range
      ZS_HIP(hipDeviceSynchronize());
      chunked_release(p, a);
      return ZS_OK;
    }
  }
  ZS_HIP(hipFree(p));
  return ZS_OK;
}

}  // extern "C"
