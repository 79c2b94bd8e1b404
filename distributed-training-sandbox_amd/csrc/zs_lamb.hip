// Fused LAMB (You et al. 2020, arXiv:1904.00962; zero_amd.optim.LAMB) for CDNA4 (gfx950): the
// kernels of its two stream passes and the finishing kernel between them ("Fused
// LAMB").  Pass L1 is an element rule of the chunk-streaming update skeleton, so this file takes
// the skeleton -- the rules, the chunk bodies and the two kernel templates -- from zs_kernels.hip
// and instantiates them here, in a translation unit that the Makefile compiles without packed fp32
// instructions; pass L2 is a kernel pair of its own.  HBM-bound streaming kernels like the
// update's: 64-wide waves, 256-thread workgroups, 16-byte fp32 and 8-byte bf16 accesses per lane,
// all of a full chunk's loads issued before the first use, no LDS, no atomics, no scratch.
#define ZS_UPDATE_SKELETON_ONLY
#include "zs_kernels.hip"

#include "zs_lamb.h"

namespace {

// LAMB (You et al. 2020, arXiv:1904.00962; zero_amd.optim.LAMB) over an Adam set's tables, in two
// stream passes ("Fused LAMB").  The trust ratio of a parameter needs the norms of
// its whole master and of its whole update before any element moves, so pass L1 (LambRule, through
// the skeleton below) moves the moments and sums the norms' partials, and pass L2
// (lamb_apply_kernel) moves the parameter once the ratio exists.  Both form the update direction
// with lamb_u from m and v as memory holds them after L1, so L2's u is L1's bit for bit and nothing
// is staged between them.
//   u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps);  [u = fma(wd, p, u)]
// one fp32 operation per operation of LAMB.step(); only the written fma fuses, sqrt and '/' are
// IEEE correctly rounded.  HPT: LambHP (L1) or LambApplyHP (L2), which name these fields alike.
template <typename HPT>
__device__ __forceinline__ float lamb_u(float m, float v, float p, const HPT& hp) {
#pragma clang fp contract(off)
  float u = (m / hp.bc1) / (sqrtf(v) / hp.bc2_sqrt + hp.eps);
  if (hp.wd != 0.0f) u = fmaf(hp.wd, p, u);
  return u;
}
// L1's Hyper: Adam's fields (neg_step and decay_mul unused) and the stats planes, plus bc1.
struct LambHP : StatsHP {
  float bc1;
};
// LambRule names pass L1's instances (zs_lambset_run_moments; fp32 moments, no carry, no vmax).
// kNoStore: elem moves m and v as Adam's does and leaves u where the skeleton holds the master,
// which its bodies then do not store; they hand stat() the master as loaded and u instead:
//   accu = fmaf(u, u, accu), accw = fmaf(p0, p0, accw)
// per lane and chunk, out through stats_store like AdamStatsRule's pair (plane 0: sum u^2, plane 1:
// sum p0^2).  A segment without a gradient is not part of the step: nothing of it is read or
// written, its slots get +0.0.
struct LambRule : AdamRule<false> {
  using Hyper = LambHP;
  using Stats = LaneStats;
  static constexpr bool kStats = true, kNoStore = true;
  template <bool CARRY, bool CLIP>
  static __device__ __forceinline__ void elem(float gsum, float& p, float& m, float& v, float&,
                                              float& carry, const LambHP& hp, float coef) {
#pragma clang fp contract(off)
    static_assert(!CARRY, "LAMB has no ZeRO-1 carry instances");
    const float g = prep_grad<CARRY, CLIP>(gsum, carry, hp, coef);
    m = fmaf(hp.lerp_w, g - m, hp.lerp_hi ? g : m);  // m.lerp_(g, 1 - beta1), as AdamRule
    v = fmaf(hp.omb2 * g, g, v * hp.beta2);          // v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p = lamb_u(m, v, p, hp);
  }
  static __device__ __forceinline__ void stat(float p0, float u, LaneStats& a) {
#pragma clang fp contract(off)
    a.d = fmaf(u, u, a.d);
    a.w = fmaf(p0, p0, a.w);
  }
};

// ----------------------------------------------------------------------------------------------
// LAMB, pass L2: p = fma(-s, u, p) over an Adam set's tables (zs_lambset_run_apply)
// ----------------------------------------------------------------------------------------------
// A kernel pair of its own, not a rule of the skeleton above: it has no gradient, moment store or
// statistics, and one thing the skeleton lacks, a scalar per table entry.  entry_param[seg] is the
// parameter of entry seg (zs_lambset_bind_params) and neg_s[parameter] = -(lr * trust ratio), which
// lamb_finish_kernel wrote: one uniform load per chunk, kept in a scalar register.  16 B/element over
// the split master (m 4, v 4, hi 2 + 2, lo 2 + 2), against L1's 22.  The traversal is the update's
// (grid-stride over chunks, bisect for the first segment, forward scan after it); an entry whose
// segment has no gradient is passed over, as L1 passed over it.
struct LambApplyHP {
  float bc1, bc2_sqrt, eps, wd;
};

__device__ __forceinline__ float lamb_neg_s(const int32_t* __restrict__ entry_param,
                                            const float* __restrict__ neg_s, int64_t seg) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(
      __builtin_amdgcn_readfirstlane(__float_as_uint(neg_s[entry_param[seg]])));
#else
  return neg_s[entry_param[seg]];
#endif
}

// Four elements: u from the stored moments, then the step on the fp32 master.
__device__ __forceinline__ void lamb_apply4(const float* mp, const float* vp, float* pp,
                                            const LambApplyHP& hp, float ns) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 4; ++j) pp[j] = fmaf(ns, lamb_u(mp[j], vp[j], pp[j], hp), pp[j]);
}

// One full chunk: all of its loads (16 for the split master's G = 4: m, v, hi, lo) into raw registers
// before the first use, through update_full_chunk's scalar bases and shared lane offsets; then u,
// the step and the stores, group by group.
template <bool SPLIT>
__device__ __forceinline__ void lamb_apply_full_chunk(const AdamSeg& s, int64_t e0,
                                                      const LambApplyHP& hp, float ns) {
  constexpr int G = adam_groups(SPLIT);
  uint32_t o4 = threadIdx.x * 16u, o2 = threadIdx.x * 8u;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(o4), "+v"(o2));  // (see update_full_chunk)
#endif
  typedef ChunkStream<float, G> S4;
  typedef ChunkStream<unsigned short, G> S2;
  const S4 sm(s.m + e0), sv(s.v + e0);
  const S4 pm(SPLIT ? nullptr : (float*)s.master + e0), po(SPLIT ? nullptr : s.master_out + e0);
  const S2 hi(SPLIT ? (unsigned short*)s.master + e0 : nullptr);
  const S2 lo(SPLIT ? (unsigned short*)s.master_out + e0 : nullptr), pb(s.p_out + e0);
  uint4 mq[G], vq[G], pq[G];
  uint2 hd[G], ld[G];
#pragma unroll
  for (int u = 0; u < G; ++u) {
    if constexpr (SPLIT) {
      hd[u] = nt_ld8(hi.at(u, o2));
      ld[u] = nt_ld8(lo.at(u, o2));
    } else {
      pq[u] = nt_ld16(pm.at(u, o4));
    }
    mq[u] = nt_ld16(sm.at(u, o4));
    vq[u] = nt_ld16(sv.at(u, o4));
  }
#pragma unroll
  for (int u = 0; u < G; ++u) {
    float pp[4], mp[4], vp[4];
    if constexpr (SPLIT) join_master4(hd[u], ld[u], pp);
    else unpack4(pq[u], pp);
    unpack4(mq[u], mp);
    unpack4(vq[u], vp);
    lamb_apply4(mp, vp, pp, hp, ns);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(o4), "+v"(o2));
#endif
    if constexpr (SPLIT) {
      uint32_t h[4], l[4];
      split_master4(pp, h, l);
      nt_st8(pb.at(u, o2), pack_u16x4(h));
      nt_st8(lo.at(u, o2), pack_u16x4(l));
    } else {
      if (s.master_out) nt_st16(po.at(u, o4), pack4(pp));
      if (s.p_out) {
        const uint2 r = pack_bf16x4(pp);
        nt_st8(pb.at(u, o2), r);
      }
    }
  }
}

// One float4 group from element e0 under its lane's `i < s.n` (a segment's last, partial chunk).
template <bool SPLIT>
__device__ __forceinline__ void lamb_apply_pred_group(const AdamSeg& s, int64_t e0,
                                                      const LambApplyHP& hp, float ns) {
  const int64_t i = e0 + int64_t(threadIdx.x) * 4;
  if (i < s.n) {  // (n % 4 == 0 in the vector table: the four elements are in range together)
    float pp[4], mp[4], vp[4];
    if constexpr (SPLIT) {
      const uint2 h = nt_ld8(reinterpret_cast<const unsigned short*>(s.master) + i);
      const uint2 l = nt_ld8(reinterpret_cast<const unsigned short*>(s.master_out) + i);
      join_master4(h, l, pp);
    } else {
      unpack4(nt_ld16(s.master + i), pp);
    }
    unpack4(nt_ld16(s.m + i), mp);
    unpack4(nt_ld16(s.v + i), vp);
    lamb_apply4(mp, vp, pp, hp, ns);
    if constexpr (SPLIT) {
      uint32_t h[4], l[4];
      split_master4(pp, h, l);
      nt_st8(s.p_out + i, pack_u16x4(h));
      nt_st8(reinterpret_cast<unsigned short*>(s.master_out) + i, pack_u16x4(l));
    } else {
      if (s.master_out) nt_st16(s.master_out + i, pack4(pp));
      if (s.p_out) {
        const uint2 r = pack_bf16x4(pp);
        nt_st8(s.p_out + i, r);
      }
    }
  }
}

template <bool SPLIT>
__global__ __launch_bounds__(kThreads) void lamb_apply_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, const int32_t* __restrict__ entry_param,
    const float* __restrict__ neg_s, LambApplyHP hp) {
  constexpr int G = adam_groups(SPLIT);
  int64_t seg = 0, hi = nseg;
  while (hi - seg > 1) {  // the segment of the first chunk, as adam_segments_kernel
    const int64_t mid = (seg + hi) >> 1;
    if (chunk_prefix[mid] <= int64_t(blockIdx.x)) seg = mid;
    else hi = mid;
  }
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const AdamSeg s = segs[seg];
    if (!s.g) continue;  // (uniform) no gradient: L1 left it out of the step
    const float ns = lamb_neg_s(entry_param, neg_s, seg);
    const int64_t e0 = (c - chunk_prefix[seg]) * adam_chunk(SPLIT);
    if (e0 + adam_chunk(SPLIT) <= s.n) {  // uniform per workgroup
      lamb_apply_full_chunk<SPLIT>(s, e0, hp, ns);
    } else {
#pragma unroll 1
      for (int u = 0; u < G && e0 + int64_t(u) * kThreads * 4 < s.n; ++u)
        lamb_apply_pred_group<SPLIT>(s, e0 + int64_t(u) * kThreads * 4, hp, ns);
    }
  }
}

// The scalar table (tails, unaligned segments): one element per lane, 256-element chunks.
template <bool SPLIT>
__global__ __launch_bounds__(kThreads) void lamb_apply_scalar_kernel(
    const AdamSeg* __restrict__ segs, const int64_t* __restrict__ chunk_prefix, int64_t nseg,
    int64_t total_chunks, const int32_t* __restrict__ entry_param,
    const float* __restrict__ neg_s, LambApplyHP hp) {
#pragma clang fp contract(off)
  int64_t seg = 0;
  for (int64_t c = blockIdx.x; c < total_chunks; c += gridDim.x) {
    while (chunk_prefix[seg + 1] <= c) ++seg;
    const AdamSeg s = segs[seg];
    if (!s.g) continue;
    const float ns = lamb_neg_s(entry_param, neg_s, seg);
    const int64_t i = (c - chunk_prefix[seg]) * kThreads + threadIdx.x;
    if (i < s.n) {
      const gptr<unsigned short> lo = glob(reinterpret_cast<unsigned short*>(s.master_out));
      float p = SPLIT ? join_master(glob(reinterpret_cast<const unsigned short*>(s.master))[i], lo[i])
                      : glob(s.master)[i];
      p = fmaf(ns, lamb_u(glob(s.m)[i], glob(s.v)[i], p, hp), p);
      if constexpr (SPLIT) {
        const unsigned short h = f32_to_bf16(p);
        glob(s.p_out)[i] = h;
        lo[i] = (unsigned short)master_residual(p, h);
      } else {
        if (s.master_out) glob(s.master_out)[i] = p;
        if (s.p_out) glob(s.p_out)[i] = f32_to_bf16(p);
      }
    }
  }
}

// Between the passes (zs_lamb_finish), one thread per parameter: sums3 = [sum u^2 | sum p0^2 |
// touched], n floats each, as UpdateNorms reduces (and all-reduces) them.
//   un = float(sqrt(double(sum u^2))), wn = float(sqrt(double(sum p0^2)))
//   r  = (wn == 0 || un == 0) ? 1 : wn / un      (one fp32 division; a NaN norm gives a NaN ratio)
//   -s = -(lr[i] * r)                            (one fp32 product)
// norms2 = [wn | un].  A parameter no set touched: wn = un = +0.0 and r = 1; L2 has no entry for it.
__global__ __launch_bounds__(kThreads) void lamb_finish_kernel(
    const float* __restrict__ sums3, int64_t n, const float* __restrict__ lr,
    float* __restrict__ norms2, float* __restrict__ ratios, float* __restrict__ neg_s) {
#pragma clang fp contract(off)
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * kThreads) {
    float wn = 0.0f, un = 0.0f;
    if (sums3[2 * n + i] != 0.0f) {
      un = float(sqrt(double(sums3[i])));
      wn = float(sqrt(double(sums3[n + i])));
    }
    const float r = (wn == 0.0f || un == 0.0f) ? 1.0f : wn / un;
    norms2[i] = wn;
    norms2[n + i] = un;
    ratios[i] = r;
    neg_s[i] = -(lr[i] * r);
  }
}

// a run-time flag as a compile-time one
template <typename Fn>
void with_flag(bool b, Fn&& fn) {
  if (b) fn(std::true_type{});
  else fn(std::false_type{});
}

}  // namespace

namespace zs {

// L1: 8 vector instances (gradient type x master storage x CLIP; loads first) and 8 scalar ones
int lamb_moments(const LambTables& t, const zs_lamb_hparams& h, const float* coef,
                 const LambPlanes& planes, uintptr_t stream) {
  LambHP hp;
  const float w = h.one_minus_beta1;  // ATen's lerp: which form, and the fma's coefficient
  hp.lerp_hi = std::fabs(w) < 0.5f ? 0 : 1;
  hp.lerp_w = hp.lerp_hi ? w - 1.0f : w;
  hp.beta2 = h.beta2;
  hp.omb2 = h.one_minus_beta2;
  hp.neg_step = 0.0f;
  hp.bc2_sqrt = h.bc2_sqrt;
  hp.eps = h.eps;
  hp.wd = h.weight_decay;
  hp.decay_mul = 1.0f;
  hp.carry_mul = 0.0f;
  int exp2 = 0;  // a power-of-two divisor is an exact reciprocal multiply
  hp.grad_div = h.grad_div;
  hp.div_pow2 = std::frexp(double(h.grad_div), &exp2) == 0.5 ? 1 : 0;
  hp.inv_div = float(1.0 / double(h.grad_div));
  hp.maximize = h.maximize ? 1 : 0;
  hp.bc1 = h.bc1;
  hp.planes = planes.planes;
  hp.nslots = planes.nslots;
  hp.vec_off = planes.vec_off;
  hp.sca_off = planes.sca_off;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const AdamSeg* vec = static_cast<const AdamSeg*>(t.vec);
  const AdamSeg* sca = static_cast<const AdamSeg*>(t.sca);
  with_flag(coef != nullptr, [&](auto clip) {
    with_flag(t.split, [&](auto s) {
      with_flag(t.g_dtype == ZS_F32, [&](auto g32) {
        using GT = std::conditional_t<decltype(g32)::value, float, unsigned short>;
        constexpr bool CLIP = decltype(clip)::value, S = decltype(s)::value;
        if (t.vec_chunks)
          hipLaunchKernelGGL((adam_segments_kernel<LambRule, GT, false, S, true, CLIP>),
                             dim3(t.vec_grid), dim3(kThreads), 0, st, vec, t.vec_prefix, t.nvec,
                             t.vec_chunks, hp, coef);
        if (t.sca_chunks)
          hipLaunchKernelGGL((adam_scalar_kernel<LambRule, GT, false, S, CLIP>), dim3(t.sca_grid),
                             dim3(kThreads), 0, st, sca, t.sca_prefix, t.nsca, t.sca_chunks, hp,
                             coef);
      });
    });
  });
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int lamb_finish(const float* sums3, int64_t n_params, const float* lr, float* norms2, float* ratios,
                float* neg_s, uintptr_t stream) {
  const int grid = int(std::min<int64_t>((n_params + kThreads - 1) / kThreads, 1024));
  hipLaunchKernelGGL(lamb_finish_kernel, dim3(grid), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), sums3, n_params, lr, norms2, ratios,
                     neg_s);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

int lamb_apply(const LambTables& t, const zs_lamb_hparams& h, const int32_t* entry_param,
               const float* neg_s, uintptr_t stream) {
  const LambApplyHP hp = {h.bc1, h.bc2_sqrt, h.eps, h.weight_decay};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const AdamSeg* vec = static_cast<const AdamSeg*>(t.vec);
  const AdamSeg* sca = static_cast<const AdamSeg*>(t.sca);
  with_flag(t.split, [&](auto s) {
    constexpr bool S = decltype(s)::value;
    if (t.vec_chunks)
      hipLaunchKernelGGL((lamb_apply_kernel<S>), dim3(t.vec_grid), dim3(kThreads), 0, st, vec,
                         t.vec_prefix, t.nvec, t.vec_chunks, entry_param, neg_s, hp);
    if (t.sca_chunks)
      hipLaunchKernelGGL((lamb_apply_scalar_kernel<S>), dim3(t.sca_grid), dim3(kThreads), 0, st, sca,
                         t.sca_prefix, t.nsca, t.sca_chunks, entry_param + t.nvec, neg_s, hp);
  });
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

}  // namespace zs
