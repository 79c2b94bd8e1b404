// Fused APOLLO (Zhu et al. 2024, arXiv:2412.05270; zero_amd.optim.Apollo's rule) for CDNA4 (gfx950):
// Adam's moments on a rank-r sign sketch of the gradient, one step scale per channel (or per
// tensor) applied to the raw gradient.  An R x C parameter has N = max(R, C) channels of
// K = min(R, C) elements: rows when R >= C ("tall"), columns otherwise ("wide").  Four kernels over
// a table with one entry per matrix, nothing on the host between them:
//
// A1, the sketch.  A workgroup (256 threads, 4 waves) owns 128 channels, one cut of K (a multiple
// of 64) and every sketch column.  Per stage it moves a 128-channel x 64-k tile of bf16(gradsum)
// through LDS (16 KB, row = channel, 128 bytes, 16-byte chunks xor-swizzled with
// (ch ^ (ch >> 3)) & 7): a tall tile lands as 16-byte rows, a wide tile is transposed on the way in
// by 32-bit writes that pair two consecutive k of one channel; either way a wave's writes and its
// ds_read_b128 operand reads spread over all banks.  Wave w owns sketch columns 32 w .. 32 w + 31 and
// 32 (w + 4) ..: per 16-k step it reads four channel operands from LDS and forms its sign operands
// in registers -- one hash word (zs_sr::bits) serves 32 k, a lane's 8 k of one column are one byte
// of it, expanded to 8 bf16 +-1 by shifts and masks -- so one sign operand feeds four
// v_mfma_f32_32x32x16_bf16.  The loader threads also take the channels' sums of g^2 (g before its
// rounding to bf16): an fp32 fma chain over the elements a thread holds of one channel and stage
// piece, doubles above, a fixed shuffle tree, the waves in order.  A cut writes its partial sketch
// to a slot of its own; nothing is atomic.
// A2, the sketch-space Adam: a wave per channel, a lane per 16 bytes of the channel's row of M and
// V; adds the cuts' slots in order, scales, updates M and V in place and leaves the channel's sums
// of Nh^2 and S^2 (fp32 inside the piece, double above).
// A3, the finish: a workgroup per matrix, in double: s_c, F, the norm-growth limiter, F_prev
// stored, a_c to scratch.
// A4, the apply: p = fma(a_c, g, p * decay) with 16-byte accesses where rows are multiples of the
// gradient vector and the streams aligned, element accesses with the same arithmetic elsewhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "zs_common.h"
#include "zs_piece.h"
#include "zs_sr.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCT = 128;                     // channels of an A1 tile
constexpr int kKT = 64;                      // k of an A1 stage
constexpr int kNCT = kCT / 32;               // MFMA row blocks of a tile
constexpr int kLd = kCT * 8 / kThreads;      // 8-element pieces a thread loads per stage
constexpr int kMaxRank = 256;
constexpr int kApplyPieces = 4;              // A4: pieces per thread and tile

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ApEntry {
  const void* g;          // the reduced gradient sum, GT, R x C
  const void* master;     // fp32 master, or (split) the bf16 parameter
  void* master_out;       // fp32 master (in place), or (split) the int16 residual
  unsigned short* p_out;  // bf16 copy of the updated parameter; (split) the bf16 parameter; or null
  float* m;               // exp_avg, N x rank
  float* v;               // exp_avg_sq, N x rank
  float* fprev;           // scaled_grad_norm, one float
  float* sp;              // scratch [ncut][N][rank]: the cuts' partial sketch sums
  double* ggp;            // scratch [ncut][N]: the cuts' sums of g^2
  double* red;            // scratch [2][N]: sum_j Nh^2, sum_j S^2
  float* a;               // scratch [N]: the channel's step a_c
  uint64_t seed;          // the optimizer's seed + the parameter's ordinal
  int32_t R, C, N, K;
  int32_t tall;           // channels are rows
  int32_t vec8;           // A1: 16-byte gradient loads of 8 elements
  int32_t vec;            // A4: 16-byte accesses of every stream
  int32_t vecs;           // A2: 16-byte accesses of sp, m, v
  int32_t ncut, kcut;     // cuts of K and the k of one (a multiple of kKT)
  int32_t reserved[2];
};

struct ApHP {
  double neg_lr;       // -lr * sqrt(scale)
  double norm_growth;
  uint64_t epoch;      // (t - 1) / update_proj_gap
  float cscale;        // 1 / (ws * sqrt(rank)), negated under maximize
  float lerp_w;        // ATen's lerp with weight w = 1 - beta1: w, or w - 1 when lerp_hi
  float beta2, omb2, bc1, bc2_sqrt, eps, decay_mul;
  float grad_div, inv_div;
  int lerp_hi, div_pow2, maximize, rank, tensor;
};

// the averaged gradient the rule starts from: `grad / ws` (a power-of-two divisor is an exact
// reciprocal multiply) and maximize
__device__ __forceinline__ float prep_grad(float s, const ApHP& hp) {
#pragma clang fp contract(off)
  float g = hp.div_pow2 ? s * hp.inv_div : s / hp.grad_div;
  if (hp.maximize) g = -g;
  return g;
}

// ---- A1 ----------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_off(int ch, int chunk) {
  return ch * (kKT * 2) + ((chunk ^ ((ch ^ (ch >> 3)) & 7)) << 4);
}

// 8 consecutive elements from element i of the gradient, the first n of them real, as fp32
template <typename GT, bool VEC>
__device__ __forceinline__ void load_g8(const void* g, int64_t i, int n, float* x) {
  if constexpr (sizeof(GT) == 4) {
    unpack_g<GT>(load_g_piece<GT, VEC>(g, i, n), x);
    unpack_g<GT>(load_g_piece<GT, VEC>(g, i + 4, n - 4), x + 4);
  } else {
    unpack_g<GT>(load_g_piece<GT, VEC>(g, i, n), x);
  }
}

__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  return uint32_t(f32_to_bf16(lo)) | (uint32_t(f32_to_bf16(hi)) << 16);
}

// a byte of a hash word as 8 bf16: bit i clear -> +1 (0x3F80), set -> -1 (0xBF80)
__device__ __forceinline__ bf16x8 expand_signs(uint32_t byte) {
  u32x4 w;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t x = byte >> (2 * d);
    w[d] = 0x3F803F80u | ((x & 1u) << 15) | ((x & 2u) << 30);
  }
  return __builtin_bit_cast(bf16x8, w);
}

template <typename GT, bool TALL, bool VEC>
__device__ __forceinline__ void sketch_body(const ApEntry& e, int tile, int cut, const ApHP& hp,
                                            unsigned char* smem) {
  const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6, half = lane >> 5;
  const int c0 = tile * kCT;
  const int kb = cut * e.kcut, ke = min(e.K, kb + e.kcut);
  const int rank = hp.rank, nj = (rank + 31) >> 5;
  uint32_t k0, k1;
  zs_sr::keys(e.seed, hp.epoch, &k0, &k1);
  // the loader.  Tall: piece i is chunk tid & 7 of channel (tid >> 3) + 32 i.  Wide: piece i is
  // channels 8 (tid & 7) .. + 7 at k = 2 (tid >> 3) + (i & 1) + 64 (i >> 1) ... of a 128-channel
  // tile there are 16 channel groups, so piece i covers group (tid & 7) + 8 (i >> 1).
  const int la = tid & 7, lb = tid >> 3;
  float x[kLd][8];
  double gacc[TALL ? kLd : 16];
#pragma unroll
  for (int i = 0; i < (TALL ? kLd : 16); ++i) gacc[i] = 0.0;
  const auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < kLd; ++i) {
      int ch, kk, n;
      int64_t at;
      if constexpr (TALL) {
        ch = c0 + lb + 32 * i, kk = k + la * 8;
        n = ch < e.N ? ke - kk : 0;
        at = int64_t(ch) * e.C + kk;
      } else {
        ch = c0 + (la + 8 * (i >> 1)) * 8, kk = k + 2 * lb + (i & 1);
        n = kk < ke ? e.N - ch : 0;
        at = int64_t(kk) * e.C + ch;
      }
      n = n < 0 ? 0 : n > 8 ? 8 : n;
      if (n == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[i][j] = 0.0f;
      } else if (VEC) {
        load_g8<GT, VEC>(e.g, at, 8, x[i]);
      } else {
        load_g8<GT, false>(e.g, at, n, x[i]);
      }
    }
  };
  const auto stage = [&]() {  // the sums of g^2, and the tile as bf16 into LDS
#pragma clang fp contract(off)
    if constexpr (TALL) {
#pragma unroll
      for (int i = 0; i < kLd; ++i) {
        constexpr int P = sizeof(GT) == 4 ? 4 : 8;  // a 16-byte piece of the gradient
#pragma unroll
        for (int h = 0; h < 8 / P; ++h) {
          float s = 0.0f;
#pragma unroll
          for (int j = 0; j < P; ++j) {
            const float g = prep_grad(x[i][h * P + j], hp);
            s = fmaf(g, g, s);
          }
          gacc[i] += double(s);
        }
        const uint4 q = make_uint4(pack_bf16(x[i][0], x[i][1]), pack_bf16(x[i][2], x[i][3]),
                                   pack_bf16(x[i][4], x[i][5]), pack_bf16(x[i][6], x[i][7]));
        *reinterpret_cast<uint4*>(smem + lds_off(lb + 32 * i, la)) = q;
      }
    } else {
#pragma unroll
      for (int gI = 0; gI < kLd / 2; ++gI)  // pieces 2 gI and 2 gI + 1: the same channels, k and k + 1
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float g0 = prep_grad(x[2 * gI][j], hp), g1 = prep_grad(x[2 * gI + 1][j], hp);
          gacc[gI * 8 + j] += double(fmaf(g1, g1, g0 * g0));
          const int ch = (la + 8 * gI) * 8 + j;
          *reinterpret_cast<uint32_t*>(smem + lds_off(ch, lb >> 2) + (lb & 3) * 4) =
              pack_bf16(x[2 * gI][j], x[2 * gI + 1][j]);
        }
    }
  };
  f32x16 acc[kNCT][2];
#pragma unroll
  for (int i = 0; i < kNCT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  // the column a lane forms signs for, per owned column block: its key word, and whether it exists
  uint32_t pre[2];
  bool live[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int j = (wave + 4 * jj) * 32 + (lane & 31);
    pre[jj] = k0 ^ (uint32_t(j) * 0x9E3779B9u);
    live[jj] = j < rank;
  }
  fetch(kb);
  for (int k = kb; k < ke; k += kKT) {
    stage();
    __syncthreads();
    if (k + kKT < ke) fetch(k + kKT);
    if (wave < nj) {
      uint32_t h[2][2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int w = 0; w < 2; ++w)  // = zs_sr::bits((uint64(j) << 32) | kw, k0, k1)
          h[jj][w] = zs_sr::lowbias32(uint32_t((k >> 5) + w) ^ pre[jj]) ^ k1;
#pragma unroll
      for (int ks = 0; ks < kKT / 16; ++ks) {
        bf16x8 av[kNCT], bv[2];
#pragma unroll
        for (int i = 0; i < kNCT; ++i)
          av[i] = __builtin_bit_cast(
              bf16x8, *reinterpret_cast<const uint4*>(smem + lds_off(i * 32 + (lane & 31), ks * 2 + half)));
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          bv[jj] = expand_signs((h[jj][ks >> 1] >> (8 * ((ks & 1) * 2 + half))) & 0xFFu);
          if (!live[jj]) bv[jj] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
        }
#pragma unroll
        for (int i = 0; i < kNCT; ++i) {
          acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[0], acc[i][0], 0, 0, 0);
          if (wave + 4 < nj)
            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[1], acc[i][1], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  // accumulator r of block (i, jj): channel c0 + 32 i + 8 (r / 4) + 4 half + r % 4, column
  // 32 (wave + 4 jj) + lane % 32
  float* sp = e.sp + int64_t(cut) * e.N * rank;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int j = (wave + 4 * jj) * 32 + (lane & 31);
    if (j >= rank) continue;
#pragma unroll
    for (int i = 0; i < kNCT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = c0 + i * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        if (ch < e.N) sp[int64_t(ch) * rank + j] = acc[i][jj][r];
      }
  }
  // the channels' sums of g^2 (the tile's LDS is free after the loop's last barrier)
  double* gs = reinterpret_cast<double*>(smem);
  double* ggp = e.ggp + int64_t(cut) * e.N;
  if constexpr (TALL) {
#pragma unroll
    for (int i = 0; i < kLd; ++i) {
      double s = gacc[i];
      s += __shfl_xor(s, 1, 64), s += __shfl_xor(s, 2, 64), s += __shfl_xor(s, 4, 64);
      const int ch = c0 + lb + 32 * i;
      if (la == 0 && ch < e.N) ggp[ch] = s;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      double s = gacc[q];
      s += __shfl_xor(s, 8, 64), s += __shfl_xor(s, 16, 64), s += __shfl_xor(s, 32, 64);
      if (lane < 8) gs[wave * kCT + (lane + 8 * (q >> 3)) * 8 + (q & 7)] = s;
    }
    __syncthreads();
    if (tid < kCT && c0 + tid < e.N)
      ggp[c0 + tid] = ((gs[tid] + gs[kCT + tid]) + gs[2 * kCT + tid]) + gs[3 * kCT + tid];
  }
}

// kernel-resource-usage (gfx950): see DESIGN.md §4 "Fused APOLLO"
template <typename GT>
__global__ __launch_bounds__(kThreads) void apollo_sketch_kernel(
    const ApEntry* __restrict__ entries, const int64_t* __restrict__ prefix, int64_t nent,
    const ApHP hp) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kCT * kKT * 2];
  const int64_t ei = find_entry(prefix, nent, blockIdx.x);
  const ApEntry e = entries[ei];
  const int it = int(int64_t(blockIdx.x) - prefix[ei]);
  const int tile = it / e.ncut, cut = it % e.ncut;
  if (e.tall) {
    if (e.vec8) sketch_body<GT, true, true>(e, tile, cut, hp, smem);
    else sketch_body<GT, true, false>(e, tile, cut, hp, smem);
  } else {
    if (e.vec8) sketch_body<GT, false, true>(e, tile, cut, hp, smem);
    else sketch_body<GT, false, false>(e, tile, cut, hp, smem);
  }
}

// ---- A2 ----------------------------------------------------------------------------------------
// ATen's lerp (Lerp.h): self + w * (end - self) for |w| < 0.5, end - (end - self) * (1 - w) otherwise
__device__ __forceinline__ float lerp_to(float self, float end, const ApHP& hp) {
#pragma clang fp contract(off)
  return fmaf(hp.lerp_w, end - self, hp.lerp_hi ? end : self);
}

template <bool VEC>
__device__ __forceinline__ void moments_body(const ApEntry& e, int ch, const ApHP& hp) {
#pragma clang fp contract(off)
  const int lane = int(threadIdx.x) & 63, rank = hp.rank;
  const int j0 = lane * 4, n = min(4, rank - j0);
  const int64_t at = int64_t(ch) * rank + j0;
  double nn = 0.0, ss = 0.0;
  if (n > 0) {
    float s[4], m[4], v[4];
    load_m<4, VEC>(e.sp, at, n, s);
    for (int c = 1; c < e.ncut; ++c) {  // the cuts' slots in order
      float t[4];
      load_m<4, VEC>(e.sp, int64_t(c) * e.N * rank + at, n, t);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = s[j] + t[j];
    }
    load_m<4, VEC>(e.m, at, n, m);
    load_m<4, VEC>(e.v, at, n, v);
    float fn = 0.0f, fs = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float S = s[j] * hp.cscale;
      m[j] = lerp_to(m[j], S, hp);
      v[j] = fmaf(hp.omb2, S * S, v[j] * hp.beta2);
      const float nh = (m[j] / hp.bc1) / (sqrtf(v[j]) / hp.bc2_sqrt + hp.eps);
      if (j < n) fn = fmaf(nh, nh, fn), fs = fmaf(S, S, fs);
    }
    store_m<4, VEC>(e.m, at, n, m);
    store_m<4, VEC>(e.v, at, n, v);
    nn = double(fn), ss = double(fs);
  }
  nn = wave_sum(nn), ss = wave_sum(ss);
  if (lane == 0) e.red[ch] = nn, e.red[e.N + ch] = ss;
}

__global__ __launch_bounds__(kThreads) void apollo_moments_kernel(
    const ApEntry* __restrict__ entries, const int64_t* __restrict__ prefix, int64_t nent,
    const ApHP hp) {
  const int64_t ei = find_entry(prefix, nent, blockIdx.x);
  const ApEntry e = entries[ei];
  const int ch = int(int64_t(blockIdx.x) - prefix[ei]) * 4 + int(threadIdx.x >> 6);
  if (ch >= e.N) return;  // (a whole wave)
  if (e.vecs) moments_body<true>(e, ch, hp);
  else moments_body<false>(e, ch, hp);
}

// ---- A3 ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void apollo_finish_kernel(const ApEntry* __restrict__ entries,
                                                                 const ApHP hp) {
  __shared__ double part[3][4];
  const ApEntry e = entries[blockIdx.x];
  const int tid = int(threadIdx.x);
  const double fprev = double(*e.fprev);
  double s_all = 0.0;
  if (hp.tensor) {
    double tn = 0.0, ts = 0.0;
    for (int c = tid; c < e.N; c += kThreads) tn += e.red[c], ts += e.red[e.N + c];
    tn = block_sum(tn, part[0]), ts = block_sum(ts, part[1]);
    s_all = sqrt(tn) / (sqrt(ts) + 1e-8);
  }
  const auto scale_of = [&](int c) {
    return hp.tensor ? s_all : sqrt(e.red[c]) / (sqrt(e.red[e.N + c]) + 1e-8);
  };
  double f2 = 0.0;
  for (int c = tid; c < e.N; c += kThreads) {
    double gg = e.ggp[c];
    for (int k = 1; k < e.ncut; ++k) gg += e.ggp[int64_t(k) * e.N + c];
    const double s = scale_of(c);
    f2 += s * s * gg;
  }
  const double F = sqrt(block_sum(f2, part[2]));
  double lam = 1.0;
  if (hp.norm_growth > 0.0 && fprev > 0.0) {  // max() that keeps a NaN
    const double r = F / (fprev + 1e-8);
    lam = (r > hp.norm_growth || r != r) ? r / hp.norm_growth : 1.0;
  }
  for (int c = tid; c < e.N; c += kThreads) e.a[c] = float(hp.neg_lr * scale_of(c) / lam);
  if (tid == 0) *e.fprev = float(F / lam);  // (every thread read it before block_sum's barrier)
}

// ---- A4 ----------------------------------------------------------------------------------------
template <typename GT, bool SPLIT, bool VEC>
__device__ __forceinline__ void apply_body(const ApEntry& e, int64_t tile, const ApHP& hp) {
#pragma clang fp contract(off)
  constexpr int V = 16 / int(sizeof(GT));
  const int64_t ne = int64_t(e.R) * e.C, base = tile * (kApplyPieces * kThreads * V);
  const int64_t brow = base / e.C;
  const uint32_t bcol = uint32_t(base % e.C), C = uint32_t(e.C);
  uint4 q[kApplyPieces];
#pragma unroll
  for (int k = 0; k < kApplyPieces; ++k) {  // every load of the gradient before the first use
    const int64_t off = base + (k * kThreads + int(threadIdx.x)) * V;
    q[k] = make_uint4(0u, 0u, 0u, 0u);
    if (off < ne) q[k] = load_g_piece<GT, VEC>(e.g, off, ne - off < V ? int(ne - off) : V);
  }
#pragma unroll
  for (int k = 0; k < kApplyPieces; ++k) {
    const uint32_t loc = uint32_t(k * kThreads + int(threadIdx.x)) * V;
    const int64_t off = base + loc;
    if (off >= ne) continue;
    const int n = ne - off < V ? int(ne - off) : V;
    float g[V], p[V], a[V];
    unpack_g<GT>(q[k], g);
    if constexpr (VEC) {  // the piece lies inside one row
      const uint32_t l = bcol + loc;
      const int64_t row = brow + l / C;
      const uint32_t col = l % C;
      if (e.tall) {
        const float ar = e.a[row];
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = ar;
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = e.a[col + j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const uint32_t l = bcol + loc + j;
        a[j] = j < n ? e.a[e.tall ? brow + l / C : int64_t(l % C)] : 0.0f;
      }
    }
    load_p<V, VEC, SPLIT>(e, off, n, p);
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = fmaf(a[j], prep_grad(g[j], hp), p[j] * hp.decay_mul);
    store_p<V, VEC, SPLIT>(e, off, n, p);
  }
}

template <typename GT, bool SPLIT>
__global__ __launch_bounds__(kThreads) void apollo_apply_kernel(
    const ApEntry* __restrict__ entries, const int64_t* __restrict__ prefix, int64_t nent,
    const ApHP hp) {
  const int64_t ei = find_entry(prefix, nent, blockIdx.x);
  const ApEntry e = entries[ei];
  const int64_t tile = int64_t(blockIdx.x) - prefix[ei];
  if (e.vec) apply_body<GT, SPLIT, true>(e, tile, hp);
  else apply_body<GT, SPLIT, false>(e, tile, hp);
}

}  // namespace

struct zs_apolloset {
  unsigned tag = zs::kApolloSetTag;
  ApEntry* d_entries = nullptr;
  int64_t* d_pre1 = nullptr;  // A1 workgroups (channel tiles x cuts) before each entry
  int64_t* d_pre2 = nullptr;  // A2 workgroups (four channels each)
  int64_t* d_pre4 = nullptr;  // A4 tiles
  // one allocation: per entry the doubles (ggp, red), then a_c of every channel in table order,
  // then per entry the cuts' sketch slots
  unsigned char* d_scratch = nullptr;
  float* d_a = nullptr;
  float* d_sp = nullptr;
  int64_t nent = 0, wg1 = 0, wg2 = 0, wg4 = 0;
  int64_t elems = 0, bytes = 0, scratch_bytes = 0, channels = 0, state_elems = 0, sp_floats = 0;
  int g_dtype = ZS_F32, p_dtype = ZS_BF16, rank = 0;
};

// mask: bit k = kernel A(k + 1)
template <typename GT, bool SPLIT>
static int run_passes(const zs_apolloset* s, const ApHP& hp, hipStream_t st, int mask) {
  const dim3 block(kThreads);
  if (mask & 1)
    apollo_sketch_kernel<GT><<<dim3(unsigned(s->wg1)), block, 0, st>>>(s->d_entries, s->d_pre1,
                                                                       s->nent, hp);
  if (mask & 2)
    apollo_moments_kernel<<<dim3(unsigned(s->wg2)), block, 0, st>>>(s->d_entries, s->d_pre2,
                                                                    s->nent, hp);
  if (mask & 4)
    apollo_finish_kernel<<<dim3(unsigned(s->nent)), block, 0, st>>>(s->d_entries, hp);
  if (mask & 8)
    apollo_apply_kernel<GT, SPLIT><<<dim3(unsigned(s->wg4)), block, 0, st>>>(
        s->d_entries, s->d_pre4, s->nent, hp);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

static int check_hparams(const char* fn, const zs_apollo_hparams* h) {
  // zero_amd.optim.Apollo.__init__'s rules (a NaN fails every comparison)
  ZS_REQUIRE(h->lr >= 0.0, "%s: invalid learning rate %g", fn, h->lr);
  ZS_REQUIRE(h->beta1 >= 0.0 && h->beta1 < 1.0, "%s: invalid beta parameter at index 0: %g", fn,
             h->beta1);
  ZS_REQUIRE(h->beta2 >= 0.0 && h->beta2 < 1.0, "%s: invalid beta parameter at index 1: %g", fn,
             h->beta2);
  ZS_REQUIRE(h->eps >= 0.0, "%s: invalid epsilon value %g", fn, h->eps);
  ZS_REQUIRE(h->weight_decay >= 0.0, "%s: invalid weight_decay value %g", fn, h->weight_decay);
  ZS_REQUIRE(h->scale > 0.0, "%s: invalid scale %g", fn, h->scale);
  ZS_REQUIRE(h->scale_type == ZS_APOLLO_CHANNEL || h->scale_type == ZS_APOLLO_TENSOR,
             "%s: scale_type must be ZS_APOLLO_CHANNEL or ZS_APOLLO_TENSOR (got %d)", fn,
             int(h->scale_type));
  ZS_REQUIRE(h->update_proj_gap >= 1, "%s: update_proj_gap must be >= 1 (got %lld)", fn,
             (long long)h->update_proj_gap);
  ZS_REQUIRE(h->norm_growth == 0.0 || h->norm_growth > 1.0,
             "%s: norm_growth must be 0 or > 1 (got %g)", fn, h->norm_growth);
  ZS_REQUIRE(h->grad_div > 0.0, "%s: grad_div must be > 0", fn);
  return ZS_OK;
}

static int run_checked(const char* fn, const zs_apolloset* as, const zs_apollo_hparams* h,
                       int64_t step, int mask, uintptr_t stream) {
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(as->tag == zs::kApolloSetTag, "%s: the set was not made by zs_apolloset_create", fn);
  ZS_REQUIRE(step >= 1, "%s: step must be >= 1 (the count after this step; got %lld)", fn,
             (long long)step);
  if (int rc = check_hparams(fn, h)) return rc;  // a struct filled by hand gets init's rules too
  if (as->nent == 0) return ZS_OK;
  // the host scalars in double, each rounded to fp32 once; A3's stay double
  const double t = double(step);
  ApHP hp;
  hp.neg_lr = -h->lr * std::sqrt(h->scale);
  hp.norm_growth = h->norm_growth;
  hp.epoch = uint64_t((step - 1) / h->update_proj_gap);
  hp.cscale = float(1.0 / (h->grad_div * std::sqrt(double(as->rank))));
  if (h->maximize) hp.cscale = -hp.cscale;
  const float w = float(1.0 - h->beta1);
  hp.lerp_hi = std::fabs(w) < 0.5f ? 0 : 1;
  hp.lerp_w = hp.lerp_hi ? w - 1.0f : w;
  hp.beta2 = float(h->beta2);
  hp.omb2 = float(1.0 - h->beta2);
  hp.bc1 = float(1.0 - std::pow(h->beta1, t));
  hp.bc2_sqrt = float(std::sqrt(1.0 - std::pow(h->beta2, t)));
  hp.eps = float(h->eps);
  hp.decay_mul = float(1.0 - h->lr * h->weight_decay);
  int exp2 = 0;
  hp.grad_div = float(h->grad_div);
  hp.div_pow2 = std::frexp(double(hp.grad_div), &exp2) == 0.5 ? 1 : 0;
  hp.inv_div = float(1.0 / double(hp.grad_div));
  hp.maximize = h->maximize ? 1 : 0;
  hp.rank = as->rank;
  hp.tensor = h->scale_type == ZS_APOLLO_TENSOR ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool g32 = as->g_dtype == ZS_F32, split = as->p_dtype == ZS_BF16_SPLIT;
  if (g32)
    return split ? run_passes<float, true>(as, hp, st, mask)
                 : run_passes<float, false>(as, hp, st, mask);
  return split ? run_passes<unsigned short, true>(as, hp, st, mask)
               : run_passes<unsigned short, false>(as, hp, st, mask);
}

extern "C" {

int zs_apollo_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                           double scale, int scale_type, int64_t update_proj_gap,
                           double norm_growth, int maximize, double grad_div,
                           zs_apollo_hparams* hp) {
  const char* fn = "zs_apollo_hparams_init";
  ZS_REQUIRE(hp != nullptr, "%s: hp is NULL", fn);
  zs_apollo_hparams h{};
  h.lr = lr, h.beta1 = beta1, h.beta2 = beta2, h.eps = eps, h.weight_decay = weight_decay;
  h.scale = scale, h.norm_growth = norm_growth, h.grad_div = grad_div;
  h.update_proj_gap = update_proj_gap;
  h.scale_type = scale_type;
  h.maximize = maximize ? 1 : 0;
  if (int rc = check_hparams(fn, &h)) return rc;
  *hp = h;
  return ZS_OK;
}

int zs_apolloset_create(const zs_apollo_seg* in, int64_t n, int g_dtype, int p_dtype, int64_t rank,
                        zs_apolloset** out) {
  const char* fn = "zs_apolloset_create";
  ZS_REQUIRE(out != nullptr, "%s: out is NULL", fn);
  *out = nullptr;
  ZS_REQUIRE(n >= 0 && (n == 0 || in), "%s: bad table", fn);
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "%s: bad g_dtype %d", fn, g_dtype);
  ZS_REQUIRE(p_dtype == ZS_BF16 || p_dtype == ZS_BF16_SPLIT,
             "%s: p_dtype must be ZS_BF16 or ZS_BF16_SPLIT (got %d)", fn, p_dtype);
  ZS_REQUIRE(rank >= 1 && rank <= kMaxRank, "%s: rank must be in [1, %d] (got %lld)", fn, kMaxRank,
             (long long)rank);
  ZS_REQUIRE(n < (int64_t(1) << 31), "%s: %lld entries (max 2^31 - 1)", fn, (long long)n);
  const bool split = p_dtype == ZS_BF16_SPLIT;
  const int64_t gsz = g_dtype == ZS_F32 ? 4 : 2, V = 16 / gsz, msz = split ? 2 : 4;
  const int64_t apply_elems = int64_t(kApplyPieces) * kThreads * V;
  std::vector<ApEntry> ent;
  std::vector<int64_t> pre1(1, 0), pre2(1, 0), pre4(1, 0);
  std::vector<int64_t> d_off, a_off, sp_off;  // per entry, in doubles / floats / floats
  int64_t doubles = 0, channels = 0, spf = 0, elems = 0, bytes = 0, state = 0;
  for (int64_t i = 0; i < n; ++i) {
    const zs_apollo_seg& s = in[i];
    ZS_REQUIRE(s.R >= 1 && s.C >= 1, "%s: entry %lld: R and C must be >= 1", fn, (long long)i);
    ZS_REQUIRE(s.R < (int64_t(1) << 31) - kCT && s.C < (int64_t(1) << 31) - kCT &&
                   s.R * s.C < (int64_t(1) << 40),
               "%s: entry %lld: R or C too large", fn, (long long)i);
    ZS_REQUIRE(s.g && s.master && s.master_out && s.m && s.v && s.fprev,
               "%s: entry %lld missing g/master/master_out/m/v/fprev", fn, (long long)i);
    ZS_REQUIRE(!split || s.p_out, "%s: entry %lld: a split master needs p_out", fn, (long long)i);
    ZS_REQUIRE(split || s.master_out == s.master,
               "%s: entry %lld: the fp32 master is updated in place (master_out == master)", fn,
               (long long)i);
    ZS_REQUIRE(aligned(s.g, uint64_t(gsz)) && aligned(s.master, uint64_t(msz)) &&
                   aligned(s.master_out, uint64_t(msz)) && aligned(s.p_out, 2) &&
                   aligned(s.m, 4) && aligned(s.v, 4) && aligned(s.fprev, 4),
               "%s: entry %lld: a pointer is not aligned to its element", fn, (long long)i);
    ZS_REQUIRE(s.param >= 0, "%s: entry %lld: param < 0", fn, (long long)i);
    ApEntry e{};
    e.g = reinterpret_cast<const void*>(s.g);
    e.master = reinterpret_cast<const void*>(s.master);
    e.master_out = reinterpret_cast<void*>(s.master_out);
    e.p_out = reinterpret_cast<unsigned short*>(s.p_out);
    e.m = reinterpret_cast<float*>(s.m);
    e.v = reinterpret_cast<float*>(s.v);
    e.fprev = reinterpret_cast<float*>(s.fprev);
    e.seed = s.seed;
    e.R = int32_t(s.R), e.C = int32_t(s.C);
    e.tall = s.R >= s.C;
    e.N = e.tall ? e.R : e.C, e.K = e.tall ? e.C : e.R;
    const uint64_t ma = split ? uint64_t(2 * V) : 16;
    e.vec8 = s.C % 8 == 0 && aligned(s.g, 16);
    e.vec = s.C % V == 0 && aligned(s.g, 16) && aligned(s.master, ma) &&
            aligned(s.master_out, ma) && aligned(s.p_out, uint64_t(2 * V));
    e.vecs = rank % 4 == 0 && aligned(s.m, 16) && aligned(s.v, 16);
    // K is cut (a function of the shape alone) only where the channel tiles are too few to fill
    // the chip, and never below 1024 k a cut
    const int64_t tiles = (e.N + kCT - 1) / kCT;
    const int64_t want = std::min<int64_t>((e.K + 1023) / 1024, (128 + tiles - 1) / tiles);
    e.kcut = int32_t(((e.K + want - 1) / want + kKT - 1) / kKT * kKT);
    e.ncut = int32_t((e.K + e.kcut - 1) / e.kcut);
    const int64_t ne = s.R * s.C, wg4 = (ne + apply_elems - 1) / apply_elems;
    ZS_REQUIRE(pre1.back() + tiles * e.ncut < (int64_t(1) << 31) &&
                   pre2.back() + (e.N + 3) / 4 < (int64_t(1) << 31) &&
                   pre4.back() + wg4 < (int64_t(1) << 31),
               "%s: too many workgroups", fn);
    pre1.push_back(pre1.back() + tiles * e.ncut);
    pre2.push_back(pre2.back() + (e.N + 3) / 4);
    pre4.push_back(pre4.back() + wg4);
    d_off.push_back(doubles), doubles += int64_t(e.ncut + 2) * e.N;
    a_off.push_back(channels), channels += e.N;
    sp_off.push_back(spf), spf += (int64_t(e.ncut) * e.N * rank + 3) / 4 * 4;
    ent.push_back(e);
    elems += ne;
    state += 2 * int64_t(e.N) * rank;
    // g twice, the master read and written, M and V read and written
    bytes += ne * (2 * gsz + 8 + (!split && s.p_out ? 2 : 0)) + 16 * int64_t(e.N) * rank;
  }
  zs_apolloset* as = new (std::nothrow) zs_apolloset();
  if (!as) return zs::fail(ZS_ERR_NOMEM, "%s: out of memory", fn);
  as->nent = int64_t(ent.size());
  as->wg1 = pre1.back(), as->wg2 = pre2.back(), as->wg4 = pre4.back();
  as->elems = elems, as->bytes = bytes, as->channels = channels, as->state_elems = state;
  as->sp_floats = spf;
  as->g_dtype = g_dtype, as->p_dtype = p_dtype, as->rank = int(rank);
  *out = as;
  if (as->nent == 0) return ZS_OK;
  const int64_t a_floats = (channels + 3) / 4 * 4;
  as->scratch_bytes = doubles * 8 + (a_floats + spf) * 4;
  int rc = ZS_OK;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&as->d_scratch), size_t(as->scratch_bytes));
  if (he != hipSuccess)
    rc = zs::fail(ZS_ERR_HIP, "%s: hipMalloc of %lld scratch bytes failed: %s", fn,
                  (long long)as->scratch_bytes, hipGetErrorString(he));
  if (rc == ZS_OK) {
    double* d0 = reinterpret_cast<double*>(as->d_scratch);
    as->d_a = reinterpret_cast<float*>(d0 + (doubles + 1) / 2 * 2);
    as->d_sp = as->d_a + a_floats;
    for (size_t k = 0; k < ent.size(); ++k) {
      ent[k].ggp = d0 + d_off[k];
      ent[k].red = ent[k].ggp + int64_t(ent[k].ncut) * ent[k].N;
      ent[k].a = as->d_a + a_off[k];
      ent[k].sp = as->d_sp + sp_off[k];
    }
    rc = upload(ent, &as->d_entries);
  }
  if (rc == ZS_OK) rc = upload(pre1, &as->d_pre1);
  if (rc == ZS_OK) rc = upload(pre2, &as->d_pre2);
  if (rc == ZS_OK) rc = upload(pre4, &as->d_pre4);
  if (rc != ZS_OK) {
    zs_apolloset_destroy(as);
    *out = nullptr;
  }
  return rc;
}

int zs_apolloset_run(const zs_apolloset* as, const zs_apollo_hparams* h, int64_t step,
                     uintptr_t stream) {
  return run_checked("zs_apolloset_run", as, h, step, 15, stream);
}

int zs_apolloset_run_pass(const zs_apolloset* as, const zs_apollo_hparams* h, int64_t step,
                          int pass, uintptr_t stream) {
  ZS_REQUIRE(pass >= 0 && pass <= 3, "zs_apolloset_run_pass: pass must be 0 .. 3 (got %d)", pass);
  return run_checked("zs_apolloset_run_pass", as, h, step, 1 << pass, stream);
}

int zs_apolloset_stats(const zs_apolloset* as, int64_t* out, int64_t n) {
  ZS_REQUIRE(as && out && n >= 0, "zs_apolloset_stats: NULL argument");
  ZS_REQUIRE(as->tag == zs::kApolloSetTag,
             "zs_apolloset_stats: the set was not made by zs_apolloset_create");
  const int64_t v[9] = {as->elems, as->bytes, as->scratch_bytes,
                        int64_t(reinterpret_cast<uintptr_t>(as->d_a)), as->channels,
                        as->state_elems, int64_t(reinterpret_cast<uintptr_t>(as->d_sp)), as->wg1,
                        as->sp_floats};
  for (int64_t k = 0; k < n && k < 9; ++k) out[k] = v[k];
  return ZS_OK;
}

int zs_apolloset_destroy(zs_apolloset* as) {
  if (!as) return ZS_OK;
  ZS_REQUIRE(as->tag == zs::kApolloSetTag,
             "zs_apolloset_destroy: the set was not made by zs_apolloset_create");
  if (as->d_entries) (void)hipFree(as->d_entries);
  if (as->d_pre1) (void)hipFree(as->d_pre1);
  if (as->d_pre2) (void)hipFree(as->d_pre2);
  if (as->d_pre4) (void)hipFree(as->d_pre4);
  if (as->d_scratch) (void)hipFree(as->d_scratch);
  delete as;
  return ZS_OK;
}

}  // extern "C"
