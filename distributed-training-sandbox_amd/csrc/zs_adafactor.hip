// Fused Adafactor (Shazeer & Stern 2018, arXiv:1804.04235; torch.optim.Adafactor's rule) for CDNA4
// (gfx950): the first shape-aware update of the library.  The second moment of an R x C matrix is
// one row vector and one column vector, so a step needs the row and column sums of g^2, the RMS of
// the parameter and the norm of the whole update before it writes its first element: three passes
// over a table with one entry per (parameter, batch matrix), small reduce kernels between them,
// every scalar on the device.  No atomics: each tile writes its partials to its own slots and the
// reductions walk them in an order fixed by the parameter's shape alone.
//
// Tiling (matrix entries).  A workgroup (256 threads, 4 waves) owns a tile of kTileRows rows x
// 64 * V columns, V = 16 bytes of gradient per lane (8 bf16, 4 fp32).  The waves interleave over
// the tile's rows (wave w takes rows w, w + 4, ...), one row per step: a row of the tile is one
// 16-byte load per lane (vector path, C % V == 0, all row starts 16-byte aligned) or V element loads
// strided by 64 (scalar path: any C).  A lane keeps the sums of g^2 of its V columns in registers
// -- fp32 over kRowGroup rows, added into V doubles between groups -- and the four waves combine
// them through LDS once per tile; a row's sum over the tile's column span is V fp32 terms per
// lane, then one double reduction across the wave per row.  Pass A's loads of the master also feed
// sum p^2.  1-D entries (variance per element) run chunks of 1024 elements through the same
// kernels and need no factor arrays.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "zs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileRows = 256;  // rows of a tile: 64 per wave
constexpr int kRowGroup = 16;   // rows a lane sums in fp32 before it adds into its doubles
constexpr int kRowsPerWave = kTileRows / kWaves;
constexpr int kChunk1d = kThreads * 4;  // elements of a 1-D entry per workgroup

#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
using gptr = __attribute__((address_space(1))) T*;
#else
template <typename T>
using gptr = T*;
#endif

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// pass A and B read what a later pass reads again, but a C4-sized set is far beyond the caches:
// every stream carries the non-temporal hint, as in the element-wise update
__device__ __forceinline__ uint4 ld16(const void* p) {
  const u32x4 v = __builtin_nontemporal_load((gptr<const u32x4>)p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint2 ld8(const void* p) {
  const u32x2 v = __builtin_nontemporal_load((gptr<const u32x2>)p);
  return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void st16(void* p, uint4 x) {
  const u32x4 v = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(v, (gptr<u32x4>)p);
}
__device__ __forceinline__ void st8(void* p, uint2 x) {
  const u32x2 v = {x.x, x.y};
  __builtin_nontemporal_store(v, (gptr<u32x2>)p);
}

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {  // RNE; a NaN stays a NaN
  __bf16 h = static_cast<__bf16>(f);
  unsigned short r;
  __builtin_memcpy(&r, &h, 2);
  return r;
}
// the split master (include/zero_amd.h, ZS_BF16_SPLIT): u = (hi << 16) + sext(lo)
__device__ __forceinline__ float join_master(uint32_t hi, uint32_t lo) {
  return __uint_as_float((hi << 16) + uint32_t(int32_t(int16_t(uint16_t(lo)))));
}
__device__ __forceinline__ uint32_t master_residual(float p, uint32_t hi) {
  const uint32_t d = __float_as_uint(p) - (hi << 16);
  return d == 0x8000u ? 0x7FFFu : (d & 0xFFFFu);
}

struct AfEntry {
  const void* g;          // the reduced gradient sum, GT
  const void* master;     // fp32 master, or (split) the bf16 parameter
  void* master_out;       // fp32 master (in place), or (split) the int16 residual, read and written
  unsigned short* p_out;  // bf16 copy of the updated parameter; (split) the bf16 parameter; or null
  float* row_var;         // R floats; a 1-D entry: variance, C floats
  float* col_var;         // C floats; null marks a 1-D entry
  float* rfac;            // scratch, R floats: row_var[i] / max(mean_i row_var, eps1)
  double* rowp;           // scratch, [ct][R]: each column tile's sum of g^2 per row
  double* colp;           // scratch, [rt][C]: each row tile's sum of g^2 per column
  int64_t slot0;          // the entry's first slot of the per-tile sums (sum p^2, sum u^2)
  int32_t R, C;           // a 1-D entry: R = 1, C = n
  int32_t rt, ct;         // row and column tiles (1-D: 1 and its chunks)
  int32_t param;          // the set's dense index of the entry's parameter
  int32_t vec;            // the vector path
};

struct AfParam {
  int64_t slot_lo, slot_hi;  // the parameter's slots, its entries' in table order
  double sqrt_numel;
};

struct AfHP {
  float lerp_w;  // ATen's lerp with weight w = t^beta2_decay: w, or w - 1 when lerp_hi
  float eps1, eps1_sq, eps2, rho, d, decay_mul;
  float grad_div, inv_div;
  int lerp_hi, div_pow2, maximize;
};

// the entry of workgroup b: prefix[e] <= b < prefix[e + 1]
__device__ __forceinline__ int64_t find_entry(const int64_t* __restrict__ prefix, int64_t nent,
                                              int64_t b) {
  int64_t e = 0, hi = nent;
  while (hi - e > 1) {
    const int64_t mid = (e + hi) >> 1;
    if (prefix[mid] <= b) e = mid;
    else hi = mid;
  }
  return e;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
  return x;  // lane 0 holds the sum
}

__device__ __forceinline__ double block_sum(double x, double* wave_part) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

// the averaged gradient the rule starts from: `grad / ws` (a power-of-two divisor is an exact
// reciprocal multiply) and maximize
__device__ __forceinline__ float prep_grad(float s, const AfHP& hp) {
#pragma clang fp contract(off)
  float g = hp.div_pow2 ? s * hp.inv_div : s / hp.grad_div;
  if (hp.maximize) g = -g;
  return g;
}

// ATen's lerp (Lerp.h): self + w * (end - self) for |w| < 0.5, end - (end - self) * (1 - w) otherwise
__device__ __forceinline__ float lerp_to(float self, float end, const AfHP& hp) {
#pragma clang fp contract(off)
  return fmaf(hp.lerp_w, end - self, hp.lerp_hi ? end : self);
}

// u = g * rsqrt(max(v, eps1^2)); a NaN v stays a NaN, as torch's clamp_ keeps it
__device__ __forceinline__ float update_of(float g, float v, const AfHP& hp) {
#pragma clang fp contract(off)
  const float vc = v < hp.eps1_sq ? hp.eps1_sq : v;
  return g * (1.0f / sqrtf(vc));
}

template <typename GT>
__device__ __forceinline__ float load_g1(const void* g, int64_t i) {
  if constexpr (sizeof(GT) == 4) return ((gptr<const float>)g)[i];
  else return __uint_as_float(uint32_t(((gptr<const unsigned short>)g)[i]) << 16);
}
template <bool SPLIT>
__device__ __forceinline__ float load_p1(const AfEntry& e, int64_t i) {
  if constexpr (SPLIT)
    return join_master(((gptr<const unsigned short>)e.master)[i],
                       ((gptr<const unsigned short>)e.master_out)[i]);
  else return ((gptr<const float>)e.master)[i];
}
template <bool SPLIT>
__device__ __forceinline__ void store_p1(const AfEntry& e, int64_t i, float p) {
  if constexpr (SPLIT) {
    const uint32_t hi = f32_to_bf16(p);
    ((gptr<unsigned short>)e.p_out)[i] = (unsigned short)hi;
    ((gptr<unsigned short>)e.master_out)[i] = (unsigned short)master_residual(p, hi);
  } else {
    ((gptr<float>)e.master_out)[i] = p;
    if (e.p_out) ((gptr<unsigned short>)e.p_out)[i] = f32_to_bf16(p);
  }
}

// One lane's V elements of row `row` (element offset of the row: row * C): columns c .. c + V - 1
// (vector path, one whole 16-byte gradient load) or c, c + 64, ... (scalar path, each column
// checked against C).  What lies outside reads as 0.
template <typename GT, int V, bool VEC>
__device__ __forceinline__ void load_g(const AfEntry& e, int64_t row_off, int c, float* g) {
  if constexpr (VEC) {
    const int64_t i = row_off + c;
    const uint4 q = ld16(static_cast<const GT*>(e.g) + i);
    if constexpr (sizeof(GT) == 4) {
      g[0] = __uint_as_float(q.x), g[1] = __uint_as_float(q.y);
      g[2] = __uint_as_float(q.z), g[3] = __uint_as_float(q.w);
    } else {
      g[0] = __uint_as_float(q.x << 16), g[1] = __uint_as_float(q.x & 0xffff0000u);
      g[2] = __uint_as_float(q.y << 16), g[3] = __uint_as_float(q.y & 0xffff0000u);
      g[4] = __uint_as_float(q.z << 16), g[5] = __uint_as_float(q.z & 0xffff0000u);
      g[6] = __uint_as_float(q.w << 16), g[7] = __uint_as_float(q.w & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      g[j] = c + j * 64 < e.C ? load_g1<GT>(e.g, row_off + c + j * 64) : 0.0f;
  }
}

template <int V, bool VEC, bool SPLIT>
__device__ __forceinline__ void load_p(const AfEntry& e, int64_t row_off, int c, float* p) {
  if constexpr (VEC) {
    const int64_t i = row_off + c;
    if constexpr (SPLIT) {
      uint32_t h[V / 2], l[V / 2];  // two 16-bit words each
      if constexpr (V == 8) {
        const uint4 a = ld16(static_cast<const unsigned short*>(e.master) + i);
        const uint4 b = ld16(static_cast<const unsigned short*>(e.master_out) + i);
        h[0] = a.x, h[1] = a.y, h[2] = a.z, h[3] = a.w;
        l[0] = b.x, l[1] = b.y, l[2] = b.z, l[3] = b.w;
      } else {
        const uint2 a = ld8(static_cast<const unsigned short*>(e.master) + i);
        const uint2 b = ld8(static_cast<const unsigned short*>(e.master_out) + i);
        h[0] = a.x, h[1] = a.y;
        l[0] = b.x, l[1] = b.y;
      }
#pragma unroll
      for (int k = 0; k < V / 2; ++k) {
        p[2 * k] = join_master(h[k] & 0xFFFFu, l[k]);
        p[2 * k + 1] = join_master(h[k] >> 16, l[k] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < V / 4; ++k) {
        const uint4 q = ld16(static_cast<const float*>(e.master) + i + 4 * k);
        p[4 * k] = __uint_as_float(q.x), p[4 * k + 1] = __uint_as_float(q.y);
        p[4 * k + 2] = __uint_as_float(q.z), p[4 * k + 3] = __uint_as_float(q.w);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      p[j] = c + j * 64 < e.C ? load_p1<SPLIT>(e, row_off + c + j * 64) : 0.0f;
  }
}

template <int V, bool VEC, bool SPLIT>
__device__ __forceinline__ void store_p(const AfEntry& e, int64_t row_off, int c, const float* p) {
  if constexpr (VEC) {
    const int64_t i = row_off + c;
    uint32_t h[V];
#pragma unroll
    for (int j = 0; j < V; ++j) h[j] = f32_to_bf16(p[j]);
    if constexpr (SPLIT) {
      uint32_t l[V];
#pragma unroll
      for (int j = 0; j < V; ++j) l[j] = master_residual(p[j], h[j]);
      if constexpr (V == 8) {
        st16(e.p_out + i, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                     h[6] | (h[7] << 16)));
        st16(static_cast<unsigned short*>(e.master_out) + i,
             make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16),
                        l[6] | (l[7] << 16)));
      } else {
        st8(e.p_out + i, make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16)));
        st8(static_cast<unsigned short*>(e.master_out) + i,
            make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16)));
      }
    } else {
#pragma unroll
      for (int k = 0; k < V / 4; ++k)
        st16(static_cast<float*>(e.master_out) + i + 4 * k,
             make_uint4(__float_as_uint(p[4 * k]), __float_as_uint(p[4 * k + 1]),
                        __float_as_uint(p[4 * k + 2]), __float_as_uint(p[4 * k + 3])));
      if (e.p_out) {
        if constexpr (V == 8)
          st16(e.p_out + i, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16),
                                       h[4] | (h[5] << 16), h[6] | (h[7] << 16)));
        else st8(e.p_out + i, make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16)));
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (c + j * 64 < e.C) store_p1<SPLIT>(e, row_off + c + j * 64, p[j]);
  }
}

struct TileLds {
  double col[kWaves][64 * 8];  // pass A: each wave's column sums of the tile (16 KiB)
  double wave_part[kWaves];
};

// One tile of a matrix entry.  PASS 0 (A): sums of g^2 per row and per column and sum p^2; PASS 1
// (B): sum u^2; PASS 2 (C): the update.  The lane's column index inside the tile is `ci` for its
// element j: lane * V + j (vector) or j * 64 + lane (scalar).
template <typename GT, bool SPLIT, bool VEC, int PASS>
__device__ __forceinline__ void tile_body(const AfEntry& e, int64_t t, const AfHP& hp,
                                          double* __restrict__ sums, const float* __restrict__ nad,
                                          TileLds& lds) {
#pragma clang fp contract(off)
  constexpr int V = 16 / int(sizeof(GT));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tr = int(t / e.ct), tc = int(t % e.ct);
  const int r0 = tr * kTileRows, c0 = tc * 64 * V;
  const int c = c0 + (VEC ? lane * V : lane);  // the lane's first column
  const bool live = VEC ? c < e.C : true;      // (scalar path: checked per column)
  float colacc[V];
  double coldbl[V];
  float cv[V];
  double tile_sum = 0.0;  // PASS 0: sum p^2; PASS 1: sum u^2
  float step = 0.0f;
  if constexpr (PASS == 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) colacc[j] = 0.0f, coldbl[j] = 0.0;
  } else {  // the lane's column factors, once per tile
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int cj = VEC ? c + j : c + j * 64;
      cv[j] = (live && cj < e.C) ? e.col_var[cj] : 0.0f;
    }
    if constexpr (PASS == 2) step = nad[e.param];
  }
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int row = r0 + k * kWaves + wave;
    if (row < e.R) {  // (uniform per wave)
      const int64_t row_off = int64_t(row) * e.C;
      float g[V], p[V];
#pragma unroll
      for (int j = 0; j < V; ++j) g[j] = 0.0f, p[j] = 0.0f;
      if (live) {
        load_g<GT, V, VEC>(e, row_off, c, g);
        if constexpr (PASS != 1) load_p<V, VEC, SPLIT>(e, row_off, c, p);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) g[j] = prep_grad(g[j], hp);
      if constexpr (PASS == 0) {
        float rs = 0.0f, ps = 0.0f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          rs = fmaf(g[j], g[j], rs);
          colacc[j] = fmaf(g[j], g[j], colacc[j]);
          ps = fmaf(p[j], p[j], ps);
        }
        tile_sum += double(ps);
        const double rsum = wave_sum(double(rs));  // once per row and tile
        if (lane == 0) e.rowp[int64_t(tc) * e.R + row] = rsum;
      } else {
        const float rf = e.rfac[row];  // (wave-uniform)
        float us = 0.0f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float u = update_of(g[j], rf * cv[j], hp);
          if constexpr (PASS == 1) us = fmaf(u, u, us);
          else p[j] = fmaf(step, u, p[j] * hp.decay_mul);
        }
        if constexpr (PASS == 1) tile_sum += double(us);
        else if (live) store_p<V, VEC, SPLIT>(e, row_off, c, p);
      }
    }
    if constexpr (PASS == 0) {
      if ((k + 1) % kRowGroup == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) coldbl[j] += double(colacc[j]), colacc[j] = 0.0f;
      }
    }
  }
  if constexpr (PASS == 0) {  // the waves' column sums through LDS, once per tile
#pragma unroll
    for (int j = 0; j < V; ++j) lds.col[wave][VEC ? lane * V + j : j * 64 + lane] = coldbl[j];
    __syncthreads();
    for (int ci = threadIdx.x; ci < 64 * V; ci += kThreads) {
      if (c0 + ci < e.C)
        e.colp[int64_t(tr) * e.C + c0 + ci] =
            ((lds.col[0][ci] + lds.col[1][ci]) + lds.col[2][ci]) + lds.col[3][ci];
    }
  }
  if constexpr (PASS != 2) {
    const double b = block_sum(tile_sum, lds.wave_part);
    if (threadIdx.x == 0) sums[e.slot0 + t] = b;
  }
}

// One chunk of a 1-D entry (variance per element, no factors).  PASS 0: sum p^2; PASS 1: the
// variance lerp, written, and sum u^2; PASS 2: the update from the updated variance.
template <typename GT, bool SPLIT, int PASS>
__device__ __forceinline__ void chunk_body(const AfEntry& e, int64_t t, const AfHP& hp,
                                           double* __restrict__ sums,
                                           const float* __restrict__ nad, TileLds& lds) {
#pragma clang fp contract(off)
  double acc = 0.0;
  float step = 0.0f;
  if constexpr (PASS == 2) step = nad[e.param];
  float part = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = t * kChunk1d + j * kThreads + threadIdx.x;
    if (i < e.C) {
      if constexpr (PASS == 0) {
        const float p = load_p1<SPLIT>(e, i);
        part = fmaf(p, p, part);
      } else {
        const float g = prep_grad(load_g1<GT>(e.g, i), hp);
        float var = e.row_var[i];
        if constexpr (PASS == 1) {
          var = lerp_to(var, g * g, hp);
          e.row_var[i] = var;
        }
        const float u = update_of(g, var, hp);
        if constexpr (PASS == 1) part = fmaf(u, u, part);
        else store_p1<SPLIT>(e, i, fmaf(step, u, load_p1<SPLIT>(e, i) * hp.decay_mul));
      }
    }
  }
  acc = double(part);
  if constexpr (PASS != 2) {
    const double b = block_sum(acc, lds.wave_part);
    if (threadIdx.x == 0) sums[e.slot0 + t] = b;
  }
}

// kernel-resource-usage (gfx950, hipcc of ROCm 7): see DESIGN.md §4 "Fused Adafactor"
template <typename GT, bool SPLIT, int PASS>
__global__ __launch_bounds__(kThreads) void adafactor_pass_kernel(
    const AfEntry* __restrict__ entries, const int64_t* __restrict__ tile_prefix, int64_t nent,
    const AfHP hp, double* __restrict__ sums, const float* __restrict__ nad) {
  __shared__ TileLds lds;
  const int64_t ei = find_entry(tile_prefix, nent, blockIdx.x);
  const AfEntry e = entries[ei];
  const int64_t t = int64_t(blockIdx.x) - tile_prefix[ei];
  if (e.col_var == nullptr) chunk_body<GT, SPLIT, PASS>(e, t, hp, sums, nad, lds);
  else if (e.vec) tile_body<GT, SPLIT, true, PASS>(e, t, hp, sums, nad, lds);
  else tile_body<GT, SPLIT, false, PASS>(e, t, hp, sums, nad, lds);
}

// After pass A: thread x of a matrix entry's workgroups takes row x (x < R) or column x - R: the
// tile partials in tile order, the mean, the lerp into row_var / col_var.
__global__ __launch_bounds__(kThreads) void adafactor_factors_kernel(
    const AfEntry* __restrict__ entries, const int64_t* __restrict__ red_prefix, int64_t nent,
    const AfHP hp) {
#pragma clang fp contract(off)
  const int64_t ei = find_entry(red_prefix, nent, blockIdx.x);
  const AfEntry e = entries[ei];
  const int64_t x = (int64_t(blockIdx.x) - red_prefix[ei]) * kThreads + threadIdx.x;
  if (e.col_var == nullptr || x >= int64_t(e.R) + e.C) return;
  double s = 0.0;
  if (x < e.R) {
    for (int k = 0; k < e.ct; ++k) s += e.rowp[int64_t(k) * e.R + x];
    e.row_var[x] = lerp_to(e.row_var[x], float(s / double(e.C)), hp);
  } else {
    const int64_t j = x - e.R;
    for (int k = 0; k < e.rt; ++k) s += e.colp[int64_t(k) * e.C + j];
    e.col_var[j] = lerp_to(e.col_var[j], float(s / double(e.R)), hp);
  }
}

// Sum of slots [lo, hi) by one workgroup: thread t takes slots lo + t, lo + t + 256, ...
__device__ __forceinline__ double slots_sum(const double* __restrict__ sums, int64_t lo, int64_t hi,
                                            double* wave_part) {
  double s = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) s += sums[i];
  return block_sum(s, wave_part);
}

// After the factors: workgroup b < nent forms entry b's row factors row_var[i] / max(mean_i
// row_var, eps1); workgroup nent + q forms alpha of parameter q from its sum p^2.
__global__ __launch_bounds__(kThreads) void adafactor_finish_a_kernel(
    const AfEntry* __restrict__ entries, int64_t nent, const AfParam* __restrict__ params,
    const AfHP hp, const double* __restrict__ psq, double* __restrict__ alpha) {
#pragma clang fp contract(off)
  __shared__ double wave_part[kWaves];
  if (int64_t(blockIdx.x) < nent) {
    const AfEntry e = entries[blockIdx.x];
    if (e.col_var == nullptr) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < e.R; i += kThreads) s += double(e.row_var[i]);
    float m = float(block_sum(s, wave_part) / double(e.R));
    m = m < hp.eps1 ? hp.eps1 : m;  // clamp_(min=eps1): a NaN stays
    for (int i = threadIdx.x; i < e.R; i += kThreads) e.rfac[i] = e.row_var[i] / m;
    return;
  }
  const int64_t q = int64_t(blockIdx.x) - nent;
  const AfParam pr = params[q];
  const double s = slots_sum(psq, pr.slot_lo, pr.slot_hi, wave_part);
  if (threadIdx.x == 0) {
    const double rms = sqrt(s) / pr.sqrt_numel;
    alpha[q] = (rms > double(hp.eps2) ? rms : double(hp.eps2)) * double(hp.rho);
  }
}

// After pass B: -alpha / max(1, ||u|| / (sqrt(numel) * d)) per parameter, rounded to fp32 once.
__global__ __launch_bounds__(kThreads) void adafactor_finish_b_kernel(
    const AfParam* __restrict__ params, const AfHP hp, const double* __restrict__ usq,
    const double* __restrict__ alpha, float* __restrict__ nad) {
#pragma clang fp contract(off)
  __shared__ double wave_part[kWaves];
  const AfParam pr = params[blockIdx.x];
  const double s = slots_sum(usq, pr.slot_lo, pr.slot_hi, wave_part);
  if (threadIdx.x == 0) {
    const double y = sqrt(s) / (pr.sqrt_numel * double(hp.d));
    nad[blockIdx.x] = float(-alpha[blockIdx.x] / (y > 1.0 ? y : 1.0));
  }
}

hipStream_t upload_stream() {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  streams[dev] = s;
  return s;
}

template <typename T>
int upload(const std::vector<T>& h, T** d) {
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

bool aligned(uint64_t p, uint64_t a) { return (p & (a - 1)) == 0; }

}  // namespace

struct zs_adafactorset {
  unsigned tag = zs::kAdafactorSetTag;
  AfEntry* d_entries = nullptr;
  int64_t* d_tile_prefix = nullptr;
  int64_t* d_red_prefix = nullptr;
  AfParam* d_params = nullptr;
  // one allocation: [psq | usq | alpha] doubles, the entries' rowp / colp doubles, then the floats
  // (nad, the entries' rfac)
  unsigned char* d_scratch = nullptr;
  double *d_psq = nullptr, *d_usq = nullptr, *d_alpha = nullptr;
  float* d_nad = nullptr;
  int64_t nent = 0, nparam = 0, tiles = 0, red_blocks = 0;
  int64_t elems = 0, bytes = 0, pass_bytes[3] = {0, 0, 0}, scratch_bytes = 0;
  int g_dtype = ZS_F32, p_dtype = ZS_BF16;
};

// mask: bit 0 = pass A with the factor and alpha kernels behind it, bit 1 = pass B with the step
// kernel behind it, bit 2 = pass C
template <typename GT, bool SPLIT>
static int run_passes(const zs_adafactorset* s, const AfHP& hp, hipStream_t st, int mask) {
  const dim3 grid(static_cast<unsigned>(s->tiles)), block(kThreads);
  if (mask & 1) {
    adafactor_pass_kernel<GT, SPLIT, 0><<<grid, block, 0, st>>>(s->d_entries, s->d_tile_prefix,
                                                                s->nent, hp, s->d_psq, s->d_nad);
    if (s->red_blocks)
      adafactor_factors_kernel<<<dim3(static_cast<unsigned>(s->red_blocks)), block, 0, st>>>(
          s->d_entries, s->d_red_prefix, s->nent, hp);
    adafactor_finish_a_kernel<<<dim3(static_cast<unsigned>(s->nent + s->nparam)), block, 0, st>>>(
        s->d_entries, s->nent, s->d_params, hp, s->d_psq, s->d_alpha);
  }
  if (mask & 2) {
    adafactor_pass_kernel<GT, SPLIT, 1><<<grid, block, 0, st>>>(s->d_entries, s->d_tile_prefix,
                                                                s->nent, hp, s->d_usq, s->d_nad);
    adafactor_finish_b_kernel<<<dim3(static_cast<unsigned>(s->nparam)), block, 0, st>>>(
        s->d_params, hp, s->d_usq, s->d_alpha, s->d_nad);
  }
  if (mask & 4)
    adafactor_pass_kernel<GT, SPLIT, 2><<<grid, block, 0, st>>>(s->d_entries, s->d_tile_prefix,
                                                                s->nent, hp, s->d_usq, s->d_nad);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

static int run_checked(const char* fn, const zs_adafactorset* as, const zs_adafactor_hparams* h,
                       int64_t step, int mask, uintptr_t stream) {
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(as->tag == zs::kAdafactorSetTag,
             "%s: the set was not made by zs_adafactorset_create", fn);
  ZS_REQUIRE(step >= 1, "%s: step must be >= 1 (the count after this step; got %lld)", fn,
             (long long)step);
  // a struct filled by hand gets zs_adafactor_hparams_init's rules too
  ZS_REQUIRE(h->lr > 0.0, "%s: invalid learning rate", fn);
  ZS_REQUIRE(h->beta2_decay <= 0.0, "%s: beta2_decay should be <= 0", fn);
  ZS_REQUIRE(h->eps1 >= 0.0 && h->eps2 > 0.0, "%s: invalid epsilon", fn);
  ZS_REQUIRE(h->d >= 1.0, "%s: clipping threshold d should be >= 1", fn);
  ZS_REQUIRE(h->weight_decay >= 0.0, "%s: invalid weight_decay", fn);
  ZS_REQUIRE(h->grad_div > 0.0, "%s: grad_div must be > 0", fn);
  if (as->nent == 0) return ZS_OK;
  // the host scalars in double, each rounded to fp32 once
  const double t = double(step);
  AfHP hp;
  const float w = float(std::pow(t, h->beta2_decay));
  hp.lerp_hi = std::fabs(w) < 0.5f ? 0 : 1;
  hp.lerp_w = hp.lerp_hi ? w - 1.0f : w;
  hp.eps1 = float(h->eps1);
  hp.eps1_sq = float(h->eps1 * h->eps1);
  hp.eps2 = float(h->eps2);
  hp.rho = float(std::min(h->lr, 1.0 / std::sqrt(t)));
  hp.d = float(h->d);
  hp.decay_mul = h->weight_decay != 0.0 ? float(1.0 - h->lr * h->weight_decay) : 1.0f;
  int exp2 = 0;
  hp.grad_div = float(h->grad_div);
  hp.div_pow2 = std::frexp(double(hp.grad_div), &exp2) == 0.5 ? 1 : 0;
  hp.inv_div = float(1.0 / double(hp.grad_div));
  hp.maximize = h->maximize ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool g32 = as->g_dtype == ZS_F32, split = as->p_dtype == ZS_BF16_SPLIT;
  if (g32)
    return split ? run_passes<float, true>(as, hp, st, mask)
                 : run_passes<float, false>(as, hp, st, mask);
  return split ? run_passes<unsigned short, true>(as, hp, st, mask)
               : run_passes<unsigned short, false>(as, hp, st, mask);
}

extern "C" {

int zs_adafactor_hparams_init(double lr, double beta2_decay, int has_eps1, double eps1, double eps2,
                              double d, double weight_decay, int maximize, double grad_div,
                              zs_adafactor_hparams* hp) {
  const char* fn = "zs_adafactor_hparams_init";
  ZS_REQUIRE(hp != nullptr, "%s: hp is NULL", fn);
  ZS_REQUIRE(grad_div > 0.0, "%s: grad_div must be > 0", fn);
  // torch.optim.Adafactor.__init__'s rules (lr = 0 would make rho 0: the library asks for lr > 0)
  ZS_REQUIRE(lr > 0.0, "%s: invalid learning rate %g", fn, lr);
  ZS_REQUIRE(beta2_decay <= 0.0, "%s: beta2_decay should be <= 0 but is %g", fn, beta2_decay);
  ZS_REQUIRE(!has_eps1 || eps1 >= 0.0, "%s: epsilon1 should be >= 0 but is %g", fn, eps1);
  ZS_REQUIRE(eps2 > 0.0, "%s: epsilon2 should be > 0 but is %g", fn, eps2);
  ZS_REQUIRE(d >= 1.0, "%s: clipping threshold d should be >= 1 but is %g", fn, d);
  ZS_REQUIRE(weight_decay >= 0.0, "%s: invalid weight_decay %g", fn, weight_decay);
  hp->lr = lr;
  hp->beta2_decay = beta2_decay;
  hp->eps1 = has_eps1 ? eps1 : 1.1920928955078125e-07;  // fp32's epsilon: the arithmetic is fp32
  hp->eps2 = eps2;
  hp->d = d;
  hp->weight_decay = weight_decay;
  hp->grad_div = grad_div;
  hp->maximize = maximize ? 1 : 0;
  hp->reserved = 0;
  return ZS_OK;
}

int zs_adafactorset_create(const zs_adafactor_seg* in, int64_t n, int g_dtype, int p_dtype,
                           zs_adafactorset** out) {
  const char* fn = "zs_adafactorset_create";
  ZS_REQUIRE(out != nullptr, "%s: out is NULL", fn);
  *out = nullptr;
  ZS_REQUIRE(n >= 0 && (n == 0 || in), "%s: bad table", fn);
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "%s: bad g_dtype %d", fn, g_dtype);
  ZS_REQUIRE(p_dtype == ZS_BF16 || p_dtype == ZS_BF16_SPLIT,
             "%s: p_dtype must be ZS_BF16 or ZS_BF16_SPLIT (got %d)", fn, p_dtype);
  ZS_REQUIRE(n < (int64_t(1) << 31), "%s: %lld entries (max 2^31 - 1)", fn, (long long)n);
  const bool split = p_dtype == ZS_BF16_SPLIT;
  const int64_t gsz = g_dtype == ZS_F32 ? 4 : 2, V = 16 / gsz;
  const int64_t msz = split ? 2 : 4;
  std::vector<AfEntry> ent;
  std::vector<AfParam> par;
  std::vector<int64_t> tpre(1, 0), rpre(1, 0);
  std::vector<int64_t> rowp_off, colp_off, rfac_off;  // per entry, in doubles / floats
  int64_t slots = 0, dbl = 0, flt = 0, elems = 0, last_param = -1;
  int64_t pass_bytes[3] = {0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const zs_adafactor_seg& s = in[i];
    ZS_REQUIRE(s.R >= 1 && s.C >= 1, "%s: entry %lld: R and C must be >= 1", fn, (long long)i);
    ZS_REQUIRE(s.R < (int64_t(1) << 31) && s.C < (int64_t(1) << 31) &&
                   s.R * s.C < (int64_t(1) << 40),
               "%s: entry %lld: R or C too large", fn, (long long)i);
    ZS_REQUIRE(s.g && s.master && s.master_out && s.row_var,
               "%s: entry %lld missing g/master/master_out/row_var", fn, (long long)i);
    ZS_REQUIRE(s.col_var || s.R == 1,
               "%s: entry %lld: a 1-D entry (col_var == 0: row_var is the variance) has R == 1", fn,
               (long long)i);
    ZS_REQUIRE(!split || s.p_out, "%s: entry %lld: a split master needs p_out", fn, (long long)i);
    ZS_REQUIRE(split || s.master_out == s.master,
               "%s: entry %lld: the fp32 master is updated in place (master_out == master)", fn,
               (long long)i);
    ZS_REQUIRE(aligned(s.g, uint64_t(gsz)) && aligned(s.master, uint64_t(msz)) &&
                   aligned(s.master_out, uint64_t(msz)) && aligned(s.p_out, 2) &&
                   aligned(s.row_var, 4) && aligned(s.col_var, 4),
               "%s: entry %lld: a pointer is not aligned to its element", fn, (long long)i);
    ZS_REQUIRE(s.param >= 0, "%s: entry %lld: param < 0", fn, (long long)i);
    // a parameter's entries (the matrices of its batch) stand together: its slots are one range
    if (s.param != last_param) {
      for (const zs_adafactor_seg* q = in; q < in + i; ++q)
        ZS_REQUIRE(q->param != s.param, "%s: entry %lld: the entries of parameter %lld are not "
                   "adjacent", fn, (long long)i, (long long)s.param);
      par.push_back(AfParam{slots, slots, 0.0});
      last_param = s.param;
    }
    AfEntry e{};
    e.g = reinterpret_cast<const void*>(s.g);
    e.master = reinterpret_cast<const void*>(s.master);
    e.master_out = reinterpret_cast<void*>(s.master_out);
    e.p_out = reinterpret_cast<unsigned short*>(s.p_out);
    e.row_var = reinterpret_cast<float*>(s.row_var);
    e.col_var = reinterpret_cast<float*>(s.col_var);
    e.R = int32_t(s.R), e.C = int32_t(s.C);
    e.param = int32_t(par.size() - 1);
    e.slot0 = slots;
    const bool oned = s.col_var == 0;
    if (oned) {
      e.rt = 1, e.ct = int32_t((s.C + kChunk1d - 1) / kChunk1d);
      rowp_off.push_back(0), colp_off.push_back(0), rfac_off.push_back(0);
      rpre.push_back(rpre.back());
    } else {
      e.rt = int32_t((s.R + kTileRows - 1) / kTileRows);
      e.ct = int32_t((s.C + 64 * V - 1) / (64 * V));
      // the vector path: every row start 16-byte aligned in every stream
      e.vec = s.R > 1 && s.C % V == 0 && aligned(s.g, 16) && aligned(s.master, uint64_t(msz * V)) &&
              aligned(s.master_out, uint64_t(msz * V)) && aligned(s.p_out, uint64_t(2 * V));
      rowp_off.push_back(dbl), dbl += int64_t(e.ct) * s.R;
      colp_off.push_back(dbl), dbl += int64_t(e.rt) * s.C;
      rfac_off.push_back(flt), flt += (s.R + 3) / 4 * 4;
      rpre.push_back(rpre.back() + (s.R + s.C + kThreads - 1) / kThreads);
    }
    const int64_t t = int64_t(e.rt) * e.ct;
    slots += t;
    ZS_REQUIRE(tpre.back() + t < (int64_t(1) << 31), "%s: too many tiles", fn);
    tpre.push_back(tpre.back() + t);
    par.back().slot_hi = slots;
    par.back().sqrt_numel += double(s.R * s.C);  // (the count until the loop ends)
    ent.push_back(e);
    const int64_t ne = s.R * s.C;
    elems += ne;
    const int64_t mrd = split ? 4 : 4;  // master read: hi + lo, or fp32
    pass_bytes[0] += ne * (gsz + mrd);
    pass_bytes[1] += ne * gsz + (oned ? ne * 8 : 0);
    pass_bytes[2] += ne * (gsz + mrd + 4 + (!split && s.p_out ? 2 : 0)) + (oned ? ne * 4 : 0);
  }
  for (AfParam& p : par) p.sqrt_numel = std::sqrt(p.sqrt_numel);
  zs_adafactorset* as = new (std::nothrow) zs_adafactorset();
  if (!as) return zs::fail(ZS_ERR_NOMEM, "%s: out of memory", fn);
  as->nent = int64_t(ent.size());
  as->nparam = int64_t(par.size());
  as->tiles = tpre.back();
  as->red_blocks = rpre.back();
  as->elems = elems;
  for (int k = 0; k < 3; ++k) as->pass_bytes[k] = pass_bytes[k];
  as->bytes = pass_bytes[0] + pass_bytes[1] + pass_bytes[2];
  as->g_dtype = g_dtype;
  as->p_dtype = p_dtype;
  *out = as;
  if (as->nent == 0) return ZS_OK;
  // scratch: doubles [psq | usq | alpha | rowp / colp of every entry], floats [nad | rfac ...]
  const int64_t np = as->nparam;
  const int64_t dbl_total = 2 * slots + np + dbl;
  const int64_t nad_pad = (np + 3) / 4 * 4;
  as->scratch_bytes = dbl_total * 8 + (nad_pad + flt) * 4;
  int rc = ZS_OK;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&as->d_scratch), size_t(as->scratch_bytes));
  if (he != hipSuccess)
    rc = zs::fail(ZS_ERR_HIP, "%s: hipMalloc of %lld scratch bytes failed: %s", fn,
                  (long long)as->scratch_bytes, hipGetErrorString(he));
  if (rc == ZS_OK) {
    double* d0 = reinterpret_cast<double*>(as->d_scratch);
    as->d_psq = d0, as->d_usq = d0 + slots, as->d_alpha = d0 + 2 * slots;
    double* dent = d0 + 2 * slots + np;
    float* f0 = reinterpret_cast<float*>(d0 + dbl_total);
    as->d_nad = f0;
    for (size_t k = 0; k < ent.size(); ++k) {
      if (!ent[k].col_var) continue;
      ent[k].rowp = dent + rowp_off[k];
      ent[k].colp = dent + colp_off[k];
      ent[k].rfac = f0 + nad_pad + rfac_off[k];
    }
    rc = upload(ent, &as->d_entries);
  }
  if (rc == ZS_OK) rc = upload(tpre, &as->d_tile_prefix);
  if (rc == ZS_OK) rc = upload(rpre, &as->d_red_prefix);
  if (rc == ZS_OK) rc = upload(par, &as->d_params);
  if (rc != ZS_OK) {
    zs_adafactorset_destroy(as);
    *out = nullptr;
  }
  return rc;
}

int zs_adafactorset_run(const zs_adafactorset* as, const zs_adafactor_hparams* h, int64_t step,
                        uintptr_t stream) {
  return run_checked("zs_adafactorset_run", as, h, step, 7, stream);
}

int zs_adafactorset_run_pass(const zs_adafactorset* as, const zs_adafactor_hparams* h,
                             int64_t step, int pass, uintptr_t stream) {
  ZS_REQUIRE(pass >= 0 && pass <= 2, "zs_adafactorset_run_pass: pass must be 0, 1 or 2 (got %d)",
             pass);
  return run_checked("zs_adafactorset_run_pass", as, h, step, 1 << pass, stream);
}

int zs_adafactorset_stats(const zs_adafactorset* as, int64_t* elems, int64_t* bytes,
                          int64_t* pass_bytes, int64_t* scratch_bytes) {
  ZS_REQUIRE(as && elems && bytes, "zs_adafactorset_stats: NULL argument");
  ZS_REQUIRE(as->tag == zs::kAdafactorSetTag,
             "zs_adafactorset_stats: the set was not made by zs_adafactorset_create");
  *elems = as->elems;
  *bytes = as->bytes;
  if (pass_bytes)
    for (int k = 0; k < 3; ++k) pass_bytes[k] = as->pass_bytes[k];
  if (scratch_bytes) *scratch_bytes = as->scratch_bytes;
  return ZS_OK;
}

int zs_adafactorset_destroy(zs_adafactorset* as) {
  if (!as) return ZS_OK;
  ZS_REQUIRE(as->tag == zs::kAdafactorSetTag,
             "zs_adafactorset_destroy: the set was not made by zs_adafactorset_create");
  if (as->d_entries) (void)hipFree(as->d_entries);
  if (as->d_tile_prefix) (void)hipFree(as->d_tile_prefix);
  if (as->d_red_prefix) (void)hipFree(as->d_red_prefix);
  if (as->d_params) (void)hipFree(as->d_params);
  if (as->d_scratch) (void)hipFree(as->d_scratch);
  delete as;
  return ZS_OK;
}

}  // extern "C"
