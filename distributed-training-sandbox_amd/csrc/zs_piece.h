// What the per-parameter optimizer sets (csrc/zs_adamini.hip, csrc/zs_apollo.hip) share: 16-byte
// streaming accesses, a "piece" (16 bytes of gradient: V = 8 bf16 or 4 fp32 elements) of each
// stream with its element-access twin, the master encodings, the fixed reduction trees of a
// 256-thread workgroup, and the table upload.  Everything sits in an anonymous namespace: each
// translation unit that includes this gets its own, inlined.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "zs_common.h"

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
using gptr = __attribute__((address_space(1))) T*;
#else
template <typename T>
using gptr = T*;
#endif

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// a C4-sized set is far beyond the caches: every stream carries the non-temporal hint
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

// the entry of work item b: prefix[e] <= b < prefix[e + 1] (entries without items are passed over)
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

// (a workgroup of four waves)
__device__ __forceinline__ double block_sum(double x, double* wave_part) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

// ---- a piece: V consecutive elements from element i of a stream, the first n of them inside the
// ---- block (n >= V on the vector path); what lies outside reads as 0 and is not written
template <typename GT, bool VEC>
__device__ __forceinline__ uint4 load_g_piece(const void* g, int64_t i, int n) {
  if constexpr (VEC) {
    return ld16(static_cast<const GT*>(g) + i);
  } else if constexpr (sizeof(GT) == 4) {
    const gptr<const unsigned> s = (gptr<const unsigned>)g + i;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (n > 0) q.x = s[0];
    if (n > 1) q.y = s[1];
    if (n > 2) q.z = s[2];
    if (n > 3) q.w = s[3];
    return q;
  } else {
    const gptr<const unsigned short> s = (gptr<const unsigned short>)g + i;
    unsigned h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = j < n ? unsigned(s[j]) : 0u;
    return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                      h[6] | (h[7] << 16));
  }
}

template <typename GT>
__device__ __forceinline__ void unpack_g(uint4 q, float* g) {
  if constexpr (sizeof(GT) == 4) {
    g[0] = __uint_as_float(q.x), g[1] = __uint_as_float(q.y);
    g[2] = __uint_as_float(q.z), g[3] = __uint_as_float(q.w);
  } else {
    g[0] = __uint_as_float(q.x << 16), g[1] = __uint_as_float(q.x & 0xffff0000u);
    g[2] = __uint_as_float(q.y << 16), g[3] = __uint_as_float(q.y & 0xffff0000u);
    g[4] = __uint_as_float(q.z << 16), g[5] = __uint_as_float(q.z & 0xffff0000u);
    g[6] = __uint_as_float(q.w << 16), g[7] = __uint_as_float(q.w & 0xffff0000u);
  }
}

template <int V, bool VEC>
__device__ __forceinline__ void load_m(const float* m, int64_t i, int n, float* x) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < V / 4; ++k) {
      const uint4 q = ld16(m + i + 4 * k);
      x[4 * k] = __uint_as_float(q.x), x[4 * k + 1] = __uint_as_float(q.y);
      x[4 * k + 2] = __uint_as_float(q.z), x[4 * k + 3] = __uint_as_float(q.w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = j < n ? ((gptr<const float>)m)[i + j] : 0.0f;
  }
}

template <int V, bool VEC>
__device__ __forceinline__ void store_m(float* m, int64_t i, int n, const float* x) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < V / 4; ++k)
      st16(m + i + 4 * k, make_uint4(__float_as_uint(x[4 * k]), __float_as_uint(x[4 * k + 1]),
                                     __float_as_uint(x[4 * k + 2]), __float_as_uint(x[4 * k + 3])));
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (j < n) ((gptr<float>)m)[i + j] = x[j];
  }
}

// the master of an entry E (its fields master, master_out, p_out as in zs_adamini_seg)
template <int V, bool VEC, bool SPLIT, typename E>
__device__ __forceinline__ void load_p(const E& e, int64_t i, int n, float* p) {
  if constexpr (!VEC) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if constexpr (SPLIT)
        p[j] = j < n ? join_master(((gptr<const unsigned short>)e.master)[i + j],
                                   ((gptr<const unsigned short>)e.master_out)[i + j])
                     : 0.0f;
      else p[j] = j < n ? ((gptr<const float>)e.master)[i + j] : 0.0f;
    }
  } else if constexpr (SPLIT) {
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
}

template <int V, bool VEC, bool SPLIT, typename E>
__device__ __forceinline__ void store_p(const E& e, int64_t i, int n, const float* p) {
  uint32_t h[V];
#pragma unroll
  for (int j = 0; j < V; ++j) h[j] = f32_to_bf16(p[j]);
  if constexpr (!VEC) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (j >= n) continue;
      if constexpr (SPLIT) {
        ((gptr<unsigned short>)e.p_out)[i + j] = (unsigned short)h[j];
        ((gptr<unsigned short>)e.master_out)[i + j] = (unsigned short)master_residual(p[j], h[j]);
      } else {
        ((gptr<float>)e.master_out)[i + j] = p[j];
        if (e.p_out) ((gptr<unsigned short>)e.p_out)[i + j] = (unsigned short)h[j];
      }
    }
  } else if constexpr (SPLIT) {
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
        st16(e.p_out + i, make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                     h[6] | (h[7] << 16)));
      else st8(e.p_out + i, make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16)));
    }
  }
}

// ---- the host side: a set's tables go up once, on a stream of their own
inline hipStream_t upload_stream() {
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

inline bool aligned(uint64_t p, uint64_t a) { return (p & (a - 1)) == 0; }

}  // namespace
