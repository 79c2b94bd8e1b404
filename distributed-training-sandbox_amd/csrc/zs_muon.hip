// Fused Muon (torch.optim.Muon's rule: momentum, Newton-Schulz orthogonalisation, decoupled weight
// decay) for CDNA4 (gfx950): the first kernel of the library that runs on the matrix cores.  Per
// owned R x C matrix a step is two stream passes (M1: momentum and the norm's partial sums; M2: the
// normalised bf16 X and its transpose), ns_steps x three bf16 products on v_mfma_f32_32x32x16_bf16
// and one stream pass (P) that applies the orthogonalised update to the master.
//
// One NT product serves the whole iteration: D[M x N] = alpha * A[M x K] * Bop[N x K]^T + beta * E,
// K contiguous in both operands, because the Gram matrix A = X X^T and the polynomial
// Bm = b A + c A A^T are symmetric and X' = a X + Bm (X^T)^T.  The two symmetric products compute
// only the tiles with tile_n >= tile_m and store each tile's mirror image as well; the third stores
// X' and its transpose, so the next iteration again finds K contiguous.
//
// Work split.  A workgroup (256 threads, 4 waves as 2 x 2) owns a 128 x 128 tile of D; a wave owns
// 64 x 64 of it as 2 x 2 MFMAs of 32 x 32 (64 fp32 accumulators per lane).  K runs in steps of 64
// through two LDS stages of 2 x 128 rows x 128 bytes (64 KiB): the next step's 16-byte global loads
// are issued before the current step's MFMAs and written to the other stage after them, one barrier
// per step.  A row's eight 16-byte chunks are stored at chunk ^ (row & 7), so the 32 rows x 2 chunks
// an operand read touches spread over all banks.  Rows, columns and K outside the matrix are zeros
// in LDS (exact for a product); operands whose rows are not 16-byte aligned take element loads in
// the same kernel.  The epilogue rounds to bf16 once, stages the tile in LDS (the stages are free by
// then) and writes whole 16-byte row pieces; the mirror / transposed tile is staged the same way
// from the same registers, so it equals its source bit for bit.  grid z = the matrix of a batch of
// same-shape matrices; no workgroup waits on another.
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
constexpr int kChunk = kThreads * 4;  // elements of a stream pass per workgroup
constexpr int kTile = 128;            // the product's output tile
constexpr int kBK = 64;               // K per LDS stage
constexpr int kStageBytes = 2 * kTile * kBK * 2;  // A rows and Bop rows of one stage
constexpr int kOutStride = kTile + 8;  // halfwords per row of the staged output tile (272 B)
constexpr int kTr = 64;                // pass M2's transposition tile
constexpr int64_t kMaxBatch = 32768;   // grid z
constexpr int64_t kDefaultBudget = int64_t(1) << 30;

#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
using gptr = __attribute__((address_space(1))) T*;
#else
template <typename T>
using gptr = T*;
#endif

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short bf16_t;  // storage

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {  // RNE; a NaN stays a NaN
  __bf16 h = static_cast<__bf16>(f);
  unsigned short r;
  __builtin_memcpy(&r, &h, 2);
  return r;
}
__device__ __forceinline__ float bf16_to_f32(uint32_t h) { return __uint_as_float(h << 16); }
// the split master (include/zero_amd.h, ZS_BF16_SPLIT): u = (hi << 16) + sext(lo)
__device__ __forceinline__ float join_master(uint32_t hi, uint32_t lo) {
  return __uint_as_float((hi << 16) + uint32_t(int32_t(int16_t(uint16_t(lo)))));
}
__device__ __forceinline__ uint32_t master_residual(float p, uint32_t hi) {
  const uint32_t d = __float_as_uint(p) - (hi << 16);
  return d == 0x8000u ? 0x7FFFu : (d & 0xFFFFu);
}

struct MuEntry {
  const void* g;          // the reduced gradient sum, GT
  const void* master;     // fp32 master, or (split) the bf16 parameter
  void* master_out;       // fp32 master (in place), or (split) the int16 residual, read and written
  unsigned short* p_out;  // bf16 copy of the updated parameter; (split) the bf16 parameter; or null
  float* buf;             // fp32 momentum buffer, R * C
};

// ATen's lerp (Lerp.h) with a host-known weight w: self + w * (end - self) for |w| < 0.5,
// end - (end - self) * (1 - w) otherwise; `w` holds w, or w - 1 when `hi`
struct Lerp {
  float w;
  int hi;
};

struct MuHP {
  Lerp to_buf;  // buf = lerp(buf, g, 1 - momentum)
  Lerp to_u;    // u = lerp(g, buf, momentum) (nesterov)
  float eps, grad_div, inv_div;
  int nesterov, div_pow2;
};

__device__ __forceinline__ float lerp_to(float self, float end, const Lerp& l) {
#pragma clang fp contract(off)
  return fmaf(l.w, end - self, l.hi ? end : self);
}

// the averaged gradient the rule starts from: `grad / ws` (a power-of-two divisor is an exact
// reciprocal multiply)
__device__ __forceinline__ float prep_grad(float s, const MuHP& hp) {
#pragma clang fp contract(off)
  return hp.div_pow2 ? s * hp.inv_div : s / hp.grad_div;
}

template <typename GT>
__device__ __forceinline__ float load_g1(const void* g, int64_t i) {
  if constexpr (sizeof(GT) == 4) return ((gptr<const float>)g)[i];
  else return bf16_to_f32(((gptr<const unsigned short>)g)[i]);
}
template <bool SPLIT>
__device__ __forceinline__ float load_p1(const MuEntry& e, int64_t i) {
  if constexpr (SPLIT)
    return join_master(((gptr<const unsigned short>)e.master)[i],
                       ((gptr<const unsigned short>)e.master_out)[i]);
  else return ((gptr<const float>)e.master)[i];
}
template <bool SPLIT>
__device__ __forceinline__ void store_p1(const MuEntry& e, int64_t i, float p) {
  if constexpr (SPLIT) {
    const uint32_t hi = f32_to_bf16(p);
    ((gptr<unsigned short>)e.p_out)[i] = (unsigned short)hi;
    ((gptr<unsigned short>)e.master_out)[i] = (unsigned short)master_residual(p, hi);
  } else {
    ((gptr<float>)e.master_out)[i] = p;
    if (e.p_out) ((gptr<unsigned short>)e.p_out)[i] = f32_to_bf16(p);
  }
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

// the momentum and the update direction of one element; M1 stores the buffer, M2 reads the new one
template <typename GT, bool STORE>
__device__ __forceinline__ float update_of(const MuEntry& e, int64_t i, const MuHP& hp) {
  const float g = prep_grad(load_g1<GT>(e.g, i), hp);
  float b = e.buf[i];
  if constexpr (STORE) {
    b = lerp_to(b, g, hp.to_buf);
    e.buf[i] = b;
  }
  const float u = hp.nesterov ? lerp_to(g, b, hp.to_u) : b;
  return bf16_to_f32(f32_to_bf16(u));
}

// Pass M1: buf = lerp(buf, g, 1 - momentum) and each 1024-element chunk's sum of bf16(u)^2: four
// fp32 terms per lane, doubles above, one slot per chunk (no atomics)
template <typename GT>
__global__ __launch_bounds__(kThreads) void muon_m1_kernel(const MuEntry* __restrict__ entries,
                                                           int64_t n, int64_t chunks, const MuHP hp,
                                                           double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double wave_part[kWaves];
  const MuEntry e = entries[blockIdx.z];
  float part = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = int64_t(blockIdx.x) * kChunk + j * kThreads + threadIdx.x;
    if (i < n) {
      const float x = update_of<GT, true>(e, i, hp);
      part = fmaf(x, x, part);
    }
  }
  const double b = block_sum(double(part), wave_part);
  if (threadIdx.x == 0) partials[int64_t(blockIdx.z) * chunks + blockIdx.x] = b;
}

// After M1: workgroup z sums matrix z's chunk slots (thread t takes slots t, t + 256, ...; then the
// block tree) and stores bf16(max(sqrt(sum), eps)) widened to fp32
__global__ __launch_bounds__(kThreads) void muon_norm_kernel(const double* __restrict__ partials,
                                                             int64_t chunks, const MuHP hp,
                                                             float* __restrict__ nrm) {
  __shared__ double wave_part[kWaves];
  const double* p = partials + int64_t(blockIdx.x) * chunks;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < chunks; i += kThreads) s += p[i];
  s = block_sum(s, wave_part);
  if (threadIdx.x == 0) {
    const double nv = sqrt(s);
    const double m = nv > double(hp.eps) ? nv : (nv != nv ? nv : double(hp.eps));
    nrm[blockIdx.x] = bf16_to_f32(f32_to_bf16(float(m)));
  }
}

// Pass M2: x = bf16(bf16(u) / norm) of a 64 x 64 tile, written in the parameter's orientation
// (`nat`, R x C) and, through LDS, transposed (`tra`, C x R); both rows are 16-byte multiples
template <typename GT>
__global__ __launch_bounds__(kThreads) void muon_m2_kernel(
    const MuEntry* __restrict__ entries, int R, int C, const MuHP hp, const float* __restrict__ nrm,
    bf16_t* __restrict__ nat, int64_t ld_nat, int64_t s_nat, bf16_t* __restrict__ tra,
    int64_t ld_tra, int64_t s_tra) {
#pragma clang fp contract(off)
  __shared__ bf16_t tile[kTr][kTr + 1];
  const MuEntry e = entries[blockIdx.z];
  const float nv = nrm[blockIdx.z];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int r0 = blockIdx.y * kTr, c0 = blockIdx.x * kTr;
  bf16_t* on = nat + int64_t(blockIdx.z) * s_nat;
  bf16_t* ot = tra + int64_t(blockIdx.z) * s_tra;
  for (int k = 0; k < kTr / kWaves; ++k) {
    const int row = r0 + ty + kWaves * k, col = c0 + tx;
    bf16_t x = 0;
    if (row < R && col < C) {
      x = f32_to_bf16(update_of<GT, false>(e, int64_t(row) * C + col, hp) / nv);
      on[int64_t(row) * ld_nat + col] = x;
    }
    tile[ty + kWaves * k][tx] = x;
  }
  __syncthreads();
  for (int k = 0; k < kTr / kWaves; ++k) {
    const int col = c0 + ty + kWaves * k, row = r0 + tx;  // the transposed matrix's row is `col`
    if (row < R && col < C) ot[int64_t(col) * ld_tra + row] = tile[tx][ty + kWaves * k];
  }
}

// Pass P: p = fma(-adjusted_lr, O, p * (1 - lr * weight_decay)), O in the parameter's orientation
template <bool SPLIT>
__global__ __launch_bounds__(kThreads) void muon_apply_kernel(
    const MuEntry* __restrict__ entries, int64_t n, int C, const bf16_t* __restrict__ o,
    int64_t ld_o, int64_t s_o, float neg_alr, float decay_mul) {
#pragma clang fp contract(off)
  const MuEntry e = entries[blockIdx.z];
  const bf16_t* om = o + int64_t(blockIdx.z) * s_o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = int64_t(blockIdx.x) * kChunk + j * kThreads + threadIdx.x;
    if (i < n) {
      const int64_t row = i / C, col = i - row * C;
      const float u = bf16_to_f32(om[row * ld_o + col]);
      store_p1<SPLIT>(e, i, fmaf(neg_alr, u, load_p1<SPLIT>(e, i) * decay_mul));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// NorMuon (zero_amd.optim.NorMuon): after the last product O stands in the scratch in the
// parameter's orientation, rows 16-byte multiples.  N1 takes each row's sum of squares, N2 the row
// second moment, the matrix's scale and a step per row, N3 applies it.  N1 and N3 are row-tiled: a
// workgroup owns a strip of kStripRows rows, wave w of it rows w, w + 4, ...; a lane moves the
// 16-byte pieces at columns lane * 8 + 512 k, kRowLoads of them in flight.  A row's step is
// wave-uniform, so no element pays a division or an index split.
constexpr int kStripRows = 8;              // rows of a workgroup's strip (two per wave)
constexpr int kRowLoads = 4;               // 16-byte pieces a lane holds in flight
constexpr int kRowSeg = 512 * kRowLoads;   // columns of a row one pass of a wave covers

struct NorHP {
  Lerp to_v;          // v = lerp(v, mean(O^2), 1 - beta2)
  float norm_eps;
  double neg_scale;   // -(0.2 lr sqrt(R C)), per batch
};

// the widened halves of a word of two bf16
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }

// the sum of the squares of the first `valid` of a piece's eight bf16: one fp32 chain (the squares
// themselves are exact); what lies past `valid` is a row's padding and may hold anything
__device__ __forceinline__ float sumsq8(const uint4 v, int valid) {
#pragma clang fp contract(off)
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = (j & 1) ? bf16_hi(w[j >> 1]) : bf16_lo(w[j >> 1]);
    s = fmaf(j < valid ? x : 0.0f, j < valid ? x : 0.0f, s);
  }
  return s;
}

// Pass N1: rowsq[matrix][i] = sum_j O_ij^2, the pieces of a lane in fp32 (sumsq8), everything above
// in double: the lane along the row, then one shuffle tree per row.  Read-only over O; no LDS
__global__ __launch_bounds__(kThreads) void normuon_rowsq_kernel(const bf16_t* __restrict__ o,
                                                                 int R, int C, int64_t ld_o,
                                                                 int64_t s_o,
                                                                 double* __restrict__ rowsq) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const bf16_t* om = o + int64_t(blockIdx.z) * s_o;
#pragma unroll 1
  for (int k = 0; k < kStripRows / kWaves; ++k) {
    const int row = blockIdx.x * kStripRows + wave + kWaves * k;
    if (row >= R) break;
    const bf16_t* orow = om + int64_t(row) * ld_o;
    double acc = 0.0;
    for (int c0 = lane * 8; c0 < C; c0 += kRowSeg) {
      uint4 v[kRowLoads];
#pragma unroll
      for (int u = 0; u < kRowLoads; ++u) {  // (a piece that starts inside the row ends inside ld_o)
        const int c = c0 + 512 * u;
        v[u] = c < C ? *reinterpret_cast<const uint4*>(orow + c) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < kRowLoads; ++u) acc += double(sumsq8(v[u], C - (c0 + 512 * u)));
    }
    acc = wave_sum(acc);
    if (lane == 0) rowsq[int64_t(blockIdx.z) * R + row] = acc;
  }
}

// Pass N2, one workgroup per matrix: v_i = lerp(v_i, fp32(rowsq_i / C), 1 - beta2), stored;
// q_i = sqrt(v_i) + norm_eps; F^2 = sum_i rowsq_i / q_i^2 in double (the squared norm of the
// row-normalised O, from the row sums alone); rowstep_i = fp32(neg_scale / (sqrt(F^2) q_i)), +0.0 for
// every row when F^2 == 0 (a NaN is not 0: it propagates)
__global__ __launch_bounds__(kThreads) void normuon_finish_kernel(
    const double* __restrict__ rowsq, float* const* __restrict__ rowv, int R, int C, const NorHP nh,
    float* __restrict__ rowstep) {
#pragma clang fp contract(off)
  __shared__ double wave_part[kWaves];
  const double* rs = rowsq + int64_t(blockIdx.x) * R;
  float* v = rowv[blockIdx.x];
  float* out = rowstep + int64_t(blockIdx.x) * R;
  double f2 = 0.0;
  for (int i = threadIdx.x; i < R; i += kThreads) {
    const double s = rs[i];
    const float vi = lerp_to(v[i], float(s / double(C)), nh.to_v);
    v[i] = vi;
    const double q = double(sqrtf(vi) + nh.norm_eps);
    f2 += s / (q * q);
  }
  f2 = block_sum(f2, wave_part);
  const double f = sqrt(f2);
  for (int i = threadIdx.x; i < R; i += kThreads) {  // (v[i]: this thread's own store)
    const double q = double(sqrtf(v[i]) + nh.norm_eps);
    out[i] = f2 == 0.0 ? 0.0f : float(nh.neg_scale / (f * q));
  }
}

// eight updated masters to element i.. through store_p1's encodings, as 16-byte stores
template <bool SPLIT>
__device__ __forceinline__ void store_p8(const MuEntry& e, int64_t i, const float (&p)[8]) {
  uint32_t hi[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) hi[j] = f32_to_bf16(p[j]);
  const uint4 h = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16),
                             hi[6] | (hi[7] << 16));
  if constexpr (SPLIT) {
    uint32_t lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) lo[j] = master_residual(p[j], hi[j]);
    *reinterpret_cast<uint4*>(e.p_out + i) = h;
    *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(e.master_out) + i) =
        make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16),
                   lo[6] | (lo[7] << 16));
  } else {
    float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(e.master_out) + i);
    dst[0] = make_float4(p[0], p[1], p[2], p[3]);
    dst[1] = make_float4(p[4], p[5], p[6], p[7]);
    if (e.p_out) *reinterpret_cast<uint4*>(e.p_out + i) = h;
  }
}

// Pass N3: p_ij = fma(rowstep_i, float(O_ij), p_ij * (1 - lr * weight_decay)).  grid x = the strip of
// rows, y = the segment of kRowSeg columns, z = the matrix.  A matrix whose rows are 16-byte
// multiples in every array (C a multiple of 8, the entry's pointers 16-byte aligned) moves 16 bytes
// of O with 2 x 16 of fp32 master (or 16 of bf16 parameter + 16 of residual); any other takes
// element accesses to the master, with the same arithmetic
template <bool SPLIT>
__global__ __launch_bounds__(kThreads) void normuon_apply_kernel(
    const MuEntry* __restrict__ entries, int R, int C, const bf16_t* __restrict__ o, int64_t ld_o,
    int64_t s_o, const float* __restrict__ rowstep, float decay_mul) {
#pragma clang fp contract(off)
  const MuEntry e = entries[blockIdx.z];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const bf16_t* om = o + int64_t(blockIdx.z) * s_o;
  const uint64_t ptrs = reinterpret_cast<uint64_t>(e.master) |
                        reinterpret_cast<uint64_t>(e.master_out) |
                        reinterpret_cast<uint64_t>(e.p_out);
  const bool vec = (C & 7) == 0 && (ptrs & 15) == 0;
  const int c0 = blockIdx.y * kRowSeg + lane * 8;
#pragma unroll 1
  for (int k = 0; k < kStripRows / kWaves; ++k) {
    const int row = blockIdx.x * kStripRows + wave + kWaves * k;
    if (row >= R) break;
    const float step = rowstep[int64_t(blockIdx.z) * R + row];
    const bf16_t* orow = om + int64_t(row) * ld_o;
    const int64_t base = int64_t(row) * C;
    uint4 ov[kRowLoads], ma[kRowLoads], mb[kRowLoads];
#pragma unroll
    for (int u = 0; u < kRowLoads; ++u) {
      const int c = c0 + 512 * u;
      if (c >= C) continue;
      ov[u] = *reinterpret_cast<const uint4*>(orow + c);  // (ends inside ld_o)
      if (!vec) continue;
      if constexpr (SPLIT) {
        ma[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(e.master) + base + c);
        mb[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(e.master_out) + base + c);
      } else {
        const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(e.master) + base + c);
        ma[u] = src[0], mb[u] = src[1];
      }
    }
#pragma unroll
    for (int u = 0; u < kRowLoads; ++u) {
      const int c = c0 + 512 * u;
      if (c >= C) continue;
      const uint32_t w[4] = {ov[u].x, ov[u].y, ov[u].z, ov[u].w};
      if (vec) {
        const uint32_t mw[8] = {ma[u].x, ma[u].y, ma[u].z, ma[u].w,
                                mb[u].x, mb[u].y, mb[u].z, mb[u].w};
        float p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int sh = 16 * (j & 1);
          float m;
          if constexpr (SPLIT)
            m = join_master((mw[j >> 1] >> sh) & 0xFFFFu, (mw[4 + (j >> 1)] >> sh) & 0xFFFFu);
          else m = __uint_as_float(mw[j]);
          const float x = (j & 1) ? bf16_hi(w[j >> 1]) : bf16_lo(w[j >> 1]);
          p[j] = fmaf(step, x, m * decay_mul);
        }
        store_p8<SPLIT>(e, base + c, p);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (c + j >= C) break;
          const float x = (j & 1) ? bf16_hi(w[j >> 1]) : bf16_lo(w[j >> 1]);
          store_p1<SPLIT>(e, base + c + j, fmaf(step, x, load_p1<SPLIT>(e, base + c + j) * decay_mul));
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The NT product
struct GemmArgs {
  const bf16_t* A;   // M x K
  const bf16_t* B;   // N x K
  const bf16_t* E;   // M x N, or null (beta unused)
  bf16_t* D;         // M x N
  bf16_t* D2;        // N x M: the transposed store, or null; (sym) D itself
  int64_t lda, ldb, lde, ldd, ldd2;  // row strides in elements
  int64_t sA, sB, sE, sD, sD2;       // strides from one matrix of the batch to the next
  int M, N, K;
  float alpha, beta;
  int sym;                  // M == N, D symmetric: tiles with tile_n >= tile_m only, mirrored
  int vecA, vecB, vecD, vecD2;  // every row start 16-byte aligned
};

// eight K-consecutive elements of row `row` from column k; zeros outside the matrix
__device__ __forceinline__ uint4 load_chunk(const bf16_t* base, int64_t ld, int row, int nrows,
                                            int k, int K, int vec) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (row >= nrows || k >= K) return v;
  const bf16_t* p = base + int64_t(row) * ld + k;
  if (vec && k + 8 <= K) return *reinterpret_cast<const uint4*>(p);
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = k + j < K ? uint32_t(p[j]) : 0u;
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                    h[6] | (h[7] << 16));
}

// byte offset of 16-byte chunk `c` of row `row` inside a stage's 128 x 128-byte operand block
__device__ __forceinline__ int lds_off(int row, int c) { return row * (kBK * 2) + ((c ^ (row & 7)) << 4); }

// the staged 128 x 128 output tile to rows row0.. and columns col0.. of dst, 16-byte pieces
__device__ __forceinline__ void flush_tile(const unsigned char* smem, bf16_t* dst, int64_t ld,
                                           int row0, int nrows, int col0, int ncols, int vec) {
#pragma unroll
  for (int i = 0; i < kTile * (kTile / 8) / kThreads; ++i) {
    const int idx = threadIdx.x + kThreads * i;
    const int row = idx >> 4, ch = idx & 15;
    const int gr = row0 + row, gc = col0 + ch * 8;
    if (gr >= nrows || gc >= ncols) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(smem + (row * kOutStride + ch * 8) * 2);
    bf16_t* p = dst + int64_t(gr) * ld + gc;
    if (vec && gc + 8 <= ncols) {
      *reinterpret_cast<uint4*>(p) = v;
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (gc + j < ncols) p[j] = bf16_t(w[j >> 1] >> (16 * (j & 1)));
    }
  }
}

// kernel-resource-usage (gfx950): see DESIGN.md §4 "Fused Muon"
__global__ __launch_bounds__(kThreads) void muon_gemm_nt_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kStageBytes];
  const int tile_m = blockIdx.y, tile_n = blockIdx.x;
  if (a.sym && tile_n < tile_m) return;
  const int m0 = tile_m * kTile, n0 = tile_n * kTile;
  const int64_t z = blockIdx.z;
  const bf16_t* A = a.A + z * a.sA;
  const bf16_t* B = a.B + z * a.sB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // the loader: thread t moves chunk t & 7 of rows (t >> 3) + 32 i of both operand blocks
  const int lc = tid & 7, lr = tid >> 3;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  uint4 ra[4], rb[4];
  const int nk = (a.K + kBK - 1) / kBK;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = load_chunk(A, a.lda, m0 + lr + 32 * i, a.M, lc * 8, a.K, a.vecA);
    rb[i] = load_chunk(B, a.ldb, n0 + lr + 32 * i, a.N, lc * 8, a.K, a.vecB);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<uint4*>(smem + lds_off(lr + 32 * i, lc)) = ra[i];
    *reinterpret_cast<uint4*>(smem + kTile * kBK * 2 + lds_off(lr + 32 * i, lc)) = rb[i];
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned char* sa = smem + (kt & 1) * kStageBytes;
    const unsigned char* sb = sa + kTile * kBK * 2;
    const bool more = kt + 1 < nk;
    if (more) {
      const int k = (kt + 1) * kBK + lc * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = load_chunk(A, a.lda, m0 + lr + 32 * i, a.M, k, a.K, a.vecA);
        rb[i] = load_chunk(B, a.ldb, n0 + lr + 32 * i, a.N, k, a.K, a.vecB);
      }
    }
#pragma unroll
    for (int kk = 0; kk < kBK / 16; ++kk) {
      const int c = kk * 2 + (lane >> 5);  // lanes 0-31 hold k 0..7 of the step, lanes 32-63 k 8..15
      bf16x8 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint4 ua = *reinterpret_cast<const uint4*>(sa + lds_off(wm * 64 + i * 32 + (lane & 31), c));
        const uint4 ub = *reinterpret_cast<const uint4*>(sb + lds_off(wn * 64 + i * 32 + (lane & 31), c));
        av[i] = __builtin_bit_cast(bf16x8, ua);
        bv[i] = __builtin_bit_cast(bf16x8, ub);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      unsigned char* na = smem + ((kt + 1) & 1) * kStageBytes;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<uint4*>(na + lds_off(lr + 32 * i, lc)) = ra[i];
        *reinterpret_cast<uint4*>(na + kTile * kBK * 2 + lds_off(lr + 32 * i, lc)) = rb[i];
      }
    }
    __syncthreads();
  }
  // Epilogue.  Accumulator r of MFMA (i, j) is the element at row wm*64 + i*32 + 8 (r / 4) +
  // 4 (lane / 32) + r % 4, column wn*64 + j*32 + lane % 32 of the tile.
  const bf16_t* E = a.E ? a.E + z * a.sE : nullptr;
  bf16_t* ts = reinterpret_cast<bf16_t*>(smem);
  const bool diag = a.sym && tile_m == tile_n;
  uint32_t out[2][2][8];  // the tile's bf16 values, two per word (rows r, r + 1)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
        const int ml = wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        float v = a.alpha * acc[i][j][r];
        if (E && m0 + ml < a.M && n0 + nl < a.N)
          v = fmaf(a.beta, bf16_to_f32(E[int64_t(m0 + ml) * a.lde + n0 + nl]), v);
        const uint32_t h = f32_to_bf16(v);
        if (r & 1) out[i][j][r >> 1] |= h << 16;
        else out[i][j][r >> 1] = h;
        // a diagonal tile of a symmetric product keeps its upper triangle and mirrors it
        if (!diag || nl >= ml) ts[ml * kOutStride + nl] = bf16_t(h);
        if (diag && nl > ml) ts[nl * kOutStride + ml] = bf16_t(h);
      }
    }
  __syncthreads();
  flush_tile(smem, a.D + z * a.sD, a.ldd, m0, a.M, n0, a.N, a.vecD);
  if (!a.D2 || diag) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // rows ml .. ml + 3 are four consecutive columns of row nl
        const int ml = wm * 64 + i * 32 + 8 * q + 4 * (lane >> 5);
        *reinterpret_cast<uint2*>(ts + nl * kOutStride + ml) =
            make_uint2(out[i][j][2 * q], out[i][j][2 * q + 1]);
      }
    }
  __syncthreads();
  flush_tile(smem, a.D2 + z * a.sD2, a.ldd2, n0, a.N, m0, a.M, a.vecD2);
}

bool aligned(uint64_t p, uint64_t a) { return (p & (a - 1)) == 0; }
int64_t round8(int64_t x) { return (x + 7) / 8 * 8; }

int launch_gemm(GemmArgs g, int64_t batch, hipStream_t st) {
  const auto vec = [](const void* p, int64_t ld, int64_t s) {
    return int(aligned(reinterpret_cast<uint64_t>(p), 16) && ld % 8 == 0 && s % 8 == 0);
  };
  if (g.sym) g.D2 = g.D, g.ldd2 = g.ldd, g.sD2 = g.sD;
  g.vecA = vec(g.A, g.lda, g.sA), g.vecB = vec(g.B, g.ldb, g.sB);
  g.vecD = vec(g.D, g.ldd, g.sD), g.vecD2 = g.D2 ? vec(g.D2, g.ldd2, g.sD2) : 0;
  const dim3 grid(unsigned((g.N + kTile - 1) / kTile), unsigned((g.M + kTile - 1) / kTile),
                  unsigned(batch));
  muon_gemm_nt_kernel<<<grid, dim3(kThreads), 0, st>>>(g);
  return ZS_OK;
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

struct Batch {
  int64_t e0, count;  // entries [e0, e0 + count) of the shape-grouped table
  int R, C;
};

// where a batch's arrays lie in the set's scratch
struct Layout {
  int r, c;            // min and max of (R, C)
  int64_t ldr, ldc;    // row strides of the r- and c-column arrays (16-byte multiples)
  int64_t chunks;      // M1's slots per matrix
  double* partials;
  float* nrm;
  bf16_t *X, *XT[2], *A, *Bm;
};

}  // namespace

struct zs_muonset {
  unsigned tag = zs::kMuonSetTag;
  MuEntry* d_entries = nullptr;
  unsigned char* d_scratch = nullptr;
  std::vector<Batch> batches;
  std::vector<int> cur;  // per batch: which XT holds the current transpose (run_pass's products)
  // NorMuon's row state (zs_muonset_attach_rows): the entries' row vectors in the shape-grouped
  // order, and the row scratch: row_slots doubles (rowsq), then row_slots floats (rowstep)
  std::vector<int64_t> order;  // the caller's index of each shape-grouped entry
  float** d_rowv = nullptr;
  unsigned char* d_rows = nullptr;
  int64_t row_slots = 0, row_bytes = 0;
  bool has_rows = false;
  int64_t partial_slots = 0, nrm_slots = 0, bf16_elems = 0;
  int64_t nent = 0, elems = 0, bytes = 0, pass_bytes[3] = {0, 0, 0}, scratch_bytes = 0;
  int64_t flops_iter = 0, flops_iter_run = 0;
  int g_dtype = ZS_F32, p_dtype = ZS_BF16;
};

static Layout layout_of(const zs_muonset* s, const Batch& b) {
  Layout l{};
  l.r = std::min(b.R, b.C), l.c = std::max(b.R, b.C);
  l.ldr = round8(l.r), l.ldc = round8(l.c);
  l.chunks = (int64_t(b.R) * b.C + kChunk - 1) / kChunk;
  l.partials = reinterpret_cast<double*>(s->d_scratch);
  l.nrm = reinterpret_cast<float*>(l.partials + s->partial_slots);
  bf16_t* h = reinterpret_cast<bf16_t*>(l.nrm + s->nrm_slots);
  l.X = h, h += b.count * l.r * l.ldc;
  l.XT[0] = h, h += b.count * l.c * l.ldr;
  l.XT[1] = h, h += b.count * l.c * l.ldr;
  l.A = h, h += b.count * l.r * l.ldr;
  l.Bm = h;
  return l;
}

static int64_t matrix_scratch_elems(int64_t R, int64_t C) {
  const int64_t r = std::min(R, C), c = std::max(R, C);
  return r * round8(c) + 2 * c * round8(r) + 2 * r * round8(r);
}

static Lerp make_lerp(double weight);

// the passes of one batch; mask: 1 = M1 and the norm, 2 = M2, 4 = the iteration, 8 = P;
// product >= 0 with mask 4: that one product of one iteration
// NorMuon (nh != NULL): 16 = N1, 32 = N2, 64 = N3
template <typename GT, bool SPLIT>
static int run_batch(zs_muonset* s, size_t bi, const zs_muon_hparams* h, const MuHP& hp, int mask,
                     int product, hipStream_t st, const zs_normuon_hparams* nh = nullptr) {
  const Batch& b = s->batches[bi];
  const Layout l = layout_of(s, b);
  const MuEntry* ent = s->d_entries + b.e0;
  const int64_t n = int64_t(b.R) * b.C;
  const unsigned nb = unsigned(b.count);
  const dim3 block(kThreads), sgrid(unsigned(l.chunks), 1, nb);
  const bool tall = b.R > b.C;  // X is the transpose of the parameter's orientation
  if (mask & 1) {
    muon_m1_kernel<GT><<<sgrid, block, 0, st>>>(ent, n, l.chunks, hp, l.partials);
    muon_norm_kernel<<<dim3(nb), block, 0, st>>>(l.partials, l.chunks, hp, l.nrm);
  }
  if (mask & 2) {
    const dim3 g2(unsigned((b.C + kTr - 1) / kTr), unsigned((b.R + kTr - 1) / kTr), nb);
    bf16_t *nat = tall ? l.XT[0] : l.X, *tra = tall ? l.X : l.XT[0];
    const int64_t ldn = tall ? l.ldr : l.ldc, ldt = tall ? l.ldc : l.ldr;
    muon_m2_kernel<GT><<<g2, block, 0, st>>>(ent, b.R, b.C, hp, l.nrm, nat, ldn, int64_t(b.R) * ldn,
                                             tra, ldt, int64_t(b.C) * ldt);
    s->cur[bi] = 0;
  }
  if (mask & 4) {
    const int steps = product >= 0 ? 1 : h->ns_steps;
    for (int it = 0; it < steps; ++it) {
      const int cur = s->cur[bi];
      GemmArgs g{};
      if (product < 0 || product == 0) {  // A = X X^T
        g = GemmArgs{};
        g.A = l.X, g.B = l.X, g.D = l.A;
        g.lda = g.ldb = l.ldc, g.ldd = l.ldr;
        g.sA = g.sB = int64_t(l.r) * l.ldc, g.sD = int64_t(l.r) * l.ldr;
        g.M = g.N = l.r, g.K = l.c, g.alpha = 1.0f, g.beta = 0.0f, g.sym = 1;
        launch_gemm(g, nb, st);
      }
      if (product < 0 || product == 1) {  // Bm = b A + c A A^T
        g = GemmArgs{};
        g.A = l.A, g.B = l.A, g.E = l.A, g.D = l.Bm;
        g.lda = g.ldb = g.lde = g.ldd = l.ldr;
        g.sA = g.sB = g.sE = g.sD = int64_t(l.r) * l.ldr;
        g.M = g.N = g.K = l.r, g.alpha = float(h->ns_c), g.beta = float(h->ns_b), g.sym = 1;
        launch_gemm(g, nb, st);
      }
      if (product < 0 || product == 2) {  // X' = a X + Bm (XT)^T, and XT' = X'^T beside XT
        g = GemmArgs{};
        g.A = l.Bm, g.B = l.XT[cur], g.E = l.X, g.D = l.X, g.D2 = l.XT[cur ^ 1];
        g.lda = l.ldr, g.ldb = l.ldr, g.lde = g.ldd = l.ldc, g.ldd2 = l.ldr;
        g.sA = int64_t(l.r) * l.ldr, g.sB = g.sD2 = int64_t(l.c) * l.ldr;
        g.sE = g.sD = int64_t(l.r) * l.ldc;
        g.M = l.r, g.N = l.c, g.K = l.r, g.alpha = 1.0f, g.beta = float(h->ns_a);
        launch_gemm(g, nb, st);
        s->cur[bi] = cur ^ 1;
      }
    }
  }
  if (mask & 8) {
    // torch's _adjust_lr, in double, rounded to fp32 once
    const double A = double(b.R), B = double(b.C);
    const double ratio = h->adjust_lr == 1 ? 0.2 * std::sqrt(std::max(A, B))
                                           : std::sqrt(std::max(1.0, A / B));
    const float neg_alr = float(-(h->lr * ratio));
    const float decay_mul = float(1.0 - h->lr * h->weight_decay);
    const bf16_t* o = tall ? l.XT[s->cur[bi]] : l.X;
    const int64_t ldo = tall ? l.ldr : l.ldc;
    muon_apply_kernel<SPLIT><<<sgrid, block, 0, st>>>(ent, n, b.C, o, ldo, int64_t(b.R) * ldo,
                                                      neg_alr, decay_mul);
  }
  if (mask & 112) {
    const bf16_t* o = tall ? l.XT[s->cur[bi]] : l.X;
    const int64_t ldo = tall ? l.ldr : l.ldc;
    double* rowsq = reinterpret_cast<double*>(s->d_rows);
    float* rowstep = reinterpret_cast<float*>(rowsq + s->row_slots);
    const unsigned strips = unsigned((b.R + kStripRows - 1) / kStripRows);
    if (mask & 16)
      normuon_rowsq_kernel<<<dim3(strips, 1, nb), block, 0, st>>>(o, b.R, b.C, ldo,
                                                                  int64_t(b.R) * ldo, rowsq);
    if (mask & 32) {
      NorHP q;
      q.to_v = make_lerp(1.0 - nh->beta2);
      q.norm_eps = float(nh->norm_eps);
      q.neg_scale = -(0.2 * h->lr * std::sqrt(double(b.R) * double(b.C)));
      normuon_finish_kernel<<<dim3(nb), block, 0, st>>>(rowsq, s->d_rowv + b.e0, b.R, b.C, q,
                                                        rowstep);
    }
    if (mask & 64) {
      const float decay_mul = float(1.0 - h->lr * h->weight_decay);
      const dim3 g3(strips, unsigned((b.C + kRowSeg - 1) / kRowSeg), nb);
      normuon_apply_kernel<SPLIT><<<g3, block, 0, st>>>(ent, b.R, b.C, o, ldo, int64_t(b.R) * ldo,
                                                        rowstep, decay_mul);
    }
  }
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

static int check_hparams(const char* fn, const zs_muon_hparams* h) {
  ZS_REQUIRE(h->lr >= 0.0 && std::isfinite(h->lr), "%s: learning rate should be >= 0", fn);
  ZS_REQUIRE(h->momentum >= 0.0 && std::isfinite(h->momentum), "%s: momentum should be >= 0", fn);
  ZS_REQUIRE(h->weight_decay >= 0.0, "%s: weight decay should be >= 0", fn);
  ZS_REQUIRE(h->ns_steps >= 0 && h->ns_steps < 100,
             "%s: the number of Newton-Schulz steps must be in [0, 100) (got %d)", fn, h->ns_steps);
  ZS_REQUIRE(h->adjust_lr == 0 || h->adjust_lr == 1,
             "%s: adjust_lr is 0 (original) or 1 (match_rms_adamw)", fn);
  ZS_REQUIRE(h->eps >= 0.0, "%s: eps should be >= 0", fn);
  ZS_REQUIRE(h->grad_div > 0.0, "%s: grad_div must be > 0", fn);
  return ZS_OK;
}

static Lerp make_lerp(double weight) {
  const float w = float(weight);
  Lerp l;
  l.hi = std::fabs(w) < 0.5f ? 0 : 1;
  l.w = l.hi ? w - 1.0f : w;
  return l;
}

static int check_normuon(const char* fn, const zs_normuon_hparams* nh) {
  if (int rc = check_hparams(fn, &nh->muon)) return rc;
  ZS_REQUIRE(nh->beta2 >= 0.0 && nh->beta2 < 1.0, "%s: beta2 must be in [0, 1)", fn);
  ZS_REQUIRE(nh->norm_eps >= 0.0, "%s: norm_eps should be >= 0", fn);
  return ZS_OK;
}

static int run_checked(const char* fn, zs_muonset* s, const zs_muon_hparams* h, int mask,
                       int product, int64_t batch, uintptr_t stream,
                       const zs_normuon_hparams* nh = nullptr) {
  ZS_REQUIRE(s && h, "%s: NULL argument", fn);
  ZS_REQUIRE(s->tag == zs::kMuonSetTag, "%s: the set was not made by zs_muonset_create", fn);
  if (int rc = nh ? check_normuon(fn, nh) : check_hparams(fn, h)) return rc;
  ZS_REQUIRE(!nh || s->has_rows, "%s: the set has no row state (zs_muonset_attach_rows)", fn);
  ZS_REQUIRE(batch >= -1 && batch < int64_t(s->batches.size()), "%s: batch %lld of %lld", fn,
             (long long)batch, (long long)s->batches.size());
  if (s->nent == 0) return ZS_OK;
  MuHP hp;
  hp.to_buf = make_lerp(1.0 - h->momentum);
  hp.to_u = make_lerp(h->momentum);
  hp.eps = float(h->eps);
  hp.nesterov = h->nesterov ? 1 : 0;
  int exp2 = 0;
  hp.grad_div = float(h->grad_div);
  hp.div_pow2 = std::frexp(double(hp.grad_div), &exp2) == 0.5 ? 1 : 0;
  hp.inv_div = float(1.0 / double(hp.grad_div));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool g32 = s->g_dtype == ZS_F32, split = s->p_dtype == ZS_BF16_SPLIT;
  for (size_t bi = 0; bi < s->batches.size(); ++bi) {
    if (batch >= 0 && int64_t(bi) != batch) continue;
    int rc;
    if (g32)
      rc = split ? run_batch<float, true>(s, bi, h, hp, mask, product, st, nh)
                 : run_batch<float, false>(s, bi, h, hp, mask, product, st, nh);
    else
      rc = split ? run_batch<unsigned short, true>(s, bi, h, hp, mask, product, st, nh)
                 : run_batch<unsigned short, false>(s, bi, h, hp, mask, product, st, nh);
    if (rc != ZS_OK) return rc;
  }
  return ZS_OK;
}

extern "C" {

int zs_muon_hparams_init(double lr, double weight_decay, double momentum, int nesterov, double ns_a,
                         double ns_b, double ns_c, double eps, int ns_steps, int adjust_lr,
                         double grad_div, zs_muon_hparams* hp) {
  const char* fn = "zs_muon_hparams_init";
  ZS_REQUIRE(hp != nullptr, "%s: hp is NULL", fn);
  zs_muon_hparams h{};
  h.lr = lr, h.weight_decay = weight_decay, h.momentum = momentum;
  h.ns_a = ns_a, h.ns_b = ns_b, h.ns_c = ns_c, h.eps = eps, h.grad_div = grad_div;
  h.nesterov = nesterov ? 1 : 0, h.ns_steps = ns_steps, h.adjust_lr = adjust_lr, h.reserved = 0;
  if (int rc = check_hparams(fn, &h)) return rc;
  *hp = h;
  return ZS_OK;
}

int zs_muonset_create(const zs_muon_seg* in, int64_t n, int g_dtype, int p_dtype,
                      int64_t scratch_budget, zs_muonset** out) {
  const char* fn = "zs_muonset_create";
  ZS_REQUIRE(out != nullptr, "%s: out is NULL", fn);
  *out = nullptr;
  ZS_REQUIRE(n >= 0 && (n == 0 || in), "%s: bad table", fn);
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "%s: bad g_dtype %d", fn, g_dtype);
  ZS_REQUIRE(p_dtype == ZS_BF16 || p_dtype == ZS_BF16_SPLIT,
             "%s: p_dtype must be ZS_BF16 or ZS_BF16_SPLIT (got %d)", fn, p_dtype);
  ZS_REQUIRE(scratch_budget >= 0, "%s: scratch_budget < 0", fn);
  const int64_t budget = scratch_budget ? scratch_budget : kDefaultBudget;
  const bool split = p_dtype == ZS_BF16_SPLIT;
  const uint64_t gsz = g_dtype == ZS_F32 ? 4 : 2, msz = split ? 2 : 4;
  for (int64_t i = 0; i < n; ++i) {
    const zs_muon_seg& s = in[i];
    ZS_REQUIRE(s.R >= 1 && s.C >= 1, "%s: entry %lld: R and C must be >= 1", fn, (long long)i);
    ZS_REQUIRE(s.R < (int64_t(1) << 24) && s.C < (int64_t(1) << 24) &&
                   matrix_scratch_elems(s.R, s.C) < (int64_t(1) << 38),
               "%s: entry %lld: R or C too large", fn, (long long)i);
    ZS_REQUIRE(s.g && s.master && s.master_out && s.buf,
               "%s: entry %lld missing g/master/master_out/buf", fn, (long long)i);
    ZS_REQUIRE(!split || s.p_out, "%s: entry %lld: a split master needs p_out", fn, (long long)i);
    ZS_REQUIRE(split || s.master_out == s.master,
               "%s: entry %lld: the fp32 master is updated in place (master_out == master)", fn,
               (long long)i);
    ZS_REQUIRE(aligned(s.g, gsz) && aligned(s.master, msz) && aligned(s.master_out, msz) &&
                   aligned(s.p_out, 2) && aligned(s.buf, 4),
               "%s: entry %lld: a pointer is not aligned to its element", fn, (long long)i);
    ZS_REQUIRE(s.param >= 0, "%s: entry %lld: param < 0", fn, (long long)i);
    ZS_REQUIRE(matrix_scratch_elems(s.R, s.C) * 2 <= budget,
               "%s: entry %lld (%lld x %lld) needs %lld scratch bytes, the budget is %lld", fn,
               (long long)i, (long long)s.R, (long long)s.C,
               (long long)(matrix_scratch_elems(s.R, s.C) * 2), (long long)budget);
  }
  zs_muonset* ms = new (std::nothrow) zs_muonset();
  if (!ms) return zs::fail(ZS_ERR_NOMEM, "%s: out of memory", fn);
  ms->g_dtype = g_dtype, ms->p_dtype = p_dtype, ms->nent = n;
  *out = ms;
  if (n == 0) return ZS_OK;
  // group the entries by shape, in the order a shape first appears; cut each group into batches
  std::vector<int64_t> order;
  std::vector<char> taken(size_t(n), 0);
  std::vector<MuEntry> ent;
  for (int64_t i = 0; i < n; ++i) {
    if (taken[size_t(i)]) continue;
    const int64_t R = in[i].R, C = in[i].C;
    const int64_t first = int64_t(ent.size());
    for (int64_t k = i; k < n; ++k) {
      if (taken[size_t(k)] || in[k].R != R || in[k].C != C) continue;
      taken[size_t(k)] = 1;
      MuEntry e{};
      e.g = reinterpret_cast<const void*>(in[k].g);
      e.master = reinterpret_cast<const void*>(in[k].master);
      e.master_out = reinterpret_cast<void*>(in[k].master_out);
      e.p_out = reinterpret_cast<unsigned short*>(in[k].p_out);
      e.buf = reinterpret_cast<float*>(in[k].buf);
      ent.push_back(e);
      order.push_back(k);
    }
    const int64_t count = int64_t(ent.size()) - first;
    const int64_t per = matrix_scratch_elems(R, C);
    const int64_t nb = std::min(std::min(count, budget / (per * 2)), kMaxBatch);
    const int64_t r = std::min(R, C), c = std::max(R, C), ne = R * C;
    const int64_t t = (r + kTile - 1) / kTile, tc = (c + kTile - 1) / kTile;
    for (int64_t e0 = first; e0 < first + count; e0 += nb) {
      const int64_t cnt = std::min(nb, first + count - e0);
      ms->batches.push_back(Batch{e0, cnt, int(R), int(C)});
      ms->partial_slots = std::max(ms->partial_slots, cnt * ((ne + kChunk - 1) / kChunk));
      ms->nrm_slots = std::max(ms->nrm_slots, (cnt + 3) / 4 * 4);
      ms->bf16_elems = std::max(ms->bf16_elems, cnt * per);
      ms->row_slots = std::max(ms->row_slots, cnt * R);
    }
    ms->elems += count * ne;
    ms->pass_bytes[0] += count * ne * int64_t(gsz + 8);
    ms->pass_bytes[1] += count * ne * int64_t(gsz + 4 + 4);
    ms->pass_bytes[2] += count * ne * int64_t(2 + (split ? 8 : 8 + (in[i].p_out ? 2 : 0)));
    ms->flops_iter += count * (4 * r * r * c + 2 * r * r * r);
    // what the tiles compute: the upper triangle of tiles of both symmetric products
    const int64_t tri = t * (t + 1) / 2, T = kTile;
    ms->flops_iter_run += count * 2 * T * T * (tri * (tc * T) + tri * (t * T) + t * tc * (t * T));
  }
  ms->cur.assign(ms->batches.size(), 0);
  ms->order = order;
  ms->bytes = ms->pass_bytes[0] + ms->pass_bytes[1] + ms->pass_bytes[2];
  ms->scratch_bytes = ms->partial_slots * 8 + ms->nrm_slots * 4 + ms->bf16_elems * 2;
  int rc = ZS_OK;
  hipStream_t st = upload_stream();
  if (!st) rc = zs::fail(ZS_ERR_HIP, "%s: no upload stream", fn);
  hipError_t he = hipSuccess;
  if (rc == ZS_OK) {
    he = hipMalloc(reinterpret_cast<void**>(&ms->d_scratch), size_t(ms->scratch_bytes));
    if (he == hipSuccess)
      he = hipMalloc(reinterpret_cast<void**>(&ms->d_entries), ent.size() * sizeof(MuEntry));
    if (he == hipSuccess)
      he = hipMemcpyAsync(ms->d_entries, ent.data(), ent.size() * sizeof(MuEntry),
                          hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess)
      rc = zs::fail(ZS_ERR_HIP, "%s: allocation or upload failed (%lld scratch bytes): %s", fn,
                    (long long)ms->scratch_bytes, hipGetErrorString(he));
  }
  if (rc != ZS_OK) {
    zs_muonset_destroy(ms);
    *out = nullptr;
  }
  return rc;
}

int zs_muonset_run(zs_muonset* ms, const zs_muon_hparams* h, uintptr_t stream) {
  return run_checked("zs_muonset_run", ms, h, 15, -1, -1, stream);
}

int zs_muonset_run_pass(zs_muonset* ms, const zs_muon_hparams* h, int pass, int product,
                        int64_t batch, uintptr_t stream) {
  const char* fn = "zs_muonset_run_pass";
  ZS_REQUIRE(pass >= 0 && pass <= 3, "%s: pass must be 0 (M1), 1 (M2), 2 (products) or 3 (P)", fn);
  ZS_REQUIRE(product >= -1 && product <= 2, "%s: product must be -1 (all) or 0, 1, 2", fn);
  return run_checked(fn, ms, h, 1 << pass, pass == 2 ? product : -1, batch, stream);
}

int zs_muonset_stats(const zs_muonset* ms, int64_t* out, int n) {
  ZS_REQUIRE(ms && out && n >= 1, "zs_muonset_stats: NULL argument");
  ZS_REQUIRE(ms->tag == zs::kMuonSetTag, "zs_muonset_stats: the set was not made by "
             "zs_muonset_create");
  const int64_t v[9] = {ms->elems, ms->bytes, ms->pass_bytes[0], ms->pass_bytes[1],
                        ms->pass_bytes[2], ms->scratch_bytes, ms->flops_iter, ms->flops_iter_run,
                        int64_t(ms->batches.size())};
  for (int k = 0; k < n && k < 9; ++k) out[k] = v[k];
  return ZS_OK;
}

int zs_muonset_batch(const zs_muonset* ms, int64_t batch, int64_t* out) {
  ZS_REQUIRE(ms && out, "zs_muonset_batch: NULL argument");
  ZS_REQUIRE(ms->tag == zs::kMuonSetTag, "zs_muonset_batch: the set was not made by "
             "zs_muonset_create");
  ZS_REQUIRE(batch >= 0 && batch < int64_t(ms->batches.size()), "zs_muonset_batch: batch %lld of "
             "%lld", (long long)batch, (long long)ms->batches.size());
  const Batch& b = ms->batches[size_t(batch)];
  const Layout l = layout_of(ms, b);
  const int64_t v[12] = {b.e0, b.count, b.R, b.C, l.ldr, l.ldc,
                         int64_t(reinterpret_cast<uintptr_t>(l.X)),
                         int64_t(reinterpret_cast<uintptr_t>(l.XT[ms->cur[size_t(batch)]])),
                         int64_t(reinterpret_cast<uintptr_t>(l.A)),
                         int64_t(reinterpret_cast<uintptr_t>(l.Bm)),
                         int64_t(reinterpret_cast<uintptr_t>(l.nrm)), ms->scratch_bytes};
  for (int k = 0; k < 12; ++k) out[k] = v[k];
  return ZS_OK;
}

int zs_muonset_destroy(zs_muonset* ms) {
  if (!ms) return ZS_OK;
  ZS_REQUIRE(ms->tag == zs::kMuonSetTag, "zs_muonset_destroy: the set was not made by "
             "zs_muonset_create");
  if (ms->d_entries) (void)hipFree(ms->d_entries);
  if (ms->d_scratch) (void)hipFree(ms->d_scratch);
  if (ms->d_rowv) (void)hipFree(ms->d_rowv);
  if (ms->d_rows) (void)hipFree(ms->d_rows);
  delete ms;
  return ZS_OK;
}

int zs_normuon_hparams_init(double lr, double weight_decay, double momentum, int nesterov,
                            double ns_a, double ns_b, double ns_c, double eps, int ns_steps,
                            double beta2, double norm_eps, double grad_div, zs_normuon_hparams* hp) {
  const char* fn = "zs_normuon_hparams_init";
  ZS_REQUIRE(hp != nullptr, "%s: hp is NULL", fn);
  zs_normuon_hparams h{};
  h.muon.lr = lr, h.muon.weight_decay = weight_decay, h.muon.momentum = momentum;
  h.muon.ns_a = ns_a, h.muon.ns_b = ns_b, h.muon.ns_c = ns_c, h.muon.eps = eps;
  h.muon.grad_div = grad_div, h.muon.nesterov = nesterov ? 1 : 0, h.muon.ns_steps = ns_steps;
  h.beta2 = beta2, h.norm_eps = norm_eps;
  if (int rc = check_normuon(fn, &h)) return rc;
  *hp = h;
  return ZS_OK;
}

int zs_muonset_attach_rows(zs_muonset* ms, const uint64_t* row_v, int64_t n) {
  const char* fn = "zs_muonset_attach_rows";
  ZS_REQUIRE(ms != nullptr, "%s: NULL argument", fn);
  ZS_REQUIRE(ms->tag == zs::kMuonSetTag, "%s: the set was not made by zs_muonset_create", fn);
  ZS_REQUIRE(!ms->has_rows, "%s: the set already has row state", fn);
  ZS_REQUIRE(n == ms->nent && (n == 0 || row_v), "%s: %lld addresses for a table of %lld entries",
             fn, (long long)n, (long long)ms->nent);
  for (int64_t i = 0; i < n; ++i)
    ZS_REQUIRE(row_v[i] && aligned(row_v[i], 4), "%s: entry %lld: a NULL or misaligned address", fn,
               (long long)i);
  if (n == 0) {
    ms->has_rows = true;
    return ZS_OK;
  }
  std::vector<float*> rowv(static_cast<size_t>(n));
  for (int64_t k = 0; k < n; ++k)
    rowv[size_t(k)] = reinterpret_cast<float*>(row_v[ms->order[size_t(k)]]);
  hipStream_t st = upload_stream();
  if (!st) return zs::fail(ZS_ERR_HIP, "%s: no upload stream", fn);
  const int64_t row_bytes = ms->row_slots * 12;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&ms->d_rows), size_t(row_bytes));
  if (he == hipSuccess)
    he = hipMalloc(reinterpret_cast<void**>(&ms->d_rowv), rowv.size() * sizeof(float*));
  if (he == hipSuccess)
    he = hipMemcpyAsync(ms->d_rowv, rowv.data(), rowv.size() * sizeof(float*),
                        hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    if (ms->d_rows) (void)hipFree(ms->d_rows);
    if (ms->d_rowv) (void)hipFree(ms->d_rowv);
    ms->d_rows = nullptr, ms->d_rowv = nullptr;
    return zs::fail(ZS_ERR_HIP, "%s: allocation or upload failed (%lld row scratch bytes): %s", fn,
                    (long long)row_bytes, hipGetErrorString(he));
  }
  ms->row_bytes = row_bytes, ms->scratch_bytes += row_bytes;
  ms->has_rows = true;
  return ZS_OK;
}

int zs_muonset_run_normuon(zs_muonset* ms, const zs_normuon_hparams* h, uintptr_t stream) {
  return run_checked("zs_muonset_run_normuon", ms, h ? &h->muon : nullptr, 7 | 112, -1, -1, stream,
                     h);
}

int zs_muonset_run_normuon_pass(zs_muonset* ms, const zs_normuon_hparams* h, int pass, int product,
                                int64_t batch, uintptr_t stream) {
  const char* fn = "zs_muonset_run_normuon_pass";
  ZS_REQUIRE(pass >= 0 && pass <= 5,
             "%s: pass must be 0 (M1), 1 (M2), 2 (products), 3 (N1), 4 (N2) or 5 (N3)", fn);
  ZS_REQUIRE(product >= -1 && product <= 2, "%s: product must be -1 (all) or 0, 1, 2", fn);
  return run_checked(fn, ms, h ? &h->muon : nullptr, pass < 3 ? 1 << pass : 16 << (pass - 3),
                     pass == 2 ? product : -1, batch, stream, h);
}

int zs_muonset_rows(const zs_muonset* ms, int64_t batch, int64_t* out) {
  const char* fn = "zs_muonset_rows";
  ZS_REQUIRE(ms && out, "%s: NULL argument", fn);
  ZS_REQUIRE(ms->tag == zs::kMuonSetTag, "%s: the set was not made by zs_muonset_create", fn);
  ZS_REQUIRE(ms->has_rows, "%s: the set has no row state (zs_muonset_attach_rows)", fn);
  ZS_REQUIRE(batch >= 0 && batch < int64_t(ms->batches.size()), "%s: batch %lld of %lld", fn,
             (long long)batch, (long long)ms->batches.size());
  const double* rowsq = reinterpret_cast<const double*>(ms->d_rows);
  out[0] = int64_t(reinterpret_cast<uintptr_t>(rowsq));
  out[1] = int64_t(reinterpret_cast<uintptr_t>(rowsq + ms->row_slots));
  out[2] = ms->batches[size_t(batch)].R;
  out[3] = ms->row_bytes;
  return ZS_OK;
}

int zs_muon_gemm_nt(uint64_t A, int64_t lda, uint64_t B, int64_t ldb, uint64_t E, int64_t lde,
                    uint64_t D, int64_t ldd, uint64_t D2, int64_t ldd2, int64_t M, int64_t N,
                    int64_t K, double alpha, double beta, int sym, uintptr_t stream) {
  const char* fn = "zs_muon_gemm_nt";
  ZS_REQUIRE(A && B && D, "%s: NULL operand", fn);
  ZS_REQUIRE(aligned(A, 2) && aligned(B, 2) && aligned(E, 2) && aligned(D, 2) && aligned(D2, 2),
             "%s: a pointer is not aligned to bf16", fn);
  const int64_t lim = int64_t(1) << 24;
  ZS_REQUIRE(M >= 1 && N >= 1 && K >= 1 && M < lim && N < lim && K < lim, "%s: bad M, N or K", fn);
  ZS_REQUIRE(lda >= K && ldb >= K && ldd >= N && (!E || lde >= N) && (!D2 || ldd2 >= M),
             "%s: a row stride is shorter than its row", fn);
  ZS_REQUIRE(E || beta == 0.0, "%s: beta != 0 needs E", fn);
  ZS_REQUIRE(!sym || (M == N && !D2), "%s: the symmetric mode has M == N and mirrors into D itself "
             "(D2 must be 0)", fn);
  ZS_REQUIRE(D != A && D != B && D2 != A && D2 != B && D2 != D && (!D2 || D2 != E),
             "%s: an output aliases an operand (only D == E is allowed)", fn);
  GemmArgs g{};
  g.A = reinterpret_cast<const bf16_t*>(A), g.B = reinterpret_cast<const bf16_t*>(B);
  g.E = reinterpret_cast<const bf16_t*>(E);
  g.D = reinterpret_cast<bf16_t*>(D), g.D2 = reinterpret_cast<bf16_t*>(D2);
  g.lda = lda, g.ldb = ldb, g.lde = lde, g.ldd = ldd, g.ldd2 = ldd2;
  g.M = int(M), g.N = int(N), g.K = int(K);
  g.alpha = float(alpha), g.beta = float(beta), g.sym = sym ? 1 : 0;
  launch_gemm(g, 1, reinterpret_cast<hipStream_t>(stream));
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

}  // extern "C"
