// Fused Adam-mini (Zhang et al. 2024, arXiv:2406.16793; zero_amd.optim.AdamMini's rule) for CDNA4
// (gfx950): Adam's first moment per element, one second moment per block of the parameter.  A block
// is `block_rows` consecutive rows of an R x C parameter (or the whole of it), that is one
// contiguous run of L elements, so the kernels know runs, not rows.  The update needs the gradient
// twice -- the block's mean of g^2, then the step -- and there are two ways to get it:
//
// Resident path (L <= resident_cap).  One workgroup (256 threads, 4 waves) owns the block.  The
// block is cut into pieces of 16 bytes of gradient (V = 8 bf16 or 4 fp32 elements); thread t holds
// pieces t, t + 256, ... as raw uint4 registers (at most kResidentMax / (256 V) of them), all loads
// issued before the first use.  Sum of g^2: an fp32 fma chain over the V elements of a piece,
// doubles above it (the thread's pieces in order, a shuffle tree across the wave, the four waves
// through LDS in order).  Thread 0 updates v_b and forms a_b in double; LDS broadcasts a_b; the
// apply runs from the held registers: 16-byte loads of m and the master, 16-byte stores.  g is read
// exactly once.
//
// Two-pass path (larger blocks).  Pass 1: a workgroup takes a tile of kTilePieces * 256 pieces of a
// block and writes one double to the tile's own slot.  A finish kernel, one thread per block, adds
// the slots in order, updates v_b and writes a_b.  Pass 2: the same tiles apply with a
// workgroup-uniform a_b.
//
// Blocks whose length is no multiple of V, or whose streams are not 16-byte aligned, take element
// accesses in the same kernels: the same pieces (what lies past the block reads as 0), the same
// arithmetic, the same tree.  No atomics, no scratch memory, nothing on the host; the order of every
// sum depends on the block's length alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "zs_common.h"
#include "zs_piece.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kResidentMax = 16384;  // elements of the largest resident block
constexpr int kTilePieces = 4;       // two-pass: pieces per thread and tile

struct AmEntry {
  const void* g;          // the reduced gradient sum, GT
  const void* master;     // fp32 master, or (split) the bf16 parameter
  void* master_out;       // fp32 master (in place), or (split) the int16 residual, read and written
  unsigned short* p_out;  // bf16 copy of the updated parameter; (split) the bf16 parameter; or null
  float* m;               // exp_avg, one per element
  float* v;               // block_exp_avg_sq, one per block
  float* a;               // scratch, one per block: the block's step a_b
  double* part;           // scratch (two-pass), [block][tile]: each tile's sum of g^2
  int64_t L;              // elements of a block
  int32_t nblk;           // blocks
  int32_t tpb;            // tiles per block (two-pass; a resident entry: 0)
  int32_t vec;            // 16-byte accesses
  int32_t reserved;
};

struct AmHP {
  double step_size;  // lr / (1 - beta1^t)
  double bc2_sqrt;   // sqrt(1 - beta2^t)
  double eps;
  float lerp_w;      // ATen's lerp with weight w = 1 - beta1: w, or w - 1 when lerp_hi
  float beta2, omb2, decay_mul;
  float grad_div, inv_div;
  int lerp_hi, div_pow2, maximize;
};

// the averaged gradient the rule starts from: `grad / ws` (a power-of-two divisor is an exact
// reciprocal multiply) and maximize
__device__ __forceinline__ float prep_grad(float s, const AmHP& hp) {
#pragma clang fp contract(off)
  float g = hp.div_pow2 ? s * hp.inv_div : s / hp.grad_div;
  if (hp.maximize) g = -g;
  return g;
}

// ATen's lerp (Lerp.h): self + w * (end - self) for |w| < 0.5, end - (end - self) * (1 - w) otherwise
__device__ __forceinline__ float lerp_to(float self, float end, const AmHP& hp) {
#pragma clang fp contract(off)
  return fmaf(hp.lerp_w, end - self, hp.lerp_hi ? end : self);
}

// v_b = v_b * beta2 + (1 - beta2) * mean g^2 (fp32: the mean rounded once, one product, one fma),
// then a_b = fp32(-(lr / bc1) / (sqrt(v_b) / sqrt(bc2) + eps)) in double
__device__ __forceinline__ float block_step(float* vp, double sum, double L, const AmHP& hp) {
#pragma clang fp contract(off)
  const float s = float(sum / L);
  const float v = fmaf(hp.omb2, s, *vp * hp.beta2);
  *vp = v;
  return float(-hp.step_size / (sqrt(double(v)) / hp.bc2_sqrt + hp.eps));
}

// the fp32 fma chain over a piece's squares
template <typename GT>
__device__ __forceinline__ float piece_sumsq(uint4 q, const AmHP& hp) {
#pragma clang fp contract(off)
  constexpr int V = 16 / int(sizeof(GT));
  float g[V];
  unpack_g<GT>(q, g);
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float x = prep_grad(g[j], hp);
    s = fmaf(x, x, s);
  }
  return s;
}

// m = lerp(m, g, 1 - beta1);  p = fma(a_b, m, p * decay) over one piece whose gradient is held in q
template <typename GT, bool SPLIT, bool VEC>
__device__ __forceinline__ void apply_piece(const AmEntry& e, int64_t i, int n, uint4 q, float a,
                                            const AmHP& hp) {
#pragma clang fp contract(off)
  constexpr int V = 16 / int(sizeof(GT));
  float g[V], m[V], p[V];
  unpack_g<GT>(q, g);
  load_m<V, VEC>(e.m, i, n, m);
  load_p<V, VEC, SPLIT>(e, i, n, p);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    m[j] = lerp_to(m[j], prep_grad(g[j], hp), hp);
    p[j] = fmaf(a, m[j], p[j] * hp.decay_mul);
  }
  store_m<V, VEC>(e.m, i, n, m);
  store_p<V, VEC, SPLIT>(e, i, n, p);
}

// ---- resident path ---------------------------------------------------------------------------
template <typename GT, bool SPLIT, bool VEC>
__device__ __forceinline__ void resident_body(const AmEntry& e, int64_t blk, const AmHP& hp,
                                              double* wave_part, float* a_sh) {
  constexpr int V = 16 / int(sizeof(GT));
  constexpr int NP = kResidentMax / (kThreads * V);  // pieces a thread holds at most
  const int L = int(e.L);                            // (<= kResidentMax)
  const int64_t base = blk * e.L;
  const int npieces = (L + V - 1) / V;
  const int tid = int(threadIdx.x);
  uint4 q[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) {  // every load of the block before the first use
    const int pc = k * kThreads + tid;
    q[k] = make_uint4(0u, 0u, 0u, 0u);
    if (pc < npieces) q[k] = load_g_piece<GT, VEC>(e.g, base + int64_t(pc) * V, L - pc * V);
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < NP; ++k)
    if (k * kThreads < npieces) acc += double(piece_sumsq<GT>(q[k], hp));  // (an idle piece: 0)
  const double sum = block_sum(acc, wave_part);
  if (tid == 0) {
    const float a = block_step(e.v + blk, sum, double(L), hp);
    e.a[blk] = a;
    *a_sh = a;
  }
  __syncthreads();
  const float a = *a_sh;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int pc = k * kThreads + tid;
    if (pc < npieces)
      apply_piece<GT, SPLIT, VEC>(e, base + int64_t(pc) * V, L - pc * V, q[k], a, hp);
  }
}

// kernel-resource-usage (gfx950): see DESIGN.md §4 "Fused Adam-mini"
template <typename GT, bool SPLIT>
__global__ __launch_bounds__(kThreads) void adamini_resident_kernel(
    const AmEntry* __restrict__ entries, const int64_t* __restrict__ res_prefix, int64_t nent,
    const AmHP hp) {
  __shared__ double wave_part[kWaves];
  __shared__ float a_sh;
  const int64_t ei = find_entry(res_prefix, nent, blockIdx.x);
  const AmEntry e = entries[ei];
  const int64_t blk = int64_t(blockIdx.x) - res_prefix[ei];
  if (e.vec) resident_body<GT, SPLIT, true>(e, blk, hp, wave_part, &a_sh);
  else resident_body<GT, SPLIT, false>(e, blk, hp, wave_part, &a_sh);
}

// ---- two-pass path ---------------------------------------------------------------------------
// tile t of a block: pieces t * kTilePieces * 256 + k * 256 + thread, k < kTilePieces
template <typename GT, bool VEC>
__device__ __forceinline__ void tile_load(const AmEntry& e, int64_t base, int64_t t, uint4* q) {
  constexpr int V = 16 / int(sizeof(GT));
#pragma unroll
  for (int k = 0; k < kTilePieces; ++k) {
    const int64_t off = ((t * kTilePieces + k) * kThreads + threadIdx.x) * V;
    q[k] = make_uint4(0u, 0u, 0u, 0u);
    if (off < e.L) {
      const int64_t left = e.L - off;
      q[k] = load_g_piece<GT, VEC>(e.g, base + off, left < V ? int(left) : V);
    }
  }
}

template <typename GT>
__global__ __launch_bounds__(kThreads) void adamini_partial_kernel(
    const AmEntry* __restrict__ entries, const int64_t* __restrict__ tile_prefix, int64_t nent,
    const AmHP hp) {
  __shared__ double wave_part[kWaves];
  const int64_t ei = find_entry(tile_prefix, nent, blockIdx.x);
  const AmEntry e = entries[ei];
  const int64_t lt = int64_t(blockIdx.x) - tile_prefix[ei];
  const int64_t blk = lt / e.tpb, t = lt % e.tpb;
  uint4 q[kTilePieces];
  if (e.vec) tile_load<GT, true>(e, blk * e.L, t, q);
  else tile_load<GT, false>(e, blk * e.L, t, q);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kTilePieces; ++k) acc += double(piece_sumsq<GT>(q[k], hp));
  const double sum = block_sum(acc, wave_part);
  if (threadIdx.x == 0) e.part[lt] = sum;
}

// one thread per two-pass block: its tiles' slots in order, v_b, a_b
__global__ __launch_bounds__(kThreads) void adamini_finish_kernel(
    const AmEntry* __restrict__ entries, const int64_t* __restrict__ fin_prefix, int64_t nent,
    const AmHP hp) {
  const int64_t x = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (x >= fin_prefix[nent]) return;
  const int64_t ei = find_entry(fin_prefix, nent, x);
  const AmEntry e = entries[ei];
  const int64_t blk = x - fin_prefix[ei];
  double s = 0.0;
  for (int k = 0; k < e.tpb; ++k) s += e.part[blk * e.tpb + k];
  e.a[blk] = block_step(e.v + blk, s, double(e.L), hp);
}

template <typename GT, bool SPLIT, bool VEC>
__device__ __forceinline__ void tile_apply(const AmEntry& e, int64_t blk, int64_t t,
                                           const AmHP& hp) {
  constexpr int V = 16 / int(sizeof(GT));
  const int64_t base = blk * e.L;
  const float a = e.a[blk];  // (uniform over the workgroup)
  uint4 q[kTilePieces];
  tile_load<GT, VEC>(e, base, t, q);
#pragma unroll
  for (int k = 0; k < kTilePieces; ++k) {
    const int64_t off = ((t * kTilePieces + k) * kThreads + threadIdx.x) * V;
    if (off < e.L) {
      const int64_t left = e.L - off;
      apply_piece<GT, SPLIT, VEC>(e, base + off, left < V ? int(left) : V, q[k], a, hp);
    }
  }
}

template <typename GT, bool SPLIT>
__global__ __launch_bounds__(kThreads) void adamini_apply_kernel(
    const AmEntry* __restrict__ entries, const int64_t* __restrict__ tile_prefix, int64_t nent,
    const AmHP hp) {
  const int64_t ei = find_entry(tile_prefix, nent, blockIdx.x);
  const AmEntry e = entries[ei];
  const int64_t lt = int64_t(blockIdx.x) - tile_prefix[ei];
  if (e.vec) tile_apply<GT, SPLIT, true>(e, lt / e.tpb, lt % e.tpb, hp);
  else tile_apply<GT, SPLIT, false>(e, lt / e.tpb, lt % e.tpb, hp);
}

}  // namespace

struct zs_adaminiset {
  unsigned tag = zs::kAdaminiSetTag;
  AmEntry* d_entries = nullptr;
  int64_t* d_res_prefix = nullptr;   // resident blocks before each entry
  int64_t* d_tile_prefix = nullptr;  // two-pass tiles before each entry
  int64_t* d_fin_prefix = nullptr;   // two-pass blocks before each entry
  // one allocation: the two-pass entries' tile slots (doubles), then a_b of every block (floats, in
  // table order)
  unsigned char* d_scratch = nullptr;
  float* d_a = nullptr;
  int64_t nent = 0, res_blocks = 0, tiles = 0, fin_blocks = 0, blocks = 0;
  int64_t elems = 0, path_elems[2] = {0, 0}, path_bytes[2] = {0, 0}, scratch_bytes = 0;
  int g_dtype = ZS_F32, p_dtype = ZS_BF16, resident_cap = 0;
};

// mask: bit 0 = the resident kernel, bit 1 = pass 1 with the finish kernel behind it, bit 2 = pass 2
template <typename GT, bool SPLIT>
static int run_paths(const zs_adaminiset* s, const AmHP& hp, hipStream_t st, int mask) {
  const dim3 block(kThreads);
  if ((mask & 1) && s->res_blocks)
    adamini_resident_kernel<GT, SPLIT><<<dim3(unsigned(s->res_blocks)), block, 0, st>>>(
        s->d_entries, s->d_res_prefix, s->nent, hp);
  if ((mask & 2) && s->tiles) {
    adamini_partial_kernel<GT><<<dim3(unsigned(s->tiles)), block, 0, st>>>(
        s->d_entries, s->d_tile_prefix, s->nent, hp);
    adamini_finish_kernel<<<dim3(unsigned((s->fin_blocks + kThreads - 1) / kThreads)), block, 0,
                            st>>>(s->d_entries, s->d_fin_prefix, s->nent, hp);
  }
  if ((mask & 4) && s->tiles)
    adamini_apply_kernel<GT, SPLIT><<<dim3(unsigned(s->tiles)), block, 0, st>>>(
        s->d_entries, s->d_tile_prefix, s->nent, hp);
  ZS_HIP(hipGetLastError());
  return ZS_OK;
}

static int check_hparams(const char* fn, double lr, double beta1, double beta2, double eps,
                         double weight_decay, double grad_div) {
  // zero_amd.optim.AdamMini.__init__'s rules (a NaN fails every comparison)
  ZS_REQUIRE(lr >= 0.0, "%s: invalid learning rate %g", fn, lr);
  ZS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "%s: invalid beta parameter at index 0: %g", fn, beta1);
  ZS_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "%s: invalid beta parameter at index 1: %g", fn, beta2);
  ZS_REQUIRE(eps >= 0.0, "%s: invalid epsilon value %g", fn, eps);
  ZS_REQUIRE(weight_decay >= 0.0, "%s: invalid weight_decay value %g", fn, weight_decay);
  ZS_REQUIRE(grad_div > 0.0, "%s: grad_div must be > 0", fn);
  return ZS_OK;
}

static int run_checked(const char* fn, const zs_adaminiset* as, const zs_adamini_hparams* h,
                       int64_t step, int mask, uintptr_t stream) {
  ZS_REQUIRE(as && h, "%s: NULL argument", fn);
  ZS_REQUIRE(as->tag == zs::kAdaminiSetTag, "%s: the set was not made by zs_adaminiset_create", fn);
  ZS_REQUIRE(step >= 1, "%s: step must be >= 1 (the count after this step; got %lld)", fn,
             (long long)step);
  // a struct filled by hand gets zs_adamini_hparams_init's rules too
  if (int rc = check_hparams(fn, h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, h->grad_div))
    return rc;
  if (as->nent == 0) return ZS_OK;
  // the host scalars in double, each rounded to fp32 once; a_b's three stay double
  const double t = double(step);
  AmHP hp;
  hp.step_size = h->lr / (1.0 - std::pow(h->beta1, t));
  hp.bc2_sqrt = std::sqrt(1.0 - std::pow(h->beta2, t));
  hp.eps = h->eps;
  const float w = float(1.0 - h->beta1);
  hp.lerp_hi = std::fabs(w) < 0.5f ? 0 : 1;
  hp.lerp_w = hp.lerp_hi ? w - 1.0f : w;
  hp.beta2 = float(h->beta2);
  hp.omb2 = float(1.0 - h->beta2);
  hp.decay_mul = h->weight_decay != 0.0 ? float(1.0 - h->lr * h->weight_decay) : 1.0f;
  int exp2 = 0;
  hp.grad_div = float(h->grad_div);
  hp.div_pow2 = std::frexp(double(hp.grad_div), &exp2) == 0.5 ? 1 : 0;
  hp.inv_div = float(1.0 / double(hp.grad_div));
  hp.maximize = h->maximize ? 1 : 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool g32 = as->g_dtype == ZS_F32, split = as->p_dtype == ZS_BF16_SPLIT;
  if (g32)
    return split ? run_paths<float, true>(as, hp, st, mask)
                 : run_paths<float, false>(as, hp, st, mask);
  return split ? run_paths<unsigned short, true>(as, hp, st, mask)
               : run_paths<unsigned short, false>(as, hp, st, mask);
}

extern "C" {

int zs_adamini_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                            int maximize, double grad_div, zs_adamini_hparams* hp) {
  const char* fn = "zs_adamini_hparams_init";
  ZS_REQUIRE(hp != nullptr, "%s: hp is NULL", fn);
  if (int rc = check_hparams(fn, lr, beta1, beta2, eps, weight_decay, grad_div)) return rc;
  hp->lr = lr;
  hp->beta1 = beta1;
  hp->beta2 = beta2;
  hp->eps = eps;
  hp->weight_decay = weight_decay;
  hp->grad_div = grad_div;
  hp->maximize = maximize ? 1 : 0;
  hp->reserved = 0;
  return ZS_OK;
}

int zs_adaminiset_create(const zs_adamini_seg* in, int64_t n, int g_dtype, int p_dtype,
                         int64_t resident_cap, zs_adaminiset** out) {
  const char* fn = "zs_adaminiset_create";
  ZS_REQUIRE(out != nullptr, "%s: out is NULL", fn);
  *out = nullptr;
  ZS_REQUIRE(n >= 0 && (n == 0 || in), "%s: bad table", fn);
  ZS_REQUIRE(g_dtype == ZS_F32 || g_dtype == ZS_BF16, "%s: bad g_dtype %d", fn, g_dtype);
  ZS_REQUIRE(p_dtype == ZS_BF16 || p_dtype == ZS_BF16_SPLIT,
             "%s: p_dtype must be ZS_BF16 or ZS_BF16_SPLIT (got %d)", fn, p_dtype);
  ZS_REQUIRE(resident_cap >= 0 && resident_cap <= kResidentMax,
             "%s: resident_cap must be in [0, %d] (got %lld)", fn, kResidentMax,
             (long long)resident_cap);
  ZS_REQUIRE(n < (int64_t(1) << 31), "%s: %lld entries (max 2^31 - 1)", fn, (long long)n);
  const bool split = p_dtype == ZS_BF16_SPLIT;
  const int64_t gsz = g_dtype == ZS_F32 ? 4 : 2, V = 16 / gsz;
  const int64_t msz = split ? 2 : 4;
  const int64_t tile_elems = int64_t(kTilePieces) * kThreads * V;
  std::vector<AmEntry> ent;
  std::vector<int64_t> rpre(1, 0), tpre(1, 0), fpre(1, 0);
  std::vector<int64_t> a_off, part_off;  // per entry, in floats / doubles
  int64_t blocks = 0, slots = 0, elems = 0;
  int64_t path_elems[2] = {0, 0}, path_bytes[2] = {0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const zs_adamini_seg& s = in[i];
    ZS_REQUIRE(s.R >= 1 && s.C >= 1, "%s: entry %lld: R and C must be >= 1", fn, (long long)i);
    ZS_REQUIRE(s.R < (int64_t(1) << 31) && s.C < (int64_t(1) << 31) &&
                   s.R * s.C < (int64_t(1) << 40),
               "%s: entry %lld: R or C too large", fn, (long long)i);
    ZS_REQUIRE(s.g && s.master && s.master_out && s.m && s.v,
               "%s: entry %lld missing g/master/master_out/m/v", fn, (long long)i);
    ZS_REQUIRE(s.block_rows >= 0 && (s.block_rows == 0 || s.R % s.block_rows == 0),
               "%s: entry %lld: block_rows %lld does not divide R = %lld", fn, (long long)i,
               (long long)s.block_rows, (long long)s.R);
    ZS_REQUIRE(!split || s.p_out, "%s: entry %lld: a split master needs p_out", fn, (long long)i);
    ZS_REQUIRE(split || s.master_out == s.master,
               "%s: entry %lld: the fp32 master is updated in place (master_out == master)", fn,
               (long long)i);
    ZS_REQUIRE(aligned(s.g, uint64_t(gsz)) && aligned(s.master, uint64_t(msz)) &&
                   aligned(s.master_out, uint64_t(msz)) && aligned(s.p_out, 2) &&
                   aligned(s.m, 4) && aligned(s.v, 4),
               "%s: entry %lld: a pointer is not aligned to its element", fn, (long long)i);
    ZS_REQUIRE(s.param >= 0, "%s: entry %lld: param < 0", fn, (long long)i);
    AmEntry e{};
    e.g = reinterpret_cast<const void*>(s.g);
    e.master = reinterpret_cast<const void*>(s.master);
    e.master_out = reinterpret_cast<void*>(s.master_out);
    e.p_out = reinterpret_cast<unsigned short*>(s.p_out);
    e.m = reinterpret_cast<float*>(s.m);
    e.v = reinterpret_cast<float*>(s.v);
    const int64_t ne = s.R * s.C;
    e.L = s.block_rows == 0 ? ne : s.block_rows * s.C;
    e.nblk = int32_t(ne / e.L);
    // 16-byte accesses: every block starts at a 16-byte multiple of every stream
    // (a piece of the split master's two 16-bit streams is 2 V bytes, of an fp32 stream 16-byte loads)
    const uint64_t ma = split ? uint64_t(2 * V) : 16;
    e.vec = e.L % V == 0 && aligned(s.g, 16) && aligned(s.m, 16) && aligned(s.master, ma) &&
            aligned(s.master_out, ma) && aligned(s.p_out, uint64_t(2 * V));
    const int path = e.L <= resident_cap ? 0 : 1;
    e.tpb = path ? int32_t((e.L + tile_elems - 1) / tile_elems) : 0;
    const int64_t tiles = int64_t(e.nblk) * e.tpb;
    ZS_REQUIRE(rpre.back() + e.nblk < (int64_t(1) << 31) && tpre.back() + tiles < (int64_t(1) << 31),
               "%s: too many blocks or tiles", fn);
    rpre.push_back(rpre.back() + (path ? 0 : e.nblk));
    tpre.push_back(tpre.back() + tiles);
    fpre.push_back(fpre.back() + (path ? e.nblk : 0));
    a_off.push_back(blocks), blocks += e.nblk;
    part_off.push_back(slots), slots += tiles;
    ent.push_back(e);
    elems += ne;
    path_elems[path] += ne;
    // g (twice on the two-pass path), m read and written, the master read and written
    path_bytes[path] += ne * (gsz * (1 + path) + 8 + 4 + 4 + (!split && s.p_out ? 2 : 0)) +
                        int64_t(e.nblk) * 8;
  }
  zs_adaminiset* as = new (std::nothrow) zs_adaminiset();
  if (!as) return zs::fail(ZS_ERR_NOMEM, "%s: out of memory", fn);
  as->nent = int64_t(ent.size());
  as->res_blocks = rpre.back(), as->tiles = tpre.back(), as->fin_blocks = fpre.back();
  as->blocks = blocks;
  as->elems = elems;
  for (int k = 0; k < 2; ++k) as->path_elems[k] = path_elems[k], as->path_bytes[k] = path_bytes[k];
  as->g_dtype = g_dtype, as->p_dtype = p_dtype, as->resident_cap = int(resident_cap);
  *out = as;
  if (as->nent == 0) return ZS_OK;
  as->scratch_bytes = slots * 8 + (blocks + 3) / 4 * 16;
  int rc = ZS_OK;
  hipError_t he = hipMalloc(reinterpret_cast<void**>(&as->d_scratch), size_t(as->scratch_bytes));
  if (he != hipSuccess)
    rc = zs::fail(ZS_ERR_HIP, "%s: hipMalloc of %lld scratch bytes failed: %s", fn,
                  (long long)as->scratch_bytes, hipGetErrorString(he));
  if (rc == ZS_OK) {
    double* d0 = reinterpret_cast<double*>(as->d_scratch);
    as->d_a = reinterpret_cast<float*>(d0 + slots);
    for (size_t k = 0; k < ent.size(); ++k) {
      ent[k].a = as->d_a + a_off[k];
      ent[k].part = d0 + part_off[k];
    }
    rc = upload(ent, &as->d_entries);
  }
  if (rc == ZS_OK) rc = upload(rpre, &as->d_res_prefix);
  if (rc == ZS_OK) rc = upload(tpre, &as->d_tile_prefix);
  if (rc == ZS_OK) rc = upload(fpre, &as->d_fin_prefix);
  if (rc != ZS_OK) {
    zs_adaminiset_destroy(as);
    *out = nullptr;
  }
  return rc;
}

int zs_adaminiset_run(const zs_adaminiset* as, const zs_adamini_hparams* h, int64_t step,
                      uintptr_t stream) {
  return run_checked("zs_adaminiset_run", as, h, step, 7, stream);
}

int zs_adaminiset_run_pass(const zs_adaminiset* as, const zs_adamini_hparams* h, int64_t step,
                           int pass, uintptr_t stream) {
  ZS_REQUIRE(pass >= 0 && pass <= 2, "zs_adaminiset_run_pass: pass must be 0, 1 or 2 (got %d)",
             pass);
  return run_checked("zs_adaminiset_run_pass", as, h, step, 1 << pass, stream);
}

int zs_adaminiset_stats(const zs_adaminiset* as, int64_t* out, int64_t n) {
  ZS_REQUIRE(as && out && n >= 0, "zs_adaminiset_stats: NULL argument");
  ZS_REQUIRE(as->tag == zs::kAdaminiSetTag,
             "zs_adaminiset_stats: the set was not made by zs_adaminiset_create");
  const int64_t v[9] = {as->elems, as->path_bytes[0] + as->path_bytes[1], as->path_elems[0],
                        as->path_bytes[0], as->path_elems[1], as->path_bytes[1],
                        as->scratch_bytes, as->blocks,
                        int64_t(reinterpret_cast<uintptr_t>(as->d_a))};
  for (int64_t k = 0; k < n && k < 9; ++k) out[k] = v[k];
  return ZS_OK;
}

int zs_adaminiset_destroy(zs_adaminiset* as) {
  if (!as) return ZS_OK;
  ZS_REQUIRE(as->tag == zs::kAdaminiSetTag,
             "zs_adaminiset_destroy: the set was not made by zs_adaminiset_create");
  if (as->d_entries) (void)hipFree(as->d_entries);
  if (as->d_res_prefix) (void)hipFree(as->d_res_prefix);
  if (as->d_tile_prefix) (void)hipFree(as->d_tile_prefix);
  if (as->d_fin_prefix) (void)hipFree(as->d_fin_prefix);
  if (as->d_scratch) (void)hipFree(as->d_scratch);
  delete as;
  return ZS_OK;
}

}  // extern "C"
