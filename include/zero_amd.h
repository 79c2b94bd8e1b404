/*
 * zero_amd.h — C ABI of the MI355X-native ZeRO sharded-optimizer step.
 *
 * The reference (xo-toybox/distributed-training-sandbox, zero/zero{1,2,3}.py) has no native code:
 * its hot path is Python calling c10d collectives and torch.optim.Adam.  This library is what the
 * drop-in ShardedOptimizer (distributed-training-sandbox_amd/zero_amd/zero{1,2,3}.py) binds with
 * ctypes.  Every entry point below names the reference interface it replaces.
 *
 * Conventions
 *  - plain C types only: no torch types cross this boundary; device buffers are raw pointers
 *    (uint64_t / void*) owned by the caller (torch tensors); the library never frees caller memory.
 *  - every launch takes a hipStream_t passed as uintptr_t (torch.cuda.Stream.cuda_stream);
 *    nothing synchronises the host except *_create (table upload) and zs_comm_init.
 *  - every function returns int status: ZS_OK (0) or a ZS_ERR_* code; zs_last_error() returns a
 *    thread-local message for the most recent failure on the calling thread.
 *  - element counts are int64_t elements; byte counts say "bytes".
 */
#ifndef ZERO_AMD_H
#define ZERO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Callers check zs_abi_version() == ZS_ABI_VERSION before any other call: version 7 kept the
 * names zs_plan_create / zs_adam_step but changed their argument lists (the version-6 forms are
 * the *_ex entry points), so a caller built against an older header links and then passes the
 * wrong arguments.  The Python binding (zero_amd/_lib.py) and tests/c/abi_host.c refuse a
 * mismatch. */
#define ZS_ABI_VERSION 13

enum zs_status {
  ZS_OK = 0,
  ZS_ERR_INVALID = 1,   /* bad argument / shape mismatch */
  ZS_ERR_HIP = 2,       /* hipError_t from the runtime */
  ZS_ERR_RCCL = 3,      /* ncclResult_t from RCCL */
  ZS_ERR_NOMEM = 4
};

enum zs_dtype {
  ZS_F32 = 0,
  ZS_BF16 = 1,
  ZS_U8 = 2,        /* raw bytes (fp8 payloads); collectives only */
  ZS_BF16_SPLIT = 3, /* zs_adamset_create p_dtype only: the fp32 master stored as the bf16 param
                        (its round-to-nearest-even high half) + a 16-bit residual, see zs_adam_seg */
  ZS_BF16_SR = 4     /* zs_adamset_create_ex p_dtype only: no master at all, the bf16 param updated
                        in place with stochastic rounding, see zs_adamset_run_psr */
};

/* Shard layouts (SURVEY.md §7 "Two shard layouts"). */
enum zs_layout {
  ZS_LAYOUT_R = 0,  /* reference owner-by-parameter-index (zero1.py:55-62, zero2.py:51-58) */
  ZS_LAYOUT_Z = 1,  /* dim-0 chunk of every parameter, torch.chunk semantics (zero3.py:105-110) */
  ZS_LAYOUT_F = 2   /* flat: one balanced contiguous 1/ws slice of the concatenated params */
};

/* Bucketing of the per-rank streams (see zs_plan_bucket). */
enum zs_bucket_mode {
  ZS_BUCKETS_RAGGED = 0, /* equal windows over the shortest stream, then per-owner ragged windows */
  ZS_BUCKETS_PADDED = 1  /* equal windows over the longest stream, shorter streams zero-padded */
};

int zs_abi_version(void);
const char* zs_last_error(void);

/* roctx range around a phase of step(), named like the reference's torch.profiler ranges
 * "all_reduce_gradients" / "optimizer_step" / "broadcast_parameters" (zero1.py:80-91), so
 * `rocprofv3 --marker-trace` shows which kernels and collectives each phase enqueued.  Host only;
 * no-ops unless a profiler is attached. */
int zs_range_push(const char* name);
int zs_range_pop(void);

/* ------------------------------------------------------------------------------------------ */
/* Layout planner (host only; callable without a GPU).                                         */
/* ------------------------------------------------------------------------------------------ */
typedef struct zs_plan zs_plan;

/* Replaces ShardedOptimizer.__init__'s ownership computation (zero1.py:44-62, zero2.py:39-58,
 * zero3.py:82-110).  numels[i] = params[i].numel(); dim0[i] = params[i].shape[0] (1 for 0-d;
 * only read for ZS_LAYOUT_Z, may be NULL otherwise).  SURVEY.md §8(b)'s signature: bucket_bytes
 * is the size of one bucket buffer in fp32 elements' bytes (a bf16 bucket of the same plan holds
 * the same elements in half the bytes; 0 = one bucket holding the whole longest stream); pieces
 * are 64-element aligned; ragged buckets (ZS_BUCKETS_RAGGED). */
int zs_plan_create(int64_t n_params, const int64_t* numels, const int64_t* dim0, int ws, int rank,
                   int layout, int64_t bucket_bytes, zs_plan** out);
/* The general form the Python engine uses: align_elems: every piece starts at a multiple of this
 * in its rank's stream (>=1).  window_elems: per-rank elements per bucket (0 = one bucket holding
 * the whole longest stream).  bucket_mode: ZS_BUCKETS_*. */
int zs_plan_create_ex(int64_t n_params, const int64_t* numels, const int64_t* dim0, int ws,
                      int rank, int layout, int64_t align_elems, int64_t window_elems,
                      int bucket_mode, zs_plan** out);
int zs_plan_destroy(zs_plan* plan);

/* info[0..9] = {n_params, ws, rank, layout, window_elems W, num_buckets K, max_stream_len M,
 *              arena_elems (all buckets, each starting align_elems-aligned), num_even_buckets,
 *              bucket_mode} */
int zs_plan_info(const zs_plan* plan, int64_t* info10);

/* Parameter-index ownership [start,end) of `rank` (zero1.py:55-62).  Same formula for every
 * layout: it is what the reference uses to filter the inner optimizer's param_groups. */
int zs_plan_owner_range(const zs_plan* plan, int rank, int64_t* start, int64_t* end);

/* Broadcast-source rank of parameter i (zero1.py:95-100, zero2.py:126-131). */
int zs_plan_owner_of(const zs_plan* plan, int64_t i, int* owner);

/* Length (elements, padded to align) of rank r's stream = its optimizer shard. */
int zs_plan_stream_len(const zs_plan* plan, int rank, int64_t* len);

/* Pieces of rank r's stream: param index, element offset inside the (flattened) param,
 * element offset inside the stream, length.  Arrays sized by zs_plan_num_pieces. */
int zs_plan_num_pieces(const zs_plan* plan, int rank, int64_t* n);
int zs_plan_pieces(const zs_plan* plan, int rank, int64_t* param, int64_t* param_off,
                   int64_t* stream_off, int64_t* len);

/* Bucket k: its offset and length (elements) in the arena, whether it is *even* (every window
 * the same length and window r at r*len: one equal-count reduce-scatter / all-gather moves it;
 * buckets 0..num_even-1) or *ragged* (one grouped reduce / broadcast per owner moves it), and per
 * rank r (arrays of ws): the window's offset inside the bucket, its length (0 = no data), and the
 * stream offset of its first element.  Replaces the per-tensor collective loop over
 * self.params (zero1.py:80-84, zero2.py:94-113) with a fixed bucket schedule. */
int zs_plan_bucket(const zs_plan* plan, int64_t bucket, int64_t* arena_off, int64_t* elems,
                   int* even, int64_t* win_off, int64_t* win_len, int64_t* win_stream);

/* Segments of bucket k (all ranks): param slices and where they sit in the bucket buffer.
 * buf_off is the element offset inside the bucket buffer (win_off[rank] + offset in window). */
int zs_plan_num_segments(const zs_plan* plan, int64_t bucket, int64_t* n);
int zs_plan_segments(const zs_plan* plan, int64_t bucket, int64_t* param, int64_t* rank,
                     int64_t* param_off, int64_t* buf_off, int64_t* len);

/* Number of buckets K (= info[5]) and the byte size of bucket k's buffer for dtype ZS_F32 /
 * ZS_BF16 (SURVEY.md §8(b) zs_plan_num_buckets / zs_plan_bucket_bytes). */
int zs_plan_num_buckets(const zs_plan* plan, int64_t* n);
int zs_plan_bucket_bytes(const zs_plan* plan, int64_t bucket, int dtype, int64_t* bytes);

/* Pack / unpack one bucket straight from the plan (SURVEY.md §8(b) zs_pack / zs_unpack).
 * grad_ptrs / param_ptrs: n_params device pointers indexed by parameter (flattened, dtype ZS_F32
 * or ZS_BF16); bucket_buf: the bucket's buffer (zs_plan_bucket_bytes long).  zs_pack copies every
 * segment of every rank's window (zero2.py:99-104 without the ws-fold torch.cat) — a NULL grad
 * is written as zeros; zs_unpack scatters every segment back into the params (the per-tensor
 * broadcast of zero2.py:122-133 after the all-gather).  Window padding is never written: zero
 * the buffer once.  The descriptor tables are built on the first call and reused while the
 * pointers are unchanged; tables replaced by new pointers are kept until zs_plan_destroy, which
 * must not be called while a pack / unpack of the plan may still run. */
int zs_pack(zs_plan* plan, int64_t bucket, const uint64_t* grad_ptrs, void* bucket_buf, int dtype,
            uintptr_t stream);
int zs_unpack(zs_plan* plan, int64_t bucket, const void* bucket_buf, const uint64_t* param_ptrs,
              int dtype, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Segment copy (pack / unpack).  Replaces the flatten + torch.cat([g]*ws) copies of            */
/* zero2.py:99-104, the chunk().contiguous() copies of zero3.py:44-51,107-108,142-143 and the   */
/* torch.cat of gathered shards (zero3.py:40).                                                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct zs_copyset zs_copyset;

/* src[i]==0 means "write nbytes[i] zero bytes to dst[i]".  The table is uploaded once. */
int zs_copyset_create(const uint64_t* src, const uint64_t* dst, const int64_t* nbytes, int64_t n,
                      zs_copyset** out);
int zs_copyset_run(const zs_copyset* cs, uintptr_t stream);
int zs_copyset_destroy(zs_copyset* cs);
/* The same copy without a table (ABI v11): the segments travel in the kernel arguments, up to 64
 * per launch (more take more launches), so pointers that change on every call cost nothing to
 * set up — backward's fresh gradients copied into their flat-arena slots (zero2.py:99-104's
 * flatten, per overlap bucket).  src[i]==0: zero fill; empty segments are skipped. */
int zs_copy_direct(int64_t n, const uint64_t* src, const uint64_t* dst, const int64_t* nbytes,
                   uintptr_t stream);

/* In-place x[i] /= div over n elements (dtype ZS_F32 / ZS_BF16, x 16-byte aligned): the
 * `param.grad /= dist.get_world_size()` of DDP's sync_gradients (DDP/ddp.py:45-47), applied to a
 * whole all-reduced gradient bucket.  fp32: IEEE division (reciprocal multiply when div and 1/div
 * are both fp32 powers of two, which is exact); bf16: computed in fp32, rounded to nearest even. */
int zs_scale(void* x, int64_t n, int dtype, double div, uintptr_t stream);

/* dst[i] = dst[i] + src[i] over n elements (dtype ZS_F32 / ZS_BF16; dst and src 16-byte aligned):
 * gradient accumulation on a shard — a later micro-batch's reduce-scattered chunks, received in a
 * staging buffer (ncclReduceScatter overwrites its receive buffer), added to the chunks already
 * held (ZeRO-3 update mode, grad_accumulation=True).  fp32: one IEEE add; bf16: both operands
 * widened exactly, one fp32 add, rounded to nearest even (NaN stays NaN) — torch's add_ on a tensor
 * of that dtype, which is what AccumulateGrad does to p.grad.  Denormals are kept.  n == 0: ZS_OK,
 * nothing launched; n < 0, a NULL or misaligned pointer with n > 0, another dtype: ZS_ERR_INVALID,
 * nothing launched.  Additive to ABI v13. */
int zs_accumulate(void* dst, const void* src, int64_t n, int dtype, uintptr_t stream);

/* The same accumulation with an fp32 sum of bf16 contributions (ZeRO-3 update mode,
 * accumulation_dtype=torch.float32), over n elements:
 *   a_bf16 != NULL:  dst[i] = widen(a[i]) + widen(src[i])   (the first accumulating pass: the
 *                    first pass's bf16 chunks plus the staging buffer; 2 + 2 B read, 4 B written)
 *   a_bf16 == NULL:  dst[i] = dst[i] + widen(src[i])        (later passes; 4 + 2 B read, 4 written)
 * Widening is exact; one IEEE fp32 add per element (NaN stays NaN, Inf + -Inf is NaN, denormals
 * are kept).  dst 16-byte aligned, a and src 8-byte aligned.  n == 0: ZS_OK, nothing launched;
 * n < 0, a NULL dst or src or a misaligned pointer with n > 0: ZS_ERR_INVALID, nothing launched.
 * Cache policy under zs_tune("accumulate_nt").  Additive to ABI v13. */
int zs_accumulate_widen(float* dst, const void* a_bf16, const void* src_bf16, int64_t n,
                        uintptr_t stream);

/* n elements fp32 -> bf16 (round to nearest even, NaN stays NaN) or bf16 -> fp32 (exact).  The
 * bf16 gradient exchange of fp32-parameter models: the reference reduces fp32
 * grads (zero2.py:107); converting them first halves the bytes every collective moves.  16-B
 * vector path when both buffers are 16-byte aligned, scalar otherwise. */
int zs_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, uintptr_t stream);

/* Row-wise fp8 (OCP E4M3, the gfx950 format) quantisation for the low-precision parameter
 * all-gather (the reference's torchao float8 all-gather, fp8/fp8_benchmark.py:79-81).
 * Row r of src (row_len elements, dtype ZS_F32 / ZS_BF16): amax = max|x|, inv = 448/amax,
 * dst[r, i] = e4m3(RNE(clamp(x * inv, ±448))), scales[r] = amax/448 (amax == 0: inv = scale = 1).
 * Dequantise: dst[r, i] = (float(q) * scales[r]) rounded to dst_dtype.  Replaces gathering the
 * bf16/fp32 shard in zero3.py:36-41 with 1 byte/element + 4 bytes/row. */
int zs_fp8_quantize_rows(const void* src, int src_dtype, void* dst, float* scales, int64_t rows,
                         int64_t row_len, uintptr_t stream);
int zs_fp8_dequantize_rows(const void* src, const float* scales, void* dst, int dst_dtype,
                           int64_t rows, int64_t row_len, uintptr_t stream);

/* A ZeRO-3 gather group's fp8 send side in one launch per 16 matrices (the per-module
 * materialize of zero3.py:36-41 with every matrix of the module at once): matrix m's rows
 * [0, rows[m]) of src[m] (row_len[m] elements each, src_dtype) are quantised exactly as by
 * zs_fp8_quantize_rows into q[m] / scales[m]; rows [rows[m], cs[m]) — the dim-0 chunk's padding
 * beyond this rank's real rows — are written as q = 0, scale = 1.  row_len[m] a multiple of 8,
 * src 16-B and q 8-B aligned. */
int zs_fp8_quantize_rowset(int64_t n, const uint64_t* src, const uint64_t* q, const uint64_t* scales,
                           const int64_t* rows, const int64_t* cs, const int64_t* row_len,
                           int src_dtype, uintptr_t stream);
/* The group's receive side after ONE all-gather of every rank's concatenated q buffer
 * (q_rank_bytes per rank) and ONE of its scales (sc_rank_elems per rank): full row R < ws*cs[m] of
 * matrix m is rank k = R / cs[m]'s local row lr = R % cs[m], read from
 * q + k*q_rank_bytes + q_off[m] + lr*row_len[m] with scale scales[k*sc_rank_elems + sc_off[m] + lr],
 * and written, dequantised to dst_dtype, at dst[m] + R*row_len[m] (16-B aligned).  One launch per
 * 16 matrices. */
int zs_fp8_dequantize_gathered(int64_t n, const void* q, const float* scales, int ws,
                               int64_t q_rank_bytes, int64_t sc_rank_elems, const int64_t* q_off,
                               const int64_t* sc_off, const int64_t* cs, const int64_t* row_len,
                               const uint64_t* dst, int dst_dtype, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused Adam / AdamW.  Replaces torch.optim.Adam.step on the owned shard (zero1.py:88,          */
/* zero2.py:120, zero3.py:161; math of torch/optim/adam.py:457-547) plus the grad averaging     */
/* (zero1.py:84 `p.grad /= ws`, zero2.py:111 `output / ws`, zero3.py:147).                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t g;          /* gradient (reduced SUM over ranks), dtype g_dtype; 0 = zero gradient */
  uint64_t master;     /* fp32 master / param read by the update */
  uint64_t master_out; /* fp32 destination of the updated master (may equal master, may be a
                          bucket slot; 0 = not written) */
  uint64_t p_out;      /* optional copy of the updated param in p_dtype (bf16); 0 = none */
  uint64_t m;          /* fp32 exp_avg, updated in place */
  uint64_t v;          /* fp32 exp_avg_sq, updated in place */
  uint64_t vmax;       /* fp32 max_exp_avg_sq (amsgrad) or 0 */
  uint64_t carry;      /* fp32 ZeRO-1 carried average A_{t-1}, rewritten with A_t; or 0 */
  int64_t n;           /* elements */
} zs_adam_seg;
/* p_dtype ZS_BF16_SPLIT (bf16 params; g bf16, or fp32 — ZeRO-3's fp32 accumulation arena — on a
 * set without carry: 28 B/element, and a carry on such a set is ZS_ERR_INVALID; zs_sgdset_create
 * the same): the fp32 master is not stored as such.
 * Its bits u are the bf16 param hi = RNE(u) and the int16 residual lo = u - (hi << 16):
 *   master     = bf16 param read (hi), 8-byte aligned for the vector path
 *   master_out = int16 residual lo, read and rewritten in place
 *   p_out      = bf16 param written (hi of the updated master; may equal master)
 * u = (hi << 16) + sign_extend(lo) exactly, except an exact tie that rounds down to an even hi
 * (residual +0x8000, 1 in 2^17 of uniformly random masters): that master is stored 1 ulp toward
 * zero (lo = 0x7FFF), the bf16 param unchanged.  26 instead of 28 B/element per update. */

typedef struct {
  /* scalars exactly as torch computes them (double on host, rounded to f32 once) */
  float one_minus_beta1;  /* lerp weight 1-beta1 */
  float beta2;
  float one_minus_beta2;
  float neg_step_size;    /* -(lr / (1 - beta1^t)) */
  float bc2_sqrt;         /* sqrt(1 - beta2^t) */
  float eps;
  float weight_decay;     /* L2 (Adam) coefficient; 0 = off */
  float decay_mul;        /* AdamW: 1 - lr*wd; 1 = off */
  float grad_div;         /* divide the reduced sum by this (world size) */
  float carry_mul;        /* ZeRO-1: sum += carry_mul * carry (ws-1) */
  int32_t amsgrad;
  int32_t maximize;
} zs_adam_hparams;

/* Fill hp the way torch.optim.Adam/AdamW (non-capturable path) derives its scalars at step t. */
int zs_adam_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                         int decoupled, int amsgrad, int maximize, int64_t step, double grad_div,
                         double carry_mul, zs_adam_hparams* hp);

typedef struct zs_adamset zs_adamset;
/* g_dtype: dtype of every seg's g; p_dtype: ZS_BF16 (fp32 master, optional bf16 p_out) or
 * ZS_BF16_SPLIT (split master, above). All fp32 pointers of a seg must be 16-byte aligned and
 * bf16 / int16 pointers 8-byte aligned for the vector path; other segments take a scalar path. */
int zs_adamset_create(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                      zs_adamset** out);
/* zs_adamset_create with the element type of the moments m and v (additive in ABI v13):
 * state_dtype ZS_F32 is zs_adamset_create itself.  ZS_BF16: m and v point at bf16 arrays (8-byte
 * aligned for the vector path).  One step widens the stored moments to fp32 (exact), runs the
 * fp32 update unchanged, updates the parameter from the unrounded fp32 moments and stores them
 * rounded to nearest even (a NaN stays a NaN, overflow rounds to Inf): 18 instead of 26 B/element
 * over a split master, 20 instead of 28 otherwise.  bf16 keeps 8 significant bits, so a decay
 * v <- beta * v moves every stored value only while 1 - beta >= 2^-8: callers keep both betas at or
 * below 0.99609375 (the library does not check).  A segment with vmax or carry is ZS_ERR_INVALID
 * on such a set, and so is a run of it with hp->amsgrad set.  set_grads, stats, the sum-of-squares
 * pass and the clipped run take such a set as any other. */
int zs_adamset_create_ex(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                         int state_dtype, zs_adamset** out);
int zs_adamset_run(const zs_adamset* as, const zs_adam_hparams* hp, uintptr_t stream);
/* Re-point the set's gradients (ABI v12): g[i] (0 = zero gradient) replaces the g of the i-th
 * segment given to zs_adamset_create (n = that count).  The new pointers travel in the arguments
 * of a small patch kernel enqueued on `stream`, which rewrites the device tables in stream order:
 * no upload, no host synchronisation, nothing launched when every pointer is unchanged.  Runs of
 * the set enqueued on `stream` afterwards read the new gradients; the set must not run on another
 * stream concurrently.  A segment with a vector part needs its new g aligned as at creation (8 B
 * bf16, 16 B fp32), else ZS_ERR_INVALID and nothing is changed.  The reference's `step()` reads
 * `p.grad` wherever backward left it after `zero_grad()` (zero2.py:94-120, 138-139): at world
 * size 1 the update reads those fresh gradient tensors in place instead of copying them into an
 * arena first. */
int zs_adamset_set_grads(zs_adamset* as, int64_t n, const uint64_t* g, uintptr_t stream);
int zs_adamset_destroy(zs_adamset* as);
/* total elements covered by the set and algorithmic HBM bytes one run moves (with the gradients
 * bound now) */
int zs_adamset_stats(const zs_adamset* as, int64_t* elems, int64_t* bytes);

/* Global gradient-norm clipping fused into the update (additive in ABI v13).  Together these
 * replace torch.nn.utils.clip_grad_norm_(params, max_norm) between zero2.py's reduce-scatter
 * (zero2.py:94-113) and its optimizer.step() (zero2.py:120): the reduced gradient is read once
 * more, never rewritten, and the host never waits for the norm.  All buffers are the caller's.
 *
 * zs_adamset_sqnorm_partials: how many double partials zs_adamset_grad_sqnorm writes for this set;
 * fixed when the set is created (it depends on the segment table alone, not on zs_tune or the
 * device), 0 for an empty set. */
int zs_adamset_sqnorm_partials(const zs_adamset* as, int64_t* n);
/* The squares of the gradients the set is bound to now (so after zs_adamset_set_grads), summed
 * into partials[0 .. n): the `torch.linalg.vector_norm(g, 2)` pass of clip_grad_norm_ over every
 * segment of the set, on the raw reduced sums (before the division by the world size).  A segment
 * with g == 0 contributes nothing and is not read.  fp32 only inside one lane's 8 (16: split
 * master) terms of a chunk, double above, no atomics: the partials have the same bits on every
 * run.  Every partial is written (plain stores); nothing else is. */
int zs_adamset_grad_sqnorm(const zs_adamset* as, double* partials, uintptr_t stream);
/* *sumsq = (float) of the double sum of partials[0 .. n), added in a fixed order by one workgroup
 * (n == 0: 0).  The partials of several sets laid side by side reduce in one call; at world size
 * > 1 the caller all-reduces the one float before zs_clip_coef. */
int zs_sqnorm_reduce(const double* partials, int64_t n, float* sumsq, uintptr_t stream);
/* out2[0] = norm = (float)(sqrt((double)*sumsq) / grad_div): the L2 norm of the averaged gradient
 * (clip_grad_norm_'s return value); out2[1] = coef = min(1, (float)max_norm / (norm + 1e-6f)) in
 * fp32 (its clip_coef_clamped, error_if_nonfinite=False: a NaN norm gives a NaN coefficient, a
 * zero norm 1; max_norm = infinity reports the norm and clips nothing).  ZS_ERR_INVALID for
 * max_norm < 0 or NaN, or grad_div <= 0. */
int zs_clip_coef(const float* sumsq, double grad_div, double max_norm, float* out2,
                 uintptr_t stream);
/* zs_adamset_run with every averaged gradient multiplied by *coef (device memory, read when the
 * kernel runs: one uniform load per workgroup) right after the division by grad_div and before
 * maximize and weight decay — clip_grad_norm_'s `g.mul_(clip_coef_clamped)` without rewriting g.
 * ZS_ERR_INVALID, nothing launched, for a set with the ZeRO-1 carry (what the carry should hold
 * under clipping is undecided). */
int zs_adamset_run_clipped(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef,
                           uintptr_t stream);

/* Stochastic rounding of bf16 moments (additive in ABI v13).  zs_adamset_run_sr is zs_adamset_run
 * (coef == NULL) or zs_adamset_run_clipped (coef: the device scalar) of a set with ZS_BF16 state,
 * except that m and v are stored rounded stochastically: for a finite fp32 value with bits u and 16
 * random bits r the stored code is (u + r) >> 16 — away from zero with probability
 * low16(u) / 65536, exact when low16(u) == 0, Inf past the largest finite value, never a NaN; a
 * NaN or Inf is stored as zs_adamset_run stores it.  The rounding is unbiased, so a decay
 * v <- beta * v moves every stored value in expectation at any beta: the bound on the betas that
 * zs_adamset_create_ex states does not apply to these runs.  The parameter is computed from the
 * unrounded fp32 moments as before, and the bytes moved are the same.
 *
 * The random bits come from no state and no memory.  With
 *   lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 * over uint32, element e draws
 *   r = lowbias32(lo32(e) ^ key0 ^ (hi32(e) * 0x9E3779B9)) ^ key1;
 * m rounds with r & 0xFFFF and v with r >> 16.  e = (the element's address in m - m_base) / 2: its
 * index in the caller's moment array, so the bits do not depend on how the array is cut into
 * segments, on alignment, on zs_tune or on where the array lies.  m_base is never dereferenced.
 * zs_sr_keys derives the keys of one launch from a 64-bit seed and the step count t of the
 * segments (torch's state['step'] after the step):
 *   key0 = lowbias32(lo32(t) ^ lo32(seed));
 *   key1 = lowbias32((key0 ^ hi32(seed) ^ hi32(t)) + 0x9E3779B9).
 * ZS_ERR_INVALID, nothing launched: a set without ZS_BF16 state (or an SGD set), hp->amsgrad, a
 * segment whose m lies below m_base or at an odd byte distance from it.
 * zs_sr_keys and zs_sr_bits are host functions (no device is touched): the definition above, for
 * callers and tests that restate the rounding. */
int zs_adamset_run_sr(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef,
                      uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream);
int zs_sr_keys(uint64_t seed, uint64_t step, uint32_t* key0, uint32_t* key1);
int zs_sr_bits(uint64_t e, uint32_t key0, uint32_t key1, uint32_t* r);

/* The guarded update: a step whose gradient norm is not finite is skipped on the device (additive
 * in ABI v13).  The host never learns of it and never waits.
 *
 * zs_clip_coef_guarded is zs_clip_coef plus the decision: out2[0] = the norm as computed; if that
 * norm is NaN or +-inf (some gradient element is not finite, or the sum of squares left fp32's
 * range), out2[1] = the quiet NaN 0x7FC00000 and *skipped (a uint64_t in device memory) is
 * incremented, by a plain load, add and store in stream order; otherwise out2[1] has zs_clip_coef's
 * bits, which are then never a NaN (max_norm is finite or inf and >= 0, norm + 1e-6f > 0).
 * ZS_ERR_INVALID as zs_clip_coef, and for skipped == NULL.
 *
 * zs_adamset_run_guarded / zs_adamset_run_sr_guarded are zs_adamset_run_clipped / zs_adamset_run_sr
 * with a coefficient (required here), except that a NaN *coef ends every workgroup right after the
 * coefficient's uniform load: no parameter, master residual, moment or vmax element is read or
 * written.  With any other coefficient every output has the unguarded run's bits.
 * ZS_ERR_INVALID, nothing launched: what the unguarded run refuses, coef == NULL, a set with the
 * ZeRO-1 carry, an SGD set (its "first step" is the host's count, which a skipped step would
 * advance). */
int zs_clip_coef_guarded(const float* sumsq, double grad_div, double max_norm, float* out2,
                         uint64_t* skipped, uintptr_t stream);
int zs_adamset_run_guarded(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef,
                           uintptr_t stream);
int zs_adamset_run_sr_guarded(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef,
                              uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream);

/* Per-parameter gradient norms from the clipping pass (additive in ABI v13): the same read-only
 * pass with its partials keyed by segment, so that the per-segment sums of squares, and from them
 * the global one, come out of one read of the gradients.
 *
 * zs_adamset_sqnorm_seg_partials: *n = the double partials ("slots")
 * zs_adamset_grad_sqnorm_segs writes for this set; seg_off[0 .. nseg] (nseg = the segments given to
 * *_create, in that order; the caller's array of nseg + 1) = where each segment's slots start,
 * seg_off[nseg] == *n.  A segment's slots are those of its vector part (the 4-aligned prefix of an
 * aligned segment, in chunks of 2,048 elements, 4,096 for ZS_BF16_SPLIT / ZS_BF16_SR) followed by
 * those of its scalar part (the tail of up to 3 elements, or a whole unaligned segment, in chunks
 * of 256): min(chunks, 128) for a vector part, min(chunks, 16) for a scalar part, none for an
 * empty segment.  The count depends on that segment's length, its alignment class and the set's
 * dtypes alone — not on the device, zs_tune or the other segments.  (A set of 326 segments has at
 * most 326 * 144 slots: 376 KB.)
 *
 * zs_adamset_grad_sqnorm_segs: zs_adamset_grad_sqnorm's pass — the gradients bound now, the same
 * loads, fp32 only inside one lane's terms of one chunk, double above, plain stores, no atomics —
 * where slot j of a part with s slots is the sum over chunks j, j + s, ... of that part.  A
 * segment with g == 0 is not read and its slots are +0.0.  Every slot is written; nothing else
 * is.  A slot's bits depend on its own segment alone.  Works on every kind of set.
 *
 * zs_sqnorm_reduce_params: out[i] = (float) of the double sum of parameter i's slots, for i in
 * [0, n_params).  row_ptr (n_params + 1), slot_lo and slot_n are device arrays: parameter i owns
 * the ranges r in [row_ptr[i], row_ptr[i + 1]), range r being partials[slot_lo[r] .. slot_lo[r] +
 * slot_n[r]) — several when the parameter is cut across sets.  One workgroup per parameter adds
 * its ranges in that order, thread t taking slots t, t + 256, ... of each range into one running
 * double; then the 64 lanes of each wave by shuffles (offsets 32, 16, .. 1) and the four waves in
 * order.  A parameter without a range gets +0.0.
 *
 * zs_param_norms: norms[i] = (float)(sqrt((double)sumsq_vec[i]) / grad_div) for i in [0, n):
 * zs_clip_coef's norm, per element (no contraction).
 *
 * ZS_ERR_INVALID, nothing launched: a NULL set, n, seg_off, row_ptr or out; NULL partials for a
 * set that has slots; n_params or n < 0; sumsq_vec or norms NULL with n > 0; grad_div <= 0. */
int zs_adamset_sqnorm_seg_partials(const zs_adamset* as, int64_t* n, int64_t* seg_off);
int zs_adamset_grad_sqnorm_segs(const zs_adamset* as, double* partials, uintptr_t stream);
int zs_sqnorm_reduce_params(const double* partials, const int64_t* row_ptr, const int64_t* slot_lo,
                            const int64_t* slot_n, int64_t n_params, float* out,
                            uintptr_t stream);
int zs_param_norms(const float* sumsq_vec, int64_t n, double grad_div, float* norms,
                   uintptr_t stream);

/* Master-free bf16 parameters (additive in ABI v13).  A set made by zs_adamset_create_ex with
 * p_dtype ZS_BF16_SR keeps no master and no residual: a seg's `master` is the bf16 param (read),
 * `p_out` the same address (written), master_out = vmax = carry = 0; g is bf16 or fp32; anything
 * else, and zs_sgdset_create, is ZS_ERR_INVALID.  One element: p, g, m and v as stored are widened
 * to fp32 (exact), zs_adamset_run's fp32 rule runs unchanged (clip coefficient, maximize, coupled
 * and decoupled weight decay), m and v are stored as the set's state says (fp32; ZS_BF16 rounded to
 * nearest, or stochastically with the draws of zs_adamset_run_sr after
 * zs_adamset_set_state_rounding(as, 1)), and the new parameter with bits u is stored as the bf16
 * code (u + r16p) >> 16 (a NaN as zs_adamset_run stores it): unbiased, so updates below half a bf16
 * ulp move the parameter in expectation instead of being lost.  14 B/element with bf16 moments and
 * gradients (18 with the split master), 22 with fp32 moments (26).
 *   r16p = zs_sr_bits(e, pkey0, pkey1) & 0xFFFF, (pkey0, pkey1) = zs_sr_pkeys(key0, key1):
 *   pkey0 = lowbias32(key0 ^ 0x85EBCA6B), pkey1 = lowbias32(key1 + 0xC2B2AE35)
 * — independent of the m and v halves of zs_sr_bits(e, key0, key1).  e = (the element's address in
 * m - m_base) / the element size of m (4 or 2).
 * zs_adamset_run_psr is the only way to run such a set: coef NULL = unclipped, otherwise as
 * zs_adamset_run_clipped, and with guard != 0 as zs_adamset_run_guarded (a NaN coefficient: nothing
 * is read or written; the step's keys are consumed all the same).  ZS_ERR_INVALID, nothing
 * launched: any other set, guard without coef, hp->amsgrad, a segment whose m lies below m_base or
 * not a whole number of elements from it.  zs_adamset_run, _run_clipped, _run_guarded, _run_sr and
 * _run_sr_guarded return ZS_ERR_INVALID on a ZS_BF16_SR set.  zs_adamset_set_grads,
 * zs_adamset_sqnorm_partials, zs_adamset_grad_sqnorm, zs_adamset_stats and zs_adamset_destroy work
 * on it.  zs_sr_pkeys is a host function. */
int zs_adamset_run_psr(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef, int guard,
                       uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream);
int zs_adamset_set_state_rounding(zs_adamset* as, int stochastic);
int zs_sr_pkeys(uint32_t key0, uint32_t key1, uint32_t* pkey0, uint32_t* pkey1);

/* Sharded EMA of the master weights, fused into the Adam update (additive in ABI v13).  Over a set
 * made by zs_adamset_create / _create_ex with fp32 state and any master storage but ZS_BF16_SR,
 * whose segments' `vmax` column points at an fp32 EMA array (the stream slot amsgrad uses, so the
 * two exclude each other): zs_adamset_run's update runs unchanged (coef NULL), or
 * zs_adamset_run_clipped's (coef given), or zs_adamset_run_guarded's (coef and guard != 0: a NaN
 * coefficient, nothing is read or written, the EMA included).  Then, per element,
 *   ema = lerp(ema, master_after, ema_weight)
 * with ATen's lerp -- fma(w, end - start, start) for w < 0.5, fma(w - 1, end - start, end)
 * otherwise -- and master_after the fp32 master as this call stored it: the fp32 parameter or master,
 * or for ZS_BF16_SPLIT (hi << 16) + sext(lo) of the two words just written.  ema_weight is
 * 1 - decay, rounded to fp32 by the caller.  A segment without a gradient runs like any other (its
 * gradient reads as zero), as in zs_adamset_run.  Bytes per element: those of the amsgrad run.
 * ZS_ERR_INVALID, nothing launched: a NULL set or hparams; a set made by zs_sgdset_create; ZS_BF16
 * state; a ZS_BF16_SR set; a set with the carry; a non-empty set without the vmax column;
 * hp->amsgrad; guard without coef; an ema_weight that is NaN or outside [0, 1]. */
int zs_adamset_run_ema(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef, int guard,
                       float ema_weight, uintptr_t stream);

/* Per-parameter update and weight norms out of the fused Adam update (additive in ABI v13).  Over a
 * set made by zs_adamset_create / _create_ex with fp32 state, any master storage but ZS_BF16_SR, no
 * carry and no vmax column, zs_adamset_run_stats runs zs_adamset_run's update unchanged (coef NULL),
 * zs_adamset_run_clipped's (coef given) or zs_adamset_run_guarded's (coef and guard != 0), with the
 * same bits in every parameter, residual and moment, and sums per element, in the same kernel,
 *   d = p1 - p0 (one fp32 subtraction),  sum d * d  and  sum p1 * p1,
 * p0 the fp32 master as the update loaded it and p1 the fp32 master as it stored it (ZS_BF16_SPLIT:
 * (hi << 16) + sext(lo) of the words read / just written).  fp32 (fmaf) covers one lane's terms of
 * one chunk -- 16 for ZS_BF16_SPLIT, 8 otherwise, 1 in the scalar part --, double the wave's 64 lanes
 * (shuffles, offsets 32 .. 1); each wave stores its pair with plain stores, no atomics.
 *
 * zs_adamset_update_norm_slots: *n = the slots per plane; seg_off[0 .. nseg] = where each input
 * segment's slots start, seg_off[nseg] == *n (the shape of zs_adamset_sqnorm_seg_partials).  A
 * segment's slots: 4 per chunk of its vector part (chunks of 2,048 elements, 4,096 for
 * ZS_BF16_SPLIT), one per wave, chunk-major, then 4 per 256-element chunk of its scalar part; none
 * for an empty segment.  A slot's value depends on its own chunk alone: not on the grid, zs_tune,
 * the device or the other segments.
 *
 * partials: two planes of *n doubles, sum d^2 first, sum p1^2 second (16 B per 512 or 1,024
 * elements: 1.5 G elements of a split-master set take 2 * 24 MB).  Every slot of both planes is
 * written by a run that is not skipped (a wave without an element in range stores +0.0); a guarded
 * run with a NaN coefficient writes none.  A segment with g == 0 runs like any other.
 * zs_sqnorm_reduce_params sums a plane's slots per parameter.
 *
 * zs_update_norms: sums3 = [sum d^2 | sum p1^2 | touched], n_params floats each.  For parameter i
 * with touched[i] != 0, and *coef not NaN where coef is given:
 *   update_norms[i] = (float)sqrt((double)sums3[i]),
 *   weight_norms[i] = (float)sqrt((double)sums3[n_params + i]);
 * otherwise update_norms[i] = +0.0 and weight_norms[i] is left as it is.
 *
 * ZS_ERR_INVALID, nothing launched: a NULL set, hparams, n or seg_off; a set made by
 * zs_sgdset_create; ZS_BF16 state; a ZS_BF16_SR set; a set with the carry or the vmax column;
 * hp->amsgrad; guard without coef; NULL partials for a set that has slots; n_params < 0; sums3,
 * update_norms or weight_norms NULL with n_params > 0. */
int zs_adamset_update_norm_slots(const zs_adamset* as, int64_t* n, int64_t* seg_off);
int zs_adamset_run_stats(const zs_adamset* as, const zs_adam_hparams* hp, const float* coef,
                         int guard, double* partials, uintptr_t stream);
int zs_update_norms(const float* sums3, int64_t n_params, const float* coef, float* update_norms,
                    float* weight_norms, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused SGD (momentum, Nesterov), additive in ABI v13.  Replaces torch.optim.SGD.step on the    */
/* owned shard where the reference's ShardedOptimizer wraps an SGD (zero1.py:88, zero2.py:120,  */
/* zero3.py:161; the optimizer of DDP/ddp.py:86,125; math of torch/optim/sgd.py                 */
/* _single_tensor_sgd) plus the grad averaging, through the Adam's tables and kernels' shape.   */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  /* doubles on the host, rounded to f32 once */
  float neg_lr;              /* -lr */
  float momentum;
  float one_minus_dampening; /* 1 - dampening */
  float weight_decay;        /* L2 coefficient; 0 = off */
  float grad_div;            /* divide the reduced sum by this (world size) */
  float carry_mul;           /* ZeRO-1: sum += carry_mul * carry (ws-1) */
  int32_t nesterov;
  int32_t maximize;
  int32_t first;             /* the segments' first step: the momentum buffer becomes the gradient
                                (sgd.py: `buf = torch.clone(grad)`), its old contents are not read
                                into the result */
} zs_sgd_hparams;

/* Fill hp from torch.optim.SGD's group scalars.  ZS_ERR_INVALID for what SGD.__init__ refuses
 * (lr, momentum or weight_decay < 0; nesterov with momentum <= 0 or dampening != 0) and for
 * grad_div <= 0. */
int zs_sgd_hparams_init(double lr, double momentum, double dampening, double weight_decay,
                        int nesterov, int maximize, int first, double grad_div, double carry_mul,
                        zs_sgd_hparams* hp);
/* A zs_adamset whose update is SGD's: segs, g_dtype, p_dtype, alignment and the vector / scalar
 * split exactly as zs_adamset_create, with m the fp32 momentum_buffer (updated in place), set on
 * all segments or on none (a set for momentum == 0, which touches no state array), and v == vmax
 * == 0 (ZS_ERR_INVALID otherwise).  zs_adamset_set_grads, zs_adamset_sqnorm_partials,
 * zs_adamset_grad_sqnorm, zs_adamset_destroy and zs_adamset_stats (gradient + parameter read and
 * write + buffer read and write if present) work on it unchanged; zs_adamset_run and
 * zs_adamset_run_clipped return ZS_ERR_INVALID on it, as zs_sgdset_run does on an Adam set. */
int zs_sgdset_create(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                     zs_adamset** out);
/* One SGD step over the set, per element (fp32, only the written fma fused):
 *   g = (sum [+ carry_mul * carry]) / grad_div;  [carry = g];  [g *= *coef];  [g = -g]
 *   [g = fma(wd, p, g)];  buf = first ? g : fma(1 - dampening, g, buf * momentum)
 *   g = nesterov ? fma(momentum, buf, g) : buf;  p = fma(-lr, g, p)
 * the buffer lines only with momentum != 0 (a set with buffers run with momentum == 0 leaves them
 * untouched, as torch never creates them then).  coef: NULL = unclipped, else the device scalar of
 * zs_clip_coef as in zs_adamset_run_clipped.  ZS_ERR_INVALID, nothing launched: an Adam set;
 * momentum != 0 on a set without buffers; coef on a set with the ZeRO-1 carry; nesterov with
 * momentum <= 0 or dampening != 0; negative lr, momentum or weight_decay. */
int zs_sgdset_run(const zs_adamset* as, const zs_sgd_hparams* hp, const float* coef,
                  uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused Lion (Chen et al. 2023, arXiv:2302.06675), additive in ABI v13.  The update of          */
/* zero_amd.optim.Lion on the owned shard: one moment (exp_avg), no bias correction, through the */
/* Adam's tables and kernels' shape.  14 B/element over the split master with bf16 momentum and  */
/* bf16 gradients, 18 with fp32 momentum (SGD-with-momentum's traffic; Adam's: 26, or 18 with    */
/* bf16 moments).                                                                                 */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  /* doubles on the host, rounded to f32 once */
  float neg_lr;           /* -lr */
  float beta1;            /* the update's interpolation: c = beta1 * m + (1 - beta1) * g */
  float one_minus_beta1;
  float beta2;            /* the momentum's decay: m = beta2 * m + (1 - beta2) * g */
  float one_minus_beta2;
  float decay_mul;        /* 1 - lr * weight_decay (decoupled); 1 when weight_decay == 0 */
  float grad_div;         /* divide the reduced sum by this (world size) */
  float carry_mul;        /* ZeRO-1: sum += carry_mul * carry (ws-1) */
  int32_t maximize;
} zs_lion_hparams;

/* Fill hp from a Lion param group's scalars.  ZS_ERR_INVALID for what zero_amd.optim.Lion refuses
 * (lr < 0, a beta outside [0, 1), weight_decay < 0), for grad_div <= 0 and for a NULL hp. */
int zs_lion_hparams_init(double lr, double beta1, double beta2, double weight_decay, int maximize,
                         double grad_div, double carry_mul, zs_lion_hparams* hp);
/* A zs_adamset whose update is Lion's: segs, g_dtype, p_dtype, alignment and the vector / scalar
 * split exactly as zs_adamset_create_ex, with m = exp_avg (updated in place) set on every
 * non-empty segment and v == vmax == 0.  state_dtype is the element type of m: ZS_F32, or ZS_BF16
 * (m 8-byte aligned for the vector part; rounded to nearest even when stored, or stochastically
 * after zs_adamset_set_state_rounding(as, 1)); a 16-bit v stream does not exist.
 * ZS_ERR_INVALID: a NULL out or table, n < 0, a bad g_dtype; p_dtype other than ZS_BF16 or
 * ZS_BF16_SPLIT (ZS_BF16_SR: Lion has no master-free instances); state_dtype other than ZS_F32 or
 * ZS_BF16; a non-empty segment without master or m, or with v or vmax; a split master without
 * master_out and p_out; a carry with ZS_BF16 state, or with fp32 gradients over the split master,
 * or on some segments only.  zs_adamset_set_grads, zs_adamset_sqnorm_partials,
 * zs_adamset_grad_sqnorm, zs_adamset_sqnorm_seg_partials, zs_adamset_grad_sqnorm_segs,
 * zs_adamset_destroy and zs_adamset_stats (gradient + parameter read and write + momentum read and
 * write) work on it unchanged; every zs_adamset_run* and zs_sgdset_run return ZS_ERR_INVALID on
 * it, as zs_lionset_run does on their sets. */
int zs_lionset_create(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                      int state_dtype, zs_adamset** out);
/* One Lion step over the set, per element (fp32, only the written fma fused):
 *   g = (sum [+ carry_mul * carry]) / grad_div;  [carry = g];  [g *= *coef];  [g = -g]
 *   p = p * decay_mul;  c = fma(1 - beta1, g, m * beta1);  u = (c > 0) - (c < 0)
 *   p = fma(-lr, u, p);  m = fma(1 - beta2, g, m * beta2)
 * u is torch.sign's value: +-0 gives +0, and so does a NaN.  A segment without a gradient reads
 * g = 0 and runs like any other.  m as stored is widened before the rule (exact) and narrowed
 * after it; the stochastic store of element e takes r16 = zs_sr_bits(e, key0, key1) & 0xFFFF, the
 * draw zs_adamset_run_sr gives exp_avg, e = (the element's address in m - m_base) / 2, and the
 * keys are the caller's zs_sr_keys(seed, t), t the parameter's step count after the step.  m_base,
 * key0 and key1 are read only after zs_adamset_set_state_rounding(as, 1).
 * coef: NULL = unclipped, else the device scalar of zs_clip_coef as in zs_adamset_run_clipped;
 * guard != 0 as zs_adamset_run_guarded: a NaN coefficient ends every workgroup after the uniform
 * load, nothing is read or written.  ZS_ERR_INVALID, nothing launched: a NULL set or hparams; a
 * set not made by zs_lionset_create; guard without coef; coef on a set with the ZeRO-1 carry; a
 * negative lr, a beta outside [0, 1] or grad_div <= 0 in a struct filled by hand; with stochastic
 * rounding, a segment whose m lies below m_base or at an odd byte distance from it. */
int zs_lionset_run(const zs_adamset* as, const zs_lion_hparams* hp, const float* coef, int guard,
                   uint64_t m_base, uint32_t key0, uint32_t key1, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused Schedule-Free AdamW (Defazio et al. 2024, arXiv:2405.15682), additive in ABI v13.  The  */
/* update of zero_amd.optim.ScheduleFreeAdamW on the owned shard through the Adam's tables and   */
/* kernels' shape: the master holds y, field m of a segment is z, v is exp_avg_sq.  Adam's        */
/* streams and bytes (26 B/element over the split master with bf16 gradients); a second kernel   */
/* swaps the model parameters between y (training) and x (evaluation).                           */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  /* doubles on the host, rounded to f32 once */
  float beta2;
  float one_minus_beta2;
  float bc2;              /* 1 - beta2^step */
  float eps;
  float weight_decay;     /* decoupled, on y */
  float c;                /* this step's averaging weight w_t / sum of w, in [0, 1] */
  float a;                /* lr_t * (beta1 * (1 - c) - 1): y's step */
  float lr_t;             /* the step's learning rate, after warm-up: z's step */
  float grad_div;         /* divide the reduced sum by this (world size) */
  float carry_mul;        /* ZeRO-1: sum += carry_mul * carry (ws-1) */
  int32_t maximize;
} zs_sfadam_hparams;

/* Fill hp from the scalars of one step of a ScheduleFreeAdamW param group: lr is the step's
 * learning rate after warm-up (lr_t), step the group's count after the increment, c the averaging
 * weight the host formed; a, bc2 and the rest are derived in double.  ZS_ERR_INVALID for what the
 * class refuses (lr < 0, beta1 outside (0, 1) -- 0 included: 1 - 1/beta1 is undefined --, beta2
 * outside [0, 1), eps < 0, weight_decay < 0), for step < 1, c outside [0, 1], grad_div <= 0 and a
 * NULL hp. */
int zs_sfadam_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                           int64_t step, double c, int maximize, double grad_div, double carry_mul,
                           zs_sfadam_hparams* hp);
/* A zs_adamset whose update is Schedule-Free AdamW's: segs, g_dtype, p_dtype, alignment and the
 * vector / scalar split exactly as zs_adamset_create, with m = z and v = exp_avg_sq (fp32, updated
 * in place) set on every non-empty segment and vmax == 0.  ZS_ERR_INVALID: a NULL out or table,
 * n < 0, a bad g_dtype; p_dtype other than ZS_BF16 or ZS_BF16_SPLIT; a non-empty segment without
 * master, m or v, or with vmax; a split master without master_out and p_out; a carry with fp32
 * gradients over the split master, or on some segments only.  zs_adamset_set_grads, the
 * sum-of-squares passes, zs_adamset_destroy and zs_adamset_stats work on it unchanged; every
 * zs_adamset_run*, zs_lionset_run, zs_sgdset_run and zs_lambset_* return ZS_ERR_INVALID on it, as
 * zs_sfadamset_run and zs_sfadamset_swap do on their sets. */
int zs_sfadamset_create(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                        zs_adamset** out);
/* One step over the set, per element (fp32, only the written fma fused; '/' and sqrt IEEE):
 *   g = (sum [+ carry_mul * carry]) / grad_div;  [carry = g];  [g *= *coef];  [g = -g]
 *   v = fma((1 - beta2) * g, g, v * beta2);  d = sqrt(v / bc2) + eps
 *   n = g / d;  [n = fma(weight_decay, y, n)]
 *   y = fma(c, z - y, y) if c < 0.5 else fma(c - 1, z - y, z);  y = fma(a, n, y)
 *   z = fma(-lr_t, n, z)
 * and y is stored as the set's p_dtype stores a master (with its bf16 copy).  A segment without a
 * gradient reads g = 0 and runs like any other.  coef as zs_lionset_run; guard must be 0: the
 * argument is reserved, no guarded instances exist (the host's weight sum would advance over a
 * skipped step).
 * ZS_ERR_INVALID, nothing launched: a NULL set or hparams; a set not made by zs_sfadamset_create;
 * guard != 0; coef on a set with the ZeRO-1 carry; in a struct filled by hand a negative
 * lr_t, eps or weight_decay, beta2 or c outside [0, 1], bc2 outside (0, 1] or grad_div <= 0. */
int zs_sfadamset_run(const zs_adamset* as, const zs_sfadam_hparams* hp, const float* coef,
                     int guard, uintptr_t stream);
/* The model parameters of the set between y and x, per element p <- lerp(p, z, weight) as ATen
 * rounds it (fma(w, z - p, p) for |w| < 0.5, fma(w - 1, z - p, z) otherwise; w = (float)weight):
 * to_eval != 0 with weight = 1 - 1/beta1 gives x, to_eval == 0 with weight = 1 - beta1 gives y back.
 * What is written depends on where a segment's master lives:
 *   ZS_BF16 with p_out (an fp32 master beside a bf16 copy): only p_out -- to_eval stores bf16(x)
 *     and the master keeps y; the way back stores bf16(master) again and reads neither z nor
 *     weight: the round trip is exact;
 *   ZS_BF16 without p_out (fp32 parameters, their own master): the master in place, both ways;
 *   ZS_BF16_SPLIT (the bf16 parameter is the master's high half): the master in place, both ways,
 *     x split into p_out and the residual as the update splits y.
 * In place, the round trip returns y to within a rounding or two of each lerp, not bit for bit.
 * ZS_ERR_INVALID, nothing launched: a NULL set, one not made by zs_sfadamset_create, a weight that
 * is not finite.  An empty set launches nothing. */
int zs_sfadamset_swap(const zs_adamset* as, double weight, int to_eval, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused AdEMAMix (Pagliardini, Ablin, Grangier 2024, arXiv:2409.03137), additive in ABI v13.    */
/* The update of zero_amd.optim.AdEMAMix on the owned shard through Adam's tables and kernels'   */
/* shape: field m of a segment is exp_avg (the fast EMA), v is exp_avg_sq, vmax holds            */
/* exp_avg_slow.  The streams and bytes of Adam with amsgrad (34 B/element over the split master */
/* with bf16 gradients).                                                                         */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  /* doubles on the host, rounded to f32 once */
  float beta1;
  float one_minus_beta1;
  float beta3;            /* the slow EMA's decay at this step (after its warm-up) */
  float one_minus_beta3;
  float beta2;
  float one_minus_beta2;
  float inv_bc1;          /* 1 / (1 - beta1^step) */
  float alpha;            /* the slow EMA's weight at this step (after its warm-up) */
  float bc2_sqrt;         /* sqrt(1 - beta2^step) */
  float eps;
  float neg_lr;
  float decay_mul;        /* 1 - lr*weight_decay (decoupled) */
  float grad_div;         /* divide the reduced sum by this (world size) */
  float carry_mul;        /* ZeRO-1: sum += carry_mul * carry (ws-1) */
  int32_t maximize;
} zs_ademamix_hparams;

/* Fill hp from the scalars of one step of an AdEMAMix param group: step is the parameter's count
 * after the increment, beta3_t and alpha_t what the class's schedulers give at that count (the
 * host runs them: zero_amd.optim.ademamix_schedule); everything else is derived in double.
 * ZS_ERR_INVALID for what the class refuses (lr < 0, a beta outside [0, 1), alpha < 0, eps < 0,
 * weight_decay < 0), for step < 1, grad_div <= 0 and a NULL hp. */
int zs_ademamix_hparams_init(double lr, double beta1, double beta2, double beta3_t, double alpha_t,
                             double eps, double weight_decay, int64_t step, int maximize,
                             double grad_div, double carry_mul, zs_ademamix_hparams* hp);
/* A zs_adamset whose update is AdEMAMix's: segs, g_dtype, p_dtype, alignment and the vector /
 * scalar split exactly as zs_adamset_create, with m = exp_avg, v = exp_avg_sq and vmax =
 * exp_avg_slow (fp32, updated in place) set on every non-empty segment.  ZS_ERR_INVALID: a NULL
 * out or table, n < 0, a bad g_dtype; p_dtype other than ZS_BF16 or ZS_BF16_SPLIT; a non-empty
 * segment without master, m, v or vmax; a split master without master_out and p_out; a carry with
 * fp32 gradients over the split master, or on some segments only.  zs_adamset_set_grads, the
 * sum-of-squares passes, zs_adamset_destroy and zs_adamset_stats work on it unchanged; every
 * zs_adamset_run*, zs_lionset_run, zs_sgdset_run, zs_sfadamset_* and zs_lambset_* return
 * ZS_ERR_INVALID on it, as zs_ademamixset_run does on their sets. */
int zs_ademamixset_create(const zs_adam_seg* segs, int64_t n, int g_dtype, int p_dtype,
                          zs_adamset** out);
/* One step over the set, per element (fp32, only the written fma fused; '/' and sqrt IEEE):
 *   g = (sum [+ carry_mul * carry]) / grad_div;  [carry = g];  [g *= *coef];  [g = -g]
 *   p = p * decay_mul
 *   m = fma(1 - beta1, g, m * beta1);  vmax = fma(1 - beta3, g, vmax * beta3)
 *   v = fma((1 - beta2) * g, g, v * beta2);  den = sqrt(v) / bc2_sqrt + eps
 *   p = fma(neg_lr, fma(alpha, vmax, m * inv_bc1) / den, p)
 * and p is stored as the set's p_dtype stores a master (with its bf16 copy).  A segment without a
 * gradient reads g = 0 and runs like any other.  coef as zs_lionset_run; no guarded instances
 * exist.
 * ZS_ERR_INVALID, nothing launched: a NULL set or hparams; a set not made by
 * zs_ademamixset_create; coef on a set with the ZeRO-1 carry; in a struct filled by hand a
 * positive neg_lr, a beta outside [0, 1], inv_bc1 < 1, bc2_sqrt outside (0, 1], a negative alpha or
 * eps, or grad_div <= 0. */
int zs_ademamixset_run(const zs_adamset* as, const zs_ademamix_hparams* hp, const float* coef,
                       uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused LAMB (You et al. 2020, arXiv:1904.00962), additive in ABI v13.  The update of          */
/* zero_amd.optim.LAMB on the owned shard, over a set made by zs_adamset_create (fp32 moments,  */
/* fp32 or split master, no carry, no vmax), in two stream passes with the per-parameter norms  */
/* between them: no atomics, no host wait, the same bits from run to run.  Over the split       */
/* master with bf16 gradients the passes move 22 and 16 B/element (Adam's one pass: 26).        */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  /* doubles on the host, rounded to f32 once */
  float one_minus_beta1;
  float beta2;
  float one_minus_beta2;
  float bc1;          /* 1 - beta1^t; 1 without bias correction */
  float bc2_sqrt;     /* sqrt(1 - beta2^t); 1 without bias correction */
  float eps;
  float weight_decay; /* decoupled, inside the trust ratio: u = fma(wd, p, u); 0 = off */
  float grad_div;     /* divide the reduced sum by this (world size) */
  int32_t maximize;
} zs_lamb_hparams;

/* Fill hp from a LAMB param group's scalars at step count `step` (after the increment, >= 1); the
 * learning rate is not part of it (zs_lamb_finish takes it per parameter).  ZS_ERR_INVALID for what
 * zero_amd.optim.LAMB refuses (a beta outside [0, 1), eps < 0, weight_decay < 0), for step < 1,
 * grad_div <= 0 and a NULL hp. */
int zs_lamb_hparams_init(double beta1, double beta2, double eps, double weight_decay,
                         int bias_correction, int maximize, int64_t step, double grad_div,
                         zs_lamb_hparams* hp);
/* Pass L1.  Per element of every segment that has a gradient (fp32, only the written fma fused):
 *   g = sum / grad_div;  [g *= *coef];  [g = -g]
 *   m = lerp(m, g, 1 - beta1);  v = fma((1 - beta2) * g, g, v * beta2)      (as zs_adamset_run)
 *   u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps);  [u = fma(wd, p, u)]
 * m and v are stored, the parameter is not; accu = fma(u, u, accu) and accw = fma(p, p, accw) (p the
 * fp32 master as loaded) go through zs_adamset_run_stats's partials: the same slots
 * (zs_adamset_update_norm_slots), plane 0 = sum u^2, plane 1 = sum p^2, every slot written.  A
 * segment with g == 0 is not part of the step: nothing of it is read or written, its slots get
 * +0.0.  coef: NULL, or the device scalar of zs_clip_coef.  ZS_ERR_INVALID, nothing launched: a NULL
 * set or hparams; a set made by zs_sgdset_create, zs_lionset_create or zs_adafactorset_create;
 * ZS_BF16 state; a ZS_BF16_SR set; the carry or the vmax column; NULL partials for a set that has
 * slots; bc1 or bc2_sqrt <= 0, eps or weight_decay < 0, grad_div <= 0 in a struct filled by hand. */
int zs_lambset_run_moments(const zs_adamset* as, const zs_lamb_hparams* hp, const float* coef,
                           double* partials, uintptr_t stream);
/* Between the passes, per parameter i of sums3 = [sum u^2 | sum p^2 | touched], n_params floats
 * each (zs_sqnorm_reduce_params over the two planes; summed over the ranks where a parameter is cut):
 *   un = (float)sqrt((double)sums3[i]),  wn = (float)sqrt((double)sums3[n_params + i])
 *   r  = (wn == 0 || un == 0) ? 1 : wn / un;   neg_s[i] = -(lr[i] * r)
 * norms2 = [wn | un], ratios[i] = r.  A NaN norm gives a NaN ratio.  touched[i] == 0: wn = un = +0.0
 * and r = 1.  All pointers are device memory.  ZS_ERR_INVALID: n_params < 0, or a NULL pointer with
 * n_params > 0. */
int zs_lamb_finish(const float* sums3, int64_t n_params, const float* lr, float* norms2,
                   float* ratios, float* neg_s, uintptr_t stream);
/* seg_param[0 .. n) (host memory): the parameter index of each input segment of the set, n the
 * number it was created with.  Uploaded as one index per table entry; binding the same indices
 * again does nothing, other indices replace the table (which waits for the device).
 * ZS_ERR_INVALID: a NULL set, n other than the set's segments, a NULL table, a negative index. */
int zs_lambset_bind_params(zs_adamset* as, int64_t n, const int32_t* seg_param);
/* Pass L2, after zs_lamb_finish in stream order.  Per element of every segment that has a gradient:
 *   u as in L1 from m and v as L1 stored them (the same operations: the same bits)
 *   p = fma(neg_s[parameter of the segment], u, p)
 * stored as zs_adamset_run stores the master (ZS_BF16_SPLIT: the bf16 parameter and the residual;
 * ZS_BF16: master_out and / or p_out).  hp is L1's.  neg_s: n_params device floats.
 * ZS_ERR_INVALID, nothing launched: what zs_lambset_run_moments refuses of the set and the struct;
 * a non-empty set without bound parameters; a NULL neg_s; a bound index >= n_params. */
int zs_lambset_run_apply(const zs_adamset* as, const zs_lamb_hparams* hp, const float* neg_s,
                         int64_t n_params, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused Adafactor (Shazeer & Stern 2018, arXiv:1804.04235; torch.optim.Adafactor's rule),      */
/* additive in ABI v13.  The second moment of an R x C matrix is a row vector and a column      */
/* vector (R + C floats), of a 1-D parameter one float per element.  A step is three passes     */
/* over the set (statistics, update norm, apply) with small reduce kernels between them; every  */
/* scalar stays on the device, nothing is atomic and the bits repeat from run to run.  With     */
/* bf16 gradients over the split master the passes move 6, 2 and 10 B/element.                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t g;          /* reduced gradient sum, R * C elements of g_dtype (required) */
  uint64_t master;     /* as zs_adam_seg: the fp32 master, or (ZS_BF16_SPLIT) the bf16 param read */
  uint64_t master_out; /* the fp32 master again (updated in place), or (ZS_BF16_SPLIT) the int16
                          residual, read and rewritten */
  uint64_t p_out;      /* optional bf16 copy of the updated param; (ZS_BF16_SPLIT) the bf16 param
                          written, required */
  uint64_t row_var;    /* fp32, R elements, updated in place; a 1-D entry: variance, C elements */
  uint64_t col_var;    /* fp32, C elements, updated in place; 0 marks a 1-D entry (R must be 1) */
  int64_t R, C;        /* rows and columns: row i starts at element i * C */
  int64_t param;       /* the caller's index of the entry's parameter: the entries of one parameter
                          (the matrices of a batch) are adjacent, and sum p^2 / sum u^2 run over all
                          of them */
} zs_adafactor_seg;

typedef struct {
  /* the group's scalars as doubles; a run rounds what it derives from them to f32 once */
  double lr;
  double beta2_decay;
  double eps1;         /* resolved: eps=(None, .) is fp32's epsilon, 2^-23 */
  double eps2;
  double d;
  double weight_decay;
  double grad_div;     /* divide the reduced sum by this (world size) */
  int32_t maximize;
  int32_t reserved;
} zs_adafactor_hparams;

/* Fill hp from a torch.optim.Adafactor param group.  has_eps1 == 0: eps1 is fp32's epsilon (the
 * arithmetic is fp32 whatever the parameter dtype).  ZS_ERR_INVALID unless lr > 0, beta2_decay <= 0,
 * eps1 >= 0 when given, eps2 > 0, d >= 1, weight_decay >= 0, grad_div > 0 and hp is not NULL. */
int zs_adafactor_hparams_init(double lr, double beta2_decay, int has_eps1, double eps1, double eps2,
                              double d, double weight_decay, int maximize, double grad_div,
                              zs_adafactor_hparams* hp);
typedef struct zs_adafactorset zs_adafactorset;
/* g_dtype ZS_F32 or ZS_BF16; p_dtype ZS_BF16 (fp32 master in place, optional bf16 p_out) or
 * ZS_BF16_SPLIT.  A matrix entry with R > 1, C a multiple of the 16-byte gradient vector (8 bf16,
 * 4 fp32) and aligned pointers takes 16-byte accesses; any other entry the element-wise path with
 * the same arithmetic and reduction order.  The set owns its scratch (per-tile partial sums, row
 * factors, per-parameter scalars).  Every check comes before any allocation or upload. */
int zs_adafactorset_create(const zs_adafactor_seg* segs, int64_t n, int g_dtype, int p_dtype,
                           zs_adafactorset** out);
/* One Adafactor step over the set, step = the entries' step count after it (>= 1), per parameter
 * p with averaged gradient g (fp32; only the written fma fused; sqrt and / correctly rounded):
 *   w = step^beta2_decay;  rho = min(lr, 1/sqrt(step));  alpha = max(eps2, ||p|| / sqrt(numel)) * rho
 *   row_var = lerp(row_var, mean_j g^2, w);  col_var = lerp(col_var, mean_i g^2, w)
 *   v = (row_var[i] / max(mean_i row_var, eps1)) * col_var[j]      (1-D: v = variance = lerp(., g^2, w))
 *   u = g * (1 / sqrt(max(v, eps1^2)));  denom = max(1, ||u|| / (sqrt(numel) * d))
 *   p = fma(-alpha / denom, u, p * (1 - lr * weight_decay))
 * Sums run in fp32 inside a lane (at most 16 terms) and in double above; the order depends on the
 * parameter's shape alone.  ZS_ERR_INVALID, nothing launched: a NULL argument, a set of another
 * family, step < 1, hyper-parameters zs_adafactor_hparams_init would refuse. */
int zs_adafactorset_run(const zs_adafactorset* as, const zs_adafactor_hparams* hp, int64_t step,
                        uintptr_t stream);
/* One pass of zs_adafactorset_run with the small kernels behind it (0: statistics, factors, alpha;
 * 1: update norm, step size; 2: apply), for measurement; 0, 1, 2 in order are one run. */
int zs_adafactorset_run_pass(const zs_adafactorset* as, const zs_adafactor_hparams* hp,
                             int64_t step, int pass, uintptr_t stream);
/* Elements covered, algorithmic HBM bytes of one run, and (optional, may be NULL) the bytes of
 * each of the three passes and of the set's scratch allocation. */
int zs_adafactorset_stats(const zs_adafactorset* as, int64_t* elems, int64_t* bytes,
                          int64_t* pass_bytes, int64_t* scratch_bytes);
int zs_adafactorset_destroy(zs_adafactorset* as);

/* ------------------------------------------------------------------------------------------ */
/* Fused Muon (torch.optim.Muon's rule), additive in ABI v13.  Per owned R x C matrix: momentum, */
/* Newton-Schulz orthogonalisation of the bf16 update on the matrix cores (bf16 MFMA, fp32       */
/* accumulators, torch's three bf16 rounding points per iteration), decoupled weight decay.      */
/* With r = min(R, C), c = max(R, C) an iteration is 4 r^2 c + 2 r^3 flops, of which the two      */
/* symmetric products compute the upper triangle of tiles only.                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t g;          /* reduced gradient sum, R * C elements of g_dtype (required) */
  uint64_t master;     /* as zs_adafactor_seg: the fp32 master, or (ZS_BF16_SPLIT) the bf16 param */
  uint64_t master_out; /* the fp32 master again (in place), or (ZS_BF16_SPLIT) the int16 residual */
  uint64_t p_out;      /* optional bf16 copy; (ZS_BF16_SPLIT) the bf16 param written, required */
  uint64_t buf;        /* fp32 momentum buffer, R * C elements, updated in place */
  int64_t R, C;        /* rows and columns: row i starts at element i * C */
  int64_t param;       /* the caller's index of the entry's parameter (>= 0) */
} zs_muon_seg;

typedef struct {
  /* the group's scalars as doubles; a run rounds what it derives from them to f32 once */
  double lr, weight_decay, momentum;
  double ns_a, ns_b, ns_c; /* ns_coefficients */
  double eps;
  double grad_div;         /* divide the reduced sum by this (world size) */
  int32_t nesterov;
  int32_t ns_steps;        /* 0 .. 99 */
  int32_t adjust_lr;       /* 0: None / "original" (sqrt(max(1, R / C))); 1: "match_rms_adamw" */
  int32_t reserved;
} zs_muon_hparams;

/* torch.optim.Muon's rules: ZS_ERR_INVALID unless lr >= 0, momentum >= 0, weight_decay >= 0,
 * 0 <= ns_steps < 100, adjust_lr in {0, 1}, eps >= 0, grad_div > 0 and hp is not NULL. */
int zs_muon_hparams_init(double lr, double weight_decay, double momentum, int nesterov, double ns_a,
                         double ns_b, double ns_c, double eps, int ns_steps, int adjust_lr,
                         double grad_div, zs_muon_hparams* hp);
typedef struct zs_muonset zs_muonset;
/* g_dtype ZS_F32 or ZS_BF16; p_dtype ZS_BF16 (fp32 master in place, optional bf16 p_out) or
 * ZS_BF16_SPLIT.  Entries are grouped by shape and run in batches of same-shape matrices (one
 * launch per pass and product, grid z = matrix).  The set owns one scratch allocation that holds a
 * batch: per matrix X (r x c), two copies of X^T (the third product writes the new transpose
 * beside the one other workgroups still read), A and Bm (r x r) in bf16, rows padded to 16 bytes.
 * scratch_budget bounds those bytes (0: 1 GiB) and so the batch size; a matrix that alone exceeds
 * it is refused.  Every check comes before any allocation or upload. */
int zs_muonset_create(const zs_muon_seg* segs, int64_t n, int g_dtype, int p_dtype,
                      int64_t scratch_budget, zs_muonset** out);
/* One Muon step over the set, per matrix p (R x C) with averaged gradient g:
 *   buf = lerp(buf, g, 1 - momentum);  u = nesterov ? lerp(g, buf, momentum) : buf   (ATen's lerp)
 *   X = bf16(u), transposed if R > C;  X = bf16(float(X) / float(bf16(max(||X||_F, eps))))
 *   ns_steps times: A = bf16(X X^T); Bm = bf16(b A + c A A); X = bf16(a X + Bm X)
 *   p = fma(-adjust_lr(lr), float(O), p * (1 - lr * weight_decay)),  O = X in p's orientation
 * The norm's squares are summed in fp32 over 4 terms and in double above, in an order fixed by the
 * shape; the root is rounded to fp32 and then to bf16.  ZS_ERR_INVALID, nothing launched: a NULL
 * argument, a set of another family, hyper-parameters zs_muon_hparams_init would refuse. */
int zs_muonset_run(zs_muonset* ms, const zs_muon_hparams* hp, uintptr_t stream);
/* One pass of zs_muonset_run over batch `batch` (-1: every batch): 0 = M1 and the norm, 1 = M2,
 * 2 = the products (product -1: all ns_steps iterations; 0, 1, 2: that one product of one
 * iteration), 3 = P.  For tests and measurement; with more than one batch the scratch holds the
 * batch run last. */
int zs_muonset_run_pass(zs_muonset* ms, const zs_muon_hparams* hp, int pass, int product,
                        int64_t batch, uintptr_t stream);
/* out[0 .. n) of: elements, stream-pass HBM bytes of one run, the bytes of M1, M2 and P, scratch
 * bytes, flops of one Newton-Schulz iteration (nominal), flops its tiles compute, batches. */
int zs_muonset_stats(const zs_muonset* ms, int64_t* out, int n);
/* Diagnostic, like zs_muonset_run_pass: out[0 .. 12) of batch `batch`: first entry (in the
 * shape-grouped order), matrices, R, C, the row strides of the r- and c-column arrays, the device
 * addresses of X, the current X^T, A, Bm and the norms (fp32, one per matrix), scratch bytes.
 * Matrix k of the batch starts k * rows * stride elements into each array. */
int zs_muonset_batch(const zs_muonset* ms, int64_t batch, int64_t* out);
int zs_muonset_destroy(zs_muonset* ms);
/* The bare product of the iteration on caller buffers (diagnostic, like zs_tune):
 *   D[M x N] = bf16(alpha * A[M x K] * B[N x K]^T + beta * E[M x N]),  bf16 in, fp32 accumulate,
 * K contiguous in A and B; D2 (optional, N x M) receives D^T, bit for bit.  sym != 0: M == N and D
 * is known symmetric: only tiles with tile_n >= tile_m are computed and each is mirrored into D
 * (D2 must be 0).  E may be D.  Any sizes and strides; 16-byte aligned rows take 16-byte accesses. */
int zs_muon_gemm_nt(uint64_t A, int64_t lda, uint64_t B, int64_t ldb, uint64_t E, int64_t lde,
                    uint64_t D, int64_t ldd, uint64_t D2, int64_t ldd2, int64_t M, int64_t N,
                    int64_t K, double alpha, double beta, int sym, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused NorMuon (zero_amd.optim.NorMuon), additive in ABI v13: Muon's orthogonalised update,   */
/* every row of it divided by a running second moment of that row (one fp32 per row), the whole */
/* rescaled so that the update's RMS is 0.2 lr.  It runs on a zs_muonset that has row state.    */
typedef struct {
  zs_muon_hparams muon;  /* adjust_lr is unused: the rescale is the adjustment */
  double beta2;          /* the row second moment's decay, in [0, 1) */
  double norm_eps;       /* added to the root of the row second moment, >= 0 */
} zs_normuon_hparams;

/* zs_muon_hparams_init's rules (adjust_lr 0), and ZS_ERR_INVALID unless 0 <= beta2 < 1 and
 * norm_eps >= 0. */
int zs_normuon_hparams_init(double lr, double weight_decay, double momentum, int nesterov,
                            double ns_a, double ns_b, double ns_c, double eps, int ns_steps,
                            double beta2, double norm_eps, double grad_div, zs_normuon_hparams* hp);
/* Gives the set its row state: row_v[k] is the device address of entry k's R fp32 (the order of
 * zs_muonset_create's table), read and written by every NorMuon run.  The set allocates the row
 * scratch here, apart from the Muon scratch: R doubles (the row sums of squares) and R floats (the
 * steps) per matrix of the largest batch; zs_muonset_stats' scratch bytes grow by it.  A set that
 * never gets row state allocates and reports what it always did.  ZS_ERR_INVALID, nothing
 * allocated: n is not the table's length, a NULL or misaligned address, row state given twice. */
int zs_muonset_attach_rows(zs_muonset* ms, const uint64_t* row_v, int64_t n);
/* One NorMuon step over the set: zs_muonset_run's M1, norm, M2 and products, then per matrix
 *   N1  rowsq_i = sum_j O_ij^2: eight squares of a 16-byte piece in fp32, doubles above, in an order
 *       fixed by C
 *   N2  v_i = lerp(v_i, fp32(rowsq_i / C), 1 - beta2);  q_i = sqrt(v_i) + norm_eps  (fp32)
 *       F^2 = sum_i rowsq_i / q_i^2  (double);  rowstep_i = fp32(-(0.2 lr sqrt(R C)) / (sqrt(F^2) q_i)),
 *       +0.0 for every row if F^2 == 0
 *   N3  p_ij = fma(rowstep_i, float(O_ij), p_ij * (1 - lr * weight_decay))
 * ZS_ERR_INVALID, nothing launched: what zs_muonset_run refuses, hyper-parameters
 * zs_normuon_hparams_init would refuse, a set without row state. */
int zs_muonset_run_normuon(zs_muonset* ms, const zs_normuon_hparams* hp, uintptr_t stream);
/* One pass of zs_muonset_run_normuon, as zs_muonset_run_pass: 0 = M1 and the norm, 1 = M2, 2 = the
 * products (`product` as there), 3 = N1, 4 = N2, 5 = N3. */
int zs_muonset_run_normuon_pass(zs_muonset* ms, const zs_normuon_hparams* hp, int pass, int product,
                                int64_t batch, uintptr_t stream);
/* Diagnostic, beside zs_muonset_batch: out[0 .. 4) of batch `batch`: the device addresses of rowsq
 * (doubles) and rowstep (floats), matrix k of the batch R elements in; R; the row scratch's bytes. */
int zs_muonset_rows(const zs_muonset* ms, int64_t batch, int64_t* out);

/* ------------------------------------------------------------------------------------------ */
/* Fused Adam-mini (Zhang et al. 2024, arXiv:2406.16793; zero_amd.optim.AdamMini's rule),        */
/* additive in ABI v13: Adam's first moment per element, one second moment per block of the      */
/* parameter (block_rows consecutive rows, or the whole of it).  A block of at most resident_cap */
/* elements is owned by one workgroup that holds its gradient in registers between the           */
/* reduction and the apply (g read once; 18 B/element with bf16 gradients over the split         */
/* master); a larger block takes two passes with a finish kernel between them (20 B/element).    */
/* Nothing is atomic, every scalar stays on the device and the bits repeat from run to run.      */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t g;          /* reduced gradient sum, R * C elements of g_dtype (required) */
  uint64_t master;     /* as zs_adafactor_seg: the fp32 master, or (ZS_BF16_SPLIT) the bf16 param read */
  uint64_t master_out; /* the fp32 master again (updated in place), or (ZS_BF16_SPLIT) the int16
                          residual, read and rewritten */
  uint64_t p_out;      /* optional bf16 copy of the updated param; (ZS_BF16_SPLIT) the bf16 param
                          written, required */
  uint64_t m;          /* fp32 exp_avg, R * C elements, updated in place */
  uint64_t v;          /* fp32 block_exp_avg_sq, one per block, updated in place */
  int64_t R, C;        /* rows and columns: row i starts at element i * C (1-D: R = 1) */
  int64_t block_rows;  /* rows of a block; it divides R; 0: the whole entry is one block */
  int64_t param;       /* the caller's index of the entry's parameter */
} zs_adamini_seg;

typedef struct {
  /* the group's scalars as doubles; a run rounds what it derives from them to f32 once */
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  double grad_div;     /* divide the reduced sum by this (world size) */
  int32_t maximize;
  int32_t reserved;
} zs_adamini_hparams;

/* Fill hp from a zero_amd.optim.AdamMini param group.  ZS_ERR_INVALID unless lr >= 0, both betas in
 * [0, 1), eps >= 0, weight_decay >= 0, grad_div > 0 and hp is not NULL. */
int zs_adamini_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                            int maximize, double grad_div, zs_adamini_hparams* hp);
typedef struct zs_adaminiset zs_adaminiset;
/* g_dtype ZS_F32 or ZS_BF16; p_dtype ZS_BF16 (fp32 master in place, optional bf16 p_out) or
 * ZS_BF16_SPLIT.  resident_cap, in [0, 16384] elements: a block of at most that many takes the
 * resident path, a larger one the two passes (0: every block).  An entry whose block length is a
 * multiple of the 16-byte gradient vector (8 bf16, 4 fp32) and whose pointers are 16-byte aligned
 * takes 16-byte accesses; any other entry element accesses in the same kernels with the same
 * arithmetic and reduction order.  The set owns its scratch (the tiles' partial sums, a_b of every
 * block).  Every check comes before any allocation or upload. */
int zs_adaminiset_create(const zs_adamini_seg* segs, int64_t n, int g_dtype, int p_dtype,
                         int64_t resident_cap, zs_adaminiset** out);
/* One Adam-mini step over the set, step = the entries' step count t after it (>= 1), per block b
 * with averaged gradient g (fp32; only the written fma fused; sqrt and / correctly rounded):
 *   m = lerp(m, g, 1 - beta1)                                   (ATen's two-range lerp)
 *   v_b = fma(1 - beta2, fp32(sum g^2 / L), v_b * beta2)
 *   a_b = fp32(-(lr / (1 - beta1^t)) / (sqrt(double(v_b)) / sqrt(1 - beta2^t) + eps))   (double)
 *   p = fma(a_b, m, p * (1 - lr * weight_decay))
 * Sums run in fp32 inside a 16-byte piece and in double above; the order depends on the block's
 * length and path alone.  ZS_ERR_INVALID, nothing launched: a NULL argument, a set of another
 * family, step < 1, hyper-parameters zs_adamini_hparams_init would refuse. */
int zs_adaminiset_run(const zs_adaminiset* as, const zs_adamini_hparams* hp, int64_t step,
                      uintptr_t stream);
/* One part of zs_adaminiset_run (0: the resident kernel; 1: pass 1 and the finish kernel; 2: pass
 * 2), for measurement; 0, 1, 2 in order are one run. */
int zs_adaminiset_run_pass(const zs_adaminiset* as, const zs_adamini_hparams* hp, int64_t step,
                           int pass, uintptr_t stream);
/* out[0 .. min(n, 9)): elements covered; algorithmic HBM bytes of one run; elements and bytes of
 * the resident path; elements and bytes of the two-pass path; bytes of the set's scratch; blocks;
 * the device address of the blocks' a_b (fp32, table order, the last run's; diagnostic). */
int zs_adaminiset_stats(const zs_adaminiset* as, int64_t* out, int64_t n);
int zs_adaminiset_destroy(zs_adaminiset* as);

/* ------------------------------------------------------------------------------------------ */
/* Fused APOLLO (Zhu et al. 2024, arXiv:2412.05270; zero_amd.optim.Apollo's rule), additive in   */
/* ABI v13: Adam's moments on a rank-r sign sketch of the gradient, one step scale per channel   */
/* (or per tensor) applied to the raw gradient; no per-element optimizer state.  An R x C entry  */
/* has N = max(R, C) channels of K = min(R, C) elements (rows when R >= C, columns otherwise).   */
/* The sketch runs on v_mfma_f32_32x32x16_bf16 with the +-1 operand formed in registers from     */
/* zs_sr_bits; nothing is atomic, every scalar stays on the device, the bits repeat from run to  */
/* run.                                                                                          */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t g;          /* reduced gradient sum, R * C elements of g_dtype (required) */
  uint64_t master;     /* as zs_adamini_seg */
  uint64_t master_out; /* as zs_adamini_seg */
  uint64_t p_out;      /* as zs_adamini_seg */
  uint64_t m;          /* fp32 exp_avg, N * rank elements, channel-major, updated in place */
  uint64_t v;          /* fp32 exp_avg_sq, likewise */
  uint64_t fprev;      /* fp32 scaled_grad_norm, one element, read and rewritten */
  int64_t R, C;        /* rows and columns: row i starts at element i * C */
  uint64_t seed;       /* the optimizer's seed + the parameter's ordinal in it */
  int64_t param;       /* the caller's index of the entry's parameter */
} zs_apollo_seg;

enum { ZS_APOLLO_CHANNEL = 0, ZS_APOLLO_TENSOR = 1 };

typedef struct {
  /* the group's scalars as doubles; a run rounds what it derives from them to f32 once */
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  double scale;            /* the step is multiplied by sqrt(scale) */
  double norm_growth;      /* the norm-growth limiter's gamma (> 1), or 0: no limiter */
  double grad_div;         /* divide the reduced sum by this (world size) */
  int64_t update_proj_gap; /* the signs are re-drawn every this many steps */
  int32_t scale_type;      /* ZS_APOLLO_CHANNEL or ZS_APOLLO_TENSOR */
  int32_t maximize;
} zs_apollo_hparams;

/* Fill hp from a zero_amd.optim.Apollo param group.  ZS_ERR_INVALID unless lr >= 0, both betas in
 * [0, 1), eps >= 0, weight_decay >= 0, scale > 0, scale_type is one of the two, update_proj_gap >= 1,
 * norm_growth is 0 or > 1, grad_div > 0 and hp is not NULL. */
int zs_apollo_hparams_init(double lr, double beta1, double beta2, double eps, double weight_decay,
                           double scale, int scale_type, int64_t update_proj_gap,
                           double norm_growth, int maximize, double grad_div,
                           zs_apollo_hparams* hp);
typedef struct zs_apolloset zs_apolloset;
/* g_dtype ZS_F32 or ZS_BF16; p_dtype ZS_BF16 (fp32 master in place, optional bf16 p_out) or
 * ZS_BF16_SPLIT; rank in [1, 256].  Entries of any shapes share a launch.  The set owns its scratch
 * (the sketch's partial sums, the channels' sums and a_c).  Every check comes before any
 * allocation or upload. */
int zs_apolloset_create(const zs_apollo_seg* segs, int64_t n, int g_dtype, int p_dtype,
                        int64_t rank, zs_apolloset** out);
/* One APOLLO step over the set, step = the entries' step count t after it (>= 1).  Per entry, with
 * g = gradsum / grad_div (fp32, negated under maximize) and G[c, k] channel c's k-th element:
 *   (k0, k1) = zs_sr_keys(seed, (t - 1) / update_proj_gap)
 *   sigma(k, j) = +1 if bit (k & 31) of zs_sr_bits((j << 32) | (k >> 5), k0, k1) is 0, else -1
 *   S[c, j] = fp32(fp32(sum_k sigma(k, j) bf16(Gsum[c, k])) * fp32(1 / (grad_div sqrt(rank))))
 *   M = lerp(M, S, 1 - beta1);  V = fma(1 - beta2, S * S, V * beta2)                      (fp32)
 *   Nh = (M / (1 - beta1^t)) / (sqrt(V) / sqrt(1 - beta2^t) + eps)                        (fp32)
 *   s_c = sqrt(sum_j Nh^2) / (sqrt(sum_j S^2) + 1e-8)          (double; "tensor": both sums over c too)
 *   F = sqrt(sum_c s_c^2 sum_k g[c, k]^2)
 *   lam = max(F / (F_prev + 1e-8), norm_growth) / norm_growth if norm_growth > 0 and F_prev > 0, else 1
 *   F_prev = fp32(F / lam);  a_c = fp32(-lr sqrt(scale) s_c / lam)
 *   p = fma(a_c, g, p * fp32(1 - lr * weight_decay))
 * The sketch accumulates in the matrix cores' fp32; other sums run in fp32 inside a 16-byte piece
 * and in double above, in an order that depends on the shape alone.  ZS_ERR_INVALID, nothing
 * launched: a NULL argument, a set of another family, step < 1, hyper-parameters
 * zs_apollo_hparams_init would refuse. */
int zs_apolloset_run(const zs_apolloset* as, const zs_apollo_hparams* hp, int64_t step,
                     uintptr_t stream);
/* One kernel of zs_apolloset_run (0: the sketch and the sums of g^2; 1: the sketch-space Adam; 2:
 * the finish; 3: the apply), for measurement; 0 .. 3 in order are one run. */
int zs_apolloset_run_pass(const zs_apolloset* as, const zs_apollo_hparams* hp, int64_t step,
                          int pass, uintptr_t stream);
/* out[0 .. min(n, 9)): elements covered; algorithmic HBM bytes of one run; bytes of the set's
 * scratch; the device address of a_c (fp32, the entries' channels in table order, the last run's);
 * channels; elements of M and V together; the device address of the first entry's partial sketch
 * sums (fp32 [cut][channel][rank] per entry, each entry at a multiple of 4 floats, before the
 * scale; diagnostic); the sketch's workgroups; the floats of all entries' partial sums. */
int zs_apolloset_stats(const zs_apolloset* as, int64_t* out, int64_t n);
int zs_apolloset_destroy(zs_apolloset* as);

/* Single-range form, SURVEY.md §8(b)'s signature: one torch.optim.Adam/AdamW step over n
 * contiguous elements — the update of one flat shard (zero1.py:88 on a flattened group) with no
 * table to build.  p: fp32 master/param, updated in place; p_bf16: optional bf16 copy of the
 * result (NULL = none); g: reduced gradient sum (g_dtype ZS_F32 or ZS_BF16; NULL = zero); m, v:
 * fp32 exp_avg / exp_avg_sq, in place; carry: ZeRO-1's A_{t-1}, READ AND REWRITTEN with A_t
 * (NULL = none; SURVEY.md §8(b) spells it const, but the kernel writes it, so it is declared
 * writable — same C calling convention); carry_scale: ws-1.  grad_scale = 1/ws: the update
 * divides by the float nearest to 1/grad_scale (the world size), as zero1.py:84 `p.grad /= ws`.
 * The float scalars are widened to double before torch's bias-correction arithmetic; torch
 * derives them from Python doubles (adam.py:508-515), so for torch's bits with hyper-parameters
 * not exactly representable in fp32 (lr=1e-3, betas 0.9 / 0.999) use zs_adam_step_ex.  Same
 * kernels as zs_adamset_run; amsgrad / maximize / the split master need an adamset.
 * Asynchronous on `stream`; its two-entry table is a stream-ordered allocation. */
int zs_adam_step(float* p, uint16_t* p_bf16, const void* g, int g_dtype, float* m, float* v,
                 int64_t n, float lr, float b1, float b2, float eps, float wd, int decoupled,
                 int64_t step, float grad_scale, float* carry, float carry_scale,
                 uintptr_t stream);
/* The same with torch's double scalars and the divisor itself (grad_div = ws; for a
 * non-power-of-two ws dividing is not multiplying by 1/ws): bit-exact with torch's arithmetic. */
int zs_adam_step_ex(float* p, uint16_t* p_bf16, const void* g, int g_dtype, float* m, float* v,
                    int64_t n, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int decoupled, int64_t step, double grad_div, float* carry,
                    double carry_mul, uintptr_t stream);

/* ------------------------------------------------------------------------------------------ */
/* Device buffers outside the caller's caching allocator (ABI v10).  The placement probe          */
/* (zero_amd/engine.py probed_zeros) streams candidate allocations of a long-lived, bandwidth-    */
/* bound buffer and keeps the fastest; candidates come from here so a rejected one goes straight */
/* back to the device without emptying torch's cache (the caller's cached blocks stay).          */
/* ------------------------------------------------------------------------------------------ */
/* hipMalloc of `bytes` (> 0) into *out; ZS_ERR_NOMEM when the device is full. */
int zs_device_alloc(int64_t bytes, void** out);
/* hipFree (NULL is a no-op).  Synchronises the device as hipFree does: only for buffers no queued
 * work still uses.  Also frees a zs_device_alloc_chunked range (unmap, release, address free). */
int zs_device_free(void* p);
/* (v13) `bytes` rounded up to whole `chunk_bytes` chunks: physical chunks of their own
 * (hipMemCreate) mapped side by side into one reserved virtual range, read / write for this
 * device.  The placement probe's second route (zero_amd/engine.py probed_zeros): tried when no
 * plain allocation streams at the acceptance rate.  Freed with zs_device_free. */
int zs_device_alloc_chunked(int64_t bytes, int64_t chunk_bytes, void** out);

/* Diagnostic A/B knobs (process-wide; the defaults are the measured best, so a product caller
 * never needs this): "dq_unroll" (4 / 8 / 16 accesses in flight per lane of the fp8 dequantise),
 * "dq_nt_store" (0 / 1: non-temporal stores), "dq_wg_per_cu" (0 = one wave per row; k = at most k
 * workgroups per CU walking several rows each), "scale_nt" (zs_scale's cache policy: -1 by size,
 * non-temporal above 256 MiB; 0 default policy; 1 non-temporal), "convert_nt" (zs_convert's, the
 * same by source + destination bytes), "copy_nt" (zs_copyset_run's, by 2 x the set's bytes),
 * "accumulate_nt" (zs_accumulate's, by the 3 x n x element size bytes it touches, and
 * zs_accumulate_widen's, by its 8 or 10 B per element),
 * "adam_wg_per_cu" (0 = the default grid of the fused Adam: 128 workgroups per CU, 1024 for the
 * loads-first kernel of a split master; k = at most k per CU), "adam_loads_first" (1: a full chunk
 * of the vector Adam issues all its loads before its first wait; 0: every chunk through the
 * per-lane predicated body that partial chunks take, one group's loads in flight at a time — the
 * kernel before the loads-first body, kept for A/B runs, tools/adam_ab.py), "sqnorm_nt" (1: the
 * gradient sum-of-squares pass loads non-temporally; 0: default cache policy; the sum's bits do
 * not depend on it, tools/clip_ab.py), "sync_host_flags" (1: flag syncs created from now on take words in pinned host
 * memory, whose satisfied waits the host skips; 0: device words, every wait enqueued — the
 * fallback the library takes by itself when pinned memory is refused), "sync_write_kernel" (1: a
 * flag sync's record is a one-wave kernel storing the epoch with a system-scope release; 0:
 * hipStreamWriteValue64 — same ordering, the runtime's stream-operation command costs more host
 * time), "sync_write_fence" (1: that store is a system-scope release; 0: relaxed), "sync_wait_kernel"
 * (1: a flag wait is a one-wave kernel polling the word with s_sleep between loads; 0:
 * hipStreamWaitValue64, on this stack a runtime kernel spinning without pause beside the compute
 * stream's kernels).  *previous (may be NULL) gets the old value;
 * ZS_ERR_INVALID for an unknown key or value. */
int zs_tune(const char* key, int64_t value, int64_t* previous);

/* ------------------------------------------------------------------------------------------ */
/* RCCL over xGMI.  Replaces the per-tensor dist.all_reduce (zero1.py:83, zero3.py:146),        */
/* dist.reduce_scatter_tensor (zero2.py:107), dist.broadcast (zero1.py:102, zero2.py:133) and   */
/* dist.all_gather (zero3.py:39) with bucketed collectives on a caller stream.                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct zs_comm zs_comm;
#define ZS_UNIQUE_ID_BYTES 128
int zs_comm_unique_id(void* out128);
int zs_comm_init(const void* unique_id128, int ws, int rank, zs_comm** out);
int zs_comm_destroy(zs_comm* comm);
/* recv_count / send_count are elements per rank (NCCL convention). In-place is allowed:
 * recv == send + rank*recv_count (reduce-scatter), send == recv + rank*send_count (all-gather). */
int zs_reduce_scatter(zs_comm* comm, const void* send, void* recv, int64_t recv_count, int dtype,
                      uintptr_t stream);
int zs_all_gather(zs_comm* comm, const void* send, void* recv, int64_t send_count, int dtype,
                  uintptr_t stream);
int zs_all_reduce(zs_comm* comm, const void* send, void* recv, int64_t count, int dtype,
                  uintptr_t stream);
/* SUM-reduce count elements onto `root` (recv only read on root; in place when send == recv) and
 * broadcast count elements from `root`.  Issued once per owner inside zs_group_start/end they
 * form the reduce-scatter-v / all-gather-v of a ragged bucket (zero2.py:107 / zero2.py:133). */
int zs_reduce(zs_comm* comm, const void* send, void* recv, int64_t count, int dtype, int root,
              uintptr_t stream);
int zs_broadcast(zs_comm* comm, const void* send, void* recv, int64_t count, int dtype, int root,
                 uintptr_t stream);
/* One RCCL group of n SUM-reduces (entry i: send[i] -> recv[i] on root[i], count[i] elements;
 * recv[i] is only written on its root and may equal send[i]) or of n in-place broadcasts
 * (buf[i] from root[i]).  The reduce-scatter-v / all-gather-v of one round of the flat
 * parameter arena: each owner's contiguous window reduced to it (zero2.py:94-113) and its
 * updated parameters broadcast from it (zero2.py:122-133), one call per round. */
int zs_reduce_group(zs_comm* comm, int64_t n, const uint64_t* send, const uint64_t* recv,
                    const int64_t* count, const int32_t* root, int dtype, uintptr_t stream);
int zs_broadcast_group(zs_comm* comm, int64_t n, const uint64_t* buf, const int64_t* count,
                       const int32_t* root, int dtype, uintptr_t stream);
/* One RCCL group of n all-gathers (entry i: send_count[i] elements from send[i] on every rank
 * into recv[i], rank-major) or of n SUM reduce-scatters (entry i: ws * recv_count[i] elements at
 * send[i] reduced, this rank's recv_count[i] into recv[i]).  ZeRO-3's per-module gather of every
 * parameter's dim-0 chunk (Zero3ParamManager.materialize, zero3.py:36-41, one group per module)
 * and one backward bucket of gradient reduce-scatters into the chunk arena (the reduction of
 * zero3.py:131-147), each as ONE call instead of one per parameter. */
int zs_all_gather_group(zs_comm* comm, int64_t n, const uint64_t* send, const uint64_t* recv,
                        const int64_t* send_count, int dtype, uintptr_t stream);
int zs_reduce_scatter_group(zs_comm* comm, int64_t n, const uint64_t* send, const uint64_t* recv,
                            const int64_t* recv_count, int dtype, uintptr_t stream);
/* The same two groups with their stream ordering in the same call (a ZeRO-3 module gather or a
 * gradient bucket is otherwise four runtime calls from Python around one library call):
 * ready_event != 0: record it on after_stream (where the inputs were produced) and make `stream`
 * wait for it; then the group (comm may be NULL when n == 0: ordering only); done_event != 0:
 * record it on `stream` after the group.  Events are HIP events (hipEvent_t as uint64_t). */
int zs_all_gather_group_ordered(zs_comm* comm, int64_t n, const uint64_t* send,
                                const uint64_t* recv, const int64_t* send_count, int dtype,
                                uintptr_t after_stream, uint64_t ready_event, uintptr_t stream,
                                uint64_t done_event);
int zs_reduce_scatter_group_ordered(zs_comm* comm, int64_t n, const uint64_t* send,
                                    const uint64_t* recv, const int64_t* recv_count, int dtype,
                                    uintptr_t after_stream, uint64_t ready_event, uintptr_t stream,
                                    uint64_t done_event);
/* hipStreamWaitEvent(stream, event): the consumer side of the ordered groups. */
int zs_stream_wait_event(uintptr_t stream, uint64_t event);
/* Sync objects (ABI v12; v13: 64-bit epochs): a cross-stream ordering point that is either a HIP
 * event (ZS_SYNC_EVENT) or a stream memory operation on a flag word in pinned host-coherent memory
 * (ZS_SYNC_FLAG: the epoch stored on the producer — a one-wave store kernel with a system-scope
 * release, or hipStreamWriteValue64 (zs_tune "sync_write_kernel") — and a wait for >= it on the
 * consumer — a one-wave polling kernel, or hipStreamWaitValue64 (zs_tune "sync_wait_kernel"); epochs only grow and never wrap).  zs_sync_record enqueues the producer side on
 * `stream`; zs_sync_wait makes `stream` wait for the latest record (hipStreamWaitEvent's
 * semantics; a never-recorded sync, or one whose latest record has already executed — the host
 * reads the flag word — enqueues nothing).  A flag record from another stream than the previous
 * record's first waits for that record (v13), so any stream may record.  The ZeRO-3 gathers and
 * gradient buckets (zero3.py:36-41, 131-147; their torch.cuda.synchronize() after each collective
 * becomes this ordering) use the synced group forms: record `ready` on after_stream and wait for
 * it on `stream`, the RCCL group, record `done` on `stream` (either sync may be NULL). */
typedef struct zs_sync zs_sync;
enum zs_sync_kind { ZS_SYNC_EVENT = 0, ZS_SYNC_FLAG = 1 };
int zs_sync_create(int kind, zs_sync** out);
int zs_sync_destroy(zs_sync* sync);
int zs_sync_record(zs_sync* sync, uintptr_t stream);
int zs_sync_wait(zs_sync* sync, uintptr_t stream);
/* Test hook (v13): move a flag sync's epoch (and its word) forward to `epoch` — every record made
 * so far must have executed.  Lets a test cross an epoch boundary (2^32) without 2^32 records.
 * ZS_ERR_INVALID for an event sync, a smaller epoch or a pending record. */
int zs_sync_set_epoch(zs_sync* sync, uint64_t epoch);
/* Diagnostic (v13): a flag sync's latest recorded epoch and the current value of its word (the
 * word read through hipMemcpy when it lives in device memory); 0 / 0 for an event sync. */
int zs_sync_query(zs_sync* sync, uint64_t* epoch, uint64_t* word);
int zs_all_gather_group_synced(zs_comm* comm, int64_t n, const uint64_t* send,
                               const uint64_t* recv, const int64_t* send_count, int dtype,
                               uintptr_t after_stream, zs_sync* ready, uintptr_t stream,
                               zs_sync* done);
int zs_reduce_scatter_group_synced(zs_comm* comm, int64_t n, const uint64_t* send,
                                   const uint64_t* recv, const int64_t* recv_count, int dtype,
                                   uintptr_t after_stream, zs_sync* ready, uintptr_t stream,
                                   zs_sync* done);
int zs_group_start(void);
int zs_group_end(void);
/* RCCL version the library is bound to at run time (e.g. 22606). */
int zs_rccl_version(int* version);

#ifdef __cplusplus
}
#endif
#endif /* ZERO_AMD_H */
