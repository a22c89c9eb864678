/*
 * stg/codec.h -- C-ABI of the MI355X-native StellaTrain gradient codec.
 *
 * This is the drop-in boundary.  It replaces the reference's
 *   class Compressor { virtual size_t compress(const std::string &name,
 *       ConstSegment<float> src, uint32_t k, Segment<uint32_t> dst_idx,
 *       Segment<float> dst_val, int32_t idx_offset = 0) = 0; }
 * (/root/reference/backend/src/compress/compressor.h:12-31) and its three
 * factory-selected implementations (engine/core.cpp:110-118, 185-195):
 *   "thresholdv16" -> ThresholdvCompressor16  (compress/thresholdv16.h:9-38)
 *   "thresholdv"   -> ThresholdvCompressor    (compress/thresholdv.h:9-29)
 *   "topk"         -> TopkCompressor          (compress/topk.h:9-31)
 * plus the inverse path of config 5: the MERGE decompress
 * (engine/modules/cpu_optimize.cpp:40-72) and the sparse SGD apply
 * (optim/sgd.cpp:34-263, SparseOptimizer::optimize_raw sparse_optimizer.h:42).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every entry point returns an int status (STG_OK == 0, < 0 on error) and
 * never throws; stg_last_error() returns a thread-local message.  The C++
 * shim in stg/compressor.h turns errors back into std::runtime_error, which
 * is what the reference throws (topk.cpp:34, core.cpp:117,193).
 *
 * Device pointers are HIP device (or host-mapped) pointers on the handle's
 * device; `stream` is a hipStream_t passed as void* (NULL = legacy default
 * stream).  Device entry points are asynchronous and never synchronise the
 * host; host entry points copy in, run, copy out and synchronise.
 */
#ifndef STG_CODEC_H
#define STG_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STG_OK 0
#define STG_ERR_INVALID (-1)     /* bad argument (e.g. capacity < k for topk)   */
#define STG_ERR_UNKNOWN (-2)     /* unknown method string                       */
#define STG_ERR_HIP (-3)         /* HIP runtime error                           */
#define STG_ERR_UNSUPPORTED (-4) /* size outside what this build handles        */
#define STG_ERR_DEVICE (-5)      /* device-side failure flag (see stg_check)    */

typedef struct stg_codec *stg_codec_t;
typedef struct stg_sgd *stg_sgd_t;
typedef struct stg_adam *stg_adam_t;

/* Method strings as in the reference factory (core.cpp:110-118).
 * "topk" reproduces the reference's shipped behaviour (the byte-count memcpy
 * of topk.cpp:31 and idx = 0..k-1); "topk_exact" is the intended top-k by
 * |x| over the whole bucket with real indices.  Replaces the
 * ThresholdvCompressor16 / ThresholdvCompressor / TopkCompressor
 * constructors (thresholdv16.h:33, thresholdv.h:25, topk.h:28). */
int stg_codec_create(const char *method, int device, stg_codec_t *out);
int stg_codec_destroy(stg_codec_t h);
/* Compressor::name() (compressor.h:28): "Thresholdv16", "Thresholdv", "Topk". */
const char *stg_codec_name(stg_codec_t h);

/* Compressor::compress on host memory (compressor.h:30), the engine's MERGE
 * call site (engine/modules/compress.cpp:141) and FasterDpEngine::compress
 * (core.cpp:1210-1245).  Copies src to the device, runs the codec, copies
 * (idx, val) back and synchronises.  *out_count receives compress()'s return
 * value.  `key` is the reference's `name` argument (persistent key
 * "layer@param", task.cpp:56-61); threshold-v ignores it and keys its AIMD
 * state by the src pointer value, as thresholdv.cpp:44 does. */
int stg_codec_compress_host(stg_codec_t h, const char *key, const float *src, size_t n, uint32_t k,
                            uint32_t *dst_idx, size_t idx_cap, float *dst_val, size_t val_cap,
                            int32_t idx_offset, size_t *out_count);

/* Same contract on device-resident buffers, fully asynchronous on `stream`:
 * no host synchronisation, per-key threshold state stays on the device.
 * The returned pair count is written to *d_count (device uint32).  dst
 * buffers are caller-owned with capacity idx_cap (val_cap >= idx_cap).
 * d_src, d_idx and d_val need only the alignment of their element (4 bytes;
 * 2 bytes for a 16-bit wire-form output): any such address gives the same
 * results and nothing outside [d_idx, d_idx + idx_cap), [d_val, d_val +
 * idx_cap) is written.  16-byte alignment of all three selects the vector
 * emission (the fast path); top-k reads a 16-byte aligned d_src by float4.
 * k and the capacities may differ from call to call on one key (the engine's
 * configure_compression_ratio): the key's state is carried over as the
 * reference carries it, and every call gives the reference's stream for the
 * state it meets (tests/test_gpu_ratio.py). */
int stg_codec_compress_device(stg_codec_t h, const char *key, const float *d_src, size_t n, uint32_t k,
                              uint32_t *d_idx, size_t idx_cap, float *d_val, size_t val_cap,
                              int32_t idx_offset, uint32_t *d_count, void *stream);

/* One bucket of a batched call: the arguments of one compress_device call
 * (d_src, d_idx, d_val: element-aligned is enough, as there; 16-byte
 * alignment of all three selects the bucket's vector emission). */
typedef struct stg_bucket {
    const char *key;
    const float *d_src;
    size_t n;
    uint32_t k;
    uint32_t *d_idx;
    size_t idx_cap;
    float *d_val;
    size_t val_cap;
    int32_t idx_offset;
    uint32_t *d_count;
} stg_bucket_t;

/* Batched compress_device: same results as calling stg_codec_compress_device
 * on buckets[0..nbuckets-1] in order on `stream`.  It stands in for the
 * engine's concurrent MERGE-compress tasks of one iteration (ThreadPool
 * workers calling compress() on different keys, engine/modules/compress.cpp:
 * 141, engine/config.h:7).  thresholdv16 runs up to 32 buckets with distinct
 * keys in one persistent launch, overlapping bucket b's count exchange with
 * bucket b+1's streaming pass; a repeated key starts a new launch. */
int stg_codec_compress_batch_device(stg_codec_t h, const stg_bucket_t *buckets, size_t nbuckets, void *stream);

/* One iteration's MERGE compress tasks with their error feedback
 * (ModuleCompress::run, engine/modules/compress.cpp:139-186): the batched
 * compress above, then for every bucket src[idx[i]] = 0 for i < idx_cap
 * (:178-179; the caller zero-fills idx, compress.cpp:60-64, so unused slots
 * zero element 0 as in the reference) and residual = src (:185), i.e.
 * d_residuals[i] ends as the bucket with the selected entries zeroed and the
 * bucket (d_src, written here) ends identical to it.  thresholdv16 fuses the
 * residual copy into its streaming pass (one HBM read of the bucket instead
 * of two); the other codecs run compress + stg_error_feedback_device. */
int stg_merge_compress_batch_device(stg_codec_t h, const stg_bucket_t *buckets, float *const *d_residuals,
                                    size_t nbuckets, void *stream);

/* One MERGE task with the intra-node gather ahead of it (ModuleCpuGather::run
 * then ModuleCompress::run on local rank r's slice, engine/modules/
 * cpu_gather.cpp:59-87 and compress.cpp:139-186).  bucket->d_src is grad[0]'s
 * slice: it receives d_residual (may be null) + d_grads[1] + ... +
 * d_grads[num_gpus - 1] (slice pointers, [0] ignored, peers' over xGMI) in
 * stg_gather_add_device's order, is compressed, and when d_residual is not
 * null its error feedback runs as in stg_merge_compress_batch_device.  The
 * same results as stg_gather_add_device, then stg_merge_compress_batch_device
 * (d_residual) or stg_codec_compress_device (no residual), on one bucket.
 * thresholdv16 sums the sources inside its one-bucket streaming pass (each
 * source read once, grad[0] stored once, the line sums taken from the sum):
 * one pass instead of the gather's and the codec's.  A key's first call, and
 * the other codecs, run the gather-add pass first.  Async on `stream`. */
int stg_merge_gather_compress_device(stg_codec_t h, const stg_bucket_t *bucket, float *d_residual,
                                     const float *const *d_grads, int num_gpus, void *stream);

/* Batched compress_device whose emission writes the wire form of each stream
 * (comm_manager.cpp:486-590 queueTx's packing, fused into the codec): bucket
 * i's pairs land in d_idx / d_val as stg_wire_encode_device(flags[i]) would
 * write them for the count = min(idx_cap, n) pairs the codec emits -- u16
 * indices when flags[i] & STG_WIRE_U16_IDX, fp16 values when
 * flags[i] & STG_WIRE_F16_VAL (the buffers hold count elements of that type),
 * the codec's own u32 / f32 otherwise.  The same bytes as
 * stg_codec_compress_batch_device followed by one encode per bucket, without
 * the encode pass.  *d_count as in compress_device.  thresholdv16 only
 * (STG_ERR_UNSUPPORTED for the other codecs).  Async on `stream`. */
int stg_codec_compress_wire_batch_device(stg_codec_t h, const stg_bucket_t *buckets, const int *flags,
                                         size_t nbuckets, void *stream);

/* One sender-side task of a batched call: one parameter tensor's gather,
 * compress with error feedback, and wire packing. */
typedef struct stg_send_task {
    stg_bucket_t bucket;          /* key; d_src = grad[0] (written); n; k; d_idx / d_val = the WIRE-form
                                     outputs (idx_cap elements of the types wire_flag selects, val_cap >=
                                     idx_cap); idx_offset; d_count                                       */
    float *d_residual;            /* n floats, read by the gather, rewritten by the error feedback;
                                     NULL = no residual term and no error feedback                      */
    const float *const *d_grads;  /* host array of num_gpus device pointers, [0] ignored; NULL if
                                     num_gpus == 1                                                      */
    int num_gpus;                 /* 1..16; 1 = no gather                                               */
    int wire_flag;                /* 0..3, STG_WIRE_* bits                                              */
} stg_send_task_t;                /* 104 bytes on LP64: bucket at 0 (80 bytes; its d_count at 72),
                                     d_residual at 80, d_grads at 88, num_gpus at 96, wire_flag at 100  */

/* The sender half of a MERGE iteration in one call: ModuleCpuGather::run
 * (cpu_gather.cpp:59-87), ModuleCompress::run with its error feedback
 * (compress.cpp:139-186) and queueTx's packing (comm_manager.cpp:486-590) for
 * every parameter tensor.  The results of task i are bitwise those of this
 * sequence on temporaries, run on tasks[0 .. ntasks-1] in order on `stream`:
 *   1. stg_merge_gather_compress_device(h, &b, d_residual, d_grads, num_gpus,
 *      stream), b being `bucket` with u32 / f32 temporaries of idx_cap slots
 *      as d_idx / d_val;
 *   2. stg_wire_encode_device(tmp_idx, tmp_val, count, wire_flag,
 *      bucket.d_idx, bucket.d_val, stream), count = min(idx_cap, n).
 * That is: grad[0] gathered and then zeroed at the selected entries; the
 * residual equal to grad[0] afterwards; the first `count` elements of the
 * wire-form d_idx / d_val (elements from `count` on are not written);
 * *d_count; the key's AIMD state.  The zeroing uses the true indices, never
 * the packed ones (a u16 index at or above 32,768 is saturated on the wire),
 * which is why error feedback and wire form need this call to be combined.
 * When idx_cap > count, element 0 is zeroed as well (the reference's
 * zero-filled unused slots, see stg_error_feedback_device).  A task with
 * n == 0 writes *d_count = 0 and touches nothing else.
 *   Launches do not grow with ntasks beyond one per 16 tasks of each kind: the
 * gather-adds of up to 16 tasks share one launch (a launch also closes before
 * its grid would pass 8 workgroups per CU; a larger tensor runs alone), then
 * the thresholdv16 scans run batched (up to 32 buckets per launch, residual
 * copy fused) into u32 / f32 staging of the stream's workspace, then one
 * launch per 16 tasks copies the ragged tails, zeroes the selected entries
 * and writes the wire form.  A single task of 2^22..2^24 elements keeps the
 * one-bucket scan with the sources summed inside its streaming pass.  Staging
 * takes 8 bytes per idx_cap slot of the call, kept with the workspace.
 *   thresholdv16, threshold-v and exact top-k.  STG_ERR_UNSUPPORTED for the
 * shipped "topk": it writes idx[i] = i, so its selected entries have no true
 * indices to zero.
 *   A threshold-v handle ("thresholdv"): the key is the pointer bucket.d_src
 * (thresholdv.cpp:44; `key` and idx_offset are ignored, and a key occurs twice
 * when two tasks with n > 0 share that pointer).  Its count varies, *d_count =
 * min(qualifiers, idx_cap), while the engine sends all W = min(idx_cap, n)
 * slots, the unused ones holding (index 0, value 0.0) (compress.cpp:60-64): the
 * first *d_count wire slots are the pairs, slots [*d_count, W) the wire form
 * of (0, 0.0f), the block / tail split at 8 * ((W - 1) / 8), nothing past W
 * written; under error feedback grad and residual are zeroed at the true
 * index of all W slots -- element 0 whenever *d_count < W -- and the residual
 * ends equal to grad[0].  That is step 1 above into zeroed temporaries and
 * step 2 with count = W.  Launches: the gather launches as above; per key's
 * first call its first-threshold select; then one scan launch per 16 tasks
 * (tv_batch.hip: a task takes max(1, ceil(n / 4 / 4096)) workgroups, a launch
 * also closes before min(2048, CUs) of them, a larger task runs alone through
 * the per-tensor scan and a copy to the residual), the residual copy fused;
 * then one finishing launch per 16 tasks (stg_debug_tv_batch_plan).
 *   An exact top-k handle ("topk_exact"): the key is `key`, as for
 * thresholdv16, and *d_count = idx_cap (topk.cpp:25; idx_cap < k is "Invalid
 * parameter k").  The winners are the min(k, n) largest |x|, ties at the k-th
 * magnitude taken in index order, emitted in index order with index +
 * idx_offset; slots [min(k, n), W), W = min(idx_cap, n), are the wire form of
 * (0, 0.0f), the block / tail split at 8 * ((W - 1) / 8), nothing past W
 * written; under error feedback grad and residual are zeroed at the true index
 * of every staged slot -- element 0 whenever min(k, n) < idx_cap -- and the
 * residual ends equal to grad[0].  That is step 1 above into zeroed temporaries
 * and step 2 with count = W.  The key's state ends as the per-tensor call
 * leaves it for this purpose (threshold = this call's k-th magnitude), so
 * batched and per-tensor calls on one key interleave freely; results never
 * depend on it.  Launches: the gather launches as above; then five select
 * launches per group of up to 16 tasks (topk_batch.hip: a task takes max(1,
 * ceil(n / 8192)) tiles, a group also closes before one tile per CU, a larger
 * task runs alone through the per-tensor top-k and a copy to the residual);
 * then one finishing launch per 16 tasks (stg_debug_topk_batch_plan).
 *   All or nothing: every task is checked before any device call or key-state
 * change, and stg_last_error() names the offending task index.
 * STG_ERR_INVALID: a null handle, a null `tasks` with ntasks > 0, the
 * conditions of stg_codec_compress_device (val_cap < idx_cap, a null d_count),
 * wire_flag bits outside 0..3, num_gpus outside 1..16, with n > 0 a null
 * bucket buffer, a null d_grads at num_gpus > 1 or a null source, and a key
 * that occurs twice in the call (the engine has one task per key per
 * iteration; the scans of a call all precede its finishing launches).
 * ntasks == 0 is STG_OK.  Buffers of different tasks must not overlap: the
 * tasks of one launch run concurrently.  Async on `stream`. */
int stg_merge_send_batch_device(stg_codec_t h, const stg_send_task_t *tasks, size_t ntasks, void *stream);

/* Per-key AIMD state (thresholdv16.cpp:243-259, thresholdv.cpp:72-80), read
 * back for parity tests; synchronises `stream`.  Returns STG_ERR_INVALID when
 * the key has never been compressed.  For threshold-v pass the src pointer
 * value as `key_ptr` (key is ignored); thresholdv16 uses `key`. */
int stg_codec_get_state(stg_codec_t h, const char *key, const void *key_ptr, float *threshold,
                        float *threshold_inc, void *stream);

/* Kernel timing, the GPU analogue of the reference's CRIT_PATH_compress stat
 * span (engine/modules/compress.cpp:140-142, core_module_api.cpp:504-514):
 * when enabled, every codec launch records HIP events on its stream:
 * [0] = the main kernel (thresholdv16: the whole batch kernel; threshold-v and
 * top-k: the streaming/count pass), [1] = the ordering/emission pass (0 for
 * thresholdv16, which has none), [2] = the whole call including first-call
 * work of threshold-v / top-k (thresholdv16's first-call launches precede
 * event [0] and are not timed).  stg_codec_get_timing synchronises the recorded events and returns
 * the accumulated milliseconds [0, 1, 2], the number of launches timed in
 * *calls and resets the accumulators (one batched call = one launch per run of
 * distinct keys). */
int stg_codec_set_timing(stg_codec_t h, int enable);
int stg_codec_get_timing(stg_codec_t h, double *ms3, uint64_t *calls);

/* Diagnostics: the first n (<= 64) scratch words of the handle's workspace
 * for `stream` (phase stamps of builds with STG_FILL_STAMPS); syncs. */
int stg_codec_debug_words(stg_codec_t h, void *stream, uint32_t *out, int n);

/* Diagnostics: workgroups a batched thresholdv16 scan launch of `chunks`
 * 128 KiB chunks gets on a device of num_cu CUs when `streams` distinct
 * streams launched the device's recent scans and the process has hw_queues
 * hardware queues.  Plain host arithmetic: needs no device.  0 on a bad
 * argument. */
int stg_debug_tv16_scan_grid(int num_cu, int streams, int hw_queues, uint32_t chunks);

/* Checks the device-side failure word of every workspace of this handle
 * (e.g. a regime-B candidate set larger than the build supports); syncs. */
int stg_codec_check(stg_codec_t h);

/* MERGE decompress (cpu_optimize.cpp:40-72): `world` rank streams of
 * `per_rank` (idx, val) pairs each, laid out back to back, are scattered
 * into a dense zeroed scratch of n floats in rank order (index_put_, no
 * accumulate, per rank: of a rank's duplicated indices -- e.g. the wire
 * format's u16 saturation -- the last occurrence wins), summed, divided by
 * `world`, and gathered at the union of indices (one entry per index,
 * unique1d :14-24).  world > 1: output index-ascending, d_dense (n floats,
 * zero, 16-byte aligned) and d_mark (n bytes, zero, 16-byte aligned) are
 * caller scratch and are left zero; a misaligned one is refused
 * (STG_ERR_INVALID) by every MERGE entry, the tasks of a batched call
 * included.  world == 1: no dense scratch (neither pointer is looked at); the
 * winners in stream order.
 * Indices >= n are dropped.  *d_out_count (device) gets the union size
 * (0xffffffff after a device failure).  Internal scratch is kept per (device,
 * stream) for reuse: 4 B per element of the largest n seen (8 B when world >
 * 1) plus 12 B per 4,096-pair tile -- about 64 MiB for n = 16 Mi at world 1,
 * 128 MiB at world > 1 -- until stg_scatter_merge_release.  The batched
 * stg_merge_optimize_{sgd,adam}_batch_device calls use the same scratch: a
 * launch of theirs takes 4 B per element of the sum of its tensors' n, a sum
 * capped at 8 Mi (32 MiB; one larger tensor: its own n), 8 B per 1,024-pair
 * tile of its tensors, and 6 KiB of per-slot hand-off words; a world > 1
 * group of theirs takes 13 B per element of the sum of its tensors' n (each n
 * rounded up to 16), a sum capped at 4 Mi: 32 MiB of winner words, 16 MiB of
 * dense floats, 4 MiB of mark bytes, and 8 B per 4,096-element tile. */
int stg_scatter_merge_device(const uint32_t *d_idx, const float *d_val, size_t per_rank, int world, size_t n,
                             float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                             uint32_t *d_out_count, void *stream);
/* The MERGE decompress scratch of (current device, stream): syncs the stream
 * and returns STG_ERR_DEVICE if a call on it hit a device failure (sticky). */
int stg_scatter_merge_check(void *stream);
/* Frees the MERGE decompress scratch of (current device, stream) after its
 * work is done (call it before destroying a stream that merged). */
int stg_scatter_merge_release(void *stream);

/* Error feedback of the MERGE compress (engine/modules/compress.cpp:172-186):
 * after compressing d_grad into numel (idx, val) slots, zero d_grad at every
 * d_idx[i], i < numel (unwritten slots hold index 0, so element 0 is zeroed
 * too, as in the reference), and copy the bucket into d_residual.  Both
 * arrays end identical.  Asynchronous on `stream`. */
int stg_error_feedback_device(float *d_grad, size_t n, const uint32_t *d_idx, size_t numel, float *d_residual,
                              void *stream);

/* Sparse SGD (optim/sgd.cpp:34-263 scalar path; options sgd.cpp:265-300).
 * optimize_raw() keeps one momentum buffer per `name` on the device. */
int stg_sgd_create(int device, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                   int maximize, stg_sgd_t *out);
int stg_sgd_destroy(stg_sgd_t o);
int stg_sgd_optimize_raw_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len,
                                const float *d_grad, const uint32_t *d_idx, uint32_t grad_len,
                                const uint32_t *d_grad_len, void *stream);
int stg_sgd_get_momentum(stg_sgd_t o, const char *name, float *host_out, uint32_t len, void *stream);
/* Smart momentum, SGD::configure("smart_momentum", bool) (sgd.cpp:291-292):
 * an element's buffer decays by pow(momentum, iterations since its index was
 * last touched) instead of by momentum (sgd.cpp:225-227, 258-259).  The
 * iteration count belongs to the handle, not to a name: every optimize_raw /
 * merge_optimize call advances it, whatever the name and even with no
 * gradients (sgd.cpp:262).  Legal at any time; a name's last-touched array is
 * created zeroed by the first call that runs with the option on (the
 * reference's stays zero while the option is off).  The factors are a table
 * computed by the host's libm when the option is first enabled and kept on the
 * device until destroy.  STG_ERR_INVALID unless 0 < momentum < 1 (the
 * reference reads a null array at momentum 0 and asserts on factors outside
 * [0, 1)); STG_ERR_UNSUPPORTED when the table would pass 2^22 entries (momentum
 * above ~0.99997).  An index repeated within one call at an iteration > 0 has
 * the factor pow(momentum, 0) == 1, on which the reference asserts: that
 * element is skipped and the handle's failure word set (stg_sgd_check). */
int stg_sgd_set_smart_momentum(stg_sgd_t o, int on);
/* The name's last-touched iterations (min(len, param_len) words) after
 * synchronising `stream`; STG_ERR_INVALID before the name's first call with
 * the option on. */
int stg_sgd_get_last(stg_sgd_t o, const char *name, uint32_t *host_out, uint32_t len, void *stream);
/* The handle's iteration count: calls made so far (m_iter). */
int stg_sgd_get_iter(stg_sgd_t o, uint32_t *out);
/* Synchronises `stream` and reports the handle's sticky device failure word:
 * STG_ERR_DEVICE if a smart-momentum element was ever skipped, else STG_OK. */
int stg_sgd_check(stg_sgd_t o, void *stream);
/* ModuleCpuOptimize::run (engine/modules/cpu_optimize.cpp:26-100): the MERGE
 * decompress of the received stream (as stg_scatter_merge_device: d_out_idx /
 * d_out_val / d_out_count get the merged stream, param_len is n) followed by
 * SparseOptimizer::optimize_raw of `o` on it (sgd.cpp:34-263), in one call.
 * world == 1: two launches, the election and the emission with every winner's
 * step in the same pass (each index is elected once, so the updates commute;
 * parameters and momentum bitwise equal to the two separate calls); world > 1:
 * the two calls, the step's length read from d_out_count on the device. */
int stg_merge_optimize_sgd_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len,
                                  const uint32_t *d_idx, const float *d_val, size_t per_rank, int world,
                                  float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                  uint32_t *d_out_count, void *stream);
/* The same with Adam (adam.cpp:19-86): world 1 without amsgrad runs the step
 * inside the emission launch; amsgrad (its running maximum is an ordered scan)
 * and world > 1 run the decompress, then stg_adam_optimize_raw_device. */
int stg_merge_optimize_adam_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                   const uint32_t *d_idx, const float *d_val, size_t per_rank, int world,
                                   float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                   uint32_t *d_out_count, void *stream);

/* Sparse Adam (optim/adam.cpp:19-86; options Adam::configure adam.cpp:90-122,
 * defaults adam.h:21-23, lr sparse_optimizer.h:30).  optimize_raw() keeps per
 * `name` the m and v arrays (param_len floats, zeroed), the amsgrad running
 * max vmax (a float, 0) on the device and the tick (1, +1 per call) on the
 * host, as adam.cpp:28-35,81-82.  Indices must be unique within a call (every
 * codec output and the MERGE union are); with amsgrad grad_len <= param_len.
 * Calls on one name are serialised by the caller's stream (the reference holds
 * a mutex, adam.cpp:47).  get_state copies m, v (len floats each) and vmax to
 * the host after synchronising `stream`, and returns the next call's tick
 * through *tick_out; STG_ERR_INVALID before the name's first call. */
int stg_adam_create(int device, float lr, float b1, float b2, float eps, float weight_decay, int amsgrad,
                    int maximize, stg_adam_t *out);
int stg_adam_destroy(stg_adam_t o);
int stg_adam_optimize_raw_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                 const float *d_grad, const uint32_t *d_idx, uint32_t grad_len,
                                 const uint32_t *d_grad_len, void *stream);
int stg_adam_get_state(stg_adam_t o, const char *name, float *host_m, float *host_v, uint32_t len,
                       float *host_vmax, uint32_t *tick_out, void *stream);
/* Synchronises `stream` and reports the handle's sticky device failure word:
 * STG_ERR_DEVICE if an amsgrad look-back ever timed out (its updates used an
 * incomplete running max), STG_OK otherwise. */
int stg_adam_check(stg_adam_t o, void *stream);

/* Intra-node gather-add before the codec (ModuleCpuGather::run,
 * engine/modules/cpu_gather.cpp:59-87, add_arrays misc/array_util.h:12-54).
 * stg_gather_slice gives local rank r's slice [n*r/N, n*(r+1)/N).  add: over
 * that slice, d_grad0 += d_residual, then += d_grads[1], ..., d_grads[N-1]
 * (d_grads is a host array of N device pointers; [0] is ignored, it is
 * d_grad0), in that order per element, in one pass.  Sources may be peer
 * GPUs' buffers when P2P access is enabled (xGMI).  d_residual may be null
 * (no residual term; differs from adding zeros only for -0.0 elements).
 * N <= 16.  Async on `stream`. */
int stg_gather_slice(uint64_t n, int local_rank, int num_gpus, uint64_t *start, uint64_t *end);
int stg_gather_add_device(float *d_grad0, const float *d_residual, const float *const *d_grads, int num_gpus,
                          uint64_t n, int local_rank, void *stream);

/* Wire format of the compressed stream (engine/comm_manager.cpp:486-590).
 * stg_wire_flag returns the flag byte queueTx would send (comm_manager.cpp:
 * 573-590, comm_manager.h:24-25): STG_WIRE_U16_IDX when tensor_numel < 65536,
 * STG_WIRE_F16_VAL when fp16_values (FP16_COMPRESSION, config.h:64).
 * encode writes numel indices as uint16 (flag & 1) or uint32 and numel values
 * as fp16 bits (flag & 2) or float; decode is the receiver's inverse
 * (comm_manager.cpp:877-906).  Both reproduce the reference's bytes exactly,
 * including its SIMD-block / scalar-tail differences (wire.hip).  NaNs cross
 * quiet in both directions, as the x86 conversions leave them: a float32 NaN
 * is sent as sign | 0x7e00 | payload >> 13; a received fp16 NaN, signalling
 * or quiet, becomes the float32 NaN sign | 0x7fc00000 | payload << 13 (0x7c01
 * -> 0x7fc02000).  The same holds wherever a 16-bit stream is read in place
 * (the MERGE calls below).  Async. */
#define STG_WIRE_U16_IDX 0x01
#define STG_WIRE_F16_VAL 0x02
int stg_wire_flag(uint64_t tensor_numel, int fp16_values);
int stg_wire_encode_device(const uint32_t *d_idx, const float *d_val, size_t numel, int flag, void *d_idx_out,
                           void *d_val_out, void *stream);
int stg_wire_decode_device(const void *d_idx_in, const void *d_val_in, size_t numel, int flag, uint32_t *d_idx,
                           float *d_val, void *stream);

/* One wire stream of a batched encode: the arguments of one encode call. */
typedef struct stg_wire_stream {
    const uint32_t *d_idx;
    const float *d_val;
    size_t numel;
    int flag;
    void *d_idx_out;
    void *d_val_out;
} stg_wire_stream_t;

/* Batched stg_wire_encode_device: the same bytes as encoding streams[0..n-1]
 * one by one (the tx queue of one iteration, comm_manager.cpp:573-640), in
 * launches of up to 16 streams instead of one launch per stream. */
int stg_wire_encode_batch_device(const stg_wire_stream_t *streams, size_t nstreams, void *stream);

/* One received stream of a batched decode: the arguments of one decode call. */
typedef struct stg_wire_rx {
    const void *d_idx_in;
    const void *d_val_in;
    size_t numel;
    int flag;
    uint32_t *d_idx;
    float *d_val;
} stg_wire_rx_t;

/* Batched stg_wire_decode_device: the same bytes as decoding streams[0..n-1]
 * one by one, in launches of up to 16 streams (for consumers that want the
 * decoded pairs; the MERGE calls below read the wire form themselves). */
int stg_wire_decode_batch_device(const stg_wire_rx_t *streams, size_t nstreams, void *stream);

/* One rank's received stream of a MERGE decompress, where it landed and in
 * the form it arrived in: per_rank u16 (flag & STG_WIRE_U16_IDX) or u32
 * indices, per_rank fp16 bits (flag & STG_WIRE_F16_VAL) or floats; flag as
 * stg_wire_flag returns it. */
typedef struct stg_rank_stream {
    const void *d_idx;
    const void *d_val;
    int flag;
} stg_rank_stream_t;

/* The MERGE decompress and the fused optimizer steps straight from received
 * streams (the receiver's decode, comm_manager.cpp:877-906, inside the merge's
 * own loads).  The results -- the merged stream and its count, parameters,
 * optimizer state, iteration count -- are bitwise those of
 * stg_wire_decode_device(per_rank, ranks[r].flag) of every rank into position
 * r * per_rank of one u32 / f32 buffer followed by the decoded entry point
 * (stg_scatter_merge_device, stg_merge_optimize_{sgd,adam}_device), without
 * the `world` decode launches and that buffer.  The decode is by position:
 * pair i < 8 * ((per_rank - 1) / 8) sign-extends its u16 index (one >= 0x8000
 * becomes >= n and is dropped) and widens its fp16 value; the last 1..8 pairs
 * zero-extend and take (float) of the 16-bit integer.  `ranks` is a host array
 * of `world` entries read at call time; the buffers need not be adjacent, and
 * a 16-bit buffer needs only 2-byte alignment (8-byte aligned ones are read
 * four pairs per load) and is never read past pair per_rank - 1.  With every
 * flag 0 this is the decoded call over separate buffers.  Scratch, failure
 * word, check and release are those of stg_scatter_merge_device.
 * STG_ERR_INVALID before any device call: world < 1, null `ranks` or a null
 * buffer with per_rank > 0, a flag outside 0..3, missing or misaligned
 * d_dense / d_mark at world > 1. */
int stg_scatter_merge_wire_device(const stg_rank_stream_t *ranks, size_t per_rank, int world, size_t n,
                                  float *d_dense, uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                  uint32_t *d_out_count, void *stream);
int stg_merge_optimize_sgd_wire_device(stg_sgd_t o, const char *name, float *d_param, uint32_t param_len,
                                       const stg_rank_stream_t *ranks, size_t per_rank, int world, float *d_dense,
                                       uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                       uint32_t *d_out_count, void *stream);
int stg_merge_optimize_adam_wire_device(stg_adam_t o, const char *name, float *d_param, uint32_t param_len,
                                        const stg_rank_stream_t *ranks, size_t per_rank, int world, float *d_dense,
                                        uint8_t *d_mark, uint32_t *d_out_idx, float *d_out_val,
                                        uint32_t *d_out_count, void *stream);

/* One ModuleCpuOptimize task of a batched call: the arguments of one
 * stg_merge_optimize_{sgd,adam}_wire_device call (param_len is n; `ranks` is a
 * host array of `world` entries, flag 0 = decoded u32 / f32). */
typedef struct stg_merge_task {
    const char *name;               /* optimizer state name                         */
    float *d_param;
    uint32_t param_len;
    const stg_rank_stream_t *ranks; /* `world` entries                              */
    size_t per_rank;
    int world;
    float *d_dense;                 /* world > 1 only, as stg_scatter_merge_device  */
    uint8_t *d_mark;
    uint32_t *d_out_idx;
    float *d_out_val;
    uint32_t *d_out_count;
} stg_merge_task_t;                 /* 88 bytes on LP64; d_dense at offset 48       */

/* The engine's per-iteration ModuleCpuOptimize tasks (one per parameter
 * tensor, cpu_optimize.cpp:26-106) in one call.  The results -- parameters,
 * momentum, last-touched words, m / v, every task's merged stream and count,
 * the SGD handle's iteration count, each name's Adam tick, the failure words
 * -- are bitwise those of stg_merge_optimize_{sgd,adam}_wire_device on
 * tasks[0 .. ntasks-1] in order on `stream`.  Task i runs at iteration
 * iter0 + i (smart momentum sees the factor it would see one by one); the
 * iterations and ticks of the whole batch are reserved under one hold of the
 * handle's lock.
 *   Batched: tasks with world == 1, per_rank > 0 and an optimizer whose step
 * fuses into the emission (SGD plain and smart, Adam without amsgrad), in the
 * decoded or any wire form, flags mixed freely.  Up to 16 consecutive such
 * tasks share one election launch and one emission launch.  A launch also
 * closes when the sum of its tensors' param_len would pass 8 Mi (32 MiB of
 * winner words in the (device, stream) scratch of stg_scatter_merge_device; a
 * larger tensor runs alone on the words a per-tensor call would take), and
 * before a task whose name already occurs in it, so two tasks on one name run
 * in order as they would one by one.  Tensors of different names must not
 * overlap in memory (parameters, streams or outputs): tasks of one launch run
 * concurrently.
 *   Batched as well: tasks with world > 1, per_rank > 0 and such an optimizer.
 * Up to 16 consecutive tasks of the same world form a group that shares
 * world + 4 launches: world + 1 that scatter rank r - 1 and elect rank r of
 * every tensor (one launch per rank, so each element's sum keeps the rank
 * order), the mark count, its scan, and the emission with the step on every
 * emitted pair.  A group also closes on a change of world (or to world 1),
 * before a task whose name already occurs in it, and before the sum of its
 * tensors' param_len would pass 4 Mi.  It works on slices of the (device,
 * stream) scratch -- per tensor 2 n winner words, n dense floats and n mark
 * bytes, each slice 16-byte aligned, zero between calls (sizes: see
 * stg_scatter_merge_device) -- and not on the tasks' d_dense / d_mark, which
 * are still required and checked and stay zero; one dense / mark pair may
 * serve every task of the call.  A tensor of more than 4 Mi elements runs the
 * per-tensor sequence on the caller's scratch.
 *   Not batched: a task with per_rank == 0, a world > 1 task above that size,
 * and every task of an Adam handle with amsgrad, runs the per-tensor sequence
 * at its place in the order.
 *   All or nothing: every task is checked before any device call or state
 * change -- a null handle or name, a null `tasks` with ntasks > 0, the
 * conditions of stg_scatter_merge_wire_device, an empty parameter or 2^32
 * pairs, a param_len that differs from the name's first call.  A refused call
 * (STG_ERR_INVALID / STG_ERR_UNSUPPORTED) advances no iteration or tick,
 * creates no buffer and names the offending task index in stg_last_error().
 * This covers argument errors only: a HIP failure (STG_ERR_HIP; e.g. an
 * allocation of a name's state that fails) is found while the tasks are being
 * prepared or launched, and leaves the tasks before it with their iterations
 * and ticks taken, as a failing call in the per-tensor sequence would.
 * ntasks == 0 is STG_OK and does nothing.  A look-back that gives up poisons
 * its own tensor's count only and sets the scratch's sticky failure word
 * (stg_scatter_merge_check). */
int stg_merge_optimize_sgd_batch_device(stg_sgd_t o, const stg_merge_task_t *tasks, size_t ntasks, void *stream);
int stg_merge_optimize_adam_batch_device(stg_adam_t o, const stg_merge_task_t *tasks, size_t ntasks, void *stream);
/* *out: the kernel launches the two batched calls above have enqueued on
 * (current device, stream) since its scratch was created -- the shared launches
 * and the per-tensor sequences run at their place, their step launches
 * included -- counted as each launch is enqueued.  The results of a batched call
 * are those of the loop, so this is how a caller sees what was shared.  0 when
 * the stream has no scratch (yet, or after stg_scatter_merge_release).
 * STG_ERR_INVALID for a null `out`, before any device call. */
int stg_merge_batch_launches(void *stream, uint64_t *out);

/* Element types of a model replica (stg_replica_t.dtype). */
#define STG_DT_F32  0
#define STG_DT_BF16 1
#define STG_DT_F16  2

/* One model copy that receives a task's changed parameters: param_len elements
 * of `dtype` at d_param, aligned to the element size (no more is needed). */
typedef struct stg_replica {
    void *d_param;
    int dtype;                     /* STG_DT_*                                                 */
} stg_replica_t;                   /* 16 bytes on LP64: d_param at 0, dtype at 8               */

/* One parameter tensor of a publish call: the master copy a step has just
 * written, the step's merged stream (d_out_idx / d_out_count of
 * stg_merge_optimize_*), and the replicas to bring up to date. */
typedef struct stg_publish_task {
    const float *d_param;          /* the master parameter, param_len floats, read only        */
    uint32_t param_len;
    const uint32_t *d_idx;         /* the step's merged indices (its d_out_idx)                */
    const uint32_t *d_count;       /* device word: pairs in d_idx (its d_out_count)            */
    uint32_t idx_cap;              /* slots d_idx holds (per_rank * world): the grid's bound   */
    const stg_replica_t *replicas; /* host array, read at call time                            */
    int nreplicas;                 /* 1..16                                                    */
} stg_publish_task_t;              /* 56 bytes on LP64: d_param at 0, param_len at 8, d_idx at 16,
                                      d_count at 24, idx_cap at 32, replicas at 40, nreplicas at 48 */

/* Publishes a step's changed parameters to the node's model replicas: the
 * device form of ModuleH2DCopy::run (engine/modules/h2d_copy.cpp:31-56,
 * gpu_param_tensor.copy_(cpu_param_tensor) per GPU), for parameters that live
 * on the node master's GPU.  The sparse steps write a parameter only at the
 * indices of the merged stream (sgd.cpp:221-260, adam.cpp:19-86), so a replica
 * that equalled the parameter before the step equals it again after k element
 * stores instead of a dense copy of param_len.
 *   Per task, with c = *d_count read on the device: for every i < c with
 * j = d_idx[i] < param_len, and every replica r, replica_r[j] = cvt_r(d_param[j]).
 * cvt is the identity for STG_DT_F32 and round-to-nearest-even for
 * STG_DT_BF16 / STG_DT_F16 (overflow to inf, fp16 subnormals kept, a NaN stays
 * a NaN of unspecified payload).  Nothing else is written: an element whose
 * index is not among the first c slots is never stored to, not even with its
 * old value (peers may be reading their replica); slots c .. idx_cap-1 are
 * ignored; an index >= param_len is skipped, as the merge drops it; a
 * repeated index writes the same value twice.  c > idx_cap -- 0xffffffff, the
 * count a failed merge leaves, included -- publishes nothing for that task
 * (that failure is sticky in stg_scatter_merge_check).  idx_cap == 0 or
 * ntasks == 0 is STG_OK and launches nothing for it.
 *   Asynchronous on `stream` of the current device and ordered after the step
 * enqueued on it before.  A replica may be a peer GPU's memory when P2P access
 * is enabled (as the sources of stg_gather_add_device); the stores are
 * complete when the work on `stream` is, and making a peer's stream wait for
 * them (an event recorded on `stream`) is the caller's job.  Peer (xGMI)
 * replicas have not been run on hardware; tests and timings use replicas on
 * the master's GPU.
 *   Up to 16 tasks share one launch, workgroups of 1024 stream slots dealt to
 * the tasks in order; a launch also closes before its grid would pass 8
 * workgroups per compute unit (the bound of the send path's gather), and a
 * task larger than that runs in a launch of its own.  The grid is sized from
 * idx_cap; workgroups past c leave after reading the count.
 *   All or nothing: every task is checked before any device call, and a
 * refused call (STG_ERR_INVALID) names the task index in stg_last_error():
 * null `tasks` with ntasks > 0; nreplicas outside 1..16; an unknown dtype;
 * with idx_cap > 0 a null d_param, d_idx, d_count, replicas or replica
 * pointer, or param_len == 0; a replica pointer not aligned to its element. */
int stg_param_publish_batch_device(const stg_publish_task_t *tasks, size_t ntasks, void *stream);
/* Diagnostics, plain host arithmetic (no device): the launches a publish call
 * with these idx_cap values makes on a device of num_cu compute units (0 for
 * a null array with ntasks > 0 or num_cu < 1). */
int stg_debug_publish_launches(const uint32_t *idx_caps, size_t ntasks, int num_cu);

/* Diagnostics, plain host arithmetic (no device): the scan launches a
 * threshold-v stg_merge_send_batch_device call makes for tasks of n[i] floats
 * on a device of num_cu compute units.  launch_of[i]: the launch of task i
 * (0xffffffff for n[i] == 0: none); first_range[i]: its first workgroup
 * there (0 for a task that runs alone).  Returns the launch count, or
 * STG_ERR_INVALID for a null array with ntasks > 0 or num_cu < 1. */
int stg_debug_tv_batch_plan(const uint64_t *n, size_t ntasks, int num_cu, uint32_t *first_range,
                            uint32_t *launch_of);

/* Diagnostics, plain host arithmetic (no device): the select groups an exact
 * top-k stg_merge_send_batch_device call makes for tasks of n[i] floats on a
 * device of num_cu compute units -- the rule the entry point packs by.
 * launch[i]: the group of task i (0xffffffff for n[i] == 0: none);
 * first_tile[i]: its first tile (workgroup) there (0 for a task that runs
 * alone); *tile_cap: the tiles a group holds at most.  Returns the number of
 * groups, a task with more tiles than the cap counting as its own, or -1 for a
 * null array or num_cu <= 0. */
int stg_debug_topk_batch_plan(const uint64_t *n, size_t ntasks, int num_cu, uint32_t *first_tile, uint32_t *launch,
                              uint32_t *tile_cap);

/* Gather-add from bf16 / fp16 gradient sources.  The node's other GPUs may
 * hold 16-bit model replicas (stg_param_publish_batch_device keeps them
 * current) and so produce 16-bit gradients; these entry points read them as
 * they are, widened in the load, instead of from fp32 temporaries. */
typedef struct stg_grad_src {
    const void *d_grad;            /* n elements of `dtype`, aligned to the element size          */
    int dtype;                     /* STG_DT_*                                                    */
} stg_grad_src_t;                  /* 16 bytes on LP64: d_grad at 0, dtype at 8                   */

/* stg_gather_add_device / stg_merge_gather_compress_device /
 * stg_merge_send_batch_device with typed sources.  Per element, in the
 * reference's order (cpu_gather.cpp:59-87):
 *   acc = term0; if d_residual: acc += d_residual[e];
 *   for s = 1 .. N-1: acc += widen(srcs[s][e]);  d_grad0[e] = acc
 * term0 is d_grad0[e] (the bucket, bucket.d_src in the codec forms) when
 * srcs[0].d_grad is null, or STG_DT_F32 and equal to the bucket: today's
 * in-place form.  Otherwise term0 = widen(srcs[0][e]) and the bucket is
 * write-only, so a 16-bit local gradient needs no widening copy.  The bucket
 * and the residual stay fp32.  widen is the identity for STG_DT_F32,
 * bits << 16 for STG_DT_BF16, and for STG_DT_F16 the exact conversion
 * (vcvtph2ps: subnormals kept, -0 keeps its sign); a NaN source yields a NaN
 * of unspecified payload.  Sources are never written; nothing outside the
 * slice (stg_gather_slice) of the bucket is.
 *   Equivalence: widening is exact, so after a typed call the bucket, the
 * residual, the wire stream, the count and the key's AIMD state are bitwise
 * those of the fp32 entry point run on fp32 copies of the sources (the bucket
 * preloaded with the widened copy of a typed term0).
 *   stg_merge_send_batch_typed_device: srcs[i] is null -- task i then uses its
 * fp32 d_grads exactly as stg_merge_send_batch_device -- or a host array of
 * tasks[i].num_gpus typed sources, and tasks[i].d_grads is ignored (with
 * num_gpus == 1 the array holds only term0).  thresholdv16, threshold-v and
 * exact top-k.
 *   Routing: a call whose sources are all fp32 and in place runs the fp32
 * entry point's launches.  Otherwise 16-bit sources load 16 (or 8) bytes per
 * lane and fp32 streams 16, in lane groups of 8 (or 4) elements, wherever one
 * head length brings every pointer of the task to its alignment; else every
 * element is a scalar lane (stg_debug_gather_plan).  A lone task of
 * 2^22..2^24 elements with a 16-bit source or a typed term0 runs the typed
 * gather-add pass and then the plain scan instead of the scan that sums fp32
 * sources in its own pass; the results are the same bits.  Launch counts are
 * those of the fp32 entry points.
 *   All or nothing, as the fp32 entry points: every check precedes any device
 * call or key-state change and the send batch names the task index in
 * stg_last_error().  STG_ERR_INVALID: what the fp32 twin refuses (a null
 * `srcs` where it refuses a null d_grads), an unknown dtype, a source pointer
 * not aligned to its element size, a null source at index >= 1 with n > 0.
 * Peer (xGMI) sources have not been run on hardware; tests and timings use
 * sources on the bucket's GPU.  Async on `stream`. */
int stg_gather_add_typed_device(float *d_grad0, const float *d_residual, const stg_grad_src_t *srcs, int num_gpus,
                                uint64_t n, int local_rank, void *stream);
int stg_merge_gather_compress_typed_device(stg_codec_t h, const stg_bucket_t *bucket, float *d_residual,
                                           const stg_grad_src_t *srcs, int num_gpus, void *stream);
int stg_merge_send_batch_typed_device(stg_codec_t h, const stg_send_task_t *tasks,
                                      const stg_grad_src_t *const *srcs, size_t ntasks, void *stream);
/* Diagnostics, plain host arithmetic (no device): the plan a typed gather-add
 * takes for `nstreams` (1..18) streams -- the bucket, the residual and the
 * sources -- of element types dtypes[i], addrs[i] being stream i's address at
 * the first element of the range of n elements.  *width: elements per lane
 * group, 8 or 4, or 0 when no head length aligns every stream (all scalar,
 * *head = 0); *head: the scalar elements before the first group, < *width and
 * <= n.  After the head an fp32 stream is 16-byte aligned and a 16-bit stream
 * 2 * width bytes aligned (when head < n). */
int stg_debug_gather_plan(const uint64_t *addrs, const int *dtypes, size_t nstreams, uint64_t n, uint32_t *width,
                          uint32_t *head);

/* Synthetic fp32 buckets from the integer-only generator of SURVEY 8(d)
 * (dist 0 = D1, 1 = D2 heavy tail, 2 = D3 zeros with prob param/1e4);
 * bit-identical to oracle/stg_oracle.cpp:orc_synth_fill. */
int stg_synth_fill_device(float *d_dst, size_t n, uint64_t seed, int dist, uint32_t param, void *stream);

/* Thread-local message for the last failing call on this thread. */
const char *stg_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* STG_CODEC_H */
