/*
 * diloco_hip.h — C-ABI of libdiloco_hip.so, the MI355X (gfx950) implementation of the DiLoCo
 * outer-step pseudo-gradient sync of mikasenghaas/diloco-swarm.
 *
 * The reference has no native code and no FFI: its hot path is per-parameter torch CPU ops
 * plus one gloo all_reduce per tensor. Each entry point below names the reference code it
 * replaces (paths relative to the reference repository root). The Python host layer
 * (diloco-swarm_amd/diloco_amd) binds these symbols with ctypes; see INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns int: 0 = ok, <0 = DL_E_* argument/state error,
 *     >0 = the hipError_t passed through. dl_last_error() returns a thread-local message.
 *   - Pointers are plain device (or pinned host, where stated) addresses; no torch types.
 *   - Memory handed in is owned by the caller; the library owns only the tree handle's
 *     device tables (freed by dl_tree_destroy).
 *   - A "packed" buffer holds the tree's tensors back to back in parameters() order, each
 *     segment starting at a multiple of DL_ALIGN_ELEMS elements; padding is never written.
 *   - "bucket" selects one bucket of the plan; DL_ALL_BUCKETS (-1) selects the whole tree.
 *   - All kernels are stream-ordered on the hipStream_t passed in; no entry point
 *     synchronises the host with a stream (dl_tree_bind is asynchronous too).
 */
#ifndef DILOCO_HIP_H
#define DILOCO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DL_API __attribute__((visibility("default")))

#define DL_ABI_VERSION 8
#define DL_ALIGN_ELEMS 64      /* segment start alignment in the packed space: 256 B of fp32 */
#define DL_CHUNK_ELEMS 4096    /* work unit of every segment walker: 16 KiB of fp32 */
#define DL_ALL_BUCKETS (-1)
#define DL_MAX_SLOTS 4         /* per-tensor pointer tables per tree */
#define DL_Q8_SLOT_BYTES 4160  /* int8 wire: 64-B header (fp32 scale) + DL_CHUNK_ELEMS int8 */
#define DL_FP4_SLOT_BYTES 2176 /* fp4 wire: DL_CHUNK_ELEMS/32 scale bytes + DL_CHUNK_ELEMS/2 */

/* wire / packed dtypes */
#define DL_F32 0
#define DL_BF16 1
#define DL_F16 2
#define DL_U8 3 /* bytes (int8 wire slots); collectives only */

/* errors (negative); positive codes are hipError_t */
#define DL_OK 0
#define DL_E_ARG (-1)
#define DL_E_STATE (-2)
#define DL_E_ALIGN (-3)
#define DL_E_RCCL (-4) /* an RCCL call failed; dl_last_error() has its message */

typedef struct dl_tree_s* dl_tree_t;
typedef void* dl_stream_t; /* hipStream_t */
typedef void* dl_comm_t;   /* ncclComm_t of the RCCL selected by dl_rccl_load */

/* ---- planner (host only; needs no GPU) -------------------------------------------------
 * Replaces the reference's implicit layout: the per-tensor loop over model.parameters()
 * in src/comm.py:120-123 and src/utils.py:220,225. Input: numel of each tensor in
 * parameters() order. Output: seg_off[n+1] (element offsets, each start aligned to
 * align_elems), bkt_bounds[n_bkt+1] (segment indices; greedy split at tensor boundaries so
 * a bucket's padded size stays <= cap_elems unless a single tensor exceeds it; cap_elems<=0
 * = one bucket). bkt_bounds must hold n+1 entries. Bit-exact contract with
 * oracle/diloco_oracle.c:or_plan_tables. */
DL_API int dl_plan_tables(const int64_t* numel, int32_t n, int64_t cap_elems, int32_t align_elems,
                          int64_t* seg_off, int64_t* bkt_bounds, int32_t* n_bkt);
/* Same rule with every bucket starting at a multiple of bucket_align_elems (a positive
 * multiple of align_elems) and seg_off[n] rounded up to it, so each bucket's range
 * [seg_off[bkt_bounds[b]], seg_off[bkt_bounds[b+1]]) splits into equal, aligned shards for a
 * reduce-scatter over n peers (bucket_align = DL_ALIGN_ELEMS * n). bucket_align ==
 * align_elems is dl_plan_tables. */
DL_API int dl_plan_tables_ex(const int64_t* numel, int32_t n, int64_t cap_elems,
                             int32_t align_elems, int64_t bucket_align_elems, int64_t* seg_off,
                             int64_t* bkt_bounds, int32_t* n_bkt);

/* ---- tree handle ------------------------------------------------------------------------
 * One parameter tree on the current device: planner tables + the chunk table + DL_MAX_SLOTS
 * per-tensor device pointer tables. Created once per model (src/utils.py:213-216
 * get_outer_model / src/comm.py:81 TrainingComm.__init__ are the natural creation points). */
DL_API int dl_tree_create(const int64_t* numel, int32_t n, int64_t cap_elems, dl_tree_t* out);
/* dl_tree_create with the dl_plan_tables_ex bucket alignment (the sharded outer step). */
DL_API int dl_tree_create_ex(const int64_t* numel, int32_t n, int64_t cap_elems,
                             int64_t bucket_align_elems, dl_tree_t* out);
DL_API int dl_tree_destroy(dl_tree_t tree);
DL_API int dl_tree_query(dl_tree_t tree, int64_t* total_elems, int32_t* n_seg, int32_t* n_bkt,
                         int32_t* n_chunk);
DL_API int dl_tree_bucket_range(dl_tree_t tree, int32_t bucket, int64_t* elem_begin,
                                int64_t* elem_end);
DL_API int dl_tree_seg_off(dl_tree_t tree, int64_t* seg_off /* n_seg+1 */);
/* Chunk index range [chunk_begin, chunk_end) of a bucket (DL_ALL_BUCKETS: the whole tree). */
DL_API int dl_tree_bucket_chunks(dl_tree_t tree, int32_t bucket, int32_t* chunk_begin,
                                 int32_t* chunk_end);
/* Upload the device addresses of the n_seg tensors of one slot (e.g. inner params, grads).
 * fp32 tensors, contiguous; a 16-B-misaligned address takes the scalar path. Stream-ordered
 * on `stream` and asynchronous for the host: the n_seg addresses are staged in a ring of
 * pinned slots and expanded into the slot's per-chunk table by a kernel, so rebinding grads
 * that torch reallocated (zero_grad(set_to_none=True) before every inner step,
 * src/train.py:164) costs no host synchronisation. Kernels queued on `stream` before the
 * call still see the previous table. A bind or kernel that uses a slot on another stream than
 * the slot's previous bind or kernel first waits for that one (an event per slot), so a
 * table is never rewritten under, or read before, work the caller did not order. */
DL_API int dl_tree_bind(dl_tree_t tree, int32_t slot, const uint64_t* dev_ptrs, int32_t n,
                        dl_stream_t stream);
/* Launch shape of every walker kernel on this tree: max_blocks caps the grid (0 = one
 * workgroup per chunk, the default); flags = DL_TUNE_AUTO (the default: the measured
 * per-kernel choice -- NT loads everywhere; NT stores in the SGD kernels, dl_scatter,
 * dl_unpack_avg, dl_unpack_sgd_q8, dl_unpack_adamw_q8, dl_unpack_avg_q8 and the int8 encoders
 * (dl_delta_q8, dl_gather_q8 and their _ef forms), and in dl_delta_pack / dl_gather over launches of more
 * than 2^28 elements; plain stores for those two producers below that size, where the next
 * kernel or RCCL re-reads their output from the Infinity Cache) or DL_TUNE_NT_LOADS [|
 * DL_TUNE_NT_STORES] for every kernel. Plain loads, DL_TUNE_WT_STORES (write-through, sc1)
 * for every kernel and DL_TUNE_PAIRS exist only in the tuning build (make TUNING=1, dl_tuning_build() == 1);
 * the product library rejects them with DL_E_ARG. Results are identical for every setting;
 * only speed differs. */
#define DL_TUNE_NT_LOADS 1
#define DL_TUNE_NT_STORES 2
#define DL_TUNE_WT_STORES 8 /* write-through (sc1) stores; tuning build only */
/* tuning build only: two chunks per workgroup, both chunks' loads issued before the first
 * store, in the 2-read / 1-write kernels (dl_delta_pack, dl_gather; measured slower) */
#define DL_TUNE_PAIRS 16
#define DL_TUNE_AUTO (-1)
DL_API int dl_tree_tune(dl_tree_t tree, int32_t max_blocks, int32_t flags);
/* 1 in the tuning build (every load / store policy instantiated), 0 in the product library. */
DL_API int dl_tuning_build(void);

/* ---- hot-path kernels ----------------------------------------------------------------- */

/* a2: compute_pseudo_gradient, src/utils.py:218-221:
 *   wire[k] = outer_packed[k] - inner[seg][j]      (fp32 subtract; bf16 wire rounds RNE)
 * outer_packed: fp32 packed θ_outer; inner: slot `inner_slot`. 12 B/param (fp32 wire). */
DL_API int dl_delta_pack(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                         const float* outer_packed, void* wire, int32_t wire_dtype,
                         dl_stream_t stream);

/* a3 unpack: src/comm.py:122-123 `param.grad /= num_peers` after the SUM all-reduce:
 *   dst[seg][j] = wire[k] / divisor   (IEEE true division; divisor 1 = plain copy)
 * dst is slot `dst_slot` (per-tensor fp32) or, when dst_slot < 0, the packed fp32 buffer
 * dst_packed (may alias an fp32 wire). 8 B/param. */
DL_API int dl_unpack_avg(dl_tree_t tree, int32_t bucket, const void* wire, int32_t wire_dtype,
                         int32_t divisor, int32_t dst_slot, float* dst_packed,
                         dl_stream_t stream);

/* ---- gradient-norm clipping ---------------------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm), norm_type 2, as the training
 * loop calls it every step right after sync_gradients (src/train.py:255 after :251), on device
 * gradients bound to a slot. `partials` is a device array of n_chunk doubles (dl_tree_query),
 * indexed by the tree's chunk index; a bucket launch writes exactly its chunk range
 * (dl_tree_bucket_chunks). All sums are fp64 in a fixed order (dl_norm.hip; restated in
 * tests/clip_restatement.py), so the norm is a function of the values and the tensor sizes
 * only: not of addresses, the grid (dl_tree_tune) or the bucket split. Unlike torch's fp32
 * accumulation it does not overflow at |g| >~ 1.8e19.
 *
 * dl_grad_sumsq: partials[c] = Σ g² over chunk c of slot src_slot. One read, 4 B/param. */
DL_API int dl_grad_sumsq(dl_tree_t tree, int32_t bucket, int32_t src_slot, double* partials,
                         dl_stream_t stream);
/* dl_unpack_avg that also writes partials[c] = Σ over the fp32 values it stores (after the
 * division). The destination bytes are dl_unpack_avg's, the partials dl_grad_sumsq's on that
 * destination: the norm of the averaged gradients costs no pass of its own. 8 B/param. */
DL_API int dl_unpack_avg_sumsq(dl_tree_t tree, int32_t bucket, const void* wire,
                               int32_t wire_dtype, int32_t divisor, int32_t dst_slot,
                               float* dst_packed, double* partials, dl_stream_t stream);
/* One workgroup: out2[0] = norm = float(sqrt(Σ partials[0:n_partials))), out2[1] = the clip
 * coefficient in torch's fp32 operations: c = (1 / (norm + 1e-6f)) * max_norm (torch evaluates
 * `max_norm / tensor` as reciprocal then multiply), coef = c < 1 ? c : (c is NaN ? c : 1).
 * n_partials 0: norm 0. out2: two floats of device memory. */
DL_API int dl_norm_finish(const double* partials, int32_t n_partials, float max_norm,
                          float* out2, dl_stream_t stream);
/* g[seg][j] *= *coef in place on slot `slot`, coef read from device memory by the kernel (no
 * host synchronisation). *coef == 1.0f: the kernel touches no gradient memory at all, which
 * equals torch's multiplication by 1.0 bit for bit; a NaN or zero coefficient multiplies.
 * 8 B/param when it clips, none when it does not. */
DL_API int dl_scale_by(dl_tree_t tree, int32_t bucket, int32_t slot, const float* coef,
                       dl_stream_t stream);

/* a3+a4+a5 fused: unpack the summed wire, average, outer SGD (torch.optim.SGD
 * _single_tensor_sgd as built by src/utils.py:62-63 and stepped at src/train.py:267),
 * then sync_inner_model (src/utils.py:223-226):
 *   g = wire/divisor; buf = first ? g : (buf*m) + g; u = nesterov ? fma(buf,m,g) : buf
 *   θ = fma(u, -lr, θ); inner[seg][j] = θ      (momentum==0: θ = fma(g,-lr,θ), no buf)
 * inner_slot < 0 skips the inner write. 24 B/param (20 on the first step). */
DL_API int dl_unpack_sgd(dl_tree_t tree, int32_t bucket, const void* wire, int32_t wire_dtype,
                         int32_t divisor, float* outer_packed, float* mom_packed, float lr,
                         float momentum, int32_t nesterov, int32_t first_step,
                         int32_t inner_slot, dl_stream_t stream);

/* dl_unpack_sgd whose inner write MERGES instead of overwriting (Streaming DiLoCo, Douillard et
 * al. 2025: the exchange ran while the inner model moved on, so inner is pulled towards the new
 * θ rather than replaced by it). dl_unpack_sgd's arguments plus alpha:
 *   x = inner[seg][j]                     (as loaded, before any store of this launch)
 *   θ, buf                                exactly dl_unpack_sgd's
 *   inner[seg][j] = fma(alpha, x - θ, θ)  (x - θ one rounded fp32 subtract, then ONE fma)
 * i.e. alpha·x + (1 - alpha)·θ. No special case for non-finite values, IEEE rules apply: an Inf or
 * NaN inner element gives an Inf or NaN there and nowhere else. inner_slot must be a bound slot (below 0, or not bound:
 * DL_E_ARG); alpha must be finite with 0 <= alpha < 1 (else DL_E_ARG, dl_last_error() names alpha).
 * alpha == 0 IS dl_unpack_sgd (the same kernel: inner is not loaded, a NaN inner is overwritten).
 * θ, the momentum and the wire get byte for byte what dl_unpack_sgd gives them; nothing is loaded
 * or stored past a chunk's length and padding is never written; results do not depend on the
 * inner tensors' alignment, the grid (dl_tree_tune) or the bucket split. Under DL_TUNE_AUTO the
 * load / store policy is dl_unpack_sgd's. 28 B/param on the fp32 wire (16 read, 12 written; 24
 * on the first step, 20 at momentum 0), where dl_unpack_sgd(inner_slot -1) followed by a lerp of
 * every inner tensor moves 20 + 12. */
DL_API int dl_unpack_sgd_merge(dl_tree_t tree, int32_t bucket, const void* wire,
                               int32_t wire_dtype, int32_t divisor, float* outer_packed,
                               float* mom_packed, float lr, float momentum, int32_t nesterov,
                               int32_t first_step, int32_t inner_slot, float alpha,
                               dl_stream_t stream);

/* a2+a4+a5 at ONE peer (src/comm.py:118-119 skips the all-reduce and the division):
 *   g = θ - inner[seg][j]; SGD as dl_unpack_sgd; θ and inner[seg][j] <- new θ
 * One pass, the delta stays in registers: 24 B/param (20 on the first step) instead of 36
 * for dl_delta_pack + dl_unpack_sgd; bit-identical results. */
DL_API int dl_delta_sgd(dl_tree_t tree, int32_t bucket, int32_t inner_slot, float* outer_packed,
                        float* mom_packed, float lr, float momentum, int32_t nesterov,
                        int32_t first_step, dl_stream_t stream);

/* a2+a3+a4+a5 at ONE peer, keeping the pseudo-gradient: dl_delta_sgd that also writes the
 * packed wire (outer.grad of src/utils.py:221, as dl_delta_pack would):
 *   g = θ - inner[seg][j]; wire[k] = g (bf16 wire: RNE, and the SGD uses the rounded value);
 *   SGD as dl_unpack_sgd (divisor 1); θ and inner[seg][j] <- new θ
 * One pass: 28 B/param (fp32 wire; 24 on the first step) instead of 36 for dl_delta_pack +
 * dl_unpack_sgd, bit-identical to that pair (wire included). */
DL_API int dl_delta_pack_sgd(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                             float* outer_packed, void* wire, int32_t wire_dtype,
                             float* mom_packed, float lr, float momentum, int32_t nesterov,
                             int32_t first_step, dl_stream_t stream);

/* dl_delta_pack_sgd (fp32 wire) with the stores of θ and the momentum left out: the wire and
 * inner[seg][j] receive what dl_delta_pack_sgd gives them, outer_packed and mom_packed keep the
 * values they had. The step is then PENDING: (outer_packed, mom_packed, wire) and this call's
 * hyper-parameters determine its θ and momentum bit for bit, and one of two calls completes it:
 *   dl_unpack_sgd(wire, DL_F32, divisor 1, ..., the same lr / momentum / nesterov / first_step,
 *                 inner_slot -1)            θ and the momentum stored, nothing else touched
 *   dl_delta_pack_sgd_resume                the next outer step, below
 * 20 B/param (16 on the first step) instead of 28: of the 16 B a step writes only the wire's 4
 * are new information, and a written stream costs more than a read one. */
DL_API int dl_delta_pack_sgd_defer(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                                   float* outer_packed, float* wire, float* mom_packed, float lr,
                                   float momentum, int32_t nesterov, int32_t first_step,
                                   dl_stream_t stream);

/* The outer step after a pending one (dl_delta_pack_sgd_defer with the pending_* values):
 *   θ, buf <- the pending step's, recomputed from outer_packed, mom_packed and wire[k]
 *   g = θ - inner[seg][j]; wire[k] = g (in place: each element is read before it is written);
 *   SGD as dl_unpack_sgd (divisor 1) with lr, momentum, nesterov, first_step;
 *   outer_packed, mom_packed and inner[seg][j] stored
 * Bit-identical to dl_delta_pack_sgd twice. The two sets of hyper-parameters are independent;
 * mom_packed is needed when either momentum is not 0. 32 B/param (16 read, 16 written), so a
 * defer / resume pair moves 52 B/param where two dl_delta_pack_sgd move 56, with 24 instead
 * of 32 of them written. */
DL_API int dl_delta_pack_sgd_resume(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                                    float* outer_packed, float* wire, float* mom_packed,
                                    float pending_lr, float pending_momentum,
                                    int32_t pending_nesterov, int32_t pending_first_step,
                                    float lr, float momentum, int32_t nesterov,
                                    int32_t first_step, dl_stream_t stream);

/* a3+a4+a5 fused for an AdamW outer optimizer (src/utils.py:60-61, configs/optimizer/adamw.toml,
 * stepped at src/train.py:267): one element of torch's _single_tensor_adamw (amsgrad, maximize
 * and capturable off; beta1 > 0.5, where torch's lerp uses this formula), then sync_inner_model.
 * The caller computes the scalars in doubles exactly as torch does and narrows each to fp32
 * once: decay = 1 - lr*wd, w1 = 1 - beta1, w2 = 1 - beta2, neg_step_size = -(lr / (1 - beta1^t)),
 * bc2_sqrt = (1 - beta2^t)^0.5, t the step count after this step.
 *   g = wire/divisor                      (IEEE division; divisor 1: untouched)
 *   θ = θ*decay;  m = fma(w1, g - m, m);  v = v*beta2;  v = fma(w2*g, g, v)
 *   den = sqrt(v)/bc2_sqrt + eps          (correctly rounded sqrt and division)
 *   θ = θ + (neg_step_size*m)/den;  inner[seg][j] = θ
 * Every other operation rounds on its own. exp_avg (m) and exp_avg_sq (v) are packed fp32
 * buffers; zeros are the first step. inner_slot < 0 skips the inner write. 32 B/param (fp32
 * wire; 28 without the inner write). */
DL_API int dl_unpack_adamw(dl_tree_t tree, int32_t bucket, const void* wire, int32_t wire_dtype,
                           int32_t divisor, float* outer_packed, float* exp_avg_packed,
                           float* exp_avg_sq_packed, float decay, float w1, float beta2, float w2,
                           float neg_step_size, float bc2_sqrt, float eps, int32_t inner_slot,
                           dl_stream_t stream);

/* dl_unpack_adamw with dl_unpack_sgd_merge's inner write: θ, exp_avg and exp_avg_sq exactly
 * dl_unpack_adamw's, then inner[seg][j] = fma(alpha, x - θ, θ), x the inner value as loaded.
 * dl_unpack_adamw's arguments plus alpha; inner_slot, alpha, alpha == 0, the footprint and the
 * load / store policy as stated at dl_unpack_sgd_merge. 36 B/param on the fp32 wire (20 read, 16
 * written). */
DL_API int dl_unpack_adamw_merge(dl_tree_t tree, int32_t bucket, const void* wire,
                                 int32_t wire_dtype, int32_t divisor, float* outer_packed,
                                 float* exp_avg_packed, float* exp_avg_sq_packed, float decay,
                                 float w1, float beta2, float w2, float neg_step_size,
                                 float bc2_sqrt, float eps, int32_t inner_slot, float alpha,
                                 dl_stream_t stream);

/* a2+a3+a4+a5 at ONE peer for an AdamW outer optimizer, keeping the pseudo-gradient:
 *   g = θ - inner[seg][j]; wire[k] = g (bf16 wire: RNE, and AdamW uses the rounded value);
 *   AdamW as dl_unpack_adamw (divisor 1); θ and inner[seg][j] <- new θ
 * One pass: 36 B/param (fp32 wire: 16 read, 20 written) instead of 12 + 32 for dl_delta_pack +
 * dl_unpack_adamw, bit-identical to that pair (wire included). */
DL_API int dl_delta_pack_adamw(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                               float* outer_packed, void* wire, int32_t wire_dtype,
                               float* exp_avg_packed, float* exp_avg_sq_packed, float decay,
                               float w1, float beta2, float w2, float neg_step_size,
                               float bc2_sqrt, float eps, dl_stream_t stream);

/* The INNER optimizer's AdamW step (src/train.py:257, every training step, right after
 * clip_grad_norm_ at :255) on the inner model's own tensors, one pass:
 *   g' = coef ? g[seg][j] * *coef : g[seg][j]   (a separate, rounded fp32 multiply)
 *   one element of dl_unpack_adamw's arithmetic on θ = param[seg][j], m = exp_avg[k],
 *   v = exp_avg_sq[k] with g', its seven scalars in its order:
 *     θ = θ*decay;  m = fma(w1, g' - m, m);  v = v*beta2;  v = fma(w2*g', g', v)
 *     den = sqrt(v)/bc2_sqrt + eps;  θ = θ + (neg_step_size*m)/den
 * θ is read and written in place through param_slot (per-tensor storage), g is only read
 * through grad_slot; both slots must be bound. exp_avg and exp_avg_sq are packed fp32 arenas in
 * the tree's layout (16-B aligned; zeros are the first step; their padding is never written).
 * coef is a device pointer (dl_norm_finish's out2 + 1: the pending clip coefficient) or NULL;
 * the kernel reads it, so no host synchronisation. There is no special case for *coef == 1:
 * multiplying by 1 is the identity. coef = c equals dl_scale_by(c) followed by coef = NULL bit
 * for bit, without the gradients being written. Results do not depend on the tensors'
 * alignment, the grid or the bucket split. 28 B/param: g, θ, m, v read, θ, m, v written. */
DL_API int dl_adamw_step(dl_tree_t tree, int32_t bucket, int32_t param_slot, int32_t grad_slot,
                         float* exp_avg_packed, float* exp_avg_sq_packed, const float* coef,
                         float decay, float w1, float beta2, float w2, float neg_step_size,
                         float bc2_sqrt, float eps, dl_stream_t stream);

/* a2 -> a3 -> a4 -> a5 at ONE peer as the two-kernel pipeline (dl_delta_pack then
 * dl_unpack_sgd with divisor 1; src/utils.py:221, src/comm.py:118-119, src/train.py:267,
 * src/utils.py:226), cache-blocked: the bucket's chunk range is walked in tiles of
 * tile_chunks chunks (0 = one tile), each tile packed then stepped, so the unpack re-reads
 * the wire and θ bytes the pack just touched from the Infinity Cache. wire holds the
 * pseudo-gradient afterwards. Bit-identical to the two whole-range launches. */
DL_API int dl_pack_sgd_tiled(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                             float* outer_packed, void* wire, int32_t wire_dtype,
                             float* mom_packed, float lr, float momentum, int32_t nesterov,
                             int32_t first_step, int32_t tile_chunks, dl_stream_t stream);

/* Gather per-tensor fp32 (slot) into a packed buffer of dtype `dtype` (fp32 or bf16).
 * Used to pack device gradients (DP sync, src/comm.py:117-123 with device grads, called at
 * src/train.py:251) and to initialise the device θ_outer mirror (src/utils.py:215). */
DL_API int dl_gather(dl_tree_t tree, int32_t bucket, int32_t src_slot, void* packed,
                     int32_t dtype, dl_stream_t stream);

/* a5: sync_inner_model, src/utils.py:223-226: dst[seg][j] = packed[k] (fp32). */
DL_API int dl_scatter(dl_tree_t tree, int32_t bucket, const float* packed, int32_t dst_slot,
                      dl_stream_t stream);

/* a3 /n + a4 on one peer's shard after a reduce-scatter (the sharded variant):
 * flat contiguous arrays of n elements, no tree: g = wire[k] / divisor (divisor 1: untouched),
 * SGD exactly as dl_unpack_sgd on outer[k], mom[k]. The caller all-gathers `outer` and
 * scatters it to the inner params (dl_scatter) afterwards. 20 B/param of the shard. All
 * pointers 16-B aligned. */
DL_API int dl_shard_sgd(const void* wire, int32_t wire_dtype, int32_t divisor, float* outer,
                        float* mom, int64_t n, float lr, float momentum, int32_t nesterov,
                        int32_t first_step, dl_stream_t stream);

/* a3 (Σ, /n) + a4 on one peer's shard after an all_to_all instead of a reduce-scatter
 * (OuterSync(exchange="a2a")): `slices` holds n_slices equal slices of `len` elements
 * (wire dtype), slice q = rank q's copy of this peer's shard of the bucket
 * (src/comm.py:122 `all_reduce(SUM)` + :123 `/= num_peers`, then the SGD of src/train.py:267).
 * g = ((s_0 + s_1) + ... + s_{n-1}) / n in fp32 in rank order -- deterministic and identical
 * on every rank, bit-exact against oracle/or_sum_avg at every n (a bf16 wire is summed in
 * fp32 and never re-rounded) -- then dl_shard_sgd's SGD on outer[k], mom[k]. len a multiple
 * of 4; all pointers 16-B aligned. Reads n·sizeof(wire) + 8 B, writes 8 B per element. */
DL_API int dl_shard_reduce_sgd(const void* slices, int32_t wire_dtype, int32_t n_slices,
                               int64_t len, float* outer, float* mom, float lr, float momentum,
                               int32_t nesterov, int32_t first_step, dl_stream_t stream);

/* The same rank-order average without the SGD, for the ordered per-step DP gradient sync
 * (GradSync(exchange="a2a"), src/comm.py:120-123 on device grads): out[k] =
 * ((s_0[k] + s_1[k]) + ... + s_{n-1}[k]) / n in fp32. len a multiple of 4; 16-B aligned. */
DL_API int dl_shard_reduce_avg(const void* slices, int32_t wire_dtype, int32_t n_slices,
                               int64_t len, float* out, dl_stream_t stream);

/* dl_shard_sgd with the AdamW rule: a3 /n + AdamW on one peer's shard after a reduce-scatter.
 * Flat contiguous arrays of n elements, no tree and no inner write: g = wire[k] / divisor
 * (divisor 1: untouched), then one element of dl_unpack_adamw on outer[k], exp_avg[k],
 * exp_avg_sq[k], with its seven scalars in its order. The same body as dl_unpack_adamw over a
 * flat shard, so bit-identical to it. The caller all-gathers `outer` and scatters it to the
 * inner params (dl_scatter) afterwards; exp_avg and exp_avg_sq stay this peer's shards.
 * 28 B per shard element (fp32 wire: 16 read, 12 written). All pointers non-null and 16-B
 * aligned. */
DL_API int dl_shard_adamw(const void* wire, int32_t wire_dtype, int32_t divisor, float* outer,
                          float* exp_avg, float* exp_avg_sq, int64_t n, float decay, float w1,
                          float beta2, float w2, float neg_step_size, float bc2_sqrt, float eps,
                          dl_stream_t stream);

/* dl_shard_reduce_sgd with the AdamW rule: a3 (Σ, /n) + AdamW on one peer's shard after an
 * all_to_all. `slices` as for dl_shard_reduce_sgd; g = ((s_0 + s_1) + ... + s_{n-1}) / n in
 * fp32 in rank order (n_slices 1: no division; a bf16 wire is summed in fp32 and never
 * re-rounded), avg_out[k] = g when avg_out (fp32) is not NULL -- the average a later .grad
 * read shows -- then one element of dl_unpack_adamw on outer[k], exp_avg[k], exp_avg_sq[k].
 * len a multiple of 4; every pointer 16-B aligned, the two state pointers non-null. Reads
 * n·sizeof(wire) + 12 B, writes 12 B (+ 4 with avg_out) per element. */
DL_API int dl_shard_reduce_adamw(const void* slices, int32_t wire_dtype, int32_t n_slices,
                                 int64_t len, float* outer, float* exp_avg, float* exp_avg_sq,
                                 float* avg_out, float decay, float w1, float beta2, float w2,
                                 float neg_step_size, float bc2_sqrt, float eps,
                                 dl_stream_t stream);

/* ---- int8 wire codec (not in the reference) --------------------------
 * One DL_Q8_SLOT_BYTES slot per chunk of the bucket, in chunk order: fp32 scale at byte 0,
 * zeros to byte 64, int8 values at byte 64, zeros past the chunk's length. The encoders
 * (dl_delta_q8, dl_delta_q8_ef) and the reduces write every byte of each slot they are launched
 * on -- the whole 64-B header and all DL_CHUNK_ELEMS payload bytes, zeros past the chunk's
 * length -- whatever the slot held before, and no byte of any other slot. Only the slots no
 * chunk owns (the zero slots that pad a bucket to a multiple of the peer count) are never
 * written: the caller zeroes those once.
 * Quantiser: s = amax/127, q = s == 0 ? 0 : clamp(rint(x/s), -127, 127), value q*s.
 * dl_delta_q8:      slots <- quantise(outer - inner) per chunk  (a2, 8 B read + 1.02 B written)
 * dl_q8_reduce:     out[j] <- quantise((sum_r deq(recv[r][j])) / divisor), r in rank order;
 *                   recv holds n_peers x n_slots slots; out may alias recv when n_peers == 1
 * dl_unpack_sgd_q8: g = deq(slot); SGD and copy-back exactly as dl_unpack_sgd (divisor 1).
 * dl_unpack_adamw_q8: the AdamW twin of dl_unpack_sgd_q8, below. */
DL_API int dl_delta_q8(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                       const float* outer_packed, void* slots, dl_stream_t stream);
DL_API int dl_q8_reduce(const void* recv, int32_t n_peers, int32_t n_slots, int32_t divisor,
                        void* out, dl_stream_t stream);
/* Error feedback for the two lossy stages (off unless the caller uses these entry points): what
 * rounding removed is kept in an fp32 residual and added to the next outer step's value, so an
 * element that stays below s/2 of its chunk is transmitted late instead of never. Each fp32
 * operation rounds on its own.
 * dl_delta_q8_ef, per chunk c of the bucket and element k of the packed space:
 *   d = outer[k] - inner[seg][j]          (as dl_delta_q8)
 *   x = d + r[k]                          (r = residual_packed: fp32, the tree's packed layout)
 *   s = amax_chunk(|x|) / 127             (fmaxf: a NaN is ignored by the scale)
 *   q = s == 0 ? 0 : clamp(rint(x / s), -127, 127)
 *   slot(c) <- header(s), int8 q          (byte for byte what dl_delta_q8 writes for this x)
 *   r[k] <- x - (float(q) * s)            (the product dl_unpack_*_q8 decode, then one subtract)
 * r is read and written in place; of θ, inner and r nothing is loaded or stored past a chunk's
 * length (the residual's padding is never written); the slot is written whole, as by
 * dl_delta_q8, zeros past the length. Results do not depend on the inner tensors' alignment,
 * the grid or the bucket split. Non-finite values
 * get no special case: a NaN/Inf element of d leaves a NaN (or Inf) residual, by IEEE rules,
 * until the caller resets the residual to zero. slots, outer_packed and residual_packed
 * non-null and 16-B aligned; the slot bound. 17.02 B/param: 12 read, 1.016 + 4 written.
 * dl_q8_reduce_ef, on the owner of the n_slots slots:
 *   acc = sum_r deq(recv[r][j]) in rank order; if divisor > 1: acc /= divisor (as dl_q8_reduce)
 *   x = acc + r2[j*DL_CHUNK_ELEMS + i]; s, q as above over all DL_CHUNK_ELEMS values;
 *   out slot j <- (s, q);  r2[...] <- x - float(q) * s
 * residual: fp32, n_slots * DL_CHUNK_ELEMS elements, 16-B aligned. A zero padding slot and the
 * zero tail of a short chunk give x = q = r2 = 0 and stay zero. out may alias recv only at
 * n_peers == 1. Every peer still receives byte-identical averaged slots. */
DL_API int dl_delta_q8_ef(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                          const float* outer_packed, float* residual_packed, void* slots,
                          dl_stream_t stream);
DL_API int dl_q8_reduce_ef(const void* recv, int32_t n_peers, int32_t n_slots, int32_t divisor,
                           float* residual, void* out, dl_stream_t stream);
DL_API int dl_unpack_sgd_q8(dl_tree_t tree, int32_t bucket, const void* slots,
                            float* outer_packed, float* mom_packed, float lr, float momentum,
                            int32_t nesterov, int32_t first_step, int32_t inner_slot,
                            dl_stream_t stream);
/* a4+a5 for an AdamW outer optimizer after the int8 exchange: one pass over the averaged slots
 * of a bucket (slot of chunk c at (c - first chunk of the bucket) * DL_Q8_SLOT_BYTES; the
 * whole tree with DL_ALL_BUCKETS). Per element k of the packed space:
 *   g = float(int8 q) * s                 (one rounded fp32 multiply: the product
 *                                          dl_unpack_sgd_q8 forms, the decoded .grad value)
 *   one element of dl_unpack_adamw's arithmetic (divisor 1), its seven scalars in its order,
 *   on θ = outer[k], m = exp_avg[k], v = exp_avg_sq[k];  inner[seg][j] = θ
 * so it is bit-identical to decoding the slots into an fp32 wire and running dl_unpack_adamw
 * on it. The slots are only read. inner_slot < 0 skips the inner write. Nothing is stored
 * past a chunk's length: the padding of the packed buffers is never written. Results do not
 * depend on the inner tensors' alignment, the grid or the bucket split. slots, outer and both
 * state pointers non-null and 16-B aligned. 29.02 B/param: 1.016 + 12 read, 12 + 4 written
 * (25.02 without the inner write). */
DL_API int dl_unpack_adamw_q8(dl_tree_t tree, int32_t bucket, const void* slots,
                              float* outer_packed, float* exp_avg_packed,
                              float* exp_avg_sq_packed, float decay, float w1, float beta2,
                              float w2, float neg_step_size, float bc2_sqrt, float eps,
                              int32_t inner_slot, dl_stream_t stream);
/* The gradient side of the int8 exchange: the per-step DP average of device gradients
 * (src/train.py:249-251) over the same slots, reduces (dl_q8_reduce, dl_q8_reduce_ef with
 * divisor n_peers) and collectives as the pseudo-gradient's. Slot of chunk c at (c - first
 * chunk of the bucket) * DL_Q8_SLOT_BYTES; the whole tree with DL_ALL_BUCKETS.
 * dl_gather_q8, per chunk c of the bucket, g = slot src_slot (per-tensor fp32):
 *   slot(c) <- header(s), int8 q of x = g[seg][j]     (s, q: the quantiser above)
 * byte for byte what dl_delta_q8 writes for outer = g, inner = +0 (x - (+0) = x bit for bit).
 * 5.02 B/param: 4 read, 1.016 written.
 * dl_gather_q8_ef, with the encoder's residual r = residual_packed (fp32, the packed layout):
 *   x = g[seg][j] + r[k];  slot(c) <- header(s), int8 q of x;  r[k] <- x - (float(q) * s)
 * dl_delta_q8_ef with d replaced by g; r is read and written in place by the same lane.
 * 13.02 B/param: 8 read, 1.016 + 4 written.
 * Both write every byte of each slot of the bucket -- the 64-B header whole, zeros past the
 * chunk's length -- whatever the slot held before, and no byte of any other slot; of g and r
 * nothing is loaded or stored past a chunk's length (the residual's padding is never written).
 * Results do not depend on the gradient tensors' alignment, the grid or the bucket split. A
 * NaN/Inf gradient leaves a NaN/Inf residual, by IEEE rules, until the caller resets it.
 * dl_unpack_avg_q8, per chunk c of the bucket, dst = slot dst_slot (per-tensor fp32):
 *   dst[seg][j] = float(int8 q) * s       (one rounded fp32 multiply: the product
 *                                          dl_unpack_sgd_q8 decodes)
 *   partials[c] = Σ over the values stored to chunk c, when partials is not NULL: fp64, in
 *                 dl_grad_sumsq's order, bit-identical to dl_grad_sumsq on dst afterwards;
 *                 written for exactly the bucket's chunk range (n_chunk doubles, 8-B aligned)
 * The slots are only read; nothing is stored past a tensor's length. 5.02 B/param: 1.016 read,
 * 4 written. slots and residual_packed non-null and 16-B aligned; the slot bound. */
DL_API int dl_gather_q8(dl_tree_t tree, int32_t bucket, int32_t src_slot, void* slots,
                        dl_stream_t stream);
DL_API int dl_gather_q8_ef(dl_tree_t tree, int32_t bucket, int32_t src_slot,
                           float* residual_packed, void* slots, dl_stream_t stream);
DL_API int dl_unpack_avg_q8(dl_tree_t tree, int32_t bucket, const void* slots, int32_t dst_slot,
                            double* partials, dl_stream_t stream);

/* ---- fp4 wire codec (OCP MX block-scaled E2M1, "MXFP4"; not in the reference) -----------
 * The pseudo-gradient exchange of the int8 wire at 4 bits: the same slot plan, collectives and
 * residual arenas, 0.531 B/param. One DL_FP4_SLOT_BYTES slot per chunk of the bucket, in chunk
 * order:
 *   bytes [0, 128)     one scale byte E per group g of 32 elements [32g, 32g + 32)
 *   bytes [128, 2176)  element i in byte 128 + i/2, low nibble for even i, high for odd i
 * A nibble is sign << 3 | code, code indexing {0, 0.5, 1, 1.5, 2, 3, 4, 6}. Elements past the
 * chunk's length count as +0: groups wholly past it are zero bytes, and an all-zero (padding)
 * slot decodes to zeros. The encoder and the reduce write every byte of each slot they are
 * launched on, whatever it held before, and no byte of any other slot.
 * Scale of a group, A = max over the group of (bits(x) & 0x7fffffff) as an unsigned integer
 * (monotone in |x|; a NaN is not dropped):
 *   A >= 0x7f800000 (a NaN or Inf in the group): E = 255, all 32 nibbles 0
 *   A == 0: E = 0, nibbles 0
 *   else, amax = float(A) = m * 2^k with m in [0.5, 1): e = k - 3 if m <= 0.75, else k - 2 --
 *   the smallest e with amax * 2^-e <= 6, so nothing saturates (the OCP rule
 *   floor(log2 amax) - 2 clamps amax * 2^-e in (6, 8)); E = max(0, e + 127) <= 253. A denormal
 *   amax is a value like any other.
 * Element: y = |x| * 2^(127 - E); code = the grid point nearest y, ties to the even code
 * (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the sign bit is set
 * only when code != 0 (nibble 8 never occurs).
 * Decode: E == 255: NaN for the group's 32 elements; else +-grid[code] * 2^(E - 127), exact in
 * fp32 for every E (2^-128, a denormal, is the smallest value; nothing flushes it). So
 * |x - deq| <= 2^(E - 127) < amax / 3 (E > 0), and deq(enc(deq(s))) == deq(s) bit for bit.
 * dl_delta_fp4, per chunk c of the bucket and element k of the packed space:
 *   x = outer[k] - inner[seg][j]           (residual_packed NULL)
 *   x = (outer[k] - inner[seg][j]) + r[k]  (r = residual_packed: two rounded fp32 operations)
 *   slot(c) <- enc(x);  r[k] <- x - deq(slot(c))   (one subtract, in place, by the same lane)
 * Nothing of θ, inner or r is loaded or stored past a chunk's length. Results do not depend on
 * the inner tensors' alignment, the grid or the bucket split. A non-finite group leaves NaN
 * residuals for its 32 elements until the caller resets the residual. 8.53 B/param (16.53 with
 * the residual).
 * dl_fp4_reduce, on the owner of n_slots slots (recv laid out [peer][slot]):
 *   acc = 0; acc = acc + deq(recv[r][j]) for r in rank order; if divisor > 1: acc /= divisor
 *   x = acc (+ r2[j*DL_CHUNK_ELEMS + i], residual not NULL);  out slot j <- enc(x);
 *   r2[...] <- x - deq(out slot j)         (all DL_CHUNK_ELEMS values of every slot)
 * out may alias recv only at n_peers == 1. Every peer receives byte-identical averaged slots.
 * (n_peers + 1) * 0.531 B per owned param (+ 8 with the residual).
 * dl_unpack_sgd_fp4 / dl_unpack_adamw_fp4: g = deq(slot), then one element of dl_unpack_sgd /
 * dl_unpack_adamw (divisor 1) and inner[seg][j] = θ (inner_slot < 0: no inner write): bit-
 * identical to decoding the slots into an fp32 wire and running those on it. The slots are only
 * read; nothing is stored past a chunk's length. 20.53 and 28.53 B/param (24.53 for AdamW
 * without the inner write). slots, outer, the state pointers (and a residual that is given)
 * 16-B aligned.
 * The gradient side (the per-step DP gradient average on this wire; dl_fp4_reduce with divisor
 * n stands between the two). dl_gather_fp4, per chunk c of the bucket, g = slot src_slot
 * (per-tensor fp32):
 *   x = g[seg][j]          (residual_packed NULL)
 *   x = g[seg][j] + r[k]   (r = residual_packed: one rounded fp32 add)
 *   slot(c) <- enc(x);  r[k] <- x - deq(slot(c))   (in place, by the lane that read it)
 * byte for byte what dl_delta_fp4 writes for outer = g, inner = +0 (x - (+0) = x bit for bit,
 * -0 included). Every byte of each slot of the bucket is written, whatever it held before --
 * scales and nibbles of groups past the chunk's length are zero -- and no byte of any other
 * slot; of g and r nothing is loaded or stored past a chunk's length (the residual's padding is
 * never written). Results do not depend on the gradient tensors' alignment, the grid or the
 * bucket split. 4.53 B/param: 4 read, 0.531 written; with the residual 12.53: 8 read,
 * 0.531 + 4 written.
 * dl_unpack_avg_fp4, per chunk c of the bucket, dst = slot dst_slot (per-tensor fp32):
 *   dst[seg][j] = deq(slot(c))[i]   (the exact power-of-two product above; an E = 255 group
 *                                    stores NaN)
 *   partials[c] = Σ of the squares of the values stored to chunk c, when partials is not NULL:
 *                 fp64, in dl_grad_sumsq's order, bit-identical to dl_grad_sumsq on dst
 *                 afterwards; written for exactly the bucket's chunk range (n_chunk doubles,
 *                 8-B aligned)
 * The slots are only read; nothing is stored past a tensor's length; results do not depend on
 * alignment, the grid or the bucket split. 4.53 B/param: 0.531 read, 4 written. slots non-null
 * and 16-B aligned, a given residual 16-B aligned; the slot bound. */
DL_API int dl_delta_fp4(dl_tree_t tree, int32_t bucket, int32_t inner_slot,
                        const float* outer_packed, float* residual_packed /* NULL: no EF */,
                        void* slots, dl_stream_t stream);
DL_API int dl_fp4_reduce(const void* recv, int32_t n_peers, int32_t n_slots, int32_t divisor,
                         float* residual /* NULL: no EF */, void* out, dl_stream_t stream);
DL_API int dl_unpack_sgd_fp4(dl_tree_t tree, int32_t bucket, const void* slots,
                             float* outer_packed, float* mom_packed, float lr, float momentum,
                             int32_t nesterov, int32_t first_step, int32_t inner_slot,
                             dl_stream_t stream);
DL_API int dl_unpack_adamw_fp4(dl_tree_t tree, int32_t bucket, const void* slots,
                               float* outer_packed, float* exp_avg_packed,
                               float* exp_avg_sq_packed, float decay, float w1, float beta2,
                               float w2, float neg_step_size, float bc2_sqrt, float eps,
                               int32_t inner_slot, dl_stream_t stream);
DL_API int dl_gather_fp4(dl_tree_t tree, int32_t bucket, int32_t src_slot,
                         float* residual_packed /* NULL: no EF */, void* slots,
                         dl_stream_t stream);
DL_API int dl_unpack_avg_fp4(dl_tree_t tree, int32_t bucket, const void* slots, int32_t dst_slot,
                             double* partials /* NULL: none */, dl_stream_t stream);

/* ---- serializer (src/serializer.py:11-15) ----------------------------------------------
 * out is fp32 of 2*numel elements: out[0] = meta0, out[1] = meta1, out[numel + i] =
 * float(src[i]) for src dtype DL_F32/DL_BF16/DL_F16. out[2..numel) is left unwritten, as
 * the reference leaves it uninitialised (torch.empty, src/serializer.py:12). numel >= 2. */
DL_API int dl_serialize(const void* src, int32_t src_dtype, int64_t numel, float meta0,
                        float meta1, float* out, dl_stream_t stream);
/* The fp64 frame (torch.cat promotes the fp32 metadata plane to the fp64 payload's dtype):
 * out is fp64 of 2*numel elements, out[0] = (double)meta0, out[1] = (double)meta1 (the
 * metadata rounds through fp32 first, as the reference's fp32 metadata tensor does),
 * out[numel + i] = src[i]. */
DL_API int dl_serialize_f64(const double* src, int64_t numel, float meta0, float meta1,
                            double* out, dl_stream_t stream);

/* ---- synthetic parameter trees (bench / tests) ------------------------------------------
 * dst[i] = base + u(seed, stream_id, i) * scale (+ add[i] if add != NULL), with
 * u = ((splitmix64(seed*0xD1B54A32D192ED03 + (stream_id<<40) + i) >> 40) - 2^23) * 2^-23,
 * all fp32 ops correctly rounded: bit-identical to diloco_amd.synth (numpy). */
DL_API int dl_fill_synth(float* dst, int64_t n, uint64_t seed, uint64_t stream_id, float base,
                         float scale, const float* add, dl_stream_t stream);
/* TEST SUPPORT, not part of the outer step: a slow producer for the ordering tests
 * (tests/test_async_order_gpu.py, the slow-producer cases of tests/test_dropin_gpu.py): one
 * workgroup that occupies `stream` for `ns` nanoseconds of the wall clock of the device
 * `stream` belongs to (at most 10 s), touching no memory. */
DL_API int dl_spin(uint64_t ns, dl_stream_t stream);

/* ---- RCCL ------------------------------------------------------------
 * The exchange of src/comm.py:122 for hosts that drive RCCL through this library instead of
 * torch.distributed. RCCL is resolved at run time: a communicator must be used with the
 * RCCL that created it (a PyTorch process carries its own; ProcessGroupNCCL._comm_ptr()
 * returns its ncclComm_t). dl_rccl_load(path): that library; NULL = the RCCL already loaded
 * in the process, else librccl.so.1. The other entry points load it on first use.
 * Collectives are SUM, enqueued on `stream`, dtype DL_F32 / DL_BF16 / DL_F16 / DL_U8. */
DL_API int dl_rccl_load(const char* path);
DL_API int dl_rccl_version(int32_t* version);
DL_API int dl_comm_unique_id(void* id /* 128 B, NCCL_UNIQUE_ID_BYTES */);
DL_API int dl_comm_init(dl_comm_t* comm, int32_t nranks, const void* id, int32_t rank);
DL_API int dl_comm_destroy(dl_comm_t comm);
/* in place: buf[0:count) <- Σ over the communicator's ranks (src/comm.py:122; /n is the
 * caller's, e.g. dl_unpack_sgd's divisor) */
DL_API int dl_allreduce(void* buf, int64_t count, int32_t dtype, dl_comm_t comm,
                        dl_stream_t stream);
/* recv[0:recv_count) <- Σ_ranks send[rank*recv_count : (rank+1)*recv_count) (sharded step) */
DL_API int dl_reduce_scatter(const void* send, void* recv, int64_t recv_count, int32_t dtype,
                             dl_comm_t comm, dl_stream_t stream);
/* recv[r*send_count : (r+1)*send_count) <- rank r's send[0:send_count) */
DL_API int dl_all_gather(const void* send, void* recv, int64_t send_count, int32_t dtype,
                         dl_comm_t comm, dl_stream_t stream);
/* Point-to-point, the payload leg of the device pipeline transport:
 * replaces src/comm.py:38 `dist.send(tensor.to("cpu"), dst)` and src/comm.py:67
 * `dist.recv(tensor, group)` (after the any-source header names the sender) with RCCL over
 * xGMI on device buffers. A send and a receive on the same rank (or several transfers that
 * must progress together) go between dl_group_start() and dl_group_end(). */
DL_API int dl_send(const void* buf, int64_t count, int32_t dtype, int32_t peer, dl_comm_t comm,
                   dl_stream_t stream);
DL_API int dl_recv(void* buf, int64_t count, int32_t dtype, int32_t peer, dl_comm_t comm,
                   dl_stream_t stream);
DL_API int dl_group_start(void);
DL_API int dl_group_end(void);

/* ---- direct peer-access exchange (one node; SURVEY §8e alternative to RCCL) ----------------
 * IPC: dl_ipc_handle(ptr) -> the handle of the allocation holding ptr + ptr's byte offset in
 * it; a peer maps it with dl_ipc_open (base address; add the offset) and unmaps with
 * dl_ipc_close(base). dl_can_access_peer: hipDeviceCanAccessPeer; dl_enable_peer_access:
 * hipDeviceEnablePeerAccess.
 * dl_xgmi_reduce_sgd: on rank `rank` of n (<= 8), for packed elements [lo, lo+len) (this rank's
 * shard; lo, len multiples of 4, buffers 16-B aligned): g = (Σ_q wires[q][k] in rank order)/n,
 * Nesterov SGD on thetas[rank][k] and mom[k - lo], then thetas[q][k] = θ for every q. wires /
 * thetas: host arrays of n device addresses (peers' IPC-mapped buffers). Order it between two
 * barriers of the n ranks: after every rank's wire is written, before any rank reads θ. */
#define DL_IPC_HANDLE_BYTES 64
DL_API int dl_ipc_handle(const void* ptr, void* handle, int64_t* offset);
DL_API int dl_ipc_open(const void* handle, void** base);
DL_API int dl_ipc_close(void* base);
DL_API int dl_can_access_peer(int32_t device, int32_t peer, int32_t* can);
/* hipDeviceEnablePeerAccess(peer) from the current device; already enabled is success */
DL_API int dl_enable_peer_access(int32_t peer);
/* Stream-ordered system-scope fence on every XCD of this GPU (L2 write-back + invalidate):
 * issue it after kernels whose stores peers will read over xGMI (before the barrier that
 * releases the peers), and after that barrier before reading what peers wrote here or
 * re-reading their memory. Coarse-grained (hipMalloc / PyTorch) buffers are otherwise
 * coherent across GPUs only at the runtime's own synchronisation points. */
DL_API int dl_sys_fence(dl_stream_t stream);
/* dl_sys_fence that also records, per workgroup, the XCD it ran on (HW_REG_XCC_ID, 0..7) into
 * the device array xcc[cap]; *grid = the workgroups launched (one per CU: multiProcessorCount).
 * Lets a test prove that the fence reached every XCD. */
DL_API int dl_sys_fence_census(uint32_t* xcc, int32_t cap, int32_t* grid, dl_stream_t stream);
/* link probe: dst[i*bytes_each ...] <- srcs[i][0 .. bytes_each) for i < nsrc (<= 8), all
 * sources streamed at once by one kernel (measures per-link and aggregate peer read rates) */
DL_API int dl_peer_gather(const uint64_t* srcs, int32_t nsrc, int64_t bytes_each, void* dst,
                          dl_stream_t stream);
DL_API int dl_xgmi_reduce_sgd(const uint64_t* wires, const uint64_t* thetas, int32_t n,
                              int32_t rank, int64_t lo, int64_t len, float* mom, float lr,
                              float momentum, int32_t nesterov, int32_t first_step,
                              dl_stream_t stream);

/* dl_xgmi_reduce_sgd without a wire: inners[q] is rank q's INNER parameters laid out in the
 * packed layout (OuterSync(exchange="xgmi_inner") keeps them in one such arena), and the
 * kernel forms g = (Σ_q (thetas[rank][k] - inners[q][k]) in rank order) / n itself -- the
 * subtraction of src/utils.py:221 rank q would have made, θ_outer being identical on every
 * rank -- so no rank runs dl_delta_pack. Bit-identical to dl_delta_pack + dl_xgmi_reduce_sgd;
 * same ordering rules (between two barriers, dl_sys_fence around each). */
DL_API int dl_xgmi_delta_sgd(const uint64_t* inners, const uint64_t* thetas, int32_t n,
                             int32_t rank, int64_t lo, int64_t len, float* mom, float lr,
                             float momentum, int32_t nesterov, int32_t first_step,
                             dl_stream_t stream);

/* ---- calibration ------------------------------------------------------------------------
 * dst[0:bytes) = src[0:bytes) with the segment walker's access shape (one 256-lane
 * workgroup per 16 KiB, 4 float4 loads per lane before the stores); flags: DL_TUNE_NT_LOADS =
 * non-temporal loads and stores, DL_COPY_WIDE = 8 float4 loads per lane (32 KiB per
 * workgroup). bench.py times every variant in the same run as the outer step and reads its
 * roofline fractions against the fastest: the copy ceiling (not on the reference's path).
 * Probes: DL_COPY_READ only reads src[0:bytes) (dst is not written, may be NULL);
 * DL_COPY_WRITE only writes dst[0:bytes), each 32-bit word its own index (src unused, may be
 * NULL). DL_COPY_STREAMS(s), s = 1..4, splits the buffer into s equal streams (bytes a
 * multiple of 16 s) and has each workgroup touch one 16 KiB tile of every stream, as a walker
 * kernel with s input (output) buffers does. bench.py combines the rates into the same-run
 * ceiling of a kernel's byte mix: t >= R / BW_read(s_r) + W / BW_write(s_w) (tools/rw_mix.hip). */
#define DL_COPY_WIDE 8
#define DL_COPY_READ 16
#define DL_COPY_WRITE 32
#define DL_COPY_STREAMS(s) ((((s) - 1) & 3) << 8)
DL_API int dl_copy(const void* src, void* dst, int64_t bytes, int32_t flags, dl_stream_t stream);

DL_API const char* dl_last_error(void);
DL_API int dl_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DILOCO_HIP_H */
