/* picotron_hip.h -- C ABI of the picotron_amd gfx950 (MI355X) kernels.
 *
 * Every entry point takes plain device pointers, element counts / strides (in ELEMENTS, not
 * bytes) and a hipStream_t, launches asynchronously on that stream, never allocates, and returns
 * 0 on success, a negative PT_E* code for an argument error detected before launch, or a
 * positive hipError_t from the launch.  bf16 tensors are passed as raw 16-bit storage.
 *
 * Each function names the reference interface it replaces (paths relative to the reference
 * checkout, okoge-kaz/picotron @ 2025-03-02).  The Python host layer (picotron_amd/_C.py) binds
 * these with ctypes; INTEGRATION.md shows the binding a picotron maintainer would add.
 */
#ifndef PICOTRON_HIP_H
#define PICOTRON_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define PT_OK 0
#define PT_EINVAL (-1)
#define PT_EALIGN (-2)
#define PT_EUNSUPPORTED (-3)

/* Device status word (int32, caller-owned, zeroed by the caller): kernels that validate DATA (not
 * shapes) set a bit here instead of trapping -- the analogue of torch's device-side assert.  The
 * host reads it when it synchronises anyway (picotron_amd.kernels.device_status). */
#define PT_STATUS_BAD_TARGET 1
#define PT_STATUS_NONFINITE_GRAD 2   /* the global gradient norm is inf / NaN: the step was skipped */

/* ---- RMSNorm ------------------------------------------------------------------------------
 * replaces picotron/model.py:51-65 (TritonRMSNorm -> flash-attn layer_norm_fn, mode 0) and
 * picotron/model.py:81-86 (LlamaRMSNorm, mode 1); `residual` fuses the bf16 residual add of
 * picotron/model.py:207-208 (z_out = bf16(x + residual) is normalised and written out).
 * x, residual, y, z_out: [rows, cols] bf16; weight [cols] bf16; rstd [rows] f32 (saved for bwd). */
int pt_rmsnorm_fwd(const void* x, const void* residual, const void* weight, void* y, void* z_out, float* rstd,
                   int64_t rows, int64_t cols, float eps, int mode, hipStream_t stream);
/* number of f32 rows of `cols` the bwd needs in dw_partial */
int pt_rmsnorm_bwd_partials(int64_t rows, int cols);
/* autograd backward of the above: dx = d/dz (+ dres), dweight [cols] (may be NULL).
 * mode = norm mode (0 / 1) | dweight sink: 0 store bf16; PT_DW_ACC_BF16 dweight = bf16(dweight +
 * bf16(dw)) (autograd's accumulation into a bf16 .grad); PT_DW_ACC_F32 dweight is f32, += dw
 * (DataParallelBucket main_grad).  The weight sum is in a fixed order (deterministic). */
#define PT_DW_ACC_BF16 4
#define PT_DW_ACC_F32 8
int pt_rmsnorm_bwd(const void* dy, const void* z, const void* weight, const float* rstd, const void* dres,
                   void* dx, void* dweight, float* dw_partial, int64_t rows, int64_t cols, int mode,
                   hipStream_t stream);
/* pt_rmsnorm_bwd with dy given as the two f32 K halves of a split-K dX GEMM (pt_gemm_dual / pt_gemm
 * with EPI_F32 partials: contiguous [rows, cols]): dy = bf16(dy_p0 + dy_p1) is formed in the kernel,
 * bit-identical to pt_gemm_splitk_sum followed by pt_rmsnorm_bwd without writing and re-reading dy.
 * (The post_attention_layernorm backward behind the gate|up dX, model.py:206-208.) */
int pt_rmsnorm_bwd_splitk(const float* dy_p0, const float* dy_p1, const void* z, const void* weight,
                          const float* rstd, const void* dres, void* dx, void* dweight, float* dw_partial,
                          int64_t rows, int64_t cols, int mode, hipStream_t stream);
/* the dweight column sums of n <= 32 pt_rmsnorm_bwd calls made with dweight = NULL (their
 * dw_partial buffers, pt_rmsnorm_bwd_partials rows each), one launch; sinks[i] as the dweight sink
 * bits of pt_rmsnorm_bwd's mode.  Bit-identical to passing dweight to each call.  (An
 * implementation detail of the same LlamaRMSNorm backward: a micro-batch's norms sum their weight
 * gradients together at the end of its backward.) */
int pt_rmsnorm_colsum_batch(const float* const* partials, const int* nparts, void* const* dweights,
                            const int* sinks, int n, int64_t cols, hipStream_t stream);

/* ---- RoPE (rotate-half, non-interleaved) --------------------------------------------------
 * replaces picotron/model.py:136-137 (flash-attn apply_rotary_emb) and model.py:12-19
 * (apply_rotary_pos_emb).  In place on the first `nheads` heads of every row of x
 * ([rows, row_stride] bf16); row r has position r % seq_len in the [seq_len, table_stride]
 * cos/sin tables of get_cos_sin (model.py:21-31).  inverse = 1 rotates by -theta (backward). */
int pt_rope(void* x, int64_t rows, int64_t row_stride, int64_t nheads, int64_t head_dim, const void* cos_table,
            const void* sin_table, int64_t seq_len, int64_t table_stride, int inverse, hipStream_t stream);

/* ---- per-head QK-norm fused with RoPE ---------------------------------------------------------
 * Not in the reference: the q_norm / k_norm of Qwen3 / OLMo-2 / Gemma-3 / Chameleon between the
 * q|k|v projection (model.py:124-126) and the rotation (model.py:136-137).  An RMSNorm over the
 * head_dim values of every q head (weight wq [head_dim] bf16) and every k head (wk), in
 * pt_rmsnorm_fwd's two modes, the bf16 result then rotated as pt_rope rotates it (position =
 * row % seq_len; cos_table = sin_table = NULL: norm only) -- bit-identical to the norm-only call
 * followed by pt_rope.  x, y: [rows, stride] bf16 whose first nheads_q + nheads_k heads are q|k;
 * later columns (v) are neither read nor written; y may be x.  rstd [rows, nheads_q + nheads_k] f32.
 * Checked in this order, before any launch: head_dim not 64 / 128 PT_EUNSUPPORTED; a NULL required
 * pointer, a count <= 0, mode not 0 / 1, exactly one of cos / sin NULL PT_EINVAL; rows, a row's
 * width, a stride or a table size past 32 bits PT_EUNSUPPORTED; a stride below the q|k width
 * PT_EINVAL; a stride not a multiple of 8 or a pointer not 16-byte aligned PT_EALIGN. */
int pt_qk_norm_rope_fwd(const void* x, int64_t x_stride, void* y, int64_t y_stride, const void* wq, const void* wk,
                        float* rstd, int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim, float eps,
                        int mode, const void* cos_table, const void* sin_table, int64_t seq_len, int64_t table_stride,
                        hipStream_t stream);
/* number of f32 rows of head_dim the backward writes into each partial buffer (negative: refused) */
int pt_qk_norm_bwd_partials(int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim);
/* Backward of the norm, from the saved pre-norm x and rstd, on dy = the gradient with respect to
 * the normed (un-rotated) y: dx = bf16(rstd * (dy w - xh mean_d(dy w xh))), xh = x rstd; dx may be
 * dy.  dwq_partial / dwk_partial [pt_qk_norm_bwd_partials, head_dim] f32: every row is written (one
 * per workgroup, summed in a fixed order: deterministic); pt_rmsnorm_colsum_batch(cols = head_dim)
 * finishes the weight gradient into its sink.  NULL: that weight's gradient is not formed. */
int pt_qk_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* wq, const void* wk,
                   const float* rstd, void* dx, int64_t dx_stride, float* dwq_partial, float* dwk_partial,
                   int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim, int mode, hipStream_t stream);

/* ---- SwiGLU: h = silu(g) * u --------------------------------------------------------------
 * replaces picotron/model.py:186 F.silu(gate_proj(x)) * up_proj(x) (fwd and autograd bwd). */
int pt_swiglu_fwd(const void* g, int64_t g_stride, const void* u, int64_t u_stride, void* h, int64_t h_stride,
                  int64_t rows, int64_t cols, hipStream_t stream);
int pt_swiglu_bwd(const void* dh, int64_t dh_stride, const void* g, int64_t g_stride, const void* u,
                  int64_t u_stride, void* dg, int64_t dg_stride, void* du, int64_t du_stride, int64_t rows,
                  int64_t cols, hipStream_t stream);

/* ---- mixture-of-experts routing ---------------------------------------------------------------
 * Not in the reference (its MLP is dense, model.py:184-186): the routing of an MoE MLP (Mixtral,
 * Qwen3-MoE, OLMoE) with a GShard / Switch capacity.  T tokens choose k of E experts; expert e owns
 * rows [e C, (e + 1) C) of the [R = E C, H] expert buffers.  Item i = t k + j is token t's j-th
 * choice (best first).  Every shape is static, nothing is read on the host, there are no atomics,
 * and two runs give the same bits.  E <= 128, k <= min(E, 8), H % 64 == 0, any T >= 1 (beyond that
 * PT_EUNSUPPORTED).  Checked before any launch, in this order: a NULL required pointer or a size
 * < 1 PT_EINVAL; the limits above, or a count past 32 bits, PT_EUNSUPPORTED; a leading dimension
 * below its row PT_EINVAL (logits) / a pointer off 16 bytes, a row stride off 8 elements or below H
 * PT_EALIGN (the [*, H] rows).
 *
 * pt_moe_route: logits bf16 [T, ldl], the first E columns valid.  probs f32 [T, E] = the softmax of
 * the stored values over all E; idx int32 [T, k] = the k largest STORED values, ties to the lower
 * expert, best first; gate f32 [T, k] = probs[idx], divided by their sum when norm_topk;
 * counts int32 [E] = the selections per expert (before any capacity); aux f32 [1] =
 * E sum_e (counts[e] / (T k)) (mean_t probs[t, e]), the Switch load-balancing loss.  workspace:
 * pt_moe_route_workspace(T, E) 4-byte words (negative: refused). */
int pt_moe_route_workspace(int64_t T, int64_t E);
int pt_moe_route(const void* logits, int64_t ldl, int64_t T, int64_t E, int64_t k, int norm_topk, int32_t* idx,
                 float* gate, float* probs, int32_t* counts, float* aux, void* workspace, hipStream_t stream);
/* pt_moe_plan: pos(i) = the number of items before i (flat order) with the same expert;
 * slot int32 [T, k] = idx C + pos where pos < C, else -1 (dropped); src int32 [E C] = the item in
 * that row, -1 for an empty row.  An idx outside [0, E) is dropped and not counted.  A prefix count
 * over workgroups of pt_moe_plan_block() items, whose result does not depend on their scheduling.
 * workspace: pt_moe_plan_workspace(T, E, k) int32 words. */
int pt_moe_plan_block(void);
int pt_moe_plan_workspace(int64_t T, int64_t E, int64_t k);
int pt_moe_plan(const int32_t* idx, int64_t T, int64_t E, int64_t k, int64_t C, int32_t* slot, int32_t* src,
                int32_t* workspace, hipStream_t stream);
/* pt_moe_dispatch: xe[r, :] = x[src[r] / k, :] (a bit copy), zeros where src[r] is outside [0, T k). */
int pt_moe_dispatch(const void* x, int64_t ldx, const int32_t* src, void* xe, int64_t ldxe, int64_t T, int64_t k,
                    int64_t R, int64_t H, hipStream_t stream);
/* pt_moe_combine: y[t, :] = bf16(residual[t, :] + sum_j gate[t, j] ye[slot[t, j], :]) over the items
 * with slot in [0, R), accumulated in f32 in j order and rounded once.  gate NULL: weights of 1 (the
 * backward of pt_moe_dispatch: dx[t] = sum_j dxe[slot[t, j]]); residual NULL: none. */
int pt_moe_combine(const void* ye, int64_t ldye, const int32_t* slot, const float* gate, const void* residual,
                   int64_t ldr, void* y, int64_t ldy, int64_t T, int64_t k, int64_t R, int64_t H, hipStream_t stream);
/* pt_moe_combine_bwd: dye[r, :] = bf16(gate[src[r]] dy[src[r] / k, :]), zeros for empty rows;
 * dgate[i] = sum_h dy[t, h] ye[slot[i], h] in f32, 0 for dropped items. */
int pt_moe_combine_bwd(const void* dy, int64_t lddy, const void* ye, int64_t ldye, const int32_t* slot,
                       const int32_t* src, const float* gate, void* dye, int64_t lddye, float* dgate, int64_t T,
                       int64_t k, int64_t R, int64_t H, hipStream_t stream);
/* pt_moe_route_bwd: dlogits bf16 [T, ldl] (columns E.. zero) from dgate [T, k] and the device scalar
 * d_aux (NULL: 0), through the selection (idx fixed), the renormalisation (norm_topk) and the softmax:
 * dp[t, idx_j] = (dgate_j - sum_i dgate_i gate_i) / sum_i p[idx_i] (or dgate_j), dp[t, e] +=
 * d_aux E counts[e] / (T k) / T (counts carry no gradient), dlogit = p (dp - sum_e p dp). */
int pt_moe_route_bwd(const float* dgate, const float* probs, const int32_t* idx, const int32_t* counts,
                     const float* d_aux, int norm_topk, void* dlogits, int64_t ldl, int64_t T, int64_t E, int64_t k,
                     hipStream_t stream);

/* ---- residual add: out = bf16(x + r), n contiguous bf16 (n % 8 == 0, 16-B aligned) ------------
 * replaces picotron/model.py:208 `x + self.mlp(...)` where the sequence-parallel TP layer adds the
 * residual to its reduce-scattered MLP output (no GEMM epilogue can carry it there). */
int pt_residual_add(const void* x, const void* r, void* out, int64_t n, hipStream_t stream);

/* ---- fused cross-entropy forward + backward -----------------------------------------------
 * replaces train.py:49 F.cross_entropy(logits, targets, 'mean') / grad_acc (+ autograd bwd) and
 * pipeline_parallel.py:103,153.  row_loss[r] = lse - logit[target]; dlogits (may alias logits) =
 * (softmax - onehot) * scale * (*inv_count if non-NULL).  targets int64, ignore_index rows -> 0;
 * a target outside [0, vocab) (not ignore_index) gives a NaN row and sets PT_STATUS_BAD_TARGET in
 * *status (may be NULL).  dlogits == NULL: loss only (one read of the logits). */
int pt_cross_entropy_fwd_bwd(const void* logits, int64_t logits_stride, const int64_t* targets, void* dlogits,
                             int64_t dlogits_stride, float* row_loss, int64_t rows, int64_t vocab, float scale,
                             const float* inv_count, int64_t ignore_index, int* status, hipStream_t stream);
/* The autograd pair (train.py:49 forward, loss.backward() at train.py:51): the forward streams the
 * logits once with an online max / sum-exp and writes row_loss and row_lse [rows] f32; the
 * backward is elementwise from the saved LSE: dlogits = (exp(x - row_lse) - onehot) *
 * scale[row * scale_stride] (scale_stride 0: one device scalar, grad_output / #valid for 'mean',
 * grad_output for 'sum'; 1: a per-row f32 gradient, reduction='none'), ignore_index rows -> 0.
 * dlogits may alias logits. */
int pt_cross_entropy_fwd_lse(const void* logits, int64_t logits_stride, const int64_t* targets, float* row_loss,
                             float* row_lse, int64_t rows, int64_t vocab, int64_t ignore_index, int* status,
                             hipStream_t stream);
int pt_cross_entropy_bwd_lse(const void* logits, int64_t logits_stride, const int64_t* targets, const float* row_lse,
                             void* dlogits, int64_t dlogits_stride, int64_t rows, int64_t vocab, const float* scale,
                             int64_t scale_stride, int64_t ignore_index, hipStream_t stream);
/* The same forward from the lm_head GEMM's statistics (pt_gemm_ce_stats) instead of a second pass
 * over the logits: float2 stats[b * rows + row] = (max, sum exp(x - max)) of the row's bf16 logits
 * in column tile b < nblk (vocab / nblk columns each); only x[row, target] is read. */
int pt_cross_entropy_fwd_stats(const void* logits, int64_t logits_stride, const int64_t* targets,
                               const float* stats, int64_t nblk, float* row_loss, float* row_lse, int64_t rows,
                               int64_t vocab, int64_t ignore_index, int* status, hipStream_t stream);

/* Vocab-parallel form (the lm_head as ColumnParallelLinear(gather_output=True), tensor_parallel.py:
 * 50 + tp_communications.py:51-72, whose logits all-gather it replaces): each tp rank reduces its
 * shard logits [rows, vocab_shard] (global columns vocab_lo ..) with the GEMM statistics to a float4
 * part[row] = (max, sum exp(x - max), x[target] if target in the shard else 0, 1 / 0); the caller
 * all-gathers the parts [tp][rows][4] and combines them (rank order) into row_loss / row_lse as
 * pt_cross_entropy_fwd_stats returns them for the whole vocabulary (same range check against
 * `vocab`).  The backward on the shard: pt_cross_entropy_bwd_lse with the one-hot at target - vocab_lo. */
int pt_cross_entropy_vp_partial(const void* logits, int64_t logits_stride, const int64_t* targets,
                                const float* stats, int64_t nblk, float* part, int64_t rows, int64_t vocab_shard,
                                int64_t vocab_lo, hipStream_t stream);
int pt_cross_entropy_vp_combine(const float* parts, int64_t tp, const int64_t* targets, float* row_loss,
                                float* row_lse, int64_t rows, int64_t vocab, int64_t ignore_index, int* status,
                                hipStream_t stream);
int pt_cross_entropy_bwd_lse_shard(const void* logits, int64_t logits_stride, const int64_t* targets,
                                   const float* row_lse, void* dlogits, int64_t dlogits_stride, int64_t rows,
                                   int64_t vocab_shard, int64_t vocab_lo, const float* scale, int64_t scale_stride,
                                   int64_t ignore_index, hipStream_t stream);

/* ---- auxiliary z-loss (PaLM / OLMo-2 / Chameleon): z_coef * lse^2 per valid row ----------------
 * Each _z function is its namesake with the z term, formed from the row LSE the forward already
 * holds (no further pass over the logits):
 *   row_z[r] = z_coef * lse^2 (optional output [rows] f32, NULL: not written; 0 on ignore_index
 *   rows, NaN for a bad target);  row_loss[r] = (lse - logit[target]) + row_z[r];
 *   dlogits = (exp(x - lse) * (1 + 2 z_coef lse) - onehot) * scale[...]  (ignored rows: +0).
 * z_coef is a finite f32 >= 0 (else PT_EINVAL before any launch); z_coef == 0 writes the bits of
 * the plain function and row_z = 0.  pt_cross_entropy_mean over row_z gives the reported z part. */
/* pt_cross_entropy_fwd_bwd with the z term in row_loss, row_z and dlogits (both kernels). */
int pt_cross_entropy_fwd_bwd_z(const void* logits, int64_t logits_stride, const int64_t* targets, void* dlogits,
                               int64_t dlogits_stride, float* row_loss, int64_t rows, int64_t vocab, float scale,
                               const float* inv_count, int64_t ignore_index, int* status, float z_coef, float* row_z,
                               hipStream_t stream);
/* pt_cross_entropy_fwd_lse with the z term; row_lse is the plain LSE, saved for the backward. */
int pt_cross_entropy_fwd_lse_z(const void* logits, int64_t logits_stride, const int64_t* targets, float* row_loss,
                               float* row_lse, int64_t rows, int64_t vocab, int64_t ignore_index, int* status,
                               float z_coef, float* row_z, hipStream_t stream);
/* pt_cross_entropy_bwd_lse with the factor 1 + 2 z_coef row_lse on the softmax. */
int pt_cross_entropy_bwd_lse_z(const void* logits, int64_t logits_stride, const int64_t* targets,
                               const float* row_lse, void* dlogits, int64_t dlogits_stride, int64_t rows,
                               int64_t vocab, const float* scale, int64_t scale_stride, int64_t ignore_index,
                               float z_coef, hipStream_t stream);
/* pt_cross_entropy_fwd_stats with the z term (the GEMM statistics are unchanged). */
int pt_cross_entropy_fwd_stats_z(const void* logits, int64_t logits_stride, const int64_t* targets,
                                 const float* stats, int64_t nblk, float* row_loss, float* row_lse, int64_t rows,
                                 int64_t vocab, int64_t ignore_index, int* status, float z_coef, float* row_z,
                                 hipStream_t stream);
/* pt_cross_entropy_vp_combine with the z term from the combined LSE (the 16-byte parts of
 * pt_cross_entropy_vp_partial are unchanged). */
int pt_cross_entropy_vp_combine_z(const float* parts, int64_t tp, const int64_t* targets, float* row_loss,
                                  float* row_lse, int64_t rows, int64_t vocab, int64_t ignore_index, int* status,
                                  float z_coef, float* row_z, hipStream_t stream);
/* pt_cross_entropy_bwd_lse_shard with the factor 1 + 2 z_coef row_lse on the shard's softmax. */
int pt_cross_entropy_bwd_lse_shard_z(const void* logits, int64_t logits_stride, const int64_t* targets,
                                     const float* row_lse, void* dlogits, int64_t dlogits_stride, int64_t rows,
                                     int64_t vocab_shard, int64_t vocab_lo, const float* scale, int64_t scale_stride,
                                     int64_t ignore_index, float z_coef, hipStream_t stream);

/* train.py:49's reduction='mean' over the per-row losses: loss = sum(row_loss) / #(target !=
 * ignore_index) in one deterministic launch; inv_count = 1 / #valid (the backward's scale);
 * reduce_sum != 0: reduction='sum' (loss = sum(row_loss), inv_count = 1);
 * loss_f32 / out (bf16 when out_bf16, else f32) optional. */
int pt_cross_entropy_mean(const float* row_loss, const int64_t* targets, int64_t rows, int64_t ignore_index,
                          float* loss_f32, float* inv_count, void* out, int out_bf16, int reduce_sum,
                          hipStream_t stream);

/* ---- token embedding ----------------------------------------------------------------------
 * replaces model.py:224-225 (F.embedding + autograd's dense backward) and the masked lookup of
 * VocabParallelEmbedding (tensor_parallel.py:246-270): rows of ids outside [vocab_lo, vocab_hi)
 * are zero.  ids int64 [T]; weight [vocab_hi - vocab_lo, H] bf16 (leading dim ldw).
 * bwd: ids sorted ascending with their token positions perm (stable; -1 = token to skip);
 * dweight[id - vocab_lo] (sink: 0 store bf16, PT_DW_ACC_BF16, PT_DW_ACC_F32) gets the f32 sum of
 * the dY rows of each id rounded to bf16 once; untouched rows are not accessed. */
int pt_embedding_fwd(const int64_t* ids, int64_t T, const void* weight, int64_t ldw, int64_t vocab_lo, int64_t vocab_hi,
                     void* out, int64_t ldo, int64_t H, hipStream_t stream);
int pt_embedding_bwd(const int64_t* sorted_ids, const int64_t* perm, int64_t T, const void* dy, int64_t ldy,
                     int64_t vocab_lo, void* dweight, int64_t lddw, int64_t H, int sink, hipStream_t stream);
/* The backward's segment order: ids keyed (0 = skipped: outside [vocab_lo, vocab_hi) or padding_idx
 * when has_padding; else id - vocab_lo + 1) and stably sorted in one launch -> sorted_ids (-1 =
 * skip) and perm (token positions), the inputs of pt_embedding_bwd.  T <= 16384 (else
 * PT_EUNSUPPORTED). */
int pt_embedding_sort(const int64_t* ids, int64_t T, int64_t vocab_lo, int64_t vocab_hi, int has_padding,
                      int64_t padding_idx, int64_t* sorted_ids, int64_t* perm, hipStream_t stream);

/* ---- fused AdamW step ---------------------------------------------------------------------
 * replaces train.py:209 torch.optim.AdamW(...).step() for one tensor: the eight foreach passes of
 * torch's multi-tensor Adam (decoupled weight decay) in one, same per-op rounding to the storage
 * dtype (dtype 0 bf16, 1 f32).  Scalars as torch casts them: decay = 1 - lr*wd, w1 = 1 - beta1,
 * c2 = 1 - beta2, bc2_sqrt = sqrt(1 - beta2^t), step_size = -lr / (1 - beta1^t).
 * Like every entry of this family it checks all of its arguments before it looks at whether there
 * is anything to do: a dtype outside {0, 1} is PT_EINVAL at n == 0 too (it used to be PT_OK here,
 * and only here). */
int pt_adamw_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int dtype,
                  float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                  hipStream_t stream);
/* The same update over a LIST of bf16 tensors in one launch (torch's foreach AdamW is a list op
 * too): `tensors` is a device array of pt_adam_tensor (every pointer 16-byte aligned),
 * `chunk_start` a device int64 [ntensors + 1] of prefix sums of ceil(n / 8), total_chunks its last
 * entry.  The caller builds and caches both (the pointers only change when tensors are re-made). */
typedef struct {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  int64_t n;
} pt_adam_tensor;
int pt_adamw_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                        hipStream_t stream);

/* ---- global gradient-norm clipping, fused into the AdamW step ------------------------------
 * replaces torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) in front of the optimizer
 * step (what a Llama training recipe adds in front of train.py:235): the L2 norm over every gradient
 * in f32, and the scaling by clip_coef = min(1, max_norm / (total_norm + 1e-6)) applied where the
 * AdamW kernel loads the gradient -- the clipped gradients are never written, the coefficient
 * never leaves the device.
 *
 * Sum of squares: sq[0] = (accumulate ? sq[0] : 0) + weight * sum g^2, over the grad field of the
 * pt_adam_tensor list pt_adamw_step_multi takes (same table, same chunk_start), or over one tensor
 * (dtype 0 bf16 at any alignment, 1 f32).  Two launches: one f32 partial per workgroup into
 * `workspace` (pt_grad_sq_workspace() floats, caller-owned, reusable by the next call on the
 * stream), then one workgroup sums them in a fixed order -- no float atomics, bit-reproducible.
 * Several lists and tensors accumulate into one scalar in stream order; `weight` scales a list's
 * share (1 / tp for gradients replicated over a tensor-parallel group, so an all-reduce of sq over
 * the group counts them once). */
int pt_grad_sq_workspace(void);
int pt_grad_sq_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                     float weight, int accumulate, float* workspace, float* sq, hipStream_t stream);
int pt_grad_sq(const void* grad, int64_t n, int dtype, float weight, int accumulate, float* workspace, float* sq,
               hipStream_t stream);
/* Every consumer below reads grad_sq[0] on the device and computes the same clip_coef (IEEE sqrt and
 * division).  If grad_sq[0] is inf or NaN it does NOTHING and sets PT_STATUS_NONFINITE_GRAD in
 * *status (may be NULL) -- torch would write NaN into every weight.  max_norm > 0.
 * In-place scale, grad = r(grad * clip_coef) (the stand-alone clip_grad_norm_; torch's
 * _foreach_mul_); clip_coef == 1 stores nothing. */
int pt_grad_scale_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        const float* grad_sq, float max_norm, int* status, hipStream_t stream);
int pt_grad_scale(void* grad, int64_t n, int dtype, const float* grad_sq, float max_norm, int* status,
                  hipStream_t stream);
/* pt_adamw_step / pt_adamw_step_multi on g' = r(grad * clip_coef): bit-identical to the in-place
 * scale followed by the unclipped step, without the gradients' second read and their rewrite (the
 * gradients are not modified). */
int pt_adamw_step_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int dtype,
                       float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                       const float* grad_sq, float max_norm, int* status, hipStream_t stream);
int pt_adamw_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                             float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                             float step_size, const float* grad_sq, float max_norm, int* status,
                             hipStream_t stream);

/* ---- AdamW with fp32 master weights and moments ---------------------------------------------
 * The mixed-precision recipe on top of train.py:209: an f32 master copy of every bf16 weight and
 * both moments in f32.  Per element, in f32, each operation rounded on its own: g32 = float(grad)
 * (grad_dtype 0 bf16, 1 f32; with clipping g32 *= clip_coef, never rounded to bf16), torch's foreach
 * f32 AdamW sequence on (master, g32, exp_avg, exp_avg_sq), then param = bf16(master), round to
 * nearest even.  28 B per parameter with bf16 gradients, 30 B with f32 gradients.
 * List form: `tensors` is a device array of pt_adam_master_tensor (every pointer 16-byte aligned,
 * all gradients of the launch of one dtype), chunk_start / total_chunks as for pt_adamw_step_multi.
 * Single-tensor form: any alignment.  The *_clip forms and pt_grad_sq_master_multi (the sum of
 * squares over the grad field of the list) behave as their pt_adam_tensor namesakes above. */
typedef struct {
  float* master;
  void* param;      /* bf16, written only */
  const void* grad; /* bf16 or f32 */
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
} pt_adam_master_tensor;
int pt_adamw_master_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                               int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                               float step_size, hipStream_t stream);
int pt_adamw_master_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors,
                                    int64_t total_chunks, int grad_dtype, float decay, float w1, float beta2, float c2,
                                    float bc2_sqrt, float eps, float step_size, const float* grad_sq, float max_norm,
                                    int* status, hipStream_t stream);
int pt_adamw_master_step(float* master, void* param, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                         float step_size, hipStream_t stream);
int pt_adamw_master_step_clip(float* master, void* param, const void* grad, float* exp_avg, float* exp_avg_sq,
                              int64_t n, int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt,
                              float eps, float step_size, const float* grad_sq, float max_norm, int* status,
                              hipStream_t stream);
int pt_grad_sq_master_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                            int grad_dtype, float weight, int accumulate, float* workspace, float* sq,
                            hipStream_t stream);

/* ---- AdamW in bf16 state with stochastic rounding -------------------------------------------
 * The recipe between the two above: param, exp_avg and exp_avg_sq stay bf16 (the plain step's 6 B
 * of state and 14 B of traffic per parameter, 16 B with f32 gradients), the update is the master
 * step's f32 sequence on the widened values -- g32 = float(grad) (grad_dtype 0 bf16, 1 f32; with
 * clipping g32 *= clip_coef, never rounded to bf16) -- and the three results are stored with
 * sr_bf16: rounded up or down with probability equal to the discarded fraction, so E[stored] is
 * the f32 value.  No other rounding to bf16 happens in the step.
 *
 * Random bits: Philox4x32-10 (Random123's constants), key = (seed_lo, seed_hi), counter =
 * (c & 0xffffffff, c >> 32, step, (rng_stream << 2) | which): c = i >> 3, the 8-element chunk of
 * element i inside its tensor; step the parameter's step count t >= 1; rng_stream < 2^30 the
 * parameter's fixed stream id; which = 0 param, 1 exp_avg, 2 exp_avg_sq.  Of the four words w the
 * element takes r = (w[(i & 7) >> 1] >> (16 * (i & 1))) & 0xffff.  The bits are a pure function of
 * (seed, stream, step, element index, which): launch geometry, list order, neighbours, alignment
 * and list or single-tensor form do not enter, and every form gives the same result bit for bit.
 * sr_bf16(x, r) for x with bits u: inf and NaN take the plain cast; otherwise the 16-bit value
 * (u + r) >> 16.  A bf16 value never changes; the magnitude goes up with probability
 * low16 / 65536 exactly; -0 stays -0; a value inside the last bf16 ulp below the largest finite
 * one may become inf.
 *
 * List form: `tensors` is a device array of pt_adam_sr_tensor (every pointer 16-byte aligned),
 * chunk_start / total_chunks as for pt_adamw_step_multi.  The table's builder keeps rng_stream in
 * [0, 2^30).  Single-tensor form: any alignment.  step == 0, rng_stream outside [0, 2^30), a
 * grad_dtype outside {0, 1} or `which` outside {0, 1, 2} is PT_EINVAL.  The *_clip forms and
 * pt_grad_sq_sr_multi behave as their namesakes above.  pt_sr_cast_bf16 is the rounding alone:
 * y[i] = sr_bf16(x[i], the draw of element i). */
typedef struct {
  void* param;
  const void* grad; /* bf16 or f32 */
  void* exp_avg;
  void* exp_avg_sq;
  int64_t n;
  int64_t rng_stream;
} pt_adam_sr_tensor;
int pt_adamw_sr_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                           int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                           float step_size, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, hipStream_t stream);
int pt_adamw_sr_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                                int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                                float step_size, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, const float* grad_sq,
                                float max_norm, int* status, hipStream_t stream);
int pt_adamw_sr_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int grad_dtype,
                     float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                     uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int64_t rng_stream, hipStream_t stream);
int pt_adamw_sr_step_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int grad_dtype,
                          float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                          uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int64_t rng_stream, const float* grad_sq,
                          float max_norm, int* status, hipStream_t stream);
int pt_grad_sq_sr_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        int grad_dtype, float weight, int accumulate, float* workspace, float* sq, hipStream_t stream);
int pt_sr_cast_bf16(const float* x, void* y, int64_t n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                    int64_t rng_stream, int which, hipStream_t stream);

/* ---- Muon: everything of the step that is not a GEMM ----------------------------------------
 * replaces torch.optim.Muon (torch/optim/_muon.py) for 2-D bf16 parameters; the products of the
 * Newton-Schulz iteration run on pt_gemm_grouped (kernels.muon_newton_schulz).
 *
 * List entries: `tensors` is a device array of pt_muon_tensor, `block_start` a device int64
 * [ntensors + 1] of prefix sums of ceil(ceil(n / 8) / pt_muon_block_chunks()), total_blocks its
 * last entry.  A tensor is a [R, C] view with unit column stride and a row stride (ld*); 16-byte
 * vector accesses where bases are 16-byte aligned and C and the row strides are multiples of 8,
 * element by element otherwise -- the same bits.  A tensor's blocks are counted from its own first
 * element, so nothing a kernel computes for it depends on its place in the list.
 * grad_dtype 0 bf16 / 1 f32: the gradients and the momentum buffers of one launch. */
typedef struct {
  void* param;            /* bf16 [R, C], row stride ldp */
  const void* grad;       /* row stride ldg */
  void* momentum_buffer;  /* the gradient's dtype, row stride ldb */
  void* x;                /* bf16 workspace image, row stride ldx: X0 out (scale), O in (apply) */
  int64_t n, cols;        /* R * C, C */
  int64_t ldp, ldg, ldb, ldx;
  float lr_ratio;         /* _adjust_lr's ratio for the shape: lr_adj = lr * lr_ratio */
  int32_t sq_slot;        /* the tensor's entry of `sq` */
} pt_muon_tensor;
int pt_muon_block_chunks(void);
/* _muon.py:310-311 `buf.lerp_(grad, 1 - momentum); update = grad.lerp(buf, momentum) if nesterov
 * else buf`, each result rounded once to its storage dtype (update to bf16; it is not stored), and
 * the first half of :59 `ortho_grad.norm()`: sq[sq_slot] = sum update^2 in f32 over the bf16
 * values.  w_buf = f32(1 - momentum), w_nes = f32(momentum); torch's lerp, both branches.
 * `partial`: total_blocks floats, one per block, summed per tensor by one workgroup in a fixed
 * order -- no float atomics, bit-reproducible, nothing read on the host. */
int pt_muon_momentum(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                     int grad_dtype, float w_buf, float w_nes, int nesterov, float* partial, float* sq,
                     hipStream_t stream);
/* The same on g' = r(grad * clip_coef), clip_coef from the device scalar grad_sq exactly as
 * pt_adamw_step_multi_clip computes it (torch.nn.utils.clip_grad_norm_ in front of the step).  A
 * non-finite grad_sq: nothing is written (buffers, partials and sq alike) and PT_STATUS_NONFINITE_GRAD
 * is set in *status. */
int pt_muon_momentum_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                          int grad_dtype, float w_buf, float w_nes, int nesterov, float* partial, float* sq,
                          const float* grad_sq, float max_norm, int* status, hipStream_t stream);
/* _muon.py:55,59 `ortho_grad = grad.bfloat16(); ortho_grad.div_(ortho_grad.norm().clamp(min=eps))`:
 * x = bf16(update / max(sqrt(sq[sq_slot]), eps)) with update recomputed from (grad, momentum_buffer)
 * (torch rounds the norm itself to bf16; this does not).  The *_clip form recomputes the clipped
 * gradient, and writes nothing on a non-finite grad_sq (status is not posted again). */
int pt_muon_scale(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, int grad_dtype,
                  float w_nes, int nesterov, const float* sq, float eps, hipStream_t stream);
int pt_muon_scale_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                       int grad_dtype, float w_nes, int nesterov, const float* sq, float eps, const float* grad_sq,
                       float max_norm, int* status, hipStream_t stream);
/* _muon.py:63-66 `gram_update = addmm(gram, gram, gram, beta=b, alpha=c)` with the `beta=a` of the
 * following addmm folded in: P[i] = bf16(a I + b A[i] + c S[i]) for nmat (<= 4) matrices [m, m]
 * (dense, m a multiple of 8; A bf16, S f32), so a X + (b A + c A^2) X is one plain GEMM P X. */
int pt_muon_poly(const void* const* A, const float* const* S, void* const* P, int nmat, int64_t m, float a, float b,
                 float c, hipStream_t stream);
/* _muon.py:317-318 `param.mul_(1 - lr * weight_decay); param.add_(update, alpha=-adjusted_lr)`:
 * param = bf16(bf16(param * decay) - lr_adj * x), both roundings, decay = 1 - lr * weight_decay and
 * lr_adj = lr * lr_ratio in f32 (the table holds only the shape's ratio, so a scheduler's new lr
 * needs no new table).  The *_clip form does nothing on a non-finite grad_sq (the whole step is
 * skipped). */
int pt_muon_apply(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, float decay,
                  float lr, hipStream_t stream);
int pt_muon_apply_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                       float decay, float lr, const float* grad_sq, float max_norm, int* status, hipStream_t stream);

/* ---- bf16 GEMM, f32 accumulate -------------------------------------------------------------
 * replaces every F.linear / matmul of the layer: model.py:124-126,161,186,270,
 * tensor_parallel.py:186, tp_communications.py:79,93,98,105.
 * C[M,N] (op)= A[M,K] B[K,N].  a_kcontig: A stored [M,K] (else [K,M]); b_kcontig: B stored
 * [N,K] (weights; else [K,N]).  B may be split into nb pointer segments along N (b_seg_dim 0)
 * or K (1), C into nc segments along M; *_bounds hold n+1 boundaries (NULL = one segment).
 * N-segments and C segments have their own leading dimensions; K-segments share one ldb
 * (PT_EUNSUPPORTED otherwise: a tile's B image is stepped with one stride through all of K).
 * epilogue 0: C bf16 = acc, 1: C bf16 += acc, 2: C f32 = acc, 3: C f32 += acc,
 * 4: C bf16 = residual + acc (residual [M, N] bf16, leading dim ldr; the residual add of
 * model.py:207-208 fused into the producing projection).  tile -1 = auto. */
int pt_gemm(const void* A, int64_t lda, int a_kcontig, const void* const* B, const int64_t* ldb,
            const int64_t* b_bounds, int nb, int b_kcontig, int b_seg_dim, void* const* C, const int64_t* ldc,
            const int64_t* c_bounds, int nc, int64_t M, int64_t N, int64_t K, int epilogue,
            const void* residual, int64_t ldr, int tile, hipStream_t stream);
int pt_gemm_pick_tile(int64_t M, int64_t N, const int64_t* mseg, int nmseg, const int64_t* nseg, int nnseg);
/* The q|k|v projection with RoPE fused into its epilogue (model.py:124-126 + 136-137): columns
 * [0, rot_cols) of C = A . [B_0; ...]^T (B K-contiguous, segments along N) are rotated like
 * pt_rope (position = row % seq_len in the [seq, table_stride] bf16 cos/sin tables); head_dim 64. */
int pt_gemm_rope(const void* A, int64_t lda, const void* const* B, const int64_t* ldb, const int64_t* b_bounds, int nb,
                 void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, const void* cos_table, const void* sin_table,
                 int64_t table_stride, int64_t seq_len, int64_t rot_cols, int64_t head_dim, int tile,
                 hipStream_t stream);
/* The lm_head (model.py:270, logits consumed by F.cross_entropy at train.py:49) with the CE forward's
 * statistics fused into its epilogue: C[M, N] = A[M, K] . W[N, K]^T stored bf16, and per row and
 * `block`-column tile b the (max, sum exp(x - max)) of the stored values as float2
 * stats[b * M + row] (block 256 or 128; M % 256 == 0, N % block == 0, K % 64 == 0). */
int pt_gemm_ce_stats(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, float* stats,
                     int64_t block, int64_t M, int64_t N, int64_t K, hipStream_t stream);
/* Grouped GEMM: nprob (<= 4) independent problems in ONE launch, each described like pt_gemm's
 * arguments, sharing layouts (a_kcontig, b_kcontig), epilogue and tile (-1 = auto over the
 * group).  Used where one problem alone would leave CUs idle (dW of q|k|v + dW of o_proj).
 * ksplit > 1 (epilogue 2 only): the problem runs as ksplit K-slices of K / ksplit (a multiple of 64)
 * whose f32 partials land kpart_stride elements apart from C (slice s at C + s kpart_stride) -- for
 * the few-tile TP-shard GEMMs (24-128 tiles on 256 CUs); pt_gemm_splitk_reduce finishes them. */
typedef struct {
  const void* A;
  int64_t lda;
  const void* B[4];
  int64_t ldb[4];
  int64_t b_bounds[5];
  int nb;
  int b_seg_dim;
  void* C[4];
  int64_t ldc[4];
  int64_t c_bounds[5];
  int nc;
  int64_t M, N, K;
  const void* residual;
  int64_t ldr;
  int ksplit;              /* 0 / 1: not split */
  int64_t kpart_stride;    /* elements between two slices' f32 partials */
  /* A K-segmented: k >= a_k2 (a multiple of 64 inside K) reads A2 (same lda) -- a weight gradient
   * over two micro-batches' token rows (dY of both; B K-segmented the same way through b_seg_dim 1,
   * b_bounds {0, a_k2, K}): one K = 2 T launch instead of two accumulating ones (data_parallel.py:
   * 122-144's main_grad read-modify-written once per two micro-batches).  NULL: not segmented.  The
   * 256x256 8-phase tile only (pt_gemm_grouped tile 12 / auto, pt_gemm_dual). */
  const void* A2;
  int64_t a_k2;
} pt_gemm_problem;
int pt_gemm_grouped(const pt_gemm_problem* probs, int nprob, int a_kcontig, int b_kcontig, int epilogue, int tile,
                    hipStream_t stream);

/* Two independent groups in ONE launch of 256x256 tiles, each with its own layouts and epilogue:
 * group 0 = dX (A = dY [M, K] K-contiguous, B = W [K, N] N-contiguous; epilogue 0 or 6 = the
 * SwiGLU backward, residual = g|u), group 1 = wgrad (dY^T X; both operands MN-contiguous;
 * epilogue 0, 1 or 3; or 2 with ksplit problems: a split-K dW's f32 slices, pt_gemm_splitk_reduce).  The dX of a layer's projection beside its dW (both read only dY and saved
 * activations): the down_proj dX's HBM-bound SwiGLU-backward tail overlaps the dW's MFMA work.
 * Group 0's epilogue: 0 (bf16), 6 (SwiGLU backward) or 2 (f32: the two K halves of a split-K dX,
 * finished by pt_gemm_splitk_sum).
 * order: 0 group 0 first, 1 group 1 first, inside each XCD's share; 2 staggered (even XCDs group 0 first,
 * odd XCDs group 1 first).
 * PT_EUNSUPPORTED when a problem does not tile by 256 x 256 or a group's tile count % 8 != 0. */
int pt_gemm_dual(const pt_gemm_problem* p0, int n0, int a_kcontig0, int b_kcontig0, int epilogue0,
                 const pt_gemm_problem* p1, int n1, int a_kcontig1, int b_kcontig1, int epilogue1, int order,
                 hipStream_t stream);
/* out (bf16, n contiguous elements) = bf16(p0 + p1), or bf16(residual + bf16(p0 + p1)) when
 * residual (bf16, n contiguous) is given (= the EPI_BF16_RES epilogue): the finishing pass of a GEMM
 * split in two K halves (two f32 problems of one pt_gemm_grouped launch, 256x256 tiles).  n % 4 == 0,
 * p0 / p1 16-byte, out / residual 8-byte aligned; residual may alias out. */
int pt_gemm_splitk_sum(const float* p0, const float* p1, const void* residual, void* out, int64_t n,
                       hipStream_t stream);
/* Split-K finish for nparts f32 partials [nparts][M][N] (ld N, part_stride >= M N elements apart):
 * the sum in part order through `mode` = the GEMM epilogue it completes -- 0 bf16 store, 1 bf16
 * accumulate, 2 f32 store, 3 f32 accumulate (main_grad), 4 bf16 residual (residual [M, N], ld ldr),
 * 6 SwiGLU backward (the sum is dh of a split-K down_proj dX, model.py:186; residual = g|u [M, 2N]
 * ld ldr; C[0] = dg|du [M, 2N], nc = 1) -- into nc (<= 4) row segments of C (c_bounds, NULL = one),
 * each with its own ld.  N % 4 == 0. */
int pt_gemm_splitk_reduce(const float* parts, int nparts, int64_t part_stride, int64_t M, int64_t N, void* const* C,
                          const int64_t* ldc, const int64_t* c_bounds, int nc, int mode, const void* residual,
                          int64_t ldr, hipStream_t stream);

/* ---- ring-attention merge ------------------------------------------------------------------
 * replaces picotron/context_parallel/context_parallel.py:157-187 update_out_and_lse (its non-first
 * call): out_new = out - sigmoid(blse - lse) * (out - block_out), lse_new = lse - logsigmoid(lse -
 * blse).  out / out_new f32 [rows, D]; block_out [rows, D] (dtype 0 bf16, 1 f32); lse, block_lse,
 * lse_new [rows] in lse_dtype (0 bf16: every lse-side op rounded to bf16 as the reference's bf16
 * ring does; 1 f32).  All contiguous; rows = B * H * S.  (The ring's own merge is fused into
 * pt_attn_fwd's merge mode.) */
int pt_lse_merge(const float* out, const void* block_out, int block_out_dtype, const void* lse, const void* block_lse,
                 int lse_dtype, float* out_new, void* lse_new, int64_t rows, int64_t D, hipStream_t stream);

/* ---- flash attention ----------------------------------------------------------------------
 * replaces model.py:33-37,154 flash_attn_func(causal=True) / model.py:157 SDPA, and the ring
 * blocks context_parallel.py:112-155 with update_out_and_lse (:157-187) fused (merge = 1).
 * q/k/v/o/dout/dq/dk/dv: token-major [B, S, H, D] views given as base + 3 strides
 * {batch, seq, head} (elements; d contiguous).  lse, delta: f32 [B, H, Sq] whose (b, h) rows are
 * lse_ld elements apart (0: Sq, dense; larger: the Sq rows are a slice of a longer sequence's LSE,
 * as the zig-zag ring's half-sequence blocks use).  D in {64, 128},
 * Sq % 128 == 0, Sk % 64 == 0 (bwd: Sk % 128 == 0).  causal: key j visible to query i iff j <= i.
 * bwd rope_cos/rope_sin (may be NULL): [S, rope_stride] bf16 tables; dq and dk are then stored
 * rotated back by -theta (pt_rope inverse fused; positions = query / key index, Sq == Sk, bf16). */
int pt_attn_fwd(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                const int64_t* v_str, void* o, const int64_t* o_str, float* lse, int64_t B, int64_t H, int64_t HKV,
                int64_t Sq, int64_t Sk, int64_t D, float scale, int causal, int merge, int64_t lse_ld,
                hipStream_t stream);
int pt_attn_bwd_delta(const void* dout, const int64_t* do_str, const void* o, const int64_t* o_str, float* delta,
                      int64_t B, int64_t H, int64_t Sq, int64_t D, int64_t lse_ld, hipStream_t stream);
int pt_attn_bwd(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                const int64_t* v_str, const void* dout, const int64_t* do_str, const float* lse, const float* delta,
                void* dq, const int64_t* dq_str, void* dk, const int64_t* dk_str, void* dv, const int64_t* dv_str,
                int64_t B, int64_t H, int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, float scale, int causal,
                int grad_f32, const void* rope_cos, const void* rope_sin, int64_t rope_stride, int64_t lse_ld,
                hipStream_t stream);
/* pt_attn_bwd computing only dQ (parts = 1) or only dK / dV (parts = 2), or both (3); the pointers
 * of a gradient not computed may be NULL.  The context-parallel mesh backward
 * (context_parallel.py:72-106's ring, restated for the xGMI full mesh) runs each rank's dQ against
 * the visiting K / V and its own keys' dK / dV against the visiting queries, so no dK / dV partial
 * travels. */
int pt_attn_bwd_part(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                     const int64_t* v_str, const void* dout, const int64_t* do_str, const float* lse,
                     const float* delta, void* dq, const int64_t* dq_str, void* dk, const int64_t* dk_str, void* dv,
                     const int64_t* dv_str, int64_t B, int64_t H, int64_t HKV, int64_t Sq, int64_t Sk, int64_t D,
                     float scale, int causal, int grad_f32, int64_t lse_ld, int parts, hipStream_t stream);
/* pt_attn_bwd with the FA2 'D' = rowsum(dO * O) computed inside the dQ kernel (run first) from o
 * (bf16 [B, S, H, D] strides o_str) and written to delta_out [B, H, Sq] f32, which the dK/dV kernel
 * then reads: the separate pt_attn_bwd_delta pass disappears.  bf16 gradients only (no grad_f32). */
int pt_attn_bwd_fused_delta(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str,
                            const void* v, const int64_t* v_str, const void* o, const int64_t* o_str,
                            const void* dout, const int64_t* do_str, const float* lse, float* delta_out, void* dq,
                            const int64_t* dq_str, void* dk, const int64_t* dk_str, void* dv,
                            const int64_t* dv_str, int64_t B, int64_t H, int64_t HKV, int64_t Sq, int64_t Sk,
                            int64_t D, float scale, int causal, const void* rope_cos, const void* rope_sin,
                            int64_t rope_stride, int64_t lse_ld, hipStream_t stream);
/* Few-head attention (a TP shard's heads: the regular launch -- one workgroup per causal query-block
 * pair -- would put fewer than 128 workgroups on the 256 CUs): the same flash_attn_func forward /
 * backward as work items of "attn_kv_chunk" K/V (Q) tiles, f32 partials in a caller-owned workspace,
 * and a merge / reduce pass.  pt_attn_split_plan: 1 and the workspace bytes when the split forms
 * apply to the shape (d64), else 0.  pt_attn_fwd_split = pt_attn_fwd with merge = 0 and a dense lse;
 * pt_attn_bwd_split = pt_attn_bwd_fused_delta with a dense lse.  Results equal the regular kernels' up
 * to the f32 summation order. */
int pt_attn_split_plan(int64_t B, int64_t H, int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, int causal,
                       int backward, int64_t* ws_bytes);
int pt_attn_fwd_split(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                      const int64_t* v_str, void* o, const int64_t* o_str, float* lse, int64_t B, int64_t H,
                      int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, float scale, int causal, void* ws,
                      int64_t ws_bytes, hipStream_t stream);
int pt_attn_bwd_split(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                      const int64_t* v_str, const void* o, const int64_t* o_str, const void* dout, const int64_t* do_str,
                      const float* lse, float* delta_out, void* dq, const int64_t* dq_str, void* dk,
                      const int64_t* dk_str, void* dv, const int64_t* dv_str, int64_t B, int64_t H, int64_t HKV,
                      int64_t Sq, int64_t Sk, int64_t D, float scale, int causal, const void* rope_cos,
                      const void* rope_sin, int64_t rope_stride, void* ws, int64_t ws_bytes, hipStream_t stream);
/* Band attention: document-masked ("varlen") and sliding-window causal attention, one mechanism.
 * For batch row b, key j is visible to query i iff kv_lo[b, i] <= j <= i.  kv_lo: int32 [B, S],
 * 0 <= kv_lo[b, i] <= i, non-decreasing in i -- the first token of i's document (documents packed
 * back to back in one row), i - W + 1 for a window of W >= 1 keys, or the larger of the two.  q_hi:
 * int32 [B, S], the key-side companion the dK/dV kernel walks: q_hi[b, j] = the first i with
 * kv_lo[b, i] > j, or S (one past the last query that sees key j; non-decreasing, q_hi[b, j] > j).
 * The two must describe the same mask; the kernels trust them (their tile ranges are clamped to the
 * sequence, so a wrong bound gives a wrong mask, not a wrong address).  Positions for the fused RoPE
 * inverse are sequence indices: RoPE scores depend on i - j only, so per-document position resets
 * would give the same attention.
 * pt_attn_fwd_band = pt_attn_fwd (causal, merge = 0, dense lse); pt_attn_bwd_band =
 * pt_attn_bwd_fused_delta (causal, bf16 gradients, dense lse, optional RoPE inverse).  Sq == Sk,
 * S % 128 == 0, D in {64, 128} (else PT_EUNSUPPORTED); a NULL bound is PT_EINVAL.  A refused call
 * launches nothing.  With kv_lo = 0 everywhere (q_hi = S) the results are bit-identical to the causal
 * kernels'.  The dK/dV kernel form follows "attn_split" as for causal calls; the few-head split forms
 * are not used under a band. */
int pt_attn_fwd_band(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                     const int64_t* v_str, void* o, const int64_t* o_str, float* lse, int64_t B, int64_t H,
                     int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, float scale, const int32_t* kv_lo,
                     const int32_t* q_hi, hipStream_t stream);
int pt_attn_bwd_band(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                     const int64_t* v_str, const void* o, const int64_t* o_str, const void* dout,
                     const int64_t* do_str, const float* lse, float* delta_out, void* dq, const int64_t* dq_str,
                     void* dk, const int64_t* dk_str, void* dv, const int64_t* dv_str, int64_t B, int64_t H,
                     int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, float scale, const void* rope_cos,
                     const void* rope_sin, int64_t rope_stride, const int32_t* kv_lo, const int32_t* q_hi,
                     hipStream_t stream);
/* Block bands: the band of one block of a context-parallel schedule (a rank's queries against one
 * owner's keys), where the block is rectangular and usually not causal.  Key j of the block is
 * visible to query i of batch row b iff kv_lo[b, i] <= j, and also j <= i when causal = 1 (the
 * diagonal block; Sq == Sk).  kv_lo: int32 [B, Sq], 0 <= kv_lo <= Sk, non-decreasing in i; Sk = the
 * row sees no key of this block.  q_hi: int32 [B, Sk], q_hi[b, j] = the first i with kv_lo[b, i] > j,
 * or Sq; non-decreasing, 0 <= q_hi <= Sq; 0 = no query of this block sees key j.  Both are dense
 * whatever lse_ld is.
 * pt_attn_fwd_block_band = pt_attn_fwd plus the bounds (causal 0 / 1, merge 0 / 1, lse_ld);
 * pt_attn_bwd_block_band = pt_attn_bwd_part plus the bounds (the given delta, grad_f32 0 / 1, parts
 * 1 / 2 / 3, lse_ld, causal 0 / 1).  Sq % 128 == 0, Sk % 128 == 0 (forward: Sk % 64), D in {64, 128}.
 *  - Trivial bounds (kv_lo = 0, q_hi = Sq): bit-identical to pt_attn_fwd / pt_attn_bwd_part called with
 *    the same causal, merge, grad_f32, lse_ld and parts.
 *  - A query row with no visible key in the block: merge = 1 leaves its accumulator row and its
 *    running LSE bitwise untouched (also a running LSE of -inf); merge = 0 stores o = 0, lse = -inf;
 *    the backward (lse: the global, finite one) adds exactly 0 to dQ, dK and dV.  No NaN is formed.
 *  - A key no query sees (q_hi = 0): dK = dV = 0 (f32 accumulators keep their value).
 *  - The bounds are trusted but clamped: a wrong bound gives a wrong mask, never a wrong address.
 *  - A NULL bound is PT_EINVAL; causal with Sq != Sk is PT_EUNSUPPORTED.  A refused call launches
 *    nothing.
 * The dK/dV kernel form follows "attn_split" and causal blocks pair under "attn_pair", with identical
 * bits; the few-head split forms are not used. */
int pt_attn_fwd_block_band(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                           const int64_t* v_str, void* o, const int64_t* o_str, float* lse, int64_t B, int64_t H,
                           int64_t HKV, int64_t Sq, int64_t Sk, int64_t D, float scale, int causal, int merge,
                           int64_t lse_ld, const int32_t* kv_lo, const int32_t* q_hi, hipStream_t stream);
int pt_attn_bwd_block_band(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                           const int64_t* v_str, const void* dout, const int64_t* do_str, const float* lse,
                           const float* delta, void* dq, const int64_t* dq_str, void* dk, const int64_t* dk_str,
                           void* dv, const int64_t* dv_str, int64_t B, int64_t H, int64_t HKV, int64_t Sq, int64_t Sk,
                           int64_t D, float scale, int causal, int grad_f32, int64_t lse_ld, int parts,
                           const int32_t* kv_lo, const int32_t* q_hi, hipStream_t stream);

/* ---- measurement variants ------------------------------------------------------------------
 * Not a reference interface: selects between kernel forms with identical results, for A/B runs and
 * the bit-identity tests.  The library reads no environment; the host sets these (picotron_amd/
 * switches.py reads PICOTRON_<NAME> once at import and pushes them here).  Names and defaults:
 *   "attn_pair"     1   causal attention: pair query/key blocks (i, n-1-i) per workgroup
 *   "attn_split"    2   dK/dV kernel form per head dim: bit 0 = d64, bit 1 = d128 use the wave pair
 *   "gemm_mix"      1   q|k|v + RoPE GEMM as one mixed 256x256 / 256x128 launch
 *   "gemm_kh"       2   auto-picked 256x128 tiles as tile 14 (K-halves) when K >= 4096; 0 never
 *   "attn_kv_chunk" 4   few-head attention (pt_attn_split_plan): K / Q tiles per work item (even;
 *                       0 = never split)
 * Returns PT_EINVAL for an unknown name.  pt_get_variant returns the value (or PT_EINVAL). */
int pt_set_variant(const char* name, int value);
int pt_get_variant(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* PICOTRON_HIP_H */
