// Every C++ function of the library that one translation unit defines and another calls, declared once.  Together
// with b4r_common.h (error text, launch timing, the reduce queue) these are all the b4r_ prototypes there are: a .hip file holds none.
// The file that defines a function includes this header too, so a wrong return type or a repeated default argument does not
// compile; a wrong parameter type declares an overload nobody defines, which the link (-Wl,--no-undefined) refuses.
// Default arguments stand here and nowhere else.  Host code only.
// Four functions below have external linkage and no caller in another file today (b4r_launch_slab_reduce, b4r_head32_dE_slices:
// called in their own files only; b4r_scatter_hot_scratch_floats, b4r_batch_colsum: not called at all).  They are declared here so
// that the exported C++ symbols and this list stay equal; giving them internal linkage changes the host object code of their files.
#pragma once
#include "b4r_common.h"

// ---- b4r_gemm.hip: ordered two-stage reductions (queued while a B4rReduceQueue is active) and the split-K / paired TN products ----
int b4r_launch_slab_reduce(const float* slab, int S, int Mo, int No, float* out, int ldo, int accumulate,
                           hipStream_t stream);
int b4r_launch_slab_reduce_full(const float* slab, int S, int Mo, int No, float* out, int ldo, int accumulate,
                                const float* cslab, float* colsum, const float* caslab, float* colsum_a, hipStream_t stream);
int b4r_gemm_f32_splitk(const b4r_gemm_desc* d, int splits, float* scratch, int k_pad_ok, hipStream_t stream);
int b4r_gemm_tn_pair(const b4r_gemm_tn_desc* d0, float* scratch0, const b4r_gemm_tn_desc* d1, float* scratch1, hipStream_t stream);

// ---- b4r_gemm_rx.hip: the split-precision products behind b4r_gemm.hip's entry points ----------------------------------------------
int b4r_gemm_rx_launch(const b4r_gemm_desc* d, hipStream_t stream);
bool b4r_gemm_rx_supported(const b4r_gemm_desc* d);
bool b4r_gemm_rx_tn_supported(const b4r_gemm_tn_desc* d);
int64_t b4r_gemm_rx_tn_scratch_floats(int R, int Mo, int No);
int b4r_gemm_rx_tn_launch(const b4r_gemm_tn_desc* d, float* scratch, hipStream_t stream);
bool b4r_gemm_rx_tn_pair_supported(const b4r_gemm_tn_desc* d0, const b4r_gemm_tn_desc* d1);
int b4r_gemm_rx_tn_pair_launch(const b4r_gemm_tn_desc* d0, float* scratch0, const b4r_gemm_tn_desc* d1, float* scratch1,
                               hipStream_t stream);
bool b4r_gemm_rx_splitk_supported(const b4r_gemm_desc* d, int k_pad_ok);
int b4r_gemm_rx_splitk_launch(const b4r_gemm_desc* d, int splits, float* slabs, int* slabs_used, hipStream_t stream);

// ---- b4r_rowops.hip: LayerNorm backward, scatter-add, embedding gradients, loss sums, gradient clear, optimizer --------------------
int b4r_ln_bwd_launch(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                      int rows, int H, float* dz, float* dgamma, float* dbeta, float* scratch, const int64_t* ids,
                      const float* table, const float* pos_table, int L, int V, DropArgs drop, hipStream_t stream,
                      const float* gelu_pre = nullptr, const B4rHeadMerge* merge = nullptr, int act = B4R_ACT_GELU);
int b4r_scatter_add_rows_impl(const float* src, const int64_t* idx, int64_t idx_add_per, int per, int n, int H,
                              float* dst, int dst_ld, const int64_t* skip_if_zero, int64_t dst_rows, int hot_rows,
                              float* hot_scratch, hipStream_t stream);
int64_t b4r_scatter_hot_scratch_floats(int hot_rows, int H);
int b4r_batch_colsum(const float* x, int B, int L, int H, float* dpos, float* scratch, hipStream_t stream);
int b4r_embed_grads(const float* x, const int64_t* ids, int B, int L, int H, float* table_grad, int64_t V, int hot_rows,
                    float* fixed, float* dpos, float* colsum_scratch, hipStream_t stream, const float* fin_rows = nullptr,
                    int fin_M = 0, b4r_train_state* state = nullptr, float* tail = nullptr);
int64_t b4r_embed_fixed_floats(int64_t V, int H, int hot_rows);
int b4r_ce_finalize_launch(const float* row_scratch, int M, b4r_train_state* state, int overwrite, hipStream_t stream);
int b4r_zero2(float* a, int64_t na, float* b, int64_t nb, hipStream_t stream, float* tail = nullptr, b4r_train_state* state = nullptr,
              const float* fin_rows = nullptr, int fin_M = 0, const void* rider = nullptr, int rider_blocks = 0);
int b4r_optimizer_fused(const b4r_adamw_config* hp, float* params, const float* grads, float* adam_m, float* adam_v, int64_t n,
                        int64_t n_decay, float* scratch, b4r_train_state* state, hipStream_t stream, int sums_from_tail = 0,
                        int np_given = 0);
// b4r_rowops.hip: the last layer's feed-forward half on the masked-LM head's rows (compact [B*P, .] operands)
int b4r_slot_rows_gather(const float* a, const float* b, const float* s0, const float* s1, const int64_t* pos, int L, int P, int M, int H,
                         float* ac, float* bc, float* s0c, float* s1c, hipStream_t s);
int b4r_slot_rows_drop(const float* src, const int64_t* pos, int L, int P, int M, int H, const DropArgs& drop, float* dst, hipStream_t s);
int b4r_slot_rows_tail(const float* y, const float* res, const int64_t* pos, int L, int P, int M, int H, const float* gamma, const float* beta,
                       float eps, const DropArgs& drop, float* z, float* mean, float* rstd, float* out, float* outc, hipStream_t s);

// ---- b4r_attn_rx.hip: the attention core on 16-token tiles (b4r_attn_fwd / b4r_attn_bwd in the bf16x3 mode; argument checks done there)
int64_t b4r_attn_rx_keep_words(int B, int L, int heads);
int b4r_attn_rx_fwd_launch(const float* qkv, const int64_t* mask, int B, int L, int heads, float* ctx, float* lse,
                           const DropArgs& drop, uint32_t* keep_bits, hipStream_t stream);
int b4r_attn_rx_bwd_launch(const float* qkv, const int64_t* mask, const float* ctx, const float* lse, const float* dctx,
                           int B, int L, int heads, float qscale, float* dqkv, const DropArgs& drop,
                           const uint32_t* keep_bits, hipStream_t stream);

// ---- b4r_attn32.hip: the attention block on 32-token tiles behind b4r_attn_block_fwd / b4r_attn_block_bwd -------------------------
int32_t b4r_attn32_supported(int32_t hidden_size, int32_t num_heads, int32_t L);
int32_t b4r_attn32_preferred(int32_t hidden_size, int32_t num_heads, int32_t L);   // supported AND long enough to pay
int b4r_attn32_fwd(const b4r_attn_block_desc* d, b4r_stream_t stream);
int b4r_attn32_bwd(const b4r_attn_block_bwd_desc* d, b4r_stream_t stream);
int64_t b4r_attn32_keep_words(int32_t B, int32_t L, int32_t heads);
// b4r_attn32.hip: the core on 32-token tiles (one workgroup per sequence and head, one launch each way), preferred from L = 65 to 224
bool b4r_attn32_core_preferred(int L);
bool b4r_attn32_core_fwd_wanted();
int b4r_attn32_core_fwd_launch(const float* qkv, const int64_t* mask, int B, int L, int heads, float* ctx, float* lse,
                               const DropArgs& drop, uint32_t* keep_bits, hipStream_t stream);
int b4r_attn32_core_bwd_launch(const float* qkv, const int64_t* mask, const float* ctx, const float* lse, const float* dctx, int B,
                               int L, int heads, float qscale, float* dqkv, const DropArgs& drop, const uint32_t* keep_bits,
                               hipStream_t stream);
// b4r_attn32.hip: the attention core with the queries restricted to the masked-LM slots (compact [B*P, .] outputs)
bool b4r_attn32_slotq_supported(int L, int P);
int64_t b4r_attn32_slotq_keep_words(int B, int L, int heads, int P);
int b4r_attn32_slotq_fwd_launch(const float* qkv, const int64_t* mask, const int64_t* pos, int B, int L, int heads, int P, float* ctx_c,
                                float* lse_c, const DropArgs& drop, uint32_t* bits_c, hipStream_t stream);
int b4r_attn32_slotq_bwd_launch(const float* qkv, const int64_t* mask, const int64_t* pos, const int64_t* ids, const float* ctx_c,
                                const float* lse_c, const float* dctx_c, int B, int L, int heads, int P, float qscale, float* dqkv,
                                const DropArgs& drop, const uint32_t* bits_c, hipStream_t stream);

// ---- b4r_attn_block.hip ---------------------------------------------------------------------------------------------------------------
bool b4r_attn32_active(int H, int heads, int L);   // the 32-token-tile backward (it can form dWqkv / dbqkv itself)

// ---- b4r_head32.hip: masked-LM head of a train step without materialised logits (hidden size 64 / 128 / 256, bf16x3 mode) ---------
bool b4r_head32_hidden_ok(int H);
int b4r_head32_fwd_slices(int M, int V, int H);
int b4r_head32_dE_slices(int M, int V, int H);
int64_t b4r_head32_fwd_scratch_floats(int M, int V, int H);
int64_t b4r_head32_dE_scratch_floats(int M, int V, int H);
bool b4r_head32_combine_foldable(int M, int V, int H);
int b4r_head32_fwd_launch(const float* T, const float* E, const float* bias, const int64_t* y, int M, int V, int H, float* scratch,
                          float* dT, float* row_out, float* lse, int32_t* ylab, int only_sweep, hipStream_t stream);
int b4r_head32_dE_pack_job(const float* T, const float* lse, const int32_t* ylab, int M, int V, int H, float* scratch, const float* fwd_part,
                           const int64_t* y, void* out, size_t out_bytes, int* blocks);
int b4r_head32_dE_launch(const float* T, const float* E, const float* bias, const float* lse, const int32_t* ylab, int M, int V, int H,
                         float* scratch, float* dE, float* db, hipStream_t stream, const float* fwd_part, const int64_t* y, int records_ready);

// ---- b4r_ffn32w.hip: the feed-forward half at hidden sizes 128 / 256 as one launch (forward without a backward to follow) ----------
bool b4r_ffn32w_supported(int H, int I);
int64_t b4r_ffn32w_rec_floats(int H, int I);
int b4r_ffn32w_fwd(const b4r_ffn_desc* d, float* recs, float* f, float* fpre, hipStream_t stream);
int b4r_ffn32w_bwd(const b4r_ffn_desc* d, float* recs, const float* fpre, float* df, float* dx1, bool records_ready, hipStream_t stream);

// ---- b4r_embed_proj.hip: the factorised embedding stage (embedding_width E < hidden size H) and its backward, one launch each -------
bool b4r_embed_proj_supported(int E, int H);
int64_t b4r_embed_proj_bwd_scratch_floats_impl(int N, int E, int H);
int b4r_embed_proj_fwd_launch(const int64_t* ids, int B, int L, const float* table, int V, const float* pos, const float* gamma,
                              const float* beta, int E, float eps, const float* Wp, const float* bp, int H, float* x0, float* mean,
                              float* rstd, DropArgs drop, hipStream_t stream);
int b4r_embed_proj_bwd_launch(const float* dx0, const int64_t* ids, int B, int L, const float* table, int V, const float* pos,
                              const float* gamma, const float* beta, int E, const float* mean, const float* rstd, const float* Wp, int H,
                              DropArgs drop, float* drows, float* dWp, float* dbp, float* dln, float* scratch, hipStream_t stream);

// ---- b4r_rank_full.hip --------------------------------------------------------------------------------------------------------------
// rnorm[j] = 1 / |table row j| for j < V, one thread per row (b4r_cosine_chain.h): enqueues the one launch and checks nothing; the
// caller's B4R_CHECK_LAUNCH after its own kernels covers it
void b4r_item_rnorm_launch(const float* table, int width, int V, float* rnorm, hipStream_t stream);
