// Model-level entry points: parameter / workspace layout and the launch sequences of one forward, loss, backward and
// optimizer step.  Host code only: every function just enqueues kernels on the caller's stream (hipGraph-capturable).
// The launchers of the other translation units that it sequences are declared in b4r_internal.h, with their default arguments.
//
// Follows  BERT4RecModel.call        bert4rec/models/bert4rec_model.py:110-149
//          Bert4RecEncoder.call      bert4rec/models/components/networks/bert4rec_encoder.py:186-231
//          (tfm TransformerEncoderBlock post-LN, Keras MultiHeadAttention, tfm MaskedLM: SURVEY.md §8 a4-a8)
//          train_step                bert4rec_model.py:151-173
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include <algorithm>
#include "b4r_common.h"
#include "b4r_internal.h"

// internal flag of b4r_backward (b4r_train_step sets it): the closing reduce launch also leaves the partial sums of squares of the
// gradients at the start of the workspace (dead by then) and their number in backward_impl's norm_np, so that the optimizer needs no
// norm launch
#define B4R_FLAG_NORM_PARTIALS_INTERNAL (1 << 20)
// internal flag of b4r_forward AND b4r_backward of one train step (b4r_train_step sets it on both; fused head + B4R_FLAG_LOSS_SUMS):
// the forward runs the head's vocabulary sweep only, the backward's dE launch merges the slices (dT, loss rows, lse, labels) in its
// prologue and the loss / metric sums are formed by one extra workgroup of the embedding-gradient launch -- one launch fewer
#define B4R_FLAG_DEFER_COMBINE_INTERNAL (1 << 21)

// ---- error message (thread local) ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void b4r_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" size_t b4r_last_error(char* buf, size_t cap) {
  const size_t n = strlen(g_err);
  if (buf && cap) {
    const size_t c = n < cap - 1 ? n : cap - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return n;
}
extern "C" int b4r_version(void) { return B4R_VERSION; }

// ---- launch timing ----------------------------------------------------------------------------------------------------------
namespace {
struct TimingRec {
  bool on = false;
  hipStream_t stream = nullptr;
  std::vector<hipEvent_t> ev;       // ev[0] = begin, ev[i + 1] = after launch i
  std::vector<std::string> names;
  char detail[96] = "";
};
thread_local TimingRec g_tr;
}  // namespace

void b4r_timing_detail(const char* fmt, ...) {
  if (!g_tr.on) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_tr.detail, sizeof(g_tr.detail), fmt, ap);
  va_end(ap);
}
void b4r_timing_mark(const char* what) {
  if (!g_tr.on || g_tr.names.size() + 1 >= g_tr.ev.size()) return;
  std::string n(what);
  if (g_tr.detail[0]) { n += " ["; n += g_tr.detail; n += "]"; g_tr.detail[0] = 0; }
  if (hipEventRecord(g_tr.ev[g_tr.names.size() + 1], g_tr.stream) == hipSuccess) g_tr.names.push_back(n);
}
extern "C" int b4r_timing_begin(b4r_stream_t stream, int32_t max_launches) {
  B4R_CHECK_ARG(!g_tr.on, B4R_E_BADARG, "b4r_timing_begin: a recording is already active on this thread");
  B4R_CHECK_ARG(max_launches > 0 && max_launches <= 1 << 16, B4R_E_BADARG, "b4r_timing_begin: bad capacity");
  g_tr.ev.assign((size_t)max_launches + 1, nullptr);
  for (auto& e : g_tr.ev)
    if (hipEventCreate(&e) != hipSuccess) { b4r_set_error("b4r_timing_begin: hipEventCreate failed"); return B4R_E_HIP; }
  g_tr.names.clear();
  g_tr.stream = (hipStream_t)stream;
  g_tr.detail[0] = 0;
  if (hipEventRecord(g_tr.ev[0], g_tr.stream) != hipSuccess) { b4r_set_error("b4r_timing_begin: hipEventRecord failed"); return B4R_E_HIP; }
  g_tr.on = true;
  return B4R_OK;
}
extern "C" int b4r_timing_end(int32_t* n_launches, float* micros, char* names, int32_t name_stride, int32_t capacity) {
  B4R_CHECK_ARG(g_tr.on, B4R_E_BADARG, "b4r_timing_end: no recording is active on this thread");
  g_tr.on = false;
  const int n = (int)g_tr.names.size();
  int rc = B4R_OK;
  if (n > 0 && hipEventSynchronize(g_tr.ev[n]) != hipSuccess) { b4r_set_error("b4r_timing_end: hipEventSynchronize failed"); rc = B4R_E_HIP; }
  const int m = n < capacity ? n : capacity;
  for (int i = 0; i < m && rc == B4R_OK; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_tr.ev[i], g_tr.ev[i + 1]) != hipSuccess) { b4r_set_error("b4r_timing_end: hipEventElapsedTime failed"); rc = B4R_E_HIP; break; }
    if (micros) micros[i] = ms * 1e3f;
    if (names && name_stride > 0) snprintf(names + (size_t)i * name_stride, (size_t)name_stride, "%s", g_tr.names[i].c_str());
  }
  for (auto e : g_tr.ev) if (e) (void)hipEventDestroy(e);
  g_tr.ev.clear();
  if (n_launches) *n_launches = m;
  return rc;
}

namespace {

#define RC(x)                 \
  do {                        \
    int rc__ = (x);           \
    if (rc__ != B4R_OK) return rc__; \
  } while (0)

inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline int64_t up32(int64_t x) { return (x + 31) & ~(int64_t)31; }

// the width of one attention head, 32 or 64 (check_cfg)
inline int head_dim(const b4r_model_config* c) { return c->hidden_size / c->num_heads; }

int check_cfg(const b4r_model_config* c) {
  B4R_CHECK_ARG(c != nullptr, B4R_E_BADARG, "null model config");
  B4R_CHECK_ARG(c->vocab_size > 0 && c->num_heads > 0 && c->inner_dim > 0 && c->max_seq_len > 0, B4R_E_SHAPE, "bad model config");
  B4R_CHECK_ARG(c->num_layers > 0 && c->num_layers <= B4R_MAX_LAYERS, B4R_E_SHAPE, "num_layers %d not supported (1 ... %d)",
                c->num_layers, B4R_MAX_LAYERS);
  B4R_CHECK_ARG(c->hidden_size == 32 * c->num_heads || c->hidden_size == 64 * c->num_heads, B4R_E_SHAPE,
                "hidden_size %d / num_heads %d: head_dim must be 32 or 64", c->hidden_size, c->num_heads);
  const int H = c->hidden_size;
  B4R_CHECK_ARG(H == 32 || H == 64 || H == 128 || H == 256 || H == 512 || H == 1024, B4R_E_SHAPE,
                "hidden_size %d not supported (32,64,128,256,512,1024)", H);
  B4R_CHECK_ARG(c->inner_dim % 4 == 0, B4R_E_SHAPE, "inner_dim must be a multiple of 4");
  B4R_CHECK_ARG(c->output_dropout >= 0.f && c->output_dropout < 1.f && c->attention_dropout >= 0.f && c->attention_dropout < 1.f,
                B4R_E_BADARG, "dropout rates must be in [0,1)");
  return B4R_OK;
}

// The model configuration every internal function takes: the classic fields plus the resolved embedding width E (== hidden_size for
// the unfactorised model).  The classic entry points reach the same code through b4r_model_config_ex with embedding_width = 0.
struct ModelCfg : b4r_model_config {
  int E;
  int act_inner, act_mlm;   // the feed-forward blocks' and the masked-LM transform's activations (B4R_ACT_*)
  bool factorised() const { return E != hidden_size; }
};

b4r_model_config_ex classic_ex(const b4r_model_config* c) {
  b4r_model_config_ex x{};
  if (c) x.base = *c;
  return x;
}

// validates the extended config and resolves E and the activations; a bad width, a bad activations word or a nonzero reserved word is
// an error, never a fault
int resolve_cfg(const b4r_model_config_ex* x, ModelCfg* out) {
  B4R_CHECK_ARG(x != nullptr, B4R_E_BADARG, "null model config");
  RC(check_cfg(&x->base));
  B4R_CHECK_ARG(x->reserved[0] == 0 && x->reserved[2] == 0, B4R_E_BADARG,
                "b4r_model_config_ex: reserved words must be zero");
  const uint32_t acts = (uint32_t)x->reserved[1];
  const int act_inner = (int)(acts & 0xFFu), act_mlm = (int)((acts >> 8) & 0xFFu);
  B4R_CHECK_ARG((acts >> 16) == 0 && act_inner < B4R_ACT_COUNT && act_mlm < B4R_ACT_COUNT, B4R_E_BADARG,
                "b4r_model_config_ex: activations word (reserved[1]) 0x%x: bits 0-7 and 8-15 must be activation ids below %d, the "
                "other bits zero", acts, (int)B4R_ACT_COUNT);
  const int H = x->base.hidden_size, E = x->embedding_width;
  B4R_CHECK_ARG(E == 0 || E == H || ((E == 64 || E == 128 || E == 256) && E < H && b4r_embed_proj_supported(E, H)), B4R_E_SHAPE,
                "embedding_width %d not supported with hidden_size %d (0, hidden_size, or 64 / 128 / 256 below hidden_size)", E, H);
  static_cast<b4r_model_config&>(*out) = x->base;
  out->E = (E == 0) ? H : E;
  out->act_inner = act_inner; out->act_mlm = act_mlm;
  return B4R_OK;
}

struct ParamEntry {
  std::string name;
  int64_t offset;
  int rows, cols, ld, decay;
};

struct ParamLayout {
  int64_t total = 0, n_decay = 0;
  int64_t word_emb = 0, pos_emb = 0, emb_ln_g = 0, emb_ln_b = 0;
  int64_t proj_w = -1, proj_b = -1;   // embedding_projection kernel [E,H] / bias [H] (factorised only)
  int64_t wqkv[B4R_MAX_LAYERS], wo[B4R_MAX_LAYERS], w1[B4R_MAX_LAYERS], w2[B4R_MAX_LAYERS];
  int64_t bqkv[B4R_MAX_LAYERS], bo[B4R_MAX_LAYERS], ln1_g[B4R_MAX_LAYERS], ln1_b[B4R_MAX_LAYERS], b1[B4R_MAX_LAYERS],
      b2[B4R_MAX_LAYERS], ln2_g[B4R_MAX_LAYERS], ln2_b[B4R_MAX_LAYERS];
  int64_t wd = 0, bd = 0, lnm_g = 0, lnm_b = 0, out_bias = 0;
  std::vector<ParamEntry> entries;
};

ParamLayout make_param_layout(const ModelCfg& c) {
  ParamLayout p;
  const int64_t H = c.hidden_size, I = c.inner_dim, V = c.vocab_size, Lm = c.max_seq_len, E = c.E;
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t o = off; off += up4(n); return o; };
  auto add = [&](const std::string& name, int64_t o, int rows, int cols, int ld, int decay) {
    p.entries.push_back(ParamEntry{name, o, rows, cols, ld, decay});
  };
  // ---- weight-decayed region: kernels and the two embedding tables
  p.word_emb = take(V * E); add("word_embeddings/embeddings", p.word_emb, (int)V, (int)E, (int)E, 1);
  p.pos_emb = take(Lm * E); add("position_embedding/embeddings", p.pos_emb, (int)Lm, (int)E, (int)E, 1);
  if (c.factorised()) { p.proj_w = take(E * H); add("embedding_projection/kernel", p.proj_w, (int)E, (int)H, (int)H, 1); }
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string pre = "transformer/layer_" + std::to_string(i);
    p.wqkv[i] = take(H * 3 * H);
    add(pre + "/self_attention/query/kernel", p.wqkv[i], (int)H, (int)H, (int)(3 * H), 1);
    add(pre + "/self_attention/key/kernel", p.wqkv[i] + H, (int)H, (int)H, (int)(3 * H), 1);
    add(pre + "/self_attention/value/kernel", p.wqkv[i] + 2 * H, (int)H, (int)H, (int)(3 * H), 1);
    p.wo[i] = take(H * H); add(pre + "/self_attention/attention_output/kernel", p.wo[i], (int)H, (int)H, (int)H, 1);
    p.w1[i] = take(H * I); add(pre + "/intermediate/kernel", p.w1[i], (int)H, (int)I, (int)I, 1);
    p.w2[i] = take(I * H); add(pre + "/output/kernel", p.w2[i], (int)I, (int)H, (int)H, 1);
  }
  p.wd = take(H * E); add("cls/predictions/transform/dense/kernel", p.wd, (int)H, (int)E, (int)E, 1);
  p.n_decay = off;
  // ---- not decayed: every bias and LayerNorm gamma/beta
  p.emb_ln_g = take(E); add("embeddings/layer_norm/gamma", p.emb_ln_g, 1, (int)E, (int)E, 0);
  p.emb_ln_b = take(E); add("embeddings/layer_norm/beta", p.emb_ln_b, 1, (int)E, (int)E, 0);
  if (c.factorised()) { p.proj_b = take(H); add("embedding_projection/bias", p.proj_b, 1, (int)H, (int)H, 0); }
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string pre = "transformer/layer_" + std::to_string(i);
    p.bqkv[i] = take(3 * H);
    add(pre + "/self_attention/query/bias", p.bqkv[i], 1, (int)H, (int)H, 0);
    add(pre + "/self_attention/key/bias", p.bqkv[i] + H, 1, (int)H, (int)H, 0);
    add(pre + "/self_attention/value/bias", p.bqkv[i] + 2 * H, 1, (int)H, (int)H, 0);
    p.bo[i] = take(H); add(pre + "/self_attention/attention_output/bias", p.bo[i], 1, (int)H, (int)H, 0);
    p.ln1_g[i] = take(H); add(pre + "/self_attention_layer_norm/gamma", p.ln1_g[i], 1, (int)H, (int)H, 0);
    p.ln1_b[i] = take(H); add(pre + "/self_attention_layer_norm/beta", p.ln1_b[i], 1, (int)H, (int)H, 0);
    p.b1[i] = take(I); add(pre + "/intermediate/bias", p.b1[i], 1, (int)I, (int)I, 0);
    p.b2[i] = take(H); add(pre + "/output/bias", p.b2[i], 1, (int)H, (int)H, 0);
    p.ln2_g[i] = take(H); add(pre + "/output_layer_norm/gamma", p.ln2_g[i], 1, (int)H, (int)H, 0);
    p.ln2_b[i] = take(H); add(pre + "/output_layer_norm/beta", p.ln2_b[i], 1, (int)H, (int)H, 0);
  }
  p.bd = take(E); add("cls/predictions/transform/dense/bias", p.bd, 1, (int)E, (int)E, 0);
  p.lnm_g = take(E); add("cls/predictions/transform/LayerNorm/gamma", p.lnm_g, 1, (int)E, (int)E, 0);
  p.lnm_b = take(E); add("cls/predictions/transform/LayerNorm/beta", p.lnm_b, 1, (int)E, (int)E, 0);
  p.out_bias = take(V); add("cls/predictions/output_bias/bias", p.out_bias, 1, (int)V, (int)V, 0);
  p.total = off;
  return p;
}

// K splits of dT = dlogits.E: enough workgroups to cover the chip (tiles of 128 rows x 64 columns)
int mlm_dt_splits(int64_t M, int64_t H, int64_t V) {
  const int64_t tiles = ((M + 127) / 128) * ((H + 63) / 64);
  int64_t s = (512 + tiles - 1) / tiles;
  const int64_t max_s = (V + 255) / 256;
  if (s > max_s) s = max_s;
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  return (int)s;
}

struct WsLayout {
  int64_t total = 0;  // floats
  int64_t N = 0, M = 0, Vp = 0;
  int64_t x0, mean0, rstd0;
  int64_t qkv[B4R_MAX_LAYERS], lse[B4R_MAX_LAYERS], keep[B4R_MAX_LAYERS], ctx[B4R_MAX_LAYERS], z1[B4R_MAX_LAYERS], mean1[B4R_MAX_LAYERS],
      rstd1[B4R_MAX_LAYERS], x1[B4R_MAX_LAYERS], fpre[B4R_MAX_LAYERS], f[B4R_MAX_LAYERS], z2[B4R_MAX_LAYERS],
      mean2[B4R_MAX_LAYERS], rstd2[B4R_MAX_LAYERS], x2[B4R_MAX_LAYERS], ffnrec[B4R_MAX_LAYERS];
  int64_t gath, upre, u, meanm, rstdm, t, logits, rowsc, pooled, head_lse, head_ylab;
  int64_t dx, hot, da, db, dctx, dqkv, df, dt, dg;   // dx | hot | db adjacent: one fill clears dx + hot, or hot + db (row-list mode)
  int64_t dz2c, maxrows;   // row-list mode of the last layer's feed-forward half: one entry per masked-LM slot
  int64_t dzc_a, dzc_b;    // the same mode through the dense products (hidden sizes without the resident block): backward temporaries
  int64_t scratch, scratch_floats;
};

// (the masked-LM head's [B*P, .] rows keep their width-H regions when E < H: same offsets, the head uses the first E columns' worth)
WsLayout make_ws_layout(const ModelCfg& c, int B, int L, int P) {
  WsLayout w;
  const int64_t H = c.hidden_size, I = c.inner_dim, V = c.vocab_size, E = c.E;
  const int64_t N = (int64_t)B * L, M = (int64_t)B * (P > 0 ? P : 0);
  w.N = N; w.M = M; w.Vp = up32(V);
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t o = off; off += up4(n); return o; };
  w.x0 = take(N * H); w.mean0 = take(N); w.rstd0 = take(N);
  for (int i = 0; i < c.num_layers; ++i) {
    w.qkv[i] = take(N * 3 * H); w.lse[i] = take((int64_t)B * c.num_heads * L);
    w.keep[i] = take(b4r_attn_keep_words(B, L, c.num_heads));   // attention dropout decisions (uint32 words)
    w.ctx[i] = take(N * H);
    w.z1[i] = take(N * H); w.mean1[i] = take(N); w.rstd1[i] = take(N); w.x1[i] = take(N * H);
    w.fpre[i] = take(N * I); w.f[i] = take(N * I);
    w.z2[i] = take(N * H); w.mean2[i] = take(N); w.rstd2[i] = take(N); w.x2[i] = take(N * H);
    w.ffnrec[i] = take(b4r_ffn32w_supported((int)H, (int)I) ? b4r_ffn32w_rec_floats((int)H, (int)I) : 0);   // packed W1 / b1 / W2 records
  }
  w.gath = take(M * H); w.upre = take(M * H); w.u = take(M * H); w.meanm = take(M); w.rstdm = take(M);
  w.t = take(M * H); w.logits = take(M * w.Vp); w.rowsc = take(4 * M); w.pooled = take((int64_t)B * H);
  w.head_lse = take(M); w.head_ylab = take(M);
  w.dx = take(N * H); w.hot = take(b4r_embed_fixed_floats(c.vocab_size, (int)E, 3)); w.db = take(N * H); w.da = take(N * H); w.dctx = take(N * H);
  w.maxrows = M;
  w.dz2c = take(w.maxrows * H);
  w.dzc_a = take(M * H); w.dzc_b = take(M * H);
  w.dqkv = take(N * 3 * H); w.df = take(N * I); w.dt = take(M * H); w.dg = take(M * H);
  // scratch: every two-stage reduction of the backward pass keeps its partials until the single deferred reduce launch,
  // so the regions are summed (not max-ed); the two immediate reductions (split-K dT, position table) have their own
  int64_t s = 4096;
  auto add = [&](int64_t v) { s += up4(v); };
  for (int i = 0; i < c.num_layers; ++i) {
    add(b4r_gemm_tn_scratch_floats((int)N, (int)H, (int)(3 * H)));
    add(b4r_gemm_tn_scratch_floats((int)N, (int)H, (int)H));
    add(b4r_gemm_tn_scratch_floats((int)N, (int)H, (int)I));
    add(b4r_gemm_tn_scratch_floats((int)N, (int)I, (int)H));
    add(2 * std::max(b4r_ln_bwd_scratch_floats((int)N, (int)H), b4r_gemm_ln_bwd_partial_floats((int)N)));
    if (H == 64 && I == 256) add(b4r_ffn_block_bwd_scratch_floats((int)N));   // partial slabs of the fused feed-forward backward
    add(b4r_attn_block_bwd_scratch_floats(B));
    add(b4r_attn_block_bwd_dw_scratch_floats(B));
  }
  add(std::max(b4r_ln_bwd_scratch_floats((int)N, (int)H), b4r_gemm_ln_bwd_partial_floats((int)N)));
  if (M > 0) {
    add(b4r_gemm_tn_scratch_floats((int)M, (int)H, (int)I));   // the last layer's weight gradients over the head's rows only
    add(b4r_gemm_tn_scratch_floats((int)M, (int)I, (int)H));
    add(b4r_gemm_tn_scratch_floats((int)M, (int)V, (int)E));
    add(b4r_gemm_tn_scratch_floats((int)M, (int)H, (int)E));
    add(b4r_ln_bwd_scratch_floats((int)M, (int)E));
    add((int64_t)mlm_dt_splits(M, E, V) * M * E);
    if (b4r_head32_hidden_ok((int)E)) add(b4r_head32_dE_scratch_floats((int)M, (int)V, (int)E));
  }
  add((int64_t)b4r_cdiv(B, 16) * L * E);  // position-table gradient partials
  if (c.factorised()) add(b4r_embed_proj_bwd_scratch_floats_impl((int)N, (int)E, (int)H));   // the projection's slabs
  // the fused head's forward partials live at the start of the scratch region; a train step's backward merges them itself (its dE
  // launch), so they stay reserved in front of the backward's own regions
  if (M > 0 && b4r_head32_hidden_ok((int)E)) add(b4r_head32_fwd_scratch_floats((int)M, (int)V, (int)E));
  w.scratch = take(s); w.scratch_floats = s;
  w.total = off;
  return w;
}

int check_batch(const b4r_batch* b, const b4r_model_config* c, bool need_mlm) {
  B4R_CHECK_ARG(b != nullptr, B4R_E_BADARG, "null batch");
  B4R_CHECK_ARG(b->input_word_ids && b->input_mask, B4R_E_BADARG, "batch needs input_word_ids and input_mask");
  B4R_CHECK_ARG(b->B > 0 && b->L > 0 && b->P >= 0, B4R_E_SHAPE, "bad batch shape B=%d L=%d P=%d", b->B, b->L, b->P);
  B4R_CHECK_ARG(b->L <= c->max_seq_len, B4R_E_SHAPE, "sequence length %d exceeds max_sequence_length %d", b->L, c->max_seq_len);
  B4R_CHECK_ARG(b->L <= 256, B4R_E_SHAPE, "sequence length %d > 256 not supported", b->L);
  B4R_CHECK_ARG(!need_mlm || (b->masked_lm_positions && b->P > 0), B4R_E_BADARG, "batch needs masked_lm_positions");
  return B4R_OK;
}

int gemm_f32(const b4r_gemm_desc& d, hipStream_t s) { return b4r_gemm_f32(&d, s); }
int gemm_tn_f32(const b4r_gemm_tn_desc& d, float* scratch, hipStream_t s) { return b4r_gemm_tn_f32(&d, scratch, s); }
int64_t ln_scratch_floats(int N, int H) { return std::max(b4r_ln_bwd_scratch_floats(N, H), b4r_gemm_ln_bwd_partial_floats(N)); }

// dense + bias + dropout + residual (-> z) + LayerNorm (-> y, mean, rstd): one launch where b4r_gemm_ln_supported (hidden
// size 64 in the bf16x3 mode), else the product with B4R_EPI_BIAS_DROP_RES followed by b4r_ln_fwd.
int dense_res_ln(const float* A, int lda, const float* W, float* z, float* y, float* mean, float* rstd, int M, int H, int K,
                 const float* bias, const float* R, const float* gamma, const float* beta, float eps, const uint32_t* rng,
                 uint32_t stream_id, float rate, hipStream_t s) {
  b4r_gemm_desc d{.A = A, .lda = lda, .B = W, .ldb = H, .C = z, .ldc = H, .M = M, .N = H, .K = K, .epilogue = B4R_EPI_BIAS_DROP_RES_LN,
                  .bias = bias, .C2 = y, .ldc2 = H, .R = R, .ldr = H, .qscale = 1.f, .rng = rng, .drop_stream = stream_id,
                  .drop_rate = rate, .c_pad_scratch = 1, .ln_gamma = gamma, .ln_beta = beta, .ln_mean = mean, .ln_rstd = rstd,
                  .ln_eps = eps};
  if (b4r_gemm_ln_supported(&d)) return gemm_f32(d, s);
  d.epilogue = B4R_EPI_BIAS_DROP_RES; d.C2 = nullptr; d.ldc2 = 0;
  RC(gemm_f32(d, s));
  return b4r_ln_fwd(z, M, H, gamma, beta, eps, y, mean, rstd, s);
}

// input-gradient product + residual gradient + the LayerNorm backward in front of it:  dz = LN'(A.W^T + R)  (W as [N=H, K]).
// One launch where b4r_gemm_ln_supported, else B4R_EPI_ADD_RES into `dz` followed by b4r_ln_bwd in place.
// With `ids` the LayerNorm is the embedding stage's (input recomputed from the tables, dy first through the dropout `drop`).
int dgrad_ln_bwd(const float* A, int lda, const float* W, int K, const float* R, float* dz, int M, int H, const float* z,
                 const float* mean, const float* rstd, const float* gamma, float* dgamma, float* dbeta, float* scratch,
                 hipStream_t s, const int64_t* ids = nullptr, const float* table = nullptr, const float* pos_table = nullptr,
                 int L = 1, int V = 1, const uint32_t* rng = nullptr, uint32_t drop_stream = 0, float drop_rate = 0.f) {
  b4r_gemm_desc d{.A = A, .lda = lda, .B = W, .ldb = K, .C = dz, .ldc = H, .M = M, .N = H, .K = K, .b_is_nk = 1,
                  .epilogue = B4R_EPI_ADD_RES_LN_BWD, .C2 = scratch, .R = R, .ldr = H, .qscale = 1.f, .rng = rng,
                  .drop_stream = drop_stream, .drop_rate = drop_rate, .c_pad_scratch = 1, .ln_gamma = gamma,
                  .ln_mean = const_cast<float*>(mean), .ln_rstd = const_cast<float*>(rstd), .ln_z = z, .ln_ldz = H, .ln_dgamma = dgamma,
                  .ln_dbeta = dbeta, .ln_ids = ids, .ln_table = table, .ln_pos = pos_table, .ln_L = L, .ln_V = V};
  if (dbeta == dgamma + 64 && b4r_gemm_ln_supported(&d)) return gemm_f32(d, s);
  d.epilogue = B4R_EPI_ADD_RES; d.C2 = nullptr; d.rng = nullptr; d.drop_rate = 0.f;
  RC(gemm_f32(d, s));
  return b4r_ln_bwd_launch(dz, z, mean, rstd, gamma, M, H, dz, dgamma, dbeta, scratch, ids, table, pos_table, L, V,
                           b4r_make_drop(rng, drop_stream, drop_rate, 1), s, nullptr);
}

// gather + dense(gelu) + LayerNorm of the masked-LM transform (`d`: B4R_EPI_BIAS_GELU_LN with gathered A rows): one launch where the
// LayerNorm tail applies (hidden size 64), else the gathered rows into `gath`, the product and b4r_ln_fwd
int transform_fwd(const b4r_gemm_desc& d, float* gath, hipStream_t s) {
  if (b4r_gemm_ln_supported(&d)) return gemm_f32(d, s);
  RC(b4r_gather_rows(d.A, d.lda, d.a_gather_idx, d.a_gather_add_per, d.a_gather_per, d.M, d.K, gath, s));
  RC(gemm_f32({.A = gath, .lda = d.K, .B = d.B, .ldb = d.ldb, .C = d.C, .ldc = d.ldc, .M = d.M, .N = d.N, .K = d.K,
               .epilogue = B4R_EPI_BIAS_GELU, .bias = d.bias, .C2 = d.C3, .ldc2 = d.ldc3, .qscale = 1.f, .c_pad_scratch = 1,
               .activation = d.activation}, s));
  return b4r_ln_fwd(d.C, d.M, d.N, d.ln_gamma, d.ln_beta, d.ln_eps, d.C2, d.ln_mean, d.ln_rstd, s);
}

// dWo = ctx^T . dropmask(dz1) (+ dbo): the weight gradient of the attention output projection
b4r_gemm_tn_desc wo_grad_desc(const float* ctx, const float* dz1, float* dWo, float* dbo, int N, int H, const uint32_t* rng,
                              uint32_t drop_stream, float drop_rate) {
  return {.A = ctx, .lda = H, .B = dz1, .ldb = H, .out = dWo, .ldo = H, .R = N, .Mo = H, .No = H, .colsum = dbo, .rng = rng,
          .drop_stream = drop_stream, .drop_rate = drop_rate, .b_dropout = 1};
}
// ... and dWqkv = x^T . dqkv (+ dbqkv) in the same launch
int attn_wgrad_pair(const b4r_gemm_tn_desc& d_wo, float* wo_scratch, const float* x, const float* dqkv, float* dWqkv, float* dbqkv,
                    float* wqkv_scratch, hipStream_t s) {
  const int N = d_wo.R, H = d_wo.Mo;
  const b4r_gemm_tn_desc d_wqkv{.A = x, .lda = H, .B = dqkv, .ldb = 3 * H, .out = dWqkv, .ldo = 3 * H, .R = N, .Mo = H, .No = 3 * H,
                                .colsum = dbqkv};
  return b4r_gemm_tn_pair(&d_wo, wo_scratch, &d_wqkv, wqkv_scratch, s);
}

// ---- the launch plan of one step ----------------------------------------------------------------------------------------------
// Each half of an encoder layer runs in one of several forms.  plan_step picks them once for the forward and the backward of a
// step and is the only caller of the shape predicates behind them, so what a forward stores is what the backward of the same plan
// reads.  (The predicates read the gemm mode and the 32-token-tile length threshold: set those between steps only.)
// AttnFwd::Block: one launch (QKV product, attention core, output projection, dropout, residual, LayerNorm; b4r_attn_block.hip).
// SlotQuery: the last layer with the masked-LM slots as its only queries, outputs on compact [B*P, .] rows (b4r_attn32.hip).  Core:
// the QKV product, the attention core and the output projection with its LayerNorm as launches of their own.  AttnBwd::BlockFolded:
// the block's backward also forms dWqkv / dbqkv and dWo / dbo.  FfnForm::Block: one launch forward, two backward (b4r_ffn_rx.hip).
// CompactRows: the last layer on the head's rows only, products on compact [B*P, .] operands (b4r_slot_rows_*).  Wide: the one-launch
// pair of b4r_ffn32w.hip.  TileProducts: two products and the LayerNorm.
enum class AttnFwd { Block, SlotQuery, Core };
enum class AttnBwd { Block, BlockFolded, SlotQuery, Core };
enum class FfnForm { Block, CompactRows, Wide, TileProducts };
struct StepPlan {
  bool emb_fused;         // the embedding stage runs inside the first layer's attention block
  bool emb_proj;          // factorised: the embedding stage at width E and the E -> H projection, one launch each way (b4r_embed_proj.hip)
  bool head_rows;         // B4R_FLAG_HEAD_ROWS_ONLY honoured by the last layer's fused feed-forward block ...
  bool head_rows_dense;   // ... or by its compact products
  bool fused_head;        // B4R_FLAG_FUSED_HEAD
  bool defer_combine;     // B4R_FLAG_DEFER_COMBINE_INTERNAL with B4R_FLAG_LOSS_SUMS
  bool qkv_stored;        // the attention block's forward stores qkv: a backward other than the block's reads it
  bool x1_stored;         // ... and x1: the fused feed-forward half, which forms x1 from z1 on load, does not run
  bool slot_only_last;    // the last layer's attention block sweeps the slots' queries only and its backward reads the slots' dz1 only
  bool slotq_rows;        // the last layer's SlotQuery forward leaves the compact rows the compact feed-forward half reads
  AttnFwd attn_fwd[B4R_MAX_LAYERS];
  AttnBwd attn_bwd[B4R_MAX_LAYERS];
  FfnForm ffn[B4R_MAX_LAYERS];
  bool rows() const { return head_rows || head_rows_dense; }   // nothing but the head's rows leave the last layer
};

StepPlan plan_step(const ModelCfg* c, const b4r_batch* b, uint32_t flags) {
  const int H = c->hidden_size, I = c->inner_dim, L = b->L, P = b->P, heads = c->num_heads, last = c->num_layers - 1;
  const bool hro = (flags & B4R_FLAG_HEAD_ROWS_ONLY) != 0, slots = b->masked_lm_positions && b->masked_lm_ids && P > 0;
  // the halves as one launch each (attention: heads of width 32 only, the blocks stage [rows][32] head slices; its backward L <= 208)
  const bool ffn_fused = b4r_ffn_block_supported(H, I) != 0;
  const bool attn_fused = head_dim(c) == 32 && b4r_attn_block_supported(H, heads, L) != 0;
  const bool attn_bwd_fused = attn_fused && b4r_attn_block_bwd_supported(H, heads, L) != 0;
  const bool attn32 = b4r_attn32_active(H, heads, L);   // the 32-token-tile block backward: it can form the weight gradients itself
  StepPlan p{};
  p.emb_proj = c->factorised();
  p.emb_fused = attn_fused && c->num_layers > 0 && !p.emb_proj;
  p.head_rows = hro && ffn_fused && slots;
  // where the last feed-forward half runs as dense products (every hidden size but 64): on compact [B*P, .] operands.  Worth it when
  // the head reads a minority of the rows (P = L / 5 at the benchmark shapes).  Those operands live inside the last layer's own dense
  // regions (an encoder-only forward has nothing else, b4r_workspace_bytes_encoder): f / fpre / z2 / mean2 / rstd2 at the start of
  // theirs, and in the unused upper half of fpre [N, I] (2 M <= N, 3 H + 8 <= I): x1 rows, z1 rows, the second product's output,
  // mean1, rstd1 (compact_rows)
  p.head_rows_dense = hro && !ffn_fused && c->num_layers > 0 && slots && 2 * P <= L && H % 32 == 0 && I >= 3 * H + 8;
  p.fused_head = (flags & B4R_FLAG_FUSED_HEAD) != 0;
  p.defer_combine = (flags & B4R_FLAG_DEFER_COMBINE_INTERNAL) && (flags & B4R_FLAG_LOSS_SUMS);
  p.qkv_stored = !attn_bwd_fused;
  p.x1_stored = !(attn_fused && ffn_fused);
  // The block forward sweeps the slots' queries only where it is asked to (out_slot_positions) AND where its 32-token-tile kernel runs
  // (attn32), with P <= 64, L > 64, not for layer 0 and with qkv not stored (b4r_attn32_fwd); its backward then reads the slots' dz1
  // only (dz1_slot_positions).  Both are asked for under this one condition, so a slot-only forward never meets a dense backward.
  p.slot_only_last = p.head_rows && attn_bwd_fused && attn32;
  // the last layer's attention with the slots as its only queries: where that half runs as products, P <= 64, heads of width 32 (at
  // width 64 the last layer's attention runs dense and the rows are gathered after it)
  p.slotq_rows = p.head_rows_dense && head_dim(c) == 32 && !attn_fused && b4r_attn32_slotq_supported(L, P) &&
                 b4r_attn32_slotq_keep_words(b->B, L, heads, P) <= b4r_attn_keep_words(b->B, L, heads);
  // The one-launch feed-forward pair: no backward follows an encoder-only forward, so [N, inner] stays on the chip.  Inside a TRAIN
  // step (the launch then also writes f and the pre-activation) measured per dense layer at N = 51 200 -- hidden 128: forward 102 us
  // against 121 (two tile products + LayerNorm), backward 103 against 124; hidden 256: 323 against 320 and 403 against 313.  So:
  // hidden 128 only.
  const bool wide = b4r_ffn32w_supported(H, I) && ((flags & B4R_FLAG_ENCODER_ONLY) || H == 128);
  for (int i = 0; i <= last; ++i) {
    const bool slotq = p.slotq_rows && i == last;
    p.attn_fwd[i] = attn_fused ? AttnFwd::Block : slotq ? AttnFwd::SlotQuery : AttnFwd::Core;
    p.attn_bwd[i] = attn_bwd_fused ? (attn32 ? AttnBwd::BlockFolded : AttnBwd::Block) : slotq ? AttnBwd::SlotQuery : AttnBwd::Core;
    p.ffn[i] = ffn_fused ? FfnForm::Block
               : (p.head_rows_dense && i == last) ? FfnForm::CompactRows
               : wide ? FfnForm::Wide : FfnForm::TileProducts;
  }
  return p;
}

struct CompactRows { int64_t x1c, z1c, yc, mean1c, rstd1c; };
CompactRows compact_rows(const WsLayout& w, int layer, int64_t M, int64_t H, int64_t I) {
  CompactRows c;
  c.x1c = w.fpre[layer] + up4(M * I); c.z1c = c.x1c + M * H; c.yc = c.z1c + M * H; c.mean1c = c.yc + M * H; c.rstd1c = c.mean1c + up4(M);
  return c;
}

// What every form of a layer half reads: the step's shapes, buffers, plan, dropout and stream, and the backward's scratch allocator.
struct Step {
  const ModelCfg& cfg; const b4r_batch& batch; const StepPlan& plan; const int32_t flags;
  const ParamLayout pl; const WsLayout w;
  const float* const params; float* const grads; float* const ws; b4r_train_state* const state;
  const int B, L, P, H, I, V, N, M, last, E;
  const uint32_t* const rng;   // the dropout stream (training only)
  const float od, adp, qscale;
  const hipStream_t s;
  int64_t scratch_used = 0;

  Step(const ModelCfg* c, const b4r_batch* b, const StepPlan& p, const float* prm, float* g, void* workspace,
       b4r_train_state* st, int32_t f, hipStream_t stream)
      : cfg(*c), batch(*b), plan(p), flags(f), pl(make_param_layout(*c)), w(make_ws_layout(*c, b->B, b->L, b->P)), params(prm),
        grads(g), ws(static_cast<float*>(workspace)), state(st), B(b->B), L(b->L), P(b->masked_lm_positions ? b->P : 0),
        H(c->hidden_size), I(c->inner_dim), V(c->vocab_size), N(B * L), M(B * P), last(c->num_layers - 1), E(c->E),
        rng((f & B4R_FLAG_TRAINING) ? reinterpret_cast<const uint32_t*>(st) : nullptr),
        od((f & B4R_FLAG_TRAINING) ? c->output_dropout : 0.f), adp((f & B4R_FLAG_TRAINING) ? c->attention_dropout : 0.f),
        qscale(1.0f / sqrtf((float)head_dim(c))), s(stream) {}
  const float* prm(int64_t off) const { return params + off; }
  float* grd(int64_t off) const { return grads + off; }
  float* at(int64_t off) const { return ws + off; }
  uint32_t* keep(int i) const { return reinterpret_cast<uint32_t*>(ws + w.keep[i]); }
  // the next region of the backward's scratch; B4R_E_NOMEM, before anything is enqueued on it, where it would end past the scratch
  int take(int64_t n, float** out) {
    B4R_CHECK_ARG(scratch_used + up4(n) <= w.scratch_floats, B4R_E_NOMEM, "b4r_backward: internal scratch overflow");
    *out = ws + w.scratch + scratch_used; scratch_used += up4(n);
    return B4R_OK;
  }
};

// the fields every form of the feed-forward half shares: shapes, weights and the output dropout
b4r_ffn_desc ffn_desc(const Step& c, int i) {
  b4r_ffn_desc fd{};
  fd.N = c.N; fd.H = c.H; fd.I = c.I;
  fd.W1 = c.prm(c.pl.w1[i]); fd.b1 = c.prm(c.pl.b1[i]); fd.W2 = c.prm(c.pl.w2[i]); fd.b2 = c.prm(c.pl.b2[i]);
  fd.rng = c.od > 0.f ? c.rng : nullptr; fd.drop_stream = B4R_STREAM_FFN_OUT(i); fd.drop_rate = c.od;
  fd.activation = c.cfg.act_inner;
  return fd;
}
// ... and of its forward forms: the output LayerNorm and the outputs
b4r_ffn_desc ffn_fwd_desc(const Step& c, int i) {
  b4r_ffn_desc fd = ffn_desc(c, i);
  fd.ln_gamma = c.prm(c.pl.ln2_g[i]); fd.ln_beta = c.prm(c.pl.ln2_b[i]); fd.ln_eps = c.cfg.ln_eps;
  fd.z2 = c.at(c.w.z2[i]); fd.x2 = c.at(c.w.x2[i]); fd.mean2 = c.at(c.w.mean2[i]); fd.rstd2 = c.at(c.w.rstd2[i]);
  return fd;
}

}  // namespace

// ===============================================================================================================
// one encoder layer = the attention block + the feed-forward block (include/b4r.h)
extern "C" int32_t b4r_encoder_layer_supported(int32_t hidden_size, int32_t num_heads, int32_t inner_dim, int32_t L) {
  return (b4r_attn_block_supported(hidden_size, num_heads, L) && b4r_attn_block_bwd_supported(hidden_size, num_heads, L) &&
          b4r_ffn_block_supported(hidden_size, inner_dim)) ? 1 : 0;
}
extern "C" int64_t b4r_encoder_layer_bwd_scratch_floats(int32_t N) {
  return b4r_gemm_tn_scratch_floats(N, 64, 64) + b4r_gemm_tn_scratch_floats(N, 64, 192);
}
extern "C" int b4r_encoder_layer_fwd(const b4r_attn_block_desc* attn, const b4r_ffn_desc* ffn, b4r_stream_t stream) {
  B4R_CHECK_ARG(attn && ffn, B4R_E_BADARG, "b4r_encoder_layer_fwd: null descriptor");
  B4R_CHECK_ARG(((attn->x1 != nullptr && attn->x1 == ffn->x1) || (ffn->x1 == nullptr && attn->z1 != nullptr && attn->z1 == ffn->z1)) &&
                    (int64_t)attn->B * attn->L == ffn->N && attn->H == ffn->H,
                B4R_E_BADARG, "b4r_encoder_layer_fwd: the attention half's x1 (or, with x1 == NULL, its z1) [B*L,H] must be the "
                "feed-forward half's input");
  // (both halves behind each other in ONE launch were measured: 68 us against 39 + 25 us -- the feed-forward phase has to wait
  // for the attention half's stores at the barrier that frees the LDS, DESIGN.md section 4.1 -- and not kept)
  RC(b4r_attn_block_fwd(attn, stream));
  return b4r_ffn_block_fwd(ffn, stream);
}
extern "C" int b4r_encoder_layer_bwd(const b4r_ffn_desc* ffn, const b4r_attn_block_bwd_desc* attn, float* dWo, float* dbo, float* dWqkv,
                                     float* dbqkv, float* tn_scratch, b4r_stream_t stream) {
  B4R_CHECK_ARG(attn && ffn && dWo && dbo && dWqkv && dbqkv && tn_scratch, B4R_E_BADARG, "b4r_encoder_layer_bwd: null argument");
  B4R_CHECK_ARG(ffn->dz1 != nullptr && attn->dz1 == ffn->dz1 && (int64_t)attn->B * attn->L == ffn->N && attn->H == ffn->H, B4R_E_BADARG,
                "b4r_encoder_layer_bwd: the feed-forward half's dz1 [B*L,H] must be the attention half's input gradient");
  RC(b4r_ffn_block_bwd(ffn, stream));
  RC(b4r_attn_block_bwd(attn, stream));
  const b4r_gemm_tn_desc d_wo = wo_grad_desc(attn->ctx, attn->dz1, dWo, dbo, ffn->N, ffn->H, attn->out_rate > 0.f ? attn->rng : nullptr,
                                             attn->out_stream, attn->out_rate);
  if (attn->dWqkv != nullptr) {   // the attention block formed dWqkv / dbqkv itself (its descriptor's dWqkv: same buffers expected)
    B4R_CHECK_ARG(attn->dWqkv == dWqkv && attn->dbqkv == dbqkv && (attn->dWo == nullptr || (attn->dWo == dWo && attn->dbo == dbo)),
                  B4R_E_BADARG, "b4r_encoder_layer_bwd: the attention descriptor's dWqkv / dbqkv / dWo / dbo must be the call's");
    return attn->dWo != nullptr ? B4R_OK : gemm_tn_f32(d_wo, tn_scratch, stream);
  }
  // dWo and dWqkv = x^T . dqkv (+ their bias gradients): one launch
  return attn_wgrad_pair(d_wo, tn_scratch, attn->x, attn->dqkv, dWqkv, dbqkv, tn_scratch + b4r_gemm_tn_scratch_floats(ffn->N, ffn->H, ffn->H),
                         stream);
}

// ===============================================================================================================
// Every config-taking entry point has an _ex twin (include/b4r.h, b4r_model_config_ex); the classic one is a wrapper with
// embedding_width = 0, so both reach one code path.
extern "C" int64_t b4r_param_total_floats_ex(const b4r_model_config_ex* cfg) {
  ModelCfg c;
  if (resolve_cfg(cfg, &c)) return -1;
  return make_param_layout(c).total;
}
extern "C" int64_t b4r_param_total_floats(const b4r_model_config* cfg) { const auto x = classic_ex(cfg); return b4r_param_total_floats_ex(cfg ? &x : nullptr); }
extern "C" int64_t b4r_param_decay_floats_ex(const b4r_model_config_ex* cfg) {
  ModelCfg c;
  if (resolve_cfg(cfg, &c)) return -1;
  return make_param_layout(c).n_decay;
}
extern "C" int64_t b4r_param_decay_floats(const b4r_model_config* cfg) { const auto x = classic_ex(cfg); return b4r_param_decay_floats_ex(cfg ? &x : nullptr); }
extern "C" int32_t b4r_param_count_ex(const b4r_model_config_ex* cfg) {
  ModelCfg c;
  if (resolve_cfg(cfg, &c)) return -1;
  return (int32_t)make_param_layout(c).entries.size();
}
extern "C" int32_t b4r_param_count(const b4r_model_config* cfg) { const auto x = classic_ex(cfg); return b4r_param_count_ex(cfg ? &x : nullptr); }
extern "C" int b4r_param_info_ex(const b4r_model_config_ex* cfg, int32_t index, char* name, size_t name_cap, int64_t* offset,
                                 int32_t* rows, int32_t* cols, int32_t* ld, int32_t* decay) {
  ModelCfg c;
  RC(resolve_cfg(cfg, &c));
  const ParamLayout p = make_param_layout(c);
  B4R_CHECK_ARG(index >= 0 && index < (int)p.entries.size(), B4R_E_BADARG, "b4r_param_info: index %d out of range", index);
  const ParamEntry& e = p.entries[index];
  if (name && name_cap) snprintf(name, name_cap, "%s", e.name.c_str());
  if (offset) *offset = e.offset;
  if (rows) *rows = e.rows;
  if (cols) *cols = e.cols;
  if (ld) *ld = e.ld;
  if (decay) *decay = e.decay;
  return B4R_OK;
}
extern "C" int b4r_param_info(const b4r_model_config* cfg, int32_t index, char* name, size_t name_cap, int64_t* offset,
                              int32_t* rows, int32_t* cols, int32_t* ld, int32_t* decay) {
  const auto x = classic_ex(cfg);
  return b4r_param_info_ex(cfg ? &x : nullptr, index, name, name_cap, offset, rows, cols, ld, decay);
}
extern "C" int64_t b4r_pooler_floats(const b4r_model_config* cfg) {
  if (check_cfg(cfg)) return -1;
  return (int64_t)cfg->hidden_size * cfg->hidden_size + cfg->hidden_size;
}
extern "C" int64_t b4r_workspace_bytes_ex(const b4r_model_config_ex* cfg, int32_t B, int32_t L, int32_t P) {
  ModelCfg c;
  if (resolve_cfg(cfg, &c) || B <= 0 || L <= 0 || P < 0) return -1;
  return make_ws_layout(c, B, L, P).total * (int64_t)sizeof(float);
}
extern "C" int64_t b4r_workspace_bytes(const b4r_model_config* cfg, int32_t B, int32_t L, int32_t P) {
  const auto x = classic_ex(cfg);
  return b4r_workspace_bytes_ex(cfg ? &x : nullptr, B, L, P);
}
extern "C" int64_t b4r_workspace_bytes_encoder_ex(const b4r_model_config_ex* cfg, int32_t B, int32_t L, int32_t P) {
  ModelCfg c;
  if (resolve_cfg(cfg, &c) != B4R_OK || B <= 0 || L <= 0 || P < 0) return -1;
  return make_ws_layout(c, B, L, P).gath * (int64_t)sizeof(float);
}
extern "C" int64_t b4r_workspace_bytes_encoder(const b4r_model_config* cfg, int32_t B, int32_t L, int32_t P) {
  const auto x = classic_ex(cfg);
  return b4r_workspace_bytes_encoder_ex(cfg ? &x : nullptr, B, L, P);
}

extern "C" int b4r_workspace_region_ex(const b4r_model_config_ex* cfg, int32_t B, int32_t L, int32_t P, const char* name,
                                       int64_t* offset_floats, int32_t* rows, int32_t* cols, int32_t* ld) {
  ModelCfg mc;
  RC(resolve_cfg(cfg, &mc));
  B4R_CHECK_ARG(name && B > 0 && L > 0 && P >= 0, B4R_E_BADARG, "b4r_workspace_region: bad argument");
  const WsLayout w = make_ws_layout(mc, B, L, P);
  const int H = mc.hidden_size, nl = mc.num_layers;
  int64_t off = -1; int r = 0, c = 0, l = 0;
  const std::string n(name);
  if (n == "sequence_output") { off = w.x2[nl - 1]; r = (int)w.N; c = H; l = H; }
  else if (n == "embeddings") { off = w.x0; r = (int)w.N; c = H; l = H; }
  else if (n == "mlm_logits") { off = w.logits; r = (int)w.M; c = mc.vocab_size; l = (int)w.Vp; }
  else if (n == "mlm_hidden") { off = w.t; r = (int)w.M; c = mc.E; l = mc.E; }
  else if (n == "pooled_output") { off = w.pooled; r = B; c = H; l = H; }
  else if (n == "grad_sequence_output") { off = w.dx; r = (int)w.N; c = H; l = H; }
  else if (n.rfind("encoder_output_", 0) == 0) {
    const int i = atoi(n.c_str() + 15);
    B4R_CHECK_ARG(i >= 0 && i < nl, B4R_E_BADARG, "b4r_workspace_region: no layer %d", i);
    off = w.x2[i]; r = (int)w.N; c = H; l = H;
  } else if (n.rfind("attention_context_", 0) == 0) {
    const int i = atoi(n.c_str() + 18);
    B4R_CHECK_ARG(i >= 0 && i < nl, B4R_E_BADARG, "b4r_workspace_region: no layer %d", i);
    off = w.ctx[i]; r = (int)w.N; c = H; l = H;
  }
  B4R_CHECK_ARG(off >= 0, B4R_E_BADARG, "b4r_workspace_region: unknown region '%s'", name);
  if (offset_floats) *offset_floats = off;
  if (rows) *rows = r;
  if (cols) *cols = c;
  if (ld) *ld = l;
  return B4R_OK;
}
extern "C" int b4r_workspace_region(const b4r_model_config* cfg, int32_t B, int32_t L, int32_t P, const char* name,
                                    int64_t* offset_floats, int32_t* rows, int32_t* cols, int32_t* ld) {
  const auto x = classic_ex(cfg);
  return b4r_workspace_region_ex(cfg ? &x : nullptr, B, L, P, name, offset_floats, rows, cols, ld);
}

// ===============================================================================================================
// the logits-free head sweeps the item table: it answers on the table's width
static bool fused_head_ok(const ModelCfg& c) { return b4r_head32_hidden_ok(c.E) && b4r_split_mode(); }
extern "C" int32_t b4r_fused_head_supported_ex(const b4r_model_config_ex* cfg) {
  ModelCfg c;
  if (cfg == nullptr || resolve_cfg(cfg, &c) != B4R_OK) return 0;
  return fused_head_ok(c) ? 1 : 0;
}
extern "C" int32_t b4r_fused_head_supported(const b4r_model_config* cfg) {
  const auto x = classic_ex(cfg);
  return b4r_fused_head_supported_ex(cfg ? &x : nullptr);
}

// The public entry points take the documented flags only: the internal bits (B4R_FLAG_*_INTERNAL) couple a forward and a backward
// of ONE b4r_train_step call and are set there alone.  Each plans its own call; a train step plans once for both.
static int forward_impl(const ModelCfg* cfg, const b4r_batch* batch, const StepPlan& plan, const float* params,
                        const float* pooler, void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags,
                        b4r_stream_t stream);
static int backward_impl(const ModelCfg* cfg, const b4r_batch* batch, const StepPlan& plan, const float* params, float* grads,
                         void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags, b4r_stream_t stream,
                         int* norm_np);
constexpr int32_t B4R_PUBLIC_FLAGS = 0xFFFF;
extern "C" int b4r_forward_ex(const b4r_model_config_ex* cfg_ex, const b4r_batch* batch, const float* params, const float* pooler,
                              void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  RC(check_batch(batch, cfg, false));
  flags &= B4R_PUBLIC_FLAGS;
  return forward_impl(cfg, batch, plan_step(cfg, batch, flags), params, pooler, workspace, workspace_bytes, state, flags, stream);
}
extern "C" int b4r_forward(const b4r_model_config* cfg, const b4r_batch* batch, const float* params, const float* pooler,
                           void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags,
                           b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_forward_ex(cfg ? &x : nullptr, batch, params, pooler, workspace, workspace_bytes, state, flags, stream);
}
extern "C" int b4r_backward_ex(const b4r_model_config_ex* cfg_ex, const b4r_batch* batch, const float* params, float* grads,
                               void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  RC(check_batch(batch, cfg, true));
  flags &= B4R_PUBLIC_FLAGS;   // (no backward follows an encoder-only forward: that flag picks forward forms only)
  return backward_impl(cfg, batch, plan_step(cfg, batch, flags & ~B4R_FLAG_ENCODER_ONLY), params, grads, workspace, workspace_bytes,
                       state, flags, stream, nullptr);
}
extern "C" int b4r_backward(const b4r_model_config* cfg, const b4r_batch* batch, const float* params, float* grads,
                            void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags,
                            b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_backward_ex(cfg ? &x : nullptr, batch, params, grads, workspace, workspace_bytes, state, flags, stream);
}

// ===============================================================================================================
// the forms of the forward (the plan picks them; forward_impl runs them layer by layer)
namespace {

// AttnFwd::Block: the descriptor of the one-launch attention half (for the first layer with the embedding stage inside)
b4r_attn_block_desc attn_block_desc(const Step& c, int i, const float* x) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  b4r_attn_block_desc ad{};
  ad.B = c.B; ad.L = c.L; ad.H = c.H; ad.heads = c.cfg.num_heads; ad.x = x; ad.input_mask = c.batch.input_mask;
  ad.Wqkv = c.prm(pl.wqkv[i]); ad.bqkv = c.prm(pl.bqkv[i]); ad.Wo = c.prm(pl.wo[i]); ad.bo = c.prm(pl.bo[i]);
  ad.ln_gamma = c.prm(pl.ln1_g[i]); ad.ln_beta = c.prm(pl.ln1_b[i]); ad.ln_eps = c.cfg.ln_eps;
  ad.rng = (c.od > 0.f || c.adp > 0.f) ? c.rng : nullptr;
  ad.probs_stream = B4R_STREAM_ATTN_PROBS(i); ad.probs_rate = c.adp; ad.out_stream = B4R_STREAM_ATTN_OUT(i); ad.out_rate = c.od;
  ad.qkv = c.plan.qkv_stored ? c.at(w.qkv[i]) : nullptr;
  ad.ctx = c.at(w.ctx[i]); ad.lse = c.at(w.lse[i]); ad.keep_bits = c.keep(i);
  ad.z1 = c.at(w.z1[i]); ad.mean1 = c.at(w.mean1[i]); ad.rstd1 = c.at(w.rstd1[i]);
  ad.x1 = c.plan.x1_stored ? c.at(w.x1[i]) : nullptr;
  if (c.plan.slot_only_last && i == c.last) {   // nothing but the head's rows leave the last layer: only those queries are swept
    ad.out_slot_positions = c.batch.masked_lm_positions; ad.out_slots = c.batch.P;
  }
  if (i == 0 && c.plan.emb_fused) {
    ad.emb_ids = c.batch.input_word_ids; ad.emb_table = c.prm(pl.word_emb); ad.emb_pos = c.prm(pl.pos_emb); ad.emb_vocab = c.V;
    ad.emb_gamma = c.prm(pl.emb_ln_g); ad.emb_beta = c.prm(pl.emb_ln_b); ad.emb_eps = c.cfg.ln_eps;
    ad.emb_stream = B4R_STREAM_EMB; ad.emb_rate = c.od; if (c.od > 0.f) ad.rng = c.rng;
    ad.emb_x = c.at(c.w.x0); ad.emb_mean = c.at(c.w.mean0); ad.emb_rstd = c.at(c.w.rstd0);
  }
  return ad;
}

// the QKV product of the other two forms: qkv = x.Wqkv + bqkv, the queries times 1/sqrt(head width)
int qkv_fwd(const Step& c, int i, const float* x) {
  return gemm_f32({.A = x, .lda = c.H, .B = c.prm(c.pl.wqkv[i]), .ldb = 3 * c.H, .C = c.at(c.w.qkv[i]), .ldc = 3 * c.H, .M = c.N,
                   .N = 3 * c.H, .K = c.H, .epilogue = B4R_EPI_BIAS_QSCALE, .bias = c.prm(c.pl.bqkv[i]), .qscale = c.qscale,
                   .qcols = c.H, .c_pad_scratch = 1}, c.s);
}

// AttnFwd::SlotQuery: only the rows the head reads leave this layer: the attention core with the slots as its queries (keys: all
// tokens), then the output projection, dropout, residual and LayerNorm on the compact [M, H] rows.  ctx / lse / decision words:
// compact, at the start of the layer's dense regions; x1 / z1 / statistics: where the compact feed-forward half expects them
int attn_fwd_slotq(const Step& c, int i, const float* x) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int64_t* pos = c.batch.masked_lm_positions;
  const CompactRows cr = compact_rows(w, i, c.M, c.H, c.I);
  float* xc = c.at(w.x1[i]);   // the layer input's rows (the residual)
  float* yc = c.at(w.x1[i] + up4((int64_t)c.M * c.H));
  RC(qkv_fwd(c, i, x));
  RC(b4r_attn32_slotq_fwd_launch(c.at(w.qkv[i]), c.batch.input_mask, pos, c.B, c.L, c.cfg.num_heads, c.P, c.at(w.ctx[i]),
                                 c.at(w.lse[i]), b4r_make_drop(c.rng, B4R_STREAM_ATTN_PROBS(i), c.adp, 1), c.keep(i), c.s));
  RC(b4r_slot_rows_gather(x, nullptr, nullptr, nullptr, pos, c.L, c.P, c.M, c.H, xc, nullptr, nullptr, nullptr, c.s));
  RC(gemm_f32({.A = c.at(w.ctx[i]), .lda = c.H, .B = c.prm(pl.wo[i]), .ldb = c.H, .C = yc, .ldc = c.H, .M = c.M, .N = c.H, .K = c.H,
               .epilogue = B4R_EPI_BIAS, .bias = c.prm(pl.bo[i]), .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  return b4r_slot_rows_tail(yc, xc, pos, c.L, c.P, c.M, c.H, c.prm(pl.ln1_g[i]), c.prm(pl.ln1_b[i]), c.cfg.ln_eps,
                            b4r_make_drop(c.rng, B4R_STREAM_ATTN_OUT(i), c.od, 1), c.at(cr.z1c), c.at(cr.mean1c), c.at(cr.rstd1c),
                            nullptr, c.at(cr.x1c), c.s);
}

// AttnFwd::Core
int attn_fwd_core(const Step& c, int i, const float* x) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  RC(qkv_fwd(c, i, x));
  RC(b4r_attn_fwd_hd(c.at(w.qkv[i]), c.batch.input_mask, c.B, c.L, c.cfg.num_heads, head_dim(&c.cfg), c.at(w.ctx[i]), c.at(w.lse[i]),
                     c.rng, B4R_STREAM_ATTN_PROBS(i), c.adp, c.keep(i), c.s));
  return dense_res_ln(c.at(w.ctx[i]), c.H, c.prm(pl.wo[i]), c.at(w.z1[i]), c.at(w.x1[i]), c.at(w.mean1[i]), c.at(w.rstd1[i]), c.N, c.H,
                      c.H, c.prm(pl.bo[i]), x, c.prm(pl.ln1_g[i]), c.prm(pl.ln1_b[i]), c.cfg.ln_eps, c.rng, B4R_STREAM_ATTN_OUT(i), c.od,
                      c.s);
}

// FfnForm::Block (on the last layer of a head-rows step: only the rows the head reads, nothing else of this output is looked at)
int ffn_fwd_block(const Step& c, int i) {
  b4r_ffn_desc fd = ffn_fwd_desc(c, i);
  fd.x1 = c.plan.x1_stored ? c.at(c.w.x1[i]) : nullptr;
  fd.z1 = c.at(c.w.z1[i]); fd.mean1 = c.at(c.w.mean1[i]); fd.rstd1 = c.at(c.w.rstd1[i]);
  fd.ln1_gamma = c.prm(c.pl.ln1_g[i]); fd.ln1_beta = c.prm(c.pl.ln1_b[i]);
  if (c.plan.head_rows && i == c.last) {
    fd.slot_positions = c.batch.masked_lm_positions; fd.slot_ids = c.batch.masked_lm_ids; fd.slots_per_seq = c.batch.P;
    fd.seq_len = c.L; fd.max_rows = (int32_t)c.w.maxrows;
  }
  return b4r_ffn_block_fwd(&fd, c.s);
}

// FfnForm::CompactRows: gather x1 (and, for the backward, z1 and its statistics) -- unless the SlotQuery attention left them --, the two
// products on [M, .] operands, then dropout + residual + LayerNorm per compact row with the result scattered to its row of x2.  The
// compact f / fpre / z2 / mean2 / rstd2 lie at the start of the layer's dense regions (the backward of this form reads them there).
int ffn_fwd_compact(const Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int64_t* pos = c.batch.masked_lm_positions;
  const CompactRows cr = compact_rows(w, i, c.M, c.H, c.I);
  if (!c.plan.slotq_rows)
    RC(b4r_slot_rows_gather(c.at(w.x1[i]), c.at(w.z1[i]), c.at(w.mean1[i]), c.at(w.rstd1[i]), pos, c.L, c.P, c.M, c.H, c.at(cr.x1c),
                            c.at(cr.z1c), c.at(cr.mean1c), c.at(cr.rstd1c), c.s));
  RC(gemm_f32({.A = c.at(cr.x1c), .lda = c.H, .B = c.prm(pl.w1[i]), .ldb = c.I, .C = c.at(w.f[i]), .ldc = c.I, .M = c.M, .N = c.I,
               .K = c.H, .epilogue = B4R_EPI_BIAS_GELU, .bias = c.prm(pl.b1[i]), .C2 = c.at(w.fpre[i]), .ldc2 = c.I, .qscale = 1.f,
               .c_pad_scratch = 1, .activation = c.cfg.act_inner}, c.s));
  RC(gemm_f32({.A = c.at(w.f[i]), .lda = c.I, .B = c.prm(pl.w2[i]), .ldb = c.H, .C = c.at(cr.yc), .ldc = c.H, .M = c.M, .N = c.H,
               .K = c.I, .epilogue = B4R_EPI_BIAS, .bias = c.prm(pl.b2[i]), .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  return b4r_slot_rows_tail(c.at(cr.yc), c.at(cr.x1c), pos, c.L, c.P, c.M, c.H, c.prm(pl.ln2_g[i]), c.prm(pl.ln2_b[i]), c.cfg.ln_eps,
                            b4r_make_drop(c.rng, B4R_STREAM_FFN_OUT(i), c.od, 1), c.at(w.z2[i]), c.at(w.mean2[i]), c.at(w.rstd2[i]),
                            c.at(w.x2[i]), nullptr, c.s);
}

// FfnForm::Wide.  After an encoder-only forward no backward follows: [N, inner] stays on the chip; otherwise the launch also writes f
// and the pre-activation, where the backward of this step expects them
int ffn_fwd_wide(const Step& c, int i) {
  const bool keep = !(c.flags & B4R_FLAG_ENCODER_ONLY);
  b4r_ffn_desc fd = ffn_fwd_desc(c, i);
  fd.x1 = c.at(c.w.x1[i]);
  return b4r_ffn32w_fwd(&fd, c.at(c.w.ffnrec[i]), keep ? c.at(c.w.f[i]) : nullptr, keep ? c.at(c.w.fpre[i]) : nullptr, c.s);
}

// FfnForm::TileProducts
int ffn_fwd_tiles(const Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  RC(gemm_f32({.A = c.at(w.x1[i]), .lda = c.H, .B = c.prm(pl.w1[i]), .ldb = c.I, .C = c.at(w.f[i]), .ldc = c.I, .M = c.N, .N = c.I,
               .K = c.H, .epilogue = B4R_EPI_BIAS_GELU, .bias = c.prm(pl.b1[i]), .C2 = c.at(w.fpre[i]), .ldc2 = c.I, .qscale = 1.f,
               .c_pad_scratch = 1, .activation = c.cfg.act_inner}, c.s));
  return dense_res_ln(c.at(w.f[i]), c.I, c.prm(pl.w2[i]), c.at(w.z2[i]), c.at(w.x2[i]), c.at(w.mean2[i]), c.at(w.rstd2[i]), c.N, c.H,
                      c.I, c.prm(pl.b2[i]), c.at(w.x1[i]), c.prm(pl.ln2_g[i]), c.prm(pl.ln2_b[i]), c.cfg.ln_eps, c.rng,
                      B4R_STREAM_FFN_OUT(i), c.od, c.s);
}

// tfm MaskedLM: gather -> dense(gelu) -> LayerNorm -> . E^T + bias (the fused head: no [M,V] tensor, loss rows, log-sum-exp and
// d loss_sum / d T straight from T, E and the bias)
int head_fwd(const Step& c, const float* x) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  RC(transform_fwd({.A = x, .lda = c.H, .B = c.prm(pl.wd), .ldb = c.E, .C = c.at(w.u), .ldc = c.E, .M = c.M, .N = c.E, .K = c.H,
                    .epilogue = B4R_EPI_BIAS_GELU_LN, .bias = c.prm(pl.bd), .C2 = c.at(w.t), .ldc2 = c.E, .qscale = 1.f,
                    .c_pad_scratch = 1, .ln_gamma = c.prm(pl.lnm_g), .ln_beta = c.prm(pl.lnm_b), .ln_mean = c.at(w.meanm),
                    .ln_rstd = c.at(w.rstdm), .ln_eps = c.cfg.ln_eps, .C3 = c.at(w.upre), .ldc3 = c.E,
                    .a_gather_idx = c.batch.masked_lm_positions, .a_gather_add_per = c.L, .a_gather_per = c.P,
                    .a_copy = c.at(w.gath) /* the transform's weight-gradient operand */, .a_copy_ld = c.H,
                    .activation = c.cfg.act_mlm}, c.at(w.gath), c.s));
  if (c.plan.fused_head)
    return b4r_head32_fwd_launch(c.at(w.t), c.prm(pl.word_emb), c.prm(pl.out_bias), c.batch.masked_lm_ids, c.M, c.V, c.E,
                                 c.at(w.scratch), c.at(w.dt), c.at(w.rowsc), c.at(w.head_lse), reinterpret_cast<int32_t*>(c.at(w.head_ylab)),
                                 c.plan.defer_combine ? 1 : 0, c.s);
  return gemm_f32({.A = c.at(w.t), .lda = c.E, .B = c.prm(pl.word_emb), .ldb = c.E, .C = c.at(w.logits), .ldc = (int)w.Vp, .M = c.M,
                   .N = c.V, .K = c.E, .b_is_nk = 1, .epilogue = B4R_EPI_BIAS, .bias = c.prm(pl.out_bias), .qscale = 1.f,
                   .c_pad_scratch = 1}, c.s);
}

}  // namespace

static int forward_impl(const ModelCfg* cfg, const b4r_batch* batch, const StepPlan& plan, const float* params,
                        const float* pooler, void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags,
                        b4r_stream_t stream) {
  B4R_CHECK_ARG(params && workspace, B4R_E_BADARG, "b4r_forward: null params/workspace");
  B4R_CHECK_ARG(b4r_aligned16(params) && b4r_aligned16(workspace), B4R_E_ALIGN, "b4r_forward: buffers must be 16-byte aligned");
  const Step c(cfg, batch, plan, params, nullptr, workspace, state, flags, stream);
  // an encoder-only forward without the pooler touches nothing behind the encoder's own regions (the masked-LM head's buffers -- the
  // [B*P, V] logits above all -- and the whole backward area): b4r_workspace_bytes_encoder is enough for it
  const int64_t ws_need = ((flags & B4R_FLAG_ENCODER_ONLY) && !(flags & B4R_FLAG_POOLER)) ? c.w.gath : c.w.total;
  B4R_CHECK_ARG(workspace_bytes >= ws_need * (int64_t)sizeof(float), B4R_E_NOMEM, "b4r_forward: workspace too small (%lld < %lld)",
                (long long)workspace_bytes, (long long)(ws_need * sizeof(float)));
  B4R_CHECK_ARG(!(flags & B4R_FLAG_TRAINING) || state || (cfg->output_dropout == 0.f && cfg->attention_dropout == 0.f), B4R_E_BADARG,
                "b4r_forward: training with dropout needs a state (rng)");
  const bool head = c.P > 0 && !(flags & B4R_FLAG_ENCODER_ONLY);
  B4R_CHECK_ARG(!head || !plan.fused_head || fused_head_ok(*cfg), B4R_E_BADARG,
                "b4r_forward: B4R_FLAG_FUSED_HEAD needs an item-table width (hidden size or embedding_width) of 64 / 128 / 256 and the "
                "bf16x3 mode");
  B4R_CHECK_ARG(!head || !plan.fused_head || batch->masked_lm_ids != nullptr, B4R_E_BADARG,
                "b4r_forward: B4R_FLAG_FUSED_HEAD needs masked_lm_ids");

  // the embedding stage: inside the first layer's attention block where that runs fused, else a launch of its own
  if (plan.emb_proj)
    RC(b4r_embed_proj_fwd_launch(batch->input_word_ids, c.B, c.L, c.prm(c.pl.word_emb), c.V, c.prm(c.pl.pos_emb), c.prm(c.pl.emb_ln_g),
                                 c.prm(c.pl.emb_ln_b), c.E, cfg->ln_eps, c.prm(c.pl.proj_w), c.prm(c.pl.proj_b), c.H, c.at(c.w.x0),
                                 c.at(c.w.mean0), c.at(c.w.rstd0), b4r_make_drop(c.rng, B4R_STREAM_EMB, c.od, 1), c.s));
  else if (!plan.emb_fused)
    RC(b4r_embed_ln_fwd(batch->input_word_ids, c.B, c.L, c.prm(c.pl.word_emb), c.V, c.prm(c.pl.pos_emb), c.prm(c.pl.emb_ln_g),
                        c.prm(c.pl.emb_ln_b), c.H, cfg->ln_eps, c.at(c.w.x0), c.at(c.w.mean0), c.at(c.w.rstd0), c.rng, c.od, c.s));
  const float* x = c.at(c.w.x0);
  for (int i = 0; i <= c.last; ++i) {
    switch (plan.attn_fwd[i]) {
      case AttnFwd::Block: { const b4r_attn_block_desc ad = attn_block_desc(c, i, x); RC(b4r_attn_block_fwd(&ad, c.s)); break; }
      case AttnFwd::SlotQuery: RC(attn_fwd_slotq(c, i, x)); break;
      case AttnFwd::Core: RC(attn_fwd_core(c, i, x)); break;
    }
    switch (plan.ffn[i]) {
      case FfnForm::Block: RC(ffn_fwd_block(c, i)); break;
      case FfnForm::CompactRows: RC(ffn_fwd_compact(c, i)); break;
      case FfnForm::Wide: RC(ffn_fwd_wide(c, i)); break;
      case FfnForm::TileProducts: RC(ffn_fwd_tiles(c, i)); break;
    }
    x = c.at(c.w.x2[i]);
  }
  if ((flags & B4R_FLAG_POOLER) && pooler)   // tanh(x[:,0,:] . Wp + bp): rows b of A are L*H apart
    RC(gemm_f32({.A = x, .lda = c.L * c.H, .B = pooler, .ldb = c.H, .C = c.at(c.w.pooled), .ldc = c.H, .M = c.B, .N = c.H, .K = c.H,
                 .epilogue = B4R_EPI_BIAS_TANH, .bias = pooler + (int64_t)c.H * c.H, .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  return head ? head_fwd(c, x) : B4R_OK;
}

extern "C" int b4r_mlm_transform_rows_ex(const b4r_model_config_ex* cfg_ex, const float* params, const float* seq, int64_t n_seq_rows,
                                         const int64_t* rows, int32_t R, float* out, float* scratch, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  B4R_CHECK_ARG(params && seq && rows && out && scratch && R > 0 && n_seq_rows > 0, B4R_E_BADARG, "b4r_mlm_transform_rows: bad argument");
  B4R_CHECK_ARG(b4r_aligned16(params) && b4r_aligned16(seq) && b4r_aligned16(out) && b4r_aligned16(scratch), B4R_E_ALIGN,
                "b4r_mlm_transform_rows: buffers must be 16-byte aligned");
  const ParamLayout pl = make_param_layout(*cfg);
  const int H = cfg->hidden_size, E = cfg->E;
  float* gath = scratch; float* upre = gath + up4((int64_t)R * H); float* u = upre + up4((int64_t)R * H);
  float* mean = u + up4((int64_t)R * H); float* rstd = mean + up4(R);
  return transform_fwd({.A = seq, .lda = H, .B = params + pl.wd, .ldb = E, .C = u, .ldc = E, .M = R, .N = E, .K = H,
                        .epilogue = B4R_EPI_BIAS_GELU_LN, .bias = params + pl.bd, .C2 = out, .ldc2 = E, .qscale = 1.f,
                        .c_pad_scratch = 0, .ln_gamma = params + pl.lnm_g, .ln_beta = params + pl.lnm_b, .ln_mean = mean,
                        .ln_rstd = rstd, .ln_eps = cfg->ln_eps, .C3 = upre, .ldc3 = E,
                        .a_gather_idx = rows, .a_gather_add_per = n_seq_rows, .a_gather_per = R /* one group: row m reads seq[rows[m]] */,
                        .activation = cfg->act_mlm},
                       gath, stream);
}
extern "C" int b4r_mlm_transform_rows(const b4r_model_config* cfg, const float* params, const float* seq, int64_t n_seq_rows,
                                      const int64_t* rows, int32_t R, float* out, float* scratch, b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_mlm_transform_rows_ex(cfg ? &x : nullptr, params, seq, n_seq_rows, rows, R, out, scratch, stream);
}

extern "C" int b4r_loss_ex(const b4r_model_config_ex* cfg_ex, const b4r_batch* batch, void* workspace, int64_t workspace_bytes,
                           b4r_train_state* state, int32_t want_grad, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  RC(check_batch(batch, cfg, true));
  B4R_CHECK_ARG(batch->masked_lm_ids && workspace && state, B4R_E_BADARG, "b4r_loss: needs masked_lm_ids, workspace, state");
  const WsLayout w = make_ws_layout(*cfg, batch->B, batch->L, batch->P);
  B4R_CHECK_ARG(workspace_bytes >= w.total * (int64_t)sizeof(float), B4R_E_NOMEM, "b4r_loss: workspace too small");
  float* ws = static_cast<float*>(workspace);
  if (want_grad & B4R_LOSS_FUSED_HEAD)   // the forward (B4R_FLAG_FUSED_HEAD) already produced the loss rows and dT
    return b4r_ce_finalize_launch(ws + w.rowsc, (int)w.M, state, (want_grad & B4R_LOSS_OVERWRITE) ? 1 : 0, (hipStream_t)stream);
  return b4r_softmax_ce(ws + w.logits, (int)w.M, cfg->vocab_size, (int)w.Vp, batch->masked_lm_ids, ws + w.rowsc, state,
                        want_grad & (1 | B4R_LOSS_OVERWRITE), stream);
}

extern "C" int b4r_loss(const b4r_model_config* cfg, const b4r_batch* batch, void* workspace, int64_t workspace_bytes,
                        b4r_train_state* state, int32_t want_grad, b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_loss_ex(cfg ? &x : nullptr, batch, workspace, workspace_bytes, state, want_grad, stream);
}

// ===============================================================================================================
// the forms of the backward
namespace {

// the opening launch (it clears the gradient buffer, dx and the scatter's hot-row slots -- in the row-list mode the hot-row slots and
// db, whose rows outside the list carry no gradient --, with B4R_FLAG_GRAD_TAIL also the step's sums behind the gradients) and the
// masked-LM head down to d sequence_output
int head_bwd(Step& c) {
  const StepPlan& p = c.plan;
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, E = c.E, M = c.M, V = c.V, Vp = (int)w.Vp;   // (the head's rows and the item table are E wide)
  const bool loss_sums = (c.flags & B4R_FLAG_LOSS_SUMS) != 0;
  // the scratch regions of the fused head are fixed here already: the records dE sweeps (the transform rows as fp16 images, -lse,
  // labels) are formed by extra workgroups of the clearing launch (b4r_zero2's rider) instead of a launch of their own.  With the
  // deferred merge the forward's partials stay where it left them, at the start of the scratch.
  float *fwd_part = nullptr, *dE_scratch = nullptr;
  if (p.fused_head && p.defer_combine) RC(c.take(b4r_head32_fwd_scratch_floats(M, V, E), &fwd_part));
  if (p.fused_head) RC(c.take(b4r_head32_dE_scratch_floats(M, V, E), &dE_scratch));
  alignas(8) char rider[128];
  int rider_blocks = 0;
  if (p.fused_head)
    RC(b4r_head32_dE_pack_job(c.at(w.t), c.at(w.head_lse), reinterpret_cast<const int32_t*>(c.at(w.head_ylab)), M, V, E, dE_scratch,
                              fwd_part, c.batch.masked_lm_ids, rider, sizeof(rider), &rider_blocks));
  // row-list mode with the slots' dz1 only in the last layer's attention backward (it never reads the other rows): db is not cleared
  RC(b4r_zero2(c.grads, pl.total, c.at(p.rows() ? w.hot : w.dx),
               p.rows() ? (p.slot_only_last ? w.db - w.hot : w.da - w.hot) : w.db - w.dx, c.s,
               ((c.flags & B4R_FLAG_GRAD_TAIL) && !p.defer_combine) ? c.grd(pl.total) : nullptr, c.state,
               (loss_sums && !p.defer_combine) ? c.at(w.rowsc) : nullptr, M, rider_blocks > 0 ? rider : nullptr, rider_blocks));

  float* dlog = c.at(w.logits);   // (the materialising head: d loss_sum / d logits, pad columns zero)
  float* sc;
  if (p.fused_head) {
    // dT came with the forward -- or (defer_combine) the forward left its per-slice partials: dE forms the lse it needs from them, the
    // transform's LayerNorm backward below merges them into dT as it reads it; dE / d output_bias recompute the logit tiles (b4r_head32.hip)
    RC(b4r_head32_dE_launch(c.at(w.t), c.prm(pl.word_emb), c.prm(pl.out_bias), c.at(w.head_lse),
                            reinterpret_cast<const int32_t*>(c.at(w.head_ylab)), M, V, E, dE_scratch, c.grd(pl.word_emb),
                            c.grd(pl.out_bias), c.s, fwd_part, c.batch.masked_lm_ids, rider_blocks > 0 ? 1 : 0));
  } else {
    // dT = dlogits . E   (K = V is long and the output small: split K so that the whole chip streams dlogits).  The loss kernel zeroed
    // columns [V, Vp) of dlogits, and the table is followed by the position table in the flat parameter buffer, so the reduction may
    // run over whole chunks of 64 (rows V..Vp-1 of "E" meet zeros)
    const b4r_gemm_desc d{.A = dlog, .lda = Vp, .B = c.prm(pl.word_emb), .ldb = E, .C = c.at(w.dt), .ldc = E, .M = M, .N = E, .K = V,
                          .b_is_nk = 0, .epilogue = B4R_EPI_NONE};
    const int splits = mlm_dt_splits(M, E, V);
    RC(c.take((int64_t)splits * M * E, &sc));
    RC(b4r_gemm_f32_splitk(&d, splits, sc, (pl.word_emb + (int64_t)Vp * E <= pl.total) ? 1 : 0, c.s));
    // dE = dlogits^T . T ; d output_bias = column sums of dlogits
    RC(c.take(b4r_gemm_tn_scratch_floats(M, V, E), &sc));
    RC(gemm_tn_f32({.A = dlog, .lda = Vp, .B = c.at(w.t), .ldb = E, .out = c.grd(pl.word_emb), .ldo = E, .R = M, .Mo = V, .No = E,
                    .colsum_a = c.grd(pl.out_bias)}, sc, c.s));
  }
  // LayerNorm of the transform (with the deferred merge: dT, the loss rows, lse and labels are formed here, from the forward's partials)
  // ... and straight through the GELU of the transform's dense layer
  const B4rHeadMerge merge{fwd_part, fwd_part ? b4r_head32_fwd_slices(M, V, E) : 0, M, V, c.at(w.t), c.prm(pl.word_emb),
                           c.prm(pl.out_bias), c.batch.masked_lm_ids, c.at(w.rowsc), c.at(w.head_lse),
                           reinterpret_cast<int32_t*>(c.at(w.head_ylab))};
  RC(c.take(b4r_ln_bwd_scratch_floats(M, E), &sc));
  RC(b4r_ln_bwd_launch(c.at(w.dt), c.at(w.u), c.at(w.meanm), c.at(w.rstdm), c.prm(pl.lnm_g), M, E, c.at(w.dt), c.grd(pl.lnm_g),
                       c.grd(pl.lnm_b), sc, nullptr, nullptr, nullptr, 1, 1, b4r_make_drop(nullptr, 0, 0.f, 0), c.s, c.at(w.upre),
                       fwd_part ? &merge : nullptr, c.cfg.act_mlm));
  // dense layer of the transform: dWd = gath^T . du (+ bias gradient) and dgath = du . Wd^T, one pass over du where the pair kernel
  // applies (hidden size 64), else the two products
  b4r_gemm_tn_desc d{.A = c.at(w.gath), .lda = H, .B = c.at(w.dt), .ldb = E, .out = c.grd(pl.wd), .ldo = E, .R = M, .Mo = H, .No = E,
                     .colsum = c.grd(pl.bd), .dgrad_w = c.prm(pl.wd), .dgrad_ldw = E, .dgrad_out = c.at(w.dg), .dgrad_ldo = H};
  RC(c.take(b4r_gemm_tn_scratch_floats(M, H, E), &sc));
  if (b4r_gemm_tn_dgrad_supported(&d)) {
    RC(gemm_tn_f32(d, sc, c.s));
  } else {
    d.dgrad_w = nullptr; d.dgrad_ldw = 0; d.dgrad_out = nullptr; d.dgrad_ldo = 0;
    RC(gemm_tn_f32(d, sc, c.s));
    RC(gemm_f32({.A = c.at(w.dt), .lda = E, .B = c.prm(pl.wd), .ldb = E, .C = c.at(w.dg), .ldc = H, .M = M, .N = H, .K = E,
                 .b_is_nk = 1, .epilogue = B4R_EPI_NONE, .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  }
  // scatter into d sequence_output (slots with y_true == 0 carry exactly zero gradient and are skipped); in the row-list mode the last
  // layer's feed-forward backward reads the slot gradients directly
  if (p.rows()) return B4R_OK;
  return b4r_scatter_add_rows_impl(c.at(w.dg), c.batch.masked_lm_positions, c.L, c.P, M, H, c.at(w.dx), H, c.batch.masked_lm_ids, c.N,
                                   0, nullptr, c.s);
}

// a weight gradient `d` with the input gradient of the same layer from one pass over its B operand where b4r_gemm_tn_dgrad_supported,
// else the input-gradient product `dx` (the same dropout on its A operand) followed by the weight gradient alone
int wgrad_with_dgrad(Step& c, b4r_gemm_tn_desc d, const b4r_gemm_desc& dx) {
  float* sc; RC(c.take(b4r_gemm_tn_scratch_floats(d.R, d.Mo, d.No), &sc));
  if (b4r_gemm_tn_dgrad_supported(&d)) return gemm_tn_f32(d, sc, c.s);
  RC(gemm_f32(dx, c.s));
  d.dgrad_w = nullptr; d.dgrad_ldw = 0; d.dgrad_out = nullptr; d.dgrad_ldo = 0; d.dgrad_gelu_pre = nullptr; d.dgrad_ldg = 0;
  return gemm_tn_f32(d, sc, c.s);
}

// FfnForm::Block: dz1 (-> db), dW1 / db1 / dW2 / db2 and the attention LayerNorm's gamma / beta gradients from dz2 (da); the
// [N, inner] pre-activation is recomputed from x1 inside the two kernels.  On the last layer of the row-list mode the output
// LayerNorm's backward runs inside, on the rows with a gradient; dz1 elsewhere stays zero.
int ffn_bwd_block(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  b4r_ffn_desc fd = ffn_desc(c, i);
  fd.x1 = c.plan.x1_stored ? c.at(w.x1[i]) : nullptr;   // as the forward of this step left it
  fd.dz2 = c.at(w.da); fd.z1 = c.at(w.z1[i]); fd.mean1 = c.at(w.mean1[i]); fd.rstd1 = c.at(w.rstd1[i]);
  fd.ln1_gamma = c.prm(pl.ln1_g[i]); fd.ln1_beta = c.prm(pl.ln1_b[i]); fd.dz1 = c.at(w.db);
  fd.dW1 = c.grd(pl.w1[i]); fd.db1 = c.grd(pl.b1[i]); fd.dW2 = c.grd(pl.w2[i]); fd.db2 = c.grd(pl.b2[i]);
  fd.dln1_gamma = c.grd(pl.ln1_g[i]);
  RC(c.take(b4r_ffn_block_bwd_scratch_floats(c.N), &fd.scratch));
  if (c.plan.head_rows && i == c.last) {
    fd.dz2 = nullptr;
    fd.slot_positions = c.batch.masked_lm_positions; fd.slot_ids = c.batch.masked_lm_ids; fd.slots_per_seq = c.batch.P; fd.seq_len = c.L;
    fd.max_rows = (int32_t)w.maxrows;
    fd.slot_grad = c.at(w.dg); fd.z2 = c.at(w.z2[i]); fd.mean2 = c.at(w.mean2[i]); fd.rstd2 = c.at(w.rstd2[i]);
    fd.ln_gamma = c.prm(pl.ln2_g[i]); fd.dln_gamma = c.grd(pl.ln2_g[i]); fd.dz2_rows = c.at(w.dz2c);
  }
  return b4r_ffn_block_bwd(&fd, c.s);
}

// FfnForm::CompactRows: the tile-product chain with every operand [M, .], one row per masked-LM slot (slots without a label carry an
// exactly zero gradient; two labelled slots never share a row).  dz1 (db) was cleared by the opening launch; the compact result is
// scatter-added into it (and left in dz2c for the SlotQuery attention backward).
int ffn_bwd_compact(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, I = c.I, M = c.M;
  const int64_t* pos = c.batch.masked_lm_positions;
  const CompactRows cr = compact_rows(w, i, M, H, I);
  float* dz2c = c.at(w.dzc_a);                      // LayerNorm2 backward of the slot gradients
  float* dz2d = c.od > 0.f ? c.at(w.dzc_b) : dz2c;   // ... through the output dropout
  float* sc; RC(c.take(ln_scratch_floats(c.N, H), &sc));
  RC(b4r_ln_bwd_launch(c.at(w.dg), c.at(w.z2[i]), c.at(w.mean2[i]), c.at(w.rstd2[i]), c.prm(pl.ln2_g[i]), M, H, dz2c, c.grd(pl.ln2_g[i]),
                       c.grd(pl.ln2_b[i]), sc, nullptr, nullptr, nullptr, 1, 1, b4r_make_drop(nullptr, 0, 0.f, 0), c.s));
  if (c.od > 0.f)
    RC(b4r_slot_rows_drop(dz2c, pos, c.L, c.P, M, H, b4r_make_drop(c.rng, B4R_STREAM_FFN_OUT(i), c.od, 1), dz2d, c.s));
  RC(gemm_f32({.A = dz2d, .lda = H, .B = c.prm(pl.w2[i]), .ldb = H, .C = c.at(w.df), .ldc = I, .M = M, .N = I, .K = H, .b_is_nk = 1,
               .epilogue = B4R_EPI_GELU_BWD, .R = c.at(w.fpre[i]), .ldr = I, .qscale = 1.f, .c_pad_scratch = 1,
               .activation = c.cfg.act_inner}, c.s));
  RC(c.take(b4r_gemm_tn_scratch_floats(M, I, H), &sc));
  RC(gemm_tn_f32({.A = c.at(w.f[i]), .lda = I, .B = dz2d, .ldb = H, .out = c.grd(pl.w2[i]), .ldo = H, .R = M, .Mo = I, .No = H,
                  .colsum = c.grd(pl.b2[i])}, sc, c.s));
  RC(c.take(ln_scratch_floats(c.N, H), &sc));
  RC(dgrad_ln_bwd(c.at(w.df), I, c.prm(pl.w1[i]), I, dz2c, c.at(w.dz2c), M, H, c.at(cr.z1c), c.at(cr.mean1c), c.at(cr.rstd1c),
                  c.prm(pl.ln1_g[i]), c.grd(pl.ln1_g[i]), c.grd(pl.ln1_b[i]), sc, c.s));
  RC(c.take(b4r_gemm_tn_scratch_floats(M, H, I), &sc));
  RC(gemm_tn_f32({.A = c.at(cr.x1c), .lda = H, .B = c.at(w.df), .ldb = I, .out = c.grd(pl.w1[i]), .ldo = I, .R = M, .Mo = H, .No = I,
                  .colsum = c.grd(pl.b1[i])}, sc, c.s));
  return b4r_scatter_add_rows_impl(c.at(w.dz2c), pos, c.L, c.P, M, H, c.at(w.db), H, c.batch.masked_lm_ids, c.N, 0, nullptr, c.s);
}

// FfnForm::Wide: dF and dX1 (residual included) in one launch from the records the forward packed; LayerNorm1's backward in place;
// the two weight gradients as products
int ffn_bwd_wide(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, I = c.I, N = c.N;
  b4r_ffn_desc fd = ffn_desc(c, i);
  fd.dz2 = c.at(w.da);
  RC(b4r_ffn32w_bwd(&fd, c.at(w.ffnrec[i]), c.at(w.fpre[i]), c.at(w.df), c.at(w.db), true, c.s));
  float* sc; RC(c.take(b4r_gemm_tn_scratch_floats(N, I, H), &sc));
  RC(gemm_tn_f32({.A = c.at(w.f[i]), .lda = I, .B = c.at(w.da), .ldb = H, .out = c.grd(pl.w2[i]), .ldo = H, .R = N, .Mo = I, .No = H,
                  .colsum = c.grd(pl.b2[i]), .rng = c.rng, .drop_stream = B4R_STREAM_FFN_OUT(i), .drop_rate = c.od, .b_dropout = 1},
                 sc, c.s));
  RC(c.take(ln_scratch_floats(N, H), &sc));
  RC(b4r_ln_bwd_launch(c.at(w.db), c.at(w.z1[i]), c.at(w.mean1[i]), c.at(w.rstd1[i]), c.prm(pl.ln1_g[i]), N, H, c.at(w.db),
                       c.grd(pl.ln1_g[i]), c.grd(pl.ln1_b[i]), sc, nullptr, nullptr, nullptr, 1, 1, b4r_make_drop(nullptr, 0, 0.f, 0), c.s));
  RC(c.take(b4r_gemm_tn_scratch_floats(N, H, I), &sc));
  return gemm_tn_f32({.A = c.at(w.x1[i]), .lda = H, .B = c.at(w.df), .ldb = I, .out = c.grd(pl.w1[i]), .ldo = I, .R = N, .Mo = H,
                      .No = I, .colsum = c.grd(pl.b1[i])}, sc, c.s);
}

// FfnForm::TileProducts: dFpre = (dropmask(dz2) . W2^T) * gelu'(fpre) with dW2 = f^T . dropmask(dz2) (+ bias gradient); then
// dz1 = the attention LayerNorm's backward of dX1 = dFpre . W1^T + dz2, and dW1
int ffn_bwd_tiles(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, I = c.I, N = c.N;
  RC(wgrad_with_dgrad(c, {.A = c.at(w.f[i]), .lda = I, .B = c.at(w.da), .ldb = H, .out = c.grd(pl.w2[i]), .ldo = H, .R = N, .Mo = I,
                          .No = H, .colsum = c.grd(pl.b2[i]), .rng = c.rng, .drop_stream = B4R_STREAM_FFN_OUT(i), .drop_rate = c.od,
                          .b_dropout = 1, .dgrad_w = c.prm(pl.w2[i]), .dgrad_ldw = H, .dgrad_out = c.at(w.df), .dgrad_ldo = I,
                          .dgrad_gelu_pre = c.at(w.fpre[i]), .dgrad_ldg = I, .activation = c.cfg.act_inner},
                      {.A = c.at(w.da), .lda = H, .B = c.prm(pl.w2[i]), .ldb = H, .C = c.at(w.df), .ldc = I, .M = N, .N = I, .K = H,
                       .b_is_nk = 1, .epilogue = B4R_EPI_GELU_BWD, .R = c.at(w.fpre[i]), .ldr = I, .qscale = 1.f, .rng = c.rng,
                       .drop_stream = B4R_STREAM_FFN_OUT(i), .drop_rate = c.od, .a_dropout = 1, .c_pad_scratch = 1,
                       .activation = c.cfg.act_inner}));
  float* sc; RC(c.take(ln_scratch_floats(N, H), &sc));
  RC(dgrad_ln_bwd(c.at(w.df), I, c.prm(pl.w1[i]), I, c.at(w.da), c.at(w.db), N, H, c.at(w.z1[i]), c.at(w.mean1[i]), c.at(w.rstd1[i]),
                  c.prm(pl.ln1_g[i]), c.grd(pl.ln1_g[i]), c.grd(pl.ln1_b[i]), sc, c.s));
  RC(c.take(b4r_gemm_tn_scratch_floats(N, H, I), &sc));
  return gemm_tn_f32({.A = c.at(w.x1[i]), .lda = H, .B = c.at(w.df), .ldb = I, .out = c.grd(pl.w1[i]), .ldo = I, .R = N, .Mo = H,
                      .No = I, .colsum = c.grd(pl.b1[i])}, sc, c.s);
}

// AttnBwd::Block / BlockFolded: the attention block's backward in one launch -- dqkv and, through the LayerNorm in front of this layer,
// da (for layer 0: through the embedding stage's dropout and LayerNorm).  Folded, the launch also forms every weight gradient of the
// half; else dWo (inputs ready since the feed-forward backward) and dWqkv follow as one launch.
int attn_bwd_block(Step& c, int i, const float* x_in) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const bool folded = c.plan.attn_bwd[i] == AttnBwd::BlockFolded;
  float* wo_scratch = nullptr;   // dWo's slabs for the pair launch after the block
  RC(c.take(b4r_gemm_tn_scratch_floats(c.N, c.H, c.H), &wo_scratch));
  b4r_attn_block_bwd_desc bd{};
  bd.B = c.B; bd.L = c.L; bd.H = c.H; bd.heads = c.cfg.num_heads;
  bd.x = x_in; bd.dz1 = c.at(w.db); bd.ctx = c.at(w.ctx[i]); bd.lse = c.at(w.lse[i]);
  bd.keep_bits = c.keep(i); bd.input_mask = c.batch.input_mask;
  bd.Wqkv = c.prm(pl.wqkv[i]); bd.bqkv = c.prm(pl.bqkv[i]); bd.Wo = c.prm(pl.wo[i]);
  bd.rng = (c.od > 0.f || c.adp > 0.f) ? c.rng : nullptr;
  bd.probs_stream = B4R_STREAM_ATTN_PROBS(i); bd.probs_rate = c.adp; bd.out_stream = B4R_STREAM_ATTN_OUT(i); bd.out_rate = c.od;
  if (i > 0) {
    bd.prev_z = c.at(w.z2[i - 1]); bd.prev_mean = c.at(w.mean2[i - 1]); bd.prev_rstd = c.at(w.rstd2[i - 1]);
    bd.prev_gamma = c.prm(pl.ln2_g[i - 1]); bd.dprev_gamma = c.grd(pl.ln2_g[i - 1]);
  } else {
    bd.prev_mean = c.at(w.mean0); bd.prev_rstd = c.at(w.rstd0); bd.prev_gamma = c.prm(pl.emb_ln_g); bd.dprev_gamma = c.grd(pl.emb_ln_g);
    bd.emb_ids = c.batch.input_word_ids; bd.emb_table = c.prm(pl.word_emb); bd.emb_pos = c.prm(pl.pos_emb); bd.emb_vocab = c.V;
    bd.emb_stream = B4R_STREAM_EMB; bd.emb_rate = c.od;
  }
  bd.dqkv = c.at(w.dqkv); bd.dx_prev = c.at(w.da);
  RC(c.take(b4r_attn_block_bwd_scratch_floats(c.B), &bd.scratch));
  if (folded) {   // dWqkv / dbqkv inside the launch: no [N, 3H] round trip, no weight-gradient launch for them, nor for dWo / dbo
    bd.dqkv = nullptr; bd.dWqkv = c.grd(pl.wqkv[i]); bd.dbqkv = c.grd(pl.bqkv[i]);
    RC(c.take(b4r_attn_block_bwd_dw_scratch_floats(c.B), &bd.dw_scratch));
    bd.dWo = c.grd(pl.wo[i]); bd.dbo = c.grd(pl.bo[i]);
  }
  if (c.plan.slot_only_last && i == c.last) {
    bd.dz1_slot_positions = c.batch.masked_lm_positions; bd.dz1_slot_ids = c.batch.masked_lm_ids; bd.dz1_slots = c.batch.P;
  }
  RC(b4r_attn_block_bwd(&bd, c.s));
  if (folded) return B4R_OK;
  float* sc; RC(c.take(b4r_gemm_tn_scratch_floats(c.N, c.H, 3 * c.H), &sc));
  return attn_wgrad_pair(wo_grad_desc(c.at(w.ctx[i]), c.at(w.db), c.grd(pl.wo[i]), c.grd(pl.bo[i]), c.N, c.H, c.rng, B4R_STREAM_ATTN_OUT(i),
                                      c.od), wo_scratch, x_in, c.at(w.dqkv), c.grd(pl.wqkv[i]), c.grd(pl.bqkv[i]), sc, c.s);
}

// AttnBwd::SlotQuery: dz1 of the slots (left in dz2c by the compact feed-forward half) -> dropout of the output projection -> dWo / dbo
// and dctx on [M, H] rows -> the attention core's backward with the slots as its queries (dq rows of the labelled slots, dk / dv of
// every token)
int attn_bwd_slotq(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, M = c.M;
  const int64_t* pos = c.batch.masked_lm_positions;
  float* dz1d = c.od > 0.f ? c.at(w.dctx + up4((int64_t)M * H)) : c.at(w.dz2c);   // (the dense dctx region is free in this form)
  float* dctx_c = c.at(w.dctx);
  if (c.od > 0.f)
    RC(b4r_slot_rows_drop(c.at(w.dz2c), pos, c.L, c.P, M, H, b4r_make_drop(c.rng, B4R_STREAM_ATTN_OUT(i), c.od, 1), dz1d, c.s));
  float* sc; RC(c.take(b4r_gemm_tn_scratch_floats(c.N, H, H), &sc));
  RC(gemm_tn_f32({.A = c.at(w.ctx[i]), .lda = H, .B = dz1d, .ldb = H, .out = c.grd(pl.wo[i]), .ldo = H, .R = M, .Mo = H, .No = H,
                  .colsum = c.grd(pl.bo[i])}, sc, c.s));
  RC(gemm_f32({.A = dz1d, .lda = H, .B = c.prm(pl.wo[i]), .ldb = H, .C = dctx_c, .ldc = H, .M = M, .N = H, .K = H, .b_is_nk = 1,
               .epilogue = B4R_EPI_NONE, .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  return b4r_attn32_slotq_bwd_launch(c.at(w.qkv[i]), c.batch.input_mask, pos, c.batch.masked_lm_ids, c.at(w.ctx[i]), c.at(w.lse[i]),
                                     dctx_c, c.B, c.L, c.cfg.num_heads, c.P, c.qscale, c.at(w.dqkv),
                                     b4r_make_drop(c.rng, B4R_STREAM_ATTN_PROBS(i), c.adp, 1), c.keep(i), c.s);
}

// AttnBwd::Core: dctx = dropmask(dz1) . Wo^T with dWo = ctx^T . dropmask(dz1) (+ bias gradient), then the attention core: dQ, dK, dV
int attn_bwd_core(Step& c, int i) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H;
  b4r_gemm_tn_desc d = wo_grad_desc(c.at(w.ctx[i]), c.at(w.db), c.grd(pl.wo[i]), c.grd(pl.bo[i]), c.N, H, c.rng, B4R_STREAM_ATTN_OUT(i),
                                    c.od);
  d.dgrad_w = c.prm(pl.wo[i]); d.dgrad_ldw = H; d.dgrad_out = c.at(w.dctx); d.dgrad_ldo = H;
  RC(wgrad_with_dgrad(c, d, {.A = c.at(w.db), .lda = H, .B = c.prm(pl.wo[i]), .ldb = H, .C = c.at(w.dctx), .ldc = H, .M = c.N, .N = H,
                             .K = H, .b_is_nk = 1, .epilogue = B4R_EPI_NONE, .qscale = 1.f, .rng = c.rng,
                             .drop_stream = B4R_STREAM_ATTN_OUT(i), .drop_rate = c.od, .a_dropout = 1, .c_pad_scratch = 1}));
  return b4r_attn_bwd_hd(c.at(w.qkv[i]), c.batch.input_mask, c.at(w.ctx[i]), c.at(w.lse[i]), c.at(w.dctx), c.B, c.L, c.cfg.num_heads,
                         head_dim(&c.cfg), c.qscale, c.at(w.dqkv), c.rng, B4R_STREAM_ATTN_PROBS(i), c.adp, c.keep(i), c.s);
}

// the QKV projection behind SlotQuery / Core: dX_in = dqkv . Wqkv^T + dz1 and straight on through the LayerNorm in front of this
// layer (-> da): layer i-1's output LayerNorm, or for layer 0 the embedding stage (dropout -> LayerNorm of item row + position row);
// then dWqkv = x_in^T . dqkv (+ bias gradient)
int qkv_bwd(Step& c, int i, const float* x_in) {
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  const int H = c.H, N = c.N;
  float* sc; RC(c.take(ln_scratch_floats(N, H), &sc));
  if (i > 0)
    RC(dgrad_ln_bwd(c.at(w.dqkv), 3 * H, c.prm(pl.wqkv[i]), 3 * H, c.at(w.db), c.at(w.da), N, H, c.at(w.z2[i - 1]), c.at(w.mean2[i - 1]),
                    c.at(w.rstd2[i - 1]), c.prm(pl.ln2_g[i - 1]), c.grd(pl.ln2_g[i - 1]), c.grd(pl.ln2_b[i - 1]), sc, c.s));
  else if (c.plan.emb_proj)   // factorised: plain dx0 = dqkv . Wqkv^T + dz1; embed_proj_bwd takes it from there
    RC(gemm_f32({.A = c.at(w.dqkv), .lda = 3 * H, .B = c.prm(pl.wqkv[i]), .ldb = 3 * H, .C = c.at(w.da), .ldc = H, .M = N, .N = H,
                 .K = 3 * H, .b_is_nk = 1, .epilogue = B4R_EPI_ADD_RES, .R = c.at(w.db), .ldr = H, .qscale = 1.f, .c_pad_scratch = 1}, c.s));
  else
    RC(dgrad_ln_bwd(c.at(w.dqkv), 3 * H, c.prm(pl.wqkv[i]), 3 * H, c.at(w.db), c.at(w.da), N, H, nullptr, c.at(w.mean0), c.at(w.rstd0),
                    c.prm(pl.emb_ln_g), c.grd(pl.emb_ln_g), c.grd(pl.emb_ln_b), sc, c.s, c.batch.input_word_ids, c.prm(pl.word_emb),
                    c.prm(pl.pos_emb), c.L, c.V, c.rng, B4R_STREAM_EMB, c.od));
  RC(c.take(b4r_gemm_tn_scratch_floats(N, H, 3 * H), &sc));
  return gemm_tn_f32({.A = x_in, .lda = H, .B = c.at(w.dqkv), .ldb = 3 * H, .out = c.grd(pl.wqkv[i]), .ldo = 3 * H, .R = N, .Mo = H,
                      .No = 3 * H, .colsum = c.grd(pl.bqkv[i])}, sc, c.s);
}

}  // namespace

// *norm_np (b4r_train_step, B4R_FLAG_NORM_PARTIALS_INTERNAL): > 0 where the closing reduce launch also left that many partial sums of
// squares of the gradients at the start of the workspace (dead by then), so that the optimizer needs no norm launch
static int backward_impl(const ModelCfg* cfg, const b4r_batch* batch, const StepPlan& plan, const float* params, float* grads,
                         void* workspace, int64_t workspace_bytes, b4r_train_state* state, int32_t flags, b4r_stream_t stream,
                         int* norm_np) {
  B4R_CHECK_ARG(params && grads && workspace && batch->masked_lm_ids, B4R_E_BADARG, "b4r_backward: null argument");
  B4R_CHECK_ARG(b4r_aligned16(params) && b4r_aligned16(grads) && b4r_aligned16(workspace), B4R_E_ALIGN,
                "b4r_backward: buffers must be 16-byte aligned");
  Step c(cfg, batch, plan, params, grads, workspace, state, flags, stream);
  B4R_CHECK_ARG(workspace_bytes >= c.w.total * (int64_t)sizeof(float), B4R_E_NOMEM, "b4r_backward: workspace too small");
  B4R_CHECK_ARG(!(flags & B4R_FLAG_GRAD_TAIL) || state, B4R_E_BADARG, "b4r_backward: B4R_FLAG_GRAD_TAIL needs the state");
  B4R_CHECK_ARG(!(flags & B4R_FLAG_LOSS_SUMS) || ((flags & B4R_FLAG_FUSED_HEAD) && state && batch->masked_lm_ids), B4R_E_BADARG,
                "b4r_backward: B4R_FLAG_LOSS_SUMS needs B4R_FLAG_FUSED_HEAD, the state and masked_lm_ids");
  B4R_CHECK_ARG(!plan.fused_head || fused_head_ok(*cfg), B4R_E_BADARG,
                "b4r_backward: B4R_FLAG_FUSED_HEAD needs an item-table width (hidden size or embedding_width) of 64 / 128 / 256 and the "
                "bf16x3 mode");
  // (the attention block forms only run at hidden size 64, where no embedding width below it is supported)
  B4R_CHECK_ARG(!plan.emb_proj || (plan.attn_bwd[0] != AttnBwd::Block && plan.attn_bwd[0] != AttnBwd::BlockFolded), B4R_E_SHAPE,
                "b4r_backward: the factorised embedding needs layer 0's attention backward as products");
  const ParamLayout& pl = c.pl; const WsLayout& w = c.w;
  B4rReduceQueue queue;
  b4r_reduce_queue_begin(&queue);   // every ordered reduction below is summed by ONE launch at the end
  RC(head_bwd(c));
  // ---- encoder layers, last to first ---------------------------------------------------------------------------------
  for (int i = c.last; i >= 0; --i) {
    const float* x_in = (i == 0) ? c.at(w.x0) : c.at(w.x2[i - 1]);
    // output LayerNorm (for every layer but the last its backward rode on the QKV input-gradient product of layer i + 1)
    if (i == c.last && !plan.rows()) {
      float* sc; RC(c.take(ln_scratch_floats(c.N, c.H), &sc));
      RC(b4r_ln_bwd_launch(c.at(w.dx), c.at(w.z2[i]), c.at(w.mean2[i]), c.at(w.rstd2[i]), c.prm(pl.ln2_g[i]), c.N, c.H, c.at(w.da),
                           c.grd(pl.ln2_g[i]), c.grd(pl.ln2_b[i]), sc, nullptr, nullptr, nullptr, 1, 1, b4r_make_drop(nullptr, 0, 0.f, 0),
                           c.s));
    }
    switch (plan.ffn[i]) {
      case FfnForm::Block: RC(ffn_bwd_block(c, i)); break;
      case FfnForm::CompactRows: RC(ffn_bwd_compact(c, i)); break;
      case FfnForm::Wide: RC(ffn_bwd_wide(c, i)); break;
      case FfnForm::TileProducts: RC(ffn_bwd_tiles(c, i)); break;
    }
    switch (plan.attn_bwd[i]) {
      case AttnBwd::Block: case AttnBwd::BlockFolded: RC(attn_bwd_block(c, i, x_in)); break;
      case AttnBwd::SlotQuery: RC(attn_bwd_slotq(c, i)); RC(qkv_bwd(c, i, x_in)); break;
      case AttnBwd::Core: RC(attn_bwd_core(c, i)); RC(qkv_bwd(c, i, x_in)); break;
    }
  }
  // ---- embedding stage: its dropout -> LayerNorm backward ran with layer 0's QKV product (da = d(item row + position row));
  // what remains: word table scatter-add, position table batch sum.  Factorised: da is dx0 [N, H]; the projection's backward forms
  // dWp / dbp, the dropout and LayerNorm backward at width E and the rows d(item row + position row) [N, E] (into dctx, free by now)
  const float* emb_rows = c.at(w.da);
  if (plan.emb_proj) {
    float* psc; RC(c.take(b4r_embed_proj_bwd_scratch_floats_impl(c.N, c.E, c.H), &psc));
    RC(b4r_embed_proj_bwd_launch(c.at(w.da), batch->input_word_ids, c.B, c.L, c.prm(pl.word_emb), c.V, c.prm(pl.pos_emb), c.prm(pl.emb_ln_g),
                                 c.prm(pl.emb_ln_b), c.E, c.at(w.mean0), c.at(w.rstd0), c.prm(pl.proj_w), c.H,
                                 b4r_make_drop(c.rng, B4R_STREAM_EMB, c.od, 1), c.at(w.dctx), c.grd(pl.proj_w), c.grd(pl.proj_b),
                                 c.grd(pl.emb_ln_g), psc, c.s));
    emb_rows = c.at(w.dctx);
  }
  // the item-table scatter sums in 64-bit fixed point beside the float gradient (bitwise reproducible; b4r_rowops.hip), so it
  // need not wait for the head's part of that gradient: ONE launch then sums every queued ordered reduction (weight / bias /
  // LayerNorm gradients, the position table) and adds the fixed-point sums to the item table
  float* sc; RC(c.take((int64_t)b4r_cdiv(c.B, 16) * c.L * c.E, &sc));
  RC(b4r_embed_grads(emb_rows, batch->input_word_ids, c.B, c.L, c.E, c.grd(pl.word_emb), c.V, 3, c.at(w.hot) /* zeroed at the top */,
                     c.grd(pl.pos_emb), sc, c.s, plan.defer_combine ? c.at(w.rowsc) : nullptr, (int)w.M, state,
                     (plan.defer_combine && (flags & B4R_FLAG_GRAD_TAIL)) ? c.grd(pl.total) : nullptr));
  if (norm_np) *norm_np = 0;
  if (!(flags & B4R_FLAG_NORM_PARTIALS_INTERNAL)) return b4r_reduce_queue_flush(c.s);
  // valid only when the jobs of this launch write EVERY gradient (then each value is squared exactly once, as it is stored)
  // every trainable entry of the layout, rows x cols -- the position table's first L rows only (its other rows carry no gradient)
  int64_t expected = 0;
  for (const ParamEntry& e : pl.entries)
    expected += (int64_t)(e.offset == pl.pos_emb ? c.L : e.rows) * e.cols;
  int np = 0;
  int64_t covered = 0;
  RC(b4r_reduce_queue_flush(c.s, c.ws, 4096, &np, &covered));
  if (norm_np && np > 0 && covered == expected) *norm_np = np;
  return B4R_OK;
}

extern "C" int b4r_optimizer_step_ex(const b4r_model_config_ex* cfg_ex, const b4r_adamw_config* hp, float* params, const float* grads,
                                     float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                                     b4r_train_state* state, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  B4R_CHECK_ARG(hp && params && grads && adam_m && adam_v && workspace && state, B4R_E_BADARG, "b4r_optimizer_step: null argument");
  B4R_CHECK_ARG(workspace_bytes >= 4096 * (int64_t)sizeof(float), B4R_E_NOMEM, "b4r_optimizer_step: workspace too small");
  const ParamLayout pl = make_param_layout(*cfg);
  // the scratch region sits at the END of the workspace; any 4096-float area works, use the start of the buffer the
  // backward no longer needs: the first floats of the workspace hold x0 which is dead after backward.
  float* scratch = static_cast<float*>(workspace);
  return b4r_optimizer_fused(hp, params, grads, adam_m, adam_v, pl.total, pl.n_decay, scratch, state, (hipStream_t)stream);
}

extern "C" int b4r_optimizer_step(const b4r_model_config* cfg, const b4r_adamw_config* hp, float* params, const float* grads,
                                  float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                                  b4r_train_state* state, b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_optimizer_step_ex(cfg ? &x : nullptr, hp, params, grads, adam_m, adam_v, workspace, workspace_bytes, state, stream);
}

extern "C" int b4r_optimizer_step_reduced_ex(const b4r_model_config_ex* cfg_ex, const b4r_adamw_config* hp, float* params,
                                             const float* grads, float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                                             b4r_train_state* state, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  B4R_CHECK_ARG(hp && params && grads && adam_m && adam_v && workspace && state, B4R_E_BADARG, "b4r_optimizer_step_reduced: null argument");
  B4R_CHECK_ARG(workspace_bytes >= 4096 * (int64_t)sizeof(float), B4R_E_NOMEM, "b4r_optimizer_step_reduced: workspace too small");
  const ParamLayout pl = make_param_layout(*cfg);
  return b4r_optimizer_fused(hp, params, grads, adam_m, adam_v, pl.total, pl.n_decay, static_cast<float*>(workspace), state,
                             (hipStream_t)stream, 1);
}

extern "C" int b4r_optimizer_step_reduced(const b4r_model_config* cfg, const b4r_adamw_config* hp, float* params, const float* grads,
                                          float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                                          b4r_train_state* state, b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_optimizer_step_reduced_ex(cfg ? &x : nullptr, hp, params, grads, adam_m, adam_v, workspace, workspace_bytes, state, stream);
}

extern "C" int b4r_train_step_ex(const b4r_model_config_ex* cfg_ex, const b4r_adamw_config* hp, const b4r_batch* batch, float* params,
                                 float* grads, float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                                 b4r_train_state* state, b4r_stream_t stream) {
  ModelCfg mc;
  RC(resolve_cfg(cfg_ex, &mc));
  const ModelCfg* cfg = &mc;
  RC(check_batch(batch, cfg, true));
  const int fused = fused_head_ok(*cfg) ? 1 : 0;   // the train step never needs the logits themselves
  const int defer = (fused && b4r_head32_combine_foldable(batch->B * batch->P, cfg->vocab_size, cfg->E))
                        ? B4R_FLAG_DEFER_COMBINE_INTERNAL : 0;
  // no b4r_state_begin_step launch: the loss reduction overwrites the sums (B4R_LOSS_OVERWRITE)
  // nothing but the loss, the metrics and the gradients leave a train step: the last layer's feed-forward half runs on the rows the
  // head gathers only (B4R_FLAG_HEAD_ROWS_ONLY)
  const int32_t fwd_flags = B4R_FLAG_TRAINING | B4R_FLAG_HEAD_ROWS_ONLY | (fused ? B4R_FLAG_FUSED_HEAD : 0) | defer;
  // with the logits-free head the loss sums are formed inside the backward's first launch (B4R_FLAG_LOSS_SUMS), else by b4r_loss
  const int32_t bwd_flags = fwd_flags | (fused ? B4R_FLAG_LOSS_SUMS : 0) | B4R_FLAG_NORM_PARTIALS_INTERNAL;
  const StepPlan plan = plan_step(cfg, batch, bwd_flags);   // (the backward's flags: the forward's and what it alone reads)
  RC(forward_impl(cfg, batch, plan, params, nullptr, workspace, workspace_bytes, state, fwd_flags, stream));
  if (!fused) RC(b4r_loss_ex(cfg_ex, batch, workspace, workspace_bytes, state, 1 | B4R_LOSS_OVERWRITE, stream));
  int np = 0;   // > 0: the backward's last launch left the norm's partial sums at the start of the workspace
  RC(backward_impl(cfg, batch, plan, params, grads, workspace, workspace_bytes, state, bwd_flags, stream, &np));
  if (np > 0) {
    B4R_CHECK_ARG(hp && adam_m && adam_v, B4R_E_BADARG, "b4r_train_step: null argument");
    const ParamLayout pl = make_param_layout(*cfg);
    return b4r_optimizer_fused(hp, params, grads, adam_m, adam_v, pl.total, pl.n_decay, static_cast<float*>(workspace), state,
                               (hipStream_t)stream, 0, np);
  }
  return b4r_optimizer_step_ex(cfg_ex, hp, params, grads, adam_m, adam_v, workspace, workspace_bytes, state, stream);
}
extern "C" int b4r_train_step(const b4r_model_config* cfg, const b4r_adamw_config* hp, const b4r_batch* batch, float* params,
                              float* grads, float* adam_m, float* adam_v, void* workspace, int64_t workspace_bytes,
                              b4r_train_state* state, b4r_stream_t stream) {
  const auto x = classic_ex(cfg);
  return b4r_train_step_ex(cfg ? &x : nullptr, hp, batch, params, grads, adam_m, adam_v, workspace, workspace_bytes, state, stream);
}
