// Full-catalogue top-K and rank of a held-out item, without an [R, V] score matrix.
//
// Serves  batched recommendation   (top K unseen items for many users: Recommender.recommend_batch, BERT4RecModel.recommend)
//         full-ranking evaluation  (rank of the held-out item among every item the user has not interacted with, the protocol of
//                                   the BERT4Rec replication studies instead of bert4rec_evaluator.py:60-120's 100 sampled negatives)
//
// Contract (include/b4r.h, b4r_rank_full): scores are the b4r_rank_candidates scores bit for bit (k-ascending fp32 fma chain +
// bias, oracle/rank_oracle.c::rank_oracle_scores); the top K is the stable descending order over the allowed ids (ties: lower id
// first); gt_rank = 1 + #{allowed j: s_j > s_gt} + #{allowed j < gt: s_j == s_gt}.
//
// Three launches per group of rows that fits the scratch:
//   1. gt key     one thread per row: s_gt by the same chain, as the order-preserving integer image ("key") of the score.
//   2. sweep      grid (group of 16 rows) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h.  Each 256-thread workgroup stages
//                 its chunk's table rows through LDS in k-blocks of 16 floats (16-byte loads), once for all 16 rows, and forms 16 x 1024 scores
//                 with the fma chain on the VALU (the hidden rows are LDS broadcasts; 2 ids per thread per k-block halve those).
//                 Scores stay in registers (4 ids x 16 rows per thread).  Excluded ids come from a per-row LDS bitmap built from
//                 exclude[r].  Per row it counts, in integers, the allowed ids that beat gt, and selects the chunk's best
//                 min(K, 1024) by a radix select on the unique 48-bit key (score key << 16 | 1023 - local id): the passes start
//                 below the bits every allowed key of the row shares, and stop as soon as the digit found holds exactly what is
//                 still missing.  The selected (score, id) pairs go to scratch in any order.
//   3. merge      one workgroup per row: the same radix select on (score key << 32 | ~id) over all chunks' candidates, then the
//                 order of the K survivors by counting, descending key; gt_rank = 1 + the sum of the chunks' counts.
// No floating-point atomics; LDS integer atomics only place or count, and the outputs do not depend on their order.
//
// b4r_rank_full_ex adds a catalogue filter (packed allow bits per filter, one filter per row: the sweep's per-row LDS bitmap starts
// from the complement of the row's 32 filter words of the chunk instead of zeros), an item scale (one fp32 multiply after the
// chain) and bias = NULL.  The sweep is a template on (filter, scale, bias); <false, false, true> is b4r_rank_full's kernel.
// b4r_item_neighbours ranks the item table against its own rows with the same sweep: item_rnorm_kernel (cosine only) and
// item_query_kernel stage 1 / |row| and the query rows in scratch first.
#include <algorithm>

#include "b4r_common.h"
#include "b4r_internal.h"
#include "b4r_catalogue_tile.h"
#include "b4r_cosine_chain.h"

namespace {

// ---- 1. score key of the held-out item ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void full_gt_key_kernel(const float* __restrict__ hidden, int hidden_ld,
                                                          const int64_t* __restrict__ hidden_row, const float* __restrict__ table,
                                                          const float* __restrict__ bias, const float* __restrict__ scale, int H,
                                                          int V, int lo, const int64_t* __restrict__ gt, int64_t r0, int n,
                                                          uint32_t* __restrict__ gkey) {
  const int lr = blockIdx.x * 64 + threadIdx.x;
  if (lr >= n) return;
  const int64_t r = r0 + lr;
  const int64_t g = gt[r];
  if (g < lo || g >= V) { gkey[lr] = 0u; return; }
  const int64_t hr = hidden_row ? hidden_row[r] : r;
  gkey[lr] = score_key(row_score(hidden + hr * hidden_ld, table + g * H, bias, scale, g, H));
}

// ---- 2. sweep: (group of TILE_G rows) x (chunk of TILE_CH ids) -----------------------------------------------------------------
struct SweepArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias;
  const int64_t* exclude; const int64_t* gt;
  const uint32_t* gkey;
  float* c_score; int32_t* c_id; int32_t* c_cnt; int32_t* c_beat;   // [n][nch][cap], [n][nch]
  int64_t r0;
  int hidden_ld, H, V, lo, E, n, nch, cap;
};

// what only the FILT / SCALE instances read: a kernel argument of its own, so that the unfiltered instance's argument block, and
// with it its scalar registers and its code, stay as they were before the filter
struct SweepExtra {
  const float* scale;                                                // [V] (SCALE instances)
  const uint32_t* allow; const int32_t* row_filter; int n_filters;   // [n_filters][ceil(V / 32)], [R] or NULL (FILT instances)
};

// FILT: the row bitmap starts from the row's filter words; SCALE: score = fl32((chain + bias) * scale[j]); BIAS = false: bias is +0.0f
template <bool FILT, bool SCALE, bool BIAS>
__global__ __launch_bounds__(TILE_T, 2) void full_sweep_kernel(SweepArgs a, SweepExtra x) {
  __shared__ float tile[TILE_IPT * TILE_T * (TILE_KB + 1)];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[TILE_G][TILE_CH / 32];
  __shared__ uint32_t hist[TILE_G][256];
  __shared__ uint32_t part[TILE_G][16];
  __shared__ Sel st[TILE_G];
  __shared__ uint32_t s_cnt[TILE_G], s_beat[TILE_G], s_kmin[TILE_G], s_kmax[TILE_G], s_out[TILE_G];
  __shared__ int s_alldone;
  __shared__ int64_t s_hoff[TILE_G], s_gt[TILE_G];

  const int tid = threadIdx.x, lane = tid & 63;
  const int lr0 = blockIdx.x * TILE_G;
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const int H = a.H;

  if (tid < TILE_G) {
    tile_row_setup(tid, lr0, a.n, a.r0, a.hidden_row, a.hidden_ld, a.gt, s_hoff, s_gt);
    s_cnt[tid] = 0; s_beat[tid] = 0; s_out[tid] = 0;
    s_kmin[tid] = 0xFFFFFFFFu; s_kmax[tid] = 0u;
  }
  tile_row_bitmap(bits, FILT, x.allow, x.row_filter, x.n_filters, a.exclude, a.E, s_hoff, a.r0, lr0, a.n, a.V, c0);

  // ---- scores: raw fp32 bits in registers, NOT_ALLOWED where the id is not ranked -----------------------------------------------
  uint32_t raw[TILE_Q][TILE_G];
#pragma unroll
  for (int ps = 0; ps < TILE_Q / TILE_IPT; ++ps) {
    // (the k-block loop is written out in each of the four sweeps: stated once as a function it changed their registers)
    float acc[TILE_IPT][TILE_G];
#pragma unroll
    for (int ii = 0; ii < TILE_IPT; ++ii)
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) acc[ii][g] = 0.f;
    const int64_t cj0 = c0 + (int64_t)ps * TILE_IPT * TILE_T;   // first id of this step
    for (int kb = 0; kb < H; kb += TILE_KB) {
      const int kn = min(TILE_KB, H - kb);   // a multiple of 4 (H % 4 == 0)
      const int k4 = kn >> 2;
      __syncthreads();   // the previous block is consumed (and, the first time, the bitmap is complete)
      for (int f = tid; f < TILE_IPT * TILE_T * k4; f += TILE_T) {
        const int i = f / k4, c4 = f - i * k4;
        const int64_t j = cj0 + i;
        const f32x4 v = j < a.V ? *reinterpret_cast<const f32x4*>(a.table + j * H + kb + 4 * c4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        float* dst = tile + i * (TILE_KB + 1) + 4 * c4;
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
      }
      {
        const int g = tid / TILE_KB, k = tid - g * TILE_KB;   // TILE_G * TILE_KB == TILE_T
        hsh[tid] = (k < kn && s_hoff[g] >= 0) ? a.hidden[s_hoff[g] + kb + k] : 0.f;
      }
      __syncthreads();
      for (int k = 0; k < kn; k += 4) {
        float e[TILE_IPT][4];
#pragma unroll
        for (int ii = 0; ii < TILE_IPT; ++ii)
#pragma unroll
          for (int u = 0; u < 4; ++u) e[ii][u] = tile[(ii * TILE_T + tid) * (TILE_KB + 1) + k + u];
#pragma unroll
        for (int g = 0; g < TILE_G; ++g) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(hsh + g * TILE_KB + k);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int ii = 0; ii < TILE_IPT; ++ii) acc[ii][g] = __builtin_fmaf(h[u], e[ii][u], acc[ii][g]);
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < TILE_IPT; ++ii) {
      const int q = ps * TILE_IPT + ii;
      const int l = q * TILE_T + tid;
      const int64_t j = c0 + l;
      const bool inb = j >= a.lo && j < a.V;
      const float b = BIAS ? (inb ? a.bias[j] : 0.f) : 0.f;
      const float sc = SCALE ? (inb ? x.scale[j] : 1.f) : 1.f;
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) {
        const bool ex = (bits[g][l >> 5] >> (l & 31)) & 1u;
        const bool ok = inb && s_hoff[g] >= 0 && (!ex || j == s_gt[g]);
        // (the unfiltered instance keeps the statement it had: a sum formed outside the select compiles to other code)
        if constexpr (SCALE) raw[q][g] = ok ? __builtin_bit_cast(uint32_t, (acc[ii][g] + b) * sc) : NOT_ALLOWED;
        else raw[q][g] = ok ? __builtin_bit_cast(uint32_t, acc[ii][g] + b) : NOT_ALLOWED;
      }
    }
  }

  // ---- per row: allowed count, ids that beat gt, key range ------------------------------------------------------------------
  // (this loop and the select after it are written out in the three sweeps that select: stated once as a function they changed the
  // sweeps' registers and this kernel measured 0.5-1.1 % slower)
#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    const bool gv = a.gt && s_gt[g] >= a.lo && s_gt[g] < a.V && s_hoff[g] >= 0;
    const uint32_t gk = gv ? a.gkey[lr0 + g] : 0u;
    const int64_t gid = s_gt[g];
    uint32_t cnt = 0, beat = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (raw[q][g] == NOT_ALLOWED) continue;
      const uint32_t k = score_key_bits(raw[q][g]);
      const int64_t j = c0 + q * TILE_T + tid;
      cnt += 1;
      beat += (gv && (k > gk || (k == gk && j < gid))) ? 1u : 0u;
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    cnt = wave_sum_u32(cnt); beat = wave_sum_u32(beat);
    kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
    if (lane == 0) {
      atomicAdd(&s_cnt[g], cnt); atomicAdd(&s_beat[g], beat);
      atomicMin(&s_kmin[g], kmin); atomicMax(&s_kmax[g], kmax);
    }
  }
  __syncthreads();
  if (tid < TILE_G && lr0 + tid < a.n) {
    const int64_t o = (int64_t)(lr0 + tid) * a.nch + chunk;
    a.c_beat[o] = (int32_t)s_beat[tid];
    const int n = (int)s_cnt[tid];
    sel_init(st[tid], n, min(a.cap, n), s_kmin[tid], s_kmax[tid]);
  } else if (tid < TILE_G) {
    sel_init(st[tid], 0, 0, 0u, 0u);
  }
  if (tid == 0) s_alldone = 0;

  // ---- radix select over (score key << 16 | TILE_CH-1 - local id) --------------------------------------------------------------
  for (int pass = 0; pass < 6; ++pass) {
    __syncthreads();
    if (tid == 0) {
      int all = 1;
      for (int g = 0; g < TILE_G; ++g) all &= st[g].done;
      s_alldone = all;
    }
    for (int i = tid; i < TILE_G * 256; i += TILE_T) (&hist[0][0])[i] = 0u;
    __syncthreads();
    if (s_alldone) break;
#pragma unroll
    for (int g = 0; g < TILE_G; ++g) {
      const Sel s = st[g];
      if (s.done) continue;
      const int nb = sel_nb(s, 48), sh = 48 - s.hi - nb;
#pragma unroll
      for (int q = 0; q < TILE_Q; ++q) {
        if (raw[q][g] == NOT_ALLOWED) continue;
        const uint64_t key = ((uint64_t)score_key_bits(raw[q][g]) << 16) | (uint64_t)(TILE_CH - 1 - (q * TILE_T + tid));
        if (sel_match(s, key, 48)) atomicAdd(&hist[g][(key >> sh) & ((1u << nb) - 1u)], 1u);
      }
    }
    __syncthreads();
    const int g = tid >> 4, qq = tid & 15;
    const Sel mine = st[g];
    if (!mine.done) sel_part(hist[g], part[g], qq);
    __syncthreads();
    if (!mine.done) sel_advance(mine, st[g], hist[g], part[g], qq, 48);
  }
  __syncthreads();

  // ---- emit the selected ids of each row (any order: the merge orders them) ------------------------------------------------
#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    const Sel s = st[g];
    if (!s.take || !s.done) continue;
    const int64_t base = ((int64_t)(lr0 + g) * a.nch + chunk) * a.cap;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (raw[q][g] == NOT_ALLOWED) continue;
      const int l = q * TILE_T + tid;
      const uint64_t key = ((uint64_t)score_key_bits(raw[q][g]) << 16) | (uint64_t)(TILE_CH - 1 - l);
      if (key < s.thr) continue;
      const uint32_t slot = atomicAdd(&s_out[g], 1u);
      if (slot < (uint32_t)a.cap) {
        a.c_score[base + slot] = __builtin_bit_cast(float, raw[q][g]);
        a.c_id[base + slot] = (int32_t)(c0 + l);
      }
    }
  }
  __syncthreads();
  if (tid < TILE_G && lr0 + tid < a.n) a.c_cnt[(int64_t)(lr0 + tid) * a.nch + chunk] = (int32_t)min(s_out[tid], (uint32_t)a.cap);
}

// ---- 3. merge: one workgroup per row ------------------------------------------------------------------------------------------
struct MergeArgs {
  const float* c_score; const int32_t* c_id; const int32_t* c_cnt; const int32_t* c_beat;
  const int64_t* gt;
  int64_t* topk_ids; float* topk_scores; int32_t* gt_rank;
  int64_t r0;
  int nch, cap, K, lo, V;
};

__global__ __launch_bounds__(TILE_T) void full_merge_kernel(MergeArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t part[16];
  __shared__ Sel st;
  __shared__ uint32_t s_n, s_kmin, s_kmax, s_out, s_beat;
  __shared__ uint64_t sel_key[SEL_K_MAX];
  __shared__ float sel_val[SEL_K_MAX];
  const MergeSel L{hist, part, st, s_n, s_kmin, s_kmax, s_out, &s_beat, sel_key, sel_val};
  const int lr = blockIdx.x;
  const int64_t r = a.r0 + lr;
  const int64_t row = (int64_t)lr * a.nch;
  const int m = merge_select<TILE_T>(L, a.c_score, a.c_id, a.c_cnt, a.c_beat, row, a.nch, a.cap, a.K);
  merge_order<TILE_T>(L, m, a.K, [&](int pos, int64_t id, float score) {
    if (a.topk_ids) a.topk_ids[r * a.K + pos] = id;
    if (a.topk_scores) a.topk_scores[r * a.K + pos] = score;
  });
  if (threadIdx.x == 0 && a.gt_rank) {
    const int64_t g = a.gt ? a.gt[r] : -1;
    a.gt_rank[r] = (a.gt && g >= a.lo && g < a.V) ? (int32_t)(1 + s_beat) : 0;
  }
}

int64_t row_bytes(int32_t V, int32_t K) { return tile_chunks_of(V) * (tile_cap_of(K) * 8 + 8) + 4; }   // scores, ids | counts, beats | gt key

// ---- item neighbours: 1 / |row| of every table row, and the staged query rows ------------------------------------------------
// one thread per row (b4r_cosine_chain.h); b4r_item_rnorm_launch below serves every entry point that needs rnorm
__global__ __launch_bounds__(TILE_T) void item_rnorm_kernel(const float* __restrict__ table, int H, int V, float* __restrict__ rnorm) {
  const int64_t j = (int64_t)blockIdx.x * TILE_T + threadIdx.x;
  if (j >= V) return;
  rnorm[j] = b4r_row_rnorm(table + j * H, H);
}

// qhat[r][k] = table[q_r][k] (* rnorm[q_r] when given); qrow[r] = r, or -1 (the sweep ranks nothing for the row) when q_r is no item
__global__ __launch_bounds__(TILE_T) void item_query_kernel(const float* __restrict__ table, int H, int V, int lo,
                                                        const int64_t* __restrict__ query, int R, const float* __restrict__ rnorm,
                                                        float* __restrict__ qhat, int64_t* __restrict__ qrow) {
  const int64_t i = (int64_t)blockIdx.x * TILE_T + threadIdx.x;
  if (i >= (int64_t)R * H) return;
  const int r = (int)(i / H), k = (int)(i - (int64_t)r * H);
  const int64_t q = query[r];
  const bool ok = q >= lo && q < V;
  float v = 0.f;
  if (ok) {
    v = table[q * H + k];
    if (rnorm) v *= rnorm[q];
  }
  qhat[i] = v;
  if (k == 0) qrow[r] = ok ? r : -1;
}

using SweepFn = void (*)(SweepArgs, SweepExtra);
SweepFn sweep_instance(bool filt, bool scale, bool bias) {
  static const SweepFn table[8] = {
      full_sweep_kernel<false, false, false>, full_sweep_kernel<false, false, true>, full_sweep_kernel<false, true, false>,
      full_sweep_kernel<false, true, true>,   full_sweep_kernel<true, false, false>, full_sweep_kernel<true, false, true>,
      full_sweep_kernel<true, true, false>,   full_sweep_kernel<true, true, true>};
  return table[(filt ? 4 : 0) | (scale ? 2 : 0) | (bias ? 1 : 0)];
}

// the one implementation behind b4r_rank_full (allow_bits, item_scale NULL; bias required), b4r_rank_full_ex and b4r_item_neighbours
int rank_full_impl(const char* what, bool bias_required, const float* hidden, int32_t hidden_ld, const int64_t* hidden_row,
                   const float* table, const float* bias, int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude,
                   int32_t E, const int64_t* gt, int32_t K, const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter,
                   const float* item_scale, int64_t* topk_ids, float* topk_scores, int32_t* gt_rank, void* scratch,
                   int64_t scratch_bytes, hipStream_t s) {
  B4R_CHECK_ARG(R >= 0 && K >= 0 && K <= SEL_K_MAX && E >= 0 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, K = %d in [0, %d], E = %d, first_item = %d)", what, R, K, SEL_K_MAX, E, first_item);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d)", what, H, hidden_ld, V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(hidden && table && (bias || !bias_required), B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int64_t per_row = row_bytes(V, K);
  const int64_t group = tile_group_of(scratch, scratch_bytes, per_row, R, TILE_G);   // whole sweep groups
  B4R_CHECK_ARG(group >= std::min<int64_t>(R, TILE_G), B4R_E_NOMEM,
                "%s: scratch of %lld bytes is too small: %lld bytes per row, %d rows at least (b4r_rank_full_scratch_bytes)", what,
                (long long)scratch_bytes, (long long)per_row, std::min<int32_t>(R, TILE_G));
  const int nch = (int)tile_chunks_of(V);
  B4R_CHECK_ARG(nch <= 65535, B4R_E_SHAPE, "%s: V = %d is too large", what, V);
  const int cap = (int)tile_cap_of(K);
  float* c_score = reinterpret_cast<float*>(tile_scratch_base(scratch));
  int32_t* c_id = reinterpret_cast<int32_t*>(c_score + group * nch * cap);
  int32_t* c_cnt = c_id + group * nch * cap;
  int32_t* c_beat = c_cnt + group * nch;
  uint32_t* gkey = reinterpret_cast<uint32_t*>(c_beat + group * nch);
  const SweepFn sweep = sweep_instance(allow_bits != nullptr, item_scale != nullptr, bias != nullptr);
  for (int64_t r0 = 0; r0 < R; r0 += group) {
    const int n = (int)std::min<int64_t>(group, R - r0);
    if (gt) {
      hipLaunchKernelGGL(full_gt_key_kernel, dim3(b4r_cdiv(n, 64)), dim3(64), 0, s, hidden, hidden_ld, hidden_row, table, bias,
                         item_scale, H, V, first_item, gt, r0, n, gkey);
    }
    SweepArgs sa{hidden, hidden_row, table, bias, exclude, gt, gkey, c_score, c_id, c_cnt, c_beat, r0,
                 hidden_ld, H, V, first_item, E, n, nch, cap};
    SweepExtra sx{item_scale, allow_bits, row_filter, n_filters};
    hipLaunchKernelGGL(sweep, dim3(b4r_cdiv(n, TILE_G), nch), dim3(TILE_T), 0, s, sa, sx);
    MergeArgs ma{c_score, c_id, c_cnt, c_beat, gt, topk_ids, topk_scores, gt_rank, r0, nch, cap, K, first_item, V};
    hipLaunchKernelGGL(full_merge_kernel, dim3(n), dim3(TILE_T), 0, s, ma);
  }
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

// b4r_item_neighbours' own regions in front of the sweep's scratch, each a multiple of 16 bytes: rnorm [V] | qhat [R, width] | qrow [R]
int64_t neighbour_bytes(int32_t R, int32_t V, int32_t width) {
  return b4r_align16((int64_t)V * 4) + b4r_align16((int64_t)R * width * 4) + b4r_align16((int64_t)R * 8);
}

}  // namespace

void b4r_item_rnorm_launch(const float* table, int width, int V, float* rnorm, hipStream_t stream) {
  hipLaunchKernelGGL(item_rnorm_kernel, dim3(b4r_cdiv(V, TILE_T)), dim3(TILE_T), 0, stream, table, width, V, rnorm);
}

extern "C" int64_t b4r_rank_full_scratch_bytes(int32_t R, int32_t V, int32_t K) {
  if (R <= 0 || V <= 0 || K < 0 || K > SEL_K_MAX) return 0;
  return (int64_t)R * row_bytes(V, K) + 64;   // + room for the 16-byte alignment of the regions
}

extern "C" int b4r_rank_full(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                             int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E, const int64_t* gt,
                             int32_t K, int64_t* topk_ids, float* topk_scores, int32_t* gt_rank, void* scratch, int64_t scratch_bytes,
                             b4r_stream_t stream) {
  return rank_full_impl("b4r_rank_full", true, hidden, hidden_ld, hidden_row, table, bias, H, V, first_item, R, exclude, E, gt, K,
                        nullptr, 0, nullptr, nullptr, topk_ids, topk_scores, gt_rank, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int b4r_rank_full_ex(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table,
                                const float* bias, int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude,
                                int32_t E, const int64_t* gt, int32_t K, int64_t* topk_ids, float* topk_scores, int32_t* gt_rank,
                                void* scratch, int64_t scratch_bytes, b4r_stream_t stream, const uint32_t* allow_bits,
                                int32_t n_filters, const int32_t* row_filter, const float* item_scale) {
  return rank_full_impl("b4r_rank_full_ex", false, hidden, hidden_ld, hidden_row, table, bias, H, V, first_item, R, exclude, E, gt, K,
                        allow_bits, n_filters, row_filter, item_scale, topk_ids, topk_scores, gt_rank, scratch, scratch_bytes,
                        (hipStream_t)stream);
}

extern "C" int64_t b4r_item_neighbours_scratch_bytes(int32_t R, int32_t V, int32_t K, int32_t width) {
  if (R <= 0 || V <= 0 || K < 0 || K > SEL_K_MAX || width <= 0) return 0;
  return neighbour_bytes(R, V, width) + b4r_rank_full_scratch_bytes(R, V, K);
}

extern "C" int b4r_item_neighbours(const float* table, int32_t ld, int32_t width, int32_t V, int32_t first_item,
                                   const int64_t* query_ids, int32_t R, int32_t metric, const uint32_t* allow_bits, int32_t n_filters,
                                   const int32_t* row_filter, int32_t K, int64_t* topk_ids, float* topk_scores, void* scratch,
                                   int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_item_neighbours";
  B4R_CHECK_ARG(R >= 0 && K >= 0 && K <= SEL_K_MAX && first_item >= 0, B4R_E_SHAPE, "%s: bad shape (R = %d, K = %d in [0, %d], first_item = %d)",
                what, R, K, SEL_K_MAX, first_item);
  // the sweep reads table row j at table + j * width: a padded table (ld > width) is not taken
  B4R_CHECK_ARG(width > 0 && width % 4 == 0 && width <= 4096 && ld == width && V > 0, B4R_E_SHAPE,
                "%s: bad shape (width = %d: a multiple of 4 up to 4096, ld = %d: must equal width, V = %d)", what, width, ld, V);
  B4R_CHECK_ARG(metric == B4R_SIM_DOT || metric == B4R_SIM_COSINE, B4R_E_BADARG, "%s: unknown metric %d", what, metric);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(table && query_ids, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int64_t pad = scratch ? (int64_t)((16 - ((uintptr_t)scratch & 15)) & 15) : 0;
  const int64_t own = neighbour_bytes(R, V, width);
  B4R_CHECK_ARG(scratch && scratch_bytes - pad > own, B4R_E_NOMEM, "%s: scratch of %lld bytes is too small (b4r_item_neighbours_scratch_bytes)",
                what, (long long)scratch_bytes);
  char* p = reinterpret_cast<char*>(scratch) + pad;
  float* rnorm = reinterpret_cast<float*>(p);
  float* qhat = reinterpret_cast<float*>(p + b4r_align16((int64_t)V * 4));
  int64_t* qrow = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(qhat) + b4r_align16((int64_t)R * width * 4));
  char* rest = p + own;
  hipStream_t s = (hipStream_t)stream;
  const bool cosine = metric == B4R_SIM_COSINE;
  if (cosine) b4r_item_rnorm_launch(table, width, V, rnorm, s);
  hipLaunchKernelGGL(item_query_kernel, dim3(b4r_cdiv((int64_t)R * width, TILE_T)), dim3(TILE_T), 0, s, table, width, V, first_item, query_ids, R,
                     cosine ? rnorm : nullptr, qhat, qrow);
  // the query excludes itself: query_ids is the [R, 1] exclude list
  return rank_full_impl(what, false, qhat, width, qrow, table, nullptr, width, V, first_item, R, query_ids, 1, nullptr, K, allow_bits,
                        n_filters, row_filter, cosine ? rnorm : nullptr, topk_ids, topk_scores, nullptr, rest,
                        scratch_bytes - pad - own, s);
}
