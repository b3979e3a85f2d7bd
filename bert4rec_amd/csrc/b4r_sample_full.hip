// Sampled recommendations: k items drawn without replacement from softmax(scores / T) over the allowed catalogue, without an
// [R, V] score matrix.  Drawing k items without replacement from a softmax is taking the k largest of t_j + Gumbel_j (the Gumbel
// top-k trick, the draw order being the descending key order), so this is b4r_rank_full's sweep with a perturbed key.
//
// Serves  exploration traffic and propensity-logged lists   (BERT4RecModel.recommend_tensor(sample_seed=), Recommender.recommend_batch)
//         full-ranking evaluation of sampled lists           (evaluation.get(full_ranking=True, list_k=, sample_seed=))
//
// Contract (include/b4r.h, b4r_sample_full): s(r, j) and allowed(r) are b4r_rank_full_ex's bit for bit, t = fl32(s * inv_temperature)
// is b4r_score_dist's, key(r, j) = fl32(t + g(word(seed, stream(r), j))) with the noise of b4r_common.h (b4r_gumbel23: a fixed
// sequence of rounded fp64 operations, the same bits on the host).  The outputs are the first K of allowed(r) by key descending
// (-0.0 as +0.0, ties to the lower id), with the unperturbed score of each.
//
// Two launches per group of rows that fits the scratch:
//   1. sweep   grid (group of 16 rows) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h, staged and selected as in b4r_rank_full.hip.  The
//              noise is added to the 4 ids x 16 rows of scores a thread holds in registers (skipped where the id is not allowed);
//              the chunk's best min(K, 1024) keys are chosen by the radix select on (key bits << 16 | 1023 - local id) and go to
//              scratch as (key, id) pairs in any order.
//   2. merge   one workgroup per row: the radix select on (key bits << 32 | ~id) over all chunks' candidates, the order of the K
//              survivors by counting, then one thread per pick recomputes the unperturbed score by the k-ascending chain.
// b4r_sample_pool is the truncated variant: one workgroup per row orders a pool of M <= 1024 (id, score) entries by their keys.
// No floating-point atomics; LDS integer atomics only place or count, and the outputs do not depend on their order.
#include <algorithm>
#include <cmath>

#include "b4r_common.h"
#include "b4r_catalogue_tile.h"

namespace {

// key = fl32(fl32(s * inv_t) + g): two rounded fp32 operations (never one fma)
__device__ __forceinline__ float sample_key(float s, float inv_t, float g) {
#pragma clang fp contract(off)
  const float t = s * inv_t;
  return t + g;
}

// ---- the noise alone (test surface): one thread per word, grid-stride ---------------------------------------------------------------
__global__ __launch_bounds__(TILE_T) void gumbel_noise_kernel(const uint32_t* __restrict__ words, int64_t n, float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * TILE_T;
  for (int64_t i = (int64_t)blockIdx.x * TILE_T + threadIdx.x; i < n; i += step) out[i] = b4r_gumbel23(words[i]);
}

// ---- 1. sweep: (group of TILE_G rows) x (chunk of TILE_CH ids) -----------------------------------------------------------------
struct SampleArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude; const int64_t* gt;
  const uint32_t* allow; const int32_t* row_filter;   // [n_filters][ceil(V / 32)], [R] or NULL
  const int64_t* row_stream;
  float* c_key; int32_t* c_id; int32_t* c_cnt;        // [n][nch][cap], [n][nch]
  int64_t r0, stream0;
  uint32_t seed_lo, seed_hi;
  float inv_t;
  int hidden_ld, H, V, lo, E, n, nch, cap, n_filters;
};

__global__ __launch_bounds__(TILE_T, 2) void sample_sweep_kernel(SampleArgs a) {
  __shared__ float tile[TILE_IPT * TILE_T * (TILE_KB + 1)];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[TILE_G][TILE_CH / 32];
  __shared__ uint32_t hist[TILE_G][256];
  __shared__ uint32_t part[TILE_G][16];
  __shared__ Sel st[TILE_G];
  __shared__ uint32_t s_cnt[TILE_G], s_kmin[TILE_G], s_kmax[TILE_G], s_out[TILE_G], s_slo[TILE_G], s_shi[TILE_G];
  __shared__ int64_t s_hoff[TILE_G], s_gt[TILE_G];
  __shared__ int s_alldone;

  const int tid = threadIdx.x, lane = tid & 63;
  const int lr0 = blockIdx.x * TILE_G;
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const int H = a.H;

  if (tid < TILE_G) {
    const int lr = lr0 + tid;
    const bool rv = lr < a.n;
    const int64_t r = a.r0 + lr;   // the absolute row of the call: the noise does not depend on the grouping
    s_hoff[tid] = rv ? (a.hidden_row ? a.hidden_row[r] : r) * a.hidden_ld : -1;
    s_gt[tid] = (rv && a.gt) ? a.gt[r] : -1;
    const uint64_t stream = rv ? (a.row_stream ? (uint64_t)a.row_stream[r] : (uint64_t)a.stream0 + (uint64_t)r) : 0ull;
    s_slo[tid] = (uint32_t)stream; s_shi[tid] = (uint32_t)(stream >> 32);
    s_cnt[tid] = 0; s_out[tid] = 0;
    s_kmin[tid] = 0xFFFFFFFFu; s_kmax[tid] = 0u;
  }
  tile_row_bitmap(bits, a.allow != nullptr, a.allow, a.row_filter, a.n_filters, a.exclude, a.E, s_hoff, a.r0, lr0, a.n, a.V, c0);

  // ---- keys: raw fp32 bits in registers, NOT_ALLOWED where the id is not drawn -----------------------------------------------------
  uint32_t raw[TILE_Q][TILE_G];
#pragma unroll
  for (int ps = 0; ps < TILE_Q / TILE_IPT; ++ps) {
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
        const int g = tid / TILE_KB, k = tid - g * TILE_KB;
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
      const float b = (a.bias && inb) ? a.bias[j] : 0.f;
      const float sc = (a.scale && inb) ? a.scale[j] : 1.f;
      const uint32_t h0 = b4r_hash32((uint32_t)(uint64_t)j ^ a.seed_lo);   // the row-independent round of b4r_sample_word_hd
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) {
        const bool ex = (bits[g][l >> 5] >> (l & 31)) & 1u;
        const bool ok = inb && s_hoff[g] >= 0 && (!ex || j == s_gt[g]);
        uint32_t kbits = NOT_ALLOWED;
        if (ok) {
          float s = acc[ii][g] + b;
          if (a.scale) s = s * sc;
          uint32_t w = b4r_hash32((h0 ^ s_slo[g]) + a.seed_hi);
          w = b4r_hash32(w ^ s_shi[g]);
          kbits = __builtin_bit_cast(uint32_t, sample_key(s, a.inv_t, b4r_gumbel23(w)));
        }
        raw[q][g] = kbits;
      }
    }
  }

  // ---- per row: allowed count, key range ------------------------------------------------------------------------------------------
#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    uint32_t cnt = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (raw[q][g] == NOT_ALLOWED) continue;
      const uint32_t k = score_key_bits(raw[q][g]);
      cnt += 1;
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    cnt = wave_sum_u32(cnt);
    kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
    if (lane == 0) {
      atomicAdd(&s_cnt[g], cnt);
      atomicMin(&s_kmin[g], kmin); atomicMax(&s_kmax[g], kmax);
    }
  }
  __syncthreads();
  if (tid < TILE_G && lr0 + tid < a.n) {
    const int n = (int)s_cnt[tid];
    sel_init(st[tid], n, min(a.cap, n), s_kmin[tid], s_kmax[tid]);
  } else if (tid < TILE_G) {
    sel_init(st[tid], 0, 0, 0u, 0u);
  }
  if (tid == 0) s_alldone = 0;

  // ---- radix select over (key image << 16 | TILE_CH-1 - local id) ------------------------------------------------------------------
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
        a.c_key[base + slot] = __builtin_bit_cast(float, raw[q][g]);
        a.c_id[base + slot] = (int32_t)(c0 + l);
      }
    }
  }
  __syncthreads();
  if (tid < TILE_G && lr0 + tid < a.n) a.c_cnt[(int64_t)(lr0 + tid) * a.nch + chunk] = (int32_t)min(s_out[tid], (uint32_t)a.cap);
}

// ---- 2. merge: one workgroup per row ------------------------------------------------------------------------------------------
struct SampleMergeArgs {
  const float* c_key; const int32_t* c_id; const int32_t* c_cnt;
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  int64_t* out_ids; float* out_scores; float* out_keys;
  int64_t r0;
  int nch, cap, K, hidden_ld, H;
};

__global__ __launch_bounds__(TILE_T) void sample_merge_kernel(SampleMergeArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t part[16];
  __shared__ Sel st;
  __shared__ uint32_t s_n, s_kmin, s_kmax, s_out;
  __shared__ uint64_t sel_key[SEL_K_MAX];
  __shared__ float sel_val[SEL_K_MAX];
  const MergeSel L{hist, part, st, s_n, s_kmin, s_kmax, s_out, nullptr, sel_key, sel_val};
  const int lr = blockIdx.x;
  const int64_t r = a.r0 + lr;
  const int64_t row = (int64_t)lr * a.nch;
  const int m = merge_select<TILE_T>(L, a.c_key, a.c_id, a.c_cnt, nullptr, row, a.nch, a.cap, a.K);
  const int64_t hr = a.hidden_row ? a.hidden_row[r] : r;
  merge_order<TILE_T>(L, m, a.K, [&](int pos, int64_t id, float key) {
    if (a.out_ids) a.out_ids[r * a.K + pos] = id;
    if (a.out_keys) a.out_keys[r * a.K + pos] = key;
    // the unperturbed score, by the chain every sweep uses: b4r_rank_full's bits for this id (id = -1: merge_order's padding call)
    if (a.out_scores)
      a.out_scores[r * a.K + pos] = id >= 0 ? row_score(a.hidden + hr * a.hidden_ld, a.table + id * a.H, a.bias, a.scale, id, a.H) : -INFINITY;
  });
}

// ---- b4r_sample_pool: one workgroup per row --------------------------------------------------------------------------------------
struct PoolArgs {
  const int64_t* pool_ids; const float* pool_scores; const int64_t* row_stream;
  int64_t* out_ids; float* out_scores; float* out_keys; int32_t* out_pos;
  uint64_t seed; int64_t stream0;
  float inv_t;
  int M, V, K;
};

__global__ __launch_bounds__(TILE_T) void sample_pool_kernel(PoolArgs a) {
  __shared__ int64_t p_id[SEL_K_MAX];
  __shared__ uint32_t p_img[SEL_K_MAX];   // the key's order-preserving image; dead entries are marked in p_id (-1)
  __shared__ float p_key[SEL_K_MAX];
  __shared__ uint32_t s_live;
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int64_t stream = a.row_stream ? a.row_stream[r] : (int64_t)((uint64_t)a.stream0 + (uint64_t)r);
  if (tid == 0) s_live = 0;
  __syncthreads();
  uint32_t live = 0;
  for (int i = tid; i < a.M; i += TILE_T) {
    const int64_t id = a.pool_ids[r * a.M + i];
    const float s = a.pool_scores[r * a.M + i];
    const bool ok = id >= 0 && id < a.V && isfinite(s);
    float key = -INFINITY;
    if (ok) key = sample_key(s, a.inv_t, b4r_gumbel23(b4r_sample_word_hd(a.seed, stream, id)));
    p_id[i] = ok ? id : -1;
    p_key[i] = key;
    p_img[i] = score_key(key);
    live += ok ? 1u : 0u;
  }
  live = wave_sum_u32(live);
  if ((tid & 63) == 0) atomicAdd(&s_live, live);
  __syncthreads();
  const int n = (int)s_live;
  for (int i = tid; i < a.M; i += TILE_T) {
    const int64_t id = p_id[i];
    if (id < 0) continue;
    const uint32_t ki = p_img[i];
    int pos = 0;
    for (int j = 0; j < a.M; ++j) {
      const int64_t idj = p_id[j];
      const uint32_t kj = p_img[j];
      const bool before = idj >= 0 && (kj > ki || (kj == ki && (idj < id || (idj == id && j < i))));
      pos += before ? 1 : 0;
    }
    if (pos >= a.K) continue;
    if (a.out_ids) a.out_ids[r * a.K + pos] = id;
    if (a.out_scores) a.out_scores[r * a.K + pos] = a.pool_scores[r * a.M + i];
    if (a.out_keys) a.out_keys[r * a.K + pos] = p_key[i];
    if (a.out_pos) a.out_pos[r * a.K + pos] = i;
  }
  for (int p = n + tid; p < a.K; p += TILE_T) {
    if (a.out_ids) a.out_ids[r * a.K + p] = -1;
    if (a.out_scores) a.out_scores[r * a.K + p] = -INFINITY;
    if (a.out_keys) a.out_keys[r * a.K + p] = -INFINITY;
    if (a.out_pos) a.out_pos[r * a.K + p] = -1;
  }
}

int64_t row_bytes(int32_t V, int32_t K) { return tile_chunks_of(V) * (tile_cap_of(K) * 8 + 4); }   // keys, ids | counts

}  // namespace

extern "C" float b4r_gumbel_from_hash(uint32_t hash_word) { return b4r_gumbel23(hash_word); }

extern "C" uint32_t b4r_sample_word(uint64_t seed, int64_t stream, int64_t id) { return b4r_sample_word_hd(seed, stream, id); }

extern "C" int b4r_gumbel_noise(const uint32_t* words, int64_t n, float* out, b4r_stream_t stream) {
  const char* what = "b4r_gumbel_noise";
  B4R_CHECK_ARG(n >= 0, B4R_E_SHAPE, "%s: n = %lld", what, (long long)n);
  if (n == 0) return B4R_OK;
  B4R_CHECK_ARG(words && out, B4R_E_BADARG, "%s: null argument", what);
  const int blocks = (int)std::min<int64_t>(((int64_t)n + TILE_T - 1) / TILE_T, 8192);
  hipLaunchKernelGGL(gumbel_noise_kernel, dim3(blocks), dim3(TILE_T), 0, (hipStream_t)stream, words, n, out);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int64_t b4r_sample_full_scratch_bytes(int32_t R, int32_t V, int32_t K) {
  if (R <= 0 || V <= 0 || K < 0 || K > SEL_K_MAX) return 0;
  return (int64_t)R * row_bytes(V, K) + 64;   // + room for the 16-byte alignment of the regions
}

extern "C" int b4r_sample_full(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                               int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E,
                               const int64_t* gt, int32_t K, const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter,
                               const float* item_scale, float inv_temperature, uint64_t seed, const int64_t* row_stream,
                               int64_t stream0, int64_t* out_ids, float* out_scores, float* out_keys, void* scratch,
                               int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_sample_full";
  B4R_CHECK_ARG(R >= 0 && K >= 0 && K <= SEL_K_MAX && E >= 0 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, K = %d in [0, %d], E = %d, first_item = %d)", what, R, K, SEL_K_MAX, E, first_item);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d)", what, H, hidden_ld, V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  B4R_CHECK_ARG(std::isfinite(inv_temperature) && inv_temperature > 0.f, B4R_E_BADARG,
                "%s: inv_temperature = %g must be finite and > 0", what, (double)inv_temperature);
  if (R == 0 || K == 0) return B4R_OK;
  B4R_CHECK_ARG(hidden && table, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int64_t per_row = row_bytes(V, K);
  const int64_t group = tile_group_of(scratch, scratch_bytes, per_row, R, TILE_G);   // whole sweep groups
  B4R_CHECK_ARG(group >= std::min<int64_t>(R, TILE_G), B4R_E_NOMEM,
                "%s: scratch of %lld bytes is too small: %lld bytes per row, %d rows at least (b4r_sample_full_scratch_bytes)", what,
                (long long)scratch_bytes, (long long)per_row, std::min<int32_t>(R, TILE_G));
  const int nch = (int)tile_chunks_of(V);
  B4R_CHECK_ARG(nch <= 65535, B4R_E_SHAPE, "%s: V = %d is too large", what, V);
  const int cap = (int)tile_cap_of(K);
  float* c_key = reinterpret_cast<float*>(tile_scratch_base(scratch));
  int32_t* c_id = reinterpret_cast<int32_t*>(c_key + group * nch * cap);
  int32_t* c_cnt = c_id + group * nch * cap;
  hipStream_t s = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < R; r0 += group) {
    const int n = (int)std::min<int64_t>(group, R - r0);
    SampleArgs sa{hidden, hidden_row, table, bias, item_scale, exclude, gt, allow_bits, row_filter, row_stream, c_key, c_id, c_cnt,
                  r0, stream0, (uint32_t)seed, (uint32_t)(seed >> 32), inv_temperature, hidden_ld, H, V, first_item, E, n, nch, cap,
                  n_filters};
    hipLaunchKernelGGL(sample_sweep_kernel, dim3(b4r_cdiv(n, TILE_G), nch), dim3(TILE_T), 0, s, sa);
    SampleMergeArgs ma{c_key, c_id, c_cnt, hidden, hidden_row, table, bias, item_scale, out_ids, out_scores, out_keys, r0,
                       nch, cap, K, hidden_ld, H};
    hipLaunchKernelGGL(sample_merge_kernel, dim3(n), dim3(TILE_T), 0, s, ma);
  }
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int b4r_sample_pool(const int64_t* pool_ids, const float* pool_scores, int32_t R, int32_t M, int32_t V, float inv_temperature,
                               uint64_t seed, const int64_t* row_stream, int64_t stream0, int32_t K, int64_t* out_ids,
                               float* out_scores, float* out_keys, int32_t* out_pos, b4r_stream_t stream) {
  const char* what = "b4r_sample_pool";
  B4R_CHECK_ARG(R >= 0 && M >= 1 && M <= SEL_K_MAX && K >= 0 && K <= M && V > 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, M = %d in [1, %d], K = %d in [0, M], V = %d)", what, R, M, SEL_K_MAX, K, V);
  B4R_CHECK_ARG(std::isfinite(inv_temperature) && inv_temperature > 0.f, B4R_E_BADARG,
                "%s: inv_temperature = %g must be finite and > 0", what, (double)inv_temperature);
  if (R == 0 || K == 0) return B4R_OK;
  B4R_CHECK_ARG(pool_ids && pool_scores, B4R_E_BADARG, "%s: null argument", what);
  PoolArgs pa{pool_ids, pool_scores, row_stream, out_ids, out_scores, out_keys, out_pos, seed, stream0, inv_temperature, M, V, K};
  hipLaunchKernelGGL(sample_pool_kernel, dim3(R), dim3(TILE_T), 0, (hipStream_t)stream, pa);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
