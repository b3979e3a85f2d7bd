// Item ranks on the catalogue sweep (include/b4r.h: b4r_item_ranks) and the multi-target metric sums over such ranks
// (b4r_rank_metrics_multi): where do Q given items stand for each row, among the items the row could be served, without Q sweeps and
// without an [R, V] buffer.
//
// Serves  BERT4RecModel.item_ranks_tensor / item_ranks, Recommender.item_ranks ("X stands at 312 of 26 000 for this user"), and the
//         multi-target evaluation (evaluation.get(full_ranking=True, multi_target=True): Recall / NDCG / MAP / MRR / AUC over the
//         last n items of a sequence).
//
// Contract: s(r, j) and the order are b4r_rank_full_ex's bit for bit (row_score of b4r_catalogue_tile.h; score descending through
// score_key, ties to the lower id).  The order is carried by one unique 64-bit key per item, key(j) = score_key(s) << 32 | ~j: j
// stands before q iff key(j) > key(q).  0 is no item's key and marks a query that is not valid.
//
// Three launches per group of rows that fits the scratch:
//   1. queries   one workgroup per row: the Q query keys by the scalar chain, their descending order by counting (sorted keys and each
//                query's place in scratch), membership in the row's allowed set, query_scores; the row's Q + 1 counters are zeroed.
//   2. sweep     grid (tile of 16 rows) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h, staged as b4r_rank_full's sweep stages
//                it (4 ids x 16 rows of raw score bits per thread in registers).  After the k-loop the staging buffer is dead and
//                holds the 16 rows' sorted query keys and their [16][Q + 1] histograms.  Every allowed (row, id) finds
//                b = #{sorted keys >= key(j)} by a branch-free search of floor(log2 Q) + 1 steps and adds 1 to bucket b of its row: j
//                stands before exactly the queries at the sorted places b, b + 1, ...  (a query never counts itself, and the places
//                of a repeated id get the same count).  Few large buckets (Q = 1: two per row) would send 64 lanes to one LDS address:
//                a wave first combines the lanes that share the first pending bucket (twice), the lanes left over add on their own.
//                Non-zero buckets leave with one global integer atomic each.
//   3. finish    one workgroup per row: the count before the query at place p is the sum of the buckets 0 .. p; back to query order,
//                the mode's zeroing, member, row_n = the sum of all buckets.
// Integer counting only: no floating-point atomics, no workgroup waits for another, and the bits do not depend on the order in which
// the atomics land.
#include <algorithm>

#include "b4r_common.h"
#include "b4r_catalogue_tile.h"

namespace {

constexpr int IR_Q_MAX = 256;            // queries per row
constexpr int IR_COMBINE = 2;            // buckets a wave combines per (row, id step) before its lanes add on their own
constexpr int IR_COMBINE_MIN = 4;        // lanes that make a combination worth its ballots
constexpr int IR_VALID = 2, IR_MEMBER = 1;   // flag bits of a query in scratch
// the sweep's LDS after the k-loop: sorted keys [16][Q] (8 bytes) and histograms [16][Q + 1] (4 bytes); before it: the staging tile
constexpr int IR_TABLE_BYTES = TILE_G * IR_Q_MAX * 8 + TILE_G * (IR_Q_MAX + 1) * 4;
constexpr int IR_STAGE_BYTES = (int)sizeof(float) * TILE_IPT * TILE_T * (TILE_KB + 1);
constexpr int IR_LDS_BYTES = IR_TABLE_BYTES > IR_STAGE_BYTES ? IR_TABLE_BYTES : IR_STAGE_BYTES;

__device__ __forceinline__ uint64_t item_key(uint32_t score_image, int64_t j) {
  return ((uint64_t)score_image << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j);
}

// ---- 1. the queries of one row ---------------------------------------------------------------------------------------------------
struct RanksQueryArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude;
  const uint32_t* allow; const int32_t* row_filter;
  const int64_t* query_ids;
  float* query_scores;
  uint64_t* skey; int32_t* spos; uint32_t* cnt; uint8_t* sflag;   // [n][Q], [n][Q], [n][Q + 1], [n][Q]
  int64_t r0;
  int hidden_ld, H, V, lo, E, n, Q, n_filters;
};

__global__ __launch_bounds__(TILE_T) void ranks_query_kernel(RanksQueryArgs a) {
  __shared__ uint64_t keys[IR_Q_MAX];
  const int tid = threadIdx.x;
  const int lr = blockIdx.x;
  const int64_t r = a.r0 + lr;
  const int Q = a.Q;
  for (int t = tid; t <= Q; t += TILE_T) a.cnt[(int64_t)lr * (Q + 1) + t] = 0u;
  uint64_t key = 0;
  int flag = 0;
  if (tid < Q) {
    const int64_t q = a.query_ids[r * Q + tid];
    const int64_t hr = a.hidden_row ? a.hidden_row[r] : r;
    float s = -INFINITY;
    if (q >= a.lo && q < a.V && hr >= 0) {
      s = row_score(a.hidden + hr * a.hidden_ld, a.table + q * a.H, a.bias, a.scale, q, a.H);
      key = item_key(score_key(s), q);
      bool ok = true;
      if (a.allow) {
        const int32_t f = a.row_filter ? a.row_filter[r] : 0;
        const int64_t W = ((int64_t)a.V + 31) >> 5;
        if (f >= 0 && f < a.n_filters) ok = (a.allow[(int64_t)f * W + (q >> 5)] >> (q & 31)) & 1u;
      }
      for (int e = 0; ok && e < a.E; ++e) ok = a.exclude[r * a.E + e] != q;
      flag = IR_VALID | (ok ? IR_MEMBER : 0);
    }
    if (a.query_scores) a.query_scores[r * Q + tid] = s;
    keys[tid] = key;
  }
  __syncthreads();
  if (tid < Q) {
    int pos = 0;
    for (int k = 0; k < Q; ++k) {
      const uint64_t o = keys[k];
      pos += (o > key || (o == key && k < tid)) ? 1 : 0;   // a permutation of 0 .. Q-1: descending key, equal keys in query order
    }
    a.skey[(int64_t)lr * Q + pos] = key;
    a.spos[(int64_t)lr * Q + tid] = pos;
    a.sflag[(int64_t)lr * Q + tid] = (uint8_t)flag;
  }
}

// ---- 2. sweep: (tile of TILE_G rows) x (chunk of TILE_CH ids) -------------------------------------------------------------------------
struct RanksSweepArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude;
  const uint32_t* allow; const int32_t* row_filter;
  const int64_t* query_ids;      // JOINT: the valid queries of a row are ranked whatever its filter and exclude list say; else NULL
  const uint64_t* skey; uint32_t* cnt;
  int64_t r0;
  int hidden_ld, H, V, lo, E, n, Q, n_filters, top;   // top: the largest power of two <= Q (0 for Q = 0)
};

__global__ __launch_bounds__(TILE_T, 2) void ranks_sweep_kernel(RanksSweepArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[IR_LDS_BYTES];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[TILE_G][TILE_CH / 32];
  __shared__ int64_t s_hoff[TILE_G], s_gt[TILE_G];
  float* tile = reinterpret_cast<float*>(lds);

  const int tid = threadIdx.x, lane = tid & 63;
  const int lr0 = blockIdx.x * TILE_G;
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const int H = a.H, Q = a.Q;

  if (tid < TILE_G) tile_row_setup(tid, lr0, a.n, a.r0, a.hidden_row, a.hidden_ld, nullptr, s_hoff, s_gt);
  tile_row_bitmap(bits, a.allow != nullptr, a.allow, a.row_filter, a.n_filters, a.exclude, a.E, s_hoff, a.r0, lr0, a.n, a.V, c0);
  if (a.query_ids) {
    __syncthreads();   // the exclude bits are set
    for (int f = tid; f < TILE_G * Q; f += TILE_T) {
      const int g = f / Q, i = f - g * Q;
      if (s_hoff[g] < 0) continue;
      const int64_t id = a.query_ids[(a.r0 + lr0 + g) * (int64_t)Q + i];
      if (id >= a.lo && id < a.V && id >= c0 && id < c0 + TILE_CH) {
        const int l = (int)(id - c0);
        atomicAnd(&bits[g][l >> 5], ~(1u << (l & 31)));
      }
    }
  }

  // ---- scores: raw fp32 bits in registers, NOT_ALLOWED where the id is not ranked -----------------------------------------------
  uint32_t raw[TILE_Q][TILE_G];
#pragma unroll
  for (int ps = 0; ps < TILE_Q / TILE_IPT; ++ps) {
    // (the k-block loop is written out in each of the sweeps: stated once as a function it changed their registers)
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
      const float b = (a.bias && inb) ? a.bias[j] : 0.f;
      const float sc = (a.scale && inb) ? a.scale[j] : 1.f;
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) {
        const bool ex = (bits[g][l >> 5] >> (l & 31)) & 1u;
        const bool ok = inb && s_hoff[g] >= 0 && !ex;
        float s = acc[ii][g] + b;
        if (a.scale) s = s * sc;
        raw[q][g] = ok ? __builtin_bit_cast(uint32_t, s) : NOT_ALLOWED;
      }
    }
  }

  // ---- the staging buffer is dead: it becomes the rows' sorted query keys and their histograms ----------------------------------
  uint64_t* s_key = reinterpret_cast<uint64_t*>(lds);                 // [TILE_G][Q]
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(s_key + TILE_G * Q);   // [TILE_G][Q + 1]
  __syncthreads();
  for (int i = tid; i < TILE_G * Q; i += TILE_T) {
    const int g = i / Q;
    s_key[i] = lr0 + g < a.n ? a.skey[(int64_t)(lr0 + g) * Q + (i - g * Q)] : 0ull;
  }
  for (int i = tid; i < TILE_G * (Q + 1); i += TILE_T) s_hist[i] = 0u;
  __syncthreads();

#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    const uint64_t* sk = s_key + g * Q;
    uint32_t* hist = s_hist + g * (Q + 1);
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      bool todo = raw[q][g] != NOT_ALLOWED;
      if (__ballot(todo) == 0ull) continue;   // uniform over the wave
      const uint64_t key = item_key(score_key_bits(raw[q][g]), c0 + q * TILE_T + tid);
      // b = #{sorted keys >= key}: the keys descend, so "sk[i] >= key" holds on a prefix; the same steps for every lane
      int b = 0;
#pragma unroll 1
      for (int step = a.top; step > 0; step >>= 1) {
        const int at = b + step;
        if (at <= Q && sk[at - 1] >= key) b = at;
      }
      // the lanes of the wave that share the first pending bucket add as one
#pragma unroll 1
      for (int it = 0; it < IR_COMBINE; ++it) {
        const uint64_t act = __ballot(todo);
        if (act == 0ull) break;
        const int first = __ffsll((unsigned long long)act) - 1;
        const int lead = __shfl(b, first, 64);
        const bool mine = todo && b == lead;
        const int c = (int)__popcll(__ballot(mine));
        if (c < IR_COMBINE_MIN) break;
        if (lane == first) atomicAdd(&hist[lead], (uint32_t)c);
        todo = todo && !mine;
      }
      if (todo) atomicAdd(&hist[b], 1u);
    }
  }
  __syncthreads();

  // flush: one global integer atomic per non-zero (row, bucket)
  for (int i = tid; i < TILE_G * (Q + 1); i += TILE_T) {
    const int g = i / (Q + 1);
    const uint32_t v = s_hist[i];
    if (v != 0u && lr0 + g < a.n) atomicAdd(&a.cnt[(int64_t)(lr0 + g) * (Q + 1) + (i - g * (Q + 1))], v);
  }
}

// ---- 3. finish: one workgroup per row ---------------------------------------------------------------------------------------------
struct RanksFinishArgs {
  const int32_t* spos; const uint32_t* cnt; const uint8_t* sflag;
  int32_t* ranks; int32_t* row_n; uint8_t* member;
  int64_t r0;
  int Q, members;
};

__global__ __launch_bounds__(TILE_T) void ranks_finish_kernel(RanksFinishArgs a) {
  __shared__ uint32_t c[IR_Q_MAX + 1];
  const int tid = threadIdx.x;
  const int lr = blockIdx.x;
  const int64_t r = a.r0 + lr;
  const int Q = a.Q;
  for (int t = tid; t <= Q; t += TILE_T) c[t] = a.cnt[(int64_t)lr * (Q + 1) + t];
  __syncthreads();
  if (tid == 0 && a.row_n) {
    uint32_t n = 0;
    for (int t = 0; t <= Q; ++t) n += c[t];
    a.row_n[r] = (int32_t)n;
  }
  if (tid >= Q) return;
  const int flag = a.sflag[(int64_t)lr * Q + tid];
  const bool valid = flag & IR_VALID, mem = flag & IR_MEMBER;
  int32_t rank = 0;
  if (valid && (mem || a.members != B4R_RANKS_STRICT)) {
    const int p = a.spos[(int64_t)lr * Q + tid];
    uint32_t before = 0;
    for (int t = 0; t <= p; ++t) before += c[t];
    rank = (int32_t)(1u + before);
  }
  if (a.ranks) a.ranks[r * Q + tid] = rank;
  if (a.member) a.member[r * Q + tid] = (valid && mem) ? 1 : 0;
}

int64_t ranks_row_bytes(int32_t Q) { return 17LL * Q + 4; }   // sorted keys (8), places (4), counters (4 (Q + 1)), flags (1)

// ---- multi-target metric sums --------------------------------------------------------------------------------------------------
// sums[m] += the sum over the rows with n > 0 entries > 0 of gain_m(row); users[0] += the number of such rows.  One workgroup: thread t
// adds its rows t, t + 256, ... in ascending order, then a tree over the 256 partial sums: bitwise reproducible.
constexpr int MM_MAX = 32;
struct MultiMetricP { int family[MM_MAX]; int cutoff[MM_MAX]; int n; };

__global__ __launch_bounds__(256) void rank_metrics_multi_kernel(const int32_t* ranks, const int32_t* row_n, int R, int Q,
                                                                 MultiMetricP mp, double* sums, int64_t* users) {
  __shared__ double red[256];
  __shared__ int64_t cnt[256];
  const int tid = threadIdx.x;
  double total[MM_MAX];
#pragma unroll
  for (int m = 0; m < MM_MAX; ++m) total[m] = 0.0;
  int64_t live = 0;
  for (int r = tid; r < R; r += 256) {
    const int32_t* rho = ranks + (int64_t)r * Q;
    int n = 0, best = 0x7fffffff;
    for (int i = 0; i < Q; ++i) {
      const int v = rho[i];
      if (v > 0) { n += 1; best = min(best, v); }
    }
    if (n == 0) continue;
    live += 1;
    double part[MM_MAX];   // the row's sums over its targets, one per metric
#pragma unroll
    for (int m = 0; m < MM_MAX; ++m) part[m] = 0.0;
    for (int i = 0; i < Q; ++i) {
      const int v = rho[i];
      if (v <= 0) continue;
      int le = 0, lt = 0;
      for (int j = 0; j < Q; ++j) {
        const int w = rho[j];
        le += (w > 0 && w <= v) ? 1 : 0;
        lt += (w > 0 && w < v) ? 1 : 0;
      }
      const double dcg = v == 1 ? 1.0 : 1.0 / log2((double)v + 1.0);
      const double prec = (double)le / (double)v;
      const double wrong = (double)(v - 1 - lt);
#pragma unroll
      for (int m = 0; m < MM_MAX; ++m) {
        if (m >= mp.n) continue;
        const int fam = mp.family[m], k = mp.cutoff[m];
        if (fam == B4R_MGAIN_RECALL) part[m] += v <= k ? 1.0 : 0.0;
        else if (fam == B4R_MGAIN_NDCG) part[m] += v <= k ? dcg : 0.0;
        else if (fam == B4R_MGAIN_MAP) part[m] += v <= k ? prec : 0.0;
        else if (fam == B4R_MGAIN_AUC) part[m] += wrong;
      }
    }
    const int others = row_n ? row_n[r] - n : 0;
#pragma unroll
    for (int m = 0; m < MM_MAX; ++m) {
      if (m >= mp.n) continue;
      const int fam = mp.family[m], k = mp.cutoff[m];
      const int top = min(n, k);
      double g = 0.0;
      if (fam == B4R_MGAIN_COUNT) g = (double)n;
      else if (fam == B4R_MGAIN_HIT) g = best <= k ? 1.0 : 0.0;
      else if (fam == B4R_MGAIN_MRR) g = 1.0 / (double)best;
      else if (fam == B4R_MGAIN_RECALL) g = part[m] / (double)n;
      else if (fam == B4R_MGAIN_NDCG) {
        double ideal = 0.0;
        for (int i = 1; i <= top; ++i) ideal += i == 1 ? 1.0 : 1.0 / log2((double)i + 1.0);
        g = top > 0 ? part[m] / ideal : 0.0;
      } else if (fam == B4R_MGAIN_MAP) g = top > 0 ? part[m] / (double)top : 0.0;
      else if (fam == B4R_MGAIN_AUC) g = others > 0 ? 1.0 - part[m] / ((double)n * (double)others) : 1.0;
      total[m] += g;
    }
  }
  cnt[tid] = live;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) cnt[tid] += cnt[tid + o]; __syncthreads(); }
  if (tid == 0) users[0] += cnt[0];
#pragma unroll
  for (int m = 0; m < MM_MAX; ++m) {
    if (m >= mp.n) continue;   // uniform over the workgroup
    __syncthreads();
    red[tid] = total[m];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) sums[m] += red[0];
  }
}

}  // namespace

extern "C" int64_t b4r_item_ranks_scratch_bytes(int32_t R, int32_t V, int32_t Q) {
  if (R <= 0 || V <= 0 || Q < 0 || Q > IR_Q_MAX) return 0;
  return (int64_t)R * ranks_row_bytes(Q) + 64;   // + room for the 16-byte alignment of the regions
}

extern "C" int b4r_item_ranks(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                              int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E,
                              const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter, const float* item_scale,
                              const int64_t* query_ids, int32_t Q, int32_t members, int32_t* ranks, float* query_scores, int32_t* row_n,
                              uint8_t* member, void* scratch, int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_item_ranks";
  B4R_CHECK_ARG(R >= 0 && Q >= 0 && Q <= IR_Q_MAX && E >= 0 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, Q = %d in [0, %d], E = %d, first_item = %d)", what, R, Q, IR_Q_MAX, E, first_item);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d)", what, H, hidden_ld, V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  B4R_CHECK_ARG(members == B4R_RANKS_STRICT || members == B4R_RANKS_SELF || members == B4R_RANKS_JOINT, B4R_E_BADARG,
                "%s: unknown members mode %d", what, members);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(hidden && table, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(Q == 0 || query_ids, B4R_E_BADARG, "%s: query_ids is NULL with Q = %d", what, Q);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int nch = (int)std::min<int64_t>(tile_chunks_of(V), 1 << 30);
  B4R_CHECK_ARG(nch <= 65535, B4R_E_SHAPE, "%s: V = %d is too large", what, V);
  const int64_t per_row = ranks_row_bytes(Q);
  const int64_t group = tile_group_of(scratch, scratch_bytes, per_row, R, TILE_G);   // whole sweep tiles
  B4R_CHECK_ARG(group >= std::min<int64_t>(R, TILE_G), B4R_E_NOMEM,
                "%s: scratch of %lld bytes is too small: %lld bytes per row, %d rows at least (b4r_item_ranks_scratch_bytes)", what,
                (long long)scratch_bytes, (long long)per_row, std::min<int32_t>(R, TILE_G));
  if (!ranks && !query_scores && !row_n && !member) return B4R_OK;
  uint64_t* skey = reinterpret_cast<uint64_t*>(tile_scratch_base(scratch));
  int32_t* spos = reinterpret_cast<int32_t*>(skey + group * Q);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(spos + group * Q);
  uint8_t* sflag = reinterpret_cast<uint8_t*>(cnt + group * (Q + 1));
  int top = 0;
  for (int p = 1; p <= Q; p <<= 1) top = p;
  const bool counts = ranks || row_n;
  hipStream_t s = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < R; r0 += group) {
    const int n = (int)std::min<int64_t>(group, R - r0);
    RanksQueryArgs qa{hidden, hidden_row, table, bias, item_scale, exclude, allow_bits, row_filter, query_ids, query_scores,
                      skey, spos, cnt, sflag, r0, hidden_ld, H, V, first_item, E, n, Q, n_filters};
    hipLaunchKernelGGL(ranks_query_kernel, dim3(n), dim3(TILE_T), 0, s, qa);
    if (counts) {
      RanksSweepArgs sa{hidden, hidden_row, table, bias, item_scale, exclude, allow_bits, row_filter,
                        (members == B4R_RANKS_JOINT && Q > 0) ? query_ids : nullptr, skey, cnt, r0, hidden_ld, H, V, first_item, E, n, Q,
                        n_filters, top};
      hipLaunchKernelGGL(ranks_sweep_kernel, dim3(b4r_cdiv(n, TILE_G), nch), dim3(TILE_T), 0, s, sa);
    }
    if (counts || member) {
      RanksFinishArgs fa{spos, cnt, sflag, ranks, row_n, member, r0, Q, members};
      hipLaunchKernelGGL(ranks_finish_kernel, dim3(n), dim3(TILE_T), 0, s, fa);
    }
  }
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int b4r_rank_metrics_multi(const int32_t* ranks, const int32_t* row_n, int32_t R, int32_t Q, const int32_t* family,
                                      const int32_t* cutoff, int32_t n_metrics, double* gain_sums, int64_t* users,
                                      b4r_stream_t stream) {
  const char* what = "b4r_rank_metrics_multi";
  B4R_CHECK_ARG(ranks && family && cutoff && gain_sums && users, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(R > 0 && Q > 0 && Q <= IR_Q_MAX && n_metrics > 0 && n_metrics <= MM_MAX, B4R_E_SHAPE,
                "%s: bad shape (R = %d, Q = %d in [1, %d], 1..%d metrics)", what, R, Q, IR_Q_MAX, MM_MAX);
  MultiMetricP mp{};
  mp.n = n_metrics;
  for (int m = 0; m < n_metrics; ++m) {
    B4R_CHECK_ARG(family[m] >= B4R_MGAIN_COUNT && family[m] <= B4R_MGAIN_AUC, B4R_E_BADARG, "%s: unknown gain family %d", what,
                  family[m]);
    B4R_CHECK_ARG(family[m] != B4R_MGAIN_AUC || row_n, B4R_E_BADARG, "%s: the AUC family needs row_n", what);
    mp.family[m] = family[m]; mp.cutoff[m] = cutoff[m];
  }
  hipLaunchKernelGGL(rank_metrics_multi_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ranks, row_n, R, Q, mp, gain_sums, users);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
