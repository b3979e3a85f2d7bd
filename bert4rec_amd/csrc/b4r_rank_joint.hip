// Joint recommendations for several users: one full-catalogue top-K list per PARTY (a set of up to 16 ranked rows), without an
// [R, V] score matrix.  The group-recommendation strategies: additive, least misery, most pleasure, each with an optional veto.
//
// Serves  several users deciding together  (BERT4RecModel.recommend_joint_tensor, Recommender.recommend_together)
//
// Contract (include/b4r.h, b4r_rank_joint): s(r, j) and allowed(r) are b4r_rank_full_ex's with gt = NULL (k-ascending fp32 fma
// chain + bias, one multiply by item_scale), t = fl32(s * inv_temperature) is b4r_score_dist's, u = fl32((double) t - row_lse[r]) its
// query_logp (u = t without row_lse).  A party's allowed set is the intersection of its members' sets minus the vetoed items (some
// member's u < min_member_util); its aggregate a(p, j) is the fma chain over the members (additive), the minimum or the maximum.
//
// Launches per group of parties that fits the scratch:
//   1. sweep   grid (tile of 16 row slots) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h, staged as in
//              b4r_rank_full.hip (table rows through LDS in k-blocks of 16 floats, once for all 16 slots; 2 ids x 16 slots of accumulators per thread).  A template on MP, the
//              smallest of {1, 2, 4, 8, 16} that holds the M members: a tile is 16 / MP parties of MP slots, so the reduction over a
//              party's members runs over statically indexed registers of one thread.  The party's not-allowed bitmap is the OR of its
//              members' (LDS atomicOr).  Each thread is left with 4 x 16 / MP aggregates; per party the chunk's best min(K, 1024) go
//              to scratch by b4r_rank_full's radix select on the unique 48-bit key (score key << 16 | 1023 - local id).
//   2. merge   one workgroup per party: the same select on (score key << 32 | ~id) over all chunks' candidates, the order of the K
//              survivors by counting; party_n = the sum of the chunks' allowed counts.
//   3. util    (only when member_util is asked for) one thread per (party, place, member): u by the scalar chain.
// No floating-point atomics; LDS integer atomics only place or count, and the outputs do not depend on their order.
#include <algorithm>
#include <cmath>

#include "b4r_common.h"
#include "b4r_catalogue_tile.h"

namespace {

// b4r_score_dist's scalar t: the k-ordered fp32 fma chain (the contract), + bias (NULL: + 0.0f), one multiply by scale (NULL:
// none), one by inv_t
__device__ __forceinline__ float joint_row_t(const float* h, const float* e, const float* bias, const float* scale, int64_t j, int H,
                                             float inv_t) {
  float acc = 0.f;
  for (int k = 0; k < H; ++k) acc = __builtin_fmaf(h[k], e[k], acc);
  float s = acc + (bias ? bias[j] : 0.f);
  if (scale) s = s * scale[j];
  return s * inv_t;
}

// ---- 1. sweep: (tile of TILE_G row slots = TILE_G / MP parties) x (chunk of TILE_CH ids) ---------------------------------------------------
struct JointArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude;
  const uint32_t* allow; const int32_t* row_filter;   // [n_filters][ceil(V / 32)], [R] or NULL
  const double* row_lse;                              // [R] or NULL
  const int32_t* party_rows; const float* member_weight;   // [NP, M]
  float* c_score; int32_t* c_id; int32_t* c_cnt; int32_t* c_n;   // [n][nch][cap], [n][nch]
  int64_t p0;
  float inv_t, min_util;
  int hidden_ld, H, V, lo, E, R, M, mode, n, nch, cap, n_filters;
};

// the reduction over the MP slots of party pp for one id: false when a present member vetoes the id
template <int MP, int MODE>
__device__ __forceinline__ bool joint_reduce(const float (&acc)[TILE_G], int pp, float b, float sc, bool scaled, float inv_t, bool has_lse,
                                             const double* s_lse, const float* s_w, uint32_t present, float min_util, float& out) {
  float agg = MODE == B4R_JOINT_ADDITIVE ? 0.f : (MODE == B4R_JOINT_LEAST_MISERY ? INFINITY : -INFINITY);
  bool veto = false;
#pragma unroll
  for (int m = 0; m < MP; ++m) {
    const int g = pp * MP + m;
    float s = acc[g] + b;
    if (scaled) s = s * sc;
    const float t = s * inv_t;
    const float u = has_lse ? (float)((double)t - s_lse[g]) : t;
    if ((present >> g) & 1u) {
      veto |= u < min_util;
      if (MODE == B4R_JOINT_ADDITIVE) agg = __builtin_fmaf(s_w[g], u, agg);
      else if (MODE == B4R_JOINT_LEAST_MISERY) agg = u < agg ? u : agg;   // equal values (-0.0 and +0.0): the earlier member's bits
      else agg = u > agg ? u : agg;
    }
  }
  out = agg;
  return !veto;
}

template <int MP>
__global__ __launch_bounds__(TILE_T, 2) void joint_sweep_kernel(JointArgs a) {
  constexpr int NPT = TILE_G / MP;   // parties per tile
  __shared__ float tile[TILE_IPT * TILE_T * (TILE_KB + 1)];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[NPT][TILE_CH / 32];
  __shared__ uint32_t hist[NPT][256];
  __shared__ uint32_t part[NPT][16];
  __shared__ Sel st[NPT];
  __shared__ uint32_t s_cnt[NPT], s_kmin[NPT], s_kmax[NPT], s_out[NPT];
  __shared__ int64_t s_hoff[TILE_G], s_row[TILE_G];
  __shared__ double s_lse[TILE_G];
  __shared__ float s_w[TILE_G];
  __shared__ uint32_t s_present, s_bad, s_live;
  __shared__ int s_alldone;

  const int tid = threadIdx.x, lane = tid & 63;
  const int lp0 = blockIdx.x * NPT;   // first party of the tile, within the group
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const int H = a.H;

  if (tid == 0) { s_present = 0u; s_bad = 0u; }
  for (int i = tid; i < NPT * (TILE_CH / 32); i += TILE_T) (&bits[0][0])[i] = 0u;
  __syncthreads();
  if (tid < TILE_G) {
    const int pp = tid / MP, m = tid - pp * MP;
    const int lp = lp0 + pp;
    int64_t r = -1;
    if (lp < a.n && m < a.M) {
      const int32_t pr = a.party_rows[(a.p0 + lp) * a.M + m];
      if (pr >= 0 && pr < a.R) r = pr;
    }
    int64_t hoff = -1;
    double lse = 0.0;
    float w = 1.0f;
    if (r >= 0) {
      const int64_t hr = a.hidden_row ? a.hidden_row[r] : r;
      hoff = hr >= 0 ? hr * a.hidden_ld : -1;
      if (a.row_lse) lse = a.row_lse[r];
      if (a.member_weight) w = a.member_weight[(a.p0 + lp) * a.M + m];
      atomicOr(&s_present, 1u << tid);
      // a member that can be served nothing (no hidden row, or an empty distribution) empties its party
      if (hoff < 0 || !(lse > -INFINITY)) atomicOr(&s_bad, 1u << pp);
    }
    s_row[tid] = r; s_hoff[tid] = hoff; s_lse[tid] = lse; s_w[tid] = w;
  }
  if (tid < NPT) { s_cnt[tid] = 0; s_out[tid] = 0; s_kmin[tid] = 0xFFFFFFFFu; s_kmax[tid] = 0u; }
  __syncthreads();
  // bit set = not ranked for the party: the OR over its members of the complement of the member's filter words of this chunk ...
  if (a.allow) {
    const int64_t W = ((int64_t)a.V + 31) >> 5;
    for (int i = tid; i < TILE_G * (TILE_CH / 32); i += TILE_T) {
      const int g = i / (TILE_CH / 32), w = i - g * (TILE_CH / 32);
      const int64_t r = s_row[g];
      const int64_t wi = (c0 >> 5) + w;
      if (r < 0 || wi >= W) continue;
      const int32_t f = a.row_filter ? a.row_filter[r] : 0;
      if (f >= 0 && f < a.n_filters) {
        const uint32_t word = ~a.allow[(int64_t)f * W + wi];
        if (word) atomicOr(&bits[g / MP][w], word);
      }
    }
  }
  // ... and of the member's excluded ids
  if (a.E > 0) {
    for (int f = tid; f < TILE_G * a.E; f += TILE_T) {
      const int g = f / a.E, e = f - g * a.E;
      const int64_t r = s_row[g];
      if (r < 0) continue;
      const int64_t id = a.exclude[r * (int64_t)a.E + e];
      if (id >= c0 && id < c0 + TILE_CH) {
        const int l = (int)(id - c0);
        atomicOr(&bits[g / MP][l >> 5], 1u << (l & 31));
      }
    }
  }
  if (tid == 0) {
    uint32_t live = 0u;
#pragma unroll
    for (int pp = 0; pp < NPT; ++pp) {
      const uint32_t members = (s_present >> (pp * MP)) & ((1u << MP) - 1u);
      if (members && !((s_bad >> pp) & 1u)) live |= 1u << pp;
    }
    s_live = live;
  }

  // ---- aggregates: raw fp32 bits in registers, NOT_ALLOWED where the id is not ranked for the party -----------------------------
  uint32_t raw[TILE_Q][NPT];
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
      __syncthreads();   // the previous block is consumed (and, the first time, the bitmap and s_live are complete)
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
    const uint32_t present = s_present, live = s_live;
    const bool has_lse = a.row_lse != nullptr, scaled = a.scale != nullptr;
#pragma unroll
    for (int ii = 0; ii < TILE_IPT; ++ii) {
      const int q = ps * TILE_IPT + ii;
      const int l = q * TILE_T + tid;
      const int64_t j = c0 + l;
      const bool inb = j >= a.lo && j < a.V;
      const float b = (a.bias && inb) ? a.bias[j] : 0.f;
      const float sc = (scaled && inb) ? a.scale[j] : 1.f;
#pragma unroll
      for (int pp = 0; pp < NPT; ++pp) {
        const bool ex = (bits[pp][l >> 5] >> (l & 31)) & 1u;
        bool ok = inb && ((live >> pp) & 1u) && !ex;
        float agg;
        if (a.mode == B4R_JOINT_ADDITIVE)
          ok &= joint_reduce<MP, B4R_JOINT_ADDITIVE>(acc[ii], pp, b, sc, scaled, a.inv_t, has_lse, s_lse, s_w, present, a.min_util, agg);
        else if (a.mode == B4R_JOINT_LEAST_MISERY)
          ok &= joint_reduce<MP, B4R_JOINT_LEAST_MISERY>(acc[ii], pp, b, sc, scaled, a.inv_t, has_lse, s_lse, s_w, present, a.min_util, agg);
        else
          ok &= joint_reduce<MP, B4R_JOINT_MOST_PLEASURE>(acc[ii], pp, b, sc, scaled, a.inv_t, has_lse, s_lse, s_w, present, a.min_util, agg);
        raw[q][pp] = ok ? __builtin_bit_cast(uint32_t, agg) : NOT_ALLOWED;
      }
    }
  }

  // ---- per party: allowed count, key range -------------------------------------------------------------------------------------
#pragma unroll
  for (int pp = 0; pp < NPT; ++pp) {
    uint32_t cnt = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (raw[q][pp] == NOT_ALLOWED) continue;
      const uint32_t k = score_key_bits(raw[q][pp]);
      cnt += 1;
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    cnt = wave_sum_u32(cnt);
    kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
    if (lane == 0) { atomicAdd(&s_cnt[pp], cnt); atomicMin(&s_kmin[pp], kmin); atomicMax(&s_kmax[pp], kmax); }
  }
  __syncthreads();
  if (tid < NPT) {
    const int n = lp0 + tid < a.n ? (int)s_cnt[tid] : 0;
    sel_init(st[tid], n, min(a.cap, n), s_kmin[tid], s_kmax[tid]);
  }
  if (tid == 0) s_alldone = 0;

  // ---- radix select over (score key << 16 | TILE_CH-1 - local id) ----------------------------------------------------------------
  for (int pass = 0; pass < 6; ++pass) {
    __syncthreads();
    if (tid == 0) {
      int all = 1;
      for (int pp = 0; pp < NPT; ++pp) all &= st[pp].done;
      s_alldone = all;
    }
    for (int i = tid; i < NPT * 256; i += TILE_T) (&hist[0][0])[i] = 0u;
    __syncthreads();
    if (s_alldone) break;
#pragma unroll
    for (int pp = 0; pp < NPT; ++pp) {
      const Sel s = st[pp];
      if (s.done) continue;
      const int nb = sel_nb(s, 48), sh = 48 - s.hi - nb;
#pragma unroll
      for (int q = 0; q < TILE_Q; ++q) {
        if (raw[q][pp] == NOT_ALLOWED) continue;
        const uint64_t key = ((uint64_t)score_key_bits(raw[q][pp]) << 16) | (uint64_t)(TILE_CH - 1 - (q * TILE_T + tid));
        if (sel_match(s, key, 48)) atomicAdd(&hist[pp][(key >> sh) & ((1u << nb) - 1u)], 1u);
      }
    }
    __syncthreads();
    const int pp = tid >> 4, qq = tid & 15;
    const bool mine_on = pp < NPT && !st[pp < NPT ? pp : 0].done;
    const Sel mine = st[pp < NPT ? pp : 0];
    if (mine_on) sel_part(hist[pp], part[pp], qq);
    __syncthreads();
    if (mine_on) sel_advance(mine, st[pp], hist[pp], part[pp], qq, 48);
  }
  __syncthreads();

  // ---- emit the selected ids of each party (any order: the merge orders them) -------------------------------------------------
#pragma unroll
  for (int pp = 0; pp < NPT; ++pp) {
    const Sel s = st[pp];
    if (!s.take || !s.done) continue;
    const int64_t base = ((int64_t)(lp0 + pp) * a.nch + chunk) * a.cap;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (raw[q][pp] == NOT_ALLOWED) continue;
      const int l = q * TILE_T + tid;
      const uint64_t key = ((uint64_t)score_key_bits(raw[q][pp]) << 16) | (uint64_t)(TILE_CH - 1 - l);
      if (key < s.thr) continue;
      const uint32_t slot = atomicAdd(&s_out[pp], 1u);
      if (slot < (uint32_t)a.cap) {
        a.c_score[base + slot] = __builtin_bit_cast(float, raw[q][pp]);
        a.c_id[base + slot] = (int32_t)(c0 + l);
      }
    }
  }
  __syncthreads();
  if (tid < NPT && lp0 + tid < a.n) {
    const int64_t o = (int64_t)(lp0 + tid) * a.nch + chunk;
    a.c_cnt[o] = (int32_t)min(s_out[tid], (uint32_t)a.cap);
    a.c_n[o] = (int32_t)s_cnt[tid];
  }
}

// ---- 2. merge: one workgroup per party ------------------------------------------------------------------------------------------
struct JointMergeArgs {
  const float* c_score; const int32_t* c_id; const int32_t* c_cnt; const int32_t* c_n;
  int64_t* ids; float* topk_scores; int32_t* party_n;   // ids: [n, K] of the group (topk_ids + p0 * K, or scratch), or NULL
  int64_t p0;
  int nch, cap, K;
};

__global__ __launch_bounds__(TILE_T) void joint_merge_kernel(JointMergeArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t part[16];
  __shared__ Sel st;
  __shared__ uint32_t s_n, s_kmin, s_kmax, s_out, s_all;
  __shared__ uint64_t sel_key[SEL_K_MAX];
  __shared__ float sel_val[SEL_K_MAX];
  const MergeSel L{hist, part, st, s_n, s_kmin, s_kmax, s_out, &s_all, sel_key, sel_val};
  const int lp = blockIdx.x;
  const int64_t p = a.p0 + lp;
  const int64_t row = (int64_t)lp * a.nch;
  const int m = merge_select<TILE_T>(L, a.c_score, a.c_id, a.c_cnt, a.c_n, row, a.nch, a.cap, a.K);
  merge_order<TILE_T>(L, m, a.K, [&](int pos, int64_t id, float score) {
    if (a.ids) a.ids[(int64_t)lp * a.K + pos] = id;
    if (a.topk_scores) a.topk_scores[p * a.K + pos] = score;
  });
  if (threadIdx.x == 0 && a.party_n) a.party_n[p] = (int32_t)s_all;
}

// ---- 3. member utilities: one thread per (party, place, member) ----------------------------------------------------------------
struct JointUtilArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const double* row_lse; const int32_t* party_rows;
  const int64_t* ids;   // [n, K] of the group
  float* member_util;   // [NP, K, M]
  int64_t p0;
  float inv_t;
  int hidden_ld, H, V, lo, R, M, n, K;
};

__global__ __launch_bounds__(TILE_T) void joint_util_kernel(JointUtilArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TILE_T + threadIdx.x;
  const int64_t per = (int64_t)a.K * a.M;
  if (i >= (int64_t)a.n * per) return;
  const int lp = (int)(i / per);
  const int64_t rest = i - (int64_t)lp * per;
  const int place = (int)(rest / a.M), m = (int)(rest - (int64_t)place * a.M);
  const int64_t p = a.p0 + lp;
  const int64_t q = a.ids[(int64_t)lp * a.K + place];
  const int32_t r = a.party_rows[p * a.M + m];
  float out = -INFINITY;
  if (q >= a.lo && q < a.V && r >= 0 && r < a.R) {
    const int64_t hr = a.hidden_row ? a.hidden_row[r] : (int64_t)r;
    if (hr >= 0) {
      const float t = joint_row_t(a.hidden + hr * a.hidden_ld, a.table + q * a.H, a.bias, a.scale, q, a.H, a.inv_t);
      out = a.row_lse ? (float)((double)t - a.row_lse[r]) : t;
    }
  }
  a.member_util[p * per + rest] = out;
}

// scores, ids of the chunks' candidates | their counts, the allowed counts | the ordered ids of the party (what the util launch reads)
int64_t joint_party_bytes(int32_t V, int32_t K) { return tile_chunks_of(V) * (tile_cap_of(K) * 8 + 8) + (int64_t)K * 8; }
int joint_mp_of(int32_t M) { return M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 16; }

using JointSweepFn = void (*)(JointArgs);
JointSweepFn joint_sweep_instance(int mp) {
  switch (mp) {
    case 1: return joint_sweep_kernel<1>;
    case 2: return joint_sweep_kernel<2>;
    case 4: return joint_sweep_kernel<4>;
    case 8: return joint_sweep_kernel<8>;
    default: return joint_sweep_kernel<16>;
  }
}

}  // namespace

extern "C" int64_t b4r_rank_joint_scratch_bytes(int32_t NP, int32_t M, int32_t V, int32_t K) {
  if (NP <= 0 || M < 1 || M > TILE_G || V <= 0 || K < 0 || K > SEL_K_MAX) return 0;
  return (int64_t)NP * joint_party_bytes(V, K) + 64;   // + room for the 16-byte alignment of the regions
}

extern "C" int b4r_rank_joint(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                              int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E,
                              const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter, const float* item_scale,
                              float inv_temperature, const double* row_lse, const int32_t* party_rows, int32_t NP, int32_t M,
                              const float* member_weight, int32_t mode, float min_member_util, int32_t K, int64_t* topk_ids,
                              float* topk_scores, int32_t* party_n, float* member_util, void* scratch, int64_t scratch_bytes,
                              b4r_stream_t stream) {
  const char* what = "b4r_rank_joint";
  B4R_CHECK_ARG(R >= 0 && NP >= 0 && K >= 0 && K <= SEL_K_MAX && E >= 0 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, NP = %d, K = %d in [0, %d], E = %d, first_item = %d)", what, R, NP, K, SEL_K_MAX, E, first_item);
  B4R_CHECK_ARG(M >= 1 && M <= TILE_G, B4R_E_SHAPE, "%s: M = %d members per party must lie in [1, %d]", what, M, TILE_G);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d)", what, H, hidden_ld, V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  B4R_CHECK_ARG(mode == B4R_JOINT_ADDITIVE || mode == B4R_JOINT_LEAST_MISERY || mode == B4R_JOINT_MOST_PLEASURE, B4R_E_BADARG,
                "%s: unknown mode %d", what, mode);
  B4R_CHECK_ARG(std::isfinite(inv_temperature) && inv_temperature > 0.f, B4R_E_BADARG,
                "%s: inv_temperature = %g must be finite and > 0", what, (double)inv_temperature);
  B4R_CHECK_ARG(!std::isnan(min_member_util), B4R_E_BADARG, "%s: min_member_util is NaN", what);
  if (NP == 0 || K == 0) return B4R_OK;
  B4R_CHECK_ARG(hidden && table && party_rows, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int nch = (int)tile_chunks_of(V);
  B4R_CHECK_ARG(nch <= 65535, B4R_E_SHAPE, "%s: V = %d is too large", what, V);
  const int mp = joint_mp_of(M);
  const int npt = TILE_G / mp;   // parties per tile
  const int64_t per_party = joint_party_bytes(V, K);
  const int64_t group = tile_group_of(scratch, scratch_bytes, per_party, NP, npt);   // whole tiles
  B4R_CHECK_ARG(group >= std::min<int64_t>(NP, npt), B4R_E_NOMEM,
                "%s: scratch of %lld bytes is too small: %lld bytes per party, %d parties at least (b4r_rank_joint_scratch_bytes)", what,
                (long long)scratch_bytes, (long long)per_party, std::min<int32_t>(NP, npt));
  const int cap = (int)tile_cap_of(K);
  int64_t* s_ids = reinterpret_cast<int64_t*>(tile_scratch_base(scratch));
  float* c_score = reinterpret_cast<float*>(s_ids + group * K);
  int32_t* c_id = reinterpret_cast<int32_t*>(c_score + group * nch * cap);
  int32_t* c_cnt = c_id + group * nch * cap;
  int32_t* c_n = c_cnt + group * nch;
  hipStream_t s = (hipStream_t)stream;
  const JointSweepFn sweep = joint_sweep_instance(mp);
  for (int64_t p0 = 0; p0 < NP; p0 += group) {
    const int n = (int)std::min<int64_t>(group, NP - p0);
    JointArgs sa{hidden, hidden_row, table, bias, item_scale, exclude, allow_bits, row_filter, row_lse, party_rows, member_weight,
                 c_score, c_id, c_cnt, c_n, p0, inv_temperature, min_member_util, hidden_ld, H, V, first_item, E, R, M, mode, n, nch, cap,
                 n_filters};
    hipLaunchKernelGGL(sweep, dim3(b4r_cdiv(n, npt), nch), dim3(TILE_T), 0, s, sa);
    int64_t* ids = topk_ids ? topk_ids + p0 * K : (member_util ? s_ids : nullptr);
    JointMergeArgs ma{c_score, c_id, c_cnt, c_n, ids, topk_scores, party_n, p0, nch, cap, K};
    hipLaunchKernelGGL(joint_merge_kernel, dim3(n), dim3(TILE_T), 0, s, ma);
    if (member_util) {
      JointUtilArgs ua{hidden, hidden_row, table, bias, item_scale, row_lse, party_rows, ids, member_util, p0, inv_temperature,
                       hidden_ld, H, V, first_item, R, M, n, K};
      hipLaunchKernelGGL(joint_util_kernel, dim3(b4r_cdiv((int64_t)n * K * M, TILE_T)), dim3(TILE_T), 0, s, ua);
    }
  }
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
