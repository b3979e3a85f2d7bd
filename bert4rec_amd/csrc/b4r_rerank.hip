// Diversity-aware re-ranking of a candidate pool: greedy Maximal Marginal Relevance (MMR) with cosine similarity in the item table,
// with or without category quotas (a pool entry also closes once a group it belongs to -- category, brand, artist, ... -- has given
// its cap of picks).
//
// Serves  BERT4RecModel.recommend_tensor(diversity=...)      b4r_rerank_diverse
//         BERT4RecModel.recommend_tensor(max_per_group=...)  b4r_rerank_quota
// (the pool is b4r_rank_full's top M of the row; the K returned items are picked one by one, each the best trade of relevance
// against similarity to the items already picked)
//
// Contract (include/b4r.h; restated on the CPU in tests/diverse_ref.py and tests/quota_ref.py): relevance is the pool score mapped to
// [0, 1]; sim(c, q) is b4r_item_neighbours' cosine with the picked item q as the query (k-ascending fp32 fma chain, no MFMA);
// mmr = fl32(fl32(lambda rel) - fl32(fl32(1 - lambda) pen)) with three separate roundings; ties go to the lower pool position.
// b4r_rerank_quota adds up to B4R_QUOTA_MAX quotas.  Quota a gives every item a group (or none) and every group a cap; left_a(c)
// starts at the cap of the group of entry c; a live entry with some left_a <= 0 is closed before step 0 (it still counts in s_min /
// s_max); a pick takes one from left_a of every still-open entry of the same group, and the entry closes at 0.  Without quotas the
// bits are b4r_rerank_diverse's.
//
// Both entry points are one kernel text, mmr_kernel<NPT, QUOTA>: the quota statements stand under `if constexpr (QUOTA)` and the
// six instances compile to what the two kernels written apart compiled to.
//
// One launch, one 256-thread workgroup per pool row; thread tid owns the pool entries tid, tid + 256, ... (NPT = 1, 2 or 4 of
// them).  rel, pen and the open (live, unpicked and not closed by a cap) flags stay in registers for all K steps, and with QUOTA
// so do n_quotas group ids and n_quotas remaining counts per entry.  A step is two barriers:
//   1. every thread forms mmr of its open entries and the key (open bit | ordered integer image of mmr | M - 1 - p), unique per
//      entry; the waves reduce it by shuffles in a fixed order and leave one key each in LDS                          -- barrier --
//   2. every thread reads the four wave keys (LDS broadcasts): the largest names the winner p.  Its owner writes the step's outputs
//      and, with QUOTA, publishes the winner's groups (it holds them in registers) in 16 bytes of LDS; all threads write
//      qhat = table[q] * rnorm[q] of the winner's item q to LDS                                                        -- barrier --
//   3a. (QUOTA) every thread compares the winner's groups with those of its open entries and closes the ones that ran out
//   3b. every thread walks the table rows of its open entries with 16-byte loads in ascending k against qhat (LDS broadcast reads,
//      one per four fmas and shared by the thread's NPT chains) and raises pen; an entry that is dead, picked or closed is skipped.
//      A pool row's M table rows are M * width * 4 bytes: at most 1 MB up to width 256, which stays in L2 over the K steps; a wider
//      table (the entry takes widths up to 4096: 16 MB at M = 1024) is streamed again from beyond L2 in each of the K steps.
// The loop carries chains, not tiles: nothing is staged but qhat.  No atomics; bitwise reproducible.
#include <type_traits>

#include "b4r_common.h"
#include "b4r_internal.h"
#include "b4r_cosine_chain.h"
#include "b4r_wave.h"

namespace {

constexpr int DT = 256;           // threads per workgroup
constexpr int DM_MAX = 1024;      // largest pool
constexpr int DW_MAX = 4096;      // largest table width
constexpr int POS_BITS = 10;      // M - 1 - p < 1024
constexpr int NQ_MAX = B4R_QUOTA_MAX;
static_assert(DM_MAX <= (1 << POS_BITS), "the pool position takes the low bits of the key");
static_assert(DM_MAX <= 4 * DT, "at most 4 entries per thread");
static_assert(NQ_MAX == 4, "the winner's groups are published as one 16-byte record");

// fl32(fl32(la * rel) - fl32(lb * pen)): the products and the difference are rounded separately (contracted to an FMA, the
// compiler's default, the value is an ulp off and two entries that tie by the contract no longer do)
__device__ __forceinline__ float mmr_value(float la, float rel, float lb, float pen) {
#pragma clang fp contract(off)
  const float x = la * rel;
  const float y = lb * pen;
  return x - y;
}
__device__ __forceinline__ float one_minus(float la) {
#pragma clang fp contract(off)
  return 1.0f - la;
}

// The kernel arguments of the two entry points.  QuotaArgs is RerankArgs with the quota members in between, as one flat struct:
// the member order is the layout of the kernel's argument segment.  Derived from RerankArgs (the quota members behind it) the
// quota instances keep their registers but not their instruction sequence.
struct RerankArgs {
  const float* table; const float* rnorm;
  const int64_t* pool_ids; const float* pool_scores;
  int64_t* out_ids; float* out_scores; float* out_mmr;
  float lambda;
  int width, V, M, K;
};
struct QuotaArgs {
  const float* table; const float* rnorm;
  const int64_t* pool_ids; const float* pool_scores;
  int64_t* out_ids; float* out_scores; float* out_mmr; int32_t* out_pos;
  const int32_t* item_group[NQ_MAX]; const int32_t* group_cap[NQ_MAX];
  int32_t n_groups[NQ_MAX], cap[NQ_MAX];
  float lambda;
  int width, V, M, K, nq;
};
template <bool QUOTA> using MmrArgs = std::conditional_t<QUOTA, QuotaArgs, RerankArgs>;

template <int NPT, bool QUOTA>
__global__ __launch_bounds__(DT) void mmr_kernel(MmrArgs<QUOTA> a) {
  constexpr int NQ = QUOTA ? NQ_MAX : 1;    // (without quotas the arrays of this size are never touched and vanish)
  __shared__ __attribute__((aligned(16))) float qhat[DW_MAX];
  __shared__ int32_t s_id[DM_MAX];          // the item of every pool entry, -1: not live
  __shared__ uint64_t s_wkey[DT / 64];
  __shared__ uint32_t s_wmin[DT / 64], s_wmax[DT / 64];
  __shared__ __attribute__((aligned(16))) int32_t s_wgrp[NQ];   // the groups of the step's winner, -1: none

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = a.K, width = a.width;
  int nq = 0;
  if constexpr (QUOTA) nq = a.nq;
  const int64_t r = blockIdx.x;
  const int64_t* ids = a.pool_ids + r * M;
  const float* scores = a.pool_scores + r * M;

  // ---- the thread's entries: live = id in [0, V) and a finite score ---------------------------------------------------------
  int32_t id[NPT];
  float rel[NPT], pen[NPT], mmr[NPT], rn[NPT];
  bool open[NPT];
  const float* row[NPT];
  int32_t grp[NPT][NQ], left[NPT][NQ];   // the entry's group under quota q (-1: none) and what that group may still give
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int p = i * DT + tid;
    id[i] = -1;
    float s = 0.f;
    if (p < M) {
      const int64_t j = ids[p];
      s = scores[p];
      const bool finite = (__builtin_bit_cast(uint32_t, s) & 0x7F800000u) != 0x7F800000u;
      if (j >= 0 && j < a.V && finite) id[i] = (int32_t)j;
      s_id[p] = id[i];
    }
    const bool live = id[i] >= 0;
    open[i] = live;
    if (live) {   // a live entry counts in s_min / s_max whether a cap closes it or not
      const uint32_t k = score_key(s);
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    if constexpr (QUOTA) {
#pragma unroll
      for (int q = 0; q < NQ_MAX; ++q) {
        grp[i][q] = -1;
        left[i][q] = 1;
        if (q < nq && live) {
          const int32_t g = a.item_group[q][id[i]];
          if (g >= 0 && g < a.n_groups[q]) {   // any other value: the item is in no group of this quota
            grp[i][q] = g;
            left[i][q] = a.group_cap[q] ? a.group_cap[q][g] : a.cap[q];
            if (left[i][q] <= 0) open[i] = false;   // closed at the start
          }
        }
      }
    }
    rel[i] = s;   // the score, until s_min and s_max are known
    pen[i] = 0.f;
    mmr[i] = 0.f;
    // (without quotas open[i] still equals `live` here and is read twice in its place: worded as `live`, or read once into a
    // local, the instances of 2 and 4 entries per thread compile to 66 and 72 registers instead of 54 and 80)
    row[i] = a.table + (int64_t)((QUOTA ? live : open[i]) ? id[i] : 0) * width;   // (not live: never read)
    rn[i] = (QUOTA ? live : open[i]) ? a.rnorm[id[i]] : 0.f;
  }
  kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
  if (lane == 0) { s_wmin[wave] = kmin; s_wmax[wave] = kmax; }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < DT / 64; ++w) { kmin = min(kmin, s_wmin[w]); kmax = max(kmax, s_wmax[w]); }
  {
    // rel = (s - s_min) / (s_max - s_min), 1 when all live scores are equal (no live entry: nothing is open, rel is not read)
    const float smin = score_key_value(kmin), smax = score_key_value(kmax);
    const float span = smax - smin;
#pragma unroll
    for (int i = 0; i < NPT; ++i) rel[i] = smax == smin ? 1.0f : (rel[i] - smin) / span;
  }

  const float la = a.lambda, lb = one_minus(la);
  int filled = 0;
  for (int t = 0; t < K; ++t) {
    // ---- 1. the best open entry: largest mmr, then the lowest position ----------------------------------------------------
    uint64_t best = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      mmr[i] = mmr_value(la, rel[i], lb, pen[i]);
      const int p = i * DT + tid;
      const uint64_t key = (1ull << (32 + POS_BITS)) | ((uint64_t)score_key(mmr[i]) << POS_BITS) | (uint64_t)(M - 1 - p);
      if (open[i] && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) s_wkey[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DT / 64; ++w) best = s_wkey[w] > best ? s_wkey[w] : best;
    if (best == 0) break;   // no open entry is left (the same for every thread)
    const int p = M - 1 - (int)(best & ((1u << POS_BITS) - 1u));   // in [0, M): the key of an open entry
    const int q = s_id[p];                                         // in [0, V): the entry is live
    if (tid == (p & (DT - 1))) {
      const int turn = p / DT;
      float m = mmr[0];
      int32_t wg[NQ];
      if constexpr (QUOTA) {
#pragma unroll
        for (int u = 0; u < NQ_MAX; ++u) wg[u] = grp[0][u];
      }
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        if (i == turn) {
          m = mmr[i]; open[i] = false;
          if constexpr (QUOTA) {
#pragma unroll
            for (int u = 0; u < NQ_MAX; ++u) wg[u] = grp[i][u];
          }
        }
      }
      if constexpr (QUOTA) {
#pragma unroll
        for (int u = 0; u < NQ_MAX; ++u) s_wgrp[u] = wg[u];
      }
      const int64_t o = r * K + t;
      if (a.out_ids) a.out_ids[o] = q;
      if (a.out_scores) a.out_scores[o] = scores[p];
      if (a.out_mmr) a.out_mmr[o] = m;
      if constexpr (QUOTA) {
        if (a.out_pos) a.out_pos[o] = p;
      }
    }
    filled = t + 1;
    if (filled == K) break;

    // ---- 2. the picked item as the cosine query -----------------------------------------------------------------------------
    b4r_stage_qhat(qhat, a.table, a.rnorm, q, width, tid, DT);
    __syncthreads();

    // ---- 3a. the pick counts against its groups: an open entry of the same group loses one and closes at 0 ---------------------
    bool any_open = false;
    if constexpr (QUOTA) {
#pragma unroll
      for (int u = 0; u < NQ_MAX; ++u) {
        if (u < nq) {
          const int32_t wg = s_wgrp[u];   // LDS broadcast
#pragma unroll
          for (int i = 0; i < NPT; ++i) {
            if (open[i] && wg >= 0 && grp[i][u] == wg) {
              left[i][u] -= 1;
              if (left[i][u] <= 0) open[i] = false;
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NPT; ++i) any_open |= open[i];

    // ---- 3b. pen = max over the picked q of sim(c, q) = fl32((chain_k(qhat[k] * table[c][k]) + 0.0f) * rnorm[c]) ----------------
    // (pen of an entry that is dead, picked or closed is never read again: only open entries walk their row)
    if (any_open) {
      // b4r_cosine_chains<NPT> (b4r_cosine_chain.h), written out: called as a function the loop costs this kernel 4 more registers
      // at 2 and 4 entries per thread and a wave of occupancy at 4
      float acc[NPT];
#pragma unroll
      for (int i = 0; i < NPT; ++i) acc[i] = 0.f;
#pragma unroll 4
      for (int k = 0; k < width; k += 4) {
        const f32x4 h = *reinterpret_cast<const f32x4*>(qhat + k);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
          if (!open[i]) continue;
          const f32x4 e = *reinterpret_cast<const f32x4*>(row[i] + k);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[i] = __builtin_fmaf(h[u], e[u], acc[i]);   // k-ordered fp32 fma chain (the contract)
        }
      }
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        const float sim = b4r_cosine_close(acc[i], rn[i]);
        pen[i] = (t == 0 || sim > pen[i]) ? sim : pen[i];   // the earlier value stays on equality
      }
    }
  }
  for (int t = filled + tid; t < K; t += DT) {
    const int64_t o = r * K + t;
    if (a.out_ids) a.out_ids[o] = -1;
    if (a.out_scores) a.out_scores[o] = -INFINITY;
    if (a.out_mmr) a.out_mmr[o] = -INFINITY;
    if constexpr (QUOTA) {
      if (a.out_pos) a.out_pos[o] = -1;
    }
  }
}

// ---- host: what both entry points check and do, `what` naming the entry point --------------------------------------------------
int64_t mmr_scratch_bytes(int32_t R, int32_t M, int32_t V) {
  if (R <= 0 || M <= 0 || M > DM_MAX || V <= 0) return 0;
  return b4r_align16((int64_t)V * 4) + 16;   // rnorm [V] + room for its 16-byte alignment
}

// the checks that come before an empty call returns (n_quotas: 0 for b4r_rerank_diverse)
int mmr_check(const char* what, int32_t ld, int32_t width, int32_t V, int32_t R, int32_t M, float lambda, int32_t K,
                    int32_t n_quotas) {
  B4R_CHECK_ARG(R >= 0 && M >= 1 && M <= DM_MAX && K >= 0 && K <= M, B4R_E_SHAPE, "%s: bad shape (R = %d, M = %d in [1, %d], K = %d in [0, M])",
                what, R, M, DM_MAX, K);
  B4R_CHECK_ARG(width > 0 && width % 4 == 0 && width <= DW_MAX && ld == width && V > 0, B4R_E_SHAPE,
                "%s: bad shape (width = %d: a multiple of 4 up to %d, ld = %d: must equal width, V = %d)", what, width, DW_MAX, ld, V);
  B4R_CHECK_ARG(n_quotas >= 0 && n_quotas <= NQ_MAX, B4R_E_SHAPE, "%s: n_quotas = %d does not lie in [0, %d]", what, n_quotas, NQ_MAX);
  B4R_CHECK_ARG(lambda >= 0.0f && lambda <= 1.0f, B4R_E_BADARG, "%s: lambda = %g does not lie in [0, 1]", what, (double)lambda);
  return B4R_OK;
}

// the rest of a call whose shape passed: a (rnorm = the caller's item_rnorm or NULL) is complete but for rnorm
template <bool QUOTA>
int mmr_launch(const char* what, MmrArgs<QUOTA> a, int32_t R, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (R == 0 || a.K == 0) return B4R_OK;
  B4R_CHECK_ARG(a.table && a.pool_ids && a.pool_scores, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(b4r_aligned16(a.table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  if (!a.rnorm) {
    float* rn = reinterpret_cast<float*>(b4r_scratch_carve(scratch, scratch_bytes, (int64_t)a.V * 4));
    B4R_CHECK_ARG(rn, B4R_E_NOMEM, "%s: scratch of %lld bytes is too small for rnorm [%d] (%s_scratch_bytes)", what,
                  (long long)scratch_bytes, a.V, what);
    b4r_item_rnorm_launch(a.table, a.width, a.V, rn, s);
    a.rnorm = rn;
  }
  if (a.M <= DT) hipLaunchKernelGGL((mmr_kernel<1, QUOTA>), dim3(R), dim3(DT), 0, s, a);
  else if (a.M <= 2 * DT) hipLaunchKernelGGL((mmr_kernel<2, QUOTA>), dim3(R), dim3(DT), 0, s, a);
  else hipLaunchKernelGGL((mmr_kernel<4, QUOTA>), dim3(R), dim3(DT), 0, s, a);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

}  // namespace

extern "C" int64_t b4r_rerank_diverse_scratch_bytes(int32_t R, int32_t M, int32_t V) { return mmr_scratch_bytes(R, M, V); }
extern "C" int64_t b4r_rerank_quota_scratch_bytes(int32_t R, int32_t M, int32_t V) { return mmr_scratch_bytes(R, M, V); }

extern "C" int b4r_rerank_diverse(const float* table, int32_t ld, int32_t width, int32_t V, const float* item_rnorm,
                                  const int64_t* pool_ids, const float* pool_scores, int32_t R, int32_t M, float lambda, int32_t K,
                                  int64_t* out_ids, float* out_scores, float* out_mmr, void* scratch, int64_t scratch_bytes,
                                  b4r_stream_t stream) {
  const char* what = "b4r_rerank_diverse";
  if (const int e = mmr_check(what, ld, width, V, R, M, lambda, K, 0)) return e;
  RerankArgs a{table, item_rnorm, pool_ids, pool_scores, out_ids, out_scores, out_mmr, lambda, width, V, M, K};
  return mmr_launch<false>(what, a, R, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int b4r_rerank_quota(const float* table, int32_t ld, int32_t width, int32_t V, const float* item_rnorm, const int64_t* pool_ids,
                                const float* pool_scores, int32_t R, int32_t M, float lambda, int32_t K, const b4r_item_quota* quotas,
                                int32_t n_quotas, int64_t* out_ids, float* out_scores, float* out_mmr, int32_t* out_pos, void* scratch,
                                int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_rerank_quota";
  if (const int e = mmr_check(what, ld, width, V, R, M, lambda, K, n_quotas)) return e;
  B4R_CHECK_ARG(n_quotas == 0 || quotas, B4R_E_BADARG, "%s: null quotas with n_quotas = %d", what, n_quotas);
  for (int q = 0; q < n_quotas; ++q)
    B4R_CHECK_ARG(quotas[q].item_group && quotas[q].n_groups >= 0, B4R_E_BADARG,
                  "%s: quota %d needs an item_group and n_groups >= 0 (item_group %s, n_groups = %d)", what, q,
                  quotas[q].item_group ? "given" : "null", quotas[q].n_groups);
  QuotaArgs a{};
  a.table = table; a.rnorm = item_rnorm; a.pool_ids = pool_ids; a.pool_scores = pool_scores;
  a.out_ids = out_ids; a.out_scores = out_scores; a.out_mmr = out_mmr; a.out_pos = out_pos;
  for (int q = 0; q < n_quotas; ++q) {
    a.item_group[q] = quotas[q].item_group; a.group_cap[q] = quotas[q].group_cap;
    a.n_groups[q] = quotas[q].n_groups; a.cap[q] = quotas[q].cap;
  }
  a.lambda = lambda; a.width = width; a.V = V; a.M = M; a.K = K; a.nq = n_quotas;
  return mmr_launch<true>(what, a, R, scratch, scratch_bytes, (hipStream_t)stream);
}
