// Calibrated re-ranking of a candidate pool (Steck, "Calibrated Recommendations", RecSys 2018): the K returned items are picked one by
// one, each the best trade of relevance against the Kullback-Leibler divergence of a per-row target distribution over the item
// groups (categories) from the group shares of the list so far.
//
// Serves  BERT4RecModel.recommend_tensor(calibrate=...)  b4r_rerank_calibrated
// (the pool is b4r_rank_full's top M of the row; the target is b4r_group_mass's masses of the row, its history's label counts, or
// any int64 [R, G] the caller brings)
//
// Contract (include/b4r.h; restated on the CPU in tests/calibrated_ref.py): live and rel are b4r_rerank_quota's; p_g =
// fl64(mass_g / T) with T the integer sum of the row's masses; at the step that makes pick number n + 1 group g has the gain
// fl32(p_g (ln qt(g, n_g + 1, n + 1) - ln qt(g, n_g, n + 1))) with qt(g, c, m) = fl64(fl64(fl64((1 - alpha) c) / m) + fl64(alpha p_g))
// and ln = b4r_xln, every operation rounded on its own; val = fl32(fl32(fl32(1 - lambda) rel) + fl32(lambda gain)); the open entry
// with the largest val wins, ties go to the lower pool position.
//
// The form is b4r_rerank.hip's: one launch, one 256-thread workgroup per pool row; thread tid owns the pool entries tid, tid + 256,
// ... (NPT = 1, 2 or 4 of them) and the groups tid, tid + 256, ... (up to 4: G <= 1024).  rel, the labels and the open flags of the
// entries and p_g, fl64(alpha p_g) and n_g of the groups stay in registers for all K steps.  A step is two barriers:
//   1. every thread forms the fp32 gains of its groups (all of them change with the denominator n + 1) and writes them to LDS
//                                                                                                                      -- barrier --
//   2. every thread reads the gains of its entries' groups, forms val of its open entries and the key (open bit | ordered integer
//      image of val | M - 1 - p), unique per entry; the waves reduce it by shuffles in a fixed order and leave one key each in LDS
//                                                                                                                      -- barrier --
//   3. every thread reads the four wave keys (LDS broadcasts): the largest names the winner p.  Its owner writes the step's outputs;
//      every thread reads the winner's label from LDS (the labels of the pool entries sit there beside their ids) and the owner of
//      that group raises n_g.  Nothing is published, so no third barrier: the gains of step t + 1 are written after barrier 2 of
//      step t, behind every read of step t's.
// After the K steps the owners form the miscalibration's terms from the final counts and one thread adds them in ascending g.
// No atomics, no scratch; bitwise reproducible.
#include "b4r_common.h"
#include "b4r_wave.h"

namespace {

constexpr int DT = 256;           // threads per workgroup
constexpr int DM_MAX = 1024;      // largest pool
constexpr int DG_MAX = 1024;      // most groups
constexpr int GPT = DG_MAX / DT;  // groups per thread
constexpr int POS_BITS = 10;      // M - 1 - p < 1024
static_assert(DM_MAX <= (1 << POS_BITS), "the pool position takes the low bits of the key");
static_assert(DM_MAX <= 4 * DT, "at most 4 entries per thread");

// fl32(fl32(lr * rel) + fl32(la * gain)): the products and the sum are rounded separately (see mmr_value in b4r_rerank.hip)
__device__ __forceinline__ float cal_value(float lr, float rel, float la, float gain) {
#pragma clang fp contract(off)
  const float x = lr * rel;
  const float y = la * gain;
  return x + y;
}
__device__ __forceinline__ float cal_one_minus(float la) {
#pragma clang fp contract(off)
  return 1.0f - la;
}
// qt(g, c, m) = fl64(fl64(fl64(A * c) / m) + ap) with ap = fl64(alpha * p_g): the smoothed share of a group with c of m picks
__device__ __forceinline__ double cal_share(double A, int c, int m, double ap) {
#pragma clang fp contract(off)
  const double x = A * (double)c;
  const double y = x / (double)m;
  return y + ap;
}
// the gain of a group with c of the m - 1 picks so far: fl32(fl64(p * fl64(ln qt(c + 1, m) - ln qt(c, m))))
__device__ __forceinline__ float cal_gain(double p, double A, double ap, int c, int m) {
#pragma clang fp contract(off)
  const double hi = b4r_xln(cal_share(A, c + 1, m, ap));
  const double lo = b4r_xln(cal_share(A, c, m, ap));
  const double d = hi - lo;
  return (float)(p * d);
}
// the group's term of KL(p || qt) with c of the m picks: fl64(p * fl64(ln p - ln qt(c, m)))
__device__ __forceinline__ double cal_kl_term(double p, double A, double ap, int c, int m) {
#pragma clang fp contract(off)
  const double d = b4r_xln(p) - b4r_xln(cal_share(A, c, m, ap));
  return p * d;
}
__device__ __forceinline__ double cal_ratio(int64_t mass, int64_t T, double alpha, double& ap) {
#pragma clang fp contract(off)
  const double p = (double)mass / (double)T;
  ap = alpha * p;
  return p;
}

struct CalArgs {
  const int64_t* pool_ids; const float* pool_scores;
  const int32_t* item_group; const int64_t* target_mass;
  int64_t* out_ids; float* out_scores; float* out_value; int32_t* out_pos; double* out_kl;
  double alpha;
  float lambda;
  int V, M, K, G;
};

template <int NPT>
__global__ __launch_bounds__(DT) void calibrated_kernel(CalArgs a) {
  __shared__ int32_t s_id[DM_MAX];          // the item of every pool entry, -1: not live
  __shared__ int32_t s_lab[DM_MAX];         // its label in [0, G), -1: in no group (or not live)
  __shared__ float s_gain[DG_MAX];          // the step's gain of every group
  __shared__ double s_term[DG_MAX];         // the miscalibration's terms
  __shared__ uint64_t s_wkey[DT / 64];
  __shared__ uint32_t s_wmin[DT / 64], s_wmax[DT / 64];
  __shared__ int64_t s_wsum[DT / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = a.K, G = a.G;
  const int64_t r = blockIdx.x;
  const int64_t* ids = a.pool_ids + r * M;
  const float* scores = a.pool_scores + r * M;
  const int64_t* target = a.target_mass + r * G;

  // ---- the thread's entries: live = id in [0, V) and a finite score ---------------------------------------------------------
  float rel[NPT], val[NPT];
  int32_t lab[NPT];
  bool open[NPT];
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int p = i * DT + tid;
    int32_t id = -1;
    float s = 0.f;
    lab[i] = -1;
    if (p < M) {
      const int64_t j = ids[p];
      s = scores[p];
      const bool finite = (__builtin_bit_cast(uint32_t, s) & 0x7F800000u) != 0x7F800000u;
      if (j >= 0 && j < a.V && finite) {
        id = (int32_t)j;
        const int32_t g = a.item_group[id];   // (read at live ids only)
        if (g >= 0 && g < G) lab[i] = g;      // any other value: the item is in no group
      }
      s_id[p] = id;
      s_lab[p] = lab[i];
    }
    open[i] = id >= 0;
    if (open[i]) {
      const uint32_t k = score_key(s);
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    rel[i] = s;   // the score, until s_min and s_max are known
    val[i] = 0.f;
  }

  // ---- the thread's groups: the clamped mass, and T = their exact integer sum over the row -------------------------------------
  int64_t mass[GPT];
  int64_t T = 0;
#pragma unroll
  for (int u = 0; u < GPT; ++u) {
    const int g = u * DT + tid;
    mass[u] = 0;
    if (g < G) {
      const int64_t v = target[g];
      mass[u] = v > 0 ? v : 0;
    }
    T += mass[u];
  }
  kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
  T = wave_sum_i64(T);
  if (lane == 0) { s_wmin[wave] = kmin; s_wmax[wave] = kmax; s_wsum[wave] = T; }
  __syncthreads();
  T = 0;
#pragma unroll
  for (int w = 0; w < DT / 64; ++w) { kmin = min(kmin, s_wmin[w]); kmax = max(kmax, s_wmax[w]); T += s_wsum[w]; }
  {
    // rel = (s - s_min) / (s_max - s_min), 1 when all live scores are equal (no live entry: nothing is open, rel is not read)
    const float smin = score_key_value(kmin), smax = score_key_value(kmax);
    const float span = smax - smin;
#pragma unroll
    for (int i = 0; i < NPT; ++i) rel[i] = smax == smin ? 1.0f : (rel[i] - smin) / span;
  }
  const double alpha = a.alpha;
  const double A = 1.0 - alpha;
  double pg[GPT], apg[GPT];   // p_g and fl64(alpha * p_g); p_g = 0: the group has no gain and no term
  int32_t ng[GPT];            // the picks so far with label g
#pragma unroll
  for (int u = 0; u < GPT; ++u) {
    pg[u] = 0.0; apg[u] = 0.0; ng[u] = 0;
    if (T > 0 && mass[u] > 0) pg[u] = cal_ratio(mass[u], T, alpha, apg[u]);
  }

  const float la = a.lambda, lr = cal_one_minus(la);
  int filled = 0;
  for (int t = 0; t < K; ++t) {
    // ---- 1. the gains of pick number t + 1 (every earlier step made a pick: n = t) ----------------------------------------------
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
      const int g = u * DT + tid;
      if (g < G) s_gain[g] = pg[u] > 0.0 ? cal_gain(pg[u], A, apg[u], ng[u], t + 1) : 0.0f;
    }
    __syncthreads();

    // ---- 2. the best open entry: largest val, then the lowest position ------------------------------------------------------------
    uint64_t best = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      const float gain = lab[i] >= 0 ? s_gain[lab[i]] : 0.0f;
      val[i] = cal_value(lr, rel[i], la, gain);
      const int p = i * DT + tid;
      const uint64_t key = (1ull << (32 + POS_BITS)) | ((uint64_t)score_key(val[i]) << POS_BITS) | (uint64_t)(M - 1 - p);
      if (open[i] && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) s_wkey[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DT / 64; ++w) best = s_wkey[w] > best ? s_wkey[w] : best;
    if (best == 0) break;   // no open entry is left (the same for every thread)

    // ---- 3. the winner: its outputs, and its group's count ------------------------------------------------------------------------
    const int p = M - 1 - (int)(best & ((1u << POS_BITS) - 1u));   // in [0, M): the key of an open entry
    if (tid == (p & (DT - 1))) {
      const int turn = p / DT;
      float v = val[0];
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        if (i == turn) { v = val[i]; open[i] = false; }
      }
      const int64_t o = r * K + t;
      if (a.out_ids) a.out_ids[o] = s_id[p];   // in [0, V): the entry is live
      if (a.out_scores) a.out_scores[o] = scores[p];
      if (a.out_value) a.out_value[o] = v;
      if (a.out_pos) a.out_pos[o] = p;
    }
    const int wl = s_lab[p];   // LDS broadcast
#pragma unroll
    for (int u = 0; u < GPT; ++u) ng[u] += (u * DT + tid == wl) ? 1 : 0;
    filled = t + 1;
  }
  for (int t = filled + tid; t < K; t += DT) {
    const int64_t o = r * K + t;
    if (a.out_ids) a.out_ids[o] = -1;
    if (a.out_scores) a.out_scores[o] = -INFINITY;
    if (a.out_value) a.out_value[o] = -INFINITY;
    if (a.out_pos) a.out_pos[o] = -1;
  }

  // ---- the miscalibration KL(p || qt) of the final list: the terms of the groups with p_g > 0, added in ascending g -----------------
  if (a.out_kl) {
    const bool defined = T > 0 && filled > 0;
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
      const int g = u * DT + tid;
      // (a group with p_g = 0 has no term: the +0.0 in its place leaves every partial sum, which starts at +0.0, as it is)
      if (g < G) s_term[g] = (defined && pg[u] > 0.0) ? cal_kl_term(pg[u], A, apg[u], ng[u], filled) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
      double kl = __builtin_nan("");
      if (defined) {
        kl = 0.0;
        for (int g = 0; g < G; ++g) kl += s_term[g];
      }
      a.out_kl[r] = kl;
    }
  }
}

}  // namespace

extern "C" int b4r_rerank_calibrated(const int64_t* pool_ids, const float* pool_scores, int32_t R, int32_t M, int32_t K, int32_t V,
                                     const int32_t* item_group, int32_t G, const int64_t* target_mass, float lambda, double alpha,
                                     int64_t* out_ids, float* out_scores, float* out_value, int32_t* out_pos, double* out_kl,
                                     b4r_stream_t stream) {
  const char* what = "b4r_rerank_calibrated";
  B4R_CHECK_ARG(R >= 0 && M >= 1 && M <= DM_MAX && K >= 0 && K <= M && V > 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, M = %d in [1, %d], K = %d in [0, M], V = %d)", what, R, M, DM_MAX, K, V);
  B4R_CHECK_ARG(G >= 1 && G <= DG_MAX, B4R_E_SHAPE, "%s: G = %d groups must lie in [1, %d]", what, G, DG_MAX);
  B4R_CHECK_ARG(lambda >= 0.0f && lambda <= 1.0f, B4R_E_BADARG, "%s: lambda = %g does not lie in [0, 1]", what, (double)lambda);
  B4R_CHECK_ARG(alpha > 0.0 && alpha < 1.0, B4R_E_BADARG, "%s: alpha = %g does not lie in (0, 1)", what, alpha);
  B4R_CHECK_ARG(R == 0 || (pool_ids && pool_scores && item_group && target_mass), B4R_E_BADARG, "%s: null argument", what);
  const bool any_list = K > 0 && (out_ids || out_scores || out_value || out_pos);
  if (R == 0 || (!any_list && !out_kl)) return B4R_OK;
  CalArgs a{pool_ids, pool_scores, item_group, target_mass, out_ids, out_scores, out_value, out_pos, out_kl, alpha, lambda, V, M, K, G};
  hipStream_t s = (hipStream_t)stream;
  if (M <= DT) hipLaunchKernelGGL(calibrated_kernel<1>, dim3(R), dim3(DT), 0, s, a);
  else if (M <= 2 * DT) hipLaunchKernelGGL(calibrated_kernel<2>, dim3(R), dim3(DT), 0, s, a);
  else hipLaunchKernelGGL(calibrated_kernel<4>, dim3(R), dim3(DT), 0, s, a);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
