// Beyond-accuracy metrics of recommendation lists, on the device: intra-list distance, novelty, hit position, item exposure.
//
// Serves  BERT4RecModel.list_metrics_tensor, Recommender.list_quality and BERT4RecEvaluator(list_k=...)  (the lists are b4r_rank_full's
//                                                          top K or b4r_rerank_diverse's picks; the evaluator's sums stay on the device
//                                                          and are read once per evaluate(), as with b4r_rank_metrics)
//
// Contract (include/b4r.h, b4r_list_metrics; restated on the CPU in tests/list_metrics_ref.py): the distance of a live pair p < p' is
// fl32(1.0f - sim(c = item at p', q = item at p)) with b4r_rerank_diverse's sim (b4r_cosine_chain.h: the earlier position is the query),
// the subtraction rounded on its own; distances and item weights enter the sums as q30(x) = (int64) rint(x * 2^30), so every per-row
// sum is an integer and does not depend on the order of its terms.
//
// Two launches (three without item_rnorm: b4r_item_rnorm_launch, b4r_cosine_chain.h, fills it first):
//   list_metrics_kernel<NPT>  one 256-thread workgroup per list; thread tid owns the positions tid, tid + 256, ... (NPT = 1, 2 or 4).
//      Loop over the query position p: qhat = table[q] * rnorm[q] to LDS (two barriers per p), then every thread walks the table rows
//      of its live positions p' > p with 16-byte loads in ascending k -- the inner step of mmr_kernel (b4r_rerank.hip).  Per-thread int64
//      partial sums, reduced once at the end by shuffles and LDS.  exposure: one 64-bit integer atomic add per live entry.
//   list_fold_kernel          one workgroup: thread t adds the per-row terms of rows t, t + 256, ... in ascending order, a fixed tree over
//      the 256 partial sums follows: the double sums are bitwise reproducible from run to run, as b4r_rank_metrics' are.
// No float atomics anywhere.
#include "b4r_common.h"
#include "b4r_internal.h"
#include "b4r_cosine_chain.h"
#include "b4r_wave.h"

namespace {

constexpr int LT = 256;           // threads per workgroup
constexpr int LK_MAX = 1024;      // longest list
constexpr int LW_MAX = 4096;      // largest table width
static_assert(LK_MAX <= 4 * LT, "at most 4 positions per thread");

// fl32(1 - sim): rounded on its own (contracted with the product that forms sim, the compiler's default, it would be an ulp off)
__device__ __forceinline__ float distance_of(float sim) {
#pragma clang fp contract(off)
  return 1.0f - sim;
}
// (int64) rint(x * 2^30): the product is exact in fp32 (a power of two; |x| < 2^20 by the contract), rint rounds ties to even
__device__ __forceinline__ int64_t q30(float x) { return (int64_t)rintf(x * 1073741824.0f); }

struct ListArgs {
  const float* table; const float* rnorm;
  const int64_t* list_ids; const int64_t* gt; const float* item_weight;
  int32_t* row_n; int64_t* row_dist; int64_t* row_nov; int32_t* hit_pos;
  int64_t* exposure;
  int width, V, K, first_item;
};

template <int NPT>
__global__ __launch_bounds__(LT) void list_metrics_kernel(ListArgs a) {
  __shared__ __attribute__((aligned(16))) float qhat[LW_MAX];
  __shared__ int32_t s_id[LK_MAX];          // the item of every position, -1: not live
  __shared__ int64_t s_dist[LT / 64], s_nov[LT / 64];
  __shared__ int32_t s_n[LT / 64], s_hit[LT / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, width = a.width;
  const int64_t r = blockIdx.x;
  const int64_t* ids = a.list_ids + r * K;

  // the ground truth this row looks for; -1: none (no id equals it: a live id is >= 0)
  int64_t want = -1;
  if (a.gt) {
    const int64_t g = a.gt[r];
    if (g >= a.first_item && g < a.V) want = g;
  }

  // ---- the thread's positions: live = id in [0, V) -----------------------------------------------------------------------------
  bool live[NPT];
  const float* row[NPT];
  float rn[NPT];
  int n = 0, hit = 0x7fffffff;
  int64_t nov = 0;
#pragma unroll
  for (int i = 0; i < NPT; ++i) {
    const int p = i * LT + tid;
    int32_t id = -1;
    if (p < K) {
      const int64_t j = ids[p];
      if (j >= 0 && j < a.V) id = (int32_t)j;
      s_id[p] = id;
    }
    live[i] = id >= 0;
    row[i] = a.table + (int64_t)(live[i] ? id : 0) * width;   // (not live: never read)
    rn[i] = live[i] ? a.rnorm[id] : 0.f;
    if (live[i]) {
      ++n;
      if (id == want) hit = min(hit, p + 1);
      if (a.item_weight) nov += q30(a.item_weight[id]);
      if (a.exposure) atomicAdd(reinterpret_cast<unsigned long long*>(a.exposure + id), 1ull);
    }
  }
  __syncthreads();   // s_id is complete

  // ---- sum over live pairs p < p' of q30(1 - sim(item at p', item at p)) ---------------------------------------------------------
  int64_t dist = 0;
  for (int p = 0; p + 1 < K; ++p) {
    const int q = s_id[p];                  // the same for every thread
    if (q < 0) continue;
    __syncthreads();                        // the chains of the previous query have read qhat
    b4r_stage_qhat(qhat, a.table, a.rnorm, q, width, tid, LT);
    __syncthreads();
    bool later[NPT];
    bool any = false;
#pragma unroll
    for (int i = 0; i < NPT; ++i) { later[i] = live[i] && i * LT + tid > p; any |= later[i]; }
    if (any) {
      float acc[NPT];
      b4r_cosine_chains<NPT>(qhat, row, later, width, acc);
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        if (later[i]) dist += q30(distance_of(b4r_cosine_close(acc[i], rn[i])));
      }
    }
  }

  // ---- the row's sums: shuffles inside a wave, LDS across the four (integer adds: any order is exact) ----------------------------
  dist = wave_sum_i64(dist); nov = wave_sum_i64(nov); n = wave_sum_i32(n); hit = wave_min_i32(hit);
  if (lane == 0) { s_dist[wave] = dist; s_nov[wave] = nov; s_n[wave] = n; s_hit[wave] = hit; }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < LT / 64; ++w) { dist += s_dist[w]; nov += s_nov[w]; n += s_n[w]; hit = min(hit, s_hit[w]); }
    if (a.row_n) a.row_n[r] = n;
    if (a.row_dist) a.row_dist[r] = dist;
    if (a.row_nov) a.row_nov[r] = nov;
    if (a.hit_pos) a.hit_pos[r] = hit == 0x7fffffff ? 0 : hit;
  }
}

// sums[0] += sum over rows with n >= 2 of (dist / 2^30) / (n (n - 1) / 2), sums[1] += sum over rows with n >= 1 of (nov / 2^30) / n,
// counts += the numbers of such rows.  One workgroup, fixed summation order.
__global__ __launch_bounds__(LT) void list_fold_kernel(const int32_t* row_n, const int64_t* row_dist, const int64_t* row_nov, int R,
                                                       double* sums, int64_t* counts) {
  __shared__ double red[2][LT];
  __shared__ int64_t cnt[2][LT];
  const int tid = threadIdx.x;
  double s_ild = 0.0, s_nov = 0.0;
  int64_t c2 = 0, c1 = 0;
  for (int i = tid; i < R; i += LT) {
    const int64_t n = row_n[i];
    if (n >= 2) { s_ild += ((double)row_dist[i] * (1.0 / 1073741824.0)) / (double)(n * (n - 1) / 2); ++c2; }
    if (n >= 1) { s_nov += ((double)row_nov[i] * (1.0 / 1073741824.0)) / (double)n; ++c1; }
  }
  red[0][tid] = s_ild; red[1][tid] = s_nov; cnt[0][tid] = c2; cnt[1][tid] = c1;
  __syncthreads();
  for (int o = LT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o];
      cnt[0][tid] += cnt[0][tid + o]; cnt[1][tid] += cnt[1][tid + o];
    }
    __syncthreads();
  }
  if (tid < 2) {
    if (sums) sums[tid] += red[tid][0];
    if (counts) counts[tid] += cnt[tid][0];
  }
}

// scratch regions, each a multiple of 16 bytes: rnorm [V] fp32 | n [R] int32 | dist [R] int64 | nov [R] int64
int64_t rnorm_bytes(int32_t V) { return b4r_align16((int64_t)V * 4); }
int64_t rows_bytes(int32_t R) { return b4r_align16((int64_t)R * 4) + 2 * b4r_align16((int64_t)R * 8); }

}  // namespace

extern "C" int64_t b4r_list_metrics_scratch_bytes(int32_t R, int32_t K, int32_t V) {
  if (R <= 0 || K < 1 || K > LK_MAX || V <= 0) return 0;
  return rnorm_bytes(V) + rows_bytes(R);   // of a 16-byte aligned scratch (an unaligned one loses the bytes up to the boundary)
}

extern "C" int b4r_list_metrics(const float* table, int32_t ld, int32_t width, int32_t V, int32_t first_item, const float* item_rnorm,
                                const int64_t* list_ids, int32_t R, int32_t K, const int64_t* gt, const float* item_weight,
                                int32_t* row_n, int64_t* row_dist, int64_t* row_nov, int32_t* hit_pos, int64_t* exposure, double* sums,
                                int64_t* counts, void* scratch, int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_list_metrics";
  B4R_CHECK_ARG(R >= 0 && K >= 1 && K <= LK_MAX, B4R_E_SHAPE, "%s: bad shape (R = %d, K = %d in [1, %d])", what, R, K, LK_MAX);
  B4R_CHECK_ARG(width > 0 && width % 4 == 0 && width <= LW_MAX && ld == width && V > 0, B4R_E_SHAPE,
                "%s: bad shape (width = %d: a multiple of 4 up to %d, ld = %d: must equal width, V = %d)", what, width, LW_MAX, ld, V);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(table && list_ids, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  // the fold reads the per-row integers: from the caller's outputs where all three are given, else from the scratch
  const bool fold = sums != nullptr || counts != nullptr;
  const bool stage_rows = fold && !(row_n && row_dist && row_nov);
  char* base = nullptr;
  if (!item_rnorm || stage_rows) {
    base = b4r_scratch_carve(scratch, scratch_bytes, rnorm_bytes(V) + rows_bytes(R));
    B4R_CHECK_ARG(base, B4R_E_NOMEM,
                  "%s: scratch of %lld bytes is too small for rnorm [%d] and the sums of %d rows (b4r_list_metrics_scratch_bytes)", what,
                  (long long)scratch_bytes, V, R);
  }
  const float* rnorm = item_rnorm;
  if (!rnorm) {
    float* rn = reinterpret_cast<float*>(base);
    b4r_item_rnorm_launch(table, width, V, rn, s);
    rnorm = rn;
  }
  if (stage_rows) {   // the outputs the caller did not ask for
    char* rows = base + rnorm_bytes(V);
    if (!row_n) row_n = reinterpret_cast<int32_t*>(rows);
    if (!row_dist) row_dist = reinterpret_cast<int64_t*>(rows + b4r_align16((int64_t)R * 4));
    if (!row_nov) row_nov = reinterpret_cast<int64_t*>(rows + b4r_align16((int64_t)R * 4) + b4r_align16((int64_t)R * 8));
  }
  ListArgs a{table, rnorm, list_ids, gt, item_weight, row_n, row_dist, row_nov, hit_pos, exposure, width, V, K, first_item};
  if (K <= LT) hipLaunchKernelGGL(list_metrics_kernel<1>, dim3(R), dim3(LT), 0, s, a);
  else if (K <= 2 * LT) hipLaunchKernelGGL(list_metrics_kernel<2>, dim3(R), dim3(LT), 0, s, a);
  else hipLaunchKernelGGL(list_metrics_kernel<4>, dim3(R), dim3(LT), 0, s, a);
  if (fold) hipLaunchKernelGGL(list_fold_kernel, dim3(1), dim3(LT), 0, s, row_n, row_dist, row_nov, R, sums, counts);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
