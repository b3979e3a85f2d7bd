// Catalogue softmax of the ranked rows without an [R, V] score matrix: the normaliser (log-sum-exp), the entropy and the log
// probability of queried items, over the set of items each row could have been served (b4r_rank_full_ex's allowed set).
//
// Serves  calibrated recommendation  (a probability per returned item, a confidence figure per user, a temperature:
//                                     BERT4RecModel.score_distribution_tensor, recommend_tensor(return_distribution=True))
//         full-ranking evaluation    (negative log-likelihood / perplexity of the held-out item, mean entropy)
//
// Contract (include/b4r.h, b4r_score_dist): s(r, j) is b4r_rank_full_ex's score bit for bit (k-ascending fp32 fma chain + bias, one
// multiply by item_scale), t = fl32(s * inv_temperature), allowed(r) is b4r_rank_full_ex's set.
//
// Three launches per group of rows that fits the scratch:
//   1. sweep    grid (group of 16 rows) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h, staged as b4r_rank_full's sweep
//               stages its table rows (k-blocks of 16 floats through LDS, once for all 16 rows; 4 ids x 16 rows of t per thread
//               in registers).  Per (row, chunk): n_c = #allowed, m_c = max t, S_c = sum (double) e_j, W_c = sum (double) e_j (double) x_j with
//               x_j = fl32(t_j - m_c), e_j = expf(x_j).  The sums run in fp64 in a fixed order: a thread's 4 ids in ascending id,
//               the xor butterfly over the wave, the 4 waves in ascending order.
//   2. merge    one wave per row: m = max m_c; f_c = exp(m_c - m) in fp64; S = sum S_c f_c, W = sum (W_c + (m_c - m) S_c) f_c, each
//               lane over its chunks in ascending order, then the butterfly;  lse = m + log S, entropy = log S - W / S.
//   3. queries  one thread per (row, query): allowed(r) restated per id, t by the same chain, logp = fl32((double) t - lse).
// No floating-point atomics anywhere: two runs give the same bits.
#include <algorithm>
#include <cmath>

#include "b4r_common.h"
#include "b4r_catalogue_tile.h"

namespace {

constexpr int DW = TILE_T / 64;   // waves per workgroup
constexpr int DK_MAX = 1024;      // most queries per row

static_assert(TILE_G <= 32, "a row's allowed ids of one q are one bit of a 32-bit mask");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct DistArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude; const int64_t* gt;
  const uint32_t* allow; const int32_t* row_filter;   // [n_filters][ceil(V / 32)], [R] or NULL
  double* c_S; double* c_W; float* c_m; int32_t* c_n;   // [n][nch]
  int64_t r0;
  float inv_t;
  int hidden_ld, H, V, lo, E, n, nch, n_filters;
};

// ---- 1. sweep: (group of TILE_G rows) x (chunk of TILE_CH ids) -------------------------------------------------------------------------
__global__ __launch_bounds__(TILE_T, 2) void dist_sweep_kernel(DistArgs a) {
  __shared__ float tile[TILE_IPT * TILE_T * (TILE_KB + 1)];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[TILE_G][TILE_CH / 32];
  __shared__ int64_t s_hoff[TILE_G], s_gt[TILE_G];
  __shared__ float s_wm[TILE_G][DW];
  __shared__ int s_wn[TILE_G][DW];
  __shared__ double s_wS[TILE_G][DW], s_wW[TILE_G][DW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr0 = blockIdx.x * TILE_G;
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const int H = a.H;

  if (tid < TILE_G) tile_row_setup(tid, lr0, a.n, a.r0, a.hidden_row, a.hidden_ld, a.gt, s_hoff, s_gt);
  tile_row_bitmap(bits, a.allow != nullptr, a.allow, a.row_filter, a.n_filters, a.exclude, a.E, s_hoff, a.r0, lr0, a.n, a.V, c0);

  // ---- t = fl32(s * inv_temperature) in registers; okm[q] bit g: id q of this thread is allowed for row g --------------------
  float t[TILE_Q][TILE_G];
  uint32_t okm[TILE_Q];
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
      uint32_t m = 0u;
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) {
        const bool ex = (bits[g][l >> 5] >> (l & 31)) & 1u;
        const bool ok = inb && s_hoff[g] >= 0 && (!ex || j == s_gt[g]);
        float s = acc[ii][g] + b;
        if (a.scale) s = s * sc;
        t[q][g] = s * a.inv_t;
        m |= ok ? (1u << g) : 0u;
      }
      okm[q] = m;
    }
  }

  // ---- per (row, chunk): the count and the maximum ---------------------------------------------------------------------------
#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    float mx = -INFINITY;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      const bool ok = (okm[q] >> g) & 1u;
      cnt += __popcll(__ballot(ok));
      if (ok) mx = fmaxf(mx, t[q][g]);
    }
    mx = b4r_wave_max(mx);
    if (lane == 0) { s_wm[g][wave] = mx; s_wn[g][wave] = cnt; }
  }
  __syncthreads();

  // ---- per (row, chunk): S_c, W_c in fp64, a fixed order -------------------------------------------------------------------------
#pragma unroll
  for (int g = 0; g < TILE_G; ++g) {
    float mc = s_wm[g][0];
#pragma unroll
    for (int w = 1; w < DW; ++w) mc = fmaxf(mc, s_wm[g][w]);
    double S = 0.0, W = 0.0;
#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      if (!((okm[q] >> g) & 1u)) continue;
      const float x = t[q][g] - mc;
      const float e = expf(x);
      S += (double)e;
      if (e > 0.f) W += (double)e * (double)x;   // (e = 0 adds nothing, whatever x is)
    }
    S = wave_sum_f64(S);
    W = wave_sum_f64(W);
    if (lane == 0) { s_wS[g][wave] = S; s_wW[g][wave] = W; }
  }
  __syncthreads();
  if (tid < TILE_G && lr0 + tid < a.n) {
    const int64_t o = (int64_t)(lr0 + tid) * a.nch + chunk;
    float mc = s_wm[tid][0];
    int n = s_wn[tid][0];
    double S = s_wS[tid][0], W = s_wW[tid][0];
#pragma unroll
    for (int w = 1; w < DW; ++w) { mc = fmaxf(mc, s_wm[tid][w]); n += s_wn[tid][w]; S += s_wS[tid][w]; W += s_wW[tid][w]; }
    a.c_n[o] = n; a.c_m[o] = mc; a.c_S[o] = S; a.c_W[o] = W;
  }
}

// ---- 2. merge: one wave per row ------------------------------------------------------------------------------------------------
struct DistMergeArgs {
  const double* c_S; const double* c_W; const float* c_m; const int32_t* c_n;
  double* lse;   // [n] in scratch: what the query kernel reads
  int32_t* row_n; float* row_max; double* row_lse; double* row_entropy;
  int64_t r0;
  int nch;
};

__global__ __launch_bounds__(64) void dist_merge_kernel(DistMergeArgs a) {
  const int lane = threadIdx.x;
  const int lr = blockIdx.x;
  const int64_t r = a.r0 + lr;
  const int64_t o = (int64_t)lr * a.nch;
  int n = 0;
  float m = -INFINITY;
  for (int c = lane; c < a.nch; c += 64) {
    const int nc = a.c_n[o + c];
    if (nc > 0) { n += nc; m = fmaxf(m, a.c_m[o + c]); }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s, 64);
  m = b4r_wave_max(m);
  double S = 0.0, W = 0.0;
  for (int c = lane; c < a.nch; c += 64) {
    if (a.c_n[o + c] <= 0) continue;
    const double d = (double)a.c_m[o + c] - (double)m;
    const double f = exp(d);
    const double Sc = a.c_S[o + c];
    S += Sc * f;
    W += (a.c_W[o + c] + d * Sc) * f;
  }
  S = wave_sum_f64(S);
  W = wave_sum_f64(W);
  if (lane != 0) return;
  double lse = -INFINITY, ent = 0.0;
  if (n > 0) {
    const double logS = log(S);
    lse = (double)m + logS;
    ent = logS - W / S;
  } else {
    m = -INFINITY;
  }
  a.lse[lr] = lse;
  if (a.row_n) a.row_n[r] = n;
  if (a.row_max) a.row_max[r] = m;
  if (a.row_lse) a.row_lse[r] = lse;
  if (a.row_entropy) a.row_entropy[r] = ent;
}

// ---- 3. queries: one thread per (row, query) -----------------------------------------------------------------------------------
struct DistQueryArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude; const int64_t* gt;
  const uint32_t* allow; const int32_t* row_filter;
  const int64_t* query_ids; const double* lse; float* query_logp;
  int64_t r0;
  float inv_t;
  int hidden_ld, H, V, lo, E, n, K, n_filters;
};

__global__ __launch_bounds__(TILE_T) void dist_query_kernel(DistQueryArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TILE_T + threadIdx.x;
  if (i >= (int64_t)a.n * a.K) return;
  const int lr = (int)(i / a.K);
  const int64_t r = a.r0 + lr;
  const int64_t at = r * a.K + (i - (int64_t)lr * a.K);
  const int64_t q = a.query_ids[at];
  const int64_t hr = a.hidden_row ? a.hidden_row[r] : r;
  float out = -INFINITY;
  if (q >= a.lo && q < a.V && hr >= 0) {
    bool ok = true;
    if (a.allow) {
      const int32_t f = a.row_filter ? a.row_filter[r] : 0;
      const int64_t W = ((int64_t)a.V + 31) >> 5;
      if (f >= 0 && f < a.n_filters) ok = (a.allow[(int64_t)f * W + (q >> 5)] >> (q & 31)) & 1u;
    }
    for (int e = 0; ok && e < a.E; ++e) ok = a.exclude[r * a.E + e] != q;
    if (!ok && a.gt && a.gt[r] == q) ok = true;
    const double lse = a.lse[lr];
    if (ok && lse > -INFINITY) {
      const float t = row_score(a.hidden + hr * a.hidden_ld, a.table + q * a.H, a.bias, a.scale, q, a.H) * a.inv_t;
      out = (float)((double)t - lse);
    }
  }
  a.query_logp[at] = out;
}

int64_t dist_row_bytes(int32_t V) { return tile_chunks_of(V) * 24 + 8; }   // S, W (double), m (float), n (int32) per chunk | lse

}  // namespace

extern "C" int64_t b4r_score_dist_scratch_bytes(int32_t R, int32_t V) {
  if (R <= 0 || V <= 0) return 0;
  return (int64_t)R * dist_row_bytes(V) + 64;   // + room for the 16-byte alignment of the regions
}

extern "C" int b4r_score_dist(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                              int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E, const int64_t* gt,
                              const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter, const float* item_scale,
                              float inv_temperature, const int64_t* query_ids, int32_t K, int32_t* row_n, float* row_max,
                              double* row_lse, double* row_entropy, float* query_logp, void* scratch, int64_t scratch_bytes,
                              b4r_stream_t stream) {
  const char* what = "b4r_score_dist";
  B4R_CHECK_ARG(R >= 0 && K >= 0 && K <= DK_MAX && E >= 0 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (R = %d, K = %d in [0, %d], E = %d, first_item = %d)", what, R, K, DK_MAX, E, first_item);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d)", what, H, hidden_ld, V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  B4R_CHECK_ARG(std::isfinite(inv_temperature) && inv_temperature > 0.f, B4R_E_BADARG,
                "%s: inv_temperature = %g must be finite and > 0", what, (double)inv_temperature);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(hidden && table, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(K == 0 || !query_logp || query_ids, B4R_E_BADARG, "%s: query_ids is NULL with K = %d", what, K);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  const int64_t per_row = dist_row_bytes(V);
  const int64_t group = tile_group_of(scratch, scratch_bytes, per_row, R, TILE_G);   // whole sweep groups
  B4R_CHECK_ARG(group >= std::min<int64_t>(R, TILE_G), B4R_E_NOMEM,
                "%s: scratch of %lld bytes is too small: %lld bytes per row, %d rows at least (b4r_score_dist_scratch_bytes)", what,
                (long long)scratch_bytes, (long long)per_row, std::min<int32_t>(R, TILE_G));
  const int nch = (int)tile_chunks_of(V);
  B4R_CHECK_ARG(nch <= 65535, B4R_E_SHAPE, "%s: V = %d is too large", what, V);
  double* c_S = reinterpret_cast<double*>(tile_scratch_base(scratch));
  double* c_W = c_S + group * nch;
  double* lse = c_W + group * nch;
  float* c_m = reinterpret_cast<float*>(lse + group);
  int32_t* c_n = reinterpret_cast<int32_t*>(c_m + group * nch);
  hipStream_t s = (hipStream_t)stream;
  for (int64_t r0 = 0; r0 < R; r0 += group) {
    const int n = (int)std::min<int64_t>(group, R - r0);
    DistArgs sa{hidden, hidden_row, table, bias, item_scale, exclude, gt, allow_bits, row_filter, c_S, c_W, c_m, c_n, r0,
                inv_temperature, hidden_ld, H, V, first_item, E, n, nch, n_filters};
    hipLaunchKernelGGL(dist_sweep_kernel, dim3(b4r_cdiv(n, TILE_G), nch), dim3(TILE_T), 0, s, sa);
    DistMergeArgs ma{c_S, c_W, c_m, c_n, lse, row_n, row_max, row_lse, row_entropy, r0, nch};
    hipLaunchKernelGGL(dist_merge_kernel, dim3(n), dim3(64), 0, s, ma);
    if (K > 0 && query_logp) {
      DistQueryArgs qa{hidden, hidden_row, table, bias, item_scale, exclude, gt, allow_bits, row_filter, query_ids, lse, query_logp,
                       r0, inv_temperature, hidden_ld, H, V, first_item, E, n, K, n_filters};
      hipLaunchKernelGGL(dist_query_kernel, dim3(b4r_cdiv((int64_t)n * K, TILE_T)), dim3(TILE_T), 0, s, qa);
    }
  }
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
