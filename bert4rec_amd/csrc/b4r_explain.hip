// Occlusion explanations (include/b4r.h: b4r_occlude_rows, b4r_attribution_select): the device-side logic between the forwards of
// "which history items drove this recommendation".  The log probabilities come from the existing sweep (b4r_score_dist); the two
// kernels here build the batch rows with one history unit removed and pick, per explained item, the units whose removal costs the
// most, so that the call reads nothing back to the host between its launches.
//
//   occlude_rows_kernel        one workgroup of 256 threads per output row, thread p owns position p of the row (L <= 256).  The kept
//                              history tokens are compacted by a prefix count: one ballot per wave, the wave totals through LDS (one
//                              exchange, which also carries "a more recent position has the same label").
//   attribution_select_kernel  one workgroup of 256 threads per (user, tile of 16 explained items).  The W <= 256 deltas of every
//                              item of the tile go into LDS as order-preserving images (0 marks a dead entry); every entry counts
//                              the entries that come before it in (delta descending, w ascending) and, when that count is below m,
//                              writes itself there.  The order is strict, so every output cell has one writer.
//
// No atomics, no floating-point reduction: the bits do not depend on the launch.  Both entry points check every argument before
// the launch and only enqueue.
#include <cmath>

#include "b4r_common.h"
#include "b4r_wave.h"   // order_image

namespace {

constexpr int RT = 256;        // threads per workgroup (4 waves), both kernels
constexpr int OC_MAX_L = 256;  // one thread per position
constexpr int AS_MAX_W = 256;
constexpr int AS_MAX_K = 1024;
constexpr int AS_TILE = 16;    // explained items per workgroup
constexpr int AS_LD = AS_MAX_W + 1;   // row stride of the image tile: rows of one wave fall into different banks

struct OccludeArgs {
  const int64_t* tokens_in; const int32_t* len_in; const int32_t* labels;
  int64_t* tokens_out; int64_t* mask_out; int32_t* len_out; int64_t* positions_out; int32_t* live_out; int32_t* unit_pos_out;
  int64_t* unit_item_out; int32_t* unit_label_out; int32_t* removed_out;
  int64_t mask_id;
  int L, P, V, w0, Wc;
};

__device__ __forceinline__ int label_of(const int32_t* labels, int64_t tok, int V) {
  return (labels && tok >= 0 && tok < V) ? labels[tok] : -1;
}

__global__ __launch_bounds__(RT) void occlude_rows_kernel(OccludeArgs a) {
  __shared__ int s_kept[RT / 64];
  __shared__ int s_dup[RT / 64];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int64_t u = n / a.Wc;
  const int c = (int)(n - u * a.Wc);
  int len = a.len_in[u];
  len = len < 1 ? 1 : (len > a.L ? a.L : len);
  const int64_t* src = a.tokens_in + u * a.L;
  // p = len - 2 - (w0 + c) without overflow: w0 + c may exceed int32 only past every history
  const int64_t p64 = (int64_t)len - 2 - ((int64_t)a.w0 + c);
  const int p = p64 < 0 ? -1 : (int)p64;                     // p <= L - 2
  const int64_t tok = tid < a.L ? src[tid] : (int64_t)0;
  const int64_t tok_p = p >= 0 ? src[p] : (int64_t)-1;      // uniform over the workgroup
  const int g_p = p >= 0 ? label_of(a.labels, tok_p, a.V) : -1;
  const bool hist = tid <= len - 2;                          // a history position of the row (len - 2 < L)
  bool gone;                                                 // the position is removed, given that the row is live
  if (a.labels) gone = hist && label_of(a.labels, tok, a.V) == g_p;
  else gone = tid == p;
  const bool keep = hist && !gone;
  const uint64_t keep_b = __ballot(keep);
  const uint64_t dup_b = __ballot(gone && tid > p);          // group mode: a more recent occurrence of the label
  if ((tid & 63) == 0) {
    s_kept[tid >> 6] = __popcll(keep_b);
    s_dup[tid >> 6] = dup_b != 0 ? 1 : 0;
  }
  __syncthreads();
  int before = 0, kept = 0, dup = 0;
  for (int w = 0; w < RT / 64; ++w) {
    const int k = s_kept[w];
    before += w < (tid >> 6) ? k : 0;
    kept += k;
    dup |= s_dup[w];
  }
  before += __popcll(keep_b & ((1ull << (tid & 63)) - 1ull));
  const bool live = p >= 0 && (a.labels == nullptr || (g_p >= 0 && dup == 0));
  const int len_o = live ? kept + 1 : len;
  int64_t* dst = a.tokens_out + n * a.L;
  if (tid < a.L) {
    if (!live) {
      dst[tid] = tok;
    } else {
      if (keep) dst[before] = tok;                           // before <= tid, before < kept
      if (tid >= kept) dst[tid] = tid == kept ? a.mask_id : (int64_t)0;
    }
    a.mask_out[n * a.L + tid] = tid < len_o ? 1 : 0;
  }
  for (int q = tid; q < a.P; q += RT) a.positions_out[n * a.P + q] = q == 0 ? (int64_t)(len_o - 1) : (int64_t)0;
  if (tid == 0) {
    a.len_out[n] = len_o;
    a.live_out[n] = live ? 1 : 0;
    if (a.unit_pos_out) a.unit_pos_out[n] = live ? p : -1;
    if (a.unit_item_out) a.unit_item_out[n] = live ? tok_p : (int64_t)-1;
    if (a.unit_label_out) a.unit_label_out[n] = live ? g_p : -1;    // item mode: g_p is -1
    if (a.removed_out) a.removed_out[n] = live ? len - 1 - kept : 0;
  }
}

struct SelectArgs {
  const float* base_logp; const float* occ_logp; const int32_t* live;
  int32_t* out_w; float* out_delta;
  int W, K, m, tiles;
};

__global__ __launch_bounds__(RT) void attribution_select_kernel(SelectArgs a) {
  __shared__ uint32_t s_img[AS_TILE * AS_LD];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x / a.tiles;
  const int i0 = (int)(blockIdx.x - u * a.tiles) * AS_TILE;
  const int nt = a.K - i0 < AS_TILE ? a.K - i0 : AS_TILE;    // explained items of this tile, >= 1
  const int n = nt * a.W;                                    // <= 4096
  // load: consecutive threads take consecutive items of one occluded row
  for (int e = tid; e < n; e += RT) {
    const int w = e / nt, ii = e - w * nt;
    const float b = a.base_logp[u * a.K + i0 + ii];
    const float o = a.occ_logp[(u * a.W + w) * a.K + i0 + ii];
    const bool ok = a.live[u * a.W + w] != 0 && b > -INFINITY && o > -INFINITY;
    s_img[ii * AS_LD + w] = ok ? order_image(b - o) : 0u;
  }
  __syncthreads();
  // count: consecutive threads take consecutive w of one item
  for (int e = tid; e < n; e += RT) {
    const int ii = e / a.W, w = e - ii * a.W;
    const uint32_t* row = s_img + ii * AS_LD;
    const uint32_t ki = row[w];
    int pos = 0, n_live = 0;
    for (int j = 0; j < a.W; ++j) {
      const uint32_t kj = row[j];
      n_live += kj != 0u ? 1 : 0;
      pos += (kj > ki || (kj == ki && j < w)) ? 1 : 0;
    }
    const int64_t o = (u * a.K + i0 + ii) * a.m;
    if (ki != 0u && pos < a.m) {                             // a live entry: pos < n_live
      if (a.out_w) a.out_w[o + pos] = w;
      if (a.out_delta) a.out_delta[o + pos] = a.base_logp[u * a.K + i0 + ii] - a.occ_logp[(u * a.W + w) * a.K + i0 + ii];
    }
    if (w < a.m && w >= n_live) {                            // m <= W: thread w fills cell w of the tail
      if (a.out_w) a.out_w[o + w] = -1;
      if (a.out_delta) a.out_delta[o + w] = -INFINITY;
    }
  }
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

extern "C" int b4r_occlude_rows(const int64_t* tokens_in, const int32_t* len_in, const int32_t* labels, int32_t U, int32_t L, int32_t P,
                                int32_t V, int64_t mask_id, int32_t w0, int32_t Wc, int64_t* tokens_out, int64_t* input_mask_out,
                                int32_t* len_out, int64_t* positions_out, int32_t* live_out, int32_t* unit_pos_out,
                                int64_t* unit_item_out, int32_t* unit_label_out, int32_t* removed_out, b4r_stream_t stream) {
  const char* what = "b4r_occlude_rows";
  B4R_CHECK_ARG(U >= 0 && L >= 2 && L <= OC_MAX_L && P >= 1 && V >= 1, B4R_E_SHAPE,
                "%s: bad shape (U = %d >= 0, L = %d in [2, %d], P = %d >= 1, V = %d >= 1)", what, U, L, OC_MAX_L, P, V);
  B4R_CHECK_ARG(w0 >= 0 && Wc >= 1 && (int64_t)U * Wc <= INT32_MAX, B4R_E_SHAPE,
                "%s: bad chunk (w0 = %d >= 0, Wc = %d >= 1, U * Wc = %lld rows <= 2^31 - 1)", what, w0, Wc, (long long)U * Wc);
  if (U == 0) return B4R_OK;
  B4R_CHECK_ARG(tokens_in && len_in && tokens_out && input_mask_out && len_out && positions_out && live_out, B4R_E_BADARG,
                "%s: null argument", what);
  const int64_t ni = U, no = (int64_t)U * Wc, tb = ni * L * 8;
  B4R_CHECK_ARG(!overlaps(tokens_out, no * L * 8, tokens_in, tb) && !overlaps(input_mask_out, no * L * 8, tokens_in, tb) &&
                    !overlaps(len_out, no * 4, tokens_in, tb) && !overlaps(positions_out, no * P * 8, tokens_in, tb) &&
                    !overlaps(live_out, no * 4, tokens_in, tb) && !overlaps(unit_pos_out, no * 4, tokens_in, tb) &&
                    !overlaps(unit_item_out, no * 8, tokens_in, tb) && !overlaps(unit_label_out, no * 4, tokens_in, tb) &&
                    !overlaps(removed_out, no * 4, tokens_in, tb) && !overlaps(len_out, no * 4, len_in, ni * 4),
                B4R_E_BADARG, "%s: an output overlaps tokens_in or len_in (every user row is read by Wc workgroups)", what);
  OccludeArgs oa{tokens_in, len_in, labels, tokens_out, input_mask_out, len_out, positions_out, live_out, unit_pos_out, unit_item_out,
                 unit_label_out, removed_out, mask_id, L, P, V, w0, Wc};
  hipLaunchKernelGGL(occlude_rows_kernel, dim3((unsigned)no), dim3(RT), 0, (hipStream_t)stream, oa);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int b4r_attribution_select(const float* base_logp, const float* occ_logp, const int32_t* live, int32_t U, int32_t W, int32_t K,
                                      int32_t m, int32_t* out_w, float* out_delta, b4r_stream_t stream) {
  const char* what = "b4r_attribution_select";
  B4R_CHECK_ARG(U >= 0 && W >= 1 && W <= AS_MAX_W && K >= 1 && K <= AS_MAX_K && m >= 1 && m <= W, B4R_E_SHAPE,
                "%s: bad shape (U = %d >= 0, W = %d in [1, %d], K = %d in [1, %d], m = %d in [1, W])", what, U, W, AS_MAX_W, K, AS_MAX_K, m);
  const int tiles = (K + AS_TILE - 1) / AS_TILE;
  B4R_CHECK_ARG((int64_t)U * tiles <= INT32_MAX, B4R_E_SHAPE, "%s: U * ceil(K / %d) = %lld workgroups exceed 2^31 - 1", what, AS_TILE,
                (long long)U * tiles);
  if (U == 0) return B4R_OK;
  B4R_CHECK_ARG(base_logp && occ_logp && live, B4R_E_BADARG, "%s: null argument", what);
  SelectArgs sa{base_logp, occ_logp, live, out_w, out_delta, W, K, m, tiles};
  hipLaunchKernelGGL(attribution_select_kernel, dim3((unsigned)((int64_t)U * tiles)), dim3(RT), 0, (hipStream_t)stream, sa);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
