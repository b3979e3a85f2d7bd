// Session store (include/b4r.h: b4r_history_append, b4r_history_batch): user histories that stay on the device between calls.  The
// state is the caller's: hist [U, C] int64, one ring of C items per user, and count [U] int64, the events accepted per user so far;
// the n-th accepted event of user u (0-based, over the user's life) lives at hist[u][n mod C].
//
//   history_plan_kernel    one thread per event, 256 events per workgroup.  The whole event list goes by in tiles of 256 keys (the
//                          user of an accepted event, -1 otherwise) through LDS; a thread counts the accepted events of its own user
//                          before and after its own index, reads count_old[u] and writes the event's plan to the scratch: the hist
//                          cell it stores to (or -1: a later event of the same call lands on that cell) and the count it leaves (or
//                          -1: it is not the user's last event of the call).  Reads count, writes scratch and accepted_out only.
//   history_commit_kernel  one thread per event: carry out the plan.  Reads the scratch and the events, writes hist and count only.
//                          Every hist cell and every count cell has at most one writer (the events of a user with after < C have
//                          pairwise different before mod C; one event per user has after == 0).
//   history_batch_kernel   one workgroup per requested row: the h most recent items out of the ring (two contiguous segments), the
//                          [MASK] placeholder, mask, length, position, weight and the exclusion list.
//
// No atomics: nothing depends on the order in which threads arrive, the bits do not depend on the launch.  The entry points check
// every argument before the launch and only enqueue.
#include "b4r_common.h"

namespace {

constexpr int HT = 256;                    // threads per workgroup (4 waves), all three kernels; the tile of the event list
constexpr int HIST_MAX_EVENTS = 65536;     // N
constexpr int HIST_MAX_CAPACITY = 4096;    // C
constexpr int HIST_MAX_LEN = 256;          // L

struct PlanArgs {
  const int64_t* count; const int32_t* ev_user; const int64_t* ev_item;
  int64_t* plan;                           // [N, 2]: the hist cell (flat index) or -1, the new count or -1
  int32_t* accepted_out;
  int64_t U, V, first_item;
  int C, N;
};

__global__ __launch_bounds__(HT) void history_plan_kernel(PlanArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t s_key[HT];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int n = tile * HT + tid;
  int32_t u = -1;
  if (n < a.N) {
    const int32_t eu = a.ev_user[n];
    const int64_t it = a.ev_item[n];
    if (eu >= 0 && eu < a.U && it >= a.first_item && it < a.V) u = eu;
  }
  const bool acc = u >= 0;
  int before = 0, after = 0;
  const int tiles = (a.N + HT - 1) / HT;
  for (int t = 0; t < tiles; ++t) {        // block-uniform trip count and branches: the barriers see whole workgroups
    int32_t key = u;
    if (t != tile) {
      const int m = t * HT + tid;
      key = -1;
      if (m < a.N) {
        const int32_t eu = a.ev_user[m];
        const int64_t it = a.ev_item[m];
        if (eu >= 0 && eu < a.U && it >= a.first_item && it < a.V) key = eu;
      }
    }
    s_key[tid] = key;
    __syncthreads();
    if (acc) {                             // an accepted u is >= 0 and never equals the -1 of a dropped or absent event
      const int4* s_key4 = reinterpret_cast<const int4*>(s_key);   // four keys per LDS read, the same address in every lane
      int same = 0;
      if (t == tile) {
        int lo = 0;
#pragma unroll 4
        for (int j = 0; j < HT / 4; ++j) {
          const int4 k = s_key4[j];
          const int h0 = k.x == u, h1 = k.y == u, h2 = k.z == u, h3 = k.w == u;
          same += h0 + h1 + h2 + h3;
          lo += (4 * j < tid ? h0 : 0) + (4 * j + 1 < tid ? h1 : 0) + (4 * j + 2 < tid ? h2 : 0) + (4 * j + 3 < tid ? h3 : 0);
        }
        before += lo;
        after += same - lo - 1;            // the event itself is one of `same`
      } else {
#pragma unroll 8
        for (int j = 0; j < HT / 4; ++j) {
          const int4 k = s_key4[j];
          same += (k.x == u) + (k.y == u) + (k.z == u) + (k.w == u);
        }
        if (t < tile) before += same; else after += same;
      }
    }
    __syncthreads();
  }
  if (n >= a.N) return;
  int64_t cell = -1, left = -1;
  if (acc) {
    const int64_t idx = a.count[u] + before;
    if (after < a.C) {
      int64_t pos = idx % a.C;
      if (pos < 0) pos += a.C;             // (a negative count is outside the contract; the cell stays inside the user's ring)
      cell = (int64_t)u * a.C + pos;
    }
    if (after == 0) left = idx + 1;
  }
  a.plan[2 * (int64_t)n] = cell;
  a.plan[2 * (int64_t)n + 1] = left;
  if (a.accepted_out) a.accepted_out[n] = acc ? 1 : 0;
}

__global__ __launch_bounds__(HT) void history_commit_kernel(const int64_t* plan, const int32_t* ev_user, const int64_t* ev_item,
                                                            int64_t* hist, int64_t* count, int N) {
  const int n = blockIdx.x * HT + threadIdx.x;
  if (n >= N) return;
  const int64_t cell = plan[2 * (int64_t)n], left = plan[2 * (int64_t)n + 1];
  if (cell >= 0) hist[cell] = ev_item[n];
  if (left >= 0) count[ev_user[n]] = left;   // left >= 0 only for an accepted event: ev_user[n] lies in [0, U)
}

struct BatchArgs {
  const int64_t* hist; const int64_t* count; const int32_t* req_user;
  int64_t* tokens_out; int64_t* mask_out; int32_t* len_out; int64_t* positions_out; int64_t* weights_out; int64_t* exclude_out;
  int32_t* live_out;
  int64_t U, mask_id;
  int C, L, P, E;
};

__global__ __launch_bounds__(HT) void history_batch_kernel(BatchArgs a) {
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int32_t u = a.req_user[r];
  const bool live = u >= 0 && u < a.U;
  int64_t n = live ? a.count[u] : 0;
  if (n < 0) n = 0;                                           // (outside the contract; reads stay inside the user's ring)
  const int64_t cap = a.C < a.L - 1 ? a.C : a.L - 1;
  const int h = (int)(n < cap ? n : cap);                     // items in the window
  const int64_t ecap = a.C < a.E ? a.C : a.E;
  const int en = (int)(n < ecap ? n : ecap);                  // items in the exclusion list
  const int64_t* ring = a.hist + (live ? (int64_t)u * a.C : 0);   // h = en = 0 for a dead row: never read
  const int w0 = (int)((n - h) % a.C), e0 = (int)((n - en) % a.C);   // the oldest item's cell; the run wraps at C at most once
  for (int p = tid; p < a.L; p += HT) {
    int64_t tok = p == h ? a.mask_id : (int64_t)0;
    if (p < h) {
      const int c = w0 + p;
      tok = ring[c >= a.C ? c - a.C : c];
    }
    a.tokens_out[r * a.L + p] = tok;
    a.mask_out[r * a.L + p] = p <= h ? 1 : 0;
  }
  for (int p = tid; p < a.P; p += HT) {
    a.positions_out[r * a.P + p] = p == 0 ? (int64_t)h : (int64_t)0;
    a.weights_out[r * a.P + p] = p == 0 ? 1 : 0;
  }
  for (int e = tid; e < a.E; e += HT) {
    int64_t x = -1;
    if (e < en) {
      const int c = e0 + e;
      x = ring[c >= a.C ? c - a.C : c];
    }
    a.exclude_out[r * a.E + e] = x;
  }
  if (tid == 0) {
    a.len_out[r] = h + 1;
    if (a.live_out) a.live_out[r] = live ? 1 : 0;
  }
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

extern "C" int64_t b4r_history_append_scratch_bytes(int32_t N) {
  if (N < 0 || N > HIST_MAX_EVENTS) {
    b4r_set_error("b4r_history_append_scratch_bytes: N = %d outside [0, %d]", N, HIST_MAX_EVENTS);
    return -1;
  }
  return (int64_t)N * 16;
}

extern "C" int b4r_history_append(int64_t* hist, int64_t* count, int64_t U, int32_t C, int32_t V, int32_t first_item, const int32_t* ev_user,
                                  const int64_t* ev_item, int32_t N, int32_t* accepted_out, void* scratch, int64_t scratch_bytes,
                                  b4r_stream_t stream) {
  const char* what = "b4r_history_append";
  B4R_CHECK_ARG(N >= 0 && N <= HIST_MAX_EVENTS && C >= 1 && C <= HIST_MAX_CAPACITY && U >= 1 && U < ((int64_t)1 << 40) / C + 1 &&
                    U * C < ((int64_t)1 << 40),
                B4R_E_SHAPE, "%s: bad shape (N = %d in [0, %d], C = %d in [1, %d], U = %lld >= 1, U * C < 2^40)", what, N,
                HIST_MAX_EVENTS, C, HIST_MAX_CAPACITY, (long long)U);
  if (N == 0) return B4R_OK;
  B4R_CHECK_ARG(hist && count && ev_user && ev_item && scratch, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG((((uintptr_t)scratch) & 7u) == 0, B4R_E_BADARG, "%s: the scratch is not 8-byte aligned", what);
  const int64_t need = (int64_t)N * 16;
  B4R_CHECK_ARG(scratch_bytes >= need, B4R_E_NOMEM, "%s: scratch of %lld bytes, %lld needed", what, (long long)scratch_bytes,
                (long long)need);
  B4R_CHECK_ARG(!overlaps(accepted_out, (int64_t)N * 4, ev_user, (int64_t)N * 4) &&
                    !overlaps(accepted_out, (int64_t)N * 4, ev_item, (int64_t)N * 8),
                B4R_E_BADARG, "%s: accepted_out overlaps the events", what);
  const int tiles = (N + HT - 1) / HT;
  PlanArgs pa{count, ev_user, ev_item, (int64_t*)scratch, accepted_out, U, (int64_t)V, (int64_t)first_item, C, N};
  hipLaunchKernelGGL(history_plan_kernel, dim3(tiles), dim3(HT), 0, (hipStream_t)stream, pa);
  B4R_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(history_commit_kernel, dim3(tiles), dim3(HT), 0, (hipStream_t)stream, (const int64_t*)scratch, ev_user, ev_item, hist,
                     count, N);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int b4r_history_batch(const int64_t* hist, const int64_t* count, int64_t U, int32_t C, const int32_t* req_user, int32_t R,
                                 int32_t L, int32_t P, int32_t E, int64_t mask_id, int64_t* tokens_out, int64_t* input_mask_out,
                                 int32_t* len_out, int64_t* positions_out, int64_t* weights_out, int64_t* exclude_out, int32_t* live_out,
                                 b4r_stream_t stream) {
  const char* what = "b4r_history_batch";
  B4R_CHECK_ARG(L >= 2 && L <= HIST_MAX_LEN && P >= 1 && E >= 1 && R >= 0, B4R_E_SHAPE,
                "%s: bad shape (L = %d in [2, %d], P = %d >= 1, E = %d >= 1, R = %d >= 0)", what, L, HIST_MAX_LEN, P, E, R);
  B4R_CHECK_ARG(C >= 1 && C <= HIST_MAX_CAPACITY && U >= 1 && U < ((int64_t)1 << 40) / C + 1 && U * C < ((int64_t)1 << 40), B4R_E_SHAPE,
                "%s: bad state shape (C = %d in [1, %d], U = %lld >= 1, U * C < 2^40)", what, C, HIST_MAX_CAPACITY, (long long)U);
  if (R == 0) return B4R_OK;
  B4R_CHECK_ARG(hist && count && req_user && tokens_out && input_mask_out && len_out && positions_out && weights_out && exclude_out,
                B4R_E_BADARG, "%s: null argument", what);
  BatchArgs ba{hist, count, req_user, tokens_out, input_mask_out, len_out, positions_out, weights_out, exclude_out, live_out,
               U, mask_id, C, L, P, E};
  hipLaunchKernelGGL(history_batch_kernel, dim3(R), dim3(HT), 0, (hipStream_t)stream, ba);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
