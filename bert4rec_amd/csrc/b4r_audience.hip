// Audience selection (include/b4r.h: b4r_audience_merge): the step ACROSS users of "given an item, which users".  The log probabilities
// come from the existing sweep (b4r_score_dist's query_logp, every row asking for the same Q items); the kernel here merges one batch
// of users into the K best users of every item, which stay on the device while the batches go by, and counts reach and demand.
//
//   audience_merge_kernel   one workgroup of 256 threads per tile of 4 items.  The R rows go by in passes of 256: a wave takes 64
//                           consecutive rows, 16 at a time (4 consecutive floats of a row per lane group, four independent loads per
//                           thread).  An entry that is live, and that comes before the item's current K-th entry when the list is
//                           full, is appended to the item's pending buffer in LDS (512 entries; the slot is a prefix count by wave
//                           ballots and one LDS exchange).  A buffer that could overflow in the next pass, and every non-empty one
//                           after the last pass, is merged into the running list: the pending entries are ordered among themselves by
//                           counting, the list (sorted, in L2) is staged in LDS, every running entry finds by bisection how many
//                           pending entries come before it, every pending entry how many running entries do not come after it, and
//                           whoever lands below K writes itself there.  The order is strict, so every output cell has one writer.
//                           Once the lists are full almost nothing passes the K-th entry and a merge is a handful of entries.
//
// No atomics, no floating-point sum: reach and demand are integer sums, so the bits depend on the set of (user, logp) pairs alone.
// The entry point checks every argument before the launch and only enqueues.
#include <cmath>

#include "b4r_common.h"
#include "b4r_wave.h"   // order_image

namespace {

constexpr int AT = 256;          // threads per workgroup (4 waves)
constexpr int AM_TILE = 4;       // items per workgroup
constexpr int AM_PASS = 256;     // rows per pass: 4 per thread
constexpr int AM_PEND = 512;     // pending entries per item
constexpr int AM_MAX_K = 1024;

// (ia, ua) comes strictly before (ib, ub): the larger log probability, then the lower user id
__device__ __forceinline__ bool before(uint32_t ia, int64_t ua, uint32_t ib, int64_t ub) { return ia > ib || (ia == ib && ua < ub); }

struct AudienceArgs {
  const float* logp; const int64_t* user_ids;
  int64_t* best_user; float* best_logp; int64_t* reach; int64_t* demand;
  int64_t user0;
  float min_logp;
  int ld, R, Q, K;
};

__global__ __launch_bounds__(AT) void audience_merge_kernel(AudienceArgs a) {
  __shared__ int64_t s_pend_user[AM_TILE * AM_PEND];   // 16 KB: the pending entries of every item, in row order
  __shared__ float s_pend_logp[AM_TILE * AM_PEND];     //  8 KB
  __shared__ int64_t s_sort_user[AM_PEND];             //  4 KB: the pending entries of the item being merged, in the order
  __shared__ float s_sort_logp[AM_PEND];               //  2 KB
  __shared__ int64_t s_run_user[AM_MAX_K];             //  8 KB: its running list; the reduction of reach and demand at the end
  __shared__ float s_run_logp[AM_MAX_K];               //  4 KB
  __shared__ int s_wcnt[AT / 64][AM_TILE];
  __shared__ int s_count[AM_TILE];                     // pending entries
  __shared__ int s_nrun[AM_TILE];                      // live running entries
  __shared__ uint32_t s_thr_img[AM_TILE];              // the K-th entry of a full list
  __shared__ int64_t s_thr_user[AM_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int q0 = blockIdx.x * AM_TILE;
  const int nt = a.Q - q0 < AM_TILE ? a.Q - q0 : AM_TILE;    // items of this tile, >= 1

  // the live length of every running list (live entries first: the caller's initial state, or what an earlier call left)
  {
    int n[AM_TILE] = {0, 0, 0, 0};
#pragma nounroll
    for (int e0 = 0; e0 < K; e0 += AT) {
      const int e = e0 + tid;
      bool ok[AM_TILE];
#pragma unroll
      for (int i = 0; i < AM_TILE; ++i) {
        const int64_t o = (int64_t)(q0 + i) * K + e;
        ok[i] = i < nt && e < K && a.best_user[o] >= 0 && a.best_logp[o] > -INFINITY;
      }
#pragma unroll
      for (int i = 0; i < AM_TILE; ++i) n[i] += __popcll(__ballot(ok[i]));
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < AM_TILE; ++i) s_wcnt[wave][i] = n[i];
    }
  }
  __syncthreads();
  if (tid < AM_TILE) {
    int n = 0;
    if (tid < nt) {
      for (int w = 0; w < AT / 64; ++w) n += s_wcnt[w][tid];
      if (n == K) {
        const int64_t o = (int64_t)(q0 + tid) * K + (K - 1);
        s_thr_img[tid] = order_image(a.best_logp[o]);
        s_thr_user[tid] = a.best_user[o];
      }
    }
    s_nrun[tid] = n;
    s_count[tid] = 0;
  }
  __syncthreads();

  const int ii = tid & (AM_TILE - 1);                        // this thread's item of the tile, in every pass
  const int rr = 64 * wave + (lane >> 2);                    // and its first row of a pass: a wave holds 64 consecutive rows
  const bool has_item = ii < nt;
  const uint64_t item_lanes = 0x1111111111111111ull << ii;   // the lanes of a wave that hold item ii
  const uint64_t below = (1ull << lane) - 1ull;
  int64_t n_reach = 0, n_demand = 0;

#pragma nounroll
  for (int r0 = 0; r0 < a.R; r0 += AM_PASS) {
    float x[4];
    int64_t u[4];
    bool keep[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + rr + 16 * j;                        // r0 + 255 <= R - 1 + 255: no overflow for R < 2^31 - 256 (checked)
      const bool in = has_item && r < a.R;
      x[j] = in ? a.logp[(int64_t)r * a.ld + q0 + ii] : -INFINITY;
      u[j] = !in ? (int64_t)-1 : (a.user_ids ? a.user_ids[r] : (int64_t)((uint64_t)a.user0 + (uint64_t)r));
    }
    const bool full = s_nrun[ii] == K;
    const uint32_t t_img = s_thr_img[ii];
    const int64_t t_user = s_thr_user[ii];
    uint64_t b[4];
    int total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = u[j] >= 0 && x[j] > -INFINITY;       // a NaN is dead
      if (live) {
        n_reach += x[j] >= a.min_logp ? 1 : 0;
        n_demand += (int64_t)llrint(exp((double)x[j]) * 1099511627776.0);
      }
      keep[j] = live && (!full || before(order_image(x[j]), u[j], t_img, t_user));
      b[j] = __ballot(keep[j]) & item_lanes;
      total += __popcll(b[j]);
    }
    if (lane < AM_TILE) s_wcnt[wave][lane] = total;          // (lane == ii here)
    __syncthreads();
    int base = s_count[ii];
    for (int w = 0; w < wave; ++w) base += s_wcnt[w][ii];
    // base + every slot below stays under AM_PEND: a buffer above AM_PEND - AM_PASS was merged after the pass before
#pragma unroll
    for (int j = 0; j < 4; ++j) {                            // waves, quarters, lanes: the slots follow the rows
      if (keep[j]) {
        const int slot = base + __popcll(b[j] & below);
        s_pend_user[ii * AM_PEND + slot] = u[j];
        s_pend_logp[ii * AM_PEND + slot] = x[j];
      }
      base += __popcll(b[j]);
    }
    __syncthreads();
    if (tid < AM_TILE) {
      int n = s_count[tid];
      for (int w = 0; w < AT / 64; ++w) n += s_wcnt[w][tid];
      s_count[tid] = n;
    }
    __syncthreads();

    const bool last = r0 + AM_PASS >= a.R;
#pragma nounroll
    for (int i = 0; i < nt; ++i) {
      const int p = s_count[i];                              // uniform over the workgroup
      if (p == 0 || (!last && p <= AM_PEND - AM_PASS)) continue;
      const int n = s_nrun[i];
      const int64_t o = (int64_t)(q0 + i) * K;
#pragma nounroll
      for (int e = tid; e < n; e += AT) {                    // the loads fly while the pending entries are ordered
        s_run_user[e] = a.best_user[o + e];
        s_run_logp[e] = a.best_logp[o + e];
      }
      const int64_t* pu = s_pend_user + i * AM_PEND;
      const float* px = s_pend_logp + i * AM_PEND;
#pragma nounroll
      for (int me = tid; me < p; me += AT) {                 // the place of every pending entry among the pending ones, by counting
        const int64_t eu = pu[me];
        const float ex = px[me];
        const uint32_t ei = order_image(ex);
        int pos = 0;
#pragma unroll 4
        for (int j = 0; j < p; ++j) {
          const uint32_t ji = order_image(px[j]);
          pos += (before(ji, pu[j], ei, eu) || (ji == ei && pu[j] == eu && j < me)) ? 1 : 0;
        }
        s_sort_user[pos] = eu;                               // pos < p: the places are a permutation
        s_sort_logp[pos] = ex;
      }
      __syncthreads();
#pragma nounroll
      for (int e = tid; e < n + p; e += AT) {
        int rank;
        int64_t eu;
        float ex;
        if (e < n) {                                         // a running entry: its place, plus the pending ones that come before it
          eu = s_run_user[e];
          ex = s_run_logp[e];
          const uint32_t ei = order_image(ex);
          int lo = 0, hi = p;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (before(order_image(s_sort_logp[mid]), s_sort_user[mid], ei, eu)) lo = mid + 1; else hi = mid;
          }
          rank = e + lo;
        } else {                                             // a pending entry: a running entry of equal key comes first
          const int me = e - n;
          eu = s_sort_user[me];
          ex = s_sort_logp[me];
          const uint32_t ei = order_image(ex);
          int lo = 0, hi = n;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (!before(ei, eu, order_image(s_run_logp[mid]), s_run_user[mid])) lo = mid + 1; else hi = mid;
          }
          rank = me + lo;
        }
        if (rank < K) {                                      // rank < n + p: the ranks are a permutation for a sorted list
          a.best_user[o + rank] = eu;
          a.best_logp[o + rank] = ex;
          if (rank == K - 1) {
            s_thr_img[i] = order_image(ex);
            s_thr_user[i] = eu;
          }
        }
      }
      __syncthreads();
      if (tid == 0) {
        s_nrun[i] = n + p < K ? n + p : K;
        s_count[i] = 0;
      }
      __syncthreads();
    }
  }

  // the tail of every list is dead, whatever the caller left there
  for (int i = 0; i < nt; ++i) {
    const int64_t o = (int64_t)(q0 + i) * K;
    for (int e = s_nrun[i] + tid; e < K; e += AT) {
      a.best_user[o + e] = -1;
      a.best_logp[o + e] = -INFINITY;
    }
  }
  // reach and demand: the 64 threads of an item, summed by one of them (integers: any order gives the same sum)
  int64_t* s_sum = s_run_user;
  s_sum[tid] = n_reach;
  s_sum[AT + tid] = n_demand;
  __syncthreads();
  if (tid < nt) {
    int64_t nr = 0, nd = 0;
#pragma unroll 4
    for (int g = 0; g < AT / AM_TILE; ++g) {
      nr += s_sum[g * AM_TILE + tid];
      nd += s_sum[AT + g * AM_TILE + tid];
    }
    if (a.reach) a.reach[q0 + tid] += nr;
    if (a.demand) a.demand[q0 + tid] += nd;
  }
}

}  // namespace

extern "C" int b4r_audience_merge(const float* logp, int32_t ld, int32_t R, int32_t Q, const int64_t* user_ids, int64_t user0,
                                  float min_logp, int32_t K, int64_t* best_user, float* best_logp, int64_t* reach, int64_t* demand,
                                  b4r_stream_t stream) {
  const char* what = "b4r_audience_merge";
  B4R_CHECK_ARG(K >= 1 && K <= AM_MAX_K && Q >= 1 && R >= 0 && R <= INT32_MAX - AM_PASS && ld >= Q, B4R_E_SHAPE,
                "%s: bad shape (K = %d in [1, %d], Q = %d >= 1, R = %d in [0, 2^31 - %d), ld = %d >= Q)", what, K, AM_MAX_K, Q, R,
                AM_PASS, ld);
  B4R_CHECK_ARG(logp && best_user && best_logp, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(!std::isnan(min_logp), B4R_E_BADARG, "%s: min_logp is NaN", what);
  if (R == 0) return B4R_OK;
  AudienceArgs aa{logp, user_ids, best_user, best_logp, reach, demand, user0, min_logp, ld, R, Q, K};
  hipLaunchKernelGGL(audience_merge_kernel, dim3((unsigned)((Q + AM_TILE - 1) / AM_TILE)), dim3(AT), 0, (hipStream_t)stream, aa);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
