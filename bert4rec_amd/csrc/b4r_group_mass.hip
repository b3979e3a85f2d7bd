// Category affinity (include/b4r.h: b4r_group_mass): the probability mass of every item group under each row's catalogue softmax,
// P(next item in group g | row r) = sum of p_j over the allowed items labelled g, without an [R, V] buffer.
//
// Serves  BERT4RecModel.group_affinity_tensor / group_audience_tensor, Recommender.category_affinity / category_audience /
//         recommend_shelves.
//
// Contract: s(r, j), allowed(r) are b4r_rank_full_ex's with gt = NULL, t = fl32(s * inv_temperature) and u = fl32((double) t - row_lse[r])
// are b4r_score_dist's t and query_logp, c = llrint(exp(min((double) u, 0.0)) * 2^40) is b4r_audience_merge's demand term.  The sums
// are integer sums (units of 2^-40): the bits do not depend on the order, the chunking or the grid.
//
//   group_mass_kernel   grid (tile of 16 rows) x (chunk of 1024 ids): the tile of b4r_catalogue_tile.h, staged as b4r_score_dist's
//                       sweep stages it (4 ids x 16 rows of t per thread in registers).  After the k-loop the staging buffer is dead
//                       and becomes the [16][GM_GW + 1] int64 window of sums over GM_GW consecutive groups (slot GM_GW: the labels
//                       outside [0, G)); the counts have a [16][GM_GW + 1] int32 window of their own.  The workgroup makes one pass
//                       per window of groups that has a label in its chunk (a 256-bit map of the windows met, ascending): the
//                       products are formed once and every item's exponential once, in the pass of its window; a pass costs the
//                       zeroing and the flush of the two windows.  In a pass a wave first combines the lanes that share a label (up
//                       to GM_COMBINE labels per id step, a butterfly per row; few large groups would otherwise send 64 lanes to one
//                       LDS address), the lanes left over add on their own.  A pass is flushed with one global integer atomic per
//                       non-zero (row, group) and output.
//
// The outputs are zeroed by enqueued memsets; no floating-point atomics, no host sync.
#include <algorithm>
#include <cmath>

#include "b4r_common.h"
#include "b4r_catalogue_tile.h"

namespace {

constexpr int GM_GW = 256;        // groups per window
constexpr int GM_SLOTS = GM_GW + 1;   // + the slot of the labels outside [0, G)
constexpr int GM_COMBINE = 2;     // labels a wave combines per id step before its lanes add on their own
constexpr int GM_COMBINE_MIN = 4; // lanes that make a combination worth its butterflies
constexpr int GM_MAX_G = 65536;
constexpr int GM_WINDOWS = GM_MAX_G / GM_GW;   // at most 256 windows
constexpr int GM_REST = -1, GM_NONE = -2;      // a thread's label for an id of the rest / an id that adds nothing
constexpr int GM_MAX_V = 1 << 22; // 2^22 items of at most 2^40 units each: a sum stays below 2^62

static_assert(sizeof(int64_t) * TILE_G * GM_SLOTS <= sizeof(float) * TILE_IPT * TILE_T * (TILE_KB + 1),
              "the window of sums lives in the dead staging buffer");

struct GroupMassArgs {
  const float* hidden; const int64_t* hidden_row; const float* table; const float* bias; const float* scale;
  const int64_t* exclude;
  const uint32_t* allow; const int32_t* row_filter;   // [n_filters][ceil(V / 32)], [R] or NULL
  const double* row_lse;                              // [R]
  const int32_t* item_group;                          // [V] (NULL: every label is outside [0, G))
  int64_t* group_mass; int32_t* group_n; int64_t* rest_mass; int32_t* rest_n;
  float inv_t;
  int hidden_ld, H, V, lo, E, n, n_filters, G;
};

__global__ __launch_bounds__(TILE_T, 2) void group_mass_kernel(GroupMassArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_IPT * TILE_T * (TILE_KB + 1)];
  __shared__ __attribute__((aligned(16))) float hsh[TILE_G * TILE_KB];
  __shared__ uint32_t bits[TILE_G][TILE_CH / 32];
  __shared__ int64_t s_hoff[TILE_G], s_gt[TILE_G];
  __shared__ double s_lse[TILE_G];
  __shared__ int s_cnt[TILE_G][GM_SLOTS];
  __shared__ uint32_t s_win[GM_WINDOWS / 32 + 1];     // bit w: a label of window w is in the chunk; the last word: a label of the rest

  const int tid = threadIdx.x, lane = tid & 63;
  const int lr0 = blockIdx.x * TILE_G;
  const int chunk = blockIdx.y;
  const int64_t c0 = (int64_t)chunk * TILE_CH;
  const bool with_rest = a.rest_mass || a.rest_n;
  const bool with_groups = a.group_mass || a.group_n;
  const int H = a.H;

  // this thread's 4 ids: the label in [0, G), GM_REST for a label outside (when the rest is wanted), GM_NONE for an id that adds nothing
  int lab[TILE_Q];
  if (tid <= GM_WINDOWS / 32) s_win[tid] = 0u;
#pragma unroll
  for (int q = 0; q < TILE_Q; ++q) {
    const int64_t j = c0 + q * TILE_T + tid;
    int l = GM_NONE;
    if (j >= a.lo && j < a.V) {
      const int32_t g = a.item_group ? a.item_group[j] : -1;
      if (g < 0 || g >= a.G) l = with_rest ? GM_REST : GM_NONE;
      else if (with_groups) l = g;
    }
    lab[q] = l;
  }
  if (tid < TILE_G) {
    tile_row_setup(tid, lr0, a.n, 0, a.hidden_row, a.hidden_ld, nullptr, s_hoff, s_gt);
    double lse = 0.0;
    if (lr0 + tid < a.n) lse = a.row_lse[lr0 + tid];
    if (!(lse > -INFINITY)) s_hoff[tid] = -1;         // -inf or NaN: a dead row, as one with a negative hidden_row
    s_lse[tid] = lse;
  }
  tile_row_bitmap(bits, a.allow != nullptr, a.allow, a.row_filter, a.n_filters, a.exclude, a.E, s_hoff, 0, lr0, a.n, a.V, c0);
#pragma unroll
  for (int q = 0; q < TILE_Q; ++q) {                  // (s_win was zeroed before the barrier inside tile_row_bitmap)
    if (lab[q] >= 0) atomicOr(&s_win[lab[q] / GM_GW / 32], 1u << ((lab[q] / GM_GW) & 31));
    else if (lab[q] == GM_REST) atomicOr(&s_win[GM_WINDOWS / 32], 1u);
  }
  __syncthreads();
  {
    uint32_t met = 0u;
#pragma unroll
    for (int w = 0; w <= GM_WINDOWS / 32; ++w) met |= s_win[w];
    if (met == 0u) return;                            // no id of the chunk adds to an output (uniform over the workgroup)
  }

  // ---- t = fl32(s * inv_temperature) in registers; okm[q] bit g: id q of this thread is allowed for row g --------------------
  float t[TILE_Q][TILE_G];
  uint32_t okm[TILE_Q];
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
        const bool ok = inb && s_hoff[g] >= 0 && !ex;
        float s = acc[ii][g] + b;
        if (a.scale) s = s * sc;
        t[q][g] = s * a.inv_t;
        m |= ok ? (1u << g) : 0u;
      }
      okm[q] = lab[q] != GM_NONE ? m : 0u;
    }
  }

  // ---- the staging buffer is dead: it becomes the window of sums; one pass per window of groups met in the chunk ------------------
  int64_t (*s_mass)[GM_SLOTS] = reinterpret_cast<int64_t (*)[GM_SLOTS]>(tile);
  bool rest_now = (s_win[GM_WINDOWS / 32] & 1u) != 0u;   // the rest rides in the first pass
  int win = -1;
#pragma unroll 1
  for (;;) {
    // the next window met, ascending (uniform over the workgroup: s_win is not written any more)
    int next = -1;
    for (int w = (win + 1) >> 5; w < GM_WINDOWS / 32 && next < 0; ++w) {
      uint32_t word = s_win[w];
      if (w == (win + 1) >> 5) word &= ~0u << ((win + 1) & 31);
      if (word) next = w * 32 + __ffs(word) - 1;
    }
    if (next < 0) {
      if (!rest_now) break;
      next = GM_WINDOWS;                                // no window was met: a pass for the rest alone
    }
    win = next;
    const int g0 = win * GM_GW;                         // first group of this pass
    __syncthreads();                                    // the k-loop, or the flush of the pass before, is done with the buffers
    for (int i = tid; i < TILE_G * GM_SLOTS; i += TILE_T) {
      (&s_mass[0][0])[i] = 0;
      (&s_cnt[0][0])[i] = 0;
    }
    __syncthreads();

#pragma unroll
    for (int q = 0; q < TILE_Q; ++q) {
      int sl = -1;                                      // the slot of the window this id adds to in this pass
      if (lab[q] >= 0) {
        if ((unsigned)(lab[q] - g0) < (unsigned)GM_GW) sl = lab[q] - g0;
      } else if (lab[q] == GM_REST && rest_now) {
        sl = GM_GW;
      }
      const uint32_t m = sl >= 0 ? okm[q] : 0u;
      int64_t c[TILE_G];
#pragma unroll
      for (int g = 0; g < TILE_G; ++g) {
        c[g] = 0;
        if ((m >> g) & 1u) {
          const float u = (float)((double)t[q][g] - s_lse[g]);           // b4r_score_dist's query_logp
          c[g] = (int64_t)llrint(exp(fmin((double)u, 0.0)) * 1099511627776.0);   // b4r_audience_merge's demand term
        }
      }
      bool todo = m != 0u;
      // the lanes of the wave that share the first pending label add as one: a butterfly per row, one LDS atomic per (row, label)
#pragma unroll 1
      for (int it = 0; it < GM_COMBINE; ++it) {
        const uint64_t act = __ballot(todo);
        if (act == 0ull) break;
        const int lead = __shfl(sl, __ffsll((unsigned long long)act) - 1, 64);
        const bool mine = todo && sl == lead;
        if (__popcll(__ballot(mine)) < GM_COMBINE_MIN) break;
#pragma unroll
        for (int g = 0; g < TILE_G; ++g) {
          const bool ok = mine && ((m >> g) & 1u);
          const uint64_t bo = __ballot(ok);
          if (bo == 0ull) continue;                       // uniform over the wave
          const int64_t sum = wave_sum_i64(ok ? c[g] : 0);
          if (lane == 0) {
            if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&s_mass[g][lead]), (unsigned long long)sum);
            atomicAdd(&s_cnt[g][lead], (int)__popcll(bo));
          }
        }
        todo = todo && !mine;
      }
      if (todo) {
#pragma unroll
        for (int g = 0; g < TILE_G; ++g) {
          if (!((m >> g) & 1u)) continue;
          if (c[g] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&s_mass[g][sl]), (unsigned long long)c[g]);
          atomicAdd(&s_cnt[g][sl], 1);
        }
      }
    }
    __syncthreads();

    // flush: one global integer atomic per non-zero (row, group) and output
    for (int i = tid; i < TILE_G * GM_SLOTS; i += TILE_T) {
      const int g = i / GM_SLOTS, sl = i - g * GM_SLOTS;
      const int lr = lr0 + g;
      if (lr >= a.n) continue;
      const int cnt = s_cnt[g][sl];
      if (cnt == 0) continue;                             // nothing was added to this cell (mass > 0 implies cnt > 0)
      const int64_t mass = s_mass[g][sl];
      if (sl == GM_GW) {
        if (a.rest_mass && mass != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.rest_mass + lr), (unsigned long long)mass);
        if (a.rest_n) atomicAdd(a.rest_n + lr, cnt);
      } else {
        const int64_t o = (int64_t)lr * a.G + g0 + sl;     // g0 + sl < G: a slot below GM_GW is only given to a label in [0, G)
        if (a.group_mass && mass != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.group_mass + o), (unsigned long long)mass);
        if (a.group_n) atomicAdd(a.group_n + o, cnt);
      }
    }
    rest_now = false;
    if (win >= GM_WINDOWS) break;
  }
}

}  // namespace

extern "C" int b4r_group_mass(const float* hidden, int32_t hidden_ld, const int64_t* hidden_row, const float* table, const float* bias,
                              int32_t H, int32_t V, int32_t first_item, int32_t R, const int64_t* exclude, int32_t E,
                              const uint32_t* allow_bits, int32_t n_filters, const int32_t* row_filter, const float* item_scale,
                              float inv_temperature, const double* row_lse, const int32_t* item_group, int32_t G, int64_t* group_mass,
                              int32_t* group_n, int64_t* rest_mass, int32_t* rest_n, b4r_stream_t stream) {
  const char* what = "b4r_group_mass";
  B4R_CHECK_ARG(R >= 0 && E >= 0 && first_item >= 0, B4R_E_SHAPE, "%s: bad shape (R = %d, E = %d, first_item = %d)", what, R, E,
                first_item);
  B4R_CHECK_ARG(G >= 0 && G <= GM_MAX_G, B4R_E_SHAPE, "%s: G = %d groups must lie in [0, %d]", what, G, GM_MAX_G);
  B4R_CHECK_ARG(H > 0 && H % 4 == 0 && H <= 4096 && hidden_ld >= H && V > 0 && V <= GM_MAX_V, B4R_E_SHAPE,
                "%s: bad shape (H = %d, hidden_ld = %d, V = %d in [1, %d])", what, H, hidden_ld, V, GM_MAX_V);
  B4R_CHECK_ARG(!allow_bits || n_filters > 0, B4R_E_SHAPE, "%s: allow_bits with n_filters = %d", what, n_filters);
  B4R_CHECK_ARG(std::isfinite(inv_temperature) && inv_temperature > 0.f, B4R_E_BADARG,
                "%s: inv_temperature = %g must be finite and > 0", what, (double)inv_temperature);
  const bool groups = G > 0 && (group_mass || group_n);
  const bool rest = rest_mass || rest_n;
  if (R == 0 || (!groups && !rest)) return B4R_OK;
  B4R_CHECK_ARG(hidden && table && row_lse, B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(G == 0 || item_group, B4R_E_BADARG, "%s: item_group is NULL with G = %d", what, G);
  B4R_CHECK_ARG(E == 0 || exclude, B4R_E_BADARG, "%s: exclude is NULL with E = %d", what, E);
  B4R_CHECK_ARG(b4r_aligned16(table), B4R_E_ALIGN, "%s: the table must be 16-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  bool zeroed = true;
  if (groups && group_mass) zeroed &= hipMemsetAsync(group_mass, 0, sizeof(int64_t) * (size_t)R * G, s) == hipSuccess;
  if (groups && group_n) zeroed &= hipMemsetAsync(group_n, 0, sizeof(int32_t) * (size_t)R * G, s) == hipSuccess;
  if (rest_mass) zeroed &= hipMemsetAsync(rest_mass, 0, sizeof(int64_t) * (size_t)R, s) == hipSuccess;
  if (rest_n) zeroed &= hipMemsetAsync(rest_n, 0, sizeof(int32_t) * (size_t)R, s) == hipSuccess;
  if (!zeroed) {
    b4r_set_error("%s: zeroing the outputs failed: %s", what, hipGetErrorString(hipGetLastError()));
    return B4R_E_HIP;
  }
  const int nch = (int)tile_chunks_of(V);               // <= 4096
  GroupMassArgs ga{hidden, hidden_row, table, bias, item_scale, exclude, allow_bits, row_filter, row_lse, item_group,
                   groups ? group_mass : nullptr, groups ? group_n : nullptr, rest_mass, rest_n, inv_temperature, hidden_ld, H, V,
                   first_item, E, R, n_filters, G};
  hipLaunchKernelGGL(group_mass_kernel, dim3(b4r_cdiv(R, TILE_G), nch), dim3(TILE_T), 0, s, ga);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
