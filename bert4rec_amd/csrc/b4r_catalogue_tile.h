// The 16 x 1024 score tile of the full-catalogue sweeps: b4r_rank_full.hip, b4r_sample_full.hip, b4r_score_dist.hip and
// b4r_rank_joint.hip each launch one 256-thread workgroup per (tile of 16 rows) x (chunk of 1024 ids).  Stated once here: the tile's
// constants, the scalar score of one (row, id), the per-row setup, the per-row "not ranked" bitmap and the host's scratch arithmetic.
// Not here: the k-block loop that forms a thread's 4 ids x 16 rows of fma chains and the sweep's side of the radix select stay
// written out in each sweep, the same text in each.  As functions they changed the sweeps' register allocation and two of them
// measured slower; a change to either block is made in every sweep that has it.
#pragma once
#include <algorithm>

#include "b4r_common.h"
#include "b4r_select.h"

namespace {

constexpr int TILE_T = 256;               // threads per workgroup
constexpr int TILE_G = 16;                // rows per sweep workgroup
constexpr int TILE_Q = 4;                 // ids per thread per chunk
constexpr int TILE_IPT = 2;               // ids scored together per k-block (TILE_Q / TILE_IPT steps)
constexpr int TILE_CH = TILE_T * TILE_Q;  // ids per chunk
constexpr int TILE_KB = 16;               // k-block (floats of a table row staged at a time)

static_assert(TILE_T == TILE_G * 16, "digit search: 16 threads per row");
static_assert(TILE_G * TILE_KB == TILE_T, "one thread per staged hidden value");
static_assert(TILE_CH <= 65536, "the local id takes the low 16 bits of the sweep key");

// the scalar score of one (row, id): bias NULL: + 0.0f; scale (NULL: none) multiplies the rounded chain once
__device__ __forceinline__ float row_score(const float* h, const float* e, const float* bias, const float* scale, int64_t j, int H) {
  float acc = 0.f;
  for (int k = 0; k < H; ++k) acc = __builtin_fmaf(h[k], e[k], acc);   // k-ordered fp32 fma chain (the contract)
  const float s = acc + (bias ? bias[j] : 0.f);
  return scale ? s * scale[j] : s;
}

// thread tid < TILE_G: where row lr0 + tid of the group starts in `hidden` (-1: no such row), and its held-out item (-1: none)
__device__ __forceinline__ void tile_row_setup(int tid, int lr0, int n, int64_t r0, const int64_t* hidden_row, int hidden_ld,
                                               const int64_t* gt, int64_t* s_hoff, int64_t* s_gt) {
  const int lr = lr0 + tid;
  const bool rv = lr < n;
  const int64_t r = r0 + lr;
  s_hoff[tid] = rv ? (hidden_row ? hidden_row[r] : r) * hidden_ld : -1;
  s_gt[tid] = (rv && gt) ? gt[r] : -1;
}

// The per-row bitmap of the chunk, bit set = not ranked.  filt: it starts from the complement of the row's filter words of this
// chunk (no filter for the row: all ranked), otherwise from zeros; then the row's `exclude` ids of the chunk are set.  Needs s_hoff
// (the barrier inside orders it); the caller puts a barrier between this and the first read of `bits`.
__device__ __forceinline__ void tile_row_bitmap(uint32_t (&bits)[TILE_G][TILE_CH / 32], bool filt, const uint32_t* allow,
                                                const int32_t* row_filter, int n_filters, const int64_t* exclude, int E,
                                                const int64_t* s_hoff, int64_t r0, int lr0, int n, int V, int64_t c0) {
  const int tid = threadIdx.x;
  if (filt) {
    const int64_t W = ((int64_t)V + 31) >> 5;
    for (int i = tid; i < TILE_G * (TILE_CH / 32); i += TILE_T) {
      const int g = i / (TILE_CH / 32), w = i - g * (TILE_CH / 32);
      const int lr = lr0 + g;
      const int64_t wi = (c0 >> 5) + w;
      uint32_t word = 0u;
      if (lr < n && wi < W) {
        const int32_t f = row_filter ? row_filter[r0 + lr] : 0;
        if (f >= 0 && f < n_filters) word = ~allow[(int64_t)f * W + wi];
      }
      bits[g][w] = word;
    }
  } else {
    for (int i = tid; i < TILE_G * (TILE_CH / 32); i += TILE_T) (&bits[0][0])[i] = 0u;
  }
  __syncthreads();
  if (E > 0) {
    for (int f = tid; f < TILE_G * E; f += TILE_T) {
      const int g = f / E, e = f - g * E;
      if (s_hoff[g] < 0) continue;
      const int64_t id = exclude[(r0 + lr0 + g) * (int64_t)E + e];
      if (id >= c0 && id < c0 + TILE_CH) {
        const int l = (int)(id - c0);
        atomicOr(&bits[g][l >> 5], 1u << (l & 31));
      }
    }
  }
}

// ---- host: chunks, candidates per chunk, and how many rows (or parties) of a call fit the scratch at a time ---------------------
inline int64_t tile_chunks_of(int32_t V) { return ((int64_t)V + TILE_CH - 1) / TILE_CH; }
inline int64_t tile_cap_of(int32_t K) { return std::min<int64_t>(K, TILE_CH); }

// the 16-byte aligned start of the scratch regions
inline char* tile_scratch_base(void* scratch) { return reinterpret_cast<char*>(((uintptr_t)scratch + 15) & ~(uintptr_t)15); }

// rows per pass: all R if they fit, otherwise whole tiles of `per_tile` rows (0: not even one tile fits; the caller reports it);
// never more than 65535 tiles of 16 rows (whole tiles still for every per_tile, a divisor of 16), which keeps every grid of a
// pass within 2^31 workgroups
inline int64_t tile_group_of(const void* scratch, int64_t scratch_bytes, int64_t per_row, int64_t R, int per_tile) {
  const int64_t usable = scratch ? scratch_bytes - (int64_t)((16 - ((uintptr_t)scratch & 15)) & 15) : 0;
  int64_t group = usable > 0 ? usable / per_row : 0;
  group = std::min<int64_t>(group, R);
  if (group < R) group = group / per_tile * per_tile;
  return std::min<int64_t>(group, 65535LL * TILE_G);
}

}  // namespace
