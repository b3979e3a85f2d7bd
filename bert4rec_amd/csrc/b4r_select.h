// The radix select of the full-catalogue kernels, stated once: the state of one row's select and its digit search (the
// order-preserving image of a score, score_key, and the wave reductions are b4r_wave.h's).  b4r_rank_full.hip, b4r_sample_full.hip and b4r_rank_joint.hip select the best K of a chunk in their sweeps
// (48-bit keys: image << 16 | 1023 - local id) and the best K of a row in their merges (64-bit keys: image << 32 | ~id) with it.
// The keys are unique and their ascending order is "score descending, then id ascending" read from the top, so the outputs do not
// depend on the order in which LDS atomics place or count.
#pragma once
#include "b4r_common.h"
#include "b4r_wave.h"

namespace {

constexpr uint32_t NOT_ALLOWED = 0xFFFFFFFFu;   // raw-bits marker of an id that is not ranked (a NaN pattern: out of contract)

// state of one row's radix select over W-bit unique keys: `hi` top bits are resolved (= prefix); `rem` ids are still to be taken
// from those whose top bits equal the prefix; done: every key >= thr is taken (take = 0: none)
struct Sel {
  uint64_t prefix, thr;
  int hi, rem, done, take;
};

// init: n allowed keys, `need` to take; kmin / kmax over the allowed score keys (the top 32 bits of every W-bit key)
__device__ __forceinline__ void sel_init(Sel& s, int n, int need, uint32_t kmin, uint32_t kmax) {
  s.take = need > 0;
  s.rem = need;
  s.thr = 0;
  if (need <= 0 || need >= n) {
    s.done = 1; s.hi = 0; s.prefix = 0;   // none, or every allowed id (thr = 0)
    return;
  }
  const uint32_t diff = kmin ^ kmax;
  s.hi = diff ? __clz(diff) : 32;
  s.prefix = (uint64_t)kmax >> (32 - s.hi);
  s.done = 0;
}

__device__ __forceinline__ bool sel_match(const Sel& s, uint64_t key, int W) {
  return s.hi == 0 || (key >> (W - s.hi)) == s.prefix;
}

__device__ __forceinline__ int sel_nb(const Sel& s, int W) { return min(8, W - s.hi); }

// the 16 threads qq = 0..15 of a row: part[qq] = count of digits 255-16qq .. 240-16qq (descending)
__device__ __forceinline__ void sel_part(const uint32_t* hist, uint32_t* part, int qq) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) c += hist[255 - 16 * qq - i];
  part[qq] = c;
}

// the thread whose 16 digits hold the rem-th key from the top writes the advanced state `s` (a copy taken before the barrier
// that precedes this call) to `out`; the other threads of the row leave it alone
__device__ __forceinline__ void sel_advance(Sel s, Sel& out, const uint32_t* hist, const uint32_t* part, int qq, int W) {
  uint32_t above = 0;
  for (int i = 0; i < qq; ++i) above += part[i];
  const uint32_t rem = (uint32_t)s.rem;
  if (!(above < rem && above + part[qq] >= rem)) return;
  const int nb = sel_nb(s, W);
  for (int i = 0; i < 16; ++i) {
    const int d = 255 - 16 * qq - i;
    const uint32_t c = hist[d];
    if (above + c >= rem) {
      const uint32_t left = rem - above;
      s.prefix = (s.prefix << nb) | (uint64_t)d;
      s.hi += nb;
      s.rem = (int)left;
      if (c == left || s.hi >= W) {
        s.done = 1;
        s.thr = s.hi >= W ? s.prefix : (s.prefix << (W - s.hi));
      }
      out = s;
      return;
    }
    above += c;
  }
}

// ---- the merge: the best K of one row over all chunks' candidates, by one workgroup of T threads ------------------------------
constexpr int SEL_K_MAX = 1024;   // largest K

// The LDS of one merge workgroup: the kernel's own __shared__ variables, named here by reference (one struct holding the arrays
// themselves compiled the merges to other register counts and 8 bytes more: DESIGN.md 6.12).  extra: NULL where no extra count.
struct MergeSel {
  uint32_t (&hist)[256];
  uint32_t (&part)[16];
  Sel& st;
  uint32_t &n, &kmin, &kmax, &out;
  uint32_t* extra;
  uint64_t (&key)[SEL_K_MAX];   // the survivors in any order: image << 32 | ~id, and what the sweep stored with the id
  float (&val)[SEL_K_MAX];
};

// The candidates of the row whose chunks start at `row` (= row index * nch) are c_val / c_id [(row + chunk) * cap + i], the first
// c_cnt[row + chunk] of each chunk.  Selects the best min(K, their number) by the radix select on (image of c_val << 32 | ~id), leaves them in L.key / L.val and returns how many (every thread gets it, after a barrier).
// c_extra (with L.extra; NULL: none): one more count per chunk, c_extra[row + chunk], summed into *L.extra beside the candidates' counts.
template <int T>
__device__ __forceinline__ int merge_select(const MergeSel& L, const float* c_val, const int32_t* c_id, const int32_t* c_cnt,
                                            const int32_t* c_extra, int64_t row, int nch, int cap, int K) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int32_t* cnt = c_cnt + row;
  const int64_t base = row * cap;
  const int64_t total_slots = (int64_t)nch * cap;

  if (tid == 0) { L.n = 0; L.kmin = 0xFFFFFFFFu; L.kmax = 0u; L.out = 0; if (c_extra) *L.extra = 0; }
  __syncthreads();
  {
    uint32_t n = 0, extra = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
    for (int c = tid; c < nch; c += T) n += (uint32_t)cnt[c];
    if (c_extra)   // (a loop of its own: inside the loop above, the choice cost the merges two vector registers)
      for (int c = tid; c < nch; c += T) extra += (uint32_t)c_extra[row + c];
    for (int64_t e = tid; e < total_slots; e += T) {
      const int c = (int)(e / cap), i = (int)(e - (int64_t)c * cap);
      if (i >= cnt[c]) continue;
      const uint32_t k = score_key(c_val[base + e]);
      kmin = min(kmin, k); kmax = max(kmax, k);
    }
    n = wave_sum_u32(n); extra = wave_sum_u32(extra);
    kmin = wave_min_u32(kmin); kmax = wave_max_u32(kmax);
    if (lane == 0) { atomicAdd(&L.n, n); if (c_extra) atomicAdd(L.extra, extra); atomicMin(&L.kmin, kmin); atomicMax(&L.kmax, kmax); }
  }
  __syncthreads();
  const int n = (int)L.n;
  const int need = min(K, n);
  if (tid == 0) sel_init(L.st, n, need, L.kmin, L.kmax);
  for (int pass = 0; pass < 8; ++pass) {
    __syncthreads();
    if (L.st.done) break;
    for (int i = tid; i < 256; i += T) L.hist[i] = 0u;
    __syncthreads();
    const Sel s = L.st;
    const int nb = sel_nb(s, 64), sh = 64 - s.hi - nb;
    for (int64_t e = tid; e < total_slots; e += T) {
      const int c = (int)(e / cap), i = (int)(e - (int64_t)c * cap);
      if (i >= cnt[c]) continue;
      const uint64_t key = ((uint64_t)score_key(c_val[base + e]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c_id[base + e]);
      if (sel_match(s, key, 64)) atomicAdd(&L.hist[(key >> sh) & ((1u << nb) - 1u)], 1u);
    }
    __syncthreads();
    if (tid < 16) sel_part(L.hist, L.part, tid);
    __syncthreads();
    if (tid < 16) sel_advance(s, L.st, L.hist, L.part, tid, 64);
  }
  __syncthreads();
  if (L.st.take && L.st.done) {
    const uint64_t thr = L.st.thr;
    for (int64_t e = tid; e < total_slots; e += T) {
      const int c = (int)(e / cap), i = (int)(e - (int64_t)c * cap);
      if (i >= cnt[c]) continue;
      const float v = c_val[base + e];
      const uint64_t key = ((uint64_t)score_key(v) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c_id[base + e]);
      if (key < thr) continue;
      const uint32_t slot = atomicAdd(&L.out, 1u);
      if (slot < (uint32_t)SEL_K_MAX) { L.key[slot] = key; L.val[slot] = v; }
    }
  }
  __syncthreads();
  return min((int)L.out, min(K, SEL_K_MAX));
}

// The order of the m survivors by counting, descending key: put(place, id, val) for each, then put(place, -1, -inf) for the places
// m .. K-1 that nothing fills.
template <int T, class Put>
__device__ __forceinline__ void merge_order(const MergeSel& L, int m, int K, Put put) {
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += T) {
    const uint64_t ki = L.key[i];
    int pos = 0;
    for (int j = 0; j < m; ++j) pos += L.key[j] > ki ? 1 : 0;   // keys are unique: a permutation of 0 .. m-1
    put(pos, (int64_t)(0xFFFFFFFFu - (uint32_t)(ki & 0xFFFFFFFFu)), L.val[i]);
  }
  for (int p = m + tid; p < K; p += T) put(p, (int64_t)-1, -INFINITY);
}

}  // namespace
