// Stock-aware allocation (include/b4r.h: b4r_allocate): limited items are shared out among the users of a batch.  The result is
// defined as one greedy walk over all live pool entries ("edges") in a global order; it is computed as deferred acceptance with the
// users proposing, in rounds that are separate launches.
//
// The state lives in the caller's scratch (int32 words): ctl [16] | ptr [R] | cap [V] | rem [V] | s_item | s_key | s_flat | s_flag |
// tile_hot, the four in the middle [R * K], slot s = r * K + k being the k-th of the K places of row r, the last [ceil(R K / 256)].
//   ptr[r]      the next pool position row r proposes from; it only ever advances
//   cap[j]      the call's copy of capacity[j] (the caller may overwrite capacity with `remaining` between resumed calls)
//   rem[j]      cap[j] minus the slots that hold item j; below 0 while the item is over-subscribed
//   s_item[s]   the item a slot holds, -1 for an empty slot;  s_key[s] its utility's order image;  s_flat[s] = r * M + pool position
//   s_flag[s]   1: the last resolve rejected the holder; the slot is cleared by the next propose and skipped by the finish
//   tile_hot[b] 1: one of the slots 256 b .. 256 b + 255 holds an over-subscribed item
//
//   allocate_init_kernel     empties the state and copies the capacities.
//   allocate_propose_kernel  one wave per row.  The lanes walk the row's K slots 64 at a time: a rejected slot is cleared (rem += 1),
//                            the empty slots are listed in LDS by ballot ranks.  Then they walk the pool 64 entries at a time from
//                            ptr[r]: the q-th live entry goes into the q-th empty slot (rem -= 1) until none is empty or the pool
//                            ends.  No decision reads rem here.
//   allocate_mark_kernel     one thread per slot: tile_hot of every tile of 256 slots.
//   allocate_resolve_kernel  one thread per slot, 256 slots per workgroup.  A workgroup whose tile is not hot returns; the others
//                            stream the hot tiles through LDS, four to a pass, and every slot of an over-subscribed item counts
//                            the holders of its item that precede it in the global order.  A count >= cap rejects the slot: the
//                            flag is written to s_flag, which no thread of this launch reads, so every count sees the same
//                            snapshot.  The workgroup adds its rejections to the round's counter.
//   allocate_finish_kernel   one thread per slot: the row's kept slots in ascending pool position, the -1 tail, row_n; one thread
//                            per item: remaining; one thread: unsettled.  It changes no state but the counter word a resumed call
//                            starts from.  After a resolve exactly -rem[j] holders of an over-subscribed item j are flagged, so
//                            remaining[j] = 0 there and rem[j] everywhere else.
//
// Round t reads the rejections of round t - 1 from ctl.rej[(t + 1) & 1] and returns at once when they are 0 or ctl.done is set (the
// first thread then sets ctl.done: every workgroup evaluates the same predicate, whichever value of done it sees); its resolve adds
// to ctl.rej[t & 1], which its propose cleared.  No workgroup waits for another, every loop bound is known on entry, the only
// atomics are integer adds whose results no thread branches on within the launch, so the bits do not depend on the schedule.
#include "b4r_common.h"
#include "b4r_wave.h"

namespace {

constexpr int AT = 256;                          // threads per workgroup (4 waves), every kernel; the resolve's LDS tile
constexpr int ROWS_PER_WG = AT / 64;             // propose: one wave per row
constexpr int RESOLVE_TILES = 4;                 // resolve: tiles of 256 slots per pass through LDS
constexpr int ALLOC_MAX_M = 1024;
constexpr int64_t ALLOC_MAX_SLOTS = (int64_t)1 << 20;   // R * K
constexpr int64_t ALLOC_MAX_ROWS = (int64_t)1 << 20;    // R (R * M stays at or below 2^30)
constexpr int CTL_WORDS = 16;

struct Ctl {                                     // the first 16 words of the scratch
  int32_t done;                                  // a round found nothing left to do
  int32_t rej[2];                                // the rejections of the rounds, by round parity; rej[1] = the round before round 0
  int32_t R, M, K, V;                            // the shape the state was initialised for
  int32_t pad[9];
};
static_assert(sizeof(Ctl) == CTL_WORDS * 4, "Ctl is 16 words");

struct AllocArgs {
  const int64_t* pool_ids; const float* pool_util; const int64_t* user_ids;
  Ctl* ctl; int32_t* ptr; int32_t* cap; int32_t* rem; int32_t* s_item; uint32_t* s_key; uint32_t* s_flat; int32_t* s_flag;
  int32_t* tile_hot;
  int R, M, K, V, slots, tiles;                  // slots = R * K, tiles = ceil(slots / 256)
};

__device__ __forceinline__ bool same_shape(const Ctl* c, const AllocArgs& a) {
  return c->R == a.R && c->M == a.M && c->K == a.K && c->V == a.V;
}

__global__ __launch_bounds__(AT) void allocate_init_kernel(AllocArgs a, const int32_t* capacity) {
  const int64_t i = (int64_t)blockIdx.x * AT + threadIdx.x;
  if (i < a.slots) {
    a.s_item[i] = -1;
    a.s_key[i] = 0;
    a.s_flat[i] = 0;
    a.s_flag[i] = 0;
  }
  if (i < a.tiles) a.tile_hot[i] = 0;
  if (i < a.R) a.ptr[i] = 0;
  if (i < a.V) {
    const int32_t c = capacity[i];
    a.cap[i] = c;
    a.rem[i] = c;
  }
  if (i == 0) {
    Ctl c{};
    c.rej[1] = 1;                                // "the round before" rejected something: round 0 runs
    c.R = a.R; c.M = a.M; c.K = a.K; c.V = a.V;
    *a.ctl = c;
  }
}

// true: the round has nothing to do.  Uniform over the whole launch.
__device__ __forceinline__ bool round_settled(const AllocArgs& a, int t) {
  const Ctl* c = a.ctl;
  return !same_shape(c, a) || c->done != 0 || c->rej[(t + 1) & 1] == 0;
}

__global__ __launch_bounds__(AT) void allocate_propose_kernel(AllocArgs a, int t) {
  __shared__ uint16_t s_empty[ROWS_PER_WG][ALLOC_MAX_M];   // per wave: the row's empty slots, ascending
  const bool shape_ok = same_shape(a.ctl, a);
  if (round_settled(a, t)) {
    if (shape_ok && blockIdx.x == 0 && threadIdx.x == 0) a.ctl->done = 1;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->rej[t & 1] = 0;   // this round's counter: nobody reads or adds to it in this launch
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = blockIdx.x * ROWS_PER_WG + wv;
  const bool row = r < a.R;
  const int base = row ? r * a.K : 0;            // r * K < slots <= 2^20
  const uint64_t below = (1ull << lane) - 1ull;
  int n_empty = 0;
  for (int k0 = 0; k0 < a.K; k0 += 64) {         // the same trip count in every wave of the workgroup
    const int k = k0 + lane;
    bool empty = false;
    if (row && k < a.K) {
      const int32_t it = a.s_item[base + k];
      empty = it < 0;
      if (!empty && a.s_flag[base + k]) {        // the rejection the last resolve flagged
        if (it < a.V) atomicAdd(&a.rem[it], 1);
        a.s_item[base + k] = -1;
        a.s_flag[base + k] = 0;
        empty = true;
      }
    }
    const uint64_t m = __ballot(empty);
    if (empty) s_empty[wv][n_empty + __popcll(m & below)] = (uint16_t)k;   // n_empty + rank < K <= 1024
    n_empty += __popcll(m);
  }
  __syncthreads();
  if (!row || n_empty == 0) return;              // wave-uniform; no barrier below
  int p0 = a.ptr[r];
  if (p0 < 0) p0 = 0;                            // (a state this library wrote holds 0 <= p0 <= M)
  if (p0 >= a.M) return;
  const int64_t rowoff = (int64_t)r * a.M;
  int taken = 0, next = a.M;
  for (int b = p0; b < a.M; b += 64) {           // at most ceil(M / 64) chunks
    const int p = b + lane;
    bool live = false;
    int64_t id = -1;
    float u = 0.0f;
    if (p < a.M) {
      id = a.pool_ids[rowoff + p];
      u = a.pool_util[rowoff + p];
      live = id >= 0 && id < a.V && fabsf(u) < INFINITY;
      if (live) live = a.cap[id] > 0;
    }
    const uint64_t m = __ballot(live);
    const int q = taken + __popcll(m & below);   // this entry is the row's q-th proposal of the round
    if (live && q < n_empty) {
      const int k = s_empty[wv][q];
      a.s_item[base + k] = (int32_t)id;
      a.s_key[base + k] = order_image(u);
      a.s_flat[base + k] = (uint32_t)(rowoff + p);
      atomicSub(&a.rem[id], 1);
    }
    const uint64_t last = __ballot(live && q == n_empty - 1);
    taken += __popcll(m);
    if (last) {                                  // the entry that filled the last empty slot: the pointer stops behind it
      next = b + __ffsll((long long)last);
      break;
    }
  }
  if (lane == 0) a.ptr[r] = next;
}

__global__ __launch_bounds__(AT) void allocate_mark_kernel(AllocArgs a, int t) {
  if (round_settled(a, t)) return;
  const int s = blockIdx.x * AT + threadIdx.x;
  bool hot = false;
  if (s < a.slots) {
    const int32_t it = a.s_item[s];
    if (it >= 0 && it < a.V) hot = a.rem[it] < 0;
  }
  const int any = __syncthreads_or(hot ? 1 : 0);
  if (threadIdx.x == 0) a.tile_hot[blockIdx.x] = any ? 1 : 0;
}

template <bool HAS_UID>
__global__ __launch_bounds__(AT) void allocate_resolve_kernel(AllocArgs a, int t) {
  // without user ids the order is one 64-bit word per holder: the inverted utility image above the flat pool index (row, position)
  constexpr int PASS = RESOLVE_TILES * AT;       // holders per pass through LDS
  __shared__ __attribute__((aligned(16))) int32_t s_it[PASS];
  __shared__ __attribute__((aligned(16))) uint64_t s_w[PASS];          // HAS_UID: the user id (as its bits)
  __shared__ __attribute__((aligned(16))) uint32_t s_ky[HAS_UID ? PASS : 4];
  __shared__ __attribute__((aligned(16))) uint32_t s_fl[HAS_UID ? PASS : 4];
  __shared__ int s_rej[AT / 64];
  if (round_settled(a, t)) return;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  if (!a.tile_hot[tile]) return;                 // workgroup-uniform: nothing of this tile can be rejected
  const int s = tile * AT + tid;
  int32_t it = -1, cap = 0;
  uint32_t ky = 0, fl = 0;
  uint64_t w = 0;
  bool contested = false;
  if (s < a.slots) {
    it = a.s_item[s];
    if (it >= a.V) it = -1;                      // (a state this library wrote holds -1 or an id below V)
    if (it >= 0) {
      ky = a.s_key[s];
      fl = a.s_flat[s];
      w = HAS_UID ? (uint64_t)a.user_ids[s / a.K] : ((uint64_t)(~ky) << 32) | fl;
      cap = a.cap[it];
      contested = a.rem[it] < 0;
    }
  }
  int before = 0;
  for (int t0 = 0; t0 < a.tiles; t0 += RESOLVE_TILES) {   // workgroup-uniform trip count and skips: the barriers see whole workgroups
    int hot = 0;
#pragma unroll
    for (int u = 0; u < RESOLVE_TILES; ++u)
      if (t0 + u < a.tiles && a.tile_hot[t0 + u]) hot |= 1 << u;
    if (!hot) continue;                          // no holder of an over-subscribed item in these tiles
#pragma unroll
    for (int u = 0; u < RESOLVE_TILES; ++u) {    // independent loads: their latencies overlap
      int32_t it2 = -1;
      uint32_t ky2 = 0, fl2 = 0;
      uint64_t w2 = 0;
      const int m = (t0 + u) * AT + tid;
      if (((hot >> u) & 1) && m < a.slots) {
        it2 = a.s_item[m];
        if (it2 >= a.V) it2 = -1;
        if (it2 >= 0) {
          ky2 = a.s_key[m];
          fl2 = a.s_flat[m];
          w2 = HAS_UID ? (uint64_t)a.user_ids[m / a.K] : ((uint64_t)(~ky2) << 32) | fl2;
        }
      }
      s_it[u * AT + tid] = it2;
      s_w[u * AT + tid] = w2;
      if (HAS_UID) {
        s_ky[u * AT + tid] = ky2;
        s_fl[u * AT + tid] = fl2;
      }
    }
    __syncthreads();
    if (contested) {                             // it >= 0 never equals the -1 of an empty or absent slot
      const int4* s_it4 = reinterpret_cast<const int4*>(s_it);       // four holders per LDS read, the same address in every lane
      const ulonglong2* s_w2 = reinterpret_cast<const ulonglong2*>(s_w);
      for (int u = 0; u < RESOLVE_TILES; ++u) {
        if (!((hot >> u) & 1)) continue;
#pragma unroll 4
        for (int j = u * (AT / 4); j < (u + 1) * (AT / 4); ++j) {
          const int4 q = s_it4[j];
          const ulonglong2 wa = s_w2[2 * j], wb = s_w2[2 * j + 1];
          if (HAS_UID) {
            const uint4 k4 = reinterpret_cast<const uint4*>(s_ky)[j], f4 = reinterpret_cast<const uint4*>(s_fl)[j];
            const int64_t ua = (int64_t)w;
#define B4R_ALLOC_BEFORE(qi, ki, ui, fi) \
  ((qi == it) & ((ki > ky) | ((ki == ky) & (((int64_t)(ui) < ua) | (((int64_t)(ui) == ua) & (fi < fl))))))
            before += B4R_ALLOC_BEFORE(q.x, k4.x, wa.x, f4.x) + B4R_ALLOC_BEFORE(q.y, k4.y, wa.y, f4.y) +
                      B4R_ALLOC_BEFORE(q.z, k4.z, wb.x, f4.z) + B4R_ALLOC_BEFORE(q.w, k4.w, wb.y, f4.w);
#undef B4R_ALLOC_BEFORE
          } else {
            before += ((q.x == it) & (wa.x < w)) + ((q.y == it) & (wa.y < w)) + ((q.z == it) & (wb.x < w)) + ((q.w == it) & (wb.y < w));
          }
        }
      }
    }
    __syncthreads();
  }
  const bool rejected = contested && before >= cap;
  if (rejected) a.s_flag[s] = 1;
  const unsigned long long votes = __ballot(rejected);
  if ((tid & 63) == 0) s_rej[tid >> 6] = __popcll(votes);
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int wv = 0; wv < AT / 64; ++wv) n += s_rej[wv];
    if (n > 0) atomicAdd(&a.ctl->rej[t & 1], n);
  }
}

struct FinishArgs {
  int64_t* out_ids; float* out_util; int32_t* out_pos; int32_t* row_n; int32_t* remaining; int32_t* unsettled;
  int last_round;
};

__global__ __launch_bounds__(AT) void allocate_finish_kernel(AllocArgs a, FinishArgs f) {
  const bool shape_ok = same_shape(a.ctl, a);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int32_t u = -1;                              // -1: the scratch does not hold a state of this shape; nothing else is written
    if (shape_ok) {
      u = a.ctl->done ? 0 : a.ctl->rej[f.last_round & 1];
      a.ctl->rej[1] = u;                         // where round 0 of a resumed call reads "the round before"
    }
    if (f.unsettled) *f.unsettled = u;
  }
  if (!shape_ok) return;
  if ((int)blockIdx.x >= a.tiles) {              // one thread per item
    const int64_t j = (int64_t)(blockIdx.x - a.tiles) * AT + threadIdx.x;
    if (j < a.V && f.remaining) {
      const int32_t c = a.cap[j], m = a.rem[j];
      f.remaining[j] = (c > 0 && m < 0) ? 0 : m;
    }
    return;
  }
  const int s = blockIdx.x * AT + threadIdx.x;   // one thread per slot
  if (s >= a.slots) return;
  const int r = s / a.K, k = s - r * a.K;
  const int base = r * a.K;
  const int32_t it = a.s_item[s];
  const bool mine = it >= 0 && it < a.V && !a.s_flag[s];
  const uint32_t flat = a.s_flat[s];
  int n = 0, rank = 0;
  for (int q = 0; q < a.K; ++q) {                // pool positions are distinct within a row
    const int32_t it2 = a.s_item[base + q];
    if (it2 < 0 || it2 >= a.V || a.s_flag[base + q]) continue;
    ++n;
    rank += a.s_flat[base + q] < flat ? 1 : 0;
  }
  const int64_t pos = (int64_t)flat - (int64_t)r * a.M;
  if (mine && pos >= 0 && pos < a.M) {           // rank < n <= K
    if (f.out_ids) f.out_ids[base + rank] = a.pool_ids[flat];
    if (f.out_util) f.out_util[base + rank] = a.pool_util[flat];
    if (f.out_pos) f.out_pos[base + rank] = (int32_t)pos;
  }
  if (k >= n) {                                  // the tail: places n .. K-1, one per slot index
    if (f.out_ids) f.out_ids[base + k] = -1;
    if (f.out_util) f.out_util[base + k] = -INFINITY;
    if (f.out_pos) f.out_pos[base + k] = -1;
  }
  if (k == 0 && f.row_n) f.row_n[r] = n;
}

int64_t scratch_words(int64_t R, int64_t K, int64_t V) { return CTL_WORDS + R + 2 * V + 4 * R * K + (R * K + AT - 1) / AT; }

bool shape_ok(int32_t R, int32_t M, int32_t K, int32_t V) {
  return R >= 0 && R <= ALLOC_MAX_ROWS && M >= 1 && M <= ALLOC_MAX_M && K >= 0 && K <= M && V >= 1 && (int64_t)R * K <= ALLOC_MAX_SLOTS;
}

}  // namespace

extern "C" int64_t b4r_allocate_scratch_bytes(int32_t R, int32_t M, int32_t K, int32_t V) {
  if (!shape_ok(R, M, K, V)) {
    b4r_set_error("b4r_allocate_scratch_bytes: bad shape (R = %d in [0, 2^20], M = %d in [1, %d], K = %d in [0, M], V = %d >= 1, R * K <= 2^20)",
                  R, M, ALLOC_MAX_M, K, V);
    return -1;
  }
  return 4 * scratch_words(R, K, V);
}

extern "C" int b4r_allocate(const int64_t* pool_ids, const float* pool_util, int32_t R, int32_t M, int32_t K, int32_t V,
                            const int32_t* capacity, const int64_t* user_ids, int32_t rounds, int32_t resume, int64_t* out_ids,
                            float* out_util, int32_t* out_pos, int32_t* row_n, int32_t* remaining, int32_t* unsettled, void* scratch,
                            int64_t scratch_bytes, b4r_stream_t stream) {
  const char* what = "b4r_allocate";
  B4R_CHECK_ARG(shape_ok(R, M, K, V), B4R_E_SHAPE,
                "%s: bad shape (R = %d in [0, 2^20], M = %d in [1, %d], K = %d in [0, M], V = %d >= 1, R * K <= 2^20)", what, R, M,
                ALLOC_MAX_M, K, V);
  B4R_CHECK_ARG(rounds >= 1 && (resume == 0 || resume == 1), B4R_E_BADARG, "%s: rounds = %d must be >= 1 and resume = %d must be 0 or 1",
                what, rounds, resume);
  B4R_CHECK_ARG(capacity, B4R_E_BADARG, "%s: null argument (capacity)", what);
  hipStream_t st = (hipStream_t)stream;
  if (R == 0 || K == 0) {                        // no row output to write; the stock is untouched
    if (remaining && remaining != capacity) {
      hipError_t e = hipMemcpyAsync(remaining, capacity, (size_t)V * 4, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) {
        b4r_set_error("%s: copying the capacities failed: %s", what, hipGetErrorString(e));
        return B4R_E_HIP;
      }
    }
    return B4R_OK;
  }
  B4R_CHECK_ARG(pool_ids && pool_util && scratch, B4R_E_BADARG, "%s: null argument (pool_ids, pool_util or scratch)", what);
  B4R_CHECK_ARG((((uintptr_t)scratch) & 7u) == 0, B4R_E_BADARG, "%s: the scratch is not 8-byte aligned", what);
  const int64_t need = 4 * scratch_words(R, K, V);
  B4R_CHECK_ARG(scratch_bytes >= need, B4R_E_NOMEM, "%s: scratch of %lld bytes, %lld needed", what, (long long)scratch_bytes,
                (long long)need);
  const int slots = R * K;
  int32_t* w = (int32_t*)scratch;
  AllocArgs a{};
  a.pool_ids = pool_ids; a.pool_util = pool_util; a.user_ids = user_ids;
  a.ctl = (Ctl*)w;
  a.ptr = w + CTL_WORDS;
  a.cap = a.ptr + R;
  a.rem = a.cap + V;
  a.s_item = a.rem + V;
  a.s_key = (uint32_t*)(a.s_item + slots);
  a.s_flat = (uint32_t*)(a.s_item + 2 * (int64_t)slots);
  a.s_flag = a.s_item + 3 * (int64_t)slots;
  a.tile_hot = a.s_item + 4 * (int64_t)slots;
  a.R = R; a.M = M; a.K = K; a.V = V; a.slots = slots; a.tiles = b4r_cdiv(slots, AT);
  const int row_blocks = b4r_cdiv(R, ROWS_PER_WG), item_blocks = b4r_cdiv(V, AT);
  if (!resume) {
    const int n = a.tiles > item_blocks ? a.tiles : item_blocks;   // slots >= R: the rows are covered
    hipLaunchKernelGGL(allocate_init_kernel, dim3(n), dim3(AT), 0, st, a, capacity);
    B4R_CHECK_LAUNCH(what);
  }
  for (int t = 0; t < rounds; ++t) {
    hipLaunchKernelGGL(allocate_propose_kernel, dim3(row_blocks), dim3(AT), 0, st, a, t);
    B4R_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(allocate_mark_kernel, dim3(a.tiles), dim3(AT), 0, st, a, t);
    B4R_CHECK_LAUNCH(what);
    if (user_ids)
      hipLaunchKernelGGL(allocate_resolve_kernel<true>, dim3(a.tiles), dim3(AT), 0, st, a, t);
    else
      hipLaunchKernelGGL(allocate_resolve_kernel<false>, dim3(a.tiles), dim3(AT), 0, st, a, t);
    B4R_CHECK_LAUNCH(what);
  }
  FinishArgs f{out_ids, out_util, out_pos, row_n, remaining, unsettled, rounds - 1};
  hipLaunchKernelGGL(allocate_finish_kernel, dim3(a.tiles + item_blocks), dim3(AT), 0, st, a, f);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
