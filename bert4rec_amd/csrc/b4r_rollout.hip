// Multi-step roll-outs (include/b4r.h: b4r_beam_select, b4r_rollout_advance): the device-side step logic between two forwards of a
// greedy, beam or sampled roll-out.  The scores of a step come from the existing sweeps (b4r_rank_full, b4r_score_dist,
// b4r_sample_full); the two kernels here choose the next beams across the parents and build the next step's batch rows, so that no
// step reads anything back to the host.
//
//   beam_select_kernel      one workgroup per user.  The Bm * C <= 4096 entries of the user go into LDS as the order-preserving image
//                           of total = fl32(beam_logp + cand_logp) (0 marks a dead entry; no live total has the image 0); every live
//                           entry counts the entries that come before it in (total descending, flat index ascending) and, when that
//                           count is below Bout, writes itself there.  The order is strict, so every output cell has one writer.
//   rollout_advance_kernel  one workgroup per output row: copy / slide the token window of the parent row, append the chosen item and
//                           the [MASK] placeholder, carry the exclusion list and the path.
//
// No atomics, no floating-point reduction: the bits do not depend on the launch.  Both entry points check every argument before
// the launch and only enqueue.
#include <cmath>

#include "b4r_common.h"
#include "b4r_wave.h"   // order_image

namespace {

constexpr int RT = 256;            // threads per workgroup (4 waves), both kernels
constexpr int BS_MAX_BEAMS = 64;   // Bm, Bout
constexpr int BS_MAX_CAND = 1024;  // C
constexpr int BS_MAX_ENTRIES = 4096;

struct BeamArgs {
  const float* beam_logp; const int64_t* cand_ids; const float* cand_logp;
  int32_t* out_parent; int64_t* out_item; float* out_logp; float* out_step_logp;
  int Bm, C, Bout;
};

__global__ __launch_bounds__(RT) void beam_select_kernel(BeamArgs a) {
  __shared__ uint32_t s_img[BS_MAX_ENTRIES];
  __shared__ float s_beam[BS_MAX_BEAMS];
  __shared__ int s_wave_live[RT / 64];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int n = a.Bm * a.C;                                  // <= BS_MAX_ENTRIES (checked on the host)
  const int64_t base = u * (int64_t)n;                       // row (u * Bm + b) of [U * Bm, C], column c: base + b * C + c
  for (int b = tid; b < a.Bm; b += RT) s_beam[b] = a.beam_logp[u * a.Bm + b];
  __syncthreads();
  int live = 0;
  for (int i0 = 0; i0 < n; i0 += RT) {                       // uniform trip count: the ballot below sees whole waves
    const int i = i0 + tid;
    bool ok = false;
    uint32_t img = 0;
    if (i < n) {
      const float bl = s_beam[i / a.C];
      const float cl = a.cand_logp[base + i];
      ok = bl > -INFINITY && cl > -INFINITY && a.cand_ids[base + i] >= 0;
      if (ok) img = order_image(bl + cl);
      s_img[i] = ok ? img : 0u;
    }
    live += __popcll(__ballot(ok));
  }
  if ((tid & 63) == 0) s_wave_live[tid >> 6] = live;
  __syncthreads();
  int n_live = 0;
  for (int w = 0; w < RT / 64; ++w) n_live += s_wave_live[w];
  for (int i = tid; i < n; i += RT) {
    const uint32_t ki = s_img[i];
    if (ki == 0u) continue;
    int pos = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t kj = s_img[j];
      pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0;         // kj >= ki > 0: a dead j never counts
    }
    if (pos >= a.Bout) continue;
    const int64_t o = u * a.Bout + pos;
    const int b = i / a.C;
    const float cl = a.cand_logp[base + i];
    if (a.out_parent) a.out_parent[o] = b;
    if (a.out_item) a.out_item[o] = a.cand_ids[base + i];
    if (a.out_logp) a.out_logp[o] = s_beam[b] + cl;
    if (a.out_step_logp) a.out_step_logp[o] = cl;
  }
  for (int p = n_live + tid; p < a.Bout; p += RT) {
    const int64_t o = u * a.Bout + p;
    if (a.out_parent) a.out_parent[o] = -1;
    if (a.out_item) a.out_item[o] = -1;
    if (a.out_logp) a.out_logp[o] = -INFINITY;
    if (a.out_step_logp) a.out_step_logp[o] = -INFINITY;
  }
}

struct AdvanceArgs {
  const int64_t* tokens_in; const int32_t* len_in; const int64_t* exclude_in; const int64_t* path_in; const float* path_logp_in;
  const int32_t* parent; const int64_t* item; const float* item_logp;
  int64_t* tokens_out; int64_t* mask_out; int32_t* len_out; int64_t* positions_out; int64_t* exclude_out; int64_t* path_out;
  float* path_logp_out;
  int64_t mask_id;
  int G_in, G_out, L, P, E, T, V, first_item, t, ex_col;
};

__global__ __launch_bounds__(RT) void rollout_advance_kernel(AdvanceArgs a) {
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  const int64_t group0 = n / a.G_out * a.G_in;               // the first input row of the output row's group
  const int par = a.parent ? a.parent[n] : (int)(n - n / a.G_out * a.G_out);   // parent NULL: G_in == G_out, s = n
  const int64_t it = a.item[n];
  const bool live = par >= 0 && par < a.G_in && it >= a.first_item && it < a.V;
  const int64_t s = live ? group0 + par : group0;            // always a row of the input
  int len = a.len_in[s];
  len = len < 1 ? 1 : (len > a.L ? a.L : len);
  const int64_t* src = a.tokens_in + s * a.L;
  int64_t* dst = a.tokens_out + n * a.L;
  int len_o = len;
  if (!live) {
    for (int p = tid; p < a.L; p += RT) dst[p] = src[p];
  } else if (len < a.L) {
    len_o = len + 1;
    for (int p = tid; p < a.L; p += RT)
      dst[p] = p < len - 1 ? src[p] : (p == len - 1 ? it : (p == len ? a.mask_id : (int64_t)0));
  } else {
    for (int p = tid; p < a.L; p += RT)
      dst[p] = p <= a.L - 3 ? src[p + 1] : (p == a.L - 2 ? it : a.mask_id);
  }
  for (int p = tid; p < a.L; p += RT) a.mask_out[n * a.L + p] = p < len_o ? 1 : 0;
  for (int p = tid; p < a.P; p += RT) a.positions_out[n * a.P + p] = p == 0 ? (int64_t)(len_o - 1) : (int64_t)0;
  if (tid == 0) a.len_out[n] = len_o;
  for (int e = tid; e < a.E; e += RT) a.exclude_out[n * a.E + e] = (live && e == a.ex_col) ? it : a.exclude_in[s * a.E + e];
  if (a.path_out)
    for (int c = tid; c < a.T; c += RT)
      a.path_out[n * a.T + c] = !live ? (int64_t)-1 : (c == a.t ? it : (a.path_in ? a.path_in[s * a.T + c] : (int64_t)-1));
  if (a.path_logp_out)
    for (int c = tid; c < a.T; c += RT)
      a.path_logp_out[n * a.T + c] =
          !live ? -INFINITY : (c == a.t ? a.item_logp[n] : (a.path_logp_in ? a.path_logp_in[s * a.T + c] : -INFINITY));
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

extern "C" int b4r_beam_select(const float* beam_logp, const int64_t* cand_ids, const float* cand_logp, int32_t U, int32_t Bm, int32_t C,
                               int32_t Bout, int32_t* out_parent, int64_t* out_item, float* out_logp, float* out_step_logp,
                               b4r_stream_t stream) {
  const char* what = "b4r_beam_select";
  B4R_CHECK_ARG(U >= 0 && Bm >= 1 && Bm <= BS_MAX_BEAMS && C >= 1 && C <= BS_MAX_CAND && (int64_t)Bm * C <= BS_MAX_ENTRIES &&
                    Bout >= 1 && Bout <= BS_MAX_BEAMS,
                B4R_E_SHAPE, "%s: bad shape (U = %d, Bm = %d in [1, %d], C = %d in [1, %d], Bm * C <= %d, Bout = %d in [1, %d])", what, U,
                Bm, BS_MAX_BEAMS, C, BS_MAX_CAND, BS_MAX_ENTRIES, Bout, BS_MAX_BEAMS);
  if (U == 0) return B4R_OK;
  B4R_CHECK_ARG(beam_logp && cand_ids && cand_logp, B4R_E_BADARG, "%s: null argument", what);
  BeamArgs ba{beam_logp, cand_ids, cand_logp, out_parent, out_item, out_logp, out_step_logp, Bm, C, Bout};
  hipLaunchKernelGGL(beam_select_kernel, dim3(U), dim3(RT), 0, (hipStream_t)stream, ba);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}

extern "C" int b4r_rollout_advance(const int64_t* tokens_in, const int32_t* len_in, const int64_t* exclude_in, const int64_t* path_in,
                                   const float* path_logp_in, const int32_t* parent, const int64_t* item, const float* item_logp,
                                   int32_t N_in, int32_t N_out, int32_t G_in, int32_t G_out, int32_t L, int32_t P, int32_t E, int32_t T,
                                   int32_t V, int32_t first_item, int64_t mask_id, int32_t t, int32_t ex_col, int64_t* tokens_out,
                                   int64_t* input_mask_out, int32_t* len_out, int64_t* positions_out, int64_t* exclude_out,
                                   int64_t* path_out, float* path_logp_out, b4r_stream_t stream) {
  const char* what = "b4r_rollout_advance";
  B4R_CHECK_ARG(L >= 2 && P >= 1 && E >= 1 && T >= 1 && V >= 1 && first_item >= 0, B4R_E_SHAPE,
                "%s: bad shape (L = %d >= 2, P = %d >= 1, E = %d >= 1, T = %d >= 1, V = %d, first_item = %d)", what, L, P, E, T, V,
                first_item);
  B4R_CHECK_ARG(t >= 0 && t < T && ex_col >= 0 && ex_col < E, B4R_E_SHAPE, "%s: t = %d outside [0, %d) or ex_col = %d outside [0, %d)",
                what, t, T, ex_col, E);
  B4R_CHECK_ARG(N_in >= 0 && N_out >= 0 && G_in >= 1 && G_out >= 1 && N_in % G_in == 0 && N_out % G_out == 0 &&
                    N_in / G_in == N_out / G_out,
                B4R_E_SHAPE, "%s: %d rows in groups of %d do not map onto %d rows in groups of %d", what, N_in, G_in, N_out, G_out);
  B4R_CHECK_ARG(parent || G_in == G_out, B4R_E_SHAPE, "%s: parent is NULL with G_in = %d != G_out = %d", what, G_in, G_out);
  if (N_out == 0) return B4R_OK;
  B4R_CHECK_ARG(tokens_in && len_in && exclude_in && item && tokens_out && input_mask_out && len_out && positions_out && exclude_out,
                B4R_E_BADARG, "%s: null argument", what);
  B4R_CHECK_ARG(!path_logp_out || item_logp, B4R_E_BADARG, "%s: path_logp_out needs item_logp", what);
  const int64_t ni = N_in, no = N_out;
  B4R_CHECK_ARG(!overlaps(tokens_out, no * L * 8, tokens_in, ni * L * 8) && !overlaps(input_mask_out, no * L * 8, tokens_in, ni * L * 8) &&
                    !overlaps(len_out, no * 4, len_in, ni * 4) && !overlaps(exclude_out, no * E * 8, exclude_in, ni * E * 8) &&
                    !overlaps(path_out, no * T * 8, path_in, ni * T * 8) && !overlaps(path_logp_out, no * T * 4, path_logp_in, ni * T * 4),
                B4R_E_BADARG, "%s: an output aliases its input (the rows are re-ordered: use the other buffer of a ping-pong pair)", what);
  AdvanceArgs aa{tokens_in, len_in, exclude_in, path_in, path_logp_in, parent, item, item_logp, tokens_out, input_mask_out, len_out,
                 positions_out, exclude_out, path_out, path_logp_out, mask_id, G_in, G_out, L, P, E, T, V, first_item, t, ex_col};
  hipLaunchKernelGGL(rollout_advance_kernel, dim3(N_out), dim3(RT), 0, (hipStream_t)stream, aa);
  B4R_CHECK_LAUNCH(what);
  return B4R_OK;
}
