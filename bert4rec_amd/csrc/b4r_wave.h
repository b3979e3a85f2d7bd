// Integer reductions over the 64 lanes of a wave, and the order-preserving integer image of an fp32 value, stated once for the
// catalogue sweeps (through b4r_select.h) and the pool kernels (b4r_rerank.hip, b4r_list_metrics.hip, b4r_group_mass.hip,
// b4r_audience.hip, b4r_rollout.hip, b4r_explain.hip).  The float reductions are b4r_common.h's b4r_wave_sum / b4r_wave_max.
#pragma once
#include "b4r_common.h"

namespace {

// ---- butterflies: every lane ends with the result of all 64 ---------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the order-preserving image of an fp32 value: a > b <=> image(a) > image(b) as unsigned integers; -0.0 counts as +0.0 (they
// compare equal).  Never 0 for a non-NaN value (-inf gives 0x007FFFFF), so 0 is free to mark a dead entry.
//
// One function in two wordings.  score_key_bits / score_key fold -0.0 on the bits, order_image folds it on the float; every input
// gives the same image.  Both stay because the compiler does not treat them alike: with the float wording every sweep, merge and
// MMR instance compiles to other code (the sweeps, which hold their scores as raw bits, in thousands of lines), and with the bit
// wording the three kernels that use order_image do (b4r_audience.hip's merge in 1 756 lines).  A kernel keeps
// the wording it was measured with.
__device__ __forceinline__ uint32_t score_key_bits(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t score_key(float s) { return score_key_bits(__builtin_bit_cast(uint32_t, s)); }
// the value whose image is k (+0.0 for the image of the zeros)
__device__ __forceinline__ float score_key_value(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ uint32_t order_image(float x) {
  if (x == 0.0f) x = 0.0f;
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace
