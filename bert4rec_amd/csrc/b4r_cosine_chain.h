// The cosine of two item-table rows as b4r_item_neighbours(B4R_SIM_COSINE) defines it (include/b4r.h), for the kernels that walk
// table rows against one query held in LDS: b4r_rerank_diverse / b4r_rerank_quota (the picked item is the query) and b4r_list_metrics
// (the earlier list position is the query).  One convention, stated once (mmr_kernel keeps b4r_cosine_chains' loop written out:
// DESIGN.md 6.3), and one launch that fills rnorm for all four entry points (b4r_item_rnorm_launch, b4r_internal.h):
//   rnorm[j]  = 1 / sqrt(max(sum_k table[j][k]^2, 1e-24f))                       one fp32 fma per element, k ascending
//   qhat[k]   = fl32(table[q][k] * rnorm[q])
//   sim(c, q) = fl32((fma-chain_k(qhat[k] * table[c][k]) + 0.0f) * rnorm[c])     k ascending, fp32, no MFMA
#pragma once
#include "b4r_common.h"

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline int64_t b4r_align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// The 16-byte aligned start of `scratch` when `need` bytes fit behind it; NULL when they do not or there is no scratch (the caller
// reports it in its own words).
inline char* b4r_scratch_carve(void* scratch, int64_t scratch_bytes, int64_t need) {
  const int64_t pad = scratch ? (int64_t)((16 - ((uintptr_t)scratch & 15)) & 15) : 0;
  return scratch && scratch_bytes - pad >= need ? reinterpret_cast<char*>(scratch) + pad : nullptr;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
// 1 / |row| of one table row of H floats (H % 4 == 0, 16-byte aligned): k ascending, one fp32 fma per element, a fixed order, so
// rnorm is bitwise reproducible
__device__ __forceinline__ float b4r_row_rnorm(const float* __restrict__ e, int H) {
  float ss = 0.f;
  for (int k = 0; k < H; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(e + k);
#pragma unroll
    for (int u = 0; u < 4; ++u) ss = __builtin_fmaf(v[u], v[u], ss);
  }
  return 1.0f / sqrtf(fmaxf(ss, 1e-24f));
}

// qhat = table[q] * rnorm[q] into LDS, by all `threads` threads of the workgroup (the caller puts the barriers around it)
__device__ __forceinline__ void b4r_stage_qhat(float* qhat, const float* table, const float* rnorm, int q, int width, int tid, int threads) {
  const float rq = rnorm[q];
  const float* e = table + (int64_t)q * width;
  for (int k = tid; k < width; k += threads) qhat[k] = e[k] * rq;
}

// acc[i] = fma-chain_k(qhat[k] * row[i][k]) for the thread's entries with on[i]; the others keep 0 and read nothing.  16-byte loads in
// ascending k; one LDS broadcast read of qhat per four fmas, shared by the thread's NPT chains.
template <int NPT>
__device__ __forceinline__ void b4r_cosine_chains(const float* qhat, const float* const (&row)[NPT], const bool (&on)[NPT], int width,
                                                  float (&acc)[NPT]) {
#pragma unroll
  for (int i = 0; i < NPT; ++i) acc[i] = 0.f;
#pragma unroll 4
  for (int k = 0; k < width; k += 4) {
    const f32x4 h = *reinterpret_cast<const f32x4*>(qhat + k);
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
      if (!on[i]) continue;
      const f32x4 e = *reinterpret_cast<const f32x4*>(row[i] + k);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[i] = __builtin_fmaf(h[u], e[u], acc[i]);   // k-ordered fp32 fma chain (the contract)
    }
  }
}
// sim(c, q) from the finished chain of c against qhat of q
__device__ __forceinline__ float b4r_cosine_close(float acc, float rnorm_c) { return (acc + 0.0f) * rnorm_c; }
