// Keras MultiHeadAttention core for heads of width 64 (hidden_size = 64 * num_heads), both arithmetic modes.
// Computes what b4r_attn.hip computes for width 32:
//
//   scores = q k^T + (1 - input_mask[b,key]) * -1e9 ; A = softmax(scores) ; A = dropout(A) ; ctx = A v
//   (q arrives pre-scaled by 1/sqrt(64); lse stored relative to the row's largest adder, b4r_seq_amax)
//
// Decomposition as in b4r_attn.hip: a wave owns 16 queries (16 keys in the dK / dV half of the backward) and sweeps the other
// dimension in 16-row tiles, with every score tile computed in the orientation whose accumulator rows are the index the next
// product sums over, so probabilities never move between lanes.  The backward is ONE launch: the first half of the grid forms dQ
// (workgroup = 128 queries), the second half dK and dV (workgroup = 128 keys); no cross-workgroup sums, bitwise reproducible.
//
// Products.  Every product is written as an 8-slot step: lane (i, g) supplies A[row i][slots 8g .. 8g+7] and B[slots][col i],
// the step adds sum over the 32 slots to a 16x16 accumulator (C/D map: col = lane & 15, row = 4 (lane >> 4) + reg).
//   * B4R_GEMM_BF16X3: one v_mfma_f32_16x16x32_bf16 per split term (x = hi + lo; Alo.Bhi + Ahi.Blo + Ahi.Bhi), the operands
//     split in registers (b4r_split8).
//   * B4R_GEMM_BF16: the same with the hi term only (Ahi.Bhi: operands rounded once to bf16, one MFMA per step).
//   * B4R_GEMM_F32: eight v_mfma_f32_16x16x4_f32, slot j of every lane group in the j-th (exact fp32 products).
// A product that consumes accumulator tiles takes two of them per step: slot (g, j) is row 16 t0 + 4g + j for j < 4 and row
// 16 t1 + 4g + j - 4 for j >= 4 (t0, t1 = an even / odd tile pair), on both operands.
//
// LDS: K and V (or Q and dO) as fp32 [rows][64] tiles, the 16-byte chunk index of a row XORed with (row & 15).  That makes the
// column reads of the accumulator-consuming products (rows 4g + j, columns 16c + i) conflict free and spreads the row reads of
// the others (16 rows, one 16-byte chunk each) over all banks.  K + V at L = 256 take 128 KiB, so a workgroup of 8 waves holds a
// CU on its own.  Dropout decisions are hashed again in the backward (nothing stored in keep_bits).
#include "b4r_common.h"

namespace {

constexpr int HD = 64;            // head width
constexpr int WAVES = 8;          // waves per workgroup
constexpr int ROWS_WG = 16 * WAVES;

struct Attn64P {
  const float* qkv; const int64_t* mask; const float* ctx; const float* lse_in; const float* dctx;
  float* ctx_out; float* lse_out; float* dqkv;
  int B, L, heads, H;
  int KT;      // 16-row tiles covering L, rounded up to even (backward)
  int nx;      // row blocks of 128 per (batch, head)
  float qscale;
  DropArgs drop;
};

// one operand of an 8-slot step: fp32 values, or their bf16 hi / lo split.  TERMS = bf16 MFMAs per step: 3 (B4R_GEMM_BF16X3),
// 1 (B4R_GEMM_BF16: the lo half is never read, so its split is dead code), 0 (B4R_GEMM_F32: the exact fp32 MFMAs)
struct Op8 {
  f32x8 v;
  b4r_bf16x8 h, l;
};
template <int TERMS>
__device__ __forceinline__ Op8 op8(const f32x8 x) {
  Op8 o;
  o.v = x;
  if constexpr (TERMS != 0) b4r_split8(x, o.h, o.l);
  return o;
}
template <int TERMS>
__device__ __forceinline__ f32x4 mma8(const Op8& a, const Op8& b, f32x4 c) {
  static_assert(TERMS == 0 || TERMS == 1 || TERMS == 3, "0 (fp32), 1 or 3 bf16 terms");
  if constexpr (TERMS != 0) {
    if constexpr (TERMS == 3) {
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, c, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  }
  return c;
}

__device__ __forceinline__ f32x8 cat(const f32x4 a, const f32x4 b) {
  return (f32x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ f32x8 load8(const float* ptr) {
  return cat(*reinterpret_cast<const f32x4*>(ptr), *reinterpret_cast<const f32x4*>(ptr + 4));
}

// swizzled float offset of (row, col) in a [rows][64] tile
__device__ __forceinline__ int tix(int row, int col) {
  return row * HD + ((((col >> 2) ^ (row & 15)) << 2) | (col & 3));
}

// rows [0,nrows) of a [*,64] head slice -> swizzled tile; rows beyond `valid` are zero
__device__ __forceinline__ void stage_rows(float* dst, const float* src, int64_t row0, int ld, int nrows, int valid) {
  for (int f = threadIdx.x; f < nrows * 16; f += 64 * WAVES) {
    const int r = f >> 4, c = f & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < valid) v = *reinterpret_cast<const f32x4*>(src + (row0 + r) * ld + 4 * c);
    *reinterpret_cast<f32x4*>(dst + r * HD + ((c ^ (r & 15)) << 2)) = v;
  }
}

// row fragment: columns 32s + 8g .. +7 of tile row `row`
__device__ __forceinline__ f32x8 row_frag(const float* tile, int row, int s, int g) {
  const int ch = 8 * s + 2 * g, sw = row & 15;
  return cat(*reinterpret_cast<const f32x4*>(tile + row * HD + ((ch ^ sw) << 2)),
             *reinterpret_cast<const f32x4*>(tile + row * HD + (((ch + 1) ^ sw) << 2)));
}

// column fragment over the tile pair (t0 = 2 tp, t1 = 2 tp + 1): column `col` of rows 32 tp + 4g + j (j < 4), 32 tp + 16 + 4g + j - 4
__device__ __forceinline__ f32x8 col_frag(const float* tile, int tp, int col, int g) {
  f32x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = tile[tix(32 * tp + 16 * (j >> 2) + 4 * g + (j & 3), col)];
  return r;
}

// D[r] = sum over the 64 columns of dO[r] * O[r], rows [0,nrows); rows beyond valid -> 0
__device__ __forceinline__ void rowdot_head(float* sD, const float* dO, const float* O, int64_t row0, int ld, int nrows, int valid) {
  for (int base = 0; base < nrows; base += 16 * WAVES) {
    const int r = base + (threadIdx.x >> 2), part = threadIdx.x & 3;
    float s = 0.f;
    if (r < valid) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(dO + (row0 + r) * ld + 16 * part + 4 * k);
        const f32x4 b = *reinterpret_cast<const f32x4*>(O + (row0 + r) * ld + 16 * part + 4 * k);
        s += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
      }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0 && r < nrows) sD[r] = s;
  }
}

__device__ __forceinline__ float key_add(const int64_t* mask, int64_t row0, int k, int L) {
  return k < L ? (1.0f - (float)mask[row0 + k]) * -1e9f : -INFINITY;
}

// -----------------------------------------------------------------------------------------------------------
// forward: workgroup = 128 queries of one (batch, head); wave = 16 queries x all keys.  LDS: [K | V | sAdd]
// -----------------------------------------------------------------------------------------------------------
template <int TERMS, int KT>
__global__ __launch_bounds__(64 * WAVES) void attn64_fwd_kernel(Attn64P p) {
  static_assert(KT % 2 == 0, "tiles are consumed in pairs");
  extern __shared__ __attribute__((aligned(16))) float smem64[];
  constexpr int Lp = KT * 16;
  float* sK = smem64;
  float* sV = sK + Lp * HD;
  float* sAdd = sV + Lp * HD;

  const int b = blockIdx.z, hd = blockIdx.y, q0 = blockIdx.x * ROWS_WG;
  const int L = p.L, H = p.H, ld3 = 3 * H;
  const int64_t row0 = (int64_t)b * L;
  const float amax = b4r_seq_amax(p.mask + row0, L);   // all threads, before any early exit
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 15, g = lane >> 4;
  const int q = q0 + 16 * wave + i;

  const float* qrow = p.qkv + (row0 + min(q, L - 1)) * ld3 + hd * HD + 8 * g;
  const Op8 qf0 = op8<TERMS>(load8(qrow)), qf1 = op8<TERMS>(load8(qrow + 32));
  stage_rows(sK, p.qkv + H + hd * HD, row0, ld3, Lp, L);
  stage_rows(sV, p.qkv + 2 * H + hd * HD, row0, ld3, Lp, L);
  for (int k = threadIdx.x; k < Lp; k += 64 * WAVES) sAdd[k] = key_add(p.mask, row0, k, L);
  __syncthreads();
  if (q0 + 16 * wave >= L) return;  // wave-uniform; no barrier below

  f32x4 acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {   // S^T = K.Q^T: lane holds keys 16t + 4g + r of query i
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = mma8<TERMS>(op8<TERMS>(row_frag(sK, 16 * t + i, 0, g)), qf0, c);
    c = mma8<TERMS>(op8<TERMS>(row_frag(sK, 16 * t + i, 1, g)), qf1, c);
    acc[t] = c;
  }
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const f32x4 ad = *reinterpret_cast<const f32x4*>(&sAdd[16 * t + 4 * g]);
#pragma unroll
    for (int r = 0; r < 4; ++r) { acc[t][r] += ad[r]; m = fmaxf(m, acc[t][r]); }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { const float e = __expf(acc[t][r] - m); acc[t][r] = e; sum += e; }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  const int64_t bh = (int64_t)b * p.heads + hd;
  if (g == 0 && q < L && p.lse_out) p.lse_out[bh * L + q] = (m - amax) + __logf(sum);

  const DropCtx dctx = b4r_drop_ctx(p.drop);
  const uint64_t dbase = ((uint64_t)bh * L + (uint64_t)(q < L ? q : 0)) * (uint64_t)B4R_ATTN_PITCH;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    if (dctx.on) {
      const B4rKeep4 k4 = b4r_keep4p(dctx, dbase + (uint64_t)(16 * t + 4 * g));
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] = k4.k[r] ? acc[t][r] * inv * dctx.scale : 0.f;
    } else {
      acc[t] = acc[t] * inv;
    }
  }

  f32x4 o[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tp = 0; tp < KT / 2; ++tp) {   // O^T[dd][query] += V^T[dd][keys of two tiles] . P^T[keys][query]
    const Op8 pb = op8<TERMS>(cat(acc[2 * tp], acc[2 * tp + 1]));
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = mma8<TERMS>(op8<TERMS>(col_frag(sV, tp, 16 * c + i, g)), pb, o[c]);
  }
  if (q < L) {
    float* dst = p.ctx_out + (row0 + q) * H + hd * HD + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(dst + 16 * c) = o[c];
  }
}

// -----------------------------------------------------------------------------------------------------------
// backward: blocks [0, nx) form dQ of 128 queries (LDS [K | V | sAdd]); blocks [nx, 2 nx) form dK / dV of 128 keys
// (LDS [Q | dO | sLse | sD]).  Probabilities recomputed from the saved log-sum-exp.
// -----------------------------------------------------------------------------------------------------------
template <int TERMS>
__device__ __forceinline__ void bwd_dq(const Attn64P p, float* smem, int b, int hd, int q0, float amax) {
  const int KT = p.KT, Lp = KT * 16;
  float* sK = smem;
  float* sV = sK + Lp * HD;
  float* sAdd = sV + Lp * HD;
  const int L = p.L, H = p.H, ld3 = 3 * H;
  const int64_t row0 = (int64_t)b * L;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 15, g = lane >> 4;
  const int q = q0 + 16 * wave + i, qc = min(q, L - 1);
  const bool qlive = q < L;

  const float* qrow = p.qkv + (row0 + qc) * ld3 + hd * HD + 8 * g;
  const float* drow = p.dctx + (row0 + qc) * H + hd * HD + 8 * g;
  const float* orow = p.ctx + (row0 + qc) * H + hd * HD + 8 * g;
  const f32x8 do0 = load8(drow), do1 = load8(drow + 32);
  float Dq;
  {
    const f32x8 o0 = load8(orow), o1 = load8(orow + 32);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += do0[j] * o0[j] + do1[j] * o1[j];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    Dq = s;
  }
  const Op8 qf0 = op8<TERMS>(load8(qrow)), qf1 = op8<TERMS>(load8(qrow + 32));
  const Op8 df0 = op8<TERMS>(do0), df1 = op8<TERMS>(do1);
  stage_rows(sK, p.qkv + H + hd * HD, row0, ld3, Lp, L);
  stage_rows(sV, p.qkv + 2 * H + hd * HD, row0, ld3, Lp, L);
  for (int k = threadIdx.x; k < Lp; k += 64 * WAVES) sAdd[k] = key_add(p.mask, row0, k, L);
  __syncthreads();
  if (q0 + 16 * wave >= L) return;   // wave-uniform; no barrier below

  const int64_t bh = (int64_t)b * p.heads + hd;
  const float lse = p.lse_in[bh * L + qc];
  const DropCtx dctx = b4r_drop_ctx(p.drop);
  const uint64_t dbase = ((uint64_t)bh * L + (uint64_t)(qlive ? q : 0)) * (uint64_t)B4R_ATTN_PITCH;

  f32x4 dq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) dq[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int tp = 0; tp < KT / 2; ++tp) {
    f32x4 ds[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = 2 * tp + u;
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
      sc = mma8<TERMS>(op8<TERMS>(row_frag(sK, 16 * t + i, 0, g)), qf0, sc);
      sc = mma8<TERMS>(op8<TERMS>(row_frag(sK, 16 * t + i, 1, g)), qf1, sc);
      da = mma8<TERMS>(op8<TERMS>(row_frag(sV, 16 * t + i, 0, g)), df0, da);
      da = mma8<TERMS>(op8<TERMS>(row_frag(sV, 16 * t + i, 1, g)), df1, da);
      const f32x4 ad = *reinterpret_cast<const f32x4*>(&sAdd[16 * t + 4 * g]);
      B4rKeep4 k4 = {{true, true, true, true}};
      if (dctx.on) k4 = b4r_keep4p(dctx, dbase + (uint64_t)(16 * t + 4 * g));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __expf(((sc[r] + ad[r]) - amax) - lse);
        float dA = da[r];
        if (dctx.on) dA = k4.k[r] ? dA * dctx.scale : 0.f;
        ds[u][r] = pr * (dA - Dq);
      }
    }
    const Op8 db = op8<TERMS>(cat(ds[0], ds[1]));   // dQ^T[dd][query] += K^T[dd][keys] . dS^T[keys][query]
#pragma unroll
    for (int c = 0; c < 4; ++c) dq[c] = mma8<TERMS>(op8<TERMS>(col_frag(sK, tp, 16 * c + i, g)), db, dq[c]);
  }
  if (qlive) {
    float* dst = p.dqkv + (row0 + q) * ld3 + hd * HD + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(dst + 16 * c) = dq[c] * p.qscale;
  }
}

template <int TERMS>
__device__ __forceinline__ void bwd_dkv(const Attn64P p, float* smem, int b, int hd, int kb, float amax) {
  const int KT = p.KT, Lp = KT * 16;
  float* sQ = smem;
  float* sdO = sQ + Lp * HD;
  float* sLse = sdO + Lp * HD;
  float* sD = sLse + Lp;
  const int L = p.L, H = p.H, ld3 = 3 * H;
  const int64_t row0 = (int64_t)b * L;
  const int64_t bh = (int64_t)b * p.heads + hd;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = lane & 15, g = lane >> 4;
  const int k0 = kb * ROWS_WG + 16 * wave, key = k0 + i, kc = min(key, L - 1);
  const bool klive = key < L;

  const float* krow = p.qkv + (row0 + kc) * ld3 + H + hd * HD + 8 * g;
  const Op8 kf0 = op8<TERMS>(load8(krow)), kf1 = op8<TERMS>(load8(krow + 32));
  const Op8 vf0 = op8<TERMS>(load8(krow + H)), vf1 = op8<TERMS>(load8(krow + H + 32));
  stage_rows(sQ, p.qkv + hd * HD, row0, ld3, Lp, L);
  stage_rows(sdO, p.dctx + hd * HD, row0, H, Lp, L);
  rowdot_head(sD, p.dctx + hd * HD, p.ctx + hd * HD, row0, H, Lp, L);
  for (int k = threadIdx.x; k < Lp; k += 64 * WAVES)
    sLse[k] = (k < L) ? p.lse_in[bh * L + k] : INFINITY;   // +inf => probability 0 for pad queries
  __syncthreads();
  if (k0 >= L) return;   // wave-uniform; no barrier below

  const float add = key_add(p.mask, row0, key, L);
  const DropCtx dctx = b4r_drop_ctx(p.drop);
  const uint64_t hbase = (uint64_t)bh * (uint64_t)L;

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { dk[c] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[c] = dk[c]; }
  for (int tp = 0; tp < KT / 2; ++tp) {
    f32x4 pa[2], ds[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {   // S = Q.K^T: lane holds queries 16t + 4g + r of key i
      const int t = 2 * tp + u;
      f32x4 sc = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
      sc = mma8<TERMS>(op8<TERMS>(row_frag(sQ, 16 * t + i, 0, g)), kf0, sc);
      sc = mma8<TERMS>(op8<TERMS>(row_frag(sQ, 16 * t + i, 1, g)), kf1, sc);
      da = mma8<TERMS>(op8<TERMS>(row_frag(sdO, 16 * t + i, 0, g)), vf0, da);
      da = mma8<TERMS>(op8<TERMS>(row_frag(sdO, 16 * t + i, 1, g)), vf1, da);
      const f32x4 ls = *reinterpret_cast<const f32x4*>(&sLse[16 * t + 4 * g]);
      const f32x4 dd = *reinterpret_cast<const f32x4*>(&sD[16 * t + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qq = 16 * t + 4 * g + r;
        const float pr = __expf(((sc[r] + add) - amax) - ls[r]);
        float ad = pr, dA = da[r];
        if (dctx.on) {
          const bool keep = b4r_keep(dctx, (hbase + (uint64_t)(qq < L ? qq : 0)) * (uint64_t)B4R_ATTN_PITCH + (uint64_t)(klive ? key : 0));
          ad = keep ? pr * dctx.scale : 0.f;
          dA = keep ? dA * dctx.scale : 0.f;
        }
        pa[u][r] = ad;
        ds[u][r] = pr * (dA - dd[r]);
      }
    }
    const Op8 pb = op8<TERMS>(cat(pa[0], pa[1])), db = op8<TERMS>(cat(ds[0], ds[1]));
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // dV^T[dd][key] += dO^T[dd][queries] . A[queries][key] ; dK^T += Q^T . dS
      dv[c] = mma8<TERMS>(op8<TERMS>(col_frag(sdO, tp, 16 * c + i, g)), pb, dv[c]);
      dk[c] = mma8<TERMS>(op8<TERMS>(col_frag(sQ, tp, 16 * c + i, g)), db, dk[c]);
    }
  }
  if (klive) {
    float* ok = p.dqkv + (row0 + key) * ld3 + H + hd * HD + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      *reinterpret_cast<f32x4*>(ok + 16 * c) = dk[c];
      *reinterpret_cast<f32x4*>(ok + H + 16 * c) = dv[c];
    }
  }
}

template <int TERMS>
__global__ __launch_bounds__(64 * WAVES) void attn64_bwd_kernel(Attn64P p) {
  extern __shared__ __attribute__((aligned(16))) float smem64[];
  const int b = blockIdx.z, hd = blockIdx.y;
  const float amax = b4r_seq_amax(p.mask + (int64_t)b * p.L, p.L);   // all threads, before any early exit
  if ((int)blockIdx.x < p.nx) bwd_dq<TERMS>(p, smem64, b, hd, blockIdx.x * ROWS_WG, amax);
  else bwd_dkv<TERMS>(p, smem64, b, hd, blockIdx.x - p.nx, amax);
}

// 16-row tiles of the forward's key sweep (even; compile-time: the score tiles live in registers)
int fwd_tiles(int L) {
  if (L <= 32) return 2;
  if (L <= 64) return 4;
  if (L <= 128) return 8;
  if (L <= 224) return 14;
  if (L <= 256) return 16;
  return 0;
}
inline int even_tiles(int L) { return ((L + 31) / 32) * 2; }

template <typename K>
int set_lds(K kernel, size_t bytes) { return b4r_raise_lds((const void*)kernel, bytes, "attention (head width 64)"); }

int check64(const char* who, const float* qkv, const int64_t* mask, int B, int L, int heads) {
  B4R_CHECK_ARG(qkv && mask, B4R_E_BADARG, "%s: null argument", who);
  B4R_CHECK_ARG(B > 0 && L > 0 && heads > 0, B4R_E_SHAPE, "%s: bad shape", who);
  B4R_CHECK_ARG(L <= 256, B4R_E_SHAPE, "%s: sequence length %d > 256 is not supported", who, L);
  B4R_CHECK_ARG(b4r_aligned16(qkv), B4R_E_ALIGN, "%s: qkv must be 16-byte aligned", who);
  return B4R_OK;
}

template <int TERMS>
int fwd_launch(const Attn64P& p, hipStream_t stream) {
  const int KT = fwd_tiles(p.L);
  const size_t sh = ((size_t)2 * KT * 16 * HD + KT * 16) * sizeof(float);
  const dim3 grid(b4r_cdiv(p.L, ROWS_WG), p.heads, p.B);
  int rc = B4R_OK;
#define FWD_CASE(KT_)                                                                                    \
  case KT_:                                                                                              \
    rc = set_lds(attn64_fwd_kernel<TERMS, KT_>, sh);                                                        \
    if (rc) return rc;                                                                                   \
    hipLaunchKernelGGL((attn64_fwd_kernel<TERMS, KT_>), grid, dim3(64 * WAVES), sh, stream, p);             \
    break;
  switch (KT) {
    FWD_CASE(2) FWD_CASE(4) FWD_CASE(8) FWD_CASE(14) FWD_CASE(16)
    default: b4r_set_error("b4r_attn_fwd_hd: internal"); return B4R_E_SHAPE;
  }
#undef FWD_CASE
  return B4R_OK;
}

template <int TERMS>
int bwd_launch(const Attn64P& p, hipStream_t stream) {
  const size_t sh = ((size_t)2 * p.KT * 16 * HD + 2 * p.KT * 16) * sizeof(float);
  const int rc = set_lds(attn64_bwd_kernel<TERMS>, sh);
  if (rc) return rc;
  hipLaunchKernelGGL(attn64_bwd_kernel<TERMS>, dim3(2 * p.nx, p.heads, p.B), dim3(64 * WAVES), sh, stream, p);
  return B4R_OK;
}

}  // namespace

extern "C" int b4r_attn_fwd_hd(const float* qkv, const int64_t* input_mask, int32_t B, int32_t L, int32_t heads, int32_t head_dim,
                               float* ctx, float* lse, const uint32_t* rng, uint32_t drop_stream, float drop_rate,
                               uint32_t* keep_bits, b4r_stream_t stream) {
  if (head_dim == 32)
    return b4r_attn_fwd(qkv, input_mask, B, L, heads, ctx, lse, rng, drop_stream, drop_rate, keep_bits, stream);
  B4R_CHECK_ARG(head_dim == 64, B4R_E_SHAPE, "b4r_attn_fwd_hd: head_dim %d not supported (32, 64)", head_dim);
  int rc = check64("b4r_attn_fwd_hd", qkv, input_mask, B, L, heads);
  if (rc) return rc;
  B4R_CHECK_ARG(ctx != nullptr, B4R_E_BADARG, "b4r_attn_fwd_hd: null ctx");
  B4R_CHECK_ARG(b4r_aligned16(ctx), B4R_E_ALIGN, "b4r_attn_fwd_hd: ctx must be 16-byte aligned");
  Attn64P p{};
  p.qkv = qkv; p.mask = input_mask; p.ctx_out = ctx; p.lse_out = lse;
  p.B = B; p.L = L; p.heads = heads; p.H = heads * HD;
  p.drop = b4r_make_drop(rng, drop_stream, drop_rate, 1);
  const int terms = b4r_gemm_terms();
  rc = terms == 3 ? fwd_launch<3>(p, (hipStream_t)stream) : terms == 1 ? fwd_launch<1>(p, (hipStream_t)stream)
                                                                      : fwd_launch<0>(p, (hipStream_t)stream);
  if (rc) return rc;
  B4R_CHECK_LAUNCH(terms == 1 ? "b4r_attn_fwd_hd (bf16)" : "b4r_attn_fwd_hd");
  return B4R_OK;
}

extern "C" int b4r_attn_bwd_hd(const float* qkv, const int64_t* input_mask, const float* ctx, const float* lse, const float* dctx,
                               int32_t B, int32_t L, int32_t heads, int32_t head_dim, float qscale, float* dqkv, const uint32_t* rng,
                               uint32_t drop_stream, float drop_rate, const uint32_t* keep_bits, b4r_stream_t stream) {
  if (head_dim == 32)
    return b4r_attn_bwd(qkv, input_mask, ctx, lse, dctx, B, L, heads, qscale, dqkv, rng, drop_stream, drop_rate, keep_bits, stream);
  B4R_CHECK_ARG(head_dim == 64, B4R_E_SHAPE, "b4r_attn_bwd_hd: head_dim %d not supported (32, 64)", head_dim);
  int rc = check64("b4r_attn_bwd_hd", qkv, input_mask, B, L, heads);
  if (rc) return rc;
  B4R_CHECK_ARG(ctx && lse && dctx && dqkv, B4R_E_BADARG, "b4r_attn_bwd_hd: null argument");
  B4R_CHECK_ARG(b4r_aligned16(ctx) && b4r_aligned16(dctx) && b4r_aligned16(dqkv), B4R_E_ALIGN,
                "b4r_attn_bwd_hd: operands must be 16-byte aligned");
  Attn64P p{};
  p.qkv = qkv; p.mask = input_mask; p.ctx = ctx; p.lse_in = lse; p.dctx = dctx; p.dqkv = dqkv;
  p.B = B; p.L = L; p.heads = heads; p.H = heads * HD; p.qscale = qscale;
  p.KT = even_tiles(L); p.nx = b4r_cdiv(L, ROWS_WG);
  p.drop = b4r_make_drop(rng, drop_stream, drop_rate, 1);
  const int terms = b4r_gemm_terms();
  rc = terms == 3 ? bwd_launch<3>(p, (hipStream_t)stream) : terms == 1 ? bwd_launch<1>(p, (hipStream_t)stream)
                                                                      : bwd_launch<0>(p, (hipStream_t)stream);
  if (rc) return rc;
  B4R_CHECK_LAUNCH(terms == 1 ? "b4r_attn_bwd_hd (bf16)" : "b4r_attn_bwd_hd");
  return B4R_OK;
}
