// Factorised item embeddings (embedding_width E < hidden_size H): the embedding stage at width E followed by the learned E -> H
// projection, forward and backward, one launch each.
//
// Follows  Bert4RecEncoder.call   bert4rec/models/components/networks/bert4rec_encoder.py:198-214
//          (word + position embedding at width E, LayerNorm, dropout, then embedding_projection, an EinsumDense '...x,xy->...y'
//           with kernel [E, H] and bias [H]; the layer is built at :103-131)
//
//   forward   z = T[id] + Pos[l] (width E), e = dropout(LN_E(z)), x0 = e . Wp + bp          (x0 [N, H], mean0 / rstd0 [N])
//   backward  dWp = e^T . dx0, dbp = colsum(dx0), de = dx0 . Wp^T, then back through the dropout and LN_E (dgamma / dbeta) to
//             d(T[id] + Pos[l]) [N, E], the rows b4r_embed_grads scatters into the item table and sums into the position table.
//
// The [N, E] intermediate e never goes to HBM: the forward forms it in LDS per tile of rows, the backward recomputes it from the ids,
// the tables and the saved row statistics.  The three products run on the matrix cores in 16 x 16 output blocks, 32 k per step (the
// Op8 steps of b4r_attn64.hip), following the project's rule: bf16x3 (v_mfma_f32_16x16x32_bf16, hi.lo + lo.hi + hi.hi) where K <= 64
// -- the forward at E = 64 in the B4R_GEMM_BF16X3 mode --, exact fp32 (v_mfma_f32_16x16x4_f32) otherwise: the forward at E = 128 / 256
// and in the B4R_GEMM_F32 mode, the backward's de = dx0 . Wp^T (K = H) and dWp = e^T . dx0 (K = rows) always.  No atomics: the
// backward's column sums go through per-workgroup slabs and the caller's ordered reduce queue, bitwise reproducible.
#include "b4r_common.h"
#include "b4r_internal.h"

namespace {

constexpr int FR = 64;    // forward: rows per workgroup (4 waves x 16 rows)
constexpr int BR = 64;    // backward, row part: rows per workgroup
constexpr int WR = 32;    // backward, weight part: rows per sub-tile
constexpr int CT = 64;    // columns of H per pass / per weight-part workgroup

struct EmbProjP {
  const int64_t* ids; const float* table; const float* pos; const float* gamma; const float* beta;
  const float* Wp; const float* bp;
  int N, L, V, H;
  float eps;
  DropArgs drop;
  float* x0; float* mean; float* rstd;   // forward outputs
  // backward
  const float* dx0; const float* smean; const float* srstd;
  float* drows;        // [N, E]
  float* slab_w;       // [S][E][H]
  float* slab_b;       // [S][H]
  float* ln_part;      // [nA][2E]
  int nA, S, rows_per_s;
};

// one 32-k operand fragment of a 16 x 16 block: lane l holds k = 8 (l / 16) .. + 7 of its row (A) or column (B) of the block, as fp32
// values and (BF) their bf16 hi / lo split.  The accumulator: rows 4 (l / 16) + i, column l % 16.
struct Frag {
  f32x8 v;
  b4r_bf16x8 h, l;
};
template <bool BF>
__device__ __forceinline__ Frag frag(const f32x8 x) {
  Frag f;
  f.v = x;
  if constexpr (BF) b4r_split8(x, f.h, f.l);
  return f;
}
template <bool BF>
__device__ __forceinline__ f32x4 mma32(const Frag& a, const Frag& b, f32x4 c) {
  if constexpr (BF) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, c, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  }
  return c;
}
__device__ __forceinline__ f32x8 load8g(const float* ptr) {   // 8 consecutive floats, 32-byte aligned
  const f32x4 a = *reinterpret_cast<const f32x4*>(ptr), b = *reinterpret_cast<const f32x4*>(ptr + 4);
  return (f32x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// One row of the embedding stage at width E, in the lanes of one wave (lane holds columns lane + 64 j): z = T[id] + Pos[l];
// with `stats` given (mean / rstd saved by the forward) they are used instead of being formed.  Returns e = dropout(LN(z)) in v[]
// and leaves zhat (the normalised z) in zh[] and the keep scale in ks[] (0 or 1 / (1 - rate), 1 without dropout).
template <int E>
__device__ __forceinline__ void emb_row(const EmbProjP& p, const DropCtx& dc, int64_t row, bool have_stats, float& mean, float& rstd,
                                        float (&v)[E / 64], float (&zh)[E / 64], float (&ks)[E / 64]) {
  constexpr int J = E / 64;
  const int lane = threadIdx.x & 63;
  int64_t id = p.ids[row];
  if (id < 0 || id >= p.V) id = 0;   // out-of-range ids read the PAD row instead of faulting
  const int l = (int)(row % p.L);
  float z[J];
#pragma unroll
  for (int j = 0; j < J; ++j) z[j] = p.table[id * E + lane + 64 * j] + p.pos[(int64_t)l * E + lane + 64 * j];
  if (!have_stats) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) s += z[j];
    mean = b4r_wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) { const float d = z[j] - mean; q += d * d; }
    rstd = rsqrtf(b4r_wave_sum(q) / (float)E + p.eps);
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int c = lane + 64 * j;
    const float inv = rstd * p.gamma[c];
    zh[j] = (z[j] - mean) * rstd;
    const float y = z[j] * inv + (p.beta[c] - mean * inv);
    ks[j] = 1.f;
    if (dc.on) ks[j] = b4r_keep(dc, (uint64_t)row * E + c) ? dc.scale : 0.f;
    v[j] = dc.on ? y * ks[j] : y;
  }
}

// forward: grid = ceil(N / FR) workgroups of 256; LDS: e [FR][E + 1].  BF: the bf16x3 product (E = 64 in the bf16x3 mode)
template <int E, bool BF>
__global__ __launch_bounds__(256) void embed_proj_fwd_kernel(EmbProjP p) {
  extern __shared__ float es[];   // [FR][E + 1]
  constexpr int LD = E + 1, J = E / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * FR;
  const DropCtx dc = b4r_drop_ctx(p.drop);
  for (int rr = wave; rr < FR; rr += 4) {
    const int64_t row = r0 + rr;
    float v[J], zh[J], ks[J];
    if (row < p.N) {
      float mean = 0.f, rstd = 0.f;
      emb_row<E>(p, dc, row, false, mean, rstd, v, zh, ks);
      if (lane == 0) { p.mean[row] = mean; p.rstd[row] = rstd; }
    } else {
#pragma unroll
      for (int j = 0; j < J; ++j) v[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) es[rr * LD + lane + 64 * j] = v[j];
  }
  __syncthreads();
  // x0[r][c] = bp[c] + sum_k e[r][k] Wp[k][c].  Wave: rows wave * 16 .. + 15, four 16-column blocks per pass of 64 columns
  const int rb = wave * 16, li = lane & 15, g = lane >> 4;
  for (int c0 = 0; c0 < p.H; c0 += CT) {
    f32x4 acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < E; k0 += 32) {
      f32x8 av;
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = es[(rb + li) * LD + k0 + 8 * g + j];
      const Frag a = frag<BF>(av);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        f32x8 bv;
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = p.Wp[(int64_t)(k0 + 8 * g + j) * p.H + c0 + 16 * nb + li];
        acc[nb] = mma32<BF>(a, frag<BF>(bv), acc[nb]);
      }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int c = c0 + 16 * nb + li;
      const float b = p.bp[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = r0 + rb + 4 * g + i;
        if (row < p.N) p.x0[row * p.H + c] = acc[nb][i] + b;
      }
    }
  }
}

// backward, row part (workgroups [0, nA)): de = dx0 . Wp^T on BR rows (exact fp32 matrix cores, K = H), then the dropout and
// LayerNorm backward per row.  LDS: de [BR][E + 1]
template <int E>
__device__ __forceinline__ void bwd_rows(const EmbProjP& p, float* lds) {
  constexpr int J = E / 64, LDE = E + 1, NB = E / 16;
  float* ds = lds;                       // [BR][LDE]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * BR;
  // wave: rows wave * 16 .. + 15, all E columns (NB blocks).  A = dx0 rows (read once, straight from HBM), B[k = c][n = e] = Wp[e][c]:
  // both fragments are 8 consecutive floats of a row
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int64_t arow = r0 + wave * 16 + li;
  for (int k0 = 0; k0 < p.H; k0 += 32) {
    const f32x8 av = arow < p.N ? load8g(p.dx0 + arow * p.H + k0 + 8 * g) : (f32x8){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const Frag a = frag<false>(av);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = mma32<false>(a, frag<false>(load8g(p.Wp + (int64_t)(16 * nb + li) * p.H + k0 + 8 * g)), acc[nb]);
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) ds[(wave * 16 + 4 * g + i) * LDE + 16 * nb + li] = acc[nb][i];
  __syncthreads();
  // per row (one wave): g = de * keep scale; dgamma += g zhat, dbeta += g; dz = rstd (gg - mean(gg) - zhat mean(gg zhat)), gg = g gamma
  const DropCtx dc = b4r_drop_ctx(p.drop);
  float dgam[J], dbet[J];
#pragma unroll
  for (int j = 0; j < J; ++j) { dgam[j] = 0.f; dbet[j] = 0.f; }
  for (int rr = wave * 16; rr < wave * 16 + 16; ++rr) {
    const int64_t row = r0 + rr;
    if (row >= p.N) break;
    float mean = p.smean[row], rstd = p.srstd[row];
    float v[J], zh[J], ks[J];
    emb_row<E>(p, dc, row, true, mean, rstd, v, zh, ks);
    float gg[J], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = lane + 64 * j;
      const float g = ds[rr * LDE + c] * ks[j];
      dgam[j] = fmaf(g, zh[j], dgam[j]);
      dbet[j] += g;
      gg[j] = g * p.gamma[c];
      s1 += gg[j];
      s2 += gg[j] * zh[j];
    }
    const float m1 = b4r_wave_sum(s1) / (float)E, m2 = b4r_wave_sum(s2) / (float)E;
#pragma unroll
    for (int j = 0; j < J; ++j) p.drows[row * E + lane + 64 * j] = rstd * (gg[j] - m1 - zh[j] * m2);
  }
  // the workgroup's LayerNorm partials: the 4 waves' sums in wave order
  __syncthreads();
#pragma unroll
  for (int j = 0; j < J; ++j) { ds[wave * 2 * E + lane + 64 * j] = dgam[j]; ds[wave * 2 * E + E + lane + 64 * j] = dbet[j]; }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * E; c += 256) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += ds[w * 2 * E + c];
    p.ln_part[(int64_t)blockIdx.x * 2 * E + c] = s;
  }
}

// backward, weight part (workgroups nA + (s * H / CT + ct)): dWp[:, c0 .. c0 + CT) and dbp over the rows of chunk s; e recomputed
// (chunks are whole multiples of WR = 32 rows: one 32-k step per sub-tile).
// LDS: e [WR][E + 1], dx0 [WR][CT + 1]
template <int E>
__device__ __forceinline__ void bwd_weights(const EmbProjP& p, float* lds, int blk) {
  constexpr int J = E / 64, LDE = E + 1, LDX = CT + 1, MB = E / 16;
  float* es = lds;                  // [WR][LDE]
  float* xs = es + WR * LDE;        // [WR][LDX]
  const int nct = p.H / CT;
  const int s = blk / nct, ct = blk % nct, c0 = ct * CT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rb = (int64_t)s * p.rows_per_s;
  const int64_t re = rb + p.rows_per_s < p.N ? rb + p.rows_per_s : p.N;
  const DropCtx dc = b4r_drop_ctx(p.drop);
  // dWp[e][c0 + c] = sum_r e[r][e] dx0[r][c0 + c] (exact fp32 matrix cores, K = the chunk's rows, 32 per sub-tile).  Wave: columns
  // c0 + 16 wave .. + 15, all E rows of dWp (MB blocks).  A[m = e][k = r] = es[r][e], B[k = r][n = c] = xs[r][c]
  const int li = lane & 15, g = lane >> 4;
  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int64_t t0 = rb; t0 < re; t0 += WR) {
    __syncthreads();
    for (int rr = wave; rr < WR; rr += 4) {
      const int64_t row = t0 + rr;
      float v[J], zh[J], ks[J];
      if (row < re) {
        float mean = p.smean[row], rstd = p.srstd[row];
        emb_row<E>(p, dc, row, true, mean, rstd, v, zh, ks);
      } else {
#pragma unroll
        for (int j = 0; j < J; ++j) v[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < J; ++j) es[rr * LDE + lane + 64 * j] = v[j];
      xs[rr * LDX + lane] = row < re ? p.dx0[row * p.H + c0 + lane] : 0.f;
    }
    __syncthreads();
    f32x8 bv;
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = xs[(8 * g + j) * LDX + 16 * wave + li];
    const Frag b = frag<false>(bv);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      f32x8 av;
#pragma unroll
      for (int j = 0; j < 8; ++j) av[j] = es[(8 * g + j) * LDE + 16 * mb + li];
      acc[mb] = mma32<false>(frag<false>(av), b, acc[mb]);
    }
    if (wave == 0)
      for (int r = 0; r < WR; ++r) bsum += xs[r * LDX + lane];   // d bp: rows in order, fp32
  }
  float* out = p.slab_w + (int64_t)s * E * p.H;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[(int64_t)(16 * mb + 4 * g + i) * p.H + c0 + 16 * wave + li] = acc[mb][i];
  if (wave == 0) p.slab_b[(int64_t)s * p.H + c0 + lane] = bsum;
}

template <int E>
__global__ __launch_bounds__(256) void embed_proj_bwd_kernel(EmbProjP p) {
  extern __shared__ float lds[];
  if ((int)blockIdx.x < p.nA) bwd_rows<E>(p, lds);
  else bwd_weights<E>(p, lds, (int)blockIdx.x - p.nA);
}

size_t fwd_lds(int E) { return (size_t)FR * (E + 1) * sizeof(float); }
size_t bwd_lds(int E) {
  const size_t rows = (size_t)BR * (E + 1);
  const size_t wts = (size_t)WR * (E + 1) + (size_t)WR * (CT + 1);
  return (rows > wts ? rows : wts) * sizeof(float);
}

// the weight part's row chunks: enough workgroups beside the row part to cover the chip, each chunk a whole number of sub-tiles
void bwd_split(int N, int H, int* S, int* rows_per_s) {
  const int nct = H / CT;
  int s = 512 / nct;
  if (s < 1) s = 1;
  const int max_s = b4r_cdiv(N, WR);
  if (s > max_s) s = max_s;
  int rps = b4r_cdiv(b4r_cdiv(N, s), WR) * WR;
  *S = b4r_cdiv(N, rps);
  *rows_per_s = rps;
}

bool shape_ok(int E, int H) { return (E == 64 || E == 128 || E == 256) && H % CT == 0 && H >= 64 && H <= 1024; }

}  // namespace

bool b4r_embed_proj_supported(int E, int H) { return shape_ok(E, H); }

int64_t b4r_embed_proj_bwd_scratch_floats_impl(int N, int E, int H) {
  int S = 0, rps = 0;
  bwd_split(N, H, &S, &rps);
  const int64_t nA = b4r_cdiv(N, BR);
  return ((int64_t)S * E * H + 3) / 4 * 4 + ((int64_t)S * H + 3) / 4 * 4 + nA * 2 * E;
}

int b4r_embed_proj_fwd_launch(const int64_t* ids, int B, int L, const float* table, int V, const float* pos, const float* gamma,
                              const float* beta, int E, float eps, const float* Wp, const float* bp, int H, float* x0, float* mean,
                              float* rstd, DropArgs drop, hipStream_t stream) {
  B4R_CHECK_ARG(shape_ok(E, H), B4R_E_SHAPE, "embed_proj_fwd: embedding width %d / hidden size %d not supported", E, H);
  EmbProjP p{};
  p.ids = ids; p.table = table; p.pos = pos; p.gamma = gamma; p.beta = beta; p.Wp = Wp; p.bp = bp;
  p.N = B * L; p.L = L; p.V = V; p.H = H; p.eps = eps; p.drop = drop; p.x0 = x0; p.mean = mean; p.rstd = rstd;
  const dim3 grid(b4r_cdiv(p.N, FR));
  const size_t lds = fwd_lds(E);
  // bf16x3 where K = E <= 64 in the bf16x3 mode, exact fp32 otherwise (include/b4r.h b4r_set_gemm_mode)
  const bool bf = E == 64 && b4r_split_mode();
  const void* k = bf ? reinterpret_cast<const void*>(embed_proj_fwd_kernel<64, true>)
                  : E == 64 ? reinterpret_cast<const void*>(embed_proj_fwd_kernel<64, false>)
                  : E == 128 ? reinterpret_cast<const void*>(embed_proj_fwd_kernel<128, false>)
                             : reinterpret_cast<const void*>(embed_proj_fwd_kernel<256, false>);
  const int rc = b4r_raise_lds(k, lds, "embed_proj_fwd");
  if (rc) return rc;
  if (bf) hipLaunchKernelGGL((embed_proj_fwd_kernel<64, true>), grid, dim3(256), lds, stream, p);
  else if (E == 64) hipLaunchKernelGGL((embed_proj_fwd_kernel<64, false>), grid, dim3(256), lds, stream, p);
  else if (E == 128) hipLaunchKernelGGL((embed_proj_fwd_kernel<128, false>), grid, dim3(256), lds, stream, p);
  else hipLaunchKernelGGL((embed_proj_fwd_kernel<256, false>), grid, dim3(256), lds, stream, p);
  B4R_CHECK_LAUNCH("embed_proj_fwd");
  return B4R_OK;
}

// dln: [2E] -- dgamma then dbeta.  The three column reductions (dWp + dbp, dgamma + dbeta) join the caller's reduce queue when one
// is active, else they are launched here
int b4r_embed_proj_bwd_launch(const float* dx0, const int64_t* ids, int B, int L, const float* table, int V, const float* pos,
                              const float* gamma, const float* beta, int E, const float* mean, const float* rstd, const float* Wp, int H,
                              DropArgs drop, float* drows, float* dWp, float* dbp, float* dln, float* scratch, hipStream_t stream) {
  B4R_CHECK_ARG(shape_ok(E, H), B4R_E_SHAPE, "embed_proj_bwd: embedding width %d / hidden size %d not supported", E, H);
  EmbProjP p{};
  p.ids = ids; p.table = table; p.pos = pos; p.gamma = gamma; p.beta = beta; p.Wp = Wp;
  p.N = B * L; p.L = L; p.V = V; p.H = H; p.drop = drop;
  p.dx0 = dx0; p.smean = mean; p.srstd = rstd; p.drows = drows;
  bwd_split(p.N, H, &p.S, &p.rows_per_s);
  p.nA = b4r_cdiv(p.N, BR);
  p.slab_w = scratch;
  p.slab_b = p.slab_w + ((int64_t)p.S * E * H + 3) / 4 * 4;
  p.ln_part = p.slab_b + ((int64_t)p.S * H + 3) / 4 * 4;
  const dim3 grid(p.nA + p.S * (H / CT));
  const size_t lds = bwd_lds(E);
  int rc = B4R_OK;
  switch (E) {
    case 64:
      rc = b4r_raise_lds(reinterpret_cast<const void*>(embed_proj_bwd_kernel<64>), lds, "embed_proj_bwd");
      if (rc) return rc;
      hipLaunchKernelGGL(embed_proj_bwd_kernel<64>, grid, dim3(256), lds, stream, p);
      break;
    case 128:
      rc = b4r_raise_lds(reinterpret_cast<const void*>(embed_proj_bwd_kernel<128>), lds, "embed_proj_bwd");
      if (rc) return rc;
      hipLaunchKernelGGL(embed_proj_bwd_kernel<128>, grid, dim3(256), lds, stream, p);
      break;
    default:
      rc = b4r_raise_lds(reinterpret_cast<const void*>(embed_proj_bwd_kernel<256>), lds, "embed_proj_bwd");
      if (rc) return rc;
      hipLaunchKernelGGL(embed_proj_bwd_kernel<256>, grid, dim3(256), lds, stream, p);
      break;
  }
  B4R_CHECK_LAUNCH("embed_proj_bwd");
  rc = b4r_launch_slab_reduce_full(p.slab_w, p.S, E, H, dWp, H, 0, p.slab_b, dbp, nullptr, nullptr, stream);
  if (rc) return rc;
  return b4r_launch_slab_reduce_full(p.ln_part, p.nA, 1, 2 * E, dln, 2 * E, 0, nullptr, nullptr, nullptr, nullptr, stream);
}

// ===============================================================================================================
// C ABI (op level)
extern "C" int b4r_embed_proj_fwd(const int64_t* ids, int32_t B, int32_t L, const float* table, int32_t V, const float* pos_table,
                                  const float* gamma, const float* beta, int32_t E, float eps, const float* Wp, const float* bp,
                                  int32_t H, float* x0, float* mean, float* rstd, const uint32_t* rng, float dropout,
                                  b4r_stream_t stream) {
  B4R_CHECK_ARG(ids && table && pos_table && gamma && beta && Wp && bp && x0 && mean && rstd, B4R_E_BADARG,
                "b4r_embed_proj_fwd: null argument");
  B4R_CHECK_ARG(B > 0 && L > 0 && V > 0, B4R_E_SHAPE, "b4r_embed_proj_fwd: bad shape");
  return b4r_embed_proj_fwd_launch(ids, B, L, table, V, pos_table, gamma, beta, E, eps, Wp, bp, H, x0, mean, rstd,
                                   b4r_make_drop(rng, B4R_STREAM_EMB, dropout, 1), (hipStream_t)stream);
}

extern "C" int64_t b4r_embed_proj_bwd_scratch_floats(int32_t N, int32_t E, int32_t H) {
  if (N <= 0 || !shape_ok(E, H)) return -1;
  return b4r_embed_proj_bwd_scratch_floats_impl(N, E, H);
}

extern "C" int b4r_embed_proj_bwd(const float* dx0, const int64_t* ids, int32_t B, int32_t L, const float* table, int32_t V,
                                  const float* pos_table, const float* gamma, const float* beta, int32_t E, const float* mean,
                                  const float* rstd, const float* Wp, int32_t H, const uint32_t* rng, float dropout, float* drows,
                                  float* dWp, float* dbp, float* dln, float* scratch, b4r_stream_t stream) {
  B4R_CHECK_ARG(dx0 && ids && table && pos_table && gamma && beta && mean && rstd && Wp && drows && dWp && dbp && dln && scratch,
                B4R_E_BADARG, "b4r_embed_proj_bwd: null argument");
  B4R_CHECK_ARG(B > 0 && L > 0 && V > 0, B4R_E_SHAPE, "b4r_embed_proj_bwd: bad shape");
  return b4r_embed_proj_bwd_launch(dx0, ids, B, L, table, V, pos_table, gamma, beta, E, mean, rstd, Wp, H,
                                   b4r_make_drop(rng, B4R_STREAM_EMB, dropout, 1), drows, dWp, dbp, dln, scratch, (hipStream_t)stream);
}
