// Low-rank adapters in weight space (include/sdt.h "LoRA"): the merge W = bf16(W0 + s * A * B) in front of a step and the projection
// of the bf16 weight gradient dW back onto the factors, dA = s * dW * B^T and dB = s * A^T * dW, behind its backward.  Both are
// grouped launches over one device job table with running tile counts (like sdt_param_prepare's descriptors), both round A and B to
// bf16 as they load them (the projection differentiates the function the merge evaluated), both accumulate in fp32 on
// mfma_f32_16x16x32_bf16 and neither uses an atomic: every output element has one writer and one fixed summation order.
// The split projection (include/sdt.h "LoCon") serves the tall K of convolution kernels: its dB stripes are cut along K, and the only
// atomic is the integer arrival counter behind which the last workgroup of a stripe adds the fp32 partials in chunk order.
// LoHa (include/sdt.h "LoHa"): the delta s * (A1 B1) o (A2 B2), element-wise - a fused merge and a fused projection that form the rank-r
// products beside each tile and never write them; its dB stripes always take the split.
//
// The kernels are assembled from five shared pieces, each written once:
//   for_rank_blocks  the rank r -> RB = ceil(r / 16) template argument of every projection (a workgroup-uniform branch)
//   merge_tile / merge_runs  the head (job, tile origin) and the tail (512 runs of 8 columns, W0 + s * tile or W0 alone) of a merge tile
//   db_walk          the walk of a dB stripe down rows [kb, ke) of dW: 32 x 64 blocks staged through a double-buffered LDS array; the
//                    variant's MFMAs are a body called per block, DoRA's sum G * W0 a hook on the vector a thread stages
//   db_store / db_finish  the end of a dB stripe for one (LoRA, LoCon) or two (LoHa) accumulator sets: dB = s * acc, or the split
//                    protocol - partial slab, arrival ticket, the last arriver's sum in chunk order
//   split_count / entry_args (host)  the chunk, stripe, counter and partial arithmetic of a job table; the argument preamble
//
// Operand lane maps of mfma_f32_16x16x32_bf16 (lane l): A[row l&15][k = 8(l>>4) + j], B[k = 8(l>>4) + j][col l&15], j = 0..7;
// C/D col = l&15, row = 4(l>>4) + reg.
#include <type_traits>

#include "sdt_common.h"

namespace {

constexpr int LT = 64;           // merge: output tile; project: rows of a dA stripe / columns of a dB stripe
constexpr int SPLIT_ROWS = 512;  // rows of dW in one chunk of a split dB stripe

// f(std::integral_constant<int, RB>) for the RB = ceil(r / 16) blocks of 16 adapter columns: RB in {1, 2, 4, 8}, up to MAXRB
// (r is a job's rank: the branch is workgroup-uniform.  check_jobs admits the ranks 4, 8, 16, 32, 64, 128 - check_loha_jobs up to 32 -
// so ceil(r / 16) is 1, 2, 4 or 8 and the last branch of each chain takes no other value)
template <int MAXRB, class F>
__device__ __forceinline__ void for_rank_blocks(int r, F f) {
  const int rb = (r + 15) / 16;
  if (rb == 1) {
    f(std::integral_constant<int, 1>{});
  } else if (MAXRB == 2 || rb == 2) {
    f(std::integral_constant<int, 2>{});
  } else if constexpr (MAXRB > 2) {
    if (rb == 4) f(std::integral_constant<int, 4>{}); else f(std::integral_constant<int, 8>{});
  }
}

// index of the last of n jobs whose first tile - first(i), a running count - is <= tile
template <class First>
__device__ __forceinline__ int find_index(int n, int tile, First first) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int find_job_index(const SdtLoraJob* jobs, int n, int tile, bool project) {
  return find_index(n, tile, [=](int i) { return project ? jobs[i].tile0_project : jobs[i].tile0_merge; });
}

// 8 consecutive float32 at p (16-byte aligned) rounded to a bf16 fragment; ok = false gives zero lanes
__device__ __forceinline__ bf16x8_t frag_from_f32(const float* p, bool ok) {
  uint4 v = {0u, 0u, 0u, 0u};
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v.x = pack2bf(a.x, a.y); v.y = pack2bf(a.z, a.w); v.z = pack2bf(b.x, b.y); v.w = pack2bf(b.z, b.w);
  }
  return __builtin_bit_cast(bf16x8_t, v);
}
// the same for r = 4: only the first four exist
__device__ __forceinline__ bf16x8_t frag_from_f32x4(const float* p, bool ok) {
  uint4 v = {0u, 0u, 0u, 0u};
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v.x = pack2bf(a.x, a.y); v.y = pack2bf(a.z, a.w);
  }
  return __builtin_bit_cast(bf16x8_t, v);
}
// elements p[0], p[stride], ... p[7 * stride] (float32) for k0 + j < kmax
__device__ __forceinline__ bf16x8_t frag_from_f32_strided(const float* p, long stride, int k0, int kmax, bool ok) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (ok && k0 + j < kmax) ? p[j * stride] : 0.f;
  const uint4 v = pack8(f);
  return __builtin_bit_cast(bf16x8_t, v);
}

// ---- merge: one 64 x 64 tile of one leaf per workgroup; wave w owns rows 16w .. 16w+15 and the four 16-column blocks ---------
// bf16(A) * bf16(B) of the tile at (r0, c0), unscaled fp32 accumulators, into `tile` (the caller synchronises before reading it)
__device__ __forceinline__ void ab_tile(const SdtLoraJob& d, const float* __restrict__ A, const float* __restrict__ B, int r0, int c0,
                                        float (*tile)[LT + 4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r;
  f32x4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int arow = r0 + 16 * wave + l15;
  for (int k0 = 0; k0 < r; k0 += 32) {  // the rank padded to the instruction's K with zero lanes
    const int k = k0 + 8 * lq;
    const bf16x8_t a = (r == 4) ? frag_from_f32x4(A + (long)arow * r, arow < d.K && k == 0)
                                : frag_from_f32(A + (long)arow * r + k, arow < d.K && k < r);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c0 + 16 * c + l15;
      const bf16x8_t b = frag_from_f32_strided(B + (long)k * d.N + col, d.N, k, r, col < d.N && k < r);
      acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[16 * wave + 4 * lq + i][16 * c + l15] = acc[c][i];
}

// the head of a merge tile: the job of workgroup blockIdx.x and the origin (r0, c0) of its tile in the leaf
struct MergeTile {
  int job, r0, c0;
};
__device__ __forceinline__ MergeTile merge_tile(const SdtLoraJob* __restrict__ jobs, int njobs) {
  const int job = find_job_index(jobs, njobs, blockIdx.x, false);
  const int tl = blockIdx.x - jobs[job].tile0_merge, tc = (jobs[job].N + LT - 1) / LT;
  return {job, (tl / tc) * LT, (tl % tc) * LT};
}

// v[0..7] = W0 + s * tile for run g (0..511) of the tile at (r0, c0): row g >> 3, 8 columns from 8 (g & 7); e = the run's element
// in the leaf.  False when the run lies outside the leaf (N is a multiple of 8: a run is whole or absent).  DELTA = false: W0 alone,
// `tile` is not read (not W0 + s * 0, which would turn -0.0f into +0.0f).
template <bool DELTA>
__device__ __forceinline__ bool merged_run(const SdtLoraJob& d, const float* __restrict__ w0_base, const float (*tile)[LT + 4], int g,
                                           int r0, int c0, float* v, long& e) {
  const int row = r0 + (g >> 3), col = c0 + (g & 7) * 8;
  if (row >= d.K || col >= d.N) return false;
  e = (long)row * d.N + col;
  const float* src = w0_base + d.w0_off + e;
  const float4 x0 = *reinterpret_cast<const float4*>(src), x1 = *reinterpret_cast<const float4*>(src + 4);
  const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (DELTA) v[j] = x[j] + d.scale * tile[g >> 3][(g & 7) * 8 + j]; else v[j] = x[j];
  }
  return true;
}

__device__ __forceinline__ void store_run(const SdtLoraJob& d, bf16_t* __restrict__ w_dst, float* __restrict__ f_dst, long e, const float* v) {
  if (w_dst) *reinterpret_cast<uint4*>(w_dst + d.w_off + e) = pack8(v);  // 16-byte bf16 store
  if (f_dst) {
    float* o = f_dst + d.f_off + e;
    *reinterpret_cast<float4*>(o) = float4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<float4*>(o + 4) = float4{v[4], v[5], v[6], v[7]};
  }
}

// the tail of a merge tile: its 512 runs of 8 columns, two per thread, into the bf16 mirror and / or the fp32 destination
template <bool DELTA>
__device__ __forceinline__ void merge_runs(const SdtLoraJob& d, const float* __restrict__ w0_base, const float (*tile)[LT + 4], int r0,
                                           int c0, bf16_t* __restrict__ w_dst, float* __restrict__ f_dst) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    float v[8];
    long e;
    if (merged_run<DELTA>(d, w0_base, tile, threadIdx.x + 256 * it, r0, c0, v, e)) store_run(d, w_dst, f_dst, e, v);
  }
}

__global__ void __launch_bounds__(256) lora_merge_kernel(const float* __restrict__ w0_base, const float* __restrict__ ab_base,
                                                         bf16_t* __restrict__ w_dst, float* __restrict__ f_dst,
                                                         const SdtLoraJob* __restrict__ jobs, int njobs) {
  __shared__ float tile[LT][LT + 4];
  const MergeTile t = merge_tile(jobs, njobs);
  const SdtLoraJob d = jobs[t.job];
  ab_tile(d, ab_base + d.a_off, ab_base + d.b_off, t.r0, t.c0, tile);
  __syncthreads();
  merge_runs<true>(d, w0_base, tile, t.r0, t.c0, w_dst, f_dst);
}

// ---- restore (include/sdt.h "DPO LOSS"): the merge's tiles and runs, W0 alone - w = bf16(W0), what sdt_param_prepare wrote there --------
__global__ void __launch_bounds__(256) lora_restore_kernel(const float* __restrict__ w0_base, bf16_t* __restrict__ w_dst,
                                                           const SdtLoraJob* __restrict__ jobs, int njobs) {
  const MergeTile t = merge_tile(jobs, njobs);
  merge_runs<false>(jobs[t.job], w0_base, nullptr, t.r0, t.c0, w_dst, nullptr);
}

// ---- DoRA merge (include/sdt.h "DoRA"): one 64-column stripe of one leaf per workgroup.  First walk over K: v tiles as above, every
// thread sums v^2 of its 8 columns over the rows it owns (row t >> 3 and 32 below it, of every 64-row block, top to bottom), the 32
// partials of a column are added in row order by one thread: one fixed order, no atomics.  c = sqrt(q) and g = m / c are formed in
// double and rounded once (53 >= 2 * 24 + 2 bits: the double rounding cannot change the result of either operation, so both are the
// correctly rounded fp32 values).  INIT: c is written into m and nothing else happens.  Second walk: the same v tiles, times g.
template <bool INIT>
__global__ void __launch_bounds__(256) dora_merge_kernel(const float* __restrict__ w0_base, const float* __restrict__ ab_base,
                                                         bf16_t* __restrict__ w_dst, float* __restrict__ f_dst, float* __restrict__ stat_base,
                                                         float* m_dst, const SdtLoraJob* __restrict__ jobs,
                                                         const SdtDoraJob* __restrict__ dj, int njobs) {
  __shared__ float tile[LT][LT + 4];
  __shared__ float red[32][LT];
  __shared__ float gcol[LT];
  const int job = find_index(njobs, blockIdx.x, [=](int i) { return dj[i].stripe0_merge; });
  const SdtLoraJob d = jobs[job];
  const SdtDoraJob x = dj[job];
  const int c0 = ((int)blockIdx.x - x.stripe0_merge) * LT;
  const float* A = ab_base + d.a_off;
  const float* B = ab_base + d.b_off;
  float qp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < d.K; r0 += LT) {
    ab_tile(d, A, B, r0, c0, tile);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      float v[8];
      long e;
      if (merged_run<true>(d, w0_base, tile, threadIdx.x + 256 * it, r0, c0, v, e)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) qp[j] += v[j] * v[j];
      }
    }
    __syncthreads();  // the tile has been consumed
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[threadIdx.x >> 3][(threadIdx.x & 7) * 8 + j] = qp[j];
  __syncthreads();
  if (threadIdx.x < LT) {
    const int n = c0 + threadIdx.x;
    float g = 0.f;
    if (n < d.N) {
      float q = 0.f;
      for (int i = 0; i < 32; ++i) q += red[i][threadIdx.x];
      const float c = (float)sqrt((double)q);
      if (INIT) {
        m_dst[x.m_off + n] = c;
      } else {
        g = c == 0.f ? 0.f : (float)((double)ab_base[x.m_off + n] / (double)c);
        stat_base[x.stat_off + n] = c;
        stat_base[x.stat_off + d.N + n] = g;
      }
    }
    gcol[threadIdx.x] = g;
  }
  if (INIT) return;
  __syncthreads();
  for (int r0 = 0; r0 < d.K; r0 += LT) {
    ab_tile(d, A, B, r0, c0, tile);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int g = threadIdx.x + 256 * it;
      float v[8];
      long e;
      if (merged_run<true>(d, w0_base, tile, g, r0, c0, v, e)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gcol[(g & 7) * 8 + j];
        store_run(d, w_dst, f_dst, e, v);
      }
    }
    __syncthreads();
  }
}

// 8 consecutive float32 at p rounded to bf16, times the 8 column factors at gp, rounded to bf16 again (DoRA: the B operand of dA)
__device__ __forceinline__ bf16x8_t frag_from_f32_scaled(const float* p, const float* gp, bool ok) {
  uint4 v = {0u, 0u, 0u, 0u};
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    const float4 ga = *reinterpret_cast<const float4*>(gp), gb = *reinterpret_cast<const float4*>(gp + 4);
    uint4 h;
    h.x = pack2bf(a.x, a.y); h.y = pack2bf(a.z, a.w); h.z = pack2bf(b.x, b.y); h.w = pack2bf(b.z, b.w);
    float f[8];
    unpack8(h, f);
    f[0] *= ga.x; f[1] *= ga.y; f[2] *= ga.z; f[3] *= ga.w; f[4] *= gb.x; f[5] *= gb.y; f[6] *= gb.z; f[7] *= gb.w;
    v = pack8(f);
  }
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ float bf_round(float x) { return __uint_as_float(pack2bf(x, 0.f) << 16); }

// what a DoRA projection has beyond the LoRA one: W0 of the leaf, its column statistics c and g, the destination of dm and the
// LDS the column reductions pass through
struct DoraCols {
  const float* W0;
  const float* c;
  const float* g;
  float* gm;
  float (*red)[LT];
};

// the end of a DoRA dB stripe: dB, the two column reductions and dm (acc = P of this lane: q = 16 b + 4 (lane >> 4) + i, one column)
template <int RB>
__device__ __forceinline__ void dora_db_tail(const SdtLoraJob& d, int c0, const float* __restrict__ B, float* __restrict__ gB,
                                             const f32x4_t* acc, const float* gw, const DoraCols& x) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r, N = d.N;
  const float s = d.scale;
  const int n = c0 + 16 * wave + l15;
  const float gn = n < N ? x.g[n] : 0.f;
  float t2 = 0.f;  // this lane's share of sum_q bf16(B[q][n]) * P[q][n], its q ascending (a column's four lanes are added below)
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 16 * b + 4 * lq + i;
      if (q < r && n < N) {
        t2 += bf_round(B[(long)q * N + n]) * acc[b][i];
        gB[(long)q * N + n] = (s * acc[b][i]) * gn;
      }
    }
  const int srow = threadIdx.x >> 3, scol = (threadIdx.x & 7) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) x.red[srow][scol + j] = gw[j];
  __syncthreads();
  float t1 = 0.f;
  if (threadIdx.x < LT)
    for (int i = 0; i < 32; ++i) t1 += x.red[i][threadIdx.x];
  __syncthreads();
  x.red[lq][16 * wave + l15] = t2;
  __syncthreads();
  if (threadIdx.x < LT && c0 + (int)threadIdx.x < N) {
    const int col = c0 + threadIdx.x;
    const float p = ((x.red[0][threadIdx.x] + x.red[1][threadIdx.x]) + x.red[2][threadIdx.x]) + x.red[3][threadIdx.x];
    const float u = t1 + s * p;
    const float c = x.c[col];
    x.gm[col] = c == 0.f ? 0.f : (float)((double)u / (double)c);  // (double, rounded once: the correctly rounded fp32 quotient)
  }
}

// ---- project: the first tiles_da tiles of a job are 64-row stripes of dA (a wave owns 16 rows and walks all of N), the others
// 64-column stripes of dB (a wave owns 16 columns and walks all of K; dW passes through LDS so that it is read with 16-byte loads) --
// DORA (include/sdt.h "DoRA"): the dA stripes scale the B fragment by g as they load it; the dB stripes also read W0 where they stage
// dW, sum G * W0 per column (each staging thread its 8 columns over the rows it stages, top to bottom; the 32 partials of a column in
// row order by one thread), form u = sum_k G W0 + s * sum_q bf16(B) P from their own accumulators and write dB = (s P) g and dm = u / c.
// one 64-row stripe of dA (shared by lora_project_kernel, dora_project_kernel and lora_project_split_kernel: one arithmetic)
template <int RB, bool DORA>  // RB = ceil(r / 16) blocks of 16 adapter columns
__device__ __forceinline__ void project_da_stripe(const SdtLoraJob& d, int tl, const bf16_t* __restrict__ dW, const float* __restrict__ B,
                                                  float* __restrict__ gA, const float* __restrict__ gcol) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r, K = d.K, N = d.N;
  const float s = d.scale;
  f32x4_t acc[RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // dA[k][q] = s * sum_n dW[k][n] * bf16(B[q][n]): A operand dW rows, B operand B^T (both contiguous along n)
  const int row = tl * LT + 16 * wave + l15;
  for (int n0 = 0; n0 < N; n0 += 32) {
    const int n = n0 + 8 * lq;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < K && n < N) v = *reinterpret_cast<const uint4*>(dW + (long)row * N + n);
    const bf16x8_t a = __builtin_bit_cast(bf16x8_t, v);
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      const int q = 16 * b + l15;
      const bf16x8_t bb = DORA ? frag_from_f32_scaled(B + (long)q * N + n, gcol + n, q < r && n < N)
                               : frag_from_f32(B + (long)q * N + n, q < r && n < N);
      acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = tl * LT + 16 * wave + 4 * lq + i, q = 16 * b + l15;
      if (k < K && q < r) gA[(long)k * r + q] = s * acc[b][i];
    }
}

// ---- the walk of a dB stripe (columns c0 .. c0 + 63) down rows [kb, ke) of dW, shared by every projection.  dW passes through LDS so
// that it is read with 16-byte loads: one load per thread stages a 32 x 64 block.  The block is double-buffered: the next block's global
// load is issued in front of this block's MFMAs - body(k0, cur), which reads stage[cur] - and lands in the other buffer behind them,
// one barrier per block.  staged(e, v) sees every vector a thread stages (element e of the leaf, rows top to bottom).  Blocks run
// ascending, so a body that feeds one MFMA chain per rank block keeps one summation order over K whatever [kb, ke) is.
struct NoStagedHook {
  __device__ __forceinline__ void operator()(long, const uint4&) const {}
};

template <class Staged, class Body>
__device__ __forceinline__ void db_walk(const bf16_t* __restrict__ dW, int N, int c0, int kb, int ke, bf16_t (*stage)[32][LT + 8],
                                        Staged staged, Body body) {
  const int srow = threadIdx.x >> 3, scol = (threadIdx.x & 7) * 8;
  const bool col_ok = c0 + scol < N;
  auto load = [&](int k0) {
    uint4 v = {0u, 0u, 0u, 0u};
    if (k0 + srow < ke && col_ok) {
      const long e = (long)(k0 + srow) * N + c0 + scol;
      v = *reinterpret_cast<const uint4*>(dW + e);
      staged(e, v);
    }
    return v;
  };
  *reinterpret_cast<uint4*>(&stage[0][srow][scol]) = load(kb);
  __syncthreads();
  int cur = 0;
  for (int k0 = kb; k0 < ke; k0 += 32, cur ^= 1) {
    const bool more = k0 + 32 < ke;
    uint4 nv = {0u, 0u, 0u, 0u};
    if (more) nv = load(k0 + 32);
    body(k0, cur);
    if (more) *reinterpret_cast<uint4*>(&stage[cur ^ 1][srow][scol]) = nv;  // (its readers finished in front of the last barrier)
    __syncthreads();
  }
}

// the LoRA body: dB[q][n] += sum_k bf16(A[k][q]) * dW[k][n] over the block's rows below ke - A operand A^T (gathered), B operand the
// wave's 16 dW columns out of the staged block
template <int RB>
__device__ __forceinline__ void lora_db_block(const float* __restrict__ A, int r, int k0, int ke, const bf16_t (*blk)[LT + 8], f32x4_t* acc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int k = k0 + 8 * lq;
  bf16x8_t bb;
#pragma unroll
  for (int j = 0; j < 8; ++j) bb[j] = (short)blk[8 * lq + j][16 * wave + l15];
#pragma unroll
  for (int b = 0; b < RB; ++b) {
    const int q = 16 * b + l15;
    const bf16x8_t a = frag_from_f32_strided(A + (long)k * r + q, r, k, ke, q < r);
    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[b], 0, 0, 0);
  }
}

// ---- the end of a dB stripe for SIDES accumulator sets (acc[side][b][i]: q = 16 b + 4 (lane >> 4) + i of the lane's column).
// db_store: dB = s * acc.  db_finish: a stripe of one chunk stores; otherwise the workgroup stores its fp32 partial slab - [r][64] of
// side 0, then of side 1 - (write-through), takes a ticket at the stripe's integer arrival counter, and the last arriver adds the
// slabs in chunk order 0, 1, 2, ... - one thread per element - and writes dB = s * sum.
template <int RB, int SIDES>
__device__ __forceinline__ void db_store(const SdtLoraJob& d, int c0, float* const (&gB)[SIDES], const f32x4_t (&acc)[SIDES][RB]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int n = c0 + 16 * wave + l15;
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 16 * b + 4 * lq + i;
      if (q < d.r && n < d.N) {
#pragma unroll
        for (int sd = 0; sd < SIDES; ++sd) gB[sd][(long)q * d.N + n] = d.scale * acc[sd][b][i];
      }
    }
}

template <int RB, int SIDES>
__device__ __forceinline__ void db_finish(const SdtLoraJob& d, const SdtLoraSplitJob& x, long part_off, int stripe, int chunk,
                                          float* const (&gB)[SIDES], const f32x4_t (&acc)[SIDES][RB], int* __restrict__ counters,
                                          float* __restrict__ parts, int* s_flag) {
  const int c0 = stripe * LT;
  if (x.chunks == 1) {
    db_store<RB, SIDES>(d, c0, gB, acc);
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int side = d.r * LT;                // floats of one set
  const long slab = (long)SIDES * side;     // floats of one workgroup's partial
  float* mine = parts + part_off + ((long)stripe * x.chunks + chunk) * slab;
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 16 * b + 4 * lq + i;
      if (q < d.r) {
#pragma unroll
        for (int sd = 0; sd < SIDES; ++sd) sdt_store_wt(mine + (long)sd * side + (long)q * LT + 16 * wave + l15, acc[sd][b][i]);
      }
    }
  if (!sdt_arrive_last<true>(counters + x.cnt0 + stripe, x.chunks, s_flag)) return;
  const float* first = parts + part_off + (long)stripe * x.chunks * slab;
  for (int e = threadIdx.x; e < (int)slab; e += 256) {
    const bool two = SIDES == 2 && e >= side;
    const int ee = two ? e - side : e;
    const int q = ee >> 6, n = c0 + (ee & 63);
    if (n >= d.N) continue;
    float sum = sdt_load_wt(first + e);
    for (int c = 1; c < x.chunks; ++c) sum += sdt_load_wt(first + c * slab + e);
    (two ? gB[SIDES - 1] : gB[0])[(long)q * d.N + n] = d.scale * sum;
  }
}

// ---- Dense projection: a dB stripe walks all of K in one workgroup (no split: its K is short, and a split would change the order)
template <int RB, bool DORA>
__device__ __forceinline__ void project_tile(const SdtLoraJob& d, int tl, const bf16_t* __restrict__ dW, const float* __restrict__ ab_base,
                                             float* __restrict__ grad_base, bf16_t (*stage)[32][LT + 8], const DoraCols& x) {
  const float* A = ab_base + d.a_off;
  const float* B = ab_base + d.b_off;
  if (tl < d.tiles_da) {
    project_da_stripe<RB, DORA>(d, tl, dW, B, grad_base + d.ga_off, x.g);
    return;
  }
  const int c0 = (tl - d.tiles_da) * LT;
  float* const gB[1] = {grad_base + d.gb_off};
  f32x4_t acc[1][RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) acc[0][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float gw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (DORA) sum over the rows a thread stages of G * W0, per staged column
  db_walk(dW, d.N, c0, 0, d.K, stage,
          [&](long e, const uint4& v) {
            if constexpr (DORA) {
              const float4 w0 = *reinterpret_cast<const float4*>(x.W0 + e), w1 = *reinterpret_cast<const float4*>(x.W0 + e + 4);
              float gf[8];
              unpack8(v, gf);
              gw[0] += gf[0] * w0.x; gw[1] += gf[1] * w0.y; gw[2] += gf[2] * w0.z; gw[3] += gf[3] * w0.w;
              gw[4] += gf[4] * w1.x; gw[5] += gf[5] * w1.y; gw[6] += gf[6] * w1.z; gw[7] += gf[7] * w1.w;
            }
          },
          [&](int k0, int cur) { lora_db_block<RB>(A, d.r, k0, d.K, stage[cur], acc[0]); });
  if constexpr (DORA) dora_db_tail<RB>(d, c0, B, gB[0], acc[0], gw, x); else db_store<RB, 1>(d, c0, gB, acc);
}

__global__ void __launch_bounds__(256) lora_project_kernel(const bf16_t* __restrict__ dw_base, const float* __restrict__ ab_base,
                                                           float* __restrict__ grad_base, const SdtLoraJob* __restrict__ jobs, int njobs) {
  __shared__ __attribute__((aligned(16))) bf16_t stage[2][32][LT + 8];
  const SdtLoraJob d = jobs[find_job_index(jobs, njobs, blockIdx.x, true)];
  const int tl = blockIdx.x - d.tile0_project;
  const DoraCols none = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for_rank_blocks<8>(d.r, [&](auto rb) { project_tile<decltype(rb)::value, false>(d, tl, dw_base + d.dw_off, ab_base, grad_base, stage, none); });
}

__global__ void __launch_bounds__(256) dora_project_kernel(const bf16_t* __restrict__ dw_base, const float* __restrict__ w0_base,
                                                           const float* __restrict__ ab_base, float* __restrict__ grad_base,
                                                           const float* __restrict__ stat_base, const SdtLoraJob* __restrict__ jobs,
                                                           const SdtDoraJob* __restrict__ dj, int njobs) {
  __shared__ __attribute__((aligned(16))) bf16_t stage[2][32][LT + 8];
  __shared__ float red[32][LT];
  const int job = find_job_index(jobs, njobs, blockIdx.x, true);  // (the DoRA table runs beside the job table, index by index)
  const SdtLoraJob d = jobs[job];
  const SdtDoraJob j = dj[job];
  const int tl = blockIdx.x - d.tile0_project;
  const DoraCols x = {w0_base + d.w0_off, stat_base + j.stat_off, stat_base + j.stat_off + d.N, grad_base + j.gm_off, red};
  for_rank_blocks<8>(d.r, [&](auto rb) { project_tile<decltype(rb)::value, true>(d, tl, dw_base + d.dw_off, ab_base, grad_base, stage, x); });
}

// ---- split projection (include/sdt.h "LoCon"): jobs with tall K.  The dA stripes are project_da_stripe; a dB stripe is cut along K
// into chunks of SPLIT_ROWS rows, one workgroup per (stripe, chunk), each a db_walk with the LoRA body over its rows and db_finish
// behind it.  A job of one chunk writes dB = s * acc as project_tile does (the same accumulation order: its bits).
__global__ void __launch_bounds__(256) lora_project_split_kernel(const bf16_t* __restrict__ dw_base, const float* __restrict__ ab_base,
                                                                 float* __restrict__ grad_base, const SdtLoraJob* __restrict__ jobs,
                                                                 const SdtLoraSplitJob* __restrict__ sj, int njobs,
                                                                 int* __restrict__ counters, float* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) bf16_t stage[2][32][LT + 8];
  __shared__ int s_flag;
  const int job = find_index(njobs, blockIdx.x, [=](int i) { return sj[i].tile0; });
  const SdtLoraJob d = jobs[job];
  const SdtLoraSplitJob x = sj[job];
  const int tl = blockIdx.x - x.tile0;
  const bf16_t* dW = dw_base + d.dw_off;
  const float* A = ab_base + d.a_off;
  for_rank_blocks<8>(d.r, [&](auto rb) {
    constexpr int RB = decltype(rb)::value;
    if (tl < d.tiles_da) {
      project_da_stripe<RB, false>(d, tl, dW, ab_base + d.b_off, grad_base + d.ga_off, nullptr);
      return;
    }
    const int t = tl - d.tiles_da, stripe = t / x.chunks, chunk = t % x.chunks;
    const int kb = chunk * SPLIT_ROWS, ke = min(d.K, kb + SPLIT_ROWS);
    float* const gB[1] = {grad_base + d.gb_off};
    f32x4_t acc[1][RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[0][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    db_walk(dW, d.N, stripe * LT, kb, ke, stage, NoStagedHook{}, [&](int k0, int cur) { lora_db_block<RB>(A, d.r, k0, ke, stage[cur], acc[0]); });
    db_finish<RB, 1>(d, x, x.part_off, stripe, chunk, gB, acc, counters, parts, &s_flag);
  });
}

// ---- LoHa (include/sdt.h "LoHa"): dW = s * (A1 B1) o (A2 B2), r <= 32 so that ONE MFMA K-step forms a 16 x 16 block of P_i = bf16(A_i)
// bf16(B_i).  The accumulator layout gives a lane 4 rows of one column, the operand layout wants 8 consecutive contraction elements:
// nothing is moved.  The 16 MFMA rows of a P block are made to stand for contraction elements 8 (m >> 2) + 4 b + (m & 3), b = 0, 1 -
// the factor rows are gathered in that order - so the accumulator registers i = 0..3 of blocks b = 0, 1 ARE elements 8 (lane >> 4) +
// 4 b + i of the lane's own row / column: the eight the operand fragment holds.  G_i = bf16(dW * P_other) is formed in registers.
// The two factor pairs are "sides" 0 and 1: everything per side is an array indexed by it, in loops the compiler unrolls.
// rows X[row][8 lq .. 8 lq + 7] of a factor X [rows][r] as an operand fragment (r in {4, 8, 16, 32}; lanes with q >= r are zero)
__device__ __forceinline__ bf16x8_t loha_rows_frag(const float* __restrict__ X, int r, long row, bool ok, int lq) {
  return r == 4 ? frag_from_f32x4(X + row * 4, ok && lq == 0) : frag_from_f32(X + row * r + 8 * lq, ok && 8 * lq < r);
}
// X[8 lq + j][col], j = 0..7, of a factor X [r][N]
__device__ __forceinline__ bf16x8_t loha_cols_frag(const float* __restrict__ X, int r, int N, int col, bool ok, int lq) {
  return frag_from_f32_strided(X + (long)(8 * lq) * N + col, N, 8 * lq, r, ok);
}
// X[8 lq + j][col] into f0 and X[8 lq + j][col + 1] into f1, j = 0..7, from 8-byte loads (col even; N a multiple of 8: a pair is whole or
// absent): the fragments of two P^T blocks whose MFMA rows interleave, row m of block b standing for column col0 + 2 m + b
__device__ __forceinline__ void loha_col_pairs(const float* __restrict__ X, int r, int N, int col, bool ok, int lq, bf16x8_t& f0,
                                               bf16x8_t& f1) {
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float2 v = {0.f, 0.f};
    if (ok && 8 * lq + j < r) v = *reinterpret_cast<const float2*>(X + (long)(8 * lq + j) * N + col);
    a[j] = v.x;
    b[j] = v.y;
  }
  const uint4 u0 = pack8(a), u1 = pack8(b);
  f0 = __builtin_bit_cast(bf16x8_t, u0);
  f1 = __builtin_bit_cast(bf16x8_t, u1);
}
__device__ __forceinline__ f32x4_t loha_block(bf16x8_t a, bf16x8_t b) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
}

// the factors and their gradients of one job, by side
struct LohaSides {
  const float *A[2], *B[2];
  float *gA[2], *gB[2];
};

// merge: lora_merge_kernel's tiles and runs; h = fl(P1 * P2) in registers, then merged_run's v = fl(W0 + fl(s * h))
__global__ void __launch_bounds__(256) loha_merge_kernel(const float* __restrict__ w0_base, const float* __restrict__ ab_base,
                                                         bf16_t* __restrict__ w_dst, float* __restrict__ f_dst,
                                                         const SdtLoraJob* __restrict__ jobs, const SdtLohaJob* __restrict__ xj, int njobs) {
  __shared__ float tile[LT][LT + 4];
  const MergeTile t = merge_tile(jobs, njobs);
  const SdtLoraJob d = jobs[t.job];
  const SdtLohaJob x = xj[t.job];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const float *B1 = ab_base + d.b_off, *B2 = ab_base + x.b2_off;
  const int arow = t.r0 + 16 * wave + l15;
  const bf16x8_t a1 = loha_rows_frag(ab_base + d.a_off, d.r, arow, arow < d.K, lq);
  const bf16x8_t a2 = loha_rows_frag(ab_base + x.a2_off, d.r, arow, arow < d.K, lq);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = t.c0 + 16 * c + l15;
    const f32x4_t p1 = loha_block(a1, loha_cols_frag(B1, d.r, d.N, col, col < d.N, lq));
    const f32x4_t p2 = loha_block(a2, loha_cols_frag(B2, d.r, d.N, col, col < d.N, lq));
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[16 * wave + 4 * lq + i][16 * c + l15] = p1[i] * p2[i];
  }
  __syncthreads();
  merge_runs<true>(d, w0_base, tile, t.r0, t.c0, w_dst, f_dst);
}

// G[0] = bf16(w * p[1]), G[1] = bf16(w * p[0]) for the lane's eight contraction elements: w = dW widened, p[side][b][i] element
// 4 b + i, or with PAIRS (interleaved blocks) element 2 i + b
template <bool PAIRS>
__device__ __forceinline__ void loha_g_frags(const float* w, const f32x4_t (&p)[2][2], bf16x8_t (&G)[2]) {
#pragma unroll
  for (int sd = 0; sd < 2; ++sd) {
    float g[8];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = PAIRS ? 2 * i + b : 4 * b + i;
        g[j] = w[j] * p[sd ^ 1][b][i];
      }
    const uint4 u = pack8(g);
    G[sd] = __builtin_bit_cast(bf16x8_t, u);
  }
}

// one 64-row stripe of dA1 and dA2: a wave owns 16 rows and walks N, 32 columns a step.  P^T blocks: A operand the B_i columns (MFMA
// row m of block b stands for column n0 + 2 m + b - the interleaved form of the trick above: registers i of blocks b are elements 2 i + b
// of the lane's eight, and a lane fetches both blocks' values with one 8-byte load, 16 lanes a contiguous 128 bytes), B operand the
// lane's own A_i row, loaded once per stripe.
template <int RB>
__device__ __forceinline__ void loha_da_stripe(const SdtLoraJob& d, const LohaSides& o, int tl, const bf16_t* __restrict__ dW) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r, K = d.K, N = d.N;
  const float s = d.scale;
  const int row = tl * LT + 16 * wave + l15;
  f32x4_t acc[2][RB];
  bf16x8_t at[2];
#pragma unroll
  for (int sd = 0; sd < 2; ++sd) {
    at[sd] = loha_rows_frag(o.A[sd], r, row, row < K, lq);
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[sd][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  for (int n0 = 0; n0 < N; n0 += 32) {
    const int n = n0 + 8 * lq, np = n0 + 2 * l15;
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < K && n < N) v = *reinterpret_cast<const uint4*>(dW + (long)row * N + n);
    float w[8];
    unpack8(v, w);
    f32x4_t p[2][2];
#pragma unroll
    for (int sd = 0; sd < 2; ++sd) {
      bf16x8_t f0, f1;
      loha_col_pairs(o.B[sd], r, N, np, np < N, lq, f0, f1);
      p[sd][0] = loha_block(f0, at[sd]);
      p[sd][1] = loha_block(f1, at[sd]);
    }
    bf16x8_t G[2];
    loha_g_frags<true>(w, p, G);
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        const int q = 16 * b + l15;
        acc[sd][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(G[sd], frag_from_f32(o.B[sd] + (long)q * N + n, q < r && n < N), acc[sd][b], 0, 0, 0);
      }
  }
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = tl * LT + 16 * wave + 4 * lq + i, q = 16 * b + l15;
      if (k < K && q < r) {
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) o.gA[sd][(long)k * r + q] = s * acc[sd][b][i];
      }
    }
}

// one (stripe, chunk) of dB1 and dB2: a db_walk over the chunk's rows and the two-sided db_finish (a stripe always takes the split
// table).  P blocks: A operand the A_i rows (MFMA row m stands for row k0 + 8 (m >> 2) + 4 b + (m & 3)), B operand the lane's own B_i
// column, loaded once per chunk.
template <int RB>
__device__ __forceinline__ void loha_db_chunk(const SdtLoraJob& d, const SdtLoraSplitJob& x, const LohaSides& o, long part_off, int stripe,
                                              int chunk, const bf16_t* __restrict__ dW, int* __restrict__ counters,
                                              float* __restrict__ parts, bf16_t (*stage)[32][LT + 8], int* s_flag) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r, N = d.N;
  const int kb = chunk * SPLIT_ROWS, ke = min(d.K, kb + SPLIT_ROWS);
  const int ncol = stripe * LT + 16 * wave + l15;
  const int kl = 8 * (l15 >> 2) + (l15 & 3);
  f32x4_t acc[2][RB];
  bf16x8_t bc[2];
#pragma unroll
  for (int sd = 0; sd < 2; ++sd) {
    bc[sd] = loha_cols_frag(o.B[sd], r, N, ncol, ncol < N, lq);
#pragma unroll
    for (int b = 0; b < RB; ++b) acc[sd][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  db_walk(dW, N, stripe * LT, kb, ke, stage, NoStagedHook{}, [&](int k0, int cur) {
    const int k = k0 + 8 * lq;
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = bf2f(stage[cur][8 * lq + j][16 * wave + l15]);
    f32x4_t p[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        const int kp = k0 + kl + 4 * b;
        p[sd][b] = loha_block(loha_rows_frag(o.A[sd], r, kp, kp < ke, lq), bc[sd]);
      }
    bf16x8_t G[2];
    loha_g_frags<false>(w, p, G);
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        const int q = 16 * b + l15;
        acc[sd][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_from_f32_strided(o.A[sd] + (long)k * r + q, r, k, ke, q < r), G[sd], acc[sd][b], 0, 0, 0);
      }
  });
  db_finish<RB, 2>(d, x, part_off, stripe, chunk, o.gB, acc, counters, parts, s_flag);
}

// (4 waves per SIMD are requested: a fourth workgroup per CU hides the gathers.  113 VGPRs and no AGPRs with the request; 107 + 16
// without it, which still fits four - the request pins the occupancy against the next change to the body)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) loha_project_kernel(const bf16_t* __restrict__ dw_base, const float* __restrict__ ab_base,
                                                           float* __restrict__ grad_base, const SdtLoraJob* __restrict__ jobs,
                                                           const SdtLoraSplitJob* __restrict__ sj, const SdtLohaJob* __restrict__ xj,
                                                           int njobs, int* __restrict__ counters, float* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) bf16_t stage[2][32][LT + 8];
  __shared__ int s_flag;
  const int job = find_index(njobs, blockIdx.x, [=](int i) { return sj[i].tile0; });
  const SdtLoraJob d = jobs[job];
  const SdtLoraSplitJob x = sj[job];
  const SdtLohaJob h = xj[job];
  const int tl = blockIdx.x - x.tile0;
  const bf16_t* dW = dw_base + d.dw_off;
  const LohaSides o = {{ab_base + d.a_off, ab_base + h.a2_off}, {ab_base + d.b_off, ab_base + h.b2_off},
                       {grad_base + d.ga_off, grad_base + h.ga2_off}, {grad_base + d.gb_off, grad_base + h.gb2_off}};
  for_rank_blocks<2>(d.r, [&](auto rb) {
    constexpr int RB = decltype(rb)::value;
    if (tl < d.tiles_da) {
      loha_da_stripe<RB>(d, o, tl, dW);
      return;
    }
    const int t = tl - d.tiles_da;
    loha_db_chunk<RB>(d, x, o, h.part_off, t / x.chunks, t % x.chunks, dW, counters, parts, stage, &s_flag);
  });
}

// Host check of the table (the host copy; the device copy must hold the same bytes).  Returns the number of tiles or -1.
long check_jobs(const char* name, const SdtLoraJob* h, int n, bool project) {
  long tiles = 0;
  for (int i = 0; i < n; ++i) {
    const SdtLoraJob& j = h[i];
    const int r = j.r;
    if (!(r == 4 || r == 8 || r == 16 || r == 32 || r == 64 || r == 128)) {
      sdt_set_error("%s: job %d: rank %d is not one of 4, 8, 16, 32, 64, 128", name, i, r);
      return -1;
    }
    if (j.K <= 0 || j.N <= 0 || j.K % 8 || j.N % 8) {
      sdt_set_error("%s: job %d: K=%d and N=%d must be positive multiples of 8", name, i, j.K, j.N);
      return -1;
    }
    const int64_t offs[8] = {j.w0_off, j.a_off, j.b_off, j.w_off, j.f_off, j.dw_off, j.ga_off, j.gb_off};
    for (int o = 0; o < 8; ++o)
      if (offs[o] < 0 || offs[o] % 8) {
        sdt_set_error("%s: job %d: offsets must be non-negative multiples of 8 elements", name, i);
        return -1;
      }
    const long tm = (long)((j.K + LT - 1) / LT) * ((j.N + LT - 1) / LT);
    const long ta = (j.K + LT - 1) / LT, tb = (j.N + LT - 1) / LT;
    if ((project ? j.tile0_project : j.tile0_merge) != tiles || j.tiles_da != ta) {
      sdt_set_error("%s: job %d: tile0 / tiles_da do not continue the running tile count", name, i);
      return -1;
    }
    tiles += project ? ta + tb : tm;
    if (tiles >= (1L << 31)) {
      sdt_set_error("%s: too many tiles", name);
      return -1;
    }
  }
  return tiles;
}

// The DoRA table beside the job table (host copies).  Returns the number of merge stripes or -1.
long check_dora_jobs(const char* name, const SdtLoraJob* h, const SdtDoraJob* x, int n) {
  long stripes = 0;
  for (int i = 0; i < n; ++i) {
    if (x[i].N != h[i].N) {
      sdt_set_error("%s: job %d: the DoRA table names N=%d, the job table N=%d (mismatched tables)", name, i, x[i].N, h[i].N);
      return -1;
    }
    const int64_t offs[3] = {x[i].m_off, x[i].gm_off, x[i].stat_off};
    for (int o = 0; o < 3; ++o)
      if (offs[o] < 0 || offs[o] % 8) {
        sdt_set_error("%s: job %d: DoRA offsets must be non-negative multiples of 8 elements", name, i);
        return -1;
      }
    if (x[i].stripe0_merge != stripes) {
      sdt_set_error("%s: job %d: stripe0_merge does not continue the running stripe count", name, i);
      return -1;
    }
    stripes += (h[i].N + LT - 1) / LT;
    if (stripes >= (1L << 31)) {
      sdt_set_error("%s: too many stripes", name);
      return -1;
    }
  }
  return stripes;
}

// The chunk and stripe arithmetic of the split projections, once: what a job adds to the workgroups (tiles), the arrival counters (one
// per dB stripe) and the partial floats (`sides` slabs of [r][64] per stripe and chunk, none for a job of one chunk) of its table.
struct SplitCount {
  long tiles = 0, counters = 0, floats = 0;
  void add(const SdtLoraJob& j, int sides) {
    const long chunks = (j.K + SPLIT_ROWS - 1) / SPLIT_ROWS, stripes = (j.N + LT - 1) / LT;
    tiles += j.tiles_da + stripes * chunks;
    counters += stripes;
    if (chunks > 1) floats += sides * stripes * chunks * j.r * LT;
  }
  long bytes() const { return (counters * 4 + 255) / 256 * 256 + 4 * floats; }  // the workspace: counters, padded to 256 bytes, then partials
  long counter_bytes() const { return bytes() - 4 * floats; }
};
SplitCount split_count(const SdtLoraJob* h, int n, int sides) {
  SplitCount t;
  for (int i = 0; i < n; ++i) t.add(h[i], sides);
  return t;
}

// The split table beside the job table (host copies; part_off counts one side's partials).  False with the message set for a bad table.
bool check_split_jobs(const char* name, const SdtLoraJob* h, const SdtLoraSplitJob* x, int n) {
  SplitCount t;
  for (int i = 0; i < n; ++i) {
    if (x[i].K != h[i].K || x[i].N != h[i].N) {
      sdt_set_error("%s: job %d: the split table names K=%d N=%d, the job table K=%d N=%d (mismatched tables)", name, i, x[i].K, x[i].N,
                    h[i].K, h[i].N);
      return false;
    }
    const long chunks = (h[i].K + SPLIT_ROWS - 1) / SPLIT_ROWS;
    if (x[i].chunks != chunks) {
      sdt_set_error("%s: job %d: chunks=%d, K=%d makes %ld chunks of %d rows", name, i, x[i].chunks, h[i].K, chunks, SPLIT_ROWS);
      return false;
    }
    if (x[i].tile0 != t.tiles || x[i].cnt0 != t.counters) {
      sdt_set_error("%s: job %d: tile0 / cnt0 do not continue the running tile and stripe counts", name, i);
      return false;
    }
    if (x[i].part_off != t.floats) {
      sdt_set_error("%s: job %d: part_off=%lld does not continue the running partial offset %ld", name, i, (long long)x[i].part_off,
                    t.floats);
      return false;
    }
    t.add(h[i], 1);
    if (t.tiles >= (1L << 31) || t.counters >= (1L << 31)) {
      sdt_set_error("%s: too many tiles", name);
      return false;
    }
  }
  return true;
}

// The LoHa table beside the job table (host copies): ranks up to 32, K / N equal, side-2 offsets, the running offset of the two-set
// partials.  False with the message set for a bad table.
bool check_loha_jobs(const char* name, const SdtLoraJob* h, const SdtLohaJob* x, int n) {
  SplitCount t;
  for (int i = 0; i < n; ++i) {
    if (h[i].r > 32) {
      sdt_set_error("%s: job %d: rank %d: LoHa takes the ranks 4, 8, 16 and 32 (one MFMA K-step forms a block of A B)", name, i, h[i].r);
      return false;
    }
    if (x[i].K != h[i].K || x[i].N != h[i].N) {
      sdt_set_error("%s: job %d: the LoHa table names K=%d N=%d, the job table K=%d N=%d (mismatched tables)", name, i, x[i].K, x[i].N,
                    h[i].K, h[i].N);
      return false;
    }
    const int64_t offs[4] = {x[i].a2_off, x[i].b2_off, x[i].ga2_off, x[i].gb2_off};
    for (int o = 0; o < 4; ++o)
      if (offs[o] < 0 || offs[o] % 8) {
        sdt_set_error("%s: job %d: LoHa offsets must be non-negative multiples of 8 elements", name, i);
        return false;
      }
    if (x[i].part_off != t.floats) {
      sdt_set_error("%s: job %d: LoHa part_off=%lld does not continue the running partial offset %ld", name, i, (long long)x[i].part_off,
                    t.floats);
      return false;
    }
    t.add(h[i], 2);
  }
  return true;
}

// The preamble of every launching entry point, in this order: n >= 0; n == 0 has nothing to do (SDT_OK, before anything else is looked
// at); the tables, the pointers and a destination exist; the OR of the addresses is 16-byte aligned.  ENTRY_GO: go on.
constexpr int ENTRY_GO = 1;
int entry_args(const char* name, int n, bool tables, bool pointers, bool destination, uintptr_t addresses) {
  SDT_CHECK_ARG(n >= 0, "%s: negative job count", name);
  if (n == 0) return SDT_OK;
  SDT_CHECK_ARG(tables, "%s: null job table", name);
  SDT_CHECK_ARG(pointers, "%s: null pointer", name);
  SDT_CHECK_ARG(destination, "%s: no destination", name);
  SDT_CHECK_ARG((addresses & 15) == 0, "%s: pointers must be 16-byte aligned", name);
  return ENTRY_GO;
}
template <class... P>
uintptr_t address_bits(P... p) { return (... | (uintptr_t)p); }

// The workspace of a split projection over the table, or -1: counters and `sides` sets of partials.
int64_t split_workspace_bytes(const char* name, const SdtLoraJob* jobs_host, int n, int sides) {
  if (n < 0 || (n > 0 && !jobs_host)) {
    sdt_set_error("%s: bad job table", name);
    return -1;
  }
  if (check_jobs(name, jobs_host, n, true) < 0) return -1;
  for (int i = 0; sides == 2 && i < n; ++i)
    if (jobs_host[i].r > 32) {
      sdt_set_error("%s: job %d: rank %d: LoHa takes the ranks 4, 8, 16 and 32", name, i, jobs_host[i].r);
      return -1;
    }
  return split_count(jobs_host, n, sides).bytes();
}

}  // namespace

extern "C" {

int sdt_lora_job_size(void) { return (int)sizeof(SdtLoraJob); }
int sdt_dora_job_size(void) { return (int)sizeof(SdtDoraJob); }
int sdt_lora_split_job_size(void) { return (int)sizeof(SdtLoraSplitJob); }
int sdt_loha_job_size(void) { return (int)sizeof(SdtLohaJob); }
int sdt_lora_project_split_rows(void) { return SPLIT_ROWS; }

int sdt_lora_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, const SdtLoraJob* jobs_host,
                   const void* jobs_device, int n, hipStream_t stream) {
  if (const int rc = entry_args("sdt_lora_merge", n, jobs_host && jobs_device, w0_base && ab_base, w_bf16 || f32_dst,
                                address_bits(w0_base, ab_base, w_bf16, f32_dst)); rc != ENTRY_GO) return rc;
  const long tiles = check_jobs("sdt_lora_merge", jobs_host, n, false);
  if (tiles < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0_base, ab_base, (bf16_t*)w_bf16, f32_dst,
                     (const SdtLoraJob*)jobs_device, n);
  SDT_LAUNCH_CHECK("sdt_lora_merge");
  return SDT_OK;
}

int sdt_lora_restore(const float* w0_base, uint16_t* w_bf16, const SdtLoraJob* jobs_host, const void* jobs_device, int n,
                     hipStream_t stream) {
  if (const int rc = entry_args("sdt_lora_restore", n, jobs_host && jobs_device, w0_base && w_bf16, true, address_bits(w0_base, w_bf16));
      rc != ENTRY_GO) return rc;
  const long tiles = check_jobs("sdt_lora_restore", jobs_host, n, false);
  if (tiles < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_restore_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0_base, (bf16_t*)w_bf16,
                     (const SdtLoraJob*)jobs_device, n);
  SDT_LAUNCH_CHECK("sdt_lora_restore");
  return SDT_OK;
}

int sdt_lora_project(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                     const void* jobs_device, int n, hipStream_t stream) {
  if (const int rc = entry_args("sdt_lora_project", n, jobs_host && jobs_device, dw_base && ab_base && grad_base, true,
                                address_bits(dw_base, ab_base, grad_base)); rc != ENTRY_GO) return rc;
  const long tiles = check_jobs("sdt_lora_project", jobs_host, n, true);
  if (tiles < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_project_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, (const bf16_t*)dw_base, ab_base, grad_base,
                     (const SdtLoraJob*)jobs_device, n);
  SDT_LAUNCH_CHECK("sdt_lora_project");
  return SDT_OK;
}

int64_t sdt_lora_project_split_workspace_bytes(const SdtLoraJob* jobs_host, int n) {
  return split_workspace_bytes("sdt_lora_project_split_workspace_bytes", jobs_host, n, 1);
}

int sdt_lora_project_split(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                           const SdtLoraSplitJob* split_host, const void* jobs_device, const void* split_device, int n, void* workspace,
                           int64_t workspace_bytes, hipStream_t stream) {
  if (const int rc = entry_args("sdt_lora_project_split", n, jobs_host && jobs_device && split_host && split_device,
                                dw_base && ab_base && grad_base && workspace, true, address_bits(dw_base, ab_base, grad_base, workspace));
      rc != ENTRY_GO) return rc;
  if (check_jobs("sdt_lora_project_split", jobs_host, n, true) < 0) return SDT_ERR_INVALID_ARG;
  if (!check_split_jobs("sdt_lora_project_split", jobs_host, split_host, n)) return SDT_ERR_INVALID_ARG;
  const SplitCount t = split_count(jobs_host, n, 1);
  if (workspace_bytes < t.bytes()) {
    sdt_set_error("sdt_lora_project_split: the workspace holds %lld bytes, the table needs %ld (counters and partials inside the workspace)",
                  (long long)workspace_bytes, t.bytes());
    return SDT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(lora_project_split_kernel, dim3((unsigned)t.tiles), dim3(256), 0, stream, (const bf16_t*)dw_base, ab_base, grad_base,
                     (const SdtLoraJob*)jobs_device, (const SdtLoraSplitJob*)split_device, n, (int*)workspace,
                     (float*)((char*)workspace + t.counter_bytes()));
  SDT_LAUNCH_CHECK("sdt_lora_project_split");
  return SDT_OK;
}

int sdt_loha_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, const SdtLoraJob* jobs_host,
                   const SdtLohaJob* loha_host, const void* jobs_device, const void* loha_device, int n, hipStream_t stream) {
  if (const int rc = entry_args("sdt_loha_merge", n, jobs_host && jobs_device && loha_host && loha_device, w0_base && ab_base,
                                w_bf16 || f32_dst, address_bits(w0_base, ab_base, w_bf16, f32_dst)); rc != ENTRY_GO) return rc;
  const long tiles = check_jobs("sdt_loha_merge", jobs_host, n, false);
  if (tiles < 0 || !check_loha_jobs("sdt_loha_merge", jobs_host, loha_host, n)) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(loha_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0_base, ab_base, (bf16_t*)w_bf16, f32_dst,
                     (const SdtLoraJob*)jobs_device, (const SdtLohaJob*)loha_device, n);
  SDT_LAUNCH_CHECK("sdt_loha_merge");
  return SDT_OK;
}

int64_t sdt_loha_project_workspace_bytes(const SdtLoraJob* jobs_host, int n) {
  return split_workspace_bytes("sdt_loha_project_workspace_bytes", jobs_host, n, 2);
}

int sdt_loha_project(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                     const SdtLoraSplitJob* split_host, const SdtLohaJob* loha_host, const void* jobs_device, const void* split_device,
                     const void* loha_device, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (const int rc = entry_args("sdt_loha_project", n, jobs_host && jobs_device && split_host && split_device && loha_host && loha_device,
                                dw_base && ab_base && grad_base && workspace, true, address_bits(dw_base, ab_base, grad_base, workspace));
      rc != ENTRY_GO) return rc;
  if (check_jobs("sdt_loha_project", jobs_host, n, true) < 0) return SDT_ERR_INVALID_ARG;
  if (!check_loha_jobs("sdt_loha_project", jobs_host, loha_host, n)) return SDT_ERR_INVALID_ARG;
  if (!check_split_jobs("sdt_loha_project", jobs_host, split_host, n)) return SDT_ERR_INVALID_ARG;
  const SplitCount t = split_count(jobs_host, n, 2);
  if (workspace_bytes < t.bytes()) {
    sdt_set_error("sdt_loha_project: the workspace holds %lld bytes, the table needs %ld (counters and two sets of partials inside the workspace)",
                  (long long)workspace_bytes, t.bytes());
    return SDT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(loha_project_kernel, dim3((unsigned)t.tiles), dim3(256), 0, stream, (const bf16_t*)dw_base, ab_base, grad_base,
                     (const SdtLoraJob*)jobs_device, (const SdtLoraSplitJob*)split_device, (const SdtLohaJob*)loha_device, n,
                     (int*)workspace, (float*)((char*)workspace + t.counter_bytes()));
  SDT_LAUNCH_CHECK("sdt_loha_project");
  return SDT_OK;
}

int sdt_dora_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, float* stat_base,
                   const SdtLoraJob* jobs_host, const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n,
                   hipStream_t stream) {
  if (const int rc = entry_args("sdt_dora_merge", n, jobs_host && jobs_device && dora_host && dora_device, w0_base && ab_base && stat_base,
                                w_bf16 || f32_dst, address_bits(w0_base, ab_base, w_bf16, f32_dst, stat_base)); rc != ENTRY_GO) return rc;
  if (check_jobs("sdt_dora_merge", jobs_host, n, false) < 0) return SDT_ERR_INVALID_ARG;
  const long stripes = check_dora_jobs("sdt_dora_merge", jobs_host, dora_host, n);
  if (stripes < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(dora_merge_kernel<false>, dim3((unsigned)stripes), dim3(256), 0, stream, w0_base, ab_base, (bf16_t*)w_bf16, f32_dst,
                     stat_base, (float*)nullptr, (const SdtLoraJob*)jobs_device, (const SdtDoraJob*)dora_device, n);
  SDT_LAUNCH_CHECK("sdt_dora_merge");
  return SDT_OK;
}

int sdt_dora_init_magnitude(const float* w0_base, const float* ab_base, float* m_base, const SdtLoraJob* jobs_host,
                            const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n, hipStream_t stream) {
  if (const int rc = entry_args("sdt_dora_init_magnitude", n, jobs_host && jobs_device && dora_host && dora_device,
                                w0_base && ab_base && m_base, true, address_bits(w0_base, ab_base, m_base)); rc != ENTRY_GO) return rc;
  if (check_jobs("sdt_dora_init_magnitude", jobs_host, n, false) < 0) return SDT_ERR_INVALID_ARG;
  const long stripes = check_dora_jobs("sdt_dora_init_magnitude", jobs_host, dora_host, n);
  if (stripes < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(dora_merge_kernel<true>, dim3((unsigned)stripes), dim3(256), 0, stream, w0_base, ab_base, (bf16_t*)nullptr,
                     (float*)nullptr, (float*)nullptr, m_base, (const SdtLoraJob*)jobs_device, (const SdtDoraJob*)dora_device, n);
  SDT_LAUNCH_CHECK("sdt_dora_init_magnitude");
  return SDT_OK;
}

int sdt_dora_project(const uint16_t* dw_base, const float* w0_base, const float* ab_base, float* grad_base, const float* stat_base,
                     const SdtLoraJob* jobs_host, const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n,
                     hipStream_t stream) {
  if (const int rc = entry_args("sdt_dora_project", n, jobs_host && jobs_device && dora_host && dora_device,
                                dw_base && w0_base && ab_base && grad_base && stat_base, true,
                                address_bits(dw_base, w0_base, ab_base, grad_base, stat_base)); rc != ENTRY_GO) return rc;
  const long tiles = check_jobs("sdt_dora_project", jobs_host, n, true);
  if (tiles < 0 || check_dora_jobs("sdt_dora_project", jobs_host, dora_host, n) < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(dora_project_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, (const bf16_t*)dw_base, w0_base, ab_base, grad_base,
                     stat_base, (const SdtLoraJob*)jobs_device, (const SdtDoraJob*)dora_device, n);
  SDT_LAUNCH_CHECK("sdt_dora_project");
  return SDT_OK;
}

}  // extern "C"
