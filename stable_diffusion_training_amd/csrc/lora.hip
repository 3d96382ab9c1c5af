// Low-rank adapters in weight space (include/sdt.h "LoRA"): the merge W = bf16(W0 + s * A * B) in front of a step and the projection
// of the bf16 weight gradient dW back onto the factors, dA = s * dW * B^T and dB = s * A^T * dW, behind its backward.  Both are
// grouped launches over one device job table with running tile counts (like sdt_param_prepare's descriptors), both round A and B to
// bf16 as they load them (the projection differentiates the function the merge evaluated), both accumulate in fp32 on
// mfma_f32_16x16x32_bf16 and neither uses an atomic: every output element has one writer and one fixed summation order.
//
// Operand lane maps of mfma_f32_16x16x32_bf16 (lane l): A[row l&15][k = 8(l>>4) + j], B[k = 8(l>>4) + j][col l&15], j = 0..7;
// C/D col = l&15, row = 4(l>>4) + reg.
#include "sdt_common.h"

namespace {

constexpr int LT = 64;  // merge: output tile; project: rows of a dA stripe / columns of a dB stripe

__device__ __forceinline__ const SdtLoraJob& find_job(const SdtLoraJob* jobs, int n, int tile, bool project) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {  // last job whose first tile is <= tile
    const int mid = (lo + hi + 1) >> 1;
    if ((project ? jobs[mid].tile0_project : jobs[mid].tile0_merge) <= tile) lo = mid; else hi = mid - 1;
  }
  return jobs[lo];
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
__global__ void __launch_bounds__(256) lora_merge_kernel(const float* __restrict__ w0_base, const float* __restrict__ ab_base,
                                                         bf16_t* __restrict__ w_dst, float* __restrict__ f_dst,
                                                         const SdtLoraJob* __restrict__ jobs, int njobs) {
  __shared__ float tile[LT][LT + 4];
  const SdtLoraJob d = find_job(jobs, njobs, blockIdx.x, false);
  const int tl = blockIdx.x - d.tile0_merge;
  const int tc = (d.N + LT - 1) / LT;
  const int r0 = (tl / tc) * LT, c0 = (tl % tc) * LT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const float* A = ab_base + d.a_off;  // [K][r]
  const float* B = ab_base + d.b_off;  // [r][N]
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
  __syncthreads();
  const float s = d.scale;
#pragma unroll
  for (int it = 0; it < 2; ++it) {  // 512 runs of 8 columns: 16-byte bf16 stores
    const int g = threadIdx.x + 256 * it;
    const int row = r0 + (g >> 3), col = c0 + (g & 7) * 8;
    if (row >= d.K || col >= d.N) continue;  // N is a multiple of 8: a run is whole or absent
    const long e = (long)row * d.N + col;
    const float* src = w0_base + d.w0_off + e;
    const float4 x0 = *reinterpret_cast<const float4*>(src), x1 = *reinterpret_cast<const float4*>(src + 4);
    const float* t = &tile[g >> 3][(g & 7) * 8];
    float v[8];
    v[0] = x0.x + s * t[0]; v[1] = x0.y + s * t[1]; v[2] = x0.z + s * t[2]; v[3] = x0.w + s * t[3];
    v[4] = x1.x + s * t[4]; v[5] = x1.y + s * t[5]; v[6] = x1.z + s * t[6]; v[7] = x1.w + s * t[7];
    if (w_dst) *reinterpret_cast<uint4*>(w_dst + d.w_off + e) = pack8(v);
    if (f_dst) {
      float* o = f_dst + d.f_off + e;
      *reinterpret_cast<float4*>(o) = float4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<float4*>(o + 4) = float4{v[4], v[5], v[6], v[7]};
    }
  }
}

// ---- project: the first tiles_da tiles of a job are 64-row stripes of dA (a wave owns 16 rows and walks all of N), the others
// 64-column stripes of dB (a wave owns 16 columns and walks all of K; dW passes through LDS so that it is read with 16-byte loads) --
template <int RB>  // RB = ceil(r / 16) blocks of 16 adapter columns
__device__ __forceinline__ void project_tile(const SdtLoraJob& d, int tl, const bf16_t* __restrict__ dW, const float* __restrict__ A,
                                             const float* __restrict__ B, float* __restrict__ gA, float* __restrict__ gB,
                                             bf16_t (*stage)[LT + 8]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
  const int r = d.r, K = d.K, N = d.N;
  const float s = d.scale;
  f32x4_t acc[RB];
#pragma unroll
  for (int b = 0; b < RB; ++b) acc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if (tl < d.tiles_da) {
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
        const bf16x8_t bb = frag_from_f32(B + (long)q * N + n, q < r && n < N);
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
    return;
  }
  // dB[q][n] = s * sum_k bf16(A[k][q]) * dW[k][n]: A operand A^T (gathered), B operand dW columns out of the staged 32 x 64 block
  const int c0 = (tl - d.tiles_da) * LT;
  const int srow = threadIdx.x >> 3, scol = (threadIdx.x & 7) * 8;  // one 16-byte load per thread stages 32 rows x 64 columns
  for (int k0 = 0; k0 < K; k0 += 32) {
    uint4 v = {0u, 0u, 0u, 0u};
    if (k0 + srow < K && c0 + scol < N) v = *reinterpret_cast<const uint4*>(dW + (long)(k0 + srow) * N + c0 + scol);
    __syncthreads();  // the previous block has been consumed
    *reinterpret_cast<uint4*>(&stage[srow][scol]) = v;
    __syncthreads();
    const int k = k0 + 8 * lq;
    bf16x8_t bb;
#pragma unroll
    for (int j = 0; j < 8; ++j) bb[j] = (short)stage[8 * lq + j][16 * wave + l15];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      const int q = 16 * b + l15;
      const bf16x8_t a = frag_from_f32_strided(A + (long)k * r + q, r, k, K, q < r);
      acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bb, acc[b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = 16 * b + 4 * lq + i, n = c0 + 16 * wave + l15;
      if (q < r && n < N) gB[(long)q * N + n] = s * acc[b][i];
    }
}

__global__ void __launch_bounds__(256) lora_project_kernel(const bf16_t* __restrict__ dw_base, const float* __restrict__ ab_base,
                                                           float* __restrict__ grad_base, const SdtLoraJob* __restrict__ jobs, int njobs) {
  __shared__ __attribute__((aligned(16))) bf16_t stage[32][LT + 8];
  const SdtLoraJob d = find_job(jobs, njobs, blockIdx.x, true);
  const int tl = blockIdx.x - d.tile0_project;
  const bf16_t* dW = dw_base + d.dw_off;
  const float* A = ab_base + d.a_off;
  const float* B = ab_base + d.b_off;
  float* gA = grad_base + d.ga_off;
  float* gB = grad_base + d.gb_off;
  switch ((d.r + 15) / 16) {  // (workgroup-uniform)
    case 1: project_tile<1>(d, tl, dW, A, B, gA, gB, stage); break;
    case 2: project_tile<2>(d, tl, dW, A, B, gA, gB, stage); break;
    case 4: project_tile<4>(d, tl, dW, A, B, gA, gB, stage); break;
    default: project_tile<8>(d, tl, dW, A, B, gA, gB, stage); break;
  }
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

}  // namespace

extern "C" {

int sdt_lora_job_size(void) { return (int)sizeof(SdtLoraJob); }

int sdt_lora_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, const SdtLoraJob* jobs_host,
                   const void* jobs_device, int n, hipStream_t stream) {
  SDT_CHECK_ARG(n >= 0, "sdt_lora_merge: negative job count");
  if (n == 0) return SDT_OK;
  SDT_CHECK_ARG(jobs_host && jobs_device, "sdt_lora_merge: null job table");
  SDT_CHECK_ARG(w0_base && ab_base, "sdt_lora_merge: null pointer");
  SDT_CHECK_ARG(w_bf16 || f32_dst, "sdt_lora_merge: no destination");
  SDT_CHECK_ARG((((uintptr_t)w0_base | (uintptr_t)ab_base | (uintptr_t)w_bf16 | (uintptr_t)f32_dst) & 15) == 0,
                "sdt_lora_merge: pointers must be 16-byte aligned");
  const long tiles = check_jobs("sdt_lora_merge", jobs_host, n, false);
  if (tiles < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, w0_base, ab_base, (bf16_t*)w_bf16, f32_dst,
                     (const SdtLoraJob*)jobs_device, n);
  SDT_LAUNCH_CHECK("sdt_lora_merge");
  return SDT_OK;
}

int sdt_lora_project(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                     const void* jobs_device, int n, hipStream_t stream) {
  SDT_CHECK_ARG(n >= 0, "sdt_lora_project: negative job count");
  if (n == 0) return SDT_OK;
  SDT_CHECK_ARG(jobs_host && jobs_device, "sdt_lora_project: null job table");
  SDT_CHECK_ARG(dw_base && ab_base && grad_base, "sdt_lora_project: null pointer");
  SDT_CHECK_ARG((((uintptr_t)dw_base | (uintptr_t)ab_base | (uintptr_t)grad_base) & 15) == 0,
                "sdt_lora_project: pointers must be 16-byte aligned");
  const long tiles = check_jobs("sdt_lora_project", jobs_host, n, true);
  if (tiles < 0) return SDT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(lora_project_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, (const bf16_t*)dw_base, ab_base, grad_base,
                     (const SdtLoraJob*)jobs_device, n);
  SDT_LAUNCH_CHECK("sdt_lora_project");
  return SDT_OK;
}

}  // extern "C"
