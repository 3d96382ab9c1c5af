// IP-Adapter's image-token term of a decoupled cross-attention (include/sdt.h "IP-ADAPTER"), fused with the add into the text
// attention's output:  out = o_txt + scale_ip[b] * softmax(scale q K_ip^T) V_ip  over T <= 16 image tokens.
// T keys do not fill an MFMA tile, so everything runs on the vector ALUs.  One thread owns one VEC-element column chunk of one
// query row; a workgroup covers RB whole rows (all heads), so every global access of q / o_txt / out / dout / dq is a run of
// consecutive 16-byte (VEC = 8) or 8-byte (VEC = 4) pieces.  A head is D / VEC consecutive chunks - 5 for D = 40, 10 for D = 80: no
// power of two, so the per-head sums go through LDS in two steps instead of lane shuffles:
//   1  every thread writes its chunk's part of the T dot products              part[t][thread]
//   2  thread ci of a head adds the head's parts, chunk order, for t = ci, ci + D/VEC, ...    sc[row][head][t]
//   3  every thread reads the T finished values of its (row, head)
// The keys and values are read from global memory where they are used: at most 80 KiB per image, shared by every workgroup of the
// image, they stay in L2 / L1 (cdna_hip_programming Appendix B "Attention decode": operands a wave does not share go straight to VGPRs).
// No float atomics and no cross-workgroup hand-off: the backward's dK / dV leave each thread as an fp32 partial in a slot of its own
// and a second small launch adds the slots in index order.
// Every multiply-add below is an explicit fmaf and the file is compiled with -ffp-contract=off (the pragma repeats it), so the
// compiler fuses nothing else: the rounding points are the ones sdt.h lists, whatever the optimiser does.
#include "sdt_common.h"

#pragma clang fp contract(off)

namespace {

struct IpPlan {
  int vec, tmax, cph, cpr, rb, nt, iters, nblk, slots;
  size_t lds_fwd, lds_bwd;
};

// The partition depends on the shape alone (never on alignment or on the device): vec = elements per thread, rb = rows per pass of
// a workgroup, iters = passes, nblk workgroups per image; the backward has one partial slot per workgroup.
static IpPlan ip_plan(int B, int H, int Nq, int T, int D, bool bwd) {
  IpPlan p;
  p.tmax = T <= 4 ? 4 : 16;
  p.vec = (bwd && T > 4) ? 4 : 8;  // the backward holds 2 * tmax * vec fp32 accumulators per thread
  const int C = H * D;
  p.cph = D / p.vec;
  p.cpr = C / p.vec;
  p.rb = 256 / p.cpr < 1 ? 1 : 256 / p.cpr;
  p.nt = (p.rb * p.cpr + 63) / 64 * 64;
  const long groups = ((long)Nq + p.rb - 1) / p.rb;
  // passes per workgroup.  Forward: a few, while the grid stays above ~2048 workgroups.  Backward: a workgroup leaves ONE fp32
  // partial of T x 2C values, so it takes ~16 T rows (the partials then move < 10% of what the rows move) unless that would leave
  // fewer than ~256 workgroups (measured at SD1.5's shapes: four times as many workgroups, and partials, cost 0.7 ms more per pass).
  const long par = groups * B / (bwd ? 256 : 2048), traffic = bwd ? (16L * T + p.rb - 1) / p.rb : 4;
  const long it = par < traffic ? par : traffic;
  p.iters = (int)(it < 1 ? 1 : it);
  p.nblk = (int)((groups + p.iters - 1) / p.iters);
  p.slots = p.nblk;
  p.lds_fwd = sizeof(float) * (size_t)p.tmax * ((size_t)p.nt + (size_t)p.rb * H);
  const size_t steps = (size_t)p.tmax * ((size_t)p.nt + 2 * (size_t)p.rb * H), fold = (size_t)p.nt * 2 * p.vec;
  p.lds_bwd = sizeof(float) * (steps > fold ? steps : fold);
  return p;
}

template <int VEC, bool AL>
__device__ __forceinline__ void ip_load(const bf16_t* p, float* f) {
  if constexpr (AL && VEC == 8) {
    unpack8(*reinterpret_cast<const uint4*>(p), f);
  } else if constexpr (AL && VEC == 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    const f32x4_t u = unpack4(v.x, v.y);
    f[0] = u[0]; f[1] = u[1]; f[2] = u[2]; f[3] = u[3];
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) f[j] = bf2f(p[j]);
  }
}

template <int VEC, bool AL>
__device__ __forceinline__ void ip_store(bf16_t* p, const bf16_t* o) {
  if constexpr (AL && VEC == 8) {
    *reinterpret_cast<uint4*>(p) = make_uint4(o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16), o[4] | ((unsigned)o[5] << 16),
                                              o[6] | ((unsigned)o[7] << 16));
  } else if constexpr (AL && VEC == 4) {
    *reinterpret_cast<uint2*>(p) = make_uint2(o[0] | ((unsigned)o[1] << 16), o[2] | ((unsigned)o[3] << 16));
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) p[j] = o[j];
  }
}

template <int VEC>
__device__ __forceinline__ float ip_dot(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) s = fmaf(a[j], b[j], s);
  return s;
}

// step 2 of the header: the head's sums for the keys this thread finishes, parts added in chunk order from +0, times `mul`
__device__ __forceinline__ void ip_head_sums(const float* part, float* dst, int nt, int first, int cph, int ci, int T, float mul) {
  for (int t = ci; t < T; t += cph) {
    float s = 0.f;
    for (int j = 0; j < cph; ++j) s += part[t * nt + first + j];
    dst[t] = mul * s;
  }
}

// p = softmax over the T finished logits: max, expf of the differences, their sum in key order from +0, one IEEE division each
template <int TMAX>
__device__ __forceinline__ void ip_softmax(const float* sc, int T, float* p) {
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    p[t] = t < T ? sc[t] : -INFINITY;
    m = fmaxf(m, p[t]);
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < TMAX; ++t) {
    p[t] = t < T ? expf(p[t] - m) : 0.f;
    sum += p[t];
  }
#pragma unroll
  for (int t = 0; t < TMAX; ++t) p[t] = p[t] / sum;
}

template <int TMAX, bool AL>
__global__ void __launch_bounds__(512) ip_attn_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv,
                                                          const bf16_t* __restrict__ o_txt, const float* __restrict__ scale_ip,
                                                          bf16_t* __restrict__ out, int H, int Nq, int T, int D, int ldq, int ldkv,
                                                          float scale, int cph, int cpr, int rb, int iters) {
  constexpr int VEC = 8;
  extern __shared__ float ip_smem[];
  const int nt = blockDim.x, tid = threadIdx.x, b = blockIdx.y, C = H * D;
  float* part = ip_smem;           // [TMAX][nt]
  float* sc = ip_smem + TMAX * nt; // [rb * H][TMAX]
  const bool lane_ok = tid < rb * cpr;
  const int r = tid / cpr, c = tid - r * cpr, h = c / cph, ci = c - h * cph;
  const float sip = scale_ip ? scale_ip[b] : 1.f;
  const bf16_t* kvb = kv + (long)b * T * ldkv;  // uniform base, 32-bit lane offsets below
  const int kc = c * VEC;
  for (int it = 0; it < iters; ++it) {
    const int row = (blockIdx.x * iters + it) * rb + r;
    const bool ok = lane_ok && row < Nq;
    if (ok) {
      float qf[VEC], kf[VEC];
      ip_load<VEC, AL>(q + ((long)b * Nq + row) * ldq + c * VEC, qf);
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) {
          ip_load<VEC, AL>(kvb + (t * ldkv + kc), kf);
          part[t * nt + tid] = ip_dot<VEC>(qf, kf);
        }
    }
    __syncthreads();
    if (ok) ip_head_sums(part, sc + (r * H + h) * TMAX, nt, r * cpr + h * cph, cph, ci, T, scale);
    __syncthreads();
    if (ok) {
      float p[TMAX], acc[VEC], vf[VEC];
      ip_softmax<TMAX>(sc + (r * H + h) * TMAX, T, p);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) {
          ip_load<VEC, AL>(kvb + (t * ldkv + C + kc), vf);
#pragma unroll
          for (int j = 0; j < VEC; ++j) acc[j] = fmaf(p[t], vf[j], acc[j]);
        }
      const long o = ((long)b * Nq + row) * C + c * VEC;
      float of[VEC];
      if (o_txt) {
        ip_load<VEC, AL>(o_txt + o, of);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) of[j] = 0.f;
      }
      bf16_t ob[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) ob[j] = double_to_bf16_rne((double)of[j] + (double)sip * (double)acc[j]);
      ip_store<VEC, AL>(out + o, ob);
    }
  }
}

template <int TMAX, int VEC, bool AL>
__global__ void __launch_bounds__(512) ip_attn_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kv,
                                                          const bf16_t* __restrict__ dout, const float* __restrict__ scale_ip,
                                                          const bf16_t* __restrict__ dq_in, bf16_t* __restrict__ dq,
                                                          float* __restrict__ partials, int H, int Nq, int T, int D, int ldq, int ldkv,
                                                          float scale, int cph, int cpr, int rb, int iters, int slots) {
  extern __shared__ float ip_smem[];
  const int nt = blockDim.x, tid = threadIdx.x, b = blockIdx.y, C = H * D;
  float* part = ip_smem;               // [TMAX][nt], used twice per pass
  float* sc = ip_smem + TMAX * nt;     // [rb * H][TMAX] logits
  float* dpv = sc + rb * H * TMAX;     // [rb * H][TMAX] dP = g . v
  const bool lane_ok = tid < rb * cpr;
  const int r = tid / cpr, c = tid - r * cpr, h = c / cph, ci = c - h * cph;
  const float sip = scale_ip ? scale_ip[b] : 1.f;
  const bf16_t* kvb = kv + (long)b * T * ldkv;  // uniform base, 32-bit lane offsets below
  const int kc = c * VEC;
  float dk[TMAX][VEC], dv[TMAX][VEC];
#pragma unroll
  for (int t = 0; t < TMAX; ++t)
#pragma unroll
    for (int j = 0; j < VEC; ++j) dk[t][j] = dv[t][j] = 0.f;
  for (int it = 0; it < iters; ++it) {
    const int row = (blockIdx.x * iters + it) * rb + r;
    const bool ok = lane_ok && row < Nq;
    const int hs = (r * H + h) * TMAX, first = r * cpr + h * cph;
    float qf[VEC], gf[VEC], tf[VEC];
    if (ok) {
      ip_load<VEC, AL>(q + ((long)b * Nq + row) * ldq + c * VEC, qf);
      ip_load<VEC, AL>(dout + ((long)b * Nq + row) * C + c * VEC, gf);
#pragma unroll
      for (int j = 0; j < VEC; ++j) gf[j] = sip * gf[j];
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) {
          ip_load<VEC, AL>(kvb + (t * ldkv + kc), tf);
          part[t * nt + tid] = ip_dot<VEC>(qf, tf);
        }
    }
    __syncthreads();
    if (ok) ip_head_sums(part, sc + hs, nt, first, cph, ci, T, scale);
    __syncthreads();
    if (ok) {
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) {
          ip_load<VEC, AL>(kvb + (t * ldkv + C + kc), tf);
          part[t * nt + tid] = ip_dot<VEC>(gf, tf);
        }
    }
    __syncthreads();
    if (ok) ip_head_sums(part, dpv + hs, nt, first, cph, ci, T, 1.f);
    __syncthreads();
    if (ok) {
      // ip_softmax's arithmetic with p[t] formed where it is used (twice) instead of held: with 2 * TMAX * VEC accumulators live, T
      // more registers for p and T for dP would spill at TMAX = 16; the logits and dP stay in LDS
      float acc[VEC], m = -INFINITY, sum = 0.f, delta = 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) m = fmaxf(m, sc[hs + t]);
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) sum += expf(sc[hs + t] - m);
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) delta = fmaf(expf(sc[hs + t] - m) / sum, dpv[hs + t], delta);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll
      for (int t = 0; t < TMAX; ++t)
        if (t < T) {
          const float p = expf(sc[hs + t] - m) / sum;
          const float ds = p * (dpv[hs + t] - delta);
          ip_load<VEC, AL>(kvb + (t * ldkv + kc), tf);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            acc[j] = fmaf(ds, tf[j], acc[j]);
            dk[t][j] = fmaf(ds, qf[j], dk[t][j]);
            dv[t][j] = fmaf(p, gf[j], dv[t][j]);
          }
        }
      const long o = ((long)b * Nq + row) * C + c * VEC;
      float df[VEC];
      bf16_t ob[VEC];
      if (dq_in) {
        ip_load<VEC, AL>(dq_in + o, df);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) df[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) ob[j] = double_to_bf16_rne((double)df[j] + (double)(scale * acc[j]));
      ip_store<VEC, AL>(dq + o, ob);
    }
  }
  // The rb row threads of a column chunk fold into one partial, key by key through LDS: thread r = 0 adds them in row-thread order
  // from its own.  Every workgroup writes its slot, rows or none: the finishing launch adds them all.
  float* fold = ip_smem;  // [nt][2 * VEC]
  float* w = partials + (((long)b * slots + blockIdx.x) * T) * 2 * C + c * VEC;
#pragma unroll
  for (int t = 0; t < TMAX; ++t)
    if (t < T) {  // uniform
      __syncthreads();
      if (lane_ok && r > 0) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          fold[tid * 2 * VEC + j] = dk[t][j];
          fold[tid * 2 * VEC + VEC + j] = dv[t][j];
        }
      }
      __syncthreads();
      if (lane_ok && r == 0) {
        for (int rr = 1; rr < rb; ++rr) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            dk[t][j] += fold[(rr * cpr + c) * 2 * VEC + j];
            dv[t][j] += fold[(rr * cpr + c) * 2 * VEC + VEC + j];
          }
        }
#pragma unroll
        for (int j = 0; j < VEC; j += 4) {
          *reinterpret_cast<float4*>(w + (long)t * 2 * C + j) = make_float4(dk[t][j], dk[t][j + 1], dk[t][j + 2], dk[t][j + 3]);
          *reinterpret_cast<float4*>(w + (long)t * 2 * C + C + j) = make_float4(dv[t][j], dv[t][j + 1], dv[t][j + 2], dv[t][j + 3]);
        }
      }
    }
}

// dkv[b][t][col] = bf16 of the slots' sum in slot order from +0 (columns [0, C): dK, times scale; [C, 2C): dV)
__global__ void __launch_bounds__(256) ip_attn_dkv_finish_kernel(const float* __restrict__ partials, bf16_t* __restrict__ dkv, long total,
                                                                 int T, int C, int slots, int ld_dkv, float scale) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int W = 2 * C, col = (int)(i % W);
  const long bt = i / W;
  const int t = (int)(bt % T);
  const long b = bt / T;
  const float* p = partials + (b * slots * T + t) * W + col;
  // the adds stay in slot order; the loads of eight slots are issued together so that a thread does not wait for each in turn
  float s = 0.f;
  const long step = (long)T * W;
  int k = 0;
  for (; k + 8 <= slots; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(k + u) * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < slots; ++k) s += p[k * step];
  dkv[bt * ld_dkv + col] = f2bf(col < C ? scale * s : s);
}

static bool ip_aligned(const void* p, int bytes) { return p == nullptr || ((uintptr_t)p % bytes) == 0; }

static int ip_check_shape(const char* fn, int B, int H, int Nq, int T, int D) {
  SDT_CHECK_ARG(B >= 1 && H >= 1 && Nq >= 1, "%s: B=%d H=%d Nq=%d must be positive", fn, B, H, Nq);
  SDT_CHECK_ARG(T >= 1 && T <= 16, "%s: T=%d image tokens (1..16 are served)", fn, T);
  SDT_CHECK_ARG(D >= 8 && D <= 160 && D % 8 == 0, "%s: head dim D=%d (a multiple of 8 up to 160)", fn, D);
  SDT_CHECK_ARG((long)H * D <= 2048, "%s: H*D=%ld is wider than 2048 channels", fn, (long)H * D);
  SDT_CHECK_ARG((long)B <= 65535, "%s: B=%d is more than 65535 images", fn, B);
  return SDT_OK;
}

}  // namespace

extern "C" int64_t sdt_ip_attention_bwd_workspace_bytes(int B, int H, int Nq, int T, int D) {
  if (ip_check_shape("sdt_ip_attention_bwd_workspace_bytes", B, H, Nq, T, D) != SDT_OK) return -1;
  const IpPlan p = ip_plan(B, H, Nq, T, D, true);
  return SDT_WS_COUNTER_BYTES + (int64_t)sizeof(float) * B * p.slots * T * 2 * H * D;
}

extern "C" int sdt_ip_attention_fwd(const uint16_t* q, const uint16_t* kv, const uint16_t* o_txt, const float* scale_ip, uint16_t* out,
                                    int B, int H, int Nq, int T, int D, int ldq, int ldkv, float scale, hipStream_t stream) {
  const char* fn = "sdt_ip_attention_fwd";
  SDT_CHECK_ARG(q && kv && out, "%s: null pointer (q, kv and out are required)", fn);
  if (int rc = ip_check_shape(fn, B, H, Nq, T, D)) return rc;
  const int C = H * D;
  SDT_CHECK_ARG(ldq >= C && ldkv >= 2 * C, "%s: row strides ldq=%d ldkv=%d are narrower than C=%d / 2C", fn, ldq, ldkv, C);
  SDT_CHECK_ARG(ip_aligned(q, 2) && ip_aligned(kv, 2) && ip_aligned(o_txt, 2) && ip_aligned(out, 2) && ip_aligned(scale_ip, 4),
                "%s: misaligned pointer (bf16 operands: 2 bytes, scale_ip: 4)", fn);
  const IpPlan p = ip_plan(B, H, Nq, T, D, false);
  SDT_CHECK_ARG(p.lds_fwd <= 65536, "%s: H=%d heads of D=%d need %zu bytes of LDS (64 KiB are served)", fn, H, D, p.lds_fwd);
  const bool al = ip_aligned(q, 16) && ip_aligned(kv, 16) && ip_aligned(o_txt, 16) && ip_aligned(out, 16) && ldq % 8 == 0 && ldkv % 8 == 0;
  const dim3 grid(p.nblk, B), block(p.nt);
#define IP_FWD(TM, AL)                                                                                                              \
  hipLaunchKernelGGL((ip_attn_fwd_kernel<TM, AL>), grid, block, p.lds_fwd, stream, q, kv, o_txt, scale_ip, out, H, Nq, T, D, ldq, ldkv, \
                     scale, p.cph, p.cpr, p.rb, p.iters)
  if (p.tmax == 4) { if (al) IP_FWD(4, true); else IP_FWD(4, false); }
  else             { if (al) IP_FWD(16, true); else IP_FWD(16, false); }
#undef IP_FWD
  SDT_LAUNCH_CHECK(fn);
  return SDT_OK;
}

extern "C" int sdt_ip_attention_bwd(const uint16_t* q, const uint16_t* kv, const uint16_t* dout, const float* scale_ip,
                                    const uint16_t* dq_in, uint16_t* dq, uint16_t* dkv, int B, int H, int Nq, int T, int D, int ldq,
                                    int ldkv, int ld_dkv, float scale, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "sdt_ip_attention_bwd";
  SDT_CHECK_ARG(q && kv && dout && dq && dkv && workspace, "%s: null pointer (q, kv, dout, dq, dkv and the workspace are required)", fn);
  if (int rc = ip_check_shape(fn, B, H, Nq, T, D)) return rc;
  const int C = H * D;
  SDT_CHECK_ARG(ldq >= C && ldkv >= 2 * C && ld_dkv >= 2 * C, "%s: row strides ldq=%d ldkv=%d ld_dkv=%d are narrower than C=%d / 2C", fn,
                ldq, ldkv, ld_dkv, C);
  SDT_CHECK_ARG(ip_aligned(q, 2) && ip_aligned(kv, 2) && ip_aligned(dout, 2) && ip_aligned(dq_in, 2) && ip_aligned(dq, 2) &&
                    ip_aligned(dkv, 2) && ip_aligned(scale_ip, 4) && ip_aligned(workspace, 16),
                "%s: misaligned pointer (bf16 operands: 2 bytes, scale_ip: 4, workspace: 16)", fn);
  const IpPlan p = ip_plan(B, H, Nq, T, D, true);
  const int64_t need = sdt_ip_attention_bwd_workspace_bytes(B, H, Nq, T, D);
  SDT_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %ld bytes, %ld needed", fn, (long)workspace_bytes, (long)need);
  SDT_CHECK_ARG(p.lds_bwd <= 65536, "%s: H=%d heads of D=%d need %zu bytes of LDS (64 KiB are served)", fn, H, D, p.lds_bwd);
  const int ab = 2 * p.vec;  // bytes of one vector access
  const bool al = ip_aligned(q, ab) && ip_aligned(kv, ab) && ip_aligned(dout, ab) && ip_aligned(dq_in, ab) && ip_aligned(dq, ab) &&
                  ldq % p.vec == 0 && ldkv % p.vec == 0;
  float* partials = reinterpret_cast<float*>(static_cast<char*>(workspace) + SDT_WS_COUNTER_BYTES);
  const dim3 grid(p.nblk, B), block(p.nt);
#define IP_BWD(TM, V, AL)                                                                                                          \
  hipLaunchKernelGGL((ip_attn_bwd_kernel<TM, V, AL>), grid, block, p.lds_bwd, stream, q, kv, dout, scale_ip, dq_in, dq, partials, H, Nq, \
                     T, D, ldq, ldkv, scale, p.cph, p.cpr, p.rb, p.iters, p.slots)
  if (p.tmax == 4) { if (al) IP_BWD(4, 8, true); else IP_BWD(4, 8, false); }
  else             { if (al) IP_BWD(16, 4, true); else IP_BWD(16, 4, false); }
#undef IP_BWD
  SDT_LAUNCH_CHECK(fn);
  const long total = (long)B * T * 2 * C;
  hipLaunchKernelGGL(ip_attn_dkv_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, partials, dkv, total, T, C,
                     p.slots, ld_dkv, scale);
  SDT_LAUNCH_CHECK(fn);
  return SDT_OK;
}
