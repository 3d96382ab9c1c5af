// HBM-bound optimizer sweep: global-norm reduction, fused clip + Lion (8-bit blockwise or fp32
// momentum) + weight decay + parameter update + EMA + bf16 re-cast, one pass over the flat
// parameter buffer.  Replaces, for the reference:
//   optax.clip_by_global_norm(1)                      training_utils.py:380, :417
//   lion_quant.py:52-64 (_quantize/_dequantize), :66-92 (block codec), :133-154 (update_fn)
//   add_decayed_weights / -lr / apply_updates         lion_quant.py:201-211, training_utils.py:732-733
//   compute_model_ema                                 training_utils.py:537-544
// Algorithmic bytes per parameter: g 4r + p 4r/4w + code 1r/1w + scale (4r/4w)/block (+ema 4r/4w, +bf16 2w).
// This translation unit is compiled with -ffp-contract=off so that every multiply/add rounds
// separately, as the NumPy float32 oracle (and XLA elementwise f32) does.
#include "sdt_common.h"

#define LION_OFFSET 3.7398995e-09f  // lion_quant.py:49

__device__ __forceinline__ float lion_deq(int code) {  // lion_quant.py:61-64
  float t = (float)code / 127.0f;
  float t2 = t * t;
  float t4 = t2 * t2;
  return t4 * t - LION_OFFSET;
}
// _quantize (lion_quant.py:52-59): code = rint(sign(x + offset) * |x + offset|^(1/5) * 127).
// The same integer without powf: _quantize is a monotone step function of a = |x + offset|, described exactly by the 127
// float32 thresholds thr[c] = smallest a whose code is >= c (thr[0] = 0, thr[128] = +inf; built on the host with the float32
// power / multiply / rint of the definition, lion_codec.quantization_thresholds).  v_log_f32 / v_exp_f32 give the code to
// well within one unit; two threshold reads settle it: thr[c] <= a < thr[c + 1].  Bit-exact against the host definition at
// every rounding boundary, and no device/host pow ulp disagreement (the HBM-bound sweep was VALU-bound on powf).
__device__ __forceinline__ int lion_quant_tab(float x, const float* __restrict__ thr) {
  const float xo = x + LION_OFFSET;
  const float a = fabsf(xo);
  const float q = __builtin_amdgcn_exp2f(0.2f * __builtin_amdgcn_logf(a)) * 127.0f;
  const float r = rintf(q);
  int c = (int)fminf(fmaxf(r, 0.f), 127.f);
  // the estimate is good to ~2e-5 code units (1-ulp v_log / v_exp): only values within 2.5e-4 of a rounding boundary can
  // land on the wrong side and need the table (about one element in 2000; the others skip the two LDS reads)
  if (fabsf(q - r) > 0.5f - 2.5e-4f) c += (a >= thr[c + 1] ? 1 : 0) - (a < thr[c] ? 1 : 0);
  return xo < 0.f ? -c : c;
}
__device__ __forceinline__ void lion_load_tables(float* deq_tab, float* thr_tab, const float* __restrict__ thr) {
  // exact lion_deq() of every int8 code (the /127 and the 5th power done once) and the codec thresholds, in LDS
  for (int i = threadIdx.x; i < 256; i += blockDim.x) deq_tab[i] = lion_deq(i - 128);
  for (int i = threadIdx.x; i < 129; i += blockDim.x) thr_tab[i] = i < 128 ? thr[i] : __builtin_inff();
  __syncthreads();
}

// Sum of squares in double: every product of two floats is exact in double and the running sum carries ~1e-16 relative
// error, so the float32 norm the optimizer kernels derive from it is the float32 rounding of the true norm - the value
// optax.global_norm rounds to - and the clipped gradients (g / norm) match the host definition bit for bit.  The pass is
// HBM-bound (4 B per parameter); four double FMAs per 16 bytes are far below the fp64 vector rate.
// Workgroups store their double partial sums to `part`; the one that arrives last adds them in workgroup order into *out (no
// float / double atomics: the norm, and with it every clipped gradient, is bitwise reproducible).
// G16: the buffer holds bf16 values (the kernel leaves' gradients [r4]): four per 8 bytes, widened exactly.
template <bool G16>
__global__ void __launch_bounds__(256) sqnorm_kernel(const void* __restrict__ gv, long n, double* __restrict__ out, int* counter,
                                                     double* __restrict__ part) {
  const long nv = n >> 2;
  double d0 = 0.0, d1 = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    float4 v;
    if (G16) {
      const uint2 h = reinterpret_cast<const uint2*>(gv)[i];
      v.x = __uint_as_float(h.x << 16); v.y = __uint_as_float(h.x & 0xffff0000u);
      v.z = __uint_as_float(h.y << 16); v.w = __uint_as_float(h.y & 0xffff0000u);
    } else {
      v = reinterpret_cast<const float4*>(gv)[i];
    }
    d0 = fma((double)v.x, (double)v.x, d0);
    d1 = fma((double)v.y, (double)v.y, d1);
    d0 = fma((double)v.z, (double)v.z, d0);
    d1 = fma((double)v.w, (double)v.w, d1);
  }
  double dacc = d0 + d1;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = G16 ? bf2f(reinterpret_cast<const bf16_t*>(gv)[(nv << 2) + threadIdx.x]) : reinterpret_cast<const float*>(gv)[(nv << 2) + threadIdx.x];
    dacc += (double)v * (double)v;
  }
  for (int o = 32; o > 0; o >>= 1) dacc += __shfl_xor(dacc, o, 64);
  __shared__ double dsc[16];
  __shared__ int s_last;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) dsc[w] = dacc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += dsc[i];
    sdt_store_wt(part + blockIdx.x, t);
  }
  if (!sdt_arrive_last<true>(counter, (int)gridDim.x, &s_last)) return;
  // last arriver: 256 threads x strided partials, then a fixed tree
  double t = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += sdt_load_wt(part + i);
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) dsc[w] = t;
  __syncthreads();
  if (threadIdx.x == 0) *out += (dsc[0] + dsc[1]) + (dsc[2] + dsc[3]);
}

// Micro-batch gradient accumulation (include/sdt.h sdt_grad_accumulate): acc (fp32) <- init / add / finish / scale of the step's
// gradient g (bf16 or fp32, widened exactly), element-wise, in one HBM-bound sweep: init 6 B (bf16 g) per element, add and finish
// 10 B, scale 8 B.  With NORM the sweep also adds sum acc_final^2 to *out exactly as sqnorm_kernel does over the finished buffer -
// same grid (the caller passes sqnorm_kernel's), same float4 walk and d0 / d1 alternation, same per-workgroup partials and ordered
// last-arriver sum - so the squared norm is bit-identical to sdt_sqnorm_accumulate run over acc afterwards.
template <bool G16, int MODE, bool NORM>
__global__ void __launch_bounds__(256) grad_accumulate_kernel(float* __restrict__ acc, const void* __restrict__ gv, long n, float scale,
                                                              double* __restrict__ out, int* counter, double* __restrict__ part) {
  const long nv = n >> 2;
  double d0 = 0.0, d1 = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (MODE != SDT_ACC_SCALE) {
      if (G16) {
        const uint2 h = reinterpret_cast<const uint2*>(gv)[i];
        v.x = __uint_as_float(h.x << 16); v.y = __uint_as_float(h.x & 0xffff0000u);
        v.z = __uint_as_float(h.y << 16); v.w = __uint_as_float(h.y & 0xffff0000u);
      } else {
        v = reinterpret_cast<const float4*>(gv)[i];
      }
    }
    if (MODE != SDT_ACC_INIT) {
      const float4 a = reinterpret_cast<const float4*>(acc)[i];
      if (MODE == SDT_ACC_SCALE) {
        v.x = a.x * scale; v.y = a.y * scale; v.z = a.z * scale; v.w = a.w * scale;
      } else {
        v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w;
        if (MODE == SDT_ACC_FINISH) {
          v.x = v.x * scale; v.y = v.y * scale; v.z = v.z * scale; v.w = v.w * scale;
        }
      }
    }
    reinterpret_cast<float4*>(acc)[i] = v;
    if (NORM) {
      d0 = fma((double)v.x, (double)v.x, d0);
      d1 = fma((double)v.y, (double)v.y, d1);
      d0 = fma((double)v.z, (double)v.z, d0);
      d1 = fma((double)v.w, (double)v.w, d1);
    }
  }
  double dacc = d0 + d1;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // the < 4 elements behind the last float4
    const long j = (nv << 2) + threadIdx.x;
    float v = 0.f;
    if (MODE != SDT_ACC_SCALE) v = G16 ? bf2f(reinterpret_cast<const bf16_t*>(gv)[j]) : reinterpret_cast<const float*>(gv)[j];
    if (MODE == SDT_ACC_SCALE) v = acc[j] * scale;
    else if (MODE != SDT_ACC_INIT) v = acc[j] + v;
    if (MODE == SDT_ACC_FINISH) v = v * scale;
    acc[j] = v;
    dacc += (double)v * (double)v;
  }
  if (!NORM) return;
  for (int o = 32; o > 0; o >>= 1) dacc += __shfl_xor(dacc, o, 64);
  __shared__ double dsc[16];
  __shared__ int s_last;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) dsc[w] = dacc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += dsc[i];
    sdt_store_wt(part + blockIdx.x, t);
  }
  if (!sdt_arrive_last<true>(counter, (int)gridDim.x, &s_last)) return;
  double t = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += sdt_load_wt(part + i);
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) dsc[w] = t;
  __syncthreads();
  if (threadIdx.x == 0) *out += (dsc[0] + dsc[1]) + (dsc[2] + dsc[3]);
}

// *out += sum of n doubles, added in a fixed order (contiguous chunk per workgroup, strided over the threads, the sqnorm_kernel's
// tree): the squared-norm partials the weight-gradient kernels wrote to their slots (include/sdt.h sdt_gemm_tn_wgrad sq_slots).
__global__ void __launch_bounds__(256) sum_f64_kernel(const double* __restrict__ x, long n, double* __restrict__ out, int* counter,
                                                      double* __restrict__ part) {
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = per * blockIdx.x, hi = lo + per < n ? lo + per : n;
  double d0 = 0.0, d1 = 0.0;
  long i = lo + threadIdx.x;
  for (; i + 256 < hi; i += 512) {
    d0 += x[i];
    d1 += x[i + 256];
  }
  if (i < hi) d0 += x[i];
  double dacc = d0 + d1;
  for (int o = 32; o > 0; o >>= 1) dacc += __shfl_xor(dacc, o, 64);
  __shared__ double dsc[16];
  __shared__ int s_last;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) dsc[w] = dacc;
  __syncthreads();
  if (threadIdx.x == 0) sdt_store_wt(part + blockIdx.x, (dsc[0] + dsc[1]) + (dsc[2] + dsc[3]));
  if (!sdt_arrive_last<true>(counter, (int)gridDim.x, &s_last)) return;
  double t = 0.0;
  for (int j = threadIdx.x; j < (int)gridDim.x; j += 256) t += sdt_load_wt(part + j);
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) dsc[w] = t;
  __syncthreads();
  if (threadIdx.x == 0) *out += (dsc[0] + dsc[1]) + (dsc[2] + dsc[3]);
}

// clip factor semantics of optax.clip_by_global_norm: g if norm < max else (g / norm) * max
__device__ __forceinline__ float clip_grad(float g, float gnorm, float max_norm, bool do_clip) {
  return do_clip ? (g / gnorm) * max_norm : g;
}

// LPB lanes cooperate on one quantisation block of BS = 4*LPB elements; each lane owns a float4.
#define LION_SLICES 4
// SCHED: neg_lr, ema_r and ema_rm come from the device block `cur` that opt_schedule_select_kernel wrote for this step (the by-value
// arguments are ignored); the instantiations without it are the by-value sweeps.
template <int LPB, bool G16, bool SCHED>
__global__ void __launch_bounds__(256) lion8_kernel(float* __restrict__ p, const void* __restrict__ g,
                                                    int8_t* __restrict__ codes, float* __restrict__ inv_scale,
                                                    float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n4,
                                                    const double* __restrict__ sqnorm, const float* __restrict__ thr,
                                                    float max_norm, float neg_lr, float wd, float c1, float c1m, float c2,
                                                    float c2m, float ema_r, float ema_rm, const float* __restrict__ cur) {
  __shared__ float deq_tab[256];
  __shared__ float thr_tab[132];
  if (SCHED) {
    neg_lr = cur[0];
    ema_r = cur[1];
    ema_rm = cur[2];
  }
  lion_load_tables(deq_tab, thr_tab, thr);
  float gnorm = 0.f;
  bool do_clip = false;
  if (sqnorm) {
    gnorm = (float)sqrt(*sqnorm);
    do_clip = !(gnorm < max_norm);
  }
  // n4 is a multiple of LPB and consecutive lanes hold consecutive float4s, so the LPB lanes of a block stay together.
  // A workgroup sweeps LION_SLICES consecutive slices of 256 float4s and the grid covers the buffer once: the resident
  // workgroups then work on ONE contiguous window of each of the seven streams (a capped grid striding over the whole buffers
  // ran the sweep at 4.1 instead of 5.9 TB/s), and every byte is touched once per step, so all of it moves non-temporally.
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const long i_end = min(n4, ((long)blockIdx.x + 1) * (LION_SLICES * 256));
  for (long i = (long)blockIdx.x * (LION_SLICES * 256) + threadIdx.x; i < i_end; i += 256) {
    f4v gv;
    if (G16) {  // bf16 gradient (8 bytes per float4 of parameters), widened exactly: what optax sees of a bf16 cotangent
      const u2v h = __builtin_nontemporal_load(&reinterpret_cast<const u2v*>(g)[i]);
      gv.x = __uint_as_float(h.x << 16); gv.y = __uint_as_float(h.x & 0xffff0000u);
      gv.z = __uint_as_float(h.y << 16); gv.w = __uint_as_float(h.y & 0xffff0000u);
    } else {
      gv = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(g)[i]);
    }
    const f4v pv = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(p)[i]);
    const unsigned cw = __builtin_nontemporal_load(&reinterpret_cast<const unsigned*>(codes)[i]);
    const long blk = i / LPB;
    const float inv = inv_scale[blk];
    float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    float mn[4];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int c = (int)(int8_t)((cw >> (8 * j)) & 0xff);
      float mf = deq_tab[c + 128] / inv;                    // lion_quant.py:88-91
      float gc = clip_grad(gg[j], gnorm, max_norm, do_clip);
      float cc = c1m * gc + c1 * mf;                        // lion_quant.py:141-143
      float u = (cc > 0.f) ? 1.f : ((cc < 0.f) ? -1.f : 0.f);
      mn[j] = c2m * gc + c2 * mf;                           // lion_quant.py:105-107
      amax = fmaxf(amax, fabsf(mn[j]));
      if (wd != 0.f) u = u + wd * pp[j];                    // add_decayed_weights
      u = neg_lr * u;                                       // _scale_by_learning_rate
      pp[j] = pp[j] + u;                                    // apply_updates
    }
#pragma unroll
    for (int o = 1; o < LPB; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float ninv = 1.0f / ((amax <= 0.f) ? 1.0f : amax);  // lion_quant.py:72-76
    unsigned ncw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int q = lion_quant_tab(mn[j] * ninv, thr_tab);
      ncw |= ((unsigned)(q & 0xff)) << (8 * j);
    }
    __builtin_nontemporal_store(ncw, &reinterpret_cast<unsigned*>(codes)[i]);
    if ((i % LPB) == 0) inv_scale[blk] = ninv;
    {
      const f4v o = {pp[0], pp[1], pp[2], pp[3]};
      __builtin_nontemporal_store(o, &reinterpret_cast<f4v*>(p)[i]);
    }
    if (ema) {
      f4v ev = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(ema)[i]);
      ev.x = ema_r * ev.x + ema_rm * pp[0];
      ev.y = ema_r * ev.y + ema_rm * pp[1];
      ev.z = ema_r * ev.z + ema_rm * pp[2];
      ev.w = ema_r * ev.w + ema_rm * pp[3];
      __builtin_nontemporal_store(ev, &reinterpret_cast<f4v*>(ema)[i]);
    }
    if (w_bf16) {
      const u2v o = {pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
      __builtin_nontemporal_store(o, &reinterpret_cast<u2v*>(w_bf16)[i]);
    }
  }
}

template <bool SCHED>  // as lion8_kernel
__global__ void __launch_bounds__(256) lion32_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ mom, float* __restrict__ ema,
                                                     bf16_t* __restrict__ w_bf16, long n,
                                                     const double* __restrict__ sqnorm, float max_norm, float neg_lr,
                                                     float wd, float c1, float c1m, float c2, float c2m, float ema_r,
                                                     float ema_rm, const float* __restrict__ cur) {
  if (SCHED) {
    neg_lr = cur[0];
    ema_r = cur[1];
    ema_rm = cur[2];
  }
  float gnorm = 0.f;
  bool do_clip = false;
  if (sqnorm) {
    gnorm = (float)sqrt(*sqnorm);
    do_clip = !(gnorm < max_norm);
  }
  const long i_end = min(n, ((long)blockIdx.x + 1) * 1024);  // a contiguous 1024-element slice per workgroup (see lion8_kernel)
  for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < i_end; i += 256) {
    float gc = clip_grad(g[i], gnorm, max_norm, do_clip);
    float mf = mom[i];
    float pv = p[i];
    float cc = c1m * gc + c1 * mf;
    float u = (cc > 0.f) ? 1.f : ((cc < 0.f) ? -1.f : 0.f);
    mom[i] = c2m * gc + c2 * mf;
    if (wd != 0.f) u = u + wd * pv;
    u = neg_lr * u;
    pv = pv + u;
    p[i] = pv;
    if (ema) ema[i] = ema_r * ema[i] + ema_rm * pv;
    if (w_bf16) w_bf16[i] = f2bf(pv);
  }
}

__global__ void __launch_bounds__(256) lion8_quantize_kernel(const float* __restrict__ x, int8_t* __restrict__ codes,
                                                             float* __restrict__ inv_scale, long nblocks, int bs,
                                                             const float* __restrict__ thr) {
  __shared__ float deq_tab[256];
  __shared__ float thr_tab[132];
  lion_load_tables(deq_tab, thr_tab, thr);
  for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += (long)gridDim.x * blockDim.x) {
    const float* xb = x + b * bs;
    float amax = 0.f;
    for (int j = 0; j < bs; ++j) amax = fmaxf(amax, fabsf(xb[j]));
    float inv = 1.0f / ((amax <= 0.f) ? 1.0f : amax);
    for (int j = 0; j < bs; ++j) codes[b * bs + j] = (int8_t)lion_quant_tab(xb[j] * inv, thr_tab);
    inv_scale[b] = inv;
  }
}

__global__ void __launch_bounds__(256) lion8_dequantize_kernel(const int8_t* __restrict__ codes,
                                                               const float* __restrict__ inv_scale,
                                                               float* __restrict__ x, long n, int bs) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = lion_deq((int)codes[i]) / inv_scale[i / bs];
}

// Per-step optimizer scalars (include/sdt.h sdt_opt_schedule_select): one lane reads the store's step counter t, copies entry
// min(t, n - 1) of each host-built table into the 16-byte block the scheduled sweeps read, and advances the counter.  Launched once
// per store and optimizer step, ahead of the sweeps on the same stream, so a replayed graph picks each step's values in turn.
__global__ void __launch_bounds__(64) opt_schedule_select_kernel(int64_t* __restrict__ step, const float* __restrict__ lr_tab, long n_lr,
                                                                  const float* __restrict__ ema_tab, long n_ema, float* __restrict__ cur) {
  if (threadIdx.x != 0) return;
  const int64_t t = *step;
  const long tc = t > 0 ? (long)t : 0;
  const long i = tc < n_lr - 1 ? tc : n_lr - 1;
  const long j = tc < n_ema - 1 ? tc : n_ema - 1;
  cur[0] = lr_tab[i];
  cur[1] = ema_tab[2 * j];
  cur[2] = ema_tab[2 * j + 1];
  cur[3] = 0.f;
  *step = t + 1;
}

// ---------------------------------------------------------------------------------------------------------------- AdamW
// Second optimizer (include/sdt.h "AdamW"): decoupled-decay Adam with bias correction, every operation a separately rounded float32
// one (division and square root correctly rounded).  The 8-bit sweep keeps the first moment m and the ROOT s = sqrt(v) of the second
// one in the block codec WITHOUT the reference's offset: code = sign(x) * c(|x|) with the same threshold table (a function of the
// magnitude alone), deq = (code / 127)^5, so zero <-> code 0 and a parameter whose gradient is exactly zero moves by decay alone.
__device__ __forceinline__ float adamw_deq(int code) {
  float t = (float)code / 127.0f;
  float t2 = t * t;
  float t4 = t2 * t2;
  return t4 * t;
}
__device__ __forceinline__ int adamw_quant_tab(float x, const float* __restrict__ thr) {  // as lion_quant_tab, a = |x|
  const float a = fabsf(x);
  const float q = __builtin_amdgcn_exp2f(0.2f * __builtin_amdgcn_logf(a)) * 127.0f;
  const float r = rintf(q);
  int c = (int)fminf(fmaxf(r, 0.f), 127.f);
  if (fabsf(q - r) > 0.5f - 2.5e-4f) c += (a >= thr[c + 1] ? 1 : 0) - (a < thr[c] ? 1 : 0);
  return x < 0.f ? -c : c;
}
__device__ __forceinline__ void adamw_load_tables(float* deq_tab, float* thr_tab, const float* __restrict__ thr) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) deq_tab[i] = adamw_deq(i - 128);
  for (int i = threadIdx.x; i < 129; i += blockDim.x) thr_tab[i] = i < 128 ? thr[i] : __builtin_inff();
  __syncthreads();
}

// Per-step scalars of an AdamW store (include/sdt.h sdt_adamw_select): one lane.  t = *step; the running products P1 = b1^(t+1),
// P2 = b2^(t+1) are carried in double by one multiplication per step (no pow: the host reproduces them with the same products);
// cur = {neg_lr, ema_r, ema_rm, 0, k1, k2, 0, 0} with k1 = 1 / (1 - P1), k2 = 1 / sqrt(1 - P2) formed in double and rounded once.
__global__ void __launch_bounds__(64) adamw_select_kernel(int64_t* __restrict__ step, double* __restrict__ prods,
                                                           const float* __restrict__ lr_tab, long n_lr, const float* __restrict__ ema_tab,
                                                           long n_ema, float neg_lr, float ema_r, float ema_rm, double b1, double b2,
                                                           float* __restrict__ cur) {
  if (threadIdx.x != 0) return;
  const int64_t t = *step;
  if (lr_tab) {
    const long tc = t > 0 ? (long)t : 0;
    const long i = tc < n_lr - 1 ? tc : n_lr - 1;
    const long j = tc < n_ema - 1 ? tc : n_ema - 1;
    neg_lr = lr_tab[i];
    ema_r = ema_tab[2 * j];
    ema_rm = ema_tab[2 * j + 1];
  }
  const double p1 = prods[0] * b1, p2 = prods[1] * b2;
  prods[0] = p1;
  prods[1] = p2;
  cur[0] = neg_lr;
  cur[1] = ema_r;
  cur[2] = ema_rm;
  cur[3] = 0.f;
  cur[4] = (float)(1.0 / (1.0 - p1));
  cur[5] = (float)(1.0 / sqrt(1.0 - p2));
  cur[6] = 0.f;
  cur[7] = 0.f;
  *step = t + 1;
}

// lion8_kernel's skeleton (LPB lanes per block, one contiguous window of LION_SLICES x 256 float4s per workgroup, non-temporal 16-byte
// traffic, tables in LDS, each inverse scale written once by its block's first lane) with two code streams and two scale streams.
template <int LPB, bool G16>
__global__ void __launch_bounds__(256) adamw8_kernel(float* __restrict__ p, const void* __restrict__ g, int8_t* __restrict__ m_codes,
                                                     float* __restrict__ m_inv, int8_t* __restrict__ s_codes, float* __restrict__ s_inv,
                                                     float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n4,
                                                     const double* __restrict__ sqnorm, const float* __restrict__ thr, float max_norm,
                                                     float wd, float c1, float c1m, float c2, float c2m, float eps,
                                                     const float* __restrict__ cur) {
  __shared__ float deq_tab[256];
  __shared__ float thr_tab[132];
  const float neg_lr = cur[0], ema_r = cur[1], ema_rm = cur[2], k1 = cur[4], k2 = cur[5];
  adamw_load_tables(deq_tab, thr_tab, thr);
  float gnorm = 0.f;
  bool do_clip = false;
  if (sqnorm) {
    gnorm = (float)sqrt(*sqnorm);
    do_clip = !(gnorm < max_norm);
  }
  typedef float f4v __attribute__((ext_vector_type(4)));
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const long i_end = min(n4, ((long)blockIdx.x + 1) * (LION_SLICES * 256));
  for (long i = (long)blockIdx.x * (LION_SLICES * 256) + threadIdx.x; i < i_end; i += 256) {
    f4v gv;
    if (G16) {
      const u2v h = __builtin_nontemporal_load(&reinterpret_cast<const u2v*>(g)[i]);
      gv.x = __uint_as_float(h.x << 16); gv.y = __uint_as_float(h.x & 0xffff0000u);
      gv.z = __uint_as_float(h.y << 16); gv.w = __uint_as_float(h.y & 0xffff0000u);
    } else {
      gv = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(g)[i]);
    }
    const f4v pv = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(p)[i]);
    const unsigned cwm = __builtin_nontemporal_load(&reinterpret_cast<const unsigned*>(m_codes)[i]);
    const unsigned cws = __builtin_nontemporal_load(&reinterpret_cast<const unsigned*>(s_codes)[i]);
    const long blk = i / LPB;
    const float minv = m_inv[blk], sinv = s_inv[blk];
    float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    float mn[4], sn[4];
    float mmax = 0.f, smax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cm = (int)(int8_t)((cwm >> (8 * j)) & 0xff);
      const int cs = (int)(int8_t)((cws >> (8 * j)) & 0xff);
      const float mf = deq_tab[cm + 128] / minv;
      const float sf = deq_tab[cs + 128] / sinv;
      const float vf = sf * sf;
      const float gc = clip_grad(gg[j], gnorm, max_norm, do_clip);
      mn[j] = c1 * mf + c1m * gc;
      const float vn = c2 * vf + c2m * (gc * gc);
      sn[j] = sqrtf(vn);
      mmax = fmaxf(mmax, fabsf(mn[j]));
      smax = fmaxf(smax, sn[j]);
      float u = (mn[j] * k1) / (sn[j] * k2 + eps);
      if (wd != 0.f) u = u + wd * pp[j];
      pp[j] = pp[j] + neg_lr * u;
    }
#pragma unroll
    for (int o = 1; o < LPB; o <<= 1) {
      mmax = fmaxf(mmax, __shfl_xor(mmax, o, 64));
      smax = fmaxf(smax, __shfl_xor(smax, o, 64));
    }
    const float nminv = 1.0f / ((mmax <= 0.f) ? 1.0f : mmax);
    const float nsinv = 1.0f / ((smax <= 0.f) ? 1.0f : smax);
    unsigned ncm = 0, ncs = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ncm |= ((unsigned)(adamw_quant_tab(mn[j] * nminv, thr_tab) & 0xff)) << (8 * j);
      ncs |= ((unsigned)(adamw_quant_tab(sn[j] * nsinv, thr_tab) & 0xff)) << (8 * j);
    }
    __builtin_nontemporal_store(ncm, &reinterpret_cast<unsigned*>(m_codes)[i]);
    __builtin_nontemporal_store(ncs, &reinterpret_cast<unsigned*>(s_codes)[i]);
    if ((i % LPB) == 0) {
      m_inv[blk] = nminv;
      s_inv[blk] = nsinv;
    }
    {
      const f4v o = {pp[0], pp[1], pp[2], pp[3]};
      __builtin_nontemporal_store(o, &reinterpret_cast<f4v*>(p)[i]);
    }
    if (ema) {
      f4v ev = __builtin_nontemporal_load(&reinterpret_cast<const f4v*>(ema)[i]);
      ev.x = ema_r * ev.x + ema_rm * pp[0];
      ev.y = ema_r * ev.y + ema_rm * pp[1];
      ev.z = ema_r * ev.z + ema_rm * pp[2];
      ev.w = ema_r * ev.w + ema_rm * pp[3];
      __builtin_nontemporal_store(ev, &reinterpret_cast<f4v*>(ema)[i]);
    }
    if (w_bf16) {
      const u2v o = {pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
      __builtin_nontemporal_store(o, &reinterpret_cast<u2v*>(w_bf16)[i]);
    }
  }
}

__global__ void __launch_bounds__(256) adamw32_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n,
                                                      const double* __restrict__ sqnorm, float max_norm, float wd, float c1, float c1m,
                                                      float c2, float c2m, float eps, const float* __restrict__ cur) {
  const float neg_lr = cur[0], ema_r = cur[1], ema_rm = cur[2], k1 = cur[4], k2 = cur[5];
  float gnorm = 0.f;
  bool do_clip = false;
  if (sqnorm) {
    gnorm = (float)sqrt(*sqnorm);
    do_clip = !(gnorm < max_norm);
  }
  const long i_end = min(n, ((long)blockIdx.x + 1) * 1024);  // a contiguous 1024-element slice per workgroup (see lion8_kernel)
  for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < i_end; i += 256) {
    const float gc = clip_grad(g[i], gnorm, max_norm, do_clip);
    float pv = p[i];
    const float mn = c1 * m[i] + c1m * gc;
    const float vn = c2 * v[i] + c2m * (gc * gc);
    m[i] = mn;
    v[i] = vn;
    float u = (mn * k1) / (sqrtf(vn) * k2 + eps);
    if (wd != 0.f) u = u + wd * pv;
    pv = pv + neg_lr * u;
    p[i] = pv;
    if (ema) ema[i] = ema_r * ema[i] + ema_rm * pv;
    if (w_bf16) w_bf16[i] = f2bf(pv);
  }
}

template <bool SCHED>
static void launch_lion8(int lpb, int g_bf16, dim3 grid, hipStream_t stream, float* p, const void* g, int8_t* codes, float* inv_scale,
                         float* ema, uint16_t* w_bf16, long n4, const double* sqnorm, const float* thresholds, float max_norm,
                         float neg_lr, float wd, float c1, float c1m, float c2, float c2m, float er, float erm, const float* cur) {
  const dim3 block(256);
#define LAUNCH_L8B(L, H)                                                                                                     \
  hipLaunchKernelGGL((lion8_kernel<L, H, SCHED>), grid, block, 0, stream, p, g, codes, inv_scale, ema, (bf16_t*)w_bf16, n4, \
                     sqnorm, thresholds, max_norm, neg_lr, wd, c1, c1m, c2, c2m, er, erm, cur)
#define LAUNCH_L8(L)      \
  do {                    \
    if (g_bf16)           \
      LAUNCH_L8B(L, true); \
    else                  \
      LAUNCH_L8B(L, false); \
  } while (0)
  switch (lpb) {
    case 1: LAUNCH_L8(1); break;
    case 2: LAUNCH_L8(2); break;
    case 4: LAUNCH_L8(4); break;
    case 8: LAUNCH_L8(8); break;
    case 16: LAUNCH_L8(16); break;
    case 32: LAUNCH_L8(32); break;
    default: LAUNCH_L8(64); break;
  }
#undef LAUNCH_L8
#undef LAUNCH_L8B
}

extern "C" {

#define SQNORM_MAX_BLOCKS 2048
int64_t sdt_sqnorm_workspace_bytes(void) { return SDT_WS_COUNTER_BYTES + SQNORM_MAX_BLOCKS * (int64_t)sizeof(double); }

/* *out_sq += sum g^2 (double).  workspace: sdt_sqnorm_workspace_bytes() bytes under the split-workspace contract (first 64 KiB
 * zero when enqueued, zero again afterwards; include/sdt.h). */
int sdt_sqnorm_accumulate(const float* g, int64_t n, double* out_sq, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(g && out_sq && n >= 0, "sdt_sqnorm_accumulate: null pointer or negative n");
  SDT_CHECK_ARG(((uintptr_t)g & 15) == 0, "sdt_sqnorm_accumulate: g must be 16-byte aligned");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_sqnorm_workspace_bytes(),
                "sdt_sqnorm_accumulate: workspace of sdt_sqnorm_workspace_bytes() needed");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(sqnorm_kernel<false>, dim3(sdt_grid_1d(n >> 2, 256 * 8, SQNORM_MAX_BLOCKS)), dim3(256), 0, stream, (const void*)g, (long)n, out_sq,
                     reinterpret_cast<int*>(workspace), reinterpret_cast<double*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_sqnorm_accumulate");
  return SDT_OK;
}

int sdt_sqnorm_accumulate_bf16(const uint16_t* g, int64_t n, double* out_sq, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(g && out_sq && n >= 0, "sdt_sqnorm_accumulate_bf16: null pointer or negative n");
  SDT_CHECK_ARG(((uintptr_t)g & 7) == 0, "sdt_sqnorm_accumulate_bf16: g must be 8-byte aligned");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_sqnorm_workspace_bytes(),
                "sdt_sqnorm_accumulate_bf16: workspace of sdt_sqnorm_workspace_bytes() needed");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(sqnorm_kernel<true>, dim3(sdt_grid_1d(n >> 2, 256 * 8, SQNORM_MAX_BLOCKS)), dim3(256), 0, stream, (const void*)g, (long)n, out_sq,
                     reinterpret_cast<int*>(workspace), reinterpret_cast<double*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_sqnorm_accumulate_bf16");
  return SDT_OK;
}

int sdt_grad_accumulate(float* acc, const void* g, int g_bf16, int64_t n, int mode, float scale, double* out_sq, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(mode >= SDT_ACC_INIT && mode <= SDT_ACC_SCALE, "sdt_grad_accumulate: unknown mode %d", mode);
  SDT_CHECK_ARG(acc && (g || mode == SDT_ACC_SCALE) && n >= 0, "sdt_grad_accumulate: null pointer or negative n");
  SDT_CHECK_ARG(((uintptr_t)acc & 15) == 0, "sdt_grad_accumulate: acc must be 16-byte aligned");
  SDT_CHECK_ARG(mode == SDT_ACC_SCALE || ((uintptr_t)g & (g_bf16 ? 7 : 15)) == 0,
                "sdt_grad_accumulate: g must be %d-byte aligned", g_bf16 ? 8 : 16);
  SDT_CHECK_ARG(!out_sq || (workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_sqnorm_workspace_bytes()),
                "sdt_grad_accumulate: workspace of sdt_sqnorm_workspace_bytes() needed with out_sq");
  if (n == 0) return SDT_OK;
  const dim3 grid(sdt_grid_1d(n >> 2, 256 * 8, SQNORM_MAX_BLOCKS)), block(256);  // sqnorm_kernel's grid: the same partition of the norm
  int* counter = reinterpret_cast<int*>(workspace);
  double* part = workspace ? reinterpret_cast<double*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES) : nullptr;
#define LAUNCH_ACC(G, M, N) \
  hipLaunchKernelGGL((grad_accumulate_kernel<G, M, N>), grid, block, 0, stream, acc, g, (long)n, scale, out_sq, counter, part)
#define LAUNCH_ACC_N(G, M)   \
  do {                       \
    if (out_sq)              \
      LAUNCH_ACC(G, M, true); \
    else                     \
      LAUNCH_ACC(G, M, false); \
  } while (0)
#define LAUNCH_ACC_M(G)                                       \
  do {                                                        \
    switch (mode) {                                           \
      case SDT_ACC_INIT: LAUNCH_ACC_N(G, SDT_ACC_INIT); break;     \
      case SDT_ACC_ADD: LAUNCH_ACC_N(G, SDT_ACC_ADD); break;       \
      case SDT_ACC_FINISH: LAUNCH_ACC_N(G, SDT_ACC_FINISH); break; \
      default: LAUNCH_ACC_N(G, SDT_ACC_SCALE); break;              \
    }                                                         \
  } while (0)
  if (g_bf16 && mode != SDT_ACC_SCALE)
    LAUNCH_ACC_M(true);
  else
    LAUNCH_ACC_M(false);
#undef LAUNCH_ACC_M
#undef LAUNCH_ACC_N
#undef LAUNCH_ACC
  SDT_LAUNCH_CHECK("sdt_grad_accumulate");
  return SDT_OK;
}

int sdt_sum_f64_accumulate(const double* x, int64_t n, double* out, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(x && out && n >= 0, "sdt_sum_f64_accumulate: null pointer or negative n");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_sqnorm_workspace_bytes(),
                "sdt_sum_f64_accumulate: workspace of sdt_sqnorm_workspace_bytes() needed");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(sum_f64_kernel, dim3(sdt_grid_1d(n, 256 * 16, SQNORM_MAX_BLOCKS)), dim3(256), 0, stream, x, (long)n, out,
                     reinterpret_cast<int*>(workspace), reinterpret_cast<double*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_sum_f64_accumulate");
  return SDT_OK;
}

#define LION8_CHECK_ARGS(NAME)                                                                                                   \
  SDT_CHECK_ARG(p && g && codes && inv_scale && thresholds, NAME ": null pointer");                                              \
  SDT_CHECK_ARG(n >= 0 && block_size >= 4 && block_size <= 256 && (block_size & (block_size - 1)) == 0,                         \
                NAME ": block_size must be a power of two in [4,256] (got %d)", block_size);                                     \
  SDT_CHECK_ARG(n % block_size == 0, NAME ": n=%ld not a multiple of block_size=%d (lion_quant.py:70 reshape)", (long)n, block_size); \
  SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)g & (g_bf16 ? 7 : 15)) == 0 && ((uintptr_t)codes & 3) == 0 && \
                    ((uintptr_t)w_bf16 & 7) == 0,                                                                                \
                NAME ": misaligned buffer")

int sdt_lion8_step(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16, int64_t n,
                   int block_size, const double* sqnorm, const float* thresholds, double max_norm, double lr, double wd,
                   double b1, double b2, double ema_rate, hipStream_t stream) {
  LION8_CHECK_ARGS("sdt_lion8_step");
  if (n == 0) return SDT_OK;
  const long n4 = n >> 2;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  const float er = (float)ema_rate, erm = (float)(1.0 - ema_rate);
  launch_lion8<false>(block_size >> 2, g_bf16, dim3(sdt_grid_1d(n4, 256 * LION_SLICES, 1 << 30)), stream, p, g, codes, inv_scale, ema,
                      w_bf16, n4, sqnorm, thresholds, (float)max_norm, (float)(-lr), (float)wd, c1, c1m, c2, c2m, er, erm, nullptr);
  SDT_LAUNCH_CHECK("sdt_lion8_step");
  return SDT_OK;
}

int sdt_lion8_step_scheduled(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16,
                             int64_t n, int block_size, const double* sqnorm, const float* thresholds, double max_norm, const float* cur,
                             double wd, double b1, double b2, hipStream_t stream) {
  LION8_CHECK_ARGS("sdt_lion8_step_scheduled");
  SDT_CHECK_ARG(cur && ((uintptr_t)cur & 15) == 0, "sdt_lion8_step_scheduled: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  const long n4 = n >> 2;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  launch_lion8<true>(block_size >> 2, g_bf16, dim3(sdt_grid_1d(n4, 256 * LION_SLICES, 1 << 30)), stream, p, g, codes, inv_scale, ema,
                     w_bf16, n4, sqnorm, thresholds, (float)max_norm, 0.f, (float)wd, c1, c1m, c2, c2m, 0.f, 0.f, cur);
  SDT_LAUNCH_CHECK("sdt_lion8_step_scheduled");
  return SDT_OK;
}
#undef LION8_CHECK_ARGS

int sdt_lion32_step(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n,
                    const double* sqnorm, double max_norm, double lr, double wd, double b1, double b2, double ema_rate,
                    hipStream_t stream) {
  SDT_CHECK_ARG(p && g && mom && n >= 0, "sdt_lion32_step: null pointer or negative n");
  if (n == 0) return SDT_OK;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  const float er = (float)ema_rate, erm = (float)(1.0 - ema_rate);
  hipLaunchKernelGGL(lion32_kernel<false>, dim3(sdt_grid_1d(n, 1024, 1 << 30)), dim3(256), 0, stream, p, g, mom, ema,
                     (bf16_t*)w_bf16, (long)n, sqnorm, (float)max_norm, (float)(-lr), (float)wd, c1, c1m, c2, c2m, er, erm,
                     (const float*)nullptr);
  SDT_LAUNCH_CHECK("sdt_lion32_step");
  return SDT_OK;
}

int sdt_lion32_step_scheduled(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                              double max_norm, const float* cur, double wd, double b1, double b2, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && mom && n >= 0, "sdt_lion32_step_scheduled: null pointer or negative n");
  SDT_CHECK_ARG(cur && ((uintptr_t)cur & 15) == 0, "sdt_lion32_step_scheduled: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  hipLaunchKernelGGL(lion32_kernel<true>, dim3(sdt_grid_1d(n, 1024, 1 << 30)), dim3(256), 0, stream, p, g, mom, ema,
                     (bf16_t*)w_bf16, (long)n, sqnorm, (float)max_norm, 0.f, (float)wd, c1, c1m, c2, c2m, 0.f, 0.f, cur);
  SDT_LAUNCH_CHECK("sdt_lion32_step_scheduled");
  return SDT_OK;
}

int sdt_opt_schedule_select(int64_t* step, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, float* cur,
                            hipStream_t stream) {
  SDT_CHECK_ARG(step && lr_tab && ema_tab && cur, "sdt_opt_schedule_select: null pointer");
  SDT_CHECK_ARG(n_lr >= 1 && n_ema >= 1, "sdt_opt_schedule_select: every table needs at least one entry (n_lr=%ld, n_ema=%ld)",
                (long)n_lr, (long)n_ema);
  SDT_CHECK_ARG(((uintptr_t)step & 7) == 0 && ((uintptr_t)cur & 15) == 0 && ((uintptr_t)ema_tab & 7) == 0,
                "sdt_opt_schedule_select: misaligned step counter, table or block");
  hipLaunchKernelGGL(opt_schedule_select_kernel, dim3(1), dim3(64), 0, stream, step, lr_tab, (long)n_lr, ema_tab, (long)n_ema, cur);
  SDT_LAUNCH_CHECK("sdt_opt_schedule_select");
  return SDT_OK;
}

int sdt_adamw_select(int64_t* step, double* prods, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, double lr,
                     double ema_rate, double b1, double b2, float* cur, hipStream_t stream) {
  SDT_CHECK_ARG(step && prods && cur, "sdt_adamw_select: null pointer");
  SDT_CHECK_ARG((lr_tab != nullptr) == (ema_tab != nullptr), "sdt_adamw_select: lr_tab and ema_tab come together or not at all");
  SDT_CHECK_ARG(!lr_tab || (n_lr >= 1 && n_ema >= 1), "sdt_adamw_select: every table needs at least one entry (n_lr=%ld, n_ema=%ld)",
                (long)n_lr, (long)n_ema);
  SDT_CHECK_ARG(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "sdt_adamw_select: b1 and b2 must lie in [0, 1) (got %g, %g)", b1, b2);
  SDT_CHECK_ARG((((uintptr_t)step | (uintptr_t)prods | (uintptr_t)ema_tab) & 7) == 0 && ((uintptr_t)cur & 15) == 0,
                "sdt_adamw_select: misaligned step counter, products, table or block");
  hipLaunchKernelGGL(adamw_select_kernel, dim3(1), dim3(64), 0, stream, step, prods, lr_tab, (long)n_lr, ema_tab, (long)n_ema,
                     (float)(-lr), (float)ema_rate, (float)(1.0 - ema_rate), b1, b2, cur);
  SDT_LAUNCH_CHECK("sdt_adamw_select");
  return SDT_OK;
}

int sdt_adamw8_step(float* p, const void* g, int g_bf16, int8_t* m_codes, float* m_inv_scale, int8_t* s_codes, float* s_inv_scale,
                    float* ema, uint16_t* w_bf16, int64_t n, int block_size, const double* sqnorm, const float* thresholds,
                    double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && m_codes && m_inv_scale && s_codes && s_inv_scale && thresholds && cur, "sdt_adamw8_step: null pointer");
  SDT_CHECK_ARG(n >= 0 && block_size >= 4 && block_size <= 256 && (block_size & (block_size - 1)) == 0,
                "sdt_adamw8_step: block_size must be a power of two in [4,256] (got %d)", block_size);
  SDT_CHECK_ARG(n % block_size == 0, "sdt_adamw8_step: n=%ld not a multiple of block_size=%d", (long)n, block_size);
  SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)ema | (uintptr_t)cur) & 15) == 0 && ((uintptr_t)g & (g_bf16 ? 7 : 15)) == 0 &&
                    (((uintptr_t)m_codes | (uintptr_t)s_codes) & 3) == 0 && ((uintptr_t)w_bf16 & 7) == 0,
                "sdt_adamw8_step: misaligned buffer");
  if (n == 0) return SDT_OK;
  const long n4 = n >> 2;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  const dim3 grid(sdt_grid_1d(n4, 256 * LION_SLICES, 1 << 30)), block(256);
#define LAUNCH_A8B(L, H)                                                                                                          \
  hipLaunchKernelGGL((adamw8_kernel<L, H>), grid, block, 0, stream, p, g, m_codes, m_inv_scale, s_codes, s_inv_scale, ema,       \
                     (bf16_t*)w_bf16, n4, sqnorm, thresholds, (float)max_norm, (float)wd, c1, c1m, c2, c2m, (float)eps, cur)
#define LAUNCH_A8(L)       \
  do {                     \
    if (g_bf16)            \
      LAUNCH_A8B(L, true);  \
    else                   \
      LAUNCH_A8B(L, false); \
  } while (0)
  switch (block_size >> 2) {
    case 1: LAUNCH_A8(1); break;
    case 2: LAUNCH_A8(2); break;
    case 4: LAUNCH_A8(4); break;
    case 8: LAUNCH_A8(8); break;
    case 16: LAUNCH_A8(16); break;
    case 32: LAUNCH_A8(32); break;
    default: LAUNCH_A8(64); break;
  }
#undef LAUNCH_A8
#undef LAUNCH_A8B
  SDT_LAUNCH_CHECK("sdt_adamw8_step");
  return SDT_OK;
}

int sdt_adamw32_step(float* p, const float* g, float* m, float* v, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                     double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && m && v && cur && n >= 0, "sdt_adamw32_step: null pointer or negative n");
  SDT_CHECK_ARG(((uintptr_t)cur & 15) == 0, "sdt_adamw32_step: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  const float c1 = (float)b1, c1m = (float)(1.0 - b1), c2 = (float)b2, c2m = (float)(1.0 - b2);
  hipLaunchKernelGGL(adamw32_kernel, dim3(sdt_grid_1d(n, 1024, 1 << 30)), dim3(256), 0, stream, p, g, m, v, ema, (bf16_t*)w_bf16, (long)n,
                     sqnorm, (float)max_norm, (float)wd, c1, c1m, c2, c2m, (float)eps, cur);
  SDT_LAUNCH_CHECK("sdt_adamw32_step");
  return SDT_OK;
}

int sdt_lion8_quantize(const float* x, int8_t* codes, float* inv_scale, int64_t n, int block_size,
                       const float* thresholds, hipStream_t stream) {
  SDT_CHECK_ARG(x && codes && inv_scale && thresholds && block_size > 0 && n % block_size == 0, "sdt_lion8_quantize: bad args");
  if (n == 0) return SDT_OK;
  long nb = n / block_size;
  hipLaunchKernelGGL(lion8_quantize_kernel, dim3(sdt_grid_1d(nb, 256, 4096)), dim3(256), 0, stream, x, codes,
                     inv_scale, nb, block_size, thresholds);
  SDT_LAUNCH_CHECK("sdt_lion8_quantize");
  return SDT_OK;
}

int sdt_lion8_dequantize(const int8_t* codes, const float* inv_scale, float* x, int64_t n, int block_size,
                         hipStream_t stream) {
  SDT_CHECK_ARG(x && codes && inv_scale && block_size > 0 && n % block_size == 0, "sdt_lion8_dequantize: bad args");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(lion8_dequantize_kernel, dim3(sdt_grid_1d(n, 256, 4096)), dim3(256), 0, stream, codes, inv_scale,
                     x, (long)n, block_size);
  SDT_LAUNCH_CHECK("sdt_lion8_dequantize");
  return SDT_OK;
}

}  // extern "C"
