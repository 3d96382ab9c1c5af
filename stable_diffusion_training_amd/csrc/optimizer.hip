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
#include <cmath>
#include <type_traits>

#include "sdt_common.h"

#define LION_OFFSET 3.7398995e-09f  // lion_quant.py:49

// The 8-bit block codec.  OFFSET: the reference's form (Lion's momentum), which shifts every value by LION_OFFSET.  Without it
// (AdamW's moments) code = sign(x) * c(|x|) with the same threshold table (a function of the magnitude alone) and
// deq = (code / 127)^5, so zero <-> code 0 and a parameter whose gradient is exactly zero moves by decay alone.
template <bool OFFSET>
__device__ __forceinline__ float codec_deq(int code) {  // lion_quant.py:61-64
  float t = (float)code / 127.0f;
  float t2 = t * t;
  float t4 = t2 * t2;
  return OFFSET ? t4 * t - LION_OFFSET : t4 * t;
}
// _quantize (lion_quant.py:52-59): code = rint(sign(x + offset) * |x + offset|^(1/5) * 127).
// The same integer without powf: _quantize is a monotone step function of a = |x + offset|, described exactly by the 127
// float32 thresholds thr[c] = smallest a whose code is >= c (thr[0] = 0, thr[128] = +inf; built on the host with the float32
// power / multiply / rint of the definition, lion_codec.quantization_thresholds).  v_log_f32 / v_exp_f32 give the code to
// well within one unit; two threshold reads settle it: thr[c] <= a < thr[c + 1].  Bit-exact against the host definition at
// every rounding boundary, and no device/host pow ulp disagreement (the HBM-bound sweep was VALU-bound on powf).
template <bool OFFSET>
__device__ __forceinline__ int codec_quant(float x, const float* __restrict__ thr) {
  const float xo = OFFSET ? x + LION_OFFSET : x;
  const float a = fabsf(xo);
  const float q = __builtin_amdgcn_exp2f(0.2f * __builtin_amdgcn_logf(a)) * 127.0f;
  const float r = rintf(q);
  int c = (int)fminf(fmaxf(r, 0.f), 127.f);
  // the estimate is good to ~2e-5 code units (1-ulp v_log / v_exp): only values within 2.5e-4 of a rounding boundary can
  // land on the wrong side and need the table (about one element in 2000; the others skip the two LDS reads)
  if (fabsf(q - r) > 0.5f - 2.5e-4f) c += (a >= thr[c + 1] ? 1 : 0) - (a < thr[c] ? 1 : 0);
  return xo < 0.f ? -c : c;
}
template <bool OFFSET>
__device__ __forceinline__ void codec_load_tables(float* deq_tab, float* thr_tab, const float* __restrict__ thr) {
  // exact codec_deq() of every int8 code (the /127 and the 5th power done once) and the codec thresholds, in LDS
  for (int i = threadIdx.x; i < 256; i += blockDim.x) deq_tab[i] = codec_deq<OFFSET>(i - 128);
  for (int i = threadIdx.x; i < 129; i += blockDim.x) thr_tab[i] = i < 128 ? thr[i] : __builtin_inff();
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------- ordered sums in double
// One float4 of the norm walk: d0 takes x and z, d1 takes y and w.  Every kernel that feeds a squared norm walks its buffer with
// this, so two of them over the same values and grid produce the same bits.
__device__ __forceinline__ void sq_accumulate(const f32x4_t v, double& d0, double& d1) {
  d0 = fma((double)v.x, (double)v.x, d0);
  d1 = fma((double)v.y, (double)v.y, d1);
  d0 = fma((double)v.z, (double)v.z, d0);
  d1 = fma((double)v.w, (double)v.w, d1);
}

// *out += the sum of every thread's dacc over the whole grid (256 threads per workgroup), in a fixed order.  Workgroups store
// their double partial sums to `part`; the one that arrives last adds them in workgroup order into *out (no float / double atomics:
// the result is bitwise reproducible).  PAIRWISE: the workgroup's partial is the tree over its four waves instead of their
// sequential sum - the association each caller has always had.  Returns in every workgroup but the last early: call it last.
// K sums at once (ordered_sums_f64): one arrival for all of them, `part` holds K runs of `part_stride` doubles and `out` K consecutive
// doubles; each sum is formed exactly as a single one is.
template <bool PAIRWISE, int K>
__device__ __forceinline__ void ordered_sums_f64(double (&dacc)[K], double* __restrict__ out, int* counter, double* __restrict__ part,
                                                 int part_stride) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) dacc[k] += __shfl_xor(dacc[k], o, 64);
  __shared__ double dsc[K][16];
  __shared__ int s_last;
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) dsc[k][w] = dacc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double t = 0.0;
      if (PAIRWISE) t = (dsc[k][0] + dsc[k][1]) + (dsc[k][2] + dsc[k][3]);
      else for (int i = 0; i < nw; ++i) t += dsc[k][i];
      sdt_store_wt(part + (long)k * part_stride + blockIdx.x, t);
    }
  }
  if (!sdt_arrive_last<true>(counter, (int)gridDim.x, &s_last)) return;
  // last arriver: 256 threads x strided partials, then a fixed tree
  double t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    t[k] = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t[k] += sdt_load_wt(part + (long)k * part_stride + i);
    for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) dsc[k][w] = t[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] += (dsc[k][0] + dsc[k][1]) + (dsc[k][2] + dsc[k][3]);
  }
}
template <bool PAIRWISE>
__device__ __forceinline__ void ordered_sum_f64(double dacc, double* __restrict__ out, int* counter, double* __restrict__ part) {
  double a[1] = {dacc};
  ordered_sums_f64<PAIRWISE, 1>(a, out, counter, part, 0);
}

// Sum of squares in double: every product of two floats is exact in double and the running sum carries ~1e-16 relative
// error, so the float32 norm the optimizer kernels derive from it is the float32 rounding of the true norm - the value
// optax.global_norm rounds to - and the clipped gradients (g / norm) match the host definition bit for bit.  The pass is
// HBM-bound (4 B per parameter); four double FMAs per 16 bytes are far below the fp64 vector rate.
// G16: the buffer holds bf16 values (the kernel leaves' gradients [r4]): four per 8 bytes, widened exactly.
template <bool G16>
__global__ void __launch_bounds__(256) sqnorm_kernel(const void* __restrict__ gv, long n, double* __restrict__ out, int* counter,
                                                     double* __restrict__ part) {
  const long nv = n >> 2;
  double d0 = 0.0, d1 = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    f32x4_t v;
    if (G16) {
      const uint2 h = reinterpret_cast<const uint2*>(gv)[i];
      v = unpack4(h.x, h.y);
    } else {
      v = reinterpret_cast<const f32x4_t*>(gv)[i];
    }
    sq_accumulate(v, d0, d1);
  }
  double dacc = d0 + d1;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = G16 ? bf2f(reinterpret_cast<const bf16_t*>(gv)[(nv << 2) + threadIdx.x]) : reinterpret_cast<const float*>(gv)[(nv << 2) + threadIdx.x];
    dacc += (double)v * (double)v;
  }
  ordered_sum_f64<false>(dacc, out, counter, part);
}

// Micro-batch gradient accumulation (include/sdt.h sdt_grad_accumulate): acc (fp32) <- init / add / finish / scale of the step's
// gradient g (bf16 or fp32, widened exactly), element-wise, in one HBM-bound sweep: init 6 B (bf16 g) per element, add and finish
// 10 B, scale 8 B.  With NORM the sweep also adds sum acc_final^2 to *out exactly as sqnorm_kernel does over the finished buffer -
// same grid (the caller passes sqnorm_kernel's), same sq_accumulate walk, same ordered_sum_f64 - so the squared norm is
// bit-identical to sdt_sqnorm_accumulate run over acc afterwards.
template <bool G16, int MODE, bool NORM>
__global__ void __launch_bounds__(256) grad_accumulate_kernel(float* __restrict__ acc, const void* __restrict__ gv, long n, float scale,
                                                              double* __restrict__ out, int* counter, double* __restrict__ part) {
  const long nv = n >> 2;
  double d0 = 0.0, d1 = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (MODE != SDT_ACC_SCALE) {
      if (G16) {
        const uint2 h = reinterpret_cast<const uint2*>(gv)[i];
        v = unpack4(h.x, h.y);
      } else {
        v = reinterpret_cast<const f32x4_t*>(gv)[i];
      }
    }
    if (MODE != SDT_ACC_INIT) {
      const f32x4_t a = reinterpret_cast<const f32x4_t*>(acc)[i];
      if (MODE == SDT_ACC_SCALE) {
        v = a * scale;
      } else {
        v = a + v;
        if (MODE == SDT_ACC_FINISH) v = v * scale;
      }
    }
    reinterpret_cast<f32x4_t*>(acc)[i] = v;
    if (NORM) sq_accumulate(v, d0, d1);
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
  if (NORM) ordered_sum_f64<false>(dacc, out, counter, part);
}

// *out += sum of n doubles, added in a fixed order (contiguous chunk per workgroup, strided over the threads, then ordered_sum_f64):
// the squared-norm partials the weight-gradient kernels wrote to their slots (include/sdt.h sdt_gemm_tn_wgrad sq_slots).
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
  ordered_sum_f64<true>(d0 + d1, out, counter, part);
}

// ------------------------------------------------------------------------------------------------------- the sweeps
// clip factor semantics of optax.clip_by_global_norm: g if norm < max else (g / norm) * max
struct Clip {
  float gnorm, max_norm;
  bool on;
  __device__ __forceinline__ float operator()(float g) const { return on ? (g / gnorm) * max_norm : g; }
};
__device__ __forceinline__ Clip clip_prologue(const double* __restrict__ sqnorm, float max_norm) {  // sqnorm null: no clipping
  Clip c = {0.f, max_norm, false};
  if (sqnorm) {
    c.gnorm = (float)sqrt(*sqnorm);
    c.on = !(c.gnorm < max_norm);
  }
  return c;
}

// Update rules.  step() takes the clipped gradient gc and the NS decoded state values, writes the new state values and returns the
// update direction u; the sweeps around it apply p <- p + neg_lr * (u + wd * p).  Every operation rounds separately, in this order.
struct LionRule {  // lion_quant.py:133-154; one state stream, the momentum, coded with the reference's offset
  static constexpr int NS = 1;
  static constexpr bool OFFSET = true;
  float c1, c1m, c2, c2m;
  __device__ __forceinline__ float step(float gc, const float* st, float* ns) const {
    const float cc = c1m * gc + c1 * st[0];  // lion_quant.py:141-143
    ns[0] = c2m * gc + c2 * st[0];           // lion_quant.py:105-107
    return (cc > 0.f) ? 1.f : ((cc < 0.f) ? -1.f : 0.f);
  }
};
// Second optimizer (include/sdt.h "AdamW"): decoupled-decay Adam with bias correction (division and square root correctly rounded).
// Two state streams, m and the second moment.  ROOT: the second stream holds s = sqrt(v) (the 8-bit sweep, whose codec resolves the
// root far better than v itself); without it the stream holds v (the fp32 sweep).  k1 = 1 / (1 - b1^t), k2 = 1 / sqrt(1 - b2^t).
template <bool ROOT>
struct AdamwRule {
  static constexpr int NS = 2;
  static constexpr bool OFFSET = false;
  float c1, c1m, c2, c2m, eps, k1, k2;
  __device__ __forceinline__ float step(float gc, const float* st, float* ns) const {
    ns[0] = c1 * st[0] + c1m * gc;
    const float vn = c2 * (ROOT ? st[1] * st[1] : st[1]) + c2m * (gc * gc);
    const float sn = sqrtf(vn);
    ns[1] = ROOT ? sn : vn;
    return (ns[0] * k1) / (sn * k2 + eps);
  }
};

__device__ __forceinline__ float decay_apply(float p, float u, float wd, float neg_lr) {
  if (wd != 0.f) u = u + wd * p;  // add_decayed_weights
  return p + neg_lr * u;          // _scale_by_learning_rate, apply_updates
}
// Scheduled sweeps: neg_lr, ema_r and ema_rm come from the device block `cur` that a select kernel wrote for this step; with
// cur == nullptr the by-value arguments stand.
__device__ __forceinline__ void scheduled_scalars(const float* __restrict__ cur, float& neg_lr, float& ema_r, float& ema_rm) {
  if (cur) {
    neg_lr = cur[0];
    ema_r = cur[1];
    ema_rm = cur[2];
  }
}

// The 8-bit sweep.  LPB lanes cooperate on one quantisation block of BS = 4*LPB elements; each lane owns a float4.  Rule::NS code
// streams and as many scale streams; each inverse scale is written once by its block's first lane.
#define LION_SLICES 4
template <class Rule, int LPB, bool G16>
__device__ __forceinline__ void sweep8_body(const Rule rule, float* p, const void* g, int8_t* const (&codes)[Rule::NS],
                                            float* const (&inv_scale)[Rule::NS], float* ema, bf16_t* w_bf16, long n4,
                                            const double* sqnorm, const float* thr, float max_norm, float neg_lr, float wd, float ema_r,
                                            float ema_rm) {
  constexpr int NS = Rule::NS;
  __shared__ float deq_tab[256];
  __shared__ float thr_tab[132];
  codec_load_tables<Rule::OFFSET>(deq_tab, thr_tab, thr);
  const Clip clip = clip_prologue(sqnorm, max_norm);
  // n4 is a multiple of LPB and consecutive lanes hold consecutive float4s, so the LPB lanes of a block stay together.
  // A workgroup sweeps LION_SLICES consecutive slices of 256 float4s and the grid covers the buffer once: the resident
  // workgroups then work on ONE contiguous window of each of the streams (a capped grid striding over the whole buffers
  // ran the sweep at 4.1 instead of 5.9 TB/s), and every byte is touched once per step, so all of it moves non-temporally.
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const long i_end = min(n4, ((long)blockIdx.x + 1) * (LION_SLICES * 256));
  for (long i = (long)blockIdx.x * (LION_SLICES * 256) + threadIdx.x; i < i_end; i += 256) {
    f32x4_t gv;
    if (G16) {  // bf16 gradient (8 bytes per float4 of parameters), widened exactly: what optax sees of a bf16 cotangent
      const u2v h = __builtin_nontemporal_load(&reinterpret_cast<const u2v*>(g)[i]);
      gv = unpack4(h.x, h.y);
    } else {
      gv = __builtin_nontemporal_load(&reinterpret_cast<const f32x4_t*>(g)[i]);
    }
    f32x4_t pv = __builtin_nontemporal_load(&reinterpret_cast<const f32x4_t*>(p)[i]);
    const long blk = i / LPB;
    unsigned cw[NS], ncw[NS];
    float inv[NS], ninv[NS], amax[NS], sn[NS][4];
#pragma unroll
    for (int k = 0; k < NS; ++k) cw[k] = __builtin_nontemporal_load(&reinterpret_cast<const unsigned*>(codes[k])[i]);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      inv[k] = inv_scale[k][blk];
      amax[k] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float st[NS], ns[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) st[k] = deq_tab[(int)(int8_t)((cw[k] >> (8 * j)) & 0xff) + 128] / inv[k];  // lion_quant.py:88-91
      const float u = rule.step(clip(gv[j]), st, ns);
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        sn[k][j] = ns[k];
        amax[k] = fmaxf(amax[k], fabsf(ns[k]));
      }
      pv[j] = decay_apply(pv[j], u, wd, neg_lr);
    }
#pragma unroll
    for (int o = 1; o < LPB; o <<= 1) {
#pragma unroll
      for (int k = 0; k < NS; ++k) amax[k] = fmaxf(amax[k], __shfl_xor(amax[k], o, 64));
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      ninv[k] = 1.0f / ((amax[k] <= 0.f) ? 1.0f : amax[k]);  // lion_quant.py:72-76
      ncw[k] = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) ncw[k] |= ((unsigned)(codec_quant<Rule::OFFSET>(sn[k][j] * ninv[k], thr_tab) & 0xff)) << (8 * j);
    }
    // stores apart from the quantisation: a store the compiler sinks into the codec's branches comes out without its non-temporal hint
#pragma unroll
    for (int k = 0; k < NS; ++k) __builtin_nontemporal_store(ncw[k], &reinterpret_cast<unsigned*>(codes[k])[i]);
    if ((i % LPB) == 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) inv_scale[k][blk] = ninv[k];
    }
    __builtin_nontemporal_store(pv, &reinterpret_cast<f32x4_t*>(p)[i]);
    if (ema) {
      const f32x4_t ev = __builtin_nontemporal_load(&reinterpret_cast<const f32x4_t*>(ema)[i]);
      __builtin_nontemporal_store(ema_r * ev + ema_rm * pv, &reinterpret_cast<f32x4_t*>(ema)[i]);
    }
    if (w_bf16) {
      const u2v o = {pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w)};
      __builtin_nontemporal_store(o, &reinterpret_cast<u2v*>(w_bf16)[i]);
    }
  }
}

// The fp32-state sweep: a contiguous 1024-element slice per workgroup (see sweep8_body), Rule::NS state buffers.
template <class Rule>
__device__ __forceinline__ void sweep32_body(const Rule rule, float* p, const float* g, float* const (&state)[Rule::NS], float* ema,
                                             bf16_t* w_bf16, long n, const double* sqnorm, float max_norm, float neg_lr, float wd,
                                             float ema_r, float ema_rm) {
  constexpr int NS = Rule::NS;
  const Clip clip = clip_prologue(sqnorm, max_norm);
  const long i_end = min(n, ((long)blockIdx.x + 1) * 1024);
  for (long i = (long)blockIdx.x * 1024 + threadIdx.x; i < i_end; i += 256) {
    float st[NS], ns[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) st[k] = state[k][i];
    const float u = rule.step(clip(g[i]), st, ns);
#pragma unroll
    for (int k = 0; k < NS; ++k) state[k][i] = ns[k];
    const float pv = decay_apply(p[i], u, wd, neg_lr);
    p[i] = pv;
    if (ema) ema[i] = ema_r * ema[i] + ema_rm * pv;
    if (w_bf16) w_bf16[i] = f2bf(pv);
  }
}

template <int LPB, bool G16>
__global__ void __launch_bounds__(256) lion8_kernel(float* __restrict__ p, const void* __restrict__ g,
                                                    int8_t* __restrict__ codes, float* __restrict__ inv_scale,
                                                    float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n4,
                                                    const double* __restrict__ sqnorm, const float* __restrict__ thr,
                                                    float max_norm, float neg_lr, float wd, float c1, float c1m, float c2,
                                                    float c2m, float ema_r, float ema_rm, const float* __restrict__ cur) {
  scheduled_scalars(cur, neg_lr, ema_r, ema_rm);
  int8_t* const cs[1] = {codes};
  float* const is[1] = {inv_scale};
  sweep8_body<LionRule, LPB, G16>(LionRule{c1, c1m, c2, c2m}, p, g, cs, is, ema, w_bf16, n4, sqnorm, thr, max_norm, neg_lr, wd, ema_r,
                                  ema_rm);
}

__global__ void __launch_bounds__(256) lion32_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ mom, float* __restrict__ ema,
                                                     bf16_t* __restrict__ w_bf16, long n,
                                                     const double* __restrict__ sqnorm, float max_norm, float neg_lr,
                                                     float wd, float c1, float c1m, float c2, float c2m, float ema_r,
                                                     float ema_rm, const float* __restrict__ cur) {
  scheduled_scalars(cur, neg_lr, ema_r, ema_rm);
  float* const st[1] = {mom};
  sweep32_body(LionRule{c1, c1m, c2, c2m}, p, g, st, ema, w_bf16, n, sqnorm, max_norm, neg_lr, wd, ema_r, ema_rm);
}

// cur = {neg_lr, ema_r, ema_rm, 0, k1, k2, 0, 0}, written by adamw_select_kernel for this step (never null here)
template <int LPB, bool G16>
__global__ void __launch_bounds__(256) adamw8_kernel(float* __restrict__ p, const void* __restrict__ g, int8_t* __restrict__ m_codes,
                                                     float* __restrict__ m_inv, int8_t* __restrict__ s_codes, float* __restrict__ s_inv,
                                                     float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n4,
                                                     const double* __restrict__ sqnorm, const float* __restrict__ thr, float max_norm,
                                                     float wd, float c1, float c1m, float c2, float c2m, float eps,
                                                     const float* __restrict__ cur) {
  int8_t* const cs[2] = {m_codes, s_codes};
  float* const is[2] = {m_inv, s_inv};
  sweep8_body<AdamwRule<true>, LPB, G16>(AdamwRule<true>{c1, c1m, c2, c2m, eps, cur[4], cur[5]}, p, g, cs, is, ema, w_bf16, n4, sqnorm,
                                         thr, max_norm, cur[0], wd, cur[1], cur[2]);
}

__global__ void __launch_bounds__(256) adamw32_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n,
                                                      const double* __restrict__ sqnorm, float max_norm, float wd, float c1, float c1m,
                                                      float c2, float c2m, float eps, const float* __restrict__ cur) {
  float* const st[2] = {m, v};
  sweep32_body(AdamwRule<false>{c1, c1m, c2, c2m, eps, cur[4], cur[5]}, p, g, st, ema, w_bf16, n, sqnorm, max_norm, cur[0], wd, cur[1],
               cur[2]);
}

__global__ void __launch_bounds__(256) lion8_quantize_kernel(const float* __restrict__ x, int8_t* __restrict__ codes,
                                                             float* __restrict__ inv_scale, long nblocks, int bs,
                                                             const float* __restrict__ thr) {
  __shared__ float deq_tab[256];
  __shared__ float thr_tab[132];
  codec_load_tables<true>(deq_tab, thr_tab, thr);
  for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += (long)gridDim.x * blockDim.x) {
    const float* xb = x + b * bs;
    float amax = 0.f;
    for (int j = 0; j < bs; ++j) amax = fmaxf(amax, fabsf(xb[j]));
    float inv = 1.0f / ((amax <= 0.f) ? 1.0f : amax);
    for (int j = 0; j < bs; ++j) codes[b * bs + j] = (int8_t)codec_quant<true>(xb[j] * inv, thr_tab);
    inv_scale[b] = inv;
  }
}

__global__ void __launch_bounds__(256) lion8_dequantize_kernel(const int8_t* __restrict__ codes,
                                                               const float* __restrict__ inv_scale,
                                                               float* __restrict__ x, long n, int bs) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    x[i] = codec_deq<true>((int)codes[i]) / inv_scale[i / bs];
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

// ------------------------------------------------------------------------------------------------------------- Prodigy
// Third optimizer (include/sdt.h "Prodigy"): Adam-style moments scaled by the running distance estimate d, which two global sums
// per step drive - so two sweeps with a one-lane kernel in front of, between and nothing behind them.  All state is float32.
//   cur = {neg_dlr, ema_r, ema_rm, first, c_m, c_v, c_s, d_eps}  (prodigy_select_kernel; d_eps by prodigy_finish_kernel)
//   st  = {d, d_max, numer, P1, P2, dot, l1, q, lr_t}             (doubles)
enum { PRODIGY_D = 0, PRODIGY_DMAX, PRODIGY_NUMER, PRODIGY_P1, PRODIGY_P2, PRODIGY_DOT, PRODIGY_L1, PRODIGY_Q, PRODIGY_LRT };

// The moments pass: the three state streams of one element, and its terms of the two sums.
struct ProdigyMomentsRule {
  float c1, c2, c3, c_m, c_v, c_s;
  static constexpr int NS = 3;  // m, v, s
  __device__ __forceinline__ void step(float gc, float dx, const float* st, float* ns, double& dot, double& l1) const {
    ns[0] = c1 * st[0] + c_m * gc;
    ns[1] = c2 * st[1] + c_v * (gc * gc);
    ns[2] = c3 * st[2] + c_s * gc;
    dot = fma((double)gc, (double)dx, dot);  // gc and dx are floats: the product is exact in double
    l1 += (double)fabsf(ns[2]);
  }
};
// The apply pass: p' from p, m', v'.
struct ProdigyApplyRule {
  float neg_dlr, neg_dlr_wd, d_eps;
  bool decay;
  __device__ __forceinline__ float step(float p, float m, float v) const {
    if (decay) p = p + neg_dlr_wd * p;
    return p + neg_dlr * (m / (sqrtf(v) + d_eps));
  }
};

// sqnorm_kernel's partition (one workgroup per 2048 float4s, at most SQNORM_MAX_BLOCKS, a grid-stride loop beyond, the n & 3 tail in
// workgroup 0) and its walk: the first accumulator of a pair takes x and z, the second y and w.
template <bool G16>
__global__ void __launch_bounds__(256) prodigy_moments_kernel(const float* __restrict__ p, const void* __restrict__ gv,
                                                              float* __restrict__ p0, float* __restrict__ m, float* __restrict__ v,
                                                              float* __restrict__ s, long n, const double* __restrict__ sqnorm,
                                                              float max_norm, float c1, float c2, float c3,
                                                              const float* __restrict__ cur, double* __restrict__ sums, int* counter,
                                                              double* __restrict__ part, int part_stride) {
  const Clip clip = clip_prologue(sqnorm, max_norm);
  const bool first = cur[3] != 0.f;
  const ProdigyMomentsRule rule = {c1, c2, c3, cur[4], cur[5], cur[6]};
  const long nv = n >> 2;
  double dot[2] = {0.0, 0.0}, l1[2] = {0.0, 0.0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    f32x4_t g4;
    if (G16) {
      const uint2 h = reinterpret_cast<const uint2*>(gv)[i];
      g4 = unpack4(h.x, h.y);
    } else {
      g4 = reinterpret_cast<const f32x4_t*>(gv)[i];
    }
    const f32x4_t p4 = reinterpret_cast<const f32x4_t*>(p)[i];
    f32x4_t q4 = p4;
    if (first) reinterpret_cast<f32x4_t*>(p0)[i] = p4;
    else q4 = reinterpret_cast<const f32x4_t*>(p0)[i];
    f32x4_t m4 = reinterpret_cast<const f32x4_t*>(m)[i];
    f32x4_t v4 = reinterpret_cast<const f32x4_t*>(v)[i];
    f32x4_t s4 = reinterpret_cast<const f32x4_t*>(s)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float st[3] = {m4[j], v4[j], s4[j]};
      float ns[3];
      rule.step(clip(g4[j]), q4[j] - p4[j], st, ns, dot[j & 1], l1[j & 1]);
      m4[j] = ns[0];
      v4[j] = ns[1];
      s4[j] = ns[2];
    }
    reinterpret_cast<f32x4_t*>(m)[i] = m4;
    reinterpret_cast<f32x4_t*>(v)[i] = v4;
    reinterpret_cast<f32x4_t*>(s)[i] = s4;
  }
  double acc[2] = {dot[0] + dot[1], l1[0] + l1[1]};
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // the < 4 elements behind the last float4
    const long j = (nv << 2) + threadIdx.x;
    const float g = G16 ? bf2f(reinterpret_cast<const bf16_t*>(gv)[j]) : reinterpret_cast<const float*>(gv)[j];
    const float pj = p[j];
    float qj = pj;
    if (first) p0[j] = pj;
    else qj = p0[j];
    const float st[3] = {m[j], v[j], s[j]};
    float ns[3];
    rule.step(clip(g), qj - pj, st, ns, acc[0], acc[1]);
    m[j] = ns[0];
    v[j] = ns[1];
    s[j] = ns[2];
  }
  ordered_sums_f64<false, 2>(acc, sums, counter, part, part_stride);
}

// A workgroup sweeps LION_SLICES consecutive slices of 256 float4s and the grid covers the buffer once (see sweep8_body).
__global__ void __launch_bounds__(256) prodigy_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                            float* __restrict__ ema, bf16_t* __restrict__ w_bf16, long n, float wd,
                                                            const float* __restrict__ cur) {
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const float neg_dlr = cur[0], ema_r = cur[1], ema_rm = cur[2];
  const ProdigyApplyRule rule = {neg_dlr, neg_dlr * wd, cur[7], wd != 0.f};
  const long nv = n >> 2;
  const long i_end = min(nv, ((long)blockIdx.x + 1) * (LION_SLICES * 256));
  for (long i = (long)blockIdx.x * (LION_SLICES * 256) + threadIdx.x; i < i_end; i += 256) {
    f32x4_t p4 = reinterpret_cast<const f32x4_t*>(p)[i];
    const f32x4_t m4 = reinterpret_cast<const f32x4_t*>(m)[i];
    const f32x4_t v4 = reinterpret_cast<const f32x4_t*>(v)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) p4[j] = rule.step(p4[j], m4[j], v4[j]);
    reinterpret_cast<f32x4_t*>(p)[i] = p4;
    if (ema) {
      const f32x4_t e4 = reinterpret_cast<const f32x4_t*>(ema)[i];
      reinterpret_cast<f32x4_t*>(ema)[i] = ema_r * e4 + ema_rm * p4;
    }
    if (w_bf16) {
      const u2v o = {pack2bf(p4.x, p4.y), pack2bf(p4.z, p4.w)};
      reinterpret_cast<u2v*>(w_bf16)[i] = o;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long j = (nv << 2) + threadIdx.x;
    const float pj = rule.step(p[j], m[j], v[j]);
    p[j] = pj;
    if (ema) ema[j] = ema_r * ema[j] + ema_rm * pj;
    if (w_bf16) w_bf16[j] = f2bf(pj);
  }
}

// Per-step scalars of a Prodigy store (include/sdt.h sdt_prodigy_select): one lane, in double, each float rounded once.
__global__ void __launch_bounds__(64) prodigy_select_kernel(int64_t* __restrict__ step, double* __restrict__ st,
                                                             const float* __restrict__ lr_tab, long n_lr, const float* __restrict__ ema_tab,
                                                             long n_ema, double lr, float ema_r, float ema_rm, double b1, double b2, double d0,
                                                             int bias_correction, int safeguard, float* __restrict__ cur) {
  if (threadIdx.x != 0) return;
  const int64_t t = *step;
  double lr_t = lr;
  if (lr_tab) {
    const long tc = t > 0 ? (long)t : 0;
    const long i = tc < n_lr - 1 ? tc : n_lr - 1;
    const long j = tc < n_ema - 1 ? tc : n_ema - 1;
    lr_t = -(double)lr_tab[i];
    ema_r = ema_tab[2 * j];
    ema_rm = ema_tab[2 * j + 1];
  }
  const double p1 = st[PRODIGY_P1] * b1, p2 = st[PRODIGY_P2] * b2;
  st[PRODIGY_P1] = p1;
  st[PRODIGY_P2] = p2;
  const double bc = bias_correction ? sqrt(1.0 - p2) / (1.0 - p1) : 1.0;
  const double d = st[PRODIGY_D];
  const double dlr = (d * lr_t) * bc;
  const double q = (d / d0) * dlr;
  cur[0] = (float)(-dlr);
  cur[1] = ema_r;
  cur[2] = ema_rm;
  cur[3] = t == 0 ? 1.f : 0.f;
  cur[4] = (float)(d * (1.0 - b1));
  cur[5] = (float)((d * d) * (1.0 - b2));
  cur[6] = (float)(safeguard ? (d / d0) * d : q);
  cur[7] = 0.f;
  st[PRODIGY_DOT] = 0.0;
  st[PRODIGY_L1] = 0.0;
  st[PRODIGY_Q] = q;
  st[PRODIGY_LRT] = lr_t;
  *step = t + 1;
}

// The step's new d from the two sums (include/sdt.h sdt_prodigy_finish): one lane, between the moments and the apply sweeps.
__global__ void __launch_bounds__(64) prodigy_finish_kernel(double* __restrict__ st, float* __restrict__ cur, double beta3, double d0,
                                                             double d_coef, double growth_rate, double eps) {
  if (threadIdx.x != 0) return;
  const double numer = beta3 * st[PRODIGY_NUMER] + st[PRODIGY_Q] * st[PRODIGY_DOT];
  const double l1 = st[PRODIGY_L1];
  double d = st[PRODIGY_D];
  st[PRODIGY_NUMER] = numer;
  if (l1 != 0.0 && st[PRODIGY_LRT] > 0.0) {
    const double d_hat = (d_coef * numer) / l1;
    double d_max = st[PRODIGY_DMAX];
    if (d == d0) d = d_hat > d ? d_hat : d;
    d_max = d_hat > d_max ? d_hat : d_max;
    const double grown = d * growth_rate;
    d = grown < d_max ? grown : d_max;
    st[PRODIGY_DMAX] = d_max;
    st[PRODIGY_D] = d;
  }
  cur[7] = (float)(d * eps);
}

// ----------------------------------------------------------------------------------------------------------- host side
// The float scalars every sweep and select launch derives from the entry points' doubles.
struct HostScalars {
  float c1, c1m, c2, c2m, neg_lr, er, erm;
};
static HostScalars host_scalars(double b1, double b2, double lr = 0.0, double ema_rate = 0.0) {
  return {(float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)(-lr), (float)ema_rate, (float)(1.0 - ema_rate)};
}

// launch(LPB, G16), both as integral constants, for the 8-bit sweep of `block_size` elements per block
template <class F>
static void dispatch_sweep8(int block_size, int g_bf16, F&& launch) {
  auto with_g = [&](auto lpb) {
    if (g_bf16)
      launch(lpb, std::true_type{});
    else
      launch(lpb, std::false_type{});
  };
  switch (block_size >> 2) {
    case 1: with_g(std::integral_constant<int, 1>{}); break;
    case 2: with_g(std::integral_constant<int, 2>{}); break;
    case 4: with_g(std::integral_constant<int, 4>{}); break;
    case 8: with_g(std::integral_constant<int, 8>{}); break;
    case 16: with_g(std::integral_constant<int, 16>{}); break;
    case 32: with_g(std::integral_constant<int, 32>{}); break;
    default: with_g(std::integral_constant<int, 64>{}); break;
  }
}

// The refusals of the three 8-bit sweeps, made before any HIP call.  adamw: the second code / scale stream and cur are required too.
static int check_sweep8_args(const char* name, bool adamw, const float* p, const void* g, int g_bf16, const int8_t* codes,
                             const float* inv_scale, const int8_t* codes2, const float* inv_scale2, const float* ema,
                             const uint16_t* w_bf16, int64_t n, int block_size, const float* thresholds, const float* cur) {
  SDT_CHECK_ARG(p && g && codes && inv_scale && thresholds && (!adamw || (codes2 && inv_scale2 && cur)), "%s: null pointer", name);
  SDT_CHECK_ARG(n >= 0 && block_size >= 4 && block_size <= 256 && (block_size & (block_size - 1)) == 0,
                "%s: block_size must be a power of two in [4,256] (got %d)", name, block_size);
  SDT_CHECK_ARG(n % block_size == 0, "%s: n=%ld not a multiple of block_size=%d%s", name, (long)n, block_size,
                adamw ? "" : " (lion_quant.py:70 reshape)");
  SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)ema | (uintptr_t)cur) & 15) == 0 && ((uintptr_t)g & (g_bf16 ? 7 : 15)) == 0 &&
                    (((uintptr_t)codes | (uintptr_t)codes2) & 3) == 0 && ((uintptr_t)w_bf16 & 7) == 0,
                "%s: misaligned buffer", name);
  return SDT_OK;
}

static void launch_lion8(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16, int64_t n,
                         int block_size, const double* sqnorm, const float* thresholds, double max_norm, double wd,
                         const HostScalars& h, const float* cur, hipStream_t stream) {
  const long n4 = n >> 2;
  dispatch_sweep8(block_size, g_bf16, [&](auto lpb, auto g16) {
    hipLaunchKernelGGL((lion8_kernel<decltype(lpb)::value, decltype(g16)::value>), dim3(sdt_grid_1d(n4, 256 * LION_SLICES, 1 << 30)),
                       dim3(256), 0, stream, p, g, codes, inv_scale, ema, (bf16_t*)w_bf16, n4, sqnorm, thresholds, (float)max_norm,
                       h.neg_lr, (float)wd, h.c1, h.c1m, h.c2, h.c2m, h.er, h.erm, cur);
  });
}

static void launch_lion32(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                          double max_norm, double wd, const HostScalars& h, const float* cur, hipStream_t stream) {
  hipLaunchKernelGGL(lion32_kernel, dim3(sdt_grid_1d(n, 1024, 1 << 30)), dim3(256), 0, stream, p, g, mom, ema, (bf16_t*)w_bf16, (long)n,
                     sqnorm, (float)max_norm, h.neg_lr, (float)wd, h.c1, h.c1m, h.c2, h.c2m, h.er, h.erm, cur);
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

int sdt_lion8_step(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16, int64_t n,
                   int block_size, const double* sqnorm, const float* thresholds, double max_norm, double lr, double wd,
                   double b1, double b2, double ema_rate, hipStream_t stream) {
  if (int rc = check_sweep8_args("sdt_lion8_step", false, p, g, g_bf16, codes, inv_scale, nullptr, nullptr, ema, w_bf16, n, block_size,
                                 thresholds, nullptr))
    return rc;
  if (n == 0) return SDT_OK;
  launch_lion8(p, g, g_bf16, codes, inv_scale, ema, w_bf16, n, block_size, sqnorm, thresholds, max_norm, wd,
               host_scalars(b1, b2, lr, ema_rate), nullptr, stream);
  SDT_LAUNCH_CHECK("sdt_lion8_step");
  return SDT_OK;
}

int sdt_lion8_step_scheduled(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16,
                             int64_t n, int block_size, const double* sqnorm, const float* thresholds, double max_norm, const float* cur,
                             double wd, double b1, double b2, hipStream_t stream) {
  if (int rc = check_sweep8_args("sdt_lion8_step_scheduled", false, p, g, g_bf16, codes, inv_scale, nullptr, nullptr, ema, w_bf16, n,
                                 block_size, thresholds, nullptr))
    return rc;
  SDT_CHECK_ARG(cur && ((uintptr_t)cur & 15) == 0, "sdt_lion8_step_scheduled: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  launch_lion8(p, g, g_bf16, codes, inv_scale, ema, w_bf16, n, block_size, sqnorm, thresholds, max_norm, wd, host_scalars(b1, b2), cur,
               stream);
  SDT_LAUNCH_CHECK("sdt_lion8_step_scheduled");
  return SDT_OK;
}

int sdt_lion32_step(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n,
                    const double* sqnorm, double max_norm, double lr, double wd, double b1, double b2, double ema_rate,
                    hipStream_t stream) {
  SDT_CHECK_ARG(p && g && mom && n >= 0, "sdt_lion32_step: null pointer or negative n");
  if (n == 0) return SDT_OK;
  launch_lion32(p, g, mom, ema, w_bf16, n, sqnorm, max_norm, wd, host_scalars(b1, b2, lr, ema_rate), nullptr, stream);
  SDT_LAUNCH_CHECK("sdt_lion32_step");
  return SDT_OK;
}

int sdt_lion32_step_scheduled(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                              double max_norm, const float* cur, double wd, double b1, double b2, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && mom && n >= 0, "sdt_lion32_step_scheduled: null pointer or negative n");
  SDT_CHECK_ARG(cur && ((uintptr_t)cur & 15) == 0, "sdt_lion32_step_scheduled: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  launch_lion32(p, g, mom, ema, w_bf16, n, sqnorm, max_norm, wd, host_scalars(b1, b2), cur, stream);
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
  const HostScalars h = host_scalars(b1, b2, lr, ema_rate);
  hipLaunchKernelGGL(adamw_select_kernel, dim3(1), dim3(64), 0, stream, step, prods, lr_tab, (long)n_lr, ema_tab, (long)n_ema, h.neg_lr,
                     h.er, h.erm, b1, b2, cur);
  SDT_LAUNCH_CHECK("sdt_adamw_select");
  return SDT_OK;
}

int sdt_adamw8_step(float* p, const void* g, int g_bf16, int8_t* m_codes, float* m_inv_scale, int8_t* s_codes, float* s_inv_scale,
                    float* ema, uint16_t* w_bf16, int64_t n, int block_size, const double* sqnorm, const float* thresholds,
                    double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream) {
  if (int rc = check_sweep8_args("sdt_adamw8_step", true, p, g, g_bf16, m_codes, m_inv_scale, s_codes, s_inv_scale, ema, w_bf16, n,
                                 block_size, thresholds, cur))
    return rc;
  if (n == 0) return SDT_OK;
  const long n4 = n >> 2;
  const HostScalars h = host_scalars(b1, b2);
  dispatch_sweep8(block_size, g_bf16, [&](auto lpb, auto g16) {
    hipLaunchKernelGGL((adamw8_kernel<decltype(lpb)::value, decltype(g16)::value>), dim3(sdt_grid_1d(n4, 256 * LION_SLICES, 1 << 30)),
                       dim3(256), 0, stream, p, g, m_codes, m_inv_scale, s_codes, s_inv_scale, ema, (bf16_t*)w_bf16, n4, sqnorm,
                       thresholds, (float)max_norm, (float)wd, h.c1, h.c1m, h.c2, h.c2m, (float)eps, cur);
  });
  SDT_LAUNCH_CHECK("sdt_adamw8_step");
  return SDT_OK;
}

int sdt_adamw32_step(float* p, const float* g, float* m, float* v, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                     double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && m && v && cur && n >= 0, "sdt_adamw32_step: null pointer or negative n");
  SDT_CHECK_ARG(((uintptr_t)cur & 15) == 0, "sdt_adamw32_step: cur must be a 16-byte aligned device block");
  if (n == 0) return SDT_OK;
  const HostScalars h = host_scalars(b1, b2);
  hipLaunchKernelGGL(adamw32_kernel, dim3(sdt_grid_1d(n, 1024, 1 << 30)), dim3(256), 0, stream, p, g, m, v, ema, (bf16_t*)w_bf16, (long)n,
                     sqnorm, (float)max_norm, (float)wd, h.c1, h.c1m, h.c2, h.c2m, (float)eps, cur);
  SDT_LAUNCH_CHECK("sdt_adamw32_step");
  return SDT_OK;
}

int64_t sdt_prodigy_workspace_bytes(void) { return SDT_WS_COUNTER_BYTES + 2 * SQNORM_MAX_BLOCKS * (int64_t)sizeof(double); }

int sdt_prodigy_select(int64_t* step, double* state, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, double lr,
                       double ema_rate, double b1, double b2, double d0, int use_bias_correction, int safeguard_warmup, float* cur,
                       hipStream_t stream) {
  SDT_CHECK_ARG(step && state && cur, "sdt_prodigy_select: null pointer");
  SDT_CHECK_ARG((lr_tab != nullptr) == (ema_tab != nullptr), "sdt_prodigy_select: lr_tab and ema_tab come together or not at all");
  SDT_CHECK_ARG(!lr_tab || (n_lr >= 1 && n_ema >= 1), "sdt_prodigy_select: every table needs at least one entry (n_lr=%ld, n_ema=%ld)",
                (long)n_lr, (long)n_ema);
  SDT_CHECK_ARG(std::isfinite(lr) && std::isfinite(ema_rate) && std::isfinite(d0), "sdt_prodigy_select: non-finite lr, ema_rate or d0");
  SDT_CHECK_ARG(lr >= 0.0, "sdt_prodigy_select: lr must not be negative (got %g)", lr);
  SDT_CHECK_ARG(d0 > 0.0, "sdt_prodigy_select: d0 must be positive (got %g)", d0);
  SDT_CHECK_ARG(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, "sdt_prodigy_select: b1 and b2 must lie in [0, 1) (got %g, %g)", b1, b2);
  SDT_CHECK_ARG((((uintptr_t)step | (uintptr_t)state | (uintptr_t)ema_tab) & 7) == 0 && ((uintptr_t)cur & 15) == 0,
                "sdt_prodigy_select: misaligned step counter, state, table or block");
  const HostScalars h = host_scalars(b1, b2, lr, ema_rate);
  hipLaunchKernelGGL(prodigy_select_kernel, dim3(1), dim3(64), 0, stream, step, state, lr_tab, (long)n_lr, ema_tab, (long)n_ema, lr, h.er,
                     h.erm, b1, b2, d0, use_bias_correction, safeguard_warmup, cur);
  SDT_LAUNCH_CHECK("sdt_prodigy_select");
  return SDT_OK;
}

int sdt_prodigy_moments_step(const float* p, const void* g, int g_bf16, float* p0, float* m, float* v, float* s, int64_t n,
                             const double* sqnorm, double max_norm, const float* cur, double* state, double b1, double b2, double beta3,
                             void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(p && g && p0 && m && v && s && cur && state, "sdt_prodigy_moments_step: null pointer");
  SDT_CHECK_ARG(n >= 0, "sdt_prodigy_moments_step: negative n (%ld)", (long)n);
  SDT_CHECK_ARG(std::isfinite(max_norm) && b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0 && beta3 >= 0.0 && beta3 < 1.0,
                "sdt_prodigy_moments_step: max_norm must be finite and b1, b2, beta3 lie in [0, 1) (got %g, %g, %g, %g)", max_norm, b1, b2,
                beta3);
  SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)p0 | (uintptr_t)m | (uintptr_t)v | (uintptr_t)s | (uintptr_t)cur) & 15) == 0 &&
                    ((uintptr_t)g & (g_bf16 ? 7 : 15)) == 0 && ((uintptr_t)state & 7) == 0,
                "sdt_prodigy_moments_step: misaligned buffer");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_prodigy_workspace_bytes(),
                "sdt_prodigy_moments_step: workspace of sdt_prodigy_workspace_bytes() needed");
  if (n == 0) return SDT_OK;
  const dim3 grid(sdt_grid_1d(n >> 2, 256 * 8, SQNORM_MAX_BLOCKS)), block(256);  // sqnorm_kernel's grid: the same partition
  int* counter = reinterpret_cast<int*>(workspace);
  double* part = reinterpret_cast<double*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES);
  const HostScalars h = host_scalars(b1, b2);
  if (g_bf16)
    hipLaunchKernelGGL(prodigy_moments_kernel<true>, grid, block, 0, stream, p, g, p0, m, v, s, (long)n, sqnorm, (float)max_norm, h.c1, h.c2,
                       (float)beta3, cur, state + PRODIGY_DOT, counter, part, SQNORM_MAX_BLOCKS);
  else
    hipLaunchKernelGGL(prodigy_moments_kernel<false>, grid, block, 0, stream, p, g, p0, m, v, s, (long)n, sqnorm, (float)max_norm, h.c1, h.c2,
                       (float)beta3, cur, state + PRODIGY_DOT, counter, part, SQNORM_MAX_BLOCKS);
  SDT_LAUNCH_CHECK("sdt_prodigy_moments_step");
  return SDT_OK;
}

int sdt_prodigy_finish(double* state, float* cur, double beta3, double d0, double d_coef, double growth_rate, double eps,
                       hipStream_t stream) {
  SDT_CHECK_ARG(state && cur, "sdt_prodigy_finish: null pointer");
  SDT_CHECK_ARG(std::isfinite(beta3) && std::isfinite(d0) && std::isfinite(d_coef) && std::isfinite(eps) && !std::isnan(growth_rate),
                "sdt_prodigy_finish: non-finite beta3, d0, d_coef or eps, or growth_rate is not a number");
  SDT_CHECK_ARG(d0 > 0.0, "sdt_prodigy_finish: d0 must be positive (got %g)", d0);
  SDT_CHECK_ARG(beta3 >= 0.0 && beta3 < 1.0, "sdt_prodigy_finish: beta3 must lie in [0, 1) (got %g)", beta3);
  SDT_CHECK_ARG(growth_rate > 0.0 && d_coef > 0.0 && eps >= 0.0,
                "sdt_prodigy_finish: growth_rate (+inf allowed) and d_coef must be positive, eps not negative (got %g, %g, %g)", growth_rate,
                d_coef, eps);
  SDT_CHECK_ARG(((uintptr_t)state & 7) == 0 && ((uintptr_t)cur & 15) == 0, "sdt_prodigy_finish: misaligned state or block");
  hipLaunchKernelGGL(prodigy_finish_kernel, dim3(1), dim3(64), 0, stream, state, cur, beta3, d0, d_coef, growth_rate, eps);
  SDT_LAUNCH_CHECK("sdt_prodigy_finish");
  return SDT_OK;
}

int sdt_prodigy_apply_step(float* p, const float* m, const float* v, float* ema, uint16_t* w_bf16, int64_t n, const float* cur, double wd,
                           hipStream_t stream) {
  SDT_CHECK_ARG(p && m && v && cur, "sdt_prodigy_apply_step: null pointer");
  SDT_CHECK_ARG(n >= 0, "sdt_prodigy_apply_step: negative n (%ld)", (long)n);
  SDT_CHECK_ARG(std::isfinite(wd), "sdt_prodigy_apply_step: non-finite wd");
  SDT_CHECK_ARG((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)cur) & 15) == 0 && ((uintptr_t)w_bf16 & 7) == 0,
                "sdt_prodigy_apply_step: misaligned buffer");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(prodigy_apply_kernel, dim3(sdt_grid_1d(n >> 2, 256 * LION_SLICES, 1 << 30)), dim3(256), 0, stream, p, m, v, ema,
                     (bf16_t*)w_bf16, (long)n, (float)wd, cur);
  SDT_LAUNCH_CHECK("sdt_prodigy_apply_step");
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
