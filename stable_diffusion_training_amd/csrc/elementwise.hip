// HBM-bound elementwise / data-movement kernels of the train_step path (all bf16 I/O is
// 16 bytes per lane, fp32 math).  Reference call sites:
//   add_noise / get_velocity   schedulers/scheduling_utils_flax.py:316-343 (via training_utils.py:628-633, 691-696)
//   posterior sample + scale   training_utils.py:582-586
//   MSE (+min-SNR weight)      training_utils.py:546-568, 704-709
//   timestep embedding         diffusers embeddings_flax.get_sinusoidal_embeddings (training_utils.py:678-684)
//   GEGLU / SiLU / quick-GELU / nearest-2x / concat: diffusers attention_flax.py, resnet_flax.py,
//   unet_2d_blocks_flax.py; transformers modeling_flax_clip.py (third-party, restated in oracle/nets.py)
#include "sdt_common.h"

// ------------------------------------------------------------------ noise add (+ velocity target)
// latents/noise: f32 NCHW (B,C,H,W).  Outputs: noisy bf16 NHWC with channels padded to cpad (zeros),
// optional noisy f32 NCHW, optional velocity target f32 NCHW.
__global__ void __launch_bounds__(256) add_noise_kernel(const float* __restrict__ lat, const float* __restrict__ noise,
                                                        const int* __restrict__ t, const float* __restrict__ acp,
                                                        bf16_t* __restrict__ noisy_nhwc, float* __restrict__ noisy_nchw,
                                                        float* __restrict__ vel_nchw, int B, int C, int HW, int cpad) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float a = acp[t[b]];
    const float sa = sqrtf(a), so = sqrtf(1.0f - a);  // ** 0.5 in the reference
    for (int c = 0; c < cpad; ++c) {
      float nz = 0.f;
      if (c < C) {
        const long off = ((long)b * C + c) * HW + p;
        const float x0 = lat[off], e = noise[off];
        nz = sa * x0 + so * e;
        if (noisy_nchw) noisy_nchw[off] = nz;
        if (vel_nchw) vel_nchw[off] = sa * e - so * x0;
      }
      noisy_nhwc[i * cpad + c] = f2bf(nz);
    }
  }
}

// One sampling step of the reference pipeline (models/pipeline_flax_stable_diffusion.py:222-232) in one launch:
// classifier-free guidance  m = un + g*(tx - un)  over the doubled UNet batch (pred rows [0,B) unconditional, [B,2B) text),
// the eta = 0 DDIM update of diffusers' scheduling_ddim_flax.py step(), and the doubled bf16 NHWC UNet input of the next
// step.  lat f32 NCHW (B,C,h,w) in place; pred / x_next bf16 NHWC (2B,h,w,cpad), padding channels written as zero.
// ptype: 0 epsilon, 1 sample, 2 v_prediction.
__global__ void __launch_bounds__(256) ddim_cfg_step_kernel(const bf16_t* __restrict__ pred, float* __restrict__ lat,
                                                            bf16_t* __restrict__ x_next, int B, int C, int HW, int cpad,
                                                            float guidance, float sa, float sb, float sa_prev, float sb_prev,
                                                            int ptype) {
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    for (int c = 0; c < cpad; ++c) {
      float nx = 0.f;
      if (c < C) {
        const long off = ((long)b * C + c) * HW + p;
        const float un = bf2f(pred[i * cpad + c]), tx = bf2f(pred[(i + total) * cpad + c]);
        const float m = un + guidance * (tx - un);
        const float x = lat[off];
        float x0, eps;
        if (ptype == 0) { x0 = (x - sb * m) / sa; eps = m; }
        else if (ptype == 1) { x0 = m; eps = (x - sa * x0) / sb; }
        else { x0 = sa * x - sb * m; eps = sa * m + sb * x; }
        nx = sa_prev * x0 + sb_prev * eps;
        lat[off] = nx;
      }
      const bf16_t v = f2bf(nx);
      x_next[i * cpad + c] = v;
      x_next[(i + total) * cpad + c] = v;
    }
  }
}

// diffusers' rescale_noise_cfg factor per sample b (arXiv:2305.08891 §3.4): cfg = un + g*(tx - un) over the C real channels of
// the (h,w) map, f_b = phi * std(tx_b) / std(cfg_b) + (1 - phi), std unbiased (N - 1); f_b = 1 when std(cfg_b) == 0.  One
// workgroup per sample, a fixed pixel-to-thread map and a fixed reduction tree (wave shuffle, then the 4 wave totals in order):
// no atomics, so the factors are the same bits on every launch.  pred bf16 NHWC (2B,h,w,cpad), cpad % 8 == 0.
__global__ void __launch_bounds__(256) cfg_rescale_factors_kernel(const uint4* __restrict__ pred, float* __restrict__ factors,
                                                                  int B, int C, int HW, int cpad, float guidance, float phi) {
  __shared__ double s_part[4][4];
  const int b = blockIdx.x, nv = cpad / 8;
  const long total = (long)B * HW;
  double st = 0.0, st2 = 0.0, sc = 0.0, sc2 = 0.0;  // sums of tx, tx^2, cfg, cfg^2
  for (int p = threadIdx.x; p < HW; p += 256) {
    const long i = (long)b * HW + p;
    for (int v = 0; v < nv; ++v) {
      float un[8], tx[8];
      unpack8(pred[i * nv + v], un);
      unpack8(pred[(i + total) * nv + v], tx);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (v * 8 + e < C) {
          const double t = tx[e], m = un[e] + guidance * (tx[e] - un[e]);
          st += t; st2 += t * t; sc += m; sc2 += m * m;
        }
      }
    }
  }
  double r[4] = {st, st2, sc, sc2};
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r[k] += __shfl_xor(r[k], o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k) s_part[w][k] = r[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[4];
    for (int k = 0; k < 4; ++k) t[k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
    const double n = (double)C * HW;
    const double var_t = fmax((t[1] - t[0] * t[0] / n) / (n - 1.0), 0.0), var_c = fmax((t[3] - t[2] * t[2] / n) / (n - 1.0), 0.0);
    factors[b] = var_c > 0.0 ? (float)(phi * sqrt(var_t / var_c) + (1.0 - phi)) : 1.0f;
  }
}

// The update of the DDIM paths sdt_ddim_cfg_step does not serve (trailing / linspace timesteps, a t with alpha_prod 0, guidance
// rescale) and of DPM-Solver++(2M) (diffusers scheduling_dpmsolver_multistep_flax.py, algorithm dpmsolver++, midpoint), per pixel:
//   m = (un + g*(tx - un)) * f_b              f_b from cfg_rescale_factors_kernel, or 1 when `factors` is null
//   x0, eps from m and x by ptype with (sa, sb) = (alpha_s, sigma_s) of the current timestep (as ddim_cfg_step_kernel)
//   x <- c_x*x + c_x0*x0 + c_eps*eps + c_d1*(x0 - x0_prev)
// The host folds each sampler into the four coefficients (schedulers.py).  hist (f32 NCHW, optional) is the x0 of the previous
// step: read only when c_d1 != 0 (its first use may find it unwritten), then overwritten with this step's x0.  pred / x_next
// bf16 NHWC (2B,h,w,cpad) as uint4 (8 channels), padding channels of x_next written as zero.
__global__ void __launch_bounds__(256) sampler_cfg_step_kernel(const uint4* __restrict__ pred, float* __restrict__ lat,
                                                               uint4* __restrict__ x_next, float* __restrict__ hist,
                                                               const float* __restrict__ factors, int B, int C, int HW, int cpad,
                                                               float guidance, float sa, float sb, int ptype, float c_x, float c_x0,
                                                               float c_eps, float c_d1) {
  const long total = (long)B * HW;
  const int nv = cpad / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float f = factors ? factors[b] : 1.0f;
    for (int v = 0; v < nv; ++v) {
      float un[8], tx[8], nx[8];
      unpack8(pred[i * nv + v], un);
      unpack8(pred[(i + total) * nv + v], tx);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = v * 8 + e;
        nx[e] = 0.f;
        if (c < C) {
          const long off = ((long)b * C + c) * HW + p;
          const float m = (un[e] + guidance * (tx[e] - un[e])) * f;
          const float x = lat[off];
          float x0, eps;
          if (ptype == 0) { x0 = (x - sb * m) / sa; eps = m; }
          else if (ptype == 1) { x0 = m; eps = (x - sa * x0) / sb; }
          else { x0 = sa * x - sb * m; eps = sa * m + sb * x; }
          float y = c_x * x + c_x0 * x0 + c_eps * eps;
          if (hist) {
            if (c_d1 != 0.f) y += c_d1 * (x0 - hist[off]);
            hist[off] = x0;
          }
          nx[e] = y;
          lat[off] = y;
        }
      }
      const uint4 o = pack8(nx);
      x_next[i * nv + v] = o;
      x_next[(i + total) * nv + v] = o;
    }
  }
}

// moments bf16 NHWC (B,h,w,mstride) with mean = ch [0,L), logvar = ch [L,2L); eps f32 NHWC (B,h,w,L)
// -> latents f32 NCHW (B,L,h,w) = (mean + exp(0.5*clip(logvar,-30,20))*eps) * scale
__global__ void __launch_bounds__(256) posterior_sample_kernel(const bf16_t* __restrict__ mom, const float* __restrict__ eps,
                                                               float* __restrict__ lat, int B, int L, int HW, int mstride,
                                                               float scale) {
  const long total = (long)B * HW * L;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % L);
    const long bp = i / L;
    const int b = (int)(bp / HW), p = (int)(bp % HW);
    const float mean = bf2f(mom[bp * mstride + c]);
    float lv = bf2f(mom[bp * mstride + L + c]);
    // jnp.clip keeps a NaN (fminf / fmaxf would return the bound and hand back a finite latent for a NaN log-variance)
    lv = lv < -30.f ? -30.f : (lv > 20.f ? 20.f : lv);
    const float v = (mean + __expf(0.5f * lv) * eps[i]) * scale;
    lat[((long)b * L + c) * HW + p] = v;
  }
}

// The front of a training step from cached posterior moments in one launch: posterior_sample_kernel, the noise mixing that
// train_step does with torch element-wise kernels in between (noise + offset[b][c] * offset_mag, then + perturb_mag * perturb:
// separate fp32 multiplies and adds) and add_noise_kernel.  One thread per latent pixel, channels in groups of 8.
// The results carry the bits of that chain, so every rounding point is spelled out instead of left to contraction: the two
// kernels above compile to  x0 = fl(fma(e, eps, mean) * scale),  noisy = fma(sa, x0, fl(so * n)),  velocity = fl(sa * n) - fl(so * x0).
// VEC_IN: a pixel's moments by 16-byte loads (mstride % 8 == 0, L % 4 == 0, 16-byte aligned base: the log-variances then start at
// a 16- or 8-byte boundary of the row); VEC_OUT: the bf16 row by 16-byte stores (cpad % 8 == 0, aligned base).
// The posterior sample of one channel with posterior_sample_kernel's bits: fl(fma(exp(0.5 * clip(lv)), eps, mean) * scale).
__device__ __forceinline__ float posterior_element(float mean, float lv, float eps, float scale) {
#pragma clang fp contract(off)
  lv = lv < -30.f ? -30.f : (lv > 20.f ? 20.f : lv);  // keeps a NaN, as posterior_sample_kernel
  return __fmaf_rn(__expf(0.5f * lv), eps, mean) * scale;
}

// One latent element of the fused front (latent_noise_target_kernel and inpaint_noise_target_kernel): the sample, the mixed noise,
// the optional fp32 outputs at `off` (NCHW) and the noisy value that goes into the bf16 row.  bc = b * L + c.
__device__ __forceinline__ float noise_target_element(float mean, float lv, float eps, long off, int bc, float sa, float so,
                                                      const float* __restrict__ noise, const float* __restrict__ offset,
                                                      const float* __restrict__ perturb, float* __restrict__ target,
                                                      float* __restrict__ lat_nchw, float* __restrict__ noisy_nchw, float scale,
                                                      float offset_mag, float perturb_mag, int ptype) {
#pragma clang fp contract(off)
  const float x0 = posterior_element(mean, lv, eps, scale);
  float n = noise[off];
  if (offset) n = n + offset[bc] * offset_mag;
  if (perturb) n = n + perturb_mag * perturb[off];
  const float v = __fmaf_rn(sa, x0, so * n);
  if (lat_nchw) lat_nchw[off] = x0;
  if (noisy_nchw) noisy_nchw[off] = v;
  if (target) target[off] = ptype == 2 ? sa * n - so * x0 : n;
  return v;
}

template <bool VEC_IN, bool VEC_OUT>
__global__ void __launch_bounds__(256) latent_noise_target_kernel(
    const bf16_t* __restrict__ mom, const float* __restrict__ eps, const float* __restrict__ noise, const float* __restrict__ offset,
    const float* __restrict__ perturb, const int* __restrict__ t, const float* __restrict__ acp, bf16_t* __restrict__ noisy_nhwc,
    float* __restrict__ target, float* __restrict__ lat_nchw, float* __restrict__ noisy_nchw, int B, int L, int HW, int mstride,
    int cpad, float scale, float offset_mag, float perturb_mag, int ptype) {
#pragma clang fp contract(off)
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float a = acp[t[b]];
    const float sa = sqrtf(a), so = sqrtf(1.0f - a);
    const bf16_t* row = mom + i * mstride;
    for (int c0 = 0; c0 < cpad; c0 += 8) {
      float nz[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (c0 < L) {
        float mean[8], lv[8];
        if (VEC_IN) {
          // mean: columns [c0, c0 + 8) (the row holds them: c0 + 8 <= roundup8(2L) <= mstride); log-variance: columns from L + c0,
          // which sit at dword 0 or 2 of an aligned vector; the vector after it is read only where it holds a channel below L
          unpack8(*reinterpret_cast<const uint4*>(row + c0), mean);
          const int s = (L + c0) & 7;
          const uint4 va = *reinterpret_cast<const uint4*>(row + L + c0 - s);
          uint4 v = va;
          if (s) {
            uint4 vb = make_uint4(0u, 0u, 0u, 0u);
            if (c0 + 4 < L) vb = *reinterpret_cast<const uint4*>(row + L + c0 - s + 8);
            v = make_uint4(va.z, va.w, vb.x, vb.y);
          }
          unpack8(v, lv);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool in = c0 + j < L;
            mean[j] = in ? bf2f(row[c0 + j]) : 0.f;
            lv[j] = in ? bf2f(row[L + c0 + j]) : 0.f;
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = c0 + j;
          if (c < L) {
            nz[j] = noise_target_element(mean[j], lv[j], eps[i * L + c], ((long)b * L + c) * HW + p, b * L + c, sa, so, noise, offset,
                                         perturb, target, lat_nchw, noisy_nchw, scale, offset_mag, perturb_mag, ptype);
          }
        }
      }
      if (VEC_OUT) {
        *reinterpret_cast<uint4*>(noisy_nhwc + i * cpad + c0) = pack8(nz);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < cpad) noisy_nhwc[i * cpad + c0 + j] = f2bf(nz[j]);
      }
    }
  }
}

// ------------------------------------------------------------------ inpainting (include/sdt.h "INPAINTING")
// 1 repaints, 0 keeps; a NaN compares false and keeps.
__device__ __forceinline__ bool repaint(float m) { return m >= 0.5f; }

// Columns [col, col + 8) of a bf16 row as four dwords; col may be any integer (negative too).  Only the columns inside [lo, hi) are
// meaningful to the caller (the others come back as 0 or as whatever the row holds there).  VEC (stride % 8 == 0, 16-byte aligned
// row): the one or two aligned 16-byte vectors that hold them, each read only where it lies inside the row and overlaps [lo, hi),
// then shifted down by col & 7 elements through static selects.  Otherwise element by element.
template <bool VEC>
__device__ __forceinline__ uint4 row_cols8(const bf16_t* __restrict__ row, int col, int lo, int hi, int stride) {
  if (VEC) {
    const int s = col & 7, a = col - s;
    uint4 va = make_uint4(0u, 0u, 0u, 0u), vb = va;
    if (a >= 0 && a + 8 <= stride && a + 8 > lo && a < hi) va = *reinterpret_cast<const uint4*>(row + a);
    if (s && a + 8 >= 0 && a + 16 <= stride && a + 16 > lo && a + 8 < hi) vb = *reinterpret_cast<const uint4*>(row + a + 8);
    unsigned d[9] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w, 0u};
    if (s & 4) {
#pragma unroll
      for (int k = 0; k < 9; ++k) d[k] = k + 2 < 9 ? d[k + 2] : 0u;
    }
    if (s & 2) {
#pragma unroll
      for (int k = 0; k < 9; ++k) d[k] = k + 1 < 9 ? d[k + 1] : 0u;
    }
    if (s & 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = (d[k] >> 16) | (d[k + 1] << 16);
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
  } else {
    unsigned d[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = col + 2 * k;
      const unsigned e0 = (c >= lo && c < hi) ? row[c] : 0u, e1 = (c + 1 >= lo && c + 1 < hi) ? row[c + 1] : 0u;
      d[k] = e0 | (e1 << 16);
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
  }
}

// pixels f32 NCHW (B,C,H,W), mask f32 (B,H,W) -> stacked bf16 NHWC (2B,H,W,cpad): rows [0,B) the image as nchw_to_nhwc_kernel
// writes it, rows [B,2B) the masked image (repaint ? +0 : x, a select), padding zero; latent_mask f32 (B,H/f,W/f) nearest
// neighbour (the top-left pixel of each f x f block).  One thread per pixel: the mask and each channel plane are read coalesced
// along W, the two bf16 rows go out by 16-byte stores (VEC: cpad % 8 == 0, aligned base).
template <bool VEC>
__global__ void __launch_bounds__(256) inpaint_mask_pixels_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                                  bf16_t* __restrict__ stacked, float* __restrict__ latent_mask,
                                                                  int B, int C, int H, int W, int cpad, int f) {
  const long HW = (long)H * W, total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const long p = i % HW;
    const int py = (int)(p / W), px = (int)(p % W);
    const bool rp = repaint(mask[i]);
    if (py % f == 0 && px % f == 0) latent_mask[((long)b * (H / f) + py / f) * (W / f) + px / f] = rp ? 1.0f : 0.0f;
    bf16_t* img = stacked + i * cpad;
    bf16_t* msk = stacked + (total + i) * cpad;
    for (int c0 = 0; c0 < cpad; c0 += 8) {
      float v[8], m[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        v[j] = c < C ? x[((long)b * C + c) * HW + p] : 0.f;
        m[j] = rp ? 0.f : v[j];
      }
      if (VEC) {
        *reinterpret_cast<uint4*>(img + c0) = pack8(v);
        *reinterpret_cast<uint4*>(msk + c0) = pack8(m);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < cpad) {
            img[c0 + j] = f2bf(v[j]);
            msk[c0 + j] = f2bf(m[j]);
          }
      }
    }
  }
}

// latent_noise_target_kernel with an inpainting UNet's input row: channels [0,L) the noisy latents (noise_target_element: the
// same bits), [L] the thresholded latent mask, [L+1,2L+1) the posterior sample of the masked image's moments with its own draw
// (posterior_element, rounded to bf16 with the row), the rest zero.  One thread per latent pixel; each 8-channel group of the row
// is built in registers and stored once.  VEC_IN: both moment rows by 16-byte loads (mstride % 8 == 0, aligned bases).
template <bool VEC_IN, bool VEC_OUT>
__global__ void __launch_bounds__(256) inpaint_noise_target_kernel(
    const bf16_t* __restrict__ mom, const bf16_t* __restrict__ mmom, const float* __restrict__ eps, const float* __restrict__ meps,
    const float* __restrict__ lmask, const float* __restrict__ noise, const float* __restrict__ offset,
    const float* __restrict__ perturb, const int* __restrict__ t, const float* __restrict__ acp, bf16_t* __restrict__ input_nhwc,
    float* __restrict__ target, float* __restrict__ lat_nchw, float* __restrict__ noisy_nchw, float* __restrict__ mlat_nchw, int B,
    int L, int HW, int mstride, int cpad, float scale, float offset_mag, float perturb_mag, int ptype) {
#pragma clang fp contract(off)
  const long total = (long)B * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float a = acp[t[b]];
    const float sa = sqrtf(a), so = sqrtf(1.0f - a);
    const float mk = repaint(lmask[i]) ? 1.0f : 0.0f;
    const bf16_t* row = mom + i * mstride;
    const bf16_t* mrow = mmom + i * mstride;
    for (int c0 = 0; c0 < cpad; c0 += 8) {
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (c0 < L) {  // noisy latents: mean columns from c0, log-variances from L + c0
        float mean[8], lv[8];
        unpack8(row_cols8<VEC_IN>(row, c0, 0, L, mstride), mean);
        unpack8(row_cols8<VEC_IN>(row, L + c0, L, 2 * L, mstride), lv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = c0 + j;
          if (c < L)
            o[j] = noise_target_element(mean[j], lv[j], eps[i * L + c], ((long)b * L + c) * HW + p, b * L + c, sa, so, noise, offset,
                                        perturb, target, lat_nchw, noisy_nchw, scale, offset_mag, perturb_mag, ptype);
        }
      }
      if (c0 + 8 > L + 1 && c0 < 2 * L + 1) {  // masked-image latents: channel c holds sample c - L - 1
        float mean[8], lv[8];
        unpack8(row_cols8<VEC_IN>(mrow, c0 - L - 1, 0, L, mstride), mean);
        unpack8(row_cols8<VEC_IN>(mrow, c0 - 1, L, 2 * L, mstride), lv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int m = c0 + j - L - 1;
          if (m >= 0 && m < L) {
            const float xm = posterior_element(mean[j], lv[j], meps[i * L + m], scale);
            o[j] = xm;
            if (mlat_nchw) mlat_nchw[((long)b * L + m) * HW + p] = xm;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j == L) o[j] = mk;
      if (VEC_OUT) {
        *reinterpret_cast<uint4*>(input_nhwc + i * cpad + c0) = pack8(o);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < cpad) input_nhwc[i * cpad + c0 + j] = f2bf(o[j]);
      }
    }
  }
}

// The sampler's UNet input from the tensor the scheduler kernels write: row r of the (doubled) batch takes channels [0,L) of its own
// latents row, the mask and the masked latents of sample r % B.  Pure bf16 moves: the values travel as 16-bit words.
template <bool VEC_IN, bool VEC_OUT>
__global__ void __launch_bounds__(256) inpaint_pack_input_kernel(const bf16_t* __restrict__ lat, const bf16_t* __restrict__ mlat,
                                                                 const float* __restrict__ lmask, bf16_t* __restrict__ out, int R,
                                                                 int B, int L, int HW, int cpad_src, int cpad_m, int cpad_dst) {
  const long total = (long)R * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / HW);
    const long q = (long)(r % B) * HW + i % HW;  // the pixel of the sample whose mask and masked latents this row takes
    const unsigned mk = repaint(lmask[q]) ? 0x3f80u : 0u;  // bf16 1.0
    const bf16_t* src = lat + i * cpad_src;
    const bf16_t* msrc = mlat + q * cpad_m;
    for (int c0 = 0; c0 < cpad_dst; c0 += 8) {
      uint4 sv = make_uint4(0u, 0u, 0u, 0u), mv = sv;
      if (c0 < L) sv = row_cols8<VEC_IN>(src, c0, 0, L, cpad_src);
      if (c0 + 8 > L + 1 && c0 < 2 * L + 1) mv = row_cols8<VEC_IN>(msrc, c0 - L - 1, 0, L, cpad_m);
      const unsigned sd[4] = {sv.x, sv.y, sv.z, sv.w}, md[4] = {mv.x, mv.y, mv.z, mv.w};
      unsigned e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        const unsigned se = (sd[j >> 1] >> (16 * (j & 1))) & 0xffffu, me = (md[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        e[j] = c < L ? se : (c == L ? mk : (c < 2 * L + 1 ? me : 0u));
      }
      if (VEC_OUT) {
        *reinterpret_cast<uint4*>(out + i * cpad_dst + c0) =
            make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < cpad_dst) out[i * cpad_dst + c0 + j] = (bf16_t)e[j];
      }
    }
  }
}

// ------------------------------------------------------------------ ControlNet injection (include/sdt.h "CONTROLNET")
// double_to_bf16_rne: sdt_common.h
__device__ __forceinline__ bf16_t control_add_element(bf16_t skip, bf16_t res, float scale) {
#pragma clang fp contract(off)
  // scale (24 bits) * res (8 bits) is exact in double; the sum rounds to double, then once to bf16
  return double_to_bf16_rne((double)bf2f(skip) + (double)scale * (double)bf2f(res));
}

// The sample of a row.  rows_per_sample <= rows, so both fit 32 bits whenever rows does, and the division is then a 32-bit one
// (64-bit integer division is emulated on CDNA); the condition is uniform over the launch.
__device__ __forceinline__ long control_sample(long r, long rows, long rows_per_sample) {
  return rows <= 0x7fffffffL ? (long)((unsigned)r / (unsigned)rows_per_sample) : r / rows_per_sample;
}

// wide (rows, Ca + Cb) = [a | skip + scale[row / rows_per_sample] * res].  Block (cx, 256 / cx): threadIdx.x walks the 16-byte chunks
// of a row, threadIdx.y and the grid walk the rows, so no index is divided by the row width; cx is a power of two >= the chunks of a
// row (at most 256), and consecutive lanes touch consecutive chunks of consecutive rows.
__global__ void __launch_bounds__(256) control_concat_add_vec_kernel(const uint4* __restrict__ a, const uint4* __restrict__ skip,
                                                                     const uint4* __restrict__ res, const float* __restrict__ scale,
                                                                     uint4* __restrict__ wide, long rows, long rows_per_sample, int Cav,
                                                                     int Cbv) {
  const int Wv = Cav + Cbv;
  for (long r = (long)blockIdx.x * blockDim.y + threadIdx.y; r < rows; r += (long)gridDim.x * blockDim.y) {
    const float s = scale ? scale[control_sample(r, rows, rows_per_sample)] : 1.f;
    for (int c = threadIdx.x; c < Wv; c += blockDim.x) {
      if (c < Cav) {
        wide[r * Wv + c] = a[r * Cav + c];
        continue;
      }
      const long j = r * Cbv + (c - Cav);
      const uint4 sv = skip[j], rv = res[j];
      const unsigned si[4] = {sv.x, sv.y, sv.z, sv.w}, ri[4] = {rv.x, rv.y, rv.z, rv.w};
      unsigned o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned lo = control_add_element((bf16_t)(si[k] & 0xffffu), (bf16_t)(ri[k] & 0xffffu), s);
        const unsigned hi = control_add_element((bf16_t)(si[k] >> 16), (bf16_t)(ri[k] >> 16), s);
        o[k] = lo | (hi << 16);
      }
      wide[r * Wv + c] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

// the same with threadIdx.x walking single elements: any widths, any 2-byte alignment
__global__ void __launch_bounds__(256) control_concat_add_scalar_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ skip,
                                                                        const bf16_t* __restrict__ res, const float* __restrict__ scale,
                                                                        bf16_t* __restrict__ wide, long rows, long rows_per_sample, int Ca,
                                                                        int Cb) {
  const int Wd = Ca + Cb;
  for (long r = (long)blockIdx.x * blockDim.y + threadIdx.y; r < rows; r += (long)gridDim.x * blockDim.y) {
    const float s = scale ? scale[control_sample(r, rows, rows_per_sample)] : 1.f;
    for (int c = threadIdx.x; c < Wd; c += blockDim.x)
      wide[r * Wd + c] = c < Ca ? a[r * Ca + c] : control_add_element(skip[r * Cb + (c - Ca)], res[r * Cb + (c - Ca)], s);
  }
}

// pred bf16 NHWC (B,h,w,cpad), target f32 NCHW (B,C,h,w), w f32 (B) or null.
// loss_sum += sum w*(t-p)^2 * inv_count ; dpred (bf16 NHWC cpad) = -2*w*(t-p)*inv_count
__global__ void __launch_bounds__(256) mse_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ target,
                                                  const float* __restrict__ w, float* __restrict__ loss,
                                                  bf16_t* __restrict__ dpred, int B, int C, int HW, int cpad,
                                                  float inv_count, int* counter, float* __restrict__ part) {
  __shared__ float scratch[16];
  __shared__ int s_last;
  const long total = (long)B * HW;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW), p = (int)(i % HW);
    const float wt = w ? w[b] : 1.f;
    for (int c = 0; c < cpad; ++c) {
      float d = 0.f;
      if (c < C) {
        const float tv = target[((long)b * C + c) * HW + p];
        const float diff = tv - bf2f(pred[i * cpad + c]);
        acc += wt * diff * diff;
        d = -2.f * wt * diff * inv_count;
      }
      if (dpred) dpred[i * cpad + c] = f2bf(d);
    }
  }
  float s = block_sum(acc, scratch);
  if (threadIdx.x == 0) sdt_store_wt(part + blockIdx.x, s);
  // the workgroup that arrives last adds the per-workgroup sums in workgroup order (no float atomics: reproducible loss)
  if (!sdt_arrive_last<true>(counter, (int)gridDim.x, &s_last)) return;
  float t = 0.f;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += sdt_load_wt(part + i);
  t = block_sum(t, scratch);
  if (threadIdx.x == 0) *loss += t * inv_count;
}

// ------------------------------------------------------------------ masked / per-sample weighted loss (include/sdt.h "MASKED LOSS")
__device__ __forceinline__ float clamp01(float m) { return fminf(fmaxf(m, 0.f), 1.f); }  // a NaN counts as 0

// mask f32 (B, h*F, w*F) -> pooled mask mp (optional) and effective mask e = fmaxf(mp, floor), f32 (B,h,w), and S[b] = sum_p e[b,p].
// Grid (nb, B): workgroup j of sample b owns the latent positions j*256 + t, + nb*256, ...; one thread per position adds the F x F
// block of clamped values in row-major order starting from +0 (so F = 1 is the clamp itself), times fl32(1 / F^2).  The sum S: each
// thread adds its positions in order, block_sum, one partial per workgroup, added in workgroup order by the one that arrives last at
// the sample's counter.  VEC: the F floats of a block row by 16-byte loads (F % 4 == 0 and a 16-byte aligned mask: every block row
// then starts on a 16-byte boundary, because the row pitch w*F is a multiple of 4 floats).
template <int F, bool VEC>
__global__ void __launch_bounds__(256) loss_mask_prepare_kernel(const float* __restrict__ mask, float floor_v, float* __restrict__ e,
                                                                float* __restrict__ mp, float* __restrict__ S, int h, int w,
                                                                int* counters, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float scratch[16];
  __shared__ int s_last;
  const int b = blockIdx.y, nb = gridDim.x, hw = h * w;
  const long Wp = (long)w * F;
  const float inv = 1.0f / (float)(F * F);
  const float* mb = mask + (long)b * hw * F * F;
  float acc = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += nb * 256) {
    const int y = p / w, x = p - y * w;
    const float* src = mb + (long)y * F * Wp + (long)x * F;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < F; ++r) {
      const float* row = src + r * Wp;
      if (VEC) {
#pragma unroll
        for (int c = 0; c < F; c += 4) {
          const float4 v = *reinterpret_cast<const float4*>(row + c);
          s += clamp01(v.x); s += clamp01(v.y); s += clamp01(v.z); s += clamp01(v.w);
        }
      } else {
#pragma unroll
        for (int c = 0; c < F; ++c) s += clamp01(row[c]);
      }
    }
    const float m = s * inv;
    const float ev = fmaxf(m, floor_v);
    const long o = (long)b * hw + p;
    if (mp) mp[o] = m;
    e[o] = ev;
    acc += ev;
  }
  const float t = block_sum(acc, scratch);
  float* pb = part + (long)b * nb;
  if (threadIdx.x == 0) sdt_store_wt(pb + blockIdx.x, t);
  if (!sdt_arrive_last<true>(counters + b, nb, &s_last)) return;
  float tot = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) tot += sdt_load_wt(pb + i);
  tot = block_sum(tot, scratch);
  if (threadIdx.x == 0) S[b] = tot;
}

// ------------------------------------------------------------------ Huber / smooth-L1 loss (include/sdt.h "ROBUST LOSS")
enum { LOSS_L2 = 0, LOSS_HUBER = 1, LOSS_SMOOTH_L1 = 2 };

// One element of the pseudo-Huber loss: g = d rho / d pred and rho from the fp32 diff = target - pred and the sample's threshold c.
// Everything between the fp32 operands and the two fp32 results is double and IEEE (add, multiply, sqrt, divide; nothing contracted):
//   dd = diff*diff and c*c are exact (24-bit factors), q = fl64(dd + c*c), r = fl64(sqrt(q)), den = fl64(r + c)
//   huber:      g = fl32(fl64((-2c * diff) / r))  (-2c * diff is exact),  rho = fl32(fl64(fl64(2c * dd) / den))
//   smooth_l1:  g = fl32(fl64((-2 * diff) / r)),                          rho = fl32(fl64((2 * dd) / den))    (2 * dd is exact)
// rho is 2c(r - c) resp. 2(r - c) without the cancellation; r == 0 (diff and c both zero) gives g = rho = 0, never 0/0.
template <int TYPE>
__device__ __forceinline__ void robust_element(float diff, float c, float& g, float& rho) {
#pragma clang fp contract(off)
  const double D = (double)diff, Cd = (double)c;
  const double dd = D * D;
  const double r = sqrt(dd + Cd * Cd);
  if (r == 0.0) {
    g = 0.f;
    rho = 0.f;
    return;
  }
  const double den = r + Cd;
  if (TYPE == LOSS_HUBER) {
    g = (float)(((-2.0 * Cd) * D) / r);
    rho = (float)(((2.0 * Cd) * dd) / den);
  } else {
    g = (float)((-2.0 * D) / r);
    rho = (float)((2.0 * dd) / den);
  }
}

// pred bf16 NHWC (B,h,w,cpad), target f32 NCHW (B,C,h,w), e f32 (B,h,w) or null (all ones), S f32 (B) or null (no normalisation),
// w1 / w2 f32 (B) or null (the min-SNR factor and the loss weight).  Grid (nb, B), the partition of loss_mask_prepare_kernel.
//   k_b = fl(fl(w1*w2) * s_b),  s_b = 1 | (S_b == 0 ? 0 : fl(fl(HW) / S_b))
//   dpred = bf16(fl(fl(fl(-2 * fl(k_b*e)) * diff) * inv_count))         (with k_b*e == 1 the chain of mse_kernel)
//   a_b   = sum e*diff*diff over the sample: per thread in order, block_sum, partials in workgroup order by the last arriver, which
//   writes loss_per_sample[b] = fl(fl(k_b*a_b) * inv_chw) and the sample's term fl(k_b*a_b); the workgroup that finishes the last sample
//   adds the B terms in sample order and adds fl(total * inv_count) to *loss.
// VEC: a position's cpad channels of pred / dpred as 16-byte vectors (cpad % 8 == 0, both aligned); padding lanes of pred are unpacked
// but never enter the arithmetic, and dpred's are written as zero.
// TYPE LOSS_HUBER / LOSS_SMOOTH_L1 (hc f32 (B): the samples' thresholds; unused by LOSS_L2): the element above in place of the square,
//   dpred = bf16(fl(fl(fl(k_b*e) * g) * inv_count)),  a_b = sum fl(e * rho); everything around the element is shared.
template <bool VEC, int TYPE>
__global__ void __launch_bounds__(256) masked_mse_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ target,
                                                         const float* __restrict__ e, const float* __restrict__ S,
                                                         const float* __restrict__ w1, const float* __restrict__ w2,
                                                         const float* __restrict__ hc, float* __restrict__ loss,
                                                         float* __restrict__ loss_ps, bf16_t* __restrict__ dpred, int B, int C, int HW,
                                                         int cpad, float inv_count, float inv_chw, int* counters,
                                                         float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float scratch[16];
  __shared__ int s_last;
  const int b = blockIdx.y, nb = gridDim.x;
  float k = (w1 ? w1[b] : 1.f) * (w2 ? w2[b] : 1.f);
  if (S) {
    const float sb = S[b];
    k = k * (sb == 0.f ? 0.f : (float)HW / sb);
  }
  const float hub = TYPE == LOSS_L2 ? 0.f : hc[b];
  const float* tb = target + (long)b * C * HW;
  float acc = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += nb * 256) {
    const long i = (long)b * HW + p;
    const float ev = e ? e[i] : 1.f;
    const float g = TYPE == LOSS_L2 ? -2.f * (k * ev) : k * ev;
    if (VEC) {
      const uint4* prow = reinterpret_cast<const uint4*>(pred + i * cpad);
      for (int c0 = 0; c0 < cpad; c0 += 8) {
        float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (c0 < C) {
          float pv[8];
          unpack8(prow[c0 >> 3], pv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (c0 + j < C) {
              const float diff = tb[(long)(c0 + j) * HW + p] - pv[j];
              if (TYPE == LOSS_L2) {
                acc += ev * diff * diff;
                d[j] = g * diff * inv_count;
              } else {
                float ge, rho;
                robust_element<TYPE>(diff, hub, ge, rho);
                acc += ev * rho;
                d[j] = g * ge * inv_count;
              }
            }
          }
        }
        if (dpred) *reinterpret_cast<uint4*>(dpred + i * cpad + c0) = pack8(d);
      }
    } else {
      for (int c = 0; c < cpad; ++c) {
        float d = 0.f;
        if (c < C) {
          const float diff = tb[(long)c * HW + p] - bf2f(pred[i * cpad + c]);
          if (TYPE == LOSS_L2) {
            acc += ev * diff * diff;
            d = g * diff * inv_count;
          } else {
            float ge, rho;
            robust_element<TYPE>(diff, hub, ge, rho);
            acc += ev * rho;
            d = g * ge * inv_count;
          }
        }
        if (dpred) dpred[i * cpad + c] = f2bf(d);
      }
    }
  }
  const float s = block_sum(acc, scratch);
  float* pb = part + (long)b * nb;   // per-workgroup partials of sample b
  float* terms = part + (long)B * nb;  // the B finished per-sample terms
  if (threadIdx.x == 0) sdt_store_wt(pb + blockIdx.x, s);
  if (!sdt_arrive_last<true>(counters + b, nb, &s_last)) return;
  float a = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) a += sdt_load_wt(pb + i);
  a = block_sum(a, scratch);
  if (threadIdx.x == 0) {
    const float term = k * a;
    loss_ps[b] = term * inv_chw;
    sdt_store_wt(terms + b, term);
  }
  // second level: the workgroup that finishes the last sample adds the samples' terms in sample order
  if (!sdt_arrive_last<true>(counters + B, B, &s_last)) return;
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < B; ++i) t += sdt_load_wt(terms + i);
    *loss += t * inv_count;
  }
}

// ------------------------------------------------------------------ Diffusion-DPO loss (include/sdt.h "DPO LOSS")
// First launch: the per-sample mean squared errors of the trained pass (pred) and the reference pass (ref), then everything per pair.
// Grid (nb, B) and the partition of masked_mse_kernel; a thread keeps two accumulators, the workgroup stores two partials (part[b*nb + j]
// trained, part[(B + b)*nb + j] reference), the last arriver of sample b adds each set in workgroup order and publishes
// sample_mse[b] = fl(a * inv_chw), sample_mse[B + b] likewise.  The workgroup that finishes the last sample evaluates the pairs - one
// thread per pair, in double from the four published fp32 values - and thread 0 adds the pair losses in pair order.
template <bool VEC>
__global__ void __launch_bounds__(256) dpo_sums_kernel(const bf16_t* __restrict__ pred, const bf16_t* __restrict__ ref,
                                                       const float* __restrict__ target, float beta, float* __restrict__ loss,
                                                       float* __restrict__ sample_mse, float* __restrict__ logits,
                                                       float* __restrict__ pair_loss, float* __restrict__ coef, int B, int C, int HW,
                                                       int cpad, float inv_chw, float inv_pairs, int* counters, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float scratch[16];
  __shared__ int s_last;
  const int b = blockIdx.y, nb = gridDim.x;
  const float* tb = target + (long)b * C * HW;
  float acc_m = 0.f, acc_r = 0.f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += nb * 256) {
    const long i = (long)b * HW + p;
    if (VEC) {
      const uint4* prow = reinterpret_cast<const uint4*>(pred + i * cpad);
      const uint4* rrow = reinterpret_cast<const uint4*>(ref + i * cpad);
      for (int c0 = 0; c0 < C; c0 += 8) {
        float pv[8], rv[8];
        unpack8(prow[c0 >> 3], pv);
        unpack8(rrow[c0 >> 3], rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (c0 + j < C) {
            const float t = tb[(long)(c0 + j) * HW + p];
            const float dm = t - pv[j], dr = t - rv[j];
            acc_m += dm * dm;
            acc_r += dr * dr;
          }
        }
      }
    } else {
      for (int c = 0; c < C; ++c) {
        const float t = tb[(long)c * HW + p];
        const float dm = t - bf2f(pred[i * cpad + c]), dr = t - bf2f(ref[i * cpad + c]);
        acc_m += dm * dm;
        acc_r += dr * dr;
      }
    }
  }
  const float sm = block_sum(acc_m, scratch);
  const float sr = block_sum(acc_r, scratch);
  float* pm = part + (long)b * nb;        // per-workgroup partials of sample b, trained pass
  float* pr = part + (long)(B + b) * nb;  // reference pass
  if (threadIdx.x == 0) {
    sdt_store_wt(pm + blockIdx.x, sm);
    sdt_store_wt(pr + blockIdx.x, sr);
  }
  if (!sdt_arrive_last<true>(counters + b, nb, &s_last)) return;
  float am = 0.f, ar = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) {
    am += sdt_load_wt(pm + i);
    ar += sdt_load_wt(pr + i);
  }
  am = block_sum(am, scratch);
  ar = block_sum(ar, scratch);
  if (threadIdx.x == 0) {
    sdt_store_wt(sample_mse + b, am * inv_chw);
    sdt_store_wt(sample_mse + B + b, ar * inv_chw);
  }
  // second level: the workgroup that finishes the last sample evaluates the pairs
  if (!sdt_arrive_last<true>(counters + B, B, &s_last)) return;
  const int P = B >> 1;
  const double bd = (double)beta, hb = -0.5 * bd;
  for (int i = threadIdx.x; i < P; i += 256) {
    const double mw = (double)sdt_load_wt(sample_mse + 2 * i), ml = (double)sdt_load_wt(sample_mse + 2 * i + 1);
    const double rw = (double)sdt_load_wt(sample_mse + B + 2 * i), rl = (double)sdt_load_wt(sample_mse + B + 2 * i + 1);
    const double dlt = (mw - ml) - (rw - rl);
    const double z = hb * dlt;
    // -logsigmoid(z) = max(-z, 0) + log1p(exp(-|z|));  s = sigmoid(-z) from the exponential of a non-positive argument
    const double e = exp(-fabs(z));
    const double pl = fmax(-z, 0.0) + log1p(e);
    const double s = z >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
    logits[i] = (float)z;
    sdt_store_wt(pair_loss + i, (float)pl);
    coef[2 * i] = (float)(-bd * s);
    coef[2 * i + 1] = (float)(bd * s);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < P; ++i) t += sdt_load_wt(pair_loss + i);
    *loss += t * inv_pairs;
  }
}

// Second launch: dpred = bf16(fl(fl(coef_b * diff) * inv_count)), diff = fl(target - pred), over the same grid and partition; padding
// channels are written as zero and the padding lanes of pred never enter the arithmetic.
template <bool VEC>
__global__ void __launch_bounds__(256) dpo_grad_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ coef, bf16_t* __restrict__ dpred, int C, int HW,
                                                       int cpad, float inv_count) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, nb = gridDim.x;
  const float k = coef[b];
  const float* tb = target + (long)b * C * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += nb * 256) {
    const long i = (long)b * HW + p;
    if (VEC) {
      const uint4* prow = reinterpret_cast<const uint4*>(pred + i * cpad);
      for (int c0 = 0; c0 < cpad; c0 += 8) {
        float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (c0 < C) {
          float pv[8];
          unpack8(prow[c0 >> 3], pv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (c0 + j < C) {
              const float diff = tb[(long)(c0 + j) * HW + p] - pv[j];
              d[j] = k * diff * inv_count;
            }
          }
        }
        *reinterpret_cast<uint4*>(dpred + i * cpad + c0) = pack8(d);
      }
    } else {
      for (int c = 0; c < cpad; ++c) {
        float d = 0.f;
        if (c < C) {
          const float diff = tb[(long)c * HW + p] - bf2f(pred[i * cpad + c]);
          d = k * diff * inv_count;
        }
        dpred[i * cpad + c] = f2bf(d);
      }
    }
  }
}

// get_sinusoidal_embeddings: out[b] = [cos(t*inv_i) | sin(t*inv_i)] (flip) or [sin|cos]
__global__ void timestep_embed_kernel(const int* __restrict__ t, bf16_t* __restrict__ out, int B, int dim,
                                      int flip_sin_to_cos, float freq_shift, float max_period) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, k = i % half;
  const float inc = logf(max_period) / ((float)half - freq_shift);
  const float e = (float)t[b] * expf((float)k * -inc);
  const float s = sinf(e), c = cosf(e);
  out[(long)b * dim + k] = f2bf(flip_sin_to_cos ? c : s);
  out[(long)b * dim + half + k] = f2bf(flip_sin_to_cos ? s : c);
}

// ------------------------------------------------------------------ activations (vectors of 8 bf16)
enum { ACT_SILU = 0, ACT_QUICK_GELU = 1, ACT_GELU_ERF = 2 };

template <int ACT>
__device__ __forceinline__ float act_fwd(float x) {
  if (ACT == ACT_SILU) return siluf_(x);
  if (ACT == ACT_QUICK_GELU) return x * sigmoidf_(1.702f * x);
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
}
template <int ACT>
__device__ __forceinline__ float act_bwd(float x, float dy) {
  if (ACT == ACT_SILU) {
    float s = sigmoidf_(x);
    return dy * s * (1.f + x * (1.f - s));
  }
  if (ACT == ACT_QUICK_GELU) {
    float s = sigmoidf_(1.702f * x);
    // |x| > 2e38: 1.702 * x overflows and inf * (1 - s) = inf * 0 (or dy * 0 * -inf) is NaN; s is exactly 0 or 1 from |x| ~ 52 on,
    // so the clamped x gives the same bits for every input that was finite before
    const float xc = fminf(fmaxf(x, -1.0e38f), 1.0e38f);
    return dy * s * (1.f + 1.702f * xc * (1.f - s));
  }
  float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
  return dy * (cdf + x * pdf);
}

template <int ACT>
__global__ void __launch_bounds__(256) act_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, long nv) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(x[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = act_fwd<ACT>(f[j]);
    y[i] = pack8(f);
  }
}
template <int ACT>
__global__ void __launch_bounds__(256) act_bwd_kernel(const uint4* __restrict__ x, const uint4* __restrict__ dy,
                                                      uint4* __restrict__ dx, long nv) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    float f[8], g[8];
    unpack8(x[i], f);
    unpack8(dy[i], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = act_bwd<ACT>(f[j], g[j]);
    dx[i] = pack8(f);
  }
}

// GEGLU: h (M, 2F) -> out (M, F) = h[:, :F] * gelu_tanh(h[:, F:])   (flax nn.gelu approximate=True)
// (gelu_tanh_f / gelu_tanh_grad: sdt_common.h - the fused feed-forward epilogues of gemm.hip evaluate the same functions)
__global__ void __launch_bounds__(256) geglu_fwd_kernel(const uint4* __restrict__ h, uint4* __restrict__ out, long M,
                                                        int Fv) {
  const long total = M * Fv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / Fv;
    const int c = (int)(i % Fv);
    float a[8], g[8];
    unpack8(h[m * 2 * Fv + c], a);
    unpack8(h[m * 2 * Fv + Fv + c], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = a[j] * gelu_tanh_f(g[j]);
    out[i] = pack8(a);
  }
}
__global__ void __launch_bounds__(256) geglu_bwd_kernel(const uint4* __restrict__ h, const uint4* __restrict__ dout,
                                                        uint4* __restrict__ dh, long M, int Fv) {
  const long total = M * Fv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / Fv;
    const int c = (int)(i % Fv);
    float a[8], g[8], d[8], da[8], dg[8];
    unpack8(h[m * 2 * Fv + c], a);
    unpack8(h[m * 2 * Fv + Fv + c], g);
    unpack8(dout[i], d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      da[j] = d[j] * gelu_tanh_f(g[j]);
      dg[j] = d[j] * a[j] * gelu_tanh_grad(g[j]);
    }
    dh[m * 2 * Fv + c] = pack8(da);
    dh[m * 2 * Fv + Fv + c] = pack8(dg);
  }
}

// ------------------------------------------------------------------ data movement
// 2-D strided copy of bf16 rows (concat / split along channels): cols % 8 == 0, strides % 8 == 0
__global__ void __launch_bounds__(256) copy2d_kernel(uint4* __restrict__ dst, long dstride_v, const uint4* __restrict__ src,
                                                     long sstride_v, long rows, int cols_v) {
  const long total = rows * cols_v;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cols_v;
    const int c = (int)(i % cols_v);
    dst[r * dstride_v + c] = src[r * sstride_v + c];
  }
}

// n column segments of a wide matrix <-> n narrow matrices, one launch (blockIdx.y = segment): channel concat / split and the
// gradient gather of column slices used to be one copy2d launch per segment
struct ColSeg {
  uint4* part[32];     // narrow matrix of segment k (nullptr when gathering: the segment is zero-filled)
  long ld_v[32];       // its row pitch (16-byte vectors)
  int col0_v[32];      // first vector column of the segment inside the wide matrix
  int cols_v[32];      // vectors per row of the segment
};
__global__ void __launch_bounds__(256) copy_cols_kernel(uint4* __restrict__ wide, long ld_wide_v, const ColSeg seg, long rows, int to_wide) {
  const int k = blockIdx.y;
  const int cv = seg.cols_v[k];
  uint4* part = seg.part[k];
  const long ldp = seg.ld_v[k];
  uint4* w0 = wide + seg.col0_v[k];
  const long total = rows * cv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cv;
    const int c = (int)(i - r * cv);
    if (to_wide) w0[r * ld_wide_v + c] = part ? part[r * ldp + c] : make_uint4(0, 0, 0, 0);
    else part[r * ldp + c] = w0[r * ld_wide_v + c];
  }
}

__global__ void __launch_bounds__(256) add_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                  uint4* __restrict__ y, long nv) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    float f[8], g[8];
    unpack8(a[i], f);
    unpack8(b[i], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] += g[j];
    y[i] = pack8(f);
  }
}

// nearest 2x upsample NHWC: out (B,2H,2W,C) ; backward: din (B,H,W,C) = sum of the 2x2 outputs
__global__ void __launch_bounds__(256) upsample2x_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, int B,
                                                             int H, int W, int Cv) {
  const long total = (long)B * 2 * H * 2 * W * Cv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cv);
    long r = i / Cv;
    const int ox = (int)(r % (2 * W));
    r /= (2 * W);
    const int oy = (int)(r % (2 * H));
    const int b = (int)(r / (2 * H));
    y[i] = x[(((long)b * H + (oy >> 1)) * W + (ox >> 1)) * Cv + c];
  }
}
__global__ void __launch_bounds__(256) upsample2x_bwd_kernel(const uint4* __restrict__ dy, uint4* __restrict__ dx, int B,
                                                             int H, int W, int Cv) {
  const long total = (long)B * H * W * Cv;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cv);
    long r = i / Cv;
    const int x = (int)(r % W);
    r /= W;
    const int y = (int)(r % H);
    const int b = (int)(r / H);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, f[8];
#pragma unroll
    for (int dyy = 0; dyy < 2; ++dyy)
#pragma unroll
      for (int dxx = 0; dxx < 2; ++dxx) {
        unpack8(dy[(((long)b * 2 * H + 2 * y + dyy) * 2 * W + 2 * x + dxx) * Cv + c], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    dx[i] = pack8(acc);
  }
}

// f32 NCHW (B,C,H,W) -> bf16 NHWC (B,H,W,cpad) zero padded
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int B,
                                                           int C, int HW, int cpad) {
  const long total = (long)B * HW * cpad;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cpad);
    const long bp = i / cpad;
    const int b = (int)(bp / HW), p = (int)(bp % HW);
    y[i] = (c < C) ? f2bf(x[((long)b * C + c) * HW + p]) : (bf16_t)0;
  }
}
// bf16 NHWC (B,H,W,cpad) -> f32 NCHW (B,C,H,W)
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, int B,
                                                           int C, int HW, int cpad) {
  const long total = (long)B * C * HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const long bc = i / HW;
    const int b = (int)(bc / C), c = (int)(bc % C);
    y[i] = bf2f(x[((long)b * HW + p) * cpad + c]);
  }
}

__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = f2bf(x[i]);
}

// batched bf16 transpose (batch, R, C) -> (batch, C, R) through a 64x64 LDS tile
__global__ void __launch_bounds__(256) transpose_bf16_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int R,
                                                             int C) {
  __shared__ bf16_t tile[64][66];
  const long base = (long)blockIdx.z * R * C;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int r = i >> 6, c = i & 63;
    tile[r][c] = (r0 + r < R && c0 + c < C) ? x[base + (long)(r0 + r) * C + c0 + c] : (bf16_t)0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int c = i >> 6, r = i & 63;
    if (r0 + r < R && c0 + c < C) y[base + (long)(c0 + c) * R + r0 + r] = tile[r][c];
  }
}

// Parameter preparation: one launch per model.  For every matrix-shaped leaf ([batch][R][C] in Flax layout: Dense batch=1
// R=in C=out; conv HWIO batch=kh*kw R=Cin C=Cout) produce the bf16 compute copy W (same layout, zero-padded to Rp x Cp) from
// the fp32 master.  Every contraction reads W as it stands (forward: k-major operand through transposing LDS reads; input
// gradient: row-major operand), so no transposed copy exists; Wt != NULL additionally writes [batch][Cp][Rp] (kept for
// callers that want it).  Per step only the few zero-padded leaves pass through here: the optimizer sweep itself mirrors
// the master into W (sdt_lion8_step / sdt_lion32_step w_bf16) for all the others.
struct SdtPrepDesc {
  long src_off, w_off, wt_off;  // element offsets into master / W / Wt flat buffers
  int batch, R, C, Rp, Cp;      // logical and padded dims
  int tile0;                    // first 64x64 tile index of this leaf in the launch
  int flags;                    // reserved (0)
};
__global__ void __launch_bounds__(256) param_prepare_kernel(const float* __restrict__ master, bf16_t* __restrict__ W,
                                                            bf16_t* __restrict__ Wt, const SdtPrepDesc* __restrict__ descs,
                                                            int ndesc) {
  __shared__ bf16_t tile[64][66];
  const int tile_id = blockIdx.x;
  int lo = 0, hi = ndesc - 1;
  while (lo < hi) {  // last desc with tile0 <= tile_id
    int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile0 <= tile_id) lo = mid; else hi = mid - 1;
  }
  const SdtPrepDesc d = descs[lo];
  int tl = tile_id - d.tile0;
  const int tc = (d.Cp + 63) >> 6, tr = (d.Rp + 63) >> 6;
  const int bz = tl / (tc * tr);
  tl -= bz * tc * tr;
  const int r0 = (tl / tc) * 64, c0 = (tl % tc) * 64;
  const float* src = master + d.src_off + (long)bz * d.R * d.C;
  bf16_t* w = W + d.w_off + (long)bz * d.Rp * d.Cp;
  bf16_t* wt = Wt ? Wt + d.wt_off + (long)bz * d.Rp * d.Cp : nullptr;
  // interior tiles of leaves whose dims are multiples of 4 (every large kernel): 16-byte loads, 8-byte stores
  const bool vec = r0 + 64 <= d.R && c0 + 64 <= d.C && (d.C & 3) == 0 && (d.Cp & 3) == 0 && (d.Rp & 3) == 0 && (d.R & 3) == 0 &&
                   ((d.src_off | d.w_off | d.wt_off) & 3) == 0;
  if (vec) {
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = ps * 16 + (threadIdx.x >> 4), c = (threadIdx.x & 15) * 4;
      const float4 f = *reinterpret_cast<const float4*>(src + (long)(r0 + r) * d.C + c0 + c);
      uint2 pk;
      pk.x = pack2bf(f.x, f.y);
      pk.y = pack2bf(f.z, f.w);
      *reinterpret_cast<uint2*>(w + (long)(r0 + r) * d.Cp + c0 + c) = pk;
      tile[r][c] = (bf16_t)(pk.x & 0xffffu); tile[r][c + 1] = (bf16_t)(pk.x >> 16);
      tile[r][c + 2] = (bf16_t)(pk.y & 0xffffu); tile[r][c + 3] = (bf16_t)(pk.y >> 16);
    }
    if (!wt) return;  // (wave-uniform: a kernel argument)
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int c = ps * 16 + (threadIdx.x >> 4), r = (threadIdx.x & 15) * 4;
      uint2 pk;
      pk.x = (unsigned)(unsigned short)tile[r][c] | ((unsigned)(unsigned short)tile[r + 1][c] << 16);
      pk.y = (unsigned)(unsigned short)tile[r + 2][c] | ((unsigned)(unsigned short)tile[r + 3][c] << 16);
      *reinterpret_cast<uint2*>(wt + (long)(c0 + c) * d.Rp + r0 + r) = pk;
    }
    return;
  }
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int r = i >> 6, c = i & 63;
    bf16_t v = 0;
    if (r0 + r < d.R && c0 + c < d.C) v = f2bf(src[(long)(r0 + r) * d.C + c0 + c]);
    tile[r][c] = v;
    if (r0 + r < d.Rp && c0 + c < d.Cp) w[(long)(r0 + r) * d.Cp + c0 + c] = v;
  }
  if (!wt) return;
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int c = i >> 6, r = i & 63;
    if (r0 + r < d.Rp && c0 + c < d.Cp) wt[(long)(c0 + c) * d.Rp + r0 + r] = tile[r][c];
  }
}

// CLIP embeddings: out[row] = tok[ids[row]] + pos[row % S]  (bf16 out, fp32 tables)
__global__ void __launch_bounds__(256) embedding_fwd_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                            const float* __restrict__ pos, bf16_t* __restrict__ out,
                                                            long rows, int S, int D) {
  const long total = rows * D;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / D;
    const int c = (int)(i % D);
    out[i] = f2bf(tok[(long)ids[r] * D + c] + pos[(long)(r % S) * D + c]);
  }
}
// Gather form, one writer per element (no atomics): workgroup r < rows owns token row ids[r] IF r is the first row carrying that
// id, and adds the gradients of every row with the same id in row order; workgroup rows + s owns position row s and adds the
// rows r = s, s + S, ... in order.
__global__ void __launch_bounds__(256) embedding_bwd_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ dout,
                                                            float* __restrict__ dtok, float* __restrict__ dpos, long rows,
                                                            int S, int D) {
  const long blk = blockIdx.x;
  if (blk >= rows) {
    const long s0 = blk - rows;
    for (int c = threadIdx.x; c < D; c += 256) {
      float g = 0.f;
      for (long r = s0; r < rows; r += S) g += bf2f(dout[r * D + c]);
      dpos[s0 * D + c] += g;
    }
    return;
  }
  const int id = ids[blk];
  int dup = 0;
  for (long j = threadIdx.x; j < blk; j += 256) dup |= ids[j] == id;
  if (__syncthreads_or(dup)) return;  // an earlier row owns this token
  for (int c = threadIdx.x; c < D; c += 256) {
    float g = 0.f;
    for (long j = blk; j < rows; ++j)
      if (ids[j] == id) g += bf2f(dout[j * D + c]);
    dtok[(long)id * D + c] += g;
  }
}

// ---- new tokens (textual inversion; include/sdt.h "NEW TOKENS"): the token table continued by a few trained rows `ext`
// The row an id selects: tok[id] for 0 <= id < V, ext[id - V] for V <= id < V + n_ext, nullptr (a row of +0.0) for every other
// id - nothing is ever read outside the two tables.
__device__ __forceinline__ const float* embedding_ext_row(int id, const float* tok, const float* ext, int D, int V, int n_ext) {
  if (id >= 0 && id < V) return tok + (long)id * D;
  const long e = (long)id - V;
  if (e >= 0 && e < n_ext) return ext + e * D;
  return nullptr;
}
// VEC: 4 columns per lane - 16-byte table loads, one 8-byte store (D % 4 == 0, bases aligned: the host decides); else a column per lane.
template <bool VEC>
__global__ void __launch_bounds__(256) embedding_ext_fwd_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                                const float* __restrict__ ext, const float* __restrict__ pos,
                                                                bf16_t* __restrict__ out, long rows, int S, int D, int V, int n_ext) {
  if (VEC) {
    const int dv = D >> 2;
    const long total = rows * dv;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long r = i / dv;
      const int c = (int)(i % dv) << 2;
      const float* t = embedding_ext_row(ids[r], tok, ext, D, V, n_ext);
      const float4 a = t ? *reinterpret_cast<const float4*>(t + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 p = *reinterpret_cast<const float4*>(pos + (long)(r % S) * D + c);
      uint2 o;
      o.x = (unsigned)f2bf(a.x + p.x) | ((unsigned)f2bf(a.y + p.y) << 16);
      o.y = (unsigned)f2bf(a.z + p.z) | ((unsigned)f2bf(a.w + p.w) << 16);
      *reinterpret_cast<uint2*>(out + r * D + c) = o;
    }
  } else {
    const long total = rows * D;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
      const long r = i / D;
      const int c = (int)(i % D);
      const float* t = embedding_ext_row(ids[r], tok, ext, D, V, n_ext);
      out[i] = f2bf((t ? t[c] : 0.f) + pos[(long)(r % S) * D + c]);
    }
  }
}
// Workgroup (j, y) owns columns [256 y, 256 y + 256) of new token j: every lane walks the rows in increasing order - ids[r] is the same
// address for the whole wave (a uniform load) - and adds the rows that carry id V + j to a sum that starts at +0; the sum is written.
__global__ void __launch_bounds__(256) embedding_ext_bwd_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ dout,
                                                                float* __restrict__ dext, long rows, int D, int V) {
  const int j = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  const long want = (long)V + j;
  if (c >= D) return;
  float g = 0.f;
  for (long r = 0; r < rows; ++r)
    if ((long)ids[r] == want) g += bf2f(dout[r * D + c]);
  dext[(long)j * D + c] = g;
}
// One workgroup: mean and unbiased standard deviation of the n values in double, two passes, thread t owns t, t + 256, ... in
// increasing order, then a block tree (256 -> 1, stride halving); every element is then scaled by the fp32 factor.
__device__ __forceinline__ double block_tree_sum_256(double v, double* sm) {
  const int t = threadIdx.x;
  __syncthreads();  // (sm may still be read from the previous sum)
  sm[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sm[t] += sm[t + s];
    __syncthreads();
  }
  return sm[0];
}
__global__ void __launch_bounds__(256) embedding_retract_kernel(float* __restrict__ ext, long n, double target_std, double power,
                                                                double* __restrict__ stats) {
  __shared__ double sm[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += (double)ext[i];
  const double mean = block_tree_sum_256(s, sm) / (double)n;
  double q = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    const double d = (double)ext[i] - mean;
    q += d * d;
  }
  const double ss = block_tree_sum_256(q, sm);
  const double sd = n > 1 ? sqrt(ss / (double)(n - 1)) : 0.0;
  const float factor = sd == 0.0 ? 1.0f : (float)pow(target_std / sd, power);
  for (long i = threadIdx.x; i < n; i += 256) ext[i] = ext[i] * factor;
  if (threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = (double)factor;
  }
}

// column sums: out[b][n] (+)= sum over the rows of batch slice b of dy[m][n].  Workgroup (x, y, z) sums rows_per_block rows of 256
// columns of slice z into its own partial row; the workgroup that arrives last at (x, z) adds the partial rows in y order (no
// float atomics) and writes the result: += into the fp32 db, or rounded into the bf16 out_bf (the per-image row-bias gradient).
// The workgroup (bx, by, bz) of a (gx, gy, batch) grid: the single launch takes them from its grid, the grouped one from its table.
__device__ __forceinline__ void colsum_body(const bf16_t* __restrict__ dy, float* __restrict__ db, bf16_t* __restrict__ out_bf, long M, int N,
                                            int ld, int rows_per_block, long batch_stride_dy, int batch_stride_db, int* counters,
                                            float* __restrict__ part, const int bx, const int by, const int bz, const int gx, const int gy) {
  dy += (long)bz * batch_stride_dy;
  // thread (tx = column-vector of 8, ty = row lane); blockDim = 256 = 32 x 8
  __shared__ float red[8][32][8];
  __shared__ int s_last;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int cv = bx * 32 + tx;
  const long m0 = (long)by * rows_per_block;
  const long m1 = (m0 + rows_per_block < M) ? m0 + rows_per_block : M;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (cv * 8 < N) {
    for (long m = m0 + ty; m < m1; m += 8) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(dy + m * ld + cv * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ty][tx][j] = acc[j];
  __syncthreads();
  const int group = bz * gx + bx;
  float* grp = part + (long)group * gy * 256;
  {
    const int col = threadIdx.x;  // 256 columns of this workgroup
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += red[k][col >> 3][col & 7];
    sdt_store_wt(grp + (long)by * 256 + col, sum);
  }
  if (!sdt_arrive_last<true>(counters + group, gy, &s_last)) return;
  const int n = bx * 256 + threadIdx.x;
  if (n < N) {
    float t = 0.f;
    for (int y = 0; y < gy; ++y) t += sdt_load_wt(grp + (long)y * 256 + threadIdx.x);
    if (out_bf) out_bf[(long)bz * batch_stride_db + n] = f2bf(t);
    else db[(long)bz * batch_stride_db + n] += t;
  }
}
__global__ void __launch_bounds__(256) colsum_kernel(const bf16_t* __restrict__ dy, float* __restrict__ db, bf16_t* __restrict__ out_bf,
                                                     long M, int N, int ld, int rows_per_block, long batch_stride_dy,
                                                     int batch_stride_db, int* counters, float* __restrict__ part) {
  colsum_body(dy, db, out_bf, M, N, ld, rows_per_block, batch_stride_dy, batch_stride_db, counters, part, (int)blockIdx.x, (int)blockIdx.y,
              (int)blockIdx.z, (int)gridDim.x, (int)gridDim.y);
}

// Several per-image column sums (sdt_colsum_batched_group) as one launch: the row-bias gradients of the ResBlocks are read only at
// the end of the UNet backward, and one alone is a 12 us launch.  Workgroups in order (problem, image, row block, column block);
// wg_end is the prefix table.  Each problem has its own counters and partial rows in the shared workspace and keeps the grid of its
// single launch, so its sums are added in the same order.
#define COLSUM_GROUP_MAX 32
struct ColsumGroupItem {
  const bf16_t* dy;
  bf16_t* out;
  long M;
  int N, ld, rows_per_block, gx, gy;
  int counter0;  // first counter of the problem
  long part0;    // first partial-sum float of the problem
};
struct ColsumGroupParams {
  int n;
  int wg_end[COLSUM_GROUP_MAX];
  ColsumGroupItem item[COLSUM_GROUP_MAX];
};
static_assert(sizeof(ColsumGroupParams) <= 4096, "the grouped column-sum launch passes its problem table as kernel arguments");
__global__ void __launch_bounds__(256) colsum_group_kernel(const ColsumGroupParams gp, int* counters, float* __restrict__ part) {
  const int blk = blockIdx.x;
  int i = 0;
  while (i + 1 < gp.n && blk >= gp.wg_end[i]) ++i;  // wave-uniform scalar walk
  const int local = blk - (i ? gp.wg_end[i - 1] : 0);
  const ColsumGroupItem it = gp.item[i];
  const int bx = local % it.gx, rest = local / it.gx;
  const int by = rest % it.gy, bz = rest / it.gy;
  colsum_body(it.dy, nullptr, it.out, it.M, it.N, it.ld, it.rows_per_block, it.M * it.ld, it.N, counters + it.counter0, part + it.part0, bx, by,
              bz, it.gx, it.gy);
}

// row bias gradient for the temb broadcast add: dt[b][n] = sum_{m in batch b} dy[m][n]  -> bf16 (B, N)
// (done with colsum per batch slice on the host side)

// in-place row softmax over bf16 rows of length n (fp32 math); one block per row
__global__ void __launch_bounds__(256) softmax_rows_kernel(bf16_t* __restrict__ x, int n, float scale) {
  __shared__ float scratch[16];
  bf16_t* row = x + (long)blockIdx.x * n;
  float mx = -3.0e38f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, bf2f(row[i]) * scale);
  mx = wave_max(mx);
  {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) scratch[w] = mx;
    __syncthreads();
    mx = scratch[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) mx = fmaxf(mx, scratch[i]);
  }
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += __expf(bf2f(row[i]) * scale - mx);
  s = block_sum(s, scratch);
  const float inv = 1.f / s;
  for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] = f2bf(__expf(bf2f(row[i]) * scale - mx) * inv);
}

// ================================================================== C ABI
// out = sum of n (<= 32) bf16 tensors, accumulated in fp32 in argument order (the autograd engine's chain of
// binary adds rounds to bf16 after every add; one pass keeps fp32 until the end)
struct SumPtrs { const uint4* p[32]; };
__global__ void __launch_bounds__(256) sum_n_kernel(const SumPtrs ptrs, uint4* __restrict__ out, int n, long nvec) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
    float acc[8], f[8];
    unpack8(ptrs.p[0][i], acc);
    for (int k = 1; k < n; ++k) {
      unpack8(ptrs.p[k][i], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
    out[i] = pack8(acc);
  }
}


// Zero a list of float ranges of one buffer in one launch: the gradient leaves that are ACCUMULATED into (norm scales and
// biases, embeddings); weight and bias gradients of Dense / conv layers are written whole by sdt_gemm_tn_wgrad and need none.
// ranges: device int64 pairs (first float4 index, float4 count), each at most ZR_CHUNK float4s (the host splits longer ones).
#define ZR_CHUNK 4096
__global__ void __launch_bounds__(256) zero_ranges_kernel(float4* __restrict__ base, const long* __restrict__ ranges) {
  const long first = ranges[2 * blockIdx.x], count = ranges[2 * blockIdx.x + 1];
  for (long i = threadIdx.x; i < count; i += 256) base[first + i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

/* Workgroups per sample of the two masked-loss kernels: one per 256 latent positions, at most MASKED_MAX_BLOCKS, and few enough that
 * the B * nb partials and the B per-sample terms fit the 64 KiB scratch of sdt_reduce_workspace_bytes() (B <= MASKED_MAX_B). */
#define MASKED_MAX_BLOCKS 128
#define MASKED_MAX_B 8192
static int masked_blocks(int B, long hw) {
  long nb = (hw + 255) / 256, fit = (65536 / (long)sizeof(float) - B) / B;
  if (nb > MASKED_MAX_BLOCKS) nb = MASKED_MAX_BLOCKS;
  if (nb > fit) nb = fit;
  return (int)(nb < 1 ? 1 : nb);
}

template <int F>
static void loss_mask_prepare_launch(bool vec, dim3 grid, hipStream_t stream, const float* mask, float floor_v, float* e, float* mp,
                                     float* S, int h, int w, int* counters, float* part) {
  if (vec) hipLaunchKernelGGL((loss_mask_prepare_kernel<F, (F >= 4)>), grid, dim3(256), 0, stream, mask, floor_v, e, mp, S, h, w, counters, part);
  else hipLaunchKernelGGL((loss_mask_prepare_kernel<F, false>), grid, dim3(256), 0, stream, mask, floor_v, e, mp, S, h, w, counters, part);
}

extern "C" {

int sdt_add_noise_velocity(const float* latents, const float* noise, const int32_t* timesteps,
                           const float* alphas_cumprod, uint16_t* noisy_nhwc_bf16, float* noisy_nchw,
                           float* velocity_nchw, int B, int C, int H, int W, int cpad, hipStream_t stream) {
  SDT_CHECK_ARG(latents && noise && timesteps && alphas_cumprod && noisy_nhwc_bf16, "sdt_add_noise_velocity: null pointer");
  SDT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C, "sdt_add_noise_velocity: bad shape B=%d C=%d H=%d W=%d cpad=%d", B, C, H, W, cpad);
  hipLaunchKernelGGL(add_noise_kernel, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, latents, noise,
                     timesteps, alphas_cumprod, (bf16_t*)noisy_nhwc_bf16, noisy_nchw, velocity_nchw, B, C, H * W, cpad);
  SDT_LAUNCH_CHECK("sdt_add_noise_velocity");
  return SDT_OK;
}

int sdt_ddim_cfg_step(const uint16_t* pred_nhwc, float* latents_nchw, uint16_t* next_input_nhwc, int B, int C, int H, int W,
                      int cpad, float guidance_scale, float alpha_prod_t, float alpha_prod_prev, int prediction_type,
                      hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && latents_nchw && next_input_nhwc, "sdt_ddim_cfg_step: null pointer");
  SDT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C, "sdt_ddim_cfg_step: bad shape B=%d C=%d H=%d W=%d cpad=%d", B, C, H, W, cpad);
  SDT_CHECK_ARG(prediction_type >= 0 && prediction_type <= 2, "sdt_ddim_cfg_step: prediction_type %d (0 epsilon, 1 sample, 2 v_prediction)", prediction_type);
  SDT_CHECK_ARG(alpha_prod_t > 0.f && alpha_prod_t <= 1.f && alpha_prod_prev > 0.f && alpha_prod_prev <= 1.f,
                "sdt_ddim_cfg_step: alpha products must lie in (0, 1]");
  hipLaunchKernelGGL(ddim_cfg_step_kernel, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, (const bf16_t*)pred_nhwc,
                     latents_nchw, (bf16_t*)next_input_nhwc, B, C, H * W, cpad, guidance_scale, sqrtf(alpha_prod_t),
                     sqrtf(1.0f - alpha_prod_t), sqrtf(alpha_prod_prev), sqrtf(1.0f - alpha_prod_prev), prediction_type);
  SDT_LAUNCH_CHECK("sdt_ddim_cfg_step");
  return SDT_OK;
}

int sdt_cfg_rescale_factors(const uint16_t* pred_nhwc, float* factors, int B, int C, int H, int W, int cpad, float guidance_scale,
                            float guidance_rescale, hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && factors, "sdt_cfg_rescale_factors: null pointer");
  SDT_CHECK_ARG(((uintptr_t)pred_nhwc & 15) == 0, "sdt_cfg_rescale_factors: pred_nhwc misaligned (16 bytes)");
  SDT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C && cpad % 8 == 0 && (long)C * H * W >= 2,
                "sdt_cfg_rescale_factors: bad shape B=%d C=%d H=%d W=%d cpad=%d (cpad a multiple of 8, C*H*W >= 2)", B, C, H, W, cpad);
  SDT_CHECK_ARG(guidance_rescale >= 0.f && guidance_rescale <= 1.f && std::isfinite(guidance_scale),
                "sdt_cfg_rescale_factors: guidance_rescale %g must lie in [0, 1], guidance_scale finite", guidance_rescale);
  hipLaunchKernelGGL(cfg_rescale_factors_kernel, dim3(B), dim3(256), 0, stream, (const uint4*)pred_nhwc, factors, B, C, H * W, cpad,
                     guidance_scale, guidance_rescale);
  SDT_LAUNCH_CHECK("sdt_cfg_rescale_factors");
  return SDT_OK;
}

int sdt_sampler_cfg_step(const uint16_t* pred_nhwc, float* latents_nchw, uint16_t* next_input_nhwc, float* x0_history_nchw,
                         const float* rescale_factors, int B, int C, int H, int W, int cpad, float guidance_scale, float alpha_s,
                         float sigma_s, int prediction_type, float c_x, float c_x0, float c_eps, float c_d1, hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && latents_nchw && next_input_nhwc, "sdt_sampler_cfg_step: null pointer");
  SDT_CHECK_ARG((((uintptr_t)pred_nhwc | (uintptr_t)next_input_nhwc) & 15) == 0, "sdt_sampler_cfg_step: pred / next input misaligned (16 bytes)");
  SDT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C && cpad % 8 == 0,
                "sdt_sampler_cfg_step: bad shape B=%d C=%d H=%d W=%d cpad=%d (cpad a multiple of 8)", B, C, H, W, cpad);
  SDT_CHECK_ARG(prediction_type >= 0 && prediction_type <= 2, "sdt_sampler_cfg_step: prediction_type %d (0 epsilon, 1 sample, 2 v_prediction)", prediction_type);
  SDT_CHECK_ARG(alpha_s >= 0.f && alpha_s <= 1.f && sigma_s >= 0.f && sigma_s <= 1.f, "sdt_sampler_cfg_step: alpha_s / sigma_s must lie in [0, 1]");
  SDT_CHECK_ARG(!(prediction_type == 0 && alpha_s == 0.f) && !(prediction_type == 1 && sigma_s == 0.f),
                "sdt_sampler_cfg_step: %s prediction needs %s > 0", prediction_type == 0 ? "epsilon" : "sample",
                prediction_type == 0 ? "alpha_s" : "sigma_s");
  SDT_CHECK_ARG(std::isfinite(guidance_scale) && std::isfinite(c_x) && std::isfinite(c_x0) && std::isfinite(c_eps) && std::isfinite(c_d1),
                "sdt_sampler_cfg_step: guidance scale and coefficients must be finite");
  SDT_CHECK_ARG(c_d1 == 0.f || x0_history_nchw, "sdt_sampler_cfg_step: c_d1 != 0 needs the x0 history");
  hipLaunchKernelGGL(sampler_cfg_step_kernel, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, (const uint4*)pred_nhwc,
                     latents_nchw, (uint4*)next_input_nhwc, x0_history_nchw, rescale_factors, B, C, H * W, cpad, guidance_scale,
                     alpha_s, sigma_s, prediction_type, c_x, c_x0, c_eps, c_d1);
  SDT_LAUNCH_CHECK("sdt_sampler_cfg_step");
  return SDT_OK;
}

int sdt_vae_posterior_sample(const uint16_t* moments_nhwc, const float* eps_nhwc, float* latents_nchw, int B, int L,
                             int H, int W, int moment_stride, float scale, hipStream_t stream) {
  SDT_CHECK_ARG(moments_nhwc && eps_nhwc && latents_nchw && B > 0 && L > 0 && moment_stride >= 2 * L,
                "sdt_vae_posterior_sample: bad args");
  hipLaunchKernelGGL(posterior_sample_kernel, dim3(sdt_grid_1d((long)B * H * W * L, 256)), dim3(256), 0, stream,
                     (const bf16_t*)moments_nhwc, eps_nhwc, latents_nchw, B, L, H * W, moment_stride, scale);
  SDT_LAUNCH_CHECK("sdt_vae_posterior_sample");
  return SDT_OK;
}

int sdt_latent_noise_target(const uint16_t* moments_nhwc, const float* eps_nhwc, const float* noise_nchw, const float* offset,
                            const float* perturb_nchw, const int32_t* timesteps, const float* alphas_cumprod,
                            uint16_t* noisy_nhwc_bf16, float* target_nchw, float* latents_nchw, float* noisy_nchw, int B, int L,
                            int H, int W, int moment_stride, int cpad, float scale, float offset_mag, float perturb_mag,
                            int prediction_type, hipStream_t stream) {
  SDT_CHECK_ARG(moments_nhwc && eps_nhwc && noise_nchw && timesteps && alphas_cumprod && noisy_nhwc_bf16,
                "sdt_latent_noise_target: null pointer");
  SDT_CHECK_ARG(B > 0 && L > 0 && H > 0 && W > 0 && cpad >= L && moment_stride >= 2 * L,
                "sdt_latent_noise_target: bad shape B=%d L=%d H=%d W=%d moment_stride=%d cpad=%d (cpad >= L, moment_stride >= 2L)", B, L,
                H, W, moment_stride, cpad);
  SDT_CHECK_ARG(prediction_type == 0 || prediction_type == 2,
                "sdt_latent_noise_target: prediction_type %d (0 epsilon, 2 v_prediction)", prediction_type);
  SDT_CHECK_ARG(offset || offset_mag == 0.f, "sdt_latent_noise_target: offset_mag %g needs the offset noise", offset_mag);
  SDT_CHECK_ARG(perturb_nchw || perturb_mag == 0.f, "sdt_latent_noise_target: perturb_mag %g needs the perturbation noise", perturb_mag);
  SDT_CHECK_ARG(target_nchw || (prediction_type == 0 && !offset && !perturb_nchw),
                "sdt_latent_noise_target: the target may be NULL only for epsilon without offset or perturbation noise (it is the noise)");
  const bool vin = moment_stride % 8 == 0 && L % 4 == 0 && ((uintptr_t)moments_nhwc & 15) == 0;
  const bool vout = cpad % 8 == 0 && ((uintptr_t)noisy_nhwc_bf16 & 15) == 0;
  auto kern = vin ? (vout ? latent_noise_target_kernel<true, true> : latent_noise_target_kernel<true, false>)
                  : (vout ? latent_noise_target_kernel<false, true> : latent_noise_target_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, (const bf16_t*)moments_nhwc, eps_nhwc,
                     noise_nchw, offset, perturb_nchw, timesteps, alphas_cumprod, (bf16_t*)noisy_nhwc_bf16, target_nchw, latents_nchw,
                     noisy_nchw, B, L, H * W, moment_stride, cpad, scale, offset_mag, perturb_mag, prediction_type);
  SDT_LAUNCH_CHECK("sdt_latent_noise_target");
  return SDT_OK;
}

int sdt_inpaint_mask_pixels(const float* pixels_nchw, const float* mask, uint16_t* stacked_nhwc_bf16, float* latent_mask, int B,
                            int C, int H, int W, int cpad, int f, hipStream_t stream) {
  SDT_CHECK_ARG(pixels_nchw && mask && stacked_nhwc_bf16 && latent_mask, "sdt_inpaint_mask_pixels: null pointer");
  SDT_CHECK_ARG(f >= 1, "sdt_inpaint_mask_pixels: f=%d must be at least 1", f);
  SDT_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && cpad >= C, "sdt_inpaint_mask_pixels: bad shape B=%d C=%d H=%d W=%d cpad=%d (cpad >= C)",
                B, C, H, W, cpad);
  SDT_CHECK_ARG(H % f == 0 && W % f == 0, "sdt_inpaint_mask_pixels: H=%d and W=%d must be multiples of f=%d", H, W, f);
  const bool vec = cpad % 8 == 0 && ((uintptr_t)stacked_nhwc_bf16 & 15) == 0;
  auto kern = vec ? inpaint_mask_pixels_kernel<true> : inpaint_mask_pixels_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, pixels_nchw, mask,
                     (bf16_t*)stacked_nhwc_bf16, latent_mask, B, C, H, W, cpad, f);
  SDT_LAUNCH_CHECK("sdt_inpaint_mask_pixels");
  return SDT_OK;
}

int sdt_inpaint_noise_target(const uint16_t* moments_nhwc, const uint16_t* masked_moments_nhwc, const float* eps_nhwc,
                             const float* masked_eps_nhwc, const float* latent_mask, const float* noise_nchw, const float* offset,
                             const float* perturb_nchw, const int32_t* timesteps, const float* alphas_cumprod,
                             uint16_t* input_nhwc_bf16, float* target_nchw, float* latents_nchw, float* noisy_nchw,
                             float* masked_latents_nchw, int B, int L, int H, int W, int moment_stride, int cpad, float scale,
                             float offset_mag, float perturb_mag, int prediction_type, hipStream_t stream) {
  SDT_CHECK_ARG(moments_nhwc && masked_moments_nhwc && eps_nhwc && masked_eps_nhwc && latent_mask && noise_nchw && timesteps &&
                    alphas_cumprod && input_nhwc_bf16,
                "sdt_inpaint_noise_target: null pointer");
  SDT_CHECK_ARG(B > 0 && L > 0 && H > 0 && W > 0 && cpad >= 2 * L + 1 && moment_stride >= 2 * L,
                "sdt_inpaint_noise_target: bad shape B=%d L=%d H=%d W=%d moment_stride=%d cpad=%d (cpad >= 2L+1, moment_stride >= 2L)",
                B, L, H, W, moment_stride, cpad);
  SDT_CHECK_ARG(prediction_type == 0 || prediction_type == 2,
                "sdt_inpaint_noise_target: prediction_type %d (0 epsilon, 2 v_prediction)", prediction_type);
  SDT_CHECK_ARG(offset || offset_mag == 0.f, "sdt_inpaint_noise_target: offset_mag %g needs the offset noise", offset_mag);
  SDT_CHECK_ARG(perturb_nchw || perturb_mag == 0.f, "sdt_inpaint_noise_target: perturb_mag %g needs the perturbation noise", perturb_mag);
  SDT_CHECK_ARG(target_nchw || (prediction_type == 0 && !offset && !perturb_nchw),
                "sdt_inpaint_noise_target: the target may be NULL only for epsilon without offset or perturbation noise (it is the noise)");
  const bool vin = moment_stride % 8 == 0 && (((uintptr_t)moments_nhwc | (uintptr_t)masked_moments_nhwc) & 15) == 0;
  const bool vout = cpad % 8 == 0 && ((uintptr_t)input_nhwc_bf16 & 15) == 0;
  auto kern = vin ? (vout ? inpaint_noise_target_kernel<true, true> : inpaint_noise_target_kernel<true, false>)
                  : (vout ? inpaint_noise_target_kernel<false, true> : inpaint_noise_target_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(sdt_grid_1d((long)B * H * W, 256)), dim3(256), 0, stream, (const bf16_t*)moments_nhwc,
                     (const bf16_t*)masked_moments_nhwc, eps_nhwc, masked_eps_nhwc, latent_mask, noise_nchw, offset, perturb_nchw,
                     timesteps, alphas_cumprod, (bf16_t*)input_nhwc_bf16, target_nchw, latents_nchw, noisy_nchw, masked_latents_nchw, B,
                     L, H * W, moment_stride, cpad, scale, offset_mag, perturb_mag, prediction_type);
  SDT_LAUNCH_CHECK("sdt_inpaint_noise_target");
  return SDT_OK;
}

int sdt_inpaint_pack_input(const uint16_t* latents_nhwc, const uint16_t* masked_latents_nhwc, const float* latent_mask,
                           uint16_t* input_nhwc, int R, int B, int L, int H, int W, int cpad_src, int cpad_m, int cpad_dst,
                           hipStream_t stream) {
  SDT_CHECK_ARG(latents_nhwc && masked_latents_nhwc && latent_mask && input_nhwc, "sdt_inpaint_pack_input: null pointer");
  SDT_CHECK_ARG(R > 0 && B > 0 && L > 0 && H > 0 && W > 0 && R % B == 0,
                "sdt_inpaint_pack_input: bad shape R=%d B=%d L=%d H=%d W=%d (R a multiple of B)", R, B, L, H, W);
  SDT_CHECK_ARG(cpad_src >= L && cpad_m >= L && cpad_dst >= 2 * L + 1,
                "sdt_inpaint_pack_input: cpad_src=%d and cpad_m=%d must hold L=%d channels, cpad_dst=%d must hold 2L+1", cpad_src, cpad_m,
                L, cpad_dst);
  const bool vin = cpad_src % 8 == 0 && cpad_m % 8 == 0 && (((uintptr_t)latents_nhwc | (uintptr_t)masked_latents_nhwc) & 15) == 0;
  const bool vout = cpad_dst % 8 == 0 && ((uintptr_t)input_nhwc & 15) == 0;
  auto kern = vin ? (vout ? inpaint_pack_input_kernel<true, true> : inpaint_pack_input_kernel<true, false>)
                  : (vout ? inpaint_pack_input_kernel<false, true> : inpaint_pack_input_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(sdt_grid_1d((long)R * H * W, 256)), dim3(256), 0, stream, (const bf16_t*)latents_nhwc,
                     (const bf16_t*)masked_latents_nhwc, latent_mask, (bf16_t*)input_nhwc, R, B, L, H * W, cpad_src, cpad_m, cpad_dst);
  SDT_LAUNCH_CHECK("sdt_inpaint_pack_input");
  return SDT_OK;
}

int sdt_control_concat_add(const uint16_t* a, const uint16_t* skip, const uint16_t* res, const float* scale, uint16_t* wide,
                           int64_t rows, int64_t rows_per_sample, int Ca, int Cb, hipStream_t stream) {
  SDT_CHECK_ARG(skip && res && wide, "sdt_control_concat_add: null pointer (skip, res and wide are required)");
  SDT_CHECK_ARG(Cb >= 1 && Ca >= 0, "sdt_control_concat_add: bad widths Ca=%d Cb=%d (Ca >= 0, Cb >= 1)", Ca, Cb);
  SDT_CHECK_ARG(a || Ca == 0, "sdt_control_concat_add: Ca=%d needs the left part (a is null)", Ca);
  SDT_CHECK_ARG(rows_per_sample >= 1, "sdt_control_concat_add: rows_per_sample=%ld must be at least 1", (long)rows_per_sample);
  SDT_CHECK_ARG(rows >= 0 && rows % rows_per_sample == 0, "sdt_control_concat_add: rows=%ld is not a multiple of rows_per_sample=%ld",
                (long)rows, (long)rows_per_sample);
  if (rows == 0) return SDT_OK;
  const uintptr_t bases = (uintptr_t)skip | (uintptr_t)res | (uintptr_t)wide | (Ca ? (uintptr_t)a : 0);
  const bool vec = Ca % 8 == 0 && Cb % 8 == 0 && (bases & 15) == 0;
  const int width = vec ? (Ca + Cb) / 8 : Ca + Cb;  // what threadIdx.x walks: 16-byte chunks or elements of a row
  int cx = 1;
  while (cx < width && cx < 256) cx <<= 1;
  const dim3 block(cx, 256 / cx), grid(sdt_grid_1d((long)rows, 256 / cx));
  if (vec) {
    hipLaunchKernelGGL(control_concat_add_vec_kernel, grid, block, 0, stream, (const uint4*)a, (const uint4*)skip, (const uint4*)res, scale,
                       (uint4*)wide, (long)rows, (long)rows_per_sample, Ca / 8, Cb / 8);
  } else {
    hipLaunchKernelGGL(control_concat_add_scalar_kernel, grid, block, 0, stream, (const bf16_t*)a, (const bf16_t*)skip, (const bf16_t*)res,
                       scale, (bf16_t*)wide, (long)rows, (long)rows_per_sample, Ca, Cb);
  }
  SDT_LAUNCH_CHECK("sdt_control_concat_add");
  return SDT_OK;
}

#define MSE_MAX_BLOCKS 512
int64_t sdt_reduce_workspace_bytes(void) { return SDT_WS_COUNTER_BYTES + 65536; }

/* workspace: sdt_reduce_workspace_bytes() bytes under the split-workspace contract (first 64 KiB zero when enqueued, zero again
 * afterwards): the per-workgroup partial losses, added in order by the workgroup that arrives last */
int sdt_mse_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* weight, float* loss_accum,
                         uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && target_nchw && loss_accum && B > 0 && C > 0 && cpad >= C, "sdt_mse_loss_fwd_bwd: bad args");
  SDT_CHECK_ARG(workspace && workspace_bytes >= sdt_reduce_workspace_bytes(), "sdt_mse_loss_fwd_bwd: workspace of sdt_reduce_workspace_bytes() needed");
  const float inv_count = 1.0f / ((float)B * C * H * W);
  hipLaunchKernelGGL(mse_kernel, dim3(sdt_grid_1d((long)B * H * W, 256, MSE_MAX_BLOCKS)), dim3(256), 0, stream,
                     (const bf16_t*)pred_nhwc, target_nchw, weight, loss_accum, (bf16_t*)dpred_nhwc, B, C, H * W, cpad,
                     inv_count, reinterpret_cast<int*>(workspace), reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_mse_loss_fwd_bwd");
  return SDT_OK;
}

int sdt_loss_mask_prepare(const float* mask, float* effective, float* pooled, float* sums, int B, int h, int w, int f, float floor_value,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(mask && effective && sums, "sdt_loss_mask_prepare: null pointer");
  SDT_CHECK_ARG((((uintptr_t)mask | (uintptr_t)effective | (uintptr_t)pooled | (uintptr_t)sums) & 3) == 0,
                "sdt_loss_mask_prepare: misaligned pointer (4 bytes)");
  SDT_CHECK_ARG(B > 0 && B <= MASKED_MAX_B && h > 0 && w > 0 && (long)h * w <= (1L << 30),
                "sdt_loss_mask_prepare: bad shape B=%d h=%d w=%d (1 <= B <= %d)", B, h, w, MASKED_MAX_B);
  SDT_CHECK_ARG(f == 1 || f == 2 || f == 4 || f == 8 || f == 16, "sdt_loss_mask_prepare: f=%d (the mask's scale must be 1, 2, 4, 8 or 16)", f);
  SDT_CHECK_ARG(floor_value >= 0.f && floor_value <= 1.f, "sdt_loss_mask_prepare: floor %g must lie in [0, 1]", floor_value);
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_reduce_workspace_bytes(),
                "sdt_loss_mask_prepare: workspace of sdt_reduce_workspace_bytes() needed");
  const dim3 grid(masked_blocks(B, (long)h * w), B);
  const bool vec = f >= 4 && ((uintptr_t)mask & 15) == 0;
  int* counters = reinterpret_cast<int*>(workspace);
  float* part = reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES);
  switch (f) {
    case 1: loss_mask_prepare_launch<1>(vec, grid, stream, mask, floor_value, effective, pooled, sums, h, w, counters, part); break;
    case 2: loss_mask_prepare_launch<2>(vec, grid, stream, mask, floor_value, effective, pooled, sums, h, w, counters, part); break;
    case 4: loss_mask_prepare_launch<4>(vec, grid, stream, mask, floor_value, effective, pooled, sums, h, w, counters, part); break;
    case 8: loss_mask_prepare_launch<8>(vec, grid, stream, mask, floor_value, effective, pooled, sums, h, w, counters, part); break;
    default: loss_mask_prepare_launch<16>(vec, grid, stream, mask, floor_value, effective, pooled, sums, h, w, counters, part); break;
  }
  SDT_LAUNCH_CHECK("sdt_loss_mask_prepare");
  return SDT_OK;
}

int sdt_masked_mse_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* effective_mask, const float* mask_sums,
                                const float* snr_weight, const float* loss_weight, float* loss_accum, float* loss_per_sample,
                                uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace, int64_t workspace_bytes,
                                hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && target_nchw && loss_accum && loss_per_sample, "sdt_masked_mse_loss_fwd_bwd: null pointer");
  SDT_CHECK_ARG((((uintptr_t)target_nchw | (uintptr_t)effective_mask | (uintptr_t)mask_sums | (uintptr_t)snr_weight | (uintptr_t)loss_weight |
                  (uintptr_t)loss_accum | (uintptr_t)loss_per_sample) & 3) == 0 && (((uintptr_t)pred_nhwc | (uintptr_t)dpred_nhwc) & 1) == 0,
                "sdt_masked_mse_loss_fwd_bwd: misaligned pointer (4 bytes, bf16: 2 bytes)");
  SDT_CHECK_ARG(B > 0 && B <= MASKED_MAX_B && C > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 30),
                "sdt_masked_mse_loss_fwd_bwd: bad shape B=%d C=%d H=%d W=%d (1 <= B <= %d)", B, C, H, W, MASKED_MAX_B);
  SDT_CHECK_ARG(cpad >= C, "sdt_masked_mse_loss_fwd_bwd: cpad=%d < C=%d", cpad, C);
  SDT_CHECK_ARG(effective_mask || !mask_sums, "sdt_masked_mse_loss_fwd_bwd: mask sums (normalisation) need the effective mask");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_reduce_workspace_bytes(),
                "sdt_masked_mse_loss_fwd_bwd: workspace of sdt_reduce_workspace_bytes() needed");
  const int HW = H * W;
  const float inv_count = 1.0f / ((float)B * C * H * W), inv_chw = 1.0f / ((float)C * H * W);
  const bool vec = cpad % 8 == 0 && (((uintptr_t)pred_nhwc | (uintptr_t)dpred_nhwc) & 15) == 0;
  auto kern = vec ? masked_mse_kernel<true, LOSS_L2> : masked_mse_kernel<false, LOSS_L2>;
  hipLaunchKernelGGL(kern, dim3(masked_blocks(B, HW), B), dim3(256), 0, stream, (const bf16_t*)pred_nhwc, target_nchw, effective_mask,
                     mask_sums, snr_weight, loss_weight, (const float*)nullptr, loss_accum, loss_per_sample, (bf16_t*)dpred_nhwc, B, C, HW,
                     cpad, inv_count, inv_chw, reinterpret_cast<int*>(workspace),
                     reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_masked_mse_loss_fwd_bwd");
  return SDT_OK;
}

int sdt_robust_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* effective_mask, const float* mask_sums,
                            const float* snr_weight, const float* loss_weight, const float* huber_c, int loss_type, float* loss_accum,
                            float* loss_per_sample, uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && target_nchw && huber_c && loss_accum && loss_per_sample, "sdt_robust_loss_fwd_bwd: null pointer");
  SDT_CHECK_ARG((((uintptr_t)target_nchw | (uintptr_t)effective_mask | (uintptr_t)mask_sums | (uintptr_t)snr_weight | (uintptr_t)loss_weight |
                  (uintptr_t)huber_c | (uintptr_t)loss_accum | (uintptr_t)loss_per_sample) & 3) == 0 &&
                    (((uintptr_t)pred_nhwc | (uintptr_t)dpred_nhwc) & 1) == 0,
                "sdt_robust_loss_fwd_bwd: misaligned pointer (4 bytes, bf16: 2 bytes)");
  SDT_CHECK_ARG(loss_type == LOSS_HUBER || loss_type == LOSS_SMOOTH_L1, "sdt_robust_loss_fwd_bwd: loss_type %d (1 huber, 2 smooth_l1)",
                loss_type);
  SDT_CHECK_ARG(B > 0 && B <= MASKED_MAX_B && C > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 30),
                "sdt_robust_loss_fwd_bwd: bad shape B=%d C=%d H=%d W=%d (1 <= B <= %d)", B, C, H, W, MASKED_MAX_B);
  SDT_CHECK_ARG(cpad >= C, "sdt_robust_loss_fwd_bwd: cpad=%d < C=%d", cpad, C);
  SDT_CHECK_ARG(effective_mask || !mask_sums, "sdt_robust_loss_fwd_bwd: mask sums (normalisation) need the effective mask");
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_reduce_workspace_bytes(),
                "sdt_robust_loss_fwd_bwd: workspace of sdt_reduce_workspace_bytes() needed");
  const int HW = H * W;
  const float inv_count = 1.0f / ((float)B * C * H * W), inv_chw = 1.0f / ((float)C * H * W);
  const bool vec = cpad % 8 == 0 && (((uintptr_t)pred_nhwc | (uintptr_t)dpred_nhwc) & 15) == 0;
  auto kern = loss_type == LOSS_HUBER ? (vec ? masked_mse_kernel<true, LOSS_HUBER> : masked_mse_kernel<false, LOSS_HUBER>)
                                      : (vec ? masked_mse_kernel<true, LOSS_SMOOTH_L1> : masked_mse_kernel<false, LOSS_SMOOTH_L1>);
  hipLaunchKernelGGL(kern, dim3(masked_blocks(B, HW), B), dim3(256), 0, stream, (const bf16_t*)pred_nhwc, target_nchw, effective_mask,
                     mask_sums, snr_weight, loss_weight, huber_c, loss_accum, loss_per_sample, (bf16_t*)dpred_nhwc, B, C, HW, cpad,
                     inv_count, inv_chw, reinterpret_cast<int*>(workspace),
                     reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_robust_loss_fwd_bwd");
  return SDT_OK;
}

/* the grid of the masked-loss kernels; the two sets of B * nb partials outgrow the 64 KiB of sdt_reduce_workspace_bytes() only when
 * B * nb > 8192 floats */
int64_t sdt_dpo_loss_workspace_bytes(int B, int H, int W) {
  if (B < 2 || B > MASKED_MAX_B || B % 2 || H <= 0 || W <= 0 || (long)H * W > (1L << 30)) return -1;
  const int64_t need = SDT_WS_COUNTER_BYTES + 2 * (int64_t)B * masked_blocks(B, (long)H * W) * (int64_t)sizeof(float);
  return need > sdt_reduce_workspace_bytes() ? need : sdt_reduce_workspace_bytes();
}

int sdt_dpo_loss_fwd_bwd(const uint16_t* pred_nhwc, const uint16_t* ref_pred_nhwc, const float* target_nchw, float beta, float* loss_accum,
                         float* sample_mse, float* logits, float* pair_loss, float* coef, uint16_t* dpred_nhwc, int B, int C, int H, int W,
                         int cpad, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(pred_nhwc && ref_pred_nhwc && target_nchw && loss_accum && sample_mse && logits && pair_loss && coef && dpred_nhwc,
                "sdt_dpo_loss_fwd_bwd: null pointer");
  SDT_CHECK_ARG((((uintptr_t)target_nchw | (uintptr_t)loss_accum | (uintptr_t)sample_mse | (uintptr_t)logits | (uintptr_t)pair_loss |
                  (uintptr_t)coef) & 3) == 0 && (((uintptr_t)pred_nhwc | (uintptr_t)ref_pred_nhwc | (uintptr_t)dpred_nhwc) & 1) == 0,
                "sdt_dpo_loss_fwd_bwd: misaligned pointer (4 bytes, bf16: 2 bytes)");
  SDT_CHECK_ARG(B >= 2 && B <= MASKED_MAX_B && B % 2 == 0,
                "sdt_dpo_loss_fwd_bwd: B=%d must be even (preferred, rejected pairs) in 2..%d", B, MASKED_MAX_B);
  SDT_CHECK_ARG(C > 0 && H > 0 && W > 0 && (long)H * W <= (1L << 30), "sdt_dpo_loss_fwd_bwd: bad shape C=%d H=%d W=%d", C, H, W);
  SDT_CHECK_ARG(cpad >= C, "sdt_dpo_loss_fwd_bwd: cpad=%d < C=%d", cpad, C);
  SDT_CHECK_ARG(beta > 0.f && beta <= 3.402823466e38f, "sdt_dpo_loss_fwd_bwd: beta=%g must be finite and > 0", (double)beta);
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= sdt_dpo_loss_workspace_bytes(B, H, W),
                "sdt_dpo_loss_fwd_bwd: workspace of sdt_dpo_loss_workspace_bytes() needed");
  const int HW = H * W, P = B / 2;
  const float inv_chw = 1.0f / ((float)C * H * W), inv_pairs = 1.0f / (float)P;
  const float inv_count = 1.0f / (float)((double)P * C * H * W);
  const bool vec = cpad % 8 == 0 && (((uintptr_t)pred_nhwc | (uintptr_t)ref_pred_nhwc | (uintptr_t)dpred_nhwc) & 15) == 0;
  const dim3 grid(masked_blocks(B, HW), B);
  hipLaunchKernelGGL(vec ? dpo_sums_kernel<true> : dpo_sums_kernel<false>, grid, dim3(256), 0, stream, (const bf16_t*)pred_nhwc,
                     (const bf16_t*)ref_pred_nhwc, target_nchw, beta, loss_accum, sample_mse, logits, pair_loss, coef, B, C, HW, cpad,
                     inv_chw, inv_pairs, reinterpret_cast<int*>(workspace),
                     reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_dpo_loss_fwd_bwd");
  hipLaunchKernelGGL(vec ? dpo_grad_kernel<true> : dpo_grad_kernel<false>, grid, dim3(256), 0, stream, (const bf16_t*)pred_nhwc,
                     target_nchw, (const float*)coef, (bf16_t*)dpred_nhwc, C, HW, cpad, inv_count);
  SDT_LAUNCH_CHECK("sdt_dpo_loss_fwd_bwd");
  return SDT_OK;
}

int sdt_timestep_embedding(const int32_t* timesteps, uint16_t* out, int B, int dim, int flip_sin_to_cos,
                           float freq_shift, hipStream_t stream) {
  SDT_CHECK_ARG(timesteps && out && B > 0 && dim > 0 && dim % 2 == 0, "sdt_timestep_embedding: bad args");
  const int n = B * (dim / 2);
  hipLaunchKernelGGL(timestep_embed_kernel, dim3(sdt_ceil_div(n, 256)), dim3(256), 0, stream, timesteps, (bf16_t*)out, B,
                     dim, flip_sin_to_cos, freq_shift, 10000.0f);
  SDT_LAUNCH_CHECK("sdt_timestep_embedding");
  return SDT_OK;
}

static int check_vec(const void* a, const void* b, const void* c, int64_t n, const char* name) {
  SDT_CHECK_ARG(n >= 0 && n % 8 == 0, "%s: element count %ld must be a multiple of 8", name, (long)n);
  SDT_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0, "%s: pointers must be 16-byte aligned", name);
  return SDT_OK;
}

int sdt_act_fwd(const uint16_t* x, uint16_t* y, int64_t n, int act, hipStream_t stream) {
  SDT_CHECK_ARG(x && y, "sdt_act_fwd: null pointer");
  int rc = check_vec(x, y, nullptr, n, "sdt_act_fwd");
  if (rc) return rc;
  if (n == 0) return SDT_OK;
  dim3 g(sdt_grid_1d(n / 8, 256)), b(256);
  switch (act) {
    case ACT_SILU: hipLaunchKernelGGL(act_fwd_kernel<ACT_SILU>, g, b, 0, stream, (const uint4*)x, (uint4*)y, (long)(n / 8)); break;
    case ACT_QUICK_GELU: hipLaunchKernelGGL(act_fwd_kernel<ACT_QUICK_GELU>, g, b, 0, stream, (const uint4*)x, (uint4*)y, (long)(n / 8)); break;
    case ACT_GELU_ERF: hipLaunchKernelGGL(act_fwd_kernel<ACT_GELU_ERF>, g, b, 0, stream, (const uint4*)x, (uint4*)y, (long)(n / 8)); break;
    default: sdt_set_error("sdt_act_fwd: unknown activation %d", act); return SDT_ERR_INVALID_ARG;
  }
  SDT_LAUNCH_CHECK("sdt_act_fwd");
  return SDT_OK;
}

int sdt_act_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int64_t n, int act, hipStream_t stream) {
  SDT_CHECK_ARG(x && dy && dx, "sdt_act_bwd: null pointer");
  int rc = check_vec(x, dy, dx, n, "sdt_act_bwd");
  if (rc) return rc;
  if (n == 0) return SDT_OK;
  dim3 g(sdt_grid_1d(n / 8, 256)), b(256);
  switch (act) {
    case ACT_SILU: hipLaunchKernelGGL(act_bwd_kernel<ACT_SILU>, g, b, 0, stream, (const uint4*)x, (const uint4*)dy, (uint4*)dx, (long)(n / 8)); break;
    case ACT_QUICK_GELU: hipLaunchKernelGGL(act_bwd_kernel<ACT_QUICK_GELU>, g, b, 0, stream, (const uint4*)x, (const uint4*)dy, (uint4*)dx, (long)(n / 8)); break;
    case ACT_GELU_ERF: hipLaunchKernelGGL(act_bwd_kernel<ACT_GELU_ERF>, g, b, 0, stream, (const uint4*)x, (const uint4*)dy, (uint4*)dx, (long)(n / 8)); break;
    default: sdt_set_error("sdt_act_bwd: unknown activation %d", act); return SDT_ERR_INVALID_ARG;
  }
  SDT_LAUNCH_CHECK("sdt_act_bwd");
  return SDT_OK;
}

int sdt_geglu_fwd(const uint16_t* h, uint16_t* out, int64_t M, int F, hipStream_t stream) {
  SDT_CHECK_ARG(h && out && M >= 0 && F > 0 && F % 8 == 0, "sdt_geglu_fwd: bad args (F=%d must be a multiple of 8)", F);
  if (M == 0) return SDT_OK;
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3(sdt_grid_1d(M * (F / 8), 256)), dim3(256), 0, stream, (const uint4*)h,
                     (uint4*)out, (long)M, F / 8);
  SDT_LAUNCH_CHECK("sdt_geglu_fwd");
  return SDT_OK;
}

int sdt_geglu_bwd(const uint16_t* h, const uint16_t* dout, uint16_t* dh, int64_t M, int F, hipStream_t stream) {
  SDT_CHECK_ARG(h && dout && dh && M >= 0 && F > 0 && F % 8 == 0, "sdt_geglu_bwd: bad args");
  if (M == 0) return SDT_OK;
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(sdt_grid_1d(M * (F / 8), 256)), dim3(256), 0, stream, (const uint4*)h,
                     (const uint4*)dout, (uint4*)dh, (long)M, F / 8);
  SDT_LAUNCH_CHECK("sdt_geglu_bwd");
  return SDT_OK;
}

int sdt_copy2d_bf16(uint16_t* dst, int64_t dst_stride, const uint16_t* src, int64_t src_stride, int64_t rows,
                    int cols, hipStream_t stream) {
  SDT_CHECK_ARG(dst && src && rows >= 0 && cols > 0, "sdt_copy2d_bf16: bad args");
  SDT_CHECK_ARG(cols % 8 == 0 && dst_stride % 8 == 0 && src_stride % 8 == 0 &&
                    (((uintptr_t)dst | (uintptr_t)src) & 15) == 0,
                "sdt_copy2d_bf16: cols/strides must be multiples of 8 and pointers 16-byte aligned");
  if (rows == 0) return SDT_OK;
  hipLaunchKernelGGL(copy2d_kernel, dim3(sdt_grid_1d(rows * (cols / 8), 256)), dim3(256), 0, stream, (uint4*)dst,
                     (long)(dst_stride / 8), (const uint4*)src, (long)(src_stride / 8), (long)rows, cols / 8);
  SDT_LAUNCH_CHECK("sdt_copy2d_bf16");
  return SDT_OK;
}

/* n (<= 32) column segments: wide[r][col0_k .. col0_k + cols_k) <-> parts[k][r][0 .. cols_k) (row pitch ld_parts[k]), segments laid
 * side by side in `wide` in index order.  to_wide = 1 gathers (parts[k] == NULL zero-fills the segment), 0 scatters. */
int sdt_copy_cols_bf16(uint16_t* wide, int64_t ld_wide, void* const* parts, const int64_t* ld_parts, const int* cols, int n,
                       int64_t rows, int to_wide, hipStream_t stream) {
  SDT_CHECK_ARG(wide && parts && ld_parts && cols && n > 0 && n <= 32 && rows >= 0, "sdt_copy_cols_bf16: bad args (1..32 segments)");
  SDT_CHECK_ARG(ld_wide % 8 == 0 && ((uintptr_t)wide & 15) == 0, "sdt_copy_cols_bf16: wide matrix must be 16-byte aligned with a pitch that is a multiple of 8");
  ColSeg seg;
  int col0 = 0, maxc = 0;
  for (int k = 0; k < n; ++k) {
    SDT_CHECK_ARG(cols[k] > 0 && cols[k] % 8 == 0 && ld_parts[k] % 8 == 0 && ld_parts[k] >= cols[k] && ((uintptr_t)parts[k] & 15) == 0,
                  "sdt_copy_cols_bf16: segment %d: widths / pitches must be multiples of 8, pointers 16-byte aligned", k);
    SDT_CHECK_ARG(parts[k] || to_wide, "sdt_copy_cols_bf16: segment %d: null destination", k);
    seg.part[k] = (uint4*)parts[k];
    seg.ld_v[k] = ld_parts[k] / 8;
    seg.col0_v[k] = col0 / 8;
    seg.cols_v[k] = cols[k] / 8;
    col0 += cols[k];
    if (cols[k] > maxc) maxc = cols[k];
  }
  SDT_CHECK_ARG(col0 <= ld_wide, "sdt_copy_cols_bf16: segments (%d columns) exceed the wide pitch %ld", col0, (long)ld_wide);
  if (rows == 0) return SDT_OK;
  hipLaunchKernelGGL(copy_cols_kernel, dim3(sdt_grid_1d(rows * (maxc / 8), 256, 4096), n), dim3(256), 0, stream, (uint4*)wide,
                     (long)(ld_wide / 8), seg, (long)rows, to_wide);
  SDT_LAUNCH_CHECK("sdt_copy_cols_bf16");
  return SDT_OK;
}

int sdt_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, int64_t n, hipStream_t stream) {
  SDT_CHECK_ARG(a && b && y, "sdt_add_bf16: null pointer");
  int rc = check_vec(a, b, y, n, "sdt_add_bf16");
  if (rc) return rc;
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(add_kernel, dim3(sdt_grid_1d(n / 8, 256)), dim3(256), 0, stream, (const uint4*)a, (const uint4*)b,
                     (uint4*)y, (long)(n / 8));
  SDT_LAUNCH_CHECK("sdt_add_bf16");
  return SDT_OK;
}

int sdt_upsample2x_fwd(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, hipStream_t stream) {
  SDT_CHECK_ARG(x && y && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "sdt_upsample2x_fwd: bad args");
  hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3(sdt_grid_1d((long)B * 4 * H * W * (C / 8), 256)), dim3(256), 0, stream,
                     (const uint4*)x, (uint4*)y, B, H, W, C / 8);
  SDT_LAUNCH_CHECK("sdt_upsample2x_fwd");
  return SDT_OK;
}

int sdt_upsample2x_bwd(const uint16_t* dy, uint16_t* dx, int B, int H, int W, int C, hipStream_t stream) {
  SDT_CHECK_ARG(dy && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "sdt_upsample2x_bwd: bad args");
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(sdt_grid_1d((long)B * H * W * (C / 8), 256)), dim3(256), 0, stream,
                     (const uint4*)dy, (uint4*)dx, B, H, W, C / 8);
  SDT_LAUNCH_CHECK("sdt_upsample2x_bwd");
  return SDT_OK;
}

int sdt_nchw_f32_to_nhwc_bf16(const float* x, uint16_t* y, int B, int C, int H, int W, int cpad, hipStream_t stream) {
  SDT_CHECK_ARG(x && y && B > 0 && C > 0 && cpad >= C, "sdt_nchw_f32_to_nhwc_bf16: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(sdt_grid_1d((long)B * H * W * cpad, 256)), dim3(256), 0, stream, x,
                     (bf16_t*)y, B, C, H * W, cpad);
  SDT_LAUNCH_CHECK("sdt_nchw_f32_to_nhwc_bf16");
  return SDT_OK;
}

int sdt_nhwc_bf16_to_nchw_f32(const uint16_t* x, float* y, int B, int C, int H, int W, int cpad, hipStream_t stream) {
  SDT_CHECK_ARG(x && y && B > 0 && C > 0 && cpad >= C, "sdt_nhwc_bf16_to_nchw_f32: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(sdt_grid_1d((long)B * H * W * C, 256)), dim3(256), 0, stream,
                     (const bf16_t*)x, y, B, C, H * W, cpad);
  SDT_LAUNCH_CHECK("sdt_nhwc_bf16_to_nchw_f32");
  return SDT_OK;
}

int sdt_cast_f32_to_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t stream) {
  SDT_CHECK_ARG(x && y && n >= 0, "sdt_cast_f32_to_bf16: bad args");
  if (n == 0) return SDT_OK;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(sdt_grid_1d(n, 256 * 4)), dim3(256), 0, stream, x, (bf16_t*)y, (long)n);
  SDT_LAUNCH_CHECK("sdt_cast_f32_to_bf16");
  return SDT_OK;
}

int sdt_transpose_bf16(const uint16_t* x, uint16_t* y, int batch, int R, int C, hipStream_t stream) {
  SDT_CHECK_ARG(x && y && batch > 0 && R > 0 && C > 0 && batch < 65536, "sdt_transpose_bf16: bad args");
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3(sdt_ceil_div(C, 64), sdt_ceil_div(R, 64), batch), dim3(256), 0, stream,
                     (const bf16_t*)x, (bf16_t*)y, R, C);
  SDT_LAUNCH_CHECK("sdt_transpose_bf16");
  return SDT_OK;
}

int sdt_param_prepare(const float* master, uint16_t* w_bf16, uint16_t* wt_bf16, const void* descs_device, int ndesc,
                      int total_tiles, hipStream_t stream) {
  SDT_CHECK_ARG(master && w_bf16 && descs_device && ndesc > 0 && total_tiles > 0, "sdt_param_prepare: bad args");
  hipLaunchKernelGGL(param_prepare_kernel, dim3(total_tiles), dim3(256), 0, stream, master, (bf16_t*)w_bf16,
                     (bf16_t*)wt_bf16, (const SdtPrepDesc*)descs_device, ndesc);
  SDT_LAUNCH_CHECK("sdt_param_prepare");
  return SDT_OK;
}

int sdt_zero_ranges_chunk(void) { return ZR_CHUNK; }

int sdt_zero_ranges(float* base, const int64_t* ranges_device, int nranges, hipStream_t stream) {
  SDT_CHECK_ARG(base && ranges_device && nranges > 0 && ((uintptr_t)base & 15) == 0, "sdt_zero_ranges: bad args");
  hipLaunchKernelGGL(zero_ranges_kernel, dim3(nranges), dim3(256), 0, stream, reinterpret_cast<float4*>(base),
                     reinterpret_cast<const long*>(ranges_device));
  SDT_LAUNCH_CHECK("sdt_zero_ranges");
  return SDT_OK;
}

int sdt_param_prepare_desc_size(void) { return (int)sizeof(SdtPrepDesc); }

int sdt_embedding_fwd(const int32_t* ids, const float* tok, const float* pos, uint16_t* out, int64_t rows, int S, int D,
                      hipStream_t stream) {
  SDT_CHECK_ARG(ids && tok && pos && out && rows > 0 && S > 0 && D > 0, "sdt_embedding_fwd: bad args");
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3(sdt_grid_1d(rows * D, 256)), dim3(256), 0, stream, ids, tok, pos,
                     (bf16_t*)out, (long)rows, S, D);
  SDT_LAUNCH_CHECK("sdt_embedding_fwd");
  return SDT_OK;
}

int sdt_embedding_bwd(const int32_t* ids, const uint16_t* dout, float* dtok, float* dpos, int64_t rows, int S, int D,
                      hipStream_t stream) {
  SDT_CHECK_ARG(ids && dout && dtok && dpos && rows > 0 && S > 0 && D > 0, "sdt_embedding_bwd: bad args");
  SDT_CHECK_ARG(rows + S < (1L << 31), "sdt_embedding_bwd: too many rows");
  hipLaunchKernelGGL(embedding_bwd_kernel, dim3((unsigned)(rows + S)), dim3(256), 0, stream, ids,
                     (const bf16_t*)dout, dtok, dpos, (long)rows, S, D);
  SDT_LAUNCH_CHECK("sdt_embedding_bwd");
  return SDT_OK;
}

static inline bool sdt_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

int sdt_embedding_ext_fwd(const int32_t* ids, const float* tok, const float* ext, const float* pos, uint16_t* out, int64_t rows, int S,
                          int D, int V, int n_ext, hipStream_t stream) {
  SDT_CHECK_ARG(sdt_aligned(ids, 4) && sdt_aligned(tok, 4) && sdt_aligned(ext, 4) && sdt_aligned(pos, 4) && sdt_aligned(out, 2),
                "sdt_embedding_ext_fwd: null or misaligned pointer");
  SDT_CHECK_ARG(rows > 0 && S > 0 && D > 0 && V > 0, "sdt_embedding_ext_fwd: rows=%ld S=%d D=%d V=%d must be positive", (long)rows, S, D, V);
  SDT_CHECK_ARG(n_ext >= 1 && n_ext <= 256, "sdt_embedding_ext_fwd: n_ext=%d outside 1..256", n_ext);
  const bool vec = D % 4 == 0 && sdt_aligned(tok, 16) && sdt_aligned(ext, 16) && sdt_aligned(pos, 16) && sdt_aligned(out, 8);
  if (vec)
    hipLaunchKernelGGL(embedding_ext_fwd_kernel<true>, dim3(sdt_grid_1d(rows * (D / 4), 256)), dim3(256), 0, stream, ids, tok, ext, pos,
                       (bf16_t*)out, (long)rows, S, D, V, n_ext);
  else
    hipLaunchKernelGGL(embedding_ext_fwd_kernel<false>, dim3(sdt_grid_1d(rows * D, 256)), dim3(256), 0, stream, ids, tok, ext, pos,
                       (bf16_t*)out, (long)rows, S, D, V, n_ext);
  SDT_LAUNCH_CHECK("sdt_embedding_ext_fwd");
  return SDT_OK;
}

int sdt_embedding_ext_bwd(const int32_t* ids, const uint16_t* dout, float* dext, int64_t rows, int D, int V, int n_ext,
                          hipStream_t stream) {
  SDT_CHECK_ARG(sdt_aligned(ids, 4) && sdt_aligned(dout, 2) && sdt_aligned(dext, 4), "sdt_embedding_ext_bwd: null or misaligned pointer");
  SDT_CHECK_ARG(rows > 0 && D > 0 && V > 0, "sdt_embedding_ext_bwd: rows=%ld D=%d V=%d must be positive", (long)rows, D, V);
  SDT_CHECK_ARG(n_ext >= 1 && n_ext <= 256, "sdt_embedding_ext_bwd: n_ext=%d outside 1..256", n_ext);
  SDT_CHECK_ARG((D + 255) / 256 <= 65535, "sdt_embedding_ext_bwd: D=%d too wide", D);
  hipLaunchKernelGGL(embedding_ext_bwd_kernel, dim3(n_ext, (D + 255) / 256), dim3(256), 0, stream, ids, (const bf16_t*)dout, dext,
                     (long)rows, D, V);
  SDT_LAUNCH_CHECK("sdt_embedding_ext_bwd");
  return SDT_OK;
}

int sdt_embedding_retract(float* ext, int n_ext, int D, double target_std, double power, double* stats, hipStream_t stream) {
  SDT_CHECK_ARG(sdt_aligned(ext, 4) && sdt_aligned(stats, 8), "sdt_embedding_retract: null or misaligned pointer");
  SDT_CHECK_ARG(D > 0, "sdt_embedding_retract: D=%d must be positive", D);
  SDT_CHECK_ARG(n_ext >= 1 && n_ext <= 256, "sdt_embedding_retract: n_ext=%d outside 1..256", n_ext);
  SDT_CHECK_ARG(target_std > 0.0 && target_std <= 3.4e38 && power == power && power >= -1e6 && power <= 1e6,
                "sdt_embedding_retract: target_std=%g must be finite and > 0, power=%g finite", target_std, power);
  hipLaunchKernelGGL(embedding_retract_kernel, dim3(1), dim3(256), 0, stream, ext, (long)n_ext * D, target_std, power, stats);
  SDT_LAUNCH_CHECK("sdt_embedding_retract");
  return SDT_OK;
}

static int64_t colsum_ws_need(int groups, int nby) { return SDT_WS_COUNTER_BYTES + (int64_t)groups * nby * 256 * (int64_t)sizeof(float); }

/* scratch of the column-sum calls (split-workspace contract: first 64 KiB zero when enqueued, zero again afterwards) */
int64_t sdt_colsum_workspace_bytes(int batch, int64_t rows_per_batch, int N) {
  if (batch <= 0 || rows_per_batch <= 0 || N <= 0) return 0;
  const int ncb = sdt_ceil_div(sdt_ceil_div(N, 8), 32);
  return colsum_ws_need(ncb * batch, (int)((rows_per_batch + 63) / 64));
}

// the grid (ncb column blocks, nby row blocks, batch) of a column sum and its rows per block
static void colsum_plan(int batch, int64_t rows, int N, int want_blocks, int* ncb_out, int* nby_out, int* rpb_out) {
  const int ncb = sdt_ceil_div(sdt_ceil_div(N, 8), 32);
  int nby = (int)((rows + 63) / 64);
  const int want = (want_blocks + ncb * batch - 1) / (ncb * batch);
  if (nby > want) nby = want;
  const int rpb = (int)((rows + nby - 1) / nby);
  *ncb_out = ncb;
  *nby_out = sdt_ceil_div(rows, rpb);
  *rpb_out = rpb;
}

static int colsum_launch(const uint16_t* dy, float* db, uint16_t* out_bf, int batch, int64_t rows, int N, int ld, int want_blocks,
                         void* workspace, int64_t workspace_bytes, const char* name, hipStream_t stream) {
  int ncb, nby, rpb;
  colsum_plan(batch, rows, N, want_blocks, &ncb, &nby, &rpb);
  SDT_CHECK_ARG((int64_t)ncb * batch * (int64_t)sizeof(int) <= SDT_WS_COUNTER_BYTES, "%s: too many column groups", name);
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= colsum_ws_need(ncb * batch, nby),
                "%s: workspace of sdt_colsum_workspace_bytes() needed", name);
  hipLaunchKernelGGL(colsum_kernel, dim3(ncb, nby, batch), dim3(256), 0, stream, (const bf16_t*)dy, db, (bf16_t*)out_bf, (long)rows, N, ld,
                     rpb, batch > 1 ? (long)rows * ld : 0L, N, reinterpret_cast<int*>(workspace),
                     reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  return SDT_OK;
}

/* db[n] += sum_m dy[m][n] */
int sdt_colsum_accumulate(const uint16_t* dy, float* db, int64_t M, int N, int ld, void* workspace, int64_t workspace_bytes,
                          hipStream_t stream) {
  SDT_CHECK_ARG(dy && db && M >= 0 && N > 0 && ld >= N && ld % 8 == 0 && ((uintptr_t)dy & 15) == 0,
                "sdt_colsum_accumulate: bad args (ld=%d must be a multiple of 8)", ld);
  if (M == 0) return SDT_OK;
  int rc = colsum_launch(dy, db, nullptr, 1, M, N, ld, 256, workspace, workspace_bytes, "sdt_colsum_accumulate", stream);
  if (rc) return rc;
  SDT_LAUNCH_CHECK("sdt_colsum_accumulate");
  return SDT_OK;
}

/* out[b][n] = bf16(sum over the rows of batch b (rows_per_batch consecutive rows each) of dy[m][n]); out is (batch, N) bf16:
 * the gradient of a per-image row bias (the time-embedding add of a ResBlock's first convolution) */
int sdt_colsum_batched_bf16(const uint16_t* dy, uint16_t* out, int batch, int64_t rows_per_batch, int N, int ld, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream) {
  SDT_CHECK_ARG(dy && out && batch > 0 && batch < 65536 && rows_per_batch > 0 && N > 0 && ld >= N && ld % 8 == 0 &&
                    ((uintptr_t)dy & 15) == 0, "sdt_colsum_batched_bf16: bad args");
  int rc = colsum_launch(dy, nullptr, out, batch, rows_per_batch, N, ld, 512, workspace, workspace_bytes, "sdt_colsum_batched_bf16", stream);
  if (rc) return rc;
  SDT_LAUNCH_CHECK("sdt_colsum_batched_bf16");
  return SDT_OK;
}

int sdt_colsum_batched_group_max(void) { return COLSUM_GROUP_MAX; }

static bool colsum_problem_ok(const SdtColsumProblem& q) {
  return q.dy && q.out && q.batch > 0 && q.batch < 65536 && q.rows_per_batch > 0 && q.N > 0 && q.ld >= q.N && q.ld % 8 == 0 &&
         ((uintptr_t)q.dy & 15) == 0;
}
// the problems' grids, counters and partial rows laid out back to back; returns the workspace bytes (0: a bad table)
static int64_t colsum_group_plan(const SdtColsumProblem* q, int n, ColsumGroupParams* gp) {
  if (!q || n <= 0 || n > COLSUM_GROUP_MAX) return 0;
  long counters = 0, parts = 0, wgs = 0;
  for (int i = 0; i < n; ++i) {
    if (!colsum_problem_ok(q[i])) return 0;
    int ncb, nby, rpb;
    colsum_plan(q[i].batch, q[i].rows_per_batch, q[i].N, 512, &ncb, &nby, &rpb);  // (512: sdt_colsum_batched_bf16's own)
    wgs += (long)ncb * nby * q[i].batch;
    if (wgs >= (1L << 30)) return 0;
    if (gp) {
      gp->item[i] = ColsumGroupItem{(const bf16_t*)q[i].dy, (bf16_t*)q[i].out, (long)q[i].rows_per_batch, q[i].N, q[i].ld, rpb, ncb, nby,
                                    (int)counters, parts};
      gp->wg_end[i] = (int)wgs;
    }
    counters += (long)ncb * q[i].batch;
    parts += (long)ncb * q[i].batch * nby * 256;
  }
  if (counters * (long)sizeof(int) > SDT_WS_COUNTER_BYTES) return 0;
  if (gp) gp->n = n;
  return SDT_WS_COUNTER_BYTES + parts * (int64_t)sizeof(float);
}

int64_t sdt_colsum_batched_group_workspace_bytes(const SdtColsumProblem* problems, int n) { return colsum_group_plan(problems, n, nullptr); }

int sdt_colsum_batched_group(const SdtColsumProblem* problems, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  ColsumGroupParams gp;
  const int64_t need = colsum_group_plan(problems, n, &gp);
  SDT_CHECK_ARG(need > 0, "sdt_colsum_batched_group: bad args (1..%d problems, each as sdt_colsum_batched_bf16 takes them)", COLSUM_GROUP_MAX);
  SDT_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                "sdt_colsum_batched_group: workspace of sdt_colsum_batched_group_workspace_bytes() needed");
  hipLaunchKernelGGL(colsum_group_kernel, dim3(gp.wg_end[n - 1]), dim3(256), 0, stream, gp, reinterpret_cast<int*>(workspace),
                     reinterpret_cast<float*>((unsigned char*)workspace + SDT_WS_COUNTER_BYTES));
  SDT_LAUNCH_CHECK("sdt_colsum_batched_group");
  return SDT_OK;
}

int sdt_softmax_rows_inplace(uint16_t* x, int64_t rows, int n, float scale, hipStream_t stream) {
  SDT_CHECK_ARG(x && rows > 0 && n > 0 && rows < 2147483647L, "sdt_softmax_rows_inplace: bad args");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, stream, (bf16_t*)x, n, scale);
  SDT_LAUNCH_CHECK("sdt_softmax_rows_inplace");
  return SDT_OK;
}

int sdt_sum_n_bf16(const uint16_t* const* inputs, int n, uint16_t* out, int64_t numel, hipStream_t stream) {
  SDT_CHECK_ARG(inputs && out && n >= 1 && n <= 32 && numel >= 0 && numel % 8 == 0, "sdt_sum_n_bf16: bad arguments (n=%d numel=%ld)", n, (long)numel);
  SumPtrs sp;
  for (int k = 0; k < n; ++k) {
    SDT_CHECK_ARG(inputs[k] && ((uintptr_t)inputs[k] & 15) == 0, "sdt_sum_n_bf16: input %d null or misaligned", k);
    sp.p[k] = reinterpret_cast<const uint4*>(inputs[k]);
  }
  for (int k = n; k < 32; ++k) sp.p[k] = nullptr;
  if (numel == 0) return SDT_OK;
  hipLaunchKernelGGL(sum_n_kernel, dim3(sdt_grid_1d(numel / 8, 256, 2048)), dim3(256), 0, stream, sp, reinterpret_cast<uint4*>(out), n, numel / 8);
  SDT_LAUNCH_CHECK("sdt_sum_n_bf16");
  return SDT_OK;
}

}  // extern "C"
