/* libsdtrain_hip.so - C ABI of the MI355X-native Stable Diffusion train_step hot path.
 *
 * The reference (lodestone-rock/stable_diffusion_training) has no FFI boundary of its own: its hot path is one
 * jitted Python function, training_utils.py:504-762 (train_step), whose arithmetic XLA lowers for the TPU.  These
 * entry points are what a binding for that path calls instead of XLA; each one cites the reference call site (or
 * the third-party module reached from it) whose computation it replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated; the caller owns all memory;
 *     kernels never allocate (scratch is passed in); every call is asynchronous on `stream` and re-entrant.
 *   - return 0 (SDT_OK) or a negative code; sdt_last_error() returns a thread-local message.
 *   - bf16 tensors are uint16_t bit patterns; activations are NHWC / row-major, channel counts multiples of 8;
 *     16-byte aligned base pointers.
 */
#ifndef SDT_H_
#define SDT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t; /* same opaque handle type as <hip/hip_runtime_api.h> */
#endif

enum { SDT_OK = 0, SDT_ERR_INVALID_ARG = -1, SDT_ERR_UNSUPPORTED = -2, SDT_ERR_LAUNCH = -3 };

const char* sdt_last_error(void);
int sdt_abi_version(void);
/* number of HIP devices visible (0 when none / no driver): lets the host fail loudly instead of falling back */
int sdt_device_count(void);

/* ---- hand-off events between a captured step and the gradient exchange (no reference counterpart: under GSPMD the
 * all-reduce lives inside the jitted step, training_utils.py:35-37, 709).  A step captured into a HIP graph marks "this
 * gradient bucket is complete" with sdt_event_record(ev, external = 1, capturing_stream), which becomes an event-record
 * NODE of the graph (a plain record when the stream is not capturing); after every launch of that graph the host calls sdt_stream_wait_event(comm_stream, ev) in front of
 * the bucket's RCCL all-reduce, which stays outside the graph.  external = 0 is an ordinary hipEventRecord.
 * sdt_stream_wait_event_external is the reverse hand-off: on a capturing stream it adds an event-wait NODE, so that every launch
 * of the graph waits THERE for the event's most recent record (the sharded optimizer's all-gather of the weight mirrors, enqueued
 * on the communication stream between two launches and needed only when the next step reaches its text encoder / UNet: it runs
 * beside the next step's VAE encode); on a stream that is not capturing it is sdt_stream_wait_event. */
int sdt_event_create(void** event);
int sdt_event_destroy(void* event);
int sdt_event_record(void* event, int external, hipStream_t stream);
int sdt_stream_wait_event(hipStream_t stream, void* event);
int sdt_stream_wait_event_external(hipStream_t stream, void* event);

/* ---- geometry descriptors (host memory) ---- */
typedef struct SdtConvGeom {
  int batch, in_h, in_w, out_h, out_w, kh, kw, stride, pad_top, pad_left;
} SdtConvGeom;

typedef struct SdtAttnDesc {
  int B, H, Nq, Nk, D;       /* D = head dim; q/k/v/o are (B, N, >=H*D) with a head = columns [h*D, h*D+D) */
  int ldq, ldk, ldv, ldo;    /* row strides in elements */
  float scale;               /* logits scale (1/sqrt(D)) */
  int causal;
  int ldgrad_q, ldgrad_k, ldgrad_v, ld_dout; /* backward only; 0 = same as ldq/ldk/ldv/ldo */
  /* optional device array w[Nk] > 0 (NULL = all ones): P = softmax(scale*q.k + ln w).  diffusers' memory-efficient attention walks
   * the keys in chunks of min(Nq, Nk) (key_chunk_patch.patch sets the chunk to the query count) and takes the last chunk with a
   * clamped jax.lax.dynamic_slice, so when Nk is not a multiple of the chunk the overlapped keys are summed twice: w = 2 there. */
  const float* key_weight;
} SdtAttnDesc;

enum { SDT_GATHER_PLAIN = 0, SDT_GATHER_CONV_FPROP = 1, SDT_GATHER_CONV_DGRAD = 2 };
enum { SDT_ACT_SILU = 0, SDT_ACT_QUICK_GELU = 1, SDT_ACT_GELU_ERF = 2 };

/* ================= scheduler / loss (schedulers/scheduling_utils_flax.py:316-343; training_utils.py:582-586, 704-709) */
/* noisy = sqrt(acp[t])*x0 + sqrt(1-acp[t])*eps ; velocity = sqrt(acp[t])*eps - sqrt(1-acp[t])*x0.
 * latents/noise/noisy_nchw/velocity_nchw: f32 (B,C,H,W); noisy_nhwc_bf16: (B,H,W,cpad) zero padded. */
int sdt_add_noise_velocity(const float* latents, const float* noise, const int32_t* timesteps,
                           const float* alphas_cumprod, uint16_t* noisy_nhwc_bf16, float* noisy_nchw,
                           float* velocity_nchw, int B, int C, int H, int W, int cpad, hipStream_t stream);
/* One sampling step (models/pipeline_flax_stable_diffusion.py:222-232 + diffusers scheduling_ddim_flax.py step(), eta = 0):
 * m = pred[0:B] + guidance_scale * (pred[B:2B] - pred[0:B]); x0 / eps from m by prediction_type (0 epsilon, 1 sample,
 * 2 v_prediction) with alpha_prod_t; latents <- sqrt(alpha_prod_prev)*x0 + sqrt(1-alpha_prod_prev)*eps (in place, f32 NCHW);
 * next_input_nhwc (2B,H,W,cpad) bf16 = the new latents twice (the doubled UNet batch of the next step), padding zero. */
int sdt_ddim_cfg_step(const uint16_t* pred_nhwc, float* latents_nchw, uint16_t* next_input_nhwc, int B, int C, int H, int W,
                      int cpad, float guidance_scale, float alpha_prod_t, float alpha_prod_prev, int prediction_type,
                      hipStream_t stream);
/* Guidance rescale (diffusers rescale_noise_cfg, arXiv:2305.08891 §3.4): factors[b] (B floats) = guidance_rescale *
 * std(tx_b) / std(cfg_b) + (1 - guidance_rescale) with cfg = un + guidance_scale * (tx - un) over the C real channels x H x W
 * of sample b, std unbiased (N - 1); 1 where std(cfg_b) == 0.  pred_nhwc as in sdt_ddim_cfg_step, cpad a multiple of 8.  One
 * workgroup per sample, double accumulation, no atomics: bitwise reproducible.  guidance_rescale in [0, 1]. */
int sdt_cfg_rescale_factors(const uint16_t* pred_nhwc, float* factors, int B, int C, int H, int W, int cpad, float guidance_scale,
                            float guidance_rescale, hipStream_t stream);
/* One step of the other samplers (DDIM with trailing / linspace timesteps, a zero-SNR step or guidance rescale; DPM-Solver++
 * orders 1 and 2, diffusers scheduling_dpmsolver_multistep_flax.py) with classifier-free guidance:
 *   m = (pred[0:B] + guidance_scale * (pred[B:2B] - pred[0:B])) * rescale_factors[b]   (factor 1 when rescale_factors is NULL)
 *   x0, eps from m and the latents x by prediction_type (0 epsilon, 1 sample, 2 v_prediction) with alpha_s, sigma_s of the
 *   current timestep; latents <- c_x*x + c_x0*x0 + c_eps*eps + c_d1*(x0 - x0_history)   (the host folds each sampler into the
 *   four coefficients).  x0_history_nchw (f32 (B,C,H,W), optional): read only when c_d1 != 0, then overwritten with this x0.
 * next_input_nhwc as in sdt_ddim_cfg_step.  Refused: epsilon with alpha_s == 0, sample with sigma_s == 0, non-finite
 * coefficients, c_d1 != 0 without a history, cpad not a multiple of 8. */
int sdt_sampler_cfg_step(const uint16_t* pred_nhwc, float* latents_nchw, uint16_t* next_input_nhwc, float* x0_history_nchw,
                         const float* rescale_factors, int B, int C, int H, int W, int cpad, float guidance_scale, float alpha_s,
                         float sigma_s, int prediction_type, float c_x, float c_x0, float c_eps, float c_d1, hipStream_t stream);
/* latents (B,L,H,W) f32 = (mean + exp(0.5*clip(logvar,-30,20))*eps)*scale from moments bf16 (B,H,W,moment_stride) */
int sdt_vae_posterior_sample(const uint16_t* moments_nhwc, const float* eps_nhwc, float* latents_nchw, int B, int L,
                             int H, int W, int moment_stride, float scale, hipStream_t stream);
/* The front of a training step from cached posterior moments, in one launch and with the bits of the chain it replaces
 * (sdt_vae_posterior_sample, the fp32 noise mixing of train_step, sdt_add_noise_velocity):
 *   x0 = (mean + exp(0.5*clip(logvar,-30,20))*eps)*scale;  n = noise [+ offset[b][c]*offset_mag] [+ perturb_mag*perturb];
 *   noisy = sqrt(acp[t])*x0 + sqrt(1-acp[t])*n;  target = n (prediction_type 0) or sqrt(acp[t])*n - sqrt(1-acp[t])*x0 (2).
 * moments bf16 (B,H,W,moment_stride >= 2L), eps f32 (B,H,W,L), noise / perturb f32 (B,L,H,W), offset f32 (B,L); offset and
 * perturb may be NULL (their magnitude must then be 0).  noisy_nhwc_bf16 (B,H,W,cpad) zero padded; target_nchw f32 (B,L,H,W),
 * NULL allowed only for epsilon without offset or perturbation noise (the target is the noise input); latents_nchw and
 * noisy_nchw f32 (B,L,H,W) optional.  16-byte loads / stores where moment_stride % 8 == 0 and L % 4 == 0 / cpad % 8 == 0 and the
 * base is aligned, a scalar path otherwise. */
int sdt_latent_noise_target(const uint16_t* moments_nhwc, const float* eps_nhwc, const float* noise_nchw, const float* offset,
                            const float* perturb_nchw, const int32_t* timesteps, const float* alphas_cumprod,
                            uint16_t* noisy_nhwc_bf16, float* target_nchw, float* latents_nchw, float* noisy_nchw, int B, int L,
                            int H, int W, int moment_stride, int cpad, float scale, float offset_mag, float perturb_mag,
                            int prediction_type, hipStream_t stream);
/* ---- INPAINTING: the input of a UNet with in_channels = 2L + 1, [noisy latents | mask | VAE latents of the masked image]
 * (diffusers' inpainting training example and pipeline).  fl() is one fp32 rounding; nothing below is contracted.
 *   repaint(m) = (m >= 0.5): 1 repaints, 0 keeps, a NaN keeps.
 *   masked image, at pixel size: repaint ? +0.0 : x - a select, never -0, a NaN pixel under the mask becomes 0.
 *   latent mask, nearest neighbour: m_lat[b][y][x] = repaint(mask[b][y*f][x*f]) ? 1.0f : 0.0f.
 *   masked-image latents: xm = fl(fma(exp(0.5*clip(lv,-30,20)), eps_m, mean) * scale), sdt_vae_posterior_sample's arithmetic on the
 *   masked image's moments with a draw of its own; rounded to bf16 (RNE) where it enters the UNet input.
 *   UNet input bf16 NHWC (B,h,w,cpad >= 2L+1): [0,L) noisy latents, [L] latent mask, [L+1,2L+1) masked-image latents, rest zero.
 * None of the three uses atomics or a workspace.
 * sdt_inpaint_mask_pixels: pixels f32 NCHW (B,C,H,W), mask f32 (B,H,W) -> stacked bf16 NHWC (2B,H,W,cpad): rows [0,B) the image with
 *   the bits of sdt_nchw_f32_to_nhwc_bf16 (one RNE rounding), rows [B,2B) the masked image (the select in fp32, then the same
 *   rounding), padding channels zero; latent_mask f32 (B,H/f,W/f) as above.  One pass over the pixels; 16-byte row stores when
 *   cpad % 8 == 0 and the base is aligned, scalar stores otherwise.  Refused: a NULL pointer, f < 1, H % f or W % f != 0, cpad < C.
 * sdt_inpaint_noise_target: sdt_latent_noise_target's operands, meaning, NULL rules and - in channels [0,L) of input_nhwc, target,
 *   latents and noisy - its bits, plus masked_moments bf16 (B,H,W,moment_stride), masked_eps f32 (B,H,W,L), latent_mask f32 (B,H,W)
 *   (thresholded again with repaint(), idempotent on 0/1) and the optional masked_latents f32 NCHW (B,L,H,W) (xm before the bf16
 *   rounding).  cpad >= 2L+1.  16-byte moment loads when moment_stride % 8 == 0 and both bases are aligned, 16-byte row stores when
 *   cpad % 8 == 0 and the base is aligned; each 8-channel group of a row is stored once.
 * sdt_inpaint_pack_input: the sampler's UNet input.  latents bf16 (R,h,w,cpad_src), masked_latents bf16 (B,h,w,cpad_m), latent_mask
 *   f32 (B,h,w) -> input bf16 (R,h,w,cpad_dst): row r takes the mask and masked latents of sample r % B (the doubled
 *   classifier-free-guidance batch); channels [0,L) and [L+1,2L+1) are 16-bit copies (of latents[..., 0:L] and
 *   masked_latents[..., 0:L]), [L] is repaint(mask) as 1.0 / 0.0, the rest zero.  R % B == 0, cpad_src, cpad_m >= L,
 *   cpad_dst >= 2L+1. */
int sdt_inpaint_mask_pixels(const float* pixels_nchw, const float* mask, uint16_t* stacked_nhwc_bf16, float* latent_mask, int B,
                            int C, int H, int W, int cpad, int f, hipStream_t stream);
int sdt_inpaint_noise_target(const uint16_t* moments_nhwc, const uint16_t* masked_moments_nhwc, const float* eps_nhwc,
                             const float* masked_eps_nhwc, const float* latent_mask, const float* noise_nchw, const float* offset,
                             const float* perturb_nchw, const int32_t* timesteps, const float* alphas_cumprod,
                             uint16_t* input_nhwc_bf16, float* target_nchw, float* latents_nchw, float* noisy_nchw,
                             float* masked_latents_nchw, int B, int L, int H, int W, int moment_stride, int cpad, float scale,
                             float offset_mag, float perturb_mag, int prediction_type, hipStream_t stream);
int sdt_inpaint_pack_input(const uint16_t* latents_nhwc, const uint16_t* masked_latents_nhwc, const float* latent_mask,
                           uint16_t* input_nhwc, int R, int B, int L, int H, int W, int cpad_src, int cpad_m, int cpad_dst,
                           hipStream_t stream);
/* ---- CONTROLNET: the injection of a ControlNet's residuals into the frozen UNet (no reference counterpart; DESIGN.md "ControlNet").
 * sdt_control_concat_add: a bf16 (rows, Ca) or NULL, skip and res bf16 (rows, Cb), scale f32 (rows / rows_per_sample) or NULL (= 1)
 *   -> wide bf16 (rows, Ca + Cb): columns [0, Ca) are 16-bit copies of a, column Ca + j is
 *   bf16_rne((double)skip + (double)scale[row / rows_per_sample] * (double)res): the product is exact in double, the sum is IEEE double
 *   (nothing contracted) and is rounded to bf16 ONCE, to nearest even (a NaN sum gives the quiet NaN 0x7fc0).  No
 *   shortcut for a zero scale: 0 * NaN and 0 * inf are NaN.  a NULL needs Ca == 0: the mid-block form, wide = skip + scale * res.
 *   No atomics, no workspace, 64-bit element counts.  Rows move 16 bytes at a time when Ca % 8 == 0, Cb % 8 == 0 and every base is
 *   16-byte aligned; one element per thread otherwise.  Refused: a NULL skip, res or wide; Cb < 1; Ca < 0; Ca > 0 with a NULL a;
 *   rows_per_sample < 1; rows % rows_per_sample != 0. */
int sdt_control_concat_add(const uint16_t* a, const uint16_t* skip, const uint16_t* res, const float* scale, uint16_t* wide,
                           int64_t rows, int64_t rows_per_sample, int Ca, int Cb, hipStream_t stream);
/* ---- IP-ADAPTER: the image-token term of a decoupled cross-attention (Ye et al. 2023, arXiv:2308.06721; no reference counterpart;
 * DESIGN.md "IP-Adapter"), fused with the add into the text attention's output.  T = 1..16 image tokens do not fill a matrix tile:
 * these calls run on the vector ALUs.  C = H*D; head h is columns [h*D, h*D + D).  fl() is one fp32 rounding, fmaf one fused
 * multiply-add (one rounding); the file is compiled without contraction and writes every multiply-add as an explicit fmaf, so the
 * compiler's contraction setting cannot change a bit of what follows.
 *   operands   q bf16 (B, Nq, >= C), row stride ldq;  kv bf16 (B, T, >= 2C) packed [k | v] (v at column C), row stride ldkv, image
 *              stride T*ldkv - it may be a column slice of a wider grouped projection;  o_txt bf16 (B, Nq, C) or NULL (= +0);
 *              scale_ip f32 (B) or NULL (= 1);  out, dout, dq_in (or NULL = +0), dq bf16 (B, Nq, C);  dkv bf16 (B, T, >= 2C), row
 *              stride ld_dkv, [dK | dV].
 *   logits     s[i,t] = fl(scale * dot), dot = the D products q[i,d] * k[t,d] (exact in fp32) added as an fmaf chain from +0 inside
 *              each 8-element group (4-element in the backward when T > 4), the groups then added in increasing order from +0:
 *              scale multiplies the finished fp32 sum, once
 *   softmax    m = max_t s;  e_t = expf(s_t - m);  z = the e_t added in key order from +0;  p_t = e_t / z (IEEE division), all fp32
 *   forward    acc[i,d] = fmaf chain over t = 0..T-1 from +0 of p_t * v[t,d], fp32;
 *              out = bf16_rne((double)o_txt + (double)scale_ip[b] * (double)acc): the product is exact in double, the sum is one IEEE
 *              double rounding, then ONE rounding to bf16 (nearest even, NaN -> 0x7fc0), as sdt_control_concat_add forms its sum.  No
 *              shortcut for a zero scale.
 *   backward   the probabilities are recomputed as above (no log-sum-exp is saved).  g = fl(scale_ip[b] * dout) (dout itself without
 *              scale_ip);  dP_t = g . v[t] summed as the logits' dot;  delta = fmaf chain over t from +0 of p_t * dP_t;
 *              dS_t = fl(p_t * fl(dP_t - delta));  all fp32, P and dS are never rounded to bf16.
 *              dq = bf16_rne((double)dq_in + (double)fl(scale * a)), a = fmaf chain over t from +0 of dS_t * k[t,d]: one rounding to
 *              bf16, the role dres plays in the norm backwards - q's two consumers cost no add launch.
 *              dK[t,d] = bf16_rne(fl(scale * S)), dV[t,d] = bf16_rne(S'), S = sum_i dS[i,t] q[i,d], S' = sum_i p[i,t] g[i,d] in fp32 in
 *              this order: the Nq rows of an image are dealt to sdt_ip_attention_bwd's partial slots by the shape alone (never by
 *              alignment, device or timing); a slot adds its rows in increasing order by fmaf from +0, and a SECOND small launch adds
 *              the slots in index order from +0.  No float atomics, no hand-off between workgroups: two calls give the same bits.
 *              The gradient of o_txt is dout itself (no launch).
 *   workspace  sdt_ip_attention_bwd_workspace_bytes(B, H, Nq, T, D) bytes (-1 for a refused shape), laid out under the split-workspace
 *              contract of REDUCTION WORKSPACES below: the first 64 KiB are the arrival counters other calls of the stream use - these
 *              two launches never touch them - the rest holds the fp32 slots, which need no initialisation.
 *   vectors    16-byte (backward with T > 4: 8-byte) row accesses when every base and row stride allows it, element accesses
 *              otherwise; both paths give the same bits.
 * Refused with SDT_ERR_INVALID_ARG before any HIP call: a null q, kv, out / dout, dq, dkv or workspace; B, H or Nq < 1; B > 65535; T
 * outside 1..16; D not a multiple of 8 in 8..160; H*D > 2048; a row stride narrower than its row; a bf16 pointer off a 2-byte, scale_ip
 * off a 4-byte or the workspace off a 16-byte boundary; a workspace that is too small. */
int sdt_ip_attention_fwd(const uint16_t* q, const uint16_t* kv, const uint16_t* o_txt, const float* scale_ip, uint16_t* out, int B, int H,
                         int Nq, int T, int D, int ldq, int ldkv, float scale, hipStream_t stream);
int sdt_ip_attention_bwd(const uint16_t* q, const uint16_t* kv, const uint16_t* dout, const float* scale_ip, const uint16_t* dq_in,
                         uint16_t* dq, uint16_t* dkv, int B, int H, int Nq, int T, int D, int ldq, int ldkv, int ld_dkv, float scale,
                         void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_ip_attention_bwd_workspace_bytes(int B, int H, int Nq, int T, int D);
/* loss_accum += mean(w_b*(target-pred)^2); dpred = d loss / d pred (bf16 NHWC, cpad channels).
 * REDUCTION WORKSPACES (this call, sdt_sqnorm_accumulate, sdt_colsum_*): sums that cross workgroups use no float atomics - each
 * workgroup stores a partial, the one that arrives last adds them in a fixed order, so results are bitwise reproducible.  They
 * follow the split-workspace contract of sdt_gemm_nt_bf16: the first 64 KiB are arrival counters that must be ZERO when the call
 * is enqueued and are zero again when it completes, the rest is scratch; one buffer (zeroed once) serves every call of a stream. */
int sdt_mse_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* weight, float* loss_accum,
                         uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream);
int64_t sdt_reduce_workspace_bytes(void);
/* ---- MASKED LOSS: a loss mask and per-sample loss weights (kohya --masked_loss; OneTrainer masked training with an unmasked weight
 * and "normalize masked area loss"; DreamBooth prior_loss_weight).  fl() is one fp32 rounding; nothing below is contracted.
 *   pooled mask     mp[b,y,x] = fl(sum of the f x f block of clamp(m)) * fl(1/f^2): the block is added in row-major order starting
 *                   from +0, clamp(m) = fminf(fmaxf(m, 0), 1) (a NaN counts as 0); f = 1 is the clamp alone (and -0 becomes +0)
 *   effective mask  e = fmaxf(mp, floor), floor in [0, 1] (OneTrainer's rule; floor 0 is kohya's plain multiply): no rounding
 *   sample factor   w_b = fl(snr_weight_b * loss_weight_b) (an absent factor is 1);  S_b = sum_p e[b,p] in the fixed order below;
 *                   s_b = 1, or with normalisation fl(fl(h*w) / S_b) and 0 where S_b == 0 (a fully masked-out sample adds nothing and
 *                   never a NaN);  k_b = fl(w_b * s_b)
 *   loss            (1/count) sum_b k_b sum_{c,p} e[b,p] (target - pred)^2, count = B*C*h*w as in sdt_mse_loss_fwd_bwd
 *   gradient        dpred[b,p,c] = bf16_rne(fl(fl(fl(-2 * fl(k_b * e)) * diff) * inv_count)), diff = target - pred,
 *                   inv_count = fl(1 / fl(B*C*h*w)); padding channels are written as zero
 *   per sample      loss_per_sample[b] = fl(fl(k_b * a_b) * fl(1/(C*h*w))), a_b = sum_{c,p} fl(fl(e * diff) * diff); the mean over b is
 *                   the loss up to rounding.  loss_accum += fl(T * inv_count), T = the terms fl(k_b * a_b) added in sample order.
 * EXACT CASE: with e == 1 (or no mask), no normalisation and loss_weight 1, fl(k_b * e) is snr_weight_b (or 1) and the gradient chain
 * is sdt_mse_loss_fwd_bwd's fl(fl(fl(-2 * w) * diff) * inv_count): every dpred bit is equal, multiplications by 1.0 are the only
 * difference.  The loss differs from that call's only by the order of its sum (per sample first).
 * ORDER of the sums: grid (nb, B), nb = min(ceil(h*w / 256), 128, what the scratch holds); workgroup j of sample b owns positions
 * j*256 + t + i*nb*256; a thread adds its positions in order (channels inside a position in order), the workgroup by block tree,
 * the nb partials in workgroup order by the workgroup that arrives last.  No float atomics: the same bits on every launch.
 *
 * sdt_loss_mask_prepare: mask f32 (B, h*f, w*f), f in {1, 2, 4, 8, 16} -> effective f32 (B,h,w), sums f32 (B) = S_b, and (optional, NULL
 * to skip) pooled f32 (B,h,w) = mp, the un-floored mask a latent cache stores.  Block rows by 16-byte loads when f >= 4 and the
 * mask is 16-byte aligned, scalar loads otherwise.
 * sdt_masked_mse_loss_fwd_bwd: pred bf16 NHWC (B,H,W,cpad) at LATENT size H x W, target f32 NCHW; effective_mask (NULL: all ones),
 * mask_sums (NULL: no normalisation; needs the mask), snr_weight, loss_weight f32 (B) (NULL: ones); loss_accum accumulated,
 * loss_per_sample (B) written, dpred optional.  pred / dpred by 16-byte vectors when cpad % 8 == 0 and both are 16-byte aligned (the
 * padding lanes of pred never enter the arithmetic), element by element otherwise (they are not read).
 * Both: workspace of sdt_reduce_workspace_bytes() under the split-workspace contract above; B <= 8192.  Refused: null or misaligned
 * pointers, B <= 0, cpad < C, another f, a floor outside [0, 1], a workspace that is too small. */
int sdt_loss_mask_prepare(const float* mask, float* effective, float* pooled, float* sums, int B, int h, int w, int f, float floor_value,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream);
int sdt_masked_mse_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* effective_mask, const float* mask_sums,
                                const float* snr_weight, const float* loss_weight, float* loss_accum, float* loss_per_sample,
                                uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace, int64_t workspace_bytes,
                                hipStream_t stream);
/* ---- ROBUST LOSS: pseudo-Huber and smooth-L1 in place of the squared error (kohya --loss_type huber | smooth_l1 with --huber_c and
 * --huber_schedule; the same three options of diffusers' training examples).  Everything around the element is MASKED LOSS above: the
 * effective mask e, the sample factor k_b (with s_b and S_b), the counts, the order of the sums.  fl() is one fp32 rounding, fl64() one
 * IEEE double rounding; nothing below is contracted.
 *   element         diff = fl(target - pred) as in every loss call; c = huber_c[b] >= 0, the sample's threshold (the step reads it
 *                   from a table over the training timesteps).  With r = sqrt(diff^2 + c^2):
 *                     huber      rho = 2c(r - c) = 2c diff^2 / (r + c),   d rho / d pred = -2c diff / r
 *                     smooth_l1  rho = 2(r - c)  = 2 diff^2 / (r + c),    d rho / d pred = -2 diff / r
 *                   The second form of rho is the one evaluated: r - c cancels when |diff| << c.  As c -> inf huber tends to diff^2.
 *   element, bits   formed in double from the two fp32 operands and rounded to fp32 once, so that nothing hangs on what a compiler
 *                   makes of fp32 sqrtf and '/':  dd = diff*diff and c*c are exact in double;  q = fl64(dd + c*c);  r = fl64(sqrt(q));
 *                   den = fl64(r + c);
 *                     huber      g = fl(fl64((-2c * diff) / r))   (-2c * diff is exact),  rho = fl(fl64(fl64(2c * dd) / den))
 *                     smooth_l1  g = fl(fl64((-2 * diff) / r)),                           rho = fl(fl64((2 * dd) / den))   (2 * dd is exact)
 *                   r == 0 (diff and c both zero): g = rho = 0, never a NaN.  fl() of a double is round-to-nearest-even.
 *   gradient        dpred[b,p,c] = bf16_rne(fl(fl(fl(k_b * e) * g) * inv_count)), inv_count = fl(1 / fl(B*C*h*w)); padding channels are
 *                   written as zero.  (g carries the -2 that the squared error's chain multiplies in first.)
 *   per sample      a_b = sum_{c,p} fl(e * rho) in MASKED LOSS's order (thread, block tree, workgroup partials by the last arriver);
 *                   loss_per_sample[b] = fl(fl(k_b * a_b) * fl(1/(C*h*w)))
 *   loss            loss_accum += fl(T * inv_count), T = the terms fl(k_b * a_b) added in sample order.  No float atomics.
 * sdt_robust_loss_fwd_bwd: the operands of sdt_masked_mse_loss_fwd_bwd (NULL effective_mask / mask_sums / snr_weight / loss_weight mean
 * what they mean there, so one launch serves plain, weighted and masked batches; sdt_loss_mask_prepare runs first when there is a mask),
 * huber_c f32 (B), loss_type 1 (huber) or 2 (smooth_l1).  The same grid, partition, workspace (sdt_reduce_workspace_bytes()) and
 * vector rule (16-byte pred / dpred vectors when cpad % 8 == 0 and both are 16-byte aligned).  Refused: null or misaligned pointers,
 * another loss_type, B outside 1..8192, cpad < C, mask sums without the mask, a workspace that is too small. */
int sdt_robust_loss_fwd_bwd(const uint16_t* pred_nhwc, const float* target_nchw, const float* effective_mask, const float* mask_sums,
                            const float* snr_weight, const float* loss_weight, const float* huber_c, int loss_type, float* loss_accum,
                            float* loss_per_sample, uint16_t* dpred_nhwc, int B, int C, int H, int W, int cpad, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream);
/* diffusers embeddings_flax.get_sinusoidal_embeddings -> bf16 (B, dim) */
int sdt_timestep_embedding(const int32_t* timesteps, uint16_t* out, int B, int dim, int flip_sin_to_cos,
                           float freq_shift, hipStream_t stream);

/* ================= optimizer (lion_quant.py:20-211; training_utils.py:355-387, 537-544, 732-746; optax clip/lion) */
/* *out_sq += sum g^2 in double (optax.global_norm; the float32 norm the sweeps derive from it is the rounding of the true norm) */
int sdt_sqnorm_accumulate(const float* g, int64_t n, double* out_sq, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* the same over a bf16 gradient buffer (the kernel leaves' gradients, ABI 5): squares of the stored values, exact in double */
int sdt_sqnorm_accumulate_bf16(const uint16_t* g, int64_t n, double* out_sq, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_sqnorm_workspace_bytes(void);
/* Micro-batch gradient accumulation into an fp32 buffer, element-wise over n, in float32 (ParamStore.accumulate):
 *   SDT_ACC_INIT acc = widen(g) | SDT_ACC_ADD acc += widen(g) | SDT_ACC_FINISH acc = (acc + widen(g)) * scale | SDT_ACC_SCALE acc *= scale
 * g: float32 (g_bf16 = 0, 16-byte aligned) or bf16 (g_bf16 = 1, 8-byte aligned); unused (may be NULL) by SDT_ACC_SCALE.  acc: 16-byte
 * aligned.  out_sq != NULL: *out_sq += sum acc_final^2 in double, bit-identical to sdt_sqnorm_accumulate run over acc afterwards (same
 * partition and ordered sum); workspace as for sdt_sqnorm_accumulate (may be NULL without out_sq). */
#define SDT_ACC_INIT 0
#define SDT_ACC_ADD 1
#define SDT_ACC_FINISH 2
#define SDT_ACC_SCALE 3
int sdt_grad_accumulate(float* acc, const void* g, int g_bf16, int64_t n, int mode, float scale, double* out_sq, void* workspace,
                        int64_t workspace_bytes, hipStream_t stream);
/* fused clip(by *sqnorm, may be NULL) + 8-bit blockwise Lion + decay + update (+EMA) (+bf16 mirror of the new parameters,
 * w_bf16[i] = bf16(p[i]), the compute copy the next forward reads; NULL to skip); in place.
 * thresholds: device float[128], the decision thresholds of _quantize (lion_quant.py:52-59): thresholds[c] = the smallest
 * float32 a >= 0 with rint(a^(1/5) * 127) >= c (thresholds[0] = 0).  The caller builds them once with float32 host arithmetic
 * (stable_diffusion_training_amd/lion_codec.py), which makes the device codes bit-identical to the host definition. */
/* g: the gradient, float32 (g_bf16 = 0) or bf16 (g_bf16 = 1, ABI 5: the kernel leaves' gradients are stored with the precision the
 * reference's kernel cotangents have - flax Dense / Conv with dtype=bfloat16 - and widened here, where optax widens them). */
int sdt_lion8_step(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16, int64_t n,
                   int block_size, const double* sqnorm, const float* thresholds, double max_norm, double lr, double wd,
                   double b1, double b2, double ema_rate, hipStream_t stream);
int sdt_lion32_step(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n,
                    const double* sqnorm, double max_norm, double lr, double wd, double b1, double b2, double ema_rate,
                    hipStream_t stream);
/* Scheduled learning rate and EMA rate: the reference's lion_8bit takes a ScalarOrSchedule learning rate, applied by optax's
 * scale_by_schedule as -lr(count) with count = the number of steps taken before this one (lion_quant.py:159-211); the EMA rate of
 * compute_model_ema (training_utils.py:537-544) is scheduled the same way (diffusers EMAModel warmup).  The host computes every step's
 * scalars (stable_diffusion_training_amd/lr_schedule.py) and the device picks the current one, so a captured step replays the schedule:
 * sdt_opt_schedule_select: one lane reads t = *step and writes cur[0..3] = {lr_tab[min(t, n_lr - 1)], ema_tab[2 m], ema_tab[2 m + 1], 0}
 *   with m = min(t, n_ema - 1), then stores *step = t + 1.  lr_tab: float32 -lr_t; ema_tab: float32 pairs (r_t, 1 - r_t); each table holds
 *   at least one entry (a constant is a one-entry table).  cur: 16-byte aligned, 16 bytes.
 * sdt_lion8_step_scheduled / sdt_lion32_step_scheduled: sdt_lion8_step / sdt_lion32_step with -lr, r and 1 - r read from cur (written by
 *   sdt_opt_schedule_select earlier on the same stream) instead of lr and ema_rate; bit-identical to the by-value sweeps given the same
 *   float32 scalars (the by-value launchers round -lr, r and 1.0 - r to float32 the same way). */
int sdt_opt_schedule_select(int64_t* step, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, float* cur,
                            hipStream_t stream);
int sdt_lion8_step_scheduled(float* p, const void* g, int g_bf16, int8_t* codes, float* inv_scale, float* ema, uint16_t* w_bf16,
                             int64_t n, int block_size, const double* sqnorm, const float* thresholds, double max_norm, const float* cur,
                             double wd, double b1, double b2, hipStream_t stream);
int sdt_lion32_step_scheduled(float* p, const float* g, float* mom, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                              double max_norm, const float* cur, double wd, double b1, double b2, hipStream_t stream);
/* AdamW with decoupled weight decay and bias correction, as a second optimizer beside Lion (not in the reference, whose
 * adam_to_lion_scale_factor only translates an Adam recipe).  All element arithmetic is float32 with every operation rounded
 * separately, division and square root correctly rounded; gc is the clipped gradient (same clip as the Lion sweeps):
 *   m' = b1 m + (1 - b1) gc;  v' = b2 v + (1 - b2) (gc gc);  s' = sqrtf(v');  u = (m' k1) / (s' k2 + eps);  if wd != 0: u = u + wd p;
 *   p' = p + neg_lr u;  ema' = r ema + (1 - r) p';  w_bf16 = bf16(p').
 * sdt_adamw_select: one lane, once per store and step, ahead of the sweeps on the same stream.  t = *step (steps taken before this
 *   one).  prods: two doubles {P1, P2}, 8-byte aligned, 1.0 before the first step; the kernel stores P1 = P1 * b1, P2 = P2 * b2 (running
 *   products in double, no pow) and *step = t + 1.  cur: the step's scalar block, 32 bytes, 16-byte aligned, eight floats
 *     {neg_lr, r, 1 - r, 0, k1, k2, 0, 0},  k1 = (float)(1 / (1 - P1)),  k2 = (float)(1 / sqrt(1 - P2))  (formed in double),
 *   the first four laid out as sdt_opt_schedule_select's block.  lr_tab / ema_tab (both or neither): the tables of
 *   sdt_opt_schedule_select, entry min(t, n - 1); NULL: neg_lr = (float)(-lr), r = (float)ema_rate, 1 - r = (float)(1.0 - ema_rate).
 * sdt_adamw8_step: the 8-bit sweep.  m' and the ROOT s' are stored through the block codec, each with its own int8 codes and per-block
 *   inverse scales: inv = 1 / (absmax <= 0 ? 1 : absmax), code = sign(x inv) c(|x inv|) with c the threshold table of sdt_lion8_step and
 *   NO offset, deq = ((code / 127)^5) / inv; the step reads m = deq(m codes), s = deq(s codes), v = s s.  Initial state: codes 0, inverse
 *   scales 1.  Refusals as sdt_lion8_step (null pointer, block size, n not a multiple of it, misalignment), made before any HIP call.
 * sdt_adamw32_step: the same with float32 m and v stored as they are.
 * b1, b2 are rounded to float32 here, 1 - b1 and 1 - b2 formed in double and rounded, as the Lion launchers do. */
int sdt_adamw_select(int64_t* step, double* prods, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, double lr,
                     double ema_rate, double b1, double b2, float* cur, hipStream_t stream);
int sdt_adamw8_step(float* p, const void* g, int g_bf16, int8_t* m_codes, float* m_inv_scale, int8_t* s_codes, float* s_inv_scale,
                    float* ema, uint16_t* w_bf16, int64_t n, int block_size, const double* sqnorm, const float* thresholds,
                    double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream);
int sdt_adamw32_step(float* p, const float* g, float* m, float* v, float* ema, uint16_t* w_bf16, int64_t n, const double* sqnorm,
                     double max_norm, const float* cur, double wd, double b1, double b2, double eps, hipStream_t stream);
/* Prodigy (Mishchenko & Defazio, arXiv:2306.06101), the Adam-style form with decoupled decay, as a third optimizer: it estimates the
 * distance-to-solution scale d while it trains and steps by d * lr, so lr is a multiplier (1 by default).  One d per store.  All element
 * state is float32 (m, v, s, and p0 = the parameters at the store's first step); every float32 operation below is rounded on its own,
 * division and square root correctly rounded; gc is the clipped gradient (same clip as the other sweeps).  Per step, on one stream:
 *   sdt_prodigy_select, sdt_prodigy_moments_step over every piece of the store, sdt_prodigy_finish, sdt_prodigy_apply_step over every piece.
 * state: ten doubles, 8-byte aligned: {d, d_max, numer, P1, P2, dot, l1, q, lr_t, 0}; before the first step {d0, d0, 0, 1, 1, 0, 0, 0, 0, 0}.
 * cur: the step's scalar block, eight floats, 16-byte aligned: {neg_dlr, r, 1 - r, first, c_m, c_v, c_s, d_eps}.
 * sdt_prodigy_select: one lane.  t = *step.  In double:
 *     P1 = P1 * b1;  P2 = P2 * b2;  bc = use_bias_correction ? sqrt(1 - P2) / (1 - P1) : 1;
 *     lr_t = lr, or -(double)lr_tab[min(t, n_lr - 1)] with tables (sdt_opt_schedule_select's: lr_tab holds -lr_t, ema_tab (r, 1 - r) pairs);
 *     dlr = (d * lr_t) * bc;  q = (d / d0) * dlr;
 *   and each float of cur rounded once from its double: neg_dlr = -dlr, c_m = d * (1 - b1), c_v = (d * d) * (1 - b2),
 *   c_s = safeguard_warmup ? (d / d0) * d : q, first = (t == 0) as 1.0 / 0.0, d_eps = 0; r, 1 - r as sdt_adamw_select forms them.
 *   Then dot = l1 = 0, q and lr_t are kept in state, *step = t + 1.
 * sdt_prodigy_moments_step: element-wise over n (g float32 or bf16 as in sdt_lion8_step), with b1, b2, beta3 rounded to float32:
 *     if first: p0 = p;   m' = b1 m + c_m gc;   v' = b2 v + c_v (gc gc);   s' = beta3 s + c_s gc;
 *     dot += (double)gc * (double)(float)(p0 - p)   (exact products);   l1 += (double)|s'|
 *   the two sums in double by ordered partials under sdt_sqnorm_accumulate's partition (each workgroup's threads walk float4s, x and z
 *   into one accumulator, y and w into a second, the n & 3 tail in workgroup 0), accumulated into state across launches in launch order.
 *   workspace: sdt_prodigy_workspace_bytes() bytes under the split-workspace contract.
 * sdt_prodigy_finish: one lane, in double:
 *     numer = beta3 * numer + q * dot;
 *     if l1 != 0 and lr_t > 0:  d_hat = (d_coef * numer) / l1;  if d == d0: d = max(d, d_hat);  d_max = max(d_max, d_hat);
 *                               d = min(d_max, d * growth_rate);
 *     d_eps = (float)(d * eps)   (the new d; max(a, b) = b > a ? b : a, min(a, b) = b < a ? b : a; growth_rate may be +inf).
 * sdt_prodigy_apply_step: element-wise, wd rounded to float32:
 *     if wd != 0: p = p + (neg_dlr * wd) p;   p' = p + neg_dlr * (m' / (sqrtf(v') + d_eps));   ema' = r ema + (1 - r) p';   w_bf16 = bf16(p').
 *   The step size is the dlr of the OLD d; only d_eps sees the new one.  lr_t == 0 moves nothing in p and leaves d alone.
 * Refusals, before any HIP call: null pointers (ema, w_bf16, sqnorm and the tables may be NULL), buffers not 16-byte aligned (bf16 g and
 * w_bf16: 8, state and step: 8), n < 0, non-finite hyper-parameters (growth_rate: NaN), d0 <= 0, b1 / b2 / beta3 outside [0, 1).  n == 0
 * launches nothing. */
int sdt_prodigy_select(int64_t* step, double* state, const float* lr_tab, int64_t n_lr, const float* ema_tab, int64_t n_ema, double lr,
                       double ema_rate, double b1, double b2, double d0, int use_bias_correction, int safeguard_warmup, float* cur,
                       hipStream_t stream);
int sdt_prodigy_moments_step(const float* p, const void* g, int g_bf16, float* p0, float* m, float* v, float* s, int64_t n,
                             const double* sqnorm, double max_norm, const float* cur, double* state, double b1, double b2, double beta3,
                             void* workspace, int64_t workspace_bytes, hipStream_t stream);
int sdt_prodigy_finish(double* state, float* cur, double beta3, double d0, double d_coef, double growth_rate, double eps,
                       hipStream_t stream);
int sdt_prodigy_apply_step(float* p, const float* m, const float* v, float* ema, uint16_t* w_bf16, int64_t n, const float* cur, double wd,
                           hipStream_t stream);
int64_t sdt_prodigy_workspace_bytes(void);
int sdt_lion8_quantize(const float* x, int8_t* codes, float* inv_scale, int64_t n, int block_size, const float* thresholds,
                       hipStream_t stream);
int sdt_lion8_dequantize(const int8_t* codes, const float* inv_scale, float* x, int64_t n, int block_size,
                         hipStream_t stream);

/* ================= norms (flax nn.GroupNorm / nn.LayerNorm inside diffusers / transformers modules) */
/* No float atomics: every sum that crosses threads or workgroups is a set of single-writer partial sums added in a fixed
   order, so a launch is bitwise reproducible (the reference's jitted step is deterministic).
   stats: (B,G,2) f32 {sum,sumsq} written by fwd and consumed by bwd.
   parts / nparts (fwd, optional): statistics of x as nparts partial rows (B,nparts,G,2), produced by the contraction that wrote
   x (sdt_gemm_nt_bf16 gn_stats); NULL / 0: a statistics pass of its own, through `workspace` (then required).
   dres (bwd, optional): gradient of the branch that forked off x before the norm (residual / skip); dx = norm_bwd(dy) + dres
   in the same pass, replacing the add the reverse-mode sweep of x -> {norm(x), x} would otherwise launch.
   dgamma / dbeta (bwd): += by ONE writer per element (NULL for a frozen norm).  bwd workspaces are required. */
int sdt_groupnorm_fwd(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* stats, int B, int HW,
                      int C, int G, float eps, int fuse_silu, const float* parts, int nparts, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_groupnorm_fwd_workspace_bytes(int B, int HW, int C, int G);
int sdt_groupnorm_bwd(const uint16_t* x, const uint16_t* dy, const float* stats, const float* gamma, const float* beta,
                      uint16_t* dx, float* dgamma, float* dbeta, const uint16_t* dres, int B, int HW, int C, int G, float eps,
                      int fuse_silu, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_groupnorm_bwd_workspace_bytes(int B, int HW, int C);
int sdt_layernorm_fwd(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* mean_rstd, int64_t M,
                      int C, float eps, hipStream_t stream);
/* defer_param_grads = 1: dgamma / dbeta are NOT touched; the per-workgroup partial rows [sdt_layernorm_bwd_partial_rows][2C] stay at
 * the start of `workspace` for a later sdt_norm_param_grads_group call (the sums of many norms in one launch). */
int sdt_layernorm_bwd(const uint16_t* x, const uint16_t* dy, const float* gamma, const float* mean_rstd, uint16_t* dx,
                      float* dgamma, float* dbeta, const uint16_t* dres, int64_t M, int C, int defer_param_grads, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_layernorm_bwd_workspace_bytes(int64_t M, int C);
int64_t sdt_layernorm_bwd_partial_rows(int64_t M, int C);
typedef struct SdtNormGradJob {
  const float* partial;  /* [nrows][2C]: rows of {dgamma | dbeta} partial sums */
  float* dgamma;         /* [C], += */
  float* dbeta;          /* [C], += */
  int nrows, C;
} SdtNormGradJob;
int sdt_norm_param_grads_group(const SdtNormGradJob* jobs, int n, hipStream_t stream);
int sdt_norm_param_grads_group_max(void);
/* CLIP pooled output with its final LayerNorm (transformers CLIPTextTransformer.forward pooling: pooled_output =
 * last_hidden_state[arange(R), p]; CLIPTextModelWithProjection then applies text_projection to it - SDXL's pooled text embedding).
 * ids int32 (R*windows, S), x bf16 (R*windows, S, D): the last encoder layer's output BEFORE final_layer_norm.  Pool row r reads
 * row r*windows (the first caption window of sample r).  p(r): eos_id < 0 - the first position of the largest id (transformers'
 * rule for configs whose eos_token_id is 2); eos_id >= 0 - the first position where ids == eos_id (0 if there is none).
 * fwd: pooled bf16 (R, D) = LayerNorm(x[r*windows, p(r)]; gamma, beta, eps) in fp32; mean_rstd f32 (R, 2) and pos int32 (R) are kept
 * for the backward.  bwd: dx bf16 (R*windows, S, D) is written whole - zero except the pooled positions; dgamma / dbeta (f32 [D]) +=
 * the sums over the R rows, added in row order by one workgroup (NULL for a frozen norm).  D <= 2048, multiple of 8. */
int sdt_clip_pool_fwd(const int32_t* ids, const uint16_t* x, const float* gamma, const float* beta, uint16_t* pooled, float* mean_rstd,
                      int32_t* pos, int R, int windows, int S, int D, int eos_id, float eps, hipStream_t stream);
int sdt_clip_pool_bwd(const uint16_t* x, const uint16_t* dpooled, const float* gamma, const float* mean_rstd, const int32_t* pos,
                      uint16_t* dx, float* dgamma, float* dbeta, int R, int windows, int S, int D, hipStream_t stream);

/* ================= dense contractions (flax nn.Dense / nn.Conv and their transposes) */
/* C[M,N] = A_g[M, taps*Kc] * Bt[N, taps*Kc]^T (+bias[N] f32) (+rowbias[m/rows_per_batch][N] bf16) (+residual).
 * Reduction segment t reads B rows at Bt + t*b_tap_stride; with gather_mode 0 (plain) and taps > 1, A is [M][taps*Kc] and
 * column block t contracts with segment t (the dgrad of Dense layers sharing an input, one launch).
 * b_kmajor = 1: the second operand is B[taps][Kc][ldb] instead (reduction index outermost, N columns contiguous) - the Flax
 * kernel layout itself ([in,out] Dense, HWIO conv), read through transposing LDS reads: the forward contractions consume the
 * bf16 mirror of the parameters as it stands and no transposed copy of the weights exists; the input gradients (which
 * contract over `out`) read the same buffer as Bt.  b_nseg > 0 (with b_kmajor): the N columns are b_nseg-wide segments, segment
 * s is the matrix at B + s*b_seg_stride with row pitch ldb (Dense layers that share an input, whose kernels are separate
 * leaves, as ONE forward GEMM).  ld_rowbias: row pitch of rowbias (0 = N): the per-image row bias of a layer may be a column
 * slice of a wider matrix (the time-embedding projections of all ResBlocks of one width come out of one GEMM). */
int sdt_gemm_nt_bf16(const uint16_t* A, const uint16_t* Bt, uint16_t* C, const float* bias, const uint16_t* rowbias,
                     const uint16_t* residual, int64_t M, int N, int Kc, int taps, int lda, int ldb,
                     int64_t b_tap_stride, int ldc, int ldres, int rows_per_batch, int gather_mode,
                     const SdtConvGeom* geom, void* workspace, int64_t workspace_bytes, float* gn_stats, int gn_groups,
                     int b_kmajor, int b_nseg, int64_t b_seg_stride, int ld_rowbias, hipStream_t stream);
/* gn_stats (optional, [batch][nparts][gn_groups][2] f32): the statistics {sum, sum of squares} of the bf16 outputs per image and
 * channel group, for the flax nn.GroupNorm that consumes this output, WRITTEN (not accumulated: no atomics, no zero fill) by
 * the epilogues as partial rows - output row tile r of an image writes rows 2r (groups that start inside the tile's columns)
 * and 2r+1 (the group that began in the column tile to its left) - which sdt_groupnorm_fwd(parts = gn_stats, nparts) adds up
 * in row order.  nparts = sdt_gemm_nt_gn_parts(...) for this problem; 0 means this shape cannot produce them (an output tile
 * would straddle two images, or a group is wider than a tile). */
int sdt_gemm_nt_gn_parts(int64_t M, int N, int Kc, int taps, int rows_per_batch, int gn_groups, int gather_mode,
                         const SdtConvGeom* geom);
/* bytes of scratch sdt_gemm_nt_bf16 wants for this shape (0 = none; split-K is used only when it is provided).
 * CONTRACT: its first 64 KiB (arrival counters) must be ZERO when the call is enqueued and are zero again when the launch completes
 * (every split of an output tile publishes its fp32 partial sums to its own slab, write-through; the split that arrives last
 * sums the slabs in split order, finishes the tile in the same launch and resets the counter); the slabs themselves need no
 * initialisation, so one buffer zeroed once serves every call issued on one stream.  No atomics touch the data: results are
 * bitwise reproducible from launch to launch. */
int64_t sdt_gemm_nt_workspace_bytes(int64_t M, int N, int Kc, int taps);
/* ---- transformer feed-forward with the GEGLU inside the first Dense layer's epilogue (diffusers FlaxFeedForward / FlaxGEGLU via
 * FlaxBasicTransformerBlock, reference training_utils.py:678-684): out = h[:, :F] * gelu_tanh(h[:, F:]) with h = x @ W1 + b1.
 * sdt_ff_geglu_fwd: x [M][K], W1 the Flax kernel [K][2F], bias [2F] fp32 -> h [M][2F] (kept for the backward) and out [M][F], one launch
 * (the epilogue pairs value and gate columns: no geglu launch, no re-read of h).  Same bf16 rounding points as sdt_gemm_nt_bf16 +
 * sdt_geglu_fwd: bit-identical results.  sdt_ff_geglu_supported: 1 when (M, F, K) is served (unsplit 128-tiles, F % 64 == 0); callers
 * fall back to the separate ops otherwise. */
int sdt_ff_geglu_supported(int64_t M, int F, int K);
int sdt_ff_geglu_fwd(const uint16_t* x, const uint16_t* W1, const float* bias, uint16_t* h, uint16_t* out, int64_t M, int F, int K,
                     hipStream_t stream);


/* dW[tap][K1_valid][N_valid] (f32) = A_g[M,K1]^T * dY[M,N]; optional fused bias gradient dbias[n] = sum_m dY[m][n]
 * (n < N_valid), NULL to skip.  Both are WRITTEN (plain stores, exactly one writer per element), not accumulated: the
 * destination needs no zero fill and no atomics are issued; the sums are bitwise reproducible from launch to launch.
 * n_seg > 0: the N columns are n_seg-wide segments and segment s is written at dW + s*seg_stride (row pitch ldw): one
 * launch for Dense layers that share their input (attention to_q/to_k/to_v), whose gradients are separate leaves.
 * workspace (optional, sdt_gemm_tn_workspace_bytes): lets the reduction over M be split across workgroups when the weight
 * is small (per-split fp32 partial tiles, summed in split order by the split that arrives last).  CONTRACT: its first
 * 64 KiB (arrival counters) must be ZERO when the call is enqueued and are zero again when the launch completes; the rest
 * is scratch, so one buffer zeroed once serves every call issued on one stream.  Without it one workgroup per output tile
 * reduces all of M (same results up to fp32 summation order). */
/* dw_bf16 (ABI 5; here and in the problem tables below): dW is a bf16 buffer - the fp32 sums are rounded once (RNE) when stored, which
 * is the precision of the reference's kernel cotangents (flax modules with dtype=bfloat16); ldw / w_tap_stride / seg_stride stay in
 * elements, sq_slots then hold the squares of the ROUNDED values.  dbias stays float32. */
int sdt_gemm_tn_wgrad(const uint16_t* A, const uint16_t* dY, void* dW, int dw_bf16, float* dbias, int64_t M, int K1, int N, int K1_valid,
                      int N_valid, int taps, int lda, int ldb, int ldw, int64_t w_tap_stride, int n_seg, int64_t seg_stride,
                      int gather_mode, const SdtConvGeom* geom, void* workspace, int64_t workspace_bytes, double* sq_slots,
                      hipStream_t stream);
/* sq_slots (here and in the problem tables below; NULL: off): sdt_wgrad_sq_slots(K1, N, taps) doubles the CALLER HAS ZEROED.  The waves
 * that store dW also add up the squares of what they store (in double: exact products) and WRITE each sum to a slot of their own, so
 * that optax.clip_by_global_norm's norm (reference training_utils.py:379, :732) needs no pass over the finished gradient buffer: the
 * caller adds all slots of all launches in index order (sdt_sum_f64_accumulate) - the float32 norm is the same rounding of the same sum
 * as sdt_sqnorm_accumulate's.  Only meaningful without a gradient exchange (the norm is that of the REDUCED gradient otherwise). */
int64_t sdt_wgrad_sq_slots(int K1, int N, int taps);
int sdt_sum_f64_accumulate(const double* x, int64_t n, double* out, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_gemm_tn_workspace_bytes(int64_t M, int K1, int N, int taps, int n_seg, int gather_mode, const SdtConvGeom* geom);
/* Several Dense-layer weight gradients (plain rows, taps = 1: the arguments of sdt_gemm_tn_wgrad with the same meaning) as ONE or
 * two launches (one per tile size).  The weight gradients of a transformer block (reverse of the flax nn.Dense layers inside diffusers
 * FlaxBasicTransformerBlock / transformers FlaxCLIPEncoderLayer) do not feed the input-gradient chain, so a caller may hold them
 * back and issue them together: each alone is 25 - 100 tiles and mostly prologue / tail.  Same arithmetic per problem as the single
 * call with the same split plan (bitwise reproducible; the split of the reduction over M, and so the fp32 summation order, may
 * differ from the single call's).  workspace: sdt_gemm_tn_wgrad_group_workspace_bytes under the split-workspace contract. */
typedef struct SdtTnProblem {
  const uint16_t* A;   /* x  [M][lda] */
  const uint16_t* dY;  /* dY [M][ldb] */
  void* dW;            /* [K1_valid][ldw] (or n_seg-wide column segments seg_stride apart), written: float32, or bf16 when dw_bf16 */
  float* dbias;        /* [N_valid] or NULL, written */
  int64_t M;
  int K1, N, K1_valid, N_valid, lda, ldb, ldw, n_seg;
  int64_t seg_stride;
  double* sq_slots;    /* or NULL: see sdt_gemm_tn_wgrad */
  int dw_bf16;
} SdtTnProblem;
int sdt_gemm_tn_wgrad_group(const SdtTnProblem* problems, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_gemm_tn_wgrad_group_workspace_bytes(const SdtTnProblem* problems, int n);
int sdt_gemm_tn_wgrad_group_max(void);
/* The same for convolution weight gradients (sdt_gemm_tn_wgrad in fprop-gather mode, dW [kh*kw][K1_valid][N_valid] written): the
 * 3x3 / stride 1 / pad 1 ones the three-taps-per-workgroup kernel serves share grouped launches, the rest run one by one. */
typedef struct SdtConvWgradProblem {
  const uint16_t* A;   /* conv input x, NHWC, channel pitch lda */
  const uint16_t* dY;  /* [M][ldb], M = batch * out_h * out_w */
  void* dW;            /* float32, or bf16 when dw_bf16 */
  float* dbias;        /* or NULL */
  SdtConvGeom geom;
  int K1, N, K1_valid, N_valid, lda, ldb;
  double* sq_slots;    /* or NULL: see sdt_gemm_tn_wgrad */
  int dw_bf16;
} SdtConvWgradProblem;
int sdt_conv_wgrad_group(const SdtConvWgradProblem* problems, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_conv_wgrad_group_workspace_bytes(const SdtConvWgradProblem* problems, int n);
/* db[n] += sum_m dy[m][n] (one writer per element) */
int sdt_colsum_accumulate(const uint16_t* dy, float* db, int64_t M, int N, int ld, void* workspace, int64_t workspace_bytes,
                          hipStream_t stream);
/* out[b][n] = bf16(sum of dy rows of batch b): gradient of the per-image time-embedding bias added by the conv epilogue
 * (diffusers FlaxResnetBlock2D: hidden_states + temb[:, None, None, :]) */
int sdt_colsum_batched_bf16(const uint16_t* dy, uint16_t* out, int batch, int64_t rows_per_batch, int N, int ld, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_colsum_workspace_bytes(int batch, int64_t rows_per_batch, int N);
/* (ABI 5, additive) n <= sdt_colsum_batched_group_max() problems of sdt_colsum_batched_bf16 as one launch.  Each problem keeps the
 * row partition and the order of additions of its single launch (the same bits); the workspace (split-workspace contract) holds the
 * counters and partial rows of all of them: sdt_colsum_batched_group_workspace_bytes(problems, n). */
typedef struct SdtColsumProblem {
  const uint16_t* dy;
  uint16_t* out;
  int batch;
  int64_t rows_per_batch;
  int N, ld;
} SdtColsumProblem;
int sdt_colsum_batched_group(const SdtColsumProblem* problems, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int sdt_colsum_batched_group_max(void);
int64_t sdt_colsum_batched_group_workspace_bytes(const SdtColsumProblem* problems, int n);

/* ================= attention (diffusers attention_flax.py + key_chunk_patch.patch; FlaxCLIPAttention) */
int sdt_attention_fwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, float* lse,
                      const SdtAttnDesc* desc, hipStream_t stream);
/* workspace: sdt_attention_bwd_workspace_bytes(desc) bytes = B*H*Nq floats (delta = rowsum(dO*O)) plus, for few keys and
 * many queries (cross-attention), fp32 dK/dV partial sums: the dK/dV pass then splits the query range over workgroups. */
int sdt_attention_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                      const float* lse, uint16_t* dq, uint16_t* dk, uint16_t* dv, float* workspace, int64_t workspace_bytes,
                      const SdtAttnDesc* desc, hipStream_t stream);
int64_t sdt_attention_bwd_workspace_bytes(const SdtAttnDesc* desc);
/* (ABI 5, additive) The two passes of sdt_attention_bwd as separate calls, for a caller that holds the dK/dV of several attentions
 * back and issues them together (cross-attention: nothing on the input-gradient chain reads dK/dV, and one such pass alone leaves
 * most of the chip idle).  sdt_attention_bwd_dq runs the dQ pass alone and writes delta (sdt_attention_bwd_delta_bytes(desc) bytes).
 * sdt_attention_bwd_dkv_group runs the dK/dV passes of n <= sdt_attention_bwd_dkv_group_max() problems: one launch per kernel
 * instantiation (head-dim class: D <= 48, 64, 80, 96, 128, 160) present in the table per 8 problems, then one launch for the
 * finishing passes of up to 8 split problems.  Every problem keeps the plan of the single call with its full workspace (the query
 * split where that takes it, the order of additions): dk / dv are the single call's bit for bit.  A problem whose plan splits needs
 * `slabs` of sdt_attention_bwd_slab_bytes(desc) bytes (0: no split, slabs may be NULL) of its own; lse, delta, the slabs and the
 * operands must stay valid and unchanged until the grouped call has run. */
typedef struct SdtAttnDkvProblem {
  const uint16_t *q, *k, *v, *dout;
  const float *lse, *delta;
  uint16_t *dk, *dv;
  float* slabs;
  SdtAttnDesc desc;
} SdtAttnDkvProblem;
int sdt_attention_bwd_dq(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const uint16_t* dout,
                         const float* lse, uint16_t* dq, float* delta, const SdtAttnDesc* desc, hipStream_t stream);
int sdt_attention_bwd_dkv_group(const SdtAttnDkvProblem* problems, int n, hipStream_t stream);
int sdt_attention_bwd_dkv_group_max(void);
int64_t sdt_attention_bwd_delta_bytes(const SdtAttnDesc* desc);
int64_t sdt_attention_bwd_slab_bytes(const SdtAttnDesc* desc);
int sdt_softmax_rows_inplace(uint16_t* x, int64_t rows, int n, float scale, hipStream_t stream);

/* ================= elementwise / data movement */
int sdt_act_fwd(const uint16_t* x, uint16_t* y, int64_t n, int act, hipStream_t stream);
int sdt_act_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int64_t n, int act, hipStream_t stream);
int sdt_geglu_fwd(const uint16_t* h, uint16_t* out, int64_t M, int F, hipStream_t stream);
int sdt_geglu_bwd(const uint16_t* h, const uint16_t* dout, uint16_t* dh, int64_t M, int F, hipStream_t stream);
/* out = sum of n <= 32 bf16 tensors of numel elements (fp32 accumulation): the fan-in of a tensor consumed n times */
int sdt_sum_n_bf16(const uint16_t* const* inputs, int n, uint16_t* out, int64_t numel, hipStream_t stream);
int sdt_copy2d_bf16(uint16_t* dst, int64_t dst_stride, const uint16_t* src, int64_t src_stride, int64_t rows, int cols,
                    hipStream_t stream);
/* n (<= 32) column segments of a wide bf16 matrix <-> n narrow matrices in ONE launch: channel concatenation / its split (the UNet's
 * skip connections, diffusers unet_2d_blocks_flax.py jnp.concatenate(..., axis=-1)) and the gradient gather of column slices.
 * Segments sit side by side in `wide` in index order.  to_wide = 1: gather (parts[k] == NULL zero-fills segment k); 0: scatter. */
int sdt_copy_cols_bf16(uint16_t* wide, int64_t ld_wide, void* const* parts, const int64_t* ld_parts, const int* cols, int n,
                       int64_t rows, int to_wide, hipStream_t stream);
int sdt_add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* y, int64_t n, hipStream_t stream);
int sdt_upsample2x_fwd(const uint16_t* x, uint16_t* y, int B, int H, int W, int C, hipStream_t stream);
int sdt_upsample2x_bwd(const uint16_t* dy, uint16_t* dx, int B, int H, int W, int C, hipStream_t stream);
int sdt_nchw_f32_to_nhwc_bf16(const float* x, uint16_t* y, int B, int C, int H, int W, int cpad, hipStream_t stream);
int sdt_nhwc_bf16_to_nchw_f32(const uint16_t* x, float* y, int B, int C, int H, int W, int cpad, hipStream_t stream);
int sdt_cast_f32_to_bf16(const float* x, uint16_t* y, int64_t n, hipStream_t stream);
int sdt_transpose_bf16(const uint16_t* x, uint16_t* y, int batch, int R, int C, hipStream_t stream);
/* fp32 master (Flax layout) -> bf16 compute copy W ([batch][Rp][Cp], zero padded) for every matrix leaf listed;
 * wt_bf16 (optional, may be NULL): additionally the per-tap transposes [batch][Cp][Rp] - the train path does not use them
 * (sdt_gemm_nt_bf16 b_kmajor reads W itself).  descs_device: array of {int64 src_off,w_off,wt_off; int32
 * batch,R,C,Rp,Cp,tile0,flags} (sdt_param_prepare_desc_size bytes each; flags reserved, 0) */
int sdt_param_prepare(const float* master, uint16_t* w_bf16, uint16_t* wt_bf16, const void* descs_device, int ndesc,
                      int total_tiles, hipStream_t stream);
int sdt_param_prepare_desc_size(void);
/* base[4*first .. 4*(first+count)) = 0 for every (first, count) pair of ranges_device (int64 pairs in float4 units, count <=
 * sdt_zero_ranges_chunk()): one launch clears the gradient leaves that are accumulated into (norm parameters, embeddings) -
 * the counterpart of jax.grad starting every leaf at zero (training_utils.py:719-729) for the leaves that need it */
int sdt_zero_ranges(float* base, const int64_t* ranges_device, int nranges, hipStream_t stream);
int sdt_zero_ranges_chunk(void);
int sdt_embedding_fwd(const int32_t* ids, const float* tok, const float* pos, uint16_t* out, int64_t rows, int S, int D,
                      hipStream_t stream);
int sdt_embedding_bwd(const int32_t* ids, const uint16_t* dout, float* dtok, float* dpos, int64_t rows, int S, int D,
                      hipStream_t stream);

/* ---- NEW TOKENS: textual inversion (no reference counterpart; DESIGN.md "New tokens") ----
 * The frozen token table tok f32 (V, D) is continued by n_ext (1..256) trained rows ext f32 (n_ext, D): placeholder j is id V + j.
 * All three calls: no atomics, one writer per element, one fixed summation order, never a read outside a buffer.  Refused with
 * SDT_ERR_INVALID_ARG before any HIP call: a null pointer or one not aligned to its element, rows / S / D / V <= 0, n_ext outside
 * 1..256.
 *
 * Forward.  out[r][c] = bf16_rne(fl32(t[c] + pos[r % S][c])), one fp32 add rounded once to bf16, with
 *   t = tok[id]      for 0 <= id < V          (the bits of sdt_embedding_fwd)
 *   t = ext[id - V]  for V <= id < V + n_ext
 *   t = +0.0         for every other id, negatives included: no table is read (a bad id must not fault)
 * pos f32 (S, D).  D % 4 == 0 with tok / ext / pos 16-byte and out 8-byte aligned: 16-byte table loads and 8-byte stores; otherwise
 * a column per lane.  Both paths give the same bits. */
int sdt_embedding_ext_fwd(const int32_t* ids, const float* tok, const float* ext, const float* pos, uint16_t* out, int64_t rows, int S,
                          int D, int V, int n_ext, hipStream_t stream);
/* dext[j][c] = the fp32 sum, started at +0 and taken in increasing r with one rounding per add, of bf2f(dout[r][c]) over the rows
 * with ids[r] == V + j; WRITTEN, not accumulated: a token no row carries gets +0.0 and the destination needs no zero fill.  One
 * workgroup per (token, 256-column slice).  No gradient for tok or pos. */
int sdt_embedding_ext_bwd(const int32_t* ids, const uint16_t* dout, float* dext, int64_t rows, int D, int V, int n_ext,
                          hipStream_t stream);
/* diffusers' advanced DreamBooth-LoRA retract_embeddings over all n = n_ext * D values of ext, in place, by one workgroup of 256:
 *   mean   = (sum x) / n               double; thread t adds elements t, t + 256, ... in increasing order, then a block tree
 *                                      (stride 128, 64, ..., 1: partial[t] += partial[t + stride])
 *   std    = sqrt(sum (x - mean)^2 / (n - 1))   double, a second pass in the same order; 0 when n == 1
 *   factor = (float) pow(target_std / std, power), the pow in double rounded once to fp32; 1.0f when std == 0
 *   ext[i] = fl32(ext[i] * factor)     one fp32 multiply
 * stats receives {mean, std, (double) factor}.  Also refused: target_std not finite or <= 0, power not finite. */
int sdt_embedding_retract(float* ext, int n_ext, int D, double target_std, double power, double* stats, hipStream_t stream);

/* ---- LoRA: low-rank adapters in weight space (no reference counterpart; DESIGN.md "LoRA") ----
 * An adapted Dense kernel W0 [K][N] (fp32 master of a frozen store) carries A [K][r] and B [r][N] (fp32 leaves of the adapter's
 * own store).  Before a step the merge writes the bf16 mirror W = RNE(W0 + s * A * B) the GEMMs read; after its backward the
 * ordinary weight-gradient kernels have left dW (bf16) in the adapter's scratch, and the projection writes the factors' gradients.
 * Both calls serve one job table in one launch (tile0_* are running tile counts, as sdt_param_prepare's tile0: 64 x 64 tiles of
 * W for the merge; ceil(K/64) row stripes of dA followed by ceil(N/64) column stripes of dB for the projection).  jobs_host and
 * jobs_device hold the same n jobs: the host copy is checked (r in {4, 8, 16, 32, 64, 128}; K, N positive multiples of 8; offsets
 * non-negative multiples of 8 elements; tile counts running) and sizes the grid, the kernels read the device copy.  n == 0 launches
 * nothing and returns SDT_OK.  A and B are rounded to bf16 (RNE) as they are loaded, products are accumulated in fp32 by
 * mfma_f32_16x16x32_bf16 with r padded by zero lanes; no atomics: one writer and one summation order per element. */
typedef struct SdtLoraJob {
  int64_t w0_off;         /* W0 in w0_base (elements) */
  int64_t a_off, b_off;   /* A, B in ab_base: the adapter store's master, or its EMA buffer */
  int64_t w_off, f_off;   /* destinations of the merge in w_bf16 / f32_dst */
  int64_t dw_off;         /* dW [K][N] bf16 in dw_base */
  int64_t ga_off, gb_off; /* dA, dB in grad_base */
  int32_t K, N, r;
  float scale;            /* s = alpha / r */
  int32_t tile0_merge, tile0_project, tiles_da, reserved;
} SdtLoraJob;
int sdt_lora_job_size(void);
/* v = W0 + s * (bf16(A) * bf16(B)) in fp32 (one product rounding, one sum rounding); w_bf16 (or NULL) receives RNE(v) with 16-byte
 * stores - the training mirror - and f32_dst (or NULL) v itself - an adapter folded into a checkpoint; at least one is given. */
int sdt_lora_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, const SdtLoraJob* jobs_host,
                   const void* jobs_device, int n, hipStream_t stream);
/* dA[k][q] = s * sum_n dW[k][n] * bf16(B[q][n]) and dB[q][n] = s * sum_k bf16(A[k][q]) * dW[k][n], WRITTEN as fp32: the gradient of
 * the function the merge evaluated.  dW is read twice (once per factor: 4 B per adapted parameter). */
int sdt_lora_project(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                     const void* jobs_device, int n, hipStream_t stream);

/* ---- DoRA: weight-decomposed LoRA (Liu et al. 2024, arXiv:2402.09353), in weight space (DESIGN.md "DoRA") ----
 * An adapted kernel carries a third trained leaf, the magnitude m [N] (one per output feature, in the adapter's store beside A and B).
 * With v[k][n] = W0[k][n] + s * sum_q bf16(A[k][q]) * bf16(B[q][n]) exactly as sdt_lora_merge forms it (fp32 MFMA accumulation, one
 * product rounding, one sum rounding):
 *   q[n] = sum_k v[k][n]^2   fp32, each square rounded, one fixed order: every thread of the stripe's workgroup adds the rows it owns top
 *                            to bottom, one thread adds the 32 partials of a column in row order; no atomics, one writer
 *   c[n] = sqrt(q[n])        correctly rounded to fp32
 *   g[n] = m[n] / c[n]       correctly rounded IEEE division; 0 when c[n] == 0 (a zero column gives zeros and a zero gradient, no NaN)
 *   W'[k][n] = fl32(v * g)   into f32_dst, RNE_bf16 of that same value into w_bf16: the mirror is the RNE rounding of the folded
 *                            checkpoint bit for bit, as for LoRA
 * sqrt and the two divisions are evaluated in double and rounded once; with 53 >= 2 * 24 + 2 bits that second rounding cannot change
 * the result, so c, g and dm are the correctly rounded fp32 values whatever the compiler makes of fp32 sqrt and '/'.
 * Backward: THE NORM IS HELD CONSTANT (the paper's section 4.3; peft and kohya do the same) - the one place where the gradient
 * written is deliberately not the gradient of the function that was evaluated: c is treated as a constant of the step.
 * With G = dW' (bf16, in the scratch) and P[q][n] = sum_k bf16(A[k][q]) * G[k][n] (the fp32 accumulator of the dB stripe):
 *   dB[q][n] = fl(fl(s * P[q][n]) * g[n])
 *   dA[k][q] = s * sum_n G[k][n] * bf16(fl32(bf16(B[q][n]) * g[n]))     the scale goes onto the B fragment as it is loaded: one
 *                                                                       more bf16 rounding point
 *   u[n]     = sum_k G[k][n] * W0[k][n] + s * sum_q bf16(B[q][n]) * P[q][n]     (= sum_k G v without forming v again)
 *   dm[n]    = u[n] / c[n], 0 when c[n] == 0
 * all WRITTEN (not accumulated) as fp32, one writer per element, no atomics.
 * The calls take the SdtLoraJob table (unchanged, 96 bytes) and a parallel table of n SdtDoraJob; both host copies are checked
 * (sdt_lora_merge's checks; N equal in both tables; DoRA offsets non-negative multiples of 8; stripe0_merge the running count of
 * ceil(N/64) column stripes).  stat_base: an fp32 buffer the adapter owns; leaf i holds c at stat_off and g at stat_off + N. */
typedef struct SdtDoraJob {
  int64_t m_off;   /* m [N] in ab_base (merge) / m_base (init) */
  int64_t gm_off;  /* dm [N] in grad_base */
  int64_t stat_off; /* c [N], then g [N], in stat_base */
  int32_t N;       /* the job's N again: a table built for other leaves is refused */
  int32_t stripe0_merge; /* running count of the merge's 64-column stripes */
} SdtDoraJob;
int sdt_dora_job_size(void);
/* One workgroup per 64-column stripe walks K twice: the column sums of squares, then W' (the second read of W0 mostly hits L2).
 * Publishes c and g; destinations as sdt_lora_merge. */
int sdt_dora_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, float* stat_base,
                   const SdtLoraJob* jobs_host, const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n,
                   hipStream_t stream);
/* m[n] = c[n] by the merge's own reduction (m_base may be ab_base): a merge that follows finds g == 1.0f in every column. */
int sdt_dora_init_magnitude(const float* w0_base, const float* ab_base, float* m_base, const SdtLoraJob* jobs_host,
                            const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n, hipStream_t stream);
/* dA, dB, dm as above from the c and g the last sdt_dora_merge published.  Beyond sdt_lora_project the dB stripes read W0 where they
 * stage dW: 4 B more per adapted parameter. */
int sdt_dora_project(const uint16_t* dw_base, const float* w0_base, const float* ab_base, float* grad_base, const float* stat_base,
                     const SdtLoraJob* jobs_host, const SdtDoraJob* dora_host, const void* jobs_device, const void* dora_device, int n,
                     hipStream_t stream);

/* ---- DPO LOSS: Diffusion-DPO preference loss on (preferred, rejected) pairs against a frozen reference pass (Wallace et al. 2023,
 * arXiv:2311.12908; diffusers train_diffusion_dpo.py; no reference counterpart; DESIGN.md "Diffusion-DPO").  B = 2P samples: sample 2i
 * is the preferred image of pair i, sample 2i+1 the rejected one; pred is the trained pass, ref_pred the reference pass over the same
 * inputs.  fl() is one fp32 rounding, fl64() one IEEE double rounding; nothing below is contracted.
 *   per sample      for x = pred and x = ref_pred alike: diff = fl(target - x); a_b = sum_{c,p} fl(diff * diff) in MASKED LOSS's order
 *                   (grid (nb, B), the same partition: thread, block tree, workgroup partials in workgroup order by the last arriver; no
 *                   float atomics); m_b = fl(a_b * fl(1/(C*h*w))).  sample_mse[0][b] = m_b (trained), sample_mse[1][b] = r_b (reference).
 *   per pair        in double from the four published fp32 values, w = 2i, l = 2i+1:
 *                   D = (m_w - m_l) - (r_w - r_l), evaluated left to right;  z64 = fl64(fl64(-0.5 * beta) * D);  logits[i] = fl(z64)
 *   loss            -logsigmoid(z) in the form that cannot overflow: pair_loss[i] = fl(max(-z64, 0) + log1p(exp(-|z64|)))
 *   weight          s = sigmoid(-z64):  z64 >= 0: s = e / (1 + e), e = exp(-z64);   z64 < 0: s = 1 / (1 + exp(z64))
 *   coefficients    coef[2i] = fl(-beta * s),  coef[2i+1] = fl(+beta * s)     (the product in double, rounded once)
 *   total           loss_accum += fl(T * fl(1/P)), T = the pair_loss terms added in pair order in fp32
 *   gradient        dpred[b,p,c] = bf16_rne(fl(fl(coef_b * diff) * inv_count)), diff the TRAINED pass's difference,
 *                   inv_count = fl(1 / fl(P*C*h*w)); padding channels are written as zero.  This is d(mean over pairs of
 *                   -logsigmoid(z)) / d pred: d m_b / d pred = -2 diff / (C*h*w) and dz/dm_w = -beta/2 = -dz/dm_l.
 * exp and log1p are the device's double functions (not correctly rounded: pair_loss and coef are within 1 fp32 ulp of a correctly
 * rounded evaluation from the published sample_mse; every other output follows bit for bit from the published values before it).
 * sdt_dpo_loss_fwd_bwd: pred, ref_pred bf16 NHWC (B,h,w,cpad), target f32 NCHW (B,C,h,w); loss_accum accumulated; sample_mse f32 (2,B),
 * logits f32 (P), pair_loss f32 (P), coef f32 (B) and dpred bf16 NHWC written.  ONE call, TWO launches on the stream - the sums, then the
 * gradient: a gradient element needs the finished sums of four samples.  16-byte pred / ref_pred / dpred vectors when cpad % 8 == 0 and
 * all three are 16-byte aligned (padding lanes of pred / ref_pred never enter the arithmetic), element by element otherwise (they are
 * not read).  Workspace: sdt_dpo_loss_workspace_bytes(B, H, W) bytes under the split-workspace contract of REDUCTION WORKSPACES above
 * (two sets of B * nb partials: sdt_reduce_workspace_bytes() while 2 * B * nb floats fit its 64 KiB of scratch, more beyond; -1 for a
 * refused shape).  Refused with SDT_ERR_INVALID_ARG before any HIP call: null or misaligned pointers (f32: 4 bytes, bf16: 2 bytes, the
 * workspace: 16 bytes), B odd or outside 2..8192, C, H or W < 1, cpad < C, beta not finite or <= 0, a workspace that is too small. */
int sdt_dpo_loss_fwd_bwd(const uint16_t* pred_nhwc, const uint16_t* ref_pred_nhwc, const float* target_nchw, float beta, float* loss_accum,
                         float* sample_mse, float* logits, float* pair_loss, float* coef, uint16_t* dpred_nhwc, int B, int C, int H, int W,
                         int cpad, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t sdt_dpo_loss_workspace_bytes(int B, int H, int W);
/* sdt_lora_restore: the inverse of sdt_lora_merge / sdt_dora_merge as far as the mirror is concerned - w_bf16[leaf] = bf16_rne(W0) for
 * every adapted leaf of the job table, the bits sdt_param_prepare leaves in those leaves of a store without an adapter: the frozen base
 * is the DPO reference model, with no second set of weights.  One grouped launch over the merge's 64 x 64 tiles, 2 x 16-byte loads and
 * one 16-byte store per run of 8 elements; the job table's checks and refusals are sdt_lora_merge's (n == 0 launches nothing; null
 * w0_base, w_bf16 or job table, pointers off a 16-byte boundary and a bad table are refused).  The factors and f_off are not read. */
int sdt_lora_restore(const float* w0_base, uint16_t* w_bf16, const SdtLoraJob* jobs_host, const void* jobs_device, int n,
                     hipStream_t stream);

/* ---- LoCon: LoRA on convolution kernels (kohya conv_dim / LyCORIS LoCon; DESIGN.md "LoCon") ----
 * A Flax HWIO kernel [kh][kw][Cin][Cout] with Cin, Cout multiples of 8 is one contiguous [K = kh*kw*Cin][N = Cout] matrix in the master
 * and in the bf16 mirror, and LoCon's delta - a kh x kw convolution down to r channels, then a 1x1 convolution up - is A [K][r] * B [r][N]
 * in that layout (A[(t*Cin + i)][q] = lora_down[q][i][tap t], B[q][o] = lora_up[o][q][0][0]).  sdt_lora_merge and sdt_lora_restore serve
 * such a job as they stand.  sdt_lora_project would give each 64-column stripe of dB to ONE workgroup that walks all of K (23040 rows for
 * an SD1.5 up-block conv1); sdt_lora_project_split is the projection for tall K: same SdtLoraJob table (unchanged, and still valid for
 * sdt_lora_project), a parallel table of n SdtLoraSplitJob, one launch.
 *   dA   ceil(K/64) row stripes, the arithmetic of sdt_lora_project bit for bit (one shared device function).
 *   dB   every 64-column stripe is cut along K into chunks of sdt_lora_project_split_rows() rows - a compile-time constant: the split of
 *        a job depends on its K alone, never on the device, r, N or the rest of the table.  One workgroup per (stripe, chunk) adds
 *        sum_k bf16(A[k][q]) * dW[k][n] over its rows, 32 rows per mfma_f32_16x16x32_bf16 step in row order, dW staged through a
 *        double-buffered LDS block with 16-byte loads (the next block's global load is in flight across the MFMAs).
 *        chunks == 1: dB = fl(s * acc) is written directly - sdt_lora_project's bits.
 *        chunks > 1: the workgroup writes its fp32 partial [r][64] into the workspace and takes a ticket at the stripe's INTEGER arrival
 *        counter; the last arriver adds the stripe's partials in chunk order 0, 1, 2, ... (one thread per element, fp32) and writes
 *        dB = fl(s * sum).  No float atomics, one summation order per element: the same bits whether the job runs alone or in any
 *        table, and on every repeated call.
 * Workspace (16-byte aligned, sdt_lora_project_split_workspace_bytes(jobs_host, n) bytes; -1 for a refused table): one int32 counter
 * per dB stripe of the table, rounded up to 256 bytes - ZERO on entry, zero again on exit, so the caller zeroes it once - followed by the
 * partials of the jobs with chunks > 1 (no initialisation needed).  Both host tables are checked before any HIP call: sdt_lora_merge's
 * checks; K, N equal in both tables; chunks == ceil(K / rows); tile0 the running count of tiles_da + stripes * chunks; cnt0 the running
 * count of stripes; part_off the running count of partial floats (stripes * chunks * r * 64 for a job with chunks > 1, else 0); the
 * workspace large enough.  n == 0 launches nothing and returns SDT_OK. */
typedef struct SdtLoraSplitJob {
  int64_t part_off;  /* first partial of the job, in floats behind the counters */
  int32_t K, N;      /* the job's K and N again: a table built for other leaves is refused */
  int32_t tile0;     /* running count of this launch's workgroups */
  int32_t chunks;    /* ceil(K / sdt_lora_project_split_rows()) */
  int32_t cnt0;      /* the job's first arrival counter: running count of ceil(N/64) */
  int32_t reserved;
} SdtLoraSplitJob;
int sdt_lora_split_job_size(void);
int sdt_lora_project_split_rows(void);
int64_t sdt_lora_project_split_workspace_bytes(const SdtLoraJob* jobs_host, int n);
int sdt_lora_project_split(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                           const SdtLoraSplitJob* split_host, const void* jobs_device, const void* split_device, int n, void* workspace,
                           int64_t workspace_bytes, hipStream_t stream);

/* ---- LoHa: Hadamard-product adapters (LyCORIS LoHa without Tucker; FedPara, Hyeon-Woo et al. 2021; DESIGN.md "LoHa") ----
 * An adapted kernel W0 [K][N] - Dense, or an HWIO convolution seen as [kh*kw*Cin][Cout] exactly as LoCon sees it - carries FOUR trained
 * fp32 leaves, in this order in the adapter store: loha_a1 [K][r], loha_b1 [r][N], loha_a2 [K][r], loha_b2 [r][N], and
 *   dW = s * (A1 B1) o (A2 B2)          (o element-wise, s = alpha / r; LyCORIS: A_i = hada_w{i}_b^T, B_i = hada_w{i}_a^T)
 * which reaches rank r^2 and is no low-rank product.  With P_i[k][n] = sum_q bf16(A_i[k][q]) * bf16(B_i[q][n]) - operands rounded RNE as
 * they are loaded, fp32 accumulation by ONE mfma_f32_16x16x32_bf16 K-step with r padded by zero lanes, hence r in {4, 8, 16, 32}:
 *   merge    h = fl(P1 * P2);  t = fl(s * h);  v = fl(W0 + t)   - three fp32 roundings in this order, nothing contracted.
 *            w_bf16 (or NULL) receives RNE(v) with 16-byte stores, f32_dst (or NULL) v itself, as sdt_lora_merge: the folded
 *            checkpoint's bf16 rounding is the training mirror bit for bit.  sdt_lora_restore serves a LoHa table as it stands.
 *   project  G1 = bf16_rne(fl(dW * P2)),  G2 = bf16_rne(fl(dW * P1))   (dW bf16; one fp32 product, rounded once more to bf16 because it
 *            becomes an MFMA operand: unit roundoff 2^-8, the one rounding LoRA's projection does not have)
 *            dA_i[k][q] = fl(s * sum_n G_i[k][n] * bf16(B_i[q][n]))      dB_i[q][n] = fl(s * sum_k bf16(A_i[k][q]) * G_i[k][n])
 *            WRITTEN as fp32: the gradient of the function the merge evaluated, the operands' bf16 rounding passed straight through
 *            as in sdt_lora_project.  P is never written anywhere: a P block leaves the MFMA with its 16 rows standing for the
 *            contraction elements 8 (m >> 2) + 4 b + (m & 3) (dB) or 2 m + b (dA), b = 0, 1, so that a lane's accumulator registers are
 *            the eight elements its operand fragment holds, and G is formed in registers.
 *            dA: ceil(K/64) row stripes walk N.  dB: ALWAYS the LoCon split protocol, for Dense tables too - 64-column stripes cut along K
 *            into chunks of sdt_lora_project_split_rows() rows, one workgroup per (stripe, chunk) accumulates dB1 and dB2 in row
 *            order; chunks == 1 writes fl(s * acc) directly, otherwise fp32 partials, the integer arrival counter, and the last
 *            arriver adds the partials in chunk order 0, 1, 2, ... and writes fl(s * sum).  dW is read twice, as LoRA reads it.
 * No float atomics, one writer and one summation order per element: the same bits whether a job is alone or anywhere in any table, and
 * on every repeated call.
 * Tables: the SdtLoraJob table (unchanged; a_off, b_off, ga_off, gb_off name side 1), the SdtLoraSplitJob table exactly as
 * sdt_lora_project_split takes it (its part_off keeps LoCon's one-set count and is checked as there, but not used), and a parallel table
 * of n SdtLohaJob.  All host copies are checked before any HIP call: sdt_lora_merge's checks; r <= 32; K, N equal across the tables;
 * LoHa offsets non-negative multiples of 8; the running tile, counter and partial counts; the workspace size.  n == 0 launches nothing.
 * Workspace (16-byte aligned, sdt_loha_project_workspace_bytes(jobs_host, n) bytes; -1 for a refused table): the counters of
 * sdt_lora_project_split - ZERO on entry, zero again on exit - followed by TWO partial sets per job with chunks > 1:
 * 2 * stripes * chunks * r * 64 floats, the slab of a (stripe, chunk) being [r][64] of dB1, then [r][64] of dB2. */
typedef struct SdtLohaJob {
  int64_t a2_off, b2_off;   /* A2, B2 in ab_base */
  int64_t ga2_off, gb2_off; /* dA2, dB2 in grad_base */
  int64_t part_off;         /* first partial of the job, in floats behind the counters: the running count of two-set partials */
  int32_t K, N;             /* the job's K and N again: a table built for other leaves is refused */
} SdtLohaJob;
int sdt_loha_job_size(void);
int sdt_loha_merge(const float* w0_base, const float* ab_base, uint16_t* w_bf16, float* f32_dst, const SdtLoraJob* jobs_host,
                   const SdtLohaJob* loha_host, const void* jobs_device, const void* loha_device, int n, hipStream_t stream);
int64_t sdt_loha_project_workspace_bytes(const SdtLoraJob* jobs_host, int n);
int sdt_loha_project(const uint16_t* dw_base, const float* ab_base, float* grad_base, const SdtLoraJob* jobs_host,
                     const SdtLoraSplitJob* split_host, const SdtLohaJob* loha_host, const void* jobs_device, const void* split_device,
                     const void* loha_device, int n, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- test hooks (not for the training path) ----
 * Output channels per tile of the 3x3 halo convolution inside sdt_gemm_nt_bf16: 64 (the default) or 128 (the reference of the
 * bitwise parity test).  Process-wide, not thread-safe; launches already enqueued keep the width they were planned with.
 * Returns the previous width, or -1 (sdt_last_error) for any other value. */
int sdt_conv_halo_set_tile_width(int bn);

#ifdef __cplusplus
}
#endif
#endif /* SDT_H_ */
