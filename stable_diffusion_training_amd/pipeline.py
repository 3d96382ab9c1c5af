"""Sampling / validation path: the reference's FlaxStableDiffusionPipeline._generate
(models/pipeline_flax_stable_diffusion.py:160-254) on the same HIP operators train_step uses - CLIP text encoder, UNet
forward, the fused classifier-free-guidance + DDIM update (`sdt_ddim_cfg_step`; DPM-Solver++, trailing / linspace timesteps and
guidance rescale: `sdt_sampler_cfg_step`), VAE decoder.  The reference uses this
class during training only as the checkpoint container (training_utils.py:1007-1023); sampling is how a run is eyeballed.

No CPU fallback: every tensor op here is a libsdtrain_hip.so launch or torch device plumbing."""
import torch

from . import _lib, nets, ops
from .params import EmaView, ParamStore
from .schedulers import DDIMScheduler


def _store_of(x):
    if isinstance(x, EmaView):
        raise TypeError("sample from EMA weights by loading them into a store (load_models on the -EMA directory)")
    return x.store if hasattr(x, "store") else x


class StableDiffusionPipeline:
    """unet / text_encoder: TrainState or ParamStore (the live training parameters are sampled in place, no copy);
    vae_params: host tree of the full VAE (decoder + post_quant_conv are loaded into a frozen store); configs as in load_models."""

    def __init__(self, unet, text_encoder, vae_params, unet_config, text_encoder_config, vae_config, scheduler=None,
                 scaling_factor=0.18215, device=None, controlnet=None, ip_adapter=None):
        """ip_adapter: None, a nets.IPAdapter (store + config; a training state's unet_state.ip_adapter samples in place), or
        dict(config=, params=) as checkpoint.load_ip_adapter returns it (loaded into a frozen store).
        controlnet: None, a nets.ControlNet (store + config; a training state's unet_state.controlnet samples in place), or
        dict(config=, params=) as checkpoint.load_controlnet returns it (loaded into a frozen store)."""
        _lib.require_device()
        self.unet, self.text_encoder = _store_of(unet), _store_of(text_encoder)
        self.unet_config, self.text_encoder_config, self.vae_config = unet_config, text_encoder_config, vae_config
        self.device = torch.device(device) if device is not None else self.unet.device
        given = dict(controlnet=controlnet, ip_adapter=ip_adapter)
        for i, net in enumerate(nets.SIDE_NETWORKS):  # self.controlnet, self.ip_adapter: None or the wrapper (nets.SideNetwork)
            side = given[net.name]
            if side is not None and nets.inpaint_latent_channels(unet_config) is not None:
                raise ValueError(f"{net.article} on an inpainting UNet is not supported")
            for other in nets.SIDE_NETWORKS[:i]:
                if side is not None and given[other.name] is not None:
                    raise ValueError(f"{net.article} beside {other.article} is not supported")
            if isinstance(side, dict):
                store = ParamStore(net.spec(side["config"]), device=self.device, trainable=False)
                store.load(side["params"])
                side = net.wrapper(store, side["config"])
            setattr(self, net.name, side)
        self.vae_decoder = ParamStore(nets.vae_decoder_spec(vae_config), device=self.device, trainable=False)
        from .checkpoint import flatten_if_nested
        vae_params = flatten_if_nested(vae_params)  # nested Flax tree -> "a/b/kernel" paths
        self.vae_decoder.load(vae_params)
        self.vae_decoder.prepare()
        self.vae_params, self.vae_encoder = vae_params, None  # the encoder store is built on first use (inpainting: _inpaint_conditioning)
        # the reference's placeholder (training_utils.py:998-1004); pass a DDIMScheduler or DPMSolverMultistepScheduler built for the
        # trained schedule instead (a zero-terminal-SNR v-prediction model: timestep_spacing="trailing" or "linspace")
        self.scheduler = scheduler or DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                                    num_train_timesteps=1000, prediction_type="v_prediction")
        self.scaling_factor = scaling_factor
        self.vae_scale_factor = 2 ** (len(vae_config["block_out_channels"]) - 1)

    def _uncond_ids(self, batch, length):
        """tokenizer([""] * batch, padding="max_length") for CLIP: <|startoftext|>, then <|endoftext|> (also the pad token)."""
        # (a checkpoint saved with trained new tokens has a resized table: the tokenizer's ids end below the num_new_tokens new rows)
        v = self.text_encoder_config["vocab_size"] - self.text_encoder_config.get("num_new_tokens", 0)
        ids = torch.full((batch, length), v - 1, dtype=torch.int32, device=self.device)
        ids[:, 0] = v - 2
        return ids

    def _sdxl_conditioning(self, prompt_ids, neg_prompt_ids, height, width):
        """SDXL (diffusers StableDiffusionXLPipeline.encode_prompt / _get_add_time_ids): prompt_ids (B, 2, 77) through the SDXL-mode
        text encoder (nets.sdxl_text_forward) -> context [negative | prompt] and added_cond {text_embeds: pooled, time_ids: (H, W, 0, 0,
        H, W)} for the doubled batch.  neg_prompt_ids None: the negative context and pooled embedding are zeros
        (force_zeros_for_empty_prompt, the SDXL base default)."""
        dev = self.device
        B = prompt_ids.shape[0]
        if prompt_ids.dim() != 3 or prompt_ids.shape[1] != 2:
            raise ValueError(f"SDXL prompt_ids must be (B, 2, 77), one row per text tower; got {tuple(prompt_ids.shape)}")
        self.unet.prepare()
        self.text_encoder.prepare()
        ids = prompt_ids.to(device=dev, dtype=torch.int32)
        if neg_prompt_ids is not None:
            ids = torch.cat([neg_prompt_ids.to(device=dev, dtype=torch.int32), ids])
        ctx, pooled = nets.sdxl_text_forward(self.text_encoder, self.text_encoder_config, ids.contiguous())
        if neg_prompt_ids is None:
            zc = torch.zeros(2 * B, *ctx.shape[1:], dtype=ctx.dtype, device=dev)
            zp = torch.zeros(2 * B, *pooled.shape[1:], dtype=pooled.dtype, device=dev)
            zc[B:].copy_(ctx)
            zp[B:].copy_(pooled)
            ctx, pooled = zc, zp
        tid = torch.zeros(2 * B, 6, dtype=torch.int32, device=dev)
        tid[:, 0::4].fill_(height)
        tid[:, 1::4].fill_(width)
        return ctx.detach(), {"text_embeds": pooled.detach(), "time_ids": tid}

    def _inpaint_conditioning(self, image, mask, masked_eps, generator, L, height, width):
        """The constant part of an inpainting UNet's input (include/sdt.h "INPAINTING"): the masked image (repaint ? 0 : x) encoded ONCE
        by the frozen VAE encoder, its latents sampled by sdt_vae_posterior_sample (draw: masked_eps (B,h,w,L), else from `generator`)
        -> (masked latents bf16 NHWC (B,h,w,pad8(L)), latent mask f32 (B,h,w))."""
        dev = self.device
        stream = torch.cuda.current_stream().cuda_stream
        B, f = image.shape[0], self.vae_scale_factor
        h, w = height // f, width // f
        if self.vae_encoder is None:
            enc = ParamStore(nets.vae_encoder_spec(self.vae_config), device=dev, trainable=False)
            enc.load(self.vae_params)
            enc.prepare()
            self.vae_encoder = enc
        image = image.to(device=dev, dtype=torch.float32).contiguous()
        mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        stacked = torch.empty(2 * B, height, width, 8, dtype=torch.bfloat16, device=dev)
        lmask = torch.empty(B, h, w, dtype=torch.float32, device=dev)
        _lib.call("sdt_inpaint_mask_pixels", image.data_ptr(), mask.data_ptr(), stacked.data_ptr(), lmask.data_ptr(), B, image.shape[1],
                  height, width, 8, f, stream)
        ops.gn_arena_begin(dev)
        moments = nets.vae_encode_moments(self.vae_encoder, self.vae_config, stacked[B:])  # the masked half only
        ops.gn_arena_end(dev)
        if masked_eps is None:
            masked_eps = torch.randn(B, h, w, L, device=dev, dtype=torch.float32, generator=generator)
        elif tuple(masked_eps.shape) != (B, h, w, L):
            raise ValueError(f"Unexpected masked_eps shape, got {tuple(masked_eps.shape)}, expected {(B, h, w, L)}")
        masked_eps = masked_eps.to(device=dev, dtype=torch.float32).contiguous()
        mlat = torch.empty(B, L, h, w, dtype=torch.float32, device=dev)
        _lib.call("sdt_vae_posterior_sample", moments.data_ptr(), masked_eps.data_ptr(), mlat.data_ptr(), B, L, h, w, moments.shape[3],
                  self.scaling_factor, stream)
        cpad = (L + 7) // 8 * 8
        mlat_nhwc = torch.empty(B, h, w, cpad, dtype=torch.bfloat16, device=dev)
        _lib.call("sdt_nchw_f32_to_nhwc_bf16", mlat.data_ptr(), mlat_nhwc.data_ptr(), B, L, h, w, cpad, stream)
        return mlat_nhwc, lmask

    @torch.no_grad()
    def generate(self, prompt_ids, num_inference_steps=50, height=512, width=512, guidance_scale=7.5, latents=None,
                 neg_prompt_ids=None, generator=None, return_latents=False, guidance_rescale=0.0, image=None, mask=None,
                 masked_eps=None, control_image=None, conditioning_scale=1.0, control_negative=True, image_embeds=None, ip_scale=1.0, aux=None):
        """_generate (:160-254).  prompt_ids int (B,77) device tensor ((B,2,77) for an SDXL-mode text encoder: _sdxl_conditioning;
        pass scaling_factor=0.13025 for the SDXL VAE); latents optional f32 (B,C,h,w) initial noise; returns the
        image (B,H,W,3) float32 in [0,1] on the device (and the final latents when return_latents).  guidance_rescale in [0, 1]
        rescales the guided prediction (epsilon or v) per sample towards the std of the text prediction (diffusers
        rescale_noise_cfg, arXiv:2305.08891 §3.4; 0.7 there); 0 leaves it as it is and launches nothing extra.
        An inpainting UNet (in_channels == 2L + 1, nets.inpaint_latent_channels) needs image f32 (B,3,H,W) in [-1, 1] and mask (B,H,W)
        (1 = repaint, m >= 0.5): the latents have L channels, the masked image is encoded once (_inpaint_conditioning; after the
        initial latents, its draw comes from `generator` unless masked_eps (B,h,w,L) is given) and before every UNet call
        sdt_inpaint_pack_input assembles [latents | mask | masked-image latents] for the doubled batch from the tensor the scheduler
        kernels write.  The untouched pixels are NOT composited back over the output.  ValueError for image / mask on a plain UNet,
        their absence on an inpainting one, and wrong shapes.
        A pipeline built with controlnet= needs control_image, f32 (B, conditioning_channels, H, W) in [0, 1]: it is packed and embedded
        once (nets.controlnet_cond_embedding) and repeated for the doubled batch; every step runs the ControlNet on the doubled input
        and hands its residuals to the UNet with the per-sample scale vector f32 (2B,) = conditioning_scale, whose negative half is 0
        with control_negative=False (control on the prompt half only; diffusers' guess mode without its per-layer ramp).  ValueError for
        control_image without a ControlNet and the reverse, a wrong shape, and an inpainting UNet.
        A pipeline built with ip_adapter= needs image_embeds, f32 or bf16 (B, image_embed_dim): the image encoder's pooled embedding
        of the image prompt.  image_proj runs once on [zeros | image_embeds] - the unconditional half of the doubled batch uses zero
        image embeddings through image_proj, the published pipeline's rule - and every attn2 adds its image term with the per-sample
        scale vector f32 (2B,) = ip_scale (ops.attention_ip scale_ip).  ValueError for image_embeds without an adapter and the reverse,
        and a wrong shape.
        aux: an optional dict that receives the FIRST step's tensors for parity tests - unet_input, timesteps, ctx, pred and, with a
        ControlNet, control_embedding, control_down, control_mid and control_scale."""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if not 0.0 <= guidance_rescale <= 1.0:
            raise ValueError(f"guidance_rescale {guidance_rescale} must lie in [0, 1]")
        cn = self.controlnet
        if cn is None and control_image is not None:
            raise ValueError("control_image needs a pipeline built with controlnet=")
        if cn is not None:
            if nets.inpaint_latent_channels(self.unet_config) is not None:
                raise ValueError("a ControlNet on an inpainting UNet is not supported")
            if control_image is None:
                raise ValueError("a pipeline built with controlnet= samples from a control_image")
            want = (prompt_ids.shape[0], cn.config["conditioning_channels"], height, width)
            if not torch.is_tensor(control_image) or tuple(control_image.shape) != want:
                raise ValueError(f"Unexpected control_image shape, got {tuple(getattr(control_image, 'shape', ()))}, expected {want}")
        ipa = getattr(self, "ip_adapter", None)
        if ipa is None and image_embeds is not None:
            raise ValueError("image_embeds need a pipeline built with ip_adapter=")
        if ipa is not None:
            if image_embeds is None:
                raise ValueError("a pipeline built with ip_adapter= samples from image_embeds")
            want = (prompt_ids.shape[0], ipa.config["image_embed_dim"])
            if not torch.is_tensor(image_embeds) or tuple(image_embeds.shape) != want:
                raise ValueError(f"Unexpected image_embeds shape, got {tuple(getattr(image_embeds, 'shape', ()))}, expected {want}")
        dev = self.device
        stream = torch.cuda.current_stream().cuda_stream
        B = prompt_ids.shape[0]
        L_inp = nets.inpaint_latent_channels(self.unet_config)
        C = self.unet_config["in_channels"] if L_inp is None else L_inp
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        if L_inp is None:
            if image is not None or mask is not None or masked_eps is not None:
                raise ValueError("image / mask / masked_eps need an inpainting UNet (in_channels == 2 * out_channels + 1); this one has "
                                 f"in_channels={self.unet_config['in_channels']}")
        else:
            if image is None or mask is None:
                raise ValueError(f"an inpainting UNet (in_channels={self.unet_config['in_channels']}) samples from an image and a mask")
            if not torch.is_tensor(image) or tuple(image.shape) != (B, self.vae_config["in_channels"], height, width):
                raise ValueError(f"Unexpected image shape, got {tuple(getattr(image, 'shape', ()))}, expected "
                                 f"{(B, self.vae_config['in_channels'], height, width)}")
            if not torch.is_tensor(mask) or tuple(mask.shape) != (B, height, width):
                raise ValueError(f"Unexpected mask shape, got {tuple(getattr(mask, 'shape', ()))}, expected {(B, height, width)}")
        if latents is None:
            latents = torch.randn(B, C, h, w, device=dev, dtype=torch.float32, generator=generator)
        elif tuple(latents.shape) != (B, C, h, w):
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {(B, C, h, w)}")
        added = None
        if nets.sdxl_conditioning(self.text_encoder_config):
            context, added = self._sdxl_conditioning(prompt_ids, neg_prompt_ids, height, width)
        elif self.unet_config.get("addition_embed_type") == "text_time":
            raise ValueError("a text_time (SDXL) UNet samples with an SDXL-mode text encoder (nets.dual_clip_config(sdxl_conditioning=True))")
        else:
            if neg_prompt_ids is None:
                neg_prompt_ids = self._uncond_ids(B, prompt_ids.shape[-1])
            self.unet.prepare()
            self.text_encoder.prepare()
            ids = torch.cat([neg_prompt_ids.to(device=dev, dtype=torch.int32), prompt_ids.to(device=dev, dtype=torch.int32)])
            context = nets.clip_text_forward(self.text_encoder, self.text_encoder_config, ids).detach()  # [negative | prompt] (:191)

        lat = (latents.to(device=dev, dtype=torch.float32) * self.scheduler.init_noise_sigma).contiguous().clone()
        cpad = (C + 7) // 8 * 8
        x_in = torch.empty(2 * B, h, w, cpad, dtype=torch.bfloat16, device=dev)
        for half in (x_in[:B], x_in[B:]):
            _lib.call("sdt_nchw_f32_to_nhwc_bf16", lat.data_ptr(), half.data_ptr(), B, C, h, w, cpad, stream)
        x_lat = x_in  # what the scheduler kernels write: the latents' channels, doubled
        if L_inp is not None:
            mlat_nhwc, lmask = self._inpaint_conditioning(image, mask, masked_eps, generator, L_inp, height, width)
            x_in = torch.empty(2 * B, h, w, (2 * C + 1 + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)
        t_dev = torch.empty(2 * B, dtype=torch.int32, device=dev)
        embedding = scale = None
        if cn is not None:  # the hint: packed and embedded once, repeated for [negative | prompt]
            cn.store.prepare()
            ci = control_image.to(device=dev, dtype=torch.float32).contiguous()
            hint = torch.empty(B, height, width, (ci.shape[1] + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)
            _lib.call("sdt_nchw_f32_to_nhwc_bf16", ci.data_ptr(), hint.data_ptr(), B, ci.shape[1], height, width, hint.shape[3], stream)
            ops.gn_arena_begin(dev)
            e = nets.controlnet_cond_embedding(cn.store, cn.config, hint)
            ops.gn_arena_end(dev)
            embedding = torch.cat([e, e]).contiguous()
            scale = torch.full((2 * B,), float(conditioning_scale), dtype=torch.float32, device=dev)
            if not control_negative:
                scale[:B] = 0.0
        ip = None
        if ipa is not None:  # the image tokens: projected once for [zeros | image_embeds]
            ipa.store.prepare()
            emb = torch.zeros(2 * B, image_embeds.shape[1], dtype=torch.bfloat16, device=dev)
            emb[B:].copy_(image_embeds.to(device=dev))
            ip = (ipa.store, nets.ip_adapter_tokens(ipa.store, ipa.config, emb).detach(),
                  torch.full((2 * B,), float(ip_scale), dtype=torch.float32, device=dev))
        for step, t in enumerate(self.scheduler.set_timesteps(num_inference_steps)):
            t_dev.fill_(int(t))
            if L_inp is not None:
                _lib.call("sdt_inpaint_pack_input", x_lat.data_ptr(), mlat_nhwc.data_ptr(), lmask.data_ptr(), x_in.data_ptr(), 2 * B, B, C,
                          h, w, cpad, mlat_nhwc.shape[3], x_in.shape[3], stream)
            ops.gn_arena_begin(dev)
            control = None
            if cn is not None:
                down, mid = nets.controlnet_forward_embedded(cn.store, cn.config, x_in, t_dev, context, embedding, added)
                control = (down, mid, scale)
            pred = nets.unet_forward(self.unet, self.unet_config, x_in, t_dev, context, added, control=control, ip=ip)
            ops.gn_arena_end(dev)
            if aux is not None and step == 0:  # the first step's tensors, for parity tests
                aux.update(unet_input=x_in.clone(), timesteps=t_dev.clone(), ctx=context, pred=pred.clone())
                if ip is not None:
                    aux.update(ip_tokens=ip[1], ip_scale=ip[2])
                if cn is not None:
                    aux.update(control_embedding=embedding, control_down=[d.clone() for d in down], control_mid=mid.clone(), control_scale=scale)
            self.scheduler.cfg_step(pred, lat, x_lat, t, guidance_scale, guidance_rescale)  # guidance + x_t -> x_{t-1} + next input

        z = torch.empty(B, h, w, cpad, dtype=torch.bfloat16, device=dev)
        scaled = lat * (1.0 / self.scaling_factor)
        _lib.call("sdt_nchw_f32_to_nhwc_bf16", scaled.data_ptr(), z.data_ptr(), B, C, h, w, cpad, stream)
        ops.gn_arena_begin(dev)
        img = nets.vae_decode(self.vae_decoder, self.vae_config, z)
        ops.gn_arena_end(dev)
        image = (img[..., : self.vae_config["in_channels"]].float() / 2 + 0.5).clamp(0, 1)
        return (image, lat) if return_latents else image
