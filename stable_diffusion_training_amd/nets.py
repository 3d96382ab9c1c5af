"""The three networks train_step runs, expressed over the HIP operators of ops.py.

  * UNet2DCondition  - diffusers 0.21.4 FlaxUNet2DConditionModel.__call__ (training_utils.py:678-684)
  * VAE encoder      - diffusers 0.21.4 FlaxAutoencoderKL.encode (training_utils.py:574-579), frozen / no grad
  * VAE decoder      - FlaxAutoencoderKL.decode, sampling path only (models/pipeline_flax_stable_diffusion.py:245-249)
  * CLIP text model  - transformers FlaxCLIPTextModel (training_utils.py:635-640), trained

Parameter trees use the diffusers-Flax names and layouts so `create_mask` patterns and
checkpoints stay drop-in.  `*_spec(cfg)` return the leaves as an ordered (path, shape) list in forward execution
order: the flat gradient buffer is laid out in that order, so backward completes all-reduce buckets back to front.
Activations are NHWC bf16 with channels padded to a multiple of 8 (4-channel latents / 3-channel pixels -> 8).
"""
import contextlib
import math
from typing import Callable, NamedTuple

import torch

from . import _lib, ops

# ----------------------------------------------------------------------------- configs (diffusers config.json keys)
_UNET_DEFAULTS = dict(in_channels=4, out_channels=4, layers_per_block=2, flip_sin_to_cos=True, freq_shift=0,
                      norm_num_groups=32, use_linear_projection=False, transformer_layers_per_block=1,
                      addition_embed_type=None, addition_time_embed_dim=None, projection_class_embeddings_input_dim=None)

UNET_CONFIGS = {
    "sd15": dict(down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",),
                 up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
                 block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8, cross_attention_dim=768),
    "sd21": dict(down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",),
                 up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
                 block_out_channels=(320, 640, 1280, 1280), attention_head_dim=(5, 10, 20, 20),
                 cross_attention_dim=1024, use_linear_projection=True),
    "sdxl": dict(down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
                 up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
                 block_out_channels=(320, 640, 1280), attention_head_dim=(5, 10, 20), cross_attention_dim=2048,
                 use_linear_projection=True, transformer_layers_per_block=(1, 2, 10), addition_embed_type="text_time",
                 addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816),
    "tiny": dict(down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
                 block_out_channels=(32, 64), attention_head_dim=2, cross_attention_dim=48, layers_per_block=1),
}
VAE_CONFIGS = {
    "sd": dict(in_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32),
    "tiny": dict(in_channels=3, latent_channels=4, block_out_channels=(32, 32, 64, 64), layers_per_block=1, norm_num_groups=32),
}
CLIP_CONFIGS = {
    "clip_l": dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                   max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5),
    # SD2.1's text tower (OpenCLIP ViT-H/14 text model, penultimate-layer export: 23 layers) and SDXL's second tower (bigG, 32 layers)
    "openclip_h": dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                       max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5),
    "openclip_bigg": dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20,
                          max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5),
    "tiny": dict(vocab_size=1000, hidden_size=48, intermediate_size=96, num_hidden_layers=2, num_attention_heads=3,
                 max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5),
}


def unet_config(name="sd15", **over):
    cfg = dict(_UNET_DEFAULTS)
    cfg.update(UNET_CONFIGS[name])
    cfg.update(over)
    return cfg


def vae_config(name="sd"):
    return dict(VAE_CONFIGS[name])


def clip_config(name="clip_l"):
    return dict(CLIP_CONFIGS[name])


def _per_block(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


def _pad8(c):
    return (c + 7) // 8 * 8


def inpaint_latent_channels(cfg):
    """L for an inpainting UNet - in_channels == 2 * out_channels + 1, the input [noisy latents | mask | masked-image latents]
    (include/sdt.h "INPAINTING") - else None."""
    cin, cout = cfg.get("in_channels"), cfg.get("out_channels")
    if cin is None or cout is None:
        return None
    return int(cout) if int(cin) == 2 * int(cout) + 1 else None


def widen_conv_in(unet_params, unet_config, in_channels):
    """A checkpoint with more input channels, the usual way (host side): conv_in/kernel (kh,kw,cin,cout) gains zero rows up to
    in_channels, so the widened UNet computes what the narrow one did whatever the new channels hold; every other leaf is shared.
    unet_params: the flat {"a/b/kernel": array} tree or the nested Flax one, torch tensors or numpy arrays.  Returns (params, config)
    copies with config["in_channels"] = in_channels.  ValueError for a target narrower than the kernel."""
    nested = "conv_in" in unet_params and isinstance(unet_params["conv_in"], dict)
    k = unet_params["conv_in"]["kernel"] if nested else unet_params["conv_in/kernel"]
    cin = int(k.shape[2])
    if cin != int(unet_config["in_channels"]):
        raise ValueError(f"conv_in/kernel has {cin} input channels, the config says in_channels={unet_config['in_channels']}")
    if not isinstance(in_channels, int) or in_channels < cin:
        raise ValueError(f"widen_conv_in: in_channels={in_channels!r} is narrower than the kernel's {cin}")
    shape = (k.shape[0], k.shape[1], in_channels, k.shape[3])
    if torch.is_tensor(k):
        wide = torch.zeros(shape, dtype=k.dtype)
        wide[:, :, :cin] = k
    else:
        import numpy as np
        k = np.asarray(k)
        wide = np.zeros(shape, dtype=k.dtype)
        wide[:, :, :cin] = k
    params = dict(unet_params)
    if nested:
        params["conv_in"] = dict(unet_params["conv_in"], kernel=wide)
    else:
        params["conv_in/kernel"] = wide
    return params, dict(unet_config, in_channels=in_channels)


# ----------------------------------------------------------------------------- parameter specs (forward order)
class _Spec(list):
    def __init__(self, *a):
        super().__init__(*a)
        self.groups = {}  # key -> [index in the list where the group goes, [(kernel leaves), ...], [(bias leaves), ...]]

    def _defer(self, key, kernels, biases=()):
        g = self.groups.setdefault(key, [len(self), [], []])
        g[1] += kernels
        g[2] += biases

    def finish(self):
        """The leaf list.  Dense layers that consume the SAME tensor in many blocks - the time-embedding projection of every
        ResBlock (input silu(temb)) and the cross-attention to_k / to_v of every transformer block (input: the text context) -
        are placed back to back per output width, kernels then biases, at the position of the group's first member, so that
        ops.linear_multi runs each width as ONE GEMM per pass (SD1.5: 22 + 32 projections, 162 launches per step -> 18).  A
        group's gradients complete when the backward reaches its first member, which is where the group sits in the buffers,
        so the exchange buckets still complete in buffer order.  Names and shapes are the diffusers ones; only positions move."""
        out = list(self)
        for at, kernels, biases in sorted(self.groups.values(), key=lambda g: -g[0]):
            out[at:at] = kernels + biases
        return out

    def conv(self, p, cin, cout, k=3):
        self.append((p + "/kernel", (k, k, cin, cout)))
        self.append((p + "/bias", (cout,)))

    def dense(self, p, cin, cout, bias=True):
        self.append((p + "/kernel", (cin, cout)))
        if bias:
            self.append((p + "/bias", (cout,)))

    def norm(self, p, c):
        self.append((p + "/scale", (c,)))
        self.append((p + "/bias", (c,)))

    def resnet(self, p, cin, cout, temb):
        self.norm(p + "/norm1", cin)
        self.conv(p + "/conv1", cin, cout)
        if temb:  # placed next to the other projections of the same width (finish())
            q = p + "/time_emb_proj"
            self._defer(("temb", cout), [(q + "/kernel", (temb, cout))], [(q + "/bias", (cout,))])
        self.norm(p + "/norm2", cout)
        self.conv(p + "/conv2", cout, cout)
        if cin != cout:
            self.conv(p + "/conv_shortcut", cin, cout, k=1)

    def transformer(self, p, c, ctx, depth, lin):
        self.norm(p + "/norm", c)
        if lin:
            self.dense(p + "/proj_in", c, c)
        else:
            self.conv(p + "/proj_in", c, c, k=1)
        for k in range(depth):
            b = f"{p}/transformer_blocks_{k}"
            self.norm(b + "/norm1", c)
            for n, kd in (("to_q", c), ("to_k", c), ("to_v", c)):
                self.dense(f"{b}/attn1/{n}", kd, c, bias=False)
            self.dense(f"{b}/attn1/to_out_0", c, c)
            self.norm(b + "/norm2", c)
            self.dense(f"{b}/attn2/to_q", c, c, bias=False)
            self._defer(("kv", c), [(f"{b}/attn2/to_k/kernel", (ctx, c)), (f"{b}/attn2/to_v/kernel", (ctx, c))])
            self.dense(f"{b}/attn2/to_out_0", c, c)
            self.norm(b + "/norm3", c)
            self.dense(f"{b}/ff/net_0/proj", c, 8 * c)
            self.dense(f"{b}/ff/net_2", 4 * c, c)
        if lin:
            self.dense(p + "/proj_out", c, c)
        else:
            self.conv(p + "/proj_out", c, c, k=1)


def _spec_time_embedding(s, cfg):
    """time_embedding (and add_embedding for text_time): the first leaves of a UNet and of a ControlNet."""
    boc = cfg["block_out_channels"]
    temb = boc[0] * 4
    s.dense("time_embedding/linear_1", boc[0], temb)
    s.dense("time_embedding/linear_2", temb, temb)
    if cfg["addition_embed_type"] == "text_time":
        s.dense("add_embedding/linear_1", cfg["projection_class_embeddings_input_dim"], temb)
        s.dense("add_embedding/linear_2", temb, temb)


def _spec_encoder(s, cfg):
    """conv_in, the down blocks and the mid block in forward order: the part of the UNet a ControlNet repeats under the same names."""
    boc = cfg["block_out_channels"]
    nb, lpb, ctx, lin = len(boc), cfg["layers_per_block"], cfg["cross_attention_dim"], cfg["use_linear_projection"]
    temb = boc[0] * 4
    depth = _per_block(cfg["transformer_layers_per_block"], nb)
    s.conv("conv_in", cfg["in_channels"], boc[0])
    out_ch = boc[0]
    for i, t in enumerate(cfg["down_block_types"]):
        in_ch, out_ch = out_ch, boc[i]
        for j in range(lpb):
            s.resnet(f"down_blocks_{i}/resnets_{j}", in_ch if j == 0 else out_ch, out_ch, temb)
            if t == "CrossAttnDownBlock2D":
                s.transformer(f"down_blocks_{i}/attentions_{j}", out_ch, ctx, depth[i], lin)
        if i != nb - 1:
            s.conv(f"down_blocks_{i}/downsamplers_0/conv", out_ch, out_ch)
    mid = boc[-1]
    s.resnet("mid_block/resnets_0", mid, mid, temb)
    s.transformer("mid_block/attentions_0", mid, ctx, depth[-1], lin)
    s.resnet("mid_block/resnets_1", mid, mid, temb)


def unet_spec(cfg):
    s = _Spec()
    boc = cfg["block_out_channels"]
    nb, lpb, ctx, lin = len(boc), cfg["layers_per_block"], cfg["cross_attention_dim"], cfg["use_linear_projection"]
    temb = boc[0] * 4
    depth = _per_block(cfg["transformer_layers_per_block"], nb)
    _spec_time_embedding(s, cfg)
    _spec_encoder(s, cfg)
    rev, rdepth = list(reversed(boc)), list(reversed(depth))
    out_ch = rev[0]
    for i, t in enumerate(cfg["up_block_types"]):
        prev, out_ch = out_ch, rev[i]
        in_ch = rev[min(i + 1, nb - 1)]
        for j in range(lpb + 1):
            skip = in_ch if j == lpb else out_ch
            s.resnet(f"up_blocks_{i}/resnets_{j}", (prev if j == 0 else out_ch) + skip, out_ch, temb)
            if t == "CrossAttnUpBlock2D":
                s.transformer(f"up_blocks_{i}/attentions_{j}", out_ch, ctx, rdepth[i], lin)
        if i != nb - 1:
            s.conv(f"up_blocks_{i}/upsamplers_0/conv", out_ch, out_ch)
    s.norm("conv_norm_out", boc[0])
    s.conv("conv_out", boc[0], cfg["out_channels"])
    return s.finish()


class ControlNet:
    """A ControlNet as the training state and the sampling pipeline hold it: its ParamStore and its config (controlnet_config)."""

    def __init__(self, store, config):
        self.store, self.config = store, config


def controlnet_config(unet_cfg, conditioning_embedding_out_channels=(16, 32, 96, 256), conditioning_channels=3, vae_downscale=8):
    """The UNet's config plus diffusers' two ControlNet keys.  The conditioning image is at pixel size and the embedder halves it once
    per entry after the first, down to the latent grid: len(conditioning_embedding_out_channels) - 1 must be log2(vae_downscale) (3 for
    every VAE here).  Entries are activation widths and must be multiples of 8.  ValueError otherwise, and for an inpainting UNet."""
    ch = tuple(int(c) for c in conditioning_embedding_out_channels)
    halvings = int(vae_downscale).bit_length() - 1
    if vae_downscale < 1 or 2 ** halvings != vae_downscale:
        raise ValueError(f"controlnet_config: vae_downscale={vae_downscale!r} must be a power of two")
    if len(ch) - 1 != halvings:
        raise ValueError(f"controlnet_config: conditioning_embedding_out_channels has {len(ch)} entries; the embedder halves the "
                         f"conditioning image {len(ch) - 1} times and the VAE's downscale {vae_downscale} needs {halvings} ({halvings + 1} entries)")
    if any(c < 8 or c % 8 for c in ch):
        raise ValueError(f"controlnet_config: conditioning_embedding_out_channels={ch} must be positive multiples of 8")
    if not isinstance(conditioning_channels, int) or conditioning_channels < 1:
        raise ValueError(f"controlnet_config: conditioning_channels={conditioning_channels!r} must be a positive integer")
    if inpaint_latent_channels(unet_cfg) is not None:
        raise ValueError("controlnet_config: a ControlNet on an inpainting UNet is not supported")
    return dict(unet_cfg, conditioning_embedding_out_channels=ch, conditioning_channels=conditioning_channels)


def skip_shapes(cfg, h=1, w=1):
    """(channels, height, width) of the UNet's skip tensors for (h, w) latents, in the order unet_forward appends them."""
    boc = cfg["block_out_channels"]
    out = [(boc[0], h, w)]
    for i in range(len(boc)):
        out += [(boc[i], h, w)] * cfg["layers_per_block"]
        if i != len(boc) - 1:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1  # the 3x3 stride-2 pad-1 downsampler
            out.append((boc[i], h, w))
    return out


def _skip_channels(cfg):
    return [c for c, _, _ in skip_shapes(cfg)]


def controlnet_spec(cfg):
    """Leaves of diffusers' FlaxControlNetModel: the UNet's time embedding, conv_in, down and mid blocks under the UNet's names (the
    helpers unet_spec itself is built from), the conditioning embedder, one 1x1 zero convolution per skip tensor and one for the mid block."""
    s = _Spec()
    boc = cfg["block_out_channels"]
    _spec_time_embedding(s, cfg)
    ch = cfg["conditioning_embedding_out_channels"]
    e = "controlnet_cond_embedding"
    s.conv(e + "/conv_in", cfg["conditioning_channels"], ch[0])
    for k in range(len(ch) - 1):
        s.conv(f"{e}/blocks_{2 * k}", ch[k], ch[k])
        s.conv(f"{e}/blocks_{2 * k + 1}", ch[k], ch[k + 1])  # stride 2
    s.conv(e + "/conv_out", ch[-1], boc[0])
    _spec_encoder(s, cfg)
    for i, c in enumerate(_skip_channels(cfg)):
        s.conv(f"controlnet_down_blocks_{i}", c, c, k=1)
    s.conv("controlnet_mid_block", boc[-1], boc[-1], k=1)
    return s.finish()


def controlnet_zero_leaves(cfg):
    """The leaves a fresh ControlNet holds as zeros: the embedder's conv_out and every zero convolution, kernels and biases."""
    heads = ["controlnet_cond_embedding/conv_out", "controlnet_mid_block"] + [f"controlnet_down_blocks_{i}" for i in range(len(_skip_channels(cfg)))]
    return [f"{h}/{leaf}" for h in heads for leaf in ("kernel", "bias")]


def controlnet_from_unet(unet_params, cfg, seed=0):
    """A fresh ControlNet for a UNet, as diffusers' from_unet builds it (host tree, flat paths): the leaves it shares with the UNet are
    copies of the UNet's, the embedder's convolutions are seeded random (init_params) and conv_out, every controlnet_down_blocks_* and
    controlnet_mid_block are zero - so the ControlNet's residuals are zero and the UNet computes what it did without it.
    unet_params: flat or nested tree, torch tensors or numpy arrays."""
    from .checkpoint import flatten_if_nested
    spec, unet_params = controlnet_spec(cfg), flatten_if_nested(unet_params)
    fresh = init_params([(p, shp) for p, shp in spec if p.startswith("controlnet_")], seed)
    zero = set(controlnet_zero_leaves(cfg))
    out = {}
    for p, shp in spec:
        if p in zero:
            out[p] = torch.zeros(shp)
        elif p in fresh:
            out[p] = fresh[p]
        else:
            v = unet_params[p]
            v = v.detach().to(torch.float32).cpu().clone() if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float32)
            if tuple(v.shape) != tuple(shp):
                raise ValueError(f"controlnet_from_unet: {p} has shape {tuple(v.shape)} in the UNet, the ControlNet's config says {tuple(shp)}")
            out[p] = v
    return out


class IPAdapter:
    """An IP-Adapter as the training state and the sampling pipeline hold it: its ParamStore and its config (ip_adapter_config)."""

    def __init__(self, store, config):
        self.store, self.config = store, config


def ip_adapter_config(unet_cfg, image_embed_dim=1024, num_tokens=4):
    """The UNet's config plus the two keys of an IP-Adapter (Ye et al. 2023): image_embed_dim E, the width of the image encoder's pooled
    embedding (1024 for CLIP ViT-H/14, 1280 for ViT-bigG), and num_tokens T, the image tokens image_proj makes of it (4; 16 for the
    Plus variants' token count).  ValueError for E not a positive multiple of 8, T outside 1..16 (what sdt_ip_attention_* serve) and
    an inpainting UNet."""
    if not isinstance(image_embed_dim, int) or image_embed_dim < 8 or image_embed_dim % 8:
        raise ValueError(f"ip_adapter_config: image_embed_dim={image_embed_dim!r} must be a positive multiple of 8")
    if not isinstance(num_tokens, int) or not 1 <= num_tokens <= 16:
        raise ValueError(f"ip_adapter_config: num_tokens={num_tokens!r} must be 1..16")
    if inpaint_latent_channels(unet_cfg) is not None:
        raise ValueError("ip_adapter_config: an IP-Adapter on an inpainting UNet is not supported")
    return dict(unet_cfg, image_embed_dim=image_embed_dim, num_tokens=num_tokens)


def ip_adapter_blocks(cfg):
    """{width: ["<block>/attn2", ...]} of the UNet's cross-attentions, widths in order of first use, blocks in forward order."""
    groups = {}
    for p, shp in unet_spec(cfg):
        if p.endswith("/attn2/to_k/kernel"):
            groups.setdefault(shp[1], []).append(p[: -len("/to_k/kernel")])
    return groups


def ip_adapter_spec(cfg):
    """Leaves of an IP-Adapter: image_proj/proj (E -> T * Dc, with bias) and image_proj/norm (LayerNorm over Dc), then to_k_ip / to_v_ip
    (Dc -> C, no bias) of every cross-attention, the blocks of one channel width back to back as [k | v] pairs: the image tokens are
    projected by ONE GEMM per width (ops.linear_multi), as _context_projections does for the text, and each block reads a column slice."""
    E, T, Dc = cfg["image_embed_dim"], cfg["num_tokens"], cfg["cross_attention_dim"]
    spec = [("image_proj/proj/kernel", (E, T * Dc)), ("image_proj/proj/bias", (T * Dc,)),
            ("image_proj/norm/scale", (Dc,)), ("image_proj/norm/bias", (Dc,))]
    for width, names in ip_adapter_blocks(cfg).items():
        for n in names:
            spec += [(n + "/to_k_ip/kernel", (Dc, width)), (n + "/to_v_ip/kernel", (Dc, width))]
    return spec


def ip_adapter_from_unet(unet_params, cfg, seed=0):
    """A fresh IP-Adapter for a UNet, as the published training script initialises it (host tree, flat paths): to_k_ip / to_v_ip are
    copies of the UNet's attn2 to_k / to_v, image_proj is drawn from the seed (init_params).  unet_params: flat or nested tree, torch
    tensors or numpy arrays."""
    from .checkpoint import flatten_if_nested
    spec, unet_params = ip_adapter_spec(cfg), flatten_if_nested(unet_params)
    out = init_params([(p, shp) for p, shp in spec if p.startswith("image_proj/")], seed)
    for p, shp in spec:
        if p in out:
            continue
        src = p.replace("/to_k_ip/", "/to_k/").replace("/to_v_ip/", "/to_v/")
        v = unet_params[src]
        v = v.detach().to(torch.float32).cpu().clone() if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float32)
        if tuple(v.shape) != tuple(shp):
            raise ValueError(f"ip_adapter_from_unet: {src} has shape {tuple(v.shape)} in the UNet, the adapter's config says {tuple(shp)}")
        out[p] = v
    return out


class SideNetwork(NamedTuple):
    """What the training layer, save_model and the sampling pipeline need to know of a network with a ParamStore of its own that is
    trained on the frozen UNet and selected by one batch key.  Everything that handles such a network is written once over this
    description (training_utils: the builder's argument, the store it builds, train_step's refusals and prepare(); checkpoint.save_model;
    StableDiffusionPipeline); the forward call and the aux taps differ in kind and stay explicit in train_step.
    The rules, for a network `name`: the builder takes name=None or dict(config=nets.<name>_config(...)[, params=host tree]) - a loaded
    network, or one initialised from the UNet (from_unet).  Both base stores are built frozen; the UNet state's field `name` holds the
    wrapper (store + config), whose store the UNet's settings configure and which steps; the text encoder only runs its forward.
    Refused beside lora=, new_tokens= and another side network, on an inpainting UNet, with a reducer, and with a config that does not
    add the keys `adds` to the UNet's or differs from it in one of `same`.  The batches of such a state carry batch_key."""
    name: str            # the TrainState / pipeline field, the builder's and the pipeline's argument
    label: str           # "ControlNet": the head of train_step's messages
    article: str         # "a ControlNet"
    the: str             # "the ControlNet": how messages name the network once it is known
    batch_key: str       # the batch entry its step reads
    adds: tuple          # the config keys beyond the UNet's, in the order <name>_config takes them
    same: tuple          # the config keys that must equal the UNet's
    config: Callable     # <name>_config(unet_cfg, *(cfg[k] for k in adds), **config_kwargs(models)): ValueError for a bad config
    config_kwargs: Callable
    spec: Callable       # <name>_spec(cfg)
    from_unet: Callable  # <name>_from_unet(unet weights, cfg)
    wrapper: type        # (store, config)
    marker: str          # the attribute of a trained store that holds the config: save_model refuses such a store as UNet weights
    beside: tuple        # the builder's refusals of other arguments: ((argument names, message), ...), in order


def _controlnet_config_kwargs(models):
    return dict(vae_downscale=2 ** (len(models["vae"]["config"]["block_out_channels"]) - 1) if "vae" in models else 8)


CONTROLNET = SideNetwork(
    "controlnet", "ControlNet", "a ControlNet", "the ControlNet", "conditioning_pixel_values",
    ("conditioning_embedding_out_channels", "conditioning_channels"),
    ("block_out_channels", "down_block_types", "layers_per_block", "in_channels", "cross_attention_dim", "attention_head_dim",
     "use_linear_projection", "transformer_layers_per_block", "norm_num_groups", "addition_embed_type"),
    controlnet_config, _controlnet_config_kwargs, controlnet_spec, controlnet_from_unet, ControlNet, "controlnet_config",
    ((("lora", "new_tokens"), "controlnet: a ControlNet beside a LoRA adapter or new tokens is not supported"),))
IP_ADAPTER = SideNetwork(
    "ip_adapter", "IP-Adapter", "an IP-Adapter", "the adapter", "image_embeds", ("image_embed_dim", "num_tokens"),
    ("block_out_channels", "down_block_types", "up_block_types", "layers_per_block", "cross_attention_dim", "attention_head_dim",
     "transformer_layers_per_block"),
    ip_adapter_config, lambda models: {}, ip_adapter_spec, ip_adapter_from_unet, IPAdapter, "ip_adapter_config",
    ((("lora",), "ip_adapter: an IP-Adapter beside a LoRA adapter is not supported"),
     (("new_tokens",), "ip_adapter: an IP-Adapter beside new tokens is not supported"),
     (("controlnet",), "ip_adapter: an IP-Adapter beside a ControlNet is not supported")))
# in the order a state is searched for them (TrainState.stepping) and train_step refuses them; a later one names the earlier ones it
# cannot stand beside
SIDE_NETWORKS = (CONTROLNET, IP_ADAPTER)


def time_emb_groups(leaves):
    """{width: [resnet path, ...]} in buffer order, from the leaves of a UNet parameter store."""
    groups = {}
    for p in leaves:
        if p.endswith("/time_emb_proj/kernel"):
            groups.setdefault(leaves[p].shape[1], []).append(p[: -len("/time_emb_proj/kernel")])
    return groups


def vae_encoder_spec(cfg):
    s = _Spec()
    boc = cfg["block_out_channels"]
    s.conv("encoder/conv_in", cfg["in_channels"], boc[0])
    out_ch = boc[0]
    for i in range(len(boc)):
        in_ch, out_ch = out_ch, boc[i]
        for j in range(cfg["layers_per_block"]):
            s.resnet(f"encoder/down_blocks_{i}/resnets_{j}", in_ch if j == 0 else out_ch, out_ch, 0)
        if i != len(boc) - 1:
            s.conv(f"encoder/down_blocks_{i}/downsamplers_0/conv", out_ch, out_ch)
    c = boc[-1]
    s.resnet("encoder/mid_block/resnets_0", c, c, 0)
    a = "encoder/mid_block/attentions_0"
    s.norm(a + "/group_norm", c)
    for n in ("query", "key", "value", "proj_attn"):
        s.dense(f"{a}/{n}", c, c)
    s.resnet("encoder/mid_block/resnets_1", c, c, 0)
    s.norm("encoder/conv_norm_out", c)
    s.conv("encoder/conv_out", c, 2 * cfg["latent_channels"])
    s.conv("quant_conv", 2 * cfg["latent_channels"], 2 * cfg["latent_channels"], k=1)
    return list(s)


def vae_decoder_spec(cfg):
    """Decoder half (+post_quant_conv) of FlaxAutoencoderKL, forward order (sampling path)."""
    s = _Spec()
    boc = tuple(cfg["block_out_channels"])[::-1]
    lc = cfg["latent_channels"]
    s.conv("post_quant_conv", lc, lc, k=1)
    s.conv("decoder/conv_in", lc, boc[0])
    c = boc[0]
    s.resnet("decoder/mid_block/resnets_0", c, c, 0)
    a = "decoder/mid_block/attentions_0"
    s.norm(a + "/group_norm", c)
    for n in ("query", "key", "value", "proj_attn"):
        s.dense(f"{a}/{n}", c, c)
    s.resnet("decoder/mid_block/resnets_1", c, c, 0)
    out_ch = boc[0]
    for i in range(len(boc)):
        in_ch, out_ch = out_ch, boc[i]
        for j in range(cfg["layers_per_block"] + 1):
            s.resnet(f"decoder/up_blocks_{i}/resnets_{j}", in_ch if j == 0 else out_ch, out_ch, 0)
        if i != len(boc) - 1:
            s.conv(f"decoder/up_blocks_{i}/upsamplers_0/conv", out_ch, out_ch)
    s.norm("decoder/conv_norm_out", boc[-1])
    s.conv("decoder/conv_out", boc[-1], cfg["in_channels"])
    return list(s)


def clip_text_spec(cfg, prefix=""):
    if "towers" in cfg:  # SDXL: two text towers in one parameter store (dual_clip_config)
        return [leaf for i, c in enumerate(cfg["towers"]) for leaf in clip_text_spec(c, cfg["prefixes"][i])]
    s = _Spec()
    d, f = cfg["hidden_size"], cfg["intermediate_size"]
    s.append((prefix + "text_model/embeddings/token_embedding/embedding", (cfg["vocab_size"], d)))
    s.append((prefix + "text_model/embeddings/position_embedding/embedding", (cfg["max_position_embeddings"], d)))
    for i in range(cfg["num_hidden_layers"]):
        b = f"{prefix}text_model/encoder/layers/{i}"
        s.norm(b + "/layer_norm1", d)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s.dense(f"{b}/self_attn/{n}", d, d)
        s.norm(b + "/layer_norm2", d)
        s.dense(b + "/mlp/fc1", d, f)
        s.dense(b + "/mlp/fc2", f, d)
    s.norm(prefix + "text_model/final_layer_norm", d)
    if cfg.get("with_projection"):  # transformers FlaxCLIPTextModelWithProjection: Dense(projection_dim, use_bias=False)
        s.dense(prefix + "text_projection", d, cfg["projection_dim"], bias=False)
    return list(s)


def dual_clip_config(first="clip_l", second="openclip_bigg", sdxl_conditioning=False):
    """SDXL conditions its UNet on the hidden states of two text towers concatenated along the feature axis (768 + 1280 = 2048 =
    cross_attention_dim).  The reference's train_step holds ONE text-encoder state (training_utils.py:635-640) and cannot drive
    SDXL (SURVEY.md §8(d) note); here both towers live in one parameter store under the diffusers sub-folder names, so the
    step's signature, optimizer sweep and gradient exchange are unchanged.  first / second: CLIP_CONFIGS names or config dicts.

    sdxl_conditioning=True: SDXL's own conditioning (sdxl_text_forward).  Each tower's context is hidden_states[-2] (hidden_layer=-2:
    the residual stream entering the last layer, no final LayerNorm), and the second tower also yields the pooled text embedding,
    text_projection(final_layer_norm(x) at the EOS token) - it gains the text_projection leaf (with_projection, projection_dim =
    its width unless given) and eos_token_id (2 unless given: the argmax rule of SDXL's released configs)."""
    towers = [dict(t) if isinstance(t, dict) else clip_config(t) for t in (first, second)]
    cfg = dict(towers=towers, prefixes=["text_encoder/", "text_encoder_2/"])
    if sdxl_conditioning:
        for t in towers:
            t["hidden_layer"] = -2
        towers[1]["with_projection"] = True
        towers[1].setdefault("projection_dim", towers[1]["hidden_size"])
        towers[1].setdefault("eos_token_id", 2)
        cfg["sdxl_conditioning"] = True
    return cfg


def sdxl_conditioning(cfg):
    """True for a two-tower text-encoder config in SDXL mode (dual_clip_config(sdxl_conditioning=True), or an SDXL checkpoint)."""
    return bool(cfg.get("sdxl_conditioning")) and "towers" in cfg


def _context_layers(tower):
    """Encoder layers the context passes through: hidden_states[hidden_layer] (hidden_states[0] is the embedding output)."""
    n = tower["num_hidden_layers"]
    hl = tower.get("hidden_layer", -1)
    k = n + 1 + hl if hl < 0 else hl
    if not 1 <= k <= n:
        raise ValueError(f"hidden_layer={hl} selects no encoder layer of a {n}-layer tower")
    return k


def unused_text_leaves(cfg):
    """Leaves an SDXL-mode forward never reads: the layers after the context of a tower without the pooled output, and that tower's
    final LayerNorm (CLIP-L).  Their gradients must be zero every step (ParamStore.mark_unused)."""
    if not sdxl_conditioning(cfg):
        return []
    out = []
    for t, pre in zip(cfg["towers"], cfg["prefixes"]):
        if t.get("with_projection"):
            continue
        k = _context_layers(t)
        dead = tuple(f"{pre}text_model/encoder/layers/{i}/" for i in range(k, t["num_hidden_layers"])) + (pre + "text_model/final_layer_norm/",)
        out += [p for p, _ in clip_text_spec(t, pre) if p.startswith(dead)]
    return out


def init_params(spec, seed=0):
    """Synthetic weights (no checkpoints offline): fan-in scaled normal kernels, ~1 norm scales, small biases."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in sorted(spec):
        leaf = k.rsplit("/", 1)[1]
        if leaf == "kernel":
            out[k] = torch.randn(shp, generator=g) / math.sqrt(math.prod(shp[:-1]))
        elif leaf == "embedding":
            out[k] = torch.randn(shp, generator=g) * 0.02
        elif leaf == "scale":
            out[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            out[k] = 0.02 * torch.randn(shp, generator=g)
    return out


# ----------------------------------------------------------------------------- UNet
def timestep_embedding(t, dim, flip_sin_to_cos=True, freq_shift=0.0):
    out = torch.empty(t.shape[0], dim, dtype=torch.bfloat16, device=t.device)
    _lib.call("sdt_timestep_embedding", t.data_ptr(), out.data_ptr(), t.shape[0], dim, int(flip_sin_to_cos), float(freq_shift),
              torch.cuda.current_stream().cuda_stream)
    return out


def _time_emb_projections(st, temb_act):
    """Linear(silu(temb)) of every ResBlock (diffusers FlaxResnetBlock2D.time_emb_proj): one GEMM per channel width where the
    projections of that width are laid out back to back (unet_spec), column slices handed to the blocks; one GEMM per block
    otherwise.  The gradients of the slices are gathered and flow back through ONE input-gradient and ONE weight-gradient GEMM
    per width."""
    groups = time_emb_groups(st.leaves)
    acts = iter(ops.fanout(temb_act, len(groups)))
    out = {}
    for width, names in groups.items():
        a = next(acts)
        y = ops.linear_multi(a, st, tuple(n + "/time_emb_proj" for n in names)) if len(names) > 1 else None
        if y is not None:
            for n, rb in zip(names, ops.col_slices(y, len(names))):
                out[n] = rb
        else:
            for n, alias in zip(names, ops.fanout(a, len(names))):
                out[n] = ops.linear(alias, st, n + "/time_emb_proj")
    return out


def _context_projections(st, ctx):
    """to_k / to_v of every cross-attention block applied to the text context (diffusers FlaxAttention: key = to_k(context),
    value = to_v(context)): one GEMM per channel width where those kernels are laid out back to back (unet_spec), the blocks
    reading their [k|v] as a column slice of its output; otherwise each block gets an alias of the context and projects it
    itself.  Returns {"<block>/attn2": _PackedKV or context alias}."""
    if getattr(st, "adapter", None) is not None and not ctx.requires_grad:
        # a frozen text encoder hands over a context without a tape: the to_k / to_v backward - the only producer of those adapters'
        # weight gradients - would never run.  Anchor it here, as unet_forward anchors x
        ctx = ctx.detach().requires_grad_(True)
    groups = {}
    for p in st.leaves:
        if p.endswith("/attn2/to_k/kernel"):
            groups.setdefault(st.leaves[p].shape[1], []).append(p[: -len("/to_k/kernel")])
    acts = iter(ops.fanout(ctx, len(groups)))
    out = {}
    for width, names in groups.items():
        a = next(acts)
        y = ops.linear_multi(a, st, tuple(n + t for n in names for t in ("/to_k", "/to_v"))) if len(names) > 1 else None
        if y is not None:
            for n, kv in zip(names, ops.col_slices(y, len(names))):
                out[n] = _PackedKV(kv)
        else:
            for n, alias in zip(names, ops.fanout(a, len(names))):
                out[n] = alias
    return out


def ip_adapter_tokens(st, cfg, image_embeds):
    """image_proj of an IP-Adapter store: image_embeds bf16 (B, E) -> Linear E -> T * Dc, viewed (B, T, Dc), LayerNorm over Dc: the image
    tokens (B, T, Dc) bf16 every cross-attention attends to."""
    _require(image_embeds.dim() == 2 and image_embeds.shape[1] == cfg["image_embed_dim"],
             f"ip_adapter_tokens: image_embeds {tuple(image_embeds.shape)} must be (B, {cfg['image_embed_dim']})")
    x = image_embeds.to(torch.bfloat16).contiguous()
    if st.trainable and torch.is_grad_enabled() and not x.requires_grad:
        x = x.detach().requires_grad_(True)  # anchors the tape: image_proj's weight gradients come from its backward
    y = ops.linear(x, st, "image_proj/proj")
    return ops.layer_norm(y.view(x.shape[0], cfg["num_tokens"], cfg["cross_attention_dim"]), st, "image_proj/norm")


def _require(cond, msg):
    if not cond:
        raise ValueError(msg)


class _ImageKV:
    """What a cross-attention block needs for its image term: the adapter's store, the block's [k|v] of the image tokens as a column
    slice of the width's grouped projection (kv) or an alias of the tokens to project itself (tokens), and the per-sample scale."""

    def __init__(self, ctx, store, kv, tokens, scale):
        self.ctx, self.store, self.kv, self.tokens, self.scale = ctx, store, kv, tokens, scale
        self.shape = ctx.shape


def _image_projections(st, tokens, ctx, scale):
    """to_k_ip / to_v_ip of every cross-attention applied to the image tokens, one GEMM per channel width (ip_adapter_spec lays the
    leaves out for it), and each entry of ctx (_context_projections) wrapped with its block's share."""
    groups = {}
    for p in st.leaves:
        if p.endswith("/attn2/to_k_ip/kernel"):
            groups.setdefault(st.leaves[p].shape[1], []).append(p[: -len("/to_k_ip/kernel")])
    _require(set(n for names in groups.values() for n in names) == set(ctx),
             "ip: the adapter's cross-attention blocks are not the UNet's (another config?)")
    acts = iter(ops.fanout(tokens, len(groups)))
    out = {}
    for width, names in groups.items():
        a = next(acts)
        y = ops.linear_multi(a, st, tuple(n + t for n in names for t in ("/to_k_ip", "/to_v_ip"))) if len(names) > 1 else None
        if y is not None:
            for n, kv in zip(names, ops.col_slices(y, len(names))):
                out[n] = _ImageKV(ctx[n], st, kv, None, scale)
        else:
            for n, alias in zip(names, ops.fanout(a, len(names))):
                out[n] = _ImageKV(ctx[n], st, None, alias, scale)
    return out


def _resnet(x, rb, st, name, groups, eps, xs=None):
    """rb: the block's time-embedding row bias (B, C_out) or None (VAE).  xs: GroupNorm statistics of x when its producer
    accumulated them (ops.conv2d / ops.linear gn_groups=).  Returns (output, statistics of the output for the next GroupNorm, or
    None)."""
    h, x = ops.group_norm(x, st, name + "/norm1", groups, eps, silu=True, skip=True, stats=xs)
    h, hs = ops.conv2d(h, st, name + "/conv1", rowbias=rb, gn_groups=groups)
    h = ops.group_norm(h, st, name + "/norm2", groups, eps, silu=True, stats=hs)
    sc = ops.conv2d(x, st, name + "/conv_shortcut", pad=0) if st.has(name + "/conv_shortcut/kernel") else x
    return ops.conv2d(h, st, name + "/conv2", residual=sc, gn_groups=groups)


_KEY_WEIGHTS = {}


def key_chunk_weights(n_query, num_kv, device):
    """How often diffusers' memory-efficient attention, as the reference patches it (key_chunk_patch.patch: key chunk = query
    count), counts each key: chunks start at 0, c, 2c, ... with c = min(n_query, num_kv), and jax.lax.dynamic_slice clamps the last
    start so that the slice fits - when c does not divide num_kv that chunk overlaps the one before it and the overlapped keys enter
    the softmax sum twice (512x512 mid block, 64 queries x 77 keys -> keys 13..63).  None when every key counts once."""
    key = (n_query, num_kv, str(device))
    if key not in _KEY_WEIGHTS:
        c = min(n_query, num_kv)
        w = torch.zeros(num_kv, dtype=torch.float32)
        for start in range(0, num_kv, c):
            s0 = min(start, num_kv - c)
            w[s0: s0 + c] += 1
        _KEY_WEIGHTS[key] = None if bool((w == 1).all()) else w.to(device)
    return _KEY_WEIGHTS[key]


class _PackedKV:
    """The [k|v] projections (B, Nk, 2C) of one cross-attention block, computed ahead of the blocks (_context_projections)."""

    def __init__(self, kv):
        self.kv = kv
        self.shape = kv.shape


def _packed_pair(x, st, kname, vname):
    """[k | v] = [x @ to_k | x @ to_v] as one packed tensor: one GEMM where the two kernels can share it (ops.linear_multi), otherwise
    two and a channel concatenation (widths that are no multiple of 64: the tiny test configs)."""
    kv = ops.linear_multi(x, st, (kname, vname))
    if kv is None:
        xk, xv = ops.fanout(x, 2)
        kv = ops.concat_channels(ops.linear(xk, st, kname), ops.linear(xv, st, vname))
    return kv


def _attn(x, ctx, st, name, heads, residual, chunked_keys=True):
    """ctx None: self-attention; otherwise one alias of the text context (ops.fanout) or the block's precomputed _PackedKV.
    The projections that share an input run as one GEMM (ops.linear_multi) and attention reads / differentiates the packed
    tensor in place."""
    c = x.shape[-1]
    scale = (c // heads) ** -0.5
    kw = key_chunk_weights(x.shape[1], ctx.shape[1], x.device) if (ctx is not None and chunked_keys) else None
    if isinstance(ctx, _ImageKV):  # decoupled cross-attention: the text term's launch, then the image term added into its output
        ip, ctx = ctx, ctx.ctx
        q = ops.linear(x, st, name + "/to_q")
        kv = ctx.kv if isinstance(ctx, _PackedKV) else _packed_pair(ctx, st, name + "/to_k", name + "/to_v")
        kv_ip = ip.kv if ip.kv is not None else _packed_pair(ip.tokens, ip.store, name + "/to_k_ip", name + "/to_v_ip")
        o = ops.attention_ip(q, kv, kv_ip, heads, scale, key_weight=kw, scale_ip=ip.scale)
        return ops.linear(o, st, name + "/to_out_0", residual=residual)
    if isinstance(ctx, _PackedKV):
        o = ops.attention_packed(ops.linear(x, st, name + "/to_q"), ctx.kv, heads, scale, key_weight=kw)
        return ops.linear(o, st, name + "/to_out_0", residual=residual)
    if ctx is None:
        qkv = ops.linear_multi(x, st, (name + "/to_q", name + "/to_k", name + "/to_v"))
        if qkv is not None:
            o = ops.attention_packed(qkv, None, heads, scale)
        else:
            xq, xk, xv = ops.fanout(x, 3)
            o = ops.attention(ops.linear(xq, st, name + "/to_q"), ops.linear(xk, st, name + "/to_k"),
                              ops.linear(xv, st, name + "/to_v"), heads, scale)
    else:
        q = ops.linear(x, st, name + "/to_q")
        kv = ops.linear_multi(ctx, st, (name + "/to_k", name + "/to_v"))
        if kv is not None:
            o = ops.attention_packed(q, kv, heads, scale, key_weight=kw)
        else:
            ck, cv = ops.fanout(ctx, 2)
            o = ops.attention(q, ops.linear(ck, st, name + "/to_k"), ops.linear(cv, st, name + "/to_v"), heads, scale, key_weight=kw)
    return ops.linear(o, st, name + "/to_out_0", residual=residual)


def _transformer(x, ctx, st, name, heads, depth, lin, groups, xs=None, chunked_keys=True):
    """ctx: {"<block>/attn2": alias of the text context or _PackedKV} (_context_projections).  xs / second result: see _resnet."""
    B, H, W, C = x.shape
    h, x = ops.group_norm(x, st, name + "/norm", groups, 1e-5, skip=True, stats=xs)
    if lin:
        h = ops.linear(h.view(B, H * W, C), st, name + "/proj_in")
    else:
        h = ops.conv2d(h, st, name + "/proj_in", pad=0).view(B, H * W, C)
    for k in range(depth):
        b = f"{name}/transformer_blocks_{k}"
        hn, h = ops.layer_norm(h, st, b + "/norm1", skip=True)
        h = _attn(hn, None, st, b + "/attn1", heads, h)
        hn, h = ops.layer_norm(h, st, b + "/norm2", skip=True)
        h = _attn(hn, ctx[b + "/attn2"], st, b + "/attn2", heads, h, chunked_keys)
        hn, h = ops.layer_norm(h, st, b + "/norm3", skip=True)
        h = ops.feed_forward_geglu(hn, st, b + "/ff/net_0/proj", b + "/ff/net_2", residual=h)
    if lin:
        y, ys = ops.linear(h, st, name + "/proj_out", residual=x.view(B, H * W, C), gn_groups=groups)
        return y.view(B, H, W, C), ys
    return ops.conv2d(h.view(B, H, W, C), st, name + "/proj_out", pad=0, residual=x, gn_groups=groups)


def _time_embedding(st, cfg, timesteps, added_cond):
    """The time embedding (plus add_embedding for a text_time config) of a UNet or ControlNet store: (B, 4 * block_out_channels[0])."""
    boc = cfg["block_out_channels"]
    te = timestep_embedding(timesteps, boc[0], cfg["flip_sin_to_cos"], cfg["freq_shift"]).requires_grad_(True)
    temb = ops.linear(ops.silu(ops.linear(te, st, "time_embedding/linear_1")), st, "time_embedding/linear_2")
    if cfg["addition_embed_type"] == "text_time":
        tid = added_cond["time_ids"]
        tide = timestep_embedding(tid.reshape(-1).to(torch.int32), cfg["addition_time_embed_dim"], True, 0.0).view(tid.shape[0], -1)
        a = ops.concat_channels(added_cond["text_embeds"].to(torch.bfloat16).contiguous(), tide).requires_grad_(True)
        temb = ops.add(temb, ops.linear(ops.silu(ops.linear(a, st, "add_embedding/linear_1")), st, "add_embedding/linear_2"))
    return temb


def _down_blocks(st, cfg, x, xs, rowbias, ctx, tap=False):
    """The down blocks from conv_in's output (x, xs) -> (x, xs, skips).  tap (ControlNet): every skip tensor has a second consumer, its
    zero convolution, so the list holds aliases (ops.fanout sums the two gradients in one launch)."""
    boc = cfg["block_out_channels"]
    nb, lpb, lin, g = len(boc), cfg["layers_per_block"], cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads = _per_block(cfg["attention_head_dim"], nb)  # Flax: attention_head_dim is the head COUNT
    depth = _per_block(cfg["transformer_layers_per_block"], nb)
    ck = cfg.get("emulate_key_chunks", True)  # False: exact softmax over the text keys (see key_chunk_weights)
    skips = []

    def keep(x):
        if tap:
            x, alias = ops.fanout(x, 2)
            skips.append(alias)
        else:
            skips.append(x)
        return x

    x = keep(x)
    for i, t in enumerate(cfg["down_block_types"]):
        for j in range(lpb):
            x, xs = _resnet(x, rowbias[f"down_blocks_{i}/resnets_{j}"], st, f"down_blocks_{i}/resnets_{j}", g, 1e-5, xs)
            if t == "CrossAttnDownBlock2D":
                x, xs = _transformer(x, ctx, st, f"down_blocks_{i}/attentions_{j}", heads[i], depth[i], lin, g, xs, ck)
            x = keep(x)
        if i != nb - 1:
            x, xs = ops.conv2d(x, st, f"down_blocks_{i}/downsamplers_0/conv", stride=2, pad=1, gn_groups=g)
            x = keep(x)
    return x, xs, skips


def _mid_block(st, cfg, x, xs, rowbias, ctx):
    boc = cfg["block_out_channels"]
    nb, lin, g = len(boc), cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads, depth = _per_block(cfg["attention_head_dim"], nb), _per_block(cfg["transformer_layers_per_block"], nb)
    x, xs = _resnet(x, rowbias["mid_block/resnets_0"], st, "mid_block/resnets_0", g, 1e-5, xs)
    x, xs = _transformer(x, ctx, st, "mid_block/attentions_0", heads[-1], depth[-1], lin, g, xs, cfg.get("emulate_key_chunks", True))
    return _resnet(x, rowbias["mid_block/resnets_1"], st, "mid_block/resnets_1", g, 1e-5, xs)


def controlnet_cond_embedding(st, cfg, cond):
    """The conditioning embedder (diffusers FlaxControlNetConditioningEmbedding): cond bf16 NHWC (B,H,W,pad8(conditioning_channels)) at
    pixel size -> (B,h,w,block_out_channels[0]) at latent size.  SiLU follows every convolution but conv_out."""
    e = "controlnet_cond_embedding"
    if st.trainable and torch.is_grad_enabled() and not cond.requires_grad:
        cond = cond.detach().requires_grad_(True)  # anchors the tape: the embedder's weight gradients come from its backward
    h = ops.silu(ops.conv2d(cond, st, e + "/conv_in"))
    for k in range(len(cfg["conditioning_embedding_out_channels"]) - 1):
        h = ops.silu(ops.conv2d(h, st, f"{e}/blocks_{2 * k}"))
        h = ops.silu(ops.conv2d(h, st, f"{e}/blocks_{2 * k + 1}", stride=2, pad=1))
    return ops.conv2d(h, st, e + "/conv_out")


def controlnet_forward_embedded(st, cfg, x, timesteps, ctx, embedding, added_cond=None):
    """controlnet_forward from an already computed controlnet_cond_embedding (the sampler embeds the hint once per generate call)."""
    g = cfg["norm_num_groups"]
    temb = _time_embedding(st, cfg, timesteps, added_cond)
    rowbias = _time_emb_projections(st, ops.silu(temb))
    if st.trainable and torch.is_grad_enabled() and not ctx.requires_grad:
        ctx = ctx.detach().requires_grad_(True)  # a frozen text encoder's context has no tape: anchor the to_k / to_v backward
    ctx = _context_projections(st, ctx)
    if not x.requires_grad:
        x = x.detach().requires_grad_(True)
    x, xs = ops.conv2d(x, st, "conv_in", residual=embedding, gn_groups=g)
    x, xs, skips = _down_blocks(st, cfg, x, xs, rowbias, ctx, tap=True)
    x, xs = _mid_block(st, cfg, x, xs, rowbias, ctx)
    down = [ops.conv2d(s, st, f"controlnet_down_blocks_{i}", pad=0) for i, s in enumerate(skips)]
    return down, ops.conv2d(x, st, "controlnet_mid_block", pad=0)


def controlnet_forward(st, cfg, x, timesteps, ctx, cond, added_cond=None):
    """diffusers FlaxControlNetModel.__call__ on a ControlNet store (controlnet_spec): x, timesteps, ctx, added_cond as unet_forward
    takes them, cond bf16 NHWC (B,H,W,pad8(conditioning_channels)) at pixel size (sdt_nchw_f32_to_nhwc_bf16 of the [0, 1] image).
    The embedded hint enters as conv_in's residual, the UNet's down and mid blocks run on this store, and a 1x1 convolution follows
    every skip tensor and the mid block.  Returns (down_residuals: list in the order unet_forward appends its skips, mid_residual)."""
    return controlnet_forward_embedded(st, cfg, x, timesteps, ctx, controlnet_cond_embedding(st, cfg, cond), added_cond)


def unet_forward(st, cfg, x, timesteps, ctx, added_cond=None, control=None, ip=None):
    """x: (B,h,w,pad8(in_channels)) bf16 NHWC; timesteps int32 (B,); ctx (B,L,cross_dim) bf16.
    Returns (B,h,w,pad8(out_channels)) bf16 NHWC (the reference returns NCHW; see train_step).
    control: None, or (down_residuals, mid_residual[, scale]) from controlnet_forward; scale f32 (B,) per-sample factors or None (1).
    Every decoder concatenation then reads skip + scale * residual and the mid block x + scale * mid_residual (ops.control_add).  On a
    store that is not trainable conv_in and the down blocks run without a tape: nothing upstream of the additions is trained.
    ip: None, or (adapter_store, image_tokens[, scale_ip]) with the tokens of ip_adapter_tokens and scale_ip f32 (B,) per-sample factors
    (sampling) or None (1): every attn2 then adds scale_ip * softmax(q K_ip^T) V_ip to its text attention (ops.attention_ip).  With
    ip=None nothing changes, neither launches nor bits."""
    boc = cfg["block_out_channels"]
    nb, lpb, lin, g = len(boc), cfg["layers_per_block"], cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads = _per_block(cfg["attention_head_dim"], nb)  # Flax: attention_head_dim is the head COUNT
    depth = _per_block(cfg["transformer_layers_per_block"], nb)
    ck = cfg.get("emulate_key_chunks", True)  # False: exact softmax over the text keys (see key_chunk_weights)
    temb = _time_embedding(st, cfg, timesteps, added_cond)
    # every resnet consumes silu(temb) and every cross-attention consumes ctx twice: hand out aliases whose gradients are
    # summed by one launch each instead of a chain of binary adds
    rowbias = _time_emb_projections(st, ops.silu(temb))  # {resnet path: (B, C_out) row bias of its first convolution}
    ctx = _context_projections(st, ctx)  # {attn2 path: the block's [k|v] projections}
    if ip is not None:
        ctx = _image_projections(ip[0], ip[1], ctx, ip[2] if len(ip) > 2 else None)
    down_r = mid_r = scale = None
    if control is not None:
        down_r, mid_r = list(control[0]), control[1]
        scale = control[2] if len(control) > 2 else None
    untaped = control is not None and not st.trainable
    if not untaped and not x.requires_grad:
        x = x.detach().requires_grad_(True)  # anchors the autograd tape (weights are not autograd leaves)
    # (x, xs): every block output travels with the GroupNorm statistics its producing GEMM accumulated (xs None after a concat)
    with torch.no_grad() if untaped else contextlib.nullcontext():
        x, xs = ops.conv2d(x, st, "conv_in", gn_groups=g)
        x, xs, skips = _down_blocks(st, cfg, x, xs, rowbias, ctx)
    if control is not None:
        if len(down_r) != len(skips):
            raise ValueError(f"control: {len(down_r)} down residuals for the UNet's {len(skips)} skip tensors")
        x, xs = ops.control_add(None, x, mid_r, scale), None  # the statistics described x before the addition
    x, xs = _mid_block(st, cfg, x, xs, rowbias, ctx)
    rheads, rdepth = list(reversed(heads)), list(reversed(depth))
    for i, t in enumerate(cfg["up_block_types"]):
        for j in range(lpb + 1):
            if control is not None:
                x = ops.control_add(x, skips.pop(), down_r.pop(), scale)
            else:
                x = ops.concat_channels(x, skips.pop())  # statistics of a concatenation: the standalone pass
            x, xs = _resnet(x, rowbias[f"up_blocks_{i}/resnets_{j}"], st, f"up_blocks_{i}/resnets_{j}", g, 1e-5, None)
            if t == "CrossAttnUpBlock2D":
                x, xs = _transformer(x, ctx, st, f"up_blocks_{i}/attentions_{j}", rheads[i], rdepth[i], lin, g, xs, ck)
        if i != nb - 1:
            x = ops.conv2d(ops.upsample2x(x), st, f"up_blocks_{i}/upsamplers_0/conv")
            xs = None
    assert not skips
    x = ops.group_norm(x, st, "conv_norm_out", g, 1e-5, silu=True, stats=xs)
    return ops.conv2d(x, st, "conv_out")


# ----------------------------------------------------------------------------- VAE encoder (frozen)
def _vae_attention(x, st, a, groups, xs=None):
    """Single-head attention with head dim C (= 512): scores materialised per image (3 % of the encoder's work)."""
    B, H, W, C = x.shape
    N = H * W
    s = torch.cuda.current_stream().cuda_stream
    h = ops.group_norm(x, st, a + "/group_norm", groups, 1e-6, stats=xs).view(B, N, C)
    q, k, v = (ops.linear(h, st, f"{a}/{n}") for n in ("query", "key", "value"))
    scores = torch.empty(N, N, dtype=torch.bfloat16, device=x.device)
    vt = torch.empty(C, N, dtype=torch.bfloat16, device=x.device)
    o = torch.empty(B, N, C, dtype=torch.bfloat16, device=x.device)
    for b in range(B):
        ops.gemm_nt(q[b], k[b], scores, N, N, C, 1, C, C, 0)
        _lib.call("sdt_softmax_rows_inplace", scores.data_ptr(), N, N, float(C) ** -0.5, s)  # q,k each * C^-1/4
        _lib.call("sdt_transpose_bf16", v[b].data_ptr(), vt.data_ptr(), 1, N, C, s)
        ops.gemm_nt(scores, vt, o[b], N, C, N, 1, N, N, 0)
    y, ys = ops.linear(o, st, a + "/proj_attn", residual=x.view(B, N, C), gn_groups=groups)
    return y.view(B, H, W, C), ys


@torch.no_grad()
def vae_encode_moments(st, cfg, pixels_nhwc):
    """pixels (B,H,W,8) bf16 (3 real channels) -> moments (B,H/8,W/8,2*latent) bf16 NHWC."""
    g, boc = cfg["norm_num_groups"], cfg["block_out_channels"]
    x, xs = ops.conv2d(pixels_nhwc, st, "encoder/conv_in", gn_groups=g)
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"]):
            x, xs = _resnet(x, None, st, f"encoder/down_blocks_{i}/resnets_{j}", g, 1e-6, xs)
        if i != len(boc) - 1:
            x, xs = ops.conv2d(x, st, f"encoder/down_blocks_{i}/downsamplers_0/conv", stride=2, pad=((0, 1), (0, 1)), gn_groups=g)
    x, xs = _resnet(x, None, st, "encoder/mid_block/resnets_0", g, 1e-6, xs)
    x, xs = _vae_attention(x, st, "encoder/mid_block/attentions_0", g, xs)
    x, xs = _resnet(x, None, st, "encoder/mid_block/resnets_1", g, 1e-6, xs)
    x = ops.group_norm(x, st, "encoder/conv_norm_out", g, 1e-6, silu=True, stats=xs)
    x = ops.conv2d(x, st, "encoder/conv_out")
    return ops.conv2d(x, st, "quant_conv", pad=0)


@torch.no_grad()
def vae_decode(st, cfg, latents_nhwc):
    """latents (B,h,w,pad8(latent)) bf16 (already divided by the scaling factor) -> image (B,8h,8w,pad8(3)) bf16 NHWC:
    diffusers 0.21.4 FlaxAutoencoderKL.decode as models/pipeline_flax_stable_diffusion.py:246-249 calls it."""
    g = cfg["norm_num_groups"]
    boc = tuple(cfg["block_out_channels"])[::-1]
    x = ops.conv2d(latents_nhwc, st, "post_quant_conv", pad=0)
    x, xs = ops.conv2d(x, st, "decoder/conv_in", gn_groups=g)
    x, xs = _resnet(x, None, st, "decoder/mid_block/resnets_0", g, 1e-6, xs)
    x, xs = _vae_attention(x, st, "decoder/mid_block/attentions_0", g, xs)
    x, xs = _resnet(x, None, st, "decoder/mid_block/resnets_1", g, 1e-6, xs)
    for i in range(len(boc)):
        for j in range(cfg["layers_per_block"] + 1):
            x, xs = _resnet(x, None, st, f"decoder/up_blocks_{i}/resnets_{j}", g, 1e-6, xs)
        if i != len(boc) - 1:
            x, xs = ops.conv2d(ops.upsample2x(x), st, f"decoder/up_blocks_{i}/upsamplers_0/conv", gn_groups=g)
    x = ops.group_norm(x, st, "decoder/conv_norm_out", g, 1e-6, silu=True, stats=xs)
    return ops.conv2d(x, st, "decoder/conv_out")


# ----------------------------------------------------------------------------- CLIP text encoder (trained)
def clip_text_forward(st, cfg, input_ids, anchor=None, prefix=""):
    """input_ids int32 (B*k, 77) -> last_hidden_state (B*k, 77, D) bf16 after final_layer_norm (causal mask).
    Two-tower configs (dual_clip_config): input_ids (B*k, 2, 77), one row of ids per tower -> (B*k, 77, D1 + D2)."""
    if "towers" in cfg:
        hs = [clip_text_forward(st, c, input_ids[:, i].contiguous(), anchor, cfg["prefixes"][i]) for i, c in enumerate(cfg["towers"])]
        return ops.concat_channels(hs[0], hs[1])
    x, _ = _clip_encoder(st, cfg, input_ids, anchor, prefix, cfg["num_hidden_layers"])
    return ops.layer_norm(x, st, prefix + "text_model/final_layer_norm", cfg["layer_norm_eps"])


def _clip_encoder(st, cfg, input_ids, anchor, prefix, n_layers, tap=None):
    """Embeddings and the first n_layers encoder layers.  tap = k: also returns an alias of the residual stream after k layers
    (hidden_states[k]; ops.fanout sums the two gradients), else None."""
    Bk, S = input_ids.shape
    d, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    if anchor is None:
        # (a frozen tower that carries a LoRA adapter still needs its backward: the adapted leaves' weight gradients come from it;
        # so does one that carries new tokens: their gradient is the embedding's)
        anchor = torch.zeros(1, device=input_ids.device, requires_grad=st.trainable or getattr(st, "adapter", None) is not None
                             or getattr(st, "tokens", None) is not None)
    x = ops.embedding(input_ids.contiguous(), st, prefix + "text_model/embeddings/token_embedding/embedding",
                      prefix + "text_model/embeddings/position_embedding/embedding", S, anchor)
    act = ops.quick_gelu if cfg["hidden_act"] == "quick_gelu" else ops.gelu_erf
    tapped = None
    for i in range(n_layers):
        if i == tap:
            x, tapped = ops.fanout(x, 2)
        L = f"{prefix}text_model/encoder/layers/{i}"
        h, x = ops.layer_norm(x, st, L + "/layer_norm1", eps, skip=True)
        qkv = ops.linear_multi(h, st, tuple(f"{L}/self_attn/{n}" for n in ("q_proj", "k_proj", "v_proj")))
        if qkv is not None:
            o = ops.attention_packed(qkv, None, heads, (d // heads) ** -0.5, causal=True)
        else:
            q, k, v = (ops.linear(hh, st, f"{L}/self_attn/{n}") for hh, n in zip(ops.fanout(h, 3), ("q_proj", "k_proj", "v_proj")))
            o = ops.attention(q, k, v, heads, (d // heads) ** -0.5, causal=True)
        x = ops.linear(o, st, L + "/self_attn/out_proj", residual=x)
        h, x = ops.layer_norm(x, st, L + "/layer_norm2", eps, skip=True)
        x = ops.linear(act(ops.linear(h, st, L + "/mlp/fc1")), st, L + "/mlp/fc2", residual=x)
    if tap == n_layers:
        tapped = x
    return x, tapped


def sdxl_text_forward(st, cfg, input_ids, windows=1, anchor=None):
    """SDXL's text conditioning (diffusers StableDiffusionXLPipeline.encode_prompt; the original SDXL trainer's embedders) on a
    dual_clip_config(sdxl_conditioning=True) store.  input_ids int32 (B*windows, 2, S), one row of ids per tower.
    Returns (context (B*windows, S, D1 + D2) bf16, pooled (B, projection_dim) bf16):
      * context: each tower's hidden_states[hidden_layer] (-2: the input of its last layer, no final LayerNorm), concatenated;
      * pooled: the second tower's text_projection(final_layer_norm(last layer output) at the EOS token) of the FIRST caption
        window of each sample (ops.clip_pool; eos_token_id == 2 selects the first largest id, as transformers does).
    The first tower stops at its context: its later layers and final LayerNorm are not run (unused_text_leaves)."""
    if not sdxl_conditioning(cfg):
        raise ValueError("sdxl_text_forward needs a two-tower config in SDXL mode (dual_clip_config(..., sdxl_conditioning=True))")
    if input_ids.dim() != 3 or input_ids.shape[1] != 2 or input_ids.shape[0] % windows:
        raise ValueError(f"input_ids must be (B*{windows}, 2, S), got {tuple(input_ids.shape)}")
    if hasattr(st, "mark_unused"):
        st.mark_unused(unused_text_leaves(cfg))
    ctxs, pooled = [], None
    for i, (t, pre) in enumerate(zip(cfg["towers"], cfg["prefixes"])):
        ids = input_ids[:, i].contiguous()
        k = _context_layers(t)
        if not t.get("with_projection"):
            x, _ = _clip_encoder(st, t, ids, anchor, pre, k)
            ctxs.append(x)
            continue
        x, c = _clip_encoder(st, t, ids, anchor, pre, t["num_hidden_layers"], tap=k)
        ctxs.append(c)
        eos = t.get("eos_token_id", 2)
        p, _ = ops.clip_pool(x, ids, st, pre + "text_model/final_layer_norm", -1 if eos == 2 else eos, t["layer_norm_eps"], windows)
        pooled = ops.linear(p, st, pre + "text_projection")
    if pooled is None:
        raise ValueError("SDXL mode: one tower must carry the text projection (with_projection)")
    return ops.concat_channels(ctxs[0], ctxs[1]), pooled
