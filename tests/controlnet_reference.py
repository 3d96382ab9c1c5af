"""CPU restatement of a ControlNet (diffusers FlaxControlNetModel) and of a UNet that takes its residuals, built from the blocks of
oracle.nets (conv2d, resnet_block, transformer_2d, silu, ...).  Parameters are flat {"a/b/kernel": tensor} trees in Flax layouts,
activations NHWC; fp32 unless oracle.nets.bf16_points() is on."""
import torch

from oracle import nets as onets

EMB = "controlnet_cond_embedding"


def rne_bf16_bits(x64):
    """float64 array -> the uint16 bit patterns of its bfloat16 roundings, to nearest even, ONE rounding (a cast through float32
    would round twice).  The two bf16 neighbours of |x| are compared with it exactly in float64: their distances are exact
    differences.  NaN -> 0x7fc0; 2^128 and above, and what rounds up to it -> inf."""
    import numpy as np
    x = np.asarray(x64, np.float64)
    sign = np.where(np.signbit(x), 0x8000, 0).astype(np.uint32)
    a = np.abs(x)
    nan = np.isnan(x)
    a = np.where(nan, 0.0, a)
    fmax = float(np.finfo(np.float32).max)
    with np.errstate(over="ignore", invalid="ignore"):
        a32 = np.minimum(a, fmax).astype(np.float32)
    lo_bits = a32.view(np.uint32) >> 16
    val = lambda b: np.where(b >= 0x7F80, 2.0 ** 128, (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64))
    lo_bits = np.where(val(lo_bits) > a, lo_bits - 1, lo_bits)  # the float32 rounding crossed a bf16 value above |x|
    hi_bits = lo_bits + 1
    d_lo, d_hi = a - val(lo_bits), val(hi_bits) - a
    up = (d_hi < d_lo) | ((d_hi == d_lo) & ((lo_bits & 1) == 1))
    out = np.where(up, hi_bits, lo_bits)
    out = np.where(a >= 2.0 ** 128, 0x7F80, out)
    out = np.where(nan, 0x7FC0, out | sign)
    return out.astype(np.uint16)


def control_add_bits(a_bits, skip_bits, res_bits, scale, rows_per_sample):
    """The expected bits of sdt_control_concat_add: a_bits uint16 (rows, Ca) or None, skip_bits / res_bits uint16 (rows, Cb), scale
    float32 (rows / rows_per_sample,) or None -> uint16 (rows, Ca + Cb).  Column Ca + j is rne_bf16(float64(skip) + float64(scale) *
    float64(res))."""
    import numpy as np
    f64 = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    rows = skip_bits.shape[0]
    # (a scale vector may be longer than rows / rows_per_sample: the kernel reads the entries of the samples there are)
    s = np.ones(rows) if scale is None else np.repeat(np.asarray(scale, np.float32).astype(np.float64)[: rows // rows_per_sample], rows_per_sample)
    with np.errstate(invalid="ignore", over="ignore"):
        right = rne_bf16_bits(f64(skip_bits) + s[:, None] * f64(res_bits))
    return right if a_bits is None else np.concatenate([a_bits, right], axis=1)


def skip_channels(cfg):
    """Channel counts of the UNet's skip tensors in the order the forward appends them."""
    boc = cfg["block_out_channels"]
    out = [boc[0]]
    for i in range(len(boc)):
        out += [boc[i]] * cfg["layers_per_block"]
        if i != len(boc) - 1:
            out.append(boc[i])
    return out


def param_shapes(cfg):
    """{path: shape} of the ControlNet of `cfg` (a UNet config plus conditioning_embedding_out_channels / conditioning_channels)."""
    unet = onets.unet_param_shapes(cfg)
    keep = ("time_embedding/", "add_embedding/", "conv_in/", "down_blocks_", "mid_block/")
    s = {p: shp for p, shp in unet.items() if p.startswith(keep)}
    ch = tuple(cfg["conditioning_embedding_out_channels"])
    onets._conv(s, EMB + "/conv_in", cfg["conditioning_channels"], ch[0])
    for k in range(len(ch) - 1):
        onets._conv(s, f"{EMB}/blocks_{2 * k}", ch[k], ch[k])
        onets._conv(s, f"{EMB}/blocks_{2 * k + 1}", ch[k], ch[k + 1])
    onets._conv(s, EMB + "/conv_out", ch[-1], cfg["block_out_channels"][0])
    for i, c in enumerate(skip_channels(cfg)):
        onets._conv(s, f"controlnet_down_blocks_{i}", c, c, k=1)
    mid = cfg["block_out_channels"][-1]
    onets._conv(s, "controlnet_mid_block", mid, mid, k=1)
    return s


def zero_conv_paths(cfg):
    heads = ["controlnet_mid_block"] + [f"controlnet_down_blocks_{i}" for i in range(len(skip_channels(cfg)))]
    return [f"{h}/{leaf}" for h in heads for leaf in ("kernel", "bias")]


def random_controlnet(unet_params, cfg, seed=0, zero_std=0.05):
    """The shared leaves copied from the UNet and perturbed (so that the two networks differ), the embedder random, and the zero
    convolutions (and the embedder's conv_out) normal with std zero_std - every gradient is then nonzero.  zero_std=0: zeros."""
    g = torch.Generator().manual_seed(seed)
    shapes = param_shapes(cfg)
    fresh = onets.init_params({p: s for p, s in shapes.items() if p.startswith("controlnet_")}, seed + 1)
    out = {}
    for p in sorted(shapes):
        if p in unet_params:
            out[p] = unet_params[p] + 0.02 * unet_params[p].abs().mean() * torch.randn(shapes[p], generator=g)
        elif p.startswith(EMB) and not p.startswith(EMB + "/conv_out"):
            out[p] = fresh[p]
        else:
            out[p] = zero_std * torch.randn(shapes[p], generator=g)
    return out


def cond_embedding(p, cfg, cond_nhwc):
    h = onets.silu(onets.conv2d(cond_nhwc, p, EMB + "/conv_in"))
    for k in range(len(cfg["conditioning_embedding_out_channels"]) - 1):
        h = onets.silu(onets.conv2d(h, p, f"{EMB}/blocks_{2 * k}"))
        h = onets.silu(onets.conv2d(h, p, f"{EMB}/blocks_{2 * k + 1}", stride=2, pad=1))
    return onets.conv2d(h, p, EMB + "/conv_out")


def _time_embedding(p, cfg, timesteps, added_cond):
    boc = cfg["block_out_channels"]
    t = onets.timestep_embedding(timesteps, boc[0], cfg["flip_sin_to_cos"], cfg["freq_shift"])
    t = onets.dense(onets.silu(onets.dense(t, p, "time_embedding/linear_1")), p, "time_embedding/linear_2")
    if cfg["addition_embed_type"] == "text_time":
        tid = added_cond["time_ids"]
        te = onets.timestep_embedding(tid.flatten(), cfg["addition_time_embed_dim"], True, 0).reshape(tid.shape[0], -1)
        a = torch.cat([added_cond["text_embeds"], te], -1)
        t = onets._r(t + onets.dense(onets.silu(onets.dense(a, p, "add_embedding/linear_1")), p, "add_embedding/linear_2"))
    return t


def _encoder(p, cfg, x, t_emb, ctx):
    """conv_in's output -> (mid-block output, skips)."""
    boc = cfg["block_out_channels"]
    nb, lpb, lin, g = len(boc), cfg["layers_per_block"], cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads = onets._per_block(cfg["attention_head_dim"], nb)
    depth = onets._per_block(cfg["transformer_layers_per_block"], nb)
    ck = cfg.get("emulate_key_chunks", True)
    skips = [x]
    for i, t in enumerate(cfg["down_block_types"]):
        for j in range(lpb):
            x = onets.resnet_block(x, t_emb, p, f"down_blocks_{i}/resnets_{j}", g)
            if t == "CrossAttnDownBlock2D":
                x = onets.transformer_2d(x, ctx, p, f"down_blocks_{i}/attentions_{j}", heads[i], depth[i], lin, g, ck)
            skips.append(x)
        if i != nb - 1:
            x = onets.conv2d(x, p, f"down_blocks_{i}/downsamplers_0/conv", stride=2, pad=1)
            skips.append(x)
    return x, skips


def _mid(p, cfg, x, t_emb, ctx):
    boc = cfg["block_out_channels"]
    nb, lin, g = len(boc), cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads = onets._per_block(cfg["attention_head_dim"], nb)
    depth = onets._per_block(cfg["transformer_layers_per_block"], nb)
    x = onets.resnet_block(x, t_emb, p, "mid_block/resnets_0", g)
    x = onets.transformer_2d(x, ctx, p, "mid_block/attentions_0", heads[-1], depth[-1], lin, g, cfg.get("emulate_key_chunks", True))
    return onets.resnet_block(x, t_emb, p, "mid_block/resnets_1", g)


def controlnet_forward(p, cfg, sample_nchw, timesteps, ctx, cond_nchw, added_cond=None):
    """-> (down residuals NHWC, in skip order; mid residual NHWC).  cond_nchw: (B, conditioning_channels, H, W) at pixel size."""
    t_emb = _time_embedding(p, cfg, timesteps, added_cond)
    emb = cond_embedding(p, cfg, cond_nchw.permute(0, 2, 3, 1))
    x = onets._r(onets.conv2d(sample_nchw.permute(0, 2, 3, 1), p, "conv_in") + emb)
    x, skips = _encoder(p, cfg, x, t_emb, ctx)
    x = _mid(p, cfg, x, t_emb, ctx)
    down = [onets.conv2d(s, p, f"controlnet_down_blocks_{i}", pad=0) for i, s in enumerate(skips)]
    return down, onets.conv2d(x, p, "controlnet_mid_block", pad=0)


def unet_forward(p, cfg, sample_nchw, timesteps, ctx, added_cond=None, down=None, mid=None, scale=None):
    """oracle.nets.unet_forward with residuals: every skip becomes skip + s * r before its concatenation, the down blocks' output
    x + s * r_mid before the mid block.  scale: None (1) or a (B,) tensor.  Returns the NCHW sample."""
    boc = cfg["block_out_channels"]
    nb, lpb, lin, g = len(boc), cfg["layers_per_block"], cfg["use_linear_projection"], cfg["norm_num_groups"]
    heads = onets._per_block(cfg["attention_head_dim"], nb)
    depth = onets._per_block(cfg["transformer_layers_per_block"], nb)
    ck = cfg.get("emulate_key_chunks", True)
    s = 1.0 if scale is None else scale.to(torch.float32)[:, None, None, None]
    t_emb = _time_embedding(p, cfg, timesteps, added_cond)
    x = onets.conv2d(sample_nchw.permute(0, 2, 3, 1), p, "conv_in")
    x, skips = _encoder(p, cfg, x, t_emb, ctx)
    if down is not None:
        assert len(down) == len(skips)
        skips = [onets._r(k + s * r) for k, r in zip(skips, down)]
        x = onets._r(x + s * mid)
    x = _mid(p, cfg, x, t_emb, ctx)
    rheads, rdepth = list(reversed(heads)), list(reversed(depth))
    for i, t in enumerate(cfg["up_block_types"]):
        for j in range(lpb + 1):
            x = torch.cat([x, skips.pop()], dim=-1)
            x = onets.resnet_block(x, t_emb, p, f"up_blocks_{i}/resnets_{j}", g)
            if t == "CrossAttnUpBlock2D":
                x = onets.transformer_2d(x, ctx, p, f"up_blocks_{i}/attentions_{j}", rheads[i], rdepth[i], lin, g, ck)
        if i != nb - 1:
            x = onets.conv2d(onets.upsample_nearest2x(x), p, f"up_blocks_{i}/upsamplers_0/conv")
    x = onets.silu(onets.group_norm(x, p, "conv_norm_out", g, 1e-5))
    return onets.conv2d(x, p, "conv_out").permute(0, 3, 1, 2)
