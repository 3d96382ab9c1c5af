"""Planted defects for tests/test_stage_parity_cpu.py: each is a set of source edits to a COPY of one of the oracle's glue functions
(stage_parity.planted), or a switch of the oracle-side shim, and names the cases it is run on."""
from tests.stage_parity import UNET_CASES

_UP = ('conv2d(upsample_nearest2x(x), p, f"up_blocks_{i}/upsamplers_0/conv")', 'upsample_nearest2x(conv2d(x, p, f"up_blocks_{i}/upsamplers_0/conv"))')
_VUP = ('conv2d(upsample_nearest2x(x), p, f"decoder/up_blocks_{i}/upsamplers_0/conv")',
        'upsample_nearest2x(conv2d(x, p, f"decoder/up_blocks_{i}/upsamplers_0/conv"))')
_VAE_PAD = "stride=2, pad=((0, 1), (0, 1)))"
_UNET_PAD = "stride=2, pad=1)"

# name -> dict(cases, edits=[(old, new)] | rowbias_silu=False)
DEFECTS = {
    "freq_shift 1": dict(cases=UNET_CASES, edits=[('cfg["flip_sin_to_cos"], cfg["freq_shift"])', 'cfg["flip_sin_to_cos"], 1)')]),
    "flip_sin_to_cos inverted": dict(cases=UNET_CASES, edits=[('boc[0], cfg["flip_sin_to_cos"]', 'boc[0], not cfg["flip_sin_to_cos"]')]),
    "no silu between the time_embedding linears": dict(
        cases=UNET_CASES, edits=[('dense(silu(dense(t_emb, p, "time_embedding/linear_1"))', 'dense((dense(t_emb, p, "time_embedding/linear_1"))')]),
    "no silu in front of time_emb_proj": dict(cases=UNET_CASES, rowbias_silu=False),
    "time_ids embedded in another order": dict(cases=("sdxl",), edits=[("timestep_embedding(tid.flatten()", "timestep_embedding(tid.flip(-1).flatten()")]),
    "text_embeds behind the time_ids embedding": dict(
        cases=("sdxl",), edits=[('torch.cat([added_cond["text_embeds"], te], -1)', 'torch.cat([te, added_cond["text_embeds"]], -1)')]),
    "no silu between the add_embedding linears": dict(
        cases=("sdxl",), edits=[('dense(silu(dense(a, p, "add_embedding/linear_1"))', 'dense((dense(a, p, "add_embedding/linear_1"))')]),
    "UNet downsampler with the VAE's pad": dict(cases=UNET_CASES, edits=[(_UNET_PAD, _VAE_PAD)]),
    "VAE downsampler with the UNet's pad": dict(cases=("vae_encode",), edits=[(_VAE_PAD, _UNET_PAD)]),
    "concat operands swapped": dict(cases=UNET_CASES, edits=[("torch.cat([x, skips.pop()], dim=-1)", "torch.cat([skips.pop(), x], dim=-1)")]),
    # (popping the whole list first-in-first-out hands the first up block a skip of another resolution and cannot run at all; inside
    # one up block the three skips share a resolution, and the last block's even a width)
    "skips popped first-in-first-out inside an up block": dict(cases=UNET_CASES, edits=[("skips.pop()", "skips.pop(-(lpb + 1 - j))")]),
    "UNet conv before the upsample": dict(cases=UNET_CASES, edits=[_UP]),
    "VAE conv before the upsample": dict(cases=("vae_decode",), edits=[_VUP]),
    "heads / depth not reversed on the up path": dict(
        cases=("sdxl",), edits=[("rheads, rdepth = list(reversed(heads)), list(reversed(depth))", "rheads, rdepth = list(heads), list(depth)")]),
    "UNet conv_norm_out eps 1e-6": dict(cases=UNET_CASES, edits=[('"conv_norm_out", g, 1e-5)', '"conv_norm_out", g, 1e-6)')]),
    "VAE encoder conv_norm_out eps 1e-5": dict(cases=("vae_encode",), edits=[('"encoder/conv_norm_out", g, 1e-6)', '"encoder/conv_norm_out", g, 1e-5)')]),
    "VAE decoder conv_norm_out eps 1e-5": dict(cases=("vae_decode",), edits=[('"decoder/conv_norm_out", g, 1e-6)', '"decoder/conv_norm_out", g, 1e-5)')]),
    "UNet silu after conv_norm_out dropped": dict(
        cases=UNET_CASES, edits=[('conv2d(silu(group_norm(x, p, "conv_norm_out", g, 1e-5)), p, "conv_out")', 'conv2d((group_norm(x, p, "conv_norm_out", g, 1e-5)), p, "conv_out")')]),
    "VAE encoder silu after conv_norm_out dropped": dict(
        cases=("vae_encode",), edits=[('conv2d(silu(group_norm(x, p, "encoder/conv_norm_out", g, 1e-6))', 'conv2d((group_norm(x, p, "encoder/conv_norm_out", g, 1e-6))')]),
    "VAE decoder silu after conv_norm_out dropped": dict(
        cases=("vae_decode",), edits=[('conv2d(silu(group_norm(x, p, "decoder/conv_norm_out", g, 1e-6))', 'conv2d((group_norm(x, p, "decoder/conv_norm_out", g, 1e-6))')]),
    "quant_conv skipped": dict(cases=("vae_encode",), edits=[('return conv2d(x, p, "quant_conv", pad=0)', "return x")]),
    "post_quant_conv skipped": dict(
        cases=("vae_decode",), edits=[('conv2d(conv2d(latents_nhwc, p, "post_quant_conv", pad=0), p, "decoder/conv_in")', 'conv2d(latents_nhwc, p, "decoder/conv_in")')]),
}
