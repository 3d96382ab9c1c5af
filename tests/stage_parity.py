"""Stage harness: teacher-forced parity for what lies BETWEEN the blocks of the UNet and the VAE.  Importable without a GPU.

nets.unet_forward / vae_encode_moments / vae_decode and their oracle twins reach their blocks through module globals (HIP:
_resnet, _transformer; oracle: resnet_block, transformer_2d).  patched() replaces those with shims, on both sides:

  * forward: a shim records what it was handed (input x, the time-embedding row bias, the [k|v] projections or context alias of
    each of its attn2 layers, the GroupNorm statistics xs, the scalar arguments) and returns an injected, seeded, bf16-representable
    output - the same tensor on both sides (the HIP shim with xs=None);
  * backward: the shim is an autograd.Function that records the dy it receives and returns injected seeded cotangents for x, the
    row bias and the [k|v] / context alias.  What is left running is the glue, a function of its parameters and the injected
    tensors; its VJP has to match for ANY cotangent, so true block gradients are not needed.

The oracle's resnet_block gets temb, not the row bias, so its shim computes dense(silu(temb), time_emb_proj) with the real oracle
ops and injects the row-bias cotangent there; likewise dense(ctx, to_k) / dense(ctx, to_v) for every attn2 whose projections the
HIP path groups into one GEMM (more than one cross-attention of that width; a lone one gets an alias of the context on both sides).
The oracle's VAE mid attention is inline code: in the VAE runs it stays real on both sides and only the ResBlocks are shimmed.

Injected scales: outputs std 1, cotangents std 0.1 (as in the block tests), except the tensor that feeds a conv_norm_out, which
gets parity_check.EPS_STD[eps of that norm] - the std at which the other epsilon misses the gate (tests/test_stage_parity_cpu.py)."""
import contextlib
import inspect
import zlib

import torch

from oracle import nets as onets
from tests.parity_check import BWD_TOL, EPS_STD, FWD_TOL, bf, gate
from tests.helpers import rel_l2

BATCH, TIMESTEPS = 3, (0, 37, 999)
LATENT, IMAGE = (8, 16), (32, 48)  # non-square: an H/W mix-up shows
TIME_IDS = ((512, 768, 0, 64, 448, 704), (1024, 640, 32, 8, 960, 576), (384, 896, 16, 48, 320, 832))

_TWO_LEVELS = dict(block_out_channels=(320, 640))
_SD15 = dict(_TWO_LEVELS, down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"))
CASES = {
    # default layers_per_block=2: the pop order crosses ResBlock, downsampler and conv_in skips; conv projections; one lone 640-wide
    # cross-attention (context alias) beside five grouped 320-wide ones
    "sd15": dict(kind="unet", base="sd15", over=_SD15, ctx=(77, 768)),
    "sdxl": dict(kind="unet", base="sdxl", ctx=(77, 2048),
                 over=dict(_TWO_LEVELS, down_block_types=("DownBlock2D", "CrossAttnDownBlock2D"),
                           up_block_types=("CrossAttnUpBlock2D", "UpBlock2D"), attention_head_dim=(5, 10),
                           transformer_layers_per_block=(1, 2), use_linear_projection=True, addition_embed_type="text_time",
                           cross_attention_dim=2048)),
    "inpaint": dict(kind="unet", base="sd15", over=dict(_SD15, in_channels=9), ctx=(77, 768)),
    "vae_encode": dict(kind="vae_encode"),
    "vae_decode": dict(kind="vae_decode"),
}
UNET_CASES = tuple(k for k, c in CASES.items() if c["kind"] == "unet")


def config(case, mod=onets):
    c = CASES[case]
    return mod.unet_config(c["base"], **c["over"]) if c["kind"] == "unet" else mod.vae_config("sd")


def last_block(case):
    """(name of the shimmed block whose output feeds conv_norm_out, that norm's epsilon)."""
    c = CASES[case]
    if c["kind"] == "vae_encode":
        return "encoder/mid_block/resnets_1", 1e-6
    if c["kind"] == "vae_decode":
        return "decoder/up_blocks_3/resnets_2", 1e-6
    cfg = config(case)
    i, j = len(cfg["block_out_channels"]) - 1, cfg["layers_per_block"]
    kind = "attentions" if cfg["up_block_types"][-1] == "CrossAttnUpBlock2D" else "resnets"
    return f"up_blocks_{i}/{kind}_{j}", 1e-5


def is_glue(path):
    """Leaves the glue reads itself; everything else sits inside a shimmed block and gets no gradient on either side."""
    return (path.split("/")[0] in ("conv_in", "time_embedding", "add_embedding", "conv_norm_out", "conv_out")
            or any(s in path for s in ("/time_emb_proj/", "/attn2/to_k/", "/attn2/to_v/", "/downsamplers_0/", "/upsamplers_0/")))


_WEIGHTS = {}


def weights(case):
    """Host fp32 weight tree of the case (cached; callers must not write into it)."""
    kind = CASES[case]["kind"]
    key = case if kind == "unet" else kind
    if key not in _WEIGHTS:
        cfg = config(case)
        shapes = {"unet": onets.unet_param_shapes, "vae_encode": onets.vae_encoder_param_shapes, "vae_decode": onets.vae_decoder_param_shapes}[kind](cfg)
        if kind == "unet":  # the leaves inside shimmed blocks are never read: no need to draw them
            w = onets.init_params({k: v for k, v in shapes.items() if is_glue(k)}, 11)
            w.update({k: torch.zeros(v) for k, v in shapes.items() if k not in w})
        else:
            w = onets.init_params(shapes, 12)
        _WEIGHTS[key] = w
    return _WEIGHTS[key]


def _seeded(tag, shape, std):
    return bf(torch.randn(tuple(shape), generator=torch.Generator().manual_seed(zlib.crc32(tag.encode()))) * std)


def inputs(case):
    """Canonical (oracle-layout, fp32, bf16-representable) inputs and output cotangent of a case."""
    c = CASES[case]
    if c["kind"] == "vae_encode":
        g = torch.Generator().manual_seed(5)
        return dict(pixels=bf(torch.rand(BATCH, 3, *IMAGE, generator=g) * 2 - 1))  # NCHW
    if c["kind"] == "vae_decode":
        return dict(latents=_seeded("latents", (BATCH, IMAGE[0] // 8, IMAGE[1] // 8, 4), 1.0))  # NHWC
    cfg = config(case)
    out = dict(sample=_seeded("sample", (BATCH, cfg["in_channels"], *LATENT), 1.0), ctx=_seeded("ctx", (BATCH, *c["ctx"]), 1.0),
               timesteps=torch.tensor(TIMESTEPS, dtype=torch.int32), dy=_seeded("dy", (BATCH, cfg["out_channels"], *LATENT), 0.1))
    if cfg["addition_embed_type"] == "text_time":
        out["added"] = dict(time_ids=torch.tensor(TIME_IDS, dtype=torch.int32), text_embeds=_seeded("text_embeds", (BATCH, 1280), 1.0))
    return out


class Tape:
    """What the shims of one run recorded, and the source of what they inject (a function of block name and shape only)."""

    def __init__(self, case, low_std=None):
        name, eps = last_block(case)
        self.std = {name: EPS_STD[eps] if low_std is None else low_std}
        self.fwd, self.bwd, self.args, self.xs, self.kinds = {}, {}, {}, {}, {}

    def output(self, name, shape, like):
        return _seeded("y|" + name, shape, self.std.get(name, 1.0)).to(device=like.device, dtype=like.dtype)

    def cot(self, name, what, like):
        return _seeded(f"d{what}|{name}", like.shape, 0.1).to(device=like.device, dtype=like.dtype)

    def take(self, key, t):
        self.fwd[key] = t.detach().float().cpu()


class _Inject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tape, name, y, cots, *ins):
        ctx.tape, ctx.name, ctx.cots = tape, name, cots
        return y.clone()

    @staticmethod
    def backward(ctx, dy):
        ctx.tape.bwd["dy@" + ctx.name] = dy.detach().float().cpu()
        return (None, None, None, None) + tuple(ctx.cots)


def _block(tape, name, x, cout, others, args):
    """Common body of the four shims.  others: [(record key or None, cotangent or the tag that seeds it, tensor or None)] after x."""
    tape.take("x@" + name, x)
    tape.args[name] = args
    ins, cots = [x], [tape.cot(name, "x", x)]
    for key, tag, t in others:
        if t is not None:
            if key is not None:
                tape.take(key, t)
            ins.append(t)
            cots.append(tag if torch.is_tensor(tag) else tape.cot(name, tag, t))
    y = tape.output(name, (*x.shape[:-1], cout), x)
    return _Inject.apply(tape, name, y, cots, *ins)


def _attn2_paths(name, depth):
    return [f"{name}/transformer_blocks_{k}/attn2" for k in range(depth)]


# ----------------------------------------------------------------------------- oracle side
def grouped_attn2(w):
    """attn2 paths whose to_k / to_v the HIP path runs as one GEMM per width: those of a width with more than one cross-attention
    (nets._context_projections, restated)."""
    by_width = {}
    for k, v in w.items():
        if k.endswith("/attn2/to_k/kernel"):
            by_width.setdefault(v.shape[1], []).append(k[: -len("/to_k/kernel")])
    return {p for ps in by_width.values() if len(ps) > 1 for p in ps}


def oracle_shims(tape, w, rowbias_silu=True):
    grouped = grouped_attn2(w)

    def resnet_block(x, temb, p, name, groups=32, eps=1e-5):
        rb = None
        if temb is not None:
            rb = onets.dense(onets.silu(temb) if rowbias_silu else temb, p, name + "/time_emb_proj")
        cout = p[name + "/conv1/kernel"].shape[-1]
        return _block(tape, name, x, cout, [("rowbias@" + name, "rb", rb)], dict(groups=int(groups), eps=float(eps)))

    def transformer_2d(x, ctx, p, name, heads, depth, linear_proj, groups=32, chunked_keys=True):
        others = []
        for b in _attn2_paths(name, depth):
            tape.kinds[b] = "packed" if b in grouped else "alias"
            if b in grouped:
                k, v = onets.dense(ctx, p, b + "/to_k"), onets.dense(ctx, p, b + "/to_v")
                kv = torch.cat([k, v], -1)
                tape.take("kv@" + b, kv)
                dk, dv = tape.cot(name, "kv|" + b, kv).chunk(2, dim=-1)  # the HIP side's [k|v] cotangent, as its two halves
                others += [(None, dk.contiguous(), k), (None, dv.contiguous(), v)]
            else:
                others.append(("kv@" + b, "ctx|" + b, ctx))
        args = dict(heads=int(heads), depth=int(depth), lin=bool(linear_proj), groups=int(groups), chunked_keys=bool(chunked_keys))
        return _block(tape, name, x, x.shape[-1], others, args)

    return dict(resnet_block=resnet_block, transformer_2d=transformer_2d)


@contextlib.contextmanager
def patched(mod, **globals_):
    old = {k: getattr(mod, k) for k in globals_}
    try:
        for k, v in globals_.items():
            setattr(mod, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


GLUE = {"unet": "unet_forward", "vae_encode": "vae_encode_moments", "vae_decode": "vae_decode"}


def planted(fn_name, edits):
    """A copy of the oracle's glue function fn_name with (old, new) source edits: the planted defect.  Called inside patched(), so
    the copy's globals hold the shims.  Every edit has to find its text: a defect that no longer applies fails loudly."""
    src = inspect.getsource(getattr(onets, fn_name))
    for old, new in edits:
        assert old in src, f"planted defect: {old!r} is not in oracle.nets.{fn_name} any more"
        src = src.replace(old, new)
    ns = dict(vars(onets))
    exec(compile(src, f"<oracle.nets.{fn_name} with a planted defect>", "exec"), ns)
    return ns[fn_name]


def run_oracle(case, mode="fp32", edits=(), rowbias_silu=True, low_std=None):
    """One oracle run of the case's glue around the shims.  mode: "fp32" or "bf16" (bf16_points).  edits: a planted defect.
    Returns dict(fwd={quantity: tensor}, bwd={...}, args={block: scalars}, kinds={attn2: "packed" | "alias"})."""
    kind = CASES[case]["kind"]
    cfg, w, inp, tape = config(case), weights(case), inputs(case), Tape(case, low_std)
    with patched(onets, **oracle_shims(tape, w, rowbias_silu)), onets.bf16_points(mode == "bf16"):
        fn = planted(GLUE[kind], edits) if edits else getattr(onets, GLUE[kind])
        if kind != "unet":
            with torch.no_grad():
                tape.take("output", fn(w, cfg, inp["pixels" if kind == "vae_encode" else "latents"]))
        else:
            leaves = [k for k in w if is_glue(k)]
            p = dict(w)
            p.update({k: w[k].clone().requires_grad_(True) for k in leaves})
            sample, ctx = inp["sample"].clone().requires_grad_(True), inp["ctx"].clone().requires_grad_(True)
            y = fn(p, cfg, sample, inp["timesteps"], ctx, inp.get("added"))
            tape.take("output", y)
            gs = torch.autograd.grad(y, [sample, ctx] + [p[k] for k in leaves], inp["dy"], allow_unused=True)
            for k, g in zip(["d sample", "d context"] + ["d " + k for k in leaves], gs):
                if g is not None:
                    tape.bwd[k] = g.detach()
    return dict(fwd=tape.fwd, bwd=tape.bwd, args=tape.args, kinds=tape.kinds)


# ----------------------------------------------------------------------------- HIP side
def hip_shims(tape, nets):
    def _resnet(x, rb, st, name, groups, eps, xs=None):
        if xs is not None:
            tape.xs[name] = xs.detach().double().cpu()
        cout = st.leaves[name + "/conv1/kernel"].shape[-1]
        return _block(tape, name, x, cout, [("rowbias@" + name, "rb", rb)], dict(groups=int(groups), eps=float(eps))), None

    def _transformer(x, ctx, st, name, heads, depth, lin, groups, xs=None, chunked_keys=True):
        if xs is not None:
            tape.xs[name] = xs.detach().double().cpu()
        others = []
        for b in _attn2_paths(name, depth):
            c = ctx[b]
            packed = isinstance(c, nets._PackedKV)
            tape.kinds[b] = "packed" if packed else "alias"
            others.append(("kv@" + b, ("kv|" if packed else "ctx|") + b, c.kv if packed else c))
        args = dict(heads=int(heads), depth=int(depth), lin=bool(lin), groups=int(groups), chunked_keys=bool(chunked_keys))
        return _block(tape, name, x, x.shape[-1], others, args), None

    return dict(_resnet=_resnet, _transformer=_transformer)


def _nhwc_pad8(t_nhwc, dev):
    """(B,H,W,C) fp32 -> bf16 on the device with the channels zero-padded to a multiple of 8 (the HIP activations' layout)."""
    c = t_nhwc.shape[-1]
    out = torch.zeros(*t_nhwc.shape[:-1], (c + 7) // 8 * 8, dtype=torch.bfloat16)
    out[..., :c] = t_nhwc
    return out.to(dev)


def run_hip(case, dev):
    """The same run on the HIP path.  Same result layout as run_oracle, plus xs={block: (B, nparts, G, 2) float64 partial rows}."""
    from stable_diffusion_training_amd import nets, params
    kind = CASES[case]["kind"]
    cfg, w, inp, tape = config(case, nets), weights(case), inputs(case), Tape(case)
    spec = {"unet": nets.unet_spec, "vae_encode": nets.vae_encoder_spec, "vae_decode": nets.vae_decoder_spec}[kind](cfg)
    st = params.ParamStore(spec, device=dev, quantise=False, trainable=kind == "unet")
    st.load(w)
    with patched(nets, **hip_shims(tape, nets)):
        if kind != "unet":
            x = inp["pixels"].permute(0, 2, 3, 1) if kind == "vae_encode" else inp["latents"]
            y = (nets.vae_encode_moments if kind == "vae_encode" else nets.vae_decode)(st, cfg, _nhwc_pad8(x, dev))
            tape.take("output", y[..., : 2 * cfg["latent_channels"] if kind == "vae_encode" else cfg["in_channels"]])
        else:
            cin, cout = cfg["in_channels"], cfg["out_channels"]
            sample = _nhwc_pad8(inp["sample"].permute(0, 2, 3, 1), dev).requires_grad_(True)
            ctx = inp["ctx"].to(dev).to(torch.bfloat16).requires_grad_(True)
            added = {k: v.to(dev) for k, v in inp["added"].items()} if "added" in inp else None
            y = nets.unet_forward(st, cfg, sample, inp["timesteps"].to(dev), ctx, added)
            tape.take("output", y[..., :cout].permute(0, 3, 1, 2))
            y.backward(_nhwc_pad8(inp["dy"].permute(0, 2, 3, 1), dev))
            tape.bwd["d sample"] = sample.grad[..., :cin].permute(0, 3, 1, 2).float().cpu()
            tape.bwd["d context"] = ctx.grad.float().cpu()
            tape.bwd.update({"d " + k: g.float().cpu() for k, g in st.export("grad").items() if is_glue(k)})
    return dict(fwd=tape.fwd, bwd=tape.bwd, args=tape.args, kinds=tape.kinds, xs=tape.xs)



# ----------------------------------------------------------------------------- comparison
def quantities(ref32):
    """[(quantity, "fwd" | "bwd", tol)] compared in a case, from the fp32 oracle's run: the forward output first."""
    q = [("output", "fwd", FWD_TOL)] + [(k, "fwd", FWD_TOL) for k in ref32["fwd"] if k != "output"]
    q += [(k, "bwd", BWD_TOL) for k in ref32["bwd"] if k.startswith("dy@") or k in ("d sample", "d context")]
    leaf = {k: v for k, v in ref32["bwd"].items() if not (k.startswith("dy@") or k in ("d sample", "d context"))}
    gmax = max((float(v.norm()) for v in leaf.values()), default=0.0)
    # (as in parity_check.check: a leaf whose gradient vanishes is rounding noise on every side)
    return q + [(k, "bwd", BWD_TOL) for k, v in leaf.items() if float(v.norm()) > 1e-4 * gmax]


def items(got, ref32, ref16):
    """The (name, got, fp32, bf16-points, tol) list parity_check.check_items takes.  A quantity the run under test lacks, or has in
    another shape, is an assertion error here: the glue handed a block something else."""
    out = []
    for k, side, tol in quantities(ref32):
        assert k in got[side], f"{k}: not produced"
        assert got[side][k].shape == ref32[side][k].shape, f"{k}: shape {tuple(got[side][k].shape)}, oracle {tuple(ref32[side][k].shape)}"
        out.append((k, got[side][k], ref32[side][k], ref16[side][k], tol))
    return out


def miss(got, ref32, ref16):
    """{quantity: distance from the fp32 oracle / gate} of a run; inf where the quantity is missing, has another shape, or (scalar
    arguments, [k|v] kind) differs.  > 1 misses the gate."""
    out = {}
    for k, side, tol in quantities(ref32):
        a, r32, r16 = got[side].get(k), ref32[side][k], ref16[side][k]
        out[k] = float("inf") if a is None or a.shape != r32.shape else rel_l2(a, r32) / gate(tol, rel_l2(r16, r32))
    for name, args in ref32["args"].items():
        out["args@" + name] = 0.0 if got["args"].get(name) == args else float("inf")
    for b, kind in ref32["kinds"].items():
        out["kind@" + b] = 0.0 if got["kinds"].get(b) == kind else float("inf")
    return out


def xs_errors(xs, x, groups=32):
    """Producer statistics against the tensor they travel with.  xs (B, nparts, G, 2) float64 partial rows {sum, sum of squares};
    x (B, ..., C) the bf16 tensor as float.  Returns (worst error / bound over sums and sums of squares, per image and group), the
    bound being the worst-case error of an fp32 summation in any order, n_terms * 2^-24 * sum |terms| (the squares of bf16 values
    are exact in fp32)."""
    B, C = x.shape[0], x.shape[-1]
    xg = x.double().reshape(B, -1, groups, C // groups)
    n = xg.shape[1] * xg.shape[3]
    got = xs.sum(dim=1)
    worst = 0.0
    for j, (val, mag) in enumerate(((xg.sum(dim=(1, 3)), xg.abs().sum(dim=(1, 3))), ((xg * xg).sum(dim=(1, 3)),) * 2)):
        bound = n * 2.0 ** -24 * mag
        worst = max(worst, float(((got[..., j] - val).abs() / bound.clamp_min(1e-300)).max()))
    return worst
