"""The teacher-forced parity rule, shared by the block tests (tests/test_gpu_blocks.py), the stage tests (tests/test_gpu_stages.py)
and their CPU proof (tests/test_stage_parity_cpu.py).  Importable without a GPU.

Gates.  One block deep the HIP path is a few bf16 roundings from the fp32 oracle: 6e-3 forward, 1.5e-2 backward (which adds the
rounding of dy through the same ops).  Where the block itself amplifies rounding noise (the first CLIP layer: a residual
stream of 0.02-sized embeddings under O(1) layer outputs) the yardstick is the reference's own precision: the distance of the
bf16-points oracle from the fp32 oracle.  The HIP path (fp32 inside fused kernels, fewer rounding points than the reference's
modules) has to be no further from fp32 than 1.25x that, and within the two distances' sum of the bf16-points oracle."""
import torch

from oracle import nets as onets
from tests.helpers import rel_l2

BF = torch.bfloat16
FWD_TOL, BWD_TOL = 6e-3, 1.5e-2


def bf(t):
    return t.to(BF).to(torch.float32)


def rand(shape, seed, scale=1.0):
    return bf(torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)


def gate(tol, floor):
    """The bound on the distance from the fp32 oracle: the fixed tolerance, or 1.25x the bf16-points oracle's own distance."""
    return max(tol, 1.25 * floor)


def oracle_run(fn, weights, inputs, dy):
    """fn(params, *inputs) -> output; returns (out, input grads, param grads) for the fp32 and the bf16-points oracle."""
    res = {}
    for mode in ("fp32", "bf16"):
        p = {k: v.clone().requires_grad_(True) for k, v in weights.items()}
        xs = [x.clone().requires_grad_(True) for x in inputs]
        with onets.bf16_points(mode == "bf16"):
            y = fn(p, *xs)
            gs = torch.autograd.grad(y, xs + list(p.values()), dy, allow_unused=True)
        res[mode] = (y.detach(), [g for g in gs[:len(xs)]], dict(zip(p.keys(), gs[len(xs):])))
    return res


def check_items(tag, items):
    """items: [(name, got, fp32 oracle, bf16-points oracle, tol)], the first one the forward output.  Asserts the rule on each and
    returns [worst forward vs fp32, its bf16-points floor, worst gradient vs fp32, its floor]."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, (name, got, r32, r16, tol) in enumerate(items):
        e32, e16, floor = rel_l2(got, r32), rel_l2(got, r16), rel_l2(r16, r32)
        assert e32 < gate(tol, floor), f"{tag}: {name} vs fp32 oracle {e32:.2e} (bf16-points oracle itself: {floor:.2e})"
        assert e16 < 1.1 * (gate(tol, floor) + floor), f"{tag}: {name} vs bf16-points oracle {e16:.2e}"
        j = 0 if (i == 0 or tol == FWD_TOL) else 2
        worst[j], worst[j + 1] = max(worst[j], e32), max(worst[j + 1], floor)
    return worst


def check(tag, y, dxs, st, ref):
    (y32, dx32, dp32), (y16, dx16, dp16) = ref["fp32"], ref["bf16"]
    g = st.export("grad")
    items = [("forward", y, y32, y16, FWD_TOL)]
    items += [(f"input gradient {i}", a, b, c, BWD_TOL) for i, (a, b, c) in enumerate(zip(dxs, dx32, dx16)) if a is not None and b is not None]
    gmax = max(float(b.norm()) for b in dp32.values() if b is not None)
    # (leaves whose gradient vanishes analytically - the key bias under a softmax - are rounding noise on every side: skipped)
    items += [(f"d {k}", g[k], b, dp16[k], BWD_TOL) for k, b in dp32.items() if b is not None and float(b.norm()) > 1e-4 * gmax]
    worst = check_items(tag, items)
    print(f"[{tag}] rel-L2 vs fp32 oracle: forward {worst[0]:.2e} (bf16-points oracle: {worst[1]:.2e}), worst gradient {worst[2]:.2e} "
          f"(bf16-points oracle: {worst[3]:.2e})")


# ----------------------------------------------------------------------------- block cases that can see a norm epsilon
# A GroupNorm divides by sqrt(var + eps): with unit-variance input, 1e-5 against 1e-6 moves the result by 4.5e-6, three orders of
# magnitude under the gate.  It shows where var is of the order of eps.  The table (oracle group_norm, 320 channels, 32 groups):
#     input std 0.01  -> 4.4e-2 between eps 1e-5 and 1e-6;  input std 0.003 -> 3.8e-1
# So the epsilon cases feed the block an input of std EPS_STD[eps] and shrink the weights in front of the inner norm (conv1 and the
# time-embedding projection for norm2; conv2 too where a following norm is under test) until that norm's input has the same std.
# A uniform input scale is not enough: a wrong epsilon would then be one common factor on every group, which the NEXT norm divides
# out again.  The input's groups therefore get stds spread over a factor of 4 around EPS_STD (group_spread), so the factor differs
# from group to group and survives the convolution that mixes them.
EPS_STD = {1e-5: 0.01, 1e-6: 0.003}
OTHER_EPS = {1e-5: 1e-6, 1e-6: 1e-5}


def group_spread(c, groups=32):
    """(c,) per-channel factors, constant inside a GroupNorm group, log-spaced from 0.5 to 2 over the groups (in a scrambled order)."""
    f = 2.0 ** torch.linspace(-1.0, 1.0, groups)
    f = f[torch.randperm(groups, generator=torch.Generator().manual_seed(groups))]
    return f.repeat_interleave(c // groups)


def eps_input(shape, seed, eps):
    """A block input whose GroupNorm groups have stds between 0.5x and 2x EPS_STD[eps]."""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * EPS_STD[eps]
    return bf(x * group_spread(shape[-1]))


def shrink(weights, prefixes, factor):
    """A copy of the weight tree with every leaf under one of the prefixes multiplied by factor."""
    return {k: (v * factor if k.startswith(tuple(prefixes)) else v.clone()) for k, v in weights.items()}


def vae_resblock_attention(x, w, resnet_block=None, attn_eps=1e-6):
    """Oracle of the VAE pieces the block test runs: ResBlock (eps 1e-6), then the single-head mid attention.  Returns (h, y)."""
    r, a = VAE_R, VAE_A
    hr = (resnet_block or onets.resnet_block)(x, None, w, r, 32, 1e-6)
    n, hh, ww, c = hr.shape
    g = onets.group_norm(hr, w, a + "/group_norm", 32, attn_eps).reshape(n, hh * ww, c)
    o = onets.attention_core(onets.dense(g, w, a + "/query"), onets.dense(g, w, a + "/key"), onets.dense(g, w, a + "/value"), 1, c ** -0.5)
    return hr, hr + onets.dense(o, w, a + "/proj_attn").reshape(n, hh, ww, c)


def resblock_eps_case(cin, cout, hw, temb_ch, eps, batch=2):
    """ResBlock "r" in which norm1 and norm2 both see their epsilon: the input's groups at 0.5x - 2x EPS_STD[eps], conv1 and the
    time-embedding projection shrunk until conv1's output plus the row bias has about that std too (it is ~0.6 with fan-in weights)."""
    shapes = {}
    onets._resnet_shapes(shapes, "r", cin, cout, temb_ch)
    w = shrink(onets.init_params(shapes, 5), ["r/conv1/", "r/time_emb_proj/"], EPS_STD[eps] / 0.6)
    return dict(w=w, x=eps_input((batch, hw, hw, cin), 1, eps), temb=rand((batch, temb_ch), 2) if temb_ch else None,
                dy=rand((batch, hw, hw, cout), 3, 0.1))


def transformer_eps_case(c, hw, ctx_len, ctx_dim, lin, batch=2):
    """Transformer2D "t" (depth 1) whose GroupNorm sees its epsilon (1e-5).  Its LayerNorms stay out of reach: they normalise the
    projected GroupNorm output plus O(1) attention outputs, whatever the block input's scale."""
    shapes = {}
    onets._transformer_shapes(shapes, "t", c, ctx_dim, 1, lin)
    return dict(w=onets.init_params(shapes, 6), x=eps_input((batch, hw, hw, c), 1, 1e-5), ctx=rand((batch, ctx_len, ctx_dim), 2),
                dy=rand((batch, hw, hw, c), 3, 0.1))


VAE_R, VAE_A = "encoder/mid_block/resnets_0", "encoder/mid_block/attentions_0"


def vae_block_shapes():
    shapes = {}
    onets._resnet_shapes(shapes, VAE_R, 512, 512, 0)
    onets._norm(shapes, VAE_A + "/group_norm", 512)
    for n in ("query", "key", "value", "proj_attn"):
        onets._dense(shapes, f"{VAE_A}/{n}", 512, 512)
    return shapes


def vae_eps_case(hw=16):
    """VAE ResBlock + mid attention in which norm1, norm2 and the attention's group_norm all see eps 1e-6: input groups at 0.5x - 2x
    0.003, conv1 shrunk for norm2, conv2 shrunk so that the ResBlock's output (input + conv2) stays at that scale for the attention."""
    w = shrink(shrink(onets.init_params(vae_block_shapes(), 8), [VAE_R + "/conv1/"], EPS_STD[1e-6] / 0.6), [VAE_R + "/conv2/"], 1 / 200)
    return dict(w=w, x=eps_input((1, hw, hw, 512), 1, 1e-6))
