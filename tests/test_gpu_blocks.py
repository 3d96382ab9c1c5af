"""Teacher-forced block parity: every composite block of the three networks (ResBlock with time embedding, Transformer2D with
self / cross attention and GEGLU, CLIP encoder layer, VAE ResBlock and mid attention) runs ALONE on the HIP path at SD1.5
widths, on the SAME input the oracle gets, and is compared with the oracle block: forward output, input gradient and every
parameter gradient.

Why this granularity: through a whole network the bf16 path sits at its rounding-noise floor against ANY reference - any two
bf16 evaluations of the network that round at different points are ~1.4 - 2e-2 apart in the prediction (the HIP path against the
fp32 oracle, the reference's own bf16 module semantics against it; round 2's HIP step against itself while fp32 atomics still
reordered sums: tools/gn_stats_probe.py) - so an end-to-end rel-L2 gate of 2e-2 cannot tell a wrong epsilon or a missing
residual in one layer from rounding.  One block deep, the noise is a few bf16 roundings (<= 6e-3 forward) and a defect in how
the block composes its kernels (norm epsilon, GELU flavour, residual / shortcut wiring, time-embedding add, head split,
key-chunk weights) is far outside the gate.  Each case is checked against BOTH oracle precisions: the fp32 oracle and the
bf16-rounding-points oracle (oracle.nets.bf16_points: the reference's dtype=bfloat16 module semantics).

What unit-scale inputs can NOT see is a norm epsilon: 1e-5 against 1e-6 under a unit variance moves a GroupNorm's output by 4.5e-6,
three orders of magnitude inside the gate, and nets._resnet carries both values (1e-5 in the UNet, 1e-6 in the VAE).  The "eps" cases
close that for the GroupNorms: input groups at 0.5x - 2x the std at which the other epsilon shows (0.01 for 1e-5, 0.003 for 1e-6), and
the weights in front of the inner norms shrunk so that norm2 (and the VAE attention's group_norm) see that scale too
(tests/parity_check.py).  tests/test_stage_parity_cpu.py proves on the CPU, per norm, that the other epsilon misses these gates by more
than 2x.  The LayerNorms' epsilon stays invisible here (DESIGN.md §2 says why); no coverage is claimed for it."""
import pytest
import torch

from oracle import nets as onets
from tests import parity_check as pc
from tests.helpers import rel_l2
from tests.parity_check import BF, FWD_TOL, check as _check, oracle_run as _oracle_run, rand as _rand

pytestmark = pytest.mark.gpu


def _store(spec, weights, dev):
    from stable_diffusion_training_amd import params
    st = params.ParamStore(spec, device=dev, quantise=False, trainable=True)
    st.load(weights)
    return st


@pytest.mark.parametrize("cin,cout,hw,eps_case", [
    pytest.param(320, 320, 32, False, id="320-320-32"), pytest.param(640, 320, 32, False, id="640-320-32"),
    pytest.param(1280, 1280, 8, False, id="1280-1280-8"), pytest.param(320, 640, 16, True, id="320-640-16-eps")])
def test_resblock(dev, cin, cout, hw, eps_case):
    """eps: norm1 and norm2 both at the scale where eps 1e-6 in place of 1e-5 misses the gate (parity_check.resblock_eps_case)."""
    from stable_diffusion_training_amd import nets, ops
    B, temb_ch = 2, 1280
    spec = nets._Spec()
    spec.resnet("r", cin, cout, temb_ch)
    spec = spec.finish()
    if eps_case:
        c = pc.resblock_eps_case(cin, cout, hw, temb_ch, 1e-5, B)
        w, x, temb, dy = c["w"], c["x"], c["temb"], c["dy"]
    else:
        w = onets.init_params(dict(spec), 5)
        x, temb, dy = _rand((B, hw, hw, cin), 1), _rand((B, temb_ch), 2), _rand((B, hw, hw, cout), 3, 0.1)
    ref = _oracle_run(lambda p, x_, t_: onets.resnet_block(x_, t_, p, "r"), w, [x, temb], dy)
    st = _store(list(spec), w, dev)
    xd, td = x.to(dev).to(BF).requires_grad_(True), temb.to(dev).to(BF).requires_grad_(True)
    y, _ = nets._resnet(xd, nets._time_emb_projections(st, ops.silu(td))["r"], st, "r", 32, 1e-5)
    y.backward(dy.to(dev).to(BF))
    _check(f"resblock {cin}->{cout}@{hw}" + (" eps" if eps_case else ""), y, [xd.grad, td.grad], st, ref)


@pytest.mark.parametrize("c,heads,hw,ctx_len,lin,eps_case", [
    pytest.param(320, 8, 32, 77, False, False, id="320-8-32-77-False"), pytest.param(1280, 8, 8, 77, False, False, id="1280-8-8-77-False"),
    pytest.param(640, 10, 16, 231, True, False, id="640-10-16-231-True"), pytest.param(320, 8, 16, 77, False, True, id="320-8-16-77-False-eps")])
def test_transformer_block(dev, c, heads, hw, ctx_len, lin, eps_case):
    """incl. the 8x8 level, where 64 queries x 77 keys exercises the reference's clamped key chunk (keys 13..63 counted twice).
    eps: the block's GroupNorm at the scale where eps 1e-6 in place of 1e-5 misses the gate (parity_check.transformer_eps_case)."""
    from stable_diffusion_training_amd import nets, ops
    B, cd = 2, 768
    spec = nets._Spec()
    spec.transformer("t", c, cd, 1, lin)
    spec = spec.finish()
    w = onets.init_params(dict(spec), 6)
    x, ctx, dy = _rand((B, hw, hw, c), 1), _rand((B, ctx_len, cd), 2), _rand((B, hw, hw, c), 3, 0.1)
    if eps_case:
        ec = pc.transformer_eps_case(c, hw, ctx_len, cd, lin, B)
        w, x, ctx, dy = ec["w"], ec["x"], ec["ctx"], ec["dy"]
    ref = _oracle_run(lambda p, x_, c_: onets.transformer_2d(x_, c_, p, "t", heads, 1, lin), w, [x, ctx], dy)
    st = _store(list(spec), w, dev)
    xd, cd_ = x.to(dev).to(BF).requires_grad_(True), ctx.to(dev).to(BF).requires_grad_(True)
    y, _ = nets._transformer(xd, nets._context_projections(st, cd_), st, "t", heads, 1, lin, 32)
    y.backward(dy.to(dev).to(BF))
    _check(f"transformer c={c}@{hw}" + (" eps" if eps_case else ""), y, [xd.grad, cd_.grad], st, ref)


def test_clip_encoder_layer(dev):
    """One CLIP-L encoder layer between the embeddings and the final norm on 77-token rows (quick-GELU MLP, causal attention)."""
    from stable_diffusion_training_amd import nets
    cfg = dict(onets.clip_config("clip_l"), num_hidden_layers=1, vocab_size=1000)
    w = onets.init_params(onets.clip_param_shapes(cfg), 7)
    ids = torch.randint(0, 1000, (3, 77), generator=torch.Generator().manual_seed(1))
    dy = _rand((3, 77, 768), 3, 0.1)
    ref = _oracle_run(lambda p: onets.clip_text_forward(p, cfg, ids), w, [], dy)
    st = _store(nets.clip_text_spec(cfg), w, dev)
    y = nets.clip_text_forward(st, cfg, ids.to(dev).to(torch.int32))
    y.backward(dy.to(dev).to(BF))
    _check("clip layers", y, [], st, ref)


def test_vae_resblock_and_attention(dev):
    """VAE encoder pieces (GroupNorm eps 1e-6, no time embedding; single-head attention with C^-1/2 logits), forward only (frozen).
    Then the same pieces at the scale where eps 1e-5 in place of 1e-6 misses the gate, in norm1, norm2 and the attention's
    group_norm (parity_check.vae_eps_case), under the rule of parity_check.check_items."""
    from stable_diffusion_training_amd import nets, params
    spec = nets._Spec()
    spec.resnet(pc.VAE_R, 512, 512, 0)
    a = pc.VAE_A
    spec.norm(a + "/group_norm", 512)
    for n in ("query", "key", "value", "proj_attn"):
        spec.dense(f"{a}/{n}", 512, 512)
    ec = pc.vae_eps_case()
    for tag, w, x in (("unit", onets.init_params(dict(spec), 8), _rand((1, 32, 32, 512), 1)), ("eps", ec["w"], ec["x"])):
        st = params.ParamStore(list(spec), device=dev, trainable=False)
        st.load(w)
        with torch.no_grad():
            xd = x.to(dev).to(BF)
            h, hs = nets._resnet(xd, None, st, pc.VAE_R, 32, 1e-6)
            y, _ = nets._vae_attention(h, st, a, 32, hs)
            ref = {}
            for mode in (False, True):
                with onets.bf16_points(mode):
                    ref[mode] = pc.vae_resblock_attention(x, w)
                if tag == "unit":
                    hr, yr = ref[mode]
                    tol = 1e-2 if mode else FWD_TOL
                    assert rel_l2(h, hr) < tol and rel_l2(y, yr) < tol, (mode, rel_l2(h, hr), rel_l2(y, yr))
            if tag == "eps":
                worst = pc.check_items("vae resblock + attention eps", [("resblock output", h, ref[False][0], ref[True][0], FWD_TOL),
                                                                        ("attention output", y, ref[False][1], ref[True][1], FWD_TOL)])
                print(f"[vae resblock + attention eps] rel-L2 vs fp32 oracle: forward {worst[0]:.2e} (bf16-points oracle: {worst[1]:.2e})")
