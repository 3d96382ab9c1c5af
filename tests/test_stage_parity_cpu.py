"""CPU proof that the stage gates (tests/test_gpu_stages.py) and the epsilon cases of the block tests (tests/test_gpu_blocks.py)
discriminate.  The harness runs oracle against oracle, on the cases and injected data the GPU tests use:

  * the bf16-points oracle passes every comparison against the fp32 oracle - the reference alone stays inside the gate;
  * every planted defect, run in fp32, misses the gate by more than 2x on at least one compared quantity.  With that margin a HIP
    path that carries the defect and sits within one gate of ITS truth is still more than one gate from the fp32 oracle (triangle
    inequality), so the GPU test fails.  Each test prints the quantity that caught the defect and by how much.

A quantity that the defective run hands over in another shape, or scalar arguments that differ, count as caught outright (inf)."""
import math

import pytest
import torch

from oracle import nets as onets
from tests import parity_check as pc
from tests import stage_parity as sp
from tests.helpers import rel_l2
from tests.stage_defects import DEFECTS

MARGIN = 2.0
_REF = {}


def _ref(case):
    if case not in _REF:
        _REF[case] = (sp.run_oracle(case, "fp32"), sp.run_oracle(case, "bf16"))
    return _REF[case]


@pytest.mark.parametrize("case", list(sp.CASES))
def test_reference_stays_inside_the_gate(case):
    ref32, ref16 = _ref(case)
    worst = pc.check_items(f"stage {case}, bf16-points oracle", sp.items(ref16, ref32, ref16))
    assert ref16["args"] == ref32["args"] and ref16["kinds"] == ref32["kinds"]
    # what the case covers: both [k|v] flavours in the sd15-like cases, the skip of every kind, the low-std tensor in front of conv_norm_out
    name, eps = sp.last_block(case)
    assert name in ref32["args"], f"{name} is not the block in front of conv_norm_out"
    if sp.CASES[case]["kind"] == "unet":
        assert "packed" in ref32["kinds"].values()
        assert ("alias" in ref32["kinds"].values()) == (case != "sdxl")
    print(f"[stage {case}] bf16-points oracle vs fp32 oracle: forward {worst[1]:.2e}, worst gradient {worst[3]:.2e}; "
          f"{len(sp.quantities(ref32))} quantities, {len(ref32['args'])} shimmed blocks")


@pytest.mark.parametrize("defect,case", [(d, c) for d, spec in DEFECTS.items() for c in spec["cases"]])
def test_planted_defect_misses_the_gate(defect, case):
    spec = DEFECTS[defect]
    got = sp.run_oracle(case, "fp32", edits=spec.get("edits", ()), rowbias_silu=spec.get("rowbias_silu", True))
    miss = sp.miss(got, *_ref(case))
    finite = {k: v for k, v in miss.items() if math.isfinite(v)}
    outright = [k for k, v in miss.items() if not math.isfinite(v)]
    by = max(finite, key=finite.get)
    print(f"[defect] {defect} ({case}): caught by {by}, {finite[by]:.1f}x the gate" + (f"; outright by {outright[0]}" if outright else ""))
    assert finite[by] > MARGIN or outright, f"{defect} ({case}): worst miss {finite[by]:.2f}x the gate, on {by}"


# ----------------------------------------------------------------------------- the block tests' epsilon cases
def _block_miss(ref, got):
    """{item: distance from the fp32 oracle / gate} for a (y, dxs, param grads) run against parity_check.oracle_run's reference."""
    (y32, dx32, dp32), (y16, dx16, dp16) = ref["fp32"], ref["bf16"]
    gy, gdx, gdp = got
    out = {"forward": rel_l2(gy, y32) / pc.gate(pc.FWD_TOL, rel_l2(y16, y32))}
    for i, (a, b, c) in enumerate(zip(gdx, dx32, dx16)):
        if b is not None:
            out[f"input gradient {i}"] = rel_l2(a, b) / pc.gate(pc.BWD_TOL, rel_l2(c, b))
    gmax = max(float(b.norm()) for b in dp32.values() if b is not None)
    for k, b in dp32.items():
        if b is not None and float(b.norm()) > 1e-4 * gmax:
            out["d " + k] = rel_l2(gdp[k], b) / pc.gate(pc.BWD_TOL, rel_l2(dp16[k], b))
    return out


def _run32(fn, w, inputs, dy):
    p = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xs = [x.clone().requires_grad_(True) for x in inputs]
    y = fn(p, *xs)
    gs = torch.autograd.grad(y, xs + list(p.values()), dy, allow_unused=True)
    return y.detach(), list(gs[:len(xs)]), dict(zip(p.keys(), gs[len(xs):]))


def _caught(tag, miss):
    by = max(miss, key=miss.get)
    print(f"[eps] {tag}: caught by {by}, {miss[by]:.1f}x the gate")
    assert miss[by] > MARGIN, f"{tag}: worst miss {miss[by]:.2f}x the gate, on {by}"


@pytest.mark.parametrize("norm", ["norm1", "norm2"])
def test_resblock_eps_case_sees_the_unet_epsilon(norm):
    """test_resblock[320-640-16-eps]: eps 1e-6 in norm1 or norm2 of the UNet's ResBlock."""
    c = pc.resblock_eps_case(320, 640, 16, 1280, 1e-5)
    bad = sp.planted("resnet_block", [(f'name + "/{norm}", groups, eps)', f'name + "/{norm}", groups, 1e-6)')])
    ref = pc.oracle_run(lambda p, x_, t_: onets.resnet_block(x_, t_, p, "r"), c["w"], [c["x"], c["temb"]], c["dy"])
    _caught(f"resblock {norm} 1e-6 for 1e-5", _block_miss(ref, _run32(lambda p, x_, t_: bad(x_, t_, p, "r"), c["w"], [c["x"], c["temb"]], c["dy"])))


def test_transformer_eps_case_sees_the_group_norm_epsilon():
    """test_transformer_block[320-8-16-77-False-eps]: eps 1e-6 in the Transformer2D's GroupNorm."""
    c = pc.transformer_eps_case(320, 16, 77, 768, False)
    bad = sp.planted("transformer_2d", [('name + "/norm", groups, 1e-5)', 'name + "/norm", groups, 1e-6)')])
    ins = [c["x"], c["ctx"]]
    ref = pc.oracle_run(lambda p, x_, c_: onets.transformer_2d(x_, c_, p, "t", 8, 1, False), c["w"], ins, c["dy"])
    _caught("transformer norm 1e-6 for 1e-5", _block_miss(ref, _run32(lambda p, x_, c_: bad(x_, c_, p, "t", 8, 1, False), c["w"], ins, c["dy"])))


def test_transformer_layer_norm_epsilon_stays_invisible():
    """Not covered, and not claimed: scaling the block input does not reach the LayerNorms (the GroupNorm in front renormalises), so
    their epsilon moves nothing by even a hundredth of the gate.  If this ever fails the claim in DESIGN.md §2 is out of date."""
    c = pc.transformer_eps_case(320, 16, 77, 768, False)
    ins = [c["x"], c["ctx"]]
    ref = pc.oracle_run(lambda p, x_, c_: onets.transformer_2d(x_, c_, p, "t", 8, 1, False), c["w"], ins, c["dy"])
    for n in ("norm1", "norm2", "norm3"):
        bad = sp.planted("transformer_2d", [(f'b + "/{n}")', f'b + "/{n}", 1e-6)')])
        miss = _block_miss(ref, _run32(lambda p, x_, c_: bad(x_, c_, p, "t", 8, 1, False), c["w"], ins, c["dy"]))
        assert max(miss.values()) < 1e-2, (n, max(miss.values()))


@pytest.mark.parametrize("norm", ["norm1", "norm2", "group_norm"])
def test_vae_eps_case_sees_the_vae_epsilon(norm):
    """test_vae_resblock_and_attention, second case: eps 1e-5 in norm1 / norm2 of the VAE's ResBlock or in its attention's group_norm."""
    c = pc.vae_eps_case()
    with torch.no_grad():
        ref32 = pc.vae_resblock_attention(c["x"], c["w"])
        with onets.bf16_points():
            ref16 = pc.vae_resblock_attention(c["x"], c["w"])
        if norm == "group_norm":
            got = pc.vae_resblock_attention(c["x"], c["w"], attn_eps=1e-5)
        else:
            bad = sp.planted("resnet_block", [(f'name + "/{norm}", groups, eps)', f'name + "/{norm}", groups, 1e-5)')])
            got = pc.vae_resblock_attention(c["x"], c["w"], resnet_block=bad)
    miss = {n: rel_l2(g, a) / pc.gate(pc.FWD_TOL, rel_l2(b, a)) for n, g, a, b in zip(("resblock output", "attention output"), got, ref32, ref16)}
    _caught(f"vae {norm} 1e-5 for 1e-6", miss)


def test_xs_bound_tells_right_statistics_from_wrong():
    """stage_parity.xs_errors: exact statistics in any number of partial rows pass; those of another tensor, or a mean in place of a
    sum, do not."""
    x = pc.rand((2, 4, 6, 64), 3)
    xg = x.double().reshape(2, 24, 32, 2)
    right = torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], -1)
    parts = torch.stack([0.25 * right, 0.75 * right], 1)
    assert sp.xs_errors(parts, x) < 1e-6
    as_fp32 = torch.stack([xg.float().sum(dim=(1, 3)), (xg.float() ** 2).sum(dim=(1, 3))], -1).double()[:, None]
    assert sp.xs_errors(as_fp32, x) <= 1.0
    assert sp.xs_errors(parts.flip(0), x) > 1.0 and sp.xs_errors(parts / 48, x) > 1.0
