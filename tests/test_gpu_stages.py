"""Teacher-forced stage parity: what lies BETWEEN the blocks of nets.unet_forward, nets.vae_encode_moments and nets.vae_decode.

The blocks are replaced by shims on both sides (tests/stage_parity.py): they record what the glue hands them and return injected
tensors, forward and backward.  What runs is the glue alone - the sinusoidal embedding and its MLP, SDXL's add_embedding, the silu
and grouped GEMM of the time-embedding projections, the grouped to_k|to_v GEMM, conv_in (4 and 9 channels), the stride-2
downsamplers with their two pad conventions, the skip stack and concat_channels, upsample2x + conv, the reversed heads / depth of
the up path, conv_norm_out + silu + conv_out, quant_conv / post_quant_conv, and the GroupNorm statistics the conv epilogues hand on.

Compared per case, each under the rule of parity_check.check_items (FWD_TOL / BWD_TOL or 1.25x the bf16-points oracle's own
distance from fp32, plus the companion bound against the bf16-points oracle): every shim's received x, row bias and [k|v]; the
network output; every shim's received dy; the gradients of the sample and the context; the gradient of every glue leaf.  The scalar
arguments (heads, depth, lin, groups, eps, chunked_keys) and the [k|v] flavour each shim received must be EQUAL on both sides, and
where a shim is handed statistics they must be those of the x it was handed.  tests/test_stage_parity_cpu.py proves that these
gates catch each of a list of planted glue defects with a 2x margin.  Batch 3, timesteps 0 / 37 / 999, non-square latents."""
import pytest

from tests import parity_check as pc
from tests import stage_parity as sp

pytestmark = pytest.mark.gpu
_REF = {}


def _ref(case):
    """The two oracle runs of a case, computed once."""
    if case not in _REF:
        _REF[case] = (sp.run_oracle(case, "fp32"), sp.run_oracle(case, "bf16"))
    return _REF[case]


def _compare(case, dev, expect_xs):
    ref32, ref16 = _ref(case)
    got = sp.run_hip(case, dev)
    assert got["args"] == ref32["args"], {k: (v, ref32["args"].get(k)) for k, v in got["args"].items() if v != ref32["args"].get(k)}
    assert got["kinds"] == ref32["kinds"], (got["kinds"], ref32["kinds"])
    # wiring of the statistics: a shim that is handed xs must be handed those of ITS x (the kernels' exactness is pinned elsewhere)
    assert set(expect_xs) <= set(got["xs"]), f"no statistics handed to {sorted(set(expect_xs) - set(got['xs']))}"
    worst_xs = 0.0
    for name, parts in got["xs"].items():
        err = sp.xs_errors(parts, got["fwd"]["x@" + name], got["args"][name]["groups"])
        assert err <= 1.0, f"{case}: statistics handed to {name} are {err:.2e}x the fp32 summation bound away from its input's"
        worst_xs = max(worst_xs, err)
    worst = pc.check_items(f"stage {case}", sp.items(got, ref32, ref16))
    print(f"[stage {case}] rel-L2 vs fp32 oracle: forward {worst[0]:.2e} (bf16-points oracle: {worst[1]:.2e}), worst gradient {worst[2]:.2e} "
          f"(bf16-points oracle: {worst[3]:.2e}); {len(got['xs'])} statistics, worst {worst_xs:.2e} of the summation bound")


@pytest.mark.parametrize("case", sp.UNET_CASES)
def test_unet_stages(dev, case):
    """Forward and backward.  conv_in hands its statistics to the ResBlock behind it (the downsampler's 4x8 output is too small for
    the epilogue to produce any: sdt_gemm_nt_gn_parts is 0 there)."""
    _compare(case, dev, ["down_blocks_0/resnets_0"])


def test_vae_encode_stages(dev):
    """Forward only (frozen).  The mid attention stays real on both sides; its output goes to mid_block/resnets_1.  Statistics: from
    conv_in and from the first ((0,1),(0,1))-padded downsampler (the smaller levels produce none at this image size)."""
    _compare("vae_encode", dev, ["encoder/down_blocks_0/resnets_0", "encoder/down_blocks_1/resnets_0"])


def test_vae_decode_stages(dev):
    """Forward only.  Statistics: from the last upsampler's conv (the 32x48 level; the smaller ones produce none)."""
    _compare("vae_decode", dev, ["decoder/up_blocks_3/resnets_0"])
