"""sdt_control_concat_add on the MI355X: every output bit against numpy float64 plus one RNE rounding (tests/controlnet_reference.py),
in guarded buffers, on both the 16-byte and the element-wise path; the backward of ops.control_add against slices of dy."""
import numpy as np
import pytest
import torch

from tests import controlnet_reference as cr
from tests import kernel_checks as kc

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32

# (rows, rows_per_sample, Ca, Cb, with a, element offset of every base)
SHAPES = {
    "vec_6x8+8": (6, 3, 8, 8, True, 0),
    "vec_130x24+8": (130, 65, 24, 8, True, 0),
    "mid_4x0+40": (4, 4, 0, 40, False, 0),
    "scalar_10x4+12": (10, 5, 4, 12, True, 0),
    "offset_6x8+8": (6, 3, 8, 8, True, 1),
    "many_workgroups_300000x8+8": (300000, 150000, 8, 8, True, 0),
}
SCALES = {"null": None, "ones": [1.0, 1.0], "zero_and_negative": [0.0, -0.75], "large_and_small": [2.5, 1e-3]}

_SUB, _MAX = 2.0 ** -133, 3.3895313892515355e38  # the smallest bf16 subnormal, the largest finite bf16
# (skip, res): signed zeros, subnormals, sums that tie at the bf16 rounding boundary (at unit scale) or sit next to a tie, inf, overflow
SPECIAL = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (_SUB, 0.0), (_SUB, _SUB), (-_SUB, _SUB), (2.0 ** -126, -_SUB), (3 * _SUB, -0.0),
           (1.0, 2.0 ** -8), (1.0078125, 2.0 ** -8), (-1.0, -(2.0 ** -8)), (1.0, 2.0 ** -9), (1.0, 2.0 ** -8 * 1.0078125), (256.0, 1.0), (258.0, 1.0),
           (float("inf"), 1.0), (1.0, float("inf")), (float("inf"), float("-inf")), (float("-inf"), 0.0), (_MAX, _MAX), (_MAX, 2.0 ** 120),
           (-_MAX, -(2.0 ** 119)), (2.0 ** -126, -(2.0 ** -127))]


def _u16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def _operands(rows, Ca, Cb, seed):
    g = torch.Generator().manual_seed(seed)
    skip = torch.randn(rows, Cb, generator=g).to(BF)
    res = (torch.randn(rows, Cb, generator=g) * torch.exp2(torch.randint(-9, 2, (rows, Cb), generator=g).float())).to(BF)
    n = rows * Cb
    sp = torch.tensor(SPECIAL, dtype=F32).to(BF)
    assert torch.equal(sp.float(), torch.tensor(SPECIAL, dtype=F32)), "a special value is not a bf16 value"
    k = min(n, len(SPECIAL))
    pos = (torch.arange(k) * 5) % n if n > 5 * len(SPECIAL) else torch.arange(k)  # spread over rows and lanes where there is room
    skip.view(-1)[pos], res.view(-1)[pos] = sp[:k, 0], sp[:k, 1]
    # the left part is copied as 16-bit patterns, whatever they encode: random bits, NaN payloads included
    a = (torch.randint(0, 65536, (rows, Ca), generator=g, dtype=torch.int32) - 32768).to(torch.int16).view(BF) if Ca else None
    return a, skip, res


@pytest.mark.parametrize("scale_id", list(SCALES))
@pytest.mark.parametrize("shape_id", list(SHAPES))
def test_every_output_bit(dev, lib, shape_id, scale_id):
    from stable_diffusion_training_amd import _lib
    rows, rps, Ca, Cb, with_a, off = SHAPES[shape_id]
    a, skip, res = _operands(rows, Ca, Cb, seed=rows + 7 * Cb)
    scale = SCALES[scale_id]
    want = cr.control_add_bits(_u16(a) if with_a else None, _u16(skip), _u16(res), scale, rps)
    if scale_id == "zero_and_negative":
        assert int((want[:rps, Ca:] == 0x7FC0).sum()) >= 1, "0 * inf must be a NaN: no shortcut for a zero scale"

    def arena(t, n):  # one flat guarded row; the payload starts `off` elements in (off = 1: 2-byte aligned bases)
        data = None
        if t is not None:
            data = torch.zeros(n + off, dtype=BF)
            data[off:] = t.reshape(-1)
        return kc.Guarded(1, n + off, BF, dev, data=None if data is None else data.to(dev), pad=0)

    ga = arena(a, rows * Ca) if with_a else None
    gs, gr = arena(skip, rows * Cb), arena(res, rows * Cb)
    gw = arena(None, rows * (Ca + Cb))
    sc = None if scale is None else kc.Guarded(1, len(scale), F32, dev, data=torch.tensor(scale, dtype=F32).to(dev), pad=0)
    p = lambda g: None if g is None else g.ptr + 2 * off
    _lib.call("sdt_control_concat_add", p(ga), p(gs), p(gr), None if sc is None else sc.ptr, p(gw), rows, rps, Ca, Cb,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = gw.t[0]
    got = out[off:].reshape(rows, Ca + Cb)
    assert bool((_u16(out[:off]) == kc.SENTINEL[BF]).all()), "the elements in front of an offset base were written"
    kc.assert_equal_bits(got.cpu(), torch.from_numpy(want.view(np.int16).copy()).view(BF), f"{shape_id} {scale_id}")
    for g, name in ((ga, "a"), (gs, "skip"), (gr, "res"), (gw, "wide"), (sc, "scale")):
        if g is not None:
            g.check(f"{shape_id} {scale_id}: {name}")


@pytest.mark.parametrize("with_a", [True, False])
def test_op_forward_bits_and_backward_are_slices_of_dy(dev, with_a):
    from stable_diffusion_training_amd import ops
    B, H, W, Ca, Cb = 2, 3, 5, 24 if with_a else 0, 16
    a, skip, res = _operands(B * H * W, Ca, Cb, seed=3)
    want = cr.control_add_bits(_u16(a) if with_a else None, _u16(skip), _u16(res), None, H * W)
    shp = lambda t, C: None if t is None else t.to(dev).reshape(B, H, W, C).contiguous().requires_grad_(True)
    ad, sd, rd = shp(a, Ca), shp(skip, Cb), shp(res, Cb)
    y = ops.control_add(ad, sd, rd)
    assert tuple(y.shape) == (B, H, W, Ca + Cb) and y.dtype == BF
    assert np.array_equal(_u16(y).reshape(-1, Ca + Cb), want)
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(B, H, W, Ca + Cb, generator=g).to(BF).to(dev)
    y.backward(dy)
    torch.cuda.synchronize()
    right = dy[..., Ca:].contiguous()
    assert torch.equal(kc.bits(sd.grad), kc.bits(right)) and torch.equal(kc.bits(rd.grad), kc.bits(right))
    if with_a:
        assert torch.equal(kc.bits(ad.grad), kc.bits(dy[..., :Ca].contiguous()))
    # skip without a gradient (the frozen UNet's untaped encoder): only res (and a) receive one
    sd2, rd2 = sd.detach(), rd.detach().requires_grad_(True)
    ops.control_add(None if ad is None else ad.detach(), sd2, rd2).backward(dy)
    assert sd2.grad is None and torch.equal(kc.bits(rd2.grad), kc.bits(right))
    # a per-sample scale in the forward (sampling)
    sc = torch.tensor([0.5, -2.0], dtype=F32, device=dev)
    ys = ops.control_add(None if ad is None else ad.detach(), sd.detach(), rd.detach(), sc)
    assert np.array_equal(_u16(ys).reshape(-1, Ca + Cb), cr.control_add_bits(_u16(a) if with_a else None, _u16(skip), _u16(res), [0.5, -2.0], H * W))


def test_scale_with_a_res_that_requires_grad_is_refused(dev):
    from stable_diffusion_training_amd import ops
    skip = torch.zeros(2, 4, 4, 8, dtype=BF, device=dev)
    res = torch.zeros(2, 4, 4, 8, dtype=BF, device=dev, requires_grad=True)
    with pytest.raises(ValueError, match="sampling only"):
        ops.control_add(None, skip, res, torch.ones(2, device=dev))
    with pytest.raises(ValueError, match="sampling only"):
        ops.control_add(torch.zeros(2, 4, 4, 8, dtype=BF, device=dev), skip, res, torch.ones(2, device=dev))


def test_op_refuses_a_scale_on_another_device_and_empty_operands(dev):
    """Refused on the host: a host pointer must never reach the kernel, and an empty batch has no rows per sample."""
    from stable_diffusion_training_amd import _lib, ops
    skip, res = (torch.zeros(2, 4, 4, 8, dtype=BF, device=dev) for _ in range(2))
    for bad in (torch.ones(2), torch.ones(2, device=dev, dtype=torch.float64), torch.ones(3, device=dev), torch.ones(2, 2, device=dev)[:, 0]):
        with pytest.raises(_lib.SdtError, match="scale must be"):
            ops.control_add(None, skip, res, bad)
    empty = torch.zeros(0, 4, 4, 8, dtype=BF, device=dev)
    with pytest.raises(_lib.SdtError, match="non-empty"):
        ops.control_add(None, empty, empty)
    with pytest.raises(_lib.SdtError, match="non-empty"):
        ops.control_add(None, torch.zeros(2, 4, 4, 0, dtype=BF, device=dev), torch.zeros(2, 4, 4, 0, dtype=BF, device=dev))
