"""sdt_loss_mask_prepare and sdt_masked_mse_loss_fwd_bwd on a real MI355X, bit for bit on exact-answer inputs (reference, case tables
and operands: tests/masked_loss_reference.py; the proof that they are exact in fp32: tests/test_masked_loss_cpu.py).

Masks hold values in {0, 0.25, 0.5, 1} (and, once per case, a negative value, a value above 1 and a NaN), pred and target integers in
-1..1, weights in {0.5, 1, 2}, per-sample mask sums whose h*w / S_b is a power of two where normalisation is on: every partial and
total is exact in fp32, so the results must equal the float64 reference in every bit whatever the partition or the workgroup that
arrives last.  Outputs sit between sentinel guards, inputs between NaN guards, pred's padding channels hold NaN; every case runs three
times over a poisoned scratch area and must leave its arrival counters at zero."""
import math

import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import masked_loss_reference as mr
from tests.kernel_checks import BF, Guarded, assert_equal_bits
from tests.test_gpu_kernel_exact import _poison_slabs, _stream, _workspace

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _flat_in(data, dev):
    return Guarded(1, data.numel(), F32, dev, data=data.reshape(1, -1), pad=0, back_rows=0)


def _flat_out(n, dev):
    return Guarded(1, n, F32, dev, pad=0, back_rows=0)


def _flat_io(data, dev):
    g = _flat_out(data.numel(), dev)
    g.t.copy_(data.reshape(1, -1))
    return g


def _ptr(g):
    return None if g is None else g.ptr


def _counters_zero(ws):
    msg = kc.counters_report(ws)
    assert msg is None, msg


# ================================================================================================ sdt_loss_mask_prepare
@pytest.mark.parametrize("case", mr.PREPARE_CASES, ids=[c[0] for c in mr.PREPARE_CASES])
def test_loss_mask_prepare_exact(dev, case):
    """e, mp and S equal the reference in every bit for floors 0, 0.25 and 1, with and without the pooled output, from a 16-byte
    aligned mask (16-byte loads from f = 4 on) and from one that starts 4 bytes behind a boundary (scalar loads): the same bits."""
    from stable_diffusion_training_amd import _lib
    name, f, B, H, W = case
    h, w = H // f, W // f
    ws = _workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    mask = mr.seeded_mask((B, H, W), 40 + f, special=True)
    assert torch.isnan(mask).sum() == 1 and (mask < 0).sum() == 1 and (mask > 1).sum() == 1
    mp = mr.pooled_mask(mask.numpy(), f, np.float32)
    aligned = _flat_in(mask, dev)
    shifted = _flat_in(torch.cat([torch.full((1,), float("nan")), mask.reshape(-1)]), dev)  # the mask starts 4 bytes in
    run = 0
    for floor in mr.FLOORS:
        e = mr.effective_mask(mp, floor)
        S = e.astype(np.float64).reshape(B, -1).sum(1)
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        for ptr, with_mp, where in ((aligned.ptr, True, "aligned"), (shifted.ptr + 4, True, "shifted"), (aligned.ptr, False, "aligned, no pooled output")):
            what = f"{name} floor {floor} {where}"
            if run:
                _poison_slabs(ws)
            run += 1
            E, MP, SS = _flat_out(B * h * w, dev), (_flat_out(B * h * w, dev) if with_mp else None), _flat_out(B, dev)
            _lib.call("sdt_loss_mask_prepare", ptr, E.ptr, _ptr(MP), SS.ptr, B, h, w, f, floor, ws.data_ptr(), ws.numel(), _stream())
            torch.cuda.synchronize()
            assert_equal_bits(E.t.cpu().view(B, h, w), torch.from_numpy(e), f"{what}: effective mask [image][row][column]")
            if MP is not None:
                assert_equal_bits(MP.t.cpu().view(B, h, w), torch.from_numpy(mp), f"{what}: pooled mask [image][row][column]")
                MP.check(f"{what}: pooled")
            assert_equal_bits(SS.t.cpu().view(B), torch.from_numpy(S.astype(np.float32)), f"{what}: sums")
            E.check(f"{what}: effective"); SS.check(f"{what}: sums")
            _counters_zero(ws)
    assert run == 9
    aligned.check("mask"); shifted.check("shifted mask")


# ================================================================================================ sdt_masked_mse_loss_fwd_bwd
@pytest.mark.parametrize("case", mr.LOSS_CASES, ids=[c[0] for c in mr.LOSS_CASES])
def test_masked_mse_loss_and_gradient_exact(dev, case):
    """Every variant of mr.LOSS_VARIANTS (with and without dpred, a mask, either weight vector, normalisation, a sample whose mask sum is
    0).  Power-of-two counts: loss_accum (3.0 before), loss_per_sample and every dpred element are exact.  Other counts (C = 3, 9):
    every sum is still exact, inv_count = fl32(1 / count) and fl32(1 / (C h w)) are not, so dpred is the documented chain
    bf16(fl(fl(fl(-2 fl(k e)) diff) inv_count)) - no addition in it - and loss_accum (0.0 before) and loss_per_sample must lie within 2
    fp32 ulps of the float64 value: one rounding of the reciprocal (<= 1/2 ulp, relative), one of the product (<= 1/2 ulp), and the slack
    between an ulp of the factors and an ulp of the result (< 2x on the first).  A sample with S_b = 0: zero loss, zero gradient, finite.
    Without a mask or with an all-ones mask, and unit loss weights, dpred equals sdt_mse_loss_fwd_bwd's on the same buffers bit for
    bit.  Three runs, identical bits."""
    from stable_diffusion_training_amd import _lib
    name, B, C, h, w, cpad = case
    ws = _workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    count = B * C * h * w
    pow2 = count & (count - 1) == 0
    l0 = mr.LOSS_ACCUM_BEFORE if pow2 else 0.0
    P = T = None
    first = True
    for variant in mr.LOSS_VARIANTS:
        vname, mask_kind, _, _, normalize, zero, has_dp = variant
        what = f"{name} {vname}"
        x = mr.loss_inputs(case, variant)
        if P is None:  # pred and target are the same for every variant of a case
            pred = torch.full((B, h, w, cpad), float("nan"))  # the padding channels of pred never enter the arithmetic
            pred[..., :C] = torch.from_numpy(x["pred"])
            P, T = Guarded(B * h * w, cpad, BF, dev, data=pred, pad=0), _flat_in(torch.from_numpy(x["target"]), dev)
        E = None if x["e"] is None else _flat_in(torch.from_numpy(x["e"]), dev)
        ref = mr.reference(x["pred"], x["target"], x["e"], x["snr"], x["lw"], normalize)
        SS = _flat_in(torch.from_numpy(ref["sums"].astype(np.float32)), dev) if normalize else None
        W1 = None if x["snr"] is None else _flat_in(torch.from_numpy(x["snr"]), dev)
        W2 = None if x["lw"] is None else _flat_in(torch.from_numpy(x["lw"]), dev)
        k32 = mr.sample_factors(B, h * w, ref["sums"].astype(np.float32), x["snr"], x["lw"], normalize, dtype=np.float32)
        want_dp = torch.zeros(B, h, w, cpad, dtype=BF)
        want_dp[..., :C] = mr.dpred_chain32(x["pred"], x["target"], x["e"], k32)
        want_loss, want_lps = l0 + ref["loss"], ref["loss_per_sample"]
        runs = []
        for run in range(3):
            if not first:
                _poison_slabs(ws)
            first = False
            L, LPS = _flat_io(torch.tensor([l0]), dev), _flat_out(B, dev)
            DP = Guarded(B * h * w, cpad, BF, dev, pad=0) if has_dp else None
            _lib.call("sdt_masked_mse_loss_fwd_bwd", P.ptr, T.ptr, _ptr(E), _ptr(SS), _ptr(W1), _ptr(W2), L.ptr, LPS.ptr, _ptr(DP), B, C, h, w, cpad,
                      ws.data_ptr(), ws.numel(), _stream())
            torch.cuda.synchronize()
            got, got_lps = float(L.t.item()), LPS.t.cpu().view(B).double().numpy()
            print(f"masked MSE {what} run {run}: loss {got!r}, float64 {want_loss!r}; per sample {got_lps.tolist()} float64 {want_lps.tolist()}")
            if pow2:
                msg = kc.sum_report(got, want_loss, f"{what} run {run}: loss_accum", init=l0)
                assert msg is None, msg
                assert np.array_equal(got_lps, want_lps), f"{what} run {run}: loss_per_sample {got_lps.tolist()}, want {want_lps.tolist()}"
            else:
                for g, r, label in [(got, want_loss, "loss_accum")] + [(got_lps[b], want_lps[b], f"loss_per_sample[{b}]") for b in range(B)]:
                    if r == 0:
                        assert g == 0, f"{what}: {label} {g!r}, want 0"
                        continue
                    ulp = 2.0 ** (math.floor(math.log2(r)) - 23)
                    assert abs(g - r) <= 2 * ulp, f"{what}: {label} {g!r}, float64 {r!r}: {abs(g - r) / ulp:.2f} fp32 ulps"
            if zero:
                assert got_lps[B - 1] == 0 and np.isfinite(got_lps).all()
            L.check(f"{what}: loss_accum"); LPS.check(f"{what}: loss_per_sample")
            if DP is not None:
                dp = DP.t.contiguous().cpu().view(B, h, w, cpad)
                assert_equal_bits(dp, want_dp, f"{what} run {run}: dpred [image][row][column][channel]")
                if zero:
                    assert torch.isfinite(dp.float()).all() and not dp[B - 1].float().any(), f"{what}: the masked-out sample's gradient is not zero"
                DP.check(f"{what}: dpred")
            kc_msg = kc.counters_report(ws)
            assert kc_msg is None, kc_msg
            runs.append((got, got_lps.tobytes(), None if DP is None else DP.t.contiguous().cpu()))
        for r in runs[1:]:
            assert r[0] == runs[0][0] and r[1] == runs[0][1] and (r[2] is None or torch.equal(r[2].view(torch.int16), runs[0][2].view(torch.int16))), \
                f"{what}: three runs gave different bits"
        if mask_kind in (None, "ones") and (x["lw"] is None or (x["lw"] == 1).all()):
            # the exact case: the plain kernel on the same buffers
            L2, DP2 = _flat_io(torch.tensor([l0]), dev), Guarded(B * h * w, cpad, BF, dev, pad=0)
            _lib.call("sdt_mse_loss_fwd_bwd", P.ptr, T.ptr, _ptr(W1), L2.ptr, DP2.ptr, B, C, h, w, cpad, ws.data_ptr(), ws.numel(), _stream())
            torch.cuda.synchronize()
            assert_equal_bits(runs[0][2].view(B, h, w, cpad), DP2.t.contiguous().cpu().view(B, h, w, cpad),
                              f"{what}: dpred against sdt_mse_loss_fwd_bwd [image][row][column][channel]")
            if pow2:
                assert float(L2.t.item()) == runs[0][0], f"{what}: exact losses differ: plain {float(L2.t.item())!r}, masked {runs[0][0]!r}"
            _counters_zero(ws)
        for gd, label in ((E, "mask"), (SS, "sums"), (W1, "snr weight"), (W2, "loss weight")):
            if gd is not None:
                gd.check(label)
    P.check("pred"); T.check("target")


def test_loss_weight_scales_one_samples_gradient_and_loss_share_exactly(dev):
    """Random (not integer) operands: with loss_weight (1, w), w a power of two, sample 1's dpred is exactly w times its dpred under unit
    weights (a power-of-two scale commutes with every rounding of the chain, bf16 included, short of under- and overflow), sample 0's is
    unchanged, and loss_per_sample[1] scales exactly."""
    from stable_diffusion_training_amd import _lib
    B, C, h, w, cpad = 2, 4, 16, 24, 8
    ws = _workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    g = torch.Generator().manual_seed(17)
    pred = torch.zeros(B, h, w, cpad)
    pred[..., :C] = torch.randn(B, h, w, C, generator=g)
    pred, target = pred.to(BF).to(dev), torch.randn(B, C, h, w, generator=g).to(dev)
    e = torch.rand(B, h, w, generator=g).to(dev)
    out = {}
    for scale in (1.0, 0.25, 4.0):
        lw = torch.tensor([1.0, scale], device=dev)
        loss, lps, dp = torch.zeros(1, device=dev), torch.empty(B, device=dev), torch.empty(B, h, w, cpad, dtype=BF, device=dev)
        _lib.call("sdt_masked_mse_loss_fwd_bwd", pred.data_ptr(), target.data_ptr(), e.data_ptr(), None, None, lw.data_ptr(), loss.data_ptr(),
                  lps.data_ptr(), dp.data_ptr(), B, C, h, w, cpad, ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        out[scale] = (lps.cpu(), dp.cpu())
    base_lps, base_dp = out[1.0]
    assert base_dp[1].float().abs().max() > 0
    for scale in (0.25, 4.0):
        lps, dp = out[scale]
        assert torch.equal(dp[0].view(torch.int16), base_dp[0].view(torch.int16)) and lps[0] == base_lps[0]
        assert_equal_bits(dp[1], (base_dp[1].float() * scale).to(BF), f"loss_weight {scale}: sample 1's dpred against the scaled unit-weight one")
        assert float(lps[1]) == float(base_lps[1]) * scale
