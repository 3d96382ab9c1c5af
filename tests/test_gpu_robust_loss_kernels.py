"""sdt_robust_loss_fwd_bwd on a real MI355X (reference, restated chain and case tables: tests/robust_loss_reference.py; what the CPU can
prove about them: tests/test_robust_loss_cpu.py).

Random operands: the element is formed in double from fp32 operands and rounded once, every other operation is a single fp32
multiplication or an addition in a fixed order, so dpred, loss_per_sample and loss_accum must equal the restated chain in every bit -
not only on exact-answer inputs.  Against the float64 reference the sums are bounded as derived in DESIGN.md "Huber and smooth-L1
loss".  Outputs sit between sentinel guards, inputs between NaN guards, pred's padding channels hold NaN; every call runs three times
over differently poisoned scratch and must leave its arrival counters at zero."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import masked_loss_reference as mr
from tests import robust_loss_reference as rr
from tests.kernel_checks import BF, Guarded, assert_equal_bits
from tests.test_gpu_kernel_exact import _stream, _workspace
from tests.test_gpu_masked_loss_kernels import _flat_in, _flat_io, _flat_out, _ptr

pytestmark = pytest.mark.gpu
F32 = np.float32


def _pred_operand(x, C, cpad, shifted, dev):
    """pred (B,h,w,cpad) bf16 with NaN in the padding channels, between NaN guards; shifted: one element behind a 16-byte boundary.
    Returns (guarded arena, device pointer)."""
    B, h, w, _ = x["pred"].shape
    pred = torch.full((B, h, w, cpad), float("nan"))
    pred[..., :C] = torch.from_numpy(x["pred"])
    if not shifted:
        P = Guarded(B * h * w, cpad, BF, dev, data=pred, pad=0)
        return P, P.ptr
    flat = torch.cat([torch.full((1,), float("nan")), pred.reshape(-1)])
    P = Guarded(1, flat.numel(), BF, dev, data=flat.reshape(1, -1), pad=0, back_rows=0)
    assert (P.ptr + 2) % 16 == 2
    return P, P.ptr + 2


@pytest.mark.parametrize("loss_type", ["huber", "smooth_l1"])
@pytest.mark.parametrize("case", rr.CASES, ids=[c[0] for c in rr.CASES])
def test_robust_loss_and_gradient_equal_the_restated_chain_bit_for_bit(dev, case, loss_type):
    """Every variant of rr.VARIANTS (null mask; mask with null sums; normalisation; either weight null; both weights; no dpred).
    dpred, loss_per_sample and loss_accum (0.5 before): the restated chain, bit for bit, three runs.  loss_per_sample and the loss
    against float64: m = C*h*w summands of 5 roundings at most (the fp32 diff twice through the square, the double operations, the
    rounding of rho, the product with e), m - 1 additions, k_b (3, and h*w more where S_b is an fp32 sum) and the two scalings (3):
    gamma(m + h*w + 11) per sample, and B + 2 more for the B terms, the scaling and the addition to loss_accum."""
    from stable_diffusion_training_amd import _lib
    name, B, C, h, w, cpad, shifted = case
    t = rr.TYPES[loss_type]
    ws = _workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    m, l0 = C * h * w, rr.LOSS_ACCUM_BEFORE
    P = T = HC = None
    for variant in rr.VARIANTS:
        what = f"{name} {loss_type} {variant[0]}"
        x = rr.random_inputs(case, variant)
        if P is None:  # pred, target and the thresholds are the same for every variant of a case
            (P, pred_ptr), T, HC = _pred_operand(x, C, cpad, shifted, dev), _flat_in(torch.from_numpy(x["target"]), dev), _flat_in(torch.from_numpy(x["c"]), dev)
        E, SS, W1, W2 = (None if x[key] is None else _flat_in(torch.from_numpy(x[key]), dev) for key in ("e", "sums", "snr", "lw"))
        ref = rr.reference(x["pred"], x["target"], x["c"], t, x["e"], x["snr"], x["lw"], x["normalize"])
        k32 = mr.sample_factors(B, h * w, x["sums"], x["snr"], x["lw"], x["normalize"], dtype=F32)
        chain_dp, terms = rr.chain(x["pred"], x["target"], x["c"], t, x["e"], k32)
        want_dp = torch.zeros(B, h, w, cpad, dtype=BF)
        want_dp[..., :C] = chain_dp
        want_loss, want_lps = rr.ordered_loss(terms, k32, C, l0)
        runs = []
        for run in range(3):
            ws[kc.CNT_BYTES:].fill_(rr.POISON[run])
            L, LPS = _flat_io(torch.tensor([l0]), dev), _flat_out(B, dev)
            DP = Guarded(B * h * w, cpad, BF, dev, pad=0) if x["dpred"] else None
            _lib.call("sdt_robust_loss_fwd_bwd", pred_ptr, T.ptr, _ptr(E), _ptr(SS), _ptr(W1), _ptr(W2), HC.ptr, t, L.ptr, LPS.ptr, _ptr(DP), B, C, h, w,
                      cpad, ws.data_ptr(), ws.numel(), _stream())
            torch.cuda.synchronize()
            got, got_lps = L.t.cpu().view(1).numpy()[0], LPS.t.cpu().view(B).numpy()
            print(f"robust loss {what} run {run}: loss {float(got)!r}, chain {float(want_loss)!r}, float64 {l0 + ref['loss']!r}; per sample "
                  f"{got_lps.tolist()} chain {want_lps.tolist()} float64 {ref['loss_per_sample'].tolist()}")
            assert got.tobytes() == want_loss.tobytes(), f"{what} run {run}: loss_accum {float(got)!r}, restated chain {float(want_loss)!r}"
            assert got_lps.tobytes() == want_lps.tobytes(), f"{what} run {run}: loss_per_sample {got_lps.tolist()}, restated chain {want_lps.tolist()}"
            bound = rr.gamma(m + h * w + B + 13) * ref["loss"] + rr.U * (l0 + ref["loss"])
            assert abs(float(got) - l0 - ref["loss"]) <= bound, f"{what}: loss {float(got) - l0!r}, float64 {ref['loss']!r}, bound {bound:.3e}"
            err = np.abs(got_lps.astype(np.float64) - ref["loss_per_sample"])
            assert (err <= rr.gamma(m + h * w + 11) * ref["loss_per_sample"]).all(), f"{what}: loss_per_sample error {err.tolist()}"
            assert np.isfinite(got_lps).all()
            L.check(f"{what}: loss_accum"); LPS.check(f"{what}: loss_per_sample")
            if DP is not None:
                dp = DP.t.contiguous().cpu().view(B, h, w, cpad)
                assert_equal_bits(dp, want_dp, f"{what} run {run}: dpred [image][row][column][channel]")
                DP.check(f"{what}: dpred")
            msg = kc.counters_report(ws)
            assert msg is None, msg
            runs.append(None if DP is None else DP.t.contiguous().cpu())
        if name == "b3_zero":
            assert got_lps[1] == 0 and (runs[0] is None or not runs[0].view(B, h, w, cpad)[1].float().any()), f"{what}: r = 0 must give zero"
            if x["normalize"]:
                assert got_lps[2] == 0 and not runs[0].view(B, h, w, cpad)[2].float().any(), f"{what}: S_b = 0 must give zero"
        for gd, label in ((E, "mask"), (SS, "sums"), (W1, "snr weight"), (W2, "loss weight")):
            if gd is not None:
                gd.check(label)
    P.check("pred"); T.check("target"); HC.check("huber_c")


def test_a_large_threshold_tends_to_the_squared_error_kernel(dev):
    """huber with c = 2^12 and |diff| < 8: rho = diff^2 (1 - O(diff^2 / c^2)), so loss_per_sample is within (m + 11) u + 2^-20 of
    sdt_masked_mse_loss_fwd_bwd's on the same buffers - the two exports share every operand's meaning."""
    from stable_diffusion_training_amd import _lib
    B, C, h, w, cpad = 2, 4, 8, 8, 8
    ws = _workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    x = rr.random_inputs(rr.CASES[0], rr.VARIANTS[4])
    pred = torch.zeros(B, h, w, cpad)
    pred[..., :C] = torch.from_numpy(x["pred"])
    pred, target = pred.to(BF).to(dev), torch.from_numpy(x["target"]).to(dev)
    e, S, w1, w2 = (torch.from_numpy(x[k]).to(dev) for k in ("e", "sums", "snr", "lw"))
    hc = torch.full((B,), 4096.0, device=dev)
    out = []
    for robust in (False, True):
        loss, lps = torch.zeros(1, device=dev), torch.empty(B, device=dev)
        head = (pred.data_ptr(), target.data_ptr(), e.data_ptr(), S.data_ptr(), w1.data_ptr(), w2.data_ptr())
        tail = (loss.data_ptr(), lps.data_ptr(), None, B, C, h, w, cpad, ws.data_ptr(), ws.numel(), _stream())
        if robust:
            _lib.call("sdt_robust_loss_fwd_bwd", *head, hc.data_ptr(), rr.HUBER, *tail)
        else:
            _lib.call("sdt_masked_mse_loss_fwd_bwd", *head, *tail)
        torch.cuda.synchronize()
        out.append(lps.cpu().double().numpy())
    assert (out[0] > 0).all() and (np.abs(out[1] - out[0]) <= (2 * rr.gamma(C * h * w + 11) + 2.0 ** -20) * out[0]).all(), out
