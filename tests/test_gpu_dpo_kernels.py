"""sdt_dpo_loss_fwd_bwd and sdt_lora_restore on a real MI355X (include/sdt.h "DPO LOSS"; reference and chains: tests/dpo_reference.py).

Loss inputs: pred, ref_pred and target hold multiples of 1/4 in [-1, 1], so a difference is a multiple of 1/4 of magnitude <= 2, its
square a multiple of 1/16 that is <= 4, and a sum of up to C*h*w = 16384 of them a multiple of 1/16 below 2^16: every partial sum is
exact in fp32 in any order, and sample_mse must equal fl(a_b * fl(1/(C*h*w))) of the float64 sum a_b in every bit, whatever the
partition or the workgroup that arrives last.  Everything after sample_mse is checked from the PUBLISHED values before it: logits bit
for bit (only +, -, x in double, one rounding), pair_loss and coef within 1 fp32 ulp (the device's double exp / log1p are not correctly
rounded - the only tolerance in this file), dpred bit for bit from the published coef, loss_accum bit for bit from the published
pair_loss.  Outputs sit between sentinel guards, inputs between NaN guards, the padding channels of pred / ref_pred hold NaN; every case
runs three times over a poisoned scratch area, must give equal bits and must leave its arrival counters at zero."""
import math

import numpy as np
import pytest
import torch

from tests import dpo_reference as dref
from tests import kernel_checks as kc
from tests.kernel_checks import BF, Guarded, assert_equal_bits
from tests.test_gpu_kernel_exact import _poison_slabs, _stream, _workspace

pytestmark = pytest.mark.gpu
F32 = torch.float32
SDT_ERR_INVALID_ARG = -1
POISON16 = 0x7FA5

# (name, P, C, h, w, cpad)
SHAPES = [("one-workgroup", 1, 4, 8, 8, 8),
          ("nb2-ragged-tail", 3, 4, 15, 20, 8),
          ("element-path-cpad-eq-C", 2, 4, 5, 7, 4),
          ("nan-padding-C3", 2, 3, 8, 8, 8),
          ("nb16", 2, 4, 64, 64, 8)]
BETA = 6.0
LOSS_BEFORE = 0.5


def _flat_in(data, dev):
    return Guarded(1, data.numel(), F32, dev, data=data.reshape(1, -1), pad=0, back_rows=0)


def _flat_out(n, dev):
    return Guarded(1, n, F32, dev, pad=0, back_rows=0)


def _flat_io(data, dev):
    g = _flat_out(data.numel(), dev)
    g.t.copy_(data.reshape(1, -1))
    return g


def _quarters(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, tuple(shape), generator=g).to(F32) / 4


def _inputs(P, C, h, w, seed):
    B = 2 * P
    return _quarters((B, h, w, C), seed), _quarters((B, h, w, C), seed + 1), _quarters((B, C, h, w), seed + 2)


def _padded(x, cpad):
    """(B,h,w,C) -> (B,h,w,cpad) with NaN in the padding channels: they must never enter the arithmetic."""
    B, h, w, C = x.shape
    out = torch.full((B, h, w, cpad), float("nan"))
    out[..., :C] = x
    return out


def _ulps32(got, want64):
    """|got - want| in units of the fp32 ulp of want (float64 `want`, fp32 `got`); 0 where both are zero."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return np.abs(got - want64) / ulp


class _Run:
    """One launch on guarded buffers; .out holds host copies of every output."""

    def __init__(self, lib, dev, ws, pred, ref, target, beta, C, loss_before=LOSS_BEFORE, shift=0):
        from stable_diffusion_training_amd import _lib
        B, h, w, cpad = pred.shape
        P = B // 2
        self.P_in = Guarded(B * h * w, cpad, BF, dev, data=pred, pad=0)
        self.R_in = Guarded(B * h * w, cpad, BF, dev, data=ref, pad=0)
        self.T_in = _flat_in(target, dev)
        self.L, self.S, self.Z = _flat_io(torch.tensor([loss_before]), dev), _flat_out(2 * B, dev), _flat_out(P, dev)
        self.PL, self.CF = _flat_out(P, dev), _flat_out(B, dev)
        self.DP = Guarded(B * h * w, cpad, BF, dev, pad=0)
        _lib.call("sdt_dpo_loss_fwd_bwd", self.P_in.ptr, self.R_in.ptr, self.T_in.ptr, beta, self.L.ptr, self.S.ptr, self.Z.ptr, self.PL.ptr,
                  self.CF.ptr, self.DP.ptr, B, C, h, w, cpad, ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        self.out = dict(loss=self.L.t.cpu().view(1), sample_mse=self.S.t.cpu().view(2, B), logits=self.Z.t.cpu().view(P),
                        pair_loss=self.PL.t.cpu().view(P), coef=self.CF.t.cpu().view(B), dpred=self.DP.t.cpu().view(B, h, w, cpad))

    def check_guards(self, what):
        for g, n in ((self.P_in, "pred"), (self.R_in, "ref_pred"), (self.T_in, "target"), (self.L, "loss_accum"), (self.S, "sample_mse"),
                     (self.Z, "logits"), (self.PL, "pair_loss"), (self.CF, "coef"), (self.DP, "dpred")):
            g.check(f"{what}: {n}")


def _check_chain(out, pred, target, beta, C, what, loss_before=LOSS_BEFORE):
    """Everything behind sample_mse from the published values before it."""
    B = pred.shape[0]
    m, r = out["sample_mse"][0].numpy(), out["sample_mse"][1].numpy()
    pr = dref.pairs(m, r, beta)
    assert_equal_bits(out["logits"], torch.from_numpy(pr["logits"]), f"{what}: logits from the published sample_mse")
    for name, want in (("pair_loss", pr["pair_loss"]), ("coef", pr["coef"])):
        got = out[name].double().numpy()
        u = _ulps32(got, want)
        print(f"{what}: {name} {got.tolist()} float64 {want.tolist()} ({u.max():.3f} fp32 ulps)")
        assert np.isfinite(got).all() and (u <= 1.0).all(), f"{what}: {name} {got.tolist()} against {want.tolist()}: {u.tolist()} ulps"
    want_dp = torch.zeros_like(out["dpred"])
    want_dp[..., :C] = dref.dpred_chain(out["coef"].numpy(), pred[..., :C].float().numpy(), target.numpy())
    assert_equal_bits(out["dpred"], want_dp, f"{what}: dpred [image][row][column][channel] from the published coef")
    want_loss = np.float32(np.float32(loss_before) + dref.loss_chain(out["pair_loss"].numpy()))
    assert_equal_bits(out["loss"], torch.tensor([want_loss]), f"{what}: loss_accum from the published pair_loss")


# ================================================================================================ sdt_dpo_loss_fwd_bwd
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_dpo_loss_bit_for_bit_on_exact_inputs(dev, lib, shape):
    name, P, C, h, w, cpad = shape
    B, n = 2 * P, C * h * w
    x, y, t = _inputs(P, C, h, w, 100 + P + h)
    ws = _workspace(lib.sdt_dpo_loss_workspace_bytes(B, h, w), dev)
    a_m, a_r = dref.sample_sq_sums(x.numpy(), t.numpy()), dref.sample_sq_sums(y.numpy(), t.numpy())
    assert max(a_m.max(), a_r.max()) * 16 < kc.LIMIT and np.array_equal(a_m * 16, np.round(a_m * 16))  # exact in fp32 in any order
    want_mse = torch.from_numpy(np.stack([dref.publish_mse(a_m, n), dref.publish_mse(a_r, n)]))
    assert len(np.unique(want_mse.numpy())) > 1
    pred, ref = _padded(x, cpad), _padded(y, cpad)
    first = None
    for run in range(3):
        if run:
            _poison_slabs(ws)
        r = _Run(lib, dev, ws, pred, ref, t, BETA, C)
        what = f"{name} run {run}"
        assert_equal_bits(r.out["sample_mse"], want_mse, f"{what}: sample_mse [pass][sample]")
        _check_chain(r.out, pred.to(BF), t, BETA, C, what)
        assert all(torch.isfinite(v.float()).all() for v in r.out.values()), f"{what}: a non-finite output"
        assert not r.out["dpred"][..., C:].float().abs().sum(), f"{what}: dpred padding channels are not zero"
        r.check_guards(what)
        msg = kc.counters_report(ws)
        assert msg is None, msg
        if first is None:
            first = r.out
        else:
            for k, v in r.out.items():
                assert_equal_bits(v, first[k], f"{what}: {k} differs from run 0")
    assert (first["logits"] != 0).any() and first["dpred"].float().abs().sum() > 0


def _known(dev, lib, m_shift_w, m_shift_l, beta, same_ref=False):
    """P = 2 pairs on (C, h, w) = (4, 8, 8): pair 0 is the pair under test - its trained errors are the constants m_shift_w^2 and
    m_shift_l^2 (pred = target - shift), its reference errors are equal (ref = target - 1/2 for both samples), so
    z = -beta/2 * (shift_w^2 - shift_l^2) - pair 1 random quarters."""
    P, C, h, w, cpad = 2, 4, 8, 8, 8
    x, y, t = _inputs(P, C, h, w, 7)
    tt = t.permute(0, 2, 3, 1)
    x[0], x[1] = tt[0] - m_shift_w, tt[1] - m_shift_l
    y[0], y[1] = tt[0] - 0.5, tt[1] - 0.5
    if same_ref:
        y = x.clone()
    ws = _workspace(lib.sdt_dpo_loss_workspace_bytes(2 * P, h, w), dev)
    pred, ref = _padded(x, cpad), _padded(y, cpad)
    r = _Run(lib, dev, ws, pred, ref, t, beta, C)
    _check_chain(r.out, pred.to(BF), t, beta, C, "known answer")
    r.check_guards("known answer")
    assert all(torch.isfinite(v.float()).all() for v in r.out.values())
    return r.out


def test_known_answer_reference_equal_to_the_trained_pass(dev, lib):
    """ref_pred == pred: logits == 0, pair_loss == float32(ln 2) and coef == -+beta/2 exactly, in every pair."""
    out = _known(dev, lib, 0.25, 0.75, 5000.0, same_ref=True)
    assert torch.equal(out["sample_mse"][0], out["sample_mse"][1])
    assert not out["logits"].abs().sum()
    assert_equal_bits(out["pair_loss"], torch.full((2,), float(np.float32(math.log(2.0)))), "pair_loss against float32(ln 2)")
    assert out["coef"].tolist() == [-2500.0, 2500.0, -2500.0, 2500.0]
    assert_equal_bits(out["loss"], torch.tensor([np.float32(np.float32(LOSS_BEFORE) + np.float32(math.log(2.0)))]), "loss_accum")


def test_known_answer_far_on_the_wrong_side(dev, lib):
    """The preferred sample is the worse one by 1 - 1/16: z64 = -5000/2 * 15/16 < -800, so exp(z64) is 0 in double and
    pair_loss == fl(-z64), coef == -+beta, everything finite."""
    out = _known(dev, lib, 1.0, 0.25, 5000.0)
    z = -2500.0 * (1.0 - 0.0625)
    assert out["logits"][0].item() == z and z < -800
    assert out["pair_loss"][0].item() == float(np.float32(-z))
    assert out["coef"][:2].tolist() == [-5000.0, 5000.0]
    assert out["dpred"][:2].float().abs().sum() > 0


def test_known_answer_far_on_the_right_side(dev, lib):
    """The preferred sample is the better one: z64 > 800, pair_loss == 0, coef == 0 and the pair's dpred rows are zero."""
    out = _known(dev, lib, 0.25, 1.0, 5000.0)
    assert out["logits"][0].item() == 2500.0 * (1.0 - 0.0625) > 800
    assert out["pair_loss"][0].item() == 0 and out["coef"][:2].abs().sum() == 0
    assert not out["dpred"][:2].float().abs().sum()
    assert out["coef"][2:].abs().sum() > 0 and out["dpred"][2:].float().abs().sum() > 0  # (the other pair is an ordinary one)


def test_every_abi_refusal_returns_invalid_arg_and_launches_nothing(dev, lib):
    B, C, h, w, cpad = 4, 4, 8, 8, 8
    ws = _workspace(lib.sdt_dpo_loss_workspace_bytes(B, h, w), dev)
    bf = lambda: torch.zeros(B * h * w * cpad + 8, dtype=BF, device=dev)
    f = lambda n: torch.full((n + 4,), 7.0, dtype=F32, device=dev)
    pred, ref, dp, tgt, loss, mse, lg, pl, cf = bf(), bf(), bf(), f(B * C * h * w), f(1), f(2 * B), f(B // 2), f(B // 2), f(B)
    outs = (dp, loss, mse, lg, pl, cf)
    before = [o.clone() for o in outs]
    good = dict(pred=pred.data_ptr(), ref=ref.data_ptr(), tgt=tgt.data_ptr(), beta=5000.0, loss=loss.data_ptr(), mse=mse.data_ptr(),
                lg=lg.data_ptr(), pl=pl.data_ptr(), cf=cf.data_ptr(), dp=dp.data_ptr(), B=B, C=C, h=h, w=w, cpad=cpad, ws=ws.data_ptr(),
                wsn=ws.numel())

    def rc(**kw):
        a = dict(good, **kw)
        return lib.sdt_dpo_loss_fwd_bwd(a["pred"], a["ref"], a["tgt"], a["beta"], a["loss"], a["mse"], a["lg"], a["pl"], a["cf"], a["dp"],
                                        a["B"], a["C"], a["h"], a["w"], a["cpad"], a["ws"], a["wsn"], _stream())

    bad = [dict(**{k: None}) for k in ("pred", "ref", "tgt", "loss", "mse", "lg", "pl", "cf", "dp", "ws")]
    bad += [dict(**{k: good[k] + 1}) for k in ("pred", "ref", "dp")]          # bf16 off a 2-byte boundary
    bad += [dict(**{k: good[k] + 2}) for k in ("tgt", "loss", "mse", "lg", "pl", "cf")]  # f32 off a 4-byte boundary
    bad += [dict(ws=good["ws"] + 8), dict(B=3), dict(B=0), dict(B=1), dict(B=8194), dict(B=-2), dict(cpad=C - 1), dict(C=0), dict(h=0),
            dict(beta=0.0), dict(beta=-1.0), dict(beta=float("nan")), dict(beta=float("inf")),
            dict(wsn=kc.CNT_BYTES + 2 * B * 4 - 1), dict(wsn=0)]
    for kw in bad:
        assert rc(**kw) == SDT_ERR_INVALID_ARG, f"{kw} was not refused"
        assert lib.sdt_last_error().decode().startswith("sdt_dpo_loss_fwd_bwd"), kw
    assert lib.sdt_dpo_loss_workspace_bytes(3, h, w) == -1 and lib.sdt_dpo_loss_workspace_bytes(B, 0, w) == -1
    assert lib.sdt_dpo_loss_workspace_bytes(B, h, w) == lib.sdt_reduce_workspace_bytes()
    assert lib.sdt_dpo_loss_workspace_bytes(128, 512, 512) == kc.CNT_BYTES + 2 * 128 * 127 * 4  # two sets of partials outgrow 64 KiB
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(kc.bits(o), kc.bits(b)), "a refused call wrote an output"
    assert rc() == 0, lib.sdt_last_error().decode()
    torch.cuda.synchronize()


# ================================================================================================ sdt_lora_restore
@pytest.mark.parametrize("dora", [False, True], ids=["lora", "dora"])
def test_restore_gives_the_bits_of_the_adapterless_mirror_and_touches_nothing_else(dev, dora):
    """Random factors merged, then restore(): every adapted leaf of the mirror holds the bits ParamStore.prepare(full=True) leaves in a
    store without an adapter; every other element of the mirror - poisoned beforehand, so each leaf sits between guard words - is
    unchanged; adapter.source is unchanged.  merge() after restore() gives the merge's bits again."""
    from tests.helpers import build_hip_states, make_case
    from tests.test_gpu_dpo import dpo_states, random_factors
    case = make_case("tiny", B=2, image=64)
    plain = build_hip_states(case, dev)[1][0].store
    plain.prepare(full=True)
    us = dpo_states(case, dev, dora=dora)[1][0]
    ad, base = us.adapter, us.store
    ad.store.load(random_factors(ad, case["weights"]["unet"], 21))
    ad.merge("master")
    w = base.w
    spans = sorted((base.leaves[p].w_off, base.leaves[p].w_off + base.leaves[p].numel) for p in ad.paths)
    inside = torch.zeros(w.numel(), dtype=torch.bool, device=dev)
    for a, b in spans:
        inside[a:b] = True
    assert 0 < int(inside.sum()) < w.numel()
    merged = w.clone()
    w.view(torch.int16)[~inside] = POISON16
    poisoned = w.clone()
    ad.restore()
    torch.cuda.synchronize()
    assert ad.source == "master"
    differs = 0
    for p in ad.paths:
        lf, pl = base.leaves[p], plain.leaves[p]
        got, want = w[lf.w_off: lf.w_off + lf.numel], plain.w[pl.w_off: pl.w_off + pl.numel]
        assert_equal_bits(got.view(lf.shape).cpu(), want.view(lf.shape).cpu(), f"restored {p}")
        differs += int((kc.bits(got) != kc.bits(merged[lf.w_off: lf.w_off + lf.numel])).sum())
    assert differs > 0, "the merge changed nothing: the restore was not exercised"
    assert torch.equal(kc.bits(w)[~inside], kc.bits(poisoned)[~inside]), "restore wrote outside the adapted leaves"
    ad.merge("master")
    torch.cuda.synchronize()
    assert torch.equal(kc.bits(w)[inside], kc.bits(merged)[inside]), "merge after restore does not give the merge's bits"
    assert torch.equal(kc.bits(w)[~inside], kc.bits(poisoned)[~inside]), "merge wrote outside the adapted leaves"


def test_restore_refusals(dev, lib):
    """The merge's checks: a null base, mirror or table, a pointer off a 16-byte boundary and a table that does not continue the running
    tile count are refused; n == 0 launches nothing."""
    from stable_diffusion_training_amd import _lib
    job = _lib.SdtLoraJob(0, 0, 64, 0, 0, 0, 0, 64, 16, 16, 4, 1.0, 0, 0, 1, 0)
    table = (_lib.SdtLoraJob * 1)(job)
    tdev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    w0 = torch.arange(256, dtype=F32, device=dev) / 64
    w = torch.zeros(256, dtype=BF, device=dev)
    call = lambda a, b, t, d, n: lib.sdt_lora_restore(a, b, t, d, n, _stream())
    assert call(None, None, None, None, 0) == 0
    for args in ((None, w.data_ptr(), table, tdev.data_ptr(), 1), (w0.data_ptr(), None, table, tdev.data_ptr(), 1),
                 (w0.data_ptr(), w.data_ptr(), None, tdev.data_ptr(), 1), (w0.data_ptr(), w.data_ptr(), table, None, 1),
                 (w0.data_ptr() + 4, w.data_ptr(), table, tdev.data_ptr(), 1), (w0.data_ptr(), w.data_ptr() + 2, table, tdev.data_ptr(), 1),
                 (w0.data_ptr(), w.data_ptr(), table, tdev.data_ptr(), -1)):
        assert call(*args) == SDT_ERR_INVALID_ARG, args
    bad = (_lib.SdtLoraJob * 1)(_lib.SdtLoraJob(0, 0, 64, 0, 0, 0, 0, 64, 16, 16, 4, 1.0, 3, 0, 1, 0))  # tile0_merge off the running count
    assert call(w0.data_ptr(), w.data_ptr(), bad, tdev.data_ptr(), 1) == SDT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not w.float().abs().sum(), "a refused call wrote the mirror"
    assert call(w0.data_ptr(), w.data_ptr(), table, tdev.data_ptr(), 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(w, w0.to(BF))
