"""The Huber / smooth-L1 loss without a GPU: the float64 reference against autograd, the stable form against the definition, the
threshold schedules, the proof that the exact-answer inputs are exact in fp32 (so the restated chain equals the float64 reference in
every bit), the export, every host refusal of sdt_robust_loss_fwd_bwd and every ValueError of train_step's three options."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

from tests import masked_loss_reference as mr
from tests import robust_loss_reference as rr
from tests.kernel_checks import LIMIT

F32, F64 = np.float32, np.float64


# ================================================================================================ the reference itself
@pytest.mark.parametrize("loss_type", ["huber", "smooth_l1"])
@pytest.mark.parametrize("masked,normalize,weights", [(False, False, False), (True, False, False), (True, True, True), (False, False, True)])
def test_reference_gradient_equals_float64_autograd_of_the_written_out_loss(loss_type, masked, normalize, weights):
    """mean(k_b * e * rho) with rho written as the definition 2c(r - c) / 2(r - c), in torch float64."""
    B, C, h, w = 3, 3, 4, 6
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(B, h, w, C, generator=g, dtype=torch.float64), torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    c = torch.tensor([0.1, 0.6, 1.0]).double()
    e = torch.rand(B, h, w, generator=g, dtype=torch.float64) if masked else torch.ones(B, h, w).double()
    if masked:
        e[2] = 0.0  # a fully masked-out sample
    snr, lw = (torch.tensor([0.7, 1.0, 0.3]).double(), torch.tensor([1.0, 0.5, 2.0]).double()) if weights else (None, None)
    t = rr.TYPES[loss_type]
    ref = rr.reference(pred.numpy(), target.numpy(), c.numpy(), t, e.numpy() if masked else None, None if snr is None else snr.numpy(),
                       None if lw is None else lw.numpy(), normalize)
    p = pred.clone().requires_grad_(True)
    S = e.reshape(B, -1).sum(1)
    s = torch.where(S == 0, torch.zeros_like(S), h * w / torch.where(S == 0, torch.ones_like(S), S)) if normalize else torch.ones(B).double()
    k = (snr * lw if weights else torch.ones(B).double()) * s
    diff = target.permute(0, 2, 3, 1) - p
    cb = c[:, None, None, None]
    r = torch.sqrt(diff ** 2 + cb ** 2)
    rho = 2 * cb * (r - cb) if loss_type == "huber" else 2 * (r - cb)
    per = (e[..., None] * rho).reshape(B, -1).sum(1)
    loss = (k * per).sum() / (B * C * h * w)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-13 * abs(ref["loss"])
    assert np.allclose(p.grad.numpy(), ref["grad"], rtol=1e-12, atol=1e-18)
    assert np.allclose((k * per / (C * h * w)).detach().numpy(), ref["loss_per_sample"], rtol=1e-12, atol=0)
    assert abs(ref["loss_per_sample"].mean() - ref["loss"]) <= 1e-14 * abs(ref["loss"])
    if masked:
        assert ref["loss_per_sample"][2] == 0 and not ref["grad"][2].any()
    assert np.isfinite(ref["grad"]).all()


@pytest.mark.parametrize("loss_type", [rr.HUBER, rr.SMOOTH_L1])
def test_stable_form_equals_the_definition_where_nothing_cancels(loss_type):
    """|diff| >= c: r - c >= (sqrt(2) - 1) c loses at most two bits, so the two float64 forms agree to 1e-12 relative.  Below, the
    definition loses digits and the stable form does not: at diff = 1e-9 c it still equals the series diff^2 (huber) to 1e-15."""
    g = np.random.default_rng(0)
    c = g.uniform(0.01, 1.0, 4000)
    diff = c * g.uniform(1.0, 1000.0, 4000) * g.choice([-1.0, 1.0], 4000)
    a, b = rr.rho64(diff, c, loss_type), rr.rho_plain64(diff, c, loss_type)
    assert (np.abs(a - b) <= 1e-12 * np.abs(b)).all() and (b > 0).all()
    small = 1e-9 * c
    series = small ** 2 if loss_type == rr.HUBER else small ** 2 / c  # rho = (2c | 2) * diff^2 / (2c) (1 + O(diff^2 / c^2))
    assert (np.abs(rr.rho64(small, c, loss_type) - series) <= 1e-15 * series).all()
    assert (np.abs(rr.rho_plain64(small, c, loss_type) - series) > 1e-3 * series).any(), "the definition should have cancelled here"
    # r == 0: zero loss, zero gradient, no NaN - in the float64 reference and in the restated chain
    assert rr.rho64(0.0, 0.0, loss_type) == 0 and rr.drho64(0.0, 0.0, loss_type) == 0
    g0, rho0 = rr.element_chain(F32(0), F32(0), loss_type)
    assert g0 == 0 and rho0 == 0


@pytest.mark.parametrize("loss_type", [rr.HUBER, rr.SMOOTH_L1])
def test_restated_chain_is_within_one_rounding_of_the_float64_element(loss_type):
    """g and rho of the chain are fp32 roundings of double results that carry at most 4 double roundings: |error| <= (1/2 + 2^-26) ulp."""
    g = np.random.default_rng(1)
    diff, c = g.standard_normal(5000).astype(F32), g.uniform(0.05, 1.0, 5000).astype(F32)
    gg, rho = rr.element_chain(diff, c, loss_type)
    for got, want in ((gg, rr.drho64(diff, c, loss_type)), (rho, rr.rho64(diff, c, loss_type))):
        assert (np.abs(got.astype(F64) - want) <= (2.0 ** -24 + 2.0 ** -50) * np.abs(want)).all()


# ================================================================================================ the schedule
def _acp(name):
    from stable_diffusion_training_amd.schedulers import make_betas
    betas = make_betas(name, 0.00085, 0.012, 1000)
    return np.cumprod((F32(1) - betas).astype(F32), dtype=F32)


def test_threshold_schedules():
    from stable_diffusion_training_amd import training_utils as tu
    T, c = 1000, 0.1
    sl, zs = _acp("scaled_linear"), _acp("zero_snr_scaled_linear")
    assert zs[-1] == 0 and sl[-1] > 0
    const = tu.huber_threshold_table(sl, c, "constant")
    assert const.dtype == F32 and const.shape == (T,) and (const == F32(c)).all()
    expo = tu.huber_threshold_table(sl, c, "exponential")
    assert expo[0] == 1.0 and expo.dtype == F32
    # c[T] = huber_c: the table ends one step short of it, at huber_c^((T-1)/T)
    assert abs(float(expo[-1]) - math.exp((T - 1) * math.log(c) / T)) <= 2.0 ** -24 * expo[-1] and c < expo[-1] < c * 1.0024
    snr = tu.huber_threshold_table(zs, c, "snr")
    assert snr.dtype == F32 and np.isfinite(snr).all() and snr[-1] == F32(c)
    # the formula, entry by entry in float64, rounded once
    t = 123
    sigma = math.sqrt((1.0 - float(zs[t])) / float(zs[t]))
    assert snr[t] == F32((1.0 - c) / ((1.0 + sigma) * (1.0 + sigma)) + c)
    for name in tu.HUBER_SCHEDULES:
        tab = tu.huber_threshold_table(sl, c, name)
        assert (np.diff(tab.astype(F64)) <= 0).all(), f"{name} must not increase with t"
        assert (tab >= F32(c)).all() and (tab <= 1).all()
    assert (np.diff(snr.astype(F64)) <= 0).all()
    assert (tu.huber_threshold_table(sl, 1.0, "snr") == 1).all() and (tu.huber_threshold_table(sl, 1.0, "exponential") == 1).all()
    assert (tu.huber_threshold_table(sl, 2.5, "constant") == 2.5).all()


def test_thresholds_of_a_batch_are_gathered_from_one_cached_table():
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.schedulers import DDPMScheduler
    sched = DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="zero_snr_scaled_linear", num_train_timesteps=1000)
    state = sched.create_state("cpu")
    ts = torch.tensor([0, 999, 500, 500], dtype=torch.int32)
    got = tu._huber_thresholds(state, ts, 0.1, "snr")
    want = tu.huber_threshold_table(state.alphas_cumprod.numpy(), 0.1, "snr")[ts.numpy()]
    assert got.dtype == torch.float32 and got.is_contiguous() and np.array_equal(got.numpy(), want)
    tab = state._huber_tables[("snr", 0.1)]
    tu._huber_thresholds(state, ts, 0.1, "snr")
    tu._huber_thresholds(state, ts, 0.3, "constant")
    assert state._huber_tables[("snr", 0.1)] is tab and set(state._huber_tables) == {("snr", 0.1), ("constant", 0.3)}


# ================================================================================================ the exact-answer inputs
@pytest.mark.parametrize("B,C,h,w", rr.EXACT_SHAPES)
@pytest.mark.parametrize("loss_type", [rr.HUBER, rr.SMOOTH_L1])
def test_the_exact_cases_are_exact_in_fp32(B, C, h, w, loss_type):
    """Sample b, j = EXACT_J[b % 3]: diff = s 3 2^j with s in {-1, 0, 1} and c = 4 2^j.  In double dd = 9 4^j s^2, c^2 = 16 4^j, their sum
    25 4^j (or 16 4^j) and its root 5 2^j (4 2^j) are exact; den = 9 2^j (8 2^j).  huber: 2c dd = 72 8^j s^2, over den: 8 4^j s^2, exact.
    smooth_l1: 2 dd / den = 2 2^j s^2, exact.  So rho is {0, 8 4^j} or {0, 2 2^j}: with a mask in {0, 1/4, 1/2, 1} every summand e * rho is
    a multiple of q = rho_min / 4 = (1/2 | 1/4) over all j, every partial sum of a sample is such a multiple below 2^24 q (checked), k_b
    is a power of two: the restated ordered chain adds without rounding and must equal the float64 reference - a_b in every bit, and the
    loss and loss_per_sample too where the counts are powers of two (otherwise up to the two roundings of the reciprocal scaling)."""
    x = rr.exact_inputs(B, C, h, w, seed=3)
    diff = (x["target"].transpose(0, 2, 3, 1) - x["pred"]).astype(F32)
    assert np.array_equal(diff, 3.0 * x["s"] * x["scale"][:, None, None, None])
    assert set(np.unique(x["e"])) <= set(mr.MASK_VALUES) and set(np.unique(x["s"])) == {-1.0, 0.0, 1.0}
    cb = x["c"][:, None, None, None]
    g, rho = rr.element_chain(diff, cb, loss_type)
    sc = x["scale"][:, None, None, None].astype(F64)
    want_rho = (8.0 * sc * sc if loss_type == rr.HUBER else 2.0 * sc) * x["s"] ** 2
    assert np.array_equal(rho.astype(F64), want_rho)
    assert np.array_equal(rho.astype(F64), rr.rho64(diff, cb, loss_type)), "the float64 reference is exact here too"
    assert np.array_equal(g.astype(F64), rr.drho64(diff, cb, loss_type).astype(F32).astype(F64))  # -24/5 2^j resp. -6/5: one rounding
    q = 0.5 if loss_type == rr.HUBER else 0.25
    terms64 = x["e"][..., None].astype(F64) * want_rho
    assert (terms64 / q == np.round(terms64 / q)).all() and terms64.reshape(B, -1).sum(1).max() / q < LIMIT
    k32 = mr.sample_factors(B, h * w, None, x["snr"], x["lw"], False, dtype=F32)
    assert (np.log2(k32) == np.round(np.log2(k32))).all() and (k32.astype(F64) * terms64.reshape(B, -1).sum(1)).sum() / (q / 2) < LIMIT
    ref = rr.reference(x["pred"], x["target"], x["c"], loss_type, x["e"], x["snr"], x["lw"], False)
    _, terms = rr.chain(x["pred"], x["target"], x["c"], loss_type, x["e"], k32)
    assert np.array_equal(terms.astype(F64).reshape(terms64.shape), terms64)
    nb = mr.partition(B, h * w)
    a = np.array([mr.ordered_sum32(terms[b], nb) for b in range(B)], F64)
    assert np.array_equal(a, terms64.reshape(B, -1).sum(1)), "a_b must be exact"
    loss, lps = rr.ordered_loss(terms, k32, C, 0.0)
    count = B * C * h * w
    if count & (count - 1) == 0:
        assert float(loss) == ref["loss"] and np.array_equal(lps.astype(F64), ref["loss_per_sample"])
    else:
        assert abs(float(loss) - ref["loss"]) <= rr.gamma(2) * ref["loss"]
        assert (np.abs(lps - ref["loss_per_sample"]) <= rr.gamma(2) * ref["loss_per_sample"]).all()


def test_random_case_tables_are_well_formed():
    """Every (case, variant) of the GPU test: shapes, the b3_zero specials, and the restated chain within the derived bound of the float64
    reference (the bound the GPU test asserts for the kernel; DESIGN.md "Huber and smooth-L1 loss")."""
    assert [c[0] for c in rr.CASES] == ["vec", "scalar_cpad4", "misaligned", "over_cap", "b3_zero"]
    assert mr.partition(1, 192 * 192) == 128 and 192 * 192 > 128 * 256
    for case in rr.CASES[:3] + rr.CASES[4:]:
        name, B, C, h, w, cpad, _ = case
        for variant in rr.VARIANTS:
            x = rr.random_inputs(case, variant)
            assert x["pred"].shape == (B, h, w, C) and x["target"].shape == (B, C, h, w) and (x["c"] >= 0).all()
            if name == "b3_zero":
                assert x["c"][1] == 0 and np.array_equal(x["target"][1], x["pred"][1].transpose(2, 0, 1)) and x["c"][0] > 0
                if x["normalize"]:
                    assert x["sums"][2] == 0 and x["sums"][0] > 0
            for t in (rr.HUBER, rr.SMOOTH_L1):
                ref = rr.reference(x["pred"], x["target"], x["c"], t, x["e"], x["snr"], x["lw"], x["normalize"])
                k32 = mr.sample_factors(B, h * w, x["sums"], x["snr"], x["lw"], x["normalize"], dtype=F32)
                dp, terms = rr.chain(x["pred"], x["target"], x["c"], t, x["e"], k32)
                loss, lps = rr.ordered_loss(terms, k32, C, 0.0)
                m = C * h * w
                assert np.isfinite(dp.float().numpy()).all() and np.isfinite(lps).all()
                assert abs(float(loss) - ref["loss"]) <= rr.gamma(m + h * w + B + 13) * ref["loss"]
                assert (np.abs(lps - ref["loss_per_sample"]) <= rr.gamma(m + h * w + 11) * ref["loss_per_sample"]).all()
                if name == "b3_zero":
                    assert lps[1] == 0 and not dp[1].float().any()


# ================================================================================================ export and host refusals
def test_library_exports_the_entry_point_with_abi_5(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_abi_version() == 5
    assert hasattr(lib, "sdt_robust_loss_fwd_bwd") and len(_lib.SIGNATURES["sdt_robust_loss_fwd_bwd"]) == 19
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdt.h")).read()
    assert "ROBUST LOSS" in header and "int sdt_robust_loss_fwd_bwd(" in header


def test_host_refusals_without_a_gpu(lib):
    """Every refusal returns before any HIP call.  Pointers are made-up aligned addresses: nothing dereferences them."""
    P, WS = 4096, lib.sdt_reduce_workspace_bytes()
    err = lambda: lib.sdt_last_error()
    loss = lambda pred=P, tgt=P, e=None, S=None, w1=None, w2=None, hc=P, t=1, la=P, lps=P, dp=P, B=2, C=4, H=8, W=8, cpad=8, ws=P, wsb=WS: \
        lib.sdt_robust_loss_fwd_bwd(pred, tgt, e, S, w1, w2, hc, t, la, lps, dp, B, C, H, W, cpad, ws, wsb, None)
    for kw in (dict(pred=None), dict(tgt=None), dict(hc=None), dict(la=None), dict(lps=None)):
        assert loss(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(pred=P + 1), dict(dp=P + 1), dict(tgt=P + 2), dict(e=P + 2), dict(e=P, S=P + 1), dict(w1=P + 2), dict(w2=P + 3), dict(hc=P + 2),
               dict(la=P + 2), dict(lps=P + 2)):
        assert loss(**kw) == -1 and b"misaligned" in err(), kw
    for t in (0, 3, -1, 16):
        assert loss(t=t) == -1 and b"1 huber, 2 smooth_l1" in err(), t
    assert loss(cpad=3) == -1 and b"cpad=3 < C=4" in err()
    for kw in (dict(B=0), dict(B=-2), dict(B=8193), dict(C=0), dict(H=0), dict(W=-1)):
        assert loss(**kw) == -1 and b"bad shape" in err(), kw
    assert loss(S=P) == -1 and b"need the effective mask" in err()
    for kw in (dict(ws=None), dict(wsb=WS - 1), dict(ws=P + 8)):
        assert loss(**kw) == -1 and b"workspace" in err(), kw


# ================================================================================================ train_step's options
def test_train_step_refuses_bad_loss_options_before_anything_else():
    """The three options are checked first: no state, batch or device is touched (every other argument is None)."""
    from stable_diffusion_training_amd import training_utils as tu
    step = lambda **kw: tu.train_step(None, None, None, None, {}, None, None, None, **kw)
    bad = [
        (dict(loss_type="l1"), "loss_type="), (dict(loss_type="Huber"), "loss_type="), (dict(loss_type=1), "loss_type="),
        (dict(loss_type="huber", huber_schedule="linear"), "huber_schedule="), (dict(huber_schedule=None), "huber_schedule="),
        (dict(loss_type="huber", huber_c=0.0), "finite number > 0"), (dict(loss_type="huber", huber_c=-0.1), "finite number > 0"),
        (dict(loss_type="smooth_l1", huber_c=float("nan")), "finite number > 0"), (dict(loss_type="huber", huber_c=float("inf")), "finite number > 0"),
        (dict(loss_type="huber", huber_c="0.1"), "finite number > 0"), (dict(loss_type="huber", huber_c=True), "finite number > 0"),
        (dict(loss_type="huber", huber_c=1.5), "needs huber_c <= 1"), (dict(loss_type="huber", huber_c=1.5, huber_schedule="exponential"), "needs huber_c <= 1"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            step(**kw)
    # well-formed options pass the check: the step goes on to its states (None here)
    for kw in (dict(), dict(loss_type="l2"), dict(loss_type="huber"), dict(loss_type="smooth_l1", huber_c=1, huber_schedule="exponential"),
               dict(loss_type="huber", huber_c=2.5, huber_schedule="constant")):
        with pytest.raises(AttributeError):
            step(**kw)
    assert tu.LOSS_TYPES == {"l2": 0, "huber": rr.HUBER, "smooth_l1": rr.SMOOTH_L1}
    assert len(dataclasses.fields(tu.TrainingConfig)) == 28


def test_example_reads_the_flags_from_the_config():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_synthetic.py")).read()
    for flag, key in (("--loss-type", '"loss_type"'), ("--huber-c", '"huber_c"'), ("--huber-schedule", '"huber_schedule"')):
        assert flag in src and f"cfg[{key}]" in src and f"config_dict.get({key}" in src
