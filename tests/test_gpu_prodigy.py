"""Prodigy on a real MI355X: sdt_prodigy_select / sdt_prodigy_finish against their host mirror, the two global sums against exact integer
answers, the two sweeps against the NumPy float32 restatement (tests/prodigy_reference.py) in every bit, ParamStore.optimizer_step for a
Prodigy store (whole, accumulated, scheduled), the train step eager / captured / resumed (full fine-tune, LoRA, DoRA) and two ranks through
gloo.  Outputs and in-place operands sit between sentinel guards, inputs between NaN guards (tests/kernel_checks.py)."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from stable_diffusion_training_amd import lr_schedule as L
from tests import kernel_checks as kc
from tests import prodigy_reference as PR
from tests.helpers import make_case, to_dev
from tests.kernel_checks import BF, assert_equal_bits
from tests.test_gpu_kernel_exact import _stream, _workspace
from tests.test_gpu_reduce_optim_exact import _flat_in, _flat_io, _flat_out, _np

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SIZES = [1, 3, 1023, 1024, 1025, 8191 * 4 + 2, (1 << 20) + 5]


def _same(a, b, what):
    if a.dtype in kc._INT_VIEW:
        assert_equal_bits(a, b, what)
    else:
        assert torch.equal(a, b), f"{what}: {a.tolist()} != {b.tolist()}"


class _Blocks:
    """The device side of the two one-lane kernels between guards (counter, state block, scalar block) and its host mirror."""

    def __init__(self, dev, hp, t0=0):
        self.hp, self.st = hp, PR.init_state(hp, t0)
        self.T = _flat_io(torch.tensor([t0], dtype=torch.int64).view(F64), F64, dev)
        self.S = _flat_io(torch.from_numpy(PR.state_block(self.st)), F64, dev)
        self.CUR = _flat_out(8, F32, dev)
        self.cur = None

    def select(self, ema_rate=0.0, LR=None, EMT=None):
        from stable_diffusion_training_amd import _lib
        hp = self.hp
        tabs = (None, 0, None, 0) if LR is None else (LR.ptr, LR.width, EMT.ptr, EMT.width // 2)
        _lib.call("sdt_prodigy_select", self.T.ptr, self.S.ptr, *tabs, hp["lr"], ema_rate, hp["b1"], hp["b2"], hp["d0"],
                  int(hp["use_bias_correction"]), int(hp["safeguard_warmup"]), self.CUR.ptr, _stream())
        kw = {} if LR is None else dict(lr_tab=_np(LR), ema_tab=_np(EMT).reshape(-1, 2))
        self.cur = PR.select(self.st, hp, ema_rate=ema_rate, **kw)
        return self.cur

    def finish(self):
        from stable_diffusion_training_amd import _lib
        hp = self.hp
        _lib.call("sdt_prodigy_finish", self.S.ptr, self.CUR.ptr, hp["beta3"], hp["d0"], hp["d_coef"], hp["growth_rate"], hp["eps"], _stream())
        PR.finish(self.st, hp, self.cur)
        return self.cur

    def inject_sums(self, dot, l1):
        """What the moments sweeps would have left: the two sums, written into the device block and the mirror."""
        self.S.t.view(-1)[5:7] = torch.tensor([dot, l1], dtype=F64)
        self.st["dot"], self.st["l1"] = float(dot), float(l1)

    def check(self, tag):
        torch.cuda.synchronize()
        assert_equal_bits(self.CUR.t.view(-1).cpu(), torch.from_numpy(self.cur), f"{tag}: scalar block")
        assert_equal_bits(self.S.t.view(-1).cpu(), torch.from_numpy(PR.state_block(self.st)), f"{tag}: state block")
        assert int(self.T.t.view(torch.int64).item()) == self.st["t"], f"{tag}: counter {int(self.T.t.view(torch.int64).item())}"
        for what, gd in (("counter", self.T), ("state block", self.S), ("scalar block", self.CUR)):
            gd.check(f"{tag}: {what}")


# ------------------------------------------------------------------------------------------------ select and finish
def _sums_for(k, rs, st, hp):
    """Step k's (dot, l1): k = 0 a d_hat below d0 (the d == d0 branch that keeps d), k = 1 l1 == 0, k = 2 a d_hat above d0 (the branch that
    takes it), then sums whose d_hat is the current d times a factor around one (q dot = factor x l1 x d x (1 - beta3), and now and then
    a negative dot), so that d climbs without leaving the doubles' range in forty steps."""
    if k == 0:
        return 0.0, 1.0
    if k == 1:
        return 5.0, 0.0
    l1 = float(abs(rs.standard_normal()) + 0.1)
    if k == 2 or st["q"] == 0.0:
        return 3.0 * hp["d0"] * l1 / (st["q"] if st["q"] else 1.0), l1
    return float(rs.standard_normal() + 1.2) * l1 * st["d"] * (1.0 - hp["beta3"]) / st["q"], l1


@pytest.mark.parametrize("flags", [False, True], ids=["plain", "bias_correction+safeguard+growth"])
def test_select_and_finish_forty_launches_equal_the_host_mirror(dev, flags):
    """Forty select / finish pairs from t = 0 with the sums of each step written in between: scalar block, all ten doubles of the state
    block and the counter equal the host mirror in every bit after every launch - through d == d0 with d_hat below and above it, l1 == 0,
    a growth rate of 1.05 that binds (flags on), by value and from tables whose first entry is lr_t = 0 and whose ends are passed."""
    kw = dict(use_bias_correction=True, safeguard_warmup=True, growth_rate=1.05, d_coef=0.8, d0=1e-5) if flags else {}
    hp = PR.hyper(**kw)
    lr_tab = torch.tensor(L.LRSchedule("cosine", hp["lr"], num_warmup_steps=3, num_training_steps=9).table())
    ema_tab = torch.tensor(L.EMASchedule("warmup", 0.999).table().reshape(-1)[:14])
    assert float(lr_tab[0]) == 0.0 and 3 < lr_tab.numel() < 20
    LR, EMT = _flat_in(lr_tab, F32, dev), _flat_in(ema_tab, F32, dev)
    for tabs in (None, (LR, EMT)):
        blk, rs, bound, moved = _Blocks(dev, hp), np.random.RandomState(3), 0, 0
        for k in range(40):
            before = blk.st["d"]
            cur = blk.select(0.9999) if tabs is None else blk.select(LR=LR, EMT=EMT)
            blk.check(f"select {k}")
            assert cur[3] == (1 if k == 0 else 0) and cur[7] == 0
            blk.inject_sums(*_sums_for(k, rs, blk.st, hp))
            blk.finish()
            blk.check(f"finish {k}")
            d = blk.st["d"]
            assert d >= before
            if tabs is not None and k == 0:
                assert blk.st["lr_t"] == 0.0 and cur[0] == 0 and d == hp["d0"] == blk.st["d_max"], "lr_t == 0 leaves d alone"
            if k == 1:
                assert d == before, "l1 == 0 leaves d alone"
            bound += int(d == before * hp["growth_rate"] and d < blk.st["d_max"])
            moved += int(d > before)
        assert blk.st["d"] > hp["d0"] and moved >= 2
        assert (bound > 0) == flags, "the finite growth rate never bound"
    LR.check("lr table"); EMT.check("ema table")


def test_select_and_finish_from_a_restored_count(dev):
    """ParamStore.set_step(10^5) rebuilds the products with 10^5 float64 multiplications; select / finish launches from there against the
    mirror in every bit (b1's product has gone denormal: the bias correction is sqrt(1 - P2) / 1)."""
    st = _store(dev, prodigy=dict(use_bias_correction=True))
    hp = PR.hyper(**{k: v for k, v in st.prodigy.items()})
    for t0 in (1000, 10 ** 5):
        st.set_step(t0)
        assert int(st.prodigy_step.item()) == t0
        prods = PR.products(t0, hp["b1"], hp["b2"])
        assert tuple(st.prodigy_state[3:5].tolist()) == prods and 0 < prods[0] < (1e-300 if t0 > 1000 else 1e-40)
        blk = _Blocks(dev, hp, t0)
        assert_equal_bits(blk.S.t.view(-1).cpu(), st.prodigy_state.cpu(), "the store's block after set_step against the mirror's")
        rs = np.random.RandomState(t0 % 89)
        for k in range(3):
            cur = blk.select(0.999)
            blk.check(f"select at {t0} + {k}")
            assert cur[3] == 0
            blk.inject_sums(*_sums_for(k + 2, rs, blk.st, hp))
            blk.finish()
            blk.check(f"finish at {t0} + {k}")
        assert blk.st["d"] > hp["d0"]


# ------------------------------------------------------------------------------------------------ the two sums
def _moments_call(P, G, g16, P0, M, V, S, n, SQ, max_norm, blk, ws):
    from stable_diffusion_training_amd import _lib
    hp = blk.hp
    _lib.call("sdt_prodigy_moments_step", P.ptr, G.ptr, g16, P0.ptr, M.ptr, V.ptr, S.ptr, n, None if SQ is None else SQ.ptr, float(max_norm),
              blk.CUR.ptr, blk.S.ptr, hp["b1"], hp["b2"], hp["beta3"], ws.data_ptr(), ws.numel(), _stream())


@pytest.mark.parametrize("g16", [0, 1], ids=["fp32", "bf16"])
def test_the_two_sums_are_exact_on_integers(dev, g16):
    """Integer-valued gc (-3..3), p0 - p (-3..3) and s' (= gc: c_s = 1 on s = 0): every product, partial and total is an integer far below
    2^53, so dot and l1 must equal the integer answers in every bit - at n = 1, 3, 1023, 1024, 1025, 8191 x 4 + 2 and 2^20 + 5, on top of
    what the block held, and over two launches that accumulate into one pair of sums.  The arrival counters are zero afterwards."""
    from stable_diffusion_training_amd import _lib
    hp = PR.hyper()
    ws = _workspace(_lib.load().sdt_prodigy_workspace_bytes(), dev)
    ws[kc.CNT_BYTES:].fill_(0xFF)  # the partials need no initialisation
    R = kc.SQNORM_RANGE
    for n in SIZES:
        blk = _Blocks(dev, hp, t0=5)
        blk.cur = np.array([-1e-3, 0, 1, 0, 1, 1, 1, 0], np.float32)  # first = 0, c_m = c_v = c_s = 1
        blk.CUR.t.view(-1).copy_(torch.from_numpy(blk.cur))
        blk.inject_sums(7.0, 11.0)
        want_dot, want_l1 = 7.0, 11.0
        for launch in range(2):
            m_ = n if launch == 0 else max(n // 3, 1)
            g = kc.exact_ints((m_,), -R, R, 10 * n + launch, dtype=F32).reshape(-1)
            p0 = kc.exact_ints((m_,), -R, R, 10 * n + launch + 2, dtype=F32).reshape(-1)
            p = kc.exact_ints((m_,), -R, R, 10 * n + launch + 4, dtype=F32).reshape(-1)
            dx = (p0 - p).double()
            want_dot += float((g.double() * dx).sum())
            want_l1 += float(g.double().abs().sum())
            P, G, P0 = _flat_in(p, F32, dev), _flat_in(g, BF if g16 else F32, dev), _flat_io(p0, F32, dev)
            M, V, S = (_flat_io(torch.zeros(m_), F32, dev) for _ in range(3))
            _moments_call(P, G, g16, P0, M, V, S, m_, None, 1.0, blk, ws)
            torch.cuda.synchronize()
            tag = f"sums n {n} launch {launch}"
            got = blk.S.t.view(-1).cpu()
            terms = g.double() * dx
            msg = kc.sum_report(got[5], want_dot, f"{tag}: dot", parts=kc.sqnorm_parts(terms, m_), tail=terms[(m_ >> 2) << 2:])
            assert msg is None, msg
            msg = kc.sum_report(got[6], want_l1, f"{tag}: l1", parts=kc.sqnorm_parts(g.double().abs(), m_), tail=g.double().abs()[(m_ >> 2) << 2:])
            assert msg is None, msg
            assert_equal_bits(S.t.view(-1).cpu(), g, f"{tag}: s' = gc")
            assert_equal_bits(M.t.view(-1).cpu(), g, f"{tag}: m' = gc")
            assert_equal_bits(V.t.view(-1).cpu(), g * g, f"{tag}: v' = gc gc")
            assert_equal_bits(P0.t.view(-1).cpu(), p0, f"{tag}: p0 is kept after the first step")
            for what, gd in (("p", P), ("g", G), ("p0", P0), ("m", M), ("v", V), ("s", S), ("state", blk.S), ("cur", blk.CUR)):
                gd.check(f"{tag}: {what}")
            msg = kc.counters_report(ws, tag)
            assert msg is None, msg
        assert want_dot < 2 ** 53 and want_l1 < 2 ** 53


# ------------------------------------------------------------------------------------------------ the sweeps
def _gradient(n, g16, clip, seed, step, special):
    base, rs = np.random.RandomState(seed).standard_normal(n), np.random.RandomState(seed * 7 + step)
    g = ((base + 0.3 * rs.standard_normal(n)) * (3.0 if clip else 0.05)).astype(np.float32)  # a direction that persists: d can grow
    if special == "zero":
        g[:] = 0.0
    elif special == "mixed" and n >= 1023:
        g[: n // 4] = 0.0                      # from zero moments: v' = 0 and m' = 0, the quotient is 0 / d_eps
        g[n // 2] = 1e19 if step % 2 == 0 else -1e19
        g[n // 2 + 1: n // 2 + 3] = [1e-30, -1e-30]  # gc gc underflows to 0 while c_m gc does not: d_eps is the whole denominator
    if g16:
        g = torch.from_numpy(g).to(BF).float().numpy()
    return g


def _sweeps_run(dev, n, g16, clip, wd, use_ema, hp, seed, ws, special=None):
    """Three carried steps of select, moments, finish, apply on one piece against three steps of the restatement; every buffer between
    guards."""
    from stable_diffusion_training_amd import _lib
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    first_p = p.copy()
    buf = PR.zeros(n)
    buf["p0"] = np.full(n, 123.0, np.float32)  # whatever the buffer held: the first step overwrites it
    if use_ema:
        buf["ema"] = p.copy()
    P, P0 = _flat_io(torch.from_numpy(p), F32, dev), _flat_io(torch.from_numpy(buf["p0"]), F32, dev)
    M, V, S = (_flat_io(torch.zeros(n), F32, dev) for _ in range(3))
    EM = _flat_io(torch.from_numpy(buf["ema"]), F32, dev) if use_ema else None
    W16 = _flat_out(n, BF, dev)
    blk = _Blocks(dev, hp)
    tag0 = f"prodigy n {n} g16 {g16} clip {clip} wd {wd} ema {use_ema} special {special}"
    for step in range(3):
        g = _gradient(n, g16, clip, seed, step, special)
        max_norm = 1.0
        sq = float(np.sum(np.asarray(g, np.float64) ** 2))
        G = _flat_in(torch.from_numpy(g), BF if g16 else F32, dev)
        SQ = _flat_io(torch.tensor([sq], dtype=F64), F64, dev) if clip else None
        cur = blk.select(0.999)
        _moments_call(P, G, g16, P0, M, V, S, n, SQ, max_norm, blk, ws)
        buf["p0"], buf["m"], buf["v"], buf["s"] = PR.moments(p, g, buf["p0"], buf["m"], buf["v"], buf["s"], cur, hp, blk.st,
                                                               max_norm=max_norm if clip else None)
        blk.finish()
        _lib.call("sdt_prodigy_apply_step", P.ptr, M.ptr, V.ptr, None if EM is None else EM.ptr, W16.ptr, n, blk.CUR.ptr, wd, _stream())
        p = PR.apply(p, buf["m"], buf["v"], cur, wd)
        if use_ema:
            buf["ema"] = PR.ema_update(buf["ema"], p, cur)
        tag = f"{tag0} step {step}"
        blk.check(tag)
        assert np.array_equal(buf["p0"], first_p), "the restatement's p0 is the parameters of the first step"
        for name, gd, want in (("p0", P0, buf["p0"]), ("m", M, buf["m"]), ("v", V, buf["v"]), ("s", S, buf["s"]), ("masters", P, p)):
            assert_equal_bits(gd.t.view(-1).cpu(), torch.from_numpy(want), f"{tag}: {name}")
        if EM is not None:
            assert_equal_bits(EM.t.view(-1).cpu(), torch.from_numpy(buf["ema"]), f"{tag}: ema")
        assert_equal_bits(W16.t.view(-1).cpu(), torch.from_numpy(p).to(BF), f"{tag}: w_bf16 against bf16(p)")
        for what, gd in (("p", P), ("p0", P0), ("m", M), ("v", V), ("s", S), ("ema", EM), ("w_bf16", W16), ("g", G), ("sqnorm", SQ)):
            if gd is not None:
                gd.check(f"{tag}: {what}")
        msg = kc.counters_report(ws, tag)
        assert msg is None, msg
        if special == "zero":
            assert not buf["m"].any() and not buf["v"].any() and blk.st["l1"] == 0 and blk.st["d"] == hp["d0"]
            assert np.array_equal(p, first_p) or wd != 0
        if special == "mixed" and n >= 1023 and step == 0:
            k = n // 2 + 1
            assert buf["v"][k] == 0 and (buf["m"][k] != 0 or clip) and not buf["v"][: n // 4].any() and np.isfinite(p).all()
    return blk


@pytest.mark.parametrize("g16", [0, 1], ids=["fp32", "bf16"])
def test_sweeps_equal_the_restatement_in_every_bit(dev, g16):
    """Both sweeps with the one-lane kernels between them at every size, three carried steps each: m, v, s, p0, p, ema, w_bf16, the state
    block (d, d_max, numer, both sums) and the scalar block equal the restatement in every bit; with and without the clip, the decay and
    the EMA, default settings and bias correction + safeguard.  The first step captures p0 (over whatever the buffer held), the later
    ones leave it."""
    from stable_diffusion_training_amd import _lib
    ws = _workspace(_lib.load().sdt_prodigy_workspace_bytes(), dev)
    plain, flagged = PR.hyper(d0=1e-3), PR.hyper(d0=1e-4, use_bias_correction=True, safeguard_warmup=True, growth_rate=1.5)
    k, moved = 0, 0
    for n in SIZES:
        combos = [(c, w, e) for c in (0, 1) for w in (0.0, 0.07) for e in (0, 1)]
        if n > (1 << 20):
            combos = [(1, 0.07, 1), (0, 0.0, 0)]
        for clip, wd, e in combos:
            blk = _sweeps_run(dev, n, g16, clip, wd, e, flagged if k % 3 == 2 else plain, seed=n % 97 + k, ws=ws)
            k += 1
            moved += int(blk.st["d"] > blk.hp["d0"])
    assert moved >= 4, "d left d0 in too few of the runs for the d != d0 branch of the finish kernel to have been compared"


@pytest.mark.parametrize("g16", [0, 1], ids=["fp32", "bf16"])
def test_sweeps_special_values(dev, g16):
    """An all-zero gradient (nothing moves but by the decay, d stays d0), and a quarter of zeros beside one element at +-1e19 and two at
    +-1e-30, whose v' is 0 while their m' is not: d_eps is the whole denominator."""
    from stable_diffusion_training_amd import _lib
    ws = _workspace(_lib.load().sdt_prodigy_workspace_bytes(), dev)
    hp = PR.hyper(d0=1e-3)
    for n in (1025, 8191 * 4 + 2):
        for clip, wd in ((0, 0.0), (0, 0.07), (1, 0.07)):
            _sweeps_run(dev, n, g16, clip, wd, 1, hp, seed=900 + n % 13, ws=ws, special="zero")
            _sweeps_run(dev, n, g16, clip, wd, 1, hp, seed=901 + n % 13, ws=ws, special="mixed")


# ------------------------------------------------------------------------------------------------ ParamStore.optimizer_step
SPEC = [("a/kernel", (64, 48)), ("b/kernel", (3, 3, 16, 16)), ("e/embedding", (10, 8)), ("a/bias", (48,))]  # tests/test_gpu_adamw.py's
STEP_HP = dict(lr=1.0, wd=0.07, eps=1e-8, max_norm=1.0)
STATE = ("master", "w", "mom", "mom2", "prodigy_s", "prodigy_p0", "ema", "prodigy_step", "prodigy_state", "prodigy_cur")


def _store(dev, **kw):
    """A leaf in each of the four (quantised x decayed) segments."""
    from stable_diffusion_training_amd import params
    st = params.ParamStore(SPEC, device=dev, quantise=True, quant_excluded=("bias", "embedding"), wd_excluded=("b", "bias"), block_size=16,
                           with_ema=True, optimizer="prodigy", **kw)
    assert [(q, d, b > a) for q, d, a, b in st.segments] == [(True, True, True), (True, False, True), (False, True, True), (False, False, True)]
    g = torch.Generator().manual_seed(11)
    st.load({p: torch.randn(shp, generator=g) * 0.1 for p, shp in SPEC})
    return st


@pytest.mark.parametrize("mode", ["grad", "acc", "scheduled"])
def test_store_step_equals_the_restatement_leaf_by_leaf(dev, mode):
    """Two optimizer steps of a Prodigy store with a leaf in each of the four segments against the restatement run launch by
    launch (the sums accumulate over the moments launches, one per gradient buffer; the apply sweep runs once per segment: the decay alternates): from the gradient buffers (bf16 for the kernels), from the
    accumulated gradient, and with a schedule installed - every leaf of masters, EMA, mirror, m, v, s, p0, and the state block with d."""
    st = _store(dev, prodigy=dict(d0=1e-4))
    hp = PR.hyper(**st.prodigy)
    host = lambda t: t.detach().cpu().numpy().copy()
    p, ema = host(st.master), host(st.ema)
    buf = PR.zeros(st.total)
    ref_st = PR.init_state(hp)
    lrs, emas = L.LRSchedule("cosine", STEP_HP["lr"], num_warmup_steps=1, num_training_steps=4), L.EMASchedule("warmup", 0.999)
    if mode == "scheduled":
        st.set_schedule(lr=lrs, ema=emas)
    ds = []
    for step in range(3 if mode == "scheduled" else 2):
        flat = torch.zeros(st.total)
        gen = torch.Generator().manual_seed(50 + step)
        for path, lf in st.leaves.items():  # the gaps between leaves stay zero, as zero_grad leaves them
            base = torch.randn(lf.numel, generator=torch.Generator().manual_seed(7 + lf.offset))  # a direction that persists
            flat[lf.offset: lf.offset + lf.numel] = (base + 0.2 * torch.randn(lf.numel, generator=gen)) * (0.5 if step else 1e-3)
        st.set_grad_flat(flat)
        if mode == "acc":
            st.accumulate("init")
            st.accumulate("scale", scale=0.5, norm=True)
            g_seen = (st.grad_flat().cpu().numpy() * np.float32(0.5)).astype(np.float32)
        else:
            g_seen = st.grad_flat().cpu().numpy()
        assert st.grad16 is not None
        st.optimizer_step(ema_rate=0.999, grad_source="acc" if mode == "acc" else "grad", **STEP_HP)
        kw = dict(lr_tab=lrs.table(), ema_tab=emas.table()) if mode == "scheduled" else {}
        cur = PR.select(ref_st, hp, ema_rate=0.999, **kw)
        sq = float(np.sum(g_seen.astype(np.float64) ** 2))
        pieces = [(a, b, d) for (q, d, a, b) in st.segments if b > a]
        # the moments sweep runs once per gradient buffer: the bf16 kernels' and the fp32 rest, or the one accumulated buffer
        for a, b in ([(0, st.total)] if mode == "acc" else [(0, st.quant_total), (st.quant_total, st.total)]):
            sl = slice(a, b)
            buf["p0"][sl], buf["m"][sl], buf["v"][sl], buf["s"][sl] = PR.moments(p[sl], g_seen[sl], buf["p0"][sl], buf["m"][sl], buf["v"][sl],
                                                                                buf["s"][sl], cur, hp, ref_st, max_norm=1.0, sq=sq)
        PR.finish(ref_st, hp, cur)
        for a, b, decayed in pieces:
            sl = slice(a, b)
            p[sl] = PR.apply(p[sl], buf["m"][sl], buf["v"][sl], cur, STEP_HP["wd"] if decayed else 0.0)
        ema = PR.ema_update(ema, p, cur)
        torch.cuda.synchronize()
        tag = f"{mode} step {step}"
        assert_equal_bits(st.prodigy_cur.cpu(), torch.from_numpy(cur), f"{tag}: scalar block")
        assert_equal_bits(st.prodigy_state.cpu(), torch.from_numpy(PR.state_block(ref_st)), f"{tag}: state block (d, d_max, numer, sums)")
        assert int(st.prodigy_step.item()) == st.count == step + 1 and float(st.prodigy_d().item()) == ref_st["d"]
        flats = dict(master=p, ema=ema, mom=buf["m"], mom2=buf["v"], prodigy_s=buf["s"], prodigy_p0=buf["p0"])
        for path, lf in st.leaves.items():
            sl = slice(lf.offset, lf.offset + lf.numel)
            for name, want in flats.items():
                assert_equal_bits(getattr(st, name)[sl].cpu(), torch.from_numpy(want[sl]), f"{tag}: {path} {name}")
            assert_equal_bits(st.w[sl].cpu(), torch.from_numpy(p[sl]).to(BF), f"{tag}: {path} bf16 mirror")
        ex = st.export_prodigy_state()
        assert ex[""]["d"] == ref_st["d"] and ex[""]["step"] == step + 1 and torch.equal(ex["a/bias"]["s"].cpu(), torch.from_numpy(buf["s"][st.leaves["a/bias"].offset:][:48]))
        msg = kc.counters_report(st.sq_ws, tag)
        assert msg is None, msg
        ds.append(ref_st["d"])
    if mode == "scheduled":  # the warm-up's first step has lr_t = 0: nothing moves in p, d stays
        assert ds[0] == hp["d0"]
    assert ds[-1] > hp["d0"], ds
    with pytest.raises(ValueError, match="sharded optimizer is not available for a Prodigy store"):
        st.optimizer_step(shard=([(0, 2048, True, True)], True), **STEP_HP)


# ------------------------------------------------------------------------------------------------ train step
RANK, ALPHA = 4, 4.0
EMA_RATE = 0.999
OPT = dict(name="prodigy", weight_decay=1e-2, d0=1e-5)


def _config(case, ema=True):
    from stable_diffusion_training_amd import training_utils as tu
    return tu.TrainingConfig(
        model_path="synthetic", batch_size=case["batch"]["pixel_values"].shape[0], learning_rate=1e-6, unet_learning_rate=1e-6,
        text_encoder_learning_rate=1e-6, lr_scheduler="constant", adam_to_lion_scale_factor=7.0, compilation_cache_path="",
        keep_compiled_fn_in_cache=False, text_encoder_context_window=77, context_window_concatenation_count=1,
        aot_compile=True, strip_bos_eos_token=False, offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0,
        perturbation_noise_magnitude=0.0, image_area_root=[512], minimum_axis_length=[512], beta_scheduler=case["sched"],
        prediction_type="epsilon", excluded_layer_pattern_from_weight_decay=["bias", "scale", "embedding"],
        excluded_layer_from_quantization=["bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj"],
        quant_block_size=16, quantize_unet_state=True, quantize_text_encoder_state=True,
        accumulate_unet_ema=ema, accumulate_text_encoder_ema=ema, ema_rate=EMA_RATE)


def _states(case, dev, adapter):
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
    tc = _config(case)
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    cfg = None
    if adapter != "none":
        dora = adapter == "dora"
        cfg = dict(unet=lora.LoraConfig(RANK, ALPHA, seed=1, dora=dora),
                   text_encoder=lora.LoraConfig(RANK, ALPHA, targets=lora.CLIP_TARGETS, seed=2, dora=dora))
    states = tu.on_device_model_training_state(tc, models, device=dev, optimizer=OPT, lora=cfg)
    for s in states[:2]:
        assert s.opt_store.optimizer == "prodigy" and s.hyper == dict(lr=1.0, wd=1e-2, eps=1e-8, max_norm=1.0)
        assert (s.adapter is not None) == (adapter != "none")
    return tc, states


def _inputs(case, dev, step):
    """Step `step`'s batch and draws: the pixels move with the step, the noise and the timesteps are the same draws every step - gradients
    that keep their direction are what lets d leave d0 within five steps (with fresh noise every step the text tower's d_hat stayed below
    d0 for all five)."""
    g = torch.Generator().manual_seed(100)
    batch = to_dev(case["batch"], dev)
    batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
    rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
            for k, v in case["rand"].items()}
    return batch, rand


def _snap(us, ts):
    torch.cuda.synchronize()
    out = {f"{name}.{b}": getattr(st.opt_store, b).clone() for name, st in (("unet", us), ("text", ts)) for b in STATE}
    for name, st in (("unet", us), ("text", ts)):
        if st.adapter is not None:
            out[f"{name}.merged_mirror"] = st.store.w.clone()
    out["counts"] = torch.tensor([us.opt_store.count, ts.opt_store.count])
    return out


def _eager(case, dev, steps, us, ts, ue, te, vae, sc, first=0):
    from stable_diffusion_training_amd import training_utils as tu
    trace = []
    for t in range(first, first + steps):
        batch, rand = _inputs(case, dev, t)
        out = tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=EMA_RATE, rand=rand)
        snap = _snap(us, ts)
        snap["loss"] = out[4]["loss"].clone()
        trace.append(snap)
    return trace


@pytest.mark.parametrize("adapter", ["none", "lora", "dora"])
def test_train_step_eager_captured_and_resumed_are_bit_identical(dev, tmp_path, adapter):
    """The tiny UNet / text tower with optimizer="prodigy" (full fine-tune, LoRA rank 4, DoRA rank 4): five eager steps against the
    graphed shape table (its last three calls replay the captured step) - masters, m, v, s, p0, EMA, mirror, counter, state block with d
    and scalar block bit-identical after every step, losses too; then save after step 2, load into fresh states and run step 3:
    identical to the uninterrupted run.  d has left d0 in both stores by step 5."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, adapter)
    eager = _eager(case, dev, 5, us, ts, ue, te, vae, sc)
    assert all(bool(torch.isfinite(e["loss"]).all()) for e in eager)
    assert not torch.equal(eager[4]["unet.master"], eager[0]["unet.master"])
    for name in ("unet", "text"):
        d = [float(e[f"{name}.prodigy_state"][0]) for e in eager]
        print(f"{adapter} {name}: d after each step {d}, losses {[float(e['loss']) for e in eager]}")
        assert d[-1] > OPT["d0"] and all(b >= a for a, b in zip(d, d[1:])), (name, d)
        assert torch.equal(eager[4][f"{name}.prodigy_p0"], eager[0][f"{name}.prodigy_p0"]), "p0 moved after the first step"
    assert eager[4]["unet.prodigy_step"].item() == 5 and eager[4]["counts"].tolist() == [5, 5]
    del us, ts, ue, te, vae
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, adapter)
    tc = dataclasses.replace(tc, ema_rate=EMA_RATE)
    table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True, per_device_batch=2)
    fn = table[[k for k in table if k[2] == 512 and k[3] == 512][0]]
    gen = torch.Generator(device=dev)
    for t in range(5):
        batch, rand = _inputs(case, dev, t)
        out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
        snap = _snap(us, ts)
        snap["loss"] = out[4]["loss"].clone()
        for k in snap:
            _same(snap[k], eager[t][k], f"{adapter} step {t}: {k}, graphed table against eager")
    assert fn.graph is not None and fn.calls == 2, "the last three calls were to replay the captured step"
    assert us.opt_store._captured
    del us, ts, ue, te, vae, table, fn
    # resume
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, adapter)
    _eager(case, dev, 2, us, ts, ue, te, vae, sc)
    path = str(tmp_path / "prodigy_state.safetensors")
    tu.save_training_state(path, us, ts)
    del us, ts, ue, te, vae
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, adapter)
    assert int(us.opt_store.prodigy_step.item()) == 0
    tu.load_training_state(path, us, ts)
    assert us.step == 2 and int(us.opt_store.prodigy_step.item()) == 2 and int(ts.opt_store.prodigy_step.item()) == 2
    assert_equal_bits(us.opt_store.prodigy_state, eager[1]["unet.prodigy_state"], "the loaded state block (products rebuilt on the host)")
    resumed = _eager(case, dev, 1, us, ts, ue, te, vae, sc, first=2)[0]
    for k in resumed:
        _same(resumed[k], eager[2][k], f"{adapter} {k}: step 3 after save / load against the uninterrupted run")


# ------------------------------------------------------------------------------------------------ two ranks
def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from stable_diffusion_training_amd import dp
        from stable_diffusion_training_amd import training_utils as tu
        torch.cuda.set_device(0)
        dev = torch.device("cuda:0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        case = make_case("tiny", B=2, image=64)
        tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, "none")
        refusal = ""
        try:
            dp.GradReducer([us.store, ts.store], bucket_bytes=1 << 16, shard=True)
        except ValueError as e:
            refusal = str(e)
        assert not us.store.sharded and not ts.store.sharded
        red = dp.GradReducer([us.store, ts.store], bucket_bytes=1 << 16)
        assert len(red.buckets) > 4 and not red.shard
        losses = []
        for step in range(3):
            batch, rand = _inputs(case, dev, step)
            sl = slice(rank, rank + 1)
            out = tu.train_step(us, ts, ue, te, {k: v[sl] for k, v in batch.items()}, torch.Generator(device=dev), vae, sc,
                                strip_bos_eos_token=False, ema_rate=EMA_RATE, rand={k: v[sl] for k, v in rand.items()}, reducer=red)
            losses.append(float(out[4]["loss"].item()))
        torch.cuda.synchronize()
        res = dict(refusal=refusal, losses=losses)
        for name, st in (("unet", us.store), ("text", ts.store)):
            res[name] = st.master.detach().cpu().numpy().copy()  # by value: see tests/test_gpu_dp.py
            res[name + ".state"] = st.prodigy_state.detach().cpu().numpy().copy()
        q.put((rank, "ok", res))
        dist.barrier()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc()[-1500:], None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_one_gpu_end_with_equal_masters_and_the_same_d():
    """Two ranks on one GPU through gloo, all-reduce exchange, three steps on different halves of the batch: both ranks see the reduced
    gradient, so their masters are torch.equal and their state blocks - d, d_max, numer, both sums - identical in every bit; d has
    left d0.  The reduce-scatter mode raises the documented ValueError (and leaves the stores unsharded)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 36500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    a, b = res[0][2], res[1][2]
    for name in ("unet", "text"):
        assert torch.equal(torch.from_numpy(a[name]), torch.from_numpy(b[name])), f"{name}: ranks diverged"
        assert_equal_bits(torch.from_numpy(a[name + ".state"]), torch.from_numpy(b[name + ".state"]), f"{name}: state blocks of the two ranks")
        assert a[name + ".state"][0] > OPT["d0"], "d never left d0"
    assert all(abs(x - y) < 1e-6 for x, y in zip(a["losses"], b["losses"]))  # the reduced (mean) loss
    for r in (a, b):
        assert "GradReducer(shard=True): the sharded optimizer is not available for a Prodigy store" in r["refusal"]
