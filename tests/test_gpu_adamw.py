"""AdamW with 8-bit block-quantised moments on a real MI355X: sdt_adamw_select, sdt_adamw8_step and sdt_adamw32_step against the NumPy
float32 restatement (tests/adamw_reference.py) in every bit, ParamStore.optimizer_step for an AdamW store (whole, accumulated, scheduled,
sliced for eight virtual ranks), the train step eager / captured / resumed, and a Lion sweep beside it.  Outputs and in-place operands sit
between sentinel guards, inputs between NaN guards (tests/kernel_checks.py)."""
import dataclasses

import numpy as np
import pytest
import torch

from stable_diffusion_training_amd import lr_schedule as L
from tests import adamw_reference as AR
from tests import kernel_checks as kc
from tests.helpers import make_case, to_dev
from tests.kernel_checks import BF, assert_equal_bits
from tests.step_matrix import STEP_HP, _check_store, _reference_store_step  # (shared with tests/test_gpu_step_combinations.py)
from tests.test_gpu_kernel_exact import _stream, _workspace
from tests.test_gpu_reduce_optim_exact import _flat_in, _flat_io, _flat_out, _lion8_run, _lion_inputs, _np, _thresholds, _ws_args

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
HP = AR.HP


def _same(a, b, what):
    """Bitwise equality with kernel_checks' report where it has an integer view for the type (the int64 counters: torch.equal)."""
    if a.dtype in kc._INT_VIEW:
        assert_equal_bits(a, b, what)
    else:
        assert torch.equal(a, b), f"{what}: {a.tolist()} != {b.tolist()}"


class _Select:
    """The device side of sdt_adamw_select between guards (counter, products, scalar block) and its host mirror."""

    def __init__(self, dev, t0=0, prods=(1.0, 1.0), b1=HP["b1"], b2=HP["b2"]):
        self.ST = _flat_io(torch.tensor([t0], dtype=torch.int64).view(F64), F64, dev)
        self.PR = _flat_io(torch.tensor(prods, dtype=F64), F64, dev)
        self.CUR = _flat_out(8, F32, dev)
        self.t, self.prods, self.b1, self.b2 = t0, tuple(prods), b1, b2

    def launch(self, lr=HP["lr"], ema_rate=HP["ema_rate"], LR=None, EMT=None):
        """One launch; returns the host's scalar block after asserting the device's equals it in every bit."""
        from stable_diffusion_training_amd import _lib
        tabs = (None, 0, None, 0) if LR is None else (LR.ptr, LR.width, EMT.ptr, EMT.width // 2)
        _lib.call("sdt_adamw_select", self.ST.ptr, self.PR.ptr, *tabs, lr, ema_rate, self.b1, self.b2, self.CUR.ptr, _stream())
        torch.cuda.synchronize()
        kw = dict(lr=lr, ema_rate=ema_rate) if LR is None else dict(lr_tab=_np(LR), ema_tab=_np(EMT).reshape(-1, 2))
        t_before = self.t
        cur, self.t, self.prods = AR.select_scalars(self.t, self.prods, self.b1, self.b2, **kw)
        tag = f"select at t = {t_before}"
        assert_equal_bits(self.CUR.t.view(-1).cpu(), torch.from_numpy(cur), f"{tag}: scalar block")
        assert int(self.ST.t.view(torch.int64).item()) == self.t, f"{tag}: counter {int(self.ST.t.view(torch.int64).item())}"
        assert_equal_bits(self.PR.t.view(-1).cpu(), torch.tensor(self.prods, dtype=F64), f"{tag}: running products")
        for what, gd in (("counter", self.ST), ("products", self.PR), ("scalar block", self.CUR)):
            gd.check(f"{tag}: {what}")
        return cur


def _special_gradients(g, bs, g16, step):
    """Block 0 all zero (from the initial state: stays code 0 / scale 1); block 1 one element at +-1e19 (its square is finite); block 2
    float32 denormals beside normal values."""
    g = g.copy()
    g[:bs] = 0.0
    g[bs + (step % bs)] = 1e19 if step % 2 == 0 else -1e19
    g[2 * bs: 2 * bs + 2] = [1e-40, -3e-39]
    if g16:
        g = torch.from_numpy(g).to(BF).float().numpy()
    return g


def _adamw8_run(dev, n, bs, g16, use_ema, use_w16, regime, wd, seed, special=False):
    """Three carried sdt_adamw_select + sdt_adamw8_step pairs (t = 0, 1, 2, the products carried on the device) against three steps of
    the restatement; every buffer between guards."""
    from stable_diffusion_training_amd import _lib
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n).astype(np.float32)
    state = AR.init_state8(n, bs)
    ema = p.copy() if use_ema else None
    P = _flat_io(torch.from_numpy(p), F32, dev)
    MC, MI, SC, SI = (_flat_io(torch.from_numpy(a.reshape(-1)), torch.int8 if a.dtype == np.int8 else F32, dev) for a in state)
    EM = _flat_io(torch.from_numpy(ema), F32, dev) if use_ema else None
    W16 = _flat_out(n, BF, dev) if use_w16 else None
    thr = _thresholds(dev)
    sel = _Select(dev)
    hp = dict(bs=bs, wd=wd, b1=HP["b1"], b2=HP["b2"], eps=HP["eps"])
    tag0 = f"adamw8 n {n} bs {bs} g16 {g16} ema {use_ema} w16 {use_w16} {regime} wd {wd}"
    for step in range(3):
        g, max_norm = _lion_inputs(n, bs, g16, regime, seed, step)
        if special:
            g = _special_gradients(g, bs, g16, step)
        clip = None if regime == "none" else max_norm
        sq = float(np.sum(np.asarray(g, np.float64) ** 2))
        cur = sel.launch()
        p0 = p
        p, state = AR.step8(p, g, state, cur, max_norm=clip, **hp)
        if use_ema:
            ema = AR.ema_update(ema, p, cur)
        if special:  # the all-zero block: code 0, scale 1, moved by the decay alone
            assert not state[0][0].any() and not state[2][0].any() and state[1][0] == 1 and state[3][0] == 1
            dec = p0[:bs] if wd == 0 else (p0[:bs] + (cur[0] * (np.float32(wd) * p0[:bs]).astype(np.float32)).astype(np.float32)).astype(np.float32)
            assert np.array_equal(p[:bs], dec)
        G = _flat_in(torch.from_numpy(g), BF if g16 else F32, dev)
        SQ = None
        if clip is not None:
            SQ = _flat_io(torch.tensor([0.0 if regime == "equal" else sq], dtype=F64), F64, dev)
            if regime == "equal":  # the device's own norm of these gradients: exact, so it equals max_norm^2
                ws = _workspace(_lib.load().sdt_sqnorm_workspace_bytes(), dev)
                _lib.call("sdt_sqnorm_accumulate_bf16" if g16 else "sdt_sqnorm_accumulate", G.ptr, n, SQ.ptr, *_ws_args(ws), _stream())
                torch.cuda.synchronize()
                assert SQ.t.item() == max_norm ** 2 == sq, f"{tag0}: the constructed norm is not exact"
        _lib.call("sdt_adamw8_step", P.ptr, G.ptr, g16, MC.ptr, MI.ptr, SC.ptr, SI.ptr, None if EM is None else EM.ptr,
                  None if W16 is None else W16.ptr, n, bs, None if SQ is None else SQ.ptr, thr.data_ptr(), float(max_norm), sel.CUR.ptr,
                  wd, HP["b1"], HP["b2"], HP["eps"], _stream())
        torch.cuda.synchronize()
        tag = f"{tag0} step {step}"
        for name, co, iv, wc, wi in (("m", MC, MI, state[0], state[1]), ("s", SC, SI, state[2], state[3])):
            msg = kc.lion_state_report(_np(co).reshape(-1, bs), _np(iv), wc, wi, f"{tag}: {name} state")
            assert msg is None, msg
        assert int(_np(SC).min()) >= 0, f"{tag}: a negative code for a root"
        assert_equal_bits(P.t.view(-1).cpu(), torch.from_numpy(p), f"{tag}: masters")
        if EM is not None:
            assert_equal_bits(EM.t.view(-1).cpu(), torch.from_numpy(ema), f"{tag}: ema")
        if W16 is not None:
            assert_equal_bits(W16.t.view(-1).cpu(), torch.from_numpy(p).to(BF), f"{tag}: w_bf16 against bf16(p)")
        for what, gd in (("p", P), ("m codes", MC), ("m inv_scale", MI), ("s codes", SC), ("s inv_scale", SI), ("ema", EM), ("w_bf16", W16),
                         ("g", G), ("sqnorm", SQ), ("scalar block", sel.CUR)):
            if gd is not None:
                gd.check(f"{tag}: {what}")


@pytest.mark.parametrize("g16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("bs", kc.LION_BLOCK_SIZES)
def test_adamw8_step_is_the_restatement_in_every_bit(dev, bs, g16):
    """Every instantiation of adamw8_kernel<LPB> (block_size 4 .. 256) x fp32 / bf16 gradients, three carried steps per case with
    sdt_adamw_select in front of each: both code streams, both scale streams, masters, EMA and w_bf16 == bf16(p) equal the restatement in
    every bit, every guard intact (each scale written once per block and nowhere else).  n: one block, 4096 -+ one block and 4096, 2^20 +
    one block.  Each of ema / w_bf16 / sqnorm present and absent, wd zero and non-zero, norms below, above and exactly at max_norm."""
    sizes = kc.lion8_sizes(bs)
    combos = [(e, w, r) for e in (0, 1) for w in (0, 1) for r in ("none", "below", "above", "equal")]
    k = 0
    for n in sizes[:-1]:
        for (e, w, r) in combos:
            _adamw8_run(dev, n, bs, g16, e, w, r, 0.07 if k % 2 else 0.0, seed=bs + n % 97 + k)
            k += 1
    for (e, w, r, wd) in ((1, 1, "above", 0.07), (0, 0, "none", 0.0), (1, 0, "equal", 0.07), (0, 1, "below", 0.0)):
        _adamw8_run(dev, sizes[-1], bs, g16, e, w, r, wd, seed=bs + 5)


@pytest.mark.parametrize("g16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("bs", kc.LION_BLOCK_SIZES)
def test_adamw8_step_special_values(dev, bs, g16):
    """An all-zero-gradient block from the initial state (stays code 0 / scale 1, p moves by the decay alone), one element at +-1e19,
    float32 denormals beside normal values - without the clip and with it, wd zero and non-zero."""
    for regime, wd in (("none", 0.07), ("none", 0.0), ("above", 0.07)):
        _adamw8_run(dev, 4096 + bs, bs, g16, 1, 1, regime, wd, seed=900 + bs, special=True)


def test_adamw32_step_is_the_restatement_in_every_bit(dev):
    """sdt_adamw32_step at n = 1, 3, 1023, 1024, 1025, 2^20 + 5 over three carried steps: m, v, p, ema, w_bf16 in every bit; ema / w_bf16
    / sqnorm present and absent, wd 0 and not, all three clip regimes; a zero gradient on zero moments moves p by the decay alone."""
    from stable_diffusion_training_amd import _lib
    k = 0
    for n in kc.LION32_SIZES:
        for (e, w, regime) in [(e, w, r) for e in (0, 1) for w in (0, 1) for r in ("none", "below", "above", "equal")]:
            if n > (1 << 20) and (e + w) == 1:
                continue
            wd = 0.07 if k % 2 else 0.0
            k += 1
            rs = np.random.RandomState(k)
            p, m, v = rs.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
            ema = p.copy() if e else None
            P, M, V = (_flat_io(torch.from_numpy(a), F32, dev) for a in (p, m, v))
            EM = _flat_io(torch.from_numpy(ema), F32, dev) if e else None
            W16 = _flat_out(n, BF, dev) if w else None
            sel = _Select(dev)
            for step in range(3):
                g, max_norm = _lion_inputs(n, 1, 0, regime, 300 + k, step)
                if regime == "equal" and n >= 3:
                    g, max_norm = kc.grads_with_exact_norm(n, 300 + k + step)
                zero_at = n // 2 if (n >= 3 and regime != "equal") else None
                if zero_at is not None:
                    g[zero_at] = 0.0
                clip = None if regime == "none" else max_norm
                sq = float(np.sum(np.asarray(g, np.float64) ** 2))
                cur = sel.launch()
                p0 = p
                p, m, v = AR.step32(p, g, m, v, cur, wd=wd, b1=HP["b1"], b2=HP["b2"], eps=HP["eps"], max_norm=clip)
                if e:
                    ema = AR.ema_update(ema, p, cur)
                if zero_at is not None:
                    assert m[zero_at] == 0 and v[zero_at] == 0
                    assert p[zero_at] == np.float32(p0[zero_at] + np.float32(cur[0] * np.float32(np.float32(wd) * p0[zero_at]))) if wd else p[zero_at] == p0[zero_at]
                G = _flat_in(torch.from_numpy(g), F32, dev)
                SQ = None if clip is None else _flat_io(torch.tensor([sq], dtype=F64), F64, dev)
                _lib.call("sdt_adamw32_step", P.ptr, G.ptr, M.ptr, V.ptr, None if EM is None else EM.ptr, None if W16 is None else W16.ptr, n,
                          None if SQ is None else SQ.ptr, float(max_norm), sel.CUR.ptr, wd, HP["b1"], HP["b2"], HP["eps"], _stream())
                torch.cuda.synchronize()
                tag = f"adamw32 n {n} ema {e} w16 {w} {regime} wd {wd} step {step}"
                assert_equal_bits(M.t.view(-1).cpu(), torch.from_numpy(m), f"{tag}: m")
                assert_equal_bits(V.t.view(-1).cpu(), torch.from_numpy(v), f"{tag}: v")
                assert_equal_bits(P.t.view(-1).cpu(), torch.from_numpy(p), f"{tag}: masters")
                if EM is not None:
                    assert_equal_bits(EM.t.view(-1).cpu(), torch.from_numpy(ema), f"{tag}: ema")
                if W16 is not None:
                    assert_equal_bits(W16.t.view(-1).cpu(), torch.from_numpy(p).to(BF), f"{tag}: w_bf16")
                for what, gd in (("p", P), ("m", M), ("v", V), ("ema", EM), ("w_bf16", W16), ("g", G), ("sqnorm", SQ)):
                    if gd is not None:
                        gd.check(f"{tag}: {what}")


# ------------------------------------------------------------------------------------------------ select
SPEC = [("a/kernel", (64, 48)), ("b/kernel", (3, 3, 16, 16)), ("e/embedding", (10, 8)), ("a/bias", (48,))]


def _store(dev, optimizer="adamw", **kw):
    """A leaf in each of the four (quantised x decayed) segments."""
    from stable_diffusion_training_amd import params
    st = params.ParamStore(SPEC, device=dev, quantise=True, quant_excluded=("bias", "embedding"), wd_excluded=("b", "bias"), block_size=16,
                           with_ema=True, optimizer=optimizer, **kw)
    assert [(q, d, b > a) for q, d, a, b in st.segments] == [(True, True, True), (True, False, True), (False, True, True), (False, False, True)]
    g = torch.Generator().manual_seed(11)
    st.load({p: torch.randn(shp, generator=g) * 0.1 for p, shp in SPEC})
    return st


def test_adamw_select_forty_launches_and_a_restored_count(dev):
    """40 consecutive launches from t = 0, and launches from t = 10^5 restored with ParamStore.set_step (the host rebuilds the running
    products with 10^5 float64 multiplications; b1's has gone denormal by then): scalar block, counter and both products against the
    host's sequential products in every bit - by value, and from tables with the index clamped past their ends."""
    sel = _Select(dev)
    for _ in range(40):
        sel.launch(lr=3e-4, ema_rate=0.9999)
    lr_tab = torch.tensor(L.LRSchedule("cosine", 2e-3, num_warmup_steps=3, num_training_steps=9).table())
    ema_tab = torch.tensor(L.EMASchedule("warmup", 0.999).table().reshape(-1)[:14])
    LR, EMT = _flat_in(lr_tab, F32, dev), _flat_in(ema_tab, F32, dev)
    assert 3 < LR.width < 20 and EMT.width == 14
    sel = _Select(dev)
    for _ in range(40):  # runs past the end of both tables
        sel.launch(LR=LR, EMT=EMT)
    LR.check("lr table"); EMT.check("ema table")
    st = _store(dev)
    for t0 in (1000, 10 ** 5):
        st.set_step(t0)
        assert int(st.adam_step.item()) == t0
        prods = AR.products(t0, *st.adam_betas)
        assert tuple(st.adam_prod.tolist()) == prods and 0 < prods[0] < (1e-300 if t0 > 1000 else 1e-40)
        for tabs in (None, (LR, EMT)):
            sel = _Select(dev, t0=t0, prods=tuple(st.adam_prod.tolist()), b1=st.adam_betas[0], b2=st.adam_betas[1])
            for _ in range(3):
                cur = sel.launch() if tabs is None else sel.launch(LR=tabs[0], EMT=tabs[1])
                assert cur[4] == 1.0 and (cur[5] > 1.0 if t0 == 1000 else cur[5] == 1.0)


# ------------------------------------------------------------------------------------------------ ParamStore.optimizer_step
STATE = ("master", "w", "codes", "inv_scale", "codes2", "inv_scale2", "mom", "mom2", "ema", "adam_step", "adam_prod", "adam_cur")


@pytest.mark.parametrize("mode", ["grad", "acc", "scheduled"])
def test_store_step_equals_the_restatement_leaf_by_leaf(dev, mode):
    """Two optimizer steps of an AdamW store with a leaf in each of the four segments against the restatement, leaf by leaf: from the
    gradient buffers (bf16 for the quantised kernels), from the accumulated gradient, and with a schedule installed."""
    st = _store(dev)
    ref = dict(p={p: st.p(p).reshape(-1).cpu().numpy().copy() for p in st.leaves}, m={}, ema={})
    for p, lf in st.leaves.items():
        ref["m"][p] = AR.init_state8(lf.numel, 16) if lf.quantised else (np.zeros(lf.numel, np.float32), np.zeros(lf.numel, np.float32))
        ref["ema"][p] = ref["p"][p].copy()
    lrs, emas = L.LRSchedule("cosine", STEP_HP["lr"], num_warmup_steps=1, num_training_steps=4), L.EMASchedule("warmup", 0.999)
    if mode == "scheduled":
        st.set_schedule(lr=lrs, ema=emas)
    t, prods = 0, (1.0, 1.0)
    for step in range(2):
        flat = torch.zeros(st.total)
        gen = torch.Generator().manual_seed(50 + step)
        for p, lf in st.leaves.items():  # the gaps between leaves stay zero, as zero_grad leaves them
            flat[lf.offset: lf.offset + lf.numel] = torch.randn(lf.numel, generator=gen) * (0.5 if step else 1e-3)
        st.set_grad_flat(flat)
        if mode == "acc":
            st.accumulate("init")
            st.accumulate("scale", scale=0.5, norm=True)
            g_seen = (st.grad_flat().cpu().numpy() * np.float32(0.5)).astype(np.float32)
        else:
            g_seen = st.grad_flat().cpu().numpy()
        assert st.grad16 is not None and not np.array_equal(g_seen[: st.quant_total], (flat.numpy() * (0.5 if mode == "acc" else 1))[: st.quant_total])
        st.optimizer_step(ema_rate=0.999, grad_source="acc" if mode == "acc" else "grad", **STEP_HP)
        kw = dict(lr_tab=lrs.table(), ema_tab=emas.table()) if mode == "scheduled" else dict(lr=STEP_HP["lr"], ema_rate=0.999)
        cur, t, prods = AR.select_scalars(t, prods, *st.adam_betas, **kw)
        _reference_store_step(st, ref, g_seen, cur)
        torch.cuda.synchronize()
        assert_equal_bits(st.adam_cur.cpu(), torch.from_numpy(cur), f"{mode} step {step}: scalar block")
        assert int(st.adam_step.item()) == st.count == step + 1 and tuple(st.adam_prod.tolist()) == prods
        _check_store(st, ref, f"{mode} step {step}")
    with pytest.raises(ValueError, match="eps belongs to AdamW"):
        _store(dev, optimizer="lion").optimizer_step(lr=1e-3, wd=0.0, eps=1e-8)


def test_eight_way_slices_of_the_adamw_sweep_equal_the_whole_store_step(dev):
    """The eight-virtual-rank slicing of tests/test_gpu_dp.py for an AdamW store: each rank sweeps its slices of every scattered bucket
    (pieces per rank, sq_done) on its own copy; the union of the slices equals the whole-store step bit for bit - masters, both code and
    scale streams, EMA, bf16 mirror - over three carried steps."""
    from stable_diffusion_training_amd import nets, params
    world = 8
    spec = nets.unet_spec(nets.unet_config("tiny"))
    weights = nets.init_params(spec, 1)
    kw = dict(device=dev, quantise=True, quant_excluded=("bias", "scale", "embedding"), wd_excluded=("bias", "scale"), block_size=16, with_ema=True,
              optimizer="adamw")
    ref = params.ParamStore(spec, **kw)
    ref.load(weights)
    ranks = []
    for r in range(world):
        st = params.ParamStore(spec, **kw)
        st.load(weights)
        st.sharded = True
        ranks.append(st)
    buckets = ref.shard_buckets(world, 1 << 16)
    assert sum(1 for a, b, q, d in buckets if q) > 4

    def pieces(r):
        out = []
        for a, b, q, d in buckets:
            n = (b - a) // world
            out.append((a + r * n, a + (r + 1) * n, q, d) if q else (a, b, q, d))
        return out

    names = ("master", "codes", "inv_scale", "codes2", "inv_scale2", "ema", "w")
    for step in range(3):
        g = (torch.randn(ref.total, generator=torch.Generator().manual_seed(step)) * (0.3 if step else 1e-4)).to(dev)
        ref.set_grad_flat(g)
        ref.optimizer_step(ema_rate=0.999, **STEP_HP)
        for r, st in enumerate(ranks):
            st.set_grad_flat(g)
            st.sqnorm.zero_()
            for rr in range(world):
                for a, b, q, d in pieces(rr):
                    if q:
                        st.sqnorm_accumulate(a, b)
            st.optimizer_step(ema_rate=0.999, shard=(pieces(r), True), **STEP_HP)
        for name in names:
            per = ref.block_size if name.startswith("inv_scale") else 1
            for a, b, q, d in buckets:
                if not q:
                    continue
                n = (b - a) // world
                for r, src in enumerate(ranks):
                    lo, hi = (a + r * n) // per, (a + (r + 1) * n) // per
                    for dst in ranks:
                        if dst is not src:
                            getattr(dst, name)[lo:hi].copy_(getattr(src, name)[lo:hi])
        torch.cuda.synchronize()
        for st in ranks[:2] + ranks[-1:]:
            for name in names + ("mom", "mom2", "adam_step", "adam_prod", "adam_cur"):
                a_, b_ = getattr(st, name), getattr(ref, name)
                n = ref.total if name in ("master", "ema", "w", "codes", "codes2") else b_.numel()
                _same(a_[:n], b_[:n], f"step {step}: {name} of a sliced rank against the whole-store step")
    assert ref.codes.any() and ref.codes2.any() and int(ref.codes2.min()) >= 0


# ------------------------------------------------------------------------------------------------ train step
_TC = []


def _states(case, dev):
    from stable_diffusion_training_amd import training_utils as tu
    from tests.helpers import build_hip_states
    if not _TC:  # the tiny TrainingConfig of the other GPU tests (it has no field for the optimizer: that is a keyword)
        _TC.append(build_hip_states(case, dev, quantize=True, ema=True)[0])
    tc = _TC[0]
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    states = tu.on_device_model_training_state(tc, models, device=dev, optimizer=dict(name="adamw", weight_decay=1e-2))
    us, ts = states[0], states[1]
    assert us.store.optimizer == ts.store.optimizer == "adamw" and us.hyper == dict(lr=1e-6, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0)
    for st in (us, ts):  # a rate at which three steps move the weights visibly
        st.hyper["lr"] = 1e-4
    return tc, states


def _inputs(case, dev, step):
    g = torch.Generator().manual_seed(100 + step)
    batch = to_dev(case["batch"], dev)
    batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
    rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
            for k, v in case["rand"].items()}
    return batch, rand


def _snap(us, ts):
    torch.cuda.synchronize()
    out = {f"{name}.{b}": getattr(st, b).clone() for name, st in (("unet", us.store), ("text", ts.store)) for b in STATE
           if getattr(st, b) is not None}
    out["counts"] = torch.tensor([us.store.count, ts.store.count])
    return out


EMA_RATE = 0.999


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


def test_train_step_eager_captured_and_resumed_are_bit_identical(dev, tmp_path):
    """The tiny UNet / text tower with optimizer="adamw": five eager steps against the graphed shape table (its last three calls replay the
    captured step) - masters, both moment states, EMA, bf16 mirror, device counters, products and scalar blocks bit-identical after every
    step; then save after step 2, load into fresh states and run step 3: identical to the uninterrupted run.  The step-3 loss is finite."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
    eager = _eager(case, dev, 5, us, ts, ue, te, vae, sc)
    assert bool(torch.isfinite(eager[2]["loss"]).all())
    assert not torch.equal(eager[2]["unet.master"], eager[0]["unet.master"]) and eager[2]["unet.codes2"].any()
    assert eager[4]["unet.adam_step"].item() == 5 and eager[4]["counts"].tolist() == [5, 5]
    del us, ts, ue, te, vae
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
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
            _same(snap[k], eager[t][k], f"step {t}: {k}, graphed table against eager")
    assert fn.graph is not None and fn.calls == 2, "the last three calls were to replay the captured step"
    assert us.store._captured
    del us, ts, ue, te, vae, table, fn
    # resume
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
    _eager(case, dev, 2, us, ts, ue, te, vae, sc)
    path = str(tmp_path / "adamw_state.safetensors")
    tu.save_training_state(path, us, ts)
    del us, ts, ue, te, vae
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
    assert int(us.store.adam_step.item()) == 0
    tu.load_training_state(path, us, ts)
    assert us.step == 2 and int(us.store.adam_step.item()) == 2 and int(ts.store.adam_step.item()) == 2
    assert_equal_bits(us.store.adam_prod, eager[1]["unet.adam_prod"], "the products rebuilt on the host against the ones the device carried")
    resumed = _eager(case, dev, 1, us, ts, ue, te, vae, sc, first=2)[0]
    for k in resumed:
        _same(resumed[k], eager[2][k], f"{k}: step 3 after save / load against the uninterrupted run")
    assert bool(torch.isfinite(resumed["loss"]).all())


# ------------------------------------------------------------------------------------------------ Lion beside it
def test_lion_sweep_beside_an_adamw_store_still_equals_its_oracle(dev):
    """In the process (and on the device) an AdamW store has just stepped in: one case of the Lion table - block 16, n = 4096 + 16, bf16
    gradient - still equals oracle.lion8 in every bit: no LDS table or template of the Lion sweep changed underneath it."""
    st = _store(dev)
    st.set_grad_flat(torch.randn(st.total, generator=torch.Generator().manual_seed(1)) * 0.1)
    st.optimizer_step(ema_rate=0.999, **STEP_HP)
    torch.cuda.synchronize()
    assert st.codes.any() and st.codes2.any()
    _lion8_run(dev, 4096 + 16, 16, 1, 1, 1, "above", 0.07, seed=21)
    _adamw8_run(dev, 4096 + 16, 16, 1, 1, 1, "above", 0.07, seed=21)
