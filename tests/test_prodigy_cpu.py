"""Prodigy, the parts that need no GPU: the NumPy float32 restatement (tests/prodigy_reference.py) against the plain float64 version on a
problem whose distance to the solution is known, the host logic of a Prodigy ParamStore (construction, refusals, set_step, checkpoints,
the state builder's dict form), and the ABI with its refusals."""
import math

import numpy as np
import pytest
import torch

from stable_diffusion_training_amd import checkpoint as ck
from stable_diffusion_training_amd import params
from tests import prodigy_reference as PR

F32 = np.float32

# ------------------------------------------------------------------------------------------------ restatement vs float64
# The largest relative deviation of the float32 restatement's d trajectory from the float64 one over the six runs below was measured as
# 4.5e-7 (flags on, D = 100; 9.8e-8 without the flags); the gate is 20 times that.
D_TRAJECTORY_GATE = 20 * 4.5e-7
SCALES = (0.01, 1.0, 100.0)


def _quadratic(D, flags):
    """f(x) = 0.5 |x - x*|^2 in 64 dimensions from x0 = 0 with |x*| = D, 400 steps: (d / D of the float64 run, f / f0 of both runs, both d
    trajectories)."""
    rs = np.random.RandomState(5)
    xs = rs.standard_normal(64)
    xs *= D / np.linalg.norm(xs)
    kw = dict(use_bias_correction=flags, safeguard_warmup=flags)
    x64, d64 = PR.textbook64(lambda x: x - xs, np.zeros(64), 400, **kw)
    hp, xs32 = PR.hyper(**kw), xs.astype(F32)
    st, buf, p, d32 = PR.init_state(hp), PR.zeros(64), np.zeros(64, F32), []
    for _ in range(400):
        p, _ = PR.step(p, (p - xs32).astype(F32), buf, st, hp)
        d32.append(st["d"])
    f = lambda x, t: 0.5 * float(np.sum((np.asarray(x, np.float64) - t) ** 2))
    return np.array(d64), np.array(d32), f(x64, xs) / f(0, xs), f(p, xs32.astype(np.float64)) / f(0, xs)


@pytest.mark.parametrize("flags", [False, True], ids=["plain", "bias_correction+safeguard"])
def test_restatement_tracks_the_float64_version_and_d_scales_with_the_distance(flags):
    ratios = []
    for D in SCALES:
        d64, d32, f64, f32 = _quadratic(D, flags)
        dev = float(np.max(np.abs(d32 - d64) / d64))
        print(f"flags {flags} D {D}: d/D {d64[-1] / D:.5f} (float32 {d32[-1] / D:.5f}), f/f0 {f64:.3e} (float32 {f32:.3e}), "
              f"max relative deviation of d {dev:.3e} (gate {D_TRAJECTORY_GATE:.1e})")
        assert np.all(np.diff(d64) >= 0) and np.all(np.diff(d32) >= 0), "d decreased"
        assert d64[0] >= 1e-6 and d64[-1] > 100 * 1e-6 and d32[-1] > 100 * 1e-6, "d never left d0"
        assert f64 < 1e-4 and f32 < 1e-4, (f64, f32)
        assert dev <= D_TRAJECTORY_GATE, (D, dev)
        ratios.append(d64[-1] / D)
    assert max(ratios) / min(ratios) < 1.5, ratios


def test_select_and_finish_scalars():
    hp = PR.hyper(use_bias_correction=True)
    st = PR.init_state(hp)
    cur = PR.select(st, hp, ema_rate=0.99)
    d0 = hp["d0"]
    bc = math.sqrt(1 - 0.999) / (1 - 0.9)
    assert st["t"] == 1 and cur[3] == 1 and cur[7] == 0 and cur[1] == F32(0.99) and cur[2] == F32(1.0 - 0.99)
    assert cur[0] == F32(-(d0 * 1.0) * bc) and cur[4] == F32(d0 * (1.0 - 0.9)) and cur[5] == F32(d0 * d0 * (1.0 - 0.999))
    assert cur[6] == F32(st["q"]) and st["q"] == (d0 / d0) * ((d0 * 1.0) * bc)
    # l1 == 0: d stays, numer moves; d_eps is the rounding of d eps
    st["dot"], st["l1"] = 2.0, 0.0
    PR.finish(st, hp, cur)
    assert st["d"] == d0 and st["numer"] == st["q"] * 2.0 and cur[7] == F32(d0 * 1e-8)
    # d == d0: d jumps to d_hat; afterwards it only follows d_max
    st["l1"] = 1e-3
    PR.finish(st, hp, cur)
    d_hat = st["numer"] / 1e-3
    assert st["d"] == st["d_max"] == d_hat > d0
    assert PR.select(st, hp)[3] == 0
    # a finite growth rate binds
    hp2 = PR.hyper(growth_rate=1.5)
    st2 = PR.init_state(hp2)
    st2.update(d=2e-6, d_max=2e-6, numer=1.0, q=0.0, dot=0.0, l1=1.0, lr_t=1.0)
    PR.finish(st2, hp2, np.zeros(8, F32))
    assert st2["d"] == 2e-6 * 1.5 and st2["d_max"] == hp2["beta3"] * 1.0 / 1.0
    # lr_t == 0 leaves d alone
    st3 = PR.init_state(hp)
    st3.update(numer=1.0, l1=1.0, lr_t=0.0)
    PR.finish(st3, hp, np.zeros(8, F32))
    assert st3["d"] == d0 and st3["d_max"] == d0
    # tables: lr_tab holds -lr_t
    st4 = PR.init_state(hp, t=7)
    cur = PR.select(st4, hp, lr_tab=np.array([-0.0, -0.5, -1.0], F32), ema_tab=np.array([[0, 1], [0.5, 0.5]], F32))
    assert st4["lr_t"] == 1.0 and st4["t"] == 8 and cur[1] == 0.5 and (st4["P1"], st4["P2"]) == PR.products(8, 0.9, 0.999)


def test_ordered_sum_is_exact_on_integers_and_follows_the_partition():
    from tests import kernel_checks as kc
    for n in (1, 3, 1023, 1024, 1025, 8191 * 4 + 2, (1 << 20) + 5):
        x = np.random.RandomState(n % 97).randint(-9, 10, n).astype(np.float64)
        assert PR.ordered_sum(x, 5.0) == 5.0 + x.sum()
    n = 8191 * 4 + 2  # the partials of the workgroups are kernel_checks' for the same partition
    x = np.random.RandomState(1).randint(-9, 10, n).astype(np.float64)
    assert float(kc.sqnorm_parts(torch.from_numpy(x), n).sum()) == PR.ordered_sum(x)


# ------------------------------------------------------------------------------------------------ ABI and refusals
NEW = ("sdt_prodigy_select", "sdt_prodigy_moments_step", "sdt_prodigy_finish", "sdt_prodigy_apply_step")


def test_new_symbols_are_exported_and_bound(lib):
    from stable_diffusion_training_amd import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert "sdt_prodigy_workspace_bytes" in _lib.WS_QUERY
    assert lib.sdt_prodigy_workspace_bytes() == 65536 + 2 * 2048 * 8 == lib.sdt_sqnorm_workspace_bytes() + 2048 * 8
    assert [len(_lib.SIGNATURES[n]) for n in NEW] == [15, 18, 8, 9]
    assert lib.sdt_abi_version() == 5


def _caller(fn, ok):
    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    return call


def test_prodigy_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    err = lambda: lib.sdt_last_error().decode()
    inf, nan = float("inf"), float("nan")
    # step, state, lr_tab, n_lr, ema_tab, n_ema, lr, ema_rate, b1, b2, d0, use_bias_correction, safeguard_warmup, cur, stream
    sel = _caller(lib.sdt_prodigy_select, [8, 8, None, 0, None, 0, 1.0, 0.0, 0.9, 0.999, 1e-6, 0, 0, 16, None])
    for idx in (0, 1, 13):
        assert sel(**{f"i{idx}": None}) == -1 and "sdt_prodigy_select: null pointer" in err()
    assert sel(i2=8) == -1 and "come together" in err()
    assert sel(i2=8, i4=8, i3=0, i5=1) == -1 and "at least one entry (n_lr=0, n_ema=1)" in err()
    for kw in (dict(i6=nan), dict(i6=inf), dict(i7=nan), dict(i10=inf)):
        assert sel(**kw) == -1 and "non-finite" in err(), kw
    for d0 in (0.0, -1e-6):
        assert sel(i10=d0) == -1 and "d0 must be positive" in err()
    for kw in (dict(i8=1.0), dict(i9=-0.1), dict(i8=nan)):
        assert sel(**kw) == -1 and "b1 and b2 must lie in [0, 1)" in err(), kw
    for kw in (dict(i0=4), dict(i1=4), dict(i13=8), dict(i2=8, i4=4, i3=1, i5=1)):
        assert sel(**kw) == -1 and "misaligned" in err(), kw
    # p, g, g_bf16, p0, m, v, s, n, sqnorm, max_norm, cur, state, b1, b2, beta3, workspace, workspace_bytes, stream
    ws = lib.sdt_prodigy_workspace_bytes()
    mom = _caller(lib.sdt_prodigy_moments_step, [16, 16, 0, 16, 16, 16, 16, 0, None, 1.0, 16, 8, 0.9, 0.999, 0.9995, 16, ws, None])
    assert mom() == 0  # n == 0 launches nothing
    for idx in (0, 1, 3, 4, 5, 6, 10, 11):
        assert mom(**{f"i{idx}": None}) == -1 and "sdt_prodigy_moments_step: null pointer" in err(), idx
    assert mom(i7=-4) == -1 and "negative n" in err()
    for idx, ptr in ((0, 8), (1, 8), (3, 8), (4, 8), (5, 4), (6, 8), (10, 8), (11, 4)):
        assert mom(**{f"i{idx}": ptr}) == -1 and "sdt_prodigy_moments_step: misaligned buffer" in err(), idx
    assert mom(i1=4, i2=1) == -1 and "misaligned" in err()  # a bf16 gradient needs 8 bytes ...
    assert mom(i1=24, i2=1) == 0                            # ... and gets by with them
    for kw in (dict(i9=nan), dict(i12=1.0), dict(i13=-0.5), dict(i14=1.0), dict(i14=nan)):
        assert mom(**kw) == -1 and "[0, 1)" in err(), kw
    for kw in (dict(i15=None), dict(i15=8), dict(i16=lib.sdt_sqnorm_workspace_bytes())):
        assert mom(**kw) == -1 and "workspace of sdt_prodigy_workspace_bytes() needed" in err(), kw
    # state, cur, beta3, d0, d_coef, growth_rate, eps, stream
    fin = _caller(lib.sdt_prodigy_finish, [8, 16, 0.9995, 1e-6, 1.0, inf, 1e-8, 0])
    for idx in (0, 1):
        assert fin(**{f"i{idx}": None}) == -1 and "sdt_prodigy_finish: null pointer" in err()
    for kw in (dict(i2=nan), dict(i3=inf), dict(i4=nan), dict(i5=nan), dict(i6=inf)):
        assert fin(**kw) == -1 and "non-finite" in err(), kw
    assert fin(i3=0.0) == -1 and "d0 must be positive" in err()
    assert fin(i2=1.0) == -1 and "beta3 must lie in [0, 1)" in err()
    for kw in (dict(i5=0.0), dict(i4=-1.0), dict(i6=-1e-8)):
        assert fin(**kw) == -1 and "must be positive" in err(), kw
    for kw in (dict(i0=4), dict(i1=8)):
        assert fin(**kw) == -1 and "misaligned" in err(), kw
    # p, m, v, ema, w_bf16, n, cur, wd, stream
    app = _caller(lib.sdt_prodigy_apply_step, [16, 16, 16, None, None, 0, 16, 0.0, None])
    assert app() == 0
    for idx in (0, 1, 2, 6):
        assert app(**{f"i{idx}": None}) == -1 and "sdt_prodigy_apply_step: null pointer" in err(), idx
    assert app(i5=-1) == -1 and "negative n" in err()
    assert app(i7=nan) == -1 and "non-finite wd" in err()
    for idx, ptr in ((0, 8), (1, 4), (2, 8), (3, 8), (4, 4), (6, 8)):
        assert app(**{f"i{idx}": ptr}) == -1 and "sdt_prodigy_apply_step: misaligned buffer" in err(), idx


# ------------------------------------------------------------------------------------------------ stores
SPEC = [("a/kernel", (32, 16)), ("a/bias", (16,)), ("b/kernel", (3, 3, 8, 16)), ("n/scale", (16,)), ("e/embedding", (10, 8))]


def _store(optimizer="prodigy", **kw):
    return params.ParamStore(SPEC, device="cpu", quantise=True, quant_excluded=("bias", "scale", "embedding"), wd_excluded=("bias", "scale"),
                             block_size=16, with_ema=True, **({} if optimizer == "lion" else dict(optimizer=optimizer)), **kw)


def test_prodigy_store_buffers_and_layout():
    assert params.OPTIMIZERS == ("lion", "adamw", "prodigy")
    st, lion = _store(), _store("lion")
    assert st.optimizer == "prodigy" and st.prodigy == dict(params.PRODIGY_DEFAULTS, beta3=math.sqrt(0.999))
    # quantise=True is ignored for the state, not for the layout: segments, offsets and the bf16 gradient are the Lion store's
    assert st.segments == lion.segments and st.total == lion.total and st.quant_total == lion.quant_total > 0
    assert {p: (lf.offset, lf.quantised, lf.decayed) for p, lf in st.leaves.items()} == \
        {p: (lf.offset, lf.quantised, lf.decayed) for p, lf in lion.leaves.items()}
    assert st.grad16 is not None and st.grad16.numel() == st.quant_total
    assert st.codes is None and st.inv_scale is None and st.codes2 is None and st.adam_step is None
    for name in ("mom", "mom2", "prodigy_s", "prodigy_p0"):
        t = getattr(st, name)
        assert t.shape == (st.total,) and t.dtype == torch.float32 and not t.any(), name
    assert st.state_bytes() == 16 * st.total
    assert st.prodigy_state.dtype == torch.float64 and st.prodigy_state.tolist() == [1e-6, 1e-6, 0, 1, 1, 0, 0, 0, 0, 0]
    assert st.prodigy_step.dtype == torch.int64 and int(st.prodigy_step) == 0
    assert st.prodigy_cur.shape == (8,) and st.prodigy_cur.dtype == torch.float32
    assert float(st.prodigy_d()) == 1e-6 and st.prodigy_d().dtype == torch.float64
    ex = st.export_prodigy_state()
    assert set(ex) == {p for p, _ in SPEC} | {""} and ex[""] == dict(d=1e-6, d_max=1e-6, numer=0.0, step=0)
    assert set(ex["b/kernel"]) == {"m", "v", "s", "p0"} and ex["b/kernel"]["p0"].shape == (3, 3, 8, 16)
    custom = _store(prodigy=dict(d0=1e-5, b2=0.99, beta3=0.9, growth_rate=1.02, use_bias_correction=True))
    assert custom.prodigy["beta3"] == 0.9 and custom.prodigy_state[:2].tolist() == [1e-5, 1e-5] and custom.prodigy["use_bias_correction"] is True
    for name in ("prodigy_s", "prodigy_p0", "prodigy_state", "prodigy_step", "prodigy_cur"):
        assert getattr(lion, name) is None and getattr(_store("adamw"), name) is None, name
    frozen = params.ParamStore(SPEC, device="cpu", trainable=False, optimizer="prodigy")
    assert frozen.prodigy_state is None and frozen.mom is None


def test_prodigy_store_refusals():
    with pytest.raises(ValueError, match="adam_betas belongs to AdamW"):
        _store(adam_betas=(0.9, 0.99))
    for opt in ("lion", "adamw"):
        with pytest.raises(ValueError, match="prodigy= belongs to optimizer='prodigy'"):
            _store(opt, prodigy=dict(d0=1e-6))
        with pytest.raises(ValueError, match="prodigy_d: this store's optimizer is"):
            _store(opt).prodigy_d()
        with pytest.raises(ValueError, match="export_prodigy_state"):
            _store(opt).export_prodigy_state()
    with pytest.raises(ValueError, match=r"prodigy= takes .* not \['lr'\]"):
        _store(prodigy=dict(lr=1.0))
    for bad, msg in ((dict(d0=0.0), "d0 must be positive"), (dict(d0=-1.0), "d0 must be positive"), (dict(b1=1.0), r"must lie in \[0, 1\)"),
                     (dict(beta3=-0.1), r"must lie in \[0, 1\)"), (dict(d_coef=float("nan")), "non-finite"), (dict(d0=float("inf")), "non-finite"),
                     (dict(growth_rate=float("nan")), "non-finite"), (dict(growth_rate=0.0), "must be positive"),
                     (dict(d_coef=0.0), "must be positive")):
        with pytest.raises(ValueError, match=msg):
            _store(prodigy=bad)
    st = _store()
    with pytest.raises(ValueError, match="sharded optimizer is not available for a Prodigy store"):
        st.optimizer_step(lr=1.0, wd=0.0, shard=([(0, 16, True, True)], True))
    with pytest.raises(ValueError, match="running products of b1=0.9, b2=0.999"):
        st.optimizer_step(lr=1.0, wd=0.0, b2=0.99)
    with pytest.raises(ValueError, match="export_momentum: a prodigy store"):
        st.export_momentum("m")
    from stable_diffusion_training_amd import dp
    with pytest.raises(ValueError, match=r"GradReducer\(shard=True\): the sharded optimizer is not available for a Prodigy store"):
        dp.GradReducer([st], shard=True)
    assert dp.GradReducer([st]).shard is False


def test_set_step_rebuilds_the_products_and_rearms_p0():
    st = _store()
    st.prodigy_state[:3].copy_(torch.tensor([3e-4, 5e-4, 0.25], dtype=torch.float64))
    for n in (1000, 10 ** 5, 0):
        st.set_step(n)
        assert st.count == n and int(st.prodigy_step) == n
        assert tuple(st.prodigy_state[3:5].tolist()) == PR.products(n, 0.9, 0.999) == params.adam_products(n, 0.9, 0.999)
        assert st.prodigy_state[:3].tolist() == [3e-4, 5e-4, 0.25], "set_step leaves d, d_max and numer alone"
    # a counter at zero is what makes the select kernel raise `first`: the next step captures p0 again
    hp = PR.hyper()
    assert PR.select(PR.init_state(hp, t=int(st.prodigy_step)), hp)[3] == 1


def _fill(st, seed):
    g = torch.Generator().manual_seed(seed)
    for name in ("master", "ema", "mom", "mom2", "prodigy_s", "prodigy_p0"):
        t = getattr(st, name)
        t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    st.prodigy_state[:3].copy_(torch.rand(3, generator=g, dtype=torch.float64))


def test_prodigy_training_state_round_trip_and_cross_optimizer_refusal(tmp_path):
    u, t = _store(), _store()
    _fill(u, 1)
    _fill(t, 2)
    u.set_step(37)
    t.set_step(37)
    path = str(tmp_path / "prodigy.safetensors")
    ck.save_training_state(path, u, t)
    u2, t2 = _store(), _store()
    ck.load_training_state(path, u2, t2)
    for a, b in ((u, u2), (t, t2)):
        assert b.count == 37 and int(b.prodigy_step) == 37
        assert tuple(b.prodigy_state[3:5].tolist()) == PR.products(37, 0.9, 0.999)
        for name in ("master", "mom", "ema", "mom2", "prodigy_s", "prodigy_p0", "prodigy_state"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        assert f.metadata()["unet.optimizer"] == "prodigy" and {"unet.prodigy_state", "unet.prodigy_p0", "unet.prodigy_s"} <= set(f.keys())
        assert "unet.codes" not in f.keys()
    with safe_open(path, framework="pt") as f:
        assert f.metadata()["unet.prodigy"] == ck._prodigy_meta(u) and "d0=1e-06" in f.metadata()["unet.prodigy"]
    for other_settings in (dict(d0=1e-5), dict(growth_rate=1.02), dict(safeguard_warmup=True), dict(beta3=0.9), dict(d_coef=2.0)):
        with pytest.raises(ValueError, match="saved by a Prodigy store with the settings .*d0=1e-06.* and this store has"):
            ck.load_training_state(path, _store(prodigy=other_settings), _store(prodigy=other_settings))
    for other in ("lion", "adamw"):
        with pytest.raises(ValueError, match=f"saved by the prodigy optimizer .* built for {other}"):
            ck.load_training_state(path, _store(other), _store(other))
        other_path = str(tmp_path / f"{other}.safetensors")
        ck.save_training_state(other_path, _store(other), _store(other))
        with pytest.raises(ValueError, match=f"saved by the {other} optimizer .* built for prodigy"):
            ck.load_training_state(other_path, _store(), _store())


def test_optimizer_argument_of_the_state_builder():
    from stable_diffusion_training_amd import training_utils as tu
    none = {"unet_state": None, "text_encoder_state": None}
    full = dict(name="prodigy", lr=0.5, b1=0.8, b2=0.99, beta3=0.9, eps=1e-6, weight_decay=0.01, d0=1e-5, d_coef=2.0, growth_rate=1.02,
                use_bias_correction=True, safeguard_warmup=True)
    for good in ("prodigy", dict(name="prodigy"), full):
        assert tu.create_lion_optimizer_states({}, train_unet=False, train_text_encoder=False, optimizer=good) == none
    for bad in (dict(name="prodigy", momentum=0.9), dict(name="adamw", d0=1e-6), dict(name="adamw", lr=1.0), dict(name="lion", d_coef=2.0)):
        with pytest.raises(ValueError, match="optimizer"):
            tu.create_lion_optimizer_states({}, train_unet=False, train_text_encoder=False, optimizer=bad)
    assert len(tu.TrainingConfig.__dataclass_fields__) == 28


def test_state_builder_makes_prodigy_stores_with_lr_one():
    """The dict form reaches the stores: hyper-parameters for optimizer_step (lr 1 unless given - the learning rates of the call are not
    used), the rest in the store's settings; with lora= the adapter's store is the Prodigy store and lora_m stays out of the decay."""
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
    from tests.helpers import make_case
    case = make_case("tiny", B=2, image=64)
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    opt = dict(name="prodigy", d0=1e-5, weight_decay=0.01, safeguard_warmup=True)
    qx = ("bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj")
    out = tu.create_lion_optimizer_states(models, device="cpu", u_net_learning_rate=123.0, text_encoder_learning_rate=456.0, optimizer=opt,
                                          quantize_unet_state=True, excluded_layer_from_quantization=qx)
    for key in ("unet_state", "text_encoder_state"):
        s = out[key]
        assert s.hyper == dict(lr=1.0, wd=0.01, eps=1e-8, max_norm=1.0)
        assert s.store.optimizer == "prodigy" and s.store.prodigy["d0"] == 1e-5 and s.store.prodigy["safeguard_warmup"] is True
        assert s.store.codes is None and s.store.mom.numel() == s.store.total
    assert out["unet_state"].store.quant_total > 0 and out["text_encoder_state"].store.quant_total == 0
    assert tu.create_lion_optimizer_states(models, device="cpu", optimizer=dict(name="prodigy", lr=0.5))["unet_state"].hyper["lr"] == 0.5
    for dora in (False, True):
        cfg = lora.LoraConfig(rank=4, alpha=4.0, dora=dora)
        te = lora.LoraConfig(rank=4, alpha=4.0, targets=lora.CLIP_TARGETS, dora=dora)
        out = tu.create_lion_optimizer_states(models, device="cpu", optimizer=opt, lora=dict(unet=cfg, text_encoder=te),
                                              excluded_layer_pattern_from_weight_decay=("bias",))
        ad = out["unet_state"].adapter
        assert ad.store.optimizer == "prodigy" and ad.store.prodigy["d0"] == 1e-5 and out["unet_state"].hyper["lr"] == 1.0
        assert not out["unet_state"].store.trainable
        ms = [lf for p, lf in ad.store.leaves.items() if p.endswith("/lora_m")]
        assert bool(ms) == dora and not any(lf.decayed or lf.quantised for lf in ms)
