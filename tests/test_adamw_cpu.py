"""AdamW with 8-bit block-quantised moments, the parts that need no GPU: the NumPy restatement (tests/adamw_reference.py) against
torch.optim.AdamW, the offset-free codec, zero gradients, the ABI and its refusals, Lion stores left as they were, checkpoints."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from stable_diffusion_training_amd import checkpoint as ck
from stable_diffusion_training_amd import lion_codec, params
from tests import adamw_reference as AR

F32 = np.float32


# ------------------------------------------------------------------------------------------------ restatement vs torch.optim.AdamW
def _gradients(rs, n, sigma):
    return (rs.standard_normal(n) * np.exp(sigma * rs.standard_normal(n))).astype(F32)


@pytest.mark.parametrize("steps,lr", [(50, 1e-3), (200, 1e-2)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fp32_restatement_tracks_torch_adamw_in_float64(steps, lr, seed):
    """Same gradients (Gaussian x log-normal, sigma 2, a fixed curvature per parameter), wd 1e-2, n 4096: max |p - p_torch| <= steps x
    2^-23 x max|p0| - one float32 ulp of the largest parameter per step.  The restatement rounds every operation to float32; torch runs
    the textbook formula in float64."""
    n, wd, b1, b2, eps = 4096, 1e-2, 0.9, 0.999, 1e-8
    rs = np.random.RandomState(seed)
    p0 = rs.standard_normal(n).astype(F32)
    scale = np.exp(2.0 * rs.standard_normal(n))
    pt = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n, F32), np.zeros(n, F32)
    t, prods = 0, (1.0, 1.0)
    for _ in range(steps):
        g = (rs.standard_normal(n) * scale).astype(F32)
        cur, t, prods = AR.select_scalars(t, prods, b1, b2, lr=lr)
        p, m, v = AR.step32(p, g, m, v, cur, wd=wd, b1=b1, b2=b2, eps=eps)
        pt.grad = torch.from_numpy(g).double()
        opt.step()
    diff = float(np.max(np.abs(p.astype(np.float64) - pt.detach().numpy())))
    bound = steps * 2.0 ** -23 * float(np.max(np.abs(p0)))
    print(f"steps {steps} lr {lr} seed {seed}: max diff {diff:.3e}, bound {bound:.3e} ({diff / bound:.3f} of it)")
    assert diff <= bound, (diff, bound)


def test_select_scalars_are_the_bias_corrections():
    t, prods = 0, (1.0, 1.0)
    for k in range(1, 30):
        cur, t, prods = AR.select_scalars(t, prods, 0.9, 0.999, lr=2e-3, ema_rate=0.99)
        assert t == k
        assert abs(float(cur[4]) - 1 / (1 - 0.9 ** k)) <= 2 ** -23 * float(cur[4])
        assert abs(float(cur[5]) - 1 / np.sqrt(1 - 0.999 ** k)) <= 2 ** -23 * float(cur[5])
        assert cur[0] == F32(-2e-3) and cur[1] == F32(0.99) and cur[2] == F32(1.0 - 0.99) and cur[3] == cur[6] == cur[7] == 0
    assert AR.products(29, 0.9, 0.999) == prods == params.adam_products(29, 0.9, 0.999)
    # the products underflow to exactly zero and stay there: k1 = k2 = 1
    p1, p2 = params.adam_products(10 ** 5, 0.25, 0.5)
    assert p1 == 0.0 and p2 == 0.0
    cur, _, _ = AR.select_scalars(10 ** 5, (p1, p2), 0.25, 0.5, lr=1e-3)
    assert cur[4] == 1 and cur[5] == 1
    # 0.9 rounds up in float64, so its running product settles on a denormal instead of zero: the definition is the sequence of
    # products, whatever it does, and the corrections are 1 all the same
    p1, p2 = params.adam_products(10 ** 5, 0.9, 0.999)
    assert 0.0 < p1 < 1e-320 and p1 * 0.9 == p1 and abs(p2 - 0.999 ** (10 ** 5)) < 1e-9 * p2
    cur, _, _ = AR.select_scalars(10 ** 5, (p1, p2), 0.9, 0.999, lr=1e-3)
    assert cur[4] == 1 and cur[5] == 1
    # table path: entry min(t, n - 1)
    lr_tab, ema_tab = np.array([-1, -2, -3], F32), np.array([[0, 1], [0.5, 0.5]], F32)
    for tt, i, j in ((0, 0, 0), (1, 1, 1), (2, 2, 1), (9, 2, 1)):
        cur, _, _ = AR.select_scalars(tt, (1.0, 1.0), 0.9, 0.999, lr_tab=lr_tab, ema_tab=ema_tab)
        assert cur[0] == lr_tab[i] and cur[1] == ema_tab[j, 0] and cur[2] == ema_tab[j, 1]


# ------------------------------------------------------------------------------------------------ codec
def test_codec_table_equals_the_direct_float32_formula():
    """Codes from the threshold table == rint(|x|^(1/5) x 127) in float32 on 2^16 random values of both signs and on every threshold
    with its two float32 neighbours; zero <-> code 0; root codes are never negative."""
    rs = np.random.RandomState(7)
    x = np.concatenate([rs.uniform(-1, 1, 1 << 15), rs.uniform(-1, 1, 1 << 15) ** 5]).astype(F32)
    assert np.array_equal(AR.quantize(x), AR.quantize_direct(x))
    thr = lion_codec.quantization_thresholds()
    edge = np.concatenate([thr, np.nextafter(thr, F32(-1)), np.nextafter(thr, F32(2))]).astype(F32)
    edge = edge[(edge >= 0) & (edge <= 1)]
    for sgn in (1, -1):
        assert np.array_equal(AR.quantize(F32(sgn) * edge), AR.quantize_direct(F32(sgn) * edge))
    for c in range(1, 128):  # the threshold is the first value of its code
        assert AR.quantize(thr[c:c + 1])[0] == c and AR.quantize(np.nextafter(thr[c:c + 1], F32(-1)))[0] == c - 1
    z = np.zeros(4, F32)
    z[1] = -0.0
    assert not AR.quantize(z).any() and not AR.dequantize(AR.quantize(z)).any()
    assert AR.dequantize(np.array([0], np.int8))[0] == 0 and np.all(AR.dequantize(np.arange(1, 128)) > 0)
    assert AR.dequantize(np.array([127, -127]))[0] == 1 and AR.dequantize(np.array([127, -127]))[1] == -1
    codes, inv = AR.block_quantize(np.abs(x[:4096]), 16)
    assert codes.min() >= 0 and codes.max() == 127
    codes0, inv0 = AR.block_quantize(np.zeros(64, F32), 16)
    assert not codes0.any() and np.all(inv0 == 1)
    for a, b in zip(AR.init_state8(64, 16), (codes0, inv0, codes0, inv0)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ zero gradient
@pytest.mark.parametrize("wd", [0.0, 0.07])
def test_zero_gradient_moves_by_the_decay_term_alone(wd):
    """From the initial state and after real steps whose gradients are zero in one block: the block of the 8-bit restatement equals the
    fp32 restatement's bit for bit - p + neg_lr (wd p) - and with wd = 0 it does not move."""
    n, bs, hp = 256, 16, dict(wd=wd, b1=0.9, b2=0.999, eps=1e-8)
    rs = np.random.RandomState(3)
    p8 = p32 = rs.standard_normal(n).astype(F32)
    st8, m, v = AR.init_state8(n, bs), np.zeros(n, F32), np.zeros(n, F32)
    t, prods = 0, (1.0, 1.0)
    for step in range(4):
        g = _gradients(rs, n, 2.0)
        g[:bs] = 0.0
        g[3 * bs + 2] = 0.0  # a lone zero inside a live block moves by its (zero) moments and the decay as well
        cur, t, prods = AR.select_scalars(t, prods, 0.9, 0.999, lr=1e-3)
        before = p8.copy()
        p8, st8 = AR.step8(p8, g, st8, cur, bs=bs, **hp)
        p32, m, v = AR.step32(p32, g, m, v, cur, **hp)
        want = before[:bs] if wd == 0 else (before[:bs] + (cur[0] * (F32(wd) * before[:bs]).astype(F32)).astype(F32)).astype(F32)
        assert np.array_equal(p8[:bs].view(np.int32), want.view(np.int32)), step
        assert np.array_equal(p8[:bs].view(np.int32), p32[:bs].view(np.int32)), step
        assert not st8[0][0].any() and not st8[2][0].any() and st8[1][0] == 1 and st8[3][0] == 1
        assert st8[2].min() >= 0
    assert p8[3 * bs + 2] == p32[3 * bs + 2]
    assert not np.array_equal(p8[bs:], before[bs:])


# ------------------------------------------------------------------------------------------------ ABI and refusals
NEW = ("sdt_adamw_select", "sdt_adamw8_step", "sdt_adamw32_step")


def test_new_symbols_are_exported_and_bound(lib):
    from stable_diffusion_training_amd import _lib
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sdt_adamw8_step"]) == 20 and len(_lib.SIGNATURES["sdt_adamw32_step"]) == 15
    assert lib.sdt_abi_version() == 5


def test_adamw_entry_points_refuse_bad_arguments_before_any_hip_call(lib):
    err = lambda: lib.sdt_last_error().decode()
    # p, g, g_bf16, m_codes, m_inv, s_codes, s_inv, ema, w_bf16, n, bs, sqnorm, thr, max_norm, cur, wd, b1, b2, eps, stream
    ok = [16, 16, 0, 16, 16, 16, 16, None, None, 32, 16, None, 16, 1.0, 16, 0.0, 0.9, 0.999, 1e-8, None]

    def a8(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.sdt_adamw8_step(*a)

    for idx in (0, 1, 3, 4, 5, 6, 12, 14):
        assert a8(**{f"i{idx}": None}) == -1 and "sdt_adamw8_step: null pointer" in err(), idx
    assert a8(i9=17) == -1 and "n=17 not a multiple of block_size=16" in err()
    for bs in (2, 3, 24, 512):
        assert a8(i10=bs, i9=bs * 2) == -1 and f"block_size must be a power of two in [4,256] (got {bs})" in err()
    for idx, ptr in ((0, 8), (1, 8), (3, 2), (5, 2), (7, 8), (8, 4), (14, 8)):
        assert a8(**{f"i{idx}": ptr}) == -1 and "sdt_adamw8_step: misaligned buffer" in err(), idx
    assert a8(i1=4, i2=1) == -1 and "misaligned" in err()  # a bf16 gradient needs 8 bytes ...
    assert a8(i1=24, i2=1, i9=0) == 0                       # ... and gets by with them (n = 0 launches nothing)
    assert a8(i9=0) == 0
    # p, g, m, v, ema, w_bf16, n, sqnorm, max_norm, cur, wd, b1, b2, eps, stream
    ok32 = [16, 16, 16, 16, None, None, 0, None, 1.0, 16, 0.0, 0.9, 0.999, 1e-8, None]
    assert lib.sdt_adamw32_step(*ok32) == 0
    for idx in (0, 1, 2, 3, 9):
        a = list(ok32)
        a[idx] = None
        assert lib.sdt_adamw32_step(*a) == -1 and "sdt_adamw32_step: null pointer or negative n" in err(), idx
    a = list(ok32)
    a[6] = -4
    assert lib.sdt_adamw32_step(*a) == -1 and "negative n" in err()
    a = list(ok32)
    a[9] = 8
    assert lib.sdt_adamw32_step(*a) == -1 and "cur must be a 16-byte aligned device block" in err()
    # step, prods, lr_tab, n_lr, ema_tab, n_ema, lr, ema_rate, b1, b2, cur, stream
    sel = [8, 8, None, 0, None, 0, 1e-3, 0.0, 0.9, 0.999, 16, None]

    def s_(**kw):
        a = list(sel)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.sdt_adamw_select(*a)

    for idx in (0, 1, 10):
        assert s_(**{f"i{idx}": None}) == -1 and "sdt_adamw_select: null pointer" in err()
    assert s_(i2=8) == -1 and "come together" in err()
    assert s_(i2=8, i4=8, i3=0, i5=1) == -1 and "at least one entry (n_lr=0, n_ema=1)" in err()
    assert s_(i8=1.0) == -1 and "b1 and b2 must lie in [0, 1)" in err()
    assert s_(i9=-0.1) == -1 and "b1 and b2 must lie in [0, 1)" in err()
    for kw in (dict(i0=4), dict(i1=4), dict(i10=8), dict(i2=8, i4=4, i3=1, i5=1)):
        assert s_(**kw) == -1 and "misaligned" in err(), kw


# ------------------------------------------------------------------------------------------------ stores
SPEC = [("a/kernel", (32, 16)), ("a/bias", (16,)), ("b/kernel", (3, 3, 8, 16)), ("n/scale", (16,)), ("e/embedding", (10, 8))]


def _store(optimizer="lion", **kw):
    return params.ParamStore(SPEC, device="cpu", quantise=True, quant_excluded=("bias", "scale", "embedding"), wd_excluded=("bias", "scale"),
                             block_size=16, with_ema=True, **({} if optimizer == "lion" else dict(optimizer=optimizer)), **kw)


def _parent_layout_digest(store):
    """checkpoint._layout_digest as it was before stores had an optimizer."""
    h = hashlib.sha256()
    for p in store.order:
        lf = store.leaves[p]
        h.update(f"{p}:{lf.shape}:{lf.offset}:{int(lf.quantised)}:{int(lf.decayed)};".encode())
    h.update(f"bs={store.block_size};total={store.total}".encode())
    return h.hexdigest()


def test_lion_store_is_what_it_was():
    st = _store()
    assert st.optimizer == "lion"
    for name in ("codes2", "inv_scale2", "mom2", "adam_step", "adam_prod", "adam_cur"):
        assert getattr(st, name) is None, name
    assert int(st.codes[0]) == 3 and torch.all(st.codes == 3) and torch.all(st.inv_scale == 1)
    assert ck._layout_digest(st) == _parent_layout_digest(st)
    with pytest.raises(ValueError, match="eps belongs to AdamW"):
        st.optimizer_step(lr=1e-3, wd=0.0, eps=1e-8)
    with pytest.raises(ValueError, match="optimizer must be one of"):
        params.ParamStore(SPEC, device="cpu", optimizer="sgd")
    frozen = params.ParamStore(SPEC, device="cpu", trainable=False, optimizer="adamw")
    assert frozen.codes2 is None and frozen.adam_step is None


def test_adamw_store_buffers_and_step_count():
    st = _store("adamw")
    assert st.optimizer == "adamw" and st.adam_betas == (0.9, 0.999)
    assert st.codes2.shape == st.codes.shape and st.codes2.dtype == torch.int8 and not st.codes.any() and not st.codes2.any()
    assert st.inv_scale2.shape == st.inv_scale.shape and torch.all(st.inv_scale2 == 1) and torch.all(st.inv_scale == 1)
    assert st.mom2.shape == st.mom.shape and not st.mom2.any()
    assert st.adam_step.dtype == torch.int64 and int(st.adam_step) == 0
    assert st.adam_prod.dtype == torch.float64 and st.adam_prod.tolist() == [1.0, 1.0]
    assert st.adam_cur.shape == (8,) and st.adam_cur.dtype == torch.float32
    assert ck._layout_digest(st) != _parent_layout_digest(st)
    st.set_step(1000)
    assert st.count == 1000 and int(st.adam_step) == 1000
    assert tuple(st.adam_prod.tolist()) == AR.products(1000, 0.9, 0.999)
    st.set_step(10 ** 5)  # b1^t has underflowed into the denormals long before
    assert st.adam_prod.tolist() == list(AR.products(10 ** 5, 0.9, 0.999)) and st.adam_prod[0] < 1e-320 and st.adam_prod[1] > 0
    with pytest.raises(ValueError, match="running products of adam_betas"):
        st.optimizer_step(lr=1e-3, wd=0.0, b2=0.99)
    lion, adamw = _store(), st
    assert adamw.state_bytes() == 2 * lion.state_bytes()
    with pytest.raises(ValueError):
        lion.export_momentum("s")
    m, s = adamw.export_momentum("m"), adamw.export_momentum("s")
    assert set(m) == set(s) == {p for p, _ in SPEC} and s["a/kernel"][0].shape == (32, 16) and s["a/bias"].shape == (16,)


def _fill(st, seed):
    g = torch.Generator().manual_seed(seed)
    for name in ("master", "ema", "mom", "mom2", "inv_scale", "inv_scale2"):
        t = getattr(st, name)
        if t is not None:
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    for name in ("codes", "codes2"):
        t = getattr(st, name)
        if t is not None:
            t.copy_(torch.randint(-127, 128, t.shape, generator=g).to(torch.int8))


def test_adamw_training_state_round_trip_and_cross_optimizer_refusal(tmp_path):
    u, t = _store("adamw"), _store("adamw")
    _fill(u, 1)
    _fill(t, 2)
    u.set_step(37)
    t.set_step(37)
    path = str(tmp_path / "adamw.safetensors")
    ck.save_training_state(path, u, t)
    u2, t2 = _store("adamw"), _store("adamw")
    ck.load_training_state(path, u2, t2)
    for a, b in ((u, u2), (t, t2)):
        assert b.count == 37 and int(b.adam_step) == 37 and torch.equal(a.adam_prod, b.adam_prod)
        assert tuple(b.adam_prod.tolist()) == AR.products(37, 0.9, 0.999)
        for name in ("master", "codes", "inv_scale", "mom", "ema", "codes2", "inv_scale2", "mom2"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        assert f.metadata()["unet.optimizer"] == "adamw" and "unet.codes2" in f.keys()
    with pytest.raises(ValueError, match="saved by the adamw optimizer .* built for lion"):
        ck.load_training_state(path, _store(), _store())
    lion_path = str(tmp_path / "lion.safetensors")
    lu, lt = _store(), _store()
    ck.save_training_state(lion_path, lu, lt)
    with safe_open(lion_path, framework="pt") as f:  # a Lion file says nothing new
        assert set(f.metadata()) == {"format", "unet.count", "unet.layout", "text_encoder.count", "text_encoder.layout"}
        assert f.metadata()["unet.layout"] == _parent_layout_digest(lu)
        assert not any("2" in k.split(".")[-1] for k in f.keys())
    with pytest.raises(ValueError, match="saved by the lion optimizer .* built for adamw"):
        ck.load_training_state(lion_path, _store("adamw"), _store("adamw"))
    ck.load_training_state(lion_path, _store(), _store())


def test_optimizer_argument_of_the_state_builder():
    from stable_diffusion_training_amd import training_utils as tu
    for bad in ("sgd", dict(name="adamw", lr=1.0), dict(b1=0.9), dict(name="lion", b1=0.8)):
        with pytest.raises(ValueError, match="optimizer"):
            tu.create_lion_optimizer_states({}, train_unet=False, train_text_encoder=False, optimizer=bad)
    assert tu.create_lion_optimizer_states({}, train_unet=False, train_text_encoder=False, optimizer="adamw") == \
        {"unet_state": None, "text_encoder_state": None}
    assert len(tu.TrainingConfig.__dataclass_fields__) == 28
