"""DoRA without a device: the float64 references (tests/dora_reference.py) proven against autograd with the norm detached, the
exactness of the integer cases tests/test_gpu_dora_kernels.py relies on, LoraConfig / adapter_spec / adapter-file plumbing and
refusals, and the library's new exports with their argument checks."""
import ctypes
import json

import numpy as np
import pytest
import torch

from oracle import nets as onets
from stable_diffusion_training_amd import _lib, lora, nets
from stable_diffusion_training_amd.params import ParamStore
from tests import dora_reference as dr
from tests import kernel_checks as kc
from tests import lora_reference as lr


# ------------------------------------------------------------------------------------------------ reference maths
@pytest.mark.parametrize("K,N,r,s", [(8, 8, 4, 2.0), (40, 72, 4, 0.5), (48, 64, 8, 1.0), (136, 72, 64, 0.25)])
def test_projection_reference_is_autograd_with_the_norm_detached(K, N, r, s):
    """d/dA, d/dB, d/dm of <G, m * v / ||v||.detach()> in float64.  The reference rounds c, g to fp32 and B * g to bf16: the comparison
    allows exactly those roundings (2^-24 relative on c and g, 2^-9 on the scaled B operand of dA)."""
    gen = torch.Generator().manual_seed(K + N + r)
    W0 = torch.randn(K, N, generator=gen, dtype=torch.float64).float()
    A = torch.randn(K, r, generator=gen).to(torch.bfloat16).double().requires_grad_(True)
    B = torch.randn(r, N, generator=gen).to(torch.bfloat16).double().requires_grad_(True)
    m = (torch.rand(N, generator=gen) + 0.5).double().requires_grad_(True)
    G = torch.randn(K, N, generator=gen).to(torch.bfloat16).double()
    v = W0.double() + s * A @ B
    norm = v.pow(2).sum(0).sqrt().detach()
    W = v * (m / norm)
    (G * W).sum().backward()
    q, c, g = dr.column_stats(v.detach(), m.detach().float())
    assert torch.allclose(c.double(), norm, rtol=2.0 ** -24, atol=0) and torch.allclose(g.double(), (m / norm).detach(), rtol=2.0 ** -22, atol=0)
    assert torch.allclose(dr.merge_ref64(W0, A.detach(), B.detach(), s, g), W.detach(), rtol=2.0 ** -22, atol=0)
    dA, dB, dm, u = dr.project_ref64(G, W0, A.detach(), B.detach(), s, c, g)
    assert torch.allclose(u, (G * v.detach()).sum(0), rtol=1e-12, atol=1e-12)
    absA = s * (G.abs() @ (B.detach().abs() * g.double()).T)
    assert bool(((dA - A.grad).abs() <= 2.0 ** -8 * absA + 1e-300).all())  # bf16(B g) carries 2^-9, g 2^-22 relative
    assert torch.allclose(dB, B.grad, rtol=2.0 ** -21, atol=1e-300)
    absu = (G.abs() * W0.double().abs()).sum(0) + s * (B.detach().abs() * (A.detach().abs().T @ G.abs())).sum(0)
    assert bool(((dm - m.grad).abs() <= 2.0 ** -22 * absu / norm).all())


def test_reference_rounding_points():
    # B * g rounded to bf16 once more: bf16(1.5 * fl32(1 + 2^-8)) = bf16(1.505859375) = 1.5078125 (RNE at 8 bits: 2^-7 steps)
    g = torch.tensor([1.0 + 2.0 ** -8])
    assert dr.scaled_b(torch.tensor([[1.5]]), g).item() == 1.5078125
    # c: float64 sqrt rounded once; g: correctly rounded quotient; zero column: g = 0, dm = 0
    q, c, gg = dr.column_stats(torch.tensor([[3.0, 0.0], [4.0, 0.0]]), torch.tensor([10.0, 7.0]))
    assert q.tolist() == [25.0, 0.0] and c.tolist() == [5.0, 0.0] and gg.tolist() == [2.0, 0.0]
    dA, dB, dm, u = dr.project_ref64(torch.ones(2, 2), torch.tensor([[3.0, 0.0], [4.0, 0.0]]), torch.zeros(2, 4), torch.zeros(4, 2), 1.0, c, gg)
    assert dm.tolist() == [7.0 / 5.0, 0.0] and not bool(torch.isnan(dA).any() | torch.isnan(dB).any())
    third = dr.fl32_div(torch.tensor([1.0]), torch.tensor([3.0]))
    assert third.item() == np.float32(1.0) / np.float32(3.0)


def test_numpy_float32_sqrt_is_the_double_rounded_root():
    x = (torch.arange(1, 20001, dtype=torch.float64) / 4)
    assert np.array_equal(np.sqrt(x.numpy().astype(np.float32)), np.sqrt(x.numpy()).astype(np.float32))


# ------------------------------------------------------------------------------------------------ exactness of the GPU cases
def test_every_integer_case_is_exact_in_fp32():
    """Per exact case of the GPU file (its own seeds): every column's q in quarter units and |u| - by the sum of magnitudes - in half
    units stay below 2^24, so c, g = 2^e, W', dA, dB and u are determined bit for bit."""
    worst_q = worst_u = 0.0
    for i, (K, N, r) in enumerate(dr.CASES):
        for seed, s in ((100 + i, dr.SCALES[i % 3]), (300 + 10 * i, dr.SCALES[(i + 1) % 3])):  # single launches; the grouped launch
            W0, A, B, G = dr.exact_operands(K, N, r, seed)
            assert float(W0.abs().max()) <= 8 and float(A.abs().max()) <= 1 and float(B.abs().max()) <= 1 and float(G.float().abs().max()) <= 3
            q4, u2 = dr.exact_units(W0, A, B, G, s)
            assert q4 < kc.LIMIT and u2 < kc.LIMIT, (K, N, r, s, q4, u2)
            worst_q, worst_u = max(worst_q, q4), max(worst_u, u2)
            v = lr.merge_ref64(W0, A, B, s)
            q, c, _ = dr.column_stats(v)
            m, g = dr.exact_magnitude(c)
            assert torch.equal(dr.fl32_div(m, c)[c != 0], g[c != 0]), "m / c is not the power of two"
            Wp = dr.merge_ref64(W0, A, B, s, g)
            dA, dB, dm, u = dr.project_ref64(G, W0, A, B, s, c, g)
            for x in (q, Wp, dA, dB, u):
                assert torch.equal(x.float().double(), x)
    print(f"largest 4q {worst_q:.0f}, largest 2|u| bound {worst_u:.0f}, limit {kc.LIMIT}")
    for K, N, r, s, seed in ((40, 72, 4, 2.0, 400), (136, 72, 64, 0.5, 410)):  # the one-destination launches
        q4, u2 = dr.exact_units(*dr.exact_operands(K, N, r, seed), s)
        assert q4 < kc.LIMIT and u2 < kc.LIMIT


# ------------------------------------------------------------------------------------------------ lora.py
def _tiny_base(**kw):
    spec = nets.unet_spec(onets.unet_config("tiny", **kw))
    st = ParamStore(spec, device="cpu", trainable=False, quantise=False)
    st.load(onets.init_params(onets.unet_param_shapes(onets.unet_config("tiny", **kw)), 1))
    return st


def test_config_and_adapter_spec():
    cfg = lora.LoraConfig(8, 4.0, lora.UNET_TARGETS, 0, True)  # dora is the last field
    assert cfg.dora and not lora.LoraConfig(8, 4.0).dora
    with pytest.raises(ValueError, match="dora"):
        lora.LoraConfig(8, 4.0, dora=1)
    spec = nets.unet_spec(onets.unet_config("tiny"))
    plain = lora.adapter_spec(spec, lora.LoraConfig(8, 4.0))
    got = lora.adapter_spec(spec, cfg)
    shapes = dict(spec)
    assert [x for x in got if not x[0].endswith("/lora_m")] == plain and len(got) == 3 * len(plain) // 2
    for i in range(0, len(got), 3):
        dense = got[i][0][: -len("/lora_a")]
        assert [p for p, _ in got[i: i + 3]] == [dense + "/lora_a", dense + "/lora_b", dense + "/lora_m"]
        assert got[i + 2][1] == (shapes[dense + "/kernel"][1],)


def test_attach_builds_tables_statistics_and_the_magnitude():
    base = _tiny_base()
    ad = lora.attach(base, lora.LoraConfig(8, 4.0, seed=3, dora=True), quantise=True, quant_excluded=("bias",), wd_excluded=("bias",))
    plain = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, seed=3), quantise=True, quant_excluded=("bias",), wd_excluded=("bias",))
    assert len(ad.dora_host) == len(ad.jobs_host) == len(ad.paths)
    assert bytes(ad.jobs_host) == bytes(plain.jobs_host), "the SdtLoraJob table of a DoRA adapter is the LoRA adapter's"
    assert plain.dora_host is None and plain.stats is None
    stripes = off = 0
    for i, p in enumerate(ad.paths):
        a, b, m = ad.adapted[p]
        K, N = base.leaves[p].shape
        lm, j, x = ad.store.leaves[m], ad.jobs_host[i], ad.dora_host[i]
        assert lm.shape == (N,) and not lm.quantised and not lm.decayed, "a magnitude keeps fp32 moments and takes no weight decay"
        assert ad.store.leaves[a].quantised and ad.store.leaves[b].decayed
        assert (x.m_off, x.gm_off, x.stat_off, x.N, x.stripe0_merge) == (lm.offset, lm.offset, off, N, stripes)
        assert (j.a_off, j.b_off) == (ad.store.leaves[a].offset, ad.store.leaves[b].offset) and x.m_off % 8 == 0
        stripes += (N + 63) // 64
        off += 2 * N
        # B = 0: m is the column norm of W0 (CPU store: float64 norm rounded to fp32)
        assert torch.equal(ad.store.p(m), base.p(p).double().pow(2).sum(0).sqrt().float())
        assert torch.equal(ad.store.p(a), plain.store.p(a)) and not bool(ad.store.p(b).any())
    assert ad.stats.numel() == off and ad.stats.dtype == torch.float32


def test_a_fresh_adapter_with_an_ema_starts_the_ema_magnitude_at_the_masters():
    """An EMA whose m started at zero would merge adapted kernels with a gain near zero until the average has caught up."""
    ad = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, seed=3, dora=True), with_ema=True)
    assert ad.store.ema is not None and torch.equal(ad.store.ema, ad.store.master)
    for p in ad.paths:
        lm = ad.store.leaves[ad.adapted[p][2]]
        assert float(ad.store.ema[lm.offset: lm.offset + lm.numel].min()) > 0, p


def test_explicit_masks_are_refused_for_a_dora_adapter():
    """quant_mask / decay_mask trees replace the exclusion patterns and would quantise or decay lora_m silently."""
    spec = lora.adapter_spec(nets.unet_spec(onets.unet_config("tiny")), lora.LoraConfig(8, 4.0, dora=True))
    every = {p: True for p, _ in spec}
    for kw in (dict(quant_mask=every), dict(decay_mask=every)):
        with pytest.raises(ValueError, match="quant_mask / decay_mask"):
            lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, dora=True), **kw)
    plain = {p: True for p, _ in lora.adapter_spec(nets.unet_spec(onets.unet_config("tiny")), lora.LoraConfig(8, 4.0))}
    lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0), decay_mask=plain)  # a LoRA adapter takes them as before


def test_adapter_file_round_trip_and_the_lora_dora_mismatch(tmp_path):
    ad = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, seed=1, dora=True))
    ad.store.master.copy_(torch.randn(ad.store.total, generator=torch.Generator().manual_seed(2)))
    dpath, lpath = str(tmp_path / "dora.npz"), str(tmp_path / "lora.npz")
    ad.save(dpath)
    fresh = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, seed=7, dora=True))
    fresh.load(dpath)
    for p in ad.store.order:
        assert torch.equal(fresh.store.p(p), ad.store.p(p)), p
    plain = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, seed=1))
    plain.save(lpath)
    with np.load(dpath) as z:
        assert json.loads(bytes(z["__meta__"]).decode())["dora"] is True and any(k.endswith("/lora_m") for k in z.files)
    with np.load(lpath) as z:  # a LoRA file is what it was: no "dora" key at all
        assert set(json.loads(bytes(z["__meta__"]).decode())) == {"rank", "alpha", "targets", "base_shapes"}
    with pytest.raises(ValueError, match="a LoRA adapter file, this adapter is a DoRA adapter"):
        fresh.load(lpath)
    with pytest.raises(ValueError, match="a DoRA adapter file, this adapter is a LoRA adapter"):
        plain.load(dpath)
    with pytest.raises(ValueError, match="rank 8, this adapter has rank 4"):
        lora.attach(_tiny_base(), lora.LoraConfig(4, 4.0, dora=True)).load(dpath)


def test_training_state_meta_tells_dora_from_lora():
    from stable_diffusion_training_amd import checkpoint
    a = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0, dora=True))
    b = lora.attach(_tiny_base(), lora.LoraConfig(8, 4.0))
    assert checkpoint._lora_meta(a) != checkpoint._lora_meta(b) and "dora" not in checkpoint._lora_meta(b)


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_and_argument_checks(lib):
    assert lib.sdt_abi_version() == 5
    for name in ("sdt_dora_merge", "sdt_dora_init_magnitude", "sdt_dora_project"):
        assert hasattr(lib, name), name
    assert lib.sdt_lora_job_size() == ctypes.sizeof(_lib.SdtLoraJob) == 96
    assert lib.sdt_dora_job_size() == ctypes.sizeof(_lib.SdtDoraJob) == 32
    jobs, _ = dr.layout([(40, 72, 4, 1.0), (8, 8, 4, 0.5)])
    good, gdora = dr.job_tables(jobs)
    p = 4096  # any aligned non-null address: every call below fails its checks before anything is launched

    def merge(t, x, host=True, xhost=True, dev=p, xdev=p, n=2, w0=p, w=p, stat=p):
        return lib.sdt_dora_merge(w0, p, w, None, stat, t if host else None, x if xhost else None, dev, xdev, n, None)

    def init(t, x, host=True, xhost=True, dev=p, xdev=p, n=2, w0=p, w=p, stat=p):
        return lib.sdt_dora_init_magnitude(w0, p, w, t if host else None, x if xhost else None, dev, xdev, n, None)

    def project(t, x, host=True, xhost=True, dev=p, xdev=p, n=2, w0=p, w=p, stat=p):
        return lib.sdt_dora_project(w, w0, p, p, stat, t if host else None, x if xhost else None, dev, xdev, n, None)

    for call in (merge, init, project):
        assert call(None, None, host=False, xhost=False, dev=None, xdev=None, n=0, w0=None, w=None, stat=None) == 0  # n == 0: nothing to do
        assert call(good, gdora, n=-1) == -1
        for kw in (dict(host=False), dict(xhost=False), dict(dev=None), dict(xdev=None)):
            assert call(good, gdora, **kw) == -1 and b"null job table" in lib.sdt_last_error(), kw
        assert call(good, gdora, w0=None) == -1 and b"null pointer" in lib.sdt_last_error()
        assert call(good, gdora, w0=p + 4) == -1 and b"aligned" in lib.sdt_last_error()
        for field, value, msg in (("r", 12, b"rank 12"), ("K", 44, b"multiples of 8"), ("N", 70, b"multiples of 8"), ("a_off", 12, b"offsets")):
            bad, _ = dr.job_tables(jobs)
            setattr(bad[0], field, value)
            assert call(bad, gdora) == -1, field
            assert msg in lib.sdt_last_error(), (field, lib.sdt_last_error())
        bad, _ = dr.job_tables(jobs)
        bad[1].N = 16  # (the last job: the running tile counts of the job table itself still hold)
        assert call(bad, gdora) == -1 and b"mismatched tables" in lib.sdt_last_error(), lib.sdt_last_error()
        for field, value, msg in (("m_off", 12, b"DoRA offsets"), ("gm_off", -8, b"DoRA offsets"), ("stat_off", 4, b"DoRA offsets"),
                                  ("N", 80, b"mismatched tables"), ("stripe0_merge", 1, b"running stripe count")):
            _, bad = dr.job_tables(jobs)
            setattr(bad[0], field, value)
            assert call(good, bad) == -1, field
            assert msg in lib.sdt_last_error(), (field, lib.sdt_last_error())
        _, bad = dr.job_tables(jobs)
        bad[1].stripe0_merge = 1  # 72 columns are two stripes
        assert call(good, bad) == -1 and b"running stripe count" in lib.sdt_last_error()
    assert merge(good, gdora, w=None) == -1 and b"no destination" in lib.sdt_last_error()
    assert merge(good, gdora, stat=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert merge(good, gdora, stat=p + 8) == -1 and b"aligned" in lib.sdt_last_error()
    assert project(good, gdora, stat=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert project(good, gdora, w=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert init(good, gdora, w=None) == -1 and b"null pointer" in lib.sdt_last_error()
