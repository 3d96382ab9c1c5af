"""LoHa without a device (DESIGN.md "LoHa"): the projection formulas proven against autograd in float64, leaf order, shapes and selection on
the model specs, algo="lora" left byte for byte what it was, every config / file / command-line refusal, the new exports and their host
checks (they return before any HIP call), and the exactness of the exact cases of tests/test_gpu_loha_kernels.py."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import nets as onets
from stable_diffusion_training_amd import _lib, lora, nets
from stable_diffusion_training_amd.params import ParamStore
from tests import kernel_checks as kc
from tests import locon_reference as lc
from tests import loha_reference as lh
from tests import lora_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAVES = ("loha_a1", "loha_b1", "loha_a2", "loha_b2")


# ------------------------------------------------------------------------------------------------ the projection is the gradient
@pytest.mark.parametrize("k,stride", [(0, 1), (3, 1), (3, 2), (1, 1)], ids=["dense", "3x3", "3x3-stride2", "1x1"])
def test_the_projection_is_autograds_gradient_of_the_hadamard_form(k, stride):
    Cin, Cout, r, s = 8, 16, 4, 0.75
    g = torch.Generator().manual_seed(10 * k + stride)
    K = Cin if k == 0 else k * k * Cin
    # factors that bf16 holds exactly: the reference's rounding is then the identity and autograd sees the same function
    f = [torch.randn(shape, generator=g).to(torch.bfloat16).double().requires_grad_(True) for shape in ((K, r), (r, Cout), (K, r), (r, Cout))]
    if k == 0:
        x = torch.randn(5, Cin, generator=g, dtype=torch.float64)
        W0 = torch.randn(Cin, Cout, generator=g, dtype=torch.float64)
        forward = lambda W: x @ W
        out = forward(W0 + s * ((f[0] @ f[1]) * (f[2] @ f[3])))
    else:
        x = torch.randn(2, Cin, 9, 10, generator=g, dtype=torch.float64)
        W0 = torch.randn(k, k, Cin, Cout, generator=g, dtype=torch.float64)
        forward = lambda W: torch.nn.functional.conv2d(x, W.permute(3, 2, 0, 1), stride=stride, padding=k // 2)
        out = lh.loha_forward64(x, W0, *f, s, stride)
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (G * out).sum().backward()
    d = [t.detach() for t in f]
    W = lh.merge_ref64(W0.reshape(K, Cout), *d, s).view(W0.shape).requires_grad_(True)
    (dW,) = torch.autograd.grad((G * forward(W)).sum(), W)
    got = lh.project_ref64(dW.reshape(K, Cout), *d, s)
    for name, mine, t in zip(LEAVES, got, f):
        assert torch.allclose(mine, t.grad, rtol=1e-10, atol=1e-12), name
        assert float(t.grad.abs().max()) > 0, name


def test_zero_b2_gives_a_zero_delta_and_a_gradient_for_b2_alone():
    g = torch.Generator().manual_seed(4)
    A1, B1, A2 = torch.randn(24, 4, generator=g), torch.randn(4, 16, generator=g), torch.randn(24, 4, generator=g)
    W0, dW = torch.randn(24, 16, generator=g), torch.randn(24, 16, generator=g).to(torch.bfloat16)
    B2 = torch.zeros(4, 16)
    assert torch.equal(lh.merge_ref64(W0, A1, B1, A2, B2, 2.0), W0.double())
    dA1, dB1, dA2, dB2 = lh.project_ref64(dW, A1, B1, A2, B2, 2.0)
    assert not bool(dA1.any()) and not bool(dB1.any()) and not bool(dA2.any()) and bool(dB2.any())


# ------------------------------------------------------------------------------------------------ selection, order, shapes
@pytest.mark.parametrize("size", ["tiny", "sd15", "sd21", "sdxl"])
def test_leaf_order_shapes_and_selection_on_the_model_specs(size):
    spec = nets.unet_spec(onets.unet_config(size))
    shapes = dict((p, tuple(s)) for p, s in spec)
    cfg = lora.LoraConfig(rank=16, alpha=16, conv_rank=8, conv_alpha=4, algo="loha")
    got = lora.select_leaves(spec, cfg)
    assert got == lora.select_leaves(spec, lora.LoraConfig(rank=16, alpha=16, conv_rank=8, conv_alpha=4)), "LoHa adapts the leaves LoCon adapts"
    aspec = lora.adapter_spec(spec, cfg)
    assert [p for p, _ in aspec] == [p[:-len("kernel")] + n for p in got for n in LEAVES]
    ashapes = dict(aspec)
    assert any(len(shapes[p]) == 4 for p in got) and any(len(shapes[p]) == 2 for p in got)
    for p in got:
        stem = p[:-len("kernel")]
        K, N, r = (shapes[p][0] * shapes[p][1] * shapes[p][2], shapes[p][3], 8) if len(shapes[p]) == 4 else (shapes[p][0], shapes[p][1], 16)
        assert [ashapes[stem + n] for n in LEAVES] == [(K, r), (r, N), (K, r), (r, N)]
    dense_only = lora.adapter_spec(spec, lora.LoraConfig(rank=4, alpha=4, algo="loha"))
    assert len(dense_only) == 4 * len(lora.select_leaves(spec, lora.LoraConfig(rank=4, alpha=4)))
    assert cfg.scale == 1.0 and cfg.conv_scale == 0.5


def _tiny_base(trainable=False, **kw):
    spec = nets.unet_spec(onets.unet_config("tiny", **kw))
    st = ParamStore(spec, device="cpu", trainable=trainable, quantise=False)
    st.load(onets.init_params(onets.unet_param_shapes(onets.unet_config("tiny", **kw)), 1))
    return st


def test_attach_initialises_like_lycoris_and_builds_the_three_tables():
    base = _tiny_base()
    cfg = lora.LoraConfig(rank=8, alpha=4, seed=3, conv_rank=4, conv_alpha=2, algo="loha")
    ad = lora.attach(base, cfg)
    assert ad.store.order == [q for p in ad.paths for q in ad.adapted[p]] and all(len(ad.adapted[p]) == 4 for p in ad.paths)
    g = torch.Generator().manual_seed(3)  # one generator, leaf order
    for p in ad.paths:
        a1, b1, a2, b2 = ad.adapted[p]
        (K, r), N = ad.store.leaves[a1].shape, ad.store.leaves[b1].shape[1]
        assert torch.equal(ad.store.p(a1), torch.randn(K, r, generator=g)) and torch.equal(ad.store.p(b1), torch.randn(r, N, generator=g) * 0.1)
        assert torch.equal(ad.store.p(a2), torch.randn(K, r, generator=g)) and not bool(ad.store.p(b2).any())
    assert abs(float(ad.store.p(ad.adapted[ad.conv_paths[-1]][0]).std()) - 1.0) < 0.1
    assert len(ad.loha) == 2 and ad.split_ws is None, "LoHa allocates its own workspace, not LoCon's"
    rows = lc.rows()
    for paths, (jh, jd, sh, sd, xh, xd, ws) in zip((ad.dense_paths, ad.conv_paths), ad.loha):
        assert bytes(jh) == bytes(ad.jobs_host if paths is ad.dense_paths else ad.conv_jobs_host) and len(jh) == len(sh) == len(xh) == len(paths)
        ts = cnt = part1 = part2 = 0
        for p, j, s_, x in zip(paths, jh, sh, xh):
            names = ad.adapted[p]
            offs = [ad.store.leaves[n].offset for n in names]
            assert (j.a_off, j.b_off, j.ga_off, j.gb_off) == (offs[0], offs[1], offs[0], offs[1])
            assert (x.a2_off, x.b2_off, x.ga2_off, x.gb2_off, x.K, x.N) == (offs[2], offs[3], offs[2], offs[3], j.K, j.N)
            tb, ch = (j.N + 63) // 64, (j.K + rows - 1) // rows
            assert (s_.K, s_.N, s_.tile0, s_.chunks, s_.cnt0, s_.part_off) == (j.K, j.N, ts, ch, cnt, part1) and x.part_off == part2
            ts, cnt = ts + j.tiles_da + tb * ch, cnt + tb
            part1 += tb * ch * j.r * 64 if ch > 1 else 0
            part2 += 2 * tb * ch * j.r * 64 if ch > 1 else 0
        assert ws.numel() == (4 * cnt + 255) // 256 * 256 + 4 * part2 and not bool(ws.any())
    assert max(x.part_off for x in ad.loha[1][4]) > 0, "the tiny UNet reaches a convolution of more than one chunk"
    # the scratch and its runs are LoCon's
    locon = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, seed=3, conv_rank=4, conv_alpha=2))
    assert ad.runs == locon.runs and ad.scratch.numel() == locon.scratch.numel()
    assert bytes(ad.jobs_host)[:8] == bytes(locon.jobs_host)[:8]


# ------------------------------------------------------------------------------------------------ algo="lora" is the parent
def test_algo_lora_changes_nothing(tmp_path):
    spec = nets.unet_spec(onets.unet_config("tiny"))
    for kw in (dict(), dict(conv_rank=4, conv_alpha=2.0), dict(dora=True)):
        old, new = lora.LoraConfig(rank=8, alpha=4, seed=1, **kw), lora.LoraConfig(rank=8, alpha=4, seed=1, algo="lora", **kw)
        assert old == new and repr(old) == repr(new) and "algo" not in repr(new)
        assert lora.adapter_spec(spec, old) == lora.adapter_spec(spec, new)
        a, b = lora.attach(_tiny_base(), old), lora.attach(_tiny_base(), new)
        assert bytes(a.jobs_host) == bytes(b.jobs_host) and a.runs == b.runs and b.loha == []
        assert torch.equal(a.store.master, b.store.master)
        if kw.get("conv_rank"):
            assert bytes(a.conv_jobs_host) == bytes(b.conv_jobs_host) and bytes(a.split_host) == bytes(b.split_host)
            assert b.split_ws is not None and a.split_ws.numel() == b.split_ws.numel()
        metas = []
        for ad, name in ((a, "a.npz"), (b, "b.npz")):
            ad.save(str(tmp_path / name))
            with np.load(str(tmp_path / name)) as z:
                metas.append(bytes(z["__meta__"]))
        assert metas[0] == metas[1] and "algo" not in json.loads(metas[0])
    assert repr(lora.LoraConfig(rank=8, alpha=4.0)) == ("LoraConfig(rank=8, alpha=4.0, targets=('to_q', 'to_k', 'to_v', 'to_out_0'), seed=0, "
                                                       "dora=False)")
    assert repr(lora.LoraConfig(rank=8, alpha=4.0, algo="loha")).endswith("dora=False, algo='loha')")
    assert [n for p, _ in lora.adapter_spec(spec, lora.LoraConfig(4, 4.0))[:2] for n in [p.rsplit("/", 1)[1]]] == ["lora_a", "lora_b"]


# ------------------------------------------------------------------------------------------------ refusals
def test_config_refusals():
    for bad in ("lokr", "LoHa", None, 1, ""):
        with pytest.raises(ValueError, match="algo must be one of"):
            lora.LoraConfig(rank=4, alpha=1, algo=bad)
    with pytest.raises(ValueError, match="DoRA combined with LoHa is not supported"):
        lora.LoraConfig(rank=4, alpha=1, algo="loha", dora=True)
    for kw in (dict(rank=64), dict(rank=128), dict(rank=4, conv_rank=64), dict(rank=32, conv_rank=128)):
        with pytest.raises(ValueError, match="algo='loha' takes rank and conv_rank up to 32"):
            lora.LoraConfig(alpha=1, algo="loha", **kw)
    for r in lh.RANKS:
        assert lora.LoraConfig(rank=r, alpha=1, conv_rank=r, algo="loha").algo == "loha"
    with pytest.raises(ValueError, match="rank must be one of"):
        lora.LoraConfig(rank=12, alpha=1, algo="loha")
    with pytest.raises(ValueError, match="not a Dense kernel"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("conv1",), algo="loha"))
    with pytest.raises(ValueError, match="must be frozen"):
        lora.attach(_tiny_base(trainable=True), lora.LoraConfig(rank=4, alpha=1, algo="loha"))


def test_adapter_file_round_trip_and_kind_mismatch(tmp_path):
    cfg = dict(rank=8, alpha=4, conv_rank=4, conv_alpha=2)
    ad = lora.attach(_tiny_base(), lora.LoraConfig(seed=1, algo="loha", **cfg))
    ad.store.master.copy_(torch.randn(ad.store.total, generator=torch.Generator().manual_seed(2)))
    path = str(tmp_path / "loha.npz")
    ad.save(path)
    with np.load(path) as z:
        meta = json.loads(bytes(z["__meta__"]).decode())
        assert sorted(z.files) == sorted(["__meta__"] + ad.store.order)
    assert meta["algo"] == "loha" and meta["conv_rank"] == 4 and "dora" not in meta
    fresh = lora.attach(_tiny_base(), lora.LoraConfig(seed=9, algo="loha", **cfg))
    fresh.load(path)
    for p in ad.store.order:
        assert torch.equal(fresh.store.p(p), ad.store.p(p)), p
    with pytest.raises(ValueError, match="a LoHa adapter file, this adapter is a LoRA adapter"):
        lora.attach(_tiny_base(), lora.LoraConfig(**cfg)).load(path)
    with pytest.raises(ValueError, match="a LoHa adapter file, this adapter is a DoRA adapter"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, dora=True)).load(path)
    plain, dora = str(tmp_path / "plain.npz"), str(tmp_path / "dora.npz")
    lora.attach(_tiny_base(), lora.LoraConfig(**cfg)).save(plain)
    lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, dora=True)).save(dora)
    with pytest.raises(ValueError, match="a LoRA adapter file, this adapter is a LoHa adapter"):
        fresh.load(plain)
    with pytest.raises(ValueError, match="a DoRA adapter file, this adapter is a LoHa adapter"):
        fresh.load(dora)
    with pytest.raises(ValueError, match="rank 8, this adapter has rank 16"):
        lora.attach(_tiny_base(), lora.LoraConfig(algo="loha", **dict(cfg, rank=16))).load(path)
    with pytest.raises(ValueError, match="conv_rank 4, this adapter has conv_rank 0"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, algo="loha")).load(path)


def test_training_state_meta_names_the_algo():
    from stable_diffusion_training_amd import checkpoint
    a = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4))
    b = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, algo="loha"))
    assert checkpoint._lora_meta(a) == "rank=8;alpha=4.0;targets=to_q,to_k,to_v,to_out_0"
    assert checkpoint._lora_meta(b) == checkpoint._lora_meta(a) + ";algo=loha"


def _example():
    spec = importlib.util.spec_from_file_location("train_synthetic_example", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_takes_loha_and_refuses_it_without_lora_and_with_dora():
    ex = _example()
    with pytest.raises(ValueError, match="lora_algo.*give lora_rank"):
        ex.lora_config({"lora_algo": "loha"})
    with pytest.raises(ValueError, match="DoRA combined with LoHa is not supported"):
        ex.lora_config({"lora_rank": 4, "lora_algo": "loha", "lora_dora": True})
    with pytest.raises(ValueError, match="algo='loha' takes rank and conv_rank up to 32"):
        ex.lora_config({"lora_rank": 64, "lora_algo": "loha"})
    with pytest.raises(ValueError, match="algo must be one of"):
        ex.lora_config({"lora_rank": 4, "lora_algo": "lokr"})
    cfg = ex.lora_config({"lora_rank": 8, "lora_algo": "loha", "lora_conv_rank": 4, "lora_conv_alpha": 2.0})["unet"]
    assert (cfg.algo, cfg.rank, cfg.alpha, cfg.conv_rank, cfg.conv_scale) == ("loha", 8, 8.0, 4, 0.5)
    assert ex.lora_config({"lora_rank": 8})["unet"] == lora.LoraConfig(8, 8.0) and ex.lora_config({}) is None
    # the command line: refused by the parser, before the configuration file is opened
    script = os.path.join(ROOT, "examples", "train_synthetic.py")
    for argv, msg in ((["--loha"], "--loha needs --lora RANK"), (["--lora", "4", "--dora", "--loha"], "--loha is refused beside --dora")):
        r = subprocess.run([sys.executable, script, "/nonexistent.json"] + argv, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (argv, r.stderr[-300:])


# ------------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_bound_and_exported(lib):
    with open(os.path.join(ROOT, "include", "sdt.h")) as f:
        header = f.read()
    for name in ("sdt_loha_merge", "sdt_loha_project", "sdt_loha_project_workspace_bytes", "sdt_loha_job_size"):
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/sdt.h"
        assert name in _lib.SIGNATURES or name in _lib.WS_QUERY or name in _lib.NOARG, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.sdt_abi_version() == 5
    assert lib.sdt_lora_job_size() == ctypes.sizeof(_lib.SdtLoraJob) == 96
    assert lib.sdt_lora_split_job_size() == ctypes.sizeof(_lib.SdtLoraSplitJob) == 32
    assert lib.sdt_loha_job_size() == ctypes.sizeof(_lib.SdtLohaJob) == 48


def test_host_checks_return_before_any_hip_call(lib):
    C = lh.rows()
    cases = [(C + 8, 72, 16, 1.0), (72, 8, 4, 0.5), (2 * C + 40, 192, 32, 2.0)]
    jobs, _ = lh.layout(cases)
    good = lr.job_table(jobs)
    split, _, locon_total = lc.split_table(jobs, C)
    table, counter_bytes, total = lh.loha_table(jobs, C)
    assert counter_bytes == 256 and total == 256 + 2 * (locon_total - 256) == 256 + 2 * 4 * 64 * (2 * 2 * 16 + 3 * 3 * 32)
    assert lib.sdt_loha_project_workspace_bytes(good, 3) == total
    assert lib.sdt_loha_project_workspace_bytes(good, 0) == 0 and lib.sdt_loha_project_workspace_bytes(None, 0) == 0
    assert lib.sdt_loha_project_workspace_bytes(None, 1) == -1 and lib.sdt_loha_project_workspace_bytes(good, -1) == -1
    for r in (12, 64, 128):
        bad = lr.job_table(jobs)
        bad[1].r = r
        assert lib.sdt_loha_project_workspace_bytes(bad, 3) == -1 and f"rank {r}".encode() in lib.sdt_last_error()
    p = 4096  # any aligned non-null address: every call below fails its checks before anything is launched

    def project(jt=good, sp=split, xt=table, host=True, sphost=True, xhost=True, dev=p, spdev=p, xdev=p, n=3, dw=p, ws=p, nbytes=total):
        return lib.sdt_loha_project(dw, p, p, jt if host else None, sp if sphost else None, xt if xhost else None, dev, spdev, xdev, n, ws,
                                    nbytes, None)

    def merge(jt=good, xt=table, host=True, xhost=True, dev=p, xdev=p, n=3, w0=p, w=p, f=p):
        return lib.sdt_loha_merge(w0, p, w, f, jt if host else None, xt if xhost else None, dev, xdev, n, None)

    assert project(host=False, sphost=False, xhost=False, dev=None, spdev=None, xdev=None, n=0, dw=None, ws=None, nbytes=0) == 0
    assert merge(host=False, xhost=False, dev=None, xdev=None, n=0, w0=None, w=None, f=None) == 0  # n == 0: nothing to do
    for kw in (dict(host=False), dict(sphost=False), dict(xhost=False), dict(dev=None), dict(spdev=None), dict(xdev=None)):
        assert project(**kw) == -1 and b"null job table" in lib.sdt_last_error(), kw
    for kw in (dict(host=False), dict(xhost=False), dict(dev=None), dict(xdev=None)):
        assert merge(**kw) == -1 and b"null job table" in lib.sdt_last_error(), kw
    assert project(n=-1) == -1 and b"negative" in lib.sdt_last_error()
    assert merge(n=-1) == -1 and b"negative" in lib.sdt_last_error()
    assert project(dw=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert project(ws=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert project(ws=p + 4) == -1 and b"aligned" in lib.sdt_last_error()
    assert project(nbytes=total - 4) == -1 and b"workspace" in lib.sdt_last_error()
    assert project(nbytes=locon_total) == -1 and b"two sets of partials" in lib.sdt_last_error(), "LoCon's workspace is too small"
    assert merge(w0=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert merge(w=None, f=None) == -1 and b"no destination" in lib.sdt_last_error()
    assert merge(w=p + 2) == -1 and b"aligned" in lib.sdt_last_error()
    # sdt_lora_merge's checks on the job table, and the LoHa rank limit
    for field, value, msg in (("r", 12, b"rank 12"), ("r", 0, b"rank 0"), ("r", 64, b"rank 64: LoHa"), ("r", 128, b"rank 128: LoHa"),
                              ("K", 44, b"multiples of 8"), ("N", 70, b"multiples of 8"), ("K", 0, b"multiples of 8"),
                              ("a_off", 12, b"offsets"), ("dw_off", -8, b"offsets")):
        bad = lr.job_table(jobs)
        setattr(bad[0], field, value)
        for call in (project, merge):
            assert call(jt=bad) == -1, field
            assert msg in lib.sdt_last_error(), (field, lib.sdt_last_error())
    for field, call in (("tile0_project", project), ("tiles_da", project), ("tile0_merge", merge)):
        bad = lr.job_table(jobs)
        setattr(bad[1], field, 1 << 20)
        assert call(jt=bad) == -1 and b"running" in lib.sdt_last_error(), field
    # the split table, as sdt_lora_project_split checks it
    for i, field, value, msg in ((0, "K", C, b"mismatched tables"), (2, "N", 64, b"mismatched tables"), (0, "chunks", 1, b"chunks"),
                                 (1, "tile0", 0, b"running"), (2, "cnt0", 64, b"running"), (2, "part_off", 0, b"partial offset")):
        bad, _, _ = lc.split_table(jobs, C)
        setattr(bad[i], field, value)
        assert project(sp=bad) == -1, (i, field)
        assert msg in lib.sdt_last_error(), (i, field, lib.sdt_last_error())
    # the LoHa table: mismatched tables, offsets, the running two-set partial offset
    for i, field, value, msg in ((0, "K", C, b"mismatched tables"), (2, "N", 64, b"mismatched tables"), (1, "a2_off", 12, b"LoHa offsets"),
                                 (0, "b2_off", -8, b"LoHa offsets"), (2, "ga2_off", 4, b"LoHa offsets"), (1, "gb2_off", -16, b"LoHa offsets"),
                                 (0, "part_off", 64, b"partial offset"), (2, "part_off", split[2].part_off, b"partial offset"),
                                 (1, "part_off", 0, b"partial offset")):
        bad, _, _ = lh.loha_table(jobs, C)
        setattr(bad[i], field, value)
        for call in (project, merge):
            assert call(xt=bad) == -1, (i, field)
            assert msg in lib.sdt_last_error(), (i, field, lib.sdt_last_error())


# ------------------------------------------------------------------------------------------------ exactness of the GPU cases
def test_every_exact_case_is_exact():
    """Per case of the GPU table: the bounds of lh.exact_bounds hold for every scale, and on the operands themselves P, P1 * P2, the merged
    sum and every factor gradient are representable in fp32, G in bf16, and the largest partial sum - in ANY order, so chunk sums and
    their sum too - is an integer below 2^24 in units of the terms' common denominator."""
    C = lh.rows()
    table = lh.cases(C)
    assert len(table) == 6 and [lc.chunks(K, C) for K, N, r in table] == [1, 1, 1, 2, 3, lc.chunks(576, C)]
    assert {r for _, _, r in table} == set(lh.RANKS)
    for i, (K, N, r) in enumerate(table):
        assert K % 8 == 0 and N % 8 == 0
        for s in lh.SCALES:
            for what, bound, limit in lh.exact_bounds(K, N, r, s):
                assert bound < limit, what
        W0, A1, B1, A2, B2, dW = lh.exact_operands(K, N, r, 100 + i)
        for f in (A1, B1, A2, B2):
            assert set(f.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(f.to(torch.bfloat16).float(), f)
        assert set(dW.float().abs().unique().tolist()) <= {0.0, 1.0, 2.0, 4.0}
        s = lh.SCALES[i % 3]
        P1, P2 = lh.products(A1, B1, A2, B2)
        assert float(P1.abs().max()) <= r and float(P2.abs().max()) <= r and torch.equal(P1, P1.round()) and torch.equal(P2, P2.round())
        h = P1 * P2
        assert torch.equal(h.float().double(), h) and torch.equal((s * h).float().double(), s * h)
        v = lh.merge_ref64(W0, A1, B1, A2, B2, s)
        assert torch.equal(v.float().double(), v) and float(v.abs().max()) * 8 < kc.LIMIT
        for G in (dW.double() * P2, dW.double() * P1):
            assert torch.equal(G.float().to(torch.bfloat16).double(), G), "G is not a bf16 value"
            assert float((G.abs() @ B1.double().abs().T).max()) * s * 2 < kc.LIMIT and float((A1.double().abs().T @ G.abs()).max()) * s * 2 < kc.LIMIT
        for x in lh.project_ref64(dW, A1, B1, A2, B2, s):
            assert torch.equal(x.float().double(), x) and float(x.abs().max()) > 0
    for K, N, r in lh.random_cases(C):
        assert r in lh.RANKS and K % 8 == 0 and N % 8 == 0
    assert lc.chunks(lh.random_cases(C)[2][0], C) == 3


def test_the_derived_bound_covers_an_emulation_of_the_kernels_roundings():
    """The bound of lh.projection_bounds against a CPU emulation that rounds where the kernel rounds (P in fp32, G to bf16, fp32 sums in
    row order, chunk partials in chunk order): the emulation stays under the bound, and the bound is no more than 2^-8 + a little of the
    magnitude sums - it is derived from the unit roundoffs, not fitted."""
    C, K, N, r, s = 64, 200, 24, 8, 0.75
    g = torch.Generator().manual_seed(7)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    A1, B1, A2, B2, dW = rn(K, r), rn(r, N) * 0.1, rn(K, r), rn(r, N) * 0.1, (rn(K, N) * 0.01).to(torch.bfloat16)
    bf32 = lambda t: t.to(torch.bfloat16).float()
    P1, P2 = bf32(A1) @ bf32(B1), bf32(A2) @ bf32(B2)  # fp32 accumulation
    got = []
    for G, A, B in ((bf32(dW.float() * P2), A1, B1), (bf32(dW.float() * P1), A2, B2)):
        got.append(s * (G @ bf32(B).T))
        parts = [bf32(A[k0: k0 + C]).T @ G[k0: k0 + C] for k0 in range(0, K, C)]
        acc = parts[0]
        for p_ in parts[1:]:
            acc = acc + p_
        got.append(s * acc)
    want = lh.project_ref64(dW, A1, B1, A2, B2, s)
    bounds = lh.projection_bounds(dW, A1, B1, A2, B2, s, C)
    for name, x, w, b in zip(LEAVES, got, want, bounds):
        assert bool(((x.double() - w).abs() <= b).all()), name
    Gabs, eG = lh.g_error(dW, A2, B2)
    Pabs = lr.bf(A2).abs() @ lr.bf(B2).abs()
    assert bool((eG <= dW.double().abs() * Pabs * (lh.U8 + 2 * lh.gamma(r + 1))).all())
