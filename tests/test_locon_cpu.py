"""LoCon without a device (DESIGN.md "LoCon"): the weight-space form proven against the two-convolution form of kohya / LyCORIS in
float64, selection on the model specs, conv_rank=0 left as it was, every refusal, the scratch layout, the new exports and their host
checks (they return before any HIP call), and the exactness of the integer cases of tests/test_gpu_locon_kernels.py."""
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
from tests import lora_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the form is LoCon
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1)], ids=["3x3", "3x3-stride2", "1x1"])
def test_the_weight_space_delta_is_a_down_convolution_and_a_1x1_up_convolution(k, stride):
    Cin, Cout, r, s = 8, 16, 4, 0.75
    g = torch.Generator().manual_seed(10 * k + stride)
    x = torch.randn(2, Cin, 9, 10, generator=g, dtype=torch.float64)
    W0 = torch.randn(k, k, Cin, Cout, generator=g, dtype=torch.float64)
    # factors that bf16 holds exactly: the reference's rounding of A and B is then the identity and autograd sees the same function
    A = torch.randn(k * k * Cin, r, generator=g).to(torch.bfloat16).double().requires_grad_(True)
    B = torch.randn(r, Cout, generator=g).to(torch.bfloat16).double().requires_grad_(True)
    merged, split = lc.locon_forward64(x, W0, A, B, s, stride)
    assert merged.shape == split.shape and torch.allclose(merged, split, rtol=1e-12, atol=1e-12 * float(merged.detach().abs().max()))
    # the projection of the flattened conv weight gradient is autograd's gradient of both factors
    G = torch.randn(merged.shape, generator=g, dtype=torch.float64)
    (G * split).sum().backward()
    W = (W0 + s * (A.detach() @ B.detach()).view(k, k, Cin, Cout)).requires_grad_(True)
    out = torch.nn.functional.conv2d(x, W.permute(3, 2, 0, 1), stride=stride, padding=k // 2)
    (dW,) = torch.autograd.grad((G * out).sum(), W)
    dA, dB = lr.project_ref64(dW.reshape(k * k * Cin, Cout), A.detach(), B.detach(), s)
    assert torch.allclose(dA, A.grad, rtol=1e-10, atol=1e-12) and torch.allclose(dB, B.grad, rtol=1e-10, atol=1e-12)
    assert float(A.grad.abs().max()) > 0 and float(B.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("size", ["tiny", "sd15", "sd21", "sdxl"])
def test_selection_on_the_model_specs(size):
    spec = nets.unet_spec(onets.unet_config(size))
    shapes = dict((p, tuple(s)) for p, s in spec)
    cfg = lora.LoraConfig(rank=16, alpha=16, conv_rank=8, conv_alpha=4)
    got = lora.select_leaves(spec, cfg)
    convs = lc.conv_leaves(spec, lora.UNET_CONV_TARGETS)
    dense = lora.select_leaves(spec, lora.LoraConfig(rank=16, alpha=16))
    assert convs and set(got) == set(convs) | set(dense) and len(got) == len(convs) + len(dense)
    order = [p for p, _ in spec]
    assert got == sorted(got, key=order.index), "forward order of the base"
    assert any(p.endswith("/conv1/kernel") for p in convs) and any("/downsamplers_0/conv/" in p for p in convs)
    assert any("/upsamplers_0/conv/" in p for p in convs) and any(p.endswith("/conv_shortcut/kernel") for p in convs)
    assert not any(p.startswith("conv_in/") or p.startswith("conv_out/") for p in got)
    proj_in = [p for p in order if p.endswith("/proj_in/kernel")]
    assert proj_in
    if size in ("tiny", "sd15"):  # a 1x1 convolution: adapted as one
        assert all(len(shapes[p]) == 4 and p in convs for p in proj_in)
    else:  # a Dense layer: the conv targets skip it, and `targets` did not name it
        assert all(len(shapes[p]) == 2 and p not in got for p in proj_in)
        with_proj = lora.select_leaves(spec, lora.LoraConfig(rank=16, alpha=16, targets=lora.UNET_TARGETS + ("proj_in",), conv_rank=8))
        assert all(p in with_proj for p in proj_in)
    aspec = lora.adapter_spec(spec, cfg)
    assert [p for p, _ in aspec] == [p[:-len("kernel")] + n for p in got for n in ("lora_a", "lora_b")]
    ashapes = dict(aspec)
    for p in got:
        stem = p[:-len("kernel")]
        if len(shapes[p]) == 4:
            kh, kw, ci, co = shapes[p]
            assert ashapes[stem + "lora_a"] == (kh * kw * ci, 8) and ashapes[stem + "lora_b"] == (8, co)
        else:
            assert ashapes[stem + "lora_a"] == (shapes[p][0], 16) and ashapes[stem + "lora_b"] == (16, shapes[p][1])
    assert cfg.scale == 1.0 and cfg.conv_scale == 0.5 and lora.LoraConfig(4, 4, conv_rank=8).conv_scale == 1.0


def _tiny_base(trainable=False, **kw):
    spec = nets.unet_spec(onets.unet_config("tiny", **kw))
    st = ParamStore(spec, device="cpu", trainable=trainable, quantise=False)
    st.load(onets.init_params(onets.unet_param_shapes(onets.unet_config("tiny", **kw)), 1))
    return st


def test_attach_orders_and_initialises_the_conv_adapters():
    base = _tiny_base()
    cfg = lora.LoraConfig(rank=8, alpha=4, seed=3, conv_rank=4, conv_alpha=2)
    ad = lora.attach(base, cfg)
    assert ad.paths == lora.select_leaves([(p, base.leaves[p].shape) for p in base.order], cfg)
    assert ad.store.order == [q for p in ad.paths for q in ad.adapted[p]]
    assert ad.conv_paths == lc.conv_leaves([(p, base.leaves[p].shape) for p in base.order], lora.UNET_CONV_TARGETS)
    assert ad.dense_paths + ad.conv_paths != ad.paths, "the tiny UNet interleaves Dense and convolution adapters"
    g = torch.Generator().manual_seed(3)  # one generator, leaf order, Dense and convolution leaves alike
    for p in ad.paths:
        a, b = ad.adapted[p]
        K, r = ad.store.leaves[a].shape
        assert torch.equal(ad.store.p(a), (torch.rand(K, r, generator=g) * 2 - 1) / K ** 0.5) and not bool(ad.store.p(b).any())
    rows = lc.rows()
    tm = tp = ts = cnt = part = 0
    for i, p in enumerate(ad.conv_paths):
        j, x, lf = ad.conv_jobs_host[i], ad.split_host[i], base.leaves[p]
        kh, kw, ci, co = lf.shape
        assert (j.K, j.N, j.r, j.scale) == (kh * kw * ci, co, 4, 0.5)
        assert (j.w0_off, j.w_off, j.f_off, j.dw_off) == (lf.offset, lf.w_off, lf.offset, ad.scratch_offset(lf.offset, lf.offset + lf.numel))
        assert (j.a_off, j.ga_off, j.b_off, j.gb_off) == (ad.store.leaves[ad.adapted[p][0]].offset,) * 2 + (ad.store.leaves[ad.adapted[p][1]].offset,) * 2
        ta, tb, ch = (j.K + 63) // 64, (j.N + 63) // 64, (j.K + rows - 1) // rows
        assert (j.tile0_merge, j.tile0_project, j.tiles_da) == (tm, tp, ta)
        assert (x.K, x.N, x.tile0, x.chunks, x.cnt0, x.part_off) == (j.K, j.N, ts, ch, cnt, part)
        tm, tp, ts, cnt = tm + ta * tb, tp + ta + tb, ts + ta + tb * ch, cnt + tb
        part += tb * ch * j.r * 64 if ch > 1 else 0
    assert max(j.K for j in ad.conv_jobs_host) == 9 * 128 and part > 0, "the tiny UNet reaches a convolution of more than one chunk"
    assert ad.split_ws.numel() == (4 * cnt + 255) // 256 * 256 + 4 * part and not bool(ad.split_ws.any())
    assert len(ad.jobs_host) == len(ad.dense_paths)


# ------------------------------------------------------------------------------------------------ conv_rank = 0
def test_conv_rank_zero_changes_nothing(tmp_path):
    spec = nets.unet_spec(onets.unet_config("tiny"))
    old, new = lora.LoraConfig(rank=8, alpha=4, seed=1), lora.LoraConfig(rank=8, alpha=4, seed=1, conv_rank=0, conv_alpha=3.0, conv_targets=("conv1",))
    assert lora.select_leaves(spec, old) == lora.select_leaves(spec, new) and lora.adapter_spec(spec, old) == lora.adapter_spec(spec, new)
    assert all(len(dict(spec)[p]) == 2 for p in lora.select_leaves(spec, new))
    a, b = lora.attach(_tiny_base(), old), lora.attach(_tiny_base(), new)
    assert bytes(a.jobs_host) == bytes(b.jobs_host) and a.scratch.numel() == b.scratch.numel() and a.runs == b.runs
    assert b.conv_paths == [] and b.conv_jobs_host is None and b.split_ws is None
    assert a.scratch.numel() == sum(a.base.leaves[p].numel for p in a.paths)
    metas = []
    for ad, name in ((a, "a.npz"), (b, "b.npz")):
        ad.save(str(tmp_path / name))
        with np.load(str(tmp_path / name)) as z:
            metas.append(bytes(z["__meta__"]))
            assert sorted(z.files) == sorted(["__meta__"] + ad.store.order)
    assert metas[0] == metas[1] and sorted(json.loads(metas[0])) == ["alpha", "base_shapes", "rank", "targets"]
    with pytest.raises(ValueError, match="not a Dense kernel"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("conv1",)))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    for bad in (12, 256, -4, True, 2):
        with pytest.raises(ValueError, match="conv_rank"):
            lora.LoraConfig(rank=4, alpha=1, conv_rank=bad)
    with pytest.raises(ValueError, match="conv_alpha"):
        lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_alpha=float("nan"))
    with pytest.raises(ValueError, match="conv_targets"):
        lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_targets=())
    with pytest.raises(ValueError, match="DoRA on convolutions is not supported"):
        lora.LoraConfig(rank=4, alpha=1, dora=True, conv_rank=4)
    spec = nets.unet_spec(onets.unet_config("sd21"))
    with pytest.raises(ValueError, match="no convolution kernel matches"):  # SD2.1's proj_in / proj_out are Dense: skipped, nothing left
        lora.select_leaves(spec, lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_targets=("proj_in", "proj_out")))
    with pytest.raises(ValueError, match="no convolution kernel matches"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_targets=("nothing",)))
    with pytest.raises(ValueError, match="padded"):  # 4 input channels: a zero-padded mirror
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_targets=("conv_in",)))
    with pytest.raises(ValueError, match="padded"):
        lora.select_leaves([("a/to_q/kernel", (8, 8)), ("emb/conv_in/kernel", (3, 3, 3, 16))],
                           lora.LoraConfig(rank=4, alpha=1, conv_rank=4, conv_targets=("conv_in",)))
    with pytest.raises(ValueError, match="not a Dense kernel"):  # `targets` still means Dense kernels
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("conv1",), conv_rank=4))
    with pytest.raises(ValueError, match="no Dense kernel"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("q_proj",), conv_rank=4))


def test_adapter_file_names_a_mismatch_in_the_conv_fields(tmp_path):
    cfg = dict(rank=8, alpha=4, conv_rank=4, conv_alpha=2)
    ad = lora.attach(_tiny_base(), lora.LoraConfig(seed=1, **cfg))
    ad.store.master.copy_(torch.randn(ad.store.total, generator=torch.Generator().manual_seed(2)))
    path = str(tmp_path / "locon.npz")
    ad.save(path)
    with np.load(path) as z:
        meta = json.loads(bytes(z["__meta__"]).decode())
    assert (meta["conv_rank"], meta["conv_alpha"], meta["conv_targets"]) == (4, 2.0, list(lora.UNET_CONV_TARGETS))
    assert any(len(s) == 4 for s in meta["base_shapes"].values())
    fresh = lora.attach(_tiny_base(), lora.LoraConfig(seed=9, **cfg))
    fresh.load(path)
    for p in ad.store.order:
        assert torch.equal(fresh.store.p(p), ad.store.p(p)), p
    with pytest.raises(ValueError, match="conv_rank 4, this adapter has conv_rank 8"):
        lora.attach(_tiny_base(), lora.LoraConfig(**dict(cfg, conv_rank=8))).load(path)
    with pytest.raises(ValueError, match="conv_rank 4, this adapter has conv_rank 0"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4)).load(path)
    with pytest.raises(ValueError, match="conv_alpha 2.0, this adapter has conv_alpha 4.0"):
        lora.attach(_tiny_base(), lora.LoraConfig(**dict(cfg, conv_alpha=None))).load(path)
    with pytest.raises(ValueError, match="conv_targets"):
        lora.attach(_tiny_base(), lora.LoraConfig(conv_targets=("conv1", "conv2"), **cfg)).load(path)
    plain = str(tmp_path / "plain.npz")
    lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4)).save(plain)
    with pytest.raises(ValueError, match="conv_rank 0, this adapter has conv_rank 4"):
        fresh.load(plain)


def _example():
    spec = importlib.util.spec_from_file_location("train_synthetic_example", os.path.join(ROOT, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_refuses_lora_conv_without_lora_and_with_dora():
    ex = _example()
    with pytest.raises(ValueError, match="lora_conv_rank.*give lora_rank"):
        ex.lora_config({"lora_conv_rank": 4})
    with pytest.raises(ValueError, match="lora_conv_alpha needs lora_conv_rank"):
        ex.lora_config({"lora_rank": 4, "lora_conv_alpha": 2.0})
    with pytest.raises(ValueError, match="DoRA on convolutions is not supported"):
        ex.lora_config({"lora_rank": 4, "lora_dora": True, "lora_conv_rank": 4})
    cfg = ex.lora_config({"lora_rank": 8, "lora_conv_rank": 4, "lora_conv_alpha": 2.0})["unet"]
    assert (cfg.rank, cfg.alpha, cfg.conv_rank, cfg.conv_alpha, cfg.conv_scale) == (8, 8.0, 4, 2.0, 0.5)
    assert ex.lora_config({"lora_rank": 8})["unet"] == lora.LoraConfig(8, 8.0) and ex.lora_config({}) is None
    # the command line: refused by the parser, before the configuration file is opened
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_synthetic.py"), "/nonexistent.json", "--lora-conv", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--lora-conv needs --lora RANK" in r.stderr


# ------------------------------------------------------------------------------------------------ scratch
def test_every_adapted_conv_leaf_has_a_scratch_slot_of_its_own():
    base = _tiny_base()
    ad = lora.attach(base, lora.LoraConfig(rank=4, alpha=4, conv_rank=4))
    spans = sorted((b, b + e - s) for s, e, b in ad.runs)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])) and spans[-1][1] <= ad.scratch.numel()
    assert all(s % 8 == 0 and b % 8 == 0 for s, e, b in ad.runs)
    assert [s for s, e, b in ad.runs] == sorted(s for s, e, b in ad.runs)
    ptrs = set()
    for p in ad.conv_paths:
        lf = base.leaves[p]
        v = ad.scratch_view(lf.offset, lf.offset + lf.numel)
        assert v.numel() == lf.numel and (lf.offset, lf.offset + lf.numel) in [(s, e) for s, e, b in ad.runs], p
        ptrs.add(v.data_ptr())
    assert len(ptrs) == len(ad.conv_paths)
    # every member of every group adapted: the scratch is as large as the adapted leaves (rounded to 8 elements per run), no larger
    assert ad.scratch.numel() == sum(base.leaves[p].numel for p in ad.paths)
    # only convolutions of one kind adapted beside to_v: the Dense groups are laid out as without LoCon
    part = lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=4, targets=("to_v",), conv_rank=4, conv_targets=("conv_shortcut",)))
    only = lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=4, targets=("to_v",)))
    assert [(s, e) for s, e, b in part.runs if (s, e) in [(x, y) for x, y, _ in only.runs]] == [(s, e) for s, e, b in only.runs]
    assert part.scratch.numel() == only.scratch.numel() + sum(part.base.leaves[p].numel for p in part.conv_paths)


# ------------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_bound_and_exported(lib):
    with open(os.path.join(ROOT, "include", "sdt.h")) as f:
        header = f.read()
    for name in ("sdt_lora_project_split", "sdt_lora_project_split_workspace_bytes", "sdt_lora_project_split_rows", "sdt_lora_split_job_size"):
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/sdt.h"
        assert name in _lib.SIGNATURES or name in _lib.WS_QUERY or name in _lib.NOARG, f"{name} is not bound in _lib.py"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.sdt_abi_version() == 5
    assert lib.sdt_lora_job_size() == ctypes.sizeof(_lib.SdtLoraJob) == 96
    assert lib.sdt_lora_split_job_size() == ctypes.sizeof(_lib.SdtLoraSplitJob) == 32
    C = lib.sdt_lora_project_split_rows()
    assert C > 0 and C % 32 == 0 and C == lc.rows()


def test_host_checks_return_before_any_hip_call(lib):
    C = lc.rows()
    cases = [(C + 8, 72, 16, 1.0), (72, 8, 4, 0.5), (2 * C + 40, 192, 32, 2.0)]
    jobs, _ = lr.layout(cases)
    good = lr.job_table(jobs)
    split, counter_bytes, total = lc.split_table(jobs, C)
    assert counter_bytes == 256 and total == 256 + 4 * 64 * (2 * 2 * 16 + 3 * 3 * 32)
    assert lib.sdt_lora_project_split_workspace_bytes(good, 3) == total
    assert lib.sdt_lora_project_split_workspace_bytes(good, 0) == 0 and lib.sdt_lora_project_split_workspace_bytes(None, 0) == 0
    assert lib.sdt_lora_project_split_workspace_bytes(None, 1) == -1 and lib.sdt_lora_project_split_workspace_bytes(good, -1) == -1
    bad = lr.job_table(jobs)
    bad[1].r = 12
    assert lib.sdt_lora_project_split_workspace_bytes(bad, 3) == -1 and b"rank 12" in lib.sdt_last_error()
    p = 4096  # any aligned non-null address: every call below fails its checks before anything is launched

    def call(table=good, sp=split, host=True, sphost=True, dev=p, spdev=p, n=3, dw=p, ws=p, nbytes=total):
        return lib.sdt_lora_project_split(dw, p, p, table if host else None, sp if sphost else None, dev, spdev, n, ws, nbytes, None)

    assert call(host=False, sphost=False, dev=None, spdev=None, n=0, dw=None, ws=None, nbytes=0) == 0  # n == 0: nothing to do
    for kw in (dict(host=False), dict(sphost=False), dict(dev=None), dict(spdev=None)):
        assert call(**kw) == -1 and b"null job table" in lib.sdt_last_error(), kw
    assert call(n=-1) == -1 and b"negative" in lib.sdt_last_error()
    assert call(dw=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert call(ws=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert call(ws=p + 4) == -1 and b"aligned" in lib.sdt_last_error()
    assert call(nbytes=total - 4) == -1 and b"workspace" in lib.sdt_last_error()
    # sdt_lora_merge's checks on the job table
    for field, value, msg in (("r", 12, b"rank 12"), ("r", 0, b"rank 0"), ("K", 44, b"multiples of 8"), ("N", 70, b"multiples of 8"),
                              ("K", 0, b"multiples of 8"), ("a_off", 12, b"offsets"), ("dw_off", -8, b"offsets"),
                              ("tile0_project", 1, b"running"), ("tiles_da", 2, b"running")):
        bad = lr.job_table(jobs)
        setattr(bad[0], field, value)
        assert call(table=bad) == -1, field
        assert msg in lib.sdt_last_error(), (field, lib.sdt_last_error())
    # the split table: mismatched tables, the chunk count, running counts, partial offsets
    for i, field, value, msg in ((0, "K", C, b"mismatched tables"), (2, "N", 64, b"mismatched tables"), (0, "chunks", 1, b"chunks"),
                                 (1, "chunks", 2, b"chunks"), (1, "tile0", 0, b"running"), (2, "tile0", 1 << 20, b"running"),
                                 (1, "cnt0", 0, b"running"), (2, "cnt0", 64, b"running"), (0, "part_off", 64, b"partial offset"),
                                 (2, "part_off", 0, b"partial offset"), (2, "part_off", total, b"partial offset")):
        bad, _, _ = lc.split_table(jobs, C)
        setattr(bad[i], field, value)
        assert call(sp=bad) == -1, (i, field)
        assert msg in lib.sdt_last_error(), (i, field, lib.sdt_last_error())


# ------------------------------------------------------------------------------------------------ exactness of the GPU cases
def test_every_integer_case_is_exact_in_fp32():
    """lora_reference.exact_bounds per (K, N, r) x scale of the GPU table - the largest partial sum in units of the terms' common
    denominator is an integer below 2^24, in ANY order, so chunk sums and their sum are exact too - and the same on the operands."""
    C = lc.rows()
    table = lc.cases(C)
    assert len(table) == 7 and [lc.chunks(K, C) for K, N, r in table] == [1, 1, 1, 2, 3, lc.chunks(576, C), 4]
    n = 0
    for i, (K, N, r) in enumerate(table):
        assert K % 8 == 0 and N % 8 == 0 and r in lora.RANKS
        for s in lc.SCALES:
            for what, bound, limit in lr.exact_bounds(K, N, r, s):
                assert bound < limit, what
                n += 1
        W0, A, B, dW = lr.exact_operands(K, N, r, 100 + i)
        s = lc.SCALES[i % 3]
        v = lr.merge_ref64(W0, A, B, s)
        dA, dB = lr.project_ref64(dW, A, B, s)
        for x in (v, dA, dB):
            assert torch.equal(x.float().double(), x)
        assert float((W0.double().abs() + s * (A.double().abs() @ B.double().abs())).max()) * 8 < kc.LIMIT
        assert float((dW.double().abs() @ B.double().abs().T).max()) * s * 2 < kc.LIMIT
        assert float((A.double().abs().T @ dW.double().abs()).max()) * s * 2 < kc.LIMIT
    assert n == 3 * len(table) * len(lc.SCALES)
    for K, N, r in lc.random_cases(C):
        assert lc.chunks(K, C) > 1 and lc.db_roundings(K, C) == C + lc.chunks(K, C) - 1
