"""LoRA without a device: the float64 references (tests/lora_reference.py) proven against autograd, target selection on the model
specs, every refusal of lora.attach / the adapter file / the state builders, the library's new exports and their argument checks, and the
exactness of the integer cases the GPU file (tests/test_gpu_lora_kernels.py) relies on."""
import ctypes

import pytest
import torch

from oracle import nets as onets
from stable_diffusion_training_amd import _lib, lora, nets
from stable_diffusion_training_amd.params import ParamStore
from tests import kernel_checks as kc
from tests import lora_reference as lr


# ------------------------------------------------------------------------------------------------ reference maths
@pytest.mark.parametrize("K,N,r,s", [(8, 8, 4, 2.0), (40, 72, 4, 0.5), (48, 64, 8, 1.0), (136, 72, 64, 0.25)])
def test_projection_reference_is_the_autograd_gradient(K, N, r, s):
    """d/dA, d/dB of f(W0 + s * A @ B) for a random linear f(W) = <G, W>, float64: the projections of dW = G."""
    g = torch.Generator().manual_seed(K + N + r)
    W0 = torch.randn(K, N, generator=g, dtype=torch.float64)
    # factors that bf16 holds exactly, so that the reference's rounding of A and B is the identity and autograd sees the same function
    A = torch.randn(K, r, generator=g).to(torch.bfloat16).double().requires_grad_(True)
    B = torch.randn(r, N, generator=g).to(torch.bfloat16).double().requires_grad_(True)
    G = torch.randn(K, N, generator=g).to(torch.bfloat16).double()
    W = W0 + s * A @ B
    assert torch.allclose(W.detach(), lr.merge_ref64(W0, A.detach(), B.detach(), s), rtol=1e-12, atol=0)
    (G * W).sum().backward()
    dA, dB = lr.project_ref64(G, A.detach(), B.detach(), s)
    assert torch.allclose(dA, A.grad, rtol=1e-12, atol=1e-300) and torch.allclose(dB, B.grad, rtol=1e-12, atol=1e-300)


def test_reference_rounds_the_factors_to_bf16():
    A = torch.tensor([[1.0 + 2.0 ** -9]])  # not a bf16 value: RNE takes it to 1.0
    B = torch.tensor([[3.0]])
    assert lr.merge_ref64(torch.zeros(1, 1), A, B, 1.0).item() == 3.0
    dA, dB = lr.project_ref64(torch.tensor([[2.0]]), A, B, 0.5)
    assert dA.item() == 3.0 and dB.item() == 1.0


# ------------------------------------------------------------------------------------------------ target selection
@pytest.mark.parametrize("size", ["tiny", "sd15", "sdxl"])
def test_unet_targets_are_the_attention_projections(size):
    spec = nets.unet_spec(onets.unet_config(size))
    got = lora.select_leaves(spec, lora.LoraConfig(rank=16, alpha=16))
    blocks = sum(1 for p, _ in spec if p.endswith("/norm3/scale"))  # one per transformer block
    assert blocks > 0 and len(got) == 8 * blocks
    want = [p for p, _ in spec if p.endswith("/kernel") and len(p.split("/")) > 3 and p.split("/")[-3] in ("attn1", "attn2")
            and p.split("/")[-2] in ("to_q", "to_k", "to_v", "to_out_0")]
    assert got == want
    aspec = lora.adapter_spec(spec, lora.LoraConfig(rank=16, alpha=16))
    shapes = dict(spec)
    assert len(aspec) == 2 * len(got)
    for p in got:
        K, N = shapes[p]
        assert (p[:-len("kernel")] + "lora_a", (K, 16)) in aspec and (p[:-len("kernel")] + "lora_b", (16, N)) in aspec


def test_clip_targets_are_the_attention_projections():
    cfg = onets.clip_config("clip_l")
    spec = nets.clip_text_spec(cfg)
    got = lora.select_leaves(spec, lora.LoraConfig(rank=8, alpha=8, targets=lora.CLIP_TARGETS))
    assert len(got) == 4 * cfg["num_hidden_layers"] == 4 * sum(1 for p, _ in spec if p.endswith("/layer_norm1/scale"))
    assert all(p.split("/")[-3] == "self_attn" and p.split("/")[-2] in lora.CLIP_TARGETS for p in got)


def _tiny_base(trainable=False):
    spec = nets.unet_spec(onets.unet_config("tiny"))
    st = ParamStore(spec, device="cpu", trainable=trainable, quantise=False)
    st.load(onets.init_params(onets.unet_param_shapes(onets.unet_config("tiny")), 1))
    return st


def test_scratch_holds_every_merged_group_of_an_adapted_leaf_at_the_masters_distances():
    """Only to_v adapted: the merged q|k|v and to_k|to_v launches still write their whole groups, at the masters' relative offsets -
    so the view of a whole group must exist, be as long as the group, and hold the adapted leaf at its distance from the group's start."""
    base = _tiny_base()
    ad = lora.attach(base, lora.LoraConfig(rank=4, alpha=4, targets=("to_v",)))
    groups = 0
    for p in ad.paths:
        lf = base.leaves[p]
        assert ad.scratch_view(lf.offset, lf.offset + lf.numel).numel() == lf.numel
        qkv = tuple(p.replace("/to_v/", f"/{n}/") for n in ("to_q", "to_k", "to_v"))
        for group in (qkv, qkv[1:]):
            if base.mergeable(group):
                groups += 1
                first = base.leaves[group[0]]
                whole = ad.scratch_view(first.offset, lf.offset + lf.numel)
                assert whole.numel() == lf.offset + lf.numel - first.offset
                assert whole[lf.offset - first.offset:].data_ptr() == ad.scratch_view(lf.offset, lf.offset + lf.numel).data_ptr()
    assert groups > 0
    # disjoint slots: no two runs overlap in the scratch, and the scratch is exactly their sum
    spans = sorted((b, b + e - s) for s, e, b in ad.runs)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])) and spans[-1][1] <= ad.scratch.numel()
    assert all(s % 8 == 0 and b % 8 == 0 for s, e, b in ad.runs)
    first = ad.runs[0][0]
    with pytest.raises(_lib.SdtError):
        ad.scratch_view(first - 8, first)
    with pytest.raises(_lib.SdtError):
        ad.scratch_view(ad.runs[0][1] - 8, ad.runs[0][1] + 8)
    # every leaf adapted in its group: the scratch is as large as the adapted leaves, no larger
    full = lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=4))
    assert full.scratch.numel() == sum(full.base.leaves[p].numel for p in full.paths)


def test_attach_builds_the_adapter_store_and_initialises_it():
    base = _tiny_base()
    cfg = lora.LoraConfig(rank=8, alpha=4, seed=3)
    ad = lora.attach(base, cfg)
    assert base.adapter is ad and ad.store.trainable and cfg.scale == 0.5
    assert ad.store.order == [q for p in ad.paths for q in ad.adapted[p]]  # the base's forward order
    for p in ad.paths:
        a, b = ad.adapted[p]
        K, N = base.leaves[p].shape
        assert ad.store.leaves[a].shape == (K, 8) and ad.store.leaves[b].shape == (8, N)
        A = ad.store.p(a)
        assert float(A.abs().max()) <= K ** -0.5 and float(A.abs().max()) > 0 and not bool(ad.store.p(b).any())
    again = lora.attach(_tiny_base(), cfg)
    assert torch.equal(again.store.master, ad.store.master)
    other = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, seed=4))
    assert not torch.equal(other.store.master, ad.store.master)
    for i, p in enumerate(ad.paths):  # the job table names the leaves
        j, lf = ad.jobs_host[i], base.leaves[p]
        assert (j.w0_off, j.w_off, j.f_off, j.dw_off) == (lf.offset, lf.w_off, lf.offset, ad.scratch_offset(lf.offset, lf.offset + lf.numel))
        assert (j.K, j.N, j.r, j.scale) == (lf.shape[0], lf.shape[1], 8, 0.5)
        assert (j.a_off, j.ga_off) == (ad.store.leaves[ad.adapted[p][0]].offset,) * 2


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(ValueError, match="rank"):
        lora.LoraConfig(rank=12, alpha=1)
    with pytest.raises(ValueError, match="rank"):
        lora.LoraConfig(rank=256, alpha=1)
    with pytest.raises(ValueError, match="targets"):
        lora.LoraConfig(rank=4, alpha=1, targets=())
    with pytest.raises(ValueError, match="frozen"):
        lora.attach(_tiny_base(trainable=True), lora.LoraConfig(rank=4, alpha=1))
    with pytest.raises(ValueError, match="not a Dense kernel"):  # a convolution
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("conv1",)))
    sd15 = nets.unet_spec(onets.unet_config("sd15"))
    with pytest.raises(ValueError, match="not a Dense kernel"):  # SD1.5's 1x1-conv proj_in
        lora.select_leaves(sd15, lora.LoraConfig(rank=4, alpha=1, targets=("proj_in",)))
    with pytest.raises(ValueError, match="no Dense kernel"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=1, targets=("q_proj",)))
    with pytest.raises(ValueError, match="padded"):
        lora.select_leaves([("x/to_q/kernel", (12, 64))], lora.LoraConfig(rank=4, alpha=1))
    padded = ParamStore([("x/to_q/kernel", (12, 64))], device="cpu", trainable=False)
    with pytest.raises(ValueError, match="padded"):
        lora.attach(padded, lora.LoraConfig(rank=4, alpha=1))
    base = _tiny_base()
    lora.attach(base, lora.LoraConfig(rank=4, alpha=1))
    with pytest.raises(ValueError, match="already"):
        lora.attach(base, lora.LoraConfig(rank=4, alpha=1))
    with pytest.raises(ValueError, match="LoraConfig"):
        lora.attach(_tiny_base(), dict(rank=4))


def test_state_builder_refuses_mixed_modes_and_bad_lora_arguments():
    from stable_diffusion_training_amd import training_utils as tu
    cfg = lora.LoraConfig(rank=4, alpha=4)
    for bad in (dict(unet=None, text_encoder=lora.LoraConfig(rank=4, alpha=4, targets=lora.CLIP_TARGETS)),  # full UNet + LoRA text encoder
                dict(text_encoder="frozen"), dict(unet=cfg, text_encoder="trained"), dict(unet=cfg, vae=None), "rank16"):
        with pytest.raises(ValueError, match="lora"):
            tu.create_lion_optimizer_states({}, lora=bad, device="cpu")
    with pytest.raises(ValueError, match="lora"):
        tu.create_lion_optimizer_states({}, lora=dict(unet=cfg), train_text_encoder=False, device="cpu")


def test_train_step_refuses_a_reducer_and_mixed_states():
    from stable_diffusion_training_amd import training_utils as tu
    base = _tiny_base()
    ad = lora.attach(base, lora.LoraConfig(rank=4, alpha=4))
    us = tu.TrainState(nets.unet_forward, base, onets.unet_config("tiny"), {}, ad)
    frozen_te = tu.TrainState(None, ParamStore([("a/kernel", (8, 8))], device="cpu", trainable=False), {}, {})
    assert us.opt_store is ad.store and frozen_te.opt_store is None and us.step == 0
    sched = tu.FrozenModel(call=None, params=None)
    with pytest.raises(ValueError, match="GradReducer over the adapter stores"):
        tu.train_step(us, frozen_te, None, None, {}, None, None, sched, reducer=object())
    trained_te = tu.TrainState(None, ParamStore([("a/kernel", (8, 8))], device="cpu", trainable=False), {}, {})
    trained_te.store.trainable = True
    with pytest.raises(ValueError, match="mixed modes"):
        tu.train_step(us, trained_te, None, None, {}, None, None, sched)


# ------------------------------------------------------------------------------------------------ adapter file
def test_adapter_file_round_trip_and_mismatches(tmp_path):
    ad = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, seed=1))
    g = torch.Generator().manual_seed(2)
    ad.store.master.copy_(torch.randn(ad.store.total, generator=g))
    path = str(tmp_path / "adapter.npz")
    ad.save(path)
    fresh = lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, seed=7))
    fresh.load(path)
    for p in ad.store.order:
        assert torch.equal(fresh.store.p(p), ad.store.p(p)), p
    with pytest.raises(ValueError, match="alpha 4.0, this adapter has alpha 16.0"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=16)).load(path)
    with pytest.raises(ValueError, match="rank 8, this adapter has rank 4"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=4, alpha=4)).load(path)
    with pytest.raises(ValueError, match="targets"):
        lora.attach(_tiny_base(), lora.LoraConfig(rank=8, alpha=4, targets=("to_q", "to_v"))).load(path)
    wide = ParamStore(nets.unet_spec(onets.unet_config("tiny", cross_attention_dim=64)), device="cpu", trainable=False)
    with pytest.raises(ValueError, match="base shapes.*attn2/to_k"):
        lora.attach(wide, lora.LoraConfig(rank=8, alpha=4)).load(path)
    import numpy as np
    np.savez(str(tmp_path / "plain.npz"), x=np.zeros(3))
    with pytest.raises(ValueError, match="not an adapter file"):
        ad.load(str(tmp_path / "plain.npz"))


# ------------------------------------------------------------------------------------------------ exports
def test_library_exports_and_argument_checks(lib):
    assert lib.sdt_abi_version() == 5
    assert hasattr(lib, "sdt_lora_merge") and hasattr(lib, "sdt_lora_project")
    assert lib.sdt_lora_job_size() == ctypes.sizeof(_lib.SdtLoraJob) == 96
    jobs, _ = lr.layout([(40, 72, 4, 1.0)])
    good = lr.job_table(jobs)
    p = 4096  # any aligned non-null address: every call below fails its checks before anything is launched

    def merge(table, host=True, dev=p, n=1, w0=p, w=p):
        return lib.sdt_lora_merge(w0, p, w, None, table if host else None, dev, n, None)

    def project(table, host=True, dev=p, n=1, dw=p):
        return lib.sdt_lora_project(dw, p, p, table if host else None, dev, n, None)

    assert merge(None, host=False, dev=None, n=0) == 0 and project(None, host=False, dev=None, n=0) == 0  # n == 0: nothing to do
    for call in (merge, project):
        assert call(good, host=False) == -1 and b"null job table" in lib.sdt_last_error()
        assert call(good, dev=None) == -1 and b"null job table" in lib.sdt_last_error()
        assert call(good, n=-1) == -1
        for field, value, msg in (("r", 12, b"rank 12"), ("r", 256, b"rank 256"), ("r", 0, b"rank 0"), ("K", 44, b"multiples of 8"),
                                  ("N", 70, b"multiples of 8"), ("K", 0, b"multiples of 8"), ("a_off", 12, b"offsets"),
                                  ("w0_off", -8, b"offsets"), ("tile0_merge", 1, b"running"), ("tile0_project", 1, b"running"),
                                  ("tiles_da", 2, b"running")):
            if (call is merge and field == "tile0_project") or (call is project and field == "tile0_merge"):
                continue
            bad = lr.job_table(jobs)
            setattr(bad[0], field, value)
            assert call(bad) == -1, field
            assert msg in lib.sdt_last_error(), (field, lib.sdt_last_error())
    assert merge(good, w0=None) == -1 and b"null pointer" in lib.sdt_last_error()
    assert merge(good, w=None) == -1 and b"no destination" in lib.sdt_last_error()
    assert merge(good, w=p + 2) == -1 and b"aligned" in lib.sdt_last_error()
    assert project(good, dw=None) == -1 and b"null pointer" in lib.sdt_last_error()


# ------------------------------------------------------------------------------------------------ exactness of the GPU cases
def test_every_integer_case_is_exact_in_fp32():
    """For every (K, N, r) x scale of the GPU table the largest partial sum, in units of the terms' common denominator, is an integer
    below 2^24: fp32 accumulation is exact in any order and the expectation is unique.  Checked by the bound and on the operands."""
    n = 0
    for i, (K, N, r) in enumerate(lr.CASES):
        for s in lr.SCALES:
            for what, bound, limit in lr.exact_bounds(K, N, r, s):
                assert bound < limit, what
                n += 1
        W0, A, B, dW = lr.exact_operands(K, N, r, 100 + i)
        assert float(W0.abs().max()) <= 128 and torch.equal(W0 * 8, (W0 * 8).round())
        for t in (A, B, dW.float()):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        s = lr.SCALES[i % 3]
        v = lr.merge_ref64(W0, A, B, s)
        dA, dB = lr.project_ref64(dW, A, B, s)
        for x in (v, dA, dB):
            assert torch.equal(x.float().double(), x)
        # worst partial sums: sum of |terms|
        assert float((W0.double().abs() + s * (A.double().abs() @ B.double().abs())).max()) * 8 < kc.LIMIT
        assert float((dW.double().abs() @ B.double().abs().T).max()) * s * 2 < kc.LIMIT
    assert n == 3 * len(lr.CASES) * len(lr.SCALES)
    # the big case rounds: ties and inexact values both occur, so the RNE expectation is a real check
    W0, A, B, _ = lr.exact_operands(640, 1280, 128, 106)
    v = lr.merge_ref64(W0, A, B, 0.5)
    low = (v.float().view(torch.int32) & 0xFFFF)
    assert bool((low == 0x8000).any()) and bool(((low != 0) & (low != 0x8000)).any())
