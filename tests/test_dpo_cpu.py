"""Diffusion-DPO without a GPU (include/sdt.h "DPO LOSS"): the reference's gradient against torch autograd, the stable forms of
-logsigmoid and sigmoid at huge logits, the exports and their bindings, the host refusals of both entry points (they return before any
HIP call) and the refusals of train_step(dpo_beta=) that are raised before the step touches a device."""
import math
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

from tests import dpo_reference as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(P, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    B = 2 * P
    pred = torch.randn(B, h, w, C, generator=g, dtype=torch.float64)
    ref = pred + 0.3 * torch.randn(B, h, w, C, generator=g, dtype=torch.float64)
    target = torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    return pred, ref, target


@pytest.mark.parametrize("beta", [0.5, 7.0, 5000.0])
def test_autograd_through_the_loss_gives_the_closed_form_gradient(beta):
    """d(mean over pairs of -logsigmoid(z)) / d pred = coef_b * (target - pred) / (P*C*h*w) with coef = -+beta * sigmoid(-z): float64
    autograd through the reference's own loss agrees to 1e-12 relative, and so do the values."""
    pred, ref, target = _case(3, 4, 5, 6, 3)
    pred.requires_grad_(True)
    loss = dref.loss_torch(pred, ref, target, beta)
    loss.backward()
    want = dref.reference(pred.detach().numpy(), ref.numpy(), target.numpy(), beta)
    assert abs(loss.item() - want["loss"]) <= 1e-12 * max(want["loss"], 1e-300)
    g, w = pred.grad.numpy(), want["dpred"]
    assert np.abs(w).max() > 0 or beta == 5000.0
    assert np.abs(g - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300)
    # the two samples of a pair pull in opposite directions with one weight
    assert np.array_equal(want["coef"][0::2], -want["coef"][1::2]) and (want["coef"][1::2] >= 0).all()


def test_stable_forms_are_finite_up_to_logits_of_a_million():
    z = np.array([-1e6, -800.0, -40.0, -1.0, 0.0, 1.0, 40.0, 800.0, 1e6])
    pl, s = dref.neg_logsigmoid(z), dref.sigmoid_neg(z)
    assert np.isfinite(pl).all() and np.isfinite(s).all()
    assert pl[0] == 1e6 and pl[1] == 800.0 and pl[-1] == 0.0 and pl[-2] == 0.0 and pl[4] == math.log(2.0)
    assert s[0] == 1.0 and s[1] == 1.0 and s[-1] == 0.0 and s[4] == 0.5 and ((0 <= s) & (s <= 1)).all()
    assert (np.diff(pl) <= 0).all() and (np.diff(s) <= 0).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        naive = np.log(1.0 + np.exp(-z))
    assert not np.isfinite(naive).all(), "the naive form was expected to overflow"
    mid = np.abs(z) <= 1  # (where 1 + exp(-z) loses nothing that matters: the naive form is accurate there)
    assert np.allclose(pl[mid], naive[mid], rtol=1e-12, atol=0)


def test_published_chains_follow_the_float64_reference():
    """pairs() from fp32 sample errors, loss_chain and dpred_chain reproduce reference() up to the fp32 / bf16 roundings they state."""
    pred, ref, target = _case(2, 4, 8, 8, 5)
    x, y, t = pred.float().numpy(), ref.float().numpy(), target.float().numpy()
    want = dref.reference(x, y, t, 3.0)
    n = 4 * 8 * 8
    m, r = dref.publish_mse(dref.sample_sq_sums(x, t), n), dref.publish_mse(dref.sample_sq_sums(y, t), n)
    assert np.allclose(m, want["model_mse"], rtol=1e-5) and np.allclose(r, want["ref_mse"], rtol=1e-5)
    pr = dref.pairs(m, r, 3.0)
    assert np.allclose(pr["z"], want["logits"], rtol=0, atol=1e-4) and np.allclose(pr["coef"], want["coef"], rtol=1e-4)
    assert abs(float(dref.loss_chain(pr["pair_loss"].astype(np.float32))) - want["loss"]) <= 1e-4 * want["loss"]
    dp = dref.dpred_chain(pr["coef"].astype(np.float32), x, t).double().numpy()
    assert np.abs(dp - want["dpred"]).max() <= 2.0 ** -7 * np.abs(want["dpred"]).max()


def test_exports_and_bindings(lib):
    from stable_diffusion_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sdt.h")).read()
    declared = set(re.findall(r"\b(sdt_[a-z0-9_]+)\s*\(", hdr))
    assert "DPO LOSS" in hdr
    for name in ("sdt_dpo_loss_fwd_bwd", "sdt_dpo_loss_workspace_bytes", "sdt_lora_restore"):
        assert name in declared and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["sdt_dpo_loss_fwd_bwd"]) == 18 and _lib.SIGNATURES["sdt_dpo_loss_fwd_bwd"][3] is _lib._F
    assert len(_lib.SIGNATURES["sdt_lora_restore"]) == 6 and _lib.WS_QUERY["sdt_dpo_loss_workspace_bytes"] == [_lib._I] * 3
    assert declared == set(_lib.SIGNATURES) | set(_lib.NOARG) | set(_lib.WS_QUERY)
    assert lib.sdt_abi_version() == 5  # additive exports


def test_host_refusals_without_a_gpu(lib):
    """Pointers are made-up aligned addresses: every refusal returns before anything dereferences them or calls HIP."""
    A, WS = 4096, lib.sdt_dpo_loss_workspace_bytes(4, 8, 8)
    assert WS == lib.sdt_reduce_workspace_bytes()
    err = lambda: lib.sdt_last_error()

    def loss(pred=A, ref=A, tgt=A, beta=5000.0, acc=A, mse=A, lg=A, pl=A, cf=A, dp=A, B=4, C=4, h=8, w=8, cpad=8, ws=A, wsb=WS):
        return lib.sdt_dpo_loss_fwd_bwd(pred, ref, tgt, beta, acc, mse, lg, pl, cf, dp, B, C, h, w, cpad, ws, wsb, None)

    for k in ("pred", "ref", "tgt", "acc", "mse", "lg", "pl", "cf", "dp"):
        assert loss(**{k: None}) == -1 and b"null pointer" in err(), k
    for k, off in (("pred", 1), ("ref", 1), ("dp", 1), ("tgt", 2), ("acc", 2), ("mse", 2), ("lg", 2), ("pl", 2), ("cf", 2)):
        assert loss(**{k: A + off}) == -1 and b"misaligned" in err(), k
    for B in (3, 1, 0, -2, 8194, 8193):
        assert loss(B=B) == -1 and b"must be even" in err(), B
    for kw in (dict(C=0), dict(h=0), dict(w=-1)):
        assert loss(**kw) == -1 and b"bad shape" in err(), kw
    assert loss(cpad=3) == -1 and b"cpad=3 < C=4" in err()
    for beta in (0.0, -5000.0, float("nan"), float("inf")):
        assert loss(beta=beta) == -1 and b"finite and > 0" in err(), beta
    for kw in (dict(ws=None), dict(ws=A + 8), dict(wsb=WS - 1)):
        assert loss(**kw) == -1 and b"workspace" in err(), kw
    assert lib.sdt_dpo_loss_workspace_bytes(128, 512, 512) > lib.sdt_reduce_workspace_bytes()
    assert loss(B=128, h=512, w=512) == -1 and b"workspace" in err()  # two sets of partials need more than the shared 64 KiB
    for bad in ((3, 8, 8), (0, 8, 8), (8194, 8, 8), (4, 0, 8)):
        assert lib.sdt_dpo_loss_workspace_bytes(*bad) == -1, bad

    from stable_diffusion_training_amd import _lib
    table = (_lib.SdtLoraJob * 1)(_lib.SdtLoraJob(0, 0, 64, 0, 0, 0, 0, 64, 16, 16, 4, 1.0, 0, 0, 1, 0))
    restore = lambda w0=A, w=A, t=table, d=A, n=1: lib.sdt_lora_restore(w0, w, t, d, n, None)
    assert restore(n=0) == 0 and restore(n=-1) == -1
    assert restore(w0=None) == -1 and b"null pointer" in err()
    assert restore(w=None) == -1 and b"null pointer" in err()
    assert restore(t=None) == -1 and b"null job table" in err()
    assert restore(d=None) == -1 and b"null job table" in err()
    assert restore(w0=A + 4) == -1 and b"16-byte aligned" in err()
    assert restore(w=A + 2) == -1 and b"16-byte aligned" in err()
    for kw, msg in ((dict(r=5), b"rank 5"), (dict(K=12), b"multiples of 8"), (dict(tile0_merge=2), b"running tile count"), (dict(w_off=4), b"offsets")):
        j = _lib.SdtLoraJob(0, 0, 64, 0, 0, 0, 0, 64, 16, 16, 4, 1.0, 0, 0, 1, 0)
        for k, v in kw.items():
            setattr(j, k, v)
        assert restore(t=(_lib.SdtLoraJob * 1)(j)) == -1 and msg in err(), kw


def test_synthetic_loader_emits_interleaved_pairs():
    """preference_pairs=True: samples 2i and 2i+1 are two different images under one caption; every other entry keeps the value it has
    without the option; an odd per-rank batch is refused."""
    from stable_diffusion_training_amd.streamer import DataLoader
    kw = dict(training_batch_size=4, maximum_resolution_areas=(64 ** 2,), bucket_lower_bound_resolutions=(64,), batches_per_chunk=2, seed=3)
    batches = []
    for pairs in (False, True):
        dl = DataLoader(preference_pairs=pairs, **kw)
        dl._print_debug = False
        dl.create_training_dataframe()
        dl.dispatch_worker()
        batches.append(dl.grab_next_batch())
    plain, paired = batches
    assert torch.equal(plain["pixel_values"], paired["pixel_values"]) and torch.equal(plain["input_ids"][0::2], paired["input_ids"][0::2])
    assert torch.equal(paired["input_ids"][1::2], paired["input_ids"][0::2]) and not torch.equal(plain["input_ids"][1::2], plain["input_ids"][0::2])
    assert not torch.equal(paired["pixel_values"][0], paired["pixel_values"][1])
    with pytest.raises(ValueError, match="preference_pairs"):
        DataLoader(preference_pairs=True, **dict(kw, training_batch_size=3))


# ------------------------------------------------------------------------------------------------ train_step refusals (no device)
def _fake_states(unet_adapter=True, te_adapter=False, tokens=None, side=None):
    """States with just the attributes train_step reads before it refuses a DPO configuration."""
    frozen = lambda: types.SimpleNamespace(trainable=False, device=torch.device("cpu"), adapter=None, tokens=None)
    us = types.SimpleNamespace(store=frozen(), config={"in_channels": 4, "out_channels": 4}, adapter=object() if unet_adapter else None,
                               tokens=None, controlnet=side, ip_adapter=None)
    ts = types.SimpleNamespace(store=frozen(), config={}, adapter=object() if te_adapter else None, tokens=tokens, controlnet=None,
                               ip_adapter=None)
    return us, ts


def _refused(match, us=None, ts=None, batch=None, **kw):
    from stable_diffusion_training_amd import training_utils as tu
    if us is None:
        us, ts = _fake_states()
    with pytest.raises(ValueError, match=match):
        tu.train_step(us, ts, None, None, batch if batch is not None else {}, None, None, None, **kw)


@pytest.mark.parametrize("beta", [0.0, -1.0, float("nan"), float("inf"), True, "5000"])
def test_step_refuses_a_bad_beta(beta):
    _refused("dpo_beta=.* must be a finite number > 0", dpo_beta=beta)


def test_step_refuses_what_the_preference_loss_cannot_run():
    _refused("must carry a LoRA / DoRA adapter", *_fake_states(unet_adapter=False), dpo_beta=5000.0)
    _refused("text-encoder adapter", *_fake_states(te_adapter=True), dpo_beta=5000.0)
    _refused("loss_mask", batch={"loss_mask": None}, dpo_beta=5000.0)
    _refused("loss_weight", batch={"loss_weight": None}, dpo_beta=5000.0)
    _refused('loss_type=.huber. is not supported', dpo_beta=5000.0, loss_type="huber")
    _refused("min_snr_gamma_magnitude=5.0 is not supported", dpo_beta=5000.0, min_snr_gamma_magnitude=5.0)
    _refused("dpo_beta: data-parallel training is not supported", dpo_beta=5000.0, reducer=object())
