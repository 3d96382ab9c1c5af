"""The masked / per-sample weighted loss without a GPU: the float64 reference against autograd, the emulated gradient chain against the
plain kernel's documented chain, the proof that the exact-answer inputs of tests/test_gpu_masked_loss_kernels.py are exact in fp32,
the exports, every host refusal of the two entry points, every ValueError of the batch check, latent-cache records with and without
masks, and the loader's defaults."""
import io
import zipfile

import numpy as np
import pytest
import torch

from tests import masked_loss_reference as mr
from tests.kernel_checks import LIMIT, exact_ints

F32 = torch.float32


def _case(B, C, h, w, seed):
    pred = exact_ints((B, h, w, C), -1, 1, seed).float().numpy()
    target = exact_ints((B, C, h, w), -1, 1, seed + 1, dtype=F32).numpy()
    return pred, target


# ================================================================================================ the reference itself
@pytest.mark.parametrize("normalize", [False, True])
def test_reference_gradient_equals_float64_autograd_of_the_written_out_loss(normalize):
    B, C, h, w, f = 3, 3, 4, 6, 2
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(B, h * f, w * f, generator=g) * 1.4 - 0.2  # values on both sides of [0, 1]
    mask[2] = 0.0  # a fully masked-out sample
    pred, target = torch.randn(B, h, w, C, generator=g, dtype=torch.float64), torch.randn(B, C, h, w, generator=g, dtype=torch.float64)
    snr, lw, floor = torch.tensor([0.7, 1.0, 0.3]).double(), torch.tensor([1.0, 0.5, 2.0]).double(), 0.0
    e = mr.effective_mask(mr.pooled_mask(mask.numpy(), f), floor)
    ref = mr.reference(pred.numpy(), target.numpy(), e, snr.numpy(), lw.numpy(), normalize)
    # the loss as include/sdt.h writes it, in torch float64
    p = pred.clone().requires_grad_(True)
    mp = torch.nn.functional.avg_pool2d(mask.double().clamp(0, 1)[:, None], f)[:, 0]
    et = torch.maximum(mp, torch.tensor(floor).double())
    assert np.allclose(et.numpy(), e, rtol=0, atol=1e-15)
    S = et.reshape(B, -1).sum(1)
    s = torch.where(S == 0, torch.zeros_like(S), h * w / torch.where(S == 0, torch.ones_like(S), S)) if normalize else torch.ones(B).double()
    k = snr * lw * s
    per = (et[..., None] * (target.permute(0, 2, 3, 1) - p) ** 2).reshape(B, -1).sum(1)
    loss = (k * per).sum() / (B * C * h * w)
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-14 * abs(ref["loss"])
    assert np.allclose(p.grad.numpy(), ref["grad"], rtol=1e-13, atol=1e-18)
    assert np.allclose((k * per / (C * h * w)).detach().numpy(), ref["loss_per_sample"], rtol=1e-13, atol=0)
    assert abs(ref["loss_per_sample"].mean() - ref["loss"]) <= 1e-14 * abs(ref["loss"])
    assert ref["loss_per_sample"][2] == 0 and np.isfinite(ref["grad"]).all() and not ref["grad"][2].any()


@pytest.mark.parametrize("B,C,h,w", [(2, 4, 8, 8), (5, 3, 7, 11), (3, 9, 5, 7)])
@pytest.mark.parametrize("weights", [False, True])
def test_unit_mask_chain_is_the_plain_kernels_chain_element_for_element(B, C, h, w, weights):
    """With e == 1 and loss_weight 1 the emulated chain bf16(fl(fl(fl(-2 fl(k e)) diff) inv_count)) equals the chain
    test_mse_loss_and_gradient_exact documents for sdt_mse_loss_fwd_bwd, for random (not only integer) operands too."""
    g = torch.Generator().manual_seed(B * 100 + C)
    for ints in (True, False):
        if ints:
            pred, target = _case(B, C, h, w, 11)
        else:
            pred = torch.randn(B, h, w, C, generator=g).bfloat16().float().numpy()
            target = torch.randn(B, C, h, w, generator=g).numpy()
        snr = (torch.rand(B, generator=g) + 0.1).numpy() if weights else None
        k = mr.sample_factors(B, h * w, None, snr, np.ones(B, np.float32), False, dtype=np.float32)
        got = mr.dpred_chain32(pred, target, np.ones((B, h, w), np.float32), k)
        want = mr.plain_dpred_chain32(pred, target, snr)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(mr.dpred_chain32(pred, target, None, k).view(torch.int16), want.view(torch.int16))


def test_the_exact_cases_are_exact_in_fp32():
    """Masks: values in {0, 0.25, 0.5, 1} and their block sums are multiples of 1/4 below 2^24 / 4, the pooled mean divides by a power of
    two: float32 == float64.  Loss, every case x variant of the GPU test: integers in -1..1, weights in {0.5, 1, 2}, the normalisation
    quotient a power of two; the bound on every partial and total is derived in the loop."""
    for name, f, B, H, W in mr.PREPARE_CASES:
        m = mr.seeded_mask((B, H, W), 7, special=True).numpy()
        mp32, mp64 = mr.pooled_mask(m, f, np.float32), mr.pooled_mask(m, f, np.float64)
        assert mp32.dtype == np.float32 and np.array_equal(mp32.astype(np.float64), mp64), name
        assert f * f * 4 < LIMIT
        for floor in mr.FLOORS:
            e = mr.effective_mask(mp32, floor)
            S64 = e.astype(np.float64).reshape(B, -1).sum(1)
            q = 4 * f * f  # every pooled value, the floors and so every sum are multiples of 1 / (4 f^2)
            assert (S64 * q == np.round(S64 * q)).all() and (S64 * q < LIMIT).all(), name
    for case in mr.LOSS_CASES:
        name, B, C, h, w, cpad = case
        count = B * C * h * w
        for variant in mr.LOSS_VARIANTS:
            what = f"{name} {variant[0]}"
            x = mr.loss_inputs(case, variant)
            assert set(np.unique(x["pred"])) <= {-1.0, 0.0, 1.0} and set(np.unique(x["target"])) <= {-1.0, 0.0, 1.0}
            assert x["e"] is None or set(np.unique(x["e"])) <= set(mr.MASK_VALUES)
            assert all(v is None or set(v.tolist()) <= set(mr.WEIGHTS) for v in (x["snr"], x["lw"]))
            ref = mr.reference(x["pred"], x["target"], x["e"], x["snr"], x["lw"], x["normalize"])
            S, k = ref["sums"], ref["k"]
            if variant[5]:
                assert S[B - 1] == 0 and k[B - 1] == (0 if x["normalize"] else k[B - 1]) and ref["loss_per_sample"][B - 1] == 0
            if x["normalize"]:
                quot = h * w / S[S > 0]
                assert (np.log2(quot) == np.round(np.log2(quot))).all(), f"{what}: h*w / S_b is not a power of two"
            k32 = mr.sample_factors(B, h * w, S.astype(np.float32), x["snr"], x["lw"], x["normalize"], dtype=np.float32)
            assert np.array_equal(k32.astype(np.float64), k), what
            pos = k[k > 0]
            assert (np.log2(pos) == np.round(np.log2(pos))).all() and pos.min() >= 0.5, f"{what}: k_b must be powers of two >= 0.5"
            # e diff^2 is a multiple of ge (1/4 with fractional masks, 1 with 0 / 1 masks), k_b a power of two >= 1/2: every partial sum of
            # a sample is a multiple of ge, every term k_b a_b and every sum of terms a multiple of g = ge / 2, and so is
            # loss_before * count.  All of them are at most loss_before * count + sum k_b a_b, which must stay below 2^24 * g.
            ge = 1.0 if x["e"] is None or set(np.unique(x["e"])) <= {0.0, 1.0} else 0.25
            diff = x["target"].transpose(0, 2, 3, 1).astype(np.float64) - x["pred"]
            a = ((np.ones((B, h, w)) if x["e"] is None else x["e"].astype(np.float64))[..., None] * diff ** 2).reshape(B, -1).sum(1)
            if count & (count - 1) == 0:
                assert (mr.LOSS_ACCUM_BEFORE * count + (k * a).sum()) / (ge / 2) < LIMIT, what
                want = mr.LOSS_ACCUM_BEFORE + ref["loss"]
                assert float(np.float32(want)) == want, what
                assert np.array_equal(ref["loss_per_sample"].astype(np.float32).astype(np.float64), ref["loss_per_sample"]), what
                d32 = mr.dpred_chain32(x["pred"], x["target"], x["e"], k32).float().numpy()
                assert np.array_equal(ref["grad"].astype(np.float32).astype(np.float64), ref["grad"]), what  # the true gradient is exact in fp32
                assert np.array_equal(d32, torch.from_numpy(ref["grad"]).to(torch.bfloat16).float().numpy()), what
            else:
                assert (k * a).sum() / (ge / 2) < LIMIT, what  # the sums themselves are still exact: only the two scalings round


def test_ordered_sum_emulation_adds_everything_once():
    g = torch.Generator().manual_seed(1)
    for hw, inner, B in ((64, 1, 2), (77, 3, 5), (700, 1, 3), (70000, 1, 4)):
        t = torch.randint(0, 4, (hw, inner), generator=g).float().numpy()
        assert float(mr.ordered_sum32(t, mr.partition(B, hw))) == float(t.sum(dtype=np.float64))
    assert mr.partition(2, 64) == 1 and mr.partition(4, 65536) == 128 and mr.partition(8, 32768) == 128 and mr.partition(8192, 65536) == 1


# ================================================================================================ exports and host refusals
def test_library_exports_both_entry_points_with_abi_5(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_abi_version() == 5
    for name in ("sdt_loss_mask_prepare", "sdt_masked_mse_loss_fwd_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sdt_loss_mask_prepare"]) == 12 and len(_lib.SIGNATURES["sdt_masked_mse_loss_fwd_bwd"]) == 17


def test_host_refusals_of_both_entry_points_without_a_gpu(lib):
    """Every refusal returns before any HIP call.  Pointers are made-up aligned addresses: nothing dereferences them."""
    P, WS = 4096, lib.sdt_reduce_workspace_bytes()
    err = lambda: lib.sdt_last_error()
    prep = lambda mask=P, e=P, mp=None, S=P, B=2, h=8, w=8, f=8, floor=0.0, ws=P, wsb=WS: lib.sdt_loss_mask_prepare(
        mask, e, mp, S, B, h, w, f, floor, ws, wsb, None)
    for kw in (dict(mask=None), dict(e=None), dict(S=None)):
        assert prep(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(mask=P + 2), dict(e=P + 1), dict(mp=P + 2), dict(S=P + 3)):
        assert prep(**kw) == -1 and b"misaligned" in err(), kw
    for f in (0, 3, 5, 32, -8):
        assert prep(f=f) == -1 and b"must be 1, 2, 4, 8 or 16" in err(), f
    for floor in (-0.01, 1.5, float("nan"), float("inf")):
        assert prep(floor=floor) == -1 and b"must lie in [0, 1]" in err(), floor
    for kw in (dict(B=0), dict(B=-1), dict(B=8193), dict(h=0), dict(w=0)):
        assert prep(**kw) == -1 and b"bad shape" in err(), kw
    for kw in (dict(ws=None), dict(wsb=WS - 1), dict(ws=P + 4)):
        assert prep(**kw) == -1 and b"workspace" in err(), kw

    loss = lambda pred=P, tgt=P, e=None, S=None, w1=None, w2=None, la=P, lps=P, dp=P, B=2, C=4, H=8, W=8, cpad=8, ws=P, wsb=WS: \
        lib.sdt_masked_mse_loss_fwd_bwd(pred, tgt, e, S, w1, w2, la, lps, dp, B, C, H, W, cpad, ws, wsb, None)
    for kw in (dict(pred=None), dict(tgt=None), dict(la=None), dict(lps=None)):
        assert loss(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(pred=P + 1), dict(dp=P + 1), dict(tgt=P + 2), dict(e=P + 2), dict(e=P, S=P + 1), dict(w1=P + 2), dict(w2=P + 3), dict(la=P + 2),
               dict(lps=P + 2)):
        assert loss(**kw) == -1 and b"misaligned" in err(), kw
    assert loss(cpad=3) == -1 and b"cpad=3 < C=4" in err()
    for kw in (dict(B=0), dict(B=8193), dict(C=0), dict(H=0), dict(W=-1)):
        assert loss(**kw) == -1 and b"bad shape" in err(), kw
    assert loss(S=P) == -1 and b"need the effective mask" in err()
    for kw in (dict(ws=None), dict(wsb=WS - 1), dict(ws=P + 8)):
        assert loss(**kw) == -1 and b"workspace" in err(), kw


# ================================================================================================ the batch check
def test_check_batch_refuses_bad_loss_entries_before_any_kernel():
    from stable_diffusion_training_amd import training_utils as tu
    cpu = torch.device("cpu")
    cfg, vae = {"in_channels": 4}, object()
    px = {"pixel_values": torch.zeros(2, 3, 64, 32), "input_ids": torch.zeros(2, 77, dtype=torch.int32)}
    mom = {"latent_moments": torch.zeros(2, 8, 4, 8, dtype=torch.bfloat16), "input_ids": px["input_ids"]}
    check = lambda b, floor=0.0, norm=False: tu._check_batch(b, cfg, vae, cpu, floor, norm)
    # well-formed entries pass, and so does a batch without them
    assert check(px) is False and check(mom) is True
    assert check(dict(px, loss_mask=torch.ones(2, 64, 32), loss_weight=torch.ones(2)), 0.25, True) is False
    assert check(dict(mom, loss_mask=torch.ones(2, 8, 4)), 1.0, True) is True
    assert check(dict(mom, loss_weight=torch.ones(2))) is True
    bad = [
        (dict(px, loss_mask=torch.ones(2, 64, 32, dtype=torch.float64)), {}, "must be a float32 tensor"),
        (dict(px, loss_mask=np.ones((2, 64, 32), np.float32)), {}, "must be a float32 tensor"),
        (dict(px, loss_mask=torch.ones(2, 64, 32, device="meta")), {}, "the step runs on"),
        (dict(px, loss_mask=torch.ones(2, 32, 64)), {}, "pixel size"),
        (dict(px, loss_mask=torch.ones(2, 8, 4)), {}, "pixel size"),
        (dict(px, loss_mask=torch.ones(2, 1, 64, 32)), {}, "pixel size"),
        (dict(px, loss_mask=torch.ones(2, 32, 64).transpose(1, 2)), {}, "must be contiguous"),
        (dict(mom, loss_mask=torch.ones(2, 64, 32)), {}, "latent size"),
        (dict(mom, loss_mask=torch.ones(1, 8, 4)), {}, "latent size"),
        (dict(px, loss_weight=torch.ones(3)), {}, "one weight per sample"),
        (dict(px, loss_weight=torch.ones(2, 1)), {}, "one weight per sample"),
        (dict(px, loss_weight=torch.ones(2, dtype=torch.float64)), {}, "must be a float32 tensor"),
        (dict(px, loss_weight=torch.ones(2, device="meta")), {}, "the step runs on"),
        (dict(px, loss_mask=torch.ones(2, 64, 32)), dict(floor=-0.1), r"must be a number in \[0, 1\]"),
        (dict(px, loss_mask=torch.ones(2, 64, 32)), dict(floor=1.01), r"must be a number in \[0, 1\]"),
        (dict(px, loss_mask=torch.ones(2, 64, 32)), dict(floor=float("nan")), r"must be a number in \[0, 1\]"),
        (dict(px, loss_mask=torch.ones(2, 64, 32)), dict(floor="0.5"), r"must be a number in \[0, 1\]"),
        (px, dict(floor=2.0), r"must be a number in \[0, 1\]"),
        (px, dict(norm=True), "needs a loss_mask"),
        (dict(mom, loss_weight=torch.ones(2)), dict(norm=True), "needs a loss_mask"),
    ]
    for batch, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            check(batch, **kw)
    import dataclasses
    assert len(dataclasses.fields(tu.TrainingConfig)) == 28
    assert tu.LOSS_KEYS == ("loss_mask", "loss_weight")


# ================================================================================================ latent cache records
def _parent_record(moments, batch):
    """What latent_cache.Writer.add wrote before loss masks existed (the parent commit's record), as np.savez bytes."""
    rec = {"moments": moments.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)}
    for k in ("input_ids", "time_ids", "text_embeds"):
        if k in batch:
            v = batch[k].detach().cpu()
            rec[k] = (v.view(torch.int16).numpy().view(np.uint16) if v.dtype == torch.bfloat16 else v.numpy())
    buf = io.BytesIO()
    np.savez(buf, **rec)
    return buf.getvalue()


def _members(data):
    """(name, bytes) of every member of an .npz, in archive order (the zip's timestamps are the only bytes np.savez does not fix)."""
    with zipfile.ZipFile(io.BytesIO(data)) as z:
        return [(i.filename, z.read(i), i.compress_type) for i in z.infolist()]


def test_cache_records_with_and_without_masks_round_trip(tmp_path):
    from stable_diffusion_training_amd import latent_cache as lc
    g = torch.Generator().manual_seed(0)
    mom = torch.randn(2, 4, 6, 8, generator=g).bfloat16()
    plain = {"input_ids": torch.randint(0, 100, (2, 77), generator=g, dtype=torch.int32), "time_ids": torch.zeros(2, 6, dtype=torch.int32),
             "text_embeds": torch.randn(2, 16, generator=g).bfloat16(), "attention_mask": torch.ones(2, 77)}
    pooled, weight = torch.rand(2, 4, 6, generator=g), torch.tensor([1.0, 0.25])
    w = lc.Writer(str(tmp_path / "c"), 4, "digest")
    w.add(mom, plain)
    w.add(mom, dict(plain, loss_weight=weight, loss_mask=torch.rand(2, 32, 48)), loss_mask=pooled)  # the batch's pixel mask is not stored
    w.add(mom, dict(plain, loss_weight=weight))
    with pytest.raises(ValueError, match="latent size"):
        w.add(mom, plain, loss_mask=torch.rand(2, 32, 48))
    with pytest.raises(ValueError, match="latent size"):
        w.add(mom, plain, loss_mask=pooled.double())
    w.close()
    assert lc.FORMAT_VERSION == 1
    # a mask-free record: the members (names, order, bytes) the parent commit's Writer wrote
    got = _members(open(lc._record_path(str(tmp_path / "c"), 0), "rb").read())
    assert got == _members(_parent_record(mom, plain)) and [n for n, _, _ in got] == ["moments.npy", "input_ids.npy", "time_ids.npy", "text_embeds.npy"]
    r = lc.Reader(str(tmp_path / "c"), device="cpu")
    b0, b1, b2 = list(r)
    assert set(b0) == {"latent_moments", "input_ids", "time_ids", "text_embeds"}
    assert set(b1) == set(b0) | {"loss_mask", "loss_weight"} and set(b2) == set(b0) | {"loss_weight"}
    assert b1["loss_mask"].dtype == F32 and torch.equal(b1["loss_mask"], pooled) and torch.equal(b1["loss_weight"], weight)
    assert torch.equal(b2["loss_weight"], weight)
    for b in (b0, b1, b2):
        assert torch.equal(b["latent_moments"].view(torch.int16), mom.view(torch.int16)) and torch.equal(b["text_embeds"].view(torch.int16), plain["text_embeds"].view(torch.int16))
        assert torch.equal(b["input_ids"], plain["input_ids"])


# ================================================================================================ the loader
def _loader(**kw):
    from stable_diffusion_training_amd.streamer import DataLoader
    d = DataLoader(training_batch_size=4, repeat_batch=1, maximum_resolution_areas=[128 ** 2], bucket_lower_bound_resolutions=[64],
                   batches_per_chunk=3, vocab_size=1000, seed=5, **kw)
    d._print_debug = False
    d.create_training_dataframe()
    d.dispatch_worker()
    return d


def test_streamer_defaults_are_unchanged_and_the_new_entries_are_seeded():
    d = _loader()
    for index in range(3):
        b = d.grab_next_batch()
        assert set(b) == {"pixel_values", "input_ids", "attention_mask"}
        # the parent commit's draws, restated
        b0, b1 = d._plan[index]
        g = torch.Generator().manual_seed((5 * 1_000_003 + 0) * 1_000_003 + index * 64 + 0)
        px = torch.rand(4, 3, b0, b1, generator=g) * 2 - 1
        ids = torch.randint(0, 998, (4, 1, 77), generator=g, dtype=torch.int32)
        ids[..., 0], ids[..., -1] = 998, 999
        assert torch.equal(b["pixel_values"], px) and torch.equal(b["input_ids"], ids.reshape(4, -1))
    assert d.grab_next_batch() == "end_of_batch"
    plain, masked, again = _loader(), _loader(loss_masks=True, prior_every=2, prior_loss_weight=0.5), _loader(loss_masks=True, prior_every=2, prior_loss_weight=0.5)
    for _ in range(3):
        a, b, c = plain.grab_next_batch(), masked.grab_next_batch(), again.grab_next_batch()
        assert set(b) == set(a) | {"loss_mask", "loss_weight"}
        for k in a:
            assert torch.equal(a[k], b[k]), k
        m = b["loss_mask"]
        assert m.dtype == F32 and m.shape == a["pixel_values"][:, 0].shape and m.is_contiguous() and torch.equal(m, c["loss_mask"])
        assert set(m.unique().tolist()) <= {0.0, 1.0} and (m.reshape(4, -1).mean(1) >= 1 / 16 - 1e-6).all()
        assert b["loss_weight"].tolist() == [1.0, 0.5, 1.0, 0.5] and b["loss_weight"].dtype == F32
    # two ranks: the class images are every second sample of the GLOBAL batch
    r1 = _loader(prior_every=3, prior_loss_weight=0.25, rank=1, world_size=2)
    assert r1.grab_next_batch()["loss_weight"].tolist() == [0.25, 1.0]  # global samples 2, 3
    with pytest.raises(ValueError, match="prior_every"):
        _loader(prior_every=-1)


def test_example_reads_the_flags_from_the_config():
    """examples/train_synthetic.py: the three command-line flags exist and land in the config under the documented names."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_synthetic.py")).read()
    for flag, key in (("--masked-loss", '"masked_loss"'), ("--normalize-masked-area", '"normalize_masked_area"'), ("--prior-loss-weight", '"prior_loss_weight"')):
        assert flag in src and f"cfg[{key}]" in src and f"config_dict.get({key}" in src
