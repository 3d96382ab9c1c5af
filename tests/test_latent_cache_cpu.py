"""Host side of training from cached VAE latents (no kernel launches): the new export and its refusals, the cache file round
trip and the reader's refusals, and the step-table key of a cached batch."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import tests.kernel_checks as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
NAME = "sdt_latent_noise_target"


def test_the_new_export_is_declared_bound_and_exported(lib):
    from stable_diffusion_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sdt.h")).read()
    assert NAME in set(re.findall(r"\b(sdt_[a-z0-9_]+)\s*\(", hdr))
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    # 11 pointers, 6 sizes, 3 floats, prediction type, stream
    P, I, F = _lib._P, _lib._I, _lib._F
    assert _lib.SIGNATURES[NAME] == [P] * 11 + [I] * 6 + [F] * 3 + [I, P]
    assert lib.sdt_abi_version() == 5  # an additive export


def test_refusals_return_before_any_hip_call(lib):
    """Every check runs before the first device call, so guarded host buffers stand in (as for the neighbouring entry points): -1,
    the message, nothing written."""
    mk = lambda dt: kc.Guarded(8, 64, dt, "cpu")
    M, E, N, OF, PN, T, A, NB, TG, LT, NZ = (mk(BF), mk(torch.float32), mk(torch.float32), mk(torch.float32), mk(torch.float32),
                                             mk(torch.float32), mk(torch.float32), mk(BF), mk(torch.float32), mk(torch.float32),
                                             mk(torch.float32))

    def call(m=M.ptr, e=E.ptr, n=N.ptr, of=None, pn=None, t=T.ptr, a=A.ptr, nb=NB.ptr, tg=TG.ptr, lt=None, nz=None, B=1, L=4, H=2, W=2,
             ms=8, cpad=8, scale=0.18215, om=0.0, pm=0.0, ptype=0):
        return lib.sdt_latent_noise_target(m, e, n, of, pn, t, a, nb, tg, lt, nz, B, L, H, W, ms, cpad, scale, om, pm, ptype, None)

    cases = [
        ("null moments", dict(m=None), b"null pointer"),
        ("null eps", dict(e=None), b"null pointer"),
        ("null noise", dict(n=None), b"null pointer"),
        ("null timesteps", dict(t=None), b"null pointer"),
        ("null alphas_cumprod", dict(a=None), b"null pointer"),
        ("null noisy", dict(nb=None), b"null pointer"),
        ("cpad < L", dict(cpad=3), b"bad shape"),
        ("moment_stride < 2L", dict(ms=7), b"bad shape"),
        ("B = 0", dict(B=0), b"bad shape"),
        ("L = 0", dict(L=0), b"bad shape"),
        ("H < 0", dict(H=-1), b"bad shape"),
        ("W = 0", dict(W=0), b"bad shape"),
        ("prediction_type sample", dict(ptype=1), b"prediction_type 1"),
        ("prediction_type 3", dict(ptype=3), b"prediction_type 3"),
        ("offset magnitude without offset", dict(om=0.1), b"needs the offset noise"),
        ("perturbation magnitude without perturbation", dict(pm=0.1), b"needs the perturbation noise"),
        ("v_prediction without target", dict(tg=None, ptype=2), b"target may be NULL only for epsilon"),
        ("epsilon with offset without target", dict(tg=None, of=OF.ptr, om=0.1), b"target may be NULL only for epsilon"),
        ("epsilon with perturbation without target", dict(tg=None, pn=PN.ptr, pm=0.1), b"target may be NULL only for epsilon"),
    ]
    for what, kw, msg in cases:
        rc = call(**kw)
        assert rc == -1, f"{what}: returned {rc}"
        assert msg in lib.sdt_last_error(), f"{what}: message {lib.sdt_last_error()!r}"
    for g in (M, E, N, OF, PN, T, A, NB, TG, LT, NZ):
        ref = kc.Guarded(8, 64, g.dtype, "cpu")
        assert torch.equal(kc.bits(g.arena), kc.bits(ref.arena)), "a refused call wrote into a buffer"


def _fake_vae(seed, L=4):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(call={"latent_channels": L}, params=types.SimpleNamespace(master=torch.randn(257, generator=g)))


def _patterns(shape, seed):
    """Random bf16 bit patterns, with every kind of NaN / inf / zero / denormal pattern planted at the front."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 65536, shape, generator=g, dtype=torch.int32)
    special = torch.tensor([0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7FFF, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x8001, 0x41A0, 0xC1F0], dtype=torch.int32)
    bits.view(-1)[: special.numel()] = special
    return bits.to(torch.int16).view(BF), bits


def test_cache_round_trip_keeps_every_bit(tmp_path):
    from stable_diffusion_training_amd import latent_cache as lc
    vae = _fake_vae(1)
    w = lc.Writer(str(tmp_path / "c"), 4, lc.vae_digest(vae))
    want = []
    for i, (B, h, wd) in enumerate([(2, 8, 8), (3, 4, 12), (1, 5, 7)]):
        mom, bits = _patterns((B, h, wd, 8), 10 + i)
        assert torch.isnan(mom.float()).sum() >= 5
        g = torch.Generator().manual_seed(20 + i)
        batch = {"pixel_values": torch.zeros(B, 3, 8 * h, 8 * wd), "input_ids": torch.randint(0, 49408, (B, 77), generator=g, dtype=torch.int32),
                 "attention_mask": torch.ones(B, 77, dtype=torch.int32)}
        if i == 1:
            batch["time_ids"] = torch.randint(0, 1024, (B, 6), generator=g, dtype=torch.int32)
            batch["text_embeds"] = torch.randn(B, 1280, generator=g)
        w.add(mom, batch)
        want.append((bits, batch))
    w.close()
    idx = json.load(open(tmp_path / "c" / "index.json"))
    assert set(idx) == {"format_version", "latent_channels", "buckets", "vae_digest"}  # settings only
    assert idx["format_version"] == 1 and idx["latent_channels"] == 4 and idx["vae_digest"] == lc.vae_digest(vae)
    assert idx["buckets"] == [[2, 3, 64, 64], [3, 3, 32, 96], [1, 3, 40, 56]]
    with np.load(tmp_path / "c" / "record_000000.npz") as rec:
        assert rec["moments"].dtype == np.uint16 and rec["moments"].shape == (2, 8, 8, 8)
    r = lc.Reader(str(tmp_path / "c"), device="cpu", vae=vae)
    assert len(r) == 3
    for rep in range(2):  # rewind() starts over
        for i, (bits, batch) in enumerate(want):
            got = r.grab_next_batch()
            assert set(got) == {"latent_moments"} | ({"input_ids", "time_ids", "text_embeds"} & set(batch))
            m = got["latent_moments"]
            assert m.dtype == BF and m.is_contiguous() and m.shape == bits.shape
            assert torch.equal(m.view(torch.int16).to(torch.int32) & 0xFFFF, bits), f"record {i}: the moments' bits changed"
            for k in got:
                if k != "latent_moments":
                    assert got[k].dtype == batch[k].dtype and torch.equal(got[k], batch[k]), k
        assert r.grab_next_batch() == "end_of_batch" and r.grab_next_batch() == "end_of_batch"
        r.rewind()
    assert [tuple(b["latent_moments"].shape) for b in r] == [(2, 8, 8, 8), (3, 4, 12, 8), (1, 5, 7, 8)]


def test_reader_refuses_an_unknown_version_and_other_vae_weights(tmp_path):
    from stable_diffusion_training_amd import latent_cache as lc
    vae, other = _fake_vae(1), _fake_vae(2)
    path = str(tmp_path / "c")
    w = lc.Writer(path, 4, lc.vae_digest(vae))
    w.add(_patterns((1, 2, 2, 8), 0)[0], {"input_ids": torch.zeros(1, 77, dtype=torch.int32)})
    w.close()
    lc.Reader(path, device="cpu")           # no VAE given: nothing to compare
    lc.Reader(path, device="cpu", vae=vae)
    with pytest.raises(ValueError, match="other VAE weights"):
        lc.Reader(path, device="cpu", vae=other)
    idx_path = os.path.join(path, "index.json")
    idx = json.load(open(idx_path))
    for version in (2, 0, None, "1"):
        json.dump(dict(idx, format_version=version), open(idx_path, "w"))
        with pytest.raises(ValueError, match="format version"):
            lc.Reader(path, device="cpu")
    with pytest.raises(ValueError, match="moments must be bfloat16"):
        lc.Writer(path, 4, "x").add(torch.zeros(1, 2, 2, 8), {})


@pytest.mark.parametrize("B,H,W", [(4, 512, 512), (2, 384, 640)])
def test_step_key_is_the_same_for_pixels_and_their_moments(B, H, W):
    from stable_diffusion_training_amd import training_utils as tu
    px = {"pixel_values": torch.empty(B, 3, H, W, device="meta")}
    mom = {"latent_moments": torch.empty(B, H // 8, W // 8, 8, dtype=BF, device="meta")}
    key = tu.step_key(px)
    assert key == (B, 3, H, W) and type(key) is tuple and tu.step_key(mom) == key
    assert hash(key) == hash(px["pixel_values"].shape)  # the table's keys are what the loop looked up before
    assert tu.step_key({"latent_moments": torch.empty(B, H // 16, W // 16, 32, dtype=BF, device="meta")}, downscale=16) == key


def test_batch_validation_refuses_malformed_batches():
    """The checks train_step makes before any kernel (tests/test_gpu_latent_cache.py runs them through train_step itself)."""
    from stable_diffusion_training_amd import training_utils as tu
    cpu = torch.device("cpu")
    cfg, vae = {"in_channels": 4}, object()
    mom, px = torch.zeros(2, 8, 8, 8, dtype=BF), torch.zeros(2, 3, 64, 64)
    check = lambda batch, v=None, c=cfg: tu._check_batch(batch, c, v, cpu)
    assert check({"latent_moments": mom}) is True and check({"pixel_values": px}, vae) is False
    for batch, v, c, msg in [
        ({"latent_moments": mom, "pixel_values": px}, vae, cfg, "not both"),
        ({"input_ids": None}, vae, cfg, "needs pixel_values"),
        ({"pixel_values": px}, None, cfg, "need the frozen VAE"),
        ({"latent_moments": mom.float()}, None, cfg, "must be a bfloat16"),
        ({"latent_moments": mom[0]}, None, cfg, "must be a bfloat16"),
        ({"latent_moments": mom.numpy}, None, cfg, "must be a bfloat16"),
        ({"latent_moments": mom[..., :7].contiguous()}, None, cfg, "must be even"),
        ({"latent_moments": torch.zeros(2, 8, 8, 16, dtype=BF)[..., :8]}, None, cfg, "must be contiguous"),
        ({"latent_moments": torch.zeros(2, 8, 8, 32, dtype=BF)}, None, cfg, "in_channels is 4"),
        ({"latent_moments": mom.to("meta")}, None, cfg, "the step runs on cpu"),
        ({"latent_moments": mom, "text_embeds": None}, None, dict(cfg, addition_embed_type="text_time"), "must hold time_ids"),
    ]:
        with pytest.raises(ValueError, match=msg):
            check(batch, v, c)
    assert check({"latent_moments": mom, "time_ids": None}, None, dict(cfg, addition_embed_type="text_time")) is True
