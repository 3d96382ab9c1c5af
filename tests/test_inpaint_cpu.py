"""Inpainting without a GPU: the exports and their host refusals, train_step's ValueErrors for the new batch keys, the UNet
recognition and conv_in widening, cache records with and without the mask, and the loader's masks."""
import numpy as np
import pytest
import torch

from tests import inpaint_reference as ir

BF, F32 = torch.bfloat16, torch.float32
NAMES = ("sdt_inpaint_mask_pixels", "sdt_inpaint_noise_target", "sdt_inpaint_pack_input")


# ================================================================================================ the reference itself
def test_reference_threshold_pooling_masked_image_and_layout():
    m = ir.MASK_VALUES
    assert ir.repaint(m).tolist() == [False, False, False, True, True, True, False, True, False]
    mask = np.zeros((1, 4, 6), np.float32)
    mask[0, 0, 2], mask[0, 1, 1], mask[0, 2, 4] = 1.0, 1.0, np.nan  # only the top-left pixel of a block counts
    assert ir.latent_mask(mask, 2).tolist() == [[[0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]]
    px = np.array([[[[-0.0, np.nan, 3.0]]]], np.float32)
    out = ir.masked_image(px, np.array([[[1.0, 1.0, 0.0]]], np.float32))
    assert out.view(np.uint32).tolist() == [[[[0, 0, np.float32(3.0).view(np.uint32)]]]]  # +0 for -0 and for NaN under the mask
    noisy = np.arange(2 * 1 * 1 * 8, dtype=np.uint16).reshape(2, 1, 1, 8) + 100
    masked = np.arange(1 * 1 * 1 * 4, dtype=np.uint16).reshape(1, 1, 1, 4) + 7
    row = ir.unet_input_bits(noisy, np.array([[[0.5]]], np.float32), masked, 3, 8)
    assert row[0, 0, 0].tolist() == [100, 101, 102, ir.BF16_ONE, 7, 8, 9, 0] and row[1, 0, 0].tolist() == [108, 109, 110, ir.BF16_ONE, 7, 8, 9, 0]


# ================================================================================================ exports and host refusals
def test_exports_are_bound_and_the_abi_is_5(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_abi_version() == 5
    for name in NAMES:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert len(_lib.SIGNATURES["sdt_inpaint_noise_target"]) == len(_lib.SIGNATURES["sdt_latent_noise_target"]) + 4


def test_host_refusals_return_before_any_hip_call(lib):
    """Pointers are made-up aligned addresses: nothing dereferences them, every call returns -1 with a message."""
    P = 4096
    err = lambda: lib.sdt_last_error()
    mp = lambda px=P, m=P, st=P, lm=P, B=2, C=3, H=16, W=24, cpad=8, f=8: lib.sdt_inpaint_mask_pixels(px, m, st, lm, B, C, H, W, cpad, f, None)
    for kw in (dict(px=None), dict(m=None), dict(st=None), dict(lm=None)):
        assert mp(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(f=0), dict(f=-8)):
        assert mp(**kw) == -1 and b"at least 1" in err(), kw
    for kw in (dict(f=5), dict(H=20), dict(W=20), dict(f=16)):
        assert mp(**kw) == -1 and b"multiples of f" in err(), kw
    for kw in (dict(cpad=2), dict(B=0), dict(C=0), dict(H=0), dict(W=-8)):
        assert mp(**kw) == -1 and b"bad shape" in err(), kw

    nt = lambda mom=P, mm=P, e=P, me=P, lm=P, n=P, off=None, pn=None, t=P, a=P, out=P, tg=P, lat=None, nz=None, ml=None, B=2, L=4, H=5, W=7, ms=8, \
        cpad=16, om=0.0, pm=0.0, pt=0: lib.sdt_inpaint_noise_target(mom, mm, e, me, lm, n, off, pn, t, a, out, tg, lat, nz, ml, B, L, H, W, ms, cpad,
                                                                    0.18215, om, pm, pt, None)
    for kw in (dict(mom=None), dict(mm=None), dict(e=None), dict(me=None), dict(lm=None), dict(n=None), dict(t=None), dict(a=None), dict(out=None)):
        assert nt(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(cpad=8), dict(cpad=4), dict(ms=7), dict(B=0), dict(L=0), dict(H=0), dict(W=0)):
        assert nt(**kw) == -1 and b"bad shape" in err(), kw
    for kw in (dict(pt=1), dict(pt=3)):
        assert nt(**kw) == -1 and b"prediction_type" in err(), kw
    assert nt(om=0.1) == -1 and b"needs the offset noise" in err()
    assert nt(pm=0.1) == -1 and b"needs the perturbation noise" in err()
    for kw in (dict(tg=None, pt=2), dict(tg=None, off=P), dict(tg=None, pn=P)):
        assert nt(**kw) == -1 and b"target may be NULL only" in err(), kw

    pk = lambda lat=P, ml=P, lm=P, out=P, R=4, B=2, L=4, h=5, w=7, cs=8, cm=8, cd=16: lib.sdt_inpaint_pack_input(lat, ml, lm, out, R, B, L, h, w, cs,
                                                                                                                 cm, cd, None)
    for kw in (dict(lat=None), dict(ml=None), dict(lm=None), dict(out=None)):
        assert pk(**kw) == -1 and b"null pointer" in err(), kw
    for kw in (dict(R=3), dict(R=0), dict(B=0), dict(L=0), dict(h=0), dict(w=0)):
        assert pk(**kw) == -1 and b"bad shape" in err(), kw
    for kw in (dict(cd=8), dict(cs=3), dict(cm=2)):
        assert pk(**kw) == -1 and b"must hold" in err(), kw


# ================================================================================================ train_step's refusals
def _cfg(cin, cout=4):
    return dict(in_channels=cin, out_channels=cout, addition_embed_type=None)


def test_inpaint_latent_channels():
    from stable_diffusion_training_amd import nets
    assert nets.inpaint_latent_channels(_cfg(9)) == 4
    assert nets.inpaint_latent_channels(_cfg(33, 16)) == 16
    assert nets.inpaint_latent_channels(_cfg(7, 3)) == 3
    for cin, cout in ((4, 4), (8, 4), (5, 4), (9, 3), (10, 4)):
        assert nets.inpaint_latent_channels(_cfg(cin, cout)) is None
    assert nets.inpaint_latent_channels(nets.unet_config("sd15")) is None
    assert nets.inpaint_latent_channels(nets.unet_config("sd15", in_channels=9)) == 4


def test_check_batch_refuses_bad_inpainting_batches():
    from stable_diffusion_training_amd import training_utils as tu
    assert tu.LOSS_KEYS == ("loss_mask", "loss_weight") and tu.INPAINT_KEYS == ("inpaint_mask",)
    cpu = torch.device("cpu")
    B, H, W, h, w = 2, 16, 24, 2, 3
    px, mom = torch.zeros(B, 3, H, W), torch.zeros(B, h, w, 8, dtype=BF)
    mask_px, mask_lat = torch.zeros(B, H, W), torch.zeros(B, h, w)
    check = lambda batch, cfg, vae="vae": tu._check_batch(batch, cfg, vae, cpu)
    # well-formed: pixel and cached, and the plain batches as before
    assert check(dict(pixel_values=px, inpaint_mask=mask_px), _cfg(9)) is False
    assert check(dict(latent_moments=mom, masked_latent_moments=mom.clone(), inpaint_mask=mask_lat), _cfg(9), None) is True
    assert check(dict(pixel_values=px), _cfg(4)) is False and check(dict(latent_moments=mom), _cfg(4), None) is True
    bad = [
        (dict(pixel_values=px), _cfg(9), "needs inpaint_mask"),
        (dict(latent_moments=mom), _cfg(9), "needs inpaint_mask"),
        (dict(pixel_values=px, inpaint_mask=mask_px), _cfg(4), "need an inpainting UNet"),
        (dict(latent_moments=mom, inpaint_mask=mask_lat), _cfg(4), "need an inpainting UNet"),
        (dict(latent_moments=mom, masked_latent_moments=mom), _cfg(4), "need an inpainting UNet"),
        (dict(pixel_values=px, inpaint_mask=mask_px), _cfg(8), "need an inpainting UNet"),
        (dict(pixel_values=px, inpaint_mask=mask_px.double()), _cfg(9), "inpaint_mask must be a float32 tensor"),
        (dict(pixel_values=px, inpaint_mask=mask_px.numpy()), _cfg(9), "inpaint_mask must be a float32 tensor"),
        (dict(pixel_values=px, inpaint_mask=mask_px.to("meta")), _cfg(9), "inpaint_mask lives on"),
        (dict(pixel_values=px, inpaint_mask=mask_lat), _cfg(9), "inpaint_mask has shape"),
        (dict(pixel_values=px, inpaint_mask=mask_px[:1]), _cfg(9), "inpaint_mask has shape"),
        (dict(pixel_values=px, inpaint_mask=torch.zeros(B, H, 2 * W)[:, :, ::2]), _cfg(9), "inpaint_mask must be contiguous"),
        (dict(latent_moments=mom, masked_latent_moments=mom, inpaint_mask=mask_px), _cfg(9), "inpaint_mask has shape"),
        (dict(latent_moments=mom, inpaint_mask=mask_lat), _cfg(9), "needs masked_latent_moments"),
        (dict(latent_moments=mom, masked_latent_moments=mom.float(), inpaint_mask=mask_lat), _cfg(9), "masked_latent_moments must be a bfloat16"),
        (dict(latent_moments=mom, masked_latent_moments=mom.to("meta"), inpaint_mask=mask_lat), _cfg(9), "masked_latent_moments live on"),
        (dict(latent_moments=mom, masked_latent_moments=mom[:, :1], inpaint_mask=mask_lat), _cfg(9), "masked_latent_moments have shape"),
        (dict(latent_moments=mom, masked_latent_moments=torch.zeros(B, h, w, 16, dtype=BF)[..., ::2], inpaint_mask=mask_lat), _cfg(9),
         "masked_latent_moments must be contiguous"),
        (dict(masked_latent_moments=mom, inpaint_mask=mask_lat), _cfg(9), "beside latent_moments"),
        (dict(pixel_values=px, masked_latent_moments=mom, inpaint_mask=mask_px), _cfg(9), "beside latent_moments"),
        # the moments' own L check: an inpainting UNet wants L = out_channels, every other mismatch is refused as before
        (dict(latent_moments=torch.zeros(B, h, w, 16, dtype=BF), masked_latent_moments=mom, inpaint_mask=mask_lat), _cfg(9), "out_channels is 4"),
        (dict(latent_moments=mom), _cfg(8), "in_channels is 8"),
        (dict(latent_moments=torch.zeros(B, h, w, 18, dtype=BF)), _cfg(4), "in_channels is 4"),
    ]
    for batch, cfg, match in bad:
        with pytest.raises(ValueError, match=match):
            check(batch, cfg, None if "latent_moments" in batch else "vae")


def test_train_step_raises_those_errors_before_touching_a_device():
    """train_step with stand-in states (only .config and .store.device are read before _check_batch)."""
    import types
    from stable_diffusion_training_amd import training_utils as tu
    store = types.SimpleNamespace(device=torch.device("cpu"), trainable=True)
    state = lambda cin: types.SimpleNamespace(config=_cfg(cin), store=store, adapter=None)
    sched = types.SimpleNamespace(call=None, params=None)
    step = lambda batch, cin: tu.train_step(state(cin), state(cin), None, None, batch, None, "vae", sched)
    px = torch.zeros(2, 3, 16, 16)
    with pytest.raises(ValueError, match="needs inpaint_mask"):
        step(dict(pixel_values=px), 9)
    with pytest.raises(ValueError, match="need an inpainting UNet"):
        step(dict(pixel_values=px, inpaint_mask=torch.zeros(2, 16, 16)), 4)
    with pytest.raises(ValueError, match="inpaint_mask has shape"):
        step(dict(pixel_values=px, inpaint_mask=torch.zeros(2, 2, 2)), 9)


# ================================================================================================ widen_conv_in
def test_widen_conv_in_keeps_old_rows_and_zeroes_new_ones():
    from stable_diffusion_training_amd import nets
    cfg = nets.unet_config("tiny")
    params = nets.init_params(nets.unet_spec(cfg), 3)
    wide, wcfg = nets.widen_conv_in(params, cfg, 9)
    assert wcfg["in_channels"] == 9 and cfg["in_channels"] == 4 and nets.inpaint_latent_channels(wcfg) == 4
    k, kw = params["conv_in/kernel"], wide["conv_in/kernel"]
    assert tuple(kw.shape) == (3, 3, 9, k.shape[3]) and kw.dtype == k.dtype and tuple(k.shape) == (3, 3, 4, k.shape[3])
    assert torch.equal(kw[:, :, :4].view(torch.int32), k.view(torch.int32)) and (kw[:, :, 4:].view(torch.int32) == 0).all()
    assert all(wide[n] is params[n] for n in params if n != "conv_in/kernel")
    assert dict(nets.unet_spec(wcfg))["conv_in/kernel"] == (3, 3, 9, k.shape[3])
    # numpy leaves and the nested tree
    nested = {"conv_in": {"kernel": k.numpy(), "bias": params["conv_in/bias"].numpy()}}
    nw, _ = nets.widen_conv_in(nested, cfg, 9)
    assert isinstance(nw["conv_in"]["kernel"], np.ndarray) and np.array_equal(nw["conv_in"]["kernel"][:, :, :4], k.numpy())
    assert not nw["conv_in"]["kernel"][:, :, 4:].any() and nw["conv_in"]["bias"] is nested["conv_in"]["bias"]
    same, scfg = nets.widen_conv_in(params, cfg, 4)
    assert torch.equal(same["conv_in/kernel"], k) and scfg["in_channels"] == 4
    for bad in (3, 0, 4.5):
        with pytest.raises(ValueError, match="narrower"):
            nets.widen_conv_in(params, cfg, bad)
    with pytest.raises(ValueError, match="config says"):
        nets.widen_conv_in(params, dict(cfg, in_channels=9), 9)


# ================================================================================================ cache records
def test_cache_records_with_and_without_the_mask_round_trip(tmp_path):
    from stable_diffusion_training_amd import latent_cache as lc
    g = torch.Generator().manual_seed(5)
    B, h, w, L = 2, 3, 5, 4
    mom, mm = torch.randn(B, h, w, 2 * L, generator=g).to(BF), torch.randn(B, h, w, 2 * L, generator=g).to(BF)
    lm = (torch.rand(B, h, w, generator=g) > 0.5).float()
    batch = {"input_ids": torch.randint(0, 100, (B, 77), generator=g, dtype=torch.int32), "pixel_values": torch.zeros(B, 3, 8 * h, 8 * w)}
    wr = lc.Writer(str(tmp_path / "c"), L, "digest")
    wr.add(mom, batch)
    wr.add(mom, batch, inpaint=(mm, lm))
    for bad in ((mm.float(), lm), (mm[:1], lm), (mm, lm.double()), (mm, lm[:, :1])):
        with pytest.raises(ValueError, match="masked_latent_moments must be|inpaint_mask must be"):
            wr.add(mom, batch, inpaint=bad)
    wr.close()
    with np.load(str(tmp_path / "c" / "record_000000.npz")) as rec:
        assert sorted(rec.files) == ["input_ids", "moments"]  # a record without the mask keeps its members
    with np.load(str(tmp_path / "c" / "record_000001.npz")) as rec:
        assert sorted(rec.files) == ["inpaint_mask", "input_ids", "masked_latent_moments", "moments"]
        assert rec["masked_latent_moments"].dtype == np.uint16 and rec["inpaint_mask"].dtype == np.float32
    r = lc.Reader(str(tmp_path / "c"), device="cpu")
    plain, inp = r.grab_next_batch(), r.grab_next_batch()
    assert r.grab_next_batch() == "end_of_batch" and r.buckets == [(B, 3, 8 * h, 8 * w)] * 2
    assert sorted(plain) == ["input_ids", "latent_moments"]
    assert sorted(inp) == ["inpaint_mask", "input_ids", "latent_moments", "masked_latent_moments"]
    assert inp["masked_latent_moments"].dtype == BF and torch.equal(inp["masked_latent_moments"].view(torch.int16), mm.view(torch.int16))
    assert torch.equal(inp["latent_moments"].view(torch.int16), mom.view(torch.int16)) and torch.equal(inp["inpaint_mask"], lm)
    assert inp["inpaint_mask"].dtype == F32 and inp["masked_latent_moments"].is_contiguous()


# ================================================================================================ the loader
def test_loader_inpaint_masks_are_seeded_rectangles():
    from stable_diffusion_training_amd.streamer import DataLoader

    def batches(seed, **kw):
        ld = DataLoader(training_batch_size=3, repeat_batch=1, maximum_resolution_areas=[128 ** 2], bucket_lower_bound_resolutions=[64],
                        batches_per_chunk=3, vocab_size=1000, seed=seed, **kw)
        ld._print_debug = False
        ld.create_training_dataframe()
        ld.dispatch_worker()
        return [ld.grab_next_batch() for _ in range(3)]

    a, b, c, plain = batches(3, inpaint_masks=True), batches(3, inpaint_masks=True), batches(4, inpaint_masks=True), batches(3)
    differs = False
    for x, y, z, p in zip(a, b, c, plain):
        m = x["inpaint_mask"]
        assert m.dtype == F32 and tuple(m.shape) == (3,) + tuple(x["pixel_values"].shape[2:]) and m.is_contiguous()
        assert set(m.unique().tolist()) == {0.0, 1.0}
        for i in range(3):  # one rectangle: the ones fill their bounding box, which is a proper part of the image
            ys, xs = m[i].nonzero(as_tuple=True)
            box = (int(ys.max() - ys.min()) + 1) * (int(xs.max() - xs.min()) + 1)
            assert int(m[i].sum()) == box and 0 < box < m[i].numel()
        assert torch.equal(m, y["inpaint_mask"])
        differs |= z["inpaint_mask"].shape != m.shape or not torch.equal(z["inpaint_mask"], m)
        assert "inpaint_mask" not in p and sorted(p) == sorted(k for k in x if k != "inpaint_mask")
        assert all(torch.equal(p[k], x[k]) for k in p)  # the other entries are what they are without it
    assert differs
    both = batches(3, inpaint_masks=True, loss_masks=True)
    assert torch.equal(both[0]["inpaint_mask"], a[0]["inpaint_mask"]) and not torch.equal(both[0]["loss_mask"], both[0]["inpaint_mask"])
