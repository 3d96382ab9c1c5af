"""ControlNet without a GPU: the CPU reference against the oracle UNet, the parameter spec, controlnet_from_unet, the config's
refusals, the checkpoint round trip, the export and its host refusals, and every ValueError of the state builders, train_step and
generate that needs no device."""
import types

import numpy as np
import pytest
import torch

from tests import controlnet_reference as cr
from tests.helpers import make_case

BF, F32 = torch.bfloat16, torch.float32
TINY_CH = (16, 16, 32, 32)


def _tiny(**over):
    from stable_diffusion_training_amd import nets
    return nets.controlnet_config(nets.unet_config("tiny", **over), TINY_CH)


# ================================================================================================ the reference itself
def test_reference_unet_with_zero_residuals_is_the_oracle_unet():
    from oracle import nets as onets
    case = make_case("tiny", B=2, image=64)
    cfg, w = dict(case["cfgs"]["unet"], conditioning_embedding_out_channels=TINY_CH, conditioning_channels=3), case["weights"]["unet"]
    g = torch.Generator().manual_seed(3)
    x, t, ctx = torch.randn(2, 4, 8, 8, generator=g), torch.tensor([11, 950]), torch.randn(2, 77, 48, generator=g)
    cond = torch.rand(2, 3, 64, 64, generator=g)
    want = onets.unet_forward(w, cfg, x, t, ctx)
    assert torch.equal(cr.unet_forward(w, cfg, x, t, ctx), want)
    cw = cr.random_controlnet(w, cfg, seed=5, zero_std=0.0)
    down, mid = cr.controlnet_forward(cw, cfg, x, t, ctx, cond)
    assert len(down) == 4 and all(float(d.abs().max()) == 0 for d in down) and float(mid.abs().max()) == 0
    assert [tuple(d.shape) for d in down] == [(2, 8, 8, 32), (2, 8, 8, 32), (2, 4, 4, 32), (2, 4, 4, 64)] and tuple(mid.shape) == (2, 4, 4, 64)
    assert torch.equal(cr.unet_forward(w, cfg, x, t, ctx, down=down, mid=mid), want)
    # random zero convolutions move the prediction, and a zero scale takes them out again
    cw = cr.random_controlnet(w, cfg, seed=5)
    down, mid = cr.controlnet_forward(cw, cfg, x, t, ctx, cond)
    assert float(mid.abs().max()) > 0 and not torch.equal(cr.unet_forward(w, cfg, x, t, ctx, down=down, mid=mid), want)
    assert torch.equal(cr.unet_forward(w, cfg, x, t, ctx, down=down, mid=mid, scale=torch.zeros(2)), want)


def test_reference_rounding_is_one_rne_rounding():
    """rne_bf16_bits against torch's float32 -> bfloat16 cast on values float32 holds exactly, and on the midpoints of neighbouring
    bf16 values and their float64 neighbours, which a cast through float32 would round twice."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(50000, generator=g) * torch.exp2(torch.randint(-140, 127, (50000,), generator=g).float())
    x = torch.cat([x, torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-45, 2.0 ** -134, 1.5 * 2.0 ** -134, 2.0 ** -133, 3.4e38, -3.4e38])])
    want = x.to(BF).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(cr.rne_bf16_bits(x.double().numpy()), want)
    val = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    lo = np.arange(0, 0x7F80, dtype=np.uint16)
    hi_v = val(lo + 1)
    hi_v[-1] = 2.0 ** 128
    mid = (val(lo) + hi_v) / 2
    even = np.where(lo % 2 == 0, lo, lo + 1)
    assert np.array_equal(cr.rne_bf16_bits(mid), even) and np.array_equal(cr.rne_bf16_bits(-mid), even | 0x8000)
    assert np.array_equal(cr.rne_bf16_bits(np.nextafter(mid, 0.0)), lo) and np.array_equal(cr.rne_bf16_bits(np.nextafter(mid, np.inf)), lo + 1)
    assert cr.rne_bf16_bits(np.array([np.nan, 1e300, -1e300])).tolist() == [0x7FC0, 0x7F80, 0xFF80]
    # 1 + 2^-8 + 2^-30: float32 rounds it to the midpoint 1 + 2^-8, a second rounding would go to even (1.0); one rounding goes up
    assert cr.rne_bf16_bits(np.array([1 + 2.0 ** -8 + 2.0 ** -30])).tolist() == [0x3F81]
    got = cr.control_add_bits(np.array([[7]], np.uint16), np.array([[0x3F80]], np.uint16), np.array([[0x3B80]], np.uint16), None, 1)
    assert got.tolist() == [[7, 0x3F80]]  # 1 + 2^-8 ties to even


# ================================================================================================ spec
@pytest.mark.parametrize("name,ch,n_down", [("tiny", TINY_CH, 4), ("sd15", (16, 32, 96, 256), 12)])
def test_spec_names_and_shapes(name, ch, n_down):
    from stable_diffusion_training_amd import nets
    cfg = nets.controlnet_config(nets.unet_config(name), ch)
    spec = nets.controlnet_spec(cfg)
    got = dict(spec)
    assert len(got) == len(spec), "a leaf appears twice"
    assert {p: tuple(s) for p, s in got.items()} == {p: tuple(s) for p, s in cr.param_shapes(cfg).items()}
    unet = dict(nets.unet_spec(cfg))
    shared = [p for p in got if not p.startswith("controlnet_")]
    assert shared and all(tuple(unet[p]) == tuple(got[p]) for p in shared)
    assert not any(p.startswith(("up_blocks_", "conv_out", "conv_norm_out")) for p in got)
    downs = sorted({p.split("/")[0] for p in got if p.startswith("controlnet_down_blocks_")}, key=lambda s: int(s.rsplit("_", 1)[1]))
    assert downs == [f"controlnet_down_blocks_{i}" for i in range(n_down)]
    boc = cfg["block_out_channels"]
    assert [got[d + "/kernel"][2] for d in downs] == cr.skip_channels(cfg) and got["controlnet_mid_block/kernel"] == (1, 1, boc[-1], boc[-1])
    e = "controlnet_cond_embedding"
    assert got[e + "/conv_in/kernel"] == (3, 3, 3, ch[0]) and got[e + "/conv_out/kernel"] == (3, 3, ch[-1], boc[0])
    for k in range(3):
        assert got[f"{e}/blocks_{2 * k}/kernel"] == (3, 3, ch[k], ch[k]) and got[f"{e}/blocks_{2 * k + 1}/kernel"] == (3, 3, ch[k], ch[k + 1])
    assert f"{e}/blocks_6/kernel" not in got
    # the deferred groups sit together: time_emb_proj kernels of one width are adjacent
    paths = [p for p, _ in spec]
    tp = [i for i, p in enumerate(paths) if p.endswith("/time_emb_proj/kernel") and got[p][1] == boc[0]]
    assert tp == list(range(tp[0], tp[0] + len(tp)))


def test_text_time_spec_has_the_add_embedding():
    from stable_diffusion_training_amd import nets
    cfg = _tiny(addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=64)
    got = dict(nets.controlnet_spec(cfg))
    assert got["add_embedding/linear_1/kernel"] == (64, 128) and got["add_embedding/linear_2/kernel"] == (128, 128)


# ================================================================================================ controlnet_from_unet
def test_controlnet_from_unet_copies_and_zeroes():
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.checkpoint import unflatten_tree
    case = make_case("tiny", B=2, image=64)
    cfg, w = _tiny(), case["weights"]["unet"]
    tree = nets.controlnet_from_unet(w, cfg, seed=4)
    assert set(tree) == {p for p, _ in nets.controlnet_spec(cfg)}
    zero = set(nets.controlnet_zero_leaves(cfg))
    assert "controlnet_cond_embedding/conv_out/kernel" in zero and "controlnet_mid_block/bias" in zero and len(zero) == 2 * (4 + 2)
    for p, v in tree.items():
        if p in zero:
            assert float(v.abs().max()) == 0, p
        elif p.startswith("controlnet_"):
            assert float(v.abs().max()) > 0, p
        else:
            assert torch.equal(v, w[p]) and v.data_ptr() != w[p].data_ptr(), p
    again, other = nets.controlnet_from_unet(w, cfg, seed=4), nets.controlnet_from_unet(w, cfg, seed=5)
    k = "controlnet_cond_embedding/blocks_1/kernel"
    assert torch.equal(tree[k], again[k]) and not torch.equal(tree[k], other[k])
    nested = nets.controlnet_from_unet(unflatten_tree({p: v.numpy() for p, v in w.items()}), cfg, seed=4)
    assert all(torch.equal(nested[p], tree[p]) for p in tree)


# ================================================================================================ config
def test_config_refusals():
    from stable_diffusion_training_amd import nets
    u = nets.unet_config("tiny")
    cfg = nets.controlnet_config(u)
    assert cfg["conditioning_embedding_out_channels"] == (16, 32, 96, 256) and cfg["conditioning_channels"] == 3
    assert {k: cfg[k] for k in u} == u
    with pytest.raises(ValueError, match="entries"):
        nets.controlnet_config(u, (16, 32, 96))
    with pytest.raises(ValueError, match="entries"):
        nets.controlnet_config(u, (16, 32, 96, 256, 256))
    assert nets.controlnet_config(u, (16, 32, 96), vae_downscale=4)["conditioning_embedding_out_channels"] == (16, 32, 96)
    with pytest.raises(ValueError, match="multiples of 8"):
        nets.controlnet_config(u, (16, 32, 100, 256))
    with pytest.raises(ValueError, match="multiples of 8"):
        nets.controlnet_config(u, (16, 0, 96, 256))
    with pytest.raises(ValueError, match="conditioning_channels"):
        nets.controlnet_config(u, conditioning_channels=0)
    with pytest.raises(ValueError, match="inpainting"):
        nets.controlnet_config(nets.unet_config("tiny", in_channels=9))


# ================================================================================================ checkpoint
def test_save_and_load_controlnet_round_trip(tmp_path):
    import json
    from stable_diffusion_training_amd import checkpoint as ck
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=2, image=64)
    cfg = _tiny()
    tree = cr.random_controlnet(case["weights"]["unet"], cfg, seed=2)
    ck.save_controlnet(str(tmp_path / "cn"), tree, cfg)
    raw = json.load(open(tmp_path / "cn" / "config.json"))
    assert raw["_class_name"] == "FlaxControlNetModel" and raw["conditioning_embedding_out_channels"] == list(TINY_CH)
    back = ck.load_controlnet(str(tmp_path / "cn"))
    assert back["config"]["conditioning_embedding_out_channels"] == TINY_CH and back["config"]["conditioning_channels"] == 3
    assert back["config"]["block_out_channels"] == cfg["block_out_channels"]
    assert set(back["params"]) == set(tree) and all(torch.equal(back["params"][p], tree[p]) for p in tree)
    assert [p for p, _ in nets.controlnet_spec(back["config"])] == [p for p, _ in nets.controlnet_spec(cfg)]
    ck.save_model({"unet": case["cfgs"]["unet"], "vae": case["cfgs"]["vae"], "text_encoder": case["cfgs"]["clip"]}, None,
                  case["weights"]["unet"], case["weights"]["clip"], case["weights"]["vae"], str(tmp_path / "pipe"))
    with pytest.raises(ValueError, match="not a ControlNet directory"):
        ck.load_controlnet(str(tmp_path / "pipe" / "unet"))


# ================================================================================================ the export
def test_export_is_bound_and_the_abi_is_5(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_abi_version() == 5
    sig = _lib.SIGNATURES["sdt_control_concat_add"]
    assert lib.sdt_control_concat_add.argtypes == sig and len(sig) == 10


def test_host_refusals_return_before_any_hip_call(lib):
    """Pointers are made-up aligned addresses: nothing dereferences them, every call returns nonzero with a message."""
    P = 4096
    err = lambda: lib.sdt_last_error()
    call = lambda a=P, skip=P, res=P, scale=P, wide=P, rows=6, rps=3, Ca=8, Cb=8: lib.sdt_control_concat_add(a, skip, res, scale, wide, rows, rps,
                                                                                                            Ca, Cb, None)
    for kw in (dict(skip=None), dict(res=None), dict(wide=None)):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    for kw in (dict(Cb=0), dict(Cb=-8), dict(Ca=-1)):
        assert call(**kw) != 0 and b"bad widths" in err(), kw
    assert call(a=None) != 0 and b"needs the left part" in err()
    for kw in (dict(rps=0), dict(rps=-3)):
        assert call(**kw) != 0 and b"at least 1" in err(), kw
    for kw in (dict(rows=7), dict(rows=6, rps=4), dict(rows=-3)):
        assert call(**kw) != 0 and b"not a multiple" in err(), kw
    assert call(rows=0) == 0 and call(rows=0, a=None, Ca=0, scale=None) == 0  # nothing to do: no launch


# ================================================================================================ the state builders
def _models(case, unet_cfg=None):
    return {"unet": {"unet_params": case["weights"]["unet"], "config": unet_cfg or case["cfgs"]["unet"]},
            "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
            "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}


def test_state_builder_refusals():
    from stable_diffusion_training_amd import lora, nets, tokens
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    cfg = _tiny()
    build = lambda cn, models=None, **kw: tu.create_lion_optimizer_states(models or _models(case), device="cpu", controlnet=cn, **kw)
    for bad in ("sd15", dict(params={}), dict(config=cfg, weights={})):
        with pytest.raises(ValueError, match="controlnet: None or dict"):
            build(bad)
    with pytest.raises(ValueError, match="beside a LoRA adapter or new tokens"):
        build(dict(config=cfg), lora=dict(unet=lora.LoraConfig(4, 4.0), text_encoder="frozen"))
    with pytest.raises(ValueError, match="beside a LoRA adapter or new tokens"):
        build(dict(config=cfg), new_tokens=tokens.TokenConfig(num_tokens=1))
    with pytest.raises(ValueError, match="needs both states"):
        build(dict(config=cfg), train_text_encoder=False)
    cfg9 = nets.unet_config("tiny", in_channels=9)
    with pytest.raises(ValueError, match="inpainting UNet"):
        build(dict(config=dict(cfg, in_channels=9)), models=_models(case, cfg9))
    with pytest.raises(ValueError, match="needs conditioning_embedding_out_channels"):
        build(dict(config=nets.unet_config("tiny")))
    with pytest.raises(ValueError, match="entries"):
        build(dict(config=dict(cfg, conditioning_embedding_out_channels=(16, 32))))
    with pytest.raises(ValueError, match="differs from the UNet's"):
        build(dict(config=nets.controlnet_config(nets.unet_config("tiny", block_out_channels=(32, 96)), TINY_CH)))
    # keys that change the network without changing a leaf shape count too
    for over in (dict(attention_head_dim=4), dict(norm_num_groups=16), dict(transformer_layers_per_block=2), dict(use_linear_projection=True)):
        with pytest.raises(ValueError, match=f"{next(iter(over))}=.* differs from the UNet's"):
            build(dict(config=nets.controlnet_config(nets.unet_config("tiny", **over), TINY_CH)))


def test_save_model_refuses_a_controlnet_store_as_unet_weights(tmp_path):
    from stable_diffusion_training_amd import checkpoint as ck
    from stable_diffusion_training_amd.params import EmaView
    store = types.SimpleNamespace(controlnet_config=_tiny(), ema=None)
    view = EmaView.__new__(EmaView)
    view.store = store
    for wrong in (store, view, types.SimpleNamespace(store=store)):
        with pytest.raises(ValueError, match="not a UNet"):
            ck.save_model({}, None, wrong, None, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_loader_emits_conditioning_images_of_the_asked_channel_count():
    from stable_diffusion_training_amd.streamer import DataLoader
    def first(ci):
        ld = DataLoader(training_batch_size=2, repeat_batch=1, maximum_resolution_areas=[64 ** 2], bucket_lower_bound_resolutions=[64],
                        batches_per_chunk=2, vocab_size=1000, seed=3, conditioning_images=ci)
        ld._print_debug = False
        ld.create_training_dataframe()
        ld.dispatch_worker()
        return ld.grab_next_batch()
    plain, three, one = first(False), first(True), first(1)
    assert "conditioning_pixel_values" not in plain
    c3, c1 = three["conditioning_pixel_values"], one["conditioning_pixel_values"]
    assert tuple(c3.shape) == (2, 3, 64, 64) and tuple(c1.shape) == (2, 1, 64, 64) and c3.dtype == F32 and c3.is_contiguous()
    assert 0.0 <= float(c3.min()) and float(c3.max()) <= 1.0 and float(c3.std()) > 0.1 and not torch.equal(c3[0], c3[1])
    assert all(torch.equal(three[k], plain[k]) for k in plain), "the conditioning image changed another entry"
    assert torch.equal(first(3)["conditioning_pixel_values"], c3)
    with pytest.raises(ValueError, match="conditioning_images"):
        first(-1)


def test_train_state_steps_the_controlnet_store():
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.checkpoint import _stepping_store
    base = types.SimpleNamespace(trainable=False, count=0)
    cstore = types.SimpleNamespace(trainable=True, count=3)
    st = tu.TrainState(None, base, {}, {}, controlnet=nets.ControlNet(cstore, {}))
    assert st.opt_store is cstore and st.step == 3 and tu._stepping_stores(st) == [cstore]
    assert _stepping_store(st) == (cstore, None)
    assert tu.TrainState(None, base, {}, {}).opt_store is None


# ================================================================================================ train_step's refusals
def _ucfg():
    return dict(in_channels=4, out_channels=4, addition_embed_type=None)


def _states(controlnet=True, trainable=False, text_trainable=False, cin=4, **unet_extra):
    from stable_diffusion_training_amd import nets
    cpu = torch.device("cpu")
    cn = nets.ControlNet(types.SimpleNamespace(device=cpu, trainable=True),
                         dict(conditioning_channels=3, conditioning_embedding_out_channels=TINY_CH)) if controlnet else None
    us = types.SimpleNamespace(config=dict(_ucfg(), in_channels=cin), store=types.SimpleNamespace(device=cpu, trainable=trainable), adapter=None,
                               tokens=None, controlnet=cn)
    ts = types.SimpleNamespace(config={}, store=types.SimpleNamespace(device=cpu, trainable=text_trainable), adapter=None, tokens=None,
                               controlnet=None)
    for k, v in unet_extra.items():
        setattr(us, k, v)
    return us, ts


def test_train_step_refusals_before_touching_a_device():
    from stable_diffusion_training_amd import training_utils as tu
    assert tu.CONTROL_KEYS == ("conditioning_pixel_values",)
    sched = types.SimpleNamespace(call=None, params=None)
    px, cond = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    good = dict(pixel_values=px, conditioning_pixel_values=cond)

    def step(batch, reducer=None, **kw):
        us, ts = _states(**kw)
        return tu.train_step(us, ts, None, None, batch, None, "vae", sched, reducer=reducer)

    with pytest.raises(ValueError, match="data-parallel training is not supported"):
        step(good, reducer=object())
    with pytest.raises(ValueError, match="LoRA adapter or new tokens beside a ControlNet"):
        step(good, adapter=object())
    with pytest.raises(ValueError, match="inpainting UNet is not supported"):
        step(dict(good, inpaint_mask=torch.zeros(2, 16, 16)), cin=9)
    with pytest.raises(ValueError, match="trainable base store"):
        step(good, trainable=True)
    with pytest.raises(ValueError, match="trainable base store"):
        step(good, text_trainable=True)
    with pytest.raises(ValueError, match="need a ControlNet state"):
        step(good, controlnet=False, trainable=True, text_trainable=True)
    with pytest.raises(ValueError, match="batch needs conditioning_pixel_values"):
        step(dict(pixel_values=px))
    bad = [(cond.double(), "must be a float32 tensor"), (cond.numpy(), "must be a float32 tensor"), (cond.to("meta"), "live on"),
           (torch.zeros(2, 3, 2, 2), "have shape"), (torch.zeros(2, 1, 16, 16), "have shape"), (torch.zeros(1, 3, 16, 16), "have shape"),
           (torch.zeros(2, 3, 16, 32)[..., ::2], "must be contiguous"), (torch.zeros(2, 16, 16, 3).permute(0, 3, 1, 2), "must be contiguous")]
    for c, match in bad:
        with pytest.raises(ValueError, match=match):
            step(dict(pixel_values=px, conditioning_pixel_values=c))
    # cached: the hint is f times the latent size
    mom = torch.zeros(2, 2, 3, 8, dtype=BF)
    with pytest.raises(ValueError, match=r"have shape .*\(2, 3, 16, 24\)"):
        step(dict(latent_moments=mom, conditioning_pixel_values=cond))


def test_control_entries_accept_well_formed_batches():
    from stable_diffusion_training_amd import training_utils as tu
    cpu = torch.device("cpu")
    us, _ = _states()
    tu._check_control_entries(dict(pixel_values=torch.zeros(2, 3, 16, 24), conditioning_pixel_values=torch.zeros(2, 3, 16, 24)), us.controlnet, cpu)
    tu._check_control_entries(dict(latent_moments=torch.zeros(2, 2, 3, 8, dtype=BF), conditioning_pixel_values=torch.zeros(2, 3, 16, 24)),
                              us.controlnet, cpu)
    tu._check_control_entries(dict(pixel_values=torch.zeros(2, 3, 16, 24)), None, cpu)


def test_control_add_refuses_a_scale_beside_a_res_that_requires_grad():
    from stable_diffusion_training_amd import ops
    skip, res = torch.zeros(2, 4, 8, dtype=BF), torch.zeros(2, 4, 8, dtype=BF, requires_grad=True)
    with pytest.raises(ValueError, match="sampling only"):
        ops.control_add(None, skip, res, torch.ones(2))


# ================================================================================================ generate's refusals
def _pipe(controlnet, cin=4):
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    p = StableDiffusionPipeline.__new__(StableDiffusionPipeline)  # (the constructor needs a device; the checks read these attributes only)
    p.unet_config = nets.unet_config("tiny", in_channels=cin)
    p.vae_config, p.vae_scale_factor, p.device = nets.vae_config("tiny"), 8, torch.device("cpu")
    p.controlnet = nets.ControlNet(None, _tiny()) if controlnet else None
    return p


def test_generate_refusals_before_touching_a_device():
    ids = torch.zeros(2, 77, dtype=torch.int32)
    img = torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match="needs a pipeline built with controlnet="):
        _pipe(False).generate(ids, 2, 64, 64, control_image=img)
    with pytest.raises(ValueError, match="samples from a control_image"):
        _pipe(True).generate(ids, 2, 64, 64)
    for bad in (torch.zeros(2, 3, 32, 32), torch.zeros(1, 3, 64, 64), torch.zeros(2, 1, 64, 64), img.numpy()):
        with pytest.raises(ValueError, match="Unexpected control_image shape"):
            _pipe(True).generate(ids, 2, 64, 64, control_image=bad)
    with pytest.raises(ValueError, match="inpainting UNet is not supported"):
        _pipe(True, cin=9).generate(ids, 2, 64, 64, control_image=img, image=img, mask=torch.zeros(2, 64, 64))


def test_pipeline_takes_a_controlnet_and_generate_its_three_options():
    import inspect
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    sig = inspect.signature(StableDiffusionPipeline.__init__).parameters
    assert "controlnet" in sig and sig["controlnet"].default is None
    gen = inspect.signature(StableDiffusionPipeline.generate).parameters
    assert gen["control_image"].default is None and gen["conditioning_scale"].default == 1.0 and gen["control_negative"].default is True
