"""IP-Adapter without a GPU: the reference (tests/ip_adapter_reference.py) against the oracle, the spec and its initialisation, the
checkpoint round trip, the bound exports and every refusal of the C calls (made before any HIP call: they return on a machine with no
device), the state builder's, train_step's and generate's refusals, the loader's embeddings and the train state's stepping store."""
import ctypes
import types

import pytest
import torch

from oracle import nets as onets
from tests import ip_adapter_reference as R
from tests import kernel_checks as kc
from tests.helpers import make_case, rel_l2

BF, F32 = torch.bfloat16, torch.float32
E, T = 64, 4


def _tiny_ip():
    from stable_diffusion_training_amd import nets
    return nets.ip_adapter_config(nets.unet_config("tiny"), E, T)


# ================================================================================================ the reference
def test_reference_block_with_zero_to_v_ip_is_the_oracle_block():
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=2, image=64)
    ucfg, uw = case["cfgs"]["unet"], case["weights"]["unet"]
    icfg = nets.ip_adapter_config(ucfg, E, T)
    iw = nets.init_params(nets.ip_adapter_spec(icfg), 6)
    g = torch.Generator().manual_seed(1)
    name, C = "mid_block/attentions_0", ucfg["block_out_channels"][-1]
    x, ctx = torch.randn(2, 4, 4, C, generator=g), torch.randn(2, 77, ucfg["cross_attention_dim"], generator=g)
    tokens = R.image_tokens(iw, icfg, torch.randn(2, E, generator=g))
    assert tuple(tokens.shape) == (2, T, ucfg["cross_attention_dim"])
    assert float(tokens.mean(-1).abs().max()) < 0.2 and abs(float(tokens.std(-1).mean()) - 1.0) < 0.2  # LayerNorm over Dc (scale ~ 1)
    args = (name, 2, 1, ucfg["use_linear_projection"], ucfg["norm_num_groups"])
    plain = onets.transformer_2d(x, ctx, uw, *args)
    zero_v = {p: (torch.zeros_like(v) if "/to_v_ip/" in p else v) for p, v in iw.items()}
    with R.with_image_tokens(zero_v, tokens):
        same = onets.transformer_2d(x, ctx, uw, *args)
    with R.with_image_tokens(iw, tokens):
        moved = onets.transformer_2d(x, ctx, uw, *args)
    with R.with_image_tokens(iw, tokens, scale_ip=torch.zeros(2)):
        scaled = onets.transformer_2d(x, ctx, uw, *args)
    assert torch.equal(same, plain) and torch.equal(scaled, plain) and rel_l2(moved - x, plain - x) > 0.05
    assert onets._attn.__module__ == "oracle.nets", "with_image_tokens must restore the oracle"


def test_expected_bits_on_a_hand_case_and_its_assertions():
    """ip_expect_bits on a selector case: out is o_txt + scale_ip * (the target's V row) rounded once; dq is dq_in (dS = 0); dV is
    the scatter of scale_ip * dout.  A case whose sums are not exact in fp32 is refused."""
    B, H, Nq, Tk, D = 2, 2, 9, 4, 16
    case = kc.selector_case(B, H, Nq, Tk, D, False, 5)
    o_txt = torch.randn(B, Nq, H * D, generator=torch.Generator().manual_seed(2)).to(BF)
    sip = torch.tensor([2.5, 2.0 ** -10])
    e = R.ip_expect_bits(case, B, H, Nq, Tk, D, D ** -0.5, o_txt=o_txt, dq_in=o_txt, scale_ip=sip)
    v4 = case["v"].view(B, Tk, H, D)
    pick = torch.stack([torch.stack([v4[b, case["target"][b, h], h] for h in range(H)], 1) for b in range(B)]).reshape(B, Nq, H * D)
    want = R.bf16_rne_f64(o_txt.double() + sip.double().view(B, 1, 1) * pick.double())
    assert torch.equal(e["out"].view(torch.int16), want.view(torch.int16))
    assert torch.equal(e["dq"].view(torch.int16), o_txt.view(torch.int16)) and int(torch.count_nonzero(e["dkv"][..., : H * D])) == 0
    assert int(torch.count_nonzero(e["dkv"][..., H * D:])) > 0
    wide = case["v"].float().view(B, Tk, H, D).clone()  # one feature at 2^20, its neighbour at 2^-7: g.v no longer fits 24 bits
    wide[..., 0] = (wide[..., 0].abs() + 1) * 2.0 ** 20
    wide[..., 1] = (wide[..., 1].abs() + 1) * 2.0 ** -7
    with pytest.raises(AssertionError, match="not exact in fp32"):
        R.ip_expect_bits(dict(case, v=wide.reshape(B, Tk, H * D).to(BF)), B, H, Nq, Tk, D, D ** -0.5)
    # one rounding, not two: 1 + 2^-8 + 2^-30 lies above the tie and rounds up
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert R.bf16_rne_f64(x).double().tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6]


def test_exact_cases_lead_by_more_than_fp32_exp_underflow():
    for (B, H, Nq, Tk, D) in [(2, 2, 70, 4, 40), (1, 3, 130, 16, 64), (1, 2, 257, 5, 160), (2, 8, 64, 4, 160)]:
        for case in (kc.selector_case(B, H, Nq, Tk, D, False, 3), kc.pair_case(B, H, Nq, Tk, D, 4)):
            assert R.min_lead(case, B, H, Nq, Tk, D, D ** -0.5) >= 161.9


# ================================================================================================ spec and initialisation
@pytest.mark.parametrize("name,ctx,widths", [("sd15", 768, {320: 5, 640: 5, 1280: 6}), ("sd21", 1024, {320: 5, 640: 5, 1280: 6}),
                                             ("sdxl", 2048, {640: 10, 1280: 60})])
def test_spec_names_and_shapes(name, ctx, widths):
    from stable_diffusion_training_amd import nets
    cfg = nets.ip_adapter_config(nets.unet_config(name), 1024, 4)
    spec = nets.ip_adapter_spec(cfg)
    assert spec[:4] == [("image_proj/proj/kernel", (1024, 4 * ctx)), ("image_proj/proj/bias", (4 * ctx,)),
                        ("image_proj/norm/scale", (ctx,)), ("image_proj/norm/bias", (ctx,))]
    assert {w: len(v) for w, v in nets.ip_adapter_blocks(cfg).items()} == widths
    rest = spec[4:]
    assert len(rest) == 2 * sum(widths.values()) and len({p for p, _ in spec}) == len(spec)
    unet = dict(nets.unet_spec(nets.unet_config(name)))
    for i in range(0, len(rest), 2):  # [k | v] pairs of one block, back to back; widths do not interleave
        (pk, sk), (pv, sv) = rest[i], rest[i + 1]
        assert pk.endswith("/attn2/to_k_ip/kernel") and pv == pk.replace("/to_k_ip/", "/to_v_ip/") and sk == sv
        assert sk == tuple(unet[pk.replace("/to_k_ip/", "/to_k/")]) and sk[0] == ctx
    seen = [s[1] for _, s in rest]
    assert seen == sorted(seen, key=list(widths).index), "the leaves of one width must lie together"
    plus = nets.ip_adapter_config(nets.unet_config(name), 1280, 16)
    assert nets.ip_adapter_spec(plus)[0] == ("image_proj/proj/kernel", (1280, 16 * ctx))


def test_config_refusals():
    from stable_diffusion_training_amd import nets
    u = nets.unet_config("tiny")
    for kw, match in ((dict(num_tokens=0), "num_tokens"), (dict(num_tokens=17), "num_tokens"), (dict(image_embed_dim=60), "image_embed_dim"),
                      (dict(image_embed_dim=0), "image_embed_dim")):
        with pytest.raises(ValueError, match=match):
            nets.ip_adapter_config(u, **kw)
    with pytest.raises(ValueError, match="inpainting UNet"):
        nets.ip_adapter_config(nets.unet_config("tiny", in_channels=9))


def test_from_unet_copies_to_k_and_to_v():
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=2, image=64)
    cfg, uw = _tiny_ip(), case["weights"]["unet"]
    w = nets.ip_adapter_from_unet(uw, cfg, seed=3)
    assert list(w) != [] and set(w) == {p for p, _ in nets.ip_adapter_spec(cfg)}
    for p, v in w.items():
        if p.startswith("image_proj/"):
            continue
        src = uw[p.replace("_ip/", "/")]
        assert torch.equal(v, src) and v.data_ptr() != src.data_ptr()
    again, other = nets.ip_adapter_from_unet(uw, cfg, seed=3), nets.ip_adapter_from_unet(uw, cfg, seed=4)
    assert torch.equal(w["image_proj/proj/kernel"], again["image_proj/proj/kernel"])
    assert not torch.equal(w["image_proj/proj/kernel"], other["image_proj/proj/kernel"])
    bad = dict(uw)
    k = next(p for p in uw if p.endswith("/attn2/to_k/kernel"))
    bad[k] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="has shape"):
        nets.ip_adapter_from_unet(bad, cfg)


def test_checkpoint_round_trip(tmp_path):
    from stable_diffusion_training_amd import checkpoint as ck
    from stable_diffusion_training_amd import nets
    cfg = _tiny_ip()
    w = nets.init_params(nets.ip_adapter_spec(cfg), 2)
    ck.save_ip_adapter(str(tmp_path / "ip"), w, cfg)
    back = ck.load_ip_adapter(str(tmp_path / "ip"))
    assert back["config"]["image_embed_dim"] == E and back["config"]["num_tokens"] == T
    assert back["config"]["block_out_channels"] == cfg["block_out_channels"]
    assert set(back["params"]) == set(w) and all(torch.equal(back["params"][p], w[p]) for p in w)
    assert nets.ip_adapter_spec(back["config"]) == nets.ip_adapter_spec(cfg)
    ck.save_controlnet(str(tmp_path / "cn"), {"a/kernel": torch.zeros(2, 2)}, nets.unet_config("tiny"))
    with pytest.raises(ValueError, match="not an IP-Adapter directory"):
        ck.load_ip_adapter(str(tmp_path / "cn"))


def test_save_model_refuses_an_ip_adapter_store_as_unet_weights(tmp_path):
    from stable_diffusion_training_amd import checkpoint as ck
    from stable_diffusion_training_amd.params import EmaView
    store = types.SimpleNamespace(ip_adapter_config=_tiny_ip(), ema=None)
    view = EmaView.__new__(EmaView)
    view.store = store
    for wrong in (store, view, types.SimpleNamespace(store=store)):
        with pytest.raises(ValueError, match="IP-Adapter's store, not a UNet"):
            ck.save_model({}, None, wrong, None, None, str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


# ================================================================================================ the C ABI
def test_exports_bound_and_abi_5(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_abi_version() == 5
    for name, n in (("sdt_ip_attention_fwd", 14), ("sdt_ip_attention_bwd", 19)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name]) == n and len(getattr(lib, name).argtypes) == n
    assert len(_lib.WS_QUERY["sdt_ip_attention_bwd_workspace_bytes"]) == 5
    need = lib.sdt_ip_attention_bwd_workspace_bytes(1, 8, 4100, 4, 40)
    assert need > kc.CNT_BYTES and (need - kc.CNT_BYTES) % (4 * 2 * 320 * 4) == 0
    assert lib.sdt_ip_attention_bwd_workspace_bytes(1, 8, 4100, 17, 40) == -1 and b"T=17" in lib.sdt_last_error()


def test_every_c_refusal_returns_before_a_hip_call(lib):
    """No device is needed (and none is touched): each call returns SDT_ERR_INVALID_ARG with its message."""
    buf = (ctypes.c_uint16 * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = dict(B=1, H=2, Nq=4, T=4, D=8)

    def fwd(q=a, kv=a, o=a, s=None, out=a, ldq=16, ldkv=32, **over):
        d = dict(ok, **over)
        return lib.sdt_ip_attention_fwd(q, kv, o, s, out, d["B"], d["H"], d["Nq"], d["T"], d["D"], ldq, ldkv, 0.35, None)

    def bwd(q=a, kv=a, do=a, s=None, di=None, dq=a, dkv=a, ldq=16, ldkv=32, ld_dkv=32, ws=a, wsb=1 << 20, **over):
        d = dict(ok, **over)
        return lib.sdt_ip_attention_bwd(q, kv, do, s, di, dq, dkv, d["B"], d["H"], d["Nq"], d["T"], d["D"], ldq, ldkv, ld_dkv, 0.35, ws, wsb, None)

    cases = [(lambda: fwd(q=None), "null pointer"), (lambda: fwd(kv=None), "null pointer"), (lambda: fwd(out=None), "null pointer"),
             (lambda: fwd(T=0), "T=0"), (lambda: fwd(T=17), "T=17"), (lambda: fwd(D=12), "D=12"), (lambda: fwd(D=168), "D=168"),
             (lambda: fwd(D=0), "D=0"), (lambda: fwd(B=0), "must be positive"), (lambda: fwd(Nq=0), "must be positive"),
             (lambda: fwd(H=300), "wider than 2048"), (lambda: fwd(ldq=8), "narrower"), (lambda: fwd(ldkv=24), "narrower"),
             (lambda: fwd(q=a + 1), "misaligned"), (lambda: fwd(out=a + 1), "misaligned"), (lambda: fwd(s=a + 2), "misaligned"),
             (lambda: bwd(do=None), "null pointer"), (lambda: bwd(dq=None), "null pointer"), (lambda: bwd(dkv=None), "null pointer"),
             (lambda: bwd(ws=None), "null pointer"), (lambda: bwd(T=17), "T=17"), (lambda: bwd(D=4), "D=4"), (lambda: bwd(ld_dkv=16), "narrower"),
             (lambda: bwd(di=a + 1), "misaligned"), (lambda: bwd(ws=a + 4), "misaligned"), (lambda: bwd(wsb=65536), "workspace of 65536 bytes")]
    for call, match in cases:
        assert call() == -1, match
        assert match in lib.sdt_last_error().decode(), (match, lib.sdt_last_error())


def test_attention_ip_refuses_a_scale_beside_a_kv_ip_that_requires_grad():
    from stable_diffusion_training_amd import ops
    q, kv = torch.zeros(2, 4, 16, dtype=BF), torch.zeros(2, 4, 32, dtype=BF)
    with pytest.raises(ValueError, match="sampling only"):
        ops.attention_ip(q, kv, kv.clone().requires_grad_(True), 2, 0.35, scale_ip=torch.ones(2))


# ================================================================================================ the state builders
def _models(case, unet_cfg=None):
    return {"unet": {"unet_params": case["weights"]["unet"], "config": unet_cfg or case["cfgs"]["unet"]},
            "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
            "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}


def test_state_builder_refusals():
    from stable_diffusion_training_amd import lora, nets, tokens
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    cfg = _tiny_ip()
    build = lambda ip, models=None, **kw: tu.create_lion_optimizer_states(models or _models(case), device="cpu", ip_adapter=ip, **kw)
    for bad in ("sd15", dict(params={}), dict(config=cfg, weights={})):
        with pytest.raises(ValueError, match="ip_adapter: None or dict"):
            build(bad)
    with pytest.raises(ValueError, match="beside a LoRA adapter"):
        build(dict(config=cfg), lora=dict(unet=lora.LoraConfig(4, 4.0), text_encoder="frozen"))
    with pytest.raises(ValueError, match="beside new tokens"):
        build(dict(config=cfg), new_tokens=tokens.TokenConfig(num_tokens=1))
    with pytest.raises(ValueError, match="beside a ControlNet"):
        build(dict(config=cfg), controlnet=dict(config=nets.controlnet_config(nets.unet_config("tiny"), (16, 16, 32, 32))))
    with pytest.raises(ValueError, match="needs both states"):
        build(dict(config=cfg), train_text_encoder=False)
    cfg9 = nets.unet_config("tiny", in_channels=9)
    with pytest.raises(ValueError, match="inpainting UNet"):
        build(dict(config=dict(cfg, in_channels=9)), models=_models(case, cfg9))
    with pytest.raises(ValueError, match="needs image_embed_dim and num_tokens"):
        build(dict(config=nets.unet_config("tiny")))
    with pytest.raises(ValueError, match="num_tokens"):
        build(dict(config=dict(cfg, num_tokens=32)))
    with pytest.raises(ValueError, match="differs from the UNet's"):
        build(dict(config=nets.ip_adapter_config(nets.unet_config("tiny", block_out_channels=(32, 96)), E, T)))


def test_train_state_steps_the_adapter_store_only():
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.checkpoint import _stepping_store
    base = types.SimpleNamespace(trainable=False, count=0)
    istore = types.SimpleNamespace(trainable=True, count=3)
    st = tu.TrainState(None, base, {}, {}, ip_adapter=nets.IPAdapter(istore, {}))
    assert st.opt_store is istore and st.step == 3 and tu._stepping_stores(st) == [istore]
    assert _stepping_store(st) == (istore, None)
    assert tu.TrainState(None, base, {}, {}).opt_store is None and tu.TrainState(None, base, {}, {}).ip_adapter is None


# ================================================================================================ train_step's refusals
def _states(ip=True, trainable=False, text_trainable=False, cin=4, **unet_extra):
    from stable_diffusion_training_amd import nets
    cpu = torch.device("cpu")
    ipa = nets.IPAdapter(types.SimpleNamespace(device=cpu, trainable=True), dict(image_embed_dim=E, num_tokens=T)) if ip else None
    us = types.SimpleNamespace(config=dict(in_channels=cin, out_channels=4, addition_embed_type=None),
                               store=types.SimpleNamespace(device=cpu, trainable=trainable), adapter=None, tokens=None, controlnet=None, ip_adapter=ipa)
    ts = types.SimpleNamespace(config={}, store=types.SimpleNamespace(device=cpu, trainable=text_trainable), adapter=None, tokens=None,
                               controlnet=None, ip_adapter=None)
    for k, v in unet_extra.items():
        setattr(us, k, v)
    return us, ts


def test_train_step_refusals_before_touching_a_device():
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    assert tu.IP_KEYS == ("image_embeds",)
    sched = types.SimpleNamespace(call=None, params=None)
    px, emb = torch.zeros(2, 3, 16, 16), torch.zeros(2, E)
    good = dict(pixel_values=px, image_embeds=emb)

    def step(batch, reducer=None, **kw):
        us, ts = _states(**kw)
        return tu.train_step(us, ts, None, None, batch, None, "vae", sched, reducer=reducer)

    with pytest.raises(ValueError, match="IP-Adapter: data-parallel training is not supported"):
        step(good, reducer=object())
    with pytest.raises(ValueError, match="LoRA adapter or new tokens beside an IP-Adapter"):
        step(good, adapter=object())
    with pytest.raises(ValueError, match="ControlNet"):
        step(good, controlnet=nets.ControlNet(types.SimpleNamespace(device=torch.device("cpu"), trainable=True), {}))
    with pytest.raises(ValueError, match="IP-Adapter: an inpainting UNet is not supported"):
        step(dict(good, inpaint_mask=torch.zeros(2, 16, 16)), cin=9)
    with pytest.raises(ValueError, match="IP-Adapter: a trainable base store"):
        step(good, trainable=True)
    with pytest.raises(ValueError, match="IP-Adapter: a trainable base store"):
        step(good, text_trainable=True)
    with pytest.raises(ValueError, match="image_embeds need an IP-Adapter state"):
        step(good, ip=False, trainable=True, text_trainable=True)
    with pytest.raises(ValueError, match="batch needs image_embeds"):
        step(dict(pixel_values=px))
    bad = [(emb.double(), "must be a float32 or bfloat16 tensor"), (emb.numpy(), "must be a float32 or bfloat16 tensor"),
           (emb.to("meta"), "live on"), (torch.zeros(2, E + 8), "have shape"), (torch.zeros(1, E), "have shape"),
           (torch.zeros(2, 1, E), "have shape"), (torch.zeros(2, 2 * E)[:, ::2], "must be contiguous")]
    for e, match in bad:
        with pytest.raises(ValueError, match=match):
            step(dict(pixel_values=px, image_embeds=e))
    with pytest.raises(ValueError, match=r"have shape .*\(2, 64\)"):
        step(dict(latent_moments=torch.zeros(2, 2, 3, 8, dtype=BF), image_embeds=torch.zeros(3, E)))
    cpu = torch.device("cpu")
    us, _ = _states()
    tu._check_ip_entries(dict(image_embeds=emb), us.ip_adapter, cpu, 2)
    tu._check_ip_entries(dict(image_embeds=emb.to(BF)), us.ip_adapter, cpu, 2)
    tu._check_ip_entries(dict(), None, cpu, 2)


# ================================================================================================ generate's refusals
def _pipe(ip, cin=4):
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    p = StableDiffusionPipeline.__new__(StableDiffusionPipeline)  # (the constructor needs a device; the checks read these attributes only)
    p.unet_config = nets.unet_config("tiny", in_channels=cin)
    p.vae_config, p.vae_scale_factor, p.device = nets.vae_config("tiny"), 8, torch.device("cpu")
    p.controlnet = None
    p.ip_adapter = nets.IPAdapter(None, _tiny_ip()) if ip else None
    return p


def test_generate_refusals_before_touching_a_device():
    import inspect
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    ids = torch.zeros(2, 77, dtype=torch.int32)
    emb = torch.zeros(2, E)
    with pytest.raises(ValueError, match="need a pipeline built with ip_adapter="):
        _pipe(False).generate(ids, 2, 64, 64, image_embeds=emb)
    with pytest.raises(ValueError, match="samples from image_embeds"):
        _pipe(True).generate(ids, 2, 64, 64)
    for bad in (torch.zeros(2, E + 8), torch.zeros(1, E), torch.zeros(2, 1, E), emb.numpy()):
        with pytest.raises(ValueError, match="Unexpected image_embeds shape"):
            _pipe(True).generate(ids, 2, 64, 64, image_embeds=bad)
    sig = inspect.signature(StableDiffusionPipeline.__init__).parameters
    assert sig["ip_adapter"].default is None
    gen = inspect.signature(StableDiffusionPipeline.generate).parameters
    assert gen["image_embeds"].default is None and gen["ip_scale"].default == 1.0


# ================================================================================================ the loader and the cache
def test_loader_emits_image_embeds_and_honours_the_drop_rate():
    from stable_diffusion_training_amd import latent_cache
    from stable_diffusion_training_amd.streamer import DataLoader

    def first(n, drop=0.0, bs=2):
        ld = DataLoader(training_batch_size=bs, repeat_batch=1, maximum_resolution_areas=[64 ** 2], bucket_lower_bound_resolutions=[64],
                        batches_per_chunk=2, vocab_size=1000, seed=3, image_embeds=n, image_embed_drop_rate=drop)
        ld._print_debug = False
        ld.create_training_dataframe()
        ld.dispatch_worker()
        return ld.grab_next_batch()

    plain, with_e = first(0), first(E)
    assert "image_embeds" not in plain
    e = with_e["image_embeds"]
    assert tuple(e.shape) == (2, E) and e.dtype == F32 and e.is_contiguous() and float(e.std()) > 0.5 and not torch.equal(e[0], e[1])
    assert all(torch.equal(with_e[k], plain[k]) for k in plain), "the embeddings changed another entry"
    assert torch.equal(first(E)["image_embeds"], e)
    assert int((first(E, drop=1.0)["image_embeds"].abs().sum(1) == 0).sum()) == 2
    some = first(E, drop=0.5, bs=64)["image_embeds"]
    dropped = int((some.abs().sum(1) == 0).sum())
    assert 12 <= dropped <= 52, dropped  # 64 draws at p = 1/2: outside this range with probability < 1e-6
    kept = some[some.abs().sum(1) != 0]
    assert torch.equal(kept, first(E, bs=64)["image_embeds"][some.abs().sum(1) != 0]), "a dropped sample must not disturb the others"
    for bad in (dict(n=-1), dict(n=True), dict(n=E, drop=1.5)):
        with pytest.raises(ValueError, match="image_embed"):
            first(**bad)
    assert "image_embeds" in latent_cache.EXTRA_KEYS
