"""Training and sampling an IP-Adapter on the MI355X (tiny config, 64 x 64): one transformer block with image tokens teacher-forced
against the reference, unet_forward(ip=) forward and backward against the fp32 CPU reference (tests/ip_adapter_reference.py), the
zero-to_v_ip adapter and ip_scale = 0 against the plain UNet, the cached step against the pixel step, micro-batches, the captured
step, resume, the example loop and generate."""
import numpy as np
import pytest
import torch

from oracle import nets as onets
from tests import ip_adapter_reference as R
from tests import parity_check as pc
from tests.helpers import make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")
E, T = 64, 4
NOISE_KW = dict(min_snr_gamma_magnitude=5.0, offset_noise_magnitude=0.1, perturbation_noise_magnitude=0.1)  # test_gpu_inpaint.py's


def _ip_case(B=2, image=64, sched="scaled_linear", zero_v=False, from_unet=False, **unet_over):
    """make_case("tiny") plus an IP-Adapter: its config, its host weights (every leaf random unless from_unet; zero_v: to_v_ip zero) and
    image embeddings in the batch."""
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=B, image=image, sched=sched)
    if unet_over:
        ucfg = dict(case["cfgs"]["unet"], **unet_over)
        case["cfgs"] = dict(case["cfgs"], unet=ucfg)
        case["weights"] = dict(case["weights"], unet=onets.init_params(onets.unet_param_shapes(ucfg), 1))
    icfg = nets.ip_adapter_config(case["cfgs"]["unet"], E, T)
    case["ip_cfg"] = icfg
    w = nets.ip_adapter_from_unet(case["weights"]["unet"], icfg, seed=6) if from_unet else nets.init_params(nets.ip_adapter_spec(icfg), 6)
    if zero_v:
        w = {p: (torch.zeros_like(v) if "/to_v_ip/" in p else v) for p, v in w.items()}
    case["ip_weights"] = w
    g = torch.Generator().manual_seed(21)
    case["batch"] = dict(case["batch"], image_embeds=torch.randn(B, E, generator=g))
    return case


def _build(case, dev, *, prediction_type="epsilon", ema=False, params=True):
    from stable_diffusion_training_amd import training_utils as tu
    tc = tu.TrainingConfig(
        model_path="synthetic", batch_size=case["batch"]["pixel_values"].shape[0], learning_rate=1e-6, unet_learning_rate=1e-6,
        text_encoder_learning_rate=1e-6, lr_scheduler="constant", adam_to_lion_scale_factor=7.0, compilation_cache_path="",
        keep_compiled_fn_in_cache=False, text_encoder_context_window=77, context_window_concatenation_count=1, aot_compile=True,
        strip_bos_eos_token=False, offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0, perturbation_noise_magnitude=0.0,
        image_area_root=[512], minimum_axis_length=[512], beta_scheduler=case["sched"], prediction_type=prediction_type,
        excluded_layer_pattern_from_weight_decay=["bias", "scale", "embedding"],
        excluded_layer_from_quantization=["bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj"],
        quant_block_size=16, quantize_unet_state=True, quantize_text_encoder_state=True, accumulate_unet_ema=ema,
        accumulate_text_encoder_ema=ema, ema_rate=0.999)
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    ip = dict(config=case["ip_cfg"], params=case["ip_weights"]) if params else dict(config=case["ip_cfg"])
    return tc, tu.on_device_model_training_state(tc, models, device=dev, ip_adapter=ip)


def _snapshot(us, out):
    st = us.ip_adapter.store
    snap = {f"ip.{b}": getattr(st, b).clone() for b in STATE if getattr(st, b) is not None}
    snap["loss"] = out[4]["loss"].clone()
    snap["ip.sqnorm"] = st.sqnorm.clone()
    return snap


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b)


def _cos(a, b):
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


def _stores(case, dev):
    from stable_diffusion_training_amd import nets, params
    ust = params.ParamStore(nets.unet_spec(case["cfgs"]["unet"]), device=dev, trainable=False)
    ust.load(case["weights"]["unet"])
    ust.prepare()
    ist = params.ParamStore(nets.ip_adapter_spec(case["ip_cfg"]), device=dev, quantise=False)
    ist.load(case["ip_weights"])
    ist.prepare()
    ist.zero_grad()
    return ust, ist


def _inputs(case, seed=12, B=2, h=8, wd=8):
    g = torch.Generator().manual_seed(seed)
    ucfg = case["cfgs"]["unet"]
    return dict(x=torch.randn(B, 4, h, wd, generator=g), t=torch.tensor([17, 803]), ctx=torch.randn(B, 77, ucfg["cross_attention_dim"], generator=g),
                emb=case["batch"]["image_embeds"], r=torch.randn(B, 4, h, wd, generator=g))


# ================================================================================================ 1. one transformer block, teacher-forced
def test_transformer_block_with_image_tokens_teacher_forced(dev):
    """The mid block's transformer fed the oracle's own input and tokens, through parity_check.check_items at FWD_TOL / BWD_TOL: the
    output, the input and token gradients and the block's to_k_ip / to_v_ip gradients against the fp32 and the bf16-points oracle."""
    from stable_diffusion_training_amd import nets, ops
    case = _ip_case()
    ucfg, uw, iw = case["cfgs"]["unet"], case["weights"]["unet"], case["ip_weights"]
    name, C = "mid_block/attentions_0", ucfg["block_out_channels"][-1]
    heads = nets._per_block(ucfg["attention_head_dim"], len(ucfg["block_out_channels"]))[-1]
    lin, groups = ucfg["use_linear_projection"], ucfg["norm_num_groups"]
    x, ctx = pc.rand((2, 4, 4, C), 3), pc.rand((2, 77, ucfg["cross_attention_dim"]), 4)
    tok, dy = pc.rand((2, T, ucfg["cross_attention_dim"]), 5), pc.rand((2, 4, 4, C), 6, 0.1)
    weights = {k: v for k, v in {**uw, **iw}.items() if k.startswith(name + "/")}

    def block(p, xin, tokens):
        with R.with_image_tokens(p, tokens):
            return onets.transformer_2d(xin, ctx, p, name, heads, 1, lin, groups)

    ref = pc.oracle_run(block, weights, [x, tok], dy)
    plain = onets.transformer_2d(x, ctx, uw, name, heads, 1, lin, groups)
    assert rel_l2(ref["fp32"][0] - x, plain - x) > 0.05, "the image tokens do not move the reference block: the test would see nothing"
    ust, ist = _stores(case, dev)
    xd, td = x.to(dev).to(BF).requires_grad_(True), tok.to(dev).to(BF).requires_grad_(True)
    ops.gn_arena_begin(dev)
    cmap = nets._image_projections(ist, td, nets._context_projections(ust, ctx.to(dev).to(BF)), None)
    y, _ = nets._transformer(xd, cmap, ust, name, heads, 1, lin, groups)
    with ops.wgrad_grouping():
        y.backward(dy.to(dev).to(BF))
    ops.gn_arena_end(dev)
    (y32, dx32, dp32), (y16, dx16, dp16) = ref["fp32"], ref["bf16"]
    got = ist.export("grad")
    items = [("block output", y.detach(), y32, y16, pc.FWD_TOL), ("block dx", xd.grad, dx32[0], dx16[0], pc.BWD_TOL),
             ("d tokens", td.grad, dx32[1], dx16[1], pc.BWD_TOL)]
    ip_leaves = [k for k in weights if "_ip/" in k]
    assert len(ip_leaves) == 2
    items += [(f"d {k}", got[k], dp32[k], dp16[k], pc.BWD_TOL) for k in ip_leaves]
    worst = pc.check_items("transformer block with image tokens", items)
    print(f"[ip block] forward {worst[0]:.2e} (bf16-points oracle {worst[1]:.2e}), worst gradient {worst[2]:.2e} ({worst[3]:.2e})")


# ================================================================================================ 2. the whole UNet with the adapter
@pytest.mark.parametrize("variant", ["tiny", "tiny_wide"])
def test_unet_with_adapter_forward_and_backward_against_the_reference(dev, variant):
    """tiny: widths 32 and 64, every block projects its own image tokens.  tiny_wide: widths 64 and 128 - the three blocks of width 64
    share ONE to_k_ip / to_v_ip GEMM and read their [k|v] as column slices (row pitch 6 C), as every width of the real models does.
    Gates: the ControlNet test's - prediction rel-L2 < 2e-2, gradient cosine > 0.995 over all adapter kernels and > 0.99 on the
    image_proj leaves and on the to_k_ip / to_v_ip leaves as subsets."""
    from stable_diffusion_training_amd import nets
    case = _ip_case(**(dict(block_out_channels=(64, 128)) if variant == "tiny_wide" else {}))
    ucfg, icfg, uw, iw = case["cfgs"]["unet"], case["ip_cfg"], case["weights"]["unet"], case["ip_weights"]
    v = _inputs(case)
    q = lambda a: a.to(BF).float()
    wl = {k: a.clone().requires_grad_(True) for k, a in iw.items()}
    with R.with_image_tokens(wl, R.image_tokens(wl, icfg, q(v["emb"]))):
        ref = onets.unet_forward(uw, ucfg, q(v["x"]), v["t"], q(v["ctx"]))
    plain = onets.unet_forward(uw, ucfg, q(v["x"]), v["t"], q(v["ctx"]))
    assert rel_l2(ref.detach(), plain) > 0.05, "the image tokens do not move the reference prediction: the test would not see them"
    ust, ist = _stores(case, dev)
    first = nets.ip_adapter_blocks(icfg)[ucfg["block_out_channels"][0]]
    grouped = ist.mergeable(tuple(f"{n}/{t}/kernel" for n in first for t in ("to_k_ip", "to_v_ip")))
    assert len(first) == 3 and grouped == (variant == "tiny_wide"), "the variant does not take the path it is here for"
    xin = torch.zeros(2, 8, 8, 8, dtype=BF, device=dev)
    xin[..., :4] = v["x"].permute(0, 2, 3, 1).to(dev)
    tdev, cdev = v["t"].to(dev).to(torch.int32), v["ctx"].to(dev).to(BF)
    from stable_diffusion_training_amd import ops
    ops.gn_arena_begin(dev)
    tokens = nets.ip_adapter_tokens(ist, icfg, v["emb"].to(dev))
    pred = nets.unet_forward(ust, ucfg, xin, tdev, cdev, ip=(ist, tokens))
    assert rel_l2(pred[..., :4].permute(0, 3, 1, 2).detach(), ref.detach()) < 2e-2
    gref = dict(zip(wl, torch.autograd.grad((ref * v["r"]).sum(), list(wl.values()))))
    dpred = torch.zeros_like(pred)
    dpred[..., :4] = v["r"].permute(0, 2, 3, 1).to(dev)
    with ops.wgrad_grouping():
        pred.backward(dpred)
    ops.gn_arena_end(dev)
    got = ist.export("grad")
    flat = lambda keys, src: torch.cat([src[k].flatten().float().cpu() for k in keys])
    kernels = [k for k in gref if k.endswith("/kernel")]
    assert len(kernels) == 9
    assert _cos(flat(kernels, got), flat(kernels, gref)) > 0.995
    proj = [k for k in gref if k.startswith("image_proj/")]
    kv = [k for k in kernels if "/to_k_ip/" in k or "/to_v_ip/" in k]
    assert len(proj) == 4 and len(kv) == 8
    for name, keys in (("image_proj", proj), ("to_k_ip / to_v_ip", kv)):
        a, b = flat(keys, got), flat(keys, gref)
        assert float(a.abs().max()) > 0 and _cos(a, b) > 0.99, (name, _cos(a, b))
    for k in proj + kv:
        assert float(got[k].abs().max()) > 0, f"{k}: zero gradient"


# ================================================================================================ 3. adapters that must change nothing
def test_zero_to_v_ip_and_zero_ip_scale_reproduce_the_plain_unet(dev):
    from stable_diffusion_training_amd import nets, ops
    v = None
    preds = {}
    for name, zero_v, scale in (("zero to_v_ip", True, None), ("ip_scale 0", False, 0.0)):
        case = _ip_case(zero_v=zero_v)
        v = v or _inputs(case)
        ust, ist = _stores(case, dev)
        xin = torch.zeros(2, 8, 8, 8, dtype=BF, device=dev)
        xin[..., :4] = v["x"].permute(0, 2, 3, 1).to(dev)
        tdev, cdev = v["t"].to(dev).to(torch.int32), v["ctx"].to(dev).to(BF)
        with torch.no_grad():
            ops.gn_arena_begin(dev)
            plain = nets.unet_forward(ust, case["cfgs"]["unet"], xin, tdev, cdev)
            tokens = nets.ip_adapter_tokens(ist, case["ip_cfg"], v["emb"].to(dev))
            sip = None if scale is None else torch.full((2,), scale, dtype=F32, device=dev)
            preds[name] = nets.unet_forward(ust, case["cfgs"]["unet"], xin, tdev, cdev, ip=(ist, tokens, sip))
            ops.gn_arena_end(dev)
        assert torch.equal(preds[name], plain), f"{name}: the prediction moved"


# ================================================================================================ 4. cached against pixels
VARIANTS = {
    "a_epsilon_rand": dict(pred="epsilon", sched="scaled_linear", kw={}, rand=True),
    "b_vpred_noise_options_generator": dict(pred="v_prediction", sched="zero_snr_scaled_linear", kw=NOISE_KW, rand=False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cached_step_equals_the_pixel_step_bit_for_bit(dev, variant):
    from stable_diffusion_training_amd import training_utils as tu
    v = VARIANTS[variant]
    case = _ip_case(sched=v["sched"])
    snaps = []
    for cached in (False, True):
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, prediction_type=v["pred"], ema=True)
        assert ue is not None and ue.store is us.ip_adapter.store and te is None and us.opt_store is us.ip_adapter.store
        assert not us.store.trainable and not ts.store.trainable
        base_u = us.store.master.clone()
        batch = to_dev(case["batch"], dev)
        if cached:
            moments = tu.encode_latent_moments(vae, batch["pixel_values"]).contiguous()
            batch = {k: val for k, val in batch.items() if k != "pixel_values"}
            batch["latent_moments"], vae = moments, None
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999,
                            rand=to_dev(case["rand"], dev) if v["rand"] else None, **v["kw"])
        torch.cuda.synchronize()
        assert us.step == 1 and us.store.count == 0 and torch.equal(us.store.master, base_u), "the frozen UNet moved"
        snap = _snapshot(us, out)
        snap["generator"] = gen.get_state().clone()
        snaps.append(snap)
        del us, ts, ue, vae
    assert float(snaps[0]["loss"]) > 0 and "ip.ema" in snaps[0] and np.isfinite(float(snaps[0]["loss"]))
    for k in snaps[0]:
        assert _same(snaps[0][k], snaps[1][k]), f"{k}: the cached step differs from the pixel step"


# ================================================================================================ 5. micro-batches
def test_identical_micro_batches_equal_the_plain_step_bit_for_bit(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = _ip_case()
    runs = []
    for K in (1, 2):
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, ema=True)
        before = us.ip_adapter.store.master.clone()
        batch, rand = to_dev(case["batch"], dev), to_dev(case["rand"], dev)
        if K == 2:
            batch, rand = ({k: torch.cat([val, val]) for k, val in d.items()} for d in (batch, rand))
        out = tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=0.999, rand=rand,
                            micro_batches=K)
        torch.cuda.synchronize()
        assert (us.ip_adapter.store.gacc is not None) == (K == 2)
        assert not torch.equal(us.ip_adapter.store.master, before), "the adapter's store did not step"
        snap = _snapshot(us, out)
        snap["ip.grad"] = us.ip_adapter.store.grad_flat().clone()
        runs.append(snap)
        del us, ts, ue, vae
    for k in runs[0]:
        assert _same(runs[0][k], runs[1][k]), f"{k}: accumulated step differs"


# ================================================================================================ 6. captured against eager
def test_captured_step_matches_eager_and_refuses_a_batch_without_the_key(dev):
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = _ip_case()
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, ema=True)
        tc.ema_rate = 0.999
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph)
        base = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace = []
        for step in range(4):  # two eager warm-ups, the capture and its replay, one more replay: every step with another embedding
            batch = dict(base, pixel_values=(base["pixel_values"] + 0.05 * step).contiguous(),
                         image_embeds=(base["image_embeds"] * (1.0 + 0.1 * step)).contiguous())
            fn = table[tu.step_key(batch)]
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            trace.append(_snapshot(us, out))
            if use_graph and step >= 2:
                assert fn.graph is not None and fn.calls == 2
        assert us.step == 4
        if use_graph:
            before = us.ip_adapter.store.master.clone()
            with pytest.raises(ValueError, match="captured with image_embeds"):
                fn(us, ts, ue, te, {k: v for k, v in batch.items() if k != "image_embeds"}, gen, vae, sc)
            torch.cuda.synchronize()
            assert us.step == 4 and torch.equal(us.ip_adapter.store.master, before)
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 4
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager run at step {step}, {k}"


# ================================================================================================ 7. resume
def test_save_load_and_step_equals_two_steps(dev, tmp_path):
    from stable_diffusion_training_amd import training_utils as tu
    case = _ip_case()
    batch = to_dev(case["batch"], dev)

    def step(states, gen):
        us, ts, ue, te, vae, sc, _ = states
        return tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999, offset_noise_magnitude=0.1)

    tc, a = _build(case, dev, ema=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    step(a, gen)
    path = str(tmp_path / "state.safetensors")
    tu.save_training_state(path, a[0], a[1], gen)
    out2 = step(a, gen)
    tc, b = _build(case, dev, ema=True)
    gen_b = torch.Generator(device=dev)
    tu.load_training_state(path, b[0], b[1], gen_b)
    assert b[0].step == 1 and b[0].ip_adapter.store.count == 1
    out_b = step(b, gen_b)
    torch.cuda.synchronize()
    sa, sb = _snapshot(a[0], out2), _snapshot(b[0], out_b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k}: the resumed run differs from the uninterrupted one"
    assert torch.equal(gen.get_state(), gen_b.get_state())
    objs = {"unet": case["cfgs"]["unet"], "vae": case["cfgs"]["vae"], "text_encoder": case["cfgs"]["clip"]}
    for wrong in (a[2], a[0].ip_adapter, a[0].ip_adapter.store):
        with pytest.raises(ValueError, match="not a UNet"):
            tu.save_model(objs, None, wrong, a[1].params, a[4].params, str(tmp_path / "wrong"))
    assert not (tmp_path / "wrong").exists()
    from tests.helpers import build_hip_states
    _, plain = build_hip_states(make_case("tiny", B=2, image=64), dev)
    with pytest.raises(ValueError):
        tu.load_training_state(path, plain[0], plain[1], None)


# ================================================================================================ 8. the example loop
def test_example_loop_trains_an_ip_adapter_from_pixels_and_from_the_cache(tmp_path):
    import importlib.util
    import json
    import os
    from stable_diffusion_training_amd import checkpoint as ck
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(root, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    case = make_case("tiny", B=2, image=64)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": vae_w, "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}, "tokenizer": None}
    base = json.load(open(os.path.join(root, "tests", "golden", "model_properties_keys.json")))
    base.pop("_note")
    runs = []
    for name in ("pixels", "cached"):
        d = tmp_path / name
        d.mkdir()
        cfg = dict(base)
        cfg.update(model_path=str(d / "model@0"), batch_size=2, image_area_root=[64], minimum_axis_length=[64],
                   context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
                   ema_rate=0.99, repeat_batch=4, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
                   loss_logging_interval=1, loss_csv=str(d / "loss.csv"), test_save_path=str(d / "test_save"), batches_per_chunk=4, DEBUG=False,
                   ip_adapter=True, ip_adapter_embed_dim=E, ip_adapter_tokens=T, ip_adapter_drop_rate=0.25)
        if name == "cached":
            cfg["cache_latents"] = str(d / "latents")
        losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
        assert us.step == 4 and len(losses) == 4 and all(np.isfinite(losses)) and us.ip_adapter is not None and us.store.count == 0
        saved = ck.load_ip_adapter(str(d / "model-ip-adapter"))
        assert saved["config"]["image_embed_dim"] == E and saved["config"]["num_tokens"] == T
        live = us.ip_adapter.store.export("master")
        assert set(saved["params"]) == set(live) and all(torch.equal(saved["params"][p], live[p].cpu()) for p in live)
        ema = ck.load_ip_adapter(str(d / "model-ip-adapter-EMA"))
        assert set(ema["params"]) == set(saved["params"])
        with open(d / "model@1" / "unet" / ck.UNET_WEIGHTS, "rb") as f:
            flat = ck.flatten_tree(ck.flax_from_bytes(f.read()))
        assert all(np.array_equal(flat[p], case["weights"]["unet"][p].numpy()) for p in flat), "model@1/unet is not the frozen base"
        runs.append((losses, us.ip_adapter.store.master.clone()))
        del us, ts
    assert runs[0][0] == runs[1][0], "the losses of the cached loop differ from the pixel loop's"
    assert torch.equal(runs[0][1], runs[1][1])


# ================================================================================================ 9. generate
def test_generate_with_image_embeds_and_ip_scale(dev):
    """image_embeds move the image, ip_scale = 0 gives the plain pipeline's latents bit for bit, and the unconditional half of the
    doubled batch holds image_proj of zero embeddings."""
    from stable_diffusion_training_amd import nets, params
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = _ip_case()
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    ust = params.ParamStore(nets.unet_spec(case["cfgs"]["unet"]), device=dev, trainable=False)
    ust.load(case["weights"]["unet"])
    tst = params.ParamStore(nets.clip_text_spec(case["cfgs"]["clip"]), device=dev, trainable=False)
    tst.load(case["weights"]["clip"])
    args = (ust, tst, vae_w, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"])
    plain = StableDiffusionPipeline(*args, device=dev)
    pipe = StableDiffusionPipeline(*args, device=dev, ip_adapter=dict(config=case["ip_cfg"], params=case["ip_weights"]))
    ids = case["batch"]["input_ids"].to(dev)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    emb = case["batch"]["image_embeds"]
    kw = dict(num_inference_steps=2, height=64, width=64, latents=lat, return_latents=True)
    _, l_plain = plain.generate(ids, **kw)
    aux = {}
    img, l_ip = pipe.generate(ids, image_embeds=emb, aux=aux, **kw)
    _, l_zero = pipe.generate(ids, image_embeds=emb, ip_scale=0.0, **kw)
    _, l_half = pipe.generate(ids, image_embeds=emb.to(BF), ip_scale=0.5, **kw)
    assert tuple(img.shape) == (2, 64, 64, 3) and bool(torch.isfinite(img).all())
    assert torch.equal(l_zero, l_plain), "ip_scale = 0 must reproduce the plain pipeline"
    assert not torch.equal(l_ip, l_plain) and not torch.equal(l_half, l_ip) and not torch.equal(l_half, l_plain)
    tok = aux["ip_tokens"]
    assert tuple(tok.shape) == (4, T, case["cfgs"]["unet"]["cross_attention_dim"]) and tuple(aux["ip_scale"].shape) == (4,)
    want = nets.ip_adapter_tokens(pipe.ip_adapter.store, case["ip_cfg"], torch.zeros(2, E, device=dev))
    assert torch.equal(tok[:2], want), "the unconditional half must use zero image embeddings through image_proj"
    assert not torch.equal(tok[2:], want)
