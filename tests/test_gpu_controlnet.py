"""Training a ControlNet on the MI355X (tiny config, 64 x 64): controlnet_forward + unet_forward(control=) against the fp32 CPU
reference forward and backward, the zero-initialised ControlNet against the plain UNet, one step with taps, the cached step against
the pixel step, micro-batches, the captured step, resume, and the example loop."""
import numpy as np
import pytest
import torch

from tests import controlnet_reference as cr
from tests.helpers import make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")
TINY_CH = (16, 16, 32, 32)
NOISE_KW = dict(min_snr_gamma_magnitude=5.0, offset_noise_magnitude=0.1, perturbation_noise_magnitude=0.1)  # test_gpu_inpaint.py's


def _cn_case(B=2, image=64, sched="scaled_linear", zero=False, **unet_over):
    """make_case("tiny") plus a ControlNet: its config, its host weights (zero: controlnet_from_unet; else every leaf random, the zero
    convolutions at std 0.05) and a conditioning image in the batch."""
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=B, image=image, sched=sched)
    if unet_over:
        from oracle import nets as onets
        ucfg = dict(case["cfgs"]["unet"], **unet_over)
        case["cfgs"] = dict(case["cfgs"], unet=ucfg)
        case["weights"] = dict(case["weights"], unet=onets.init_params(onets.unet_param_shapes(ucfg), 1))
    ccfg = nets.controlnet_config(case["cfgs"]["unet"], TINY_CH)
    case["cn_cfg"] = ccfg
    uw = case["weights"]["unet"]
    case["cn_weights"] = nets.controlnet_from_unet(uw, ccfg, seed=6) if zero else cr.random_controlnet(uw, ccfg, seed=6)
    g = torch.Generator().manual_seed(21)
    case["batch"] = dict(case["batch"], conditioning_pixel_values=torch.rand(B, 3, image, image, generator=g))
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
    cn = dict(config=case["cn_cfg"], params=case["cn_weights"]) if params else dict(config=case["cn_cfg"])
    return tc, tu.on_device_model_training_state(tc, models, device=dev, controlnet=cn)


def _snapshot(us, out):
    st = us.controlnet.store
    snap = {f"controlnet.{b}": getattr(st, b).clone() for b in STATE if getattr(st, b) is not None}
    snap["loss"] = out[4]["loss"].clone()
    snap["controlnet.sqnorm"] = st.sqnorm.clone()
    return snap


def _cos(a, b):
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


def _pack_hint(cond, dev):
    from stable_diffusion_training_amd import _lib
    B, C, H, W = cond.shape
    src = cond.to(dev).contiguous()
    hint = torch.empty(B, H, W, 8, dtype=BF, device=dev)
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", src.data_ptr(), hint.data_ptr(), B, C, H, W, 8, torch.cuda.current_stream().cuda_stream)
    return hint


# ================================================================================================ 1. the two networks against the reference
@pytest.mark.parametrize("variant", ["tiny", "tiny_text_time"])
def test_controlnet_and_unet_forward_and_backward_against_the_reference(dev, variant):
    """Zero convolutions random at std 0.05: the residuals are distinct per skip and the mid residual is nonzero, so a swapped skip
    order or stale mid-block statistics miss the prediction gate.  Gates: tests/test_gpu_model.py's, as test_gpu_inpaint.py applies them."""
    from stable_diffusion_training_amd import nets, params
    tt = variant == "tiny_text_time"
    over = dict(addition_embed_type="text_time", addition_time_embed_dim=8, projection_class_embeddings_input_dim=64) if tt else {}
    case = _cn_case(**over)
    ucfg, ccfg, uw, cw = case["cfgs"]["unet"], case["cn_cfg"], case["weights"]["unet"], case["cn_weights"]
    g = torch.Generator().manual_seed(12)
    B, h, wd = 2, 8, 8
    x = torch.randn(B, 4, h, wd, generator=g)
    t = torch.tensor([17, 803])
    ctx = torch.randn(B, 77, ucfg["cross_attention_dim"], generator=g)
    cond = case["batch"]["conditioning_pixel_values"]
    r = torch.randn(B, 4, h, wd, generator=g)
    added = dict(text_embeds=torch.randn(B, 16, generator=g), time_ids=torch.tensor([[64, 64, 0, 0, 64, 64]] * B, dtype=torch.int32)) if tt else None
    # the reference sees what the device sees: bf16 values of the inputs
    q = lambda v: v.to(BF).float()
    radded = None if added is None else dict(text_embeds=q(added["text_embeds"]), time_ids=added["time_ids"])
    wl = {k: v.clone().requires_grad_(not tt) for k, v in cw.items()}
    rdown, rmid = cr.controlnet_forward(wl, ccfg, q(x), t, q(ctx), q(cond), radded)
    ref = cr.unet_forward(uw, ucfg, q(x), t, q(ctx), radded, down=rdown, mid=rmid)
    plain = cr.unet_forward(uw, ucfg, q(x), t, q(ctx), radded)
    assert rel_l2(ref.detach(), plain) > 0.05, "the residuals do not move the reference prediction: the test would not see them"
    for i in range(len(rdown)):
        for j in range(i):
            if rdown[i].shape == rdown[j].shape:
                assert rel_l2(rdown[i].detach(), rdown[j].detach()) > 0.5, (i, j)

    ust = params.ParamStore(nets.unet_spec(ucfg), device=dev, trainable=False)
    ust.load(uw)
    cst = params.ParamStore(nets.controlnet_spec(ccfg), device=dev, quantise=False)
    cst.load(cw)
    cst.prepare()
    cst.zero_grad()
    xin = torch.zeros(B, h, wd, 8, dtype=BF, device=dev)
    xin[..., :4] = x.permute(0, 2, 3, 1).to(dev)
    tdev, cdev = t.to(dev).to(torch.int32), ctx.to(dev).to(BF)
    dadded = None if added is None else to_dev(added, dev)
    down, mid = nets.controlnet_forward(cst, ccfg, xin, tdev, cdev, _pack_hint(cond, dev), dadded)
    assert len(down) == len(rdown) == 4
    for i, (a, b) in enumerate(zip(down, rdown)):
        assert tuple(a.shape) == tuple(b.shape) and rel_l2(a.detach(), b.detach()) < 2e-2, f"down residual {i}: {rel_l2(a.detach(), b.detach())}"
    assert rel_l2(mid.detach(), rmid.detach()) < 2e-2 and float(mid.detach().abs().max()) > 0
    pred = nets.unet_forward(ust, ucfg, xin, tdev, cdev, dadded, control=(down, mid))
    assert rel_l2(pred[..., :4].permute(0, 3, 1, 2).detach(), ref.detach()) < 2e-2
    if tt:
        return
    assert not xin.requires_grad and xin.grad is None
    gref = dict(zip(wl, torch.autograd.grad((ref * r).sum(), list(wl.values()), allow_unused=True)))
    dpred = torch.zeros_like(pred)
    dpred[..., :4] = r.permute(0, 2, 3, 1).to(dev)
    pred.backward(dpred)
    got = cst.export("grad")
    flat = lambda keys, src: torch.cat([src[k].flatten().float().cpu() for k in keys])
    kernels = [k for k in gref if k.endswith("/kernel") and gref[k] is not None]
    assert len(kernels) == len([k for k in wl if k.endswith("/kernel")]), "a ControlNet kernel leaf without a reference gradient"
    assert _cos(flat(kernels, got), flat(kernels, gref)) > 0.995
    embedder = [k for k in kernels if k.startswith("controlnet_cond_embedding/")]
    zero_convs = [k for k in kernels if k.startswith(("controlnet_down_blocks_", "controlnet_mid_block"))]
    assert len(embedder) == 8 and len(zero_convs) == 5
    for name, keys in (("embedder", embedder), ("zero convolutions", zero_convs)):
        a, b = flat(keys, got), flat(keys, gref)
        assert float(a.abs().max()) > 0 and _cos(a, b) > 0.99, (name, _cos(a, b))
    for k in embedder + zero_convs:
        assert float(got[k].abs().max()) > 0, f"{k}: zero gradient"


# ================================================================================================ 2. the zero-initialised ControlNet
def test_zero_initialised_controlnet_leaves_the_prediction_alone_and_trains_only_its_zero_convolutions(dev):
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    case = _cn_case(zero=True)
    tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, params=False)  # (initialised by controlnet_from_unet inside)
    assert us.controlnet is not None and us.opt_store is us.controlnet.store and not us.store.trainable and not ts.store.trainable
    assert ts.opt_store is None and ue is None and te is None
    base_u, base_t = us.store.master.clone(), ts.store.master.clone()
    w_u, w_t = us.store.w.clone(), ts.store.w.clone()
    aux = {}
    out = tu.train_step(us, ts, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev), aux=aux)
    torch.cuda.synchronize()
    assert all(float(d.abs().max()) == 0 for d in aux["control_down"]) and float(aux["control_mid"].abs().max()) == 0
    # the same UNet input without the ControlNet
    xin = torch.zeros(2, 8, 8, 8, dtype=BF, device=dev)
    xin[..., :4] = aux["noisy"].permute(0, 2, 3, 1)
    plain = nets.unet_forward(us.store, us.config, xin, to_dev(case["rand"], dev)["timesteps"].to(torch.int32), aux["ctx"])
    assert torch.equal(aux["pred"], plain.detach()), "a zero ControlNet changed the prediction"
    grads = us.controlnet.store.export("grad")
    zero_convs = [p for p in grads if p.startswith(("controlnet_down_blocks_", "controlnet_mid_block"))]
    assert len(zero_convs) == 10
    for p, gval in grads.items():
        if p in zero_convs:
            assert float(gval.abs().max()) > 0 and bool(torch.isfinite(gval).all()), f"{p}: no gradient"
        else:
            assert float(gval.abs().max()) == 0, f"{p}: a gradient behind zero convolutions"
    assert us.step == 1 and us.store.count == 0 and np.isfinite(out[4]["loss"].item())
    assert torch.equal(us.store.master, base_u) and torch.equal(ts.store.master, base_t), "a frozen master moved"
    assert torch.equal(us.store.w.view(torch.int16), w_u.view(torch.int16)) and torch.equal(ts.store.w.view(torch.int16), w_t.view(torch.int16))


# ================================================================================================ 3. one step with taps
def test_one_step_with_taps_matches_the_reference_loss(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = _cn_case()
    tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev)
    base_u, base_t, before = us.store.master.clone(), ts.store.master.clone(), us.controlnet.store.master.clone()
    batch = to_dev(case["batch"], dev)
    aux = {}
    out = tu.train_step(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev), aux=aux)
    torch.cuda.synchronize()
    loss = out[4]["loss"].item()
    hint = aux["control_hint"]
    assert hint.dtype == BF and tuple(hint.shape) == (2, 64, 64, 8) and float(hint[..., 3:].abs().max()) == 0
    assert torch.equal(hint[..., :3].float().cpu(), case["batch"]["conditioning_pixel_values"].permute(0, 2, 3, 1).to(BF).float())
    assert len(aux["control_down"]) == 4 and tuple(aux["control_mid"].shape) == (2, 4, 4, 64)
    # the reference networks fed the step's own taps
    noisy, ctx, t = aux["noisy"].cpu().to(BF).float(), aux["ctx"].float().cpu(), case["rand"]["timesteps"]
    rdown, rmid = cr.controlnet_forward(case["cn_weights"], case["cn_cfg"], noisy, t, ctx, hint[..., :3].float().cpu().permute(0, 3, 1, 2))
    for a, b in zip(aux["control_down"] + [aux["control_mid"]], rdown + [rmid]):
        assert rel_l2(a, b) < 2e-2
    ref = cr.unet_forward(case["weights"]["unet"], case["cfgs"]["unet"], noisy, t, ctx, down=rdown, mid=rmid)
    assert rel_l2(aux["pred"][..., :4].permute(0, 3, 1, 2), ref) < 2e-2
    ref_loss = float(((ref.double() - aux["target"].cpu().double()) ** 2).mean())
    assert abs(loss - ref_loss) / ref_loss < 1e-2, (loss, ref_loss)
    assert us.step == 1 and us.controlnet.store.count == 1 and us.store.count == 0 and ts.store.count == 0
    assert torch.equal(us.store.master, base_u) and torch.equal(ts.store.master, base_t)
    assert not torch.equal(us.controlnet.store.master, before) and bool(torch.isfinite(us.controlnet.store.master).all())
    assert all(v.grad is None for v in batch.values() if torch.is_tensor(v)) and aux["noisy"].grad is None
    gn = us.controlnet.store.grad_norm()
    assert np.isfinite(gn) and gn > 0


# ================================================================================================ 4. cached against pixel step
VARIANTS = {
    "a_epsilon_rand": dict(pred="epsilon", sched="scaled_linear", kw={}, rand=True),
    "b_vpred_noise_options_rand": dict(pred="v_prediction", sched="zero_snr_scaled_linear", kw=NOISE_KW, rand=True),
    "c_vpred_noise_options_generator": dict(pred="v_prediction", sched="zero_snr_scaled_linear", kw=NOISE_KW, rand=False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cached_step_equals_the_pixel_step_bit_for_bit(dev, variant):
    from stable_diffusion_training_amd import training_utils as tu
    v = VARIANTS[variant]
    case = _cn_case(sched=v["sched"])
    if v["kw"]:
        g = torch.Generator().manual_seed(7)
        case["rand"]["offset_noise"] = torch.randn(2, 4, 1, 1, generator=g)
        case["rand"]["perturb_noise"] = torch.randn(2, 4, 8, 8, generator=g)
    snaps = []
    for cached in (False, True):
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, prediction_type=v["pred"], ema=True)
        assert ue is not None and ue.store is us.controlnet.store and te is None
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
        snap = _snapshot(us, out)
        snap["generator"] = gen.get_state().clone()
        snaps.append(snap)
        del us, ts, ue, vae
    assert float(snaps[0]["loss"]) > 0 and "controlnet.ema" in snaps[0]
    for k in snaps[0]:
        a, b = snaps[0][k], snaps[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b), \
            f"{k}: the cached step differs from the pixel step"


# ================================================================================================ 5. micro-batches
def test_identical_micro_batches_equal_the_plain_step_bit_for_bit(dev):
    """tests/test_gpu_grad_accum.py's rule: the batch b ++ b with micro_batches=2 accumulates g + g and scales by 1/2, exact in fp32, so
    everything the step writes equals the plain step on b (the ControlNet step always takes the ordinary norm pass)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = _cn_case()
    runs = []
    for K in (1, 2):
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, ema=True)
        batch, rand = to_dev(case["batch"], dev), to_dev(case["rand"], dev)
        if K == 2:
            batch, rand = ({k: torch.cat([val, val]) for k, val in d.items()} for d in (batch, rand))
        out = tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=0.999, rand=rand,
                            micro_batches=K)
        torch.cuda.synchronize()
        assert (us.controlnet.store.gacc is not None) == (K == 2)
        snap = _snapshot(us, out)
        snap["controlnet.grad"] = us.controlnet.store.grad_flat().clone()
        runs.append(snap)
        del us, ts, ue, vae
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b), f"{k}: accumulated step differs"


# ================================================================================================ 6. captured against eager
def test_captured_step_matches_eager_and_refuses_a_batch_without_the_key(dev):
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = _cn_case()
        tc, (us, ts, ue, te, vae, sc, _) = _build(case, dev, ema=True)
        tc.ema_rate = 0.999
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph)
        assert list(table) == [(2, 3, 64, 64)]
        base = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace = []
        for step in range(5):  # two eager warm-ups, the capture and its replay, two more replays: every step with another hint
            batch = dict(base, pixel_values=(base["pixel_values"] + 0.05 * step).contiguous(),
                         conditioning_pixel_values=((base["conditioning_pixel_values"] + 0.1 * step) % 1.0).contiguous())
            fn = table[tu.step_key(batch)]
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            trace.append(_snapshot(us, out))
            if use_graph and step >= 2:
                assert fn.graph is not None and fn.calls == 2
        assert us.step == 5
        if use_graph:
            before = us.controlnet.store.master.clone()
            with pytest.raises(ValueError, match="captured with conditioning_pixel_values"):
                fn(us, ts, ue, te, {k: v for k, v in batch.items() if k != "conditioning_pixel_values"}, gen, vae, sc)
            torch.cuda.synchronize()
            assert us.step == 5 and torch.equal(us.controlnet.store.master, before)
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 5
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager run at step {step}, {k}"


# ================================================================================================ 7. resume
def test_save_load_and_step_equals_two_steps(dev, tmp_path):
    from stable_diffusion_training_amd import training_utils as tu
    case = _cn_case()
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
    assert b[0].step == 1 and b[0].controlnet.store.count == 1
    out_b = step(b, gen_b)
    torch.cuda.synchronize()
    sa, sb = _snapshot(a[0], out2), _snapshot(b[0], out_b)
    assert a[0].step == 2 and b[0].step == 2
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k}: the resumed run differs from the uninterrupted one"
    assert torch.equal(gen.get_state(), gen_b.get_state())
    # save_model takes the frozen UNet, never the ControlNet's store or the EMA view over it
    objs = {"unet": case["cfgs"]["unet"], "vae": case["cfgs"]["vae"], "text_encoder": case["cfgs"]["clip"]}
    for wrong in (a[2], a[0].controlnet, a[0].controlnet.store):
        with pytest.raises(ValueError, match="not a UNet"):
            tu.save_model(objs, None, wrong, a[1].params, a[4].params, str(tmp_path / "wrong"))
    assert not (tmp_path / "wrong").exists()
    # a state without a ControlNet does not take the file
    from tests.helpers import build_hip_states
    _, plain = build_hip_states(make_case("tiny", B=2, image=64), dev)
    with pytest.raises(ValueError):
        tu.load_training_state(path, plain[0], plain[1], None)


# ================================================================================================ 8. the example loop
def test_example_loop_trains_a_controlnet_from_pixels_and_from_the_cache(tmp_path):
    import importlib.util
    import json
    import os
    from oracle import nets as onets
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
                   ema_rate=0.99, repeat_batch=5, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
                   loss_logging_interval=1, loss_csv=str(d / "loss.csv"), test_save_path=str(d / "test_save"), batches_per_chunk=5, DEBUG=False,
                   controlnet=True, controlnet_channels=list(TINY_CH))
        if name == "cached":
            cfg["cache_latents"] = str(d / "latents")
        losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
        assert us.step == 5 and len(losses) == 5 and all(np.isfinite(losses)) and us.controlnet is not None and us.store.count == 0
        saved = ck.load_controlnet(str(d / "model-controlnet"))
        assert saved["config"]["conditioning_embedding_out_channels"] == TINY_CH
        live = us.controlnet.store.export("master")
        assert all(torch.equal(saved["params"][p], live[p].cpu()) for p in live)
        assert float(saved["params"]["controlnet_mid_block/kernel"].abs().max()) > 0, "the zero convolutions did not train"
        # the pipeline directories, the -EMA one too, hold the frozen UNet: exactly unet_spec's leaves, the weights the run began with;
        # the ControlNet's EMA goes to a submodel directory of its own
        from stable_diffusion_training_amd import nets
        want_leaves = {p: tuple(s) for p, s in nets.unet_spec(case["cfgs"]["unet"])}
        for pipe_dir in ("model@1", "model-EMA@1"):
            with open(d / pipe_dir / "unet" / ck.UNET_WEIGHTS, "rb") as f:
                flat = ck.flatten_tree(ck.flax_from_bytes(f.read()))
            assert {p: tuple(v.shape) for p, v in flat.items()} == want_leaves, f"{pipe_dir}/unet does not hold a UNet"
            assert all(np.array_equal(flat[p], case["weights"]["unet"][p].numpy()) for p in flat), f"{pipe_dir}/unet is not the frozen base"
        ema = ck.load_controlnet(str(d / "model-controlnet-EMA"))
        assert set(ema["params"]) == set(saved["params"]) and not torch.equal(ema["params"]["controlnet_mid_block/kernel"],
                                                                              saved["params"]["controlnet_mid_block/kernel"])
        runs.append((losses, us.controlnet.store.master.clone()))
        del us, ts
    assert runs[0][0] == runs[1][0], "the losses of the cached loop differ from the pixel loop's"
    assert torch.equal(runs[0][1], runs[1][1])
