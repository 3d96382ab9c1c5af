"""Training an inpainting UNet on the MI355X (tiny config, 64 x 64, 9 input channels): the UNet at 9 channels against the fp32
oracle, the step's input layout and prediction, the zero-widened UNet against the 4-channel one, the cached step against the pixel
step and the captured step against the eager one bit for bit, and the step beside LoRA and the masked Huber loss."""
import math

import numpy as np
import pytest
import torch

from tests import inpaint_reference as ir
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")


def _rect_masks(B, H, W, seed):
    """One rectangle of ones per image, a different one for every (seed, image)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, H, W)
    for i in range(B):
        hh, ww = (int(torch.randint(n // 4, 3 * n // 4 + 1, (1,), generator=g)) for n in (H, W))
        y0, x0 = int(torch.randint(0, H - hh + 1, (1,), generator=g)), int(torch.randint(0, W - ww + 1, (1,), generator=g))
        m[i, y0: y0 + hh, x0: x0 + ww] = 1.0
    return m


def _inpaint_case(B=2, image=64, sched="scaled_linear", zero_rows=False):
    """make_case("tiny") with the UNet widened to 9 input channels (new conv_in rows random unless zero_rows), an inpaint_mask in the
    batch and the masked image's posterior draw in rand."""
    from stable_diffusion_training_amd import nets
    case = make_case("tiny", B=B, image=image, sched=sched)
    case["plain"] = dict(cfgs=case["cfgs"], weights=case["weights"])
    wide, cfg9 = nets.widen_conv_in(case["weights"]["unet"], case["cfgs"]["unet"], 9)
    if not zero_rows:
        g = torch.Generator().manual_seed(77)
        k = wide["conv_in/kernel"]
        k[:, :, 4:] = torch.randn(3, 3, 5, k.shape[3], generator=g) / math.sqrt(9 * 9)
    case["cfgs"] = dict(case["cfgs"], unet=cfg9)
    case["weights"] = dict(case["weights"], unet=wide)
    case["batch"] = dict(case["batch"], inpaint_mask=_rect_masks(B, image, image, 5))
    g = torch.Generator().manual_seed(78)
    case["rand"] = dict(case["rand"], masked_posterior_eps=torch.randn(B, image // 8, image // 8, 4, generator=g))
    return case


def _snapshot(us, ts, out):
    snap = {f"{name}.{b}": getattr(st, b).clone() for name, st in (("unet", us.store), ("text", ts.store)) for b in STATE}
    snap["loss"] = out[4]["loss"].clone()
    snap["unet.sqnorm"], snap["text.sqnorm"] = us.store.sqnorm.clone(), ts.store.sqnorm.clone()
    return snap


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF else torch.equal(a, b)


def _u16(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


# ================================================================================================ 1. the UNet at 9 channels
def test_unet_forward_and_backward_at_nine_input_channels(dev):
    """Forward and the gradient of <pred, r> for every kernel leaf against oracle.nets.unet_forward under autograd, with
    tests/test_gpu_model.py's gates; conv_in's weight gradient has all 9 input rows."""
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets, params
    case = _inpaint_case()
    cfg, w = case["cfgs"]["unet"], case["weights"]["unet"]
    C0 = cfg["block_out_channels"][0]
    g = torch.Generator().manual_seed(12)
    B, h, wd = 2, 8, 8
    x = torch.randn(B, 9, h, wd, generator=g)
    t = torch.tensor([17, 803])
    ctx = torch.randn(B, 77, cfg["cross_attention_dim"], generator=g)
    r = torch.randn(B, 4, h, wd, generator=g)
    wl = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    ref = onets.unet_forward(wl, cfg, x, t, ctx)
    gref = dict(zip(wl, torch.autograd.grad((ref * r).sum(), list(wl.values()), allow_unused=True)))

    st = params.ParamStore(nets.unet_spec(cfg), device=dev, quantise=False)
    st.load(w)
    st.prepare()
    st.zero_grad()
    xin = torch.zeros(B, h, wd, 16, dtype=BF, device=dev)
    xin[..., :9] = x.permute(0, 2, 3, 1).to(dev)
    pred = nets.unet_forward(st, cfg, xin, t.to(dev).to(torch.int32), ctx.to(dev).to(BF).requires_grad_(True))
    assert rel_l2(pred[..., :4].permute(0, 3, 1, 2), ref.detach()) < 2e-2
    dpred = torch.zeros_like(pred)
    dpred[..., :4] = r.permute(0, 2, 3, 1).to(dev)
    pred.backward(dpred)
    got = st.export("grad")
    assert tuple(got["conv_in/kernel"].shape) == (3, 3, 9, C0) == tuple(gref["conv_in/kernel"].shape)
    keys = [k for k in gref if k.endswith("/kernel") and gref[k] is not None]
    a = torch.cat([got[k].flatten().cpu() for k in keys])
    b = torch.cat([gref[k].flatten() for k in keys])
    assert float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.995
    ca, cb = got["conv_in/kernel"].cpu(), gref["conv_in/kernel"]
    for rows in (slice(0, 4), slice(4, 9)):
        fa, fb = ca[:, :, rows].flatten(), cb[:, :, rows].flatten()
        assert float(fa.abs().max()) > 0 and float(torch.dot(fa, fb) / (fa.norm() * fb.norm())) > 0.99, rows


# ================================================================================================ 2. a step with taps
@pytest.mark.parametrize("pred_type,sched", [("epsilon", "scaled_linear"), ("v_prediction", "zero_snr_scaled_linear")])
def test_step_builds_the_reference_input_and_matches_the_oracle_unet(dev, pred_type, sched):
    from oracle import nets as onets
    from stable_diffusion_training_amd import training_utils as tu
    case = _inpaint_case(sched=sched)
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, prediction_type=pred_type)
    aux = {}
    out = tu.train_step(us, ts, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev), aux=aux)
    torch.cuda.synchronize()
    loss = out[4]["loss"].item()
    mask = case["batch"]["inpaint_mask"].numpy()
    assert np.array_equal(aux["inpaint_mask"].cpu().numpy(), ir.latent_mask(mask, 8)) and 0 < aux["inpaint_mask"].mean() < 1
    x = aux["unet_input"]
    assert x.dtype == BF and tuple(x.shape) == (2, 8, 8, 16)
    nhwc = lambda t: _u16(t.to(BF).permute(0, 2, 3, 1))  # f32 NCHW tap -> the bf16 (RNE) NHWC bit patterns
    want = ir.unet_input_bits(nhwc(aux["noisy"]), aux["inpaint_mask"].cpu().numpy(), nhwc(aux["masked_latents"]), 4, 16)
    assert np.array_equal(_u16(x), want), "unet_input differs from the reference layout built from the taps"
    # the masked-image latents are those of the masked image: the oracle VAE on repaint ? 0 : x
    mref = onets.vae_encode_moments(case["weights"]["vae"], case["cfgs"]["vae"],
                                    torch.from_numpy(ir.masked_image(case["batch"]["pixel_values"].numpy(), mask)))
    assert rel_l2(aux["masked_moments"], mref) < 2e-2
    # the oracle UNet fed that input
    ref = onets.unet_forward(case["weights"]["unet"], case["cfgs"]["unet"], x[..., :9].float().cpu().permute(0, 3, 1, 2), case["rand"]["timesteps"],
                             aux["ctx"].float().cpu())
    pred = aux["pred"][..., :4].permute(0, 3, 1, 2)
    assert rel_l2(pred, ref) < 2e-2
    ref_loss = float(((ref.double() - aux["target"].cpu().double()) ** 2).mean())
    assert abs(loss - ref_loss) / ref_loss < 1e-2, (loss, ref_loss)
    gk = us.store.export("grad")["conv_in/kernel"]
    assert tuple(gk.shape)[:3] == (3, 3, 9) and float(gk[:, :, 4:].abs().max()) > 0 and bool(torch.isfinite(gk).all())
    assert all(float(gk[:, :, c].abs().max()) > 0 for c in range(9)), "an input channel without a gradient"
    assert us.step == 1


# ================================================================================================ 3. zero-widened against 4 channels
def test_zero_widened_unet_agrees_with_the_four_channel_step(dev, capsys):
    """Zero new rows: the widened UNet computes what the 4-channel one does.  The 4-channel step runs from the widened step's own
    image moments (a cached batch), so both UNets see bit-equal noisy latents and targets and only conv_in's K extent (4 -> 9 rows,
    padded 8 -> 16) separates them: within the gates, not asserted bit for bit; whether it happens to be bit-equal is printed, and
    recorded in DESIGN.md."""
    from stable_diffusion_training_amd import training_utils as tu
    case = _inpaint_case(zero_rows=True)
    runs, moments = [], None
    for wide in (True, False):
        c = case if wide else dict(case, **case["plain"])
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(c, dev)
        batch = to_dev(case["batch"], dev)
        rand = to_dev(case["rand"], dev)
        if not wide:
            batch = {"input_ids": batch["input_ids"], "latent_moments": moments}
            rand.pop("masked_posterior_eps")
            vae = None
        aux = {}
        out = tu.train_step(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, rand=rand, aux=aux)
        torch.cuda.synchronize()
        moments = aux["moments"].clone().contiguous()
        runs.append((out[4]["loss"].item(), aux["pred"].clone(), aux["noisy"].clone(), aux["target"].clone()))
        del us, ts, vae
    (l9, p9, n9, t9), (l4, p4, n4, t4) = runs
    assert torch.equal(t4, t9) and torch.equal(n4, n9), "noisy latents or target changed with the inpainting front"
    e = rel_l2(p9[..., :4], p4[..., :4])
    with capsys.disabled():
        print(f"\n[inpaint] zero-widened vs 4-channel step: pred bit-equal {torch.equal(p4.view(torch.int16), p9.view(torch.int16))}, "
              f"loss {l4!r} vs {l9!r}, pred rel-L2 {e:.3e}")
    assert e < 2e-2 and abs(l9 - l4) / l4 < 1e-2, (l4, l9, e)


# ================================================================================================ 4. cached against pixel step
def _cached_batch(tu, vae, batch, K):
    n = batch["pixel_values"].shape[0] // K
    parts = [tu.encode_inpaint_moments(vae, batch["pixel_values"][k * n: (k + 1) * n].contiguous(),
                                       batch["inpaint_mask"][k * n: (k + 1) * n].contiguous()) for k in range(K)]
    out = {k: v for k, v in batch.items() if k not in ("pixel_values", "inpaint_mask")}
    out["latent_moments"], out["masked_latent_moments"], out["inpaint_mask"] = (torch.cat([p[i] for p in parts]).contiguous() for i in range(3))
    return out


NOISE_KW = dict(min_snr_gamma_magnitude=5.0, offset_noise_magnitude=0.1, perturbation_noise_magnitude=0.1)
VARIANTS = {
    "a_epsilon_rand": dict(B=2, pred="epsilon", sched="scaled_linear", kw={}, rand=True, K=1),
    "b_micro_batches": dict(B=4, pred="epsilon", sched="scaled_linear", kw={}, rand=True, K=2),
    "c_vpred_offset_perturb_rand": dict(B=2, pred="v_prediction", sched="zero_snr_scaled_linear", kw=NOISE_KW, rand=True, K=1),
    "d_vpred_offset_perturb_generator": dict(B=2, pred="v_prediction", sched="zero_snr_scaled_linear", kw=NOISE_KW, rand=False, K=1),
    "e_micro_batches_generator": dict(B=4, pred="epsilon", sched="scaled_linear", kw={}, rand=False, K=2),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cached_step_equals_the_pixel_step_bit_for_bit(dev, variant):
    """Identically built states, one stepped from pixels + mask, one from the moments of the same stacked encode with no VAE: every
    state buffer, the loss, the squared gradient norms and (without rand=) the generator's final state are equal."""
    from stable_diffusion_training_amd import training_utils as tu
    v = VARIANTS[variant]
    B, K = v["B"], v["K"]
    case = _inpaint_case(B=B, sched=v["sched"])
    if v["kw"]:
        g = torch.Generator().manual_seed(7)
        case["rand"]["offset_noise"] = torch.randn(B, 4, 1, 1, generator=g)
        case["rand"]["perturb_noise"] = torch.randn(B, 4, 8, 8, generator=g)
    snaps = []
    for cached in (False, True):
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, prediction_type=v["pred"], ema=True)
        batch = to_dev(case["batch"], dev)
        if cached:
            batch, vae = _cached_batch(tu, vae, batch, K), None
            assert batch["masked_latent_moments"].dtype == BF and tuple(batch["inpaint_mask"].shape) == (B, 8, 8)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        aux = {} if K == 1 else None
        out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999,
                            rand=to_dev(case["rand"], dev) if v["rand"] else None, micro_batches=K, aux=aux, **v["kw"])
        torch.cuda.synchronize()
        snap = _snapshot(us, ts, out)
        snap["generator"] = gen.get_state().clone()
        if aux is not None:
            for k in ("latents", "noisy", "target", "moments", "masked_moments", "masked_latents", "unet_input", "inpaint_mask"):
                snap[f"aux.{k}"] = aux[k].clone()
        snaps.append(snap)
        del us, ts, ue, te, vae
    assert float(snaps[0]["loss"]) > 0
    for k in snaps[0]:
        a, b = snaps[0][k], snaps[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert _same(a, b), f"{k}: the cached step differs from the pixel step ({(a.double() - b.double()).abs().max().item():.3e} max abs)"


# ================================================================================================ 5. captured against eager
def test_captured_step_matches_eager_and_refuses_a_batch_without_the_mask(dev):
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = _inpaint_case()
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        tc.ema_rate = 0.999
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph)
        assert list(table) == [(2, 3, 64, 64)]
        base = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace = []
        for step in range(5):  # two eager warm-ups, the capture and its replay, two more replays: every step with another mask
            batch = dict(base, pixel_values=(base["pixel_values"] + 0.05 * step).contiguous(), inpaint_mask=_rect_masks(2, 64, 64, 100 + step).to(dev))
            fn = table[tu.step_key(batch)]
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            trace.append(_snapshot(us, ts, out))
            if use_graph and step >= 2:
                assert fn.graph is not None and fn.calls == 2
        assert us.step == 5
        if use_graph:
            before = us.store.master.clone()
            with pytest.raises(ValueError, match="captured with inpaint_mask"):
                fn(us, ts, ue, te, {k: v for k, v in batch.items() if k != "inpaint_mask"}, gen, vae, sc)
            torch.cuda.synchronize()
            assert us.step == 5 and torch.equal(us.store.master, before)
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 5
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager run at step {step}, {k}"


# ================================================================================================ 6. beside LoRA and the robust masked loss
def test_one_lora_step_on_the_inpainting_unet(dev):
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
    case = _inpaint_case()
    tc, _ = build_hip_states(make_case("tiny", B=2, image=64), dev)  # (the config object only)
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    us, ts, ue, te, vae, sc, _ = tu.on_device_model_training_state(tc, models, device=dev,
                                                                   lora=dict(unet=lora.LoraConfig(4, 4.0, seed=1), text_encoder="frozen"))
    base, ad = us.store.master.clone(), us.adapter.store.master.clone()
    out = tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev))
    torch.cuda.synchronize()
    assert np.isfinite(out[4]["loss"].item()) and out[4]["loss"].item() > 0
    assert torch.equal(us.store.master, base), "the frozen master moved"
    assert not torch.equal(us.adapter.store.master, ad) and bool(torch.isfinite(us.adapter.store.master).all())
    assert us.step == 1 and us.store.count == 0 and np.isfinite(us.adapter.store.grad_norm()) and us.adapter.store.grad_norm() > 0


def test_one_masked_huber_step_on_the_inpainting_unet(dev):
    """loss_mask stays independent of inpaint_mask: both in one batch, with the Huber loss."""
    from stable_diffusion_training_amd import training_utils as tu
    case = _inpaint_case()
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev)
    batch = to_dev(dict(case["batch"], loss_mask=_rect_masks(2, 64, 64, 9)), dev)
    before = us.store.master.clone()
    aux = {}
    out = tu.train_step(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev), loss_type="huber", huber_c=0.1, huber_schedule="snr", aux=aux)
    torch.cuda.synchronize()
    lps = out[4]["loss_per_sample"]
    assert np.isfinite(out[4]["loss"].item()) and out[4]["loss"].item() > 0 and tuple(lps.shape) == (2,) and bool(torch.isfinite(lps).all())
    assert not torch.equal(aux["loss_mask"], aux["inpaint_mask"]) and tuple(aux["loss_mask"].shape) == tuple(aux["inpaint_mask"].shape)
    assert us.step == 1 and not torch.equal(us.store.master, before) and np.isfinite(us.store.grad_norm()) and us.store.grad_norm() > 0


# ================================================================================================ 7. loader, cache and the example loop
def test_cache_built_from_a_loader_with_inpaint_masks_trains_like_the_pixels(dev, tmp_path):
    """streamer.DataLoader(inpaint_masks=True) -> latent_cache.build (the stacked 2B encode, masked moments and the latent mask in the
    records) -> three steps from the Reader without a VAE against three steps from the loader's pixels: bit-identical stores."""
    from stable_diffusion_training_amd import latent_cache as lc
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.streamer import DataLoader
    case = _inpaint_case()
    loader = DataLoader(training_batch_size=2, repeat_batch=1, maximum_resolution_areas=[64 ** 2], bucket_lower_bound_resolutions=[64],
                        batches_per_chunk=3, vocab_size=1000, seed=3, device=dev, inpaint_masks=True)
    loader._print_debug = False
    loader.create_training_dataframe()
    snaps = []
    for cached in (False, True):
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        loader.dispatch_worker()
        batches = loader
        if cached:
            assert lc.build(loader, vae, str(tmp_path / "cache")) == 3
            batches = lc.Reader(str(tmp_path / "cache"), device=dev, vae=vae)
            vae = None
        gen = torch.Generator(device=dev)
        gen.manual_seed(11)
        losses = []
        while True:
            batch = batches.grab_next_batch()
            if isinstance(batch, str):
                break
            assert ("masked_latent_moments" in batch) == cached and tu.step_key(batch) == (2, 3, 64, 64)
            assert tuple(batch["inpaint_mask"].shape) == ((2, 8, 8) if cached else (2, 64, 64))
            out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999, offset_noise_magnitude=0.1)
            losses.append(out[4]["loss"].clone())
        torch.cuda.synchronize()
        assert us.step == 3 and len(losses) == 3
        snap = _snapshot(us, ts, out)
        snap["losses"] = torch.stack(losses)
        snaps.append(snap)
        del us, ts, ue, te, vae
    for k in snaps[0]:
        assert torch.equal(snaps[0][k], snaps[1][k]), f"{k}: training from the cache differs from training from the pixels"


def test_example_loop_with_inpaint_widens_the_unet_and_trains_from_pixels_and_cache(tmp_path):
    """examples/train_synthetic.py with "inpaint": the 4-channel synthetic UNet is widened to 9 channels and trained from batches with an
    inpaint mask (captured steps); with cache_latents as well the losses and final weights are the pixel run's."""
    import importlib.util
    import json
    import os
    from stable_diffusion_training_amd import nets
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(root, "examples", "train_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from oracle import nets as onets
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
                   inpaint=True)
        if name == "cached":
            cfg["cache_latents"] = str(d / "latents")
        losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
        assert us.step == 5 and len(losses) == 5 and all(np.isfinite(losses))
        assert us.config["in_channels"] == 9 and nets.inpaint_latent_channels(us.config) == 4 and models["unet"]["config"]["in_channels"] == 4
        runs.append((losses, us.store.master.clone(), ts.store.master.clone()))
        del us, ts
    assert runs[0][0] == runs[1][0], "the losses of the cached loop differ from the pixel loop's"
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
