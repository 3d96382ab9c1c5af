"""train_step with loss_type "huber" / "smooth_l1" on the MI355X (tiny model, the configs and gates of tests/test_gpu_masked_loss.py):
an explicit "l2" against the plain step, the loss launch against the reference evaluated on the step's own aux taps and the schedule
table at the drawn timesteps, captured against eager steps, micro-batches, a LoRA state and a latent cache.  Kernel-level checks:
tests/test_gpu_robust_loss_kernels.py."""
import numpy as np
import pytest
import torch

from tests import masked_loss_reference as mr
from tests import robust_loss_reference as rr
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev
from tests.test_gpu_masked_loss import _assert_same, _pixel_mask, _snapshot, _step

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _check_loss_launch_against_taps(tu, sched_state, out, aux, timesteps, loss_type, huber_c, schedule, *, C, lw=None, normalize=False,
                                    snr_gamma=0.0, prediction_type="epsilon"):
    """huber_c tap == the schedule table at the drawn timesteps; dpred, loss_per_sample and loss == the restated chain of the tapped
    pred, target and effective mask, bit for bit; loss and loss_per_sample within the derived bound of the float64 reference."""
    t = rr.TYPES[loss_type]
    pred, target = aux["pred"][..., :C].float().cpu().numpy(), aux["target"].cpu().numpy()
    B, h, w, _ = pred.shape
    table = tu.huber_threshold_table(sched_state.alphas_cumprod.cpu().numpy(), huber_c, schedule)
    c = table[timesteps.cpu().numpy()]
    assert aux["huber_c"].dtype == F32 and aux["huber_c"].cpu().numpy().tobytes() == c.tobytes(), "thresholds against the schedule table"
    e = aux["loss_mask"].cpu().numpy() if "loss_mask" in aux else None
    w1 = tu._min_snr_weights(sched_state, timesteps.to(torch.int32), snr_gamma, prediction_type).cpu().numpy() if snr_gamma else None
    sums = rr.kernel_sums32(e) if normalize else None
    k32 = mr.sample_factors(B, h * w, sums, w1, lw, normalize, dtype=np.float32)
    want_dp, terms = rr.chain(pred, target, c, t, e, k32)
    dp = aux["dpred"].cpu()
    assert torch.equal(dp[..., :C].contiguous().view(torch.int16), want_dp.view(torch.int16)), "dpred against the restated chain"
    assert not dp[..., C:].float().any(), "dpred's padding channels"
    want_loss, want_lps = rr.ordered_loss(terms, k32, C, 0.0)
    loss, lps = out[4]["loss"].cpu().numpy(), out[4]["loss_per_sample"].cpu().numpy()
    ref = rr.reference(pred, target, c, t, e, w1, lw, normalize)
    print(f"{loss_type} {schedule}: c {c.tolist()} loss {float(loss)!r} chain {float(want_loss)!r} float64 {ref['loss']!r}; per sample {lps.tolist()} "
          f"float64 {ref['loss_per_sample'].tolist()}")
    assert loss.tobytes() == want_loss.tobytes() and lps.tobytes() == want_lps.tobytes(), "loss / loss_per_sample against the ordered chain"
    m = C * h * w
    assert ref["loss"] > 0 and abs(float(loss) - ref["loss"]) <= rr.gamma(m + h * w + B + 13) * ref["loss"]
    assert (np.abs(lps.astype(np.float64) - ref["loss_per_sample"]) <= rr.gamma(m + h * w + 11) * ref["loss_per_sample"]).all()
    return c


# ================================================================================================ "l2" is the plain step
def test_explicit_l2_trains_like_the_plain_step_bit_for_bit(dev):
    """loss_type="l2" with other huber options: the plain step's launches - every trained buffer, the loss and the generator state equal,
    and no loss_per_sample."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64, sched="zero_snr_scaled_linear")
    snaps, gens = [], []
    for kw in ({}, dict(loss_type="l2", huber_c=0.3, huber_schedule="constant")):
        states = build_hip_states(case, dev, prediction_type="v_prediction", ema=True)[1]
        out, gen = _step(tu, states, to_dev(case["batch"], dev), dev, min_snr_gamma_magnitude=5.0, **kw)
        assert set(out[4]) == {"loss"}
        snaps.append(_snapshot(states[0], states[1], out))
        gens.append(gen.get_state().clone())
        del states
    _assert_same(snaps[0], snaps[1], "explicit l2 against the plain step")
    assert torch.equal(gens[0], gens[1])


# ================================================================================================ values against the aux taps
@pytest.mark.parametrize("loss_type,schedule,full", [("huber", "snr", False), ("smooth_l1", "exponential", True), ("huber", "constant", True)])
def test_loss_launch_equals_the_reference_of_the_aux_taps(dev, loss_type, schedule, full):
    """A plain batch, and (full) a batch with mask + floor + normalisation + loss_weight + min-SNR.  The plain batch's timesteps are
    (T - 1, 17): on the zero-terminal-SNR schedule the first sample's threshold is huber_c itself (sigma = inf)."""
    from stable_diffusion_training_amd import training_utils as tu
    B, C = 2, 4
    case = make_case("tiny", B=B, image=64, sched="zero_snr_scaled_linear")
    states = build_hip_states(case, dev, prediction_type="v_prediction")[1]
    batch, lw = dict(case["batch"]), None
    if full:
        lw = np.array([1.0, 0.3], np.float32)
        batch.update(loss_mask=_pixel_mask(B, 64, 2), loss_weight=torch.from_numpy(lw))
    # (with min-SNR weights a v-prediction sample at T - 1 has weight 0: the full batch draws an interior timestep instead)
    rand = to_dev(dict(case["rand"], timesteps=torch.tensor([600 if full else 999, 17])), dev)
    aux = {}
    kw = dict(masked_loss_floor=0.25, normalize_masked_area=True, min_snr_gamma_magnitude=5.0) if full else {}
    out, _ = _step(tu, states, to_dev(batch, dev), dev, rand=rand, aux=aux, loss_type=loss_type, huber_c=0.1, huber_schedule=schedule, **kw)
    assert ("loss_mask" in aux) == full
    c = _check_loss_launch_against_taps(tu, states[5].params, out, aux, rand["timesteps"], loss_type, 0.1, schedule, C=C, lw=lw, normalize=full,
                                        snr_gamma=5.0 if full else 0.0, prediction_type="v_prediction")
    if schedule == "snr":
        assert c[0] == np.float32(0.1) and c[1] > 0.5


# ================================================================================================ captured and eager
def test_captured_huber_step_equals_eager(dev):
    """The step table with loss_type / huber_c / huber_schedule through step_overrides, plain batches: two eager warm-ups, capture on the
    third call, replay on the fourth.  Every step's state, loss and loss_per_sample equal the eager run's bit for bit (the thresholds are
    gathered on the device from the table the warm-ups left there)."""
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = make_case("tiny", B=2, image=64)
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph,
                                                    step_overrides=dict(loss_type="huber", huber_c=0.2, huber_schedule="snr"))
        batch = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace = []
        for step in range(4):
            fn = table[tu.step_key(batch)]
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            trace.append(_snapshot(us, ts, out))
        if use_graph:
            assert fn.graph is not None and fn.calls == 2 and us.step == 4
        assert set(sc.params._huber_tables) == {("snr", 0.2)}
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 4 and all(s["loss_per_sample"].shape == (2,) for s in graph)
    for step, (a, b) in enumerate(zip(eager, graph)):
        _assert_same(a, b, f"graph replay against the eager run at step {step}")


# ================================================================================================ micro-batches
def test_huber_micro_batches_match_the_step_over_the_whole_batch(dev):
    """test_masked_micro_batches_match_the_masked_step_over_the_whole_batch (tests/test_gpu_masked_loss.py) with loss_type="huber": the
    same batch of 4 with masks, weights and normalisation, the same draws and the same gates (loss 1e-2, gradient norm 3e-2, cosine >
    0.995, worst leaf < 0.1, update signs > 0.97), micro_batches=2 against the step over all 4 samples; loss_per_sample is the
    micro-batches' concatenated.  The loss launch is the same in both (dpred differs by the factor 2 of inv_count, exactly): what the
    gates see is the bf16 noise of two backward passes over different batch sizes.  Measured on an MI355X: this test's worst leaf is
    0.071 (conv_in/bias; cosine 0.99935).  On the same batch without masks the worst
    leaf (a LayerNorm bias, a sum that cancels) is 0.054 under l2, 0.062 under smooth_l1 and 0.088 under huber at huber_c 0.1, whose
    gradient saturates at +-2c and so carries less signal into such sums; with min-SNR weights on top (one sample at weight 0.07)
    that leaf reaches 0.104, which is why min-SNR is checked on the loss launch (the aux-tap test) and not through this noise gate."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests.test_gpu_masked_loss import _masked_batch_of_4
    case = make_case("tiny", B=4, image=64)
    got = {}
    for K in (1, 2):
        states = build_hip_states(case, dev)[1]
        us, ts = states[0], states[1]
        before = {n: st.store.master.clone() for n, st in (("unet", us), ("text", ts))}
        out, _ = _step(tu, states, _masked_batch_of_4(case, dev), dev, rand=to_dev(case["rand"], dev), micro_batches=K,
                       normalize_masked_area=True, loss_type="huber", huber_c=0.1, huber_schedule="snr")
        got[K] = dict(loss=float(out[4]["loss"]), lps=out[4]["loss_per_sample"].cpu(),
                      stores={n: (st.store.grad_norm(), {k: v.float().cpu() for k, v in st.store.export("grad").items()},
                                  torch.sign(st.store.master - before[n]).cpu()) for n, st in (("unet", us), ("text", ts))})
        del states
    a, b = got[1], got[2]
    assert b["lps"].shape == (4,) and a["lps"].shape == (4,)
    assert abs(b["loss"] - a["loss"]) / a["loss"] < 1e-2 and abs(float(b["lps"].mean()) - b["loss"]) < 1e-5 * b["loss"]
    assert ((b["lps"] - a["lps"]).abs() <= 1e-2 * a["lps"]).all()
    for n in ("unet", "text"):
        (gn1, g1, s1), (gn2, g2, s2) = a["stores"][n], b["stores"][n]
        assert abs(gn2 - gn1) / gn1 < 3e-2, (n, gn1, gn2)
        f1, f2 = torch.cat([g1[k].flatten() for k in g1]), torch.cat([g2[k].flatten() for k in g1])
        cos = float(torch.dot(f1, f2) / (f1.norm() * f2.norm()))
        worst = max((rel_l2(g2[k], g1[k]), k) for k in g1 if g1[k].norm() > 1e-3 * f1.norm())
        print(f"{n}: gradient norm {gn1!r} against {gn2!r}, cosine {cos!r}, worst leaf {worst}")
        assert cos > 0.995, f"{n}: gradient cosine {cos}"
        assert worst[0] < 0.1, f"{n}: worst leaf {worst}"
        assert float((s1 == s2).float().mean()) > 0.97, f"{n}: update sign agreement"


# ================================================================================================ the example loop
def test_example_loop_passes_the_loss_options_to_its_captured_steps(tmp_path):
    """examples/train_synthetic.py with loss_type / huber_c / huber_schedule in its config, over one chunk of aspect-ratio buckets
    (captured steps): the options reach the steps - every loss differs from the l2 run's and is what a second huber run gives."""
    import importlib.util
    import json
    import os
    from oracle import nets as onets
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
    runs = {}
    for name in ("l2", "huber", "huber_again"):
        d = tmp_path / name
        d.mkdir()
        cfg = dict(base)
        cfg.update(model_path=str(d / "model@0"), batch_size=2, image_area_root=[128], minimum_axis_length=[64],
                   context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
                   ema_rate=0.99, repeat_batch=3, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
                   loss_logging_interval=1, loss_csv=str(d / "loss.csv"), test_save_path=str(d / "test_save"), batches_per_chunk=6, DEBUG=False)
        if name != "l2":
            cfg.update(loss_type="huber", huber_c=0.2, huber_schedule="exponential")
        losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
        assert us.step == 6 and len(losses) == 6 and all(np.isfinite(v) and v > 0 for v in losses)
        runs[name] = losses
        del us, ts
    assert runs["huber"] == runs["huber_again"]
    assert all(a != b for a, b in zip(runs["l2"], runs["huber"])), "the loss options did not reach the steps"


# ================================================================================================ LoRA
def test_lora_step_under_the_smooth_l1_loss(dev):
    """One LoRA step (adapters on both models) with loss_type="smooth_l1": the loss launch equals the reference of its taps and the
    adapters' trained state moves."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests.test_gpu_lora import _lora_states
    case = make_case("tiny", B=2, image=64)
    states = _lora_states(case, dev, ema=True)[1]
    us, ts = states[0], states[1]
    assert us.adapter is not None and ts.adapter is not None
    start = us.adapter.store.master.clone()
    rand, aux = to_dev(case["rand"], dev), {}
    out, _ = _step(tu, states, to_dev(case["batch"], dev), dev, rand=rand, aux=aux, loss_type="smooth_l1", huber_c=0.1, huber_schedule="snr")
    assert us.adapter.store.count == 1 and not torch.equal(us.adapter.store.master, start)
    _check_loss_launch_against_taps(tu, states[5].params, out, aux, rand["timesteps"], "smooth_l1", 0.1, "snr", C=4)


# ================================================================================================ cache and pixels
def test_huber_step_from_a_latent_cache_equals_the_pixel_step_bit_for_bit(dev, tmp_path):
    """A step from latent_cache's Reader, without a VAE, equals the pixel step under the huber loss (mask, weights and offset noise on)
    in every trained buffer, the loss, loss_per_sample and the generator state."""
    from stable_diffusion_training_amd import latent_cache as lc
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    pixel_batch = dict(case["batch"], loss_mask=_pixel_mask(2, 64, 30), loss_weight=torch.tensor([1.0, 0.25]))
    kw = dict(masked_loss_floor=0.125, normalize_masked_area=True, offset_noise_magnitude=0.1, loss_type="huber", huber_c=0.05,
              huber_schedule="exponential")
    snaps = []
    for cached in (False, True):
        states = list(build_hip_states(case, dev, ema=True)[1])
        batch = to_dev(pixel_batch, dev)
        if cached:
            assert lc.build([pixel_batch], states[4], str(tmp_path / "cache")) == 1
            batch = lc.Reader(str(tmp_path / "cache"), device=dev, vae=states[4]).grab_next_batch()
            assert set(batch) == {"latent_moments", "input_ids", "loss_mask", "loss_weight"}
            states[4] = None
        out, gen = _step(tu, states, batch, dev, **kw)
        snap = _snapshot(states[0], states[1], out)
        snap["generator"] = gen.get_state().clone()
        assert snap["loss_per_sample"].shape == (2,) and float(snap["loss"]) > 0
        snaps.append(snap)
        del states
    _assert_same(snaps[0], snaps[1], "the cached huber step against the pixel step")
