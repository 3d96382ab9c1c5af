"""train_step with a loss mask and per-sample loss weights on the MI355X (tiny model): the unit mask against the plain step, a fully
masked-out sample, loss values against the float64 reference of the aux taps, captured against eager steps, micro-batches, a latent
cache built from masked pixel batches, and a LoRA step.  Kernel-level checks: tests/test_gpu_masked_loss_kernels.py."""
import numpy as np
import pytest
import torch

from tests import masked_loss_reference as mr
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")
U = 2.0 ** -24  # unit roundoff of fp32


def _snapshot(us, ts, out=None):
    snap = {}
    for name, state in (("unet", us), ("text", ts)):
        st = state.opt_store
        if st is not None:
            snap.update({f"{name}.{b}": getattr(st, b).clone() for b in STATE if getattr(st, b, None) is not None})
            snap[f"{name}.sqnorm"] = st.sqnorm.clone()
    if out is not None:
        snap.update({k: v.clone() for k, v in out[4].items()})
    return snap


def _assert_same(a, b, what, skip=()):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        if k in skip:
            continue
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        same = torch.equal(x.view(torch.int16), y.view(torch.int16)) if x.dtype == BF else torch.equal(x, y)
        assert same, f"{what}: {k} differs ({(x.double() - y.double()).abs().max().item():.3e} max abs)"


def _pixel_mask(B, image, seed, zero=None):
    """(B, image, image) f32: a rectangle of ones on a background of fractional values, the bottom quarter zero, a few values outside
    [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, image, image, generator=g) * 0.5
    m[:, image // 4: 3 * image // 4, image // 8: image // 2] = 1.0
    m[:, -(image // 4):, :] = 0.0
    m[:, 0, :4] = torch.tensor([-0.5, 1.5, 0.0, 1.0])
    if zero is not None:
        m[zero] = 0.0
    return m.contiguous()


def _step(tu, states, batch, dev, rand=None, **kw):
    us, ts, ue, te, vae, sc, _ = states
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999, rand=rand, **kw)
    torch.cuda.synchronize()
    return out, gen


# ================================================================================================ unit mask == plain step
def test_unit_mask_and_weights_train_like_the_plain_step_bit_for_bit(dev):
    """An all-ones loss_mask and unit loss_weight (min-SNR weights on): dpred is the plain kernel's in every bit, so masters, optimizer
    state, EMA and gradient norms equal the plain step's from the same state and draws; the generator ends in the same state.  The two
    losses are fp32 sums of the same n = B*C*h*w non-negative terms in two orders (one over the batch; per sample first, the weight
    applied to the sample's sum), each term carrying at most 2 roundings: |difference| <= 2 (n + 4) u loss."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64, sched="zero_snr_scaled_linear")
    snaps, gens = [], []
    for masked in (False, True):
        states = build_hip_states(case, dev, prediction_type="v_prediction", ema=True)[1]
        batch = to_dev(case["batch"], dev)
        if masked:
            batch = dict(batch, loss_mask=torch.ones(2, 64, 64, device=dev), loss_weight=torch.ones(2, device=dev))
        out, gen = _step(tu, states, batch, dev, min_snr_gamma_magnitude=5.0)
        assert ("loss_per_sample" in out[4]) == masked
        snaps.append(_snapshot(states[0], states[1], out))
        gens.append(gen.get_state().clone())
        del states
    lps = snaps[1].pop("loss_per_sample")
    _assert_same(snaps[0], snaps[1], "unit mask against the plain step", skip=("loss",))
    assert torch.equal(gens[0], gens[1]), "the masked step took other draws from train_rng"
    a, b = float(snaps[0]["loss"]), float(snaps[1]["loss"])
    n = 2 * 4 * 8 * 8
    print(f"plain loss {a!r}, unit-mask loss {b!r}, bound {2 * (n + 4) * U * a:.3e}")
    assert a > 0 and abs(a - b) <= 2 * (n + 4) * U * a
    assert lps.shape == (2,) and abs(float(lps.mean()) - b) <= 4 * U * b


# ================================================================================================ a fully masked-out sample
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalized"])
def test_a_fully_masked_out_sample_leaves_no_trace_in_the_trained_state(dev, normalize):
    """Batch of 2, the second sample's mask all zero, floor 0: its dpred rows are zero and nothing in the networks mixes samples, so
    other pixels and another caption for that sample leave every trained buffer unchanged; its loss_per_sample is 0 and everything is
    finite (with normalisation its mask sum is 0: factor 0, no NaN)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    other = make_case("tiny", B=2, image=64, seed=5)
    snaps = []
    for changed in (False, True):
        states = build_hip_states(case, dev, ema=True)[1]
        batch = {k: v.clone() for k, v in case["batch"].items()}
        if changed:
            batch["pixel_values"][1] = other["batch"]["pixel_values"][1]
            batch["input_ids"][1] = other["batch"]["input_ids"][1]
        batch = to_dev(dict(batch, loss_mask=_pixel_mask(2, 64, 1, zero=1), loss_weight=torch.tensor([1.0, 2.0])), dev)
        out, _ = _step(tu, states, batch, dev, rand=to_dev(case["rand"], dev), normalize_masked_area=normalize)
        snap = _snapshot(states[0], states[1], out)
        assert all(torch.isfinite(v.float()).all() for k, v in snap.items() if v.dtype.is_floating_point)
        assert float(snap["loss_per_sample"][1]) == 0 and float(snap["loss_per_sample"][0]) > 0
        snaps.append(snap)
        del states
    assert not torch.equal(case["batch"]["input_ids"][1], other["batch"]["input_ids"][1])
    _assert_same(snaps[0], snaps[1], "the masked-out sample changed")


# ================================================================================================ values against the aux taps
@pytest.mark.parametrize("floor,normalize,snr", [(0.0, False, False), (0.25, True, True)])
def test_loss_values_equal_the_float64_reference_of_the_aux_taps(dev, floor, normalize, snr):
    """aux["loss_mask"] equals the reference's effective mask (the fp32 chain: block added in row-major order, times 1/64, floored) in
    every bit.  loss and loss_per_sample against the float64 reference of the tapped pred, target and mask.  Bound: per term 4
    roundings (the fp32 difference twice in the square, two products), the sample's sum of m = C*h*w terms (m - 1), the factor k_b (w1 w2,
    h*w / S_b with S_b an fp32 sum of h*w terms, the product: h*w + 3) and the two final products (2), then for the loss the B terms and
    its scaling (B + 2): relative error <= (m + h*w + 10) u per sample, (m + h*w + B + 12) u for the loss."""
    from stable_diffusion_training_amd import training_utils as tu
    B, C, h, w = 2, 4, 8, 8
    case = make_case("tiny", B=B, image=64, sched="zero_snr_scaled_linear")
    states = build_hip_states(case, dev, prediction_type="v_prediction")[1]
    mask, lw = _pixel_mask(B, 64, 2), torch.tensor([1.0, 0.3])
    batch = to_dev(dict(case["batch"], loss_mask=mask, loss_weight=lw), dev)
    aux = {}
    rand = to_dev(case["rand"], dev)
    out, _ = _step(tu, states, batch, dev, rand=rand, aux=aux, masked_loss_floor=floor, normalize_masked_area=normalize,
                   min_snr_gamma_magnitude=5.0 if snr else 0.0)
    e_want = mr.effective_mask(mr.pooled_mask(mask.numpy(), 8, np.float32), floor)
    e_got = aux["loss_mask"].cpu()
    assert e_got.dtype == F32 and torch.equal(e_got.view(torch.int32), torch.from_numpy(e_want).view(torch.int32)), "effective mask tap"
    assert (e_want >= floor).all() and len(np.unique(e_want)) > 8
    w1 = None
    if snr:
        w1 = tu._min_snr_weights(states[5].params, rand["timesteps"].to(torch.int32), 5.0, "v_prediction").cpu().numpy()
    ref = mr.reference(aux["pred"][..., :C].float().cpu().numpy(), aux["target"].cpu().numpy(), e_want, w1, lw.numpy(), normalize)
    m = C * h * w
    loss, lps = float(out[4]["loss"]), out[4]["loss_per_sample"].cpu().double().numpy()
    print(f"loss {loss!r} reference {ref['loss']!r}; per sample {lps.tolist()} reference {ref['loss_per_sample'].tolist()}")
    assert ref["loss"] > 0 and abs(loss - ref["loss"]) <= (m + h * w + B + 12) * U * ref["loss"]
    assert (np.abs(lps - ref["loss_per_sample"]) <= (m + h * w + 10) * U * ref["loss_per_sample"]).all()


# ================================================================================================ captured and eager
def test_captured_masked_step_equals_eager_and_is_bound_to_its_loss_keys(dev):
    """The table entry of a masked batch (floor and normalisation through step_overrides): two eager warm-ups, capture on the third call,
    replay on the fourth with other masks and weights every step.  Every step's state, loss and loss_per_sample equal the eager run's bit
    for bit; a replay returns its own copy of loss_per_sample.  After capture a batch that drops or adds a loss key raises ValueError."""
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = make_case("tiny", B=2, image=64)
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph,
                                                    step_overrides=dict(masked_loss_floor=0.25, normalize_masked_area=True))
        base = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace, outs = [], []
        for step in range(4):
            batch = dict(base, loss_mask=_pixel_mask(2, 64, 10 + step).to(dev), loss_weight=torch.tensor([1.0, 0.5 + step], device=dev))
            fn = table[tu.step_key(batch)]
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            outs.append(out[4])
            trace.append(_snapshot(us, ts, out))
        if use_graph:
            assert fn.graph is not None and fn.calls == 2 and fn.loss_keys == (True, True)
            assert outs[2]["loss_per_sample"].data_ptr() != outs[3]["loss_per_sample"].data_ptr()
            for drop in ("loss_mask", "loss_weight"):
                with pytest.raises(ValueError, match="adds or drops"):
                    fn(us, ts, ue, te, {k: v for k, v in batch.items() if k != drop}, gen, vae, sc)
            assert us.step == 4
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 4 and all(s["loss_per_sample"].shape == (2,) for s in graph)
    for step, (a, b) in enumerate(zip(eager, graph)):
        _assert_same(a, b, f"graph replay against the eager run at step {step}")


def test_a_step_captured_without_loss_keys_refuses_a_batch_that_adds_one(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev)
    tc.image_area_root, tc.minimum_axis_length = [64], [64]
    fn = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True)[(2, 3, 64, 64)]
    batch = to_dev(case["batch"], dev)
    gen = torch.Generator(device=dev)
    for _ in range(3):
        out = fn(us, ts, ue, te, batch, gen, vae, sc)
    assert fn.graph is not None and fn.loss_keys == (False, False) and set(out[4]) == {"loss"}
    with pytest.raises(ValueError, match="adds or drops"):
        fn(us, ts, ue, te, dict(batch, loss_weight=torch.ones(2, device=dev)), gen, vae, sc)
    assert us.step == 3
    out = fn(us, ts, ue, te, batch, gen, vae, sc)  # and the plain batch still replays
    assert us.step == 4 and torch.isfinite(out[4]["loss"])


# ================================================================================================ micro-batches
def _masked_batch_of_4(case, dev):
    return to_dev(dict(case["batch"], loss_mask=_pixel_mask(4, 64, 21), loss_weight=torch.tensor([1.0, 0.5, 2.0, 1.0])), dev)


def test_identical_masked_micro_batches_equal_the_plain_masked_step_bit_for_bit(dev, monkeypatch):
    """test_gpu_grad_accum's first gate with masks and weights: batch = b ++ b with K = 2 accumulates g + g and halves it, exactly, so
    everything the step writes equals the K = 1 step over b (ordinary norm pass); loss_per_sample is the concatenation."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    monkeypatch.setattr(tu, "_FUSED_NORM", False)
    extra = dict(loss_mask=_pixel_mask(2, 64, 20), loss_weight=torch.tensor([2.0, 0.5]))
    snaps = []
    for K in (1, 2):
        states = build_hip_states(case, dev, ema=True)[1]
        batch, rand = to_dev(dict(case["batch"], **extra), dev), to_dev(case["rand"], dev)
        if K == 2:
            batch, rand = {k: torch.cat([v, v]) for k, v in batch.items()}, {k: torch.cat([v, v]) for k, v in rand.items()}
        out, _ = _step(tu, states, batch, dev, rand=rand, micro_batches=K, masked_loss_floor=0.25, normalize_masked_area=True)
        snaps.append(_snapshot(states[0], states[1], out))
        del states
    lps1, lps2 = snaps[0].pop("loss_per_sample"), snaps[1].pop("loss_per_sample")
    assert lps2.shape == (4,) and torch.equal(lps2, torch.cat([lps1, lps1]))
    _assert_same(snaps[0], snaps[1], "K = 2 over b ++ b against K = 1 over b")


def test_masked_micro_batches_match_the_masked_step_over_the_whole_batch(dev):
    """test_gpu_grad_accum's parity gates (loss 1e-2, gradient norm 3e-2, cosine > 0.995, worst leaf < 0.1, update signs > 0.97) for
    micro_batches=2 on a batch of 4 with masks, weights and normalisation, against the masked step over all 4 samples at once (which the
    tests above tie to the float64 reference): normalisation is per sample, so the accumulated step is the step over the whole batch."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    got = {}
    for K in (1, 2):
        states = build_hip_states(case, dev)[1]
        us, ts = states[0], states[1]
        before = {n: st.store.master.clone() for n, st in (("unet", us), ("text", ts))}
        out, _ = _step(tu, states, _masked_batch_of_4(case, dev), dev, rand=to_dev(case["rand"], dev), micro_batches=K,
                       normalize_masked_area=True)
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
        assert cos > 0.995, f"{n}: gradient cosine {cos}"
        worst = max((rel_l2(g2[k], g1[k]), k) for k in g1 if g1[k].norm() > 1e-3 * f1.norm())
        assert worst[0] < 0.1, f"{n}: worst leaf {worst}"
        assert float((s1 == s2).float().mean()) > 0.97, f"{n}: update sign agreement"


# ================================================================================================ cache and pixels
def test_step_from_a_cache_of_masked_pixel_batches_equals_the_pixel_step_bit_for_bit(dev, tmp_path):
    """latent_cache.build over masked pixel batches stores the pooled mask (before the floor) and the weights; a step from the Reader,
    without a VAE, equals the pixel step with the pixel mask in every trained buffer, the loss and loss_per_sample - at a floor the
    cache never saw."""
    from stable_diffusion_training_amd import latent_cache as lc
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    mask = _pixel_mask(2, 64, 30)
    pixel_batch = dict(case["batch"], loss_mask=mask, loss_weight=torch.tensor([1.0, 0.25]))
    kw = dict(masked_loss_floor=0.125, normalize_masked_area=True, offset_noise_magnitude=0.1)
    snaps = []
    for cached in (False, True):
        states = list(build_hip_states(case, dev, ema=True)[1])
        batch = to_dev(pixel_batch, dev)
        if cached:
            assert lc.build([pixel_batch], states[4], str(tmp_path / "cache")) == 1
            reader = lc.Reader(str(tmp_path / "cache"), device=dev, vae=states[4])
            batch = reader.grab_next_batch()
            assert set(batch) == {"latent_moments", "input_ids", "loss_mask", "loss_weight"} and batch["loss_mask"].shape == (2, 8, 8)
            want = mr.pooled_mask(mask.numpy(), 8, np.float32)
            assert torch.equal(batch["loss_mask"].cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)), "the cached pooled mask"
            assert want.min() < 0.125, "the floor must bite for the cache to prove that it was not applied at build time"
            states[4] = None
        out, gen = _step(tu, states, batch, dev, **kw)
        snap = _snapshot(states[0], states[1], out)
        snap["generator"] = gen.get_state().clone()
        snaps.append(snap)
        del states
    _assert_same(snaps[0], snaps[1], "the cached masked step against the pixel step")


def test_example_loop_with_the_loss_flags_trains_from_pixels_and_from_a_cache_alike(tmp_path):
    """examples/train_synthetic.py with masked_loss, normalize_masked_area and prior_loss_weight in its config, over one chunk of
    aspect-ratio buckets (captured steps): the loader's masks and weights reach the steps (the cache holds them, the losses differ from
    the run without the keys), and the run from cache_latents reproduces the pixel run's losses and weights."""
    import importlib.util
    import json
    import os
    from oracle import nets as onets
    from stable_diffusion_training_amd import latent_cache as lc
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
    for name in ("plain", "pixels", "cached"):
        d = tmp_path / name
        d.mkdir()
        cfg = dict(base)
        cfg.update(model_path=str(d / "model@0"), batch_size=2, image_area_root=[128], minimum_axis_length=[64],
                   context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
                   ema_rate=0.99, repeat_batch=3, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
                   loss_logging_interval=1, loss_csv=str(d / "loss.csv"), test_save_path=str(d / "test_save"), batches_per_chunk=6, DEBUG=False)
        if name != "plain":
            cfg.update(masked_loss=0.1, normalize_masked_area=True, prior_loss_weight=0.5)
        if name == "cached":
            cfg["cache_latents"] = str(d / "latents")
        losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
        assert us.step == 6 and len(losses) == 6
        runs[name] = (losses, us.store.master.clone(), ts.store.master.clone())
        if name == "cached":
            r = lc.Reader(str(d / "latents" / "rank0" / "chunk0"), device="cpu")
            rec = r.grab_next_batch()
            assert rec["loss_mask"].shape == rec["latent_moments"].shape[:3] and rec["loss_weight"].tolist() == [1.0, 0.5]
            assert 0 < float(rec["loss_mask"].mean()) < 1
        del us, ts
    assert runs["pixels"][0] == runs["cached"][0], "the losses of the cached masked loop differ from the pixel loop's"
    assert torch.equal(runs["pixels"][1], runs["cached"][1]) and torch.equal(runs["pixels"][2], runs["cached"][2])
    assert all(a != b for a, b in zip(runs["plain"][0], runs["pixels"][0])), "the loss flags did not reach the steps"


# ================================================================================================ LoRA
def test_lora_step_with_a_mask_obeys_the_masked_out_sample_property(dev):
    """One LoRA step (adapters on both models) with a mask whose second sample is zero: the adapters' trained state moves, and it is the
    same whatever that sample's pixels and caption are."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests.test_gpu_lora import _lora_states
    case = make_case("tiny", B=2, image=64)
    other = make_case("tiny", B=2, image=64, seed=5)
    snaps = []
    for changed in (False, True):
        states = _lora_states(case, dev, ema=True)[1]
        us, ts = states[0], states[1]
        assert us.adapter is not None and ts.adapter is not None
        start = us.adapter.store.master.clone()
        batch = {k: v.clone() for k, v in case["batch"].items()}
        if changed:
            batch["pixel_values"][1] = other["batch"]["pixel_values"][1]
            batch["input_ids"][1] = other["batch"]["input_ids"][1]
        batch = to_dev(dict(batch, loss_mask=_pixel_mask(2, 64, 3, zero=1), loss_weight=torch.tensor([0.5, 1.0])), dev)
        out, _ = _step(tu, states, batch, dev, rand=to_dev(case["rand"], dev), normalize_masked_area=True)
        assert us.adapter.store.count == 1 and not torch.equal(us.adapter.store.master, start)
        assert float(out[4]["loss_per_sample"][1]) == 0 and float(out[4]["loss_per_sample"][0]) > 0
        snaps.append(_snapshot(us, ts, out))
        del states, us, ts
    _assert_same(snaps[0], snaps[1], "the masked-out sample changed the adapters")
