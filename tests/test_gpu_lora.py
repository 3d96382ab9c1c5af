"""LoRA training on the MI355X at model level (lora.py, train_step with adapter states), on the tiny configuration: a UNet with a
non-mergeable width (32), merged q|k|v and merged context projections at width 64 and a 48-wide context.  The oracle is unchanged:
it runs on fp32 trees with the adapters folded in by the float64 reference, and its gradients are projected by the float64 reference
(tests/lora_reference.py)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import lora_reference as lr
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu
RANK, ALPHA = 8, 4.0
STATE = ("master", "codes", "inv_scale", "mom", "ema")


def _models(case):
    return {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
            "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
            "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}


def _lora_states(case, dev, te="lora", ema=False, prediction_type="epsilon", unet_targets=None):
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
    tc = tu.TrainingConfig(
        model_path="synthetic", batch_size=case["batch"]["pixel_values"].shape[0], learning_rate=1e-6, unet_learning_rate=1e-6,
        text_encoder_learning_rate=1e-6, lr_scheduler="constant", adam_to_lion_scale_factor=7.0, compilation_cache_path="",
        keep_compiled_fn_in_cache=False, text_encoder_context_window=77, context_window_concatenation_count=1,
        aot_compile=True, strip_bos_eos_token=False, offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0,
        perturbation_noise_magnitude=0.0, image_area_root=[512], minimum_axis_length=[512], beta_scheduler=case["sched"],
        prediction_type=prediction_type, excluded_layer_pattern_from_weight_decay=["bias", "scale", "embedding"],
        excluded_layer_from_quantization=["bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj"],
        quant_block_size=16, quantize_unet_state=True, quantize_text_encoder_state=True,
        accumulate_unet_ema=ema, accumulate_text_encoder_ema=ema, ema_rate=0.999)
    cfg = dict(unet=lora.LoraConfig(RANK, ALPHA, seed=1, **({} if unet_targets is None else {"targets": unet_targets})),
               text_encoder=lora.LoraConfig(RANK, ALPHA, targets=lora.CLIP_TARGETS, seed=2) if te == "lora" else "frozen")
    return tc, tu.on_device_model_training_state(tc, _models(case), device=dev, lora=cfg)


def _random_factors(ad, weights, seed, rel=0.1):
    """{adapter path: tensor}: random A and B, scaled so that the delta s * A @ B is `rel` of its base kernel's norm."""
    g = torch.Generator().manual_seed(seed)
    tree = {}
    for p in ad.paths:
        a, b = ad.adapted[p]
        K, N = weights[p].shape
        A, B = torch.randn(K, ad.cfg.rank, generator=g), torch.randn(ad.cfg.rank, N, generator=g)
        c = rel * float(weights[p].double().norm()) / float((ad.cfg.scale * lr.bf(A) @ lr.bf(B)).norm())
        tree[a], tree[b] = A * c ** 0.5, B * c ** 0.5
    return tree


def _folded64(ad, weights, factors):
    """The fp32 tree the oracle runs on: W0 + s * bf16(A) @ bf16(B) (float64 reference) for adapted kernels."""
    out = dict(weights)
    for p in ad.paths:
        a, b = ad.adapted[p]
        out[p] = lr.merge_ref64(weights[p], factors[a], factors[b], ad.cfg.scale).float()
    return out


def _project_tree(ad, grads, factors):
    """The oracle's kernel gradients projected onto the factors by the float64 reference."""
    out = {}
    for p in ad.paths:
        a, b = ad.adapted[p]
        dA, dB = lr.project_ref64(torch.as_tensor(grads[p]), factors[a], factors[b], ad.cfg.scale)
        out[a], out[b] = dA.float(), dB.float()
    return out


def _gates(store, ref, what):
    """test_tiny_train_step_parity's gradient gates on an adapter store against the projected oracle gradients."""
    g = store.export("grad")
    flat = torch.cat([g[k].flatten().cpu() for k in ref])
    rflat = torch.cat([ref[k].flatten() for k in ref])
    cos = float(torch.dot(flat, rflat) / (flat.norm() * rflat.norm()))
    worst = max((rel_l2(g[k], ref[k]), k) for k in ref if ref[k].norm() > 1e-3 * rflat.norm())
    gn = float(rflat.double().norm())
    print(f"[{what}] cosine {cos:.5f}, worst leaf {worst[0]:.4f} ({worst[1]}), |g| {store.grad_norm():.5e} vs {gn:.5e}")
    assert cos > 0.995, f"{what}: gradient cosine {cos}"
    assert worst[0] < 0.1, f"{what}: worst leaf {worst}"
    assert abs(store.grad_norm() - gn) / gn < 3e-2, (what, store.grad_norm(), gn)
    return g


def _oracle(case, unet_w, clip_w):
    from oracle import train_step as ots
    return ots.train_step(unet_w, clip_w, case["weights"]["vae"], case["sched_state"], case["cfgs"], case["batch"], case["rand"],
                          dict(ots.DEFAULT_OPT))


def _step(tu, st, case, dev, **kw):
    us, ts, ue, te, vae, sc, _ = st
    return tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                         rand=to_dev(case["rand"], dev), **kw)


# ------------------------------------------------------------------------------------------------ 1
def test_zero_b_gives_the_bits_of_the_base(dev):
    """B = 0 as initialised: the merged mirror is the base's own and the prediction of the LoRA step equals, bit for bit, the one of
    a full fine-tune state built from the same weights."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    preds = []
    for build in (lambda: build_hip_states(case, dev)[1], lambda: _lora_states(case, dev)[1]):
        st, aux = build(), {}
        out = _step(tu, st, case, dev, aux=aux)
        assert np.isfinite(out[4]["loss"].item())
        preds.append(aux["pred"].clone())
    assert torch.equal(preds[0], preds[1])


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("te", ["lora", "frozen", "frozen-ff"])
def test_adapter_gradients_match_the_projected_oracle_gradients(dev, te):
    """frozen-ff: the feed-forward kernels carry the adapters instead of the attention projections - the scratch path of the fused
    feed-forward backward's two weight gradients, which the default targets never take."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    ff = te == "frozen-ff"
    te = "frozen" if ff else te
    tc, st = _lora_states(case, dev, te=te, unet_targets=("net_0", "net_2") if ff else None)
    if ff:
        assert st[0].adapter.paths and all("/ff/net_0/proj/" in p or "/ff/net_2/" in p for p in st[0].adapter.paths)
    us, ts = st[0], st[1]
    fu = _random_factors(us.adapter, case["weights"]["unet"], 11)
    us.adapter.store.load(fu)
    unet_w, clip_w, ft = _folded64(us.adapter, case["weights"]["unet"], fu), case["weights"]["clip"], None
    if te == "lora":
        ft = _random_factors(ts.adapter, case["weights"]["clip"], 12)
        ts.adapter.store.load(ft)
        clip_w = _folded64(ts.adapter, case["weights"]["clip"], ft)
    else:
        assert ts.adapter is None and ts.opt_store is None and not ts.store.trainable
    ref = _oracle(case, unet_w, clip_w)
    out = _step(tu, st, case, dev)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    want = _project_tree(us.adapter, ref["unet_grads"], fu)
    g = _gates(us.adapter.store, want, f"unet adapters, text encoder {te}")
    if te == "lora":
        _gates(ts.adapter.store, _project_tree(ts.adapter, ref["te_grads"], ft), "text-encoder adapters")
    elif not ff:
        # the context projections of a frozen text encoder: their backward runs only because _context_projections anchors the tape
        kv = [q for p in us.adapter.paths if "/attn2/to_k/" in p or "/attn2/to_v/" in p for q in us.adapter.adapted[p]]
        assert len(kv) == 4 * sum(1 for p in us.adapter.paths if "/attn2/to_k/" in p)
        for q in kv:
            assert float(g[q].abs().max()) > 0, f"{q}: no gradient"
            assert rel_l2(g[q], want[q]) < 0.1, (q, rel_l2(g[q], want[q]))
    assert us.step == 1 and us.store.count == 0


# ------------------------------------------------------------------------------------------------ 3
def test_step_semantics(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _lora_states(case, dev, ema=True)
    for state, seed, weights in ((st[0], 21, case["weights"]["unet"]), (st[1], 22, case["weights"]["clip"])):
        state.adapter.store.load(_random_factors(state.adapter, weights, seed))
    before = []
    for state in st[:2]:
        ad = state.adapter
        before.append(dict(master=state.store.master.clone(), w=state.store.w.clone(), folded=ad.folded(),
                           amaster=ad.store.master.clone(), ema=ad.store.ema.clone()))
    out = _step(tu, st, case, dev, ema_rate=0.999)
    torch.cuda.synchronize()
    assert out[2] is st[2] and out[3] is st[3] and st[2].store is st[0].adapter.store
    for state, b in zip(st[:2], before):
        base, ad = state.store, state.adapter
        assert torch.equal(base.master, b["master"]), "the frozen master moved"
        adapted = torch.zeros(base.w.numel(), dtype=torch.bool, device=dev)
        for p in ad.paths:
            lf = base.leaves[p]
            adapted[lf.w_off: lf.w_off + lf.numel] = True
            assert torch.equal(base.w[lf.w_off: lf.w_off + lf.numel].view(lf.shape), b["folded"][p].to(torch.bfloat16)), p
        assert torch.equal(base.w[~adapted], b["w"][~adapted]), "the mirror of a non-adapted leaf was rewritten"
        # Lion: p' = p - lr * (sign(c) + wd * p), c = (1 - b1) * g on the first step: every element with a gradient moves by lr
        lr_, wd = state.hyper["lr"], state.hyper["wd"]
        p0, p1, g = b["amaster"].double(), ad.store.master.double(), ad.store.grad_flat().double()
        moved = (p1 - p0 + lr_ * wd * p0).abs()
        ulp = torch.maximum(p0.abs(), p1.abs()).float().abs().clamp_min(1e-30)
        ulp = (torch.nextafter(ulp, torch.full_like(ulp, float("inf"))) - ulp).double()
        nz = g != 0
        assert int(nz.sum()) > 0.9 * sum(lf.numel for lf in ad.store.leaves.values())
        assert bool(((moved[nz] - lr_).abs() <= 2 * ulp[nz]).all()), float(((moved[nz] - lr_).abs() / ulp[nz]).max())
        assert bool((torch.sign(p0 - p1)[nz] == torch.sign(g)[nz]).float().mean() > 0.99)
        want = 0.999 * b["ema"].double() + (1 - 0.999) * p1
        assert torch.allclose(ad.store.ema.double(), want, atol=1e-6, rtol=0)
        assert state.step == 1


# ------------------------------------------------------------------------------------------------ 4, 5
_RUNS = {}


def _trajectory(dev, use_graph, fresh=False):
    """Four steps through dp_compile_all_unique_resolution with explicit draws; per step the adapter stores' state and a digest."""
    key = ("traj", use_graph)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = _lora_states(case, dev, ema=True)
    for state, seed, weights in ((us, 31, case["weights"]["unet"]), (ts, 32, case["weights"]["clip"])):
        state.adapter.store.load(_random_factors(state.adapter, weights, seed))
    table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph, per_device_batch=2)
    fn = table[[k for k in table if k[2] == 512 and k[3] == 512][0]]
    assert isinstance(fn, tu._GraphedStep) == use_graph
    gen = torch.Generator(device=dev)
    trace = []
    for step in range(4):
        g = torch.Generator().manual_seed(100 + step)
        batch = to_dev(case["batch"], dev)
        batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
        rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
                for k, v in case["rand"].items()}
        out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
        snap = {"loss": out[4]["loss"].clone()}
        for name, state in (("unet", us), ("text", ts)):
            for b in STATE:
                snap[f"{name}.{b}"] = getattr(state.adapter.store, b).clone()
        trace.append(snap)
    if use_graph:
        assert fn.graph is not None and fn.calls == 2
    assert us.step == 4 and ts.step == 4 and us.store.count == 0
    h = hashlib.sha256()
    for name in ("unet.master", "text.master"):
        h.update(trace[-1][name].cpu().numpy().tobytes())
    _RUNS[key] = (trace, h.hexdigest())
    return _RUNS[key]


def test_captured_steps_equal_eager_steps(dev):
    eager, graph = _trajectory(dev, False)[0], _trajectory(dev, True)[0]
    assert len({float(s["loss"]) for s in graph}) == 4
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager step at step {step}, {k}"
    assert not torch.equal(eager[0]["unet.master"], eager[3]["unet.master"])


def test_four_steps_are_reproducible(dev):
    first = _trajectory(dev, False)
    again = _trajectory(dev, False, fresh=True)
    assert first[1] == again[1]


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("te", ["frozen", "lora"])
def test_micro_batches_match_the_full_batch_oracle_step(dev, te):
    """micro_batches=2 on B = 4 against the oracle's one step over all four samples: test_gpu_grad_accum's comparison and its loss,
    cosine, worst-leaf and norm gates, on one adapter store (text encoder frozen) and on two.  That test's update-sign-agreement gate
    has no counterpart here: the oracle steps the full weights with its own optimizer and has no adapter leaves whose updates could be
    compared (the adapter's update is checked in test_step_semantics)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    tc, st = _lora_states(case, dev, te=te)
    us, ts = st[0], st[1]
    fu = _random_factors(us.adapter, case["weights"]["unet"], 41)
    us.adapter.store.load(fu)
    clip_w = case["weights"]["clip"]
    if te == "lora":
        ft = _random_factors(ts.adapter, clip_w, 42)
        ts.adapter.store.load(ft)
        clip_w = _folded64(ts.adapter, clip_w, ft)
    ref = _oracle(case, _folded64(us.adapter, case["weights"]["unet"], fu), clip_w)
    out = _step(tu, st, case, dev, micro_batches=2)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    assert us.adapter.store.gacc is not None
    _gates(us.adapter.store, _project_tree(us.adapter, ref["unet_grads"], fu), f"K=2 accumulated unet adapters, text encoder {te}")
    if te == "lora":
        assert ts.adapter.store.gacc is not None
        _gates(ts.adapter.store, _project_tree(ts.adapter, ref["te_grads"], ft), "K=2 accumulated text-encoder adapters")


# ------------------------------------------------------------------------------------------------ 7
def test_checkpoint_resume_is_bitwise(dev, tmp_path):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    path = str(tmp_path / "state.safetensors")

    def fresh(seed):
        tc, st = _lora_states(case, dev, ema=True)
        for state, s, weights in ((st[0], seed, case["weights"]["unet"]), (st[1], seed + 1, case["weights"]["clip"])):
            state.adapter.store.load(_random_factors(state.adapter, weights, s))
        return st

    def two_steps(st, gen):
        for _ in range(2):
            us, ts, ue, te, vae, sc, _ = st
            out = tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), gen, vae, sc, strip_bos_eos_token=False, ema_rate=0.999)
        snap = {f"{n}.{b}": getattr(s.adapter.store, b).clone() for n, s in (("unet", st[0]), ("text", st[1])) for b in STATE}
        snap["loss"] = out[4]["loss"].clone()
        snap["unet.w"] = st[0].store.w.clone()
        return snap

    st, gen = fresh(51), torch.Generator(device=dev)
    gen.manual_seed(5)
    tu.train_step(st[0], st[1], st[2], st[3], to_dev(case["batch"], dev), gen, st[4], st[5], strip_bos_eos_token=False, ema_rate=0.999)
    tu.save_training_state(path, st[0], st[1], train_rng=gen)
    from safetensors import safe_open
    with safe_open(path, framework="pt", device="cpu") as f:
        assert f.get_tensor("unet.master").numel() == st[0].adapter.store.total  # the adapter's leaves: the frozen base is not written
    a = two_steps(st, gen)
    st2, gen2 = fresh(61), torch.Generator(device=dev)  # other factors: everything must come from the file
    tu.load_training_state(path, st2[0], st2[1], train_rng=gen2)
    assert st2[0].step == 1 and st2[1].step == 1
    b = two_steps(st2, gen2)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 8
def test_sampling_uses_the_adapter_and_equals_the_folded_checkpoint(dev):
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.params import ParamStore
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = make_case("tiny", B=2, image=64)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    tc, st = _lora_states(case, dev, ema=True)
    us, ts = st[0], st[1]
    for state, seed, weights in ((us, 71, case["weights"]["unet"]), (ts, 72, case["weights"]["clip"])):
        state.adapter.store.load(_random_factors(state.adapter, weights, seed, rel=0.3))
        state.adapter.store.ema.mul_(0.5)  # an EMA that differs from the master
    ids = case["batch"]["input_ids"].to(dev)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)

    def generate(unet, text):
        pipe = StableDiffusionPipeline(unet, text, vae_w, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], device=dev)
        return pipe.generate(ids, num_inference_steps=2, height=64, width=64, latents=lat)

    def plain(unet_tree, clip_tree):
        u = ParamStore(nets.unet_spec(case["cfgs"]["unet"]), device=dev, trainable=False)
        t = ParamStore(nets.clip_text_spec(case["cfgs"]["clip"]), device=dev, trainable=False)
        u.load(unet_tree)
        t.load(clip_tree)
        return u, t

    with_adapter = generate(us, ts)
    base = generate(*plain(case["weights"]["unet"], case["weights"]["clip"]))
    assert not torch.equal(with_adapter, base)
    assert torch.equal(with_adapter, generate(*plain(us.adapter.folded(), ts.adapter.folded())))
    us.adapter.merge(source="ema")
    ts.adapter.merge(source="ema")
    ema_img = generate(us, ts)
    assert not torch.equal(ema_img, with_adapter)
    assert torch.equal(ema_img, generate(*plain(us.adapter.folded(source="ema"), ts.adapter.folded(source="ema"))))


# ------------------------------------------------------------------------------------------------ 9
def test_a_reducer_is_refused(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _lora_states(case, dev, te="frozen")
    with pytest.raises(ValueError, match="GradReducer over the adapter stores"):
        _step(tu, st, case, dev, reducer=object())


# ------------------------------------------------------------------------------------------------ 10
def test_sd15_structure_one_step(dev):
    """SD1.5 (1x1-conv proj_in / proj_out, merged groups of every width): one eager LoRA step - finite loss, every adapter leaf
    reported written exactly once, no leaf of a frozen base written."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("sd15", B=2, image=64)
    tc, st = _lora_states(case, dev)
    seen = {}
    for state in st[:2]:
        for store in (state.store, state.adapter.store):
            def note(path, store=store, real=store.note_written):
                seen.setdefault(id(store), []).append(path)
                real(path)
            store.note_written = note
    out = _step(tu, st, case, dev)
    assert np.isfinite(out[4]["loss"].item())
    for state in st[:2]:
        assert id(state.store) not in seen, "a gradient leaf of a frozen base was written"
        got = seen[id(state.adapter.store)]
        assert sorted(got) == sorted(state.adapter.store.order) and len(set(got)) == len(got)
        g = state.adapter.store.grad_flat()
        assert bool(torch.isfinite(g).all())
    lora_b = [q for p in st[0].adapter.paths for q in st[0].adapter.adapted[p][1:]]
    gb = st[0].adapter.store.export("grad")
    assert all(float(gb[q].abs().max()) > 0 for q in lora_b), "an adapted UNet leaf received no gradient"
