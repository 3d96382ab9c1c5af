"""DoRA training on the MI355X at model level (lora.py with LoraConfig(dora=True), train_step with adapter states), on the tiny
configuration tests/test_gpu_lora.py uses and with its gates.  The oracle is unchanged: it runs on fp32 trees with the adapters folded in
by the float64 reference (W' = v * m / ||v||), and its kernel gradients are pushed through the float64 reference with the norm held
constant (tests/dora_reference.py)."""
import numpy as np
import pytest
import torch

from tests import dora_reference as dr
from tests import lora_reference as lr
from tests import test_gpu_lora as tl  # its builders and gates: _models, _gates, _oracle, _step (nothing of it is collected from here)
from tests.helpers import make_case, to_dev

pytestmark = pytest.mark.gpu
RANK, ALPHA = tl.RANK, tl.ALPHA
STATE = tl.STATE


def _dora_states(case, dev, te="dora", ema=False, dora=True):
    """test_gpu_lora._lora_states with DoRA adapters (dora=False: the same states with plain LoRA adapters)."""
    from stable_diffusion_training_amd import lora
    from stable_diffusion_training_amd import training_utils as tu
    tc = tu.TrainingConfig(
        model_path="synthetic", batch_size=case["batch"]["pixel_values"].shape[0], learning_rate=1e-6, unet_learning_rate=1e-6,
        text_encoder_learning_rate=1e-6, lr_scheduler="constant", adam_to_lion_scale_factor=7.0, compilation_cache_path="",
        keep_compiled_fn_in_cache=False, text_encoder_context_window=77, context_window_concatenation_count=1,
        aot_compile=True, strip_bos_eos_token=False, offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0,
        perturbation_noise_magnitude=0.0, image_area_root=[512], minimum_axis_length=[512], beta_scheduler=case["sched"],
        prediction_type="epsilon", excluded_layer_pattern_from_weight_decay=["bias", "scale", "embedding"],
        excluded_layer_from_quantization=["bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj"],
        quant_block_size=16, quantize_unet_state=True, quantize_text_encoder_state=True,
        accumulate_unet_ema=ema, accumulate_text_encoder_ema=ema, ema_rate=0.999)
    cfg = dict(unet=lora.LoraConfig(RANK, ALPHA, seed=1, dora=dora),
               text_encoder=lora.LoraConfig(RANK, ALPHA, targets=lora.CLIP_TARGETS, seed=2, dora=dora) if te == "dora" else "frozen")
    return tc, tu.on_device_model_training_state(tc, tl._models(case), device=dev, lora=cfg)


def _random_leaves(ad, weights, seed, rel=0.1):
    """{adapter path: tensor}: tl._random_factors' A and B, and m = the column norm of v times (1 + 0.1 * normal)."""
    tree = tl._random_factors(_Pairs(ad), weights, seed, rel)
    g = torch.Generator().manual_seed(seed + 1000)
    for p in ad.paths:
        a, b, m = ad.adapted[p]
        _, c, _ = dr.column_stats(lr.merge_ref64(weights[p], tree[a], tree[b], ad.cfg.scale))
        tree[m] = c * (1 + 0.1 * torch.randn(c.numel(), generator=g))
    return tree


class _Pairs:
    """An adapter as the LoRA file's helpers see it: adapted[p] = (lora_a, lora_b)."""

    def __init__(self, ad):
        self.paths, self.cfg, self.adapted = ad.paths, ad.cfg, {p: ad.adapted[p][:2] for p in ad.paths}


def _stats(ad, weights, leaves, p):
    a, b, m = ad.adapted[p]
    return dr.column_stats(lr.merge_ref64(weights[p], leaves[a], leaves[b], ad.cfg.scale), leaves[m])


def _folded64(ad, weights, leaves):
    """The fp32 tree the oracle runs on: (W0 + s * bf16(A) @ bf16(B)) * g, g = fl32(m / c) (float64 reference)."""
    out = dict(weights)
    for p in ad.paths:
        a, b, m = ad.adapted[p]
        _, c, g = _stats(ad, weights, leaves, p)
        out[p] = dr.merge_ref64(weights[p], leaves[a], leaves[b], ad.cfg.scale, g).float()
    return out


def _project_tree(ad, grads, weights, leaves):
    """The oracle's kernel gradients pushed through the float64 reference: dA, dB and dm with the norm held constant."""
    out = {}
    for p in ad.paths:
        a, b, m = ad.adapted[p]
        _, c, g = _stats(ad, weights, leaves, p)
        dA, dB, dm, _ = dr.project_ref64(torch.as_tensor(grads[p]), weights[p], leaves[a], leaves[b], ad.cfg.scale, c, g)
        out[a], out[b], out[m] = dA.float(), dB.float(), dm.float()
    return out


def _load_random(st, case, seed):
    out = []
    for state, s, weights in ((st[0], seed, case["weights"]["unet"]), (st[1], seed + 1, case["weights"]["clip"])):
        if state.adapter is None:
            out.append(None)
            continue
        leaves = _random_leaves(state.adapter, weights, s)
        state.adapter.store.load(leaves)
        out.append(leaves)
    return out


# ------------------------------------------------------------------------------------------------ 1
def test_a_fresh_adapter_leaves_the_mirror_of_the_frozen_base(dev):
    """B = 0 and m initialised by the merge's own reduction: g == 1.0f, so the merged mirror is the frozen store's prepared mirror
    bit for bit - for the UNet and the text encoder - and the step's prediction is the full fine-tune state's."""
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.params import ParamStore
    from tests.helpers import build_hip_states
    case = make_case("tiny", B=2, image=64)
    tc, st = _dora_states(case, dev)
    for state, spec, weights in ((st[0], nets.unet_spec(case["cfgs"]["unet"]), case["weights"]["unet"]),
                                 (st[1], nets.clip_text_spec(case["cfgs"]["clip"]), case["weights"]["clip"])):
        plain = ParamStore(spec, device=dev, trainable=False)
        plain.load(weights)
        plain.prepare(full=True)
        state.store.prepare()
        torch.cuda.synchronize()
        ad = state.adapter
        assert ad.cfg.dora and all(len(ad.adapted[p]) == 3 for p in ad.paths)
        assert torch.equal(state.store.w.view(torch.int16), plain.w.view(torch.int16)), "a fresh DoRA adapter changed the mirror"
        for i, p in enumerate(ad.paths):
            N, so = ad.jobs_host[i].N, ad.dora_host[i].stat_off
            assert torch.equal(ad.stats[so + N: so + 2 * N], torch.ones(N, device=dev)), f"{p}: g != 1.0f"
            assert torch.equal(ad.stats[so: so + N], ad.store.p(ad.adapted[p][2])), f"{p}: m is not the published c"
    preds = []
    for states in (build_hip_states(case, dev)[1], st):
        aux = {}
        out = tl._step(tu, states, case, dev, aux=aux)
        assert np.isfinite(out[4]["loss"].item())
        preds.append(aux["pred"].clone())
    assert torch.equal(preds[0], preds[1])


def test_a_fresh_adapter_with_an_ema_merges_the_base_from_the_ema_too(dev):
    """The init writes m into the EMA as well as into the master: on a fresh adapter that keeps an EMA, merge('ema') and
    folded(source='ema') give the frozen base, bit for bit - not kernels with a gain near zero."""
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.params import ParamStore
    case = make_case("tiny", B=2, image=64)
    tc, st = _dora_states(case, dev, ema=True)
    for state, spec, weights in ((st[0], nets.unet_spec(case["cfgs"]["unet"]), case["weights"]["unet"]),
                                 (st[1], nets.clip_text_spec(case["cfgs"]["clip"]), case["weights"]["clip"])):
        plain = ParamStore(spec, device=dev, trainable=False)
        plain.load(weights)
        plain.prepare(full=True)
        ad = state.adapter
        assert ad.store.ema is not None
        for p in ad.paths:
            lm = ad.store.leaves[ad.adapted[p][2]]
            m = ad.store.master[lm.offset: lm.offset + lm.numel]
            assert float(m.min()) > 0 and torch.equal(ad.store.ema[lm.offset: lm.offset + lm.numel], m), f"{p}: the EMA's m is not the master's"
        state.store.w.zero_()
        state.store.prepare()
        ad.merge("ema")
        torch.cuda.synchronize()
        assert torch.equal(state.store.w.view(torch.int16), plain.w.view(torch.int16)), "merge('ema') of a fresh adapter is not the base's mirror"
        N = ad.jobs_host[0].N
        assert torch.equal(ad.stats[ad.dora_host[0].stat_off + N: ad.dora_host[0].stat_off + 2 * N], torch.ones(N, device=dev))
        folded = ad.folded(source="ema")
        for p in ad.paths:
            assert torch.equal(folded[p], state.store.p(p)), f"{p}: folded(source='ema') of a fresh adapter is not W0"


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("te", ["dora", "frozen"])
def test_adapter_gradients_match_the_oracle_gradients_pushed_through_the_reference(dev, te):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _dora_states(case, dev, te=te)
    us, ts = st[0], st[1]
    fu, ft = _load_random(st, case, 11)
    unet_w = _folded64(us.adapter, case["weights"]["unet"], fu)
    clip_w = case["weights"]["clip"] if ft is None else _folded64(ts.adapter, case["weights"]["clip"], ft)
    ref = tl._oracle(case, unet_w, clip_w)
    out = tl._step(tu, st, case, dev)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    want = _project_tree(us.adapter, ref["unet_grads"], case["weights"]["unet"], fu)
    g = tl._gates(us.adapter.store, want, f"unet DoRA adapters, text encoder {te}")
    ms = [us.adapter.adapted[p][2] for p in us.adapter.paths]
    flat, rflat = torch.cat([g[q].flatten().cpu() for q in ms]), torch.cat([want[q].flatten() for q in ms])
    cos = float(torch.dot(flat, rflat) / (flat.norm() * rflat.norm()))
    print(f"lora_m alone: cosine {cos:.5f}, |dm| {float(flat.norm()):.4e} vs {float(rflat.norm()):.4e}")
    assert cos > 0.995 and float(rflat.norm()) > 0, "the magnitude gradients alone miss the gate of the whole store"
    if ft is not None:
        tl._gates(ts.adapter.store, _project_tree(ts.adapter, ref["te_grads"], case["weights"]["clip"], ft), "text-encoder DoRA adapters")
    assert us.step == 1 and us.store.count == 0


# ------------------------------------------------------------------------------------------------ 3
def test_one_step_moves_factors_and_magnitude_and_leaves_the_base(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _dora_states(case, dev, ema=True)
    _load_random(st, case, 21)
    before = [dict(master=s.store.master.clone(), w=s.store.w.clone(), folded=s.adapter.folded(), amaster=s.adapter.store.master.clone())
              for s in st[:2]]
    seen = {}
    for state in st[:2]:
        def note(path, store=state.adapter.store, real=state.adapter.store.note_written):
            seen.setdefault(id(store), []).append(path)
            real(path)
        state.adapter.store.note_written = note
    tl._step(tu, st, case, dev, ema_rate=0.999)
    torch.cuda.synchronize()
    for state, b in zip(st[:2], before):
        base, ad = state.store, state.adapter
        assert torch.equal(base.master, b["master"]), "the frozen master moved"
        got = seen[id(ad.store)]
        assert sorted(got) == sorted(ad.store.order) and len(set(got)) == len(got), "every adapter leaf is reported written once"
        adapted = torch.zeros(base.w.numel(), dtype=torch.bool, device=dev)
        for p in ad.paths:
            lf = base.leaves[p]
            adapted[lf.w_off: lf.w_off + lf.numel] = True
            assert torch.equal(base.w[lf.w_off: lf.w_off + lf.numel].view(lf.shape), b["folded"][p].to(torch.bfloat16)), p
            a, bb, m = ad.adapted[p]
            for q in (a, bb, m):
                lq = ad.store.leaves[q]
                assert not torch.equal(ad.store.master[lq.offset: lq.offset + lq.numel], b["amaster"][lq.offset: lq.offset + lq.numel]), f"{q} did not move"
            lm = ad.store.leaves[m]
            assert not lm.quantised and not lm.decayed
            # Lion without weight decay on a magnitude: every element with a gradient moves by exactly lr
            lr_ = state.hyper["lr"]
            p0 = b["amaster"][lm.offset: lm.offset + lm.numel].double()
            p1, gm = ad.store.p(m).double(), ad.store.grad_flat()[lm.offset: lm.offset + lm.numel]
            nz = gm != 0
            ulp = torch.nextafter(p0.float().abs(), torch.full_like(p0.float(), float("inf"))).double() - p0.abs()
            assert bool((((p0 - p1)[nz] - lr_ * torch.sign(gm.double())[nz]).abs() <= 2 * ulp[nz]).all()), m
        assert torch.equal(base.w[~adapted], b["w"][~adapted]), "the mirror of a non-adapted leaf was rewritten"
        assert state.step == 1


# ------------------------------------------------------------------------------------------------ 4
_RUNS = {}


def _trajectory(dev, use_graph):
    """Four steps through dp_compile_all_unique_resolution with explicit draws; per step the adapter stores' state."""
    if use_graph in _RUNS:
        return _RUNS[use_graph]
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, (us, ts, ue, te, vae, sc, _) = _dora_states(case, dev, ema=True)
    _load_random((us, ts), case, 31)
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
        snap = {"loss": out[4]["loss"].clone(), "unet.stats": us.adapter.stats.clone()}
        for name, state in (("unet", us), ("text", ts)):
            for b in STATE:
                snap[f"{name}.{b}"] = getattr(state.adapter.store, b).clone()
        trace.append(snap)
    if use_graph:
        assert fn.graph is not None and fn.calls == 2
    assert us.step == 4 and ts.step == 4
    _RUNS[use_graph] = trace
    return trace


def test_captured_steps_equal_eager_steps(dev):
    eager, graph = _trajectory(dev, False), _trajectory(dev, True)
    assert len({float(s["loss"]) for s in graph}) == 4
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager step at step {step}, {k}"
    assert not torch.equal(eager[0]["unet.master"], eager[3]["unet.master"])
    assert not torch.equal(eager[0]["unet.stats"], eager[3]["unet.stats"]), "the column statistics never followed the factors"


# ------------------------------------------------------------------------------------------------ 5
def test_micro_batches_match_the_full_batch_oracle_step(dev):
    """micro_batches=2 on B = 4 against the oracle's one step over all four samples, text encoder frozen: test_gpu_lora's comparison."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    tc, st = _dora_states(case, dev, te="frozen")
    us = st[0]
    fu, _ = _load_random(st, case, 41)
    ref = tl._oracle(case, _folded64(us.adapter, case["weights"]["unet"], fu), case["weights"]["clip"])
    out = tl._step(tu, st, case, dev, micro_batches=2)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    assert us.adapter.store.gacc is not None
    tl._gates(us.adapter.store, _project_tree(us.adapter, ref["unet_grads"], case["weights"]["unet"], fu), "K=2 accumulated unet DoRA adapters")


# ------------------------------------------------------------------------------------------------ 6
def test_adapter_file_and_training_state_resume_are_bitwise(dev, tmp_path):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    path, apath = str(tmp_path / "state.safetensors"), str(tmp_path / "adapter.npz")

    def fresh(seed):
        tc, st = _dora_states(case, dev, ema=True)
        _load_random(st, case, seed)
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
    st[0].adapter.save(apath)
    st[0].adapter.merge("master")  # the mirror of the saved leaves (the step's own merge ran before its optimizer step)
    w_saved = st[0].store.w.clone()
    a = two_steps(st, gen)
    st2, gen2 = fresh(61), torch.Generator(device=dev)  # other leaves: everything must come from the files
    st2[0].adapter.load(apath)  # (loads and merges)
    torch.cuda.synchronize()
    assert torch.equal(st2[0].store.w, w_saved), "an adapter file does not restore the merged mirror bit for bit"
    tu.load_training_state(path, st2[0], st2[1], train_rng=gen2)
    assert st2[0].step == 1 and st2[1].step == 1
    b = two_steps(st2, gen2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a training state of LoRA adapters is refused by DoRA states, and the adapter files are told apart
    tc, lst = _dora_states(case, dev, ema=True, dora=False)
    with pytest.raises(ValueError, match="LoRA settings"):
        tu.load_training_state(path, lst[0], lst[1], train_rng=gen2)
    with pytest.raises(ValueError, match="a DoRA adapter file, this adapter is a LoRA adapter"):
        lst[0].adapter.load(apath)
    lpath = str(tmp_path / "lora.npz")
    lst[0].adapter.save(lpath)
    with pytest.raises(ValueError, match="a LoRA adapter file, this adapter is a DoRA adapter"):
        st2[0].adapter.load(lpath)


# ------------------------------------------------------------------------------------------------ 7
def test_folded_checkpoint_rounds_to_the_mirror_and_samples_the_same(dev):
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.params import ParamStore
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = make_case("tiny", B=2, image=64)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    tc, st = _dora_states(case, dev, ema=True)
    us, ts = st[0], st[1]
    for state, seed, weights in ((us, 71, case["weights"]["unet"]), (ts, 72, case["weights"]["clip"])):
        state.adapter.store.load(_random_leaves(state.adapter, weights, seed, rel=0.3))
        state.adapter.store.ema.mul_(0.5)  # an EMA that differs from the master
        state.store.prepare()
        stats = state.adapter.stats.clone()
        folded = state.adapter.folded()
        for p in state.adapter.paths:  # the bf16 rounding of the folded checkpoint is the mirror
            lf = state.store.leaves[p]
            assert torch.equal(state.store.w[lf.w_off: lf.w_off + lf.numel].view(lf.shape), folded[p].to(torch.bfloat16)), p
        state.adapter.folded(source="ema")
        assert torch.equal(state.adapter.stats, stats), "folding a checkpoint moved the statistics the projection reads"
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
    assert not torch.equal(with_adapter, generate(*plain(case["weights"]["unet"], case["weights"]["clip"])))
    assert torch.equal(with_adapter, generate(*plain(us.adapter.folded(), ts.adapter.folded())))
    us.adapter.merge(source="ema")
    ts.adapter.merge(source="ema")
    ema_img = generate(us, ts)
    assert not torch.equal(ema_img, with_adapter)
    assert torch.equal(ema_img, generate(*plain(us.adapter.folded(source="ema"), ts.adapter.folded(source="ema"))))
