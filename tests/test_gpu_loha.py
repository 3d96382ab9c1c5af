"""LoHa training on the MI355X at model level (LoraConfig(algo="loha"); DESIGN.md "LoHa"), on the tiny configuration: rank 4 on the
attention projections and conv rank 4 on every conv target, four trained leaves per adapted kernel.  Fixtures, oracle and gates are those of
tests/test_gpu_lora.py and tests/test_gpu_locon.py (imported, not restated): the oracle runs on fp32 trees with the adapters folded in by
the float64 reference (tests/loha_reference.py) and its weight gradients are projected by the float64 reference.

The gradient comparisons load random factors with all four leaves away from zero instead of first taking steps from the initialisation:
a few steps at the test's learning rate leave B2 near 1e-6, where dA1, dB1 and dA2 are a millionth of dB2 and fall under the worst-leaf
gate's floor - the loaded factors put every one of the four gradients among the checked leaves."""
import hashlib

import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import loha_reference as lh
from tests import test_gpu_locon as tlc  # its builders (nothing of it is collected from here)
from tests import test_gpu_lora as tl
from tests.helpers import build_hip_states, make_case, to_dev

pytestmark = pytest.mark.gpu
RANK, ALPHA, CONV_RANK, CONV_ALPHA = 4, 2.0, 4, 2.0
STATE = tl.STATE
_mat, _scale, _conv_kinds = tlc._mat, tlc._scale, tlc._conv_kinds


def _loha_states(case, dev, te="loha", ema=False, conv_alpha=CONV_ALPHA, alpha=ALPHA):
    """(tc, states) as tests/test_gpu_locon._locon_states, the UNet (and with te="loha" the text encoder) under LoHa."""
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
    cfg = dict(unet=lora.LoraConfig(RANK, alpha, seed=1, conv_rank=CONV_RANK, conv_alpha=conv_alpha, algo="loha"),
               text_encoder=lora.LoraConfig(RANK, alpha, targets=lora.CLIP_TARGETS, seed=2, algo="loha") if te == "loha" else "frozen")
    return tc, tu.on_device_model_training_state(tc, tl._models(case), device=dev, lora=cfg)


def _random_factors(ad, weights, seed, rel=0.1):
    """Four random factors per adapted kernel, the delta s * (A1 B1) * (A2 B2) `rel` of its base kernel's norm."""
    g = torch.Generator().manual_seed(seed)
    tree = {}
    for p in ad.paths:
        names = ad.adapted[p]
        (K, r), N = ad.store.leaves[names[0]].shape, ad.store.leaves[names[1]].shape[1]
        f = [torch.randn(K, r, generator=g), torch.randn(r, N, generator=g), torch.randn(K, r, generator=g), torch.randn(r, N, generator=g)]
        delta = lh.merge_ref64(torch.zeros(K, N), *f, _scale(ad, p))
        c = (rel * float(torch.as_tensor(weights[p]).double().norm()) / float(delta.norm())) ** 0.25
        tree.update({n: x * c for n, x in zip(names, f)})
    return tree


def _folded64(ad, weights, factors):
    out = dict(weights)
    for p in ad.paths:
        out[p] = lh.merge_ref64(_mat(weights[p]), *(factors[n] for n in ad.adapted[p]), _scale(ad, p)).float().view(weights[p].shape)
    return out


def _project_tree(ad, grads, factors):
    out = {}
    for p in ad.paths:
        got = lh.project_ref64(_mat(grads[p]), *(factors[n] for n in ad.adapted[p]), _scale(ad, p))
        out.update({n: g.float() for n, g in zip(ad.adapted[p], got)})
    return out


def _load_both(st, case, seed, rel=0.1):
    fu = _random_factors(st[0].adapter, case["weights"]["unet"], seed, rel)
    st[0].adapter.store.load(fu)
    ft = None
    if st[1].adapter is not None:
        ft = _random_factors(st[1].adapter, case["weights"]["clip"], seed + 1, rel)
        st[1].adapter.store.load(ft)
    return fu, ft


def _mirror(base, p):
    lf = base.leaves[p]
    return base.w[lf.w_off: lf.w_off + lf.numel].view(lf.shape).cpu()


# ------------------------------------------------------------------------------------------------ 1
def test_first_step_mirror_equals_the_base(dev):
    """LyCORIS initialisation (B2 = 0): the merged mirror is bf16(W0) bit for bit in every adapted leaf, the first step predicts what the
    base predicts, and only the B2 leaves receive a gradient."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    preds = []
    for build in (lambda: build_hip_states(case, dev)[1], lambda: _loha_states(case, dev, te="frozen")[1]):
        st, aux = build(), {}
        out = tl._step(tu, st, case, dev, aux=aux)
        assert np.isfinite(out[4]["loss"].item())
        preds.append(aux["pred"].clone())
    ad = st[0].adapter
    assert ad.conv_paths and ad.dense_paths and len(ad.loha) == 2 and torch.equal(preds[0], preds[1])
    g = ad.store.export("grad")
    for p in ad.paths:
        kc.assert_equal_bits(_mirror(st[0].store, p), torch.as_tensor(case["weights"]["unet"][p]).float().to(torch.bfloat16), f"first mirror {p}")
        a1, b1, a2, b2 = ad.adapted[p]
        assert not bool(g[a1].any()) and not bool(g[b1].any()) and not bool(g[a2].any()) and float(g[b2].abs().max()) > 0, p


# ------------------------------------------------------------------------------------------------ 2
def test_adapter_gradients_match_the_projected_oracle_gradients(dev):
    """tl._gates over Dense and convolution LoHa adapters.  A Dense leaf, a 1x1, a 3x3 and the stride-2 downsampler's leaves must be among
    the leaves the worst-leaf gate checks, and the tallest convolution takes more than one chunk."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _loha_states(case, dev, te="frozen")
    us = st[0]
    ad = us.adapter
    kinds = dict(_conv_kinds(ad), dense=ad.dense_paths)
    assert all(kinds.values()), {k: len(v) for k, v in kinds.items()}
    assert max(j.K for j in ad.conv_jobs_host) == 9 * 128 and max(x.chunks for t in ad.loha for x in t[2]) > 1
    fu, _ = _load_both(st, case, 11)
    ref = tl._oracle(case, _folded64(ad, case["weights"]["unet"], fu), case["weights"]["clip"])
    out = tl._step(tu, st, case, dev)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    want = _project_tree(ad, ref["unet_grads"], fu)
    total = torch.cat([v.flatten() for v in want.values()]).norm()
    checked = {k for k, v in want.items() if v.norm() > 1e-3 * total}  # the leaves tl._gates' worst-leaf gate looks at
    for kind, paths in kinds.items():
        hit = [q for p in paths for q in ad.adapted[p] if q in checked]
        print(f"{kind}: {len(hit)} of {4 * len(paths)} adapter leaves among the checked leaves")
        assert hit, f"no {kind} adapter is among the checked leaves"
    for side in ("loha_a1", "loha_b1", "loha_a2", "loha_b2"):
        assert any(q.endswith(side) for q in checked), f"no {side} leaf is among the checked leaves"
    g = tl._gates(ad.store, want, "unet LoHa adapters, text encoder frozen")
    for p in ad.paths:
        for q in ad.adapted[p]:
            assert float(g[q].abs().max()) > 0, f"{q}: no gradient"
    assert us.step == 1 and us.store.count == 0


# ------------------------------------------------------------------------------------------------ 3, 4
_RUNS = {}


def _trajectory(dev, use_graph, fresh=False):
    """tests/test_gpu_locon._trajectory on LoHa states (UNet and text encoder)."""
    key = ("traj", use_graph)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    tc, st = _loha_states(case, dev, ema=True)
    us, ts, ue, te, vae, sc, _ = st
    _load_both(st, case, 31)
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
        snap = {"loss": out[4]["loss"].clone(), "unet.grad": us.adapter.store.grad.clone(), "text.grad": ts.adapter.store.grad.clone()}
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


# ------------------------------------------------------------------------------------------------ 5
def test_micro_batches_match_the_full_batch_oracle_step(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    tc, st = _loha_states(case, dev, te="frozen")
    us = st[0]
    fu, _ = _load_both(st, case, 41)
    ref = tl._oracle(case, _folded64(us.adapter, case["weights"]["unet"], fu), case["weights"]["clip"])
    out = tl._step(tu, st, case, dev, micro_batches=2)
    assert abs(out[4]["loss"].item() - ref["loss"]) / ref["loss"] < 1e-2
    assert us.adapter.store.gacc is not None
    tl._gates(us.adapter.store, _project_tree(us.adapter, ref["unet_grads"], fu), "K=2 accumulated unet LoHa adapters")


# ------------------------------------------------------------------------------------------------ 6
def test_checkpoint_resume_is_bitwise(dev, tmp_path):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    path = str(tmp_path / "state.safetensors")

    def fresh(seed):
        tc, st = _loha_states(case, dev, ema=True)
        _load_both(st, case, seed)
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
    a = two_steps(st, gen)
    st2, gen2 = fresh(61), torch.Generator(device=dev)  # other factors: everything must come from the file
    tu.load_training_state(path, st2[0], st2[1], train_rng=gen2)
    assert st2[0].step == 1 and st2[1].step == 1
    b = two_steps(st2, gen2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the adapter file: LoHa round trip, and a LoRA adapter refuses it by name
    f = str(tmp_path / "adapter.npz")
    st[0].adapter.save(f)
    st2[0].adapter.store.load(_random_factors(st2[0].adapter, case["weights"]["unet"], 71))
    st2[0].adapter.load(f)  # (merges what it loaded; the first adapter's mirror still holds its last step's merge)
    st[0].adapter.merge()
    assert torch.equal(st2[0].adapter.store.master, st[0].adapter.store.master) and torch.equal(st2[0].store.w, st[0].store.w)
    _, plain = tlc._locon_states(case, dev, te="frozen")
    with pytest.raises(ValueError, match="a LoHa adapter file, this adapter is a LoRA adapter"):
        plain[0].adapter.load(f)


# ------------------------------------------------------------------------------------------------ 7
def test_sampling_uses_the_adapter_and_equals_the_folded_checkpoint(dev):
    from oracle import nets as onets
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd.params import ParamStore
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    case = make_case("tiny", B=2, image=64)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    tc, st = _loha_states(case, dev, te="frozen")
    us, ts = st[0], st[1]
    _load_both(st, case, 71, rel=0.3)
    ids = case["batch"]["input_ids"].to(dev)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)

    def generate(unet, text):
        pipe = StableDiffusionPipeline(unet, text, vae_w, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], device=dev)
        return pipe.generate(ids, num_inference_steps=2, height=64, width=64, latents=lat)

    def plain(unet_tree):
        u = ParamStore(nets.unet_spec(case["cfgs"]["unet"]), device=dev, trainable=False)
        u.load(unet_tree)
        return u

    with_adapter = generate(us, ts.store)
    assert not torch.equal(with_adapter, generate(plain(case["weights"]["unet"]), ts.store))
    folded = us.adapter.folded()
    assert torch.equal(with_adapter, generate(plain(folded), ts.store))
    for p, w in case["weights"]["unet"].items():
        same = torch.equal(folded[p].cpu(), torch.as_tensor(w).float())
        assert same != (p in us.adapter.paths), p


# ------------------------------------------------------------------------------------------------ 8
def _exact_factors(ad, seed):
    """Integers in -3..3 over 8 in all four factors: P_i is a multiple of 1/64 below 1, P1 * P2 a multiple of 1/4096 with at most 11
    significant bits - exact in fp32 - so v = fl32(W0 + P1 * P2) carries the one rounding of the sum and the mirror is RNE_bf16(v)."""
    tree = {}
    for i, p in enumerate(ad.paths):
        for t, n in enumerate(ad.adapted[p]):
            tree[n] = kc.exact_ints(ad.store.leaves[n].shape, -3, 3, seed + 4 * i + t, dtype=torch.float32) / 8
    return tree


def test_dpo_step_restores_and_merges(dev):
    """One Diffusion-DPO step on LoHa states (scale 1).  restore(): every adapted leaf of the mirror is bf16(W0) bit for bit; after the
    step the mirror holds the step's merge, RNE_bf16 of fl32(merge_ref64)."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests import test_gpu_dpo as tdpo
    case = make_case("tiny", B=4, image=64)
    tc, st = _loha_states(case, dev, te="frozen", alpha=float(RANK), conv_alpha=None)
    us = st[0]
    ad, base, W = us.adapter, us.store, case["weights"]["unet"]
    assert ad.cfg.scale == 1.0 and ad.cfg.conv_scale == 1.0 and ad.conv_paths
    factors = _exact_factors(ad, 81)
    ad.store.load(factors)
    merged = {p: kc.rne_bf16(lh.merge_ref64(_mat(W[p]), *(factors[n] for n in ad.adapted[p]), 1.0).float().double()).view(W[p].shape)
              for p in ad.paths}
    w_before = base.w.clone()
    ad.restore()
    torch.cuda.synchronize()
    for p in ad.paths:
        kc.assert_equal_bits(_mirror(base, p), torch.as_tensor(W[p]).float().to(torch.bfloat16), f"restored {p}")
        assert not torch.equal(kc.bits(_mirror(base, p)), kc.bits(merged[p])), f"{p}: the adapter leaves the mirror where the base has it"
    out = tdpo._step(tu, st, to_dev(case["batch"], dev), dev, rand=tdpo.pair_rand(case), dpo_beta=tdpo.BETA)
    assert np.isfinite(out[4]["loss"].item()) and set(out[4]) >= {"loss", "implicit_acc", "model_mse", "ref_mse"}
    assert not torch.equal(kc.bits(out[4]["model_mse"]), kc.bits(out[4]["ref_mse"])), "the reference pass saw the adapter"
    for p in ad.paths:
        kc.assert_equal_bits(_mirror(base, p), merged[p], f"merged {p}")
    adapted = torch.zeros(base.w.numel(), dtype=torch.bool, device=dev)
    for p in ad.paths:
        lf = base.leaves[p]
        adapted[lf.w_off: lf.w_off + lf.numel] = True
    assert torch.equal(base.w[~adapted], w_before[~adapted]), "the mirror of a non-adapted leaf was rewritten"
    g = ad.store.export("grad")
    assert all(float(g[q].abs().max()) > 0 and bool(torch.isfinite(g[q]).all()) for p in ad.paths for q in ad.adapted[p])


# ------------------------------------------------------------------------------------------------ 9
def test_sd15_structure_one_step(dev):
    """SD1.5 at tests/test_gpu_locon.test_sd15_structure_one_step's input size (B=2, image 64), one eager LoHa step (K up to 9 * 2560: 45
    chunks): finite loss, every adapter leaf reported written exactly once with a finite non-zero gradient, no leaf of the frozen base
    written, every adapted leaf of the mirror merged (it differs from bf16(W0))."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("sd15", B=2, image=64)
    tc, st = _loha_states(case, dev, te="frozen")
    us = st[0]
    ad = us.adapter
    assert max(j.K for j in ad.conv_jobs_host) == 9 * 2560 and any(len(us.store.leaves[p].shape) == 4 and "/proj_in/" in p for p in ad.conv_paths)
    tree = {k: v.cpu() for k, v in ad.store.export().items()}
    g = torch.Generator().manual_seed(91)
    for p in ad.paths:  # B2 away from zero, so that a merged leaf differs from its base and every factor has a gradient
        b2 = ad.adapted[p][3]
        tree[b2] = 0.005 * torch.randn(tree[b2].shape, generator=g)
    ad.store.load(tree)
    seen = {}
    for store in (us.store, ad.store):
        def note(path, store=store, real=store.note_written):
            seen.setdefault(id(store), []).append(path)
            real(path)
        store.note_written = note
    out = tl._step(tu, st, case, dev)
    assert np.isfinite(out[4]["loss"].item())
    assert id(us.store) not in seen, "a gradient leaf of a frozen base was written"
    got = seen[id(ad.store)]
    assert sorted(got) == sorted(ad.store.order) and len(set(got)) == len(got)
    assert bool(torch.isfinite(ad.store.grad_flat()).all())
    gb = ad.store.export("grad")
    assert all(float(gb[q].abs().max()) > 0 for p in ad.paths for q in ad.adapted[p]), "an adapter leaf received no gradient"
    for p in ad.paths:
        lf = us.store.leaves[p]
        w = us.store.w[lf.w_off: lf.w_off + lf.numel]
        w0 = us.store.master[lf.offset: lf.offset + lf.numel].to(torch.bfloat16)
        assert not torch.equal(w, w0), f"{p}: the mirror still holds bf16(W0)"
