"""Diffusion-DPO steps on the MI355X (train_step dpo_beta=; include/sdt.h "DPO LOSS"), on the tiny model with 2 pairs: the frozen base
under a LoRA / DoRA adapter is the reference model.  Kernel-level checks: tests/test_gpu_dpo_kernels.py; the float64 reference and the
chains between the published values: tests/dpo_reference.py."""
import math

import numpy as np
import pytest
import torch

from tests import dpo_reference as dref
from tests import kernel_checks as kc
from tests import test_gpu_dora as td  # its builders: _dora_states, _random_leaves (nothing of it is collected from here)
from tests import test_gpu_lora as tl
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
STATE = ("master", "codes", "inv_scale", "mom", "ema")
BETA = 5000.0  # diffusers' value for SD1.5 / SDXL


def dpo_states(case, dev, dora=False, ema=False, prediction_type="epsilon"):
    """tests/test_gpu_lora.py's _lora_states with te="frozen" (DoRA: tests/test_gpu_dora.py's _dora_states): (tc, states)."""
    if dora:
        assert prediction_type == "epsilon"
        return td._dora_states(case, dev, te="frozen", ema=ema)
    return tl._lora_states(case, dev, te="frozen", ema=ema, prediction_type=prediction_type)


def random_factors(ad, weights, seed, rel=0.1):
    """Random A and B at relative size `rel` of the base kernel (tl._random_factors); DoRA: and m around the column norms."""
    return td._random_leaves(ad, weights, seed, rel) if ad.cfg.dora else tl._random_factors(ad, weights, seed, rel)


def pair_rand(case, offset=False, seed=3):
    """The case's draws at DPO sizes: posterior_eps per sample (N), noise / timesteps (/ offset_noise) per pair (P = N / 2)."""
    r = case["rand"]
    P = r["noise"].shape[0] // 2
    out = dict(posterior_eps=r["posterior_eps"], noise=r["noise"][:P].clone(), timesteps=r["timesteps"][:P].clone())
    if offset:
        out["offset_noise"] = torch.randn(P, 4, 1, 1, generator=torch.Generator().manual_seed(seed))
    return out


def expanded(rand):
    """The per-sample draws a plain step needs to see what the DPO step's pairs saw."""
    return {k: (v if k == "posterior_eps" else v.repeat_interleave(2, 0)) for k, v in rand.items()}


def _step(tu, st, batch, dev, rand=None, gen=None, **kw):
    us, ts, ue, te, vae, sc, _ = st
    gen = gen if gen is not None else torch.Generator(device=dev)
    out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, rand=None if rand is None else to_dev(rand, dev), **kw)
    torch.cuda.synchronize()
    return out


def _snapshot(us, out=None):
    st = us.opt_store
    snap = {b: getattr(st, b).clone() for b in STATE if getattr(st, b, None) is not None}
    snap["sqnorm"] = st.sqnorm.clone()
    if out is not None:
        snap.update({k: v.clone() for k, v in out[4].items()})
    return snap


def _assert_same(a, b, what, skip=()):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        if k not in skip:
            assert a[k].shape == b[k].shape and torch.equal(kc.bits(a[k]), kc.bits(b[k])), \
                f"{what}: {k} differs ({(a[k].double() - b[k].double()).abs().max().item():.3e} max abs)"


def _adapted_bits(us):
    base = us.store
    return torch.cat([kc.bits(base.w[base.leaves[p].w_off: base.leaves[p].w_off + base.leaves[p].numel]) for p in us.adapter.paths])


LN2 = float(np.float32(math.log(2.0)))


# ------------------------------------------------------------------------------------------------ 1
def test_fresh_adapter_sits_on_the_reference(dev):
    """B = 0: the merged mirror is the base's, so both passes are one function: loss == float32(ln 2) exactly, every logit 0,
    implicit_acc 0, model_mse == ref_mse bit for bit - and the adapter's B factors still move (coef = -+beta/2)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    st = dpo_states(case, dev)[1]
    ad = st[0].adapter
    before = ad.store.export()
    out = _step(tu, st, to_dev(case["batch"], dev), dev, rand=pair_rand(case), dpo_beta=BETA)
    m = out[4]
    assert set(m) == {"loss", "implicit_acc", "dpo_logits", "model_mse", "ref_mse"}
    assert m["loss"].item() == LN2 and m["implicit_acc"].item() == 0
    assert m["dpo_logits"].shape == (2,) and not m["dpo_logits"].abs().sum()
    assert m["model_mse"].shape == (4,) and torch.equal(kc.bits(m["model_mse"]), kc.bits(m["ref_mse"])) and (m["model_mse"] > 0).all()
    after = ad.store.export()
    moved = [p for p in ad.paths if not torch.equal(after[ad.adapted[p][1]], before[ad.adapted[p][1]])]
    assert len(moved) == len(ad.paths), f"only {len(moved)} of {len(ad.paths)} B factors moved"


# ------------------------------------------------------------------------------------------------ 2
def test_reference_pass_is_the_base_and_the_loss_follows_the_reference(dev):
    """Random factors.  aux["ref_pred"] equals, bit for bit, the pred of an adapter-less state built from the same weights and draws;
    pred differs from it; metrics, loss and aux["dpred"] follow tests/dpo_reference.py from the aux taps under the kernel-level rules:
    logits bit for bit from the published errors, pair_loss / coef within 1 fp32 ulp, dpred bit for bit from the published coef, the
    loss bit for bit from the published pair losses.  The published errors against float64 means of the taps: the fp32 sum of n = C*h*w
    non-negative terms of 2 roundings each, then 2 more: relative error <= (n + 3) u."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    rand, beta = pair_rand(case), 50.0
    plain_aux = {}
    _step(tu, build_hip_states(case, dev)[1], to_dev(case["batch"], dev), dev, rand=expanded(rand), aux=plain_aux)
    st = dpo_states(case, dev)[1]
    ad = st[0].adapter
    ad.store.load(random_factors(ad, case["weights"]["unet"], 11))
    aux = {}
    out = _step(tu, st, to_dev(case["batch"], dev), dev, rand=rand, aux=aux, dpo_beta=beta)
    assert torch.equal(kc.bits(aux["ref_pred"]), kc.bits(plain_aux["pred"])), "the reference pass is not the base model's"
    assert not torch.equal(kc.bits(aux["pred"]), kc.bits(aux["ref_pred"]))
    m = {k: v.cpu() for k, v in out[4].items()}
    C, n, U = 4, 4 * 8 * 8, 2.0 ** -24
    x, y, t = aux["pred"][..., :C].float().cpu().numpy(), aux["ref_pred"][..., :C].float().cpu().numpy(), aux["target"].cpu().numpy()
    ref = dref.reference(x, y, t, beta)
    for got, want, name in ((m["model_mse"], ref["model_mse"], "model_mse"), (m["ref_mse"], ref["ref_mse"], "ref_mse")):
        err = np.abs(got.double().numpy() - want) / want
        print(f"{name} {got.tolist()} float64 {want.tolist()} rel err {err.tolist()}")
        assert (err <= (n + 3) * U).all(), (name, err.tolist())
    pr = dref.pairs(m["model_mse"].numpy(), m["ref_mse"].numpy(), beta)
    kc.assert_equal_bits(m["dpo_logits"], torch.from_numpy(pr["logits"]), "dpo_logits from the published errors")
    assert m["implicit_acc"].item() == float((pr["logits"] > 0).mean())
    print(f"logits {m['dpo_logits'].tolist()} (float64 from the taps {ref['logits'].tolist()}), loss {m['loss'].item()!r} (float64 {ref['loss']!r})")
    assert (m["dpo_logits"] != 0).all() and (m["dpo_logits"].abs() < 30).all(), "the logits saturate: the gradient check would be empty"
    coef, pl = aux["dpo_coef"].cpu(), aux["dpo_pair_loss"].cpu()
    for got, want, name in ((pl, pr["pair_loss"], "pair_loss"), (coef, pr["coef"], "coef")):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.double().numpy() - want) <= ulp).all(), (name, got.tolist(), want.tolist())
    kc.assert_equal_bits(m["loss"].view(1), torch.tensor([dref.loss_chain(pl.numpy())]), "loss from the published pair losses")
    want_dp = torch.zeros_like(aux["dpred"].cpu())
    want_dp[..., :C] = dref.dpred_chain(coef.numpy(), x, t)
    kc.assert_equal_bits(aux["dpred"].cpu(), want_dp, "dpred [image][row][column][channel] from the published coef")
    assert aux["dpred"].float().abs().sum() > 0


# ------------------------------------------------------------------------------------------------ 3
def test_a_pair_shares_noise_and_timestep_and_the_generator_takes_pair_sized_draws(dev):
    """Images, captions and posterior draws equal inside each pair, noise and timesteps from train_rng: both samples of a pair are one
    input, so every logit is exactly 0 whatever the factors - unless the noise or the timestep differed inside a pair.  The generator
    ends where randn(P, L, h, w) (noise) and randint(P) (timesteps), in that order, leave it."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    batch = {k: v.clone() for k, v in case["batch"].items()}
    eps = case["rand"]["posterior_eps"].clone()
    for i in (0, 2):
        batch["pixel_values"][i + 1], batch["input_ids"][i + 1], eps[i + 1] = batch["pixel_values"][i], batch["input_ids"][i], eps[i]
    st = dpo_states(case, dev)[1]
    ad = st[0].adapter
    ad.store.load(random_factors(ad, case["weights"]["unet"], 12))
    gen, twin = torch.Generator(device=dev), torch.Generator(device=dev)
    gen.manual_seed(77), twin.manual_seed(77)
    out = _step(tu, st, to_dev(batch, dev), dev, rand=dict(posterior_eps=eps), gen=gen, dpo_beta=BETA)
    m = out[4]
    assert not m["dpo_logits"].abs().sum(), f"logits {m['dpo_logits'].tolist()}: a pair did not share its noise or its timestep"
    assert torch.equal(m["model_mse"][0::2], m["model_mse"][1::2]) and not torch.equal(m["model_mse"], m["ref_mse"])
    assert m["model_mse"][0] != m["model_mse"][2]
    torch.randn(2, 4, 8, 8, device=dev, generator=twin)
    torch.randint(0, 1000, (2,), device=dev, generator=twin)
    assert torch.equal(gen.get_state(), twin.get_state()), "the step did not take the documented draws from train_rng"


# ------------------------------------------------------------------------------------------------ 4
def test_captured_steps_equal_eager_steps(dev):
    """dp_compile_all_unique_resolution(step_overrides=dict(dpo_beta=...)): two eager warm-ups, the capture on the third call, two
    replays; every step's adapter state and metrics equal the eager run's bit for bit."""
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = make_case("tiny", B=4, image=64)
        tc, st = dpo_states(case, dev, ema=True)
        us, ts, ue, te, vae, sc, _ = st
        us.adapter.store.load(random_factors(us.adapter, case["weights"]["unet"], 13))
        tc.image_area_root, tc.minimum_axis_length = [64], [64]
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph, step_overrides=dict(dpo_beta=50.0))
        batch = to_dev(case["batch"], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        trace = []
        fn = table[tu.step_key(batch)]
        for step in range(5):
            out = fn(us, ts, ue, te, batch, gen, vae, sc)
            torch.cuda.synchronize()
            trace.append(_snapshot(us, out))
        if use_graph:
            assert fn.graph is not None and fn.calls == 2 and us.opt_store.count == 5
        return trace

    eager, graph = run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 5
    for step, (a, b) in enumerate(zip(eager, graph)):
        _assert_same(a, b, f"graph replay against the eager run at step {step}")


# ------------------------------------------------------------------------------------------------ 5
def test_cached_latents_give_every_bit_of_the_pixel_step(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    rand, snaps = pair_rand(case), []
    for cached in (False, True):
        st = dpo_states(case, dev, ema=True)[1]
        st[0].adapter.store.load(random_factors(st[0].adapter, case["weights"]["unet"], 14))
        batch = to_dev(case["batch"], dev)
        if cached:
            batch = {"latent_moments": tu.encode_latent_moments(st[4], batch["pixel_values"]), "input_ids": batch["input_ids"]}
        out = _step(tu, st, batch, dev, rand=rand, dpo_beta=50.0)
        snaps.append(_snapshot(st[0], out))
    _assert_same(snaps[0], snaps[1], "cached latents against the pixel step")


# ------------------------------------------------------------------------------------------------ 6
def test_identical_micro_batches_equal_the_plain_step_bit_for_bit(dev):
    """tests/test_gpu_grad_accum.py's exact rule: batch = b ++ b (b: one pair) with K = 2 accumulates g + g and scales by 1/2, exact in
    fp32, so everything the step writes equals the K = 1 step over b; the metrics are the micro-batches' concatenated."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    rand = pair_rand(case)
    snaps = []
    for K in (1, 2):
        st = dpo_states(case, dev, ema=True)[1]
        st[0].adapter.store.load(random_factors(st[0].adapter, case["weights"]["unet"], 15))
        batch, rnd = case["batch"], rand
        if K == 2:
            batch, rnd = {k: torch.cat([v, v]) for k, v in batch.items()}, {k: torch.cat([v, v]) for k, v in rand.items()}
        out = _step(tu, st, to_dev(batch, dev), dev, rand=rnd, dpo_beta=50.0, micro_batches=K, ema_rate=0.999)
        snaps.append(_snapshot(st[0], out))
    per_pair = ("dpo_logits", "model_mse", "ref_mse")
    for k in per_pair:
        assert torch.equal(snaps[1][k], torch.cat([snaps[0][k], snaps[0][k]])), f"{k}: not the micro-batches' concatenated"
    _assert_same(snaps[0], snaps[1], "K = 2 over b ++ b against K = 1 over b", skip=per_pair)


def test_micro_batches_match_the_full_batch_step(dev):
    """Two different pairs, K = 2 against K = 1 under the gates tests/test_gpu_grad_accum.py holds accumulated steps to: loss within
    1e-2, gradient norm within 3e-2, cosine > 0.995, worst leaf < 0.1.  (The loss is a mean over pairs and nothing mixes samples: the
    two steps differ by the order of fp32 sums and by the bf16 rounding of dpred's 1/P.)"""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    rand, grads, outs = pair_rand(case), [], []
    for K in (1, 2):
        st = dpo_states(case, dev)[1]
        st[0].adapter.store.load(random_factors(st[0].adapter, case["weights"]["unet"], 16))
        out = _step(tu, st, to_dev(case["batch"], dev), dev, rand=rand, dpo_beta=50.0, micro_batches=K)
        store = st[0].adapter.store
        grads.append(({k: v.cpu() for k, v in store.export("grad").items()}, store.grad_norm()))
        outs.append({k: v.cpu() for k, v in out[4].items()})
    (gref, nref), (g, n) = grads
    # the per-sample errors are losses and take the loss's gate; the logits are beta/2 times a difference of four errors that cancel
    # to about a hundredth of their size, so a relative gate on the errors says nothing relative about them: shape only
    assert outs[1]["dpo_logits"].shape == outs[0]["dpo_logits"].shape == (2,)
    print(f"logits K = 1 {outs[0]['dpo_logits'].tolist()}, K = 2 {outs[1]['dpo_logits'].tolist()}")
    for k in ("model_mse", "ref_mse"):
        assert outs[1][k].shape == outs[0][k].shape and torch.allclose(outs[1][k], outs[0][k], rtol=1e-2, atol=0), k
    assert abs(outs[1]["loss"].item() - outs[0]["loss"].item()) / outs[0]["loss"].item() < 1e-2
    assert nref > 0 and abs(n - nref) / nref < 3e-2, (n, nref)
    flat, rflat = torch.cat([g[k].flatten() for k in gref]), torch.cat([gref[k].flatten() for k in gref])
    cos = float(torch.dot(flat, rflat) / (flat.norm() * rflat.norm()))
    worst = max((rel_l2(g[k], gref[k]), k) for k in gref if gref[k].norm() > 1e-3 * rflat.norm())
    print(f"K = 2 against K = 1: cosine {cos:.6f}, worst leaf {worst}, |g| {n:.5e} vs {nref:.5e}")
    assert cos > 0.995 and worst[0] < 0.1, (cos, worst)


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("variant", ["dora", "v_prediction", "offset_noise"])
def test_variants_run_against_the_base(dev, variant):
    """One step each: finite, and the reference pass equals the adapter-less state's prediction bit for bit."""
    from stable_diffusion_training_amd import training_utils as tu
    vp, off = variant == "v_prediction", variant == "offset_noise"
    case = make_case("tiny", B=4, image=64, sched="zero_snr_scaled_linear" if vp else "scaled_linear")
    ptype = "v_prediction" if vp else "epsilon"
    rand = pair_rand(case, offset=off)
    kw = dict(offset_noise_magnitude=0.1) if off else {}
    plain_aux, aux = {}, {}
    _step(tu, build_hip_states(case, dev, prediction_type=ptype)[1], to_dev(case["batch"], dev), dev, rand=expanded(rand), aux=plain_aux, **kw)
    st = dpo_states(case, dev, dora=variant == "dora", prediction_type=ptype)[1]
    ad = st[0].adapter
    ad.store.load(random_factors(ad, case["weights"]["unet"], 17))
    before = ad.store.export()
    out = _step(tu, st, to_dev(case["batch"], dev), dev, rand=rand, aux=aux, dpo_beta=50.0, **kw)
    assert all(torch.isfinite(v.float()).all() for v in out[4].values())
    assert torch.equal(kc.bits(aux["ref_pred"]), kc.bits(plain_aux["pred"])), f"{variant}: the reference pass is not the base model's"
    assert torch.equal(kc.bits(aux["target"]), kc.bits(plain_aux["target"]))
    assert (out[4]["dpo_logits"] != 0).all()
    after = ad.store.export()
    assert any(not torch.equal(after[k], before[k]) for k in before) and all(torch.isfinite(v).all() for v in after.values())


# ------------------------------------------------------------------------------------------------ 8
def test_the_mirror_holds_the_merged_weights_after_a_step(dev):
    """As after a LoRA step, never the restored base: the adapted leaves equal what a merge of the factors the step STARTED from
    writes (the step merges before its taped forward and the optimizer moves only the adapter's master)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    st = dpo_states(case, dev)[1]
    ad = st[0].adapter
    ad.store.load(random_factors(ad, case["weights"]["unet"], 18))
    ad.merge("master")
    merged = _adapted_bits(st[0]).clone()
    ad.restore()
    base_bits = _adapted_bits(st[0]).clone()
    assert not torch.equal(merged, base_bits)
    _step(tu, st, to_dev(case["batch"], dev), dev, rand=pair_rand(case), dpo_beta=50.0)
    assert torch.equal(_adapted_bits(st[0]), merged), "the mirror does not hold the merged weights after the step"
    assert ad.source == "master"


# ------------------------------------------------------------------------------------------------ 9
def test_refusals(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    batch, rand = to_dev(case["batch"], dev), pair_rand(case)
    st = dpo_states(case, dev)[1]
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="must be a finite number > 0"):
            _step(tu, st, batch, dev, rand=rand, dpo_beta=beta)
    with pytest.raises(ValueError, match="must carry a LoRA / DoRA adapter"):
        _step(tu, build_hip_states(case, dev)[1], batch, dev, rand=rand, dpo_beta=BETA)
    with pytest.raises(ValueError, match="text-encoder adapter"):
        _step(tu, tl._lora_states(case, dev, te="lora")[1], batch, dev, rand=rand, dpo_beta=BETA)
    odd = {k: v[:3] for k, v in batch.items()}
    with pytest.raises(ValueError, match="must be even"):
        _step(tu, st, odd, dev, dpo_beta=BETA)
    with pytest.raises(ValueError, match="must be even"):
        _step(tu, st, batch, dev, dpo_beta=BETA, micro_batches=4)
    for key, val in (("loss_mask", torch.ones(4, 64, 64, device=dev)), ("loss_weight", torch.ones(4, device=dev))):
        with pytest.raises(ValueError, match=f"dpo_beta: {key}"):
            _step(tu, st, dict(batch, **{key: val}), dev, rand=rand, dpo_beta=BETA)
    with pytest.raises(ValueError, match="loss_type"):
        _step(tu, st, batch, dev, rand=rand, dpo_beta=BETA, loss_type="smooth_l1")
    with pytest.raises(ValueError, match="min_snr_gamma_magnitude"):
        _step(tu, st, batch, dev, rand=rand, dpo_beta=BETA, min_snr_gamma_magnitude=5.0)
    with pytest.raises(ValueError, match="data-parallel"):
        _step(tu, st, batch, dev, rand=rand, dpo_beta=BETA, reducer=object())
    out = _step(tu, st, batch, dev, rand=rand, dpo_beta=BETA)  # none of the refusals left the state unusable
    assert out[4]["loss"].item() == LN2


# ------------------------------------------------------------------------------------------------ 10
def test_four_steps_twice_give_equal_bits(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=4, image=64)
    runs = []
    for _ in range(2):
        st = dpo_states(case, dev, ema=True)[1]
        st[0].adapter.store.load(random_factors(st[0].adapter, case["weights"]["unet"], 19))
        gen = torch.Generator(device=dev)
        gen.manual_seed(9)
        trace = []
        for step in range(4):
            out = _step(tu, st, to_dev(case["batch"], dev), dev, gen=gen, dpo_beta=50.0, ema_rate=0.999)
            trace.append(_snapshot(st[0], out))
        runs.append(trace)
    assert len({float(s["loss"]) for s in runs[0]}) == 4
    for step, (a, b) in enumerate(zip(*runs)):
        _assert_same(a, b, f"second run at step {step}")
