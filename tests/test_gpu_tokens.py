"""New tokens (textual inversion, alone and beside a UNet LoRA) on the MI355X at model level, on the tiny configuration at 64 x 64,
batch 2.  The oracle is unchanged: it runs on the text encoder's tree with the token table resized to V + n rows, and rows V... of its
token-embedding gradient are the reference of the token gradient."""
import types

import numpy as np
import pytest
import torch

from tests import token_reference as tr
from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu
TOK = "text_model/embeddings/token_embedding/embedding"
NEW = "text_model/embeddings/token_embedding/new_tokens"
STATE = ("master", "codes", "inv_scale", "mom", "ema")
N = 2
SLOTS = ((1, 0), (2, 1), (9, 0), (10, 1), (30, 1), (31, 0))  # (caption position, placeholder): each placeholder in three positions


def _models(case):
    return {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
            "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
            "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}


def _states(case, dev, cfg=None, pivotal=False, ema=False):
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
    lo = dict(unet=lora.LoraConfig(8, 4.0, seed=1), text_encoder="frozen") if pivotal else None
    return tc, tu.on_device_model_training_state(tc, _models(case), device=dev, lora=lo, new_tokens=cfg)


def _place(ids, ids_of):
    """input_ids with ids_of[j] at placeholder j's SLOTS in every caption row (last axis: the caption)."""
    ids = ids.clone()
    for pos, j in SLOTS:
        ids[..., pos] = ids_of[j]
    return ids


def _case(V_ids, B=2):
    """The tiny case whose captions carry V_ids[j] at placeholder j's positions."""
    case = make_case("tiny", B=B, image=64)
    case["batch"] = dict(case["batch"], input_ids=_place(case["batch"]["input_ids"], V_ids))
    return case


def _vocab(case):
    return case["cfgs"]["clip"]["vocab_size"]


def _step(tu, st, case, dev, **kw):
    us, ts, ue, te, vae, sc, _ = st
    return tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                         rand=to_dev(case["rand"], dev), **kw)


def _random_rows(tk, seed):
    """Random new rows at the base table's scale (an EMA, when kept, starts equal)."""
    g = torch.Generator().manual_seed(seed)
    tk.store.load({p: torch.randn(tk.store.leaves[p].shape, generator=g) * float(tk.target_std[i]) for i, p in enumerate(tk.store.order)})


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("pivotal", [False, True])
def test_tokens_copied_from_init_ids_give_the_bits_of_the_init_ids(dev, pivotal):
    """Placeholder rows that are copies of tok[5] and tok[17]: context, prediction and loss equal, bit for bit, those of states
    without tokens whose captions carry 5 and 17 in the same places - alone against a full fine-tune state, and with a fresh UNet
    LoRA (B = 0) against the same LoRA state without tokens."""
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    got = {}
    for name, case, build in (("base", _case((5, 17)), lambda c: _states(c, dev, pivotal=True)[1] if pivotal else build_hip_states(c, dev)[1]),
                              ("tokens", _case((V, V + 1)), lambda c: _states(c, dev, tokens.TokenConfig(N, init_ids=(5, 17)), pivotal)[1])):
        st, aux = build(case), {}
        out = _step(tu, st, case, dev, aux=aux)
        got[name] = dict(ctx=aux["ctx"].clone(), pred=aux["pred"].clone(), loss=out[4]["loss"].clone())
    assert np.isfinite(got["tokens"]["loss"].item())
    for k in ("ctx", "pred", "loss"):
        assert torch.equal(got["base"][k], got["tokens"][k]), k


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("pivotal", [False, True])
def test_token_gradient_matches_the_oracle_on_the_resized_table(dev, pivotal, K):
    """oracle/train_step.py, unmodified, on the (V + n)-row table: rows V... of its token-embedding gradient.  test_gpu_lora.py's
    gates for the same reason (the same tiny step with bf16 activations and gradients): loss within 1e-2, rel-L2 of the leaf below
    0.1.  K = 2: two micro-batches of 2 against the oracle's one step over all four samples."""
    from oracle import train_step as ots
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1), B=2 * K)
    tc, st = _states(case, dev, tokens.TokenConfig(N, seed=4), pivotal)
    us, ts = st[0], st[1]
    _random_rows(ts.tokens, 7)
    clip_w = dict(case["weights"]["clip"])
    clip_w[TOK] = torch.cat([clip_w[TOK], ts.tokens.store.export("master")[NEW].cpu()])
    cfgs = dict(case["cfgs"], clip=dict(case["cfgs"]["clip"], vocab_size=V + N))
    ref = ots.train_step(case["weights"]["unet"], clip_w, case["weights"]["vae"], case["sched_state"], cfgs, case["batch"], case["rand"],
                         dict(ots.DEFAULT_OPT))
    out = _step(tu, st, case, dev, micro_batches=K)
    loss = out[4]["loss"].item()
    want = torch.as_tensor(ref["te_grads"][TOK])[V:].float()
    got = ts.tokens.store.export("grad")[NEW]
    e = rel_l2(got, want)
    print(f"[tokens pivotal={pivotal} K={K}] loss {loss:.6f} vs {ref['loss']:.6f}, token gradient rel-L2 {e:.4f}, |g| {float(want.norm()):.3e}")
    assert abs(loss - ref["loss"]) / ref["loss"] < 1e-2
    assert float(want.norm()) > 0 and e < 0.1, e
    assert (ts.tokens.store.gacc is not None) == (K > 1)
    assert ts.step == 1 and ts.store.count == 0 and us.store.count == 0 and us.step == (1 if pivotal else 0)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("pivotal", [False, True])
def test_step_semantics(dev, pivotal):
    """Only the new_tokens leaves move (and the LoRA leaves in pivotal mode); masters and mirrors of both frozen bases keep every bit."""
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    tc, st = _states(case, dev, tokens.TokenConfig(N, seed=4), pivotal, ema=True)
    us, ts = st[0], st[1]
    _random_rows(ts.tokens, 8)
    assert st[3].store is ts.tokens.store and (st[2] is None) == (not pivotal)
    before = [(s.store.master.clone(), s.store.w.clone()) for s in (us, ts)]
    t0, e0 = ts.tokens.store.master.clone(), ts.tokens.store.ema.clone()
    a0 = us.adapter.store.master.clone() if pivotal else None
    out = _step(tu, st, case, dev, ema_rate=0.999)
    torch.cuda.synchronize()
    assert np.isfinite(out[4]["loss"].item())
    if not pivotal:  # nothing of the UNet's is merged or stepped: the mirror is the load's
        assert torch.equal(us.store.w, before[0][1]), "the frozen UNet's mirror was rewritten"
        assert us.opt_store is None and us.step == 0
    else:
        lb = [us.adapter.adapted[p][1] for p in us.adapter.paths]
        assert all(not torch.equal(us.adapter.store.p(q), torch.zeros_like(us.adapter.store.p(q))) for q in lb), "a LoRA B leaf did not move"
        assert not torch.equal(us.adapter.store.master, a0)
    for s, (m, w) in zip((us, ts), before):
        assert torch.equal(s.store.master, m), "a frozen master moved"
    assert torch.equal(ts.store.w, before[1][1]), "the frozen text encoder's mirror was rewritten"
    g = ts.tokens.store.export("grad")[NEW]
    assert bool((g != 0).float().mean() > 0.9)
    moved = ts.tokens.store.p(NEW) != t0[ts.tokens.store.leaves[NEW].offset:][: g.numel()].view(g.shape)
    assert bool(moved[g != 0].all()) and ts.step == 1
    # Lion: every element with a gradient moves against it; the EMA follows the stepped master
    lf = ts.tokens.store.leaves[NEW]
    p0, p1 = t0[lf.offset: lf.offset + lf.numel].view(g.shape).double(), ts.tokens.store.p(NEW).double()
    assert bool((torch.sign(p0 - p1)[g != 0] == torch.sign(g)[g != 0]).float().mean() > 0.99)
    want = 0.999 * e0.double() + (1 - 0.999) * ts.tokens.store.master.double()
    assert torch.allclose(ts.tokens.store.ema.double(), want, atol=1e-6, rtol=0)


def test_retract_acts_on_the_stepped_master_and_leaves_the_ema(dev):
    """Two states that differ only in TokenConfig.retract: the retracting one's master is the reference's retraction of the other's
    stepped master - mean and std within the kernel test's bounds, the factor within one fp32 ulp of the float64 pow at the published
    std, the rows fl32(x * factor) bit for bit - and its EMA is the other's (the sweep's value)."""
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    res = {}
    for retract in (False, True):
        tc, st = _states(case, dev, tokens.TokenConfig(N, seed=4, retract=retract, retract_power=0.5), ema=True)
        tk = st[1].tokens
        g = torch.Generator().manual_seed(9)
        tk.store.load({NEW: torch.randn(tk.store.leaves[NEW].shape, generator=g) * 3 * tk.target_std[0]})  # (well off the target)
        _step(tu, st, case, dev, ema_rate=0.999)
        torch.cuda.synchronize()
        res[retract] = (tk.store.p(NEW).cpu().numpy().copy(), tk.store.ema.clone(), tk.stats.cpu().numpy().copy(), tk.target_std[0])
    stepped, ema_off, _, target = res[False]
    got, ema_on, stats, _ = res[True]
    mean, std, factor = (float(v) for v in stats[0])
    rmean, rstd = tr.retract_stats(stepped)
    n, u = stepped.size, 2.0 ** -53
    b_mean = tr.sum_bound(stepped.astype(np.float64)) / n + 2 * u * abs(rmean)
    assert abs(mean - rmean) <= b_mean and abs(std - rstd) <= 2 * rstd * ((n + 2) * u / 2 + 2 * u) + 1e-300
    want_f = tr.retract_factor(std, target, 0.5)
    ulp = float(np.nextafter(want_f, np.float32(np.inf)) - want_f)
    assert abs(factor - float(want_f)) <= ulp and abs(factor - 3.0 ** -0.5) < 0.1
    assert np.array_equal(got.view(np.int32), tr.retract_apply(stepped, factor).view(np.int32))
    assert torch.equal(ema_on, ema_off)


# ------------------------------------------------------------------------------------------------ 4, 5, 6
_RUNS = {}


def _fresh(case, dev, seed):
    from stable_diffusion_training_amd import tokens
    tc, st = _states(case, dev, tokens.TokenConfig(N, seed=4, retract=True), pivotal=True, ema=True)
    _random_rows(st[1].tokens, seed)
    return tc, st


def _snapshot(us, ts, out):
    snap = {"loss": out[4]["loss"].clone()}
    for name, store in (("unet", us.adapter.store), ("tokens", ts.tokens.store)):
        for b in STATE:
            if getattr(store, b, None) is not None:
                snap[f"{name}.{b}"] = getattr(store, b).clone()
    return snap


def _trajectory(dev, use_graph, fresh=False):
    """Four pivotal-tuning steps (tokens with retraction + UNet LoRA, EMA on) through dp_compile_all_unique_resolution."""
    key = ("traj", use_graph)
    if key in _RUNS and not fresh:
        return _RUNS[key]
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    tc, (us, ts, ue, te, vae, sc, _) = _fresh(case, dev, 31)
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
        trace.append(_snapshot(us, ts, fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)))
    if use_graph:
        assert fn.graph is not None and fn.calls == 2
    assert us.step == 4 and ts.step == 4 and us.store.count == 0 and ts.store.count == 0
    _RUNS[key] = trace
    return trace


def test_captured_steps_equal_eager_steps(dev):
    eager, graph = _trajectory(dev, False), _trajectory(dev, True)
    assert len({float(s["loss"]) for s in graph}) == 4
    for step, (a, b) in enumerate(zip(eager, graph)):
        assert set(a) == set(b) and "tokens.master" in a and "tokens.ema" in a
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager step at step {step}, {k}"
    assert not torch.equal(eager[0]["tokens.master"], eager[3]["tokens.master"])


def test_four_steps_are_reproducible(dev):
    first, again = _trajectory(dev, False), _trajectory(dev, False, fresh=True)
    for a, b in zip(first, again):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_checkpoint_resume_is_bitwise(dev, tmp_path):
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    path = str(tmp_path / "state.safetensors")

    def two_steps(st, gen):
        for _ in range(2):
            out = tu.train_step(st[0], st[1], st[2], st[3], to_dev(case["batch"], dev), gen, st[4], st[5], strip_bos_eos_token=False, ema_rate=0.999)
        return _snapshot(st[0], st[1], out)

    (_, st), gen = _fresh(case, dev, 51), torch.Generator(device=dev)
    gen.manual_seed(5)
    tu.train_step(st[0], st[1], st[2], st[3], to_dev(case["batch"], dev), gen, st[4], st[5], strip_bos_eos_token=False, ema_rate=0.999)
    tu.save_training_state(path, st[0], st[1], train_rng=gen)
    from safetensors import safe_open
    with safe_open(path, framework="pt", device="cpu") as f:
        assert f.get_tensor("text_encoder.master").numel() == st[1].tokens.store.total  # the token rows: the frozen base is not written
        assert "num_tokens=2" in f.metadata()["text_encoder.tokens"]
    a = two_steps(st, gen)
    (_, st2), gen2 = _fresh(case, dev, 61), torch.Generator(device=dev)  # other rows: everything must come from the file
    tu.load_training_state(path, st2[0], st2[1], train_rng=gen2)
    assert st2[0].step == 1 and st2[1].step == 1
    b = two_steps(st2, gen2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a state of another kind is refused: more tokens, no tokens at all (a frozen text encoder), a LoRA-only file's counterpart
    _, other = _states(case, dev, tokens.TokenConfig(3), pivotal=True, ema=True)
    with pytest.raises(ValueError, match="new-token settings"):
        tu.load_training_state(path, other[0], other[1])
    _, lora_only = _states(case, dev, None, pivotal=True, ema=True)
    with pytest.raises(ValueError, match="frozen in only one"):
        tu.load_training_state(path, lora_only[0], lora_only[1])


# ------------------------------------------------------------------------------------------------ 7
def test_sampling_reads_the_tokens_and_equals_the_resized_checkpoint(dev, tmp_path):
    """generate with the tokens attached == generate from save_model's resized checkpoint loaded into plain stores, for the master
    and for the EMA."""
    from oracle import nets as onets
    from stable_diffusion_training_amd import checkpoint as ck
    from stable_diffusion_training_amd import nets, tokens
    from stable_diffusion_training_amd.params import ParamStore
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    cfgs = case["cfgs"]
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(cfgs["vae"]), 9))
    tc, st = _states(case, dev, tokens.TokenConfig(N, seed=4), ema=True)
    us, ts, te_ema = st[0], st[1], st[3]
    _random_rows(ts.tokens, 71)
    ts.tokens.store.ema.mul_(-0.5)  # an EMA that differs from the master
    ids = case["batch"]["input_ids"].to(dev)
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)

    def generate(unet, text, clip_cfg):
        pipe = StableDiffusionPipeline(unet, text, vae_w, cfgs["unet"], clip_cfg, cfgs["vae"], device=dev)
        return pipe.generate(ids, num_inference_steps=2, height=64, width=64, latents=lat)

    def from_checkpoint(text_params, name):
        root = str(tmp_path / name)
        ck.save_model({"unet": cfgs["unet"], "vae": cfgs["vae"], "text_encoder": cfgs["clip"]}, None, us, text_params, vae_w, root)
        m = ck.load_models(types.SimpleNamespace(model_path=root), load_tokenizer=False)
        ccfg = m["text_encoder"]["config"]
        assert ccfg["vocab_size"] == V + N and ccfg["num_new_tokens"] == N
        u = ParamStore(nets.unet_spec(m["unet"]["config"]), device=dev, trainable=False)
        t = ParamStore(nets.clip_text_spec(ccfg), device=dev, trainable=False)
        u.load(m["unet"]["unet_params"])
        t.load(m["text_encoder"]["text_encoder_params"])
        assert t.tokens is None and t.leaves[TOK].shape[0] == V + N
        return generate(u, t, ccfg)

    with_tokens = generate(us, ts, cfgs["clip"])
    assert torch.equal(with_tokens, from_checkpoint(ts, "master"))
    ts.tokens.select("ema")
    ema_img = generate(us, ts, cfgs["clip"])
    assert not torch.equal(ema_img, with_tokens)
    assert torch.equal(ema_img, from_checkpoint(te_ema, "ema"))


# ------------------------------------------------------------------------------------------------ 8
def test_sdxl_mode_one_step_moves_both_towers_leaves(dev):
    from stable_diffusion_training_amd import tokens
    from stable_diffusion_training_amd import training_utils as tu
    from tests.test_gpu_sdxl_conditioning import _case as sdxl_case
    case = sdxl_case()
    vocabs = [t["vocab_size"] for t in case["cfgs"]["clip"]["towers"]]
    ids = case["batch"]["input_ids"].clone()
    for i, v in enumerate(vocabs):
        ids[:, i, 1], ids[:, i, 2], ids[:, i, 5] = v, v + 1, v
    case["batch"] = dict(case["batch"], input_ids=ids)
    tc, st = _states(case, dev, tokens.TokenConfig(N, init_ids=(3, 4)))
    tk = st[1].tokens
    assert len(tk.store.order) == 2 and [V for V, _ in tk.geometry] == vocabs
    t0 = tk.store.master.clone()
    out = _step(tu, st, case, dev)
    assert np.isfinite(out[4]["loss"].item())
    for p in tk.store.order:
        lf = tk.store.leaves[p]
        assert bool((tk.store.export("grad")[p] != 0).any()), p
        assert not torch.equal(tk.store.p(p), t0[lf.offset: lf.offset + lf.numel].view(lf.shape)), f"{p} did not move"


# ------------------------------------------------------------------------------------------------ 9
def test_refusals_on_the_device(dev):
    from stable_diffusion_training_amd import lora, tokens
    from stable_diffusion_training_amd import training_utils as tu
    V = _vocab(make_case("tiny"))
    case = _case((V, V + 1))
    tc, st = _states(case, dev, tokens.TokenConfig(N))
    with pytest.raises(ValueError, match="new tokens: data-parallel"):
        _step(tu, st, case, dev, reducer=object())
    with pytest.raises(ValueError, match="already"):
        tokens.attach(st[1].store, tokens.TokenConfig(N))
    with pytest.raises(ValueError, match="new tokens"):
        lora.attach(st[1].store, lora.LoraConfig(4, 4.0, targets=lora.CLIP_TARGETS))
    full = build_hip_states(case, dev)[1]
    with pytest.raises(ValueError, match="frozen"):
        tokens.attach(full[1].store, tokens.TokenConfig(N))
    with pytest.raises(ValueError, match="new tokens: mixed modes"):  # a fully fine-tuned UNet beside the tokens
        tu.train_step(full[0], st[1], None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), st[4], st[5])
    with pytest.raises(ValueError, match="text-encoder LoRA"):
        tu.on_device_model_training_state(tc, _models(case), device=dev, new_tokens=tokens.TokenConfig(N),
                                          lora=dict(unet=lora.LoraConfig(8, 4.0), text_encoder=lora.LoraConfig(8, 4.0, targets=lora.CLIP_TARGETS)))


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("pivotal", [False, True])
def test_example_loop_trains_tokens_and_saves_the_resized_model(tmp_path, pivotal):
    """examples/train_synthetic.py with "new_tokens" (captured steps): the loader's captions carry the placeholder ids, only the token
    rows (and the UNet's adapter with lora_rank) step, and the saves are the resized model plus the token file."""
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
    V = _vocab(case)
    vae_w = dict(case["weights"]["vae"])
    vae_w.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    models = dict(_models(case), tokenizer=None)
    models["vae"] = {"vae_params": vae_w, "config": case["cfgs"]["vae"]}
    cfg = json.load(open(os.path.join(root, "tests", "golden", "model_properties_keys.json")))
    cfg.pop("_note")
    cfg.update(model_path=str(tmp_path / "model@0"), batch_size=2, image_area_root=[64], minimum_axis_length=[64],
               context_window_concatenation_count=1, strip_bos_eos_token=False, beta_scheduler="scaled_linear", prediction_type="epsilon",
               ema_rate=0.99, repeat_batch=5, chunk_number=0, chunk_steps=1, chunk_limit=1, keep_trained_model_buffer=1, master_seed=3,
               loss_logging_interval=1, loss_csv=str(tmp_path / "loss.csv"), test_save_path=str(tmp_path / "test_save"), batches_per_chunk=5,
               DEBUG=False, new_tokens=N, new_tokens_init_id=7, new_tokens_retract=True)
    if pivotal:
        cfg["lora_rank"] = 4
    losses, us, ts = mod.main(cfg, models=models, log=lambda *_: None)
    assert len(losses) == 5 and all(np.isfinite(losses)) and ts.step == 5 and us.step == (5 if pivotal else 0)
    base_rows = torch.as_tensor(case["weights"]["clip"][TOK])[[7, 7]].to(ts.store.device)
    assert not torch.equal(ts.tokens.store.p(NEW), base_rows) and ts.tokens.cfg.retract
    saved = ck.load_models(types.SimpleNamespace(model_path=str(tmp_path / "model@1")), load_tokenizer=False)
    assert saved["text_encoder"]["config"]["vocab_size"] == V + N
    table = saved["text_encoder"]["text_encoder_params"][TOK]
    assert torch.equal(torch.as_tensor(table)[V:], ts.tokens.store.p(NEW).cpu())
    assert torch.equal(torch.as_tensor(table)[:V], torch.as_tensor(case["weights"]["clip"][TOK]))
    with np.load(str(tmp_path / "model-tokens.npz")) as z:
        assert np.array_equal(z[NEW], ts.tokens.store.p(NEW).cpu().numpy())
    assert os.path.exists(str(tmp_path / "model-state.safetensors")) and os.path.exists(str(tmp_path / "model-lora.npz")) == pivotal
