"""SDXL text conditioning on a real MI355X (nets.dual_clip_config(sdxl_conditioning=True)): the EOS-pooling kernel with its final
LayerNorm (sdt_clip_pool_fwd / _bwd), both towers against transformers (tests/golden/sdxl_text_pin_*.npz, made by
make_sdxl_text_pin.py), a tiny SDXL train_step from ids and pixels alone against a CPU fp32 restatement written here from oracle.nets
primitives (the oracle's own train_step takes the pooled embedding as an input), its captured replay and micro-batches, and SDXL
sampling.  Tolerances: bf16 activations against fp32 references, the gates of test_gpu_model.py / test_gpu_grad_accum.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import rel_l2, to_dev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cos(a, b):
    a, b = a.float().flatten().cpu(), b.float().flatten().cpu()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))


# ----------------------------------------------------------------------------- 1. the pooling kernel
def _pool_ref(ids, x, gamma, beta, eos_id, windows, eps=1e-5):
    rows = ids[::windows].long()
    pos = rows.argmax(-1) if eos_id < 0 else (rows == eos_id).int().argmax(-1)
    xs = x[::windows][torch.arange(rows.shape[0]), pos].float().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xs, (x.shape[-1],), gamma, beta, eps)
    return pos, xs, y


@pytest.mark.parametrize("D", [48, 768, 1280])
@pytest.mark.parametrize("R,windows", [(1, 1), (3, 1), (10, 1), (3, 2)])
@pytest.mark.parametrize("rule", ["argmax", "eos"])
def test_clip_pool_kernel_matches_torch(dev, D, R, windows, rule):
    from stable_diffusion_training_amd import _lib
    S, V = 77, 100
    g = torch.Generator().manual_seed(D + 7 * R + windows)
    ids = torch.randint(0, V - 2, (R * windows, S), generator=g, dtype=torch.int32)
    ids[:, 0] = V - 2
    for r in range(R * windows):  # eos at varying places, padded with eos (argmax / first occurrence) or with 0
        e = int(torch.randint(1, S, (1,), generator=g))
        ids[r, e] = V - 1
        ids[r, e + 1:] = V - 1 if r % 2 else 0
    eos_id = -1 if rule == "argmax" else V - 1
    x = (torch.randn(R * windows, S, D, generator=g) * 2 + 0.5).to(torch.bfloat16)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(R, D, generator=g).to(torch.bfloat16)
    rg, rb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    pos, xs, y = _pool_ref(ids, x.float(), rg, rb, eos_id, windows)
    y.backward(dy.float())
    s = torch.cuda.current_stream().cuda_stream

    def run():
        d_ids, d_x, d_g, d_b, d_dy = (t.to(dev).contiguous() for t in (ids, x, gamma, beta, dy))
        pooled = torch.empty(R, D, dtype=torch.bfloat16, device=dev)
        mr = torch.empty(R, 2, device=dev)
        p = torch.empty(R, dtype=torch.int32, device=dev)
        _lib.call("sdt_clip_pool_fwd", d_ids.data_ptr(), d_x.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), pooled.data_ptr(), mr.data_ptr(),
                  p.data_ptr(), R, windows, S, D, eos_id, 1e-5, s)
        dx = torch.full_like(d_x, float("nan"))  # every element must be written
        dg, db = torch.full((D,), 0.25, device=dev), torch.full((D,), -0.5, device=dev)  # accumulated into (+=)
        _lib.call("sdt_clip_pool_bwd", d_x.data_ptr(), d_dy.data_ptr(), d_g.data_ptr(), mr.data_ptr(), p.data_ptr(), dx.data_ptr(),
                  dg.data_ptr(), db.data_ptr(), R, windows, S, D, s)
        torch.cuda.synchronize()
        return pooled.cpu(), p.cpu(), dx.cpu(), dg.cpu(), db.cpu()

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two runs differ"
    pooled, p, dx, dg, db = a
    assert torch.equal(p.long(), pos)
    assert rel_l2(pooled, y.detach()) < 1e-2
    rows = torch.arange(R) * windows
    mask = torch.zeros(R * windows, S, dtype=torch.bool)
    mask[rows, pos] = True
    assert not torch.isnan(dx).any() and float(dx[~mask].abs().max()) == 0.0  # exactly zero off the pooled rows
    assert rel_l2(dx[rows, pos], xs.grad) < 2e-2
    assert rel_l2(dg - 0.25, rg.grad) < 1e-3 and rel_l2(db + 0.5, rb.grad) < 1e-3


# ----------------------------------------------------------------------------- 2. both towers against transformers
def _pin_store(dev, z):
    from stable_diffusion_training_amd import nets, params
    t1, t2 = json.loads(str(z["towers"]))
    cfg = nets.dual_clip_config(t1, t2, sdxl_conditioning=True)
    st = params.ParamStore(nets.clip_text_spec(cfg), device=dev, quantise=False)
    st.load({k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")})
    st.prepare()
    return cfg, st


@pytest.mark.parametrize("case", ["argmax", "eos", "pad_ne_eos"])
def test_towers_match_transformers(dev, case):
    from stable_diffusion_training_amd import nets
    z = np.load(os.path.join(GOLDEN, f"sdxl_text_pin_{case}.npz"))
    cfg, st = _pin_store(dev, z)
    st.fill_grad(7.0)  # stale gradients: the leaves SDXL mode never reads must come out exactly zero all the same
    st.mark_unused(nets.unused_text_leaves(cfg))
    st.zero_grad()
    ctx, pooled = nets.sdxl_text_forward(st, cfg, torch.from_numpy(z["ids"]).to(dev))
    assert rel_l2(ctx, torch.from_numpy(z["context"])) < 2e-2
    assert rel_l2(pooled, torch.from_numpy(z["pooled"])) < 2e-2
    cots = [torch.from_numpy(z[k].astype(np.float32)).to(dev, torch.bfloat16) for k in ("cot_context", "cot_pooled")]
    torch.autograd.backward([ctx, pooled], cots)
    got = st.export("grad")
    unused = set(nets.unused_text_leaves(cfg))
    assert unused and any("final_layer_norm" in k for k in unused)
    for k in unused:
        assert float(got[k].abs().max()) == 0.0, k
    flat = [k for k in got if k not in unused]
    assert "text_encoder_2/text_projection/kernel" in flat
    a = torch.cat([got[k].flatten().cpu() for k in flat])
    b = torch.cat([torch.from_numpy(z["g:" + k].astype(np.float32)).flatten() for k in flat])
    assert rel_l2(a, b) < 3e-2
    for k in flat:
        ref = torch.from_numpy(z["g:" + k].astype(np.float32))
        if ref.norm() > 1e-3 * b.norm():
            assert _cos(got[k], ref) > 0.99, (k, _cos(got[k], ref))


# ----------------------------------------------------------------------------- 3. a tiny SDXL train_step from ids and pixels
UNET_OVER = dict(block_out_channels=(64, 128, 256), attention_head_dim=(2, 4, 8), cross_attention_dim=80,
                 transformer_layers_per_block=(1, 2, 1), addition_time_embed_dim=32, projection_class_embeddings_input_dim=40 + 6 * 32)


def _case(B=2, image=64, seed=0):
    from oracle import nets as onets
    from oracle import schedulers as osched
    from stable_diffusion_training_amd import nets
    z = np.load(os.path.join(GOLDEN, "sdxl_text_pin_argmax.npz"))
    t1, t2 = json.loads(str(z["towers"]))
    clip = nets.dual_clip_config(t1, t2, sdxl_conditioning=True)
    cfgs = dict(unet=onets.unet_config("sdxl", **UNET_OVER), vae=onets.vae_config("tiny"), clip=clip)
    w = dict(unet=onets.init_params(onets.unet_param_shapes(cfgs["unet"]), seed + 1),
             vae=onets.init_params(onets.vae_encoder_param_shapes(cfgs["vae"]), seed + 2),
             clip=onets.init_params(dict(nets.clip_text_spec(clip)), seed + 3))
    g = torch.Generator().manual_seed(seed + 10)
    ids = torch.randint(0, 62, (B, 2, 77), generator=g)
    ids[..., 0] = 62
    for r in range(B):
        ids[r, :, 20 + 11 * r:] = 63
    lh = image // 8
    batch = dict(pixel_values=torch.rand(B, 3, image, image, generator=g) * 2 - 1, input_ids=ids)
    rand = dict(posterior_eps=torch.randn(B, lh, lh, 4, generator=g), noise=torch.randn(B, 4, lh, lh, generator=g),
                timesteps=torch.randint(0, 1000, (B,), generator=g))
    return dict(cfgs=cfgs, weights=w, batch=batch, rand=rand, sched_state=osched.create_state("scaled_linear"), sched="scaled_linear")


def _oracle_tower(p, t, ids, prefix, n_layers):
    """oracle.nets.clip_text_forward's layers, stopped after n_layers and without the final LayerNorm"""
    import torch.nn.functional as F
    from oracle import nets as onets
    d, heads, eps = t["hidden_size"], t["num_attention_heads"], t["layer_norm_eps"]
    x = p[prefix + "text_model/embeddings/token_embedding/embedding"][ids.long()]
    x = x + p[prefix + "text_model/embeddings/position_embedding/embedding"][: ids.shape[1]][None]
    for i in range(n_layers):
        L = f"{prefix}text_model/encoder/layers/{i}"
        h = onets.layer_norm(x, p, L + "/layer_norm1", eps)
        q, k, v = (onets.dense(h, p, f"{L}/self_attn/{n}") for n in ("q_proj", "k_proj", "v_proj"))
        x = x + onets.dense(onets.attention_core(q, k, v, heads, (d // heads) ** -0.5, causal=True), p, L + "/self_attn/out_proj")
        h = onets.dense(onets.layer_norm(x, p, L + "/layer_norm2", eps), p, L + "/mlp/fc1")
        h = h * torch.sigmoid(1.702 * h) if t["hidden_act"] == "quick_gelu" else F.gelu(h)
        x = x + onets.dense(h, p, L + "/mlp/fc2")
    return x


def oracle_sdxl_text(p, cfg, ids, windows=1):
    """(context, pooled): hidden_states[-2] of both towers; text_projection(final LN of the last layer at the EOS token)."""
    from oracle import nets as onets
    (t1, t2), (p1, p2) = cfg["towers"], cfg["prefixes"]
    c1 = _oracle_tower(p, t1, ids[:, 0], p1, t1["num_hidden_layers"] - 1)
    c2 = _oracle_tower(p, t2, ids[:, 1], p2, t2["num_hidden_layers"] - 1)
    xn = _oracle_tower(p, t2, ids[::windows, 1], p2, t2["num_hidden_layers"])
    rows = ids[::windows, 1].long()
    pos = rows.argmax(-1) if t2["eos_token_id"] == 2 else (rows == t2["eos_token_id"]).int().argmax(-1)
    pooled = onets.layer_norm(xn[torch.arange(rows.shape[0]), pos], p, p2 + "text_model/final_layer_norm", t2["layer_norm_eps"])
    return torch.cat([c1, c2], -1), pooled @ p[p2 + "text_projection/kernel"]


def oracle_sdxl_step(case, vae_scale=0.18215):
    """loss and gradients of oracle.train_step.compute_loss with the conditioning of oracle_sdxl_text (epsilon target)."""
    from oracle import nets as onets
    from oracle import schedulers as osched
    w, cfgs, batch, rand = case["weights"], case["cfgs"], case["batch"], case["rand"]
    up = {k: v.clone().requires_grad_(True) for k, v in w["unet"].items()}
    tp = {k: v.clone().requires_grad_(True) for k, v in w["clip"].items()}
    with torch.no_grad():
        moments = onets.vae_encode_moments(w["vae"], cfgs["vae"], batch["pixel_values"])
        latents = onets.vae_sample_latents(moments, rand["posterior_eps"], vae_scale).contiguous()
    t = rand["timesteps"]
    noisy = torch.from_numpy(osched.add_noise(case["sched_state"], latents.numpy(), rand["noise"].numpy(), t.numpy()))
    B, _, H, W = batch["pixel_values"].shape
    ctx, pooled = oracle_sdxl_text(tp, cfgs["clip"], batch["input_ids"])
    tid = torch.tensor([[H, W, 0, 0, H, W]] * B)
    pred = onets.unet_forward(up, cfgs["unet"], noisy, t, ctx, dict(text_embeds=pooled, time_ids=tid))
    loss = ((rand["noise"] - pred) ** 2).mean()
    leaves = list(up.values()) + list(tp.values())
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    z = [torch.zeros_like(v) if g is None else g for v, g in zip(leaves, grads)]
    return float(loss.detach()), dict(zip(up, z[: len(up)])), dict(zip(tp, z[len(up):]))


def _states(case, dev, ema=False):
    from tests.helpers import build_hip_states
    return build_hip_states(case, dev, quantize=False, ema=ema)


def test_sdxl_train_step_from_ids_matches_restatement(dev):
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    case = _case()
    loss_ref, gu_ref, gt_ref = oracle_sdxl_step(case)
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
    ts.store.fill_grad(3.0)  # stale values in the never-written CLIP-L leaves would survive a step that does not clear them
    batch = to_dev(case["batch"], dev)
    aux = {}
    out = tu.train_step(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False,
                        rand=to_dev(case["rand"], dev), aux=aux)
    loss = out[4]["loss"].item()
    assert abs(loss - loss_ref) / loss_ref < 1e-2, (loss, loss_ref)
    assert tuple(aux["text_embeds"].shape) == (2, 40)
    unused = set(nets.unused_text_leaves(case["cfgs"]["clip"]))
    for store, ref in ((us.store, gu_ref), (ts.store, gt_ref)):
        got = store.export("grad")
        keys = [k for k in ref if k not in unused]
        a = torch.cat([got[k].flatten().cpu() for k in keys])
        b = torch.cat([ref[k].flatten() for k in keys])
        assert _cos(a, b) > 0.995
        worst = max((rel_l2(got[k], ref[k]), k) for k in keys if ref[k].norm() > 1e-3 * b.norm())
        assert worst[0] < 0.1, worst
    gt = ts.store.export("grad")
    for k in unused:
        assert float(gt[k].abs().max()) == 0.0, k
    for k in ("text_encoder_2/text_projection/kernel", "text_encoder_2/text_model/final_layer_norm/scale",
              "text_encoder/text_model/encoder/layers/0/mlp/fc2/kernel", "add_embedding/linear_1/kernel"):
        ref = gt_ref.get(k, gu_ref.get(k))
        assert _cos((gt if k in gt else us.store.export("grad"))[k], ref) > 0.99, k
    # the pooled embedding is the towers' output: an explicit one is refused
    bad = dict(batch, text_embeds=torch.zeros(2, 40, device=dev))
    with pytest.raises(ValueError, match="text_embeds"):
        tu.train_step(us, ts, None, None, bad, torch.Generator(device=dev), vae, sc, rand=to_dev(case["rand"], dev))


def _snapshot(us, ts):
    return {f"{n}.{b}": getattr(s.store, b).clone() for n, s in (("unet", us), ("te", ts)) for b in ("master", "mom", "grad")
            if getattr(s.store, b) is not None}


def test_sdxl_captured_step_equals_eager_and_micro_batches_match(dev):
    from stable_diffusion_training_amd import training_utils as tu
    case = _case()

    def run(use_graph):
        tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph, per_device_batch=2)
        fn = table[(2, 3, 512, 512)]
        trace = []
        for step in range(3):
            g = torch.Generator().manual_seed(50 + step)
            batch = to_dev(case["batch"], dev)
            batch["pixel_values"] = (batch["pixel_values"] * (1 - 0.1 * step)).contiguous()
            rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
                    for k, v in case["rand"].items()}
            out = fn(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, rand=rand)
            snap = _snapshot(us, ts)
            snap["loss"] = out[4]["loss"].clone()
            trace.append(snap)
        if use_graph:
            assert fn.graph is not None
        return trace

    eager, graph = run(False), run(True)
    for step, (a, b) in enumerate(zip(eager, graph)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"graph replay differs from the eager run at step {step}, {k}"

    # K = 2 micro-batches of 1 against the plain step over both samples (gates of test_gpu_grad_accum.py)
    res = {}
    for K in (1, 2):
        tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
        out = tu.train_step(us, ts, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc,
                            strip_bos_eos_token=False, rand=to_dev(case["rand"], dev), micro_batches=K)
        res[K] = (out[4]["loss"].item(), us.store.export("grad"), ts.store.export("grad"))
    assert abs(res[2][0] - res[1][0]) / res[1][0] < 1e-2
    for i in (1, 2):
        g1, g2 = res[1][i], res[2][i]
        keys = [k for k in g1 if g1[k].norm() > 0]
        assert _cos(torch.cat([g2[k].flatten() for k in keys]), torch.cat([g1[k].flatten() for k in keys])) > 0.995


# ----------------------------------------------------------------------------- 4. SDXL sampling
def oracle_sdxl_generate(case, w_vae, ids, neg, lat0, steps, scale, H, W, ptype):
    from oracle import nets as onets
    from oracle import schedulers as osched
    with torch.no_grad():
        cfgs = case["cfgs"]
        ctx, pooled = oracle_sdxl_text(case["weights"]["clip"], cfgs["clip"], ids)
        if neg is None:
            nctx, npooled = torch.zeros_like(ctx), torch.zeros_like(pooled)
        else:
            nctx, npooled = oracle_sdxl_text(case["weights"]["clip"], cfgs["clip"], neg)
        ctx, pooled = torch.cat([nctx, ctx]), torch.cat([npooled, pooled])
        tid = torch.tensor([[H, W, 0, 0, H, W]] * ctx.shape[0])
        lat = lat0.clone()
        for t in osched.ddim_timesteps(steps):
            x2 = torch.cat([lat, lat])
            out = onets.unet_forward(case["weights"]["unet"], cfgs["unet"], x2, torch.full((x2.shape[0],), int(t)), ctx,
                                     dict(text_embeds=pooled, time_ids=tid))
            un, tx = out.chunk(2)
            lat = torch.from_numpy(osched.ddim_step(case["sched_state"], (un + scale * (tx - un)).numpy(), int(t), lat.numpy(), steps, ptype))
        img = onets.vae_decode(w_vae, cfgs["vae"], (lat / 0.13025).permute(0, 2, 3, 1))
        return (img / 2 + 0.5).clamp(0, 1), lat


def test_sdxl_generate_matches_restatement(dev):
    from oracle import nets as onets
    from stable_diffusion_training_amd.pipeline import StableDiffusionPipeline
    from stable_diffusion_training_amd.schedulers import DDIMScheduler
    case = _case()
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev)
    w_vae = dict(case["weights"]["vae"])
    w_vae.update(onets.init_params(onets.vae_decoder_param_shapes(case["cfgs"]["vae"]), 9))
    sch = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon")
    pipe = StableDiffusionPipeline(us, ts, w_vae, case["cfgs"]["unet"], case["cfgs"]["clip"], case["cfgs"]["vae"], scheduler=sch,
                                   scaling_factor=0.13025)
    ids = case["batch"]["input_ids"]
    neg = ids.flip(0).clone()
    lat0 = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4))
    for n in (None, neg):
        want_img, want_lat = oracle_sdxl_generate(case, w_vae, ids, n, lat0, 2, 5.0, 128, 128, "epsilon")
        img, lat = pipe.generate(ids.to(dev), num_inference_steps=2, height=128, width=128, guidance_scale=5.0, latents=lat0.to(dev),
                                 neg_prompt_ids=None if n is None else n.to(dev), return_latents=True)
        assert tuple(img.shape) == (2, 128, 128, 3)
        assert rel_l2(lat, want_lat) < 3e-2, n is None
        assert float((img.cpu() - want_img).abs().mean()) < 1e-2
    with pytest.raises(ValueError, match="2, 77"):
        pipe.generate(ids[:, 0].to(dev), num_inference_steps=2, height=128, width=128)
