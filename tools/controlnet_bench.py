"""Developer tool: the full fine-tune step against the ControlNet step (captured steps, one GPU).
For each configuration of bench.py it times the step bench.py times (bench.build_states' states) and the ControlNet step on the same
weights and batch - a ControlNet initialised from the UNet (nets.controlnet_from_unet, diffusers' default embedder widths), frozen UNet
and text encoder - as tools/lora_bench.py does: three set-up calls (two eager, capture + first replay), warm-up replays, then timed graph
replays, same box and same session.  The new op's share is measured by events around graph replays of ops.control_add at every shape
the UNet calls it with, and of the copy_cols launches of its backward: device time, summed over one step.
usage: python tools/controlnet_bench.py [--config sd15_512] [--steps 32] [--warmup 2] [--skip-full]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import nets, ops
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--config", nargs="+", choices=sorted(bench.CONFIGS), default=["sd15_512"])
ap.add_argument("--steps", type=int, default=32)  # > 1 s of timed replays at sd15_512
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-full", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)


def time_steps(step, states, batch, B):
    us, ts, ue, te, vae, sched = states
    rng = torch.Generator(device=dev)
    rng.manual_seed(1000)
    for _ in range(3 + args.warmup):  # two eager set-up steps, capture + first replay, warm-up replays
        out = step(us, ts, ue, te, batch, rng, vae, sched)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step(us, ts, ue, te, batch, rng, vae, sched)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    assert step.graph is not None
    return 1e3 * dt, B / dt, float(out[4]["loss"])


def event_ms(fn, n=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def control_add_ms(cfg, B, h, w):
    """Forward and backward milliseconds of every ops.control_add call of one UNet pass: the mid-block addition and one concatenation
    per decoder ResBlock, at the shapes unet_forward meets."""
    boc = cfg["block_out_channels"]
    nb, lpb = len(boc), cfg["layers_per_block"]
    skips = nets.skip_shapes(cfg, h, w)
    calls = [(0,) + skips[-1]]  # (Ca, Cb, h, w): the mid block, at the last skip's shape
    rev = list(reversed(boc))
    out_ch = rev[0]
    for i in range(nb):
        prev, out_ch = out_ch, rev[i]
        for j in range(lpb + 1):
            cb, hh, ww = skips.pop()
            calls.append(((prev if j == 0 else out_ch), cb, hh, ww))
    # eager launches of kernels this small are bound by the host (autograd, ctypes): each pass over the 13 shapes is captured into a
    # HIP graph and the replays are timed by events, so the figures are device time
    ops_in = []
    for ca, cb, hh, ww in calls:
        a = torch.randn(B, hh, ww, ca, device=dev).to(torch.bfloat16) if ca else None
        s, r = (torch.randn(B, hh, ww, cb, device=dev).to(torch.bfloat16) for _ in range(2))
        dy = torch.randn(B, hh, ww, ca + cb, device=dev).to(torch.bfloat16)
        da = None if a is None else torch.empty_like(a)
        ops_in.append((a, s, r, dy, da, torch.empty_like(r)))

    def forward():
        with torch.no_grad():
            for a, s, r, dy, da, dr in ops_in:
                ops.control_add(a, s, r)

    def backward():  # what _ControlAdd.backward launches: the column split of dy (nothing for the mid block: dy itself is returned)
        for a, s, r, dy, da, dr in ops_in:
            if a is not None:
                rows = dy.numel() // dy.shape[-1]
                ops.copy_cols(dy.view(rows, -1), [da.view(rows, -1), dr.view(rows, -1)], [a.shape[-1], r.shape[-1]], rows, False)

    def graphed_ms(fn, n=50):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return event_ms(g.replay, n)

    return len(calls), graphed_ms(forward), graphed_ms(backward)


for config in args.config:
    c = bench.CONFIGS[config]
    B = c["batch"]
    tc, cfgs, weights, (us, ts, ue, te, vae, sched, _) = bench.build_states(dev, B, config=config)
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
    batch = bench.synthetic_batch(dev, B, 0, config)
    res = {"config": config, "batch": B}
    if not args.skip_full:
        step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
        ms, ips, loss = time_steps(step, (us, ts, ue, te, vae, sched), batch, B)
        res["full"] = {"ms_per_step": round(ms, 3), "images_per_sec": round(ips, 2), "loss": loss}
        print(f"{config}  full: {ms:.2f} ms/step, {ips:.1f} images/sec, loss {loss:.4f}", flush=True)
        del step
    del us, ts, ue, te, vae, sched
    torch.cuda.empty_cache()

    models = {"unet": {"unet_params": weights["unet"], "config": cfgs["unet"]}, "vae": {"vae_params": weights["vae"], "config": cfgs["vae"]},
              "text_encoder": {"text_encoder_params": weights["clip"], "config": cfgs["clip"]}}
    f = 2 ** (len(cfgs["vae"]["block_out_channels"]) - 1)
    ccfg = nets.controlnet_config(cfgs["unet"], vae_downscale=f)
    us, ts, ue, te, vae, sched, _ = tu.on_device_model_training_state(tc, models, device=dev, controlnet=dict(config=ccfg))
    H, W = batch["pixel_values"].shape[2:]
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    cbatch = dict(batch, conditioning_pixel_values=torch.rand(B, 3, H, W, device=dev, generator=g))
    step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
    ms, ips, loss = time_steps(step, (us, ts, ue, te, vae, sched), cbatch, B)
    res["controlnet"] = {"ms_per_step": round(ms, 3), "images_per_sec": round(ips, 2), "loss": loss,
                         "trained_params": sum(lf.numel for lf in us.controlnet.store.leaves.values())}
    print(f"{config}  controlnet: {ms:.2f} ms/step, {ips:.1f} images/sec, loss {loss:.4f}", flush=True)
    n, fwd, bwd = control_add_ms(cfgs["unet"], B, H // f, W // f)
    res["control_add"] = {"calls": n, "forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4),
                          "share_of_step": round((fwd + bwd) / ms, 4)}
    print(json.dumps(res), flush=True)
    del step, us, ts, ue, te, vae, sched, batch, cbatch
    torch.cuda.empty_cache()
