"""Developer tool: the full fine-tune step against the LoRA step (captured steps, one GPU).
For each configuration of bench.py it times the step bench.py times (bench.build_states' states) and the LoRA step on the same weights
and batch - rank 16, the default UNet targets, text encoder frozen - as tools/latent_cache_bench.py does: three set-up calls (two eager,
capture + first replay), then timed graph replays.  The adapter's two launches (merge, project) and its optimizer step are timed by
events around eager calls.
--dora times the DoRA step (LoraConfig(dora=True): the column-stripe merge and the projection with the magnitude gradient) in its place.
--optimizer names the adapter store's optimizer; several names time one LoRA step each on the same base, in the order given (a name given
twice shows the run-to-run spread of the session: "adamw adamw prodigy").  --skip-full leaves the full fine-tune step out.
usage: python tools/lora_bench.py [--config sd15_512 sd21_768 sdxl_1024] [--steps 8] [--warmup 2] [--rank 16] [--dora]
                                  [--optimizer lion adamw prodigy] [--skip-full]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import lora
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--config", nargs="+", choices=sorted(bench.CONFIGS), default=sorted(bench.CONFIGS))
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--dora", action="store_true")
ap.add_argument("--optimizer", nargs="+", choices=("lion", "adamw", "prodigy"), default=["lion"])
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


for config in args.config:
    c = bench.CONFIGS[config]
    B = c["batch"]
    tc, cfgs, weights, (us, ts, ue, te, vae, sched, _) = bench.build_states(dev, B, config=config)
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
    batch = bench.synthetic_batch(dev, B, 0, config)
    res = {"config": config, "batch": B, "rank": args.rank, "dora": args.dora}
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
    for optimizer in args.optimizer:
        res["optimizer"] = optimizer
        us, ts, ue, te, vae, sched, _ = tu.on_device_model_training_state(
            tc, models, device=dev, optimizer=optimizer,
            lora=dict(unet=lora.LoraConfig(args.rank, float(args.rank), dora=args.dora), text_encoder="frozen"))
        ad = us.adapter
        step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
        ms, ips, loss = time_steps(step, (us, ts, ue, te, vae, sched), batch, B)
        res["lora"] = {"ms_per_step": round(ms, 3), "images_per_sec": round(ips, 2), "loss": loss}
        print(f"{config}  {'dora' if args.dora else 'lora'} ({optimizer}): {ms:.2f} ms/step, {ips:.1f} images/sec, loss {loss:.4f}", flush=True)
        adapted = sum(us.store.leaves[p].numel for p in ad.paths)
        res["adapter"] = {"leaves": len(ad.paths), "adapted_params": adapted, "trained_params": sum(lf.numel for lf in ad.store.leaves.values()),
                          "scratch_bytes": 2 * ad.scratch.numel(), "merge_ms": round(event_ms(ad.merge), 4),
                          "project_ms": round(event_ms(ad.project), 4)}

        def opt():
            ad.store.zero_grad()
            ad.store.optimizer_step(ema_rate=tc.ema_rate if ue is not None else 0.0, **us.hyper)

        res["adapter"]["optimizer_ms"] = round(event_ms(opt), 4)
        if "full" in res:
            res["saved_ms"] = round(res["full"]["ms_per_step"] - res["lora"]["ms_per_step"], 3)
        print(json.dumps(res), flush=True)
        del step, us, ts, ue, te, vae, sched, ad
        torch.cuda.empty_cache()
    del batch
