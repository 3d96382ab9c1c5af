"""Developer tool: the full fine-tune step against the LoRA step (captured steps, one GPU).
For each configuration of bench.py it times the step bench.py times (bench.build_states' states) and the LoRA step on the same weights
and batch - rank 16, the default UNet targets, text encoder frozen - as tools/latent_cache_bench.py does: three set-up calls (two eager,
capture + first replay), then timed graph replays.  The adapter's two launches (merge, project) and its optimizer step are timed by
events around eager calls.
--dora times the DoRA step (LoraConfig(dora=True): the column-stripe merge and the projection with the magnitude gradient) in its place.
--optimizer names the adapter store's optimizer; several names time one LoRA step each on the same base, in the order given (a name given
twice shows the run-to-run spread of the session: "adamw adamw prodigy").  --skip-full leaves the full fine-tune step out.
--conv-rank R times LoCon (LoraConfig(conv_rank=R): the attention adapters plus every conv target at rank R) in one session with the
variants alternating: per round, --steps graph replays each of the attention-only LoRA step, the LoCon step and the full fine-tune step
between events; then, on the LoCon adapter's convolution table, the split projection (sdt_lora_project_split) against sdt_lora_project on
the same table, alternating per round.  It prints medians and ranges over --rounds rounds, the merge / restore / project times and the
scratch and workspace bytes.
--algo loha times LoHa (LoraConfig(algo="loha")) against the step it extends, in one session with the variants alternating per round:
the attention-only LoHa step against the LoRA step, or with --conv-rank R the LoHa step on attention and convolutions against the LoCon
step; then merge / restore / project of both adapters by events, alternating per round, and the scratch and workspace bytes.
usage: python tools/lora_bench.py [--config sd15_512 sd21_768 sdxl_1024] [--steps 8] [--warmup 2] [--rank 16] [--dora]
                                  [--optimizer lion adamw prodigy] [--skip-full] [--conv-rank R [--rounds 7]] [--algo loha]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import _lib, lora
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--config", nargs="+", choices=sorted(bench.CONFIGS), default=sorted(bench.CONFIGS))
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--dora", action="store_true")
ap.add_argument("--optimizer", nargs="+", choices=("lion", "adamw", "prodigy"), default=["lion"])
ap.add_argument("--skip-full", action="store_true")
ap.add_argument("--conv-rank", type=int, default=0)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--algo", choices=lora.ALGOS, default="lora")
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


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def locon_session(config):
    """--conv-rank: attention-only LoRA, LoCon and the full fine-tune in one session, alternating; then the projection A/B."""
    c = bench.CONFIGS[config]
    B = c["batch"]
    tc, cfgs, weights, full = bench.build_states(dev, B, config=config)
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
    batch = bench.synthetic_batch(dev, B, 0, config)
    models = {"unet": {"unet_params": weights["unet"], "config": cfgs["unet"]}, "vae": {"vae_params": weights["vae"], "config": cfgs["vae"]},
              "text_encoder": {"text_encoder_params": weights["clip"], "config": cfgs["clip"]}}
    r = args.rank
    variants = {}
    for name, cfg in (("lora", lora.LoraConfig(r, float(r))), ("locon", lora.LoraConfig(r, float(r), conv_rank=args.conv_rank))):
        variants[name] = tu.on_device_model_training_state(tc, models, device=dev, optimizer=args.optimizer[0],
                                                           lora=dict(unet=cfg, text_encoder="frozen"))[:6]
    if not args.skip_full:
        variants["full"] = full[:6]
    steps, rngs = {}, {}
    for name, st in variants.items():  # two eager set-up steps, capture + first replay, warm-up replays
        steps[name] = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
        rngs[name] = torch.Generator(device=dev)
        rngs[name].manual_seed(1000)
        for _ in range(3 + args.warmup):
            out = steps[name](st[0], st[1], st[2], st[3], batch, rngs[name], st[4], st[5])
        torch.cuda.synchronize()
        assert steps[name].graph is not None
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, st in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                steps[name](st[0], st[1], st[2], st[3], batch, rngs[name], st[4], st[5])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    res = {"config": config, "batch": B, "rank": r, "conv_rank": args.conv_rank, "rounds": args.rounds, "steps_per_round": args.steps,
           "step_ms": {name: spread(t) for name, t in times.items()}}
    ad = variants["locon"][0].adapter
    stream = torch.cuda.current_stream().cuda_stream
    n = len(ad.conv_jobs_host)

    def split():
        _lib.call("sdt_lora_project_split", ad.scratch.data_ptr(), ad.store.master.data_ptr(), ad.store.grad.data_ptr(), ad.conv_jobs_host,
                  ad.split_host, ad.conv_jobs_dev.data_ptr(), ad.split_dev.data_ptr(), n, ad.split_ws.data_ptr(), ad.split_ws.numel(), stream)

    def parent():
        _lib.call("sdt_lora_project", ad.scratch.data_ptr(), ad.store.master.data_ptr(), ad.store.grad.data_ptr(), ad.conv_jobs_host,
                  ad.conv_jobs_dev.data_ptr(), n, stream)

    ab = {"split": [], "sdt_lora_project": []}
    for _ in range(args.rounds):
        ab["split"].append(event_ms(split))
        ab["sdt_lora_project"].append(event_ms(parent))
    res["project_conv_table_ms"] = {k: spread(v) for k, v in ab.items()}
    res["project_conv_table_ms"]["jobs"] = n
    res["project_conv_table_ms"]["dw_bytes"] = 2 * sum(j.K * j.N for j in ad.conv_jobs_host)
    base = variants["lora"][0].adapter
    res["adapter"] = {name: {"leaves": len(a.paths), "conv_leaves": len(a.conv_paths),
                             "adapted_params": sum(a.base.leaves[p].numel for p in a.paths),
                             "trained_params": sum(lf.numel for lf in a.store.leaves.values()), "scratch_bytes": 2 * a.scratch.numel(),
                             "workspace_bytes": 0 if a.split_ws is None else a.split_ws.numel(),
                             "merge_ms": round(event_ms(a.merge), 4), "restore_ms": round(event_ms(a.restore), 4),
                             "project_ms": round(event_ms(a.project), 4)} for name, a in (("lora", base), ("locon", ad))}
    print(json.dumps(res), flush=True)


def loha_session(config):
    """--algo loha: the LoRA (with --conv-rank: LoCon) step and the LoHa step on the same leaves in one session, alternating."""
    c = bench.CONFIGS[config]
    B = c["batch"]
    tc, cfgs, weights, full = bench.build_states(dev, B, config=config)
    del full
    torch.cuda.empty_cache()
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
    batch = bench.synthetic_batch(dev, B, 0, config)
    models = {"unet": {"unet_params": weights["unet"], "config": cfgs["unet"]}, "vae": {"vae_params": weights["vae"], "config": cfgs["vae"]},
              "text_encoder": {"text_encoder_params": weights["clip"], "config": cfgs["clip"]}}
    r, parent = args.rank, "locon" if args.conv_rank else "lora"
    variants = {}
    for name, cfg in ((parent, lora.LoraConfig(r, float(r), conv_rank=args.conv_rank)),
                      ("loha", lora.LoraConfig(r, float(r), conv_rank=args.conv_rank, algo="loha"))):
        variants[name] = tu.on_device_model_training_state(tc, models, device=dev, optimizer=args.optimizer[0],
                                                           lora=dict(unet=cfg, text_encoder="frozen"))[:6]
    steps, rngs = {}, {}
    for name, st in variants.items():  # two eager set-up steps, capture + first replay, warm-up replays
        steps[name] = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
        rngs[name] = torch.Generator(device=dev)
        rngs[name].manual_seed(1000)
        for _ in range(3 + args.warmup):
            steps[name](st[0], st[1], st[2], st[3], batch, rngs[name], st[4], st[5])
        torch.cuda.synchronize()
        assert steps[name].graph is not None
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, st in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                steps[name](st[0], st[1], st[2], st[3], batch, rngs[name], st[4], st[5])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    res = {"config": config, "batch": B, "rank": r, "conv_rank": args.conv_rank, "rounds": args.rounds, "steps_per_round": args.steps,
           "step_ms": {name: spread(t) for name, t in times.items()}}
    launches = {name: {"merge_ms": [], "restore_ms": [], "project_ms": []} for name in variants}
    for _ in range(args.rounds):
        for name, st in variants.items():
            a = st[0].adapter
            for what, fn in (("merge_ms", a.merge), ("restore_ms", a.restore), ("project_ms", a.project)):
                launches[name][what].append(event_ms(fn))
    res["adapter"] = {}
    for name, st in variants.items():
        a = st[0].adapter
        ws = sum(t[6].numel() for t in a.loha) if a.loha else 0 if a.split_ws is None else a.split_ws.numel()
        res["adapter"][name] = dict({"leaves": len(a.paths), "conv_leaves": len(a.conv_paths),
                                     "adapted_params": sum(a.base.leaves[p].numel for p in a.paths),
                                     "trained_params": sum(lf.numel for lf in a.store.leaves.values()), "scratch_bytes": 2 * a.scratch.numel(),
                                     "workspace_bytes": ws}, **{k: spread(v) for k, v in launches[name].items()})
    print(json.dumps(res), flush=True)


if args.algo == "loha":
    if args.dora:
        ap.error("--algo loha is refused beside --dora")
    for config in args.config:
        loha_session(config)
        torch.cuda.empty_cache()
    sys.exit(0)

if args.conv_rank:
    for config in args.config:
        locon_session(config)
        torch.cuda.empty_cache()
    sys.exit(0)

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
                          "restore_ms": round(event_ms(ad.restore), 4), "project_ms": round(event_ms(ad.project), 4)}
        ad.merge()  # (the mirror the step expects, after the timed restore)

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
