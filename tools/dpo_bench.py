"""Developer tool: the Diffusion-DPO step against the LoRA step (captured steps, one GPU, one session).
For a configuration of bench.py it builds two LoRA states on the same weights - rank 16, the default UNet targets, text encoder frozen -
and times the LoRA step at the configuration's batch (4 for sd15_512) against the DPO step on the same batch read as 2 pairs
(train_step dpo_beta=): three set-up calls each (two eager, capture + first replay), then --rounds rounds that ALTERNATE the two
variants, --steps graph replays per visit; the figure of a variant is the median over its visits, with the range.  The DPO step's three
own launches - sdt_lora_restore, the merge, sdt_dpo_loss_fwd_bwd (two kernels) - are timed by events around replays of a small graph
that holds --reps of them.  Expectation, not a threshold: DPO step = LoRA step + one UNet forward + well under 1 % for the three
launches.
usage: python tools/dpo_bench.py [--config sd15_512] [--steps 8] [--rounds 4] [--warmup 2] [--rank 16] [--beta 5000] [--dora]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import _lib, lora, ops
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=sorted(bench.CONFIGS), default="sd15_512")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--beta", type=float, default=5000.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--dora", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
c = bench.CONFIGS[args.config]
B = c["batch"]
if B % 2:
    raise SystemExit(f"{args.config}: batch {B} is odd; the DPO step needs whole pairs")
tc, cfgs, weights, full = bench.build_states(dev, B, config=args.config)
del full
torch.cuda.empty_cache()
models = {"unet": {"unet_params": weights["unet"], "config": cfgs["unet"]}, "vae": {"vae_params": weights["vae"], "config": cfgs["vae"]},
          "text_encoder": {"text_encoder_params": weights["clip"], "config": cfgs["clip"]}}
kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
batch = bench.synthetic_batch(dev, B, 0, args.config)


def build(extra):
    us, ts, ue, te, vae, sched, _ = tu.on_device_model_training_state(
        tc, models, device=dev, lora=dict(unet=lora.LoraConfig(args.rank, float(args.rank), dora=args.dora), text_encoder="frozen"))
    step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **extra, **k))
    rng = torch.Generator(device=dev)
    rng.manual_seed(1000)
    return dict(step=step, states=(us, ts, ue, te, vae, sched), rng=rng, ms=[], out=None)


def run(v, n):
    us, ts, ue, te, vae, sched = v["states"]
    for _ in range(n):
        v["out"] = v["step"](us, ts, ue, te, batch, v["rng"], vae, sched)


variants = {"lora": build({}), "dpo": build(dict(dpo_beta=args.beta))}
for v in variants.values():
    run(v, 3 + args.warmup)  # two eager set-up steps, capture + first replay, warm-up replays
    torch.cuda.synchronize()
    assert v["step"].graph is not None
for _ in range(args.rounds):
    for v in variants.values():  # alternating: both variants see the same minutes of the box
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(v, args.steps)
        torch.cuda.synchronize()
        v["ms"].append(1e3 * (time.perf_counter() - t0) / args.steps)
res = {"config": args.config, "batch": B, "pairs": B // 2, "rank": args.rank, "dora": args.dora, "beta": args.beta,
       "steps_per_visit": args.steps, "rounds": args.rounds}
for name, v in variants.items():
    med = statistics.median(v["ms"])
    res[name] = {"ms_per_step": round(med, 3), "min": round(min(v["ms"]), 3), "max": round(max(v["ms"]), 3),
                 "images_per_sec": round(B / med * 1e3, 2), "loss": float(v["out"][4]["loss"])}
    print(f"{args.config}  {name}: {med:.2f} ms/step ({min(v['ms']):.2f} - {max(v['ms']):.2f}), loss {res[name]['loss']:.5f}", flush=True)
res["dpo"]["implicit_acc"] = float(variants["dpo"]["out"][4]["implicit_acc"])
res["extra_ms"] = round(res["dpo"]["ms_per_step"] - res["lora"]["ms_per_step"], 3)


def graph_ms(fn, visits=5):
    """Per-call time of `fn` from events around replays of a graph that holds args.reps calls of it: median over `visits` replays."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(visits):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.reps)
    return statistics.median(times)


us = variants["dpo"]["states"][0]
ad = us.adapter
L = cfgs["vae"].get("latent_channels", 4)
h = w = c["image"] // 8
cpad = -(-L // 8) * 8
pred = torch.randn(B, h, w, cpad, device=dev).to(torch.bfloat16)
ref = torch.randn(B, h, w, cpad, device=dev).to(torch.bfloat16)
target = torch.randn(B, L, h, w, device=dev)
loss, mse = torch.zeros(1, device=dev), torch.empty(2, B, device=dev)
lg, pl, cf, dp = torch.empty(B // 2, device=dev), torch.empty(B // 2, device=dev), torch.empty(B, device=dev), torch.empty_like(pred)
rws = ops.reduce_workspace(_lib.load().sdt_dpo_loss_workspace_bytes(B, h, w), dev)


def dpo_loss():
    _lib.call("sdt_dpo_loss_fwd_bwd", pred.data_ptr(), ref.data_ptr(), target.data_ptr(), args.beta, loss.data_ptr(), mse.data_ptr(),
              lg.data_ptr(), pl.data_ptr(), cf.data_ptr(), dp.data_ptr(), B, L, h, w, cpad, rws.data_ptr(), rws.numel(),
              torch.cuda.current_stream().cuda_stream)


res["launches"] = {"restore_ms": round(graph_ms(ad.restore), 4), "merge_ms": round(graph_ms(lambda: ad.merge("master")), 4),
                   "dpo_loss_ms": round(graph_ms(dpo_loss), 4)}
three = sum(res["launches"].values())
res["launches"]["share_of_dpo_step"] = round(three / res["dpo"]["ms_per_step"], 5)
print(json.dumps(res), flush=True)
