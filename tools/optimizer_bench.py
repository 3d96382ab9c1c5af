"""Developer tool: the step time of the optimizers on the SD1.5 512^2 batch-4 captured step (bench.py config sd15_512: EMA, one HIP graph
per step).  One set of states per row in one process - by default lion (bench.py's, 8-bit momentum) and adamw (8-bit block-quantised
moments); --optimizers also takes adamw32 (the same config with the quantisation switches off: fp32 moments) and prodigy (fp32 m, v, s,
p0; two sweeps) - whose captured steps are timed in alternating rounds, so clocks and box noise hit all alike.  Prints one JSON line per
row (median ms/step over the rounds, images/sec, the UNet store's optimizer-state bytes) and a last line: with lion and adamw among the
rows their difference as before (delta_ms, ratio, fp32_adam_state_bytes, adamw_step_counter); with other rows also "against_first", the
difference and ratio of every row to the first one named (the Prodigy row against its AdamW-fp32 yardstick: --optimizers adamw32 prodigy).
usage: python tools/optimizer_bench.py [--steps 10] [--rounds 5] [--optimizers lion adamw | adamw32 prodigy | ...]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--optimizers", nargs="+", choices=("lion", "adamw", "adamw32", "prodigy"), default=["lion", "adamw"])
args = ap.parse_args()
C = bench.CONFIGS["sd15_512"]
B = C["batch"]
dev = torch.device("cuda", 0)


TC, CFGS, WEIGHTS, LION_STATES = bench.build_states(dev, B, config="sd15_512")


def build(optimizer):
    tc, name = TC, optimizer
    if optimizer == "lion":
        (us, ts, ue, te, vae, sched, _) = LION_STATES
    else:  # the same weights and config through the same entry point, with the optimizer keyword
        models = {"unet": {"unet_params": WEIGHTS["unet"], "config": CFGS["unet"]}, "vae": {"vae_params": WEIGHTS["vae"], "config": CFGS["vae"]},
                  "text_encoder": {"text_encoder_params": WEIGHTS["clip"], "config": CFGS["clip"]}}
        if optimizer == "adamw32":
            tc, name = dataclasses.replace(TC, quantize_unet_state=False, quantize_text_encoder_state=False), "adamw"
        (us, ts, ue, te, vae, sched, _) = tu.on_device_model_training_state(tc, models, device=dev, optimizer=name)
    assert us.store.optimizer == name and ts.store.optimizer == name
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=C["vae_scale"])
    step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
    rng = torch.Generator(device=dev)
    rng.manual_seed(2)
    batch = bench.synthetic_batch(dev, B, 0, "sd15_512")
    args_ = (us, ts, ue, te, batch, rng, vae, sched)
    for _ in range(3):  # two eager warm-ups, capture + first replay
        step(*args_)
    torch.cuda.synchronize()
    assert step.graph is not None
    return step, args_


runs = {name: build(name) for name in args.optimizers}
times = {k: [] for k in runs}
losses = {}
for _ in range(args.rounds):
    for name, (step, a) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step(*a)
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        losses[name] = float(out[4]["loss"])
res = {}
for name, ts_ in times.items():
    ms = statistics.median(ts_)
    res[name] = ms
    store = runs[name][1][0].store
    print(json.dumps(dict(optimizer=name, batch=B, image=C["image"], ms_per_step=round(ms, 3), images_per_sec=round(B / ms * 1e3, 3),
                          rounds=[round(t, 3) for t in ts_], loss=None if name == "lion" else losses[name],
                          unet_params=store.total, unet_state_bytes=store.state_bytes(),
                          unet_state_bytes_per_param=round(store.state_bytes() / store.total, 4))), flush=True)
last = dict(fp32_adam_state_bytes=8 * next(iter(runs.values()))[1][0].store.total)
if "lion" in runs and "adamw" in runs:
    last.update(delta_ms=round(res["adamw"] - res["lion"], 3), ratio=round(res["adamw"] / res["lion"], 4),
                adamw_step_counter=int(runs["adamw"][1][0].store.adam_step.item()))
if set(runs) - {"lion", "adamw"}:
    first = args.optimizers[0]
    last["against_first"] = {k: dict(first=first, delta_ms=round(v - res[first], 3), ratio=round(v / res[first], 4))
                             for k, v in res.items() if k != first}
if "prodigy" in runs:
    last["prodigy_d"] = float(runs["prodigy"][1][0].store.prodigy_d().item())
print(json.dumps(last), flush=True)
