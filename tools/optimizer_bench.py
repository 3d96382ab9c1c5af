"""Developer tool: the step time of the two optimizers on the SD1.5 512^2 batch-4 captured step (bench.py config sd15_512: 8-bit states,
EMA, one HIP graph per step).  Two sets of states in one process - Lion (bench.py's) and AdamW with 8-bit block-quantised moments - whose
captured steps are timed in alternating rounds, so clocks and box noise hit both alike.  Prints one JSON line per optimizer (median
ms/step over the rounds, images/sec), the difference, and each UNet store's optimizer-state bytes beside what fp32 Adam would hold.
usage: python tools/optimizer_bench.py [--steps 10] [--rounds 5]"""
import argparse
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
args = ap.parse_args()
C = bench.CONFIGS["sd15_512"]
B = C["batch"]
dev = torch.device("cuda", 0)


TC, CFGS, WEIGHTS, LION_STATES = bench.build_states(dev, B, config="sd15_512")


def build(optimizer):
    if optimizer == "lion":
        (us, ts, ue, te, vae, sched, _) = LION_STATES
    else:  # the same weights and config through the same entry point, with the optimizer keyword
        models = {"unet": {"unet_params": WEIGHTS["unet"], "config": CFGS["unet"]}, "vae": {"vae_params": WEIGHTS["vae"], "config": CFGS["vae"]},
                  "text_encoder": {"text_encoder_params": WEIGHTS["clip"], "config": CFGS["clip"]}}
        (us, ts, ue, te, vae, sched, _) = tu.on_device_model_training_state(TC, models, device=dev, optimizer=optimizer)
    tc = TC
    assert us.store.optimizer == optimizer and ts.store.optimizer == optimizer
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


runs = {name: build(name) for name in ("lion", "adamw")}
times = {k: [] for k in runs}
for _ in range(args.rounds):
    for name, (step, a) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step(*a)
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
res = {}
for name, ts_ in times.items():
    ms = statistics.median(ts_)
    res[name] = ms
    store = runs[name][1][0].store
    print(json.dumps(dict(optimizer=name, batch=B, image=C["image"], ms_per_step=round(ms, 3), images_per_sec=round(B / ms * 1e3, 3),
                          rounds=[round(t, 3) for t in ts_], loss=float(out[4]["loss"]) if name == "adamw" else None,
                          unet_params=store.total, unet_state_bytes=store.state_bytes(),
                          unet_state_bytes_per_param=round(store.state_bytes() / store.total, 4))), flush=True)
total = runs["adamw"][1][0].store.total
print(json.dumps(dict(delta_ms=round(res["adamw"] - res["lion"], 3), ratio=round(res["adamw"] / res["lion"], 4),
                      fp32_adam_state_bytes=8 * total, adamw_step_counter=int(runs["adamw"][1][0].store.adam_step.item()))), flush=True)
