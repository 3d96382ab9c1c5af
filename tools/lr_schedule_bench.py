"""Developer tool: the cost of a learning-rate / EMA schedule on the SD1.5 512^2 batch-4 captured step (bench.py config sd15_512:
Lion-8bit, EMA, one HIP graph per step).  Two sets of states in one process: one without a schedule (the by-value sweeps) and one
with cosine + a 500-step warmup and the EMA warmup installed (ParamStore.set_schedule: one sdt_opt_schedule_select launch per store and
step, the _scheduled sweeps).  The two captured steps are timed in alternating rounds, so clocks and box noise hit both alike.
Prints one JSON line per mode (median ms/step over the rounds, images/sec) and the difference.
usage: python tools/lr_schedule_bench.py [--steps 10] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import lr_schedule as L
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
C = bench.CONFIGS["sd15_512"]
B = C["batch"]
dev = torch.device("cuda", 0)


def build(scheduled):
    tc, cfgs, _, (us, ts, ue, te, vae, sched, _) = bench.build_states(dev, B, config="sd15_512")
    if scheduled:
        for st in (us, ts):
            st.store.set_schedule(lr=L.LRSchedule("cosine", st.hyper["lr"], num_warmup_steps=500, num_training_steps=100000),
                                  ema=L.EMASchedule("warmup", tc.ema_rate))
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


runs = {"none": build(False), "cosine_ema_warmup": build(True)}
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
    print(json.dumps(dict(mode=name, batch=B, image=C["image"], ms_per_step=round(ms, 3), images_per_sec=round(B / ms * 1e3, 3),
                          rounds=[round(t, 3) for t in ts_])), flush=True)
us = runs["cosine_ema_warmup"][1][0].store
print(json.dumps(dict(delta_ms=round(res["cosine_ema_warmup"] - res["none"], 3), scheduled_step_counter=int(us._sched["step"].item()),
                      host_count=us.count)), flush=True)
