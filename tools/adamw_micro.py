"""Developer tool: device time and HBM rate of sdt_adamw8_step beside sdt_lion8_step on a flat buffer of the SD1.5 UNet store's size
(859.5 M parameters, block 16, bf16 gradient, EMA and bf16 mirror on), the two sweeps alternated in one process (HIP events).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/adamw_micro.py` for the kernels' own durations.
--lib PATH: another build of the library (the parent commit's, say).  Its sdt_lion8_step, sdt_adamw8_step and sdt_adamw_select then run
on states of their own, alternated with this tree's in the same rounds, and both builds' figures are printed.
Bytes per parameter: g 2, p 4 + 4, ema 4 + 4, bf16 mirror 2, and codes 1 + 1, scales (4 + 4) / 16 - once for Lion (22.5 B), twice for
AdamW (25 B)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stable_diffusion_training_amd import _lib, params

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=859_520_000 // 2048 * 2048)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--lib", default=None)
args = ap.parse_args()
_lib.require_device()
NAMES = ("sdt_lion8_step", "sdt_adamw8_step", "sdt_adamw_select")
builds = {"tree": {nm: getattr(_lib.load(), nm) for nm in NAMES}}
if args.lib:
    alt = ctypes.CDLL(os.path.abspath(args.lib))
    builds["lib"] = {nm: getattr(alt, nm) for nm in NAMES}
    for nm, fn in builds["lib"].items():
        fn.argtypes, fn.restype = _lib.SIGNATURES[nm], ctypes.c_int
dev = torch.device("cuda", 0)
n, bs = args.n, 16
gen = torch.Generator(device=dev)
gen.manual_seed(0)
grads = [(torch.randn(n, device=dev, generator=gen) * 1e-3).to(torch.bfloat16) for _ in range(2)]
thr = params.lion_thresholds(dev)
sq = torch.tensor([float(grads[0].double().pow(2).sum())], dtype=torch.float64, device=dev)
s = torch.cuda.current_stream().cuda_stream
p0 = torch.randn(n, device=dev, generator=gen) * 0.05


def state(code0, two):
    st = dict(p=p0.clone(), ema=p0.clone(), w=torch.empty(n, dtype=torch.bfloat16, device=dev),
              codes=torch.full((n,), code0, dtype=torch.int8, device=dev), inv=torch.ones(n // bs, device=dev))
    if two:
        st.update(codes2=torch.zeros(n, dtype=torch.int8, device=dev), inv2=torch.ones(n // bs, device=dev),
                  step=torch.zeros(1, dtype=torch.int64, device=dev), prod=torch.ones(2, dtype=torch.float64, device=dev),
                  cur=torch.zeros(8, device=dev))
    return st


def lion_step(fns, L, k):
    rc = fns["sdt_lion8_step"](L["p"].data_ptr(), grads[k % 2].data_ptr(), 1, L["codes"].data_ptr(), L["inv"].data_ptr(), L["ema"].data_ptr(),
                               L["w"].data_ptr(), n, bs, sq.data_ptr(), thr.data_ptr(), 1.0, 1e-6 / 7, 7e-2, 0.9, 0.99, 0.9999, s)
    assert rc == 0


def adam_select(fns, A):
    rc = fns["sdt_adamw_select"](A["step"].data_ptr(), A["prod"].data_ptr(), None, 0, None, 0, 1e-6, 0.9999, 0.9, 0.999, A["cur"].data_ptr(), s)
    assert rc == 0


def adam_step(fns, A, k):
    rc = fns["sdt_adamw8_step"](A["p"].data_ptr(), grads[k % 2].data_ptr(), 1, A["codes"].data_ptr(), A["inv"].data_ptr(), A["codes2"].data_ptr(),
                                A["inv2"].data_ptr(), A["ema"].data_ptr(), A["w"].data_ptr(), n, bs, sq.data_ptr(), thr.data_ptr(), 1.0,
                                A["cur"].data_ptr(), 1e-2, 0.9, 0.999, 1e-8, s)
    assert rc == 0


# one (kernel, build) sweep after the other, each on a state of its own
runs = [(kernel, build, fns, state(3, False) if kernel == "lion8" else state(0, True))
        for kernel in ("lion8", "adamw8") for build, fns in builds.items()]
for k in range(3):  # every state leaves its initial codes behind
    for kernel, build, fns, st in runs:
        if kernel == "adamw8":
            adam_select(fns, st)
        (lion_step if kernel == "lion8" else adam_step)(fns, st, k)
torch.cuda.synchronize()
times = {(kernel, build): [] for kernel, build, _, _ in runs}
for k in range(args.rounds):
    for kernel, build, fns, st in runs:
        if kernel == "adamw8":  # the one-lane select is not part of the sweep's time
            adam_select(fns, st)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        (lion_step if kernel == "lion8" else adam_step)(fns, st, k)
        b.record()
        torch.cuda.synchronize()
        times[kernel, build].append(a.elapsed_time(b))
bpp = {"lion8": 2 + 8 + 8 + 2 + 2 + 8 / bs, "adamw8": 2 + 8 + 8 + 2 + 2 * (2 + 8 / bs)}
med = {k: statistics.median(v) for k, v in times.items()}
for (kernel, build), v in times.items():
    print(json.dumps(dict(kernel=kernel, build=args.lib if build == "lib" else "tree", params=n, median_ms=round(med[kernel, build], 4),
                          min_ms=round(min(v), 4), bytes_per_param=bpp[kernel],
                          tb_per_s=round(n * bpp[kernel] / med[kernel, build] / 1e9, 3))), flush=True)
finite = all(bool(torch.isfinite(st["p"]).all()) for _, _, _, st in runs)
print(json.dumps(dict(ratio_adamw8_over_lion8=round(med["adamw8", "tree"] / med["lion8", "tree"], 4),
                      byte_ratio=round(bpp["adamw8"] / bpp["lion8"], 4), finite=finite)), flush=True)
if args.lib:
    same = all(torch.equal(a[3][key], b[3][key]) for a, b in ((runs[0], runs[1]), (runs[2], runs[3])) for key in a[3])
    print(json.dumps(dict(tree_over_lib={kernel: round(med[kernel, "tree"] / med[kernel, "lib"], 4) for kernel in bpp},
                          states_bit_identical=same)), flush=True)
