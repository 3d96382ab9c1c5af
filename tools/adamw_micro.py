"""Developer tool: device time and HBM rate of sdt_adamw8_step beside sdt_lion8_step on a flat buffer of the SD1.5 UNet store's size
(859.5 M parameters, block 16, bf16 gradient, EMA and bf16 mirror on), the two sweeps alternated in one process (HIP events).  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/adamw_micro.py` for the kernels' own durations.
--lion-lib PATH times sdt_lion8_step of another build of the library (the parent commit's) instead of this tree's.
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
ap.add_argument("--lion-lib", default=None)
args = ap.parse_args()
_lib.require_device()
lion = _lib.load().sdt_lion8_step
if args.lion_lib:
    alt = ctypes.CDLL(os.path.abspath(args.lion_lib))
    lion = alt.sdt_lion8_step
    lion.argtypes, lion.restype = _lib.SIGNATURES["sdt_lion8_step"], ctypes.c_int
adam, select = _lib.load().sdt_adamw8_step, _lib.load().sdt_adamw_select
dev = torch.device("cuda", 0)
n, bs = args.n, 16
gen = torch.Generator(device=dev)
gen.manual_seed(0)
grads = [(torch.randn(n, device=dev, generator=gen) * 1e-3).to(torch.bfloat16) for _ in range(2)]
thr = params.lion_thresholds(dev)
sq = torch.tensor([float(grads[0].double().pow(2).sum())], dtype=torch.float64, device=dev)
s = torch.cuda.current_stream().cuda_stream


def state(code0, two):
    st = dict(p=torch.randn(n, device=dev, generator=gen) * 0.05, w=torch.empty(n, dtype=torch.bfloat16, device=dev),
              codes=torch.full((n,), code0, dtype=torch.int8, device=dev), inv=torch.ones(n // bs, device=dev))
    st["ema"] = st["p"].clone()
    if two:
        st.update(codes2=torch.zeros(n, dtype=torch.int8, device=dev), inv2=torch.ones(n // bs, device=dev),
                  step=torch.zeros(1, dtype=torch.int64, device=dev), prod=torch.ones(2, dtype=torch.float64, device=dev),
                  cur=torch.zeros(8, device=dev))
    return st


L, A = state(3, False), state(0, True)


def lion_step(k):
    rc = lion(L["p"].data_ptr(), grads[k % 2].data_ptr(), 1, L["codes"].data_ptr(), L["inv"].data_ptr(), L["ema"].data_ptr(), L["w"].data_ptr(), n,
              bs, sq.data_ptr(), thr.data_ptr(), 1.0, 1e-6 / 7, 7e-2, 0.9, 0.99, 0.9999, s)
    assert rc == 0


def adam_step(k):
    rc = select(A["step"].data_ptr(), A["prod"].data_ptr(), None, 0, None, 0, 1e-6, 0.9999, 0.9, 0.999, A["cur"].data_ptr(), s)
    assert rc == 0
    rc = adam(A["p"].data_ptr(), grads[k % 2].data_ptr(), 1, A["codes"].data_ptr(), A["inv"].data_ptr(), A["codes2"].data_ptr(), A["inv2"].data_ptr(),
              A["ema"].data_ptr(), A["w"].data_ptr(), n, bs, sq.data_ptr(), thr.data_ptr(), 1.0, A["cur"].data_ptr(), 1e-2, 0.9, 0.999, 1e-8, s)
    assert rc == 0


for k in range(3):  # both states leave their initial codes behind
    lion_step(k)
    adam_step(k)
torch.cuda.synchronize()
times = {"lion8": [], "adamw8": []}
for k in range(args.rounds):
    for name, fn in (("lion8", lion_step), ("adamw8", adam_step)):
        if name == "adamw8":  # the one-lane select is not part of the sweep's time
            select(A["step"].data_ptr(), A["prod"].data_ptr(), None, 0, None, 0, 1e-6, 0.9999, 0.9, 0.999, A["cur"].data_ptr(), s)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if name == "adamw8":
            rc = adam(A["p"].data_ptr(), grads[k % 2].data_ptr(), 1, A["codes"].data_ptr(), A["inv"].data_ptr(), A["codes2"].data_ptr(),
                      A["inv2"].data_ptr(), A["ema"].data_ptr(), A["w"].data_ptr(), n, bs, sq.data_ptr(), thr.data_ptr(), 1.0, A["cur"].data_ptr(),
                      1e-2, 0.9, 0.999, 1e-8, s)
            assert rc == 0
        else:
            fn(k)
        b.record()
        torch.cuda.synchronize()
        times[name].append(a.elapsed_time(b))
bpp = {"lion8": 2 + 8 + 8 + 2 + 2 + 8 / bs, "adamw8": 2 + 8 + 8 + 2 + 2 * (2 + 8 / bs)}
med = {k: statistics.median(v) for k, v in times.items()}
for name in times:
    print(json.dumps(dict(kernel=name, params=n, median_ms=round(med[name], 4), min_ms=round(min(times[name]), 4), bytes_per_param=bpp[name],
                          tb_per_s=round(n * bpp[name] / med[name] / 1e9, 3), lion_lib=args.lion_lib if name == "lion8" else None)), flush=True)
print(json.dumps(dict(ratio_adamw8_over_lion8=round(med["adamw8"] / med["lion8"], 4), byte_ratio=round(bpp["adamw8"] / bpp["lion8"], 4),
                      finite=bool(torch.isfinite(A["p"]).all()) and bool(torch.isfinite(L["p"]).all()))), flush=True)
