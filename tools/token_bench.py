"""Times the three new-token launches (include/sdt.h "NEW TOKENS") with events around back-to-back eager calls, at a text shape:
python tools/token_bench.py [--batch 4] [--seq 77] [--width 768] [--vocab 49408] [--tokens 4] [--iters 200]
Prints one JSON line (microseconds per launch).  The plain sdt_embedding_fwd at the same shape is timed beside the extended one."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stable_diffusion_training_amd import _lib


def timed(fn, iters):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    for name, default in (("batch", 4), ("seq", 77), ("width", 768), ("vocab", 49408), ("tokens", 4), ("iters", 200)):
        ap.add_argument("--" + name, type=int, default=default)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda:0")
    rows, S, D, V, n = args.batch * args.seq, args.seq, args.width, args.vocab, args.tokens
    g = torch.Generator().manual_seed(0)
    tok, ext, pos = (torch.randn(r, D, generator=g).mul_(0.02).to(dev) for r in (V, n, S))
    ids = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    ids[1::S] = V + torch.arange(args.batch, dtype=torch.int32) % n  # one placeholder per caption
    ids = ids.to(dev)
    out = torch.empty(rows, D, dtype=torch.bfloat16, device=dev)
    dout = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    dext = torch.empty(n, D, device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ids_plain = ids.clamp(max=V - 1)
    res = dict(rows=rows, D=D, n_ext=n,
               embedding_fwd_us=timed(lambda: _lib.call("sdt_embedding_fwd", ids_plain.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                                                        out.data_ptr(), rows, S, D, s), args.iters),
               ext_fwd_us=timed(lambda: _lib.call("sdt_embedding_ext_fwd", ids.data_ptr(), tok.data_ptr(), ext.data_ptr(), pos.data_ptr(),
                                                  out.data_ptr(), rows, S, D, V, n, s), args.iters),
               ext_bwd_us=timed(lambda: _lib.call("sdt_embedding_ext_bwd", ids.data_ptr(), dout.data_ptr(), dext.data_ptr(), rows, D, V, n, s),
                                args.iters),
               retract_us=timed(lambda: _lib.call("sdt_embedding_retract", ext.data_ptr(), n, D, 0.02, 0.1, stats.data_ptr(), s), args.iters))
    print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in res.items()}))
