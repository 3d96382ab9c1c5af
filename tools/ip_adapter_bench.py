"""Developer tool: the IP-Adapter's fused image-token attention against the composition it replaces, and the IP-Adapter step.
1. Kernels.  Over the attn2 shapes of one UNet pass (bench.py's configuration, its batch), for T = 4 and T = 16 image tokens:
   fused        sdt_ip_attention_fwd on the text attention's output, sdt_ip_attention_bwd with dq_in (what ops.attention_ip adds to the
                text attention's launches)
   composition  the existing attention at Nk = T (ops.attention_packed forward / backward), torch's scaled add into the text output
                and the add of the two dQ
   each variant's pass over all shapes is captured into a HIP graph; the replays are timed by device events, the variants alternating
   in one session, `--rounds` times: the median and the spread (max - min) of each are reported.
2. Steps.  ms/step of the full fine-tune step (the step bench.py times) and of the IP-Adapter step on the same weights and batch
   (captured steps), and the fused launches' share of the latter.
usage: python tools/ip_adapter_bench.py [--config sd15_512] [--rounds 7] [--steps 32] [--skip-steps]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from stable_diffusion_training_amd import _lib, nets, ops
from stable_diffusion_training_amd import training_utils as tu

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=sorted(bench.CONFIGS), default="sd15_512")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--replays", type=int, default=20)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--skip-steps", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
BF = torch.bfloat16


def attn2_shapes(cfg, B, h, w):
    """(B, heads, Nq, D) of every attn2 call of one UNet pass, in forward order."""
    boc = cfg["block_out_channels"]
    nb, lpb = len(boc), cfg["layers_per_block"]
    heads = nets._per_block(cfg["attention_head_dim"], nb)
    depth = nets._per_block(cfg["transformer_layers_per_block"], nb)
    out, hw = [], [(h, w)]
    for i, t in enumerate(cfg["down_block_types"]):
        if t == "CrossAttnDownBlock2D":
            out += [(B, heads[i], hw[-1][0] * hw[-1][1], boc[i] // heads[i])] * (lpb * depth[i])
        if i != nb - 1:
            hw.append(((hw[-1][0] - 1) // 2 + 1, (hw[-1][1] - 1) // 2 + 1))
    out += [(B, heads[-1], hw[-1][0] * hw[-1][1], boc[-1] // heads[-1])] * depth[-1]
    for i, t in enumerate(cfg["up_block_types"]):
        j = nb - 1 - i
        if t == "CrossAttnUpBlock2D":
            out += [(B, heads[j], hw[j][0] * hw[j][1], boc[j] // heads[j])] * ((lpb + 1) * depth[j])
    return out


def graphed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def event_ms(g, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernel_variants(shapes, T):
    """Four graphs - fused forward, fused backward, composition forward, composition backward - over all shapes, random operands."""
    stream = lambda: torch.cuda.current_stream().cuda_stream  # (read at call time: a capture runs on a stream of its own)
    lib = _lib.load()
    r = lambda *s: torch.randn(*s, device=dev).to(BF)
    data = []
    for B, H, Nq, D in shapes:
        C = H * D
        need = lib.sdt_ip_attention_bwd_workspace_bytes(B, H, Nq, T, D)
        data.append(dict(dims=(B, H, Nq, T, D), C=C, scale=D ** -0.5, q=r(B, Nq, C), kv=r(B, T, 2 * C), o_txt=r(B, Nq, C), dout=r(B, Nq, C),
                         dq_txt=r(B, Nq, C), out=torch.empty(B, Nq, C, dtype=BF, device=dev), dq=torch.empty(B, Nq, C, dtype=BF, device=dev),
                         dkv=torch.empty(B, T, 2 * C, dtype=BF, device=dev),
                         c_out=torch.empty(B, Nq, C, dtype=BF, device=dev), c_dq=torch.empty(B, Nq, C, dtype=BF, device=dev), ws=torch.zeros(need, dtype=torch.uint8, device=dev), need=need))

    def fused_fwd():
        for d in data:
            B, H, Nq, T_, D = d["dims"]
            _lib.call("sdt_ip_attention_fwd", d["q"].data_ptr(), d["kv"].data_ptr(), d["o_txt"].data_ptr(), None, d["out"].data_ptr(), B, H, Nq,
                      T_, D, d["C"], 2 * d["C"], d["scale"], stream())

    def fused_bwd():
        for d in data:
            B, H, Nq, T_, D = d["dims"]
            _lib.call("sdt_ip_attention_bwd", d["q"].data_ptr(), d["kv"].data_ptr(), d["dout"].data_ptr(), None, d["dq_txt"].data_ptr(),
                      d["dq"].data_ptr(), d["dkv"].data_ptr(), B, H, Nq, T_, D, d["C"], 2 * d["C"], 2 * d["C"], d["scale"], d["ws"].data_ptr(),
                      d["need"], stream())

    tapes = []

    def comp_fwd():
        tapes.clear()
        for d in data:
            q, kv = d["q"].detach().requires_grad_(True), d["kv"].detach().requires_grad_(True)
            o = ops.attention_packed(q, kv, d["dims"][1], d["scale"])
            # the scaled add into the text attention's output.  Every variant writes buffers of its OWN that stay bound for the life of the
            # graphs: a captured graph holds raw pointers, and torch.cuda.graph() empties the allocator's cache on entry, so a buffer that
            # is rebound (freed) after another graph captured it is unmapped by the next capture and that graph's replays fault
            torch.add(d["o_txt"], o.detach(), alpha=1.0, out=d["c_out"])
            tapes.append((o, q, kv))

    def comp_bwd():
        for d, (o, q, kv) in zip(data, tapes):
            q.grad = kv.grad = None
            o.backward(d["dout"], retain_graph=True)
            torch.add(d["dq_txt"], q.grad, out=d["c_dq"])             # q's two consumers

    comp_fwd()
    return dict(fused_fwd=graphed(fused_fwd), fused_bwd=graphed(fused_bwd), comp_fwd=graphed(comp_fwd), comp_bwd=graphed(comp_bwd))


def time_steps(step, states, batch, B):
    us, ts, ue, te, vae, sched = states
    rng = torch.Generator(device=dev)
    rng.manual_seed(1000)
    for _ in range(3 + args.warmup):
        out = step(us, ts, ue, te, batch, rng, vae, sched)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step(us, ts, ue, te, batch, rng, vae, sched)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    assert step.graph is not None
    return 1e3 * dt, B / dt, float(out[4]["loss"])


c = bench.CONFIGS[args.config]
B = c["batch"]
tc, cfgs, weights, states = bench.build_states(dev, B, config=args.config)
batch = bench.synthetic_batch(dev, B, 0, args.config)
f = 2 ** (len(cfgs["vae"]["block_out_channels"]) - 1)
H, W = batch["pixel_values"].shape[2:]
shapes = attn2_shapes(cfgs["unet"], B, H // f, W // f)
res = {"config": args.config, "batch": B, "attn2_calls": len(shapes), "kernels": {}}
fused_total = {}
for T in (4, 16):
    graphs = kernel_variants(shapes, T)
    times = {k: [] for k in graphs}
    for _ in range(args.rounds):  # the variants alternate inside every round
        for k, g in graphs.items():
            times[k].append(event_ms(g, args.replays))
    row = {k: {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)} for k, v in times.items()}
    med = lambda k: statistics.median(times[k])
    row["fused_sum_ms"] = round(med("fused_fwd") + med("fused_bwd"), 4)
    row["composition_sum_ms"] = round(med("comp_fwd") + med("comp_bwd"), 4)
    res["kernels"][f"T={T}"] = row
    fused_total[T] = med("fused_fwd") + med("fused_bwd")
    print(f"{args.config} T={T}: fused {row['fused_sum_ms']} ms, composition {row['composition_sum_ms']} ms over {len(shapes)} attn2 calls", flush=True)
    del graphs

if not args.skip_steps:
    kw = dict(strip_bos_eos_token=False, ema_rate=tc.ema_rate, vae_scale=c["vae_scale"])
    us, ts, ue, te, vae, sched, _ = states
    step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
    ms, ips, loss = time_steps(step, (us, ts, ue, te, vae, sched), batch, B)
    res["full"] = {"ms_per_step": round(ms, 3), "images_per_sec": round(ips, 2), "loss": loss}
    print(f"{args.config}  full: {ms:.2f} ms/step, {ips:.1f} images/sec", flush=True)
    del step, us, ts, ue, te, vae, sched, states
    torch.cuda.empty_cache()
    models = {"unet": {"unet_params": weights["unet"], "config": cfgs["unet"]}, "vae": {"vae_params": weights["vae"], "config": cfgs["vae"]},
              "text_encoder": {"text_encoder_params": weights["clip"], "config": cfgs["clip"]}}
    icfg = nets.ip_adapter_config(cfgs["unet"], 1024, 4)
    us, ts, ue, te, vae, sched, _ = tu.on_device_model_training_state(tc, models, device=dev, ip_adapter=dict(config=icfg))
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    ibatch = dict(batch, image_embeds=torch.randn(B, 1024, device=dev, generator=g))
    step = tu._GraphedStep(lambda *a, **k: tu.train_step(*a, **kw, **k))
    ms, ips, loss = time_steps(step, (us, ts, ue, te, vae, sched), ibatch, B)
    res["ip_adapter"] = {"ms_per_step": round(ms, 3), "images_per_sec": round(ips, 2), "loss": loss,
                         "trained_params": sum(lf.numel for lf in us.ip_adapter.store.leaves.values()),
                         "fused_share_of_step": round(fused_total[4] / ms, 4)}
    print(f"{args.config}  ip-adapter: {ms:.2f} ms/step, {ips:.1f} images/sec", flush=True)
print(json.dumps(res), flush=True)
