"""Scheduled learning rate and EMA rate on the MI355X (ParamStore.set_schedule, sdt_opt_schedule_select, the _scheduled Lion sweeps):
bit-exactness against the by-value sweeps and against steps whose rates are set by hand, graph replay of the schedule, micro-batches,
resume, the optimizer facade, the oracle trajectory and two data-parallel ranks."""
import dataclasses
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from stable_diffusion_training_amd import lr_schedule as L
from tests.helpers import build_hip_states, make_case, to_dev

pytestmark = pytest.mark.gpu

STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")
LR_SCHED = dict(num_warmup_steps=2, num_training_steps=6)  # a 2-step warmup, then cosine to step 6
EMA_SCHED = dict(kind="warmup")
EMA_RATE = 0.999


def _cur(lr, r, dev):
    return torch.from_numpy(np.array([np.float32(-lr), np.float32(r), np.float32(1.0 - r), 0.0], dtype=np.float32)).to(dev)


@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("g16", [0, 1])
def test_scheduled_lion8_sweep_equals_the_by_value_sweep(dev, bs, g16):
    from stable_diffusion_training_amd import _lib, lion_codec
    n = 64 * 1024 + 3 * bs
    g = torch.Generator(device=dev).manual_seed(bs + g16)
    thr = torch.from_numpy(lion_codec.quantization_thresholds().copy()).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    for lr, r in ((1e-4, 0.999), (0.0, 0.0), (3.3e-7, 0.18181818181818182), (1e-6 / 7, 0.99998)):
        p0 = torch.randn(n, device=dev, generator=g) * 0.05
        grad = torch.randn(n, device=dev, generator=g) * 1e-2
        gbuf = grad.to(torch.bfloat16) if g16 else grad
        mom = torch.randn(n, device=dev, generator=g) * 1e-3
        codes0 = torch.empty(n, dtype=torch.int8, device=dev)
        inv0 = torch.empty(n // bs, dtype=torch.float32, device=dev)
        _lib.call("sdt_lion8_quantize", mom.data_ptr(), codes0.data_ptr(), inv0.data_ptr(), n, bs, thr.data_ptr(), s)
        ema0 = torch.randn(n, device=dev, generator=g) * 0.05
        sq = (grad.double() ** 2).sum().reshape(1) * 4  # a norm above 1: the clip is applied
        outs = []
        for sched in (False, True):
            p, codes, inv, ema = p0.clone(), codes0.clone(), inv0.clone(), ema0.clone()
            w = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            head = (p.data_ptr(), gbuf.data_ptr(), g16, codes.data_ptr(), inv.data_ptr(), ema.data_ptr(), w.data_ptr(), n, bs,
                    sq.data_ptr(), thr.data_ptr(), 1.0)
            if sched:
                cur = _cur(lr, r, dev)
                _lib.call("sdt_lion8_step_scheduled", *head, cur.data_ptr(), 0.07, 0.9, 0.99, s)
            else:
                _lib.call("sdt_lion8_step", *head, lr, 0.07, 0.9, 0.99, r, s)
            torch.cuda.synchronize()
            outs.append((p, codes, inv, ema, w.view(torch.int16)))
        for name, a, b in zip(("master", "codes", "inv_scale", "ema", "bf16 mirror"), *outs):
            assert torch.equal(a, b), f"{name} differs (lr={lr}, r={r})"
        if lr == 0.0:
            assert torch.equal(outs[1][0], p0) and torch.equal(outs[1][3], p0)  # lr 0: masters unchanged; r 0: EMA := params


def test_scheduled_lion32_sweep_equals_the_by_value_sweep(dev):
    from stable_diffusion_training_amd import _lib
    n = 50 * 1024 + 5
    g = torch.Generator(device=dev).manual_seed(5)
    s = torch.cuda.current_stream().cuda_stream
    for lr, r in ((1e-4, 0.999), (0.0, 0.0), (2.5e-5, 0.37003947505256), (1e-6 / 7, 0.99998)):
        p0, grad = torch.randn(n, device=dev, generator=g) * 0.05, torch.randn(n, device=dev, generator=g) * 1e-2
        mom0, ema0 = torch.randn(n, device=dev, generator=g) * 1e-3, torch.randn(n, device=dev, generator=g) * 0.05
        sq = (grad.double() ** 2).sum().reshape(1) * 4
        outs = []
        for sched in (False, True):
            p, mom, ema = p0.clone(), mom0.clone(), ema0.clone()
            w = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            head = (p.data_ptr(), grad.data_ptr(), mom.data_ptr(), ema.data_ptr(), w.data_ptr(), n, sq.data_ptr(), 1.0)
            if sched:
                cur = _cur(lr, r, dev)
                _lib.call("sdt_lion32_step_scheduled", *head, cur.data_ptr(), 0.07, 0.9, 0.99, s)
            else:
                _lib.call("sdt_lion32_step", *head, lr, 0.07, 0.9, 0.99, r, s)
            torch.cuda.synchronize()
            outs.append((p, mom, ema, w.view(torch.int16)))
        for name, a, b in zip(("master", "momentum", "ema", "bf16 mirror"), *outs):
            assert torch.equal(a, b), f"{name} differs (lr={lr}, r={r})"


def test_select_clamps_and_advances_eager_and_replayed(dev):
    from stable_diffusion_training_amd import _lib
    lr_tab = torch.tensor([-1.0, -2.0, -3.0, -4.0, -5.0], device=dev)
    ema_tab = torch.tensor([[0.0, 1.0], [0.5, 0.5], [0.75, 0.25]], device=dev).reshape(-1)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    cur = torch.full((4,), 7.0, device=dev)
    want = [[-float(min(t, 4) + 1), [0.0, 0.5, 0.75][min(t, 2)], [1.0, 0.5, 0.25][min(t, 2)], 0.0] for t in range(8)]

    def launch():
        _lib.call("sdt_opt_schedule_select", step.data_ptr(), lr_tab.data_ptr(), 5, ema_tab.data_ptr(), 3, cur.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)

    for t in range(8):
        launch()
        assert cur.tolist() == want[t], t
        assert int(step.item()) == t + 1
    step.zero_()
    cur.fill_(7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    torch.cuda.synchronize()
    assert int(step.item()) == 0 and cur.tolist() == [7.0] * 4  # a capture executes nothing
    for t in range(8):
        graph.replay()
        assert cur.tolist() == want[t], t
        assert int(step.item()) == t + 1


def _states(case, dev, quantize, scheduled):
    """The tiny states, with the schedule installed from the config (scheduled) or none (the hand-set side)."""
    from stable_diffusion_training_amd import training_utils as tu
    tc, states = build_hip_states(case, dev, quantize=quantize, ema=True)
    if not scheduled:
        return tc, states
    del states
    models = {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
              "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
              "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}
    tc = dataclasses.replace(tc, lr_scheduler="cosine")
    return tc, tu.on_device_model_training_state(tc, models, device=dev, lr_schedule=LR_SCHED, ema_schedule=EMA_SCHED)


def _inputs(case, dev, step):
    g = torch.Generator().manual_seed(100 + step)
    batch = to_dev(case["batch"], dev)
    batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
    rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
            for k, v in case["rand"].items()}
    return batch, rand


def _snap(us, ts):
    torch.cuda.synchronize()
    return {f"{name}.{b}": getattr(st, b).clone() for name, st in (("unet", us.store), ("text", ts.store)) for b in STATE
            if getattr(st, b) is not None}


def _run(case, dev, quantize, scheduled, mode, steps=6):
    """mode: "eager" (train_step), "graph" (the shape table with graphs: steps 3 .. 6 replay), "micro" (micro_batches=2)."""
    from stable_diffusion_training_amd import training_utils as tu
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, quantize, scheduled)
    lru, lrt = L.LRSchedule("cosine", us.hyper["lr"], **LR_SCHED), L.LRSchedule("cosine", ts.hyper["lr"], **LR_SCHED)
    ema = L.EMASchedule("warmup", EMA_RATE)
    if scheduled:
        assert us.store.schedule is not None and ts.store.schedule is not None
    K = 2 if mode == "micro" else 1
    gen = torch.Generator(device=dev)  # (unused: every draw is explicit) one object, as a captured step is bound to it
    fn = None
    if mode == "graph":
        tc = dataclasses.replace(tc, ema_rate=EMA_RATE)
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True, per_device_batch=2)
        fn = table[[k for k in table if k[2] == 512 and k[3] == 512][0]]
    trace = []
    for t in range(steps):
        batch, rand = _inputs(case, dev, t)
        if scheduled:
            r = EMA_RATE
        else:  # the hand-set side: the schedule's values, by value
            us.hyper["lr"], ts.hyper["lr"] = lru.rate(t), lrt.rate(t)
            r = ema.rate(t)
        if fn is not None:
            out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
        else:
            out = tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=r,
                                rand=rand, micro_batches=K)
        snap = _snap(us, ts)
        snap["loss"] = out[4]["loss"].clone()
        trace.append(snap)
    if fn is not None:
        assert fn.graph is not None and fn.calls == 2
    assert us.step == steps and ts.step == steps
    if scheduled:
        assert int(us.store._sched["step"].item()) == steps and int(ts.store._sched["step"].item()) == steps
    return trace


@pytest.mark.parametrize("quantize,mode", [(True, "eager"), (False, "eager"), (True, "graph"), (True, "micro")])
def test_scheduled_steps_equal_hand_set_steps_bit_for_bit(dev, quantize, mode):
    """Six scheduled steps (cosine with a 2-step warmup, EMA warmup) against six steps whose lr and ema_rate are set by hand to the
    schedule's values before each step.  With graphs, steps 3 to 6 are replays: the schedule must advance in them."""
    case = make_case("tiny", B=2, image=64)
    hand = _run(case, dev, quantize, False, "eager" if mode == "graph" else mode)
    sched = _run(case, dev, quantize, True, mode)
    for t, (a, b) in enumerate(zip(hand, sched)):
        for k in a:
            assert torch.equal(a[k], b[k]), f"step {t}: {k} differs between the hand-set and the scheduled run ({mode})"
    # after step 0 (lr 0, EMA rate 0): masters as loaded and the bf16 mirror theirs, the momentum moved, EMA = masters
    tc, (us0, ts0, *_rest) = _states(case, dev, quantize, False)
    s0 = sched[0]
    for name, st in (("unet", us0.store), ("text", ts0.store)):
        assert torch.equal(s0[f"{name}.master"], st.master), name
        # (the sweep mirrors every element of [0, total); the zero-padded copies behind it are the loaded ones)
        assert torch.equal(s0[f"{name}.w"][: st.total], st.master.to(torch.bfloat16)), name
        assert torch.equal(s0[f"{name}.w"][st.total:], st.w[st.total:]), name
        assert torch.equal(s0[f"{name}.ema"], s0[f"{name}.master"]), name
        moved = "codes" if quantize else "mom"
        assert not torch.equal(s0[f"{name}.{moved}"], getattr(st, moved)), name
    assert not torch.equal(sched[1]["unet.master"], sched[0]["unet.master"])  # the warmup's second step moves the weights


def test_schedule_trajectory_follows_the_oracle(dev):
    """The schedule (base rate 3e-4) against oracle.train_step driven per step with opt["lr"] = lr_t and ema_rate = r_t: the gates of
    test_tiny_four_step_trajectory_vs_oracle."""
    from oracle import train_step as ots
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    base = 3e-4
    lrs, ema = L.LRSchedule("cosine", base, **LR_SCHED), L.EMASchedule("warmup", EMA_RATE)
    up, tp, ust, tst = case["weights"]["unet"], case["weights"]["clip"], None, None
    uema = {k: v.numpy().copy() for k, v in up.items()}
    ref_losses = []
    for t in range(6):
        r = ots.train_step(up, tp, case["weights"]["vae"], case["sched_state"], case["cfgs"], case["batch"], case["rand"],
                           dict(ots.DEFAULT_OPT, lr=lrs.rate(t)), unet_state=ust, te_state=tst, unet_ema=uema, ema_rate=ema.rate(t))
        ref_losses.append(r["loss"])
        up = {k: torch.from_numpy(np.asarray(v)) for k, v in r["unet_params"].items()}
        tp = {k: torch.from_numpy(np.asarray(v)) for k, v in r["te_params"].items()}
        ust, tst = r["unet_state"], r["te_state"]
        uema = r.get("unet_ema", uema)
    tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
    for st in (us, ts):
        st.hyper["lr"] = base
        st.store.set_schedule(lr=L.LRSchedule("cosine", base, **LR_SCHED), ema=L.EMASchedule("warmup", EMA_RATE))
    losses = []
    for _ in range(6):
        out = tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc,
                            strip_bos_eos_token=False, rand=to_dev(case["rand"], dev), ema_rate=EMA_RATE)
        losses.append(float(out[4]["loss"].item()))
    assert ref_losses[-1] < 0.9 * ref_losses[0] and losses[-1] < 0.9 * losses[0], (ref_losses, losses)
    for a, b in zip(losses, ref_losses):
        assert abs(a - b) / b < 3e-2, (losses, ref_losses)
    got, got_ema = us.store.export(), us.store.export("ema")
    moved = agree = 0
    for k, v in up.items():
        w0 = case["weights"]["unet"][k].numpy()
        d_ref, d_got = np.sign(v.numpy() - w0), np.sign(got[k].cpu().numpy() - w0)
        moved += int((d_ref != 0).sum())
        agree += int(((d_ref == d_got) & (d_ref != 0)).sum())
    assert agree / moved > 0.9, agree / moved
    # the EMA, warmed up over the same rates, tracks the oracle's: the same net displacement direction
    moved = agree = 0
    for k, v in uema.items():
        w0 = case["weights"]["unet"][k].numpy()
        d_ref, d_got = np.sign(np.asarray(v) - w0), np.sign(got_ema[k].cpu().numpy() - w0)
        moved += int((d_ref != 0).sum())
        agree += int(((d_ref == d_got) & (d_ref != 0)).sum())
    assert agree / moved > 0.9, agree / moved


def test_resume_continues_the_schedule_bit_for_bit(dev, tmp_path):
    """3 steps, save_training_state, fresh states, load_training_state, 3 steps through the graphed table (the last one a replay): the
    device step counter resumes with the saved count, and the result equals 6 uninterrupted steps."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case("tiny", B=2, image=64)
    whole = _run(case, dev, True, True, "eager")[-1]
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, True, True)
    for t in range(3):
        batch, rand = _inputs(case, dev, t)
        tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=EMA_RATE, rand=rand)
    path = str(tmp_path / "state.safetensors")
    tu.save_training_state(path, us, ts)
    del us, ts, ue, te, vae
    tc, (us, ts, ue, te, vae, sc, _) = _states(case, dev, True, True)
    assert int(us.store._sched["step"].item()) == 0
    tu.load_training_state(path, us, ts)
    assert us.step == 3 and int(us.store._sched["step"].item()) == 3 and int(ts.store._sched["step"].item()) == 3
    tc = dataclasses.replace(tc, ema_rate=EMA_RATE)
    table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True, per_device_batch=2)
    fn = table[[k for k in table if k[2] == 512 and k[3] == 512][0]]
    gen = torch.Generator(device=dev)
    for t in range(3, 6):
        batch, rand = _inputs(case, dev, t)
        fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
    assert fn.graph is not None
    got = _snap(us, ts)
    for k in got:
        assert torch.equal(got[k], whole[k]), f"{k}: resumed run differs from the uninterrupted one"


def test_facade_takes_a_schedule(dev):
    """lion_quant.lion_8bit(schedule) for three updates against oracle.lion8.lion_step with lr = schedule(count): the exactness of
    test_lion_quant_facade_matches_oracle."""
    from oracle import lion8
    from stable_diffusion_training_amd import lion_quant
    g = torch.Generator().manual_seed(3)
    params = {"a/kernel": torch.randn(48, 32, generator=g) * 0.05, "a/bias": torch.randn(32, generator=g) * 0.05,
              "b/kernel": torch.randn(3, 3, 16, 16, generator=g) * 0.05, "n/scale": torch.ones(16)}
    qmask = {"a/kernel": True, "a/bias": False, "b/kernel": True, "n/scale": False}
    dmask = {"a/kernel": True, "a/bias": False, "b/kernel": True, "n/scale": False}
    wd = 0.07
    schedule = L.LRSchedule("cosine", 1e-3, num_warmup_steps=1, num_training_steps=3).rate
    tx = lion_quant.lion_8bit(schedule, block_size=16, weight_decay=wd, mask=dmask, excluded_layer_mask=qmask)
    p_dev = {k: v.to(dev) for k, v in params.items()}
    state = tx.init(p_dev)
    p_ref = {k: v.numpy() for k, v in params.items()}
    s_ref = lion8.init_state(p_ref, qmask, 16)
    for step in range(3):
        grads = {k: torch.randn(v.shape, generator=g) * 1e-2 for k, v in params.items()}
        before = {k: v.clone() for k, v in p_dev.items()}
        upd, state = tx.update({k: v.to(dev) for k, v in grads.items()}, state, p_dev)
        p_dev = {k: p_dev[k] + upd[k] for k in p_dev}
        p_ref, s_ref, _ = lion8.lion_step(p_ref, {k: v.numpy() for k, v in grads.items()}, s_ref, lr=schedule(step), wd=wd,
                                          block_size=16, decay_mask=dmask, clip=None)
        assert state.count == step + 1
        if step == 0:  # schedule(0) = 0: no update, the momentum advances
            assert all(torch.equal(p_dev[k], before[k]) for k in p_dev)
        for k in params:
            diff = (p_dev[k].cpu().numpy() - p_ref[k])
            assert (abs(diff) > 1e-7).mean() < 5e-3, (k, step)
        assert np.array_equal(state.mu_quant["a/kernel"][0].cpu().numpy(), s_ref["mu"]["a/kernel"][0])


def _dp_worker(rank, world, port, q):
    """Captured steps with the schedule on two ranks, replicated and sharded."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from stable_diffusion_training_amd import dp
        from stable_diffusion_training_amd import training_utils as tu
        torch.cuda.set_device(0)
        dev = torch.device("cuda:0")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        case = make_case("tiny", B=2, image=64)
        sl = slice(rank, rank + 1)
        batch = to_dev({k: v[sl] for k, v in case["batch"].items()}, dev)
        rand = to_dev({k: v[sl] for k, v in case["rand"].items()}, dev)
        res = {}
        for mode in ("replicated", "sharded"):
            tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, quantize=True, ema=True,
                                                                 quant_excluded=["bias", "scale", "embedding"])
            for st in (us, ts):
                st.store.set_schedule(lr=L.LRSchedule("cosine", st.hyper["lr"], **LR_SCHED), ema=L.EMASchedule("warmup", EMA_RATE))
            init = (us.store.master.clone(), ts.store.master.clone())
            red = dp.GradReducer([us.store, ts.store], bucket_bytes=1 << 16, shard=mode == "sharded")

            def bound(us, ts, ue, te, batch, rng, vae, sched, **extra):
                return tu.train_step(us, ts, ue, te, batch, rng, vae, sched, strip_bos_eos_token=False, ema_rate=EMA_RATE, reducer=red,
                                     **extra)

            step = tu._GraphedStep(bound, warmup=1, reducer=red)
            rng = torch.Generator(device=dev)
            step(us, ts, ue, te, batch, rng, vae, sc, rand=rand)  # step 0: eager, lr 0
            red.gather_state()
            torch.cuda.synchronize()
            first_same = bool(torch.equal(us.store.master, init[0]) and torch.equal(ts.store.master, init[1]))
            for _ in range(4):  # capture + replays: steps 1 .. 4
                step(us, ts, ue, te, batch, rng, vae, sc, rand=rand)
            torch.cuda.synchronize()
            assert step.graph_b is not None and not step.disabled
            red.gather_state()
            torch.cuda.synchronize()
            snap = tuple(getattr(st, b).detach().cpu().numpy().copy() for st in (us.store, ts.store) for b in ("master", "codes", "ema"))
            counters = (int(us.store._sched["step"].item()), int(ts.store._sched["step"].item()))
            moved = not torch.equal(us.store.master, init[0])
            res[mode] = (snap, first_same, counters, moved)
            del red, step
        q.put((rank, "ok", res))
        dist.barrier()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc()[-1500:], None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_captured_schedule_replicated_and_sharded():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 43500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    r0, r1 = res[0][2], res[1][2]
    for mode in ("replicated", "sharded"):
        for a, b in zip(r0[mode][0], r1[mode][0]):
            assert (a == b).all(), f"{mode}: the ranks hold different state"
        for r in (r0, r1):
            assert r[mode][1], f"{mode}: the lr = 0 first step moved the masters"
            assert r[mode][2] == (5, 5), f"{mode}: device step counters {r[mode][2]}"
            assert r[mode][3], f"{mode}: the scheduled steps never moved the weights"
