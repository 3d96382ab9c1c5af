"""Micro-batch gradient accumulation (train_step micro_batches=K, ParamStore.accumulate, sdt_grad_accumulate) on the MI355X:
bit-exactness against the plain step where the arithmetic allows it, parity with the oracle's full-batch step, graph replay,
reproducibility, and the fp32 exchange of two data-parallel ranks."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.helpers import build_hip_states, make_case, rel_l2, to_dev

pytestmark = pytest.mark.gpu

STATE = ("master", "w", "codes", "inv_scale", "mom", "ema")


def _snapshot(us, ts):
    return {f"{name}.{b}": getattr(st, b).clone() for name, st in (("unet", us.store), ("text", ts.store)) for b in STATE}


def _doubled(d):
    return {k: torch.cat([v, v]) for k, v in d.items()}


@pytest.mark.parametrize("size,B,image,quantize", [("tiny", 2, 64, True), ("tiny", 2, 64, False), ("sd15", 1, 256, True)])
def test_identical_micro_batches_equal_the_plain_step_bit_for_bit(dev, monkeypatch, size, B, image, quantize):
    """batch = b ++ b with K = 2 accumulates g + g and scales by 1/2: exact in fp32, so the optimizer sees the plain step's gradient
    widened - the 8-bit sweep reads it as fp32 instead of bf16 - and the finish pass's norm has the partition of the plain step's
    norm pass.  Everything the step writes must then equal the plain step (ordinary norm pass) bit for bit."""
    from stable_diffusion_training_amd import training_utils as tu
    case = make_case(size, B=B, image=image)
    runs = []
    for K in (1, 2):
        monkeypatch.setattr(tu, "_FUSED_NORM", False)
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, quantize=quantize, ema=True)
        batch, rand = to_dev(case["batch"], dev), to_dev(case["rand"], dev)
        if K == 2:
            batch, rand = _doubled(batch), _doubled(rand)
        out = tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=0.999,
                            rand=rand, micro_batches=K)
        torch.cuda.synchronize()
        assert (us.store.gacc is not None) == (K == 2)
        snap = _snapshot(us, ts)
        snap["loss"] = out[4]["loss"].clone()
        snap["unet.sqnorm"], snap["text.sqnorm"] = us.store.sqnorm.clone(), ts.store.sqnorm.clone()
        snap["unet.grad"] = us.store.grad_flat().clone()  # after K = 2: the mean gradient the optimizer consumed
        runs.append(snap)
        del us, ts, ue, te, vae
    for k in runs[0]:
        a, b = runs[0][k], runs[1][k]
        assert torch.equal(a, b), f"{k}: accumulated step differs ({(a.double() - b.double()).abs().max().item():.3e} max abs)"


def _oracle(case, **kw):
    from oracle import train_step as ots
    return ots.train_step(case["weights"]["unet"], case["weights"]["clip"], case["weights"]["vae"], case["sched_state"],
                          case["cfgs"], case["batch"], case["rand"], dict(ots.DEFAULT_OPT), **kw)


@pytest.mark.parametrize("variant", ["epsilon", "vpred_minsnr_offset"])
def test_micro_batches_match_the_oracle_full_batch_step(dev, variant):
    """The oracle steps once over all 4 samples; the HIP path accumulates K = 2 micro-batches of 2 and K = 4 of 1 (rand sliced the
    same way).  Gates of test_tiny_train_step_parity."""
    from stable_diffusion_training_amd import training_utils as tu
    if variant == "epsilon":
        case = make_case("tiny", B=4, image=64)
        pred_type, kw = "epsilon", {}
    else:
        case = make_case("tiny", B=4, image=64, sched="zero_snr_scaled_linear")
        case["rand"]["offset_noise"] = torch.randn(4, 4, 1, 1, generator=torch.Generator().manual_seed(7))
        pred_type, kw = "v_prediction", dict(min_snr_gamma_magnitude=5.0, offset_noise_magnitude=0.1)
    ref = _oracle(case, prediction_type=pred_type, **kw)
    for K in (2, 4):
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, prediction_type=pred_type)
        out = tu.train_step(us, ts, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae, sc,
                            strip_bos_eos_token=False, rand=to_dev(case["rand"], dev), micro_batches=K, **kw)
        loss = out[4]["loss"].item()
        assert abs(loss - ref["loss"]) / ref["loss"] < 1e-2, (K, loss, ref["loss"])
        for store, gref, gn in ((us.store, ref["unet_grads"], ref["unet_gnorm"]), (ts.store, ref["te_grads"], ref["te_gnorm"])):
            assert abs(store.grad_norm() - float(gn)) / float(gn) < 3e-2, (K, store.grad_norm(), float(gn))
            g = store.export("grad")
            flat = torch.cat([g[k].flatten().cpu() for k in gref])
            rflat = torch.cat([gref[k].flatten() for k in gref])
            cos = torch.dot(flat, rflat) / (flat.norm() * rflat.norm())
            assert cos > 0.995, f"K={K}: gradient cosine {cos}"
            worst = max((rel_l2(g[k], gref[k]), k) for k in gref if gref[k].norm() > 1e-3 * rflat.norm())
            assert worst[0] < 0.1, f"K={K}: worst leaf {worst}"
        for store, pref, w0 in ((us.store, ref["unet_params"], case["weights"]["unet"]), (ts.store, ref["te_params"], case["weights"]["clip"])):
            got = store.export()
            agree = tot = 0
            for k, v in pref.items():
                d_ref = np.sign(v - w0[k].numpy())
                d_got = np.sign(got[k].cpu().numpy() - w0[k].numpy())
                agree += (d_ref == d_got).sum()
                tot += d_ref.size
            assert agree / tot > 0.97, f"K={K}: update sign agreement {agree / tot}"
        del us, ts, ue, te, vae


def test_captured_accumulated_step_matches_eager_and_is_reproducible(dev):
    """A K = 2 table entry (key: the loader's batch of 2 x 1): two eager warm-up steps, then capture and replays.  Every step of
    the replayed run equals the eager run bit for bit, as does a second eager run from scratch."""
    from stable_diffusion_training_amd import training_utils as tu

    def run(use_graph):
        case = make_case("tiny", B=2, image=64)
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        tc.ema_rate = 0.999
        table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=use_graph, per_device_batch=1,
                                                    micro_batches=2)
        assert list(table) == [(2, 3, 512, 512)]
        fn = table[(2, 3, 512, 512)]
        gen = torch.Generator(device=dev)
        trace = []
        for step in range(4):
            g = torch.Generator().manual_seed(100 + step)
            batch = to_dev(case["batch"], dev)
            batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
            rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype)).to(dev)
                    for k, v in case["rand"].items()}
            out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
            snap = _snapshot(us, ts)
            snap["loss"] = out[4]["loss"].clone()
            snap["unet.sqnorm"] = us.store.sqnorm.clone()
            trace.append(snap)
        if use_graph:
            assert fn.graph is not None and fn.calls == 2
        assert us.step == 4
        with pytest.raises(ValueError, match="divides the batch"):
            tu.train_step(us, ts, ue, te, to_dev(case["batch"], dev), gen, vae, sc, micro_batches=3)
        return trace

    eager, eager2, graph = run(False), run(False), run(True)
    assert len({float(s["loss"]) for s in graph}) == 4
    for name, other in (("second eager run", eager2), ("graph replay", graph)):
        for step, (a, b) in enumerate(zip(eager, other)):
            for k in a:
                assert torch.equal(a[k], b[k]), f"{name} differs from the eager run at step {step}, {k}"


def _dp_worker(rank, world, port, q):
    """Rank r takes samples [2r, 2r + 2) of a batch of 4 as K = 2 micro-batches of 1; the fp32 sums are all-reduced once."""
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
        case = make_case("tiny", B=4, image=64)
        sl = slice(2 * rank, 2 * rank + 2)
        batch = to_dev({k: v[sl] for k, v in case["batch"].items()}, dev)
        rand = to_dev({k: v[sl] for k, v in case["rand"].items()}, dev)
        res = {}
        for mode in ("eager", "graph"):
            tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, quantize=True)
            red = dp.GradReducer([us.store, ts.store], bucket_bytes=1 << 16)

            def bound(us, ts, ue, te, batch, rng, vae, sched, **extra):
                return tu.train_step(us, ts, ue, te, batch, rng, vae, sched, strip_bos_eos_token=False, reducer=red, micro_batches=2,
                                     **extra)

            step = tu._GraphedStep(bound, warmup=1, reducer=red) if mode == "graph" else bound
            rng = torch.Generator(device=dev)
            losses = []
            for i in range(3 if mode == "graph" else 1):  # graph: 1 eager warm-up, then capture + replay, replay
                out = step(us, ts, None, None, batch, rng, vae, sc, rand=rand)
                losses.append(float(out[4]["loss"].item()))
                if i == 0 and mode == "eager":
                    g = us.store.grad_flat().detach().cpu().clone()
                    gnorm = us.store.grad_norm()
            torch.cuda.synchronize()
            if mode == "graph":
                assert step.graph_b is not None and not step.disabled
            res[mode] = (us.store.master.detach().cpu().numpy().copy(), ts.store.master.detach().cpu().numpy().copy(), losses)
        # the sharded optimizer does not take micro-batches: refused before any collective
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, quantize=True)
        red = dp.GradReducer([us.store, ts.store], bucket_bytes=1 << 16, shard=True)
        try:
            tu.train_step(us, ts, None, None, batch, torch.Generator(device=dev), vae, sc, reducer=red, rand=rand, micro_batches=2)
            res["shard_refused"] = False
        except ValueError as e:
            res["shard_refused"] = "sharded optimizer" in str(e)
        if rank == 0:
            def worst(g2, st2, floor):
                """(worst cosine, worst relative norm error) over the kernel leaves whose reference gradient exceeds floor x its norm"""
                wc, wn = 1.0, 0.0
                for pth, lf in us.store.leaves.items():
                    lf2 = st2.leaves[pth]
                    a, b = g[lf.offset: lf.offset + lf.numel], g2[lf2.offset: lf2.offset + lf2.numel]
                    if lf.numel >= 256 and float(b.norm()) > floor * float(g2.norm()):
                        wc = min(wc, float(torch.dot(a, b) / (a.norm() * b.norm())))
                        wn = max(wn, abs(float(a.norm() / b.norm()) - 1.0))
                return wc, wn
            # single process, the same four micro-batches of 1 accumulated in one process: only the order of the fp32 sums differs
            tc1, (us1, ts1, _, _, vae1, sc1, _) = build_hip_states(case, dev, quantize=True)
            tu.train_step(us1, ts1, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae1, sc1,
                          strip_bos_eos_token=False, rand=to_dev(case["rand"], dev), micro_batches=4)
            # single process, the whole batch of 4 in one pass, float32 gradients, no exchange
            tc2, (us2, ts2, _, _, vae2, sc2, _) = build_hip_states(case, dev, quantize=False)
            out2 = tu.train_step(us2, ts2, None, None, to_dev(case["batch"], dev), torch.Generator(device=dev), vae2, sc2,
                                 strip_bos_eos_token=False, rand=to_dev(case["rand"], dev))
            torch.cuda.synchronize()
            floor = 1e-3 / len(us.store.leaves) ** 0.5
            res["ref"] = (float(out2[4]["loss"].item()), us2.store.grad_norm(), gnorm, us1.store.grad_norm(),
                          worst(us1.store.grad_flat().detach().cpu(), us1.store, floor),
                          worst(us2.store.grad_flat().detach().cpu(), us2.store, 1e-3))
        q.put((rank, "ok", res))
        dist.barrier()
    except Exception as e:  # pragma: no cover
        import traceback
        q.put((rank, "ERR " + repr(e) + traceback.format_exc()[-1500:], None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_accumulate_and_exchange_fp32_sums(dev):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(120)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    r0, r1 = res[0][2], res[1][2]
    for mode in ("eager", "graph"):
        assert (r0[mode][0] == r1[mode][0]).all() and (r0[mode][1] == r1[mode][1]).all(), f"{mode}: ranks diverged"
        assert r0[mode][2] == r1[mode][2], f"{mode}: mean loss differs between the ranks"
    # the captured run's first (eager) step is the eager run's step
    assert (r0["graph"][2][0] == r0["eager"][2][0])
    assert r0["shard_refused"] and r1["shard_refused"]
    ref_loss, ref_norm, norm, acc_norm, (cos1, dn1), (cos2, dn2) = r0["ref"]
    # against the same micro-batches accumulated in one process: every kernel leaf of size, down to the ones test_gpu_dp gates
    assert cos1 > 0.9999 and dn1 < 1e-3, f"vs one-process K=4: worst kernel leaf cosine {cos1}, norm off by {dn1}"
    assert abs(norm - acc_norm) / acc_norm < 1e-4, (norm, acc_norm)
    # against one pass over the batch of 4: the gates of test_tiny_train_step_parity's leaf selection (leaves above 1e-3 of the
    # model's gradient norm).  Below that, down_blocks_0/resnets_0/time_emb_proj/kernel (1e-4 of the norm, a sum over the latent
    # pixels that cancels to bf16 noise) already differs between one pass over 4 samples and two plain passes over 2 (cosine 0.33)
    assert cos2 > 0.995 and dn2 < 0.03, f"vs one pass over 4: worst kernel leaf cosine {cos2}, norm off by {dn2}"
    assert abs(norm - ref_norm) / ref_norm < 3e-2, (norm, ref_norm)
    assert abs(r0["eager"][2][0] - ref_loss) / ref_loss < 1e-2
