"""The grouped launches that take work off the input-gradient chain: the dK/dV passes of several cross-attentions
(sdt_attention_bwd_dkv_group after sdt_attention_bwd_dq) and the row-bias column sums of several ResBlocks (sdt_colsum_batched_group).
Both run every problem with the plan of its single launch, so everything here is compared with torch.equal: the grouped calls
against the single ones on random bf16 inputs with guard bytes around every output and slab, and a tiny UNet + text tower train_step
with the deferrals on against the same steps with them off (ops.wgrad_grouping(offchain=False)), eagerly and replayed from a graph -
also at 32 x 32 latents, where the deferred problems carry slabs - and the operators that defer (attention_packed, attention_ip,
conv2d's row bias) over the column slices of one projection in both forms.  The exact tables: tests/test_gpu_grouped_exact.py."""
import ctypes
import functools

import pytest
import torch

from oracle import nets as onets
from stable_diffusion_training_amd import _lib, ops
from tests.helpers import build_hip_states, make_case, to_dev
from tests.kernel_checks import Guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, NK = 2, 2, 77

# (D, Nq, key weights).  D = 40 holds three problems of one instantiation (the prefix table) and D = 80 two; D = 160 and D = 128 are
# instantiations with a single problem each (a one-entry table, no prefix walk).  Nq = 64 is a single query tile; attn_qsplits splits
# the query range from Nq = 1024 on (Nq / 256 >= 2 AND Nq >= 1024), so the Nq = 512 problems run unsplit like 64 and 256, and the
# Nq = 1024 ones bring slabs and the grouped finishing pass (two problems of two instantiations).
DKV_PROBLEMS = [(40, 64, False), (40, 512, True), (80, 256, True), (160, 256, False), (40, 1024, False), (80, 1024, True), (128, 512, True)]


def test_the_problem_list_holds_shared_and_single_instantiations():
    from collections import Counter
    per_class = Counter(next(i for i, top in enumerate((48, 64, 80, 96, 128, 160)) if D <= top) for D, _, _ in DKV_PROBLEMS)
    assert sorted(per_class.values()) == [1, 1, 2, 3], per_class


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dkv_case(dev, D, Nq, weighted, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = H * D
    q, k, v, dout = (torch.randn(B, n, C, generator=g).to(BF).to(dev) for n in (Nq, NK, NK, Nq))
    kw = (1.0 + torch.randint(0, 2, (NK,), generator=g).float()).to(dev) if weighted else None
    desc = _lib.SdtAttnDesc(B, H, Nq, NK, D, C, C, C, C, D ** -0.5, 0, 0, 0, 0, 0, None if kw is None else kw.data_ptr())
    out = torch.empty_like(q)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=dev)
    _lib.call("sdt_attention_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), ctypes.addressof(desc), _stream())
    return dict(q=q, k=k, v=v, dout=dout, kw=kw, desc=desc, out=out, lse=lse, D=D, Nq=Nq, C=C)


def _inline_bwd(c):
    """Today's call: dq, dk, dv and the delta it leaves at the start of its workspace."""
    lib = _lib.load()
    dp = ctypes.addressof(c["desc"])
    need = lib.sdt_attention_bwd_workspace_bytes(dp)
    assert need == lib.sdt_attention_bwd_delta_bytes(dp) + lib.sdt_attention_bwd_slab_bytes(dp)
    ws = torch.empty(need, dtype=torch.uint8, device=c["q"].device)
    dq, dk, dv = torch.empty_like(c["q"]), torch.empty_like(c["k"]), torch.empty_like(c["v"])
    _lib.call("sdt_attention_bwd", c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), c["out"].data_ptr(), c["dout"].data_ptr(),
              c["lse"].data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), need, dp, _stream())
    torch.cuda.synchronize()
    return dq, dk, dv, ws[: B * H * c["Nq"] * 4].view(torch.float32).clone()


def test_grouped_dkv_equals_inline_calls(dev):
    lib = _lib.load()
    cases = [_dkv_case(dev, D, Nq, w, 100 + i) for i, (D, Nq, w) in enumerate(DKV_PROBLEMS)]
    want = [_inline_bwd(c) for c in cases]
    probs, guards = [], []
    for i, c in enumerate(cases):
        dp = ctypes.addressof(c["desc"])
        delta = Guarded(1, lib.sdt_attention_bwd_delta_bytes(dp) // 4, torch.float32, dev, pad=0, back_rows=1)
        dq = torch.empty_like(c["q"])
        _lib.call("sdt_attention_bwd_dq", c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), c["out"].data_ptr(), c["dout"].data_ptr(),
                  c["lse"].data_ptr(), dq.data_ptr(), delta.ptr, dp, _stream())
        torch.cuda.synchronize()
        assert torch.equal(dq, want[i][0]), f"problem {i}: dq of the dQ pass alone"
        assert torch.equal(delta.t.reshape(-1)[: B * H * c["Nq"]], want[i][3]), f"problem {i}: delta of the dQ pass alone"
        delta.check(f"problem {i} delta")
        dk, dv = (Guarded(B * NK, c["C"], BF, dev) for _ in range(2))
        nslab = lib.sdt_attention_bwd_slab_bytes(dp)
        assert (nslab > 0) == (c["Nq"] >= 1024), (c["Nq"], nslab)
        slabs = Guarded(1, nslab // 4, torch.float32, dev, pad=0, back_rows=1) if nslab else None
        desc = _lib.SdtAttnDesc.from_buffer_copy(c["desc"])
        desc.ldgrad_k = desc.ldgrad_v = dk.ld  # the padded pitch of the guarded outputs
        probs.append(_lib.SdtAttnDkvProblem(c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), c["dout"].data_ptr(), c["lse"].data_ptr(),
                                            delta.ptr, dk.ptr, dv.ptr, None if slabs is None else slabs.ptr, desc))
        guards.append((dk, dv, slabs, delta))
    assert len(probs) <= lib.sdt_attention_bwd_dkv_group_max()
    arr = (_lib.SdtAttnDkvProblem * len(probs))(*probs)
    _lib.call("sdt_attention_bwd_dkv_group", arr, len(probs), _stream())
    torch.cuda.synchronize()
    for i, (dk, dv, slabs, delta) in enumerate(guards):
        what = f"problem {i} {DKV_PROBLEMS[i]}"
        assert torch.equal(dk.t.reshape(B, NK, -1), want[i][1]), what + ": dk"
        assert torch.equal(dv.t.reshape(B, NK, -1), want[i][2]), what + ": dv"
        dk.check(what + " dk")
        dv.check(what + " dv")
        delta.check(what + " delta")
        if slabs is not None:
            slabs.check(what + " slabs")


def test_grouped_dkv_refuses_a_split_problem_without_slabs(dev):
    c = _dkv_case(dev, 40, 1024, False, 7)
    dk = torch.empty_like(c["k"])
    delta = torch.zeros(B * H * 1024, dtype=torch.float32, device=dev)
    arr = (_lib.SdtAttnDkvProblem * 1)(_lib.SdtAttnDkvProblem(c["q"].data_ptr(), c["k"].data_ptr(), c["v"].data_ptr(), c["dout"].data_ptr(),
                                                               c["lse"].data_ptr(), delta.data_ptr(), dk.data_ptr(), dk.data_ptr(), None, c["desc"]))
    with pytest.raises(_lib.SdtError, match="slabs"):
        _lib.call("sdt_attention_bwd_dkv_group", arr, 1, _stream())


COLSUM_PROBLEMS = [(2, 64, 64), (2, 256, 320), (1, 16, 8)]  # (batch, rows per image, N): a whole tile, a tail of columns, the smallest width


def test_grouped_column_sums_equal_single_launches(dev):
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(5)
    dys = [torch.randn(b * rows, N, generator=g).to(BF).to(dev) for b, rows, N in COLSUM_PROBLEMS]
    want = []
    for dy, (b, rows, N) in zip(dys, COLSUM_PROBLEMS):
        out = torch.empty(b, N, dtype=BF, device=dev)
        ws = ops.reduce_workspace(lib.sdt_colsum_workspace_bytes(b, rows, N), dev)
        _lib.call("sdt_colsum_batched_bf16", dy.data_ptr(), out.data_ptr(), b, rows, N, N, ws.data_ptr(), ws.numel(), _stream())
        want.append(out)
    outs = [Guarded(b, N, BF, dev, pad=0, back_rows=8) for b, rows, N in COLSUM_PROBLEMS]
    arr = (_lib.SdtColsumProblem * len(dys))(*[_lib.SdtColsumProblem(dy.data_ptr(), o.ptr, b, rows, N, N)
                                              for dy, o, (b, rows, N) in zip(dys, outs, COLSUM_PROBLEMS)])
    need = lib.sdt_colsum_batched_group_workspace_bytes(arr, len(dys))
    assert need > 65536
    ws = ops.reduce_workspace(need, dev)
    _lib.call("sdt_colsum_batched_group", arr, len(dys), ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    for o, w, p in zip(outs, want, COLSUM_PROBLEMS):
        assert torch.equal(o.t, w), f"column sums of {p}"
        o.check(f"column sums of {p}")
    assert int(ws[:65536].view(torch.int32).abs().sum()) == 0, "the arrival counters are zero again"


# ------------------------------------------------------------------------------------------------ the whole step
def _wide_tiny_case(image=64):
    """The tiny two-level UNet with widths (64, 128): multiples of 64, so the [k|v] and time-embedding projections of one width run
    as one GEMM (ops.linear_multi) and the blocks read column slices - the path the deferrals take."""
    case = make_case("tiny", B=2, image=image)
    cfg = onets.unet_config("tiny", block_out_channels=(64, 128))
    case["cfgs"]["unet"] = cfg
    case["weights"]["unet"] = onets.init_params(onets.unet_param_shapes(cfg), 1)
    return case


def _three_steps(dev, case, offchain, graph, monkeypatch):
    from stable_diffusion_training_amd import training_utils as tu
    seen = []
    real_call, real_deferred = ops.call, ops._attention_bwd_deferred

    def deferred(*a):
        real_deferred(*a)
        slabs = ops._DKV_QUEUE[-1][1][3]
        seen.append("a queued dK/dV problem with slabs" if slabs is not None else "a queued dK/dV problem without slabs")

    with monkeypatch.context() as m:
        m.setattr(ops, "wgrad_grouping", functools.partial(ops.wgrad_grouping, offchain=offchain))
        m.setattr(ops, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
        m.setattr(ops, "_attention_bwd_deferred", deferred)
        tc, (us, ts, ue, te, vae, sc, _) = build_hip_states(case, dev, ema=True)
        batch, rand = to_dev(case["batch"], dev), to_dev(case["rand"], dev)
        rng = torch.Generator(device=dev)

        def bound(us, ts, ue, te, batch, rng, vae, sched, **extra):
            return tu.train_step(us, ts, ue, te, batch, rng, vae, sched, strip_bos_eos_token=False, ema_rate=0.999, **extra)

        step = tu._GraphedStep(bound, warmup=1) if graph else bound
        for _ in range(3):  # graph: eager, capture + replay, replay
            out = step(us, ts, ue, te, batch, rng, vae, sc, rand=rand)
        torch.cuda.synchronize()
        if graph:
            assert step.graph is not None
    snap = {"loss": out[4]["loss"].clone()}
    for name, st in (("unet", us.store), ("text", ts.store)):
        for b in ("master", "codes", "inv_scale", "ema"):
            snap[f"{name}.{b}"] = getattr(st, b).clone()
    return snap, seen


# image = 64: 8 x 8 latents, no deferred problem splits its query range.  image = 256: 32 x 32 latents, the top level's cross-attentions
# have Nq = 1024 and queue slabs of their own - eagerly and in the captured graph, where the slabs must outlive the capture.
@pytest.mark.parametrize("graph,image", [(False, 64), (True, 64), (False, 256), (True, 256)], ids=["eager", "graph", "eager-256", "graph-256"])
def test_step_with_deferrals_equals_step_without(dev, graph, image, monkeypatch):
    case = _wide_tiny_case(image)
    on, seen_on = _three_steps(dev, case, True, graph, monkeypatch)
    off, seen_off = _three_steps(dev, case, False, graph, monkeypatch)
    assert ("a queued dK/dV problem with slabs" in seen_on) == (image == 256)
    assert image == 256 or "a queued dK/dV problem without slabs" in seen_on
    assert not any(s.startswith("a queued") for s in seen_off)
    # the deferrals were really taken (and really switched off): otherwise the comparison below says nothing
    assert seen_on.count("sdt_attention_bwd_dkv_group") >= 1 and seen_on.count("sdt_colsum_batched_group") >= 1
    assert seen_on.count("sdt_attention_bwd_dq") >= 3 and seen_on.count("sdt_colsum_batched_bf16") < seen_off.count("sdt_colsum_batched_bf16")
    assert "sdt_attention_bwd_dkv_group" not in seen_off and "sdt_colsum_batched_group" not in seen_off and "sdt_attention_bwd_dq" not in seen_off
    for k in on:
        assert torch.equal(on[k], off[k]), f"{k} differs between the deferred and the inline form"
    assert torch.isfinite(on["loss"]).all()


# ------------------------------------------------------------------------------------------------ the operators, both forms
def _both_forms(monkeypatch, run):
    """run() -> {name: gradient} under ops.wgrad_grouping() and under ops.wgrad_grouping(offchain=False), the same seeded inputs
    each time; returns (gradients deferred, inline, call names deferred, inline)."""
    out = []
    real_call = ops.call
    for offchain in (True, False):
        seen = []
        with monkeypatch.context() as m:
            m.setattr(ops, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
            grads = run(offchain)
        torch.cuda.synchronize()
        out.append((grads, seen))
    (on, seen_on), (off, seen_off) = out
    assert set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), f"{k} differs between the deferred and the inline form"
        assert torch.isfinite(on[k].float()).all() and bool((on[k] != 0).any()), k
    return on, off, seen_on, seen_off


# (heads, Nq) over C = 80: head dims 40, 80 and 8 - three instantiations, the first problem splits its query range
PACKED_CONSUMERS = [(2, 1024), (1, 70), (10, 64)]


def _packed_attentions(dev, ip):
    """Three attentions over the column slices of ONE (B, 77, 3 * 2C) projection output, the middle one with a key weight; ip: the
    first consumer is ops.attention_ip with T = 4 image tokens."""
    C, T = 80, 4
    g = torch.Generator(device="cpu").manual_seed(31)
    wide0 = torch.randn(B, NK, 3 * 2 * C, generator=g).to(BF)
    qs0 = [torch.randn(B, nq, C, generator=g).to(BF) for _, nq in PACKED_CONSUMERS]
    douts = [torch.randn(B, nq, C, generator=g).to(BF).to(dev) for _, nq in PACKED_CONSUMERS]
    kv_ip0 = torch.randn(B, T, 2 * C, generator=g).to(BF)
    kw = (1.0 + torch.randint(0, 3, (NK,), generator=g).float() / 2).to(dev)

    def run(offchain):
        wide = wide0.to(dev).requires_grad_(True)
        qs = [q.to(dev).requires_grad_(True) for q in qs0]
        kv_ip = kv_ip0.to(dev).requires_grad_(True)
        slices = ops.col_slices(wide, 3)
        assert all(s.stride(1) == 3 * 2 * C for s in slices)
        outs = []
        for i, ((heads, nq), q, kv) in enumerate(zip(PACKED_CONSUMERS, qs, slices)):
            scale = (C // heads) ** -0.5
            if ip and i == 0:
                outs.append(ops.attention_ip(q, kv, kv_ip, heads, scale))
            else:
                outs.append(ops.attention_packed(q, kv, heads, scale, key_weight=kw if i == 1 else None))
        with ops.wgrad_grouping(offchain=offchain):
            torch.autograd.backward(outs, douts)
        grads = {f"dq{i}": q.grad for i, q in enumerate(qs)}
        grads["the gradient of the wide [k|v] tensor"] = wide.grad
        if ip:
            grads["kv_ip.grad"] = kv_ip.grad
        return grads

    return run


@pytest.mark.parametrize("ip", [False, True], ids=["packed", "ip_adapter"])
def test_packed_attentions_over_one_projection_in_both_forms(dev, ip, monkeypatch):
    """The step's layout: [k|v] halves at the pitch of a wider projection, dk / dv halves of a packed 2C gradient, one of the three
    problems split (slabs of its own), another with key weights - through attention_packed and, for one slice, through attention_ip."""
    lib = _lib.load()
    d = _lib.SdtAttnDesc(B, 2, 1024, NK, 40, 80, 480, 480, 80, 40 ** -0.5, 0, 80, 160, 160, 0, None)
    assert lib.sdt_attention_bwd_slab_bytes(ctypes.addressof(d)) > 0
    on, off, seen_on, seen_off = _both_forms(monkeypatch, _packed_attentions(dev, ip))
    assert seen_on.count("sdt_attention_bwd_dkv_group") == 1 and seen_on.count("sdt_attention_bwd_dq") == 3 and "sdt_attention_bwd" not in seen_on
    assert seen_off.count("sdt_attention_bwd") == 3 and "sdt_attention_bwd_dkv_group" not in seen_off and "sdt_attention_bwd_dq" not in seen_off
    assert seen_on.count("sdt_ip_attention_bwd") == seen_off.count("sdt_ip_attention_bwd") == int(ip)
    assert seen_on.index("sdt_attention_bwd_dkv_group") < seen_on.index("sdt_copy_cols_bf16")  # the flush runs in front of its reader


def test_row_biases_over_one_projection_in_both_forms(dev, monkeypatch):
    """Two convolutions whose row biases are the halves of one (B, 2 * Cout) tensor; the second runs on 9 x 9 pixels, where the column
    sum has two row blocks of 41 and 40 rows."""
    from tests import kernel_checks as kc
    from tests import op_checks as oc
    Cc, sizes = 64, (8, 9)
    plans = [kc.colsum_plan(B, hw * hw, Cc, 512) for hw in sizes]
    assert plans[0][1] == 1 and plans[1][1] == 2 and (sizes[1] ** 2) % plans[1][2] != 0, plans
    spec = [(f"c{i}/" + l, sh) for i in range(2) for l, sh in (("kernel", (3, 3, Cc, Cc)), ("bias", (Cc,)))]
    ints = oc.IntStore(spec, dev, 41, quantise=False, trainable=False)
    g = torch.Generator(device="cpu").manual_seed(37)
    wide0 = torch.randn(B, 2 * Cc, generator=g).to(BF)
    xs0 = [torch.randn(B, hw, hw, Cc, generator=g).to(BF) for hw in sizes]
    dys = [torch.randn(B, hw, hw, Cc, generator=g).to(BF).to(dev) for hw in sizes]

    def run(offchain):
        wide = wide0.to(dev).requires_grad_(True)
        xs = [x.to(dev).requires_grad_(True) for x in xs0]
        rbs = ops.col_slices(wide, 2)
        ys = [ops.conv2d(x, ints.st, f"c{i}", rowbias=rb) for i, (x, rb) in enumerate(zip(xs, rbs))]
        with ops.wgrad_grouping(offchain=offchain):
            torch.autograd.backward(ys, dys)
        return {"the gradient of the wide row-bias tensor": wide.grad, "dx0": xs[0].grad, "dx1": xs[1].grad}

    on, off, seen_on, seen_off = _both_forms(monkeypatch, run)
    assert seen_on.count("sdt_colsum_batched_group") == 1 and "sdt_colsum_batched_bf16" not in seen_on
    assert seen_off.count("sdt_colsum_batched_bf16") == 2 and "sdt_colsum_batched_group" not in seen_off
