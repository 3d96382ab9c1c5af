"""The operator layer, element by element on exact inputs, on a real MI355X (stores, references and case tables: tests/op_checks.py;
their proof on the CPU: tests/test_op_checks_cpu.py).

The kernel files pin the C ABI on raw pointers.  This file pins what stable_diffusion_training_amd/ops.py and the two grouping
helpers of nets.py make of it: leaf geometry (Rp / Cp / R / C), merged launches, where a gradient lands in the store's flat buffers
and when (immediately, from the deferred queues, with the squared-norm slots).  Masters and activations are small integers, so every
output has one right bit pattern; gradients are judged by the whole-buffer check (op_checks.expect_whole_gradient), which also sees
the neighbouring leaf, the alignment gaps and a leaf nobody wrote.

Every assertion is equality of integer views (dQ / dK of the selector cases: zero of either sign, as in the kernel file).  This file
has no tolerance."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import op_checks as oc
from tests.kernel_checks import BF, exact_ints

pytestmark = pytest.mark.gpu

# "plain": outside any context, all-fp32 gradient store; "grouped": inside ops.wgrad_grouping(), bf16 kernel gradients (grad16);
# "sq": between ops.sq_begin and ops.sq_end, grad16
MODES = ["plain", "grouped", "sq"]
G = kc.GEMM_RANGE


def _quantise(mode):
    return mode != "plain"


def _fail(msgs):
    msgs = [m for m in msgs if m]
    assert not msgs, "\n".join(msgs)


def _eq(got, want, what, tile=None):
    return kc.mismatch_report(got.detach().cpu(), want.detach().cpu(), what, tile)


def _zero_either_sign(g, what):
    b = kc.bits(g.detach().cpu()) & 0x7FFF
    n = int((b != 0).sum())
    return None if n == 0 else f"{what}: {n} elements are not zero, first at {(b != 0).nonzero()[0].tolist()}"


def _step(ints, mode, forward, dys, expected, queued, what, sq_covered=True):
    """One forward and backward of a case in a mode, with the whole-buffer check around it.  queued: the leaves whose gradient a
    wgrad_grouping context holds back (they must still hold their pre-backward contents before it closes).  Returns forward()'s outputs."""
    from stable_diffusion_training_amd import ops
    st = ints.st
    armed = oc.arm_gradient(st)
    if mode == "sq":
        ops.sq_begin(st)
    outs = forward()
    flat = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    dys = list(dys) if isinstance(dys, (tuple, list)) else [dys]
    if mode == "grouped":
        with ops.wgrad_grouping():
            torch.autograd.backward(flat, dys)
            torch.cuda.synchronize()
            oc.expect_whole_gradient(st, {p: v for p, v in expected.items() if p not in queued}, armed,
                                     f"{what}: before the context closes (queued leaves must be untouched)")
    else:
        torch.autograd.backward(flat, dys)
    if mode == "sq":
        r = ops.sq_end(st)
        if sq_covered:
            assert r is not None, f"{what}: sq_end returned None although every quantised leaf was written once"
            buf, used = r
            got, want = float(buf[:used].sum()), oc.stored_sq_sum(st, expected)
            assert got == want, f"{what}: squared-norm slots add up to {got!r}, the stored gradients to {want!r}"
        else:
            assert r is None, f"{what}: sq_end returned slots although a quantised leaf was never written"
    oc.expect_whole_gradient(st, expected, armed, what)
    return outs


# ================================================================================================ Linear
LINEAR_VARIANTS = [("bias_x", True, True, False), ("bias_x_res", True, True, True), ("nobias_res_only", False, False, True)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", LINEAR_VARIANTS, ids=[v[0] for v in LINEAR_VARIANTS])
@pytest.mark.parametrize("case", oc.LINEAR_CASES, ids=[c[0] for c in oc.LINEAR_CASES])
def test_linear(dev, case, variant, mode):
    """ops.linear with / without bias, residual and an input gradient: y at every element (pad columns +0.0), dx, the residual's
    gradient = dy bit for bit, dW / db and everything around them through the whole-buffer check.  The pad columns of x and dy hold
    non-zero integers: only the zero padding of W and K1_valid / N_valid keep them out.  The split-K shape runs twice through the
    persistent workspace, whose counters must read zero afterwards."""
    from stable_diffusion_training_amd import ops
    name, M, K, N = case
    vid, has_bias, x_grad, has_res = variant
    spec, seed, x, dy, res = oc.linear_operands(case, has_bias, has_res)
    ints = oc.IntStore(spec, dev, seed, quantise=_quantise(mode))
    Rp, Cp = oc.pad8(K), oc.pad8(N)
    want = oc.linear_expect(x, ints.w("l"), ints.b("l"), res, dy, need_dx=x_grad)
    expected = {"l/kernel": want["dW"]}
    if has_bias:
        expected["l/bias"] = want["db"]
    for run in range(2 if name == "splitk" else 1):
        xd = x.to(dev).requires_grad_(x_grad)
        rd = None if res is None else res.to(dev).requires_grad_(True)
        dyd = dy.to(dev)
        y = _step(ints, mode, lambda: ops.linear(xd, ints.st, "l", residual=rd), dyd, expected, set(expected), f"linear {name} {vid} run {run}")
        msgs = [_eq(y, want["y"], "y", tile=(64, 64)), oc.pad_columns_report(y, N, "y")]
        if x_grad:
            msgs.append(_eq(xd.grad, want["dx"], "dx", tile=(64, 64)))
        if has_res:
            msgs.append(_eq(rd.grad, dy, "residual gradient (must be dy)"))
        _fail(msgs)
    if name == "splitk":
        assert ops._WS_CACHE[(M, Cp, Rp, 1)] > 0, "the planner no longer splits this shape"
        for ws in ops._SPLITK_WS.values():
            assert int(torch.count_nonzero(ws[: kc.CNT_BYTES])) == 0, "split-K arrival counters not back at zero"


def test_linear_on_a_frozen_store(dev):
    """trainable=False: dx is right, the store holds no gradient buffer, and no launch fails."""
    from stable_diffusion_training_amd import ops
    spec, seed, x, dy, _ = oc.linear_operands(oc.LINEAR_CASES[3], True, False)
    ints = oc.IntStore(spec, dev, seed, quantise=False, trainable=False)
    assert ints.st.grad is None and ints.st.grad16 is None
    want = oc.linear_expect(x, ints.w("l"), ints.b("l"), None, dy)
    xd = x.to(dev).requires_grad_(True)
    y = ops.linear(xd, ints.st, "l")
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    _fail([_eq(y, want["y"], "y"), _eq(xd.grad, want["dx"], "dx")])
    assert ints.st.grad is None and ints.st.grad16 is None


# ================================================================================================ Linear + GroupNorm statistics
def _gn_stats_check(dev, y, stats, groups, ints, what):
    from stable_diffusion_training_amd import ops
    assert stats is not None, f"{what}: this shape no longer fuses the statistics"
    B, C = y.shape[0], y.shape[-1]
    yg = y.detach().double().reshape(B, -1, groups, C // groups)
    want = torch.stack([yg.sum((1, 3)), (yg * yg).sum((1, 3))], -1)
    assert float(want.abs().max()) < kc.LIMIT
    got = stats.double().sum(1)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} statistics differ, first (image, group, sum / sumsq) {bad[0].tolist()}"
    yd = y.detach().reshape(B, -1, C).contiguous()
    ya, yb = yd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    na = ops.group_norm(ya, ints.st, "n", groups=groups, stats=stats)
    nb = ops.group_norm(yb, ints.st, "n", groups=groups)
    torch.cuda.synchronize()
    _fail([_eq(na, nb, f"{what}: group_norm(stats=) against its own pass"),
           _eq(na.grad_fn.saved_tensors[1], nb.grad_fn.saved_tensors[1], f"{what}: saved (B, G, 2) statistics")])


def test_linear_groupnorm_statistics(dev):
    """ops.linear(gn_groups=32): the statistics the epilogue writes, summed over their parts, are the float64 sums of the stored bf16
    y; group_norm(stats=) returns and saves the same bits as with its own pass."""
    from stable_diffusion_training_amd import ops
    M, N, Kc, rpb, groups = kc.GN_DENSE_CASES[0]
    a, b, bias = kc.gn_dense_operands(M, N, Kc)
    ints = oc.IntStore([("l/kernel", (Kc, N)), ("l/bias", (N,)), ("n/scale", (N,)), ("n/bias", (N,))], dev, 11, quantise=False,
                       override={"l/kernel": b, "l/bias": bias})
    x = a.view(M // rpb, rpb, Kc).to(dev).requires_grad_(True)
    y, stats = ops.linear(x, ints.st, "l", gn_groups=groups)
    torch.cuda.synchronize()
    _fail([_eq(y.reshape(M, N), kc.expect_gemm_nt(a, b, bias), "y", tile=(64, 64))])
    _gn_stats_check(dev, y, stats, groups, ints, "linear")


def test_conv_groupnorm_statistics(dev):
    from stable_diffusion_training_amd import ops
    B, H, W, Cin, Cout, groups = kc.GN_HALO_CASES[1]
    x, w, bias = kc.gn_halo_operands(B, H, W, Cin, Cout)
    ints = oc.IntStore([("c/kernel", (3, 3, Cin, Cout)), ("c/bias", (Cout,)), ("n/scale", (Cout,)), ("n/bias", (Cout,))], dev, 12,
                       quantise=False, override={"c/kernel": w, "c/bias": bias})
    xd = x.to(dev).requires_grad_(True)
    y, stats = ops.conv2d(xd, ints.st, "c", gn_groups=groups)
    torch.cuda.synchronize()
    want = kc.epilogue_nt(kc.conv_ref64(x, w, 1, ((1, 1), (1, 1))).reshape(-1, Cout), bias)
    _fail([_eq(y.reshape(-1, Cout), want, "y")])
    _gn_stats_check(dev, y, stats, groups, ints, "conv2d")


# ================================================================================================ Linear multi
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["grouped", "interleaved"])
@pytest.mark.parametrize("case", oc.LINEAR_MULTI_CASES, ids=[c[0] for c in oc.LINEAR_MULTI_CASES])
def test_linear_multi(dev, case, layout, mode):
    """ops.linear_multi on leaves laid out back to back: y per segment, dx from the taps = n reduction, every leaf's dW and db (ONE
    dbias pointer, seg_stride from master offsets) through the whole-buffer check.  Interleaved layout: linear_multi declines and the
    per-layer path must meet the same expectations; the spacer leaves stay unwritten, so in "sq" mode sq_end must answer None."""
    from stable_diffusion_training_amd import ops
    name, M, K, N, n, bias = case
    names, seed, x, dy = oc.multi_operands(case)
    ints = oc.IntStore(oc.multi_spec(names, K, N, bias, layout), dev, seed, quantise=_quantise(mode))
    want = oc.linear_multi_expect(x, [ints.w(nm) for nm in names], [ints.b(nm) for nm in names] if bias else None, dy, per_layer=True)
    expected = {}
    for i, nm in enumerate(names):
        expected[nm + "/kernel"] = want["dW"][i]
        if bias:
            expected[nm + "/bias"] = want["db"][i]
    xd = x.to(dev).requires_grad_(True)

    def forward():
        y = ops.linear_multi(xd, ints.st, names)
        if layout == "grouped":
            assert y is not None, "linear_multi declined the grouped layout"
            return y
        assert y is None, "linear_multi accepted leaves that are not back to back"
        return [ops.linear(a, ints.st, nm) for a, nm in zip(ops.fanout(xd, n), names)]

    dyd = dy.to(dev)
    dys = dyd if layout == "grouped" else [s.contiguous() for s in oc.segments(dyd, n)]
    y = _step(ints, mode, forward, dys, expected, set(expected), f"linear_multi {name} {layout}", sq_covered=layout == "grouped")
    y = y if layout == "grouped" else torch.cat(list(y), -1)
    _fail([_eq(seg, w, f"y segment {i}") for i, (seg, w) in enumerate(zip(oc.segments(y, n), oc.segments(want["y"], n)))]
          + [_eq(xd.grad, want["dx"], "dx")])


# ================================================================================================ Conv2d
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", oc.CONV_CASES, ids=[f"{c[3]}to{c[4]}_k{c[5]}s{c[6]}_{c[1]}x{c[2]}_{i}" for i, c in enumerate(oc.CONV_CASES)])
def test_conv2d(dev, case, mode):
    """ops.conv2d with bias, residual and a row bias that is the middle column slice (stride(0) = 3 * Cp) of a wider tensor whose
    neighbouring slices hold other integers: y and dx at every pixel, dW (all taps) / db / the gaps through the whole-buffer check,
    drb = bf16 of the per-image column sums, the residual's gradient = dy bit for bit.  Pad channels of x and dy are non-zero."""
    from stable_diffusion_training_amd import ops
    B, H, W, Cin, Cout, k, stride, pad = case
    spec, seed, x, dy, res, rb, wide = oc.conv_operands(case)
    ints = oc.IntStore(spec, dev, seed, quantise=_quantise(mode))
    Cp = oc.pad8(Cout)
    want = oc.conv_expect(x, ints.w("c"), ints.b("c"), rb, res, dy, stride, pad)
    expected = {"c/kernel": want["dW"], "c/bias": want["db"]}
    xd, rd, wd = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True), wide.to(dev).requires_grad_(True)
    rbd = wd[:, Cp: 2 * Cp]
    assert rbd.stride(0) == 3 * Cp
    y = _step(ints, mode, lambda: ops.conv2d(xd, ints.st, "c", stride=stride, pad=pad, rowbias=rbd, residual=rd), dy.to(dev), expected,
              set(expected), f"conv2d {case}")
    want_wide = torch.zeros(B, 3 * Cp, dtype=BF)
    want_wide[:, Cp: 2 * Cp] = want["drb"]
    _fail([_eq(y, want["y"], "y [image][row][column][channel]"), oc.pad_columns_report(y, Cout, "y"),
           _eq(xd.grad, want["dx"], "dx [image][row][column][channel]"), _eq(rd.grad, dy, "residual gradient (must be dy)"),
           _eq(wd.grad, want_wide, "gradient of the wide row-bias tensor [image][3 * Cp]: drb in slice 1, +0.0 beside it")])


# ================================================================================================ grouping limits
def test_grouping_limits(dev):
    """33 Dense layers, 9 convolutions and 3 LayerNorms run backward in ONE wgrad_grouping context: the dense queue flushes at
    WGRAD_GROUP_LIMIT with a job left over, the conv queue at CONV_GROUP_LIMIT with one left over, the norm queue when the context
    closes.  Every leaf holds its reference, store._written names every leaf exactly once, and a second backward through a layer
    without a new zero_grad() is refused."""
    from stable_diffusion_training_amd import _lib, ops
    lib = _lib.load()
    assert len(oc.GROUP_DENSE) > min(ops.WGRAD_GROUP_LIMIT, lib.sdt_gemm_tn_wgrad_group_max())
    assert len(oc.GROUP_CONVS) > min(ops.CONV_GROUP_LIMIT, lib.sdt_gemm_tn_wgrad_group_max())
    spec, M = [], oc.GROUP_M
    for i, (K, N) in enumerate(oc.GROUP_DENSE):
        spec += [(f"d{i}/kernel", (K, N)), (f"d{i}/bias", (N,))]
    for i, (B, H, W, Cin, Cout) in enumerate(oc.GROUP_CONVS):
        spec += [(f"c{i}/kernel", (3, 3, Cin, Cout)), (f"c{i}/bias", (Cout,))]
    ln_cases, affine = [], {}
    for i, (cid, shift) in enumerate(oc.GROUP_LN):
        _, Mr, C = kc.ln_case(cid)
        case = kc.layernorm_balanced_case(Mr, C, 900 + shift)
        ln_cases.append(case)
        affine[f"n{i}"] = (case["gamma"], case["beta"])
        spec += [(f"n{i}/scale", (C,)), (f"n{i}/bias", (C,))]
    ints = oc.IntStore(spec, dev, 13, quantise=True, norm_affine=affine)
    st = ints.st
    outs, dys, expected, checks = [], [], {}, []
    armed = oc.arm_gradient(st)
    for i, (K, N) in enumerate(oc.GROUP_DENSE):
        x, dy = exact_ints((M, K), -G, G, 2000 + i), exact_ints((M, N), -G, G, 3000 + i)
        want = oc.linear_expect(x, ints.w(f"d{i}"), ints.b(f"d{i}"), None, dy)
        expected[f"d{i}/kernel"], expected[f"d{i}/bias"] = want["dW"], want["db"]
        xd = x.to(dev).requires_grad_(True)
        outs.append(ops.linear(xd, st, f"d{i}"))
        dys.append(dy.to(dev))
        checks.append((f"d{i}", outs[-1], want["y"], xd, want["dx"]))
    for i, (B, H, W, Cin, Cout) in enumerate(oc.GROUP_CONVS):
        x, dy = exact_ints((B, H, W, Cin), -G, G, 4000 + i), exact_ints((B, H, W, Cout), -G, G, 5000 + i)
        want = oc.conv_expect(x, ints.w(f"c{i}"), ints.b(f"c{i}"), None, None, dy, 1, 1)
        expected[f"c{i}/kernel"], expected[f"c{i}/bias"] = want["dW"], want["db"]
        xd = x.to(dev).requires_grad_(True)
        outs.append(ops.conv2d(xd, st, f"c{i}"))
        dys.append(dy.to(dev))
        checks.append((f"c{i}", outs[-1], want["y"], xd, want["dx"]))
    for i, case in enumerate(ln_cases):
        exp = kc.norm_exact_expectation(case, 0, 0.0)
        expected[f"n{i}/scale"], expected[f"n{i}/bias"] = exp["dgamma"], exp["dbeta"]
        xd = case["x"].to(dev).requires_grad_(True)
        outs.append(ops.layer_norm(xd, st, f"n{i}", eps=0.0))
        dys.append(case["dy"].to(dev))
        checks.append((f"n{i}", outs[-1], exp["y"], xd, exp["dx"]))
    with ops.wgrad_grouping():
        torch.autograd.backward(outs, dys, retain_graph=True)
        torch.cuda.synchronize()
        # what a full queue has flushed is there, what is still queued is untouched: every leaf is either right or as zero_grad() left it
        flushed = {p: v for p, v in expected.items() if p in st._written}
        assert 0 < len(flushed) < len(expected)
        oc.expect_whole_gradient(st, flushed, armed, "before the context closes")
    oc.expect_whole_gradient(st, expected, armed, "after the context closed")
    assert st._written == set(st.leaves), f"not reported: {sorted(set(st.leaves) - st._written)}"
    _fail([m for nm, y, wy, xd, wdx in checks for m in (_eq(y, wy.view(y.shape), f"{nm}: y"), _eq(xd.grad, wdx.view(xd.shape), f"{nm}: dx"))])
    with pytest.raises(RuntimeError, match="produced twice"):
        outs[0].backward(dys[0])


# ================================================================================================ norm operators
def _norm_store(dev, case, C, mode, trainable=True):
    return oc.IntStore([("n/scale", (C,)), ("n/bias", (C,))], dev, 17, quantise=False, trainable=trainable,
                       norm_affine={"n": (case["gamma"], case["beta"])})


@pytest.mark.parametrize("mode", ["plain", "grouped"])
def test_group_norm_skip(dev, mode):
    """ops.group_norm(skip=True) on a balanced case in the exact regime (count a power of two, eps = 0): y, dx with the skip branch's
    gradient folded in (dres: two roundings), dgamma / dbeta added onto what zero_grad() left - GroupNorm parameters are never
    deferred, so inside a grouping context they are there before it closes."""
    from stable_diffusion_training_amd import ops
    cid = oc.GN_EXACT_CASE
    _, B, HW, C, groups = kc.gn_case(cid)
    case = kc.gn_balanced(cid)
    assert kc.is_pow2(case["cnt"])
    exp = kc.norm_exact_expectation(case, groups, 0.0)
    ints = _norm_store(dev, case, C, mode)
    xd = case["x"].to(dev).requires_grad_(True)
    expected = {"n/scale": exp["dgamma"], "n/bias": exp["dbeta"]}
    y, _ = _step(ints, mode, lambda: ops.group_norm(xd, ints.st, "n", groups=groups, eps=0.0, skip=True),
                 [case["dy"].to(dev), case["dres"].to(dev)], expected, set(), f"group_norm {cid}")
    _fail([_eq(y, exp["y"], "y"), _eq(xd.grad, exp["dx_dres"], "dx (+ skip gradient)")])


def test_group_norm_skip_straddling_groups_frozen(dev):
    """The smallest balanced row whose 8-wide vectors straddle groups (3 channels per group, count 108, eps = 1e-5): y and dx with the
    skip gradient in every bit.  Its dgamma / dbeta are not exact at a count that is no power of two (tests/test_gpu_norm_exact.py
    holds them to the per-channel rule), so this row runs on a frozen store: dx only, no gradient buffer."""
    from stable_diffusion_training_amd import ops
    cid = oc.GN_OP_CASE
    _, B, HW, C, groups = kc.gn_case(cid)
    case = kc.gn_balanced(cid)
    exp = kc.norm_exact_expectation(case, groups, 1e-5)
    ints = _norm_store(dev, case, C, "plain", trainable=False)
    xd = case["x"].to(dev).requires_grad_(True)
    y, xs = ops.group_norm(xd, ints.st, "n", groups=groups, eps=1e-5, skip=True)
    torch.autograd.backward([y, xs], [case["dy"].to(dev), case["dres"].to(dev)])
    torch.cuda.synchronize()
    _fail([_eq(y, exp["y"], "y"), _eq(xd.grad, exp["dx_dres"], "dx (+ skip gradient)")])
    assert ints.st.grad is None


@pytest.mark.parametrize("mode", ["plain", "grouped"])
def test_layer_norm_skip(dev, mode):
    """ops.layer_norm(skip=True): immediately, and deferred through flush_norm_grads when a grouping context closes (until then
    dgamma / dbeta hold what zero_grad() left)."""
    from stable_diffusion_training_amd import ops
    cid = oc.LN_OP_CASE
    _, M, C = kc.ln_case(cid)
    case = kc.ln_balanced(cid)
    exp = kc.norm_exact_expectation(case, 0, 0.0)
    ints = _norm_store(dev, case, C, mode)
    xd = case["x"].to(dev).requires_grad_(True)
    expected = {"n/scale": exp["dgamma"], "n/bias": exp["dbeta"]}
    y, _ = _step(ints, mode, lambda: ops.layer_norm(xd, ints.st, "n", eps=0.0, skip=True), [case["dy"].to(dev), case["dres"].to(dev)],
                 expected, set(expected), f"layer_norm {cid}")
    _fail([_eq(y, exp["y"], "y"), _eq(xd.grad, exp["dx_dres"], "dx (+ skip gradient)")])


# ================================================================================================ attention operators
def _attn_run(dev, form, q, k, v, do, H, scale, causal=False, key_weight=None):
    """out, dq, dk, dv (bf16, host) of one attention form; "slice": also the gathered gradient of the wide tensor."""
    from stable_diffusion_training_amd import ops
    B, Nq, C = q.shape
    Nk = k.shape[1]
    extra = {}
    if form == "plain":
        qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
        out = ops.attention(qd, kd, vd, H, scale, causal, key_weight)
        out.backward(do.to(dev))
        dq, dk, dv = qd.grad, kd.grad, vd.grad
    elif form == "packed_self":
        a = torch.cat([q, k, v], -1).to(dev).requires_grad_(True)
        out = ops.attention_packed(a, None, H, scale, causal, key_weight)
        out.backward(do.to(dev))
        dq, dk, dv = a.grad[..., :C], a.grad[..., C: 2 * C], a.grad[..., 2 * C:]
    else:
        wide = torch.full((B, Nk, 3 * 2 * C), float("nan"), dtype=BF)
        wide[..., 2 * C: 4 * C] = torch.cat([k, v], -1)
        wd = wide.to(dev).requires_grad_(True)
        qd = q.to(dev).requires_grad_(True)
        b = ops.col_slices(wd, 3)[1]
        assert b.stride(1) == 6 * C
        out = ops.attention_packed(qd, b, H, scale, causal, key_weight)
        out.backward(do.to(dev))
        dq, dk, dv = qd.grad, wd.grad[..., 2 * C: 3 * C], wd.grad[..., 3 * C: 4 * C]
        extra["outer"] = torch.cat([wd.grad[..., : 2 * C], wd.grad[..., 4 * C:]], -1)
    torch.cuda.synchronize()
    return dict(o=out.detach().cpu(), dq=dq.contiguous().cpu(), dk=dk.contiguous().cpu(), dv=dv.contiguous().cpu(),
                **{n: t.contiguous().cpu() for n, t in extra.items()})


def _outer_zero(got):
    if "outer" not in got:
        return None
    return kc.mismatch_report(got["outer"], torch.zeros_like(got["outer"]), "slices 0 and 2 of the wide gradient (no consumer: +0.0)")


@pytest.mark.parametrize("form", ["plain", "packed_self", "slice"])
def test_attention_selector(dev, form):
    """Selector inputs through ops.attention, the packed [q|k|v] form and the [k|v] column slice of a wider tensor (pitch 6C, the
    other slices NaN; the gradient pitch ldg = 2C differs from ldkv): out the selected V rows, dV the integer sums, dQ = dK = 0."""
    p = oc.ATTN_OP
    B, H, D, Nq = p["B"], p["H"], p["D"], p["Nq"]
    Nk = Nq if form == "packed_self" else p["Nk"]
    scale = D ** -0.5
    case = kc.selector_case(B, H, Nq, Nk, D, False, seed=41)
    want_o, _, want_dv = kc.selector_expect(case, B, H, Nq, Nk, D, scale)
    got = _attn_run(dev, form, case["q"], case["k"], case["v"], case["dout"], H, scale)
    _fail([_eq(got["o"], want_o, "out", tile=(128, D)), _eq(got["dv"], want_dv, "dv", tile=(128, D)),
           _zero_either_sign(got["dq"], "dq"), _zero_either_sign(got["dk"], "dk"), _outer_zero(got)])


@pytest.mark.parametrize("form", ["plain", "packed_self", "slice"])
def test_attention_tied_pairs(dev, form):
    """Tied-pair inputs (exact non-zero dQ and dK) through the three forms."""
    p = oc.ATTN_OP
    B, H, D, Nq = p["B"], p["H"], p["D"], p["Nq"]
    Nk = Nq if form == "packed_self" else p["Nk"]
    scale = D ** -0.5
    case = kc.pair_case(B, H, Nq, Nk, D, seed=43)
    want = kc.pair_expect(case, B, H, Nq, Nk, D, scale)
    got = _attn_run(dev, form, case["q"], case["k"], case["v"], case["dout"], H, scale)
    _fail(kc.pair_reports(got, want, D) + [_outer_zero(got)])


@pytest.mark.parametrize("form,causal,kw", [("plain", True, False), ("slice", False, True), ("plain", False, True)])
def test_attention_causal_and_key_weight(dev, form, causal, kw):
    p = oc.ATTN_OP
    B, H, D, Nq, Nk = p["B"], p["H"], p["D"], p["Nq"], p["Nk"]
    scale = D ** -0.5
    case = kc.selector_case(B, H, Nq, Nk, D, causal, seed=47)
    w = (1.0 + (torch.arange(Nk) % 3 == 1).float()).contiguous() if kw else None
    want_o, _, want_dv = kc.selector_expect(case, B, H, Nq, Nk, D, scale, w)
    got = _attn_run(dev, form, case["q"], case["k"], case["v"], case["dout"], H, scale, causal, None if w is None else w.to(dev))
    _fail([_eq(got["o"], want_o, "out", tile=(128, D)), _eq(got["dv"], want_dv, "dv", tile=(128, D)),
           _zero_either_sign(got["dq"], "dq"), _zero_either_sign(got["dk"], "dk"), _outer_zero(got)])


# ================================================================================================ glue helpers
@pytest.mark.parametrize("mode", MODES)
def test_time_emb_projections(dev, mode):
    """nets._time_emb_projections on the grouped layout: every row bias is a column slice (pitch n * C) of ONE GEMM's output; the
    backward runs through the convolutions that consume them: drb per block, the gathered gradient through ONE input-gradient and
    ONE weight-gradient GEMM - temb's gradient and every projection leaf's dW and db."""
    from stable_diffusion_training_amd import nets, ops
    B, T, C, n, hw = 2, 64, 64, 3, 8
    names = [f"r{i}" for i in range(n)]
    spec = ([(nm + "/conv1/" + l, sh) for nm in names for l, sh in (("kernel", (3, 3, C, C)), ("bias", (C,)))]
            + [(nm + "/time_emb_proj/kernel", (T, C)) for nm in names] + [(nm + "/time_emb_proj/bias", (C,)) for nm in names])
    ints = oc.IntStore(spec, dev, 19, quantise=_quantise(mode))
    temb = exact_ints((B, T), -G, G, 1)
    xs = [exact_ints((B, hw, hw, C), -G, G, 10 + i) for i in range(n)]
    dys = [exact_ints((B, hw, hw, C), -G, G, 20 + i) for i in range(n)]
    expected, want_rb, want_y, want_dx, acc = {}, [], [], [], 0
    for i, nm in enumerate(names):
        wt, bt = ints.w(nm + "/time_emb_proj"), ints.b(nm + "/time_emb_proj")
        rb = kc.expect_gemm_nt(temb, wt, bias=bt)
        cv = oc.conv_expect(xs[i], ints.w(nm + "/conv1"), ints.b(nm + "/conv1"), rb, None, dys[i], 1, 1)
        drb = cv["drb"].double()
        expected.update({nm + "/conv1/kernel": cv["dW"], nm + "/conv1/bias": cv["db"],
                         nm + "/time_emb_proj/kernel": temb.double().t() @ drb + 0.0, nm + "/time_emb_proj/bias": drb.sum(0) + 0.0})
        acc = acc + drb @ wt.t()
        want_rb.append(rb), want_y.append(cv["y"]), want_dx.append(cv["dx"])
    td = temb.to(dev).requires_grad_(True)
    xds = [x.to(dev).requires_grad_(True) for x in xs]
    got = {}

    def forward():
        rbs = nets._time_emb_projections(ints.st, td)
        assert set(rbs) == set(names) and all(rbs[nm].stride(0) == n * C for nm in names), "not column slices of one GEMM's output"
        got["rb"] = [rbs[nm].detach().clone() for nm in names]
        return [ops.conv2d(x, ints.st, nm + "/conv1", rowbias=rbs[nm]) for x, nm in zip(xds, names)]

    ys = _step(ints, mode, forward, [d.to(dev) for d in dys], expected, set(expected), "time_emb_projections")
    msgs = [_eq(td.grad, kc.rne_bf16(acc + 0.0), "gradient of temb")]
    for i in range(n):
        msgs += [_eq(got["rb"][i], want_rb[i], f"row bias {i}"), _eq(ys[i], want_y[i], f"y {i}"), _eq(xds[i].grad, want_dx[i], f"dx {i}")]
    _fail(msgs)


@pytest.mark.parametrize("mode", MODES)
def test_context_projections(dev, mode):
    """nets._context_projections on the grouped layout: every block's [k|v] is a column slice (pitch n * 2C) of ONE GEMM over the
    context; the attention consumers read it through attention_packed and their [dk|dv] are gathered for ONE input-gradient and ONE
    weight-gradient GEMM.  Selector construction with projected keys (op_checks.context_selector_case)."""
    from stable_diffusion_training_amd import nets, ops
    B, Nk, cd, C, heads, n, Nq = 2, 77, 72, 64, 2, 2, 40
    names = [f"b{i}/attn2" for i in range(n)]
    spec = [(nm + "/" + l + "/kernel", (cd, C)) for nm in names for l in ("to_k", "to_v")]
    case = oc.context_selector_case(B, Nq, Nk, cd, C, heads, n, seed=23)
    ints = oc.IntStore(spec, dev, 29, quantise=_quantise(mode), override={nm + "/to_k/kernel": case["wk"] for nm in names})
    want = oc.context_selector_expect(case, [ints.w(nm + "/to_v") for nm in names], heads)
    expected = {}
    for i, nm in enumerate(names):
        expected[nm + "/to_k/kernel"], expected[nm + "/to_v/kernel"] = want["dWk"][i], want["dWv"][i]
    cx = case["ctx"].to(dev).requires_grad_(True)
    qds = [q.to(dev).requires_grad_(True) for q in case["q"]]
    got = {}

    def forward():
        kv = nets._context_projections(ints.st, cx)
        assert set(kv) == set(names) and all(isinstance(v, nets._PackedKV) and v.kv.stride(1) == n * 2 * C for v in kv.values())
        got["kv"] = [kv[nm].kv.detach().clone() for nm in names]
        return [ops.attention_packed(q, kv[nm].kv, heads, (C // heads) ** -0.5) for q, nm in zip(qds, names)]

    outs = _step(ints, mode, forward, [d.to(dev) for d in case["dout"]], expected, set(expected), "context_projections")
    msgs = [_eq(cx.grad, want["dctx"], "gradient of ctx")]
    for i in range(n):
        msgs += [_eq(got["kv"][i], want["kv"][i], f"[k|v] slice {i}"), _eq(outs[i], want["out"][i], f"out {i}"),
                 _zero_either_sign(qds[i].grad, f"dq {i}")]
    _fail(msgs)


# ================================================================================================ movement operators
def test_upsample_concat_add(dev):
    from stable_diffusion_training_amd import ops
    x = exact_ints((2, 5, 7, 16), -G, G, 1)
    dy = exact_ints((2, 10, 14, 16), -G, G, 2)
    xd = x.to(dev).requires_grad_(True)
    y = ops.upsample2x(xd)
    y.backward(dy.to(dev))
    msgs = [_eq(y, x.repeat_interleave(2, 1).repeat_interleave(2, 2), "upsample2x: y"), _eq(xd.grad, oc.upsample_bwd_expect(dy), "upsample2x: dx")]
    a, b = exact_ints((3, 11, 24), -G, G, 3), exact_ints((3, 11, 40), -G, G, 4)
    dc = exact_ints((3, 11, 64), -G, G, 5)
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    c = ops.concat_channels(ad, bd)
    c.backward(dc.to(dev))
    msgs += [_eq(c, torch.cat([a, b], -1), "concat_channels: y"), _eq(ad.grad, dc[..., :24], "concat_channels: da"),
             _eq(bd.grad, dc[..., 24:], "concat_channels: db")]
    p, q = exact_ints((77, 24), -100, 100, 6), exact_ints((77, 24), -100, 100, 7)
    ds = exact_ints((77, 24), -G, G, 8)
    pd, qd = p.to(dev).requires_grad_(True), q.to(dev).requires_grad_(True)
    s = ops.add(pd, qd)
    s.backward(ds.to(dev))
    torch.cuda.synchronize()
    msgs += [_eq(s, kc.rne_bf16(p.double() + q.double()), "add: y"), _eq(pd.grad, ds, "add: da"), _eq(qd.grad, ds, "add: db")]
    _fail(msgs)


@pytest.mark.parametrize("n,silent", oc.FANOUT_CASES)
def test_fanout(dev, n, silent):
    """ops.fanout: the n gradients summed in one pass; consumers that give no gradient are skipped; n = 40 chains a second launch
    onto the bf16 running sum of the first 31 (|sum| <= 256 at every prefix, so that store is exact)."""
    from stable_diffusion_training_amd import ops
    shape = (13, 24)
    gs, tot = oc.fanout_grads(shape, n, silent, 70 + n)
    xd = exact_ints(shape, -G, G, 1).to(dev).requires_grad_(True)
    outs = ops.fanout(xd, n)
    assert len(outs) == n
    live = [i for i in range(n) if gs[i] is not None]
    torch.autograd.backward([outs[i] for i in live], [gs[i].to(dev) for i in live])
    torch.cuda.synchronize()
    _fail([_eq(xd.grad, kc.rne_bf16(tot), f"fanout n = {n}: summed gradient")])


def test_embedding(dev):
    """ops.embedding: token + position rows; the backward adds repeated ids (the padding id fills most of a sequence) and the
    position rows of every sequence onto what zero_grad() left."""
    from stable_diffusion_training_amd import ops
    S, D, nseq, vocab = kc.EMB_S, 48, 3, 300
    ints = oc.IntStore([("tok/embedding", (vocab, D)), ("pos/embedding", (S, D))], dev, 31, quantise=False)
    ids = kc.embedding_ids("clip", nseq, vocab, 5).view(nseq, S)
    dout = exact_ints((nseq, S, D), -G, G, 6)
    tok, pos = ints.w64["tok/embedding"], ints.w64["pos/embedding"]
    want = kc.rne_bf16(tok[ids.long()] + pos[None])
    dtok = torch.zeros(vocab, D, dtype=torch.float64).index_add_(0, ids.reshape(-1).long(), dout.double().reshape(-1, D))
    expected = {"tok/embedding": dtok, "pos/embedding": dout.double().sum(0)}
    anchor = torch.zeros(1, device=dev, requires_grad=True)
    idd = ids.to(dev).contiguous()
    out = _step(ints, "plain", lambda: ops.embedding(idd, ints.st, "tok/embedding", "pos/embedding", S, anchor), dout.to(dev), expected, set(),
                "embedding")
    _fail([_eq(out, want, "embedding rows")])
