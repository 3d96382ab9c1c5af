"""The proof that tests/test_gpu_ops_exact.py would fail on a subtly wrong operator layer, without breaking the layer on a GPU (the
pattern of tests/test_kernel_checks_cpu.py):
  - the arithmetic: on the very operands of every case, each sum the references take for exact is an integer below 2^24, and every
    value claimed exact in bf16 is (fan-in sums, the row-bias gradients that travel on, the upsample backward, the tied pairs);
  - independence: the references of tests/op_checks.py equal float64 torch.autograd of the plain PyTorch ops (F.linear, F.conv2d on
    NCHW with explicit padding, torch.cat, repeat_interleave, softmax attention) on the UNPADDED tensors, rounded at the documented
    points - they do not restate ops.py;
  - planted defects: one element one bf16 ulp off, the next leaf's first element touched, a word in an alignment gap, a pad column of
    y, two segments of a merged gradient exchanged, the row-bias gradients of two images exchanged, a leaf left at its sentinel: each
    is reported with its coordinates;
  - the fused feed-forward kernel's ragged M values are what the planner says today."""
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_checks as kc
from tests import op_checks as oc

BF = torch.bfloat16
CPU = torch.device("cpu")


def _int_below_limit(v, what):
    assert torch.equal(v, v.round()) and float(v.abs().max()) < kc.LIMIT, f"{what}: not an integer below 2^24"


# ================================================================================================ exactness
def test_stated_bounds_stay_below_2_pow_24():
    for what, bound in oc.exact_bounds():
        assert bound < kc.LIMIT, what


@pytest.mark.parametrize("case", oc.LINEAR_CASES, ids=[c[0] for c in oc.LINEAR_CASES])
def test_linear_cases_are_exact_on_their_operands(case):
    name, M, K, N = case
    spec, seed, x, dy, res = oc.linear_operands(case)
    ints = oc.IntStore(spec, CPU, seed, quantise=True)
    Wp = oc.pad_weight(ints.w("l"), oc.pad8(K), oc.pad8(N)).abs()
    _int_below_limit(x.double().abs() @ Wp + oc.pad_last(ints.b("l"), oc.pad8(N)).abs() + res.double().abs(), "sum |x||W| + |b| + |res|")
    _int_below_limit(dy.double().abs() @ Wp.t(), "sum |dy||W|")
    _int_below_limit(x.double().abs().t() @ dy.double().abs(), "sum |x||dy|")
    # the pad columns of the operands ARE non-zero where the leaf is padded: the result must not rest on the caller's zeros
    if oc.pad8(K) != K:
        assert bool((x[:, K:] != 0).all())
    if oc.pad8(N) != N:
        assert bool((dy[:, N:] != 0).all()) and bool((res[:, N:] == 0).all())
    assert ints.st.leaves["l/kernel"].numel % ints.st.block_size == 0


@pytest.mark.parametrize("case", oc.CONV_CASES, ids=[str(i) for i in range(len(oc.CONV_CASES))])
def test_conv_cases_are_exact_on_their_operands(case):
    B, H, W, Cin, Cout, k, stride, pad = case
    spec, seed, x, dy, res, rb, wide = oc.conv_operands(case)
    ints = oc.IntStore(spec, CPU, seed, quantise=True)
    Wp = oc.pad_weight(ints.w("c"), oc.pad8(Cin), oc.pad8(Cout)).abs()
    p = kc.norm_pad(pad)
    _int_below_limit(kc.conv_ref64(x.abs(), Wp, stride, p), "sum |x||W|")
    _int_below_limit(kc.conv_dgrad_ref64(dy.abs(), Wp, (H, W), stride, p), "sum |dy||W|")
    _int_below_limit(kc.conv_wgrad_ref64(x.abs(), dy.abs(), (k, k), stride, p), "sum |x||dy|")
    _int_below_limit(oc.per_image_colsum(dy.abs(), B), "per-image column sums")
    Cp = oc.pad8(Cout)
    assert torch.equal(wide[:, Cp: 2 * Cp], rb) and bool((wide[:, :Cp] != 0).all()) and bool((wide[:, 2 * Cp:] != 0).all())
    lf = ints.st.leaves["c/kernel"]
    assert (lf.R, lf.C, lf.Rp, lf.Cp) == (Cin, Cout, oc.pad8(Cin), Cp) and (lf.w_off >= ints.st.total) == ((lf.Rp, lf.Cp) != (lf.R, lf.C))


@pytest.mark.parametrize("case", oc.LINEAR_MULTI_CASES, ids=[c[0] for c in oc.LINEAR_MULTI_CASES])
def test_linear_multi_cases_layouts_and_per_layer_path(case):
    """Both layouts are what they claim in both store variants, and the per-layer input gradients are exact in bf16, so the
    interleaved layout's path must meet the merged launch's expectation."""
    name, M, K, N, n, bias = case
    names, seed, x, dy = oc.multi_operands(case)
    for quantise in (False, True):
        for layout in ("grouped", "interleaved"):
            ints = oc.IntStore(oc.multi_spec(names, K, N, bias, layout), CPU, seed, quantise=quantise)
            wp = tuple(nm + "/kernel" for nm in names)
            bp = tuple(nm + "/bias" for nm in names) if bias else None
            assert ints.st.mergeable(wp, bp) == (layout == "grouped"), (quantise, layout)
    ints = oc.IntStore(oc.multi_spec(names, K, N, bias, "grouped"), CPU, seed, quantise=True)
    want = oc.linear_multi_expect(x, [ints.w(nm) for nm in names], [ints.b(nm) for nm in names] if bias else None, dy, per_layer=True)
    assert float(want["dx"].double().abs().max()) <= 256
    # segment bookkeeping: the merged launch's seg_stride is the distance between two leaves' master offsets
    lfs = [ints.st.leaves[nm + "/kernel"] for nm in names]
    assert all(b.offset - a.offset == K * N for a, b in zip(lfs, lfs[1:]))


def test_values_claimed_exact_in_bf16_are():
    for n, silent in oc.FANOUT_CASES:
        gs, tot = oc.fanout_grads((13, 24), n, silent, 70 + n)
        run = torch.zeros(13, 24, dtype=torch.float64)
        for g in gs:
            if g is not None:
                run = run + g.double()
                assert float(run.abs().max()) <= 256 and torch.equal(kc.rne_bf16(run).double(), run)  # every prefix: the chained store is exact
        assert torch.equal(run, tot) and sum(g is not None for g in gs) == n - len(silent)
    assert sum(g is not None for g in oc.fanout_grads((1, 8), 40, (0, 17), 1)[0]) > 31 >= sum(g is not None for g in oc.fanout_grads((1, 8), 32, (5,), 1)[0])
    dy = kc.exact_ints((2, 10, 14, 16), -3, 3, 2)
    up = oc.upsample_bwd_expect(dy)
    assert torch.equal(up.double(), dy.double().view(2, 5, 2, 7, 2, 16).sum((2, 4)))
    p = oc.ATTN_OP
    for Nk in (p["Nq"], p["Nk"]):  # pair_expect asserts P.V, P^T.dO, dS exact in bf16 and the accumulators exact in fp32
        case = kc.pair_case(p["B"], p["H"], p["Nq"], Nk, p["D"], seed=43)
        kc.pair_expect(case, p["B"], p["H"], p["Nq"], Nk, p["D"], p["D"] ** -0.5)
        tie, lead, _ = kc.pair_min_gap(case, p["B"], p["H"], p["Nq"], Nk, p["D"], p["D"] ** -0.5)
        assert tie == 0.0 and lead > 100
    for causal, Nk in ((False, p["Nk"]), (False, p["Nq"]), (True, p["Nk"])):
        case = kc.selector_case(p["B"], p["H"], p["Nq"], Nk, p["D"], causal, seed=47)
        gap, _ = kc.selector_min_gap(case, p["B"], p["H"], p["Nq"], Nk, p["D"], p["D"] ** -0.5)
        assert gap > 100  # every other probability underflows in fp32


def test_time_emb_row_bias_gradients_travel_on_exactly():
    """drb of the glue case is exact in bf16 (|column sum| <= 3 * 64 = 192 <= 256), so the merged backward consumes integers."""
    B, hw, C = 2, 8, 64
    for i in range(3):
        dy = kc.exact_ints((B, hw, hw, C), -3, 3, 20 + i)
        s = oc.per_image_colsum(dy, B)
        assert float(s.abs().max()) <= 256 and torch.equal(kc.rne_bf16(s).double(), s)


def test_grouping_tables_cross_the_limits():
    from stable_diffusion_training_amd import ops
    assert len(set(oc.GROUP_DENSE)) == len(oc.GROUP_DENSE) == 33 > ops.WGRAD_GROUP_LIMIT
    assert all(8 <= K <= 72 and 8 <= N <= 136 and K % 8 == 0 and N % 8 == 0 for K, N in oc.GROUP_DENSE)
    assert len(oc.GROUP_CONVS) == 9 > ops.CONV_GROUP_LIMIT and len(oc.GROUP_LN) == 3
    assert kc.is_pow2(kc.gn_balanced(oc.GN_EXACT_CASE)["cnt"]) and not kc.is_pow2(kc.gn_balanced(oc.GN_OP_CASE)["cnt"])


# ================================================================================================ independence
def _autograd_linear(x, w64, b64, res, dy):
    """float64 torch.autograd of the plain op on the UNPADDED tensors, rounded where the kernels round."""
    R, C = w64.shape
    xa = x[:, :R].double().requires_grad_(True)
    wa = w64.clone().requires_grad_(True)
    ba = b64.clone().requires_grad_(True)
    acc = F.linear(xa, wa.t(), ba)
    acc.backward(dy[:, :C].double())
    y = kc.rne_bf16(kc.rne_bf16(acc.detach()).double() + res[:, :C].double())
    return y, kc.rne_bf16(xa.grad), wa.grad, ba.grad


@pytest.mark.parametrize("case", [oc.LINEAR_CASES[1], oc.LINEAR_CASES[3], oc.LINEAR_CASES[4]], ids=lambda c: c[0])
def test_linear_reference_is_autograd_of_the_plain_op(case):
    name, M, K, N = case
    spec, seed, x, dy, res = oc.linear_operands(case)
    ints = oc.IntStore(spec, CPU, seed, quantise=False)
    want = oc.linear_expect(x, ints.w("l"), ints.b("l"), res, dy)
    y, dx, dW, db = _autograd_linear(x, ints.w("l"), ints.b("l"), res, dy)
    assert torch.equal(kc.bits(want["y"][:, :N]), kc.bits(y)) and kc.mismatch_report(want["y"][:, N:], torch.zeros(M, oc.pad8(N) - N, dtype=BF), "pad") is None
    assert torch.equal(kc.bits(want["dx"][:, :K]), kc.bits(dx)) and int((kc.bits(want["dx"][:, K:]) != 0).sum()) == 0
    assert torch.equal(want["dW"], dW) and torch.equal(want["db"], db)


@pytest.mark.parametrize("case", [oc.CONV_CASES[2], oc.CONV_CASES[3], oc.CONV_CASES[5], oc.CONV_CASES[9]], ids=lambda c: f"{c[3]}to{c[4]}k{c[5]}s{c[6]}")
def test_conv_reference_is_autograd_of_the_plain_op(case):
    B, H, W, Cin, Cout, k, stride, pad = case
    spec, seed, x, dy, res, rb, wide = oc.conv_operands(case)
    ints = oc.IntStore(spec, CPU, seed, quantise=False)
    want = oc.conv_expect(x, ints.w("c"), ints.b("c"), rb, res, dy, stride, pad)
    (pt, pb), (pl, pr) = kc.norm_pad(pad)
    xa = x[..., :Cin].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)                     # NCHW
    wa = ints.w("c").permute(3, 2, 0, 1).contiguous().requires_grad_(True)                                # HWIO -> OIHW
    ba = ints.b("c").clone().requires_grad_(True)
    rba = rb[:, :Cout].double().requires_grad_(True)
    acc = F.conv2d(F.pad(xa, (pl, pr, pt, pb)), wa, ba, stride=stride)
    y1 = kc.rne_bf16(acc.detach()).double()                                                              # first rounding point
    y = kc.rne_bf16(y1 + rba.detach()[:, :, None, None] + res[..., :Cout].double().permute(0, 3, 1, 2))  # second
    (acc + rba[:, :, None, None]).backward(dy[..., :Cout].double().permute(0, 3, 1, 2))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(kc.bits(want["y"][..., :Cout]), kc.bits(nhwc(y)))
    assert int((kc.bits(want["y"][..., Cout:]) != 0).sum()) == 0
    assert torch.equal(kc.bits(want["dx"][..., :Cin]), kc.bits(kc.rne_bf16(nhwc(xa.grad))))
    assert int((kc.bits(want["dx"][..., Cin:]) != 0).sum()) == 0
    assert torch.equal(want["dW"], wa.grad.permute(2, 3, 1, 0)) and torch.equal(want["db"], ba.grad)
    assert torch.equal(kc.bits(want["drb"][:, :Cout]), kc.bits(kc.rne_bf16(rba.grad)))


def test_linear_multi_reference_is_autograd_of_the_plain_ops():
    case = oc.LINEAR_MULTI_CASES[0]
    name, M, K, N, n, bias = case
    names, seed, x, dy = oc.multi_operands(case)
    ints = oc.IntStore(oc.multi_spec(names, K, N, bias, "grouped"), CPU, seed, quantise=False)
    want = oc.linear_multi_expect(x, [ints.w(nm) for nm in names], [ints.b(nm) for nm in names], dy)
    xa = x.double().requires_grad_(True)
    ws = [ints.w(nm).clone().requires_grad_(True) for nm in names]
    bs = [ints.b(nm).clone().requires_grad_(True) for nm in names]
    y = torch.cat([F.linear(xa, w.t(), b) for w, b in zip(ws, bs)], -1)
    y.backward(dy.double())
    assert torch.equal(kc.bits(want["y"]), kc.bits(kc.rne_bf16(y.detach()))) and torch.equal(kc.bits(want["dx"]), kc.bits(kc.rne_bf16(xa.grad)))
    for i in range(n):
        assert torch.equal(want["dW"][i], ws[i].grad) and torch.equal(want["db"][i], bs[i].grad)


def test_movement_references_are_autograd_of_the_plain_ops():
    x = kc.exact_ints((2, 5, 7, 16), -3, 3, 1).double().requires_grad_(True)
    dy = kc.exact_ints((2, 10, 14, 16), -3, 3, 2)
    x.repeat_interleave(2, 1).repeat_interleave(2, 2).backward(dy.double())
    assert torch.equal(oc.upsample_bwd_expect(dy).double(), x.grad)
    a, b = (kc.exact_ints((3, 11, c), -3, 3, s).double().requires_grad_(True) for c, s in ((24, 3), (40, 4)))
    dc = kc.exact_ints((3, 11, 64), -3, 3, 5).double()
    torch.cat([a, b], -1).backward(dc)
    assert torch.equal(a.grad, dc[..., :24]) and torch.equal(b.grad, dc[..., 24:])


def test_selector_attention_reference_is_softmax_attention():
    """float64 softmax attention and its autograd on a selector case: rounded to bf16 it is the gather selector_expect states (the
    losers' probabilities are below 1e-40), dv included; dq and dk are below any bf16 value of their scale."""
    p = oc.ATTN_OP
    B, H, D, Nq, Nk = p["B"], p["H"], p["D"], 24, 40
    scale = D ** -0.5
    case = kc.selector_case(B, H, Nq, Nk, D, False, seed=41)
    want_o, _, want_dv = kc.selector_expect(case, B, H, Nq, Nk, D, scale)
    q, k, v = (case[n].double().view(B, -1, H, D).transpose(1, 2).requires_grad_(True) for n in ("q", "k", "v"))
    o = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v
    o.backward(case["dout"].double().view(B, Nq, H, D).transpose(1, 2))
    flat = lambda t, n: t.transpose(1, 2).reshape(B, n, H * D)
    # (by value: where the selected V element is 0 the losers' 1e-140 decides the SIGN of the float64 zero; in fp32 they are exactly 0)
    assert torch.equal(flat(o.detach(), Nq).float().to(BF), want_o)
    assert torch.equal(flat(v.grad, Nk).float().to(BF), want_dv)
    assert float(q.grad.abs().max()) < 1e-30 and float(k.grad.abs().max()) < 1e-30


def test_context_selector_case_is_softmax_attention_of_the_projections():
    """The glue case: k = ctx @ Wk is exact in bf16 and float64 softmax attention over the PROJECTED keys and values, rounded, is the
    gather context_selector_expect states; its dctx and weight gradients are autograd's."""
    B, Nk, cd, C, heads, n, Nq = 2, 77, 72, 64, 2, 2, 40
    D = C // heads
    case = oc.context_selector_case(B, Nq, Nk, cd, C, heads, n, seed=23)
    wvs = [kc.exact_ints((cd, C), -3, 3, 900 + i, dtype=torch.float32).double() for i in range(n)]
    want = oc.context_selector_expect(case, wvs, heads)
    ctx = case["ctx"].double().requires_grad_(True)
    wka = [case["wk"].double().clone().requires_grad_(True) for _ in range(n)]
    wva = [w.clone().requires_grad_(True) for w in wvs]
    outs = []
    for i in range(n):
        k, v = ctx @ wka[i], ctx @ wva[i]
        assert torch.equal(k.detach().float().to(BF).double(), k.detach())  # the projected keys are exact in bf16
        assert torch.equal(kc.bits(torch.cat([kc.rne_bf16(k.detach()), kc.rne_bf16(v.detach())], -1)), kc.bits(want["kv"][i]))
        # (the kernels attend over the bf16-rounded projections; the straight-through value below keeps autograd's path to ctx)
        vr = v + (kc.rne_bf16(v.detach()).double() - v.detach())
        hd = lambda t, m: t.view(B, m, heads, D).transpose(1, 2)
        o = torch.softmax(hd(case["q"][i].double(), Nq) @ hd(k, Nk).transpose(-1, -2) * D ** -0.5, -1) @ hd(vr, Nk)
        outs.append(o.transpose(1, 2).reshape(B, Nq, C))
        assert torch.equal(outs[-1].detach().float().to(BF), want["out"][i])  # (by value: the sign of a float64 zero is the losers')
    torch.autograd.backward(outs, [d.double() for d in case["dout"]])
    r = lambda t: t.float().to(BF)
    assert torch.equal(r(ctx.grad), want["dctx"])
    for i in range(n):
        assert torch.equal(wva[i].grad.round(), want["dWv"][i]) and float((wva[i].grad - want["dWv"][i]).abs().max()) < 1e-20
        assert float(wka[i].grad.abs().max()) < 1e-20  # dk = 0: the to_k kernels' gradient is +0.0


# ================================================================================================ planted defects
def _filled_store(quantise=True):
    """A CPU store of two Dense layers and a norm (gaps behind the 4-wide bias and at the segment ends), armed and then filled with
    its expectation as a correct backward would leave it."""
    spec = [("a/kernel", (8, 24)), ("a/bias", (24,)), ("b/kernel", (16, 4)), ("b/bias", (4,)), ("n/scale", (8,)), ("n/bias", (8,))]
    ints = oc.IntStore(spec, CPU, 5, quantise=quantise)
    st = ints.st
    armed = oc.arm_gradient(st, zero=oc.host_zero_grad)
    g = torch.Generator().manual_seed(9)
    expected = {p: torch.randint(-2000, 2001, shp, generator=g).double() for p, shp in spec}
    for p, v in expected.items():
        st.g(p).copy_(v if st.g(p).dtype == torch.float32 else kc.rne_bf16(v))
    return ints, st, armed, expected


@pytest.mark.parametrize("quantise", [False, True])
def test_whole_gradient_check_accepts_a_correct_backward(quantise):
    ints, st, armed, expected = _filled_store(quantise)
    assert (st.grad16 is not None) == quantise
    assert oc.whole_gradient_report(st, expected, armed) is None
    # what zero_grad left: sentinel in the written leaves, zeros in the accumulated-into ones and in every gap
    sent16 = oc.sentinel_int(BF)
    if quantise:
        lf = st.leaves["a/kernel"]
        assert int(kc.bits(armed["grad16"])[lf.offset]) == sent16 and int(kc.bits(armed["grad16"])[st.leaves["b/kernel"].offset + 64]) == 0
    assert float(armed["grad"][st.leaves["n/scale"].offset - st.g32_base]) == 0.0


def test_one_element_one_bf16_ulp_off_is_reported_with_its_leaf_and_coordinates():
    ints, st, armed, expected = _filled_store()
    v = st.g("a/kernel")
    assert v.dtype == BF
    v.view(torch.int16)[5, 7] += 1
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "1 elements" in msg and "leaf a/kernel at (5, 7)" in msg and "grad16[" in msg


def test_the_next_leafs_first_element_touched_is_reported():
    """A bias gradient written one leaf too far, a seg_stride off by a gap: the element belongs to a leaf the case never wrote."""
    ints, st, armed, expected = _filled_store()
    del expected["b/bias"]
    st.g("b/bias").view(torch.int32).fill_(oc.sentinel_int(torch.float32))  # as zero_grad() left it
    assert oc.whole_gradient_report(st, expected, armed) is None
    st.g("b/bias")[0] = 3.0
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "leaf b/bias at (0,)" in msg and "no op of the case writes it" in msg


def test_a_word_in_an_alignment_gap_is_reported():
    ints, st, armed, expected = _filled_store()
    lf = st.leaves["b/bias"]  # 4 elements, the next leaf starts 8 further on
    st.grad[lf.offset - st.g32_base + 5] = 1.0
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "gap after leaf b/bias, element 1" in msg
    ints, st, armed, expected = _filled_store()
    lf = st.leaves["b/kernel"]  # the last quantised leaf: the gap up to the segment end
    st.grad16[lf.offset + lf.numel + 2] = -0.0
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "gap after leaf b/kernel, element 2" in msg and "0x8000" in msg  # -0.0 is not +0.0


def test_exchanged_segments_of_a_merged_gradient_are_reported():
    names = ["p0", "p1", "p2"]
    ints = oc.IntStore(oc.multi_spec(names, 64, 64, True, "grouped"), CPU, 3, quantise=True)
    st = ints.st
    armed = oc.arm_gradient(st, zero=oc.host_zero_grad)
    g = torch.Generator().manual_seed(1)
    expected = {p: torch.randint(-200, 201, lf.shape, generator=g).double() for p, lf in st.leaves.items()}
    for p, v in expected.items():
        st.g(p).copy_(v)
    assert oc.whole_gradient_report(st, expected, armed) is None
    a, b = st.g("p0/bias").clone(), st.g("p1/bias").clone()
    st.g("p0/bias").copy_(b), st.g("p1/bias").copy_(a)
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "leaf p0/bias at" in msg
    a, b = st.g("p1/kernel").clone(), st.g("p2/kernel").clone()
    st.g("p1/kernel").copy_(b), st.g("p2/kernel").copy_(a)
    msg = oc.whole_gradient_report(st, expected, armed, limit=10000)
    assert "leaf p1/kernel at" in msg and "leaf p2/kernel at" in msg and "leaf p0/kernel" not in msg


def test_a_leaf_left_at_its_sentinel_is_reported_as_never_written():
    """What a job dropped from a queue leaves behind."""
    ints, st, armed, expected = _filled_store()
    st.g("b/kernel").view(torch.int16).fill_(oc.sentinel_int(BF))
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and f"{st.leaves['b/kernel'].numel} elements" in msg and "leaf b/kernel at (0, 0)" in msg and "never written" in msg
    # an accumulated-into leaf that was never added to holds zero, not its sum
    ints, st, armed, expected = _filled_store()
    st.g("n/scale").zero_()
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "leaf n/scale at" in msg


def test_accumulated_leaves_are_expected_on_top_of_what_zero_grad_left():
    ints, st, armed, expected = _filled_store()
    armed["grad"][st.leaves["n/bias"].offset - st.g32_base] = 2.0  # pretend zero_grad() had left a 2 there
    msg = oc.whole_gradient_report(st, expected, armed)
    assert msg is not None and "leaf n/bias at (0,)" in msg
    st.g("n/bias")[0] += 2.0
    assert oc.whole_gradient_report(st, expected, armed) is None


def test_output_checkers_report_pad_columns_and_exchanged_row_bias_gradients():
    case = oc.CONV_CASES[8]  # Cout 4 -> Cp 8
    B, H, W, Cin, Cout, k, stride, pad = case
    spec, seed, x, dy, res, rb, wide = oc.conv_operands(case)
    ints = oc.IntStore(spec, CPU, seed, quantise=False)
    want = oc.conv_expect(x, ints.w("c"), ints.b("c"), rb, res, dy, stride, pad)
    assert oc.output_reports(dict(want), want, C=Cout) == []
    y = want["y"].clone()
    y[1, 3, 5, 6] = 1.0
    msgs = oc.output_reports(dict(want, y=y), want, C=Cout)
    assert len(msgs) == 2 and "(1, 3, 5, 6)" in msgs[0] and "pad columns 4..7" in msgs[1] and "(1, 3, 5, 2)" in msgs[1]
    y = want["y"].clone()
    y[0, 0, 0, 7] = -0.0  # even a negative zero in a pad column
    assert "(0, 0, 0, 3)" in oc.pad_columns_report(y, Cout, "y")
    assert not torch.equal(want["drb"][0], want["drb"][1])
    msgs = oc.output_reports(dict(want, drb=want["drb"].flip(0)), want)
    assert len(msgs) == 1 and msgs[0].startswith("drb") and "at (0, " in msgs[0] and "bounding box: (0, " in msgs[0] and ".. (1, " in msgs[0]


# ================================================================================================ the fused feed-forward kernel's shapes
def test_ff_geglu_ragged_shapes_are_what_the_planner_serves(lib):
    for F_, K in oc.FF_GEGLU_PAIRS:
        Ms = oc.ff_geglu_served(lib.sdt_ff_geglu_supported, F_, K)
        assert Ms == oc.FF_GEGLU_M[(F_, K)], (F_, K, Ms)
        assert lib.sdt_ff_geglu_supported(Ms[0] - 1, F_, K) == 0 and Ms[1] % 128 == 1 and Ms[2] % 128 == 127
        assert all(lib.sdt_ff_geglu_supported(M, F_, K) == 1 for M in Ms)
