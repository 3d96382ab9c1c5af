"""The proof that tests/test_gpu_kernel_exact.py would fail on a subtly wrong kernel, without breaking a kernel on a GPU: start from
a correct expectation, plant the defects a whole-tensor norm cannot see (one element off by one bf16 ulp, one unwritten row, one
column that lost its product term, one store outside the output) and assert that the checkers of tests/kernel_checks.py report each
at the right coordinates.  Plus the arithmetic the exact tests rest on: every exact case keeps sum |a||b| below 2^24.
For attention: selector inputs make it a gather, tied pairs give dQ and dK exact nonzero values that survive perturbed probabilities,
five planted gradient faults are reported, and the case tables reach every head dim, instantiation and planner branch they name.
The same for tests/test_gpu_reduce_optim_exact.py (second half of this file): a missing workgroup partial, a dropped tail element, = for
+=, a non-zero counter, a code off by one, a neighbour's inverse scale, an unclipped log-variance, exchanged sin / cos halves.
And for tests/test_gpu_norm_exact.py (the end of this file): the balanced cases have a unique representable result that fp32 arithmetic of
the kernels' shape lands on, the geometry mirror is the library's, and a neighbour group's mean, a dropped partial row, an early dres
and = for += are each caught."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import kernel_checks as kc

BF = torch.bfloat16


def _case():
    M, K, N = 130, 72, 136
    a = kc.exact_ints((M, K), -3, 3, 1)
    b = kc.exact_ints((K, N), -3, 3, 2)
    bias = kc.exact_ints((N,), -5, 5, 3, dtype=torch.float32)
    res = kc.exact_ints((M, N), -5, 5, 4)
    return a, b, bias, res, kc.expect_gemm_nt(a, b, bias=bias, residual=res)


def test_exact_ints_are_seeded_integers_in_range():
    a = kc.exact_ints((64, 64), -3, 3, 7)
    assert a.dtype == BF and torch.equal(a, kc.exact_ints((64, 64), -3, 3, 7))
    assert not torch.equal(a, kc.exact_ints((64, 64), -3, 3, 8))
    assert torch.equal(a.float(), a.float().round()) and a.min() == -3 and a.max() == 3


def test_integer_contraction_is_exact_in_fp32_in_any_order_and_hits_ties():
    K = 23040  # the largest reduction in the GPU file is 9 * 2560 wide
    a, b = kc.exact_ints((64, K), -3, 3, 1).float(), kc.exact_ints((K, 64), -3, 3, 2).float()
    e = a.double() @ b.double()
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(0))
    assert torch.equal((a @ b).double(), e) and torch.equal((a[:, perm] @ b[perm]).double(), e)
    o = kc.rne_bf16(e)
    ties = ((e.abs() >= 256) & (e.abs() < 512) & ((e.abs() % 4) == 2)).sum().item()  # half-way between two bf16 values
    assert ties > 50 and o.unique().numel() > 200


def test_expectation_rounds_at_the_documented_points_in_order():
    # acc + bias = 257 rounds to 256 (tie to even) BEFORE the residual is added: 256 + 1 = 257 -> 256; a single rounding of the
    # whole sum 258 would give 258
    a = torch.tensor([[1.0]]).to(BF)
    b = torch.tensor([[255.0]]).to(BF)
    got = kc.expect_gemm_nt(a, b, bias=torch.tensor([2.0]), residual=torch.tensor([[1.0]]).to(BF))
    assert got.item() == 256.0
    rb = kc.expect_gemm_nt(torch.ones(4, 1).to(BF), torch.ones(1, 1).to(BF), rowbias=torch.tensor([[1.0], [5.0]]).to(BF), rows_per_batch=2)
    assert rb.view(-1).tolist() == [2.0, 2.0, 6.0, 6.0]


def test_one_ulp_is_reported_with_its_coordinates():
    *_, want = _case()
    got = want.clone()
    kc.bits(got)  # (contiguous)
    gi = got.view(torch.int16)
    gi[77, 130] += 1
    msg = kc.mismatch_report(got, want, "y", tile=(64, 64))
    assert msg is not None and "1 of" in msg and "(77, 130)" in msg
    assert "bounding box: (77, 130) .. (77, 130)" in msg
    assert "[(1, 2)]" in msg and "rows inside a tile: [13]" in msg and "columns inside a tile: [2]" in msg
    with pytest.raises(AssertionError, match=r"\(77, 130\)"):
        kc.assert_equal_bits(got, want, "y", tile=(64, 64))
    kc.assert_equal_bits(want.clone(), want, "y")


def test_zeroed_last_row_is_reported():
    *_, want = _case()
    got = want.clone()
    got[129] = 0
    msg = kc.mismatch_report(got, want, "y", tile=(64, 64))
    nz = int((want[129] != 0).sum())
    assert msg is not None and f"{nz} of" in msg
    assert "bounding box: (129," in msg and ".. (129," in msg and "rows inside a tile: [1];" in msg
    # ... and a whole-tensor norm at the suite's tolerance does not see it
    rel = ((got.float() - want.float()).norm() / want.float().norm()).item()
    assert rel < 0.2


def test_column_without_its_product_term_is_reported():
    a, b, bias, res, want = _case()
    got = want.clone()
    got[:, 135] = kc.epilogue_nt(torch.zeros(130, 1, dtype=torch.float64), bias[135:], None, res[:, 135:])[:, 0]
    msg = kc.mismatch_report(got, want, "y", tile=(64, 64))
    assert msg is not None and "columns inside a tile: [7]" in msg
    assert "bounding box: (" in msg and ", 135) .. (" in msg and "(0, 2), (1, 2), (2, 2)" in msg


def test_sign_of_zero_and_nan_payload_are_bits():
    z = torch.zeros(8, dtype=BF)
    assert kc.mismatch_report(-z, z, "z") is not None
    n = torch.full((8,), float("nan"), dtype=BF)
    assert kc.mismatch_report(n.clone(), n, "n") is None


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int8, torch.float64])
def test_guard_element_changes_are_reported(dtype):
    g = kc.Guarded(5, 24, dtype, "cpu")
    assert g.ld == 40 and g.ptr % 16 == 0 and g.front * g.arena.element_size() >= 4096
    assert g.arena.numel() - g.front - 5 * g.ld >= 128 * g.ld
    g.t.copy_(torch.ones(5, 24).to(dtype))
    g.check("out")
    g.arena[g.front + 3 * g.ld + 24] = 1   # first pad column of row 3
    assert "pad row 3 column 24" in g.guard_report("out")
    g = kc.Guarded(5, 24, dtype, "cpu")
    g.arena[g.front - 1] = 1
    assert "front guard, 1 elements before the base" in g.guard_report("out")
    g = kc.Guarded(5, 24, dtype, "cpu")
    g.arena[g.front + 5 * g.ld + 2] = 1    # the row after the last: what a ragged tile's 16-byte store would hit
    with pytest.raises(AssertionError, match="back guard, row 5 column 2"):
        g.check("out")


def test_input_guards_hold_nan_and_surface_in_the_result():
    a = kc.exact_ints((5, 8), -3, 3, 1)
    g = kc.Guarded(5, 8, BF, "cpu", data=a)
    assert torch.equal(g.t, a) and torch.isnan(g.arena[: g.front]).all() and torch.isnan(g.arena[g.front + 8: g.front + g.ld]).all()
    wide = g.arena[g.front: g.front + 5 * g.ld].view(5, g.ld)
    assert torch.isnan(wide[:, :9].float() @ torch.ones(9, 1)).all()  # one column too many: every output is NaN
    g.check("a")
    g.arena[g.front + 1] = 9
    assert "payload row 0 column 1" in g.guard_report("a")
    f = kc.Guarded(3, 8, torch.float32, "cpu", data=torch.ones(3, 8), guard=3e38)
    assert f.arena[0] == 3e38


def test_conv_reference_is_conv2d():
    for (B, H, W, Cin, Cout, k, stride, pad) in [(2, 9, 7, 8, 16, 3, 1, 1), (2, 8, 10, 8, 8, 3, 2, ((0, 1), (0, 1))), (1, 6, 6, 8, 8, 3, 2, 1), (1, 5, 5, 8, 8, 1, 1, 0)]:
        pad = kc.norm_pad(pad)
        x = kc.exact_ints((B, H, W, Cin), -3, 3, 1).double().requires_grad_(True)
        w = kc.exact_ints((k, k, Cin, Cout), -3, 3, 2).double().requires_grad_(True)
        (pt, pb), (pl, pr) = pad
        ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=stride).permute(0, 2, 3, 1)
        y = kc.conv_ref64(x.detach(), w.detach(), stride, pad)
        assert tuple(y.shape[1:3]) == kc.conv_out_hw(H, W, k, stride, pad) and torch.equal(y, ref.detach())
        dy = kc.exact_ints(tuple(y.shape), -3, 3, 3).double()
        ref.backward(dy)
        assert torch.equal(kc.conv_dgrad_ref64(dy, w.detach(), (H, W), stride, pad), x.grad)
        assert torch.equal(kc.conv_wgrad_ref64(x.detach(), dy, (k, k), stride, pad), w.grad)


def test_every_exact_case_stays_below_2_to_24():
    rows = kc.exact_reductions()
    assert len(rows) > 60
    for what, amax, bmax, terms in rows:
        assert kc.abs_sum_bound(amax, bmax, terms) < kc.LIMIT, what
    assert max(t for *_, t in rows) >= 9 * 2560
    # epilogue terms on top of the accumulator: |acc| + bias + row bias + residual stays exact too
    assert max(kc.abs_sum_bound(a, b, t) for _, a, b, t in rows) + 3 * kc.EPI_RANGE < kc.LIMIT


def test_conv_cases_are_geometries_of_the_existing_suite():
    from tests import test_gpu_kernels as tk
    for c in kc.CONV_EXACT_CASES:
        assert c in tk.CONV_CASES, c
    for c in kc.WGRAD_CONV_CASES[:5]:
        assert c[:8] in tk.CONV_CASES, c


def test_gn_statistics_cases_stay_exact():
    """The GroupNorm statistics are fp32 sums of bf16 OUTPUTS and of their squares over (rows of a tile) x (columns of a group): with
    operands in -1..1 and Kc <= 64 the sums of |y| and of y^2 stay below 2^24 however the kernel orders them - asserted on the very
    operands the GPU test uses, with the largest row of a group times the rows of a tile (128 Dense, 256 halo) as the bound."""
    for M, N, Kc, rpb, G in kc.GN_DENSE_CASES:
        a, b, bias = kc.gn_dense_operands(M, N, Kc)
        y = kc.expect_gemm_nt(a, b, bias=bias).double().view(M, G, N // G)
        assert Kc <= 64 and M % rpb == 0
        assert (y ** 2).sum(2).max() * 128 < kc.LIMIT and y.abs().sum(2).max() * 128 < kc.LIMIT
    for B, H, W, Cin, Cout, G in kc.GN_HALO_CASES:
        x, w, bias = kc.gn_halo_operands(B, H, W, Cin, Cout)
        y = kc.rne_bf16(kc.conv_ref64(x, w, 1, kc.norm_pad(1)) + bias.double()).double().view(-1, G, Cout // G)
        assert Cin <= 64
        assert (y ** 2).sum(2).max() * 256 < kc.LIMIT and y.abs().sum(2).max() * 256 < kc.LIMIT


def test_expected_partial_rows_follow_the_header():
    y = torch.arange(4 * 24, dtype=torch.float32).view(4, 24).to(BF)  # 24 columns, 4 groups of 6, column tiles of 8
    rows = [torch.tensor([0, 1]), torch.tensor([2, 3])]
    p = kc.expect_gn_parts(y, rows, 4, 8)
    assert p.shape == (4, 4, 2)
    yd = y.double()
    assert p[0, 0, 0] == yd[:2, 0:6].sum() and p[1, 0, 0] == 0          # group 0: columns 0..5, complete in tile 0
    assert p[0, 1, 0] == yd[:2, 6:8].sum() and p[1, 1, 0] == yd[:2, 8:12].sum()   # group 1 starts in tile 0, ends in tile 1
    assert p[2, 2, 1] == (yd[2:, 12:16] ** 2).sum() and p[3, 2, 1] == (yd[2:, 16:18] ** 2).sum()
    assert p[:, :, 0].sum() == yd.sum()


def test_selector_inputs_make_attention_a_gather():
    """float64 softmax, P rounded to bf16, O rounded to bf16: exactly the gathered V rows, on every selector shape small enough for
    the CPU; the winner leads by >= 2 c^2 / sqrt(D) >= 162 logits and the largest logit is finite in fp32."""
    for (B, H, Nq, Nk, D, causal, packed, kw) in kc.ATTN_SELECTOR_CASES + kc.ATTN_HEADDIM_CASES + kc.ATTN_EDGE_CASES:
        if Nq * Nk > 300000:
            B, H = 1, 1
        if Nq * Nk > 2000000:
            continue
        scale = D ** -0.5
        case = kc.selector_case(B, H, Nq, Nk, D, causal, seed=Nq + Nk + D)
        gap, top = kc.selector_min_gap(case, B, H, Nq, Nk, D, scale)
        assert gap >= 2 * 32.0 ** 2 / D ** 0.5 - 1e-9 >= 161.9 and top < 3000
        out, lse2, dv = kc.selector_expect(case, B, H, Nq, Nk, D, scale)
        q4, k4, v4 = (case[n].view(B, -1, H, D).transpose(1, 2).double() for n in ("q", "k", "v"))
        s = (q4 @ k4.transpose(-1, -2)) * scale
        if causal:
            assert (case["target"] <= torch.arange(Nq)).all() and (case["target"][:, :, 0] == 0).all()
            s = s + torch.full((Nq, Nk), float("-inf"), dtype=torch.float64).triu(1)
        p = torch.softmax(s, -1).to(BF).double()
        assert torch.equal(p.sum(-1), torch.ones(B, H, Nq, dtype=torch.float64)) and (p.max(-1).values == 1).all()
        o = (p @ v4).float().to(BF).transpose(1, 2).reshape(B, Nq, H * D)
        assert torch.equal(o, out)
        do4 = case["dout"].view(B, Nq, H, D).transpose(1, 2).double()
        assert torch.equal(kc.rne_bf16(p.transpose(-1, -2) @ do4).transpose(1, 2).reshape(B, Nk, H * D), dv)
        dp = do4 @ v4.transpose(-1, -2)
        delta = (do4 * (p @ v4)).sum(-1, keepdim=True)
        assert ((p * (dp - delta)) == 0).all()   # dS = 0: dQ and dK are exactly zero
        lse_ref = torch.logsumexp(s, -1) * 1.4426950408889634
        assert ((lse2 - lse_ref).abs() <= 1e-6 * lse_ref.abs()).all()


def _pair(c, **kw):
    """(case, expectation, kv_chunk) of one ATTN_PAIR_CASES entry, as test_attention_tied_pairs_every_bit builds them."""
    B, H, Nq, Nk, D, packed = c
    case = kc.pair_case(B, H, Nq, Nk, D, seed=Nq + Nk + D, **kw)
    planned, chunk, launched = kc.attention_qsplit(B, H, Nq, Nk, False)
    kvc = chunk if planned > 1 else None
    return case, kc.pair_expect(case, B, H, Nq, Nk, D, D ** -0.5, kv_chunk=kvc), kvc


def _pair_shares(c, exp):
    """(nonzero share of the expected dQ, its floor, nonzero share of dK, its floor).  The floors are 1/4 and 1/3, with one
    derived exception.  dQ is nonzero on the key-extra features only (the twins' codes cancel in dS.K); they make up
    (D - nb + 1) // 2 of the D features, and within such a column dq = dS (k1 - k2) is nonzero with probability
    P(dS != 0) P(k1 != k2) = (6/7)^2 = 0.73.  At D = 16 with 100 pairs (7 code features, 5 key extras: ceiling 0.31, expected 0.23)
    and at D = 8 with 36 pairs (6 code features, ONE key extra: ceiling 0.125, expected 0.09) 1/4 is out of the construction's
    reach, so the floor is min(1/4, 2/3 of the ceiling): 1/4 for every other case."""
    D = c[4]
    nb = max(1, math.ceil(math.log2(max(-(-c[3] // 2), 2))))
    ceiling = ((D - nb + 1) // 2) / D
    return (float((exp["dq"] != 0).double().mean()), min(0.25, ceiling * 2 / 3),
            float((exp["dk"] != 0).double().mean()), 1 / 3)


@pytest.mark.parametrize("c", kc.ATTN_PAIR_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_tied_pair_cases_are_exact_nonzero_and_keep_their_bits_under_perturbed_probabilities(c):
    """Every pair case: the twins tie exactly and lead the rest by >= 2 * 32^2 / sqrt(D); dS is exact in bf16 and both accumulators
    (every query chunk's part included) in fp32 below 2^24 - pair_expect asserts it, and it is asserted again here; dQ and dK cannot
    degenerate to zeros; the rounding-point emulation lands on the expectation (by value: the sign of a zero in the float64
    emulation is the BLAS's).  Margin: the kernels' exp2 / log2 are not exact - the error of P is about the fp32 ulp of lse2, 2^-13
    relative, the bf16 half-ulp is 2^-9 - so the expectation recomputed with every probability (the forward's row sum included)
    scaled by 1 +- 2^-10 and rounded as the kernels round must keep every bit of O, dS, dQ, dK and dV."""
    B, H, Nq, Nk, D, packed = c
    scale = D ** -0.5
    case, exp, kvc = _pair(c)
    tie, lead, top = kc.pair_min_gap(case, B, H, Nq, Nk, D, scale)
    assert tie == 0.0 and lead >= 2 * 32.0 ** 2 / D ** 0.5 - 1e-9 >= 161.9 and top < 3000
    assert set(exp["p"].unique().tolist()) <= {0.0, 0.5, 1.0} and torch.equal(exp["p"].sum(-1), torch.ones(B, H, Nq, dtype=torch.float64))
    assert ((exp["p"] == 0.5).sum(-1) == 2).any() and (Nk % 2 == 0) == (not (exp["p"] == 1).any())
    assert torch.equal(exp["ds"].float().to(BF).double(), exp["ds"]) and float(exp["ds"].abs().max()) <= 3 and (exp["ds"] * 4 == (exp["ds"] * 4).round()).all()
    for n in ("acc_q", "acc_k"):
        assert torch.equal(exp[n].float().double(), exp[n]) and float(exp[n].abs().max()) < kc.LIMIT and (exp[n] * 4 == (exp[n] * 4).round()).all(), n
    sq, fq, sk, fk = _pair_shares(c, exp)
    assert sq >= fq and sk >= fk, f"dQ nonzero share {sq:.3f} (floor {fq:.3f}), dK {sk:.3f} (floor {fk:.3f})"
    assert (fq == 0.25) == (D > 16)
    ref, emu, mag = kc.attention_ref_and_emulation(case["q"], case["k"], case["v"], case["dout"], H, scale, kv_chunk=kvc)
    for n in ("o", "dq", "dk", "dv"):
        assert torch.equal(emu[n], exp[n].double()), kc.mismatch_report((emu[n] + 0.0).to(BF), exp[n], f"emulation {n}", tile=(128, D))
    for e in (2.0 ** -10, -2.0 ** -10):
        per = kc.pair_expect(case, B, H, Nq, Nk, D, scale, kv_chunk=kvc, perturb=e)
        assert torch.equal(per["ds"], exp["ds"]), f"dS moves under P (1 {e:+.1e})"
        msgs = kc.pair_reports(per, exp, D)
        assert not msgs, f"P (1 {e:+.1e}): " + "\n".join(msgs)


def test_degenerate_pair_cases_are_refused():
    """Without the extras dS.K is zero everywhere and dS^T.Q on the query-extra features: the share floors must say so."""
    for c in (kc.ATTN_PAIR_CASES[0], kc.ATTN_PAIR_CASES[12], kc.ATTN_PAIR_CASES[15]):
        case, exp, kvc = _pair(c, extras=False)
        sq, fq, sk, fk = _pair_shares(c, exp)
        assert sq == 0.0 and sq < fq, (c, sq)
        case, exp, kvc = _pair(c)
        assert _pair_shares(c, exp)[0] >= fq


def test_planted_attention_gradient_faults_are_each_reported_with_coordinates():
    """dq all zero; the dq columns of two heads exchanged; dk without the last query chunk's slab; scale applied twice; dk and dv
    exchanged: the pair checker names the tensor, the first element and the tiles of each."""
    c = kc.ATTN_PAIR_CASES[15]
    B, H, Nq, Nk, D, packed = c
    assert (B, H, Nq, Nk, D) == (1, 2, 1100, 100, 64)
    case, exp, kvc = _pair(c)
    assert kvc == 320
    good = {n: exp[n].clone() for n in ("o", "dq", "dk", "dv")}
    assert kc.pair_reports(good, exp, D) == []

    def first_diff(a, b):
        return tuple(int(v) for v in (kc.bits(a) != kc.bits(b)).nonzero()[0])

    def only(msgs, name, got):
        assert len(msgs) == 1 and msgs[0].startswith(name + " ["), msgs
        assert f"at {first_diff(got, exp[name])}:" in msgs[0] and "output tiles (128 x 64) hit" in msgs[0], msgs[0]
        return msgs[0]

    bad = dict(good, dq=torch.zeros_like(good["dq"]))
    m = only(kc.pair_reports(bad, exp, D), "dq", bad["dq"])
    assert f"{int((exp['dq'] != 0).sum())} of {exp['dq'].numel()} elements differ" in m
    bad = dict(good, dq=torch.cat([good["dq"][..., D:], good["dq"][..., :D]], -1))
    m = only(kc.pair_reports(bad, exp, D), "dq", bad["dq"])
    assert "(0, 0)" in m and "(0, 1)" in m  # both heads' column tiles
    drop = kc.pair_expect(case, B, H, Nq, Nk, D, D ** -0.5, kv_chunk=kvc, drop_rows=(Nq - 320, Nq))
    bad = dict(good, dk=drop["dk"])
    m = only(kc.pair_reports(bad, exp, D), "dk", bad["dk"])
    twice = kc.pair_expect(case, B, H, Nq, Nk, D, D ** -0.5, kv_chunk=kvc, scale_twice=True)
    bad = dict(good, dq=twice["dq"], dk=twice["dk"])
    msgs = kc.pair_reports(bad, exp, D)
    assert [m.split(" [")[0] for m in msgs] == ["dq", "dk"] and f"at {first_diff(bad['dk'], exp['dk'])}:" in msgs[1]
    assert int((kc.bits(twice["dq"]) != kc.bits(exp["dq"])).sum()) == int((exp["dq"] != 0).sum())  # every nonzero element, no other
    bad = dict(good, dk=good["dv"], dv=good["dk"])
    msgs = kc.pair_reports(bad, exp, D)
    assert [m.split(" [")[0] for m in msgs] == ["dk", "dv"] and f"at {first_diff(bad['dv'], exp['dv'])}:" in msgs[1]


def test_attention_tables_reach_every_instantiation():
    """Over the selector, head-dim, pair, edge and row tables (every case runs the forward, dQ and dK/dV): each of the six
    instantiations, in each row-sum variant of its forward, occurs causal and not in the bit-for-bit tables and not causal in the
    row tables (the pair cases, not causal, hold the values of dQ and dK for each); each meets both values of packed and of
    key_weights; the split dK/dV pass runs on pair inputs in every instantiation; every head dim 8 ... 160 occurs in the head-dim
    and in the row tables."""
    every = list(range(8, 168, 8))
    variants = {kc.attention_instance(D) for D in every}
    assert len(variants) == 10 and len({v[:3] for v in variants}) == 6
    assert {v[:3] for v in variants if v[3]} == {v[:3] for v in variants} and len({v[:3] for v in variants if not v[3]}) == 4  # <64,3,2> and <128,5,3>: ones column only
    assert [kc.attention_msum(D) for D in (48, 56, 64, 80, 88, 96, 120, 128, 152, 160)] == [True, True, False, True, True, False, True, False, True, False]
    bitwise = kc.ATTN_SELECTOR_CASES + kc.ATTN_HEADDIM_CASES + kc.ATTN_EDGE_CASES
    rows = kc.ATTN_ROW_CASES + kc.ATTN_ROW_HEADDIM_CASES
    for causal in (False, True):
        assert {kc.attention_instance(c[4]) for c in bitwise if bool(c[5]) == causal} == variants, causal
    assert {kc.attention_instance(c[4]) for c in rows if not c[5]} == variants
    assert {kc.attention_instance(c[4])[:3] for c in rows if c[5]} == {(64, 3, 2), (64, 4, 2), (128, 6, 3), (256, 10, 5)}
    assert {kc.attention_instance(c[4]) for c in kc.ATTN_PAIR_CASES} == variants
    for flag in (6, 7):
        for value in (False, True):
            assert {kc.attention_instance(c[4]) for c in kc.ATTN_HEADDIM_CASES if c[flag] == value and not c[5]} == variants, (flag, value)
    split = lambda tab: {kc.attention_instance(c[4])[:3] for c in tab if kc.attention_qsplit(c[0], c[1], c[2], c[3], len(c) > 6 and c[5] or False)[0] > 1}
    assert split(kc.ATTN_PAIR_CASES) == {v[:3] for v in variants} and (128, 5, 3) in split(bitwise) and (128, 5, 3) in split(rows)
    assert all(kc.attention_qsplit(*c[:4], False)[0] > 1 for c in kc.ATTN_PAIR_SPLIT_CASES)
    assert {c[4] for c in kc.ATTN_HEADDIM_CASES if not c[5] and c[:4] == (1, 3, 136, 200)} == set(every)
    assert {c[4] for c in rows} == set(every) and {c[4] for c in rows if not c[5]} == set(every) - {16}  # (16: causal only)
    assert {kc.attention_instance(D)[:3] for B, H, Nq, Nk, D in kc.ATTN_ROW_KEYWEIGHT_CASES} == {(128, 6, 3), (256, 10, 5)}
    assert len(set(bitwise)) == len(bitwise) and len(set(rows)) == len(rows) and len(set(kc.ATTN_PAIR_CASES)) == len(kc.ATTN_PAIR_CASES)
    # the size edges the tables name
    assert {(1, 1), (1, 77), (77, 1)} <= {(c[2], c[3]) for c in kc.ATTN_EDGE_CASES}
    assert {(D, Nk) for D in (64, 88) for Nk in (63, 64, 65, 127, 128, 129)} <= {(c[4], c[3]) for c in kc.ATTN_EDGE_CASES if c[2] == 136}
    assert {127, 128, 129} <= {c[2] for c in kc.ATTN_EDGE_CASES if c[4] == 96}
    assert kc.attention_qsplit(1, 1, 1600, 77, False) == (6, 320, 5) and kc.attention_qsplit(1, 1, 1023, 77, False)[0] == 1 and kc.attention_qsplit(1, 1, 1024, 77, False)[0] == 4


def test_per_slice_norm_sees_one_wrong_row():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(2, 4, 512, 40, generator=g)
    got = ref.to(BF).float()
    got[1, 2, 300] = 0
    whole = ((got - ref).norm() / ref.norm()).item()
    assert whole < 2e-2  # (a single figure for the tensor barely moves)
    rel = kc.per_slice_rel(got, ref, (3,))
    assert rel.shape == (2, 4, 512)
    (idx, err), (_, second) = kc.worst_slices(rel, 2)
    assert idx == (1, 2, 300) and abs(err - 1.0) < 1e-12 and second < 6e-3


def test_activation_bound_and_references():
    x = kc.all_bf16_patterns().double()
    fin = torch.isfinite(x)
    for kind in ("silu", "quick_gelu", "gelu_erf", "gelu_tanh"):
        y, d = kc.act_ref64(kind, x[fin])
        assert torch.isfinite(y).all() and torch.isfinite(d).all(), kind
        assert (d[x[fin] > 40] == 1).all() and (d[x[fin] < -800].abs() < 1e-300).all(), kind
    xs = torch.linspace(-6, 6, 1001, dtype=torch.float64).requires_grad_(True)
    for kind, fn in (("silu", F.silu), ("gelu_erf", F.gelu), ("gelu_tanh", lambda t: F.gelu(t, approximate="tanh")),
                     ("quick_gelu", lambda t: t * torch.sigmoid(1.702 * t))):
        xs.grad = None
        yr = fn(xs)
        yr.sum().backward()
        y, d = kc.act_ref64(kind, xs.detach())
        assert torch.allclose(y, yr.detach(), rtol=1e-12, atol=1e-15) and torch.allclose(d, xs.grad, rtol=1e-10, atol=1e-14), kind
    # the bound: one bf16 ulp passes, two do not; NaN never passes
    xv = torch.tensor([1.0, 1.0, 1.0, 100.0], dtype=torch.float64)
    ref = torch.tensor([1.0, 1.0, 1.0, 1e-9], dtype=torch.float64)
    got = torch.tensor([1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, float("nan"), 0.0], dtype=torch.float64)
    assert kc.act_bound_violations(got, ref, xv, torch.ones(4, dtype=torch.float64)).tolist() == [1, 2]
    assert kc.bf16_ulp(torch.tensor([1.0, 1.5, 2.0, 0.0], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]


# ------------------------------------------------------------------------------------------------ host side of the library
def test_case_tables_take_the_planner_branches_they_name(lib):
    """The workspace queries answer without a device: every case marked split asks for scratch, every other one for none."""
    import ctypes
    from stable_diffusion_training_amd import _lib
    for name, M, N, Kc, taps, bkm, nseg, has_bias, rpb, has_res, use_ws, split, edge in kc.GEMM_PLAIN_CASES:
        assert (lib.sdt_gemm_nt_workspace_bytes(M, N, Kc, taps) > 0) == split, name
        # the tile edge a failure report names is the planner's: with every row one "image", a problem of whole 128-tiles gets
        # 2 * (rows / edge) partial statistics rows (include/sdt.h), which tells the edge plan_nt chose for (M, N, Kc, taps)
        Mp, Np = -(-M // 128) * 128, -(-N // 128) * 128
        if lib.sdt_gemm_nt_workspace_bytes(Mp, Np, Kc, taps) == lib.sdt_gemm_nt_workspace_bytes(M, N, Kc, taps):
            parts = lib.sdt_gemm_nt_gn_parts(Mp, Np, Kc, taps, Mp, Np // 8 if Np // 8 <= 64 else 0, _lib.GATHER_PLAIN, None)
            assert parts == 0 or 2 * Mp // parts == edge, (name, parts, edge)
        assert N % 8 == 0 and Kc % 8 == 0 and (rpb == 0 or rpb * -(-M // rpb) >= M) and (not use_ws or split)
    for name, M, K1, N, K1v, Nv, nseg, split in kc.WGRAD_DENSE_CASES:
        assert (lib.sdt_gemm_tn_workspace_bytes(M, K1, N, 1, nseg, _lib.GATHER_PLAIN, None) > 0) == split, name
    for B, H, W, Cin, Cout, k, stride, pad, what in kc.WGRAD_CONV_CASES:
        OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
        (pt, _), (pl, _) = kc.norm_pad(pad)
        geom = _lib.SdtConvGeom(B, H, W, OH, OW, k, k, stride, pt, pl)
        need = lib.sdt_gemm_tn_workspace_bytes(B * OH * OW, Cin, Cout, k * k, 0, _lib.GATHER_FPROP, ctypes.addressof(geom))
        assert (need > 0) == what.endswith("split"), what
    for M, N, Kc, rpb, G in kc.GN_DENSE_CASES:
        assert lib.sdt_gemm_nt_gn_parts(M, N, Kc, 1, rpb, G, _lib.GATHER_PLAIN, None) > 0
    assert {2 * rpb // lib.sdt_gemm_nt_gn_parts(M, N, Kc, 1, rpb, G, _lib.GATHER_PLAIN, None) for M, N, Kc, rpb, G in kc.GN_DENSE_CASES} == {64, 128}
    for B, H, W, Cin, Cout, G in kc.GN_HALO_CASES:
        geom = _lib.SdtConvGeom(B, H, W, H, W, 3, 3, 1, 1, 1)
        assert lib.sdt_gemm_nt_gn_parts(B * H * W, Cout, Cin, 9, H * W, G, _lib.GATHER_FPROP, ctypes.addressof(geom)) > 0
    # attention: the split / no-split claims of the tables, and the Python mirror of the query-split planner (kc.attention_qsplit)
    # for every case of every attention table, against sdt_attention_bwd_workspace_bytes
    def attn_need(B, H, Nq, Nk, D, causal):
        d = _lib.SdtAttnDesc(B, H, Nq, Nk, D, H * D, H * D, H * D, H * D, D ** -0.5, int(causal), 0, 0, 0, 0, None)
        return lib.sdt_attention_bwd_workspace_bytes(ctypes.addressof(d))
    for (B, H, Nq, Nk, causal), claim in kc.ATTN_SPLIT_CLAIMS.items():
        assert (attn_need(B, H, Nq, Nk, 64, causal) > kc.attention_delta_bytes(B, H, Nq)) == claim, (B, H, Nq, Nk, causal)
    shapes = {(c[0], c[1], c[2], c[3], c[4], bool(c[5])) for c in kc.ATTN_SELECTOR_CASES + kc.ATTN_HEADDIM_CASES + kc.ATTN_EDGE_CASES
              + kc.ATTN_ROW_CASES + kc.ATTN_ROW_HEADDIM_CASES} | {c[:5] + (False,) for c in kc.ATTN_PAIR_CASES}
    for B, H, Nq, Nk, D, causal in shapes:
        planned, chunk, launched = kc.attention_qsplit(B, H, Nq, Nk, causal)
        slabs = planned * 2 * B * Nk * H * D * 4 if planned > 1 else 0
        assert attn_need(B, H, Nq, Nk, D, causal) == kc.attention_delta_bytes(B, H, Nq) + slabs, (B, H, Nq, Nk, D, causal)
        assert chunk % 64 == 0 and launched <= planned and (launched - 1) * chunk < Nq <= launched * chunk
    assert all(kc.ATTN_SPLIT_CLAIMS[c[:4] + (False,)] for c in kc.ATTN_PAIR_SPLIT_CASES)
    # the Python mirror of the halo planner (kc.halo_tile) against the library, for the forward and the input gradient of every
    # convolution case: a one-image halo tiling answers 2 * tiles_x * tiles_y partial rows; a four-image
    # tiling answers 0 (a tile straddles images) where the plain planner would not
    seen = set()
    for B, H, W, Cin, Cout, k, stride, pad in kc.CONV_EXACT_CASES:
        for ci, co in ((Cin, Cout), (Cout, Cin)):
            g = co // 8 if co // 8 <= 64 else 32   # groups of 8 channels, or 32 groups of up to 64
            if k != 3 or stride != 1 or co < 16 or co % g or co // g > 64:
                continue
            M = B * H * W
            geom = _lib.SdtConvGeom(B, H, W, H, W, 3, 3, 1, 1, 1)
            parts = lib.sdt_gemm_nt_gn_parts(M, co, ci, 9, H * W, g, _lib.GATHER_FPROP, ctypes.addressof(geom))
            plain = lib.sdt_gemm_nt_gn_parts(M, co, ci, 9, H * W, g, _lib.GATHER_PLAIN, None)
            t = kc.halo_tile(H, W, ci, M, k, stride, pad)
            seen.add(t)
            if t is None:
                assert parts == plain, (B, H, W, ci, co)
            elif t[0] == 1:
                assert parts == 2 * (H // t[1]) * (W // t[2]), (B, H, W, ci, co, parts)
            else:
                assert parts == 0, (B, H, W, ci, co, parts)
    assert {None, (1, 4, 64), (1, 8, 32), (1, 16, 16), (4, 8, 8)} <= seen


def test_documented_violations_are_refused_and_write_nothing(lib):
    """sdt_gemm_nt_bf16, sdt_gemm_tn_wgrad, sdt_attention_fwd / _bwd with each documented violation: a negative code, a message, and
    not one byte written.  Every one of these checks runs before the first device call, so host buffers stand in for device memory
    (guarded: a write anywhere in them would show)."""
    import ctypes
    from stable_diffusion_training_amd import _lib
    mk = lambda dt=BF: kc.Guarded(64, 64, dt, "cpu")
    A, B_, C, R, W32, WS = mk(), mk(), mk(), mk(), mk(torch.float32), mk(torch.float32)
    g3 = _lib.SdtConvGeom(1, 8, 8, 8, 8, 3, 3, 1, 1, 1)
    gp = ctypes.addressof(g3)

    def nt(A=A.ptr, Bt=B_.ptr, Cp=C.ptr, M=64, N=64, Kc=8, taps=1, lda=80, ldb=80, ldc=80, res=None, ldres=0, mode=0, geom=None):
        return lib.sdt_gemm_nt_bf16(A, Bt, Cp, None, None, res, M, N, Kc, taps, lda, ldb, 0, ldc, ldres, 0, mode, geom, None, 0, None, 0, 0, 0, 0, 0, None)

    def tn(A=A.ptr, dY=B_.ptr, dW=W32.ptr, M=64, K1=64, N=64, K1v=64, Nv=64, taps=1, lda=80, ldb=80, ldw=80, mode=0, geom=None, ws=None):
        return lib.sdt_gemm_tn_wgrad(A, dY, dW, 0, None, M, K1, N, K1v, Nv, taps, lda, ldb, ldw, 64 * 80, 0, 0, mode, geom, ws, 0, None, None)

    def desc(D=64, ld=80, Nq=8):
        return _lib.SdtAttnDesc(1, 1, Nq, 8, D, ld, ld, ld, ld, 0.125, 0, 0, 0, 0, 0, None)

    d_ok, d168, d_ld = desc(), desc(D=168, ld=176), desc(ld=68)
    cases = [
        ("gemm_nt misaligned A", lambda: nt(A=A.ptr + 2), b"16-byte aligned"),
        ("gemm_nt misaligned C", lambda: nt(Cp=C.ptr + 8), b"16-byte aligned"),
        ("gemm_nt N % 8", lambda: nt(N=60), b"multiples of 8"),
        ("gemm_nt ldc % 8", lambda: nt(ldc=68), b"multiples of 8"),
        ("gemm_nt lda < taps * Kc", lambda: nt(Kc=32, taps=3, lda=80), b"lda >= taps*Kc"),
        ("gemm_nt ldres < N", lambda: nt(res=R.ptr, ldres=56), b"ldres"),
        ("gemm_nt taps != kh * kw", lambda: nt(taps=4, mode=_lib.GATHER_FPROP, geom=gp), b"kh*kw"),
        ("gemm_nt M against the geometry", lambda: nt(M=60, taps=9, mode=_lib.GATHER_FPROP, geom=gp), b"conv geometry"),
        ("gemm_tn misaligned dY", lambda: tn(dY=B_.ptr + 2), b"16-byte aligned"),
        ("gemm_tn N % 8", lambda: tn(N=60, Nv=60), b"multiples of 8"),
        ("gemm_tn K1_valid > K1", lambda: tn(K1v=72), b"valid dims"),
        ("gemm_tn ldw < N_valid", lambda: tn(ldw=56), b"valid dims"),
        ("gemm_tn plain taps", lambda: tn(taps=3), b"taps == 1"),
        ("gemm_tn taps != kh * kw", lambda: tn(taps=4, mode=_lib.GATHER_FPROP, geom=gp), b"kh*kw"),
        ("attention_fwd D = 168", lambda: lib.sdt_attention_fwd(A.ptr, B_.ptr, R.ptr, C.ptr, W32.ptr, ctypes.addressof(d168), None), b"head dim 168"),
        ("attention_fwd row stride % 8", lambda: lib.sdt_attention_fwd(A.ptr, B_.ptr, R.ptr, C.ptr, W32.ptr, ctypes.addressof(d_ld), None), b"row strides"),
        ("attention_fwd misaligned out", lambda: lib.sdt_attention_fwd(A.ptr, B_.ptr, R.ptr, C.ptr + 2, W32.ptr, ctypes.addressof(d_ok), None), b"16-byte aligned"),
        ("attention_bwd D = 168", lambda: lib.sdt_attention_bwd(A.ptr, B_.ptr, R.ptr, A.ptr, A.ptr, W32.ptr, C.ptr, C.ptr, C.ptr, WS.ptr, 1 << 20, ctypes.addressof(d168), None), b"head dim 168"),
        ("attention_bwd workspace too small", lambda: lib.sdt_attention_bwd(A.ptr, B_.ptr, R.ptr, A.ptr, A.ptr, W32.ptr, C.ptr, C.ptr, C.ptr, WS.ptr, 4 * 8 - 1, ctypes.addressof(d_ok), None), b"workspace too small"),
    ]
    for what, fn, msg in cases:
        rc = fn()
        assert rc < 0, f"{what}: accepted (returned {rc})"
        assert msg in lib.sdt_last_error(), f"{what}: message {lib.sdt_last_error()!r}"
    for name, g in (("A", A), ("B", B_), ("C", C), ("residual", R), ("dW / lse", W32), ("workspace", WS)):
        g.check(name)
        assert g.guard_report(name) is None
        ref = kc.Guarded(64, 64, g.dtype, "cpu")
        assert torch.equal(kc.bits(g.arena), kc.bits(ref.arena)), f"{name}: a refused call wrote into the payload"


# ------------------------------------------------------------------------------------------------ emulations of the rounding points
def test_attention_emulation_reference_and_floor():
    """The float64 half of attention_ref_and_emulation is autograd's attention; the emulation lands at bf16 distance from it; the
    denominator floor gives query 0 of a causal problem (reference gradient exactly zero) a finite figure."""
    g = torch.Generator().manual_seed(0)
    B, H, N, D = 1, 2, 96, 16
    q, k, v, do = (torch.randn(B, N, H * D, generator=g).to(BF) for _ in range(4))
    ref, emu, mag = kc.attention_ref_and_emulation(q, k, v, do, H, D ** -0.5, causal=True)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, N, H, D).transpose(1, 2) for t in (qr, kr, vr))
    s = (qh @ kh.transpose(-1, -2)) * D ** -0.5 + torch.full((N, N), float("-inf"), dtype=torch.float64).triu(1)
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, N, H * D)
    o.backward(do.double())
    for n, t in (("o", o.detach()), ("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad)):
        assert (ref[n] - t).abs().max() < 1e-12, n
        rows = lambda x: x.view(B, N, H, D)
        rel = kc.per_slice_rel(rows(emu[n]), rows(ref[n]), (3,), rows(mag[n]))
        assert torch.isfinite(rel).all() and 5e-4 < rel.max() < 5e-2, (n, rel.max())
    assert ref["dq"][:, 0].abs().max() < 1e-15 and (mag["dq"][:, 0] != 0).any()
    assert torch.equal(emu["o"][:, 0], v[:, 0].double())  # one key: P = 1, l = 1
    assert kc.attention_msum(40) and kc.attention_msum(80) and not kc.attention_msum(64) and not kc.attention_msum(128) and not kc.attention_msum(160)


def test_norm_emulation_reference():
    g = torch.Generator().manual_seed(1)
    for G, shape, silu in ((32, (2, 64, 320), True), (32, (2, 16, 64), False), (0, (33, 48), False)):
        C = shape[-1]
        x, dy = (torch.randn(shape, generator=g) * 2 + 0.5).to(BF), torch.randn(shape, generator=g).to(BF)
        ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
        ref, emu, terms = kc.norm_ref_and_emulation(x, ga, be, dy, G, 1e-5, silu)
        xr, gr, br = x.double().requires_grad_(True), ga.double().requires_grad_(True), be.double().requires_grad_(True)
        y = F.group_norm(xr.transpose(1, 2), 32, gr, br, 1e-5).transpose(1, 2) if G else F.layer_norm(xr, (C,), gr, br, 1e-5)
        y = F.silu(y) if silu else y
        y.backward(dy.double())
        for n, t in (("y", y.detach()), ("dx", xr.grad), ("dgamma", gr.grad), ("dbeta", br.grad)):
            assert (ref[n] - t).abs().max() < 1e-11, n
        assert ((emu["dgamma"] - ref["dgamma"]).abs() / terms["dgamma"]).max() < 1e-6
        assert kc.per_slice_rel(emu["y"], ref["y"], (len(shape) - 1,)).max() < 4e-3


# ================================================================================================ reductions, optimizer sweeps, loss kernels
# (the checkers of tests/test_gpu_reduce_optim_exact.py: each fault it exists for, planted into a correct result)
def _sq_case(n=8192 * 5 + 3):
    x = kc.exact_ints((n,), -kc.SQNORM_RANGE, kc.SQNORM_RANGE, 3, dtype=torch.float32)
    sq = x.double() ** 2
    return n, sq, kc.sqnorm_parts(sq, n), sq[(n >> 2) << 2:]


def test_sum_report_names_a_missing_workgroup_partial():
    n, sq, parts, tail = _sq_case()
    init = 12345.0
    want = init + float(sq.sum())
    assert parts.numel() == 5 and float(parts.sum()) == float(sq.sum())
    assert kc.sum_report(want, want, "out", init, parts, tail) is None
    parts[3] += 0.5  # (make the partial unique so that the report can only name this one)
    msg = kc.sum_report(want - float(parts[3]) + 0.5, want + 0.5, "out", init, parts, tail)
    assert msg is not None and "partial of workgroup [3] of 5" in msg
    # one workgroup of 2048 is far below what a 1e-6 relative check of the norm sees
    assert float(parts[3]) / want < 0.25 and (1 / 2048) ** 0.5 > 1e-6


def test_sum_report_names_a_dropped_tail_element():
    n, sq, parts, tail = _sq_case()
    assert tail.numel() == 3
    sq[-1] = 9.0
    tail = sq[(n >> 2) << 2:]
    want = float(sq.sum())
    msg = kc.sum_report(want - 9.0, want, "out", 0.0, None, tail)
    assert msg is not None and "last 1 of the 3 tail elements" in msg
    msg = kc.sum_report(want - float(tail.sum()), want, "out", 0.0, None, tail)
    assert "last 3 of the 3 tail elements" in msg
    assert 9.0 / want < 1e-4  # invisible to a relative tolerance on the norm


def test_sum_report_names_a_store_where_an_accumulation_belongs():
    n, sq, parts, tail = _sq_case()
    s = float(sq.sum())
    msg = kc.sum_report(s, 12345.0 + s, "out", 12345.0, parts, tail)
    assert msg is not None and "= where += belongs" in msg
    db0, colsum = kc.exact_ints((264,), -5, 5, 1, dtype=torch.float32), kc.exact_ints((264,), -100, 100, 2, dtype=torch.float32)
    rep = kc.mismatch_report(colsum, db0 + colsum, "db")
    assert rep is not None and f"{int((db0 != 0).sum())} of 264" in rep


def test_nonzero_counter_is_reported():
    ws = torch.zeros(kc.CNT_BYTES + 4096, dtype=torch.uint8)
    ws[kc.CNT_BYTES:] = 0xFF  # the slabs may hold anything
    assert kc.counters_report(ws) is None
    ws[4 * 17] = 1
    assert "counter 17 = 1" in kc.counters_report(ws)


def _lion_state(bs=16, nblk=40):
    rs = np.random.RandomState(0)
    return kc.LION_ORACLE.block_quantize((rs.standard_normal(nblk * bs) * 10.0 ** rs.uniform(-3, 0, nblk).repeat(bs)).astype(np.float32), bs)


def test_one_code_off_by_one_and_a_neighbours_scale_are_reported():
    codes, inv = _lion_state()
    assert kc.lion_state_report(codes.copy(), inv.copy(), codes, inv, "s") is None
    c = codes.copy()
    c[7, 5] += 1
    assert "1 codes differ, first: block 7 element 5" in kc.lion_state_report(c, inv, codes, inv, "s")
    i = inv.copy()
    i[12] = inv[11]  # what a store by the wrong lane, or a skipped store after the neighbour's, leaves behind
    msg = kc.lion_state_report(codes, i, codes, inv, "s")
    assert "1 inverse scales differ, first: block 12" in msg and "(the oracle's scale of block 11)" in msg
    i = inv.copy()
    i[3] = np.nextafter(i[3], np.float32(0))  # one ulp: what a reciprocal instead of a division would do
    assert "block 3" in kc.lion_state_report(codes, i, codes, inv, "s")


def test_optimizer_references_are_the_oracles_own_functions():
    from oracle import lion8
    assert kc.LION_ORACLE is lion8
    bs, n = 16, 256
    rs = np.random.RandomState(1)
    p, g = rs.standard_normal(n).astype(np.float32), (3 * rs.standard_normal(n)).astype(np.float32)
    codes, inv = lion8.block_quantize(np.zeros(n, np.float32), bs)
    got = kc.lion8_reference_step(p, g, codes, inv, p.copy(), bs, 1.0, 0.07)
    newp, st, gn = lion8.lion_step({"x": p}, {"x": g}, {"count": 0, "mu": {"x": (codes, inv)}}, lr=kc.LION_HP["lr"], wd=0.07, b1=0.9, b2=0.99, block_size=bs, clip=1.0)
    assert np.array_equal(got[0], newp["x"]) and np.array_equal(got[1], st["mu"]["x"][0]) and np.array_equal(got[2], st["mu"]["x"][1])
    assert np.array_equal(got[3], lion8.ema_update({"x": p}, newp, kc.LION_HP["ema_rate"])["x"])
    assert np.float32(np.sqrt(got[5])) == gn and torch.equal(got[4], torch.from_numpy(newp["x"]).to(BF))
    m32 = kc.lion32_reference_step(p, g, np.zeros(n, np.float32), None, None, 0.0)
    newp, st, _ = lion8.lion_step({"x": p}, {"x": g}, {"count": 0, "mu": {"x": np.zeros(n, np.float32)}}, lr=kc.LION_HP["lr"], wd=0.0, b1=0.9, b2=0.99, clip=None)
    assert np.array_equal(m32[0], newp["x"]) and np.array_equal(m32[1], st["mu"]["x"]) and m32[2] is None


def test_gradients_with_a_norm_exactly_at_the_threshold():
    from oracle import lion8
    for n in (1, 3, 4, 256, 4096 - 4, 4096 + 256, (1 << 20) + 5):
        g, mx = kc.grads_with_exact_norm(n, n)
        assert g.dtype == np.float32 and g.shape == (n,) and float(np.sum(g.astype(np.float64) ** 2)) == mx * mx
        assert np.array_equal(torch.from_numpy(g).to(BF).float().numpy(), g) and float(np.float32(mx)) == mx
        clipped, norm = lion8.clip_by_global_norm({"x": g}, mx)
        assert float(norm) == mx  # not below: optax's else branch
        if n >= 256:  # ... whose result differs from the untouched gradient: taking the wrong branch shows
            assert (clipped["x"] != g).sum() >= n // 32
    assert not (np.float32(1.0) < np.float32(1.0))


def _posterior_inputs():
    pat = torch.arange(65536, dtype=torch.int32)
    lv_bits, eps_idx = pat.repeat_interleave(len(kc.POST_EPS)), torch.arange(len(kc.POST_EPS)).repeat(65536)
    lv = lv_bits.to(torch.int16).view(BF)
    return lv_bits, eps_idx, lv, torch.zeros_like(lv), torch.tensor(kc.POST_EPS)[eps_idx]


def test_unclipped_logvar_and_a_number_for_nan_are_reported():
    lv_bits, eps_idx, lv, mean, eps = _posterior_inputs()
    good = kc.posterior_emulation(mean, lv, eps).float()
    assert kc.posterior_clip_report(good, lv_bits, eps_idx) is None
    sc = float(torch.tensor(kc.POST_SCALE, dtype=torch.float32))
    for lo, what in ((-40.0, "<= -30"), (-30.0, None)):  # a clip at -40 instead of -30; the right bound
        bad = ((mean.double() + torch.exp(0.5 * lv.double().clamp(lo, 20.0)) * eps.double()) * sc).float()
        msg = kc.posterior_clip_report(bad, lv_bits, eps_idx)
        assert (msg is None) == (what is None)
        if what:
            assert what in msg and "0xc1f1" in msg and "eps 1.0" in msg  # the first pattern below -30, the first eps that shows it
    # fminf(fmaxf(NaN, -30), 20) = -30: a finite latent for a NaN log-variance
    nan_as_lo = torch.where(torch.isnan(lv.double()), torch.full_like(lv, -30.0), lv)
    msg = kc.posterior_clip_report(kc.posterior_emulation(mean, nan_as_lo, eps).float(), lv_bits, eps_idx)
    assert "NaN logvar pattern 0x7f81 gave the number" in msg
    # the float64 reference keeps NaN, as jnp.clip and oracle.nets.vae_sample_latents do
    from oracle import nets as onets
    m = torch.tensor([[[[0.5, float("nan")]]]])
    assert torch.isnan(onets.vae_sample_latents(m, torch.ones(1, 1, 1, 1))).all()
    assert torch.isnan(kc.posterior_ref64(mean[:1], torch.tensor([float("nan")]), eps[:1])).all()
    # the emulation is the float64 reference up to fp32 roundings
    fin = ~torch.isnan(lv.double())
    rel = (good[fin].double() - kc.posterior_ref64(mean[fin], lv[fin], eps[fin])).abs() / kc.posterior_term_magnitude(mean[fin], lv[fin], eps[fin]).clamp_min(1e-300)
    assert 1e-8 < rel.max() < 2e-6


def test_exchanged_sin_and_cos_halves_are_reported():
    from oracle import nets as onets
    t = torch.tensor([0, 1, 64, 999, 1024, 4096], dtype=torch.int32)
    for dim, flip, shift in ((320, True, 0.0), (256, True, 0.0), (100, False, 1.0)):
        e = onets.timestep_embedding(t, dim, flip, shift).to(BF)
        assert kc.timestep_report(e, t, dim, int(flip), shift) is None
        half = dim // 2
        msg = kc.timestep_report(torch.cat([e[:, half:], e[:, :half]], -1), t, dim, int(flip), shift)
        assert msg is not None and "halves are exchanged" in msg and "first at (row, column) [(0, 0)" in msg
        one = e.clone()
        one.view(torch.int16)[3, 7] += 2  # two bf16 ulps on one element
        msg = kc.timestep_report(one, t, dim, int(flip), shift)
        assert "1 of" in msg and "(3, 7)" in msg and "exchanged" not in msg
    ref = torch.cos(t.double()[:, None] * torch.exp(torch.arange(160, dtype=torch.float64) * -math.log(10000.0) / 160))
    assert (kc.timestep_ref64(t, 320, True, 0.0)[:, :160] - ref).abs().max() < 1e-11


def test_guards_around_in_place_operands_are_reported():
    for dtype in (torch.float64, torch.float32, torch.int8):
        g = kc.Guarded(1, 5, dtype, "cpu", pad=0, back_rows=0)
        g.t.copy_(torch.ones(1, 5).to(dtype))
        g.check("in place")
        g.t.mul_(2)  # the payload may change
        g.check("in place")
        g.arena[g.front + 5] = 1  # the element a tail store one too wide would hit
        assert "back guard, row 1 column 0" in g.guard_report("in place")
        g = kc.Guarded(1, 1, dtype, "cpu", pad=0, back_rows=0)
        g.arena[g.front - 1] = 1  # the word in front of *out_sq
        assert "front guard, 1 elements before the base" in g.guard_report("out_sq")


def test_reduction_case_tables_are_exact_and_take_every_path(lib):
    rows = kc.exact_case_bounds()
    assert len(rows) > 45
    for what, bound, limit in rows:
        assert bound < limit, what
    # squared norms: only a tail, one workgroup, many, the capped grid with a second stride pass
    grids = [kc.sqnorm_partition(n) for n in kc.SQNORM_SIZES]
    assert [g for g, _ in grids[:9]] == [1] * 9 and grids[9][0] == 128 and grids[10][0] == 2048 and grids[10][1] > 2048 * 2048
    assert {n & 3 for n in kc.SQNORM_SIZES} == {0, 1, 2, 3} and lib.sdt_sqnorm_workspace_bytes() == kc.CNT_BYTES + 2048 * 8
    parts = kc.sqnorm_parts(torch.ones(8192 * 3 + 2, dtype=torch.float64), 8192 * 3 + 2)
    assert parts.tolist() == [8194.0, 8192.0, 8192.0]
    g, per = kc.sum_f64_partition(kc.SUMF64_SIZES[-1])
    assert g == 2048 and per > 4096 and [kc.sum_f64_partition(n)[0] for n in kc.SUMF64_SIZES[:9]] == [1] * 8 + [2]
    # MSE: one workgroup, exactly the cap of 512, beyond it; the exact cases have power-of-two counts
    wgs = {name: -(-B * H * W // 256) for name, B, C, H, W, *_ in kc.MSE_CASES}
    assert wgs["one_wg"] == 1 and wgs["cap_512_wg"] == 512 and wgs["stride_2_passes"] == 1024 and wgs["c3_unpadded"] == 2
    assert {(C, cpad) for _, B, C, H, W, cpad, *_ in kc.MSE_CASES} >= {(4, 4), (4, 8), (4, 16), (3, 3), (3, 8), (9, 9), (9, 16)}
    assert lib.sdt_reduce_workspace_bytes() >= kc.CNT_BYTES + 512 * 4
    for name, B, C, H, W, cpad, wt, dp, l0 in kc.MSE_CASES:
        cnt = B * C * H * W
        assert (l0 != 0) == (cnt & (cnt - 1) == 0), name
    # column sums: the planner's branches, by its own formulas
    seen = set()
    for N, ld, rows_, batch, r in kc.COLSUM_CASES:
        assert ld >= N and ld % 8 == 0 and rows_ * r < kc.LIMIT
        for b, want_blocks in ((1, 256), (batch, 512)):
            ncb, nby, rpb, want = kc.colsum_plan(b, rows_, N, want_blocks)
            assert nby * rpb >= rows_ > (nby - 1) * rpb and nby <= (rows_ + 63) // 64
            assert lib.sdt_colsum_workspace_bytes(b, rows_, N) >= kc.CNT_BYTES + ncb * b * nby * 256 * 4
            seen |= {"one row block"} if nby == 1 else set()
            seen |= {"nby == want"} if nby == want and nby > 1 else set()
            seen |= {"ragged last row block"} if rows_ % rpb else set()
            seen |= {"N % 8"} if N % 8 else set()
            seen |= {"ld > N"} if ld > N else set()
    assert seen == {"one row block", "nby == want", "ragged last row block", "N % 8", "ld > N"}
    assert {c[0] for c in kc.COLSUM_CASES} >= {8, 248, 256, 264, 1280, 2560} and {c[2] for c in kc.COLSUM_CASES} >= {1, 7, 63, 64, 65, 4096, 65537, 1 << 20}
    assert {c[3] for c in kc.COLSUM_CASES} == {1, 2, 5}
    dy = kc.exact_ints((5 * 64, 256), -200, 200, 256 + 64 + 5).double().view(5, 64, 256).sum(1)
    assert int(((dy.abs() >= 256) & (dy.abs() < 512) & (dy.abs() % 4 == 2)).sum()) > 3  # results on bf16 ties
    # embeddings
    for D, nseq, pat, vocab in kc.EMB_CASES:
        ids = kc.embedding_ids(pat, nseq, vocab, D + nseq)
        assert ids.numel() == nseq * kc.EMB_S and ids.min() >= 0 and ids.max() == (0 if pat == "equal_first" else vocab - 1) and ids.unique().numel() < vocab
        if pat == "distinct":
            assert ids.unique().numel() == ids.numel() and ids.min() == 0
        if pat == "clip":
            assert (ids.view(nseq, -1)[:, -60:] == vocab - 1).all() and ids.unique().numel() > 3
    assert {c[0] for c in kc.EMB_CASES} == {48, 768, 1280} and {c[1] for c in kc.EMB_CASES} >= {1, 12}
    # optimizer sizes: the end of the buffer inside a wave, on and just past a slice of 1024 float4s
    for bs in kc.LION_BLOCK_SIZES:
        s = kc.lion8_sizes(bs)
        assert all(n % bs == 0 for n in s) and s[0] == bs and s[2] == 4096 and s[1] < 4096 < s[3] and s[4] > 1 << 20
    assert kc.LION_BLOCK_SIZES == [4 << i for i in range(7)] and kc.LION32_SIZES == [1, 3, 1023, 1024, 1025, (1 << 20) + 5]
    # parameter preparation: which leaves take the vectorised interior path
    vec = {name: R >= 64 and C >= 64 and not (R | C | Rp | Cp) & 3 and rem == 0 for name, b, R, C, Rp, Cp, rem in kc.PREP_LEAVES}
    assert vec == {"interior": True, "padded": False, "conv": False, "small": False, "odd_offset": False, "interior_after_odd": True}


def test_documented_refusals_of_the_reduction_and_optimizer_entry_points(lib):
    """cpad < C, moment_stride < 2L, n % block_size, a misaligned acc, a workspace that is too small: -1, a message, nothing written
    (every check runs before the first device call, so guarded host buffers stand in)."""
    mk = lambda dt: kc.Guarded(8, 64, dt, "cpu")
    A, B_, O, I8, D64, WS = mk(torch.float32), mk(BF), mk(torch.float32), mk(torch.int8), mk(torch.float64), mk(torch.float32)
    big = 1 << 20
    cases = [
        ("add_noise cpad < C", lambda: lib.sdt_add_noise_velocity(A.ptr, A.ptr, A.ptr, A.ptr, B_.ptr, None, None, 1, 4, 2, 2, 3, None), b"bad shape"),
        ("ddim cpad < C", lambda: lib.sdt_ddim_cfg_step(B_.ptr, O.ptr, B_.ptr, 1, 4, 2, 2, 3, 7.5, 0.5, 0.6, 0, None), b"bad shape"),
        ("mse cpad < C", lambda: lib.sdt_mse_loss_fwd_bwd(B_.ptr, A.ptr, None, O.ptr, None, 1, 4, 2, 2, 3, WS.ptr, big, None), b"bad args"),
        ("mse workspace too small", lambda: lib.sdt_mse_loss_fwd_bwd(B_.ptr, A.ptr, None, O.ptr, None, 1, 4, 2, 2, 4, WS.ptr, lib.sdt_reduce_workspace_bytes() - 1, None), b"workspace"),
        ("posterior moment_stride < 2L", lambda: lib.sdt_vae_posterior_sample(B_.ptr, A.ptr, O.ptr, 1, 4, 2, 2, 7, 0.18215, None), b"bad args"),
        ("sqnorm workspace too small", lambda: lib.sdt_sqnorm_accumulate(A.ptr, 64, D64.ptr, WS.ptr, lib.sdt_sqnorm_workspace_bytes() - 1, None), b"workspace"),
        ("sqnorm misaligned g", lambda: lib.sdt_sqnorm_accumulate(A.ptr + 4, 64, D64.ptr, WS.ptr, big, None), b"16-byte aligned"),
        ("sqnorm_bf16 misaligned g", lambda: lib.sdt_sqnorm_accumulate_bf16(B_.ptr + 4, 64, D64.ptr, WS.ptr, big, None), b"8-byte aligned"),
        ("sum_f64 without workspace", lambda: lib.sdt_sum_f64_accumulate(D64.ptr, 8, D64.ptr, None, 0, None), b"workspace"),
        ("grad_accumulate misaligned acc", lambda: lib.sdt_grad_accumulate(O.ptr + 4, A.ptr, 0, 64, 1, 1.0, None, None, 0, None), b"acc must be 16-byte aligned"),
        ("grad_accumulate out_sq without workspace", lambda: lib.sdt_grad_accumulate(O.ptr, A.ptr, 0, 64, 1, 1.0, D64.ptr, None, 0, None), b"workspace"),
        ("grad_accumulate unknown mode", lambda: lib.sdt_grad_accumulate(O.ptr, A.ptr, 0, 64, 4, 1.0, None, None, 0, None), b"unknown mode"),
        ("lion8 n % block_size", lambda: lib.sdt_lion8_step(O.ptr, A.ptr, 0, I8.ptr, O.ptr, None, None, 40, 16, None, A.ptr, 1.0, 1e-3, 0.0, 0.9, 0.99, 0.999, None), b"not a multiple of block_size"),
        ("lion8 block_size 512", lambda: lib.sdt_lion8_step(O.ptr, A.ptr, 0, I8.ptr, O.ptr, None, None, 512, 512, None, A.ptr, 1.0, 1e-3, 0.0, 0.9, 0.99, 0.999, None), b"power of two"),
        ("lion8 misaligned p", lambda: lib.sdt_lion8_step(O.ptr + 4, A.ptr, 0, I8.ptr, O.ptr, None, None, 64, 16, None, A.ptr, 1.0, 1e-3, 0.0, 0.9, 0.99, 0.999, None), b"misaligned"),
        ("lion8_quantize n % block_size", lambda: lib.sdt_lion8_quantize(A.ptr, I8.ptr, O.ptr, 40, 16, A.ptr, None), b"bad args"),
        ("colsum ld % 8", lambda: lib.sdt_colsum_accumulate(B_.ptr, O.ptr, 8, 60, 60, WS.ptr, big, None), b"multiple of 8"),
        ("colsum workspace too small", lambda: lib.sdt_colsum_accumulate(B_.ptr, O.ptr, 8, 64, 80, WS.ptr, kc.CNT_BYTES, None), b"workspace"),
    ]
    for what, fn, msg in cases:
        rc = fn()
        assert rc == -1, f"{what}: returned {rc}"
        assert msg in lib.sdt_last_error(), f"{what}: message {lib.sdt_last_error()!r}"
    for g in (A, B_, O, I8, D64, WS):
        ref = kc.Guarded(8, 64, g.dtype, "cpu")
        assert torch.equal(kc.bits(g.arena), kc.bits(ref.arena)), "a refused call wrote into a buffer"


# ================================================================================================ norms on balanced inputs
# (the checkers, generators and case tables of tests/test_gpu_norm_exact.py)
def _ulps(t, k):
    """fp32 tensor moved by k units in the last place."""
    return (t.contiguous().view(torch.int32) + k).view(torch.float32)


def _norm_model(case, G, eps, rstd_ulps=0, fault=None, stats=None):
    """A torch fp32 restatement of the norm kernels' formulas (norm.hip), NOT used by the GPU tests: it shows that the float64
    expectation is what fp32 arithmetic of this shape lands on.  GroupNorm (G > 0; gn_apply_kernel, gn_bwd_stats_kernel,
    gn_bwd_apply_kernel): mean = tot * fl(1 / cnt), var = tot2 * fl(1 / cnt) - mean^2, rstd = fl((var + eps)^-1/2) moved by rstd_ulps
    (rsqrtf is an approximation), a = rstd * gamma, sh = beta - mean * a, y = bf16(a x + sh); xhat = (x - mean) * rstd, {S1, S2} =
    sums of gamma dy {1, xhat}, k = rstd * S * fl(1 / cnt), dx = bf16(rstd gamma dy - k1 - xhat k2), with dres bf16(bf16(dx) + dres).
    LayerNorm (G = 0; ln_fwd_kernel, ln_bwd_kernel): mean = s / C, y = bf16((x - mean) * rstd * gamma + beta), dx = bf16(rstd * (g - s1 -
    xhat * s2)).  dgamma / dbeta = previous value + fp32 sums.  fault: 'neighbour_mean' (group g normalises with the mean of group
    g + 1), 'previous_image' (image b normalises, forward and backward, with the statistics of image b - 1; the stats output stays right),
    'dres_early' (dres added before the first rounding), 'store' (= where += belongs)."""
    f = torch.float32
    x, dy, gamma, beta = case["x"].to(f), case["dy"].to(f), case["gamma"], case["beta"]
    cnt = case["cnt"]
    if G:
        B, HW, C = x.shape
        cpg = C // G
        xg = x.view(B, HW, G, cpg)
        tot = torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1) if stats is None else stats
        inv = torch.tensor(1.0, dtype=f) / torch.tensor(float(cnt), dtype=f)
        used = tot.roll(1, 0) if fault == "previous_image" else tot
        mean = used[..., 0] * inv
        var = (used[..., 1] * inv - mean * mean).clamp_min(0)
        ex = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]  # (B, G) -> (B, 1, C)
        red = lambda t: t.view(B, HW, G, cpg).sum((1, 3))
    else:
        mean = x.sum(1) / cnt
        var = ((x * x).sum(1) / cnt - mean * mean).clamp_min(0)
        ex = lambda t: t[:, None]
        red = lambda t: t.sum(1)
        inv = None
    rstd = _ulps((var.double() + eps).rsqrt().to(f), rstd_ulps)
    if fault == "neighbour_mean":
        mean = mean.roll(-1, -1)
    m, r = ex(mean), ex(rstd)
    if G:
        a = r * gamma
        y = a * x + (beta - m * a)
    else:
        y = (x - m) * r * gamma + beta
    xh = (x - m) * r
    gd = dy * gamma
    if G:
        k1, k2 = ex(rstd * red(gd) * inv), ex(rstd * red(gd * xh) * inv)
        dx = r * gamma * dy - k1 - xh * k2
    else:
        dx = r * (gd - ex(red(gd) / cnt) - xh * ex(red(gd * xh) / cnt))
    lead = tuple(range(x.dim() - 1))
    zero = torch.zeros_like(gamma)
    out = dict(y=y.to(BF), dx=dx.to(BF), stats=tot if G else None, mean=mean, rstd=rstd,
               dgamma=(zero if fault == "store" else case["prev_dgamma"]) + (dy * xh).sum(lead),
               dbeta=(zero if fault == "store" else case["prev_dbeta"]) + dy.sum(lead))
    d = case["dres"].to(f)
    out["dx_dres"] = (dx + d).to(BF) if fault == "dres_early" else (dx.to(BF).to(f) + d).to(BF)
    return out


def _norm_compare(case, exp, got, shape, G, exact):
    """What tests/test_gpu_norm_exact.py asserts, as a list of failure messages."""
    fails = []
    for n in ("y", "dx", "dx_dres"):
        msg = kc.gn_mismatch_report(got[n], exp[n], n, *shape, G) if G else kc.mismatch_report(got[n], exp[n], n)
        fails += [msg] if msg else []
    if G:
        msg = kc.stats_report(got["stats"], exp["stats"], "stats")
        fails += [msg] if msg else []
    for n in ("dgamma", "dbeta"):
        if exact:
            msg = kc.mismatch_report(got[n], (case["prev_" + n].double() + exp[n]).float(), n)
        else:
            msg = kc.param_grad_rule(got[n], case["prev_" + n], exp["rule2"], n)[0]
        fails += [msg] if msg else []
    return fails


def _balanced(kind, c):
    if kind == "gn":
        cid, B, HW, C, G = c
        case = kc.gn_balanced(cid)
        return case, G, (B, HW, C), kc.is_pow2(case["cnt"])
    cid, M, C = c
    return kc.ln_balanced(cid), 0, (M, C), True


@pytest.mark.parametrize("kind,c", [("gn", c) for c in kc.GN_BALANCED_CASES] + [("ln", c) for c in kc.LN_BALANCED_CASES], ids=lambda v: v if isinstance(v, str) else v[0])
def test_balanced_norm_cases_have_a_unique_representable_result_and_fp32_lands_on_it(kind, c):
    """On the very operands of the GPU file: the float64 results are bf16-representable and non-zero and every sum is an integer below
    2^24 (asserted inside norm_exact_expectation); inputs are integers in -3..3; the fp32 restatement of the kernels' formulas - with
    fl(1 / cnt), eps = 1e-5 and rstd one ulp up or down - passes the very comparisons of the GPU file, and with eps = 0 and an exact
    rstd the fp32 parameter gradients are exact too wherever the GPU file asks for that."""
    case, G, shape, pow2 = _balanced(kind, c)
    exact = pow2 or not G
    exp = kc.norm_exact_expectation(case, G, 0.0 if exact else 1e-5)
    assert float(case["x"].float().abs().max()) <= 3 and torch.equal(case["x"].float(), case["x"].float().round())
    assert float(exp["y"].float().abs().min()) >= 1 and float(exp["dx"].float().abs().min()) >= 0.5
    assert int((exp["dx_dres"].float() != exp["dx"].float() + case["dres"].float()).sum()) > 0 or case["x"].numel() < 64, "no dres tie in this case"
    if G:
        assert bool((case["c"][:, 1:] != case["c"][:, :-1]).all()), "neighbouring groups share a mean: a mixed-up group would not show"
        for d in range(1, shape[0]):  # every pair of images (B <= 3): no group shares (c, s), so none shares {sum, sumsq}, mean or xhat
            cs = torch.stack([case["c"], case["s"]], -1)
            assert bool((cs[d:] != cs[:-d]).any(-1).all()) and bool((case["c"][d:] != case["c"][:-d]).all()), f"images {d} apart share (c, s) in a group"
            assert bool((exp["stats"][d:, :, 0] != exp["stats"][:-d, :, 0]).all()), f"images {d} apart share a group's sum: another image's statistics would not show"
        if shape[0] > 1:
            assert bool((case["s"][1:] != case["s"][:-1]).any()) or G == 1, "no group changes its rstd from image to image"
    if not exact:  # the per-channel rule runs onto zero: its denominator knows nothing of the rounding of (previous value + sum)
        case["prev_dgamma"], case["prev_dbeta"] = torch.zeros_like(case["gamma"]), torch.zeros_like(case["gamma"])
    for ulps in (-1, 0, 1):
        fails = _norm_compare(case, exp, _norm_model(case, G, 1e-5, ulps), shape, G, exact)
        if exact:  # (fp32 parameter gradients at eps = 0: below)
            fails = [m for m in fails if not m.startswith(("dgamma", "dbeta"))]
        assert not fails, "\n".join(fails)
    if exact:
        got = _norm_model(case, G, 0.0, 0)
        fails = _norm_compare(case, exp, got, shape, G, True)
        assert not fails, "\n".join(fails)
        assert torch.equal(got["mean"].reshape(-1), exp["mean"].reshape(-1)) and torch.equal(got["rstd"].reshape(-1), exp["rstd"].reshape(-1))


def test_planted_norm_faults_are_each_caught():
    """A neighbour group's mean, the previous image's statistics or partial rows, one partial row dropped out of 200 (named by the
    report), dres added before the first rounding, and = instead of += on dgamma (where the sums are exact): each fails the comparison
    it is meant for."""
    for cid in ("pow2_cpg2", "cpg10_straddle_ty6"):
        c = kc.gn_case(cid)
        case, G, shape, pow2 = _balanced("gn", c)
        exp = kc.norm_exact_expectation(case, G, 0.0 if pow2 else 1e-5)
        eps = 0.0 if pow2 else 1e-5
        if not pow2:
            case["prev_dgamma"], case["prev_dbeta"] = torch.zeros_like(case["gamma"]), torch.zeros_like(case["gamma"])
        assert not _norm_compare(case, exp, _norm_model(case, G, eps), shape, G, pow2)
        f = _norm_compare(case, exp, _norm_model(case, G, eps, fault="neighbour_mean"), shape, G, pow2)
        assert any(m.startswith("y:") and "image 0 group 0" in m and "thread row" in m for m in f) and any(m.startswith("dx:") for m in f), f
        # the per-slice L2 of the older test would not see it at a realistic size; here every element of the group is wrong
        # image b with the statistics of image b - 1 (gn_apply_kernel / the backward reading stats + (b - 1) * 2G): stats itself is right
        f = _norm_compare(case, exp, _norm_model(case, G, eps, fault="previous_image"), shape, G, pow2)
        assert any(m.startswith("y:") and "image 0 group 0" in m for m in f) and any(m.startswith("dx:") for m in f) and not any("statistics differ" in m for m in f), f
        f = _norm_compare(case, exp, _norm_model(case, G, 1e-5, 1, fault="dres_early"), shape, G, pow2)
        assert [m.split(":")[0] for m in f if not m.startswith(("dgamma", "dbeta"))] == ["dx_dres"], f
        if pow2:  # (+= is proven where the sums are exact; the per-channel rule runs onto zero)
            f = _norm_compare(case, exp, _norm_model(case, G, eps, fault="store"), shape, G, True)
            assert sorted(m.split(":")[0] for m in f) == ["dbeta", "dgamma"], f
        rows = kc.gn_parts_decomposition(exp["stats"], 200, 5)
        assert kc.stats_report(rows.sum(1), exp["stats"], "stats", parts=rows) is None
        kept = rows.clone()
        kept[1, 137] = 0
        msg = kc.stats_report(kept.sum(1), exp["stats"], "stats", parts=rows)
        assert msg is not None and "image 1 group 0 sum" in msg and "workgroup [137]" in msg, msg
        # image b adds up the partial rows of image b - 1 (gn_sum_parts / gn_group_reduce_kernel reading part + (b - 1) * nparts * 2G)
        msg = kc.stats_report(rows.roll(1, 0).sum(1), exp["stats"], "stats", parts=rows)
        assert msg is not None and "image 0 group 0 sum" in msg, msg
        got = _norm_model(case, G, eps, stats=rows.roll(1, 0).sum(1))
        f = _norm_compare(case, exp, got, shape, G, pow2)
        assert any(m.startswith("y:") and "image 0 group 0" in m for m in f) and any("statistics differ" in m for m in f), f
    case, G, shape, _ = _balanced("ln", kc.LN_BALANCED_CASES[1])
    exp = kc.norm_exact_expectation(case, 0, 0.0)
    f = _norm_compare(case, exp, _norm_model(case, 0, 1e-5, -1, fault="dres_early"), shape, 0, True)
    assert "dx_dres" in [m.split(":")[0] for m in f], f
    f = _norm_compare(case, exp, _norm_model(case, 0, 0.0, fault="store"), shape, 0, True)
    assert sorted(m.split(":")[0] for m in f) == ["dbeta", "dgamma"], f


def test_groupnorm_geometry_mirror_is_the_librarys_and_the_cases_reach_their_branches(lib):
    """kc.gn_chunks / gn_layout against the workspace queries (host calls), and the branch every case id names."""
    for cid, B, HW, C, G in kc.GN_BALANCED_CASES:
        assert lib.sdt_groupnorm_fwd_workspace_bytes(B, HW, C, G) == kc.gn_fwd_workspace_bytes(B, HW, C, G), cid
        assert lib.sdt_groupnorm_bwd_workspace_bytes(B, HW, C) == kc.gn_bwd_workspace_bytes(B, HW, C), cid
        assert C % 8 == 0 and C % G == 0 and (HW * C // G) % 4 == 0 and B * HW * C <= 2_700_000, cid
    for B, HW, C, G in ((2, 4096, 320, 32), (1, 512 * 512, 128, 32), (3, 256, 2560, 32), (16, 64, 1280, 32), (1, 1, 8, 1), (2000, 7, 64, 8)):
        assert lib.sdt_groupnorm_fwd_workspace_bytes(B, HW, C, G) == kc.gn_fwd_workspace_bytes(B, HW, C, G)
        assert lib.sdt_groupnorm_bwd_workspace_bytes(B, HW, C) == kc.gn_bwd_workspace_bytes(B, HW, C)
    geo = {c[0]: (kc.gn_layout(c[3]), kc.gn_chunks(c[1], c[2], c[3], True), kc.gn_chunks(c[1], c[2], c[3], False), c) for c in kc.GN_BALANCED_CASES}
    pow2 = {cid for cid, B, HW, C, G in kc.GN_BALANCED_CASES if kc.is_pow2(HW * C // G)}
    assert {"pow2_cpg2", "pow2_cpg8"} <= pow2 and len(pow2) < len(kc.GN_BALANCED_CASES) - 4
    (Cv, TX, TY, J), _, _, c = geo["cpg10_straddle_ty6"]
    assert TY == 6 and TX * TY < 256 and (c[3] // c[4]) % 8 != 0 and 8 % (c[3] // c[4]) != 0
    assert geo["cpg3"][3][3] // geo["cpg3"][3][4] == 3
    (Cv, TX, TY, J), _, _, c = geo["cpg1_fewer_pixels_than_thread_rows"]
    assert c[3] == c[4] and c[2] < TY
    (Cv, TX, TY, J), _, _, c = geo["j2_ragged_second_vector"]
    assert J == 2 and TY == 1 and Cv % TX != 0
    (Cv, TX, TY, J), _, _, c = geo["g64_widest_c4096"]
    assert c[4] == 64 and c[3] == 4096 and J == 2 and Cv == 2 * TX
    (Cv, TX, TY, J), (ns, ps), (na, pa), c = geo["ty1_128_stat_rows_ragged_last"]
    assert TY == 1 and ns == kc.GN_MAX_INLINE_PARTS and c[2] % ps != 0 and (na, pa) != (ns, ps)
    assert geo["g8"][3][4] == 8 and geo["g8"][1][0] > 1 and geo["g8"][3][2] % geo["g8"][1][1] != 0
    assert 256 % (2 * geo["g24_2g_not_dividing_256"][3][4]) != 0 and geo["g1"][3][4] == 1
    where = kc.gn_locate(2, 636, 2048, 32, 1, 635, 2047)
    assert "image 1 group 31" in where and "chunk 127 of 128 (5 pixels each, the last 1)" in where and "chunk 158 of 159" in where, where
    # producer rows: both sides of the 128-row threshold, a ragged rows_per, and the odd slice splits through gn_group_reduce_kernel
    ns = {n for _, n in kc.GN_PARTS_CASES}
    assert {1, 2, 127, 128, 129, 200, 2048} <= ns and -(-200 // kc.GN_L2_PARTS) * kc.GN_L2_PARTS != 200
    assert any(kc.gn_case(cid)[4] == 24 and n > 128 for cid, n in kc.GN_PARTS_CASES) and any(kc.gn_case(cid)[4] == 64 and n > 128 for cid, n in kc.GN_PARTS_CASES)
    # LayerNorm: ln_rows_per_block / the 1024-workgroup cap (norm.hip sdt_layernorm_bwd) and the 4096-workgroup forward grid
    ln = {c[0]: c for c in kc.LN_BALANCED_CASES}
    for cid, M, C in kc.LN_BALANCED_CASES:
        assert lib.sdt_layernorm_bwd_partial_rows(M, C) == min(1024, -(-M // kc.ln_rows_per_block(C))), cid
        assert C % 8 == 0 and C <= 2048
    assert ln["nr4_clamped_tail_row"][1] % 4 != 0 and ln["maxv2_nr2_odd_m"][1] % 2 == 1 and 512 < ln["maxv2_nr2_odd_m"][2] <= 1024
    assert ln["maxv4"][2] > 1536 and (ln["cv129_ragged_third_vector"][2] // 8) % 64 == 1
    assert ln["grid_stride_loop"][1] > 1024 * 16 and ln["grid_stride_loop"][1] > 4096 * 4
    for D, R, win, S, eos in kc.CLIP_POOL_CASES:
        cc = kc.clip_pool_case(D, R, win, S, eos, 300 + D)
        assert S % 8 != 0 and {0, S - 1} <= set(cc["pos"].tolist())
        ids = cc["ids"].view(R, win, S)[:, 0]
        want = ids.argmax(1) if eos < 0 else torch.where((ids == eos).any(1), (ids == eos).int().argmax(1), 0)
        assert torch.equal(want.to(torch.int32), cc["pos"]), (D, want, cc["pos"])
        kc.norm_exact_expectation(cc["rows"], 0, 0.0)


# ================================================================================================ grouped off-chain launches
# (the tables and mirrors of tests/test_gpu_grouped_exact.py)
def _is_a_run(idx):
    return idx == list(range(idx[0], idx[0] + len(idx)))


def _dkv_table_facts(lib, table):
    """Per entry: (class, planned, launched, kblocks, gx, split), with the mirrors held to the library's byte queries."""
    from stable_diffusion_training_amd import _lib
    facts = []
    for spec in table:
        B, H, Nq, Nk, D, kind, packed, kw, causal = spec
        planned, chunk, launched, kblocks, gx = kc.dkv_group_plan(spec)
        d = _lib.SdtAttnDesc(B, H, Nq, Nk, D, H * D, H * D, H * D, H * D, D ** -0.5, int(causal), 0, 0, 0, 0, None)
        p = _lib.ctypes.addressof(d)
        assert lib.sdt_attention_bwd_delta_bytes(p) == kc.attention_delta_bytes(B, H, Nq), spec
        assert lib.sdt_attention_bwd_slab_bytes(p) == (planned * 2 * B * Nk * H * D * 4 if planned > 1 else 0), spec
        assert launched <= planned and (launched - 1) * chunk < Nq <= launched * chunk and chunk % 64 == 0
        assert kc.attention_instance(D)[:3] == kc.attention_instance(kc.ATTN_CLASS_TOPS[kc.attention_class(D)])[:3]
        facts.append((kc.attention_class(D), planned, launched, kblocks, gx, planned > 1))
    return facts


def _dkv_inputs_are_exact(spec):
    """A pair problem: pair_expect's own asserts ran in kc.dkv_group_problem; the tie is exactly 0, the lead at least 160 logits, dQ and
    dK nonzero wherever there is more than one key (and exactly zero where there is one).  A selector problem: the lead
    test_attention_selector_inputs_every_bit asserts - key weights of 1/2 .. 3 take at most ln 6 < 1.8 logits of it."""
    B, H, Nq, Nk, D, kind, packed, kw, causal = spec
    case, want = kc.dkv_group_problem(spec)
    if kind == "pair":
        tie, lead, top = kc.pair_min_gap(case, B, H, Nq, Nk, D, D ** -0.5)
        assert tie == 0.0 and lead >= 2 * 32.0 ** 2 / D ** 0.5 - 1e-9 >= 161.9 and lead >= 160 and top < 3000, spec
        for n in ("dq", "dk"):
            for b in range(B):
                for h in range(H):
                    blk = want[n][b, :, h * D: (h + 1) * D]
                    assert bool((blk != 0).any()) == (Nk > 1), (spec, n, b, h)
        assert bool((want["dv"] != 0).any())
    else:
        gap, top = kc.selector_min_gap(case, B, H, Nq, Nk, D, D ** -0.5)
        assert gap >= 2 * 32.0 ** 2 / D ** 0.5 - 1e-9 >= 161.9 and top < 3000, spec
        assert gap - math.log(6.0) >= 160
        if kw:
            w = kc.group_key_weights(Nk)
            assert set(w.tolist()) == {0.5, 1.0, 2.0, 3.0} if Nk >= 4 else True
        if causal:
            assert (case["target"] <= torch.arange(Nq)).all()


def test_grouped_dkv_tables_hold_what_they_are_listed_for(lib):
    from collections import Counter
    assert lib.sdt_attention_bwd_dkv_group_max() == kc.ATTN_GROUP_ABI
    # ---- DKV_GROUP_MIXED
    tab = kc.DKV_GROUP_MIXED
    facts = _dkv_table_facts(lib, tab)
    per_class = Counter(f[0] for f in facts)
    assert dict(per_class) == {0: 11, 1: 2, 2: 2, 3: 1, 4: 1, 5: 2} and len(tab) == len(set(tab)) == 19
    for cls, n in per_class.items():
        if n > 1:
            assert not _is_a_run([i for i, f in enumerate(facts) if f[0] == cls]), f"class {cls} is one run of the table"
    dkv, finish = kc.dkv_group_launches(tab)
    assert [len(l) for l in dkv] == [8, 3, 2, 2, 1, 1, 2] and [len(l) for l in finish] == [4]
    assert len({tab[i][0] for i in dkv[0]}) > 1 and len({tab[i][1] for i in dkv[0]}) > 1 and len({facts[i][4] for i in dkv[0]}) > 2  # B, H, gx differ inside one launch
    assert any(not f[5] and f[4] > 1 for f in facts), "an unsplit problem with gx > 1"
    assert any(not f[5] and f[3] == 3 for f in facts) and any(f[5] and f[3] > 1 for f in facts), "three key blocks unsplit; a split problem with kblocks > 1"
    assert any(f[5] and s[2] % kc.attention_qsplit(*s[:4], False)[1] for f, s in zip(facts, tab)), "a ragged last query chunk"
    assert any(s[0] * s[1] * s[2] % 4 for s in tab) and any(s[2] % 64 for s in tab if not kc.dkv_group_plan(s)[0] > 1)
    assert sum(s[6] for s in tab) == 3 and any(s[6] and f[5] for f, s in zip(facts, tab)) and any(s[6] and not f[5] for f, s in zip(facts, tab))
    assert [s[:5] for s in tab if s[5] == "selector"] == [(2, 2, 77, 77, 64), (2, 2, 64, 77, 8), (2, 2, 256, 77, 80)]
    assert sum(s[8] for s in tab) == 1 and sum(s[7] for s in tab) == 2 and any(s[3] < 8 and s[3] % 2 for s in tab) and any(s[3] == 1 for s in tab)
    assert {s[0] for s in tab} == {1, 2, 3} and {s[1] for s in tab} == {1, 2, 3, 4}
    # ---- DKV_GROUP_SPLITS
    tab = kc.DKV_GROUP_SPLITS
    facts = _dkv_table_facts(lib, tab)
    assert len(tab) == len(set(tab)) == 10 and all(f[5] for f in facts) and len({f[0] for f in facts}) == 2
    assert sum(s[4] == 8 and s[2] >= 1024 and s[3] <= 77 for s in tab) == 8 and Counter(f[0] for f in facts) == {0: 9, 2: 1}
    dkv, finish = kc.dkv_group_launches(tab)
    assert [len(l) for l in dkv] == [8, 1, 1] and [len(l) for l in finish] == [8, 2]
    assert all(f != d for f in finish for d in dkv), "the finishing tables are indexed as a dK/dV table is"
    assert len({facts[i][0] for i in finish[0]}) == 2 and len({facts[i][2] for i in finish[0]}) > 1  # both classes, several slab counts in one launch
    assert any(f[2] < f[1] for f in facts) and kc.dkv_group_plan(kc._pair(1, 1, 1600, 16, 8))[:3] == (6, 320, 5)
    # ---- DKV_GROUP_FULL
    tab = kc.DKV_GROUP_FULL
    facts = _dkv_table_facts(lib, tab)
    assert len(tab) == len(set(tab)) == kc.ATTN_GROUP_ABI and all(s[5] == "pair" and not f[5] for f, s in zip(facts, tab))
    assert {s[2] for s in tab} == {64, 70} and {s[3] for s in tab} == {2, 5, 16, 77}
    assert Counter(f[0] for f in facts) == {0: 13, 1: 7, 2: 12} and [len(l) for l in kc.dkv_group_launches(tab)[0]] == [8, 5, 7, 8, 4]


@pytest.mark.parametrize("name", ["DKV_GROUP_MIXED", "DKV_GROUP_SPLITS", "DKV_GROUP_FULL"])
def test_grouped_dkv_inputs_are_exact_and_a_decode_with_the_first_problems_heads_is_seen(name):
    """Every problem's inputs are exact (pair: tie 0, lead, nonzero dQ / dK; selector: lead).  The mirror of the grouped kernel's
    workgroup decode covers every (image, head, key block, query chunk) of every problem exactly once, so the grouped expectation
    is each problem's own; decoded with the H of the launch's first problem - a kernel that took H from problem 0 - every problem
    whose H differs from it loses or doubles workgroups, and the expectation says so for each of them."""
    tab = getattr(kc, name)
    for spec in tab:
        _dkv_inputs_are_exact(spec)
    seen = kc.dkv_group_cover(tab)
    assert set(seen.values()) == {1}
    for i, spec in enumerate(tab):
        gx = kc.dkv_group_plan(spec)[4]
        assert {k[1:] for k in seen if k[0] == i} == {(b, h, bx) for b in range(spec[0]) for h in range(spec[1]) for bx in range(gx)}, spec
    true, planted = kc.dkv_group_expect(tab), kc.dkv_group_expect(tab, h_of_first=True)
    first_h = {i: tab[l[0]][1] for l in kc.dkv_group_launches(tab)[0] for i in l}
    differ = 0
    for i, spec in enumerate(tab):
        want = kc.dkv_group_problem(spec)[1]
        for j, n in enumerate(("dk", "dv")):
            assert torch.equal(kc.bits(true[i][j]), kc.bits(want[n])), (spec, n)
            same = torch.equal(kc.bits(planted[i][j]), kc.bits(want[n]))
            # (one image decoded with MORE heads than it has: rest / H' = 0, rest % H' = rest - the one wrong H that changes nothing)
            assert same == (spec[1] == first_h[i] or (spec[0] == 1 and first_h[i] > spec[1])), (spec, n, first_h[i])
            differ += not same
            if not same:
                assert kc.mismatch_report(planted[i][j], want[n], n, tile=(128, spec[4])).startswith(f"{n}: ")
    assert differ >= 4


def test_grouped_column_sum_tables_hold_what_they_are_listed_for(lib):
    assert lib.sdt_colsum_batched_group_max() == kc.COLSUM_GROUP_ABI == len(kc.COLSUM_GROUP_MAXED) == len(set(kc.COLSUM_GROUP_MAXED))
    assert len(kc.COLSUM_CASES) <= kc.COLSUM_GROUP_ABI
    for N, ld, rows, batch, r in kc.COLSUM_GROUP_MAXED:
        assert 1 <= batch <= 5 and rows in (1, 7, 63, 64, 65, 200) and N in (8, 13, 250, 256, 264, 520)
        assert ld - -(-N // 8) * 8 in (0, 16) and rows * r < kc.LIMIT
    for col, n in ((0, 6), (2, 6), (3, 5)):
        assert len({c[col] for c in kc.COLSUM_GROUP_MAXED}) == n
    for name in ("COLSUM_CASES", "COLSUM_GROUP_MAXED"):
        tab, seen, counters = getattr(kc, name), set(), 0
        for N, ld, rows, batch, r in tab:
            ncb, nby, rpb, want = kc.colsum_plan(batch, rows, N, 512)
            counters += ncb * batch
            seen |= {"want clamp"} if (rows + 63) // 64 > want else set()
            seen |= {"ragged last row block"} if rows % rpb else set()
            seen |= {"several row blocks"} if nby > 1 else set()
            seen |= {"ld > N"} if ld > N else set()
            seen |= {"N % 8"} if N % 8 else set()
            seen |= {"behind a problem with many partial rows"} if counters > ncb * batch and nby == 1 else set()
        # (rows <= 200 never exceeds the planner's want: the clamp is COLSUM_CASES', which the GPU file also runs as one group)
        assert seen == {"ragged last row block", "several row blocks", "ld > N", "N % 8", "behind a problem with many partial rows"} | (
            {"want clamp"} if name == "COLSUM_CASES" else set()), (name, seen)
        assert counters * 4 <= kc.CNT_BYTES
