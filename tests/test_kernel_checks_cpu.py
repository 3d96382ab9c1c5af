"""The proof that tests/test_gpu_kernel_exact.py would fail on a subtly wrong kernel, without breaking a kernel on a GPU: start from
a correct expectation, plant the defects a whole-tensor norm cannot see (one element off by one bf16 ulp, one unwritten row, one
column that lost its product term, one store outside the output) and assert that the checkers of tests/kernel_checks.py report each
at the right coordinates.  Plus the arithmetic the exact tests rest on: every exact case keeps sum |a||b| below 2^24."""
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
    for (B, H, Nq, Nk, D, causal, packed, kw) in kc.ATTN_SELECTOR_CASES:
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
