"""Element-wise kernel checks on a real MI355X (the checkers and case tables: tests/kernel_checks.py; their proof on the CPU:
tests/test_kernel_checks_cpu.py).

The contraction kernels (sdt_gemm_nt_bf16 plain and gathered, the weight gradients, the GroupNorm statistics of the epilogues) and
attention on selector and tied-pair inputs run on small-integer operands whose exact answer is known: every output element, and every fp32
statistic, must hold the bits of the float64 reference rounded at the kernels' documented rounding points.  Outputs sit in guarded
arenas (tests/kernel_checks.py Guarded: a sentinel in front, behind and in 16 pad columns of every row, checked afterwards),
inputs in arenas whose guards are NaN, so that an out-of-range operand that reaches the arithmetic surfaces in the result.  Calls go
through _lib.call on raw pointers, because the ops layer hides ldc, ldres, lda and ld_rowbias.

The only tolerances in this file: the derived one-ulp bound of the activation sweep, the 1e-6 bound on the attention lse, and the
3x-of-emulation bounds of the per-row / per-slice checks (figures per shape: DESIGN.md "kernel test tolerances")."""
import ctypes

import pytest
import torch

from tests import kernel_checks as kc
from tests import op_checks as oc
from tests.kernel_checks import BF, Guarded, assert_equal_bits, exact_ints

pytestmark = pytest.mark.gpu

CNT = 65536  # the arrival-counter area at the head of every split workspace (include/sdt.h)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(g):
    return None if g is None else g.ptr


def _workspace(need, dev):
    return torch.zeros(max(int(need), CNT), dtype=torch.uint8, device=dev)


def _poison_slabs(ws):
    """Everything behind the counters holds NaN patterns / garbage; the counters are left alone (the contract says they are zero)."""
    ws[CNT:].fill_(0xFF)


def _counters_zero(ws):
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws[:CNT])) == 0, "arrival counters not reset"


def _check_all(guards):
    for what, g in guards.items():
        if g is not None:
            g.check(what)


# ================================================================================================ sdt_gemm_nt_bf16, plain rows
def _b_operand(b, taps, Kc, N, b_kmajor, nseg, dev):
    """b: logical [taps][Kc][N].  Returns (Guarded, ldb, b_tap_stride, b_seg_stride) in the layout the flags ask for."""
    if b_kmajor and nseg:
        ns = N // nseg
        g = Guarded(ns * taps * Kc, nseg, BF, dev, data=b.view(taps, Kc, ns, nseg).permute(2, 0, 1, 3).reshape(-1, nseg))
        return g, g.ld, Kc * g.ld, taps * Kc * g.ld
    if b_kmajor:
        g = Guarded(taps * Kc, N, BF, dev, data=b.reshape(taps * Kc, N))
        return g, g.ld, Kc * g.ld, 0
    g = Guarded(taps * N, Kc, BF, dev, data=b.transpose(1, 2).reshape(taps * N, Kc))
    return g, g.ld, N * g.ld, 0


@pytest.mark.parametrize("case", kc.GEMM_PLAIN_CASES, ids=[c[0] for c in kc.GEMM_PLAIN_CASES])
def test_gemm_nt_plain_every_bit(dev, case):
    """Every kernel plan_nt can choose for plain rows (the table in tests/kernel_checks.py names the branch of each case), both B
    layouts, column segments, taps > 1, every epilogue term with a pitch wider than N, ragged M / N / K.  Split cases run three
    times over a poisoned slab area: right each time, not merely the same as last time."""
    from stable_diffusion_training_amd import _lib
    name, M, N, Kc, taps, bkm, nseg, has_bias, rpb, has_res, use_ws, split, edge = case
    lib = _lib.load()
    need = lib.sdt_gemm_nt_workspace_bytes(M, N, Kc, taps)
    assert (need > 0) == split, f"{name}: the planner no longer {'splits' if split else 'leaves unsplit'} this shape"
    seed = 1000 + 7 * kc.GEMM_PLAIN_CASES.index(case)
    a = exact_ints((M, taps * Kc), -kc.GEMM_RANGE, kc.GEMM_RANGE, seed)
    b = exact_ints((taps, Kc, N), -kc.GEMM_RANGE, kc.GEMM_RANGE, seed + 1)
    bias = exact_ints((N,), -kc.EPI_RANGE, kc.EPI_RANGE, seed + 2, dtype=torch.float32) if has_bias else None
    nb = -(-M // rpb) if rpb else 0
    rowbias = exact_ints((nb, N), -kc.EPI_RANGE, kc.EPI_RANGE, seed + 3) if rpb else None
    res = exact_ints((M, N), -kc.EPI_RANGE, kc.EPI_RANGE, seed + 4) if has_res else None
    A = Guarded(M, taps * Kc, BF, dev, data=a)
    Bg, ldb, tap_stride, seg_stride = _b_operand(b, taps, Kc, N, bkm, nseg, dev)
    G = dict(A=A, B=Bg,
             bias=None if bias is None else Guarded(1, N, torch.float32, dev, data=bias),
             rowbias=None if rowbias is None else Guarded(nb, N, BF, dev, data=rowbias),
             residual=None if res is None else Guarded(M, N, BF, dev, data=res))
    dv = lambda t: None if t is None else t.to(dev)
    want = kc.expect_gemm_nt(a.to(dev), b.reshape(taps * Kc, N).to(dev), dv(bias), dv(rowbias), dv(res), rpb)
    ws = _workspace(need, dev) if use_ws else None
    tile = (edge, edge)
    for run in range(3 if (use_ws and split) else 1):
        if run:
            _poison_slabs(ws)
        C = Guarded(M, N, BF, dev)
        _lib.call("sdt_gemm_nt_bf16", A.ptr, Bg.ptr, C.ptr, _ptr(G["bias"]), _ptr(G["rowbias"]), _ptr(G["residual"]), M, N, Kc, taps,
                  A.ld, ldb, tap_stride, C.ld, G["residual"].ld if has_res else 0, rpb, _lib.GATHER_PLAIN, None,
                  None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), None, 0, bkm, nseg, seg_stride,
                  G["rowbias"].ld if rpb else 0, _stream())
        torch.cuda.synchronize()
        assert_equal_bits(C.t, want, f"{name} run {run}: C", tile=tile)
        C.check(f"{name}: C")
        _check_all(G)
        if ws is not None:
            _counters_zero(ws)


# ================================================================================================ sdt_gemm_nt_bf16, gathered rows
def _conv_nt(dev, lib, A, Wg, C, M, N, Kc, taps, tap_stride, mode, geom, bias, rowbias, res, rpb, bkm, ws):
    from stable_diffusion_training_amd import _lib
    _lib.call("sdt_gemm_nt_bf16", A.ptr, Wg.ptr, C.ptr, _ptr(bias), _ptr(rowbias), _ptr(res), M, N, Kc, taps, A.ld, Wg.ld, tap_stride,
              C.ld, res.ld if res is not None else 0, rpb, mode, None if geom is None else ctypes.addressof(geom),
              None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), None, 0, bkm, 0, 0,
              rowbias.ld if rowbias is not None else 0, _stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,pad", kc.CONV_EXACT_CASES)
def test_conv_fprop_dgrad_every_pixel(dev, B, H, W, Cin, Cout, k, stride, pad):
    """Forward convolution (bias, per-image row bias with a wide pitch, residual) and input gradient (with a residual) of the
    geometries of CONV_CASES against the float64 convolution: every border and corner pixel, bit for bit.  Halo-eligible
    geometries run at both tile widths (sdt_conv_halo_set_tile_width, restored in `finally`), with the workspace the planner asks
    for (split where it splits: three runs, the slab area poisoned before every launch but the first) and, where it asks for one,
    without it (unsplit).  The table names the kernel of each case."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    pad = kc.norm_pad(pad)
    (pt, pb), (pl, pr) = pad
    OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
    M, Min, taps = B * OH * OW, B * H * W, k * k
    plain = k == 1 and stride == 1 and pt == 0 and pl == 0
    seed = 2000 + H * W + Cin + Cout
    R, E = kc.GEMM_RANGE, kc.EPI_RANGE
    x, w = exact_ints((B, H, W, Cin), -R, R, seed), exact_ints((k, k, Cin, Cout), -R, R, seed + 1)
    bias, rb = exact_ints((Cout,), -E, E, seed + 2, dtype=torch.float32), exact_ints((B, Cout), -E, E, seed + 3)
    res, dy, dres = exact_ints((M, Cout), -E, E, seed + 4), exact_ints((B, OH, OW, Cout), -R, R, seed + 5), exact_ints((Min, Cin), -E, E, seed + 6)
    geom = None if plain else _lib.SdtConvGeom(B, H, W, OH, OW, k, k, stride, pt, pl)
    fmode = _lib.GATHER_PLAIN if plain else _lib.GATHER_FPROP
    dmode = _lib.GATHER_PLAIN if plain else _lib.GATHER_DGRAD
    # (the eight-taps-per-K-step path wants the 8 channels of a pixel as the whole row: lda = 8, no pad columns)
    X = Guarded(Min, Cin, BF, dev, data=x, pad=0 if Cin == 8 else 16)
    Wg = Guarded(taps * Cin, Cout, BF, dev, data=w.reshape(taps * Cin, Cout))
    G = dict(x=X, w=Wg, bias=Guarded(1, Cout, torch.float32, dev, data=bias), rowbias=Guarded(B, Cout, BF, dev, data=rb),
             residual=Guarded(M, Cout, BF, dev, data=res), dy=Guarded(M, Cout, BF, dev, data=dy), dres=Guarded(Min, Cin, BF, dev, data=dres))
    want_y = kc.epilogue_nt(kc.conv_ref64(x.to(dev), w.to(dev), stride, pad).view(M, Cout), bias.to(dev), rb.to(dev), res.to(dev), OH * OW)
    want_dx = kc.epilogue_nt(kc.conv_dgrad_ref64(dy.to(dev), w.to(dev), (H, W), stride, pad).reshape(Min, Cin), None, None, dres.to(dev))
    halo_f, halo_d = kc.halo_tile(H, W, Cin, M, k, stride, pad), kc.halo_tile(H, W, Cout, Min, k, stride, pad)
    try:
        for bn in ((64, 128) if (halo_f or halo_d) else (64,)):
            assert lib.sdt_conv_halo_set_tile_width(bn) in (64, 128)
            need_f = lib.sdt_gemm_nt_workspace_bytes(M, Cout, Cin, taps)
            need_d = lib.sdt_gemm_nt_workspace_bytes(Min, Cin, Cout, taps)
            for with_ws in ((True, False) if (need_f or need_d) else (False,)):
                ws = _workspace(max(need_f, need_d), dev) if with_ws else None
                # with the workspace (split where the planner splits): three runs, the slab area poisoned between them
                for run in range(3 if with_ws else 1):
                    if run:
                        _poison_slabs(ws)
                    tag = f"tile width {bn}, {'with' if with_ws else 'without'} workspace, run {run}"
                    Y = Guarded(M, Cout, BF, dev)
                    _conv_nt(dev, lib, X, Wg, Y, M, Cout, Cin, taps, Cin * Wg.ld, fmode, geom, G["bias"], G["rowbias"], G["residual"], OH * OW, 1, ws)
                    assert_equal_bits(Y.t.contiguous().view(B, OH, OW, Cout), want_y.view(B, OH, OW, Cout),
                                      f"fprop ({tag}): y [image][row][column][channel]" + (f", halo tile (images, rows, columns) = {halo_f}" if halo_f else ""))
                    Y.check(f"fprop ({tag}): y")
                    if ws is not None:
                        _counters_zero(ws)
                        _poison_slabs(ws)
                    DX = Guarded(Min, Cin, BF, dev)
                    _conv_nt(dev, lib, G["dy"], Wg, DX, Min, Cin, Cout, taps, Cin * Wg.ld, dmode, geom, None, None, G["dres"], 0, 0, ws)
                    assert_equal_bits(DX.t.contiguous().view(B, H, W, Cin), want_dx.view(B, H, W, Cin),
                                      f"dgrad ({tag}): dx [image][row][column][channel]" + (f", halo tile (images, rows, columns) = {halo_d}" if halo_d else ""))
                    DX.check(f"dgrad ({tag}): dx")
                    _check_all(G)
                    if ws is not None:
                        _counters_zero(ws)
    finally:
        lib.sdt_conv_halo_set_tile_width(64)


# ================================================================================================ weight gradients
def _wgrad_check(tag, DW, DB, SQ, want_w64, want_b64, dw_bf16):
    """dW as fp32: exactly the integer; as bf16: its RNE rounding; dbias exact; all sq slots together: the sum of squares of what
    was stored (integers below 2^53, exact in double)."""
    want = kc.rne_bf16(want_w64) if dw_bf16 else want_w64.float()
    assert torch.equal(want.double(), want_w64) or dw_bf16
    assert_equal_bits(DW.t, want, f"{tag}: dW")
    DW.check(f"{tag}: dW")
    if DB is not None:
        assert_equal_bits(DB.t.view(-1), want_b64.float(), f"{tag}: dbias")
        DB.check(f"{tag}: dbias")
    if SQ is not None:
        got, ref = float(SQ.sum().item()), float((want.double() ** 2).sum().item())
        assert got == ref, f"{tag}: sq_slots add up to {got!r}, the stored values' squares to {ref!r}"


def _dense_wgrad_operands(dev, case, idx):
    name, M, K1, N, K1v, Nv, nseg, split = case
    R = kc.WGRAD_RANGE
    a, dy = exact_ints((M, K1), -R, R, 3000 + 2 * idx), exact_ints((M, N), -R, R, 3001 + 2 * idx)
    A, DY = Guarded(M, K1, BF, dev, data=a), Guarded(M, N, BF, dev, data=dy)
    w64 = a.to(dev).double()[:, :K1v].t() @ dy.to(dev).double()[:, :Nv]
    b64 = dy.to(dev).double()[:, :Nv].sum(0)
    if nseg:  # segment s = columns [s * nseg, (s + 1) * nseg), stored as its own [K1v][ldw] matrix
        w64 = w64.view(K1v, Nv // nseg, nseg).permute(1, 0, 2).reshape(-1, nseg)
    return A, DY, w64, b64


def _dense_dw(dev, case, dw_bf16):
    name, M, K1, N, K1v, Nv, nseg, split = case
    rows, width = (K1v * (Nv // nseg), nseg) if nseg else (K1v, Nv)
    return Guarded(rows, width, BF if dw_bf16 else torch.float32, dev)


@pytest.mark.parametrize("dw_bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", kc.WGRAD_DENSE_CASES, ids=[c[0] for c in kc.WGRAD_DENSE_CASES])
def test_dense_wgrad_every_bit(dev, case, dw_bf16):
    """sdt_gemm_tn_wgrad, plain rows: both tiles, K1_valid < K1, N_valid < N, column segments, split and unsplit reductions (three
    runs over poisoned slabs where split), dW with ldw > N_valid and dbias inside guards, sq_slots."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    name, M, K1, N, K1v, Nv, nseg, split = case
    need = lib.sdt_gemm_tn_workspace_bytes(M, K1, N, 1, nseg, _lib.GATHER_PLAIN, None)
    assert (need > 0) == split, f"{name}: the planner no longer {'splits' if split else 'leaves unsplit'} this reduction"
    A, DY, w64, b64 = _dense_wgrad_operands(dev, case, kc.WGRAD_DENSE_CASES.index(case))
    ws = _workspace(need, dev) if split else None
    for run in range(3 if split else 1):
        if run:
            _poison_slabs(ws)
        DW, DB = _dense_dw(dev, case, dw_bf16), Guarded(1, Nv, torch.float32, dev)
        SQ = torch.zeros(int(lib.sdt_wgrad_sq_slots(K1, N, 1)), dtype=torch.float64, device=dev)
        _lib.call("sdt_gemm_tn_wgrad", A.ptr, DY.ptr, DW.ptr, dw_bf16, DB.ptr, M, K1, N, K1v, Nv, 1, A.ld, DY.ld, DW.ld, K1v * DW.ld, nseg,
                  K1v * DW.ld, _lib.GATHER_PLAIN, None, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), SQ.data_ptr(),
                  _stream())
        torch.cuda.synchronize()
        _wgrad_check(f"{name} run {run}", DW, DB, SQ, w64, b64, dw_bf16)
        A.check("A"); DY.check("dY")
        if ws is not None:
            _counters_zero(ws)


def test_grouped_dense_wgrad_every_bit(dev):
    """The same problems as ONE sdt_gemm_tn_wgrad_group call (fp32 and bf16 destinations alternating), three runs over poisoned slabs."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    ops, keep = [], []
    for i, case in enumerate(kc.WGRAD_DENSE_CASES):
        name, M, K1, N, K1v, Nv, nseg, split = case
        A, DY, w64, b64 = _dense_wgrad_operands(dev, case, i)
        ops.append((case, A, DY, w64, b64, i % 2))
    ws = None
    for run in range(3):
        outs, probs = [], []
        for case, A, DY, w64, b64, bf in ops:
            name, M, K1, N, K1v, Nv, nseg, split = case
            DW, DB = _dense_dw(dev, case, bf), Guarded(1, Nv, torch.float32, dev)
            SQ = torch.zeros(int(lib.sdt_wgrad_sq_slots(K1, N, 1)), dtype=torch.float64, device=dev)
            outs.append((DW, DB, SQ))
            probs.append(_lib.SdtTnProblem(A.ptr, DY.ptr, DW.ptr, DB.ptr, M, K1, N, K1v, Nv, A.ld, DY.ld, DW.ld, nseg, K1v * DW.ld, SQ.data_ptr(), bf))
        arr = (_lib.SdtTnProblem * len(probs))(*probs)
        if ws is None:
            need = lib.sdt_gemm_tn_wgrad_group_workspace_bytes(arr, len(probs))
            assert need > CNT, "no problem of the group splits its reduction any more"
            ws = _workspace(need, dev)
        else:
            _poison_slabs(ws)
        _lib.call("sdt_gemm_tn_wgrad_group", arr, len(probs), ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        for (case, A, DY, w64, b64, bf), (DW, DB, SQ) in zip(ops, outs):
            _wgrad_check(f"group {case[0]} run {run}", DW, DB, SQ, w64, b64, bf)
            A.check("A"); DY.check("dY")
        _counters_zero(ws)


def _conv_wgrad_operands(dev, case, idx):
    B, H, W, Cin, Cout, k, stride, pad, _ = case
    pad = kc.norm_pad(pad)
    OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
    R = kc.WGRAD_RANGE
    x, dy = exact_ints((B, H, W, Cin), -R, R, 4000 + 2 * idx), exact_ints((B, OH, OW, Cout), -R, R, 4001 + 2 * idx)
    K1v = 4 if Cin == 8 else Cin                   # the 4 -> 8 padded input channels: only the logical ones are written
    Nv = Cout - 4 if Cout in (72, 136) else Cout   # N_valid < N
    w64 = kc.conv_wgrad_ref64(x.to(dev), dy.to(dev), (k, k), stride, pad)[:, :, :K1v, :Nv].reshape(k * k * K1v, Nv)
    b64 = dy.to(dev).double().reshape(-1, Cout)[:, :Nv].sum(0)
    geom = (B, H, W, OH, OW, k, k, stride, pad[0][0], pad[1][0])
    return Guarded(B * H * W, Cin, BF, dev, data=x), Guarded(B * OH * OW, Cout, BF, dev, data=dy), w64, b64, geom, K1v, Nv


@pytest.mark.parametrize("dw_bf16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", kc.WGRAD_CONV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}x{c[3]}x{c[4]}s{c[6]}" for c in kc.WGRAD_CONV_CASES])
def test_conv_wgrad_every_bit(dev, case, dw_bf16):
    """sdt_gemm_tn_wgrad in fprop-gather mode: the three-tap kernel at the widths 96 / 48 / 24 and its smallest size, the nine-tap
    kernel (12 wide, stride 2, fewer than 64 pixels per image, 8 input channels), split and unsplit, against the float64 weight
    gradient; dW [tap][K1_valid][ldw > N_valid] and dbias inside guards, sq_slots."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    B, H, W, Cin, Cout, k, stride, pad, what = case
    X, DY, w64, b64, g, K1v, Nv = _conv_wgrad_operands(dev, case, kc.WGRAD_CONV_CASES.index(case))
    geom = _lib.SdtConvGeom(*g)
    M, taps = DY.rows, k * k
    need = lib.sdt_gemm_tn_workspace_bytes(M, Cin, Cout, taps, 0, _lib.GATHER_FPROP, ctypes.addressof(geom))
    assert (need > 0) == what.endswith("split"), f"{what}: workspace query says {need}"
    ws = _workspace(need, dev) if need else None
    for run in range(3 if need else 1):
        if run:
            _poison_slabs(ws)
        DW, DB = Guarded(taps * K1v, Nv, BF if dw_bf16 else torch.float32, dev), Guarded(1, Nv, torch.float32, dev)
        SQ = torch.zeros(int(lib.sdt_wgrad_sq_slots(Cin, Cout, taps)), dtype=torch.float64, device=dev)
        _lib.call("sdt_gemm_tn_wgrad", X.ptr, DY.ptr, DW.ptr, dw_bf16, DB.ptr, M, Cin, Cout, K1v, Nv, taps, X.ld, DY.ld, DW.ld, K1v * DW.ld, 0, 0,
                  _lib.GATHER_FPROP, ctypes.addressof(geom), None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                  SQ.data_ptr(), _stream())
        torch.cuda.synchronize()
        _wgrad_check(f"{what} run {run}", DW, DB, SQ, w64, b64, dw_bf16)
        X.check("x"); DY.check("dY")
        if ws is not None:
            _counters_zero(ws)


def test_grouped_conv_wgrad_every_bit(dev):
    """All convolution cases as ONE sdt_conv_wgrad_group call (the three-tap shapes share a launch, the others follow one by one);
    the grouped ABI has no pitch for dW, so its guards are the arena's front and back.  Three runs over poisoned slabs."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    ops = [(c,) + _conv_wgrad_operands(dev, c, i) + (i % 2,) for i, c in enumerate(kc.WGRAD_CONV_CASES)]
    ws = None
    for run in range(3):
        outs, probs = [], []
        for case, X, DY, w64, b64, g, K1v, Nv, bf in ops:
            B, H, W, Cin, Cout, k = case[:6]
            DW, DB = Guarded(k * k * K1v, Nv, BF if bf else torch.float32, dev, pad=0), Guarded(1, Nv, torch.float32, dev)
            SQ = torch.zeros(int(lib.sdt_wgrad_sq_slots(Cin, Cout, k * k)), dtype=torch.float64, device=dev)
            outs.append((DW, DB, SQ))
            probs.append(_lib.SdtConvWgradProblem(X.ptr, DY.ptr, DW.ptr, DB.ptr, _lib.SdtConvGeom(*g), Cin, Cout, K1v, Nv, X.ld, DY.ld, SQ.data_ptr(), bf))
        arr = (_lib.SdtConvWgradProblem * len(probs))(*probs)
        if ws is None:
            ws = _workspace(lib.sdt_conv_wgrad_group_workspace_bytes(arr, len(probs)), dev)
        else:
            _poison_slabs(ws)
        _lib.call("sdt_conv_wgrad_group", arr, len(probs), ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        for (case, X, DY, w64, b64, g, K1v, Nv, bf), (DW, DB, SQ) in zip(ops, outs):
            _wgrad_check(f"conv group {case[8]} run {run}", DW, DB, SQ, w64, b64, bf)
            X.check("x"); DY.check("dY")
        _counters_zero(ws)


# ================================================================================================ GroupNorm statistics of the epilogues
def _stats_equal(got, want64, what):
    """fp32 statistics against float64 integers, by value (adding 0 maps -0 to +0), with the checker's coordinates on failure."""
    assert_equal_bits(got.float().cpu() + 0.0, want64.float() + 0.0, what)
    assert torch.equal(got.double().cpu(), want64), what


@pytest.mark.parametrize("M,N,Kc,rpb,groups", kc.GN_DENSE_CASES)
def test_dense_epilogue_groupnorm_statistics_per_partial_row(dev, M, N, Kc, rpb, groups):
    """gn_stats of the Dense path (64- and 128-tiles): every partial row equals the float64 sum over exactly the rows and columns
    include/sdt.h:231-236 assigns to it - row 2r the groups that start inside the tile's columns, row 2r+1 the part of a group
    that began in the tile to the left.  Operands in -1..1: the fp32 sums are exact."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    a, b, bias = kc.gn_dense_operands(M, N, Kc)
    parts = lib.sdt_gemm_nt_gn_parts(M, N, Kc, 1, rpb, groups, _lib.GATHER_PLAIN, None)
    assert parts > 0, "this shape no longer produces GroupNorm statistics"
    edge = 2 * rpb // parts
    assert edge in (64, 128)
    nb = M // rpb
    A, Bg, Bi = Guarded(M, Kc, BF, dev, data=a), Guarded(Kc, N, BF, dev, data=b), Guarded(1, N, torch.float32, dev, data=bias)
    C, ST = Guarded(M, N, BF, dev), Guarded(1, nb * parts * groups * 2, torch.float32, dev, pad=0)
    _lib.call("sdt_gemm_nt_bf16", A.ptr, Bg.ptr, C.ptr, Bi.ptr, None, None, M, N, Kc, 1, A.ld, Bg.ld, Kc * Bg.ld, C.ld, 0, rpb, _lib.GATHER_PLAIN,
              None, None, 0, ST.ptr, groups, 1, 0, 0, 0, _stream())
    torch.cuda.synchronize()
    want = kc.expect_gemm_nt(a, b, bias=bias)
    assert_equal_bits(C.t.contiguous().cpu(), want, "y", tile=(edge, edge))
    C.check("y"); ST.check("gn_stats")
    got = ST.t.view(nb, parts, groups, 2)
    for img in range(nb):
        rows = [torch.arange(r * edge, (r + 1) * edge) for r in range(rpb // edge)]
        _stats_equal(got[img], kc.expect_gn_parts(want[img * rpb: (img + 1) * rpb], rows, groups, edge), f"image {img}: gn_stats [partial row][group][sum, sumsq], {edge}-tiles")


@pytest.mark.parametrize("B,H,W,Cin,Cout,groups", kc.GN_HALO_CASES)
def test_halo_epilogue_groupnorm_statistics_per_partial_row(dev, B, H, W, Cin, Cout, groups):
    """The same for the halo convolution at both tile widths (the two cut the channels differently): output row tile r = the
    th x tw pixel tile (ty, tx), r = ty * tiles_x + tx."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    x, w, bias = kc.gn_halo_operands(B, H, W, Cin, Cout)
    M = B * H * W
    ni, th, tw = kc.halo_tile(H, W, Cin, M, 3, 1, kc.norm_pad(1))
    geom = _lib.SdtConvGeom(B, H, W, H, W, 3, 3, 1, 1, 1)
    want = kc.rne_bf16(kc.conv_ref64(x, w, 1, kc.norm_pad(1)).view(M, Cout) + bias.double())
    rows = []
    for ty in range(H // th):
        for tx in range(W // tw):
            yy, xx = torch.meshgrid(torch.arange(ty * th, (ty + 1) * th), torch.arange(tx * tw, (tx + 1) * tw), indexing="ij")
            rows.append((yy * W + xx).reshape(-1))
    X, Wg, Bi = Guarded(M, Cin, BF, dev, data=x), Guarded(9 * Cin, Cout, BF, dev, data=w.reshape(9 * Cin, Cout)), Guarded(1, Cout, torch.float32, dev, data=bias)
    try:
        for bn in (64, 128):
            assert lib.sdt_conv_halo_set_tile_width(bn) in (64, 128)
            parts = lib.sdt_gemm_nt_gn_parts(M, Cout, Cin, 9, H * W, groups, _lib.GATHER_FPROP, ctypes.addressof(geom))
            assert ni == 1 and parts == 2 * len(rows), f"the halo planner tiles {H} x {W} differently now ({parts} partial rows)"
            C, ST = Guarded(M, Cout, BF, dev), Guarded(1, B * parts * groups * 2, torch.float32, dev, pad=0)
            _lib.call("sdt_gemm_nt_bf16", X.ptr, Wg.ptr, C.ptr, Bi.ptr, None, None, M, Cout, Cin, 9, X.ld, Wg.ld, Cin * Wg.ld, C.ld, 0, H * W,
                      _lib.GATHER_FPROP, ctypes.addressof(geom), None, 0, ST.ptr, groups, 1, 0, 0, 0, _stream())
            torch.cuda.synchronize()
            assert_equal_bits(C.t.contiguous().cpu(), want, f"y (tile width {bn})")
            C.check("y"); ST.check("gn_stats"); X.check("x"); Wg.check("w")
            got = ST.t.view(B, parts, groups, 2)
            for img in range(B):
                _stats_equal(got[img], kc.expect_gn_parts(want[img * H * W: (img + 1) * H * W], rows, groups, bn),
                             f"image {img}, tile width {bn}: gn_stats [partial row][group][sum, sumsq]")
    finally:
        lib.sdt_conv_halo_set_tile_width(64)


# ================================================================================================ attention
def _attn_arenas(dev, case, B, H, Nq, Nk, D, packed):
    C = H * D
    Q = Guarded(B * Nq, C, BF, dev, data=case["q"])
    DO = Guarded(B * Nq, C, BF, dev, data=case["dout"])
    if packed:  # k | v side by side in one arena: the row pitch of each is 2C + 16
        KV = Guarded(B * Nk, 2 * C, BF, dev, data=torch.cat([case["k"], case["v"]], -1))
        return Q, DO, KV, None, KV.ptr, KV.ptr + 2 * C, KV.ld
    K, V = Guarded(B * Nk, C, BF, dev, data=case["k"]), Guarded(B * Nk, C, BF, dev, data=case["v"])
    return Q, DO, K, V, K.ptr, V.ptr, K.ld


def _key_weights(dev, Nq, Nk):
    from stable_diffusion_training_amd import nets
    w = nets.key_chunk_weights(Nq, Nk, dev)
    if w is None:  # (as test_attention_key_weights: a synthetic vector where the chunks divide evenly)
        w = (1.0 + (torch.arange(Nk, device=dev) % 3 == 1).float()).contiguous()
    return w


@pytest.mark.parametrize("B,H,Nq,Nk,D,causal,packed,kw", kc.ATTN_SELECTOR_CASES + kc.ATTN_HEADDIM_CASES + kc.ATTN_EDGE_CASES)
def test_attention_selector_inputs_every_bit(dev, B, H, Nq, Nk, D, causal, packed, kw):
    """Selector inputs (tests/kernel_checks.py selector_case): the winner leads by >= 162 logits, P is exactly one-hot, so out must be
    the selected V row, dV the RNE of the integer sum of the dO rows that selected a key, dQ and dK zero (by value: either sign),
    lse2 the winning logit times log2(e) (+ log2 w) to 1e-6 relative (the kernel's two or three fp32 roundings: <= 2^-22).  Every
    operand and result sits in a guarded arena with a pitch wider than H*D; out-of-range tokens and features come from a zero page
    (attention.hip:23), so the NaN guards must not surface."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    C, scale = H * D, D ** -0.5
    case = kc.selector_case(B, H, Nq, Nk, D, causal, seed=Nq + Nk + D)
    w = _key_weights(dev, Nq, Nk) if kw else None
    WG = None if w is None else Guarded(1, Nk, torch.float32, dev, data=w, pad=0)
    want_o, want_lse, want_dv = kc.selector_expect(case, B, H, Nq, Nk, D, scale, None if w is None else w.cpu())
    Q, DO, KG, VG, kptr, vptr, ldkv = _attn_arenas(dev, case, B, H, Nq, Nk, D, packed)
    O, LSE = Guarded(B * Nq, C, BF, dev), Guarded(1, B * H * Nq, torch.float32, dev, pad=0)
    DQ = Guarded(B * Nq, C, BF, dev)
    if packed:
        DKV = Guarded(B * Nk, 2 * C, BF, dev)
        dkptr, dvptr, ldg = DKV.ptr, DKV.ptr + 2 * C, DKV.ld
    else:
        DK, DV = Guarded(B * Nk, C, BF, dev), Guarded(B * Nk, C, BF, dev)
        dkptr, dvptr, ldg = DK.ptr, DV.ptr, DK.ld
    desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, Q.ld, ldkv, ldkv, O.ld, scale, int(causal), DQ.ld, ldg, ldg, DO.ld, None if WG is None else WG.ptr)
    _lib.call("sdt_attention_fwd", Q.ptr, kptr, vptr, O.ptr, LSE.ptr, ctypes.addressof(desc), _stream())
    torch.cuda.synchronize()
    assert_equal_bits(O.t.contiguous().cpu().view(B, Nq, C), want_o, "out [batch][query][head * D + feature]", tile=(128, D))
    O.check("out"); LSE.check("lse")
    lse = LSE.t.view(B, H, Nq).double().cpu()
    bad = ~((lse - want_lse).abs() <= 1e-6 * want_lse.abs())
    assert not bad.any(), f"lse2: {int(bad.sum())} rows off, first at {bad.nonzero()[0].tolist()}: got {lse[bad][0].item()!r}, want {want_lse[bad][0].item()!r}"
    need = lib.sdt_attention_bwd_workspace_bytes(ctypes.addressof(desc))
    if (Nq >= 1024 and Nk <= 100):
        assert need > 4 * ((B * H * Nq + 3) // 4 * 4), "the dK/dV pass no longer splits the query range for this shape"
    claim = kc.ATTN_SPLIT_CLAIMS.get((B, H, Nq, Nk, bool(causal)))
    if claim is not None:  # (Nq = 1023 must get the delta part only, 1024 the slabs as well)
        assert (need > kc.attention_delta_bytes(B, H, Nq)) == claim, f"workspace {need} bytes: the dK/dV pass must {'split' if claim else 'not split'} here"
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)
    _lib.call("sdt_attention_bwd", Q.ptr, kptr, vptr, O.ptr, DO.ptr, LSE.ptr, DQ.ptr, dkptr, dvptr, ws.data_ptr(), need, ctypes.addressof(desc), _stream())
    torch.cuda.synchronize()
    if packed:
        DKV.check("dk | dv")
        dk, dv = DKV.t[:, :C].contiguous().cpu(), DKV.t[:, C:].contiguous().cpu()
    else:
        DK.check("dk"); DV.check("dv")
        dk, dv = DK.t.contiguous().cpu(), DV.t.contiguous().cpu()
    DQ.check("dq")
    assert_equal_bits(dv.reshape(B, Nk, C), want_dv, "dv [batch][key][head * D + feature]", tile=(128, D))
    for name, g in (("dq", DQ.t.contiguous().cpu()), ("dk", dk)):
        nz = (g != 0) | torch.isnan(g)
        assert not nz.any(), f"{name}: {int(nz.sum())} elements are not zero, first at row, column {nz.nonzero()[0].tolist()}: {g[nz][0].item()!r}"
    for what, g in (("q", Q), ("dout", DO), ("k", KG), ("v", VG), ("key_weight", WG), ("out", O), ("lse", LSE)):
        if g is not None:
            g.check(what)


def _attention_pairs(dev, B, H, Nq, Nk, D, packed, delta_only):
    """One tied-pair case (tests/kernel_checks.py pair_case / pair_expect) through sdt_attention_fwd and sdt_attention_bwd on guarded
    arenas, as the selector test runs its cases: out, dq, dk and dv must hold the expected bits, lse2 the winning logit x log2(e)
    + log2(ties) to 1e-6 relative.  delta_only: the workspace is the delta part alone, so a shape that would split the query range
    of the dK/dV pass must be served by the unsplit kernel (attention.hip:819) - with the unsplit expectation."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    C, scale = H * D, D ** -0.5
    case = kc.pair_case(B, H, Nq, Nk, D, seed=Nq + Nk + D)
    planned, chunk, _ = kc.attention_qsplit(B, H, Nq, Nk, False)
    want = kc.pair_expect(case, B, H, Nq, Nk, D, scale, kv_chunk=chunk if planned > 1 and not delta_only else None)
    Q, DO, KG, VG, kptr, vptr, ldkv = _attn_arenas(dev, case, B, H, Nq, Nk, D, packed)
    O, LSE = Guarded(B * Nq, C, BF, dev), Guarded(1, B * H * Nq, torch.float32, dev, pad=0)
    DQ = Guarded(B * Nq, C, BF, dev)
    if packed:
        DKV = Guarded(B * Nk, 2 * C, BF, dev)
        dkptr, dvptr, ldg = DKV.ptr, DKV.ptr + 2 * C, DKV.ld
    else:
        DK, DV = Guarded(B * Nk, C, BF, dev), Guarded(B * Nk, C, BF, dev)
        dkptr, dvptr, ldg = DK.ptr, DV.ptr, DK.ld
    desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, Q.ld, ldkv, ldkv, O.ld, scale, 0, DQ.ld, ldg, ldg, DO.ld, None)
    _lib.call("sdt_attention_fwd", Q.ptr, kptr, vptr, O.ptr, LSE.ptr, ctypes.addressof(desc), _stream())
    torch.cuda.synchronize()
    got = dict(o=O.t.contiguous().cpu().view(B, Nq, C))
    assert_equal_bits(got["o"], want["o"], "out [batch][query][head * D + feature]", tile=(128, D))
    O.check("out"); LSE.check("lse")
    lse = LSE.t.view(B, H, Nq).double().cpu()
    bad = ~((lse - want["lse2"]).abs() <= 1e-6 * want["lse2"].abs())
    assert not bad.any(), f"lse2: {int(bad.sum())} rows off, first at {bad.nonzero()[0].tolist()}: got {lse[bad][0].item()!r}, want {want['lse2'][bad][0].item()!r}"
    need = lib.sdt_attention_bwd_workspace_bytes(ctypes.addressof(desc))
    claim = kc.ATTN_SPLIT_CLAIMS[(B, H, Nq, Nk, False)]
    assert (need > kc.attention_delta_bytes(B, H, Nq)) == claim, f"workspace {need} bytes: the dK/dV pass must {'split' if claim else 'not split'} here"
    if delta_only:
        assert claim
        need = kc.attention_delta_bytes(B, H, Nq)
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.sdt_attention_bwd(Q.ptr, kptr, vptr, O.ptr, DO.ptr, LSE.ptr, DQ.ptr, dkptr, dvptr, ws.data_ptr(), need, ctypes.addressof(desc), _stream())
    assert rc == 0, f"sdt_attention_bwd returned {rc}: {lib.sdt_last_error()!r}"
    torch.cuda.synchronize()
    if packed:
        DKV.check("dk | dv")
        got["dk"], got["dv"] = (t.contiguous().cpu().view(B, Nk, C) for t in (DKV.t[:, :C], DKV.t[:, C:]))
    else:
        DK.check("dk"); DV.check("dv")
        got["dk"], got["dv"] = (g.t.contiguous().cpu().view(B, Nk, C) for g in (DK, DV))
    DQ.check("dq")
    got["dq"] = DQ.t.contiguous().cpu().view(B, Nq, C)
    msgs = kc.pair_reports(got, want, D)
    assert not msgs, "\n".join(msgs)
    for what, g in (("q", Q), ("dout", DO), ("k", KG), ("v", VG), ("out", O), ("lse", LSE)):
        if g is not None:
            g.check(what)


@pytest.mark.parametrize("B,H,Nq,Nk,D,packed", kc.ATTN_PAIR_CASES)
def test_attention_tied_pairs_every_bit(dev, B, H, Nq, Nk, D, packed):
    """Tied-pair inputs: every query ties two keys that usually lie in different 64-key tiles, P is exactly 1/2, 1/2, and the
    extras make dS.K and dS^T.Q nonzero: dQ and dK are exact multiples of scale / 4, pinned in every bit - also through the
    query-split slabs and attn_kv_finish_kernel (the last four cases)."""
    _attention_pairs(dev, B, H, Nq, Nk, D, packed, delta_only=False)


@pytest.mark.parametrize("B,H,Nq,Nk,D,packed", [kc.ATTN_PAIR_SPLIT_CASES[1], kc.ATTN_PAIR_SPLIT_CASES[2]])
def test_attention_split_shape_with_delta_only_workspace(dev, B, H, Nq, Nk, D, packed):
    """A shape that splits the query range, called with workspace_bytes = 4 * ceil4(B * H * Nq): OK, and the exact bits."""
    _attention_pairs(dev, B, H, Nq, Nk, D, packed, delta_only=True)


@pytest.mark.parametrize("B,H,N,D", [(3, 12, 77, 64), (1, 3, 77, 16), (2, 8, 256, 40), (2, 4, 200, 80), (1, 2, 130, 128), (1, 2, 64, 160)])
def test_attention_causal_row_zero_is_v_row_zero(dev, B, H, N, D):
    """Query 0 of a causal problem sees one key: P = exp2(0) = 1, l = 1, so O[:, 0] == V[:, 0] bit for bit for any Gaussian q, k, v
    (the forward only: dV[0] collects from every query)."""
    from stable_diffusion_training_amd import _lib
    C = H * D
    g = torch.Generator().manual_seed(N + D)
    q, k, v = (torch.randn(B, N, C, generator=g).to(BF) for _ in range(3))
    Q, K, V = (Guarded(B * N, C, BF, dev, data=t) for t in (q, k, v))
    O = Guarded(B * N, C, BF, dev)
    desc = _lib.SdtAttnDesc(B, H, N, N, D, Q.ld, K.ld, V.ld, O.ld, D ** -0.5, 1, 0, 0, 0, 0, None)
    _lib.call("sdt_attention_fwd", Q.ptr, K.ptr, V.ptr, O.ptr, None, ctypes.addressof(desc), _stream())
    torch.cuda.synchronize()
    assert_equal_bits(O.t.contiguous().cpu().view(B, N, C)[:, 0], v[:, 0], "out[:, 0] against v[:, 0]: [batch][head * D + feature]")
    O.check("out")


ATTN_ROW_CASES = kc.ATTN_ROW_CASES + kc.ATTN_ROW_HEADDIM_CASES  # (B, H, Nq, Nk, D, causal)
ROW_FACTOR = kc.ROW_FACTOR  # kernel worst row <= 3 x emulation worst row (what the emulation leaves out: kernel_checks.attention_ref_and_emulation)


def _attention_rows(dev, q, k, v, do, H, D, causal, what, key_weight=None):
    """Per (batch, head, query row) for O and dQ, per (batch, head, key row) for dK and dV: relative L2 error against the float64
    reference; the kernel's worst row must stay within ROW_FACTOR of the worst row of the rounding-point emulation on the same
    inputs.  The figures are printed (DESIGN.md "kernel test tolerances" records them)."""
    from stable_diffusion_training_amd import ops
    B = q.shape[0]
    scale = D ** -0.5
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ops.attention(qg, kg, vg, H, scale, causal, key_weight)
    o.backward(do)
    torch.cuda.synchronize()
    ref, emu, mag = kc.attention_ref_and_emulation(q, k, v, do, H, scale, causal, key_weight)
    got = dict(o=o.detach(), dq=qg.grad, dk=kg.grad, dv=vg.grad)
    fails = []
    for n in ("o", "dq", "dk", "dv"):
        rows = lambda t: t.double().view(B, -1, H, D)
        rk = kc.per_slice_rel(rows(got[n]), rows(ref[n]), (3,), rows(mag[n]))
        re = kc.per_slice_rel(rows(emu[n]), rows(ref[n]), (3,), rows(mag[n]))
        (ik, wk), (ie, we) = kc.worst_slices(rk, 1)[0], kc.worst_slices(re, 1)[0]
        fb = kc.floor_binds(rows(ref[n]), (3,), rows(mag[n]))
        print(f"ROWS {what} {n}: kernel worst row {wk:.3e} at (batch, row, head) {ik}, emulation worst row {we:.3e} at {ie}; measured against "
              f"the floor: {int(fb.sum())} of {fb.numel()} rows, the kernel's worst row {'among them' if bool(fb[ik]) else 'not'}")
        if not wk <= ROW_FACTOR * we:
            fails.append(f"{n}: kernel worst row {wk:.3e} at (batch, row, head) {ik} > {ROW_FACTOR} x emulation worst row {we:.3e}")
    assert not fails, f"{what}: " + "; ".join(fails)


@pytest.mark.parametrize("B,H,Nq,Nk,D,causal", ATTN_ROW_CASES)
def test_attention_gaussian_inputs_per_row(dev, B, H, Nq, Nk, D, causal):
    g = torch.Generator().manual_seed(Nq + D)
    q, do = (torch.randn(B, Nq, H * D, generator=g).to(BF).to(dev) for _ in range(2))
    k, v = (torch.randn(B, Nk, H * D, generator=g).to(BF).to(dev) for _ in range(2))
    _attention_rows(dev, q, k, v, do, H, D, causal, f"{(B, H, Nq, Nk, D, causal)}")


@pytest.mark.parametrize("B,H,Nq,Nk,D", kc.ATTN_ROW_KEYWEIGHT_CASES)
def test_attention_gaussian_inputs_per_row_with_key_weights(dev, B, H, Nq, Nk, D):
    """The same rule with the key weights of the clamped chunks (64 queries x 77 keys: keys 13..63 count twice), at two head dims
    whose forward takes the row sum from the ones column."""
    from stable_diffusion_training_amd import nets
    w = nets.key_chunk_weights(Nq, Nk, dev)
    assert w is not None and kc.attention_msum(D)
    g = torch.Generator().manual_seed(Nq + D)
    q, do = (torch.randn(B, Nq, H * D, generator=g).to(BF).to(dev) for _ in range(2))
    k, v = (torch.randn(B, Nk, H * D, generator=g).to(BF).to(dev) for _ in range(2))
    _attention_rows(dev, q, k, v, do, H, D, False, f"{(B, H, Nq, Nk, D)} key weights", key_weight=w)


@pytest.mark.parametrize("D", [64, 40, 80])
@pytest.mark.parametrize("spike", [6.0, 1.0, 0.35])
def test_attention_rescale_spikes_per_row(dev, D, spike):
    """The spike cases of test_attention_rescale_branch_forced (both sides of the deferred rescale), judged per row."""
    B, H, N = 1, 2, 320
    g = torch.Generator().manual_seed(D)
    q, k, v, do = (torch.randn(B, N, H * D, generator=g).to(BF) for _ in range(4))
    k[:, 200] = q[:, 7] * spike
    k[:, 290] = q[:, 150] * spike
    _attention_rows(dev, *(t.to(dev) for t in (q, k, v, do)), H, D, False, f"spike {spike} D {D}")


# ================================================================================================ norms, per slice
def _norm_slices(dev, kind, shape, silu):
    """y and dx per (image, group) (GroupNorm) or per row (LayerNorm): relative L2 against float64; dgamma / dbeta per channel:
    |error| / sum |terms|.  The kernel's worst slice must stay within ROW_FACTOR of the worst slice of the rounding-point emulation
    (kernel_checks.norm_ref_and_emulation) on the same inputs; figures printed for DESIGN.md."""
    from stable_diffusion_training_amd import ops
    from tests.test_gpu_kernels import FakeStore, rnd
    C = shape[-1]
    fs = FakeStore([("n/scale", (C,)), ("n/bias", (C,))], dev, seed=C)
    x = (rnd(shape, dev, 1) * 2 + 0.5).requires_grad_(True)
    dy = rnd(shape, dev, 2)
    G = 32 if kind == "group" else 0
    y = ops.group_norm(x, fs.st, "n", 32, 1e-5, silu=silu) if G else ops.layer_norm(x, fs.st, "n", 1e-5)
    y.backward(dy)
    torch.cuda.synchronize()
    gamma, beta = fs.w["n/scale"].to(dev), fs.w["n/bias"].to(dev)
    ref, emu, terms = kc.norm_ref_and_emulation(x.detach(), gamma, beta, dy, G, 1e-5, silu)
    got = dict(y=y.detach(), dx=x.grad, dgamma=fs.st.g("n/scale"), dbeta=fs.st.g("n/bias"))
    fails = []
    for n in ("y", "dx", "dgamma", "dbeta"):
        if n in ("y", "dx"):
            if G:
                v = lambda t: t.double().view(shape[0], shape[1], G, C // G)
                rk, re = kc.per_slice_rel(v(got[n]), v(ref[n]), (1, 3)), kc.per_slice_rel(v(emu[n]), v(ref[n]), (1, 3))
            else:
                rk, re = kc.per_slice_rel(got[n], ref[n], (1,)), kc.per_slice_rel(emu[n], ref[n], (1,))
        else:
            rk, re = (got[n].double() - ref[n]).abs() / terms[n], (emu[n] - ref[n]).abs() / terms[n]
        (ik, wk), (ie, we) = kc.worst_slices(rk, 1)[0], kc.worst_slices(re, 1)[0]
        print(f"SLICES {kind} {shape} silu={silu} {n}: kernel worst slice {wk:.3e} at {ik}, emulation worst slice {we:.3e} at {ie}"
              + ("; the 2^-24 floor binds" if n in ("dgamma", "dbeta") and we < 2.0 ** -24 else ""))
        # dgamma / dbeta are stored in fp32: whatever the summation order, the stored value carries up to half an fp32 ulp of its
        # magnitude (<= sum |terms|), 2^-24 - the least the emulation's figure can mean (a short sum of bf16 values can come out exact)
        if n in ("dgamma", "dbeta"):
            we = max(we, 2.0 ** -24)
        if not wk <= ROW_FACTOR * we:
            fails.append(f"{n}: kernel worst slice {wk:.3e} at {ik} > {ROW_FACTOR} x emulation worst slice {we:.3e}")
    assert not fails, f"{kind} norm {shape}: " + "; ".join(fails)


@pytest.mark.parametrize("B,HW,C,silu", [(2, 64, 320, True), (2, 4096, 320, True), (3, 256, 2560, True), (2, 64, 1920, False), (2, 100, 32, True), (1, 1024, 960, True),
                                         (1, 512 * 512, 128, True)])  # the VAE's size: 128 own-pass statistics rows (gn_group_reduce_kernel: test_gpu_norm_exact.py)
def test_groupnorm_per_image_and_group(dev, B, HW, C, silu):
    _norm_slices(dev, "group", (B, HW, C), silu)


@pytest.mark.parametrize("M,C", [(512, 320), (77 * 3, 768), (100, 1280), (64, 48), (33, 2048), (4096, 640), (2048, 2048)])
def test_layernorm_per_row(dev, M, C):
    _norm_slices(dev, "layer", (M, C), False)


# ================================================================================================ activations over every bf16 value
ACTS = (("silu", 0), ("quick_gelu", 1), ("gelu_erf", 2))


def _violations_msg(what, bad, x, got, ref64):
    i = bad[:5].tolist()
    return (f"{what}: {bad.numel()} of {x.numel()} bf16 inputs miss the bound; first x = {[x[j].item() for j in i]}, got {[got[j].item() for j in i]}, "
            f"float64 reference {[ref64[j].item() for j in i]}")


def _act_assert(what, x, got, ref64, dy_abs):
    """NaN in -> NaN out; every finite input -> a finite result inside the derived bound (tests/kernel_checks.py act_bound_violations);
    +-inf inputs are not asserted."""
    x64, got64 = x.double(), got.double().cpu()
    nan, fin = torch.isnan(x64), torch.isfinite(x64)
    assert torch.isnan(got64[nan]).all(), f"{what}: a NaN input gave a number"
    notfin = (~torch.isfinite(got64)) & fin
    assert not notfin.any(), f"{what}: {int(notfin.sum())} finite inputs gave a non-finite result, first x = {x64[notfin][:5].tolist()} -> {got64[notfin][:5].tolist()}"
    bad = kc.act_bound_violations(got64[fin], ref64[fin], x64[fin], dy_abs[fin] if torch.is_tensor(dy_abs) else torch.full_like(x64[fin], dy_abs))
    assert bad.numel() == 0, _violations_msg(what, bad, x64[fin], got64[fin], ref64[fin])


@pytest.mark.parametrize("kind,act", ACTS)
def test_activations_over_every_bf16_value(dev, kind, act):
    """sdt_act_fwd and sdt_act_bwd (dy = 1 and dy = -0.75) on all 65536 bf16 bit patterns against the float64 function."""
    from stable_diffusion_training_amd import _lib
    x = kc.all_bf16_patterns()
    n = x.numel()
    X = Guarded(1, n, BF, dev, data=x)
    Y = Guarded(1, n, BF, dev)
    _lib.call("sdt_act_fwd", X.ptr, Y.ptr, n, act, _stream())
    torch.cuda.synchronize()
    Y.check(f"{kind}: y")
    fin = torch.isfinite(x.double())
    xs = torch.where(fin, x.double(), torch.zeros((), dtype=torch.float64))
    y64, d64 = kc.act_ref64(kind, xs)
    _act_assert(f"{kind} forward", x, Y.t.view(-1), y64, 1.0)
    for dyv in (1.0, -0.75):
        DYg = Guarded(1, n, BF, dev, data=torch.full((n,), dyv).to(BF))
        DX = Guarded(1, n, BF, dev)
        _lib.call("sdt_act_bwd", X.ptr, DYg.ptr, DX.ptr, n, act, _stream())
        torch.cuda.synchronize()
        DX.check(f"{kind}: dx")
        _act_assert(f"{kind} backward, dy = {dyv}", x, DX.t.view(-1), d64 * dyv, abs(dyv))
    X.check("x")


def test_geglu_gate_over_every_bf16_value(dev):
    """sdt_geglu_fwd / sdt_geglu_bwd with the gate sweeping all bf16 values (value column 1 and -0.75, dout 1 and -0.75): out = a *
    gelu_tanh(g), d a = dout * gelu_tanh(g), d g = dout * a * gelu_tanh'(g).  A gate beyond 1.8e19 used to return NaN from the
    derivative (0 * inf in gelu_tanh_grad, sdt_common.h); the true derivative there is 0 or 1."""
    from stable_diffusion_training_amd import _lib
    g = kc.all_bf16_patterns()
    F = g.numel()
    fin = torch.isfinite(g.double())
    gs = torch.where(fin, g.double(), torch.zeros((), dtype=torch.float64))
    y64, d64 = kc.act_ref64("gelu_tanh", gs)
    for av, dov in ((1.0, 1.0), (-0.75, 1.0), (1.0, -0.75)):
        h = torch.cat([torch.full((F,), av).to(BF), g]).view(1, 2 * F)
        Hg, O = Guarded(1, 2 * F, BF, dev, data=h), Guarded(1, F, BF, dev)
        _lib.call("sdt_geglu_fwd", Hg.ptr, O.ptr, 1, F, _stream())
        torch.cuda.synchronize()
        O.check("geglu out")
        _act_assert(f"geglu forward, value {av}", g, O.t.view(-1), y64 * av, abs(av))
        DO, DH = Guarded(1, F, BF, dev, data=torch.full((F,), dov).to(BF)), Guarded(1, 2 * F, BF, dev)
        _lib.call("sdt_geglu_bwd", Hg.ptr, DO.ptr, DH.ptr, 1, F, _stream())
        torch.cuda.synchronize()
        DH.check("geglu dh")
        dh = DH.t.view(-1)
        _act_assert(f"geglu backward, d value (dout {dov})", g, dh[:F], y64 * dov, abs(dov))
        _act_assert(f"geglu backward, d gate (value {av}, dout {dov})", g, dh[F:], d64 * (av * dov), abs(av * dov))
        Hg.check("h")


@pytest.mark.parametrize("F,K", oc.FF_GEGLU_PAIRS)
def test_ff_geglu_fused_epilogue_at_ragged_m(dev, F, K):
    """sdt_ff_geglu_fwd where its last row tile is ragged: the smallest M the fused kernel serves, the smallest served M with
    M % 128 == 1 and with M % 128 == 127 (asked of sdt_ff_geglu_supported; the CPU proof pins them).  Every M the feed-forward test
    of tests/test_gpu_kernels.py hands this kernel is a multiple of 128.  x sits in an arena whose rows >= M are NaN, h and out in
    guarded arenas (the ABI has no pitch for them: pad 0): h must hold the integer GEMM bit for bit, out what sdt_geglu_fwd writes
    from that h (pinned over every bf16 gate by test_geglu_gate_over_every_bf16_value), and every guard must be intact."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    Ms = oc.ff_geglu_served(lib.sdt_ff_geglu_supported, F, K)
    assert Ms == oc.FF_GEGLU_M[(F, K)], f"the planner serves other shapes now: {Ms}"
    w = exact_ints((K, 2 * F), -kc.GEMM_RANGE, kc.GEMM_RANGE, 7 + F)
    bias = exact_ints((2 * F,), -kc.EPI_RANGE, kc.EPI_RANGE, 8 + F, dtype=torch.float32)
    Wg = Guarded(K, 2 * F, BF, dev, data=w, pad=0)
    Bg = Guarded(1, 2 * F, torch.float32, dev, data=bias, pad=0)
    for M in sorted(set(Ms)):
        x = exact_ints((M, K), -kc.GEMM_RANGE, kc.GEMM_RANGE, M)
        X = Guarded(M, K, BF, dev, data=x, pad=0)
        H, O, O2 = Guarded(M, 2 * F, BF, dev, pad=0), Guarded(M, F, BF, dev, pad=0), Guarded(M, F, BF, dev, pad=0)
        _lib.call("sdt_ff_geglu_fwd", X.ptr, Wg.ptr, Bg.ptr, H.ptr, O.ptr, M, F, K, _stream())
        torch.cuda.synchronize()
        assert_equal_bits(H.t, kc.expect_gemm_nt(x.to(dev), w.to(dev), bias.to(dev)), f"M {M}: h", tile=(128, 128))
        _lib.call("sdt_geglu_fwd", H.ptr, O2.ptr, M, F, _stream())
        torch.cuda.synchronize()
        assert_equal_bits(O.t, O2.t.clone(), f"M {M}: out against sdt_geglu_fwd of the same h", tile=(128, 64))
        for what, g in (("h", H), ("out", O), ("separate out", O2), ("x", X), ("W1", Wg), ("bias", Bg)):
            g.check(f"M {M}: {what}")


# ================================================================================================ tail sizes, zero sizes
def test_cast_f32_to_bf16_tails_and_special_values(dev):
    """n % 8 != 0; values on RNE ties, +-inf, NaN and fp32 denormals: the result is torch's RNE cast bit for bit (NaN: any NaN)."""
    from stable_diffusion_training_amd import _lib
    special = torch.tensor([1.00390625, 1.01171875, -1.00390625, 257.0, 259.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.1754942e-38,
                            3.3895314e38, 3.4e38, 0.0, -0.0, 65280.0, 65408.0], dtype=torch.float32)
    for n in (1, 7, 9, 1023, 4099):
        gen = torch.Generator().manual_seed(n)
        x = torch.randn(n, generator=gen) * 100
        x[: min(n, special.numel())] = special[: min(n, special.numel())]
        X, Y = Guarded(1, n, torch.float32, dev, data=x), Guarded(1, n, BF, dev)
        _lib.call("sdt_cast_f32_to_bf16", X.ptr, Y.ptr, n, _stream())
        torch.cuda.synchronize()
        got, want = Y.t.view(-1).cpu(), x.to(BF)
        nan = torch.isnan(want)
        assert torch.isnan(got[nan]).all()
        assert_equal_bits(torch.where(nan, torch.zeros((), dtype=BF), got), torch.where(nan, torch.zeros((), dtype=BF), want), f"cast n = {n}")
        Y.check(f"cast n = {n}: y"); X.check("x")


def test_transpose_odd_sizes(dev):
    from stable_diffusion_training_amd import _lib
    for batch, R, C in ((1, 1, 1), (2, 63, 65), (3, 129, 7), (1, 5, 131)):
        x = exact_ints((batch * R, C), -100, 100, R + C)
        X, Y = Guarded(batch * R, C, BF, dev, data=x, pad=0), Guarded(batch * C, R, BF, dev, pad=0)
        _lib.call("sdt_transpose_bf16", X.ptr, Y.ptr, batch, R, C, _stream())
        torch.cuda.synchronize()
        assert_equal_bits(Y.t.contiguous().cpu().view(batch, C, R), x.view(batch, R, C).transpose(1, 2).contiguous(), f"transpose {(batch, R, C)}", tile=(64, 64))
        Y.check("y"); X.check("x")


@pytest.mark.parametrize("C", [3, 4, 5])
@pytest.mark.parametrize("cpad", [8, 16])
def test_layout_conversions_write_zero_padding_and_nothing_else(dev, C, cpad):
    """sdt_nchw_f32_to_nhwc_bf16 / sdt_nhwc_bf16_to_nchw_f32: the padding channels are written as zero and nothing beyond them."""
    from stable_diffusion_training_amd import _lib
    B, H, W = 2, 5, 7
    x = exact_ints((B, C, H, W), -100, 100, C + cpad, dtype=torch.float32) * 0.5
    X, Y = Guarded(1, x.numel(), torch.float32, dev, data=x, pad=0), Guarded(1, B * H * W * cpad, BF, dev, pad=0)
    _lib.call("sdt_nchw_f32_to_nhwc_bf16", X.ptr, Y.ptr, B, C, H, W, cpad, _stream())
    torch.cuda.synchronize()
    want = torch.zeros(B, H, W, cpad, dtype=BF)
    want[..., :C] = x.permute(0, 2, 3, 1).to(BF)
    assert_equal_bits(Y.t.contiguous().cpu().view(B, H, W, cpad), want, "nhwc")
    Y.check("nhwc"); X.check("nchw")
    xin = want.clone()
    xin[..., C:] = float("nan")  # the padding channels of the input are not read
    Xn, Z = Guarded(1, xin.numel(), BF, dev, data=xin, pad=0), Guarded(1, B * C * H * W, torch.float32, dev, pad=0)
    _lib.call("sdt_nhwc_bf16_to_nchw_f32", Xn.ptr, Z.ptr, B, C, H, W, cpad, _stream())
    torch.cuda.synchronize()
    assert_equal_bits(Z.t.contiguous().cpu().view(B, C, H, W), want[..., :C].float().permute(0, 3, 1, 2).contiguous(), "nchw")
    Z.check("nchw"); Xn.check("nhwc")


@pytest.mark.parametrize("n", [1, 7, 500, 1025])
def test_softmax_rows_tail_sizes(dev, n):
    """sdt_softmax_rows_inplace on rows of n elements inside one guarded arena (rows are n apart: a tail store past a row would hit
    its neighbour, past the last row the guard).  One-hot rows (a 200-logit winner) are exact; Gaussian rows stay within one bf16
    ulp of the float64 softmax rounded to bf16 (fp32 evaluation: the result can only cross a rounding boundary)."""
    from stable_diffusion_training_amd import _lib
    rows = 5
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(rows, n, generator=g) * 3).to(BF)
    x[0] = 0
    x[0, n // 2] = 200.0
    X = Guarded(1, rows * n, BF, dev, data=x, pad=0)
    before = X.arena.clone()
    _lib.call("sdt_softmax_rows_inplace", X.ptr, rows, n, 0.5, _stream())
    torch.cuda.synchronize()
    got = X.t.view(rows, n).cpu()
    guard_changed = kc.bits(X.arena) != kc.bits(before)
    guard_changed[X.front: X.front + rows * n] = False
    assert not guard_changed.any(), f"softmax n = {n}: {int(guard_changed.sum())} elements outside the rows changed"
    want = torch.softmax(x.double() * 0.5, -1)
    one_hot = torch.zeros(n, dtype=BF)
    one_hot[n // 2] = 1
    assert_equal_bits(got[0] + 0.0, one_hot, "one-hot row")
    wb = want.float().to(BF).double()
    err = (got.double() - wb).abs()
    assert (err <= kc.bf16_ulp(wb)).all(), f"softmax n = {n}: worst {err.max().item():.3e} at {err.argmax().item()}"


def test_copies_and_fan_in_sum(dev):
    """sdt_copy2d_bf16 (pitches on both sides), sdt_copy_cols_bf16 (gather with a NULL part that zero-fills, and the scatter back),
    sdt_sum_n_bf16 with n = 1 and n = 32 (integers: the fp32 sum is exact)."""
    from stable_diffusion_training_amd import _lib
    rows = 37
    src = exact_ints((rows, 24), -100, 100, 1)
    S, D = Guarded(rows, 24, BF, dev, data=src), Guarded(rows, 24, BF, dev)
    _lib.call("sdt_copy2d_bf16", D.ptr, D.ld, S.ptr, S.ld, rows, 24, _stream())
    torch.cuda.synchronize()
    assert_equal_bits(D.t.contiguous().cpu(), src, "copy2d"); D.check("copy2d dst"); S.check("copy2d src")
    cols = [8, 16, 24]
    parts = [exact_ints((rows, c), -100, 100, 10 + c) for c in cols]
    P = [Guarded(rows, c, BF, dev, data=p) for c, p in zip(cols, parts)]
    Wd = Guarded(rows, sum(cols), BF, dev)
    ptrs = (ctypes.c_void_p * 3)(P[0].ptr, None, P[2].ptr)
    lds = (ctypes.c_int64 * 3)(*[p.ld for p in P])
    cs = (ctypes.c_int * 3)(*cols)
    _lib.call("sdt_copy_cols_bf16", Wd.ptr, Wd.ld, ptrs, lds, cs, 3, rows, 1, _stream())
    torch.cuda.synchronize()
    assert_equal_bits(Wd.t.contiguous().cpu(), torch.cat([parts[0], torch.zeros(rows, 16, dtype=BF), parts[2]], 1), "copy_cols gather"); Wd.check("wide")
    Q = [Guarded(rows, c, BF, dev) for c in cols]
    ptrs = (ctypes.c_void_p * 3)(*[q.ptr for q in Q])
    _lib.call("sdt_copy_cols_bf16", Wd.ptr, Wd.ld, ptrs, lds, cs, 3, rows, 0, _stream())
    torch.cuda.synchronize()
    for q, want in zip(Q, (parts[0], torch.zeros(rows, 16, dtype=BF), parts[2])):
        assert_equal_bits(q.t.contiguous().cpu(), want, "copy_cols scatter"); q.check("part")
    for n in (1, 32):
        numel = 8 * 131
        ins = [exact_ints((numel,), -100, 100, 50 + i) for i in range(n)]
        I = [Guarded(1, numel, BF, dev, data=t, pad=0) for t in ins]
        O = Guarded(1, numel, BF, dev, pad=0)
        ptrs = (ctypes.c_void_p * n)(*[g.ptr for g in I])
        _lib.call("sdt_sum_n_bf16", ptrs, n, O.ptr, numel, _stream())
        torch.cuda.synchronize()
        assert_equal_bits(O.t.view(-1).cpu(), kc.rne_bf16(torch.stack(ins).double().sum(0)), f"sum of {n}"); O.check("sum")


def test_zero_size_calls_return_ok_and_write_nothing(dev):
    """The entry points that accept M, n or rows == 0 (elementwise.hip) return SDT_OK and leave guarded outputs untouched."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    s = _stream()
    X = Guarded(1, 64, BF, dev, data=torch.ones(64))
    F32 = Guarded(1, 64, torch.float32, dev, data=torch.ones(64))
    O, O32 = Guarded(1, 64, BF, dev), Guarded(1, 64, torch.float32, dev)
    ws = _workspace(CNT, dev)
    one = (ctypes.c_void_p * 1)(X.ptr)
    ld1, c1 = (ctypes.c_int64 * 1)(8), (ctypes.c_int * 1)(8)
    calls = [("sdt_act_fwd", (X.ptr, O.ptr, 0, 0, s)), ("sdt_act_bwd", (X.ptr, X.ptr, O.ptr, 0, 0, s)), ("sdt_geglu_fwd", (X.ptr, O.ptr, 0, 8, s)),
             ("sdt_geglu_bwd", (X.ptr, X.ptr, O.ptr, 0, 8, s)), ("sdt_copy2d_bf16", (O.ptr, 8, X.ptr, 8, 0, 8, s)),
             ("sdt_copy_cols_bf16", (O.ptr, 8, one, ld1, c1, 1, 0, 1, s)), ("sdt_add_bf16", (X.ptr, X.ptr, O.ptr, 0, s)),
             ("sdt_cast_f32_to_bf16", (F32.ptr, O.ptr, 0, s)), ("sdt_sum_n_bf16", (one, 1, O.ptr, 0, s)),
             ("sdt_colsum_accumulate", (X.ptr, O32.ptr, 0, 8, 8, ws.data_ptr(), ws.numel(), s))]
    for name, args in calls:
        rc = getattr(lib, name)(*args)
        assert rc == 0, f"{name} with a zero size returned {rc}: {lib.sdt_last_error().decode()}"
    torch.cuda.synchronize()
    O.check("bf16 output of the zero-size calls"); O32.check("fp32 output of the zero-size calls")
    _counters_zero(ws)
