"""GroupNorm, LayerNorm and the CLIP pooling norm (csrc/norm.hip) bit for bit on a real MI355X, on balanced inputs whose true result is
exactly representable (generators, expectations, the mirror of the launch geometry and the case tables: tests/kernel_checks.py "norms
on balanced inputs"; their proof on the CPU: tests/test_kernel_checks_cpu.py).

Every (image, group) and every LayerNorm row holds only c - s and c + s, equally often, so mean c, variance s^2 and xhat = +-1 are
exact, y = +-gamma + beta is a small integer and dx = r / s a multiple of 1/2.  The kernels' fp32 arithmetic moves a value by about 1e-5
relative; a bf16-representable value is at least 2^-10 relative away from a rounding boundary, so y and dx must hold the bits of the
float64 result in both regimes:
  exact regime (GroupNorm counts that are powers of two, every LayerNorm shape; eps = 0): the fp32 outputs are exact as well - stats,
    the stored mean, dgamma and dbeta (onto non-zero previous values) bit for bit, the stored rstd within one fp32 ulp;
  ragged regime (any other count, eps = 1e-5): stats bit for bit (integer sums), dgamma / dbeta under the per-channel rule of
    test_gpu_kernel_exact._norm_slices (kernel_checks.param_grad_rule; figures printed for DESIGN.md).
Calls go through _lib.call on raw pointers; inputs sit between NaN guards, outputs and workspaces between sentinels (the workspace
payload is NaN patterns too: nothing is assumed zero), all checked after every call."""
import pytest
import torch

from tests import kernel_checks as kc
from tests.kernel_checks import BF, Guarded, assert_equal_bits
from tests.test_gpu_kernel_exact import _check_all, _ptr, _stream

pytestmark = pytest.mark.gpu
F32 = torch.float32
EPS = 1e-5


def _in(data, dtype, dev):
    """A contiguous operand (the norm ABI has no pitch) between NaN guards."""
    return Guarded(1, data.numel(), dtype, dev, data=data.reshape(1, -1), guard=float("nan") if dtype.is_floating_point else -1, pad=0, back_rows=0)


def _out(n, dtype, dev):
    return Guarded(1, n, dtype, dev, pad=0, back_rows=0)


def _io(data, dtype, dev):
    g = _out(data.numel(), dtype, dev)
    g.t.copy_(data.reshape(1, -1).to(dtype))
    return g


def _ws(nbytes, dev):
    """A workspace of exactly nbytes between sentinel guards, its payload NaN patterns."""
    return _out(max(int(nbytes) // 4, 1), F32, dev)


def _sync_check(guards):
    torch.cuda.synchronize()
    _check_all(guards)


def _eps(cnt):
    return 0.0 if kc.is_pow2(cnt) else EPS


def _within_one_ulp(got, want, what):
    d = (kc.bits(got.float().contiguous()).long() - kc.bits(want.float().contiguous()).long()).abs()
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} values more than one fp32 ulp off, worst {int(d.max())} ulps"
    return int(d.max())


_CASES = {}


def _gn(cid, dev):
    """The balanced case, its expectation and its input arenas, built once per case id and never modified."""
    if cid not in _CASES:
        case = kc.gn_balanced(cid)
        exp = kc.norm_exact_expectation(case, kc.gn_case(cid)[4], _eps(case["cnt"]))
        g = dict(x=_in(case["x"], BF, dev), dy=_in(case["dy"], BF, dev), dres=_in(case["dres"], BF, dev), gamma=_in(case["gamma"], F32, dev),
                 beta=_in(case["beta"], F32, dev), stats=_in(exp["stats"], F32, dev))
        _CASES[cid] = (case, exp, g)
    return _CASES[cid]


def _gn_fwd(g, B, HW, C, G, eps, silu, dev, parts=None, nparts=0, stats=None):
    """One sdt_groupnorm_fwd call into fresh output arenas; returns (y, stats) as tensors after the guards were checked."""
    from stable_diffusion_training_amd import _lib
    need = _lib.load().sdt_groupnorm_fwd_workspace_bytes(B, HW, C, G)
    assert need == kc.gn_fwd_workspace_bytes(B, HW, C, G)
    W = _ws(need, dev)
    Y = _out(B * HW * C, BF, dev)
    S = _out(B * G * 2, F32, dev) if stats is None else stats
    _lib.call("sdt_groupnorm_fwd", g["x"].ptr, g["gamma"].ptr, g["beta"].ptr, Y.ptr, S.ptr, B, HW, C, G, eps, silu,
              S.ptr if parts == "stats" else _ptr(parts), nparts, W.ptr, need, _stream())
    _sync_check(dict(y=Y, stats=S, workspace=W, parts=None if parts == "stats" else parts, **{k: g[k] for k in ("x", "gamma", "beta")}))
    return Y.t.view(B, HW, C), S.t.view(B, G, 2)


# ================================================================================================ GroupNorm forward, own statistics pass
@pytest.mark.parametrize("cid", [c[0] for c in kc.GN_BALANCED_CASES])
def test_groupnorm_fwd_own_statistics_every_bit(dev, cid):
    """silu = 0: stats == the exact {sum, sumsq} and y == the float64 result, in every bit.  silu = 1 on the same inputs: z is an exact
    integer, so y must meet the activation bound (kc.act_bound_violations) against float64 silu(z); stats as before."""
    _, B, HW, C, G = kc.gn_case(cid)
    case, exp, g = _gn(cid, dev)
    eps = _eps(case["cnt"])
    y, stats = _gn_fwd(g, B, HW, C, G, eps, 0, dev)
    msg = kc.stats_report(stats.cpu(), exp["stats"], f"{cid}: stats")
    assert msg is None, msg
    msg = kc.gn_mismatch_report(y.cpu(), exp["y"], f"{cid}: y", B, HW, C, G)
    assert msg is None, msg
    ys, stats = _gn_fwd(g, B, HW, C, G, eps, 1, dev)
    assert kc.stats_report(stats.cpu(), exp["stats"], f"{cid} silu: stats") is None
    z = exp["y"].double().reshape(-1)
    bad = kc.act_bound_violations(ys.cpu().reshape(-1), kc.act_ref64("silu", z)[0], z, torch.zeros_like(z))
    assert bad.numel() == 0, (f"{cid}: silu(y) misses the activation bound at {bad.numel()} elements, first: "
                              + kc.gn_locate(B, HW, C, G, int(bad[0]) // (HW * C), (int(bad[0]) // C) % HW, int(bad[0]) % C))


# ================================================================================================ GroupNorm forward, producer statistics
@pytest.mark.parametrize("cid,nparts", kc.GN_PARTS_CASES, ids=[f"{c}-{'gn_group_reduce_kernel' if n > 128 else 'inline'}_{n}_rows" for c, n in kc.GN_PARTS_CASES])
def test_groupnorm_fwd_producer_partial_rows(dev, cid, nparts):
    """parts = an integer decomposition of the true {sum, sumsq} into nparts rows (most non-zero, distinct): up to 128 rows are added in
    the apply prologue, more go through gn_group_reduce_kernel first (200 rows: a ragged rows_per and three empty workgroups).  stats
    must equal the column sums exactly - a failure names the row whose value is missing - and y the own-pass y, bit for bit."""
    _, B, HW, C, G = kc.gn_case(cid)
    case, exp, g = _gn(cid, dev)
    eps = _eps(case["cnt"])
    rows = kc.gn_parts_decomposition(exp["stats"], nparts, 31 * nparts + B)
    P = _in(rows, F32, dev)
    y, stats = _gn_fwd(g, B, HW, C, G, eps, 0, dev, parts=P, nparts=nparts)
    msg = kc.stats_report(stats.cpu(), exp["stats"], f"{cid} {nparts} rows: stats", parts=rows)
    assert msg is None, msg
    y_own, _ = _gn_fwd(g, B, HW, C, G, eps, 0, dev)
    for what, want in (("the float64 result", exp["y"]), ("the own-pass y", y_own.cpu())):
        msg = kc.gn_mismatch_report(y.cpu(), want, f"{cid} {nparts} rows: y against {what}", B, HW, C, G)
        assert msg is None, msg


@pytest.mark.parametrize("cid", ["pow2_cpg2", "cpg10_straddle_ty6", "g64_widest_c4096"])
def test_groupnorm_fwd_already_reduced_statistics(dev, cid):
    """parts == stats with nparts == 1: y as ever, and stats (an input arena here: every byte compared) left unchanged."""
    _, B, HW, C, G = kc.gn_case(cid)
    case, exp, g = _gn(cid, dev)
    y, _ = _gn_fwd(g, B, HW, C, G, _eps(case["cnt"]), 0, dev, parts="stats", nparts=1, stats=g["stats"])
    msg = kc.gn_mismatch_report(y.cpu(), exp["y"], f"{cid}: y from parts == stats", B, HW, C, G)
    assert msg is None, msg


# ================================================================================================ GroupNorm backward
def _param_grads(cid, form, exact, got, prev, exp, fails):
    for n in ("dgamma", "dbeta"):
        if exact:
            msg = kc.mismatch_report(got[n].cpu(), (prev[n].double() + exp[n]).float(), f"{cid} {form}: {n} (previous value + exact sum)")
        else:
            msg, wk, we = kc.param_grad_rule(got[n].cpu(), prev[n], exp["rule2"], n)
            print(f"NORM RULE2 {cid} {form} {n}: kernel worst channel {wk:.3e}, emulation worst channel {we:.3e}")
        if msg is not None:
            fails.append(msg)


@pytest.mark.parametrize("form", ["plain", "dres", "frozen"])
@pytest.mark.parametrize("cid", [c[0] for c in kc.GN_BALANCED_CASES], ids=[f"{c[0]}-B{c[1]}" for c in kc.GN_BALANCED_CASES])
def test_groupnorm_bwd_every_bit(dev, cid, form):
    """stats come from the reference, so the backward stands alone.  dx == r / s in every bit (with dres: bf16(bf16(dx) + dres), two
    roundings; every fourth dres makes the sum a tie); dgamma / dbeta == non-zero previous value + exact sum in every bit where the count
    is a power of two, under the per-channel rule (onto zero) elsewhere; frozen (dgamma = dbeta = NULL) writes dx and nothing else.  B > 1: partial_rows_reduce adds the
    rows of several images."""
    from stable_diffusion_training_amd import _lib
    _, B, HW, C, G = kc.gn_case(cid)
    case, exp, g = _gn(cid, dev)
    eps = _eps(case["cnt"])
    need = _lib.load().sdt_groupnorm_bwd_workspace_bytes(B, HW, C)
    assert need == kc.gn_bwd_workspace_bytes(B, HW, C)
    W = _ws(need, dev)
    DX = _out(B * HW * C, BF, dev)
    # previous values: non-zero where the sums are exact (this proves +=); zero under the per-channel rule, whose denominator knows
    # nothing of the rounding of (previous value + sum)
    prev = {n: case["prev_" + n] if eps == 0.0 else torch.zeros(C) for n in ("dgamma", "dbeta")}
    DG, DB = (None, None) if form == "frozen" else (_io(prev["dgamma"], F32, dev), _io(prev["dbeta"], F32, dev))
    _lib.call("sdt_groupnorm_bwd", g["x"].ptr, g["dy"].ptr, g["stats"].ptr, g["gamma"].ptr, g["beta"].ptr, DX.ptr, _ptr(DG), _ptr(DB),
              g["dres"].ptr if form == "dres" else None, B, HW, C, G, eps, 0, W.ptr, need, _stream())
    _sync_check(dict(dx=DX, dgamma=DG, dbeta=DB, workspace=W, **g))
    msg = kc.gn_mismatch_report(DX.t.view(B, HW, C).cpu(), exp["dx_dres" if form == "dres" else "dx"], f"{cid} {form}: dx", B, HW, C, G)
    fails = [] if msg is None else [msg]
    if form != "frozen":
        _param_grads(cid, form, eps == 0.0, dict(dgamma=DG.t.reshape(-1), dbeta=DB.t.reshape(-1)), prev, exp, fails)
    assert not fails, "\n".join(fails)


# ================================================================================================ LayerNorm
_LN = {}


def _ln(cid, dev):
    if cid not in _LN:
        case = kc.ln_balanced(cid)
        exp = kc.norm_exact_expectation(case, 0, 0.0)
        mr = torch.stack([exp["mean"], exp["rstd"]], -1)
        g = dict(x=_in(case["x"], BF, dev), dy=_in(case["dy"], BF, dev), dres=_in(case["dres"], BF, dev), gamma=_in(case["gamma"], F32, dev),
                 beta=_in(case["beta"], F32, dev), mean_rstd=_in(mr, F32, dev))
        _LN[cid] = (case, exp, g, mr)
    return _LN[cid]


@pytest.mark.parametrize("form", ["eps0_mean_rstd", "eps1e-5_mean_rstd_null"])
@pytest.mark.parametrize("cid", [c[0] for c in kc.LN_BALANCED_CASES])
def test_layernorm_fwd_every_bit(dev, cid, form):
    """y == the float64 result in every bit at eps = 0 and at eps = 1e-5; the stored mean is exact (an IEEE division of an exact
    multiple), the stored rstd = rsqrtf(1 or 4) within one fp32 ulp (what the hardware returns is printed); mean_rstd == NULL is
    accepted."""
    from stable_diffusion_training_amd import _lib
    _, M, C = kc.ln_case(cid)
    case, exp, g, mr = _ln(cid, dev)
    Y = _out(M * C, BF, dev)
    MR = _out(M * 2, F32, dev) if form == "eps0_mean_rstd" else None
    _lib.call("sdt_layernorm_fwd", g["x"].ptr, g["gamma"].ptr, g["beta"].ptr, Y.ptr, _ptr(MR), M, C, 0.0 if MR is not None else EPS, _stream())
    _sync_check(dict(y=Y, mean_rstd=MR, **{k: g[k] for k in ("x", "gamma", "beta")}))
    assert_equal_bits(Y.t.view(M, C).cpu(), exp["y"], f"{cid} {form}: y (row, channel)")
    if MR is not None:
        got = MR.t.view(M, 2).cpu()
        assert_equal_bits(got[:, 0].contiguous(), exp["mean"], f"{cid}: stored mean")
        worst = _within_one_ulp(got[:, 1], exp["rstd"], f"{cid}: stored rstd")
        seen = sorted({(s, r.hex()) for s, r in zip(case["s"].tolist(), got[:, 1].tolist())})
        print(f"RSQRTF {cid}: (s, rsqrtf(s^2)) observed {seen}, worst distance {worst} ulp")


@pytest.mark.parametrize("form", ["immediate", "deferred_param_grads", "dres", "frozen"])
@pytest.mark.parametrize("cid", [c[0] for c in kc.LN_BALANCED_CASES])
def test_layernorm_bwd_every_bit(dev, cid, form):
    """mean_rstd comes from the reference (rstd = 1 / s is exact), so xhat = +-1 in the kernel and everything is exact: dx == r / s (with
    dres: two roundings), dgamma / dbeta == previous value + exact sum, in every bit.  Deferred: sdt_layernorm_bwd leaves dgamma / dbeta
    alone and sdt_norm_param_grads_group adds the partial rows later; frozen writes dx only."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    _, M, C = kc.ln_case(cid)
    case, exp, g, mr = _ln(cid, dev)
    frozen, defer = form == "frozen", form == "deferred_param_grads"
    need = 0 if frozen else lib.sdt_layernorm_bwd_workspace_bytes(M, C)
    W = None if frozen else _ws(need, dev)
    DX = _out(M * C, BF, dev)
    prev = dict(dgamma=case["prev_dgamma"], dbeta=case["prev_dbeta"])
    DG, DB = (None, None) if frozen else (_io(prev["dgamma"], F32, dev), _io(prev["dbeta"], F32, dev))
    guards = dict(dx=DX, dgamma=DG, dbeta=DB, workspace=W, **g)
    _lib.call("sdt_layernorm_bwd", g["x"].ptr, g["dy"].ptr, g["gamma"].ptr, g["mean_rstd"].ptr, DX.ptr, _ptr(DG), _ptr(DB),
              g["dres"].ptr if form == "dres" else None, M, C, int(defer), _ptr(W), need, _stream())
    _sync_check(guards)
    fails = []
    msg = kc.mismatch_report(DX.t.view(M, C).cpu(), exp["dx_dres" if form == "dres" else "dx"], f"{cid} {form}: dx (row, channel)")
    if msg:
        fails.append(msg + "\n  " + kc.ln_geometry(M, C))
    if defer:
        for n, G_ in (("dgamma", DG), ("dbeta", DB)):
            msg = kc.mismatch_report(G_.t.reshape(-1).cpu(), prev[n], f"{cid}: {n} before the deferred sum (must be untouched)")
            if msg:
                fails.append(msg)
        job = (_lib.SdtNormGradJob * 1)(_lib.SdtNormGradJob(W.ptr, DG.ptr, DB.ptr, int(lib.sdt_layernorm_bwd_partial_rows(M, C)), C))
        _lib.call("sdt_norm_param_grads_group", job, 1, _stream())
        _sync_check(guards)
    if not frozen:
        _param_grads(cid, form, True, dict(dgamma=DG.t.reshape(-1), dbeta=DB.t.reshape(-1)), prev, exp, fails)
    assert not fails, "\n".join(fails)


# ================================================================================================ CLIP pooled output
@pytest.mark.parametrize("D,R,windows,S,eos_id", kc.CLIP_POOL_CASES, ids=[f"D{c[0]}_S{c[3]}_{'argmax' if c[4] < 0 else 'eos'}-zero_fill" for c in kc.CLIP_POOL_CASES])
def test_clip_pool_fwd_bwd_every_bit(dev, D, R, windows, S, eos_id):
    """Forward (eps = 0): pos, pooled and the stored mean in every bit, rstd within one fp32 ulp (the two-pass variance gives c and s^2
    exactly on these rows).  Backward from the reference's (mean, rstd, pos): dx holds r / s on the pooled position of the first window
    of every sample and ZERO BITS everywhere else of (R * windows, S, D) - S is no multiple of the 8-position slab -, dgamma / dbeta ==
    previous value + exact sum."""
    from stable_diffusion_training_amd import _lib
    cc = kc.clip_pool_case(D, R, windows, S, eos_id, 300 + D)
    rows = cc["rows"]
    exp = kc.norm_exact_expectation(rows, 0, 0.0)
    mr = torch.stack([exp["mean"], exp["rstd"]], -1)
    g = dict(ids=_in(cc["ids"], torch.int32, dev), x=_in(cc["x"], BF, dev), gamma=_in(rows["gamma"], F32, dev), beta=_in(rows["beta"], F32, dev),
             dpooled=_in(rows["dy"], BF, dev), mean_rstd=_in(mr, F32, dev), pos=_in(cc["pos"], torch.int32, dev))
    P, MR, POS = _out(R * D, BF, dev), _out(R * 2, F32, dev), _out(R, torch.int32, dev)
    _lib.call("sdt_clip_pool_fwd", g["ids"].ptr, g["x"].ptr, g["gamma"].ptr, g["beta"].ptr, P.ptr, MR.ptr, POS.ptr, R, windows, S, D, eos_id, 0.0, _stream())
    _sync_check(dict(pooled=P, mean_rstd_out=MR, pos_out=POS, **g))
    assert_equal_bits(POS.t.reshape(-1).cpu(), cc["pos"], f"D {D}: pos")
    assert_equal_bits(P.t.view(R, D).cpu(), exp["y"], f"D {D}: pooled (row, channel)")
    got = MR.t.view(R, 2).cpu()
    assert_equal_bits(got[:, 0].contiguous(), exp["mean"], f"D {D}: stored mean")
    worst = _within_one_ulp(got[:, 1], exp["rstd"], f"D {D}: stored rstd")
    seen = sorted({(s, r.hex()) for s, r in zip(rows["s"].tolist(), got[:, 1].tolist())})
    print(f"RSQRTF clip pool D {D}: (s, rsqrtf(s^2)) observed {seen}, worst distance {worst} ulp")

    DX = _out(R * windows * S * D, BF, dev)
    prev = dict(dgamma=rows["prev_dgamma"], dbeta=rows["prev_dbeta"])
    DG, DB = _io(prev["dgamma"], F32, dev), _io(prev["dbeta"], F32, dev)
    _lib.call("sdt_clip_pool_bwd", g["x"].ptr, g["dpooled"].ptr, g["gamma"].ptr, g["mean_rstd"].ptr, g["pos"].ptr, DX.ptr, DG.ptr, DB.ptr, R, windows, S, D, _stream())
    _sync_check(dict(dx=DX, dgamma=DG, dbeta=DB, **g))
    want = torch.zeros(R * windows, S, D, dtype=BF)
    for r in range(R):
        want[r * windows, int(cc["pos"][r])] = exp["dx"][r]
    assert_equal_bits(DX.t.view(R * windows, S, D).cpu(), want, f"D {D}: dx (row, position, channel)")
    fails = []
    _param_grads(f"clip pool D {D}", "bwd", True, dict(dgamma=DG.t.reshape(-1), dbeta=DB.t.reshape(-1)), prev, exp, fails)
    assert not fails, "\n".join(fails)
