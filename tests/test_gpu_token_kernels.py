"""The three new-token kernels (include/sdt.h "NEW TOKENS") on the MI355X against the numpy references of tests/token_reference.py:
bit for bit where the definition is exact, inside a written-down bound for the double reductions of the retraction.  Every operand
lives in a guarded arena (kernel_checks.Guarded), every case runs twice and the two runs must agree in every bit."""
import numpy as np
import pytest
import torch

from tests import kernel_checks as kc
from tests import token_reference as tr

pytestmark = pytest.mark.gpu
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
ROWS = tr.NSEQ * tr.S


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tables(D, n_ext, seed, dev):
    g = torch.Generator().manual_seed(seed)
    tok, ext, pos = (torch.randn(r, D, generator=g) for r in (tr.V, n_ext, tr.S))
    return tok, ext, pos, [kc.Guarded(t.shape[0], D, F32, dev, data=t, pad=0) for t in (tok, ext, pos)]


def _ids(ids, dev):
    return kc.Guarded(ROWS, 1, I32, dev, data=torch.from_numpy(ids).view(ROWS, 1), guard=-7, pad=0)


@pytest.mark.parametrize("n_ext", tr.N_EXT)
@pytest.mark.parametrize("D", tr.SHAPES)
def test_forward_bits(dev, lib, D, n_ext):
    from stable_diffusion_training_amd import _lib
    tok, ext, pos, (gt, ge, gp) = _tables(D, n_ext, 10 * D + n_ext, dev)
    for name, ids in tr.id_patterns(n_ext, D).items():
        gi = _ids(ids, dev)
        want = tr.forward_ref(ids, tok.numpy(), ext.numpy(), pos.numpy())
        runs = []
        for _ in range(2):
            out = kc.Guarded(ROWS, D, BF, dev, pad=0)
            _lib.call("sdt_embedding_ext_fwd", gi.ptr, gt.ptr, ge.ptr, gp.ptr, out.ptr, ROWS, tr.S, D, tr.V, n_ext, _stream())
            torch.cuda.synchronize()
            out.check(f"{name}: out")
            runs.append(out.t.cpu().clone())
        for g_, what in ((gi, "ids"), (gt, "tok"), (ge, "ext"), (gp, "pos")):
            g_.check(f"{name}: {what}")
        kc.assert_equal_bits(runs[0], want, f"forward D={D} n_ext={n_ext} {name}")
        assert torch.equal(kc.bits(runs[0]), kc.bits(runs[1])), f"{name}: two runs differ"
        if name == "bad_ids":  # ids -1, V + n_ext and 2^30 read no table: the position row alone
            for r in tr.BAD_ROWS:
                assert torch.equal(kc.bits(runs[0][r]), kc.bits(pos[r % tr.S].to(BF))), (name, r)
        if name == "no_new":  # the same buffers through the plain kernel
            plain = kc.Guarded(ROWS, D, BF, dev, pad=0)
            _lib.call("sdt_embedding_fwd", gi.ptr, gt.ptr, gp.ptr, plain.ptr, ROWS, tr.S, D, _stream())
            torch.cuda.synchronize()
            assert torch.equal(kc.bits(plain.t.cpu()), kc.bits(runs[0])), "ids below V: not the bits of sdt_embedding_fwd"


def test_forward_unaligned_bases_take_the_scalar_path_with_the_same_bits(dev, lib):
    """D % 4 == 0 but the tables start 4 bytes off a 16-byte boundary: the column-per-lane path must give the vector path's bits."""
    from stable_diffusion_training_amd import _lib
    D, n_ext = 12, 5
    tok, ext, pos, _ = _tables(D, n_ext, 3, dev)
    ids = tr.id_patterns(n_ext, 3)["mixed"]
    want = tr.forward_ref(ids, tok.numpy(), ext.numpy(), pos.numpy())
    di = torch.from_numpy(ids).to(dev)
    bufs = [torch.zeros(t.numel() + 1, device=dev) for t in (tok, ext, pos)]
    for b, t in zip(bufs, (tok, ext, pos)):
        b[1:].copy_(t.reshape(-1))
    out = torch.empty(ROWS, D, dtype=BF, device=dev)
    _lib.call("sdt_embedding_ext_fwd", di.data_ptr(), *(b.data_ptr() + 4 for b in bufs), out.data_ptr(), ROWS, tr.S, D, tr.V, n_ext, _stream())
    torch.cuda.synchronize()
    kc.assert_equal_bits(out.cpu(), want, "forward, unaligned tables")


@pytest.mark.parametrize("n_ext", tr.N_EXT)
@pytest.mark.parametrize("D", tr.SHAPES)
def test_backward_exact(dev, lib, D, n_ext):
    """Integer gradients in [-3, 3]: every partial sum is an integer below 21 * 3, exact in float32, so the expectation is unique."""
    from stable_diffusion_training_amd import _lib
    dout = kc.exact_ints((ROWS, D), -3, 3, 100 + D + n_ext)
    gd = kc.Guarded(ROWS, D, BF, dev, data=dout, pad=0)
    for name, ids in tr.id_patterns(n_ext, D).items():
        gi = _ids(ids, dev)
        want = torch.from_numpy(tr.backward_ref(ids, dout.float().numpy(), tr.V, n_ext))
        runs = []
        for _ in range(2):
            dext = kc.Guarded(n_ext, D, F32, dev, pad=0)  # poisoned: the kernel must write every element, absent tokens as +0.0
            _lib.call("sdt_embedding_ext_bwd", gi.ptr, gd.ptr, dext.ptr, ROWS, D, tr.V, n_ext, _stream())
            torch.cuda.synchronize()
            dext.check(f"{name}: dext")
            runs.append(dext.t.cpu().clone())
        gi.check(f"{name}: ids")
        gd.check(f"{name}: dout")
        kc.assert_equal_bits(runs[0], want, f"backward D={D} n_ext={n_ext} {name}")
        assert torch.equal(kc.bits(runs[0]), kc.bits(runs[1])), f"{name}: two runs differ"
        present = {int(i) - tr.V for i in ids if tr.V <= int(i) < tr.V + n_ext}
        for j in range(n_ext):
            if j not in present:
                assert not bool(kc.bits(runs[0][j]).any()), f"{name}: absent token {j} is not +0.0"
        if name == "no_new":
            assert not present


def test_backward_adds_in_row_order(dev, lib):
    """One column whose rows hold 2^24, 1, 1, -2^24 (all exact in bf16): in row order both ones are absorbed and the sum is 0; any
    order that adds the ones first, or pairs the large values first, gives 2."""
    from stable_diffusion_training_amd import _lib
    D, n_ext = 5, 1
    ids = np.full(ROWS, 3, np.int32)
    rows = [2, 6, 11, 19]
    ids[rows] = tr.V
    dout = torch.zeros(ROWS, D)
    dout[rows, 2] = torch.tensor([2.0 ** 24, 1.0, 1.0, -2.0 ** 24])
    dout[:, 4] = 1.0  # (a column every order agrees on)
    assert torch.equal(dout.to(BF).float(), dout)
    want = tr.backward_ref(ids, dout.numpy(), tr.V, n_ext)
    assert want[0, 2] == 0.0 and want[0, 4] == 4.0
    gi, gd = _ids(ids, dev), kc.Guarded(ROWS, D, BF, dev, data=dout, pad=0)
    dext = kc.Guarded(n_ext, D, F32, dev, pad=0)
    _lib.call("sdt_embedding_ext_bwd", gi.ptr, gd.ptr, dext.ptr, ROWS, D, tr.V, n_ext, _stream())
    torch.cuda.synchronize()
    dext.check("dext")
    kc.assert_equal_bits(dext.t.cpu(), torch.from_numpy(want), "backward, row order")


def _ulp32(x):
    x = np.float32(abs(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


_POW_DIFF = {"ulps": 0.0, "rel": 0.0}


@pytest.mark.parametrize("power", [0.1, 1.0])
@pytest.mark.parametrize("shape", tr.RETRACT_SHAPES)
def test_retract(dev, lib, shape, power):
    from stable_diffusion_training_amd import _lib
    n_ext, D = shape
    n = n_ext * D
    target = 0.0137
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n_ext, D, generator=g) * 0.05 + 0.01
    runs = []
    for _ in range(2):
        ext = kc.Guarded(n_ext, D, F32, dev, data=x, pad=0)
        stats = kc.Guarded(1, 3, F64, dev, pad=0)
        _lib.call("sdt_embedding_retract", ext.ptr, n_ext, D, target, power, stats.ptr, _stream())
        torch.cuda.synchronize()
        stats.check("stats")
        bad = kc.bits(ext.arena) != kc.bits(ext.before)  # an in-place operand: only the payload may change
        bad[ext.front: ext.front + n] = False
        assert not bool(bad.any()), "retract wrote outside the table"
        runs.append((ext.t.cpu().clone(), stats.t.cpu().clone().reshape(3)))
    got, st = runs[0]
    assert torch.equal(kc.bits(got), kc.bits(runs[1][0])) and torch.equal(kc.bits(st), kc.bits(runs[1][1])), "two runs differ"
    mean, std, factor = (float(v) for v in st)
    rmean, rstd = tr.retract_stats(x.numpy())
    x64 = x.numpy().astype(np.float64).reshape(-1)
    u = 2.0 ** -53
    # mean: an ordered double sum of n terms is within (n - 1) u sum|x| of the exact sum in ANY order (tr.sum_bound doubles it for the
    # second-order terms and numpy's own sum); the division by n adds one rounding, u |mean|.
    b_mean = tr.sum_bound(x64) / n + 2 * u * abs(rmean)
    print(f"[retract {shape} p={power}] mean {mean!r} vs {rmean!r} (|diff| {abs(mean - rmean):.3e}, bound {b_mean:.3e})")
    assert abs(mean - rmean) <= b_mean
    # std = sqrt(ss / (n - 1)), ss = sum (x - m)^2 with the COMPUTED mean m: sum (x - m)^2 = sum (x - mean)^2 + n (m - mean)^2 exactly,
    # every term carries two roundings (the subtraction, doubled by the square, and the square: <= 3 u relative; a fused multiply-add
    # only removes one), the ordered sum of n non-negative terms (n - 1) u relative, the division and the root one rounding each and
    # the root halves what comes before it: |std - exact| <= std * ((n + 2) u / 2 + 2 u) + the mean's term; doubled as above.
    b_std = 2 * rstd * ((n + 2) * u / 2 + 2 * u) + (n * b_mean ** 2) / (2 * max(rstd, 1e-300) * max(n - 1, 1)) + 5e-324
    print(f"[retract {shape} p={power}] std {std!r} vs {rstd!r} (|diff| {abs(std - rstd):.3e}, bound {b_std:.3e})")
    assert abs(std - rstd) <= b_std
    # factor: judged from the PUBLISHED std, so that only the device pow and its rounding to float32 are in question
    want_f = tr.retract_factor(std, target, power)
    exact = (np.float64(target) / np.float64(std)) ** np.float64(power)
    d_ulps = abs(factor - float(want_f)) / _ulp32(want_f)
    _POW_DIFF["ulps"] = max(_POW_DIFF["ulps"], d_ulps)
    _POW_DIFF["rel"] = max(_POW_DIFF["rel"], abs(factor - exact) / exact)
    print(f"[retract {shape} p={power}] factor {factor!r} vs float32(float64 pow) {float(want_f)!r}: {d_ulps:.1f} fp32 ulp; "
          f"largest so far {_POW_DIFF['ulps']:.1f} ulp, |factor - pow64| / pow64 {_POW_DIFF['rel']:.3e}")
    assert np.float32(factor) == factor and d_ulps <= 1.0
    kc.assert_equal_bits(got, torch.from_numpy(tr.retract_apply(x.numpy(), factor)), f"retract {shape}: rows")


def test_retract_of_a_constant_table_changes_nothing(dev, lib):
    from stable_diffusion_training_amd import _lib
    for n_ext, D in tr.RETRACT_SHAPES:
        x = torch.full((n_ext, D), 0.1)
        ext = kc.Guarded(n_ext, D, F32, dev, data=x, pad=0)
        stats = kc.Guarded(1, 3, F64, dev, pad=0)
        _lib.call("sdt_embedding_retract", ext.ptr, n_ext, D, 0.02, 0.1, stats.ptr, _stream())
        torch.cuda.synchronize()
        ext.check("a constant table: std == 0, factor 1, every bit kept")
        mean, std, factor = stats.t.cpu().reshape(3).tolist()
        assert (mean, std, factor) == (float(np.float32(0.1)), 0.0, 1.0)
