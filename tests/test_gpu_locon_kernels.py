"""sdt_lora_project_split on the MI355X, element by element (include/sdt.h "LoCon"), and sdt_lora_merge / sdt_lora_restore at the
tall-K shapes of convolution kernels.

Exact cases (tests/locon_reference.cases around the chunk length C = sdt_lora_project_split_rows()): integers in -3..3, every sum exact
in fp32 in any order (tests/test_locon_cpu.py proves the bound per case), so dA and dB must equal the float64 reference bit for bit, the
merged mirror its RNE bf16 rounding and the restored mirror RNE bf16 of W0.  Every launch runs on poisoned gradient buffers and a
workspace whose partial area and margins are poisoned: nothing outside the named leaves and nothing outside the workspace's declared bytes
may be written, and the arrival counters must be zero again."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import locon_reference as lc
from tests import lora_reference as lr
from tests.test_gpu_lora_kernels import POISON16, POISON32, _Buffers, _stream

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MARGIN = 256  # poisoned bytes in front of and behind the workspace


class _Split:
    """The split table and the workspace of one launch over b.jobs."""

    def __init__(self, b, C):
        self.b = b
        self.table, self.counter_bytes, self.bytes = lc.split_table(b.jobs, C)
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(b.dev)
        self.buf = torch.full((self.bytes + 2 * MARGIN,), 0xA5, dtype=torch.uint8, device=b.dev)
        self.buf[MARGIN: MARGIN + self.counter_bytes] = 0  # the counters: zero on entry (zeroed once, never again)

    def project(self, lib, n=None):
        b = self.b
        n = len(b.jobs) if n is None else n
        assert lib.sdt_lora_project_split_workspace_bytes(b.table, len(b.jobs)) == self.bytes
        rc = lib.sdt_lora_project_split(b.dw.data_ptr(), b.ab.data_ptr(), b.grad.data_ptr(), b.table, self.table, b.table_dev.data_ptr(),
                                        self.table_dev.data_ptr(), n, self.buf.data_ptr() + MARGIN, self.bytes, _stream())
        assert rc == 0, lib.sdt_last_error().decode()

    def check(self):
        """Margins untouched, counters back at zero."""
        host = self.buf.cpu()
        assert bool((host[:MARGIN] == 0xA5).all()) and bool((host[MARGIN + self.bytes:] == 0xA5).all()), "written outside the workspace's declared bytes"
        assert not bool(host[MARGIN: MARGIN + self.counter_bytes].any()), "an arrival counter was left non-zero"


def _gspans(jobs):
    out = []
    for j in jobs:
        out += [(j["a_off"], j["a_off"] + j["K"] * j["r"]), (j["b_off"], j["b_off"] + j["r"] * j["N"])]
    return out


def _check_exact(lib, dev, cases, order, seed):
    C = lc.rows()
    jobs, sizes = lr.layout(cases, order)
    operands = [lr.exact_operands(K, N, r, seed + 10 * i) for i, (K, N, r, s) in enumerate(cases)]
    b = _Buffers(jobs, sizes, operands, dev)
    sp = _Split(b, C)
    b.merge(lib)
    sp.project(lib)
    torch.cuda.synchronize()
    wspans = []
    for j in jobs:
        W0, A, B, dW = operands[j["index"]]
        K, N, r, s = j["K"], j["N"], j["r"], j["s"]
        what = f"K={K} N={N} r={r} s={s}"
        v = lr.merge_ref64(W0, A, B, s)
        o = j["w0_off"]
        wspans.append((o, o + K * N))
        kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(v), f"merged mirror {what}", tile=(64, 64))
        kc.assert_equal_bits(b.f[o: o + K * N].view(K, N).cpu(), v.float(), f"merged fp32 {what}", tile=(64, 64))
        dA, dB = lr.project_ref64(dW, A, B, s)
        assert torch.equal(dA.float().double(), dA) and torch.equal(dB.float().double(), dB)
        kc.assert_equal_bits(b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu(), dA.float(), f"dA {what}", tile=(64, 16))
        kc.assert_equal_bits(b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu(), dB.float(), f"dB {what}", tile=(16, 64))
    b.untouched(b.w, wspans, POISON16, "bf16 mirror")
    b.untouched(b.f, wspans, POISON32, "fp32 destination")
    b.untouched(b.grad, _gspans(jobs), POISON32, "gradient buffer")
    sp.check()
    # restore: RNE bf16 of W0 in every named leaf, nothing else
    b.poison()
    rc = lib.sdt_lora_restore(b.master.data_ptr(), b.w.data_ptr(), b.table, b.table_dev.data_ptr(), len(jobs), _stream())
    assert rc == 0, lib.sdt_last_error().decode()
    torch.cuda.synchronize()
    for j in jobs:
        W0 = operands[j["index"]][0]
        o, K, N = j["w0_off"], j["K"], j["N"]
        kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(W0.double()), f"restored mirror K={K} N={N}", tile=(64, 64))
    b.untouched(b.w, wspans, POISON16, "bf16 mirror after restore")


@pytest.mark.parametrize("i", range(7))
def test_exact_single(lib, dev, i):
    K, N, r = lc.cases(lc.rows())[i]
    _check_exact(lib, dev, [(K, N, r, lc.SCALES[i % 3])], None, 100 + i)


def _shuffled(n, seed=5):
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    assert order != sorted(order)
    return order


def test_exact_grouped_shuffled(lib, dev):
    """One launch holding every case, the jobs in shuffled order: the lookup by running tile counts, the counters and partial offsets of
    neighbouring jobs, one-chunk and many-chunk jobs side by side."""
    cases = [(K, N, r, lc.SCALES[(i + 1) % 3]) for i, (K, N, r) in enumerate(lc.cases(lc.rows()))]
    _check_exact(lib, dev, cases, _shuffled(len(cases)), 300)


def _random_operands(K, N, r, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, N, generator=g) * 0.05, torch.randn(K, r, generator=g) * 0.1, torch.randn(r, N, generator=g) * 0.1,
            (torch.randn(K, N, generator=g) * 0.01).to(BF))


def _grads(b, j):
    K, N, r = j["K"], j["N"], j["r"]
    return (b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu().clone(), b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu().clone())


@pytest.mark.parametrize("i", range(2))
def test_random_values_order_reproducibility_and_derived_bound(lib, dev, i):
    """The same dA / dB bits for the job alone, inside the shuffled table of all cases, and on a second call with the same workspace and
    no reset in between (the counters reset themselves; the partials are overwritten).  Accuracy, derived: one dB element is a sum of
    exact bf16 x bf16 products accumulated in fp32 - at most C - 1 additions inside a chunk (the first product enters a zero accumulator
    exactly), chunks - 1 additions of the chunk sums in chunk order, and one scaling: n = (C - 1) + (chunks - 1) + 1 roundings
    (tests/locon_reference.db_roundings), so |dB - ref64| <= gamma_n * s * sum_k |bf16(A)| |dW|; dA is sdt_lora_project's:
    |dA - ref64| <= gamma_N * s * sum_n |dW| |bf16(B)|."""
    C = lc.rows()
    K, N, r = lc.random_cases(C)[i]
    s = 0.75
    ops_ = _random_operands(K, N, r, K + N + r)
    W0, A, B, dW = ops_
    jobs, sizes = lr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [ops_], dev)
    sp = _Split(b, C)
    sp.project(lib)
    torch.cuda.synchronize()
    alone = _grads(b, jobs[0])
    b.poison()
    sp.project(lib)  # the same workspace, not reset
    torch.cuda.synchronize()
    again = _grads(b, jobs[0])
    sp.check()
    # inside the shuffled table of every exact case
    others = [(k, n, q, 1.0) for k, n, q in lc.cases(C)]
    cases = others[:3] + [(K, N, r, s)] + others[3:]
    operands = [lr.exact_operands(k, n, q, 700 + t) for t, (k, n, q, _) in enumerate(cases)]
    operands[3] = ops_
    tj, tsizes = lr.layout(cases, _shuffled(len(cases), seed=6))
    tb = _Buffers(tj, tsizes, operands, dev)
    tsp = _Split(tb, C)
    tsp.project(lib)
    torch.cuda.synchronize()
    inside = _grads(tb, [j for j in tj if j["index"] == 3][0])
    tsp.check()
    for name, got in (("second call", again), ("shuffled table", inside)):
        assert torch.equal(kc.bits(got[0]), kc.bits(alone[0])), f"dA differs: {name}"
        assert torch.equal(kc.bits(got[1]), kc.bits(alone[1])), f"dB differs: {name}"
    dA, dB = lr.project_ref64(dW, A, B, s)
    boundA = lr.gamma(N) * s * (dW.double().abs() @ lr.bf(B).abs().T)
    boundB = lr.gamma(lc.db_roundings(K, C)) * s * (lr.bf(A).abs().T @ dW.double().abs())
    errA, errB = (alone[0].double() - dA).abs(), (alone[1].double() - dB).abs()
    print(f"K={K} N={N} r={r}: dA worst err/bound {(errA / boundA).max():.3f}  dB {(errB / boundB).max():.3f}")
    assert bool((errA <= boundA).all()) and bool((errB <= boundB).all())


def test_one_chunk_job_has_the_bits_of_sdt_lora_project(lib, dev):
    C = lc.rows()
    K, N, r, s = C - 8, 72, 4, 0.75
    ops_ = _random_operands(K, N, r, 77)
    jobs, sizes = lr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [ops_], dev)
    sp = _Split(b, C)
    assert sp.table[0].chunks == 1 and sp.bytes == sp.counter_bytes
    sp.project(lib)
    torch.cuda.synchronize()
    split = _grads(b, jobs[0])
    b.untouched(b.grad, _gspans(jobs), POISON32, "gradient buffer")
    b.poison()
    b.project(lib)
    torch.cuda.synchronize()
    plain = _grads(b, jobs[0])
    assert torch.equal(kc.bits(split[0]), kc.bits(plain[0])) and torch.equal(kc.bits(split[1]), kc.bits(plain[1]))
    sp.check()


def test_empty_launch(lib, dev):
    jobs, sizes = lr.layout([(72, 8, 4, 1.0)])
    b = _Buffers(jobs, sizes, [lr.exact_operands(72, 8, 4, 1)], dev)
    sp = _Split(b, lc.rows())
    sp.project(lib, n=0)
    assert lib.sdt_lora_project_split(None, None, None, None, None, None, None, 0, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    b.untouched(b.grad, [], POISON32, "gradient buffer after n == 0")
    sp.check()
