"""sdt_loha_merge / sdt_loha_project on the MI355X, element by element (include/sdt.h "LoHa").

Exact cases (tests/loha_reference.cases around the chunk length C = sdt_lora_project_split_rows()): factors in {-1, 0, 1}, dW in {0, +-1, +-2,
+-4}, W0 a multiple of 1/8 - every P, P1 * P2, G (in bf16) and partial sum is exact (tests/test_loha_cpu.py proves it per case), so the
four factor gradients and the fp32 destination must equal the float64 reference bit for bit, the merged mirror its RNE bf16 rounding and the
restored mirror RNE bf16 of W0.  Every launch runs on poisoned gradient buffers, a poisoned mirror and fp32 destination and a workspace whose
partial area and margins are poisoned: nothing outside the named leaves and nothing outside the workspace's declared bytes may be written,
and the arrival counters must be zero again.  Random values: the bound derived in DESIGN.md "LoHa" (tests/loha_reference.projection_bounds); measured
worst error / bound for dA1, dB1, dA2, dB2: 136 x 72 r32 0.353, 0.273, 0.333, 0.233; 320 x 320 r16 0.179, 0.174, 0.157, 0.168; 1064 x 192 r8
0.227, 0.091, 0.268, 0.091."""
import pytest
import torch

from tests import kernel_checks as kc
from tests import locon_reference as lc
from tests import loha_reference as lh
from tests import lora_reference as lr
from tests.test_gpu_lora_kernels import POISON16, POISON32, _Buffers, _stream

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MARGIN = 256  # poisoned bytes in front of and behind the workspace
NAMES = ("dA1", "dB1", "dA2", "dB2")


class _Loha:
    """The buffers (tests/test_gpu_lora_kernels._Buffers for W0, side 1 and dW; side 2 written into the same `ab` buffer), the split and LoHa
    tables and the workspace of one launch.  operands: (W0, A1, B1, A2, B2, dW) per case."""

    def __init__(self, jobs, sizes, operands, dev, C):
        self.jobs = jobs
        b = self.b = _Buffers(jobs, sizes, [(o[0], o[1], o[2], o[5]) for o in operands], dev)
        for j in jobs:
            A2, B2 = operands[j["index"]][3:5]
            K, N, r = j["K"], j["N"], j["r"]
            b.ab[j["a2_off"]: j["a2_off"] + K * r] = A2.reshape(-1).to(dev)
            b.ab[j["b2_off"]: j["b2_off"] + r * N] = B2.reshape(-1).to(dev)
        self.split, _, _ = lc.split_table(jobs, C)
        self.table, self.counter_bytes, self.bytes = lh.loha_table(jobs, C)
        up = lambda t: torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
        self.split_dev, self.table_dev = up(self.split), up(self.table)
        self.buf = torch.full((self.bytes + 2 * MARGIN,), 0xA5, dtype=torch.uint8, device=dev)
        self.buf[MARGIN: MARGIN + self.counter_bytes] = 0  # the counters: zero on entry (zeroed once, never again)

    def merge(self, lib, w=True, f=True, n=None):
        b = self.b
        n = len(self.jobs) if n is None else n
        rc = lib.sdt_loha_merge(b.master.data_ptr(), b.ab.data_ptr(), b.w.data_ptr() if w else None, b.f.data_ptr() if f else None, b.table,
                                self.table, b.table_dev.data_ptr(), self.table_dev.data_ptr(), n, _stream())
        assert rc == 0, lib.sdt_last_error().decode()

    def project(self, lib, n=None):
        b = self.b
        n = len(self.jobs) if n is None else n
        assert lib.sdt_loha_project_workspace_bytes(b.table, len(self.jobs)) == self.bytes
        rc = lib.sdt_loha_project(b.dw.data_ptr(), b.ab.data_ptr(), b.grad.data_ptr(), b.table, self.split, self.table, b.table_dev.data_ptr(),
                                  self.split_dev.data_ptr(), self.table_dev.data_ptr(), n, self.buf.data_ptr() + MARGIN, self.bytes, _stream())
        assert rc == 0, lib.sdt_last_error().decode()

    def check_workspace(self):
        """Margins untouched, counters back at zero."""
        host = self.buf.cpu()
        assert bool((host[:MARGIN] == 0xA5).all()) and bool((host[MARGIN + self.bytes:] == 0xA5).all()), "written outside the workspace's declared bytes"
        assert not bool(host[MARGIN: MARGIN + self.counter_bytes].any()), "an arrival counter was left non-zero"

    def grads(self, j):
        K, N, r, g = j["K"], j["N"], j["r"], self.b.grad
        return tuple(g[o: o + n].view(shape).cpu().clone() for o, n, shape in (
            (j["a_off"], K * r, (K, r)), (j["b_off"], r * N, (r, N)), (j["a2_off"], K * r, (K, r)), (j["b2_off"], r * N, (r, N))))


def _gspans(jobs):
    out = []
    for j in jobs:
        K, N, r = j["K"], j["N"], j["r"]
        out += [(j["a_off"], j["a_off"] + K * r), (j["b_off"], j["b_off"] + r * N), (j["a2_off"], j["a2_off"] + K * r), (j["b2_off"], j["b2_off"] + r * N)]
    return out


def _check_exact(lib, dev, cases, order, seed):
    C = lh.rows()
    jobs, sizes = lh.layout(cases, order)
    operands = [lh.exact_operands(K, N, r, seed + 10 * i) for i, (K, N, r, s) in enumerate(cases)]
    x = _Loha(jobs, sizes, operands, dev, C)
    b = x.b
    x.merge(lib)
    x.project(lib)
    torch.cuda.synchronize()
    wspans = []
    for j in jobs:
        W0, A1, B1, A2, B2, dW = operands[j["index"]]
        K, N, r, s = j["K"], j["N"], j["r"], j["s"]
        what = f"K={K} N={N} r={r} s={s}"
        v = lh.merge_ref64(W0, A1, B1, A2, B2, s)
        assert torch.equal(v.float().double(), v)
        o = j["w0_off"]
        wspans.append((o, o + K * N))
        kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(v), f"merged mirror {what}", tile=(64, 64))
        kc.assert_equal_bits(b.f[o: o + K * N].view(K, N).cpu(), v.float(), f"merged fp32 {what}", tile=(64, 64))
        want = lh.project_ref64(dW, A1, B1, A2, B2, s)
        for name, got, ref in zip(NAMES, x.grads(j), want):
            assert torch.equal(ref.float().double(), ref)
            kc.assert_equal_bits(got, ref.float(), f"{name} {what}", tile=(64, 16) if name[1] == "A" else (16, 64))
    b.untouched(b.w, wspans, POISON16, "bf16 mirror")
    b.untouched(b.f, wspans, POISON32, "fp32 destination")
    b.untouched(b.grad, _gspans(jobs), POISON32, "gradient buffer")
    x.check_workspace()
    # restore on the same table: RNE bf16 of W0 in every named leaf, nothing else
    b.poison()
    rc = lib.sdt_lora_restore(b.master.data_ptr(), b.w.data_ptr(), b.table, b.table_dev.data_ptr(), len(jobs), _stream())
    assert rc == 0, lib.sdt_last_error().decode()
    torch.cuda.synchronize()
    for j in jobs:
        W0 = operands[j["index"]][0]
        o, K, N = j["w0_off"], j["K"], j["N"]
        kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(W0.double()), f"restored mirror K={K} N={N}", tile=(64, 64))
    b.untouched(b.w, wspans, POISON16, "bf16 mirror after restore")


@pytest.mark.parametrize("i", range(6))
def test_exact_single(lib, dev, i):
    K, N, r = lh.cases(lh.rows())[i]
    _check_exact(lib, dev, [(K, N, r, lh.SCALES[i % 3])], None, 100 + i)


def _shuffled(n, seed=5):
    order = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    assert order != sorted(order)
    return order


def test_exact_grouped_shuffled(lib, dev):
    """One launch holding every case, the jobs in shuffled order: the lookup by running tile counts, the counters and two-set partial
    offsets of neighbouring jobs, one-chunk and many-chunk jobs side by side."""
    cases = [(K, N, r, lh.SCALES[(i + 1) % 3]) for i, (K, N, r) in enumerate(lh.cases(lh.rows()))]
    _check_exact(lib, dev, cases, _shuffled(len(cases)), 300)


def _random_operands(K, N, r, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    return (rn(K, N) * 0.05, rn(K, r), rn(r, N) * 0.1, rn(K, r), rn(r, N) * 0.1, (rn(K, N) * 0.01).to(BF))


@pytest.mark.parametrize("i", range(3))
def test_random_values_order_reproducibility_and_derived_bound(lib, dev, i):
    """The same bits for the job alone, inside the shuffled table of all exact cases, and on a second call with the same workspace and no
    reset in between.  Accuracy: tests/loha_reference.projection_bounds - the bf16 rounding of G (2^-8), the r-term fp32 accumulation of P,
    the chunk accumulation, the chunks - 1 partial additions and the scaling - derived, not measured; the merge under merge_bound."""
    C = lh.rows()
    K, N, r = lh.random_cases(C)[i]
    s = 0.75
    ops_ = _random_operands(K, N, r, K + N + r)
    W0, A1, B1, A2, B2, dW = ops_
    jobs, sizes = lh.layout([(K, N, r, s)])
    x = _Loha(jobs, sizes, [ops_], dev, C)
    x.merge(lib)
    x.project(lib)
    torch.cuda.synchronize()
    alone = x.grads(jobs[0])
    o = jobs[0]["w0_off"]
    got32, got16 = x.b.f[o: o + K * N].view(K, N).cpu(), x.b.w[o: o + K * N].view(K, N).cpu()
    x.b.poison()
    x.project(lib)  # the same workspace, not reset
    torch.cuda.synchronize()
    again = x.grads(jobs[0])
    x.b.untouched(x.b.grad, _gspans(jobs), POISON32, "gradient buffer")
    x.check_workspace()
    others = [(k, n, q, 1.0) for k, n, q in lh.cases(C)]
    cases = others[:3] + [(K, N, r, s)] + others[3:]
    operands = [lh.exact_operands(k, n, q, 700 + t) for t, (k, n, q, _) in enumerate(cases)]
    operands[3] = ops_
    tj, tsizes = lh.layout(cases, _shuffled(len(cases), seed=6))
    tx = _Loha(tj, tsizes, operands, dev, C)
    tx.project(lib)
    torch.cuda.synchronize()
    inside = tx.grads([j for j in tj if j["index"] == 3][0])
    tx.check_workspace()
    for what, got in (("second call", again), ("shuffled table", inside)):
        for name, g, a in zip(NAMES, got, alone):
            assert torch.equal(kc.bits(g), kc.bits(a)), f"{name} differs: {what}"
    want = lh.project_ref64(dW, A1, B1, A2, B2, s)
    bounds = lh.projection_bounds(dW, A1, B1, A2, B2, s, C)
    fr = [float(((g.double() - w).abs() / b).max()) for g, w, b in zip(alone, want, bounds)]
    print(f"K={K} N={N} r={r}: worst err/bound " + "  ".join(f"{n} {f:.3f}" for n, f in zip(NAMES, fr)))
    for name, g, w, b in zip(NAMES, alone, want, bounds):
        assert bool(((g.double() - w).abs() <= b).all()), f"{name}: beyond the derived bound"
    v, e = lh.merge_ref64(W0, A1, B1, A2, B2, s), lh.merge_bound(W0, A1, B1, A2, B2, s)
    assert bool(((got32.double() - v).abs() <= e).all())
    assert torch.equal(kc.bits(got32.to(BF)), kc.bits(got16)), "the mirror is the RNE rounding of the fp32 output"


def test_zero_b2_merge_is_the_restore(lib, dev):
    """LyCORIS initialisation: B2 = 0 makes the delta exactly zero - the merged mirror has the bits of sdt_lora_restore's."""
    C = lh.rows()
    cases = [(136, 72, 32, 2.0), (C + 8, 72, 4, 0.5)]
    jobs, sizes = lh.layout(cases)
    operands = []
    for t, (K, N, r, s) in enumerate(cases):
        W0, A1, B1, A2, B2, dW = _random_operands(K, N, r, 40 + t)
        operands.append((W0, A1, B1, A2, torch.zeros_like(B2), dW))
    x = _Loha(jobs, sizes, operands, dev, C)
    b = x.b
    x.merge(lib, f=False)
    torch.cuda.synchronize()
    merged = b.w.clone()
    b.untouched(b.f, [], POISON32, "fp32 destination (not given)")
    b.poison()
    rc = lib.sdt_lora_restore(b.master.data_ptr(), b.w.data_ptr(), b.table, b.table_dev.data_ptr(), len(jobs), _stream())
    assert rc == 0, lib.sdt_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(kc.bits(merged), kc.bits(b.w))
    # and only B2 receives a gradient: P2 = 0 makes G1 = 0
    x.project(lib)
    torch.cuda.synchronize()
    for j in jobs:
        dA1, dB1, dA2, dB2 = x.grads(j)
        assert not bool(dA1.any()) and not bool(dB1.any()) and not bool(dA2.any()) and bool(dB2.any())


def test_empty_launch(lib, dev):
    jobs, sizes = lh.layout([(72, 8, 4, 1.0)])
    x = _Loha(jobs, sizes, [lh.exact_operands(72, 8, 4, 1)], dev, lh.rows())
    x.merge(lib, n=0)
    x.project(lib, n=0)
    assert lib.sdt_loha_merge(None, None, None, None, None, None, None, None, 0, _stream()) == 0
    assert lib.sdt_loha_project(None, None, None, None, None, None, None, None, None, 0, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    x.b.untouched(x.b.w, [], POISON16, "bf16 mirror after n == 0")
    x.b.untouched(x.b.grad, [], POISON32, "gradient buffer after n == 0")
    x.check_workspace()
