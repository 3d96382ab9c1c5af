"""sdt_lora_merge / sdt_lora_project on the MI355X, element by element (include/sdt.h "LoRA").

Exact cases: A, B, dW integers in -3..3, W0 a multiple of 1/8 with |W0| <= 128, s in {0.5, 1, 2}: every sum is exact in fp32 in any
order (tests/test_lora_cpu.py proves the bound per case), so the merged mirror must be the RNE bf16 rounding of the float64 reference
bit for bit - ties included - and the fp32 output, dA and dB must equal the reference exactly.  Every launch runs on poisoned buffers:
each byte of the mirror, the fp32 destination and the gradient buffer outside the named leaves must be unchanged (front and back
margins, the 8-element alignment gaps, non-adapted neighbours).  Random values: the derived bounds of the docstrings below."""

import pytest
import torch

from tests import kernel_checks as kc
from tests import lora_reference as lr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON32, POISON16 = 0x7FA5A5A5, 0x7FA5


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Buffers:
    """The flat buffers of one (grouped) launch, filled from per-job operands; destinations poisoned."""

    def __init__(self, jobs, sizes, operands, dev):
        self.jobs, self.dev = jobs, dev
        self.master = torch.full((sizes["master"],), float("nan"), dtype=torch.float32)
        self.ab = torch.full((sizes["ab"],), float("nan"), dtype=torch.float32)
        self.dw = torch.full((sizes["dw"],), float("nan"), dtype=BF)
        for j in jobs:
            W0, A, B, dW = operands[j["index"]]
            K, N, r = j["K"], j["N"], j["r"]
            self.master[j["w0_off"]: j["w0_off"] + K * N] = W0.reshape(-1)
            self.ab[j["a_off"]: j["a_off"] + K * r] = A.reshape(-1)
            self.ab[j["b_off"]: j["b_off"] + r * N] = B.reshape(-1)
            self.dw[j["dw_off"]: j["dw_off"] + K * N] = dW.reshape(-1)
        self.master, self.ab, self.dw = self.master.to(dev), self.ab.to(dev), self.dw.to(dev)
        self.w = torch.empty(sizes["master"], dtype=BF, device=dev)
        self.f = torch.empty(sizes["master"], dtype=torch.float32, device=dev)
        self.grad = torch.empty(sizes["ab"], dtype=torch.float32, device=dev)
        self.poison()
        self.table = lr.job_table(jobs)
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(dev)

    def poison(self):
        self.w.view(torch.int16).fill_(POISON16)
        self.f.view(torch.int32).fill_(POISON32)
        self.grad.view(torch.int32).fill_(POISON32)

    def merge(self, lib, w=True, f=True, n=None):
        n = len(self.jobs) if n is None else n
        rc = lib.sdt_lora_merge(self.master.data_ptr(), self.ab.data_ptr(), self.w.data_ptr() if w else None,
                                self.f.data_ptr() if f else None, self.table, self.table_dev.data_ptr(), n, _stream())
        assert rc == 0, lib.sdt_last_error().decode()

    def project(self, lib, n=None):
        n = len(self.jobs) if n is None else n
        rc = lib.sdt_lora_project(self.dw.data_ptr(), self.ab.data_ptr(), self.grad.data_ptr(), self.table, self.table_dev.data_ptr(), n,
                                  _stream())
        assert rc == 0, lib.sdt_last_error().decode()

    def untouched(self, buf, spans, poison, what):
        """Every element of `buf` outside `spans` still holds the poison pattern."""
        iv = kc.bits(buf).cpu()
        keep = torch.ones(iv.numel(), dtype=torch.bool)
        for a, b in spans:
            keep[a:b] = False
        top = 1 << (8 * buf.element_size())
        bad = (iv != (poison - top if poison >= top // 2 else poison)) & keep
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the named leaves were written, first at {int(bad.nonzero()[0])}"


def _check_exact(lib, dev, cases, order, seed, w=True, f=True):
    jobs, sizes = lr.layout(cases, order)
    operands = [lr.exact_operands(K, N, r, seed + 10 * i) for i, (K, N, r, s) in enumerate(cases)]
    b = _Buffers(jobs, sizes, operands, dev)
    b.merge(lib, w=w, f=f)
    b.project(lib)
    torch.cuda.synchronize()
    wspans, gspans = [], []
    for j in jobs:
        W0, A, B, dW = operands[j["index"]]
        K, N, r, s = j["K"], j["N"], j["r"], j["s"]
        what = f"K={K} N={N} r={r} s={s}"
        v = lr.merge_ref64(W0, A, B, s)
        o = j["w0_off"]
        wspans.append((o, o + K * N))
        if w:
            kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(v), f"merged mirror {what}", tile=(64, 64))
        if f:
            kc.assert_equal_bits(b.f[o: o + K * N].view(K, N).cpu(), v.float(), f"merged fp32 {what}", tile=(64, 64))
            assert torch.equal(v.float().double(), v)
        dA, dB = lr.project_ref64(dW, A, B, s)
        assert torch.equal(dA.float().double(), dA) and torch.equal(dB.float().double(), dB)
        kc.assert_equal_bits(b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu(), dA.float(), f"dA {what}", tile=(64, 16))
        kc.assert_equal_bits(b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu(), dB.float(), f"dB {what}", tile=(16, 64))
        gspans += [(j["a_off"], j["a_off"] + K * r), (j["b_off"], j["b_off"] + r * N)]
    b.untouched(b.w, wspans if w else [], POISON16, "bf16 mirror")
    b.untouched(b.f, wspans if f else [], POISON32, "fp32 destination")
    b.untouched(b.grad, gspans, POISON32, "gradient buffer")
    return b


@pytest.mark.parametrize("i", range(len(lr.CASES)), ids=[f"{K}x{N}r{r}" for K, N, r in lr.CASES])
def test_exact_single(lib, dev, i):
    K, N, r = lr.CASES[i]
    _check_exact(lib, dev, [(K, N, r, lr.SCALES[i % 3])], None, 100 + i)


def test_exact_grouped_shuffled(lib, dev):
    """One launch holding every case, the jobs in shuffled order (tile lookup by running counts, neighbours, alignment gaps)."""
    cases = [(K, N, r, lr.SCALES[(i + 1) % 3]) for i, (K, N, r) in enumerate(lr.CASES)]
    order = torch.randperm(len(cases), generator=torch.Generator().manual_seed(5)).tolist()
    assert order != sorted(order)
    _check_exact(lib, dev, cases, order, 300)


@pytest.mark.parametrize("w,f", [(True, False), (False, True)], ids=["mirror-only", "fp32-only"])
def test_exact_one_destination(lib, dev, w, f):
    """The training path gives the mirror only, a folded checkpoint the fp32 destination only: the other buffer stays untouched."""
    _check_exact(lib, dev, [(40, 72, 4, 2.0), (136, 72, 64, 0.5)], [1, 0], 400, w=w, f=f)


@pytest.mark.parametrize("K,N,r", lr.RANDOM_CASES)
def test_random_values_within_derived_bounds(lib, dev, K, N, r):
    """fp32 accumulation of exact bf16 x bf16 products: |dA - ref64| <= gamma_N * s * sum|dW||B| and |dB - ref64| <= gamma_K * s * sum|A||dW|
    (n - 1 additions and the scaling: n roundings).  Merge: v carries r - 1 additions, the scaling and the sum with W0, e = gamma_{r+2} *
    (|W0| + s * sum|A||B|), and the mirror lies between RNE(ref - e) and RNE(ref + e).  Derived, not measured."""
    s = 0.75
    g = torch.Generator().manual_seed(K + N + r)
    W0 = torch.randn(K, N, generator=g) * 0.05
    A = torch.randn(K, r, generator=g) * 0.1
    B = torch.randn(r, N, generator=g) * 0.1
    dW = (torch.randn(K, N, generator=g) * 0.01).to(BF)
    jobs, sizes = lr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [(W0, A, B, dW)], dev)
    b.merge(lib)
    b.project(lib)
    torch.cuda.synchronize()
    j = jobs[0]
    dA, dB = lr.project_ref64(dW, A, B, s)
    gotA = b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu().double()
    gotB = b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu().double()
    boundA = lr.gamma(N) * s * (dW.double().abs() @ lr.bf(B).abs().T)
    boundB = lr.gamma(K) * s * (lr.bf(A).abs().T @ dW.double().abs())
    print(f"dA worst err/bound {((gotA - dA).abs() / boundA).max():.3f}  dB {((gotB - dB).abs() / boundB).max():.3f}")
    assert bool(((gotA - dA).abs() <= boundA).all()) and bool(((gotB - dB).abs() <= boundB).all())
    v = lr.merge_ref64(W0, A, B, s)
    e = lr.gamma(r + 2) * (W0.double().abs() + s * (lr.bf(A).abs() @ lr.bf(B).abs()))
    o = j["w0_off"]
    got = b.w[o: o + K * N].view(K, N).cpu().double()
    lo, hi = (v - e).float().to(BF).double(), (v + e).float().to(BF).double()
    assert bool(((got >= lo) & (got <= hi)).all())
    got32 = b.f[o: o + K * N].view(K, N).cpu()
    assert bool(((got32.double() - v).abs() <= e).all())
    assert torch.equal(kc.bits(got32.to(BF)), kc.bits(b.w[o: o + K * N].view(K, N).cpu())), "the mirror is the RNE rounding of the fp32 output"


def test_repeatable_and_empty_launch(lib, dev):
    K, N, r, s = 136, 72, 64, 1.0
    g = torch.Generator().manual_seed(9)
    ops_ = (torch.randn(K, N, generator=g), torch.randn(K, r, generator=g), torch.randn(r, N, generator=g), torch.randn(K, N, generator=g).to(BF))
    jobs, sizes = lr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [ops_], dev)
    b.merge(lib, n=0)  # n == 0: success, nothing launched, nothing written
    b.project(lib, n=0)
    assert lib.sdt_lora_merge(None, None, None, None, None, None, 0, _stream()) == 0
    assert lib.sdt_lora_project(None, None, None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    b.untouched(b.w, [], POISON16, "bf16 mirror after n == 0")
    b.untouched(b.f, [], POISON32, "fp32 destination after n == 0")
    b.untouched(b.grad, [], POISON32, "gradient buffer after n == 0")
    runs = []
    for _ in range(2):
        b.poison()
        b.merge(lib)
        b.project(lib)
        torch.cuda.synchronize()
        runs.append((b.w.clone(), b.f.clone(), b.grad.clone()))
    for x, y in zip(*runs):
        assert torch.equal(kc.bits(x), kc.bits(y))
