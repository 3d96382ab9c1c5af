"""sdt_dora_merge / sdt_dora_init_magnitude / sdt_dora_project on the MI355X, element by element (include/sdt.h "DoRA").

Exact cases: W0 integers in -8..8, A and B in -1..1, G in -3..3, s in {0.5, 1, 2}, m[n] = c[n] * 2^e with e cycling over -1, 0, 1:
every partial sum is exact in fp32 in any order (tests/test_dora_cpu.py proves 4 q and 2 |u| below 2^24 for these very seeds, and
_check_exact asserts it again), so c = fl32(sqrt(q)) and g = 2^e are determined bit for bit, the mirror must be the RNE bf16 rounding
of the float64 reference bit for bit, the fp32 output, dA and dB must equal the reference exactly, dm must be the correctly rounded
fl32(u / c), and the published c and g must match bit for bit.  Every launch runs on poisoned buffers: each byte of the mirror, the fp32
destination, the gradient buffer and the statistics buffer outside the named spans must be unchanged.  Random values: the derived
bounds of the docstring below."""

import pytest
import torch

from tests import dora_reference as dr
from tests import kernel_checks as kc
from tests import lora_reference as lr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON32, POISON16 = 0x7FA5A5A5, 0x7FA5


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Buffers:
    """The flat buffers of one (grouped) launch, filled from per-job operands (W0, A, B, G, m); destinations poisoned."""

    def __init__(self, jobs, sizes, operands, dev):
        self.jobs, self.dev = jobs, dev
        master = torch.full((sizes["master"],), float("nan"), dtype=torch.float32)
        ab = torch.full((sizes["ab"],), float("nan"), dtype=torch.float32)
        dw = torch.full((sizes["dw"],), float("nan"), dtype=BF)
        for j in jobs:
            W0, A, B, G, m = operands[j["index"]]
            K, N, r = j["K"], j["N"], j["r"]
            master[j["w0_off"]: j["w0_off"] + K * N] = W0.reshape(-1)
            ab[j["a_off"]: j["a_off"] + K * r] = A.reshape(-1)
            ab[j["b_off"]: j["b_off"] + r * N] = B.reshape(-1)
            ab[j["m_off"]: j["m_off"] + N] = m
            dw[j["dw_off"]: j["dw_off"] + K * N] = G.reshape(-1)
        self.master, self.ab, self.dw = master.to(dev), ab.to(dev), dw.to(dev)
        self.w = torch.empty(sizes["master"], dtype=BF, device=dev)
        self.f = torch.empty(sizes["master"], dtype=torch.float32, device=dev)
        self.grad = torch.empty(sizes["ab"], dtype=torch.float32, device=dev)
        self.stat = torch.empty(sizes["stat"], dtype=torch.float32, device=dev)
        self.poison()
        self.table, self.dtable = dr.job_tables(jobs)
        self.table_dev = torch.frombuffer(bytearray(bytes(self.table)), dtype=torch.uint8).to(dev)
        self.dtable_dev = torch.frombuffer(bytearray(bytes(self.dtable)), dtype=torch.uint8).to(dev)

    def poison(self):
        self.w.view(torch.int16).fill_(POISON16)
        for t in (self.f, self.grad, self.stat):
            t.view(torch.int32).fill_(POISON32)

    def _tables(self, n):
        return self.table, self.dtable, self.table_dev.data_ptr(), self.dtable_dev.data_ptr(), len(self.jobs) if n is None else n, _stream()

    def merge(self, lib, w=True, f=True, n=None):
        rc = lib.sdt_dora_merge(self.master.data_ptr(), self.ab.data_ptr(), self.w.data_ptr() if w else None,
                                self.f.data_ptr() if f else None, self.stat.data_ptr(), *self._tables(n))
        assert rc == 0, lib.sdt_last_error().decode()

    def init_magnitude(self, lib, n=None):
        rc = lib.sdt_dora_init_magnitude(self.master.data_ptr(), self.ab.data_ptr(), self.ab.data_ptr(), *self._tables(n))
        assert rc == 0, lib.sdt_last_error().decode()

    def project(self, lib, n=None):
        rc = lib.sdt_dora_project(self.dw.data_ptr(), self.master.data_ptr(), self.ab.data_ptr(), self.grad.data_ptr(), self.stat.data_ptr(),
                                  *self._tables(n))
        assert rc == 0, lib.sdt_last_error().decode()

    def untouched(self, buf, spans, poison, what):
        """Every element of `buf` outside `spans` still holds the poison pattern."""
        iv = kc.bits(buf).cpu()
        keep = torch.ones(iv.numel(), dtype=torch.bool)
        for a, b in spans:
            keep[a:b] = False
        top = 1 << (8 * buf.element_size())
        bad = (iv != (poison - top if poison >= top // 2 else poison)) & keep
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the named spans were written, first at {int(bad.nonzero()[0])}"

    def span(self, j, name, n):
        return (j[name], j[name] + n)


def _exact_case(K, N, r, s, seed):
    W0, A, B, G = dr.exact_operands(K, N, r, seed)
    q4, u2 = dr.exact_units(W0, A, B, G, s)
    assert q4 < kc.LIMIT and u2 < kc.LIMIT, (K, N, r, s, q4, u2)
    _, c, _ = dr.column_stats(lr.merge_ref64(W0, A, B, s))
    m, g = dr.exact_magnitude(c)
    return (W0, A, B, G, m), c, g


def _check_exact(lib, dev, cases, order, seed, w=True, f=True):
    jobs, sizes = dr.layout(cases, order)
    built = [_exact_case(K, N, r, s, seed + 10 * i) for i, (K, N, r, s) in enumerate(cases)]
    b = _Buffers(jobs, sizes, [x[0] for x in built], dev)
    b.merge(lib, w=w, f=f)
    b.project(lib)
    torch.cuda.synchronize()
    wspans, gspans, sspans = [], [], []
    for j in jobs:
        (W0, A, B, G, m), c, g = built[j["index"]]
        K, N, r, s = j["K"], j["N"], j["r"], j["s"]
        what = f"K={K} N={N} r={r} s={s}"
        so = j["stat_off"]
        kc.assert_equal_bits(b.stat[so: so + N].cpu(), c, f"published c {what}")
        kc.assert_equal_bits(b.stat[so + N: so + 2 * N].cpu(), g, f"published g {what}")
        sspans.append((so, so + 2 * N))
        v = dr.merge_ref64(W0, A, B, s, g)
        o = j["w0_off"]
        wspans.append((o, o + K * N))
        if w:
            kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), kc.rne_bf16(v), f"merged mirror {what}", tile=(64, 64))
        if f:
            assert torch.equal(v.float().double(), v)
            kc.assert_equal_bits(b.f[o: o + K * N].view(K, N).cpu(), v.float(), f"merged fp32 {what}", tile=(64, 64))
        dA, dB, dm, u = dr.project_ref64(G, W0, A, B, s, c, g)
        assert torch.equal(dA.float().double(), dA) and torch.equal(dB.float().double(), dB) and torch.equal(u.float().double(), u)
        kc.assert_equal_bits(b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu(), dA.float(), f"dA {what}", tile=(64, 16))
        kc.assert_equal_bits(b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu(), dB.float(), f"dB {what}", tile=(16, 64))
        kc.assert_equal_bits(b.grad[j["m_off"]: j["m_off"] + N].cpu(), dr.fl32_div(u, c), f"dm {what}")
        gspans += [b.span(j, "a_off", K * r), b.span(j, "b_off", r * N), b.span(j, "m_off", N)]
    b.untouched(b.w, wspans if w else [], POISON16, "bf16 mirror")
    b.untouched(b.f, wspans if f else [], POISON32, "fp32 destination")
    b.untouched(b.grad, gspans, POISON32, "gradient buffer")
    b.untouched(b.stat, sspans, POISON32, "statistics buffer")
    return b


@pytest.mark.parametrize("i", range(len(dr.CASES)), ids=[f"{K}x{N}r{r}" for K, N, r in dr.CASES])
def test_exact_single(lib, dev, i):
    K, N, r = dr.CASES[i]
    _check_exact(lib, dev, [(K, N, r, dr.SCALES[i % 3])], None, 100 + i)


def test_exact_grouped_shuffled(lib, dev):
    """One launch holding every case, the jobs in shuffled order (stripe lookup by running counts, neighbours, alignment gaps)."""
    cases = [(K, N, r, dr.SCALES[(i + 1) % 3]) for i, (K, N, r) in enumerate(dr.CASES)]
    order = torch.randperm(len(cases), generator=torch.Generator().manual_seed(5)).tolist()
    assert order != sorted(order)
    _check_exact(lib, dev, cases, order, 300)


@pytest.mark.parametrize("w,f", [(True, False), (False, True)], ids=["mirror-only", "fp32-only"])
def test_exact_one_destination(lib, dev, w, f):
    """The training path gives the mirror only, a folded checkpoint the fp32 destination only: the other buffer stays untouched."""
    _check_exact(lib, dev, [(40, 72, 4, 2.0), (136, 72, 64, 0.5)], [1, 0], 400, w=w, f=f)


def test_fresh_adapter_has_unit_gain_and_the_mirror_of_the_base(lib, dev):
    """B = 0 and m written by the init mode: the merge runs the reduction the init ran, so g == 1.0f in every column and the mirror is
    RNE_bf16(W0) bit for bit - on random W0, where c is not a value a host could reproduce without the kernel's summation order.  The
    init call writes the m spans of its destination and nothing else."""
    cases = [(136, 72, 64, 0.75), (320, 320, 16, 2.0), (8, 8, 4, 1.0)]
    jobs, sizes = dr.layout(cases, [2, 0, 1])
    gen = torch.Generator().manual_seed(17)
    operands = [(torch.randn(K, N, generator=gen) * 0.05, torch.randn(K, r, generator=gen), torch.zeros(r, N), torch.zeros(K, N).to(BF),
                 torch.full((N,), float("nan"))) for K, N, r, s in cases]
    b = _Buffers(jobs, sizes, operands, dev)
    before = b.ab.clone()
    b.init_magnitude(lib)
    torch.cuda.synchronize()
    changed = kc.bits(b.ab).cpu() != kc.bits(before).cpu()
    inside = torch.zeros_like(changed)
    for j in jobs:
        inside[j["m_off"]: j["m_off"] + j["N"]] = True
    assert not bool((changed & ~inside).any()), "the init call wrote outside the magnitude leaves"
    b.untouched(b.stat, [], POISON32, "statistics buffer after the init call")
    b.merge(lib)
    torch.cuda.synchronize()
    for j in jobs:
        W0 = operands[j["index"]][0]
        K, N, so, o = j["K"], j["N"], j["stat_off"], j["w0_off"]
        m = b.ab[j["m_off"]: j["m_off"] + N].cpu()
        c64 = W0.double().pow(2).sum(0).sqrt()
        assert bool(((m.double() - c64).abs() <= (lr.gamma(K) / 2 / (1 - lr.gamma(K)) + 2.0 ** -23) * c64).all()), "m is not the column norm"
        kc.assert_equal_bits(b.stat[so: so + N].cpu(), m, f"published c against the initialised m, K={K} N={N}")
        kc.assert_equal_bits(b.stat[so + N: so + 2 * N].cpu(), torch.ones(N), f"g of a fresh adapter, K={K} N={N}")
        kc.assert_equal_bits(b.w[o: o + K * N].view(K, N).cpu(), W0.to(BF), f"mirror of a fresh adapter, K={K} N={N}", tile=(64, 64))
        kc.assert_equal_bits(b.f[o: o + K * N].view(K, N).cpu(), W0, f"fp32 output of a fresh adapter, K={K} N={N}", tile=(64, 64))


def test_zero_column_gives_zeros_and_no_nan(lib, dev):
    """W0 has zero columns (one of them in an edge stripe) and B = 0: c = 0, g = 0, zeros in the mirror, dm = 0, no NaN anywhere."""
    K, N, r, s = 136, 72, 64, 1.0
    gen = torch.Generator().manual_seed(23)
    W0 = torch.randn(K, N, generator=gen)
    zero = [3, 70]
    W0[:, zero] = 0
    ops_ = (W0, torch.randn(K, r, generator=gen), torch.zeros(r, N), torch.randn(K, N, generator=gen).to(BF), torch.rand(N, generator=gen) + 0.5)
    jobs, sizes = dr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [ops_], dev)
    b.merge(lib)
    b.project(lib)
    torch.cuda.synchronize()
    j = jobs[0]
    o, so = j["w0_off"], j["stat_off"]
    w = b.w[o: o + K * N].view(K, N).cpu()
    f = b.f[o: o + K * N].view(K, N).cpu()
    stat = b.stat[so: so + 2 * N].cpu()
    assert not bool(kc.bits(w[:, zero]).any()) and not bool(kc.bits(f[:, zero]).any()), "a zero column is not all +0"
    assert stat[zero].tolist() == [0.0, 0.0] and stat[N:][zero].tolist() == [0.0, 0.0]
    spans = [b.grad[j[k]: j[k] + n].cpu() for k, n in (("a_off", K * r), ("b_off", r * N), ("m_off", N))]
    assert spans[2][zero].tolist() == [0.0, 0.0]
    assert float(spans[1].view(r, N)[:, zero].abs().max()) == 0.0
    for t in (w.float(), f, stat, *spans):
        assert bool(torch.isfinite(t).all())
    keep = [n for n in range(N) if n not in zero]
    assert bool((spans[2][keep] != 0).any()) and bool((w[:, keep] != 0).all())


@pytest.mark.parametrize("K,N,r", dr.RANDOM_CASES)
def test_random_values_within_derived_bounds(lib, dev, K, N, r):
    """Derived, not measured (u_ = 2^-24, gamma_n = n u_ / (1 - n u_), everything evaluated in float64 on the float64 reference).
    v:  as the LoRA file: r - 1 additions, the scaling, the sum with W0: |v_gpu - v| <= ev = gamma_{r+2} (|W0| + s sum|A||B|).
    q:  sums K squares - one product rounding and K - 1 additions: K roundings - of v_gpu:
        |q_gpu - q| <= eq = gamma_K (q + dq) + dq, dq = sum_k (2 |v| ev + ev^2).
    c:  one more rounding: |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b), so |c_gpu - c| <= ec = eq / c + u_ (c + eq / c).
    g:  one more: |g_gpu - m / c| <= eg = |m| ec / (c (c - ec)) + u_ |m| / (c - ec).
    W': fl32(v_gpu g_gpu): e = ev (|g| + eg) + |v| eg + u_ (|v| + ev)(|g| + eg); the mirror must lie between the RNE roundings of
        ref -+ e and must be the RNE rounding of the fp32 output.
    The projection is checked at the c and g the kernel published (just bounded): its bf16 rounding of B g is an evaluation point and
    another g, one ulp away, would flip roundings.  dA: N - 1 additions and the scaling: gamma_N s sum|G||bf16(B g)|.  dB: K - 1
    additions, the scaling, the gain: gamma_{K+2} s sum|A||G| |g|.  dm: a term of P carries K - 1 additions, then the product with B,
    r - 1 additions, the scaling, the sum with sum_k G W0 (whose terms carry K + 1) and the division: gamma_{K+r+2} of
    (sum|G||W0| + s sum_q |B| sum_k |A||G|) / c."""
    s, u_ = 0.75, 2.0 ** -24
    gen = torch.Generator().manual_seed(K + N + r)
    W0 = torch.randn(K, N, generator=gen) * 0.05
    A = torch.randn(K, r, generator=gen) * 0.1
    B = torch.randn(r, N, generator=gen) * 0.1
    G = (torch.randn(K, N, generator=gen) * 0.01).to(BF)
    v = lr.merge_ref64(W0, A, B, s)
    q, c32, _ = dr.column_stats(v)
    m = (c32 * (1 + 0.2 * torch.randn(N, generator=gen))).float()
    jobs, sizes = dr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [(W0, A, B, G, m)], dev)
    b.merge(lib)
    b.project(lib)
    torch.cuda.synchronize()
    j = jobs[0]
    so, o = j["stat_off"], j["w0_off"]
    cp, gp = b.stat[so: so + N].cpu(), b.stat[so + N: so + 2 * N].cpu()
    ev = lr.gamma(r + 2) * (W0.double().abs() + s * (lr.bf(A).abs() @ lr.bf(B).abs()))
    dq = (2 * v.abs() * ev + ev ** 2).sum(0)
    eq = lr.gamma(K) * (q + dq) + dq
    c, md = q.sqrt(), m.double()
    ec = eq / c + u_ * (c + eq / c)
    g = md / c
    eg = md.abs() * ec / (c * (c - ec)) + u_ * md.abs() / (c - ec)
    print(f"c worst err/bound {((cp.double() - c).abs() / ec).max():.3f}  g {((gp.double() - g).abs() / eg).max():.3f}")
    assert bool(((cp.double() - c).abs() <= ec).all()) and bool(((gp.double() - g).abs() <= eg).all())
    ref = v * g[None, :]
    e = ev * (g.abs() + eg)[None, :] + v.abs() * eg[None, :] + u_ * (v.abs() + ev) * (g.abs() + eg)[None, :]
    got32 = b.f[o: o + K * N].view(K, N).cpu()
    got16 = b.w[o: o + K * N].view(K, N).cpu()
    print(f"W' worst err/bound {((got32.double() - ref).abs() / e).max():.3f}")
    assert bool(((got32.double() - ref).abs() <= e).all())
    lo, hi = (ref - e).float().to(BF).double(), (ref + e).float().to(BF).double()
    assert bool(((got16.double() >= lo) & (got16.double() <= hi)).all())
    assert torch.equal(kc.bits(got32.to(BF)), kc.bits(got16)), "the mirror is the RNE rounding of the fp32 output"
    dA, dB, dm, _ = dr.project_ref64(G, W0, A, B, s, cp, gp)
    gotA = b.grad[j["a_off"]: j["a_off"] + K * r].view(K, r).cpu().double()
    gotB = b.grad[j["b_off"]: j["b_off"] + r * N].view(r, N).cpu().double()
    gotm = b.grad[j["m_off"]: j["m_off"] + N].cpu().double()
    absP = lr.bf(A).abs().T @ G.double().abs()
    boundA = lr.gamma(N) * s * (G.double().abs() @ dr.scaled_b(B, gp).abs().T)
    boundB = lr.gamma(K + 2) * s * absP * gp.double().abs()[None, :]
    boundm = lr.gamma(K + r + 2) * ((G.double().abs() * W0.double().abs()).sum(0) + s * (lr.bf(B).abs() * absP).sum(0)) / cp.double()
    print(f"dA worst err/bound {((gotA - dA).abs() / boundA).max():.3f}  dB {((gotB - dB).abs() / boundB).max():.3f}  "
          f"dm {((gotm - dm).abs() / boundm).max():.3f}")
    assert bool(((gotA - dA).abs() <= boundA).all()) and bool(((gotB - dB).abs() <= boundB).all())
    assert bool(((gotm - dm).abs() <= boundm).all())


def test_repeatable_and_empty_launch(lib, dev):
    K, N, r, s = 136, 72, 64, 1.0
    gen = torch.Generator().manual_seed(9)
    ops_ = (torch.randn(K, N, generator=gen), torch.randn(K, r, generator=gen), torch.randn(r, N, generator=gen),
            torch.randn(K, N, generator=gen).to(BF), torch.rand(N, generator=gen) + 0.5)
    jobs, sizes = dr.layout([(K, N, r, s)])
    b = _Buffers(jobs, sizes, [ops_], dev)
    before = b.ab.clone()
    b.merge(lib, n=0)  # n == 0: success, nothing launched, nothing written
    b.project(lib, n=0)
    b.init_magnitude(lib, n=0)
    assert lib.sdt_dora_merge(None, None, None, None, None, None, None, None, None, 0, _stream()) == 0
    assert lib.sdt_dora_init_magnitude(None, None, None, None, None, None, None, 0, _stream()) == 0
    assert lib.sdt_dora_project(None, None, None, None, None, None, None, None, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    b.untouched(b.w, [], POISON16, "bf16 mirror after n == 0")
    b.untouched(b.f, [], POISON32, "fp32 destination after n == 0")
    b.untouched(b.grad, [], POISON32, "gradient buffer after n == 0")
    b.untouched(b.stat, [], POISON32, "statistics buffer after n == 0")
    assert torch.equal(kc.bits(b.ab), kc.bits(before)), "the init call with n == 0 wrote"
    runs = []
    for _ in range(2):
        b.poison()
        b.merge(lib)
        b.project(lib)
        torch.cuda.synchronize()
        runs.append((b.w.clone(), b.f.clone(), b.grad.clone(), b.stat.clone()))
    for x, y in zip(*runs):
        assert torch.equal(kc.bits(x), kc.bits(y))
