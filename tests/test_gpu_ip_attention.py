"""sdt_ip_attention_fwd / _bwd (include/sdt.h "IP-ADAPTER") on a real MI355X: every bit on the exact constructions of
tests/kernel_checks.py against tests/ip_adapter_reference.ip_expect_bits, the project's attention gates on random values, guarded
buffers, reproducibility, and ops.attention_ip on top of the C calls.

Shapes (B, H, Nq, T, D):
  (2, 2, 70, 4, 40)    ragged rows, two images with different scale_ip, 5 sixteen-byte chunks per head
  (1, 3, 130, 16, 64)  largest T (the 8-byte backward), power-of-two scale
  (2, 1, 65, 1, 8)     T = 1: p == 1, dK exactly zero, smallest D
  (1, 2, 257, 5, 160)  odd T, largest D
  (2, 8, 64, 4, 160)   SD1.5's mid block
  (1, 8, 4100, 4, 40)  the dK / dV sum crosses many workgroups' partials
The only tolerances are tests/test_gpu_kernels.py::test_attention_fwd_bwd's: rel-L2 < 8e-3 forward, < 1.5e-2 for dq, dk and dv."""
import pytest
import torch

from tests import ip_adapter_reference as R
from tests import kernel_checks as kc
from tests.helpers import rel_l2
from tests.kernel_checks import BF, Guarded, assert_equal_bits

pytestmark = pytest.mark.gpu

SMALL = [(2, 2, 70, 4, 40), (1, 3, 130, 16, 64), (2, 1, 65, 1, 8), (1, 2, 257, 5, 160), (2, 8, 64, 4, 160)]
LARGE = (1, 8, 4100, 4, 40)
SCALE_SETS = [None, [1.0, 1.0], [0.0, -0.75], [2.5, 2.0 ** -10]]
FWD_GATE, BWD_GATE = 8e-3, 1.5e-2
_IDS = lambda s: "x".join(str(v) for v in s)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A [rows][ld] bf16 operand (payload columns [0, width)) inside one Guarded arena, `shift` elements past its 16-byte aligned base
    (shift = 1: a 2-byte offset base, the element path).  Outputs: every element outside the payload must still hold the sentinel."""

    def __init__(self, rows, width, ld, dev, data=None, shift=0):
        self.rows, self.width, self.ld, self.shift = rows, width, ld, shift
        n = rows * ld + shift
        img = None
        if data is not None:
            img = torch.full((n,), float("nan"), dtype=BF)
            img[shift:].view(rows, ld)[:, :width] = data.reshape(rows, width).to(BF)
        self.g = Guarded(1, n, BF, dev, data=img, pad=0, back_rows=1)  # one 'row': a back guard as long as the operand

    @property
    def ptr(self):
        return self.g.ptr + 2 * self.shift

    @property
    def t(self):
        return self.g.t.reshape(-1)[self.shift:].view(self.rows, self.ld)[:, : self.width]

    def check(self, what):
        self.g.check(what)
        if not self.g.is_input:
            flat = kc.bits(self.g.t.reshape(-1)).clone()
            s = kc.SENTINEL[BF]
            flat[self.shift:].view(self.rows, self.ld)[:, : self.width] = s
            bad = int((flat != s).sum())
            assert bad == 0, f"{what}: {bad} elements outside the payload were written (ld {self.ld}, width {self.width}, shift {self.shift})"


def _workspace(need, dev):
    """A guarded fp32 arena of `need` bytes: counters zero (the contract), slots poisoned with the sentinel NaN."""
    g = Guarded(1, need // 4, torch.float32, dev, pad=0, back_rows=1)
    g.t.view(-1)[: kc.CNT_BYTES // 4] = 0
    return g


def _run(lib_call, dev, case, shape, wide, shift, o_txt, dq_in, scale_ip):
    """One forward and one backward launch on guarded operands; returns (out, dq, dkv) on the CPU after checking every guard and the
    workspace counters."""
    from stable_diffusion_training_amd import _lib
    B, H, Nq, T, D = shape
    C, scale = H * D, D ** -0.5
    ldq, ldkv, ld_dkv = (C + 24, 2 * C + 40, 2 * C + 8) if wide else (C, 2 * C, 2 * C)
    kv = torch.cat([case["k"], case["v"]], -1)
    q_b = Buf(B * Nq, C, ldq, dev, case["q"], shift)
    kv_b = Buf(B * T, 2 * C, ldkv, dev, kv, shift)
    do_b = Buf(B * Nq, C, C, dev, case["dout"], shift)
    ot_b = None if o_txt is None else Buf(B * Nq, C, C, dev, o_txt, shift)
    di_b = None if dq_in is None else Buf(B * Nq, C, C, dev, dq_in, shift)
    out_b, dq_b = Buf(B * Nq, C, C, dev, shift=shift), Buf(B * Nq, C, C, dev, shift=shift)
    dkv_b = Buf(B * T, 2 * C, ld_dkv, dev, shift=shift)
    sip = None if scale_ip is None else torch.tensor(scale_ip[:B], dtype=torch.float32, device=dev)
    need = _lib.load().sdt_ip_attention_bwd_workspace_bytes(B, H, Nq, T, D)
    assert need >= kc.CNT_BYTES
    ws = _workspace(need, dev)
    p = lambda b: None if b is None else b.ptr
    lib_call("sdt_ip_attention_fwd", q_b.ptr, kv_b.ptr, p(ot_b), None if sip is None else sip.data_ptr(), out_b.ptr, B, H, Nq, T, D, ldq,
             ldkv, scale, _stream())
    lib_call("sdt_ip_attention_bwd", q_b.ptr, kv_b.ptr, do_b.ptr, None if sip is None else sip.data_ptr(), p(di_b), dq_b.ptr, dkv_b.ptr,
             B, H, Nq, T, D, ldq, ldkv, ld_dkv, scale, ws.ptr, need, _stream())
    torch.cuda.synchronize()
    for what, b in dict(q=q_b, kv=kv_b, dout=do_b, o_txt=ot_b, dq_in=di_b, out=out_b, dq=dq_b, dkv=dkv_b).items():
        if b is not None:
            b.check(f"{what} {shape} wide={wide} shift={shift}")
    ws.check("workspace")
    msg = kc.counters_report(ws.t.reshape(-1).view(torch.uint8), "sdt_ip_attention_bwd workspace")
    assert msg is None, msg
    return (out_b.t.cpu().reshape(B, Nq, C), dq_b.t.cpu().reshape(B, Nq, C), dkv_b.t.cpu().reshape(B, T, 2 * C))


def _bf16_noise(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(BF)


@pytest.fixture(scope="module")
def exact_cases():
    """(shape, kind) -> the exact inputs, built once: selector (P one-hot) and tied pairs (P = 1/2, 1/2) with Nk = T."""
    cases = {}
    for i, (B, H, Nq, T, D) in enumerate(SMALL):
        cases[(B, H, Nq, T, D), "selector"] = kc.selector_case(B, H, Nq, T, D, False, 310 + i)
        cases[(B, H, Nq, T, D), "pair"] = kc.pair_case(B, H, Nq, T, D, 320 + i)
    return cases


@pytest.mark.parametrize("kind", ["selector", "pair"])
@pytest.mark.parametrize("wide", [False, True], ids=["contiguous", "wide"])
@pytest.mark.parametrize("shape", SMALL, ids=_IDS)
def test_ip_attention_every_bit(dev, exact_cases, shape, wide, kind):
    """out, dq and dkv hold the bits of ip_expect_bits with random bf16 o_txt / dq_in under every scale_ip set, forward and backward
    at every small shape (D = 64: a power-of-two scale; 40, 8 and 160: scales that are not)."""
    from stable_diffusion_training_amd._lib import call
    B, H, Nq, T, D = shape
    C = H * D
    case = exact_cases[shape, kind]
    lead = R.min_lead(case, B, H, Nq, T, D, D ** -0.5)
    assert lead > 110.0, f"lead {lead}: the losers' fp32 exponentials would not underflow to zero"
    o_txt, dq_in = _bf16_noise((B, Nq, C), 7), _bf16_noise((B, Nq, C), 8)
    for s in SCALE_SETS:
        sip = None if s is None else torch.tensor(s[:B], dtype=torch.float32)
        want = R.ip_expect_bits(case, B, H, Nq, T, D, D ** -0.5, o_txt=o_txt, dq_in=dq_in, scale_ip=sip)
        out, dq, dkv = _run(call, dev, case, shape, wide, 0, o_txt, dq_in, s)
        what = f"{kind} {shape} scale_ip={s}"
        assert_equal_bits(out, want["out"], f"out {what}", tile=(64, D))
        assert_equal_bits(dq, want["dq"], f"dq {what}", tile=(64, D))
        assert_equal_bits(dkv, want["dkv"], f"dkv {what}")
        if T == 1:
            assert int(torch.count_nonzero(dkv[..., :C])) == 0, "T = 1: p == 1 and dK must be exactly zero"
    if kind == "pair" and T > 1:
        assert int(torch.count_nonzero(want["dkv"][..., :C])) > 0 and not torch.equal(want["dq"], dq_in), "the pair case must move dq and dK"


def test_ip_attention_element_path(dev, exact_cases):
    """2-byte-offset bases: no vector access is possible; the same bits as the aligned path, with and without the text operands."""
    from stable_diffusion_training_amd._lib import call
    for shape in (SMALL[0], SMALL[1]):
        B, H, Nq, T, D = shape
        case = exact_cases[shape, "pair"]
        o_txt, dq_in = _bf16_noise((B, Nq, H * D), 17), _bf16_noise((B, Nq, H * D), 18)
        for ot, di, s in ((o_txt, dq_in, SCALE_SETS[3]), (None, None, None)):
            sip = None if s is None else torch.tensor(s[:B], dtype=torch.float32)
            want = R.ip_expect_bits(case, B, H, Nq, T, D, D ** -0.5, o_txt=ot, dq_in=di, scale_ip=sip)
            out, dq, dkv = _run(call, dev, case, shape, True, 1, ot, di, s)
            for n, got in (("out", out), ("dq", dq), ("dkv", dkv)):
                assert_equal_bits(got, want[n], f"{n} {shape} at a 2-byte offset")


def _random_case(shape, seed):
    B, H, Nq, T, D = shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF)
    return dict(q=r(B, Nq, H * D), k=r(B, T, H * D), v=r(B, T, H * D), dout=r(B, Nq, H * D))


@pytest.fixture(scope="module")
def random_refs():
    """shape -> (case, fp32 torch softmax reference), computed once and shared."""
    refs = {}
    for i, shape in enumerate(SMALL + [LARGE]):
        case = _random_case(shape, 400 + i)
        refs[shape] = (case, R.softmax_ref32(case["q"], torch.cat([case["k"], case["v"]], -1), case["dout"], shape[1], shape[4] ** -0.5))
    return refs


@pytest.mark.parametrize("wide", [False, True], ids=["contiguous", "wide"])
@pytest.mark.parametrize("shape", SMALL + [LARGE], ids=_IDS)
def test_ip_attention_random(dev, random_refs, shape, wide):
    """The image term alone (o_txt = dq_in = NULL, so the text term cannot hide an error) against fp32 torch softmax under the
    project's attention gates; two launches give equal bits."""
    from stable_diffusion_training_amd._lib import call
    B, H, Nq, T, D = shape
    C = H * D
    case, (o_ref, dq_ref, dkv_ref) = random_refs[shape]
    out, dq, dkv = _run(call, dev, case, shape, wide, 0, None, None, None)
    figs = dict(out=rel_l2(out, o_ref), dq=rel_l2(dq, dq_ref), dk=rel_l2(dkv[..., :C], dkv_ref[..., :C]), dv=rel_l2(dkv[..., C:], dkv_ref[..., C:]))
    print(f"ip_attention random {shape} wide={wide}: " + ", ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert figs["out"] < FWD_GATE, figs
    assert figs["dq"] < BWD_GATE and figs["dk"] < BWD_GATE and figs["dv"] < BWD_GATE, figs
    again = _run(call, dev, case, shape, wide, 0, None, None, None)
    for n, a, b in zip(("out", "dq", "dkv"), (out, dq, dkv), again):
        assert_equal_bits(b, a, f"{n} {shape}: second launch")


def test_ip_attention_random_with_text_terms(dev, random_refs):
    """Random o_txt / dq_in and a per-image scale: out under the forward gate, dq under the backward gate."""
    from stable_diffusion_training_amd._lib import call
    shape = SMALL[0]
    B, H, Nq, T, D = shape
    case, (o_ref, dq_ref, _) = random_refs[shape]
    o_txt, dq_in = _bf16_noise((B, Nq, H * D), 27), _bf16_noise((B, Nq, H * D), 28)
    out, dq, _ = _run(call, dev, case, shape, False, 0, o_txt, dq_in, None)
    assert rel_l2(out, o_txt.float() + o_ref) < FWD_GATE
    assert rel_l2(dq, dq_in.float() + dq_ref) < BWD_GATE
    s = [0.5, -1.25]
    out, _, _ = _run(call, dev, case, shape, False, 0, o_txt, dq_in, s)
    assert rel_l2(out, o_txt.float() + torch.tensor(s).view(B, 1, 1) * o_ref) < FWD_GATE


def test_attention_ip_op(dev, random_refs):
    """ops.attention_ip: a zero v slice returns the text attention's output; q.grad is the C call's dq bit for bit; kv_ip as a column
    slice of a wider projection; the sampling-only refusal."""
    from stable_diffusion_training_amd import ops
    from stable_diffusion_training_amd._lib import call, load
    shape = SMALL[0]
    B, H, Nq, T, D = shape
    C, scale, Nk = H * D, D ** -0.5, 77
    case, _ = random_refs[shape]
    q = case["q"].to(dev)
    kv_txt = _bf16_noise((B, Nk, 2 * C), 31).to(dev)
    wide = torch.zeros(B, T, 2 * C + 64, dtype=BF, device=dev)
    wide[..., 32: 32 + C] = case["k"].to(dev)
    kv_zero_v = wide[..., 32: 32 + 2 * C]
    kw = torch.ones(Nk, dtype=torch.float32, device=dev)
    kw[5] = 2.0
    o_txt = ops.attention_packed(q, kv_txt, H, scale, key_weight=kw)
    assert torch.equal(ops.attention_ip(q, kv_txt, kv_zero_v, H, scale, key_weight=kw), o_txt)
    assert torch.equal(ops.attention_ip(q, kv_txt, kv_zero_v, H, scale, key_weight=kw, scale_ip=torch.tensor([3.0, -2.0], device=dev)), o_txt)

    wide[..., 32 + C: 32 + 2 * C] = case["v"].to(dev)
    kv_ip = wide[..., 32: 32 + 2 * C].detach().requires_grad_(True)
    qa, qb = q.clone().requires_grad_(True), q.clone().requires_grad_(True)
    kva, kvb = kv_txt.clone().requires_grad_(True), kv_txt.clone().requires_grad_(True)
    dout = case["dout"].to(dev)
    out = ops.attention_ip(qa, kva, kv_ip, H, scale, key_weight=kw)
    assert rel_l2(out, o_txt.float()) > 0.05, "the image term must be visible"
    out.backward(dout)
    ops.attention_packed(qb, kvb, H, scale, key_weight=kw).backward(dout)
    assert torch.equal(kva.grad, kvb.grad), "the text keys' gradient is the text attention's"
    dq, dkv = torch.empty_like(q), torch.empty(B, T, 2 * C, dtype=BF, device=dev)
    need = load().sdt_ip_attention_bwd_workspace_bytes(B, H, Nq, T, D)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    call("sdt_ip_attention_bwd", q.data_ptr(), kv_ip.data_ptr(), dout.data_ptr(), None, qb.grad.data_ptr(), dq.data_ptr(), dkv.data_ptr(),
         B, H, Nq, T, D, C, kv_ip.stride(1), 2 * C, scale, ws.data_ptr(), need, _stream())
    assert_equal_bits(qa.grad.cpu(), dq.cpu(), "q.grad of ops.attention_ip against the C call's dq")
    assert_equal_bits(kv_ip.grad.cpu(), dkv.cpu(), "kv_ip.grad of ops.attention_ip against the C call's dkv")
    with pytest.raises(ValueError, match="sampling only"):
        ops.attention_ip(q, kv_txt, kv_ip, H, scale, scale_ip=torch.ones(B, device=dev))
