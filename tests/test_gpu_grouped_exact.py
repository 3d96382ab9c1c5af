"""The grouped off-chain launches, every bit, on a real MI355X (tables and mirrors: tests/kernel_checks.py "grouped off-chain launches";
their proof on the CPU: tests/test_kernel_checks_cpu.py).

sdt_attention_bwd_dkv_group runs tables of tied-pair and selector problems (kernel_checks.pair_case / selector_case) that differ in B, H,
key blocks, query split, layout and instantiation: dk and dv of every problem must hold the bits of pair_expect / selector_expect -
the float64 expectation of that ONE problem, so a workgroup decoded with a neighbour's H or gx, a second launch of a class that starts
at the wrong entry or a finishing pass that adds the planned instead of the launched slabs shows in a named problem - and also the
bits of the inline sdt_attention_bwd.  sdt_colsum_batched_group runs kernel_checks.COLSUM_CASES and COLSUM_GROUP_MAXED as single
calls: the RNE bf16 of the float64 sums, three launches on one workspace whose counters nobody zeroes in between.

Every operand, result, delta row, slab area and workspace sits in a guarded arena (kernel_checks.Guarded).  This file has no tolerance."""
import ctypes
import random

import pytest
import torch

from tests import kernel_checks as kc
from tests.kernel_checks import BF, Guarded, assert_equal_bits, exact_ints, pair_reports
from tests.test_gpu_kernel_exact import _attn_arenas, _stream

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _sentinel_everywhere(g):
    """Whether every element of an output arena - payload included - still holds the sentinel."""
    ref = Guarded(g.rows, g.width, g.dtype, g.arena.device, pad=g.ld - g.width)
    return ref.arena.numel() == g.arena.numel() and torch.equal(kc.bits(g.arena), kc.bits(ref.arena))


# ================================================================================================ sdt_attention_bwd_dkv_group
class _Problem:
    """One table entry on guarded arenas: the forward and the dQ pass have run (out and dq checked against the expectation, delta
    against the inline call's); arm() gives fresh dk / dv / slab arenas, entry() the table entry over them, check() judges them."""

    def __init__(self, dev, lib, spec):
        from stable_diffusion_training_amd import _lib
        self.dev, self.lib, self.spec = dev, lib, spec
        B, H, Nq, Nk, D, kind, packed, kw, causal = spec
        C = H * D
        self.what = f"problem {spec}"
        self.case, self.want = kc.dkv_group_problem(spec)
        self.plan = kc.dkv_group_plan(spec)
        w = kc.group_key_weights(Nk) if kw else None
        self.WG = None if w is None else Guarded(1, Nk, F32, dev, data=w, pad=0, back_rows=1)
        self.Q, self.DO, self.KG, self.VG, self.kptr, self.vptr, ldkv = _attn_arenas(dev, self.case, B, H, Nq, Nk, D, packed)
        self.O, self.LSE = Guarded(B * Nq, C, BF, dev), Guarded(1, B * H * Nq, F32, dev, pad=0, back_rows=1)
        self.DQ = Guarded(B * Nq, C, BF, dev)
        ldg = 2 * C + 16 if packed else C + 16
        self.desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, self.Q.ld, ldkv, ldkv, self.O.ld, D ** -0.5, int(causal), self.DQ.ld, ldg, ldg, self.DO.ld,
                                     None if self.WG is None else self.WG.ptr)
        dp = ctypes.addressof(self.desc)
        _lib.call("sdt_attention_fwd", self.Q.ptr, self.kptr, self.vptr, self.O.ptr, self.LSE.ptr, dp, _stream())
        ndelta, self.nslab = lib.sdt_attention_bwd_delta_bytes(dp), lib.sdt_attention_bwd_slab_bytes(dp)
        assert ndelta == kc.attention_delta_bytes(B, H, Nq) and (self.nslab > 0) == (self.plan[0] > 1), (self.what, ndelta, self.nslab)
        self.DELTA = Guarded(1, ndelta // 4, F32, dev, pad=0, back_rows=1)
        _lib.call("sdt_attention_bwd_dq", self.Q.ptr, self.kptr, self.vptr, self.O.ptr, self.DO.ptr, self.LSE.ptr, self.DQ.ptr, self.DELTA.ptr, dp, _stream())
        torch.cuda.synchronize()
        self.got = dict(o=self.O.t.contiguous().cpu().view(B, Nq, C), dq=self.DQ.t.contiguous().cpu().view(B, Nq, C))
        self.inline = self._inline()
        assert torch.equal(self.DQ.t.reshape(B, Nq, C), self.inline[0]), f"{self.what}: dq of the dQ pass alone differs from the inline call's"
        assert torch.equal(self.DELTA.t.reshape(-1)[: B * H * Nq], self.inline[3]), f"{self.what}: delta of the dQ pass alone differs from the inline call's"
        self.arm()

    def _inline(self):
        """sdt_attention_bwd of the same problem into plain tensors: (dq, dk, dv, delta)."""
        from stable_diffusion_training_amd import _lib
        B, H, Nq, Nk, D = self.spec[:5]
        C = H * D
        desc = _lib.SdtAttnDesc.from_buffer_copy(self.desc)
        desc.ldgrad_q = desc.ldgrad_k = desc.ldgrad_v = C
        dp = ctypes.addressof(desc)
        need = self.lib.sdt_attention_bwd_workspace_bytes(dp)
        assert need == kc.attention_delta_bytes(B, H, Nq) + self.nslab
        ws = torch.full((need // 4,), float("nan"), dtype=F32, device=self.dev)
        dq, dk, dv = (torch.empty(B, n, C, dtype=BF, device=self.dev) for n in (Nq, Nk, Nk))
        _lib.call("sdt_attention_bwd", self.Q.ptr, self.kptr, self.vptr, self.O.ptr, self.DO.ptr, self.LSE.ptr, dq.data_ptr(), dk.data_ptr(),
                  dv.data_ptr(), ws.data_ptr(), need, dp, _stream())
        torch.cuda.synchronize()
        return dq, dk, dv, ws[: B * H * Nq].clone()

    def arm(self):
        B, H, Nq, Nk, D, kind, packed = self.spec[:7]
        C = H * D
        if packed:  # dk | dv are the halves of one packed 2C gradient
            self.DKV = Guarded(B * Nk, 2 * C, BF, self.dev)
            self.grads = [self.DKV]
            self.dkptr, self.dvptr = self.DKV.ptr, self.DKV.ptr + 2 * C
            assert self.DKV.ld == self.desc.ldgrad_k
        else:
            self.DK, self.DV = Guarded(B * Nk, C, BF, self.dev), Guarded(B * Nk, C, BF, self.dev)
            self.grads = [self.DK, self.DV]
            self.dkptr, self.dvptr = self.DK.ptr, self.DV.ptr
            assert self.DK.ld == self.desc.ldgrad_k
        self.SLABS = Guarded(1, self.nslab // 4, F32, self.dev, pad=0, back_rows=1) if self.nslab else None

    def entry(self, slabs=True):
        from stable_diffusion_training_amd import _lib
        return _lib.SdtAttnDkvProblem(self.Q.ptr, self.kptr, self.vptr, self.DO.ptr, self.LSE.ptr, self.DELTA.ptr, self.dkptr, self.dvptr,
                                      self.SLABS.ptr if (slabs and self.SLABS is not None) else None, self.desc)

    def dk_dv(self):
        B, H, Nq, Nk, D, kind, packed = self.spec[:7]
        C = H * D
        halves = (self.DKV.t[:, :C], self.DKV.t[:, C:]) if packed else (self.DK.t, self.DV.t)
        return tuple(t.contiguous().view(B, Nk, C) for t in halves)

    def check(self, where):
        """Messages (empty: all well) on dk and dv after a grouped call: the expectation's bits, the inline call's, every guard."""
        B, H, Nq, Nk, D, kind = self.spec[:6]
        what = f"{where}, {self.what} (planned, chunk, launched, kblocks, gx = {self.plan})"
        dk, dv = self.dk_dv()
        got = dict(self.got, dk=dk.cpu(), dv=dv.cpu())
        if kind == "pair":
            msgs = pair_reports(got, self.want, D)
        else:
            msgs = [kc.mismatch_report(got[n], self.want[n], n, tile=(128, D)) for n in ("o", "dv")]
            for n in ("dq", "dk"):
                nz = (got[n] != 0) | torch.isnan(got[n])
                msgs.append(f"{n}: {int(nz.sum())} elements are not zero, first at {nz.nonzero()[0].tolist()}" if nz.any() else None)
        for n, g, ref in (("dk", dk, self.inline[1]), ("dv", dv, self.inline[2])):
            msgs.append(None if torch.equal(g, ref) else f"{n} differs from the inline sdt_attention_bwd in {int((kc.bits(g) != kc.bits(ref)).sum())} elements")
        arenas = [("q", self.Q), ("dout", self.DO), ("k", self.KG), ("v", self.VG), ("key_weight", self.WG), ("out", self.O), ("lse", self.LSE),
                  ("dq", self.DQ), ("delta", self.DELTA), ("slabs", self.SLABS)] + [("dk / dv", g) for g in self.grads]
        msgs += [g.guard_report(n) for n, g in arenas if g is not None]
        return [f"{what}: {m}" for m in msgs if m]


def _build(dev, lib, table):
    probs = [_Problem(dev, lib, spec) for spec in table]
    msgs = []
    for p in probs:  # the forward and the dQ pass, once per table
        if p.spec[5] == "pair":
            msgs += [f"{p.what}: {m}" for n in ("o", "dq") for m in [kc.mismatch_report(p.got[n], p.want[n], n, tile=(128, p.spec[4]))] if m]
    assert not msgs, "\n".join(msgs)
    return probs


def _run_group(probs, order, where):
    """One sdt_attention_bwd_dkv_group call over the problems in `order` (outputs and slabs armed afresh); every problem judged.
    Returns the (dk, dv) bits per problem, by table index."""
    from stable_diffusion_training_amd import _lib
    for p in probs:
        p.arm()
    arr = (_lib.SdtAttnDkvProblem * len(order))(*[probs[i].entry() for i in order])
    _lib.call("sdt_attention_bwd_dkv_group", arr, len(order), _stream())
    torch.cuda.synchronize()
    msgs = [m for i in order for m in probs[i].check(where)]
    assert not msgs, "\n".join(msgs[:12]) + (f"\n... {len(msgs)} messages" if len(msgs) > 12 else "")
    return {i: tuple(kc.bits(t).cpu() for t in probs[i].dk_dv()) for i in order}


@pytest.fixture(scope="module")
def mixed(dev, lib):
    return _build(dev, lib, kc.DKV_GROUP_MIXED)


def test_grouped_dkv_mixed_table_every_bit(dev, lib, mixed):
    """One call over 19 problems of all six instantiations: B and H differ inside a launch, unsplit problems with two and three key
    blocks, split ones with one and two, ragged query counts and chunks, packed halves, key weights, a causal problem, one key."""
    _run_group(mixed, list(range(len(mixed))), "table order")


def test_grouped_dkv_mixed_table_in_any_order(dev, lib, mixed):
    """Reversed and shuffled, every problem lands in another launch slot behind other neighbours: the same bits as in table order."""
    n = len(mixed)
    base = _run_group(mixed, list(range(n)), "table order")
    shuffled = list(range(n))
    random.Random(2024).shuffle(shuffled)
    assert shuffled != list(range(n)) and shuffled != list(range(n))[::-1]
    for name, order in (("reversed", list(range(n))[::-1]), ("shuffled", shuffled)):
        got = _run_group(mixed, order, name)
        for i in range(n):
            for j, t in enumerate(("dk", "dv")):
                assert torch.equal(got[i][j], base[i][j]), f"{name}: {t} of problem {mixed[i].spec} differs from its bits in table order"


def test_grouped_dkv_ten_split_problems_every_bit(dev, lib):
    """Nine split problems of one instantiation and one of another: a second dK/dV launch of the class, and two finishing launches
    whose tables are indexed differently from either; one problem launches fewer chunks than its slabs are sized for."""
    probs = _build(dev, lib, kc.DKV_GROUP_SPLITS)
    assert all(p.SLABS is not None for p in probs)
    _run_group(probs, list(range(len(probs))), "table order")


def test_grouped_dkv_full_table_every_bit(dev, lib):
    """sdt_attention_bwd_dkv_group_max() problems in one call: second launches in two classes."""
    assert len(kc.DKV_GROUP_FULL) == lib.sdt_attention_bwd_dkv_group_max()
    probs = _build(dev, lib, kc.DKV_GROUP_FULL)
    _run_group(probs, list(range(len(probs))), "table order")


def test_a_refused_dkv_table_launches_nothing(dev, lib, mixed):
    """Three problems, the last one a split problem without slabs: -1, the message names the slabs, and the first two problems' dk and
    dv arenas hold the sentinel in every element - the check of the last entry ran before the first launch."""
    from stable_diffusion_training_amd import _lib
    probs = [mixed[0], mixed[1], mixed[6]]
    assert probs[2].plan[0] > 1 and probs[0].plan[0] == probs[1].plan[0] == 1
    for p in probs:
        p.arm()
    arr = (_lib.SdtAttnDkvProblem * 3)(probs[0].entry(), probs[1].entry(), probs[2].entry(slabs=False))
    rc = lib.sdt_attention_bwd_dkv_group(arr, 3, _stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"problem 2" in lib.sdt_last_error() and b"slabs" in lib.sdt_last_error(), (rc, lib.sdt_last_error())
    for p in probs:
        for g in p.grads:
            assert _sentinel_everywhere(g), f"{p.what}: dk / dv were written by a refused call"


# ================================================================================================ sdt_colsum_batched_group
def _colsum_group(dev, lib, table, order):
    """The table's problems in `order` as one grouped call, three times on one guarded workspace of exactly the bytes the library asks
    for: counters zeroed once, partial rows poisoned before every launch."""
    from stable_diffusion_training_amd import _lib
    cases = []
    for i in order:
        N, ld, rows, batch, r = table[i]
        dy = exact_ints((batch * rows, N), -r, r, N + rows % 1000 + batch + i)
        DY = Guarded(batch * rows, N, BF, dev, data=dy, pad=ld - N)
        assert DY.ld == ld
        want = kc.rne_bf16(dy.to(dev).double().view(batch, rows, N).sum(1)).cpu()
        cases.append((table[i], DY, want))

    def entries(outs):
        return (_lib.SdtColsumProblem * len(cases))(*[_lib.SdtColsumProblem(DY.ptr, o.ptr, batch, rows, N, ld)
                                                      for ((N, ld, rows, batch, r), DY, _), o in zip(cases, outs)])

    outs = [Guarded(batch, N, BF, dev, pad=0) for (N, ld, rows, batch, r), _, _ in cases]
    need = lib.sdt_colsum_batched_group_workspace_bytes(entries(outs), len(cases))
    assert need == kc.colsum_group_workspace_bytes([c[0] for c in cases]) > kc.CNT_BYTES
    WS = Guarded(1, need, torch.int8, dev, pad=0, back_rows=0)
    WS.t[:, : kc.CNT_BYTES] = 0
    for run in range(3):
        WS.t[:, kc.CNT_BYTES:] = -1  # NaN patterns in every partial row; the counters are as the last launch left them
        if run:
            outs = [Guarded(batch, N, BF, dev, pad=0) for (N, ld, rows, batch, r), _, _ in cases]
        _lib.call("sdt_colsum_batched_group", entries(outs), len(cases), WS.ptr, need, _stream())
        torch.cuda.synchronize()
        msgs = []
        for j, (((N, ld, rows, batch, r), DY, want), o) in enumerate(zip(cases, outs)):
            what = f"run {run}, problem {j} (N, ld, rows, batch) = {(N, ld, rows, batch)}, plan (ncb, nby, rpb, want) = {kc.colsum_plan(batch, rows, N, 512)}"
            msgs += [kc.mismatch_report(o.t.cpu(), want, what + ": out [batch][column]"), o.guard_report(what + ": out")]
        msgs.append(kc.counters_report(WS.t.reshape(-1), f"run {run}: workspace"))
        msgs.append(WS.guard_report(f"run {run}: workspace"))
        msgs = [m for m in msgs if m]
        assert not msgs, "\n".join(msgs[:12])
    for _, DY, _ in cases:
        DY.check("dy")


def test_grouped_column_sums_of_the_single_launch_cases_exact(dev, lib):
    """kernel_checks.COLSUM_CASES as one call: the planner's want clamp, ragged last row blocks, N % 8, ld > N with NaN in the pad
    columns, and small problems whose counters and partial rows lie behind those of a problem with hundreds of row blocks."""
    _colsum_group(dev, lib, kc.COLSUM_CASES, list(range(len(kc.COLSUM_CASES))))


@pytest.mark.parametrize("order", ["table", "shuffled"])
def test_grouped_column_sums_at_the_problem_limit_exact(dev, lib, order):
    idx = list(range(len(kc.COLSUM_GROUP_MAXED)))
    assert len(idx) == lib.sdt_colsum_batched_group_max()
    if order == "shuffled":
        random.Random(7).shuffle(idx)
        assert idx != sorted(idx)
    _colsum_group(dev, lib, kc.COLSUM_GROUP_MAXED, idx)
