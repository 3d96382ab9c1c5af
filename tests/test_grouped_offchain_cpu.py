"""The queue-and-flush logic behind ops.wgrad_grouping(offchain=True), on the CPU: the kernel launches are replaced by a stub that
records their names, so only the ORDER of the calls is under test - the deferred column sums (and dK/dV passes, which share the
flush) must be issued before their one reader, _ColSlices.backward, gathers the slices' gradients, and a queue that is still
filled when the context closes must be issued there.  The second half fills either queue beyond one table (33 entries: launches of
32 and 1, the queued tensors alive until then and no longer) and holds the grouped entry points to their documented refusals and
workspace size on host buffers: every check returns before a launch."""
import pytest
import torch

from stable_diffusion_training_amd import ops

BF = torch.bfloat16


@pytest.fixture
def calls(lib, monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *a: seen.append(name))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return seen


class _RowBiasUser(torch.autograd.Function):
    """What _Conv2d does with its row bias: counts the use of the slice in forward, queues the column sum in backward."""

    @staticmethod
    def forward(ctx, rb):
        ctx.tag = ops._slice_tag(rb)
        return rb.float().sum()

    @staticmethod
    def backward(ctx, g):
        drb = torch.zeros(2, 8, dtype=BF)
        if ops._deferrable(ctx.tag):
            ops.defer_colsum(torch.zeros(2 * 16, 8, dtype=BF), drb, 2, 16, 8, 8)
            ops._note_deferred(ctx.tag, drb)
        else:
            ops.call("sdt_colsum_batched_bf16")
        return drb


def _slices(n=2):
    y = torch.zeros(2, n * 8, dtype=BF, requires_grad=True)
    return y, ops.col_slices(y, n)


def test_the_reader_of_the_slices_flushes_first(calls):
    y, (a, b) = _slices()
    with ops.wgrad_grouping():
        (_RowBiasUser.apply(a) + _RowBiasUser.apply(b)).backward()
        assert calls == ["sdt_colsum_batched_group", "sdt_copy_cols_bf16"], calls  # ONE launch for both, in front of the gather
        assert not ops._COLSUM_QUEUE
    assert calls == ["sdt_colsum_batched_group", "sdt_copy_cols_bf16"]  # nothing left for the closing context
    assert y.grad is not None


def test_closing_the_context_flushes_what_is_left(calls):
    with ops.wgrad_grouping():
        ops.defer_colsum(torch.zeros(32, 8, dtype=BF), torch.zeros(2, 8, dtype=BF), 2, 16, 8, 8)
        assert calls == [] and len(ops._COLSUM_QUEUE) == 1
    assert calls == ["sdt_colsum_batched_group"] and not ops._COLSUM_QUEUE


def test_nothing_is_deferred_outside_the_context_or_with_the_switch_off(calls):
    y, (a, b) = _slices()
    (_RowBiasUser.apply(a) + _RowBiasUser.apply(b)).backward()
    assert calls == ["sdt_colsum_batched_bf16"] * 2 + ["sdt_copy_cols_bf16"]
    del calls[:]
    y, (a, b) = _slices()
    with ops.wgrad_grouping(offchain=False):
        (_RowBiasUser.apply(a) + _RowBiasUser.apply(b)).backward()
    assert calls == ["sdt_colsum_batched_bf16"] * 2 + ["sdt_copy_cols_bf16"]


def test_a_slice_with_two_users_or_a_plain_tensor_is_not_deferred(calls):
    y, (a, b) = _slices()
    with ops.wgrad_grouping():
        (_RowBiasUser.apply(a) + _RowBiasUser.apply(a)).backward()  # autograd adds the two gradients of `a`: both must be written
        assert calls[:2] == ["sdt_colsum_batched_bf16"] * 2 and "sdt_colsum_batched_group" not in calls
        del calls[:]
        t = torch.zeros(2, 8, dtype=BF, requires_grad=True)
        _RowBiasUser.apply(t).backward()
        assert calls == ["sdt_colsum_batched_bf16"]


def test_group_calls_validate_their_tables_without_a_gpu(lib):
    from stable_diffusion_training_amd import _lib
    assert lib.sdt_attention_bwd_dkv_group(None, 0, None) == -1 and b"problems" in lib.sdt_last_error()
    assert lib.sdt_colsum_batched_group(None, 0, None, 0, None) == -1 and b"bad args" in lib.sdt_last_error()
    # the grouped workspace is the counters plus every problem's own partial rows: the single launches' partitions, back to back
    shapes = [(2, 64, 64), (2, 256, 320), (1, 16, 8)]
    dy = torch.zeros(2 * 256 * 320, dtype=BF)
    out = torch.zeros(2 * 320, dtype=BF)
    arr = (_lib.SdtColsumProblem * 3)(*[_lib.SdtColsumProblem(dy.data_ptr(), out.data_ptr(), b, r, n, n) for b, r, n in shapes])
    single = [lib.sdt_colsum_workspace_bytes(b, r, n) for b, r, n in shapes]
    assert all(s > 65536 for s in single)
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, 3) <= 65536 + sum(s - 65536 for s in single)
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, 3) > 65536
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, lib.sdt_colsum_batched_group_max() + 1) == 0
    # the split of the inline workspace into its two parts
    for nq in (512, 1024):
        d = _lib.SdtAttnDesc(2, 2, nq, 77, 40, 80, 80, 80, 80, 0.1, 0, 0, 0, 0, 0, None)
        p = _lib.ctypes.addressof(d)
        assert lib.sdt_attention_bwd_delta_bytes(p) == 2 * 2 * nq * 4
        assert (lib.sdt_attention_bwd_slab_bytes(p) > 0) == (nq >= 1024)
        assert lib.sdt_attention_bwd_workspace_bytes(p) == lib.sdt_attention_bwd_delta_bytes(p) + lib.sdt_attention_bwd_slab_bytes(p)


def test_an_exception_drops_the_queues(calls):
    with pytest.raises(RuntimeError):
        with ops.wgrad_grouping():
            ops.defer_colsum(torch.zeros(32, 8, dtype=BF), torch.zeros(2, 8, dtype=BF), 2, 16, 8, 8)
            raise RuntimeError("backward failed")
    assert calls == [] and not ops._COLSUM_QUEUE and not ops._DKV_QUEUE


def test_a_second_consumer_that_does_not_count_itself_is_refused(calls):
    """A slice whose gradient was deferred also feeds a plain torch operator: autograd adds the two gradients before the deferred one is
    written.  _ColSlices.backward must refuse the sum instead of gathering it."""
    from stable_diffusion_training_amd import _lib
    y, (a, b) = _slices()
    with pytest.raises(_lib.SdtError, match="second consumer"):
        with ops.wgrad_grouping():
            (_RowBiasUser.apply(a) + a.float().sum() + _RowBiasUser.apply(b)).backward()


# ------------------------------------------------------------------------------------------------ the queues beyond one table
@pytest.fixture
def launches(lib, monkeypatch):
    """As `calls`, with the problem count of every grouped launch: (name, n), n = None for the other calls."""
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *a: seen.append((name, a[1] if name.endswith("_group") else None)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    return seen


def test_more_column_sums_than_one_table_holds_flush_as_two_launches(launches, lib):
    step = lib.sdt_colsum_batched_group_max()
    assert step == 32
    with ops.wgrad_grouping():
        for _ in range(step + 1):
            ops.defer_colsum(torch.zeros(32, 8, dtype=BF), torch.zeros(2, 8, dtype=BF), 2, 16, 8, 8)
        assert launches == [] and len(ops._COLSUM_QUEUE) == step + 1
    assert launches == [("sdt_colsum_batched_group", step), ("sdt_colsum_batched_group", 1)]
    assert not ops._COLSUM_QUEUE and not ops._DKV_QUEUE


def test_more_dkv_passes_than_one_table_holds_flush_as_two_launches_and_keep_their_tensors(launches, lib):
    """33 deferred backward passes on CPU tensors (the byte queries are host code): 33 dQ passes at once, then two grouped launches of
    32 and 1.  Until the flush the queue alone keeps every entry's dout, lse, delta and slabs alive; afterwards nothing does."""
    import gc
    import weakref
    from stable_diffusion_training_amd import _lib
    step = lib.sdt_attention_bwd_dkv_group_max()
    assert step == 32
    B, H, Nk, D = 1, 2, 77, 40
    C = H * D
    refs, with_slabs = [], 0
    with ops.wgrad_grouping():
        for i in range(step + 1):
            Nq = 1024 if i % 3 == 0 else 64  # (every third problem plans a query split: slabs)
            desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, C, 2 * C, 2 * C, C, D ** -0.5, 0, C, 2 * C, 2 * C, 0, None)
            q, out, dout, dq = (torch.zeros(B, Nq, C, dtype=BF) for _ in range(4))
            kv, dkv = torch.zeros(B, Nk, 2 * C, dtype=BF), torch.zeros(B, Nk, 2 * C, dtype=BF)
            lse = torch.zeros(B, H, Nq)
            ops._attention_bwd_deferred(desc, q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * C, out, dout, lse, dq.data_ptr(), dkv.data_ptr(),
                                        dkv.data_ptr() + 2 * C, (q, kv, dkv, None))
            prob, keep = ops._DKV_QUEUE[-1]
            delta, slabs = keep[2], keep[3]
            assert keep[0] is dout and keep[1] is lse and prob.delta == delta.data_ptr() and delta.numel() == B * H * Nq
            assert (slabs is not None) == (Nq == 1024) and prob.slabs == (slabs.data_ptr() if slabs is not None else None)
            assert prob.dout == dout.data_ptr() and prob.lse == lse.data_ptr() and prob.dk == dkv.data_ptr() and prob.dv == dkv.data_ptr() + 2 * C
            with_slabs += slabs is not None
            refs.append([weakref.ref(t) for t in (dout, lse, delta, slabs, dkv) if t is not None])
            del q, out, dout, dq, kv, dkv, lse, delta, slabs, keep, prob
        gc.collect()
        assert with_slabs == 11 and len(ops._DKV_QUEUE) == step + 1
        assert all(r() is not None for rs in refs for r in rs), "a queued tensor was freed before the flush"
        assert launches == [("sdt_attention_bwd_dq", None)] * (step + 1)
    assert launches[step + 1:] == [("sdt_attention_bwd_dkv_group", step), ("sdt_attention_bwd_dkv_group", 1)]
    assert not ops._DKV_QUEUE and not ops._COLSUM_QUEUE
    gc.collect()
    assert all(r() is None for rs in refs for r in rs), "the flushed queue still holds tensors"


def _dkv_entry(bufs, Nq=64, dk_off=0, ldg=None, slabs=None):
    """One well-formed table entry on host buffers (the checks under test run before any launch)."""
    from stable_diffusion_training_amd import _lib
    B, H, Nk, D = 1, 2, 77, 40
    C = H * D
    desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, C, C, C, C, D ** -0.5, 0, C, C if ldg is None else ldg, C if ldg is None else ldg, C, None)
    p = bufs.data_ptr()
    return _lib.SdtAttnDkvProblem(p, p, p, p, p, p, p + dk_off, p, slabs, desc)


def test_grouped_dkv_refuses_bad_tables_without_a_gpu(lib):
    from stable_diffusion_training_amd import _lib
    bufs = torch.zeros(1 << 16, dtype=torch.uint8)
    assert bufs.data_ptr() % 16 == 0
    n = lib.sdt_attention_bwd_dkv_group_max()
    arr = (_lib.SdtAttnDkvProblem * (n + 1))(*[_dkv_entry(bufs) for _ in range(n + 1)])
    assert lib.sdt_attention_bwd_dkv_group(arr, n + 1, None) == -1 and b"1..32 problems" in lib.sdt_last_error()
    arr = (_lib.SdtAttnDkvProblem * 2)(_dkv_entry(bufs), _dkv_entry(bufs, dk_off=8))
    assert lib.sdt_attention_bwd_dkv_group(arr, 2, None) == -1 and b"problem 1: pointers must be 16-byte aligned" in lib.sdt_last_error()
    arr = (_lib.SdtAttnDkvProblem * 2)(_dkv_entry(bufs), _dkv_entry(bufs, ldg=84))
    assert lib.sdt_attention_bwd_dkv_group(arr, 2, None) == -1 and b"problem 1: row strides must be multiples of 8" in lib.sdt_last_error()
    arr = (_lib.SdtAttnDkvProblem * 3)(_dkv_entry(bufs), _dkv_entry(bufs), _dkv_entry(bufs, Nq=1024))
    assert lib.sdt_attention_bwd_dkv_group(arr, 3, None) == -1 and b"problem 2: slabs" in lib.sdt_last_error()


def _colsum_entries(table, ptr):
    from stable_diffusion_training_amd import _lib
    return (_lib.SdtColsumProblem * len(table))(*[_lib.SdtColsumProblem(ptr, ptr, batch, rows, N, ld) for N, ld, rows, batch, r in table])


def test_grouped_column_sum_workspace_and_refusals_without_a_gpu(lib):
    from tests import kernel_checks as kc
    bufs = torch.zeros(1 << 12, dtype=torch.uint8)
    ptr = bufs.data_ptr()
    assert ptr % 16 == 0
    for table in (kc.COLSUM_CASES, kc.COLSUM_GROUP_MAXED):
        arr = _colsum_entries(table, ptr)
        need = lib.sdt_colsum_batched_group_workspace_bytes(arr, len(table))
        assert need == kc.colsum_group_workspace_bytes(table) == 65536 + 4 * sum(
            ncb * batch * nby * 256 for (N, ld, rows, batch, r) in table for ncb, nby, rpb, want in [kc.colsum_plan(batch, rows, N, 512)])
        # every check runs before the launch: a short workspace is refused on any machine
        assert lib.sdt_colsum_batched_group(arr, len(table), ptr, need - 16, None) == -1 and b"workspace" in lib.sdt_last_error()
    n = lib.sdt_colsum_batched_group_max()
    table = kc.COLSUM_GROUP_MAXED + kc.COLSUM_GROUP_MAXED[:1]
    assert len(table) == n + 1
    arr = _colsum_entries(table, ptr)
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, n) > 65536 and lib.sdt_colsum_batched_group_workspace_bytes(arr, n + 1) == 0
    assert lib.sdt_colsum_batched_group(arr, n + 1, ptr, 1 << 30, None) == -1 and b"bad args" in lib.sdt_last_error()
    # 2 x 8200 arrival counters: each problem alone fits the 64 KiB counter area, the table does not
    big = (512, 512, 1, 4100, 1)
    assert lib.sdt_colsum_workspace_bytes(4100, 1, 512) == 65536 + 2 * 4100 * 256 * 4 and 2 * 4100 * 4 <= 65536 < 2 * 2 * 4100 * 4
    arr = _colsum_entries([big, big], ptr)
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, 1) == lib.sdt_colsum_workspace_bytes(4100, 1, 512)
    assert lib.sdt_colsum_batched_group_workspace_bytes(arr, 2) == 0
    assert lib.sdt_colsum_batched_group(arr, 2, ptr, 1 << 30, None) == -1 and b"bad args" in lib.sdt_last_error()
