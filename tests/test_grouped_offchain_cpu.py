"""The queue-and-flush logic behind ops.wgrad_grouping(offchain=True), on the CPU: the kernel launches are replaced by a stub that
records their names, so only the ORDER of the calls is under test - the deferred column sums (and dK/dV passes, which share the
flush) must be issued before their one reader, _ColSlices.backward, gathers the slices' gradients, and a queue that is still
filled when the context closes must be issued there."""
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
