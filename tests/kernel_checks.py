"""Element-wise checkers for the kernel tests (tests/test_gpu_kernel_exact.py; proved on the CPU by tests/test_kernel_checks_cpu.py).

The contraction kernels are "bf16 in, fp32 accumulate, round once per documented rounding point".  With small-integer operands
every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact in any order, tiling or split, and the
result is unique: the fp32 accumulator equals the float64 reference and the bf16 output is its RNE rounding, bit for bit.  This
module holds the operand generators, the expectations (float64 reference followed by the kernels' rounding points), the bitwise
comparison with a report that names the tile edge, guarded allocations, per-slice error norms, and the case tables that the GPU
file and the CPU proof share.  Attention gets two exact constructions: selector inputs (P one-hot: a gather, dQ = dK = 0) and
tied pairs (P = 1/2, 1/2: exact nonzero dQ and dK), at every head dim the ABI accepts.

The second half serves tests/test_gpu_reduce_optim_exact.py: exact scalar sums with a report that names the missing partial, tail
element or overwritten destination, mirrors of the reduction launchers' partitions, the optimizer references (oracle/lion8.py itself),
the posterior-sample and timestep-embedding bounds, and the case tables with the bound that makes each of them exact.

The last part serves tests/test_gpu_norm_exact.py: balanced norm inputs whose float64 result is exactly representable, the expectation
with the assertions that make it unique, a mirror of the GroupNorm launch geometry for failure reports, and the case tables.

The end serves tests/test_gpu_grouped_exact.py: the problem tables of the grouped dK/dV and column-sum launches, mirrors of their
launch lists, workgroup decode and workspace, and the per-problem expectations."""
import functools
import math

import numpy as np
import torch

from oracle import lion8 as LION_ORACLE  # the float32 restatement of lion_quant.py the project trusts: the ONLY optimizer reference

BF = torch.bfloat16
LIMIT = 1 << 24  # integers up to here are exact in fp32

_INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64,
             torch.int8: torch.int8, torch.int32: torch.int32}
# what an untouched output element holds: NaN patterns for the float types, so that an element the kernel never wrote also fails
# the value comparison
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.float64: 0x7FF5A5A5A5A5A5A5, torch.int8: 0x5A, torch.int32: 0x5A5A5A5A}


def bits(t):
    """The integer view of a tensor's bit patterns."""
    return t.contiguous().view(_INT_VIEW[t.dtype])


# ------------------------------------------------------------------------------------------------ operands
def exact_ints(shape, lo, hi, seed, dtype=BF, device="cpu"):
    """Seeded integers in [lo, hi], exactly representable in bf16 (|v| <= 256)."""
    assert -256 <= lo <= hi <= 256
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype).to(device)


def rne_bf16(x64):
    """RNE rounding of float64 values that fp32 holds exactly (integers below 2^24): fp32 -> bf16 is torch's RNE cast."""
    x32 = x64.to(torch.float32)
    assert torch.equal(x32.double(), x64), "value not exact in fp32: the expectation would round twice"
    return x32.to(BF)


def abs_sum_bound(a_absmax, b_absmax, terms):
    return a_absmax * b_absmax * terms


# ------------------------------------------------------------------------------------------------ expectations
def epilogue_nt(acc64, bias=None, rowbias=None, residual=None, rows_per_batch=0):
    """The rounding points of the sdt_gemm_nt_bf16 epilogues, in order (gemm.hip gemm_nt_kernel "---- epilogue", lines 695-767,
    and conv3x3_halo_kernel's, lines 1066-1111):
      1. v = acc (+ bias[n], fp32) -> bf16 (pack2bf into the LDS C tile, gemm.hip:707-715 / 1081-1088);
      2. only with a row bias or a residual: widen, (+ rowbias[m / rows_per_batch][n]) (+ residual[m][n]) in fp32 -> bf16
         (gemm.hip:752-765 / 1102-1115).
    With integer operands both sums are exact, so the result is unique."""
    v = acc64 if bias is None else acc64 + bias.double()[None, :]
    v = rne_bf16(v)
    if rowbias is None and residual is None:
        return v
    f = v.double()
    if rowbias is not None:
        f = f + rowbias.double().repeat_interleave(rows_per_batch, 0)[: f.shape[0]]
    if residual is not None:
        f = f + residual.double()
    return rne_bf16(f)


def expect_gemm_nt(a, b, bias=None, rowbias=None, residual=None, rows_per_batch=0):
    """a [M][K], b [K][N] (any dtype, integer valued) -> the bf16 output sdt_gemm_nt_bf16 must produce, bit for bit."""
    return epilogue_nt(a.double() @ b.double(), bias, rowbias, residual, rows_per_batch)


def conv_ref64(x, w, stride, pad):
    """float64 NHWC convolution as one matrix product per tap: x (B,H,W,Cin), w (kh,kw,Cin,Cout) HWIO, pad ((top, bottom),
    (left, right)).  The same operation as F.conv2d (the CPU proof compares the two); written with matmul so that it runs in
    float64 on any device."""
    (pt, pb), (pl, pr) = pad
    B, H, W, Cin = x.shape
    kh, kw, _, Cout = w.shape
    OH, OW = (H + pt + pb - kh) // stride + 1, (W + pl + pr - kw) // stride + 1
    xp = torch.nn.functional.pad(x.double(), (0, 0, pl, pr, pt, pb))
    y = torch.zeros(B * OH * OW, Cout, dtype=torch.float64, device=x.device)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i: i + stride * (OH - 1) + 1: stride, j: j + stride * (OW - 1) + 1: stride, :]
            y = y + xs.reshape(-1, Cin) @ w[i, j].double()
    return y.view(B, OH, OW, Cout)


def conv_dgrad_ref64(dy, w, in_hw, stride, pad):
    """float64 input gradient of conv_ref64: dx (B,H,W,Cin) from dy (B,OH,OW,Cout)."""
    (pt, pb), (pl, pr) = pad
    B, OH, OW, Cout = dy.shape
    kh, kw, Cin, _ = w.shape
    H, W = in_hw
    dxp = torch.zeros(B, H + pt + pb, W + pl + pr, Cin, dtype=torch.float64, device=dy.device)
    for i in range(kh):
        for j in range(kw):
            t = (dy.double().reshape(-1, Cout) @ w[i, j].double().t()).view(B, OH, OW, Cin)
            dxp[:, i: i + stride * (OH - 1) + 1: stride, j: j + stride * (OW - 1) + 1: stride, :] += t
    return dxp[:, pt: pt + H, pl: pl + W, :]


def conv_wgrad_ref64(x, dy, khw, stride, pad):
    """float64 weight gradient of conv_ref64: dW (kh,kw,Cin,Cout)."""
    (pt, pb), (pl, pr) = pad
    kh, kw = khw
    B, OH, OW, Cout = dy.shape
    Cin = x.shape[-1]
    xp = torch.nn.functional.pad(x.double(), (0, 0, pl, pr, pt, pb))
    out = torch.empty(kh, kw, Cin, Cout, dtype=torch.float64, device=x.device)
    for i in range(kh):
        for j in range(kw):
            xs = xp[:, i: i + stride * (OH - 1) + 1: stride, j: j + stride * (OW - 1) + 1: stride, :]
            out[i, j] = xs.reshape(-1, Cin).t() @ dy.double().reshape(-1, Cout)
    return out


def expect_gn_parts(y, rows_of_tile, groups, tile_cols):
    """The partial statistics rows include/sdt.h:231-236 assigns to the epilogues, from the stored bf16 output y [rows][N] of ONE
    image: rows_of_tile is a list (one entry per output row tile r, in the kernel's tile order) of row-index tensors.  Row 2r takes,
    for every group, the columns of the group that lie in the column tile the group STARTS in; row 2r+1 takes the columns that lie
    in the next column tile (a group is at most one tile wide); slots nobody contributes to are written as zero.
    Returns float64 [2 * len(rows_of_tile)][groups][2] = {sum, sum of squares}."""
    N = y.shape[1]
    cpg = N // groups
    out = torch.zeros(2 * len(rows_of_tile), groups, 2, dtype=torch.float64)
    yd = y.double().cpu()
    for r, rows in enumerate(rows_of_tile):
        blk = yd[rows.cpu()]
        for g in range(groups):
            lo, hi = g * cpg, (g + 1) * cpg
            cut = min(hi, (lo // tile_cols + 1) * tile_cols)
            for side, (a, b) in enumerate(((lo, cut), (cut, hi))):
                if a < b:
                    out[2 * r + side, g, 0] = blk[:, a:b].sum()
                    out[2 * r + side, g, 1] = (blk[:, a:b] ** 2).sum()
    return out


def gn_dense_operands(M, N, Kc):
    """a [M][Kc], b [Kc][N] in -1..1 and an fp32 bias in -1..1: the operands of the GroupNorm-statistics cases."""
    return exact_ints((M, Kc), -1, 1, 11), exact_ints((Kc, N), -1, 1, 12), exact_ints((N,), -1, 1, 13, dtype=torch.float32)


def gn_halo_operands(B, H, W, Cin, Cout):
    return exact_ints((B, H, W, Cin), -1, 1, 21), exact_ints((3, 3, Cin, Cout), -1, 1, 22), exact_ints((Cout,), -1, 1, 23, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ comparison
def _coords(flat_idx, shape):
    return [tuple(int(v) for v in c) for c in torch.stack(torch.unravel_index(flat_idx, shape), -1).tolist()]


def mismatch_report(got, want, what, tile=None, limit=6):
    """None when got and want hold the same bits; otherwise a message: the count, the first coordinates with both values, the
    bounding box, and (tile = (rows, cols) of an output tile over the last two dimensions flattened to [rows][cols]) which
    tiles and which rows / columns inside a tile the mismatches fall on."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    bad = bits(got) != bits(want)
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.reshape(-1).nonzero().reshape(-1).cpu()
    shape = tuple(got.shape)
    first = _coords(idx[:limit], shape)
    gc, wc = got.reshape(-1).cpu(), want.reshape(-1).cpu()
    lines = [f"{what}: {n} of {got.numel()} elements differ"]
    for c, i in zip(first, idx[:limit].tolist()):
        lines.append(f"  at {c}: got {gc[i].item()!r} (0x{int(bits(gc[i:i + 1])[0]) & ((1 << (8 * got.element_size())) - 1):x}), want {wc[i].item()!r}")
    allc = torch.stack(torch.unravel_index(idx, shape), -1)
    lines.append(f"  bounding box: {tuple(int(v) for v in allc.min(0).values)} .. {tuple(int(v) for v in allc.max(0).values)}")
    if tile is not None:
        cols = shape[-1]
        r, c = idx // cols, idx % cols
        tr, tc = tile
        tiles = sorted({(int(a), int(b)) for a, b in zip((r // tr).tolist(), (c // tc).tolist())})
        lines.append(f"  output tiles ({tr} x {tc}) hit: {tiles[:8]}{' ...' if len(tiles) > 8 else ''} ({len(tiles)} tiles)")
        lines.append(f"  rows inside a tile: {sorted(set((r % tr).tolist()))[:16]}; columns inside a tile: {sorted(set((c % tc).tolist()))[:16]}")
    return "\n".join(lines)


def assert_equal_bits(got, want, what, tile=None):
    msg = mismatch_report(got, want, what, tile)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ guarded allocations
class Guarded:
    """A payload [rows][ld], ld = width + pad (pad = 16 elements unless the ABI has no pitch for this operand: pad = 0), inside one
    arena: front guard >= 4 KiB, back guard >= 128 rows of ld elements (one full tile of rows).  Base pointers are 16-byte aligned.
    Outputs (data = None): every element holds SENTINEL; check() asserts afterwards that every guard element still does.
    Inputs (data given): the guards hold `guard` (NaN: an out-of-range element that reaches the arithmetic surfaces in the
    result) and check() asserts that the call left the whole arena alone."""

    def __init__(self, rows, width, dtype, device, data=None, guard=float("nan"), pad=16, back_rows=128):
        self.rows, self.width, self.ld, self.dtype = rows, width, width + pad, dtype
        es = torch.empty(0, dtype=dtype).element_size()
        self.front = -(-4096 // es)
        while (self.front * es) % 16:
            self.front += 1
        back = max(back_rows * self.ld, self.front)
        self.arena = torch.empty(self.front + rows * self.ld + back, dtype=dtype, device=device)
        self.is_input = data is not None
        if self.is_input:
            if dtype.is_floating_point:
                self.arena.fill_(guard)
            else:
                self.arena.fill_(int(guard))
            self.t.copy_(data.reshape(rows, width).to(dtype))
            self.before = self.arena.clone()
        else:
            s = SENTINEL[dtype]
            iv = _INT_VIEW[dtype]
            top = 1 << (8 * es)
            self.arena.view(iv).fill_(s - top if s >= top // 2 else s)
        assert self.ptr % 16 == 0

    @property
    def t(self):
        """The payload as a strided [rows][width] view."""
        return self.arena[self.front: self.front + self.rows * self.ld].view(self.rows, self.ld)[:, : self.width]

    @property
    def ptr(self):
        return self.arena.data_ptr() + self.front * self.arena.element_size()

    def guard_report(self, what):
        """None, or a message naming where the arena outside the payload (inputs: anywhere) was changed."""
        if self.is_input:
            bad = bits(self.arena) != bits(self.before)
        else:
            ref = torch.empty_like(self.arena)
            s = SENTINEL[self.dtype]
            top = 1 << (8 * self.arena.element_size())
            ref.view(_INT_VIEW[self.dtype]).fill_(s - top if s >= top // 2 else s)
            bad = bits(self.arena) != bits(ref)
            bad[self.front: self.front + self.rows * self.ld].view(self.rows, self.ld)[:, : self.width] = False
        n = int(bad.sum())
        if n == 0:
            return None
        idx = bad.nonzero().reshape(-1).cpu().tolist()
        where = []
        for i in idx[:6]:
            if i < self.front:
                where.append(f"front guard, {self.front - i} elements before the base")
            elif i >= self.front + self.rows * self.ld:
                j = i - self.front - self.rows * self.ld
                where.append(f"back guard, row {self.rows + j // self.ld} column {j % self.ld}")
            else:
                j = i - self.front
                where.append(f"{'payload' if j % self.ld < self.width else 'pad'} row {j // self.ld} column {j % self.ld}")
        return f"{what}: {n} guarded elements changed ({'input' if self.is_input else 'output'} arena, ld {self.ld}, width {self.width}): " + "; ".join(where)

    def check(self, what):
        msg = self.guard_report(what)
        assert msg is None, msg


# ------------------------------------------------------------------------------------------------ per-slice norms
def per_slice_rel(got, ref, dims, mag=None):
    """Relative L2 error of every slice: the norm runs over `dims`, one figure per index of the remaining dimensions.
    mag (optional, same shape): per element, the sum of the magnitudes of the terms the reference value is the sum of.  The
    denominator is then max(||ref||, 2^-9 ||mag||) over the slice: a slice computed from bf16-rounded factors carries an absolute
    error of the order of one bf16 rounding (2^-9) of its terms whatever the terms add up to, so where the reference has
    cancelled below that (exactly zero for query 0 of a causal problem) "relative to the reference" is not defined by the
    arithmetic and the error is measured against the rounding of the terms instead."""
    g, r = got.double(), ref.double()
    num = ((g - r) ** 2).sum(dims).sqrt()
    den = (r ** 2).sum(dims).sqrt()
    if mag is not None:
        den = torch.maximum(den, 2.0 ** -9 * (mag.double() ** 2).sum(dims).sqrt())
    return num / den.clamp_min(1e-300)


def floor_binds(ref, dims, mag):
    """Per slice: whether per_slice_rel measures against the floor 2^-9 ||mag|| instead of ||ref||."""
    return (ref.double() ** 2).sum(dims).sqrt() < 2.0 ** -9 * (mag.double() ** 2).sum(dims).sqrt()


def worst_slices(rel, k=3):
    """[(index tuple, error)] of the k worst slices of a per_slice_rel result."""
    flat = rel.reshape(-1)
    v, i = flat.topk(min(k, flat.numel()))
    return [(c, float(e)) for c, e in zip(_coords(i.cpu(), tuple(rel.shape)), v.tolist())]


# The per-slice rules (attention rows, norm slices, norm parameter-gradient channels): kernel worst slice <= ROW_FACTOR x the worst
# slice of the rounding-point emulation (what the emulation leaves out: attention_ref_and_emulation)
ROW_FACTOR = 3.0


# ------------------------------------------------------------------------------------------------ selector attention
def selector_case(B, H, Nq, Nk, D, causal, seed, c=32.0, vmax=8, domax=3):
    """Inputs whose attention is exactly a gather.  Key j of (b, h) carries the code c * (+-1 per bit of s(j)) on the first
    ceil(log2 Nk) head dimensions (s a seeded permutation), query i the code of its target key t(i): the matching key beats every
    other by at least 2 c^2 / sqrt(D) logits, every other probability underflows to 0 in fp32, P is one-hot.  Non-causal:
    t(i) = p(i mod Nk) for a seeded permutation p; causal: t(i) seeded in [0, i], the diagonal included (t(0) = 0).
    Returns dict(q, k, v, dout: bf16 (B, N, H*D); target: int64 (B, H, Nq); nbits)."""
    nb = max(1, math.ceil(math.log2(max(Nk, 2))))
    assert nb <= D
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, Nq, H, D)
    k = torch.zeros(B, Nk, H, D)
    target = torch.empty(B, H, Nq, dtype=torch.int64)
    sh = torch.arange(nb)
    for b in range(B):
        for h in range(H):
            s = torch.randperm(Nk, generator=g)
            if causal:
                t = (torch.rand(Nq, generator=g) * (torch.arange(Nq).clamp_max(Nk - 1) + 1)).long().clamp_max(Nk - 1)
                t = torch.minimum(t, torch.arange(Nq).clamp_max(Nk - 1))
                if Nq > 1:
                    t[Nq - 1] = min(Nq, Nk) - 1  # the diagonal itself at least once
            else:
                t = torch.randperm(Nk, generator=g)[torch.arange(Nq) % Nk]
            target[b, h] = t
            k[b, :, h, :nb] = (((s[:, None] >> sh) & 1) * 2 - 1).float() * c
            q[b, :, h, :nb] = (((s[t][:, None] >> sh) & 1) * 2 - 1).float() * c
    v = torch.randint(-vmax, vmax + 1, (B, Nk, H * D), generator=g).float()
    do = torch.randint(-domax, domax + 1, (B, Nq, H * D), generator=g).float()
    return dict(q=q.reshape(B, Nq, H * D).to(BF), k=k.reshape(B, Nk, H * D).to(BF), v=v.to(BF), dout=do.to(BF), target=target, nbits=nb, c=c)


def selector_expect(case, B, H, Nq, Nk, D, scale, key_weight=None):
    """out (bf16), lse2 (float64, log2 domain: attention.hip:8-9), dv (bf16) of a selector case; dq and dk are zero by value."""
    t = case["target"]
    v4 = case["v"].view(B, Nk, H, D)
    do4 = case["dout"].view(B, Nq, H, D).double()
    out = torch.empty(B, Nq, H, D, dtype=BF)
    dv = torch.zeros(B, Nk, H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            out[b, :, h] = v4[b, t[b, h], h]
            dv[b, :, h].index_add_(0, t[b, h], do4[b, :, h])
    logit = case["nbits"] * case["c"] ** 2 * float(torch.tensor(scale, dtype=torch.float32))
    lse2 = torch.full((B, H, Nq), logit * 1.4426950408889634, dtype=torch.float64)
    if key_weight is not None:
        lse2 = lse2 + torch.log2(key_weight.double().cpu())[t]
    return out.reshape(B, Nq, H * D), lse2, rne_bf16(dv).reshape(B, Nk, H * D)


def selector_min_gap(case, B, H, Nq, Nk, D, scale):
    """Smallest logit gap between the target key and the runner-up, and the largest logit (float64)."""
    q4, k4 = case["q"].view(B, Nq, H, D).double(), case["k"].view(B, Nk, H, D).double()
    gap, top = float("inf"), 0.0
    for b in range(B):
        for h in range(H):
            s = (q4[b, :, h] @ k4[b, :, h].t()) * scale
            win = s.gather(1, case["target"][b, h][:, None])
            s2 = s.scatter(1, case["target"][b, h][:, None], float("-inf"))
            if Nk > 1:
                gap = min(gap, float((win[:, 0] - s2.max(1).values).min()))
            top = max(top, float(win.max()))
    return gap, top


def attention_msum(D):
    """Whether the forward kernel takes the softmax row sum from a ones column of the P.V MFMAs (the sum of the ROUNDED
    probabilities) instead of an fp32 sum of the unrounded ones: D <= NB * 32 - 8 for the head dim's instantiation
    (attention.hip:174-176, 702, 745-750)."""
    return attention_instance(D)[3]


def attention_instance(D):
    """(DPP, NS, NB, msum): the template instantiation sdt_attention_fwd / _bwd dispatch head dim D to (attention.hip:782-787,
    822-827) and the forward's row-sum variant (attention_msum; the backward kernels have one variant)."""
    assert D % 8 == 0 and 8 <= D <= 160
    dpp, ns, nb = ((64, 3, 2) if D <= 48 else (64, 4, 2) if D <= 64 else (128, 5, 3) if D <= 80 else (128, 6, 3) if D <= 96
                   else (128, 8, 4) if D <= 128 else (256, 10, 5))
    return dpp, ns, nb, D <= nb * 32 - 8


def attention_qsplit(B, H, Nq, Nk, causal):
    """(planned, chunk, launched): a mirror of attn_qsplits (attention.hip:695-703) and of launch_bwd (:758-761).  `planned` query
    chunks size the workspace (1: the dK/dV pass does not split); the chunk is rounded up to whole 64-query tiles, so `launched`
    chunks of `chunk` queries cover Nq and launched <= planned.  The CPU proof holds `planned` to sdt_attention_bwd_workspace_bytes."""
    base = -(-Nk // 128) * H * B
    planned = 1
    if not causal and base < 128 and Nq >= 1024:
        planned = max(1, min(-(-256 // base), Nq // 256))
    chunk = -(-(-(-Nq // planned)) // 64) * 64
    return planned, chunk, -(-Nq // chunk)


def attention_delta_bytes(B, H, Nq):
    """The `delta` part of the backward workspace: B*H*Nq floats rounded up to four (attention.hip:796-797)."""
    return 4 * ((B * H * Nq + 3) // 4 * 4)


# ------------------------------------------------------------------------------------------------ tied-pair attention
def pair_case(B, H, Nq, Nk, D, seed, c=32.0, extras=True):
    """Inputs whose attention is exactly a mean of two V rows, with exact NONZERO dQ and dK.  The Nk keys of (b, h) form
    ceil(Nk / 2) pairs of twins (the last key of an odd Nk stays alone) laid on a seeded permutation of the key slots, so twins
    usually sit in different 64-key tiles.  Both twins carry the selector code of their pair (c * (+-1 per bit of a seeded
    permutation)) on the first nb = ceil(log2(pairs)) features; query i carries the code of its target pair.  Features nb, nb + 2,
    ... are key extras (each key its own integers in -3..3, every query zero), features nb + 1, nb + 3, ... query extras (each query
    integers in -3..3, every key zero): they never enter a logit, so the twins tie exactly and lead every other key by
    >= 2 c^2 / sqrt(D); P is exactly 1/2, 1/2 (1 for the lone key).  V: the pair's base row holds integers in -6..6 and the odd twin
    differs from it by +-2 in two seeded features; dO integers in -3..3.  extras=False zeroes the extras (the degenerate
    construction the CPU proof must refuse).
    Returns dict(q, k, v, dout: bf16 (B, N, H*D); pair: int64 (B, H, Nk), the pair of every key slot; target: int64 (B, H, Nq), the
    pair every query selects; nbits, c)."""
    npair = -(-Nk // 2)
    nb = max(1, math.ceil(math.log2(max(npair, 2))))
    assert nb + 2 <= D, f"pair_case: {npair} pairs need {nb} code features and two extras, D = {D}"
    g = torch.Generator().manual_seed(seed)
    q, k, v = torch.zeros(B, Nq, H, D), torch.zeros(B, Nk, H, D), torch.zeros(B, Nk, H, D)
    pair = torch.empty(B, H, Nk, dtype=torch.int64)
    target = torch.empty(B, H, Nq, dtype=torch.int64)
    sh = torch.arange(nb)
    kx, qx = torch.arange(nb, D, 2), torch.arange(nb + 1, D, 2)
    for b in range(B):
        for h in range(H):
            s = torch.randperm(npair, generator=g)
            slot = torch.randperm(Nk, generator=g)
            pr = torch.empty(Nk, dtype=torch.int64)
            pr[slot] = torch.arange(Nk) // 2
            odd = torch.zeros(Nk, dtype=torch.bool)
            odd[slot] = (torch.arange(Nk) % 2) == 1
            t = torch.randperm(npair, generator=g)[torch.arange(Nq) % npair]
            pair[b, h], target[b, h] = pr, t
            k[b, :, h, :nb] = (((s[pr][:, None] >> sh) & 1) * 2 - 1).float() * c
            q[b, :, h, :nb] = (((s[t][:, None] >> sh) & 1) * 2 - 1).float() * c
            kext = torch.randint(-3, 4, (Nk, kx.numel()), generator=g).float()
            qext = torch.randint(-3, 4, (Nq, qx.numel()), generator=g).float()
            if extras:
                k[b, :, h][:, kx] = kext
                q[b, :, h][:, qx] = qext
            base = torch.randint(-6, 7, (npair, D), generator=g).float()
            vh = base[pr]
            f0 = torch.randint(0, D, (Nk,), generator=g)
            f1 = (f0 + 1 + torch.randint(0, D - 1, (Nk,), generator=g)) % D   # a second, different feature
            sg = torch.randint(0, 2, (Nk, 2), generator=g).float() * 4 - 2
            rows = torch.arange(Nk)[odd]
            vh[rows, f0[odd]] += sg[odd, 0]
            vh[rows, f1[odd]] += sg[odd, 1]
            v[b, :, h] = vh
    do = torch.randint(-3, 4, (B, Nq, H * D), generator=g).float()
    return dict(q=q.reshape(B, Nq, H * D).to(BF), k=k.reshape(B, Nk, H * D).to(BF), v=v.reshape(B, Nk, H * D).to(BF), dout=do.to(BF),
                pair=pair, target=target, nbits=nb, c=c)


def pair_expect(case, B, H, Nq, Nk, D, scale, kv_chunk=None, perturb=None, drop_rows=None, scale_twice=False):
    """The bits sdt_attention_fwd / _bwd must produce on a pair case, in float64 from the IDEAL P (1 / number of tied keys on the
    target pair's keys, 0 elsewhere - not from a float64 softmax, whose losers do not underflow), rounded where the kernels round:
      O = RNE_bf16(P.V); dV = RNE_bf16(P^T.dO); dS = P o (dO.V^T - rowsum(dO o O)), exact in bf16;
      dQ = RNE_bf16(fl32(scale_f32 * (dS.K))) (attention.hip:492-493);
      dK = RNE_bf16(fl32(scale_f32 * (dS^T.Q))) where the dK/dV pass is one kernel (:657-658).  Where it splits the query range
        (kv_chunk: the chunk of attention_qsplit) every chunk stores fl32(scale_f32 * (its part of dS^T.Q)) to its fp32 slab
        (:639-640) and attn_kv_finish_kernel adds the slabs in chunk order in fp32 (:681-688) before the one bf16 rounding:
        dK = RNE_bf16(fp32 sum over chunks of fl32(scale_f32 * part)), which is not always fl32(scale_f32 * total) rounded when
        scale is not a power of two.  dV's slabs hold exact fp32 sums, so dV does not depend on the split.
      lse2 = (winning logit) * log2(e) + log2(number of tied keys), float64.
    perturb=None asserts that every one of these roundings is exact where it must be (P.V, P^T.dO, dS in bf16, both accumulators
    in fp32 below 2^24).  perturb=e (the margin proof) scales every probability, the forward's row sum included, by 1 + e and
    rounds as the kernels do: bf16(P) for P^T.dO, bf16(P (dP - delta)) with delta from the stored O.
    drop_rows=(lo, hi) leaves the queries lo..hi-1 out of dS^T.Q and scale_twice applies scale twice: the planted faults of the
    CPU proof.  Returns dict(o, dq, dk, dv: bf16 (B, N, H*D); lse2: float64 (B, H, Nq); ds: float64 (B, H, Nq, Nk); acc_q, acc_k:
    float64 accumulators (B, N, H*D); p: float64 (B, H, Nq, Nk))."""
    C = H * D
    q4, k4, v4 = (case[n].view(B, -1, H, D).transpose(1, 2).double() for n in ("q", "k", "v"))
    do4 = case["dout"].view(B, Nq, H, D).transpose(1, 2).double()
    hit = (case["pair"][:, :, None, :] == case["target"][:, :, :, None]).double()  # (B, H, Nq, Nk)
    ties = hit.sum(-1, keepdim=True)
    assert (ties >= 1).all() and (ties <= 2).all()
    p = hit / ties
    r16 = lambda t: t.to(torch.float32).to(BF).double()
    f32 = lambda t: t.to(torch.float32).double()
    exact = perturb is None
    pk = p if exact else p * (1.0 + perturb)

    def rounded(x, what, to):
        y = to(x + 0.0)  # (+ 0.0: a sum of -0 terms is +0 in an accumulator that starts at +0)
        assert not exact or torch.equal(y, x), f"pair_expect: {what} is not exact"
        return y

    o = rounded(pk @ v4, "P.V in bf16", r16)            # (the perturbed row sum scales every P alike: pk is already P (1 + e))
    dv = rounded(r16(pk).transpose(-1, -2) @ do4, "P^T.dO in bf16", r16)
    delta = (do4 * o).sum(-1, keepdim=True)
    ds = rounded(pk * (do4 @ v4.transpose(-1, -2) - delta), "dS in bf16", r16)
    scale_f = float(torch.tensor(scale, dtype=torch.float32))
    if scale_twice:
        scale_f = scale_f * scale_f
    acc_q = ds @ k4 + 0.0
    dsk = ds.clone()
    if drop_rows is not None:
        dsk[:, :, drop_rows[0]: drop_rows[1]] = 0
    chunks = [(0, Nq)] if kv_chunk is None else [(lo, min(lo + kv_chunk, Nq)) for lo in range(0, Nq, kv_chunk)]
    parts = [dsk[:, :, lo:hi].transpose(-1, -2) @ q4[:, :, lo:hi] + 0.0 for lo, hi in chunks]
    acc_k = sum(parts)
    for what, a in [("dS.K", acc_q)] + [("a part of dS^T.Q", a) for a in parts] + [("dS^T.Q", acc_k)]:
        assert torch.equal(f32(a), a) and float(a.abs().max()) < LIMIT, f"pair_expect: {what} is not exact in fp32 below 2^24"
    dq = r16(f32(acc_q * scale_f))
    dk32 = torch.zeros_like(acc_k, dtype=torch.float32)
    for a in parts:  # the finishing pass: fp32 additions in chunk order (one part: 0 + x = x)
        dk32 = dk32 + (a * scale_f).to(torch.float32)
    dk = dk32.to(BF).double()
    win = (q4[:, :, :, : case["nbits"]] ** 2).sum(-1) * scale_f   # the target's logit: nbits * c^2 * scale
    lse2 = win * 1.4426950408889634 + torch.log2(ties[..., 0])
    flat = lambda t, n: t.transpose(1, 2).reshape(B, n, C)
    return dict(o=flat(o, Nq).to(BF), dq=flat(dq, Nq).to(BF), dk=flat(dk, Nk).to(BF), dv=flat(dv, Nk).to(BF), lse2=lse2, ds=ds,
                acc_q=flat(acc_q, Nq), acc_k=flat(acc_k, Nk), p=p)


def pair_min_gap(case, B, H, Nq, Nk, D, scale):
    """(largest logit difference between two keys of the target pair, smallest lead of the pair over every other key, largest
    logit), float64: the tie must be exactly 0."""
    q4, k4 = (case[n].view(B, -1, H, D).transpose(1, 2).double() for n in ("q", "k"))
    s = (q4 @ k4.transpose(-1, -2)) * scale
    hit = case["pair"][:, :, None, :] == case["target"][:, :, :, None]
    win = s.masked_fill(~hit, float("-inf")).max(-1).values
    low = s.masked_fill(~hit, float("inf")).min(-1).values
    rest = s.masked_fill(hit, float("-inf")).max(-1).values
    return float((win - low).max()), float((win - rest).min()), float(win.max())


def pair_reports(got, want, D):
    """The pair checker: mismatch_report of out, dq, dk and dv (dicts of bf16 (B, N, H*D) tensors) against pair_expect, with the
    128-row x head tile named; a list of messages, empty when every bit agrees."""
    names = dict(o="out [batch][query][head * D + feature]", dq="dq [batch][query][head * D + feature]",
                 dk="dk [batch][key][head * D + feature]", dv="dv [batch][key][head * D + feature]")
    return [m for m in (mismatch_report(got[n], want[n], what, tile=(128, D)) for n, what in names.items()) if m is not None]


def attention_ref_and_emulation(q, k, v, do, H, scale, causal=False, key_weight=None, kv_chunk=None):
    """float64 attention (forward and the three gradients) and a torch emulation of the kernels' rounding points, head by head on
    the tensors' device.  q, do (B, Nq, H*D), k, v (B, Nk, H*D) bf16.  The emulation computes in float64 and rounds where the
    kernels round:
      forward (attention.hip:222-328): keys in tiles of 64; the probabilities are formed UNNORMALISED against the running row
        maximum, Pt = exp2(s * scale2 - m * scale2) (:268-276) (* w), and m is only raised - for all 32 queries of a wave at once -
        when some row's tile maximum exceeds it by more than 2^8 (:258-267), so Pt may exceed 1; Pt is rounded to bf16 for the P.V
        product (:301); the row sum l adds the unrounded Pt in fp32 (:286-291) or, for head dims with a spare padded feature, the
        rounded ones through a ones column (:310, attention_msum); O = bf16(acc / l) (:323); lse2 = fp32(m * scale2 + log2 l) (:314).
      backward (:371-390, :414-437, :455; :547-582, :622-627): delta = sum_d dO * O with the STORED bf16 O; P = exp2(s * scale2 -
        lse2) from the stored fp32 lse2; dS = P (dP - delta) rounded to bf16 before dS.K and dS^T.Q; P rounded to bf16 before
        P^T.dO; dQ = bf16(fl32(scale * acc)) (:492-493), dV = bf16(acc); dK = bf16(fl32(scale * acc)) (:657-658), except where the
        dK/dV pass splits the query range (kv_chunk: the chunk of attention_qsplit; None: one kernel): every chunk stores
        fl32(scale * its acc) to an fp32 slab (:639-640) and attn_kv_finish_kernel adds the slabs in chunk order in fp32 before the
        bf16 rounding (:681-690) - scale is applied per slab, not to the sum.
    Left out: fp32 accumulation order, the hardware exp2.
    Returns (ref, emu, mag): dicts of float64 tensors o, dq, dk, dv in the input layout; mag holds, per element, the sum of the
    magnitudes of the terms before any cancellation (o: P |V|; dv: P^T |dO|; dq: scale * (P (|dP| + |delta|)) |K|; dk likewise
    with |Q|) - the denominator floor of per_slice_rel for rows that are the result of cancellation."""
    B, Nq, C = q.shape
    Nk, D = k.shape[1], C // H
    dev = q.device
    names = ("o", "dq", "dk", "dv")
    ref = {n: torch.empty(B, (Nq if n in ("o", "dq") else Nk), C, dtype=torch.float64, device=dev) for n in names}
    emu = {n: torch.empty_like(t) for n, t in ref.items()}
    mag = {n: torch.empty_like(t) for n, t in ref.items()}
    r16 = lambda t: t.to(torch.float32).to(BF).double()
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    scale_f = float(f32(scale))
    scale2 = float(f32(scale) * f32(1.4426950408889634))  # attention.hip:683, an fp32 product
    msum = attention_msum(D)
    NEG = -1.0e30
    allowed = None
    if causal:
        allowed = torch.arange(Nk, device=dev)[None, :] <= torch.arange(Nq, device=dev)[:, None]
    w = None if key_weight is None else key_weight.double().to(dev)
    nw = -(-Nq // 32)
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            qh, kh, vh, doh = (t[b, :, sl].double() for t in (q, k, v, do))
            sr = qh @ kh.t()  # raw scores (exact: bf16 products, a sum far below 2^53)
            s = sr * scale
            if w is not None:
                s = s + torch.log(w)
            if allowed is not None:
                s = s.masked_fill(~allowed, float("-inf"))
            p = torch.softmax(s, -1)
            del s
            dp = doh @ vh.t()
            # ---- float64 reference and term magnitudes
            o = p @ vh
            delta = (doh * o).sum(-1, keepdim=True)
            ds = p * (dp - delta)
            ref["o"][b, :, sl], ref["dv"][b, :, sl] = o, p.t() @ doh
            ref["dq"][b, :, sl], ref["dk"][b, :, sl] = (ds @ kh) * scale, (ds.t() @ qh) * scale
            am = p * (dp.abs() + delta.abs())
            mag["o"][b, :, sl], mag["dv"][b, :, sl] = p @ vh.abs(), p.t() @ doh.abs()
            mag["dq"][b, :, sl], mag["dk"][b, :, sl] = (am @ kh.abs()) * scale, (am.t() @ qh.abs()) * scale
            del p, ds, am
            # ---- forward as the kernel runs it
            st = sr if allowed is None else sr.masked_fill(~allowed, NEG)
            m = torch.full((Nq,), NEG, dtype=torch.float64, device=dev)
            l = torch.zeros(Nq, dtype=torch.float64, device=dev)
            acc = torch.zeros(Nq, D, dtype=torch.float64, device=dev)
            for kb in range(0, Nk, 64):
                t = st[:, kb: kb + 64]
                mx = t.max(1).values
                trig = (mx - m) * scale2 > 8.0
                trig = torch.nn.functional.pad(trig, (0, nw * 32 - Nq)).view(nw, 32).any(1).repeat_interleave(32)[:Nq]
                m_new = torch.where(trig, torch.maximum(m, mx), m)
                alpha = torch.exp2((m - m_new) * scale2)
                m, l, acc = m_new, l * alpha, acc * alpha[:, None]
                pt = torch.exp2(t * scale2 - (m * scale2)[:, None])
                if w is not None:
                    pt = pt * w[kb: kb + 64]
                ptb = r16(pt)
                l = l + (ptb if msum else pt).sum(1)
                acc = acc + ptb @ vh[kb: kb + 64]
            ob = r16(acc / l[:, None])
            lse2 = (m * scale2 + torch.log2(l)).to(torch.float32).double()
            # ---- backward
            pbw = torch.exp2(sr * scale2 - lse2[:, None])
            if allowed is not None:
                pbw = pbw.masked_fill(~allowed, 0.0)
            if w is not None:
                pbw = pbw * w
            dsb = r16(pbw * (dp - (doh * ob).sum(-1, keepdim=True)))
            pb = r16(pbw)
            emu["o"][b, :, sl], emu["dv"][b, :, sl] = ob, r16(pb.t() @ doh)
            emu["dq"][b, :, sl] = r16((dsb @ kh) * scale_f)
            if kv_chunk is None:
                emu["dk"][b, :, sl] = r16((dsb.t() @ qh) * scale_f)
            else:
                slab = torch.zeros(Nk, D, dtype=torch.float32, device=dev)
                for lo in range(0, Nq, kv_chunk):
                    slab = slab + ((dsb[lo: lo + kv_chunk].t() @ qh[lo: lo + kv_chunk]) * scale_f).to(torch.float32)
                emu["dk"][b, :, sl] = slab.to(BF).double()
            del sr, st, dp, pbw, dsb, pb
    return ref, emu, mag


# ------------------------------------------------------------------------------------------------ norms
def _silu_and_grad(z):
    s = torch.sigmoid(z)
    return z * s, s * (1 + z * (1 - s))


def norm_ref_and_emulation(x, gamma, beta, dy, groups, eps, silu):
    """float64 GroupNorm (groups > 0: x (B, HW, C), statistics per image and group) or LayerNorm (groups = 0: x (M, C), per row),
    forward and backward, and an emulation of the kernels' rounding points (norm.hip): the statistics, the normalisation and the
    gradient formula are evaluated in fp32 and y / dx are rounded to bf16 ONCE when stored (gn_apply_kernel :189-195,
    gn_bwd_apply_kernel :392-407, ln_fwd_kernel :449-450, ln_bwd_kernel :523-531); dgamma / dbeta are fp32 sums of fp32 terms
    (gn_bwd_stats_kernel :246-250, partial_reduce_kernel).  The emulation therefore runs the same formulas in torch fp32 (torch's
    own summation order) and rounds y and dx to bf16.
    Returns (ref, emu, terms): ref / emu dicts of y, dx, dgamma, dbeta (ref float64); terms: per channel, sum |terms| of dgamma
    and dbeta (float64) - the denominator of their per-channel error."""
    out = []
    for dt in (torch.float64, torch.float32):
        xf, dyf, g, b = x.to(dt), dy.to(dt), gamma.to(dt), beta.to(dt)
        if groups:
            B, HW, C = xf.shape
            xg = xf.view(B, HW, groups, C // groups)
            red = (1, 3)
        else:
            xg, red = xf, (1,)
        mean = xg.mean(red, keepdim=True)
        var = (xg * xg).mean(red, keepdim=True) - mean * mean
        rstd = torch.rsqrt(var + eps)
        xh = ((xg - mean) * rstd).view(xf.shape)
        z = xh * g + b
        if silu:
            y, dact = _silu_and_grad(z)
            dz = dyf * dact
        else:
            y, dz = z, dyf
        dxh = dz * g
        sh = xg.shape
        m1 = dxh.view(sh).mean(red, keepdim=True)
        m2 = (dxh * xh).view(sh).mean(red, keepdim=True)
        dx = (rstd * (dxh.view(sh) - m1 - xh.view(sh) * m2)).view(xf.shape)
        lead = tuple(range(xf.dim() - 1))
        res = dict(y=y, dx=dx, dgamma=(dz * xh).sum(lead), dbeta=dz.sum(lead))
        if dt == torch.float64:
            terms = dict(dgamma=(dz * xh).abs().sum(lead), dbeta=dz.abs().sum(lead))
        out.append(res)
    ref, emu = out
    emu = dict(y=emu["y"].to(BF).double(), dx=emu["dx"].to(BF).double(), dgamma=emu["dgamma"].double(), dbeta=emu["dbeta"].double())
    return ref, emu, terms


# ------------------------------------------------------------------------------------------------ activations
def act_ref64(kind, x):
    """float64 value and derivative of the activations (x float64): 'silu', 'quick_gelu', 'gelu_erf', 'gelu_tanh'.  The tails are
    written without cancellation (erfc, sigmoid) so that the reference is accurate where the fp32 kernels are not."""
    if kind == "silu":
        s = torch.sigmoid(x)
        return x * s, s * (1 + x * (1 - s))
    if kind == "quick_gelu":
        s = torch.sigmoid(1.702 * x)
        return x * s, s * (1 + 1.702 * x * (1 - s))
    if kind == "gelu_erf":
        cdf = 0.5 * torch.special.erfc(-x * 0.7071067811865476)
        pdf = 0.3989422804014327 * torch.exp(-0.5 * x * x)
        return x * cdf, cdf + x * pdf
    if kind == "gelu_tanh":
        k = 0.7978845608028654
        u = k * (x + 0.044715 * x * x * x)
        s = torch.sigmoid(2 * u)                 # 0.5 * (1 + tanh u)
        sech2 = 4 * s * (1 - s)                  # 1 - tanh(u)^2
        du = k * (1 + 3 * 0.044715 * x * x)
        return x * s, s + 0.5 * x * sech2 * du
    raise ValueError(kind)


def bf16_ulp(v):
    """One bf16 unit in the last place at the magnitude of v (float64 tensor of bf16-representable values; 2^-133 below the normals)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def all_bf16_patterns():
    """All 65536 bf16 bit patterns (already a multiple of 8) as a bf16 tensor."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


def act_bound_violations(got, ref64, x64, dy_abs):
    """Indices where a finite activation result misses  |got - RNE_bf16(ref)| <= max(1 bf16 ulp of RNE_bf16(ref),
    8 * 2^-24 * max(|x|, 1) * |dy|)  (both terms derived in DESIGN.md "kernel test tolerances"); evaluated in float64."""
    want = ref64.to(torch.float32).to(BF).double()
    bound = torch.maximum(bf16_ulp(want), 8 * 2.0 ** -24 * x64.abs().clamp_min(1.0) * dy_abs)
    err = (got.double() - want).abs()
    return (~(err <= bound)).nonzero().reshape(-1)


# ------------------------------------------------------------------------------------------------ case tables
# sdt_gemm_nt_bf16, plain rows: (id, M, N, Kc, taps, b_kmajor, b_nseg, bias, rows_per_batch (0 = no row bias), residual, workspace,
# split, tile edge) - `split` is what sdt_gemm_nt_workspace_bytes must say (> 0 or == 0), the tile edge (64 / 128) is the kernel's
# output tile, named in a failure report; every case runs with ldc, ldres, ld_rowbias = N + 16
# and lda = taps * Kc + 16.  Branches of plan_nt / sdt_gemm_nt_bf16 (gemm.hip:1766-1797, 2123-2151):
GEMM_PLAIN_CASES = [
    ("t64_m1_n8_k8", 1, 8, 8, 1, 0, 0, True, 0, False, False, False, 64),           # 64-tiles at their smallest: M = 1, N = 8, Kc = 8
    ("t64_m5_kmajor", 5, 72, 40, 1, 1, 0, True, 0, True, False, False, 64),          # 64-tiles, k-major B, N % 64 == 8, Kc % 64 == 40
    ("t64_m63_rowbias", 63, 136, 72, 1, 0, 0, True, 21, True, False, False, 64),     # 64-tiles, row bias of 3 batches, Kc % 32 == 8
    ("t64_m65", 65, 200, 104, 1, 1, 0, False, 13, False, False, False, 64),          # 64-tiles, M % 64 == 1, N % 128 == 72, row bias only
    ("t64_m127", 127, 64, 64, 1, 0, 0, False, 0, True, False, False, 64),            # 64-tiles, one short row, residual only
    ("t64_m129", 129, 320, 320, 1, 1, 0, True, 43, True, False, False, 64),          # 64-tiles, M % 128 == 1 on three row tiles
    ("t64_taps3", 130, 72, 40, 3, 0, 0, True, 0, True, False, False, 64),            # plain rows with taps = 3: the shared-input dgrad
    ("t64_taps2_kmajor", 70, 136, 72, 2, 1, 0, True, 0, False, False, False, 64),    # ... with a k-major B
    ("t64_nseg", 300, 192, 72, 1, 1, 64, True, 0, True, False, False, 64),           # three 64-wide column segments (b_nseg)
    ("k32_m33025", 33025, 136, 72, 1, 1, 0, True, 6605, True, False, False, 128),     # 128-tiles, 32-wide K-steps, a large M % 128 == 1, all epilogue terms
    ("k32_rowmajor", 33025, 136, 72, 1, 0, 0, True, 0, True, False, False, 128),      # ... with a row-major Bt
    ("t128_k64", 4097, 1096, 1320, 1, 1, 0, True, 0, True, False, False, 128),        # 128-tiles, 64-wide K-steps (T = 21 > 20), N % 128 == 72, Kc % 64 == 40
    ("t128_k64_rowmajor", 4097, 1096, 1320, 1, 0, 0, False, 241, False, False, False, 128),
    ("t128_nosplit", 512, 520, 3080, 1, 1, 0, True, 0, True, False, True, 128),       # a split-K shape WITHOUT workspace: unsplit 128-tiles
    ("splitk128", 512, 520, 3080, 1, 1, 0, True, 128, True, True, True, 128),         # split-K, 128-tiles (T = 49, 20 tiles)
    ("splitk64", 200, 72, 4104, 1, 1, 0, True, 0, True, True, True, 64),             # split-K, 64-tiles (8 tiles, T = 65, Kc % 64 == 8)
    ("splitk64_rowmajor", 200, 72, 4104, 1, 0, 0, True, 50, True, True, True, 64),
    ("splitk64_few", 5, 1280, 1280, 1, 1, 0, True, 0, False, True, True, 64),        # a handful of tiles (time-embedding shape): T / 4 splits
]

# sdt_gemm_nt_bf16, gathered rows (fprop and dgrad): geometries of tests/test_gpu_kernels.py CONV_CASES (the CPU proof asserts
# membership), each with the kernel it is for
CONV_EXACT_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad
    (2, 16, 16, 64, 64, 3, 1, 1),                    # halo 16 x 16 tile = one image, unsplit or split by the planner
    (2, 16, 16, 64, 128, 3, 2, 1),                   # stride 2: generic gather; its dgrad is the GENERIC kernel
    (2, 16, 16, 64, 64, 3, 2, ((0, 1), (0, 1))),     # the VAE's asymmetric padding
    (2, 256, 256, 64, 128, 3, 2, ((0, 1), (0, 1))),  # gathered rows through the 32-wide-step 128-tile kernel
    (2, 8, 8, 128, 64, 1, 1, 0),                     # 1x1 (plain rows)
    (2, 12, 20, 8, 32, 3, 1, 1),                     # conv_in pack-8 path, 64-tiles
    (4, 64, 64, 8, 320, 3, 1, 1),                    # conv_in pack-8 path, 128-tiles, ragged channel tile
    (2, 16, 16, 320, 8, 3, 1, 1),                    # conv_out: N = 8
    (3, 8, 8, 2560, 1280, 3, 1, 1),                  # halo 8 x 8 x four images, ragged image group (3 of 4), split, the largest reduction: 9 * 2560
    (2, 64, 64, 320, 320, 3, 1, 1),                  # halo 4 x 64 tiles, N = 2.5 / 5 channel tiles, split
    (1, 8, 128, 128, 128, 3, 1, 1),                  # halo 4 x 64, two tiles per row
    (2, 32, 32, 640, 1280, 3, 1, 1),                 # halo 8 x 32 tiles, split over channel chunks
    (2, 36, 28, 64, 64, 3, 1, 1),                    # not tileable: the generic path
    (2, 24, 40, 64, 64, 3, 1, 1),                    # halo 8 x 8, two of the four image slots empty
    (3, 16, 24, 64, 128, 3, 1, 1),                   # halo 8 x 8, ragged image group (3 of 4)
    (1, 32, 48, 128, 64, 3, 1, 1),                   # halo 16 x 16, 2 x 3 tiles per image
    (1, 256, 320, 64, 128, 3, 1, 1),                 # halo 4 x 64, 320 tiles, unsplit
]

# weight gradients.  Dense (sdt_gemm_tn_wgrad plain, and the same problems through sdt_gemm_tn_wgrad_group):
# (id, M, K1, N, K1_valid, N_valid, n_seg, split) - split: sdt_gemm_tn_workspace_bytes > 0
WGRAD_DENSE_CASES = [
    ("t64_small", 100, 64, 136, 64, 136, 0, False),          # 64-tiles (K1 < 128), ragged N
    ("t64_valid", 77, 72, 72, 68, 70, 0, False),             # K1_valid < K1, N_valid < N
    ("t128", 300, 320, 320, 320, 320, 0, False),             # 128-tiles, 2.5 tiles each way, unsplit (M < 2 * 1024)
    ("t128_valid", 1000, 136, 264, 130, 260, 0, False),
    ("t128_split", 16384, 320, 320, 320, 320, 0, True),      # split reduction over M
    ("t64_split", 4096, 64, 72, 64, 72, 0, True),
    ("t128_seg", 2048, 320, 960, 320, 960, 320, True),       # three 320-wide segments (to_q / to_k / to_v), split
    ("t64_seg", 130, 72, 192, 72, 192, 64, False),
]
# convolutions (sdt_gemm_tn_wgrad in fprop-gather mode and sdt_conv_wgrad_group): (B, H, W, Cin, Cout, k, stride, pad, kernel)
WGRAD_CONV_CASES = [
    (1, 96, 96, 64, 64, 3, 1, 1, "three-tap, 96 wide (a chunk is 2/3 of a row), split"),
    (2, 48, 48, 128, 64, 3, 1, 1, "three-tap, 48 wide, split"),
    (4, 24, 24, 64, 136, 3, 1, 1, "three-tap, 24 wide, ragged channel tile, split"),
    (8, 12, 12, 64, 64, 3, 1, 1, "nine-tap (12 wide is not a multiple of 8), split"),
    (4, 8, 8, 128, 72, 3, 1, 1, "three-tap at its smallest, one pass"),
    (4, 64, 64, 64, 64, 3, 1, 1, "three-tap, 64 wide, split"),
    (2, 16, 16, 64, 128, 3, 2, 1, "nine-tap, stride 2 (row walk), one pass"),
    (16, 4, 4, 64, 64, 3, 1, 1, "nine-tap generic (fewer than 64 pixels per image), one pass"),
    (2, 12, 20, 8, 32, 3, 1, 1, "nine-tap, 8 input channels, one pass"),
]
# (a case whose description ends in "split" must get scratch from sdt_gemm_tn_workspace_bytes, the others none)

# GroupNorm statistics from the epilogues: operands in -1..1, Kc <= 64, so that the fp32 sums and sums of squares of the bf16 outputs
# stay below 2^24 (asserted by the CPU proof on the very operands).  Dense: (M, N, Kc, rows_per_batch, groups); halo: conv geometry + groups
GN_DENSE_CASES = [
    (512, 320, 64, 256, 32),     # 64-tiles: groups of 10 columns straddle the tile edges at 64, 128, ...
    (33024, 160, 64, 16512, 32),  # 128-tiles (32-wide K-steps), ragged second channel tile, 129 row tiles per image
]
GN_HALO_CASES = [
    (2, 64, 64, 64, 320, 32),    # 4 x 64 tiles, N = 2.5 / 5 channel tiles: groups of 10 straddle
    (1, 32, 32, 64, 96, 32),     # 8 x 32 tiles, groups of 3 over a ragged channel tile
    (2, 32, 48, 64, 64, 32),     # 16 x 16 tiles, one channel tile
]

# attention, selector inputs: the shapes of test_attention_fwd_bwd / test_attention_key_weights.
# (B, H, Nq, Nk, D, causal, packed, key_weights)
ATTN_SELECTOR_CASES = [
    (2, 8, 256, 256, 40, False, False, False),
    (1, 8, 1024, 1024, 40, False, True, False),
    (2, 8, 64, 77, 160, False, False, True),     # head dim 160, ragged Nk, key weights of the clamped chunks
    (2, 8, 256, 77, 80, False, False, False),
    (2, 5, 144, 144, 64, False, False, False),
    (3, 12, 77, 77, 64, True, False, False),     # causal, ragged
    (1, 3, 77, 77, 16, True, False, False),      # causal, head dim 16
    (1, 2, 200, 333, 128, False, True, False),   # head dim 128, ragged Nq and Nk, packed k|v
    (1, 5, 9216, 9216, 64, False, False, False),  # the long self-attention
    (2, 8, 2048, 77, 40, False, True, True),     # few keys: the query-split dK/dV pass, packed, synthetic key weights
    (1, 4, 1100, 100, 64, False, False, False),  # query-split, ragged
    (4, 8, 1024, 77, 80, False, False, True),    # query-split, head dim 80, key weights
    (1, 8, 144, 231, 80, False, True, True),
]

# ... at every head dim the ABI accepts: Nq = 136 and Nk = 200 are ragged against the 64 and 128 tiles, ceil(log2 200) = 8 code
# features fit D = 8, and H = 3 puts heads 1 and 2 at column offsets that are no multiple of 64.  packed / key_weights rotate with a
# period of four, and the head dims that are alone in their (instantiation, row-sum variant) run a second time with both flags
# inverted: every one of the ten (attention_instance) tuples meets both values of both flags.  Then causal cases, one per tuple but
# <64,4,2> without the ones column (ATTN_SELECTOR_CASES has it: 77 x 77 at D = 64).
_HD_FLAGS = [(False, False), (True, True), (False, True), (True, False)]
ATTN_HEADDIM_CASES = (
    [(1, 3, 136, 200, D, False) + _HD_FLAGS[i % 4] for i, D in enumerate(range(8, 168, 8))]
    + [(1, 3, 136, 200, D, False) + tuple(not f for f in _HD_FLAGS[(D // 8 - 1) % 4]) for D in (56, 64, 88, 96, 128, 160)]
    + [(1, 3, 200, 200, D, True, False, False) for D in (8, 56, 72, 88, 96, 120, 128, 152, 160)])

# ... at the size edges: one query, one key, Nk and Nq at and around the 64 / 128 tile edges, and the query-split planner at its
# threshold (Nq = 1023 must not split, 1024 must: ATTN_SPLIT_CLAIMS)
ATTN_EDGE_CASES = (
    [(1, 1, 1, 1, 8, False, False, False), (1, 2, 1, 77, 40, False, False, False), (1, 2, 77, 1, 64, False, False, False),
     (2, 1, 1, 1, 160, False, False, False)]
    + [(1, 2, 136, Nk, D, False, False, False) for D in (64, 88) for Nk in (63, 64, 65, 127, 128, 129)]
    + [(1, 2, Nq, 200, 96, False, False, False) for Nq in (127, 128, 129)]
    + [(1, 1, 1023, 77, 40, False, False, False), (1, 1, 1024, 77, 40, False, False, False)])

# attention, tied-pair inputs (pair_case): (B, H, Nq, Nk, D, packed)
_PAIR_UNSPLIT = (
    [(1, 2, 136, 200, D, False) for D in (16, 40, 56, 64, 72, 80, 88, 96, 120, 128, 152, 160)]
    + [(1, 2, 136, 72, 8, False),       # D = 8: six code features and one extra each leave room for 64 pairs at most
       (2, 3, 130, 77, 96, True)])      # batch strides, an odd Nk (one lone key), packed k|v
ATTN_PAIR_SPLIT_CASES = [               # the dK/dV pass splits the query range: fp32 slabs and attn_kv_finish_kernel
    (1, 1, 1600, 77, 40, False),        # plans 6 query chunks, launches 5 of 320
    (1, 2, 1100, 100, 64, False),
    (1, 2, 1024, 77, 96, False),
    (2, 2, 1024, 90, 152, True),
    (1, 2, 1024, 77, 120, False),       # <128,8,4>, which no other split case reaches
    (1, 3, 1024, 77, 72, False)]        # <128,5,3>: with these two, the split pass of every instantiation
ATTN_PAIR_CASES = _PAIR_UNSPLIT + ATTN_PAIR_SPLIT_CASES

# (B, H, Nq, Nk, causal) -> whether sdt_attention_bwd_workspace_bytes must ask for slabs beyond the delta part
ATTN_SPLIT_CLAIMS = dict(
    [((B, H, Nq, Nk, False), True) for B, H, Nq, Nk, D, packed in ATTN_PAIR_SPLIT_CASES]
    + [((B, H, Nq, Nk, False), False) for B, H, Nq, Nk, D, packed in _PAIR_UNSPLIT]
    + [((1, 1, 1023, 77, False), False), ((1, 1, 1024, 77, False), True), ((2, 8, 2048, 77, False), True),
       ((1, 4, 1100, 100, False), True), ((4, 8, 1024, 77, False), True), ((1, 8, 1024, 1024, False), True),
       ((2, 20, 1024, 1024, False), False)])  # (64 key blocks x heads x images leave the chip half idle: split; 320 do not)

# attention, Gaussian inputs judged per row (test_attention_gaussian_inputs_per_row): (B, H, Nq, Nk, D, causal)
ATTN_ROW_CASES = [
    # the shapes of test_attention_fwd_bwd
    (2, 8, 256, 256, 40, False), (1, 8, 1024, 1024, 40, False), (2, 8, 64, 77, 160, False), (2, 8, 256, 77, 80, False),
    (2, 5, 144, 144, 64, False), (3, 12, 77, 77, 64, True), (1, 3, 77, 77, 16, True), (1, 2, 200, 333, 128, False),
    (1, 8, 4096, 4096, 40, False), (1, 5, 9216, 9216, 64, False), (1, 10, 2304, 2304, 64, False), (2, 20, 1024, 1024, 64, False),
    (2, 8, 2048, 77, 40, False), (1, 4, 1100, 100, 64, False), (4, 8, 1024, 77, 80, False)]
# ... every other head dim at the ragged shape of the D = 128 row, and causal rows for three instantiations more
ATTN_ROW_HEADDIM_CASES = (
    [(1, 2, 200, 333, D, False) for D in range(8, 168, 8) if D not in {c[4] for c in ATTN_ROW_CASES}]
    + [(1, 2, 200, 200, D, True) for D in (56, 96, 152)])
# ... with the key weights of the clamped chunks (nets.key_chunk_weights: 64 queries x 77 keys)
ATTN_ROW_KEYWEIGHT_CASES = [(2, 4, 64, 77, 88), (2, 4, 64, 77, 136)]


def halo_tile(H, W, Cin, M, k, stride, pad):
    """(images, rows, columns) of the tile conv_halo_plan (gemm.hip:1960-1982) gives a 3x3 / stride 1 / pad 1 convolution, or None
    where it declines.  A mirror of the planner: it decides which cases run at both tile widths and names the tile in a report.  The
    CPU proof holds it to the library (sdt_gemm_nt_gn_parts) for every convolution case."""
    if k != 3 or stride != 1 or norm_pad(pad) != ((1, 1), (1, 1)) or Cin % 64 or M < 256:
        return None
    if W % 64 == 0 and H % 4 == 0:
        return (1, 4, 64)
    if W == 32 and H % 8 == 0:
        return (1, 8, 32)
    if W % 16 == 0 and H % 16 == 0:
        return (1, 16, 16)
    if W % 8 == 0 and H % 8 == 0:
        return (4, 8, 8)
    return None


def norm_pad(pad):
    return ((pad, pad), (pad, pad)) if isinstance(pad, int) else pad


def conv_out_hw(H, W, k, stride, pad):
    (pt, pb), (pl, pr) = norm_pad(pad)
    return (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1


def exact_reductions():
    """(what, |a|max, |b|max, terms) of every exact contraction the GPU file runs: sum |a||b| <= |a|max |b|max terms must stay below
    2^24 (the CPU proof asserts it).  Operand ranges: GEMM_RANGE for forward / input-gradient operands, WGRAD_RANGE for the weight
    gradients (their reduction runs over M)."""
    out = []
    for c in GEMM_PLAIN_CASES:
        out.append((f"gemm {c[0]}", GEMM_RANGE, GEMM_RANGE, c[4] * c[3]))
    for B, H, W, Cin, Cout, k, stride, pad in CONV_EXACT_CASES:
        out.append((f"conv fprop {(B, H, W, Cin, Cout)}", GEMM_RANGE, GEMM_RANGE, k * k * Cin))
        out.append((f"conv dgrad {(B, H, W, Cin, Cout)}", GEMM_RANGE, GEMM_RANGE, k * k * Cout))
    for c in WGRAD_DENSE_CASES:
        out.append((f"wgrad {c[0]}", WGRAD_RANGE, WGRAD_RANGE, c[1]))
    for B, H, W, Cin, Cout, k, stride, pad, _ in WGRAD_CONV_CASES:
        OH, OW = conv_out_hw(H, W, k, stride, pad)
        out.append((f"conv wgrad {(B, H, W, Cin, Cout)}", WGRAD_RANGE, WGRAD_RANGE, B * OH * OW))
    for B, H, Nq, Nk, D, *_ in ATTN_SELECTOR_CASES + ATTN_HEADDIM_CASES + ATTN_EDGE_CASES:
        out.append((f"attention dV {(B, H, Nq, Nk, D)}", 3, 1, Nq))
    return out


GEMM_RANGE = 3   # operands of the forward / input-gradient contractions: integers in -3..3
WGRAD_RANGE = 3  # operands of the weight gradients
EPI_RANGE = 5    # bias, row bias, residual: integers in -5..5


# ================================================================================================ reductions, optimizer sweeps, loss kernels
# (tests/test_gpu_reduce_optim_exact.py; their proof on the CPU: tests/test_kernel_checks_cpu.py)
CNT_BYTES = 65536  # arrival counters at the head of every reduction workspace (include/sdt.h)


def counters_report(ws_bytes, what="workspace"):
    """None when the 64 KiB counter area (uint8 tensor, any device) is zero; otherwise which int32 counters are not."""
    c = ws_bytes[:CNT_BYTES].cpu().view(torch.int32)
    nz = c.nonzero().reshape(-1)
    if nz.numel() == 0:
        return None
    return f"{what}: {nz.numel()} arrival counters not reset, first: counter {int(nz[0])} = {int(c[nz[0]])}"


def sum_report(got, want, what, init=0.0, parts=None, tail=None):
    """Comparison of one exact scalar sum (float64 values of what the kernel stored and of the reference `init + total`).  None when
    equal; otherwise a message that names what the difference equals: the partial of ONE workgroup (parts: float64 tensor, the sum of
    each workgroup's share under the kernel's partition), ONE tail element's term (tail: float64 tensor of the terms behind the last
    vector), or the destination's previous value (a store where an accumulation belongs)."""
    got, want = float(got), float(want)
    if got == want:
        return None
    diff = want - got
    hints = []
    if init != 0.0 and diff == init:
        hints.append(f"the difference is the destination's previous value {init!r}: stored with = where += belongs")
    if parts is not None:
        hit = (parts.double() == diff).nonzero().reshape(-1)
        if diff != 0 and hit.numel():
            hints.append(f"the difference is the partial of workgroup {hit[:4].tolist()} of {parts.numel()}")
    if tail is not None:
        t = tail.double().reshape(-1)
        for k in range(1, t.numel() + 1):  # the last k tail elements missing
            if diff == float(t[-k:].sum()) and diff != 0:
                hints.append(f"the difference is the term of the last {k} of the {t.numel()} tail elements (n & 3)")
                break
        hit = (t == diff).nonzero().reshape(-1)
        if diff != 0 and hit.numel() and not hints:
            hints.append(f"the difference is the term of tail element {hit.tolist()}")
    return f"{what}: got {got!r}, want {want!r} (want - got = {diff!r})" + ("; " + "; ".join(hints) if hints else "")


def sqnorm_partition(n):
    """(grid, float4s) of sqnorm_kernel / grad_accumulate_kernel (optimizer.hip): one workgroup per 2048 float4s, at most 2048
    workgroups, a grid-stride loop beyond; the n & 3 tail belongs to workgroup 0."""
    nv = n >> 2
    return max(1, min(2048, -(-nv // 2048))), nv


def sqnorm_parts(x64sq, n):
    """float64 partial of every workgroup under sqnorm_partition (x64sq: the n squared terms, float64)."""
    grid, nv = sqnorm_partition(n)
    parts = torch.zeros(grid, dtype=torch.float64)
    if nv:
        v = x64sq[: nv * 4].view(nv, 4).sum(1)
        wg = (torch.arange(nv) // 256) % grid
        parts.index_add_(0, wg, v)
    parts[0] += x64sq[nv * 4:].sum()
    return parts


def sum_f64_partition(n):
    """(grid, per) of sum_f64_kernel: ceil(n / 4096) workgroups, at most 2048; workgroup b sums [b * per, (b + 1) * per)."""
    grid = max(1, min(2048, -(-n // 4096)))
    return grid, -(-n // grid)


def colsum_plan(batch, rows, N, want_blocks):
    """colsum_launch (elementwise.hip): (ncb, nby, rpb, want).  want_blocks: 256 for sdt_colsum_accumulate, 512 for the batched form."""
    ncb = -(-(-(-N // 8)) // 32)
    nby = (rows + 63) // 64
    want = (want_blocks + ncb * batch - 1) // (ncb * batch)
    nby = min(nby, want)
    rpb = (rows + nby - 1) // nby
    return ncb, -(-rows // rpb), rpb, want


# ---- case tables: every one carries the bound that makes its sums exact (asserted by the CPU proof)
SQNORM_RANGE = 3  # integers in -3..3: every square, partial and total is an integer far below 2^53
SQNORM_SIZES = [1, 2, 3, 4, 5, 7, 8191, 8192, 8193, (1 << 20) + 3, (1 << 24) + 8192 * 3 + 5]  # the last: capped grid, second stride pass
ACC_SIZES = SQNORM_SIZES[:-1]
SUMF64_RANGE = 1 << 20  # integer-valued doubles in +-2^20: n * 2^20 < 2^53
SUMF64_SIZES = [1, 255, 256, 257, 511, 512, 513, 4096, 4097, (1 << 20) + 1, 2048 * 4096 + 4099]  # the last: per > 4096

# sdt_mse_loss_fwd_bwd: (id, B, C, H, W, cpad, weight, dpred, loss_accum before).  pred and target integers in -1..1 (diff^2 <= 4),
# weights in {0.5, 1, 2}: sum w diff^2 <= 8 * B*C*H*W must stay below 2^24 and, for the power-of-two counts, so must
# loss_before * count + that sum (then loss_before + sum / count is exact too).
MSE_WMAX, MSE_DIFF2 = 2.0, 4
MSE_CASES = [
    ("one_wg", 2, 4, 8, 8, 8, True, True, 3.0),
    ("one_wg_noweight", 2, 4, 8, 8, 4, False, True, 3.0),
    ("one_wg_nodpred", 2, 4, 8, 8, 16, True, False, 3.0),
    ("cap_512_wg", 2, 4, 256, 256, 4, True, True, 3.0),
    ("cap_512_wg_nodpred_noweight", 2, 4, 256, 256, 8, False, False, 3.0),
    ("stride_2_passes", 4, 4, 256, 256, 16, True, True, 3.0),
    ("stride_b8", 8, 4, 128, 256, 8, True, True, 1.0),
    # counts that are not powers of two: loss within 2 fp32 ulps (1 / count and t * inv_count round), loss_accum starts at 0
    ("c3", 2, 3, 8, 9, 8, True, True, 0.0),
    ("c3_unpadded", 5, 3, 7, 11, 3, False, True, 0.0),
    ("c9", 3, 9, 5, 7, 16, True, True, 0.0),
    ("c9_unpadded", 2, 9, 16, 16, 9, True, True, 0.0),
]

# column sums: (N, ld, rows, batch, range).  |value| <= range, rows * range < 2^24.
COLSUM_CASES = [
    (8, 8, 1, 1, 200), (8, 24, 1 << 20, 1, 3), (8, 16, 65537, 2, 50), (248, 264, 7, 2, 200), (250, 256, 63, 1, 200), (256, 256, 64, 5, 200),
    (256, 272, 65, 5, 200), (264, 280, 65537, 1, 50), (1280, 1296, 4096, 2, 100), (2560, 2560, 65, 1, 200), (2560, 2576, 4096, 1, 100),
    (1280, 1280, 63, 5, 200), (2556, 2560, 7, 1, 200),
]

# embeddings: (D, sequences, id pattern, vocabulary); S = 77, dout in -3..3, tables preloaded with integers in -100..100
EMB_S = 77
EMB_CASES = [(48, 1, "distinct", 1000), (48, 12, "distinct", 1000), (768, 12, "clip", 1000), (1280, 5, "equal_last", 300), (1280, 1, "clip", 300),
             (768, 3, "equal_first", 300)]


def embedding_ids(pattern, nseq, vocab, seed):
    """int32 (nseq * 77,) ids: 'distinct' - no id twice, ids 0 and vocab - 1 among them; 'equal_first' / 'equal_last' - row 0 / the last
    row of the table everywhere; 'clip' - per sequence a begin token, a few words, then one padding id (the last row) to the end."""
    rows = nseq * EMB_S
    g = torch.Generator().manual_seed(seed)
    if pattern == "distinct":
        ids = torch.randperm(vocab - 2, generator=g)[: rows - 2] + 1
        ids = torch.cat([torch.tensor([vocab - 1]), ids, torch.tensor([0])])
    elif pattern == "equal_first":
        ids = torch.zeros(rows, dtype=torch.int64)
    elif pattern == "equal_last":
        ids = torch.full((rows,), vocab - 1, dtype=torch.int64)
    else:
        ids = torch.full((nseq, EMB_S), vocab - 1, dtype=torch.int64)
        ids[:, 0] = vocab - 2
        for s in range(nseq):
            k = 3 + (5 * s) % 9
            ids[s, 1: 1 + k] = torch.randint(0, 4, (k,), generator=g) if s % 2 else torch.randint(0, vocab - 2, (k,), generator=g)
        ids = ids.reshape(-1)
    return ids.to(torch.int32)


# optimizer sweeps
LION_BLOCK_SIZES = [4, 8, 16, 32, 64, 128, 256]
LION32_SIZES = [1, 3, 1023, 1024, 1025, (1 << 20) + 5]
LION_HP = dict(lr=1e-3, b1=0.9, b2=0.99, ema_rate=0.999)


def lion8_sizes(bs):
    """One block; the buffer's end inside a wave, on a 1024-float4 slice boundary, one block past it; 2^20 + one block."""
    return [bs, 4096 - bs, 4096, 4096 + bs, (1 << 20) + bs]


def lion8_reference_step(p, g, codes, inv, ema, bs, max_norm, wd, hp=LION_HP):
    """One carried step of oracle.lion8 on flat float32 arrays: (p, codes [blocks][bs], inv [blocks][1], ema, bf16(p),
    sum of squares handed to the kernel).  max_norm None: no clip (the kernel gets a NULL sqnorm)."""
    state = {"count": 0, "mu": {"x": (codes.reshape(-1, bs), inv.reshape(-1, 1))}}
    sq = float(np.sum(np.asarray(g, np.float64) * np.asarray(g, np.float64)))
    newp, st, _ = LION_ORACLE.lion_step({"x": p}, {"x": g}, state, lr=hp["lr"], wd=wd, b1=hp["b1"], b2=hp["b2"], block_size=bs, clip=max_norm)
    c, i = st["mu"]["x"]
    e = None if ema is None else LION_ORACLE.ema_update({"x": ema}, newp, hp["ema_rate"])["x"]
    return newp["x"], c, i, e, torch.from_numpy(newp["x"]).to(BF), sq


def lion32_reference_step(p, g, mom, ema, max_norm, wd, hp=LION_HP):
    state = {"count": 0, "mu": {"x": mom}}
    sq = float(np.sum(np.asarray(g, np.float64) * np.asarray(g, np.float64)))
    newp, st, _ = LION_ORACLE.lion_step({"x": p}, {"x": g}, state, lr=hp["lr"], wd=wd, b1=hp["b1"], b2=hp["b2"], clip=max_norm)
    e = None if ema is None else LION_ORACLE.ema_update({"x": ema}, newp, hp["ema_rate"])["x"]
    return newp["x"], st["mu"]["x"], e, torch.from_numpy(newp["x"]).to(BF), sq


def grads_with_exact_norm(n, seed):
    """(g float32 [n], max_norm): multiples of 2^-4 (exact in bf16) whose norm is EXACTLY max_norm = M * 2^-4, M an integer that is not
    a power of two: random a_i in -15..15 behind a reserve of leading elements that are set to 15s and 1s so that sum a_i^2 = M^2.  The
    squares sum to an integer below 2^53 in any order.  M is chosen (for n >= 256) so that (g / norm) * max_norm != g in float32 for at
    least n / 32 elements (the round trip returns most small integers unchanged): the two branches of optax's clip give different bits."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randint(-15, 16, (n,), generator=gen)
    reserve = n // 2 if n >= 64 else n - 1
    a[:reserve] = 0
    S = int((a * a).sum())
    af = a.float().numpy() / np.float32(16)
    for M in range(math.isqrt(S) + 1, math.isqrt(S) + 400):
        q, r = divmod(M * M - S, 225)
        if q + r > reserve or M & (M - 1) == 0:
            continue
        mx = np.float32(M / 16.0)
        if n >= 256 and np.count_nonzero(((af / mx).astype(np.float32) * mx).astype(np.float32) != af) < n // 32:
            continue
        a[:q], a[q: q + r] = 15, 1
        assert int((a * a).sum()) == M * M
        return a.float().numpy() / np.float32(16), M / 16.0
    assert n < 64, "no exact norm found"
    a[:] = 0
    a[0] = 3
    return a.float().numpy() / np.float32(16), 3.0 / 16


def lion_state_report(codes, inv, want_codes, want_inv, what):
    """None, or where the 8-bit state differs from the oracle's: codes [blocks][bs] by block and element, inverse scales by block -
    naming a scale that is the oracle's scale of a NEIGHBOURING block (the store that went to the wrong block or was skipped)."""
    msgs = []
    bad = np.argwhere(codes != want_codes)
    if bad.size:
        b, e = bad[0]
        msgs.append(f"{len(bad)} codes differ, first: block {b} element {e}: got {int(codes[b, e])}, want {int(want_codes[b, e])}")
    gi, wi = inv.reshape(-1), want_inv.reshape(-1)
    badi = np.flatnonzero(gi.view(np.int32) != wi.view(np.int32))
    if badi.size:
        b = int(badi[0])
        m = f"{badi.size} inverse scales differ, first: block {b}: got {gi[b]!r}, want {wi[b]!r}"
        for o in (-1, 1):
            if 0 <= b + o < wi.size and gi[b].view(np.int32) == wi[b + o].view(np.int32):
                m += f" (the oracle's scale of block {b + o})"
        msgs.append(m)
    return None if not msgs else f"{what}: " + "; ".join(msgs)


# ---- VAE posterior sample
POST_EPS = (0.0, 1.0, -1.0, 3.5, -3.5)
POST_SCALE = 0.18215
LV_HI, LV_LO = 0x41A0, 0xC1F0  # the bf16 patterns of 20 and -30


def posterior_ref64(mean, lv, eps, scale=POST_SCALE):
    return (mean.double() + torch.exp(0.5 * lv.double().clamp(-30.0, 20.0)) * eps.double()) * float(torch.tensor(scale, dtype=torch.float32))


def posterior_emulation(mean, lv, eps, scale=POST_SCALE):
    """The kernel's rounding points (posterior_sample_kernel): h = fl32(0.5 lv) (exact), a = fl32(h * fl32(log2 e)), e = fl32(2^a) with an
    exact exp2, then fl32(fl32(mean + e * eps) * scale) with one rounding for the multiply-add (the file is built with contraction)."""
    f32 = lambda t: t.to(torch.float32).double()
    a = f32(f32(0.5 * lv.double().clamp(-30.0, 20.0)) * float(torch.tensor(1.4426950408889634, dtype=torch.float32)))
    e = f32(torch.exp2(a))
    return f32(f32(mean.double() + e * eps.double()) * float(torch.tensor(scale, dtype=torch.float32)))


def posterior_term_magnitude(mean, lv, eps, scale=POST_SCALE):
    return (mean.double().abs() + torch.exp(0.5 * lv.double().clamp(-30.0, 20.0)) * eps.double().abs()) * scale


def posterior_clip_report(got, lv_bits, eps_idx):
    """got: float32 latents, one per (logvar pattern, eps) pair; lv_bits: the bf16 pattern (0..65535) of each; eps_idx: which eps.
    Every pattern >= 20 (+inf included) must hold the bits of the pattern 20 with the same eps, every pattern <= -30 (-inf included)
    those of -30; NaN patterns must give NaN.  None, or the first offending pattern of each rule."""
    v = lv_bits.to(torch.int32).to(torch.int16).view(BF).double()
    gb = bits(got)
    msgs = []
    for name, sel, anchor in ((">= 20", v >= 20.0, LV_HI), ("<= -30", v <= -30.0, LV_LO)):
        for k in range(len(POST_EPS)):
            m = sel & (eps_idx == k)
            ref = gb[(lv_bits == anchor) & (eps_idx == k)]
            assert ref.numel() == 1
            bad = m & (gb != ref)
            if bad.any():
                i = int(bad.nonzero()[0])
                msgs.append(f"logvar pattern 0x{int(lv_bits[i]):04x} ({float(v[i])!r}) with eps {POST_EPS[k]}: got {float(got[i])!r}, the clipped "
                            f"value gives {float(got[(lv_bits == anchor) & (eps_idx == k)][0])!r} ({int(bad.sum())} patterns {name} differ)")
                break
    nan = torch.isnan(v)
    bad = nan & ~torch.isnan(got.double())
    if bad.any():
        i = int(bad.nonzero()[0])
        msgs.append(f"NaN logvar pattern 0x{int(lv_bits[i]):04x} gave the number {float(got[i])!r} ({int(bad.sum())} of {int(nan.sum())} NaN patterns)")
    return None if not msgs else "posterior sample: " + "; ".join(msgs)


# ---- timestep embedding
def timestep_ref64(t, dim, flip, shift):
    half = dim // 2
    inc = math.log(10000.0) / (half - shift)
    e = t.double()[:, None] * torch.exp(torch.arange(half, dtype=torch.float64) * -inc)[None]
    return torch.cat([torch.cos(e), torch.sin(e)], -1) if flip else torch.cat([torch.sin(e), torch.cos(e)], -1)


def timestep_report(got, t, dim, flip, shift):
    """|got - ref| <= 1/2 bf16 ulp(ref) + 2^-22 max(t, 1) for every element (the bound: DESIGN.md §7a); None, or the first violations -
    and whether the result would pass with its sin and cos halves exchanged."""
    ref = timestep_ref64(t, dim, flip, shift)
    bound = 0.5 * bf16_ulp(ref) + 2.0 ** -22 * t.double().clamp_min(1.0)[:, None]
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    if not bad.any():
        return None
    half = dim // 2
    sw = torch.cat([got[:, half:], got[:, :half]], -1).double()
    swapped = bool(((sw - ref).abs() <= bound).all())
    c = _coords(bad.reshape(-1).nonzero().reshape(-1)[:4], tuple(got.shape))
    return (f"timestep embedding dim {dim} flip {flip} shift {shift}: {int(bad.sum())} of {got.numel()} elements miss the bound, first at (row, column) {c}: "
            f"got {[float(got[i]) for i in c]}, want {[float(ref[i]) for i in c]}" + ("; the sin and cos halves are exchanged" if swapped else ""))


# ---- parameter preparation: (name, batch, R, C, Rp, Cp, src offset alignment remainder)
PREP_LEAVES = [("interior", 1, 256, 320, 256, 320, 0), ("padded", 1, 130, 72, 136, 72, 0), ("conv", 9, 4, 320, 8, 320, 0), ("small", 1, 33, 48, 40, 48, 0),
               ("odd_offset", 1, 64, 64, 64, 64, 2), ("interior_after_odd", 1, 128, 64, 128, 64, 0)]


def exact_case_bounds():
    """(what, bound on the largest partial or total, limit) for every exact reduction of tests/test_gpu_reduce_optim_exact.py."""
    out = []
    for n in SQNORM_SIZES:
        out.append((f"sqnorm n={n}", n * SQNORM_RANGE ** 2 + (1 << 30), 1 << 53))
    for n in SUMF64_SIZES:
        out.append((f"sum_f64 n={n}", n * SUMF64_RANGE + (1 << 30), 1 << 53))
    for name, B, C, H, W, cpad, wt, dp, l0 in MSE_CASES:
        cnt = B * C * H * W
        out.append((f"mse {name}", MSE_WMAX * MSE_DIFF2 * cnt + (l0 * cnt if cnt & (cnt - 1) == 0 else 0), LIMIT))
    for N, ld, rows, batch, r in COLSUM_CASES:
        out.append((f"colsum {(N, rows, batch)}", rows * r + 1000, LIMIT))
    for D, nseq, pat, vocab in EMB_CASES:
        out.append((f"embedding {(D, nseq, pat)}", 3 * nseq * EMB_S + 100, LIMIT))
    return out


# ================================================================================================ norms on balanced inputs
# (tests/test_gpu_norm_exact.py; their proof on the CPU: tests/test_kernel_checks_cpu.py)
#
# A norm divides by a standard deviation, so random inputs have no unique result.  Here every (image, group) - every LayerNorm row -
# holds only the two values c - s and c + s, equally often: mean c, variance s^2, xhat = +-1, all exact, and with gamma in {+-1, +-2}
# and an integer beta, |beta| > |gamma|, y = +-gamma + beta is a small non-zero integer.  The kernels' fp32 arithmetic is NOT exact
# (1 / count rounds, rsqrtf approximates, eps is added), but it moves a value by about 1e-5 relative and a bf16-representable value
# lies at least 2^-10 relative from the nearest rounding boundary: RNE lands on it, and the float64 result is the unique expectation.
NORM_COMBOS = [(-2, 1), (-1, 1), (-1, 2), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1)]  # (c, s), |c| + s <= 3; equal c only next to each other
NORM_DRES_BIG = (128, 255)  # |dres| of every fourth element: dx = +-0.5, +-1.5 plus one of these is a bf16 TIE (ulp 1 from 128 to 256)


NORM_COMBO_STEP, NORM_COMBO_IMAGE_STEP = 3, 5  # NORM_COMBOS entries 2, 3 or 5 apart (mod 8) never share c


def balanced_norm_inputs(nslices, n, seed, per_image=None):
    """Per slice (nslices of n elements, n % 4 == 0; images of per_image slices each, default: one image), float32 [nslices][n]:
      x = c + s * sign, sign = +-1 equally often in a seeded order, (c, s) = NORM_COMBOS[(3 * slice in its image + 5 * image + seed)
        % 8]: a slice never shares c with its neighbours (the group or row before and after), nor with the same group of the image
        before or after (index 5 apart) or two images away (10 = 2 apart), whatever the number of groups - so the true {sum, sumsq},
        mean and mostly rstd (6 index pairs of 8) differ from image to image and another image's statistics show;
      gdy = a + b * sign + r, what gamma * dy must be: a, b non-zero integers in +-{1, 2} per slice; r non-zero integers in +-{1, 2, 3}
        laid out as quadruples (u, -u, w, -w) on sign (+, +, -, -), so sum r = sum r * sign = 0 over the slice.
    Returns dict(x, sign, gdy, r, c, s, a, b) (c, s, a, b: float32 [nslices])."""
    assert n % 4 == 0, f"a slice of {n} elements cannot be balanced in quadruples"
    g = torch.Generator().manual_seed(seed)
    perm = torch.rand(nslices, n, generator=g).argsort(1)
    h, q = n // 2, n // 4
    sorted_sign = torch.cat([torch.ones(h), -torch.ones(h)]).expand(nslices, n)
    pm = lambda shape: torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    u = torch.randint(1, 4, (nslices, q), generator=g).float() * pm((nslices, q))
    w = torch.randint(1, 4, (nslices, q), generator=g).float() * pm((nslices, q))
    sorted_r = torch.cat([u, -u, w, -w], 1)
    sign = torch.empty(nslices, n).scatter_(1, perm, sorted_sign)
    r = torch.empty(nslices, n).scatter_(1, perm, sorted_r)
    per_image = nslices if per_image is None else per_image
    sl = torch.arange(nslices)
    k = (NORM_COMBO_STEP * (sl % per_image) + NORM_COMBO_IMAGE_STEP * (sl // per_image) + seed) % 8
    combos = torch.tensor(NORM_COMBOS, dtype=torch.float32)
    c, s = combos[k, 0], combos[k, 1]
    a = torch.randint(1, 3, (nslices,), generator=g).float() * pm((nslices,))
    b = torch.randint(1, 3, (nslices,), generator=g).float() * pm((nslices,))
    return dict(x=c[:, None] + s[:, None] * sign, sign=sign, gdy=a[:, None] + b[:, None] * sign + r, r=r, c=c, s=s, a=a, b=b)


def balanced_affine(C, seed):
    """gamma in {+-1, +-2}, beta an integer with |gamma| < |beta| <= |gamma| + 2 (float32 [C]); dgamma / dbeta previous values (non-zero integers)."""
    g = torch.Generator().manual_seed(seed)
    pm = lambda: torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    gamma = torch.randint(1, 3, (C,), generator=g).float() * pm()
    beta = (gamma.abs() + torch.randint(1, 3, (C,), generator=g).float()) * pm()
    prev_g = torch.randint(1, 100, (C,), generator=g).float() * pm()
    prev_b = torch.randint(1, 100, (C,), generator=g).float() * pm()
    return gamma, beta, prev_g, prev_b


def balanced_dres(shape, seed):
    """float32 integers: -3..3, and every fourth element (seeded phase) +-(128..255), which turns a half-odd dx into a tie."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randint(-3, 4, shape, generator=g).float()
    big = torch.randint(NORM_DRES_BIG[0], NORM_DRES_BIG[1] + 1, shape, generator=g).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    return torch.where(torch.randint(0, 4, shape, generator=g) == 0, big, d)


def _group_major(t, B, HW, G, cpg):
    """[B * G][HW * cpg] -> (B, HW, C)"""
    return t.view(B, G, HW, cpg).permute(0, 2, 1, 3).reshape(B, HW, G * cpg)


def groupnorm_balanced_case(B, HW, C, G, seed, dres=False):
    """dict(x, dy (bf16 (B, HW, C)), gamma, beta, prev_dgamma, prev_dbeta (float32 [C]), c, s, a, b (float32 (B, G)), r (float32 like
    x), cnt, and with dres: dres (bf16 like x)).  Element order inside a group is the kernels': pixel-major, channel-minor."""
    cpg = C // G
    n = HW * cpg
    sl = balanced_norm_inputs(B * G, n, seed, per_image=G)
    gamma, beta, pg, pb = balanced_affine(C, seed + 1)
    gm = lambda t: _group_major(t, B, HW, G, cpg)
    dy = gm(sl["gdy"]) / gamma
    out = dict(x=gm(sl["x"]).to(BF), dy=dy.to(BF), gamma=gamma, beta=beta, prev_dgamma=pg, prev_dbeta=pb, r=gm(sl["r"]), cnt=n,
               **{k: sl[k].view(B, G) for k in ("c", "s", "a", "b")})
    assert torch.equal(out["dy"].float(), dy), "dy is not exact in bf16"
    if dres:
        out["dres"] = balanced_dres((B, HW, C), seed + 2).to(BF)
    return out


def layernorm_balanced_case(M, C, seed, dres=False):
    """The LayerNorm form of groupnorm_balanced_case: x, dy (M, C); c, s, a, b [M]."""
    sl = balanced_norm_inputs(M, C, seed)
    gamma, beta, pg, pb = balanced_affine(C, seed + 1)
    dy = sl["gdy"] / gamma
    out = dict(x=sl["x"].to(BF), dy=dy.to(BF), gamma=gamma, beta=beta, prev_dgamma=pg, prev_dbeta=pb, r=sl["r"], cnt=C,
               **{k: sl[k] for k in ("c", "s", "a", "b")})
    assert torch.equal(out["dy"].float(), dy), "dy is not exact in bf16"
    if dres:
        out["dres"] = balanced_dres((M, C), seed + 2).to(BF)
    return out


def norm_exact_expectation(case, groups, eps_kernel):
    """The unique results of a balanced case from the ordinary float64 formula with eps = 0 (norm_ref_and_emulation's float64 branch),
    after asserting what makes them unique: y and dx are bf16-representable and non-zero, every sum is an integer (dgamma / dbeta:
    a multiple of 1/2) below 2^24.  Nothing of the kernels enters.
    Returns dict: y, dx (bf16), dx_dres (bf16, with dres: bf16(bf16(dx) + dres), two roundings), stats (float32 (B, G, 2) {sum, sumsq},
    GroupNorm), mean, rstd (float32 per slice), dgamma, dbeta (float64 sums WITHOUT the previous values), and for the counts that
    are not powers of two (eps_kernel > 0): ref / emu / terms of dgamma and dbeta at eps_kernel, for the per-channel rule."""
    x, dy, gamma, beta = case["x"], case["dy"], case["gamma"], case["beta"]
    ref, _, _ = norm_ref_and_emulation(x, gamma, beta, dy, groups, 0.0, False)
    out = {}
    for n in ("y", "dx"):
        v = ref[n]
        assert torch.equal(v.float().to(BF).double(), v), f"{n}: the float64 result is not bf16-representable"
        assert bool((v != 0).all()), f"{n}: a true zero - the kernel's perturbed value would not round to it"
        out[n] = v.float().to(BF)
    xd = x.double()
    if groups:
        B, HW, C = x.shape
        xg = xd.view(B, HW, groups, C // groups)
        stats = torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)
        assert float(stats.abs().max()) < LIMIT and torch.equal(stats, stats.round())
        out["stats"] = stats.float()
        mean, var = stats[..., 0] / case["cnt"], stats[..., 1] / case["cnt"] - (stats[..., 0] / case["cnt"]) ** 2
    else:
        assert float((xd * xd).sum(1).max()) < LIMIT
        mean, var = xd.mean(1), (xd * xd).mean(1) - xd.mean(1) ** 2
    assert torch.equal(mean, case["c"].double().view(mean.shape)) and torch.equal(var, (case["s"].double() ** 2).view(var.shape))
    out["mean"], out["rstd"] = mean.float(), (1.0 / var.sqrt()).float()
    assert torch.equal(out["rstd"].double() ** 2 * var, torch.ones_like(var))
    sgn = ((xd.view(-1, case["cnt"]) if not groups else xg.permute(0, 2, 1, 3).reshape(-1, case["cnt"])) - mean.reshape(-1, 1)).sign()
    rr = case["r"].double() / (case["s"].double().view(-1)[:, None] if not groups
                                else case["s"].double().repeat_interleave(C // groups, 1)[:, None, :])
    assert torch.equal(ref["dx"], rr), "dx is not r / s: the construction of dy is off"
    assert bool((sgn.abs() == 1).all())
    lead = tuple(range(x.dim() - 1))
    for n in ("dgamma", "dbeta"):
        v = ref[n]
        assert torch.equal(v * 2, (v * 2).round()), f"{n}: not a multiple of 1/2"
        mag = (dy.double().abs()).sum(lead)
        assert float(mag.max()) + 100 < LIMIT, f"{n}: partial sums may leave the exact range of fp32"
        out[n] = v
    if "dres" in case:
        out["dx_dres"] = (out["dx"].float() + case["dres"].float()).to(BF)  # fp32 sum of two bf16 values with |.| < 2^9: exact; then RNE
    if eps_kernel > 0:
        r2, e2, t2 = norm_ref_and_emulation(x, gamma, beta, dy, groups, eps_kernel, False)
        out["rule2"] = dict(ref={n: r2[n] for n in ("dgamma", "dbeta")}, emu={n: e2[n] for n in ("dgamma", "dbeta")}, terms=t2)
    return out


def param_grad_rule(got, prev, rule2, name):
    """The per-channel rule of the per-slice norm test (test_gpu_kernel_exact._norm_slices), for counts that are not powers of two:
    |got - prev - ref| / sum |terms| of the worst channel <= ROW_FACTOR x the torch fp32 emulation's, floored at 2^-24.
    Returns (message or None, kernel worst, emulation worst)."""
    rk = (got.double() - prev.double() - rule2["ref"][name]).abs() / rule2["terms"][name]
    re = (rule2["emu"][name] - rule2["ref"][name]).abs() / rule2["terms"][name]
    (ik, wk), (ie, we) = worst_slices(rk, 1)[0], worst_slices(re, 1)[0]
    ok = wk <= ROW_FACTOR * max(we, 2.0 ** -24)
    msg = None if ok else f"{name}: kernel worst channel {wk:.3e} at {ik} > {ROW_FACTOR} x max(emulation worst channel {we:.3e}, 2^-24)"
    return msg, wk, we


def is_pow2(n):
    return n & (n - 1) == 0


# ---- mirror of the GroupNorm launch geometry (norm.hip gn_layout, gn_chunks, gn_stat_chunks and the workspace queries)
GN_FINE_BLOCKS, GN_MAX_INLINE_PARTS, GN_L2_PARTS = 1024, 128, 32


def gn_layout(C):
    """(Cv, TX, TY, J): 8-channel vectors, threads across the vectors, thread rows (pixels in flight), vectors per thread."""
    Cv = C >> 3
    TX = min(Cv, 256)
    return Cv, TX, 256 // TX, -(-Cv // TX)


def gn_chunks(B, HW, C, stats):
    """(chunks per image, pixels per chunk) of the apply kernels (stats False) or of the statistics passes (at most 128 per image)."""
    target = max(GN_FINE_BLOCKS // B, 1)
    if stats:
        target = min(target, GN_MAX_INLINE_PARTS)
    ty = gn_layout(C)[2]
    ppb = max(-(-HW // target), 4 * ty)
    return -(-HW // ppb), ppb


def gn_fwd_workspace_bytes(B, HW, C, G):
    return max(gn_chunks(B, HW, C, True)[0], GN_L2_PARTS) * B * 2 * G * 4


def gn_bwd_workspace_bytes(B, HW, C):
    return gn_chunks(B, HW, C, True)[0] * B * (2 * C + 128) * 4


def gn_locate(B, HW, C, G, b, p, ch):
    """Where element (image b, pixel p, channel ch) is handled, as text for a failure report."""
    Cv, TX, TY, J = gn_layout(C)
    cv = ch >> 3
    out = [f"image {b} group {ch // (C // G)} (pixel {p}, channel {ch}; vector {cv} = thread column {cv % TX}, j = {cv // TX} of {J}, element {ch & 7})"]
    for stats in (False, True):
        nch, ppb = gn_chunks(B, HW, C, stats)
        out.append(f"{'statistics' if stats else 'apply'} pass: chunk {p // ppb} of {nch} ({ppb} pixels each, the last {HW - (nch - 1) * ppb}), "
                   f"thread row {(p % ppb) % TY} of {TY}")
    return "; ".join(out)


def gn_mismatch_report(got, want, what, B, HW, C, G):
    """mismatch_report over (B, HW, C) tensors, with the chunk and thread row of the first differing element."""
    msg = mismatch_report(got.reshape(B, HW, C), want.reshape(B, HW, C), what)
    if msg is None:
        return None
    i = int((bits(got.reshape(-1)) != bits(want.reshape(-1))).nonzero()[0])
    return msg + "\n  first: " + gn_locate(B, HW, C, G, i // (HW * C), (i // C) % HW, i % C)


def gn_parts_decomposition(totals, nparts, seed):
    """Integer rows [B][nparts][G][2] (float32) that add up to totals (B, G, 2): in every column the magnitudes 1 .. nparts in a seeded
    order (no two rows alike, so a difference names ONE row) with seeded signs; the last row takes the rest.  sum |rows| <= 2048 * 2049 / 2
    + |totals| stays below 2^24, so the sum is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    B, G, _ = totals.shape
    mag = torch.rand(B, nparts, G, 2, generator=g).argsort(1).float() + 1
    rows = mag * (torch.randint(0, 2, (B, nparts, G, 2), generator=g).float() * 2 - 1)
    rows[:, -1] = totals.float() - rows[:, :-1].sum(1)
    assert torch.equal(rows.double().sum(1), totals.double()) and float(rows.abs().sum(1).max()) < LIMIT
    return rows


def stats_report(got, want, what, parts=None):
    """stats (B, G, 2) against the exact totals: None, or sum_report's message for the first differing entry, which names the partial row
    (parts [B][nparts][G][2]) whose value the difference equals."""
    bad = (bits(got.float().contiguous()) != bits(want.float().contiguous())).nonzero()
    if bad.numel() == 0:
        return None
    b, g, w = (int(v) for v in bad[0])
    col = None if parts is None else parts[b, :, g, w]
    return f"{bad.shape[0]} of {got.numel()} statistics differ; " + sum_report(got[b, g, w], want[b, g, w], f"{what} image {b} group {g} {'sumsq' if w else 'sum'}", parts=col)


# ---- case tables (id, B, HW, C, G); the CPU proof holds the branch each id names to the mirror above
GN_BALANCED_CASES = [
    ("pow2_cpg2", 2, 64, 64, 32),                    # count 128: exact regime
    ("pow2_cpg8", 1, 256, 256, 32),                  # count 2048: exact regime
    ("cpg10_straddle_ty6", 3, 100, 320, 32),         # 8-wide vectors straddle groups, TY = 6 leaves 16 threads idle
    ("cpg3", 2, 36, 96, 32),
    ("cpg1_fewer_pixels_than_thread_rows", 1, 8, 32, 32),
    ("j2_ragged_second_vector", 2, 4, 2560, 32),
    ("g64_widest_c4096", 1, 60, 4096, 64),
    ("ty1_128_stat_rows_ragged_last", 2, 636, 2048, 32),  # 127 chunks of 5 pixels and one of 1; the apply pass cuts it in 159 chunks of 4
    ("g8", 2, 1028, 64, 8),
    ("g24_2g_not_dividing_256", 1, 16, 48, 24),
    ("g1", 2, 12, 8, 1),
]
# producer statistics: (case id of GN_BALANCED_CASES, nparts); <= 128 rows: the apply prologue; more: gn_group_reduce_kernel first
GN_PARTS_CASES = [(cid, n) for cid in ("pow2_cpg2", "cpg10_straddle_ty6") for n in (1, 2, 127, 128, 129, 200, 2048)] + [
    ("g24_2g_not_dividing_256", 7), ("g24_2g_not_dividing_256", 200), ("g64_widest_c4096", 129), ("g1", 200)]

# LayerNorm: (id, M, C)
LN_BALANCED_CASES = [
    ("smallest", 1, 8),
    ("nr4_clamped_tail_row", 5, 48),
    ("maxv2_nr2_odd_m", 33, 520),
    ("maxv4", 7, 2048),
    ("cv129_ragged_third_vector", 3, 1032),
    ("grid_stride_loop", 16389, 8),
    ("workload_308x768", 308, 768),
]
# CLIP pooling: (D, R, windows, S, eos_id (-1: argmax))
CLIP_POOL_CASES = [(8, 3, 2, 13, -1), (48, 4, 1, 77, 7), (1032, 3, 2, 11, -1), (2048, 3, 3, 9, 5)]


def gn_case(cid):
    return next(c for c in GN_BALANCED_CASES if c[0] == cid)


def ln_case(cid):
    return next(c for c in LN_BALANCED_CASES if c[0] == cid)


def gn_balanced(cid):
    """The operands of a GN_BALANCED_CASES row (seed: 100 + its place in the table), the same for the GPU file and its CPU proof."""
    _, B, HW, C, G = gn_case(cid)
    return groupnorm_balanced_case(B, HW, C, G, 100 + GN_BALANCED_CASES.index(gn_case(cid)), dres=True)


def ln_balanced(cid):
    """The operands of an LN_BALANCED_CASES row (seed: 200 + its place in the table)."""
    _, M, C = ln_case(cid)
    return layernorm_balanced_case(M, C, 200 + LN_BALANCED_CASES.index(ln_case(cid)), dres=True)


def ln_rows_per_block(C):
    """norm.hip ln_rows_per_block: rows one workgroup of four waves takes per pass (each wave NR = 4, 2 or 1 rows)."""
    return 16 if C <= 512 else 8 if C <= 1024 else 4


def ln_geometry(M, C):
    """Text for a failure report: the row split of ln_bwd_kernel (at most 1024 workgroups, grid-stride beyond)."""
    rpb = ln_rows_per_block(C)
    return f"rows per wave pass {rpb // 4}, rows per workgroup pass {rpb}, workgroups {min(1024, -(-M // rpb))}"


def clip_pool_case(D, R, windows, S, eos_id, seed):
    """ids (R * windows, S) int32 and the pooled positions: row r * windows has its key (the largest id for eos_id < 0, else eos_id)
    FIRST at pos[r] and again later where there is room; pos covers position 0, the last one (inside the ragged slab) and one in
    between; with eos_id >= 0 the last pooled row holds no EOS at all (position 0).  x (R * windows, S, D) bf16: integers in -3..3
    everywhere, a balanced row at every pooled position.  Returns dict(ids, pos, x, rows = layernorm_balanced_case(R, D))."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(10, 1000, (R * windows, S), generator=g).to(torch.int32)
    pos = torch.tensor([(0, S - 1, S // 2, 1)[r % 4] for r in range(R)], dtype=torch.int32)
    key = 5000 if eos_id < 0 else eos_id
    for r in range(R):
        if eos_id >= 0 and r == R - 1 and R > 1:
            pos[r] = 0
            continue
        p = int(pos[r])
        ids[r * windows, p] = key
        if p + 2 < S:
            ids[r * windows, p + 2] = key
    rows = layernorm_balanced_case(R, D, seed + 1)
    x = exact_ints((R * windows, S, D), -3, 3, seed + 2)
    for r in range(R):
        x[r * windows, int(pos[r])] = rows["x"][r]
    return dict(ids=ids, pos=pos, x=x, rows=rows)


# ================================================================================================ grouped off-chain launches
# (tests/test_gpu_grouped_exact.py; their proof on the CPU: tests/test_kernel_checks_cpu.py)
# sdt_attention_bwd_dkv_group: (B, H, Nq, Nk, D, kind, packed, key_weights, causal); kind "pair" (pair_case / pair_expect) or
# "selector" (selector_case / selector_expect).  Operands are seeded with Nq + Nk + D, as the single-launch tables are.
ATTN_CLASS_TOPS = (48, 64, 80, 96, 128, 160)  # the largest head dim of each instantiation (attention.hip attn_class)
ATTN_GROUP_LAUNCH = 8                         # problems per grouped launch (attention.hip ATTN_GROUP_MAX)
ATTN_GROUP_ABI = 32                           # problems per sdt_attention_bwd_dkv_group call


def _pair(B, H, Nq, Nk, D, packed=False):
    return (B, H, Nq, Nk, D, "pair", packed, False, False)


def _sel(B, H, Nq, Nk, D, key_weights=False, causal=False):
    return (B, H, Nq, Nk, D, "selector", False, key_weights, causal)


# One table for one call.  The eleven problems with D <= 48 (more than one launch of that instantiation) are spread between the other
# five instantiations, so the members of a class are picked out of the table, never a run of it.
DKV_GROUP_MIXED = [
    _pair(1, 1, 64, 77, 40),               # baseline
    _pair(1, 2, 64, 77, 64),
    _pair(3, 2, 70, 77, 40, True),         # ragged Nq, B = 3, halves of packed [k|v] / [dk|dv]
    _pair(1, 2, 1024, 77, 72, True),       # split
    _pair(2, 3, 64, 200, 32),              # two key blocks, unsplit (gx = 2), H = 3
    _pair(1, 2, 64, 77, 160),
    _pair(1, 2, 1024, 77, 40, True),       # split 4 x 256
    _pair(1, 2, 64, 77, 96),
    _pair(1, 1, 1030, 130, 48),            # split with two key blocks, 4 chunks of 320 (the last ragged), B*H*Nq % 4 == 2
    _sel(2, 2, 77, 77, 64, causal=True),
    _sel(2, 2, 64, 77, 8, key_weights=True),
    _pair(1, 2, 1024, 77, 120),            # split
    _pair(1, 1, 64, 16, 24),
    _pair(2, 1, 130, 77, 16),
    _sel(2, 2, 256, 77, 80, key_weights=True),
    _pair(1, 3, 64, 77, 48),
    _pair(1, 4, 128, 5, 16),               # odd tiny Nk
    _pair(1, 1, 64, 300, 152),             # three key blocks, unsplit
    _pair(1, 1, 64, 1, 8),                 # one key: dK exactly zero
]

# Ten split problems: nine of the instantiation D <= 48 (a second launch of it) and one of <128,5,3> at table index 1, so the
# finishing pass (two launches: table indices 0..7 and 8..9) is indexed differently from either dK/dV table.
DKV_GROUP_SPLITS = [
    _pair(1, 1, 1024, 16, 8), _pair(1, 2, 1024, 77, 72), _pair(1, 1, 1024, 33, 8), _pair(2, 1, 1024, 16, 8), _pair(1, 2, 1024, 20, 16),
    _pair(1, 1, 1280, 16, 8), _pair(1, 1, 1024, 77, 8),
    _pair(1, 1, 1600, 16, 8),              # plans 6 chunks, launches 5 of 320
    _pair(1, 2, 1024, 5, 8), _pair(1, 1, 1088, 2, 8),
]

# The ABI limit: 32 tiny pair problems over three instantiations (13 of D <= 48, 7 of D = 64, 12 of D in {72, 80}); B, H, Nq, Nk and D
# cycle with periods 2, 3, 2 (of three), 4 and 5
DKV_GROUP_FULL = [_pair(1 + i % 2, 1 + i % 3, (64, 70)[(i // 3) % 2], (2, 5, 16, 77)[i % 4], (8, 64, 80, 24, 72)[i % 5]) for i in range(ATTN_GROUP_ABI)]


def attention_class(D):
    """Index of the instantiation of head dim D (attention.hip attn_class)."""
    return next(i for i, top in enumerate(ATTN_CLASS_TOPS) if D <= top)


def group_key_weights(Nk):
    """Key weights of the grouped selector problems: 1, 2, 3 and 1/2 in turn (float32 (Nk,))."""
    return torch.tensor([1.0, 2.0, 3.0, 0.5])[torch.arange(Nk) % 4].contiguous()


def dkv_group_plan(spec):
    """(planned, chunk, launched, kblocks, gx) of one problem: attention_qsplit, the key blocks of 128, and the workgroups per (image,
    head) of its dK/dV pass (sdt_attention_bwd_dkv_group: kblocks * launched where it splits, else kblocks)."""
    B, H, Nq, Nk = spec[:4]
    planned, chunk, launched = attention_qsplit(B, H, Nq, Nk, spec[8])
    kblocks = -(-Nk // 128)
    return planned, chunk, launched, kblocks, kblocks * launched if planned > 1 else kblocks


def dkv_group_launches(table):
    """(dkv, finish): the launches of one sdt_attention_bwd_dkv_group call as lists of table indices - per instantiation in class
    order, ATTN_GROUP_LAUNCH problems each, then the finishing passes of the split problems in table order, eight each."""
    dkv = []
    for cls in range(len(ATTN_CLASS_TOPS)):
        mine = [i for i, s in enumerate(table) if attention_class(s[4]) == cls]
        dkv += [mine[j: j + ATTN_GROUP_LAUNCH] for j in range(0, len(mine), ATTN_GROUP_LAUNCH)]
    split = [i for i, s in enumerate(table) if dkv_group_plan(s)[0] > 1]
    return dkv, [split[j: j + ATTN_GROUP_LAUNCH] for j in range(0, len(split), ATTN_GROUP_LAUNCH)]


def dkv_group_cover(table, h_of_first=False):
    """The workgroups of the grouped dK/dV launches decoded as attn_bwd_dkv_group_kernel decodes them (problem by the prefix table,
    rest = local / gx, bx = local - rest * gx, b = rest / H, h = rest - b * H): a dict (table index, b, h, bx) -> how many workgroups
    land there.  h_of_first: the planted fault - every problem decoded with the H of its launch's first problem."""
    seen = {}
    for launch in dkv_group_launches(table)[0]:
        for i in launch:
            B, H = table[i][:2]
            gx = dkv_group_plan(table[i])[4]
            Hd = table[launch[0]][1] if h_of_first else H
            for local in range(gx * H * B):  # (the host sizes the prefix table with the problem's own B and H)
                rest, bx = divmod(local, gx)
                b, h = divmod(rest, Hd)
                seen[(i, b, h, bx)] = seen.get((i, b, h, bx), 0) + 1
    return seen


@functools.lru_cache(maxsize=None)
def dkv_group_problem(spec):
    """(case, want) of one table entry.  want: dict(o, dk, dv bf16; dq bf16 for pair problems, None for selector ones (zero by value,
    dk too); lse2 float64) - pair_expect with the problem's own query chunk, or selector_expect."""
    B, H, Nq, Nk, D, kind, packed, kw, causal = spec
    scale = D ** -0.5
    if kind == "pair":
        assert not kw and not causal
        case = pair_case(B, H, Nq, Nk, D, seed=Nq + Nk + D)
        planned, chunk, _ = attention_qsplit(B, H, Nq, Nk, False)
        exp = pair_expect(case, B, H, Nq, Nk, D, scale, kv_chunk=chunk if planned > 1 else None)
        return case, {n: exp[n] for n in ("o", "dq", "dk", "dv", "lse2")}
    case = selector_case(B, H, Nq, Nk, D, causal, seed=Nq + Nk + D)
    o, lse2, dv = selector_expect(case, B, H, Nq, Nk, D, scale, group_key_weights(Nk) if kw else None)
    return case, dict(o=o, dq=None, dk=torch.zeros_like(dv), dv=dv, lse2=lse2)


def dkv_group_expect(table, h_of_first=False):
    """Per table entry, the (dk, dv) the grouped call leaves: the problem's expectation on every (image, head, block of 128 keys)
    whose workgroups - one per launched query chunk where the pass splits - each occur exactly once under dkv_group_cover, NaN (an
    element nobody wrote) elsewhere.  With the true decode this is the expectation itself (the CPU proof asserts it)."""
    seen = dkv_group_cover(table, h_of_first)
    out = []
    for i, spec in enumerate(table):
        B, H, Nq, Nk, D = spec[:5]
        planned, chunk, launched, kblocks, gx = dkv_group_plan(spec)
        want = dkv_group_problem(spec)[1]
        dk, dv = (torch.full_like(want[n], float("nan")) for n in ("dk", "dv"))
        for b in range(B):
            for h in range(H):
                for kb in range(kblocks):
                    wgs = [c * kblocks + kb for c in range(launched)] if planned > 1 else [kb]
                    if all(seen.get((i, b, h, bx), 0) == 1 for bx in wgs):
                        rows, cols = slice(kb * 128, min(Nk, kb * 128 + 128)), slice(h * D, (h + 1) * D)
                        dk[b, rows, cols], dv[b, rows, cols] = want["dk"][b, rows, cols], want["dv"][b, rows, cols]
        out.append((dk, dv))
    return out


# sdt_colsum_batched_group: (N, ld, rows, batch, range) as COLSUM_CASES.  32 problems (the limit of one call): batch, rows, N and the
# pad of ld cycle with periods 5, 6, 6 (shifted every sixth entry) and 2; |value| <= 200 and rows <= 200 keep every sum below 2^24.
COLSUM_GROUP_ABI = 32
COLSUM_GROUP_MAXED = [((8, 13, 250, 256, 264, 520)[(i + i // 6) % 6], -(-(8, 13, 250, 256, 264, 520)[(i + i // 6) % 6] // 8) * 8 + 16 * (i % 2),
                       (1, 7, 63, 64, 65, 200)[i % 6], 1 + i % 5, 200) for i in range(COLSUM_GROUP_ABI)]


def colsum_group_workspace_bytes(table):
    """sdt_colsum_batched_group_workspace_bytes: the counters and every problem's partial rows (its single launch's: colsum_plan with
    the batched form's 512 blocks), back to back."""
    total = CNT_BYTES
    for N, ld, rows, batch, r in table:
        ncb, nby, rpb, want = colsum_plan(batch, rows, N, 512)
        total += 4 * ncb * batch * nby * 256
    return total
