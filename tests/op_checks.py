"""Exact-answer checks of the operator layer (stable_diffusion_training_amd/ops.py and the grouping helpers of nets.py): integer
parameter stores, the whole-gradient-buffer comparison, the references the kernel checkers (tests/kernel_checks.py) do not already
hold, and the case tables of tests/test_gpu_ops_exact.py.  Proved on the CPU by tests/test_op_checks_cpu.py.

The kernel files call the C ABI on raw pointers; this layer decides what those pointers and pitches ARE: padded leaf geometry
(Rp / Cp / R / C -> K1 / N / K1_valid / N_valid), merged launches (segment strides taken from master offsets), where a gradient lands
(views into the store's flat grad16 / grad buffers) and when (the deferred queues).  With integer masters and integer activations
every sum is an integer below 2^24, fp32 accumulation is exact in any order, and every output has ONE right bit pattern.

The gradient check never reads single leaves: it compares the store's WHOLE gradient buffers, so a write one leaf too far, a word in
an alignment gap or a leaf a dropped job never produced all show, with the leaf (or the gap) named."""
import torch

from tests import kernel_checks as kc

BF = kc.BF
QUANT_EXCLUDED = ("bias", "scale", "embedding")  # what the real stores keep out of quantisation: those gradients stay fp32
EMB_RANGE = 3


# ------------------------------------------------------------------------------------------------ integer stores
def _is_norm(spec_paths, path):
    """A norm's scale, or the bias that sits beside a scale."""
    head = path.rsplit("/", 1)[0]
    return path.endswith("/scale") or (path.endswith("/bias") and head + "/scale" in spec_paths)


class IntStore:
    """A params.ParamStore whose masters are seeded integers, loaded and prepared; self.w64 keeps the float64 copies for the
    references.  Kernels: -GEMM_RANGE..GEMM_RANGE; Dense / conv biases: -EPI_RANGE..EPI_RANGE; norm scale / bias: kc.balanced_affine
    (non-zero, |beta| > |gamma|); embeddings: -EMB_RANGE..EMB_RANGE.
    quantise=False: every gradient fp32 (store.grad).  quantise=True: biases, scales and embeddings excluded as in the real stores, so
    the kernel gradients live in bf16 (store.grad16, asserted) - pick kernel shapes whose numel is a multiple of the block size.
    norm_affine (optional): {norm name: (gamma, beta)} float32 to load instead of the seeded ones (the balanced norm cases);
    override (optional): {path: tensor} masters to load as they are (bf16-exact values: the selector projections)."""

    def __init__(self, spec, dev, seed, *, quantise, trainable=True, norm_affine=None, override=None):
        from stable_diffusion_training_amd import params
        spec = [(p, tuple(s)) for p, s in spec]
        paths = {p for p, _ in spec}
        self.spec = spec
        self.st = params.ParamStore(spec, device=dev, quantise=quantise, quant_excluded=QUANT_EXCLUDED if quantise else (),
                                    trainable=trainable)
        self.w64 = {}
        for i, (p, shp) in enumerate(spec):
            s = seed * 1009 + 31 * i
            if override is not None and p in override:
                v = override[p].float().reshape(shp)
            elif _is_norm(paths, p):
                name = p.rsplit("/", 1)[0]
                if norm_affine is not None and name in norm_affine:
                    gamma, beta = norm_affine[name]
                else:
                    gamma, beta, _, _ = kc.balanced_affine(shp[0], seed * 1009 + 31 * sorted(paths).index(name + "/scale"))
                v = gamma if p.endswith("/scale") else beta
            elif p.endswith("/kernel"):
                v = kc.exact_ints(shp, -kc.GEMM_RANGE, kc.GEMM_RANGE, s, dtype=torch.float32)
            elif p.endswith("/bias"):
                v = kc.exact_ints(shp, -kc.EPI_RANGE, kc.EPI_RANGE, s, dtype=torch.float32)
            else:
                v = kc.exact_ints(shp, -EMB_RANGE, EMB_RANGE, s, dtype=torch.float32)
            self.w64[p] = v.double()
        self.st.load({p: v.float() for p, v in self.w64.items()})
        if self.st.device.type == "cuda":
            self.st.prepare()
        if quantise and trainable:
            assert self.st.grad16 is not None, "a quantised integer store must keep its kernel gradients in grad16"
            assert all(self.st.leaves[p].quantised == p.endswith("/kernel") for p in paths)
        if not quantise and trainable:
            assert self.st.grad16 is None

    def w(self, name):
        return self.w64[name + "/kernel"]

    def b(self, name):
        return self.w64.get(name + "/bias")


# ------------------------------------------------------------------------------------------------ the whole-buffer gradient check
def written_paths(store):
    """Leaves the weight-gradient kernels WRITE (one writer, no zero fill): matrix kernels and the biases beside them - the rule of
    ParamStore._build_zero_ranges.  Every other leaf (norm parameters, embeddings) is accumulated into and starts a step at zero."""
    out = set()
    for p, lf in store.leaves.items():
        if lf.w_off >= 0 and p not in store._unused:
            out.add(p)
            b = p[: -len("kernel")] + "bias"
            if b in store.leaves and b not in store._unused:
                out.add(b)
    return out


def _buffers(store):
    """[(name, tensor, first master element, one past the last master element)] of the gradient buffers."""
    out = []
    if store.grad16 is not None:
        out.append(("grad16", store.grad16, 0, store.quant_total))
    if store.total > store.g32_base:  # (a store without fp32 leaves keeps a 4-element placeholder no sweep reads: not part of the gradient)
        out.append(("grad", store.grad[: store.total - store.g32_base], store.g32_base, store.total))
    return out


def sentinel_int(dtype):
    """kc.SENTINEL[dtype] as the signed integer an integer view holds."""
    s, top = kc.SENTINEL[dtype], 1 << (8 * torch.empty(0, dtype=dtype).element_size())
    return s - top if s >= top // 2 else s


def fill_sentinel(store):
    """Every element of both gradient buffers holds the NaN sentinel of its type (kc.SENTINEL)."""
    store.fill_grad(float("nan"))
    for _, buf, _, _ in _buffers(store):
        buf.view(kc._INT_VIEW[buf.dtype]).fill_(sentinel_int(buf.dtype))


def host_zero_grad(store):
    """What ParamStore.zero_grad() leaves, done on the host (the CPU proof has no sdt_zero_ranges): everything outside the written
    leaves - the accumulated-into leaves and every alignment gap - is +0.0; the written leaves keep what they held."""
    store._written = set()
    keep = written_paths(store)
    for _, buf, lo, hi in _buffers(store):
        mask = torch.ones(buf.numel(), dtype=torch.bool)
        for p in keep:
            lf = store.leaves[p]
            if lo <= lf.offset < hi:
                mask[lf.offset - lo: lf.offset - lo + lf.numel] = False
        buf[mask.to(buf.device)] = 0


def arm_gradient(store, zero=None):
    """Steps 1 of the check: sentinel everywhere, then zero_grad() (zero: a stand-in for it on the CPU).  Returns the snapshot of both
    buffers that expect_whole_gradient measures "untouched" against."""
    fill_sentinel(store)
    (zero or (lambda s: s.zero_grad()))(store)
    if store.device.type == "cuda":
        torch.cuda.synchronize()
    return {name: buf.detach().cpu().clone() for name, buf, _, _ in _buffers(store)}


def _locate(store, i):
    """Master element i -> (leaf path, index inside the leaf) or (None, 'gap after leaf X, element k')."""
    prev = None
    for p in store.order:
        lf = store.leaves[p]
        if lf.offset <= i < lf.offset + lf.numel:
            return p, i - lf.offset
        if lf.offset > i:
            break
        prev = lf
    if prev is None:
        return None, f"gap before the first leaf, element {i}"
    return None, f"gap after leaf {prev.path}, element {i - prev.offset - prev.numel}"


def expected_buffers(store, expected, armed):
    """{buffer name: tensor} of what the buffers must hold: a written leaf its reference (bf16 RNE of the integer in grad16, the fp32
    integer in grad); an accumulated-into leaf its reference added onto what zero_grad() left; a leaf no op touched what zero_grad()
    left (the snapshot); every alignment gap +0.0."""
    written = written_paths(store)
    out = {}
    for name, buf, lo, hi in _buffers(store):
        want = armed[name].clone()
        gap = torch.ones(want.numel(), dtype=torch.bool)
        for p in store.order:
            lf = store.leaves[p]
            if not (lo <= lf.offset < hi):
                continue
            sl = slice(lf.offset - lo, lf.offset - lo + lf.numel)
            gap[sl] = False
            if p not in expected:
                continue
            v = expected[p].double().reshape(-1).cpu()
            assert v.numel() == lf.numel, f"{p}: expectation has {v.numel()} elements, the leaf {lf.numel}"
            if p not in written:
                v = want[sl].double() + v  # += onto what zero_grad() left
            if want.dtype == BF:
                want[sl] = kc.rne_bf16(v)
            else:
                v32 = v.float()
                assert torch.equal(v32.double(), v), f"{p}: expectation not exact in fp32"
                want[sl] = v32
        want[gap] = 0.0
        out[name] = want
        for p in expected:
            assert p in store.leaves, f"{p}: no such leaf"
    return out


def whole_gradient_report(store, expected, armed, what="gradient", limit=6):
    """None when every element of grad16 and grad holds the expected bits; otherwise a message in the manner of kc.mismatch_report:
    the count, then for the first mismatches the buffer, the leaf with the coordinates inside it (or 'gap after leaf X, element k'),
    both values and the bit pattern found."""
    if store.device.type == "cuda":
        torch.cuda.synchronize()
    want = expected_buffers(store, expected, armed)
    lines, total = [], 0
    for name, buf, lo, hi in _buffers(store):
        got = buf.detach().cpu()
        bad = (kc.bits(got) != kc.bits(want[name])).nonzero().reshape(-1)
        total += bad.numel()
        mask = (1 << (8 * got.element_size())) - 1
        for i in bad[: max(limit - len(lines), 0)].tolist():
            p, k = _locate(store, i + lo)
            if p is None:
                where = k
            else:
                shape = store.leaves[p].shape
                state = "" if p in expected else " (no op of the case writes it)"
                where = f"leaf {p} at {kc._coords(torch.tensor([k]), shape)[0]}{state}"
            sent = (int(kc.bits(got[i: i + 1])[0]) & mask) == kc.SENTINEL[got.dtype]
            lines.append(f"  {name}[{i}] {where}: got {got[i].item()!r} (0x{int(kc.bits(got[i: i + 1])[0]) & mask:x}"
                         f"{', the sentinel: never written' if sent else ''}), want {want[name][i].item()!r}")
    if not total:
        return None
    return "\n".join([f"{what}: {total} elements of the gradient buffers differ"] + lines)


def expect_whole_gradient(store, expected, armed, what="gradient"):
    msg = whole_gradient_report(store, expected, armed, what)
    assert msg is None, msg


def stored_sq_sum(store, expected):
    """float64 sum of squares of what the quantised leaves of `expected` hold once stored (bf16 in grad16): integers, exact in double."""
    tot = 0.0
    for p, v in expected.items():
        if store.leaves[p].quantised:
            s = (kc.rne_bf16(v.double().cpu()) if store.grad16 is not None else v).double()
            tot += float((s * s).sum())
    assert tot < 2.0 ** 53
    return tot


# ------------------------------------------------------------------------------------------------ padding and segments
def pad_last(t, width, seed=None):
    """t (..., C) -> (..., width): the pad columns hold zeros, or with a seed NON-ZERO integers in +-1..3 (an operand whose pad
    columns must not reach the result: only the zero padding of W and K1_valid / N_valid keep them out)."""
    C = t.shape[-1]
    if width == C:
        return t.clone()
    out = torch.zeros(*t.shape[:-1], width, dtype=t.dtype)
    out[..., :C] = t
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        shp = (*t.shape[:-1], width - C)
        out[..., C:] = (torch.randint(1, 4, shp, generator=g) * (torch.randint(0, 2, shp, generator=g) * 2 - 1)).to(t.dtype)
    return out


def pad_weight(w64, Rp, Cp):
    """(..., R, C) -> (..., Rp, Cp), zero padded: the bf16 compute copy of a padded leaf."""
    out = torch.zeros(*w64.shape[:-2], Rp, Cp, dtype=w64.dtype)
    out[..., : w64.shape[-2], : w64.shape[-1]] = w64
    return out


def pad8(n):
    return (n + 7) // 8 * 8


def per_image_colsum(dy, B):
    """float64 (B, C): the column sums of each image's rows of dy (B, ..., C) - the gradient of a broadcast row bias."""
    return dy.double().reshape(B, -1, dy.shape[-1]).sum(1)


def segments(t, n):
    """The n equal column segments of a merged (..., n * N) tensor."""
    N = t.shape[-1] // n
    return [t[..., i * N: (i + 1) * N] for i in range(n)]


def wide_with_slice(slice_value, n, which, seed):
    """A (rows, n * C) bf16 tensor whose column slice `which` is slice_value (rows, C) and whose other slices hold other, non-zero
    integers: a consumer that reads the slice at the wrong pitch or offset picks those up."""
    rows, C = slice_value.shape
    wide = kc.exact_ints((rows, n * C), 1, kc.EPI_RANGE, seed)
    wide[:, which * C: (which + 1) * C] = slice_value
    return wide


# ------------------------------------------------------------------------------------------------ references
def linear_expect(x, w64, b64, res, dy, need_dx=True):
    """ops.linear on a leaf (R, C) padded to (Rp, Cp) = (x.shape[-1], dy.shape[-1]): x (M, Rp), dy and res (M, Cp) bf16 integers
    (pad columns of x and dy non-zero).  Returns dict(y, dx: bf16; dW (R, C), db (C): float64)."""
    R, C = w64.shape
    Rp, Cp = x.shape[-1], dy.shape[-1]
    Wp = pad_weight(w64, Rp, Cp)
    bp = None if b64 is None else pad_last(b64, Cp)
    out = dict(y=kc.expect_gemm_nt(x, Wp, bias=bp, residual=res))
    if need_dx:
        out["dx"] = kc.rne_bf16(dy.double() @ Wp.t() + 0.0)
    out["dW"] = (x.double().t() @ dy.double())[:R, :C] + 0.0  # (+ 0.0: an accumulator that starts at +0 never ends at -0)
    if b64 is not None:
        out["db"] = dy.double().sum(0)[:C] + 0.0
    return out


def conv_expect(x, w64, b64, rowbias, res, dy, stride, pad):
    """ops.conv2d on a leaf (k, k, R, C) padded to (Rp, Cp): x (B, H, W, Rp), dy / res (B, OH, OW, Cp), rowbias (B, Cp) bf16 integers.
    Returns dict(y, dx, drb: bf16; dW (k, k, R, C), db (C): float64)."""
    pad = kc.norm_pad(pad)
    k, _, R, C = w64.shape
    B, H, W, Rp = x.shape
    Cp = dy.shape[-1]
    Wp = pad_weight(w64, Rp, Cp)
    OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
    acc = kc.conv_ref64(x, Wp, stride, pad).reshape(-1, Cp) + 0.0
    y = kc.epilogue_nt(acc, None if b64 is None else pad_last(b64, Cp), rowbias, None if res is None else res.reshape(-1, Cp), OH * OW)
    out = dict(y=y.view(B, OH, OW, Cp), dx=kc.rne_bf16(kc.conv_dgrad_ref64(dy, Wp, (H, W), stride, pad) + 0.0),
               dW=kc.conv_wgrad_ref64(x, dy, (k, k), stride, pad)[:, :, :R, :C] + 0.0)
    if b64 is not None:
        out["db"] = dy.double().sum((0, 1, 2))[:C] + 0.0
    if rowbias is not None:
        out["drb"] = kc.rne_bf16(per_image_colsum(dy, B) + 0.0)
    return out


def linear_multi_expect(x, w64s, b64s, dy, per_layer=False):
    """ops.linear_multi over n unpadded leaves (K, N): y (M, n * N) per segment, dx = the sum over the segments (ONE fp32 reduction of
    n * N terms, rounded once), dW / db per leaf.  per_layer: also assert that the per-layer path (n input gradients rounded to
    bf16 each, then summed by ops.fanout and rounded again) gives the same dx - every partial and the total are exact in bf16."""
    n = len(w64s)
    ys, dWs, dbs, acc, parts = [], [], [], 0, []
    for i, dyi in enumerate(segments(dy, n)):
        ys.append(kc.expect_gemm_nt(x, w64s[i], bias=None if b64s is None else b64s[i]))
        parts.append(dyi.double() @ w64s[i].t())
        acc = acc + parts[-1]
        dWs.append(x.double().t() @ dyi.double() + 0.0)
        dbs.append(dyi.double().sum(0) + 0.0)
    dx = kc.rne_bf16(acc + 0.0)
    if per_layer:
        two_step = kc.rne_bf16(sum(kc.rne_bf16(p + 0.0).double() for p in parts))
        assert torch.equal(kc.bits(two_step), kc.bits(dx)) and torch.equal(dx.double(), acc + 0.0), \
            "linear_multi: the per-layer input gradients are not exact in bf16, the two paths would round differently"
    return dict(y=torch.cat(ys, -1), dx=dx, dW=dWs, db=dbs)


def upsample_bwd_expect(dy):
    """dx (B, H, W, C) of the nearest 2x upsampling: the sum of the four output pixels, rounded once."""
    B, H2, W2, C = dy.shape
    return kc.rne_bf16(dy.double().view(B, H2 // 2, 2, W2 // 2, 2, C).sum((2, 4)))


def fanout_grads(shape, n, silent, seed):
    """n gradients (None at the indices `silent`) of integers whose running sum stays within +-256 at every prefix: each is in
    -(256 // n)..(256 // n), so the bf16 store between two chained launches is exact.  Returns (list, float64 sum)."""
    r = max(256 // n, 1)
    gs = [None if i in silent else kc.exact_ints(shape, -r, r, seed + i) for i in range(n)]
    tot = sum(g.double() for g in gs if g is not None)
    return gs, tot


def context_selector_case(B, Nq, Nk, cd, C, heads, n, seed, c=32.0):
    """Inputs that make the cross-attention behind nets._context_projections an exact gather (the construction of kc.selector_case,
    with the keys PROJECTED): ctx (B, Nk, cd) carries, on its first nb = ceil(log2 Nk) columns, the +-1 code bits of a seeded
    permutation of the key slots and integers in -3..3 elsewhere; every to_k kernel (cd, C) maps code bit r to feature r of every head
    with weight c (zero elsewhere), so k = ctx @ Wk holds c * code in every head and is exact in bf16; the to_v kernels are ordinary
    integers; the queries of block i carry the code of their target key.  The winner leads by >= 2 c^2 / sqrt(D) logits: P is one-hot.
    Returns dict(ctx bf16, wk (cd, C) float32, q [n] bf16 (B, Nq, C), dout [n] bf16, target [n] int64 (B, heads, Nq), nbits)."""
    import math
    D = C // heads
    nb = max(1, math.ceil(math.log2(max(Nk, 2))))
    assert nb <= D and nb < cd and Nq <= Nk
    g = torch.Generator().manual_seed(seed)
    sh = torch.arange(nb)
    ctx = torch.randint(-3, 4, (B, Nk, cd), generator=g).float()
    codes = torch.empty(B, Nk, nb)
    for b in range(B):
        s = torch.randperm(Nk, generator=g)
        codes[b] = (((s[:, None] >> sh) & 1) * 2 - 1).float()
    ctx[:, :, :nb] = codes
    wk = torch.zeros(cd, C)
    for h in range(heads):
        wk[sh, h * D + sh] = c
    qs, dos, targets = [], [], []
    for i in range(n):
        t = torch.stack([torch.stack([torch.randperm(Nk, generator=g)[:Nq] for _ in range(heads)]) for _ in range(B)])  # each key at most once
        q = torch.zeros(B, Nq, heads, D)
        for b in range(B):
            for h in range(heads):
                q[b, :, h, :nb] = codes[b][t[b, h]] * c
        qs.append(q.reshape(B, Nq, C).to(BF))
        dos.append(torch.randint(-3, 4, (B, Nq, C), generator=g).to(BF))
        targets.append(t)
    return dict(ctx=ctx.to(BF), wk=wk, q=qs, dout=dos, target=targets, nbits=nb, c=c)


def context_selector_expect(case, wv64s, heads):
    """Per block i: kv (B, Nk, 2C) bf16 = [ctx @ Wk | ctx @ Wv_i], out (the selected V rows), dkv = [0 | dv_i]; and dctx, the ONE
    reduction over all [dk|dv] segments, with the to_k / to_v weight gradients (float64)."""
    ctx = case["ctx"]
    B, Nk, cd = ctx.shape
    C = case["wk"].shape[1]
    D = C // heads
    x2 = ctx.reshape(-1, cd)
    k = kc.expect_gemm_nt(x2, case["wk"]).view(B, Nk, C)
    out = dict(kv=[], out=[], dkv=[], dWk=[], dWv=[])
    acc = torch.zeros(B * Nk, cd, dtype=torch.float64)
    for i, wv in enumerate(wv64s):
        v = kc.expect_gemm_nt(x2, wv).view(B, Nk, C)
        t, do = case["target"][i], case["dout"][i]
        Nq = do.shape[1]
        o = torch.empty(B, Nq, heads, D, dtype=BF)
        dv = torch.zeros(B, Nk, heads, D, dtype=torch.float64)
        for b in range(B):
            for h in range(heads):
                o[b, :, h] = v.view(B, Nk, heads, D)[b, t[b, h], h]
                dv[b, :, h].index_add_(0, t[b, h], do.view(B, Nq, heads, D)[b, :, h].double())
        dv = kc.rne_bf16(dv.reshape(B, Nk, C))
        out["kv"].append(torch.cat([k, v], -1))
        out["out"].append(o.reshape(B, Nq, C))
        out["dkv"].append(torch.cat([torch.zeros_like(dv), dv], -1))
        out["dWk"].append(torch.zeros(cd, C, dtype=torch.float64))
        out["dWv"].append(x2.double().t() @ dv.double().reshape(-1, C) + 0.0)
        acc = acc + dv.double().reshape(-1, C) @ wv.t()
    out["dctx"] = kc.rne_bf16(acc + 0.0).view(B, Nk, cd)
    return out


# ------------------------------------------------------------------------------------------------ output checks
def pad_columns_report(y, C, what):
    """None when y[..., C:] is +0.0 everywhere, else a kc.mismatch_report naming the coordinates."""
    if y.shape[-1] == C:
        return None
    padc = y[..., C:].detach().cpu()
    return kc.mismatch_report(padc, torch.zeros_like(padc), f"{what}: pad columns {C}..{y.shape[-1] - 1} (coordinates count from column {C})")


def output_reports(got, want, C=None):
    """Messages for every output of a case: got / want {name: tensor}; C: valid output columns of 'y' (pad columns must be +0.0)."""
    msgs = []
    for n, w in want.items():
        if n in got and torch.is_tensor(w) and w.dtype == BF:
            m = kc.mismatch_report(got[n].detach().cpu(), w, n)
            if m:
                msgs.append(m)
    if C is not None and "y" in got:
        m = pad_columns_report(got["y"], C, "y")
        if m:
            msgs.append(m)
    return msgs


# ------------------------------------------------------------------------------------------------ case tables
# ops.linear: (id, M, K (in-features), N (out-features)) and the host-side decision each row is there for
LINEAR_CASES = [
    ("m1_k8_n8", 1, 8, 8),                 # the smallest leaf: lda = ldb = 8, one row
    ("m130_k72_n136", 130, 72, 136),       # ragged M, K and N on the 64-tiles: K1 / N handed over unpadded and odd
    ("m129_k320_n320", 129, 320, 320),     # M % 128 == 1; the weight gradient on 128-tiles
    ("pad_in_130", 77, 130, 72),           # padded in-features: Rp 136, K1_valid 130, W read from its own zero-padded slot
    ("pad_out_4", 100, 64, 4),             # padded out-features: Cp 8, N_valid 4, _padded_bias, ldw = 4
    ("splitk", 200, 4104, 72),             # split-K through the persistent _splitk_workspace (kc.GEMM_PLAIN_CASES "splitk64")
]

# ops.linear_multi: (id, M, K, N, n, bias)
LINEAR_MULTI_CASES = [
    ("n3_bias", 100, 64, 64, 3, True),     # b_nseg / b_seg_stride, seg_stride from master offsets, ONE dbias pointer for n leaves
    ("n2_nobias", 77, 72, 128, 2, False),  # ragged K, no bias: dbias None
]

# ops.conv2d: (B, H, W, Cin, Cout, k, stride, pad) and what each row reaches
CONV_CASES = [
    (2, 16, 16, 64, 64, 3, 1, 1),                  # the halo kernel; tap stride Rp * Cp
    (2, 16, 16, 64, 128, 3, 2, 1),                 # stride 2: out_h / out_w of the geometry
    (2, 16, 16, 64, 64, 3, 2, ((0, 1), (0, 1))),   # stride 2, asymmetric pad: pt / pl only reach the kernel
    (2, 8, 8, 128, 64, 1, 1, 0),                   # 1x1: the plain path and wgrad_dense
    (2, 36, 28, 64, 64, 3, 1, 1),                  # generic, untileable
    (2, 12, 20, 4, 32, 3, 1, 1),                   # padded leaf, conv_in: Rp 8, K1_valid 4
    (2, 12, 20, 9, 32, 3, 1, 1),                   # padded leaf, inpaint conv_in: Rp 16
    (2, 12, 20, 3, 32, 3, 1, 1),                   # padded leaf, VAE pixels
    (2, 16, 16, 320, 4, 3, 1, 1),                  # padded leaf, conv_out: Cp 8, N_valid 4
    (2, 16, 16, 64, 3, 3, 1, 1),                   # padded leaf, VAE out
]

# grouping limits: 33 distinct Dense shapes (K, N) with M = 16, 9 convolutions, 3 LayerNorms in ONE wgrad_grouping context
GROUP_M = 16
GROUP_DENSE = [(8 + 8 * (i % 9), 8 + 8 * ((5 * i) % 17)) for i in range(33)]   # K 8..72, N 8..136, no pair twice (9 and 17 coprime)
GROUP_CONVS = [(4, 8, 8, 128, 72)] * 5 + [(2, 12, 20, 8, 32)] * 4   # (B, H, W, Cin, Cout), 3x3 / stride 1 / pad 1
GROUP_LN = [("nr4_clamped_tail_row", 0), ("nr4_clamped_tail_row", 1), ("smallest", 2)]  # (kc.LN_BALANCED_CASES id, seed shift)

# norm operators: the smallest balanced rows with a straddling group / a ragged row block
GN_OP_CASE = "cpg3"                    # 3 channels per group: the 8-wide vectors straddle groups (96 channels, 36 pixels, 2 images)
GN_EXACT_CASE = "pow2_cpg2"            # count 128, a power of two: dgamma / dbeta are exact too, so the whole-buffer check applies
LN_OP_CASE = "nr4_clamped_tail_row"    # 5 rows of 48: the last wave's rows are clamped

# ops.fanout: (n, consumers that give no gradient): 2 gradients; 31 = one full launch; 38 = a second launch chained onto the first
FANOUT_CASES = [(3, (1,)), (32, (5,)), (40, (0, 17))]

# attention operators
ATTN_OP = dict(B=2, H=3, D=40, Nq=136, Nk=200)

# the fused feed-forward kernel at a ragged M: (F, K) -> [smallest served M, smallest with M % 128 == 1, smallest with M % 128 == 127]
FF_GEGLU_PAIRS = [(256, 64), (1280, 320)]
FF_GEGLU_M = {(256, 64): (8065, 8065, 8191), (1280, 320): (1537, 1537, 1663)}


def linear_operands(case, has_bias=True, has_res=True):
    """(spec, seed, x (M, Rp), dy (M, Cp), res (M, Cp) or None) of a LINEAR_CASES row: the same on the GPU and in the CPU proof.
    Pad columns of x and dy are non-zero, those of the residual zero (it is an earlier output)."""
    name, M, K, N = case
    g, e = kc.GEMM_RANGE, kc.EPI_RANGE
    seed = 100 + 10 * LINEAR_CASES.index(case)
    spec = [("l/kernel", (K, N))] + ([("l/bias", (N,))] if has_bias else [])
    x = pad_last(kc.exact_ints((M, K), -g, g, seed + 1), pad8(K), seed=seed + 2)
    dy = pad_last(kc.exact_ints((M, N), -g, g, seed + 3), pad8(N), seed=seed + 4)
    res = pad_last(kc.exact_ints((M, N), -e, e, seed + 5), pad8(N)) if has_res else None
    return spec, seed, x, dy, res


def multi_operands(case):
    """(names, seed, x (M, K), dy (M, n * N) in -1..1) of a LINEAR_MULTI_CASES row.  dy stays in -1..1 so that every per-layer input
    gradient is exact in bf16 and the per-layer path must give the merged launch's bits (linear_multi_expect(per_layer=True))."""
    name, M, K, N, n, bias = case
    seed = 300 + 10 * LINEAR_MULTI_CASES.index(case)
    return ([f"p{i}" for i in range(n)], seed, kc.exact_ints((M, K), -kc.GEMM_RANGE, kc.GEMM_RANGE, seed + 1),
            kc.exact_ints((M, n * N), -1, 1, seed + 2))


def multi_spec(names, K, N, bias, layout):
    """grouped: kernels back to back, then biases back to back (what the real specs emit); interleaved: a small spacer layer after
    every layer, in the kernels' segment and in the biases' alike, so the leaves are not adjacent whatever the store's segments do."""
    if layout == "grouped":
        return [(nm + "/kernel", (K, N)) for nm in names] + ([(nm + "/bias", (N,)) for nm in names] if bias else [])
    spec = []
    for i, nm in enumerate(names):
        spec.append((nm + "/kernel", (K, N)))
        if bias:
            spec.append((nm + "/bias", (N,)))
        spec += [(f"gap{i}/kernel", (8, 16)), (f"gap{i}/bias", (16,))]
    return spec


def conv_operands(case):
    """(spec, seed, x (B, H, W, Rp), dy, res (B, OH, OW, Cp), rb (B, Cp), wide (B, 3 * Cp) with rb as its middle slice) of a CONV_CASES
    row.  Pad channels of x and dy are non-zero; those of the residual and of the row bias are zero."""
    B, H, W, Cin, Cout, k, stride, pad = case
    g, e = kc.GEMM_RANGE, kc.EPI_RANGE
    seed = 500 + 10 * CONV_CASES.index(case)
    Rp, Cp = pad8(Cin), pad8(Cout)
    OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
    x = pad_last(kc.exact_ints((B, H, W, Cin), -g, g, seed + 1), Rp, seed=seed + 2)
    dy = pad_last(kc.exact_ints((B, OH, OW, Cout), -g, g, seed + 3), Cp, seed=seed + 4)
    res = pad_last(kc.exact_ints((B, OH, OW, Cout), -e, e, seed + 5), Cp)
    rb = pad_last(kc.exact_ints((B, Cout), -e, e, seed + 6), Cp)
    spec = [("c/kernel", (k, k, Cin, Cout)), ("c/bias", (Cout,))]
    return spec, seed, x, dy, res, rb, wide_with_slice(rb, 3, 1, seed + 7)


def ff_geglu_served(supported, F, K, limit=1 << 15):
    """The three M of section FF_GEGLU_M from the host function `supported(M, F, K)`."""
    served = [M for M in range(1, limit) if supported(M, F, K)]
    return (served[0], next(M for M in served if M % 128 == 1), next(M for M in served if M % 128 == 127))


def exact_bounds():
    """(what, bound on the largest |partial sum|) of every contraction the operator cases run; the CPU proof asserts each < 2^24
    (and recomputes the bound on the very operands for one case per family)."""
    g, e = kc.GEMM_RANGE, kc.EPI_RANGE
    out = []
    for name, M, K, N in LINEAR_CASES:
        out += [(f"linear {name} y", g * g * pad8(K) + 2 * e), (f"linear {name} dx", g * g * pad8(N)), (f"linear {name} dW", g * g * M)]
    for name, M, K, N, n, _ in LINEAR_MULTI_CASES:
        out += [(f"multi {name} y", g * g * K + e), (f"multi {name} dx", g * g * n * N), (f"multi {name} dW", g * g * M)]
    for B, H, W, Cin, Cout, k, stride, pad in CONV_CASES:
        OH, OW = kc.conv_out_hw(H, W, k, stride, pad)
        out += [(f"conv {(B, H, W, Cin, Cout)} y", g * g * k * k * pad8(Cin) + 3 * e), (f"conv {(B, H, W, Cin, Cout)} dx", g * g * k * k * pad8(Cout)),
                (f"conv {(B, H, W, Cin, Cout)} dW", g * g * B * OH * OW)]
    return out
