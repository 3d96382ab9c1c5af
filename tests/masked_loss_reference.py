"""Reference of the masked / per-sample weighted loss (include/sdt.h "MASKED LOSS"): float64 numpy for the pooled mask, the effective
mask, the per-sample sums, the loss, the per-sample loss and the gradient, and the float32 emulation of the kernels' rounding chain for
the masks and dpred.  Layouts: mask (B, h*f, w*f), pred (B, h, w, C) (the real channels of the NHWC prediction), target (B, C, h, w)."""
import numpy as np
import torch

F32 = np.float32
FACTORS = (1, 2, 4, 8, 16)


def clamp01(m):
    """fminf(fmaxf(m, 0), 1): a NaN counts as 0."""
    m = np.asarray(m)
    return np.where(np.isnan(m), 0.0, np.clip(m, 0.0, 1.0)).astype(m.dtype)


def pooled_mask(mask, f, dtype=np.float64):
    """mp: the f x f block of clamp(m) added in row-major order starting from +0, times 1 / f^2, every operation in `dtype`
    (float32: the kernel's bits; float64: the reference)."""
    B, H, W = mask.shape
    h, w = H // f, W // f
    assert f in FACTORS and (H, W) == (h * f, w * f)
    c = clamp01(np.asarray(mask, F32)).astype(dtype).reshape(B, h, f, w, f)
    s = np.zeros((B, h, w), dtype)
    for r in range(f):
        for q in range(f):
            s = (s + c[:, :, r, :, q]).astype(dtype)
    return (s * dtype(1.0 / (f * f))).astype(dtype)


def effective_mask(mp, floor):
    """e = fmaxf(mp, floor): no rounding."""
    return np.maximum(mp, mp.dtype.type(floor))


def partition(B, hw):
    """Workgroups per sample of both kernels (elementwise.hip masked_blocks): one per 256 positions, at most 128, and few enough that
    B * nb partials and B terms fit 16384 floats."""
    return max(1, min(-(-hw // 256), 128, (16384 - B) // B))


def ordered_sum32(terms, nb):
    """The float32 sum of one sample in the kernels' order.  terms: (positions, inner) float32, inner = 1 (the mask) or C (the loss), added
    per thread position by position (inner in order), then the block tree (xor-shuffle butterfly over 64 lanes, the 4 wave totals in order),
    then the nb workgroup partials in the last arriver's order (thread t takes partials t, t + 256, ...; block tree again)."""
    def block_tree(v):  # v: (256,) float32
        v = v.reshape(4, 64).copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[:, np.arange(64) ^ o]).astype(F32)
        r = F32(0)
        for k in range(4):
            r = F32(r + v[k, 0])
        return r
    hw = terms.shape[0]
    parts = np.zeros(nb, F32)
    for j in range(nb):
        acc = np.zeros(256, F32)
        for p0 in range(j * 256, hw, nb * 256):
            blk = terms[p0: p0 + 256]
            for c in range(blk.shape[1]):
                acc[: blk.shape[0]] = (acc[: blk.shape[0]] + blk[:, c]).astype(F32)
        parts[j] = block_tree(acc)
    acc = np.zeros(256, F32)
    for j0 in range(0, nb, 256):
        blk = parts[j0: j0 + 256]
        acc[: blk.shape[0]] = (acc[: blk.shape[0]] + blk).astype(F32)
    return block_tree(acc)


def sample_factors(B, hw, sums, snr_weight=None, loss_weight=None, normalize=False, dtype=np.float64):
    """k_b = fl(fl(snr * lw) * s_b), s_b = 1 or fl(fl(hw) / S_b), 0 where S_b == 0."""
    one = np.ones(B, dtype)
    k = ((one if snr_weight is None else np.asarray(snr_weight, dtype)) * (one if loss_weight is None else np.asarray(loss_weight, dtype))).astype(dtype)
    if normalize:
        S = np.asarray(sums, dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(S == 0, dtype(0), dtype(hw) / np.where(S == 0, dtype(1), S)).astype(dtype)
        k = (k * s).astype(dtype)
    return k


def reference(pred, target, e=None, snr_weight=None, loss_weight=None, normalize=False):
    """float64: dict(loss, loss_per_sample (B,), grad (B,h,w,C) = d loss / d pred, k (B,), sums (B,))."""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    B, h, w, C = pred.shape
    e64 = np.ones((B, h, w)) if e is None else np.asarray(e, np.float64)
    sums = e64.reshape(B, -1).sum(1)
    k = sample_factors(B, h * w, sums, snr_weight, loss_weight, normalize)
    diff = target.transpose(0, 2, 3, 1) - pred  # (B,h,w,C)
    a = (e64[..., None] * diff ** 2).reshape(B, -1).sum(1)
    count = B * C * h * w
    return dict(loss=float((k * a).sum() / count), loss_per_sample=k * a / (C * h * w),
                grad=-2.0 * (k[:, None, None] * e64)[..., None] * diff / count, k=k, sums=sums)


def dpred_chain32(pred, target, e=None, k=None):
    """The kernel's gradient chain in float32, then RNE to bf16 (torch's cast):
    bf16(fl(fl(fl(-2 * fl(k_b * e)) * diff) * inv_count)), inv_count = fl(1 / fl(B*C*h*w)).  Returns a bf16 torch tensor (B,h,w,C)."""
    pred, target = np.asarray(pred, F32), np.asarray(target, F32)
    B, h, w, C = pred.shape
    e32 = np.ones((B, h, w), F32) if e is None else np.asarray(e, F32)
    k32 = np.ones(B, F32) if k is None else np.asarray(k, F32)
    inv = F32(1.0) / F32(B * C * h * w)
    diff = (target.transpose(0, 2, 3, 1) - pred).astype(F32)
    g = (F32(-2.0) * (k32[:, None, None] * e32).astype(F32)).astype(F32)
    d = ((g[..., None] * diff).astype(F32) * inv).astype(F32)
    return torch.from_numpy(d).to(torch.bfloat16)


def plain_dpred_chain32(pred, target, weight=None):
    """sdt_mse_loss_fwd_bwd's documented chain (tests/test_gpu_reduce_optim_exact.py test_mse_loss_and_gradient_exact):
    bf16(fl(fl(fl(-2 * w) * diff) * inv_count))."""
    pred, target = np.asarray(pred, F32), np.asarray(target, F32)
    B, h, w, C = pred.shape
    wt = np.ones(B, F32) if weight is None else np.asarray(weight, F32)
    inv = F32(1.0) / F32(B * C * h * w)
    diff = (target.transpose(0, 2, 3, 1) - pred).astype(F32)
    d = ((F32(-2.0) * wt[:, None, None, None] * diff).astype(F32) * inv).astype(F32)
    return torch.from_numpy(d).to(torch.bfloat16)


# ---- the exact-answer inputs of tests/test_gpu_masked_loss_kernels.py (proved exact on the CPU by tests/test_masked_loss_cpu.py)
MASK_VALUES = (0.0, 0.25, 0.5, 1.0)
WEIGHTS = (0.5, 1.0, 2.0)
# sdt_loss_mask_prepare: (id, f, B, H, W)
PREPARE_CASES = [("f1", 1, 2, 8, 8), ("f8", 8, 2, 64, 64), ("f8_nonsquare", 8, 3, 56, 88), ("f2", 2, 5, 14, 22), ("f16", 16, 1, 64, 32),
                 ("f4", 4, 2, 24, 40), ("f2_over_cap", 2, 2, 512, 1024)]  # the last: 131072 positions, 128 workgroups, 4 passes
FLOORS = (0.0, 0.25, 1.0)
# sdt_masked_mse_loss_fwd_bwd: (id, B, C, h, w, cpad)
LOSS_CASES = [("one_wg", 2, 4, 8, 8, 8), ("one_wg_unaligned", 2, 4, 8, 8, 4), ("odd", 5, 3, 7, 11, 3), ("c9", 3, 9, 5, 7, 16),
              ("over_cap", 4, 4, 256, 256, 16), ("at_cap_b8", 8, 4, 128, 256, 8)]


def seeded_mask(shape, seed, special=False):
    """Values of MASK_VALUES; special: also a negative value, a value above 1 and a NaN (which count as 0, 1 and 0)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.tensor(MASK_VALUES)[torch.randint(0, len(MASK_VALUES), tuple(shape), generator=g)]
    if special:
        flat = m.reshape(-1)
        flat[1], flat[flat.numel() // 2], flat[-2] = -3.0, 7.5, float("nan")
    return m.contiguous()


def normalising_mask(B, h, w, zero_sample=None, fractional=True):
    """An effective mask (B,h,w) whose h*w / S_b is a power of two: sample b holds one value at every 2^(b % 3)-th position (where that
    step divides h*w; everywhere otherwise) and zero elsewhere.  The value is (1, 0.5, 0.25)[(b + 1) % 3] (fractional: all of
    MASK_VALUES occur from B = 3 on) or 1.  zero_sample: that sample is masked out entirely (S_b = 0)."""
    hw = h * w
    e = torch.ones(B, hw)
    for b in range(B):
        step = 1 << (b % 3)
        if hw % step == 0:
            e[b] = (torch.arange(hw) % step == 0).float()
        if fractional:
            e[b] *= (1.0, 0.5, 0.25)[(b + 1) % 3]
    if zero_sample is not None:
        e[zero_sample] = 0.0
    return e.view(B, h, w).contiguous()


# (id, mask, snr_weight, loss_weight, normalize, zero-sum sample, dpred): which optional operands a loss call gets.  mask "ones": an
# all-ones mask, the call whose dpred must equal sdt_mse_loss_fwd_bwd's bit for bit (as must the calls without a mask or loss weight).
LOSS_VARIANTS = [
    ("bare", None, False, False, False, False, True),
    ("ones_snr_unit_lw", "ones", True, "unit", False, False, True),
    ("mask", "mask", False, False, False, False, True),
    ("mask_norm_zero_both_weights", "mask", True, True, True, True, True),
    ("mask_norm_snr_nodpred", "mask", True, False, True, False, False),
    ("lw_only", None, False, True, False, False, True),
    ("mask_lw_zero_nodpred", "mask", False, True, False, True, False),
    ("mask_norm", "mask", False, False, True, False, True),
]
LOSS_ACCUM_BEFORE = 3.0


def loss_inputs(case, variant):
    """The operands of one (LOSS_CASES entry, LOSS_VARIANTS entry): dict(pred (B,h,w,C) f32 integers in -1..1, target (B,C,h,w), e, snr,
    lw (None where absent), normalize, dpred).  snr * lw is a power of two >= 0.5; masks of the cases with more than 2^16 terms per
    sample hold only 0 and 1, so that every sum keeps a granule of 1/2 (tests/test_masked_loss_cpu.py proves the bound)."""
    name, B, C, h, w, cpad = case
    vname, mask, snr, lw, normalize, zero, dpred = variant
    seed = 900 + 7 * [c[0] for c in LOSS_CASES].index(name)
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(-1, 2, (B, h, w, C), generator=g).float().numpy()
    target = torch.randint(-1, 2, (B, C, h, w), generator=g).float().numpy()
    e = None
    if mask == "ones":
        e = np.ones((B, h, w), F32)
    elif mask == "mask":
        e = normalising_mask(B, h, w, zero_sample=B - 1 if zero else None, fractional=C * h * w <= 1 << 16).numpy()
    snr_v = np.array((0.5, 1.0, 2.0) * 3, F32)[:B] if snr else None
    lw_v = None
    if lw == "unit":
        lw_v = np.ones(B, F32)
    elif lw:
        lw_v = np.array((1.0, 2.0, 0.5) * 3, F32)[:B]
    return dict(pred=pred, target=target, e=e, snr=snr_v, lw=lw_v, normalize=normalize, dpred=dpred)
