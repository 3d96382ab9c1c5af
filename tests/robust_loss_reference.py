"""Reference of the Huber / smooth-L1 loss (include/sdt.h "ROBUST LOSS"): the float64 reference (plain formulas), the exact restatement
of the kernel's chain (double element operations, fp32 roundings, the ordered sums of tests/masked_loss_reference.py) and the case
tables of tests/test_gpu_robust_loss_kernels.py.  Layouts as there: pred (B,h,w,C) (the real channels of the NHWC prediction), target
(B,C,h,w), e (B,h,w), c (B,) the samples' thresholds."""
import numpy as np
import torch

from tests import masked_loss_reference as mr

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of fp32
HUBER, SMOOTH_L1 = 1, 2  # sdt_robust_loss_fwd_bwd's loss_type
TYPES = {"huber": HUBER, "smooth_l1": SMOOTH_L1}


def gamma(n):
    """n roundings: (1 + u)^n - 1 <= n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


# ================================================================================================ float64, plain formulas
def rho_plain64(diff, c, loss_type):
    """The definition: 2c(r - c) (huber) or 2(r - c) (smooth_l1), r = sqrt(diff^2 + c^2).  r - c cancels for |diff| << c."""
    diff, c = np.asarray(diff, F64), np.asarray(c, F64)
    r = np.sqrt(diff * diff + c * c)
    return (2.0 * c if loss_type == HUBER else 2.0) * (r - c)


def rho64(diff, c, loss_type):
    """The same function without the cancellation: 2c diff^2 / (r + c) or 2 diff^2 / (r + c); 0 where r == 0."""
    diff, c = np.asarray(diff, F64), np.asarray(c, F64)
    r = np.sqrt(diff * diff + c * c)
    den = np.where(r == 0, 1.0, r + c)
    return np.where(r == 0, 0.0, (2.0 * c if loss_type == HUBER else 2.0) * diff * diff / den)


def drho64(diff, c, loss_type):
    """d rho / d pred = -2c diff / r or -2 diff / r (diff = target - pred); 0 where r == 0."""
    diff, c = np.asarray(diff, F64), np.asarray(c, F64)
    r = np.sqrt(diff * diff + c * c)
    return np.where(r == 0, 0.0, (-2.0 * c if loss_type == HUBER else -2.0) * diff / np.where(r == 0, 1.0, r))


def reference(pred, target, c, loss_type, e=None, snr_weight=None, loss_weight=None, normalize=False):
    """float64: dict(loss, loss_per_sample (B,), grad (B,h,w,C) = d loss / d pred, k (B,), sums (B,)) of
    loss = (1/count) sum_b k_b sum_{c,p} e rho, with masked_loss_reference's k_b."""
    pred, target = np.asarray(pred, F64), np.asarray(target, F64)
    B, h, w, C = pred.shape
    e64 = np.ones((B, h, w)) if e is None else np.asarray(e, F64)
    sums = e64.reshape(B, -1).sum(1)
    k = mr.sample_factors(B, h * w, sums, snr_weight, loss_weight, normalize)
    diff = target.transpose(0, 2, 3, 1) - pred
    cb = np.asarray(c, F64)[:, None, None, None]
    a = (e64[..., None] * rho64(diff, cb, loss_type)).reshape(B, -1).sum(1)
    count = B * C * h * w
    return dict(loss=float((k * a).sum() / count), loss_per_sample=k * a / (C * h * w),
                grad=(k[:, None, None] * e64)[..., None] * drho64(diff, cb, loss_type) / count, k=k, sums=sums)


# ================================================================================================ the kernel's chain, restated
def element_chain(diff32, c32, loss_type):
    """(g, rho) float32 of fp32 diff and c, the kernel's operations one by one.  Every numpy float64 operation below is one IEEE double
    operation (the products marked exact have at most 48 significant bits); .astype(float32) is the single round-to-nearest-even."""
    D, Cd = np.asarray(diff32, F32).astype(F64), np.asarray(c32, F32).astype(F64)
    D, Cd = np.broadcast_arrays(D, Cd)
    dd = D * D                  # exact
    r = np.sqrt(dd + Cd * Cd)   # c*c exact; fl64 of the sum, fl64 of the root
    zero = r == 0
    rs = np.where(zero, 1.0, r)
    den = np.where(zero, 1.0, r + Cd)
    if loss_type == HUBER:
        g = ((-2.0 * Cd) * D) / rs      # (-2c)*diff exact
        rho = ((2.0 * Cd) * dd) / den   # fl64 of the product, fl64 of the quotient
    else:
        g = (-2.0 * D) / rs
        rho = (2.0 * dd) / den          # 2*dd exact
    return np.where(zero, 0.0, g).astype(F32), np.where(zero, 0.0, rho).astype(F32)


def chain(pred, target, c, loss_type, e=None, k=None):
    """dpred as a bf16 torch tensor (B,h,w,C) = bf16(fl(fl(fl(k_b*e) * g) * inv_count)), and the summands fl(e * rho) float32 (B, h*w, C)."""
    pred, target = np.asarray(pred, F32), np.asarray(target, F32)
    B, h, w, C = pred.shape
    e32 = np.ones((B, h, w), F32) if e is None else np.asarray(e, F32)
    k32 = np.ones(B, F32) if k is None else np.asarray(k, F32)
    inv = F32(1.0) / F32(B * C * h * w)
    diff = (target.transpose(0, 2, 3, 1) - pred).astype(F32)
    g, rho = element_chain(diff, np.asarray(c, F32)[:, None, None, None], loss_type)
    ke = (k32[:, None, None] * e32).astype(F32)
    d = ((ke[..., None] * g).astype(F32) * inv).astype(F32)
    terms = (e32[..., None] * rho).astype(F32)
    return torch.from_numpy(d).to(torch.bfloat16), terms.reshape(B, h * w, C)


def ordered_loss(terms, k32, C, loss_before=0.0):
    """(loss_accum, loss_per_sample (B,)) float32 in the kernel's order: a_b by masked_loss_reference.ordered_sum32 over the partition,
    term_b = fl(k_b a_b), loss_per_sample = fl(term_b * fl(1/(C h w))), loss_accum = fl(before + fl(T * inv_count)), T = the terms added
    in sample order from +0."""
    B, hw, _ = terms.shape
    nb = mr.partition(B, hw)
    inv_count, inv_chw = F32(1.0) / F32(B * C * hw), F32(1.0) / F32(C * hw)
    lps, T = np.zeros(B, F32), F32(0)
    for b in range(B):
        term = F32(F32(k32[b]) * mr.ordered_sum32(terms[b], nb))
        lps[b] = F32(term * inv_chw)
        T = F32(T + term)
    return F32(F32(loss_before) + F32(T * inv_count)), lps


def kernel_sums32(e32):
    """S_b as sdt_loss_mask_prepare leaves it: the fp32 sum of the effective mask in the kernels' order."""
    B = e32.shape[0]
    hw = e32[0].size
    return np.array([mr.ordered_sum32(np.asarray(e32[b], F32).reshape(hw, 1), mr.partition(B, hw)) for b in range(B)], F32)


# ================================================================================================ case tables
# sdt_robust_loss_fwd_bwd: (id, B, C, h, w, cpad, pred shifted by one bf16 element: a base that is not 16-byte aligned)
CASES = [
    ("vec", 2, 4, 8, 8, 8, False),               # 16-byte vectors; pred's padding lanes hold NaN
    ("scalar_cpad4", 2, 3, 8, 8, 4, False),      # cpad % 8 != 0: element by element
    ("misaligned", 2, 4, 8, 8, 8, True),         # a vector shape from a misaligned pred: element by element
    ("over_cap", 1, 1, 192, 192, 8, False),      # 36,864 positions > 128 workgroups x 256: the stride loop, 128 partials
    ("b3_zero", 3, 4, 8, 8, 8, False),           # sample 1: c = 0 and diff = 0 everywhere (r = 0); sample 2: S_b = 0 under normalisation
]
# (id, mask, sums (normalisation), snr weight, loss weight, dpred)
VARIANTS = [
    ("bare", False, False, False, False, True),
    ("mask_null_sums", True, False, False, False, True),
    ("mask_norm_snr", True, True, True, False, True),
    ("lw_only_nodpred", False, False, False, True, False),
    ("mask_norm_both_weights", True, True, True, True, True),
]
LOSS_ACCUM_BEFORE = 0.5
POISON = (0xFF, 0x5A, 0x7F)  # the scratch behind the arrival counters before each of the three runs


def random_inputs(case, variant):
    """Random operands of one (CASES entry, VARIANTS entry): dict(pred (B,h,w,C) f32 holding bf16 values, target (B,C,h,w), c (B,), e, sums,
    snr, lw (None where absent), normalize, dpred).  The b3_zero case: sample 1 has c = 0 and target == pred, sample 2's mask is zero."""
    name, B, C, h, w, cpad, _ = case
    vname, mask, norm, snr, lw, dpred = variant
    g = torch.Generator().manual_seed(500 + [c[0] for c in CASES].index(name))
    pred = torch.randn(B, h, w, C, generator=g).bfloat16().float()
    target = torch.randn(B, C, h, w, generator=g)
    c = torch.rand(B, generator=g) * 0.95 + 0.05
    e = torch.rand(B, h, w, generator=g)
    e[torch.rand(B, h, w, generator=g) < 0.25] = 0.0
    snr_v = torch.rand(B, generator=g) + 0.2
    lw_v = torch.rand(B, generator=g) * 2 + 0.1
    if name == "b3_zero":
        c[1] = 0.0
        target[1] = pred[1].permute(2, 0, 1)
        e[2] = 0.0
    e = e.numpy() if mask else None
    sums = kernel_sums32(e) if norm else None
    return dict(pred=pred.numpy(), target=target.numpy(), c=c.numpy(), e=e, sums=sums, snr=snr_v.numpy() if snr else None,
                lw=lw_v.numpy() if lw else None, normalize=norm, dpred=dpred)


# ---- exact-answer inputs: diff in {0, +-3 * 2^j}, c = 4 * 2^j, so r = 5 * 2^j and rho = 8 * 4^j (huber) or 2 * 2^j (smooth_l1) exactly
EXACT_J = (-1, 0, 1)
EXACT_SHAPES = [(2, 4, 8, 8), (3, 3, 7, 11), (1, 1, 192, 192)]


def exact_inputs(B, C, h, w, seed=0, masked=True):
    """Sample b uses j = EXACT_J[b % 3]: pred in {-1, 0, 1} * 2^j, target = pred + s * 3 * 2^j with s in {-1, 0, 1}, c_b = 4 * 2^j, a mask of
    masked_loss_reference.MASK_VALUES, weights in {0.5, 1, 2}."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([2.0 ** EXACT_J[b % 3] for b in range(B)])
    p = torch.randint(-1, 2, (B, h, w, C), generator=g).float()
    s = torch.randint(-1, 2, (B, h, w, C), generator=g).float()
    pred = p * scale[:, None, None, None]
    target = ((p + 3.0 * s) * scale[:, None, None, None]).permute(0, 3, 1, 2).contiguous()
    e = mr.seeded_mask((B, h, w), seed + 1).numpy() if masked else None
    return dict(pred=pred.numpy(), target=target.numpy(), c=(4.0 * scale).numpy(), e=e, s=s.numpy(), scale=scale.numpy(),
                snr=np.array((0.5, 1.0, 2.0), F32)[:B], lw=np.array((2.0, 2.0, 0.5), F32)[:B])
