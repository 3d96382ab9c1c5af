"""NumPy float32 restatement of the AdamW optimizer (include/sdt.h "AdamW"; DESIGN.md "AdamW with 8-bit moments"): the reference the
AdamW tests hold the kernels and the host code to, bit for bit.

Every element operation is a float32 one rounded on its own (.astype(F32) after each); division and square root are NumPy's correctly
rounded ones.  The per-step scalars come from running float64 products (select_scalars).  The clip is oracle.lion8's
(optax.clip_by_global_norm), the codec's thresholds are lion_codec.quantization_thresholds() - a function of the magnitude alone - used
WITHOUT the reference's offset."""
import numpy as np

from oracle import lion8
from stable_diffusion_training_amd import lion_codec

F32 = np.float32
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, ema_rate=0.999)


# ------------------------------------------------------------------------------------------------ per-step scalars
def products(n, b1, b2):
    """(P1, P2) after n steps: n sequential float64 products from 1.0 (python floats are IEEE doubles, gradual underflow included)."""
    p1 = p2 = 1.0
    for _ in range(int(n)):
        p1 *= b1
        p2 *= b2
        if p1 == 0.0 and p2 == 0.0:
            break
    return p1, p2


def select_scalars(t, prods, b1, b2, *, lr=None, ema_rate=0.0, lr_tab=None, ema_tab=None):
    """One sdt_adamw_select launch: t the counter before it, prods = (P1, P2) before it.  Returns (cur float32[8], t + 1, (P1', P2')).
    lr_tab (float32 -lr_t) / ema_tab (float32 [n][2]) as lr_schedule builds them, entry min(t, n - 1); without tables the by-value
    roundings of the launcher."""
    p1, p2 = prods[0] * b1, prods[1] * b2
    if lr_tab is not None:
        tc = max(int(t), 0)
        neg_lr = F32(lr_tab[min(tc, len(lr_tab) - 1)])
        e = np.asarray(ema_tab, F32).reshape(-1, 2)[min(tc, len(ema_tab) - 1)]
        r, rm = F32(e[0]), F32(e[1])
    else:
        neg_lr, r, rm = F32(-lr), F32(ema_rate), F32(1.0 - ema_rate)
    k1 = F32(1.0 / (1.0 - p1))
    k2 = F32(1.0 / float(np.sqrt(np.float64(1.0 - p2))))
    return np.array([neg_lr, r, rm, 0, k1, k2, 0, 0], F32), int(t) + 1, (p1, p2)


# ------------------------------------------------------------------------------------------------ codec (no offset)
def quantize(x):
    """int8 codes of x in [-1, 1]: sign(x) * c(|x|), c by the threshold table (what the kernel settles its estimate against)."""
    x = np.asarray(x, F32)
    t = lion_codec.quantization_thresholds()
    mag = np.searchsorted(t[1:], np.abs(x), side="right").astype(np.int32)
    return (np.where(x < 0, -mag, mag)).astype(np.int8)


def quantize_direct(x):
    """The definition the table restates: rint(|x|^(1/5) * 127) in float32, signed."""
    x = np.asarray(x, F32)
    q = np.power(np.abs(x), F32(1 / 5)).astype(F32)
    mag = np.rint((q * F32(127)).astype(F32)).astype(np.int32)
    return (np.where(x < 0, -mag, mag)).astype(np.int8)


def dequantize(c):
    t = (np.asarray(c).astype(F32) / F32(127)).astype(F32)
    t2 = (t * t).astype(F32)
    t4 = (t2 * t2).astype(F32)
    return (t4 * t).astype(F32)


def block_quantize(x, bs):
    flat = np.asarray(x, F32).reshape(-1, bs)
    absmax = np.max(np.abs(flat), axis=-1, keepdims=True).astype(F32)
    inv = (F32(1) / np.where(absmax <= F32(0), F32(1), absmax)).astype(F32)
    return quantize((flat * inv).astype(F32)), inv


def block_dequantize(codes, inv):
    return (dequantize(codes) / inv).astype(F32).reshape(-1)


def init_state8(n, bs):
    """(m codes, m inverse scales, s codes, s inverse scales): codes 0, scales 1."""
    nb = n // bs
    return (np.zeros((nb, bs), np.int8), np.ones((nb, 1), F32), np.zeros((nb, bs), np.int8), np.ones((nb, 1), F32))


# ------------------------------------------------------------------------------------------------ the step
def clip(g, max_norm, sq=None):
    """gc of the sweeps: g when max_norm is None, else optax's clip with norm = float32(sqrt(sum of squares in double)).  sq: the
    squared norm of a larger buffer g is a piece of."""
    g = np.asarray(g, F32)
    if max_norm is None:
        return g
    if sq is None:
        return lion8.clip_by_global_norm({"x": g}, max_norm)[0]["x"]
    n = F32(np.sqrt(np.float64(sq)))
    return g if n < F32(max_norm) else ((g / n).astype(F32) * F32(max_norm)).astype(F32)


def _update(p, gc, m, v, cur, wd, b1, b2, eps):
    c1, c1m, c2, c2m = F32(b1), F32(1.0 - b1), F32(b2), F32(1.0 - b2)
    neg_lr, k1, k2 = cur[0], cur[4], cur[5]
    mn = ((c1 * m).astype(F32) + (c1m * gc).astype(F32)).astype(F32)
    vn = ((c2 * v).astype(F32) + (c2m * (gc * gc).astype(F32)).astype(F32)).astype(F32)
    sn = np.sqrt(vn).astype(F32)
    u = ((mn * k1).astype(F32) / ((sn * k2).astype(F32) + F32(eps)).astype(F32)).astype(F32)
    if wd != 0:
        u = (u + (F32(wd) * p).astype(F32)).astype(F32)
    pn = (p + (neg_lr * u).astype(F32)).astype(F32)
    return pn, mn, vn, sn


def ema_update(ema, p, cur):
    return ((cur[1] * np.asarray(ema, F32)).astype(F32) + (cur[2] * p).astype(F32)).astype(F32)


def step32(p, g, m, v, cur, *, wd, b1, b2, eps, max_norm=None, sq=None):
    """fp32-state step on flat arrays: (p', m', v')."""
    pn, mn, vn, _ = _update(np.asarray(p, F32), clip(g, max_norm, sq), np.asarray(m, F32), np.asarray(v, F32), cur, wd, b1, b2, eps)
    return pn, mn, vn


def step8(p, g, state, cur, *, bs, wd, b1, b2, eps, max_norm=None, sq=None):
    """8-bit step: state = (m codes, m inv, s codes, s inv) -> (p', new state)."""
    mc, mi, sc, si = state
    m = block_dequantize(mc, mi)
    s = block_dequantize(sc, si)
    v = (s * s).astype(F32)
    pn, mn, _, sn = _update(np.asarray(p, F32), clip(g, max_norm, sq), m, v, cur, wd, b1, b2, eps)
    return pn, block_quantize(mn, bs) + block_quantize(sn, bs)
