"""NumPy float32 restatement of the Prodigy optimizer (include/sdt.h "Prodigy"; DESIGN.md "Prodigy"): the reference the Prodigy tests hold
the kernels and the host code to, bit for bit - and, beside it, a plain float64 textbook version of the same algorithm (textbook64).

Restatement: every element operation is a float32 one rounded on its own (.astype(F32) after each); division and square root are NumPy's
correctly rounded ones.  The per-step scalars are formed from Python floats (IEEE doubles) and rounded once.  The two global sums are
taken in double in the kernels' order (ordered_sum: sqnorm_kernel's partition, kernel_checks.sqnorm_partition).  The clip and the EMA are
adamw_reference's."""
import math

import numpy as np

from tests import kernel_checks as kc
from tests.adamw_reference import clip, ema_update  # noqa: F401  (ema_update reads cur[1], cur[2]: the same slots here)

F32 = np.float32
DEFAULTS = dict(lr=1.0, b1=0.9, b2=0.999, beta3=None, eps=1e-8, weight_decay=0.0, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                use_bias_correction=False, safeguard_warmup=False)


def hyper(**kw):
    hp = dict(DEFAULTS, **kw)
    if hp["beta3"] is None:
        hp["beta3"] = math.sqrt(hp["b2"])
    return hp


# ------------------------------------------------------------------------------------------------ the float64 textbook version
def textbook64(grad, x0, steps, **kw):
    """Adam-style Prodigy with decoupled decay in plain float64, as the issue states it.  grad: x -> gradient.  Returns (x, [d after every
    step])."""
    hp = hyper(**kw)
    lr, b1, b2, b3, d0 = hp["lr"], hp["b1"], hp["b2"], hp["beta3"], hp["d0"]
    x, p0 = np.array(x0, np.float64), np.array(x0, np.float64)
    m, v, s = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    d = d_max = d0
    numer, ds = 0.0, []
    for k in range(1, steps + 1):
        g = grad(x)
        bc = math.sqrt(1 - b2 ** k) / (1 - b1 ** k) if hp["use_bias_correction"] else 1.0
        dlr = d * lr * bc
        q = d / d0 * dlr
        m = b1 * m + d * (1 - b1) * g
        v = b2 * v + d * d * (1 - b2) * g * g
        s = b3 * s + (d / d0 * d if hp["safeguard_warmup"] else q) * g
        numer = b3 * numer + q * float(np.dot(g, p0 - x))
        l1 = float(np.abs(s).sum())
        if l1 != 0 and lr > 0:
            d_hat = hp["d_coef"] * numer / l1
            if d == d0:
                d = max(d, d_hat)
            d_max = max(d_max, d_hat)
            d = min(d_max, d * hp["growth_rate"])
        if hp["weight_decay"]:
            x = x - dlr * hp["weight_decay"] * x
        x = x - dlr * m / (np.sqrt(v) + d * hp["eps"])
        ds.append(d)
    return x, ds


# ------------------------------------------------------------------------------------------------ one-lane kernels
def products(n, b1, b2):
    from tests.adamw_reference import products as pr
    return pr(n, b1, b2)


def init_state(hp, t=0):
    """The device state before step t of a fresh run (d, d_max, numer as at the start; products and counter as set_step(t) leaves them)."""
    p1, p2 = products(t, hp["b1"], hp["b2"])
    return dict(d=hp["d0"], d_max=hp["d0"], numer=0.0, P1=p1, P2=p2, dot=0.0, l1=0.0, q=0.0, lr_t=0.0, t=int(t))


def state_block(st):
    """The ten doubles of the device block."""
    return np.array([st["d"], st["d_max"], st["numer"], st["P1"], st["P2"], st["dot"], st["l1"], st["q"], st["lr_t"], 0.0], np.float64)


def select(st, hp, *, ema_rate=0.0, lr_tab=None, ema_tab=None):
    """One sdt_prodigy_select launch on the state dict (in place).  Returns cur float32[8] = {neg_dlr, r, 1 - r, first, c_m, c_v, c_s, 0}."""
    t = st["t"]
    if lr_tab is not None:
        tc = max(t, 0)
        lr_t = -float(F32(lr_tab[min(tc, len(lr_tab) - 1)]))
        e = np.asarray(ema_tab, F32).reshape(-1, 2)
        e = e[min(tc, len(e) - 1)]
        r, rm = F32(e[0]), F32(e[1])
    else:
        lr_t, r, rm = float(hp["lr"]), F32(ema_rate), F32(1.0 - ema_rate)
    st["P1"] *= hp["b1"]
    st["P2"] *= hp["b2"]
    bc = math.sqrt(1.0 - st["P2"]) / (1.0 - st["P1"]) if hp["use_bias_correction"] else 1.0
    d, d0 = st["d"], hp["d0"]
    dlr = (d * lr_t) * bc
    q = (d / d0) * dlr
    c_s = (d / d0) * d if hp["safeguard_warmup"] else q
    cur = np.array([F32(-dlr), r, rm, F32(1.0 if t == 0 else 0.0), F32(d * (1.0 - hp["b1"])), F32((d * d) * (1.0 - hp["b2"])), F32(c_s), 0],
                   F32)
    st.update(dot=0.0, l1=0.0, q=q, lr_t=lr_t, t=t + 1)
    return cur


def finish(st, hp, cur):
    """One sdt_prodigy_finish launch: the state dict and cur[7] (d_eps) in place."""
    numer = hp["beta3"] * st["numer"] + st["q"] * st["dot"]
    st["numer"] = numer
    d = st["d"]
    if st["l1"] != 0.0 and st["lr_t"] > 0.0:
        d_hat = (hp["d_coef"] * numer) / st["l1"]
        if d == hp["d0"]:
            d = d_hat if d_hat > d else d
        d_max = d_hat if d_hat > st["d_max"] else st["d_max"]
        with np.errstate(over="ignore"):
            grown = float(np.float64(d) * np.float64(hp["growth_rate"]))
        d = grown if grown < d_max else d_max
        st["d_max"], st["d"] = d_max, d
    cur[7] = F32(d * hp["eps"])
    return cur


# ------------------------------------------------------------------------------------------------ the two sums
def _wave_tree(x):
    """__shfl_xor butterfly over the last axis (64 lanes): what lane 0 holds."""
    o = x.shape[-1] // 2
    while o:
        x = x[..., :o] + x[..., o: 2 * o]
        o //= 2
    return x[..., 0]


def ordered_sum(terms, out=0.0):
    """out + the sum of the n float64 terms in the order of ordered_sums_f64 behind sqnorm_kernel's walk (optimizer.hip): each thread adds
    the x and z terms of its float4s into one accumulator and y and w into a second, adds the two, thread i < n & 3 of workgroup 0 adds tail
    term i; a butterfly per wave, the four waves of a workgroup in sequence; the last workgroup adds the partials 256 apart per thread, a
    butterfly per wave again and (w0 + w1) + (w2 + w3)."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    n = terms.size
    grid, nv = kc.sqnorm_partition(n)
    T = grid * 256
    iters = max(-(-nv // T), 1)
    x = np.zeros(iters * T * 4, np.float64)
    x[: nv * 4] = terms[: nv * 4]
    x = x.reshape(iters, T, 4)
    d0, d1 = np.zeros(T), np.zeros(T)
    for it in range(iters):
        d0 = d0 + x[it, :, 0]
        d1 = d1 + x[it, :, 1]
        d0 = d0 + x[it, :, 2]
        d1 = d1 + x[it, :, 3]
    acc = d0 + d1
    tail = terms[nv * 4:]
    acc[: tail.size] = acc[: tail.size] + tail
    waves = _wave_tree(acc.reshape(grid, 4, 64))
    part = np.zeros(grid)
    for w in range(4):
        part = part + waves[:, w]
    rows = -(-grid // 256)
    pp = np.zeros(rows * 256)
    pp[:grid] = part
    t = np.zeros(256)
    for r in range(rows):
        t = t + pp[r * 256: (r + 1) * 256]
    w = _wave_tree(t.reshape(4, 64))
    return float(out + ((w[0] + w[1]) + (w[2] + w[3])))


# ------------------------------------------------------------------------------------------------ the sweeps
def moments(p, g, p0, m, v, s, cur, hp, st, *, max_norm=None, sq=None):
    """One sdt_prodigy_moments_step launch over flat arrays: returns (p0', m', v', s') and adds the launch's two sums to st."""
    p, m, v, s = (np.asarray(a, F32) for a in (p, m, v, s))
    gc = clip(g, max_norm, sq)
    c1, c2, c3 = F32(hp["b1"]), F32(hp["b2"]), F32(hp["beta3"])
    c_m, c_v, c_s = cur[4], cur[5], cur[6]
    p0n = p.copy() if cur[3] != 0 else np.asarray(p0, F32)
    mn = ((c1 * m).astype(F32) + (c_m * gc).astype(F32)).astype(F32)
    vn = ((c2 * v).astype(F32) + (c_v * (gc * gc).astype(F32)).astype(F32)).astype(F32)
    sn = ((c3 * s).astype(F32) + (c_s * gc).astype(F32)).astype(F32)
    dx = (p0n - p).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        st["dot"] = ordered_sum(gc.astype(np.float64) * dx.astype(np.float64), st["dot"])
        st["l1"] = ordered_sum(np.abs(sn).astype(np.float64), st["l1"])
    return p0n, mn, vn, sn


def apply(p, m, v, cur, wd):
    """One sdt_prodigy_apply_step launch: p' (the EMA: ema_update(ema, p', cur); the mirror: bf16(p'))."""
    p = np.asarray(p, F32)
    neg_dlr, d_eps = cur[0], cur[7]
    if wd != 0:
        p = (p + ((neg_dlr * F32(wd)).astype(F32) * p).astype(F32)).astype(F32)
    den = (np.sqrt(np.asarray(v, F32)).astype(F32) + d_eps).astype(F32)
    return (p + (neg_dlr * (np.asarray(m, F32) / den).astype(F32)).astype(F32)).astype(F32)


def step(p, g, buf, st, hp, *, wd=0.0, ema_rate=0.0, max_norm=None, lr_tab=None, ema_tab=None):
    """A whole one-piece step on flat arrays: buf = dict(p0, m, v, s[, ema]) and st updated in place; returns (p', cur)."""
    cur = select(st, hp, ema_rate=ema_rate, lr_tab=lr_tab, ema_tab=ema_tab)
    buf["p0"], buf["m"], buf["v"], buf["s"] = moments(p, g, buf["p0"], buf["m"], buf["v"], buf["s"], cur, hp, st, max_norm=max_norm)
    finish(st, hp, cur)
    p = apply(p, buf["m"], buf["v"], cur, wd)
    if buf.get("ema") is not None:
        buf["ema"] = ema_update(buf["ema"], p, cur)
    return p, cur


def zeros(n):
    return dict(p0=np.zeros(n, F32), m=np.zeros(n, F32), v=np.zeros(n, F32), s=np.zeros(n, F32))
