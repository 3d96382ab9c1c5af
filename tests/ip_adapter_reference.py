"""References for the IP-Adapter tests (Ye et al. 2023, arXiv:2308.06721).

Network level: a torch restatement of the image projection and of the decoupled cross-attention on the oracle's own primitives
(oracle.nets), and `with_image_tokens`, which runs any oracle network (a transformer block, the whole UNet) with the image term
added to every attn2 - the oracle itself is not edited.

Kernel level: `ip_expect_bits`, the bits sdt_ip_attention_fwd / _bwd must produce on the exact constructions of
tests/kernel_checks.py (selector_case: P one-hot; pair_case: P = 1/2, 1/2), computed in float64 from the IDEAL P and rounded at the
rounding points include/sdt.h "IP-ADAPTER" documents.  Every intermediate in front of a rounding point is asserted exact, so the
expectation does not depend on the order of any sum."""
import contextlib
import math

import torch

from oracle import nets as N

from tests import kernel_checks as kc

BF = torch.bfloat16
LIMIT = float(1 << 24)


# ------------------------------------------------------------------------------------------------ network level
def image_tokens(ip, cfg, image_embeds):
    """image_proj of the published ImageProjModel: Linear E -> T*Dc, reshape (B, T, Dc), LayerNorm over Dc."""
    T, Dc = cfg["num_tokens"], cfg["cross_attention_dim"]
    y = N.dense(image_embeds, ip, "image_proj/proj")
    return N.layer_norm(y.reshape(image_embeds.shape[0], T, Dc), ip, "image_proj/norm")


def decoupled_attn(x, ctx, tokens, p, ip, name, heads, chunked_keys=True, scale_ip=None):
    """IPAttnProcessor: to_out(softmax(q K_txt^T) V_txt + scale_ip * softmax(q K_ip^T) V_ip), one q for both terms; the text term is
    the oracle's (key-chunk weights included), the image tokens count once each."""
    c = x.shape[-1]
    q = N.dense(x, p, name + "/to_q")
    k, v = N.dense(ctx, p, name + "/to_k"), N.dense(ctx, p, name + "/to_v")
    bias = None
    if chunked_keys:
        w = N.key_chunk_weights(x.shape[1], ctx.shape[1])
        if not bool((w == 1).all()):
            bias = torch.log(w)
    scale = (c // heads) ** -0.5
    o = N.attention_core(q, k, v, heads, scale, key_logit_bias=bias)
    ki, vi = N.dense(tokens, ip, name + "/to_k_ip"), N.dense(tokens, ip, name + "/to_v_ip")
    oi = N.attention_core(q, ki, vi, heads, scale)
    if scale_ip is not None:
        oi = oi * scale_ip.reshape(-1, 1, 1).to(oi.dtype)
    return N.dense(N._r(o + oi), p, name + "/to_out_0")


@contextlib.contextmanager
def with_image_tokens(ip, tokens, scale_ip=None):
    """Inside the block every cross-attention (…/attn2) of an oracle forward is the decoupled one."""
    plain = N._attn

    def attn(x, ctx, p, name, heads, chunked_keys=True):
        if name.endswith("/attn2"):
            return decoupled_attn(x, ctx, tokens, p, ip, name, heads, chunked_keys, scale_ip)
        return plain(x, ctx, p, name, heads, chunked_keys)

    N._attn = attn
    try:
        yield
    finally:
        N._attn = plain


# ------------------------------------------------------------------------------------------------ kernel level
def ideal_p(case, B, H, Nq, T):
    """(B, H, Nq, T) float64: one-hot on a selector case's target, 1 / ties on a pair case's target pair."""
    if "pair" in case:
        hit = (case["pair"][:, :, None, :] == case["target"][:, :, :, None]).double()
        return hit / hit.sum(-1, keepdim=True)
    return torch.nn.functional.one_hot(case["target"], T).double()


def bf16_rne_f64(x):
    """float64 -> bf16 with ONE rounding to nearest even: float64 -> float32 rounded to odd, then torch's RNE float32 -> bf16 (24 bits
    are more than 8 + 2, so the second rounding sees everything the first dropped).  Finite values in the float32 normal range."""
    f = x.to(torch.float32)
    d = f.double()
    i = f.view(torch.int32).clone()
    inexact = d != x
    away = inexact & (d.abs() > x.abs())       # RNE went away from zero: step the magnitude back (sign-magnitude bits)
    i = torch.where(away, i - 1, i)
    i = torch.where(inexact, i | 1, i)
    return i.view(torch.float32).to(BF)


def _quantum(t):
    """Largest power of two that divides every element (2^8 for all zeros)."""
    for e in range(8, -60, -1):
        s = t * 2.0 ** -e
        if torch.equal(s, s.round()):
            return 2.0 ** e
    raise AssertionError("ip_expect_bits: an operand is not a dyadic rational above 2^-60")


def _contract(a, b, what):
    """a @ b in float64 with the assertion that makes it the fp32 result in ANY order: every product is a multiple of one quantum and
    the sum of the magnitudes stays below 2^24 quanta."""
    q = _quantum(a) * _quantum(b)
    assert float((a.abs() @ b.abs()).max()) < LIMIT * q, f"ip_expect_bits: {what} is not exact in fp32"
    return a @ b + 0.0


def _fl32(x, what, exact=True):
    y = x.to(torch.float32).double()
    assert not exact or torch.equal(y, x), f"ip_expect_bits: {what} is not exact in fp32"
    return y


def ip_expect_bits(case, B, H, Nq, T, D, scale, o_txt=None, dq_in=None, scale_ip=None):
    """dict(out, dq: bf16 (B, Nq, C); dkv: bf16 (B, T, 2C); p) for q = case['q'], [k | v] = case['k'], case['v'], dout = case['dout'].
    o_txt, dq_in: bf16 (B, Nq, C) or None (= +0); scale_ip: float32 (B,) or None (= 1).  Rounding points (include/sdt.h):
      out = bf16_rne(f64(o_txt) + f64(scale_ip) * f64(acc)), acc = P.V exact in fp32
      g = fl32(scale_ip * dout) (asserted exact), dP = g.V^T, delta = rowsum(P o dP), dS = P o (dP - delta): all exact in fp32
      dq = bf16_rne(f64(dq_in) + f64(fl32(scale_f32 * (dS.K))))
      dK = bf16_rne(fl32(scale_f32 * (dS^T.Q))), dV = bf16_rne(P^T.g)."""
    C = H * D
    q4, k4, v4, do4 = (case[n].view(B, -1, H, D).transpose(1, 2).double() for n in ("q", "k", "v", "dout"))
    p = ideal_p(case, B, H, Nq, T)
    sip = torch.ones(B, dtype=torch.float64) if scale_ip is None else scale_ip.double().cpu()
    sip = sip.view(B, 1, 1, 1)
    flat = lambda t, n: t.transpose(1, 2).reshape(B, n, C)
    zeros = torch.zeros(B, Nq, C, dtype=torch.float64)
    acc = _contract(p, v4, "P.V")
    out = bf16_rne_f64((zeros if o_txt is None else o_txt.double().cpu()) + flat(sip * acc, Nq))
    g = _fl32(sip * do4, "scale_ip * dout")
    dp = _contract(g, v4.transpose(-1, -2), "dP = g.V^T")
    delta = _fl32((p * dp).sum(-1, keepdim=True), "delta")
    assert float((p.abs() * dp.abs()).sum(-1).max()) < LIMIT * _quantum(p) * _quantum(dp), "ip_expect_bits: delta is not exact in fp32"
    ds = _fl32(p * _fl32(dp - delta, "dP - delta"), "dS")
    scale_f = float(torch.tensor(scale, dtype=torch.float32))
    dq_ip = _fl32(_contract(ds, k4, "dS.K") * scale_f, "scale * dS.K", exact=False)
    dq = bf16_rne_f64((zeros if dq_in is None else dq_in.double().cpu()) + flat(dq_ip, Nq))
    dk = _fl32(_contract(ds.transpose(-1, -2), q4, "dS^T.Q") * scale_f, "scale * dS^T.Q", exact=False).to(torch.float32).to(BF)
    dv = _contract(p.transpose(-1, -2), g, "P^T.g").to(torch.float32).to(BF)
    dkv = torch.cat([flat(dk, T), flat(dv, T)], -1)
    return dict(out=out, dq=dq, dkv=dkv, p=p)


def min_lead(case, B, H, Nq, T, D, scale):
    """Smallest lead (natural units) of the target key or pair over every other key; inf when there is no other key."""
    if "pair" in case:
        tie, lead, _ = kc.pair_min_gap(case, B, H, Nq, T, D, scale)
        assert tie == 0.0
        return lead if math.isfinite(lead) else float("inf")
    gap, _ = kc.selector_min_gap(case, B, H, Nq, T, D, scale)
    return gap


def softmax_ref32(q, kv, dout, H, scale):
    """fp32 torch softmax attention over the image tokens alone and its three gradients: (out, dq, dkv)."""
    B, Nq, C = q.shape
    D = C // H
    qr, kvr = q.float().requires_grad_(True), kv.float().requires_grad_(True)
    qh = qr.view(B, Nq, H, D).transpose(1, 2)
    kh, vh = (kvr[..., s].reshape(B, -1, H, D).transpose(1, 2) for s in (slice(0, C), slice(C, 2 * C)))
    o = (torch.softmax((qh @ kh.transpose(-1, -2)) * scale, -1) @ vh).transpose(1, 2).reshape(B, Nq, C)
    o.backward(dout.float())
    return o.detach(), qr.grad, kvr.grad
