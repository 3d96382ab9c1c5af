"""Float64 references, case tables and buffer layouts for the DoRA kernels (sdt_dora_merge / sdt_dora_init_magnitude /
sdt_dora_project; include/sdt.h "DoRA"), shared by tests/test_dora_cpu.py (which proves them) and the GPU files.

The references evaluate at the kernels' rounding points: bf16(A), bf16(B), the fp32 column norm c and gain g, and bf16(fl32(bf16(B) * g)).

merge:    v = W0 + s * bf16(A) @ bf16(B);  q[n] = sum_k v[k][n]^2;  c = fl32(sqrt(q));  g = fl32(m / c), 0 where c == 0;  W' = v * g
project:  the norm is held constant (the paper's section 4.3).  With G = dW' and P = bf16(A)^T @ G:
          dB = (s * P) * g,   dA = s * G @ bf16(fl32(bf16(B) * g))^T,   u = sum_k G * W0 + s * sum_q bf16(B) * P,   dm = u / c (0 where c == 0)

c is a float64 sqrt rounded to fp32 by numpy (53 >= 2 * 24 + 2 bits: for an fp32 argument that is the correctly rounded fp32 root).
torch's float32 sqrt is NOT used anywhere: it is not correctly rounded on every platform.
"""
import numpy as np
import torch

from tests import kernel_checks as kc
from tests import lora_reference as lr

BF = torch.bfloat16
# (K, N, r): one partial tile; edge tiles both ways; two instruction steps of rank; several stripes; a stripe that walks ten K blocks at
# the top rank
CASES = [c for c in lr.CASES if c in ((8, 8, 4), (40, 72, 4), (136, 72, 64), (320, 320, 16), (640, 1280, 128))]
SCALES = lr.SCALES
RANDOM_CASES = lr.RANDOM_CASES
FRONT = lr.FRONT
bf, gamma = lr.bf, lr.gamma


def fl32_sqrt(q64):
    """sqrt in float64, rounded once to fp32 (numpy; not torch's float32 sqrt)."""
    return torch.from_numpy(np.sqrt(q64.double().numpy()).astype(np.float32))


def fl32_div(a, b):
    """a / b in float64 rounded once to fp32 - the correctly rounded quotient of fp32 operands - and 0 where b == 0."""
    a, b = a.double(), b.double()
    return torch.where(b == 0, torch.zeros_like(a), a / torch.where(b == 0, torch.ones_like(b), b)).float()


def column_stats(v64, m=None):
    """(q float64, c fp32, g fp32 or None) of v [K][N]."""
    q = (v64.double() ** 2).sum(0)
    c = fl32_sqrt(q)
    return q, c, (None if m is None else fl32_div(m, c))


def merge_ref64(W0, A, B, s, g):
    """W' in float64 at the fp32 gain g: (W0 + s * bf16(A) @ bf16(B)) * g."""
    return lr.merge_ref64(W0, A, B, s) * g.double()[None, :]


def scaled_b(B, g):
    """bf16(fl32(bf16(B) * g)) as float64: the B operand of the dA stripes."""
    return bf((bf(B) * g.double()[None, :]).float())


def project_ref64(G, W0, A, B, s, c, g):
    """(dA, dB, dm, u) in float64 at the fp32 statistics c, g; G is the bf16 weight gradient (any dtype that holds it exactly)."""
    Gd = G.double()
    P = bf(A).T @ Gd
    dB = (s * P) * g.double()[None, :]
    dA = s * (Gd @ scaled_b(B, g).T)
    u = (Gd * W0.double()).sum(0) + s * (bf(B) * P).sum(0)
    cd = c.double()
    dm = torch.where(cd == 0, torch.zeros_like(u), u / torch.where(cd == 0, torch.ones_like(cd), cd))
    return dA, dB, dm, u


def exact_operands(K, N, r, seed):
    """W0 integers in -8..8, A and B in -1..1, G in -3..3: with s in SCALES every partial sum below is exact in fp32."""
    W0 = kc.exact_ints((K, N), -8, 8, seed + 3, dtype=torch.float32)
    A = kc.exact_ints((K, r), -1, 1, seed, dtype=torch.float32)
    B = kc.exact_ints((r, N), -1, 1, seed + 1, dtype=torch.float32)
    G = kc.exact_ints((K, N), -3, 3, seed + 2, dtype=BF)
    return W0, A, B, G


def exact_magnitude(c):
    """m[n] = c[n] * 2^e, e cycling over -1, 0, 1 by column: g = m / c = 2^e bit for bit.  Returns (m, g)."""
    g = torch.tensor([0.5, 1.0, 2.0])[torch.arange(c.numel()) % 3]
    return c * g, g


def exact_units(W0, A, B, G, s):
    """(largest 4 q[n], largest 2 * (sum_k |G||W0| + s * sum_q |B| sum_k |A||G|)): v is a multiple of 1/2 (s * integer), so q is one of
    1/4 and its partial sums - all non-negative - are bounded by q; every term of u is a multiple of 1/2 and every partial sum of u and
    of P is bounded by the sum of the magnitudes.  Below 2^24 both are exact in fp32 in any order."""
    v = lr.merge_ref64(W0, A, B, s)
    assert torch.equal(v * 2, (v * 2).round())
    absu = (G.double().abs() * W0.double().abs()).sum(0) + s * (B.double().abs() * (A.double().abs().T @ G.double().abs())).sum(0)
    return float((v ** 2).sum(0).max()) * 4, float(absu.max()) * 2


def layout(cases, order=None):
    """lora_reference.layout with the magnitude leaf: per case also m_off (in the ab buffer, after A and B) and stat_off (c [N] then
    g [N] in the statistics buffer), gaps of 0, 8 or 16 elements between neighbours, FRONT elements in front and behind; the tables get
    stripe0_merge beside tile0_merge / tile0_project.  Returns (jobs in table order, sizes: dict(master=, ab=, dw=, stat=))."""
    pos = dict(master=FRONT, ab=FRONT, dw=FRONT, stat=FRONT)
    placed = []

    def take(buf, n, i):
        off = pos[buf]
        pos[buf] = (off + n + 7) // 8 * 8 + 8 * (i % 3)
        return off

    for i, (K, N, r, s) in enumerate(cases):
        j = dict(K=K, N=N, r=r, s=s, index=i)
        j["w0_off"] = take("master", K * N, i)
        j["a_off"] = take("ab", K * r, i)
        j["b_off"] = take("ab", r * N, i + 1)
        j["m_off"] = take("ab", N, i + 2)
        j["dw_off"] = take("dw", K * N, i + 2)
        j["stat_off"] = take("stat", 2 * N, i + 1)
        placed.append(j)
    order = list(range(len(cases))) if order is None else list(order)
    jobs, tm, tp, sm = [], 0, 0, 0
    for i in order:
        j = dict(placed[i])
        ta, tb = (j["K"] + 63) // 64, (j["N"] + 63) // 64
        j.update(tile0_merge=tm, tile0_project=tp, tiles_da=ta, stripe0_merge=sm)
        tm += ta * tb
        tp += ta + tb
        sm += tb
        jobs.append(j)
    return jobs, {k: v + FRONT for k, v in pos.items()}


def job_tables(jobs):
    """(SdtLoraJob array, SdtDoraJob array) the DoRA entry points take (dm at m's offset: a store's gradient shares its master's)."""
    from stable_diffusion_training_amd import _lib
    return lr.job_table(jobs), (_lib.SdtDoraJob * len(jobs))(*[
        _lib.SdtDoraJob(j["m_off"], j["m_off"], j["stat_off"], j["N"], j["stripe0_merge"]) for j in jobs])
