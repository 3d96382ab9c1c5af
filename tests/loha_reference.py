"""Float64 references, case tables, table builders, exact operands and the derived error bound of LoHa (include/sdt.h "LoHa"; DESIGN.md
"LoHa"), shared by tests/test_loha_cpu.py (which proves them) and the GPU files.

P_i = bf16(A_i) @ bf16(B_i)
merge:    v = W0 + s * P1 * P2                          (mirror: RNE bf16 of v; folded checkpoint: v itself)
project:  G1 = dW * P2, G2 = dW * P1 (exact here: the kernel rounds them to bf16, which the bound below pays for)
          dA_i = s * G_i @ bf16(B_i)^T,  dB_i = s * bf16(A_i)^T @ G_i
"""
import torch

from tests import kernel_checks as kc
from tests import locon_reference as lc
from tests import lora_reference as lr

BF = torch.bfloat16
SCALES = lr.SCALES
RANKS = (4, 8, 16, 32)
U8, U24 = 2.0 ** -8, 2.0 ** -24  # unit roundoffs of bf16 and fp32


def rows():
    return lc.rows()


def cases(C):
    """(K, N, r) of the exact cases: one partial tile; the last K of one chunk; exactly one chunk; one chunk and 8 rows; two chunks and a
    ragged third with three column stripes at the top rank; a 3x3 kernel of 64 channels with edge tiles both ways at the top rank."""
    return [(72, 8, 4), (C - 8, 72, 4), (C, 64, 8), (C + 8, 72, 16), (2 * C + 40, 192, 32), (9 * 64, 136, 32)]


def random_cases(C):
    return [(136, 72, 32), (320, 320, 16), (2 * C + 40, 192, 8)]


def products(A1, B1, A2, B2):
    return lr.bf(A1) @ lr.bf(B1), lr.bf(A2) @ lr.bf(B2)


def merge_ref64(W0, A1, B1, A2, B2, s):
    P1, P2 = products(A1, B1, A2, B2)
    return W0.double() + s * (P1 * P2)


def project_ref64(dW, A1, B1, A2, B2, s):
    """(dA1, dB1, dA2, dB2) in float64, G exact; dW is the bf16 weight gradient (any dtype that holds it exactly)."""
    d = dW.double()
    P1, P2 = products(A1, B1, A2, B2)
    G1, G2 = d * P2, d * P1
    return s * (G1 @ lr.bf(B1).T), s * (lr.bf(A1).T @ G1), s * (G2 @ lr.bf(B2).T), s * (lr.bf(A2).T @ G2)


def exact_operands(K, N, r, seed):
    """(W0, A1, B1, A2, B2, dW): factors in {-1, 0, 1}, so P is an integer with |P| <= r <= 32; dW in {0, +-1, +-2, +-4}, so G = dW * P has
    at most 6 significant bits and bf16 holds it; W0 a multiple of 1/8 with |W0| <= 128.  exact_bounds() bounds every partial sum."""
    f = [kc.exact_ints(shape, -1, 1, seed + t, dtype=torch.float32) for t, shape in enumerate(((K, r), (r, N), (K, r), (r, N)))]
    g = torch.Generator().manual_seed(seed + 4)
    mag = torch.tensor([0.0, 1.0, 2.0, 4.0])[torch.randint(0, 4, (K, N), generator=g)]
    sign = torch.randint(0, 2, (K, N), generator=g).float() * 2 - 1
    dW = (mag * sign).to(BF)
    W0 = torch.randint(-1024, 1025, (K, N), generator=g).to(torch.float32) / 8
    return (W0, *f, dW)


def exact_bounds(K, N, r, s):
    """[(what, largest |partial sum| in units, limit)] as lr.exact_bounds: |P| <= r, |P1 P2| <= r^2 (integers); the merged sum in units of
    1/8; |G| <= 4 r with <= 6 significant bits; the projections' partial sums in units of 1/2."""
    return [(f"P r{r}", r, kc.LIMIT), (f"P1*P2 r{r}", r * r, kc.LIMIT), (f"merge {K}x{N} r{r} s{s}", (128 + s * r * r) * 8, kc.LIMIT),
            (f"G r{r} (bf16: 8 significant bits, G = 2^e * P with |P| <= 32 < 2^6)", r, 63),
            (f"dA {K}x{N} r{r} s{s}", s * 4 * r * N * 2, kc.LIMIT), (f"dB {K}x{N} r{r} s{s}", s * 4 * r * K * 2, kc.LIMIT)]


def layout(cases_, order=None):
    """lr.layout for side 1, with A2 / B2 of every case appended to the `ab` buffer (a2_off, b2_off; the same alignment gaps)."""
    jobs, sizes = lr.layout(cases_, order)
    pos = sizes["ab"] - lr.FRONT
    side2 = {}
    for i, (K, N, r, s) in enumerate(cases_):
        a2 = pos
        b2 = (a2 + K * r + 7) // 8 * 8 + 8 * (i % 3)
        pos = (b2 + r * N + 7) // 8 * 8 + 8 * ((i + 1) % 3)
        side2[i] = (a2, b2)
    for j in jobs:
        j["a2_off"], j["b2_off"] = side2[j["index"]]
    sizes = dict(sizes, ab=pos + lr.FRONT)
    return jobs, sizes


def loha_table(jobs, C):
    """The SdtLohaJob array beside lr.job_table(jobs) / lc.split_table(jobs, C) and the workspace's (counter bytes, total bytes): the
    counters of the split projection, then two partial sets - 2 * stripes * chunks * r * 64 floats - per job of more than one chunk."""
    from stable_diffusion_training_amd import _lib
    out, cnt, part = [], 0, 0
    for j in jobs:
        tb, ch = (j["N"] + 63) // 64, lc.chunks(j["K"], C)
        out.append(_lib.SdtLohaJob(j["a2_off"], j["b2_off"], j["a2_off"], j["b2_off"], part, j["K"], j["N"]))
        cnt += tb
        part += 2 * tb * ch * j["r"] * 64 if ch > 1 else 0
    counter_bytes = (4 * cnt + 255) // 256 * 256
    return (_lib.SdtLohaJob * len(out))(*out), counter_bytes, counter_bytes + 4 * part


def gamma(n, u=U24):
    return n * u / (1 - n * u)


def g_error(dW, A, B):
    """(|G|, eG) for G = dW * P, P = bf16(A) @ bf16(B): the kernel's G^ = bf16(fl32(dW * P^)) with P^ the fp32 MFMA accumulation of r exact
    products, |P^ - P| <= gamma_r * sum_q |A||B| - an ABSOLUTE error, P may cancel - so
    |G^ - G| <= |dW| * (|P| * ((1 + u8)(1 + u24) - 1) + gamma_r * sum_q |A||B| * (1 + u8)(1 + u24))."""
    r = A.shape[1]
    d = dW.double().abs()
    P, Pabs = lr.bf(A) @ lr.bf(B), lr.bf(A).abs() @ lr.bf(B).abs()
    two = (1 + U8) * (1 + U24)
    return d * P.abs(), d * (P.abs() * (two - 1) + gamma(r) * Pabs * two)


def projection_bounds(dW, A1, B1, A2, B2, s, C):
    """Derived bounds (bA1, bB1, bA2, bB2) on |kernel - project_ref64|.  A factor gradient is fl(s * S^), S^ the fp32 accumulation of the
    exact products G^ * bf16(X) (bf16 x bf16 is exact in fp32) carrying m roundings - N for dA (N - 1 additions and the scaling), for dB
    lc.db_roundings(K, C): the additions inside a chunk, the chunks - 1 partial additions, the scaling:
    |fl(s S^) - s S| <= s * ((1 + gamma_m) * sum eG |X| + gamma_m * sum |G| |X|)."""
    K, N = dW.shape
    out = []
    for (Aother, Bother), A, B in (((A2, B2), A1, B1), ((A1, B1), A2, B2)):
        G, eG = g_error(dW, Aother, Bother)
        Bt, At = lr.bf(B).abs().T, lr.bf(A).abs().T
        ma, mb = N, lc.db_roundings(K, C)
        out.append(s * ((1 + gamma(ma)) * (eG @ Bt) + gamma(ma) * (G @ Bt)))
        out.append(s * ((1 + gamma(mb)) * (At @ eG) + gamma(mb) * (At @ G)))
    return tuple(out)


def merge_bound(W0, A1, B1, A2, B2, s):
    """|v - merge_ref64|: two r-term fp32 accumulations, the product, the scaling and the sum: (1 + gamma_r)^2 (1 + u)^3 - 1 <= gamma_{2r+3}
    on the magnitudes |W0| + s * (sum |A1||B1|) * (sum |A2||B2|)."""
    r = A1.shape[1]
    return gamma(2 * r + 3) * (W0.double().abs() + s * (lr.bf(A1).abs() @ lr.bf(B1).abs()) * (lr.bf(A2).abs() @ lr.bf(B2).abs()))


def loha_forward64(x, W0, A1, B1, A2, B2, s, stride):
    """conv(x, W0 + s * (A1 B1) * (A2 B2) as HWIO) in float64, NCHW - the function whose weight gradient the projection maps back."""
    import torch.nn.functional as F
    kh, kw, Cin, Cout = W0.shape
    W = W0 + s * ((A1 @ B1) * (A2 @ B2)).view(kh, kw, Cin, Cout)
    return F.conv2d(x, W.permute(3, 2, 0, 1).contiguous(), stride=stride, padding=kh // 2)
