"""Float64 references, case tables and buffer layouts for the LoRA kernels (sdt_lora_merge / sdt_lora_project) and lora.py, shared by
tests/test_lora_cpu.py (which proves them) and the GPU files.

merge:    v = W0 + s * bf16(A) @ bf16(B)                 (mirror: RNE bf16 of v; folded checkpoint: v itself)
project:  dA = s * dW @ bf16(B)^T,  dB = s * bf16(A)^T @ dW   - the gradient of f(W0 + s * A @ B) with dW = df/dW, evaluated at the
          bf16 factors the merge used.
"""
import torch

from tests import kernel_checks as kc

BF = torch.bfloat16

# (K, N, r): the smallest that can go wrong - one partial tile; edge tiles both ways; the tiny model's context projection; a padded rank
# step; a rank of two instruction steps with edge tiles; the SD1.5 width; several tiles with a full-length reduction and the top rank
CASES = [(8, 8, 4), (40, 72, 4), (48, 64, 8), (64, 192, 32), (136, 72, 64), (320, 320, 16), (640, 1280, 128)]
SCALES = (0.5, 1.0, 2.0)
RANDOM_CASES = [(136, 72, 64), (320, 320, 16)]
FRONT = 1024  # elements in front of the first leaf and behind the last one: poisoned, must stay untouched


def bf(x):
    """The bf16 (RNE) rounding of fp32 values, as float64."""
    return x.to(torch.float32).to(BF).double()


def merge_ref64(W0, A, B, s):
    return W0.double() + s * (bf(A) @ bf(B))


def project_ref64(dW, A, B, s):
    """(dA, dB) in float64; dW is the bf16 weight gradient (any dtype that holds it exactly)."""
    d = dW.double()
    return s * (d @ bf(B).T), s * (bf(A).T @ d)


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def rne_bf16_bits(x64):
    """Integer view of the bf16 RNE rounding of float64 values that fp32 holds exactly."""
    return kc.bits(kc.rne_bf16(x64))


def exact_operands(K, N, r, seed):
    """Integers in -3..3 for A, B, dW; W0 a multiple of 1/8 with |W0| <= 128: every product and sum below is exact in fp32."""
    A = kc.exact_ints((K, r), -3, 3, seed, dtype=torch.float32)
    B = kc.exact_ints((r, N), -3, 3, seed + 1, dtype=torch.float32)
    dW = kc.exact_ints((K, N), -3, 3, seed + 2, dtype=BF)
    g = torch.Generator().manual_seed(seed + 3)
    W0 = torch.randint(-1024, 1025, (K, N), generator=g).to(torch.float32) / 8
    return W0, A, B, dW


def exact_bounds(K, N, r, s):
    """[(what, largest |partial sum| in units, limit)]: the unit is the common denominator of every term (1/8 for the merge: W0 is a
    multiple of 1/8 and s * integer one of 1/2; 1/2 for the projections), so a partial sum is unit * integer and exact while the integer
    stays below 2^24."""
    merge = (128 + s * 9 * r) * 8
    da = s * 9 * N * 2
    db = s * 9 * K * 2
    return [(f"merge {K}x{N} r{r} s{s}", merge, kc.LIMIT), (f"dA {K}x{N} r{r} s{s}", da, kc.LIMIT), (f"dB {K}x{N} r{r} s{s}", db, kc.LIMIT)]


def layout(cases, order=None):
    """Flat buffers for a grouped launch: every leaf at an 8-aligned offset with gaps of 0, 8 or 16 elements between neighbours (the
    8-element alignment gaps and non-adapted neighbours of a real store), FRONT elements in front and behind.  cases: [(K, N, r, s)];
    order: the order of the jobs in the table (the offsets follow the case order).
    Returns (jobs: list of dict in table order, sizes: dict(master=, ab=, dw=, grad=))."""
    pos = dict(master=FRONT, ab=FRONT, dw=FRONT)
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
        j["dw_off"] = take("dw", K * N, i + 2)
        placed.append(j)
    order = list(range(len(cases))) if order is None else list(order)
    jobs, tm, tp = [], 0, 0
    for i in order:
        j = dict(placed[i])
        ta, tb = (j["K"] + 63) // 64, (j["N"] + 63) // 64
        j.update(tile0_merge=tm, tile0_project=tp, tiles_da=ta)
        tm += ta * tb
        tp += ta + tb
        jobs.append(j)
    return jobs, {k: v + FRONT for k, v in pos.items()}


def job_table(jobs):
    """The ctypes array sdt_lora_merge / sdt_lora_project take (w_off = f_off = w0_off, ga_off / gb_off = a_off / b_off: a store's
    mirror and gradient share the offsets of its master)."""
    from stable_diffusion_training_amd import _lib
    return (_lib.SdtLoraJob * len(jobs))(*[
        _lib.SdtLoraJob(j["w0_off"], j["a_off"], j["b_off"], j["w0_off"], j["w0_off"], j["dw_off"], j["a_off"], j["b_off"], j["K"], j["N"],
                        j["r"], j["s"], j["tile0_merge"], j["tile0_project"], j["tiles_da"], 0) for j in jobs])
