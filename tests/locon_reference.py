"""Case tables, the split table and the float64 form of LoCon (include/sdt.h "LoCon"; DESIGN.md "LoCon"), shared by
tests/test_locon_cpu.py (which proves them) and the GPU files.  The float64 merge / projection references, the operand builders and the
buffer layout are tests/lora_reference.py's: a convolution kernel [kh, kw, Cin, Cout] is the matrix [kh*kw*Cin, Cout] there."""
import ctypes

import torch

from tests import lora_reference as lr

SCALES = lr.SCALES


def rows():
    """The chunk length of sdt_lora_project_split (a compile-time constant of the library)."""
    from stable_diffusion_training_amd import _lib
    return int(_lib.load().sdt_lora_project_split_rows())


def cases(C):
    """(K, N, r) of the exact cases: one partial tile; the last K of one chunk; exactly one chunk; one chunk and 8 rows; two chunks and a
    ragged third with three column stripes; a 3x3 kernel of 64 channels with edge tiles both ways; four chunks at the top rank."""
    return [(72, 8, 4), (C - 8, 72, 4), (C, 64, 8), (C + 8, 72, 16), (2 * C + 40, 192, 32), (9 * 64, 136, 64), (3 * C + 72, 72, 128)]


def random_cases(C):
    return [(2 * C + 40, 72, 16), (3 * C + 72, 136, 64)]


def chunks(K, C):
    return (K + C - 1) // C


def split_table(jobs, C):
    """The SdtLoraSplitJob array beside lr.job_table(jobs) and the workspace's (counter bytes, total bytes), by the rule of include/sdt.h:
    one int32 counter per dB stripe rounded up to 256 bytes, then stripes * chunks * r * 64 floats for every job of more than one chunk."""
    from stable_diffusion_training_amd import _lib
    out, tile0, cnt, part = [], 0, 0, 0
    for j in jobs:
        ta, tb, ch = (j["K"] + 63) // 64, (j["N"] + 63) // 64, chunks(j["K"], C)
        out.append(_lib.SdtLoraSplitJob(part, j["K"], j["N"], tile0, ch, cnt, 0))
        tile0 += ta + tb * ch
        cnt += tb
        part += tb * ch * j["r"] * 64 if ch > 1 else 0
    counter_bytes = (4 * cnt + 255) // 256 * 256
    return (_lib.SdtLoraSplitJob * len(out))(*out), counter_bytes, counter_bytes + 4 * part


def db_roundings(K, C):
    """The roundings one dB element of sdt_lora_project_split carries: min(K, C) - 1 additions inside a chunk (the first product enters
    a zero accumulator exactly), chunks - 1 additions of chunk sums, one scaling."""
    return (min(K, C) - 1) + (chunks(K, C) - 1) + 1


def conv_leaves(spec, components):
    """The 4-D '/kernel' leaves of `spec` under one of the named components, in spec order - written without lora.select_leaves."""
    out = []
    for path, shape in spec:
        parts = path.split("/")
        if parts[-1] == "kernel" and len(tuple(shape)) == 4 and set(parts[:-1]) & set(components):
            out.append(path)
    return out


def locon_forward64(x, W0, A, B, s, stride):
    """(merged, decomposed) in float64, NCHW: conv(x, W0 + s * (A @ B) as HWIO) and conv(x, W0) + s * conv1x1(conv_kxk(x, A), B), the
    kohya / LyCORIS form with lora_down[q, i, kh, kw] = A[(t * Cin + i), q] and lora_up[o, q, 0, 0] = B[q, o]."""
    import torch.nn.functional as F
    kh, kw, Cin, Cout = W0.shape
    r = A.shape[1]
    pad = kh // 2
    oihw = lambda w: w.permute(3, 2, 0, 1).contiguous()
    merged = F.conv2d(x, oihw(W0 + s * (A @ B).view(kh, kw, Cin, Cout)), stride=stride, padding=pad)
    down = F.conv2d(x, oihw(A.view(kh, kw, Cin, r)), stride=stride, padding=pad)
    up = F.conv2d(down, B.T.contiguous().view(Cout, r, 1, 1))
    return merged, F.conv2d(x, oihw(W0), stride=stride, padding=pad) + s * up


def sizeof_split_job():
    from stable_diffusion_training_amd import _lib
    return ctypes.sizeof(_lib.SdtLoraSplitJob)
