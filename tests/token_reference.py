"""Host references of the new-token kernels (include/sdt.h "NEW TOKENS") at the kernels' rounding points: float32 / float64 numpy,
nothing of the code under test."""
import numpy as np
import torch

SHAPES = (5, 12, 768)   # D: the scalar path, the vector path at a width that is no multiple of 8, CLIP-L's width
S, NSEQ, V = 7, 3, 11   # sequence length, sequences, vocabulary of the kernel cases
N_EXT = (1, 5)
RETRACT_SHAPES = ((1, 8), (3, 12), (5, 768))


def rows_of(ids, tok, ext):
    """(rows, D) float32: tok[id] for 0 <= id < V, ext[id - V] for V <= id < V + n, +0.0 for every other id."""
    tok, ext = np.asarray(tok, np.float32), np.asarray(ext, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    Vv, n = tok.shape[0], ext.shape[0]
    table = np.concatenate([tok, ext, np.zeros((1, tok.shape[1]), np.float32)])
    idx = np.where((ids >= 0) & (ids < Vv + n), ids, Vv + n)
    return table[idx]


def forward_ref(ids, tok, ext, pos):
    """bf16 (rows, D) as a torch tensor: rne_bf16(fl32(t + pos[r % S])) - one float32 add, one rounding to bf16."""
    pos = np.asarray(pos, np.float32)
    ids = np.asarray(ids).reshape(-1)
    t = rows_of(ids, tok, ext)
    p = pos[np.arange(ids.shape[0]) % pos.shape[0]]
    return torch.from_numpy((t + p).astype(np.float32)).to(torch.bfloat16)


def backward_ref(ids, dout, Vv, n):
    """float32 (n, D): for every new token the sum of the rows of dout (float32 values of the bf16 gradient) that carry its id, a
    sequential float32 loop in row order that starts at +0."""
    ids = np.asarray(ids).reshape(-1)
    dout = np.asarray(dout, np.float32)
    out = np.zeros((n, dout.shape[1]), np.float32)
    for r in range(ids.shape[0]):
        j = int(ids[r]) - Vv
        if 0 <= j < n:
            out[j] = (out[j] + dout[r]).astype(np.float32)
    return out


def retract_stats(ext):
    """(mean, unbiased std) of all values in float64, two passes."""
    x = np.asarray(ext, np.float32).astype(np.float64).reshape(-1)
    mean = x.sum() / x.size
    std = float(np.sqrt(((x - mean) ** 2).sum() / (x.size - 1))) if x.size > 1 else 0.0
    return float(mean), std


def retract_factor(std, target_std, power):
    """(float32) pow(target_std / std, power) from a float64 pow; 1 when std == 0."""
    return np.float32(1.0) if std == 0 else np.float32(np.power(np.float64(target_std) / np.float64(std), np.float64(power)))


def retract_apply(ext, factor):
    """fl32(x * factor): one float32 multiply."""
    return (np.asarray(ext, np.float32) * np.float32(factor)).astype(np.float32)


def sum_bound(x64, terms_abs_sum=None):
    """|error| of an ordered double sum of n terms against the exact sum, whatever the order: (n - 1) * 2^-53 * sum |x_i| to first order
    (Higham, Accuracy and Stability, (4.4)); doubled for the second-order terms and for numpy's own (pairwise) summation error on the
    reference side, which obeys the same bound."""
    x64 = np.asarray(x64, np.float64).reshape(-1)
    s = float(np.abs(x64).sum()) if terms_abs_sum is None else terms_abs_sum
    return 2.0 * (x64.size - 1) * 2.0 ** -53 * s + 5e-324


def id_patterns(n_ext, seed):
    """{name: int32 (NSEQ * S,)} the id patterns of the kernel cases."""
    g = np.random.default_rng(seed)
    rows = NSEQ * S
    base = g.integers(0, V, rows).astype(np.int32)
    out = {"no_new": base.copy()}
    one = base.copy()
    one[[1, 4, 9, 16]] = V + n_ext - 1
    out["one_new_in_several_rows"] = one
    out["all_rows_one_new"] = np.full(rows, V + (n_ext - 1) // 2, np.int32)
    mixed = base.copy()
    mixed[::2] = V + g.integers(0, n_ext, mixed[::2].shape[0]).astype(np.int32)
    out["mixed"] = mixed
    bad = base.copy()
    bad[[0, 5, 13]] = (-1, V + n_ext, 2 ** 30)
    bad[7] = V  # a valid new id beside the bad ones
    out["bad_ids"] = bad
    return out


BAD_ROWS = (0, 5, 13)
