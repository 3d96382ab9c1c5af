"""Developer tool (CPU, NumPy): what the 8-bit AdamW state stores.  Runs the float32 restatement of the optimizer (tests/adamw_reference.py)
on 4096 parameters with log-normal curvature - gradient_i = scale_i * N(0, 1), scale_i = exp(sigma * N(0, 1)), times --gscale - for 400
steps at lr 1e-3, b2 0.999, block 16, three ways: fp32 moments, 8-bit m and ROOT s = sqrt(v) (what sdt_adamw8_step stores), 8-bit m and v
itself.  Prints the trajectory error of each 8-bit variant relative to the distance the fp32-state run travelled, and checks that an
all-zero-gradient block moves by the weight decay alone, bit-identically to fp32 states.
usage: python tools/adamw_codec_model.py [--sigma 3] [--gscale 1]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tests import adamw_reference as AR

ap = argparse.ArgumentParser()
ap.add_argument("--sigma", type=float, default=3.0)
ap.add_argument("--gscale", type=float, default=1.0)
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()
F32 = np.float32
n, bs, hp = 4096, 16, dict(wd=1e-2, b1=0.9, b2=0.999, eps=1e-8)
rs = np.random.RandomState(a.seed)
p0 = rs.standard_normal(n).astype(F32)
scale = np.exp(a.sigma * rs.standard_normal(n)) * a.gscale
scale[:bs] = 0.0  # one block never sees a gradient


def step8_v(p, g, state, cur):
    """The variant that stores v instead of its root."""
    mc, mi, vc, vi = state
    m, v = AR.block_dequantize(mc, mi), AR.block_dequantize(vc, vi)
    pn, mn, vn, _ = AR._update(p, g, m, v, cur, hp["wd"], hp["b1"], hp["b2"], hp["eps"])
    return pn, AR.block_quantize(mn, bs) + AR.block_quantize(vn, bs)


p32, m, v = p0.copy(), np.zeros(n, F32), np.zeros(n, F32)
ps, ss = p0.copy(), AR.init_state8(n, bs)
pv, sv = p0.copy(), AR.init_state8(n, bs)
t, prods = 0, (1.0, 1.0)
for _ in range(a.steps):
    g = (rs.standard_normal(n) * scale).astype(F32)
    cur, t, prods = AR.select_scalars(t, prods, hp["b1"], hp["b2"], lr=1e-3)
    p32, m, v = AR.step32(p32, g, m, v, cur, **hp)
    ps, ss = AR.step8(ps, g, ss, cur, bs=bs, **hp)
    pv, sv = step8_v(pv, g, sv, cur)
dist = np.linalg.norm(p32.astype(np.float64) - p0)
err = lambda p: float(np.linalg.norm(p.astype(np.float64) - p32) / dist)
print(f"sigma {a.sigma} gscale {a.gscale} steps {a.steps}: store s {err(ps):.3f}, store v {err(pv):.3f} (trajectory error / distance travelled)")
zero_ok = np.array_equal(ps[:bs].view(np.int32), p32[:bs].view(np.int32)) and not ss[0][0].any() and not ss[2][0].any()
print(f"all-zero-gradient block: moved by the decay alone, bit-identical to fp32 states: {zero_ok}")
