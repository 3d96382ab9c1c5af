"""Seeded attention cases whose outputs are pinned bit for bit (tests/test_gpu_attention_bits.py against
tests/golden/attention_digests.json, written by tests/golden/make_attention_digests.py from an EARLIER build).  The kernels are
bitwise reproducible, so a change that only re-orders instructions, waits, addressing or staging depth must leave every digest
as it is.  The cases are the smallest shapes at which the staging ring, the DMA / LDS waits and the ragged paths can go wrong:
1..5 key tiles full and ragged, a steady-state ring, every padded head dim of the 64-wide image (D 56: last with the ones column,
D 64: first without), causal, key weights plain and packed, the query-split dK/dV pass, both sides of the deferred rescale, and one
case per wider template (which only the shared helpers touch).  Inputs are generated on the CPU (the suite's rnd)."""
import ctypes
import hashlib

import torch

from tests.test_gpu_kernels import rnd


def _case(name, B, H, Nq, Nk, D, causal=False, kw=False, packed=False, spike=None):
    return dict(name=name, B=B, H=H, Nq=Nq, Nk=Nk, D=D, causal=causal, kw=kw, packed=packed, spike=spike)


CASES = (
    [_case(f"tiles_nk{nk}", 1, 2, 160, nk, 40) for nk in (40, 64, 72, 128, 136, 192, 200, 264)]
    + [_case("ring_1024", 1, 8, 1024, 1024, 40)]
    + [_case(f"headdim_{d}", 1, 2, 200, 200, d) for d in (8, 16, 48, 56, 64)]
    + [_case("causal_77_d64", 3, 12, 77, 77, 64, causal=True), _case("causal_200_d40", 1, 2, 200, 200, 40, causal=True)]
    + [_case("keyw_16x77_d32", 2, 2, 16, 77, 32, kw=True), _case("keyw_packed_256x77_d40", 1, 8, 256, 77, 40, kw=True, packed=True)]
    + [_case("qsplit_1024x77", 1, 2, 1024, 77, 40), _case("qsplit_keyw_1024x77", 1, 2, 1024, 77, 40, kw=True)]
    + [_case(f"spike{s}_d{d}", 1, 2, 320, 320, d, spike=s) for d in (40, 64) for s in (6.0, 0.35)]
    + [_case("wide_d80", 1, 2, 136, 200, 80), _case("wide_d128", 1, 2, 64, 77, 128), _case("wide_d160", 1, 1, 72, 136, 160)]
)
TENSORS = ("out", "lse", "dq", "dk", "dv")


def run_case(c, dev, sync=True):
    """sdt_attention_fwd + sdt_attention_bwd through the C ABI on the current stream; returns {out, lse, dq, dk, dv} on the device
    (sync=False: the launches are left in flight)."""
    from stable_diffusion_training_amd import _lib
    lib = _lib.load()
    B, H, Nq, Nk, D = c["B"], c["H"], c["Nq"], c["Nk"], c["D"]
    C = H * D
    stream = torch.cuda.current_stream().cuda_stream
    q = rnd((B, Nq, C), dev, 1)
    k = rnd((B, Nk, C), dev, 2)
    v = rnd((B, Nk, C), dev, 3)
    do = rnd((B, Nq, C), dev, 4)
    if c["spike"] is not None:  # the construction of test_attention_rescale_branch_forced
        k[:, 200] = q[:, 7] * c["spike"]
        k[:, 290] = q[:, 150] * c["spike"]
    w = (1.0 + (torch.arange(Nk, device=dev) % 3 == 1).float()).contiguous() if c["kw"] else None
    if c["packed"]:  # k | v as the two halves of one (B, Nk, 2C) projection, gradients into a packed tensor of the same shape
        kv = torch.cat([k, v], dim=2).contiguous()
        dkv = torch.zeros_like(kv)
        kp, vp, dkp, dvp, ldkv, ldg = kv.data_ptr(), kv.data_ptr() + 2 * C, dkv.data_ptr(), dkv.data_ptr() + 2 * C, 2 * C, 2 * C
    else:
        dk, dv = torch.zeros_like(k), torch.zeros_like(v)
        kp, vp, dkp, dvp, ldkv, ldg = k.data_ptr(), v.data_ptr(), dk.data_ptr(), dv.data_ptr(), C, 0
    desc = _lib.SdtAttnDesc(B, H, Nq, Nk, D, C, ldkv, ldkv, C, D ** -0.5, int(c["causal"]), 0, ldg, ldg, 0,
                            w.data_ptr() if w is not None else None)
    out = torch.zeros_like(q)
    dq = torch.zeros_like(q)
    lse = torch.zeros(B, H, Nq, dtype=torch.float32, device=dev)
    _lib.call("sdt_attention_fwd", q.data_ptr(), kp, vp, out.data_ptr(), lse.data_ptr(), ctypes.addressof(desc), stream)
    need = lib.sdt_attention_bwd_workspace_bytes(ctypes.addressof(desc))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.call("sdt_attention_bwd", q.data_ptr(), kp, vp, out.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dkp, dvp,
              ws.data_ptr(), need, ctypes.addressof(desc), stream)
    if sync:
        torch.cuda.synchronize()
    if c["packed"]:
        dk, dv = dkv[..., :C].contiguous(), dkv[..., C:].contiguous()
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def digest(t):
    """sha256 of the tensor's raw bytes (row-major)."""
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
