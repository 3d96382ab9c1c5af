"""Developer tool: SHA-256 of every buffer the adapter kernels write (csrc/lora.hip: LoRA, DoRA, LoCon, LoHa), on fixed-seed random
operands - where, unlike on the exact-integer operands of tests/test_gpu_*_kernels.py, a changed summation order changes bits.  Per family:
the random shapes of tests/*_reference.py as one grouped table, then the exact cases' shapes as a shuffled grouped table; every entry point
once, on poisoned outputs (0xA5 bytes; arrival counters zero), whole buffers hashed, so a stray write shows too.  A/B of two builds: run
once per build (SDT_LIB selects it: tools/build_variant.sh, or a build of another commit) and diff the two outputs.
usage: adapter_bits_ab.py > bits.txt"""
import hashlib
import os
import random
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stable_diffusion_training_amd import _lib
from tests import dora_reference as dr, locon_reference as lc, loha_reference as lh, lora_reference as lr

dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
C = lc.rows()
up = lambda t: torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
poison = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
P = lambda t: t.data_ptr()


def digest(tag, **bufs):
    torch.cuda.synchronize()
    for name, t in bufs.items():
        print(f"{tag:16s} {name:9s} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


def workspace(counter_bytes, nbytes):
    ws = poison(nbytes)
    ws[:counter_bytes] = 0
    return ws


def run(family, shapes, shuffle, seed):
    cases = [(K, N, r, lr.SCALES[i % 3]) for i, (K, N, r) in enumerate(shapes)]
    order = list(range(len(cases)))
    if shuffle:
        random.Random(seed).shuffle(order)
    jobs, sz = {"dora": dr.layout, "loha": lh.layout}.get(family, lr.layout)(cases, order)
    g = torch.Generator().manual_seed(seed)
    master, ab = (torch.randn(sz[k], generator=g).to(dev) for k in ("master", "ab"))  # (gaps and margins random too: never read)
    dw = torch.randn(sz["dw"], generator=g).to(torch.bfloat16).to(dev)
    w, f, grad, restored = poison(2 * sz["master"]), poison(4 * sz["master"]), poison(4 * sz["ab"]), poison(2 * sz["master"])
    jt, n, tag = lr.job_table(jobs), len(jobs), family + ("/shuffled" if shuffle else "")
    jd = up(jt)
    if family == "dora":
        dt = dr.job_tables(jobs)[1]
        dd, stats, m = up(dt), poison(4 * sz["stat"]), poison(4 * sz["ab"])
        _lib.call("sdt_dora_init_magnitude", P(master), P(ab), P(m), jt, dt, P(jd), P(dd), n, stream)
        _lib.call("sdt_dora_merge", P(master), P(ab), P(w), P(f), P(stats), jt, dt, P(jd), P(dd), n, stream)
        _lib.call("sdt_dora_project", P(dw), P(master), P(ab), P(grad), P(stats), jt, dt, P(jd), P(dd), n, stream)
        digest(tag, mirror=w, fp32=f, grad=grad, stats=stats, magnitude=m)
    elif family == "loha":
        st, (xt, cb, nb) = lc.split_table(jobs, C)[0], lh.loha_table(jobs, C)
        sd, xd, ws = up(st), up(xt), workspace(cb, nb)
        _lib.call("sdt_loha_merge", P(master), P(ab), P(w), P(f), jt, xt, P(jd), P(xd), n, stream)
        _lib.call("sdt_loha_project", P(dw), P(ab), P(grad), jt, st, xt, P(jd), P(sd), P(xd), n, P(ws), nb, stream)
        digest(tag, mirror=w, fp32=f, grad=grad, workspace=ws)
    else:
        _lib.call("sdt_lora_merge", P(master), P(ab), P(w), P(f), jt, P(jd), n, stream)
        if family == "locon":
            st, cb, nb = lc.split_table(jobs, C)
            sd, ws = up(st), workspace(cb, nb)
            _lib.call("sdt_lora_project_split", P(dw), P(ab), P(grad), jt, st, P(jd), P(sd), n, P(ws), nb, stream)
            digest(tag, workspace=ws)
        else:
            _lib.call("sdt_lora_project", P(dw), P(ab), P(grad), jt, P(jd), n, stream)
        digest(tag, mirror=w, fp32=f, grad=grad)
    _lib.call("sdt_lora_restore", P(master), P(restored), jt, P(jd), n, stream)
    digest(tag, restored=restored)


print(f"# {_lib.LIB_PATH}", file=sys.stderr)
for i, (family, rand, exact) in enumerate((("lora", lr.RANDOM_CASES, lr.CASES), ("dora", dr.RANDOM_CASES, dr.CASES),
                                           ("locon", lc.random_cases(C), lc.cases(C)), ("loha", lh.random_cases(C), lh.cases(C)))):
    run(family, rand, False, 1000 + 10 * i)
    run(family, exact, True, 1005 + 10 * i)
