"""Writes tests/golden/attention_digests.json ON A GPU: sha256 of the raw bytes of out / lse / dq / dk / dv of every case of
tests/attention_bits.py, produced by the build in the tree (or the one SDT_LIB names).  The fixture pins the attention kernels'
bits across changes that may only re-order their instructions, so it is written from a build of the commit BEFORE such a change
and records that commit's hash; it is never regenerated from the code under test.
Run:  python tests/golden/make_attention_digests.py <commit hash of the build> [out.json]   then copy the file to tests/golden/."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.attention_bits import CASES, TENSORS, digest, run_case  # noqa: E402


def main(commit, out_path):
    dev = torch.device("cuda:0")
    cases = {}
    for c in CASES:
        res = run_case(c, dev)
        cases[c["name"]] = {t: digest(res[t]) for t in TENSORS}
        print(c["name"], cases[c["name"]]["out"][:16])
    with open(out_path, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "attention_digests.json"))
