"""The attention kernels, bit for bit: sha256 of out / lse / dq / dk / dv of the seeded cases of tests/attention_bits.py against
tests/golden/attention_digests.json (written from the build of the commit the fixture names, before the tile loops were
re-scheduled), and a run-to-run comparison behind other kernels' traffic.  Equality is the gate: there is no tolerance."""
import json
import os

import pytest
import torch

from tests.attention_bits import CASES, TENSORS, digest, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_digests.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(c["name"] for c in CASES)
    assert len(GOLDEN["commit"]) == 40


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_attention_bits_match_fixture(dev, case):
    res = run_case(case, dev)
    got = {t: digest(res[t]) for t in TENSORS}
    want = GOLDEN["cases"][case["name"]]
    bad = [t for t in TENSORS if got[t] != want[t]]
    assert not bad, f"{case['name']}: {bad} differ from the build of {GOLDEN['commit'][:7]}"


def test_attention_bits_stable_behind_other_traffic(dev):
    """A stage of the LDS ring re-used too early, or a wait that counts one piece too few, shows as a run-to-run difference once
    the timing around the kernel changes: the five-tile ragged case runs twice, each time with different attention launches in
    flight on two side streams (other shapes, other LDS contents), and every output must be equal."""
    case = next(c for c in CASES if c["name"] == "tiles_nk264")
    traffic = [[c for c in CASES if c["name"] in ("ring_1024", "headdim_64")], [c for c in CASES if c["name"] in ("wide_d80", "qsplit_1024x77")]]
    runs = []
    for prior in traffic:
        for c in prior:
            with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                run_case(c, dev, sync=False)
        runs.append(run_case(case, dev))
    for t in TENSORS:
        assert torch.equal(runs[0][t], runs[1][t]), t
