"""ParamStore.optimizer_step, launch for launch, and save_training_state, name for name, against tests/golden/optimizer_launches.json
(tests/golden/make_optimizer_launches.py: how a CPU store runs the dispatch under a recorder, the cases, and what a record holds).
The golden file pins the launch sequence of every optimizer x quantise x schedule x EMA x clip x gradient source, the fused-norm,
sharded and resumed steps, the refusals that must come before any launch, and what a training-state file holds per optimizer."""
import json
import os

import pytest
import torch

from stable_diffusion_training_amd import checkpoint
from tests.golden import make_optimizer_launches as gen

with open(gen.OUT) as _f:
    GOLDEN = json.load(_f)
LAUNCH_CASES, REFUSALS, FILES = gen.launch_cases(), gen.refusal_cases(), gen.file_cases()


def test_the_golden_file_holds_exactly_the_cases():
    assert set(GOLDEN["launches"]) == set(LAUNCH_CASES) and len(LAUNCH_CASES) == 3 * 2 * 2 * 2 * 2 * 3 + 2 + 2 + 3
    assert set(GOLDEN["refusals"]) == set(REFUSALS) and set(GOLDEN["files"]) == set(FILES)
    assert all(c["raised"] is None and c["launches"] for c in GOLDEN["launches"].values())


@pytest.mark.parametrize("case", sorted(LAUNCH_CASES))
def test_optimizer_step_launches(case):
    got, want = json.loads(json.dumps(LAUNCH_CASES[case]())), GOLDEN["launches"][case]
    for i, (g, w) in enumerate(zip(got["launches"], want["launches"])):
        assert g == w, f"{case}: launch {i}"
    assert len(got["launches"]) == len(want["launches"]), [sym for sym, _ in got["launches"]]
    assert got == want  # count, state_whole, _grad_is_acc, _acc_norm, the counters and running products


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_come_before_any_launch(case):
    got = json.loads(json.dumps(REFUSALS[case]()))
    assert got["raised"] == "ValueError" and got["launches"] == [] and got["count"] == 0
    assert got == GOLDEN["refusals"][case]


@pytest.mark.parametrize("case", sorted(FILES))
def test_training_state_files_hold_what_they_held(case, tmp_path):
    opt, with_lora = FILES[case]
    path = str(tmp_path / "state.safetensors")
    assert json.loads(json.dumps(gen.file_record(opt, with_lora, path))) == GOLDEN["files"][case]
    assert os.path.exists(path)
    u, t = gen.file_states(opt, with_lora)  # fresh states of the same build read the file back
    for st in (u, t):
        store = checkpoint._stepping_store(st)[0]
        if store is not None:
            store.set_step(0)
    checkpoint.load_training_state(path, u, t)
    saved, _ = gen.file_states(opt, with_lora)
    a, b = checkpoint._stepping_store(saved)[0], checkpoint._stepping_store(u)[0]
    assert b.count == 5 and a.optimizer == b.optimizer == opt
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        for key in f.keys():
            model, name = key.split(".")
            if model == "unet":
                assert torch.equal(f.get_tensor(key), getattr(b, name)), key
    for name in ("adam_step", "adam_prod", "prodigy_step", "prodigy_state"):
        assert (getattr(a, name) is None) == (getattr(b, name) is None)
        assert getattr(a, name) is None or getattr(a, name).tolist() == getattr(b, name).tolist(), name
