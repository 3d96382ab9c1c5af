"""Every refusal of the training layer that needs no device, by exception type and full message, against tests/golden/step_refusals.json
(tests/golden/make_step_refusals.py: the cases and how each is provoked).  The golden file pins the ValueErrors of
create_lion_optimizer_states for lora=, new_tokens=, controlnet= and ip_adapter=, the refusals at the top of train_step, every branch of
the five batch checkers, a captured step's key guards, and - the both/ cases - which message wins when an input breaks two rules."""
import json

import pytest

from tests.golden import make_step_refusals as gen

with open(gen.OUT) as _f:
    GOLDEN = json.load(_f)
CASES = gen.all_cases()


def test_the_golden_file_holds_exactly_the_cases():
    assert set(GOLDEN["cases"]) == set(CASES)
    assert all(v is not None and v[0] == "ValueError" and v[1] for v in GOLDEN["cases"].values())
    assert sum(k.startswith("both/") for k in CASES) >= 6
    for group in ("builder/lora/", "builder/new_tokens/", "builder/controlnet/", "builder/ip_adapter/", "step/tokens/", "step/lora/",
                  "step/controlnet/", "step/ip_adapter/", "batch/loss/", "batch/inpaint/", "batch/control/", "batch/ip/", "batch/image/",
                  "graph/"):
        assert any(k.startswith(group) for k in CASES), group


def test_the_batch_key_constants():
    assert gen.constants() == GOLDEN["constants"]
    assert GOLDEN["constants"] == dict(LOSS_KEYS=["loss_mask", "loss_weight"], INPAINT_KEYS=["inpaint_mask"],
                                       CONTROL_KEYS=["conditioning_pixel_values"], IP_KEYS=["image_embeds"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case):
    assert gen.record(CASES[case]) == GOLDEN["cases"][case]
