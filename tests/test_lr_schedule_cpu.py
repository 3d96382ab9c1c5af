"""Learning-rate and EMA-rate schedules (stable_diffusion_training_amd/lr_schedule.py), host side: the float64 rates against
transformers' get_scheduler driving a torch LambdaLR, the EMA warmup against a restatement of diffusers EMAModel.get_decay, the float32
tables the device reads, and the resolution from the training config."""
import math

import numpy as np
import pytest
import torch

from stable_diffusion_training_amd import lr_schedule as L

BASE = 1e-6 / 7  # the reference's effective rate (on_device_model_training_state's quirk)


def _transformers_rates(name, base, n_steps, **kw):
    """param_groups[0]["lr"] read before each scheduler.step(), for steps 0 .. n_steps - 1."""
    from transformers import get_scheduler
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    extra = {k: kw.pop(k) for k in ("num_cycles", "power", "lr_end") if k in kw}
    sch = get_scheduler(name, opt, scheduler_specific_kwargs=extra or None, **kw)
    out = []
    for _ in range(n_steps):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return np.array(out, dtype=np.float64)


CASES = []
for _w in (0, 3):
    CASES.append(("constant", {}))
    CASES.append(("constant_with_warmup", dict(num_warmup_steps=_w)))
    CASES.append(("linear", dict(num_warmup_steps=_w, num_training_steps=17)))
    for _c in (1, 3):
        CASES.append(("cosine", dict(num_warmup_steps=_w, num_training_steps=23, num_cycles=_c)))
        CASES.append(("cosine_with_restarts", dict(num_warmup_steps=_w, num_training_steps=23, num_cycles=_c)))
    for _pw in (1.0, 2.0):
        CASES.append(("polynomial", dict(num_warmup_steps=_w, num_training_steps=19, power=_pw, lr_end=BASE / 10)))
CASES = list({(n, tuple(sorted(k.items()))): (n, k) for n, k in CASES}.values())


@pytest.mark.parametrize("name,kw", CASES, ids=[f"{n}-{'-'.join(f'{a}{b}' for a, b in sorted(k.items()))}" for n, k in CASES])
def test_lr_rates_equal_transformers_bit_for_bit(name, kw):
    sch = L.LRSchedule(name, BASE, **kw)
    n = kw.get("num_training_steps", kw.get("num_warmup_steps", 0) + 4)
    ref = _transformers_rates(name, BASE, n, **dict(kw))
    got = np.array([sch.rate(t) for t in range(n)], dtype=np.float64)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), np.nonzero(got != ref)
    # past the last planned step the last value holds (transformers would keep evaluating its formula)
    last = sch.rate(sch.table_len() - 1)
    for t in (sch.table_len(), sch.table_len() + 1, 10 * n + 7):
        assert sch.rate(t) == last
    # the device table: float32 -lr_t, exactly as the by-value launchers round (float)(-lr)
    tab = sch.table()
    assert tab.dtype == np.float32 and len(tab) == sch.table_len() >= 1
    want = np.array([np.float32(-sch.rate(t)) for t in range(len(tab))], dtype=np.float32)
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32))


def test_lr_table_lengths():
    assert len(L.LRSchedule("constant", BASE).table()) == 1
    assert len(L.LRSchedule("constant_with_warmup", BASE, num_warmup_steps=5).table()) == 6
    assert len(L.LRSchedule("cosine", BASE, num_warmup_steps=2, num_training_steps=6).table()) == 6
    cw = L.LRSchedule("cosine", BASE, num_warmup_steps=2, num_training_steps=6)
    assert cw.rate(0) == 0.0 and cw.rate(2) == BASE  # update of size 0 on the first step, the full rate after the warmup


def _get_decay(optimization_step, *, decay, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3, min_decay=0.0):
    """diffusers.training_utils.EMAModel.get_decay (diffusers 0.2x), restated: the rate EMAModel.step uses after incrementing
    optimization_step."""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur_decay_value = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur_decay_value = (1 + step) / (10 + step)
    cur_decay_value = min(cur_decay_value, decay)
    cur_decay_value = max(cur_decay_value, min_decay)
    return cur_decay_value


EMA_CASES = [
    dict(ema_rate=0.999),
    dict(ema_rate=0.999, use_ema_warmup=True),
    dict(ema_rate=0.99, use_ema_warmup=True, inv_gamma=3.0, power=0.75),
    dict(ema_rate=0.9995, update_after_step=5),
    dict(ema_rate=0.995, min_decay=0.4),
    dict(ema_rate=0.995, update_after_step=2, min_decay=0.3, use_ema_warmup=True),
    dict(ema_rate=0.6),  # the cap bites at step 4
]


@pytest.mark.parametrize("kw", EMA_CASES)
def test_ema_warmup_equals_diffusers_get_decay(kw):
    kw = dict(kw)
    rate = kw.pop("ema_rate")
    sch = L.EMASchedule("warmup", rate, **kw)
    tab = sch.table()
    n = len(tab)
    assert tab.shape == (n, 2) and tab.dtype == np.float32
    for t in list(range(min(n, 3000))) + [n - 2, n - 1, n, n + 1, 3 * n + 11]:
        if t < 0:
            continue
        want = _get_decay(t + 1, decay=rate, **kw)  # EMAModel.step increments optimization_step first
        assert sch.rate(t) == want, (t, sch.rate(t), want)
        row = tab[min(t, n - 1)]
        assert row[0].view(np.uint32) == np.float32(want).view(np.uint32)
        assert row[1].view(np.uint32) == np.float32(1.0 - want).view(np.uint32)
    assert sch.rate(0) == 0.0 and tab[0, 0] == 0.0 and tab[0, 1] == 1.0  # the EMA starts as a copy of the parameters
    # the table ends where the value stops changing: the cap (or the floor) holds from its last entry on
    assert _get_decay(n, decay=rate, **kw) != _get_decay(n - 1, decay=rate, **kw) or n == 1
    assert all(_get_decay(n + k, decay=rate, **kw) == _get_decay(n, decay=rate, **kw) for k in (1, 2, 100, 10000))


def test_ema_table_length_at_the_reference_rate():
    tab = L.EMASchedule("warmup", 0.99998).table()
    assert 440_000 < len(tab) < 460_000  # (1 + s) / (10 + s) reaches 0.99998 at s ~ 9 / 2e-5
    assert tab[-1, 0] == np.float32(0.99998) and tab[-1, 1] == np.float32(1.0 - 0.99998)


def test_constant_ema_is_one_entry():
    tab = L.EMASchedule("constant", 0.99998).table()
    assert tab.shape == (1, 2) and tab[0, 0] == np.float32(0.99998) and tab[0, 1] == np.float32(1.0 - 0.99998)


def test_resolution_from_the_config():
    assert L.resolve("constant", BASE, 0.99998) is None
    assert L.resolve("constant", BASE, 0.99998, lr_schedule=dict(num_warmup_steps=3)) is None
    lr, ema = L.resolve("constant", BASE, 0.999, ema_schedule=dict(kind="warmup"))
    assert lr.table_len() == 1 and ema.kind == "warmup"
    lr, ema = L.resolve("cosine", BASE, 0.999, lr_schedule=dict(num_warmup_steps=2, num_training_steps=6))
    assert lr.name == "cosine" and lr.base_lr == BASE and ema.kind == "constant" and ema.table().shape == (1, 2)
    with pytest.raises(ValueError, match="num_training_steps"):
        L.resolve("cosine", BASE, 0.999)
    with pytest.raises(ValueError, match="num_training_steps"):
        L.resolve("linear", BASE, 0.999, lr_schedule=dict(num_warmup_steps=2))
    with pytest.raises(ValueError, match="num_warmup_steps"):
        L.resolve("constant_with_warmup", BASE, 0.999)
    with pytest.raises(ValueError, match="unknown"):
        L.resolve("exponential", BASE, 0.999, lr_schedule=dict(num_training_steps=6))
    with pytest.raises(ValueError, match="negative"):
        L.resolve("cosine", BASE, 0.999, lr_schedule=dict(num_warmup_steps=-1, num_training_steps=6))
    with pytest.raises(ValueError, match="negative"):
        L.resolve("linear", BASE, 0.999, lr_schedule=dict(num_training_steps=-6))
    with pytest.raises(ValueError, match="lr_end"):
        L.resolve("polynomial", BASE, 0.999, lr_schedule=dict(num_training_steps=6, lr_end=2 * BASE))
    with pytest.raises(ValueError, match="unknown EMA"):
        L.resolve("constant", BASE, 0.999, ema_schedule=dict(kind="karras"))


def test_config_names_a_schedule_without_counts_raises_before_any_allocation():
    """create_lion_optimizer_states resolves the schedule before it builds a store: no device, no weights needed to get the error."""
    from stable_diffusion_training_amd import training_utils as tu
    from oracle import nets as onets
    cfg = onets.unet_config("tiny")
    models = {"unet": {"unet_params": None, "config": cfg}}
    with pytest.raises(ValueError, match="num_training_steps"):
        tu.create_lion_optimizer_states(models, train_text_encoder=False, lr_scheduler="cosine", device="cpu")


def test_store_schedule_install_and_step_on_cpu():
    """set_schedule / set_step bookkeeping (CPU store: no kernel runs)."""
    from stable_diffusion_training_amd.params import ParamStore
    st = ParamStore([("a/kernel", (4, 8)), ("a/bias", (8,))], device="cpu", quantise=False)
    lr = L.LRSchedule("cosine", BASE, num_warmup_steps=2, num_training_steps=6)
    st.set_step(3)
    st.set_schedule(lr=lr, ema=L.EMASchedule("warmup", 0.999))
    assert int(st._sched["step"][0]) == 3 and st.count == 3
    lr_ptr, ema_ptr = st._sched["lr_tab"].data_ptr(), st._sched["ema_tab"].data_ptr()
    # a shorter schedule is rewritten in place, padded with its last entry (what the clamped index would read)
    st.set_schedule(lr=L.LRSchedule("linear", BASE, num_training_steps=4), ema=L.EMASchedule("constant", 0.999))
    assert st._sched["lr_tab"].data_ptr() == lr_ptr and st._sched["ema_tab"].data_ptr() == ema_ptr
    tab = st._sched["lr_tab"].numpy()
    assert len(tab) == 6 and tab[4] == tab[3] == tab[5] == np.float32(-BASE / 4)
    st.set_step(5)
    assert int(st._sched["step"][0]) == 5 and st.count == 5
    with pytest.raises(ValueError):
        st.set_step(-1)
    # once a graph has captured the store's step, a schedule that does not fit is refused
    st._captured = True
    with pytest.raises(RuntimeError, match="capture"):
        st.set_schedule(lr=L.LRSchedule("cosine", BASE, num_training_steps=60), ema=L.EMASchedule("constant", 0.999))
    st.set_schedule(lr=lr, ema=L.EMASchedule("constant", 0.999))  # fits: fine


def test_facade_accepts_a_schedule_callable():
    """lion_quant.lion_8bit no longer refuses optax's ScalarOrSchedule (the GPU test runs it)."""
    from stable_diffusion_training_amd import lion_quant
    tx = lion_quant.lion_8bit(lambda count: 1e-3 * (count + 1))
    assert callable(tx.init) and callable(tx.update)
    assert math.isclose(L.LRSchedule("linear", 1.0, num_training_steps=4).rate(1), 0.75)
