"""The option matrix of tests/step_matrix.py without a GPU: its rows cover every pair of values of every two axes, rows are dropped
only for pairs the code refuses, the builder's keywords reach the stepping stores (hyper-parameters, masks, schedules - the stores are
built on the CPU, no kernel runs), and the harness's reference step is the project's restatements run leaf by leaf."""
import itertools
import re

import numpy as np
import pytest
import torch

from oracle import lion8
from tests import adamw_reference as AR
from tests import step_matrix as sm


def test_rows_cover_every_pair_of_values_of_every_two_axes():
    rs = sm.rows()
    assert len(list(itertools.combinations(sm.AXES, 2))) == 15
    assert len({(r.opt, r.adapter) for r in rs}) == len(rs) == 16 - sum(1 for r in sm.all_rows() if sm.refused(r))
    assert [sm.row_for(o, a)[:2] for o in range(4) for a in range(4)] == list(itertools.product(sm.OPTS, sm.ADAPTERS))
    missing = sm.all_pairs() - sm.covered_pairs(rs)
    refused = {e[:4] for e in sm.REFUSED}
    assert missing <= refused, f"pairs no row holds: {sorted(missing - refused)}"
    assert len({sm.row_id(r) for r in rs}) == len(rs)
    assert sm.row_id(sm.row_for(2, 3)).startswith("adamw8-dora-") and sm.ALL_ON not in rs


def test_rows_are_dropped_only_for_refused_pairs():
    assert len(sm.REFUSED) <= 2
    for e in sm.REFUSED:
        ax, u, ay, v, msg = e
        assert ax in sm.AXES and ay in sm.AXES and ax != ay and u in sm.AXES[ax] and v in sm.AXES[ay]
        re.compile(msg)
    for r in sm.all_rows():
        assert (r in sm.rows()) == (sm.refused(r) is None)
    for ax, values in sm.AXES.items():
        for v in values:
            assert any(getattr(r, ax) == v for r in sm.rows()), f"{ax}={v} lost all of its rows"
    # at this commit nothing in train_step or create_lion_optimizer_states refuses a pair of the six single-process axes
    assert sm.REFUSED == () and len(sm.rows()) == 16


@pytest.mark.parametrize("row", sm.rows() + [sm.ALL_ON], ids=sm.row_id)
def test_builder_keywords_reach_the_stepping_stores(row):
    """create_lion_optimizer_states on the CPU with a row's keywords: the stepping stores are the adapters' (or the weight stores), carry
    the row's optimizer, quantisation and EMA, the documented hyper-parameters, the cosine / EMA-warmup schedule over the store's own
    rate, and the masks of the config's exclusion lists (DoRA: lora_m with fp32 moments and no decay)."""
    from stable_diffusion_training_amd import training_utils as tu
    case = sm.case_for(row)
    tc = sm.training_config(row, case)
    out = tu.create_lion_optimizer_states(
        sm.models_of(case), adam_to_lion_scale_factor=7, excluded_layer_pattern_from_weight_decay=tc.excluded_layer_pattern_from_weight_decay,
        excluded_layer_from_quantization=tc.excluded_layer_from_quantization, lion_8bit_block_size=tc.quant_block_size,
        quantize_unet_state=tc.quantize_unet_state, quantize_text_encoder_state=tc.quantize_text_encoder_state, with_unet_ema=True,
        with_text_encoder_ema=True, device="cpu", lr_scheduler=tc.lr_scheduler, ema_rate=tc.ema_rate, **sm.state_kwargs(row))
    states = (out["unet_state"], out["text_encoder_state"])
    for name, st in zip(("unet", "text"), states):
        store = st.opt_store
        assert (st.adapter is not None) == (row.adapter != "none" and not (name == "text" and row.adapter == "lora_te_frozen"))
        assert st.store.trainable == (row.adapter == "none")
        if store is None:
            assert name == "text" and row.adapter == "lora_te_frozen"
            continue
        assert store is (st.adapter.store if st.adapter is not None else st.store)
        assert store.optimizer == ("adamw" if row.opt.startswith("adamw") else "lion") and store.ema is not None
        assert (store.quant_total > 0) == row.opt.endswith("8")
        assert (store.codes2 is not None) == row.opt.startswith("adamw")
    schedules = sm.raise_rates(row, states)
    sm.check_flags(row, tc, states)
    for name, st in sm.stepping(states):
        if row.sched == "constant":
            assert schedules[name] is None
        else:
            lrs, emas = schedules[name]
            assert lrs.base_lr == st.hyper["lr"] == sm.documented_hyper(row.opt, sm.RATE)["lr"]
            assert lrs.rate(0) == 0.0 and lrs.rate(1) == lrs.base_lr and 0 < lrs.rate(5) < lrs.rate(2) < lrs.base_lr
            assert emas.rate(0) == 0.0 and 0 < emas.rate(1) < emas.rate(3) < sm.EMA_RATE


# ------------------------------------------------------------------------------------------------ the reference step
def _adapter_store(optimizer, dora):
    """A CPU adapter store on a two-kernel base with a leaf in each (quantised x decayed) segment."""
    from stable_diffusion_training_amd import lora, params
    spec = [("blk/to_q/kernel", (32, 48)), ("blk/to_q/bias", (48,)), ("blk/to_out_0/kernel", (48, 32)), ("blk/to_out_0/bias", (32,))]
    base = params.ParamStore(spec, device="cpu", trainable=False)
    g = torch.Generator().manual_seed(3)
    base.load({p: torch.randn(shp, generator=g) * 0.2 for p, shp in spec})
    okw = dict(optimizer="adamw", adam_betas=(0.9, 0.999)) if optimizer == "adamw" else {}
    ad = lora.attach(base, lora.LoraConfig(8, 4.0, seed=5, dora=dora), quantise=True, quant_excluded=("bias", "to_out_0"),
                     wd_excluded=("bias", "lora_b"), block_size=16, with_ema=True, **okw)
    st = ad.store
    tree = {p: torch.randn(lf.shape, generator=g) * 0.1 for p, lf in st.leaves.items()}
    st.load(tree)
    want = {(True, True), (True, False), (False, True), (False, False)}
    assert {(lf.quantised, lf.decayed) for lf in st.leaves.values()} == want
    assert dora == any(p.endswith("lora_m") for p in st.leaves)
    return st


@pytest.mark.parametrize("optimizer,dora,scheduled", [("lion", True, False), ("adamw", True, True), ("adamw", False, False), ("lion", False, True)])
def test_reference_step_is_the_restatements_run_leaf_by_leaf(optimizer, dora, scheduled):
    """Three carried reference steps (below and above the clip norm) of a CPU adapter store against adamw_reference.step8 / step32 /
    ema_update with select_scalars, and oracle.lion8.lion_step / ema_update, called here leaf by leaf on gradients clipped by
    oracle.lion8.clip_by_global_norm over the whole tree - another route to the clip than the harness's."""
    from stable_diffusion_training_amd import lr_schedule as L
    st = _adapter_store(optimizer, dora)
    hp = sm.documented_hyper("adamw8" if optimizer == "adamw" else "lion8", sm.RATE)
    schedule = (L.LRSchedule("cosine", hp["lr"], **sm.LR_SCHEDULE), L.EMASchedule("warmup", sm.EMA_RATE)) if scheduled else None
    ref = sm.reference_state(st)
    assert ref["t"] == 0 and ref["prods"] == ((1.0, 1.0) if optimizer == "adamw" else None)
    mine = dict(p={k: v.copy() for k, v in ref["p"].items()}, ema={k: v.copy() for k, v in ref["ema"].items()}, m=dict(ref["m"]))
    t, prods = 0, (1.0, 1.0)
    for step in range(3):
        rs = np.random.RandomState(10 + step)
        g_flat = np.zeros(st.total, np.float32)
        for lf in st.leaves.values():
            g_flat[lf.offset: lf.offset + lf.numel] = rs.standard_normal(lf.numel).astype(np.float32) * (1e-3 if step == 0 else 0.5)
        cur = sm.reference_store_step(st, ref, g_flat, hp, sm.EMA_RATE, schedule)
        clipped, norm = lion8.clip_by_global_norm({p: g_flat[lf.offset: lf.offset + lf.numel] for p, lf in st.leaves.items()}, 1.0)
        assert (norm < 1.0) == (step == 0)
        if optimizer == "adamw":
            kw = dict(lr=hp["lr"], ema_rate=sm.EMA_RATE) if schedule is None else dict(lr_tab=schedule[0].table(), ema_tab=schedule[1].table())
            want_cur, t, prods = AR.select_scalars(t, prods, 0.9, 0.999, **kw)
            assert np.array_equal(cur.view(np.int32), want_cur.view(np.int32)) and (ref["t"], ref["prods"]) == (t, prods)
            if scheduled:
                assert want_cur[0] == np.float32(-schedule[0].rate(step)) and want_cur[1] == np.float32(schedule[1].rate(step))
        else:
            assert cur is None and ref["t"] == step + 1
        for p, lf in st.leaves.items():
            wd = (1e-2 if optimizer == "adamw" else 0.07) if lf.decayed else 0.0
            if optimizer == "adamw":
                kw = dict(wd=wd, b1=0.9, b2=0.999, eps=1e-8, max_norm=None)
                if lf.quantised:
                    mine["p"][p], mine["m"][p] = AR.step8(mine["p"][p], clipped[p], mine["m"][p], want_cur, bs=16, **kw)
                else:
                    mine["p"][p], m, v = AR.step32(mine["p"][p], clipped[p], *mine["m"][p], want_cur, **kw)
                    mine["m"][p] = (m, v)
                mine["ema"][p] = AR.ema_update(mine["ema"][p], mine["p"][p], want_cur)
            else:
                lr, r = (hp["lr"], sm.EMA_RATE) if schedule is None else (schedule[0].rate(step), schedule[1].rate(step))
                newp, state, _ = lion8.lion_step({p: mine["p"][p]}, {p: clipped[p]}, {"count": 0, "mu": {p: mine["m"][p]}}, lr=lr, wd=0.07,
                                                 b1=0.9, b2=0.99, block_size=16, decay_mask={p: lf.decayed}, clip=None)
                mine["p"][p], mine["m"][p] = newp[p], state["mu"][p]
                mine["ema"][p] = lion8.ema_update({p: mine["ema"][p]}, newp, r)[p]
            bits = lambda a: np.ascontiguousarray(a).view(np.int8 if a.dtype == np.int8 else np.int32)
            assert np.array_equal(bits(ref["p"][p]), bits(mine["p"][p])), f"step {step}: {p} master"
            assert np.array_equal(bits(ref["ema"][p]), bits(mine["ema"][p])), f"step {step}: {p} ema"
            ms, mm = ref["m"][p], mine["m"][p]
            for a, b in zip(ms if isinstance(ms, tuple) else (ms,), mm if isinstance(mm, tuple) else (mm,)):
                assert np.array_equal(bits(a), bits(b)), f"step {step}: {p} moments"
            assert not np.array_equal(ref["p"][p], st.p(p).reshape(-1).numpy()) or (scheduled and step == 0), f"step {step}: {p} never moved"
    # a magnitude moved without decay and kept fp32 moments
    if dora:
        p = next(q for q in st.leaves if q.endswith("lora_m"))
        assert not isinstance(ref["m"][p], tuple) or (optimizer == "adamw" and len(ref["m"][p]) == 2 and ref["m"][p][0].dtype == np.float32)
