"""The task matrix of tests/task_matrix.py without a GPU: its rows cover every pair of values of every two of the eight axes, rows are
dropped only for pairs the code refuses, the builder's keywords reach the task's own store and no other (the stores are built on the CPU,
no kernel runs), the float64 loss the harness differentiates is the masked and the robust loss references' and its operands are
theirs, and the harness's Prodigy reference step is tests/prodigy_reference.py run over the store's pieces in sweep order."""
import itertools
import re

import numpy as np
import pytest
import torch

from oracle import lion8
from tests import masked_loss_reference as mr
from tests import prodigy_reference as PR
from tests import robust_loss_reference as rr
from tests import step_matrix as sm
from tests import task_matrix as tm


# ------------------------------------------------------------------------------------------------ 1. coverage
def test_rows_cover_every_pair_of_values_of_every_two_axes():
    rs = tm.rows()
    assert len(list(itertools.combinations(tm.AXES, 2))) == 28
    base = [r for r in rs if r not in tm.REPLACEMENTS]
    assert len({(r.opt, r.task) for r in base}) == len(base) == 16 - sum(1 for r in tm.all_rows() if tm.refused(r))
    assert [tm.row_for(o, a)[:2] for o in range(4) for a in range(4)] == list(itertools.product(tm.OPTS, tm.TASKS))
    missing = tm.all_pairs() - tm.covered_pairs(rs)
    refused = {e[:4] for e in tm.REFUSED}
    assert missing <= refused, f"pairs no row holds: {sorted(missing - refused)}"
    assert len({tm.row_id(r) for r in rs + [tm.ALL_ON]}) == len(rs) + 1
    assert tm.ALL_ON not in rs and tm.ALL_ON.opt == "prodigy" and tm.ALL_ON[2:] == ("cached", 2, "cosine+ema_warmup", "sdxl", "on", "huber")
    # the first matrix's four forms are kept
    for o in range(4):
        for a in range(4):
            assert tm.row_for(o, a)[2:6] == sm.row_for(o, a)[2:6]


def test_each_binary_axis_varies_along_both_indices_and_no_two_agree():
    """The rule's own reason: every binary axis changes with the optimizer index at a fixed task and with the task index at a fixed
    optimizer, and no two binary axes are equal or opposite over the 16 rows."""
    binary = [ax for ax, vals in tm.AXES.items() if len(vals) == 2]
    assert len(binary) == 6
    table = {ax: [tm.AXES[ax].index(getattr(tm.row_for(o, a), ax)) for o in range(4) for a in range(4)] for ax in binary}
    for ax in binary:
        for fixed in range(4):
            assert len({table[ax][fixed * 4 + a] for a in range(4)}) == 2 and len({table[ax][o * 4 + fixed] for o in range(4)}) == 2, ax
    for x, y in itertools.combinations(binary, 2):
        agree = sum(u == v for u, v in zip(table[x], table[y]))
        assert agree == 8, f"{x} and {y} agree in {agree} of 16 rows"


def test_rows_are_dropped_only_for_refused_pairs():
    assert len(tm.REFUSED) <= 2
    for ax, u, ay, v, msg in tm.REFUSED:
        assert ax in tm.AXES and ay in tm.AXES and ax != ay and u in tm.AXES[ax] and v in tm.AXES[ay]
        re.compile(msg)
    for r in tm.all_rows():
        assert (r in tm.rows()) == (tm.refused(r) is None)
    for r in tm.REPLACEMENTS:
        assert tm.refused(r) is None
    for ax, values in tm.AXES.items():
        for v in values:
            assert any(getattr(r, ax) == v for r in tm.rows()), f"{ax}={v} lost all of its rows"
    # at this commit nothing in train_step or the state builders refuses a pair of the eight axes
    assert tm.REFUSED == () and tm.REPLACEMENTS == () and len(tm.rows()) == 16


# ------------------------------------------------------------------------------------------------ 2. builder wiring
@pytest.mark.parametrize("row", tm.rows() + [tm.ALL_ON], ids=tm.row_id)
def test_builder_keywords_reach_the_tasks_own_store(row):
    """create_lion_optimizer_states on the CPU with a row's keywords: the stepping store is the task's own (the UNet and text stores, the
    token store, the ControlNet's, the IP-Adapter's; pivotal tuning: the UNet adapter's and the token store), every other state is
    frozen with an empty hyper; the stepping store carries the row's optimizer, quantisation and EMA, the documented hyper-parameters
    (Prodigy: no rate, lr 1, the dict's decay, d0 and d_coef, the documented rest) and the cosine / EMA-warmup tables over its own
    base rate; the masks follow the config's exclusion lists."""
    from stable_diffusion_training_amd import training_utils as tu
    case = tm.case_for(row)
    tc = tm.training_config(row, case)
    out = tu.create_lion_optimizer_states(
        sm.models_of(case), adam_to_lion_scale_factor=7, excluded_layer_pattern_from_weight_decay=tc.excluded_layer_pattern_from_weight_decay,
        excluded_layer_from_quantization=tc.excluded_layer_from_quantization, lion_8bit_block_size=tc.quant_block_size,
        quantize_unet_state=tc.quantize_unet_state, quantize_text_encoder_state=tc.quantize_text_encoder_state, with_unet_ema=True,
        with_text_encoder_ema=True, device="cpu", lr_scheduler=tc.lr_scheduler, ema_rate=tc.ema_rate, **tm.state_kwargs(row, case))
    states = (out["unet_state"], out["text_encoder_state"])
    us, ts = states
    assert (us.controlnet is not None) == (row.task == "controlnet") and (us.ip_adapter is not None) == (row.task == "ip_adapter")
    assert (ts.tokens is not None) == tm.with_tokens(row) and (us.adapter is not None) == (row.task == tm.PIVOTAL)
    assert ts.adapter is None and ts.controlnet is None and ts.ip_adapter is None and us.tokens is None
    assert us.store.trainable == ts.store.trainable == (row.task == "inpaint")
    assert (us.config["in_channels"] == 9) == tm.inpainting(row)
    schedules = tm.raise_rates(row, states)  # the stepping names, the frozen rest, the documented hyper-parameters, the schedules
    tm.check_flags(row, tc, states)
    assert tuple(schedules) == tm.STEPPING[row.task]
    for name, st in tm.stepping(states):
        store = st.opt_store
        hp = tm.documented_hyper(row.opt, tm.RATE)
        assert st.hyper == hp
        if row.opt == "prodigy":
            assert "b1" not in hp and hp["lr"] == 1.0 and float(store.prodigy_state[0]) == float(store.prodigy_state[1]) == tm.PRODIGY_OPT["d0"]
            assert store.prodigy["d_coef"] == tm.PRODIGY_OPT["d_coef"] == 4.0 and store.prodigy["growth_rate"] == float("inf") and not store.prodigy["use_bias_correction"]
        if row.sched == "constant":
            assert schedules[name] is None
        else:
            lrs, emas = schedules[name]
            assert lrs.base_lr == hp["lr"]
            assert lrs.rate(0) == 0.0 and lrs.rate(1) == lrs.base_lr and 0 < lrs.rate(5) < lrs.rate(2) < lrs.base_lr
            assert emas.rate(0) == 0.0 and 0 < emas.rate(1) < emas.rate(3) < tm.EMA_RATE
    # the settings of the RIGHT model: built again with the two models' rates, quantisation and EMA switches apart, the token store
    # takes the text encoder's and every store on the UNet state (its own, an adapter's, a ControlNet's, an IP-Adapter's) the UNet's
    apart = tu.create_lion_optimizer_states(
        sm.models_of(case), adam_to_lion_scale_factor=7, u_net_learning_rate=3e-6, text_encoder_learning_rate=5e-6,
        excluded_layer_pattern_from_weight_decay=tc.excluded_layer_pattern_from_weight_decay,
        excluded_layer_from_quantization=tc.excluded_layer_from_quantization, lion_8bit_block_size=tc.quant_block_size,
        quantize_unet_state=True, quantize_text_encoder_state=False, with_unet_ema=True, with_text_encoder_ema=False, device="cpu",
        lr_scheduler=tc.lr_scheduler, ema_rate=tc.ema_rate, **tm.state_kwargs(row, case))
    for name, st in tm.stepping((apart["unet_state"], apart["text_encoder_state"])):
        store, unet = st.opt_store, name == "unet"
        assert st.hyper == tm.documented_hyper(row.opt, 3e-6 if unet else 5e-6), f"{name}: the other model's rate"
        assert (store.ema is not None) == unet, f"{name}: the other model's EMA switch"
        assert any(lf.quantised for lf in store.leaves.values()) == unet, f"{name}: the other model's quantisation switch"
        if row.sched != "constant":
            assert store.schedule[0].base_lr == st.hyper["lr"] and store.schedule[1].ema_rate == tc.ema_rate
    if tm.with_tokens(row):
        tk = ts.tokens
        assert tk.cfg.retract and tk.store.quant_total == 0 and tk.store.grad16 is None
        assert all(not lf.quantised and lf.decayed for lf in tk.store.leaves.values())
        ids = case["batch"]["input_ids"]
        for tower, (V, _) in enumerate(tk.geometry):
            col = ids[:, tower] if ids.dim() == 3 else ids
            assert sorted(set(col[col >= V].tolist())) == [V, V + 1], "the captions do not carry both placeholders"
    if row.mask == "on":
        m, lw = case["batch"]["loss_mask"], case["batch"]["loss_weight"]
        assert tuple(m.shape) == (2 * row.K, 64, 64) and len(set(lw.tolist())) == 2 * row.K
        assert all(0 < float(m[b].mean()) < 1 for b in range(m.shape[0])) and len({float(m[b].mean()) for b in range(m.shape[0])}) == m.shape[0]
        p = tm.pooled_host(m)
        assert bool(((p > tm.MASK_FLOOR) & (p < 1)).any())
        for step in range(tm.STEPS):  # the rolled masks of the later steps pool exactly too
            tm.pooled_host(tm.host_inputs(row, case, step)[0]["loss_mask"])


def test_inputs_differ_every_step():
    row = tm.row_for(0, 2)
    case = tm.case_for(row)
    seen = [tm.host_inputs(row, case, t) for t in range(tm.STEPS)]
    for (b0, r0), (b1, r1) in itertools.combinations(seen, 2):
        assert not torch.equal(b0["pixel_values"], b1["pixel_values"]) and not torch.equal(b0["conditioning_pixel_values"], b1["conditioning_pixel_values"])
        assert all(not torch.equal(r0[k], r1[k]) for k in r0)
    assert all(0 <= int(r["timesteps"].min()) and int(r["timesteps"].max()) < 1000 for _, r in seen)


# ------------------------------------------------------------------------------------------------ 3. the loss restatement
def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1e-300) + 1e-300))


def _loss_and_grad(pred_nhwc, target, e, k, c, loss_type):
    p = torch.from_numpy(np.asarray(pred_nhwc, np.float64)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    t = lambda v: None if v is None else torch.from_numpy(np.asarray(v, np.float64))
    loss = tm.loss64(p, torch.from_numpy(np.asarray(target, np.float64)), t(e), t(k), t(c), loss_type)
    (g,) = torch.autograd.grad(loss, p)
    return float(loss.detach()), g.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", [c for c in mr.LOSS_CASES if c[0] != "over_cap"], ids=lambda c: c[0])
def test_loss64_is_the_masked_loss_reference(case):
    """loss64 with the factors k formed by loss_operands (times the min-SNR weight of the variants that carry one) on
    masked_loss_reference's own cases: the loss and its autograd gradient equal reference() to float64 rounding."""
    for variant in mr.LOSS_VARIANTS:
        inp = mr.loss_inputs(case, variant)
        B, h, w, C = inp["pred"].shape
        batch = {}
        if inp["e"] is not None:
            batch["loss_mask"] = torch.from_numpy(inp["e"])
        if inp["lw"] is not None:
            batch["loss_weight"] = torch.from_numpy(inp["lw"])
        e, k, c = tm.loss_operands(batch, None, None, (h, w), normalize=inp["normalize"])
        assert c is None and (e is None) == (inp["e"] is None)
        if inp["snr"] is not None:
            k = torch.from_numpy(inp["snr"].astype(np.float64)) * (1.0 if k is None else k)
        ref = mr.reference(inp["pred"], inp["target"], inp["e"], inp["snr"], inp["lw"], inp["normalize"])
        assert _close(np.ones(B) if k is None else k.numpy(), ref["k"]), variant[0]
        loss, grad = _loss_and_grad(inp["pred"], inp["target"], None if e is None else e.numpy(), None if k is None else k.numpy(), None, "l2")
        assert _close(loss, ref["loss"]) and _close(grad, ref["grad"], 1e-11), variant[0]


@pytest.mark.parametrize("loss_type", ["huber", "smooth_l1"])
@pytest.mark.parametrize("case", rr.CASES, ids=lambda c: c[0])
def test_loss64_is_the_robust_loss_reference(case, loss_type):
    """The same on robust_loss_reference's random cases (c = 0 with a zero difference, an empty sample under normalisation): the loss
    equals reference(), the autograd gradient equals drho64 times k_b e / count."""
    for variant in rr.VARIANTS:
        inp = rr.random_inputs(case, variant)
        B, h, w, C = inp["pred"].shape
        batch = {}
        if inp["e"] is not None:
            batch["loss_mask"] = torch.from_numpy(inp["e"])
        if inp["lw"] is not None:
            batch["loss_weight"] = torch.from_numpy(inp["lw"])
        e, k, _ = tm.loss_operands(batch, None, None, (h, w), normalize=inp["normalize"])
        if inp["snr"] is not None:
            k = torch.from_numpy(inp["snr"].astype(np.float64)) * (1.0 if k is None else k)
        ref = rr.reference(inp["pred"], inp["target"], inp["c"], rr.TYPES[loss_type], inp["e"], inp["snr"], inp["lw"], inp["normalize"])
        assert _close(np.ones(B) if k is None else k.numpy(), ref["k"]), variant[0]
        loss, grad = _loss_and_grad(inp["pred"], inp["target"], None if e is None else e.numpy(), None if k is None else k.numpy(), inp["c"],
                                    loss_type)
        diff = inp["target"].astype(np.float64).transpose(0, 2, 3, 1) - inp["pred"].astype(np.float64)
        ke = ref["k"][:, None, None] * (np.ones((B, h, w)) if inp["e"] is None else inp["e"].astype(np.float64))
        want = ke[..., None] * rr.drho64(diff, inp["c"].astype(np.float64)[:, None, None, None], rr.TYPES[loss_type]) / (B * C * h * w)
        assert _close(loss, ref["loss"], 1e-11), (variant[0], loss, ref["loss"])
        assert bool(np.all(np.abs(grad - want) <= 1e-11 * np.abs(want) + 1e-18)) and _close(want, ref["grad"]), variant[0]


@pytest.mark.parametrize("prep", [c for c in mr.PREPARE_CASES if c[0] != "f2_over_cap"], ids=lambda c: c[0])
def test_loss_operands_are_the_references(prep):
    """e = effective_mask(pooled_mask(mask, f), floor) (clamped, a NaN counting as 0) and k = sample_factors of its sums and the loss
    weights, for every floor, with and without normalisation."""
    name, f, B, H, W = prep
    mask = mr.seeded_mask((B, H, W), 7, special=True)
    lw = torch.tensor(([0.5, 2.0, 1.0, 1.5, 0.25] * 2)[:B])
    for floor in mr.FLOORS:
        for normalize in (False, True):
            e, k, c = tm.loss_operands(dict(loss_mask=mask, loss_weight=lw), None, None, (H // f, W // f), floor=floor, normalize=normalize)
            want_e = mr.effective_mask(mr.pooled_mask(mask.numpy(), f, np.float64), floor)
            assert c is None and _close(e.numpy(), want_e, 1e-15)
            want_k = mr.sample_factors(B, (H // f) * (W // f), want_e.reshape(B, -1).sum(1), None, lw.numpy(), normalize)
            assert _close(k.numpy(), want_k)
    empty = torch.zeros(2, 8, 8)
    empty[1, 3, 3] = 1.0
    _, k, _ = tm.loss_operands(dict(loss_mask=empty), None, None, (8, 8), normalize=True)
    assert k.tolist() == [0.0, 64.0]


@pytest.mark.parametrize("beta_schedule", ["scaled_linear", "zero_snr_scaled_linear"])
def test_thresholds_are_the_projects_table(beta_schedule):
    from oracle import schedulers as osched
    from stable_diffusion_training_amd import training_utils as tu
    ac = osched.create_state(beta_schedule)["alphas_cumprod"]
    t = torch.tensor([0, 1, 17, 499, 803, 998, 999])
    for schedule in tu.HUBER_SCHEDULES:
        for hc in (tm.HUBER_C, 0.05, 1.0):
            _, _, c = tm.loss_operands({}, t, ac, (8, 8), loss_type="huber", huber_c=hc, huber_schedule=schedule)
            want = tu.huber_threshold_table(ac, hc, schedule)[t.numpy()]
            assert c.dtype == torch.float64 and np.array_equal(c.numpy(), want.astype(np.float64)), (schedule, hc)
    assert tm.loss_operands({}, t, ac, (8, 8))[2] is None


# ------------------------------------------------------------------------------------------------ 4. Prodigy's reference step
SPEC = [("a/kernel", (64, 48)), ("b/kernel", (3, 3, 16, 16)), ("e/embedding", (10, 8)), ("a/bias", (48,))]  # tests/test_gpu_prodigy.py's


def _prodigy_store():
    """A CPU Prodigy store with a leaf in each of the four (quantised x decayed) segments and the matrix's settings."""
    from stable_diffusion_training_amd import params
    st = params.ParamStore(SPEC, device="cpu", quantise=True, quant_excluded=("bias", "embedding"), wd_excluded=("b", "bias"), block_size=16,
                           with_ema=True, optimizer="prodigy", prodigy=dict(d0=tm.PRODIGY_OPT["d0"], d_coef=tm.PRODIGY_OPT["d_coef"]))
    assert [(q, d, b > a) for q, d, a, b in st.segments] == [(True, True, True), (True, False, True), (False, True, True), (False, False, True)]
    g = torch.Generator().manual_seed(11)
    st.load({p: torch.randn(shp, generator=g) * 0.1 for p, shp in SPEC})
    assert st.grad16 is not None and 0 < st.quant_total < st.total
    return st


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("from_acc,scheduled", [(False, False), (True, False), (False, True)], ids=["grad", "acc", "grad-scheduled"])
def test_prodigy_reference_step_is_the_restatement_over_the_pieces_in_sweep_order(from_acc, scheduled):
    """Three carried reference steps (below and above the clip norm, a direction that persists so that d leaves d0) of a CPU Prodigy
    store against tests/prodigy_reference.py called here leaf by leaf - the moments, the apply sweep with each leaf's own decay and the
    EMA on one leaf at a time, from gradients clipped by oracle.lion8.clip_by_global_norm over the whole tree - with the two sums taken
    by ordered_sum over term arrays assembled here, one launch per gradient buffer (or one over the accumulated buffer): another route
    to every number than the harness's flat ranges."""
    from stable_diffusion_training_amd import lr_schedule as L
    st = _prodigy_store()
    hp = tm.documented_hyper("prodigy", tm.RATE)
    schedule = (L.LRSchedule("cosine", hp["lr"], **sm.LR_SCHEDULE), L.EMASchedule("warmup", tm.EMA_RATE)) if scheduled else None
    assert tm.moments_ranges(st, from_acc) == ([(0, st.total)] if from_acc else [(0, st.quant_total), (st.quant_total, st.total)])
    ref = tm.reference_state(st)
    assert ref["st"] == PR.init_state(PR.hyper(**tm.documented_prodigy())) and ref["t"] == 0
    php = PR.hyper(lr=1.0, eps=1e-8, weight_decay=tm.PRODIGY_OPT["weight_decay"], **tm.documented_prodigy())
    mine = {p: dict(p=st.p(p).reshape(-1).numpy().copy(), ema=st.p(p).reshape(-1).numpy().copy(), **PR.zeros(lf.numel)) for p, lf in st.leaves.items()}
    state = PR.init_state(php)
    ds = []
    for step in range(3):
        g_flat = np.zeros(st.total, np.float32)
        rs = np.random.RandomState(10 + step)
        for lf in st.leaves.values():  # the gaps between the leaves stay zero, as zero_grad leaves them
            base = np.random.RandomState(7 + lf.offset).standard_normal(lf.numel)
            g_flat[lf.offset: lf.offset + lf.numel] = ((base + 0.2 * rs.standard_normal(lf.numel)) * (1e-3 if step == 0 else 0.5)).astype(np.float32)
        cur = tm.prodigy_reference_step(st, ref, g_flat, hp, tm.EMA_RATE, schedule, from_acc=from_acc)
        clipped, norm = lion8.clip_by_global_norm({p: g_flat[lf.offset: lf.offset + lf.numel] for p, lf in st.leaves.items()}, 1.0)
        assert (norm < 1.0) == (step == 0)
        kw = dict(lr_tab=schedule[0].table(), ema_tab=schedule[1].table()) if scheduled else {}
        want_cur = PR.select(state, php, ema_rate=tm.EMA_RATE, **kw)
        dot, l1 = np.zeros(st.total), np.zeros(st.total)
        for p, lf in st.leaves.items():
            b, sl = mine[p], slice(lf.offset, lf.offset + lf.numel)
            b["p0"], b["m"], b["v"], b["s"] = PR.moments(b["p"], clipped[p], b["p0"], b["m"], b["v"], b["s"], want_cur, php, dict(dot=0.0, l1=0.0))
            dot[sl] = clipped[p].astype(np.float64) * (b["p0"] - b["p"]).astype(np.float32).astype(np.float64)
            l1[sl] = np.abs(b["s"]).astype(np.float64)
        for a, e in ([(0, st.total)] if from_acc else [(0, st.quant_total), (st.quant_total, st.total)]):
            state["dot"] = PR.ordered_sum(dot[a:e], state["dot"])
            state["l1"] = PR.ordered_sum(l1[a:e], state["l1"])
        PR.finish(state, php, want_cur)
        assert np.array_equal(_bits(cur), _bits(want_cur)), f"step {step}: scalar block"
        assert np.array_equal(_bits(PR.state_block(ref["st"])), _bits(PR.state_block(state))), f"step {step}: state block {ref['st']} != {state}"
        assert ref["t"] == ref["st"]["t"] == step + 1
        for p, lf in st.leaves.items():
            b, sl = mine[p], slice(lf.offset, lf.offset + lf.numel)
            before = b["p"].copy()
            b["p"] = PR.apply(b["p"], b["m"], b["v"], want_cur, hp["wd"] if lf.decayed else 0.0)
            b["ema"] = PR.ema_update(b["ema"], b["p"], want_cur)
            for mk, rk in (("p", "p"), ("ema", "ema"), ("m", "m"), ("v", "v"), ("s", "s"), ("p0", "p0")):
                assert np.array_equal(_bits(b[mk]), _bits(ref[rk][sl])), f"step {step}: {p} {rk}"
            assert not np.array_equal(b["p"], before) or (scheduled and step == 0), f"step {step}: {p} never moved"
        ds.append(state["d"])
    if scheduled:  # the warm-up's first step has lr_t = 0: d stays
        assert ds[0] == php["d0"]
    assert ds[-1] > php["d0"], ds
