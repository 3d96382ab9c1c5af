"""train_step where the features added after the first option matrix meet, on a real MI355X: the pairwise matrix of
tests/task_matrix.py (optimizer incl. Prodigy x task x front x micro-batches x schedule x conditioning x loss mask x loss type, 16
rows) and one row with everything on (Prodigy, pivotal tuning on the inpainting UNet), at the tiny configuration (image 64, B = 2 * K,
77 tokens), four steps per run with different inputs every step.

(a) path equivalences, bit for bit on every buffer the step writes (Prodigy's m, v, s, p0, state block, counter and scalar block, the
    loss per sample, a token store's retracted rows): the graphed shape table - which then refuses a batch without the row's keys -
    save / load (and the adapter and token files) after step 2 with two more steps, cached latents against pixels, two identical
    micro-batches against the plain step;
(b) every optimizer step against the project's restatements (oracle/lion8.py, tests/adamw_reference.py, tests/prodigy_reference.py
    over the store's pieces in sweep order) applied to a host copy of the previous state, from the gradient the sweep read, with the
    DOCUMENTED hyper-parameters and the schedule's tables;
(c) the loss and the gradients of step 1 over the whole batch against a CPU reference of the task under autograd with the float64
    loss restatement task_matrix.loss64, with the gates of the single-feature tests.
The checks of a row are separate tests over one shared eager run of the row."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import step_matrix as sm
from tests import task_matrix as tm
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
ROWS = tm.rows()
ROWS_AB = ROWS + [tm.ALL_ON]


@dataclasses.dataclass
class _Eager:
    trace: list
    restatement_error: object
    steps_checked: int
    grads: dict        # after step 0: {"unet" / "text": (exported gradient tree, gradient norm)}
    loss0: float
    built: object
    files: dict        # written after step 2: training state, adapter / token files, the mirror merged from the saved leaves
    initial: dict      # {"unet" / "text": the stepping store's master before the first step}


_RUNS = {}


def _eager(row, dev, tmp_path_factory):
    """The row's uninterrupted eager run, once: four steps, each followed by the restatement check (b) - its first failure is kept for
    test_optimizer_steps_equal_the_restatement, the run goes on - with the gradients of step 0 set aside for (c) and the files of the
    resume test written after step 2.  A run that failed is remembered: every check of the row reports it, none repeats it."""
    if row in _RUNS:
        if isinstance(_RUNS[row], BaseException):
            raise _RUNS[row]
        return _RUNS[row]
    try:
        _RUNS[row] = _run_eager(row, dev, tmp_path_factory)
    except Exception as e:
        _RUNS[row] = e
        raise
    return _RUNS[row]


def _run_eager(row, dev, tmp_path_factory):
    from stable_diffusion_training_amd import training_utils as tu
    case = tm.case_for(row)
    tc, states = tm.build(row, case, dev)
    built = tm.build.last
    refs = {name: tm.reference_state(st.opt_store) for name, st in tm.stepping(states)}
    frozen = tm.frozen_record(states)
    tmp = tmp_path_factory.mktemp("resume")
    rec = _Eager([], None, 0, {}, 0.0, built, dict(state=str(tmp / "state.safetensors"), adapter=None, tokens=None, mirror=None),
                 {name: st.opt_store.master.clone() for name, st in tm.stepping(states)})

    def after_step(t, states, out):
        torch.cuda.synchronize()
        if t == 0:
            rec.loss0 = float(out[4]["loss"].item())
            for name, st in tm.stepping(states):
                rec.grads[name] = (st.opt_store.export("grad"), st.opt_store.grad_norm())
        if rec.restatement_error is None:
            try:
                for name, st in tm.stepping(states):
                    g = sm.gradient_seen(st.opt_store, row.K)
                    tm.restate_and_check(row, st, refs[name], g, built.schedules[name], f"{tm.row_id(row)} step {t}: {name}")
                rec.steps_checked = t + 1
            except AssertionError as e:
                rec.restatement_error = e
        if t == 1:
            tu.save_training_state(rec.files["state"], states[0], states[1])
            if states[0].adapter is not None:
                rec.files["adapter"] = str(tmp / "unet_adapter.npz")
                states[0].adapter.save(rec.files["adapter"])
                states[0].adapter.merge("master")  # the mirror of the saved leaves (the next step's own merge writes the same)
                torch.cuda.synchronize()
                rec.files["mirror"] = states[0].store.w.clone()
            if states[1].tokens is not None:
                rec.files["tokens"] = str(tmp / "tokens.npz")
                states[1].tokens.save(rec.files["tokens"])

    rec.trace = tm.run_eager(row, case, dev, states, after_step=after_step)
    assert all(st.opt_store.count == tm.STEPS for _, st in tm.stepping(states))
    losses = [float(s["loss"]) for s in rec.trace]
    assert len(set(losses)) == tm.STEPS and all(np.isfinite(v) and v > 0 for v in losses), losses
    for name, st in tm.stepping(states):
        first, last = rec.trace[0], rec.trace[-1]
        assert not torch.equal(first[f"{name}.master"], last[f"{name}.master"]), f"{name}: the masters never moved"
        assert bool(torch.isfinite(last[f"{name}.master"]).all())
        if row.sched != "constant":  # step 0 ran at rate 0 (a retracting token store: the EMA, set to the sweep's value, shows it)
            retracts = st.tokens is not None and st.opt_store is st.tokens.store and st.tokens.cfg.retract
            assert torch.equal(first[f"{name}.ema" if retracts else f"{name}.master"], rec.initial[name]), f"{name}: step 0 moved the parameters"
            assert not torch.equal(rec.trace[1][f"{name}.master"], first[f"{name}.master"]), f"{name}: step 1 ran at rate 0 too"
        else:
            assert not torch.equal(first[f"{name}.master"], rec.initial[name]), f"{name}: step 0 did not move the parameters"
        if row.opt == "prodigy":
            d = [float(s[f"{name}.prodigy_state"][0]) for s in rec.trace]
            print(f"[{tm.row_id(row)}] {name}: d after each step {d}")
            assert d[-1] > tm.PRODIGY_OPT["d0"], f"{name}: d never left d0: {d}"
    tm.assert_frozen_unchanged(frozen, states)
    return rec


# ------------------------------------------------------------------------------------------------ (a) path equivalences
def _untouched(states):
    stores = [st.opt_store for _, st in tm.stepping(states)]
    before = [(s, s.count, s.master.clone()) for s in stores]

    def check():
        torch.cuda.synchronize()
        for s, count, master in before:
            assert s.count == count and torch.equal(s.master, master), "a refused step changed a store"
    return check


@pytest.mark.parametrize("row", ROWS_AB, ids=tm.row_id)
def test_graphed_table_equals_the_eager_steps(dev, tmp_path_factory, row):
    """Four steps through dp_compile_all_unique_resolution(use_graph=True, micro_batches=K, step_overrides=the row's loss options):
    two eager calls, the capture, then replays - every snapshot key of every step equals the eager run's.  The captured step then
    refuses a batch that drops the loss keys, and one that drops the task's own key, each before anything is written."""
    eager = _eager(row, dev, tmp_path_factory)
    case = tm.case_for(row)
    tc, states = tm.build(row, case, dev)
    fn, trace, (batch, rand, gen, vae) = tm.run_graphed(row, case, dev, tc, states)
    assert fn.graph is not None and fn.calls == 2, "the last calls were to replay the captured step"
    for name, st in tm.stepping(states):
        assert st.opt_store.count == tm.STEPS and st.step == tm.STEPS, f"{name}: host step count {st.opt_store.count} after four calls"
    assert states[0].store.count == 0 or row.task == "inpaint"
    for t, (a, b) in enumerate(zip(eager.trace, trace)):
        sm.assert_snapshots_equal(b, a, f"step {t}, graphed table against eager")
    us, ts, ue, te, _, sc, _ = states
    dropped = []
    if row.mask == "on":
        dropped.append((("loss_mask", "loss_weight"), r"captured with \['loss_mask', 'loss_weight'\]"))
    dropped += [((k,), f"captured with {k}") for k in tm.BATCH_KEYS[row.task]]
    check = _untouched(states)
    for keys, message in dropped:
        assert all(k in batch for k in keys)
        with pytest.raises(ValueError, match=message):
            fn(us, ts, ue, te, {k: v for k, v in batch.items() if k not in keys}, gen, vae, sc, rand=rand)
        check()


@pytest.mark.parametrize("row", ROWS_AB, ids=tm.row_id)
def test_resumed_steps_equal_the_uninterrupted_run(dev, tmp_path_factory, row):
    """save_training_state after step 2 (and the adapter's and the tokens' own files), fresh states with OTHER LoRA factors and token
    rows, load, steps 3 and 4: the schedule's position, AdamW's counter and products, Prodigy's d, d_max, numer, p0 and s, the token
    rows and the re-merged mirror continue the uninterrupted run."""
    from stable_diffusion_training_amd import training_utils as tu
    eager = _eager(row, dev, tmp_path_factory)
    case = tm.case_for(row)
    tc, states = tm.build(row, case, dev, seed=61)
    saved = eager.trace[1]
    for name, st in tm.stepping(states):
        assert st.opt_store.count == 0
    if states[0].adapter is not None:
        assert not torch.equal(states[0].opt_store.master, saved["unet.master"])
        states[0].adapter.load(eager.files["adapter"])  # (loads and merges)
        torch.cuda.synchronize()
        assert torch.equal(states[0].store.w, eager.files["mirror"]), "the adapter file does not restore the merged mirror"
    if states[1].tokens is not None:
        tk = states[1].tokens
        assert not torch.equal(tk.store.master, saved["text.master"])
        tk.load(eager.files["tokens"])
        for q, lf in tk.store.leaves.items():
            assert torch.equal(tk.store.p(q).reshape(-1), saved["text.master"][lf.offset: lf.offset + lf.numel]), q
    tu.load_training_state(eager.files["state"], states[0], states[1])
    for name, st in tm.stepping(states):
        store = st.opt_store
        assert st.step == 2 and store.count == 2
        if store.optimizer == "adamw":
            assert int(store.adam_step.item()) == 2 and torch.equal(store.adam_prod, saved[f"{name}.adam_prod"])
        elif store.optimizer == "prodigy":
            assert int(store.prodigy_step.item()) == 2
            for b in ("prodigy_p0", "prodigy_s", "mom", "mom2"):
                assert torch.equal(getattr(store, b), saved[f"{name}.{b}"]), f"{name}: {b} is not the saved one"
            assert torch.equal(store.prodigy_state[:5], saved[f"{name}.prodigy_state"][:5]), "d, d_max, numer or the rebuilt products"
        elif row.sched != "constant":
            assert int(store._sched["step"].item()) == 2
    resumed = tm.run_eager(row, case, dev, states, steps=2, first=2)
    for t in (2, 3):
        sm.assert_snapshots_equal(resumed[t - 2], eager.trace[t], f"step {t + 1} after save / load against the uninterrupted run")


@pytest.mark.parametrize("row", [r for r in ROWS_AB if r.front == "cached"], ids=tm.row_id)
def test_cached_front_equals_the_pixel_front(dev, tmp_path_factory, row):
    """The same row from pixels with the VAE present (masks at pixel size): every step of the run from latent_moments - for an
    inpainting UNet with masked_latent_moments and the latent-size mask - equals it."""
    eager = _eager(row, dev, tmp_path_factory)
    pixel_row = row._replace(front="pixels")
    case = tm.case_for(row)
    tc, states = tm.build(pixel_row, case, dev)
    trace = tm.run_eager(pixel_row, case, dev, states)
    for t, (a, b) in enumerate(zip(eager.trace, trace)):
        sm.assert_snapshots_equal(a, b, f"step {t}, cached against pixels")


# what the two sums of a Prodigy step do not reach within the step: the moments, s and p0 read the scalars select formed from the
# PREVIOUS d; the master, the EMA and the mirror read d_eps of the d that finish has just formed from the sums
_SUM_FREE = ("mom", "mom2", "prodigy_s", "prodigy_p0", "sqnorm", "count", "prodigy_step")


@pytest.mark.parametrize("row", [r for r in ROWS_AB if r.K == 2], ids=tm.row_id)
def test_identical_micro_batches_equal_the_plain_step(dev, monkeypatch, row):
    """batch = b ++ b with identical draws and K = 2, the row's mask and loss type on, accumulates g + g and scales by 1/2, exact in
    fp32: after the optimizer step every buffer of every stepping store equals the plain K = 1 step on b (ordinary norm pass) - over
    two carried steps.  A Prodigy store with bf16 gradients takes its two sums in one launch over the accumulated buffer instead of
    one per gradient buffer - another partition of the same terms, so the sums agree to rounding only: its first step is compared in
    full but for the l1 slot (the dot is zero and d stays), its second in the buffers the sums do not reach."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests.helpers import to_dev
    monkeypatch.setattr(tu, "_FUSED_NORM", False)
    case = tm.case_for(row)
    half = lambda d: {k: v[: v.shape[0] // 2] for k, v in d.items()}
    twice = lambda d: {k: torch.cat([v, v]).contiguous() for k, v in d.items()}
    runs, lps, partitioned = [], [], set()
    for K in (1, 2):
        tc, states = tm.build(row, case, dev)
        gen = torch.Generator(device=dev)
        trace = []
        for t in range(2):
            hb, hr = tm.host_inputs(row, case, t)
            batch, rand = (half(hb), half(hr)) if K == 1 else (twice(half(hb)), twice(half(hr)))
            batch, rand = to_dev(batch, dev), to_dev(rand, dev)
            if row.front == "cached":
                batch = tm.cached_batch(batch, case, dev, K)
            out = tm.step(row, states, batch, rand, gen, K)
            snap = tm.snapshot(row, states, out, gen)
            lps.append(snap.pop("loss_per_sample", None))
            trace.append(snap)
        for name, st in tm.stepping(states):
            assert (st.opt_store.gacc is not None) == (K == 2), f"{name}: K = {K}"
            if st.opt_store.optimizer == "prodigy" and st.opt_store.grad16 is not None:
                partitioned.add(name)
        runs.append(trace)
    assert (lps[0] is not None) == (row.mask == "on" or row.loss != "l2")
    for t in range(2):
        a, b = dict(runs[1][t]), dict(runs[0][t])
        for name in partitioned:
            keys = [k for k in a if k.startswith(name + ".")]
            if t == 0:
                for s in (a, b):
                    s[f"{name}.prodigy_state"] = s[f"{name}.prodigy_state"].clone()
                    s[f"{name}.prodigy_state"][6] = 0.0
                assert float(a[f"{name}.prodigy_state"][5]) == 0.0
            else:
                for k in keys:
                    if k.split(".", 1)[1] not in _SUM_FREE:
                        a.pop(k), b.pop(k)
        sm.assert_snapshots_equal(a, b, f"step {t}: two identical micro-batches against the plain step")
        if lps[t] is not None:
            assert torch.equal(lps[2 + t], torch.cat([lps[t], lps[t]])), f"step {t}: loss per sample"


# ------------------------------------------------------------------------------------------------ (b) the optimizer step
@pytest.mark.parametrize("row", ROWS_AB, ids=tm.row_id)
def test_optimizer_steps_equal_the_restatement(dev, tmp_path_factory, row):
    """Master, EMA, bf16 mirror, moments, step counts and scalar blocks after each of the four eager steps equal the restatement
    applied to the previous state - Lion by oracle/lion8.py, AdamW by tests/adamw_reference.py, Prodigy by tests/prodigy_reference.py
    with d, d_max, numer and the two ordered sums carried across the launches of the store - with each leaf's own flags, the
    documented hyper-parameters and the schedule's table entry of the step; a token store's rows after its retraction.  The flags
    themselves: the config's exclusion lists; the stepping store: the task's own."""
    eager = _eager(row, dev, tmp_path_factory)
    tm.check_flags(row, eager.built.tc, eager.built.states)
    if eager.restatement_error is not None:
        raise eager.restatement_error
    assert eager.steps_checked == tm.STEPS


# ------------------------------------------------------------------------------------------------ (c) gradients
def _cos(a, b):
    """In float64: a float32 norm over the 25 M gradient elements of the SDXL rows comes out up to 0.5 % low, which lifts a float32
    cosine above 1 and would let a gradient at 0.990 through a 0.995 gate."""
    a, b = a.double(), b.double()
    return float(torch.dot(a, b) / (a.norm() * b.norm()))


def _gates(tree, norm, ref, what):
    """test_gpu_lora._gates - cosine > 0.995 over all leaves, rel-L2 of the worst significant leaf < 0.1, the norm the clip saw within
    3e-2 - on a recorded gradient tree, with the sums taken in float64 (_cos)."""
    flat = torch.cat([tree[k].flatten().cpu() for k in ref]).double()
    rflat = torch.cat([ref[k].flatten() for k in ref]).double()
    cos = _cos(flat, rflat)
    worst = max((rel_l2(tree[k], ref[k]), k) for k in ref if ref[k].double().norm() > 1e-3 * rflat.norm())
    gn = float(rflat.norm())
    print(f"[{what}] cosine {cos:.5f}, worst leaf {worst[0]:.4f} ({worst[1]}), |g| {norm:.5e} vs {gn:.5e}")
    assert cos > 0.995, f"{what}: gradient cosine {cos}"
    assert worst[0] < 0.1, f"{what}: worst leaf {worst}"
    assert abs(norm - gn) / gn < 3e-2, (what, norm, gn)


def _taps(row, case, dev):
    """A K = 1 aux= step over the whole batch of 2 K samples, from pixels, on identically built states and the inputs of step 0: the
    quantities that depend on no trained leaf."""
    pixel_row = row._replace(front="pixels", K=1)
    tc, states = tm.build(pixel_row, case, dev)
    hb, hr = tm.host_inputs(row, case, 0)
    batch, rand = tm.device_inputs(pixel_row, case, dev, hb, hr, 1)
    aux = {}
    tm.step(pixel_row, states, batch, rand, torch.Generator(device=dev), 1, aux=aux)
    torch.cuda.synchronize()
    return aux, hb, hr


def _check_taps(row, case, aux, hb, hr, e, c):
    """Each tap against its own reference: the noisy latents (and the packed inpainting input) against the oracle's VAE and scheduler
    (rel-L2 < 2e-2, test_step_builds_the_reference_input_and_matches_the_oracle_unet's), the target against the draw, the effective
    mask against masked_loss_reference in every bit, the thresholds against the step's own table in every bit."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests import masked_loss_reference as mr
    front = tm.cpu_front(row, case, hb, hr)
    assert rel_l2(aux["noisy"], front["noisy"]) < 2e-2
    assert torch.equal(aux["target"].cpu(), hr["noise"])
    if tm.inpainting(row):
        x = aux["unet_input"].float().cpu().permute(0, 3, 1, 2)
        assert torch.equal(x[:, :4], aux["noisy"].cpu().to(torch.bfloat16).float())
        assert torch.equal(x[:, 4], front["lmask"]) and 0 < float(front["lmask"].mean()) < 1
        assert rel_l2(x[:, 5:9], front["masked_latents"]) < 2e-2 and float(x[:, 9:].abs().max()) == 0
        x = x[:, :9]
    else:
        x = aux["noisy"].cpu().to(torch.bfloat16).float()
    if row.mask == "on":
        mask = hb["loss_mask"].numpy()
        want = mr.effective_mask(mr.pooled_mask(mask, 8, np.float32), tm.MASK_FLOOR)
        assert np.array_equal(aux["loss_mask"].cpu().numpy().view(np.int32), want.view(np.int32)), "the effective mask"
        assert np.array_equal(want.astype(np.float64), e.numpy()), "loss_operands' mask is not the step's"
        pooled = mr.pooled_mask(mask, 8, np.float64)
        assert all(0 < float(hb["loss_mask"][b].mean()) < 1 for b in range(mask.shape[0])) and bool(((pooled > tm.MASK_FLOOR) & (pooled < 1)).any())
    else:
        assert "loss_mask" not in aux
    if row.loss == "huber":
        table = tu.huber_threshold_table(case["sched_state"]["alphas_cumprod"], tm.HUBER_C, "snr")
        want = table[hr["timesteps"].numpy()]
        assert np.array_equal(aux["huber_c"].cpu().numpy().view(np.int32), want.view(np.int32)), "the thresholds"
        assert np.array_equal(want.astype(np.float64), c.numpy()), "loss_operands' thresholds are not the step's"
    else:
        assert "huber_c" not in aux
    return x


@pytest.mark.parametrize("row", ROWS, ids=tm.row_id)
def test_step_one_loss_and_gradients_match_the_cpu_reference(dev, tmp_path_factory, row):
    """The loss and the gradients of the first step over the whole batch of 2 K samples (K = 2: the accumulated gradient) against the
    task's CPU reference under autograd - oracle.nets, tests/controlnet_reference.py, tests/ip_adapter_reference.py, the text encoder
    recomputed where tokens or the text encoder train - with loss64 on the effective mask, sample factors and thresholds formed on the
    host.  Gates, those of the single-feature tests: the loss within 1e-2; inpaint: test_gpu_lora._gates' (cosine > 0.995, worst
    significant leaf < 0.1, norm within 3e-2); tokens: rel-L2 of the rows' gradient < 0.1; ControlNet and IP-Adapter: cosine > 0.995
    over the kernels and > 0.99 on each of their two groups.  The reference alone must show that the row's options act: the masked
    and the Huber loss differ from the plain one by more than the loss gate, and the Huber threshold cuts through the errors."""
    eager = _eager(row, dev, tmp_path_factory)
    case = tm.case_for(row)
    aux, hb, hr = _taps(row, case, dev)
    kw = tm.loss_kw(row)
    e, k, c = tm.loss_operands(hb, hr["timesteps"], case["sched_state"]["alphas_cumprod"], (8, 8), floor=kw.get("masked_loss_floor", 0.0),
                               normalize=kw.get("normalize_masked_area", False), loss_type=row.loss)
    x = _check_taps(row, case, aux, hb, hr, e, c)
    ctx_tap = embeds_tap = None
    if row.task in ("controlnet", "ip_adapter"):  # the frozen text encoder's output: a tap, held to the oracle's
        ctx_tap = aux["ctx"].float().cpu()
        ctx_ref, added = tm.text_conditioning(case, case["weights"]["clip"], hb["input_ids"], x.shape[0])
        assert rel_l2(ctx_tap, ctx_ref) < 2e-2
        if added is not None:
            embeds_tap = aux["text_embeds"].float().cpu()
            assert rel_l2(embeds_tap, added["text_embeds"]) < 2e-2
    pred, leaves = tm.task_prediction(row, case, eager.built, x, hr["timesteps"], hb, ctx_tap, embeds_tap)
    assert rel_l2(aux["pred"][..., :4].permute(0, 3, 1, 2), pred.detach()) < 2e-2
    loss = tm.loss64(pred, hr["noise"], e, k, c, row.loss)
    got_loss, want_loss = eager.loss0, float(loss.detach())
    # the row's options act on the reference
    p64 = pred.detach()
    if row.mask == "on":
        off = float(tm.loss64(p64, hr["noise"], None, None, c, row.loss))
        assert abs(want_loss - off) / off > 1e-2, f"the mask and the weights move the reference loss by {abs(want_loss - off) / off:.2e} only"
    if row.loss == "huber":
        l2 = float(tm.loss64(p64, hr["noise"], e, k, None, "l2"))
        assert abs(want_loss - l2) / l2 > 1e-2, f"the Huber loss differs from l2 by {abs(want_loss - l2) / l2:.2e} only"
        d = (hr["noise"].double() - p64.double()).abs()
        for b in range(d.shape[0]):
            assert bool((d[b] > c[b]).any()) and bool((d[b] < c[b]).any()), f"sample {b}: the threshold {float(c[b])} cuts nothing"
    flat_leaves = [v for _, tree in leaves for v in tree.values()]
    grads = torch.autograd.grad(loss, flat_leaves, allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for v, g in zip(flat_leaves, grads)]
    print(f"[{tm.row_id(row)}] loss {got_loss:.6f}, reference {want_loss:.6f}")
    assert abs(got_loss - want_loss) / want_loss < 1e-2, f"loss {got_loss}, reference {want_loss}"
    assert [n for n, _ in leaves] == list(eager.grads)
    at = 0
    for name, tree in leaves:
        want = {p: grads[at + i].float() for i, p in enumerate(tree)}
        at += len(tree)
        got, norm = eager.grads[name]
        tag = f"{tm.row_id(row)}: {name}"
        flat = lambda keys, src: torch.cat([src[p].flatten().float().cpu() for p in keys])
        if row.task == "inpaint":
            _gates(got, norm, want, tag)
        elif row.task == "tokens":
            for p, w in want.items():
                err = rel_l2(got[p], w)
                print(f"[{tag}] {p}: rel-L2 {err:.4f}, |g| {float(w.norm()):.3e}")
                assert float(w.norm()) > 0 and err < 0.1, (p, err)
        else:
            kernels = [p for p in want if p.endswith("/kernel")]
            if row.task == "controlnet":
                groups = {"embedder": [p for p in kernels if p.startswith("controlnet_cond_embedding/")],
                          "zero convolutions": [p for p in kernels if p.startswith(("controlnet_down_blocks_", "controlnet_mid_block"))]}
            else:
                groups = {"image_proj": [p for p in want if p.startswith("image_proj/")],
                          "to_k_ip / to_v_ip": [p for p in kernels if "/to_k_ip/" in p or "/to_v_ip/" in p]}
            cos = _cos(flat(kernels, got), flat(kernels, want))
            print(f"[{tag}] cosine over {len(kernels)} kernels {cos:.5f}")
            assert cos > 0.995, (tag, cos)
            for gname, keys in groups.items():
                a, b = flat(keys, got), flat(keys, want)
                assert keys and float(a.abs().max()) > 0 and _cos(a, b) > 0.99, (tag, gname, _cos(a, b))


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_pairs_are_refused_off_default(dev):
    """Every REFUSED pair by its ValueError, in a row that holds the pair with the other options off their defaults, before any
    kernel runs.  (The list is empty at this commit: the loop then checks nothing and the coverage test shows that no row is missing.)"""
    for ax, u, ay, v, message in tm.REFUSED:
        row = next(r for r in tm.all_rows() if getattr(r, ax) == u and getattr(r, ay) == v)
        case = tm.case_for(row)
        with pytest.raises(ValueError, match=message):
            tc, states = tm.build(row, case, dev)
            check = _untouched(states)
            batch, rand = tm.inputs(row, case, dev, 0)
            try:
                tm.step(row, states, batch, rand, torch.Generator(device=dev), row.K)
            finally:
                check()
    assert len(tm.rows()) == 16 - sum(1 for r in tm.all_rows() if tm.refused(r)) + len(tm.REPLACEMENTS)
