"""train_step where its options meet, on a real MI355X: the pairwise matrix of tests/step_matrix.py (optimizer x adapter x front x
micro-batches x schedule x conditioning, 16 rows) and one row with everything on, at the tiny configuration (image 64, B = 2 * K, 77
tokens), four steps per run.

(a) path equivalences, bit for bit on every buffer the step writes: the graphed shape table, save / load (and the adapter file) in the
    middle of a run, cached latents against pixels, two identical micro-batches against the plain step;
(b) every optimizer step against the project's restatements (tests/adamw_reference.py, oracle/lion8.py) applied leaf by leaf to a host
    copy of the previous state, from the gradient the sweep read, with the DOCUMENTED hyper-parameters and the schedule's tables - the
    restatements equal the kernels bit for bit (test_gpu_adamw.py, test_gpu_reduce_optim_exact.py), so a mismatch here is wiring;
(c) the gradients of step 1 against the CPU oracle with the gates of test_gpu_lora._gates / test_tiny_train_step_parity.
The checks of a row are separate tests over one shared eager run of the row."""
import dataclasses

import pytest
import torch

from tests import step_matrix as sm

pytestmark = pytest.mark.gpu
ROWS = sm.rows()
ROWS_AB = ROWS + [sm.ALL_ON]


@dataclasses.dataclass
class _Eager:
    trace: list
    restatement_error: object
    steps_checked: int
    grads: dict        # after step 0: {"unet" / "text": (exported gradient tree, gradient norm)}
    loss0: float
    built: object
    files: dict        # written after step 2: training state, adapter files, the mirrors merged from the saved leaves


_RUNS = {}


def _eager(row, dev, tmp_path_factory):
    """The row's uninterrupted eager run, once: four steps, each followed by the restatement check (b) - its first failure is kept for
    test_optimizer_steps_equal_the_restatement, the run goes on - with the gradients of step 0 set aside for (c) and the files of the
    resume test written after step 2."""
    if row in _RUNS:
        if isinstance(_RUNS[row], BaseException):  # the run failed once: every check of the row reports it, none repeats it
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
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev)
    built = sm.build.last
    hp = sm.documented_hyper(row.opt, sm.RATE)
    refs = {name: sm.reference_state(st.opt_store) for name, st in sm.stepping(states)}
    tmp = tmp_path_factory.mktemp("resume")
    rec = _Eager([], None, 0, {}, 0.0, built, dict(state=str(tmp / "state.safetensors"), adapters={}, mirrors={}))

    def after_step(t, states, out):
        torch.cuda.synchronize()
        if t == 0:
            rec.loss0 = float(out[4]["loss"].item())
            for name, st in sm.stepping(states):
                rec.grads[name] = (st.opt_store.export("grad"), st.opt_store.grad_norm())
        if rec.restatement_error is None:
            try:
                for name, st in sm.stepping(states):
                    store = st.opt_store
                    g = sm.gradient_seen(store, row.K)
                    cur = sm.reference_store_step(store, refs[name], g, hp, sm.EMA_RATE, built.schedules[name])
                    sm.check_store(store, refs[name], cur, f"{sm.row_id(row)} step {t}: {name}")
                rec.steps_checked = t + 1
            except AssertionError as e:
                rec.restatement_error = e
        if t == 1:
            tu.save_training_state(rec.files["state"], states[0], states[1])
            for name, st in sm.stepping(states):
                if st.adapter is not None:
                    rec.files["adapters"][name] = str(tmp / f"{name}_adapter.npz")
                    st.adapter.save(rec.files["adapters"][name])
                    st.adapter.merge("master")  # the mirror of the saved leaves (the next step's own merge writes the same)
                    torch.cuda.synchronize()
                    rec.files["mirrors"][name] = st.store.w.clone()

    rec.trace = sm.run_eager(row, case, dev, states, after_step=after_step)
    assert all(st.opt_store.count == sm.STEPS for _, st in sm.stepping(states))
    assert len({float(s["loss"]) for s in rec.trace}) == sm.STEPS and all(bool(torch.isfinite(s["loss"])) for s in rec.trace)
    for name, _ in sm.stepping(states):  # four steps moved the masters and the moments
        assert not torch.equal(rec.trace[0][f"{name}.master"], rec.trace[-1][f"{name}.master"]), f"{name}: the masters never moved"
    return rec


# ------------------------------------------------------------------------------------------------ (a) path equivalences
@pytest.mark.parametrize("row", ROWS_AB, ids=sm.row_id)
def test_graphed_table_equals_the_eager_steps(dev, tmp_path_factory, row):
    """Four steps through dp_compile_all_unique_resolution(use_graph=True, micro_batches=K): two eager calls, the capture, then replays -
    every snapshot key of every step equals the eager run's."""
    eager = _eager(row, dev, tmp_path_factory)
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev)
    fn, trace = sm.run_graphed(row, case, dev, tc, states)
    assert fn.graph is not None and fn.calls == 2, "the last calls were to replay the captured step"
    for name, st in sm.stepping(states):
        assert st.opt_store.count == sm.STEPS and st.step == sm.STEPS, f"{name}: host step count {st.opt_store.count} after four calls"
        if st.adapter is not None:
            assert st.store.count == 0
    for t, (a, b) in enumerate(zip(eager.trace, trace)):
        sm.assert_snapshots_equal(b, a, f"step {t}, graphed table against eager")


@pytest.mark.parametrize("row", ROWS_AB, ids=sm.row_id)
def test_resumed_step_equals_the_uninterrupted_run(dev, tmp_path_factory, row):
    """save_training_state after step 2 (and adapter.save of every adapter), fresh states with OTHER adapter leaves, load, step 3: the
    schedule's position, AdamW's counter and products, the adapter stores and the re-merged mirror continue the uninterrupted run."""
    from stable_diffusion_training_amd import training_utils as tu
    eager = _eager(row, dev, tmp_path_factory)
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev, factor_seed=61)
    for name, st in sm.stepping(states):
        assert st.opt_store.count == 0
        if st.adapter is not None:
            assert not torch.equal(st.opt_store.master, eager.trace[1][f"{name}.master"])
            st.adapter.load(eager.files["adapters"][name])  # (loads and merges)
            torch.cuda.synchronize()
            assert torch.equal(st.store.w, eager.files["mirrors"][name]), f"{name}: the adapter file does not restore the merged mirror"
            for q, lf in st.opt_store.leaves.items():  # (leaf by leaf: the file holds no alignment gaps)
                assert torch.equal(st.opt_store.p(q).reshape(-1), eager.trace[1][f"{name}.master"][lf.offset: lf.offset + lf.numel]), q
    tu.load_training_state(eager.files["state"], states[0], states[1])
    for name, st in sm.stepping(states):
        store = st.opt_store
        assert st.step == 2 and store.count == 2
        if store.optimizer == "adamw":
            assert int(store.adam_step.item()) == 2
            assert torch.equal(store.adam_prod, eager.trace[1][f"{name}.adam_prod"]), "the products rebuilt on the host"
        elif row.sched != "constant":
            assert int(store._sched["step"].item()) == 2
    resumed = sm.run_eager(row, case, dev, states, steps=1, first=2)[0]
    sm.assert_snapshots_equal(resumed, eager.trace[2], "step 3 after save / load against the uninterrupted run")


@pytest.mark.parametrize("row", [r for r in ROWS_AB if r.front == "cached"], ids=sm.row_id)
def test_cached_front_equals_the_pixel_front(dev, tmp_path_factory, row):
    """The same row from pixels with the VAE present: every step of the run from latent_moments with frozen_vae_state=None equals it."""
    eager = _eager(row, dev, tmp_path_factory)
    pixel_row = row._replace(front="pixels")
    case = sm.case_for(row)
    tc, states = sm.build(pixel_row, case, dev)
    trace = sm.run_eager(pixel_row, case, dev, states)
    for t, (a, b) in enumerate(zip(eager.trace, trace)):
        sm.assert_snapshots_equal(a, b, f"step {t}, cached against pixels")


@pytest.mark.parametrize("row", [r for r in ROWS_AB if r.K == 2], ids=sm.row_id)
def test_identical_micro_batches_equal_the_plain_step(dev, monkeypatch, row):
    """batch = b ++ b with identical draws and K = 2 accumulates g + g and scales by 1/2, exact in fp32: after the optimizer step every
    buffer of every stepping store equals the plain K = 1 step on b (ordinary norm pass) - over two carried steps, so that nothing of
    the first step's sum survives into the second."""
    from stable_diffusion_training_amd import training_utils as tu
    from tests.helpers import to_dev
    monkeypatch.setattr(tu, "_FUSED_NORM", False)
    case = sm.case_for(row)
    half = lambda d: {k: v[: v.shape[0] // 2] for k, v in d.items()}
    twice = lambda d: {k: torch.cat([v, v]).contiguous() for k, v in d.items()}
    runs = []
    for K in (1, 2):
        tc, states = sm.build(row, case, dev)
        gen = torch.Generator(device=dev)
        trace = []
        for t in range(2):
            hb, hr = sm.host_inputs(row, case, t)
            batch, rand = (half(hb), half(hr)) if K == 1 else (twice(half(hb)), twice(half(hr)))
            batch, rand = to_dev(batch, dev), to_dev(rand, dev)
            if row.front == "cached":
                batch = sm.cached_batch(batch, case, dev, K)
            out = sm.step(states, batch, rand, gen, K, vae=None if row.front == "cached" else "own")
            trace.append(sm.snapshot(states, out, gen))
        for name, st in sm.stepping(states):
            assert (st.opt_store.gacc is not None) == (K == 2), f"{name}: K = {K}"
        runs.append(trace)
    for t in range(2):
        sm.assert_snapshots_equal(runs[1][t], runs[0][t], f"step {t}: two identical micro-batches against the plain step")


# ------------------------------------------------------------------------------------------------ (b) the optimizer step
@pytest.mark.parametrize("row", ROWS_AB, ids=sm.row_id)
def test_optimizer_steps_equal_the_restatement(dev, tmp_path_factory, row):
    """Master, EMA, bf16 mirror, both moment states and AdamW's scalar block, counter and products after each of the four eager steps
    equal the restatement applied to the previous state - with each leaf's own decayed / quantised flags, the documented hyper-parameters
    (AdamW: the rate as given, wd 1e-2, b2 0.999, eps 1e-8; Lion: rate / 7, wd 0.07, b2 0.99; clip at norm 1) and the rates of the
    schedule's tables at that step.  The flags themselves: the config's exclusion lists, and DoRA's lora_m with fp32 moments, undecayed."""
    eager = _eager(row, dev, tmp_path_factory)
    sm.check_flags(row, eager.built.tc, eager.built.states)
    if eager.restatement_error is not None:
        raise eager.restatement_error
    assert eager.steps_checked == sm.STEPS


# ------------------------------------------------------------------------------------------------ (c) gradients
class _Recorded:
    """The gradient of a store as recorded after step 0, with the two methods test_gpu_lora._gates reads."""

    def __init__(self, tree, norm):
        self.tree, self.norm = tree, norm

    def export(self, which):
        assert which == "grad"
        return self.tree

    def grad_norm(self):
        return self.norm


@pytest.mark.parametrize("row", ROWS, ids=sm.row_id)
def test_step_one_gradients_match_the_cpu_oracle(dev, tmp_path_factory, row):
    """The gradients of the first step - of the weight stores, or of the adapter stores against the oracle's kernel gradients on the
    folded tree pushed through the float64 projection - with test_gpu_lora._gates: cosine > 0.995, worst significant leaf < 0.1, norm
    within 3e-2; the loss within 1e-2.  K = 2: the oracle runs the whole batch.  sdxl: the oracle is oracle_sdxl_step."""
    from tests.test_gpu_lora import _gates
    eager = _eager(row, dev, tmp_path_factory)
    loss, refs = sm.oracle_gradients(row, sm.case_for(row), eager.built)
    assert abs(eager.loss0 - loss) / loss < 1e-2, (eager.loss0, loss)
    assert len(refs) == len(eager.grads)
    for (name, (tree, norm)), (store, want) in zip(eager.grads.items(), refs):
        assert set(want) <= set(tree)
        _gates(_Recorded(tree, norm), want, f"{sm.row_id(row)}: {name}")


# ------------------------------------------------------------------------------------------------ refusals
def _untouched(states):
    """A check that no store of the states took a step or had its master written."""
    stores = [s for st in states[:2] for s in (st.store, st.opt_store) if s is not None]
    before = [(s, s.count, s.master.clone()) for s in stores]

    def check():
        torch.cuda.synchronize()
        for s, count, master in before:
            assert s.count == count and torch.equal(s.master, master), "a refused step changed a store"
    return check


def test_refusals_hold_off_default(dev, tmp_path):
    """The three refusals that guard unsupported pairs, with the other options off their defaults; each before any kernel."""
    import torch.distributed as dist
    from stable_diffusion_training_amd import dp
    # a reducer with adapter states: AdamW-8bit, DoRA, a schedule installed
    row = sm.Row("adamw8", "dora", "pixels", 1, "cosine+ema_warmup", "sd")
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev)
    batch, rand = sm.inputs(row, case, dev, 0)
    check = _untouched(states)
    with pytest.raises(ValueError, match="GradReducer over the adapter stores"):
        _step_with(states, batch, rand, dev, 1, reducer=object())
    check()
    # micro_batches = 2 with the sharded optimizer over AdamW stores (a one-rank group with the exchange forced on)
    row = sm.Row("adamw8", "none", "pixels", 2, "constant", "sd")
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev)
    batch, rand = sm.inputs(row, case, dev, 0)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'group'}", rank=0, world_size=1)
    try:
        red = dp.GradReducer([states[0].store, states[1].store], bucket_bytes=1 << 16, force=True, shard=True)
        assert red.shard and red.active and states[0].store.optimizer == "adamw"
        check = _untouched(states)
        with pytest.raises(ValueError, match="not supported with the sharded optimizer"):
            _step_with(states, batch, rand, dev, 2, reducer=red)
        check()
    finally:
        dist.destroy_process_group()
    # cached latents in SDXL mode without time_ids
    row = sm.ALL_ON
    case = sm.case_for(row)
    tc, states = sm.build(row, case, dev)
    batch, rand = sm.inputs(row, case, dev, 0)
    assert "latent_moments" in batch and "time_ids" in batch
    check = _untouched(states)
    with pytest.raises(ValueError, match="must hold time_ids"):
        _step_with(states, {k: v for k, v in batch.items() if k != "time_ids"}, rand, dev, 2, vae=None)
    check()


def _step_with(states, batch, rand, dev, K, **kw):
    from stable_diffusion_training_amd import training_utils as tu
    us, ts, ue, te, vae, sc, _ = states
    vae = kw.pop("vae", vae)
    return tu.train_step(us, ts, ue, te, batch, torch.Generator(device=dev), vae, sc, strip_bos_eos_token=False, ema_rate=sm.EMA_RATE, rand=rand,
                         micro_batches=K, **kw)
