"""The pairwise matrix of train_step options and the harness its tests share (DESIGN.md "Option combinations").

Six axes - optimizer, adapter, front, micro-batches, schedule, conditioning - and 16 rows, one per (optimizer, adapter) pair; the four
binary axes follow from the two indices by a fixed rule (row_for) under which every pair of values of every two axes meets in some row
(tests/test_step_matrix_cpu.py recomputes that).  build / inputs / snapshot make the states, the per-step inputs and the bitwise
record of a step for a row; reference_store_step / check_store apply the project's restatements of the optimizer (tests/adamw_reference.py,
oracle/lion8.py) leaf by leaf to a host copy of a store and hold the store to it in every bit.  Nothing here touches a GPU at import."""
import collections
import dataclasses
import itertools

import numpy as np
import torch

from oracle import lion8
from tests import adamw_reference as AR
from tests import kernel_checks as kc
from tests.kernel_checks import BF, assert_equal_bits

OPTS = ("lion8", "lion32", "adamw8", "adamw32")  # 8: quantize_*_state=True
ADAPTERS = ("none", "lora", "lora_te_frozen", "dora")  # lora / dora adapt the text encoder too
AXES = collections.OrderedDict(opt=OPTS, adapter=ADAPTERS, front=("pixels", "cached"), K=(1, 2), sched=("constant", "cosine+ema_warmup"),
                               cond=("sd", "sdxl"))
Row = collections.namedtuple("Row", tuple(AXES))

# Pairs of axis values that train_step or create_lion_optimizer_states refuse by ValueError: (axis, value, axis, value, message regex).
# Only a row that holds such a pair may be missing from rows(); at this commit every pair of the six axes is supported.
REFUSED = ()

ALL_ON = Row("adamw8", "lora", "cached", 2, "cosine+ema_warmup", "sdxl")  # no rule forces all of these into one row
STEPS = 4
EMA_RATE = 0.999
RATE = 1e-4   # the learning rate the runs use (the states are built with the reference's 1e-6): four steps move every buffer
BUILT_RATE = 1e-6
LR_SCHEDULE = dict(num_warmup_steps=1, num_training_steps=6)
EMA_SCHEDULE = dict(kind="warmup")
# the exclusion lists of the other model tests plus one pattern each that reaches adapter leaves, so that an adapter store holds a leaf
# in each of the four (quantised x decayed) segments: lora_b takes no decay, the output projections keep fp32 moments
WD_EXCLUDED = ["bias", "scale", "embedding", "lora_b"]
QUANT_EXCLUDED = ["bias", "scale", "embedding", "conv_in", "conv_out", "time_embedding", "embeddings", "time_emb_proj", "to_out_0", "out_proj"]
RANK, ALPHA = 8, 4.0
# (a store holds None for the buffers of another optimizer: Prodigy's are skipped by a Lion / AdamW store and the reverse)
STATE = ("master", "w", "codes", "inv_scale", "codes2", "inv_scale2", "mom", "mom2", "ema", "adam_step", "adam_prod", "adam_cur", "sqnorm",
         "prodigy_s", "prodigy_p0", "prodigy_state", "prodigy_step", "prodigy_cur")
STEP_HP = dict(lr=1e-3, wd=0.07, eps=1e-8, max_norm=1.0)  # tests/test_gpu_adamw.py's store-level steps
WORKERS = 8  # threads the harness's reference step spreads a store's leaves over


# ------------------------------------------------------------------------------------------------ the matrix
def row_for(o, a):
    """The row of optimizer index o and adapter index a (0..3): front = o0^a0, K = 1 + (o1^a1), sched = o0^a1, cond = o1^a0, with o0 / o1
    the low and high bit of o and a0 / a1 those of a."""
    o0, o1, a0, a1 = o & 1, o >> 1, a & 1, a >> 1
    return Row(OPTS[o], ADAPTERS[a], AXES["front"][o0 ^ a0], AXES["K"][o1 ^ a1], AXES["sched"][o0 ^ a1], AXES["cond"][o1 ^ a0])


def refused(row):
    """The REFUSED entry a row falls under, or None."""
    for entry in REFUSED:
        if getattr(row, entry[0]) == entry[1] and getattr(row, entry[2]) == entry[3]:
            return entry
    return None


def all_rows():
    return [row_for(o, a) for o in range(4) for a in range(4)]


def rows():
    """The 16 (optimizer, adapter) rows, less those that hold a refused pair."""
    return [r for r in all_rows() if refused(r) is None]


def row_id(row):
    return f"{row.opt}-{row.adapter}-{row.front}-K{row.K}-{row.sched.split('+')[0]}-{row.cond}"


def covered_pairs(rs):
    """{(axis, value, axis, value)} over all C(6, 2) axis pairs that some row of rs holds."""
    return {(x, getattr(r, x), y, getattr(r, y)) for r in rs for x, y in itertools.combinations(AXES, 2)}


def all_pairs():
    return {(x, u, y, v) for x, y in itertools.combinations(AXES, 2) for u in AXES[x] for v in AXES[y]}


def documented_hyper(opt, rate):
    """TrainState.hyper as create_lion_optimizer_states documents it: AdamW takes the rate as given with wd 1e-2, b2 0.999, eps 1e-8; Lion
    takes rate / 7 with wd 0.07, b2 0.99; both clip at global norm 1."""
    if opt.startswith("adamw"):
        return dict(lr=rate, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0)
    return dict(lr=rate / 7, wd=0.07, b1=0.9, b2=0.99, max_norm=1.0)


# ------------------------------------------------------------------------------------------------ restatements, leaf by leaf
def _leaves(st, fn, workers):
    """fn(path, leaf) for every leaf of the store; the leaves are independent, so a harness with large stores spreads them over threads
    (NumPy releases the interpreter lock inside its loops; every leaf's result is the same either way)."""
    if workers <= 1:
        for path, lf in st.leaves.items():
            fn(path, lf)
        return
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda item: fn(*item), list(st.leaves.items())))


def _reference_store_step(st, ref, g_flat, cur, hp=STEP_HP, workers=1):
    """One restatement step of every leaf of the AdamW store `st` on ref = dict(p, m (path -> state), ema): g_flat the float32 gradient in
    master order as the sweep reads it."""
    sq = float(np.sum(g_flat.astype(np.float64) ** 2))
    b1, b2 = st.adam_betas

    def leaf(path, lf):
        g = g_flat[lf.offset: lf.offset + lf.numel]
        kw = dict(wd=hp["wd"] if lf.decayed else 0.0, b1=b1, b2=b2, eps=hp["eps"], max_norm=hp["max_norm"], sq=sq)
        if lf.quantised:
            ref["p"][path], ref["m"][path] = AR.step8(ref["p"][path], g, ref["m"][path], cur, bs=st.block_size, **kw)
        else:
            ref["p"][path], m, v = AR.step32(ref["p"][path], g, *ref["m"][path], cur, **kw)
            ref["m"][path] = (m, v)
        ref["ema"][path] = AR.ema_update(ref["ema"][path], ref["p"][path], cur)

    _leaves(st, leaf, workers)


def _lion_reference_store_step(st, ref, g_flat, lr, ema_rate, hp, workers=1):
    """The same for a Lion store by oracle.lion8: the clip with the whole buffer's norm (adamw_reference.clip is oracle.lion8's with the
    squared norm handed in), then lion_step and ema_update on one leaf at a time.  lr and ema_rate: the step's float64 scalars."""
    sq = float(np.sum(g_flat.astype(np.float64) ** 2))

    def leaf(path, lf):
        g = AR.clip(g_flat[lf.offset: lf.offset + lf.numel], hp["max_norm"], sq)
        newp, state, _ = lion8.lion_step({"x": ref["p"][path]}, {"x": g}, {"count": 0, "mu": {"x": ref["m"][path]}}, lr=lr, wd=hp["wd"],
                                         b1=hp["b1"], b2=hp["b2"], block_size=st.block_size, decay_mask={"x": lf.decayed}, clip=None)
        ref["p"][path], ref["m"][path] = newp["x"], state["mu"]["x"]
        if ref["ema"] is not None:
            ref["ema"][path] = lion8.ema_update({"x": ref["ema"][path]}, newp, ema_rate)["x"]

    _leaves(st, leaf, workers)


def _check_store(st, ref, tag, mirror_of=None):
    """Master, EMA, bf16 mirror and the moment states of every leaf of `st` against ref, in every bit.  mirror_of: {path: the values
    the sweep mirrored} where something rewrote the master after the sweep (a token store's retraction); None: the master's."""
    adamw = st.optimizer == "adamw"
    master, ema = st.export("master"), (st.export("ema") if st.ema is not None else None)
    mm, ss = st.export_momentum("m"), (st.export_momentum("s") if adamw else None)
    for path, lf in st.leaves.items():
        assert_equal_bits(master[path].reshape(-1).cpu(), torch.from_numpy(ref["p"][path]), f"{tag}: {path} master")
        if ema is not None:
            assert_equal_bits(ema[path].reshape(-1).cpu(), torch.from_numpy(ref["ema"][path]), f"{tag}: {path} ema")
        mirrored = ref["p"][path] if mirror_of is None else mirror_of[path]
        assert_equal_bits(st.w[lf.offset: lf.offset + lf.numel].cpu(), torch.from_numpy(mirrored).to(BF), f"{tag}: {path} bf16 mirror")
        if lf.quantised and adamw:
            for name, (c, i), wc, wi in (("m", mm[path], *ref["m"][path][:2]), ("s", ss[path], *ref["m"][path][2:])):
                msg = kc.lion_state_report(c.cpu().numpy(), i.cpu().numpy(), wc, wi, f"{tag}: {path} {name}")
                assert msg is None, msg
        elif lf.quantised:
            msg = kc.lion_state_report(mm[path][0].cpu().numpy(), mm[path][1].cpu().numpy(), *ref["m"][path], f"{tag}: {path} momentum")
            assert msg is None, msg
        elif adamw:
            assert_equal_bits(mm[path].reshape(-1).cpu(), torch.from_numpy(ref["m"][path][0]), f"{tag}: {path} m")
            assert_equal_bits(ss[path].reshape(-1).cpu(), torch.from_numpy(ref["m"][path][1]), f"{tag}: {path} v")
        else:
            assert_equal_bits(mm[path].reshape(-1).cpu(), torch.from_numpy(ref["m"][path]), f"{tag}: {path} momentum")


def reference_state(st):
    """ref = dict(p, m, ema) of flat host copies of every leaf of `st` as it stands, plus the optimizer's host scalars: t (steps taken)
    and, for AdamW, the running products."""
    host = lambda t: t.detach().reshape(-1).cpu().numpy().copy()
    ref = dict(p={p: host(st.p(p)) for p in st.leaves}, m={}, ema=None, t=int(st.count), prods=None)
    if st.ema is not None:
        ref["ema"] = {p: host(st.ema[lf.offset: lf.offset + lf.numel]) for p, lf in st.leaves.items()}
    adamw = st.optimizer == "adamw"
    mm, ss = st.export_momentum("m"), (st.export_momentum("s") if adamw else None)
    for p, lf in st.leaves.items():
        if lf.quantised:
            m = tuple(x.cpu().numpy().copy() for x in mm[p])
            ref["m"][p] = m + tuple(x.cpu().numpy().copy() for x in ss[p]) if adamw else m
        else:
            ref["m"][p] = (host(mm[p]), host(ss[p])) if adamw else host(mm[p])
    if adamw:
        ref["prods"] = tuple(st.adam_prod.tolist())
    return ref


def reference_store_step(st, ref, g_flat, hp, ema_rate, schedule=None):
    """The reference step on exported gradients: one optimizer step of the stepping store `st` restated on ref (reference_state) from
    g_flat, the float32 gradient in master order that the sweep read.  hp: the DOCUMENTED hyper-parameters (documented_hyper), not the
    state's own; ema_rate: the rate train_step was given (0: no EMA); schedule: the (LRSchedule, EMASchedule) the store was built with,
    whose tables give the step's rates at index t.  Returns the scalar block an AdamW store must hold (None for Lion)."""
    g_flat = np.asarray(g_flat, np.float32)
    er = ema_rate if ref["ema"] is not None else 0.0
    if st.optimizer == "adamw":
        assert tuple(st.adam_betas) == (hp["b1"], hp["b2"]), f"the store carries betas {st.adam_betas}, documented {hp['b1'], hp['b2']}"
        kw = dict(lr=hp["lr"], ema_rate=er) if schedule is None else dict(lr_tab=schedule[0].table(), ema_tab=schedule[1].table())
        cur, ref["t"], ref["prods"] = AR.select_scalars(ref["t"], ref["prods"], hp["b1"], hp["b2"], **kw)
        if ref["ema"] is None:  # (ema_update is then never read; keep the dicts' shape)
            ref["ema"] = {p: ref["p"][p] for p in ref["p"]}
            _reference_store_step(st, ref, g_flat, cur, hp, WORKERS)
            ref["ema"] = None
        else:
            _reference_store_step(st, ref, g_flat, cur, hp, WORKERS)
        return cur
    t = ref["t"]
    lr, r = (hp["lr"], er) if schedule is None else (schedule[0].rate(t), schedule[1].rate(t))
    _lion_reference_store_step(st, ref, g_flat, lr, r, hp, WORKERS)
    ref["t"] = t + 1
    return None


def check_store(st, ref, cur, tag, mirror_of=None):
    """_check_store plus the optimizer's scalars: host count, and for AdamW the device counter, products and scalar block."""
    _check_store(st, ref, tag, mirror_of)
    assert st.count == ref["t"], f"{tag}: host step count {st.count}, expected {ref['t']}"
    if st.optimizer == "adamw":
        assert_equal_bits(st.adam_cur.cpu(), torch.from_numpy(cur), f"{tag}: scalar block")
        assert int(st.adam_step.item()) == ref["t"], f"{tag}: device counter {int(st.adam_step.item())}, expected {ref['t']}"
        assert tuple(st.adam_prod.tolist()) == ref["prods"], f"{tag}: running products"


def check_flags(row, tc, states):
    """The masks of the stepping stores: every leaf with a path component in the config's exclusion lists is excluded and no other is;
    DoRA's magnitudes keep fp32 moments (both of them under AdamW) and take no decay."""
    quant = row.opt.endswith("8")
    for st in states[:2]:
        store = st.opt_store
        if store is None:
            continue
        dora = st.adapter is not None and st.adapter.cfg.dora
        wd_ex = list(tc.excluded_layer_pattern_from_weight_decay) + (["lora_m"] if dora else [])
        q_ex = list(tc.excluded_layer_from_quantization) + (["lora_m"] if dora else [])
        seen = set()
        for path, lf in store.leaves.items():
            comps = path.split("/")
            assert lf.decayed == (not any(e in comps for e in wd_ex)), f"{path}: decayed {lf.decayed}"
            assert lf.quantised == (quant and not any(e in comps for e in q_ex)), f"{path}: quantised {lf.quantised}"
            seen.add((lf.quantised, lf.decayed))
            if comps[-1] == "lora_m":
                assert not lf.quantised and not lf.decayed, f"{path}: a magnitude is quantised / decayed"
                o = lf.offset - store.quant_total
                assert o >= 0 and store.mom[o: o + lf.numel].dtype == torch.float32
                if row.opt.startswith("adamw"):
                    assert store.mom2 is not None and store.mom2[o: o + lf.numel].numel() == lf.numel, f"{path}: no fp32 second moment"
        if st.adapter is not None:
            assert len(seen) == (4 if quant else 2), f"the adapter store holds leaves in {sorted(seen)} only"
            assert dora == (row.adapter == "dora") and any(p.endswith("lora_m") for p in store.leaves) == dora


# ------------------------------------------------------------------------------------------------ cases, states, inputs
_CASES = {}


def case_for(row):
    """The host case of a row (weights, configs, batch of 2 * K, draws), built once per (cond, K) and never written to."""
    key = (row.cond, row.K)
    if key not in _CASES:
        B = 2 * row.K
        if row.cond == "sd":
            from tests.helpers import make_case
            case = make_case("tiny", B=B, image=64)
        else:
            from tests.test_gpu_sdxl_conditioning import _case
            case = _case(B=B, image=64)
            case["batch"]["time_ids"] = torch.tensor([[64, 64, 0, 0, 64, 64]] * B, dtype=torch.int32)
            assert "text_embeds" not in case["batch"]
        _CASES[key] = case
    return _CASES[key]


def models_of(case):
    return {"unet": {"unet_params": case["weights"]["unet"], "config": case["cfgs"]["unet"]},
            "vae": {"vae_params": case["weights"]["vae"], "config": case["cfgs"]["vae"]},
            "text_encoder": {"text_encoder_params": case["weights"]["clip"], "config": case["cfgs"]["clip"]}}


def training_config(row, case):
    from stable_diffusion_training_amd import training_utils as tu
    quant = row.opt.endswith("8")
    return tu.TrainingConfig(
        model_path="synthetic", batch_size=2, learning_rate=BUILT_RATE, unet_learning_rate=BUILT_RATE, text_encoder_learning_rate=BUILT_RATE,
        lr_scheduler="constant" if row.sched == "constant" else "cosine", adam_to_lion_scale_factor=7.0, compilation_cache_path="",
        keep_compiled_fn_in_cache=False, text_encoder_context_window=77, context_window_concatenation_count=1, aot_compile=True,
        strip_bos_eos_token=False, offset_noise_magnitude=0.0, min_snr_gamma_magnitude=0.0, perturbation_noise_magnitude=0.0,
        image_area_root=[512], minimum_axis_length=[512], beta_scheduler=case["sched"], prediction_type="epsilon",
        excluded_layer_pattern_from_weight_decay=list(WD_EXCLUDED), excluded_layer_from_quantization=list(QUANT_EXCLUDED),
        quant_block_size=16, quantize_unet_state=quant, quantize_text_encoder_state=quant, accumulate_unet_ema=True,
        accumulate_text_encoder_ema=True, ema_rate=EMA_RATE)


def lora_config(row):
    from stable_diffusion_training_amd import lora
    if row.adapter == "none":
        return None
    dora = row.adapter == "dora"
    te = "frozen" if row.adapter == "lora_te_frozen" else lora.LoraConfig(RANK, ALPHA, targets=lora.CLIP_TARGETS, seed=2, dora=dora)
    return dict(unet=lora.LoraConfig(RANK, ALPHA, seed=1, dora=dora), text_encoder=te)


def state_kwargs(row):
    """The keywords of on_device_model_training_state / create_lion_optimizer_states a row sets."""
    sched = row.sched != "constant"
    return dict(optimizer="adamw" if row.opt.startswith("adamw") else "lion", lora=lora_config(row),
                lr_schedule=dict(LR_SCHEDULE) if sched else None, ema_schedule=dict(EMA_SCHEDULE) if sched else None)


def raise_rates(row, states):
    """Hold the hyper-parameters the builder wired to the documented ones (built with the reference's 1e-6), then raise the rate to RATE
    as tests/test_gpu_adamw.py does - with a schedule installed, by installing the same schedule over the new base rate.  Returns
    {"unet" / "text": (LRSchedule, EMASchedule) or None} of the stepping stores."""
    from stable_diffusion_training_amd import lr_schedule as L
    out = {}
    for name, st in zip(("unet", "text"), states[:2]):
        store = st.opt_store
        if store is None:
            assert st.hyper == {}, f"{name}: a frozen state carries hyper-parameters {st.hyper}"
            continue
        assert st.hyper == documented_hyper(row.opt, BUILT_RATE), f"{name}: built with {st.hyper}, documented {documented_hyper(row.opt, BUILT_RATE)}"
        st.hyper["lr"] = documented_hyper(row.opt, RATE)["lr"]
        out[name] = None
        if row.sched != "constant":
            lrs, emas = store.schedule
            assert (lrs.name, lrs.base_lr, lrs.num_warmup_steps, lrs.num_training_steps) == ("cosine", documented_hyper(row.opt, BUILT_RATE)["lr"], 1, 6)
            assert (emas.kind, emas.ema_rate) == ("warmup", EMA_RATE)
            store.set_schedule(lr=L.LRSchedule("cosine", st.hyper["lr"], **LR_SCHEDULE), ema=emas)
            out[name] = store.schedule
        else:
            assert store.schedule is None
    return out


def random_adapter_leaves(row, case, states, seed):
    """Random non-zero factors (tests/test_gpu_lora._random_factors; DoRA: test_gpu_dora._random_leaves) loaded into the adapters.
    Returns [unet leaves, text leaves] (None without an adapter)."""
    out = []
    for st, s, weights in ((states[0], seed, case["weights"]["unet"]), (states[1], seed + 1, case["weights"]["clip"])):
        if st.adapter is None:
            out.append(None)
            continue
        if st.adapter.cfg.dora:
            from tests.test_gpu_dora import _random_leaves
            leaves = _random_leaves(st.adapter, weights, s)
        else:
            from tests.test_gpu_lora import _random_factors
            leaves = _random_factors(st.adapter, weights, s)
        st.adapter.store.load(leaves)
        out.append(leaves)
    return out


@dataclasses.dataclass
class Built:
    tc: object
    states: tuple
    schedules: dict
    leaves: list  # the adapters' loaded leaves (host trees), [unet, text]


def build(row, case, dev, factor_seed=31):
    """(tc, states) of a row through on_device_model_training_state, EMA on for both models, the rates raised (raise_rates), random
    non-zero adapter leaves loaded.  The schedules and the adapter leaves travel on build.last (a Built)."""
    from stable_diffusion_training_amd import training_utils as tu
    tc = training_config(row, case)
    states = tu.on_device_model_training_state(tc, models_of(case), device=dev, **state_kwargs(row))
    schedules = raise_rates(row, states)
    leaves = random_adapter_leaves(row, case, states, factor_seed) if row.adapter != "none" else [None, None]
    build.last = Built(tc, states, schedules, leaves)
    return tc, states


def host_inputs(row, case, step):
    """(batch, rand) of a step on the host: the case's pixels shifted by 0.05 * step, fresh seeded draws."""
    g = torch.Generator().manual_seed(100 + step)
    batch = dict(case["batch"])
    batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
    rand = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else torch.randint(0, 1000, v.shape, generator=g).to(v.dtype))
            for k, v in case["rand"].items()}
    return batch, rand


_VAE = {}


def _frozen_vae(case, dev):
    """The frozen VAE of a case on its own (what builds a latent cache), one per case."""
    from stable_diffusion_training_amd import nets
    from stable_diffusion_training_amd import training_utils as tu
    from stable_diffusion_training_amd.params import ParamStore
    if id(case) not in _VAE:
        store = ParamStore(nets.vae_encoder_spec(case["cfgs"]["vae"]), device=dev, trainable=False)
        store.load(case["weights"]["vae"])
        store.prepare()
        _VAE[id(case)] = tu.FrozenModel(call=case["cfgs"]["vae"], params=store)
    return _VAE[id(case)]


def cached_batch(batch, case, dev, micro_batches):
    """The batch with latent_moments in place of its pixels: encode_latent_moments at the micro-batch composition."""
    from stable_diffusion_training_amd import training_utils as tu
    vae, px = _frozen_vae(case, dev), batch["pixel_values"]
    n = px.shape[0] // micro_batches
    out = {k: v for k, v in batch.items() if k != "pixel_values"}
    out["latent_moments"] = torch.cat([tu.encode_latent_moments(vae, px[k * n: (k + 1) * n].contiguous()) for k in range(micro_batches)]).contiguous()
    return out


def inputs(row, case, dev, step):
    """(batch, rand) of a step on the device; different every step, B = 2 * K."""
    from tests.helpers import to_dev
    batch, rand = host_inputs(row, case, step)
    batch, rand = to_dev(batch, dev), to_dev(rand, dev)
    if row.front == "cached":
        batch = cached_batch(batch, case, dev, row.K)
    return batch, rand


def stepping(states):
    """[("unet" / "text", TrainState)] of the states whose store takes the optimizer step."""
    return [(n, st) for n, st in zip(("unet", "text"), states[:2]) if st.opt_store is not None]


def snapshot(states, out, gen):
    """Clones of everything a step writes: every buffer of every stepping store and its host count; for adapter states the base store's
    bf16 mirror and DoRA's column statistics; the loss and the generator state."""
    torch.cuda.synchronize()
    snap = {}
    for name, st in stepping(states):
        store = st.opt_store
        for b in STATE:
            t = getattr(store, b)
            if t is not None:
                snap[f"{name}.{b}"] = t.clone()
        snap[f"{name}.count"] = torch.tensor([store.count])
        if store._sched is not None and store.optimizer == "lion":  # the device counter that indexes a Lion store's schedule tables
            snap[f"{name}.sched_step"] = store._sched["step"].clone()
        if st.adapter is not None:
            snap[f"{name}.base_w"] = st.store.w.clone()
            if st.adapter.stats is not None:
                snap[f"{name}.stats"] = st.adapter.stats.clone()
    snap["loss"] = out[4]["loss"].clone()
    snap["generator"] = gen.get_state().clone()
    return snap


def assert_snapshots_equal(a, b, what):
    assert sorted(a) == sorted(b), f"{what}: keys {sorted(set(a) ^ set(b))}"
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {k}"
        if x.dtype in kc._INT_VIEW:
            assert_equal_bits(x.reshape(-1).cpu(), y.reshape(-1).cpu(), f"{what}: {k}")
        else:
            assert torch.equal(x, y), f"{what}: {k}"


def gradient_seen(store, K):
    """The float32 gradient in master order that the store's sweep read: the gradient buffers for K = 1; for K > 1 the accumulated buffer,
    which the last accumulate pass has already scaled by float32(1 / K)."""
    if K == 1:
        g = store.grad[: store.total] if store.grad16 is None else torch.cat([store.grad16.float(), store.grad[: store.total - store.g32_base]])
    else:
        assert store.gacc is not None, "micro_batches > 1 never accumulated into this store"
        g = store.gacc[: store.total]
    return g.detach().cpu().numpy().astype(np.float32)


def step(states, batch, rand, gen, K, vae="own"):
    from stable_diffusion_training_amd import training_utils as tu
    us, ts, ue, te, v, sc, _ = states
    return tu.train_step(us, ts, ue, te, batch, gen, v if vae == "own" else vae, sc, strip_bos_eos_token=False, ema_rate=EMA_RATE, rand=rand,
                         micro_batches=K)


def run_eager(row, case, dev, states, steps=STEPS, first=0, after_step=None):
    """`steps` eager steps from step index `first`; a cached row runs without a VAE.  after_step(t, states, out) runs after each, behind
    its snapshot.  Returns the snapshots."""
    gen = torch.Generator(device=dev)
    trace = []
    for t in range(first, first + steps):
        batch, rand = inputs(row, case, dev, t)
        out = step(states, batch, rand, gen, row.K, vae=None if row.front == "cached" else "own")
        trace.append(snapshot(states, out, gen))
        if after_step is not None:
            after_step(t, states, out)
    return trace


def run_graphed(row, case, dev, tc, states, steps=STEPS):
    """The same through dp_compile_all_unique_resolution's shape table with use_graph: two eager calls, then the captured step replayed."""
    from stable_diffusion_training_amd import training_utils as tu
    us, ts, ue, te, vae, sc, _ = states
    vae = None if row.front == "cached" else vae
    table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True, per_device_batch=2, micro_batches=row.K)
    fn = table[(2 * row.K, 3, 512, 512)]
    gen = torch.Generator(device=dev)
    trace = []
    for t in range(steps):
        batch, rand = inputs(row, case, dev, t)
        out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
        trace.append(snapshot(states, out, gen))
    return fn, trace


# ------------------------------------------------------------------------------------------------ the CPU oracle's gradients
def oracle_gradients(row, case, built):
    """[(stepping store, {adapter or weight path: reference gradient})] of step 0 from the CPU oracle on the whole batch: oracle.train_step
    (sd) or test_gpu_sdxl_conditioning.oracle_sdxl_step (sdxl); for adapter rows on the tree with the adapters folded in by the float64
    reference, its kernel gradients pushed through lora_reference.project_ref64 / dora_reference."""
    from tests import test_gpu_dora as td
    from tests import test_gpu_lora as tl
    us, ts = built.states[:2]
    unet_w, clip_w = case["weights"]["unet"], case["weights"]["clip"]
    for st, leaves, key in ((us, built.leaves[0], "unet"), (ts, built.leaves[1], "clip")):
        if st.adapter is not None:
            fold = td._folded64 if st.adapter.cfg.dora else tl._folded64
            folded = fold(st.adapter, case["weights"][key], leaves)
            unet_w, clip_w = (folded, clip_w) if key == "unet" else (unet_w, folded)
    batch, rand = host_inputs(row, case, 0)
    if row.cond == "sd":
        from oracle import train_step as ots
        ref = ots.train_step(unet_w, clip_w, case["weights"]["vae"], case["sched_state"], case["cfgs"], batch, rand, dict(ots.DEFAULT_OPT))
        loss, gu, gt = ref["loss"], ref["unet_grads"], ref["te_grads"]
    else:
        from tests.test_gpu_sdxl_conditioning import oracle_sdxl_step
        loss, gu, gt = oracle_sdxl_step(dict(case, weights=dict(case["weights"], unet=unet_w, clip=clip_w), batch=batch, rand=rand))
    out = []
    for st, leaves, grads, key in ((us, built.leaves[0], gu, "unet"), (ts, built.leaves[1], gt, "clip")):
        if st.opt_store is None:
            continue
        grads = {k: torch.as_tensor(v) for k, v in grads.items()}
        if st.adapter is None:
            out.append((st.opt_store, grads))
        elif st.adapter.cfg.dora:
            out.append((st.opt_store, td._project_tree(st.adapter, grads, case["weights"][key], leaves)))
        else:
            out.append((st.opt_store, tl._project_tree(st.adapter, grads, leaves)))
    return float(loss), out
