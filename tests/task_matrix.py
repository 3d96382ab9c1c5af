"""The second pairwise matrix of train_step options - the features that arrived after tests/step_matrix.py - and the harness its tests
share (DESIGN.md "Task combinations").

Eight axes - optimizer (prodigy, lion8, adamw8, lion32), task (what is trained: an inpainting UNet + text encoder, new tokens, a
ControlNet, an IP-Adapter), front, micro-batches, schedule, conditioning, loss mask, loss type - and 16 rows, one per (optimizer, task)
pair; the six binary axes follow from the two indices by a fixed rule (row_for) under which every pair of values of every two axes meets
in some row (tests/test_task_matrix_cpu.py recomputes that).  The first matrix's helpers are used where they fit (cases, configs,
snapshots, the Lion / AdamW restatement steps); what is new here: the task states and their batches, Prodigy's reference step over the
pieces of a store in sweep order (tests/prodigy_reference.py), the retraction of a token store, the float64 restatement of the loss the
harness differentiates (loss64, loss_operands) and the CPU references of the four tasks.  Nothing here touches a GPU at import."""
import collections
import dataclasses
import itertools
import math

import numpy as np
import torch

from tests import masked_loss_reference as mr
from tests import prodigy_reference as PR
from tests import step_matrix as sm
from tests import token_reference as tr
from tests.kernel_checks import BF, assert_equal_bits

OPTS = ("prodigy", "lion8", "adamw8", "lion32")  # 8: quantize_*_state=True (Prodigy: which gradients are kept in bf16)
TASKS = ("inpaint", "tokens", "controlnet", "ip_adapter")
AXES = collections.OrderedDict(opt=OPTS, task=TASKS, front=("pixels", "cached"), K=(1, 2), sched=("constant", "cosine+ema_warmup"),
                               cond=("sd", "sdxl"), mask=("off", "on"), loss=("l2", "huber"))
Row = collections.namedtuple("Row", tuple(AXES))

# Pairs of axis values that train_step or the state builders refuse by ValueError: (axis, value, axis, value, message regex).  Only a
# row that holds such a pair may be missing from rows(); at this commit every pair of the eight axes is supported (the known refusals -
# an IP-Adapter, a ControlNet and tokens beside one another or on an inpainting UNet - lie between values of the one task axis).
REFUSED = ()
REPLACEMENTS = ()  # hand-added rows that cover again what a dropped row was alone in covering

PIVOTAL = "pivotal_inpaint"  # new tokens beside a UNet LoRA, on the inpainting UNet: the one supported pair of two trained things
ALL_ON = Row("prodigy", PIVOTAL, "cached", 2, "cosine+ema_warmup", "sdxl", "on", "huber")  # no rule forces all of these into one row
STEPS, EMA_RATE, RATE, BUILT_RATE = sm.STEPS, sm.EMA_RATE, sm.RATE, sm.BUILT_RATE
# Prodigy as the runs build it: d0 and the decay of tests/test_gpu_prodigy.py, and d_coef 4.  Measured on the MI355X over the four steps
# of the five Prodigy rows: at d_coef 1 the scheduled ControlNet row (its first step at rate 0) ends at d0 and every other store
# leaves d0 at step 3 only (final d 2.7e-5 .. 5.4e-5); at d_coef 4 every store has left d0 by step 3 (final d 5.7e-5 .. 4.9e-4); at 16
# the final d is 2.3e-4 .. 4.9e-3.  The steps stay four; 4 is the smallest of the three that lifts every row
PRODIGY_OPT = dict(name="prodigy", weight_decay=1e-2, d0=1e-5, d_coef=4.0)
HUBER_C = 0.3
MASK_FLOOR = 0.25
LOSS_WEIGHTS = (0.5, 1.5, 1.0, 2.0)
NUM_TOKENS = 2
SD_SLOTS = ((1, 0), (2, 1), (9, 0), (10, 1), (30, 1), (31, 0))  # (caption position, placeholder): tests/test_gpu_tokens.py's
SDXL_SLOTS = ((1, 0), (2, 1), (5, 0))                           # before every caption's EOS (test_sdxl_mode_one_step_moves_both_towers_leaves)
TOKEN_TABLE = "text_model/embeddings/token_embedding/embedding"
CN_CHANNELS = (16, 16, 32, 32)  # tests/test_gpu_controlnet.py's embedder
IP_EMBED, IP_TOKENS = 64, 4     # tests/test_gpu_ip_adapter.py's adapter
STEPPING = {"inpaint": ("unet", "text"), "tokens": ("text",), "controlnet": ("unet",), "ip_adapter": ("unet",), PIVOTAL: ("unet", "text")}
BATCH_KEYS = {"inpaint": ("inpaint_mask",), "tokens": (), "controlnet": ("conditioning_pixel_values",), "ip_adapter": ("image_embeds",),
              PIVOTAL: ("inpaint_mask",)}


# ------------------------------------------------------------------------------------------------ the matrix
def row_for(o, a):
    """The row of optimizer index o and task index a (0..3).  With o0 / o1 the low and high bit of o and a0 / a1 those of a: the first
    matrix's front = o0^a0, K = 1 + (o1^a1), sched = o0^a1, cond = o1^a0, and mask = o0^o1^a0^a1, loss = o0^o1^a0."""
    o0, o1, a0, a1 = o & 1, o >> 1, a & 1, a >> 1
    return Row(OPTS[o], TASKS[a], AXES["front"][o0 ^ a0], AXES["K"][o1 ^ a1], AXES["sched"][o0 ^ a1], AXES["cond"][o1 ^ a0],
               AXES["mask"][o0 ^ o1 ^ a0 ^ a1], AXES["loss"][o0 ^ o1 ^ a0])


def refused(row):
    """The REFUSED entry a row falls under, or None."""
    for entry in REFUSED:
        if getattr(row, entry[0]) == entry[1] and getattr(row, entry[2]) == entry[3]:
            return entry
    return None


def all_rows():
    return [row_for(o, a) for o in range(4) for a in range(4)]


def rows():
    """The 16 (optimizer, task) rows, less those that hold a refused pair, plus the replacement rows."""
    return [r for r in all_rows() if refused(r) is None] + list(REPLACEMENTS)


def row_id(row):
    return f"{row.opt}-{row.task}-{row.front}-K{row.K}-{row.sched.split('+')[0]}-{row.cond}-mask_{row.mask}-{row.loss}"


def covered_pairs(rs):
    """{(axis, value, axis, value)} over all C(8, 2) axis pairs that some row of rs holds."""
    return {(x, getattr(r, x), y, getattr(r, y)) for r in rs for x, y in itertools.combinations(AXES, 2)}


def all_pairs():
    return {(x, u, y, v) for x, y in itertools.combinations(AXES, 2) for u in AXES[x] for v in AXES[y]}


def documented_hyper(opt, rate):
    """TrainState.hyper as create_lion_optimizer_states documents it.  Prodigy: the rates are NOT USED - lr is the multiplier of d
    (1 unless the dict says otherwise), the decay is the dict's, eps 1e-8, the clip at global norm 1; the others: step_matrix's."""
    if opt == "prodigy":
        return dict(lr=1.0, wd=PRODIGY_OPT["weight_decay"], eps=1e-8, max_norm=1.0)
    return sm.documented_hyper(opt, rate)


def documented_prodigy():
    """ParamStore.prodigy as documented (include/sdt.h "Prodigy"): the defaults with the dict's d0 and d_coef."""
    return dict(b1=0.9, b2=0.999, beta3=math.sqrt(0.999), d0=PRODIGY_OPT["d0"], d_coef=PRODIGY_OPT["d_coef"], growth_rate=float("inf"),
                use_bias_correction=False, safeguard_warmup=False)


def optimizer_name(opt):
    return "prodigy" if opt == "prodigy" else ("adamw" if opt.startswith("adamw") else "lion")


def quantised(opt):
    return opt != "lion32"


def loss_kw(row):
    """The loss keywords of train_step a row sets."""
    kw = {}
    if row.mask == "on":
        kw.update(masked_loss_floor=MASK_FLOOR, normalize_masked_area=True)
    if row.loss == "huber":
        kw.update(loss_type="huber", huber_c=HUBER_C, huber_schedule="snr")
    return kw


def inpainting(row):
    return row.task in ("inpaint", PIVOTAL)


def with_tokens(row):
    return row.task in ("tokens", PIVOTAL)


# ------------------------------------------------------------------------------------------------ the loss, restated in float64
def loss64(pred, target, e, k, c, loss_type):
    """The loss train_step's loss launch forms, as one float64 torch function: (1 / count) sum_b k_b sum_{c,p} e_bp rho(target - pred)
    with rho the square (l2), 2c(sqrt(diff^2 + c^2) - c) (huber) or 2(sqrt(diff^2 + c^2) - c) (smooth_l1), written without the
    cancellation.  pred, target (B,C,h,w); e (B,h,w) the effective mask or None; k (B,) the sample factors or None; c (B,) the
    thresholds (None for l2)."""
    pred, target = pred.to(torch.float64), target.to(torch.float64)
    B, C, h, w = pred.shape
    diff = target - pred
    if loss_type == "l2":
        rho = diff * diff
    else:
        cb = torch.as_tensor(c, dtype=torch.float64).view(B, 1, 1, 1)
        rr_ = diff * diff + cb * cb
        zero = rr_ == 0
        r = torch.sqrt(torch.where(zero, torch.ones_like(rr_), rr_))
        lead = 2.0 * cb if loss_type == "huber" else 2.0
        rho = torch.where(zero, torch.zeros_like(rr_), lead * diff * diff / (r + cb))
    if e is not None:
        rho = rho * torch.as_tensor(e, dtype=torch.float64).view(B, 1, h, w)
    if k is not None:
        rho = rho * torch.as_tensor(k, dtype=torch.float64).view(B, 1, 1, 1)
    return rho.sum() / (B * C * h * w)


def loss_operands(batch, timesteps, alphas_cumprod, latent_hw, *, floor=0.0, normalize=False, loss_type="l2", huber_c=HUBER_C,
                  huber_schedule="snr"):
    """(e, k, c) of a host batch as loss64 takes them, float64: e (B,h,w) the loss_mask clamped to [0, 1], pooled to the latent grid by
    block means and floored (None without a mask); k (B,) = loss_weight * (h w / sum e, 0 for an empty sample, when normalising) (None
    with neither); c (B,) the snr / exponential / constant threshold of each sample's timestep, rounded to float32 as the step's table
    holds it (None for l2)."""
    h, w = latent_hw
    mask, lw = batch.get("loss_mask"), batch.get("loss_weight")
    e = k = c = None
    if mask is not None:
        B, H, W = mask.shape
        f = H // h
        assert (H, W) == (h * f, w * f)
        m = torch.nan_to_num(mask.to(torch.float64), nan=0.0).clamp(0.0, 1.0)
        e = m.view(B, h, f, w, f).sum((2, 4)) / (f * f)
        e = torch.maximum(e, torch.tensor(float(floor), dtype=torch.float64))
    if lw is not None or (normalize and e is not None):
        B = (mask if mask is not None else lw).shape[0]
        k = torch.ones(B, dtype=torch.float64) if lw is None else lw.to(torch.float64).clone()
        if normalize:
            S = e.reshape(B, -1).sum(1)
            k = k * torch.where(S == 0, torch.zeros_like(S), float(h * w) / torch.where(S == 0, torch.ones_like(S), S))
    if loss_type != "l2":
        ac = torch.as_tensor(np.asarray(alphas_cumprod), dtype=torch.float64)[torch.as_tensor(timesteps).long()]
        if huber_schedule == "constant":
            c = torch.full_like(ac, float(huber_c))
        elif huber_schedule == "exponential":
            c = torch.exp(torch.as_tensor(timesteps).to(torch.float64) * (math.log(huber_c) / len(alphas_cumprod)))
        else:
            sigma = torch.sqrt((1.0 - ac) / ac)
            c = (1.0 - huber_c) / (1.0 + sigma) ** 2 + huber_c
        c = c.to(torch.float32).to(torch.float64)
    return e, k, c


# ------------------------------------------------------------------------------------------------ cases
_CASES = {}


def _loss_mask(B, image):
    """A pixel-size loss mask of masked_loss_reference.MASK_VALUES (dyadic: every block mean is exact in float32 at any scale), another
    region per sample with edges that are no multiples of 8: 0 < mean < 1 in every sample, fractional block means inside and at the
    edges, zeros (floored) outside."""
    m = mr.seeded_mask((B, image, image), 41)
    for b in range(B):
        m[b, : 12 + 6 * b, :] = 0.0
        m[b, :, image - 10 - 4 * b:] = 0.0
    return m.contiguous()


def case_for(row):
    """The host case of a row: step_matrix's case of its (cond, K) with the task's weights, configs and batch entries, built once per
    (task, cond, K, mask) and never written to."""
    key = (row.task, row.cond, row.K, row.mask)
    if key in _CASES:
        return _CASES[key]
    from stable_diffusion_training_amd import nets
    base = sm.case_for(row)
    B, image = 2 * row.K, 64
    case = dict(base, cfgs=dict(base["cfgs"]), weights=dict(base["weights"]), batch=dict(base["batch"]), rand=dict(base["rand"]))
    if inpainting(row):
        from tests.test_gpu_inpaint import _rect_masks
        wide, cfg9 = nets.widen_conv_in(base["weights"]["unet"], base["cfgs"]["unet"], 9)
        kern = wide["conv_in/kernel"]
        kern[:, :, 4:] = torch.randn(3, 3, 5, kern.shape[3], generator=torch.Generator().manual_seed(77)) / 9.0
        case["cfgs"]["unet"], case["weights"]["unet"] = cfg9, wide
        case["batch"]["inpaint_mask"] = _rect_masks(B, image, image, 5)
        case["rand"]["masked_posterior_eps"] = torch.randn(B, image // 8, image // 8, 4, generator=torch.Generator().manual_seed(78))
    if with_tokens(row):
        ids = case["batch"]["input_ids"].clone()
        clip = case["cfgs"]["clip"]
        if "towers" in clip:
            for i, t in enumerate(clip["towers"]):
                for pos, j in SDXL_SLOTS:
                    ids[:, i, pos] = t["vocab_size"] + j
        else:
            for pos, j in SD_SLOTS:
                ids[..., pos] = clip["vocab_size"] + j
        case["batch"]["input_ids"] = ids
    if row.task == "controlnet":
        from tests import controlnet_reference as cr
        case["cn_cfg"] = nets.controlnet_config(case["cfgs"]["unet"], CN_CHANNELS)
        case["cn_weights"] = cr.random_controlnet(case["weights"]["unet"], case["cn_cfg"], seed=6)
        case["batch"]["conditioning_pixel_values"] = torch.rand(B, 3, image, image, generator=torch.Generator().manual_seed(21))
    if row.task == "ip_adapter":
        case["ip_cfg"] = nets.ip_adapter_config(case["cfgs"]["unet"], IP_EMBED, IP_TOKENS)
        case["ip_weights"] = nets.init_params(nets.ip_adapter_spec(case["ip_cfg"]), 6)
        case["batch"]["image_embeds"] = torch.randn(B, IP_EMBED, generator=torch.Generator().manual_seed(21))
    if row.mask == "on":
        case["batch"]["loss_mask"] = _loss_mask(B, image)
        case["batch"]["loss_weight"] = torch.tensor(LOSS_WEIGHTS[:B])
    _CASES[key] = case
    return case


def training_config(row, case):
    """step_matrix's config with the row's quantisation switches (on for Prodigy: they decide which gradients are kept in bf16)."""
    tc = sm.training_config(row, case)
    return dataclasses.replace(tc, quantize_unet_state=quantised(row.opt), quantize_text_encoder_state=quantised(row.opt))


def state_kwargs(row, case):
    """The keywords of on_device_model_training_state / create_lion_optimizer_states a row sets."""
    from stable_diffusion_training_amd import lora, tokens
    sched = row.sched != "constant"
    kw = dict(optimizer=dict(PRODIGY_OPT) if row.opt == "prodigy" else optimizer_name(row.opt),
              lr_schedule=dict(sm.LR_SCHEDULE) if sched else None, ema_schedule=dict(sm.EMA_SCHEDULE) if sched else None)
    if with_tokens(row):
        kw["new_tokens"] = tokens.TokenConfig(NUM_TOKENS, seed=4, retract=True)
    if row.task == PIVOTAL:
        kw["lora"] = dict(unet=lora.LoraConfig(sm.RANK, sm.ALPHA, seed=1), text_encoder="frozen")
    if row.task == "controlnet":
        kw["controlnet"] = dict(config=case["cn_cfg"], params=case["cn_weights"])
    if row.task == "ip_adapter":
        kw["ip_adapter"] = dict(config=case["ip_cfg"], params=case["ip_weights"])
    return kw


def stepping(states):
    """[("unet" / "text", TrainState)] of the states whose opt_store takes the optimizer step."""
    return sm.stepping(states)


def raise_rates(row, states):
    """Hold the wiring of the builder: the stepping stores are the task's own, every other state is frozen with an empty hyper, the
    stepping states carry the documented hyper-parameters (built with the reference's 1e-6; Prodigy: no rate at all) and, in a
    scheduled row, the cosine / EMA-warmup schedule over the store's own base rate.  Then raise Lion's and AdamW's rate to RATE as
    step_matrix.raise_rates does.  Returns {"unet" / "text": (LRSchedule, EMASchedule) or None} of the stepping stores."""
    from stable_diffusion_training_amd import lr_schedule as L
    out = {}
    names = tuple(n for n, _ in stepping(states))
    assert names == STEPPING[row.task], f"{row.task}: the stepping states are {names}, expected {STEPPING[row.task]}"
    for name, st in zip(("unet", "text"), states[:2]):
        store = st.opt_store
        if store is None:
            assert st.hyper == {}, f"{name}: a frozen state carries hyper-parameters {st.hyper}"
            assert not st.store.trainable
            continue
        built = documented_hyper(row.opt, BUILT_RATE)
        assert st.hyper == built, f"{name}: built with {st.hyper}, documented {built}"
        assert store.optimizer == optimizer_name(row.opt)
        if row.opt == "prodigy":
            assert store.prodigy == documented_prodigy(), f"{name}: Prodigy settings {store.prodigy}, documented {documented_prodigy()}"
        st.hyper["lr"] = documented_hyper(row.opt, RATE)["lr"]
        out[name] = None
        if row.sched != "constant":
            lrs, emas = store.schedule
            assert (lrs.name, lrs.base_lr, lrs.num_warmup_steps, lrs.num_training_steps) == ("cosine", built["lr"], 1, 6)
            assert (emas.kind, emas.ema_rate) == ("warmup", EMA_RATE)
            if st.hyper["lr"] != built["lr"]:
                store.set_schedule(lr=L.LRSchedule("cosine", st.hyper["lr"], **sm.LR_SCHEDULE), ema=emas)
            out[name] = store.schedule
        else:
            assert store.schedule is None
    return out


def task_store(row, states, name):
    """The store of the state `name` that the row's task trains (the identity the builder must have wired)."""
    st = states[0] if name == "unet" else states[1]
    if row.task == "controlnet":
        return st.controlnet.store
    if row.task == "ip_adapter":
        return st.ip_adapter.store
    if with_tokens(row) and name == "text":
        return st.tokens.store
    if row.task == PIVOTAL:
        return st.adapter.store
    return st.store


def check_flags(row, tc, states):
    """The masks of the stepping stores follow the config's exclusion lists (a token store also excludes new_tokens from
    quantisation: tokens.attach); a Prodigy store keeps float32 state whatever the switches say."""
    quant = quantised(row.opt)
    for name, st in stepping(states):
        store = st.opt_store
        assert store is task_store(row, states, name), f"{name}: the stepping store is not the task's own"
        wd_ex = list(tc.excluded_layer_pattern_from_weight_decay)
        q_ex = list(tc.excluded_layer_from_quantization) + (["new_tokens"] if st.tokens is not None and store is st.tokens.store else [])
        for path, lf in store.leaves.items():
            comps = path.split("/")
            assert lf.decayed == (not any(e in comps for e in wd_ex)), f"{path}: decayed {lf.decayed}"
            assert lf.quantised == (quant and not any(e in comps for e in q_ex)), f"{path}: quantised {lf.quantised}"
        if row.opt == "prodigy":
            assert store.codes is None and store.codes2 is None and store.mom.dtype == torch.float32 and store.mom.numel() >= store.total
            assert store.prodigy_s.numel() >= store.total and store.prodigy_p0.numel() >= store.total
        else:
            assert (store.quant_total > 0) == (quant and any(lf.quantised for lf in store.leaves.values()))
            assert (store.codes2 is not None) == row.opt.startswith("adamw") and store.prodigy_state is None
        assert store.ema is not None, f"{name}: no EMA"


@dataclasses.dataclass
class Built:
    tc: object
    states: tuple
    schedules: dict
    lora_leaves: object   # the UNet adapter's loaded leaves (pivotal tuning), or None
    token_rows: object    # {new_tokens path: host rows} as loaded (rows with tokens), or None


def build(row, case, dev, seed=31):
    """(tc, states) of a row through on_device_model_training_state, EMA on for both models, the wiring held and the rates raised
    (raise_rates), random LoRA factors and random token rows loaded from `seed`.  The rest travels on build.last (a Built)."""
    from stable_diffusion_training_amd import training_utils as tu
    tc = training_config(row, case)
    states = tu.on_device_model_training_state(tc, sm.models_of(case), device=dev, **state_kwargs(row, case))
    schedules = raise_rates(row, states)
    lora_leaves = token_rows = None
    if row.task == PIVOTAL:
        from tests.test_gpu_lora import _random_factors
        lora_leaves = _random_factors(states[0].adapter, case["weights"]["unet"], seed)
        states[0].adapter.store.load(lora_leaves)
    if with_tokens(row):
        tk = states[1].tokens
        g = torch.Generator().manual_seed(seed + 1)
        token_rows = {p: torch.randn(tk.store.leaves[p].shape, generator=g) * float(tk.target_std[i]) for i, p in enumerate(tk.store.order)}
        tk.store.load(token_rows)
    build.last = Built(tc, states, schedules, lora_leaves, token_rows)
    return tc, states


# ------------------------------------------------------------------------------------------------ inputs
def host_inputs(row, case, step):
    """(batch, rand) of a step on the host, different every step: the pixels shifted by 0.05 * step, the conditioning image shifted
    and wrapped, the loss mask rolled; draws that keep half of their direction (sqrt(3/4) of the case's draw + 1/2 of a fresh one) and
    timesteps that move by 50 a step - gradients that keep some direction are what lets Prodigy's d leave d0 within four steps."""
    g = torch.Generator().manual_seed(100 + step)
    batch = dict(case["batch"])
    batch["pixel_values"] = (batch["pixel_values"] + 0.05 * step).contiguous()
    if "conditioning_pixel_values" in batch:
        batch["conditioning_pixel_values"] = ((batch["conditioning_pixel_values"] + 0.1 * step) % 1.0).contiguous()
    if "loss_mask" in batch:
        batch["loss_mask"] = torch.roll(batch["loss_mask"], shifts=5 * step, dims=2).contiguous()
    rand = {}
    for k, v in case["rand"].items():
        if v.is_floating_point():
            rand[k] = (math.sqrt(0.75) * v + 0.5 * torch.randn(v.shape, generator=g)).contiguous()
        else:
            rand[k] = ((v + 50 * step) % 1000).to(v.dtype)
    return batch, rand


def pooled_host(mask, f=8):
    """The block means of a dyadic host mask, exact in float32 (asserted): what a cached batch carries at latent size."""
    B, H, W = mask.shape
    m = mask.to(torch.float64).clamp(0.0, 1.0).view(B, H // f, f, W // f, f)
    s = m.sum((2, 4))
    assert bool((s * 4 == (s * 4).round()).all()), "the mask's block sums are no multiples of 1/4: the pooled mask would not be exact"
    return (s / (f * f)).to(torch.float32).contiguous()


def cached_batch(batch, case, dev, micro_batches):
    """The device batch with latent_moments in place of its pixels (encode_latent_moments / encode_inpaint_moments at the micro-batch
    composition), masks at latent size: the inpaint mask as the encoder pooled it, the loss mask as its exact block means."""
    from stable_diffusion_training_amd import training_utils as tu
    vae, px = sm._frozen_vae(case, dev), batch["pixel_values"]
    n = px.shape[0] // micro_batches
    parts = [slice(k * n, (k + 1) * n) for k in range(micro_batches)]
    out = {k: v for k, v in batch.items() if k not in ("pixel_values", "inpaint_mask", "loss_mask")}
    if "inpaint_mask" in batch:
        enc = [tu.encode_inpaint_moments(vae, px[s].contiguous(), batch["inpaint_mask"][s].contiguous()) for s in parts]
        out["latent_moments"] = torch.cat([e[0] for e in enc]).contiguous()
        out["masked_latent_moments"] = torch.cat([e[1] for e in enc]).contiguous()
        out["inpaint_mask"] = torch.cat([e[2] for e in enc]).contiguous()
    else:
        out["latent_moments"] = torch.cat([tu.encode_latent_moments(vae, px[s].contiguous()) for s in parts]).contiguous()
    if "loss_mask" in batch:
        out["loss_mask"] = pooled_host(batch["loss_mask"].cpu()).to(dev)
    return out


def device_inputs(row, case, dev, batch, rand, K):
    from tests.helpers import to_dev
    batch, rand = to_dev(batch, dev), to_dev(rand, dev)
    if row.front == "cached":
        batch = cached_batch(batch, case, dev, K)
    return batch, rand


def inputs(row, case, dev, step):
    """(batch, rand) of a step on the device; B = 2 * K."""
    return device_inputs(row, case, dev, *host_inputs(row, case, step), row.K)


# ------------------------------------------------------------------------------------------------ steps and snapshots
def step(row, states, batch, rand, gen, K, **extra):
    from stable_diffusion_training_amd import training_utils as tu
    us, ts, ue, te, vae, sc, _ = states
    vae = None if "latent_moments" in batch else vae
    return tu.train_step(us, ts, ue, te, batch, gen, vae, sc, strip_bos_eos_token=False, ema_rate=EMA_RATE, rand=rand, micro_batches=K,
                         **loss_kw(row), **extra)


def snapshot(row, states, out, gen):
    """step_matrix.snapshot (every buffer of every stepping store - Prodigy's m, v, s, p0, state block, counter and scalar block among
    them - the host counts, a Lion store's schedule counter, an adapter's merged mirror, the loss, the generator state) plus the loss
    per sample and a token store's retraction record."""
    snap = sm.snapshot(states, out, gen)
    if row.mask == "on" or row.loss != "l2":
        snap["loss_per_sample"] = out[4]["loss_per_sample"].clone()
    else:
        assert "loss_per_sample" not in out[4]
    if with_tokens(row):
        snap["text.retract_stats"] = states[1].tokens.stats.clone()
    return snap


def frozen_record(states):
    """[(what, tensor or count)] of every frozen store: master, step count and - unless an adapter's merge rewrites it - the mirror."""
    torch.cuda.synchronize()
    rec = []
    for name, st in zip(("unet", "text"), states[:2]):
        if not st.store.trainable:
            rec.append((f"{name} master", st.store.master.clone()))
            rec.append((f"{name} count", st.store.count))
            if st.adapter is None:
                rec.append((f"{name} mirror", st.store.w.clone()))
    return rec


def assert_frozen_unchanged(before, states):
    for (what, a), (_, b) in zip(before, frozen_record(states)):
        same = a == b if isinstance(a, int) else (torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == BF else torch.equal(a, b))
        assert same, f"a frozen store changed: {what}"


def run_eager(row, case, dev, states, steps=STEPS, first=0, after_step=None):
    """`steps` eager steps from step index `first`.  after_step(t, states, out) runs after each, behind its snapshot."""
    gen = torch.Generator(device=dev)
    trace = []
    for t in range(first, first + steps):
        batch, rand = inputs(row, case, dev, t)
        out = step(row, states, batch, rand, gen, row.K)
        trace.append(snapshot(row, states, out, gen))
        if after_step is not None:
            after_step(t, states, out)
    return trace


def graphed_table(row, tc, states):
    from stable_diffusion_training_amd import training_utils as tu
    us, ts, ue, te, vae, sc, _ = states
    vae = None if row.front == "cached" else vae
    table = tu.dp_compile_all_unique_resolution(us, ts, ue, te, vae, sc, tc, use_graph=True, per_device_batch=2, micro_batches=row.K,
                                                step_overrides=loss_kw(row))
    return table[(2 * row.K, 3, 512, 512)], vae


def run_graphed(row, case, dev, tc, states, steps=STEPS):
    """The same through dp_compile_all_unique_resolution's shape table with use_graph and the row's loss options as step_overrides:
    two eager calls, then the captured step replayed.  Returns (the table's callable, the snapshots, the last batch and draws)."""
    us, ts, ue, te, _, sc, _ = states
    fn, vae = graphed_table(row, tc, states)
    gen = torch.Generator(device=dev)
    trace = []
    for t in range(steps):
        batch, rand = inputs(row, case, dev, t)
        out = fn(us, ts, ue, te, batch, gen, vae, sc, rand=rand)
        trace.append(snapshot(row, states, out, gen))
    return fn, trace, (batch, rand, gen, vae)


# ------------------------------------------------------------------------------------------------ Prodigy's reference step
def moments_ranges(st, from_acc):
    """The element ranges of the moments sweep's launches, in sweep order (optimizers.Prodigy.step): one launch per run of neighbouring
    non-empty pieces that read their gradient from the same buffer - the bf16 gradients of the quantised segments and the float32
    rest, or the one accumulated buffer."""
    bf16 = st.grad16 is not None and not from_acc
    runs = []
    for quant, _, a, b in st.segments:
        if b == a:
            continue
        key = bool(quant and bf16)
        if runs and runs[-1][1] == a and runs[-1][2] == key:
            runs[-1][1] = b
        else:
            runs.append([a, b, key])
    return [(a, b) for a, b, _ in runs]


def prodigy_reference_state(st):
    """Flat host copies of a Prodigy store as it stands (master order, alignment gaps included: the two sums run over them) and the
    device state as prodigy_reference's dict."""
    host = lambda t: t.detach().reshape(-1).cpu().numpy().copy()
    blk = st.prodigy_state.cpu().numpy()
    state = dict(d=float(blk[0]), d_max=float(blk[1]), numer=float(blk[2]), P1=float(blk[3]), P2=float(blk[4]), dot=float(blk[5]),
                 l1=float(blk[6]), q=float(blk[7]), lr_t=float(blk[8]), t=int(st.prodigy_step.item()))
    n = st.total
    return dict(p=host(st.master)[:n], ema=None if st.ema is None else host(st.ema)[:n], m=host(st.mom)[:n], v=host(st.mom2)[:n],
                s=host(st.prodigy_s)[:n], p0=host(st.prodigy_p0)[:n], st=state, t=int(st.count), prodigy=True)


def prodigy_reference_step(st, ref, g_flat, hp, ema_rate, schedule=None, from_acc=False):
    """One step of the Prodigy store `st` restated on ref (prodigy_reference_state) by tests/prodigy_reference.py run over the store's
    pieces in sweep order: select; one moments launch per gradient buffer, the two sums carried across the launches in double;
    finish; the apply sweep with each piece's own decay; the EMA.  hp: the DOCUMENTED hyper-parameters; the store's settings must be
    the documented ones.  Returns the scalar block the store must hold."""
    g_flat = np.asarray(g_flat, np.float32)
    assert st.prodigy == documented_prodigy(), f"the store carries {st.prodigy}, documented {documented_prodigy()}"
    php = PR.hyper(lr=hp["lr"], eps=hp["eps"], weight_decay=hp["wd"], **documented_prodigy())
    er = ema_rate if ref["ema"] is not None else 0.0
    kw = {} if schedule is None else dict(lr_tab=schedule[0].table(), ema_tab=schedule[1].table())
    cur = PR.select(ref["st"], php, ema_rate=er, **kw)
    sq = float(np.sum(g_flat.astype(np.float64) ** 2))
    for a, b in moments_ranges(st, from_acc):
        sl = slice(a, b)
        ref["p0"][sl], ref["m"][sl], ref["v"][sl], ref["s"][sl] = PR.moments(ref["p"][sl], g_flat[sl], ref["p0"][sl], ref["m"][sl], ref["v"][sl],
                                                                            ref["s"][sl], cur, php, ref["st"], max_norm=hp["max_norm"], sq=sq)
    PR.finish(ref["st"], php, cur)
    for _, decayed, a, b in st.segments:
        if b > a:
            ref["p"][a:b] = PR.apply(ref["p"][a:b], ref["m"][a:b], ref["v"][a:b], cur, hp["wd"] if decayed else 0.0)
    if ref["ema"] is not None:
        ref["ema"] = PR.ema_update(ref["ema"], ref["p"], cur)
    ref["t"] += 1
    return cur


def prodigy_check_store(st, ref, cur, tag, mirror_of=None):
    """Every leaf of master, EMA, bf16 mirror, m, v, s and p0, the ten-double state block, the scalar block and the counters, in every
    bit."""
    flats = dict(master=ref["p"], ema=ref["ema"], mom=ref["m"], mom2=ref["v"], prodigy_s=ref["s"], prodigy_p0=ref["p0"])
    for path, lf in st.leaves.items():
        sl = slice(lf.offset, lf.offset + lf.numel)
        for name, want in flats.items():
            if want is not None:
                assert_equal_bits(getattr(st, name)[sl].cpu(), torch.from_numpy(want[sl]), f"{tag}: {path} {name}")
        mirrored = ref["p"][sl] if mirror_of is None else mirror_of[path]
        assert_equal_bits(st.w[sl].cpu(), torch.from_numpy(np.ascontiguousarray(mirrored)).to(BF), f"{tag}: {path} bf16 mirror")
    assert_equal_bits(st.prodigy_cur.cpu(), torch.from_numpy(cur), f"{tag}: scalar block")
    assert_equal_bits(st.prodigy_state.cpu(), torch.from_numpy(PR.state_block(ref["st"])), f"{tag}: state block (d, d_max, numer, sums)")
    assert int(st.prodigy_step.item()) == st.count == ref["t"] == ref["st"]["t"], f"{tag}: step counts {int(st.prodigy_step.item())}, {st.count}, {ref['t']}"


def reference_state(st):
    return prodigy_reference_state(st) if st.optimizer == "prodigy" else sm.reference_state(st)


def leaf_of(ref, st, path):
    lf = st.leaves[path]
    return ref["p"][lf.offset: lf.offset + lf.numel] if ref.get("prodigy") else ref["p"][path]


def set_leaf(ref, st, path, value):
    lf = st.leaves[path]
    if ref.get("prodigy"):
        ref["p"][lf.offset: lf.offset + lf.numel] = value
    else:
        ref["p"][path] = value


def restate_and_check(row, state, ref, g_flat, schedule, tag):
    """One optimizer step of the state's stepping store restated on ref from the gradient the sweep read - with the documented
    hyper-parameters and the schedule's table entry of the step - and the store held to it in every bit.  A token store that retracts:
    the sweep's value is what the EMA and the mirror saw; the master is that value times the factor the device published, which must
    be float32(pow) of the restated rows' statistics within 2 ulp (the device pow's 1 ulp of tests/test_gpu_token_kernels.py plus the
    rounding of its own standard deviation)."""
    store = state.opt_store
    hp = documented_hyper(row.opt, RATE)
    if store.optimizer == "prodigy":
        cur = prodigy_reference_step(store, ref, g_flat, hp, EMA_RATE, schedule, from_acc=row.K > 1)
    else:
        cur = sm.reference_store_step(store, ref, g_flat, hp, EMA_RATE, schedule)
    mirror_of = None
    tk = state.tokens
    if tk is not None and store is tk.store and tk.cfg.retract:
        mirror_of = {p: leaf_of(ref, store, p).copy() for p in store.leaves}
        stats = tk.stats.cpu().numpy()
        for i, tp in enumerate(tk.tok_paths):
            path = tk.new_paths[tp]
            x = mirror_of[path]
            _, std = tr.retract_stats(x)
            want = tr.retract_factor(std, tk.target_std[i], tk.cfg.retract_power)
            factor = float(stats[i, 2])
            ulp = float(np.spacing(np.float32(want)))
            assert np.float32(factor) == factor and abs(factor - float(want)) <= 2 * ulp, f"{tag}: retraction factor {factor!r}, restated {float(want)!r}"
            set_leaf(ref, store, path, tr.retract_apply(x, factor))
    if store.optimizer == "prodigy":
        prodigy_check_store(store, ref, cur, tag, mirror_of)
    else:
        sm.check_store(store, ref, cur, tag, mirror_of)
    return cur


# ------------------------------------------------------------------------------------------------ the CPU references of the tasks
def cpu_front(row, case, batch, rand):
    """What the step's front hands the UNet, wholly on the CPU from the oracle's VAE: dict(noisy (B,4,h,w) float32, unet_input
    (B,4 or 9,h,w), target, lmask, masked_latents) for a host batch and its draws (epsilon target)."""
    from oracle import nets as onets
    from oracle import schedulers as osched
    from tests import inpaint_reference as ir
    w, cfgs = case["weights"], case["cfgs"]
    t = rand["timesteps"].numpy()
    with torch.no_grad():
        px = batch["pixel_values"]
        latents = onets.vae_sample_latents(onets.vae_encode_moments(w["vae"], cfgs["vae"], px), rand["posterior_eps"]).contiguous()
        noisy = torch.from_numpy(osched.add_noise(case["sched_state"], latents.numpy(), rand["noise"].numpy(), t))
        out = dict(noisy=noisy, unet_input=noisy, target=rand["noise"])
        if "inpaint_mask" in batch:
            mask = batch["inpaint_mask"].numpy()
            lmask = torch.from_numpy(ir.latent_mask(mask, 8)).to(torch.float32)
            mpx = torch.from_numpy(ir.masked_image(px.numpy(), mask))
            mlat = onets.vae_sample_latents(onets.vae_encode_moments(w["vae"], cfgs["vae"], mpx), rand["masked_posterior_eps"]).contiguous()
            out.update(lmask=lmask, masked_latents=mlat, unet_input=torch.cat([noisy, lmask[:, None], mlat], 1))
    return out


def text_conditioning(case, clip_w, ids, B):
    """(ctx, added) of the oracle's text encoder on the weights clip_w: SD's last hidden state, or SDXL's two towers with the pooled
    embedding and the batch's time_ids."""
    from oracle import nets as onets
    clip = case["cfgs"]["clip"]
    if "towers" in clip:
        from tests.test_gpu_sdxl_conditioning import oracle_sdxl_text
        ctx, pooled = oracle_sdxl_text(clip_w, clip, ids)
        return ctx, dict(text_embeds=pooled, time_ids=case["batch"]["time_ids"])
    return onets.assemble_context(onets.clip_text_forward(clip_w, clip, ids), B, False), None


def token_tables(case, clip_w, rows):
    """clip_w with every tower's token table continued by its trained rows (rows: {new_tokens path: (n, D) tensor})."""
    out = dict(clip_w)
    for path, r in rows.items():
        tab = path[: -len("new_tokens")] + "embedding"
        assert tab in out and tab.endswith(TOKEN_TABLE)
        out[tab] = torch.cat([clip_w[tab], r])
    return out


def task_prediction(row, case, built, x, t, batch, ctx_tap=None, embeds_tap=None):
    """The prediction of the row's networks on the CPU under autograd, whatever depends on a trained leaf recomputed from it.  x: the
    UNet's input (the values the device fed it); ctx_tap / embeds_tap: the frozen text encoder's output where no trained leaf reaches
    it.  Returns (pred (B,4,h,w), [(state name, {path: leaf})] the trained leaves in the order of the stepping states)."""
    from oracle import nets as onets
    w, cfgs = case["weights"], case["cfgs"]
    B = x.shape[0]
    ids = batch["input_ids"]
    q = lambda v: v.to(BF).float()
    leaf = lambda d: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    if row.task == "inpaint":
        up, tp = leaf(w["unet"]), leaf(w["clip"])
        ctx, added = text_conditioning(case, tp, ids, B)
        return onets.unet_forward(up, cfgs["unet"], x, t, ctx, added), [("unet", up), ("text", tp)]
    if row.task == "tokens":
        rows_ = leaf(built.token_rows)
        ctx, added = text_conditioning(case, token_tables(case, w["clip"], rows_), ids, B)
        return onets.unet_forward(w["unet"], cfgs["unet"], x, t, ctx, added), [("text", rows_)]
    added = None if embeds_tap is None else dict(text_embeds=embeds_tap, time_ids=batch["time_ids"])
    if row.task == "controlnet":
        from tests import controlnet_reference as cr
        wl = leaf(case["cn_weights"])
        down, mid = cr.controlnet_forward(wl, case["cn_cfg"], x, t, ctx_tap, q(batch["conditioning_pixel_values"]), added)
        return cr.unet_forward(w["unet"], cfgs["unet"], x, t, ctx_tap, added, down=down, mid=mid), [("unet", wl)]
    if row.task == "ip_adapter":
        from tests import ip_adapter_reference as R
        wl = leaf(case["ip_weights"])
        with R.with_image_tokens(wl, R.image_tokens(wl, case["ip_cfg"], q(batch["image_embeds"]))):
            return onets.unet_forward(w["unet"], cfgs["unet"], x, t, ctx_tap, added), [("unet", wl)]
    raise ValueError(row.task)
