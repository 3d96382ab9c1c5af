"""MI355X-native drop-in for the reference's train-step assembly layer (reference training_utils.py).

Same public names and argument meaning as the reference for the hot path only:
  TrainingConfig (:52-113), create_mask (:116-131), calculate_resolution_array (:134-174), FrozenModel (:40-49),
  create_lion_optimizer_states (:281-427), on_device_model_training_state (:430-501), train_step (:504-762),
  dp_compile_all_unique_resolution (:765-983).
What differs by design: there is no XLA program to compile - kernels are shape-generic - so the "compiled" table
maps pixel_values.shape -> a bound step callable; data parallelism is one process per GPU with a bucketed RCCL
all-reduce of the flat gradient buffer overlapped with backward (dp.GradReducer) instead of GSPMD; parameters,
optimizer state and EMA live in flat HBM buffers (params.ParamStore) updated in place (the reference donates them).
"""
import math
from dataclasses import dataclass, field
from typing import Any, Callable

import numpy as np
import torch

from . import _lib, lora as lora_mod, nets, ops, optimizers, tokens as tokens_mod, trace
from .checkpoint import flatten_if_nested, load_models, load_training_state, save_model, save_training_state  # noqa: F401  (reference names)
from .lr_schedule import resolve as resolve_schedule
from .params import EmaView, ParamStore, create_mask  # noqa: F401  (create_mask re-exported, reference name)
from .schedulers import _PTYPE, DDPMScheduler


@dataclass
class TrainingConfig:
    """The 28 keys of model_properties.json that the reference's TrainingConfig consumes (training_utils.py:86-113)."""
    model_path: str
    batch_size: int
    learning_rate: float
    unet_learning_rate: float
    text_encoder_learning_rate: float
    lr_scheduler: str
    adam_to_lion_scale_factor: float
    compilation_cache_path: str
    keep_compiled_fn_in_cache: bool
    text_encoder_context_window: int
    context_window_concatenation_count: int
    aot_compile: bool
    strip_bos_eos_token: bool
    offset_noise_magnitude: float
    min_snr_gamma_magnitude: float
    perturbation_noise_magnitude: float
    image_area_root: list
    minimum_axis_length: list
    beta_scheduler: str
    prediction_type: str
    excluded_layer_pattern_from_weight_decay: list
    excluded_layer_from_quantization: list
    quant_block_size: int
    quantize_unet_state: bool
    quantize_text_encoder_state: bool
    accumulate_unet_ema: bool
    accumulate_text_encoder_ema: bool
    ema_rate: float

    @classmethod
    def from_dict(cls, config_dict):
        """training.py:38-40: pick the dataclass fields by name out of the full JSON dict."""
        return cls(**{k: config_dict[k] for k in cls.__dataclass_fields__})


def calculate_resolution_array(max_res_area=512 ** 2, bucket_lower_bound_res=256, rounding=64):
    """Aspect-ratio buckets (width, height) with area <= max_res_area, both sides multiples of `rounding`,
    minor axis >= bucket_lower_bound_res; mirrored around the square (training_utils.py:134-174)."""
    centroid = int(max_res_area ** 0.5)
    lo = bucket_lower_bound_res // rounding * rounding
    hi = centroid // rounding * rounding
    minor = np.arange(lo, hi + rounding, rounding)
    major = ((max_res_area / minor) // rounding * rounding).astype(int)
    n = len(minor) - 1 if minor[-1] == major[-1] else len(minor)  # do not repeat the square bucket
    w = np.concatenate([minor, major[:n][::-1]])
    h = np.concatenate([major, minor[:n][::-1]])
    return np.stack([w, h]).T


@dataclass
class FrozenModel:
    """(callable/config, params) bundle for the frozen VAE and the scheduler (training_utils.py:40-49)."""
    call: Any
    params: Any


@dataclass
class TrainState:
    """Stand-in for flax TrainState (training_utils.py:383-387): apply_fn + params + optimizer, all in `store`.
    LoRA (lora=): `store` stays the network's - frozen - weight store, `adapter` is the lora.LoraAdapter whose own store holds the trained
    leaves and takes the optimizer step (None with an empty hyper: a frozen text encoder that only runs its forward).
    New tokens (new_tokens=): the text state's `tokens` is the tokens.TokenAdapter hung on its frozen store; its store of trained rows
    takes the optimizer step.
    Side networks (controlnet=, ip_adapter=; nets.SIDE_NETWORKS): the UNet state's `controlnet` is the nets.ControlNet, its `ip_adapter`
    the nets.IPAdapter (store + config) trained on the frozen UNet; that store takes the optimizer step."""
    apply_fn: Callable
    store: ParamStore
    config: dict
    hyper: dict = field(default_factory=dict)
    adapter: Any = None
    tokens: Any = None
    controlnet: Any = None
    ip_adapter: Any = None

    @staticmethod
    def stepping_of(state):
        """(the store that takes the optimizer step, the LoRA adapter if it is the adapter's store) of a state - or of a stand-in that
        lacks some of the fields, or of a bare store.  The one place that knows the precedence: a side network's store, the adapter's,
        the token store, the weight store itself, or None (frozen, with nothing hung on it)."""
        for net in nets.SIDE_NETWORKS:
            side = getattr(state, net.name, None)
            if side is not None:
                return side.store, None
        adapter, toks = getattr(state, "adapter", None), getattr(state, "tokens", None)
        if adapter is not None:
            return adapter.store, adapter
        if toks is not None:
            return toks.store, None
        store = getattr(state, "store", state)
        return (store if getattr(store, "trainable", True) else None), None

    @property
    def stepping(self):
        return TrainState.stepping_of(self)

    @property
    def opt_store(self):
        """The store that takes the optimizer step, or None (stepping_of)."""
        return self.stepping[0]

    @property
    def step(self):
        st = self.opt_store
        return self.store.count if st is None else st.count

    @property
    def params(self):
        return self.store


def _stepping_stores(*states):
    """The stores whose optimizer steps a train_step of these states takes (TrainState.opt_store): their host step counts follow the
    replays of a captured step."""
    stores = [TrainState.stepping_of(st)[0] for st in states]
    return [st for st in stores if st is not None]


def create_lion_optimizer_states(models, train_unet=True, train_text_encoder=True, adam_to_lion_scale_factor=7,
                                 u_net_learning_rate=1e-6, text_encoder_learning_rate=1e-6,
                                 excluded_layer_pattern_from_weight_decay=(), excluded_layer_from_quantization=(),
                                 lion_8bit_block_size=None, quantize_unet_state=False, quantize_text_encoder_state=False,
                                 with_unet_ema=False, with_text_encoder_ema=False, device="cuda", lr_scheduler="constant",
                                 lr_schedule=None, ema_schedule=None, ema_rate=0.0, optimizer="lion", lora=None, new_tokens=None,
                                 controlnet=None, ip_adapter=None):
    """training_utils.py:281-427.  lr = learning_rate / adam_to_lion_scale_factor, wd = 1e-2 * scale, b1=.9, b2=.99,
    chain(clip_by_global_norm(1), lion_8bit | lion).  Builds the flat HBM stores and loads the weights.
    lr_scheduler / lr_schedule / ema_schedule / ema_rate: the per-step schedules of lr_schedule.resolve, installed in each trained store
    (ParamStore.set_schedule; the lr schedule scales each store's own rate).  "constant" without an EMA schedule installs nothing.
    optimizer: "lion" (the reference's), "adamw", or dict(name=, b1=, b2=, eps=, weight_decay=).  AdamW (8-bit block-quantised or fp32
    moments by the same quantize_* switches) takes the learning rates AS GIVEN - an Adam recipe needs no translation, so
    adam_to_lion_scale_factor does not apply - with wd=1e-2, b1=.9, b2=.999, eps=1e-8 unless the dict says otherwise.
    "prodigy", or dict(name="prodigy", lr=, b1=, b2=, beta3=, eps=, weight_decay=, d0=, d_coef=, growth_rate=, use_bias_correction=,
    safeguard_warmup=): the learning-rate-free optimizer (include/sdt.h "Prodigy").  The learning rates above are NOT USED: Prodigy steps
    by d * lr with d estimated while it trains, lr is a multiplier that defaults to 1 (schedules scale it), weight_decay defaults to 0.
    Its state is float32 whatever the quantize_* switches say (they still decide which gradients are kept in bf16).
    lora: None, or dict(unet=lora.LoraConfig, text_encoder=lora.LoraConfig | None | "frozen").  The base stores are then built frozen
    (trainable=False) and loaded once; every setting above (quantisation, decay and quantisation exclusions, EMA, optimizer, rates and
    schedules) configures the ADAPTER's store of that model instead (TrainState.adapter.store), which is the one that steps.  A text
    encoder without a LoraConfig only runs its forward.  Mixed modes - one model fully fine-tuned, the other adapted - are refused.
    new_tokens: None, or a tokens.TokenConfig (textual inversion).  Both base stores are built frozen; the text encoder's store carries
    the trained rows (TrainState.tokens, tokens.attach), and the text encoder's settings above - rate, optimizer, quantisation switches,
    schedules, EMA - configure the TOKEN store.  Alone, the UNet has no adapter and steps nothing; with lora=dict(unet=LoraConfig,
    text_encoder=None | "frozen") the UNet's adapter trains beside the tokens (pivotal tuning).  A text-encoder LoraConfig beside new
    tokens is refused.
    controlnet, ip_adapter: None, or dict(config=nets.controlnet_config(...) / nets.ip_adapter_config(...)[, params=host tree]) - a loaded
    ControlNet / IP-Adapter, or one initialised from the UNet (nets.controlnet_from_unet, nets.ip_adapter_from_unet).  Both follow the
    rules of nets.SideNetwork: frozen base stores, the UNet state's field of that name holds the network's store, which the UNet's
    settings above configure and which steps; refused beside lora=, new_tokens= and each other, on an inpainting UNet, and with a
    config that does not extend the UNet's."""
    out = {"unet_state": None, "text_encoder_state": None}
    given = dict(lora=lora, new_tokens=new_tokens, controlnet=controlnet, ip_adapter=ip_adapter)
    for net in reversed(nets.SIDE_NETWORKS):  # (ip_adapter= is validated before controlnet=)
        side, name = given[net.name], net.name
        if side is None:
            continue
        if not isinstance(side, dict) or "config" not in side or set(side) - {"config", "params"}:
            raise ValueError(f"{name}: None or dict(config=nets.{name}_config(...)[, params=tree]), not {side!r}")
        for others, message in net.beside:
            if any(given[o] is not None for o in others):
                raise ValueError(message)
        if not (train_unet and train_text_encoder):
            raise ValueError(f"{name}: needs both states (train_unet and train_text_encoder)")
        scfg, ucfg = side["config"], models["unet"]["config"]
        if nets.inpaint_latent_channels(ucfg) is not None:
            raise ValueError(f"{name}: {net.article} on an inpainting UNet is not supported")
        if any(k not in scfg for k in net.adds):
            raise ValueError(f"{name}: the config needs {' and '.join(net.adds)} (nets.{name}_config)")
        net.config(ucfg, *(scfg[k] for k in net.adds), **net.config_kwargs(models))
        for k in net.same:
            if _plain(scfg.get(k)) != _plain(ucfg.get(k)):
                raise ValueError(f"{name}: the config's {k}={scfg.get(k)!r} differs from the UNet's {ucfg.get(k)!r}")
    if new_tokens is not None:
        if not isinstance(new_tokens, tokens_mod.TokenConfig):
            raise ValueError(f"new_tokens: None or a tokens.TokenConfig, not {new_tokens!r}")
        if not (train_unet and train_text_encoder):
            raise ValueError("new_tokens: needs both states (train_unet and train_text_encoder)")
        if isinstance(lora, dict) and isinstance(lora.get("text_encoder"), lora_mod.LoraConfig):
            raise ValueError("new_tokens: a text-encoder LoRA together with new tokens is not supported (lora['text_encoder'] must be "
                             "None or 'frozen')")
    if lora is not None:
        if not isinstance(lora, dict) or set(lora) - {"unet", "text_encoder"}:
            raise ValueError(f"lora: None or dict(unet=LoraConfig, text_encoder=LoraConfig | None | 'frozen'), not {lora!r}")
        te_l = lora.get("text_encoder")
        te_l = None if te_l == "frozen" else te_l
        if not isinstance(lora.get("unet"), lora_mod.LoraConfig) or not (te_l is None or isinstance(te_l, lora_mod.LoraConfig)):
            raise ValueError("lora: unet must be a LoraConfig and text_encoder a LoraConfig, None or 'frozen' - a fully fine-tuned UNet "
                             "beside an adapted text encoder (or the reverse) is not supported")
        if not (train_unet and train_text_encoder):
            raise ValueError("lora: needs both states (train_unet and train_text_encoder); the text encoder is frozen by "
                             "text_encoder='frozen'")
        lora = {"unet": lora["unet"], "text_encoder": te_l}
    # the base stores only run; adapters' / the tokens' / a side network's own stores step
    frozen = any(v is not None for v in given.values())
    opt_cls, opt = optimizers.parse(optimizer)

    def make(spec, weights, cfg, fn, lr, quant, ema, which):
        hyper, okw = opt_cls.builder(lr, adam_to_lion_scale_factor, opt)
        sched = resolve_schedule(lr_scheduler, hyper["lr"], ema_rate, lr_schedule=lr_schedule, ema_schedule=ema_schedule)
        okw = dict(okw, quantise=quant, quant_excluded=tuple(excluded_layer_from_quantization),
                   wd_excluded=tuple(excluded_layer_pattern_from_weight_decay), block_size=lion_8bit_block_size or 16, with_ema=ema)
        # full fine-tune: the store itself is trained.  LoRA: a frozen base, loaded once, and (unless the model only runs its forward)
        # an adapter whose own store takes those keywords and the optimizer step
        store = ParamStore(spec, device=device, **(dict(trainable=False) if frozen else okw))
        store.load(weights)
        adapter = lora_mod.attach(store, lora[which], **okw) if lora is not None and lora[which] is not None else None
        toks = tokens_mod.attach(store, new_tokens, **okw) if new_tokens is not None and which == "text_encoder" else None
        sides = {}
        for net in nets.SIDE_NETWORKS:  # a side network's own store takes the UNet's keywords and the optimizer step
            side = given[net.name]
            if side is not None and which == "unet":
                sstore = ParamStore(net.spec(side["config"]), device=device, **okw)
                tree = side.get("params")
                sstore.load(flatten_if_nested(tree) if tree is not None else net.from_unet(weights, side["config"]))
                setattr(sstore, net.marker, side["config"])  # marks the store: save_model refuses it (and its EMA view) as UNet weights
                sides[net.name] = net.wrapper(sstore, side["config"])
        state = TrainState(fn, store, cfg, hyper, adapter, toks, **sides)
        if state.opt_store is None:  # a frozen model with nothing hung on it only runs its forward
            state.hyper = {}
        if sched is not None and state.opt_store is not None:
            state.opt_store.set_schedule(lr=sched[0], ema=sched[1])
        return state

    if train_unet:
        m = models["unet"]
        out["unet_state"] = make(nets.unet_spec(m["config"]), m["unet_params"], m["config"], nets.unet_forward,
                                 u_net_learning_rate, quantize_unet_state, with_unet_ema, "unet")
    if train_text_encoder:
        m = models["text_encoder"]
        out["text_encoder_state"] = make(nets.clip_text_spec(m["config"]), m["text_encoder_params"], m["config"],
                                         nets.clip_text_forward, text_encoder_learning_rate,
                                         quantize_text_encoder_state, with_text_encoder_ema, "text_encoder")
        out["text_encoder_state"].store.mark_unused(nets.unused_text_leaves(m["config"]))
    return out


def _plain(v):
    return list(v) if isinstance(v, (tuple, list)) else v


def on_device_model_training_state(training_config: TrainingConfig, models=None, device="cuda", *, lr_schedule=None,
                                   ema_schedule=None, optimizer="lion", lora=None, new_tokens=None, controlnet=None, ip_adapter=None):
    """training_utils.py:430-501.  `models`: load_models' result - host weight trees + configs
    ({"unet": {"unet_params", "config"}, "vae": {"vae_params", "config"}, "text_encoder": {...}}); None reads the
    diffusers directory at training_config.model_path (checkpoint.load_models).  Note the reference passes NEITHER learning
    rate from the config (:432-442) - the effective lr is the 1e-6 default / 7 - which is mirrored here.
    training_config.lr_scheduler names the learning-rate schedule (lr_schedule.LR_SCHEDULES); its step counts come as
    lr_schedule=dict(num_warmup_steps=, num_training_steps=, num_cycles=, power=, lr_end=), and
    ema_schedule=dict(kind="warmup", update_after_step=, use_ema_warmup=, inv_gamma=, power=, min_decay=) warms the EMA rate up to
    training_config.ema_rate (lr_schedule.resolve; ValueError for a name without the counts it needs).
    optimizer: create_lion_optimizer_states' (TrainingConfig has no field for it).
    lora: create_lion_optimizer_states' - dict(unet=lora.LoraConfig(rank, alpha), text_encoder=LoraConfig | None | "frozen") trains low-rank
    adapters on frozen base weights.  The tuple keeps its shape: the states' `store` are the frozen weight stores, `adapter` the adapters,
    and the EMA views wrap the adapters' stores (None for a text encoder without an adapter).
    new_tokens: create_lion_optimizer_states' - a tokens.TokenConfig trains placeholder-token embeddings on the frozen text encoder, alone or
    beside a UNet LoRA.  The text state's `tokens` is the TokenAdapter and its EMA view wraps the token store; a UNet without an adapter
    has no EMA view (None).
    controlnet, ip_adapter: create_lion_optimizer_states' - dict(config=[, params=]) trains a ControlNet / an IP-Adapter on the frozen UNet
    (nets.SideNetwork): unet_state.controlnet / unet_state.ip_adapter holds its store and config, the UNet EMA view wraps that store, the
    text encoder has none; batches carry conditioning_pixel_values / image_embeds."""
    _lib.require_device()
    if models is None:
        models = load_models(training_config)
    states = create_lion_optimizer_states(
        models, train_text_encoder=True, train_unet=True, adam_to_lion_scale_factor=7,
        excluded_layer_pattern_from_weight_decay=training_config.excluded_layer_pattern_from_weight_decay,
        excluded_layer_from_quantization=training_config.excluded_layer_from_quantization,
        lion_8bit_block_size=training_config.quant_block_size,
        quantize_unet_state=training_config.quantize_unet_state,
        quantize_text_encoder_state=training_config.quantize_text_encoder_state,
        with_unet_ema=training_config.accumulate_unet_ema, with_text_encoder_ema=training_config.accumulate_text_encoder_ema,
        device=device, lr_scheduler=training_config.lr_scheduler, lr_schedule=lr_schedule, ema_schedule=ema_schedule,
        ema_rate=training_config.ema_rate, optimizer=optimizer, lora=lora, new_tokens=new_tokens, controlnet=controlnet,
        ip_adapter=ip_adapter)
    vae_cfg = models["vae"]["config"]
    vae_store = ParamStore(nets.vae_encoder_spec(vae_cfg), device=device, trainable=False)
    vae_store.load(models["vae"]["vae_params"])
    vae_store.prepare()
    # the train path holds the encoder only; save_model(vae_params=frozen_vae.params) (training.py:151-158) must still write
    # the whole frozen VAE, so the store keeps a reference to the host tree it was loaded from
    vae_store.full_tree = models["vae"]["vae_params"]
    frozen_vae = FrozenModel(call=vae_cfg, params=vae_store)
    sched = DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule=training_config.beta_scheduler,
                          num_train_timesteps=1000, prediction_type=training_config.prediction_type)  # :223-230
    frozen_sched = FrozenModel(call=sched, params=sched.create_state(device))
    unet_state, te_state = states["unet_state"], states["text_encoder_state"]
    unet_ema = EmaView(unet_state.opt_store) if (training_config.accumulate_unet_ema and unet_state.opt_store is not None) else None
    te_ema = EmaView(te_state.opt_store) if (training_config.accumulate_text_encoder_ema and te_state.opt_store is not None) else None
    model_object_dict = {"unet": unet_state.config, "vae": vae_cfg, "text_encoder": te_state.config, "schedulers": sched}
    return unet_state, te_state, unet_ema, te_ema, frozen_vae, frozen_sched, model_object_dict


def _min_snr_weights(sched_state, timesteps, gamma, prediction_type):
    """training_utils.py:546-568 (tiny gather on (B,) values)."""
    ac = sched_state.alphas_cumprod
    snr = (ac / (1 - ac))[timesteps.long()]
    m = torch.minimum(snr, torch.full_like(snr, gamma))
    return (m / (snr + 1) if prediction_type == "v_prediction" else m / snr).to(torch.float32).contiguous()


LOSS_TYPES = {"l2": 0, "huber": 1, "smooth_l1": 2}  # the values are sdt_robust_loss_fwd_bwd's loss_type
HUBER_SCHEDULES = ("constant", "exponential", "snr")


def _check_loss_type(loss_type, huber_c, huber_schedule):
    """ValueError for loss options train_step cannot run (kohya's --loss_type / --huber_c / --huber_schedule)."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type={loss_type!r} must be one of {', '.join(LOSS_TYPES)}")
    if huber_schedule not in HUBER_SCHEDULES:
        raise ValueError(f"huber_schedule={huber_schedule!r} must be one of {', '.join(HUBER_SCHEDULES)}")
    c = huber_c
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or not c > 0:
        raise ValueError(f"huber_c={c!r} must be a finite number > 0")
    if c > 1 and huber_schedule != "constant":
        raise ValueError(f"huber_c={c!r} > 1: the {huber_schedule} schedule runs from 1 down to huber_c and needs huber_c <= 1")


def _check_dpo(beta, unet_state, text_encoder_state, tokens, side, batch, loss_type, min_snr_gamma, reducer):
    """ValueError for what a Diffusion-DPO step (train_step dpo_beta=) cannot run; each message names the rule."""
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not math.isfinite(beta) or not beta > 0:
        raise ValueError(f"dpo_beta={beta!r} must be a finite number > 0 (diffusers trains SD1.5 / SDXL with 5000)")
    if side is not None or tokens is not None or getattr(unet_state, "adapter", None) is None:
        raise ValueError("dpo_beta: the UNet state must carry a LoRA / DoRA adapter and nothing else - the frozen base under the adapter "
                         "is the reference model; full fine-tuning, side networks and new tokens would need a second reference store")
    if getattr(text_encoder_state, "adapter", None) is not None:
        raise ValueError("dpo_beta: a text-encoder adapter is not supported - the context would differ between the trained and the "
                         "reference pass (build the text encoder \"frozen\")")
    held = [k for k in ("loss_mask", "loss_weight") if k in batch]
    if held:
        raise ValueError(f"dpo_beta: {' / '.join(held)} in the batch is not supported - the preference loss has no masked or weighted form")
    if loss_type != "l2":
        raise ValueError(f"dpo_beta: loss_type={loss_type!r} is not supported - the preference loss compares squared errors (\"l2\")")
    if min_snr_gamma:
        raise ValueError(f"dpo_beta: min_snr_gamma_magnitude={min_snr_gamma!r} is not supported - a pair's samples share one timestep and "
                         "the loss takes no per-sample weight (it must be 0)")
    if reducer is not None:
        raise ValueError("dpo_beta: data-parallel training is not supported - LoRA states take no reducer")


def huber_threshold_table(alphas_cumprod, huber_c, huber_schedule):
    """The Huber threshold of every training timestep, float32 (T,), computed in float64 and rounded once (include/sdt.h "ROBUST LOSS";
    kohya / diffusers huber_schedule).  alphas_cumprod: the scheduler's host table (T,).
      constant     c[t] = huber_c
      exponential  c[t] = exp(t * ln(huber_c) / T): 1 at t = 0, towards huber_c at high noise
      snr          sigma = sqrt((1 - abar_t) / abar_t), c[t] = (1 - huber_c) / (1 + sigma)^2 + huber_c.  abar = 0 (zero terminal SNR) gives
                   sigma = inf and c = huber_c by IEEE division, never 0 * inf."""
    _check_loss_type("huber", huber_c, huber_schedule)
    ac = np.asarray(alphas_cumprod, np.float64)
    T, c = ac.shape[0], float(huber_c)
    if huber_schedule == "constant":
        tab = np.full(T, c, np.float64)
    elif huber_schedule == "exponential":
        tab = np.exp(np.arange(T, dtype=np.float64) * (math.log(c) / T))
    else:
        with np.errstate(divide="ignore"):
            sigma = np.sqrt((1.0 - ac) / ac)
            tab = (1.0 - c) / (1.0 + sigma) ** 2 + c
    return tab.astype(np.float32)


def _huber_thresholds(sched_state, timesteps, huber_c, huber_schedule):
    """c_b of a (micro-)batch, f32 (B,): the table above, built once per scheduler state and option pair and kept on the device (a
    captured step only gathers from it, as _min_snr_weights gathers from alphas_cumprod)."""
    tables = sched_state.__dict__.setdefault("_huber_tables", {})
    key = (huber_schedule, float(huber_c))
    tab = tables.get(key)
    if tab is None:
        ac = sched_state.alphas_cumprod
        tab = tables[key] = torch.from_numpy(huber_threshold_table(ac.cpu().numpy(), huber_c, huber_schedule)).to(ac.device)
    return tab[timesteps.long()].contiguous()


def assemble_context(hs, batch, strip_bos_eos_token):
    """training_utils.py:643-673: (B*k,77,D) -> (B,k,77,D) -> (B,L,D).  k=1 without stripping is a free view."""
    d = hs.shape[-1]
    e = hs.view(batch, -1, 77, d)
    if strip_bos_eos_token:
        return torch.cat([e[:, 0, :-1, :], e[:, 1:-1, 1:-1, :].reshape(batch, -1, d), e[:, -1, 1:, :]], dim=1).contiguous()
    return e.view(batch, -1, d)


def encode_latent_moments(frozen_vae, pixel_values):
    """The pixel front of a step: f32 NCHW (B,3,H,W) device pixels -> the frozen VAE's posterior moments, bf16 NHWC (B,H/8,W/8,2L)
    (mean | log-variance), which is what a latent cache stores (latent_cache.build) and what train_step samples from.  Inside a step
    the GroupNorm statistics go to the step's arena; called on its own it opens and closes one."""
    vae_store, vae_cfg = frozen_vae.params, frozen_vae.call
    dev = vae_store.device
    B, C_in, H, W = pixel_values.shape
    with ops.gn_arena(dev):
        pix = torch.empty(B, H, W, 8, dtype=torch.bfloat16, device=dev)
        _lib.call("sdt_nchw_f32_to_nhwc_bf16", pixel_values.data_ptr(), pix.data_ptr(), B, C_in, H, W, 8,
                  torch.cuda.current_stream().cuda_stream)
        with trace.phase("vae_encode"):
            return nets.vae_encode_moments(vae_store, vae_cfg, pix)


def encode_inpaint_moments(frozen_vae, pixel_values, inpaint_mask):
    """The pixel front of an inpainting step: f32 NCHW (B,3,H,W) pixels and the f32 (B,H,W) repaint mask -> (moments, masked-image
    moments, latent mask): one sdt_inpaint_mask_pixels launch writes the image and the masked image (repaint ? 0 : x) as one bf16 stack
    of 2B rows plus the nearest-neighbour latent mask f32 (B,H/f,W/f), and ONE encoder pass over the stack gives both halves' moments,
    bf16 (B,H/f,W/f,2L) each (contiguous views of the stacked result).  latent_cache.build stores exactly these."""
    vae_store, vae_cfg = frozen_vae.params, frozen_vae.call
    dev = vae_store.device
    B, C_in, H, W = pixel_values.shape
    f = 2 ** (len(vae_cfg["block_out_channels"]) - 1)
    if H % f or W % f:
        raise ValueError(f"pixel_values {tuple(pixel_values.shape)}: height and width must be multiples of the VAE's downscale {f}")
    with ops.gn_arena(dev):
        pix = torch.empty(2 * B, H, W, 8, dtype=torch.bfloat16, device=dev)
        lmask = torch.empty(B, H // f, W // f, dtype=torch.float32, device=dev)
        _lib.call("sdt_inpaint_mask_pixels", pixel_values.data_ptr(), inpaint_mask.data_ptr(), pix.data_ptr(), lmask.data_ptr(), B, C_in,
                  H, W, 8, f, torch.cuda.current_stream().cuda_stream)
        with trace.phase("vae_encode"):
            both = nets.vae_encode_moments(vae_store, vae_cfg, pix)
        return both[:B], both[B:], lmask


def step_key(batch, downscale=8):
    """The key of dp_compile_all_unique_resolution's table for a loader batch of either kind: pixel_values' shape (B,3,H,W), or
    the shape of the pixels that cached latent_moments (B,h,w,2L) were encoded from, (B,3,h*downscale,w*downscale)."""
    if "pixel_values" in batch:
        return tuple(int(n) for n in batch["pixel_values"].shape)
    B, h, w, _ = batch["latent_moments"].shape
    return (int(B), 3, int(h) * downscale, int(w) * downscale)


LOSS_KEYS = ("loss_mask", "loss_weight")  # the optional batch entries that select the masked / weighted loss kernels
INPAINT_KEYS = ("inpaint_mask",)  # the batch entry that selects the inpainting front of the step (include/sdt.h "INPAINTING")
CONTROL_KEYS = (nets.CONTROLNET.batch_key,)  # "conditioning_pixel_values": what a ControlNet state's step reads (diffusers' name)
IP_KEYS = (nets.IP_ADAPTER.batch_key,)  # "image_embeds": what an IP-Adapter state's step reads (the published training script's name)
# every entry with one row per sample besides the image itself: what a micro-batch slices (input_ids hold k rows per sample)
PER_SAMPLE_KEYS = ("text_embeds", "time_ids", "masked_latent_moments") + LOSS_KEYS + INPAINT_KEYS + CONTROL_KEYS + IP_KEYS
# the keys whose presence selects launches, in the order a captured step reports a batch that adds or drops one (_GraphedStep)
LAUNCH_KEYS = LOSS_KEYS + INPAINT_KEYS + CONTROL_KEYS + IP_KEYS
_DTYPE_NAMES = {torch.float32: "float32", torch.bfloat16: "bfloat16"}


def _on_device(t, device):
    return t.device.type == device.type and (device.index is None or t.device.index == device.index)


def _check_entry(name, t, dtypes, want, device, tail, plural=False):
    """ValueError unless batch entry `name` is a contiguous tensor of one of `dtypes` and shape `want` on the step's device, reported in
    that order: type / dtype, device, shape, layout.  tail: how the shape message ends (what the shape follows from); plural: the
    name is one ("image_embeds live on")."""
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        raise ValueError(f"{name} must be a {' or '.join(_DTYPE_NAMES[d] for d in dtypes)} tensor, not {getattr(t, 'dtype', type(t))}")
    if not _on_device(t, device):
        raise ValueError(f"{name} {'live' if plural else 'lives'} on {t.device}, the step runs on {device}")
    if tuple(t.shape) != tuple(want):
        raise ValueError(f"{name} {'have' if plural else 'has'} shape {tuple(t.shape)}{tail}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _image_grid(batch, channels=(), scale=1):
    """(want, where) of an entry at the grid of the batch's image (which _check_batch has validated): pixel size beside pixel_values,
    latent size - times `scale`, a hint's downscale - beside latent_moments; (B, *channels, height, width) and how to say it."""
    if "latent_moments" in batch:
        m = batch["latent_moments"]
        return (int(m.shape[0]), *channels, int(m.shape[1]) * scale, int(m.shape[2]) * scale), "latent_moments (B,h,w,2L)"
    px = batch["pixel_values"]
    return (int(px.shape[0]), *channels, int(px.shape[2]), int(px.shape[3])), "pixel_values (B,3,H,W)"


def _mask_grid(batch):
    """_image_grid for a (B, height, width) mask, with the size named."""
    want, where = _image_grid(batch)
    return want, where + (": latent size (B,h,w)" if "latent_moments" in batch else ": pixel size (B,H,W)")


def _check_loss_entries(batch, device, masked_loss_floor, normalize_masked_area):
    """ValueError for loss_mask / loss_weight entries (and their two options) that the masked loss cannot take."""
    floor = masked_loss_floor
    if isinstance(floor, bool) or not isinstance(floor, (int, float)) or not 0.0 <= float(floor) <= 1.0:
        raise ValueError(f"masked_loss_floor={floor!r} must be a number in [0, 1]")
    mask, weight = batch.get("loss_mask"), batch.get("loss_weight")
    if normalize_masked_area and mask is None:
        raise ValueError("normalize_masked_area needs a loss_mask in the batch")
    if mask is not None:
        want, where = _mask_grid(batch)
        _check_entry("loss_mask", mask, (torch.float32,), want, device, f"; beside {where} = {want}")
    if weight is not None:
        B = int(batch["latent_moments" if "latent_moments" in batch else "pixel_values"].shape[0])
        _check_entry("loss_weight", weight, (torch.float32,), (B,), device, f": one weight per sample, ({B},)")


def _check_inpaint_entries(batch, unet_cfg, device):
    """ValueError for inpaint_mask / masked_latent_moments entries that do not fit the UNet or the batch's image (which _check_batch
    has validated).  An inpainting UNet (nets.inpaint_latent_channels) needs the mask, a plain one refuses both keys."""
    L = nets.inpaint_latent_channels(unet_cfg)
    mask, mm = batch.get("inpaint_mask"), batch.get("masked_latent_moments")
    if L is None:
        if mask is not None or mm is not None:
            raise ValueError(f"inpaint_mask / masked_latent_moments need an inpainting UNet (in_channels == 2 * out_channels + 1); this one "
                             f"has in_channels={unet_cfg.get('in_channels')}, out_channels={unet_cfg.get('out_channels')}")
        return
    if mask is None:
        raise ValueError(f"an inpainting UNet (in_channels={unet_cfg['in_channels']} = 2 * {L} + 1) needs inpaint_mask in the batch")
    want, where = _mask_grid(batch)
    _check_entry("inpaint_mask", mask, (torch.float32,), want, device, f"; beside {where} = {want}")
    if "latent_moments" in batch:
        if mm is None:
            raise ValueError("a cached batch for an inpainting UNet needs masked_latent_moments (bf16 (B,h,w,2L)) beside latent_moments")
        shape = tuple(batch["latent_moments"].shape)
        _check_entry("masked_latent_moments", mm, (torch.bfloat16,), shape, device, f"; latent_moments {shape}", plural=True)


def _refuse_without_state(net, entry):
    """ValueError for a side network's batch entry in a batch whose UNet state carries no such network."""
    if entry is not None:
        raise ValueError(f"{net.batch_key} need {net.article} state (on_device_model_training_state({net.name}=)); this UNet state carries "
                         "none")


def _check_ip_entries(batch, ip_adapter, device, rows):
    """ValueError for an image_embeds entry that does not fit the state or the batch: an IP-Adapter state needs it, f32 or bf16 (B, E)
    with E = the config's image_embed_dim, contiguous on the step's device; a state without an IP-Adapter refuses it."""
    emb = batch.get("image_embeds")
    if ip_adapter is None:
        return _refuse_without_state(nets.IP_ADAPTER, emb)
    E = int(ip_adapter.config["image_embed_dim"])
    if emb is None:
        raise ValueError(f"an IP-Adapter state's batch needs image_embeds (f32 or bf16 (B, {E}): the image encoder's pooled embedding)")
    _check_entry("image_embeds", emb, (torch.float32, torch.bfloat16), (rows, E), device,
                 f"; the batch has {rows} samples and the adapter's image_embed_dim is {E}: ({rows}, {E})", plural=True)


def _check_control_entries(batch, controlnet, device):
    """ValueError for a conditioning_pixel_values entry that does not fit the state or the batch's image (which _check_batch has
    validated): a ControlNet state needs it, f32 NCHW (B, conditioning_channels, H, W) at pixel size - the size of pixel_values, or
    f times the latent size of latent_moments - contiguous on the step's device; a state without a ControlNet refuses it."""
    cond = batch.get("conditioning_pixel_values")
    if controlnet is None:
        return _refuse_without_state(nets.CONTROLNET, cond)
    if cond is None:
        raise ValueError("a ControlNet state's batch needs conditioning_pixel_values (f32 (B, conditioning_channels, H, W) in [0, 1])")
    f = 2 ** (len(controlnet.config["conditioning_embedding_out_channels"]) - 1)
    want, where = _image_grid(batch, (int(controlnet.config["conditioning_channels"]),), f)
    if "latent_moments" in batch:
        where += f" and the downscale {f}"
    _check_entry("conditioning_pixel_values", cond, (torch.float32,), want, device, f"; beside {where}: {want}", plural=True)


def _check_batch(batch, unet_cfg, frozen_vae_state, device, masked_loss_floor=0.0, normalize_masked_area=False):
    """ValueError for a batch train_step cannot run, before any kernel.  Returns whether the batch holds cached moments."""
    has_px, has_mom = "pixel_values" in batch, "latent_moments" in batch
    if "masked_latent_moments" in batch and (has_px or not has_mom):
        raise ValueError("masked_latent_moments go beside latent_moments (a cached inpainting batch), not beside pixel_values or alone")
    if has_px and has_mom:
        raise ValueError("a batch holds either pixel_values or latent_moments, not both")
    if not has_px and not has_mom:
        raise ValueError("a batch needs pixel_values (f32 (B,3,H,W)) or latent_moments (bf16 (B,h,w,2L))")
    if has_px:
        if frozen_vae_state is None:
            raise ValueError("pixel_values need the frozen VAE: frozen_vae_state is None (only latent_moments train without it)")
        _check_inpaint_entries(batch, unet_cfg, device)
        _check_loss_entries(batch, device, masked_loss_floor, normalize_masked_area)
        return False
    m = batch["latent_moments"]
    if not torch.is_tensor(m) or m.dtype != torch.bfloat16 or m.dim() != 4:
        raise ValueError(f"latent_moments must be a bfloat16 (B,h,w,2L) tensor, not {getattr(m, 'dtype', type(m))} "
                         f"{tuple(getattr(m, 'shape', ()))}")
    if not _on_device(m, device):
        raise ValueError(f"latent_moments live on {m.device}, the step runs on {device}")
    if m.shape[3] % 2:
        raise ValueError(f"latent_moments' last dimension holds mean | log-variance and must be even, not {m.shape[3]}")
    if not m.is_contiguous():
        raise ValueError("latent_moments must be contiguous")
    Li = nets.inpaint_latent_channels(unet_cfg)
    if Li is not None:
        if m.shape[3] // 2 != Li:
            raise ValueError(f"latent_moments hold {m.shape[3] // 2} latent channels, the inpainting UNet's out_channels is {Li}")
    elif m.shape[3] // 2 != unet_cfg["in_channels"]:
        raise ValueError(f"latent_moments hold {m.shape[3] // 2} latent channels, the UNet's in_channels is {unet_cfg['in_channels']}")
    if unet_cfg.get("addition_embed_type") == "text_time" and "time_ids" not in batch:
        raise ValueError("a text_time (SDXL) UNet's default time_ids come from the pixel size, which cached latent_moments no longer "
                         "carry: the batch must hold time_ids")
    _check_inpaint_entries(batch, unet_cfg, device)
    _check_loss_entries(batch, device, masked_loss_floor, normalize_masked_area)
    return True


_FUSED_NORM = True  # False: always the pass over the gradient buffer (same bits)


def train_step(unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params, batch, train_rng,
               frozen_vae_state, frozen_noise_scheduler_state, strip_bos_eos_token=True, offset_noise_magnitude=0.0,
               min_snr_gamma_magnitude=0.0, perturbation_noise_magnitude=0.0, ema_rate=0.0, *, rand=None, reducer=None,
               vae_scale=0.18215, aux=None, micro_batches=1, masked_loss_floor=0.0, normalize_masked_area=False, loss_type="l2",
               huber_c=0.1, huber_schedule="snr", dpo_beta=None):
    """One DDPM training step on this rank's shard of the batch (training_utils.py:504-762), in place.

    batch: {"pixel_values": f32 (B,3,H,W) NCHW device tensor, "input_ids": i32 (B*k,77), "attention_mask": unused}.
    Instead of pixel_values a batch may hold "latent_moments": the bf16 (B,h,w,2L) contiguous device tensor encode_latent_moments
    gives for those pixels (latent_cache keeps them on disk).  The step then skips the VAE - frozen_vae_state may be None - and its
    front is one launch (sdt_latent_noise_target); the draws, and with the same moments every bit of the result, are the pixel
    step's.  ValueError for both keys or neither, pixel_values without a VAE, moments of another dtype / layout / channel count, and
    for a text_time UNet without time_ids (their default needs the pixel size).
    A `text_time` (SDXL) UNet also reads "time_ids" i32 (B,6) - (H, W, 0, 0, H, W) when absent - and "text_embeds" (B,1280), unless the
    text encoder is in SDXL mode (nets.dual_clip_config(sdxl_conditioning=True)): then input_ids are (B*k,2,77) (or (B, k*2*77)), the
    towers compute the pooled embedding (nets.sdxl_text_forward; from each sample's first window) and a text_embeds entry is refused.
    train_rng: a torch.Generator on the device (the reference threads a JAX key; joint distribution only matters).
    rand: optional dict of explicit draws for parity tests (posterior_eps NHWC, noise NCHW, timesteps[, offset_noise,
    perturb_noise]) - the reference's threefry stream is not reproducible outside JAX.
    micro_batches: K > 1 accumulates the gradient over K micro-batches of len(batch) / K samples (ParamStore.accumulate): each runs
    the forward and backward on its slice of `batch` and `rand` (without rand=, its draws come from train_rng in the order a plain
    step of that size takes them), and the optimizer steps once on the fp32 mean - the step over the whole batch, with the
    activation memory of one micro-batch.  metrics["loss"] is the mean of the micro-batch losses.  K = 1 is the plain step.
    LoRA states (TrainState.adapter): the step merges the adapters into the bf16 mirrors instead of preparing the stores, runs the same
    forward and backward - the weight-gradient kernels write dW of the adapted leaves into the adapters' scratch, every other weight
    gradient is skipped - projects dW onto the factors (adapter.project) and steps the adapters' stores; a text encoder without an
    adapter only runs its forward.  A reducer is refused (ValueError): the data-parallel exchange would have to be built over the adapter
    stores.
    New tokens (TrainState.tokens on the text state; include/sdt.h "NEW TOKENS"): input_ids may hold the placeholder ids V + j.  Both base
    stores are frozen; the stores that step are the UNet adapter's (pivotal tuning), if there is one, and the token store - a frozen UNet
    without an adapter steps nothing.  The backward runs through the UNet's input-gradient chain and the frozen text encoder down to the
    embedding, whose backward writes the gradient of the new rows (sdt_embedding_ext_bwd); weight gradients are skipped wherever no
    adapter takes them.  With TokenConfig(retract=True) the rows are rescaled after the token store's optimizer step
    (TokenAdapter.retract): it acts on the MASTER; the EMA, which the optimizer sweep updated from the un-retracted value, keeps the
    sweep's value.  ValueError for a reducer and for mixed modes (a trained base store, a text-encoder LoRA, tokens on the store
    without the state's `tokens`).
    Masked and weighted loss (include/sdt.h "MASKED LOSS"): a batch may hold "loss_mask", f32 contiguous on the step's device - (B,H,W)
    at pixel size beside pixel_values, (B,h,w) at latent size beside latent_moments - and "loss_weight", f32 (B,).  The mask is pooled to
    the latent grid (the mean of each block of clamp(m, 0, 1)), floored (masked_loss_floor in [0, 1]: OneTrainer's unmasked weight; 0 is a
    plain multiply) and multiplies each position's squared error; normalize_masked_area rescales each sample by h*w / (the sum of its
    effective mask), 0 for a sample that is masked out entirely; loss_weight multiplies the sample's loss (DreamBooth's
    prior_loss_weight) beside the min-SNR factor.  Neither enters the forward pass, the draws or the target.  With either key the loss
    runs as sdt_loss_mask_prepare (mask only) + sdt_masked_mse_loss_fwd_bwd and metrics gains "loss_per_sample" (B,) (the micro-batches'
    concatenated); aux= taps record the effective mask as aux["loss_mask"].  With neither, the step is launch for launch the plain one.
    ValueError for a mask of another dtype, device, shape or layout, a loss_weight that is not (B,), a floor outside [0, 1] and
    normalize_masked_area without a mask.
    Huber and smooth-L1 loss (include/sdt.h "ROBUST LOSS"): loss_type "huber" or "smooth_l1" replaces the squared error of an element by
    the pseudo-Huber 2c(sqrt(diff^2 + c^2) - c) or 2(sqrt(diff^2 + c^2) - c); the threshold c of a sample comes from its timestep by
    huber_schedule ("constant": huber_c; "exponential": from 1 at t = 0 towards huber_c; "snr": from 1 at no noise to huber_c at pure
    noise; huber_threshold_table).  The loss launch is then sdt_robust_loss_fwd_bwd for every kind of batch (after sdt_loss_mask_prepare
    when there is a mask): min-SNR, masks, weights and normalisation act as above, metrics always holds "loss_per_sample", and aux= taps
    record the thresholds as aux["huber_c"] and a copy of d loss / d pred as aux["dpred"].  "l2" (the default) is launch for launch
    the step described above.  ValueError for an unknown type or schedule, a huber_c that is not finite and > 0, and a huber_c > 1 with the snr or exponential schedule.
    Inpainting (include/sdt.h "INPAINTING"): a UNet with in_channels == 2L + 1 (nets.inpaint_latent_channels) reads [noisy latents | mask |
    VAE latents of the masked image], and its batch must hold "inpaint_mask", f32 contiguous on the step's device, 1 = repaint (m >= 0.5),
    0 = keep: (B,H,W) beside pixel_values - one sdt_inpaint_mask_pixels launch, then ONE VAE pass over the stack [image | masked image]
    of 2B (encode_inpaint_moments) - or (B,h,w) at latent size beside latent_moments, together with "masked_latent_moments" bf16
    (B,h,w,2L).  Either way the front is one sdt_inpaint_noise_target launch.  The masked image's posterior draw, rand
    ["masked_posterior_eps"] (B,h,w,L), is taken from train_rng after the plain step's draws of the (micro-)batch.  Noise, timesteps,
    target and the loss with all its options are the plain step's: the loss compares pred (L channels) with the target over the whole
    image, and loss_mask stays independent of inpaint_mask.  aux= taps gain "inpaint_mask" (latent size, 0/1), "masked_latents" (f32
    NCHW), "masked_moments" and "unet_input" (the bf16 tensor handed to the UNet).  ValueError for an inpainting UNet without the mask,
    either key on a plain UNet, a wrong dtype, device, shape or layout, and masked_latent_moments without latent_moments.
    ControlNet (TrainState.controlnet on the UNet state; include/sdt.h "CONTROLNET"): the batch must hold
    "conditioning_pixel_values", f32 NCHW (B, conditioning_channels, H, W) contiguous on the step's device, in [0, 1], at pixel size
    (pixel_values' size, or f times the latent size of latent_moments).  After the front the image is packed to bf16 NHWC,
    nets.controlnet_forward runs on the ControlNet's (trained) store, and the frozen UNet takes its residuals at unit scale
    (unet_forward(control=), ops.control_add); the loss with every option, the clip and the optimizer act on the ControlNet's store
    alone.  aux= taps gain "control_hint", "control_down" (list) and "control_mid".  ValueError for a batch without the key or with a
    key of another dtype, device, shape or layout, the key on a state without a ControlNet, a reducer, a LoRA adapter or new tokens
    beside the ControlNet, an inpainting UNet, and a trainable base store.
    IP-Adapter (TrainState.ip_adapter on the UNet state; nets.SideNetwork): as the ControlNet, with "image_embeds", f32 or bf16 (B,
    image_embed_dim) - nets.ip_adapter_tokens runs on the adapter's (trained) store and every attn2 of the frozen UNet adds its image
    term at unit scale (unet_forward(ip=)); aux= taps gain "ip_tokens".  The same ValueErrors, and one for a ControlNet beside it.
    Diffusion-DPO (dpo_beta; include/sdt.h "DPO LOSS", DESIGN.md §6 "Diffusion-DPO"): preference training of a LoRA / DoRA UNet state on
    (preferred, rejected) pairs against the frozen base as the reference model.  The batch is an ordinary batch of N = 2P samples,
    interleaved (preferred, rejected, preferred, ...); input_ids cover all N samples.  posterior_eps is per sample (N); noise, timesteps,
    offset_noise and perturb_noise are per PAIR: rand= entries have leading dim P (sliced per micro-batch at pair granularity), and
    without rand= they are drawn from train_rng at size P in the plain step's order; the step expands them with repeat_interleave(2, 0)
    in front of the unchanged front kernels.  Per (micro-)batch, after the front and the frozen text encoder: adapter.restore()
    (sdt_lora_restore: the mirror's adapted leaves are the base's), the UNet forward without a tape -> ref_pred, adapter.merge("master"),
    the taped forward -> pred, sdt_dpo_loss_fwd_bwd, then the LoRA step's backward, projection and optimizer step.  The context and the
    SDXL conditioning are computed once for both passes.  When the step returns the mirror holds the merged weights, as after a LoRA
    step.  metrics: "loss" (the mean over pairs of -logsigmoid(-beta/2 * ((m_w - m_l) - (r_w - r_l)))), "implicit_acc" (the mean of
    logits > 0, as diffusers logs it), "dpo_logits" (P,), "model_mse" (N,), "ref_mse" (N,) - the micro-batches' concatenated; aux= taps
    gain "ref_pred", "dpo_coef", "dpo_pair_loss" and "dpred".  diffusers trains SD1.5 / SDXL with beta = 5000.  ValueError for a dpo_beta that is not
    finite and > 0, a UNet state without a LoRA / DoRA adapter (full fine-tune, side networks and new tokens would need a second
    reference store), a text-encoder adapter (the context would differ between the passes), an odd batch or micro-batch, loss_mask /
    loss_weight in the batch, loss_type other than "l2", a min-SNR gamma and a reducer.  dpo_beta=None is launch for launch the step
    described above.
    Returns the reference's 6-tuple; metrics["loss"] is a device scalar (read it to synchronise, as training.py:238-245)."""
    _check_loss_type(loss_type, huber_c, huber_schedule)
    text_time = unet_state.config.get("addition_embed_type") == "text_time"
    sdxl = text_time and nets.sdxl_conditioning(text_encoder_state.config)
    if sdxl and "text_embeds" in batch:
        raise ValueError("the text encoder is in SDXL mode and computes the pooled text embedding itself: a batch in that mode must "
                         "not carry text_embeds")
    us, ts = unet_state.store, text_encoder_state.store
    adapters = [a for a in (getattr(unet_state, "adapter", None), getattr(text_encoder_state, "adapter", None)) if a is not None]
    tk = getattr(text_encoder_state, "tokens", None)
    if tk is not None:
        if us.trainable or ts.trainable or getattr(text_encoder_state, "adapter", None) is not None or tk is not getattr(ts, "tokens", None):
            raise ValueError("new tokens: mixed modes are not supported - both base stores are frozen, the text encoder's store carries "
                             "the tokens and no LoRA adapter (the UNet trains through an adapter of its own or not at all)")
        if reducer is not None:
            raise ValueError("new tokens: data-parallel training is not supported - the GradReducer would have to be built over the "
                             "token store (TrainState.tokens.store)")
    elif getattr(unet_state, "tokens", None) is not None or getattr(ts, "tokens", None) is not None or getattr(us, "tokens", None) is not None:
        raise ValueError("new tokens: the text-encoder state must carry the TokenAdapter its store carries (TrainState.tokens; "
                         "create_lion_optimizer_states(new_tokens=) builds both)")
    sides = {}  # the side networks the UNet state carries (nets.SIDE_NETWORKS): past the refusals, one at the most
    for i, net in enumerate(nets.SIDE_NETWORKS):
        side = sides[net.name] = getattr(unet_state, net.name, None)
        if side is None:
            if getattr(text_encoder_state, net.name, None) is not None:
                raise ValueError(f"{net.label}: the UNet state carries the {net.label}, not the text-encoder state")
            continue
        if reducer is not None:
            raise ValueError(f"{net.label}: data-parallel training is not supported - the GradReducer would have to be built over "
                             f"{net.the}'s store (TrainState.{net.name}.store)")
        if adapters or tk is not None or getattr(us, "adapter", None) is not None or getattr(ts, "tokens", None) is not None:
            raise ValueError(f"{net.label}: a LoRA adapter or new tokens beside {net.article} are not supported")
        for other in nets.SIDE_NETWORKS[:i]:
            if sides[other.name] is not None:
                raise ValueError(f"{net.label}: {other.article} beside {net.article} is not supported")
        if nets.inpaint_latent_channels(unet_state.config) is not None:
            raise ValueError(f"{net.label}: an inpainting UNet is not supported")
        if us.trainable or ts.trainable:
            raise ValueError(f"{net.label}: a trainable base store is not supported - the UNet and the text encoder are frozen and only "
                             f"{net.the}'s store steps")
    cn, ipa = sides["controlnet"], sides["ip_adapter"]
    side = cn or ipa  # the side network whose store steps, or None
    dpo = dpo_beta is not None
    if dpo:
        _check_dpo(dpo_beta, unet_state, text_encoder_state, tk, side, batch, loss_type, min_snr_gamma_magnitude, reducer)
    lora = bool(adapters) or tk is not None  # the frozen-base step: adapters' and / or the tokens' own stores are the ones that step
    if adapters:
        if us.trainable or ts.trainable or unet_state.adapter is None:
            raise ValueError("LoRA: mixed modes are not supported - the UNet carries the adapter and both base stores are frozen "
                             "(a text encoder trains through an adapter of its own or not at all)")
        if reducer is not None:
            raise ValueError("LoRA: data-parallel training of adapter states is not supported yet - the follow-up is to build the "
                             "GradReducer over the adapter stores (TrainState.adapter.store) instead of the frozen weight stores")
    # the stores that are zeroed, accumulated into and stepped: the weight stores themselves, or the adapters' / the tokens' / the side
    # network's own
    opt_stores = _stepping_stores(unet_state, text_encoder_state)
    sched, sched_state = frozen_noise_scheduler_state.call, frozen_noise_scheduler_state.params
    dev = us.device
    cached = _check_batch(batch, unet_state.config, frozen_vae_state, dev, masked_loss_floor, normalize_masked_area)
    _check_control_entries(batch, cn, dev)
    _check_ip_entries(batch, ipa, dev, int(batch["latent_moments" if cached else "pixel_values"].shape[0]))
    masked = any(k in batch for k in LOSS_KEYS)
    inpaint = "inpaint_mask" in batch  # (_check_batch: exactly the batches of an inpainting UNet)
    robust = LOSS_TYPES[loss_type]  # 0: the squared error
    image_key = "latent_moments" if cached else "pixel_values"
    stream = torch.cuda.current_stream().cuda_stream
    rand = rand or {}
    K = micro_batches
    N = batch[image_key].shape[0]
    if not isinstance(K, int) or K < 1 or N % K:
        raise ValueError(f"micro_batches={micro_batches!r} must be a positive integer that divides the batch ({N})")
    if K > 1 and aux is not None:
        raise ValueError("aux= taps record a single forward pass: not available with micro_batches > 1")
    if K > 1 and reducer is not None and reducer.shard:
        raise ValueError("micro_batches > 1 is not supported with the sharded optimizer (GradReducer(shard=True))")
    B = N // K
    if dpo and (N % 2 or B % 2):
        raise ValueError(f"dpo_beta: the batch holds interleaved (preferred, rejected) pairs - the batch ({N}) and every micro-batch "
                         f"({B}) must be even")
    Bd = B // 2 if dpo else B  # leading dim of the draws a pair shares (noise, timesteps, offset and perturbation noise)
    L = batch["latent_moments"].shape[3] // 2 if cached else frozen_vae_state.call["latent_channels"]

    if reducer is not None:
        reducer.begin_step(hold=K > 1)  # accumulating: no bucket leaves before the last micro-batch (exchange_accumulated)

    def forward_backward(k, fused_norm):
        """Micro-batch k (the whole batch when K = 1): VAE encode, draws, CLIP, UNet, MSE, backward into grad / grad16.
        Returns (loss (1,), squared-norm slots of the two stores or None, loss per sample (B,) or None)."""
        if K == 1:
            mb, rnd = batch, rand
        else:
            sl = slice(k * B, (k + 1) * B)
            kc = batch["input_ids"].shape[0] // N  # text-encoder rows per sample
            mb = {n: v[sl] for n, v in batch.items() if n == image_key or n in PER_SAMPLE_KEYS}
            mb["input_ids"] = batch["input_ids"][k * B * kc: (k + 1) * B * kc]
            psl = slice(k * Bd, (k + 1) * Bd) if dpo else sl  # DPO: everything but the posterior draw is per pair
            rnd = {n: v[sl if n in ("posterior_eps", "masked_posterior_eps") else psl] for n, v in rand.items()}

        ops.gn_arena_begin(dev)  # GroupNorm statistics accumulated by producer epilogues: one memset per (micro-)batch

        # VAE encode -> posterior sample -> NCHW * 0.18215           (training_utils.py:574-586)
        mmoments = lmask = None
        if cached:
            moments, mmoments, lmask = mb["latent_moments"], mb.get("masked_latent_moments"), mb.get("inpaint_mask")
            H = W = None  # the pixel size is not known (and not needed: a text_time batch carries its time_ids)
        else:
            H, W = mb["pixel_values"].shape[2:]
            if inpaint:  # the image and the masked image through the VAE as one stack of 2B
                moments, mmoments, lmask = encode_inpaint_moments(frozen_vae_state, mb["pixel_values"], mb["inpaint_mask"])
            else:
                moments = encode_latent_moments(frozen_vae_state, mb["pixel_values"])
        fused = cached or inpaint  # the front is one launch: sdt_latent_noise_target / sdt_inpaint_noise_target
        h, w = moments.shape[1], moments.shape[2]
        eps = rnd.get("posterior_eps")
        if eps is None:
            eps = torch.randn(B, h, w, L, device=dev, generator=train_rng)
        if not fused:
            latents = torch.empty(B, L, h, w, dtype=torch.float32, device=dev)
            _lib.call("sdt_vae_posterior_sample", moments.data_ptr(), eps.data_ptr(), latents.data_ptr(), B, L, h, w,
                      moments.shape[3], vae_scale, stream)

        # The frozen VAE is all the step has read so far: the trained weights are first touched here.  With the sharded optimizer the
        # all-gather of the bf16 mirrors the previous step's owners wrote is still running beside the VAE encode (dp.GradReducer.wait_gathered)
        if k == 0 and reducer is not None:
            reducer.wait_gathered()
        with trace.phase("prepare_weights"):
            if k == 0 and lora:
                for ad in adapters:  # the frozen mirrors stay as the load left them: only the adapted leaves are rewritten
                    if not dpo:  # (a DPO step merges after its reference pass, in every micro-batch)
                        ad.merge("master")
                if tk is not None:
                    tk.select("master")  # (no launch: the embedding reads the trained rows where they are)
            elif k == 0 and side is not None:
                side.store.prepare()  # (the frozen mirrors stay as the load left them)
            elif k == 0:
                us.prepare()
                ts.prepare()
            for st in opt_stores:
                st.zero_grad()

        # noise, timesteps                                            (training_utils.py:590-624)
        noise = rnd.get("noise")
        if noise is None:
            noise = torch.randn(Bd, L, h, w, device=dev, generator=train_rng)
        pair = (lambda t: t.repeat_interleave(2, 0)) if dpo else (lambda t: t)  # a pair shares its noise and its timestep
        noise = pair(noise)
        off = pn = None
        if offset_noise_magnitude:
            off = rnd.get("offset_noise")
            if off is None:
                off = torch.randn(Bd, L, 1, 1, device=dev, generator=train_rng)
            off = pair(off)
            if not fused:
                noise = noise + off * offset_noise_magnitude
        if perturbation_noise_magnitude:
            pn = rnd.get("perturb_noise")
            if pn is None:
                pn = torch.randn(Bd, L, h, w, device=dev, generator=train_rng)
            pn = pair(pn)
            if not fused:
                noise = noise + perturbation_noise_magnitude * pn
        noise = noise.contiguous()
        timesteps = rnd.get("timesteps")
        if timesteps is None:
            timesteps = torch.randint(0, sched.num_train_timesteps, (Bd,), device=dev, generator=train_rng)
        timesteps = pair(timesteps).to(torch.int32).contiguous()
        meps = mlat = None
        if inpaint:  # the masked image's own posterior draw, after the plain step's draws so that those keep their positions
            meps = rnd.get("masked_posterior_eps")
            if meps is None:
                meps = torch.randn(B, h, w, L, device=dev, generator=train_rng)
            meps = meps.contiguous()

        # forward diffusion (+ v target)                              (training_utils.py:628-633, 688-701)
        if fused:
            # posterior sample, the mixing above, add_noise and the target in one launch, with the bits of the pixel path's chain
            if sched.prediction_type not in ("epsilon", "v_prediction"):
                raise ValueError(f"Unknown prediction type {sched.prediction_type}")  # training_utils.py:697-701
            cpad = -(-(2 * L + 1 if inpaint else L) // 8) * 8
            eps = eps.contiguous()
            off = None if off is None else off.contiguous()
            pn = None if pn is None else pn.contiguous()
            noisy = torch.empty(B, h, w, cpad, dtype=torch.bfloat16, device=dev)
            plain = sched.prediction_type == "epsilon" and off is None and pn is None  # the target is the noise as drawn
            target = noise if plain else torch.empty(B, L, h, w, dtype=torch.float32, device=dev)
            latents = torch.empty(B, L, h, w, dtype=torch.float32, device=dev) if aux is not None else None
            noisy_nchw = torch.empty(B, L, h, w, dtype=torch.float32, device=dev) if aux is not None else None
            ptr = lambda t: None if t is None else t.data_ptr()
            tail = (B, L, h, w, moments.shape[3], cpad, vae_scale, offset_noise_magnitude if off is not None else 0.0,
                    perturbation_noise_magnitude if pn is not None else 0.0, _PTYPE[sched.prediction_type], stream)
            if inpaint:  # the same front plus the mask and masked-image latent channels of the UNet input (`noisy` is that input)
                mlat = torch.empty(B, L, h, w, dtype=torch.float32, device=dev) if aux is not None else None
                _lib.call("sdt_inpaint_noise_target", moments.data_ptr(), mmoments.data_ptr(), eps.data_ptr(), meps.data_ptr(),
                          lmask.data_ptr(), noise.data_ptr(), ptr(off), ptr(pn), timesteps.data_ptr(), sched_state.alphas_cumprod.data_ptr(),
                          noisy.data_ptr(), None if plain else target.data_ptr(), ptr(latents), ptr(noisy_nchw), ptr(mlat), *tail)
            else:
                _lib.call("sdt_latent_noise_target", moments.data_ptr(), eps.data_ptr(), noise.data_ptr(), ptr(off), ptr(pn),
                          timesteps.data_ptr(), sched_state.alphas_cumprod.data_ptr(), noisy.data_ptr(), None if plain else target.data_ptr(),
                          ptr(latents), ptr(noisy_nchw), *tail)
        else:
            noisy, target, noisy_nchw = sched.add_noise_and_target(sched_state, latents, noise, timesteps, cpad=8,
                                                                   want_noisy_nchw=aux is not None)

        # text encoder + context assembly                             (training_utils.py:635-674)
        ids = mb["input_ids"]
        ids = ids if ids.dtype == torch.int32 else ids.to(torch.int32)
        pooled = None
        with trace.phase("text_encoder_forward"):
            if sdxl:  # both towers' hidden_states[-2] as the context, bigG's projected EOS embedding as text_embeds
                ids = ids.reshape(-1, 2, ids.shape[-1] if ids.dim() == 3 else 77)
                hs, pooled = nets.sdxl_text_forward(ts, text_encoder_state.config, ids, windows=ids.shape[0] // B)
            else:
                hs = text_encoder_state.apply_fn(ts, text_encoder_state.config, ids)
        ctx = assemble_context(hs, B, strip_bos_eos_token)

        # UNet                                                        (training_utils.py:678-684)
        added = None
        if text_time:
            # SDXL micro-conditioning.  Beyond the reference (its call passes no added_cond_kwargs): the pooled text embedding comes from
            # the text encoder in SDXL mode, otherwise from the batch; time_ids = (orig h, w, crop top, left, target h, w) default to the
            # uncropped pixel size (SURVEY.md §8(d) note on configs[4])
            tid = mb.get("time_ids")
            if tid is None:
                tid = torch.zeros(B, 6, dtype=torch.int32, device=dev)
                tid[:, 0::4].fill_(H)
                tid[:, 1::4].fill_(W)
            added = {"text_embeds": pooled if sdxl else mb["text_embeds"], "time_ids": tid}
        hint = down_r = mid_r = None
        if cn is not None:
            # the conditioning image f32 NCHW in [0, 1] -> bf16 NHWC, then the ControlNet on its own (trained) store; its residuals enter
            # the frozen UNet at unit scale and the tape starts at those additions
            cpv = mb["conditioning_pixel_values"]
            hint = torch.empty(B, cpv.shape[2], cpv.shape[3], -(-cpv.shape[1] // 8) * 8, dtype=torch.bfloat16, device=dev)
            _lib.call("sdt_nchw_f32_to_nhwc_bf16", cpv.data_ptr(), hint.data_ptr(), B, cpv.shape[1], cpv.shape[2], cpv.shape[3],
                      hint.shape[3], stream)
            with trace.phase("controlnet_forward"):
                down_r, mid_r = nets.controlnet_forward(cn.store, cn.config, noisy, timesteps, ctx, hint, added)
        ref_pred = None
        if dpo:
            # the reference pass: the same mirror with the adapted leaves put back to bf16(W0), no tape; then the merge the LoRA step
            # makes in front of its forward.  ctx and added serve both passes (the text encoder is frozen and carries no adapter).
            with trace.phase("dpo_reference_forward"):
                unet_state.adapter.restore()
                with torch.no_grad():
                    ref_pred = unet_state.apply_fn(us, unet_state.config, noisy, timesteps, ctx.detach(), added)
                unet_state.adapter.merge("master")
        with trace.phase("unet_forward"):
            ip_tokens = None
            if ipa is not None:
                # image_proj on the adapter's (trained) store, then every attn2 of the frozen UNet adds its image term at unit scale
                ip_tokens = nets.ip_adapter_tokens(ipa.store, ipa.config, mb["image_embeds"])
                pred = unet_state.apply_fn(us, unet_state.config, noisy, timesteps, ctx, added, ip=(ipa.store, ip_tokens))
            elif cn is not None:
                pred = unet_state.apply_fn(us, unet_state.config, noisy, timesteps, ctx, added, control=(down_r, mid_r))
            else:
                pred = unet_state.apply_fn(us, unet_state.config, noisy, timesteps, ctx, added)

        # MSE (+ min-SNR), forward and d loss / d pred in one launch  (training_utils.py:704-709)
        wts = None
        if min_snr_gamma_magnitude:
            wts = _min_snr_weights(sched_state, timesteps, min_snr_gamma_magnitude, sched.prediction_type)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        dpred = torch.empty_like(pred)
        C_out = unet_state.config["out_channels"]
        rws = ops.reduce_workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
        lps = emask = hub = None
        if dpo:
            # per-sample errors of both passes, the pairs' logits, losses and coefficients, then d loss / d pred: one call, two launches
            Pm = B // 2
            rws = ops.reduce_workspace(_lib.load().sdt_dpo_loss_workspace_bytes(B, h, w), dev)
            smse = torch.empty(2, B, dtype=torch.float32, device=dev)
            dlog, dpl = torch.empty(Pm, dtype=torch.float32, device=dev), torch.empty(Pm, dtype=torch.float32, device=dev)
            dcoef = torch.empty(B, dtype=torch.float32, device=dev)
            _lib.call("sdt_dpo_loss_fwd_bwd", pred.data_ptr(), ref_pred.data_ptr(), target.data_ptr(), float(dpo_beta), loss.data_ptr(),
                      smse.data_ptr(), dlog.data_ptr(), dpl.data_ptr(), dcoef.data_ptr(), dpred.data_ptr(), B, C_out, h, w, pred.shape[3],
                      rws.data_ptr(), rws.numel(), stream)
            lps = (dlog, smse[0], smse[1])
            if aux is not None:
                aux.update(ref_pred=ref_pred, dpo_coef=dcoef, dpred=dpred.clone(), dpo_pair_loss=dpl)
        elif masked or robust:
            # the effective latent mask and its per-sample sums, then the loss per sample first; a batch with loss_weight only passes no mask
            msum = None
            mask = mb.get("loss_mask")
            if mask is not None:
                f = mask.shape[1] // h
                if f not in (1, 2, 4, 8, 16) or tuple(mask.shape[1:]) != (h * f, w * f):
                    raise ValueError(f"loss_mask {tuple(mask.shape)} against the latent grid ({h}, {w}): the scale must be the same power of "
                                     "two, at most 16, on both axes")
                emask = torch.empty(B, h, w, dtype=torch.float32, device=dev)
                msum = torch.empty(B, dtype=torch.float32, device=dev)
                _lib.call("sdt_loss_mask_prepare", mask.data_ptr(), emask.data_ptr(), None, msum.data_ptr(), B, h, w, f,
                          float(masked_loss_floor), rws.data_ptr(), rws.numel(), stream)
            lw = mb.get("loss_weight")
            lps = torch.empty(B, dtype=torch.float32, device=dev)
            operands = (pred.data_ptr(), target.data_ptr(), None if emask is None else emask.data_ptr(),
                        msum.data_ptr() if normalize_masked_area else None, None if wts is None else wts.data_ptr(),
                        None if lw is None else lw.data_ptr())
            tail = (loss.data_ptr(), lps.data_ptr(), dpred.data_ptr(), B, C_out, h, w, pred.shape[3], rws.data_ptr(), rws.numel(), stream)
            if robust:  # the sample's threshold from its timestep, then the pseudo-Huber element in place of the square
                hub = _huber_thresholds(sched_state, timesteps, huber_c, huber_schedule)
                _lib.call("sdt_robust_loss_fwd_bwd", *operands, hub.data_ptr(), robust, *tail)
            else:
                _lib.call("sdt_masked_mse_loss_fwd_bwd", *operands, *tail)
        else:
            _lib.call("sdt_mse_loss_fwd_bwd", pred.data_ptr(), target.data_ptr(), None if wts is None else wts.data_ptr(),
                      loss.data_ptr(), dpred.data_ptr(), B, C_out, h, w, pred.shape[3], rws.data_ptr(), rws.numel(), stream)
        if aux is not None:
            if emask is not None:
                aux["loss_mask"] = emask
            if hub is not None:
                aux.update(huber_c=hub, dpred=dpred.clone())
            aux.update(latents=latents, noisy=noisy_nchw, ctx=ctx.detach(), pred=pred.detach(), target=target, moments=moments)
            if pooled is not None:
                aux["text_embeds"] = pooled.detach()
            if inpaint:
                aux.update(inpaint_mask=(lmask >= 0.5).to(torch.float32), masked_latents=mlat, unet_input=noisy.detach(),
                           masked_moments=mmoments)
            if ip_tokens is not None:
                aux["ip_tokens"] = ip_tokens.detach()
            if cn is not None:
                aux.update(control_hint=hint, control_down=[r.detach() for r in down_r], control_mid=mid_r.detach())

        # reverse mode through UNet and text encoder                  (training_utils.py:719-729)
        if fused_norm:
            ops.sq_begin(us)
            ops.sq_begin(ts)
        with trace.phase("backward_unet_text"), ops.wgrad_grouping():  # Dense weight gradients are issued a dozen per launch
            pred.backward(dpred)
        for ad in adapters:  # (the grouped weight gradients have been flushed: dW of every adapted leaf is in the scratch)
            ad.project()
        sq_u = ops.sq_end(us) if fused_norm else None
        sq_t = ops.sq_end(ts) if fused_norm else None
        return loss, sq_u, sq_t, lps

    if K == 1:
        # one process: the norm clip_by_global_norm needs is that of the gradients as the weight-gradient kernels write them - they leave
        # its partial sums behind (ops.sq_begin / sq_end), and the 4-byte-per-parameter pass over the finished buffer is not needed
        loss, sq_u, sq_t, lps = forward_backward(0, reducer is None and _FUSED_NORM and dev.type == "cuda" and not lora and side is None)
        grad_source = "grad"
        # data-parallel mean of the gradients (implicit all-reduce under GSPMD in the reference)
        if reducer is not None:
            with trace.phase("grad_exchange_finish"):
                reducer.finish()
                loss = reducer.mean_scalar(loss)
    else:
        # K micro-batches summed in fp32 (ParamStore.gacc) and scaled by 1/K: the mean gradient of the whole batch, as the loss is a
        # per-sample mean and nothing in the VAE / CLIP / UNet mixes samples.  One process: the last pass (finish) also scales and
        # takes the squared norm.  Data parallel: the last pass is an add, the fp32 sums are all-reduced, then scale + norm.
        exchange = reducer is not None and reducer.active
        losses, per_sample = [], []
        for k in range(K):
            out_k = forward_backward(k, False)
            losses.append(out_k[0])
            per_sample.append(out_k[3])
            mode = "init" if k == 0 else ("finish" if k == K - 1 and not exchange else "add")
            with trace.phase("grad_accumulate"):
                for st in opt_stores:
                    st.accumulate(mode, 1.0 / K if mode == "finish" else 1.0, norm=mode == "finish")
        loss = torch.cat(losses).mean(0, keepdim=True)
        if dpo:
            lps = tuple(torch.cat(t) for t in zip(*per_sample))
        else:
            lps = torch.cat(per_sample) if masked or robust else None
        sq_u = sq_t = None
        grad_source = "acc"
        if exchange:
            with trace.phase("grad_exchange_finish"):
                reducer.exchange_accumulated()
                loss = reducer.mean_scalar(loss)
            with trace.phase("grad_accumulate"):
                for st in opt_stores:
                    st.accumulate("scale", 1.0 / K, norm=True)

    # clip -> Lion(8-bit) -> decay -> -lr -> apply -> EMA         (training_utils.py:732-746)
    ur = ema_rate if (ema_rate and unet_ema_params is not None) else 0.0
    tr = ema_rate if (ema_rate and text_encoder_ema_params is not None) else 0.0
    with trace.phase("optimizer_clip_lion8_ema"):  # (LoRA: no fused partials - the norm by the ordinary pass over the adapters' few MB)
        for state, rate, sq in ((unet_state, ur, sq_u), (text_encoder_state, tr, sq_t)):
            store = state.opt_store
            if store is not None:  # (None: a LoRA run's text encoder without an adapter only ran its forward)
                store.optimizer_step(ema_rate=rate, shard=None if reducer is None else reducer.shard_pieces(store), sq_partials=sq,
                                     grad_source=grad_source, **state.hyper)
        if tk is not None and tk.cfg.retract:
            tk.retract()  # on the stepped master; the EMA keeps the value the sweep gave it
        if reducer is not None:
            reducer.after_optimizer()  # sharded optimizer: all-gather the bf16 weight mirrors the owners have just written
    ops.gn_arena_end(dev)
    metrics = {"loss": loss[0]}
    if dpo:
        metrics.update(implicit_acc=(lps[0] > 0).to(torch.float32).mean(), dpo_logits=lps[0], model_mse=lps[1], ref_mse=lps[2])
    elif masked or robust:
        metrics["loss_per_sample"] = lps  # local to this rank under data parallelism
    return (unet_state, text_encoder_state, unet_ema_params if ur else None, text_encoder_ema_params if tr else None,
            metrics, train_rng)


# Other threads keep making HIP calls while a step is captured (RCCL's watchdog polls events, loaders pin memory): only the
# capturing thread's own unsafe calls should fail the capture.
_CAPTURE_MODE = "thread_local"


class _GraphedStep:
    """One resolution's train_step, captured once into a HIP graph and replayed (the MI355X counterpart of the
    reference jit-compiling train_step per bucket shape, training_utils.py:765-983).

    A step is ~1,250 kernel launches; issued from Python the device idles ~15 % of the step waiting for the host, so
    after `warmup` eager calls (which size every workspace and set kernel attributes) the whole step - VAE encode, CLIP,
    UNet forward/backward, clip + Lion-8bit + EMA - is captured on a side stream and replayed with the batch copied into
    static buffers.  Calls that pass aux= taps stay eager.  With a data-parallel reducer the step is captured as two graphs around
    the gradient exchange (_capture_split)."""

    _pool = None  # graphs of different resolutions are never replayed concurrently: they share one memory pool

    def __init__(self, fn, warmup=2, reducer=None):
        self.fn, self.warmup, self.calls = fn, warmup, 0
        self.graph = self.static = self.static_rand = self.out = self.sig = self.held = None
        # multi-rank: graph A (forward + backward) | eager bucketed all-reduce behind per-bucket events | graph B (optimizer)
        self.reducer = reducer if (reducer is not None and reducer.active) else None
        self.graph_b = self.plan = None
        self.disabled = False

    @property
    def loss_keys(self):
        """Which of LOSS_KEYS the captured batch held, as (mask, weight) flags; None before the capture."""
        return None if self.held is None else tuple(k in self.held for k in LOSS_KEYS)

    def _capture(self, us, ts, ue, te, batch, rng, vae, sched, rand):
        self.static = {k: v.clone() for k, v in batch.items() if torch.is_tensor(v)}
        self.static_rand = None if rand is None else {k: v.clone() for k, v in rand.items()}
        self.sig = self._sig(us, ts, ue, te, rng, vae, sched, rand)
        self.held = tuple(k for k in LAUNCH_KEYS if k in batch)  # the launch-selecting keys of the captured batch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        if rng is not None and hasattr(g, "register_generator_state"):
            g.register_generator_state(rng)
        if _GraphedStep._pool is None:
            _GraphedStep._pool = torch.cuda.graph_pool_handle()
        if self.reducer is None:
            with torch.cuda.graph(g, pool=_GraphedStep._pool, capture_error_mode=_CAPTURE_MODE):
                self.out = self.fn(us, ts, ue, te, self.static, rng, vae, sched, rand=self.static_rand)
        else:
            self._capture_split(g, us, ts, ue, te, rng, vae, sched)
            if self.disabled:
                return
        # capturing executed nothing on the device, but the host-side step counters moved: undo, replay() re-applies
        for st in _stepping_stores(us, ts):
            st.count -= 1
        self.graph = g

    def _capture_split(self, g, us, ts, ue, te, rng, vae, sched):
        """Two graphs around the gradient exchange: reducer.finish() (called by train_step after the backward) ends graph A
        and begins graph B; the buckets' completion points are event-record nodes of graph A (dp.ExchangePlan)."""
        import gc
        import sys
        from . import dp
        red, pool = self.reducer, _GraphedStep._pool
        gb = torch.cuda.CUDAGraph()
        plan = dp.ExchangePlan(us.store.device)
        state = {"cur": None}
        counts = (us.store.count, ts.store.count)

        def split():
            g.capture_end()
            state["cur"] = None
            gb.capture_begin(pool=pool, capture_error_mode=_CAPTURE_MODE)
            state["cur"] = gb

        plan.split = split
        gc.collect()
        torch.cuda.empty_cache()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(side):
                g.capture_begin(pool=pool, capture_error_mode=_CAPTURE_MODE)
                state["cur"] = g
                red.capture = plan
                self.out = self.fn(us, ts, ue, te, self.static, rng, vae, sched, rand=self.static_rand)
                if state["cur"] is not gb:
                    raise RuntimeError("train_step never reached reducer.finish()")
                gb.capture_end()
                state["cur"] = None
        except Exception as e:  # leave the stream usable and fall back to eager steps (every rank takes the same branch)
            if state["cur"] is not None:
                try:
                    state["cur"].capture_end()
                except Exception:
                    pass
            us.store.count, ts.store.count = counts
            plan.close()
            self.disabled = True
            print(f"[sdt] step graph capture failed ({type(e).__name__}: {e}); this shape runs eagerly", file=sys.stderr)
            return
        finally:
            red.capture = None
        torch.cuda.current_stream().wait_stream(side)
        self.graph_b, self.plan = gb, plan

    @staticmethod
    def _sig(us, ts, ue, te, rng, vae, sched, rand):
        return (id(us), id(ts), id(ue), id(te), id(rng), id(vae), id(sched), None if rand is None else tuple(sorted(rand)))

    def __call__(self, us, ts, ue, te, batch, rng, vae, sched, rand=None, **extra):
        if extra:  # aux= taps and per-call overrides: eager
            return self.fn(us, ts, ue, te, batch, rng, vae, sched, rand=rand, **extra)
        if self.graph is None:
            if self.calls < self.warmup or self.disabled:
                self.calls += 1
                return self.fn(us, ts, ue, te, batch, rng, vae, sched, rand=rand)
            self._capture(us, ts, ue, te, batch, rng, vae, sched, rand)
            if self.disabled:
                return self.fn(us, ts, ue, te, batch, rng, vae, sched, rand=rand)
        if self.sig != self._sig(us, ts, ue, te, rng, vae, sched, rand):
            raise ValueError("a captured train_step is bound to the state objects (and rand= keys) it was captured with")
        if self.held != tuple(k for k in LAUNCH_KEYS if k in batch):
            key = next(k for k in LAUNCH_KEYS if (k in batch) != (k in self.held))  # the first one that was added or dropped
            if key in LOSS_KEYS:
                had = [k for k in LOSS_KEYS if k in self.held] or "neither"
                raise ValueError(f"this step was captured with {had} of {list(LOSS_KEYS)} in its batch and replays those launches: a batch "
                                 "that adds or drops one of them needs a step table of its own")
            raise ValueError(f"this step was captured {'with' if key in self.held else 'without'} {key} in its batch and replays those "
                             "launches: a batch that adds or drops it needs a step table of its own")
        for k, v in self.static.items():
            v.copy_(batch[k], non_blocking=True)
        if rand is not None:
            for k, v in self.static_rand.items():
                v.copy_(rand[k], non_blocking=True)
        self.graph.replay()
        if self.graph_b is not None:
            self.reducer.run_exchange(self.plan)  # overlaps the rest of graph A bucket by bucket
            self.graph_b.replay()
            self.reducer.run_post(self.plan)      # sharded optimizer: all-gather of the weight mirrors
            if self.reducer.shard:
                # what optimizer_step(shard=...) does when it runs as Python: a replayed sharded sweep leaves fp32 master / EMA / momentum
                # current only on the owners of the slices, so exports must raise until GradReducer.gather_state() (ParamStore._gather)
                us.store.state_whole = False
                ts.store.state_whole = False
        for st in _stepping_stores(us, ts):
            st.count += 1
        o = self.out
        return o[0], o[1], o[2], o[3], {k: v.clone() for k, v in o[4].items()}, o[5]


def dp_compile_all_unique_resolution(unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params,
                                     frozen_vae, frozen_schedulers, training_config: TrainingConfig, reducer=None,
                                     per_device_batch=None, use_graph=None, step_overrides=None, micro_batches=1):
    """training_utils.py:765-983: table {pixel_values.shape: step callable}.  Keys are the bucket shapes
    (B, 3, bucket[0], bucket[1]) of every (image_area_root, minimum_axis_length) pair.  Nothing is compiled up front:
    with use_graph (the default; SDT_GRAPH=0 turns it off) each shape captures its step into HIP graphs on its third call:
    one graph for a single process; with an active reducer, graph A (forward + backward) and graph B (optimizer) around
    the bucketed all-reduce, which stays outside the graphs and overlaps graph A bucket by bucket (dp.ExchangePlan).
    micro_batches=K: every step accumulates K micro-batches of per_device_batch (train_step micro_batches); the keys are then the
    batch the loader delivers, (K * per_device_batch, 3, H, W), and one graph (graph A: through the last micro-batch's add pass, with
    a reducer) holds all K forward / backward passes.
    step_overrides: keyword options of train_step that TrainingConfig has no field for, e.g. vae_scale, or masked_loss_floor /
    normalize_masked_area for batches with a loss_mask, or loss_type / huber_c / huber_schedule, or dpo_beta (Diffusion-DPO on LoRA states).  A captured step replays the launches
    of the batch it was captured with: it
    raises ValueError for a later batch that adds or drops loss_mask / loss_weight, or inpaint_mask (an inpainting UNet's batches
    always carry it; the static buffers take the mask and, for cached batches, masked_latent_moments like any other tensor key), or
    conditioning_pixel_values (a ControlNet state's batches always carry it; CONTROL_KEYS), or image_embeds (an IP-Adapter state's; IP_KEYS)."""
    import os
    B = per_device_batch or training_config.batch_size
    if not isinstance(micro_batches, int) or micro_batches < 1:
        raise ValueError(f"micro_batches={micro_batches!r} must be a positive integer")
    kw = dict(strip_bos_eos_token=training_config.strip_bos_eos_token,
              offset_noise_magnitude=training_config.offset_noise_magnitude,
              min_snr_gamma_magnitude=training_config.min_snr_gamma_magnitude,
              perturbation_noise_magnitude=training_config.perturbation_noise_magnitude,
              ema_rate=training_config.ema_rate)
    kw.update(step_overrides or {})  # e.g. vae_scale=0.13025 for the SDXL VAE (the reference hard-codes 0.18215, :586)
    if use_graph is None:
        env = os.environ.get("SDT_GRAPH")
        use_graph = env != "0" and unet_state.store.device.type == "cuda"

    def bound(us, ts, ue, te, batch, rng, vae, sched, **extra):
        return train_step(us, ts, ue, te, batch, rng, vae, sched, reducer=reducer, micro_batches=micro_batches, **kw, **extra)

    table = {}
    for area_root, min_axis in zip(training_config.image_area_root, training_config.minimum_axis_length):
        for bucket in calculate_resolution_array(area_root ** 2, min_axis, 64):
            table[(micro_batches * B, 3, int(bucket[0]), int(bucket[1]))] = _GraphedStep(bound, reducer=reducer) if use_graph else bound
    return table
