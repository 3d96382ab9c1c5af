"""The reference's training.py loop (training.py:43-307) on the MI355X path with the synthetic stand-in loader: loader ->
shape-keyed step table -> train_step -> loss CSV -> per-chunk save_model (+ -EMA) -> training-state file for resume.
One process per GPU:  python -m torch.distributed.run --nproc-per-node N examples/train_synthetic.py config.json
(single GPU: python examples/train_synthetic.py config.json).  config.json holds the reference's model_properties.json keys
(model_properties_example.json) plus "batches_per_chunk"; "model_path" is a diffusers-Flax pipeline directory.
--micro-batches K (or "micro_batches" in the config): every step accumulates the gradient over K micro-batches of
batch_size / (world * K) samples - the step over the global batch_size with the activation memory of one micro-batch.
An SDXL directory (text_encoder_2/) trains both text towers in SDXL mode: the loader emits ids for two towers and time_ids, the
pooled text embedding comes from the towers, and the saves are SDXL pipeline directories.
Schedules: "lr_scheduler" (constant, constant_with_warmup, linear, cosine, cosine_with_restarts, polynomial) takes its counts from the
optional keys lr_warmup_steps, lr_num_training_steps, lr_num_cycles, lr_power and lr_end; "ema_warmup": true warms the EMA rate up to
ema_rate (diffusers EMAModel), with the optional ema_inv_gamma, ema_power, ema_min_decay, ema_update_after_step and
ema_use_warmup_power (the 1 - (1 + s / inv_gamma) ** -power form).  Both advance once per optimizer step.
--cache-latents DIR (or "cache_latents" in the config): every chunk the run will visit is encoded once with the frozen VAE into a latent
cache under DIR (latent_cache.build: one record per batch, at the batch composition it is trained at), the VAE's device store is
dropped, and the steps train from the cache's readers without a VAE.
--masked-loss [FLOOR] (or "masked_loss" in the config: true or the floor): the loader emits a loss mask per image and the loss counts
each latent position by its pooled mask, at least FLOOR (default 0: only the masked area trains); --normalize-masked-area
("normalize_masked_area") rescales every sample by area / masked area; --prior-loss-weight W ("prior_loss_weight"): every second sample is a
class image whose loss counts W times (DreamBooth prior preservation).  A latent cache keeps the pooled masks and the weights.
--loss-type huber | smooth_l1 ("loss_type"; l2 is the default) trains on the pseudo-Huber loss, with --huber-c C ("huber_c", default 0.1)
and --huber-schedule snr | exponential | constant ("huber_schedule", default snr) for the threshold of each sample's timestep.
--inpaint ("inpaint": true) trains an inpainting UNet: a UNet that is not one already (in_channels != 2 * out_channels + 1) is widened
with zero conv_in rows (nets.widen_conv_in), the loader emits an inpaint_mask per image, and every step feeds [noisy latents | mask |
latents of the masked image].  With --cache-latents the cache keeps the masked image's moments and the latent mask.
--new-tokens N [--init-token ID] [--retract] ("new_tokens", "new_tokens_init_id", "new_tokens_retract"): textual inversion - N placeholder
tokens are trained on the frozen text encoder (tokens.TokenConfig; rows copied from token ID, else seeded noise at the table's scale;
--retract rescales them towards the table's standard deviation after every step), the loader puts their ids after BOS in every caption,
the text encoder's rate / optimizer / EMA settings configure the token store, and the saves hold the resized text encoder plus
<model>-tokens.npz.  Alone the UNet stays frozen; with --lora RANK the UNet's adapter trains beside the tokens (pivotal tuning).
--controlnet [DIR] ("controlnet": true or a directory): trains a ControlNet on the frozen UNet and text encoder - loaded from DIR
(checkpoint.load_controlnet) or initialised from the UNet (nets.controlnet_from_unet; "controlnet_channels" sets the embedder's widths) -
from batches with a conditioning image per sample; the UNet's rate / optimizer / EMA settings configure its store, every chunk writes
<model>-controlnet (and -controlnet-EMA), and --cache-latents keeps the conditioning images beside the moments.
--ip-adapter [DIR] ("ip_adapter": true or a directory): trains an IP-Adapter on the frozen UNet and text encoder - loaded from DIR
(checkpoint.load_ip_adapter) or initialised from the UNet (nets.ip_adapter_from_unet; "ip_adapter_embed_dim", "ip_adapter_tokens" and
"ip_adapter_drop_rate" set the embedding width, the token count and the loader's image-prompt dropout).  The loader adds image_embeds,
the adapter is written to <model>-ip-adapter (and -ip-adapter-EMA), and --cache-latents keeps the embeddings beside the moments.
--dpo BETA ("dpo_beta"; needs --lora RANK, with or without --dora): Diffusion-DPO preference training - the loader emits interleaved
(preferred, rejected) pairs under one caption (DataLoader(preference_pairs=True)), every step runs the frozen base as the reference
model beside the adapted one (train_step dpo_beta=; diffusers trains SD1.5 / SDXL with 5000), and the log shows the loss and
implicit_acc, the share of pairs the adapter ranks like the data.
--lora-conv R [--lora-conv-alpha A] ("lora_conv_rank", "lora_conv_alpha"; needs --lora RANK, refused with --dora): LoCon - rank-R adapters
also on the UNet's convolutions (ResNet conv1 / conv2 / conv_shortcut, the samplers' conv, SD1.5's 1x1 proj_in / proj_out), alpha A
(default R): kohya's conv_dim / conv_alpha.
--loha ("lora_algo": "loha"; needs --lora RANK, optionally --lora-conv R; ranks up to 32; refused with --dora): LoHa - every adapted kernel
carries four factors and the delta (alpha / rank) * (A1 B1) o (A2 B2), LyCORIS' algo=loha without Tucker."""
import argparse
import json
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist

from stable_diffusion_training_amd import dp, latent_cache, lora, nets, tokens
from stable_diffusion_training_amd import training_utils as tu
from stable_diffusion_training_amd.checkpoint import gather_rng_states, load_controlnet, load_ip_adapter, save_controlnet, save_ip_adapter
from stable_diffusion_training_amd.streamer import DataLoader


def delete_file_or_folder(path):
    if os.path.isdir(path):
        shutil.rmtree(path, ignore_errors=True)
    elif os.path.exists(path):
        os.remove(path)


def schedule_kwargs(config_dict):
    """on_device_model_training_state's lr_schedule / ema_schedule from the optional config keys (absent keys: the defaults)."""
    lr = {arg: config_dict[key] for key, arg in (("lr_warmup_steps", "num_warmup_steps"), ("lr_num_training_steps", "num_training_steps"),
                                                 ("lr_num_cycles", "num_cycles"), ("lr_power", "power"), ("lr_end", "lr_end"))
          if config_dict.get(key) is not None}
    ema = None
    if config_dict.get("ema_warmup"):
        ema = {arg: config_dict[key] for key, arg in (("ema_inv_gamma", "inv_gamma"), ("ema_power", "power"), ("ema_min_decay", "min_decay"),
                                                      ("ema_update_after_step", "update_after_step"),
                                                      ("ema_use_warmup_power", "use_ema_warmup"))
               if config_dict.get(key) is not None}
        ema["kind"] = "warmup"
    return dict(lr_schedule=lr or None, ema_schedule=ema)


def current_lr(state):
    """The learning rate of the store's last optimizer step (the schedule's value, or the constant rate)."""
    if state.opt_store is None:  # a frozen model (the UNet of a tokens-only run)
        return 0.0
    sched = state.opt_store.schedule
    return sched[0].rate(max(state.step - 1, 0)) if sched else state.hyper["lr"]


def lora_config(config_dict, world=1):
    """The lora= argument of on_device_model_training_state from "lora_rank" (--lora), "lora_alpha", "lora_dora" (--dora),
    "lora_conv_rank" (--lora-conv) and "lora_conv_alpha" (--lora-conv-alpha): rank-r adapters on the UNet's attention projections,
    with lora_conv_rank also LoCon adapters on its convolutions; frozen text encoder; alpha = rank unless given.  None without lora_rank."""
    if config_dict.get("lora_dora") and not config_dict.get("lora_rank"):
        raise ValueError("lora_dora: DoRA is a LoRA adapter with a trained magnitude - give lora_rank (--lora RANK --dora)")
    if (config_dict.get("lora_conv_rank") or config_dict.get("lora_conv_alpha") is not None) and not config_dict.get("lora_rank"):
        raise ValueError("lora_conv_rank: LoCon adapts the convolutions beside the attention projections - give lora_rank (--lora RANK --lora-conv R)")
    if config_dict.get("lora_conv_alpha") is not None and not config_dict.get("lora_conv_rank"):
        raise ValueError("lora_conv_alpha needs lora_conv_rank (--lora-conv R --lora-conv-alpha A)")
    algo = config_dict.get("lora_algo", "lora")
    if algo != "lora" and not config_dict.get("lora_rank"):
        raise ValueError("lora_algo: LoHa adapts the kernels --lora names - give lora_rank (--lora RANK --loha)")
    if algo == "loha" and config_dict.get("lora_dora"):
        raise ValueError("lora_algo: DoRA combined with LoHa is not supported (--loha with --dora)")
    if not config_dict.get("lora_rank"):
        return None
    if world > 1:
        raise ValueError("lora_rank: adapter training runs on one GPU (train_step refuses a reducer with adapter states)")
    r = int(config_dict["lora_rank"])
    conv = {}
    if config_dict.get("lora_conv_rank"):
        conv = dict(conv_rank=int(config_dict["lora_conv_rank"]),
                    conv_alpha=None if config_dict.get("lora_conv_alpha") is None else float(config_dict["lora_conv_alpha"]))
    if algo != "lora":  # (without it the configuration is what it was)
        conv["algo"] = algo
    return dict(unet=lora.LoraConfig(r, float(config_dict.get("lora_alpha", r)), dora=bool(config_dict.get("lora_dora", False)), **conv),
                text_encoder="frozen")


def main(config_dict, models=None, tokenizer=None, log=print):
    """models: optional load_models-style dict (tests pass seeded weights); otherwise read from config_dict["model_path"]."""
    assert len(config_dict["image_area_root"]) == len(config_dict["minimum_axis_length"]), \
        "number of elements in image_area_root and minimum_axis_length is not match! check your config files!"
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, pg_options=dp.rccl_group_options())
    training_config = tu.TrainingConfig.from_dict(config_dict)
    micro_batches = int(config_dict.get("micro_batches", 1))
    if config_dict["batch_size"] % (world * micro_batches):
        raise ValueError(f'batch_size {config_dict["batch_size"]} is not a multiple of world size x micro_batches ({world} x {micro_batches})')
    if models is None:
        models = tu.load_models(training_config)
        tokenizer = models["tokenizer"]
        if "tokenizer_2" in models:  # SDXL: save_model writes both
            tokenizer = (tokenizer, models["tokenizer_2"])
    inpaint = bool(config_dict.get("inpaint"))
    if inpaint and nets.inpaint_latent_channels(models["unet"]["config"]) is None:
        ucfg = models["unet"]["config"]
        params, ucfg = nets.widen_conv_in(models["unet"]["unet_params"], ucfg, 2 * int(ucfg["out_channels"]) + 1)
        models = dict(models, unet=dict(models["unet"], unet_params=params, config=ucfg))
    te_cfg = models["text_encoder"]["config"]
    sdxl = nets.sdxl_conditioning(te_cfg)  # an SDXL directory: two towers, pooled embedding from the text encoder
    vocab = te_cfg["towers"][0]["vocab_size"] if "towers" in te_cfg else te_cfg["vocab_size"]
    # masked / weighted loss: "masked_loss" is true or the floor (false / absent: off), "prior_loss_weight" a number (absent: off)
    masked_loss = config_dict.get("masked_loss", False)
    use_mask = masked_loss is not False and masked_loss is not None
    prior_w = config_dict.get("prior_loss_weight")
    if config_dict.get("normalize_masked_area") and not use_mask:
        raise ValueError("normalize_masked_area needs masked_loss (--masked-loss)")
    control = None
    if config_dict.get("controlnet"):  # a ControlNet on the frozen UNet: loaded from a directory, or initialised from the UNet
        if world > 1:
            raise ValueError("controlnet: ControlNet training runs on one GPU (train_step refuses a reducer with a ControlNet)")
        if isinstance(config_dict["controlnet"], str):
            control = load_controlnet(config_dict["controlnet"])
        else:
            f = 2 ** (len(models["vae"]["config"]["block_out_channels"]) - 1)
            control = dict(config=nets.controlnet_config(models["unet"]["config"], tuple(config_dict.get("controlnet_channels", (16, 32, 96, 256))),
                                                         vae_downscale=f))
    ip_cfg = None
    if config_dict.get("ip_adapter"):  # an IP-Adapter on the frozen UNet: loaded from a directory, or initialised from the UNet
        if world > 1:
            raise ValueError("ip_adapter: IP-Adapter training runs on one GPU (train_step refuses a reducer with an IP-Adapter)")
        if isinstance(config_dict["ip_adapter"], str):
            ip_cfg = load_ip_adapter(config_dict["ip_adapter"])
        else:
            ip_cfg = dict(config=nets.ip_adapter_config(models["unet"]["config"], int(config_dict.get("ip_adapter_embed_dim", 1024)),
                                                        int(config_dict.get("ip_adapter_tokens", 4))))
    loss_loader_kw = dict(inpaint_masks=inpaint, loss_masks=use_mask,
                          conditioning_images=int(control["config"]["conditioning_channels"]) if control is not None else False, prior_every=2 if prior_w is not None else 0,
                          prior_loss_weight=1.0 if prior_w is None else float(prior_w))
    if ip_cfg is not None:
        loss_loader_kw.update(image_embeds=int(ip_cfg["config"]["image_embed_dim"]),
                              image_embed_drop_rate=float(config_dict.get("ip_adapter_drop_rate", 0.05)))
    loss_overrides = {}
    if use_mask:
        loss_overrides = dict(masked_loss_floor=0.0 if masked_loss is True else float(masked_loss),
                              normalize_masked_area=bool(config_dict.get("normalize_masked_area", False)))
    # Huber / smooth-L1: "loss_type" (absent or "l2": the squared error), "huber_c", "huber_schedule"
    if config_dict.get("loss_type", "l2") != "l2":
        loss_overrides.update(loss_type=config_dict["loss_type"], huber_c=float(config_dict.get("huber_c", 0.1)),
                              huber_schedule=config_dict.get("huber_schedule", "snr"))
    dpo_beta = config_dict.get("dpo_beta")
    if dpo_beta is not None:  # Diffusion-DPO: pairs from the loader, the frozen base under the adapter as the reference
        if not config_dict.get("lora_rank"):
            raise ValueError("dpo_beta: preference training needs a LoRA / DoRA adapter - the frozen base is the reference model (--lora RANK)")
        loss_overrides["dpo_beta"] = float(dpo_beta)
        loss_loader_kw["preference_pairs"] = True
    token_cfg = None
    if config_dict.get("new_tokens"):  # textual inversion: placeholder j is id vocab + j of every tower
        if world > 1:
            raise ValueError("new_tokens: token training runs on one GPU (train_step refuses a reducer with new tokens)")
        init = config_dict.get("new_tokens_init_id")
        token_cfg = tokens.TokenConfig(int(config_dict["new_tokens"]), init_ids=None if init is None else int(init),
                                       seed=int(config_dict["master_seed"]), retract=bool(config_dict.get("new_tokens_retract", False)))
        towers = te_cfg["towers"] if "towers" in te_cfg else [te_cfg]
        loss_loader_kw["placeholder_ids"] = [[t["vocab_size"] + j for j in range(token_cfg.num_tokens)] for t in towers][: 2 if sdxl else 1]
    dataloader = DataLoader(
        tokenizer_obj=tokenizer, config=None, ramdisk_path=config_dict.get("ramdisk_path"),
        training_batch_size=config_dict["batch_size"], repeat_batch=config_dict["repeat_batch"],
        maximum_resolution_areas=[x ** 2 for x in config_dict["image_area_root"]],
        bucket_lower_bound_resolutions=config_dict["minimum_axis_length"],
        numb_of_worker_thread=config_dict.get("numb_of_dataloader_worker_thread", 1),
        queue_get_timeout=config_dict.get("queue_get_timeout", 60), chunk_number=config_dict["chunk_number"],
        seed=config_dict["master_seed"], context_concatenation_multiplier=config_dict["context_window_concatenation_count"],
        batches_per_chunk=config_dict.get("batches_per_chunk", 100), vocab_size=vocab,
        rank=rank, world_size=world, device=dev, text_towers=2 if sdxl else 1, **loss_loader_kw)
    dataloader._print_debug = bool(config_dict.get("DEBUG"))

    lora_cfg = lora_config(config_dict, world)
    train_rngs = torch.Generator(device=dev)
    train_rngs.manual_seed(config_dict["master_seed"] * 1009 + rank)  # different noise / timesteps on every shard
    (unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params, frozen_vae, frozen_schedulers,
     model_object_dict) = tu.on_device_model_training_state(training_config, models, device=dev, optimizer=config_dict.get("optimizer", "lion"),
                                                           **schedule_kwargs(config_dict), lora=lora_cfg, new_tokens=token_cfg, controlnet=control,
                                                           ip_adapter=ip_cfg)
    reducer = dp.GradReducer([unet_state.store, text_encoder_state.store]) if world > 1 else None
    train_step_funcs = tu.dp_compile_all_unique_resolution(
        unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params, frozen_vae, frozen_schedulers, training_config,
        reducer=reducer, per_device_batch=config_dict["batch_size"] // (world * micro_batches), micro_batches=micro_batches,
        step_overrides=dict(loss_overrides, **(dict(vae_scale=models["vae"]["config"].get("scaling_factor", 0.13025)) if sdxl else {})) or None)
    resume = config_dict.get("resume_training_state")
    if resume and os.path.exists(resume):
        tu.load_training_state(resume, unet_state, text_encoder_state, train_rngs, rank=rank, world=world)
        log(f"resumed optimizer / RNG state from {resume} at step {unet_state.step}")

    vae_params = frozen_vae.params  # what save_model writes as the VAE
    cache_dir = config_dict.get("cache_latents")
    if cache_dir:
        # encode every chunk this run visits, once, then train without the VAE: only its host tree stays, for the saves
        visits, n = [], config_dict["chunk_number"]
        for _ in range(config_dict["chunk_limit"]):
            n = 0 if n >= config_dict["chunk_limit"] else n
            visits.append(n)
            n += 1
        for n in dict.fromkeys(visits):
            dataloader.chunk_number = n
            dataloader.create_training_dataframe()
            dataloader.dispatch_worker()
            count = latent_cache.build(dataloader, frozen_vae, os.path.join(cache_dir, f"rank{rank}", f"chunk{n}"))
            log(f"cached the latent moments of chunk {n}: {count} batches")
        vae_params, frozen_vae = frozen_vae.params.full_tree, None
        torch.cuda.empty_cache()

    if rank == 0 and not os.path.isfile(config_dict["loss_csv"]):
        with open(config_dict["loss_csv"], "w") as f:
            f.write("steps, step_size, loss, time, chunk, seed\n")

    def save(ema):
        base = config_dict["model_path"].split("@")[0] + ("-EMA" if ema else "")
        # (a model without an EMA view - accumulate_*_ema off, or a text encoder frozen under LoRA - is saved as it stands)
        up = unet_ema_params if (ema and config_dict["accumulate_unet_ema"] and unet_ema_params is not None) else unet_state.params
        if unet_state.controlnet is not None or unet_state.ip_adapter is not None:
            up = unet_state.params  # the UNet EMA view wraps the ControlNet's / the IP-Adapter's store: the pipeline directory holds the frozen base either way
        tp = (text_encoder_ema_params if (ema and config_dict["accumulate_text_encoder_ema"] and text_encoder_ema_params is not None)
              else text_encoder_state.params)
        tu.save_model(model_object_dict, tokenizer, up, tp, vae_params, f'{base}@{config_dict["chunk_steps"]}')
        delete_file_or_folder(f'{base}@{config_dict["chunk_steps"] - config_dict["keep_trained_model_buffer"]}')

    losses = []
    for _ in range(config_dict["chunk_limit"]):
        if config_dict["chunk_number"] >= config_dict["chunk_limit"]:
            config_dict["chunk_number"] = 0
        dataloader.chunk_number = config_dict["chunk_number"]
        dataloader.grab_and_prefetch_chunk(numb_of_prefetched_batch=config_dict.get("numb_of_prefetched_batch", 1))
        dataloader.prepare_training_dataframe()
        dataloader.create_training_dataframe()
        dataloader.dispatch_worker()
        batches = dataloader
        if cache_dir:
            batches = latent_cache.Reader(os.path.join(cache_dir, f"rank{rank}", f'chunk{config_dict["chunk_number"]}'), device=dev)
        if reducer is not None:
            reducer.gather_state()  # sharded optimizer: whole state on every rank before the rank-0 save (collective; no-op otherwise)
        if rank == 0:  # pre-flight save (training.py:149-184): fail before the chunk, not after it
            tu.save_model(model_object_dict, tokenizer, unet_state.params, text_encoder_state.params, vae_params,
                          config_dict["test_save_path"])
            delete_file_or_folder(config_dict["test_save_path"])
        start = time.time()
        train_metrics, dpo_acc = [], []
        for count in range(int(dataloader._bulk_batch_count + dataloader._first_batch_count)):
            current_batch = batches.grab_next_batch()
            if current_batch == "end_of_batch":
                break
            if current_batch is None:
                continue
            w = config_dict["text_encoder_context_window"]
            rows = (-1, 2, w) if sdxl else (-1, w)  # SDXL: (B*k, 2, 77), one row of ids per tower
            current_batch["input_ids"] = current_batch["input_ids"].reshape(rows)
            if "attention_mask" in current_batch:  # unused by the step, and not kept by a latent cache
                current_batch["attention_mask"] = current_batch["attention_mask"].reshape(rows)
            (unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params, train_metric, train_rngs) = \
                train_step_funcs[tu.step_key(current_batch)](
                    unet_state, text_encoder_state, unet_ema_params, text_encoder_ema_params, current_batch, train_rngs,
                    frozen_vae, frozen_schedulers)
            train_metrics.append(train_metric["loss"])  # device scalars: reading them below is the only synchronisation
            if dpo_beta is not None:
                dpo_acc.append(train_metric["implicit_acc"])
            if count % config_dict["loss_logging_interval"] == 0:
                loss = float(sum(train_metrics) / len(train_metrics))
                losses.append(loss)
                elapsed = round(time.time() - start, 4)
                start = time.time()
                train_metrics = []
                acc = ""
                if dpo_acc:
                    acc, dpo_acc = f", implicit_acc {float(sum(dpo_acc) / len(dpo_acc)):.3f}", []
                if rank == 0:
                    opt_store = unet_state.opt_store  # Prodigy: lr multiplies the estimated d, which is worth a look beside the loss
                    d = f', unet d {float(opt_store.prodigy_d().item()):.4e}' if opt_store is not None and opt_store.optimizer == "prodigy" else ""
                    log(f'at steps {count}, avg loss for {config_dict["loss_logging_interval"]} steps: {loss}, took {elapsed} second(s), '
                        f'unet lr {current_lr(unet_state):.4e}{d}{acc}')
                    with open(config_dict["loss_csv"], "a") as f:
                        f.write(f'\n{count},{config_dict["loss_logging_interval"]},{loss},{elapsed},{config_dict["chunk_steps"]},{config_dict["master_seed"]}')
        rng_states = gather_rng_states(train_rngs)  # every rank resumes ITS noise / timestep stream (collective)
        if reducer is not None:
            reducer.gather_state()                  # ... and the sharded optimizer's state becomes whole (collective, all ranks)
        if rank == 0:
            save(ema=False)
            if config_dict["ema_rate"]:
                save(ema=True)
            state_path = config_dict["model_path"].split("@")[0] + "-state.safetensors"
            tu.save_training_state(state_path, unet_state, text_encoder_state, rng_states=rng_states)
            if unet_state.controlnet is not None:  # the ControlNet as a submodel directory of its own; its EMA, when there is one, beside it
                cbase = config_dict["model_path"].split("@")[0] + "-controlnet"
                save_controlnet(cbase, unet_state.controlnet, unet_state.controlnet.config)
                if config_dict["ema_rate"] and unet_ema_params is not None:
                    save_controlnet(cbase + "-EMA", unet_ema_params, unet_state.controlnet.config)
            if unet_state.ip_adapter is not None:  # the IP-Adapter as a directory of its own; its EMA, when there is one, beside it
                ibase = config_dict["model_path"].split("@")[0] + "-ip-adapter"
                save_ip_adapter(ibase, unet_state.ip_adapter, unet_state.ip_adapter.config)
                if config_dict["ema_rate"] and unet_ema_params is not None:
                    save_ip_adapter(ibase + "-EMA", unet_ema_params, unet_state.ip_adapter.config)
            if unet_state.adapter is not None:  # the adapter alone (the saves above hold the base with the adapter folded in)
                unet_state.adapter.save(config_dict["model_path"].split("@")[0] + "-lora.npz")
            if text_encoder_state.tokens is not None:  # the trained rows alone (the saves above hold the resized text encoder)
                text_encoder_state.tokens.save(config_dict["model_path"].split("@")[0] + "-tokens.npz")
        config_dict["model_path"] = f'{config_dict["model_path"].split("@")[0]}@{config_dict["chunk_steps"]}'  # training.py:301-304
        config_dict["chunk_number"] += 1
        config_dict["chunk_steps"] += 1
    if world > 1:
        dist.barrier()
    return losses, unet_state, text_encoder_state


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="model_properties.json")
    ap.add_argument("--micro-batches", type=int, default=None, help="gradient accumulation over K micro-batches per step")
    ap.add_argument("--optimizer", choices=("lion", "adamw", "prodigy"), default=None,
                    help="lion (the reference's, default); adamw: learning rates taken as given, 8-bit moments where the config quantises; "
                         "prodigy: learning-rate-free (the config's rates are not used, lr = 1 multiplies the estimated d, fp32 state)")
    ap.add_argument("--cache-latents", metavar="DIR", default=None,
                    help="encode the run's chunks once into a latent cache under DIR, drop the VAE and train from the cache")
    ap.add_argument("--lora", metavar="RANK", type=int, default=None,
                    help="train rank-RANK LoRA adapters on the UNet's attention projections (frozen base and text encoder) instead of every weight")
    ap.add_argument("--dora", action="store_true",
                    help="with --lora: DoRA - also train a per-output-feature magnitude of every adapted kernel (weight-decomposed LoRA)")
    ap.add_argument("--lora-conv", metavar="R", type=int, default=None,
                    help="with --lora: LoCon - also train rank-R adapters on the UNet's convolutions (kohya conv_dim); not with --dora")
    ap.add_argument("--lora-conv-alpha", metavar="A", type=float, default=None, help="with --lora-conv: the conv adapters' alpha (default R)")
    ap.add_argument("--loha", action="store_true",
                    help="with --lora (and --lora-conv): LoHa - Hadamard-product adapters, ranks up to 32 (LyCORIS algo=loha); not with --dora")
    ap.add_argument("--dpo", metavar="BETA", type=float, default=None,
                    help="with --lora: Diffusion-DPO preference training on (preferred, rejected) pairs against the frozen base (diffusers: 5000)")
    ap.add_argument("--new-tokens", metavar="N", type=int, default=None,
                    help="textual inversion: train N placeholder-token embeddings on the frozen text encoder (alone, or beside --lora)")
    ap.add_argument("--init-token", metavar="ID", type=int, default=None, help="with --new-tokens: start every new row as a copy of token ID")
    ap.add_argument("--retract", action="store_true", help="with --new-tokens: rescale the rows towards the table's std after every step")
    ap.add_argument("--masked-loss", metavar="FLOOR", type=float, nargs="?", const=0.0, default=None,
                    help="train with a loss mask per image; FLOOR in [0, 1] is the least weight of a position outside the mask (default 0)")
    ap.add_argument("--normalize-masked-area", action="store_true", default=None,
                    help="with --masked-loss: rescale each sample's loss by area / masked area")
    ap.add_argument("--prior-loss-weight", metavar="W", type=float, default=None,
                    help="every second sample is a class image whose loss counts W times (DreamBooth prior preservation)")
    ap.add_argument("--loss-type", choices=("l2", "huber", "smooth_l1"), default=None,
                    help="l2 (default); huber / smooth_l1: the pseudo-Huber losses, robust to outlier images and high-noise timesteps")
    ap.add_argument("--inpaint", action="store_true", default=None,
                    help="train an inpainting UNet (widened from the checkpoint's when it is not one) from batches with an inpaint mask")
    ap.add_argument("--controlnet", metavar="DIR", nargs="?", const=True, default=None,
                    help="train a ControlNet on the frozen UNet from batches with a conditioning image (DIR: continue a saved one)")
    ap.add_argument("--ip-adapter", metavar="DIR", nargs="?", const=True, default=None,
                    help="train an IP-Adapter on the frozen UNet from batches with image embeddings (DIR: continue a saved one)")
    ap.add_argument("--huber-c", metavar="C", type=float, default=None, help="the Huber threshold the schedule ends at (default 0.1)")
    ap.add_argument("--huber-schedule", choices=("constant", "exponential", "snr"), default=None,
                    help="how the threshold follows the timestep: snr (default), exponential or constant")
    args = ap.parse_args()
    if args.dora and args.lora is None:
        ap.error("--dora needs --lora RANK")
    if args.lora_conv is not None and args.lora is None:
        ap.error("--lora-conv needs --lora RANK")
    if args.loha and args.lora is None:
        ap.error("--loha needs --lora RANK")
    if args.loha and args.dora:
        ap.error("--loha is refused beside --dora (DoRA combined with LoHa is not supported)")
    if args.lora_conv_alpha is not None and args.lora_conv is None:
        ap.error("--lora-conv-alpha needs --lora-conv R")
    if args.dpo is not None and args.lora is None:
        ap.error("--dpo needs --lora RANK")
    if (args.init_token is not None or args.retract) and args.new_tokens is None:
        ap.error("--init-token / --retract need --new-tokens N")
    with open(args.config) as f:
        cfg = json.load(f)
    if args.micro_batches is not None:
        cfg["micro_batches"] = args.micro_batches
    if args.optimizer is not None:
        cfg["optimizer"] = args.optimizer
    if args.lora is not None:
        cfg["lora_rank"] = args.lora
    if args.dora:
        cfg["lora_dora"] = True
    if args.lora_conv is not None:
        cfg["lora_conv_rank"] = args.lora_conv
    if args.loha:
        cfg["lora_algo"] = "loha"
    if args.lora_conv_alpha is not None:
        cfg["lora_conv_alpha"] = args.lora_conv_alpha
    if args.new_tokens is not None:
        cfg["new_tokens"] = args.new_tokens
    if args.init_token is not None:
        cfg["new_tokens_init_id"] = args.init_token
    if args.retract:
        cfg["new_tokens_retract"] = True
    if args.cache_latents is not None:
        cfg["cache_latents"] = args.cache_latents
    if args.masked_loss is not None:
        cfg["masked_loss"] = args.masked_loss
    if args.normalize_masked_area:
        cfg["normalize_masked_area"] = True
    if args.prior_loss_weight is not None:
        cfg["prior_loss_weight"] = args.prior_loss_weight
    if args.loss_type is not None:
        cfg["loss_type"] = args.loss_type
    if args.dpo is not None:
        cfg["dpo_beta"] = args.dpo
    if args.inpaint:
        cfg["inpaint"] = True
    if args.controlnet is not None:
        cfg["controlnet"] = args.controlnet
    if args.ip_adapter is not None:
        cfg["ip_adapter"] = args.ip_adapter
    if args.huber_c is not None:
        cfg["huber_c"] = args.huber_c
    if args.huber_schedule is not None:
        cfg["huber_schedule"] = args.huber_schedule
    main(cfg)
