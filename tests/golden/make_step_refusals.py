"""Generates tests/golden/step_refusals.json: every refusal of the training layer that needs no device, by exception type and FULL
message (tests/test_step_refusals_cpu.py compares case by case).

  builder/...   create_lion_optimizer_states' ValueErrors for lora=, new_tokens=, controlnet= and ip_adapter=, on host-only `models`
                dicts of the tiny configs (every branch raises before a store is built)
  step/...      the refusals at the top of train_step for token, LoRA, ControlNet and IP-Adapter states, on stand-in states
  batch/...     every branch of _check_loss_entries, _check_inpaint_entries, _check_control_entries, _check_ip_entries and _check_batch:
                an entry of the wrong type, dtype, device ("meta"), shape or layout, a missing one, one without its state or UNet
  both/...      inputs that break two rules at once: the message is that of the rule that is checked first
  graph/...     a captured step's refusal of a batch that adds or drops a launch-selecting key (the capture itself is stubbed)
and the constants LOSS_KEYS, INPAINT_KEYS, CONTROL_KEYS, IP_KEYS.

The committed file is a pin, written by the training layer as it stood before the side networks were described once (nets.SIDE_NETWORKS):
a refactor reproduces it and does not regenerate it.  Regenerate only with a change that is meant to alter a message.
Run:  python tests/golden/make_step_refusals.py
"""
import contextlib
import json
import os
import sys
import types
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stable_diffusion_training_amd import lora, nets, tokens  # noqa: E402
from stable_diffusion_training_amd import training_utils as tu  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "step_refusals.json")
NS = types.SimpleNamespace
CPU = torch.device("cpu")
BF, F32 = torch.bfloat16, torch.float32
E, T = 64, 4
TINY_CH = (16, 16, 32, 32)
CN_SAME = ("block_out_channels", "down_block_types", "layers_per_block", "in_channels", "cross_attention_dim", "attention_head_dim",
           "use_linear_projection", "transformer_layers_per_block", "norm_num_groups", "addition_embed_type")
IP_SAME = ("block_out_channels", "down_block_types", "up_block_types", "layers_per_block", "cross_attention_dim", "attention_head_dim",
           "transformer_layers_per_block")


def record(fn):
    """[exception type, full message] of a case, or None for one that raises nothing."""
    try:
        fn()
    except Exception as e:  # noqa: BLE001  (the type is part of the record)
        return [type(e).__name__, str(e)]
    return None


# ------------------------------------------------------------------------------------------------ create_lion_optimizer_states
def _models(unet_cfg=None, vae=True, vae_blocks=None):
    m = {"unet": {"config": unet_cfg or nets.unet_config("tiny")}, "text_encoder": {"config": {}}}
    if vae:
        vcfg = nets.vae_config("tiny")
        m["vae"] = {"config": vcfg if vae_blocks is None else dict(vcfg, block_out_channels=tuple(vcfg["block_out_channels"][:vae_blocks]))}
    return m


def builder_cases():
    u = nets.unet_config("tiny")
    u9 = nets.unet_config("tiny", in_channels=9)
    ccfg, icfg = nets.controlnet_config(u, TINY_CH), nets.ip_adapter_config(u, E, T)
    lo = dict(unet=lora.LoraConfig(4, 4.0), text_encoder="frozen")
    te_lo = lora.LoraConfig(4, 4.0, targets=lora.CLIP_TARGETS)
    tok = tokens.TokenConfig(num_tokens=1)
    build = lambda models=None, **kw: tu.create_lion_optimizer_states(_models() if models is None else models, device="cpu", **kw)
    without = lambda cfg, *keys: {k: v for k, v in cfg.items() if k not in keys}
    cases = {}
    for name, cfg in (("ip_adapter", icfg), ("controlnet", ccfg)):
        c = lambda tag, name=name, **kw: cases.__setitem__(f"builder/{name}/{tag}", lambda: build(**kw))
        c("not-a-dict", **{name: "sd15"})
        c("no-config", **{name: dict(params={})})
        c("unknown-key", **{name: dict(config={"k": 1}, weights={})})
        c("beside-lora", lora=lo, **{name: dict(config=cfg)})
        c("beside-tokens", new_tokens=tok, **{name: dict(config=cfg)})
        c("no-text-state", train_text_encoder=False, **{name: dict(config=cfg)})
        c("no-unet-state", train_unet=False, **{name: dict(config=cfg, params={})})
        c("inpainting-unet", models=_models(u9), **{name: dict(config=dict(cfg, in_channels=9))})
        c("plain-unet-config", **{name: dict(config=u)})
    for k in IP_SAME:
        cases[f"builder/ip_adapter/differs-{k}"] = lambda k=k: build(ip_adapter=dict(config=dict(icfg, **{k: "other"})))
    for k in CN_SAME:
        cases[f"builder/controlnet/differs-{k}"] = lambda k=k: build(controlnet=dict(config=dict(ccfg, **{k: "other"})))
    cases.update({
        "builder/ip_adapter/beside-controlnet": lambda: build(ip_adapter=dict(config=icfg), controlnet=dict(config=ccfg)),
        "builder/ip_adapter/no-image_embed_dim": lambda: build(ip_adapter=dict(config=without(icfg, "image_embed_dim"))),
        "builder/ip_adapter/no-num_tokens": lambda: build(ip_adapter=dict(config=without(icfg, "num_tokens"))),
        "builder/ip_adapter/validator-num_tokens": lambda: build(ip_adapter=dict(config=dict(icfg, num_tokens=32))),
        "builder/ip_adapter/validator-image_embed_dim": lambda: build(ip_adapter=dict(config=dict(icfg, image_embed_dim=12))),
        "builder/ip_adapter/tuple-equals-list": lambda: build(ip_adapter=dict(config=dict(icfg, block_out_channels=list(u["block_out_channels"]),
                                                                                        cross_attention_dim="other"))),
        "builder/controlnet/no-embedding-channels": lambda: build(controlnet=dict(config=without(ccfg, "conditioning_embedding_out_channels"))),
        "builder/controlnet/no-conditioning_channels": lambda: build(controlnet=dict(config=without(ccfg, "conditioning_channels"))),
        "builder/controlnet/validator-entries": lambda: build(controlnet=dict(config=dict(ccfg, conditioning_embedding_out_channels=(16, 32)))),
        "builder/controlnet/validator-multiples": lambda: build(controlnet=dict(config=dict(ccfg, conditioning_embedding_out_channels=(16, 32, 100, 256)))),
        "builder/controlnet/validator-channels": lambda: build(controlnet=dict(config=dict(ccfg, conditioning_channels=0))),
        "builder/controlnet/downscale-of-the-vae": lambda: build(models=_models(vae_blocks=3), controlnet=dict(config=ccfg)),
        "builder/controlnet/downscale-without-a-vae": lambda: build(models=_models(vae=False),
                                                                    controlnet=dict(config=dict(ccfg, conditioning_embedding_out_channels=(16, 32, 96)))),
        "builder/new_tokens/not-a-config": lambda: build(models={}, new_tokens=dict(num_tokens=2)),
        "builder/new_tokens/no-unet-state": lambda: build(models={}, new_tokens=tok, train_unet=False),
        "builder/new_tokens/no-text-state": lambda: build(models={}, new_tokens=tok, train_text_encoder=False),
        "builder/new_tokens/text-encoder-lora": lambda: build(models={}, new_tokens=tok, lora=dict(unet=lora.LoraConfig(4, 4.0), text_encoder=te_lo)),
        "builder/lora/not-a-dict": lambda: build(models={}, lora="rank16"),
        "builder/lora/unknown-key": lambda: build(models={}, lora=dict(unet=lora.LoraConfig(4, 4.0), vae=None)),
        "builder/lora/full-unet-beside-adapted-text": lambda: build(models={}, lora=dict(unet=None, text_encoder=te_lo)),
        "builder/lora/no-unet-entry": lambda: build(models={}, lora=dict(text_encoder="frozen")),
        "builder/lora/text-encoder-string": lambda: build(models={}, lora=dict(unet=lora.LoraConfig(4, 4.0), text_encoder="trained")),
        "builder/lora/no-text-state": lambda: build(models={}, lora=dict(unet=lora.LoraConfig(4, 4.0)), train_text_encoder=False),
        "builder/lora/no-unet-state": lambda: build(models={}, lora=lo, train_unet=False),
        # two rules at once
        "both/builder/ip-controlnet-lora": lambda: build(ip_adapter=dict(config=icfg), controlnet=dict(config=ccfg), lora=lo),
        "both/builder/ip-tokens-controlnet": lambda: build(ip_adapter=dict(config=icfg), controlnet=dict(config=ccfg), new_tokens=tok),
        "both/builder/bad-ip-beside-lora": lambda: build(ip_adapter="sd15", lora=lo),
        "both/builder/ip-beside-a-bad-controlnet": lambda: build(ip_adapter=dict(config=icfg), controlnet="sd15"),
        "both/builder/ip-one-state-inpainting": lambda: build(models=_models(u9), ip_adapter=dict(config=icfg), train_unet=False),
        "both/builder/ip-inpainting-plain-config": lambda: build(models=_models(u9), ip_adapter=dict(config=u9)),
        "both/builder/ip-validator-and-differs": lambda: build(ip_adapter=dict(config=dict(icfg, num_tokens=32, layers_per_block="other"))),
        "both/builder/ip-differs-twice": lambda: build(ip_adapter=dict(config=dict(icfg, transformer_layers_per_block="other", up_block_types="other"))),
        "both/builder/controlnet-tokens-one-state": lambda: build(controlnet=dict(config=ccfg), new_tokens=tok, train_unet=False),
        "both/builder/controlnet-lora-and-tokens": lambda: build(controlnet=dict(config=ccfg), new_tokens=tok, lora=lo),
        "both/builder/controlnet-inpainting-differs": lambda: build(models=_models(u9), controlnet=dict(config=ccfg)),
        "both/builder/controlnet-validator-and-differs": lambda: build(controlnet=dict(config=dict(ccfg, conditioning_channels=0, in_channels="other"))),
        "both/builder/controlnet-differs-twice": lambda: build(controlnet=dict(config=dict(ccfg, norm_num_groups="other", in_channels="other"))),
        "both/builder/bad-controlnet-bad-tokens": lambda: build(controlnet="sd15", new_tokens=dict(num_tokens=2)),
        "both/builder/bad-tokens-bad-lora": lambda: build(models={}, new_tokens=dict(num_tokens=2), lora="rank16"),
        "both/builder/tokens-one-state-text-lora": lambda: build(models={}, new_tokens=tok, train_unet=False,
                                                                 lora=dict(unet=lora.LoraConfig(4, 4.0), text_encoder=te_lo)),
        "both/builder/lora-unknown-key-no-unet": lambda: build(models={}, lora=dict(vae=None)),
        "both/builder/lora-bad-entry-one-state": lambda: build(models={}, lora=dict(unet=None), train_unet=False),
    })
    return cases


# ------------------------------------------------------------------------------------------------ train_step's refusals
def _cn(cfg=None):
    return nets.ControlNet(NS(device=CPU, trainable=True), dict(conditioning_channels=3, conditioning_embedding_out_channels=TINY_CH) if cfg is None else cfg)


def _ipa():
    return nets.IPAdapter(NS(device=CPU, trainable=True), dict(image_embed_dim=E, num_tokens=T))


def _states(cin=4, trainable=False, text_trainable=False, unet=None, text=None, unet_store=None, text_store=None, text_time=False):
    """Stand-in states with every field; unet= / text= set state fields, unet_store= / text_store= set fields of their stores."""
    ucfg = dict(in_channels=cin, out_channels=4, addition_embed_type="text_time" if text_time else None)
    us = NS(config=ucfg, store=NS(device=CPU, trainable=trainable, **(unet_store or {})), adapter=None, tokens=None, controlnet=None, ip_adapter=None)
    ts = NS(config={}, store=NS(device=CPU, trainable=text_trainable, **(text_store or {})), adapter=None, tokens=None, controlnet=None,
            ip_adapter=None)
    for st, over in ((us, unet), (ts, text)):
        for k, v in (over or {}).items():
            setattr(st, k, v)
    return us, ts


SCHED = NS(call=None, params=None)
PX = torch.zeros(2, 3, 16, 16)
COND = torch.zeros(2, 3, 16, 16)
EMB = torch.zeros(2, E)
MOM = torch.zeros(2, 2, 3, 8, dtype=BF)


def _step(batch=None, reducer=None, vae="vae", **kw):
    us, ts = _states(**kw)
    return tu.train_step(us, ts, None, None, dict(pixel_values=PX) if batch is None else batch, None, vae, SCHED, reducer=reducer)


def step_cases():
    tk = object()
    tok = dict(text=dict(tokens=tk), text_store=dict(tokens=tk))  # a well-formed token pair: the state and its store carry the adapter
    ad = object()
    cn, ip = dict(controlnet=_cn()), dict(ip_adapter=_ipa())
    cn_batch, ip_batch = dict(pixel_values=PX, conditioning_pixel_values=COND), dict(pixel_values=PX, image_embeds=EMB)
    s = lambda **kw: (lambda: _step(**kw))
    cases = {
        "step/tokens/trainable-unet": s(trainable=True, **tok),
        "step/tokens/trainable-text": s(text_trainable=True, **tok),
        "step/tokens/text-adapter": s(text=dict(tokens=tk, adapter=ad), text_store=dict(tokens=tk)),
        "step/tokens/store-carries-others": s(text=dict(tokens=tk), text_store=dict(tokens=object())),
        "step/tokens/store-carries-none": s(text=dict(tokens=tk)),
        "step/tokens/reducer": s(reducer=object(), **tok),
        "step/tokens/on-the-unet-state": s(unet=dict(tokens=tk)),
        "step/tokens/on-the-text-store-only": s(text_store=dict(tokens=tk)),
        "step/tokens/on-the-unet-store-only": s(unet_store=dict(tokens=tk)),
        "step/lora/trainable-unet": s(trainable=True, unet=dict(adapter=ad)),
        "step/lora/trainable-text": s(text_trainable=True, unet=dict(adapter=ad)),
        "step/lora/text-adapter-alone": s(text=dict(adapter=ad)),
        "step/lora/reducer": s(reducer=object(), unet=dict(adapter=ad)),
        "step/sdxl-mode-with-text_embeds": lambda: tu.train_step(
            NS(config=dict(addition_embed_type="text_time")), NS(config=dict(towers=[{}, {}], sdxl_conditioning=True)), None, None,
            dict(text_embeds=0), None, None, SCHED),
    }
    for name, side, batch in (("controlnet", cn, cn_batch), ("ip_adapter", ip, ip_batch)):
        cases.update({
            f"step/{name}/reducer": s(batch=batch, reducer=object(), unet=side),
            f"step/{name}/unet-adapter": s(batch=batch, unet=dict(side, adapter=ad)),
            f"step/{name}/text-adapter": s(batch=batch, unet=side, text=dict(adapter=ad)),
            f"step/{name}/tokens": s(batch=batch, unet=side, **tok),
            f"step/{name}/adapter-on-the-unet-store": s(batch=batch, unet=side, unet_store=dict(adapter=ad)),
            f"step/{name}/inpainting-unet": s(batch=dict(batch, inpaint_mask=torch.zeros(2, 16, 16)), cin=9, unet=side),
            f"step/{name}/trainable-unet": s(batch=batch, trainable=True, unet=side),
            f"step/{name}/trainable-text": s(batch=batch, text_trainable=True, unet=side),
            f"step/{name}/on-the-text-state": s(batch=batch, text=side),
            f"step/{name}/key-without-the-state": s(batch=batch, trainable=True, text_trainable=True),
            f"step/{name}/state-without-the-key": s(unet=side),
            f"both/step/{name}-reducer-and-trainable": s(batch=batch, reducer=object(), trainable=True, unet=side),
            f"both/step/{name}-adapter-and-inpainting": s(batch=batch, cin=9, unet=dict(side, adapter=ad)),
            f"both/step/{name}-inpainting-and-trainable": s(batch=batch, cin=9, text_trainable=True, unet=side),
            f"both/step/{name}-tokens-and-reducer": s(batch=batch, reducer=object(), unet=side, **tok),
            f"both/step/{name}-mixed-token-modes": s(batch=batch, trainable=True, unet=side, **tok),
        })
    cases.update({
        "step/ip_adapter/beside-a-controlnet": s(batch=ip_batch, unet=dict(cn, **ip)),
        "both/step/controlnet-reducer-beside-ip": s(batch=ip_batch, reducer=object(), unet=dict(cn, **ip)),
        "both/step/ip-adapter-and-controlnet": s(batch=ip_batch, unet=dict(cn, adapter=ad, **ip)),
        "both/step/ip-trainable-beside-controlnet": s(batch=ip_batch, text_trainable=True, unet=dict(cn, **ip)),
        "both/step/tokens-mixed-and-reducer": s(reducer=object(), trainable=True, **tok),
        "both/step/lora-mixed-and-reducer": s(reducer=object(), trainable=True, unet=dict(adapter=ad)),
        "both/step/lora-reducer-bad-batch": s(batch={}, reducer=object(), unet=dict(adapter=ad)),
        "both/step/controlnet-key-and-ip-key-without-states": s(batch=dict(cn_batch, image_embeds=EMB), trainable=True, text_trainable=True),
        "both/step/controlnet-bad-batch-and-no-key": s(batch=dict(pixel_values=PX, latent_moments=MOM), unet=cn),
        "both/step/bad-loss-type-and-reducer": lambda: tu.train_step(*_states(unet=cn), None, None, {}, None, None, SCHED, reducer=object(),
                                                                     loss_type="l1"),
    })
    # stand-ins without the newer fields (states of the tests that came before them): read as None
    bare = lambda cin=4: NS(config=dict(in_channels=cin, out_channels=4, addition_embed_type=None), store=NS(device=CPU, trainable=True), adapter=None)
    cases["step/bare-states/key-without-the-state"] = lambda: tu.train_step(bare(), bare(), None, None, cn_batch, None, "vae", SCHED)
    cases["step/bare-states/inpainting-unet-without-its-mask"] = lambda: tu.train_step(bare(9), bare(), None, None, dict(pixel_values=PX), None,
                                                                                      "vae", SCHED)
    return cases


# ------------------------------------------------------------------------------------------------ the batch checkers
def _bad_entries(good, wrong_dtype):
    """{tag: value} of one entry broken one way at a time, and two ways at once (both/: the earlier rule's message)."""
    shape = tuple(good.shape)
    strided = torch.zeros(*shape[:-1], 2 * shape[-1], dtype=good.dtype)[..., ::2]
    longer = torch.zeros(shape[0] + 1, *shape[1:], dtype=good.dtype)
    return {"a-list": good.tolist(), "a-numpy-array": good.float().numpy(), "dtype": good.to(wrong_dtype), "device": good.to("meta"),
            "shape": longer, "rank": good[None], "strided": strided,
            "both:dtype-and-device": good.to(wrong_dtype).to("meta"), "both:device-and-shape": longer.to("meta"),
            "both:shape-and-strided": torch.zeros(shape[0] + 1, *shape[1:-1], 2 * shape[-1], dtype=good.dtype)[..., ::2],
            "both:dtype-and-strided": strided.to(wrong_dtype)[..., :]}


def _add(cases, group, name, good, wrong_dtype, call):
    for tag, bad in _bad_entries(good, wrong_dtype).items():
        both, _, t = tag.rpartition(":")
        cases[f"{'both/' if both else ''}batch/{group}/{name}-{t}"] = lambda bad=bad: call(bad)


def batch_cases():
    cases = {}
    plain, inp = dict(in_channels=4, out_channels=4), dict(in_channels=9, out_channels=4)
    px_batch, mom_batch = dict(pixel_values=torch.zeros(2, 3, 16, 24)), dict(latent_moments=torch.zeros(2, 2, 3, 8, dtype=BF))
    images = (("pixels", px_batch, (2, 16, 24)), ("cached", mom_batch, (2, 2, 3)))
    loss = lambda batch, floor=0.0, norm=False: tu._check_loss_entries(batch, CPU, floor, norm)
    for tag, floor in (("a-bool", True), ("a-string", "0.5"), ("negative", -0.1), ("above-one", 1.5), ("none", None)):
        cases[f"batch/loss/floor-{tag}"] = lambda floor=floor: loss(px_batch, floor=floor)
    cases["batch/loss/normalize-without-a-mask"] = lambda: loss(dict(px_batch, loss_weight=torch.zeros(2)), norm=True)
    cases["both/batch/loss/floor-and-normalize"] = lambda: loss(px_batch, floor=2, norm=True)
    cases["both/batch/loss/normalize-and-bad-weight"] = lambda: loss(dict(px_batch, loss_weight=torch.zeros(3)), norm=True)
    for where, image, grid in images:
        _add(cases, "loss", f"loss_mask-{where}", torch.zeros(*grid), torch.float64, lambda v, image=image: loss(dict(image, loss_mask=v)))
        _add(cases, "loss", f"loss_weight-{where}", torch.zeros(2), torch.float16, lambda v, image=image: loss(dict(image, loss_weight=v)))
        cases[f"both/batch/loss/mask-and-weight-{where}"] = lambda image=image: loss(dict(image, loss_mask=torch.zeros(1), loss_weight=torch.zeros(1)))
        # inpainting
        inpaint = lambda batch, cfg=inp: tu._check_inpaint_entries(batch, cfg, CPU)
        full = dict(image, inpaint_mask=torch.zeros(*grid))
        if where == "cached":
            full["masked_latent_moments"] = torch.zeros(2, 2, 3, 8, dtype=BF)
            _add(cases, "inpaint", "masked_latent_moments", full["masked_latent_moments"], F32,
                 lambda v, full=full: inpaint(dict(full, masked_latent_moments=v)))
            cases["batch/inpaint/cached-without-masked_latent_moments"] = lambda image=image, grid=grid: inpaint(dict(image, inpaint_mask=torch.zeros(*grid)))
            cases["batch/inpaint/masked_latent_moments-on-a-plain-unet"] = lambda image=image: inpaint(
                dict(image, masked_latent_moments=torch.zeros(2, 2, 3, 8, dtype=BF)), plain)
            cases["both/batch/inpaint/bad-mask-and-no-masked_latent_moments"] = lambda image=image: inpaint(dict(image, inpaint_mask=torch.zeros(1)))
            cases["both/batch/inpaint/bad-mask-and-bad-masked_latent_moments"] = lambda image=image: inpaint(
                dict(image, inpaint_mask=torch.zeros(1), masked_latent_moments=torch.zeros(1)))
        _add(cases, "inpaint", f"inpaint_mask-{where}", torch.zeros(*grid), torch.float64, lambda v, full=full: inpaint(dict(full, inpaint_mask=v)))
        cases[f"batch/inpaint/mask-on-a-plain-unet-{where}"] = lambda full=full: inpaint(full, plain)
        cases[f"batch/inpaint/no-mask-{where}"] = lambda image=image: inpaint(image)
        # ControlNet
        cn = _cn()
        control = lambda batch, cn=cn: tu._check_control_entries(batch, cn, CPU)
        _add(cases, "control", f"conditioning_pixel_values-{where}", torch.zeros(2, 3, 16, 24), torch.float64,
             lambda v, image=image: control(dict(image, conditioning_pixel_values=v)))
        cases[f"batch/control/channels-{where}"] = lambda image=image: control(dict(image, conditioning_pixel_values=torch.zeros(2, 1, 16, 24)))
        cases[f"batch/control/missing-{where}"] = lambda image=image: control(image)
        cases[f"batch/control/without-the-state-{where}"] = lambda image=image: control(dict(image, conditioning_pixel_values=torch.zeros(1)), None)
    cases["batch/control/downscale-4-cached"] = lambda: tu._check_control_entries(
        dict(mom_batch, conditioning_pixel_values=torch.zeros(2, 2, 16, 24)),
        _cn(dict(conditioning_channels=2, conditioning_embedding_out_channels=(16, 16, 32))), CPU)
    # IP-Adapter
    ipa = _ipa()
    ipe = lambda batch, ipa=ipa, rows=2: tu._check_ip_entries(batch, ipa, CPU, rows)
    _add(cases, "ip", "image_embeds", torch.zeros(2, E), torch.float64, lambda v: ipe(dict(image_embeds=v)))
    _add(cases, "ip", "image_embeds-bf16", torch.zeros(2, E, dtype=BF), torch.float16, lambda v: ipe(dict(image_embeds=v)))
    cases["batch/ip/width"] = lambda: ipe(dict(image_embeds=torch.zeros(2, E + 8)))
    cases["batch/ip/rows"] = lambda: ipe(dict(image_embeds=torch.zeros(2, E)), rows=3)
    cases["batch/ip/missing"] = lambda: ipe({})
    cases["batch/ip/without-the-state"] = lambda: ipe(dict(image_embeds=torch.zeros(1)), None)
    # _check_batch: which image, the cached moments themselves, then the inpainting and loss entries in that order
    check = lambda batch, cfg=plain, vae="vae", **kw: tu._check_batch(batch, cfg, vae, CPU, **kw)
    mom = mom_batch["latent_moments"]
    cases.update({
        "batch/image/masked_latent_moments-beside-pixels": lambda: check(dict(px_batch, masked_latent_moments=mom)),
        "batch/image/masked_latent_moments-alone": lambda: check(dict(masked_latent_moments=mom)),
        "batch/image/both": lambda: check(dict(px_batch, **mom_batch)),
        "batch/image/neither": lambda: check({}),
        "batch/image/pixels-without-a-vae": lambda: check(px_batch, vae=None),
        "batch/image/latent_moments-rank": lambda: check(dict(latent_moments=mom[0])),
        "batch/image/latent_moments-odd-width": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 7, dtype=BF))),
        "batch/image/latent_moments-channels": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 6, dtype=BF))),
        "batch/image/latent_moments-channels-inpainting": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 6, dtype=BF)), inp),
        "batch/image/text_time-without-time_ids": lambda: check(mom_batch, dict(plain, addition_embed_type="text_time")),
        "both/batch/image/all-three-keys": lambda: check(dict(px_batch, masked_latent_moments=mom, **mom_batch)),
        "both/batch/image/both-and-no-vae": lambda: check(dict(px_batch, **mom_batch), vae=None),
        "both/batch/image/odd-width-and-strided": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 14, dtype=BF)[..., ::2])),
        "both/batch/image/strided-and-channels": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 12, dtype=BF)[..., ::2])),
        "both/batch/image/channels-and-no-time_ids": lambda: check(dict(latent_moments=torch.zeros(2, 2, 3, 6, dtype=BF)),
                                                                    dict(plain, addition_embed_type="text_time")),
        "both/batch/image/no-time_ids-and-bad-mask": lambda: check(dict(mom_batch, loss_mask=torch.zeros(1)),
                                                                    dict(plain, addition_embed_type="text_time")),
        "both/batch/image/bad-moments-and-bad-mask": lambda: check(dict(latent_moments=mom.float(), loss_mask=torch.zeros(1))),
        "both/batch/image/no-vae-and-bad-mask": lambda: check(dict(px_batch, loss_mask=torch.zeros(1)), vae=None),
    })
    _add(cases, "image", "latent_moments", mom, F32, lambda v: check(dict(latent_moments=v)))
    del cases["batch/image/latent_moments-shape"]  # (a batch of another size is a good batch)
    for where, image, grid in images:
        bad = torch.zeros(1)
        cases[f"both/batch/image/loss_mask-and-inpaint_mask-{where}"] = lambda image=image: check(dict(image, loss_mask=bad, inpaint_mask=bad), inp)
        cases[f"both/batch/image/loss_mask-and-no-inpaint_mask-{where}"] = lambda image=image: check(dict(image, loss_mask=bad), inp)
        cases[f"both/batch/image/floor-and-inpaint_mask-on-a-plain-unet-{where}"] = lambda image=image: check(
            dict(image, inpaint_mask=bad), masked_loss_floor=3)
        cases[f"batch/image/floor-{where}"] = lambda image=image: check(image, masked_loss_floor=3)
        cases[f"batch/image/normalize-{where}"] = lambda image=image: check(image, normalize_masked_area=True)
    return cases


# ------------------------------------------------------------------------------------------------ a captured step's key guards
def _captured(batch):
    """A _GraphedStep that has "captured" `batch`: the capture runs with torch.cuda's graph machinery stubbed out."""
    st = NS(store=NS(count=1, device=CPU))
    step = tu._GraphedStep(lambda *a, **k: (None, None, None, None, {}, None), warmup=0)
    graph = NS(replay=lambda: None)
    with mock.patch.object(torch.cuda, "synchronize", lambda: None), mock.patch.object(torch.cuda, "CUDAGraph", lambda: graph), \
            mock.patch.object(torch.cuda, "graph_pool_handle", lambda: "pool"), \
            mock.patch.object(torch.cuda, "graph", lambda *a, **k: contextlib.nullcontext()), mock.patch.object(tu._GraphedStep, "_pool", None):
        step(st, st, None, None, batch, None, None, None)
    return lambda later, other=None: step(other or st, st, None, None, later, None, None, None)


def graph_cases():
    z = torch.zeros(1)
    keys = dict(loss_mask=z, loss_weight=z, inpaint_mask=z, conditioning_pixel_values=z, image_embeds=z)
    plain = dict(pixel_values=z)
    pick = lambda *names: dict(plain, **{k: keys[k] for k in names})
    cases = {}
    for k in keys:
        cases[f"graph/adds-{k}"] = lambda k=k: _captured(plain)(pick(k))
        cases[f"graph/drops-{k}"] = lambda k=k: _captured(pick(k))(plain)
    cases.update({
        "graph/mask-for-weight": lambda: _captured(pick("loss_mask"))(pick("loss_weight")),
        "graph/drops-one-of-two-loss-keys": lambda: _captured(pick("loss_mask", "loss_weight"))(pick("loss_weight")),
        "graph/other-states": lambda: _captured(plain)(plain, NS(store=NS(count=1, device=CPU))),
        "both/graph/loss-and-inpaint": lambda: _captured(plain)(pick("loss_weight", "inpaint_mask")),
        "both/graph/inpaint-and-control": lambda: _captured(pick("inpaint_mask"))(pick("conditioning_pixel_values")),
        "both/graph/control-and-ip": lambda: _captured(pick("conditioning_pixel_values"))(pick("image_embeds")),
        "both/graph/all-four": lambda: _captured(pick(*keys))(plain),
    })
    return cases


def all_cases():
    """{case id: thunk}; record(thunk) is what the golden file holds."""
    return {**builder_cases(), **step_cases(), **batch_cases(), **graph_cases()}


def constants():
    return {k: list(getattr(tu, k)) for k in ("LOSS_KEYS", "INPAINT_KEYS", "CONTROL_KEYS", "IP_KEYS")}


def main():
    out = dict(cases={k: record(fn) for k, fn in all_cases().items()}, constants=constants())
    quiet = sorted(k for k, v in out["cases"].items() if v is None)
    if quiet:
        raise SystemExit(f"cases that raise nothing: {quiet}")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    kinds = sorted({v[0] for v in out["cases"].values()})
    print(f"{len(out['cases'])} cases ({sum(k.startswith('both/') for k in out['cases'])} break two rules), {kinds} -> {OUT}")


if __name__ == "__main__":
    main()
