"""Checkpoint I/O around train_step: the diffusers / transformers Flax directory layout the
reference reads (`load_models`, training_utils.py:177-250) and writes (`save_model`, training_utils.py:986-1025, called
from training.py:151-184 and :262-299), plus what the reference lacks: the optimizer state (8-bit Lion codes + scales,
fp32 momenta, EMA, step count) and the sampling RNG, so a run can resume bit-exactly.

The reference delegates the file formats to third-party code that is not vendored under /root/reference:
  * flax.serialization.to_bytes / from_bytes (flax 0.7.x, pinned by diffusers 0.21.4 / requirements.txt): msgpack of the
    nested parameter dict; an ndarray is ExtType(1, msgpack((shape, dtype.name, C-order bytes))), a numpy scalar ExtType(3,
    same payload), a python complex ExtType(2, msgpack((re, im))); arrays above 2**30 bytes are replaced by
    {"__msgpack_chunked_array__": True, "shape": {"0": ..}, "chunks": {"0": ..}}.  Restated here from that published
    format (flax is not installed in this image: the byte-level known-answer test in tests/test_checkpoint_cpu.py is built
    from the format description, not from flax output - "parity unpinned" for this file format).
  * diffusers FlaxModelMixin.save_pretrained / FlaxDiffusionPipeline.save_pretrained: <sub>/config.json +
    <sub>/diffusion_flax_model.msgpack, model_index.json; transformers FlaxPreTrainedModel: config.json + flax_model.msgpack.

Host-side code: parameters cross PCIe once per save (the reference's save forces the same device->host transfer).
"""
import hashlib
import json
import os

import msgpack
import numpy as np
import torch

from . import nets, optimizers
from .params import EmaView, ParamStore

DIFFUSERS_VERSION = "0.21.4"  # the version the reference pins
MAX_CHUNK_SIZE = 2 ** 30      # flax.serialization.MAX_CHUNK_SIZE
_EXT_NDARRAY, _EXT_NATIVE_COMPLEX, _EXT_NPSCALAR = 1, 2, 3

UNET_WEIGHTS = "diffusion_flax_model.msgpack"   # diffusers FLAX_WEIGHTS_NAME
CLIP_WEIGHTS = "flax_model.msgpack"             # transformers FLAX_WEIGHTS_NAME


# ----------------------------------------------------------------------------- flax msgpack
def _ndarray_payload(arr):
    arr = np.asarray(arr)
    if arr.dtype.hasobject:
        raise ValueError("object arrays cannot be serialised")
    return msgpack.packb((arr.shape, arr.dtype.name, arr.tobytes("C")), use_bin_type=True)


def _ext_pack(x):
    if isinstance(x, np.ndarray):
        return msgpack.ExtType(_EXT_NDARRAY, _ndarray_payload(x))
    if isinstance(x, np.generic):
        return msgpack.ExtType(_EXT_NPSCALAR, _ndarray_payload(x))
    if isinstance(x, complex):
        return msgpack.ExtType(_EXT_NATIVE_COMPLEX, msgpack.packb((x.real, x.imag)))
    return x


def _ndarray_from_payload(data):
    shape, dtype_name, buf = msgpack.unpackb(data, raw=True)
    name = dtype_name.decode() if isinstance(dtype_name, bytes) else dtype_name
    if name == "bfloat16":  # numpy has no bfloat16: widen to float32 (exact)
        u = np.frombuffer(buf, dtype=np.uint16).astype(np.uint32) << 16
        return u.view(np.float32).reshape(shape)
    return np.frombuffer(buf, dtype=np.dtype(name)).reshape(shape, order="C")


def _ext_unpack(code, data):
    if code == _EXT_NDARRAY:
        return _ndarray_from_payload(data)
    if code == _EXT_NPSCALAR:
        return _ndarray_from_payload(data)[()]
    if code == _EXT_NATIVE_COMPLEX:
        re, im = msgpack.unpackb(data)
        return complex(re, im)
    return msgpack.ExtType(code, data)


def _chunk_leaves(tree):
    if isinstance(tree, dict):
        return {k: _chunk_leaves(v) for k, v in tree.items()}
    if isinstance(tree, np.ndarray) and tree.size * tree.dtype.itemsize > MAX_CHUNK_SIZE:
        per = max(1, MAX_CHUNK_SIZE // tree.dtype.itemsize)
        flat = tree.reshape(-1)
        return {"__msgpack_chunked_array__": True, "shape": {str(i): int(d) for i, d in enumerate(tree.shape)},
                "chunks": {str(i): flat[o: o + per] for i, o in enumerate(range(0, flat.size, per))}}
    return tree


def _unchunk_leaves(tree):
    if not isinstance(tree, dict):
        return tree
    if "__msgpack_chunked_array__" in tree:
        shape = tuple(tree["shape"][str(i)] for i in range(len(tree["shape"])))
        return np.concatenate([tree["chunks"][str(i)] for i in range(len(tree["chunks"]))]).reshape(shape)
    return {k: _unchunk_leaves(v) for k, v in tree.items()}


def flax_to_bytes(tree):
    """flax.serialization.to_bytes of a nested dict of numpy arrays / scalars."""
    return msgpack.packb(_chunk_leaves(tree), default=_ext_pack, strict_types=True)


def _bin_header(n):
    if n < 256:
        return bytes([0xC4, n])
    if n < 65536:
        return bytes([0xC5]) + n.to_bytes(2, "big")
    return bytes([0xC6]) + n.to_bytes(4, "big")


def _ext_header(n, code):
    if n in (1, 2, 4, 8, 16):
        return bytes([{1: 0xD4, 2: 0xD5, 4: 0xD6, 8: 0xD7, 16: 0xD8}[n], code])
    if n < 256:
        return bytes([0xC7, n, code])
    if n < 65536:
        return bytes([0xC8]) + n.to_bytes(2, "big") + bytes([code])
    return bytes([0xC9]) + n.to_bytes(4, "big") + bytes([code])


def flax_write(f, tree):
    """flax_to_bytes(tree) streamed into the binary file f, byte for byte the same output, without materialising it: array
    payloads go from the numpy buffer straight to the file (a 3.4 GB UNet would otherwise be copied three times)."""
    packer = msgpack.Packer(default=_ext_pack, strict_types=True, autoreset=True)

    def emit(node):
        if isinstance(node, dict):
            f.write(packer.pack_map_header(len(node)))
            for k, v in node.items():
                f.write(packer.pack(k))
                emit(v)
        elif isinstance(node, np.ndarray) and not node.dtype.hasobject and node.nbytes >= 4096:
            arr = np.ascontiguousarray(node)
            prefix = bytes([0x93]) + msgpack.packb(arr.shape) + msgpack.packb(arr.dtype.name) + _bin_header(arr.nbytes)
            f.write(_ext_header(len(prefix) + arr.nbytes, _EXT_NDARRAY))
            f.write(prefix)
            f.write(memoryview(arr).cast("B"))
        else:
            f.write(packer.pack(node))

    emit(_chunk_leaves(tree))


def flax_from_bytes(data):
    """flax.serialization.msgpack_restore: nested dict of numpy arrays."""
    return _unchunk_leaves(msgpack.unpackb(data, ext_hook=_ext_unpack, raw=False, strict_map_key=False))


# ----------------------------------------------------------------------------- trees
def flatten_tree(tree, prefix=""):
    """Nested Flax parameter dict -> {"a/b/kernel": leaf} (the path form ParamStore.load and create_mask use)."""
    out = {}
    for k, v in tree.items():
        p = f"{prefix}/{k}" if prefix else str(k)
        if isinstance(v, dict):
            out.update(flatten_tree(v, p))
        else:
            out[p] = v
    return out


def flatten_if_nested(tree):
    """A parameter tree in the path form, whichever form it came in (flat trees pass through as they are)."""
    return flatten_tree(tree) if any(isinstance(v, dict) for v in tree.values()) else tree


def unflatten_tree(flat):
    out = {}
    for p, v in flat.items():
        node = out
        parts = p.split("/")
        for k in parts[:-1]:
            node = node.setdefault(k, {})
        node[parts[-1]] = v
    return out


def _to_numpy(v):
    if torch.is_tensor(v):
        v = v.detach()
        if v.dtype == torch.bfloat16:
            v = v.float()
        return v.cpu().numpy()
    return np.asarray(v)


def params_to_tree(params):
    """Whatever the training loop holds as `params` -> nested dict of host numpy arrays: a ParamStore / TrainState (its fp32
    master), an EmaView (the EMA buffer), or a flat / nested dict of tensors."""
    if hasattr(params, "store") and isinstance(params.store, ParamStore) and not isinstance(params, EmaView):
        params = params.store
    if isinstance(params, ParamStore) and getattr(params, "full_tree", None) is not None:
        flat = flatten_tree(params.full_tree)  # frozen VAE: the device store holds the encoder half only
    elif isinstance(params, EmaView) and getattr(params.store, "lora_of", None) is not None:
        flat = params.store.lora_of.folded(source="ema")  # the EMA of a LoRA adapter, folded into its frozen base
    elif isinstance(params, EmaView) and getattr(params.store, "tokens_of", None) is not None:
        flat = params.store.tokens_of.resized_tree("ema")  # the EMA of the new tokens behind the frozen base's token table
    elif isinstance(params, EmaView):
        flat = params.store.export_host("ema")
    elif isinstance(params, ParamStore) and getattr(params, "tokens", None) is not None:
        flat = params.tokens.resized_tree("master")  # a frozen text encoder with its new tokens: the (V + n)-row table
    elif isinstance(params, ParamStore) and getattr(params, "adapter", None) is not None:
        flat = params.adapter.folded()  # a frozen base with its LoRA adapter folded in: an ordinary checkpoint
    elif isinstance(params, ParamStore):
        flat = params.export_host("master")
    elif isinstance(params, dict):
        flat = flatten_tree(params)
    else:
        raise TypeError(f"cannot serialise parameters of type {type(params).__name__}")
    return unflatten_tree({p: _to_numpy(v) for p, v in flat.items()})


# ----------------------------------------------------------------------------- configs
def _jsonable(cfg):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}


def _write_json(path, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=2, sort_keys=True)
        f.write("\n")


def _read_config(path, defaults=None):
    with open(path) as f:
        raw = json.load(f)
    cfg = dict(defaults or {})
    for k, v in raw.items():
        if not k.startswith("_"):
            cfg[k] = tuple(v) if isinstance(v, list) else v
    return cfg


def _write_submodel(out_dir, sub, config, header, weights_name, params):
    d = os.path.join(out_dir, sub)
    os.makedirs(d, exist_ok=True)
    cfg = dict(header)
    cfg.update(_jsonable(config))
    _write_json(os.path.join(d, "config.json"), cfg)
    tmp = os.path.join(d, weights_name + ".tmp")
    with open(tmp, "wb") as f:
        flax_write(f, params_to_tree(params))
    os.replace(tmp, os.path.join(d, weights_name))  # a crash mid-write never leaves a truncated checkpoint under the final name


def _model_config(model_object_dict, key):
    m = model_object_dict[key]
    if isinstance(m, dict) and "config" in m and isinstance(m["config"], dict):
        return m["config"]
    if isinstance(m, dict):
        return m
    return dict(getattr(m, "config"))


def _tokens_of(params):
    """The tokens.TokenAdapter behind what save_model was handed as text_encoder_params (a TrainState, its frozen store, or the EmaView
    of the token store), or None."""
    if isinstance(params, EmaView):
        return getattr(params.store, "tokens_of", None)
    store = params.store if hasattr(params, "store") and isinstance(params.store, ParamStore) else params
    return getattr(store, "tokens", None) if isinstance(store, ParamStore) else None


def _resized_text_config(te_cfg, tk):
    """The text-encoder config with vocab_size = V + n, as after transformers' resize_token_embeddings (every tower of a two-tower one),
    and num_new_tokens = n: the tokenizer's special ids stay where they were, below the new rows (pipeline._uncond_ids)."""
    n = tk.num_tokens
    grow = lambda t: dict(t, vocab_size=t["vocab_size"] + n, num_new_tokens=t.get("num_new_tokens", 0) + n)
    if "towers" in te_cfg:
        return dict(te_cfg, towers=[grow(t) for t in te_cfg["towers"]])
    return grow(te_cfg)


# ----------------------------------------------------------------------------- the reference's two entry points
def save_model(model_object_dict, tokenizer_object, unet_params, text_encoder_params, vae_params, output_dir):
    """training_utils.py:986-1025: write a FlaxStableDiffusionPipeline directory (a FlaxStableDiffusionXLPipeline one when the text
    encoder has two towers: _save_sdxl).  The scheduler entry is the reference's hard-coded DDIM placeholder (scaled_linear,
    v_prediction, :998-1004), whatever the run trained with.
    A text encoder that carries new tokens (tokens.attach) is written resized: its token table holds the V base rows followed by the n
    trained ones and its config's vocab_size is V + n, so the directory loads into a plain store of this project."""
    ustore = unet_params.store if hasattr(unet_params, "store") else unet_params
    for net in nets.SIDE_NETWORKS:
        if getattr(ustore, net.marker, None) is not None:
            raise ValueError(f"save_model: unet_params is (the EMA view of) {net.article}'s store, not a UNet: pass the frozen UNet "
                             f"(unet_state.params) here and write {net.the} with save_{net.name}")
    os.makedirs(output_dir, exist_ok=True)
    dv = {"_diffusers_version": DIFFUSERS_VERSION}
    _write_submodel(output_dir, "unet", _model_config(model_object_dict, "unet"),
                    {"_class_name": "FlaxUNet2DConditionModel", **dv}, UNET_WEIGHTS, unet_params)
    _write_submodel(output_dir, "vae", _model_config(model_object_dict, "vae"),
                    {"_class_name": "FlaxAutoencoderKL", **dv}, UNET_WEIGHTS, vae_params)
    te_cfg = _model_config(model_object_dict, "text_encoder")
    tk = _tokens_of(text_encoder_params)
    if tk is not None:
        te_cfg = _resized_text_config(te_cfg, tk)
    if "towers" not in te_cfg:
        _write_submodel(output_dir, "text_encoder", te_cfg,
                        {"architectures": ["CLIPTextModel"], "model_type": "clip_text_model"}, CLIP_WEIGHTS, text_encoder_params)
    os.makedirs(os.path.join(output_dir, "scheduler"), exist_ok=True)
    _write_json(os.path.join(output_dir, "scheduler", "scheduler_config.json"),
                {"_class_name": "FlaxDDIMScheduler", **dv, "beta_start": 0.00085, "beta_end": 0.012,
                 "beta_schedule": "scaled_linear", "num_train_timesteps": 1000, "prediction_type": "v_prediction",
                 "set_alpha_to_one": True, "steps_offset": 0, "trained_betas": None})
    if "towers" in te_cfg:  # SDXL: the one two-tower store is written as the pipeline's two text encoders
        _save_sdxl(output_dir, dv, te_cfg, tokenizer_object, text_encoder_params)
        return
    index = {"_class_name": "FlaxStableDiffusionPipeline", **dv,
             "scheduler": ["diffusers", "FlaxDDIMScheduler"], "text_encoder": ["transformers", "FlaxCLIPTextModel"],
             "tokenizer": ["transformers", "CLIPTokenizer"], "unet": ["diffusers", "FlaxUNet2DConditionModel"],
             "vae": ["diffusers", "FlaxAutoencoderKL"],
             # save_pretrained records every registered module, None ones as [null, null]; from_pretrained expects the entries
             "safety_checker": [None, None], "feature_extractor": [None, None]}
    if tokenizer_object is not None:
        tokenizer_object.save_pretrained(os.path.join(output_dir, "tokenizer"))
    _write_json(os.path.join(output_dir, "model_index.json"), index)
    print("f model saved ")  # the reference's message, verbatim (training_utils.py:1025)


def save_controlnet(output_dir, controlnet, config):
    """A diffusers-Flax ControlNet submodel directory: config.json (FlaxControlNetModel) and the msgpack weights file.  controlnet: a
    nets.ControlNet, its ParamStore, the EmaView over it (the EMA weights) or a flat / nested host tree; config: nets.controlnet_config."""
    _write_submodel(output_dir, "", config, {"_class_name": "FlaxControlNetModel", "_diffusers_version": DIFFUSERS_VERSION},
                    UNET_WEIGHTS, controlnet)


def load_controlnet(directory):
    """Inverse of save_controlnet: dict(config=, params=flat {"path": float32 tensor} host tree), what
    on_device_model_training_state(controlnet=) and StableDiffusionPipeline(controlnet=) build their stores from."""
    cfg = _read_config(os.path.join(directory, "config.json"), nets._UNET_DEFAULTS)
    for k in ("conditioning_embedding_out_channels", "conditioning_channels"):
        if k not in cfg:
            raise ValueError(f"{directory}: config.json has no {k}: not a ControlNet directory")
    path = os.path.join(directory, UNET_WEIGHTS)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: expected the ControlNet's Flax weights")
    with open(path, "rb") as f:
        flat = flatten_tree(flax_from_bytes(f.read()))
    return {"config": cfg, "params": {p: torch.from_numpy(np.array(v, dtype=np.float32)) for p, v in flat.items()}}


def save_ip_adapter(output_dir, ip_adapter, config):
    """An IP-Adapter directory in this project's layout: config.json (the UNet's config plus image_embed_dim and num_tokens) and the
    msgpack weights file under the leaf paths of nets.ip_adapter_spec (DESIGN.md "IP-Adapter" maps them to the published state-dict
    names).  ip_adapter: a nets.IPAdapter, its ParamStore, the EmaView over it (the EMA weights) or a flat / nested host tree."""
    _write_submodel(output_dir, "", config, {"_class_name": "IPAdapter", "_diffusers_version": DIFFUSERS_VERSION}, UNET_WEIGHTS, ip_adapter)


def load_ip_adapter(directory):
    """Inverse of save_ip_adapter: dict(config=, params=flat {"path": float32 tensor} host tree), what
    on_device_model_training_state(ip_adapter=) and StableDiffusionPipeline(ip_adapter=) build their stores from."""
    cfg = _read_config(os.path.join(directory, "config.json"), nets._UNET_DEFAULTS)
    for k in ("image_embed_dim", "num_tokens"):
        if k not in cfg:
            raise ValueError(f"{directory}: config.json has no {k}: not an IP-Adapter directory")
    path = os.path.join(directory, UNET_WEIGHTS)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: expected the IP-Adapter's weights")
    with open(path, "rb") as f:
        flat = flatten_tree(flax_from_bytes(f.read()))
    return {"config": cfg, "params": {p: torch.from_numpy(np.array(v, dtype=np.float32)) for p, v in flat.items()}}


# keys of a tower config that describe how this project runs it, not the transformers model: not written to config.json
_RUN_KEYS = ("hidden_layer", "with_projection")
SDXL_PIPELINE = "FlaxStableDiffusionXLPipeline"


def _tower_json(cfg):
    return {k: v for k, v in cfg.items() if k not in _RUN_KEYS}


def _save_sdxl(output_dir, dv, te_cfg, tokenizer_object, text_encoder_params):
    """The rest of save_model for a two-tower text encoder: text_encoder/ (CLIPTextModel) and text_encoder_2/
    (CLIPTextModelWithProjection, with text_projection) split out of the store by their prefixes, and the XL pipeline index.
    tokenizer_object: None, one tokenizer, or (tokenizer, tokenizer_2)."""
    tree = params_to_tree(text_encoder_params)
    index = {"_class_name": SDXL_PIPELINE, **dv, "scheduler": ["diffusers", "FlaxDDIMScheduler"],
             "unet": ["diffusers", "FlaxUNet2DConditionModel"], "vae": ["diffusers", "FlaxAutoencoderKL"],
             "tokenizer": ["transformers", "CLIPTokenizer"], "tokenizer_2": ["transformers", "CLIPTokenizer"]}
    for tower, prefix in zip(te_cfg["towers"], te_cfg["prefixes"]):
        sub = prefix.rstrip("/")
        arch = "CLIPTextModelWithProjection" if tower.get("with_projection") else "CLIPTextModel"
        _write_submodel(output_dir, sub, _tower_json(tower), {"architectures": [arch], "model_type": "clip_text_model"},
                        CLIP_WEIGHTS, tree[sub])
        index[sub] = ["transformers", "Flax" + arch]
    toks = tokenizer_object if isinstance(tokenizer_object, (tuple, list)) else (tokenizer_object, None)
    for name, tok in zip(("tokenizer", "tokenizer_2"), toks):
        if tok is not None:
            tok.save_pretrained(os.path.join(output_dir, name))
    _write_json(os.path.join(output_dir, "model_index.json"), index)
    print("f model saved ")


def is_sdxl_dir(root):
    """An SDXL pipeline directory: a text_encoder_2/ sub-folder, or an XL pipeline index."""
    if os.path.isdir(os.path.join(root, "text_encoder_2")):
        return True
    idx = os.path.join(root, "model_index.json")
    if os.path.exists(idx):
        with open(idx) as f:
            return json.load(f).get("_class_name") == SDXL_PIPELINE
    return False


def sdxl_text_config(cfg1, cfg2):
    """The SDXL-mode two-tower config (nets.dual_clip_config(sdxl_conditioning=True)) of the two text encoders' config.json
    contents: CLIP-L and bigG with their own widths, activations, projection_dim and eos_token_id."""
    t1 = {k: v for k, v in cfg1.items() if k not in ("projection_dim", "eos_token_id")}  # CLIP-L: no projection, no pooling
    return nets.dual_clip_config(t1, dict(cfg2), sdxl_conditioning=True)


def load_models(training_config, load_tokenizer=True):
    """training_utils.py:177-250: read the pipeline directory at training_config.model_path.  Returns the dict
    on_device_model_training_state() takes: {"unet": {"unet_params", "config"}, "vae": {...}, "text_encoder": {...},
    "tokenizer": CLIPTokenizer | None} (+ "tokenizer_2" for SDXL); parameter trees are flat {"path/with/slashes": float32 tensor} on the host (the
    reference loads fp32 masters and computes in bf16, :209-222)."""
    root = training_config.model_path

    def weights(sub, name):
        path = os.path.join(root, sub, name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: expected Flax weights (the reference loads Flax checkpoints, training_utils.py:209-222)")
        with open(path, "rb") as f:
            flat = flatten_tree(flax_from_bytes(f.read()))
        return {p: torch.from_numpy(np.array(v, dtype=np.float32)) for p, v in flat.items()}  # a writable fp32 copy

    unet_cfg = _read_config(os.path.join(root, "unet", "config.json"), nets._UNET_DEFAULTS)
    vae_cfg = _read_config(os.path.join(root, "vae", "config.json"))
    clip_cfg = _read_config(os.path.join(root, "text_encoder", "config.json"))
    te_params = weights("text_encoder", CLIP_WEIGHTS)
    sdxl = is_sdxl_dir(root)
    if sdxl:  # both towers in one store, under the sub-folder names (nets.dual_clip_config), in SDXL mode
        clip_cfg = sdxl_text_config(clip_cfg, _read_config(os.path.join(root, "text_encoder_2", "config.json")))
        te_params = {**{"text_encoder/" + p: v for p, v in te_params.items()},
                     **{"text_encoder_2/" + p: v for p, v in weights("text_encoder_2", CLIP_WEIGHTS).items()}}
    tokenizer = tokenizer_2 = None
    if load_tokenizer and os.path.isdir(os.path.join(root, "tokenizer")):
        from transformers import CLIPTokenizer
        tokenizer = CLIPTokenizer.from_pretrained(root, subfolder="tokenizer")
    if load_tokenizer and sdxl and os.path.isdir(os.path.join(root, "tokenizer_2")):
        from transformers import CLIPTokenizer
        tokenizer_2 = CLIPTokenizer.from_pretrained(root, subfolder="tokenizer_2")
    out = {"unet": {"unet_params": weights("unet", UNET_WEIGHTS), "config": unet_cfg},
           "vae": {"vae_params": weights("vae", UNET_WEIGHTS), "config": vae_cfg},
           "text_encoder": {"text_encoder_params": te_params, "config": clip_cfg},
           "tokenizer": tokenizer}
    if sdxl:
        out["tokenizer_2"] = tokenizer_2
    return out


# ----------------------------------------------------------------------------- optimizer / RNG state (not in the reference)
def _layout_digest(store):
    h = hashlib.sha256()
    for p in store.order:
        lf = store.leaves[p]
        h.update(f"{p}:{lf.shape}:{lf.offset}:{int(lf.quantised)}:{int(lf.decayed)};".encode())
    h.update(f"bs={store.block_size};total={store.total}".encode())
    named = store.opt.file_meta().get("optimizer")  # Lion names none: its digests (and files) stay what they were before there was a choice
    if named is not None:
        h.update(f";optimizer={named}".encode())
    return h.hexdigest()


def _state_buffers(store):
    """The store attributes a training-state file holds: master, EMA and the saved rows of the optimizer's state table (the optimizer's
    counter and running products are not among them: ParamStore.set_step rebuilds them from the count)."""
    return ("master", "ema") + optimizers.saved(store)


# -2: flat-buffer layout of round 2 (8-element leaf alignment, segment ends at multiples of 2048, time_emb_proj / cross-attention
# to_k / to_v grouped per width).  -1 files (round 1) hold the same tensors at other offsets and cannot be re-dealt.
STATE_FORMAT = "sdt-training-state-2"
_OLD_FORMATS = {"sdt-training-state-1": "the flat-buffer layout changed after that format (leaf alignment, grouped projection leaves); "
                                        "re-export the weights with save_model from the build that wrote the file and restart the optimizer state"}


def _prodigy_meta(store):
    """A Prodigy store's settings as the string its files carry (optimizers.Prodigy.file_meta)."""
    return store.opt.file_meta()["prodigy"]


def _stepping_store(st):
    """The store of a state (or a bare store) whose buffers a training-state file holds, and its LoRA adapter if that is what steps:
    TrainState.stepping_of.  The frozen base under an adapter, new tokens or a side network is not written: it is the checkpoint the
    run started from (a side network's layout digest tells its file from the UNet's)."""
    from .training_utils import TrainState
    return TrainState.stepping_of(st)


def _tokens_meta(st):
    """The new-token settings a training-state file carries for a state (None without tokens)."""
    tk = getattr(st, "tokens", None)
    if tk is None:
        return None
    c = tk.cfg
    return (f"num_tokens={c.num_tokens};geometry={','.join(f'{V}x{D}' for V, D in tk.geometry)};retract={int(c.retract)};"
            f"retract_power={float(c.retract_power)!r}")


def _lora_meta(ad):
    return f"rank={ad.cfg.rank};alpha={float(ad.cfg.alpha)!r};targets={','.join(ad.cfg.targets)}" + (";dora=1" if ad.cfg.dora else "") + (
        f";algo={ad.cfg.algo}" if ad.cfg.algo != "lora" else "")


def save_training_state(path, unet_state, text_encoder_state, train_rng=None, rng_states=None):
    """Everything train_step mutates, so that load_training_state + the same batches continue the run: fp32 masters, 8-bit
    Lion codes + per-block scales, fp32 momenta of the unquantised leaves, EMA, step counts, and the sampling generator(s).
    Data-parallel runs draw different noise / timesteps on every rank: pass rng_states = the list of ALL ranks' generator states
    (gather_rng_states) so that each rank resumes its own stream; train_rng alone stores this process's generator (world 1)."""
    from safetensors.torch import save_file
    tensors, meta = {}, {"format": STATE_FORMAT}
    for name, st in (("unet", unet_state), ("text_encoder", text_encoder_state)):
        store, ad = _stepping_store(st)
        if store is None:  # frozen, no adapter: nothing of it changes
            meta[f"{name}.frozen"] = "1"
            continue
        if ad is not None:  # LoRA: the adapter store's master, moments, EMA and count
            meta[f"{name}.lora"] = _lora_meta(ad)
        if _tokens_meta(st) is not None:  # new tokens: the token store's master, moments, EMA and count
            meta[f"{name}.tokens"] = _tokens_meta(st)
        store._gather()  # sharded optimizer: raises unless GradReducer.gather_state() (collective, all ranks) made the state whole
        for b in _state_buffers(store):
            t = getattr(store, b)
            if t is not None:
                tensors[f"{name}.{b}"] = t.detach().cpu().contiguous()
        meta.update({f"{name}.{k}": v for k, v in store.opt.file_meta().items()})  # nothing for Lion: its files are byte for byte what they were
        meta[f"{name}.count"] = str(int(store.count))
        meta[f"{name}.layout"] = _layout_digest(store)
    if rng_states is not None:
        meta["train_rng.world"] = str(len(rng_states))
        for r, stt in enumerate(rng_states):
            tensors[f"train_rng.state.{r}"] = stt.cpu()
    elif train_rng is not None:
        meta["train_rng.world"] = "1"
        tensors["train_rng.state.0"] = train_rng.get_state().cpu()
    tmp = path + ".tmp"
    save_file(tensors, tmp, metadata=meta)
    os.replace(tmp, path)


def gather_rng_states(train_rng):
    """All ranks' generator states, in rank order, on every rank (a collective when torch.distributed is initialised)."""
    import torch
    import torch.distributed as dist
    mine = train_rng.get_state().cpu()
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [mine]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, mine)
    return out


def load_training_state(path, unet_state, text_encoder_state, train_rng=None, rank=0, world=1):
    """Inverse of save_training_state, into states built for the same model / quantisation settings (checked by a digest of
    the buffer layout).  Rank `rank` of `world` restores ITS generator; a file written by a different world size is refused
    (the ranks' noise streams cannot be re-dealt).  Returns the generator (state restored in place when given).
    With the sharded optimizer every rank calls this with the same file (each loads the whole buffers; the store is whole afterwards);
    a pending all-gather of the weight mirrors is drained first (ParamStore.begin_external_write)."""
    from safetensors import safe_open
    with safe_open(path, framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        fmt = meta.get("format")
        if fmt in _OLD_FORMATS:
            raise ValueError(f"{path}: training-state format {fmt}, this build reads {STATE_FORMAT}: {_OLD_FORMATS[fmt]}")
        if fmt != STATE_FORMAT:
            raise ValueError(f"{path}: not a training-state file (format {fmt!r}, expected {STATE_FORMAT})")
        keys = set(f.keys())
        for name, st in (("unet", unet_state), ("text_encoder", text_encoder_state)):
            store, ad = _stepping_store(st)
            if (store is None) != (meta.get(f"{name}.frozen") == "1"):
                raise ValueError(f"{path}: {name} is frozen in only one of file / state")
            if store is None:
                continue
            if meta.get(f"{name}.lora") != (None if ad is None else _lora_meta(ad)):
                raise ValueError(f"{path}: {name} state was saved with LoRA settings {meta.get(f'{name}.lora')!r}, this state has "
                                 f"{None if ad is None else _lora_meta(ad)!r}")
            if meta.get(f"{name}.tokens") != _tokens_meta(st):
                raise ValueError(f"{path}: {name} state was saved with new-token settings {meta.get(f'{name}.tokens')!r}, this state has "
                                 f"{_tokens_meta(st)!r}")
            saved_opt, opt = meta.get(f"{name}.optimizer", optimizers.FILE_DEFAULT), store.optimizer
            if saved_opt != opt:
                raise ValueError(f"{path}: {name} state was saved by the {saved_opt} optimizer and this state is built for {opt}: their "
                                 "moments are different quantities; build the state with the optimizer that wrote the file")
            settings = store.opt.file_meta().get("prodigy")  # (the optimizers agree: both None unless they are Prodigy)
            if meta.get(f"{name}.prodigy") != settings:
                raise ValueError(f"{path}: {name} state was saved by a Prodigy store with the settings {meta.get(f'{name}.prodigy')!r} and "
                                 f"this store has {settings!r}: d, d_max and numer continue one recursion only; build the "
                                 "store with the settings that wrote the file (prodigy=dict(...))")
            if meta.get(f"{name}.layout") != _layout_digest(store):
                raise ValueError(f"{path}: {name} state was saved for a different parameter layout / quantisation setting "
                                 f"(layout version {STATE_FORMAT}; digest {meta.get(f'{name}.layout', '?')[:12]} != {_layout_digest(store)[:12]}: "
                                 "model config, quantisation / weight-decay exclusion lists and quant_block_size must match)")
            store.begin_external_write()  # sharded optimizer: a mirror all-gather of the last step may still be in flight
            for b in _state_buffers(store):
                dst = getattr(store, b)
                if (dst is not None) != (f"{name}.{b}" in keys):
                    raise ValueError(f"{path}: {name}.{b} present in only one of file / state")
                if dst is not None:
                    dst.copy_(f.get_tensor(f"{name}.{b}"))
            store.set_step(int(meta[f"{name}.count"]))  # with a schedule: the device step counter resumes too
            if store.device.type == "cuda":
                store.prepare(full=True)  # the masters changed under the bf16 compute copies
                if ad is not None:
                    ad.merge()            # ... and under the merged mirrors of the adapted leaves
            store.state_whole = True      # every rank loaded the whole buffers (sharded optimizer: nothing to gather before a save)
        if train_rng is not None:
            saved_world = int(meta.get("train_rng.world", "0"))
            if saved_world == 0 and "train_rng.state" in keys:  # files of the first format: one generator
                saved_world, key = 1, "train_rng.state"
            else:
                key = f"train_rng.state.{rank}"
            if saved_world == 0:
                raise ValueError(f"{path}: holds no sampling-generator state (saved without train_rng / rng_states): pass train_rng=None to "
                                 "load the optimizer state alone")
            if saved_world != world:
                raise ValueError(f"{path}: generator states of {saved_world} rank(s), this run has {world}: every rank draws its own "
                                 "noise / timestep stream and the streams cannot be re-dealt")
            if key not in keys:
                raise ValueError(f"{path}: no generator state saved for rank {rank}")
            train_rng.set_state(f.get_tensor(key))
    return train_rng
