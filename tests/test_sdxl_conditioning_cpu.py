"""SDXL conditioning, host side (no GPU): the SDXL-mode config and its parameter leaves, SDXL pipeline directories through
save_model / load_models, the two-tower loader, the step's refusal of an ambiguous pooled embedding, and argument checks of the
pooling exports (sdt_clip_pool_fwd / _bwd)."""
import json
import os

import numpy as np
import pytest
import torch

from stable_diffusion_training_amd import checkpoint as ck
from stable_diffusion_training_amd import nets, params
from stable_diffusion_training_amd import training_utils as tu
from stable_diffusion_training_amd.streamer import DataLoader

T1 = dict(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2,
          max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
T2 = dict(vocab_size=64, hidden_size=48, intermediate_size=96, num_hidden_layers=2, num_attention_heads=3,
          max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=40)


def test_default_dual_config_is_unchanged():
    cfg = nets.dual_clip_config()
    assert not nets.sdxl_conditioning(cfg) and "sdxl_conditioning" not in cfg
    assert all("hidden_layer" not in t and "with_projection" not in t for t in cfg["towers"])
    assert not any("text_projection" in p for p, _ in nets.clip_text_spec(cfg))
    assert nets.unused_text_leaves(cfg) == []


def test_sdxl_config_leaves():
    cfg = nets.dual_clip_config(sdxl_conditioning=True)
    t1, t2 = cfg["towers"]
    assert nets.sdxl_conditioning(cfg) and t1["hidden_layer"] == t2["hidden_layer"] == -2
    assert t2["projection_dim"] == 1280 and t2["eos_token_id"] == 2 and "projection_dim" not in t1
    spec = dict(nets.clip_text_spec(cfg))
    assert spec["text_encoder_2/text_projection/kernel"] == (1280, 1280)
    assert "text_encoder_2/text_projection/bias" not in spec
    base = dict(nets.clip_text_spec(nets.dual_clip_config()))
    assert set(spec) - set(base) == {"text_encoder_2/text_projection/kernel"}
    unused = nets.unused_text_leaves(cfg)
    assert all(p.startswith(("text_encoder/text_model/encoder/layers/11/", "text_encoder/text_model/final_layer_norm/")) for p in unused)
    assert len(unused) == 16 + 2  # the last CLIP-L layer (8 Dense kernels / biases, 2 norms) and its final LayerNorm


def test_unused_leaves_are_zero_ranges():
    cfg = nets.dual_clip_config(T1, T2, sdxl_conditioning=True)
    st = params.ParamStore(nets.clip_text_spec(cfg), device="cpu", quantise=False)
    st.fill_grad(5.0)
    unused = nets.unused_text_leaves(cfg)
    st.mark_unused(unused)
    g = st.export("grad")
    assert all(float(g[p].abs().max()) == 0.0 for p in unused)
    st._build_zero_ranges()
    # every unused element is inside a cleared range (fp32 gradient buffer: 4 elements per 16-byte unit)
    (buf, table, n), = [t for t in st._zero if t[0] is not None and t[0].dtype == torch.float32]
    cleared = torch.zeros(st.total, dtype=torch.bool)
    for u0, cnt in table.view(-1, 2).tolist():
        cleared[st.g32_base + 4 * u0: st.g32_base + 4 * (u0 + cnt)] = True
    for p in unused:
        lf = st.leaves[p]
        assert bool(cleared[lf.offset: lf.offset + lf.numel].all()), p
    used_kernel = st.leaves["text_encoder/text_model/encoder/layers/0/mlp/fc1/kernel"]
    assert not bool(cleared[used_kernel.offset: used_kernel.offset + used_kernel.numel].any())


def _models(te_cfg, seed=0):
    from oracle import nets as onets
    unet = nets.unet_config("tiny")
    vae = nets.vae_config("tiny")
    return {"unet": {"unet_params": onets.init_params(onets.unet_param_shapes(unet), seed), "config": unet},
            "vae": {"vae_params": onets.init_params(onets.vae_encoder_param_shapes(vae), seed + 1), "config": vae},
            "text_encoder": {"text_encoder_params": nets.init_params(nets.clip_text_spec(te_cfg), seed + 2), "config": te_cfg}}


def _save(models, out):
    m = models
    objs = {"unet": m["unet"]["config"], "vae": m["vae"]["config"], "text_encoder": m["text_encoder"]["config"]}
    ck.save_model(objs, None, m["unet"]["unet_params"], m["text_encoder"]["text_encoder_params"], m["vae"]["vae_params"], out)


def _tc(path):
    return type("TC", (), {"model_path": path})()


def test_sdxl_directory_round_trip(tmp_path):
    cfg = nets.dual_clip_config(T1, dict(T2, eos_token_id=63), sdxl_conditioning=True)
    models = _models(cfg)
    out = str(tmp_path / "xl")
    _save(models, out)
    for sub in ("unet", "vae", "text_encoder", "text_encoder_2", "scheduler"):
        assert os.path.isdir(os.path.join(out, sub)), sub
    index = json.load(open(os.path.join(out, "model_index.json")))
    assert index["_class_name"] == "FlaxStableDiffusionXLPipeline"
    assert index["text_encoder"] == ["transformers", "FlaxCLIPTextModel"]
    assert index["text_encoder_2"] == ["transformers", "FlaxCLIPTextModelWithProjection"]
    assert index["tokenizer_2"] == ["transformers", "CLIPTokenizer"]
    c2 = json.load(open(os.path.join(out, "text_encoder_2", "config.json")))
    assert c2["architectures"] == ["CLIPTextModelWithProjection"] and c2["projection_dim"] == 40 and c2["eos_token_id"] == 63
    assert "with_projection" not in c2 and "hidden_layer" not in c2
    tree2 = ck.flax_from_bytes(open(os.path.join(out, "text_encoder_2", ck.CLIP_WEIGHTS), "rb").read())
    assert set(tree2) == {"text_model", "text_projection"} and tree2["text_projection"]["kernel"].shape == (48, 40)
    tree1 = ck.flax_from_bytes(open(os.path.join(out, "text_encoder", ck.CLIP_WEIGHTS), "rb").read())
    assert set(tree1) == {"text_model"}

    back = ck.load_models(_tc(out))
    te = back["text_encoder"]
    assert nets.sdxl_conditioning(te["config"]) and back["tokenizer"] is None and back["tokenizer_2"] is None
    for got, want in zip(te["config"]["towers"], cfg["towers"]):
        got = {k: v for k, v in got.items() if k not in ("architectures", "model_type")}
        assert got == want
    assert te["config"]["prefixes"] == cfg["prefixes"]
    src = models["text_encoder"]["text_encoder_params"]
    assert set(te["text_encoder_params"]) == set(src)
    assert all(torch.equal(te["text_encoder_params"][k], src[k]) for k in src)
    for k, v in models["unet"]["unet_params"].items():
        assert torch.equal(back["unet"]["unet_params"][k], v)
    # the loaded config builds the same store layout, and the tree saves again byte for byte
    assert nets.clip_text_spec(te["config"]) == nets.clip_text_spec(cfg)
    out2 = str(tmp_path / "xl2")
    _save(dict(back, text_encoder=te), out2)
    for sub in ("text_encoder", "text_encoder_2"):
        for f in ("config.json", ck.CLIP_WEIGHTS):
            assert open(os.path.join(out, sub, f), "rb").read() == open(os.path.join(out2, sub, f), "rb").read(), (sub, f)


def test_xl_index_alone_marks_an_sdxl_directory(tmp_path):
    out = str(tmp_path / "xl")
    _save(_models(nets.dual_clip_config(T1, T2, sdxl_conditioning=True)), out)
    assert ck.is_sdxl_dir(out)
    os.makedirs(tmp_path / "plain")
    assert not ck.is_sdxl_dir(str(tmp_path / "plain"))


def test_sd15_directory_is_unchanged(tmp_path):
    """A single-tower store writes exactly the files it wrote before SDXL support: no text_encoder_2, the SD index, no run keys."""
    models = _models(nets.clip_config("tiny"))
    out = str(tmp_path / "sd")
    _save(models, out)
    assert sorted(os.listdir(out)) == ["model_index.json", "scheduler", "text_encoder", "unet", "vae"]
    index = json.load(open(os.path.join(out, "model_index.json")))
    assert index["_class_name"] == "FlaxStableDiffusionPipeline" and "text_encoder_2" not in index
    assert index["safety_checker"] == [None, None]
    back = ck.load_models(_tc(out))
    assert "towers" not in back["text_encoder"]["config"] and "tokenizer_2" not in back
    assert set(back["text_encoder"]["text_encoder_params"]) == set(models["text_encoder"]["text_encoder_params"])


def test_two_tower_loader_shapes_and_time_ids():
    dl = DataLoader(training_batch_size=4, repeat_batch=1, maximum_resolution_areas=(512 ** 2,), bucket_lower_bound_resolutions=(256,),
                    batches_per_chunk=3, vocab_size=64, context_concatenation_multiplier=2, text_towers=2)
    dl.create_training_dataframe()
    dl.dispatch_worker()
    dl._print_debug = False
    for _ in range(3):
        b = dl.grab_next_batch()
        B, _, H, W = b["pixel_values"].shape
        assert b["input_ids"].shape == (4, 2 * 2 * 77) and b["input_ids"].dtype == torch.int32
        ids = b["input_ids"].reshape(-1, 2, 77)
        assert ids.shape == (8, 2, 77)
        assert bool((ids[..., 0] == 62).all()) and bool((ids[..., -1] == 63).all())
        assert b["time_ids"].dtype == torch.int32 and b["time_ids"].tolist() == [[H, W, 0, 0, H, W]] * 4
    one = DataLoader(training_batch_size=2, repeat_batch=1, batches_per_chunk=1, vocab_size=64)
    one.create_training_dataframe()
    one._print_debug = False
    b1 = one.grab_next_batch()
    assert b1["input_ids"].shape == (2, 77) and "time_ids" not in b1
    with pytest.raises(ValueError):
        DataLoader(text_towers=3)


def test_text_embeds_with_sdxl_mode_is_refused():
    """The pooled embedding comes from the towers in SDXL mode: a batch that also carries one is ambiguous.  Refused before any
    device work (CPU stand-ins for the states)."""
    ns = type("NS", (), {})

    def state(cfg):
        s = ns()
        s.store, s.config = ns(), cfg
        s.store.device = torch.device("cpu")
        return s

    us = state(nets.unet_config("sdxl"))
    ts = state(nets.dual_clip_config(sdxl_conditioning=True))
    vae = tu.FrozenModel(call=nets.vae_config("tiny"), params=None)
    sch = tu.FrozenModel(call=None, params=None)
    batch = {"pixel_values": torch.zeros(2, 3, 64, 64), "input_ids": torch.zeros(2, 2, 77, dtype=torch.int32),
             "text_embeds": torch.zeros(2, 1280)}
    with pytest.raises(ValueError, match="text_embeds"):
        tu.train_step(us, ts, None, None, batch, None, vae, sch)


def test_clip_pool_argument_validation(lib):
    # every call below is refused by the argument checks, which run before any HIP call
    p = 4096  # an aligned address that is never dereferenced
    assert lib.sdt_clip_pool_fwd(None, p, p, p, p, p, p, 1, 1, 77, 48, -1, 1e-5, None) == -1
    assert b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_clip_pool_fwd(p, p, p, p, p, p, p, 1, 1, 77, 4096, -1, 1e-5, None) == -1
    assert b"D=4096" in lib.sdt_last_error()
    assert lib.sdt_clip_pool_fwd(p, p, p, p, p, p, p, 1, 1, 77, 44, -1, 1e-5, None) == -1  # not a multiple of 8
    assert lib.sdt_clip_pool_fwd(p, p, p, p, p, p, p, 0, 1, 77, 48, -1, 1e-5, None) == -1
    assert b"bad shape" in lib.sdt_last_error()
    assert lib.sdt_clip_pool_fwd(p, p + 2, p, p, p, p, p, 1, 1, 77, 48, -1, 1e-5, None) == -1
    assert b"misaligned" in lib.sdt_last_error()
    assert lib.sdt_clip_pool_bwd(p, p, p, p, p, p, p, None, 1, 1, 77, 48, None) == -1  # dgamma without dbeta
    assert b"null pointer" in lib.sdt_last_error()
    assert lib.sdt_clip_pool_bwd(p, p, p, p, p, p, None, None, 1, 0, 77, 48, None) == -1
    assert lib.sdt_clip_pool_bwd(p, p, p, p, p, p, None, None, 1, 1, 77, 2056, None) == -1
    assert lib.sdt_clip_pool_bwd(p, p, p, p, p, p + 8, None, None, 1, 1, 77, 48, None) == -1
    assert b"misaligned" in lib.sdt_last_error()
