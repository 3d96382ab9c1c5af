"""Generates tests/golden/sdxl_text_pin_*.npz: SDXL's text conditioning computed by the `transformers` PyTorch classes, a THIRD-PARTY
implementation of the two towers SDXL pipelines run (CLIPTextModel and CLIPTextModelWithProjection with output_hidden_states, as
diffusers' StableDiffusionXLPipeline.encode_prompt uses them).  The vectors pin nets.sdxl_text_forward (context = both towers'
hidden_states[-2], pooled = text_embeds) to something this project did not write (tests/test_gpu_sdxl_conditioning.py).  Runs in the
BUILD container only (transformers 5.15.0 is installed there); nothing of `transformers` is imported by tests, by the package or on
the GPU box - only the .npz files travel.

Two small towers: CLIP-L-like (3 layers, 32 wide, quick_gelu) and bigG-like (2 layers, 48 wide, erf-GELU, projection to 40).  Every
weight comes from transformers' own initialiser (perturbed so that biases / norms matter) and is stored under the Flax names of the
two-tower store (text_encoder/..., text_encoder_2/...; Dense kernel [in,out] = weight.T), with the ids, the context, text_embeds and
the gradient of EVERY leaf under fixed cotangents on (context, text_embeds).  Weights and cotangents are fp16-representable and
stored as fp16 (exact), gradients as fp16, context / text_embeds as fp32: a few hundred KB per case.

Cases (the pooling rule of CLIPTextTransformer.forward):
  argmax      eos_token_id = 2: pooled at the first largest id (SDXL's released configs)
  eos         eos_token_id = vocab - 1, pad = eos: the FIRST eos of a padded caption
  pad_ne_eos  eos_token_id = vocab - 1, second tower padded with id 0 after the eos (tokenizer_2's "!" padding)
Run:  python tests/golden/make_sdxl_text_pin.py
"""
import json
import os

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
VOCAB = 64
TOWER1 = dict(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
TOWER2 = dict(vocab_size=VOCAB, hidden_size=48, intermediate_size=96, num_hidden_layers=2, num_attention_heads=3,
              max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=40)
CASES = {"argmax": 2, "eos": VOCAB - 1, "pad_ne_eos": VOCAB - 1}


def hf_tower(cfg, eos, with_projection):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    c = CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                       num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                       max_position_embeddings=cfg["max_position_embeddings"], hidden_act=cfg["hidden_act"],
                       layer_norm_eps=cfg["layer_norm_eps"], bos_token_id=cfg["vocab_size"] - 2, eos_token_id=eos,
                       pad_token_id=cfg["vocab_size"] - 1, projection_dim=cfg.get("projection_dim", cfg["hidden_size"]),
                       attn_implementation="eager")
    m = (CLIPTextModelWithProjection if with_projection else CLIPTextModel)(c).float().eval()
    with torch.no_grad():  # transformers initialises biases to zero and norm scales to one: perturb so that they are pinned too
        g = torch.Generator().manual_seed(11 + int(with_projection))
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.add_(0.05 * torch.randn(p.shape, generator=g))
            elif "layer_norm" in n and n.endswith("weight"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("weight") and p.dim() == 2 and "embedding" not in n:
                p.mul_(3.0)  # default std 0.02-ish leaves the attention logits ~0: make the softmax matter
        for p in m.parameters():
            p.copy_(p.half().float())  # fp16-representable: the fixture stores the weights in fp16, exactly
    return m


def flax_name(torch_name):
    """state-dict key of the PyTorch model -> (Flax leaf path under text_model/ or text_projection/, transpose?)."""
    n = torch_name if torch_name.startswith(("text_model.", "text_projection.")) else "text_model." + torch_name
    if n.endswith(".weight"):
        base = n[: -len(".weight")]
        if "embedding" in base:
            return base.replace(".", "/") + "/embedding", False
        if "layer_norm" in base:
            return base.replace(".", "/") + "/scale", False
        return base.replace(".", "/") + "/kernel", True
    return n.replace(".", "/"), False


def ids_for(case, g, rows=3):
    ids = torch.randint(0, VOCAB - 2, (rows, 2, 77), generator=g)
    ids[:, :, 0] = VOCAB - 2
    ends = (9, 30, 76)
    for r in range(rows):
        e = ends[r % len(ends)]
        ids[r, :, e] = VOCAB - 1
        ids[r, 0, e + 1:] = VOCAB - 1                         # first tower: padded with eos
        ids[r, 1, e + 1:] = 0 if case == "pad_ne_eos" else VOCAB - 1
    return ids


def main():
    torch.manual_seed(20261016)
    for ci, (case, eos) in enumerate(CASES.items()):
        m1, m2 = hf_tower(TOWER1, eos, False), hf_tower(TOWER2, eos, True)
        g = torch.Generator().manual_seed(100 + ci)
        ids = ids_for(case, g)
        o1 = m1(input_ids=ids[:, 0], output_hidden_states=True)
        o2 = m2(input_ids=ids[:, 1], output_hidden_states=True)
        ctx = torch.cat([o1.hidden_states[-2], o2.hidden_states[-2]], -1)
        pooled = o2.text_embeds
        cot_ctx = torch.randn(ctx.shape, generator=g).half().float()
        cot_pooled = torch.randn(pooled.shape, generator=g).half().float()
        ((ctx * cot_ctx).sum() + (pooled * cot_pooled).sum()).backward()
        out = {"ids": ids.numpy().astype(np.int32), "context": ctx.detach().numpy(), "pooled": pooled.detach().numpy(),
               "cot_context": cot_ctx.numpy().astype(np.float16), "cot_pooled": cot_pooled.numpy().astype(np.float16),
               "towers": np.array(json.dumps([TOWER1, dict(TOWER2, eos_token_id=eos)]))}
        for prefix, m in (("text_encoder/", m1), ("text_encoder_2/", m2)):
            for n, p in m.named_parameters():
                path, tr = flax_name(n)
                w = p.detach().t() if tr else p.detach()
                gr = torch.zeros_like(p) if p.grad is None else p.grad
                out["w:" + prefix + path] = w.contiguous().numpy().astype(np.float16)  # exact (hf_tower)
                out["g:" + prefix + path] = (gr.t() if tr else gr).contiguous().numpy().astype(np.float16)  # 1e-3 relative: far inside the bf16 gates
        np.savez_compressed(os.path.join(OUT, f"sdxl_text_pin_{case}.npz"), **out)
        print(f"{case}: |ctx| {ctx.norm():.4f} |pooled| {pooled.norm():.4f}, {sum(k.startswith('w:') for k in out)} leaves")


if __name__ == "__main__":
    main()
