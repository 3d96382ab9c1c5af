"""Latent cache: the frozen VAE's posterior moments of every loader batch, encoded once and kept on disk, so that training steps
skip the VAE (train_step with batch["latent_moments"]).

What is cached is the encoder's output - mean | log-variance, bf16 (B,h,w,2L), training_utils.encode_latent_moments - not a
sampled latent: the posterior draw and vae_scale stay in the step, so a step from the cache takes the same draws from its
generator as the pixel step and, from the same moments, computes the same bits.  "The same moments" has one condition: the
GEMM tile and split plans depend on the batch shape, so the encoder's bits are those of the batch composition it ran at.  build()
therefore encodes every batch as the loader delivers it - one record per batch, never re-batched by the Reader.

Layout of a cache directory (plain numpy, nothing compressed):
  index.json          {"format_version": 1, "latent_channels": L, "buckets": [[B, 3, H, W], ...] (training_utils.step_key of each
                      record, in order), "vae_digest": sha256 of the encoder weights the moments came from}
  record_000000.npz   moments uint16 (B,h,w,2L) (the bf16 bit patterns), input_ids, and time_ids / text_embeds where the batch has them;
                      for a batch with a loss_mask, loss_mask float32 (B,h,w): the mask pooled to the latent grid by
                      sdt_loss_mask_prepare, before the floor (the floor is applied in the step: one cache serves any floor); and
                      loss_weight float32 (B,) as the batch holds it.  A record of a batch without them is what it was before they existed.
                      For a batch with an inpaint_mask (an inpainting UNet's, include/sdt.h "INPAINTING"): masked_latent_moments uint16
                      (B,h,w,2L), the moments of the masked image out of the SAME stacked 2B encode the step runs
                      (training_utils.encode_inpaint_moments: `moments` is then that encode's first half), and inpaint_mask float32
                      (B,h,w), the nearest-neighbour 0/1 latent mask.  A record without the mask keeps its members and bytes.
                      For a ControlNet batch: conditioning_pixel_values float32 (B,C,H,W) as the batch holds them (the hint stays at
                      pixel size: the ControlNet's embedder, which is trained, reads it every step).
                      For an IP-Adapter batch: image_embeds (B,E) as the batch holds them.
A cached SD1.5 512x512 sample is 64 KiB; its fp32 pixels are 3 MiB (as is a ControlNet batch's conditioning image, which is kept).
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import _lib, ops
from .training_utils import encode_inpaint_moments, encode_latent_moments, step_key

FORMAT_VERSION = 1
# what a record keeps of a batch besides the moments (conditioning_pixel_values: a ControlNet batch's hint, float32 at pixel size;
# image_embeds: an IP-Adapter batch's image embedding (B, E), as the batch holds it)
EXTRA_KEYS = ("input_ids", "time_ids", "text_embeds", "conditioning_pixel_values", "image_embeds")
LOSS_WEIGHT_KEY, LOSS_MASK_KEY = "loss_weight", "loss_mask"  # kept too: the weight as it is, the mask pooled to the latent grid
INPAINT_MASK_KEY, MASKED_MOMENTS_KEY = "inpaint_mask", "masked_latent_moments"  # the latent 0/1 mask and the masked image's moments


def vae_digest(frozen_vae):
    """sha256 over the fp32 encoder weights of a frozen VAE (training_utils.FrozenModel: its store's flat master buffer)."""
    master = frozen_vae.params.master
    return hashlib.sha256(master.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _record_path(path, i):
    return os.path.join(path, f"record_{i:06d}.npz")


def _walk(batches):
    """A loader (grab_next_batch until "end_of_batch", None = nothing yet) or any iterable of batches ("end_of_batch" ends it too)."""
    if hasattr(batches, "grab_next_batch"):
        while True:
            b = batches.grab_next_batch()
            if isinstance(b, str) and b == "end_of_batch":
                return
            if b is not None:
                yield b
    else:
        for b in batches:
            if isinstance(b, str) and b == "end_of_batch":
                return
            if b is not None:
                yield b


class Writer:
    """Appends records to a cache directory; close() writes index.json (a directory without one is not a cache)."""

    def __init__(self, path, latent_channels, digest):
        os.makedirs(path, exist_ok=True)
        self.path, self.latent_channels, self.digest, self.buckets = path, int(latent_channels), str(digest), []

    def add(self, moments, batch, loss_mask=None, inpaint=None):
        """moments: bf16 (B,h,w,2L) tensor of `batch` (any device); batch: the loader's dict, of which EXTRA_KEYS and loss_weight are
        kept; loss_mask: the batch's mask at LATENT size, f32 (B,h,w) (pool_loss_mask), or None; inpaint: None, or (masked-image
        moments bf16 (B,h,w,2L), latent inpaint mask f32 (B,h,w)) as encode_inpaint_moments returns them."""
        if moments.dtype != torch.bfloat16 or moments.dim() != 4 or moments.shape[3] != 2 * self.latent_channels:
            raise ValueError(f"moments must be bfloat16 (B,h,w,{2 * self.latent_channels}), not {moments.dtype} {tuple(moments.shape)}")
        rec = {"moments": moments.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)}
        for k in EXTRA_KEYS:
            if k in batch:
                v = batch[k].detach().cpu()
                rec[k] = (v.view(torch.int16).numpy().view(np.uint16) if v.dtype == torch.bfloat16 else v.numpy())
        if loss_mask is not None:
            if loss_mask.dtype != torch.float32 or tuple(loss_mask.shape) != tuple(moments.shape[:3]):
                raise ValueError(f"loss_mask must be float32 {tuple(moments.shape[:3])} (latent size), not {loss_mask.dtype} "
                                 f"{tuple(loss_mask.shape)}")
            rec[LOSS_MASK_KEY] = loss_mask.detach().contiguous().cpu().numpy()
        if inpaint is not None:
            mm, lm = inpaint
            if mm.dtype != torch.bfloat16 or tuple(mm.shape) != tuple(moments.shape):
                raise ValueError(f"masked_latent_moments must be bfloat16 {tuple(moments.shape)}, not {mm.dtype} {tuple(mm.shape)}")
            if lm.dtype != torch.float32 or tuple(lm.shape) != tuple(moments.shape[:3]):
                raise ValueError(f"inpaint_mask must be float32 {tuple(moments.shape[:3])} (latent size), not {lm.dtype} {tuple(lm.shape)}")
            rec[MASKED_MOMENTS_KEY] = mm.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
            rec[INPAINT_MASK_KEY] = lm.detach().contiguous().cpu().numpy()
        if LOSS_WEIGHT_KEY in batch:
            rec[LOSS_WEIGHT_KEY] = batch[LOSS_WEIGHT_KEY].detach().to(torch.float32).contiguous().cpu().numpy()
        with open(_record_path(self.path, len(self.buckets)), "wb") as f:
            np.savez(f, **rec)
        self.buckets.append(list(step_key({"latent_moments": moments})))

    def close(self):
        with open(os.path.join(self.path, "index.json"), "w") as f:
            json.dump({"format_version": FORMAT_VERSION, "latent_channels": self.latent_channels, "buckets": self.buckets,
                       "vae_digest": self.digest}, f, indent=1)
        return self.path


def pool_loss_mask(mask, h, w):
    """A batch's loss_mask f32 (B,H,W) on the GPU -> the pooled mask f32 (B,h,w) of the latent grid, by the kernel the step itself
    uses (sdt_loss_mask_prepare with floor 0 writes the un-floored pooled mask beside the effective one)."""
    B, H, W = mask.shape
    f = H // h
    if f not in (1, 2, 4, 8, 16) or (H, W) != (h * f, w * f):
        raise ValueError(f"loss_mask {tuple(mask.shape)} against the latent grid ({h}, {w}): the scale must be the same power of two, "
                         "at most 16, on both axes")
    dev = mask.device
    pooled, eff = torch.empty(B, h, w, dtype=torch.float32, device=dev), torch.empty(B, h, w, dtype=torch.float32, device=dev)
    sums = torch.empty(B, dtype=torch.float32, device=dev)
    rws = ops.reduce_workspace(_lib.load().sdt_reduce_workspace_bytes(), dev)
    _lib.call("sdt_loss_mask_prepare", mask.data_ptr(), eff.data_ptr(), pooled.data_ptr(), sums.data_ptr(), B, h, w, f, 0.0,
              rws.data_ptr(), rws.numel(), torch.cuda.current_stream().cuda_stream)
    return pooled


@torch.no_grad()
def build(batches, frozen_vae, path):
    """Encode every batch of `batches` (a loader with grab_next_batch, or an iterable; "end_of_batch" ends it) with the frozen VAE,
    at the shape it arrives in, into the cache directory `path`.  A batch's loss_mask is stored pooled to the latent grid, its
    loss_weight as it is.  A batch with an inpaint_mask is encoded as the stack [image | masked image] of 2B the inpainting step
    encodes, and its record gains masked_latent_moments and the latent-size inpaint_mask.  Returns the number of records."""
    w = Writer(path, frozen_vae.call["latent_channels"], vae_digest(frozen_vae))
    dev = frozen_vae.params.device
    for batch in _walk(batches):
        px = batch["pixel_values"].to(dev, torch.float32).contiguous()
        inpaint = None
        if INPAINT_MASK_KEY in batch:
            moments, mm, lm = encode_inpaint_moments(frozen_vae, px, batch[INPAINT_MASK_KEY].to(dev, torch.float32).contiguous())
            inpaint = (mm, lm)
        else:
            moments = encode_latent_moments(frozen_vae, px)
        pooled = None
        if LOSS_MASK_KEY in batch:
            pooled = pool_loss_mask(batch[LOSS_MASK_KEY].to(dev, torch.float32).contiguous(), moments.shape[1], moments.shape[2])
        w.add(moments, batch, loss_mask=pooled, inpaint=inpaint)
    w.close()
    return len(w.buckets)


class Reader:
    """The batches of a cache directory, in the order they were written, behind the loader's grab_next_batch interface: dicts with
    latent_moments (bf16, on `device`) in place of pixel_values, then "end_of_batch"; rewind() starts over.
    ValueError for a format version this code does not know and, given the frozen VAE of the run, for moments that came from
    other encoder weights."""

    def __init__(self, path, device="cuda", vae=None):
        with open(os.path.join(path, "index.json")) as f:
            idx = json.load(f)
        if idx.get("format_version") != FORMAT_VERSION:
            raise ValueError(f"{path}: latent cache format version {idx.get('format_version')!r}, this reader knows {FORMAT_VERSION}")
        if vae is not None and vae_digest(vae) != idx["vae_digest"]:
            raise ValueError(f"{path}: the cache was encoded with other VAE weights (digest {idx['vae_digest'][:12]}..., this VAE "
                             f"{vae_digest(vae)[:12]}...): rebuild it")
        self.path, self.device = path, torch.device(device)
        self.latent_channels, self.buckets, self.digest = idx["latent_channels"], [tuple(b) for b in idx["buckets"]], idx["vae_digest"]
        self._cursor = 0

    def __len__(self):
        return len(self.buckets)

    def rewind(self):
        self._cursor = 0

    def grab_next_batch(self):
        if self._cursor >= len(self.buckets):
            return "end_of_batch"
        with np.load(_record_path(self.path, self._cursor)) as rec:
            arrays = {k: rec[k] for k in rec.files}
        self._cursor += 1
        batch = {"latent_moments": torch.from_numpy(arrays.pop("moments").view(np.int16)).view(torch.bfloat16)}
        for k, v in arrays.items():
            batch[k] = torch.from_numpy(v.view(np.int16)).view(torch.bfloat16) if v.dtype == np.uint16 else torch.from_numpy(v)
        return {k: v.to(self.device) for k, v in batch.items()}

    def __iter__(self):
        self.rewind()
        while True:
            b = self.grab_next_batch()
            if isinstance(b, str):
                return
            yield b
