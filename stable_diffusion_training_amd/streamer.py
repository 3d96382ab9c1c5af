"""Synthetic stand-in for the reference's `streamer.dataloader.DataLoader` (an un-vendored submodule: `streamer/` is empty
under /root/reference; its surface is what training.py:49-81, 122-139, 193-203 uses).  Same constructor arguments and the
same methods / attributes the loop touches, but the images and captions are seeded noise of the shapes the real loader
emits: aspect-ratio buckets from `calculate_resolution_array` (training_utils.py:134-174), `repeat_batch` consecutive
batches per bucket (so the step dispatcher does not bounce between shapes), k concatenated 77-token caption windows.

Data-parallel use: every rank builds the loader with the same seed and its (rank, world_size); all ranks walk the same
bucket sequence and each materialises its own shard of the GLOBAL batch (training_utils.py:805).  SURVEY.md §8(f)4.
"""
import numpy as np
import torch

from .training_utils import calculate_resolution_array


class DataLoader:
    def __init__(self, tokenizer_obj=None, config=None, ramdisk_path=None, training_batch_size=8, repeat_batch=10,
                 maximum_resolution_areas=(512 ** 2,), bucket_lower_bound_resolutions=(256,), numb_of_worker_thread=1,
                 queue_get_timeout=60, chunk_number=0, seed=0, context_concatenation_multiplier=1, *,
                 batches_per_chunk=100, vocab_size=49408, context_window=77, rank=0, world_size=1, device="cpu", text_towers=1,
                 loss_masks=False, prior_every=0, prior_loss_weight=1.0, inpaint_masks=False, placeholder_ids=None, conditioning_images=False,
                 image_embeds=0, image_embed_drop_rate=0.0, preference_pairs=False):
        if len(maximum_resolution_areas) != len(bucket_lower_bound_resolutions):
            raise ValueError("number of elements in maximum_resolution_areas and bucket_lower_bound_resolutions is not match!")
        if training_batch_size % world_size:
            raise ValueError(f"global batch {training_batch_size} is not divisible by {world_size} ranks")
        self.tokenizer_obj, self.config, self.ramdisk_path = tokenizer_obj, config, ramdisk_path
        self.training_batch_size, self.repeat_batch = training_batch_size, max(int(repeat_batch), 1)
        self.chunk_number, self.seed = chunk_number, seed
        self.k, self.vocab_size, self.context_window = context_concatenation_multiplier, vocab_size, context_window
        self.rank, self.world_size, self.device = rank, world_size, torch.device(device)
        if text_towers not in (1, 2):
            raise ValueError(f"text_towers={text_towers!r}: 1 (SD1.x / 2.x) or 2 (SDXL)")
        self.text_towers = text_towers
        if not isinstance(prior_every, int) or prior_every < 0:
            raise ValueError(f"prior_every={prior_every!r}: 0 (no class images) or n > 0 (every n-th sample is one)")
        self.loss_masks, self.prior_every, self.prior_loss_weight = bool(loss_masks), prior_every, float(prior_loss_weight)
        self.inpaint_masks = bool(inpaint_masks)
        if isinstance(conditioning_images, bool):
            conditioning_images = 3 if conditioning_images else 0
        if not isinstance(conditioning_images, int) or conditioning_images < 0:
            raise ValueError(f"conditioning_images={conditioning_images!r}: False, True (3 channels) or the ControlNet's conditioning_channels")
        self.conditioning_images = conditioning_images  # channels of the conditioning image, 0: none
        if not isinstance(image_embeds, int) or isinstance(image_embeds, bool) or image_embeds < 0:
            raise ValueError(f"image_embeds={image_embeds!r}: 0 (none) or the IP-Adapter's image_embed_dim")
        if not 0.0 <= float(image_embed_drop_rate) <= 1.0:
            raise ValueError(f"image_embed_drop_rate={image_embed_drop_rate!r} must lie in [0, 1]")
        self.image_embeds, self.image_embed_drop_rate = image_embeds, float(image_embed_drop_rate)  # width of the embedding, 0: none
        self.preference_pairs = bool(preference_pairs)
        if self.preference_pairs and (training_batch_size // world_size) % 2:
            raise ValueError(f"preference_pairs: every rank's batch ({training_batch_size // world_size}) holds interleaved (preferred, "
                             "rejected) pairs and must be even")
        self.placeholder_ids = self._check_placeholders(placeholder_ids, text_towers, context_window)
        self.buckets = [tuple(int(v) for v in b) for area, lo in zip(maximum_resolution_areas, bucket_lower_bound_resolutions)
                        for b in calculate_resolution_array(area, lo, 64)]
        self._batches_per_chunk = batches_per_chunk
        self._bulk_batch_count, self._first_batch_count = 0, 0
        self._print_debug = True
        self._plan, self._cursor = [], 0

    @staticmethod
    def _check_placeholders(ids, towers, window):
        """None, or one list of placeholder ids per tower (a flat list serves every tower): the ids a tokenizer would emit for the
        trained new tokens (tokens.TokenAdapter.placeholder_ids)."""
        if ids is None:
            return None
        ids = list(ids)
        if ids and not isinstance(ids[0], (list, tuple)):
            ids = [ids] * towers
        ids = [[int(i) for i in t] for t in ids]
        if len(ids) != towers or not ids[0] or any(len(t) != len(ids[0]) for t in ids):
            raise ValueError(f"placeholder_ids: a non-empty list of ids, or one such list of the same length per tower ({towers}), not {ids!r}")
        if len(ids[0]) > window - 2:
            raise ValueError(f"placeholder_ids: {len(ids[0])} ids do not fit a caption window of {window} between BOS and EOS")
        return ids

    # ---- chunk bookkeeping the loop calls (no files behind it here)
    def delete_prev_chunks(self, prev_chunk):
        return None

    def grab_and_prefetch_chunk(self, numb_of_prefetched_batch=1):
        return None

    def prepare_training_dataframe(self):
        return None

    def create_training_dataframe(self):
        """Lay out this chunk's batches: runs of `repeat_batch` batches per bucket, bucket order shuffled by (seed, chunk)."""
        rng = np.random.default_rng([int(self.seed), int(self.chunk_number)])
        plan = []
        while len(plan) < self._batches_per_chunk:
            plan.extend([self.buckets[int(rng.integers(len(self.buckets)))]] * self.repeat_batch)
        self._plan = plan[: self._batches_per_chunk]
        self._first_batch_count, self._bulk_batch_count = min(self.repeat_batch, len(self._plan)), max(len(self._plan) - self.repeat_batch, 0)

    def dispatch_worker(self):
        self._cursor = 0

    # ---- batches
    def grab_next_batch(self):
        """dict(pixel_values f32 (B,3,bucket[0],bucket[1]) in [-1,1], input_ids / attention_mask int32 (B, k*77)) for this
        rank's shard, or "end_of_batch" when the chunk is exhausted (training.py:195-199).  text_towers=2 (SDXL): input_ids /
        attention_mask (B, k*2*77), which reshape to (B*k, 2, 77) - one row per tower - and time_ids int32 (B, 6) = (bucket height,
        width, 0, 0, height, width): the uncropped size micro-conditioning.
        loss_masks=True adds loss_mask f32 (B, bucket[0], bucket[1]): one seeded rectangle of ones per image (the "subject"), zero
        outside, drawn from a generator of its own - the other entries are what they are without it.  prior_every=n > 0 marks every n-th
        sample of the global batch (global index % n == n - 1) as a class image and adds loss_weight f32 (B,): 1.0 for instance images,
        prior_loss_weight for class images (DreamBooth prior preservation).  inpaint_masks=True adds inpaint_mask f32 (B, bucket[0],
        bucket[1]) for an inpainting UNet: one seeded rectangle of ones (the region to repaint) per image, from a third generator of its
        own.  conditioning_images=True (3 channels) or n adds conditioning_pixel_values f32 (B, n, bucket[0], bucket[1]) in [0, 1] for a ControlNet: a
        seeded coarse 8 x 8 pattern per image, nearest-neighbour enlarged to the pixel size, from a fourth generator.  image_embeds=E adds
        image_embeds f32 (B, E) for an IP-Adapter - a seeded normal vector per image, the stand-in for an image encoder's pooled embedding,
        from a fifth generator; image_embed_drop_rate=p zeroes a sample's embedding with probability p (the published training script's
        image-prompt dropout, which lets classifier-free guidance drop the image prompt).  The defaults add none of them.
        placeholder_ids (a list of ids, or one list per tower for text_towers=2) overwrites the positions after BOS of every caption
        window with those ids - the caption "<sks> ..." of a textual-inversion run; the other entries keep their values.
        preference_pairs=True (Diffusion-DPO, train_step dpo_beta=): the batch holds interleaved (preferred, rejected) pairs - samples 2i
        and 2i+1 are two different images under ONE caption: sample 2i+1's input_ids are sample 2i's; every other entry keeps its
        value."""
        if self._cursor >= len(self._plan):
            return "end_of_batch"
        b0, b1 = self._plan[self._cursor]
        index = self._cursor
        self._cursor += 1
        per_rank = self.training_batch_size // self.world_size
        g = torch.Generator().manual_seed((int(self.seed) * 1_000_003 + int(self.chunk_number)) * 1_000_003 + index * 64 + self.rank)
        px = torch.rand(per_rank, 3, b0, b1, generator=g) * 2 - 1
        shape = (per_rank, self.k, self.context_window) if self.text_towers == 1 else (per_rank, self.k, 2, self.context_window)
        ids = torch.randint(0, self.vocab_size - 2, shape, generator=g, dtype=torch.int32)
        ids[..., 0] = self.vocab_size - 2   # <|startoftext|>
        ids[..., -1] = self.vocab_size - 1  # <|endoftext|>
        if self.placeholder_ids is not None:
            for t, pl in enumerate(self.placeholder_ids):
                row = torch.tensor(pl, dtype=torch.int32)
                if self.text_towers == 1:
                    ids[..., 1: 1 + len(pl)] = row
                else:
                    ids[:, :, t, 1: 1 + len(pl)] = row
        if self.preference_pairs:
            ids[1::2] = ids[0::2]  # a pair shares its caption; its two images stay different
        ids = ids.reshape(per_rank, -1)
        batch = {"pixel_values": px, "input_ids": ids, "attention_mask": torch.ones_like(ids)}
        if self.text_towers == 2:
            batch["time_ids"] = torch.tensor([[b0, b1, 0, 0, b0, b1]] * per_rank, dtype=torch.int32)
        if self.loss_masks:
            gm = torch.Generator().manual_seed(((int(self.seed) * 1_000_003 + int(self.chunk_number)) * 1_000_003 + index * 64 + self.rank) ^ 0x5DEECE66D)
            mask = torch.zeros(per_rank, b0, b1)
            for i in range(per_rank):  # a rectangle covering between a quarter and the whole of each axis
                hh, ww = (int(torch.randint(n // 4, n + 1, (1,), generator=gm)) for n in (b0, b1))
                y0, x0 = int(torch.randint(0, b0 - hh + 1, (1,), generator=gm)), int(torch.randint(0, b1 - ww + 1, (1,), generator=gm))
                mask[i, y0: y0 + hh, x0: x0 + ww] = 1.0
            batch["loss_mask"] = mask
        if self.inpaint_masks:
            gi = torch.Generator().manual_seed(((int(self.seed) * 1_000_003 + int(self.chunk_number)) * 1_000_003 + index * 64 + self.rank) ^ 0x2545F4914F6CDD1D)
            mask = torch.zeros(per_rank, b0, b1)
            for i in range(per_rank):  # a rectangle covering between a quarter and three quarters of each axis
                hh, ww = (int(torch.randint(n // 4, 3 * n // 4 + 1, (1,), generator=gi)) for n in (b0, b1))
                y0, x0 = int(torch.randint(0, b0 - hh + 1, (1,), generator=gi)), int(torch.randint(0, b1 - ww + 1, (1,), generator=gi))
                mask[i, y0: y0 + hh, x0: x0 + ww] = 1.0
            batch["inpaint_mask"] = mask
        if self.conditioning_images:
            gc = torch.Generator().manual_seed(((int(self.seed) * 1_000_003 + int(self.chunk_number)) * 1_000_003 + index * 64 + self.rank) ^ 0x1E3779B97F4A7C15)
            coarse = torch.rand(per_rank, self.conditioning_images, 8, 8, generator=gc)
            ys, xs = torch.arange(b0) * 8 // b0, torch.arange(b1) * 8 // b1
            batch["conditioning_pixel_values"] = coarse[:, :, ys][:, :, :, xs].contiguous()
        if self.image_embeds:
            ge = torch.Generator().manual_seed(((int(self.seed) * 1_000_003 + int(self.chunk_number)) * 1_000_003 + index * 64 + self.rank) ^ 0x3C6EF372FE94F82B)
            emb = torch.randn(per_rank, self.image_embeds, generator=ge)
            if self.image_embed_drop_rate:
                emb[torch.rand(per_rank, generator=ge) < self.image_embed_drop_rate] = 0.0
            batch["image_embeds"] = emb
        if self.prior_every:
            first = self.rank * per_rank  # this shard's first sample in the global batch
            batch["loss_weight"] = torch.tensor([self.prior_loss_weight if (first + i) % self.prior_every == self.prior_every - 1 else 1.0
                                                 for i in range(per_rank)], dtype=torch.float32)
        if self.device.type != "cpu":
            batch = {k: v.to(self.device, non_blocking=True) for k, v in batch.items()}
        if self._print_debug:
            print(f"[streamer] chunk {self.chunk_number} batch {index}: {tuple(px.shape)}")
        return batch
