"""New-token embeddings trained on a frozen text encoder: textual inversion, alone or beside a UNet LoRA (pivotal tuning) (DESIGN.md
"New tokens"; include/sdt.h "NEW TOKENS").

The frozen token table tok (V, D) of every tower of a text-encoder ParamStore is continued by n trained rows, one leaf per tower in a
ParamStore of the adapter's own: <prefix>text_model/embeddings/token_embedding/new_tokens (n, D).  Placeholder j is id V + j of its
tower.  The embedding forward reads both tables (sdt_embedding_ext_fwd: the base table is never copied or resized while training), its
backward writes the gradient of the n rows only (sdt_embedding_ext_bwd, into the adapter store's float32 gradient), and that store
takes the optimizer step like any other (Lion / AdamW / Prodigy, EMA, schedules, clipping, checkpoints, micro-batch accumulation).
"""
import json
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .params import ParamStore

MAX_TOKENS = 256
TOKEN_TABLE = "text_model/embeddings/token_embedding/embedding"
NEW_TOKENS = "text_model/embeddings/token_embedding/new_tokens"


@dataclass(frozen=True)
class TokenConfig:
    """num_tokens placeholder tokens (1..256).  init_ids: one id, or num_tokens ids, below the vocabulary size - row j starts as a copy
    of tok[init_ids[j]], bit for bit; None draws the rows on the host from `seed` as a normal scaled to the base table's standard
    deviation.  retract: after every optimizer step rescale the rows towards the base table's standard deviation (diffusers' advanced
    DreamBooth-LoRA script: factor = (target_std / std) ** retract_power)."""
    num_tokens: int
    init_ids: tuple = None
    seed: int = 0
    retract: bool = False
    retract_power: float = 0.1

    def __post_init__(self):
        n = self.num_tokens
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_TOKENS:
            raise ValueError(f"TokenConfig: num_tokens must be an integer in 1..{MAX_TOKENS}, not {n!r}")
        ids = self.init_ids
        if ids is not None:
            ids = (ids,) if isinstance(ids, int) and not isinstance(ids, bool) else ids
            try:
                ids = tuple(ids)
            except TypeError:
                raise ValueError(f"TokenConfig: init_ids must be an id or a sequence of ids, not {self.init_ids!r}") from None
            if not all(isinstance(i, int) and not isinstance(i, bool) and i >= 0 for i in ids):
                raise ValueError(f"TokenConfig: init_ids must be non-negative integers, not {self.init_ids!r}")
            if len(ids) == 1:
                ids = ids * n
            if len(ids) != n:
                raise ValueError(f"TokenConfig: init_ids holds {len(ids)} ids for num_tokens={n} (one id, or one per token)")
            object.__setattr__(self, "init_ids", ids)
        if isinstance(self.seed, bool) or not isinstance(self.seed, int):
            raise ValueError(f"TokenConfig: seed must be an integer, not {self.seed!r}")
        if not isinstance(self.retract, bool):
            raise ValueError(f"TokenConfig: retract must be a bool, not {self.retract!r}")
        p = self.retract_power
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p):
            raise ValueError(f"TokenConfig: retract_power must be a finite number, not {p!r}")


def table_std(table):
    """The unbiased standard deviation of a whole table in float64 (a host float): retract's target."""
    return float(table.detach().to("cpu", torch.float64).std(unbiased=True)) if table.numel() > 1 else 0.0


class TokenAdapter:
    """What attach() hangs on a frozen text-encoder store (store.tokens): the trained rows (self.store), one leaf per tower."""

    def __init__(self, base, cfg, store_kwargs):
        if base.trainable:
            raise ValueError("new tokens: the base store must be frozen (ParamStore(trainable=False)); training tokens beside a fully "
                             "fine-tuned text encoder is not supported")
        if getattr(base, "tokens", None) is not None:
            raise ValueError("new tokens: the store already carries new tokens")
        if getattr(base, "adapter", None) is not None:
            raise ValueError("new tokens: the store carries a LoRA adapter; a text-encoder LoRA together with new tokens is not supported")
        self.base, self.cfg, self.source = base, cfg, "master"
        self.tok_paths = [p for p in base.order if p.endswith(TOKEN_TABLE)]
        if not self.tok_paths:
            raise ValueError(f"new tokens: the store holds no token table (no leaf ends in {TOKEN_TABLE})")
        self.prefixes = [p[: -len(TOKEN_TABLE)] for p in self.tok_paths]
        self.new_paths = {p: pre + NEW_TOKENS for p, pre in zip(self.tok_paths, self.prefixes)}
        self.geometry = [tuple(base.leaves[p].shape) for p in self.tok_paths]  # (V_i, D_i) per tower
        n = cfg.num_tokens
        for (V, _), p in zip(self.geometry, self.tok_paths):
            if cfg.init_ids is not None and max(cfg.init_ids) >= V:
                raise ValueError(f"new tokens: init_ids {cfg.init_ids!r} must lie below the vocabulary size {V} of {p}")
            if V + n >= 1 << 31:
                raise ValueError(f"new tokens: {V} + {n} ids do not fit int32")
        kw = dict(store_kwargs)
        kw.setdefault("device", base.device)
        if kw.get("quant_mask") is not None:
            raise ValueError("new tokens: configure the token store with quant_excluded patterns, not with an explicit quant_mask tree "
                             "(it would override the exclusion of new_tokens from quantisation)")
        kw["quant_excluded"] = tuple(kw.get("quant_excluded", ())) + ("new_tokens",)
        self.store = ParamStore([(self.new_paths[p], (n, D)) for p, (_, D) in zip(self.tok_paths, self.geometry)], trainable=True, **kw)
        self.store.tokens_of = self
        if self.store.grad16 is not None or self.store.g32_base:
            raise ValueError("new tokens: the token store must keep its gradients in float32")
        self.target_std = [table_std(base.p(p)) for p in self.tok_paths]  # computed once; kept in the file's meta
        self.stats = torch.zeros(len(self.tok_paths), 3, dtype=torch.float64, device=base.device)  # retract: {mean, std, factor} per tower
        self.init_weights()
        base.tokens = self

    # ------------------------------------------------------------------ parameters
    @property
    def num_tokens(self):
        return self.cfg.num_tokens

    def init_weights(self):
        g = torch.Generator().manual_seed(int(self.cfg.seed))
        tree = {}
        for p, (V, D), std in zip(self.tok_paths, self.geometry, self.target_std):
            if self.cfg.init_ids is not None:
                rows = self.base.p(p)[torch.tensor(self.cfg.init_ids, device=self.base.device)].clone()
            else:
                rows = torch.randn(self.num_tokens, D, generator=g) * std
            tree[self.new_paths[p]] = rows
        self.store.load(tree)

    def placeholder_ids(self, tower=0):
        """The ids of the placeholders in tower `tower`: V_i + j."""
        V = self.geometry[tower][0]
        return [V + j for j in range(self.num_tokens)]

    def select(self, source):
        """Which copy of the trained rows the forward reads: "master" or "ema".  The choice sticks (as LoraAdapter.merge's does);
        train_step selects "master"."""
        if source not in ("master", "ema"):
            raise ValueError(f"select: source must be 'master' or 'ema', not {source!r}")
        if source == "ema" and self.store.ema is None:
            raise ValueError("select(source='ema'): the token store keeps no EMA")
        self.source = source

    def rows(self, tok_path, source=None):
        """The (n, D) float32 view of the trained rows that continue `tok_path`, from the master or the EMA buffer."""
        source = self.source if source is None else source
        buf = self.store.master if source == "master" else self.store.ema
        if buf is None:
            raise ValueError("rows(source='ema'): the token store keeps no EMA")
        lf = self.store.leaves[self.new_paths[tok_path]]
        return buf[lf.offset: lf.offset + lf.numel].view(lf.shape)

    def grad(self, tok_path):
        return self.store.g(self.new_paths[tok_path])

    def retract(self):
        """Rescale every tower's rows (the master) towards the base table's standard deviation: sdt_embedding_retract, one launch per
        tower; {mean, std, factor} of the last call stay in self.stats[tower].  The EMA is not touched."""
        p = float(self.cfg.retract_power)
        for i, (tp, (_, D)) in enumerate(zip(self.tok_paths, self.geometry)):
            _lib.call("sdt_embedding_retract", self.rows(tp, "master").data_ptr(), self.num_tokens, D, self.target_std[i], p,
                      self.stats[i].data_ptr(), torch.cuda.current_stream().cuda_stream)

    def resized_tree(self, source=None):
        """{path: float32 tensor} of the text encoder with (V + n, D) token tables - the base rows followed by the new ones - as
        transformers' resize_token_embeddings leaves it; every other leaf is the base's."""
        tree = self.base.export("master")
        for p in self.tok_paths:
            tree[p] = torch.cat([tree[p], self.rows(p, source).detach().to(tree[p].device)], dim=0)
        return tree

    # ------------------------------------------------------------------ token file
    def _meta(self):
        return dict(num_tokens=int(self.num_tokens), towers=[dict(prefix=pre, vocab_size=int(V), width=int(D))
                                                             for pre, (V, D) in zip(self.prefixes, self.geometry)],
                    target_std=[float(s) for s in self.target_std],
                    init_ids=None if self.cfg.init_ids is None else [int(i) for i in self.cfg.init_ids])

    def save(self, path, which="master"):
        """One .npz: the new_tokens leaves (fp32) and __meta__ (JSON: num_tokens, vocabulary size and width per tower, target_std,
        init_ids)."""
        tree = self.store.export_host(which)
        with open(path, "wb") as f:
            np.savez(f, __meta__=np.frombuffer(json.dumps(self._meta()).encode(), dtype=np.uint8), **{p: np.asarray(v) for p, v in tree.items()})

    def load(self, path):
        """Inverse of save().  ValueError naming the mismatch for a file with another token count or another base geometry.  The
        file's target_std replaces the one computed at attach."""
        with np.load(path) as z:
            if "__meta__" not in z.files:
                raise ValueError(f"{path}: not a token file (no __meta__)")
            meta = json.loads(bytes(z["__meta__"]).decode())
            mine = self._meta()
            if "num_tokens" not in meta or "towers" not in meta:
                raise ValueError(f"{path}: not a token file (its __meta__ holds {sorted(meta)})")
            if meta["num_tokens"] != mine["num_tokens"]:
                raise ValueError(f"{path}: {meta['num_tokens']} tokens in the file, {mine['num_tokens']} attached here")
            if meta["towers"] != mine["towers"]:
                raise ValueError(f"{path}: trained on another base geometry: towers {meta['towers']} in the file, {mine['towers']} here")
            tree = {p: torch.from_numpy(np.array(z[p])) for p in self.store.order}
        self.store.load(tree)
        self.target_std = [float(s) for s in meta["target_std"]]


def attach(text_store, cfg, **store_kwargs):
    """Hang new tokens on the frozen text-encoder store `text_store` (text_store.tokens).  store_kwargs configure the token store
    (quantise, quant_excluded, wd_excluded, block_size, with_ema, optimizer, adam_betas, prodigy).  ValueError: a trainable base, a
    second attach, a store that carries a LoRA adapter, init_ids outside the vocabulary."""
    if not isinstance(cfg, TokenConfig):
        raise ValueError(f"attach: cfg must be a TokenConfig, not {type(cfg).__name__}")
    return TokenAdapter(text_store, cfg, store_kwargs)
