"""Low-rank adapters (LoRA) trained in weight space on a frozen base (DESIGN.md "LoRA"; include/sdt.h "LoRA").

An adapted Dense kernel W0 [K, N] of a frozen ParamStore carries two trained leaves A [K, r] and B [r, N] in a ParamStore of the
adapter's own.  Every GEMM of the model reads one bf16 mirror (ParamStore.w), so the adapter never enters the forward / input-gradient
chain: before a step ONE launch writes w[leaf] = bf16(W0 + s * A @ B) for every adapted leaf (s = alpha / rank, the sum rounded once from
fp32), the step runs as it stands - merged GEMMs, packed attention, HIP graphs - the ordinary weight-gradient kernels leave dW (bf16)
of the adapted leaves in the adapter's scratch, and ONE launch projects dA = s * dW @ B^T, dB = s * A^T @ dW into the gradient buffer
of the adapter's store, which then takes the optimizer step like any other store (Lion / AdamW, 8-bit or fp32 moments, EMA, schedules,
clipping, checkpoints, micro-batch accumulation).

LoCon (LoraConfig(conv_rank=R); include/sdt.h "LoCon"; DESIGN.md "LoCon"): a convolution kernel [kh, kw, Cin, Cout] whose channel counts are
multiples of 8 is one contiguous [K = kh*kw*Cin, N = Cout] matrix in the master and in the mirror, and LoCon's k x k down-convolution to R
channels followed by a 1x1 up-convolution is A [K, R] @ B [R, N] in that layout: the same merge, the same scratch, and a projection
whose dB stripes are split along the tall K (sdt_lora_project_split).

DoRA (LoraConfig(dora=True); include/sdt.h "DoRA"): a third trained leaf m [N] per adapted kernel, W' = v * (m / ||v||_column) with
v = W0 + s * A @ B.  The column norm is one more reduction inside the merge launch and the magnitude gradient one more inside the
projection launch, so the step between them is the LoRA step, launch for launch.

LoHa (LoraConfig(algo="loha"); include/sdt.h "LoHa"; DESIGN.md "LoHa"): four trained leaves A1, B1, A2, B2 per adapted kernel and the delta
s * (A1 @ B1) * (A2 @ B2), element-wise - rank r^2 at the parameters of a rank-2r LoRA.  The same interface: one fused merge launch and one
fused projection launch per job table (sdt_loha_merge / sdt_loha_project; the projection's dB stripes always take LoCon's split), the
same restore, scratch and step.  With conv_rank > 0 the convolutions carry LoHa adapters too.
"""
import bisect
import json
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .params import ParamStore

RANKS = (4, 8, 16, 32, 64, 128)
ALGOS = ("lora", "loha")
LOHA_MAX_RANK = 32  # one MFMA K-step forms a block of A_i @ B_i; the effective rank is r^2
UNET_TARGETS = ("to_q", "to_k", "to_v", "to_out_0")
CLIP_TARGETS = ("q_proj", "k_proj", "v_proj", "out_proj")
UNET_CONV_TARGETS = ("conv1", "conv2", "conv_shortcut", "proj_in", "proj_out", "conv")  # "conv": downsamplers_0/conv, upsamplers_0/conv


@dataclass(frozen=True)
class LoraConfig:
    """rank in RANKS; the delta is (alpha / rank) * A @ B; targets are matched against path components (as params.create_mask does);
    seed draws A (B starts at zero); dora adds the trained magnitude leaf <dense>/lora_m (it starts at the column norms of W0).
    conv_rank > 0 (LoCon) also adapts the 4-D kernels whose path has a component in conv_targets, at rank conv_rank and scale
    conv_alpha / conv_rank (conv_alpha None: conv_rank); a conv target that meets a 2-D kernel leaves it to `targets`.
    algo "loha": every adapted kernel carries loha_a1, loha_b1, loha_a2, loha_b2 and the delta (alpha / rank) * (A1 @ B1) * (A2 @ B2),
    element-wise, at ranks up to 32 (seed draws A1, B1 and A2; B2 starts at zero); not with dora."""
    rank: int
    alpha: float
    targets: tuple = UNET_TARGETS
    seed: int = 0
    dora: bool = False
    conv_rank: int = 0
    conv_alpha: float = None
    conv_targets: tuple = UNET_CONV_TARGETS
    algo: str = "lora"

    def __post_init__(self):
        object.__setattr__(self, "targets", tuple(self.targets))
        if isinstance(self.rank, bool) or self.rank not in RANKS:
            raise ValueError(f"LoraConfig: rank must be one of {RANKS}, not {self.rank!r}")
        if not self.targets or not all(isinstance(t, str) and t for t in self.targets):
            raise ValueError(f"LoraConfig: targets must be a non-empty tuple of path components, not {self.targets!r}")
        if not math.isfinite(float(self.alpha)):
            raise ValueError(f"LoraConfig: alpha must be finite, not {self.alpha!r}")
        if not isinstance(self.dora, bool):
            raise ValueError(f"LoraConfig: dora must be a bool, not {self.dora!r}")
        object.__setattr__(self, "conv_targets", tuple(self.conv_targets))
        if isinstance(self.conv_rank, bool) or (self.conv_rank != 0 and self.conv_rank not in RANKS):
            raise ValueError(f"LoraConfig: conv_rank must be 0 or one of {RANKS}, not {self.conv_rank!r}")
        if self.conv_alpha is not None and not math.isfinite(float(self.conv_alpha)):
            raise ValueError(f"LoraConfig: conv_alpha must be finite or None, not {self.conv_alpha!r}")
        if not self.conv_targets or not all(isinstance(t, str) and t for t in self.conv_targets):
            raise ValueError(f"LoraConfig: conv_targets must be a non-empty tuple of path components, not {self.conv_targets!r}")
        if self.conv_rank and self.dora:
            raise ValueError("LoraConfig: DoRA on convolutions is not supported (dora=True with conv_rank > 0): the DoRA merge walks K "
                             "twice per column stripe and has no split for a convolution's tall K")
        if self.algo not in ALGOS:
            raise ValueError(f"LoraConfig: algo must be one of {ALGOS}, not {self.algo!r}")
        if self.algo == "loha":
            if self.dora:
                raise ValueError("LoraConfig: DoRA combined with LoHa is not supported (algo='loha' with dora=True): the DoRA merge and "
                                 "projection are built on the low-rank product")
            if self.rank > LOHA_MAX_RANK or self.conv_rank > LOHA_MAX_RANK:
                raise ValueError(f"LoraConfig: algo='loha' takes rank and conv_rank up to {LOHA_MAX_RANK} (the effective rank is the square), "
                                 f"not rank={self.rank!r}, conv_rank={self.conv_rank!r}")

    def __repr__(self):  # (without LoCon / LoHa the text is what it was: refusal messages quote it)
        conv = f", conv_rank={self.conv_rank!r}, conv_alpha={self.conv_alpha!r}, conv_targets={self.conv_targets!r}" if self.conv_rank else ""
        algo = f", algo={self.algo!r}" if self.algo != "lora" else ""
        return (f"LoraConfig(rank={self.rank!r}, alpha={self.alpha!r}, targets={self.targets!r}, seed={self.seed!r}, dora={self.dora!r}"
                f"{conv}{algo})")

    @property
    def scale(self):
        return float(self.alpha) / self.rank

    @property
    def conv_scale(self):
        return float(self.conv_rank if self.conv_alpha is None else self.conv_alpha) / self.conv_rank if self.conv_rank else 0.0


def select_leaves(spec, cfg):
    """The kernel paths of `spec` ([(path, shape)], forward order) that `cfg` adapts: '/kernel' leaves with a path component equal to a
    target, and with cfg.conv_rank > 0 also the 4-D '/kernel' leaves with a component equal to a conv target.  ValueError for a
    convolution (4-D) kernel that `targets` matches, for a kernel whose dims are not multiples of 8 (its bf16 mirror is a zero-padded
    copy), when no Dense kernel matches `targets` and, with cfg.conv_rank > 0, when no 4-D kernel matches `conv_targets`."""
    out, convs = [], 0
    for path, shape in spec:
        if not path.endswith("/kernel"):
            continue
        parts, shape = path.split("/")[:-1], tuple(shape)
        if any(t in parts for t in cfg.targets):
            if len(shape) != 2:
                raise ValueError(f"LoRA: target matches {path} {shape}, which is not a Dense kernel (convolutions are not adapted"
                                 + (" by `targets`: name them in conv_targets)" if cfg.conv_rank else ")"))
            if shape[0] % 8 or shape[1] % 8:
                raise ValueError(f"LoRA: {path} {shape} is a padded leaf (dims not multiples of 8) and cannot carry an adapter")
            out.append(path)
        elif cfg.conv_rank and len(shape) == 4 and any(t in parts for t in cfg.conv_targets):
            if shape[2] % 8 or shape[3] % 8:
                raise ValueError(f"LoRA: {path} {shape} is a padded leaf (channel counts not multiples of 8) and cannot carry an adapter")
            out.append(path)
            convs += 1
    if len(out) == convs:
        raise ValueError(f"LoRA: no Dense kernel matches the targets {cfg.targets!r}")
    if cfg.conv_rank and not convs:
        raise ValueError(f"LoRA: no convolution kernel matches the conv targets {cfg.conv_targets!r}")
    return out


def leaf_factors(shape, cfg):
    """(K, N, rank, scale) of the adapter of a selected kernel: Dense [K, N] at cfg.rank; HWIO [kh, kw, Cin, Cout] as the matrix
    [kh*kw*Cin, Cout] at cfg.conv_rank."""
    if len(shape) == 2:
        return shape[0], shape[1], cfg.rank, cfg.scale
    return shape[0] * shape[1] * shape[2], shape[3], cfg.conv_rank, cfg.conv_scale


LOHA_LEAVES = ("loha_a1", "loha_b1", "loha_a2", "loha_b2")


def leaf_names(cfg):
    """The trained leaves of one adapted kernel, in store order."""
    if cfg.algo == "loha":
        return LOHA_LEAVES
    return ("lora_a", "lora_b", "lora_m") if cfg.dora else ("lora_a", "lora_b")


def adapter_spec(spec, cfg):
    """[(<layer path>/lora_a, (K, r)), (<layer path>/lora_b, (r, N))] for the adapted kernels of `spec`, in its order (Dense and
    convolution adapters interleaved as the base runs them); with cfg.dora each pair is followed by (<dense path>/lora_m, (N,)).
    algo "loha": loha_a1 (K, r), loha_b1 (r, N), loha_a2 (K, r), loha_b2 (r, N) per kernel."""
    shapes = dict((p, tuple(s)) for p, s in spec)
    out = []
    for path in select_leaves(spec, cfg):
        K, N, r, _ = leaf_factors(shapes[path], cfg)
        dense = path[: -len("/kernel")]
        if cfg.algo == "loha":
            out += [(f"{dense}/{n}", (K, r) if "_a" in n else (r, N)) for n in LOHA_LEAVES]
            continue
        out += [(dense + "/lora_a", (K, r)), (dense + "/lora_b", (r, N))]
        if cfg.dora:
            out.append((dense + "/lora_m", (N,)))
    return out


def scratch_runs(leaves, adapted):
    """The compact layout of the dW scratch: ([(start, end, base)], size).  A merged launch (ops.linear_multi) writes its whole group at
    the masters' relative offsets, and a group is a run of same-shape Dense kernels laid out back to back.  So every maximal such run
    that holds an adapted leaf gets one slot of its own length at `base`, and master element e of the run [start, end) lives at scratch
    element base + e - start: inside a run the masters' distances are kept, a group or a single leaf never straddles two runs, and runs
    without an adapted leaf take no room.  A run that is only partly adapted gets room for all of it (the extra gradients are computed
    and ignored).  An adapted convolution kernel (4-D, LoCon) is a run of its own: no merged launch serves convolutions, so it never
    joins a group.  Starts, ends and bases are multiples of 8 elements; the runs are in master order."""
    dense = sorted((lf for lf in leaves.values() if lf.path.endswith("/kernel") and len(lf.shape) == 2 and lf.batch == 1
                    and (lf.R, lf.C) == (lf.Rp, lf.Cp)), key=lambda lf: lf.offset)
    spans = [(lf.offset, lf.offset + lf.numel) for lf in leaves.values() if len(lf.shape) == 4 and lf.path in adapted]
    i = 0
    while i < len(dense):
        j = i
        while (j + 1 < len(dense) and dense[j + 1].shape == dense[i].shape
               and dense[j + 1].offset == dense[j].offset + dense[j].numel):
            j += 1
        if any(lf.path in adapted for lf in dense[i: j + 1]):
            spans.append((dense[i].offset, dense[j].offset + dense[j].numel))
        i = j + 1
    runs, size = [], 0
    for start, end in sorted(spans):
        runs.append((start, end, size))
        size += (end - start + 7) // 8 * 8
    return runs, size


class LoraAdapter:
    """What attach() hangs on a frozen store: the trained A / B (/ m) leaves (self.store), the bf16 dW scratch and the job table; for
    DoRA also the parallel SdtDoraJob table and the column statistics (c, g of every adapted leaf) the merge leaves for the projection;
    for LoCon a second job table over the adapted convolution leaves with its SdtLoraSplitJob table and the split projection's workspace;
    for LoHa, beside every non-empty job table, the SdtLoraSplitJob and SdtLohaJob tables and the workspace of sdt_loha_project (self.loha)."""

    def __init__(self, base, cfg, store_kwargs):
        if base.trainable:
            raise ValueError("LoRA: the base store must be frozen (ParamStore(trainable=False)); a trained store takes no adapter")
        if getattr(base, "adapter", None) is not None:
            raise ValueError("LoRA: the store already carries an adapter")
        if getattr(base, "tokens", None) is not None:
            raise ValueError("LoRA: the store carries new tokens (tokens.attach); a text-encoder LoRA together with new tokens is not supported")
        self.base, self.cfg, self.source = base, cfg, "master"
        base_spec = [(p, base.leaves[p].shape) for p in base.order]
        self.paths = select_leaves(base_spec, cfg)
        for p in self.paths:
            lf = base.leaves[p]
            if (lf.R, lf.C) != (lf.Rp, lf.Cp) or lf.w_off != lf.offset:
                raise ValueError(f"LoRA: {p} is a padded leaf and cannot carry an adapter")
        self.adapted = {p: tuple(p[: -len("kernel")] + n for n in leaf_names(cfg)) for p in self.paths}
        kw = dict(store_kwargs)
        kw.setdefault("device", base.device)
        if cfg.dora:  # a magnitude keeps fp32 moments and takes no weight decay
            if kw.get("quant_mask") is not None or kw.get("decay_mask") is not None:
                raise ValueError("DoRA: configure the adapter store with quant_excluded / wd_excluded patterns, not with explicit quant_mask / "
                                 "decay_mask trees (they would override the exclusion of lora_m from quantisation and weight decay)")
            for k in ("quant_excluded", "wd_excluded"):
                kw[k] = tuple(kw.get(k, ())) + ("lora_m",)
        self.store = ParamStore(adapter_spec(base_spec, cfg), trainable=True, **kw)
        self.store.lora_of = self  # (checkpoint.params_to_tree folds an EmaView of this store into the base)
        if self.store.grad16 is not None or self.store.g32_base:
            raise ValueError("LoRA: the adapter store must keep its gradients in float32")
        self.runs, size = scratch_runs(base.leaves, self.adapted)
        self._run_starts = [r[0] for r in self.runs]
        dev = base.device
        # dW of every adapted leaf (and of the non-adapted members of a merged group, computed and ignored): scratch_runs' layout
        self.scratch = torch.zeros(size, dtype=torch.bfloat16, device=dev)
        # two job tables: the Dense leaves (self.jobs_host, as without LoCon) and the convolution leaves (self.conv_jobs_host, with the
        # split table and workspace of sdt_lora_project_split beside it); merge / restore / folded launch once per non-empty table
        self.dense_paths = [p for p in self.paths if len(base.leaves[p].shape) == 2]
        self.conv_paths = [p for p in self.paths if len(base.leaves[p].shape) == 4]
        self.jobs_host = self._job_table(self.dense_paths)
        self.jobs_dev = self._to_device(self.jobs_host)
        self._tables = [(self.dense_paths, self.jobs_host, self.jobs_dev)]
        self.dora_host = self.dora_dev = self.stats = None
        if cfg.dora:
            dora, sm, so = [], 0, 0
            for p, j in zip(self.dense_paths, self.jobs_host):
                lm = self.store.leaves[self.adapted[p][2]]
                dora.append(_lib.SdtDoraJob(lm.offset, lm.offset, so, j.N, sm))
                sm += (j.N + 63) // 64
                so += 2 * j.N  # c [N], then g [N]
            self.dora_host = (_lib.SdtDoraJob * len(dora))(*dora)
            self.dora_dev = self._to_device(self.dora_host)
            self.stats = torch.zeros(so, dtype=torch.float32, device=dev)
        self.conv_jobs_host = self.conv_jobs_dev = self.split_host = self.split_dev = self.split_ws = None
        if self.conv_paths:
            self.conv_jobs_host = self._job_table(self.conv_paths)
            self.conv_jobs_dev = self._to_device(self.conv_jobs_host)
            self._tables.append((self.conv_paths, self.conv_jobs_host, self.conv_jobs_dev))
            self.split_host = self._split_table(self.conv_jobs_host)
            self.split_dev = self._to_device(self.split_host)
            if cfg.algo == "lora":
                self.split_ws = self._workspace("sdt_lora_project_split_workspace_bytes", self.conv_jobs_host)
        # LoHa: per non-empty job table (jobs_host, jobs_dev, split_host, split_dev, loha_host, loha_dev, workspace)
        self.loha = [self._loha_tables(*t) for t in self._tables if t[0]] if cfg.algo == "loha" else []
        self.init_weights()
        base.adapter = self
        if dev.type == "cuda":
            self.merge()

    def _to_device(self, table):
        return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.base.device)

    def _job_table(self, paths):
        """The SdtLoraJob table of `paths`, with the running first tiles of its merge and its projection."""
        jobs, tm, tp = [], 0, 0
        for p in paths:
            lf = self.base.leaves[p]
            la, lb = (self.store.leaves[q] for q in self.adapted[p][:2])
            K, N, r, scale = leaf_factors(lf.shape, self.cfg)
            ta, tb = (K + 63) // 64, (N + 63) // 64
            jobs.append(_lib.SdtLoraJob(lf.offset, la.offset, lb.offset, lf.w_off, lf.offset, self.scratch_offset(lf.offset, lf.offset + lf.numel),
                                        la.offset, lb.offset, K, N, r, scale, tm, tp, ta, 0))
            tm += ta * tb
            tp += ta + tb
        return (_lib.SdtLoraJob * len(jobs))(*jobs)

    def _split_table(self, jobs_host):
        """The SdtLoraSplitJob table beside a job table: chunks of sdt_lora_project_split_rows() rows, and the running first workgroup,
        first arrival counter and (one-sided) partial offset of every job."""
        rows = _lib.load().sdt_lora_project_split_rows()
        split, ts, cnt, part = [], 0, 0, 0
        for j in jobs_host:
            tb, chunks = (j.N + 63) // 64, (j.K + rows - 1) // rows
            split.append(_lib.SdtLoraSplitJob(part, j.K, j.N, ts, chunks, cnt, 0))
            ts += j.tiles_da + tb * chunks
            cnt += tb
            part += tb * chunks * j.r * 64 if chunks > 1 else 0
        return (_lib.SdtLoraSplitJob * len(split))(*split)

    def _workspace(self, sizer, jobs_host):
        """The workspace `sizer` asks for: arrival counters (zero between launches) and partials, allocated and zeroed once so that a
        captured step replays it."""
        need = getattr(_lib.load(), sizer)(jobs_host, len(jobs_host))
        if need < 0:
            raise _lib.SdtError(f"{sizer}: {_lib.load().sdt_last_error().decode()}")
        return torch.zeros(need, dtype=torch.uint8, device=self.base.device)

    def _loha_tables(self, paths, jobs_host, jobs_dev):
        """The SdtLoraSplitJob and SdtLohaJob tables beside one job table and the workspace of sdt_loha_project (two partial sets per
        job of more than one chunk: a LoHa partial offset is twice the split table's)."""
        split_host = self._split_table(jobs_host)
        loha = []
        for p, j, x in zip(paths, jobs_host, split_host):
            la2, lb2 = (self.store.leaves[q] for q in self.adapted[p][2:])
            loha.append(_lib.SdtLohaJob(la2.offset, lb2.offset, la2.offset, lb2.offset, 2 * x.part_off, j.K, j.N))
        loha_host = (_lib.SdtLohaJob * len(loha))(*loha)
        return (jobs_host, jobs_dev, split_host, self._to_device(split_host), loha_host, self._to_device(loha_host),
                self._workspace("sdt_loha_project_workspace_bytes", jobs_host))

    # ------------------------------------------------------------------ parameters
    def init_weights(self):
        """A: Kaiming-uniform (a = sqrt(5): U(-1/sqrt(K), 1/sqrt(K))) drawn on the host from cfg.seed in leaf order; B: zero; m (DoRA):
        the column norms of W0 + s * A @ B = W0 by the merge kernel's own reduction, so that the first merge finds g == 1.0f exactly."""
        g = torch.Generator().manual_seed(int(self.cfg.seed))
        tree = {}
        if self.cfg.algo == "loha":  # LyCORIS: A1 ~ N(0, 1), B1 ~ N(0, 0.1^2), A2 ~ N(0, 1), B2 = 0 - the delta starts at exactly zero
            for p in self.paths:     # and only B2 receives a gradient on the first step; drawn in leaf order
                a1, b1, a2, b2 = self.adapted[p]
                (K, r), (_, N) = self.store.leaves[a1].shape, self.store.leaves[b1].shape
                tree[a1] = torch.randn(K, r, generator=g)
                tree[b1] = torch.randn(r, N, generator=g) * 0.1
                tree[a2] = torch.randn(K, r, generator=g)
                tree[b2] = torch.zeros(r, N)
            self.store.load(tree)
            return
        for p in self.paths:
            a, b = self.adapted[p][:2]
            K, r = self.store.leaves[a].shape  # (a convolution's K = kh * kw * Cin: the fan-in of its down-convolution)
            tree[a] = (torch.rand(K, r, generator=g) * 2 - 1) / math.sqrt(K)
            tree[b] = torch.zeros(self.store.leaves[b].shape)
            if self.cfg.dora:
                tree[self.adapted[p][2]] = torch.zeros(self.store.leaves[self.adapted[p][2]].shape)
        self.store.load(tree)
        if self.cfg.dora:
            self.init_magnitude()

    def init_magnitude(self):
        """m = the column norms of W0 + s * A @ B at the master's current A and B.  On a GPU store by sdt_dora_init_magnitude; on a CPU
        store (host-logic tests only) by a float64 norm rounded to fp32.  Like ParamStore.load, it writes the master from outside a
        step: the EMA's m (when the store keeps one) becomes the master's - an EMA that started at m = 0 would merge adapted kernels
        with a gain near zero for its first thousands of steps - and the store's bf16 copies are refreshed."""
        self.store.begin_external_write()
        if self.base.device.type == "cuda":
            _lib.call("sdt_dora_init_magnitude", self.base.master.data_ptr(), self.store.master.data_ptr(), self.store.master.data_ptr(),
                      self.jobs_host, self.dora_host, self.jobs_dev.data_ptr(), self.dora_dev.data_ptr(), len(self.jobs_host), self._stream())
        else:
            bf = lambda t: t.to(torch.bfloat16).double()
            for p in self.paths:
                a, b, m = self.adapted[p]
                v = self.base.p(p).double() + self.cfg.scale * (bf(self.store.p(a)) @ bf(self.store.p(b)))
                self.store.p(m).copy_(v.pow(2).sum(0).sqrt().float())
        if self.store.ema is not None:
            for p in self.paths:
                lm = self.store.leaves[self.adapted[p][2]]
                self.store.ema[lm.offset: lm.offset + lm.numel].copy_(self.store.master[lm.offset: lm.offset + lm.numel])
        if self.base.device.type == "cuda":
            self.store.prepare(full=True)  # whoever writes the master refreshes the bf16 copies

    def scratch_offset(self, a, b):
        """The scratch element of master element a; [a, b) must lie inside one run of scratch_runs."""
        i = bisect.bisect_right(self._run_starts, a) - 1
        if i < 0 or a > b or b > self.runs[i][1]:
            raise _lib.SdtError(f"LoRA: gradient range [{a}, {b}) lies outside the runs the adapter's scratch holds")
        start, _, base = self.runs[i]
        return base + a - start

    def scratch_view(self, a, b):
        """bf16 view of the dW scratch for master elements [a, b) (ops: the weight-gradient destination of an adapted leaf / group)."""
        o = self.scratch_offset(a, b)
        return self.scratch[o: o + b - a]

    def takes(self, wpaths):
        return any(p in self.adapted for p in wpaths)

    # ------------------------------------------------------------------ launches
    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _merge_into(self, ab, w_ptr, f_ptr, stats):
        """The merge of every table, factors from `ab`, into the bf16 mirror at w_ptr and / or the fp32 buffer at f_ptr (None: not
        written).  LoHa: w = bf16(W0 + s * (A1 @ B1) * (A2 @ B2)); DoRA also leaves c and g of every leaf in `stats`."""
        w0, ab, stream = self.base.master.data_ptr(), ab.data_ptr(), self._stream()
        if self.loha:
            for jh, jd, _, _, xh, xd, _ in self.loha:
                _lib.call("sdt_loha_merge", w0, ab, w_ptr, f_ptr, jh, xh, jd.data_ptr(), xd.data_ptr(), len(jh), stream)
        elif self.cfg.dora:
            _lib.call("sdt_dora_merge", w0, ab, w_ptr, f_ptr, stats.data_ptr(), self.jobs_host, self.dora_host, self.jobs_dev.data_ptr(),
                      self.dora_dev.data_ptr(), len(self.jobs_host), stream)
        else:
            for _, jh, jd in self._tables:
                _lib.call("sdt_lora_merge", w0, ab, w_ptr, f_ptr, jh, jd.data_ptr(), len(jh), stream)

    def merge(self, source=None):
        """w[leaf] = bf16(W0 + s * A @ B) for every adapted leaf (one launch per table), A / B from the adapter store's master or its
        EMA.  The choice sticks: source=None (ParamStore.prepare, so StableDiffusionPipeline.generate) merges what was merged last;
        train_step merges "master".  DoRA: self.stats is what project() reads."""
        source = self.source if source is None else source
        if source not in ("master", "ema"):
            raise ValueError(f"merge: source must be 'master' or 'ema', not {source!r}")
        ab = self.store.master if source == "master" else self.store.ema
        if ab is None:
            raise ValueError("merge(source='ema'): the adapter store keeps no EMA")
        self.source = source
        self._merge_into(ab, self.base.w.data_ptr(), None, self.stats)

    def restore(self):
        """w[leaf] = bf16(W0) for every adapted leaf (one launch per table, sdt_lora_restore): the mirror of the store without its
        adapter, bit for bit - the reference model of a Diffusion-DPO step.  The inverse of merge() as far as the mirror is concerned;
        self.source (what a later merge(None) merges) and, for DoRA, self.stats (what project() reads) stay what the last merge left."""
        for _, jh, jd in self._tables:
            _lib.call("sdt_lora_restore", self.base.master.data_ptr(), self.base.w.data_ptr(), jh, jd.data_ptr(), len(jh), self._stream())

    def project(self):
        """dA, dB of every adapted leaf from the dW scratch into the adapter store's gradient (one launch; with LoCon a second one,
        sdt_lora_project_split, for the convolution table; written, not accumulated)."""
        from . import ops
        dw, ab, grad, stream = self.scratch.data_ptr(), self.store.master.data_ptr(), self.store.grad.data_ptr(), self._stream()
        if self.loha:  # the four factor gradients of every leaf: one launch per table (include/sdt.h "LoHa")
            for jh, jd, sh, sd, xh, xd, ws in self.loha:
                _lib.call("sdt_loha_project", dw, ab, grad, jh, sh, xh, jd.data_ptr(), sd.data_ptr(), xd.data_ptr(), len(jh), ws.data_ptr(),
                          ws.numel(), stream)
        elif self.cfg.dora:  # also dm, from the c and g the step's merge left in self.stats
            _lib.call("sdt_dora_project", dw, self.base.master.data_ptr(), ab, grad, self.stats.data_ptr(), self.jobs_host, self.dora_host,
                      self.jobs_dev.data_ptr(), self.dora_dev.data_ptr(), len(self.jobs_host), stream)
        else:
            _lib.call("sdt_lora_project", dw, ab, grad, self.jobs_host, self.jobs_dev.data_ptr(), len(self.jobs_host), stream)
            if self.conv_paths:  # tall K: the dB stripes split along K (include/sdt.h "LoCon")
                _lib.call("sdt_lora_project_split", dw, ab, grad, self.conv_jobs_host, self.split_host, self.conv_jobs_dev.data_ptr(),
                          self.split_dev.data_ptr(), len(self.conv_jobs_host), self.split_ws.data_ptr(), self.split_ws.numel(), stream)
        for p in self.paths:
            ops._ready(self.store, *self.adapted[p])

    def folded(self, source="master"):
        """{path: fp32 tensor} of the base with the adapter folded in (W0 + s * A @ B by the merge kernel's fp32 output: its bf16
        rounding is the training-time mirror bit for bit) - what save_model writes as an ordinary checkpoint."""
        ab = self.store.master if source == "master" else self.store.ema
        if ab is None:
            raise ValueError("folded(source='ema'): the adapter store keeps no EMA")
        buf = self.base.master.clone()
        # (DoRA: statistics of its own, bound to a name until the call has been enqueued - self.stats stays what the last merge into
        # the mirror left)
        stats = torch.empty_like(self.stats) if self.cfg.dora else None
        self._merge_into(ab, None, buf.data_ptr(), stats)
        return {p: buf[lf.offset: lf.offset + lf.numel].view(lf.shape) for p, lf in self.base.leaves.items()}

    # ------------------------------------------------------------------ adapter file
    def _meta(self):
        meta = dict(rank=int(self.cfg.rank), alpha=float(self.cfg.alpha), targets=list(self.cfg.targets),
                    base_shapes={p: list(self.base.leaves[p].shape) for p in self.paths})
        if self.cfg.dora:  # (a LoRA file stays byte for byte what it was)
            meta["dora"] = True
        if self.cfg.conv_rank:
            meta.update(conv_rank=int(self.cfg.conv_rank), conv_alpha=float(self.cfg.conv_scale * self.cfg.conv_rank),
                        conv_targets=list(self.cfg.conv_targets))
        if self.cfg.algo != "lora":
            meta["algo"] = self.cfg.algo
        return meta

    def save(self, path, which="master"):
        """One .npz: the A / B (/ m) leaves (fp32) and __meta__ (JSON: rank, alpha, targets, the adapted base kernels' shapes, and
        "dora": true for a DoRA adapter, conv_rank / conv_alpha / conv_targets for a LoCon adapter, "algo": "loha" for a LoHa adapter,
        whose leaves are A1 / B1 / A2 / B2)."""
        tree = self.store.export_host(which)
        with open(path, "wb") as f:
            np.savez(f, __meta__=np.frombuffer(json.dumps(self._meta()).encode(), dtype=np.uint8), **{p: np.asarray(v) for p, v in tree.items()})

    def load(self, path):
        """Inverse of save().  ValueError naming the mismatch for a file of another rank, another alpha, other targets, another conv_rank / conv_alpha / conv_targets or other base shapes."""
        with np.load(path) as z:
            if "__meta__" not in z.files:
                raise ValueError(f"{path}: not an adapter file (no __meta__)")
            meta = json.loads(bytes(z["__meta__"]).decode())
            mine = self._meta()
            if meta.get("algo", "lora") != mine.get("algo", "lora"):
                kind = lambda m: "LoHa" if m.get("algo", "lora") == "loha" else "DoRA" if m.get("dora", False) else "LoRA"
                raise ValueError(f"{path}: a {kind(meta)} adapter file, this adapter is a {kind(mine)} adapter (attach with algo="
                                 f"{meta.get('algo', 'lora')!r})")
            if bool(meta.get("dora", False)) != bool(mine.get("dora", False)):
                kind = lambda m: "DoRA" if m.get("dora", False) else "LoRA"
                raise ValueError(f"{path}: a {kind(meta)} adapter file, this adapter is a {kind(mine)} adapter (attach with dora="
                                 f"{bool(meta.get('dora', False))})")
            if meta["rank"] != mine["rank"]:
                raise ValueError(f"{path}: adapter of rank {meta['rank']}, this adapter has rank {mine['rank']}")
            if list(meta["targets"]) != mine["targets"]:
                raise ValueError(f"{path}: adapter for targets {meta['targets']}, this adapter has targets {mine['targets']}")
            if float(meta["alpha"]) != mine["alpha"]:
                raise ValueError(f"{path}: adapter trained with alpha {meta['alpha']}, this adapter has alpha {mine['alpha']} (the factors "
                                 "mean another delta under another scale: attach with the file's alpha)")
            if int(meta.get("conv_rank", 0)) != mine.get("conv_rank", 0):
                raise ValueError(f"{path}: adapter of conv_rank {int(meta.get('conv_rank', 0))}, this adapter has conv_rank "
                                 f"{mine.get('conv_rank', 0)}")
            if mine.get("conv_rank", 0):
                if list(meta["conv_targets"]) != mine["conv_targets"]:
                    raise ValueError(f"{path}: adapter for conv_targets {meta['conv_targets']}, this adapter has conv_targets "
                                     f"{mine['conv_targets']}")
                if float(meta["conv_alpha"]) != mine["conv_alpha"]:
                    raise ValueError(f"{path}: adapter trained with conv_alpha {meta['conv_alpha']}, this adapter has conv_alpha "
                                     f"{mine['conv_alpha']} (attach with the file's conv_alpha)")
            if meta["base_shapes"] != mine["base_shapes"]:
                a, b = meta["base_shapes"], mine["base_shapes"]
                bad = sorted(set(a) ^ set(b)) or [p for p in b if a[p] != b[p]]
                raise ValueError(f"{path}: adapter for other base shapes ({len(bad)} kernels differ, first {bad[0]}: "
                                 f"{a.get(bad[0])} in the file, {b.get(bad[0])} here)")
            tree = {p: torch.from_numpy(np.array(z[p])) for p in self.store.order}
        self.store.load(tree)
        if self.base.device.type == "cuda":
            self.merge()


def attach(base_store, cfg, **store_kwargs):
    """Hang a LoRA adapter on the frozen `base_store`.  store_kwargs configure the adapter's own ParamStore (quantise, quant_excluded,
    wd_excluded, block_size, with_ema, optimizer, adam_betas, prodigy).  ValueError: a trained base, a target that matches a convolution or a
    padded kernel, no matching leaf (Dense, or with conv_rank > 0 convolution), an invalid rank."""
    if not isinstance(cfg, LoraConfig):
        raise ValueError(f"attach: cfg must be a LoraConfig, not {type(cfg).__name__}")
    return LoraAdapter(base_store, cfg, store_kwargs)
