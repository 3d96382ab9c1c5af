"""Generates tests/golden/optimizer_launches.json: every library call ParamStore.optimizer_step makes on a CPU store, per optimizer and
option, and what checkpoint.save_training_state writes for each optimizer (tests/test_optimizer_dispatch_cpu.py compares both).

A ParamStore(device="cpu") runs the whole dispatch once `params._lib.call` is replaced by a recorder, torch.cuda's capture query by
`lambda: False`, and stream=0 is passed: no kernel runs, the record is the launch list.  A launch is [symbol, [args]]; an integer that
falls inside one of the store's tensors is written "<attribute>+<byte offset>" (attributes tried in the order of POINTERS), a float
with repr, None as null.  After each case the store's count, state_whole, _grad_is_acc and _acc_norm are recorded, and the host-written
device counters and running products.

The committed file is a pin, written by the dispatch as it stood before stable_diffusion_training_amd/optimizers.py existed: a refactor of
the dispatch reproduces it and does not regenerate it.  Regenerate only with a change that is meant to alter a launch or a file.
Run:  python tests/golden/make_optimizer_launches.py
"""
import itertools
import json
import os
import sys
import tempfile
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stable_diffusion_training_amd import checkpoint, lora, lr_schedule, params  # noqa: E402
from stable_diffusion_training_amd import training_utils as tu  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "optimizer_launches.json")
# two 64x64 kernels and two vectors, one of each under the weight-decay exclusion: all four (quantised x decayed) segments are
# non-empty with quantise=True, the two quantised ones are empty with quantise=False
SPEC = [("a/kernel", (64, 64)), ("a/bias", (64,)), ("nodecay/kernel", (64, 64)), ("nodecay/scale", (64,))]
POINTERS = ("master", "w", "grad16", "grad", "gacc", "ema", "codes", "inv_scale", "mom", "codes2", "inv_scale2", "mom2", "adam_step",
            "adam_prod", "adam_cur", "prodigy_s", "prodigy_p0", "prodigy_state", "prodigy_step", "prodigy_cur", "sqnorm", "sq_ws",
            "thresholds")
SCHED = ("step", "lr_tab", "ema_tab", "cur")
OPTIMIZERS = ("lion", "adamw", "prodigy")
LR = {"lion": 1e-4, "adamw": 1e-3, "prodigy": 1.0}
WD = 0.07
EMA_RATE = 0.999


def make_store(optimizer, quantise=True, with_ema=True, scheduled=False, **kw):
    st = params.ParamStore(SPEC, device="cpu", quantise=quantise, quant_excluded=("bias", "scale"), wd_excluded=("nodecay",),
                           block_size=16, with_ema=with_ema, optimizer=optimizer, **kw)
    if scheduled:
        st.set_schedule(lr=lr_schedule.LRSchedule("cosine", LR[optimizer], num_warmup_steps=1, num_training_steps=6),
                        ema=lr_schedule.EMASchedule("warmup", EMA_RATE))
    return st


class Recorder:
    """Stands in for _lib.call: keeps (symbol, args) with the pointers named after the tensors they fall in."""

    def __init__(self, store, extra=()):
        self.store, self.extra, self.launches = store, dict(extra), []

    def tensors(self):
        st = self.store
        for name in POINTERS:
            yield name, getattr(st, name)
        for name in SCHED:
            yield "_sched." + name, None if st._sched is None else st._sched[name]
        yield from self.extra.items()

    def name(self, v):
        if v is None or isinstance(v, str):
            return v
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"launch argument {v!r} of type {type(v).__name__}")
        for name, t in self.tensors():
            if t is not None and t.data_ptr() <= v < t.data_ptr() + max(t.numel() * t.element_size(), 1):
                return f"{name}+{v - t.data_ptr()}"
        return v

    def __call__(self, symbol, *args):
        self.launches.append([symbol, [self.name(a) for a in args]])


def run(store, prepare=None, extra=(), **step_kw):
    """One optimizer_step of `store` under the two stubs.  Returns the record of the case; a ValueError is recorded by its type (and
    must have launched nothing)."""
    rec = Recorder(store, extra)
    with mock.patch.object(params._lib, "call", rec), mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: False):
        if prepare is not None:
            prepare(store)
        rec.launches.clear()
        try:
            store.optimizer_step(stream=0, **step_kw)
            raised = None
        except ValueError:
            raised = "ValueError"
    out = dict(launches=rec.launches, count=store.count, state_whole=store.state_whole, grad_is_acc=store._grad_is_acc,
               acc_norm=store._acc_norm, raised=raised)
    for name in ("adam_step", "adam_prod", "prodigy_step", "prodigy_state"):
        t = getattr(store, name)
        if t is not None:
            out[name] = [repr(x) for x in t.tolist()]
    if store._sched is not None:
        out["_sched.step"] = int(store._sched["step"])
    return out


def _acc_with_norm(st):
    st.accumulate("init", stream=0)
    st.accumulate("finish", 0.5, norm=True, stream=0)


def _acc_without_norm(st):
    st.accumulate("init", stream=0)
    st.accumulate("finish", 0.5, stream=0)


SOURCES = {"grad": (None, "grad"), "acc_norm": (_acc_with_norm, "acc"), "acc_plain": (_acc_without_norm, "acc")}


def launch_cases():
    """{case id: thunk -> record}."""
    cases = {}
    for opt, quant, sched, ema, clip, src in itertools.product(OPTIMIZERS, (True, False), (False, True), (True, False), (1.0, None),
                                                               SOURCES):
        def grid(opt=opt, quant=quant, sched=sched, ema=ema, clip=clip, src=src):
            prepare, source = SOURCES[src]
            return run(make_store(opt, quant, ema, sched), prepare, lr=LR[opt], wd=WD, max_norm=clip, ema_rate=EMA_RATE if ema else 0.0,
                       grad_source=source)
        cases[f"{opt}-{'q8' if quant else 'f32'}-{'cosine' if sched else 'const'}-{'ema' if ema else 'noema'}-"
              f"{'clip' if clip else 'noclip'}-{src}"] = grid
    for opt in ("lion", "adamw"):
        def partials(opt=opt):
            sq = torch.zeros(8, dtype=torch.float64)
            return run(make_store(opt), extra={"sq_partials": sq}, lr=LR[opt], wd=WD, ema_rate=EMA_RATE, sq_partials=(sq, 3))

        def sharded(opt=opt):
            st = make_store(opt)
            st.sharded = True
            return run(st, lr=LR[opt], wd=WD, ema_rate=EMA_RATE, shard=(st.shard_buckets(2), True))
        cases[f"{opt}-sq_partials"] = partials
        cases[f"{opt}-sharded"] = sharded
    for opt in OPTIMIZERS:
        def resumed(opt=opt):
            return run(make_store(opt, scheduled=True), lambda st: st.set_step(3), lr=LR[opt], wd=WD, ema_rate=EMA_RATE)
        cases[f"{opt}-set_step3"] = resumed
    return cases


def refusal_cases():
    """{case id: thunk -> record}: each raises ValueError before any launch."""
    return {
        "lion-eps": lambda: run(make_store("lion"), lr=1e-4, wd=WD, eps=1e-8),
        "adamw-betas": lambda: run(make_store("adamw"), lr=1e-3, wd=WD, b2=0.99),
        "prodigy-betas": lambda: run(make_store("prodigy"), lr=1.0, wd=WD, b1=0.8),
        "prodigy-shard": lambda: run(make_store("prodigy"), lr=1.0, wd=WD, shard=([(0, 2048, True, True)], True)),
        "lion-lr-not-the-schedules": lambda: run(make_store("lion", scheduled=True), lr=2e-4, wd=WD, max_norm=None),
        "adamw-lr-not-the-schedules": lambda: run(make_store("adamw", scheduled=True), lr=2e-3, wd=WD, max_norm=None),
        "lion-bad-grad_source": lambda: run(make_store("lion"), lr=1e-4, wd=WD, grad_source="gacc"),
        "adamw-acc-without-accumulate": lambda: run(make_store("adamw"), lr=1e-3, wd=WD, grad_source="acc"),
        "prodigy-acc-without-accumulate": lambda: run(make_store("prodigy"), lr=1.0, wd=WD, grad_source="acc"),
    }


# ------------------------------------------------------------------------------------------------ training-state files
LORA_SPEC = [("blk/to_q/kernel", (32, 48)), ("blk/to_q/bias", (48,)), ("blk/to_out_0/kernel", (48, 32)), ("blk/to_out_0/bias", (32,))]


def file_states(optimizer, with_lora):
    """(unet state, text-encoder state) for save_training_state: two plain stores, or a frozen base with a LoRA adapter beside a frozen
    text encoder."""
    okw = {"adamw": dict(adam_betas=(0.9, 0.99)), "prodigy": dict(prodigy=dict(d0=1e-5, growth_rate=1.02))}.get(optimizer, {})
    if not with_lora:
        u, t = make_store(optimizer, **okw), make_store(optimizer, quantise=False, with_ema=False, **okw)
    else:
        base = params.ParamStore(LORA_SPEC, device="cpu", trainable=False)
        ad = lora.attach(base, lora.LoraConfig(8, 4.0, seed=5), quantise=True, quant_excluded=("bias", "to_out_0"),
                         wd_excluded=("bias", "lora_b"), block_size=16, with_ema=True, optimizer=optimizer, **okw)
        u, t = tu.TrainState(None, base, {}, {}, ad), params.ParamStore(LORA_SPEC, device="cpu", trainable=False)
    for st in (u, t):
        store = checkpoint._stepping_store(st)[0]
        if store is not None:
            store.set_step(5)
    return u, t


def file_record(optimizer, with_lora, path):
    """What save_training_state writes for the pair: tensor names with dtype and shape, the metadata, the stepping stores' digests."""
    from safetensors import safe_open
    u, t = file_states(optimizer, with_lora)
    checkpoint.save_training_state(path, u, t)
    with safe_open(path, framework="pt") as f:
        tensors = {k: [str(f.get_tensor(k).dtype), list(f.get_tensor(k).shape)] for k in sorted(f.keys())}
        meta = dict(sorted(f.metadata().items()))
    stores = [checkpoint._stepping_store(st)[0] for st in (u, t)]
    return dict(tensors=tensors, metadata=meta, digests=[None if s is None else checkpoint._layout_digest(s) for s in stores])


def file_cases():
    return {f"{opt}-{'lora' if with_lora else 'plain'}": (opt, with_lora) for opt in OPTIMIZERS for with_lora in (False, True)}


def main():
    out = dict(launches={k: fn() for k, fn in launch_cases().items()}, refusals={k: fn() for k, fn in refusal_cases().items()}, files={})
    with tempfile.TemporaryDirectory() as d:
        for k, (opt, with_lora) in file_cases().items():
            out["files"][k] = file_record(opt, with_lora, os.path.join(d, k + ".safetensors"))
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    n = sum(len(c["launches"]) for c in out["launches"].values())
    print(f"{len(out['launches'])} cases, {n} launches, {len(out['refusals'])} refusals, {len(out['files'])} files -> {OUT}")


if __name__ == "__main__":
    main()
