"""The three optimizers of a ParamStore - Lion (the reference's), AdamW and Prodigy - and everything that tells them apart: their
settings and checks, the state buffers a store holds for them, the state set_step rebuilds, the launches of one step, what the state
builder and a training-state file take from them.  ParamStore, checkpoint, dp and training_utils ask the store's `opt`; none of them
compares an optimizer's name.

A state table row is Buf(name, dtype, extent, init, saved, gather): the store attribute, how many elements (one per quantised element
QUANT, one per quantisation block BLOCK, the fp32 tail [quant_total, total) TAIL, the whole store WHOLE, or an int: a fixed small
block), the initial value (a number, or the list of values), whether training-state files hold the buffer, and whether the sharded
optimizer all-gathers it (dp.GradReducer.gather_state; the fp32 tail is replicated and the small blocks are the same on every rank)."""
import math
from collections import namedtuple

import torch

from . import _lib

QUANT, BLOCK, TAIL, WHOLE = "quant", "block", "tail", "whole"
Buf = namedtuple("Buf", "name dtype extent init saved gather", defaults=(False, False))
_F32, _F64, _I64 = torch.float32, torch.float64, torch.int64
# Prodigy's store-level settings (include/sdt.h "Prodigy"): what the device state is built from.  beta3 None: sqrt(b2).  lr, eps and
# the weight decay are arguments of optimizer_step, as for the other optimizers.
PRODIGY_DEFAULTS = dict(b1=0.9, b2=0.999, beta3=None, d0=1e-6, d_coef=1.0, growth_rate=float("inf"), use_bias_correction=False,
                        safeguard_warmup=False)
PRODIGY_STATE_DOUBLES = 10  # {d, d_max, numer, P1, P2, dot, l1, q, lr_t, 0}
_DICT_KEYS = frozenset({"name", "b1", "b2", "eps", "weight_decay"})  # of the state builder's optimizer=dict(...)


def prodigy_settings(given):
    """PRODIGY_DEFAULTS overridden by `given`, checked: ValueError for an unknown key, a non-finite value, d0 <= 0, d_coef <= 0,
    growth_rate <= 0 or NaN, or a beta outside [0, 1)."""
    given = dict(given or {})
    unknown = set(given) - set(PRODIGY_DEFAULTS)
    if unknown:
        raise ValueError(f"ParamStore: prodigy= takes {sorted(PRODIGY_DEFAULTS)}, not {sorted(unknown)} (lr, eps and the weight decay "
                         "are optimizer_step's)")
    hp = dict(PRODIGY_DEFAULTS, **given)
    for k in ("b1", "b2", "d0", "d_coef", "growth_rate"):
        hp[k] = float(hp[k])
    hp["beta3"] = math.sqrt(hp["b2"]) if hp["beta3"] is None else float(hp["beta3"])
    for k in ("use_bias_correction", "safeguard_warmup"):
        hp[k] = bool(hp[k])
    if not all(math.isfinite(hp[k]) for k in ("b1", "b2", "beta3", "d0", "d_coef")) or math.isnan(hp["growth_rate"]):
        raise ValueError(f"ParamStore: non-finite Prodigy setting in {hp!r}")
    if not all(0.0 <= hp[k] < 1.0 for k in ("b1", "b2", "beta3")):
        raise ValueError(f"ParamStore: Prodigy's b1, b2 and beta3 must lie in [0, 1), got {hp['b1']!r}, {hp['b2']!r}, {hp['beta3']!r}")
    if hp["d0"] <= 0.0:
        raise ValueError(f"ParamStore: Prodigy's d0 must be positive, got {hp['d0']!r}")
    if hp["d_coef"] <= 0.0 or hp["growth_rate"] <= 0.0:
        raise ValueError(f"ParamStore: Prodigy's d_coef and growth_rate must be positive, got {hp['d_coef']!r}, {hp['growth_rate']!r}")
    return hp


def adam_products(n, b1, b2):
    """(b1^n, b2^n) as n sequential float64 products from 1.0 - what sdt_adamw_select has carried on the device after n steps, bit for
    bit (one IEEE multiplication per step, no pow).  Stops once both have underflowed to 0."""
    p1 = p2 = 1.0
    for _ in range(int(n)):
        p1 *= b1
        p2 *= b2
        if p1 == 0.0 and p2 == 0.0:
            break
    return p1, p2


class Lion:
    """The reference's optimizer: 8-bit momentum codes + per-block scales for the quantised leaves (quant(0) == 3, the codec's offset),
    fp32 momentum for the others.  Its files and layout digests name no optimizer: they are what they were before there was a choice."""
    name = "lion"
    moments = {"m": ("codes", "inv_scale", "mom")}  # export_momentum(which): (codes, scales, fp32 tail)
    workspace = "sdt_sqnorm_workspace_bytes"        # the _lib symbol that sizes the store's sq_ws
    unshardable = None                              # or why dp.GradReducer(shard=True) refuses a store of this optimizer
    prodigy = None                                  # ParamStore.prodigy
    always_selects = False  # its select launch (which takes the schedule's tables) runs only with a schedule installed
    keys = _DICT_KEYS       # of the state builder's optimizer= dict (a Lion dict with more than the name is refused: parse)
    state = (Buf("codes", torch.int8, QUANT, 3, True, True), Buf("inv_scale", _F32, BLOCK, 1, True, True), Buf("mom", _F32, TAIL, 0, True))

    def __init__(self, adam_betas=None):
        self.adam_betas = tuple(float(b) for b in ((0.9, 0.999) if adam_betas is None else adam_betas))  # ParamStore.adam_betas

    @staticmethod
    def builder(rate, scale, opt):
        """(TrainState.hyper, ParamStore keywords) of create_lion_optimizer_states for its learning rate, adam_to_lion_scale_factor and
        optimizer= dict."""
        return dict(lr=rate / scale, wd=1e-2 * scale, b1=0.9, b2=0.99, max_norm=1.0), {}

    def file_meta(self):
        """What a training-state file records about the optimizer, under "<model>.<key>"."""
        return {}

    def step_args(self, b1, b2, eps, shard):
        """optimizer_step's (b1, b2, eps) resolved against the store's settings; ValueError for what this optimizer refuses."""
        if eps is not None:
            raise ValueError("optimizer_step: eps belongs to AdamW; this store's optimizer is Lion (ParamStore(optimizer='adamw'))")
        return 0.9 if b1 is None else b1, 0.99 if b2 is None else b2, None

    def set_step(self, st, n):
        """Rebuild the device state that follows from the step count alone."""

    def step(self, st, pieces, piece, *, lr, wd, b1, b2, eps, er, sq_ptr, max_norm, sc, tabs, s):
        """The launches of one step.  pieces: [(a, b, quantised, decayed)]; piece(a, quantised): the pointers of the piece at a; er: the
        EMA rate (0: off); sc / tabs: the installed schedule's device tensors and its (lr table, length, EMA table, length), or None and
        the null table; s: the stream."""
        if sc is not None:
            cur = sc["cur"].data_ptr()
            _lib.call("sdt_opt_schedule_select", sc["step"].data_ptr(), *tabs, cur, s)
        entry, rates = ("_step", (lr,)) if sc is None else ("_step_scheduled", (cur,))
        tail = (b1, b2, er, s) if sc is None else (b1, b2, s)
        bs, thr = st.block_size, st.thresholds.data_ptr()
        for (a, b, quant, decay) in pieces:
            if b == a:
                continue
            mp, gp, g16, ema_ptr, wp = piece(a, quant)
            wd_eff = wd if decay else 0.0
            if quant:  # the 8-bit streams: one code per element, one float scale per block
                _lib.call("sdt_lion8" + entry, mp, gp, g16, st.codes.data_ptr() + a, st.inv_scale.data_ptr() + 4 * (a // bs), ema_ptr, wp, b - a, bs,
                          sq_ptr, thr, max_norm, *rates, wd_eff, *tail)
            else:      # the fp32 state buffers start behind the quantised segments
                _lib.call("sdt_lion32" + entry, mp, gp, st.mom.data_ptr() + 4 * (a - st.quant_total), ema_ptr, wp, b - a, sq_ptr, max_norm, *rates,
                          wd_eff, *tail)


class AdamW:
    """include/sdt.h "AdamW": a second set of state buffers - codes2 / inv_scale2 hold the ROOT of the second moment of the quantised
    leaves (the codec has no offset: zero is code 0), mom2 the second moment of the others - and the device step counter, the two running
    products of adam_betas and the step's scalar block, which set_step rebuilds from the count."""
    name = "adamw"
    moments = {"m": ("codes", "inv_scale", "mom"), "s": ("codes2", "inv_scale2", "mom2")}
    workspace, unshardable, prodigy, always_selects, keys = Lion.workspace, None, None, True, _DICT_KEYS
    state = (Buf("codes", torch.int8, QUANT, 0, True, True), Buf("inv_scale", _F32, BLOCK, 1, True, True), Buf("mom", _F32, TAIL, 0, True),
             Buf("codes2", torch.int8, QUANT, 0, True, True), Buf("inv_scale2", _F32, BLOCK, 1, True, True), Buf("mom2", _F32, TAIL, 0, True),
             Buf("adam_step", _I64, 1, 0),   # steps taken, advanced by sdt_adamw_select
             Buf("adam_prod", _F64, 2, 1),   # b1^t, b2^t as running products
             Buf("adam_cur", _F32, 8, 0))    # the step's scalars (include/sdt.h)

    def __init__(self, adam_betas=None):
        self.adam_betas = tuple(float(b) for b in ((0.9, 0.999) if adam_betas is None else adam_betas))
        if not all(0.0 <= b < 1.0 for b in self.adam_betas):
            raise ValueError(f"ParamStore: adam_betas must lie in [0, 1), got {adam_betas!r}")

    @staticmethod
    def builder(rate, scale, opt):
        """The learning rate as given: an Adam recipe needs no translation, so adam_to_lion_scale_factor does not apply."""
        hyper = dict(lr=rate, wd=opt.get("weight_decay", 1e-2), b1=opt.get("b1", 0.9), b2=opt.get("b2", 0.999), eps=opt.get("eps", 1e-8),
                     max_norm=1.0)
        return hyper, dict(optimizer="adamw", adam_betas=(hyper["b1"], hyper["b2"]))

    def file_meta(self):
        return {"optimizer": self.name}

    def step_args(self, b1, b2, eps, shard):
        b1 = self.adam_betas[0] if b1 is None else b1
        b2 = self.adam_betas[1] if b2 is None else b2
        if (float(b1), float(b2)) != self.adam_betas:
            raise ValueError(f"optimizer_step: b1={b1!r}, b2={b2!r} but the store carries the running products of adam_betas="
                             f"{self.adam_betas!r} (set them when the store is built)")
        return b1, b2, 1e-8 if eps is None else eps

    def set_step(self, st, n):
        # the device carries b1^t and b2^t as running float64 products: rebuild them with the same n multiplications
        st.adam_step.fill_(n)
        st.adam_prod.copy_(torch.tensor(adam_products(n, *self.adam_betas), dtype=torch.float64))

    def step(self, st, pieces, piece, *, lr, wd, b1, b2, eps, er, sq_ptr, max_norm, sc, tabs, s):
        # one counter for both: adam_step indexes the schedule's tables too (the schedule's own counter and block stay unused)
        cur = st.adam_cur.data_ptr()
        _lib.call("sdt_adamw_select", st.adam_step.data_ptr(), st.adam_prod.data_ptr(), *tabs, lr, er, b1, b2, cur, s)
        bs, thr = st.block_size, st.thresholds.data_ptr()
        for (a, b, quant, decay) in pieces:
            if b == a:
                continue
            mp, gp, g16, ema_ptr, wp = piece(a, quant)
            wd_eff = wd if decay else 0.0
            if quant:
                blk = 4 * (a // bs)
                _lib.call("sdt_adamw8_step", mp, gp, g16, st.codes.data_ptr() + a, st.inv_scale.data_ptr() + blk, st.codes2.data_ptr() + a,
                          st.inv_scale2.data_ptr() + blk, ema_ptr, wp, b - a, bs, sq_ptr, thr, max_norm, cur, wd_eff, b1, b2, eps, s)
            else:
                o = 4 * (a - st.quant_total)
                _lib.call("sdt_adamw32_step", mp, gp, st.mom.data_ptr() + o, st.mom2.data_ptr() + o, ema_ptr, wp, b - a, sq_ptr, max_norm, cur,
                          wd_eff, b1, b2, eps, s)


class Prodigy:
    """include/sdt.h "Prodigy", the learning-rate-free optimizer.  ALL of its state is float32 - mom, mom2, prodigy_s and prodigy_p0 (m, v,
    s, p0) each span the whole store, master order - beside the device state block, step counter and scalar block.  set_step rebuilds the
    counter and the block's running products; d, d_max and numer stay (a checkpoint carries them), and a counter at zero makes the next
    step capture p0 again.  Not shardable: the step's two global sums would need a collective between its two sweeps."""
    name = "prodigy"
    moments = None  # no 8-bit moments: export_prodigy_state
    workspace = "sdt_prodigy_workspace_bytes"  # the moments sweep carries two sums through sq_ws
    always_selects, keys = True, _DICT_KEYS | {"lr"} | set(PRODIGY_DEFAULTS)
    unshardable = ("the sharded optimizer is not available for a Prodigy store (its two global sums would need a collective between the "
                   "two sweeps); use the all-reduce exchange")

    def __init__(self, prodigy=None):
        self.adam_betas = (0.9, 0.999)
        hp = self.prodigy = prodigy_settings(prodigy)
        # m, v, s and p0 (written by the sweep of the step that finds the counter at zero)
        whole = [Buf(n, _F32, WHOLE, 0, True) for n in ("mom", "mom2", "prodigy_s", "prodigy_p0")]
        block = [hp["d0"], hp["d0"], 0.0, 1.0, 1.0] + [0.0] * (PRODIGY_STATE_DOUBLES - 5)
        self.state = (*whole, Buf("prodigy_state", _F64, PRODIGY_STATE_DOUBLES, block, True), Buf("prodigy_step", _I64, 1, 0),
                      Buf("prodigy_cur", _F32, 8, 0))

    @staticmethod
    def builder(rate, scale, opt):
        """The config's learning rate is not used: lr multiplies the estimated d."""
        hyper = dict(lr=opt.get("lr", 1.0), wd=opt.get("weight_decay", 0.0), eps=opt.get("eps", 1e-8), max_norm=1.0)
        return hyper, dict(optimizer="prodigy", prodigy={k: opt[k] for k in PRODIGY_DEFAULTS if k in opt})

    def file_meta(self):
        """The settings as one string: the recursion a file's d, d_max and numer belong to (the finish kernel branches on d == d0; beta3,
        d_coef, growth_rate and the two flags shape every later d)."""
        return {"optimizer": self.name, "prodigy": ";".join(f"{k}={self.prodigy[k]!r}" for k in sorted(self.prodigy))}

    def step_args(self, b1, b2, eps, shard):
        hp = self.prodigy
        if shard is not None:
            raise ValueError(f"optimizer_step: {self.unshardable}")
        if (b1 is not None and float(b1) != hp["b1"]) or (b2 is not None and float(b2) != hp["b2"]):
            raise ValueError(f"optimizer_step: b1={b1!r}, b2={b2!r} but the store carries the running products of b1={hp['b1']!r}, "
                             f"b2={hp['b2']!r} (set them when the store is built: prodigy=dict(b1=, b2=))")
        return hp["b1"], hp["b2"], 1e-8 if eps is None else eps

    def set_step(self, st, n):
        st.prodigy_step.fill_(n)
        st.prodigy_state[3:5].copy_(torch.tensor(adam_products(n, self.prodigy["b1"], self.prodigy["b2"]), dtype=torch.float64))

    def step(self, st, pieces, piece, *, lr, wd, b1, b2, eps, er, sq_ptr, max_norm, sc, tabs, s):
        hp = self.prodigy
        # as for AdamW: the store's own counter indexes the schedule's tables
        cur, state = st.prodigy_cur.data_ptr(), st.prodigy_state.data_ptr()
        _lib.call("sdt_prodigy_select", st.prodigy_step.data_ptr(), state, *tabs, lr, er, b1, b2, hp["d0"], int(hp["use_bias_correction"]),
                  int(hp["safeguard_warmup"]), cur, s)

        def runs(key):
            """The non-empty pieces, neighbours with the same key joined: [a, b, key, quantised]."""
            out = []
            for (a, b, quant, decay) in pieces:
                if b > a and out and out[-1][1] == a and out[-1][2] == key(quant, decay):
                    out[-1][1] = b
                elif b > a:
                    out.append([a, b, key(quant, decay), quant])
            return out

        # a sweep per run of pieces that differ in nothing it reads: the moments sweep only cares which gradient buffer a piece lies in
        # (two launches, one from gacc), the apply sweep only about its decay (one launch without weight decay)
        bf16 = piece(0, True)[2]  # whether the quantised pieces read their gradient from the bf16 buffer
        for (a, b, _, quant) in runs(lambda quant, decay: quant and bf16):
            mp, gp, g16, ema_ptr, wp = piece(a, quant)
            _lib.call("sdt_prodigy_moments_step", mp, gp, g16, st.prodigy_p0.data_ptr() + 4 * a, st.mom.data_ptr() + 4 * a,
                      st.mom2.data_ptr() + 4 * a, st.prodigy_s.data_ptr() + 4 * a, b - a, sq_ptr, max_norm, cur, state, b1, b2, hp["beta3"],
                      st.sq_ws.data_ptr(), st.sq_ws.numel(), s)
        _lib.call("sdt_prodigy_finish", state, cur, hp["beta3"], hp["d0"], hp["d_coef"], hp["growth_rate"], eps, s)
        for (a, b, wd_eff, quant) in runs(lambda quant, decay: wd if decay else 0.0):
            mp, gp, g16, ema_ptr, wp = piece(a, quant)
            _lib.call("sdt_prodigy_apply_step", mp, st.mom.data_ptr() + 4 * a, st.mom2.data_ptr() + 4 * a, ema_ptr, wp, b - a, cur, wd_eff, s)


_CLASSES = {c.name: c for c in (Lion, AdamW, Prodigy)}
OPTIMIZERS = tuple(_CLASSES)
FILE_DEFAULT = Lion.name  # the optimizer of a training-state file that names none
STATE_NAMES = ("codes", "inv_scale", "mom", "codes2", "inv_scale2", "mom2", "adam_step", "adam_prod", "adam_cur", "prodigy_s", "prodigy_p0",
               "prodigy_state", "prodigy_step", "prodigy_cur")  # every table's attributes: None in a store whose optimizer has no such row


def for_store(optimizer, adam_betas, prodigy):
    """The optimizer object of a ParamStore(optimizer=, adam_betas=, prodigy=); adam_betas belongs to AdamW and prodigy= to Prodigy."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"ParamStore: optimizer must be one of {OPTIMIZERS}, not {optimizer!r}")
    if optimizer == Prodigy.name and adam_betas is not None:
        raise ValueError("ParamStore: adam_betas belongs to AdamW; a Prodigy store takes its betas in prodigy=dict(b1=, b2=, beta3=)")
    if optimizer != Prodigy.name and prodigy is not None:
        raise ValueError(f"ParamStore: prodigy= belongs to optimizer='prodigy'; this store's optimizer is {optimizer!r}")
    return Prodigy(prodigy) if optimizer == Prodigy.name else _CLASSES[optimizer](adam_betas)


def allocate(st, device):
    """Set every state attribute of the store `st`: its optimizer's table rows as tensors (a trained store), the others None."""
    sizes = {QUANT: max(st.quant_total, 4), BLOCK: max(st.quant_total // st.block_size, 1), TAIL: max(st.total - st.quant_total, 4),
             WHOLE: max(st.total, 4)}
    rows = {b.name: b for b in st.opt.state} if st.trainable else {}
    for name in STATE_NAMES:
        b = rows.get(name)
        if b is None:
            setattr(st, name, None)
        elif isinstance(b.init, list):
            setattr(st, name, torch.tensor(b.init, dtype=b.dtype, device=device))
        else:
            setattr(st, name, torch.full((sizes.get(b.extent, b.extent),), b.init, dtype=b.dtype, device=device))


def moments(st):
    """The store's moment buffers - the rows that grow with the store (codes, scales, fp32 moments), not the small blocks."""
    return [getattr(st, b.name) for b in st.opt.state if isinstance(b.extent, str)] if st.trainable else []


def saved(st):
    """Names of the optimizer's buffers a training-state file holds."""
    return tuple(b.name for b in st.opt.state if b.saved)


def gathered(st):
    """[(buffer, elements of the parameter range per buffer element)] of the state the sharded optimizer all-gathers."""
    return [(getattr(st, b.name), st.block_size if b.extent == BLOCK else 1) for b in st.opt.state if b.gather]


def parse(optimizer):
    """create_lion_optimizer_states' optimizer= ("lion", "adamw", "prodigy" or a dict with name=) -> (the optimizer's class, the dict)."""
    opt = {"name": optimizer} if isinstance(optimizer, str) else dict(optimizer)
    cls = _CLASSES.get(opt.get("name"))
    if cls is None or set(opt) - cls.keys:
        raise ValueError(f"optimizer: 'lion', 'adamw', 'prodigy' or dict(name=, b1=, b2=, eps=, weight_decay=) (Prodigy's dict also takes "
                         f"lr= and {sorted(set(PRODIGY_DEFAULTS) - {'b1', 'b2'})}), not {optimizer!r}")
    if cls is Lion and len(opt) > 1:
        raise ValueError("optimizer: Lion's hyper-parameters are the reference's (adam_to_lion_scale_factor); the dict form is AdamW's")
    return cls, opt
