"""Learning-rate and EMA-rate schedules of the optimizer step, computed on the host in float64.

The reference's lion_8bit takes a ScalarOrSchedule learning rate (lion_quant.py:159-211, chained through optax's
_scale_by_learning_rate); its EMA (compute_model_ema, training_utils.py:537-544) runs at one fixed rate.  This module gives both a
per-step value:

* LRSchedule: the six diffusers / transformers `get_scheduler` names.  The rate of step t is base_lr * lambda(t) with lambda the
  multiplier of transformers.optimization as torch's LambdaLR applies it (diffusers' optimization.py has the same lambdas).  t is the
  number of optimizer steps the store has taken before this one (0 for the first), optax's `count` and LambdaLR's `last_epoch`.
  With a warmup, step 0 therefore applies an update of size 0 (Lion's momentum still advances).  From t = num_training_steps on, the
  value of the last planned step (t = num_training_steps - 1) is held: transformers keeps evaluating its formula there (cosine rises
  again, cosine_with_restarts and linear drop to 0).
* EMASchedule: "constant" (the rate ema_rate on every step, today's behaviour) or "warmup": diffusers EMAModel.get_decay with the
  store's step t evaluated as get_decay(t + 1) (EMAModel.step increments optimization_step first), capped by ema_rate.  Step 0 has rate
  0: the EMA starts as a copy of the parameters.  The EMA arithmetic stays ema = r * ema + (1 - r) * p.

ParamStore.set_schedule uploads the tables (`lr_table`, `ema_table`): float32 -lr_t and float32 pairs (r_t, 1 - r_t), rounded exactly
as the by-value launchers of sdt_lion8_step / sdt_lion32_step round their double arguments, so a scheduled step equals a by-value step
with the same float64 scalars bit for bit.  Each table ends at the step after which its value no longer changes; the device clamps its
index to the last entry (sdt_opt_schedule_select)."""
import math

import numpy as np

LR_SCHEDULES = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")
EMA_KINDS = ("constant", "warmup")
MAX_TABLE = 1 << 25  # entries per table (a 128 MiB LR table, a 256 MiB EMA table)


def _count(name, v, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what}: {name} must be an integer, not {v!r}")
    if v < 0:
        raise ValueError(f"{what}: {name} must not be negative (got {v})")
    return int(v)


class LRSchedule:
    """rate(t) = base_lr * lambda(t) for the transformers / diffusers schedule `name`.  Arguments and defaults as transformers'
    get_*_schedule_with_warmup: num_cycles 0.5 (cosine) / 1 (cosine_with_restarts), power 1.0 and lr_end 1e-7 (polynomial).
    num_warmup_steps defaults to 0 except for constant_with_warmup, which needs it; the decaying schedules need num_training_steps."""

    def __init__(self, name, base_lr, *, num_warmup_steps=None, num_training_steps=None, num_cycles=None, power=1.0, lr_end=1e-7):
        if name not in LR_SCHEDULES:
            raise ValueError(f"unknown learning-rate schedule {name!r}: one of {', '.join(LR_SCHEDULES)}")
        what = f"lr schedule {name!r}"
        if name == "constant_with_warmup" and num_warmup_steps is None:
            raise ValueError(f"{what} needs num_warmup_steps")
        if name not in ("constant", "constant_with_warmup") and num_training_steps is None:
            raise ValueError(f"{what} needs num_training_steps")
        self.name = name
        self.base_lr = float(base_lr)
        self.num_warmup_steps = 0 if num_warmup_steps is None else _count("num_warmup_steps", num_warmup_steps, what)
        self.num_training_steps = None if num_training_steps is None else _count("num_training_steps", num_training_steps, what)
        if self.num_training_steps == 0:
            raise ValueError(f"{what}: num_training_steps must be at least 1")
        self.num_cycles = float((1 if name == "cosine_with_restarts" else 0.5) if num_cycles is None else num_cycles)
        self.power = float(power)
        self.lr_end = float(lr_end)
        if name == "polynomial" and not (self.base_lr > self.lr_end):  # transformers raises the same
            raise ValueError(f"lr_end ({self.lr_end}) must be smaller than initial lr ({self.base_lr})")

    def _lambda(self, t):
        """transformers.optimization's _get_*_lr_lambda(t), statement for statement."""
        w, n, name = self.num_warmup_steps, self.num_training_steps, self.name
        if name == "constant":
            return 1.0
        if name == "constant_with_warmup":
            if t < w:
                return float(t) / float(max(1.0, w))
            return 1.0
        if t < w:
            return float(t) / float(max(1, w))
        if name == "linear":
            return max(0.0, float(n - t) / float(max(1, n - w)))
        if name == "polynomial":
            if t > n:
                return self.lr_end / self.base_lr
            pct_remaining = 1 - (t - w) / (n - w)
            decay = (self.base_lr - self.lr_end) * pct_remaining ** self.power + self.lr_end
            return decay / self.base_lr
        progress = float(t - w) / float(max(1, n - w))
        if name == "cosine":
            factor = 0.5 * (1.0 + math.cos(math.pi * float(self.num_cycles) * 2.0 * progress))
            return max(0, factor * (1 - 0.0) + 0.0)
        if progress >= 1.0:  # cosine_with_restarts
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(self.num_cycles) * progress) % 1.0))))

    def table_len(self):
        """Entries up to the step after which the value no longer changes."""
        if self.name == "constant":
            return 1
        if self.name == "constant_with_warmup":
            return self.num_warmup_steps + 1
        return self.num_training_steps

    def rate(self, t):
        """float64 learning rate of the step taken with t steps before it (held past the planned steps)."""
        t = _count("t", t, "lr schedule")
        return self.base_lr * self._lambda(min(t, self.table_len() - 1))

    def rates(self, n=None):
        """float64 rates of steps 0 .. n - 1 (default: the table's length)."""
        n = self.table_len() if n is None else n
        return np.array([self.rate(t) for t in range(n)], dtype=np.float64)

    def table(self):
        """float32 -lr_t, t = 0 .. table_len() - 1 (the by-value launchers' (float)(-lr))."""
        n = self.table_len()
        if n > MAX_TABLE:
            raise ValueError(f"lr schedule {self.name!r}: a table of {n} steps exceeds {MAX_TABLE}")
        return (-self.rates(n)).astype(np.float32)

    def __repr__(self):
        return (f"LRSchedule({self.name!r}, {self.base_lr!r}, num_warmup_steps={self.num_warmup_steps}, "
                f"num_training_steps={self.num_training_steps}, num_cycles={self.num_cycles}, power={self.power}, lr_end={self.lr_end})")


class EMASchedule:
    """kind "constant": r_t = ema_rate.  kind "warmup": r_t = diffusers EMAModel(decay=ema_rate, update_after_step, use_ema_warmup,
    inv_gamma, power, min_decay).get_decay(t + 1), defaults as diffusers (0, False, 1.0, 2/3, 0.0):
        s = t - update_after_step; r = 0 if s <= 0, else max(min(v, ema_rate), min_decay) with
        v = (1 + s) / (10 + s) [use_ema_warmup=False] or 1 - (1 + s / inv_gamma) ** -power [use_ema_warmup=True]."""

    def __init__(self, kind="constant", ema_rate=0.0, *, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3,
                 min_decay=0.0):
        if kind not in EMA_KINDS:
            raise ValueError(f"unknown EMA schedule kind {kind!r}: one of {', '.join(EMA_KINDS)}")
        self.kind = kind
        self.ema_rate = float(ema_rate)
        if not 0.0 <= self.ema_rate < 1.0:
            raise ValueError(f"ema_rate must lie in [0, 1) (got {self.ema_rate})")
        self.update_after_step = _count("update_after_step", update_after_step, "EMA schedule")
        self.use_ema_warmup = bool(use_ema_warmup)
        self.inv_gamma = float(inv_gamma)
        self.power = float(power)
        self.min_decay = float(min_decay)
        if self.inv_gamma <= 0.0 or self.power <= 0.0:
            raise ValueError(f"EMA schedule: inv_gamma and power must be positive (got {self.inv_gamma}, {self.power})")
        if kind == "warmup" and self.ema_rate <= 0.0:
            raise ValueError("EMA warmup needs a positive ema_rate (its cap)")

    def _values(self, s):
        """float64 r for the int64 array s = t - update_after_step (s <= 0: rate 0)."""
        sf = s.astype(np.float64)
        if self.use_ema_warmup:  # Python's float ** (C pow), as diffusers computes it, not a vectorised pow
            v = np.array([1 - (1 + x / self.inv_gamma) ** -self.power for x in s.tolist()], dtype=np.float64)
        else:
            v = (1 + sf) / (10 + sf)  # int / int in diffusers: the correctly rounded quotient, as here (exact operands)
        v = np.maximum(np.minimum(v, self.ema_rate), self.min_decay)
        return np.where(s <= 0, 0.0, v)  # get_decay returns 0 before the cap and the floor

    def _capped_step(self):
        """A step s from which the formula stays at the cap (monotone increasing value)."""
        c = 1.0 - self.ema_rate
        if self.use_ema_warmup:
            s = (c ** (-1.0 / self.power) - 1.0) * self.inv_gamma
        else:
            s = (10.0 * self.ema_rate - 1.0) / c
        return int(math.ceil(s * (1 + 1e-9))) + 16

    def rates(self, n=None):
        """float64 rates of steps 0 .. n - 1 (default: the table's length)."""
        if self.kind == "constant":
            return np.full(1 if n is None else n, self.ema_rate, dtype=np.float64)
        if n is None:
            return self._table_rates()
        return self._values(np.maximum(np.arange(n, dtype=np.int64) - self.update_after_step, 0))

    def rate(self, t):
        t = _count("t", t, "EMA schedule")
        return float(self.rates(t + 1)[t]) if self.kind == "warmup" else self.ema_rate

    def _table_rates(self):
        end = self.update_after_step + 1 + self._capped_step()
        if end > MAX_TABLE:
            raise ValueError(f"EMA warmup with ema_rate {self.ema_rate}: {end} steps before the rate reaches its cap exceed the table "
                             f"limit of {MAX_TABLE}")
        r = self.rates(end)
        ch = np.nonzero(r[1:] != r[:-1])[0]
        return r[: (int(ch[-1]) + 2) if ch.size else 1]

    def table(self):
        """float32 pairs (r_t, 1 - r_t), shape (n, 2): the by-value launchers' (float)ema_rate and (float)(1.0 - ema_rate)."""
        r = self.rates()
        return np.stack([r.astype(np.float32), (1.0 - r).astype(np.float32)], axis=1)

    def __repr__(self):
        return (f"EMASchedule({self.kind!r}, {self.ema_rate!r}, update_after_step={self.update_after_step}, "
                f"use_ema_warmup={self.use_ema_warmup}, inv_gamma={self.inv_gamma}, power={self.power}, min_decay={self.min_decay})")


def resolve(lr_scheduler, base_lr, ema_rate, lr_schedule=None, ema_schedule=None):
    """(LRSchedule, EMASchedule) for a store, or None when nothing is scheduled ("constant" and no EMA schedule: the by-value path).
    lr_scheduler: TrainingConfig.lr_scheduler; lr_schedule: dict(num_warmup_steps=, num_training_steps=, num_cycles=, power=, lr_end=);
    ema_schedule: dict(kind=, update_after_step=, use_ema_warmup=, inv_gamma=, power=, min_decay=) - the cap is ema_rate.
    A name that needs step counts raises ValueError without them."""
    name = lr_scheduler or "constant"
    ema_kw = dict(ema_schedule or {})
    kind = ema_kw.pop("kind", "warmup" if ema_schedule else "constant")
    if name == "constant" and kind == "constant":
        return None
    lr = LRSchedule(name, base_lr, **dict(lr_schedule or {}))
    ema = EMASchedule(kind, ema_rate, **ema_kw)
    return lr, ema
