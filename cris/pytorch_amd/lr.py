"""Per-step learning-rate tables for NativeTrainer(lr_schedule=...) / set_lr_schedule: float32 arrays [n_steps, n_groups], row t =
the rates of 0-based optimizer step t (the trainer takes two groups: backbone, rest; steps past the end use the last row).

Host only, numpy; all arithmetic in float64, rounded to float32 once at the end.  The trainer copies the values to the device and
the step copies them into the Adam tables (csrc/lr.hip), so what is computed here is what the update uses, bit for bit.  The closed
forms are those of torch.optim.lr_scheduler (MultiStepLR, CosineAnnealingLR, PolynomialLR, LinearLR); from_torch records any torch
scheduler as it is.  (Not called `schedule`: in this package that word means launch schedules.)
"""
import bisect
import math

import numpy as np


def _finish(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).astype(np.float32))


def _base(base_lrs):
    b = np.atleast_1d(np.asarray(base_lrs, dtype=np.float64))
    if b.ndim != 1 or b.size < 1:
        raise ValueError("base_lrs must be a number or a sequence of numbers (one per group), got %r" % (base_lrs,))
    return b


def _steps(n_steps):
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise ValueError("n_steps must be an integer >= 1, got %r" % (n_steps,))
    return int(n_steps)


def reference_epochs(base_lr, lr_multi, milestones, gamma, steps_per_epoch, epochs):
    """the reference's recipe as a table of steps_per_epoch * epochs rows: row t = trainer.epoch_group_lrs(t // steps_per_epoch,
    ...) - epoch 0 runs both groups at base_lr, later epochs (lr_multi * base_lr, base_lr) * gamma ** #{m <= epoch}"""
    from .trainer import epoch_group_lrs
    if steps_per_epoch < 1 or epochs < 1:
        raise ValueError("steps_per_epoch and epochs must be >= 1")
    return _finish([epoch_group_lrs(t // steps_per_epoch, base_lr, lr_multi, milestones, gamma)
                    for t in range(int(steps_per_epoch) * int(epochs))])


def constant(base_lrs, n_steps=1):
    b = _base(base_lrs)
    return _finish([b for _ in range(_steps(n_steps))])


def multistep(base_lrs, milestones, gamma, n_steps):
    """MultiStepLR: base * gamma ** #{m in milestones : m <= t}"""
    b, ms = _base(base_lrs), sorted(milestones)
    return _finish([b * float(gamma) ** bisect.bisect_right(ms, t) for t in range(_steps(n_steps))])


def cosine(base_lrs, n_steps, eta_min=0.0):
    """CosineAnnealingLR with T_max = n_steps: eta_min + (base - eta_min) * (1 + cos(pi * t / n_steps)) / 2"""
    b, n = _base(base_lrs), _steps(n_steps)
    return _finish([eta_min + (b - eta_min) * (1.0 + math.cos(math.pi * t / n)) / 2.0 for t in range(n)])


def poly(base_lrs, n_steps, power=1.0):
    """PolynomialLR with total_iters = n_steps: base * (1 - t / n_steps) ** power"""
    b, n = _base(base_lrs), _steps(n_steps)
    return _finish([b * (1.0 - t / n) ** power for t in range(n)])


def with_warmup(table, warmup_steps, start_factor):
    """rows t < warmup_steps of `table` times start_factor + (1 - start_factor) * t / warmup_steps: LinearLR(start_factor,
    end_factor=1, total_iters=warmup_steps) chained onto the table's schedule (torch's ChainedScheduler)"""
    a = np.asarray(table, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("table must be 2-d [n_steps, n_groups], got shape %r" % (a.shape,))
    if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, (int, np.integer)) or warmup_steps < 0:
        raise ValueError("warmup_steps must be an integer >= 0, got %r" % (warmup_steps,))
    if not 0.0 < start_factor <= 1.0:
        raise ValueError("start_factor must lie in (0, 1], got %r" % (start_factor,))
    a = a.copy()
    for t in range(min(int(warmup_steps), a.shape[0])):
        a[t] *= start_factor + (1.0 - start_factor) * t / warmup_steps
    return _finish(a)


def from_torch(make_scheduler, base_lrs, n_steps):
    """any torch scheduler as a table: make_scheduler(optimizer) is called on a dummy torch.optim.SGD (CPU) with one group per
    entry of base_lrs; row t = scheduler.get_last_lr() before the t-th `optimizer.step(); scheduler.step()`."""
    import torch
    b, n = _base(base_lrs), _steps(n_steps)
    opt = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": float(x)} for x in b], lr=float(b[0]))
    sched = make_scheduler(opt)
    rows = []
    for t in range(n):
        rows.append([float(x) for x in sched.get_last_lr()])
        opt.step()
        sched.step()
    return _finish(rows)
