"""A pure-Python model of vitamd_sched_advance (csrc/optim.hip): one schedule entry in, the entry advanced and the three step-dependent
floats of its row out, in the kernel's own order of operations and in Python floats (IEEE doubles), each result rounded to fp32 once.
Written from the header's description, not from vitamd.optim: test_optim_graph_host.py holds it against optim.hyper_row and
utils.lr_factor, test_gpu_optim_graph.py holds the kernel against it.  Also the cases the two files share."""
import math

import numpy as np

# the three groups of the kernel test: (base_lr, (beta1, beta2), (warmup_steps, train_steps, min_ratio) or None)
GROUPS = [(1e-3, (0.9, 0.999), (3, 8, 0.1)),
          (3e-4, (0.8, 0.95), None),
          (0.0, (0.9, 0.999), (3, 8, 0.0))]
LAUNCHES = 12                                   # crosses the warm-up milestone (3) and train_steps (8), then stays constant
PRESETS = [10 ** 3 - 1, 10 ** 5 - 1, 10 ** 7 - 1]  # counters before one launch; at 10^7 beta2^k underflows: bc2 is exactly 1


def entry(base_lr, betas, schedule, step=0, sched_t=0):
    warmup, train, ratio = schedule if schedule is not None else (0, 0, 0.0)
    return {"step": int(step), "sched_t": int(sched_t), "base_lr": float(base_lr), "beta1": float(betas[0]), "beta2": float(betas[1]),
            "min_ratio": float(ratio), "warmup_steps": int(warmup), "train_steps": int(train)}


def factor(t, warmup, train, min_ratio):
    if train == 0:
        return 1.0
    if t < warmup:
        f = t / warmup
        return f if f < 1.0 else 1.0
    if t < train:
        tt = float(t - warmup)
        return min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * tt / float(train))) / 2.0
    return 1.0


def advance(e):
    """Advances e in place -> (lr, inv_bc1, inv_sqrt_bc2) as np.float32"""
    k, t = e["step"] + 1, e["sched_t"]
    e["step"], e["sched_t"] = k, t + 1
    bc1, bc2 = 1.0 - math.pow(e["beta1"], float(k)), 1.0 - math.pow(e["beta2"], float(k))
    lr = e["base_lr"] * factor(t, e["warmup_steps"], e["train_steps"], e["min_ratio"])
    return np.float32(lr), np.float32(1.0 / bc1), np.float32(1.0 / math.sqrt(bc2))
