"""Sampler: temperature / top-k / top-p sampling of next tokens on the device, one kernel launch per call (ops.sample_logits).

The position in the random stream is a device uint64 that the kernel reads and a device add advances after each call, as KVCache keeps
its length: drawing a token never synchronises with the host, and a captured decode step would replay with fresh numbers.  The uniform
number of (seed, row, step) is the first word of Philox4x32-10 - the row is part of the counter, so identical prompts in one batch get
different continuations, and a (seed, step) pair always gives the same tokens."""
from __future__ import annotations

import torch

from . import ops


class Sampler:
    def __init__(self, temperature=1.0, top_k=0, top_p=1.0, seed=0):
        ops.check_sampling(temperature, top_k, top_p)
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"Sampler: seed must be an integer in [0, 2^64), got {seed!r}")
        self.temperature, self.top_k, self.top_p, self.seed = float(temperature), int(top_k), float(top_p), seed
        self.step_dev = None            # device uint64 [1], created on the device of the first logits
        self.step = 0                   # host mirror (never read back from the device)

    def _counter(self, device):
        if self.step_dev is None or self.step_dev.device != device:
            # uint64 has no arithmetic in torch: the counter is kept as int64 (the same bits below 2^63) and handed over as uint64
            self._step_i64 = torch.full((1,), self.step, dtype=torch.int64, device=device)
            self.step_dev = self._step_i64.view(torch.uint64)
        return self.step_dev

    def reset(self, step=0):
        """Move to position `step` of the stream (a device fill, no synchronisation)."""
        self.step = int(step)
        if self.step_dev is not None:
            self._step_i64.fill_(self.step)

    def __call__(self, logits, return_info=False):
        """logits fp32 [B, V] on the device -> tokens int64 [B]; the stream position advances by one."""
        ops.check_sampling(self.temperature, self.top_k, self.top_p, logits.shape[-1] if isinstance(logits, torch.Tensor) and logits.dim() == 2 else None)
        step = self._counter(logits.device) if isinstance(logits, torch.Tensor) and logits.is_cuda else None
        out = ops.sample_logits(logits, self.temperature, self.top_k, self.top_p, seed=self.seed, step=step, return_info=return_info)
        self._step_i64.add_(1)          # a device op, ordered after the kernel on the current stream
        self.step += 1
        return out
