"""hipGraph capture of the forward + loss + backward step (torch.cuda.CUDAGraph is hipGraph on ROCm).

New functionality - the reference has no graph capture.  Every libvitamd entry point only enqueues work on the
stream it is given (include/vitamd.h), so a whole training step - the per-step weight cast, ~25 kernels per
layer, the side-stream weight-gradient GEMMs with their event fork/join, the loss - records into one graph.
What it buys: the launch-bound configurations.  BASELINE configs[0] (ViT-S, 32x32, batch 64) spends 2.8 ms per
step in Python + launch overhead eagerly and 1.4 ms replayed; the headline ViT-B/16 batch-256 step is GPU-bound
(36 ms of kernels) and gains nothing.

    step = GraphedStep(model, torch.nn.functional.cross_entropy, x_example, y_example)
    for x, y in loader:
        loss = step(x, y)          # static tensor: read it before the next call
        optim.step()               # p.grad are the graph's static gradient tensors (re-attached every call)

Shapes and dtypes are frozen at capture.  Not for dropout > 0 (the mask seed is a host value baked into the
captured launches) and not under vitamd.ddp.DataParallel: its per-parameter hooks and the per-layer `layer_ready` calls are Python
that runs DURING backward and decides, from bucket state, what to enqueue (and torch.distributed work handles are waited for on the
host in finish()); none of that replays from a graph.  A DataParallel model is refused at construction.

GraphedTrainStep records the optimiser as well: with vitamd.optim.AdamW(capturable=True) the step count, the bias corrections and the
learning-rate schedule live on the device, so the whole iteration - the update included - is one graph launch.

GraphedDecoder is the other captured form: one decode step of KV-cached generation (vitamd/decode.py) as one graph launch.  Every value
a decode step depends on lives on the device - the cache length, the sampler's stream position, the token just picked - so a replay
needs no host value and generation never synchronises.
"""
from __future__ import annotations

import contextlib
import gc

import torch

from . import decode as _decode
from . import functions as F
from . import ops as _ops


@contextlib.contextmanager
def quiet_collector():
    """Around every capture.  Cyclic garbage may hold a torch.cuda.CUDAGraph - a model that keeps its GraphedDecoder is such a cycle, the
    decoder's head being a bound method of the model - and on ROCm that object's destructor synchronises the device: refused while a
    stream captures, and fatal (an exception out of a destructor) when the cyclic collector happens to run it there.  torch.cuda.graph no
    longer collects before it captures, so: collect now, and hold the automatic collector until the capture is over."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def _fresh_workspace(device, stream):
    """Before the warm-up of a capture: forget the split-K workspace of the capture stream (ops._WORKSPACES), so that the warm-up
    allocates one that this graph alone bakes and, through the reference its owner takes after the capture, keeps alive.  Streams are
    handles out of a pool of 32, so an entry found here was left by an older graph or by eager work on a recycled handle, and
    ops._workspace replaces an entry that is too small - which would free memory that older graph still writes on replay."""
    _ops._WORKSPACES.pop((device, stream.cuda_stream), None)


class GraphedStep:
    def __init__(self, model: torch.nn.Module, loss_fn, example_x: torch.Tensor, example_y: torch.Tensor, warmup: int = 3):
        if not example_x.is_cuda:
            raise F.ops._lib.VitamdError("GraphedStep needs device tensors (there is no CPU path)")
        for m in model.modules():
            if float(getattr(m, "dropout", 0.0) or 0.0) > 0.0:      # attention dropout is applied in eval() too (reference transformer.py:28)
                raise NotImplementedError("GraphedStep with dropout > 0: the mask seed would be frozen into the graph")
        from .ddp import DataParallel
        if isinstance(model, DataParallel) or any(isinstance(m, DataParallel) for m in model.modules()):
            raise NotImplementedError("GraphedStep around vitamd.ddp.DataParallel: the bucket hooks run Python during backward (see the module docstring)")
        self.model, self.loss_fn = model, loss_fn
        self.x = example_x.detach().clone()
        self.y = example_y.detach().clone()
        self.params = [p for p in model.parameters() if p.requires_grad]
        # warm up (allocator pools, hipFuncSetAttribute one-time calls, weight-cache groups) ON THE STREAM THE CAPTURE WILL USE: autograd's
        # AccumulateGrad nodes remember the stream they were created on, and nodes created on another stream than the capturing one
        # made every replayed backward warn about (and potentially synchronise on) a stream mismatch
        s = torch.cuda.Stream()
        _fresh_workspace(self.x.device, s)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(max(1, warmup)):
                self._eager()
            model.zero_grad(set_to_none=True)      # so the captured backward ASSIGNS fresh gradient tensors
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with quiet_collector(), torch.cuda.graph(self.graph, stream=s):
            # detached: the static loss tensor must not keep the captured step's autograd graph (and with it the parameters'
            # AccumulateGrad nodes, bound to the capture stream) alive - an eager backward on another stream afterwards would warn
            self.loss = self._eager(zero=False).detach()
        self._ws = _ops._WORKSPACES.get((self.x.device, s.cuda_stream))      # kept alive: its address is in the graph
        self.grads = [p.grad for p in self.params]

    def _eager(self, zero=True):
        if zero:
            self.model.zero_grad(set_to_none=True)
        F.WEIGHTS.clear()                            # the weight casts are part of every step (the optimiser changes the weights)
        loss = self.loss_fn(self.model(self.x), self.y)
        loss.backward()
        return loss

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if x.shape != self.x.shape or y.shape != self.y.shape or x.dtype != self.x.dtype or y.dtype != self.y.dtype:
            raise F.ops._lib.VitamdError(f"GraphedStep was captured for {tuple(self.x.shape)} / {tuple(self.y.shape)}")
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        self.graph.replay()
        F.WEIGHTS.clear()                            # host-side cache state: whatever eager call comes next must re-cast
        for p, g in zip(self.params, self.grads):
            p.grad = g
        return self.loss


class GraphedTrainStep:
    """The whole training iteration as one graph launch: weight casts, forward, loss, backward, [gradient norm + clip], the advance of
    the optimiser's device-resident counters and schedule, and the update.

        optim = vitamd.optim.AdamW(model.parameters(), lr=..., capturable=True, schedule=(warmup_steps, train_steps, min_lr))
        step = GraphedTrainStep(model, lambda x, y: lm.cross_entropy(model(x), y), (x_example, y_example), optim)
        for x, y in loader:
            loss = step(x, y)          # static tensor: read it before the next call; optim.param_groups[0]["lr"] follows on the host

    step_fn(*inputs) -> 0-dim loss is free-form (`lambda tok: model.loss(tok)` for VideoGPT).  Shapes and dtypes of the inputs are frozen
    at capture; dropout > 0 and vitamd.ddp.DataParallel are refused for GraphedStep's reasons.  Construction runs forward and backward
    (never the optimiser) on the model, and the optimiser's launches once over a throw-away table: parameters, moments, step counts and
    the schedule position are what they were, and the first replay is step 1.

    The graph bakes in addresses: the parameters, the moments, the static gradients and the optimiser's resident table.  Every call
    compares them with the current ones first and captures again when one moved (`captures` counts) - after optim.load_state_dict, for
    instance, whose moments are new tensors and whose step counts re-seed the device counters."""

    def __init__(self, model: torch.nn.Module, step_fn, example_inputs, optim, warmup: int = 3):
        from . import optim as _optim
        from .ddp import DataParallel
        if isinstance(example_inputs, torch.Tensor):
            example_inputs = (example_inputs,)
        example_inputs = tuple(example_inputs)
        if not example_inputs or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in example_inputs):
            raise F.ops._lib.VitamdError("GraphedTrainStep needs device tensors as example inputs (there is no CPU path)")
        for m in model.modules():
            if float(getattr(m, "dropout", 0.0) or 0.0) > 0.0:
                raise NotImplementedError("GraphedTrainStep with dropout > 0: the mask seed would be frozen into the graph")
        if isinstance(model, DataParallel) or any(isinstance(m, DataParallel) for m in model.modules()):
            raise NotImplementedError("GraphedTrainStep around vitamd.ddp.DataParallel: the bucket hooks run Python during backward (see the module docstring)")
        if not (isinstance(optim, _optim.AdamW) and optim.capturable):
            raise ValueError("GraphedTrainStep needs vitamd.optim.AdamW(..., capturable=True): any other optimiser step reads host values "
                             "that a graph would freeze")
        self.model, self.step_fn, self.optim = model, step_fn, optim
        self.inputs = [t.detach().clone() for t in example_inputs]
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.device = self.inputs[0].device
        self.stream = torch.cuda.Stream(device=self.device)
        self.warmup = max(1, int(warmup))
        self.graph, self.loss, self.grads, self.captures, self._table, self._table_grads = None, None, [], 0, None, []
        with torch.cuda.device(self.device):
            self._capture()

    def _eager(self, zero=True):
        if zero:
            self._drop_grads()
        F.WEIGHTS.clear()                               # the weight casts are part of every step (the update changes the weights)
        loss = self.step_fn(*self.inputs)
        if loss.dim() != 0:
            raise ValueError(f"GraphedTrainStep: step_fn must return a 0-dim loss, got {tuple(loss.shape)}")
        loss.backward()
        return loss

    def _drop_grads(self):
        self.model.zero_grad(set_to_none=True)
        for group in self.optim.param_groups:
            for p in group["params"]:
                p.grad = None

    def _capture(self):
        optim, s = self.optim, self.stream
        self.graph = self.loss = self._table = None     # a graph being replaced is never replayed again
        self.grads, self._table_grads = [], []
        optim._check_lr()
        items = [(group, p) for group in optim.param_groups for p in group["params"] if p.requires_grad]
        # warm up ON THE CAPTURE STREAM, as GraphedStep does; the optimiser's launches too, over a table of their own
        _fresh_workspace(self.device, s)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(self.warmup):
                self._eager()
            missing = sum(p.grad is None for _, p in items)
            self._drop_grads()                          # so the captured backward ASSIGNS fresh gradient tensors
            if not missing:
                optim.warm_launches(self.device)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        if missing or not items:
            raise F.ops._lib.VitamdError(f"GraphedTrainStep: {missing} of the optimiser's {len(items)} parameters got no gradient from "
                                         "step_fn; the resident table needs one for every row (freeze or drop those parameters)")
        optim._build(items, bind=False)                 # moments (created here when missing) and device buffers: outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with quiet_collector(), torch.cuda.graph(graph, stream=s):
            loss = self._eager(zero=False).detach()     # detached for GraphedStep's reason
            optim._bind()                               # host work: the static gradients' addresses, known only now
            optim._enqueue(torch.cuda.current_stream().cuda_stream)
        optim._upload_table()                           # the capture ran nothing: the table reaches the device before the first replay
        self.graph, self.loss, self._table = graph, loss, optim._table
        self._ws = _ops._WORKSPACES.get((self.device, s.cuda_stream))        # kept alive: its address is in the graph
        self.grads = [p.grad for p in self.params]
        self._table_grads = [p.grad for _, p in items]
        self.captures += 1

    def _stale(self):
        optim, t = self.optim, self._table
        if self.graph is None or t is None or optim._table is not t or t.hypers != optim._hypers():
            return True
        now = []
        for (_, p), g in zip(t.items, self._table_grads):
            st = optim.state[p] if p in optim.state else {}
            now.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr() if "exp_avg" in st else 0,
                        st["exp_avg_sq"].data_ptr() if "exp_avg_sq" in st else 0))
        return now != t.ptrs

    def __call__(self, *inputs) -> torch.Tensor:
        if len(inputs) != len(self.inputs) or any(not isinstance(a, torch.Tensor) or a.shape != b.shape or a.dtype != b.dtype
                                                 for a, b in zip(inputs, self.inputs)):
            raise F.ops._lib.VitamdError("GraphedTrainStep was captured for inputs of "
                                         + ", ".join(f"{tuple(b.shape)} {b.dtype}" for b in self.inputs))
        with torch.cuda.device(self.device):
            self.optim._check_lr()
            if self._stale():
                self._capture()
            for dst, src in zip(self.inputs, inputs):
                dst.copy_(src, non_blocking=True)
            self.graph.replay()
        self.optim._advance_mirrors()                   # step counts, schedule position and group["lr"]: no device read
        F.WEIGHTS.clear()                               # host-side cache state: whatever eager call comes next must re-cast
        for p, g in zip(self.params, self.grads):
            p.grad = g
        return self.loss


class GraphedDecoder:
    """One captured call of decode.forward_cached(x_static, cache), its length advance included, on a single stream (no fork or join).

        dec = model.graphed_decoder(batch, max_len)     # model: a causal transformer.Transformer
        h = dec.prefill(x_prompt)                       # eager, into the decoder's own cache
        h = dec.step(x_t)                               # [B, 1, D] -> the static output [B, 1, D]: read it before the next step

    Two optional stages are recorded in the same graph.  embed=(tok_table, pos_table) (fp32 parameters): x_static is computed by
    ops.decode_embed from the static token buffer `tokens` (int64 [B]) at the cache's device length, before the stack.  head=callable
    ([B, D] hidden states -> fp32 logits [B, V]): after the stack the logits are picked - torch.argmax, or `sampler` (a
    vitamd.sampling.Sampler, whose device counter add is then part of the capture) - and the pick is written back into `tokens`, so
    step() after step() generates.  head_weights: the fp32 parameters `head` reads (matrices through functions.WEIGHTS, biases directly).

    The graph bakes in addresses: the cache, the static buffers, the capture stream's workspace, the bf16 weight copies of
    functions.WEIGHTS (kept across refreshes) and the fp32 biases / tables.  begin() - called before every generation - refreshes the
    weight copies eagerly and compares every such address with the captured ones; when one moved it captures again (`captures`
    counts), so a stale graph is never replayed."""

    def __init__(self, model, batch, max_len=None, *, embed=None, head=None, sampler=None, head_weights=(), warmup=2):
        _decode.check_decodable(model)
        self.model, self.batch, self.head, self.sampler = model, int(batch), head, sampler
        self.embed = None if embed is None else tuple(embed)
        self.head_weights = list(head_weights)
        if sampler is not None and head is None:
            raise ValueError("GraphedDecoder: a sampler needs a head (logits to draw from)")
        self.cache = _decode.new_cache(model, batch, max_len)
        device, D = self.cache.device, model.n_embd
        if self.embed is not None:
            tok, pos = self.embed
            if pos.shape[0] < self.cache.max_len:
                raise ValueError(f"GraphedDecoder: the position table holds {pos.shape[0]} rows, the cache {self.cache.max_len}")
            if tok.shape[1] != D or pos.shape[1] != D:
                raise ValueError(f"GraphedDecoder: the embedding tables must be [rows, {D}]")
        self.x = torch.zeros((batch, 1, D), dtype=torch.float32, device=device)
        self.tokens = torch.zeros((batch,), dtype=torch.int64, device=device)
        self.stream = torch.cuda.Stream(device=device)
        self.warmup = max(1, int(warmup))
        self.graph, self.out, self.captures, self._baked, self._ws = None, None, 0, None, None
        with torch.cuda.device(device):
            self._capture()

    # ---- what the capture records
    def _body(self):
        with torch.no_grad():
            if self.embed is not None:
                _ops.decode_embed(self.embed[0].detach(), self.embed[1].detach(), self.tokens, self.cache.len_dev, out=self.x.view(self.batch, -1))
            h = _decode.forward_cached(self.model, self.x, self.cache)
            if self.head is not None:
                logits = self.head(h[:, 0])
                nxt = torch.argmax(logits, dim=-1) if self.sampler is None else self.sampler(logits)
                self.tokens.copy_(nxt.view(self.batch))
        return h

    def _weights(self):
        return [p[j] for layer in self.model.layers for p in (layer._params(),) for j in (0, 2, 4)]

    def _refresh(self):
        """bf16 weight copies made fresh eagerly (inside the capture WEIGHTS.prepare / get are then no-ops) -> every baked address"""
        F.WEIGHTS.prepare(self._weights(), False)
        ptrs = [F.WEIGHTS.get(w, False)[0].data_ptr() for w in self._weights() + [w for w in self.head_weights if w.dim() >= 2]]
        ptrs += [t.data_ptr() for layer in self.model.layers for t in layer._params()]
        ptrs += [t.data_ptr() for t in self.head_weights]
        if self.embed is not None:
            ptrs += [t.data_ptr() for t in self.embed]
        return tuple(ptrs)

    def _capture(self):
        cache, sampler, s = self.cache, self.sampler, self.stream
        self.graph = self.out = None                    # a graph being replaced is never replayed again
        self.reset()
        baked = self._refresh()
        # warm up ON THE CAPTURE STREAM (as GraphedStep does): vitamd_init, code-object loading, the first hipFuncSetAttribute of each skinny GEMM form, the
        # allocator and that stream's split-K / attention workspace all happen here, none of them inside the capture
        _fresh_workspace(cache.device, s)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _ops.init(cache.device)
            for _ in range(min(self.warmup, cache.max_len)):
                self._body()
            self.reset()                                # length and sampler position back; stale K/V rows past the length are harmless
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._ws = _ops._WORKSPACES.get((cache.device, s.cuda_stream))      # kept alive: its address is in the graph
        graph = torch.cuda.CUDAGraph()
        with quiet_collector(), torch.cuda.graph(graph, stream=s):
            out = self._body()
        # the capture ran nothing on the device, but the host mirrors moved
        cache.len = 0
        if sampler is not None:
            sampler.step = 0
        if self._refresh() != baked:
            raise F.ops._lib.VitamdError("GraphedDecoder: an operand moved during the capture")
        self.graph, self.out, self._baked = graph, out, baked
        self.captures += 1

    # ---- interface
    def begin(self):
        """Before every generation (prefill() calls it on an empty cache): fresh weight copies, a graph that matches them (captured again when an operand moved), an empty cache and
        the sampler at position 0."""
        with torch.cuda.device(self.cache.device):
            if self.graph is None or self._refresh() != self._baked:
                self._capture()
            self.reset()
        return self

    def reset(self):
        """Empty cache, sampler at position 0: device fills only."""
        self.cache.reset()
        if self.sampler is not None:
            self.sampler.reset(0)

    def prefill(self, x):
        """x [B, T, D]: the prompt's positions, run eagerly (the full causal path) into the decoder's cache -> hidden states [B, T, D]"""
        if self.cache.len == 0:                         # the start of a generation: the graph must match the operands it is about to meet
            self.begin()
        return _decode.forward_cached(self.model, x, self.cache)

    def step(self, x=None):
        """One replay: position cache.len.  x [B, 1, D] is copied into the static input (leave it out with an embed stage: the input then
        comes from `tokens`).  -> the static hidden states [B, 1, D], overwritten by the next step."""
        if self.cache.len + 1 > self.cache.max_len:
            raise ValueError(f"GraphedDecoder.step: {self.cache.len} cached + 1 new position exceed the cache length {self.cache.max_len}")
        if self.graph is None:
            raise F.ops._lib.VitamdError("GraphedDecoder.step: no captured graph (a capture failed); call begin()")
        if x is not None:
            if self.embed is not None:
                raise ValueError("GraphedDecoder.step: this decoder embeds its own token buffer; write `tokens` instead of passing x")
            if tuple(x.shape) != tuple(self.x.shape) or not x.is_cuda:
                raise F.ops._lib.VitamdError(f"GraphedDecoder was captured for a device input of {tuple(self.x.shape)}, got {tuple(x.shape)}")
            self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        self.cache.len += 1
        if self.sampler is not None:
            self.sampler.step += 1
        return self.out
