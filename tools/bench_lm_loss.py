"""The training route of the causal stack (vitamd/lm.py, csrc/loss.hip) against the present route, at the reference's training shape
(train_videogpt.py:73-79: batch 32, 16 frames x 64 tokens, codebook 1024, preset B: M = 32 768 rows, D = 768, V = 1024).  Device-event
timings, warmed, the two routes alternated in one process, median of --rounds rounds with the spread (min .. max); prints one JSON line.
Before anything is timed each pair of routes must agree on the loss.

  head       - head + loss, forward + backward alone: functions.linear + F.cross_entropy against lm.linear_cross_entropy
  embed      - embedding forward + backward alone: the two torch gathers and their backward against lm.token_embed
  step       - a whole VideoGPT-B forward + backward: model(x)[1].backward() against model.loss(x).backward()
  bytes      - each route's HBM bytes around the head and the loss, counted from shapes (the GEMMs' own operands left out on both sides)
  launches   - what the host issues per step on each route: C-ABI calls of the library plus torch device ops (views and allocations
               left out), counted, not timed
usage: bench_lm_loss.py [--rounds N] [--reps N] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))

B, FRAMES, FRAME, CODES, PRESET = 32, 16, 64, 1024, "B"

_NO_LAUNCH = {"view", "_unsafe_view", "select", "slice", "reshape", "_reshape_alias", "unsqueeze", "squeeze", "expand", "permute", "transpose", "t",
              "detach", "alias", "as_strided", "empty", "empty_like", "empty_strided", "new_empty", "lift_fresh", "unbind", "split", "narrow"}


class _HostCalls:
    """Counts what the host issues inside a `with`: C-ABI calls of libvitamd and torch device ops (views and allocations left out)."""

    def __init__(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        from vitamd import lib
        self.n, self.lib = 0, lib.load()
        outer = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                if func.overloadpacket.__name__ not in _NO_LAUNCH:
                    outer.n += 1
                return func(*args, **(kwargs or {}))

        self.mode = Mode()

    def __enter__(self):
        from vitamd import lib
        self.saved = {}
        for name in lib.SIGNATURES:
            if name.endswith("_bytes") or name in ("vitamd_abi_version", "vitamd_init", "vitamd_gemm_nt_plan", "vitamd_attention_keep_forms", "vitamd_attention_form"):
                continue
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def counted(*a, _fn=fn):
                self.n += 1
                return _fn(*a)

            setattr(self.lib, name, counted)
        self.mode.__enter__()
        return self

    def __exit__(self, *exc):
        self.mode.__exit__(*exc)
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def _timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def _ab(routes, rounds, reps):
    """routes: {name: callable}; warmed, then alternated round by round -> {name: {median_ms, min_ms, max_ms}}"""
    for fn in routes.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(_timed(fn, reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def _count(fn):
    fn()
    torch.cuda.synchronize()
    with _HostCalls() as c:
        fn()
    torch.cuda.synchronize()
    return c.n


def _agree(a, b, what, tol=2e-3):
    a, b = float(a), float(b)
    if not abs(a - b) <= tol * max(1.0, abs(b)):
        raise SystemExit(f"bench_lm_loss: the two routes disagree on the {what}: {a} vs {b}")
    return {"present": round(b, 6), "new": round(a, 6)}


def head_bytes(M, V):
    """HBM bytes around the two head GEMMs, from shapes (logits / gradient traffic only; GEMM operands are the same on both routes)"""
    bf, f32 = 2 * M * V, 4 * M * V
    present = {"upcast (read bf16, write fp32)": bf + f32, "log_softmax (read, write fp32)": 2 * f32, "nll backward (write fp32)": f32,
               "softmax backward (read 2, write 1 fp32)": 3 * f32, "pad: zero fill": f32, "pad: copy (read, write fp32)": 2 * f32,
               "cast (read fp32, write bf16)": f32 + bf}
    new = {"loss forward (read bf16)": bf, "loss backward (read bf16, write bf16 in place)": 2 * bf}
    return {"present": sum(present.values()), "new": sum(new.values()), "present_parts": present, "new_parts": new}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_lm_loss: at least 5 rounds")
    import train_videogpt as V
    from vitamd import lm
    from vitamd.functions import WEIGHTS, linear
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cfg = V.VideoGPTConfig(FRAME, CODES, PRESET, FRAMES, 0.0)
    D, M = cfg.n_embd, B * FRAMES * FRAME
    out = {"shape": {"M": M, "D": D, "V": CODES, "batch": B, "tokens": FRAMES * FRAME}, "rounds": args.rounds, "reps": args.reps}

    # ---- (a) head + loss
    h = torch.randn(M, D, device=dev, requires_grad=True)
    w = (torch.randn(CODES, D, device=dev) * 0.02).requires_grad_(True)
    b = torch.zeros(CODES, device=dev, requires_grad=True)
    y = torch.randint(0, CODES, (M,), device=dev)

    def head_present():
        for t in (h, w, b):
            t.grad = None
        WEIGHTS.clear()
        loss = F.cross_entropy(linear(h, w, b), y)
        loss.backward()
        return loss

    def head_new():
        for t in (h, w, b):
            t.grad = None
        WEIGHTS.clear()
        loss = lm.linear_cross_entropy(h, w, b, y)
        loss.backward()
        return loss

    out["head_loss_check"] = _agree(head_new().detach(), head_present().detach(), "head loss")
    out["head"] = _ab({"present": head_present, "new": head_new}, args.rounds, args.reps)
    out["head_launches"] = {"present": _count(head_present), "new": _count(head_new)}
    out["head_bytes"] = head_bytes(M, CODES)

    # ---- (b) embedding
    tok = torch.randn(CODES + 1, D, device=dev, requires_grad=True)
    pos = torch.randn(FRAMES * FRAME, D, device=dev, requires_grad=True)
    ids = torch.randint(0, CODES + 1, (B, FRAMES * FRAME), device=dev)
    dy = torch.randn(B, FRAMES * FRAME, D, device=dev)
    ar = torch.arange(FRAMES * FRAME, device=dev)

    def embed_present():
        tok.grad = pos.grad = None
        x = F.embedding(ids, tok) + F.embedding(ar, pos)
        x.backward(dy)
        return x

    def embed_new():
        tok.grad = pos.grad = None
        x = lm.token_embed(ids, tok, pos)
        x.backward(dy)
        return x

    if not torch.equal(embed_new().detach(), embed_present().detach()):
        raise SystemExit("bench_lm_loss: the two embedding routes disagree")
    out["embed"] = _ab({"present": embed_present, "new": embed_new}, args.rounds, args.reps)
    out["embed_launches"] = {"present": _count(embed_present), "new": _count(embed_new)}
    act = 4 * M * D
    out["embed_bytes"] = {"present": "gather + gather + add forward (~3 x activation); sort-based embedding backward (not countable from shapes)",
                          "new_forward": 2 * act + 4 * FRAMES * FRAME * D, "new_backward": act + act + 4 * FRAMES * FRAME * D,
                          "activation": act}
    del h, w, b, y, tok, pos, ids, dy

    # ---- (c) the whole step
    if not args.skip_step:
        model = V.VideoGPT(cfg).to(dev)
        x = torch.randint(0, CODES, (B, FRAMES, FRAME), device=dev)

        def step_present():
            model.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            loss = model(x)[1]
            loss.backward()
            return loss

        def step_new():
            model.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            loss = model.loss(x)
            loss.backward()
            return loss

        out["step_loss_check"] = _agree(step_new().detach(), step_present().detach(), "step loss")
        out["step"] = _ab({"present": step_present, "new": step_new}, args.rounds, max(1, args.reps // 2))
        out["step_launches"] = {"present": _count(step_present), "new": _count(step_new)}
        out["step_tokens_per_s"] = {k: round(M / (v["median_ms"] * 1e-3)) for k, v in out["step"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
