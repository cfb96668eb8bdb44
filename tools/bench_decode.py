"""KV-cached generation against the uncached loop, in the reference's generate_frames setup (train_videogpt.py:69-76,140: preset B,
64 tokens per frame, 1024 codes, 16 frames, 8 conditioning frames, batch 32): prints one JSON line.

  cached      - one whole VideoGPT.generate_frames call (prefill of 513 positions + 511 decode steps), ms per generated token and tokens/s
  sampled     - the same call with temperature=1.0, top_k=100, top_p=0.95 (one sampling kernel + one counter add per token in place of the
                argmax), timed in rounds interleaved with the greedy ones
  graph       - the same two calls with graph=True (vitamd.graph.GraphedDecoder: every token after the first is one graph launch plus one
                copy of the picked tokens), greedy and sampled, in the same interleaved rounds; min / median / max over the reps and the
                launches per token of each path (counted, not timed: every C-ABI call and every torch device op of one decode step)
  uncached    - the reference's loop (the whole prefix through the stack per token, on the HIP stack), timed for single steps at prefix
                lengths spread over the run (513 .. 1024) and averaged: ms per generated token
  kernels     - hipEvent time of each decode kernel at the shapes of one decode step, against its HBM byte floor (skinny GEMMs: the weight
                bytes; decode attention: the K/V bytes at the current length; K/V append: the bytes it moves) at HBM_TBPS
usage: bench_decode.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))

HBM_TBPS = 8.0        # MI355X HBM3E peak (spec); bench.py's roofline block is bound by the MFMA rate and carries no HBM figure of its own
B, FRAME, CODES, FRAMES, COND = 32, 64, 1024, 16, 8


def _events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


_NO_LAUNCH = {"view", "_unsafe_view", "select", "slice", "reshape", "_reshape_alias", "unsqueeze", "squeeze", "expand", "permute", "transpose", "t",
              "detach", "alias", "as_strided", "empty", "empty_like", "empty_strided", "new_empty", "lift_fresh", "unbind", "split", "narrow"}


class _HostCalls:
    """Counts what the host issues inside a `with`: C-ABI calls of libvitamd (one or two kernels each: a split-K GEMM or a split attention
    has a second, reducing launch), torch device ops (views and allocations left out) and graph replays."""

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
            fn = getattr(self.lib, name)
            if name.endswith("_bytes") or name in ("vitamd_abi_version", "vitamd_gemm_nt_plan", "vitamd_attention_keep_forms", "vitamd_attention_form"):
                continue
            self.saved[name] = fn

            def counted(*a, _fn=fn):
                self.n += 1
                return _fn(*a)
            setattr(self.lib, name, counted)
        self.replay = torch.cuda.CUDAGraph.replay

        def replay(g):
            self.n += 1
            return self.replay(g)
        torch.cuda.CUDAGraph.replay = replay
        self.mode.__enter__()
        return self

    def __exit__(self, *exc):
        self.mode.__exit__(*exc)
        torch.cuda.CUDAGraph.replay = self.replay
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def _host_calls(fn):
    with _HostCalls() as c:
        fn()
        torch.cuda.synchronize()
    return c.n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import train_videogpt as V
    from vitamd import ops
    from vitamd.functions import WEIGHTS
    assert torch.cuda.is_available(), "bench_decode.py needs a GPU"
    torch.manual_seed(0)
    cfg = V.VideoGPTConfig(FRAME, CODES, "B", FRAMES, 0.0)
    model = V.VideoGPT(cfg).cuda().eval()
    video = torch.randint(0, CODES, (B, COND, FRAME), device="cuda")
    n_gen = (FRAMES - COND) * FRAME
    S0 = COND * FRAME

    # ---- cached: whole generate_frames calls
    out = model.generate_frames(video, n=FRAMES - COND)            # warm-up (code objects, allocator, weight cache)
    torch.cuda.synchronize()
    SAMPLING = dict(temperature=1.0, top_k=100, top_p=0.95)
    model.generate_frames(video, n=FRAMES - COND, seed=0, **SAMPLING)
    torch.cuda.synchronize()
    out_g = model.generate_frames(video, n=FRAMES - COND, graph=True)      # the capture happens here, outside the timed rounds
    torch.cuda.synchronize()
    assert torch.equal(out_g, out), "graph=True must give the eager cached tokens"

    def timed(**kw):
        t0 = time.perf_counter()
        o = model.generate_frames(video, n=FRAMES - COND, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, o
    times, times_s, times_g, times_gs = [], [], [], []
    # Eager and graph rounds interleaved: one process, one clock state.  The model keeps ONE decoder, so alternating greedy and sampled
    # graph rounds would capture every time: the sampled graph rounds follow in a second loop, each beside an eager sampled round, with
    # one seed throughout (the seed is part of the decoder's key).
    for r in range(args.reps):
        t, out = timed()
        times.append(t)
        times_s.append(timed(seed=0, **SAMPLING)[0])
        times_g.append(timed(graph=True)[0])
    model.generate_frames(video, n=FRAMES - COND, graph=True, seed=0, **SAMPLING)      # capture of the sampled decoder, untimed
    torch.cuda.synchronize()
    for r in range(args.reps):
        times_s.append(timed(seed=0, **SAMPLING)[0])
        times_gs.append(timed(graph=True, seed=0, **SAMPLING)[0])
    med = lambda ts: sorted(ts)[len(ts) // 2]
    t_cached, t_sampled = med(times), med(times_s)
    cached_ms_tok = t_cached * 1e3 / n_gen
    sampled_ms_tok = t_sampled * 1e3 / n_gen

    def spread(ts):
        return {"ms_per_token": round(med(ts) * 1e3 / n_gen, 4), "min": round(min(ts) * 1e3 / n_gen, 4), "max": round(max(ts) * 1e3 / n_gen, 4),
                "reps": len(ts)}
    # launches per token: the host's calls of one whole generation minus those of the prefill and first pick, over the remaining tokens
    tokens0 = video.reshape(B, -1)
    first = _host_calls(lambda: model.generate(tokens0, n=1))
    first_s = _host_calls(lambda: model.generate(tokens0, n=1, seed=0, **SAMPLING))
    calls = {"eager_greedy": (_host_calls(lambda: model.generate_frames(video, n=FRAMES - COND)) - first) / (n_gen - 1),
             "eager_sampled": (_host_calls(lambda: model.generate_frames(video, n=FRAMES - COND, seed=0, **SAMPLING)) - first_s) / (n_gen - 1),
             "graph_sampled": (_host_calls(lambda: model.generate_frames(video, n=FRAMES - COND, graph=True, seed=0, **SAMPLING)) - first_s) / (n_gen - 1)}
    model.generate_frames(video, n=FRAMES - COND, graph=True)              # back to the greedy decoder (a capture, not counted)
    calls["graph_greedy"] = (_host_calls(lambda: model.generate_frames(video, n=FRAMES - COND, graph=True)) - first) / (n_gen - 1)
    graph = {"greedy": dict(spread(times_g), eager=spread(times), host_calls_per_token=round(calls["graph_greedy"], 2),
                            eager_host_calls_per_token=round(calls["eager_greedy"], 2),
                            eager_over_graph=round(med(times) / med(times_g), 3)),
             "sampled": dict(spread(times_gs), eager=spread(times_s), host_calls_per_token=round(calls["graph_sampled"], 2),
                             eager_host_calls_per_token=round(calls["eager_sampled"], 2),
                             eager_over_graph=round(med(times_s) / med(times_gs), 3))}

    # ---- uncached: single steps of the reference loop at prefix lengths spread over the run
    toks = out[:, : S0 + n_gen - 1]
    step_ms = {}
    for L in (S0 + 1, S0 + 129, S0 + 257, S0 + 385, S0 + n_gen):      # sequence length fed to the stack (SOS + prefix)
        prefix = toks[:, : L - 1]

        def step():
            with torch.no_grad():
                h = model.transformer(model._embed(torch.cat([model._sos(B, prefix.device), prefix], dim=-1)))
                return torch.argmax(model._head(h[:, -1]), dim=-1)
        step_ms[L] = round(_events_ms(step, 2), 3)
    uncached_ms_tok = sum(step_ms.values()) / len(step_ms)

    # ---- per kernel, at one decode step's shapes
    D, H = cfg.n_embd, cfg.trans_config.n_heads
    layer = model.transformer.layers[0]
    wq, w1, w2 = (WEIGHTS.get(w, False)[0] for w in (layer.multi_attn.qkv.weight, layer.mlp[0].weight, layer.mlp[2].weight))
    wp = WEIGHTS.get(model.proj.weight, False)[0]
    a768, a3072 = torch.randn(B, D, device="cuda").to(torch.bfloat16), torch.randn(B, 4 * D, device="cuda").to(torch.bfloat16)
    resid = torch.randn(B, D, device="cuda")
    bq, b1, b2, bp = (t.detach().float().contiguous() for t in (layer.multi_attn.qkv.bias, layer.mlp[0].bias, layer.mlp[2].bias, model.proj.bias))
    kern = {}

    def rec(name, fn, nbytes, reps=50):
        ms = _events_ms(fn, reps)
        floor_us = nbytes / (HBM_TBPS * 1e12) * 1e6
        kern[name] = {"us": round(ms * 1e3, 2), "floor_us": round(floor_us, 2), "of_floor": round(floor_us / (ms * 1e3), 3), "bytes": int(nbytes)}

    rec("skinny_qkv[32x2304x768]", lambda: ops.gemm_skinny(a768, wq, ops.EPI_BIAS_BF16, bias=bq), wq.numel() * 2)
    rec("skinny_fc1_gelu[32x3072x768]", lambda: ops.gemm_skinny(a768, w1, ops.EPI_GELU, bias=b1), w1.numel() * 2)
    rec("skinny_fc2_resid[32x768x3072]", lambda: ops.gemm_skinny(a3072, w2, ops.EPI_RESID_F32, bias=b2, aux=resid), w2.numel() * 2)
    rec("skinny_head_f32[32x1024x768]", lambda: ops.gemm_skinny(a768, wp, ops.EPI_F32, bias=bp), wp.numel() * 2)
    Lmax = cfg.max_tokens
    kc = torch.randn(B, H, Lmax, 64, device="cuda").to(torch.bfloat16)
    vc = torch.randn(B, H, Lmax, 64, device="cuda").to(torch.bfloat16)
    qkv = torch.randn(B, 3 * D, device="cuda").to(torch.bfloat16)
    for n in (S0 + 1, S0 + 256, Lmax):
        length = torch.tensor([n - 1], dtype=torch.int32, device="cuda")
        rec(f"decode_attention[len={n}]", lambda: ops.decode_attention(qkv, kc, vc, length, B, H), 2 * B * H * n * 64 * 2)
    length = torch.tensor([S0], dtype=torch.int32, device="cuda")
    rec("kv_append[T=1]", lambda: ops.kv_append(qkv, kc, vc, length, B, 1, H), 2 * 2 * B * D * 2)

    for V in (1024, 16384):
        lg = torch.randn(B, V, device="cuda") * 3
        rec(f"sample_logits[{B}x{V}]", lambda: ops.sample_logits(lg, **SAMPLING), B * V * 4)
    lg = torch.randn(B, CODES, device="cuda") * 3
    kern["argmax[32x1024]"] = {"us": round(_events_ms(lambda: torch.argmax(lg, dim=-1, keepdim=True), 50) * 1e3, 2)}      # what greedy launches instead

    print(json.dumps({
        "config": {"preset": "B", "frame_size": FRAME, "codebook": CODES, "max_frames": FRAMES, "condition_frames": COND, "batch": B,
                   "generated_tokens_per_sequence": n_gen},
        "cached": {"generate_frames_s": round(t_cached, 4), "ms_per_token": round(cached_ms_tok, 4),
                   "tokens_per_s": round(B * n_gen / t_cached, 1)},
        "sampled": dict(SAMPLING, generate_frames_s=round(t_sampled, 4), ms_per_token=round(sampled_ms_tok, 4),
                        tokens_per_s=round(B * n_gen / t_sampled, 1), over_cached=round(sampled_ms_tok / cached_ms_tok, 4)),
        "graph": graph,
        "uncached": {"ms_per_token": round(uncached_ms_tok, 3), "step_ms_by_length": step_ms,
                     "generate_frames_s_estimate": round(uncached_ms_tok * n_gen / 1e3, 3)},
        "speedup": round(uncached_ms_tok / cached_ms_tok, 2),
        "hbm_tbps": HBM_TBPS, "kernels": kern,
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
