"""The training route of the code-id TiTok (train_llamagen_titok.TiTok.loss: vitamd.lm.prefixed_token_embed / prefixed_rows,
csrc/assemble.hip, and the head fused with the cross-entropy) against the present route (torch embedding / add / cat, linear / add / cat,
functions.linear + lm.cross_entropy), at the reference's defaults (16 384 VQ codes, 256 VQ tokens, 256 latents, 16 384 codes x 12,
preset S, batch 32) and at one larger shape (1 024 VQ tokens).  Device-event timings, warmed, the two routes alternated in one process,
median of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before anything is
timed each pair of routes must agree: the assembled sequences bit for bit, the losses and the latent ids as bench_tokenizer_loss asks.

  enc_assembly - the encoder's input sequence, forward + backward alone: embedding + add + expand + cat against prefixed_token_embed
  dec_assembly - the decoder's, given the projected latents: add + expand + cat against prefixed_rows
  head         - output head + cross-entropy, forward + backward alone: functions.linear + lm.cross_entropy against lm.linear_cross_entropy
  step         - whole forward + backward of the model: model(ids) + lm.cross_entropy against model.loss(ids)
  launches     - what the host issues per call on each route (C-ABI calls plus torch device ops), counted, not timed
  kernels      - device time of the four assembly kernels alone (20 launches replayed from a graph: the host's launch cost, which bounds
                 the two assembly stages above at these shapes, stays outside) with the bytes they move, in both geometries
usage: bench_code_titok.py [--rounds N] [--reps N] [--skip-step] [--only-kernels] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lm_loss import _ab, _count  # noqa: E402  (the same timing and counting)
from bench_tokenizer_loss import _verdict  # noqa: E402  (medians apart only when the ranges [min, max] do not overlap)

VQ_CODES, LATENTS, CODES, DIM, PRESET, BATCH = 16384, 256, 16384, 12, "S", 32
SHAPES = {"default_256": 256, "large_1024": 1024}          # name -> vq_latent_tokens


def _agree(a, b, what, tol=2e-3):
    a, b = float(a), float(b)
    if not abs(a - b) <= tol * max(1.0, abs(b)):
        raise SystemExit(f"bench_code_titok: the two routes disagree on the {what}: {a} vs {b}")
    return {"present": round(b, 6), "new": round(a, 6)}


def _ids_agree(a, b, what):
    frac = float((a == b).float().mean())
    if frac < 0.999:
        raise SystemExit(f"bench_code_titok: the two routes disagree on the {what} ids: {frac:.5f} equal")
    return round(frac, 6)


def assembly_bytes(B, E, S, D, gather):
    """HBM bytes of one forward + backward of a sequence assembly, counted from shapes (tables left out: they are small or cached)"""
    x, body = 4 * B * (E + S) * D, 4 * B * S * D
    present = {"gather or projected rows + pos (read, write)": 2 * body, "cat (read body, write x)": body + x,
               "backward: slices of g (read, write)": 2 * x, "sum over the batch of the prefix slice": 4 * B * E * D,
               "sum over the batch of the body slice": body, "embedding backward (read)": body if gather else 0}
    new = {"forward (read rows, write x)": body + x, "backward (read g once)": x, "atomics into the token table": body if gather else 0}
    return {"present": sum(present.values()), "new": sum(new.values())}


def kernel_times(B, E, S, D, rows, rounds, calls=20):
    """Device time of the four assembly kernels alone at one shape: `calls` launches of one kernel recorded into a graph (the entry points
    only enqueue), replayed `rounds` times; the host's launch cost, which bounds the autograd-level stages, is outside the measurement.
    -> {kernel: {us: median per launch, min_us, max_us, GB_per_s: bytes moved (from shapes) / median}}"""
    import statistics
    from vitamd import ops
    dev = torch.device("cuda")
    prefix, pos, tok = torch.randn(E, D, device=dev), torch.randn(S, D, device=dev), torch.randn(rows, D, device=dev)
    body, g = torch.randn(B, S, D, device=dev), torch.randn(B, E + S, D, device=dev)
    ids = torch.randint(0, rows, (B, S), device=dev)
    x, dprefix, dpos, dtok = torch.empty_like(g), torch.zeros_like(prefix), torch.zeros_like(pos), torch.zeros_like(tok)
    xb, bb = 4 * B * (E + S) * D, 4 * B * S * D
    kernels = {"fwd_gather": (lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids, tok_table=tok, out=x), bb + xb),
               "fwd_dense": (lambda: ops.assemble_tokens_fwd(prefix, pos, body=body, out=x), bb + xb),
               "bwd_gather": (lambda: ops.assemble_tokens_bwd(g, dprefix, dpos, ids=ids, dtok=dtok), xb + bb),      # g read + the atomics' payload
               "bwd_dense": (lambda: ops.assemble_tokens_bwd(g, dprefix, dpos), xb)}
    out = {}
    for name, (fn, nbytes) in kernels.items():
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        t = []
        for _ in range(rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            graph.replay()
            e.record()
            e.synchronize()
            t.append(s.elapsed_time(e) * 1e3 / calls)
        med = statistics.median(t)
        out[name] = {"us": round(med, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "MB": round(nbytes / 1e6, 1),
                     "GB_per_s": round(nbytes / med / 1e3, 1)}
        del graph
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--only-kernels", action="store_true", help="the device times of the assembly kernels alone, nothing else")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_code_titok: at least 5 rounds")
    import train_llamagen_titok as T
    from vitamd import lm
    from vitamd.functions import WEIGHTS, linear
    dev = torch.device("cuda")
    out = {"rounds": args.rounds, "reps": args.reps, "batch": BATCH}

    for name, vq_tokens in SHAPES.items():
        torch.manual_seed(0)
        model = T.TiTok(T.TiTokConfig(VQ_CODES, vq_tokens, LATENTS, CODES, DIM, PRESET)).to(dev)
        D = model.config.n_embd
        ids = torch.randint(0, VQ_CODES, (BATCH, vq_tokens), generator=torch.Generator().manual_seed(1)).to(dev)
        res = out[name] = {"vq_latent_tokens": vq_tokens, "latent_tokens": LATENTS, "n_embd": D}

        def record(key, run, extra=None):
            r = dict(extra or {})
            r.update(_ab({"present": lambda: run("present"), "new": lambda: run("new")}, args.rounds, args.reps))
            r["launches"] = {"present": _count(lambda: run("present")), "new": _count(lambda: run("new"))}
            r["verdict"] = _verdict(r)
            res[key] = r

        # ---- (0) the assembly kernels alone, device time: the encoder's geometry (gather) and the decoder's (dense)
        res["kernels_enc_geometry"] = kernel_times(BATCH, LATENTS, vq_tokens, D, VQ_CODES, args.rounds)
        res["kernels_dec_geometry"] = kernel_times(BATCH, vq_tokens, LATENTS, D, VQ_CODES, args.rounds)
        if args.only_kernels:
            continue

        # ---- (a) the encoder's sequence: E = latent rows in front of S = vq_tokens embedded ids
        dy = torch.randn(BATCH, LATENTS + vq_tokens, D, device=dev)

        def enc(route):
            model.zero_grad(set_to_none=True)
            x = model.enc.tokens(ids, fused=route == "new")
            x.backward(dy)
            return x.detach()

        if not torch.equal(enc("new"), enc("present")):
            raise SystemExit(f"bench_code_titok: {name}: the two routes disagree on the encoder's sequence")
        record("enc_assembly", enc, {"B_E_S_D": [BATCH, LATENTS, vq_tokens, D], "bytes": assembly_bytes(BATCH, LATENTS, vq_tokens, D, True)})

        # ---- (b) the decoder's sequence: E = vq_tokens mask rows in front of S = latent rows, given the projected latents
        body = torch.randn(BATCH, LATENTS, D, device=dev, requires_grad=True)
        dy2 = torch.randn(BATCH, vq_tokens + LATENTS, D, device=dev)

        def dec(route):
            model.zero_grad(set_to_none=True)
            body.grad = None
            if route == "new":
                x = lm.prefixed_rows(body, model.dec.pos_emb, model.dec.mask_tokens.weight)
            else:
                x = torch.cat([model.dec.mask_tokens.weight.unsqueeze(0).expand(BATCH, -1, -1), body + model.dec.pos_emb[:LATENTS]], dim=1)
            x.backward(dy2)
            return x.detach()

        if not torch.equal(dec("new"), dec("present")):
            raise SystemExit(f"bench_code_titok: {name}: the two routes disagree on the decoder's sequence")
        record("dec_assembly", dec, {"B_E_S_D": [BATCH, vq_tokens, LATENTS, D], "bytes": assembly_bytes(BATCH, vq_tokens, LATENTS, D, False)})
        del dy, dy2, body

        # ---- (c) head + cross-entropy
        h = torch.randn(BATCH, vq_tokens, D, device=dev, requires_grad=True)
        proj, target = model.dec.emb_proj, ids.reshape(-1)

        def head(route):
            h.grad = None
            model.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            if route == "new":
                loss = lm.linear_cross_entropy(h, proj.weight, proj.bias, target)
            else:
                loss = lm.cross_entropy(linear(h, proj.weight, proj.bias).reshape(-1, VQ_CODES), target)
            loss.backward()
            return loss.detach()

        record("head", head, {"rows": BATCH * vq_tokens, "V": VQ_CODES, "loss_check": _agree(head("new"), head("present"), f"{name} head loss")})
        del h

        # ---- (d) whole forward + backward
        if not args.skip_step:
            def step(route):
                model.zero_grad(set_to_none=True)
                WEIGHTS.clear()
                if route == "new":
                    rl, ql, latent_ids = model.loss(ids)
                else:
                    logits, latent_ids, ql = model(ids)
                    rl = lm.cross_entropy(logits.reshape(-1, VQ_CODES), target)
                loss = rl + ql
                loss.backward()
                return latent_ids, loss.detach()

            (i1, l1), (i0, l0) = step("new"), step("present")
            record("step", step, {"loss_check": _agree(l1, l0, f"{name} step loss"), "ids_equal": _ids_agree(i1, i0, f"{name} step")})
            res["step"]["sequences_per_s"] = {k: round(BATCH / (res["step"][k]["median_ms"] * 1e-3), 1) for k in ("present", "new")}
        del model, ids
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
