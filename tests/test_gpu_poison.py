"""Every route of the package, clean against poisoned (tests/_poison.py).

Each workload returns a dict of CPU tensors (loss, outputs, every gradient; after training steps every parameter and optimiser state) and
is run three times in one process: clean, clean again, and inside `poisoned(log)` with `dirty_scratch()` just before (and between the
two iterations of a training workload), so every buffer the wrappers of vitamd/*.py leave uninitialised, and every long-lived scratch
they reuse, holds 0xFF bytes.  Asserted per workload:

  - the two clean runs agree bit for bit in every key listed as exact (a broken reproducibility claim is reported as such, apart from
    the poison result);
  - compare(clean, poisoned, exact) is empty: exact keys have equal bits, every other key is finite wherever the clean run is;
  - the log is not empty.

`exact` holds every key except those that include/vitamd.h documents as depending on the arrival order of fp32 atomics - the header's
sentence is quoted beside each exclusion in ATOMIC_* below - and, in a training workload, everything computed after the first optimiser
step of a model that has such a gradient (the parameters of iteration 2 are functions of it).  Where the route's own test holds such a
gradient to a bound against a reference fixture, the poisoned run's gradient is held to the same bound (imported, not restated).

The last test of the file compares the union of the call sites all workloads logged with empty_sites(): every `torch.empty` of the
package is exercised, except the NOT_REACHED list.
"""
import functools
import re
import time
import types

import pytest
import torch

import _poison as P
import weights as W
from conftest import load_golden

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
UNION = []          # the log entries of every poisoned run of the session (the coverage test reads it)
STATS = {}          # workload -> (poisoned allocations, distinct sites, seconds)

# ------------------------------------------------------------------------------------------------ what the header says about atomics
Q_EMBED_BWD = ("vitamd_embed_bwd: 'dpos, dextra and dbias are ACCUMULATED into (atomics): zero them for a fresh gradient.'")
Q_DTOK = ("vitamd_embed_tokens_bwd: 'dtok fp32 [tok_rows, D] += the g rows by fp32 atomics (order-dependent in the last bits, as "
          "vitamd_embed_bwd's outputs are)'")
Q_ASSEMBLE = ("vitamd_assemble_tokens_bwd: 'dtok fp32 [tok_rows, D] += g[b, E+t] at row ids[b*S+t] by fp32 atomics (order-dependent in the "
              "last bits)'")
Q_DCODEBOOK = ("vitamd_vq_quantize_bwd: 'dcodebook depends on arrival order in its last bits where a code is picked in more than one "
               "256-row block; dx never does.'")
Q_CONV3X3 = "vitamd_conv3x3_bwd: 'dw [Cout,Cin,3,3] (or null) and db [Cout] (or null) are ACCUMULATED into (atomics)'"
Q_AFFINE_LN = ("vitamd_layernorm_affine_bwd: 'dgamma, dbeta are ACCUMULATED into (zero them first); optional bf16 copy of g_out and its "
               "column sums as above.'")
Q_TN_ATOMIC = "vitamd_gemm_tn_bf16: 'Accumulates with fp32 atomics, so `out` must hold the running gradient'"
Q_ATTN_DBIAS = "ops.attention_bwd: 'the column sums of dqkv (QKV bias gradient) are added to `dbias` if given' (atomics, functions.py BIAS_QKV_FROM_WGRAD)"
Q_COLSUM = ("vitamd_colsum_bf16: 'out[n] += sum_m X[m,n]  (bias gradients).'; csrc/misc.hip colsum_bf16_kernel: 'the 8 row-groups of a block "
            "are combined through LDS, then one shaped atomic per column' (one block per 64 rows or more: order-dependent above 128 rows)")
Q_NT_COLSUM = ("functions.py BIAS_FROM_WGRAD: 'dgrad-fc2's epilogue (column sums, butterfly and one atomic per wave and tile)' - the "
               "colsum= of ops.gemm_nt(EPI_DMUL) that vitamd/block_functions.py still uses")


def _cpu(t):
    return t.detach().cpu().clone()


def _noop(*holders):
    return 0


def three_runs(name, workload, atomic=(), downstream=False):
    """workload(dirty) -> dict of CPU tensors; `dirty(*holders)` is what it calls before its work and between iterations (a no-op in the
    clean runs, dirty_scratch in the poisoned one).  atomic: (regex, header sentence) pairs of the keys left out of `exact`; downstream:
    the model has such a gradient, so keys outside 'it1/' (after the first optimiser step) are left out too.
    -> (clean, poisoned, exact); raises AssertionError on any of the three findings."""
    t0 = time.time()
    clean, again = workload(_noop), workload(_noop)
    log = []
    with P.poisoned(log):
        P.dirty_scratch()
        dirty = workload(P.dirty_scratch)
    torch.cuda.synchronize()
    UNION.extend(log)
    sites = {e[:2] for e in log}
    STATS[name] = (len(log), len(sites), time.time() - t0)
    patterns = [re.compile(rx) for rx, _ in atomic]
    exact = {k for k in clean if not any(p.search(k) for p in patterns) and not (downstream and not k.startswith("it1/"))}
    unrepro = P.compare(clean, again, exact)
    fails = P.compare(clean, dirty, exact)
    print(f"\n[{name}] {len(log)} poisoned allocations at {len(sites)} sites, {len(clean)} keys ({len(exact)} exact), {STATS[name][2]:.2f} s")
    loose = [k for k in clean if k not in exact and P.compare({k: clean[k]}, {k: again[k]}, {k})]
    print(f"[{name}] keys outside `exact` whose clean runs differ: {len(loose)} of {len(clean) - len(exact)}: "
          f"{sorted({re.sub(r'[0-9]+', 'N', k) for k in loose if not k.startswith(('it2/', 'final/'))})}")
    for f in unrepro:
        print(f"[{name}] CLEAN RUNS DIFFER {f}")
    for f in fails:
        print(f"[{name}] POISON {f}")
    assert not unrepro, f"{name}: two clean runs differ in keys documented as reproducible (not a poison finding): {unrepro[:6]}"
    assert not fails, f"{name}: the poisoned run differs: {fails[:6]}"
    assert log, f"{name}: nothing was poisoned"
    return clean, dirty, exact


def _train_two(model, step, optim, dirty, holders=()):
    """two iterations of step() -> loss; gradients of each iteration, then every parameter and optimiser state"""
    out = {}
    names = {id(p): k for k, p in model.named_parameters()}
    for it in (1, 2):
        dirty(optim, *holders)
        loss = step()
        out[f"it{it}/loss"] = _cpu(loss).reshape(1)
        for k, p in model.named_parameters():
            if p.grad is not None:
                out[f"it{it}/grad/{k}"] = _cpu(p.grad)
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        out[f"final/param/{k}"] = _cpu(p)
    for p, st in optim.state.items():
        for key, v in st.items():
            if isinstance(v, torch.Tensor):
                out[f"final/state/{names[id(p)]}/{key}"] = _cpu(v)
    return out


def _held_to(dirty, keys, err, bound):
    """the excluded gradients of the poisoned run against the route's own reference and bound"""
    bad, worst = [], (0.0, None)
    for key, ref_key in keys:
        e, b = err(dirty[key], ref_key), bound(ref_key)
        worst = max(worst, (e / b, key))
        if not e < b:
            bad.append((key, e, b))
    print(f"  {len(keys)} excluded gradients against their reference: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert keys and not bad, bad


# ------------------------------------------------------------------------------------------------ 1. the transformer stack
@pytest.mark.parametrize("mode", ["plain", "p_mlp", "keep"])
def test_stack_forward_backward(hip, mode):
    """test_gpu_tn_colsum._run_stack as it stands (2 layers, D = 256, H = 4, B = 3, N = 40, BIAS_FROM_WGRAD on): bit-reproducible in
    everything, so every key is exact"""
    from test_gpu_tn_colsum import _run_stack

    def workload(dirty):
        dirty()
        return _run_stack(True, mode, [])
    three_runs(f"stack-{mode}", workload)


def test_stack_causal_with_attention_dropout(hip):
    """the same stack with causal=True, attention dropout 0.1 and MLP dropout 0.1 (the masks come from torch's CPU generator, seeded)"""
    import transformer as T
    from vitamd.functions import TransformerStackFn
    L, D, H, B, N, seed = 2, 256, 4, 3, 40, 17

    def workload(dirty):
        dirty()
        m = T.Transformer(T.TransformerConfig(n_layers=L, n_heads=H, n_embd=D, block_size=N))
        m.load_state_dict(W.transformer_state(seed, "", L, D), strict=True)
        m = m.cuda()
        x = W.normal(seed, "x", (B, N, D)).cuda().requires_grad_(True)
        dy = W.normal(seed, "dy", (B, N, D)).cuda()
        params = [p for layer in m.layers for p in layer._params()]
        torch.manual_seed(1234)
        y = TransformerStackFn.apply(x, H, True, 0.1, 0.1, None, *params)
        (y * dy).sum().backward()
        torch.cuda.synchronize()
        return {"y": _cpu(y), "dx": _cpu(x.grad), **{k: _cpu(p.grad) for k, p in m.named_parameters()}}
    three_runs("stack-causal-dropout", workload)


def test_standalone_attention_and_layer_modules(hip):
    """transformer.Attention and TransformerLayer on their own (test_gpu_parity.test_standalone_attention_and_layer_modules' shapes): the
    fused-QKV AttentionFn, whose bias gradient is still attention_bwd's dbias"""
    import transformer as T

    def workload(dirty):
        dirty()
        cfg = T.TransformerConfig(n_layers=1, n_heads=2, n_embd=128, block_size=50)
        sd = W.transformer_state(5, "", 1, 128)
        layer = T.TransformerLayer(cfg)
        layer.load_state_dict({k[len("layers.0."):]: v for k, v in sd.items()})
        layer = layer.cuda()
        x = W.normal(5, "x", (2, 50, 128)).cuda().requires_grad_(True)
        dy = W.normal(5, "dy", (2, 50, 128)).cuda()
        y = layer(x)
        (y * dy).sum().backward()
        out = {"layer/y": _cpu(y), "layer/dx": _cpu(x.grad), **{f"layer/{k}": _cpu(p.grad) for k, p in layer.named_parameters()}}
        layer.zero_grad(set_to_none=True)
        xa = W.normal(5, "xa", (2, 50, 128)).cuda().requires_grad_(True)
        ya = layer.multi_attn(xa)
        (ya * dy).sum().backward()
        torch.cuda.synchronize()
        out.update({"attn/y": _cpu(ya), "attn/dx": _cpu(xa.grad)}, **{f"attn/{k}": _cpu(p.grad) for k, p in layer.multi_attn.named_parameters()})
        return out
    three_runs("standalone-attention", workload, [(r"^attn/qkv\.bias$", Q_ATTN_DBIAS)])


# ------------------------------------------------------------------------------------------------ 2. the ViT classifier
ATOMIC_VIT = [(r"grad/vit\.(pos_emb\.weight|extra_emb\.weight|patch_proj\.bias)$", Q_EMBED_BWD),
              (r"grad/head\.bias$", Q_COLSUM)]


def _classifier(g, **optim_kwargs):
    import train_vit as TV
    from vitamd.optim import AdamW
    c = g["cfg"]
    cfg = TV.ViTConfig(c["image_size"], 3, c["patch"], c["preset"], c["extra_tokens"], 0.0)
    m = TV.ViTClassifier(cfg, num_classes=c["num_classes"])
    m.load_state_dict(W.classifier_state(c["seed"], 3, c["patch"], c["n_patches"], c["extra_tokens"], c["n_layers"], c["n_embd"],
                                         c["num_classes"]), strict=True)
    m = m.cuda()
    return TV, m, AdamW(m.parameters(), lr=1e-3, weight_decay=0.05, **optim_kwargs)


def _classifier_workload(dirty, g=None):
    """the model, images and labels of test_gpu_parity._run_classifier (vit_s32.pt), two train_vit.train_step under vitamd.optim.AdamW"""
    g = load_golden("vit_s32.pt") if g is None else g
    c = g["cfg"]
    torch.manual_seed(7)
    dirty()
    TV, m, optim = _classifier(g)
    images = W.normal(c["seed"], "images", (c["batch"], 3, c["image_size"], c["image_size"])).cuda()
    labels = W.randint(c["seed"], "labels", (c["batch"],), c["num_classes"]).cuda()
    return _train_two(m, lambda: TV.train_step(m, images, labels, optim), optim, dirty)


def _classifier_bounds(dirty):
    from test_gpu_parity import _err, classifier_grad_bound
    g = load_golden("vit_s32.pt")
    keys = [(f"it1/grad/{k}", k) for k in ("vit.pos_emb.weight", "vit.extra_emb.weight", "vit.patch_proj.bias", "head.bias")]
    _held_to(dirty, keys, lambda t, k: _err(t, g["grads"][k]), lambda k: classifier_grad_bound(g["ref_bf16_floor"], k))


def test_classifier_two_training_steps(hip):
    _, dirty, _ = three_runs("vit-classifier", _classifier_workload, ATOMIC_VIT, downstream=True)
    _classifier_bounds(dirty)


def test_classifier_on_frames(hip):
    """the same model on uint8 vitamd.data.Frames (test_gpu_data._frames32: crop and flip per sample, the ImageNet table)"""
    from test_gpu_data import _frames32, _table
    g = load_golden("vit_s32.pt")

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        TV, m, optim = _classifier(g)
        make, table = _frames32(), _table(3)
        labels = W.randint(3, "labels", (4,), g["cfg"]["num_classes"]).cuda()
        return _train_two(m, lambda: TV.train_step(m, make(table), labels, optim), optim, dirty)
    three_runs("vit-classifier-frames", workload, ATOMIC_VIT, downstream=True)


def test_classifier_graphed_step(hip):
    """test_gpu_optim_graph._vit through GraphedTrainStep with the capturable optimiser: construction and capture inside poisoned(), two
    replays on new inputs with the scratch dirtied between them"""
    from test_gpu_optim_graph import VIT_SCHEDULE, _vit
    from vitamd import lm
    from vitamd.graph import GraphedTrainStep

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        m, opt, xs, ys = _vit(capturable=True, schedule=VIT_SCHEDULE)
        step = GraphedTrainStep(m, lambda x, y: lm.cross_entropy(m(x), y), (xs[0], ys[0]), opt)
        batches = iter(zip(xs, ys))
        out = _train_two(m, lambda: step(*next(batches)), opt, dirty, holders=(step,))
        assert step.captures == 1
        return out
    three_runs("vit-classifier-graph", workload, ATOMIC_VIT, downstream=True)


# ------------------------------------------------------------------------------------------------ 3. the blocks.py surface
ATOMIC_BLOCKS = [(r"(^|\.)(ln_\d|norm\d)\.(weight|bias)$", Q_AFFINE_LN), (r"(in_proj_bias|qkv\.bias)$", Q_ATTN_DBIAS),
                 (r"bias$", Q_COLSUM + " / " + Q_NT_COLSUM + " / the colsum= of " + Q_AFFINE_LN)]
BLOCK_DROPS = {"uvit_skip": dict(drop=0.1, attn_drop=0.1, drop_path=0.1), "uvit_bias": dict(drop=0.1, attn_drop=0.1, drop_path=0.1),
               "attn": dict(attn_drop=0.1, proj_drop=0.1), "mlp": dict(drop=0.1)}


@pytest.mark.parametrize("name", ["rab", "rab_nomlp", "uvit_skip", "uvit_bias", "attn", "mlp"])
def test_blocks_surface_in_training_mode(hip, name):
    """test_gpu_parity.BLOCK_CTORS in training mode with non-zero drop rates (affine LayerNorm, proj_drop, Mlp.drop, DropPath).  The
    reference fixture of these blocks has no dropout, so the excluded gradients (affine LayerNorm parameters and bias column sums) have
    no bound of an existing test to be held to here: they are held finite."""
    import blocks as BK
    from test_gpu_parity import BLOCK_CTORS
    case = load_golden("blocks_tiny.pt")[name]
    cls, kw = BLOCK_CTORS[name]
    L, N, D = 37, 3, 128

    def workload(dirty):
        torch.manual_seed(21)
        dirty()
        m = getattr(BK, cls)(**kw, **BLOCK_DROPS.get(name, {}))
        m.load_state_dict(W.module_state(case["seed"], case["shapes"]), strict=True)
        m = m.cuda().train()
        x = W.normal(case["seed"], "x", (L, N, D) if name.startswith("rab") else (N, L, D)).cuda().requires_grad_(True)
        dy = W.normal(case["seed"], "dy", tuple(x.shape)).cuda()
        args = [x]
        if name == "uvit_skip":
            args.append(W.normal(case["seed"], "skip", (N, L, D)).cuda().requires_grad_(True))
        y = m(*args)
        (y * dy).sum().backward()
        torch.cuda.synchronize()
        out = {"y": _cpu(y), "dx": _cpu(x.grad), **{k: _cpu(p.grad) for k, p in m.named_parameters()}}
        if len(args) == 2:
            out["dskip"] = _cpu(args[1].grad)
        return out
    three_runs(f"blocks-{name}", workload, ATOMIC_BLOCKS)


# ------------------------------------------------------------------------------------------------ 4. VideoGPT
ATOMIC_GPT = [(r"grad/tok_embed\.weight$", Q_DTOK), (r"grad/proj\.bias$", Q_COLSUM)]


def test_videogpt_two_training_steps_ragged_vocabulary(hip):
    """test_gpu_lm._videogpt_sized(250): the head shapes the fused route does not take; train_videogpt.train_step twice"""
    import train_videogpt as V
    from test_gpu_lm import VIDEOGPT_GRAD_BOUND, _oracle_grads, _videogpt_sized
    import vit_oracle as O
    from vitamd.optim import AdamW
    made = {}

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        model, sd, cfg = _videogpt_sized(250)
        made.update(sd=sd, cfg=cfg)
        model.train()
        x = W.randint(0, "video", (4, cfg.max_frames, cfg.frame_size), cfg.codebook_size).cuda()
        optim = AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
        return _train_two(model, lambda: V.train_step(model, x, optim), optim, dirty)
    _, dirty, _ = three_runs("videogpt-train-250", workload, ATOMIC_GPT, downstream=True)
    x = W.randint(0, "video", (4, made["cfg"].max_frames, made["cfg"].frame_size), made["cfg"].codebook_size)
    _, ograds = _oracle_grads(x, made["sd"], made["cfg"], ["tok_embed.weight"])
    _held_to(dirty, [("it1/grad/tok_embed.weight", "tok_embed.weight")], lambda t, k: O.rel_l2(t, ograds[k]), lambda k: VIDEOGPT_GRAD_BOUND)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_videogpt_generation_from_a_poisoned_cache(hip, graph):
    """test_gpu_decode_graph._videogpt: cached greedy and sampled generation; the fresh KVCache is torch.empty, so in the poisoned run
    every position the prefill and the steps have not written holds NaN.  The tokens are the exact output."""
    from test_gpu_decode_graph import SAMPLED, _prompt, _videogpt

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        model, cfg = _videogpt()
        video = _prompt(cfg, "prompt")
        out = {"greedy": _cpu(model.generate_frames(video, n=2, graph=graph))}
        dirty()
        out["sampled"] = _cpu(model.generate_frames(video, n=2, graph=graph, **SAMPLED))
        dirty()
        out["greedy_again"] = _cpu(model.generate_frames(_prompt(cfg, "prompt2"), n=2, graph=graph))
        return out
    three_runs(f"videogpt-generate-{'graph' if graph else 'eager'}", workload)


# ------------------------------------------------------------------------------------------------ 5. the tokenizers
# the tokenizers on train_vit.ViT stacks (TiTok, ViT-VQGAN): the stack itself is reproducible (BIAS_FROM_WGRAD), its embedding and the Linears around it are not
ATOMIC_VIT_TOK = [(r"grad/\w+\.vit\.(pos_emb\.weight|extra_emb\.weight|patch_proj\.bias)$", Q_EMBED_BWD), (r"grad/quant\.codebook\.weight$", Q_DCODEBOOK),
                  (r"grad/\w+\.(proj|quant_proj|embd_proj)\.bias$", Q_COLSUM)]
# the code-id TiTok: dpos and dprefix of the assembly are 'no atomics, reproducible bits' and stay exact
ATOMIC_CODE_TITOK = [(r"grad/enc\.tok_emb\.weight$", Q_ASSEMBLE), (r"grad/quant\.codebook\.weight$", Q_DCODEBOOK),
                     (r"grad/\w+\.(proj|quant_proj|emb_proj)\.bias$", Q_COLSUM)]
# the TA-TiTok on blocks.py: affine LayerNorms, attention's dbias, column sums; the conv tail gives 'The same bits on every call' and stays exact
ATOMIC_TATITOK = [(r"grad/.*\.(ln_pre|ln_post|ln_1|ln_2)\.(weight|bias)$", Q_AFFINE_LN), (r"grad/.*in_proj_bias$", Q_ATTN_DBIAS),
                  (r"grad/.*\.(out_proj|c_fc|c_proj|decoder_embed|patch_embed|ffn\.\d+)\.bias$", Q_COLSUM + " / " + Q_NT_COLSUM + " / the colsum= of " + Q_AFFINE_LN),
                  (r"grad/quantize\.embedding\.weight$", Q_DCODEBOOK)]
# the Enhancing ViT-VQGAN: the tanh MLP's bias gradients come from ops.gemm_tn(colsum=) ('no atomics, bitwise reproducible') and stay exact
ATOMIC_ENHANCING = [(r"grad/.*\.norm\.(weight|bias)$", Q_AFFINE_LN), (r"grad/quant\.codebook\.weight$", Q_DCODEBOOK),
                    (r"grad/(.*\.to_out|.*\.to_patch_embedding\.\d+|.*\.to_pixel\.\d+|pre_quant_proj|quant_proj)\.bias$", Q_COLSUM)]


def _tokenizer_bounds(dirty, clean, exact, g, err):
    """every step-1 gradient that is not exact, against the golden of the model's own test at that test's bound"""
    from test_gpu_parity import tokenizer_grad_bound
    floor = g["ref_bf16_floor"]
    keys = []
    for key in clean:
        k = key[len("it1/grad/"):]
        if key.startswith("it1/grad/") and key not in exact and k in g["grads"] and g["grads"][k]["norm"] != 0.0 and clean[key].numel():
            keys.append((key, k))
    _held_to(dirty, keys, lambda t, k: err(t, g["grads"][k]), lambda k: tokenizer_grad_bound(floor, k))


@pytest.mark.parametrize("name", ["titok_s256.pt", "vitvqgan_b256.pt"])
def test_tokenizer_two_training_steps(hip, name):
    """test_gpu_parity._tokenizer_model on its loss route (vq_quantize, linear_recon_mse), torch.optim.AdamW as the route's own test"""
    from test_gpu_parity import _err, _tokenizer_model
    made = {}

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        g, m, _, images = _tokenizer_model(name)
        made["g"] = g
        optim = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)

        def step():
            optim.zero_grad(set_to_none=True)
            recon_loss, qloss, _ = m.loss(images)
            loss = recon_loss + qloss
            loss.backward()
            optim.step()
            return loss
        return _train_two(m, step, optim, dirty)
    clean, dirty, exact = three_runs(f"tokenizer-{name[:-3]}", workload, ATOMIC_VIT_TOK, downstream=True)
    _tokenizer_bounds(dirty, clean, exact, made["g"], _err)


def test_tatitok_two_training_steps(hip):
    """test_gpu_tatitok._tatitok_model: the unit-code quantiser and the conv tail (linear_conv_recon_mse)"""
    import train_tatitok as TA
    from test_gpu_parity import _err
    from test_gpu_tatitok import _tatitok_model
    made = {}

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        g, m, images = _tatitok_model()
        made["g"] = g
        optim = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
        return _train_two(m, lambda: TA.train_step(m, images, optim), optim, dirty)
    clean, dirty, exact = three_runs("tokenizer-tatitok", workload, ATOMIC_TATITOK, downstream=True)
    _tokenizer_bounds(dirty, clean, exact, made["g"], _err)


def test_code_titok_two_training_steps(hip):
    """test_gpu_code_titok._model: token assembly, linear_cross_entropy"""
    import train_llamagen_titok as T
    from test_gpu_code_titok import _model
    from test_gpu_parity import _err
    made = {}

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        g, m, ids = _model()
        made["g"] = g
        optim = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
        return _train_two(m, lambda: T.train_step(m, ids, optim), optim, dirty)
    clean, dirty, exact = three_runs("tokenizer-code-titok", workload, ATOMIC_CODE_TITOK, downstream=True)
    _tokenizer_bounds(dirty, clean, exact, made["g"], _err)


def test_enhancing_two_training_steps(hip):
    """test_gpu_enhancing._model: tanh MLPs, the L1 tail"""
    from test_gpu_enhancing import _gerr, _model
    made = {}

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        EV, g, m, images = _model()
        made["g"] = g
        optim = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-4)
        return _train_two(m, lambda: EV.train_step(m, images, optim), optim, dirty)
    clean, dirty, exact = three_runs("tokenizer-enhancing", workload, ATOMIC_ENHANCING, downstream=True)
    g = made["g"]
    _tokenizer_bounds(dirty, clean, exact, g, lambda t, ref: _gerr(t, ref, g["grad_stride"]))


def test_titok_with_the_perceptual_term(hip):
    """train_titok.train_step with the small PerceptualLoss of test_gpu_perceptual.py (SMALL): its prepared()["scratch"] is dirtied too.
    The step-1 loss has no golden with this term; the excluded gradients are held finite."""
    import _perceptual_ref as R
    import train_titok as TT
    from test_gpu_parity import _tokenizer_model
    from test_gpu_perceptual import SMALL, _small_module

    def workload(dirty):
        torch.manual_seed(7)
        dirty()
        _, m, _, images = _tokenizer_model("titok_s256.pt")
        perc = _small_module(R.random_state(SMALL["depths"], SMALL["dims"], SMALL["num_classes"], 0))
        optim = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
        return _train_two(m, lambda: TT.train_step(m, images, optim, perceptual=perc, perceptual_weight=0.5), optim, dirty, holders=(perc,))
    three_runs("tokenizer-titok-perceptual", workload, ATOMIC_VIT_TOK, downstream=True)


# ------------------------------------------------------------------------------------------------ 6. the optimiser
def test_multi_tensor_adamw_with_active_clipping_and_clip_in_place(hip):
    """test_gpu_optim_multi._clip_inputs: two clipped steps of the multi-tensor AdamW (eager and with the resident table), then
    clip_grad_norm_ and grad_norm on the gradients alone.  'No float atomics: the same gradients give the same bits on every call':
    everything is exact."""
    from test_gpu_optim_multi import _clip_inputs
    from test_gpu_streaming import ADAMW_LRS
    from vitamd import optim as VO
    ps, gs = _clip_inputs(hip.vitamd_mt_chunk_elems())

    def workload(dirty):
        dirty()
        out = {}
        for tag, kwargs in (("eager", {}), ("resident", dict(capturable=True))):
            params = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
            opt = VO.AdamW(params, lr=ADAMW_LRS[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_grad_norm=1.0, **kwargs)
            for k in range(2):
                dirty(opt)
                for p, g in zip(params, gs[k]):
                    p.grad = g.clone().cuda()
                opt.step()
                out[f"{tag}/norm{k}"], out[f"{tag}/coef{k}"] = _cpu(opt.grad_norm).reshape(1), _cpu(opt.clip_coef).reshape(1)
            for i, p in enumerate(params):
                out[f"{tag}/p{i}"], out[f"{tag}/m{i}"], out[f"{tag}/v{i}"] = _cpu(p), _cpu(opt.state[p]["exp_avg"]), _cpu(opt.state[p]["exp_avg_sq"])
        params = [torch.nn.Parameter(torch.zeros(g.shape, device="cuda")) for g in gs[0]]
        for p, g in zip(params, gs[0]):
            p.grad = g.clone().cuda()
        dirty()
        out["grad_norm"] = _cpu(VO.grad_norm(params)).reshape(1)
        out["clip/norm"] = _cpu(VO.clip_grad_norm_(params, 1.0)).reshape(1)
        for i, p in enumerate(params):
            out[f"clip/g{i}"] = _cpu(p.grad)
        return out
    three_runs("optim-multi-tensor", workload)


# ------------------------------------------------------------------------------------------------ 7. the op sweep
def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _sweep_inputs():
    """CPU inputs of the sweep, made once and never modified"""
    g = torch.Generator().manual_seed(5)
    return types.SimpleNamespace(
        a=_rand((128, 128), 1), b=_rand((128, 128), 2, 0.05), bias=_rand((128,), 3), resid=_rand((128, 128), 4),
        x=_rand((40, 256), 5), addend=_rand((40, 256), 6), dy=_rand((40, 256), 7), gamma=_rand((256,), 8), beta=_rand((256,), 9),
        xk=_rand((16, 256), 10), addk=_rand((6, 256), 11), gk=_rand((6, 256), 12),
        qkv=_rand((2 * 40, 3 * 2 * 64), 13), d_o=_rand((2 * 40, 2 * 64), 14), ares=_rand((2 * 40, 2 * 64), 15),
        qkv_keep=_rand((2 * 130, 3 * 2 * 64), 16), do_keep=_rand((2 * 5, 2 * 64), 17),
        img=torch.rand((2, 3, 16, 16), generator=g), gemb=_rand((2 * 5, 256), 18),
        vx=_rand((10, 12), 19), cb=_rand((64, 12), 20), gq=_rand((10, 12), 21),
        cx=_rand((2, 3, 8, 8), 22), cw=_rand((3, 3, 3, 3), 23, 0.3), cbias=_rand((3,), 24),
        dqkv=_rand((2 * 3, 3 * 2 * 64), 25), dq1=_rand((2, 3 * 2 * 64), 26), da=_rand((2, 128), 27), dw=_rand((3 * 2 * 64, 128), 28, 0.05),
        dbias=_rand((3 * 2 * 64,), 29), tok=_rand((20, 64), 30), pos=_rand((8, 64), 31), prefix=_rand((2, 64), 32),
        ids=torch.randint(0, 20, (2, 5), generator=g), logits=_rand((6, 50), 33), target=torch.randint(0, 50, (6,), generator=g),
        u=torch.rand((6,), generator=g), rtok=_rand((8, 48), 34), rimg=torch.rand((2, 3, 8, 8), generator=g), grecon=_rand((2, 3, 8, 8), 35),
        dwx=_rand((2, 2, 2, 8), 36), dww=_rand((8, 7, 7), 37, 1 / 7), dwb=_rand((8,), 38), rimg20=torch.rand((2, 3, 20, 20), generator=g),
        grows=_rand((2 * 16, 64), 39), src=torch.randint(0, 256, (2, 9, 10, 3), generator=g, dtype=torch.uint8), table=_rand((3, 256), 40))


def _sweep(dirty):
    """one call of every wrapper of vitamd/ops.py at a small legal shape, on whatever the wrapper returns"""
    from vitamd import ops, perceptual
    I = _sweep_inputs()
    c, out = (lambda t: t.cuda()), {}
    cb16 = lambda t: t.cuda().to(BF16)

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                out[f"{name}/{i}"] = _cpu(t)
    dirty()
    a, b, bias = cb16(I.a), cb16(I.b), c(I.bias)
    put("gemm_nt_bias", ops.gemm_nt(a, b, ops.EPI_BIAS_BF16, bias=bias))
    put("gemm_nt_gelu", *ops.gemm_nt(a, b, ops.EPI_GELU, bias=bias))
    put("gemm_nt_f32", ops.gemm_nt(a, b, ops.EPI_F32, bias=bias))
    put("gemm_nt_resid", ops.gemm_nt(a, b, ops.EPI_RESID_F32, bias=bias, aux=c(I.resid)))
    put("linear_dropout_resid", ops.linear_dropout_resid(a, b, bias, c(I.resid), (0.1, 7)))
    dirty()
    put("gemm_tn", ops.gemm_tn(a, b, torch.zeros((128, 128), device="cuda"), accumulate=False))
    cs = torch.zeros(128, device="cuda")
    put("gemm_tn_colsum", ops.gemm_tn(a, b, torch.zeros((128, 128), device="cuda"), splits=2, accumulate=True, colsum=cs), cs)
    put("gemm_tn_atomic", ops.gemm_tn(a, b, torch.zeros((128, 128), device="cuda"), atomic=True))
    # LayerNorm
    x, dy = c(I.x), cb16(I.dy)
    xs, y, mean, rstd = ops.layernorm_fwd(x, cb16(I.addend))
    put("layernorm_fwd", xs, y, mean, rstd)
    put("layernorm_fwd_keep", *ops.layernorm_fwd_keep(c(I.xk), cb16(I.addk), 2, 8, 3))
    put("layernorm_bwd", *ops.layernorm_bwd(dy, xs, mean, rstd, g_res=x, want_bf16=True, dropout=(0.1, 3)))
    put("layernorm_bwd_xhat", *ops.layernorm_bwd(dy, xs, mean, rstd, want_bf16=True, xhat=y))
    xk, yk, mk, rk = ops.layernorm_fwd(c(I.xk))
    put("layernorm_bwd_keep", *ops.layernorm_bwd(cb16(I.xk), xk, mk, rk, g_res=c(I.gk), want_bf16=True, keep=(8, 3)))
    gamma, beta = c(I.gamma), c(I.beta)
    ya, ma, ra = ops.layernorm_affine_fwd(x, gamma, beta)
    put("layernorm_affine_fwd", ya, ma, ra)
    dg, db = torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")
    put("layernorm_affine_bwd", *ops.layernorm_affine_bwd(dy, x, ma, ra, gamma, dg, db, g_res=x, want_bf16=True), dg, db)
    yf, mf, rf = ops.layernorm_affine_fwd_f32(x, gamma, beta)
    put("layernorm_affine_fwd_f32", yf, mf, rf)
    dg2, db2 = torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")
    put("layernorm_affine_bwd_f32", ops.layernorm_affine_bwd_f32(c(I.dy), x, mf, rf, gamma, dg2, db2), dg2, db2)
    # attention
    dirty()
    qkv, d_o = cb16(I.qkv), cb16(I.d_o)
    o, lse = ops.attention_fwd(qkv, 2, 40, 2)
    put("attention_fwd", o, lse)
    put("attention_fwd_resid", *ops.attention_fwd(qkv, 2, 40, 2, causal=True, dropout=(0.1, 9), resid=c(I.ares)))
    dbq = torch.zeros(3 * 128, device="cuda")
    put("attention_bwd", ops.attention_bwd(qkv, o, lse, d_o, 2, 40, 2, dbias=dbq), dbq)
    qk = cb16(I.qkv_keep)
    ok, lk = ops.attention_fwd_keep(qk, 2, 130, 2, 5)
    put("attention_fwd_keep", ok, lk[..., :5])                       # 'lse2 fp32 [B, H, N] of which only [..., :nq] is written'
    put("attention_bwd_keep", ops.attention_bwd_keep(qk, ok, lk, cb16(I.do_keep), 2, 130, 2, 5))
    # helpers
    put("cast_bf16_dropout", ops.cast_bf16_dropout(x, (0.1, 5)))
    put("dropout", ops.dropout(x, 0.1, 5), ops.dropout(dy, 0.1, 5, group=256))
    put("cast_bf16", ops.cast_bf16(x))
    put("cast_weight", *ops.cast_weight(c(I.b), True, True))
    put("im2col", ops.im2col(c(I.img), 8))
    put("colsum", ops.colsum(a))
    put("embed_bwd", *ops.embed_bwd(c(I.gemb), 2, 5, 1, 256))
    put("vq_nearest", ops.vq_nearest(c(I.vx), c(I.cb)))
    cx, cw = c(I.cx), c(I.cw)
    put("conv3x3_fwd", ops.conv3x3_fwd(cx, cw, c(I.cbias)))
    put("conv3x3_bwd", *ops.conv3x3_bwd(cx, cw, c(I.grecon)))
    # decoding: a fresh (poisoned) cache, three positions appended, then one step at position 3
    dirty()
    kc = torch.empty((2, 2, 16, 64), dtype=BF16, device="cuda")
    vc = torch.empty_like(kc)
    if P._active:
        assert bool(torch.isnan(kc.float()).all())
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.kv_append(cb16(I.dqkv), kc, vc, n, 2, 3, 2, host_len=0)
    n.add_(3)
    q1 = ops.gemm_skinny_qkv_append(cb16(I.da), cb16(I.dw), c(I.dbias), kc, vc, n, 2, host_len=3)
    put("gemm_skinny_qkv_append", q1, kc[:, :, :4], vc[:, :, :4])
    put("decode_attention", ops.decode_attention(q1, kc, vc, n, 2, 2, host_len=3))
    put("gemm_skinny", *ops.gemm_skinny(cb16(I.da), cb16(I.dw), ops.EPI_GELU, bias=c(I.dbias)))
    put("gemm_skinny_f32", ops.gemm_skinny(cb16(I.da), cb16(I.dw), ops.EPI_F32, bias=c(I.dbias)))
    tok, pos, ids = c(I.tok), c(I.pos), c(I.ids)
    put("decode_embed", ops.decode_embed(tok, pos, ids[:, 0].contiguous(), n))
    put("sample_logits", *ops.sample_logits(c(I.logits), 0.8, 5, 0.9, u=c(I.u), return_info=True))
    # training the causal stack
    lr, ls, st = ops.cross_entropy_fwd(c(I.logits), c(I.target))
    put("cross_entropy_fwd", lr, ls, st)
    put("cross_entropy_bwd", ops.cross_entropy_bwd(c(I.logits), c(I.target), ls, st), ops.cross_entropy_bwd(c(I.logits), c(I.target), ls, st, out_dtype=BF16))
    put("embed_tokens_fwd", ops.embed_tokens_fwd(ids, tok, pos))
    put("assemble_tokens_fwd", ops.assemble_tokens_fwd(c(I.prefix), pos, ids=ids, tok_table=tok))
    # the tokenizers' kernels
    vx, cb, gq = c(I.vx), c(I.cb), c(I.gq)
    gl = torch.full((), 0.5, device="cuda")
    for name, fwd, bwd in (("vq_quantize", ops.vq_quantize_fwd, ops.vq_quantize_bwd), ("vq_quantize_unit", ops.vq_quantize_unit_fwd, ops.vq_quantize_unit_bwd)):
        unit, rnorm, q, idx, loss, codes = fwd(vx, cb, return_unit_codes=True)
        put(f"{name}_fwd", unit, rnorm, q, idx, loss, codes)
        put(f"{name}_bwd", *bwd(gq, gl, unit, rnorm, idx, cb))
    rtok, rimg, grecon = c(I.rtok), c(I.rimg), c(I.grecon)
    put("recon_mse_fwd", ops.recon_mse_fwd(rtok, rimg, 2, 4))
    put("recon_mse_bwd", ops.recon_mse_bwd(rtok, rimg, 2, 4))
    put("conv_recon_mse_fwd", *ops.conv_recon_mse_fwd(rtok, cw, c(I.cbias), rimg, 2, 4, want_recon=True))
    put("conv_recon_mse_bwd", *ops.conv_recon_mse_bwd(rtok, cw, c(I.cbias), rimg, 2, 4, g_loss=gl, g_recon=grecon))
    put("recon_l1_fwd", *ops.recon_l1_fwd(rtok, rimg, 2, 4, want_recon=True))
    put("recon_l1_bwd", ops.recon_l1_bwd(rtok, rimg, 2, 4, g_loss=gl, g_recon=grecon))
    put("tanh_bf16", ops.tanh_bf16(dy))
    put("tanh_bwd_bf16", ops.tanh_bwd_bf16(dy, cb16(I.x)))
    # the perceptual loss's kernels
    dwx, dww = c(I.dwx), c(I.dww)
    put("dwconv7_fwd", ops.dwconv7_fwd(dwx, dww, c(I.dwb)))
    put("dwconv7_bwd", ops.dwconv7_bwd(dwx, dww))
    th = perceptual.band_tables(20, 16, torch.device("cuda"))
    mean, std = torch.tensor([0.485, 0.456, 0.406], device="cuda"), torch.tensor([0.229, 0.224, 0.225], device="cuda")
    put("resize_norm_fwd", *ops.resize_norm_fwd(c(I.rimg20), th[0], th[0], mean, std, 16, want_rows=True, want_nchw=True))
    put("resize_norm_bwd", ops.resize_norm_bwd(c(I.grows), th[1], th[1], std, 2, 20, 20, 16))
    # the input pipeline
    geom = ops.crop_flip_draw(2, (9, 10), (8, 8), 11, 0)
    put("crop_flip_draw", geom)
    patches, img = ops.frames_prep(c(I.src), (8, 8), c(I.table), patch=4, image=True, geom=geom)
    put("frames_prep", patches, img)
    put("frames_to_u8", ops.frames_to_u8(c(I.rimg)))
    torch.cuda.synchronize()
    return out


ATOMIC_SWEEP = [(r"^gemm_tn_atomic/", Q_TN_ATOMIC), (r"^attention_bwd/1$", Q_ATTN_DBIAS), (r"^layernorm_affine_bwd(_f32)?/[1-9]$", Q_AFFINE_LN),
                (r"^embed_bwd/[013]$", Q_EMBED_BWD), (r"^conv3x3_bwd/[12]$", Q_CONV3X3), (r"^colsum/", Q_COLSUM)]


def test_op_sweep(hip):
    """The wrappers the models above do not reach (and, cheaply, those they do).  At these sizes a quantiser's dcodebook is exact: one
    256-row block ('where a code is picked in more than one 256-row block')."""
    three_runs("op-sweep", _sweep, ATOMIC_SWEEP)


# ------------------------------------------------------------------------------------------------ 8. teeth on the device
def test_zeros_replaced_by_empty_in_ops_is_reported(hip, monkeypatch):
    """vitamd.ops with torch.zeros / zeros_like turned into torch.empty / empty_like, on the classifier workload: under poison the
    accumulators of embed_bwd (dpos, dbias) and ops.colsum start from NaN, and compare() reports the gradients they become - poison
    reaches the kernels and comes back.  Only floating accumulators change; no integer input is affected, and a kernel that adds to
    NaN cannot fault (the second iteration then runs on NaN parameters)."""
    from vitamd import ops

    class Proxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def zeros(*args, **kwargs):
            return torch.empty(*args, **kwargs)

        @staticmethod
        def zeros_like(*args, **kwargs):
            return torch.empty_like(*args, **kwargs)

    clean = _classifier_workload(_noop)
    monkeypatch.setattr(ops, "torch", Proxy())
    with P.poisoned([]):
        dirty = _classifier_workload(P.dirty_scratch)
    monkeypatch.undo()
    fails = P.compare(clean, dirty, exact=set(clean))
    hit = {f.split(":")[0] for f in fails}
    print("reported:", sorted(k for k in hit if k.startswith("it1/")))
    want = {f"it1/grad/{k}" for k in ("vit.pos_emb.weight", "vit.patch_proj.bias", "head.bias")}      # embed_bwd's dpos and dbias, ops.colsum's out
    assert want <= hit
    assert all(not bool(torch.isfinite(dirty[k]).any()) for k in want)
    assert torch.equal(clean["it1/loss"], dirty["it1/loss"])        # the forward has no zeroed buffer: untouched
    assert want <= {f.split(":")[0] for f in P.compare(clean, dirty, exact=set())}      # and the finiteness rule alone sees it


# ------------------------------------------------------------------------------------------------ 9. the coverage condition (keep last)
NOT_REACHED = {
    ("ops.py", 137): "seam_probe: a timing probe of one device at 49152 x 2304, run once per process outside any workload; its output is never read",
    ("functions.py", 182): "streams_overlap: the seam timing probe of the two streams; its outputs are never read",
    ("data.py", 229): "DeviceLoader: pinned host slot of the loader (host memory, filled by copy_ before use)",
    ("data.py", 230): "DeviceLoader: the device half of a loader slot, filled by the copy from the pinned slot",
    ("data.py", 243): "DeviceLoader: pinned host slot for the labels",
}


def test_every_empty_site_of_the_package_was_poisoned(hip):
    """The union of the call sites logged by the workloads above against empty_sites(): everything but NOT_REACHED (at most one site in
    eight, each with its reason).  Run with the whole file: it reads what the other tests logged."""
    spans = P.site_spans()
    sites = set(spans)
    assert len(STATS) >= 25, f"the coverage test reads the logs of the workloads of this file: run the whole file ({len(STATS)} workloads ran)"
    hit = P.sites_hit(UNION, spans)
    missing = sorted(sites - hit - set(NOT_REACHED))
    stale = sorted(set(NOT_REACHED) - sites)
    reached_anyway = sorted(set(NOT_REACHED) & hit)
    print(f"\n{len(UNION)} poisoned allocations over {len(hit)} of {len(sites)} sites; NOT_REACHED {len(NOT_REACHED)}")
    for name, (n, s, sec) in STATS.items():
        print(f"  {name}: {n} allocations, {s} sites, {sec:.2f} s")
    print("missing:", missing)
    assert not stale, f"NOT_REACHED names lines that hold no call any more: {stale}"
    assert not reached_anyway, f"NOT_REACHED lists sites a workload does reach: {reached_anyway}"
    assert 8 * len(NOT_REACHED) <= len(sites)
    assert not missing, f"{len(missing)} torch.empty sites of vitamd/ were never poisoned: {missing}"
