"""The evaluation path on the device (csrc/loss.hip vitamd_classify_metrics, vitamd/metrics.py, the models' evaluate) against the
float64 reference of tests/_metrics_ref.py.  Integers (ranks, counts) must be equal; the per-row loss must have the bits of
ops.cross_entropy_fwd and lie within the rule of tests/_lm_ref.py::check_cross_entropy; loss_sum within the sum of the per-row bounds."""
import functools

import pytest
import torch

import _lm_ref as LR
import _metrics_ref as MR
import weights as W

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
IGNORE = -100

# (M, V, ld - V, base offset in elements, topk): V below one 16-byte piece (2, 7), one piece (8), a ragged tail (1000), whole pieces
# (1024), both sides of the wave-per-row / workgroup-per-row switch (4096, 4097), a wide ragged row (5000); dense and padded rows; the
# base offset by one element (the element-load path); topk in {1, 2, 5, V}
SHAPES = [(5, 2, 0, 0, 1), (9, 2, 24, 0, 2), (13, 7, 24, 0, 5), (12, 7, 0, 1, 7), (70, 8, 0, 1, 2), (31, 8, 24, 0, 8), (33, 1000, 0, 0, 5),
          (17, 1000, 24, 1, 1000), (21, 1024, 0, 0, 5), (10, 4096, 24, 0, 1), (6, 4096, 0, 1, 2), (9, 4097, 0, 0, 5), (7, 4097, 24, 1, 2),
          (6, 5000, 0, 0, 5), (5, 5000, 24, 1, 5000)]


def _place(x, pad, offset):
    """x [M, V] on the device with row stride V + pad, its first element `offset` elements into the allocation; the gaps hold NaN"""
    M, V = x.shape
    buf = torch.full((M * (V + pad) + offset,), float("nan"), dtype=x.dtype, device="cuda")
    view = buf[offset:].as_strided((M, V), (V + pad, 1))
    view.copy_(x)
    return view


def _draw(M, V, seed, ties):
    """ties: logits from five small integers; else randn x 3.  Targets include 0 and V - 1; rows 2 and M - 1 carry ignore_index; row 3's
    target holds the row's maximum and row 4's shares it with the next column (wide rows would otherwise never be hit)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (M, V), generator=g).to(F32) if ties else torch.randn(M, V, generator=g) * 3.0
    t = torch.randint(0, V, (M,), generator=g)
    x[3, int(t[3])] = 9.0
    x[4, int(t[4])] = x[4, (int(t[4]) + 1) % V] = 9.0
    t[0], t[1], t[2], t[M - 1] = 0, V - 1, IGNORE, IGNORE
    return x, t


def _run(x_dev, t_dev, topk):
    """one call from zeroed accumulators -> got dict (host) + loss_row (device)"""
    from vitamd import ops
    loss_sum = torch.zeros(1, dtype=F64, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    loss_row, rank = ops.classify_metrics(x_dev, t_dev, loss_sum, counts, topk=topk, ignore_index=IGNORE)
    return {"rank": rank.cpu(), "counts": counts.cpu().tolist(), "loss_sum": float(loss_sum.cpu()[0])}, loss_row


def _check_case(x, t, pad, offset, topk, label):
    """x: CPU logits in their dtype, t: CPU targets -> failures of one shape against every demand on a regular shape"""
    from vitamd import ops
    xd, td = _place(x.cuda(), pad, offset), t.cuda()
    got, loss_row = _run(xd, td, topk)
    ref = MR.metrics_ref(x, t, topk, IGNORE)
    ce_ref, t32 = LR.cross_entropy_ref(x, t, IGNORE), LR.cross_entropy_torch32(x, t, IGNORE)
    bound = LR.bound(LR.cross_entropy_errors({"loss_row": t32["loss_row"]}, ce_ref)["loss_row"])
    fails = MR.check_metrics(got, ref, MR.sum_allowance(ref, bound), label)
    fails += LR.check_cross_entropy({"loss_row": loss_row.cpu()}, ce_ref, t32, label)
    ce_rows = ops.cross_entropy_fwd(xd, td, IGNORE)[0]
    if not torch.equal(loss_row.view(torch.int32), ce_rows.view(torch.int32)):
        fails.append(f"{label}: loss_row differs in its bits from ops.cross_entropy_fwd's in "
                     f"{int((loss_row.view(torch.int32) != ce_rows.view(torch.int32)).sum())} rows")
    return fails


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M, V, pad, offset, topk", SHAPES)
def test_rank_counts_and_loss_match_the_reference(hip, M, V, pad, offset, topk, dtype):
    fails = []
    for ties in (False, True):
        x, t = _draw(M, V, seed=1000 * V + M, ties=ties)
        fails += _check_case(x.to(dtype), t, pad, offset, topk, f"[{M}x{V} ld+{pad} off{offset} k{topk} {'ties' if ties else 'randn'}]")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_row_stride_loop_past_the_grid_cap(hip, dtype):
    from vitamd import ops
    M = ops.cross_entropy_grid_rows(8) + 3
    x, t = _draw(M, 8, seed=8, ties=True)
    t[M - 2] = 7                                             # a row the second sweep of the grid reaches
    fails = _check_case(x.to(dtype), t, 0, 0, 2, f"[{M}x8]")
    assert not fails, "\n".join(fails)


def _check_special(x, t, topk, label):
    """shapes with non-finite losses: ranks and counts equal, the same rows non-finite, loss_sum non-finite as the reference's"""
    got, loss_row = _run(x.cuda(), t.cuda(), topk)
    ref = MR.metrics_ref(x, t, topk, IGNORE)
    fails = MR.check_metrics(got, ref, 0.0, label)
    if not torch.equal(torch.isfinite(loss_row.cpu()), torch.isfinite(ref["loss_row"])):
        fails.append(f"{label}: the non-finite rows differ: got {loss_row.cpu().tolist()}, reference {ref['loss_row'].tolist()}")
    assert not (ref["loss_sum"] - ref["loss_sum"] == 0.0), "the case was meant to have a non-finite sum"
    return fails


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_minus_infinity_entries(hip, dtype):
    x, t = _draw(12, 1000, seed=21, ties=False)
    x[1, 250:500] = float("-inf")                            # a block beside the target (V - 1): a finite loss
    x[3, int(t[3])] = float("-inf")                          # at the target: loss +inf, the -inf ties are broken by the column
    x[4, :] = float("-inf")
    x[4, 7] = 0.5                                            # one finite logit
    x[5, 10:20] = float("-inf")
    x[5, int(t[5])] = float("-inf")
    fails = _check_special(x.to(dtype), t, 5, "[-inf]")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_nan_never_makes_a_row_correct(hip, dtype):
    x, t = _draw(10, 1024, seed=22, ties=False)
    x[1, :] = -1.0
    x[1, int(t[1])] = float("nan")                           # the target would be the argmax of any order that lets a NaN win
    x[3, :] = -1.0
    x[3, int(t[3])] = 4.0                                    # the clear maximum ...
    x[3, (int(t[3]) + 5) % 1024] = float("nan")              # ... but a NaN elsewhere ranks above it
    ref = MR.metrics_ref(x.to(dtype), t, 1, IGNORE)
    assert int(ref["rank"][1]) == 1023 and int(ref["rank"][3]) == 1
    fails = _check_special(x.to(dtype), t, 1, "[NaN]")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_out_of_range_target_counts_as_wrong(hip, dtype):
    x, t = _draw(9, 7, seed=23, ties=True)
    t[3], t[4], t[5] = 7, -5, 1 << 40                        # none is ignore_index: counted, wrong for every k, NaN loss, no address formed
    ref = MR.metrics_ref(x.to(dtype), t, 7, IGNORE)
    assert ref["counts"][0] == 7 and ref["counts"][2] == 4 and [int(ref["rank"][i]) for i in (3, 4, 5)] == [7, 7, 7]
    fails = _check_special(x.to(dtype), t, 7, "[out of range]")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the accumulating object
def _batches():
    """three updates of different M, one of another V (topk = 2 fits both), fp32 and bf16, leading dimensions to flatten"""
    out = []
    for M, V, dtype, lead in ((24, 1000, F32, (4, 6)), (40, 1000, BF16, (40,)), (9, 8, F32, (3, 3))):
        x, t = _draw(M, V, seed=31 + M, ties=V == 8)
        out.append((x.to(dtype), t, lead))
    return out


def _accumulated_reference():
    refs, allow = [], 0.0
    for x, t, _ in _batches():
        r = MR.metrics_ref(x, t, 2, IGNORE)
        refs.append(r)
        allow += MR.sum_allowance(r, MR.row_bound(x, t, IGNORE))
    return MR.accumulate(refs), allow, refs


ACCUMULATED = functools.lru_cache(maxsize=None)(_accumulated_reference)


def _feed(m):
    for x, t, lead in _batches():
        assert m.update(x.cuda().reshape(*lead, x.shape[-1]), t.cuda().reshape(lead)) is m
    return m


def test_updates_accumulate_reset_zeroes_and_runs_repeat(hip):
    from vitamd.metrics import ClassifyMetrics
    total, allow, refs = ACCUMULATED()
    m = _feed(ClassifyMetrics(topk=2, ignore_index=IGNORE))
    assert m.loss_sum.dtype == F64 and m.loss_sum.is_cuda and m.counts.dtype == torch.int64 and m.counts.is_cuda
    got = {"counts": m.counts.cpu().tolist(), "loss_sum": float(m.loss_sum.cpu()[0])}
    fails = MR.check_metrics(got, total, allow, "three updates")
    loss_row, rank = m.rows()                                # the last update's rows
    assert tuple(loss_row.shape) == (9,) == tuple(rank.shape) and torch.equal(rank.cpu().long(), refs[-1]["rank"])
    r = m.result()
    assert r["count"] == total["counts"][0] and r["top1"] == total["counts"][1] / r["count"] and r["topk"] == total["counts"][2] / r["count"]
    assert r["loss"] == got["loss_sum"] / r["count"] and abs(r["perplexity"] - torch.tensor(r["loss"], dtype=F64).exp().item()) < 1e-9 * r["perplexity"]
    first = (m.loss_sum.clone(), m.counts.clone())
    assert m.reset() is m and float(m.loss_sum.cpu()[0]) == 0.0 and m.counts.cpu().tolist() == [0, 0, 0]
    _feed(m)                                                 # the same object after reset(), its scratch reused
    again = _feed(ClassifyMetrics(topk=2, ignore_index=IGNORE))
    for other in (m, again):
        assert torch.equal(other.loss_sum, first[0]) and torch.equal(other.counts, first[1])
        assert torch.equal(other.loss_sum.view(torch.int64), first[0].view(torch.int64))
    assert not fails, "\n".join(fails)


def test_update_records_into_a_graph_and_never_reads_back(hip):
    """a capture refuses any synchronising call: an update that records proves it reads nothing back; three replays add three times"""
    from vitamd.metrics import ClassifyMetrics
    x, t = _draw(24, 1000, seed=41, ties=False)
    xd, td = x.to(BF16).cuda(), t.cuda()
    ref = MR.metrics_ref(x.to(BF16), t, 5, IGNORE)
    m = ClassifyMetrics(topk=5, ignore_index=IGNORE)
    m.update(xd, td)                                         # eager once: the scratch exists before the capture
    one = float(m.loss_sum.cpu()[0])
    assert m.counts.cpu().tolist() == ref["counts"]
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(xd, td)
    assert m.counts.cpu().tolist() == [0, 0, 0]              # recorded, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert m.counts.cpu().tolist() == [3 * c for c in ref["counts"]]
    assert float(m.loss_sum.cpu()[0]) == (one + one) + one   # the same fp64 adds in the same order
    assert m.result()["count"] == 3 * ref["counts"][0]


# ------------------------------------------------------------------------------------------------ the models
def _model_fails(m, result, logits_cpu, target_cpu, label):
    """the accumulators of the ClassifyMetrics an evaluate call filled, and the result formed from them, against the reference applied
    to the logits the model gives for the same batches"""
    ref = MR.metrics_ref(logits_cpu, target_cpu, m.topk, IGNORE)
    allow = MR.sum_allowance(ref, MR.row_bound(logits_cpu, target_cpu, IGNORE))
    got = {"counts": m.counts.cpu().tolist(), "loss_sum": float(m.loss_sum.cpu()[0])}
    fails = MR.check_metrics(got, ref, allow, label)
    n = got["counts"][0]
    if result != {"loss": got["loss_sum"] / n, "top1": got["counts"][1] / n, "topk": got["counts"][2] / n, "count": n,
                  "perplexity": result["perplexity"]}:
        fails.append(f"{label}: result {result} is not formed from the accumulators {got}")
    return fails


def test_evaluate_vit(hip):
    import train_vit as TV
    from vitamd import data
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    model = TV.ViTClassifier(cfg, num_classes=10)
    model.load_state_dict(W.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10))
    model = model.cuda().train()
    images = W.normal(3, "images", (8, 3, 32, 32)).cuda()
    u8 = torch.randint(0, 256, (8, 32, 32, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    labels = [W.randint(3, "labels", (8,), 10).cuda(), W.randint(4, "labels", (8,), 10).cuda()]
    from vitamd.metrics import ClassifyMetrics
    m = ClassifyMetrics(topk=3, ignore_index=IGNORE)
    result = TV.evaluate(model, [(images, labels[0]), (data.Frames(u8, 32), labels[1])], metrics=m)
    assert model.training and all(p.grad is None for p in model.parameters())
    model.eval()
    with torch.no_grad():
        logits = torch.cat([model(images), model(data.Frames(u8, 32))]).float().cpu()
    fails = _model_fails(m, result, logits, torch.cat(labels).cpu(), "ViT")
    assert result["count"] == 16 and set(result) == {"loss", "top1", "topk", "count", "perplexity"}
    assert not fails, "\n".join(fails)
    model.train()
    with pytest.raises(RuntimeError, match="boom"):
        TV.evaluate(model, (_ for _ in [(images, labels[0])] if not _boom()), topk=3)
    assert model.training


def _boom():
    raise RuntimeError("boom")


@pytest.mark.parametrize("codebook", [64, 50])
def test_evaluate_videogpt(hip, codebook):
    import train_videogpt as V
    from test_gpu_lm import _videogpt_sized
    from vitamd import lm
    from vitamd.metrics import ClassifyMetrics
    model, _, cfg = _videogpt_sized(codebook)
    fused = lm.fused_head_applies(codebook, cfg.n_embd)
    assert fused == (codebook == 64)
    xs = [W.randint(s, "video", (2, cfg.max_frames, cfg.frame_size), codebook).cuda() for s in (0, 1)]
    model.train()
    m = ClassifyMetrics(topk=5, ignore_index=IGNORE)
    result = V.evaluate(model, xs, metrics=m)
    assert model.training and all(p.grad is None for p in model.parameters())
    model.eval()
    with torch.no_grad():
        outs = [model.eval_logits(x) for x in xs]
    assert all(o[0].dtype == (BF16 if fused else F32) and tuple(o[0].shape) == (x.numel(), codebook) and tuple(o[1].shape) == (x.numel(),)
               for o, x in zip(outs, xs))
    logits, target = torch.cat([o[0] for o in outs]).cpu(), torch.cat([o[1] for o in outs]).cpu()
    fails = _model_fails(m, result, logits, target, f"VideoGPT V={codebook}")
    assert result["count"] == sum(x.numel() for x in xs)
    one = V.evaluate(model, xs[:1], topk=5)
    ref = MR.metrics_ref(outs[0][0].cpu(), outs[0][1].cpu(), 5, IGNORE)
    allow = MR.sum_allowance(ref, MR.row_bound(outs[0][0].cpu(), outs[0][1].cpu(), IGNORE)) / one["count"]
    with torch.no_grad():
        mean = float(model.loss(xs[0]))
    print(f"VideoGPT V={codebook}: evaluate loss {one['loss']!r}, model.loss {mean!r}, |difference| {abs(one['loss'] - mean):.3e}, allowed {allow:.3e}")
    if not abs(one["loss"] - mean) <= allow:                 # the bound of the mean: the summed per-row bound over the count
        fails.append(f"evaluate loss {one['loss']!r} against model.loss {mean!r}: {abs(one['loss'] - mean):.3e} > {allow:.3e}")
    assert not fails, "\n".join(fails)
