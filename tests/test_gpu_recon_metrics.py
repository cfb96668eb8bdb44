"""The tokenizer evaluation on the device (csrc/recon_metrics.hip, vitamd/metrics.py ReconMetrics / CodebookMetrics / evaluate_tokenizer)
against the float64 reference and the derived bounds of tests/_recon_ref.py.  Integers must be equal; identical images must give
mse == 0, psnr == +inf and ssim == 1.0 exactly; every other value lies within its bound.  Each comparison records its error as a
fraction of the bound; the last test of the file prints the largest ones (a fraction above 1 has failed its own test before)."""
import functools

import pytest
import torch

import _recon_ref as RR

pytestmark = pytest.mark.gpu

F32, F64, BF16, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int64


def _tile():
    from vitamd import ops
    return ops.recon_metrics_tile()


def _offset_view(x):
    """x on the device as a contiguous view that starts one element into its allocation (off 16-byte alignment); the gap holds NaN"""
    buf = torch.full((x.numel() + 1,), float("nan"), dtype=x.dtype, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(x)
    return view


def _run(recon, target, data_range=1.0, clamp=False, ssim=True, offset=False, poison=False):
    """one call through the C ABI wrapper from zeroed accumulators -> (rows fp64 [B, 4], sums fp64 [4], count), on the host"""
    from vitamd import ops
    rd = _offset_view(recon.cuda()) if offset else recon.cuda()
    td = target.cuda()
    sums, count = torch.zeros(4, dtype=F64, device="cuda"), torch.zeros(1, dtype=I64, device="cuda")
    per_image = ws = None
    if poison:
        B, C, H, Wd = recon.shape
        per_image = torch.zeros((B, 4), dtype=F64, device="cuda")
        ws = torch.zeros((ops.recon_metrics_ws_bytes(B, C, H, Wd, ssim) // 4,), dtype=F32, device="cuda")
        per_image.view(torch.int64).fill_(-1)
        ws.view(torch.int32).fill_(-1)
    rows = ops.recon_metrics(rd, td, sums, count, per_image, ws, data_range=data_range, clamp=clamp, ssim=ssim)
    return rows.cpu(), sums.cpu(), int(count.cpu()[0])


def _check(recon, target, data_range, clamp, ssim, label, offset=False):
    rows, sums, count = _run(recon, target, data_range, clamp, ssim, offset)
    ref = RR.recon_ref(recon, target, data_range, clamp, ssim)
    return RR.check_rows(rows, ref, label) + RR.check_sums(sums, count, ref, label)


SIZES = list(range(9))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", SIZES)
def test_values_match_the_reference_at_the_tile_edges(hip, size, dtype):
    H, Wd = RR.sizes(_tile())[size]
    fails = []
    for n, kind in enumerate(("noise", "near", "flat", "outside", "outside_clamped", "range255")):
        B, C = ((1, 3), (3, 1), (3, 3), (1, 1))[(n + size) % 4]
        recon, target, R, clamp = RR.draw(kind, B, C, H, Wd, seed=100 * H + Wd + n)
        recon = recon.to(dtype)
        for ssim in (True, False):
            fails += _check(recon, target, R, clamp, ssim, f"[{kind} {B}x{C}x{H}x{Wd} ssim={int(ssim)}]")
        fails += _check(recon, target, R, clamp, True, f"[{kind} {B}x{C}x{H}x{Wd} offset view]", offset=True)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", SIZES)
def test_identical_images_are_exact(hip, size, dtype):
    H, Wd = RR.sizes(_tile())[size]
    t = torch.rand(3, 3, H, Wd, generator=torch.Generator().manual_seed(size)).to(dtype).to(F32)      # representable in both dtypes
    for offset in (False, True):
        rd = _offset_view(t.to(dtype).cuda()) if offset else t.to(dtype).cuda()
        from vitamd import ops
        sums, count = torch.zeros(4, dtype=F64, device="cuda"), torch.zeros(1, dtype=I64, device="cuda")
        rows = ops.recon_metrics(rd, t.cuda(), sums, count).cpu()
        assert rows[:, 0].tolist() == [0.0] * 3 and rows[:, 1].tolist() == [0.0] * 3
        assert rows[:, 2].tolist() == [float("inf")] * 3 and rows[:, 3].tolist() == [1.0] * 3
        assert sums.cpu().tolist() == [0.0, 0.0, float("inf"), 3.0] and int(count.cpu()[0]) == 3


@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_a_nan_marks_its_image_and_the_sums_only(hip, dtype, clamp):
    T = _tile()
    recon, target, _, _ = RR.draw("outside", 3, 3, T + 11, T + 10, seed=7)
    recon = recon.to(dtype)
    clean = _run(recon, target, clamp=clamp)[0]
    recon[1, 2, T + 3, 5] = float("nan")
    rows, sums, count = _run(recon, target, clamp=clamp)
    ref = RR.recon_ref(recon, target, 1.0, clamp)
    assert torch.isnan(ref["rows"][1]).all() and not torch.isnan(ref["rows"][[0, 2]]).any()
    assert torch.isnan(rows[1]).all() and torch.isnan(sums).all() and count == 3
    assert torch.equal(rows[[0, 2]], clean[[0, 2]])                                       # the other images: the same bits
    fails = RR.check_rows(rows, ref, "[NaN]")
    rows0 = _run(recon, target, clamp=clamp, ssim=False)[0]
    assert torch.isnan(rows0[1]).all() and not torch.isnan(rows0[[0, 2], :3]).any()
    recon[1, 2, T + 3, 5] = 0.5
    target[2, 0, 0, 0] = float("nan")                                                    # a NaN in the target marks its image too
    rows = _run(recon, target, clamp=clamp)[0]
    assert torch.isnan(rows[2]).all() and not torch.isnan(rows[:2]).any()
    assert not fails, "\n".join(fails)


def test_more_tiles_than_the_grid_cap(hip):
    from vitamd import ops
    B = ops.recon_metrics_grid_cap() + 37
    recon, target, _, _ = RR.draw("noise", B, 1, 11, 11, seed=9)
    recon[B - 2] = target[B - 2]                                                          # an image the second sweep of the grid reaches
    rows, sums, count = _run(recon, target)
    ref = RR.recon_ref(recon, target)
    fails = RR.check_rows(rows, ref, "[grid cap]")
    assert rows[B - 2].tolist() == [0.0, 0.0, float("inf"), 1.0] and count == B
    assert not fails, "\n".join(fails[:10])


# ------------------------------------------------------------------------------------------------ the accumulating object
def _batches():
    T = RR_T()
    out = []
    for n, (B, dtype, kind) in enumerate(((2, F32, "noise"), (5, BF16, "near"), (1, F32, "flat"))):
        recon, target, _, _ = RR.draw(kind, B, 3, T + 11, T + 8, seed=50 + n)
        out.append((recon.to(dtype), target))
    return out


@functools.lru_cache(maxsize=None)
def RR_T():
    return _tile()


@functools.lru_cache(maxsize=None)
def _accumulated():
    refs = [RR.recon_ref(r, t) for r, t in _batches()]
    return RR.accumulate(refs), refs


def _feed(m, poison=False):
    for r, t in _batches():
        assert m.update(r.cuda(), t.cuda()) is m
        if poison:                                           # what the next update finds in the scratch must not matter
            m._ws.view(torch.int32).fill_(-1)
            m._per_image.view(torch.int64).fill_(-1)
    return m


def test_updates_accumulate_reset_zeroes_and_runs_repeat(hip):
    from vitamd.metrics import ReconMetrics
    total, refs = _accumulated()
    m = ReconMetrics()
    with pytest.raises(RuntimeError):
        m.rows()
    _feed(m)
    assert m.sums.dtype == F64 and m.sums.is_cuda and tuple(m.sums.shape) == (4,) and m.count.dtype == I64 and tuple(m.count.shape) == (1,)
    fails = RR.check_sums(m.sums, m.count.cpu()[0], total, "three updates")
    fails += RR.check_rows(m.rows(), refs[-1], "rows of the last update")
    r = m.result()
    sums = m.sums.cpu().tolist()
    assert r == {"mse": sums[0] / 8, "mae": sums[1] / 8, "psnr": sums[2] / 8, "ssim": sums[3] / 8, "count": 8}
    first = (m.sums.clone(), m.count.clone())
    assert m.reset() is m and m.sums.cpu().tolist() == [0.0] * 4 and m.count.cpu().tolist() == [0]
    _feed(m, poison=True)                                    # the same object after reset(), its scratch reused and poisoned between updates
    again = _feed(ReconMetrics())
    for other in (m, again):
        assert torch.equal(other.sums.view(I64), first[0].view(I64)) and torch.equal(other.count, first[1])
    assert not fails, "\n".join(fails)


def test_poisoned_scratch_gives_the_same_bits(hip):
    recon, target, _, _ = RR.draw("near", 3, 3, RR_T() + 11, 37, seed=61)
    for ssim in (True, False):
        clean, poisoned = _run(recon, target, ssim=ssim), _run(recon, target, ssim=ssim, poison=True)
        assert torch.equal(clean[0].view(I64), poisoned[0].view(I64)) and torch.equal(clean[1].view(I64), poisoned[1].view(I64))
        assert clean[2] == poisoned[2] == 3


def test_update_records_into_a_graph_and_never_reads_back(hip):
    from vitamd.metrics import CodebookMetrics, ReconMetrics
    recon, target, _, _ = RR.draw("near", 4, 3, 64, 64, seed=71)
    ids = torch.randint(-1, 65, (4, 16), generator=torch.Generator().manual_seed(72))
    rd, td, idd = recon.to(BF16).cuda(), target.cuda(), ids.cuda()
    m, c = ReconMetrics(), CodebookMetrics(64)
    m.update(rd, td)                                         # eager once: the scratch exists before the capture
    c.update(idd)
    one, hist1, bad1 = m.sums.clone(), c.hist.clone(), c.bad.clone()
    m.reset(), c.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(rd, td)
        c.update(idd)
    assert m.count.cpu().tolist() == [0] and int(c.hist.sum()) == 0       # recorded, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert m.count.cpu().tolist() == [12] and torch.equal(m.sums, (one + one) + one)      # the same fp64 adds in the same order
    assert torch.equal(c.hist, 3 * hist1) and torch.equal(c.bad, 3 * bad1)
    assert m.result()["count"] == 12 and c.result()["count"] == int(3 * hist1.sum())


# ------------------------------------------------------------------------------------------------ the histogram
def _hist_run(ids, K):
    from vitamd import ops
    hist, bad = torch.zeros(K, dtype=I64, device="cuda"), torch.zeros(1, dtype=I64, device="cuda")
    ops.code_hist(ids.cuda(), hist, bad)
    return hist.cpu(), int(bad.cpu()[0])


def _ks():
    from vitamd import ops
    top = ops.code_hist_lds_max_k()
    assert 16384 <= top < 65536
    return [2, 2048, 16384, top, top + 1, 65536]


@pytest.mark.parametrize("k_index", range(6))
def test_histogram_equals_bincount(hip, k_index):
    K = _ks()[k_index]
    g = torch.Generator().manual_seed(K)
    fails = []
    cases = {
        "random": torch.randint(0, K, (8, 1000), generator=g),
        "all equal": torch.full((5000,), K - 1, dtype=I64),                               # every id on one bin
        "every bin once": torch.randperm(K, generator=g),
        "one id": torch.tensor([K // 2]),
    }
    mixed = torch.randint(0, K, (3001,), generator=g)
    mixed[::7] = -1
    mixed[3::11] = K
    mixed[5::13] = 1 << 40
    cases["out of range mixed in"] = mixed
    for label, ids in cases.items():
        hist, bad = _hist_run(ids, K)
        ref = RR.hist_ref(ids, K)
        assert int(ref["hist"].sum()) + ref["bad"] == ids.numel()
        assert torch.equal(ref["hist"], torch.bincount(ids.reshape(-1)[(ids.reshape(-1) >= 0) & (ids.reshape(-1) < K)], minlength=K))
        fails += RR.check_hist(hist, bad, ref, f"[K={K} {label}]")
    assert RR.hist_ref(mixed, K)["bad"] > 600
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("K", [2048, 65536])
def test_histogram_past_one_sweep_of_the_grid(hip, K):
    from vitamd import ops
    M = ops.code_hist_grid_cap() * 4096 + 4096 + 5           # the chunk of 4 096 ids per workgroup and sweep is the kernel's
    ids = torch.randint(0, K, (M,), generator=torch.Generator().manual_seed(3))
    ids[M - 1], ids[M - 2] = K - 1, -7                       # the tail the second sweep reaches
    hist, bad = _hist_run(ids, K)
    fails = RR.check_hist(hist, bad, RR.hist_ref(ids, K), f"[K={K} M={M}]")
    assert bad == 1 and not fails, "\n".join(fails)


def test_codebook_metrics_accumulate_and_report(hip):
    from vitamd.metrics import CodebookMetrics
    K = 2048
    g = torch.Generator().manual_seed(5)
    a, b = torch.randint(0, 300, (4, 32), generator=g), torch.randint(200, K + 3, (7, 3, 5), generator=g)
    b[0, 0, 0], b[1, 1, 1], b[6, 2, 4] = K, -3, 1 << 40
    c = CodebookMetrics(K)
    assert c.update(a.cuda()) is c and c.update(b.cuda().transpose(0, 2)) is c            # any shape, also a non-contiguous view
    ref = RR.hist_ref(torch.cat([a.reshape(-1), b.reshape(-1)]), K)
    fails = RR.check_hist(c.hist, c.bad.cpu()[0], ref, "two updates")
    r = c.result()
    fails += RR.check_stats(r, RR.stats_ref(ref["hist"]), "result")
    assert r["bad"] == ref["bad"] > 0 and set(r) == {"usage", "used", "dead", "perplexity", "entropy", "count", "bad"}
    usage = torch.zeros(K)
    ok = torch.cat([a.reshape(-1), b.reshape(-1)])
    usage[ok[(ok >= 0) & (ok < K)]] = 1                                    # the reference loops' counter
    assert r["usage"] == usage.sum().item() / K
    assert c.reset() is c and int(c.hist.sum()) == 0 and int(c.bad.sum()) == 0
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ the models
def _boom():
    raise RuntimeError("boom")


def _tiny(kind):
    import train_titok as TT
    import train_vit_vqgan as VQ
    torch.manual_seed(11)
    if kind == "titok":
        return TT, TT.TiTok(TT.TiTokConfig(32, 8, 8, 64, 12, "S")).cuda()
    return VQ, VQ.ViTVQGAN(VQ.ViTVQGANConfig(32, 8, 64, 12, "S")).cuda()


@pytest.mark.parametrize("kind", ["titok", "vitvqgan"])
def test_evaluate_of_a_tiny_tokenizer(hip, kind):
    from vitamd import data
    from vitamd.metrics import CodebookMetrics, ReconMetrics
    mod, model = _tiny(kind)
    model.train()
    images = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).cuda()
    u8 = torch.randint(0, 256, (4, 32, 32, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()
    recon, codes = ReconMetrics(), CodebookMetrics(64)
    result = mod.evaluate(model, [images, data.Frames(u8, 32)], recon=recon, codes=codes)
    assert model.training and all(p.grad is None for p in model.parameters())
    model.eval()
    frames = data.Frames(u8, 32)
    with torch.no_grad():
        outs = [model(images), model(frames)]
    targets = [images, frames.images()]
    refs = [RR.recon_ref(o[0].float().cpu(), t.cpu()) for o, t in zip(outs, targets)]
    fails = RR.check_sums(recon.sums, recon.count.cpu()[0], RR.accumulate(refs), kind)
    href = RR.hist_ref(torch.cat([o[1].reshape(-1).cpu() for o in outs]), 64)
    fails += RR.check_hist(codes.hist, codes.bad.cpu()[0], href, kind)
    expect = codes.result()
    expect["codes"] = expect.pop("count")
    expect.update(recon.result())
    assert result == expect and result["count"] == 8 and result["codes"] == sum(o[1].numel() for o in outs)
    assert 0.0 < result["usage"] <= 1.0 and result["bad"] == 0 and result["mse"] > 0.0
    model.train()
    with pytest.raises(RuntimeError, match="boom"):
        mod.evaluate(model, (_ for _ in [images] if not _boom()))
    assert model.training
    model.eval()
    mod.evaluate(model, [images])
    assert not model.training
    assert not fails, "\n".join(fails)


def test_zz_report_the_largest_fractions_of_the_bounds(hip):
    """not a check of its own: every comparison above has asserted its fraction <= 1; this prints what a GPU visit writes down"""
    print("\n" + RR.report_worst())
    assert all(v <= 1.0 for v in RR.WORST.values())
