"""Host-side checks of the tokenizer evaluation (vitamd/metrics.py, csrc/recon_metrics.hip): the float64 reference of
tests/_recon_ref.py against independent statements, a torch fp32 restatement of the kernel's arithmetic inside the derived bounds on
the inputs the GPU tests use, the comparison of the GPU tests against planted mistakes, the C ABI's symbols and refusals, the Python
surface's refusals, the allocation rule of tests/_poison.py and the scripts' flags.  No GPU is needed."""
import ast
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import _abi
import _poison as P
import _recon_ref as RR

F32, F64, BF16, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int64
ERR_SHAPE, ERR_ARG = 1, 2
TILE = 32


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_against_independent_statements():
    r, t, _, _ = RR.draw("noise", 3, 3, 23, 17, seed=1)
    ref = RR.recon_ref(r, t)
    for b in range(3):
        assert abs(float(ref["rows"][b, 0]) - float(F.mse_loss(r[b].to(F64), t[b].to(F64)))) < 1e-15
        assert abs(float(ref["rows"][b, 1]) - float(F.l1_loss(r[b].to(F64), t[b].to(F64)))) < 1e-15
        assert abs(float(ref["rows"][b, 2]) - 10 * math.log10(1.0 / float(ref["rows"][b, 0]))) < 1e-12
    assert ref["count"] == 3 and torch.equal(ref["sums"], ref["rows"].sum(dim=0))
    same = RR.recon_ref(t, t)
    assert same["rows"][:, 3].tolist() == [1.0] * 3 and same["rows"][:, 0].tolist() == [0.0] * 3            # exactly
    assert same["rows"][:, 2].tolist() == [float("inf")] * 3
    off = RR.recon_ref(r, t, ssim=False)
    assert torch.isnan(off["rows"][:, 3]).all() and torch.equal(off["rows"][:, :3], ref["rows"][:, :3])
    g = RR.gauss()
    assert abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0)) and abs(float(g[5] / g[4]) - math.exp(1 / 4.5)) < 1e-14


def test_single_window_ssim_is_the_formula_written_out():
    x, y, _, _ = RR.draw("noise", 1, 1, 11, 11, seed=2)
    g = RR.gauss()
    got = float(RR.recon_ref(x, y)["rows"][0, 3])
    mx = my = xx = yy = xy = 0.0
    for i in range(11):
        for j in range(11):
            w, a, b = float(g[i]) * float(g[j]), float(x[0, 0, i, j]), float(y[0, 0, i, j])
            mx, my, xx, yy, xy = mx + w * a, my + w * b, xx + w * a * a, yy + w * b * b, xy + w * a * b
    vx, vy, vxy = xx - mx * mx, yy - my * my, xy - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    want = (2 * mx * my + c1) * (2 * vxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    assert abs(got - want) < 1e-13
    x255 = RR.recon_ref(255 * x.to(F64), 255 * y.to(F64), data_range=255.0)              # SSIM and PSNR do not depend on the scale
    assert abs(float(x255["rows"][0, 3]) - want) < 1e-12 and abs(float(x255["rows"][0, 2]) - float(RR.recon_ref(x, y)["rows"][0, 2])) < 1e-12


def test_usage_is_the_reference_loops_counter_and_perplexity_has_its_ends():
    from vitamd.metrics import codebook_stats
    K = 64
    ids = torch.randint(0, 40, (7, 9), generator=torch.Generator().manual_seed(3))
    codebook_usage = torch.zeros([K])
    codebook_usage[ids] = 1                                                               # the reference loops' two lines
    ref = RR.hist_ref(ids, K)
    for stats in (RR.stats_ref(ref["hist"]), codebook_stats(ref["hist"])):
        assert stats["usage"] == codebook_usage.sum().item() / K and stats["dead"] == K - stats["used"] and stats["count"] == 63
    assert RR.check_stats(codebook_stats(ref["hist"], 2), RR.stats_ref(ref["hist"])) == []
    uniform, one = codebook_stats([3] * K), codebook_stats([0] * 5 + [17] + [0] * 58)
    assert abs(uniform["perplexity"] - K) < 1e-10 and uniform["usage"] == 1.0 and abs(RR.stats_ref(torch.full((K,), 3))["perplexity"] - K) < 1e-10
    assert one["perplexity"] == 1.0 and one["entropy"] == 0.0 and one["used"] == 1 and RR.stats_ref(torch.tensor([0, 17]))["perplexity"] == 1.0
    empty = codebook_stats([0] * K)
    assert empty["usage"] == 0.0 and empty["count"] == 0 and empty["perplexity"] != empty["perplexity"]


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic, in fp32, on the CPU
@pytest.mark.parametrize("size", range(9))
def test_fp32_restatement_of_the_kernel_lies_inside_the_bounds(size):
    """every value pattern and size of tests/test_gpu_recon_metrics.py, fp32 and bf16 reconstructions, the flat bright case included"""
    H, W = RR.sizes(TILE)[size]
    fails = []
    for n, kind in enumerate(RR.KINDS):
        for dtype in (F32, BF16):
            recon, target, R, clamp = RR.draw(kind, 2, 3, H, W, seed=100 * H + W + n)
            recon = recon.to(dtype)
            fails += RR.check_rows(RR.kernel32(recon, target, R, clamp), RR.recon_ref(recon, target, R, clamp), f"[{kind} {H}x{W} {dtype}]")
    assert not fails, "\n".join(fails)


def test_shifted_moments_are_what_keeps_the_flat_bright_case_small():
    """the cancellation argument of DESIGN.md section 25 in numbers: per window, raw fp32 second moments against the shifted ones"""
    x, y, _, _ = RR.draw("flat", 1, 1, 43, 42, seed=4)
    exact = RR.ssim_map(x.to(F64), y.to(F64), 1.0)
    g = RR.gauss().to(F32)
    blur = lambda z: F.conv2d(F.conv2d(z, g.reshape(1, 1, 1, 11)), g.reshape(1, 1, 11, 1))

    def fp32_map(shift):
        xs, ys = x - shift, y - shift
        m0, m1 = blur(xs), blur(ys)
        vx, vy, vxy = blur(xs * xs) - m0 * m0, blur(ys * ys) - m1 * m1, blur(xs * ys) - m0 * m1
        mx, my = m0 + shift, m1 + shift
        return ((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))

    raw, shifted = float((fp32_map(0.0).to(F64) - exact).abs().max()), float((fp32_map(0.5).to(F64) - exact).abs().max())
    print(f"flat bright case, largest error of one window: raw moments {raw:.2e}, shifted by R / 2 {shifted:.2e}")
    assert shifted < raw and shifted < float(RR.ssim_bound(x.to(F64), y.to(F64), 1.0)[0])


# ------------------------------------------------------------------------------------------------ the comparison
def test_comparison_catches_every_planted_mistake():
    """each mistake is applied to the reference and handed, as `got`, to the comparison the GPU tests use: it must be reported; the
    unchanged reference must pass"""
    recon, target, _, _ = RR.draw("outside", 3, 3, 40, 37, seed=5)               # values outside [0, 1]: the clamp matters
    target[0] = target[0] * 1.4 - 0.2                                             # ... also for a clamp wrongly put on the target
    recon[2] = recon[2] * 0.5 + 0.25                                              # images of different error: the batch mse is no image's
    nan = recon.clone()
    nan[1, 0, 20, 20] = float("nan")
    for bug in RR.BUGS:
        r = nan if bug == "nan_dropped" else recon
        ref = RR.recon_ref(r, target, clamp=True)
        assert RR.check_rows(ref["rows"], ref, "reference") == [] and RR.check_sums(ref["sums"], ref["count"], ref, "reference") == []
        bad = RR.recon_ref(r, target, clamp=True, bug=bug)
        assert RR.check_rows(bad["rows"], ref, bug), bug
        assert RR.check_sums(bad["sums"], bad["count"], ref, bug), bug
    refs = [RR.recon_ref(*RR.draw("noise", B, 3, 30, 30, seed=B)[:2]) for B in (2, 5, 1)]
    total = RR.accumulate(refs)
    assert total["count"] == 8 and RR.check_sums(total["sums"], total["count"], total, "accumulated") == []
    for bug in RR.ACC_BUGS:
        bad = RR.accumulate(refs, bug=bug)
        assert RR.check_sums(bad["sums"], bad["count"], total, bug), bug
    ids = torch.randint(0, 16, (200,), generator=torch.Generator().manual_seed(6))
    ids[::9], ids[4::17] = -1, 16
    href = RR.hist_ref(ids, 16)
    assert href["bad"] > 20 and RR.check_hist(href["hist"], href["bad"], href) == []
    for bug in ("oor_bin0", "oor_binK"):
        bad = RR.hist_ref(ids, 16, bug=bug)
        assert RR.check_hist(bad["hist"], bad["bad"], href, bug), bug
    assert RR.check_hist(href["hist"], href["bad"] - 1, href, "bad")
    few = RR.hist_ref(torch.tensor([1, 1, 1, 2, 2, 2, 2, 2]), 4)["hist"]          # 8 ids on 2 of 4 codes: usage 0.5, not 1
    assert RR.check_stats(RR.stats_ref(few), RR.stats_ref(few)) == []
    assert RR.check_stats(RR.stats_ref(few, bug="usage_from_count"), RR.stats_ref(few), "usage_from_count")


# ------------------------------------------------------------------------------------------------ the library
NEW = {"vitamd_recon_metrics": 16, "vitamd_recon_metrics_ws_bytes": 5, "vitamd_recon_metrics_grid_cap": 0, "vitamd_recon_metrics_tile": 0,
       "vitamd_recon_metrics_sum_depth": 0, "vitamd_code_hist": 6, "vitamd_code_hist_lds_max_k": 0, "vitamd_code_hist_grid_cap": 0}


def test_symbols_are_declared_bound_and_the_abi_stays_9():
    from vitamd import lib
    L = lib.load()
    text = open(os.path.join(os.path.dirname(_abi.HEADER), "vitamd_eval.h")).read()
    decls = {name: (ret, params) for ret, name, params in re.findall(r"\b(int|long)\s+(vitamd_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    assert set(decls) == set(NEW) == set(lib.EVAL_SIGNATURES) and not set(NEW) & set(lib.SIGNATURES)      # vitamd.h's table is untouched
    assert not set(NEW) & set(_abi.declared()[0])
    for name, n in NEW.items():
        fn = getattr(L, name)
        ret, params = decls[name]
        assert fn.argtypes == lib.EVAL_SIGNATURES[name] and len(fn.argtypes) == n == (0 if params.strip() in ("", "void") else params.count(",") + 1), name
        assert ret == ("long" if name.endswith("_ws_bytes") else "int") and fn.restype is lib.EVAL_RESTYPES[name]
    assert L.vitamd_recon_metrics_ws_bytes.restype is ctypes.c_long and L.vitamd_recon_metrics.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert L.vitamd_recon_metrics_tile() == TILE and L.vitamd_recon_metrics_sum_depth() == RR.SUM_DEPTH
    assert L.vitamd_recon_metrics_grid_cap() >= 256
    assert 16384 <= L.vitamd_code_hist_lds_max_k() < 65536 == lib.CONSTANTS["VITAMD_CODE_HIST_MAX_K"]
    assert L.vitamd_code_hist_lds_max_k() * 4 <= 160 * 1024 and L.vitamd_code_hist_grid_cap() >= 1
    assert "recon_metrics.hip" in open(os.path.join(lib.CSRC, "Makefile")).read()
    taps = [float(v) for v in RR.gauss().to(F32)]                                # the fp64-normalised taps rounded to fp32 once
    src = open(os.path.join(lib.CSRC, "recon_metrics.hip")).read()
    body = src[src.index("GAUSS[11] = {") + len("GAUSS[11] = {"):]
    held = [float(v.strip().rstrip("f")) for v in body[:body.index("}")].split(",")]
    assert [torch.tensor(v, dtype=F32).item() for v in held] == taps


def test_the_compiler_agrees_with_the_binding_of_the_new_header(tmp_path):
    """as tests/test_abi_parser_host.py does for vitamd.h: a function pointer of the parser's types initialised from every entry point of
    vitamd_eval.h; -fsyntax-only, any diagnostic fails"""
    from vitamd import lib
    lines = [f'#include "{lib.EVAL_HEADER}"']
    for name, (ret, types) in lib.EVAL_PROTOTYPES.items():
        lines.append(f"{ret} (*chk_{name})({', '.join(types)}) = &{name};")
    src = tmp_path / "eval_abi_check.cpp"
    src.write_text("\n".join(lines) + "\n")
    makefile = open(os.path.join(lib.CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)
    r = subprocess.run([hipcc, "-fsyntax-only", "-x", "c++", "-std=c++17", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip() and not r.stdout.strip(), r.stderr + r.stdout


def test_workspace_bytes_and_shape_limits():
    from vitamd import lib
    L = lib.load()
    ws = L.vitamd_recon_metrics_ws_bytes
    assert ws(1, 1, 11, 11, 1) == 12 and ws(2, 3, TILE, TILE, 1) == 72 and ws(2, 3, TILE + 1, TILE, 1) == 144 and ws(1, 1, 1, 1, 0) == 12
    top = lib.CONSTANTS["VITAMD_RECON_METRICS_MAX_DIM"]
    assert ws(1, 1, top, 11, 1) > 0
    for B, C, H, W, ssim in ((0, 1, 11, 11, 1), (1, 0, 11, 11, 1), (1, 1, 10, 11, 1), (1, 1, 11, 10, 1), (1, 1, 0, 5, 0), (1, 1, 5, 0, 0),
                             (1, 1, top + 1, 11, 1), (1, 1, 11, top + 1, 0), (1 << 31, 1, 11, 11, 1), (1 << 20, 1 << 12, 11, 11, 1),
                             (1 << 11, 1, top, top, 0)):
        assert ws(B, C, H, W, ssim) == -ERR_SHAPE, (B, C, H, W, ssim)


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; with real host addresses
    in every pointer a bad data_range is still refused; nothing is launched (no device is needed)"""
    from vitamd import lib
    L = lib.load()
    rm = L.vitamd_recon_metrics
    null = lambda B, C, H, W, ssim, ws_bytes=1 << 30, R=1.0: rm(None, 0, None, None, None, None, None, ws_bytes, B, C, H, W, R, 0, ssim, None)
    for B, C, H, W, ssim in ((0, 3, 32, 32, 1), (2, 0, 32, 32, 1), (2, 3, 10, 32, 1), (2, 3, 32, 10, 1), (2, 3, 0, 32, 0), (2, 3, 32, 0, 0),
                             (2, 3, 32769, 32, 1), (1 << 31, 1, 11, 11, 0)):
        assert null(B, C, H, W, ssim) == ERR_SHAPE, (B, C, H, W, ssim)
        assert null(B, C, H, W, ssim, R=-1.0) == ERR_SHAPE                       # the shape comes first
    assert null(2, 3, 32, 32, 1, ws_bytes=71) == ERR_SHAPE and null(2, 3, 32, 32, 1, ws_bytes=72) == ERR_ARG
    assert null(2, 3, 10, 10, 0) == ERR_ARG and null(2, 3, 1, 1, 0) == ERR_ARG
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    full = lambda R: rm(p, 0, p, p, p, p, p, 256, 1, 1, 11, 11, R, 0, 1, None)
    for R in (0.0, -1.0, float("inf"), float("nan"), 1e39):
        assert full(R) == ERR_ARG, R
    for missing in range(6):                                                     # each pointer alone
        ptrs = [p] * 6
        ptrs[missing] = None
        assert rm(ptrs[0], 0, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], 256, 1, 1, 11, 11, 1.0, 0, 1, None) == ERR_ARG, missing
    ch = L.vitamd_code_hist
    for M, K in ((0, 64), (-1, 64), (1 << 31, 64), (10, 1), (10, 0), (10, 65537)):
        assert ch(None, M, K, None, None, None) == ERR_SHAPE, (M, K)
    assert ch(None, 10, 2, None, None, None) == ERR_ARG and ch(None, 10, 65536, None, None, None) == ERR_ARG
    for missing in range(3):
        ptrs = [p] * 3
        ptrs[missing] = None
        assert ch(ptrs[0], 10, 64, ptrs[1], ptrs[2], None) == ERR_ARG, missing
    assert bytes(buf) == bytes(256)                                              # nothing was written


def test_python_surface_refuses_before_any_launch():
    from vitamd import metrics, ops
    from vitamd.lib import VitamdError
    r, t = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    acc = (torch.zeros(4, dtype=F64), torch.zeros(1, dtype=I64))
    for R in (0, -1.0, float("inf"), float("nan"), True, "1", None):
        with pytest.raises(ValueError):
            ops.recon_metrics(r, t, *acc, data_range=R)                          # also on CPU tensors: nothing has looked at a device yet
        with pytest.raises(ValueError):
            metrics.ReconMetrics(data_range=R, device="cpu")
    for flag in (2, -1, 0.5, "yes"):
        with pytest.raises(ValueError):
            ops.recon_metrics(r, t, *acc, clamp=flag)
        with pytest.raises(ValueError):
            ops.recon_metrics(r, t, *acc, ssim=flag)
    with pytest.raises(VitamdError):
        ops.recon_metrics(r, t, *acc)                                            # CPU tensors
    with pytest.raises(VitamdError):
        ops.recon_metrics(r.double(), t, *acc)
    with pytest.raises(ValueError):
        ops.code_hist(torch.zeros(4, dtype=I64), torch.zeros(1, dtype=I64), torch.zeros(1, dtype=I64))      # K = 1
    with pytest.raises(ValueError):
        ops.code_hist(torch.zeros(4, dtype=I64), torch.zeros(65537, dtype=I64), torch.zeros(1, dtype=I64))
    with pytest.raises(VitamdError):
        ops.code_hist(torch.zeros(4, dtype=I64), torch.zeros(8, dtype=I64), torch.zeros(1, dtype=I64))      # CPU tensors
    m = metrics.ReconMetrics(device="cpu")                                       # the accumulators exist; every update is refused
    assert m.sums.dtype == F64 and tuple(m.sums.shape) == (4,) and m.count.dtype == I64 and tuple(m.count.shape) == (1,)
    for bad in ((r, t), (r, t[:1]), (r[0], t[0]), (r, t.transpose(2, 3)), (None, t)):
        with pytest.raises(VitamdError):
            m.update(*bad)
    with pytest.raises(RuntimeError):
        m.rows()
    assert m.sums.tolist() == [0.0] * 4 and m.count.tolist() == [0]
    res = m.result()
    assert res["count"] == 0 and set(res) == {"mse", "mae", "psnr", "ssim", "count"} and all(res[k] != res[k] for k in ("mse", "mae", "psnr", "ssim"))
    for K in (1, 0, 65537, 64.0, True):
        with pytest.raises(ValueError):
            metrics.CodebookMetrics(K, device="cpu")
    c = metrics.CodebookMetrics(64, device="cpu")
    assert c.hist.dtype == I64 and tuple(c.hist.shape) == (64,) and tuple(c.bad.shape) == (1,)
    for bad in (torch.zeros(4, dtype=I64), torch.zeros(4, dtype=torch.int32), [1, 2]):
        with pytest.raises(VitamdError):
            c.update(bad)
    res = c.result()
    assert res["count"] == 0 and res["usage"] == 0.0 and res["dead"] == 64 and set(res) == {"usage", "used", "dead", "perplexity", "entropy", "count", "bad"}
    with pytest.raises(ValueError, match="no batches"):
        metrics.evaluate_tokenizer(torch.nn.Identity(), [])


def test_evaluate_tokenizer_restores_the_mode_and_reads_the_outputs():
    """on the CPU every update is refused, so the walk up to it is what can be checked here: the mode is put back when a batch raises,
    and both output forms are understood"""
    from vitamd import metrics
    from vitamd.lib import VitamdError
    ids = torch.zeros(2, 4, dtype=I64)
    assert metrics._tokenizer_outputs((1, ids, 0.0)) == (1, ids)
    assert metrics._tokenizer_outputs((1, {"min_encoding_indices": ids, "quantizer_loss": 0.0})) == (1, ids)
    with pytest.raises(TypeError):
        metrics._tokenizer_outputs(ids)

    class Tok(torch.nn.Module):
        config = type("C", (), {"codebook_size": 8})()

        def forward(self, x):
            assert not self.training and not torch.is_grad_enabled()
            return x, ids, 0.0

    model = Tok().train()
    with pytest.raises(VitamdError):
        metrics.evaluate_tokenizer(model, [torch.rand(2, 3, 16, 16)])
    assert model.training
    model.eval()
    with pytest.raises(VitamdError):
        metrics.evaluate_tokenizer(model, [torch.rand(2, 3, 16, 16)])
    assert not model.training


def test_no_uninitialised_allocation_was_added():
    """tests/test_gpu_poison.py demands that its workloads reach every torch.empty-family call of the package and names the ones they
    cannot by line: the tokenizer evaluation adds none, and the lines that test names still hold such calls"""
    spans = P.site_spans()
    assert not [k for k in spans if k[0] == "metrics.py"]
    import test_gpu_poison as TP
    for name, line in TP.NOT_REACHED:
        assert (name, line) in spans, (name, line)
    src = open(os.path.join(P.PKG_DIR, "ops.py")).read()
    first = min(n.lineno for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "recon_metrics_tile")
    assert not [k for k in spans if k[0] == "ops.py" and k[1] >= first]          # everything from there to the end of the file is new


_COMMON = {"image_size": 128, "patch_size": 16, "codebook_size": 2048, "latent_dim": 12, "transformer": "B", "bs": 32, "lr": 0.0001,
           "weight_decay": 0.0001, "warmup_steps": 5000, "train_steps": 50, "max_grad_norm": None, "u8": False, "resize": None,
           "perceptual_weight": 0.0, "perceptual_weights": None}
# every default the scripts had before the evaluation flags were added
DEFAULTS = {
    "train_titok": dict(_COMMON, latent_tokens=256),
    "train_vit_vqgan": dict(_COMMON),
    "train_tatitok": {"image_size": 256, "patch_size": 16, "latent_tokens": 256, "codebook_size": 16384, "latent_dim": 12, "transformer": "small",
                      "bs": 32, "lr": 0.0001, "weight_decay": 0.0001, "warmup_steps": 10000, "train_steps": 50, "max_grad_norm": 1.0,
                      "perceptual_weight": 0.0, "perceptual_weights": None},
    "train_enhancing_vitvqgan": {"image_size": 128, "patch_size": 16, "latent_tokens": 256, "codebook_size": 2048, "latent_dim": 12,
                                 "transformer": "B", "bs": 32, "lr": 0.0001, "weight_decay": 0.0001, "warmup_steps": 10000, "train_steps": 20,
                                 "perceptual_weight": 0.0, "perceptual_weights": None},
    "train_llamagen_titok": {"vq_codebook_size": 16384, "vq_latent_tokens": 256, "latent_tokens": 256, "codebook_size": 16384, "latent_dim": 12,
                             "transformer": "S", "bs": 32, "lr": 0.0001, "weight_decay": 0.0001, "warmup_steps": 5000, "train_steps": 1000000,
                             "steps": 50, "max_grad_norm": None, "vq": "none"},
}


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_scripts_accept_the_flags_and_default_to_off(name):
    import importlib
    mod = importlib.import_module(name)
    a = mod.parse_args([])
    assert a.eval_every == 0 and a.eval_batches >= 1
    b = mod.parse_args(["--eval_every", "10", "--eval_batches", "3"])
    assert (b.eval_every, b.eval_batches) == (10, 3)
    rest = lambda ns: {k: v for k, v in vars(ns).items() if not k.startswith("eval_")}
    assert rest(a) == rest(b) == DEFAULTS[name]
    assert callable(mod.evaluate)
    loop = open(importlib.import_module("train_titok" if name == "train_vit_vqgan" else name).__file__).read()      # run() is shared
    assert "if val is not None and (step + 1) % args.eval_every == 0:" in loop and "if args.eval_every > 0" in loop
