"""Weight-gradient (TN) GEMM forms on the three ViT-B shapes: the 8-wave ping-pong kernel (TN_FORM_SHARED) against the 12-wave loader-wave form
(TN_FORM_EXCLUSIVE, csrc/gemm_tn.hip), each without and with the column sums of L (colsum=: the bias gradient formed beside the MFMAs), split-K
workspace + reduce pass as in the step: interleaved rounds in one process, random data, medians.
usage: bench_tn.py"""
import os, sys, statistics, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
from vitamd import ops
cfgs = {"pp_d4": (ops.TN_FORM_SHARED, False), "pp_d4+colsum": (ops.TN_FORM_SHARED, True),
        "loader_waves": (ops.TN_FORM_EXCLUSIVE, False), "loader_waves+colsum": (ops.TN_FORM_EXCLUSIVE, True)}
dev = torch.device("cuda")
R = 256 * 197
shapes = [("dWqkv", 2304, 768), ("dW1", 3072, 768), ("dW2", 768, 3072)]
g = torch.Generator(device="cpu").manual_seed(3)
for name, P, Q in shapes:
    l = torch.randn(R, P, generator=g).to(dev, torch.bfloat16)
    r = torch.randn(R, Q, generator=g).to(dev, torch.bfloat16)
    out = torch.empty(P, Q, device=dev)
    cs = torch.zeros(P, device=dev)
    ref = None
    res = {k: [] for k in cfgs}
    for rnd in range(5):
        for k, (form, with_cs) in cfgs.items():
            kw = dict(colsum=cs) if with_cs else {}
            ops.gemm_tn(l, r, out, accumulate=False, form=form, **kw)
            if rnd == 0:
                torch.cuda.synchronize()
                if ref is None: ref = out.clone()
                else:
                    err = float((out - ref).norm() / ref.norm())
                    print(f"  {name} {k}: rel diff vs first variant {err:.2e}", flush=True)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); s.record()
            for _ in range(10): ops.gemm_tn(l, r, out, accumulate=False, form=form, **kw)
            e.record(); torch.cuda.synchronize()
            res[k].append(s.elapsed_time(e) / 10 * 1e3)
    fl = 2.0 * R * P * Q
    for k in cfgs:
        med = statistics.median(res[k])
        print(f"{name:6s} {k:20s} {med:7.1f} us  {fl / med / 1e6:7.1f} TF  {['%.0f' % v for v in res[k]]}", flush=True)
