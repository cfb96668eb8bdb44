"""References for the perceptual-loss tests (vitamd/perceptual.py, csrc/perceptual.hip).

Two independent evaluations of the same mathematics, both plain torch on the CPU:
  * the RESTATEMENT: the resize as its two tap matrices (closed form), the depthwise convolution as 49 shifted multiply-adds, LayerNorm,
    erf-GELU and the Linears written out, the network assembled by the key layout of torchvision's convnext_small.  Evaluated in float64 it
    is the reference of every GPU test; its `bug=` switches plant the mistakes the bounds must catch.
  * torch's OWN evaluation (F.interpolate, F.conv2d(groups=C), F.layer_norm, F.gelu, F.linear, autograd): the yardstick.  In float64 it
    must agree with the restatement; in fp32 (kernels) or under bf16 autocast (the network) its distance from the float64 reference is
    the floor the bounds are made of.

Bounds.  Kernels (fp32 arithmetic): the rule of _tokenizer_ref.bound, max |got - ref| / max(1, |ref|) <= max(4 e32, 8 * 2^-24) with e32
torch's fp32 figure at the same inputs; a kernel output stored as bf16 adds half a bf16 ulp, 2^-8 of the value.  Network (bf16 GEMM operands): relative
loss error and rel-L2 of the gradient <= 2 * floor + 1e-3, floor = the same distance for torch's bf16-autocast evaluation, the largest of
three seeds (the convention of test_gpu_parity.py)."""
import math

import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 8 * 2.0 ** -24
HALF_BF16_ULP = 2.0 ** -8          # bf16 keeps 8 significant bits: a value in [2^e, 2^(e+1)) is rounded by at most 2^(e-8) <= 2^-8 |value|
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-6

KERNEL_BUGS = ("no_flip", "clamp_border", "no_bias", "shift")
RESIZE_BUGS = ("no_antialias", "align_corners", "no_renorm", "no_std")      # + the untransposed table, planted by hand in the host test
NET_BUGS = ("no_layer_scale", "no_residual", "no_down_ln", "mean_over_batch")


def bound(e32, bf16_out=False):
    return max(4 * e32, FLOOR) + (HALF_BF16_ULP if bf16_out else 0.0)


def dist(got, ref):
    """max |got - ref| / max(1, |ref|); a NaN or inf in got counts as infinite"""
    ref = ref.to(F64)
    d = (got.to(F64) - ref).abs() / ref.abs().clamp_min(1.0)
    return float("inf") if not bool(torch.isfinite(got).all()) else float(d.max())


def rel(got, ref):
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1e-30)


# ------------------------------------------------------------------------------------------ resize
def taps(n_in, n_out, bug=None):
    """float64 [n_out, n_in]: one axis of the antialiased bilinear resize (align_corners=False) as a matrix, by the closed form"""
    scale = n_in / n_out
    if bug == "align_corners":
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    support = 1.0 if bug == "no_antialias" else max(scale, 1.0)
    m = torch.zeros((n_out, n_in), dtype=F64)
    for o in range(n_out):
        centre = o * scale + 0.5 if bug == "align_corners" else (o + 0.5) * scale
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)
        full = [max(0.0, 1.0 - abs((j - centre + 0.5) / support)) for j in range(int(centre - support + 0.5), int(centre + support + 0.5))]
        w = torch.tensor([max(0.0, 1.0 - abs((j - centre + 0.5) / support)) for j in range(lo, hi)], dtype=F64)
        m[o, lo:hi] = w / (sum(full) if bug == "no_renorm" else w.sum())
    return m


def resize_norm_ref(img, size, bug=None):
    """float64: (Wh . img . Ww^T - mean) / std"""
    img = img.to(F64)
    wh, ww = taps(img.shape[2], size, bug), taps(img.shape[3], size, bug)
    out = torch.einsum("oh,bchw,pw->bcop", wh, img, ww)
    return (out - torch.tensor(MEAN, dtype=F64)[None, :, None, None]) / torch.tensor(STD, dtype=F64)[None, :, None, None]


def resize_norm_bwd_ref(g, h_in, w_in, bug=None):
    """float64: Wh^T . g . Ww / std"""
    g = g.to(F64)
    size = g.shape[2]
    wh, ww = taps(h_in, size), taps(w_in, size)
    s = torch.ones(3, dtype=F64) if bug == "no_std" else torch.tensor(STD, dtype=F64)
    return torch.einsum("oh,bcop,pw->bchw", wh, g / s[None, :, None, None], ww)


def resize_norm_torch(img, size, dtype=F64, g=None):
    """torch's own evaluation -> (out, dimg or None)"""
    x = img.detach().to(dtype).clone().requires_grad_(g is not None)
    mean, std = torch.tensor(MEAN, dtype=dtype)[None, :, None, None], torch.tensor(STD, dtype=dtype)[None, :, None, None]
    out = (F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=True) - mean) / std
    if g is None:
        return out.detach(), None
    out.backward(g.to(dtype))
    return out.detach(), x.grad


def rows_to_nchw(rows, B, size):
    """the patch-row layout of include/vitamd.h vitamd_resize_norm_fwd [B*(S/4)^2, >= 48] -> [B, 3, S, S]"""
    P = size // 4
    return rows[:, :48].reshape(B, P, P, 3, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, size, size)


def nchw_to_rows(x, ld=64):
    B, _, size, _ = x.shape
    P = size // 4
    rows = torch.zeros((B * P * P, ld), dtype=x.dtype)
    rows[:, :48] = x.reshape(B, 3, P, 4, P, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * P * P, 48)
    return rows


# ------------------------------------------------------------------------------------------ depthwise 7x7
def dwconv_ref(x, w, bias=None, bug=None):
    """float64, channels-last x [B, H, W, C], w [C, 7, 7]: y = bias + sum_k w[c, kh, kw] x[h + kh - 3, w + kw - 3], 49 shifted multiply-adds"""
    x, w = x.to(F64), w.to(F64)
    B, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3), mode="replicate" if bug == "clamp_border" else "constant").permute(0, 2, 3, 1)
    y = torch.zeros_like(x)
    off = 1 if bug == "shift" else 0
    xp = F.pad(xp, (0, 0, 0, 1, 0, 0))              # one spare column so the shifted window stays inside
    for kh in range(7):
        for kw in range(7):
            y += w[:, kh, kw] * xp[:, kh:kh + H, kw + off:kw + off + W, :]
    if bias is not None and bug != "no_bias":
        y += bias.to(F64)
    return y


def dwconv_bwd_ref(g, w, bug=None):
    """float64 input gradient: dx[h, w] = sum_k w[c, kh, kw] g[h + 3 - kh, w + 3 - kw] = the forward with the taps reversed"""
    wf = w if bug == "no_flip" else torch.flip(w, dims=(1, 2))
    return dwconv_ref(g, wf, None, bug if bug in ("clamp_border", "shift") else None)


def dwconv_torch(x, w, bias, g=None, dtype=F64):
    """torch's own evaluation (F.conv2d with groups=C, NCHW inside) -> (y, dx or None), channels-last in and out"""
    xx = x.detach().to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(g is not None)
    y = F.conv2d(xx, w.to(dtype)[:, None], None if bias is None else bias.to(dtype), padding=3, groups=w.shape[0])
    if g is None:
        return y.detach().permute(0, 2, 3, 1), None
    y.backward(g.to(dtype).permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xx.grad.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------ the network
def keys(depths, dims, num_classes):
    """{key: shape} of torchvision's convnext (without any prefix), by the published structure"""
    out = {"features.0.0.weight": (dims[0], 3, 4, 4), "features.0.0.bias": (dims[0],), "features.0.1.weight": (dims[0],), "features.0.1.bias": (dims[0],)}
    for s in range(4):
        f, d = 2 * s + 1, dims[s]
        for i in range(depths[s]):
            p = f"features.{f}.{i}."
            out.update({p + "block.0.weight": (d, 1, 7, 7), p + "block.0.bias": (d,), p + "block.2.weight": (d,), p + "block.2.bias": (d,),
                        p + "block.3.weight": (4 * d, d), p + "block.3.bias": (4 * d,), p + "block.5.weight": (d, 4 * d), p + "block.5.bias": (d,),
                        p + "layer_scale": (d, 1, 1)})
        if s < 3:
            p = f"features.{f + 1}."
            out.update({p + "0.weight": (d,), p + "0.bias": (d,), p + "1.weight": (dims[s + 1], d, 2, 2), p + "1.bias": (dims[s + 1],)})
    out.update({"classifier.0.weight": (dims[3],), "classifier.0.bias": (dims[3],), "classifier.2.weight": (num_classes, dims[3]),
                "classifier.2.bias": (num_classes,)})
    return out


def random_state(depths, dims, num_classes, seed):
    """weights at order-one scale, so every layer matters: weights ~ N(0, 1/fan_in), biases ~ N(0, 0.1^2), LayerNorm weight 1 + N(0, 0.1^2),
    layer_scale ~ N(0, 0.5^2) (with torchvision's 1e-6 the blocks would not be tested)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in keys(depths, dims, num_classes).items():
        if k.endswith("layer_scale"):
            v = torch.randn(shape, generator=g) * 0.5
        elif k.endswith("bias"):
            v = torch.randn(shape, generator=g) * 0.1
        elif len(shape) == 1:
            v = 1 + torch.randn(shape, generator=g) * 0.1
        else:
            v = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
        sd[k] = v
    return sd


def _ln(x, w, b):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * w + b


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def logits_restated(sd, img, depths, size, bug=None):
    """the restatement, in the dtype of sd / img (float64 for the reference), channels-last inside"""
    dt = img.dtype
    wh, ww = taps(img.shape[2], size).to(dt), taps(img.shape[3], size).to(dt)
    x = (torch.einsum("oh,bchw,pw->bcop", wh, img, ww) - torch.tensor(MEAN, dtype=dt)[None, :, None, None]) / torch.tensor(STD, dtype=dt)[None, :, None, None]
    B = x.shape[0]
    P = size // 4
    w = sd["features.0.0.weight"]
    x = x.reshape(B, 3, P, 4, P, 4).permute(0, 2, 4, 1, 3, 5).reshape(B, P, P, 48) @ w.reshape(w.shape[0], 48).t() + sd["features.0.0.bias"]
    x = _ln(x, sd["features.0.1.weight"], sd["features.0.1.bias"])
    for s in range(4):
        f = 2 * s + 1
        for i in range(depths[s]):
            p = f"features.{f}.{i}."
            y = dwconv_ref(x, sd[p + "block.0.weight"][:, 0], sd[p + "block.0.bias"]).to(dt)
            y = _ln(y, sd[p + "block.2.weight"], sd[p + "block.2.bias"])
            y = _gelu(y @ sd[p + "block.3.weight"].t() + sd[p + "block.3.bias"]) @ sd[p + "block.5.weight"].t() + sd[p + "block.5.bias"]
            if bug != "no_layer_scale":
                y = y * sd[p + "layer_scale"].reshape(-1)
            x = y if bug == "no_residual" else x + y
        if s < 3:
            p = f"features.{f + 1}."
            if bug != "no_down_ln":
                x = _ln(x, sd[p + "0.weight"], sd[p + "0.bias"])
            Bq, H, W, C = x.shape
            w = sd[p + "1.weight"]                  # [C', C, 2, 2]: y[h, w] = sum_{c, kh, kw} w[:, c, kh, kw] x[2h + kh, 2w + kw, c]
            x = torch.einsum("bhkwlc,ockl->bhwo", x.reshape(Bq, H // 2, 2, W // 2, 2, C), w) + sd[p + "1.bias"]
    x = x.mean(dim=(1, 2))
    x = _ln(x, sd["classifier.0.weight"], sd["classifier.0.bias"])
    return x @ sd["classifier.2.weight"].t() + sd["classifier.2.bias"]


def logits_torch(sd, img, depths, size):
    """torch's own operators, NCHW with the two permutes per block as torchvision writes it"""
    x = F.interpolate(img, size=size, mode="bilinear", align_corners=False, antialias=True)
    x = (x - torch.tensor(MEAN, dtype=img.dtype)[None, :, None, None]) / torch.tensor(STD, dtype=img.dtype)[None, :, None, None]
    x = F.conv2d(x, sd["features.0.0.weight"], sd["features.0.0.bias"], stride=4)
    ln2d = lambda t, w, b: F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), w, b, EPS).permute(0, 3, 1, 2)
    x = ln2d(x, sd["features.0.1.weight"], sd["features.0.1.bias"])
    for s in range(4):
        f = 2 * s + 1
        for i in range(depths[s]):
            p = f"features.{f}.{i}."
            y = F.conv2d(x, sd[p + "block.0.weight"], sd[p + "block.0.bias"], padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (y.shape[-1],), sd[p + "block.2.weight"], sd[p + "block.2.bias"], EPS)
            y = F.linear(F.gelu(F.linear(y, sd[p + "block.3.weight"], sd[p + "block.3.bias"])), sd[p + "block.5.weight"], sd[p + "block.5.bias"])
            x = x + sd[p + "layer_scale"] * y.permute(0, 3, 1, 2)
        if s < 3:
            p = f"features.{f + 1}."
            x = F.conv2d(ln2d(x, sd[p + "0.weight"], sd[p + "0.bias"]), sd[p + "1.weight"], sd[p + "1.bias"], stride=2)
    x = F.layer_norm(x.mean(dim=(2, 3)), (x.shape[1],), sd["classifier.0.weight"], sd["classifier.0.bias"], EPS)
    return F.linear(x, sd["classifier.2.weight"], sd["classifier.2.bias"])


def loss_and_grad(sd, inp, tgt, depths, size, how="restated", dtype=F64, autocast=False, bug=None):
    """-> (loss, d loss / d input) of mse_loss(logits(input), logits(target)); how: 'restated' or 'torch'; autocast: torch's CPU bf16
    autocast around fp32 weights and images (how='torch'), the flow a user of the torch-op route gets"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = inp.detach().to(dtype).clone().requires_grad_(True)
    t = tgt.detach().to(dtype)
    fn = (lambda im: logits_restated(sd, im, depths, size, bug)) if how == "restated" else (lambda im: logits_torch(sd, im, depths, size))
    with torch.autocast("cpu", dtype=BF16, enabled=autocast):
        li = fn(x)
        with torch.no_grad():
            lt = fn(t)
        li, lt = li.float() if autocast else li, lt.float() if autocast else lt
        loss = ((li - lt) ** 2).mean(dim=0).sum() if bug == "mean_over_batch" else ((li - lt) ** 2).mean()
    loss.backward()
    return loss.detach(), x.grad


def images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = torch.rand((B, 3, H, W), generator=g)
    return (tgt + 0.1 * torch.randn((B, 3, H, W), generator=g)).clamp(0, 1), tgt


# one CNBlock on rows, for the stage-1 test at real width
def block_ref(x, sd, p, dtype=F64, how="restated"):
    """x [B, H, W, C] channels-last -> block output, in dtype; sd keys as in keys() under the prefix p"""
    if how == "torch":
        xc = x.permute(0, 3, 1, 2)
        y = F.conv2d(xc, sd[p + "block.0.weight"], sd[p + "block.0.bias"], padding=3, groups=xc.shape[1]).permute(0, 2, 3, 1)
        y = F.layer_norm(y, (y.shape[-1],), sd[p + "block.2.weight"], sd[p + "block.2.bias"], EPS)
        y = F.linear(F.gelu(F.linear(y, sd[p + "block.3.weight"], sd[p + "block.3.bias"])), sd[p + "block.5.weight"], sd[p + "block.5.bias"])
        return x + sd[p + "layer_scale"].reshape(-1) * y
    y = dwconv_ref(x, sd[p + "block.0.weight"][:, 0], sd[p + "block.0.bias"]).to(dtype)
    y = _ln(y, sd[p + "block.2.weight"], sd[p + "block.2.bias"])
    y = _gelu(y @ sd[p + "block.3.weight"].t() + sd[p + "block.3.bias"]) @ sd[p + "block.5.weight"].t() + sd[p + "block.5.bias"]
    return x + y * sd[p + "layer_scale"].reshape(-1)
