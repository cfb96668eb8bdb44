"""float64 restatements of what the Enhancing ViT-VQGAN kernels compute (csrc/enhancing.hip: tanh and its backward from the saved
output, the L1 pixel tail in the (c p1 p2) feature order of nn.ConvTranspose2d), the checks their GPU tests hold them to, and torch fp32
stand-ins that the host test plants mistakes in.  No GPU, no library: plain torch.

Bounds.  tanh and its backward: every element within one bf16 ulp (taken at the float64 reference) of the float64 value, no share of
elements excused - a correctly computed fp32 value lies within 2^-20 of it and the rounding to bf16 adds half an ulp.  The L1 loss:
the bound of the squared-error loss (tests/_tokenizer_ref.py: max(4 e32, 8 * 2^-24) on the scale max(1, |ref|), e32 being the distance of
torch's fp32 CPU evaluation) - the sum has the same length and structure.  The image: exactly the shuffled tokens.  The gradient
g sign(recon - image) / N + g_image: within one ulp of the tokens' dtype, and exactly g_image (or 0) at the planted ties."""
import torch

from _tokenizer_ref import _dist, bound

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
G_LOSS = 2.5                      # an upstream gradient other than 1


def ulp(ref, dtype):
    """the spacing of `dtype` (bf16 or fp32) at |ref|, float64; subnormal range: the smallest spacing"""
    bits, emin = (7, -126) if dtype == BF16 else (23, -126)
    e = torch.floor(torch.log2(ref.to(F64).abs().clamp_min(2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - bits)


def outside_ulp(got, ref, dtype, n_ulp=1.0):
    """mask of the elements further than n_ulp spacings of dtype from the float64 reference (a NaN or inf in got counts as outside)"""
    d = (got.to(F64) - ref.to(F64)).abs()
    return ~(d <= n_ulp * ulp(ref, dtype))


# ------------------------------------------------------------------------------------------------ tanh
def tanh_values(n, seed):
    """bf16 inputs: uniform in +-4 with +-0, +-1e-30, +-20 and +-80 planted (as many as fit) -> (x bf16, positions of the planted values)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 8 - 4).to(BF16)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 80.0, -80.0]).to(BF16)
    k = min(n, special.numel())
    pos = torch.randperm(n, generator=g)[:k]
    x[pos] = special[:k]
    return x, pos


def tanh_ref(x):
    return torch.tanh(x.to(F64))


def check_tanh(got, x, label=""):
    """-> list of failure strings: one bf16 ulp everywhere, +-1 exactly where |x| >= 20, signed zeros kept, no NaN"""
    ref = tanh_ref(x)
    fails = []
    if got.dtype != BF16 or got.shape != x.shape:
        return [f"{label}: dtype / shape {got.dtype} {tuple(got.shape)}"]
    if bool(torch.isnan(got.float()).any()):
        fails.append(f"{label}: NaN in the output")
    bad = outside_ulp(got, ref, BF16)
    worst = float(((got.to(F64) - ref).abs() / ulp(ref, BF16)).max())
    print(f"{label} tanh: worst |got - ref| {worst:.3f} bf16 ulp")
    if bool(bad.any()):
        fails.append(f"{label}: {int(bad.sum())} elements further than one bf16 ulp, worst {worst:.3f}")
    xf, gf = x.float(), got.float()
    sat = xf.abs() >= 20
    if not torch.equal(gf[sat], torch.sign(xf[sat])):
        fails.append(f"{label}: |x| >= 20 does not give exactly +-1")
    zero = xf == 0
    if not (torch.equal(gf[zero], xf[zero]) and torch.equal(torch.signbit(gf[zero]), torch.signbit(xf[zero]))):
        fails.append(f"{label}: a zero lost its sign or value")
    return fails


def tanh_bwd_values(n, seed):
    """t: bf16 uniform in (-1, 1) with +-1 and 0 planted; dh: bf16 N(0, 1) -> (dh, t, positions of t = +-1)"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.rand(n, generator=g) * 1.98 - 0.99).to(BF16)
    dh = torch.randn(n, generator=g).to(BF16)
    special = torch.tensor([1.0, -1.0, 0.0]).to(BF16)
    k = min(n, special.numel())
    pos = torch.randperm(n, generator=g)[:k]
    t[pos] = special[:k]
    return dh, t, pos[:min(k, 2)]


def tanh_bwd_ref(dh, t):
    """from the SAVED OUTPUT t"""
    t64 = t.to(F64)
    return dh.to(F64) * (1.0 - t64 * t64)


def check_tanh_bwd(got, dh, t, label=""):
    ref = tanh_bwd_ref(dh, t)
    fails = []
    if got.dtype != BF16 or got.shape != dh.shape:
        return [f"{label}: dtype / shape {got.dtype} {tuple(got.shape)}"]
    bad = outside_ulp(got, ref, BF16)
    nz = ref != 0
    worst = float(((got.to(F64) - ref).abs()[nz] / ulp(ref, BF16)[nz]).max()) if bool(nz.any()) else 0.0
    print(f"{label} tanh backward: worst |got - ref| {worst:.3f} bf16 ulp")
    if bool(bad.any()):
        fails.append(f"{label}: {int(bad.sum())} elements further than one bf16 ulp, worst {worst:.3f}")
    one = t.float().abs() == 1
    if bool((got.float()[one] != 0).any()):
        fails.append(f"{label}: t = +-1 does not give exactly 0")
    return fails


# ------------------------------------------------------------------------------------------------ the (c p1 p2) shuffle and the L1 tail
def conv_shuffle(y, B, G, p, c):
    """[B*G*G, c*p*p] -> [B, c, G*p, G*p]: 'b (h w) (c p1 p2) -> b c (h p1) (w p2)', the layout nn.ConvTranspose2d(dim, c, p, p) writes"""
    return y.view(B, G, G, c, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, c, G * p, G * p)


def l1_index(B, G, p, c, order="cp1p2"):
    """for every image element [B, c, H, W]: (token row, token column); order 'p1p2c': the planted mistake (tokenizer.pixel_shuffle_tokens)"""
    H = G * p
    b, ch, h, w = torch.meshgrid(torch.arange(B), torch.arange(c), torch.arange(H), torch.arange(H), indexing="ij")
    gh, p1, gw, p2 = h // p, h % p, w // p, w % p
    row = b * G * G + gh * G + gw
    col = (ch * p + p1) * p + p2 if order == "cp1p2" else (p1 * p + p2) * c + ch
    return row, col


def l1_inputs(B, G, p, c, seed, dtype=F32, ties=300):
    """tokens ~ N(0.5, 0.5) in dtype; images ~ U(0, 1) with up to `ties` pixels overwritten by the float value of the token element that
    maps to them (exact ties); g_image ~ N(0, 1) / N -> (tokens, images, g_image, tie mask [B, c, H, W])"""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B * G * G, p * p * c, generator=g) * 0.5 + 0.5).to(dtype)
    img = torch.rand(B, c, G * p, G * p, generator=g)
    g_img = torch.randn(B, c, G * p, G * p, generator=g) / img.numel()
    n = img.numel()
    pick = torch.randperm(n, generator=g)[:min(ties, n // 4)]
    tie = torch.zeros(n, dtype=torch.bool)
    tie[pick] = True
    tie = tie.view(img.shape)
    row, col = l1_index(B, G, p, c)
    img = torch.where(tie, y.float()[row, col], img)
    return y, img, g_img, tie


def l1_ref(y, img, G, p, g_loss=1.0, g_img=None):
    """float64: loss = mean |float(y)[row, col] - img|, recon = float(y) in image layout, dy = g sign(diff) / N + g_image in token layout"""
    B, c = img.shape[:2]
    row, col = l1_index(B, G, p, c)
    y64 = y.to(F64)
    recon = y64[row, col]
    diff = recon - img.to(F64)
    dimg = float(g_loss) * torch.sign(diff) / img.numel()
    if g_img is not None:
        dimg = dimg + g_img.to(F64)
    dy = torch.zeros_like(y64)
    dy[row, col] = dimg
    return {"loss": diff.abs().mean(), "recon": recon, "dy": dy, "N": img.numel(), "index": (row, col)}


def l1_torch(y, img, G, p, dtype=F32):
    """torch's own evaluation of (conv_shuffle(float(tokens)) - images).abs().mean(): the fp32 yardstick of the loss bound"""
    B, c = img.shape[:2]
    return {"loss": (conv_shuffle(y.to(dtype), B, G, p, c) - img.to(dtype)).abs().mean()}


L1_BUGS = ("p1p2c_order", "sign0_is_1", "mean_tokens", "no_g_image")


def l1_standin32(y, img, G, p, g_loss=1.0, g_img=None, bug=None):
    """what the two kernels compute, in torch fp32 (the gradient sum in float64, rounded once, as the kernel forms it); bug: one of L1_BUGS"""
    B, c = img.shape[:2]
    row, col = l1_index(B, G, p, c, "p1p2c" if bug == "p1p2c_order" else "cp1p2")
    y32 = y.to(F32)
    recon = y32[row, col]
    diff = recon - img
    count = B * G * G if bug == "mean_tokens" else img.numel()
    s = torch.sign(diff)
    if bug == "sign0_is_1":
        s = torch.where(diff == 0, torch.ones_like(s), s)
    dimg = s.to(F64) * (float(g_loss) / count)
    if g_img is not None and bug != "no_g_image":
        dimg = dimg + g_img.to(F64)
    dy = torch.zeros(y.shape, dtype=F32)
    dy[row, col] = dimg.to(F32)
    return {"loss": diff.abs().sum() / count, "recon": recon, "dy": dy.to(y.dtype)}


def check_l1(got, ref, t32, tie, g_img, dtype, label=""):
    """got: any of loss, recon, dy -> list of failure strings; prints every figure"""
    fails = []
    if "loss" in got:
        e, e32 = _dist(got["loss"].reshape(1), ref["loss"].reshape(1)), _dist(t32["loss"].reshape(1), ref["loss"].reshape(1))
        b = bound(e32)
        print(f"{label} loss: {e:.3e} (torch fp32 {e32:.3e}, bound {b:.3e})")
        if not e <= b:
            fails.append(f"{label} loss: {e:.3e} > {b:.3e}")
    if "recon" in got:
        if got["recon"].dtype != F32 or not torch.equal(got["recon"].to(F64), ref["recon"]):
            fails.append(f"{label} image: not the shuffled tokens")
    if "dy" in got:
        dy = got["dy"]
        if dy.dtype != dtype:
            fails.append(f"{label} gradient: dtype {dy.dtype}")
        bad = outside_ulp(dy, ref["dy"], dtype)
        nz = ref["dy"] != 0
        worst = float(((dy.to(F64) - ref["dy"]).abs()[nz] / ulp(ref["dy"], dtype)[nz]).max())
        print(f"{label} gradient: worst |got - ref| {worst:.3f} ulp of {dtype}")
        if bool(bad.any()):
            fails.append(f"{label} gradient: {int(bad.sum())} elements further than one ulp, worst {worst:.3f}")
        row, col = ref["index"]
        at_tie = dy.to(F64)[row, col][tie]
        want = (torch.zeros_like(at_tie) if g_img is None else g_img.to(dtype).to(F64)[tie])
        if not torch.equal(at_tie, want):
            fails.append(f"{label} gradient: {int((at_tie != want).sum())} of {int(tie.sum())} ties are not exactly g_image")
    return fails


# (B, G, p, c) of the kernel cases; patch 2 (a 12-feature row) is a case of its own.  The last cuts its grid row into strips: 8 + 1 tokens
# in bf16 (6 KiB each), 4 + 4 + 1 in fp32
L1_SHAPES = [(3, 2, 4, 3), (3, 3, 8, 3), (3, 1, 16, 3), (1, 9, 32, 3)]


# ------------------------------------------------------------------------------------------------ the MLP
def tanh_mlp_ref(x, w1, b1, w2, b2, g):
    """float64 forward and the five gradients of fc2(tanh(fc1(x))) at upstream gradient g, on the operands as given (the test rounds
    them to bf16 first) -> dict y, dx, dw1, db1, dw2, db2"""
    x, w1, b1, w2, b2 = (t.detach().to(F64).clone().requires_grad_(True) for t in (x, w1, b1, w2, b2))
    y = torch.tanh(x @ w1.t() + b1) @ w2.t() + b2
    y.backward(g.to(F64))
    return {"y": y.detach(), "dx": x.grad, "dw1": w1.grad, "db1": b1.grad, "dw2": w2.grad, "db2": b2.grad}
