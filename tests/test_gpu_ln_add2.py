"""The two-addend / store-free forms of the LayerNorm forward (functions.STREAM_ONCE) against the kernels they replace,
run one after the other on the same inputs.  Everything is torch.equal: the per-row arithmetic keeps its order - s = fl(x + add1), then
s = fl(s + add2), then the same statistics and normalisation - so the sums, y, mean and rstd are the same bits, and a stack computes the same
loss, output and gradients with the switch on and off."""
import pytest
import torch

import _poison as P
import weights as W

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
EPS = 1e-5
WIDTHS = [256, 768, 1024, 320]            # three register-resident widths and one for the generic kernels
ROWS = [1, 5, 4 * 3 + 1]                  # one wave, more than one workgroup (4 rows each), a ragged last workgroup
KEPT = [(2, 5, 1), (3, 7, 2), (2, 4, 4)]  # (B, seq, keep); keep == seq: every row kept


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _outputs(M, D, store):
    """caller-owned outputs, poisoned: an element the kernel leaves out cannot equal the reference"""
    return (P.poison_(torch.empty((M, D), dtype=F32, device=DEV)) if store else None, P.poison_(torch.empty((M, D), dtype=BF16, device=DEV)),
            P.poison_(torch.empty((M,), dtype=F32, device=DEV)), P.poison_(torch.empty((M,), dtype=F32, device=DEV)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same(got, want, store):
    xs, y, mean, rstd = got
    xs_w, y_w, mean_w, rstd_w = want
    assert torch.equal(y, y_w) and torch.equal(mean, mean_w) and torch.equal(rstd, rstd_w)
    if store:
        assert torch.equal(xs, xs_w)
    else:
        assert xs is None


# ------------------------------------------------------------------------------------------ 1. the C entry point, every combination
@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("D", WIDTHS)
def test_add2_equals_the_existing_kernels_one_after_the_other(hip, D, M, store, second):
    from vitamd import ops
    x = randn((M, D), 1, 2.0).to(DEV)
    add1 = randn((M, D), 2).to(DEV, BF16)
    add2 = randn((M, D), 3).to(DEV, BF16) if second else None
    want = ops.layernorm_fwd(x, addend=add1)
    if second:
        want = ops.layernorm_fwd(want[0], addend=add2)
    got = _outputs(M, D, store)
    assert hip.vitamd_layernorm_fwd_add2(x.data_ptr(), add1.data_ptr(), _ptr(add2), _ptr(got[0]), got[1].data_ptr(), got[2].data_ptr(),
                                         got[3].data_ptr(), M, D, EPS, _stream()) == 0
    _same(got, want, store)
    # ... and the host wrapper, whose route the layer takes
    _same(ops.layernorm_fwd(x, addend=add1, addend2=add2, store=store), want, store)


# ------------------------------------------------------------------------------------------ 2. the kept-row form
@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("B,seq,keep", KEPT)
@pytest.mark.parametrize("D", WIDTHS)
def test_keep_add2_equals_the_existing_kernels_one_after_the_other(hip, D, B, seq, keep, store):
    from vitamd import ops
    M, Mk = B * seq, B * keep
    x = randn((M, D), 4, 2.0).to(DEV)
    add1 = randn((M, D), 5).to(DEV, BF16)
    add2 = randn((Mk, D), 6).to(DEV, BF16)
    x0 = ops.layernorm_fwd(x, addend=add1)[0]
    want = ops.layernorm_fwd_keep(x0, add2, B, seq, keep)
    got = _outputs(Mk, D, store)
    assert hip.vitamd_layernorm_fwd_keep_add2(x.data_ptr(), add1.data_ptr(), add2.data_ptr(), _ptr(got[0]), got[1].data_ptr(), got[2].data_ptr(),
                                              got[3].data_ptr(), B, seq, keep, D, EPS, _stream()) == 0
    _same(got, want, store)
    if store:
        _same(ops.layernorm_fwd_keep(x, add2, B, seq, keep, pending=add1), want, True)


# ------------------------------------------------------------------------------------------ 3. a stack, the switch on against off
@pytest.mark.parametrize("keep", [None, 2])
def test_stack_same_bits_with_the_stream_stored_once(hip, keep):
    """L = 3: layer 0 has no pending addend (today's path), layers 1 and 2 take the new one; with keep the last layer's LN2 is the gather form.
    The switched-on run is repeated with every uninitialised buffer of the package poisoned."""
    import transformer as T
    from vitamd import functions as F
    L, D, H, N, B, seed = 3, 256, 4, 5, 2, 23
    m = T.Transformer(T.TransformerConfig(n_layers=L, n_heads=H, n_embd=D, block_size=N))
    m.load_state_dict(W.transformer_state(seed, "", L, D), strict=True)
    m = m.cuda()
    x0 = W.normal(seed, "x", (B, N, D))
    dy = W.normal(seed, "dy", (B, N if keep is None else keep, D))
    calls = []
    plain = F.ops.layernorm_fwd

    def counting(x, addend=None, addend2=None, store=True):
        calls.append((addend is not None, addend2 is not None, store))
        return plain(x, addend, addend2, store)

    def run():
        m.zero_grad(set_to_none=True)
        x = x0.cuda().requires_grad_(True)
        y = m(x) if keep is None else m(x, keep=keep)
        loss = (y * dy.cuda()).sum()
        loss.backward()
        torch.cuda.synchronize()
        return {"loss": loss.detach(), "y": y.detach(), "dx": x.grad, **{k: p.grad for k, p in m.named_parameters()}}

    saved = F.STREAM_ONCE
    try:
        F.ops.layernorm_fwd = counting
        F.STREAM_ONCE = True
        on = run()
        n_fwd = len(calls)
        once_calls = [c for c in calls if not c[2] or c[1]]
        F.STREAM_ONCE = False
        off = run()
        assert all(c[2] and not c[1] for c in calls[n_fwd:])
        F.STREAM_ONCE = True
        with P.poisoned():
            dirty = run()
    finally:
        F.STREAM_ONCE = saved
        F.ops.layernorm_fwd = plain
    # layers 1 and 2: a store-free LN1 each; LN2 with two addends in layer 1, and in layer 2 unless it is the kept-row form
    assert once_calls.count((True, False, False)) == 2 and once_calls.count((True, True, True)) == (2 if keep is None else 1)
    assert on.keys() == off.keys() == dirty.keys() and len(on) == 3 + 6 * L
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert not P.compare(on, dirty, exact=set(on))
