"""Single-query attention over the KV cache and the K/V append at every split edge, on a real MI355X, through the C ABI (vitamd.lib.load()),
so that the test owns the workspace: it is exactly vitamd_decode_attention_ws_bytes long and filled with NaN before every call, and a
combine pass that read one partial too many would show.

Spike cases (tests/_decode_ref.py): one key dominates so far that every other softmax weight is exactly 0 in fp32; o must equal that
key's value row BIT FOR BIT in any split and merge order, at every length 1 .. 40, at every 128k - 1, 128k, 128k + 1 (a chunk is a
multiple of 128: every chunk edge of every plan, whatever the CU count), with the spike on the last key, the first key and the first key
of the last started 128-group.  The key right behind the length would win if the mask let it in; everything after it is NaN.
Random cases: each (b, h) row against the fp64 reference, held to 2 x the bf16 floor of its case (_decode_ref.random_reference: derived,
not a literal).  tests/test_decode_ref_host.py proves on the CPU that these checks reject every mutation of _decode_ref.MUTANTS.
Then *len outside the cache, vitamd_kv_append's dropped rows, the grid's last row (B*H = 65535) and a stack decoded from an empty cache."""
import pytest
import torch

import _decode_ref as R
import _gemm_ref as G
from _gemm_ref import BF16, GUARD

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = 1, 2
WS_PER_CHUNK = 66 * 4                          # bytes per (b, h, chunk): 64 weighted-V sums, the max and the sum


def _st():
    return torch.cuda.current_stream().cuda_stream


def _plan(hip, B, H, Lmax):
    """-> (ws_bytes, nch) as the workspace size implies them"""
    ws_bytes = hip.vitamd_decode_attention_ws_bytes(B, H, Lmax)
    assert ws_bytes >= 0 and ws_bytes % (B * H * WS_PER_CHUNK) == 0, ws_bytes
    nch = ws_bytes // (B * H * WS_PER_CHUNK) if ws_bytes else 1
    assert nch != 1 or ws_bytes == 0
    assert nch <= (Lmax + 127) // 128
    return ws_bytes, nch


class _Attn:
    """one (B, H, Lmax): the exact-size workspace, every length as a device int32, and sentinel-framed outputs"""

    def __init__(self, hip, B, H, Lmax):
        self.hip, self.B, self.H, self.Lmax = hip, B, H, Lmax
        self.ws_bytes, self.nch = _plan(hip, B, H, Lmax)
        self.ws = torch.empty((self.ws_bytes // 4,), device="cuda") if self.ws_bytes else None
        self.lens = torch.arange(-1, Lmax + 1, dtype=torch.int32, device="cuda")      # lens[i] = i - 1
        self.blank = G.sentinel(B + 2 * GUARD, H * 64, BF16).cuda()

    def __call__(self, qkv, kc, vc, length, ws_bytes=None, ws="own"):
        """-> (return code, the whole o buffer with its guard rows, on the device).  The workspace is NaN before the call."""
        o = self.blank.clone()
        if self.ws is not None:
            self.ws.fill_(float("nan"))
        wp = None if (self.ws is None or ws is None) else self.ws.data_ptr()
        code = self.hip.vitamd_decode_attention(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr() + GUARD * self.H * 64 * 2,
                                                self.lens.data_ptr() + 4 * (length + 1), self.B, self.H, 64, self.Lmax, wp,
                                                self.ws_bytes if ws_bytes is None else ws_bytes, _st())
        return code, o


def _body(o):
    """the whole o buffer (bit patterns, CPU) -> (o bf16 [B, H*64], the guard rows)"""
    return o[GUARD:-GUARD].view(BF16), torch.cat([o[:GUARD], o[-GUARD:]])


def _assert_o_untouched(what, o):
    changed = o != G.SENT16
    nan = torch.isnan(o.view(BF16).float())
    assert not bool(changed.any()), f"{what}: {int(changed.sum())} elements of o written, {int(nan.sum())} of them NaN"


# ---------------------------------------------------------------------------------------------- the workspace
ALL_SHAPES = sorted(set(R.SPIKE_TABLES) | {c[:3] for c in R.RANDOM_CASES} | {(3, 5, 96), (2, 3, 96), (2, 3, 640)})


def test_workspace_size_and_refusals(hip):
    """a workspace four bytes short or missing: VITAMD_ERR_ARG and nothing written"""
    split = 0
    for (B, H, Lmax) in ALL_SHAPES:
        a = _Attn(hip, B, H, Lmax)
        print(f"PLAN B{B} H{H} Lmax{Lmax}: ws_bytes={a.ws_bytes} nch={a.nch}")
        if not a.ws_bytes:
            continue
        split += 1
        qkv = torch.zeros((B, 3 * H * 64), dtype=BF16, device="cuda")
        kc = torch.zeros((B, H, Lmax, 64), dtype=BF16, device="cuda")
        for kw in ({"ws_bytes": a.ws_bytes - 4}, {"ws": None}):
            code, o = a(qkv, kc, kc, 0, **kw)
            torch.cuda.synchronize()
            assert code == ERR_ARG, (B, H, Lmax, kw, code)
            _assert_o_untouched(f"refused call B{B} H{H} Lmax{Lmax} {kw}", o.cpu())
        code, o = a(qkv, kc, kc, 0)
        assert code == 0
    assert split >= 1                                                            # (1, 1, 16384) is split on any part
    assert hip.vitamd_decode_attention_ws_bytes(1, 1, 16385) < 0 and hip.vitamd_decode_attention_ws_bytes(1, 1, 0) < 0


# ---------------------------------------------------------------------------------------------- spike cases
@pytest.mark.parametrize("table", R.SPIKE_TABLES, ids=lambda t: "B{}-H{}-Lmax{}".format(*t))
def test_spike_returns_the_value_row_bit_for_bit_at_every_edge(hip, table):
    B, H, Lmax = table
    a = _Attn(hip, B, H, Lmax)
    print(f"PLAN B{B} H{H} Lmax{Lmax}: ws_bytes={a.ws_bytes} nch={a.nch}")
    cases = [c for c in R.SPIKE_CASES if c[:3] == table]
    assert len(cases) > 100
    qkv0, kc0, vc0 = R.spike_base(B, H, Lmax)
    qkv, kcd, vcd = qkv0.cuda(), kc0.cuda(), vc0.cuda()
    outs = []
    for (_, _, _, n, j) in cases:                                                # queued; compared at the end
        kc, vc = R.fill_past(kcd.clone(), vcd.clone(), n, j)
        for rep in range(2):
            code, o = a(qkv, kc, vc, n - 1)
            assert code == 0, (n, j, code)
            outs.append(o)
    got = torch.stack(outs).cpu()
    failures = []
    for i, c in enumerate(cases):
        first, second = got[2 * i], got[2 * i + 1]
        o, guards = _body(first)
        bad = R.check_spike(o, vc0[:, :, c[4]])
        if bool((guards != G.SENT16).any()):
            bad.append("guard rows of o written")
        if not torch.equal(first, second):
            bad.append("the second call gave other bits")
        if bad:
            failures.append(f"{R.spike_id(c)}: " + "; ".join(bad))
    print(f"SPIKE B{B} H{H} Lmax{Lmax}: {len(cases)} cases x 2 calls, {len(failures)} failed")
    assert not failures, f"{len(failures)} of {len(cases)} cases (nch = {a.nch}):\n" + "\n".join(failures[:20])


# ---------------------------------------------------------------------------------------------- random cases
@pytest.mark.parametrize("B,H,Lmax,ns", R.RANDOM_CASES, ids=[f"B{c[0]}-H{c[1]}-Lmax{c[2]}" for c in R.RANDOM_CASES])
def test_random_rows_against_fp64_within_twice_the_floor(hip, B, H, Lmax, ns, record_property):
    a = _Attn(hip, B, H, Lmax)
    print(f"PLAN B{B} H{H} Lmax{Lmax}: ws_bytes={a.ws_bytes} nch={a.nch}")
    qkv, kcd, vcd = (t.cuda() for t in R.random_base(B, H, Lmax))
    outs = []
    for n in ns:
        kc, vc = R.fill_past(kcd.clone(), vcd.clone(), n)
        for rep in range(2):
            code, o = a(qkv, kc, vc, n - 1)
            assert code == 0, (n, code)
            outs.append(o)
    got = torch.stack(outs).cpu()
    failures = []
    for i, n in enumerate(ns):
        r = R.random_reference(B, H, Lmax, n)
        o, guards = _body(got[2 * i])
        worst, bad = R.check_random(o.float(), r)
        print(f"STAT {R.random_id(B, H, Lmax, n)} worst_row={worst:.3e} floor={r['floor']:.3e} bound={r['bound']:.3e}")
        record_property(f"worst_row_n{n}", worst)
        G.assert_untouched(f"guard rows n={n}", guards)
        assert torch.equal(got[2 * i], got[2 * i + 1]), f"n={n}: the second call gave other bits"
        failures += [f"n={n}: {b}" for b in bad]
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- *len outside the cache
@pytest.mark.parametrize("Lmax,split", [(96, False), (1000, True)])
def test_len_at_capacity_reads_nothing_past_the_cache(hip, Lmax, split):
    """*len = Lmax is clamped: the bits of *len = Lmax - 1.  NaN rows stand behind the caches, and a key read at position Lmax of any other
    (b, h) would be the next head's first row."""
    B, H = 3, 5
    a = _Attn(hip, B, H, Lmax)
    assert (a.nch > 1) == split, f"Lmax {Lmax}: nch = {a.nch}"
    qkv, kc0, vc0 = R.random_base(B, H, Lmax)
    tail = torch.full((8, 64), float("nan"), dtype=BF16)
    kc, vc = (torch.cat([c.reshape(-1, 64), tail]).cuda() for c in (kc0, vc0))
    qkv = qkv.cuda()
    code1, inside = a(qkv, kc, vc, Lmax - 1)
    code2, at_cap = a(qkv, kc, vc, Lmax)
    assert code1 == 0 and code2 == 0
    inside, at_cap = inside.cpu(), at_cap.cpu()
    o, guards = _body(inside)
    worst, bad = R.check_random(o.float(), R.random_reference(B, H, Lmax, Lmax))
    assert not bad, bad
    G.assert_untouched("guard rows", guards)
    assert not bool(torch.isnan(_body(at_cap)[0].float()).any()), "*len = Lmax read the NaN rows behind the cache"
    assert torch.equal(at_cap, inside), "*len = Lmax differs from *len = Lmax - 1"


@pytest.mark.parametrize("Lmax,split", [(96, False), (640, True)])
def test_negative_len_leaves_o_untouched_in_both_forms(hip, Lmax, split):
    B, H = 2, 3
    a = _Attn(hip, B, H, Lmax)
    assert (a.nch > 1) == split, f"Lmax {Lmax}: nch = {a.nch}"                    # the plan this case is here for
    qkv, kc, vc = (t.cuda() for t in R.random_base(B, H, Lmax))
    code, o = a(qkv, kc, vc, -1)
    assert code == 0
    _assert_o_untouched(f"*len = -1, {'split' if split else 'unsplit'} form (nch = {a.nch})", o.cpu())


# ---------------------------------------------------------------------------------------------- K/V append
# (B, T, H, Lmax, *len): two rows land and three are dropped at the end; two dropped in front; the whole cache at once; 1680 16-byte pieces
# (6.56 workgroups of 256)
APPEND_CASES = [(2, 5, 3, 40, 38), (2, 5, 3, 40, -2), (2, 40, 3, 40, 0), (3, 7, 5, 40, 11)]


def _append(hip, qkv, B, T, H, Lmax, length):
    caches = [G.sentinel(B * H * Lmax + 2 * GUARD, 64, BF16).cuda() for _ in range(2)]
    ln = torch.tensor([length], dtype=torch.int32, device="cuda")
    code = hip.vitamd_kv_append(qkv.data_ptr(), caches[0].data_ptr() + GUARD * 128, caches[1].data_ptr() + GUARD * 128, ln.data_ptr(), B, T, H, 64, Lmax,
                                _st())
    torch.cuda.synchronize()
    return code, [c.cpu() for c in caches]


@pytest.mark.parametrize("B,T,H,Lmax,length", APPEND_CASES, ids=["B{}-T{}-H{}-Lmax{}-len{}".format(*c) for c in APPEND_CASES])
def test_kv_append_drops_rows_outside_the_cache(hip, B, T, H, Lmax, length):
    qkv = R.randn_bf16((B * T, 3 * H * 64), 900 + T + length)
    code, got = _append(hip, qkv.cuda(), B, T, H, Lmax, length)
    assert code == 0
    landed = [t for t in range(T) if 0 <= length + t < Lmax]
    print(f"FORM kv_append pieces={B * T * H * 16} ragged={B * T * H * 16 % 256 != 0} rows landed per sequence={len(landed)} of {T}")
    for name, g, w in zip("kv", got, R.kv_frame(qkv, B, T, H, Lmax, length)):
        G.assert_bits_equal(f"{name} cache", g, w)


def test_kv_append_case_list_holds_the_edges():
    assert any(L + T > Lmax and L >= 0 for (_, T, _, Lmax, L) in APPEND_CASES) and any(L < 0 for (*_, L) in APPEND_CASES)
    assert any(T == Lmax and L == 0 for (_, T, _, Lmax, L) in APPEND_CASES) and any(B * T * H * 16 % 256 for (B, T, H, _, _) in APPEND_CASES)


def test_kv_append_refuses_more_rows_than_the_cache_holds(hip):
    B, H, Lmax = 2, 3, 40
    qkv = R.randn_bf16((B * (Lmax + 1), 3 * H * 64), 901)
    code, got = _append(hip, qkv.cuda(), B, Lmax + 1, H, Lmax, 0)
    assert code == ERR_SHAPE
    for g in got:
        G.assert_untouched("T = Lmax + 1", g)


# ---------------------------------------------------------------------------------------------- the grid's last row
def test_bh_65535_runs_and_65536_is_refused(hip):
    B, H, Lmax, n, j = R.SPIKE_LIMIT
    a = _Attn(hip, B, H, Lmax)
    qkv, kc, vc = R.spike_inputs(R.SPIKE_LIMIT)
    qkvd, kcd, vcd = qkv.cuda(), kc.cuda(), vc.cuda()
    code, o = a(qkvd, kcd, vcd, n - 1)
    assert code == 0
    o, guards = _body(o.cpu())
    G.assert_untouched("guard rows", guards)
    want = vc[:, :, j]
    for bh in (0, 32767, 65534):                                                  # the first, a middle and the last (b, h)
        b, h = divmod(bh, H)
        assert torch.equal(G.bits(o[b, h * 64:h * 64 + 64]), G.bits(want[b, h])), f"bh {bh}"
    assert not R.check_spike(o, want)
    # one more: VITAMD_ERR_SHAPE before anything is launched (4096 x 16; no buffer is touched)
    blank = G.sentinel(8, 64, BF16).cuda()
    code = hip.vitamd_decode_attention(qkvd.data_ptr(), kcd.data_ptr(), vcd.data_ptr(), blank.data_ptr(), a.lens.data_ptr() + 4, 4096, 16, 64, Lmax,
                                       None, 0, _st())
    torch.cuda.synchronize()
    assert code == ERR_SHAPE
    G.assert_untouched("B*H = 65536", blank.cpu())


# ---------------------------------------------------------------------------------------------- one stack
def test_stack_decoded_from_an_empty_cache_matches_full_sequence_and_oracle(hip):
    """no prefill: the first step runs at *len = 0 in every layer, and every length 1 .. 40 follows"""
    import transformer as T
    import vit_oracle as O
    import weights as W
    seed, B, S = 9, 2, 40
    cfg = T.TransformerConfig(n_layers=2, n_heads=4, n_embd=256, block_size=S, causal=True)
    sd = W.transformer_state(seed, "", cfg.n_layers, cfg.n_embd, causal_block=S)
    m = T.Transformer(cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = W.normal(seed, "x", (B, S, cfg.n_embd))
    xc = x.cuda()
    with torch.no_grad():
        y_full = m(xc).cpu()
    cache = m.new_cache(B)
    assert cache.max_len == S and cache.len == 0
    y_cached = torch.cat([m.forward_cached(xc[:, t:t + 1], cache) for t in range(S)], dim=1).cpu()
    assert cache.len == S and int(cache.len_dev.item()) == S
    y_oracle = O.transformer(x, sd, "", cfg.n_layers, cfg.n_heads, causal=True, lowp=True)
    e_full, e_cached, e_first = O.rel_l2(y_full, y_oracle), O.rel_l2(y_cached, y_oracle), O.rel_l2(y_cached[:, :1], y_oracle[:, :1])
    print(f"rel-L2 vs oracle: full {e_full:.2e}, cached {e_cached:.2e} (first position {e_first:.2e})")
    assert e_cached <= 2 * e_full + 1e-3
