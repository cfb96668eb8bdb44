"""The code-id TiTok without a GPU: the CPU reference of tests/_code_titok_ref.py against the reference's golden (so that the GPU tests
compare against something validated here), the module's keys, shapes and arithmetic, and the refusals of the new ops - CPU tensors and
bad arguments at the Python surface, bad shapes and missing pointers at the C entry points, all before any device work."""
import ctypes
import os

import pytest
import torch

import _abi
import _code_titok_ref as C
import vit_oracle as O
from conftest import ROOT, load_golden

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ERR_SHAPE, ERR_ARG = 1, 2
NEW_SYMBOLS = ("vitamd_assemble_tokens_grid_cap", "vitamd_assemble_tokens_fwd", "vitamd_assemble_tokens_bwd")


def _err(got, ref):
    if "full" in ref:
        return O.rel_l2(got, ref["full"])
    return O.rel_l2(got.detach().flatten()[::997].float(), ref["sample"])


# ------------------------------------------------------------------------------------------------ the references
def test_cpu_reference_reproduces_the_golden():
    """fp32 on the CPU both times, composed differently: the bounds of tests/test_oracle.py for the tokenizers (outputs 1e-5, gradients
    2e-4), the ids equal, the losses to 1e-5"""
    g = load_golden("llamagen_titok_tiny.pt")
    sd, ids = C.golden_case(g)
    r = C.model_loss_and_grads(ids, sd, g["cfg"])
    assert torch.equal(r["indices"], g["indices"])
    assert O.rel_l2(r["latents"], g["latents"]) < 1e-5
    assert _err(r["logits"], g["logits"]) < 1e-5
    assert torch.equal(r["logits"].argmax(-1), g["argmax"])
    assert abs(r["quantize_loss"] - g["quantize_loss"]) < 1e-5 and abs(r["recon_loss"] - g["recon_loss"]) < 1e-5
    assert abs(r["loss"] - g["loss"]) < 1e-5
    assert sorted(r["grads"]) == sorted(g["grads"])
    for k, ref in g["grads"].items():
        assert ref["norm"] > 0.0, k
        assert _err(r["grads"][k], ref) < 2e-4, k
    with torch.no_grad():
        from_idx = C.decode(sd["quant.codebook.weight"][g["indices"]], sd, g["cfg"])
    assert _err(from_idx, g["logits_from_indices"]) < 1e-5


def test_golden_holds_summaries_only_and_records_its_seed_choice():
    g = load_golden("llamagen_titok_tiny.pt")                                  # weights_only=True: tensors and plain containers
    c, floor = g["cfg"], g["ref_bf16_floor"]
    assert (c["vq_codebook_size"], c["vq_latent_tokens"], c["latent_tokens"], c["codebook_size"], c["latent_dim"], c["transformer"], c["batch"]) \
        == (64, 16, 16, 32, 12, "S", 4)
    assert floor["index_agreement"] >= 0.9
    assert set(floor["grads"]) == set(g["grads"]) == set(k for k in g["state_keys"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "llamagen_titok_tiny.pt")) < 1 << 20
    assert not any(k in g for k in ("state_dict", "weights"))


def test_assembly_reference_is_the_autograd_of_the_torch_expression():
    """float64 autograd through cat / expand / embedding against assemble_grads_ref, both modes, E = 0 included, ids out of range skipped"""
    gen = torch.Generator().manual_seed(5)
    for B, E, S, D, rows, pos_rows in ((2, 3, 5, 8, 7, 6), (3, 0, 4, 4, 5, 4)):
        prefix, pos, tok, body = (torch.randn(n, D, generator=gen, dtype=F64).requires_grad_(True) for n in (E, pos_rows, rows, B * S))
        ids = torch.randint(0, rows, (B, S), generator=gen)
        up = torch.randn(B, E + S, D, generator=gen, dtype=F64)
        x = C.assemble_ref(prefix, pos, ids=ids, tok=tok)
        assert x.shape == (B, E + S, D)
        (x * up).sum().backward()
        bad = ids.clone()
        bad[0, 0] = rows                                                       # out of range: drop its term from the autograd result
        ref, ref_bad = C.assemble_grads_ref(up, E, pos_rows, ids, rows), C.assemble_grads_ref(up, E, pos_rows, bad, rows)
        assert torch.allclose(prefix.grad, ref["dprefix"]) and torch.allclose(pos.grad, ref["dpos"]) and torch.allclose(tok.grad, ref["dtok"])
        want = tok.grad.clone()
        want[ids[0, 0]] -= up[0, E]
        assert torch.allclose(want, ref_bad["dtok"]) and int(ref_bad["n_tok"].sum()) == B * S - 1
        assert torch.equal(ref["n_tok"], torch.bincount(ids.reshape(-1), minlength=rows))
        prefix.grad = pos.grad = None
        xb = C.assemble_ref(prefix, pos, body=body.view(B, S, D))
        (xb * up).sum().backward()
        dense = C.assemble_grads_ref(up, E, pos_rows)
        assert torch.allclose(prefix.grad, dense["dprefix"]) and torch.allclose(pos.grad, dense["dpos"]) and "dtok" not in dense
        assert torch.allclose(body.grad.view(B, S, D), up[:, E:])
        g32 = up.float()
        assert torch.allclose(C.batch_sum_f32(g32[:, E:]).double(), ref["dpos"][:S], atol=1e-5)
        assert bool((C.dtok_allowance(ref) >= 0).all())


# ------------------------------------------------------------------------------------------------ the module
def test_state_keys_shapes_and_config_arithmetic():
    import train_llamagen_titok as T
    g = load_golden("llamagen_titok_tiny.pt")
    c = g["cfg"]
    cfg = T.TiTokConfig(c["vq_codebook_size"], c["vq_latent_tokens"], c["latent_tokens"], c["codebook_size"], c["latent_dim"], c["transformer"])
    assert cfg.trans_config.block_size == c["vq_latent_tokens"] + c["latent_tokens"] == c["block_size"] and cfg.n_embd == c["n_embd"] == 512
    assert cfg.trans_config.dropout == 0.0 and not cfg.trans_config.causal
    torch.manual_seed(0)
    m = T.TiTok(cfg)
    assert m.block_size == 32 and m.enc.latent_tokens == 16 and m.dec.config is cfg and m.config is cfg
    assert sorted(m.state_dict().keys()) == g["state_keys"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == g["state_shapes"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    keys = set(m.state_dict())
    for k in ("enc.tok_emb.weight", "enc.pos_emb", "enc.extra_emb.weight", "enc.proj.weight", "quant.codebook.weight", "dec.pos_emb",
              "dec.quant_proj.bias", "dec.emb_proj.weight", "dec.mask_tokens.weight", "enc.transformer.layers.0.multi_attn.qkv.weight",
              "dec.transformer.layers.5.mlp.2.bias"):
        assert k in keys, k
    # the initialisation rule: Linear and Embedding weights ~ trunc_normal(0, 0.02) - the codebook too, whose uniform +-1/K draw would
    # stay within 1/32 with a standard deviation of 0.018 - biases zero; the pos_emb Parameters keep randn * n_embd^-0.5 (std 0.044)
    for k, p in m.state_dict().items():
        if k.endswith("bias"):
            assert not bool(p.any()), k
        elif k.endswith("pos_emb"):
            assert 0.035 < float(p.std()) < 0.055, k
        else:
            assert 0.015 < float(p.std()) < 0.025, k
    assert float(m.quant.codebook.weight.detach().abs().max()) > 1.0 / 32


def test_parse_args_gives_the_reference_defaults():
    import train_llamagen_titok as T
    a = T.parse_args([])
    assert (a.vq_codebook_size, a.vq_latent_tokens, a.latent_tokens, a.codebook_size, a.latent_dim, a.transformer, a.bs) \
        == (16384, 256, 256, 16384, 12, "S", 32)
    assert (a.lr, a.weight_decay, a.warmup_steps, a.train_steps) == (1e-4, 1e-4, 5000, 1_000_000)
    assert a.max_grad_norm is None and a.vq == "none"
    assert T.parse_args(["--vq", "vitvqgan", "--max_grad_norm", "1.0"]).vq == "vitvqgan"
    with pytest.raises(SystemExit):
        T.parse_args(["--vq", "llamagen"])
    for name in ("TiTokConfig", "TiTokEncoder", "Quantizer", "TiTokDecoder", "TiTok", "train_step", "make_optim", "codes_from", "main"):
        assert hasattr(T, name), name
    assert "clip" in T.train_step.__doc__


def test_codes_from_refuses_what_is_not_a_batch_of_ids():
    import train_llamagen_titok as T

    class Enc:
        def __init__(self, out):
            self.out = out

        def encode(self, images):
            return self.out
    ids = torch.arange(6).view(2, 3)
    assert torch.equal(T.codes_from(Enc(ids.t()), None), ids.t()) and T.codes_from(Enc(ids.t()), None).is_contiguous()
    for bad in (ids.int(), ids.reshape(-1), (ids, {})):
        with pytest.raises(TypeError):
            T.codes_from(Enc(bad), None)


# ------------------------------------------------------------------------------------------------ the library and its wrappers
def test_symbols_are_exported_typed_and_in_the_header():
    from vitamd import lib, ops
    L = lib.load()
    header = _abi.header()
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES and f"int {name}(" in header
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert len(lib.SIGNATURES["vitamd_assemble_tokens_fwd"]) == 13 and len(lib.SIGNATURES["vitamd_assemble_tokens_bwd"]) == 12
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION                       # additive: the version does not move
    assert ops.assemble_tokens_grid_cap() == L.vitamd_assemble_tokens_grid_cap() >= 256


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; nothing is launched"""
    from vitamd import lib
    L = lib.load()
    one = ctypes.c_void_p(16)            # a non-null pointer that is never followed: every call below returns before its launch

    def fwd(B, E, S, D, tok_rows, pos_rows, prefix=None, pos=None, tok=None, ids=None, body=None, x=None):
        return L.vitamd_assemble_tokens_fwd(prefix, pos, tok, ids, body, x, B, E, S, D, tok_rows, pos_rows, None)

    def bwd(B, E, S, D, tok_rows, pos_rows, g=None, ids=None, dprefix=None, dpos=None, dtok=None):
        return L.vitamd_assemble_tokens_bwd(g, ids, dprefix, dpos, dtok, B, E, S, D, tok_rows, pos_rows, None)
    for B, E, S, D, pos_rows in ((2, 1, 8, 6, 8), (2, 1, 8, 2, 8), (2, 1, 9, 8, 8), (0, 1, 8, 8, 8), (2, -1, 8, 8, 8), (2, 1, 0, 8, 8), (2, 0, 0, 8, 8)):
        assert fwd(B, E, S, D, 10, pos_rows) == ERR_SHAPE, (B, E, S, D, pos_rows)
        assert bwd(B, E, S, D, 10, pos_rows) == ERR_SHAPE, (B, E, S, D, pos_rows)
    assert fwd(2, 1, 8, 8, 0, 8, tok=one, ids=one) == ERR_SHAPE and bwd(2, 1, 8, 8, 0, 8, ids=one, dtok=one) == ERR_SHAPE   # a table without rows
    assert fwd(2, 1, 8, 8, 10, 8) == ERR_ARG and bwd(2, 1, 8, 8, 10, 8) == ERR_ARG and fwd(1, 0, 1, 4, 1, 1) == ERR_ARG
    assert fwd(2, 1, 8, 8, 10, 8, prefix=one, pos=one, x=one) == ERR_ARG                                  # no source
    assert fwd(2, 1, 8, 8, 10, 8, prefix=one, pos=one, x=one, tok=one, ids=one, body=one) == ERR_ARG      # both sources
    assert fwd(2, 1, 8, 8, 10, 8, prefix=one, pos=one, x=one, tok=one) == ERR_ARG                         # a table without ids
    assert fwd(2, 1, 8, 8, 10, 8, pos=one, x=one, body=one) == ERR_ARG                                    # E > 0 without a prefix
    assert bwd(2, 1, 8, 8, 10, 8, g=one, dpos=one, dprefix=one, ids=one) == ERR_ARG                       # ids without dtok
    assert bwd(2, 1, 8, 8, 10, 8, g=one, dpos=one) == ERR_ARG                                             # E > 0 without dprefix
    assert bwd(2, 1, 8, 8, 10, 8, g=one, dprefix=one, dtok=one, ids=one) == ERR_ARG                       # no dpos


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    """CPU tensors: VitamdError from every op; dtypes and shapes are looked at before the device, so the bad arguments are named here,
    without a GPU, and on a GPU machine before anything is launched"""
    from vitamd import lm, ops
    from vitamd.lib import VitamdError
    B, E, S, D, rows = 2, 3, 5, 8, 7
    prefix, pos, tok, body = torch.randn(E, D), torch.randn(S, D), torch.randn(rows, D), torch.randn(B, S, D)
    ids, g = torch.zeros(B, S, dtype=torch.long), torch.randn(B, E + S, D)
    dev = "expected a ROCm device tensor"
    for call in (lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids, tok_table=tok),
                 lambda: ops.assemble_tokens_fwd(prefix, pos, body=body),
                 lambda: ops.assemble_tokens_fwd(None, pos, body=body),
                 lambda: ops.assemble_tokens_bwd(g, torch.zeros(E, D), torch.zeros(S, D), ids=ids, dtok=torch.zeros(rows, D)),
                 lambda: ops.assemble_tokens_bwd(g, torch.zeros(E, D), torch.zeros(S, D)),
                 lambda: lm.prefixed_token_embed(ids, tok, pos, prefix),
                 lambda: lm.prefixed_rows(body, pos, prefix),
                 lambda: lm.prefixed_rows(body.bfloat16(), pos, prefix)):
        with pytest.raises(VitamdError, match=dev):
            call()
    cases = {
        "ids: expected a 2-d torch.int64": lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids.int(), tok_table=tok),
        "tok_table: expected a 2-d torch.float32": lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids, tok_table=tok.double()),
        "body: expected a 3-d torch.float32": lambda: ops.assemble_tokens_fwd(prefix, pos, body=body.bfloat16()),
        "prefix: expected a 2-d torch.float32": lambda: ops.assemble_tokens_fwd(prefix.half(), pos, body=body),
        "g: expected a 3-d torch.float32": lambda: ops.assemble_tokens_bwd(g.view(-1, D), torch.zeros(E, D), torch.zeros(S, D)),
        "share D": lambda: ops.assemble_tokens_fwd(torch.randn(E, D + 4), pos, body=body),                      # prefix width
        "share D with": lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids, tok_table=torch.randn(rows, D + 4)),   # table width
        "D % 4 == 0": lambda: ops.assemble_tokens_fwd(torch.randn(E, 6), torch.randn(S, 6), body=torch.randn(B, S, 6)),
        "pos_rows >= S": lambda: ops.assemble_tokens_fwd(prefix, pos[: S - 1], body=body),
        "positions \\(pos_rows >= S\\)": lambda: ops.assemble_tokens_bwd(g, torch.zeros(E, D), torch.zeros(S - 1, D)),
        "do not fit": lambda: ops.assemble_tokens_bwd(g, torch.zeros(E + 1, D), torch.zeros(S, D), ids=ids, dtok=torch.zeros(rows, D)),
        "either ids with a token table or a dense body": lambda: ops.assemble_tokens_fwd(prefix, pos, ids=ids, tok_table=tok, body=body),
        "either ids with a token table": lambda: ops.assemble_tokens_fwd(prefix, pos),
        "go together": lambda: ops.assemble_tokens_bwd(g, torch.zeros(E, D), torch.zeros(S, D), ids=ids),
        "ids must be int64 \\[B, S\\]": lambda: lm.prefixed_token_embed(ids.reshape(-1), tok, pos, prefix),
        "body must be fp32 or bf16": lambda: lm.prefixed_rows(body.double(), pos, prefix),
    }
    for msg, call in cases.items():
        with pytest.raises(VitamdError, match=msg):
            call()
