"""Host-side checks of the kept-row path (no GPU): the new C-ABI names, the split rule for a short reduction, argument checking."""

import pytest
import torch

import _abi

NEW_SYMBOLS = ("vitamd_layernorm_fwd_keep", "vitamd_layernorm_bwd_keep", "vitamd_attention_keep_forms", "vitamd_attention_fwd_keep",
               "vitamd_attention_bwd_keep")


def test_new_entry_points_are_in_header_and_binding():
    from vitamd import lib
    for name in NEW_SYMBOLS:
        assert _abi.declared()[1].get(name) == "int", name
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION == 9          # additive: the version does not move


def test_keep_forms_rule():
    from vitamd import lib
    L = lib.load()
    forms = L.vitamd_attention_keep_forms
    assert forms(197, 1) == 3 and forms(197, 33) == 3 and forms(197, 128) == 3
    assert forms(197, 129) == 1                      # more than four query tiles: no kept backward
    assert forms(256, 1) == 1 and forms(64, 1) == 2 and forms(224, 32) == 3
    assert forms(5, 1) == 0 and forms(288, 32) == 0
    assert forms(197, 0) == 0 and forms(197, 198) == 0


def test_tn_splits_rule_for_a_short_reduction(monkeypatch):
    from vitamd import functions as F, ops
    monkeypatch.setattr(F.SIDE, "enabled", True)
    monkeypatch.setattr(F, "TN_TARGET_WGS", None)
    monkeypatch.setattr(ops, "NT_PERSISTENT", True)
    dW = torch.empty(768, 3072)                      # 36 tiles, 252 workgroups wanted: 7 splits on a long reduction
    assert F._tn_splits(dW) == 7 and F._tn_splits(dW, 50432) == 7
    assert F._tn_splits(dW, 256) == 4                # one 64-row step per split at the most
    assert F._tn_splits(dW, 70) == 2 and F._tn_splits(dW, 64) == 1 and F._tn_splits(dW, 2) == 1
    for R in (1, 2, 63, 64, 65, 128, 200, 256):
        assert 1 <= F._tn_splits(dW, R) <= min(4, (R + 63) // 64)
    monkeypatch.setattr(F.SIDE, "enabled", False)
    assert F._tn_splits(dW, 256) == 0                # no side stream: the kernel's own rule (it caps at the step count itself)


def test_keep_rows_takes_the_old_path_where_it_must():
    from vitamd import functions as F
    assert F.KEEP_ROWS is True
    assert F.keep_rows(1, 197, False, 0.0, 0.0) == 1
    assert F.keep_rows(None, 197, False, 0.0, 0.0) is None
    assert F.keep_rows(197, 197, False, 0.0, 0.0) is None and F.keep_rows(300, 197, False, 0.0, 0.0) is None
    assert F.keep_rows(1, 197, True, 0.0, 0.0) is None
    assert F.keep_rows(1, 197, False, 0.1, 0.0) is None and F.keep_rows(1, 197, False, 0.0, 0.1) is None


@pytest.mark.parametrize("bad", [0, -1, 1.5, True])
def test_transformer_forward_rejects_a_bad_keep(bad):
    import transformer as T
    m = T.Transformer(T.TransformerConfig(n_layers=1, n_heads=1, n_embd=64, block_size=8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 8, 64), keep=bad)           # raised before any device is looked at


def test_transformer_forward_keep_at_or_beyond_the_sequence_is_the_old_path(monkeypatch):
    import transformer as T
    seen = []
    monkeypatch.setattr(T.TransformerStackFn, "apply", staticmethod(lambda x, h, c, pa, pm, keep, *params: seen.append(keep) or x))
    m = T.Transformer(T.TransformerConfig(n_layers=1, n_heads=1, n_embd=64, block_size=8))
    x = torch.zeros(1, 8, 64)
    m(x); m(x, keep=8); m(x, keep=9); m(x, keep=3)
    assert seen == [None, None, None, 3]
