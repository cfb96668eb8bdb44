"""KV-cached forward of a causal transformer stack: prefill a prompt once, then one token per sequence per call.

The reference samples its causal Transformer without a cache (train_videogpt.py:56-65): every new token re-runs the whole stack over
the whole prefix.  Here each layer keeps its K and V rows; a decode step runs LN1 -> QKV -> K/V append -> single-query attention
over the cache -> residual + LN2 -> fc1 + GELU -> fc2 + residual per layer, with the skinny-M GEMM (weights streamed once) for the
Linears; the QKV GEMM's epilogue writes the K/V rows itself.  The prefill is the existing full causal path (the same kernels as Transformer.forward) plus the append.

Same dtype flow as the training path (vitamd/functions.py): fp32 residual stream and LayerNorm statistics, bf16 GEMM / attention
operands, the bf16 weights of functions.WEIGHTS.  A no-grad forward; autocast neither changes nor is needed by it.
"""
from __future__ import annotations

import torch

from . import ops
from .functions import WEIGHTS, _f32c
from .lib import VitamdError

BF16, F32 = torch.bfloat16, torch.float32


class KVCache:
    """Per-layer K / V buffers bf16 [n_layers, B, H, Lmax, 64] (each layer's [B, H, Lmax, 64] is contiguous), the number of positions
    held as a device int32 (`len_dev`, read by the kernels: no host synchronisation per step) and its host mirror `len` (bounds checks)."""

    def __init__(self, n_layers, batch, n_heads, max_len, device):
        if not 1 <= max_len <= ops.DECODE_MAX_LEN:
            raise ValueError(f"KVCache: max_len must be in [1, {ops.DECODE_MAX_LEN}], got {max_len}")
        device = torch.device(device)
        if device.type != "cuda":
            raise VitamdError("KVCache: expected a ROCm device (the HIP kernels are the only implementation)")
        self.n_layers, self.batch, self.n_heads, self.max_len = n_layers, batch, n_heads, max_len
        self.k = torch.empty((n_layers, batch, n_heads, max_len, 64), dtype=BF16, device=device)
        self.v = torch.empty_like(self.k)
        self.len_dev = torch.zeros((1,), dtype=torch.int32, device=device)
        self.len = 0

    @property
    def device(self):
        return self.k.device

    def reset(self):
        """Forget every position (the buffers are kept)."""
        self.len_dev.zero_()
        self.len = 0

    def _advance(self, T):
        self.len_dev.add_(T)            # a device op, ordered after this step's kernels on the current stream
        self.len += T


def check_decodable(model):
    if not model.causal:
        raise ValueError("KV-cached decoding needs a causal Transformer (TransformerConfig(causal=True))")
    if model.dropout > 0:
        raise ValueError(f"KV-cached decoding does not support dropout > 0 (got {model.dropout}): the reference applies SDPA dropout even "
                         "in eval mode (transformer.py:28), which a cache cannot reproduce; use the uncached path")
    if model.n_embd // model.n_heads != 64 or model.n_embd % model.n_heads:
        raise ValueError("KV-cached decoding supports head_dim 64 only")


def new_cache(model, batch, max_len=None, device=None):
    check_decodable(model)
    if device is None:
        device = model.layers[0].multi_attn.qkv.weight.device
    return KVCache(len(model.layers), batch, model.n_heads, model.block_size if max_len is None else max_len, device)


def _skinny(a, w, epi, bias, aux=None):
    """gemm_skinny over row blocks of at most 64 (a decode batch larger than the kernel's M)"""
    M = a.shape[0]
    if M <= ops.SKINNY_MAX_M:
        return ops.gemm_skinny(a, w, epi, bias=bias, aux=aux)
    parts = [ops.gemm_skinny(a[i:i + ops.SKINNY_MAX_M], w, epi, bias=bias, aux=None if aux is None else aux[i:i + ops.SKINNY_MAX_M])
             for i in range(0, M, ops.SKINNY_MAX_M)]
    if epi == ops.EPI_GELU:
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    return torch.cat(parts)


def _qkv_append(a, w, bias, k_cache, v_cache, cache, H):
    """the QKV Linear with the K/V append in its epilogue, over row blocks of at most 64 sequences (each block owns its rows of the caches)"""
    M, S = a.shape[0], ops.SKINNY_MAX_M
    if M <= S:
        return ops.gemm_skinny_qkv_append(a, w, bias, k_cache, v_cache, cache.len_dev, H, host_len=cache.len)
    return torch.cat([ops.gemm_skinny_qkv_append(a[i:i + S], w, bias, k_cache[i:i + S], v_cache[i:i + S], cache.len_dev, H, host_len=cache.len)
                      for i in range(0, M, S)])


def forward_cached(model, x, cache: KVCache):
    """x fp32 / bf16 [B, T, D]: positions cache.len .. cache.len+T-1 -> their hidden states (x's dtype), cache advanced by T.
    T > 1 (prefill) needs an empty cache."""
    check_decodable(model)
    if x.dim() != 3:
        raise ValueError(f"forward_cached: x must be [B, T, D], got {tuple(x.shape)}")
    B, T, D = x.shape
    H = model.n_heads
    if D != model.n_embd or B != cache.batch or len(model.layers) != cache.n_layers or H != cache.n_heads:
        raise ValueError(f"forward_cached: x [B={B}, T={T}, D={D}] does not match the cache (batch {cache.batch}, {cache.n_layers} layers, "
                         f"{cache.n_heads} heads) or the model (n_embd {model.n_embd})")
    if T < 1:
        raise ValueError("forward_cached: T must be >= 1")
    if cache.len + T > cache.max_len:
        raise ValueError(f"forward_cached: {cache.len} cached + {T} new positions exceed the cache length {cache.max_len}")
    if T > 1 and cache.len > 0:
        raise ValueError("forward_cached: a prefill (T > 1) needs an empty cache; decode one token at a time after it")
    if not x.is_cuda:
        raise VitamdError("forward_cached: expected a ROCm device tensor (the HIP kernels are the only implementation)")
    params = [layer._params() for layer in model.layers]
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        WEIGHTS.prepare([p[j] for p in params for j in (0, 2, 4)], False)
        cur = _f32c(x).view(B * T, D)
        for i, (wqkv, bqkv, w1, b1, w2, b2) in enumerate(params):
            wqkv_b, w1_b, w2_b = (WEIGHTS.get(w, False)[0] for w in (wqkv, w1, w2))
            bqkv, b1, b2 = _f32c(bqkv), _f32c(b1), _f32c(b2)
            k_cache, v_cache = cache.k[i], cache.v[i]
            _, a, _, _ = ops.layernorm_fwd(cur)                                          # LN1            transformer.py:43
            if T == 1:
                qkv = _qkv_append(a, wqkv_b, bqkv, k_cache, v_cache, cache, H)           # fused QKV + K/V append   transformer.py:27
                o = ops.decode_attention(qkv, k_cache, v_cache, cache.len_dev, B, H, host_len=cache.len)   # SDPA, last row   transformer.py:28-29
                x1, bln, _, _ = ops.layernorm_fwd(cur, addend=o)                         # residual + LN2 transformer.py:43-44
                _, h = _skinny(bln, w1_b, ops.EPI_GELU, b1)                              # fc1 + GELU     transformer.py:37-38
                cur = _skinny(h, w2_b, ops.EPI_RESID_F32, b2, aux=x1)                    # fc2 + residual transformer.py:39,44
            else:
                qkv = ops.gemm_nt(a, wqkv_b, ops.EPI_BIAS_BF16, bias=bqkv)
                ops.kv_append(qkv, k_cache, v_cache, cache.len_dev, B, T, H, host_len=cache.len)
                o, _ = ops.attention_fwd(qkv, B, T, H, causal=True)
                x1, bln, _, _ = ops.layernorm_fwd(cur, addend=o)
                _, h = ops.gemm_nt(bln, w1_b, ops.EPI_GELU, bias=b1)
                cur = ops.gemm_nt(h, w2_b, ops.EPI_RESID_F32, bias=b2, aux=x1)
        cache._advance(T)
    return cur.view(B, T, D).to(x.dtype)
