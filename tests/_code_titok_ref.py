"""References for the code-id TiTok (train_llamagen_titok.py, csrc/assemble.hip).  No GPU, no library: plain torch.

1. The sequence-assembly op, x[b] = cat([prefix, src(b) + pos[:S]]), as the torch expression in the tensors' own dtype (one add per
   element: what the kernel is bit-equal to), and its three gradients as float64 sums together with what their tests need: the fp32
   ascending-batch loop the kernel's dprefix / dpos are bit-equal to, and for dtok the number of terms per table row and the sum of
   their magnitudes (the order of fp32 atomics is free: |got - ref| <= n 2^-24 sum|terms|, n the row's multiplicity - every one of the
   n - 1 additions rounds a partial sum that is at most sum|terms|).
2. The model composed on the CPU from the restatement of oracle/vit_oracle.py (transformer, linear, vq_quantize, cross_entropy), in the
   reference's state-dict keys: tests/test_code_titok_host.py holds it to the reference's golden, the GPU tests then compare against it."""
import torch

import vit_oracle as O

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PRESETS = {"S": (6, 8, 512), "B": (12, 12, 768), "L": (24, 16, 1024)}      # reference transformer.py: layers, heads, width


# ------------------------------------------------------------------------------------------------ 1. sequence assembly
def assemble_ref(prefix, pos, ids=None, tok=None, body=None):
    """cat([prefix expanded over the batch, src + pos[:S]], dim=1) in the tensors' dtype; src = tok[ids] or body [B, S, D]"""
    src = tok[ids] if ids is not None else body
    B, S = src.shape[:2]
    return torch.cat([prefix.unsqueeze(0).expand(B, -1, -1), src + pos[:S]], dim=1)


def batch_sum_f32(g):
    """sum over dim 0 of g fp32 [B, ...] as the kernel takes it: an fp32 accumulator from zero, b ascending"""
    acc = torch.zeros(g.shape[1:], dtype=F32)
    for b in range(g.shape[0]):
        acc = acc + g[b]
    return acc


def assemble_grads_ref(g, E, pos_rows, ids=None, tok_rows=None):
    """float64 gradients of assemble_ref for the upstream g [B, E+S, D]: dprefix [E, D], dpos [pos_rows, D] (rows >= S zero) and, in
    gather mode, dtok [tok_rows, D] (ids outside the table add nothing) with dtok_abs (the same sum over |g|) and n_tok (terms per row)"""
    B, T, D = g.shape
    S = T - E
    g64 = g.to(F64)
    out = {"dprefix": g64[:, :E].sum(dim=0), "dpos": torch.zeros((pos_rows, D), dtype=F64)}
    out["dpos"][:S] = g64[:, E:].sum(dim=0)
    if ids is not None:
        flat = ids.reshape(-1)
        ok = (flat >= 0) & (flat < tok_rows)
        rows = g64[:, E:].reshape(B * S, D)[ok]
        out["dtok"] = torch.zeros((tok_rows, D), dtype=F64).index_add_(0, flat[ok], rows)
        out["dtok_abs"] = torch.zeros((tok_rows, D), dtype=F64).index_add_(0, flat[ok], rows.abs())
        out["n_tok"] = torch.bincount(flat[ok], minlength=tok_rows)
    return out


def dtok_allowance(ref):
    """n 2^-24 sum|terms| per element of dtok"""
    return ref["n_tok"].to(F64)[:, None] * 2.0 ** -24 * ref["dtok_abs"]


# ------------------------------------------------------------------------------------------------ 2. the model on the CPU
def model_forward(ids, sd, cfg, lowp=False):
    """train_llamagen_titok.TiTok.forward on state dict sd (reference keys) -> (logits [B, S, Vq], latent ids, quantiser loss, latents).
    cfg: the golden's cfg dict (vq_latent_tokens, latent_tokens, transformer)."""
    L, H, _ = PRESETS[cfg["transformer"]]
    B, S = ids.shape
    emb = sd["enc.tok_emb.weight"][ids] + sd["enc.pos_emb"][:S]
    x = torch.cat([sd["enc.extra_emb.weight"].unsqueeze(0).expand(B, -1, -1), emb], dim=1)
    h = O.transformer(x, sd, "enc.transformer.", L, H, False, lowp)[:, : cfg["latent_tokens"]]
    latents = O.linear(h, sd["enc.proj.weight"], sd["enc.proj.bias"], lowp)
    quantized, idx, qloss = O.vq_quantize(latents, sd["quant.codebook.weight"])
    return decode(quantized, sd, cfg, lowp), idx, qloss, latents


def decode(z, sd, cfg, lowp=False):
    """train_llamagen_titok.TiTokDecoder.forward: quantised latents [B, n, latent_dim] -> logits [B, vq_latent_tokens, Vq]"""
    L, H, _ = PRESETS[cfg["transformer"]]
    emb = O.linear(z, sd["dec.quant_proj.weight"], sd["dec.quant_proj.bias"], lowp) + sd["dec.pos_emb"][: z.shape[1]]
    x = torch.cat([sd["dec.mask_tokens.weight"].unsqueeze(0).expand(z.shape[0], -1, -1), emb], dim=1)
    y = O.transformer(x, sd, "dec.transformer.", L, H, False, lowp)[:, : cfg["vq_latent_tokens"]]
    return O.linear(y, sd["dec.emb_proj.weight"], sd["dec.emb_proj.bias"], lowp)


def model_loss_and_grads(ids, sd, cfg, lowp=False):
    """-> dict: logits, indices, latents, quantize_loss, recon_loss, loss (floats) and grads {key: tensor} of recon_loss + quantize_loss"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    logits, idx, qloss, latents = model_forward(ids, leaf, cfg, lowp)
    recon = O.cross_entropy(logits.reshape(-1, logits.shape[-1]), ids.reshape(-1))
    loss = recon + qloss
    loss.backward()
    return {"logits": logits.detach(), "indices": idx, "latents": latents.detach(), "quantize_loss": float(qloss.detach()),
            "recon_loss": float(recon.detach()), "loss": float(loss.detach()),
            "grads": {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}}


def golden_case(g):
    """the golden's model inputs rebuilt from its seeds: (state dict, ids)"""
    import weights as W
    c = g["cfg"]
    return W.module_state(c["seed"], g["state_shapes"]), W.randint(c["seed"], "ids", (c["batch"], c["vq_latent_tokens"]), c["vq_codebook_size"])
