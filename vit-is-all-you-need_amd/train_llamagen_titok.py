"""MI355X-native drop-in for the model half of the reference's `train_llamagen_titok` module (reference train_llamagen_titok.py:20-116):
a 1D TiTok over the CODE IDS of an existing VQ tokenizer instead of pixels, trained by cross-entropy against its own input.
TiTokConfig, TiTokEncoder, Quantizer, TiTokDecoder and TiTok keep the reference's constructor signatures, attributes, initialisation
rule and state_dict keys (`enc.transformer.*`, `enc.tok_emb.weight`, `enc.pos_emb`, `enc.extra_emb.weight`, `enc.proj.*`,
`quant.codebook.weight`, `dec.transformer.*`, `dec.pos_emb`, `dec.quant_proj.*`, `dec.emb_proj.*`, `dec.mask_tokens.weight`).

Two routes lead through the model.  `forward` is the reference's: it returns the fp32 logits over the VQ vocabulary, with both input
sequences built by torch device ops (embedding / add / expand / cat).  `loss` is the training route: each input
sequence is assembled by one kernel (vitamd.lm.prefixed_token_embed / prefixed_rows, csrc/assemble.hip), the quantiser is
vitamd.tokenizer.vq_quantize, and the head runs fused with the cross-entropy (vitamd.lm.linear_cross_entropy) - no logits in fp32, no
padded copies.  `train_step` is one iteration of the reference loop on that route; `main()` runs it on seeded random ids, or with
`--vq vitvqgan` on the ids a freshly initialised ViT-VQGAN of this project gives seeded random images.  The reference's VQ model, its
checkpoints, its perceptual network and its data loading are not part of this module, and nothing is fetched."""
import argparse
import time
from dataclasses import dataclass

import torch
import torch.nn as nn

from train_titok import HipLinear, Quantizer, make_optim
from transformer import Transformer, transformer_configs
from utils import get_lr_scheduler
from vitamd import lm, tokenizer


@dataclass
class TiTokConfig:
    vq_codebook_size: int
    vq_latent_tokens: int
    latent_tokens: int
    codebook_size: int
    latent_dim: int
    transformer: str

    def __post_init__(self):
        self.trans_config = transformer_configs[self.transformer](block_size=self.vq_latent_tokens + self.latent_tokens, dropout=0.0)
        self.n_embd = self.trans_config.n_embd


class TiTokEncoder(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.latent_tokens = titok_config.latent_tokens
        self.transformer = Transformer(titok_config.trans_config)
        self.tok_emb = nn.Embedding(titok_config.vq_codebook_size, titok_config.n_embd)
        self.pos_emb = nn.Parameter(torch.randn(titok_config.vq_latent_tokens, titok_config.n_embd) * titok_config.n_embd ** -0.5)
        self.extra_emb = nn.Embedding(titok_config.latent_tokens, titok_config.n_embd)
        self.proj = HipLinear(titok_config.n_embd, titok_config.latent_dim)

    def tokens(self, x, fused=False):
        """ids [b, s] -> the stack's input [b, latent_tokens + s, n_embd]: the learned latent rows in front of tok_emb(x) + pos_emb[:s]
        (train_llamagen_titok.py:43-46).  fused: one kernel instead of the torch ops, the same bits"""
        if fused:
            return lm.prefixed_token_embed(x, self.tok_emb.weight, self.pos_emb, self.extra_emb.weight)
        emb = self.tok_emb(x) + self.pos_emb[: x.shape[1]]
        return torch.cat([self.extra_emb.weight.unsqueeze(0).expand(x.shape[0], -1, -1), emb], dim=1)

    def forward(self, x, fused=False):
        return self.proj(self.transformer(self.tokens(x, fused), keep=self.latent_tokens))     # the latents are the PREPENDED rows


class TiTokDecoder(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.config = titok_config
        self.transformer = Transformer(titok_config.trans_config)
        self.pos_emb = nn.Parameter(torch.randn(titok_config.latent_tokens, titok_config.n_embd) * titok_config.n_embd ** -0.5)
        self.quant_proj = HipLinear(titok_config.latent_dim, titok_config.n_embd)
        self.emb_proj = HipLinear(titok_config.n_embd, titok_config.vq_codebook_size)
        self.mask_tokens = nn.Embedding(titok_config.vq_latent_tokens, titok_config.n_embd)

    def tokens(self, z, fused=False):
        """quantised latents [b, n, latent_dim] -> the stack's input [b, vq_latent_tokens + n, n_embd]: the learned mask rows in front of
        quant_proj(z) + pos_emb[:n] (train_llamagen_titok.py:80-82)"""
        body = self.quant_proj(z)
        if fused:
            return lm.prefixed_rows(body, self.pos_emb, self.mask_tokens.weight)
        emb = body + self.pos_emb[: z.shape[1]]
        return torch.cat([self.mask_tokens.weight.unsqueeze(0).expand(z.shape[0], -1, -1), emb], dim=1)

    def features(self, z, fused=False):
        """-> the stack's output at the mask rows [b, vq_latent_tokens, n_embd], before the head"""
        return self.transformer(self.tokens(z, fused), keep=self.config.vq_latent_tokens)

    def forward(self, z):
        return self.emb_proj(self.features(z))


class TiTok(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.config = titok_config
        self.block_size = titok_config.trans_config.block_size
        self.enc = TiTokEncoder(titok_config)
        self.quant = Quantizer(titok_config)
        self.dec = TiTokDecoder(titok_config)
        self.apply(self._init_weights)

    def encode(self, z):
        """VQ code ids [b, s] -> latent ids [b, latent_tokens]"""
        return self.quant(self.enc(z))[1]

    def decode(self, z_quant):
        return self.dec(z_quant)

    def decode_indices(self, indices):
        return self.dec(self.quant.codebook(indices))

    def forward(self, x):
        """-> (logits fp32 [b, s, vq_codebook_size], latent ids, quantiser loss)"""
        quantized, indices, quantize_loss = self.quant(self.enc(x))
        return self.dec(quantized), indices, quantize_loss

    def loss(self, x):
        """-> (cross-entropy of the decoded logits against x, quantiser loss, latent ids) on the fused route:
        prefixed_token_embed -> stack -> proj -> vq_quantize -> quant_proj -> prefixed_rows -> stack -> linear_cross_entropy on emb_proj's
        parameters.  No logits are formed in fp32 (forward() stays the route that yields them); where the head runs fused, a second
        backward through the same loss raises RuntimeError."""
        quantized, ids, qloss = tokenizer.vq_quantize(self.enc(x, fused=True), self.quant.codebook.weight)
        h = self.dec.features(quantized, fused=True)
        recon = lm.linear_cross_entropy(h, self.dec.emb_proj.weight, self.dec.emb_proj.bias, x.reshape(-1))
        return recon, qloss, ids

    @torch.no_grad()
    def reconstruct(self, x):
        """VQ code ids [b, s] -> the model's reading of them, int64 [b, s]: the argmax of the decoded logits (train_llamagen_titok.py:238)"""
        return self(x)[0].argmax(dim=-1)

    def _init_weights(self, module):
        """the reference's rule (train_llamagen_titok.py:104-116): Linear and Embedding weights ~ trunc_normal(0, 0.02) - the quantiser's
        codebook included, whose uniform initialisation it overwrites - biases zero; the two pos_emb Parameters keep their own draw"""
        if isinstance(module, (nn.Linear, nn.Conv1d, nn.Conv2d)):
            nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)


def codes_from(vq_tokenizer, images):
    """the VQ code ids of images, int64 [b, n], from any module whose encode(images) returns them (train_vit_vqgan.ViTVQGAN,
    train_titok.TiTok): the reference loop's use of its frozen VQ model (train_llamagen_titok.py:208-210)"""
    with torch.no_grad():
        ids = vq_tokenizer.encode(images)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 2:
        raise TypeError(f"codes_from: encode(images) must return int64 ids [b, n], got {getattr(ids, 'dtype', type(ids))} "
                        f"{tuple(getattr(ids, 'shape', ()))}")
    return ids.contiguous()


def train_step(model, ids, optim, lr_sched=None):
    """One iteration of the reference hot loop (train_llamagen_titok.py:212-226) without the fp16 scaler, on model.loss.
    The reference clips the gradients AFTER the optimiser step, where the clip changes no update; this step does not clip
    (make_optim's --max_grad_norm clips before the update, on the device).  -> the detached device loss"""
    optim.zero_grad(set_to_none=True)
    recon_loss, qloss, _ = model.loss(ids)
    loss = recon_loss + qloss
    loss.backward()
    optim.step()
    if lr_sched is not None:
        lr_sched.step()
    return loss.detach()


def evaluate(model, batches, topk=5, metrics=None, codes=None):
    """The validation half of the loop for the model without pixels: eval mode under torch.no_grad() over `batches` of VQ code ids
    int64 [b, s]; the decoded logits of model(ids) against the ids go to a vitamd.metrics.ClassifyMetrics (loss, top-1, top-k), the
    latent ids to a vitamd.metrics.CodebookMetrics.  No host read before the two final results, which are merged ("count", "perplexity":
    the positions scored and exp(loss); "codes", "code_perplexity": the latent ids counted and the perplexity of their histogram).  model.training is put back, also when a batch raises."""
    from vitamd.metrics import ClassifyMetrics, CodebookMetrics
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for ids in batches:
                if metrics is None:
                    metrics = ClassifyMetrics(topk=topk, device=ids.device)
                if codes is None:
                    codes = CodebookMetrics(int(model.config.codebook_size), device=ids.device)
                logits, latent_ids, _ = model(ids)
                metrics.update(logits, ids)
                codes.update(latent_ids)
    finally:
        model.train(was_training)
    if metrics is None or codes is None:
        raise ValueError("evaluate: no batches")
    out = codes.result()
    out["codes"], out["code_perplexity"] = out.pop("count"), out.pop("perplexity")      # the classifier's result has both names too
    out.update(metrics.result())
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="TiTok over VQ code ids, cross-entropy training on synthetic ids (MI355X-native path)")
    p.add_argument("--vq_codebook_size", type=int, default=16384)
    p.add_argument("--vq_latent_tokens", type=int, default=256)
    p.add_argument("--latent_tokens", type=int, default=256)
    p.add_argument("--codebook_size", type=int, default=16384)
    p.add_argument("--latent_dim", type=int, default=12)
    p.add_argument("--transformer", type=str, default="S")
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=5000)
    p.add_argument("--train_steps", type=int, default=1_000_000, help="the horizon of the learning-rate schedule")
    p.add_argument("--steps", type=int, default=50, help="iterations this run makes")
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip the global gradient norm on the device (vitamd.optim.AdamW, multi-tensor path); default: no clipping")
    p.add_argument("--vq", type=str, default="none", choices=("none", "vitvqgan"),
                   help="none: seeded random ids; vitvqgan: the ids of seeded random images through a freshly initialised ViT-VQGAN "
                        "of this project (patch 16, vq_latent_tokens patches, vq_codebook_size codes)")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate every N training steps on seeded held-out random data (evaluate / vitamd.metrics: cross-entropy, top-1 and top-5 of the decoded logits, codebook usage of the latent ids "
                        "from counters on the device, one host read per evaluation); 0 = never")
    p.add_argument("--eval_batches", type=int, default=2, help="the batches of one evaluation (--eval_every)")
    return p.parse_args(argv)


def make_ids(args, dev):
    """the batch of VQ code ids the run trains on, int64 [bs, vq_latent_tokens]"""
    g = torch.Generator(device="cpu").manual_seed(0)
    if args.vq == "none":
        return torch.randint(0, args.vq_codebook_size, (args.bs, args.vq_latent_tokens), generator=g).to(dev)
    from train_vit_vqgan import ViTVQGAN, ViTVQGANConfig
    side = int(round(args.vq_latent_tokens ** 0.5))
    if side * side != args.vq_latent_tokens:
        raise ValueError(f"--vq vitvqgan needs a square number of tokens, got {args.vq_latent_tokens}")
    vq = ViTVQGAN(ViTVQGANConfig(16 * side, 16, args.vq_codebook_size, args.latent_dim, args.transformer)).to(dev).eval()
    images = torch.rand((args.bs, 3, 16 * side, 16 * side), generator=g).to(dev)
    return codes_from(vq, images)


def main():
    args = parse_args()
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        raise SystemExit("--eval_every needs N >= 0 and --eval_batches >= 1")
    dev = torch.device("cuda")
    cfg = TiTokConfig(args.vq_codebook_size, args.vq_latent_tokens, args.latent_tokens, args.codebook_size, args.latent_dim, args.transformer)
    ids = make_ids(args, dev)
    model = TiTok(cfg).to(dev)
    optim = make_optim(model, args)
    sched = get_lr_scheduler(optim, args.warmup_steps, args.train_steps, args.lr / 10)
    usage = torch.zeros([cfg.codebook_size], device=dev)
    val = None
    if args.eval_every > 0:
        g = torch.Generator(device="cpu").manual_seed(1)
        val = [torch.randint(0, args.vq_codebook_size, (args.bs, args.vq_latent_tokens), generator=g).to(dev) for _ in range(args.eval_batches)]
    for step in range(args.steps):
        t0 = time.time()
        loss = train_step(model, ids, optim, sched)
        with torch.no_grad():
            usage[model.encode(ids)] = 1
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} codebook_usage {usage.sum().item() / cfg.codebook_size:.3f} "
              f"{args.bs / (time.time() - t0):.1f} sequences/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            r = evaluate(model, val)
            print(f"step {step} val loss {r['loss']:.4f} top1 {r['top1']:.4f} top5 {r['topk']:.4f} codebook_usage {r['usage']:.3f} "
                  f"code perplexity {r['code_perplexity']:.1f} over {r['count']} positions")
    print(f"reconstructed ids equal to the input: {(model.reconstruct(ids) == ids).float().mean().item():.3f}")


if __name__ == "__main__":
    main()
