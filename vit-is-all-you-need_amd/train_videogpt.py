"""MI355X-native drop-in for the reference's `train_videogpt` module (reference train_videogpt.py:18-66 and the body of its training
loop, :130-136): VideoGPTConfig and VideoGPT with the same constructor signatures, attributes and state_dict keys (`tok_embed.weight`,
`pos_embed.weight`, `transformer.layers.*` including the causal `mask` buffers, `proj.{weight,bias}`), so reference checkpoints load.

The causal stack runs on the HIP kernels (transformer.Transformer -> TransformerStackFn), the output projection on the MFMA GEMMs.
Two routes lead to the loss.  `forward` is the reference's: it returns the fp32 logits (functions.linear) and the loss, with the embedding
gathers and the cross-entropy as torch device ops.  `loss` is the training route (vitamd/lm.py, csrc/loss.hip): the token + position
embedding, the head GEMM with bf16 logits and the cross-entropy, forward and backward, are all kernels of the library - no logits in
fp32, no padding, nothing left to the framework's ops.  `train_step` is one iteration of the reference loop on that route and `main()`
runs it on seeded random tokens.  The greedy argmax of generation is a torch device op; sampled generation (temperature / top-k /
top-p) draws each token in one HIP kernel (csrc/sample.hip).  `generate` adds a KV cache (vitamd/decode.py): the prompt is prefilled
once and every further token costs one single-row pass through the stack - with graph=True one graph launch (vitamd/graph.py
GraphedDecoder).  `frames_to_tokens` and `tokens_to_frames` are the reference loop's two uses of its frame tokenizer
(train_videogpt.py:122-127 and :148-156) for any object with `encode(x) -> (z_q, {"min_encoding_indices": ...})` and
`decode_tokens(ids) -> frames` - train_tatitok.TiTok is one - and `main(--tokenizer tatitok)` trains on the code ids of seeded random
frames and decodes a generated continuation.  The reference's data loading is not part of this module."""
import argparse
import time
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from transformer import Transformer, transformer_configs
from utils import get_lr_scheduler
from vitamd import data, lm, ops
from vitamd.functions import WEIGHTS, linear


@dataclass
class VideoGPTConfig:
    frame_size: int
    codebook_size: int
    transformer: str
    max_frames: int
    dropout: float

    def __post_init__(self):
        self.max_tokens = self.max_frames * self.frame_size
        self.trans_config = transformer_configs[self.transformer](block_size=self.max_tokens, dropout=self.dropout, causal=True)
        self.n_embd = self.trans_config.n_embd


class VideoGPT(nn.Module):
    """Next-token model over flattened video tokens [B, T*N]; index codebook_size is the start-of-sequence token."""

    def __init__(self, config: VideoGPTConfig):
        super().__init__()
        self.config = config
        self.tok_embed = nn.Embedding(config.codebook_size + 1, config.n_embd)
        self.pos_embed = nn.Embedding(config.max_tokens, config.n_embd)
        self.transformer = Transformer(config.trans_config)
        self.proj = nn.Linear(config.n_embd, config.codebook_size)
        self._graph_key, self._graph_decoder = None, None      # generate(graph=True): the most recent captured decoder and what it was built for

    def _embed(self, ids, pos0=0):
        """token + position embeddings of ids [B, S] at positions pos0 .. pos0+S-1 (train_videogpt.py:49,59), fp32"""
        pos = torch.arange(pos0, pos0 + ids.shape[1], device=ids.device)
        return (self.tok_embed(ids) + self.pos_embed(pos)).float()

    def _sos(self, B, device):
        return torch.full((B, 1), self.config.codebook_size, device=device, dtype=torch.long)

    def forward(self, x):
        """x [B, T, N] token ids -> (logits [B, T*N, codebook_size], cross-entropy) (train_videogpt.py:44-53)"""
        B, T, N = x.shape
        y = x.reshape(B, T * N)
        inp = torch.cat([self._sos(B, x.device), y[:, :-1]], dim=-1)
        h = self.transformer(self._embed(inp))
        logits = linear(h, self.proj.weight, self.proj.bias)
        loss = F.cross_entropy(logits.reshape(B * T * N, -1), y.reshape(B * T * N))
        return logits, loss

    def loss(self, x):
        """x [B, T, N] token ids -> the scalar cross-entropy of `forward`, by the training route: lm.token_embed, the stack,
        lm.linear_cross_entropy (bf16 logits that live from the head GEMM to their own gradient; no logits are returned)"""
        B, T, N = x.shape
        y = x.reshape(B, T * N)
        inp = torch.cat([self._sos(B, x.device), y[:, :-1]], dim=-1)
        h = self.transformer(lm.token_embed(inp, self.tok_embed.weight, self.pos_embed.weight))
        return lm.linear_cross_entropy(h, self.proj.weight, self.proj.bias, y.reshape(B * T * N))

    def eval_logits(self, x):
        """x [B, T, N] token ids -> (logits [B*T*N, codebook_size], targets int64 [B*T*N]): the validation route, what
        vitamd.metrics.ClassifyMetrics.update takes.  Where lm.fused_head_applies holds the logits are bf16 straight from the head GEMM
        (lm.token_embed, the stack, lm.head_logits: the numbers `loss` takes its cross-entropy of, never in fp32); otherwise
        functions.linear's fp32 logits.  No graph is kept under torch.no_grad()."""
        B, T, N = x.shape
        y = x.reshape(B, T * N)
        inp = torch.cat([self._sos(B, x.device), y[:, :-1]], dim=-1)
        h = self.transformer(lm.token_embed(inp, self.tok_embed.weight, self.pos_embed.weight))
        return lm.head_logits(h, self.proj.weight, self.proj.bias), y.reshape(B * T * N)

    def _head(self, h_last):
        """fp32 logits [B, codebook_size] of hidden states [B, D]: the skinny-M GEMM (one row per sequence) where its shape rules hold,
        else the padded generic Linear"""
        B, D = h_last.shape
        Nc = self.config.codebook_size
        if Nc % 4 == 0 and D % 64 == 0:
            hb = ops.cast_bf16(h_last.float().contiguous())
            wb, _ = WEIGHTS.get(self.proj.weight, False)
            bias = self.proj.bias.detach().float().contiguous()
            rows = [ops.gemm_skinny(hb[i:i + ops.SKINNY_MAX_M], wb, ops.EPI_F32, bias=bias) for i in range(0, B, ops.SKINNY_MAX_M)]
            return rows[0] if len(rows) == 1 else torch.cat(rows)
        return linear(h_last, self.proj.weight, self.proj.bias)

    def _use_cache(self, use_cache):
        if use_cache is None:
            return self.config.dropout == 0
        if use_cache and self.config.dropout > 0:
            raise ValueError(f"generate(use_cache=True) needs dropout == 0 (got {self.config.dropout}): the reference applies SDPA dropout "
                             "in eval mode too, which a KV cache cannot reproduce; use use_cache=False")
        return bool(use_cache)

    def _sampler(self, temperature, top_k, top_p, seed):
        """None when all three are None (greedy), else the Sampler of one generate call; parameter errors as ValueError, no device work"""
        if temperature is None and top_k is None and top_p is None:
            return None
        from vitamd import ops as _ops
        from vitamd.sampling import Sampler
        sampler = Sampler(1.0 if temperature is None else temperature, 0 if top_k is None else top_k, 1.0 if top_p is None else top_p, seed)
        _ops.check_sampling(sampler.temperature, sampler.top_k, sampler.top_p, self.config.codebook_size)
        return sampler

    def _decoder(self, B, max_len, sampling, device):
        """the captured decode step for this key, reused when the last call had the same one (its sampler then starts again at position 0)"""
        key = (B, max_len, sampling, str(device))
        if self._graph_key != key or self._graph_decoder is None:
            self._graph_key = self._graph_decoder = None         # the old graph's memory goes before the new capture
            sampler = None if sampling is None else self._sampler(*sampling)
            dec = self.transformer.graphed_decoder(B, max_len, embed=(self.tok_embed.weight, self.pos_embed.weight), head=self._head,
                                                   sampler=sampler, head_weights=[self.proj.weight, self.proj.bias])
            self._graph_key, self._graph_decoder = key, dec
        self._graph_decoder.reset()                              # empty cache: prefill() then checks the graph against the current operands
        return self._graph_decoder

    @torch.no_grad()
    def generate(self, tokens, n=1, use_cache=None, *, temperature=None, top_k=None, top_p=None, seed=0, graph=False):
        """Continuation of tokens [B, S] by n tokens -> [B, S + n] (train_videogpt.py:54-63).  use_cache: None = cached when
        dropout == 0; False = the reference's loop (the whole prefix through the stack per token) on the HIP stack.
        temperature / top_k / top_p all None: greedy (the reference's argmax).  Any of them given: sampled on the device, one kernel
        launch per token (vitamd.sampling.Sampler: temperature -> top-k -> top-p -> draw; the others default to 1.0 / 0 / 1.0 = off),
        token t of the continuation drawn at position t of the Philox stream of `seed` on either loop: one seed, one continuation.
        graph=True (implies the cached loop; dropout must be 0): the prefill and the first pick run eagerly, every further token is one
        replay of a captured decode step (vitamd.graph.GraphedDecoder: embedding, stack, head and pick in one graph launch), never
        synchronising with the host - the same tokens as graph=False, bit for bit.  The model keeps its most recent decoder and reuses it
        for the same (batch, S + n, sampling parameters and seed, device); another key captures again."""
        B, S = tokens.shape
        if graph:
            if use_cache is not None and not use_cache:
                raise ValueError("generate(graph=True) replays the KV-cached decode step; it cannot be combined with use_cache=False")
            if self.config.dropout > 0:
                raise ValueError(f"generate(graph=True) needs dropout == 0 (got {self.config.dropout}): it runs the KV-cached loop")
        if n < 1:
            return tokens
        if S + n > self.config.max_tokens:
            raise ValueError(f"generate: {S} + {n} tokens need {S + n} positions, the model has max_tokens = {self.config.max_tokens}")
        cached = self._use_cache(use_cache)
        sampler = self._sampler(temperature, top_k, top_p, seed)
        if graph:
            return self._generate_graphed(tokens, n, sampler)

        def pick(logits):
            if sampler is None:
                return torch.argmax(logits, dim=-1, keepdim=True)
            return sampler(logits).unsqueeze(-1)

        if not cached:
            for _ in range(n):
                h = self.transformer(self._embed(torch.cat([self._sos(B, tokens.device), tokens], dim=-1)))
                nxt = pick(self._head(h[:, -1]))
                tokens = torch.cat([tokens, nxt], dim=-1)
            return tokens
        cache = self.transformer.new_cache(B, max_len=S + n)
        h = self.transformer.forward_cached(self._embed(torch.cat([self._sos(B, tokens.device), tokens], dim=-1)), cache)   # prefill
        out = [tokens]
        for step in range(n):
            nxt = pick(self._head(h[:, -1]))
            out.append(nxt)
            if step + 1 < n:
                h = self.transformer.forward_cached(self._embed(nxt, pos0=cache.len), cache)
        return torch.cat(out, dim=-1)

    def _generate_graphed(self, tokens, n, sampler):
        B, S = tokens.shape
        sampling = None if sampler is None else (sampler.temperature, sampler.top_k, sampler.top_p, sampler.seed)
        dec = self._decoder(B, S + n, sampling, tokens.device)           # the eager cached path's max_len: the same attention chunking
        out = torch.empty((B, S + n), dtype=tokens.dtype, device=tokens.device)
        out[:, :S] = tokens
        h = dec.prefill(self._embed(torch.cat([self._sos(B, tokens.device), tokens], dim=-1)))
        logits = self._head(h[:, -1])
        first = torch.argmax(logits, dim=-1) if dec.sampler is None else dec.sampler(logits)        # position 0 of the sampler's stream
        dec.tokens.copy_(first)
        out[:, S] = first
        for t in range(1, n):
            dec.step()                                                    # one graph launch: embed, stack, head, pick -> dec.tokens
            out[:, S + t] = dec.tokens                                    # the one eager device op per token
        return out

    def generate_frames(self, video_tokens, n=1, use_cache=None, *, temperature=None, top_k=None, top_p=None, seed=0, graph=False):
        """video_tokens [B, T, N] -> [B, T*N + n*frame_size] (train_videogpt.py:64-66)"""
        B, T, N = video_tokens.shape
        return self.generate(video_tokens.reshape(B, T * N), n * self.config.frame_size, use_cache=use_cache, temperature=temperature,
                             top_k=top_k, top_p=top_p, seed=seed, graph=graph)


@torch.no_grad()
def frames_to_tokens(tokenizer, videos, index=None, size=None):
    """videos [B, T, 3, H, W] -> code ids int64 [B, T, N] (train_videogpt.py:122-127): every frame through tokenizer.encode, in eval mode
    and without a graph; the tokenizer's training flag is put back.  videos may also be raw uint8 [B, T, H, W, C] on the device (what the
    reference's video sets hold): they go through vitamd.data.Frames, scaled to [0, 1].  index (uint8 videos only): int64 [B, T'] of
    frame numbers into the flattened [B*T] frames - the window videos[:, offset:offset+T'] without a copy -> ids [B, T', N].  size (uint8
    videos only; an int or (H, W)): the tokenizer's frame size where the videos have another - the shorter side is resized to the shorter
    side of `size` (antialiased bilinear) and the centre is cropped, inside the same launch (vitamd.resize.ResizedFrames)"""
    if videos.dim() != 5:
        raise ValueError(f"frames_to_tokens: expected videos [B, T, C, H, W] or uint8 [B, T, H, W, C], got {tuple(videos.shape)}")
    B, T = videos.shape[:2]
    if videos.dtype == torch.uint8:
        if index is not None:
            if index.dim() != 2 or index.shape[0] != B:
                raise ValueError(f"frames_to_tokens: index must be int64 [{B}, T'], got {tuple(index.shape)}")
            T = index.shape[1]
            index = index.reshape(-1)
        if size is not None and data._hw(size) != tuple(videos.shape[2:4]):
            from vitamd import resize
            out_hw = data._hw(size)
            box = resize.resize_center_boxes(B * T, tuple(videos.shape[2:4]), min(out_hw), out_hw)
            frames = resize.ResizedFrames(videos, out_hw, box, index=index)
        else:
            frames = data.Frames(videos, tuple(videos.shape[2:4]), index=index)
    elif index is not None or size is not None:
        raise ValueError("frames_to_tokens: index and size go with uint8 videos; slice or resize a float tensor instead")
    else:
        frames = videos.reshape(B * T, *videos.shape[2:])
    was_training = getattr(tokenizer, "training", False)
    if was_training:
        tokenizer.eval()
    try:
        _, info = tokenizer.encode(frames)
    finally:
        if was_training:
            tokenizer.train()
    ids = info["min_encoding_indices"]
    if ids.dim() == 3:
        ids = ids.squeeze(1)                                     # [B*T, 1, N] -> [B*T, N]
    return ids.reshape(B, T, -1).long()


@torch.no_grad()
def tokens_to_frames(tokenizer, tokens, T, as_u8=False):
    """flattened code ids [B, T*N] (what generate_frames returns) -> frames [B, T, 3, H, W] clamped to [0, 1] (train_videogpt.py:148-156);
    as_u8: uint8 [B, T, H, W, 3] instead, rint(clamp * 255) in one kernel (vitamd.data.to_u8): what goes to the host or a video file"""
    if tokens.dim() != 2 or T < 1 or tokens.shape[1] % T:
        raise ValueError(f"tokens_to_frames: expected tokens [B, T*N] with T = {T}, got {tuple(tokens.shape)}")
    B = tokens.shape[0]
    was_training = getattr(tokenizer, "training", False)
    if was_training:
        tokenizer.eval()
    try:
        frames = tokenizer.decode_tokens(tokens.reshape(B * T, -1))
    finally:
        if was_training:
            tokenizer.train()
    if as_u8:
        out = data.to_u8(frames)
        return out.reshape(B, T, *out.shape[1:])
    return torch.clamp(frames, 0.0, 1.0).reshape(B, T, *frames.shape[1:])


def train_step(model, tokens, optim, lr_sched=None):
    """One iteration of the reference hot loop (train_videogpt.py:130-136) without the fp16 scaler, on VideoGPT.loss."""
    optim.zero_grad(set_to_none=True)
    loss = model.loss(tokens)
    loss.backward()
    optim.step()
    if lr_sched is not None:
        lr_sched.step()
    return loss


def evaluate(model, token_batches, topk=5, metrics=None):
    """Token-level validation of a VideoGPT: the model in eval mode under torch.no_grad() over `token_batches` of ids [B, T, N], every
    batch's eval_logits added to a vitamd.metrics.ClassifyMetrics on the device (metrics: one to continue; None: a fresh one).  The host
    reads nothing before the final result() -> {"loss" (mean next-token cross-entropy), "top1", "topk" (token accuracies), "count",
    "perplexity"}.  model.training is put back, also when a batch raises."""
    from vitamd.metrics import ClassifyMetrics
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for tokens in token_batches:
                if metrics is None:
                    metrics = ClassifyMetrics(topk=topk, device=tokens.device)
                metrics.update(*model.eval_logits(tokens))
    finally:
        model.train(was_training)
    if metrics is None:
        raise ValueError("evaluate: no batches")
    return metrics.result()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="VideoGPT training on synthetic tokens (MI355X-native path)")
    p.add_argument("--frame_size", type=int, default=64)
    p.add_argument("--codebook_size", type=int, default=1024)
    p.add_argument("--transformer", type=str, default="B")
    p.add_argument("--max_frames", type=int, default=16)
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=5000)
    p.add_argument("--train_steps", type=int, default=50)
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip the global gradient norm on the device (vitamd.optim.AdamW, multi-tensor path); default: no clipping")
    p.add_argument("--graph", action="store_true",
                   help="one graph launch per iteration (vitamd.graph.GraphedTrainStep): forward, loss, backward, the clip, the LR schedule "
                        "and the AdamW update, all replayed from the device; needs --dropout 0")
    p.add_argument("--tokenizer", type=str, default="none", choices=("none", "tatitok"),
                   help="none: seeded random token ids; tatitok: a random-weight train_tatitok.TiTok (latent_tokens = frame_size) tokenises "
                        "seeded random frames and decodes one generated continuation at the end")
    p.add_argument("--image_size", type=int, default=64, help="frame side for --tokenizer tatitok")
    p.add_argument("--patch_size", type=int, default=16, help="patch side for --tokenizer tatitok")
    p.add_argument("--condition_frames", type=int, default=1, help="frames the final generation is conditioned on (--tokenizer tatitok)")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate every N training steps on seeded held-out random tokens (evaluate / vitamd.metrics.ClassifyMetrics: loss, "
                        "perplexity and token accuracy from counters on the device, one host read per evaluation); 0 = never")
    p.add_argument("--eval_batches", type=int, default=2, help="the batches of one evaluation (--eval_every)")
    return p.parse_args(argv)


def make_tatitok(args, device):
    """a random-weight 1D TiTok whose frames have args.frame_size code ids out of args.codebook_size"""
    import train_tatitok as TA
    torch.manual_seed(0)
    cfg = TA.TiTokConfig(args.image_size, args.patch_size, args.frame_size, args.codebook_size, 12, "small")
    return TA.TiTok(cfg).to(device).eval()


def make_optim(model, args):
    from vitamd.optim import AdamW
    if getattr(args, "graph", False):
        return AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, capturable=True,
                     schedule=(args.warmup_steps, args.train_steps, args.lr / 10))
    if args.max_grad_norm is None:
        return torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    return AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)


def main(argv=None):
    args = parse_args(argv)
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        raise SystemExit("--eval_every needs N >= 0 and --eval_batches >= 1")
    topk = min(5, args.codebook_size)                                 # of the evaluations: top-5, or all the classes of a smaller head
    dev = torch.device("cuda")
    cfg = VideoGPTConfig(args.frame_size, args.codebook_size, args.transformer, args.max_frames, args.dropout)
    model = VideoGPT(cfg).to(dev)
    optim = make_optim(model, args)
    sched = None if args.graph else get_lr_scheduler(optim, args.warmup_steps, args.train_steps, args.lr / 10)
    g = torch.Generator(device="cpu").manual_seed(0)
    titok = None
    if args.tokenizer == "tatitok":
        titok = make_tatitok(args, dev)
        videos = torch.rand((args.bs, args.max_frames, 3, args.image_size, args.image_size), generator=g).to(dev)
        tokens = frames_to_tokens(titok, videos)
    else:
        tokens = torch.randint(0, args.codebook_size, (args.bs, args.max_frames, args.frame_size), generator=g).to(dev)
    graphed = None
    if args.graph:
        from vitamd.graph import GraphedTrainStep
        graphed = GraphedTrainStep(model, lambda tok: model.loss(tok), (tokens,), optim)      # refuses dropout > 0
    val = None
    if args.eval_every > 0:                                       # held-out ids under their own seed
        gv = torch.Generator(device="cpu").manual_seed(1)
        val = [torch.randint(0, args.codebook_size, (args.bs, args.max_frames, args.frame_size), generator=gv).to(dev)
               for _ in range(args.eval_batches)]
    for step in range(args.train_steps):
        t0 = time.time()
        loss = graphed(tokens) if graphed is not None else train_step(model, tokens, optim, sched)
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} {tokens.numel() / (time.time() - t0):.0f} tokens/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            r = evaluate(model, val, topk=topk)
            print(f"step {step} val loss {r['loss']:.4f} perplexity {r['perplexity']:.2f} top1 {r['top1']:.4f} top{topk} "
                  f"{r['topk']:.4f} over {r['count']} tokens")
    if titok is not None:
        model.eval()
        cond = min(max(args.condition_frames, 1), args.max_frames - 1)
        gen = model.generate_frames(tokens[:1, :cond], n=args.max_frames - cond)
        frames = tokens_to_frames(titok, gen, args.max_frames)
        print(f"generated {tuple(frames.shape)} frames from {cond} conditioning frame(s): min {float(frames.min()):.3f} max {float(frames.max()):.3f}")


if __name__ == "__main__":
    main()
