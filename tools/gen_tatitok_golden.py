"""Writes tests/golden/tatitok_tiny.pt: the reference's 1D TiTok (train_tatitok.TiTok) on seeded weights and images, fp32 on the CPU.

Runs on the build machine only, where the reference checkout exists; no test calls it.  The reference's train_tatitok module cannot be
imported without its data and logging dependencies, so this imports the reference's `blocks` classes and composes them as that module's
TiTok does: encoder(pixel_values, latent_tokens) -> quantize -> decoder, the quantiser VectorQuantizer(commitment_cost=0.25,
use_l2_norm=True).  Weights come from oracle/weights.py (module_state: seeds, not tensors, are what the fixture stores), so the tests
rebuild the same model without the reference.  The fixture has the shape of titok_s256.pt: summaries only, no weights, and the
reference's own bf16-autocast deviation from its fp32 result as the floor the tolerances are judged against.

    python tools/gen_tatitok_golden.py [path of the reference checkout]
"""
import os
import sys
from types import SimpleNamespace as NS

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.dont_write_bytecode = True

import weights as W  # noqa: E402
from gen_golden import REF, rel_l2, save, summarize  # noqa: E402

CFG = dict(image_size=32, patch_size=8, transformer="small", latent_tokens=8, latent_dim=12, codebook_size=64, use_l2_norm=True)
SEED, BATCH = 91, 3


def compose(RB, c):
    """the reference's TiTok out of the reference's blocks (train_tatitok.py:40-54, 71-93), state_dict keys included"""
    cfg = NS(**c)

    class TiTok(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = RB.TiTokEncoder(cfg)
            self.decoder = RB.TiTokDecoder(cfg)
            self.latent_tokens = torch.nn.Parameter(torch.zeros(c["latent_tokens"], self.encoder.width))
            self.quantize = RB.VectorQuantizer(codebook_size=c["codebook_size"], token_size=c["latent_dim"], commitment_cost=0.25,
                                               use_l2_norm=c["use_l2_norm"])

        def encode(self, x):
            z = self.encoder(pixel_values=x, latent_tokens=self.latent_tokens)
            return self.quantize(z) + (z,)

        def decode_tokens(self, tokens):
            tokens = tokens.squeeze(1)
            b, n = tokens.shape
            zq = self.quantize.get_codebook_entry(tokens.reshape(-1)).reshape(b, 1, n, -1)
            return self.decoder(zq.permute(0, 3, 1, 2).contiguous())

        def forward(self, x):
            zq, res, z = self.encode(x)
            return self.decoder(zq), res, z

    return TiTok()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    sys.path.insert(0, ref)
    import blocks as RB       # the reference's module (torch + einops only)
    m = compose(RB, CFG)
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(W.module_state(SEED, shapes), strict=True)
    images = W.uniform(SEED, "images", (BATCH, 3, CFG["image_size"], CFG["image_size"]), 0.5) + 0.5

    def run(bf16):
        m.zero_grad(set_to_none=True)
        if bf16:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                recon, res, z = m(images)
                loss = (recon - images).pow(2).mean() + res["quantizer_loss"]
        else:
            recon, res, z = m(images)
            loss = (recon - images).pow(2).mean() + res["quantizer_loss"]
        loss.backward()
        return (recon.detach().float(), res["min_encoding_indices"].clone(), float(res["quantizer_loss"]), float(loss), z.detach().float(),
                {k: p.grad.detach().clone() for k, p in m.named_parameters()})

    recon, idx, qloss, loss, z, grads = run(False)
    recon16, idx16, _, loss16, _, g16 = run(True)
    with torch.no_grad():
        from_idx = m.decode_tokens(idx)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            from_idx16 = m.decode_tokens(idx).float()
    save("tatitok_tiny.pt", {
        "cfg": dict(CFG, seed=SEED, batch=BATCH),
        "n_params": sum(p.numel() for p in m.parameters()),
        "state_keys": sorted(shapes), "state_shapes": shapes,
        "latents": z, "indices": idx, "quantize_loss": qloss, "loss": loss,
        "recon": summarize(recon), "recon_from_indices": summarize(from_idx),
        "grads": {k: summarize(v) for k, v in grads.items()},
        "ref_bf16_floor": {"recon": rel_l2(from_idx16, from_idx), "index_agreement": float((idx16 == idx).float().mean()),
                           "loss_abs": abs(loss16 - loss), "grads": {k: rel_l2(g16[k], grads[k]) for k in grads}},
    })


if __name__ == "__main__":
    main()
