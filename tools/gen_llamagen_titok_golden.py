"""Writes tests/golden/llamagen_titok_tiny.pt: the reference's TiTok over VQ code ids (train_llamagen_titok.TiTok) on seeded weights and
ids, fp32 on the CPU, with the cross-entropy of its loop (train_llamagen_titok.py:214-216).

Runs on the build machine only, where the reference checkout exists; no test calls it.  The reference module is imported as it is
through oracle/gen_golden.import_reference(); the packages it names at the top and never uses from the model classes (its data loaders,
the LlamaGen VQ model, tqdm) get empty placeholder modules here, as gen_golden does for wandb and lpips.  Weights come from
oracle/weights.py (module_state: seeds, not tensors, are what the fixture stores), so the tests rebuild the same model without the
reference.  The fixture has the shape of tatitok_tiny.pt: summaries only, no weights, and the reference's own bf16-autocast deviation
from its fp32 result as the floor the tolerances are judged against.  The seed is the first from SEED0 on at which the reference's bf16
run picks the same latent id as its fp32 run for at least MIN_AGREEMENT of the latents: a draw on which the reference's own two
precisions disagree about the codes cannot hold an implementation to them.

    python tools/gen_llamagen_titok_golden.py
"""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.dont_write_bytecode = True

import weights as W  # noqa: E402
import gen_golden as G  # noqa: E402
from gen_golden import rel_l2, save, summarize  # noqa: E402

CFG = dict(vq_codebook_size=64, vq_latent_tokens=16, latent_tokens=16, codebook_size=32, latent_dim=12, transformer="S")
SEED0, BATCH, MIN_AGREEMENT = 101, 4, 0.9


def import_titok():
    """the reference's train_llamagen_titok module, with placeholders for the imports its model classes never touch"""
    G.import_reference()
    loaders = types.ModuleType("datasets")
    loaders.get_imagenet_loaders = loaders.get_dmlab_image_loaders = loaders.get_minecraft_image_loaders = None
    sys.modules["datasets"] = loaders
    for name in ("LlamaGen", "LlamaGen.tokenizer", "LlamaGen.tokenizer.tokenizer_image"):
        G._placeholder(name)
    G._placeholder("LlamaGen.tokenizer.tokenizer_image.vq_model", VQ_models={})
    G._placeholder("tqdm")
    import train_llamagen_titok as REF_CODE_TITOK
    return REF_CODE_TITOK


def run_seed(m, shapes, seed):
    m.load_state_dict(W.module_state(seed, shapes), strict=True)
    ids = W.randint(seed, "ids", (BATCH, CFG["vq_latent_tokens"]), CFG["vq_codebook_size"])
    loss_fn = torch.nn.CrossEntropyLoss()

    def run(bf16):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
            logits, idx, qloss = m(ids)
            recon_loss = loss_fn(logits.reshape(-1, logits.shape[-1]), ids.reshape(-1))
            loss = recon_loss + qloss
        loss.backward()
        return (logits.detach().float(), idx.clone(), float(qloss.detach()), float(recon_loss.detach()), float(loss.detach()),
                {k: p.grad.detach().clone() for k, p in m.named_parameters()})

    with torch.no_grad():
        latents = m.enc(ids).detach().float()
    fp32, bf16 = run(False), run(True)
    return ids, latents, fp32, bf16, float((bf16[1] == fp32[1]).float().mean())


def main():
    R = import_titok()
    m = R.TiTok(R.TiTokConfig(**CFG))
    shapes = {k: list(v.shape) for k, v in m.state_dict().items()}
    for seed in range(SEED0, SEED0 + 64):
        ids, latents, (logits, idx, qloss, recon_loss, loss, grads), (l16, _, q16, r16, loss16, g16), agree = run_seed(m, shapes, seed)
        print(f"seed {seed}: the reference's bf16 run agrees with its fp32 run on {agree:.3f} of the latent ids")
        if agree >= MIN_AGREEMENT:
            break
    else:
        raise SystemExit("no seed with the wanted agreement")
    with torch.no_grad():
        from_idx = m.decode_indices(idx).float()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            from_idx16 = m.decode_indices(idx).float()
    save("llamagen_titok_tiny.pt", {
        "cfg": dict(CFG, seed=seed, batch=BATCH, block_size=m.config.trans_config.block_size, n_embd=m.config.n_embd),
        "n_params": sum(p.numel() for p in m.parameters()),
        "state_keys": sorted(shapes), "state_shapes": shapes,
        "latents": latents, "indices": idx, "quantize_loss": qloss, "recon_loss": recon_loss, "loss": loss,
        "logits": summarize(logits), "logits_from_indices": summarize(from_idx), "argmax": logits.argmax(-1),
        "grads": {k: summarize(v) for k, v in grads.items()},
        "ref_bf16_floor": {"logits": rel_l2(l16, logits), "logits_from_indices": rel_l2(from_idx16, from_idx), "index_agreement": agree,
                           "loss_abs": abs(loss16 - loss), "quantize_loss_abs": abs(q16 - qloss),
                           "grads": {k: rel_l2(g16[k], grads[k]) for k in grads}},
    })


if __name__ == "__main__":
    main()
