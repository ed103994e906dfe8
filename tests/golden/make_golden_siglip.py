#!/usr/bin/env python3
"""Generate tests/golden/siglip_similarity.npz by RUNNING THE REFERENCE'S OWN siglip_image_similarity_score (adv_grpo/rewards.py:69-144).

Runs only in the build container (needs the reference checkout; the GPU box never has it, and no test imports this file).  Nothing
from the reference is copied: its module is imported with make_golden.py's shims, and only numeric inputs / outputs are stored.

``SiglipModel.from_pretrained`` is patched to return a small SiglipModel (vision tower: width 576, 8 heads of 72, 2 layers, mlp 4304,
384 px, so400m's patch 14 and eps) whose vision weights are ``synthetic.siglip_weights(cfg, SEED)`` drawn on the CPU generator: the GPU
test rebuilds the same weights from the seed, so no weights are stored.  The reference scorer then runs as written (bf16 model on the
CPU).  Inputs are f32 NCHW images at sizes that are neither 384 nor multiples of 14 (3 at 130^2, 4 at 90^2): solid colours,
gradients, checkerboards and gratings (tests/siglip_reference.structured_images), whose cosines spread over most of [0, 1] -- on noise
images the synthetic tower's pooled embeddings hardly depend on the image.  The CPU and GPU F.interpolate differ on bf16 inputs, so those
are covered on the GPU.

Usage:  python tests/golden/make_golden_siglip.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: the structured test images

SEED = 2024
SMALL = dict(hidden=576, layers=2, heads=8, mlp=4304, image_size=384)


def main():
    import make_golden
    make_golden.install_shims()
    import transformers
    from transformers import SiglipConfig
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    cfg = SiglipVisionConfig(**SMALL)
    sd = synthetic.siglip_weights(cfg, SEED)

    def from_pretrained(name, *a, **k):
        vc = dict(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                  image_size=cfg.image_size, patch_size=cfg.patch, layer_norm_eps=cfg.eps, hidden_act="gelu_pytorch_tanh")
        tc = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1, vocab_size=64)
        torch.manual_seed(0)                                          # (the text tower is never run)
        m = transformers.SiglipModel(SiglipConfig(vision_config=vc, text_config=tc)).eval()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith("text_model.") or k in ("logit_scale", "logit_bias") for k in missing), missing
        return m
    transformers.SiglipModel.from_pretrained = staticmethod(from_pretrained)

    import adv_grpo.rewards as RW
    fn = RW.siglip_image_similarity_score("cpu")
    from siglip_reference import structured_images
    images, refs = structured_images(3, 130, 11), structured_images(4, 90, 12)
    scores, info = fn(images.clone(), refs.clone())
    out = dict(seed=np.int64(SEED), images=images.numpy(), ref_images=refs.numpy(), scores=scores.float().numpy(),
               pairwise=info["pairwise"].float().numpy(), **{k: np.int64(v) for k, v in SMALL.items()})
    path = os.path.join(HERE, "siglip_similarity.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; scores", out["scores"])


if __name__ == "__main__":
    main()
