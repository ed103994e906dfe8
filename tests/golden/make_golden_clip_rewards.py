#!/usr/bin/env python3
"""Generate tests/golden/clip_rewards.npz by RUNNING THE REFERENCE'S OWN aesthetic_score() and clip_score() (adv_grpo/rewards.py:37-66,
adv_grpo/aesthetic_scorer.py, adv_grpo/clip_scorer.py).

Runs only in the build container (needs the reference checkout; the GPU box never has it, and no test imports this file).  Nothing
from the reference is copied: its modules are imported with make_golden.py's shims, and only numeric inputs / outputs are stored.

* ``CLIPModel.from_pretrained`` returns a small quick_gelu CLIPModel (vision: width 256, 4 heads of 64, 2 layers, mlp 1024, 224 px,
  patch 14; text: the same widths, 2 layers, the full 49408 vocabulary, legacy eos_token_id 2; projection_dim 768, which the aesthetic
  head reads) whose weights are ``synthetic.clip_weights(SMALL, SEED)`` on the CPU generator.  Its ``get_image_features`` returns the
  projected tensor, as in the transformers 4 releases the reference was written against (5 wraps it in a model output).
* ``CLIPProcessor.from_pretrained`` returns transformers' PIL-backend CLIPImageProcessor with the openai/clip-vit-large-patch14 settings
  and a stand-in tokenizer that maps each prompt to stored token ids (``synthetic.clip_input_ids``): no tokenizer files exist here.
* ``torch.load`` returns ``synthetic.aesthetic_head_weights(HEAD_SEED)``; ``Module.cuda`` is the identity (the reference runs on the CPU).
* torchvision is not installed here, so ``torchvision.transforms`` is shimmed with tensor Resize / CenterCrop / Normalize / Compose.  The
  shim is a restatement of torchvision's tensor code path (transforms._compute_resized_output_size, F.resize casting non-f32/f64 inputs
  to f32 around F.interpolate(bilinear, antialias=True), F.center_crop's int(round((h - s) / 2.0)), F.normalize's sub then div with
  mean / std in the image's dtype), not torchvision itself.  The kernel is pinned against torch's GPU F.interpolate directly
  (tests/test_gpu_clip_rewards.py); the shim matters only for these end-to-end numbers.

Inputs are structured f32 images (tests/siglip_reference.structured_images): aesthetic 4 at 300 x 300 (square, as the Pillow-exact
path requires), clipscore 4 at 300 x 260 (a non-square crop of 300 x 300 ones).  They are not stored: the GPU test rebuilds them from
the seeds and checks their sha256 against the one stored here.  No weights are stored either.

Usage:  python tests/golden/make_golden_clip_rewards.py
"""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))          # tests/: the structured test images

SEED, HEAD_SEED, IDS_SEED = 2025, 2026, 2027
SMALL = dict(v_hidden=256, v_layers=2, v_heads=4, v_mlp=1024, image_size=224, patch=14, t_hidden=256, t_layers=2, t_heads=4, t_mlp=1024,
             vocab=49408, max_pos=77, proj=768, eos_token_id=2)
AES_IMAGES = dict(n=4, size=300, seed=31)
CLIP_IMAGES = dict(n=4, size=300, seed=32, width=260)
OPENAI_MEAN = [0.48145466, 0.4578275, 0.40821073]
OPENAI_STD = [0.26862954, 0.26130258, 0.27577711]


def aesthetic_images():
    from siglip_reference import structured_images
    return structured_images(AES_IMAGES["n"], AES_IMAGES["size"], AES_IMAGES["seed"])


def clip_images():
    from siglip_reference import structured_images
    c = CLIP_IMAGES
    return structured_images(c["n"], c["size"], c["seed"])[..., : c["width"]].contiguous()


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


class _Resize:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        h, w = img.shape[-2:]
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = self.size, int(self.size * long / short)
        out = [new_long, new_short] if w <= h else [new_short, new_long]
        if [h, w] == out:
            return img
        dt = img.dtype
        x = img if dt in (torch.float32, torch.float64) else img.to(torch.float32)
        x = F.interpolate(x, size=out, mode="bilinear", align_corners=False, antialias=True)
        return x if x.dtype == dt else x.to(dt)


class _CenterCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        ch, cw = self.size
        h, w = img.shape[-2:]
        top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        return img[..., top:top + ch, left:left + cw]


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, x):
        m = torch.as_tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return x.clone().sub_(m).div_(s)


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


def main():
    import make_golden
    make_golden.install_shims()
    import transformers
    from transformers import CLIPConfig
    from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
    import torchvision.transforms as T
    T.Resize, T.CenterCrop, T.Normalize, T.Compose = _Resize, _CenterCrop, _Normalize, _Compose

    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import ClipConfig
    cfg = ClipConfig(act="quick_gelu", **SMALL)
    sd = synthetic.clip_weights(cfg, SEED)
    head = synthetic.aesthetic_head_weights(HEAD_SEED)

    def clip_from_pretrained(name, *a, **k):
        vc = dict(hidden_size=cfg.v_hidden, intermediate_size=cfg.v_mlp, num_hidden_layers=cfg.v_layers, num_attention_heads=cfg.v_heads,
                  image_size=cfg.image_size, patch_size=cfg.patch, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=cfg.proj)
        tc = dict(hidden_size=cfg.t_hidden, intermediate_size=cfg.t_mlp, num_hidden_layers=cfg.t_layers, num_attention_heads=cfg.t_heads,
                  vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2,
                  projection_dim=cfg.proj)
        m = transformers.CLIPModel(CLIPConfig(vision_config=vc, text_config=tc, projection_dim=cfg.proj)).eval()
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("position_ids") for k in missing), (missing, unexpected)
        # transformers 5 returns a model output where the 4.x the reference was written against returned the projected tensor; its own
        # forward (clipscore) passes interpolate_pos_encoding and reads the model output, AestheticScorer passes pixel_values only
        feats = transformers.CLIPModel.get_image_features
        m.get_image_features = lambda **kw: feats(m, **kw) if "interpolate_pos_encoding" in kw else feats(m, **kw).pooler_output
        return m

    prompts = [f"prompt {i}" for i in range(CLIP_IMAGES["n"])]
    ids = synthetic.clip_input_ids(len(prompts), seed=IDS_SEED)
    table = {p: ids[i] for i, p in enumerate(prompts)}

    class Processor:
        """CLIPProcessor stand-in: the real PIL-backend image processor (openai/clip-vit-large-patch14 preprocessor_config.json values)
        and a tokenizer that looks the prompts up."""
        def __init__(self):
            self.image_processor = CLIPImageProcessorPil(
                do_resize=True, size={"shortest_edge": 224}, resample=3, do_center_crop=True, crop_size={"height": 224, "width": 224},
                do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=OPENAI_MEAN, image_std=OPENAI_STD,
                do_convert_rgb=True)

        def __call__(self, images=None, text=None, padding=None, truncation=None, return_tensors=None, **kw):
            out = {}
            if images is not None:
                out.update(self.image_processor(images=images, return_tensors="pt"))
            if text is not None:
                assert padding == "max_length" and truncation
                out["input_ids"] = torch.stack([table[t] for t in text])
            return transformers.BatchFeature(out)

    transformers.CLIPModel.from_pretrained = staticmethod(clip_from_pretrained)
    transformers.CLIPProcessor.from_pretrained = staticmethod(lambda *a, **k: Processor())
    torch.load = lambda *a, **k: {k2: v.clone() for k2, v in head.items()}
    torch.nn.Module.cuda = lambda self, *a, **k: self

    import adv_grpo.rewards as RW
    ai, ci = aesthetic_images(), clip_images()
    aes, _ = RW.aesthetic_score()(ai.clone(), None, None)
    aes_zero, _ = RW.aesthetic_score()(torch.zeros_like(ai), None, None)
    cs, _ = RW.clip_score()(ci.clone(), prompts, None)
    cs_zero, _ = RW.clip_score()(torch.zeros_like(ci), prompts, None)
    out = dict(seed=np.int64(SEED), head_seed=np.int64(HEAD_SEED), input_ids=ids.numpy(),
               aesthetic_images_sha256=np.array(sha(ai)), clip_images_sha256=np.array(sha(ci)),
               aesthetic=aes.float().numpy(), aesthetic_zero=aes_zero.float().numpy(),
               clipscore=cs.float().numpy(), clipscore_zero=cs_zero.float().numpy(),
               **{f"cfg_{k}": np.int64(v) for k, v in SMALL.items()},
               **{f"aes_images_{k}": np.int64(v) for k, v in AES_IMAGES.items()},
               **{f"clip_images_{k}": np.int64(v) for k, v in CLIP_IMAGES.items()})
    path = os.path.join(HERE, "clip_rewards.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in ("aesthetic", "aesthetic_zero", "clipscore", "clipscore_zero"):
        print(k, out[k])


if __name__ == "__main__":
    main()
