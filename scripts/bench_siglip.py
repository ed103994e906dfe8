"""siglip_image_similarity on the kernels: the scorer end to end on 16 generated (bf16) + 16 reference (f32) images at 512^2 with the
so400m/14 tower (synthetic weights), the tower's share of the bf16 MFMA peak, and one layer's attention (16 heads, 729 tokens, 32
images) at head dim 72 next to the head-dim-80 kernel at the same shape.  Prints one JSON line.
--layers N: a shallower tower (the 27-layer figure is what the reward costs)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import ops, preprocess, rewards, synthetic, vit  # noqa: E402
from adv_grpo_amd.model_configs import SiglipVisionConfig  # noqa: E402

PEAK_BF16 = 2.5e15          # MI355X dense bf16 MFMA, FLOP/s


def timed(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def tower_flop(cfg, n):
    P, D, F = cfg.tokens, cfg.hidden, cfg.mlp
    layer = P * 2 * D * (3 * D + D + 2 * F) + 2 * 2 * P * P * D          # GEMMs + QK^T and PV
    embed = P * 2 * D * 588
    head = P * 2 * D * 2 * D + 2 * 2 * P * D + 2 * D * (D + 2 * F)     # K|V over the tokens, one-query attention, out-proj + MLP
    return n * (cfg.layers * layer + embed + head)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=27)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    cfg = SiglipVisionConfig(layers=a.layers)
    with synthetic.on_device("cuda"):
        sd = synthetic.siglip_weights(cfg, 1)
    model = vit.SiglipVision({k: v.to(torch.bfloat16) for k, v in sd.items()}, cfg, "cuda")
    del sd
    rewards.configure_siglip(model)
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = torch.rand(16, 3, 512, 512, generator=g, device="cuda").to(torch.bfloat16)
    refs = torch.rand(16, 3, 512, 512, generator=g, device="cuda")
    fn = rewards.multi_score("cuda", {"siglip_image_similarity": 1})
    score_ms = timed(lambda: fn(imgs, None, None, ref_images=refs), a.iters)     # (includes the max() > 1 host check of both batches)
    patches = torch.cat([preprocess.siglip_patches(x, cfg.image_size) for x in (imgs, refs)])
    tower_ms = timed(lambda: model.pooler_output(pixel_patches=patches), a.iters)

    B, H, S = 32, 16, cfg.tokens
    att = {}
    for hd in (72, 80):
        qkv = torch.randn(B, S, 3 * H * hd, generator=g, device="cuda").to(torch.bfloat16)
        D = H * hd
        o = torch.empty(B, S, D, dtype=torch.bfloat16, device="cuda")
        att[hd] = timed(lambda: ops.attention(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], H, out=o), 20) * 1e3
    flop = tower_flop(cfg, 32)
    print(json.dumps({"images": "16 bf16 + 16 f32 at 512x512", "layers": cfg.layers, "scorer_ms": round(score_ms, 3),
                      "tower_ms": round(tower_ms, 3), "tower_tflop": round(flop / 1e12, 2),
                      "tower_frac_bf16_peak": round(flop / (tower_ms * 1e-3) / PEAK_BF16, 4),
                      "attention_us_per_layer": {"hd72": round(att[72], 1), "hd80_same_shape": round(att[80], 1)},
                      "attention_shape": [B, H, S, S]}))


if __name__ == "__main__":
    main()
