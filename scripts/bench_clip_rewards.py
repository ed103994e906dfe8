"""aesthetic and clipscore on the kernels: ms per call of each reward for 16 images at 512^2 with the CLIP ViT-L/14 tower (synthetic
weights), in both arithmetics (f32 = the split-bf16 tower of vit_x3.py, the reference's; bf16 = vit.py), and the torchvision
preprocessing kernel's achieved bytes/s (image read once + patch rows written) against the HBM peak.  Prints one JSON line.
Times are device events over --iters calls after 3 warm-up calls."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import preprocess, rewards, synthetic, vit, vit_x3  # noqa: E402
from adv_grpo_amd.model_configs import ClipConfig  # noqa: E402

PEAK_HBM = 8.0e12           # MI355X HBM3E, bytes/s


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    cfg = ClipConfig.vit_l14()
    with synthetic.on_device("cuda"):
        sd = synthetic.clip_weights(cfg, 1)
    head = synthetic.aesthetic_head_weights(2)
    towers = {"f32": vit_x3.CLIPModelX3(sd, cfg, "cuda"), "bf16": vit.CLIPModel({k: v.to(torch.bfloat16) for k, v in sd.items()}, cfg, "cuda")}
    del sd
    g = torch.Generator(device="cuda").manual_seed(0)
    imgs = torch.rand(16, 3, 512, 512, generator=g, device="cuda")
    ids = synthetic.clip_input_ids(16, 3).cuda()
    prompts = rewards.PromptBatch(["a prompt"] * 16, clip_ids=ids)
    out = {"images": "16 at 512x512", "ms_per_call": {}}
    for dt, model in towers.items():
        rewards.configure_aesthetic(model, head)
        rewards.configure_clip(model)
        x = imgs if dt == "f32" else imgs.to(torch.bfloat16)
        for name in ("aesthetic", "clipscore"):
            fn = rewards.multi_score("cuda", {name: 1})
            out["ms_per_call"][f"{name}_{dt}"] = round(timed(lambda: fn(x, prompts, None), a.iters), 3)
    for dt, x3 in (("f32", True), ("bf16", False)):
        x = imgs if dt == "f32" else imgs.to(torch.bfloat16)
        ms = timed(lambda: preprocess.tv_clip_patches(x, x3=x3), 20)
        nbytes = x.numel() * x.element_size() + 16 * 256 * 640 * 2 * (3 if x3 else 1)
        out[f"tv_preprocess_{dt}"] = {"us": round(ms * 1e3, 1), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                                      "frac_hbm_peak": round(nbytes / (ms * 1e-3) / PEAK_HBM, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
