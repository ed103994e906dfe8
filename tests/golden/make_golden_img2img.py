#!/usr/bin/env python3
"""Generate tests/golden/img2img.npz by RUNNING THE REFERENCE'S OWN flux_to_sd3_denoise_random / image_to_latent / get_sigmas.

Runs only where the reference checkout is present (no test imports this file).  Nothing of the reference is copied: its module is imported
behind the import shims of make_golden.py and only numeric inputs / outputs are stored.  Stand-ins, as in make_golden.py: oracle.scheduler
for the scheduler object, oracle.standin.StandinVelocity for the transformer, standin_vae_decode for vae.decode, and a stand-in vae.encode
whose latent_dist.sample() is a fixed function of the image (tests/vae_encoder_reference.py: standin_latent_sample) -- this golden pins the
plumbing around the encoder (start-step draw, bf16 rounding points of the forward noising, per-image prompt repeat, the recorded steps), not
the encoder.  The images are 512 x 512 already, so the reference's host Resize is the identity whatever its filter.

Usage:  python tests/golden/make_golden_img2img.py
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (shims, paths)
from oracle.scheduler import FlowMatchEulerScheduler  # noqa: E402
from oracle.standin import StandinVelocity, standin_vae_decode  # noqa: E402
import vae_encoder_reference as ver  # noqa: E402

SEED_RANDOM, SEED_TORCH, STEPS, B, GUIDANCE, NOISE_LEVEL = 31, 77, 20, 2, 4.5, 0.8


def main():
    mg.install_shims()
    from PIL import Image
    from adv_grpo.diffusers_patch import sd3_pipeline_with_logprob_fast as PF
    dtype = torch.bfloat16
    net = StandinVelocity()
    net.config = types.SimpleNamespace(in_channels=16)
    sch = FlowMatchEulerScheduler()
    g = torch.Generator().manual_seed(23)
    pe = torch.randn(1, 5, 32, generator=g).to(dtype); ppe = torch.randn(1, 16, generator=g).to(dtype)
    npe = torch.randn(1, 5, 32, generator=g).to(dtype); nppe = torch.randn(1, 16, generator=g).to(dtype)
    u8 = ver.structured_images_u8(B, 512, seed=1)
    pil = [Image.fromarray(a.numpy()) for a in u8]

    class Pipe:
        transformer = net; scheduler = sch
        _execution_device = "cpu"
        def encode_prompt(self, **k):
            return (k["prompt_embeds"], k["negative_prompt_embeds"], k["pooled_prompt_embeds"], k["negative_pooled_prompt_embeds"])
        @property
        def do_classifier_free_guidance(self): return self._guidance_scale > 1
        @property
        def guidance_scale(self): return self._guidance_scale
        @property
        def clip_skip(self): return self._clip_skip
    pipe = Pipe()
    pipe.vae = types.SimpleNamespace(
        config=types.SimpleNamespace(scaling_factor=1.5305, shift_factor=0.0609), dtype=torch.float32,
        encode=lambda x: types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: ver.standin_latent_sample(x))),
        decode=lambda z, return_dict=False: (standin_vae_decode(z),))
    pipe.image_processor = types.SimpleNamespace(postprocess=lambda im, output_type="pt": (im / 2 + 0.5).clamp(0, 1))

    out = {}
    # image_to_latent alone
    z = PF.image_to_latent(pipe, pil, "cpu")
    out["z"] = z.float().numpy()
    # get_sigmas on a 20-step schedule
    sch.set_timesteps(STEPS)
    ts = sch.timesteps
    pick = torch.stack([ts[0], ts[7], ts[STEPS - 1]])
    out["sigmas_f32"] = PF.get_sigmas(sch, pick, "cpu", n_dim=4, dtype=torch.float32).numpy()
    out["sigmas_bf16"] = PF.get_sigmas(sch, pick, "cpu", n_dim=4, dtype=torch.bfloat16).float().numpy()
    out["sigmas_pick"] = np.array([0, 7, STEPS - 1], dtype=np.int64)
    out["schedule_timesteps"] = ts.numpy()
    out["schedule_sigmas"] = sch.sigmas.numpy()
    # the start-step draw: what random.randint(5, 10) gives for a list of seeds of the global stream
    seeds = list(range(12)) + [SEED_RANDOM]
    draws = []
    for s in seeds:
        random.seed(s)
        draws.append(random.randint(5, 10))
    out["draw_seeds"] = np.array(seeds, dtype=np.int64)
    out["draws"] = np.array(draws, dtype=np.int64)
    # the draws the function will make, replayed from the same torch seed: randn_like(bf16 latents), then one f32 epsilon per step
    random.seed(SEED_RANDOM)
    target_idx = random.randint(5, 10)
    nsteps = STEPS - target_idx
    torch.manual_seed(SEED_TORCH)
    mix_noise = torch.randn(z.shape, dtype=torch.bfloat16)
    noises = [torch.randn(z.shape) for _ in range(nsteps)]
    random.seed(SEED_RANDOM)
    torch.manual_seed(SEED_TORCH)
    with torch.no_grad():
        image, lats, lps, tss = PF.flux_to_sd3_denoise_random(
            pipe, flux_images=pil, device="cpu", output_type="pt", num_inference_steps=STEPS, guidance_scale=GUIDANCE,
            prompt_embeds=pe, negative_prompt_embeds=npe, pooled_prompt_embeds=ppe, negative_pooled_prompt_embeds=nppe,
            noise_level=NOISE_LEVEL)
    after = random.randint(0, 10 ** 9)          # the global stream's NEXT value: exactly one randint was consumed
    random.seed(SEED_RANDOM); random.randint(5, 10)
    assert after == random.randint(0, 10 ** 9)
    assert len(lats) == 3 and len(lps) == 2 and len(tss) == 2
    f = lambda a: a.float().numpy()
    out.update({"pe": f(pe), "ppe": f(ppe), "npe": f(npe), "nppe": f(nppe), "mix_noise": f(mix_noise), "noises": torch.stack(noises).numpy(),
                "image": f(image), "latents": f(torch.stack(lats, 1)), "log_probs": f(torch.stack(lps, 1)), "timesteps": f(torch.stack(tss, 1)),
                "meta": np.array([STEPS, B, target_idx, SEED_RANDOM, 1], dtype=np.int64),
                "scalars": np.array([GUIDANCE, NOISE_LEVEL], dtype=np.float64)})
    np.savez_compressed(os.path.join(HERE, "img2img.npz"), **out)
    print("img2img.npz: target_idx", target_idx, "steps run", nsteps, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
