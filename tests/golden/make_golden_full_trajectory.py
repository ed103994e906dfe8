#!/usr/bin/env python3
"""Generate tests/golden/full_trajectory.npz by RUNNING THE REFERENCE'S OWN full-trajectory pipeline_with_logprob
(adv_grpo/diffusers_patch/sd3_pipeline_with_logprob.py:11-198).

Runs only where the reference checkout is present (no test imports this file).  Nothing of the reference is copied: its module is imported
behind the import shims of make_golden.py and only numeric inputs / outputs are stored, plus the function's keyword names and the repr() of
their defaults.  The fake pipeline object and the stand-in transformer are those of make_golden_branch_rollout.py (imported).

Every run: 2 prompts, 4 steps, 16 x 8 x 8 latents, noise_level 0.7; fp32 / bf16 embeddings x guidance 4.5 / 1.0 (without CFG).  Stored per run:
the embeddings, every latent (the initial one and the float32 sample of each step), every log-prob and the image; the epsilon of each step
is the global torch stream's, replayed here from the same seed and stored once (``noise/<step>``), as are the initial latents (``lat0``).

The file is written with fixed zip timestamps: running this twice gives the same bytes.

Usage:  python tests/golden/make_golden_full_trajectory.py
"""
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (shims, paths)
import make_golden_branch_rollout as br  # noqa: E402  (make_pipe, save_npz, P, HW)

STEPS, NOISE_LEVEL = 4, 0.7
SEED_EMBEDS, SEED_NOISE = 31, 137


def main():
    mg.install_shims()
    from adv_grpo.diffusers_patch import sd3_pipeline_with_logprob as PFULL
    fn = PFULL.pipeline_with_logprob
    params = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
    out = {"signature/names": np.array([p.name for p in params]), "signature/defaults": np.array([repr(p.default) for p in params])}
    f = lambda a: a.float().numpy()
    shape = (br.P, 16, br.HW // 8, br.HW // 8)
    for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for gname, guidance in (("cfg", 4.5), ("nocfg", 1.0)):
            g = torch.Generator().manual_seed(SEED_EMBEDS)
            pe = torch.randn(br.P, 5, 32, generator=g).to(dtype); ppe = torch.randn(br.P, 16, generator=g).to(dtype)
            npe = torch.randn(br.P, 5, 32, generator=g).to(dtype); nppe = torch.randn(br.P, 16, generator=g).to(dtype)
            lat0 = torch.randn(shape, generator=g)
            pipe = br.make_pipe(lat0)
            type(pipe).interrupt = property(lambda self: self._interrupt)        # (read by this function's loop only, PFull:149)
            torch.manual_seed(SEED_NOISE)
            noises = [torch.randn(shape) for _ in range(STEPS)]
            torch.manual_seed(SEED_NOISE)
            with torch.no_grad():
                image, lats, lps = fn(pipe, prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=npe,
                                      negative_pooled_prompt_embeds=nppe, num_inference_steps=STEPS, guidance_scale=guidance,
                                      output_type="pt", height=br.HW, width=br.HW, noise_level=NOISE_LEVEL)
            assert len(lats) == STEPS + 1 and len(lps) == STEPS and lats[0].dtype == dtype
            assert all(a.dtype == torch.float32 for a in lats[1:]) and image.shape[0] == br.P
            name = f"{dname}_{gname}"
            for key, val in (("lat0", f(lat0)), *((f"noise/{i}", e.numpy()) for i, e in enumerate(noises))):
                assert key not in out or np.array_equal(out[key], val)          # the same draws in every run
                out[key] = val
            out.update({f"{name}/pe": f(pe), f"{name}/ppe": f(ppe), f"{name}/npe": f(npe), f"{name}/nppe": f(nppe), f"{name}/image": f(image),
                        f"{name}/latents": f(torch.stack(lats, 1)), f"{name}/log_probs": f(torch.stack(lps, 1)),
                        f"{name}/meta": np.array([STEPS, br.P, br.HW], dtype=np.int64),
                        f"{name}/scalars": np.array([guidance, NOISE_LEVEL], dtype=np.float64)})
            print(name, "latents", tuple(torch.stack(lats, 1).shape), "log_probs", torch.stack(lps, 1)[0].tolist())
    path = os.path.join(HERE, "full_trajectory.npz")
    br.save_npz(path, out)
    print("full_trajectory.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
