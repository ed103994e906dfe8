#!/usr/bin/env python3
"""Generate tests/golden/flow_sde.npz by RUNNING THE REFERENCE'S OWN sde_step_with_logprob (the Flow-SDE step, sd3_sde_with_logprob.py:13-73).

Runs only where the reference checkout is present (no test imports this file).  Nothing of the reference is copied: its module is imported
behind the import shims of make_golden.py and only numeric inputs / outputs are stored.  The scheduler object is oracle.scheduler.

Cases, all [2, 16, 8, 8] with seeded v, x and epsilon, noise_level 0.7: the 10-step schedule at index 0 (sigma == 1: the sigma_max branch of
:49), 1, 5 and 9 (sigma_prev == 0); the 4-step schedule at index 0 and 2.  One more case at noise_level 0 (10 steps, index 1) stores `next`
and `mean` only: its log-prob is NaN by construction.  Per case: v, x, eps, sigmas, meta = [steps, index, noise_level], next, mean,
std (std_dev_t), log_prob, and the replay log-prob (prev_sample=...) from the float32 `next` and from its bf16 rounding.

The file is written with fixed zip timestamps: running this twice gives the same bytes.

Usage:  python tests/golden/make_golden_flow_sde.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (shims, paths)
from make_golden_branch_rollout import save_npz  # noqa: E402
from oracle.scheduler import FlowMatchEulerScheduler  # noqa: E402

SHAPE = (2, 16, 8, 8)
CASES = [("s10_i0", 10, 0, 0.7), ("s10_i1", 10, 1, 0.7), ("s10_i5", 10, 5, 0.7), ("s10_i9", 10, 9, 0.7), ("s4_i0", 4, 0, 0.7),
         ("s4_i2", 4, 2, 0.7), ("s10_i1_nl0", 10, 1, 0.0)]


def main():
    mg.install_shims()
    from adv_grpo.diffusers_patch.sd3_sde_with_logprob import sde_step_with_logprob as ref_step
    out = {}
    for name, steps, idx, nl in CASES:
        sch = FlowMatchEulerScheduler()
        sch.set_timesteps(steps)
        g = torch.Generator().manual_seed(sum(map(ord, name)) + 7)
        v, x = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
        t = sch.timesteps[idx].repeat(SHAPE[0])
        torch.manual_seed(4321)
        eps = torch.randn(SHAPE)                              # what the reference draws from the global stream
        torch.manual_seed(4321)
        nxt, lp, mean, std = ref_step(sch, v, t, x, noise_level=nl)
        out.update({f"{name}/v": v.numpy(), f"{name}/x": x.numpy(), f"{name}/eps": eps.numpy(), f"{name}/sigmas": sch.sigmas.numpy(),
                    f"{name}/meta": np.array([steps, idx, nl], dtype=np.float64), f"{name}/next": nxt.numpy(), f"{name}/mean": mean.numpy()})
        if nl == 0:
            assert torch.equal(nxt, mean) and torch.isnan(lp).all()
            continue
        _, lp_f32, mean_r, _ = ref_step(sch, v, t, x, noise_level=nl, prev_sample=nxt)
        _, lp_bf16, _, _ = ref_step(sch, v, t, x, noise_level=nl, prev_sample=nxt.to(torch.bfloat16))
        assert torch.equal(mean_r, mean) and all(torch.isfinite(a).all() for a in (nxt, lp, mean, std, lp_f32, lp_bf16))
        out.update({f"{name}/std": std.reshape(-1).numpy(), f"{name}/log_prob": lp.numpy(), f"{name}/log_prob_replay_f32": lp_f32.numpy(),
                    f"{name}/log_prob_replay_bf16": lp_bf16.numpy()})
        print(name, "sigma", float(sch.sigmas[idx]), "std", std.reshape(-1).tolist(), "log_prob", lp.tolist(), "replay bf16", lp_bf16.tolist())
    path = os.path.join(HERE, "flow_sde.npz")
    save_npz(path, out)
    print("flow_sde.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
