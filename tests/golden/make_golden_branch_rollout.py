#!/usr/bin/env python3
"""Generate tests/golden/branch_rollout.npz by RUNNING THE REFERENCE'S OWN pipeline_with_logprob / pipeline_with_logprob_new.

Runs only where the reference checkout is present (no test imports this file).  Nothing of the reference is copied: its module is imported
behind the import shims of make_golden.py and only numeric inputs / outputs are stored, plus the two functions' keyword names and the
repr() of their defaults (what the host test compares our signatures with).  Stand-ins, as in make_golden.py: oracle.scheduler for the
scheduler object, oracle.standin.StandinVelocity for the transformer, standin_vae_decode for vae.decode.

One stand-in detail is this file's own.  pipeline_with_logprob keeps its latents in float32 and hands them to the transformer as they are;
the reference's call sites run under autocast, where a bf16 transformer rounds them at its first layer.  StandinVelocity follows the dtype
of ``hidden_states`` and would mix float32 latents with bf16 embeddings, so the transformer handed to the reference rounds
``hidden_states`` to the embedding dtype at its door and is StandinVelocity from there on (a no-op wherever the two dtypes agree).

Every run: P = 2 prompts, G = 3 images per prompt, T = 6 steps, train_num_steps = 2, 16 x 8 x 8 latents; both functions x fp32 / bf16
embeddings x random_timestep in {0, 2}; one more run per function with random_timestep=None and process_index=1 pins the draw.
The epsilon of every step is the global torch stream's, replayed here from the same seed with the reference's own draw shapes (P rows
before the branch step, P * G rows from it on); runs with the same branch step r drew the same numbers, stored once as ``noise/r<r>/<step>``.
``<run>/meta`` = [steps, train_num_steps, P, G, height, branch step, process_index, the random_timestep argument or -1 for None].

The file is written with fixed zip timestamps: running this twice gives the same bytes.

Usage:  python tests/golden/make_golden_branch_rollout.py
"""
import contextlib
import inspect
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (shims, paths)
from oracle.scheduler import FlowMatchEulerScheduler  # noqa: E402
from oracle.standin import StandinVelocity, standin_vae_decode  # noqa: E402

P, G, STEPS, T, HW, GUIDANCE, NOISE_LEVEL = 2, 3, 6, 2, 64, 4.5, 0.8
SEED_EMBEDS, SEED_NOISE = 29, 131


class DoorCast(torch.nn.Module):
    """StandinVelocity behind the rounding of the latents to the embedding dtype (see the module docstring)."""

    def __init__(self):
        super().__init__()
        self.net = StandinVelocity()
        self.config = types.SimpleNamespace(in_channels=16)

    def forward(self, hidden_states, timestep, encoder_hidden_states, pooled_projections, joint_attention_kwargs=None, return_dict=False):
        return self.net(hidden_states.to(encoder_hidden_states.dtype), timestep, encoder_hidden_states, pooled_projections)


def make_pipe(lat0):
    class Pipe:
        default_sample_size = HW // 8
        vae_scale_factor = 8
        _execution_device = "cpu"

        def check_inputs(self, *a, **k): pass

        def encode_prompt(self, **k):
            return (k["prompt_embeds"], k["negative_prompt_embeds"], k["pooled_prompt_embeds"], k["negative_pooled_prompt_embeds"])

        def prepare_latents(self, b, c, h, w, dt, device, generator, latents):
            assert b == P and (h, w) == (HW, HW)
            return lat0.to(dt)

        @property
        def do_classifier_free_guidance(self): return self._guidance_scale > 1

        @property
        def guidance_scale(self): return self._guidance_scale

        @property
        def clip_skip(self): return self._clip_skip

        @property
        def joint_attention_kwargs(self): return self._joint_attention_kwargs

        def progress_bar(self, total=None):
            class PB:
                def update(s): pass
            return contextlib.nullcontext(PB())

        def maybe_free_model_hooks(self): pass
    pipe = Pipe()
    pipe.transformer = DoorCast()
    pipe.scheduler = FlowMatchEulerScheduler()
    pipe.vae = types.SimpleNamespace(config=types.SimpleNamespace(scaling_factor=1.5305, shift_factor=0.0609), dtype=torch.float32,
                                     decode=lambda z, return_dict=False: (standin_vae_decode(z),))
    pipe.image_processor = types.SimpleNamespace(postprocess=lambda im, output_type="pt": (im / 2 + 0.5).clamp(0, 1))
    return pipe


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the wall clock into every zip member)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    mg.install_shims()
    import random
    from adv_grpo.diffusers_patch import sd3_pipeline_with_logprob_fast as PF
    fns = {"plain": PF.pipeline_with_logprob, "new": PF.pipeline_with_logprob_new}
    out = {}
    for fname, fn in fns.items():
        params = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
        out[f"signature/{fname}/names"] = np.array([p.name for p in params])
        out[f"signature/{fname}/defaults"] = np.array([repr(p.default) for p in params])
    f = lambda a: a.float().numpy()
    shape = lambda rows: (rows, 16, HW // 8, HW // 8)
    runs = [(fname, dname, dtype, r, 0) for fname in fns for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)) for r in (0, 2)]
    runs += [(fname, "bf16", torch.bfloat16, None, 1) for fname in fns]
    for fname, dname, dtype, r, process_index in runs:
        g = torch.Generator().manual_seed(SEED_EMBEDS)
        pe = torch.randn(P, 5, 32, generator=g).to(dtype); ppe = torch.randn(P, 16, generator=g).to(dtype)
        npe = torch.randn(P, 5, 32, generator=g).to(dtype); nppe = torch.randn(P, 16, generator=g).to(dtype)
        lat0 = torch.randn(shape(P), generator=g)
        pipe = make_pipe(lat0)
        drawn = r if r is not None else random.Random(process_index).randint(0, STEPS // 2)     # PF:140-142 with random.seed(process_index)
        torch.manual_seed(SEED_NOISE)
        noises = [torch.randn(shape(P if i < drawn else P * G)) for i in range(STEPS)]
        torch.manual_seed(SEED_NOISE)
        with torch.no_grad():
            image, lats, lps, tss = fns[fname](
                pipe, prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=nppe,
                num_inference_steps=STEPS, guidance_scale=GUIDANCE, output_type="pt", height=HW, width=HW, noise_level=NOISE_LEVEL,
                mini_num_image_per_prompt=G, train_num_steps=T, process_index=process_index, sample_num_steps=STEPS, random_timestep=r)
        assert len(lats) == T + 1 and len(lps) == T and len(tss) == T, (len(lats), len(lps), len(tss))
        assert all(a.shape[0] == P * G for a in lats) and image.shape[0] == P * G
        want = torch.float32 if fname == "plain" else dtype
        assert all(a.dtype == want for a in lats), [a.dtype for a in lats]
        name = f"{fname}_{dname}_r{'draw' if r is None else r}"
        assert "lat0" not in out or np.array_equal(out["lat0"], f(lat0))
        out["lat0"] = f(lat0)                              # the same initial latents in every run
        out.update({f"{name}/pe": f(pe), f"{name}/ppe": f(ppe), f"{name}/npe": f(npe), f"{name}/nppe": f(nppe),
                    f"{name}/image": f(image), f"{name}/latents": f(torch.stack(lats, 1)), f"{name}/log_probs": f(torch.stack(lps, 1)),
                    f"{name}/timesteps": f(torch.stack(tss, 1)),
                    f"{name}/meta": np.array([STEPS, T, P, G, HW, drawn, process_index, -1 if r is None else r], dtype=np.int64),
                    f"{name}/scalars": np.array([GUIDANCE, NOISE_LEVEL], dtype=np.float64)})
        for i, e in enumerate(noises):                     # a function of the seed and of the draw shapes alone: stored once per branch step
            key = f"noise/r{drawn}/{i}"
            assert key not in out or np.array_equal(out[key], e.numpy())
            out[key] = e.numpy()
        print(name, "branch step", drawn, "latents", tuple(torch.stack(lats, 1).shape), lats[0].dtype)
    path = os.path.join(HERE, "branch_rollout.npz")
    save_npz(path, out)
    print("branch_rollout.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
