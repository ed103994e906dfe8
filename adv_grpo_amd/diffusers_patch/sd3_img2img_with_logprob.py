"""SD3 rollouts that start from reference images, with per-step log-prob, on the gfx950 kernels.

Drop-ins for ``image_to_latent``, ``get_sigmas`` and ``flux_to_sd3_denoise_random``
(adv_grpo/diffusers_patch/sd3_pipeline_with_logprob_fast.py:686-717 and :914-1081): encode reference images with the SD3 VAE, noise them to
a drawn step of the schedule, denoise from there to the end with ``noise_level`` on every step, and record the start latents and the first
two steps in the format of ``pipeline_with_logprob_random``: ``(image, all_latents, all_log_probs, all_timesteps)`` with list lengths
3 / 2 / 2.  ``self`` / ``pipe`` is an adv_grpo_amd.pipeline.SD3Pipeline built with ``vae_encoder=``.

Same control flow, cast order and draw order as the reference: ONE ``random.randint(5, 10)`` on the global ``random`` module for the start
index; the encoded latents rounded to bf16 (PF:705), sigma taken from the schedule in bf16 and the mix ``(1 - sigma) * z + sigma * noise``
in bf16 arithmetic (PF:961-965); prompt embeddings repeated per image (PF:1009-1012); SDE step in f32, latents stored in bf16.
What changes underneath: the encoder chain is one C-ABI call and sampling + scaling + cast + forward noising one kernel launch
(vae_encoder.py), each denoise step one transformer call and one fused CFG + SDE + log-prob kernel (``sde_step_cfg``), epsilon from the
in-kernel Philox stream unless injected.  The latents keep the reference's convention ``sample * scaling_factor`` without ``- shift_factor``.

Keyword-only hooks for parity tests, defaulting to the reference's behaviour: ``target_idx`` (skips the randint), ``encode_noise`` (the VAE
sampling epsilon), ``mix_noise`` (the forward-noising draw), ``noises`` (per denoise step, indexed from the start step), ``seed`` and
``output_type="latent"``.

The denoise loop is its own (start offset, Philox offsets, fixed noise level and recording rule differ from ``_rollout.rollout``) over that
module's helpers.  ``pipe.cfg_two_streams`` (default false) is honoured as in the other rollouts: the two halves of the CFG batch as two
forwards on two HIP streams, with the same bits as one forward of twice the batch.
"""
import random

import torch

from .. import _lib
from ._rollout import NEED_EMBEDS, cfg_embeddings, hoist, output, velocity
from .sd3_sde_with_logprob import sde_step_cfg

NO_ENCODER = ("this SD3Pipeline was built without a VAE encoder: pass vae_encoder=AutoencoderKLEncoder(...) "
              "(adv_grpo_amd/vae_encoder.py) to start rollouts from images")


def _encoder(pipe):
    enc = getattr(pipe, "vae_encoder", None)
    if enc is None:
        raise RuntimeError(NO_ENCODER)
    return enc


def _host_images(images):
    """A PIL image or a list of them through the reference's host path: resize to 512 x 512 (torchvision's Resize default: bilinear,
    antialiased on PIL input), ToTensor -> uint8 [B,512,512,3] (the division by 255 and the Normalize run in the encoder's first kernel)."""
    import numpy as np
    from PIL import Image
    if isinstance(images, Image.Image):
        images = [images]
    arrs = [np.asarray(im.convert("RGB").resize((512, 512), Image.BILINEAR), dtype=np.uint8) for im in images]
    return torch.from_numpy(np.stack(arrs))


def _as_device_images(images, device):
    if isinstance(images, torch.Tensor):
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"image_to_latent: a tensor of images must be [B,3,H,W] in [0,1], got {tuple(images.shape)}")
        return images.to(device)
    return _host_images(images).to(device)


def image_to_latent(pipe, images, device="cuda", *, seed=None, noise=None, sample=True):
    """PIL image / list (resized to 512 x 512 on the host, PF:691-699) or a device tensor [B,3,H,W] in [0,1] (taken as is) ->
    ``vae.encode(2 x - 1).latent_dist.sample() * scaling_factor`` as bf16 [B,C,H/8,W/8] (PF:703-705)."""
    enc = _encoder(pipe)
    return enc.encode(_as_device_images(images, device), seed=seed, noise=noise, sample=sample, out_dtype=torch.bfloat16)


def get_sigmas(noise_scheduler, timesteps, device, n_dim=4, dtype=torch.float32):
    """sigma of each timestep, looked up on the installed schedule, shaped [len, 1, ...] with n_dim axes (PF:708-717).  The index is resolved
    on the host copy of the schedule where the scheduler has one (no device sync per timestep)."""
    sigmas = noise_scheduler.sigmas.to(device=device, dtype=dtype)
    if hasattr(noise_scheduler, "index_for_timestep") and hasattr(noise_scheduler, "_timesteps_host"):
        idx = [noise_scheduler.index_for_timestep(float(t)) for t in timesteps.reshape(-1).tolist()]
    else:
        sched = noise_scheduler.timesteps.to(device)
        idx = [(sched == t).nonzero().item() for t in timesteps.to(device)]
    sigma = sigmas[idx].flatten()
    while sigma.dim() < n_dim:
        sigma = sigma.unsqueeze(-1)
    return sigma


def start_index(timesteps, t):
    """Index of the first denoise step for start time t: the LAST schedule entry that is >= t (PF:1025).  timesteps: descending sequence."""
    hits = [i for i, v in enumerate(timesteps) if float(v) >= float(t)]
    if not hits:
        raise ValueError(f"start time {float(t)} is above the schedule")
    return hits[-1]


def draw_target_idx():
    """The reference's start-step draw: one call on the GLOBAL random module (PF:958)."""
    return random.randint(5, 10)


@torch.no_grad()
def flux_to_sd3_denoise_random(self, prompt=None, prompt_2=None, prompt_3=None, flux_images=None, device="cuda", output_type="pt",
                               num_inference_steps=20, guidance_scale=7.0, negative_prompt=None, negative_prompt_2=None,
                               negative_prompt_3=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
                               negative_pooled_prompt_embeds=None, max_sequence_length=256, noise_level=0.7, random_timestep=None,
                               noise_timestep_ratio=0.4, clip_skip=None, *, target_idx=None, encode_noise=None, mix_noise=None,
                               noises=None, seed=None):
    enc = _encoder(self)
    if prompt_embeds is None:
        raise ValueError(NEED_EMBEDS)
    if flux_images is None:
        raise ValueError("flux_to_sd3_denoise_random: flux_images (PIL images or a [B,3,H,W] tensor in [0,1]) is required")
    self._guidance_scale = guidance_scale
    device = self._execution_device if device == "cuda" else torch.device(device)
    images = _as_device_images(flux_images, device)
    sched = self.scheduler
    sched.set_timesteps(num_inference_steps, device=device)                    # PF:948-949
    timesteps, sigma_table = sched.timesteps, sched.sigmas                     # rollout-local view (see _rollout.rollout)
    ts_host = [float(v) for v in sched._timesteps_host] if hasattr(sched, "_timesteps_host") else timesteps.tolist()
    if target_idx is None:
        target_idx = draw_target_idx()                                         # PF:958
    target_idx = int(target_idx)
    if not 0 <= target_idx < len(ts_host):
        raise ValueError(f"flux_to_sd3_denoise_random: start step {target_idx} is outside a schedule of {len(ts_host)} steps "
                         f"(the reference draws it from 5 .. 10: use num_inference_steps > 10)")
    start = start_index(ts_host, ts_host[target_idx])                          # PF:1025
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    # ---- encode, round to bf16, noise to sigma[target_idx] in bf16 arithmetic (PF:942, :961-965)
    sigma = sigma_table[target_idx:target_idx + 1].to(torch.float32)
    if hasattr(enc, "encode_and_noise"):
        _, latents = enc.encode_and_noise(images, sigma, seed=seed, noise=encode_noise, mix_noise=mix_noise)
    else:
        # an encoder object with encode() only (the stand-in of the parity test): the same mix as separate bf16 torch operations
        z = enc.encode(images, seed=seed, noise=encode_noise, out_dtype=torch.bfloat16)
        if mix_noise is None:
            mix_noise = torch.empty_like(z)
            _lib.check(_lib.load().advgrpo_randn(mix_noise.data_ptr(), _lib.BF16, mix_noise.numel(), int(seed), (z.numel() + 3) // 4 + 1,
                                                 _lib.stream_ptr()))
        sg = sigma.to(torch.bfloat16).view(1, 1, 1, 1)
        latents = (1.0 - sg) * z + sg * mix_noise.to(device=device, dtype=torch.bfloat16)
    B = latents.shape[0]
    dtype = latents.dtype
    tem_pe, tem_ppe, do_cfg = cfg_embeddings(prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds,
                                             device, guidance_scale, repeat=B)                       # PF:1009-1012
    run = timesteps[start:]                                                    # PF:1026
    all_latents, all_log_probs, all_timesteps = [], [], []
    ctr = (latents.numel() + 3) // 4 + 1      # Philox counters: [0, ctr) the VAE sampling draw, [ctr, 2 ctr) the mix, then one range per step
    mods_all, ctx_rows = hoist(self.transformer, run, tem_pe, tem_ppe)
    for k in range(len(run)):
        t = run[k]
        if k == 0:
            all_latents.append(latents)                                        # PF:1032-1033
        vu, vt = velocity(self, latents, t, B, tem_pe, tem_ppe, None if mods_all is None else mods_all[k], ctx_rows, do_cfg)
        _, cast, log_prob, _, _ = sde_step_cfg(sched, vu, vt, guidance_scale, None, latents, noise_level,       # PF:1055-1063
                                               noise=None if noises is None else noises[k], seed=seed, offset=(2 + k) * ctr,
                                               out_dtype=dtype, want_mean=False, step_index=start + k, sigmas=sigma_table)
        latents = cast
        if k < 2:                                                              # PF:1066-1070
            all_latents.append(latents)
            all_log_probs.append(log_prob)
            all_timesteps.append(t.repeat(B))
    return output(self, latents, output_type, pil=True), all_latents, all_log_probs, all_timesteps      # PF:1074-1079
