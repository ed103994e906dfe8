"""Full-trajectory SD3 rollout with per-step log-prob on the gfx950 kernels.

Drop-in for ``pipeline_with_logprob`` of adv_grpo/diffusers_patch/sd3_pipeline_with_logprob.py:11-198 (PFull): the reference's keyword names
and defaults plus the project's ``noises=``, ``seed=`` and ``sde_type=``, the same return tuple ``(image, all_latents, all_log_probs)``.
Every step is stochastic at ``noise_level`` and every step is recorded -- the form ``inference_t2i.py`` and the Flow-GRPO recipes build on.
The windowed rollouts (sd3_pipeline_with_logprob_fast.py) record ``train_num_steps`` steps in the embedding dtype instead.

* ``all_latents[0]``: the initial latents in the embedding dtype (PFull:118-127, :142).
* ``all_latents[1:]``: the **float32** ``x'`` of each step, recorded before the cast; the next step continues from the cast to the embedding
  dtype (PFull:173-184).  The fused step writes both in one pass.  A replayed log-prob is computed from what was stored: on the last
  steps of a schedule, where the Flow-SDE noise scale is ~6e-3, bf16 storage alone would move it by ~2e-2.
* ``sde_type``: ``"cps"`` -- Flow-CPS, the step the reference's module imports (PFull:8) -- or ``"sde"`` (Flow-SDE, SDE:13-73).
* ``self.cfg_rescale`` (absent: off): Qwen-Image's norm-rescaled true CFG instead of the SD3 combine in every step (``sde_step_cfg``).  The
  keyword list above is pinned, so the switch travels on the pipeline object, as ``sde_type`` does for the branching rollouts.
* Philox counters as in the windowed rollouts: the initial latents from 0, the epsilon of step i in ``[(1 + i) * ctr, (2 + i) * ctr)``.
"""
import torch

from ..scheduler import retrieve_timesteps
from ._rollout import NEED_EMBEDS, cfg_embeddings, hoist, output, velocity
from .sd3_sde_with_logprob import sde_step_cfg


@torch.no_grad()
def pipeline_with_logprob(self, prompt=None, prompt_2=None, prompt_3=None, height=None, width=None, num_inference_steps=28,
                          sigmas=None, guidance_scale=7.0, negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None,
                          num_images_per_prompt=1, generator=None, latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                          pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pil",
                          joint_attention_kwargs=None, clip_skip=None, callback_on_step_end_tensor_inputs=["latents"],
                          max_sequence_length=256, skip_layer_guidance_scale=2.8, noise_level=0.7, noises=None, seed=None,
                          sde_type="cps"):
    if prompt_embeds is None:
        raise ValueError(NEED_EMBEDS)
    if num_images_per_prompt != 1:
        # encode_prompt repeats what it encodes from strings; embeddings handed in are used as they are (PFull:84-101)
        raise ValueError("pipeline_with_logprob: with prompt_embeds, repeat the embeddings instead of passing num_images_per_prompt")
    height = height or self.default_sample_size * self.vae_scale_factor
    width = width or self.default_sample_size * self.vae_scale_factor
    self._guidance_scale = guidance_scale
    device = self._execution_device
    tem_pe, tem_ppe, do_cfg = cfg_embeddings(prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds,
                                             device, guidance_scale)                                 # PFull:102-104
    dtype = prompt_embeds.dtype
    B = prompt_embeds.shape[0]
    if latents is None and generator is not None and seed is None:             # as _rollout.rollout: the caller's torch generator, diffusers' draw
        gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
        shape = (B, self.transformer.config.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    if latents is None:                                                        # PFull:118-127 prepare_latents
        latents = self.prepare_latents(B, self.transformer.config.in_channels, height, width, dtype, device, seed)
    latents = latents.to(device=device, dtype=dtype)
    timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device)   # PFull:131-137
    sigma_table = self.scheduler.sigmas                                        # rollout-local view (see _rollout.rollout)
    all_latents, all_log_probs = [latents], []                                 # PFull:142-143
    cfg_rescale = bool(getattr(self, "cfg_rescale", False))
    ctr = (latents.numel() + 3) // 4 + 1
    mods_all, ctx_rows = hoist(self.transformer, timesteps, tem_pe, tem_ppe)
    for i in range(len(timesteps)):
        vu, vt = velocity(self, latents, timesteps[i], B, tem_pe, tem_ppe, None if mods_all is None else mods_all[i], ctx_rows, do_cfg,
                          joint_attention_kwargs)                                                    # PFull:153-169
        nxt, cast, log_prob, _, _ = sde_step_cfg(                              # PFull:173-184 fused: the f32 sample and its cast
            self.scheduler, vu, vt, guidance_scale, None, latents, noise_level,
            noise=None if noises is None else noises[i], seed=seed, offset=(1 + i) * ctr,
            out_dtype=dtype, want_mean=False, step_index=i, sigmas=sigma_table, sde_type=sde_type,
            **({"cfg_rescale": True} if cfg_rescale else {}))
        all_latents.append(nxt)
        all_log_probs.append(log_prob)
        latents = nxt if cast is None else cast
    return output(self, latents, output_type, pil=True), all_latents, all_log_probs      # PFull:190-198
