"""SD3 rollout with per-step log-prob on the gfx950 kernels.

Drop-in for ``pipeline_with_logprob_random``
(adv_grpo/diffusers_patch/sd3_pipeline_with_logprob_fast.py:453-674): same keyword arguments, same return
tuple ``(image, all_latents, all_log_probs, all_timesteps)``, same cast order (SDE step in f32, latents stored
in the prompt-embedding dtype, log-prob from the pre-cast sample) and the same RNG call pattern (one epsilon
draw per step, also when noise_level == 0).  ``self`` is a pipeline object exposing ``transformer``,
``scheduler``, ``vae`` (see adv_grpo_amd/pipeline.py).

What changes underneath: per step ONE transformer call on the CFG batch, then ONE fused kernel for CFG
combine + SDE step + log-prob + cast (instead of ~12 torch kernels, a randn and two host syncs), epsilon from
an in-kernel Philox stream (or injected via ``noises=`` for parity tests), no ``index_for_timestep`` sync.

``pipeline_with_logprob`` (PF:16-229) and ``pipeline_with_logprob_new`` (PF:234-448) are the same module's BRANCHING rollouts: one latent
per prompt through the noise-free prefix, repeated ``mini_num_image_per_prompt`` times at the first SDE step.  The ``G`` samples of a group
share their initial noise and their prefix, so the group's spread comes from the SDE window alone -- that is how the reference defines them.

The three functions are three entry shapes of ONE denoise loop, ``_rollout.rollout``: without a branch step and with the embeddings repeated
``G`` times up front (``pipeline_with_logprob_random``), with the branch step and the fused ``cast`` output as the next latent
(``pipeline_with_logprob_new``), with the branch step and float32 latents between steps (``pipeline_with_logprob``).
"""
import torch

from ._rollout import rollout


@torch.no_grad()
def pipeline_with_logprob_random(self, prompt=None, prompt_2=None, prompt_3=None, height=None, width=None,
                                 num_inference_steps=28, mini_num_image_per_prompt=1, sigmas=None, guidance_scale=7.0,
                                 negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None, generator=None,
                                 latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                                 pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pt",
                                 joint_attention_kwargs=None, clip_skip=None,
                                 callback_on_step_end_tensor_inputs=("latents",), max_sequence_length=256,
                                 skip_layer_guidance_scale=2.8, noise_level=0.7, train_num_steps=1, process_index=0,
                                 sample_num_steps=10, random_timestep=None, noises=None, seed=None, sde_type="cps", cfg_rescale=False):
    """``sde_type``: ``"cps"`` (Flow-CPS, the reference's step for this rollout) or ``"sde"`` (Flow-SDE, SDE:13-73) for the steps of the window;
    the default reproduces the bits this function always gave.  ``cfg_rescale=True``: every step combines its two predictions with
    Qwen-Image's norm-rescaled true CFG (``sde_step_cfg``) instead of the SD3 combine; the latents must be [B, 16, H, W]."""
    return rollout(self, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                   num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type, joint_attention_kwargs,
                   noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed,
                   branch=False, keep_f32=False, sde_type=sde_type, cfg_rescale=cfg_rescale)


@torch.no_grad()
def pipeline_with_logprob_new(self, prompt=None, prompt_2=None, prompt_3=None, height=None, width=None,
                              num_inference_steps=28, mini_num_image_per_prompt=1, sigmas=None, guidance_scale=7.0,
                              negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None, generator=None,
                              latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                              pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pil",
                              joint_attention_kwargs=None, clip_skip=None,
                              callback_on_step_end_tensor_inputs=["latents"], max_sequence_length=256,
                              skip_layer_guidance_scale=2.8, noise_level=0.7, train_num_steps=1, process_index=0,
                              sample_num_steps=10, random_timestep=None, noises=None, seed=None):
    """Drop-in for the reference's branching rollout ``pipeline_with_logprob_new`` (PF:234-448): same keyword arguments and defaults (plus
    ``noises=`` / ``seed=`` as in pipeline_with_logprob_random), same return tuple.

    * ``P = prompt_embeds.shape[0]`` initial latents (PF:335-344); the embeddings are not repeated up front.
    * steps ``i < random_timestep``: noise level 0 on the P rows.
    * step ``i == random_timestep`` (PF:382-393): ``latents.repeat(G, 1, 1, 1)`` is recorded as the window's first latent and the four embedding
      tensors are repeated the same way.  The transformer runs on the P un-repeated rows and ``advgrpo_sde_step_branch`` writes the P * G next
      latents and log-probs: the bits of the literal repeat-then-forward, at 1 / G of that forward's rows.
    * ``random_timestep < i < random_timestep + train_num_steps``: noise level ``noise_level``; afterwards 0; all on P * G rows.
    * latents, log-probs and timesteps are recorded for the ``train_num_steps`` steps of the window (PF:431-434).
    * the stepped latents are cast back to the embedding dtype after every step (PF:428-429): the fused ``cast`` output.
    * ``random_timestep=None`` draws ``random.Random(process_index).randint(0, sample_num_steps // 2)`` (PF:361-363, without reseeding the
      global stream) and sets ``self.last_random_timestep``.
    * ``noises[i]``: P rows for ``i < random_timestep``, P * G rows from there on -- what the reference draws.  Philox counters as in
      pipeline_with_logprob_random for P * G rows, so ``mini_num_image_per_prompt=1`` returns that function's bits for the same ``seed``.
    * ``output_type``: ``"pil"`` (the reference's default) a list of PIL images, ``"latent"`` the final latents undecoded (as
      pipeline_with_logprob_random), anything else the [0, 1] image tensor.
    * the keyword list is the reference's plus ``noises`` / ``seed`` and nothing else, so the choice of step travels on the pipeline object,
      like ``cfg_two_streams``: ``self.sde_type`` = ``"cps"`` (the default when absent) or ``"sde"`` (Flow-SDE, SDE:13-73).
    * ``self.cfg_rescale`` (Qwen-Image's norm-rescaled true CFG) is read the same way and refused: the fan-out step has no rescaled form.
    The G samples of a group share their initial noise and prefix: the group's spread comes from the SDE window alone."""
    return rollout(self, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                   num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type, joint_attention_kwargs,
                   noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed,
                   branch=True, keep_f32=False, sde_type=getattr(self, "sde_type", "cps"), cfg_rescale=getattr(self, "cfg_rescale", False))


@torch.no_grad()
def pipeline_with_logprob(self, prompt=None, prompt_2=None, prompt_3=None, height=None, width=None,
                          num_inference_steps=28, mini_num_image_per_prompt=1, sigmas=None, guidance_scale=7.0,
                          negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None, generator=None,
                          latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                          pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pil",
                          joint_attention_kwargs=None, clip_skip=None,
                          callback_on_step_end_tensor_inputs=["latents"], max_sequence_length=256,
                          skip_layer_guidance_scale=2.8, noise_level=0.7, train_num_steps=1, process_index=0,
                          sample_num_steps=10, random_timestep=None, noises=None, seed=None):
    """Drop-in for the reference's branching rollout ``pipeline_with_logprob`` (PF:16-229).  Everything pipeline_with_logprob_new's
    docstring says holds, except the cast order: the initial latents are drawn in the embedding dtype and then ``.float()``-ed (PF:114-123)
    and the cast back after a step is commented out (PF:206-207), so the latents -- and every recorded ``all_latents`` entry -- stay float32
    through the whole rollout.  The transformer input is rounded to the embedding dtype at its door (the reference's call sites run under
    autocast); its output is combined (CFG) in that dtype and promoted to f32 for the step, as in the other rollouts."""
    return rollout(self, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                   num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type, joint_attention_kwargs,
                   noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed,
                   branch=True, keep_f32=True, sde_type=getattr(self, "sde_type", "cps"), cfg_rescale=getattr(self, "cfg_rescale", False))
