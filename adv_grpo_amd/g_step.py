"""One G-step micro-batch: compute_log_prob with gradient -> clipped GRPO loss -> backward into the LoRA grads.

Mirror of the inner training loop body, scripts/train_sd3_fast_pickscore.py:1102-1165 (beta == 0 in every shipped config;
beta > 0 adds the KL term of TP:1105-1108,1126-1130 against the adapter-free transformer): compute_log_prob (TP:233-267) = transformer on the CFG batch + CFG combine + SDE step in replay mode;
loss block TP:1111-1130; accelerator.backward(loss) TP:1165.  The backward is explicit:
d loss/d log_prob (grpo_loss kernel) -> d/d v_uncond, d/d v_text (sde_step_bwd kernel) -> MMDiT backward."""
import torch

from . import losses
from .diffusers_patch.sd3_sde_with_logprob import sde_step_cfg, sde_step_cfg_bwd


@torch.no_grad()
def micro_step(model, scheduler, sample, j, embeds, pooled_embeds, old_log_prob, advantages, *, guidance_scale,
               noise_level, adv_clip_max, clip_range, loss_scale=1.0, step_index=None, beta=0.0, sde_type="cps", embeds_mask=None,
               cfg_rescale=False):
    """sample: dict with latents / next_latents [G,T,16,h,w], timesteps [G,T].  embeds / pooled: CFG-concatenated
    (negative first, TP:1084-1091).  Accumulates into model.grads; returns the diagnostics of TP:1132-1162.
    step_index: scheduler index of timestep j, carried on the host by the caller (the rollout knows it); without it the
    index is looked up from the timestep value as the reference does (scheduler.index_for_timestep, SDE:106-110), which
    costs a device -> host copy per micro-step.
    beta > 0: a second, gradient-free forward with the adapters disabled gives prev_sample_mean_ref;
    loss = policy_loss + beta * mean((prev_sample_mean - prev_sample_mean_ref)^2) and "kl_loss" joins the diagnostics.
    sde_type: the step the rollout recorded its log-probs with -- "cps" (Flow-CPS) or "sde" (Flow-SDE, SDE:13-73): the replay forward, the
    reference mean and both backward entries follow it.  `scheduler.sigmas` must be the table the rollout recorded with (Trainer.g_step
    re-installs it with set_timesteps(sample.num_steps) before the first micro-step): `step_index` indexes it, and Flow-SDE's sigma_max
    = sigmas[1] depends on the number of steps as well.
    embeds_mask: the prompt mask of `embeds` ([2 G, Nt], same row order; Qwen-Image), handed to forward_train as encoder_hidden_states_mask
    and to the reference forward; None: nothing is passed.
    cfg_rescale: the rollout combined its predictions with Qwen-Image's norm-rescaled true CFG (sde_step_cfg(cfg_rescale=True)): the
    replay forward, the reference mean and the backward (sde_step_cfg_bwd, whose gradient then passes through the norm ratio) do too."""
    x = sample["latents"][:, j].contiguous()
    nxt = sample["next_latents"][:, j].contiguous()
    ts = sample["timesteps"][:, j]
    G = x.shape[0]
    mask_kw = {} if embeds_mask is None else {"encoder_hidden_states_mask": embeds_mask}
    v, ctx = model.forward_train(torch.cat([x, x]), torch.cat([ts, ts]).float(), embeds, pooled_embeds, **mask_kw)
    vu, vt = v[:G].contiguous(), v[G:].contiguous()
    rescale_kw = {"cfg_rescale": True} if cfg_rescale else {}
    if step_index is None:
        step_index = scheduler.index_for_timestep(float(ts[0]))
    _, _, log_prob, _, _ = sde_step_cfg(scheduler, vu, vt, guidance_scale, None, x, noise_level, prev_sample=nxt,
                                        want_mean=False, step_index=step_index, sde_type=sde_type, **rescale_kw)
    mean_ref = None
    if beta > 0:
        v_ref = model.forward_reference(torch.cat([x, x]), torch.cat([ts, ts]).float(), embeds, pooled_embeds,
                                        **({} if embeds_mask is None else {"joint_attention_kwargs": mask_kw}))
        _, _, _, mean_ref, _ = sde_step_cfg(scheduler, v_ref[:G].contiguous(), v_ref[G:].contiguous(), guidance_scale, None, x,
                                            noise_level, prev_sample=nxt, want_mean=True, step_index=step_index, sde_type=sde_type, **rescale_kw)
    scal, dlp = losses.grpo_loss(log_prob, old_log_prob, advantages, adv_clip_max, clip_range)
    if loss_scale != 1.0:
        dlp = dlp * loss_scale
    gu, gt, kl = sde_step_cfg_bwd(scheduler, vu, vt, guidance_scale, x, noise_level, nxt, dlp, step_index, mean_ref=mean_ref,
                                  kl_weight=float(beta) * float(loss_scale), sde_type=sde_type, cfg_rescale=cfg_rescale)
    model.backward(ctx, torch.cat([gu, gt]))
    info = {"log_prob": log_prob, "scalars": scal, **{k: scal[i] for i, k in enumerate(losses.INFO_KEYS)}}
    if kl is not None:                                   # TP:1126-1130,1158-1160
        info["kl_loss"] = kl.mean()
        info["loss"] = info["policy_loss"] + beta * info["kl_loss"]
    return info
