"""The one denoise loop under the SD3 rollout entry points, and the pieces the img2img rollout shares with it.

``rollout`` is the body of ``pipeline_with_logprob_random``, ``pipeline_with_logprob`` and ``pipeline_with_logprob_new``
(sd3_pipeline_with_logprob_fast.py); ``flux_to_sd3_denoise_random`` (sd3_img2img_with_logprob.py) has its own short loop (other start, other
Philox offsets, fixed noise level, other recording rule) over the same helpers: ``cfg_embeddings``, ``hoist``, ``velocity``, ``output``.
``velocity`` holds the only copy of the ``cfg_two_streams`` schedule.
"""
import random
import threading

import torch

from ..scheduler import retrieve_timesteps
from .sd3_sde_with_logprob import sde_step_cfg

NEED_EMBEDS = ("prompt strings need text encoders, which are outside the accelerated path "
               "(SURVEY.md 8a2 / f3): pass prompt_embeds / pooled_prompt_embeds")

_CFG_SIDES_LOCK = threading.Lock()


def cfg_embeddings(prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, device, guidance_scale,
                   repeat=None):
    """-> (tem_pe, tem_ppe, do_cfg): the embeddings on ``device``, each repeated ``repeat`` times along the batch axis unless that is None
    (PF:551-554, :1009-1012), the negative rows in front of the positive ones when ``guidance_scale > 1`` (PF:598-599)."""
    def rows(t):
        t = t.to(device)
        return t if repeat is None else t.repeat(repeat, *[1] * (t.dim() - 1))
    pe, ppe = rows(prompt_embeds), rows(pooled_prompt_embeds)
    do_cfg = guidance_scale > 1
    if not do_cfg:
        return pe, ppe, do_cfg
    npe, nppe = rows(negative_prompt_embeds), rows(negative_pooled_prompt_embeds)
    return torch.cat([npe, pe], dim=0), torch.cat([nppe, ppe], dim=0), do_cfg


def hoist(transformer, timesteps, tem_pe, tem_ppe):
    """-> (mods_all, ctx_rows): what the transformer computes from the embeddings and the schedule alone, once per rollout.  None for a
    transformer without the method (the tests' stand-ins)."""
    # every adaLN modulation row of the rollout from ONE pass over the 1.5 GB modulation matrix (mmdit.precompute_mods:
    # bit for bit the rows the per-forward GEMM gives; rollout step 412.8 -> 409.6 ms on one box)
    pre = getattr(transformer, "precompute_mods", None)
    mods_all = pre(timesteps, tem_ppe) if pre is not None else None
    emb = getattr(transformer, "embed_context", None)
    ctx_rows = emb(tem_pe) if emb is not None else None                        # the context embedder is timestep-free as well
    return mods_all, ctx_rows


def velocity(pipe, latents, t, B, tem_pe, tem_ppe, mods, ctx_rows, do_cfg, joint_attention_kwargs=None):
    """One denoise step's transformer output on the CFG batch -> (vu, vt); vt is None without CFG.  ``latents``: the B rows as the
    transformer sees them (embedding dtype); ``mods``: that step's row of ``hoist``'s mods_all."""
    if do_cfg and getattr(pipe, "cfg_two_streams", False) and mods is not None and ctx_rows is not None:
        # optional schedule (config `sample.cfg_two_streams`, bench.py's `cfg_two_streams` leg; LABNOTES.md 6 round 5): the unconditional and the conditional half of the CFG batch are
        # independent until the combine -- two forwards of batch B on two HIP streams instead of one of batch 2 B (every row of
        # every kernel is independent of the others: the same bits)
        device = latents.device
        main = torch.cuda.current_stream(device)
        # one side stream per calling THREAD, created under a lock and kept together with the stream OBJECT it was made for (ADVICE r5:
        # a map keyed by the integer stream handle is mutated by concurrent rollout threads, and a handle re-used after its stream
        # was destroyed would alias the old entry)
        with _CFG_SIDES_LOCK:
            sides = pipe.__dict__.setdefault("_cfg_sides", {})
            ent = sides.get(threading.get_ident())
            if ent is None or ent[0].cuda_stream != main.cuda_stream:
                ent = sides[threading.get_ident()] = (main, torch.cuda.Stream(device=device))
        side = ent[1]
        Nt = tem_pe.shape[1]
        # a prompt mask (Qwen-Image: joint_attention_kwargs["encoder_hidden_states_mask"], [2 B, Nt]) is split like the embeddings
        mask = (joint_attention_kwargs or {}).get("encoder_hidden_states_mask")
        half = (lambda lo, hi: {}) if mask is None else \
            (lambda lo, hi: {"joint_attention_kwargs": dict(joint_attention_kwargs, encoder_hidden_states_mask=mask[lo:hi])})
        # the modulation rows: one per sample of the CFG batch (SD3: the pooled embedding enters them), or ONE shared row (Qwen-Image:
        # the timestep alone), which serves both halves as it is -- slicing it [B:] would hand the conditional half an empty tensor
        mods_u, mods_t = (mods[:B], mods[B:]) if mods.shape[0] == 2 * B else (mods, mods)
        ready = torch.cuda.Event()
        ready.record(main)
        side.wait_event(ready)
        with torch.cuda.stream(side):
            vt = pipe.transformer(hidden_states=latents, timestep=t.expand(B), encoder_hidden_states=tem_pe[B:], pooled_projections=tem_ppe[B:],
                                  return_dict=False, mods=mods_t, context=ctx_rows[B * Nt:], **half(B, 2 * B))[0]
        latents.record_stream(side)
        vu = pipe.transformer(hidden_states=latents, timestep=t.expand(B), encoder_hidden_states=tem_pe[:B], pooled_projections=tem_ppe[:B],
                              return_dict=False, mods=mods_u, context=ctx_rows[:B * Nt], **half(0, B))[0]
        main.wait_stream(side)
        vt.record_stream(main)
        return vu, vt
    inp = torch.cat([latents] * 2) if do_cfg else latents                      # PF:625
    v = pipe.transformer(hidden_states=inp, timestep=t.expand(inp.shape[0]), encoder_hidden_states=tem_pe,
                         pooled_projections=tem_ppe, joint_attention_kwargs=joint_attention_kwargs,
                         return_dict=False, **({} if mods is None else {"mods": mods}),
                         **({} if ctx_rows is None else {"context": ctx_rows}))[0]                                     # PF:630-637
    return (v[:B], v[B:]) if do_cfg else (v, None)


def output(pipe, latents, output_type, pil):
    """The first member of a rollout's return tuple: the [0, 1] image tensor, or a list of PIL images for ``"pil"`` where the entry point
    converts (``pil``), or for ``"latent"`` the final latents undecoded."""
    if output_type == "latent":
        # diffusers' StableDiffusion3Pipeline.__call__ option (`if output_type == "latent": image = latents`) that the reference's trimmed copy
        # of the function dropped: the final latents are returned undecoded so that the caller can run `self.vae.decode_to_image` wherever
        # it schedules the reward computation (bench.py / Trainer: inside the reward future, beside the next group's rollout)
        return latents
    image = pipe.vae.decode_to_image(latents)                                  # PF:667-670 (rescale, decode, postprocess)
    if pil and output_type == "pil":
        from PIL import Image
        arr = (image.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        image = [Image.fromarray(a) for a in arr]
    return image


def rollout(self, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
            num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type, joint_attention_kwargs,
            noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed, *, branch, keep_f32,
            sde_type="cps", cfg_rescale=False):
    """The denoise loop of the three text-to-image entry points, for P prompts and G = mini_num_image_per_prompt samples of each.

    * ``branch=False`` (pipeline_with_logprob_random): the embeddings repeated G times up front, P * G initial latents, every step on
      P * G rows.
    * ``branch=True`` (pipeline_with_logprob / _new): P initial latents through the prefix; at step ``random_timestep`` the transformer
      still runs on the P rows, the SDE step fans each out to G (``copies=G``) and the embeddings, modulation and context rows are
      gathered to P * G rows for the steps after it.  ``output_type="pil"`` gives PIL images, the reference's default for these two
      (pipeline_with_logprob_random returns the tensor for every value but ``"latent"``).
    * ``keep_f32`` (pipeline_with_logprob): the latents stay float32 between steps and are rounded to the embedding dtype only at the
      transformer's door; otherwise the fused step's ``cast`` output is the next latent.
    * ``sde_type``: ``"cps"`` (Flow-CPS) or ``"sde"`` (Flow-SDE), handed to ``sde_step_cfg`` for every step.
    * ``cfg_rescale``: Qwen-Image's norm-rescaled true CFG instead of the SD3 combine in every step (``sde_step_cfg(cfg_rescale=True)``);
      not with ``branch``: the fan-out step has no rescaled form.  Without CFG (``guidance_scale <= 1``) it changes nothing.
    """
    if prompt_embeds is None:
        raise ValueError(NEED_EMBEDS)
    if cfg_rescale and branch:
        raise NotImplementedError("cfg_rescale with a branching rollout: the fan-out step (advgrpo_sde_step_branch) has no rescaled form")
    height = height or self.default_sample_size * self.vae_scale_factor
    width = width or self.default_sample_size * self.vae_scale_factor
    self._guidance_scale = guidance_scale
    device = self._execution_device
    G = int(mini_num_image_per_prompt)
    tem_pe, tem_ppe, do_cfg = cfg_embeddings(prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds,
                                             device, guidance_scale, repeat=None if branch else G)   # PF:551-554; not repeated: PF:114-123, :335-344
    dtype = prompt_embeds.dtype
    B = tem_ppe.shape[0] // (2 if do_cfg else 1)                               # rows of `latents`: P before a branch step, P * G otherwise
    if latents is None and generator is not None and seed is None:
        # the eval loop's path (TP:298-299,319): initial latents from the caller's torch generator exactly as diffusers'
        # prepare_latents / randn_tensor draws them (a CPU generator draws on the CPU in the embedding dtype, then moves)
        gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
        shape = (B, self.transformer.config.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    if latents is None:                                                        # PF:559-568, :114-123, :335-344 prepare_latents
        latents = self.prepare_latents(B, self.transformer.config.in_channels, height, width, dtype, device, seed)
    lat_dtype = torch.float32 if keep_f32 else dtype
    latents = latents.to(device=device, dtype=dtype).to(lat_dtype)             # PF:123 `.float()` on the embedding-dtype draw
    timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device)   # PF:574, :129, :350
    # rollout-local view of the schedule: rollouts of other prompt groups run at the same time on other streams / host
    # threads (trainer.sample_epoch) and re-install the scheduler's tables; this call keeps the objects it started with
    sigma_table = self.scheduler.sigmas
    if random_timestep is None:                                                # PF:585-586: random.seed(process_index); randint
        random_timestep = random.Random(process_index).randint(0, sample_num_steps // 2)   # same draw, no global reseed
    self.last_random_timestep = random_timestep    # host int, per calling thread (pipeline.py): first recorded scheduler index
    r = random_timestep
    all_latents, all_log_probs, all_timesteps = [], [], []
    n_per = latents[0].numel()
    # One Philox key per rollout call, disjoint counter ranges per draw, laid out for the P * G rows of the window whether or not the
    # rollout starts with them: the initial latents use counters from 0, the epsilon of denoise step i the range
    # [(1 + i) * ctr, (2 + i) * ctr).  (Separate keys seed + 1 + i per step made rank r + 1's latents equal rank r's step-0 noise
    # whenever callers numbered their ranks' seeds consecutively.)  With G == 1 a branching rollout draws the numbers of the plain one.
    ctr = (B * (G if branch else 1) * n_per + 3) // 4 + 1
    mods_all, ctx_rows = hoist(self.transformer, timesteps, tem_pe, tem_ppe)   # with `branch`: for the P-row CFG batch
    want_f32 = lat_dtype == torch.float32
    for i in range(len(timesteps)):
        t = timesteps[i]
        copies = G if branch and i == r else None
        if i == r:                                                             # PF:606-623, :160-171, :382-393
            cur = noise_level
            all_latents.append(latents if copies is None else latents.repeat(G, 1, 1, 1))
        elif r < i < r + train_num_steps:
            cur = noise_level
        else:
            cur = 0
        vu, vt = velocity(self, latents.to(dtype), t, B, tem_pe, tem_ppe, None if mods_all is None else mods_all[i], ctx_rows, do_cfg,
                          joint_attention_kwargs)
        # at a branch step the transformer ran on the P un-repeated rows (G identical copies of a row give G identical velocities); the step fans out
        nxt, cast, log_prob, _, _ = sde_step_cfg(                              # PF:640-655, :192-204, :414-429 fused
            self.scheduler, vu, vt, guidance_scale, None, latents, cur,
            noise=None if noises is None else noises[i], seed=seed, offset=(1 + i) * ctr,
            out_dtype=None if want_f32 else lat_dtype, want_mean=False, step_index=i, sigmas=sigma_table, copies=copies, sde_type=sde_type,
            **({"cfg_rescale": True} if cfg_rescale else {}))
        latents = nxt if want_f32 else cast
        if copies is not None:                                                 # PF:163-170, :385-392: the embeddings follow the latents
            P, B = B, B * G
            rows = torch.arange(B, device=device) % P
            if do_cfg:
                rows = torch.cat([rows, P + rows])
            tem_pe, tem_ppe = tem_pe[rows], tem_ppe[rows]                      # = cat([npe.repeat(G, 1, 1), pe.repeat(G, 1, 1)]), ...
            if mods_all is not None:                                           # every row of the modulation GEMM and of the context embedder is
                mods_all = mods_all[:, rows]                                   # independent of the batch it was computed in: gathered, not recomputed
            if ctx_rows is not None:
                Nt = tem_pe.shape[1]
                ctx_rows = ctx_rows.view(-1, Nt, ctx_rows.shape[-1])[rows].reshape(-1, ctx_rows.shape[-1])
        if r <= i < r + train_num_steps:                                       # PF:657-660, :209-212, :431-434
            all_latents.append(latents)
            all_log_probs.append(log_prob)
            all_timesteps.append(t.repeat(B))
    return output(self, latents, output_type, pil=branch), all_latents, all_log_probs, all_timesteps
