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
"""
import random
import threading

import torch

from ..scheduler import retrieve_timesteps
from .sd3_sde_with_logprob import sde_step_cfg

_CFG_SIDES_LOCK = threading.Lock()


@torch.no_grad()
def pipeline_with_logprob_random(self, prompt=None, prompt_2=None, prompt_3=None, height=None, width=None,
                                 num_inference_steps=28, mini_num_image_per_prompt=1, sigmas=None, guidance_scale=7.0,
                                 negative_prompt=None, negative_prompt_2=None, negative_prompt_3=None, generator=None,
                                 latents=None, prompt_embeds=None, negative_prompt_embeds=None,
                                 pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, output_type="pt",
                                 joint_attention_kwargs=None, clip_skip=None,
                                 callback_on_step_end_tensor_inputs=("latents",), max_sequence_length=256,
                                 skip_layer_guidance_scale=2.8, noise_level=0.7, train_num_steps=1, process_index=0,
                                 sample_num_steps=10, random_timestep=None, noises=None, seed=None):
    if prompt_embeds is None:
        raise ValueError("prompt strings need text encoders, which are outside the accelerated path "
                         "(SURVEY.md 8a2 / f3): pass prompt_embeds / pooled_prompt_embeds")
    height = height or self.default_sample_size * self.vae_scale_factor
    width = width or self.default_sample_size * self.vae_scale_factor
    self._guidance_scale = guidance_scale
    device = self._execution_device
    G = mini_num_image_per_prompt
    pe = prompt_embeds.to(device).repeat(G, 1, 1)                              # PF:551-554
    ppe = pooled_prompt_embeds.to(device).repeat(G, 1)
    do_cfg = guidance_scale > 1
    if do_cfg:
        npe = negative_prompt_embeds.to(device).repeat(G, 1, 1)
        nppe = negative_pooled_prompt_embeds.to(device).repeat(G, 1)
        tem_pe = torch.cat([npe, pe], dim=0)                                   # PF:598-599
        tem_ppe = torch.cat([nppe, ppe], dim=0)
    else:
        tem_pe, tem_ppe = pe, ppe
    dtype = prompt_embeds.dtype
    B = pe.shape[0]
    if latents is None and generator is not None and seed is None:
        # the eval loop's path (TP:298-299,319): initial latents from the caller's torch generator exactly as diffusers'
        # prepare_latents / randn_tensor draws them (a CPU generator draws on the CPU in the embedding dtype, then moves)
        gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
        shape = (B, self.transformer.config.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    if latents is None:                                                        # PF:559-568 prepare_latents
        latents = self.prepare_latents(B, self.transformer.config.in_channels, height, width, dtype, device, seed)
    latents = latents.to(device=device, dtype=dtype)
    timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device)   # PF:574
    # rollout-local view of the schedule: rollouts of other prompt groups run at the same time on other streams / host
    # threads (trainer.sample_epoch) and re-install the scheduler's tables; this call keeps the objects it started with
    sigma_table = self.scheduler.sigmas
    if random_timestep is None:                                                # PF:585-586: random.seed(process_index); randint
        random_timestep = random.Random(process_index).randint(0, sample_num_steps // 2)   # same draw, no global reseed
    self.last_random_timestep = random_timestep    # host int, per calling thread (pipeline.py): first recorded scheduler index
    all_latents, all_log_probs, all_timesteps = [], [], []
    n_per = latents[0].numel()
    # One Philox key per rollout call, disjoint counter ranges per draw: the initial latents use counters [0, ctr), the
    # epsilon of denoise step i the range [(1 + i) * ctr, (2 + i) * ctr).  (Separate keys seed + 1 + i per step made rank
    # r + 1's latents equal rank r's step-0 noise whenever callers numbered their ranks' seeds consecutively.)
    ctr = (B * n_per + 3) // 4 + 1
    # every adaLN modulation row of the rollout from ONE pass over the 1.5 GB modulation matrix (mmdit.precompute_mods:
    # bit for bit the rows the per-forward GEMM gives; rollout step 412.8 -> 409.6 ms on one box)
    pre = getattr(self.transformer, "precompute_mods", None)
    mods_all = pre(timesteps, tem_ppe) if pre is not None else None
    emb = getattr(self.transformer, "embed_context", None)
    ctx_rows = emb(tem_pe) if emb is not None else None                        # the context embedder is timestep-free as well
    for i in range(len(timesteps)):
        t = timesteps[i]
        if i == random_timestep:                                               # PF:606-623
            cur = noise_level
            all_latents.append(latents)
        elif random_timestep < i < random_timestep + train_num_steps:
            cur = noise_level
        else:
            cur = 0
        if do_cfg and getattr(self, "cfg_two_streams", False) and mods_all is not None and ctx_rows is not None:
            # optional schedule (config `sample.cfg_two_streams`, bench.py's `cfg_two_streams` leg; LABNOTES.md 6 round 5): the unconditional and the conditional half of the CFG batch are
            # independent until the combine -- two forwards of batch B on two HIP streams instead of one of batch 2 B (every row of
            # every kernel is independent of the others: the same bits)
            main = torch.cuda.current_stream(device)
            # one side stream per calling THREAD, created under a lock and kept together with the stream OBJECT it was made for (ADVICE r5:
            # a map keyed by the integer stream handle is mutated by concurrent rollout threads, and a handle re-used after its stream
            # was destroyed would alias the old entry)
            with _CFG_SIDES_LOCK:
                sides = self.__dict__.setdefault("_cfg_sides", {})
                ent = sides.get(threading.get_ident())
                if ent is None or ent[0].cuda_stream != main.cuda_stream:
                    ent = sides[threading.get_ident()] = (main, torch.cuda.Stream(device=device))
            side = ent[1]
            Nt = tem_pe.shape[1]
            ready = torch.cuda.Event()
            ready.record(main)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                vt = self.transformer(hidden_states=latents, timestep=t.expand(B), encoder_hidden_states=tem_pe[B:], pooled_projections=tem_ppe[B:],
                                      return_dict=False, mods=mods_all[i][B:], context=ctx_rows[B * Nt:])[0]
            latents.record_stream(side)
            vu = self.transformer(hidden_states=latents, timestep=t.expand(B), encoder_hidden_states=tem_pe[:B], pooled_projections=tem_ppe[:B],
                                  return_dict=False, mods=mods_all[i][:B], context=ctx_rows[:B * Nt])[0]
            main.wait_stream(side)
            vt.record_stream(main)
        else:
            inp = torch.cat([latents] * 2) if do_cfg else latents                  # PF:625
            v = self.transformer(hidden_states=inp, timestep=t.expand(inp.shape[0]), encoder_hidden_states=tem_pe,
                                 pooled_projections=tem_ppe, joint_attention_kwargs=joint_attention_kwargs,
                                 return_dict=False, **({} if mods_all is None else {"mods": mods_all[i]}),
                                 **({} if ctx_rows is None else {"context": ctx_rows}))[0]                             # PF:630-637
            vu, vt = (v[:B], v[B:]) if do_cfg else (v, None)
        want_f32 = dtype == torch.float32
        nxt, cast, log_prob, _, _ = sde_step_cfg(                              # PF:640-655 fused
            self.scheduler, vu, vt, guidance_scale, None, latents, cur,
            noise=None if noises is None else noises[i], seed=seed, offset=(1 + i) * ctr,
            out_dtype=None if want_f32 else dtype, want_mean=False, step_index=i, sigmas=sigma_table)
        latents = nxt if want_f32 else cast
        if random_timestep <= i < random_timestep + train_num_steps:           # PF:657-660
            all_latents.append(latents)
            all_log_probs.append(log_prob)
            all_timesteps.append(t.repeat(B))
    if output_type == "latent":
        # diffusers' StableDiffusion3Pipeline.__call__ option (`if output_type == "latent": image = latents`) that the reference's trimmed copy
        # of the function dropped: the final latents are returned undecoded so that the caller can run `self.vae.decode_to_image` wherever
        # it schedules the reward computation (bench.py / Trainer: inside the reward future, beside the next group's rollout)
        return latents, all_latents, all_log_probs, all_timesteps
    image = self.vae.decode_to_image(latents)                                  # PF:667-670 (rescale, decode, postprocess)
    return image, all_latents, all_log_probs, all_timesteps


def _branch_rollout(self, keep_f32, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                    num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type, joint_attention_kwargs,
                    noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed):
    """The body of pipeline_with_logprob (keep_f32=True) and pipeline_with_logprob_new (keep_f32=False)."""
    if prompt_embeds is None:
        raise ValueError("prompt strings need text encoders, which are outside the accelerated path "
                         "(SURVEY.md 8a2 / f3): pass prompt_embeds / pooled_prompt_embeds")
    height = height or self.default_sample_size * self.vae_scale_factor
    width = width or self.default_sample_size * self.vae_scale_factor
    self._guidance_scale = guidance_scale
    device = self._execution_device
    G = int(mini_num_image_per_prompt)
    pe, ppe = prompt_embeds.to(device), pooled_prompt_embeds.to(device)        # P rows: NOT repeated up front (PF:114-123, :335-344)
    do_cfg = guidance_scale > 1
    if do_cfg:
        npe, nppe = negative_prompt_embeds.to(device), negative_pooled_prompt_embeds.to(device)
        tem_pe, tem_ppe = torch.cat([npe, pe], dim=0), torch.cat([nppe, ppe], dim=0)       # PF:150-152, :372-374
    else:
        tem_pe, tem_ppe = pe, ppe
    dtype = prompt_embeds.dtype
    P = pe.shape[0]
    if latents is None and generator is not None and seed is None:             # as pipeline_with_logprob_random: diffusers' randn_tensor draw
        gdev = generator.device if isinstance(generator, torch.Generator) else torch.device("cpu")
        shape = (P, self.transformer.config.in_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    if latents is None:                                                        # PF:114-123, :335-344 prepare_latents on P rows
        latents = self.prepare_latents(P, self.transformer.config.in_channels, height, width, dtype, device, seed)
    latents = latents.to(device=device, dtype=dtype)
    lat_dtype = torch.float32 if keep_f32 else dtype
    latents = latents.to(lat_dtype)                                            # PF:123 `.float()` on the embedding-dtype draw
    timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device)   # PF:129, :350
    sigma_table = self.scheduler.sigmas                                        # rollout-local view (see pipeline_with_logprob_random)
    if random_timestep is None:                                                # PF:140-142, :361-363
        random_timestep = random.Random(process_index).randint(0, sample_num_steps // 2)
    self.last_random_timestep = random_timestep
    r = random_timestep
    all_latents, all_log_probs, all_timesteps = [], [], []
    n_per = latents[0].numel()
    # pipeline_with_logprob_random's Philox layout for its P * G rows: the initial latents use counters from 0 (over P rows here), the epsilon
    # of step i the range from (1 + i) * ctr.  With G == 1 the two functions draw the same numbers.
    ctr = (P * G * n_per + 3) // 4 + 1
    pre = getattr(self.transformer, "precompute_mods", None)
    mods_all = pre(timesteps, tem_ppe) if pre is not None else None           # once, for the P-row CFG batch
    emb = getattr(self.transformer, "embed_context", None)
    ctx_rows = emb(tem_pe) if emb is not None else None
    B = P                                                                      # rows of `latents`; P * G after the branch step
    for i in range(len(timesteps)):
        t = timesteps[i]
        if i == r:                                                             # PF:160-171, :382-393
            cur = noise_level
            all_latents.append(latents.repeat(G, 1, 1, 1))
        elif r < i < r + train_num_steps:
            cur = noise_level
        else:
            cur = 0
        inp_lat = latents.to(dtype)                                            # keep_f32: rounded to the embedding dtype at the transformer's door
        mods_i = None if mods_all is None else mods_all[i]
        if do_cfg and getattr(self, "cfg_two_streams", False) and mods_all is not None and ctx_rows is not None:
            # the schedule of pipeline_with_logprob_random's cfg_two_streams branch (same bits as one forward of twice the batch)
            main = torch.cuda.current_stream(device)
            with _CFG_SIDES_LOCK:
                sides = self.__dict__.setdefault("_cfg_sides", {})
                ent = sides.get(threading.get_ident())
                if ent is None or ent[0].cuda_stream != main.cuda_stream:
                    ent = sides[threading.get_ident()] = (main, torch.cuda.Stream(device=device))
            side = ent[1]
            Nt = tem_pe.shape[1]
            ready = torch.cuda.Event()
            ready.record(main)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                vt = self.transformer(hidden_states=inp_lat, timestep=t.expand(B), encoder_hidden_states=tem_pe[B:], pooled_projections=tem_ppe[B:],
                                      return_dict=False, mods=mods_i[B:], context=ctx_rows[B * Nt:])[0]
            inp_lat.record_stream(side)
            vu = self.transformer(hidden_states=inp_lat, timestep=t.expand(B), encoder_hidden_states=tem_pe[:B], pooled_projections=tem_ppe[:B],
                                  return_dict=False, mods=mods_i[:B], context=ctx_rows[:B * Nt])[0]
            main.wait_stream(side)
            vt.record_stream(main)
        else:
            inp = torch.cat([inp_lat] * 2) if do_cfg else inp_lat             # PF:177, :399
            v = self.transformer(hidden_states=inp, timestep=t.expand(inp.shape[0]), encoder_hidden_states=tem_pe,
                                 pooled_projections=tem_ppe, joint_attention_kwargs=joint_attention_kwargs,
                                 return_dict=False, **({} if mods_i is None else {"mods": mods_i}),
                                 **({} if ctx_rows is None else {"context": ctx_rows}))[0]                             # PF:182-189, :404-411
            vu, vt = (v[:B], v[B:]) if do_cfg else (v, None)
        want_f32 = lat_dtype == torch.float32
        # at i == r the transformer ran on the P un-repeated rows (G identical copies of a row give G identical velocities); the step fans out
        nxt, cast, log_prob, _, _ = sde_step_cfg(                              # PF:192-204, :414-429 fused
            self.scheduler, vu, vt, guidance_scale, None, latents, cur,
            noise=None if noises is None else noises[i], seed=seed, offset=(1 + i) * ctr,
            out_dtype=None if want_f32 else lat_dtype, want_mean=False, step_index=i, sigmas=sigma_table,
            copies=G if i == r else None)
        latents = nxt if want_f32 else cast
        if i == r:                                                             # PF:163-170, :385-392: the embeddings follow the latents
            B = P * G
            if do_cfg:
                rows = torch.arange(B, device=device) % P
                rows = torch.cat([rows, P + rows])
            else:
                rows = torch.arange(B, device=device) % P
            tem_pe, tem_ppe = tem_pe[rows], tem_ppe[rows]                      # = cat([npe.repeat(G, 1, 1), pe.repeat(G, 1, 1)]), ...
            if mods_all is not None:                                           # every row of the modulation GEMM and of the context embedder is
                mods_all = mods_all[:, rows]                                   # independent of the batch it was computed in: gathered, not recomputed
            if ctx_rows is not None:
                Nt = tem_pe.shape[1]
                ctx_rows = ctx_rows.view(-1, Nt, ctx_rows.shape[-1])[rows].reshape(-1, ctx_rows.shape[-1])
        if r <= i < r + train_num_steps:                                       # PF:209-212, :431-434
            all_latents.append(latents)
            all_log_probs.append(log_prob)
            all_timesteps.append(t.repeat(B))
    if output_type == "latent":                                                # as pipeline_with_logprob_random
        return latents, all_latents, all_log_probs, all_timesteps
    image = self.vae.decode_to_image(latents)                                  # PF:219-225, :441-444
    if output_type == "pil":                                                   # the reference's default (the trainers pass "pt")
        from PIL import Image
        arr = (image.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        image = [Image.fromarray(a) for a in arr]
    return image, all_latents, all_log_probs, all_timesteps


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
    The G samples of a group share their initial noise and prefix: the group's spread comes from the SDE window alone."""
    return _branch_rollout(self, False, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                           num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type,
                           joint_attention_kwargs, noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed)


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
    return _branch_rollout(self, True, prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, height, width,
                           num_inference_steps, mini_num_image_per_prompt, guidance_scale, generator, latents, output_type,
                           joint_attention_kwargs, noise_level, train_num_steps, process_index, sample_num_steps, random_timestep, noises, seed)
