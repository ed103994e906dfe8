"""GPU: the shared-prefix branching rollouts pipeline_with_logprob / pipeline_with_logprob_new and the fan-out SDE step under them
(advgrpo_sde_step_branch), on reduced stacks: the kernel against advgrpo_sde_step on the materialised repeat (bit for bit), both functions
against the trajectory of the REFERENCE's own functions (tests/golden/branch_rollout.npz), the shared prefix against the literal
repeat-then-forward, G == 1 against pipeline_with_logprob_random, replay, the Trainer option and the C entry's argument checks."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "branch_rollout.npz")


# ----------------------------------------------------------------------------- 1. the kernel
def _scheduler(steps=10):
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler(device=torch.device("cuda"))
    sch.set_timesteps(steps, device=torch.device("cuda"))
    return sch


@pytest.mark.parametrize("mode", ["philox", "eps", "replay"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fan_out_step_has_the_bits_of_the_step_on_the_repeated_batch(mode, dtype):
    """advgrpo_sde_step_branch(P rows, G copies) == advgrpo_sde_step(x.repeat(G, ...)) with torch.equal on next, cast, mean, log_prob and
    std: with and without CFG, (P, G) in {(1, 8), (2, 3), (3, 16)} (one block of copies, a partial one, two), n a multiple of the
    2048-element chunk (4096), not one (1600) and longer than one pass of the 64 blocks of a row (147456), sigma stride 0 and 1, noise
    level 0 and 0.7."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    sch = _scheduler()
    gen = torch.Generator().manual_seed(3)
    checked = 0
    for (P, G) in ((1, 8), (2, 3), (3, 16)):
        for shape in ((16, 16, 16), (16, 10, 10), (16, 96, 96)):
            vu = torch.randn(P, *shape, generator=gen).to(dtype).cuda()
            vt = torch.randn(P, *shape, generator=gen).to(dtype).cuda()
            x = torch.randn(P, *shape, generator=gen).to(dtype).cuda()
            eps = torch.randn(P * G, *shape, generator=gen).cuda()
            prev = torch.randn(P * G, *shape, generator=gen).to(dtype).cuda()
            rep = lambda t: t.repeat(G, 1, 1, 1)
            for cfg in (True, False):
                for stride in (0, 1):
                    for nl in (0, 0.7):
                        kw = dict(noise_level=nl, out_dtype=torch.bfloat16, want_mean=True)
                        kw.update({"philox": dict(seed=1234, offset=77), "eps": dict(noise=eps), "replay": dict(prev_sample=prev)}[mode])
                        if stride == 0:
                            t_in = t_rep = None
                            kw["step_index"] = 3
                        else:                      # one schedule index per row (P == 1: a single index, which is the stride-0 table again)
                            t_in = torch.stack([sch.timesteps[(2 + 3 * p) % 10] for p in range(P)])
                            t_rep = t_in.repeat(G)
                        a = sde_step_cfg(sch, vu, vt if cfg else None, 4.5, t_in, x, copies=G, **kw)
                        b = sde_step_cfg(sch, rep(vu), rep(vt) if cfg else None, 4.5, t_rep, rep(x), **kw)
                        for name, u, v in zip(("next", "cast", "log_prob", "mean", "std"), a, b):
                            if mode == "replay" and name in ("next", "cast"):
                                assert u is None and v is None
                                continue
                            assert u.shape == v.shape and u.dtype == v.dtype, (name, u.shape, v.shape)
                            assert torch.equal(u, v), (name, P, G, shape, cfg, stride, nl, (u.float() - v.float()).abs().max().item())
                        assert a[2].shape == (P * G,) and torch.isfinite(a[2]).all()
                        if mode != "replay" and nl > 0:    # the copies of a row really differ (their own epsilon each)
                            assert not torch.equal(a[0][0], a[0][P])
                        checked += 1
    assert checked == 3 * 3 * 2 * 2 * 2


# ----------------------------------------------------------------------------- 2. the reference's trajectory
def _groups(npz):
    names = sorted({k.split("/")[0] for k in npz.files})
    return {n: {k.split("/", 1)[1]: npz[k] for k in npz.files if k.startswith(n + "/")} for n in names}


class _StandinVae:
    """Same arithmetic as the stand-in used for the golden: rescale, stand-in decode, postprocess."""

    def decode_to_image(self, latents):
        from oracle.standin import standin_vae_decode
        z = (latents / 1.5305) + 0.0609
        return (standin_vae_decode(z.to(torch.float32)) / 2 + 0.5).clamp(0, 1)


class _DoorCast(torch.nn.Module):
    """The golden's transformer stand-in (make_golden_branch_rollout.py): StandinVelocity behind the rounding of the latents to the embedding
    dtype.  Both rollouts round at the door themselves, so the cast here never changes a value."""

    def __init__(self):
        super().__init__()
        from oracle.standin import StandinVelocity
        self.net = StandinVelocity()
        self.config = type("C", (), {"in_channels": 16})()

    def forward(self, hidden_states, timestep, encoder_hidden_states, pooled_projections, joint_attention_kwargs=None, return_dict=False):
        assert hidden_states.dtype == encoder_hidden_states.dtype
        return self.net(hidden_states, timestep, encoder_hidden_states, pooled_projections)


_RUNS = [(f, d, r) for f in ("plain", "new") for d in ("fp32", "bf16") for r in ("0", "2")] + [("plain", "bf16", "draw"), ("new", "bf16", "draw")]


@pytest.mark.parametrize("fname,case,r", _RUNS)
def test_branching_rollouts_match_the_reference_trajectory(fname, case, r):
    """Both functions with the reference's epsilon injected, against what the reference's own functions returned (stand-in velocity network
    and decoder).  Tolerances: those of tests/test_gpu_rollout.py::test_rollout_matches_reference_trajectory for the pipeline_with_logprob_random
    golden, keyed by the embedding dtype (the stand-in network runs through torch-on-GPU: one ulp of the dtype it computes in).  `draw`:
    random_timestep=None with process_index=1 -- the branch step is the reference's draw."""
    from adv_grpo_amd.diffusers_patch import sd3_pipeline_with_logprob_fast as PF
    from adv_grpo_amd.pipeline import SD3Pipeline
    npz = np.load(GOLD)
    g = _groups(npz)[f"{fname}_{case}_r{r}"]
    dtype = torch.float32 if case == "fp32" else torch.bfloat16
    steps, T, P, Gn, hw, drawn, process_index, r_arg = (int(v) for v in g["meta"])
    guidance, noise_level = (float(v) for v in g["scalars"])
    pipe = SD3Pipeline(_DoorCast().cuda(), _StandinVae(), "cuda")
    tt = lambda k: torch.from_numpy(g[k]).to(dtype).cuda()
    noises = [torch.from_numpy(npz[f"noise/r{drawn}/{i}"]).cuda() for i in range(steps)]
    fn = PF.pipeline_with_logprob if fname == "plain" else PF.pipeline_with_logprob_new
    image, lats, lps, tss = fn(
        pipe, prompt_embeds=tt("pe"), pooled_prompt_embeds=tt("ppe"), negative_prompt_embeds=tt("npe"),
        negative_pooled_prompt_embeds=tt("nppe"), num_inference_steps=steps, guidance_scale=guidance, output_type="pt",
        height=hw, width=hw, noise_level=noise_level, mini_num_image_per_prompt=Gn, train_num_steps=T, process_index=process_index,
        sample_num_steps=steps, random_timestep=None if r_arg < 0 else r_arg, latents=torch.from_numpy(npz["lat0"]).cuda(), noises=noises)
    assert pipe.last_random_timestep == drawn
    lat = torch.stack(lats, 1); lp = torch.stack(lps, 1); ts = torch.stack(tss, 1)
    want = torch.float32 if fname == "plain" else dtype          # pipeline_with_logprob never casts back (PF:123, :206-207)
    assert lat.dtype == want and lp.dtype == torch.float32 and lat.shape == g["latents"].shape == (P * Gn, T + 1, 16, hw // 8, hw // 8)
    assert np.array_equal(ts.float().cpu().numpy(), g["timesteps"])
    tol = 2e-5 if dtype == torch.float32 else 2 ** -7
    d_lat = np.abs(lat.float().cpu().numpy() - g["latents"]).max()
    d_lp = np.abs(lp.cpu().numpy() / g["log_probs"] - 1).max()
    d_img = np.abs(image.float().cpu().numpy() - g["image"]).max()
    print(f"{fname}_{case}_r{r}: max |latents diff| {d_lat:.3e}  max log-prob rel diff {d_lp:.3e}  max |image diff| {d_img:.3e}")
    assert np.allclose(lat.float().cpu().numpy(), g["latents"], atol=tol * 4, rtol=tol)
    assert np.allclose(lp.cpu().numpy(), g["log_probs"], rtol=5e-3 if dtype == torch.bfloat16 else 1e-4)
    assert np.allclose(image.float().cpu().numpy(), g["image"], atol=2e-2 if dtype == torch.bfloat16 else 1e-4)


# ----------------------------------------------------------------------------- 3 - 5. the reduced SD3 stack
_STACK = {}


def _stack():
    """The reduced stack of tests/test_gpu_rollout.py (3 MMDiT blocks, 256 x 256), built once for this module."""
    if not _STACK:
        from adv_grpo_amd import synthetic
        from adv_grpo_amd.mmdit import SD3Transformer2DModel
        from adv_grpo_amd.model_configs import MMDiTConfig, VaeConfig
        from adv_grpo_amd.pipeline import SD3Pipeline
        from adv_grpo_amd.vae import AutoencoderKLDecoder
        mcfg = MMDiTConfig(num_layers=3, num_heads=6, pos_embed_max_size=96, dual_attention_layers=(0, 1))
        with synthetic.on_device("cuda"):
            vae = AutoencoderKLDecoder(synthetic.vae_decoder_weights(VaeConfig(), 22, fp16_checkpoint=True), VaeConfig(), "cuda")
            _STACK["pipe"] = SD3Pipeline(SD3Transformer2DModel(synthetic.mmdit_weights(mcfg, 21), mcfg, "cuda"), vae, "cuda")
        emb = [[t.cuda().to(torch.bfloat16) for t in synthetic.prompt_embeddings(s)] for s in (5, 6)]
        _STACK["embeds"] = {1: tuple(emb[0]), 2: tuple(torch.cat([a, b]) for a, b in zip(*emb))}
    return _STACK["pipe"], _STACK["embeds"]


def _kw(embeds, G, r, steps=4, seed=77, T=2):
    pe, ppe, npe, nppe = embeds
    return dict(prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=nppe,
                num_inference_steps=steps, guidance_scale=4.5, height=256, width=256, noise_level=0.8, mini_num_image_per_prompt=G,
                train_num_steps=T, process_index=0, sample_num_steps=steps, random_timestep=r, seed=seed, output_type="pt")


def _naive_branch_rollout(pipe, embeds, G, r, steps=4, seed=77, T=2):
    """pipeline_with_logprob_new as PF:379-434 literally runs it: at step r the latents and the four embedding tensors are repeated BEFORE
    the transformer call, which then sees G identical copies of every row; modulation rows and context rows are computed on the batch they
    are used with.  Same Philox counters as the product."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    from adv_grpo_amd.scheduler import retrieve_timesteps
    pe, ppe, npe, nppe = embeds
    P = pe.shape[0]
    tr = pipe.transformer
    latents = pipe.prepare_latents(P, 16, 256, 256, pe.dtype, pipe.device, seed)
    timesteps, _ = retrieve_timesteps(pipe.scheduler, steps, pipe.device)
    sig = pipe.scheduler.sigmas
    ctr = (P * G * latents[0].numel() + 3) // 4 + 1
    tem_pe, tem_ppe = torch.cat([npe, pe]), torch.cat([nppe, ppe])
    mods, ctx = tr.precompute_mods(timesteps, tem_ppe), tr.embed_context(tem_pe)
    lats, lps = [], []
    for i in range(steps):
        if i == r:
            latents = latents.repeat(G, 1, 1, 1)
            pe, ppe, npe, nppe = pe.repeat(G, 1, 1), ppe.repeat(G, 1), npe.repeat(G, 1, 1), nppe.repeat(G, 1)
            tem_pe, tem_ppe = torch.cat([npe, pe]), torch.cat([nppe, ppe])
            mods, ctx = tr.precompute_mods(timesteps, tem_ppe), tr.embed_context(tem_pe)
            lats.append(latents)
        B = latents.shape[0]
        v = tr(hidden_states=torch.cat([latents] * 2), timestep=timesteps[i].expand(2 * B), encoder_hidden_states=tem_pe,
               pooled_projections=tem_ppe, return_dict=False, mods=mods[i], context=ctx)[0]
        _, latents, lp, _, _ = sde_step_cfg(pipe.scheduler, v[:B], v[B:], 4.5, None, latents, 0.8 if r <= i < r + T else 0, seed=seed,
                                            offset=(1 + i) * ctr, out_dtype=pe.dtype, want_mean=False, step_index=i, sigmas=sig)
        if r <= i < r + T:
            lats.append(latents)
            lps.append(lp)
    return pipe.vae.decode_to_image(latents), lats, lps, (mods, ctx)


@pytest.mark.parametrize("P,G,r", [(1, 4, 1), (2, 3, 2), (2, 3, 0)])
def test_shared_prefix_changes_no_bits(P, G, r):
    """pipeline_with_logprob_new (transformer on the P un-repeated rows at the branch step, fan-out inside the SDE step, modulation and
    context rows gathered from the P-row precompute) against the literal repeat-then-forward: every recorded latent, every log-prob and the
    image with torch.equal; with the CFG halves on two streams as well.  Also the gather itself: rows of precompute_mods / embed_context
    taken from the P-row CFG batch equal those computed on the repeated batch."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_new
    pipe, embeds = _stack()
    pipe.cfg_two_streams = False
    img_n, lats_n, lps_n, (mods_rep, ctx_rep) = _naive_branch_rollout(pipe, embeds[P], G, r)
    # the gather of the P-row precompute == the precompute on the repeated batch
    pe, ppe, npe, nppe = embeds[P]
    from adv_grpo_amd.scheduler import retrieve_timesteps
    timesteps, _ = retrieve_timesteps(pipe.scheduler, 4, pipe.device)
    rows = torch.arange(P * G, device="cuda") % P
    rows = torch.cat([rows, P + rows])
    mods_p = pipe.transformer.precompute_mods(timesteps, torch.cat([nppe, ppe]))
    ctx_p = pipe.transformer.embed_context(torch.cat([npe, pe]))
    Nt = pe.shape[1]
    assert torch.equal(mods_p[:, rows], mods_rep)
    assert torch.equal(ctx_p.view(2 * P, Nt, -1)[rows].reshape(2 * P * G * Nt, -1), ctx_rep)
    for two_streams in (False, True):
        pipe.cfg_two_streams = two_streams
        img, lats, lps, tss = pipeline_with_logprob_new(pipe, **_kw(embeds[P], G, r))
        torch.cuda.synchronize()
        assert len(lats) == 3 and len(lps) == 2 and all(a.shape[0] == P * G for a in lats) and all(t.shape == (P * G,) for t in tss)
        for k, (a, b) in enumerate(zip(lats, lats_n)):
            assert a.dtype == b.dtype and torch.equal(a, b), (two_streams, "latent", k)
        for k, (a, b) in enumerate(zip(lps, lps_n)):
            assert torch.equal(a, b), (two_streams, "log_prob", k)
        assert torch.equal(img, img_n) and torch.isfinite(img).all()
    pipe.cfg_two_streams = False


def test_one_copy_per_prompt_is_the_random_rollout():
    """mini_num_image_per_prompt == 1: nothing is shared, and pipeline_with_logprob_new returns pipeline_with_logprob_random's bits for the
    same seed (the same Philox counters)."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_new, pipeline_with_logprob_random
    pipe, embeds = _stack()
    for P, r in ((1, 1), (2, 0)):
        a = pipeline_with_logprob_random(pipe, **_kw(embeds[P], 1, r))
        b = pipeline_with_logprob_new(pipe, **_kw(embeds[P], 1, r))
        assert torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) == 3
        for x, y in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]):
            assert x.dtype == y.dtype and torch.equal(x, y)


def test_replay_of_a_branching_rollout_and_what_the_group_shares():
    """The recorded (latents, next_latents, timesteps) of a pipeline_with_logprob_new rollout through the replay path compute_log_prob takes
    (sde_step_with_logprob(prev_sample=...)) give its log-probs back, to the bound tests/test_gpu_rollout.py uses for the replay of a bf16
    trajectory (rtol 2e-2).  The group shares the window's first latent (rows j and j + P of all_latents[0] are equal) and nothing after it.
    Six steps with the window on steps 1 and 2, as the Trainer places it (random_timestep <= num_steps // 2): std_dev_t is 0.78 and 0.63 there.
    On the LAST step of a schedule std_dev_t is 0.0085, the rollout's log-prob (from the f32 sample) is -7e-5, and the bf16 rounding of the
    stored next latents alone adds (2^-9 |x|)^2 / 3 ~ 1e-5 to a replayed one: no relative bound holds there, in the reference either."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_new
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_with_logprob
    pipe, embeds = _stack()
    P, G, r, T = 2, 3, 1, 2
    img, lats, lps, tss = pipeline_with_logprob_new(pipe, **_kw(embeds[P], G, r, steps=6))
    for j in range(P):
        for g in range(1, G):
            assert torch.equal(lats[0][j], lats[0][j + g * P])
            assert not torch.equal(lats[1][j], lats[1][j + g * P])
    assert not torch.equal(lats[0][0], lats[0][1])
    pe, ppe, npe, nppe = embeds[P]
    tem_pe = torch.cat([npe.repeat(G, 1, 1), pe.repeat(G, 1, 1)])
    tem_ppe = torch.cat([nppe.repeat(G, 1), ppe.repeat(G, 1)])
    B = P * G
    for j in range(T):
        x = lats[j]
        v = pipe.transformer(hidden_states=torch.cat([x] * 2), timestep=tss[j].repeat(2), encoder_hidden_states=tem_pe,
                             pooled_projections=tem_ppe, return_dict=False)[0]
        vv = v[:B] + 4.5 * (v[B:] - v[:B])                                   # TP:252-256
        _, lp, _, _ = sde_step_with_logprob(pipe.scheduler, vv.float(), tss[j], x.float(), noise_level=0.8, prev_sample=lats[j + 1].float())
        rel = ((lp - lps[j]).abs() / lps[j].abs()).max().item()
        print(f"replay step {j}: max log-prob rel diff {rel:.3e}")
        assert torch.allclose(lp, lps[j], rtol=2e-2), (lp, lps[j])


# ----------------------------------------------------------------------------- 6 - 7. the Trainer option
def _trainer(**sample_over):
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.mmdit_train import SD3TransformerLoRA
    from adv_grpo_amd.model_configs import ClipConfig, MMDiTConfig, VaeConfig
    from adv_grpo_amd.pickscore_scorer import PickScoreScorer
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.trainer import SyntheticData, Trainer
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = get_config("pickscore_cotrain_sd3_fast", gpu_number=1)           # the small stack of tests/test_gpu_trainer.py
    cfg.resolution = 256
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 4
    cfg.sample.num_batches_per_epoch = 2
    cfg.train.gradient_accumulation_steps = 1
    cfg.train_d = False
    for k, v in sample_over.items():
        setattr(cfg.sample, k, v)
    mcfg = MMDiTConfig(num_layers=2, num_heads=4, joint_attention_dim=256, pooled_projection_dim=128,
                       pos_embed_max_size=96, dual_attention_layers=(0,))
    tr = SD3TransformerLoRA({k: v.to(torch.bfloat16) for k, v in synthetic.mmdit_weights(mcfg, 1).items()}, mcfg, "cuda")
    vae = AutoencoderKLDecoder({k: v.to(torch.bfloat16) for k, v in synthetic.vae_decoder_weights(VaeConfig(), 2).items()},
                               VaeConfig(), "cuda")
    cc = ClipConfig(v_layers=2, t_layers=2)
    scorer = PickScoreScorer("cuda", dtype=torch.bfloat16, model_sd=synthetic.clip_weights(cc, 4), clip_cfg=cc)
    data = SyntheticData(n_prompts=100, n_tokens=21, ctx_dim=256, pooled_dim=128, resolution=256)
    return Trainer(cfg, SD3Pipeline(tr, vae, "cuda"), data, scorer, None), tr


def test_trainer_epoch_with_branch_rollout():
    """sample.branch_rollout = True on the small stack: one epoch runs, rewards / advantages / the G-step loss are finite, the sample dict
    has its usual keys and shapes, and the first latent of the window is shared within a prompt group (latents[:, 0])."""
    tr_, model = _trainer(branch_rollout=True)
    G, T, nb = 4, tr_.cfg.sample.train_num_steps, 2
    seen = {}
    g_step = tr_.g_step
    tr_.g_step = lambda samples: (seen.update(samples), g_step(samples))[1]
    recs = []
    log = tr_.logger.log
    tr_.logger.log = lambda rec, step=None: (recs.append(dict(rec)), log(rec, step))[1]
    p0 = model.params.clone()
    info = tr_.run_epoch()
    losses = [float(r["loss"]) for r in recs if "loss" in r]
    assert info["phase"] == "G" and losses and all(math.isfinite(v) for v in losses) and not torch.equal(model.params, p0)
    assert torch.isfinite(model.params).all()
    assert seen["rewards"].shape == (nb * G,) and torch.isfinite(seen["rewards"]).all()
    assert seen["advantages"].shape == (nb * G, T) and torch.isfinite(seen["advantages"]).all()
    assert seen["latents"].shape == seen["next_latents"].shape == (nb * G, T, 16, 32, 32) and seen["log_probs"].shape == (nb * G, T)
    assert seen["timesteps"].shape == (nb * G, T) and seen["images"].shape == (nb * G, 3, 256, 256)
    for b in range(nb):
        grp = seen["latents"][b * G:(b + 1) * G]
        assert all(torch.equal(grp[0, 0], grp[k, 0]) for k in range(1, G))
        assert not any(torch.equal(grp[0, 1], grp[k, 1]) for k in range(1, G))
    assert not torch.equal(seen["latents"][0, 0], seen["latents"][G, 0])


def test_trainer_without_the_option_samples_what_it_always_did():
    """sample.branch_rollout = False against a config without the key: the sample dicts of the same seed are equal, torch.equal on every
    tensor (latents, log-probs, timesteps, embeddings, images, rewards)."""
    tr_a, _ = _trainer()
    assert tr_a.cfg.sample.get("branch_rollout") is None
    a = tr_a.sample_epoch()
    tr_b, _ = _trainer(branch_rollout=False)
    b = tr_b.sample_epoch()
    torch.cuda.synchronize()
    assert set(a) == set(b) and sum(isinstance(v, torch.Tensor) for v in a.values()) >= 9
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


# ----------------------------------------------------------------------------- 8. the C entry's argument checks
def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every bad-argument case returns non-zero, raises _lib.AdvGrpoError through _lib.check, and leaves the sentinel-filled outputs alone.
    Argument checks only: each call is refused on the host, nothing reaches the device."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    P, G, n = 2, 3, 2048
    vu = torch.randn(P, n, device="cuda"); vt = torch.randn(P, n, device="cuda"); x = torch.randn(P, n, device="cuda")
    sig = torch.tensor([0.9], device="cuda"); sigp = torch.tensor([0.8], device="cuda")
    eps = torch.randn(P * G, n, device="cuda"); prev = torch.randn(P * G, n, device="cuda")
    SENT = -12288.0                                  # (exact in bf16 as well)
    outs = {k: torch.full(s, SENT, device="cuda") for k, s in
            (("next", (P * G, n)), ("mean", (P * G, n)), ("lp", (P * G,)), ("std", (P * G,)))}
    cast = torch.full((P * G, n), SENT, device="cuda", dtype=torch.bfloat16)
    ws = torch.full((lib.advgrpo_sde_step_workspace_bytes(P * G, n) // 4,), SENT, device="cuda")

    def call(**over):
        a = dict(vu=vu.data_ptr(), vt=vt.data_ptr(), x=x.data_ptr(), sig=sig.data_ptr(), sigp=sigp.data_ptr(), mode=_lib.SDE_PHILOX,
                 eps=None, prev=None, lp=outs["lp"].data_ptr(), ws=ws.data_ptr(), P=P, G=G, n=n, vdt=_lib.F32)
        a.update(over)
        return lib.advgrpo_sde_step_branch(a["vu"], a["vt"], a["vdt"], 4.5, a["x"], _lib.F32, a["sig"], a["sigp"], 0, 0.5, a["mode"], a["eps"], 1, 0,
                                           a["prev"], _lib.F32, outs["next"].data_ptr(), cast.data_ptr(), _lib.BF16, outs["mean"].data_ptr(),
                                           a["lp"], outs["std"].data_ptr(), a["ws"], a["P"], a["G"], a["n"], _lib.stream_ptr())
    bad = [dict(vu=None), dict(x=None), dict(sig=None), dict(sigp=None), dict(lp=None), dict(ws=None), dict(P=0), dict(P=-1), dict(G=0),
           dict(G=-2), dict(n=0), dict(n=-8), dict(n=12), dict(mode=_lib.SDE_EPS), dict(mode=_lib.SDE_REPLAY), dict(mode=3), dict(vdt=7)]
    for over in bad:
        rc = call(**over)
        assert rc != 0, over
        with pytest.raises(_lib.AdvGrpoError, match="sde_step"):
            _lib.check(rc)
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + [("cast", cast), ("workspace", ws)]:
        assert (t.float() == SENT).all(), k
    # and the same arguments without a fault are accepted (EPS with eps, REPLAY with prev_sample)
    assert call() == 0 and call(mode=_lib.SDE_EPS, eps=eps.data_ptr()) == 0 and call(mode=_lib.SDE_REPLAY, prev=prev.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(outs["lp"]).all() and (outs["lp"] != SENT).all()
