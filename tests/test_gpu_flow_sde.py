"""GPU: the Flow-SDE siblings of the fused step (advgrpo_flow_sde_step, _branch, _bwd, _bwd_kl), `sde_step_cfg(sde_type="sde")`, the
full-trajectory rollout and the Trainer option.  The kernels against what the REFERENCE's own function returned
(tests/golden/flow_sde.npz), against the restatement tests/flow_sde_reference.py (float64, and in float32 as the reference's operation
sequence for the bit-for-bit comparisons), the fan-out form against the plain entry on the repeated batch, the backward entries against
autograd, the rollout against tests/golden/full_trajectory.npz.

Sizes: n = 1024 (one block), 4096 (two blocks), 16 x 128 x 128 (the only one where the 64-block grid-stride loop iterates); fan-out with
G = 3 and G = 9 (more than the SDE_BRANCH_COPIES = 8 copies one block carries)."""
import math
import os

import numpy as np
import pytest
import torch

import flow_sde_reference as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "flow_sde.npz")
GOLD_FULL = os.path.join(os.path.dirname(__file__), "golden", "full_trajectory.npz")
SHAPES = [(16, 8, 8), (16, 16, 16), (16, 128, 128)]


def _case(name):
    npz = np.load(GOLD, allow_pickle=False)
    g = {k.split("/", 1)[1]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(name + "/")}
    return g, int(g["meta"][1]), float(g["meta"][2])


def _scheduler(steps=10):
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler(device=torch.device("cuda"))
    sch.set_timesteps(steps, device=torch.device("cuda"))
    return sch


# ----------------------------------------------------------------------------- 1. the reference's own numbers
@pytest.mark.parametrize("name", ["s10_i0", "s10_i1", "s10_i5", "s10_i9", "s4_i0", "s4_i2"])
def test_flow_sde_step_vs_reference_golden(name):
    """float32 inputs, the reference's epsilon injected, the golden's own sigma table: mean, next and std bit for bit; log_prob and the two
    replayed log-probs (from the float32 next and from its bf16 rounding) within 2e-6 (|q| + |log w| + 0.919)."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    g, idx, nl = _case(name)
    sig = g["sigmas"].cuda()
    v, x, eps = g["v"].cuda(), g["x"].cuda(), g["eps"].cuda()
    nxt, cast, lp, mean, std = sde_step_cfg(None, v, None, 1.0, None, x, nl, noise=eps, step_index=idx, sigmas=sig, sde_type="sde")
    assert cast is None and torch.equal(mean.cpu(), g["mean"]) and torch.equal(nxt.cpu(), g["next"])
    assert torch.equal(std.reshape(-1).cpu(), g["std"])
    w = g["std"] * torch.sqrt(-1 * (g["sigmas"][idx + 1] - g["sigmas"][idx]))
    bound = R.log_prob_bound(g["next"], g["mean"], w)
    print(name, "log_prob", lp.tolist(), "golden", g["log_prob"].tolist(), "|diff|", (lp.cpu() - g["log_prob"]).abs().tolist(), "bound", bound.tolist())
    assert ((lp.cpu().double() - g["log_prob"].double()).abs() <= bound).all()
    for key, prev in (("log_prob_replay_f32", g["next"]), ("log_prob_replay_bf16", g["next"].to(torch.bfloat16))):
        a, b, lp_r, mean_r, _ = sde_step_cfg(None, v, None, 1.0, None, x, nl, prev_sample=prev.cuda(), step_index=idx, sigmas=sig, sde_type="sde")
        bound = R.log_prob_bound(prev.float(), g["mean"], w)
        print(name, key, lp_r.tolist(), "golden", g[key].tolist(), "bound", bound.tolist())
        assert a is None and b is None and torch.equal(mean_r.cpu(), g["mean"])
        assert ((lp_r.cpu().double() - g[key].double()).abs() <= bound).all(), key


def test_flow_sde_step_with_logprob_has_the_reference_signature_and_numbers():
    """The drop-in for the reference's `sde_step_with_logprob`, on the project's own scheduler with per-sample timesteps (sigma stride 1)."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import flow_sde_step_with_logprob
    g, idx, nl = _case("s10_i5")
    sch = _scheduler(10)
    assert torch.equal(sch.sigmas.cpu(), g["sigmas"])
    t = torch.stack([sch.timesteps[idx], sch.timesteps[1]])
    v, x, eps = g["v"].cuda(), g["x"].cuda(), g["eps"].cuda()
    nxt, lp, mean, std = flow_sde_step_with_logprob(sch, v, t, x, noise_level=nl, noise=eps)
    assert std.shape == (2, 1, 1, 1) and torch.equal(nxt[0].cpu(), g["next"][0]) and torch.equal(mean[0].cpu(), g["mean"][0])
    o_nxt, o_lp, o_mean, o_std, _ = R.flow_sde_step(g["v"][1:], g["x"][1:], g["sigmas"][1:2], g["sigmas"][2:3], float(g["sigmas"][1]), nl,
                                                    eps=g["eps"][1:], dtype=torch.float32)
    assert torch.equal(nxt[1:].cpu(), o_nxt) and torch.equal(mean[1:].cpu(), o_mean) and torch.equal(std.reshape(-1)[1:].cpu(), o_std)
    prev, lp_r, _, _ = flow_sde_step_with_logprob(sch, v, t, x, noise_level=nl, prev_sample=nxt)
    assert torch.equal(prev, nxt) and torch.allclose(lp_r, lp, rtol=0, atol=1e-5)
    a = flow_sde_step_with_logprob(sch, v, t, x, noise_level=nl, generator=torch.Generator().manual_seed(5))
    b = flow_sde_step_with_logprob(sch, v, t, x, noise_level=nl, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], nxt) and torch.isfinite(a[1]).all()


def test_noise_level_zero_steps_to_the_mean_and_its_log_prob_is_nan():
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    g, idx, nl = _case("s10_i1_nl0")
    assert nl == 0
    for mode in (dict(noise=g["eps"].cuda()), dict(seed=9, offset=3)):
        nxt, cast, lp, mean, std = sde_step_cfg(None, g["v"].cuda(), None, 1.0, None, g["x"].cuda(), 0, step_index=idx, sigmas=g["sigmas"].cuda(),
                                                out_dtype=torch.bfloat16, sde_type="sde", **mode)
        assert torch.equal(nxt.cpu(), g["mean"]) and torch.equal(mean.cpu(), g["mean"]) and torch.equal(cast.cpu(), g["mean"].to(torch.bfloat16))
        assert torch.isnan(lp).all() and (std == 0).all()


# ----------------------------------------------------------------------------- 2. bf16 inputs with CFG
@pytest.mark.parametrize("shape", SHAPES)
def test_flow_sde_step_cfg_bf16(shape):
    """bf16 v_u, v_t and x, CFG 4.5, at steps 0 (sigma == 1), 4 and 9 (sigma_prev == 0) of the 10-step schedule, epsilon injected: mean / next
    bit-equal to the float32 torch-CPU evaluation of the reference's operation sequence fed the reference's bf16 CFG roundings, cast ==
    next.to(bf16), log_prob within the bound of the float64 restatement, and the size-free identity
    log_prob == -mean(eps^2) / 2 - log w - log sqrt(2 pi) to rtol 2e-4."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    B = 2
    gen = torch.Generator().manual_seed(shape[1])
    full = (B,) + shape
    vu, vt, x = (torch.randn(full, generator=gen).to(torch.bfloat16) for _ in range(3))
    eps = torch.randn(full, generator=gen)
    sch = _scheduler(10)
    sig = sch.sigmas.cpu()
    v = R.cfg_combine(vu, vt, 4.5)
    assert v.dtype == torch.bfloat16
    for step in (0, 4, 9):
        nxt, cast, lp, mean, std = sde_step_cfg(sch, vu.cuda(), vt.cuda(), 4.5, None, x.cuda(), 0.7, noise=eps.cuda(), out_dtype=torch.bfloat16,
                                                step_index=step, sde_type="sde")
        s, sp = sig[step].repeat(B), sig[step + 1].repeat(B)
        o_nxt, _, o_mean, o_std, _ = R.flow_sde_step(v, x, s, sp, float(sig[1]), 0.7, eps=eps, dtype=torch.float32)
        assert torch.equal(mean.cpu(), o_mean) and torch.equal(nxt.cpu(), o_nxt) and torch.equal(std.reshape(-1).cpu(), o_std)
        assert torch.equal(cast.cpu(), o_nxt.to(torch.bfloat16))
        _, d_lp, _, _, w = R.flow_sde_step(v, x, s, sp, float(sig[1]), 0.7, eps=eps)
        bound = R.log_prob_bound(o_nxt, o_mean, w)
        print(shape, step, "log_prob", lp.tolist(), "float64", d_lp.tolist(), "bound", bound.tolist())
        assert ((lp.cpu().double() - d_lp).abs() <= bound).all()
        ident = -(eps.double() ** 2).mean(dim=(1, 2, 3)) / 2 - torch.log(w) - R.LOG_SQRT_2PI
        np.testing.assert_allclose(lp.cpu().numpy(), ident.numpy(), rtol=2e-4)


# ----------------------------------------------------------------------------- 3. the fan-out form
@pytest.mark.parametrize("mode", ["philox", "eps", "replay"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fan_out_flow_sde_step_has_the_bits_of_the_step_on_the_repeated_batch(mode, dtype):
    """advgrpo_flow_sde_step_branch(P = 2 rows, G copies) == advgrpo_flow_sde_step(x.repeat(G, ...)) with torch.equal on next, cast, mean,
    log_prob and std, for G = 3 and G = 9 at the three sizes, with CFG, sigma stride 0 and 1."""
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    sch = _scheduler()
    gen = torch.Generator().manual_seed(4)
    P, checked = 2, 0
    for G in (3, 9):
        for shape in SHAPES:
            vu, vt, x = (torch.randn(P, *shape, generator=gen).to(dtype).cuda() for _ in range(3))
            eps = torch.randn(P * G, *shape, generator=gen).cuda()
            prev = torch.randn(P * G, *shape, generator=gen).to(dtype).cuda()
            rep = lambda t: t.repeat(G, 1, 1, 1)
            for stride in (0, 1):
                kw = dict(noise_level=0.7, out_dtype=torch.bfloat16, want_mean=True, sde_type="sde")
                kw.update({"philox": dict(seed=1234, offset=77), "eps": dict(noise=eps), "replay": dict(prev_sample=prev)}[mode])
                if stride == 0:
                    t_in = t_rep = None
                    kw["step_index"] = 3
                else:
                    t_in = torch.stack([sch.timesteps[0], sch.timesteps[5]])
                    t_rep = t_in.repeat(G)
                a = sde_step_cfg(sch, vu, vt, 4.5, t_in, x, copies=G, **kw)
                b = sde_step_cfg(sch, rep(vu), rep(vt), 4.5, t_rep, rep(x), **kw)
                for name, u, v in zip(("next", "cast", "log_prob", "mean", "std"), a, b):
                    if mode == "replay" and name in ("next", "cast"):
                        assert u is None and v is None
                        continue
                    assert u.shape == v.shape and u.dtype == v.dtype, (name, u.shape, v.shape)
                    assert torch.equal(u, v), (name, G, shape, stride, (u.float() - v.float()).abs().max().item())
                assert a[2].shape == (P * G,) and torch.isfinite(a[2]).all()
                if mode != "replay":                       # the copies of a row really differ (their own epsilon each)
                    assert not torch.equal(a[0][0], a[0][P])
                checked += 1
    assert checked == 2 * 3 * 2


# ----------------------------------------------------------------------------- 4. backward, and backward with the KL term
def _bwd_inputs(dt, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (4, 16, 16, 16)
    vu, vt, ru, rt, x = (torch.randn(shape, generator=g).to(dt) for _ in range(5))
    prev = (x.float() + 0.1 * torch.randn(shape, generator=g)).to(dt)
    return shape, vu, vt, ru, rt, x, prev, g


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_flow_sde_step_backward_matches_autograd(dt):
    """Gradient w.r.t. both CFG halves against torch autograd on the restatement.  The tolerances of the Flow-CPS tests: 1e-5 of the gradient
    scale in f32; 2e-2 in bf16, where autograd itself rounds the gradient to bf16."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    shape, vu, vt, _, _, x, prev, g = _bwd_inputs(dt, 5)
    B, n = shape[0], vu[0].numel()
    glp = torch.randn(B, generator=g)
    sch = _scheduler(10)
    sig = sch.sigmas.cpu()
    vu_r, vt_r = vu.clone().requires_grad_(True), vt.clone().requires_grad_(True)
    _, lp, _, _, _ = R.flow_sde_step(R.cfg_combine(vu_r, vt_r, 4.5), x, sig[2].repeat(B), sig[3].repeat(B), float(sig[1]), 0.7, prev_sample=prev)
    (lp * glp.double()).sum().backward()
    gu, gt = torch.empty(shape, dtype=dt, device="cuda"), torch.empty(shape, dtype=dt, device="cuda")
    a = [t.cuda().contiguous() for t in (vu, vt, x, prev, glp)]
    _lib.check(lib.advgrpo_flow_sde_step_bwd(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.dtype_code(dt), 4.5, _lib.ptr(a[2]), _lib.dtype_code(dt),
                                             _lib.ptr(sch.sigmas[2:3]), _lib.ptr(sch.sigmas[3:4]), 0, 0.7, _lib.ptr(sch.sigmas[1:2]),
                                             _lib.ptr(a[3]), _lib.dtype_code(dt), _lib.ptr(a[4]), _lib.ptr(gu), _lib.ptr(gt), B, n,
                                             _lib.stream_ptr()))
    tol = 1e-5 if dt == torch.float32 else 2e-2
    scale = vt_r.grad.float().abs().max().item()
    d_t, d_u = (gt.cpu().float() - vt_r.grad.float()).abs().max().item(), (gu.cpu().float() - vu_r.grad.float()).abs().max().item()
    print(dt, "gradient scale", scale, "max |diff| text", d_t, "uncond", d_u)
    assert scale > 0 and d_t <= tol * scale and d_u <= tol * scale


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_flow_sde_step_backward_with_kl_term_matches_autograd(dt):
    """loss = sum_b glp_b log_prob_b + w * mean_b mean_elem (mean - mean_ref)^2: the gradient and the per-sample KL value against autograd on
    the restatement; with weight 0 the policy-only entry's bits."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    shape, vu, vt, ru, rt, x, prev, g = _bwd_inputs(dt, 6)
    B, n, wkl = shape[0], vu[0].numel(), 0.37
    glp = torch.randn(B, generator=g) * 1e-3              # (policy and KL gradients of the same order)
    sch = _scheduler(10)
    sig = sch.sigmas.cpu()
    step = lambda p, q: R.flow_sde_step(R.cfg_combine(p, q, 4.5), x, sig[2].repeat(B), sig[3].repeat(B), float(sig[1]), 0.7, prev_sample=prev)
    with torch.no_grad():
        mean_ref = step(ru, rt)[2].float()                # what the forward under the adapter-free transformer hands over: f32
    vu_r, vt_r = vu.clone().requires_grad_(True), vt.clone().requires_grad_(True)
    _, lp, mean, _, _ = step(vu_r, vt_r)
    kl_ref = ((mean - mean_ref.double()) ** 2).mean(dim=(1, 2, 3))
    ((lp * glp.double()).sum() + wkl * kl_ref.mean()).backward()
    gu, gt = torch.empty(shape, dtype=dt, device="cuda"), torch.empty(shape, dtype=dt, device="cuda")
    kl = torch.empty(B, dtype=torch.float32, device="cuda")
    ws = torch.empty(max(1, lib.advgrpo_sde_step_workspace_bytes(B, n) // 4), dtype=torch.float32, device="cuda")
    a = [t.cuda().contiguous() for t in (vu, vt, x, prev, glp, mean_ref)]
    head = (_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.dtype_code(dt), 4.5, _lib.ptr(a[2]), _lib.dtype_code(dt), _lib.ptr(sch.sigmas[2:3]),
            _lib.ptr(sch.sigmas[3:4]), 0, 0.7, _lib.ptr(sch.sigmas[1:2]), _lib.ptr(a[3]), _lib.dtype_code(dt), _lib.ptr(a[4]))
    _lib.check(lib.advgrpo_flow_sde_step_bwd_kl(*head, _lib.ptr(a[5]), wkl, _lib.ptr(gu), _lib.ptr(gt), _lib.ptr(kl), _lib.ptr(ws), B, n,
                                                _lib.stream_ptr()))
    tol = 1e-5 if dt == torch.float32 else 2e-2
    scale = vt_r.grad.float().abs().max().item()
    d_t, d_u = (gt.cpu().float() - vt_r.grad.float()).abs().max().item(), (gu.cpu().float() - vu_r.grad.float()).abs().max().item()
    print(dt, "gradient scale", scale, "max |diff| text", d_t, "uncond", d_u, "kl", kl.tolist(), "autograd", kl_ref.tolist())
    assert scale > 0 and d_t <= tol * scale and d_u <= tol * scale
    assert torch.allclose(kl.cpu(), kl_ref.detach().float(), rtol=2e-5 if dt == torch.float32 else 2e-2)
    gu0, gt0 = torch.empty_like(gu), torch.empty_like(gt)
    _lib.check(lib.advgrpo_flow_sde_step_bwd(*head, _lib.ptr(gu0), _lib.ptr(gt0), B, n, _lib.stream_ptr()))
    _lib.check(lib.advgrpo_flow_sde_step_bwd_kl(*head, _lib.ptr(a[5]), 0.0, _lib.ptr(gu), _lib.ptr(gt), _lib.ptr(kl), _lib.ptr(ws), B, n,
                                                _lib.stream_ptr()))
    assert torch.equal(gu, gu0) and torch.equal(gt, gt0)


# ----------------------------------------------------------------------------- 5. the full-trajectory rollout
class _StandinVae:
    """Same arithmetic as the stand-in used for the golden: rescale, stand-in decode, postprocess."""

    def decode_to_image(self, latents):
        from oracle.standin import standin_vae_decode
        z = (latents / 1.5305) + 0.0609
        return (standin_vae_decode(z.to(torch.float32)) / 2 + 0.5).clamp(0, 1)


class _Standin(torch.nn.Module):
    """The golden's transformer stand-in (make_golden_branch_rollout.py's DoorCast; the latents arrive in the embedding dtype here)."""

    def __init__(self):
        super().__init__()
        from oracle.standin import StandinVelocity
        self.net = StandinVelocity()
        self.config = type("C", (), {"in_channels": 16})()

    def forward(self, hidden_states, timestep, encoder_hidden_states, pooled_projections, joint_attention_kwargs=None, return_dict=False):
        assert hidden_states.dtype == encoder_hidden_states.dtype
        return self.net(hidden_states, timestep, encoder_hidden_states, pooled_projections)


@pytest.mark.parametrize("case", ["fp32_cfg", "fp32_nocfg", "bf16_cfg", "bf16_nocfg"])
def test_full_trajectory_rollout_matches_the_reference(case):
    """pipeline_with_logprob (sd3_pipeline_with_logprob.py) with the reference's epsilon injected, against what the reference's own function
    returned on the stand-in network and decoder: len(all_latents) == steps + 1, the first in the embedding dtype and the rest float32, every
    latent, every log-prob and the image within the bounds tests/test_gpu_branch_rollout.py uses for its reference trajectory."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob import pipeline_with_logprob
    from adv_grpo_amd.pipeline import SD3Pipeline
    npz = np.load(GOLD_FULL)
    g = {k.split("/", 1)[1]: npz[k] for k in npz.files if k.startswith(case + "/")}
    dtype = torch.float32 if case.startswith("fp32") else torch.bfloat16
    steps, P, hw = (int(v) for v in g["meta"])
    guidance, noise_level = (float(v) for v in g["scalars"])
    pipe = SD3Pipeline(_Standin().cuda(), _StandinVae(), "cuda")
    tt = lambda k: torch.from_numpy(g[k]).to(dtype).cuda()
    noises = [torch.from_numpy(npz[f"noise/{i}"]).cuda() for i in range(steps)]
    image, lats, lps = pipeline_with_logprob(
        pipe, prompt_embeds=tt("pe"), pooled_prompt_embeds=tt("ppe"), negative_prompt_embeds=tt("npe"), negative_pooled_prompt_embeds=tt("nppe"),
        num_inference_steps=steps, guidance_scale=guidance, output_type="pt", height=hw, width=hw, noise_level=noise_level,
        latents=torch.from_numpy(npz["lat0"]).cuda(), noises=noises)
    assert len(lats) == steps + 1 and len(lps) == steps
    assert lats[0].dtype == dtype and all(a.dtype == torch.float32 for a in lats[1:]) and all(a.dtype == torch.float32 for a in lps)
    lat = torch.stack([a.float() for a in lats], 1).cpu().numpy()
    lp = torch.stack(lps, 1).cpu().numpy()
    assert lat.shape == g["latents"].shape == (P, steps + 1, 16, hw // 8, hw // 8) and lp.shape == g["log_probs"].shape
    if dtype == torch.bfloat16:                            # recorded before the cast: not bf16 values
        assert not torch.equal(lats[1], lats[1].to(torch.bfloat16).float())
    tol = 2e-5 if dtype == torch.float32 else 2 ** -7
    print(f"{case}: max |latents diff| {np.abs(lat - g['latents']).max():.3e}  log-probs {lp[0].tolist()} golden {g['log_probs'][0].tolist()}  "
          f"max |image diff| {np.abs(image.float().cpu().numpy() - g['image']).max():.3e}")
    assert np.allclose(lat, g["latents"], atol=tol * 4, rtol=tol)
    assert np.allclose(lp, g["log_probs"], rtol=5e-3 if dtype == torch.bfloat16 else 1e-4)
    assert np.allclose(image.float().cpu().numpy(), g["image"], atol=2e-2 if dtype == torch.bfloat16 else 1e-4)


def test_full_trajectory_rollout_with_the_flow_sde_step():
    """sde_type="sde" on the stand-in stack with in-kernel Philox: every log-prob finite (every step is stochastic), the same seed gives the
    same bits, and each recorded float32 latent replays to its own log-prob through flow_sde_step_with_logprob."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob import pipeline_with_logprob
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import flow_sde_step_with_logprob
    from adv_grpo_amd.pipeline import SD3Pipeline
    npz = np.load(GOLD_FULL)
    tt = lambda k: torch.from_numpy(npz["bf16_nocfg/" + k]).to(torch.bfloat16).cuda()
    pipe = SD3Pipeline(_Standin().cuda(), _StandinVae(), "cuda")
    kw = dict(prompt_embeds=tt("pe"), pooled_prompt_embeds=tt("ppe"), num_inference_steps=4, guidance_scale=1.0, output_type="latent", height=64,
              width=64, seed=11, sde_type="sde")
    final, lats, lps = pipeline_with_logprob(pipe, **kw)
    final2, lats2, lps2 = pipeline_with_logprob(pipe, **kw)
    assert len(lats) == 5 and all(torch.isfinite(a).all() for a in lps) and torch.equal(final, lats[-1].to(torch.bfloat16))
    assert all(torch.equal(a, b) for a, b in zip(lats + lps + [final], lats2 + lps2 + [final2]))
    for i in range(4):
        x = lats[i].to(torch.bfloat16)
        t = pipe.scheduler.timesteps[i]
        v = pipe.transformer(x, t.expand(2), tt("pe"), tt("ppe"))[0]
        _, lp, _, _ = flow_sde_step_with_logprob(pipe.scheduler, v, t.repeat(2), x, noise_level=0.7, prev_sample=lats[i + 1])
        print("step", i, "log_prob", lps[i].tolist(), "replayed", lp.tolist())
        assert torch.allclose(lp, lps[i], rtol=0, atol=2e-5)


# ----------------------------------------------------------------------------- 6 - 7. defaults and the Trainer option
def test_default_sde_type_changes_no_bits():
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_random
    from test_gpu_branch_rollout import _kw, _stack
    pipe, embeds = _stack()
    a = pipeline_with_logprob_random(pipe, **_kw(embeds[2], 2, 0))
    b = pipeline_with_logprob_random(pipe, sde_type="cps", **_kw(embeds[2], 2, 0))
    c = pipeline_with_logprob_random(pipe, sde_type="sde", **_kw(embeds[2], 2, 0))
    assert torch.equal(a[0], b[0]) and len(a[1]) == 3
    for x, y in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert torch.equal(a[1][0], c[1][0]) and not torch.equal(a[1][1], c[1][1])       # the same initial latents, another step from there
    assert all(torch.isfinite(v).all() for v in c[2]) and not torch.equal(a[2][0], c[2][0])


def test_trainer_with_cps_samples_what_it_always_did():
    """sample.sde_type = "cps" against a config without the key: the sample dicts of the same seed are torch.equal on every tensor."""
    from test_gpu_branch_rollout import _trainer
    tr_a, _ = _trainer()
    assert tr_a.cfg.sample.get("sde_type") is None
    a = tr_a.sample_epoch()
    tr_b, _ = _trainer(sde_type="cps")
    b = tr_b.sample_epoch()
    torch.cuda.synchronize()
    assert set(a) == set(b) and sum(isinstance(v, torch.Tensor) for v in a.values()) >= 9
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("beta", [0.0, 0.04])
def test_trainer_epoch_with_the_flow_sde_step(beta):
    """sample.sde_type = "sde" on the small stack: one epoch runs, rewards / advantages / the G-step loss are finite and the adapters move;
    beta > 0 goes through advgrpo_flow_sde_step_bwd_kl."""
    from test_gpu_branch_rollout import _trainer
    tr_, model = _trainer(sde_type="sde")
    tr_.cfg.train.beta = beta
    seen, recs = {}, []
    g_step = tr_.g_step
    tr_.g_step = lambda samples: (seen.update(samples), g_step(samples))[1]
    log = tr_.logger.log
    tr_.logger.log = lambda rec, step=None: (recs.append(dict(rec)), log(rec, step))[1]
    p0 = model.params.clone()
    info = tr_.run_epoch()
    losses = [float(r["loss"]) for r in recs if "loss" in r]
    assert info["phase"] == "G" and losses and all(math.isfinite(v) for v in losses) and not torch.equal(model.params, p0)
    assert torch.isfinite(model.params).all()
    assert torch.isfinite(seen["rewards"]).all() and torch.isfinite(seen["advantages"]).all() and torch.isfinite(seen["log_probs"]).all()
    if beta > 0:
        kls = [float(r["kl_loss"]) for r in recs if "kl_loss" in r]
        assert kls and all(math.isfinite(v) for v in kls)


# ----------------------------------------------------------------------------- 8. the C entries' argument checks
def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every bad-argument case returns non-zero, raises _lib.AdvGrpoError through _lib.check and leaves the sentinel-filled outputs alone.
    Argument checks only: each call is refused on the host, nothing reaches the device."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    B, n = 2, 2048
    vu, vt, x, prev, eps = (torch.randn(B, n, device="cuda") for _ in range(5))
    glp = torch.randn(B, device="cuda")
    sig = torch.tensor([0.9, 0.8, 0.7], device="cuda")
    SENT = -12288.0
    outs = {k: torch.full(s, SENT, device="cuda") for k, s in (("next", (B, n)), ("mean", (B, n)), ("lp", (B,)), ("std", (B,)), ("gu", (B, n)),
                                                               ("gt", (B, n)), ("kl", (B,)))}
    ws = torch.full((lib.advgrpo_sde_step_workspace_bytes(B, n) // 4,), SENT, device="cuda")

    def fwd(branch=False, **over):
        a = dict(vu=vu.data_ptr(), smax=sig[1:2].data_ptr(), mode=_lib.SDE_PHILOX, eps=None, prev=None, n=n)
        a.update(over)
        fn = lib.advgrpo_flow_sde_step_branch if branch else lib.advgrpo_flow_sde_step
        return fn(a["vu"], vt.data_ptr(), _lib.F32, 4.5, x.data_ptr(), _lib.F32, sig[0:1].data_ptr(), sig[1:2].data_ptr(), 0, 0.7, a["smax"],
                  a["mode"], a["eps"], 1, 0, a["prev"], _lib.F32, outs["next"].data_ptr(), None, 0, outs["mean"].data_ptr(),
                  outs["lp"].data_ptr(), outs["std"].data_ptr(), ws.data_ptr(), *((1, B) if branch else (B,)), a["n"], _lib.stream_ptr())

    def bwd(kl=False, **over):
        a = dict(smax=sig[1:2].data_ptr(), n=n, mean_ref=outs["mean"].data_ptr())
        a.update(over)
        head = (vu.data_ptr(), vt.data_ptr(), _lib.F32, 4.5, x.data_ptr(), _lib.F32, sig[0:1].data_ptr(), sig[1:2].data_ptr(), 0, 0.7, a["smax"],
                prev.data_ptr(), _lib.F32, glp.data_ptr())
        if kl:
            return lib.advgrpo_flow_sde_step_bwd_kl(*head, a["mean_ref"], 0.1, outs["gu"].data_ptr(), outs["gt"].data_ptr(), outs["kl"].data_ptr(),
                                                    ws.data_ptr(), B, a["n"], _lib.stream_ptr())
        return lib.advgrpo_flow_sde_step_bwd(*head, outs["gu"].data_ptr(), outs["gt"].data_ptr(), B, a["n"], _lib.stream_ptr())
    bad = [dict(n=12), dict(n=0), dict(smax=None), dict(mode=3), dict(mode=-1), dict(mode=_lib.SDE_EPS), dict(mode=_lib.SDE_REPLAY), dict(vu=None)]
    calls = [(fwd, dict(branch=br, **o)) for br in (False, True) for o in bad]
    calls += [(bwd, dict(kl=k, **o)) for k in (False, True) for o in (dict(n=12), dict(smax=None))] + [(bwd, dict(kl=True, mean_ref=None))]
    for fn, over in calls:
        rc = fn(**over)
        assert rc != 0, over
        with pytest.raises(_lib.AdvGrpoError, match="sde_step"):
            _lib.check(rc)
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + [("workspace", ws)]:
        assert (t == SENT).all(), k
    # and the same arguments without a fault are accepted
    assert fwd() == 0 and fwd(branch=True) == 0 and fwd(mode=_lib.SDE_EPS, eps=eps.data_ptr()) == 0
    assert fwd(mode=_lib.SDE_REPLAY, prev=prev.data_ptr()) == 0 and bwd() == 0 and bwd(kl=True) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(outs["lp"]).all() and torch.isfinite(outs["gu"]).all() and torch.isfinite(outs["kl"]).all()
