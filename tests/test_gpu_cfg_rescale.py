"""GPU: the stochastic steps under Qwen-Image's norm-rescaled true CFG -- advgrpo_sde_step_rescaled, advgrpo_flow_sde_step_rescaled,
their backward entries, ``sde_step_cfg(cfg_rescale=True)``, the rollout keyword, ``micro_step`` and the Trainer option.

1. The fused entry against kernels already in the tree, bit for bit: advgrpo_qwen_cfg_euler_step on an f32 zero sample with sigma = 0,
   sigma_next = 1 returns exactly the rescaled v (dt = 1), and advgrpo_sde_step / advgrpo_flow_sde_step with v_text = NULL steps from it.
   next, cast, mean and std are torch.equal with no cap; log_prob differs by summation order only (the 2e-6 bound of
   flow_sde_reference.log_prob_bound; for Flow-CPS, whose log_prob is the one term -mean d^2, 2e-6 of it).
2. Against the torch restatement (the `sequenced=True` path): tokens whose bf16 norms round as torch.norm's do are elementwise equal,
   the others are excluded and their share is capped by qwen_sampler_reference.MISMATCH_CAP.
3. The backward against float64 autograd of the restatement, bound by the rule of cfg_rescale_reference.measure_emulation.
4. An all-zero token makes its own sample's log_prob NaN and leaves the other samples' bits alone.
5. Sample, then replay.   6. End to end on a tiny Qwen-Image.

Shapes: qwen_sampler_reference.SHAPES -- one token; 15 tokens per sample in the one-token-per-lane layout (a block that mixed samples
would show here); a token row longer than one block; the two-tokens-per-lane layout over several blocks."""
import math

import pytest
import torch

import cfg_rescale_reference as R
import flow_sde_reference as F
import qwen_sampler_reference as Q

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SHAPES]
SIG = None


def _sig():
    global SIG
    if SIG is None:
        SIG = R.SIGMAS.cuda()
    return SIG


def _step(vu, vt, x, sde_type, **kw):
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    kw.setdefault("out_dtype", bf16)
    out = sde_step_cfg(None, vu, vt, R.SCALE, None, x, R.NOISE_LEVEL, step_index=R.STEP, sigmas=_sig(), sde_type=sde_type, **kw)
    torch.cuda.synchronize()
    return out


def _mode_kw(mode, shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(shape, generator=g)
    prev = torch.randn(shape, generator=g).to(dt)
    return {"philox": dict(seed=1234, offset=77), "eps": dict(noise=eps.cuda()), "replay": dict(prev_sample=prev.cuda())}[mode]


def _kernel_v(neg, pos):
    """The rescaled prediction out of advgrpo_qwen_cfg_euler_step: zero f32 sample, sigma 0 -> 1, so dt = 1 and the output is v."""
    from adv_grpo_amd import qwen_generate as G
    table = torch.tensor([0.0, 1.0], device="cuda")
    v = G.cfg_euler_step(neg, pos, torch.zeros(neg.shape, dtype=torch.float32, device="cuda"), table, 0, R.SCALE)
    assert torch.equal(v.to(neg.dtype).float(), v)          # bf16 predictions: the values are bf16 values
    return v.to(neg.dtype)


def _lp_bound(sde_type, nxt_or_prev, mean, B):
    d2 = ((nxt_or_prev.double() - mean.double()) ** 2).flatten(1).mean(1)
    if sde_type == "cps":
        return 2e-6 * d2
    sig, sigp = R.schedule_rows(B)
    z = torch.zeros(B, 1)
    w = F.flow_sde_step(z, z, sig, sigp, float(R.SIGMAS[1]), R.NOISE_LEVEL, prev_sample=z)[4]
    return F.log_prob_bound(nxt_or_prev.cpu(), mean.cpu(), w).to(d2.device)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode", ["eps", "philox", "replay"])
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("dt", [bf16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_fused_step_has_the_bits_of_the_kernels_already_in_the_tree(shape, dt, sde_type, mode):
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, dt, dt, 1.0, 2000 + R.SHAPES.index(shape)))
    kw = _mode_kw(mode, shape, dt, 31)
    got = _step(neg, pos, x, sde_type, cfg_rescale=True, **kw)
    ref = _step(_kernel_v(neg, pos), None, x, sde_type, **kw)
    for name, a, b in zip(("next", "cast", "log_prob", "mean", "std"), got, ref):
        if mode == "replay" and name in ("next", "cast"):
            assert a is None and b is None
        elif name != "log_prob":
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    assert got[1] is None or got[1].dtype == bf16
    moved = kw["prev_sample"] if mode == "replay" else got[0]
    bound = _lp_bound(sde_type, moved, got[3], shape[0])
    diff = (got[2].double() - ref[2].double()).abs()
    print(shape, dt, sde_type, mode, "log_prob", got[2].tolist(), "reference kernels", ref[2].tolist(), "|diff|", diff.tolist(), "bound", bound.tolist())
    assert torch.isfinite(got[2]).all() and (diff <= bound).all()
    again = _step(neg, pos, x, sde_type, cfg_rescale=True, **kw)
    assert torch.equal(again[2], got[2]) and torch.equal(again[3], got[3])        # fixed reduction order: run to run the same bits


@pytest.mark.parametrize("sde_type", ["cps", "sde"])
def test_philox_draws_are_the_plain_steps_and_no_second_prediction_is_the_plain_step(sde_type):
    """Element i of sample b gets the normal advgrpo_sde_step gives it: with v_text = None (nothing to rescale) the rescaled entry IS
    the plain step, in both lane layouts -- called directly, since sde_step_cfg routes that case to the plain entry."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    for shape in ((2, 16, 6, 10), (3, 16, 64, 64)):
        v, _, x = (t.cuda() for t in R.make_inputs(shape, bf16, bf16, 1.0, 41))
        ref = _step(v, None, x, sde_type, seed=99, offset=12345)
        B = shape[0]
        nxt, mean = (torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(2))
        cast = torch.empty(shape, dtype=bf16, device="cuda")
        lp, std = (torch.empty(B, device="cuda") for _ in range(2))
        ws = torch.empty(lib.advgrpo_sde_step_rescaled_workspace_bytes(*shape, 2) // 4, device="cuda")
        sig = _sig()
        flow = sde_type == "sde"
        level = (R.NOISE_LEVEL, sig[1:2].data_ptr()) if flow else (float(math.sin(R.NOISE_LEVEL * math.pi / 2)),)
        fn = lib.advgrpo_flow_sde_step_rescaled if flow else lib.advgrpo_sde_step_rescaled
        _lib.check(fn(v.data_ptr(), None, _lib.BF16, R.SCALE, x.data_ptr(), _lib.BF16, sig[R.STEP:R.STEP + 1].data_ptr(),
                      sig[R.STEP + 1:R.STEP + 2].data_ptr(), 0, *level, _lib.SDE_PHILOX, None, 99, 12345, None, 0, nxt.data_ptr(),
                      cast.data_ptr(), _lib.BF16, mean.data_ptr(), lp.data_ptr(), std.data_ptr(), ws.data_ptr(), *shape, 2, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(nxt, ref[0]) and torch.equal(cast, ref[1]) and torch.equal(mean, ref[3]) and torch.equal(std, ref[4].reshape(-1))
        assert ((lp.double() - ref[2].double()).abs() <= _lp_bound(sde_type, nxt, mean, B)).all()


def test_shapes_the_kernels_are_not_built_for_are_refused():
    from adv_grpo_amd import _lib
    for shape in ((1, 8, 4, 4), (1, 16, 4, 3), (1, 16, 3, 4)):
        t = torch.zeros(shape, dtype=bf16, device="cuda")
        with pytest.raises((_lib.AdvGrpoError, ValueError)):
            _step(t, t, t, "cps", seed=1, cfg_rescale=True)
    lib = _lib.load()
    t = torch.zeros(1, 16, 4, 4, dtype=bf16, device="cuda")
    lp = torch.full((1,), -7.0, device="cuda")
    ws = torch.empty(16, device="cuda")
    sig = _sig()
    for C, H, W, patch in ((8, 4, 4, 2), (16, 4, 4, 1), (16, 3, 4, 2), (16, 4, 6 + 1, 2)):       # refused on the host: nothing is launched
        rc = lib.advgrpo_sde_step_rescaled(t.data_ptr(), t.data_ptr(), _lib.BF16, 4.0, t.data_ptr(), _lib.BF16, sig[0:1].data_ptr(),
                                           sig[1:2].data_ptr(), 0, 0.5, _lib.SDE_PHILOX, None, 1, 0, None, 0, None, None, 0, None,
                                           lp.data_ptr(), None, ws.data_ptr(), 1, C, H, W, patch, _lib.stream_ptr())
        assert rc != 0
        with pytest.raises(_lib.AdvGrpoError, match="sde_step_rescaled"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert lp.item() == -7.0


# ---------------------------------------------------------------------------------------------------------------- 2
RESTATEMENT_CASES = [c for c in Q.cases() if c[2] == bf16 and c[4] == 1.0]      # bf16 predictions, both sample dtypes, every shape


@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("name,shape,vd,xd,mult,seed", RESTATEMENT_CASES, ids=[c[0] for c in RESTATEMENT_CASES])
def test_fused_step_against_the_torch_restatement(name, shape, vd, xd, mult, seed, sde_type):
    """The bf16-prediction inputs of tests/test_gpu_qwen_sampler.py (tests/test_qwen_sampler_host.py measures their norms).  `sequenced=True` is the restatement on the device: torch's combine, norms and rescale, then the plain step.  A
    token whose two bf16 norms come out of the kernel's summation order as they come out of torch.norm has the restatement's bits in
    mean and next; the other tokens are left out, at most MISMATCH_CAP of them."""
    cpu = R.make_inputs(shape, vd, xd, mult, seed)
    neg, pos, x = (t.cuda() for t in cpu)
    eps = torch.randn(shape, generator=torch.Generator().manual_seed(32)).cuda()
    got = _step(neg, pos, x, sde_type, cfg_rescale=True, noise=eps)
    ref = _step(neg, pos, x, sde_type, cfg_rescale=True, sequenced=True, noise=eps)
    cn_k, nn_k = R.kernel_order_norms(cpu[0], cpu[1])
    p, c = Q.pack(pos), Q.combine(Q.pack(neg), Q.pack(pos), R.SCALE)               # torch.norm where the restatement ran it: on the device
    same = ((cn_k.cuda() == torch.norm(p, dim=-1, keepdim=True)) & (nn_k.cuda() == torch.norm(c, dim=-1, keepdim=True))).squeeze(-1)   # [B, N]
    share = 1.0 - same.double().mean().item()
    print(name, sde_type, "tokens", same.numel(), "excluded share", share)
    assert share <= Q.MISMATCH_CAP
    for name, a, b in (("mean", got[3], ref[3]), ("next", got[0], ref[0]), ("cast", got[1], ref[1])):
        eq = (Q.pack(a) == Q.pack(b)).all(dim=-1)
        assert eq[same].all(), (name, (~eq[same]).sum().item())
    assert torch.equal(got[4], ref[4])
    moved = got[0]
    if bool(same.all()):
        assert ((got[2].double() - ref[2].double()).abs() <= _lp_bound(sde_type, moved, got[3], shape[0])).all()


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def bwd_bound():
    worst, bound = R.measure_emulation()
    print("float32 emulation against float64 autograd (share of the gradient scale):", worst, "-> GPU bound", bound)
    return bound


@pytest.mark.parametrize("with_kl", [False, True], ids=["policy", "kl"])
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("dt", [torch.float32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_backward_against_float64_autograd(bwd_bound, shape, dt, sde_type, with_kl):
    """Both gradients within the bound of the tolerance rule (cfg_rescale_reference.measure_emulation: the project's 1e-5 of the gradient
    scale in f32; in bf16 four times the float32 emulation's own error, 3.1e-2, because that error -- 7.7e-3 -- exceeds a quarter of
    the project's 2e-2).  With mean_ref the per-sample KL value too: rtol 2e-5 in f32, 2e-2 in bf16, as tests/test_gpu_flow_sde.py."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    c = R.bwd_case(shape, dt, sde_type, with_kl)
    ref_n, ref_p, kl_ref = R.grad_autograd(sde_type, c["v_neg"], c["v_pos"], c["x"], c["sig"], c["sigp"], c["prev"], c["glp"], c["mean_ref"],
                                           c["kl_weight"])
    B = shape[0]
    d = {k: (v.cuda().contiguous() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    gu, gt = (torch.empty(shape, dtype=dt, device="cuda") for _ in range(2))
    kl = torch.empty(B, device="cuda") if with_kl else None
    ws = torch.empty(lib.advgrpo_sde_step_rescaled_workspace_bytes(*shape, 2) // 4, device="cuda") if with_kl else None
    sig = _sig()
    flow = sde_type == "sde"
    level = (R.NOISE_LEVEL, sig[1:2].data_ptr()) if flow else (float(math.sin(R.NOISE_LEVEL * math.pi / 2)),)
    fn = lib.advgrpo_flow_sde_step_rescaled_bwd if flow else lib.advgrpo_sde_step_rescaled_bwd
    code = _lib.dtype_code(dt)
    _lib.check(fn(d["v_neg"].data_ptr(), d["v_pos"].data_ptr(), code, R.SCALE, d["x"].data_ptr(), code, sig[R.STEP:R.STEP + 1].data_ptr(),
                  sig[R.STEP + 1:R.STEP + 2].data_ptr(), 0, *level, d["prev"].data_ptr(), code, d["glp"].data_ptr(), _lib.ptr(d["mean_ref"]),
                  c["kl_weight"], gu.data_ptr(), gt.data_ptr(), _lib.ptr(kl), _lib.ptr(ws), *shape, 2, _lib.stream_ptr()))
    torch.cuda.synchronize()
    err = R.rel_err(gu.cpu(), gt.cpu(), ref_n, ref_p)
    print(shape, dt, sde_type, "kl" if with_kl else "policy", "gradient scale", ref_p.abs().max().item(), "error / scale", err, "bound", bwd_bound[dt])
    assert torch.isfinite(gu.float()).all() and torch.isfinite(gt.float()).all() and ref_p.abs().max().item() > 0
    assert err <= bwd_bound[dt]
    if with_kl:
        print("kl", kl.tolist(), "autograd", kl_ref.tolist())
        assert torch.allclose(kl.cpu(), kl_ref.float(), rtol=2e-5 if dt == torch.float32 else 2e-2, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("shape", [(3, 16, 6, 10), (3, 16, 64, 64)], ids=["3x16x6x10", "3x16x64x64"])
def test_all_zero_token_is_nan_in_its_own_sample_only(shape, sde_type):
    """The pipeline's own behaviour (no epsilon in the norm ratio): 0 / 0 in one token of sample 1 makes that sample's log_prob NaN; the
    samples before and after it keep the bits of the run without the zero token."""
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, bf16, bf16, 1.0, 79))
    clean = _step(neg, pos, x, sde_type, cfg_rescale=True, seed=5, offset=9)
    neg[1, :, 2:4, 4:6] = 0
    pos[1, :, 2:4, 4:6] = 0
    got = _step(neg, pos, x, sde_type, cfg_rescale=True, seed=5, offset=9)
    assert torch.isnan(got[2][1]) and torch.isfinite(got[2][[0, 2]]).all() and torch.isfinite(clean[2]).all()
    assert torch.equal(got[2][[0, 2]], clean[2][[0, 2]])
    nan = torch.isnan(got[0])
    want = torch.zeros_like(nan)
    want[1, :, 2:4, 4:6] = True
    assert torch.equal(nan, want)
    for a, b in ((got[0], clean[0]), (got[3], clean[3])):
        assert torch.equal(a[[0, 2]], b[[0, 2]]) and torch.equal(a[~want], b[~want])


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_sampled_step_replays_to_its_own_log_prob(shape, sde_type):
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, bf16, bf16, 1.0, 81))
    nxt, cast, lp, mean, std = _step(neg, pos, x, sde_type, cfg_rescale=True, seed=7, offset=3)
    stored = nxt.clone()
    a, b, lp_r, mean_r, std_r = _step(neg, pos, x, sde_type, cfg_rescale=True, prev_sample=nxt)
    print(shape, sde_type, "log_prob", lp.tolist(), "replayed", lp_r.tolist())
    assert a is None and b is None and torch.equal(nxt, stored)            # the replay hands nothing back and leaves prev_sample alone
    assert torch.equal(mean_r, mean) and torch.equal(std_r, std) and torch.equal(cast, nxt.to(bf16))
    assert torch.isfinite(lp).all() and torch.allclose(lp_r, lp, rtol=0, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------- 6
RES = 256
# The windowed rollout stores next_latents in bf16 and records log_prob from the sample before that cast, so a replay moves by
# mean(2 d e) with e the cast's error: about 2 * 0.85 * 8e-4 / sqrt(n) for d ~ std ~ 0.85 -- 1.1e-5 at the n = 16384 of a 256 x 256
# image, 5e-6 at the 65536 of 512 x 512.  The Trainer test replays within 2e-5, so it runs at 512.
RES_REPLAY = 512


def _rollout_kw(qcfg, G):
    from test_gpu_qwen_masked import NT
    g = torch.Generator().manual_seed(8)
    pe, npe = (torch.randn(1, NT, qcfg.joint_attention_dim, generator=g).to(bf16).cuda() for _ in range(2))
    pooled = torch.zeros(1, 8, dtype=bf16, device="cuda")
    return dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=pooled,
                num_inference_steps=4, guidance_scale=4.0, height=RES, width=RES, noise_level=0.8, mini_num_image_per_prompt=G,
                train_num_steps=2, process_index=0, sample_num_steps=4, random_timestep=0, seed=77, output_type="latent")


def test_rollout_keyword_off_changes_no_bits_and_on_changes_the_latents():
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_random
    from test_gpu_qwen_masked import _cfg, _pipe
    qcfg = _cfg(2)
    pipe, _ = _pipe(qcfg, 5)
    kw = _rollout_kw(qcfg, 2)
    a = pipeline_with_logprob_random(pipe, **kw)
    b = pipeline_with_logprob_random(pipe, cfg_rescale=False, **kw)
    c = pipeline_with_logprob_random(pipe, cfg_rescale=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and len(a[1]) == 3 and len(a[2]) == 2
    for u, v in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]):
        assert u.dtype == v.dtype and torch.equal(u, v)
    assert torch.equal(a[1][0], c[1][0]) and not torch.equal(a[1][1], c[1][1])     # the same initial latents, another step from there
    assert all(torch.isfinite(v).all() for v in c[2]) and all(torch.isfinite(v.float()).all() for v in c[1])
    # the full-trajectory rollout reads the switch from the pipeline object (its keyword list is pinned)
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob import pipeline_with_logprob as full_trajectory
    fkw = {k: kw[k] for k in ("prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds",
                              "num_inference_steps", "guidance_scale", "height", "width", "noise_level", "seed", "output_type")}
    plain = full_trajectory(pipe, **fkw)
    pipe.cfg_rescale = True
    try:
        resc = full_trajectory(pipe, **fkw)
    finally:
        del pipe.cfg_rescale
    assert torch.equal(plain[1][0], resc[1][0]) and not torch.equal(plain[1][1], resc[1][1]) and len(resc[1]) == 5
    assert all(torch.isfinite(v).all() for v in resc[2])
    again = full_trajectory(pipe, **fkw)
    assert all(torch.equal(u, v) for u, v in zip(plain[1] + plain[2], again[1] + again[2]))     # the attribute gone: the default bits again
    one = pipeline_with_logprob_random(pipe, cfg_rescale=True, **dict(kw, guidance_scale=1.0))   # without CFG: a no-op
    two = pipeline_with_logprob_random(pipe, **dict(kw, guidance_scale=1.0))
    assert all(torch.equal(u, v) for u, v in zip(one[1] + one[2], two[1] + two[2]))


@pytest.mark.parametrize("beta", [0.0, 0.04])
def test_micro_step_replays_the_rollout_and_the_trainer_moves_the_adapters(monkeypatch, beta):
    """Trainer.run_epoch with sample.cfg_rescale on the tiny Qwen-Image: rollout and micro_step get the keyword; before the first optimizer
    step the policy is the rollout's, so the first group's micro-steps replay the recorded log-probs (atol 2e-5); the G-step then
    changes the LoRA parameters, with finite losses.  beta > 0: the reference mean follows the option and the backward entry takes
    mean_ref, kl_out and the workspace."""
    from adv_grpo_amd import trainer as T
    from adv_grpo_amd.config.experiments import get_config
    from test_gpu_qwen_masked import NT, _cfg, _pipe
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
    cfg.resolution = RES_REPLAY
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.num_batches_per_epoch = 2
    cfg.sample.groups_in_flight = 1
    cfg.sample.cfg_rescale = True
    cfg.train.gradient_accumulation_steps = 1
    cfg.train.beta = beta
    qcfg = _cfg(2)
    pipe, model = _pipe(qcfg, 5)
    data = T.SyntheticData(n_prompts=50, n_tokens=NT, ctx_dim=qcfg.joint_attention_dim, pooled_dim=8, resolution=RES_REPLAY)
    tr = T.Trainer(cfg, pipe, data, None, None)
    assert tr.cfg_rescale is True
    seen = {"rollout": [], "replay": []}
    recs = []
    real_rollout, real_micro = T.pipeline_with_logprob_random, T.g_step.micro_step

    def rollout(p, **kw):
        seen["rollout"].append(kw.get("cfg_rescale"))
        return real_rollout(p, **kw)

    def micro(m, sched, sample, j, embeds, pooled, old, adv, **kw):
        info = real_micro(m, sched, sample, j, embeds, pooled, old, adv, **kw)
        seen["replay"].append((kw.get("cfg_rescale"), (info["log_prob"] - old).abs().max().item(), torch.isfinite(old).all().item()))
        return info
    monkeypatch.setattr(T, "pipeline_with_logprob_random", rollout)
    monkeypatch.setattr(T.g_step, "micro_step", micro)
    log = tr.logger.log
    monkeypatch.setattr(tr.logger, "log", lambda rec, step=None: (recs.append(dict(rec)), log(rec, step))[1])
    p0 = model.params.clone()
    info = tr.run_epoch()
    Tn = cfg.sample.train_num_steps
    print("replayed - recorded log_prob, max |diff| per micro-step:", [d for _, d, _ in seen["replay"]])
    assert info["phase"] == "G" and seen["rollout"] == [True, True] and len(seen["replay"]) == 2 * Tn
    assert all(flag is True and finite for flag, _, finite in seen["replay"])
    for _, diff, _ in seen["replay"][:Tn]:                                   # on-policy: the first group, before the optimizer step
        assert diff <= 2e-5, diff
    losses = [float(r["loss"]) for r in recs if "loss" in r]
    assert losses and all(math.isfinite(v) for v in losses)
    if beta > 0:
        kls = [float(r["kl_loss"]) for r in recs if "kl_loss" in r]
        assert kls and all(math.isfinite(v) and v >= 0 for v in kls)
    assert not torch.equal(model.params, p0) and torch.isfinite(model.params).all()
