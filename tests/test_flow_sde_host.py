"""CPU: the Flow-SDE step's restatement (tests/flow_sde_reference.py) against what the REFERENCE's own function returned
(tests/golden/flow_sde.npz), the closed-form gradients the backward kernels evaluate against torch autograd, and the surface of the
feature: the launcher flag, the config default, the Trainer's hand-over, the argument check, the C declarations, the full-trajectory
function's signature against the reference's (tests/golden/full_trajectory.npz)."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flow_sde_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "flow_sde.npz")
GOLD_FULL = os.path.join(ROOT, "tests", "golden", "full_trajectory.npz")
CASES = ["s10_i0", "s10_i1", "s10_i5", "s10_i9", "s4_i0", "s4_i2"]


def _case(name):
    npz = np.load(GOLD, allow_pickle=False)
    g = {k.split("/", 1)[1]: npz[k] for k in npz.files if k.startswith(name + "/")}
    steps, idx, nl = int(g["meta"][0]), int(g["meta"][1]), float(g["meta"][2])
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    B = t["v"].shape[0]
    return t, t["sigmas"][idx].repeat(B), t["sigmas"][idx + 1].repeat(B), float(t["sigmas"][1]), nl


# ----------------------------------------------------------------------------- 1. the restatement is the reference
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_golden(name):
    """float64: next / mean to 1e-6 absolute on O(1) values, std to float32 precision, the three log-probs to the bound of
    flow_sde_reference.log_prob_bound.  float32: the same lines are the reference's operation sequence -- mean, next and std bit for bit."""
    t, sig, sigp, smax, nl = _case(name)
    assert t["v"].shape == (2, 16, 8, 8) and nl == 0.7
    nxt, lp, mean, std, w = R.flow_sde_step(t["v"], t["x"], sig, sigp, smax, nl, eps=t["eps"])
    assert (nxt - t["next"]).abs().max() <= 1e-6 * max(1.0, t["next"].abs().max().item()) and (mean - t["mean"]).abs().max() <= 1e-6
    assert torch.allclose(std, t["std"].double(), rtol=1e-6, atol=0)
    bound = R.log_prob_bound(t["next"], t["mean"], w)
    print(name, "log_prob", lp.tolist(), "golden", t["log_prob"].tolist(), "bound", bound.tolist())
    assert ((lp - t["log_prob"]).abs() <= bound).all()
    for key, prev in (("log_prob_replay_f32", t["next"]), ("log_prob_replay_bf16", t["next"].to(torch.bfloat16))):
        _, lp_r, _, _, _ = R.flow_sde_step(t["v"], t["x"], sig, sigp, smax, nl, prev_sample=prev.float())
        assert ((lp_r - t[key]).abs() <= R.log_prob_bound(prev.float(), t["mean"], w)).all(), key
    nxt32, lp32, mean32, std32, _ = R.flow_sde_step(t["v"], t["x"], sig, sigp, smax, nl, eps=t["eps"], dtype=torch.float32)
    assert torch.equal(mean32, t["mean"]) and torch.equal(nxt32, t["next"]) and torch.equal(std32, t["std"])
    assert torch.equal(lp32, t["log_prob"])


def test_noise_level_zero_is_the_deterministic_step_and_its_log_prob_is_nan():
    t, sig, sigp, smax, nl = _case("s10_i1_nl0")
    assert nl == 0 and np.array_equal(t["next"].numpy(), t["mean"].numpy()) and "log_prob" not in t
    nxt, lp, mean, std, w = R.flow_sde_step(t["v"], t["x"], sig, sigp, smax, 0.0, eps=t["eps"], dtype=torch.float32)
    assert torch.equal(nxt, t["mean"]) and torch.equal(mean, t["mean"]) and (std == 0).all() and torch.isnan(lp).all()
    dt = (sigp - sig).view(-1, 1, 1, 1)
    assert torch.allclose(mean, t["x"] + t["v"] * dt, atol=1e-6)


def test_replaying_from_bf16_latents_moves_the_log_prob_on_the_last_step():
    """What DESIGN.md 3 notes: on the last step w is ~6e-3, and the bf16 rounding of the stored next latents alone moves the reference's own
    replayed log-prob by ~2e-2 to 4e-2; from float32 latents it comes back to float32 rounding."""
    t, *_ = _case("s10_i9")
    assert (t["log_prob_replay_f32"] - t["log_prob"]).abs().max() < 1e-5
    moved = (t["log_prob_replay_bf16"] - t["log_prob"]).abs()
    assert 1e-2 < moved.min() and moved.max() < 1e-1


def test_golden_holds_numbers_only():
    for path in (GOLD, GOLD_FULL):
        g = np.load(path, allow_pickle=False)
        for k in g.files:
            assert g[k].dtype.kind in "fi" or (k.startswith("signature/") and g[k].dtype.kind == "U"), (k, g[k].dtype)
        assert os.path.getsize(path) < 400 * 1024


# ----------------------------------------------------------------------------- 2. the closed-form gradients
@pytest.mark.parametrize("name", ["s10_i0", "s10_i5", "s10_i9", "s4_i2"])
def test_closed_form_gradients_match_autograd(name):
    """g_v of the policy term and of the KL term (what advgrpo_flow_sde_step_bwd(_kl) evaluate) against autograd on the restatement."""
    t, sig, sigp, smax, nl = _case(name)
    g = torch.Generator().manual_seed(3)
    B = t["v"].shape[0]
    glp = torch.randn(B, generator=g, dtype=torch.float64)
    mean_ref = t["mean"].double() + 0.05 * torch.randn(t["mean"].shape, generator=g, dtype=torch.float64)
    for kl_weight in (0.0, 0.37):
        v = t["v"].double().requires_grad_(True)
        _, lp, mean, _, _ = R.flow_sde_step(v, t["x"], sig, sigp, smax, nl, prev_sample=t["next"])
        ((lp * glp).sum() + kl_weight * ((mean - mean_ref) ** 2).mean()).backward()
        want = R.grad_v(t["v"], t["x"], sig, sigp, smax, nl, t["next"], glp, mean_ref if kl_weight else None, kl_weight)
        assert torch.allclose(v.grad, want, rtol=1e-9, atol=1e-12 * v.grad.abs().max().item())


# ----------------------------------------------------------------------------- 3. the surface
def _launcher():
    spec = importlib.util.spec_from_file_location("train_sd3_fast_launcher", os.path.join(ROOT, "scripts", "train_sd3_fast.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launcher_parses_sde_type():
    ap = _launcher().build_parser()
    base = ["--config", "config/grpo.py:pickscore_sd3_fast"]
    assert ap.parse_args(base).sde_type is None
    assert ap.parse_args(base + ["--sde-type", "sde"]).sde_type == "sde" and ap.parse_args(base + ["--sde-type", "cps"]).sde_type == "cps"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--sde-type", "ddim"])
    assert "--sde-type" in ap.format_help()


def test_sde_type_is_not_a_config_default():
    from adv_grpo_amd.config.experiments import get_config
    for name in ("pickscore_sd3_fast", "pickscore_cotrain_sd3_fast", "dino_cotrain_sd3_patch_fast"):
        assert get_config(name, gpu_number=1).sample.get("sde_type") is None


class _Done:
    def result(self):
        return {"avg": [0.0, 0.0]}, None, None


@pytest.mark.parametrize("branch", [False, True])
@pytest.mark.parametrize("setting", [None, "cps", "sde"])
def test_trainer_hands_the_setting_to_the_rollout(monkeypatch, setting, branch):
    """Trainer.sample_epoch on the CPU with both rollout names replaced by counters.  Without `sample.sde_type` the rollout gets the
    arguments it always got; with it, pipeline_with_logprob_random gets the keyword and the branching rollout (whose keyword list is the
    reference's) finds it on the pipeline object."""
    from adv_grpo_amd import trainer as T
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.pipeline import SD3Pipeline
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
    cfg.async_reward = False
    cfg.resolution = 64
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.num_batches_per_epoch = 2
    cfg.sample.groups_in_flight = 1
    if setting is not None:
        cfg.sample.sde_type = setting
    if branch:
        cfg.sample.branch_rollout = True
    calls = {"random": [], "new": []}

    def fake(which):
        def rollout(pipe, **kw):
            calls[which].append((kw, getattr(pipe, "sde_type", None)))
            pipe.last_random_timestep = 0
            Gn, Tn = kw["mini_num_image_per_prompt"], kw["train_num_steps"]
            lat = [torch.zeros(Gn, 16, 8, 8) for _ in range(Tn + 1)]
            return torch.zeros(Gn, 3, 64, 64), lat, [torch.zeros(Gn)] * Tn, [torch.zeros(Gn)] * Tn
        return rollout
    monkeypatch.setattr(T, "pipeline_with_logprob_random", fake("random"))
    monkeypatch.setattr(T, "pipeline_with_logprob_new", fake("new"))
    data = T.SyntheticData(n_prompts=10, n_tokens=3, ctx_dim=8, pooled_dim=4, resolution=64, device="cpu")
    tr = T.Trainer(cfg, SD3Pipeline(object(), object(), "cpu"), data, None, None)
    monkeypatch.setattr(tr, "_submit_score", lambda *a, **k: _Done())
    tr.profile_phases = False
    tr.sample_epoch()
    used, other = ("new", "random") if branch else ("random", "new")
    assert len(calls[used]) == 2 and not calls[other]
    for kw, on_pipe in calls[used]:
        if branch:
            assert "sde_type" not in kw and on_pipe == (setting or "cps")     # always assigned: a pipe never keeps an earlier Trainer's choice
        else:
            assert kw.get("sde_type") == setting and ("sde_type" in kw) == (setting is not None) and on_pipe is None


@pytest.mark.parametrize("setting", [None, "sde"])
def test_eval_loop_hands_the_setting_to_the_rollout(monkeypatch, setting):
    """Trainer.evaluate on the CPU with the rollout and the scorer replaced by stubs: the eval rollout gets `sde_type` exactly when the
    config has it."""
    from adv_grpo_amd import trainer as T
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.pipeline import SD3Pipeline
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
    cfg.async_reward = False
    cfg.resolution = 64
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.test_batch_size = 2
    if setting is not None:
        cfg.sample.sde_type = setting
    calls = []

    def rollout(pipe, **kw):
        calls.append(kw)
        n = kw["prompt_embeds"].shape[0]
        return torch.zeros(n, 3, 64, 64), [], [], []
    monkeypatch.setattr(T, "pipeline_with_logprob_random", rollout)
    monkeypatch.setattr(T.rewards, "multi_score", lambda device, spec: (lambda images, prompts, meta, **kw: ({"avg": [0.5] * len(images)}, {})))
    data = T.SyntheticData(n_prompts=10, n_tokens=3, ctx_dim=8, pooled_dim=4, resolution=64, device="cpu")
    tr = T.Trainer(cfg, SD3Pipeline(object(), object(), "cpu"), data, None, None)
    out = tr.evaluate(n_prompts=2, eval_reward_fn={"jpeg_compressibility": 1})
    assert out == {"eval_reward_avg": 0.5} and len(calls) == 1 and calls[0]["noise_level"] == 0
    assert calls[0].get("sde_type") == setting and ("sde_type" in calls[0]) == (setting is not None)


@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
def test_g_step_selects_the_matching_replay_and_backward_entries(monkeypatch, sde_type, beta):
    """g_step.micro_step on the CPU with the library, the fused step and the loss replaced by recorders: both replay forwards get
    `sde_type`, and exactly one backward entry of the matching family is called, with (noise_level, sigma_max pointer) for Flow-SDE and the
    sine coefficient for Flow-CPS in the tenth argument's place."""
    import math
    from adv_grpo_amd import _lib, g_step
    G, n = 2, 16 * 8 * 8
    sched = type("S", (), {"sigmas": torch.linspace(1, 0, 5)})()
    fwd, bwd = [], []

    class Lib:
        def advgrpo_sde_step_workspace_bytes(self, B, n):
            return 4 * B

        def __getattr__(self, name):
            return lambda *a: (bwd.append((name, a)), 0)[1]

    def step(scheduler, vu, vt, guidance, timestep, x, noise_level, **kw):
        fwd.append(kw)
        return None, None, torch.zeros(G), torch.zeros(G, 16, 8, 8) if kw.get("want_mean") else None, None

    class Model:
        def forward_train(self, x, t, e, p):
            return torch.zeros(2 * G, 16, 8, 8), "ctx"

        def forward_reference(self, x, t, e, p):
            return torch.zeros(2 * G, 16, 8, 8)

        def backward(self, ctx, grad):
            assert ctx == "ctx" and grad.shape == (2 * G, 16, 8, 8)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(g_step, "sde_step_cfg", step)
    monkeypatch.setattr(g_step.losses, "grpo_loss", lambda lp, old, adv, a, c: (torch.zeros(len(g_step.losses.INFO_KEYS)), torch.ones(G)))
    sample = {"latents": torch.zeros(G, 1, 16, 8, 8), "next_latents": torch.zeros(G, 1, 16, 8, 8), "timesteps": torch.zeros(G, 1)}
    g_step.micro_step(Model(), sched, sample, 0, None, None, torch.zeros(G), torch.zeros(G), guidance_scale=4.5, noise_level=0.7,
                      adv_clip_max=5, clip_range=1e-4, step_index=2, beta=beta, sde_type=sde_type)
    assert len(fwd) == (2 if beta > 0 else 1) and all(kw["sde_type"] == sde_type and kw["step_index"] == 2 for kw in fwd)
    assert len(bwd) == 1
    name, a = bwd[0]
    assert name == "advgrpo_" + ("flow_" if sde_type == "sde" else "") + "sde_step_bwd" + ("_kl" if beta > 0 else "")
    assert a[6] == sched.sigmas[2:3].data_ptr() and a[7] == sched.sigmas[3:4].data_ptr() and a[8] == 0
    if sde_type == "sde":
        assert a[9] == 0.7 and a[10] == sched.sigmas[1:2].data_ptr() and a[-3:-1] == (G, n)
        assert len(a) == len(_lib.SIGNATURES[name][1])
    else:
        assert a[9] == math.sin(0.7 * math.pi / 2) and len(a) == len(_lib.SIGNATURES[name][1])


def test_unknown_sde_type_is_refused_before_the_library_is_loaded(monkeypatch):
    from adv_grpo_amd import _lib
    from adv_grpo_amd.diffusers_patch import sd3_sde_with_logprob as S

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    x = torch.zeros(1, 16, 8, 8)
    with pytest.raises(ValueError, match="sde_type"):
        S.sde_step_cfg(None, x, None, 1.0, None, x, noise=x, step_index=0, sde_type="x")
    with pytest.raises(AssertionError, match="the library was loaded"):
        S.sde_step_cfg(None, x, None, 1.0, None, x, noise=x, step_index=0, sde_type="sde")
    assert S.sde_step_with_logprob_new is S.sde_step_with_logprob            # both names keep meaning Flow-CPS
    ours = inspect.signature(S.flow_sde_step_with_logprob)
    assert list(ours.parameters) == ["scheduler", "model_output", "timestep", "sample", "noise_level", "prev_sample", "generator", "noise"]
    assert ours.parameters["noise_level"].default == 0.7


def test_header_declares_the_flow_sde_entries_and_the_binding_mirrors_them():
    """Each Flow-SDE entry has the argument list of its Flow-CPS namesake with `float noise_level` in the place of `float sin_coeff`
    and `const float* sigma_max` after it."""
    from adv_grpo_amd import _lib
    text = open(os.path.join(ROOT, "include", "advgrpo.h")).read()

    def args(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/advgrpo.h does not declare {name}"
        return [" ".join(a.split()) for a in m.group(1).split(",")]
    for suffix in ("", "_branch", "_bwd", "_bwd_kl"):
        cps, flow = args("advgrpo_sde_step" + suffix), args("advgrpo_flow_sde_step" + suffix)
        k = cps.index("float sin_coeff")
        assert flow == cps[:k] + ["float noise_level", "const float* sigma_max"] + cps[k + 1:], suffix
        (res, flow_t), (_, cps_t) = _lib.SIGNATURES["advgrpo_flow_sde_step" + suffix], _lib.SIGNATURES["advgrpo_sde_step" + suffix]
        assert res is _lib.c_int and flow_t == cps_t[:k + 1] + [_lib.c_void_p] + cps_t[k + 1:] and cps_t[k] is _lib.c_float


def test_full_trajectory_signature_is_the_references_plus_noises_seed_and_sde_type():
    from adv_grpo_amd.diffusers_patch import sd3_pipeline_with_logprob as PFULL
    from adv_grpo_amd.diffusers_patch._rollout import NEED_EMBEDS
    g = np.load(GOLD_FULL)
    names, defaults = [str(v) for v in g["signature/names"]], [str(v) for v in g["signature/defaults"]]
    assert "noise_level" in names and "num_images_per_prompt" in names and "train_num_steps" not in names
    params = [p for p in inspect.signature(PFULL.pipeline_with_logprob).parameters.values() if p.name != "self"]
    assert [p.name for p in params] == names + ["noises", "seed", "sde_type"]
    assert [repr(p.default) for p in params] == defaults + ["None", "None", "'cps'"]
    with pytest.raises(ValueError) as e:
        PFULL.pipeline_with_logprob(object(), prompt="a photo of a cat")
    assert str(e.value) == NEED_EMBEDS
