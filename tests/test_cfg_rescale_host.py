"""CPU: the norm-rescaled true CFG in the stochastic GRPO steps -- the closed-form backward of tests/cfg_rescale_reference.py against
float64 autograd of the restatement, and the surface: the C symbols and their declarations, the launcher flag, the option on
``sde_step_cfg``, the rollouts and the Trainer."""
import importlib.util
import os
import re

import pytest
import torch

import cfg_rescale_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("advgrpo_sde_step_rescaled_workspace_bytes", "advgrpo_sde_step_rescaled", "advgrpo_flow_sde_step_rescaled",
           "advgrpo_sde_step_rescaled_bwd", "advgrpo_flow_sde_step_rescaled_bwd")


# ---------------------------------------------------------------------------------------------------------------- 1. the closed form
@pytest.mark.parametrize("with_kl", [False, True], ids=["policy", "kl"])
@pytest.mark.parametrize("sde_type", ["cps", "sde"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_analytic_backward_is_float64_autograd_of_the_restatement(shape, sde_type, with_kl):
    """dL/dc = r (g - (c.g) / b^2 c), dL/dp = s dL/dc + (c.g) / (a b) p, dL/dn = (1 - s) dL/dc against autograd: 1e-12 relative."""
    c = R.bwd_case(shape, torch.float32, sde_type, with_kl)
    args = (sde_type, c["v_neg"], c["v_pos"], c["x"], c["sig"], c["sigp"], c["prev"], c["glp"], c["mean_ref"], c["kl_weight"])
    ref_n, ref_p, _ = R.grad_autograd(*args)
    got_n, got_p = R.grad_analytic(*args)
    assert ref_n.abs().max().item() > 0 and ref_p.abs().max().item() > 0
    for got, ref in ((got_n, ref_n), (got_p, ref_p)):
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_gradient_is_orthogonal_to_the_combined_prediction_when_the_conditional_norm_is_held():
    """v = c ||p|| / ||c|| does not change along c, so dL/dc is orthogonal to c in every token: the structure the second reduction buys."""
    c = R.bwd_case((2, 16, 6, 10), torch.float32, "cps", False)
    n_, p_ = c["v_neg"].double(), c["v_pos"].double()
    g_n, _ = R.grad_analytic("cps", n_, p_, c["x"], c["sig"], c["sigp"], c["prev"], c["glp"])
    dc = R.Q.pack(g_n / (1 - R.SCALE))
    comb = R.Q.pack(n_ + R.SCALE * (p_ - n_))
    assert ((dc * comb).sum(-1).abs() <= 1e-12 * dc.norm(dim=-1) * comb.norm(dim=-1)).all()


def test_emulation_follows_the_tolerance_rule_the_gpu_test_uses():
    """The float32 emulation of the kernel's operation order against float64 autograd, over the GPU test's case list: inside the project
    bound in f32, and in bf16 of the size that makes the GPU bound four times the measured error (LABNOTES has the figures)."""
    worst, bound = R.measure_emulation()
    print("emulation error (share of the gradient scale):", worst, "GPU bound:", bound)
    for dt in worst:
        assert 0 < worst[dt] and bound[dt] >= R.PROJECT_BOUND[dt] and bound[dt] in (R.PROJECT_BOUND[dt], 4 * worst[dt])
    assert worst[torch.float32] <= R.PROJECT_BOUND[torch.float32] / 4           # f32: the project's own 1e-5 holds


# ---------------------------------------------------------------------------------------------------------------- 2. the surface
def test_library_exports_and_header_declares_the_five_entries():
    from adv_grpo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "advgrpo.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
    # the shape arguments take the place of (B, n): five ints where the namesake has (int, int64)
    for new, old in (("advgrpo_sde_step_rescaled", "advgrpo_sde_step"), ("advgrpo_flow_sde_step_rescaled", "advgrpo_flow_sde_step"),
                     ("advgrpo_sde_step_rescaled_bwd", "advgrpo_sde_step_bwd_kl"), ("advgrpo_flow_sde_step_rescaled_bwd", "advgrpo_flow_sde_step_bwd_kl")):
        a, b = _lib.SIGNATURES[new][1], _lib.SIGNATURES[old][1]
        assert a[:-6] == b[:-3] and a[-6:-1] == [_lib.c_int] * 5 and a[-1] == b[-1] == _lib._P, new
    assert lib.advgrpo_sde_step_rescaled_workspace_bytes(3, 16, 64, 64, 2) == 3 * 16 * 4      # 1024 tokens: 16 blocks of 64 per sample


def _launcher():
    spec = importlib.util.spec_from_file_location("train_sd3_fast_launcher_cfg_rescale", os.path.join(ROOT, "scripts", "train_sd3_fast.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launcher_flag_reaches_the_config():
    from adv_grpo_amd.config.experiments import get_config
    tool = _launcher()
    ap = tool.build_parser()
    base = ["--config", "config/grpo.py:pickscore_sd3_fast"]
    assert ap.parse_args(base).cfg_rescale is False and "--cfg-rescale" in ap.format_help()
    for name in ("pickscore_sd3_fast", "pickscore_cotrain_sd3_fast", "dino_cotrain_sd3_patch_fast"):
        assert get_config(name, gpu_number=1).sample.get("cfg_rescale") is None          # not a config default
    cfg = tool.apply_sample_flags(get_config("pickscore_sd3_fast", gpu_number=1), ap.parse_args(base))
    assert cfg.sample.get("cfg_rescale") is None and cfg.sample.get("sde_type") is None
    cfg = tool.apply_sample_flags(get_config("pickscore_sd3_fast", gpu_number=1), ap.parse_args(base + ["--cfg-rescale", "--sde-type", "sde"]))
    assert cfg.sample.cfg_rescale is True and cfg.sample.sde_type == "sde"


def test_fan_out_step_refuses_the_rescaled_combine():
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    t = torch.zeros(2, 16, 4, 4)
    with pytest.raises(ValueError, match="copies"):
        sde_step_cfg(None, t, t, 4.0, None, t, 0.7, seed=1, step_index=0, sigmas=R.SIGMAS, copies=3, cfg_rescale=True)
    with pytest.raises(ValueError, match=r"\[B, 16, H, W\]"):
        sde_step_cfg(None, t[:, :8], t[:, :8], 4.0, None, t[:, :8], 0.7, seed=1, step_index=0, sigmas=R.SIGMAS, cfg_rescale=True)


def test_branching_rollouts_refuse_the_option_on_the_pipeline_object():
    from adv_grpo_amd.diffusers_patch import sd3_pipeline_with_logprob_fast as PF

    class Pipe:
        cfg_rescale = True
    pe = torch.zeros(1, 3, 8)
    for fn in (PF.pipeline_with_logprob, PF.pipeline_with_logprob_new):
        with pytest.raises(NotImplementedError, match="cfg_rescale"):
            fn(Pipe(), prompt_embeds=pe, pooled_prompt_embeds=torch.zeros(1, 4))


def _config(**sample):
    from adv_grpo_amd.config.experiments import get_config
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
    cfg.async_reward = False
    cfg.resolution = 64
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.num_batches_per_epoch = 2
    cfg.sample.groups_in_flight = 1
    cfg.sample.test_batch_size = 2
    for k, v in sample.items():
        setattr(cfg.sample, k, v)
    return cfg


def _trainer(cfg):
    from adv_grpo_amd import trainer as T
    from adv_grpo_amd.pipeline import SD3Pipeline
    data = T.SyntheticData(n_prompts=10, n_tokens=3, ctx_dim=8, pooled_dim=4, resolution=64, device="cpu")
    return T.Trainer(cfg, SD3Pipeline(object(), object(), "cpu"), data, None, None)


def test_trainer_refuses_the_option_with_the_branching_rollout():
    with pytest.raises(NotImplementedError, match="cfg_rescale"):
        _trainer(_config(cfg_rescale=True, branch_rollout=True))
    assert _trainer(_config(branch_rollout=True)).cfg_rescale is False
    assert _trainer(_config(cfg_rescale=True)).cfg_rescale is True
    assert _trainer(_config(cfg_rescale=True, guidance_scale=1.0)).cfg_rescale is False     # nothing to rescale without CFG: a no-op


class _Done:
    def result(self):
        return {"avg": [0.0, 0.0]}, None, None


@pytest.mark.parametrize("setting", [None, False, True])
def test_trainer_hands_the_option_to_rollout_and_evaluation(monkeypatch, setting):
    """Trainer.sample_epoch and Trainer.evaluate on the CPU with the rollout replaced by a recorder: the keyword appears exactly when the option is on,
    so a config without the key calls what it always called."""
    from adv_grpo_amd import trainer as T
    tr = _trainer(_config(**({} if setting is None else {"cfg_rescale": setting})))
    calls = {"rollout": []}

    def rollout(pipe, **kw):
        calls["rollout"].append(kw)
        pipe.last_random_timestep = 0
        Gn, Tn = kw["mini_num_image_per_prompt"], kw.get("train_num_steps", 1)
        lat = [torch.zeros(Gn, 16, 8, 8) for _ in range(Tn + 1)]
        return torch.zeros(kw["prompt_embeds"].shape[0] * Gn, 3, 64, 64), lat, [torch.zeros(Gn)] * Tn, [torch.zeros(Gn)] * Tn
    monkeypatch.setattr(T, "pipeline_with_logprob_random", rollout)
    monkeypatch.setattr(tr, "_submit_score", lambda *a, **k: _Done())
    tr.profile_phases = False
    tr.sample_epoch()
    monkeypatch.setattr(T.rewards, "multi_score", lambda device, spec: (lambda images, prompts, meta, **kw: ({"avg": [0.5] * len(images)}, {})))
    tr.evaluate(n_prompts=2, eval_reward_fn={"jpeg_compressibility": 1})
    assert len(calls["rollout"]) == 3
    for kw in calls["rollout"]:
        assert ("cfg_rescale" in kw) == (setting is True) and kw.get("cfg_rescale", False) == bool(setting)
