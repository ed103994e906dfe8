"""CPU: the surface of the shared-prefix branching rollouts -- the two function signatures against the reference's (recorded in
tests/golden/branch_rollout.npz by make_golden_branch_rollout.py), the launcher flag, the Trainer's choice of rollout and the C entry's
declaration."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "branch_rollout.npz")


@pytest.mark.parametrize("fname,key", [("pipeline_with_logprob", "plain"), ("pipeline_with_logprob_new", "new")])
def test_signatures_are_the_references_plus_noises_and_seed(fname, key):
    from adv_grpo_amd.diffusers_patch import sd3_pipeline_with_logprob_fast as PF
    g = np.load(GOLD)
    names, defaults = [str(v) for v in g[f"signature/{key}/names"]], [str(v) for v in g[f"signature/{key}/defaults"]]
    assert len(names) == 29 and "random_timestep" in names and "mini_num_image_per_prompt" in names
    params = [p for p in inspect.signature(getattr(PF, fname)).parameters.values() if p.name != "self"]
    assert [p.name for p in params] == names + ["noises", "seed"]
    assert [repr(p.default) for p in params] == defaults + ["None", "None"]


def test_golden_holds_numbers_and_names_only():
    g = np.load(GOLD, allow_pickle=False)            # no pickled objects: every member is a plain array
    runs = sorted({k.split("/")[0] for k in g.files} - {"signature", "noise", "lat0"})
    assert runs == sorted([f"{f}_{d}_r{r}" for f in ("plain", "new") for d in ("fp32", "bf16") for r in (0, 2)] +
                          ["plain_bf16_rdraw", "new_bf16_rdraw"])
    for k in g.files:
        kind = g[k].dtype.kind
        assert kind in "fi" or (k.startswith("signature/") and kind == "U"), (k, g[k].dtype)
    assert os.path.getsize(GOLD) < 1 << 20
    steps, T, P, G, hw, drawn, process_index, r_arg = (int(v) for v in g["new_bf16_rdraw/meta"])
    assert (steps, T, P, G, hw, process_index, r_arg) == (6, 2, 2, 3, 64, 1, -1)
    import random
    assert drawn == random.Random(1).randint(0, steps // 2)
    for i in range(steps):                           # the reference's draw shapes: P rows before the branch step, P * G from it on
        assert g[f"noise/r{drawn}/{i}"].shape == ((P if i < drawn else P * G), 16, 8, 8)


def _launcher():
    spec = importlib.util.spec_from_file_location("train_sd3_fast_launcher", os.path.join(ROOT, "scripts", "train_sd3_fast.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launcher_parses_branch_rollout(monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "8"))     # (the launcher's setdefault is undone after the test)
    ap = _launcher().build_parser()
    assert ap.parse_args(["--config", "config/grpo.py:pickscore_sd3_fast"]).branch_rollout is False
    assert ap.parse_args(["--config", "config/grpo.py:pickscore_sd3_fast", "--branch-rollout"]).branch_rollout is True
    text = " ".join(ap.format_help().split())
    assert "--branch-rollout" in text and "share their initial noise" in text


def test_branch_rollout_is_not_a_config_default():
    from adv_grpo_amd.config.experiments import get_config
    for name in ("pickscore_sd3_fast", "pickscore_cotrain_sd3_fast", "dino_cotrain_sd3_patch_fast"):
        cfg = get_config(name, gpu_number=1)
        assert cfg.sample.get("branch_rollout") is None and cfg.sample.get("branch_rollout", False) is False


class _Done:
    def result(self):
        return {"avg": [0.0, 0.0]}, None, None


@pytest.mark.parametrize("setting,want", [(None, "random"), (False, "random"), (True, "new")])
def test_trainer_calls_the_branching_rollout_only_when_asked(monkeypatch, setting, want):
    """Trainer.sample_epoch on the CPU with both rollout names replaced by counters: a config without `sample.branch_rollout` (or with it
    false) goes through pipeline_with_logprob_random with the arguments it always passed; with it true the SAME arguments go to
    pipeline_with_logprob_new."""
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
        cfg.sample.branch_rollout = setting
    calls = {"random": [], "new": []}

    def fake(which):
        def rollout(pipe, **kw):
            calls[which].append(kw)
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
    tr.profile_phases = False                        # (the phase timers drain the calling thread's HIP stream)
    s = tr.sample_epoch()
    other = "new" if want == "random" else "random"
    assert len(calls[want]) == 2 and not calls[other]
    assert s["latents"].shape == (4, cfg.sample.train_num_steps, 16, 8, 8) and s["log_probs"].shape == (4, cfg.sample.train_num_steps)
    kw = calls[want][0]
    assert sorted(kw) == sorted(["prompt_embeds", "pooled_prompt_embeds", "negative_prompt_embeds", "negative_pooled_prompt_embeds",
                                 "num_inference_steps", "guidance_scale", "output_type", "height", "width", "noise_level",
                                 "mini_num_image_per_prompt", "train_num_steps", "process_index", "sample_num_steps", "random_timestep", "seed"])
    assert kw["output_type"] == "pt" and kw["mini_num_image_per_prompt"] == 2 and kw["seed"] == T.rollout_seed(cfg.seed, 0, 0)


def test_eval_loop_keeps_the_random_rollout():
    from adv_grpo_amd import trainer as T
    src = inspect.getsource(T.Trainer.evaluate)
    assert "pipeline_with_logprob_random(" in src and "pipeline_with_logprob_new" not in src and "rollout_fn" not in src


def test_header_declares_the_branch_entry_and_the_binding_mirrors_it():
    from adv_grpo_amd import _lib
    text = open(os.path.join(ROOT, "include", "advgrpo.h")).read()
    m = re.search(r"\bint\s+advgrpo_sde_step_branch\s*\(([^;]*)\)\s*;", text)
    assert m, "include/advgrpo.h does not declare advgrpo_sde_step_branch"
    args = [a.strip() for a in m.group(1).split(",")]
    plain = [a.strip() for a in re.search(r"\bint\s+advgrpo_sde_step\s*\(([^;]*)\)\s*;", text).group(1).split(",")]
    # the arguments of advgrpo_sde_step with (P, G) in the place of B
    assert args == plain[:-3] + ["int P", "int G"] + plain[-2:] and plain[-3] == "int B"
    res, argt = _lib.SIGNATURES["advgrpo_sde_step_branch"]
    _, plain_t = _lib.SIGNATURES["advgrpo_sde_step"]
    assert res is _lib.c_int and argt == plain_t[:-3] + [_lib.c_int, _lib.c_int] + plain_t[-2:]
    assert len(argt) == len(args)
