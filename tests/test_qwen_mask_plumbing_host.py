"""CPU: the optional prompt-mask pass-through of the Trainer, with the rollout replaced by a recorder (the pattern of
tests/test_flow_sde_host.py).  A data source with prompt_mask(idx) / neg_mask gets the CFG-batch mask -- negative rows first, like the
embeddings -- to the rollout through joint_attention_kwargs and into the samples; a data source without them changes nothing."""
import pytest
import torch


class _Done:
    def result(self):
        return {"avg": [0.0, 0.0]}, None, None


def _trainer(monkeypatch, data_cls, **cfg_over):
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
    for k, v in cfg_over.items():
        setattr(cfg.sample, k, v)
    calls = []

    def rollout(pipe, **kw):
        calls.append(kw)
        pipe.last_random_timestep = 0
        Gn, Tn = kw["mini_num_image_per_prompt"], kw["train_num_steps"]
        lat = [torch.zeros(Gn, 16, 8, 8) for _ in range(Tn + 1)]
        return torch.zeros(Gn, 3, 64, 64), lat, [torch.zeros(Gn)] * Tn, [torch.zeros(Gn)] * Tn
    monkeypatch.setattr(T, "pipeline_with_logprob_random", rollout)
    monkeypatch.setattr(T, "pipeline_with_logprob_new", lambda pipe, **kw: rollout(pipe, **kw))
    data = data_cls(n_prompts=10, n_tokens=7, ctx_dim=8, pooled_dim=4, resolution=64, device="cpu")
    tr = T.Trainer(cfg, SD3Pipeline(object(), object(), "cpu"), data, None, None)
    monkeypatch.setattr(tr, "_submit_score", lambda *a, **k: _Done())
    tr.profile_phases = False
    return tr, calls


def _masked_data():
    from adv_grpo_amd import trainer as T

    class MaskedData(T.SyntheticData):
        neg_mask = (torch.arange(7)[None] < 2).to(torch.int64)

        def prompt_mask(self, idx):
            return (torch.arange(7)[None] < 3 + idx % 5).to(torch.int64)
    return MaskedData


def test_a_data_source_with_masks_reaches_the_rollout_and_the_samples(monkeypatch):
    tr, calls = _trainer(monkeypatch, _masked_data())
    samples = tr.sample_epoch()
    assert len(calls) == 2
    G = 2
    for n, kw in enumerate(calls):
        m = kw["joint_attention_kwargs"]["encoder_hidden_states_mask"]
        assert m.shape == (2 * G, 7)
        assert m[:G].sum(1).tolist() == [2] * G                                  # the negative prompt's rows come first
        assert torch.equal(m[G:], samples["prompt_embeds_mask"][n * G:(n + 1) * G])
        assert m[G].sum().item() >= 3 and torch.equal(m[G], m[G + 1])
    assert samples["prompt_embeds_mask"].shape == (2 * G, 7)


def test_without_cfg_only_the_positive_rows_are_handed_over(monkeypatch):
    tr, calls = _trainer(monkeypatch, _masked_data(), guidance_scale=1.0)
    tr.sample_epoch()
    assert all(kw["joint_attention_kwargs"]["encoder_hidden_states_mask"].shape == (2, 7) for kw in calls)


def test_a_data_source_without_masks_changes_nothing(monkeypatch):
    from adv_grpo_amd import trainer as T
    tr, calls = _trainer(monkeypatch, T.SyntheticData)
    samples = tr.sample_epoch()
    assert len(calls) == 2 and all("joint_attention_kwargs" not in kw for kw in calls)
    assert "prompt_embeds_mask" not in samples


def test_a_mask_with_the_branching_rollout_is_refused(monkeypatch):
    tr, _ = _trainer(monkeypatch, _masked_data(), branch_rollout=True)
    with pytest.raises(NotImplementedError, match="branch_rollout"):
        tr.sample_epoch()
