"""CPU: the siglip_image_similarity reward's host side -- the synthetic key layout against transformers' SiglipVisionModel, the float
reference of tests/siglip_reference.py against transformers' pooler_output, hub.load_siglip, the registry and the launcher refusal."""
import json
import os
import subprocess
import sys

import pytest
import torch

import siglip_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_config(cfg):
    from transformers import SiglipVisionConfig
    return SiglipVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers,
                              num_attention_heads=cfg.heads, image_size=cfg.image_size, patch_size=cfg.patch, layer_norm_eps=cfg.eps,
                              hidden_act="gelu_pytorch_tanh", attn_implementation="eager")


def _prefixed(keys):
    """transformers 5 keeps SiglipVisionModel's parameters without the ``vision_model.`` prefix its checkpoints carry."""
    return {(k if k.startswith("vision_model.") else "vision_model." + k): v for k, v in keys.items()}


def test_synthetic_key_layout_is_transformers_siglip_so400m():
    from transformers import SiglipVisionModel
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    cfg = SiglipVisionConfig()
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.mlp, cfg.image_size, cfg.patch, cfg.head_dim, cfg.tokens) == \
        (1152, 27, 16, 4304, 384, 14, 72, 729)
    with torch.device("meta"):
        m = SiglipVisionModel(_hf_config(cfg))
    want = _prefixed({k: tuple(v.shape) for k, v in m.state_dict().items()})
    assert synthetic.shapes(synthetic.siglip_weights, cfg) == want


def test_float_reference_matches_transformers_pooler_output():
    """Head dim 72 (2 heads x 72), 2 layers, mlp 200, 56 px -> 16 tokens; all f32."""
    from transformers import SiglipVisionModel
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    cfg = SiglipVisionConfig(hidden=144, layers=2, heads=2, mlp=200, image_size=56)
    sd = synthetic.siglip_weights(cfg, 5)
    m = SiglipVisionModel(_hf_config(cfg)).eval()
    own = m.state_dict()
    m.load_state_dict({k: sd[k] if k in sd else sd["vision_model." + k] for k in own})
    px = torch.randn(3, 3, 56, 56, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        want = m(pixel_values=px).pooler_output
        got = siglip_reference.pooler_output(sd, cfg, px)
    # both are f32 evaluations of the same expression; only summation order differs (a few f32 ulp per op, O(1) values)
    assert got.shape == want.shape == (3, 144)
    assert (got - want).abs().max().item() < 1e-4


def _snapshot(d, cfg, sd, full_model=True, **vision_over):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    v = {"hidden_size": cfg.hidden, "intermediate_size": cfg.mlp, "num_hidden_layers": cfg.layers, "num_attention_heads": cfg.heads,
         "image_size": cfg.image_size, "patch_size": cfg.patch, "model_type": "siglip_vision_model"}
    v.update(vision_over)
    if full_model:
        conf = {"architectures": ["SiglipModel"], "model_type": "siglip", "vision_config": v,
                "text_config": {"hidden_size": 32, "model_type": "siglip_text_model"}}
        sd = dict(sd, **{"text_model.embeddings.token_embedding.weight": torch.zeros(8, 32), "logit_scale": torch.zeros(1),
                         "logit_bias": torch.zeros(1)})
    else:
        conf = dict(v, architectures=["SiglipVisionModel"])
        sd = {k[len("vision_model."):]: t for k, t in sd.items()}            # as transformers 5 saves a SiglipVisionModel
    json.dump(conf, open(os.path.join(d, "config.json"), "w"))
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(d, "model.safetensors"))
    return d


def test_hub_loads_siglip_snapshots_and_refuses_what_is_not_built(tmp_path):
    from adv_grpo_amd import hub, synthetic
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    cfg = SiglipVisionConfig(hidden=144, layers=2, heads=2, mlp=200, image_size=56)
    sd = synthetic.siglip_weights(cfg, 9)
    for full in (True, False):
        got, gcfg = hub.load_siglip(_snapshot(str(tmp_path / f"ok{full}"), cfg, sd, full_model=full))
        assert gcfg == cfg and set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)

    bad = dict(sd)
    bad["vision_model.post_layernorm.weight"] = torch.zeros(7)
    with pytest.raises(hub.HubError, match="another shape"):
        hub.load_siglip(_snapshot(str(tmp_path / "shape"), cfg, bad))
    missing = {k: v for k, v in sd.items() if k != "vision_model.head.probe"}
    with pytest.raises(hub.HubError, match="missing.*vision_model.head.probe"):
        hub.load_siglip(_snapshot(str(tmp_path / "missing"), cfg, missing))
    with pytest.raises(hub.HubError, match="vision_use_head"):
        hub.load_siglip(_snapshot(str(tmp_path / "nohead"), cfg, sd, vision_use_head=False))
    with pytest.raises(hub.HubError, match="hidden_act = 'gelu'"):
        hub.load_siglip(_snapshot(str(tmp_path / "act"), cfg, sd, hidden_act="gelu"))
    with pytest.raises(hub.HubError, match="patch_size = 16"):
        hub.load_siglip(_snapshot(str(tmp_path / "patch"), cfg, sd, patch_size=16))
    with pytest.raises(hub.HubError, match="head dim 144/1"):
        hub.load_siglip(_snapshot(str(tmp_path / "hd"), cfg, sd, num_attention_heads=1))


def test_siglip_image_similarity_is_registered():
    from adv_grpo_amd import rewards
    assert "siglip_image_similarity" in rewards.score_functions
    assert "siglip_image_similarity" not in rewards._OUT_OF_SCOPE
    fn = rewards.multi_score("cpu", {"siglip_image_similarity": 1.0})        # building the scorer touches no device
    rewards.configure_siglip(None)
    with pytest.raises(RuntimeError, match="siglip_image_similarity.*configure_siglip"):
        fn(torch.zeros(1, 3, 8, 8), None, None, ref_images=torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="siglip_image_similarity.*ref_images"):
        fn(torch.zeros(1, 3, 8, 8), None, None)


def test_launcher_refuses_siglip_image_similarity_for_training():
    script = os.path.join(ROOT, "scripts", "train_sd3_fast.py")
    cfg = os.path.join(ROOT, "config", "grpo.py") + ":pickscore_sd3_fast"
    r = subprocess.run([sys.executable, script, "--config", cfg, "--reward-fn", "siglip_image_similarity=1"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "siglip_image_similarity" in r.stderr and "reference images" in r.stderr, r.stderr[-2000:]
