"""CPU: the aesthetic and clipscore rewards' host side -- the CLIP ViT-L/14 config and loaders (hub.load_clip, hub.load_aesthetic_head),
registration, the unconfigured factories' errors, torchvision's resize / crop geometry and the launcher's flags and refusals."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_clip_dir(d, cfg, sd):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    v = dict(hidden_size=cfg.v_hidden, num_hidden_layers=cfg.v_layers, num_attention_heads=cfg.v_heads, intermediate_size=cfg.v_mlp,
             image_size=cfg.image_size, patch_size=cfg.patch, hidden_act="quick_gelu")
    t = dict(hidden_size=cfg.t_hidden, num_hidden_layers=cfg.t_layers, num_attention_heads=cfg.t_heads, intermediate_size=cfg.t_mlp,
             vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos, hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1)
    json.dump({"architectures": ["CLIPModel"], "projection_dim": 768, "vision_config": v, "text_config": t}, open(os.path.join(d, "config.json"), "w"))
    save_file({k: x.contiguous() for k, x in sd.items()}, os.path.join(d, "model.safetensors"))


def test_vit_l14_config():
    from adv_grpo_amd.model_configs import ClipConfig
    c = ClipConfig.vit_l14()
    assert (c.v_hidden, c.v_layers, c.v_heads, c.v_mlp, c.image_size, c.patch) == (1024, 24, 16, 4096, 224, 14)
    assert (c.t_hidden, c.t_layers, c.t_heads, c.t_mlp, c.proj, c.act, c.eos_token_id) == (768, 12, 12, 3072, 768, "quick_gelu", 2)
    assert ClipConfig().act == "gelu"                                   # PickScore's default is unchanged


def test_load_clip_reads_an_openai_layout_directory(tmp_path):
    from adv_grpo_amd import hub, synthetic
    from adv_grpo_amd.model_configs import ClipConfig
    cfg = ClipConfig(v_hidden=128, v_layers=1, v_heads=2, v_mlp=256, t_hidden=128, t_layers=1, t_heads=2, t_mlp=256, proj=768,
                     eos_token_id=2, act="quick_gelu")
    sd = synthetic.clip_weights(cfg, 3)
    d = str(tmp_path / "clip-l")
    _write_clip_dir(d, cfg, sd)
    got, gcfg = hub.load_clip(d)
    assert gcfg == cfg
    assert set(got) == set(sd) and torch.equal(got["visual_projection.weight"], sd["visual_projection.weight"])
    bad = dict(sd)
    bad["visual_projection.weight"] = torch.zeros(512, 128)              # a projection of another width
    _write_clip_dir(d, cfg, bad)
    with pytest.raises(hub.HubError, match="visual_projection"):
        hub.load_clip(d)


def test_load_aesthetic_head(tmp_path):
    from adv_grpo_amd import hub, synthetic
    sd = synthetic.aesthetic_head_weights(4)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        "layers.0.weight": (1024, 768), "layers.0.bias": (1024,), "layers.2.weight": (128, 1024), "layers.2.bias": (128,),
        "layers.4.weight": (64, 128), "layers.4.bias": (64,), "layers.6.weight": (16, 64), "layers.6.bias": (16,),
        "layers.7.weight": (1, 16), "layers.7.bias": (1,)}
    p = str(tmp_path / "head.pth")
    torch.save(sd, p)
    got = hub.load_aesthetic_head(p)
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    bad = dict(sd)
    bad["layers.6.weight"] = torch.zeros(16, 32)
    torch.save(bad, p)
    with pytest.raises(hub.HubError, match="layers.6.weight"):
        hub.load_aesthetic_head(p)
    torch.save({k: v for k, v in sd.items() if k != "layers.7.bias"}, p)
    with pytest.raises(hub.HubError, match="missing"):
        hub.load_aesthetic_head(p)


def test_rewards_are_registered_and_name_their_configure_call():
    from adv_grpo_amd import rewards
    for name, call in (("aesthetic", "configure_aesthetic"), ("clipscore", "configure_clip")):
        assert name in rewards.score_functions and name not in rewards._OUT_OF_SCOPE
    saved = dict(rewards._AESTHETIC), dict(rewards._CLIP)
    rewards._AESTHETIC.clear(), rewards._CLIP.clear()
    try:
        for name, call in (("aesthetic", "configure_aesthetic"), ("clipscore", "configure_clip")):
            with pytest.raises(RuntimeError, match=call):
                rewards.multi_score("cuda", {name: 1})
    finally:
        rewards._AESTHETIC.update(saved[0]), rewards._CLIP.update(saved[1])


def test_torchvision_resize_and_crop_geometry():
    from adv_grpo_amd.preprocess import tv_resize_geometry
    assert tv_resize_geometry(512, 512) == (224, 224, 0, 0)
    assert tv_resize_geometry(300, 500) == (224, 373, 0, 74)          # int(224 * 500 / 300) = 373; round(74.5) = 74 (half to even)
    assert tv_resize_geometry(500, 300) == (373, 224, 74, 0)
    assert tv_resize_geometry(300, 260) == (258, 224, 17, 0)
    assert tv_resize_geometry(150, 151) == (224, 225, 0, 0)            # round(0.5) = 0


def test_launcher_flags_and_refusals():
    script = os.path.join(ROOT, "scripts", "train_sd3_fast.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--clip-l-weights" in r.stdout and "--aesthetic-head" in r.stdout
    cfg = os.path.join(ROOT, "config", "grpo.py") + ":pickscore_sd3_fast"
    for args, needles in ((["--reward-fn", "aesthetic=1"], ("aesthetic", "--clip-l-weights", "--aesthetic-head")),
                          (["--reward-fn", "aesthetic=1", "--clip-l-weights", "x"], ("aesthetic", "--aesthetic-head")),
                          (["--reward-fn", "clipscore=1"], ("clipscore", "--clip-l-weights"))):
        r = subprocess.run([sys.executable, script, "--config", cfg] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(n in r.stderr for n in needles), (args, r.stderr[-2000:])
        assert "Traceback" not in r.stderr
