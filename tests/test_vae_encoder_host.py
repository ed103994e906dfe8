"""CPU: the host side of the VAE encoder and the img2img entry points -- the float restatement (tests/vae_encoder_reference.py) against
itself in float64, its Downsample2D semantics, hub.load_vae_encoder on a synthetic checkpoint directory, get_sigmas and the start-index rule
against the golden made by the reference (tests/golden/img2img.npz), and the behaviour of a pipeline built without an encoder.  None of
these loads the HIP library."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch
from safetensors.torch import save_file

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_reference as ver  # noqa: E402

from adv_grpo_amd import hub, synthetic  # noqa: E402
from adv_grpo_amd.model_configs import VaeConfig  # noqa: E402

SMALL = VaeConfig(block_out_channels=(32, 32, 64, 64), norm_num_groups=8)
G = os.path.join(os.path.dirname(__file__), "golden")


def test_restatement_f32_against_f64():
    W = synthetic.vae_encoder_weights(SMALL, 3)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    m32 = ver.moments_from_images(W, SMALL, x)
    m64 = ver.moments_from_images({k: v.double() for k, v in W.items()}, SMALL, x.double())
    assert m32.shape == (2, 2 * SMALL.latent_channels, 8, 8) and m32.dtype == torch.float32 and m64.dtype == torch.float64
    e = (m32.double() - m64).abs().max().item() / m64.abs().max().item()
    print("f32 restatement vs f64: normalised max error", e)
    assert torch.isfinite(m64).all() and e < 1e-4          # f32 round-off through 11 resnets: ~1e-6 expected, 1e-4 is two orders of slack
    z = ver.sample_latents(m64, torch.zeros(2, SMALL.latent_channels, 8, 8, dtype=torch.float64), 1.5305)
    assert torch.equal(z, m64[:, :SMALL.latent_channels] * 1.5305)


def test_downsample2d_semantics():
    """output H/2 x W/2; the last row / column of the output see the zero pad, the first do not"""
    W = {"d.weight": torch.ones(1, 1, 3, 3), "d.bias": torch.zeros(1)}
    x = torch.ones(1, 1, 8, 6)
    y = ver.downsample2d(W, "d", x)
    assert y.shape == (1, 1, 4, 3)
    assert y[0, 0, 0, 0] == 9 and y[0, 0, 1, 1] == 9        # interior windows: nine ones, no padding on the top / left
    assert y[0, 0, -1, 0] == 6 and y[0, 0, 0, -1] == 6 and y[0, 0, -1, -1] == 4     # one zero row / column / both
    x = torch.zeros(1, 1, 8, 6); x[0, 0, 0, 0] = 1.0         # the first pixel is read by output (0, 0) only, at tap (0, 0)
    Wt = {"d.weight": torch.arange(9.0).view(1, 1, 3, 3) + 1, "d.bias": torch.zeros(1)}
    y = ver.downsample2d(Wt, "d", x)
    assert y[0, 0, 0, 0] == 1 and y.sum() == 1


def _write(d, sd, **over):
    os.makedirs(d, exist_ok=True)
    cfg = dict(_class_name="AutoencoderKL", act_fn="silu", latent_channels=16, block_out_channels=list(SMALL.block_out_channels), layers_per_block=2,
               norm_num_groups=SMALL.norm_num_groups, scaling_factor=1.5305, shift_factor=0.0609, use_post_quant_conv=False, use_quant_conv=False,
               mid_block_add_attention=True)
    cfg.update(over)
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    save_file({k: v.to(torch.float16).contiguous() for k, v in sd.items()}, os.path.join(d, "diffusion_pytorch_model.safetensors"))


def test_hub_load_vae_encoder(tmp_path):
    W = synthetic.vae_encoder_weights(SMALL, 4)
    full = dict(W)
    full.update(synthetic.vae_decoder_weights(SMALL, 5))       # a full AutoencoderKL carries its decoder too
    _write(tmp_path / "ok", full)
    sd, cfg = hub.load_vae_encoder(str(tmp_path / "ok"))
    assert cfg == SMALL and set(sd) == set(W)
    assert all(v.dtype == torch.float32 and torch.equal(v, W[k].half().float()) for k, v in sd.items())
    dsd, _ = hub.load_vae_decoder(str(tmp_path / "ok"))        # unchanged by the encoder half next to it
    assert all(k.startswith("decoder.") for k in dsd)
    # the key set is diffusers' AutoencoderKL encoder layout
    assert "encoder.down_blocks.0.downsamplers.0.conv.weight" in sd and "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sd
    assert sd["encoder.conv_out.weight"].shape == (32, 64, 3, 3) and "encoder.down_blocks.2.resnets.0.conv_shortcut.weight" in sd
    # legacy attention names as 1x1 convolutions
    leg = dict(full)
    a = "encoder.mid_block.attentions.0"
    for new, old in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
        leg[f"{a}.{old}.weight"] = leg.pop(f"{a}.{new}.weight")[:, :, None, None]
        leg[f"{a}.{old}.bias"] = leg.pop(f"{a}.{new}.bias")
    _write(tmp_path / "legacy", leg)
    lsd, _ = hub.load_vae_encoder(str(tmp_path / "legacy"))
    assert set(lsd) == set(W) and all(torch.equal(lsd[k], sd[k]) for k in sd)
    miss = dict(full); miss.pop("encoder.mid_block.resnets.1.norm2.bias")
    _write(tmp_path / "missing", miss)
    with pytest.raises(hub.HubError, match="encoder.mid_block.resnets.1.norm2.bias"):
        hub.load_vae_encoder(str(tmp_path / "missing"))
    bad = dict(full); bad["encoder.conv_in.weight"] = torch.zeros(32, 4, 3, 3)
    _write(tmp_path / "shape", bad)
    with pytest.raises(hub.HubError, match="encoder.conv_in.weight"):
        hub.load_vae_encoder(str(tmp_path / "shape"))
    _write(tmp_path / "quant", full, use_quant_conv=True)
    with pytest.raises(hub.HubError, match="use_quant_conv"):
        hub.load_vae_encoder(str(tmp_path / "quant"))


def test_get_sigmas_and_start_index_against_golden():
    from adv_grpo_amd.diffusers_patch import sd3_img2img_with_logprob as I2I
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    g = np.load(os.path.join(G, "img2img.npz"))
    steps = int(g["meta"][0])
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(steps)
    assert np.array_equal(sch.timesteps.numpy(), g["schedule_timesteps"]) and np.array_equal(sch.sigmas.numpy(), g["schedule_sigmas"])
    pick = sch.timesteps[torch.from_numpy(g["sigmas_pick"])]
    s32 = I2I.get_sigmas(sch, pick, "cpu", n_dim=4, dtype=torch.float32)
    s16 = I2I.get_sigmas(sch, pick, "cpu", n_dim=4, dtype=torch.bfloat16)
    assert s32.shape == (3, 1, 1, 1) and s16.dtype == torch.bfloat16
    assert np.array_equal(s32.numpy(), g["sigmas_f32"]) and np.array_equal(s16.float().numpy(), g["sigmas_bf16"])
    assert I2I.get_sigmas(sch, pick[:1], "cpu", n_dim=2).shape == (1, 1)
    # the start step: one randint(5, 10) on the global stream, the same draws the reference's interpreter made
    for seed, want in zip(g["draw_seeds"], g["draws"]):
        random.seed(int(seed))
        assert I2I.draw_target_idx() == int(want)
        after = random.random()
        random.seed(int(seed)); random.randint(5, 10)
        assert after == random.random()
    # the denoise loop starts at the LAST schedule entry >= t, i.e. at the drawn index itself on a strictly descending schedule
    ts = [float(v) for v in g["schedule_timesteps"]]
    for i in range(steps):
        assert I2I.start_index(ts, ts[i]) == i
    assert I2I.start_index(ts, 0.5 * (ts[3] + ts[4])) == 3
    with pytest.raises(ValueError):
        I2I.start_index(ts, ts[0] + 1)
    tgt = int(g["meta"][2])
    assert np.array_equal(g["timesteps"], np.broadcast_to(g["schedule_timesteps"][tgt:tgt + 2], g["timesteps"].shape))


def test_pipeline_without_encoder_still_works_and_new_entries_refuse():
    from adv_grpo_amd.diffusers_patch import sd3_img2img_with_logprob as I2I
    from adv_grpo_amd.pipeline import SD3Pipeline
    pipe = SD3Pipeline(object(), object(), "cpu")
    assert pipe.vae_encoder is None and pipe.do_classifier_free_guidance is False
    with pytest.raises(RuntimeError, match="without a VAE encoder"):
        I2I.image_to_latent(pipe, torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="without a VAE encoder"):
        I2I.flux_to_sd3_denoise_random(pipe, flux_images=torch.zeros(1, 3, 64, 64), prompt_embeds=torch.zeros(1, 4, 8))
    enc = object()
    assert SD3Pipeline(object(), object(), "cpu", vae_encoder=enc).vae_encoder is enc
    import inspect
    sig = inspect.signature(I2I.flux_to_sd3_denoise_random)
    assert [p for p in sig.parameters][:5] == ["self", "prompt", "prompt_2", "prompt_3", "flux_images"]
    assert sig.parameters["noise_level"].default == 0.7 and sig.parameters["num_inference_steps"].default == 20
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("target_idx", "encode_noise", "mix_noise", "noises", "seed"))


def test_encoder_constructor_refuses_what_it_does_not_run():
    from adv_grpo_amd.vae_encoder import AutoencoderKLEncoder
    W = synthetic.vae_encoder_weights(SMALL, 4)
    with pytest.raises(ValueError, match="bf16x3"):
        AutoencoderKLEncoder(W, SMALL, "cpu", mode="bf16")
    with pytest.raises(ValueError, match="encoder"):
        AutoencoderKLEncoder(synthetic.vae_decoder_weights(SMALL, 4), SMALL, "cpu")
    assert set(synthetic.shapes(synthetic.vae_encoder_weights, SMALL)) == set(W)
    a = synthetic.vae_encoder_weights(SMALL, 4, fp16_checkpoint=True)
    assert all(torch.equal(v.half().float(), v) for v in a.values())
