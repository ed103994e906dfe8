"""Plain-torch restatement of diffusers' AutoencoderKL encoder (SD3 / SD3.5 configuration) on the state-dict names of
``AutoencoderKL.state_dict()`` (``encoder.*``), in the dtype of its weights.  Helper for tests/test_vae_encoder_host.py and
tests/test_gpu_vae_encoder.py, not a test module.

PARITY UNPINNED: diffusers is not installed where this file was written, so it restates the architecture from its published definition
(Encoder -> DownEncoderBlock2D x 4 -> UNetMidBlock2D -> GroupNorm / SiLU / conv_out; ResnetBlock2D without time embedding;
Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + Conv2d(stride 2, padding 0); single-head Attention with residual connection) exactly as
oracle/vae.py restates the decoder.  scripts/verify_against_diffusers.py pins it against the real class where the wheel exists.
"""
import torch
import torch.nn.functional as F


def _gn(W, p, x, groups):
    return F.group_norm(x, groups, W[p + ".weight"], W[p + ".bias"], 1e-6)


def _conv(W, p, x, stride=1, padding=1):
    return F.conv2d(x, W[p + ".weight"], W[p + ".bias"], stride=stride, padding=padding)


def downsample2d(W, p, x):
    """Downsample2D(padding=0): zero-pad one column on the right and one row at the bottom, then a 3x3 convolution of stride 2."""
    return _conv(W, p, F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)


def resnet(W, p, x, groups):
    h = _conv(W, p + ".conv1", F.silu(_gn(W, p + ".norm1", x, groups)))
    h = _conv(W, p + ".conv2", F.silu(_gn(W, p + ".norm2", h, groups)))
    if p + ".conv_shortcut.weight" in W:
        x = _conv(W, p + ".conv_shortcut", x, padding=0)
    return x + h


def attention(W, p, x, groups):
    B, C, H, Wd = x.shape
    h = _gn(W, p + ".group_norm", x, groups).view(B, C, H * Wd).transpose(1, 2)
    q = F.linear(h, W[p + ".to_q.weight"], W[p + ".to_q.bias"])
    k = F.linear(h, W[p + ".to_k.weight"], W[p + ".to_k.bias"])
    v = F.linear(h, W[p + ".to_v.weight"], W[p + ".to_v.bias"])
    a = torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1)
    o = F.linear(a @ v, W[p + ".to_out.0.weight"], W[p + ".to_out.0.bias"])
    return x + o.transpose(1, 2).reshape(B, C, H, Wd)


def vae_encode_moments(W, cfg, x):
    """x [B,3,H,W] in [-1,1] -> moments [B, 2 * latent_channels, H/8, W/8] (mean | logvar), in x's dtype (= the weights')."""
    G = cfg.norm_num_groups
    n = len(cfg.block_out_channels)
    h = _conv(W, "encoder.conv_in", x)
    for i in range(n):
        for j in range(cfg.layers_per_block):
            h = resnet(W, f"encoder.down_blocks.{i}.resnets.{j}", h, G)
        if i < n - 1:
            h = downsample2d(W, f"encoder.down_blocks.{i}.downsamplers.0.conv", h)
    h = resnet(W, "encoder.mid_block.resnets.0", h, G)
    h = attention(W, "encoder.mid_block.attentions.0", h, G)
    h = resnet(W, "encoder.mid_block.resnets.1", h, G)
    return _conv(W, "encoder.conv_out", F.silu(_gn(W, "encoder.conv_norm_out", h, G)))


def moments_from_images(W, cfg, images):
    """images in [0,1] -> Normalize([0.5], [0.5]) -> moments."""
    return vae_encode_moments(W, cfg, (images - 0.5) / 0.5)


def sample_latents(moments, eps, scaling_factor):
    """DiagonalGaussianDistribution.sample() * scaling_factor (no shift, as the reference's image_to_latent)."""
    mean, logvar = moments.chunk(2, dim=1)
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    return (mean + std * eps) * scaling_factor


# ---- stand-ins of the img2img plumbing golden (tests/golden/make_golden_img2img.py and tests/test_gpu_vae_encoder.py use the SAME functions)
def structured_images_u8(B, size=512, seed=0):
    """Deterministic smooth uint8 images [B, size, size, 3] from a closed formula (integer arithmetic: the same bytes everywhere)."""
    y = torch.arange(size, dtype=torch.int64).view(1, size, 1, 1)
    x = torch.arange(size, dtype=torch.int64).view(1, 1, size, 1)
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1, 1)
    c = torch.arange(3, dtype=torch.int64).view(1, 1, 1, 3)
    v = (y * (3 + c + b) + x * (5 + 2 * c + seed) + (x * y) // (7 + b) + 40 * c + 17 * b) % 256
    return v.to(torch.uint8)


def standin_latent_sample(x):
    """Stand-in for ``vae.encode(x).latent_dist.sample()``: a fixed cheap function of the normalised image x [B,3,H,W] in [-1,1] -> f32
    [B,16,H/32,W/32] (draws nothing: the golden tests the plumbing around the encoder, not the encoder)."""
    p = F.avg_pool2d(x.float(), 32)
    c = torch.arange(16, device=x.device, dtype=torch.float32).view(1, 16, 1, 1)
    return p[:, torch.arange(16, device=x.device) % 3] * (0.5 + 0.1 * c) + 0.05 * c - 0.4
