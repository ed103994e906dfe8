"""Float reference of the SigLIP vision tower and its attention-pooling head, in plain torch (test helper, not a test module).

Follows transformers' SiglipVisionModel (SiglipVisionEmbeddings -> SiglipEncoder -> post_layernorm -> SiglipMultiheadAttentionPoolingHead)
on a state dict keyed like adv_grpo_amd.synthetic.siglip_weights (``vision_model.`` prefix), in the dtype of the weights given (f32 for the
parity tests).  tests/test_siglip_host.py pins it against transformers; the GPU tests compare the kernels against it.
"""
import math

import torch
import torch.nn.functional as F


def _ln(sd, p, x, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(sd, p, x):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def _mha(q, k, v, heads):
    """q [B,Sq,D], k/v [B,S,D] -> softmax(q k^T / sqrt(hd)) v per head, [B,Sq,D]."""
    B, Sq, D = q.shape
    hd = D // heads
    sp = lambda t: t.reshape(B, t.shape[1], heads, hd).transpose(1, 2)
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(hd), dim=-1)
    return (a @ sp(v)).transpose(1, 2).reshape(B, Sq, D)


def _mlp(sd, p, x):
    return _lin(sd, p + ".fc2", F.gelu(_lin(sd, p + ".fc1", x), approximate="tanh"))


def last_hidden_state(sd, cfg, pixel_values):
    """pixel_values [B,3,S,S] (normalised) -> post_layernorm(encoder(embeddings)) [B, P, D]."""
    v = "vision_model"
    x = F.conv2d(pixel_values, sd[f"{v}.embeddings.patch_embedding.weight"], sd[f"{v}.embeddings.patch_embedding.bias"], stride=cfg.patch)
    x = x.flatten(2).transpose(1, 2) + sd[f"{v}.embeddings.position_embedding.weight"][None]
    for i in range(cfg.layers):
        p = f"{v}.encoder.layers.{i}"
        h = _ln(sd, f"{p}.layer_norm1", x, cfg.eps)
        a = f"{p}.self_attn"
        o = _mha(_lin(sd, f"{a}.q_proj", h), _lin(sd, f"{a}.k_proj", h), _lin(sd, f"{a}.v_proj", h), cfg.heads)
        x = x + _lin(sd, f"{a}.out_proj", o)
        x = x + _mlp(sd, f"{p}.mlp", _ln(sd, f"{p}.layer_norm2", x, cfg.eps))
    return _ln(sd, f"{v}.post_layernorm", x, cfg.eps)


def pool(sd, cfg, x):
    """SiglipMultiheadAttentionPoolingHead: [B, P, D] -> pooler_output [B, D] (no residual around the attention)."""
    h, D = "vision_model.head", x.shape[-1]
    w, b = sd[f"{h}.attention.in_proj_weight"], sd[f"{h}.attention.in_proj_bias"]
    q = F.linear(sd[f"{h}.probe"].expand(x.shape[0], 1, D), w[:D], b[:D])
    o = _mha(q, F.linear(x, w[D:2 * D], b[D:2 * D]), F.linear(x, w[2 * D:], b[2 * D:]), cfg.heads)
    o = _lin(sd, f"{h}.attention.out_proj", o)
    o = o + _mlp(sd, f"{h}.mlp", _ln(sd, f"{h}.layernorm", o, cfg.eps))
    return o[:, 0]


def pooler_output(sd, cfg, pixel_values):
    return pool(sd, cfg, last_hidden_state(sd, cfg, pixel_values))


def preprocess(images, size=384):
    """The reference's _preprocess (adv_grpo/rewards.py:87-115) for a device tensor [B,3,H,W]: /255 when max > 1, bicubic resize in the
    input's dtype, (x - 0.5) / 0.5 against f32 tensors, bf16."""
    if images.max() > 1.0:
        images = images / 255.0
    images = F.interpolate(images, size=(size, size), mode="bicubic", align_corners=False)
    mean = torch.tensor([0.5, 0.5, 0.5], device=images.device)[None, :, None, None]
    std = torch.tensor([0.5, 0.5, 0.5], device=images.device)[None, :, None, None]
    return ((images - mean) / std).to(torch.bfloat16)


def patch_rows(pixel_values, patch=14):
    """[B,3,S,S] -> the im2col rows [B*P, 640] of the patch conv (588 real columns + zeros); pixels past (S // 14) * 14 are not read."""
    B, g = pixel_values.shape[0], pixel_values.shape[-1] // patch
    x = pixel_values[:, :, :g * patch, :g * patch].reshape(B, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, -1)
    return F.pad(x, (0, 640 - x.shape[1]))


def structured_images(n, size, seed):
    """[n,3,size,size] f32 in [0,1]: solid colours, two-colour gradients, checkerboards and sine gratings (cycling), plus faint noise.
    Noise images average out over SigLIP's 729 patches and the pooled embeddings of the synthetic towers then barely depend on the
    image (cosines within ~0.01 of each other); these give cosines spread over most of [0, 1], so a scorer that ignores or mis-scales
    its input is far outside the tolerances."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.linspace(0, 1, size), torch.linspace(0, 1, size), indexing="ij")
    out = []
    for i in range(n):
        c = torch.rand(3, 1, 1, generator=g)
        kind = i % 4
        if kind == 0:
            im = c.expand(3, size, size)
        elif kind == 1:
            im = c * xs + (1 - c) * ys
        elif kind == 2:
            p = int(torch.randint(4, 24, (1,), generator=g))
            idx = torch.arange(size)
            im = c * ((idx[:, None] // p + idx[None] // p) % 2).float()
        else:
            im = 0.5 + 0.5 * torch.sin(c * 20 * xs + (1 - c) * 13 * ys)
        out.append(im + 0.05 * torch.rand(3, size, size, generator=g))
    return torch.stack(out).clamp(0, 1).float()
