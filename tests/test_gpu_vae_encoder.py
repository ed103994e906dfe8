"""GPU: the SD3 VAE encoder -- strided split-bf16 convolution, image head, latent tail, the whole chain against the float64 restatement
(tests/vae_encoder_reference.py), the C entry against the launch-by-launch path, and the img2img rollout against the golden produced by the
REFERENCE's flux_to_sd3_denoise_random (tests/golden/img2img.npz)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_reference as ver  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _encoder(seed=99, fp16_checkpoint=False):
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import VaeConfig
    from adv_grpo_amd.vae_encoder import AutoencoderKLEncoder
    cfg = VaeConfig()
    W = synthetic.vae_encoder_weights(cfg, seed, fp16_checkpoint=fp16_checkpoint)
    return AutoencoderKLEncoder(W, cfg, "cuda"), W, cfg


def _images(B, H, W, seed):
    """smooth structure + noise in [0,1] (an encoder input with both flat regions and edges)"""
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(B, 3, H // 16, W // 16, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    return (0.8 * base + 0.2 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)


def test_strided_convolution_vs_float64():
    """3x3, stride 2, (0, 1, 0, 1) zero padding folded into the tap addressing, against F.conv2d(F.pad(x, (0,1,0,1)), w, b, stride=2) in f64 at
    the encoder's three channel counts; a ragged tile (H/2 W/2 = 35 pixels per image, 105 < 192), W/2 = 1, and a batch whose 192-pixel tiles
    straddle images (3 x 130 pixels).  Bound: that of advgrpo_conv3x3_nhwc_x3 in tests/test_gpu_vae.py (same arithmetic, same input scale)."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    for (B, H, W, C) in [(1, 16, 24, 128), (3, 10, 14, 128), (2, 14, 2, 256), (3, 20, 26, 256), (2, 12, 12, 512), (1, 2, 2, 512)]:
        x = torch.randn(B, H, W, C, device="cuda", generator=g)
        wt = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (3 * C ** 0.5)
        bias = torch.randn(C, device="cuda", generator=g)
        w3 = ops.split_x3(wt.permute(0, 2, 3, 1).contiguous(), order=1).reshape(C, -1)
        y = ops.conv3x3_s2_x3(ops.split_x3(x), w3, bias=bias)
        ref = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (0, 1, 0, 1)), wt.double(), bias.double(), stride=2).permute(0, 2, 3, 1)
        assert y.shape == ref.shape == (B, H // 2, W // 2, C)
        err = (y.double() - ref).abs().max().item()
        print("conv s2 x3", (B, H, W, C), "max err", err, "of", ref.abs().max().item())
        assert err < 1e-4 * ref.abs().max().item()
        x2 = torch.full((B, H, W, 3 * C), float("nan"), device="cuda", dtype=torch.bfloat16)     # the middle third is never read
        s2 = ops.split_x3(x, 2)
        x2[..., :C] = s2[..., :C]
        x2[..., 2 * C:] = s2[..., 2 * C:]
        assert torch.equal(ops.conv3x3_s2_x3(x2, w3, bias=bias), y)


def test_image_head_rows():
    """(x - 0.5) / 0.5 as split rows: hi + lo reproduces the f32 value to 2^-16 relative, padded channels are zero, uint8 NHWC and bf16 / f32
    NCHW inputs agree with torch."""
    from adv_grpo_amd import ops
    img = _images(2, 32, 64, 3).cuda()
    for x, want in ((img, (img - 0.5) / 0.5), (img.bfloat16(), (img.bfloat16().float() - 0.5) / 0.5)):
        r = ops.image_to_nhwc_x3(x, 64).float()
        got = r[..., :3] + r[..., 128:131]
        w = want.permute(0, 2, 3, 1)
        assert ((got - w).abs() <= 2.0 ** -15 * w.abs() + 1e-30).all()
        assert (r[..., 3:64] == 0).all() and (r[..., 131:] == 0).all()
    u8 = (img * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    r = ops.image_to_nhwc_x3(u8, 64).float()
    w = (u8.float() / 255.0 - 0.5) / 0.5
    assert ((r[..., :3] + r[..., 128:131] - w).abs() <= 2.0 ** -15 * w.abs() + 1e-30).all()


def _ulp32(a, b):
    ai = a.contiguous().view(torch.int32).long()
    bi = b.contiguous().view(torch.int32).long()
    ai = torch.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = torch.where(bi < 0, -(bi & 0x7fffffff), bi)
    return (ai - bi).abs()


def _bf16_ulps(a, b):
    ai = a.contiguous().view(torch.int16).long()
    bi = b.contiguous().view(torch.int16).long()
    ai = torch.where(ai < 0, -(ai & 0x7fff), ai)
    bi = torch.where(bi < 0, -(bi & 0x7fff), bi)
    return (ai - bi).abs()


def test_latent_tail_vs_torch_rounding_points():
    """Same moments, eps and noise: f32 z * scaling within 2 ulp of torch (device expf against torch's exp, the only inexact step); the bf16
    latents and the bf16 forward noising within one bf16 ulp (a 2-ulp f32 difference can straddle a bf16 rounding boundary); the share of
    elements that differ at all is printed, not bounded.  mode "mean" is the mean times scaling exactly."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(9)
    B, C, h, w = 3, 16, 8, 12
    mom = torch.randn(B, h, w, 2 * C, device="cuda", generator=g) * 2
    mom[0, 0, 0, C:] = 100.0                # clamps
    mom[0, 0, 1, C:] = -100.0
    eps = torch.randn(B, C, h, w, device="cuda", generator=g)
    noise = torch.randn(B, C, h, w, device="cuda", generator=g).bfloat16()
    sf = 1.5305
    m = mom.permute(0, 3, 1, 2)
    mean, logvar = m[:, :C], m[:, C:].clamp(-30.0, 20.0)
    want = (mean + torch.exp(0.5 * logvar) * eps) * sf
    z32 = ops.vae_latent_tail(mom, sf, "eps", eps=eps, out_dtype=torch.float32)
    ulp = _ulp32(z32, want.contiguous())
    print("latent tail f32: max ulp", ulp.max().item(), "share differing", (ulp > 0).float().mean().item())
    assert ulp.max().item() <= 2
    assert torch.equal(ops.vae_latent_tail(mom, sf, "mean", out_dtype=torch.float32), (mean * sf).contiguous())
    sigma = torch.tensor([0.7371], device="cuda")
    z16, mix = ops.vae_latent_tail(mom, sf, "eps", eps=eps, out_dtype=torch.bfloat16, sigma=sigma, mix_noise=noise)
    wz = want.bfloat16()
    sg = sigma.bfloat16().view(1, 1, 1, 1)
    wmix = (1.0 - sg) * wz + sg * noise                      # PF:965 on bf16 tensors
    assert wmix.dtype == torch.bfloat16
    for name, a, b in (("z", z16, wz), ("mix", mix, wmix)):
        d = _bf16_ulps(a, b.contiguous())
        print("latent tail bf16", name, "max ulp", d.max().item(), "share differing", (d > 0).float().mean().item())
        assert d.max().item() <= 1
    # given the kernel's own bf16 z, the mix arithmetic is exact
    assert torch.equal(mix, ((1.0 - sg) * z16 + sg * noise).contiguous())


def test_latent_tail_philox_statistics_and_randn_equality():
    from adv_grpo_amd import _lib, ops
    lib = _lib.load()
    B, C, h, w = 4, 16, 128, 128                               # 2^20 draws
    mom = torch.zeros(B, h, w, 2 * C, device="cuda")           # mean 0, logvar 0: z = eps exactly
    z = ops.vae_latent_tail(mom, 1.0, "philox", seed=1234, offset=77, out_dtype=torch.float32)
    ref = torch.empty_like(z)
    _lib.check(lib.advgrpo_randn(ref.data_ptr(), _lib.F32, ref.numel(), 1234, 77, _lib.stream_ptr()))
    assert torch.equal(z, ref)
    g = torch.Generator(device="cuda").manual_seed(1)
    mom = torch.randn(B, h, w, 2 * C, device="cuda", generator=g)
    z = ops.vae_latent_tail(mom, 1.0, "philox", seed=99, offset=0, out_dtype=torch.float32)
    m = mom.permute(0, 3, 1, 2)
    e = (z.double() - m[:, :C].double()) / torch.exp(0.5 * m[:, C:].double())
    n = e.numel()
    print("philox tail: mean", e.mean().item(), "var", e.var().item(), "n", n)
    assert abs(e.mean().item()) < 5 / n ** 0.5 and abs(e.var().item() - 1) < 5 * (2 / n) ** 0.5      # five standard errors
    # the mix noise stream: Philox under (mix_seed, mix_offset) rounded to bf16
    sigma = torch.ones(1, device="cuda")                       # sigma 1: mix = noise
    _, mix = ops.vae_latent_tail(mom, 1.0, "mean", sigma=sigma, mix_seed=5, mix_offset=11)
    ref16 = torch.empty(B, C, h, w, device="cuda", dtype=torch.bfloat16)
    _lib.check(lib.advgrpo_randn(ref16.data_ptr(), _lib.BF16, ref16.numel(), 5, 11, _lib.stream_ptr()))
    assert torch.equal(mix, ref16 + 0 * mix)


def _norm_err(got, ref):
    d = (got.double() - ref).abs()
    return d.max().item() / ref.abs().max().item(), d.mean().item() / ref.abs().max().item()


def _decoder_err(B, hw, fp16_checkpoint):
    """the yardstick: the decoder in the same mode against oracle/vae.py in float64 at the same latent size, unclamped, same recipe"""
    from adv_grpo_amd import ops, synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=fp16_checkpoint)
    dec = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3")
    lat = torch.randn(B, 16, hw, hw, generator=torch.Generator().manual_seed(hw)).to(torch.bfloat16)
    got = []
    orig = ops.image_postprocess
    ops.image_postprocess = lambda y: (got.append(y[..., :3].permute(0, 3, 1, 2).clone()), orig(y))[1]
    try:
        dec.c_decode = False                       # launch by launch (bit-identical to the C entry): the unclamped conv_out output is visible
        dec.two_streams = False
        dec.decode_to_image(lat.cuda())
    finally:
        ops.image_postprocess = orig
    W64 = {k: v.double().cuda() for k, v in W.items()}
    ref = o.vae_decode(W64, cfg, lat.double().cuda() / cfg.scaling_factor + cfg.shift_factor)
    return _norm_err(got[0], ref)


# fixed bounds: twice the largest values measured on an MI355X over the four cases below (3.34e-5 max at 512^2, 2.51e-6 mean at 3 x 64^2)
ENC_BOUND_MAX, ENC_BOUND_MEAN = 6.6e-5, 5.0e-6


@pytest.mark.parametrize("B,size,fp16_checkpoint", [(1, 128, False), (3, 64, False), (3, 128, True), (1, 512, False)])
def test_encoder_moments_vs_float64_restatement(B, size, fp16_checkpoint):
    """mode="bf16x3", synthetic weights, against the restatement in float64.  e = max|gpu - ref64| / max|ref64| (and the mean likewise) must be
    at most 2x the decoder's figure by the same recipe at the same latent size (same arithmetic on a shorter chain; the factor pays for the
    first layers reading un-normalised pixels).  The f32 restatement's own error against f64 is printed for scale at the small sizes.
    Measured on an MI355X (encoder max / mean; decoder max / mean; ratios):
      B=1 128^2        1.57e-5 / 2.35e-6;  2.62e-5 / 3.64e-6;  0.60 / 0.64      (f32 torch restatement vs f64: 1.4e-6 / 2.0e-7)
      B=3  64^2        1.27e-5 / 2.51e-6;  2.18e-5 / 3.18e-6;  0.58 / 0.79      (6.9e-7 / 1.4e-7)
      B=3 128^2 fp16   1.72e-5 / 1.98e-6;  1.27e-5 / 1.63e-6;  1.35 / 1.22      (1.5e-6 / 1.5e-7; the decoder runs its f16x2 path here, the encoder not)
      B=1 512^2        3.34e-5 / 2.10e-6;  2.37e-5 / 3.27e-6;  1.41 / 0.64
    The fixed bounds ENC_BOUND_* are twice the largest measured values; the ratio stays as the second assertion."""
    enc, W, cfg = _encoder(99, fp16_checkpoint)
    img = _images(B, size, size, size + B)
    mom = enc.moments(img.cuda())
    assert mom.shape == (B, 32, size // 8, size // 8) and mom.dtype == torch.float32
    W64 = {k: v.double().cuda() for k, v in W.items()}
    ref = ver.moments_from_images(W64, cfg, img.double().cuda())
    e_max, e_mean = _norm_err(mom, ref)
    if size <= 128:
        W32 = {k: v.float().cuda() for k, v in W.items()}
        f_max, f_mean = _norm_err(ver.moments_from_images(W32, cfg, img.float().cuda()), ref)
        print("f32 torch restatement vs f64: max", f_max, "mean", f_mean)
    d_max, d_mean = _decoder_err(B, size // 8, fp16_checkpoint)
    print(f"encoder B={B} {size}^2 fp16={fp16_checkpoint}: max {e_max:.3e} mean {e_mean:.3e}; decoder max {d_max:.3e} mean {d_mean:.3e}; "
          f"ratio max {e_max / d_max:.2f} mean {e_mean / d_mean:.2f}")
    assert torch.isfinite(mom).all()
    assert e_max <= 2 * d_max and e_mean <= 2 * d_mean
    assert e_max <= ENC_BOUND_MAX and e_mean <= ENC_BOUND_MEAN


def test_c_entry_is_bit_identical_to_launch_by_launch_and_batch_independent():
    enc, W, cfg = _encoder(7)
    img = _images(3, 64, 128, 11).cuda()
    enc.c_encode = True
    a = enc.moments(img)
    enc.c_encode = False
    b = enc.moments(img)
    assert torch.equal(a, b)
    enc.c_encode = True
    for i in range(3):                                         # image i of a batch of 3 gives the bits it gives alone
        assert torch.equal(enc.moments(img[i:i + 1]), a[i:i + 1])
    u8 = (img * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    # uint8 NHWC in: ToTensor's division by 255 runs in the first kernel (a true f32 division, as on the host; torch on the GPU multiplies by
    # the reciprocal instead, so the f32 image is made on the CPU)
    assert torch.equal(enc.moments(u8), enc.moments((u8.cpu().permute(0, 3, 1, 2).float() / 255.0).contiguous().cuda()))
    z = enc.encode(img, seed=3)
    assert z.dtype == torch.bfloat16 and z.shape == (3, 16, 8, 16) and torch.equal(z, enc.encode(img, seed=3))
    assert not torch.equal(z, enc.encode(img, seed=4))
    zm = enc.encode(img, sample=False, out_dtype=torch.float32)
    assert torch.equal(zm, (a[:, :16] * cfg.scaling_factor).contiguous())


def test_c_entry_error_behaviour():
    """bad shape, null pointer, short workspace -> error code and message, no launch"""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    enc, W, cfg = _encoder(7)
    img = _images(1, 64, 64, 1).cuda()
    d = _lib.VaeDecoderDesc.from_buffer_copy(enc._e_desc())
    d.B, d.h, d.w = 1, 64, 64
    need = lib.advgrpo_vae_encode_workspace_bytes(ctypes.byref(d))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    mom = torch.full((1, 8, 8, 32), 7.0, device="cuda")
    st = _lib.stream_ptr()
    assert lib.advgrpo_vae_encode(ctypes.byref(d), img.data_ptr(), _lib.F32, mom.data_ptr(), ws.data_ptr(), need - 1, st) != 0
    assert b"workspace" in lib.advgrpo_last_error()
    assert lib.advgrpo_vae_encode(ctypes.byref(d), None, _lib.F32, mom.data_ptr(), ws.data_ptr(), need, st) != 0
    assert b"null" in lib.advgrpo_last_error()
    assert lib.advgrpo_vae_encode(ctypes.byref(d), img.data_ptr(), _lib.F64, mom.data_ptr(), ws.data_ptr(), need, st) != 0
    bad = _lib.VaeDecoderDesc.from_buffer_copy(d)
    bad.h = 60                                                 # not a multiple of 8
    assert lib.advgrpo_vae_encode_workspace_bytes(ctypes.byref(bad)) == -1
    assert lib.advgrpo_vae_encode(ctypes.byref(bad), img.data_ptr(), _lib.F32, mom.data_ptr(), ws.data_ptr(), need, st) != 0
    assert b"descriptor" in lib.advgrpo_last_error()
    bad = _lib.VaeDecoderDesc.from_buffer_copy(d)
    bad.conv_in.form = 1
    assert lib.advgrpo_vae_encode(ctypes.byref(bad), img.data_ptr(), _lib.F32, mom.data_ptr(), ws.data_ptr(), need, st) != 0
    torch.cuda.synchronize()
    assert (mom == 7.0).all()                                  # nothing was launched
    with pytest.raises(ValueError, match="multiples of 8"):
        enc.moments(torch.zeros(1, 3, 48, 64, device="cuda"))
    d96 = _lib.VaeDecoderDesc.from_buffer_copy(d)
    d96.w = 96                                                 # 8 x 12 latent pixels: not a multiple of 64
    assert lib.advgrpo_vae_encode(ctypes.byref(d96), img.data_ptr(), _lib.F32, mom.data_ptr(), ws.data_ptr(), need, st) != 0
    assert b"multiple of 64" in lib.advgrpo_last_error()
    with pytest.raises(ValueError, match="bf16x3"):
        type(enc)(W, cfg, "cuda", mode="bf16")
    # the cached descriptor follows the weights it points at
    k = "encoder.conv_out.bias"
    before = enc.moments(img)
    enc.w[k] = enc.w[k] + 1.0                                  # a NEW tensor under the same name
    after = enc.moments(img)
    assert not torch.equal(after, before) and torch.allclose(after, before + 1.0, rtol=0, atol=1e-5)


class _StandinVae:
    def decode_to_image(self, latents):
        from oracle.standin import standin_vae_decode
        z = (latents / 1.5305) + 0.0609
        return (standin_vae_decode(z.to(torch.float32)) / 2 + 0.5).clamp(0, 1)


class _StandinEncoder:
    """the golden's stand-in vae.encode: takes what image_to_latent hands the encoder (uint8 NHWC from the host path)"""
    def encode(self, images, seed=None, noise=None, sample=True, out_dtype=torch.bfloat16):
        assert images.dtype == torch.uint8
        x = (images.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5
        return (ver.standin_latent_sample(x) * 1.5305).to(out_dtype)


def test_img2img_matches_reference_trajectory():
    """flux_to_sd3_denoise_random against the golden made by the reference's own function (stand-in velocity net, VAE and encoder; the same
    draws injected).  Tolerances: those of tests/test_gpu_rollout.py for pipeline_with_logprob_random in bf16 (same kernels, same comparison)."""
    from PIL import Image
    from adv_grpo_amd.diffusers_patch import sd3_img2img_with_logprob as I2I
    from adv_grpo_amd.pipeline import SD3Pipeline
    from oracle.standin import StandinVelocity
    g = np.load(os.path.join(G, "img2img.npz"))
    steps, B, target_idx, seed_random, img_seed = (int(v) for v in g["meta"])
    guidance, noise_level = (float(v) for v in g["scalars"])
    net = StandinVelocity().cuda()
    net.config = type("C", (), {"in_channels": 16})()
    pipe = SD3Pipeline(net, _StandinVae(), "cuda", vae_encoder=_StandinEncoder())
    pil = [Image.fromarray(a.numpy()) for a in ver.structured_images_u8(B, 512, seed=img_seed)]
    z = I2I.image_to_latent(pipe, pil)
    assert z.dtype == torch.bfloat16 and np.allclose(z.float().cpu().numpy(), g["z"], atol=2 ** -7 * 4, rtol=2 ** -7)
    tt = lambda k: torch.from_numpy(g[k]).to(torch.bfloat16).cuda()
    kw = dict(flux_images=pil, num_inference_steps=steps, guidance_scale=guidance, prompt_embeds=tt("pe"), negative_prompt_embeds=tt("npe"),
              pooled_prompt_embeds=tt("ppe"), negative_pooled_prompt_embeds=tt("nppe"), noise_level=noise_level, output_type="pt",
              mix_noise=tt("mix_noise"), noises=list(torch.from_numpy(g["noises"]).cuda()))
    random.seed(seed_random)
    image, lats, lps, tss = I2I.flux_to_sd3_denoise_random(pipe, **kw)
    after = random.randint(0, 10 ** 9)
    random.seed(seed_random)
    assert random.randint(5, 10) == target_idx and after == random.randint(0, 10 ** 9)     # exactly one draw consumed
    assert len(lats) == 3 and len(lps) == 2 and len(tss) == 2
    lat = torch.stack(lats, 1); lp = torch.stack(lps, 1); ts = torch.stack(tss, 1)
    assert lat.dtype == torch.bfloat16 and lp.dtype == torch.float32 and lat.shape == g["latents"].shape
    sched_ts = g["schedule_timesteps"]
    assert np.array_equal(ts.float().cpu().numpy(), np.broadcast_to(sched_ts[target_idx:target_idx + 2], (B, 2)))
    assert np.array_equal(ts.float().cpu().numpy(), g["timesteps"])
    tol = 2 ** -7
    assert np.allclose(lat.float().cpu().numpy(), g["latents"], atol=tol * 4, rtol=tol)
    assert np.allclose(lp.cpu().numpy(), g["log_probs"], rtol=5e-3)
    assert np.allclose(image.float().cpu().numpy(), g["image"], atol=2e-2)
    # the hook skips the draw and gives the same result
    state = random.getstate()
    image2, lats2, _, _ = I2I.flux_to_sd3_denoise_random(pipe, target_idx=target_idx, **kw)
    assert random.getstate() == state and torch.equal(image2, image) and all(torch.equal(a, b) for a, b in zip(lats, lats2))


def _own_models():
    """-> (pipe, encoder, decoder, images, kwargs): a 2-block MMDiT, the VAE encoder and decoder on synthetic weights, two 128 x 128 images"""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.mmdit import SD3Transformer2DModel
    from adv_grpo_amd.model_configs import MMDiTConfig
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    enc, _, vcfg = _encoder(21)
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(vcfg, 22), vcfg, "cuda", mode="bf16x3")
    mcfg = MMDiTConfig(num_layers=2, num_heads=6, joint_attention_dim=256, pooled_projection_dim=128, pos_embed_max_size=96,
                       dual_attention_layers=(0,))
    Wm = {k: v.to(torch.bfloat16) for k, v in synthetic.mmdit_weights(mcfg, 5).items()}
    pipe = SD3Pipeline(SD3Transformer2DModel(Wm, mcfg, "cuda"), dec, "cuda", vae_encoder=enc)
    gen = torch.Generator().manual_seed(9)
    pe = torch.randn(1, 21, 256, generator=gen).to(torch.bfloat16).cuda(); ppe = torch.randn(1, 128, generator=gen).to(torch.bfloat16).cuda()
    npe = torch.randn(1, 21, 256, generator=gen).to(torch.bfloat16).cuda(); nppe = torch.randn(1, 128, generator=gen).to(torch.bfloat16).cuda()
    img = _images(2, 128, 128, 8).cuda()
    kw = dict(flux_images=img, num_inference_steps=20, guidance_scale=4.5, prompt_embeds=pe, negative_prompt_embeds=npe,
              pooled_prompt_embeds=ppe, negative_pooled_prompt_embeds=nppe)
    return pipe, enc, dec, img, kw


def test_img2img_end_to_end_on_own_models():
    """encoder -> noise -> denoise -> decode at 128 x 128 with a 2-block MMDiT: runs, finite, repeatable for a fixed seed; with noise_level 0,
    the start at the LAST step (sigma of the mix and of the one denoise step small) the image stays close to decode(encode(x))."""
    from adv_grpo_amd.diffusers_patch import sd3_img2img_with_logprob as I2I
    pipe, enc, dec, img, kw = _own_models()
    random.seed(1)
    a = I2I.flux_to_sd3_denoise_random(pipe, seed=11, **kw)
    random.seed(1)
    b = I2I.flux_to_sd3_denoise_random(pipe, seed=11, **kw)
    assert a[0].shape == (2, 3, 128, 128) and torch.isfinite(a[0]).all() and all(torch.isfinite(t).all() for t in a[1] + a[2])
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]))
    assert len(a[1]) == 3 and len(a[2]) == 2 and len(a[3]) == 2
    # start at the last step of a long schedule: sigma -> small, one deterministic step
    image, lats, lps, _ = I2I.flux_to_sd3_denoise_random(pipe, seed=11, target_idx=199, noise_level=0.0,
                                                         **dict(kw, num_inference_steps=200, guidance_scale=1.0))
    assert len(lats) == 2 and len(lps) == 1
    want = dec.decode_to_image(enc.encode(img, seed=11))
    err = (image - want).abs().mean().item()
    print("img2img at the last step vs decode(encode(x)): mean abs", err, "image std", want.std().item())
    assert err < 0.05 * max(want.std().item(), 1e-3) + 0.02


def test_img2img_cfg_halves_on_two_streams_give_the_same_rollout():
    """pipe.cfg_two_streams under flux_to_sd3_denoise_random: the two halves of the CFG batch as two forwards on two HIP streams give the image,
    the recorded latents and the log-probs of the one forward of twice the batch, bit for bit (every row of every kernel of the transformer
    is independent of the other rows; tests/test_gpu_rollout.py has the same statement for pipeline_with_logprob_random)."""
    from adv_grpo_amd.diffusers_patch import sd3_img2img_with_logprob as I2I
    pipe, _, _, _, kw = _own_models()
    a = I2I.flux_to_sd3_denoise_random(pipe, seed=11, target_idx=7, **kw)
    pipe.cfg_two_streams = True
    try:
        b = I2I.flux_to_sd3_denoise_random(pipe, seed=11, target_idx=7, **kw)
        torch.cuda.synchronize()
        assert "_cfg_sides" in pipe.__dict__                  # the second call did go through the two-stream schedule
    finally:
        pipe.cfg_two_streams = False
    assert len(a[1]) == 3 and len(a[2]) == 2 and torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
