"""GPU parity of the VAE decoder path against the fp32 torch oracle (itself "parity unpinned" vs diffusers)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_conv3x3_implicit_gemm_matches_fp32_conv():
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    # Cout >= 128 runs on the dedicated kernel (192-pixel tiles: 768 = 4 x 192 pixels, 1600 is ragged), below it on the
    # generic one over the tripled contraction axis
    for (B, H, W, Ci, Co, up) in [(2, 16, 24, 64, 96, False), (1, 8, 8, 128, 64, True), (2, 32, 32, 128, 3, False),
                                  (2, 16, 24, 64, 128, False), (1, 20, 20, 128, 256, True), (1, 13, 11, 192, 384, False),
                                  # degenerate rows / columns: every pixel is at both image-row edges (W = 1), one image row
                                  # (H = 1), tiles that straddle images (3 x 65 pixels), an odd upsampled width
                                  (2, 7, 1, 64, 128, False), (3, 1, 65, 64, 128, False), (5, 3, 3, 64, 128, True)]:
        x = torch.randn(B, H, W, Ci, device="cuda", generator=g).to(torch.bfloat16)
        wt = (torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (3 * Ci ** 0.5)).to(torch.bfloat16)
        bias = torch.randn(Co, device="cuda", generator=g).to(torch.bfloat16)
        Ho, Wo = (2 * H, 2 * W) if up else (H, W)
        res = torch.randn(B, Ho, Wo, Co, device="cuda", generator=g).to(torch.bfloat16)
        y = ops.conv3x3(x, wt.permute(0, 2, 3, 1).reshape(Co, -1).contiguous(), bias=bias, upsample=up, residual=res,
                        out_dtype=torch.float32)
        xin = x.float().permute(0, 3, 1, 2)
        if up:
            xin = torch.nn.functional.interpolate(xin, scale_factor=2.0, mode="nearest")
        ref = torch.nn.functional.conv2d(xin, wt.float(), bias.float(), padding=1).permute(0, 2, 3, 1) + res.float()
        assert (y - ref).abs().max().item() < 2e-3 * ref.abs().max().item() + 1e-3


def test_groupnorm_silu_and_softmax_rows():
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    for C in (128, 256, 512):
        x = (torch.randn(2, 24, 24, C, device="cuda", generator=g) * 2 + 0.5).to(torch.bfloat16)
        w = torch.randn(C, device="cuda", generator=g).to(torch.bfloat16)
        b = torch.randn(C, device="cuda", generator=g).to(torch.bfloat16)
        y = ops.groupnorm_nhwc(x, w, b, 32, 1e-6, True)
        ref = torch.nn.functional.silu(torch.nn.functional.group_norm(x.float().permute(0, 3, 1, 2), 32, w.float(),
                                                                       b.float(), 1e-6)).permute(0, 2, 3, 1)
        # bf16 output rounding (2^-8 relative) + f32 statistics
        assert ((y.float() - ref).abs() <= 2 ** -8 * ref.abs() + 5e-3).all()
    s = (torch.randn(37, 4096, device="cuda", generator=g) * 3).to(torch.bfloat16)
    ref = s.float().softmax(-1)
    ops.softmax_rows_(s)
    assert (s.float() - ref).abs().max().item() < 1e-3
    assert ((s.float().sum(-1) - 1).abs() < 2e-2).all()
    # long rows: the 16384 keys of the decoder's mid-block attention at 1024^2 (one workgroup per row)
    s = (torch.randn(5, 16384, device="cuda", generator=g) * 3).to(torch.bfloat16)
    ref = s.float().softmax(-1)
    ops.softmax_rows_(s)
    assert (s.float() - ref).abs().max().item() < 1e-3 and ((s.float().sum(-1) - 1).abs() < 2e-2).all()


@pytest.mark.parametrize("B,hw", [(2, 16), (1, 64)])
def test_vae_decode_vs_fp32_oracle(B, hw):
    """Full SD3 VAE decoder shapes (conv widths 512/512/256/128, one mid attention).  hw=64 is the C2
    latent size (512^2 image).  Tolerance (bf16 operands vs the reference's fp32): mean abs error on the
    [0,1] image <= 4e-3 (about one 8-bit level), max abs <= 6e-2."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99)
    Wb = {k: v.to(torch.bfloat16) for k, v in W.items()}
    g = torch.Generator().manual_seed(hw)
    lat = torch.randn(B, 16, hw, hw, generator=g).to(torch.bfloat16)
    dec = AutoencoderKLDecoder(Wb, cfg, "cuda", mode="bf16")
    img = dec.decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in Wb.items()}
    z = lat.float().cuda() / cfg.scaling_factor + cfg.shift_factor
    ref = o.postprocess(o.vae_decode(W32, cfg, z))
    assert img.shape == (B, 3, 8 * hw, 8 * hw) and img.dtype == torch.float32
    err = (img - ref).abs()
    print("vae image err mean", err.mean().item(), "max", err.max().item(), "ref std", ref.std().item())
    assert err.mean().item() < 4e-3 and err.max().item() < 6e-2


def test_split_bf16x3_kernels_vs_fp32():
    """The pieces of the split-bf16 decode mode against fp32 torch: hi/lo split (hi + lo reproduces f32 to 2^-16), the
    convolution over [hi|hi|lo] x [hi|lo|hi] operands with f32 bias / residual (1e-4 of the output range: three bf16 MFMA
    products, f32 accumulate), GroupNorm(+SiLU) f32 -> split, softmax f32 -> split."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(33, 64, device="cuda", generator=g) * 5
    b = torch.randn(64, device="cuda", generator=g)
    for order in (0, 1):
        s3 = ops.split_x3(x, order, bias=b).float()
        hi, lo = s3[:, :64], (s3[:, 128:] if order == 0 else s3[:, 64:128])
        assert torch.equal(hi, (x + b).to(torch.bfloat16).float())
        assert torch.equal(s3[:, 64:128] if order == 0 else s3[:, 128:], hi)
        assert ((hi + lo - (x + b)).abs() <= 2.0 ** -16 * (x + b).abs()).all()
    # Cout >= 128 runs on the dedicated kernel (192-pixel tiles: 768 = 4 x 192 pixels, 1600 is ragged), below it on the
    # generic one over the tripled contraction axis
    for (B, H, W, Ci, Co, up) in [(2, 16, 24, 64, 96, False), (1, 8, 8, 128, 64, True), (2, 32, 32, 128, 3, False),
                                  (2, 16, 24, 64, 128, False), (1, 20, 20, 128, 256, True), (1, 13, 11, 192, 384, False),
                                  # degenerate rows / columns: every pixel is at both image-row edges (W = 1), one image row
                                  # (H = 1), tiles that straddle images (3 x 65 pixels), an odd upsampled width
                                  (2, 7, 1, 64, 128, False), (3, 1, 65, 64, 128, False), (5, 3, 3, 64, 128, True)]:
        x = torch.randn(B, H, W, Ci, device="cuda", generator=g)
        wt = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (3 * Ci ** 0.5)
        bias = torch.randn(Co, device="cuda", generator=g)
        Ho, Wo = (2 * H, 2 * W) if up else (H, W)
        res = torch.randn(B, Ho, Wo, Co, device="cuda", generator=g)
        w3 = ops.split_x3(wt.permute(0, 2, 3, 1).contiguous(), order=1).reshape(Co, -1)
        y = ops.conv3x3_x3(ops.split_x3(x), w3, bias=bias, upsample=up, residual=res)
        xin = x.double().permute(0, 3, 1, 2)
        if up:
            xin = torch.nn.functional.interpolate(xin, scale_factor=2.0, mode="nearest")
        ref = torch.nn.functional.conv2d(xin, wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1) + res.double()
        err = (y.double() - ref).abs().max().item()
        print("conv x3", (B, H, W, Ci, Co, up), "max err", err, "of", ref.abs().max().item())
        assert err < 1e-4 * ref.abs().max().item()
        if Co >= 128:      # the dedicated kernel reads the hi and lo thirds only: order 2 leaves the middle one unwritten
            x2 = torch.full((B, H, W, 3 * Ci), float("nan"), device="cuda", dtype=torch.bfloat16)
            x2[..., :Ci] = ops.split_x3(x, 2)[..., :Ci]
            x2[..., 2 * Ci:] = ops.split_x3(x, 2)[..., 2 * Ci:]
            assert torch.equal(ops.conv3x3_x3(x2, w3, bias=bias, upsample=up, residual=res), y)
    for C in (128, 256, 512):
        x = torch.randn(2, 24, 24, C, device="cuda", generator=g) * 2 + 0.5
        w = torch.randn(C, device="cuda", generator=g)
        b = torch.randn(C, device="cuda", generator=g)
        y3 = ops.groupnorm_nhwc_x3(x, w, b, 32, 1e-6, True).float()
        ref = torch.nn.functional.silu(torch.nn.functional.group_norm(x.double().permute(0, 3, 1, 2), 32, w.double(), b.double(),
                                                                       1e-6)).permute(0, 2, 3, 1)
        assert torch.equal(y3[..., :C], y3[..., C:2 * C])
        got = y3[..., :C].double() + y3[..., 2 * C:].double()
        assert ((got - ref).abs() <= 2.0 ** -15 * ref.abs() + 2e-6).all()
        p3 = ops.groupnorm_nhwc_x3(x, w, b, 32, 1e-6, True, pair_only=True).float()
        assert torch.equal(p3[..., :C], y3[..., :C]) and torch.equal(p3[..., 2 * C:], y3[..., 2 * C:])
    s = torch.randn(37, 4096, device="cuda", generator=g) * 3
    p3 = ops.softmax_rows_x3(s).float()
    got = p3[:, :4096].double() + p3[:, 8192:].double()
    ref = s.double().softmax(-1)
    assert ((got - ref).abs() <= 2.0 ** -15 * ref + 1e-9).all() and ((got.sum(-1) - 1).abs() < 1e-4).all()
    a = torch.randn(50, 128, device="cuda", generator=g)
    c = torch.randn(50, 128, device="cuda", generator=g)
    bias = torch.randn(128, device="cuda", generator=g)
    assert torch.equal(ops.add_rows_f32(a, c, bias), a + c + bias)


@pytest.mark.parametrize("fp16_checkpoint", [False, True])
def test_vae_decode_two_streams_is_bit_identical(fp16_checkpoint):
    """mode="bf16x3" decodes a batch as two half batches on two HIP streams (vae.py: _decode_x3); every image must come out
    bit for bit as from the single-stream chain, for even and odd batches -- also on the f16x2 path, whose GroupNorm statistics
    come out of the convolutions' epilogues in blocks that do not depend on the image's position in the batch."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import VaeConfig
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = VaeConfig()
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=fp16_checkpoint), cfg, "cuda", mode="bf16x3")
    g = torch.Generator(device="cuda").manual_seed(3)
    for B in (2, 3, 8):
        lat = torch.randn(B, 16, 16, 16, device="cuda", generator=g).to(torch.bfloat16)
        dec.two_streams = True
        two = dec.decode_to_image(lat)
        again = dec.decode_to_image(lat)
        dec.two_streams = False
        one = dec.decode_to_image(lat)
        torch.cuda.synchronize()
        assert two.shape == one.shape and torch.equal(two, one) and torch.equal(again, one)


@pytest.mark.parametrize("B,hw", [(2, 16), (1, 64)])
def test_vae_decode_bf16x3_mode_vs_fp32_oracle(B, hw):
    """mode="bf16x3": f32 weights (NOT rounded to bf16 -- the mode exists to reproduce the reference's fp32 decode,
    TP:481), f32 between the matrix products.  Tolerance on the [0,1] image: mean abs <= 2e-5, max abs <= 1e-3 -- a
    hundredth of an 8-bit level on average, against 4e-3 / 6e-2 for the default bf16 mode on bf16-rounded weights."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99)
    g = torch.Generator().manual_seed(hw)
    lat = torch.randn(B, 16, hw, hw, generator=g).to(torch.bfloat16)
    dec = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3")
    img = dec.decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in W.items()}
    z = lat.float().cuda() / cfg.scaling_factor + cfg.shift_factor
    ref = o.postprocess(o.vae_decode(W32, cfg, z))
    assert img.shape == (B, 3, 8 * hw, 8 * hw) and img.dtype == torch.float32
    err = (img - ref).abs()
    print("vae x3 image err mean", err.mean().item(), "max", err.max().item(), "ref std", ref.std().item())
    assert err.mean().item() < 2e-5 and err.max().item() < 1e-3
    with pytest.raises(ValueError):
        AutoencoderKLDecoder(W, cfg, "cuda", mode="fp32")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_vae_decode_at_1024_vs_fp32_oracle(mode):
    """BASELINE config 4's decode size: one 128 x 128 latent -> 1024^2 image (the mid-block attention runs over 16384 keys,
    the last up block over 1024^2 x 128 activations) in both modes, against the fp32 oracle decode; same bounds as at 512^2."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99)
    if mode == "bf16":
        W = {k: v.to(torch.bfloat16) for k, v in W.items()}
    lat = torch.randn(1, 16, 128, 128, generator=torch.Generator().manual_seed(128)).to(torch.bfloat16)
    img = AutoencoderKLDecoder(W, cfg, "cuda", mode=mode).decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in W.items()}
    with torch.no_grad():
        ref = o.postprocess(o.vae_decode(W32, cfg, lat.float().cuda() / cfg.scaling_factor + cfg.shift_factor))
    assert img.shape == (1, 3, 1024, 1024) and torch.isfinite(img).all()
    err = (img - ref).abs()
    print(f"vae {mode} @1024^2: image err mean {err.mean().item():.3e} max {err.max().item():.3e}")
    if mode == "bf16x3":
        assert err.mean().item() < 2e-5 and err.max().item() < 1e-3
    else:
        assert err.mean().item() < 4e-3 and err.max().item() < 6e-2


def test_bf16_vae_decode_reward_deltas_vs_fp32_decode_at_config2():
    """The reference decodes in fp32 (TP:481, PF:667-670); the product's decoder runs bf16 MFMA / f32 accumulate with bf16
    activations (fp32 matrix math is 1/16 of the bf16 rate on gfx950).  What matters downstream is the REWARD of a decoded
    image relative to the spread of rewards inside its GRPO group (advantages are (r - mean) / std over the 8 images of a
    prompt), not the image error itself.  At BASELINE config 2 sizes (8 latents of one group, 64x64x16 -> 512^2) the same
    latents are decoded by the product decoder and by the fp32 oracle decoder, and both image sets go through the SAME
    product scorers (full-size PickScore CLIP ViT-H/14, DINOv2-B/14 patch head).
    No trained scorer weights exist on the box, and a random-weight tower has no invariance to pixel noise: it moves as
    much under HALF AN 8-BIT LEVEL of uniform noise -- which the reference's own uint8 quantisation (RW:567) injects --
    as under the bf16 decode.  The stated tolerance is therefore two-sided (deviation 1; measured: PickScore
    0.22-0.35 of the group std = 0.55-0.85 of the half-level effect; DINO patch 2x the half-level effect, its group std of
    1.5e-4 being numerical dust with a random head):
      * PickScore: max |r_bf16 - r_fp32| <= 0.5 x within-group std and <= 2 x the half-level-noise effect (largest of six
        seeded noise draws; with unseeded draws the yardstick itself moved between 2.3e-3 and 3.9e-3 from run to run);
      * DINO patch: <= 3 x the half-level-noise effect."""
    from adv_grpo_amd import rewards, synthetic, vit
    from adv_grpo_amd.d_step import DinoHeadTrainable
    from adv_grpo_amd.model_configs import ClipConfig, DinoConfig
    from adv_grpo_amd.pickscore_scorer import PickScoreScorer
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    Wb = {k: v.to(torch.bfloat16) for k, v in synthetic.vae_decoder_weights(cfg, 4321).items()}
    g = torch.Generator().manual_seed(8)
    # a group of 8 related samples, as a rollout produces them: a shared component plus per-sample variation
    lat = (0.8 * torch.randn(1, 16, 64, 64, generator=g) + 0.6 * torch.randn(8, 16, 64, 64, generator=g)).to(torch.bfloat16)
    img_b = AutoencoderKLDecoder(Wb, cfg, "cuda", mode="bf16").decode_to_image(lat.cuda())
    img_x = AutoencoderKLDecoder({k: v.float() for k, v in Wb.items()}, cfg, "cuda", mode="bf16x3").decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in Wb.items()}
    with torch.no_grad():
        img_f = torch.cat([o.postprocess(o.vae_decode(W32, cfg, lat[i:i + 2].float().cuda() / cfg.scaling_factor + cfg.shift_factor))
                           for i in range(0, 8, 2)])
    del W32
    err = (img_b - img_f).abs()
    errx = (img_x - img_f).abs()
    u8 = lambda im: (im.to(torch.bfloat16).float() * 255).round()
    flips_x, flips_b = (u8(img_x) != u8(img_f)).float().mean().item(), (u8(img_b) != u8(img_f)).float().mean().item()
    print(f"bf16x3 image err mean {errx.mean():.2e} max {errx.max():.2e}; uint8 pixels that differ from the fp32 decode: "
          f"bf16x3 {flips_x:.4%}, bf16 {flips_b:.2%}")
    assert errx.max().item() < 1e-4 and flips_x < 2e-3 and (u8(img_x) - u8(img_f)).abs().max().item() <= 1
    ccfg, dcfg = ClipConfig(), DinoConfig()
    pick = PickScoreScorer("cuda", dtype=torch.bfloat16, model_sd=synthetic.clip_weights(ccfg, 777), clip_cfg=ccfg)
    ids = synthetic.clip_input_ids(1, 3).repeat(8, 1).cuda()
    dino = vit.DinoV2({k: v.to(torch.bfloat16) for k, v in synthetic.dino_weights(dcfg, 7).items()}, dcfg, "cuda")
    head = DinoHeadTrainable(device="cuda", seed=0)
    idx = torch.randint(0, 1369, (8, 64), generator=g).cuda()
    dfn = rewards.dino_patch_cotrain_score("cuda")
    out = {}
    for name, score in (("pickscore", lambda im: pick(ids, im.to(torch.bfloat16))),
                        ("dino_patch", lambda im: dfn(dino, head, im.to(torch.bfloat16), None, None, idx=idx)[0])):
        rb, rf = score(img_b).double(), score(img_f).double()
        std = rf.std(unbiased=False).item()
        d = (rb - rf).abs().max().item()
        out[name] = (d, std)
        print(f"{name}: max |r_bf16 - r_fp32| {d:.3e}  within-group std {std:.3e}  ratio {d / std:.4f}   image err mean {err.mean():.2e} max {err.max():.2e}")
        # what the same scorer does with half an 8-bit level of uniform noise on the fp32 images
        # (seeded draws, the largest of six: the yardstick itself varied by 1.7x between unseeded runs)
        gn = torch.Generator(device="cuda").manual_seed(1234)
        noise = max((score((img_f + (torch.rand(img_f.shape, device="cuda", generator=gn) - 0.5) / 255).clamp(0, 1)).double()
                     - rf).abs().max().item() for _ in range(6))
        print(f"   (effect of +-0.5/255 uniform pixel noise on this random-weight scorer: {noise:.3e})")
        # mode="bf16x3" (the fp32-equivalent decode).  Its images are within 3e-5 of the fp32 decode and, as uint8 (RW:567),
        # differ from it in < 0.2 % of the pixels by one level -- yet these random-weight towers still move by about as
        # much as under the bf16 decode (measured 1.5e-3 vs 1.3e-3 on PickScore): with untrained weights the reward delta
        # measures the tower's sensitivity to ANY flipped pixel, which is why the image-level numbers are the ones asserted
        # tightly and the reward-level ones only against the half-level yardstick.
        dx = (score(img_x).double() - rf).abs().max().item()
        print(f"   bf16x3 mode: max |r_x3 - r_fp32| {dx:.3e}  ({dx / noise:.4f} of the half-level effect)")
        assert dx <= 2.0 * noise, (name, dx, noise)
        if name == "pickscore":
            assert d <= 0.5 * std and d <= 2.0 * noise, (name, d, std, noise)
        else:
            assert d <= 3.0 * noise, (name, d, std, noise)


def test_vae_decode_is_bitwise_reproducible():
    """Two decodes of the same latents give the same bits (GroupNorm sums its statistics in a fixed order; with atomics
    the statistics differed in the last bit from run to run and the decoder amplified that to 2e-2 on the image)."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import VaeConfig
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 5)
    lat = torch.randn(2, 16, 32, 32, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).cuda()
    for mode in ("bf16", "bf16x3"):
        dec = AutoencoderKLDecoder(W, cfg, "cuda", mode=mode)
        a = dec.decode_to_image(lat)
        b = dec.decode_to_image(lat)
        assert torch.equal(a, b), mode


@pytest.mark.parametrize("B,H,W,C,Co,up,gn", [(2, 16, 24, 128, 128, False, True), (1, 33, 20, 256, 128, False, True),
                                              (2, 8, 12, 512, 512, True, False), (1, 16, 16, 64, 256, False, False),
                                              # >= 1024 tiles of 192 x 256: the wide tile of round 6 (ragged last pixel tile; two column tiles + upsample)
                                              (1, 448, 448, 128, 256, False, True), (1, 224, 224, 64, 512, True, False)])
def test_conv3x3_f16x2_vs_fp64_conv(B, H, W, C, Co, up, gn):
    """The two-product convolution for fp16-exact weights (include/advgrpo.h "f16x2"): fp16-pair activations (from the
    GroupNorm + SiLU producer, or the plain split with the 2^-4 pre-scale of un-normalised inputs) x one-piece fp16 weights
    against an fp64 convolution of the same f32 operands; the nearest x2 upsample folded in; activations of magnitude ~300 on
    the raw path (fp16 range).  Error bound: the activations' 22-bit pairs, i.e. better than the split-bf16 kernel's 2^-16."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(H * 7 + C)
    x = torch.randn(B, H, W, C, device="cuda", generator=g) * (1.0 if gn else 300.0)
    wt = (torch.randn(Co, C, 3, 3, device="cuda", generator=g) / (C * 9) ** 0.5).half().float()      # fp16-exact
    bias = torch.randn(Co, device="cuda", generator=g) * 0.1
    w16 = wt.permute(0, 2, 3, 1).contiguous().half().reshape(Co, -1)
    res = torch.randn(B, H * (2 if up else 1), W * (2 if up else 1), Co, device="cuda", generator=g)
    if gn:
        gw, gb = 1 + 0.1 * torch.randn(C, device="cuda", generator=g), 0.1 * torch.randn(C, device="cuda", generator=g)
        a = ops.groupnorm_nhwc_f16x2(x, gw, gb, 32, 1e-6, True)
        xin = torch.nn.functional.silu(torch.nn.functional.group_norm(x.permute(0, 3, 1, 2).double(), 32, gw.double(), gb.double(), 1e-6))
        y = ops.conv3x3_f16x2(a, w16, bias=bias, upsample=up, residual=res)
    else:
        a = ops.split_f16x2(x, prescale=2.0 ** -4)
        xin = x.permute(0, 3, 1, 2).double()
        y = ops.conv3x3_f16x2(a, w16, bias=bias, upsample=up, residual=res, alpha=2.0 ** 4)
    if up:
        xin = torch.nn.functional.interpolate(xin, scale_factor=2, mode="nearest")
    ref = torch.nn.functional.conv2d(xin, wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1) + res.double()
    err = (y.double() - ref).abs().max().item() / ref.abs().max().item()
    print("f16x2 conv rel max err", err)
    assert err < 3e-6, err


@pytest.mark.parametrize("B,hw", [(2, 16), (2, 64)])
def test_vae_decode_f16x2_path_for_an_fp16_checkpoint(B, hw):
    """The decoder on weights as the reference holds them -- the released fp16 VAE checkpoint upcast to fp32 (TP:447,481): every
    3x3 convolution with >= 128 output channels takes the two-product f16x2 kernel (checked), the image stays within the bf16x3
    mode's bound of the fp32 oracle decode, a weight set that is NOT exact in fp16 keeps the three-product kernels (checked), and
    f16_weights=False on the fp16 checkpoint gives the three-product result within the same bound."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=True)
    lat = torch.randn(B, 16, hw, hw, generator=torch.Generator().manual_seed(hw)).to(torch.bfloat16)
    dec = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3")
    n16 = sum(k.endswith("@f16") for k in dec.w)
    assert n16 == 31, n16        # 2 x 14 resnets + 3 upsamplers: every 3x3 convolution but conv_in (16 input channels) and conv_out (3 outputs)
    img = dec.decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in W.items()}
    ref = o.postprocess(o.vae_decode(W32, cfg, lat.float().cuda() / cfg.scaling_factor + cfg.shift_factor))
    err = (img - ref).abs()
    print("vae f16x2 image err mean", err.mean().item(), "max", err.max().item(), "convolutions on the f16x2 kernel:", n16)
    assert err.mean().item() < 2e-5 and err.max().item() < 1e-3
    img3 = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3", f16_weights=False).decode_to_image(lat.cuda())
    assert (img3 - ref).abs().mean().item() < 2e-5
    dec_inexact = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 99), cfg, "cuda", mode="bf16x3")
    assert not any(k.endswith("@f16") for k in dec_inexact.w)


def _tf32(t):
    """f32 -> the value a TF32 operand keeps: 10 explicit mantissa bits, round to nearest with ties away from zero (cvt.rna.tf32.f32)."""
    i = t.contiguous().view(torch.int32)
    return ((i + 0x1000) & ~0x1FFF).view(torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw", [(2, 64), (1, 128)])
def test_vae_decode_f16x1_tf32_class_mode_is_no_worse_than_a_simulated_tf32_decode(B, hw):
    """The opt-in "f16x1" decoder (AutoencoderKLDecoder(f16_single=True): ONE fp16 product per f32 product in the 31 wide 3x3 convolutions,
    f32 accumulation, f32 between kernels) against what the reference's own settings compute on the hardware it was written for:
    allow_tf32 = True (config/base.py:22-23, TP:537-538) makes every fp32 convolution and matmul of the fp32 VAE (TP:481) round BOTH operands
    to TF32.  Simulated here on the fp32 oracle by rounding the operands of every F.conv2d / F.linear to 10 explicit mantissa bits.
    Stated bound: the f16x1 image is no further from the exact-fp32 oracle decode than the simulated-TF32 decode is (mean; max within 1.5 x),
    at 512^2 and 1024^2.  It is a priced leg (bench.py `vae.value_if_tf32_class`), not the default mode."""
    import torch.nn.functional as F
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    W = synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=True)
    lat = torch.randn(B, 16, hw, hw, generator=torch.Generator().manual_seed(hw)).to(torch.bfloat16)
    dec = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3", f16_single=True)
    assert dec.arithmetic()["f16x1"] == 31 and dec.arithmetic()["f16x2"] == 0 and "f16x1 (31/33 convs)" in dec.arithmetic()["text"]
    img = dec.decode_to_image(lat.cuda())
    W32 = {k: v.float().cuda() for k, v in W.items()}
    z = lat.float().cuda() / cfg.scaling_factor + cfg.shift_factor
    ref = o.postprocess(o.vae_decode(W32, cfg, z))
    conv2d, linear = F.conv2d, F.linear
    try:
        F.conv2d = lambda x, w, b=None, **kw: conv2d(_tf32(x), _tf32(w), b, **kw)
        F.linear = lambda x, w, b=None: linear(_tf32(x), _tf32(w), b)
        sim = o.postprocess(o.vae_decode(W32, cfg, z))
    finally:
        F.conv2d, F.linear = conv2d, linear
    e1, et = (img - ref).abs(), (sim - ref).abs()
    dec_default_img = AutoencoderKLDecoder(W, cfg, "cuda", mode="bf16x3").decode_to_image(lat.cuda())
    e2 = (dec_default_img - ref).abs()
    print(f"vs the fp32 oracle at {8 * hw}^2: f16x1 mean {e1.mean().item():.3e} max {e1.max().item():.3e} | simulated TF32 mean {et.mean().item():.3e} "
          f"max {et.max().item():.3e} | default (f16x2) mean {e2.mean().item():.3e} max {e2.max().item():.3e}")
    assert et.mean().item() > 0 and e1.mean().item() <= et.mean().item() and e1.max().item() <= 1.5 * et.max().item()
    # what the scorers receive is the uint8 image (RW:567): pixels that land on another 8-bit level than the exact-fp32 decode's
    u8 = lambda im: (im.to(torch.bfloat16).float() * 255).round()
    f1, ft, f2 = ((u8(x) != u8(ref)).float().mean().item() for x in (img, sim, dec_default_img))
    print(f"uint8 pixels that differ from the fp32 decode at {8 * hw}^2: f16x1 {f1:.3%} | simulated TF32 {ft:.3%} | default {f2:.3%}")
    assert f1 <= 1.1 * ft and (u8(img) - u8(ref)).abs().max().item() <= 1
    assert e2.mean().item() < 2e-5                                   # (the default mode on the same inputs: the fp32-equivalent bound)


@pytest.mark.gpu
@pytest.mark.parametrize("offset,tol", [(40.0, 3e-5), (400.0, 3e-5), (4000.0, 3e-4)])
def test_groupnorm_statistics_with_a_mean_far_from_zero(offset, tol):
    """the group statistics are f32 {sum, sum of squares} over blocks of 64 values (conv epilogue) or a thread's pixels (own
    pass), combined in f64, variance = E[x^2] - E[x]^2: cancellation when |mean| >> std.  What is lost is the f32 rounding of the squares,
    so the relative error of the variance grows as (mean / std)^2: without a guard 9e-5 of the output at mean / std = 34 (own pass; 1.6e-5
    from the epilogue sums) and 7e-3 at 340.  Guard (vae.hip groupnorm_refine): when the first estimate has mean^2 > 256 var the finalize
    workgroup re-reads its (image, group) and sums deviations from that estimate in f64 -- fp32-equivalent again at any mean (what is left
    at 3 000 is the f32 subtraction x - mean of the apply pass, one ulp of x); never taken on ordinary inputs, whose bits are unchanged."""
    from adv_grpo_amd import ops
    B, H, W, C, Co = 2, 32, 32, 128, 128
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(B, H, W, C, device="cuda", generator=g)
    gw, gb = 1 + 0.1 * torch.randn(C, device="cuda", generator=g), 0.1 * torch.randn(C, device="cuda", generator=g)
    w16 = (torch.randn(Co, 9 * C, device="cuda", generator=g) / (C * 9) ** 0.5).half()
    bias = offset + 0.1 * torch.randn(Co, device="cuda", generator=g)
    res = torch.randn(B, H, W, Co, device="cuda", generator=g)
    a = ops.groupnorm_nhwc_f16x2(x, gw, gb, 32, 1e-6, True)
    y = ops.conv3x3_f16x2(a, w16, bias=bias, residual=res, gn_stats=True)
    ratio = (y.mean() / y.std()).item()
    assert 0.5 * offset / 1.5 < ratio < 2 * offset
    gw2, gb2 = 1 + 0.1 * torch.randn(Co, device="cuda", generator=g), 0.1 * torch.randn(Co, device="cuda", generator=g)
    ref = torch.nn.functional.silu(torch.nn.functional.group_norm(y.permute(0, 3, 1, 2).double(), 32, gw2.double(), gb2.double(), 1e-6)).permute(0, 2, 3, 1)

    def value(n):       # fp16 pair -> f32
        h = n.view(torch.float16).view(B, H, W, 3, Co)
        return h[..., 0, :].float() + h[..., 2, :].float()
    for n in (ops.groupnorm_nhwc_f16x2(y, gw2, gb2, 32, 1e-6, True, tile_stats=y.gn_tile_stats), ops.groupnorm_nhwc_f16x2(y, gw2, gb2, 32, 1e-6, True),
              None):
        v = value(n) if n is not None else ops.groupnorm_nhwc_x3(y, gw2, gb2, 32, 1e-6, True).float().view(B, H, W, 3, Co)[..., [0, 2], :].sum(-2)
        assert torch.isfinite(v).all()
        err = (v.double() - ref).abs().max().item() / ref.abs().max().item()
        assert err < tol, (offset, ratio, err)


@pytest.mark.parametrize("B,H,W,C,Co,up", [(3, 24, 24, 128, 256, False), (2, 16, 16, 512, 512, True), (5, 40, 24, 256, 128, False),
                                           (2, 320, 320, 128, 256, False)])       # (the last: the wide 192 x 256 tile's epilogue)
def test_groupnorm_statistics_from_the_conv_epilogue(B, H, W, C, Co, up):
    """advgrpo_conv3x3_nhwc_f16x2's gn_partial: {sum, sum of squares} per block of 16 pixels x 4 output channels (HW is not a
    multiple of the kernel's 192-pixel tile in any of these cases) -- against the sums of the stored output, and the
    GroupNorm that consumes them against the one that runs its own statistics pass (same f16-pair output up to the last bit of
    mean / rstd: the two sum the same values in a different order)."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(C + H)
    x = torch.randn(B, H, W, C, device="cuda", generator=g)
    gw, gb = 1 + 0.1 * torch.randn(C, device="cuda", generator=g), 0.1 * torch.randn(C, device="cuda", generator=g)
    w16 = (torch.randn(Co, 9 * C, device="cuda", generator=g) / (C * 9) ** 0.5).half()
    bias = torch.randn(Co, device="cuda", generator=g)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    res = torch.randn(B, Ho, Wo, Co, device="cuda", generator=g)
    a = ops.groupnorm_nhwc_f16x2(x, gw, gb, 32, 1e-6, True)
    y = ops.conv3x3_f16x2(a, w16, bias=bias, upsample=up, residual=res, gn_stats=True)
    y0 = ops.conv3x3_f16x2(a, w16, bias=bias, upsample=up, residual=res)
    assert torch.equal(y, y0) and not hasattr(y0, "gn_tile_stats")
    part = y.gn_tile_stats                                    # [B HW / 16, Co / 4, 2]
    HW = Ho * Wo
    rows = y.view(B * HW // 16, 16, Co // 4, 4).double()
    want_s, want_q = rows.sum(dim=(1, 3)), (rows ** 2).sum(dim=(1, 3))
    assert (part[..., 0].double() - want_s).abs().max().item() <= 1e-5 * max(1.0, want_q.max().item() ** 0.5 * 8)
    assert (part[..., 1].double() - want_q).abs().max().item() <= 1e-5 * max(1.0, want_q.max().item())
    # an image's sums do not depend on where it stands in the batch
    yb = ops.conv3x3_f16x2(a[1:].contiguous(), w16, bias=bias, upsample=up, residual=res[1:].contiguous(), gn_stats=True)
    assert torch.equal(yb, y[1:]) and torch.equal(yb.gn_tile_stats, part[HW // 16:])
    gw2, gb2 = 1 + 0.1 * torch.randn(Co, device="cuda", generator=g), 0.1 * torch.randn(Co, device="cuda", generator=g)
    n_fused = ops.groupnorm_nhwc_f16x2(y, gw2, gb2, 32, 1e-6, True, tile_stats=part)
    n_plain = ops.groupnorm_nhwc_f16x2(y, gw2, gb2, 32, 1e-6, True)
    def value(n):       # fp16 pair -> f32
        h = n.view(torch.float16).view(B, Ho, Wo, 3, Co)
        return h[..., 0, :].float() + h[..., 2, :].float()
    ref = torch.nn.functional.silu(torch.nn.functional.group_norm(y.permute(0, 3, 1, 2).double(), 32, gw2.double(), gb2.double(), 1e-6)).permute(0, 2, 3, 1)
    assert (value(n_fused).double() - ref).abs().max().item() < 2e-5 * ref.abs().max().item()
    assert (value(n_fused) - value(n_plain)).abs().max().item() < 2e-6 * ref.abs().max().item()


def test_pair_output_epilogue_equals_the_split_pass():
    """The f16x2 convolution that writes its output directly as the next convolution's fp16-pair operand rows (a resnet's conv2 in front
    of an upsampler) against the f32 output + split_f16x2 pass it replaces: the rows bit for bit, and the decoded image bit for bit with
    the switch on and off."""
    from adv_grpo_amd import ops, synthetic
    from adv_grpo_amd.model_configs import VaeConfig
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    g = torch.Generator(device="cuda").manual_seed(21)
    B, H, W, Ci, Co = 2, 12, 20, 128, 256
    x = torch.randn(B, H, W, Ci, device="cuda", generator=g) * 3
    wt = (torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (3 * Ci ** 0.5)).half()
    bias = torch.randn(Co, device="cuda", generator=g)
    res = torch.randn(B, H, W, Co, device="cuda", generator=g) * 50
    w16 = wt.permute(0, 2, 3, 1).reshape(Co, -1).contiguous()
    a = ops.split_f16x2(x, prescale=1.0)
    y = ops.conv3x3_f16x2(a, w16, bias=bias, residual=res)
    want = ops.split_f16x2(y, prescale=2.0 ** -4).view(torch.int16).view(B, H, W, 3, Co)
    got = ops.conv3x3_f16x2_pair(a, w16, 2.0 ** -4, bias=bias, residual=res).view(torch.int16).view(B, H, W, 3, Co)
    assert torch.equal(got[:, :, :, 0], want[:, :, :, 0]) and torch.equal(got[:, :, :, 2], want[:, :, :, 2])
    cfg = VaeConfig()
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=True), cfg, "cuda", mode="bf16x3")
    lat = torch.randn(3, 16, 24, 24, device="cuda", generator=g).to(torch.bfloat16)
    dec.fused_pair_out = True
    on = dec.decode_to_image(lat)
    dec.fused_pair_out = False
    off = dec.decode_to_image(lat)
    torch.cuda.synchronize()
    assert torch.equal(on, off)


def test_decoder_reports_the_arithmetic_it_runs():
    """AutoencoderKLDecoder.arithmetic(): what bench.py prints as vae.mode_ran -- fp16-exact weights put 31 of the 33 3x3 convolutions on
    the two-product kernel (conv_in has 16 input channels, conv_out 3 output channels: three products), other weights none."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import VaeConfig
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = VaeConfig()
    a = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 4321, fp16_checkpoint=True), cfg, "cuda", mode="bf16x3").arithmetic()
    assert (a["f16x2"], a["bf16x3"], a["total"]) == (31, 2, 33) and a["text"] == "f16x2 (31/33 convs), bf16x3 (2/33)"
    b = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 4321), cfg, "cuda", mode="bf16x3").arithmetic()
    assert (b["f16x2"], b["bf16x3"]) == (0, 33) and b["text"] == "bf16x3 (33/33 convs)"
    c = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 4321), cfg, "cuda", mode="bf16").arithmetic()
    assert c["bf16"] == 33 and c["text"] == "bf16 (33/33 convs)"


def test_f16_pair_split_saturates_instead_of_overflowing():
    """The fp16-pair operand rows (f16x2 convolutions) of activations beyond the fp16 range: hi + lo reproduces the value to 22 bits
    inside the range, and is CLIPPED at +-65504 / prescale outside it -- finite, never inf / NaN (unsaturated, |s x| > 65504
    gave hi = inf, lo = NaN and a silently NaN image)."""
    from adv_grpo_amd import ops
    x = torch.tensor([[1.0, -3.5e4, 6.5e4, 7.0e4, -1.0e6, 2.0e6, 3.0e38, -3.0e38] * 8], device="cuda")
    for s in (1.0, 2.0 ** -4):
        rows = ops.split_f16x2(x.contiguous(), prescale=s).view(torch.float16).float()          # [1, 3 K]: hi | - | lo
        K = x.shape[1]
        got = (rows[:, :K] + rows[:, 2 * K:]) / s
        want = x.clamp(-65504.0 / s, 65504.0 / s)
        assert torch.isfinite(rows[:, :K]).all() and torch.isfinite(rows[:, 2 * K:]).all()
        assert ((got - want).abs() <= want.abs() * 2.0 ** -20 + 1e-30).all(), (s, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("fp16_checkpoint,single", [(True, False), (False, False), (True, True)])
def test_vae_decode_through_the_c_entry_is_bit_identical_to_the_python_sequencing(fp16_checkpoint, single):
    """advgrpo_vae_decode (csrc/vae_decode.cpp): the decoder's ~190 launches behind one C-ABI call -- the same kernels in the same order
    with the same fusions (GroupNorm sums from the producing epilogue, pair-row outputs in front of the upsamplers) as vae.py's Python chain:
    the image has the same bits, for an fp16-exact checkpoint (f16x2 kernels), a non-exact one (three products everywhere), the f16x1 opt-in,
    and through the two-stream split of a batch."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    cfg = o.VaeConfig()
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 99, fp16_checkpoint=fp16_checkpoint), cfg, "cuda", mode="bf16x3", f16_single=single)
    lat = torch.randn(3, 16, 24, 40, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).cuda()      # odd batch, non-square
    imgs = {}
    for c_entry in (True, False):
        dec.c_decode = c_entry
        imgs[c_entry] = dec.decode_to_image(lat)
        torch.cuda.synchronize()
    dec.c_decode = True
    assert imgs[True].shape == (3, 3, 192, 320) and torch.equal(imgs[True], imgs[False])
    dec.two_streams = False
    assert torch.equal(dec.decode_to_image(lat), imgs[True])
    assert torch.equal(dec.decode_to_image(lat.float()), dec.decode_to_image(lat.float()))     # f32 latents take the same entry


@pytest.mark.gpu
def test_vae_c_entry_refuses_bad_arguments_without_launching():
    """The C entry's error behaviour: a null argument, an empty descriptor and a short or misaligned workspace come back as an error code with a
    message (advgrpo_last_error), never as a launch."""
    import ctypes
    from adv_grpo_amd import _lib, synthetic
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    from oracle import vae as o
    lib = _lib.load()
    empty = _lib.VaeDecoderDesc()
    assert lib.advgrpo_vae_decode_workspace_bytes(ctypes.byref(empty)) == -1
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert lib.advgrpo_vae_decode(None, buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr(), buf.numel(), None) != 0
    assert b"null" in lib.advgrpo_last_error()
    assert lib.advgrpo_vae_decode(ctypes.byref(empty), buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr(), buf.numel(), None) != 0
    assert b"descriptor" in lib.advgrpo_last_error()
    cfg = o.VaeConfig()
    dec = AutoencoderKLDecoder(synthetic.vae_decoder_weights(cfg, 3), cfg, "cuda", mode="bf16x3")
    d = _lib.VaeDecoderDesc.from_buffer_copy(dec._c_desc())
    d.B, d.h, d.w, d.f16_single = 1, 8, 8, 0
    need = int(lib.advgrpo_vae_decode_workspace_bytes(ctypes.byref(d)))
    assert need > 0
    lat = torch.zeros(1, 16, 8, 8, dtype=torch.bfloat16, device="cuda")
    img = torch.empty(1, 3, 64, 64, dtype=torch.float32, device="cuda")
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    assert lib.advgrpo_vae_decode(ctypes.byref(d), lat.data_ptr(), 1, img.data_ptr(), ws.data_ptr(), need - 1, None) != 0      # short
    assert b"workspace" in lib.advgrpo_last_error()
    assert lib.advgrpo_vae_decode(ctypes.byref(d), lat.data_ptr(), 1, img.data_ptr(), ws.data_ptr() + 16, need, None) != 0      # misaligned
    assert b"workspace" in lib.advgrpo_last_error()


def test_conv3x3_x3_both_routes_agree():
    """The two routes out of advgrpo_conv3x3_nhwc_x3 on one problem: Cout = 128 runs the dedicated split-operand kernel, Cout = 3 (the
    first three filters of the same weights) the generic implicit-GEMM tile over the tripled contraction axis.  Each is held to the bound
    test_split_bf16x3_kernels_vs_fp32 uses, 1e-4 of the range of the float64 reference of its own output, so the two differ by at most the
    sum of the two bounds."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(21)
    B, H, W, Ci, Co = 1, 8, 8, 64, 128
    x = torch.randn(B, H, W, Ci, device="cuda", generator=g)
    wt = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) / (3 * Ci ** 0.5)
    bias = torch.randn(Co, device="cuda", generator=g)
    res = torch.randn(B, H, W, Co, device="cuda", generator=g)
    w3 = ops.split_x3(wt.permute(0, 2, 3, 1).contiguous(), order=1).reshape(Co, -1)
    x3 = ops.split_x3(x)
    wide = ops.conv3x3_x3(x3, w3, bias=bias, residual=res)
    narrow = ops.conv3x3_x3(x3, w3[:3].contiguous(), bias=bias[:3].contiguous(), residual=res[..., :3].contiguous())
    ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1) + res.double()
    scale = ref.abs().max().item()
    assert wide.shape == (B, H, W, Co) and narrow.shape == (B, H, W, 3)
    assert (wide.double() - ref).abs().max().item() < 1e-4 * scale
    scale3 = ref[..., :3].abs().max().item()
    assert (narrow.double() - ref[..., :3]).abs().max().item() < 1e-4 * scale3
    assert (wide[..., :3] - narrow).abs().max().item() < 1e-4 * (scale + scale3)
