"""GPU: the aesthetic and clipscore rewards -- the torchvision preprocessing kernel against torch's own GPU F.interpolate, the aesthetic
head kernel against float64, the CLIP towers with quick_gelu against the oracle, both rewards against the reference's own outputs
(tests/golden/clip_rewards.npz, tests/golden/make_golden_clip_rewards.py) and one G-step epoch on the aesthetic reward."""
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import siglip_reference

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_rewards.npz")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _tv_reference(x, size=224):
    """torchvision's tensor path on the GPU: T.Resize(size) (non-f32/f64 images are cast to f32 around F.interpolate and back; an image
    already at the output size is returned as is), T.CenterCrop(size), T.Normalize (sub then div, mean / std in the image's dtype)."""
    from adv_grpo_amd import preprocess
    dt = x.dtype
    H, W = x.shape[-2:]
    RH, RW, top, left = preprocess.tv_resize_geometry(H, W, size)
    if (RH, RW) != (H, W):
        y = F.interpolate(x.float() if dt not in (torch.float32, torch.float64) else x, size=(RH, RW), mode="bilinear",
                          align_corners=False, antialias=True).to(dt)
    else:
        y = x
    y = y[..., top:top + size, left:left + size]
    m = torch.tensor(preprocess.CLIP_MEAN, dtype=dt, device=x.device).view(-1, 1, 1)
    s = torch.tensor(preprocess.CLIP_STD, dtype=dt, device=x.device).view(-1, 1, 1)
    return (y - m) / s


def _rows(v, size=224):
    """[B,3,S,S] -> [B*(S/14)^2, 640] im2col rows (588 real columns, zero pad), in v's dtype."""
    B, g = v.shape[0], size // 14
    r = v.reshape(B, 3, g, 14, g, 14).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 588)
    return torch.cat([r, torch.zeros(r.shape[0], 52, dtype=r.dtype, device=r.device)], 1)


SIZES = [(512, 512), (1024, 1024), (300, 500), (500, 300), (224, 224), (150, 150)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", SIZES)
def test_tv_preprocess_is_bit_equal_to_torch_gpu(H, W, dt):
    from adv_grpo_amd import preprocess
    g = torch.Generator(device="cuda").manual_seed(H * 7 + W)
    x = torch.rand(2, 3, H, W, generator=g, device="cuda").to(dt)
    ref = _rows(_tv_reference(x))
    got = preprocess.tv_clip_patches(x)
    assert got.dtype == torch.bfloat16 and got.shape == (2 * 256, 640)
    n = (got.float() != ref.to(torch.bfloat16).float()).sum().item()
    assert n == 0, f"{n} of {got.numel()} patch values differ from torch's GPU resize + crop + normalise"
    if dt == torch.float32:                                     # the split-bf16 layout of vit_x3 holds exactly those f32 values
        hi = ref.to(torch.bfloat16)
        lo = (ref - hi.float()).to(torch.bfloat16)
        assert torch.equal(preprocess.tv_clip_patches(x, x3=True), torch.cat([hi, hi, lo], 1))


@pytest.mark.parametrize("H,W", [(300, 500), (512, 512)])
def test_tv_preprocess_uint8_follows_the_ndarray_path(H, W):
    """rewards.py:59-61: an NHWC uint8 array becomes torch.tensor(u8) / 255.0 (a true f32 division) before the transform."""
    from adv_grpo_amd import preprocess
    g = torch.Generator().manual_seed(H + W)
    u8 = torch.randint(0, 256, (2, 3, H, W), generator=g, dtype=torch.uint8)
    ref = _rows(_tv_reference((u8 / 255.0).cuda()))
    got = preprocess.tv_clip_patches(u8.cuda())
    assert torch.equal(got, ref.to(torch.bfloat16))


def _head64(e, head):
    """Float64 reference of the aesthetic head, plus a rigorous bound on the kernel's f32 error.
    gamma_n = n u / (1 - n u), u = 2^-24.  Normalisation: the f32 sum of D squares has relative error <= gamma_D, its square root halves
    that and adds u, the division adds u: |e^_k - e_k / |e|| <= (gamma_D / 2 + 2 u (1 + ...)) |e_k / |e||, taken as gamma_{D/2 + 3}.
    Layer y = W x + b with K inputs (each lane's fused chain plus the 6-level wave tree plus the bias add is at most K + 1 roundings per
    term): |y^ - y| <= |W| d + gamma_{K+1} (|W| (|x| + d) + |b|), d the bound on x's error."""
    from adv_grpo_amd.synthetic import AESTHETIC_HEAD_LAYERS
    u = 2.0 ** -24
    gam = lambda n: n * u / (1 - n * u)
    e = e.double()
    x = e / e.norm(dim=-1, keepdim=True)
    d = gam(e.shape[1] // 2 + 3) * x.abs()
    for i in AESTHETIC_HEAD_LAYERS:
        W, b = head[f"layers.{i}.weight"].double(), head[f"layers.{i}.bias"].double()
        K = W.shape[1]
        d = d @ W.abs().T + gam(K + 1) * ((x.abs() + d) @ W.abs().T + b.abs())
        x = x @ W.T + b
    return x[:, 0], d[:, 0]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_aesthetic_head_vs_float64_repeatable_and_batch_independent(dt):
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.aesthetic_scorer import aesthetic_head
    head = {k: v.cuda() for k, v in synthetic.aesthetic_head_weights(5).items()}
    N = 37                                                      # not a multiple of the 4 rows of a workgroup
    e = (torch.randn(N, 768, generator=torch.Generator().manual_seed(6)) * 0.3 + 0.05).to(dt).cuda()
    got = aesthetic_head(e, head)
    ref, bound = _head64(e.float(), head)
    err = (got.double() - ref).abs()
    print(f"aesthetic head {dt}: max |err| {err.max().item():.3e}, worst err / bound {(err / bound).max().item():.3f}, "
          f"scores in [{ref.min().item():.3f}, {ref.max().item():.3f}]")
    assert got.dtype == torch.float32 and got.shape == (N,)
    assert (err <= bound).all()
    assert ref.std().item() > 0.05                              # the scores spread: the bound is not met by a constant
    assert torch.equal(aesthetic_head(e, head), got)            # bit-repeatable
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(7)).cuda()
    assert torch.equal(aesthetic_head(e[perm], head), got[perm])                      # position in the batch does not matter
    alone = torch.cat([aesthetic_head(e[i:i + 1], head) for i in range(N)])
    assert torch.equal(alone, got)                                                    # nor does the batch size


def _golden():
    z = np.load(GOLDEN)
    from adv_grpo_amd.model_configs import ClipConfig
    cfg = ClipConfig(act="quick_gelu", **{k[4:]: int(z[k]) for k in z.files if k.startswith("cfg_")})
    return z, cfg


def test_clip_towers_honour_quick_gelu_vs_oracle():
    """CLIP ViT-L/14's activation: vit.CLIPModel used to run GELU whatever the config said.  At the golden's small quick_gelu config the
    bf16 tower must sit within 2e-2 (test_gpu_vit.py's bound for the bf16 towers) of the quick_gelu oracle AND clearly nearer to it than
    to the GELU oracle; the fp32-equivalent tower within 5e-5 (the ViT-H bound of test_gpu_vit.py)."""
    import dataclasses
    from adv_grpo_amd import synthetic, vit, vit_x3
    from oracle import vit as o
    z, cfg = _golden()
    ocfg = o.ClipConfig(**dataclasses.asdict(cfg))
    W = synthetic.clip_weights(cfg, int(z["seed"]))
    ids = torch.from_numpy(z["input_ids"])
    px = _tv_reference(siglip_reference.structured_images(4, 300, 3).cuda())
    Wb = {k: v.to(torch.bfloat16) for k, v in W.items()}
    Wb32 = {k: v.float().cuda() for k, v in Wb.items()}                     # the bf16 tower's weights and pixels, in f32
    pxb = px.to(torch.bfloat16).float()
    ri, rt = o.clip_image_features(Wb32, ocfg, pxb), o.clip_text_features(Wb32, ocfg, ids.cuda())
    gelu = dataclasses.replace(ocfg, act="gelu")
    gi, gt = o.clip_image_features(Wb32, gelu, pxb), o.clip_text_features(Wb32, gelu, ids.cuda())
    m = vit.CLIPModel(Wb, cfg, "cuda")
    ie = m.get_image_features(pixel_patches=_rows(px).to(torch.bfloat16))
    te = m.get_text_features(ids)
    print(f"bf16 tower: image {_rel(ie, ri):.2e} (gelu oracle {_rel(gi, ri):.2e}), text {_rel(te, rt):.2e} (gelu oracle {_rel(gt, rt):.2e})")
    assert _rel(ie, ri) < 2e-2 and _rel(te, rt) < 2e-2
    # bf16 noise (~5e-3) is of the size of the GELU / quick_gelu gap (~7e-3): the tower must be clearly nearer the quick_gelu oracle than
    # the GELU one (measured ratios ~0.6; a GELU tower gives > 1)
    print(f"bf16 tower vs the GELU oracle: image {_rel(ie, gi):.2e}, text {_rel(te, gt):.2e}")
    assert _rel(ie, ri) < 0.8 * _rel(ie, gi) and _rel(te, rt) < 0.8 * _rel(te, gt)
    W32 = {k: v.float().cuda() for k, v in W.items()}
    ri, rt = o.clip_image_features(W32, ocfg, px), o.clip_text_features(W32, ocfg, ids.cuda())
    m3 = vit_x3.CLIPModelX3(W, cfg, "cuda")
    r = _rows(px)
    hi = r.to(torch.bfloat16)
    ie3 = m3.get_image_features(pixel_patches3=torch.cat([hi, hi, (r - hi.float()).to(torch.bfloat16)], 1))
    te3 = m3.get_text_features(ids)
    print(f"x3 tower: image {_rel(ie3, ri):.2e}, text {_rel(te3, rt):.2e}")
    assert _rel(ie3, ri) < 5e-5 and _rel(te3, rt) < 5e-5


def _golden_setup(dtype=torch.float32):
    from adv_grpo_amd import rewards, synthetic, vit, vit_x3
    z, cfg = _golden()
    W = synthetic.clip_weights(cfg, int(z["seed"]))
    model = vit_x3.CLIPModelX3(W, cfg, "cuda") if dtype == torch.float32 else \
        vit.CLIPModel({k: v.to(torch.bfloat16) for k, v in W.items()}, cfg, "cuda")
    rewards.configure_aesthetic(model, synthetic.aesthetic_head_weights(int(z["head_seed"])))
    rewards.configure_clip(model)
    a = siglip_reference.structured_images(int(z["aes_images_n"]), int(z["aes_images_size"]), int(z["aes_images_seed"]))
    c = siglip_reference.structured_images(int(z["clip_images_n"]), int(z["clip_images_size"]),
                                           int(z["clip_images_seed"]))[..., :int(z["clip_images_width"])].contiguous()
    for t, key in ((a, "aesthetic_images_sha256"), (c, "clip_images_sha256")):
        assert hashlib.sha256(t.numpy().tobytes()).hexdigest() == str(z[key]), "the structured test images are not the golden's"
    prompts = rewards.PromptBatch([f"prompt {i}" for i in range(len(c))], clip_ids=torch.from_numpy(z["input_ids"]).cuda())
    return z, a.cuda(), c.cuda(), prompts


def test_aesthetic_and_clipscore_match_the_reference():
    """multi_score on f32 device images against the reference's own scorers (fp32 transformers CLIPModel on the CPU).  aesthetic: the same
    uint8 pixels (the Pillow-exact path), then towers that agree to ~1e-5 relative: held to 2e-3.  clipscore: the GPU resize differs
    from the CPU one the golden ran in the last f32 bits only; 100 / 30 times a cosine: held to 2e-3.  All-zero images miss by > 0.1."""
    from adv_grpo_amd import rewards
    z, a, c, prompts = _golden_setup()
    det, _ = rewards.multi_score("cuda", {"aesthetic": 1})(a, prompts, [{}] * len(a))
    got = det["aesthetic"]
    assert got.is_cuda and got.dtype == torch.float32
    ea = np.abs(got.cpu().numpy() - z["aesthetic"]).max()
    zero_a = rewards.multi_score("cuda", {"aesthetic": 1})(torch.zeros_like(a), prompts, [{}] * len(a))[0]["aesthetic"]
    na = np.abs(zero_a.cpu().numpy() - z["aesthetic"]).max()
    assert np.abs(zero_a.cpu().numpy() - z["aesthetic_zero"]).max() < 2e-3
    det, _ = rewards.multi_score("cuda", {"clipscore": 1})(c, prompts, [{}] * len(c))
    got_c = det["clipscore"]
    assert got_c.is_cuda and got_c.dtype == torch.float32
    ec = np.abs(got_c.cpu().numpy() - z["clipscore"]).max()
    zero_c = rewards.multi_score("cuda", {"clipscore": 1})(torch.zeros_like(c), prompts, [{}] * len(c))[0]["clipscore"]
    nc = np.abs(zero_c.cpu().numpy() - z["clipscore"]).max()
    print(f"aesthetic: max |err| {ea:.2e} (zeros: {na:.3f});  clipscore: max |err| {ec:.2e} (zeros: {nc:.3f})")
    assert ea < 2e-3 and ec < 2e-3
    assert na > 0.1 and nc > 0.1


def test_bf16_scorers_track_the_reference():
    """The bf16 towers (compute_dtype "bf16") on the same inputs: bf16 products over two layers, held to 5e-2 on scores of O(1)."""
    from adv_grpo_amd import rewards
    z, a, c, prompts = _golden_setup(torch.bfloat16)
    sa = rewards.aesthetic_score()(a.to(torch.bfloat16), prompts, None)[0]
    sc = rewards.clip_score()(c.to(torch.bfloat16), prompts, None)[0]
    print("bf16 aesthetic err", np.abs(sa.cpu().numpy() - z["aesthetic"]).max(), "clipscore err", np.abs(sc.cpu().numpy() - z["clipscore"]).max())
    assert np.abs(sa.cpu().numpy() - z["aesthetic"]).max() < 5e-2
    assert np.abs(sc.cpu().numpy() - z["clipscore"]).max() < 5e-2


def test_aesthetic_refuses_non_square_images():
    from adv_grpo_amd import rewards
    _golden_setup()
    with pytest.raises(ValueError, match="square"):
        rewards.aesthetic_score()(torch.rand(2, 3, 256, 300, device="cuda"), None, None)


def test_g_step_epoch_on_the_aesthetic_reward():
    """reward_fn = {aesthetic: 1} with small synthetic CLIP-L weights: one sampled epoch scores finite rewards and trains."""
    from adv_grpo_amd import rewards, synthetic, vit_x3
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.mmdit_train import SD3TransformerLoRA
    from adv_grpo_amd.model_configs import ClipConfig, MMDiTConfig, VaeConfig
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.trainer import SyntheticData, Trainer
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    z, ccfg = _golden()
    rewards.configure_aesthetic(vit_x3.CLIPModelX3(synthetic.clip_weights(ccfg, 9), ccfg, "cuda"), synthetic.aesthetic_head_weights(10))
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"aesthetic": 1}
    cfg.resolution = 256
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.num_batches_per_epoch = 2
    cfg.train.gradient_accumulation_steps = 1
    mcfg = MMDiTConfig(num_layers=2, num_heads=4, joint_attention_dim=256, pooled_projection_dim=128,
                       pos_embed_max_size=96, dual_attention_layers=(0,))
    model = SD3TransformerLoRA({k: v.to(torch.bfloat16) for k, v in synthetic.mmdit_weights(mcfg, 1).items()}, mcfg, "cuda")
    vae = AutoencoderKLDecoder({k: v.to(torch.bfloat16) for k, v in synthetic.vae_decoder_weights(VaeConfig(), 2).items()},
                               VaeConfig(), "cuda")
    data = SyntheticData(n_prompts=100, n_tokens=21, ctx_dim=256, pooled_dim=128, resolution=256)
    tr_ = Trainer(cfg, SD3Pipeline(model, vae, "cuda"), data, None, None)
    p0 = model.params.clone()
    s = tr_.sample_epoch()
    r = s["rewards"]
    assert r.shape == (2 * 2,) and torch.isfinite(r).all()
    advs, update = [], tr_.stat_tracker.update
    tr_.stat_tracker.update = lambda *a, **k: advs.append(update(*a, **k)) or advs[-1]        # the advantages of the epoch
    info = tr_.run_epoch()
    assert len(advs) == 1 and torch.isfinite(advs[0]).all() and advs[0].abs().max().item() > 0
    assert info["phase"] == "G" and not torch.equal(model.params, p0) and torch.isfinite(model.params).all()
