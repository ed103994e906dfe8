"""GPU: the siglip_image_similarity reward -- the head-dim-72 attention, the C encoder entry at head dim 72, the SigLIP preprocessing,
the full so400m tower and attention-pooling head against the float reference (tests/siglip_reference.py), the scorer against the
reference's own outputs (tests/golden/siglip_similarity.npz, tests/golden/make_golden_siglip.py) and Trainer.evaluate."""
import os

import numpy as np
import pytest
import torch

import siglip_reference

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.mark.parametrize("B,H,Sq,Skv,q_bs0", [(1, 16, 729, 729, False), (2, 16, 729, 729, False), (2, 16, 100, 729, False),
                                              (1, 1, 17, 33, False), (3, 16, 1, 729, True)])
def test_attention_head_dim_72_vs_fp32(B, H, Sq, Skv, q_bs0):
    from adv_grpo_amd import ops
    hd, D = 72, H * 72
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 10 + Sq)
    kv = torch.randn(B, Skv, 3 * D, generator=g, device="cuda").to(torch.bfloat16)           # packed q | k | v rows, read in place
    k, v = kv[:, :, D:2 * D], kv[:, :, 2 * D:]
    if q_bs0:                                                   # the pooling head's single probe query, shared by the batch
        q = torch.randn(1, 1, D, generator=g, device="cuda").to(torch.bfloat16).expand(B, 1, D)
        assert q.stride(0) == 0
    else:
        q = torch.randn(B, Sq, 3 * D, generator=g, device="cuda").to(torch.bfloat16)[:, :, :D]
    ldo = D + 24
    sentinel = -123.0
    outs = []
    for _ in range(2):
        buf = torch.full((B, Sq, ldo), sentinel, dtype=torch.bfloat16, device="cuda")
        ops.attention(q, k, v, H, out=buf[:, :, :D])
        outs.append(buf)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])                        # bitwise repeatable
    buf = outs[0]
    assert (buf[:, :, D:] == sentinel).all()                    # nothing written past the last head
    sp = lambda t: t.float().reshape(B, t.shape[1], H, hd).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / hd ** 0.5, dim=-1)
    ref = (p @ sp(v)).transpose(1, 2)                           # [B, Sq, H, hd]
    bound = (p @ sp(v).abs()).transpose(1, 2)                   # sum_k p_k |v_k|
    got = buf[:, :, :D].float().view(B, Sq, H, hd)
    # the kernel rounds each probability to bf16 before the PV product (relative error <= 2^-9 per term, so <= 2^-9 sum_k p_k |v_k|
    # on the sum; the normaliser uses the unrounded sum) and rounds the output to bf16 (<= 2^-9 |o|); scores, exp2 and the f32
    # sums add a few f32 ulp.  A factor 2 covers the f32 terms; each head is checked in its own 72 columns.
    tol = 2.0 * 2.0 ** -9 * (bound + ref.abs()) + 1e-6
    err = (got - ref).abs()
    print(f"hd72 attention {B, H, Sq, Skv}: max |err| {err.max().item():.3e}, worst err / tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all()


def _layers(D, F, n, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev, torch.bfloat16)
    return [{"ln1.w": 1 + r(D, sc=0.1), "ln1.b": r(D, sc=0.1), "ln2.w": 1 + r(D, sc=0.1), "ln2.b": r(D, sc=0.1),
             "qkv.w": r(3 * D, D, sc=D ** -0.5), "qkv.b": r(3 * D, sc=0.1), "out.w": r(D, D, sc=D ** -0.5), "out.b": r(D, sc=0.1),
             "fc1.w": r(F, D, sc=D ** -0.5), "fc1.b": r(F, sc=0.1), "fc2.w": r(D, F, sc=F ** -0.5), "fc2.b": r(D, sc=0.1)}
            for _ in range(n)]


def test_vit_c_entry_at_head_dim_72_is_bit_identical_to_the_python_sequencing():
    from adv_grpo_amd import vit
    B, S, D, H, F = 2, 729, 576, 8, 4352
    enc = vit._Encoder(_layers(D, F, 2, 21), H, 1e-6, "gelu_tanh")
    x0 = torch.randn(B * S, D, generator=torch.Generator().manual_seed(22)).to("cuda", torch.bfloat16)
    outs = {}
    for c_stack in (True, False):
        vit._Encoder.c_stack = c_stack
        try:
            outs[c_stack] = enc(x0.clone(), B, S)
        finally:
            vit._Encoder.c_stack = True
    assert torch.isfinite(outs[True].float()).all() and not torch.equal(outs[True], x0)
    assert torch.equal(outs[True], outs[False])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32, torch.uint8])
@pytest.mark.parametrize("size", [512, 200, 96])
def test_siglip_preprocess_matches_the_reference_expression(dt, size):
    from adv_grpo_amd import preprocess
    g = torch.Generator().manual_seed(size)
    img = torch.randint(0, 256, (2, 3, size, size), generator=g, dtype=torch.uint8) if dt == torch.uint8 else \
        torch.rand(2, 3, size, size, generator=g).to(dt)
    img = img.cuda()
    got = preprocess.siglip_patches(img, 384)
    ref = siglip_reference.patch_rows(siglip_reference.preprocess(img, 384))
    assert got.shape == (2 * 729, 640) and (got[:, 588:] == 0).all()
    err = (got.float() - ref.float()).abs()
    # Not bit-exact: the kernel evaluates torch's bicubic tap formulas but its f32 sums (order, fma contraction) round differently from
    # torch's build, as in the DINO kernel it shares the body with (tests/test_gpu_vit.py).  Where an f32 resize value straddles a bf16
    # rounding boundary -- of the bf16 resize result (bf16 inputs) or of the final normalised pixel -- the pixel lands one bf16 ulp
    # away: one ulp of the resize result (|x| < 1.25 after bicubic overshoot: <= 2^-8) doubles under / 0.5 and can carry one more final
    # ulp (|y| < 1.5: 2^-7), so <= 2^-6.  Measured on these inputs: at most 5.8e-5 of the pixels (deterministic); bound 1e-4.
    frac = (err > 0).float().mean().item()
    print(f"siglip preprocess {dt} {size}: mismatch fraction {frac:.2e}, max {err.max().item():.3e}")
    assert err.max().item() <= 2.0 ** -6 and frac <= 1e-4


def _bf_sd(sd, dev="cuda"):
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


def test_siglip_so400m_full_depth_tower_vs_float_reference():
    """27 layers of 16 x 72, 729 tokens, the pooling head: pooler_output against the f32 reference on the same bf16 weights."""
    from adv_grpo_amd import synthetic, vit
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    cfg = SiglipVisionConfig()
    Wb = _bf_sd(synthetic.siglip_weights(cfg, 6))
    model = vit.SiglipVision(Wb, cfg, "cuda")
    px = torch.randn(2, 3, 384, 384, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    got = model.pooler_output(pixel_patches=siglip_reference.patch_rows(px).contiguous())
    W32 = {k: v.float().cuda() for k, v in Wb.items()}
    with torch.no_grad():
        want = siglip_reference.pooler_output(W32, cfg, px.float())
    # bf16 activations between every GEMM / attention / norm (the reference is f32 throughout): each rounding is <= 2^-9 relative and
    # 27 residual layers accumulate them about like CLIP ViT-H's 32 (tests/test_gpu_vit.py bounds that tower at 3e-2)
    print("SigLIP so400m 27 layers + pooling head, bf16 vs f32 reference:", _rel(got, want))
    assert got.shape == (2, 1152) and got.dtype == torch.bfloat16
    assert _rel(got, want) < 3e-2


def _small_model():
    from adv_grpo_amd import synthetic, vit
    from adv_grpo_amd.model_configs import SiglipVisionConfig
    z = np.load(os.path.join(HERE, "golden", "siglip_similarity.npz"))
    cfg = SiglipVisionConfig(hidden=int(z["hidden"]), layers=int(z["layers"]), heads=int(z["heads"]), mlp=int(z["mlp"]),
                             image_size=int(z["image_size"]))
    sd = synthetic.siglip_weights(cfg, int(z["seed"]))                  # the CPU generator, as the golden script drew them
    return vit.SiglipVision(_bf_sd(sd), cfg, "cuda"), sd, cfg, z


# Tolerance of the scorer tests on the cosine matrix.  The reference rounds its normalised embeddings and the [N, M] matrix to bf16: at
# cosines below 1 that is <= 2^-9 each, <= 3 * 2^-9 = 5.9e-3 together; the towers round bf16 activations at other points (fused GEMM
# epilogues here), which moves a unit embedding by a few 1e-3 on this 2-layer tower (the f32 float reference is 2.5e-3 from the
# golden).  1e-2 covers both and is ~90x below what a scorer that ignores its input would show: the golden's cosines spread from
# 0.09 to 0.99, and all-zero images are 0.91 away from them (checked below).
SCORE_TOL = 1e-2


def test_siglip_image_similarity_reproduces_the_reference_golden():
    from adv_grpo_amd import rewards
    model, _, _, z = _small_model()
    golden = torch.from_numpy(z["pairwise"])
    assert golden.max() - golden.min() > 50 * SCORE_TOL           # the golden discriminates its images
    rewards.configure_siglip(model)
    try:
        fn = rewards.multi_score("cuda", {"siglip_image_similarity": 1})
        imgs, refs = torch.from_numpy(z["images"]).cuda(), torch.from_numpy(z["ref_images"]).cuda()
        details, _ = fn(imgs, None, None, ref_images=refs)
        _, info = rewards.siglip_image_similarity_score("cuda")(imgs, refs)
        _, blind = rewards.siglip_image_similarity_score("cuda")(torch.zeros_like(imgs), torch.zeros_like(refs))
    finally:
        rewards.configure_siglip(None)
    s = details["siglip_image_similarity"]
    pair_err = (info["pairwise"].cpu() - golden).abs().max().item()
    score_err = (s.cpu() - torch.from_numpy(z["scores"])).abs().max().item()
    blind_err = (blind["pairwise"].cpu() - golden).abs().max().item()
    print(f"siglip golden: max |pairwise diff| {pair_err:.3e}, max |score diff| {score_err:.3e}; all-zero images {blind_err:.3f}")
    assert s.shape == (3,) and s.dtype == torch.float32 and torch.equal(details["avg"], s)
    assert pair_err <= SCORE_TOL and score_err <= SCORE_TOL
    assert blind_err > 50 * SCORE_TOL                               # a scorer blind to its input fails this test


def test_siglip_image_similarity_on_bf16_inputs_vs_the_reference_expression():
    """bf16 generated images (as Trainer.evaluate passes them) and uint8-range f32 NHWC references against the reference expression
    (torch's GPU resize, the reference's rounding points) feeding the f32 float tower on the same bf16 weights.  The rounding points of
    the preprocessing themselves are pinned pixel by pixel in test_siglip_preprocess_matches_the_reference_expression."""
    from adv_grpo_amd import rewards
    model, sd, cfg, _ = _small_model()
    imgs = siglip_reference.structured_images(3, 512, 5).to(torch.bfloat16).cuda()
    refs = (siglip_reference.structured_images(2, 512, 6) * 255).permute(0, 2, 3, 1).contiguous().cuda()    # NHWC, 0..255
    rewards.configure_siglip(model)
    try:
        s, info = rewards.siglip_image_similarity_score("cuda")(imgs, refs)
    finally:
        rewards.configure_siglip(None)
    W32 = {k: v.to(torch.bfloat16).float().cuda() for k, v in sd.items()}

    def emb(x):
        with torch.no_grad():
            e = siglip_reference.pooler_output(W32, cfg, siglip_reference.preprocess(x, cfg.image_size).float())
        return e / e.norm(dim=-1, keepdim=True)
    pair = emb(imgs) @ emb(refs.permute(0, 3, 1, 2)).T
    err = (info["pairwise"] - pair).abs().max().item()
    print(f"siglip bf16 inputs: expected cosines {pair.min().item():.3f} .. {pair.max().item():.3f}, max |pairwise diff| {err:.3e}")
    assert pair.max() - pair.min() > 20 * SCORE_TOL
    assert info["pairwise"].shape == (3, 2) and (s - info["pairwise"].max(dim=1).values).abs().max().item() == 0
    assert err <= SCORE_TOL          # SCORE_TOL less the reference's bf16 roundings: the bf16 tower against the f32 one


def test_trainer_evaluate_reports_siglip_image_similarity():
    from adv_grpo_amd import rewards, synthetic, vit
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.mmdit_train import SD3TransformerLoRA
    from adv_grpo_amd.model_configs import ClipConfig, MMDiTConfig, SiglipVisionConfig, VaeConfig
    from adv_grpo_amd.pickscore_scorer import PickScoreScorer
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.trainer import SyntheticData, Trainer
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = get_config("pickscore_cotrain_sd3_fast", gpu_number=1)
    cfg.resolution = 256
    cfg.sample.num_steps = 4
    cfg.sample.eval_num_steps = 4
    cfg.sample.test_batch_size = 2
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    mcfg = MMDiTConfig(num_layers=2, num_heads=4, joint_attention_dim=256, pooled_projection_dim=128, pos_embed_max_size=96,
                       dual_attention_layers=(0,))
    tr = SD3TransformerLoRA({k: v.to(torch.bfloat16) for k, v in synthetic.mmdit_weights(mcfg, 1).items()}, mcfg, "cuda")
    vae = AutoencoderKLDecoder({k: v.to(torch.bfloat16) for k, v in synthetic.vae_decoder_weights(VaeConfig(), 2).items()},
                               VaeConfig(), "cuda")
    cc = ClipConfig(v_layers=2, t_layers=2)
    scorer = PickScoreScorer("cuda", dtype=torch.bfloat16, model_sd=synthetic.clip_weights(cc, 4), clip_cfg=cc)
    data = SyntheticData(n_prompts=100, n_tokens=21, ctx_dim=256, pooled_dim=128, resolution=256)
    trainer = Trainer(cfg, SD3Pipeline(tr, vae, "cuda"), data, scorer, None)
    scfg = SiglipVisionConfig(hidden=576, layers=2, heads=8)
    rewards.configure_siglip(vit.SiglipVision(_bf_sd(synthetic.siglip_weights(scfg, 8)), scfg, "cuda"))
    try:
        ev = trainer.evaluate(n_prompts=2, eval_reward_fn={"siglip_image_similarity": 1})
    finally:
        rewards.configure_siglip(None)
    v = ev["eval_reward_siglip_image_similarity"]
    assert np.isfinite(float(v)) and -1.0 <= float(v) <= 1.0 + 1e-3, ev
