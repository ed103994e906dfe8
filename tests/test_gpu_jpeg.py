"""GPU: the on-device JPEG encoder (csrc/jpeg.hip) byte for byte against PIL.Image.save(format="JPEG"), the sizes it leaves on
the device, the input quantisation of f32 / bf16 pixels, the jpeg_compressibility reward against the reference's numpy formula,
and a G-step epoch trained on that reward alone."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

QUALITIES = (1, 10, 50, 75, 95, 100)


def _pillow(a, q):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="JPEG", quality=q)
    return b.getvalue()


def _patterns(H, W, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 255 // max(H + W - 2, 1))], -1)
    mod = np.stack([(x * 7 + y * 3) % 256, (x * y) % 256, (x ^ y) % 256], -1)
    ff = np.where(rs.rand(H, W, 1) < 0.5, 255, rs.randint(200, 256, (H, W, 1))).repeat(3, -1)   # near-white noise: many 0xFF
    out = [rs.randint(0, 256, (H, W, 3)), ramp, mod, ff, np.full((H, W, 3), (37, 200, 91))]
    for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255), (0, 0, 0)):
        out.append(np.broadcast_to(np.array(c), (H, W, 3)))
    return np.ascontiguousarray(np.stack(out).astype(np.uint8))


def _check(batch, q):
    from adv_grpo_amd import jpeg
    got = jpeg.encode(batch, quality=q)
    want = [_pillow(a, q) for a in batch]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (batch.shape, q, i, len(g), len(w))
    sz = jpeg.sizes(batch, quality=q)
    assert sz.is_cuda and sz.dtype == torch.int64
    assert sz.cpu().tolist() == [len(w) for w in want]
    return want


@pytest.mark.parametrize("H,W", [(16, 16), (48, 32), (32, 48)])
def test_encode_matches_pillow_small(H, W):
    batch = _patterns(H, W, H * W)
    for q in QUALITIES:
        _check(batch, q)


def test_encode_matches_pillow_large_and_stuffed():
    big = _patterns(512, 512, 3)[:4]                     # noise, ramp, modular, near-white
    for q in (10, 75, 95, 100):
        want = _check(big, q)
    assert want[3].count(b"\xff\x00") > 500               # the stuffing path is exercised
    _check(_patterns(768, 512, 4)[[0, 1, 5]], 95)         # 768 x 512 (a rectangular SD resolution), mixed content
    _check(_patterns(1024, 1024, 5)[[0, 3]], 95)


def test_final_padded_byte_is_a_stuffed_ff():
    """An image whose last entropy-coded byte (after the 1-bit padding) is 0xFF: the stuffed 0x00 sits just before the EOI."""
    hits = []
    for seed in range(4000):
        a = np.random.RandomState(seed).randint(0, 256, (16, 16, 3), dtype=np.uint8)
        if _pillow(a, 75)[-4:-2] == b"\xff\x00":
            hits.append(a)
        if len(hits) == 3:
            break
    assert hits
    _check(np.stack(hits), 75)


def test_mixed_batch_of_shapes_content_and_quality_is_deterministic():
    from adv_grpo_amd import jpeg
    x = torch.rand(6, 3, 256, 384, generator=torch.Generator().manual_seed(0)).cuda()
    x[1] = x[1] * 0.02 + 0.98                                            # near-white
    x[2] = torch.linspace(0, 1, 384).cuda()                              # ramp
    a = jpeg.encode(x, quality=95)
    b = jpeg.encode(x, quality=95)
    assert a == b
    assert torch.equal(jpeg.sizes(x, 95), jpeg.sizes(x, 95))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_float_inputs_are_quantised_like_torch(dtype):
    from adv_grpo_amd import jpeg
    g = torch.Generator().manual_seed(7)
    x = torch.rand(3, 3, 64, 80, generator=g)
    k = torch.randint(0, 255, x.shape, generator=g).float()
    halves = ((k + 0.5) / 255).to(dtype).float()
    x = torch.where(torch.rand(x.shape, generator=g) < 0.5, halves, x)   # half the pixels land on (or next to) .5 after x 255
    x[0, :, :8] = -0.25                                                   # clamped below
    x[0, :, 8:16] = 1.5                                                   # clamped above
    x = x.to(dtype).cuda()
    prod = (x * 255)
    assert ((prod.float() - prod.float().floor()) == 0.5).sum() > 100    # the tie-breaking case is exercised
    u8 = (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()   # rewards.py:15-17
    host = u8.cpu().numpy()
    for q in (75, 95):
        want = [_pillow(a, q) for a in host]
        assert jpeg.encode(x, quality=q) == want
        assert jpeg.encode(u8, quality=q) == want                         # device uint8 NHWC
        assert jpeg.sizes(host, quality=q).cpu().tolist() == [len(w) for w in want]   # host ndarray (the reference's branch)


def test_jpeg_compressibility_reward_is_bit_equal_to_the_reference_formula():
    from adv_grpo_amd import rewards
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).cuda()
    x[1] = 0.5
    host = (x * 255).round().clamp(0, 255).to(torch.uint8).cpu().numpy().transpose(0, 2, 3, 1)
    ref_inc = np.array([len(_pillow(a, 95)) / 1000 for a in host])          # rewards.py:15-23
    ref = -ref_inc / 500                                                    # rewards.py:31-33
    det, meta = rewards.multi_score("cuda", {"jpeg_compressibility": 1})(x, ["p"] * 4, [{}] * 4)
    got = det["jpeg_compressibility"]
    assert meta == {} and got.is_cuda and got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(det["avg"].cpu().numpy(), 1 * ref)
    toy = torch.tensor([0.25, -1.5, 3.0, 0.125], dtype=torch.float32, device="cuda")
    saved = dict(rewards.score_functions)
    try:
        rewards.register_scorer("toy", lambda: (lambda images, prompts, metadata: (toy, {})))
        det, _ = rewards.multi_score("cuda", {"jpeg_compressibility": 2, "toy": 0.5})(x, ["p"] * 4, [{}] * 4)
    finally:
        rewards.score_functions.clear()
        rewards.score_functions.update(saved)
    want = 2 * ref + (0.5 * toy.cpu().numpy()).astype(np.float64)
    assert np.array_equal(det["avg"].cpu().numpy(), want)


def test_refused_calls_launch_nothing():
    from adv_grpo_amd import _lib
    lib = _lib.load()
    N, H, W = 2, 32, 48
    x = torch.rand(N, 3, H, W, device="cuda")
    wsb = lib.advgrpo_jpeg_workspace_bytes(N, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    sizes = torch.full((N,), -7, dtype=torch.int64, device="cuda")
    stride = lib.advgrpo_jpeg_max_file_bytes(H, W)
    files = torch.full((N, stride), 0xAB, dtype=torch.uint8, device="cuda")
    base = [x.data_ptr(), _lib.F32, _lib.JPEG_NCHW, N, H, W, 95, sizes.data_ptr(), files.data_ptr(), stride, ws.data_ptr(), wsb,
            _lib.stream_ptr()]
    for i, v in ((4, 40), (5, 24), (3, 0), (6, 0), (6, 101), (1, _lib.F64), (2, 5), (0, None), (7, None), (10, None),
                 (11, wsb - 1), (10, ws.data_ptr() + 8), (9, stride - 1)):
        a = list(base)
        a[i] = v
        assert lib.advgrpo_jpeg_encode(*a) < 0 and lib.advgrpo_last_error().decode().startswith("jpeg_encode")
    torch.cuda.synchronize()
    assert (sizes == -7).all() and (files == 0xAB).all()
    _lib.check(lib.advgrpo_jpeg_encode(*base))
    torch.cuda.synchronize()
    assert (sizes > 623).all() and files[:, :2].cpu().tolist() == [[0xFF, 0xD8]] * N


def test_g_step_epoch_on_the_compressibility_reward():
    """The GRPO sanity check the issue names: reward_fn = {jpeg_compressibility: 1}, no scorer weights at all."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.mmdit_train import SD3TransformerLoRA
    from adv_grpo_amd.model_configs import MMDiTConfig, VaeConfig
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.trainer import SyntheticData, Trainer
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
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
    assert r.shape == (2 * 2,) and torch.isfinite(r).all() and (r < 0).all()
    info = tr_.run_epoch()
    assert info["phase"] == "G" and not torch.equal(model.params, p0) and torch.isfinite(model.params).all()
