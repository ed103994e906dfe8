"""GPU: advgrpo_qwen_cfg_euler_step (Qwen-Image's norm-rescaled true-CFG combine + the Euler step, one launch) against the torch
restatement tests/qwen_sampler_reference.py run on the same device, and QwenImageSampler end to end on a tiny synthetic Qwen-Image.

Bounds of the kernel cases.  The kernel adds a token's 64 squares in another (fixed) order than torch.norm, so a token's bf16 norm
can round the other way: at most 1 % of the tokens of a case (tests/test_qwen_sampler_host.py measures the share on these very
inputs: 0) may differ from the restatement at all, every other token is bit-identical.  Inside a differing token an element must be
within 2 bf16 ulp; with f32 predictions (no bf16 rounding point in the step) every element is within 4 f32 ulp.  The ulp is taken at
the element's magnitude in the step's last operation, prev = sample + dt * out: the largest of |prev|, |sample| and |dt * out| (the
result alone would not do: where the two operands cancel, the rounding of the larger operand is all that is left of it).  A bf16
`sample` adds the final cast: two f32 sums within 4 f32 ulp of each other become the same bf16 value or, where a rounding boundary
lies between them (8 f32 ulp out of a bf16 ulp's 65536: about 1 element in 10^4), neighbouring ones -- those cases ask for at most
one bf16 ulp, on at most 1 % of the elements.

Measured on one MI355X: bf16 predictions 0 differing tokens in all 24 cases; f32 predictions and latents worst element 2 - 4 f32 ulp
(4.000 at (3,16,64,64): at the bound); f32 predictions with bf16 latents at most 5e-6 of the elements differing."""
import pytest
import torch

import qwen_sampler_reference as R

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
STEP = 10            # of the 50-step table of a 512 x 512 image: sigma 0.871 -> 0.857


def _sigmas():
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler
    sch = QwenImageFlowMatchScheduler()
    sch.set_timesteps(50, 1024, device="cuda")
    return sch.sigmas


def _ulp(x, bits):
    """Spacing at |x| of a format with `bits` explicit mantissa bits (7: bf16, 23: f32)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -126))) - bits)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _run(neg, pos, x, sig, out=None):
    from adv_grpo_amd import qwen_generate as Q
    got = Q.cfg_euler_step(neg, pos, x, sig, STEP, R.SCALE, out=out)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name,shape,vd,xd,mult,seed", R.cases(), ids=[c[0] for c in R.cases()])
def test_kernel_against_the_restatement(name, shape, vd, xd, mult, seed):
    sig = _sigmas()
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, vd, xd, mult, seed))
    got = _run(neg, pos, x, sig)
    ref = R.cfg_euler_step(neg, pos, x, sig[STEP], sig[STEP + 1])
    assert got.dtype == xd and got.shape == ref.shape and torch.isfinite(got.float()).all()
    again = _run(neg, pos, x, sig)
    assert torch.equal(_bits(got), _bits(again))                          # fixed reduction order: run to run the same bits
    same = (R.pack(_bits(got)) == R.pack(_bits(ref))).all(dim=-1)          # [B, N] tokens
    share = 1.0 - same.double().mean().item()
    mag = torch.maximum(torch.maximum(ref.double().abs(), x.double().abs()), (ref.double() - x.double()).abs())
    diff = (got.double() - ref.double()).abs()
    if vd == bf16:
        worst = (diff / _ulp(mag, 7)).max().item()
        print(f"{name}: tokens {same.numel()} differing share {share:.5f} worst element {worst:.3f} bf16 ulp")
        assert share <= R.MISMATCH_CAP, (name, share)
        assert (diff <= 2 * _ulp(mag, 7)).all(), (name, worst)
    elif xd == torch.float32:
        worst = (diff / _ulp(mag, 23)).max().item()
        print(f"{name}: tokens {same.numel()} differing share {share:.5f} worst element {worst:.3f} f32 ulp")
        assert (diff <= 4 * _ulp(mag, 23)).all(), (name, worst)
    else:                                                                  # f32 predictions, bf16 sample: the final cast (module docstring)
        elem = (diff > 0).double().mean().item()
        worst = (diff / _ulp(mag, 7)).max().item()
        print(f"{name}: elements differing share {elem:.6f} worst element {worst:.3f} bf16 ulp")
        assert elem <= R.MISMATCH_CAP and (diff <= _ulp(mag, 7)).all(), (name, elem, worst)


@pytest.mark.parametrize("shape", R.SHAPES, ids=["x".join(map(str, s)) for s in R.SHAPES])
@pytest.mark.parametrize("vd,xd", [(bf16, bf16), (bf16, torch.float32), (torch.float32, bf16), (torch.float32, torch.float32)])
def test_single_prediction_form_is_the_plain_euler_step(shape, vd, xd):
    sig = _sigmas()
    v, _, x = (t.cuda() for t in R.make_inputs(shape, vd, xd, 1.0, 77))
    got = _run(v, None, x, sig)
    assert torch.equal(_bits(got), _bits(R.cfg_euler_step(v, None, x, sig[STEP], sig[STEP + 1])))


@pytest.mark.parametrize("shape,guard", [((3, 16, 64, 64), 64), ((3, 16, 64, 64), 2), ((1, 16, 2, 258), 2), ((2, 16, 6, 10), 6)])
@pytest.mark.parametrize("xd", [bf16, torch.float32])
def test_guard_rows_stay_untouched_and_both_lane_layouts_agree(shape, guard, xd):
    """The output sits inside a sentinel-filled buffer.  guard = 64 elements keeps the 16-byte alignment of the two-tokens-per-lane
    layout; guard = 2 leaves only the alignment of one token row and takes the one-token layout: the same bits either way.  In place
    (prev_sample == sample) gives them too."""
    sig = _sigmas()
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, bf16, xd, 1.0, 78))
    n = x.numel()
    buf = torch.full((n + 2 * guard,), 7.0, dtype=xd, device="cuda")
    out = buf[guard:guard + n].view(shape)
    plain = _run(neg, pos, x, sig)
    _run(neg, pos, x, sig, out=out)
    assert (buf[:guard] == 7.0).all() and (buf[guard + n:] == 7.0).all()
    assert torch.equal(_bits(out), _bits(plain))
    inplace = x.clone()
    _run(neg, pos, inplace, sig, out=inplace)
    assert torch.equal(_bits(inplace), _bits(plain))


@pytest.mark.parametrize("shape", [(2, 16, 6, 10), (3, 16, 64, 64)])
def test_all_zero_token_is_nan_in_that_token_only(shape):
    sig = _sigmas()
    neg, pos, x = (t.cuda() for t in R.make_inputs(shape, bf16, bf16, 1.0, 79))
    neg[1, :, 2:4, 4:6] = 0
    pos[1, :, 2:4, 4:6] = 0
    got = _run(neg, pos, x, sig)
    nan = torch.isnan(got.float())
    want = torch.zeros_like(nan)
    want[1, :, 2:4, 4:6] = True
    assert torch.equal(nan, want) and torch.isfinite(got.float()[~want]).all()
    ref = R.cfg_euler_step(neg, pos, x, sig[STEP], sig[STEP + 1])
    assert torch.equal(torch.isnan(ref.float()), want)                     # as the pipeline's ops do


def test_shapes_the_kernel_is_not_built_for_are_refused():
    from adv_grpo_amd import _lib
    from adv_grpo_amd import qwen_generate as Q
    sig = _sigmas()
    for shape in ((1, 8, 4, 4), (1, 16, 4, 3), (1, 16, 3, 4)):
        t = torch.zeros(shape, dtype=bf16, device="cuda")
        with pytest.raises(_lib.AdvGrpoError):
            Q.cfg_euler_step(t, t, t, sig, STEP, 4.0)
    t = torch.zeros(1, 16, 4, 4, dtype=bf16, device="cuda")
    with pytest.raises(ValueError):
        Q.cfg_euler_step(t, t.float(), t, sig, STEP, 4.0)


# ---------------------------------------------------------------------------------------------------------------- end to end
B, T_POS, T_NEG, VALID_1, STEPS, SIDE = 2, 34 + 21, 34 + 5, 34 + 16, 4, 64


@pytest.fixture(scope="module")
def tiny():
    """A 2-block MMDiT, a 2-layer text tower and the synthetic Qwen VAE; prompts of 21 and 16 tokens, a 5-token negative prompt;
    the fused, the sequenced and the sequenced-in-f32 runs from the same noise, computed once."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import QwenMMDiTConfig, QwenTextConfig, QwenVaeConfig
    from adv_grpo_amd.qwen_generate import QwenImageSampler
    from adv_grpo_amd.qwen_mmdit import QwenImageTransformer2DModel
    from adv_grpo_amd.qwen_text_encoder import Qwen25VLTextEncoder
    from adv_grpo_amd.qwen_vae import AutoencoderKLQwenImageDecoder
    tcfg = QwenTextConfig(vocab_size=400, hidden_size=256, intermediate_size=512, num_layers=2, num_heads=2, num_kv_heads=1)
    enc = Qwen25VLTextEncoder({k: v.to(bf16) for k, v in synthetic.qwen_text_weights(tcfg, 3).items()}, tcfg, "cuda")
    mcfg = QwenMMDiTConfig(num_layers=2, num_heads=4, joint_attention_dim=256)
    tr = QwenImageTransformer2DModel({k: v.to(bf16) for k, v in synthetic.qwen_mmdit_weights(mcfg, 3).items()}, mcfg, "cuda")
    vcfg = QwenVaeConfig()
    vae = AutoencoderKLQwenImageDecoder(synthetic.qwen_vae_decoder_weights(vcfg, 7, dtype=bf16), vcfg, "cuda", mode="bf16")
    sampler = QwenImageSampler(enc, tr, vae)
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 400, (B, T_POS), generator=g)
    mask = torch.ones(B, T_POS, dtype=torch.long)
    mask[1, VALID_1:] = 0
    nids = torch.randint(0, 400, (1, T_NEG), generator=g)
    nmask = torch.ones(1, T_NEG, dtype=torch.long)
    noise = torch.randn(B, 16, SIDE // 8, SIDE // 8, generator=g)
    kw = dict(attention_mask=mask, neg_input_ids=nids, neg_attention_mask=nmask, height=SIDE, width=SIDE, num_inference_steps=STEPS,
              true_cfg_scale=4.0, noises=noise)
    runs = {"fused": sampler(ids, output_type="latent", **kw).clone(),
            "sequenced": sampler(ids, output_type="latent", sequenced=True, **kw).clone(),
            "f32": sampler(ids, output_type="latent", sequenced=True, step_f32=True, **kw).clone()}
    torch.cuda.synchronize()
    return dict(sampler=sampler, ids=ids, kw=kw, runs=runs)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_fused_sampler_stays_inside_the_restatements_own_rounding_noise(tiny):
    r = tiny["runs"]
    assert all(t.shape == (B, 16, SIDE // 8, SIDE // 8) and torch.isfinite(t.float()).all() for t in r.values())
    err, noise = _rel(r["fused"], r["sequenced"]), _rel(r["sequenced"], r["f32"])
    print(f"final latents: fused vs sequenced rel L2 {err:.3e}; sequenced vs sequenced-with-the-step-in-f32 {noise:.3e}; ratio "
          f"{err / noise if noise else float('nan'):.3f}")
    assert noise > 0 and err <= 2 * noise
    vae = tiny["sampler"].vae
    a, b = ((vae.decode_to_image(r[k]).clamp(0, 1) * 255).round().to(torch.int16) for k in ("fused", "sequenced"))
    assert a.shape == (B, 3, SIDE, SIDE)
    close = ((a - b).abs() <= 1).double().mean().item()
    print(f"images: {close:.5f} of the uint8 pixels within 1")
    assert close >= 0.99


def test_noises_reproduce_and_padding_positions_do_not_matter(tiny):
    s, ids, kw, r = tiny["sampler"], tiny["ids"], tiny["kw"], tiny["runs"]
    assert torch.equal(s(ids, output_type="latent", **kw), r["fused"])
    other = ids.clone()
    other[1, VALID_1:] = (other[1, VALID_1:] + 123) % 400                   # what the padding positions of the shorter prompt hold
    assert torch.equal(s(other, output_type="latent", **kw), r["fused"])
    changed = ids.clone()
    changed[1, VALID_1 - 1] = (changed[1, VALID_1 - 1] + 1) % 400           # ... while a valid token does
    assert not torch.equal(s(changed, output_type="latent", **kw), r["fused"])
    seeded = dict(kw, noises=None)
    a, b = s(ids, seed=11, output_type="latent", **seeded).clone(), s(ids, seed=11, output_type="latent", **seeded)
    assert torch.equal(a, b) and not torch.equal(a, s(ids, seed=12, output_type="latent", **seeded))
    img = s(ids, output_type="pil", **kw)
    assert len(img) == B and img[0].size == (SIDE, SIDE)
    # true_cfg_scale <= 1 (or no negative prompt): one transformer call and the single-prediction step
    one = s(ids, output_type="latent", **dict(kw, true_cfg_scale=1.0))
    assert torch.isfinite(one.float()).all() and not torch.equal(one, r["fused"])
    assert torch.equal(one, s(ids, output_type="latent", **dict(kw, neg_input_ids=None, neg_attention_mask=None)))


def test_one_captured_step_replays_to_the_eager_bits(tiny):
    """Step 1 of the loop -- two transformer calls and the fused launch -- under torch.cuda.graph: the replay reads sigma through
    the table's device pointer and gives the eager step's bits, twice."""
    s, ids, kw = tiny["sampler"], tiny["ids"], tiny["kw"]
    st = s.prepare(ids, **kw)
    s.step(st, 0)
    start = st["latents"].clone()
    s.step(st, 1)
    eager = st["latents"].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up on the capture's kind of stream
        st["latents"].copy_(start)
        s.step(st, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    st["latents"].copy_(start)
    with torch.cuda.graph(graph):
        s.step(st, 1)
    for _ in range(2):
        st["latents"].copy_(start)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st["latents"], eager)
