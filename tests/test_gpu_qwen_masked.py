"""MI355X: the Qwen-Image MMDiT with a prompt mask (encoder_hidden_states_mask -> per-sample attention lengths).

What the mask means is what it means in diffusers' QwenImagePipeline: the padding keys are masked, i.e. each sample is computed as on its
own unpadded prompt.  So the reference of a masked batch is, per sample, the oracle (oracle/qwen_mmdit.py) on the unpadded prompt, with
the criteria tests/test_gpu_qwen.py and tests/test_gpu_qwen_train.py already use; everything else here is bit equality.
Small configs as there: 2-4 blocks of 4 heads x 128, a 16 x 16 packed grid, Nt = 29 text positions, text lengths (3, 29, 17)."""
import pytest
import torch

from test_gpu_qwen_train import _cos, _lora_init

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
LENS = (3, 29, 17)
NT, HW = 29, 32


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _cfg(layers=3):
    from oracle.qwen_mmdit import QwenMMDiTConfig
    return QwenMMDiTConfig(num_layers=layers, num_heads=4, joint_attention_dim=256)


def _weights(cfg, seed):
    from adv_grpo_amd import synthetic
    return {k: v.to(bf16) for k, v in synthetic.qwen_mmdit_weights(cfg, seed).items()}


def _inputs(cfg, seed, lens=LENS):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    lat = torch.randn(B, 16, HW, HW, generator=g).to(bf16).cuda()
    ctx = torch.randn(B, NT, cfg.joint_attention_dim, generator=g).to(bf16).cuda()
    mask = (torch.arange(NT)[None, :] < torch.tensor(lens)[:, None]).to(torch.int64).cuda()
    t = torch.full((B,), 913.3488, dtype=torch.float32).cuda()
    return lat, ctx, mask, t


def _garbage(ctx, mask, scale, seed):
    """The same embeddings with finite garbage of magnitude `scale` at the padding positions."""
    g = torch.Generator().manual_seed(seed)
    junk = (torch.randn(ctx.shape, generator=g) * scale).to(bf16).cuda()
    return torch.where(mask.bool()[..., None], ctx, junk)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_output_does_not_depend_on_what_the_padding_positions_hold(fp8):
    """Two runs whose encoder_hidden_states differ only at the padding positions (garbage of magnitude 1e-2 and 30): the same bits.  An
    all-ones mask gives the bits of the call without a mask, and the ragged mask does not."""
    from adv_grpo_amd.qwen_mmdit import QwenImageTransformer2DModel
    cfg = _cfg()
    model = QwenImageTransformer2DModel(_weights(cfg, 11), cfg, "cuda")
    if fp8:
        model.enable_fp8()
    lat, ctx, mask, t = _inputs(cfg, 12)
    a = model(lat, t, _garbage(ctx, mask, 1e-2, 1), encoder_hidden_states_mask=mask)[0]
    b = model(lat, t, _garbage(ctx, mask, 30.0, 2), joint_attention_kwargs={"encoder_hidden_states_mask": mask})[0]
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    plain = model(lat, t, ctx)[0]
    assert torch.equal(model(lat, t, ctx, encoder_hidden_states_mask=torch.ones_like(mask))[0], plain)
    assert torch.equal(model(lat, t, ctx, encoder_hidden_states_mask=torch.ones_like(mask).bool())[0], plain)
    full = [i for i, L in enumerate(LENS) if L == NT]
    assert not torch.equal(a, plain) and torch.equal(a[full], plain[full])      # the full-length sample keeps its bits, the others move
    from adv_grpo_amd import ops
    assert ops.bad_count(reset=True) == 0


def test_masked_forward_against_the_oracle_on_the_unpadded_prompts():
    """Per sample, oracle.qwen_mmdit.qwen_forward on the unpadded prompt is the reference; criterion of tests/test_gpu_qwen.py:
    rel(hip, f32 oracle) < max(2 rel(torch bf16 oracle, f32 oracle), 1e-2)."""
    from adv_grpo_amd.qwen_mmdit import QwenImageTransformer2DModel
    from oracle import qwen_mmdit as o
    cfg = _cfg(4)
    W = _weights(cfg, 21)
    model = QwenImageTransformer2DModel(dict(W), cfg, "cuda")
    lat, ctx, mask, t = _inputs(cfg, 22)
    out = model(lat, t, _garbage(ctx, mask, 5.0, 3), encoder_hidden_states_mask=mask)[0]
    Wb = {k: v.cuda() for k, v in W.items()}
    W32 = {k: v.float() for k, v in Wb.items()}
    for b, L in enumerate(LENS):
        ref = o.qwen_forward(W32, cfg, lat[b:b + 1].float(), t[b:b + 1] / 1000, ctx[b:b + 1, :L].float())
        tb = o.qwen_forward(Wb, cfg, lat[b:b + 1], t[b:b + 1] / 1000, ctx[b:b + 1, :L])
        e_hip, e_torch = _rel(out[b:b + 1], ref), _rel(tb, ref)
        print(f"masked qwen sample {b} (text length {L}): rel err hip {e_hip:.4g} torch-bf16 {e_torch:.4g}")
        assert e_hip < max(2 * e_torch, 1e-2), (b, e_hip, e_torch)


def _train_run(model, lat, t, ctx, mask, dv):
    model.grads.zero_()
    v, saved = model.forward_train(lat, t, ctx, encoder_hidden_states_mask=mask)
    dx, dc = model.backward(saved, dv)
    return v, dx, dc, {k: g.clone() for k, g in model.lora_grads().items()}


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_training_pass_does_not_depend_on_the_padding_and_padding_rows_carry_zero_gradient(fp8):
    """forward_train + backward on two paddings: v, dx, the text-stream gradient at the valid rows and every LoRA gradient are bit-equal;
    the text-stream gradient at the padding rows is exactly zero (which is why the adapter-gradient GEMMs, which sum over all rows, do
    not see them)."""
    from adv_grpo_amd.qwen_mmdit_train import QwenImageTransformerLoRA
    cfg = _cfg()
    model = QwenImageTransformerLoRA(_weights(cfg, 31), cfg, "cuda", lora_state=_lora_init(cfg, 32))
    if fp8:
        model.enable_fp8()
    lat, ctx, mask, t = _inputs(cfg, 33)
    dv = torch.randn(lat.shape, generator=torch.Generator().manual_seed(34)).to(bf16).cuda()
    v1, dx1, dc1, g1 = _train_run(model, lat, t, _garbage(ctx, mask, 1e-2, 1), mask, dv)
    v2, dx2, dc2, g2 = _train_run(model, lat, t, _garbage(ctx, mask, 30.0, 2), mask, dv)
    assert torch.equal(v1, model(lat, t, ctx, encoder_hidden_states_mask=mask)[0])           # training forward == rollout forward
    assert torch.equal(v1, v2) and torch.equal(dx1, dx2)
    live = mask.bool().reshape(-1)
    assert torch.equal(dc1[live], dc2[live])
    assert not bool(dc1[~live].any()) and not bool(dc2[~live].any())
    assert set(g1) == set(g2) and any(g.abs().max().item() > 0 for g in g1.values())
    for k in g1:
        assert torch.isfinite(g1[k]).all() and torch.equal(g1[k], g2[k]), k


def test_lora_gradients_of_a_ragged_batch_against_autograd_on_the_unpadded_samples():
    """fp32 autograd through the oracle's W + s B A, each sample on its unpadded prompt, summed over the batch.  The limits are those of
    tests/test_gpu_qwen_train.py::_lora_case for its bf16 small-config case: cosine > 0.97, 0.9 < norm ratio < 1.1."""
    from adv_grpo_amd.qwen_mmdit_train import QwenImageTransformerLoRA
    from oracle import lora as o_lora
    from oracle import qwen_mmdit as o
    cfg = _cfg()
    W, lora = _weights(cfg, 41), _lora_init(cfg, 42)
    model = QwenImageTransformerLoRA(dict(W), cfg, "cuda", lora_state=lora)
    lat, ctx, mask, t = _inputs(cfg, 43)
    dv = torch.randn(lat.shape, generator=torch.Generator().manual_seed(44)).to(bf16).cuda()
    v, _, _, grads = _train_run(model, lat, t, _garbage(ctx, mask, 5.0, 3), mask, dv)
    W32 = {k: x.float().cuda() for k, x in W.items()}
    lo = {k: x.cuda().requires_grad_(True) for k, x in lora.items()}
    We = o_lora.effective_weights(W32, lo)
    total = 0.0
    for b, L in enumerate(LENS):
        out = o.qwen_forward(We, cfg, lat[b:b + 1].float(), t[b:b + 1] / 1000, ctx[b:b + 1, :L].float())
        assert _rel(v[b:b + 1], out) < 3e-2
        total = total + (out * dv[b:b + 1].float()).sum()
    total.backward()
    c_min, r_lo, r_hi = 0.97, 0.9, 1.1
    worst, worst_ratio = 1.0, 1.0
    for k, gr in grads.items():
        ref = lo[k].grad
        if ref is None or ref.norm().item() == 0:          # add_q_proj / to_add_out of the last block: nothing reads its text-stream output
            assert gr.abs().max().item() == 0, k
            continue
        c, ratio = _cos(gr, ref), (gr.norm() / ref.norm()).item()
        worst, worst_ratio = min(worst, c), max(worst_ratio, max(ratio, 1 / ratio))
        assert c > c_min and r_lo < ratio < r_hi, (k, c, ratio)
    print("masked qwen LoRA grads: worst cosine", worst, "worst norm ratio", worst_ratio)


# ---------------------------------------------------------------------------------------------------------------- rollout, trainer
def _pipe(cfg, seed, lora=True):
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import QwenVaeConfig
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.qwen_mmdit_train import QwenImageTransformerLoRA
    from adv_grpo_amd.qwen_vae import AutoencoderKLQwenImageDecoder
    model = QwenImageTransformerLoRA(_weights(cfg, seed), cfg, "cuda", lora_state=_lora_init(cfg, seed + 1))
    vcfg = QwenVaeConfig()
    vae = AutoencoderKLQwenImageDecoder(synthetic.qwen_vae_decoder_weights(vcfg, 7, dtype=bf16), vcfg, "cuda", mode="bf16")
    return SD3Pipeline(model, vae, "cuda"), model


def test_rollout_carries_the_mask_to_the_kernel_on_both_cfg_schedules():
    """pipeline_with_logprob_random on a ragged CFG batch (a 3-token negative prompt, a 17-token positive one, Nt = 29) with the mask in
    joint_attention_kwargs: cfg_two_streams on and off give the same bits, and the result differs from the run without the mask."""
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_random
    cfg = _cfg(2)
    pipe, _ = _pipe(cfg, 5)
    g = torch.Generator().manual_seed(8)
    pe, npe = (torch.randn(1, NT, cfg.joint_attention_dim, generator=g).to(bf16).cuda() for _ in range(2))
    pooled = torch.zeros(1, 8, dtype=bf16, device="cuda")
    G = 2
    pos = (torch.arange(NT)[None] < 17).to(torch.int64).cuda()
    neg = (torch.arange(NT)[None] < 3).to(torch.int64).cuda()
    rows = torch.cat([neg.repeat(G, 1), pos.repeat(G, 1)])                      # the CFG batch's order: negative rows first
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=pooled,
              num_inference_steps=4, guidance_scale=4.0, height=256, width=256, noise_level=0.8, mini_num_image_per_prompt=G,
              train_num_steps=2, process_index=0, sample_num_steps=4, random_timestep=0, seed=77, output_type="latent")
    runs = {}
    for name, two, jk in (("one", False, {"encoder_hidden_states_mask": rows}), ("two", True, {"encoder_hidden_states_mask": rows}),
                          ("nomask", False, None)):
        pipe.cfg_two_streams = two
        _, lats, lps, _ = pipeline_with_logprob_random(pipe, joint_attention_kwargs=jk, **kw)
        torch.cuda.synchronize()
        runs[name] = (lats, lps)
    pipe.cfg_two_streams = False
    assert all(torch.equal(a, b) for a, b in zip(runs["one"][0], runs["two"][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs["one"][1], runs["two"][1]))
    assert all(torch.isfinite(x.float()).all() for x in runs["one"][0])
    assert not torch.equal(runs["one"][0][-1], runs["nomask"][0][-1])           # the mask reaches the kernel


def test_one_trainer_step_with_a_data_source_that_yields_masks(monkeypatch):
    """Trainer.run_epoch on a data source with prompt_mask / neg_mask: the rollout gets the CFG-batch mask, the replay gets it through
    forward_train, and the replayed log-probs are the rollout's to the limit of test_gpu_qwen_train.py's chain test (3e-4)."""
    from adv_grpo_amd import trainer as T
    from adv_grpo_amd.config.experiments import get_config
    cfg = get_config("pickscore_sd3_fast", gpu_number=1)
    cfg.reward_fn = {"jpeg_compressibility": 1}
    cfg.resolution = 256
    cfg.sample.num_steps = 4
    cfg.sample.num_image_per_prompt = cfg.sample.mini_num_image_per_prompt = 2
    cfg.sample.num_batches_per_epoch = 2
    cfg.sample.groups_in_flight = 1
    cfg.train.gradient_accumulation_steps = 1
    qcfg = _cfg(2)
    pipe, model = _pipe(qcfg, 5)

    class MaskedData(T.SyntheticData):
        neg_mask = (torch.arange(NT)[None] < 3).to(torch.int64)

        def prompt_mask(self, idx):
            return (torch.arange(NT)[None] < 5 + idx % 20).to(torch.int64)
    data = MaskedData(n_prompts=50, n_tokens=NT, ctx_dim=qcfg.joint_attention_dim, pooled_dim=8, resolution=256)
    tr = T.Trainer(cfg, pipe, data, None, None)
    seen = {"rollout": [], "replay": []}
    real_rollout, real_micro = T.pipeline_with_logprob_random, T.g_step.micro_step

    def rollout(p, **kw):
        seen["rollout"].append(kw["joint_attention_kwargs"]["encoder_hidden_states_mask"].clone())
        return real_rollout(p, **kw)

    def micro(m, sched, sample, j, embeds, pooled, old, adv, **kw):
        info = real_micro(m, sched, sample, j, embeds, pooled, old, adv, **kw)
        seen["replay"].append((kw["embeds_mask"].clone(), (info["log_prob"] - old).abs().max().item()))
        return info
    monkeypatch.setattr(T, "pipeline_with_logprob_random", rollout)
    monkeypatch.setattr(T.g_step, "micro_step", micro)
    p0 = model.params.clone()
    info = tr.run_epoch()
    assert info["phase"] == "G" and not torch.equal(model.params, p0)
    G = 2
    assert len(seen["rollout"]) == 2 and len(seen["replay"]) == 2 * cfg.sample.train_num_steps
    for m in seen["rollout"]:
        assert m.shape == (2 * G, NT) and m[:G].sum(1).tolist() == [3] * G and m[G].sum().item() >= 5
    rollout_masks = {tuple(m.flatten().tolist()) for m in seen["rollout"]}
    for m, diff in seen["replay"][:cfg.sample.train_num_steps * 2]:
        assert tuple(m.flatten().tolist()) in rollout_masks                    # the replay's mask is a rollout's, row for row
    # before the first optimizer step the policy is the rollout's: the first group's replays are on-policy
    for m, diff in seen["replay"][:cfg.sample.train_num_steps]:
        assert diff < 3e-4, diff
