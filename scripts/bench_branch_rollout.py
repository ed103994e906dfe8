"""The shared-prefix branching rollout (pipeline_with_logprob_new) next to pipeline_with_logprob_random at BASELINE config 2's shape:
SD3.5-medium, 512^2, G = sample.mini_num_image_per_prompt images of one prompt, T = sample.num_steps denoise steps with CFG, synthetic weights.

  python scripts/bench_branch_rollout.py [--iters N] [--layers L]

For every branch step r in 0 .. T // 2 the two functions run alternately in ONE process (warm-up first, median of `--iters` timed calls each),
with output_type="latent": the MMDiT forwards and the SDE steps, which is what the row-count model describes -- a branch at r puts
r * P + (T - r) * P * G latent rows through the MMDiT instead of T * P * G (`row_model`; with the branch step's own forward on the P
un-repeated rows, as the fan-out step allows, (r + 1) * P + (T - r - 1) * P * G: `row_model_fan_out`).  The decode of the G final latents is the same call in both and is
timed once beside them.  The second measurement is the branch step's kernel alone: advgrpo_sde_step_branch (P rows in, P * G out) against
advgrpo_sde_step on the materialised repeat (with and without the three .repeat copies) and against G launches of advgrpo_sde_step.

Each of the two measurements is a child process under its own `timeout`; the parent never opens the GPU.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, iters):
    import torch
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return statistics.median(out)


def child_rollouts(iters, layers):
    import torch
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.diffusers_patch.sd3_pipeline_with_logprob_fast import pipeline_with_logprob_new, pipeline_with_logprob_random
    from adv_grpo_amd.mmdit import SD3Transformer2DModel
    from adv_grpo_amd.model_configs import MMDiTConfig, VaeConfig
    from adv_grpo_amd.pipeline import SD3Pipeline
    from adv_grpo_amd.vae import AutoencoderKLDecoder
    cfg = get_config("pickscore_cotrain_sd3_fast", gpu_number=1)
    G, T, train_T, res = cfg.sample.mini_num_image_per_prompt, cfg.sample.num_steps, cfg.sample.train_num_steps, cfg.resolution
    mcfg = MMDiTConfig() if layers is None else MMDiTConfig(num_layers=layers, dual_attention_layers=tuple(range(min(13, layers))))
    with synthetic.on_device("cuda"):
        tr = SD3Transformer2DModel(synthetic.mmdit_weights(mcfg, 1234), mcfg, "cuda")
        vae = AutoencoderKLDecoder(synthetic.vae_decoder_weights(VaeConfig(), 4321, fp16_checkpoint=True), VaeConfig(), "cuda")
    pipe = SD3Pipeline(tr, vae, "cuda")
    pe, ppe, npe, nppe = (t.cuda().to(torch.bfloat16) for t in synthetic.prompt_embeddings(5))
    P = pe.shape[0]

    def call(fn, r):
        return fn(pipe, prompt_embeds=pe, pooled_prompt_embeds=ppe, negative_prompt_embeds=npe, negative_pooled_prompt_embeds=nppe,
                  num_inference_steps=T, guidance_scale=cfg.sample.guidance_scale, height=res, width=res, noise_level=cfg.sample.noise_level,
                  mini_num_image_per_prompt=G, train_num_steps=train_T, process_index=0, sample_num_steps=T, random_timestep=r, seed=11,
                  output_type="latent")
    rows = []
    for r in range(T // 2 + 1):
        for fn in (pipeline_with_logprob_random, pipeline_with_logprob_new):          # warm-up: allocator, streams, code objects
            call(fn, r)
        t_rand, t_new = [], []
        for _ in range(iters):                                                         # alternating: drift hits both alike
            t_rand.append(_median_ms(lambda: call(pipeline_with_logprob_random, r), 1))
            t_new.append(_median_ms(lambda: call(pipeline_with_logprob_new, r), 1))
        m_rand, m_new = statistics.median(t_rand), statistics.median(t_new)
        model = (r * P + (T - r) * P * G) / (T * P * G)                  # the reference's rows: the branch step on P * G rows
        fan = ((r + 1) * P + (T - r - 1) * P * G) / (T * P * G)          # here the branch step's forward has P rows as well (the fan-out step)
        rows.append({"r": r, "random_ms": round(m_rand, 2), "new_ms": round(m_new, 2), "new_over_random": round(m_new / m_rand, 4),
                     "row_model": round(model, 4), "row_model_ms": round(m_rand * model, 2),
                     "row_model_fan_out": round(fan, 4), "row_model_fan_out_ms": round(m_rand * fan, 2)})
    lat = call(pipeline_with_logprob_new, 0)[0]
    vae.decode_to_image(lat)
    decode_ms = _median_ms(lambda: vae.decode_to_image(lat), max(3, iters))
    print(json.dumps({"shape": {"P": P, "G": G, "T": T, "train_num_steps": train_T, "resolution": res, "mmdit_layers": mcfg.num_layers},
                      "iters": iters, "timed": "MMDiT forwards + SDE steps (output_type=latent)", "per_r": rows,
                      "decode_ms_same_in_both": round(decode_ms, 2)}))


def child_step(iters):
    import torch
    from adv_grpo_amd.config.experiments import get_config
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    cfg = get_config("pickscore_cotrain_sd3_fast", gpu_number=1)
    P, G, res = 1, cfg.sample.mini_num_image_per_prompt, cfg.resolution
    sch = FlowMatchEulerDiscreteScheduler(device=torch.device("cuda"))
    sch.set_timesteps(cfg.sample.num_steps, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(0)
    vu, vt, x = (torch.randn(P, 16, res // 8, res // 8, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    kw = dict(noise_level=0.8, seed=5, offset=1000, out_dtype=torch.bfloat16, want_mean=False, step_index=2)
    rep = lambda t: t.repeat(G, 1, 1, 1)
    ru, rt, rx = rep(vu), rep(vt), rep(x)
    n4 = x[0].numel() // 4

    def loop(fn, inner=50):
        fn()
        return _median_ms(lambda: [fn() for _ in range(inner)], iters) / inner
    fan = loop(lambda: sde_step_cfg(sch, vu, vt, 4.5, None, x, copies=G, **kw))
    plain = loop(lambda: sde_step_cfg(sch, ru, rt, 4.5, None, rx, **kw))
    with_repeat = loop(lambda: sde_step_cfg(sch, rep(vu), rep(vt), 4.5, None, rep(x), **kw))
    launches = loop(lambda: [sde_step_cfg(sch, vu, vt, 4.5, None, x, **{**kw, "offset": 1000 + k * n4}) for k in range(G)])
    print(json.dumps({"shape": {"P": P, "G": G, "n": x[0].numel(), "dtype": "bf16", "mode": "philox", "cfg": True},
                      "note": "host-inclusive ms per call of sde_step_cfg (allocations and two launches each), 50 calls per timed interval",
                      "fan_out_ms": round(fan, 4), "plain_on_repeated_batch_ms": round(plain, 4),
                      "repeat_then_plain_ms": round(with_repeat, 4), "G_plain_launches_ms": round(launches, 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="timed calls per function and branch step (median reported)")
    ap.add_argument("--layers", type=int, default=None, help="reduce the MMDiT depth (a quick look; the reported numbers use the full 24)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds, per child process")
    ap.add_argument("child", nargs="?", choices=["rollouts", "step"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "rollouts":
        return child_rollouts(args.iters, args.layers)
    if args.child == "step":
        return child_step(max(3, args.iters))
    out = {}
    for name in ("step", "rollouts"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), name, "--iters", str(args.iters)]
        if args.layers is not None:
            cmd += ["--layers", str(args.layers)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                          # nothing more is started on the GPU after a failed step
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"bench_branch_rollout: child '{name}' ended with status {res.returncode}")
        out[name] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps({"bench": "branch_rollout", **out}))


if __name__ == "__main__":
    main()
