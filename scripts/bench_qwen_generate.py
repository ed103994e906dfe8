"""Qwen-Image sampling: the fused true-CFG combine + Euler step against the sequenced torch step, and a whole 512 x 512 sample.

  python scripts/bench_qwen_generate.py [--iters N] [--steps 50] [--batch 4]

Two legs, each in a fresh child process under its own `timeout`; the parent never opens the GPU.
  step    [batch, 16, 64, 64] bf16 predictions and latents (a 512^2 image): host-inclusive milliseconds per call of
          qwen_generate.cfg_euler_step (one launch) and of cfg_euler_step_sequenced (the pipeline's torch ops), median over `--iters`
          (>= 5) timed intervals of 50 calls.
  sample  QwenImageSampler end to end at the synthetic small configuration of scripts/qwen_generate.py (2 transformer blocks, 2 text
          layers, the full-width VAE): prompt encoding, `--steps` steps of two transformer calls + the fused step, decode; median
          milliseconds per batch over `--iters` runs, fused and sequenced.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("step", "sample")
INNER = 50


def leg_step(iters, batch, steps):
    import torch
    from adv_grpo_amd import qwen_generate as Q
    from adv_grpo_amd.scheduler import QwenImageFlowMatchScheduler
    sch = QwenImageFlowMatchScheduler()
    sch.set_timesteps(50, 1024, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(0)
    neg, pos, x = (torch.randn(batch, 16, 64, 64, generator=g).to(torch.bfloat16).cuda() for _ in range(3))

    def interval(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(INNER):
            out = fn(neg, pos, x, sch.sigmas, 10, 4.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / INNER * 1e3, out
    res = {}
    for name, fn in (("fused", Q.cfg_euler_step), ("sequenced", Q.cfg_euler_step_sequenced)):
        for _ in range(3):                               # warm-up: code object, allocator
            _, out = interval(fn)
        assert out.shape == x.shape and torch.isfinite(out.float()).all()
        times = [interval(fn)[0] for _ in range(iters)]
        res[name + "_ms"] = round(statistics.median(times), 4)
        res[name + "_min_ms"], res[name + "_max_ms"] = round(min(times), 4), round(max(times), 4)
    print(json.dumps(res))


def leg_sample(iters, batch, steps):
    import torch
    from scripts.qwen_generate import build_sampler
    sampler = build_sampler(None, torch.device("cuda"))
    prompts = [f"a photo of object number {i}, Ultra HD, 4K, cinematic composition." for i in range(batch)]
    res = {}
    for name, seq in (("fused", False), ("sequenced", True)):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = sampler(prompts, neg_input_ids=[" "], height=512, width=512, num_inference_steps=steps, true_cfg_scale=4.0, seed=1,
                          output_type="pt", sequenced=seq)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, img
        _, img = run()                                   # warm-up
        assert img.shape == (batch, 3, 512, 512) and torch.isfinite(img).all()
        times = [run()[0] for _ in range(iters)]
        res[name + "_ms_per_batch"] = round(statistics.median(times), 2)
        res[name + "_ms_per_step"] = round(statistics.median(times) / steps, 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="timed intervals per leg (median reported; at least 5)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per child process")
    ap.add_argument("child", nargs="?", help=argparse.SUPPRESS)
    args = ap.parse_args()
    iters = max(5, args.iters)
    if args.child:
        return {"step": leg_step, "sample": leg_sample}[args.child](iters, args.batch, args.steps)
    out = {}
    for leg in LEGS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), leg, "--iters", str(iters),
               "--steps", str(args.steps), "--batch", str(args.batch)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                          # nothing more is started on the GPU after a failed leg
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"bench_qwen_generate: leg {leg} ended with status {res.returncode}")
        out[leg] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps({"bench": "qwen_generate", "shape": {"batch": args.batch, "latents": [16, 64, 64], "dtype": "bf16", "true_cfg_scale": 4.0,
                                                           "steps": args.steps, "image": 512},
                      "unit": "host-inclusive ms, median of %d intervals" % iters, **out}))


if __name__ == "__main__":
    main()
