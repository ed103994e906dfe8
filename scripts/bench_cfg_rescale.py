"""The Flow-CPS step under Qwen-Image's norm-rescaled true CFG at [8, 16, 128, 128] bf16 (a 1024 x 1024 Qwen-Image latent batch): the
fused kernels next to the same step as separate operations.

  python scripts/bench_cfg_rescale.py [--iters N] [--sde-type cps|sde]

Four legs, each in a fresh child process under its own `timeout`; the parent never opens the GPU:

  fwd_fused       sde_step_cfg(cfg_rescale=True), in-kernel Philox: one launch + the log-prob finalize
  fwd_sequenced   sde_step_cfg(cfg_rescale=True, sequenced=True): torch's combine, two norms and rescale, then the plain fused step
  bwd_fused       advgrpo_sde_step_rescaled_bwd (advgrpo_flow_sde_step_rescaled_bwd) on the replayed step, policy gradient only
  bwd_sequenced   the plain step's backward entry for dL/dv, then torch autograd through the combine, the norms and the rescale
                  (the autograd graph is rebuilt every call, as a training step would)

A leg warms up, then reports the median over `--iters` (>= 5) timed intervals of 20 calls: host-inclusive microseconds per call.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ["fwd_fused", "fwd_sequenced", "bwd_fused", "bwd_sequenced"]
SHAPE, INNER, SCALE, NOISE_LEVEL, STEP = (8, 16, 128, 128), 20, 4.0, 0.8, 2


def child(leg, sde_type, iters):
    import torch
    from adv_grpo_amd import _lib
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import rescaled_prediction, sde_step_cfg
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    lib = _lib.load()
    sch = FlowMatchEulerDiscreteScheduler(device=torch.device("cuda"))
    sch.set_timesteps(10, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(0)
    bf16 = torch.bfloat16
    vu, vt, x = (torch.randn(SHAPE, generator=g).to(bf16).cuda() for _ in range(3))
    prev = (x.float() + 0.1 * torch.randn(SHAPE, generator=g).cuda()).to(bf16)
    glp = torch.randn(SHAPE[0], generator=g).cuda()
    B, n = SHAPE[0], SHAPE[1] * SHAPE[2] * SHAPE[3]
    sig, sigp = sch.sigmas[STEP:STEP + 1], sch.sigmas[STEP + 1:STEP + 2]
    flow = sde_type == "sde"
    level = (NOISE_LEVEL, sch.sigmas[1:2].data_ptr()) if flow else (float(math.sin(NOISE_LEVEL * math.pi / 2)),)
    fwd_kw = dict(noise_level=NOISE_LEVEL, seed=5, offset=1000, out_dtype=bf16, want_mean=False, step_index=STEP, sde_type=sde_type,
                  cfg_rescale=True, sequenced=leg == "fwd_sequenced")
    gu, gt = torch.empty_like(vu), torch.empty_like(vt)
    code = _lib.BF16

    def head(a, b):
        return (a.data_ptr(), None if b is None else b.data_ptr(), code, SCALE, x.data_ptr(), code, sig.data_ptr(), sigp.data_ptr(), 0, *level,
                prev.data_ptr(), code, glp.data_ptr())

    def call():
        if leg.startswith("fwd"):
            return sde_step_cfg(sch, vu, vt, SCALE, None, x, **fwd_kw)[1]
        if leg == "bwd_fused":
            fn = lib.advgrpo_flow_sde_step_rescaled_bwd if flow else lib.advgrpo_sde_step_rescaled_bwd
            _lib.check(fn(*head(vu, vt), None, 0.0, gu.data_ptr(), gt.data_ptr(), None, None, *SHAPE, 2, _lib.stream_ptr()))
            return gt
        with torch.enable_grad():
            a, b = vu.detach().requires_grad_(True), vt.detach().requires_grad_(True)
            v = rescaled_prediction(a, b, SCALE)
        gv = torch.empty_like(v)
        fn = lib.advgrpo_flow_sde_step_bwd if flow else lib.advgrpo_sde_step_bwd
        _lib.check(fn(*head(v.detach(), None), gv.data_ptr(), None, B, n, _lib.stream_ptr()))
        v.backward(gv)
        return b.grad

    def interval():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(INNER):
            out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / INNER * 1e6, out
    for _ in range(3):                                   # warm-up: code object, allocator
        _, out = interval()
    assert out.shape == SHAPE and torch.isfinite(out.float()).all()
    times = [interval()[0] for _ in range(iters)]
    print(json.dumps({"us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7, help="timed intervals of 20 calls per leg (median reported; at least 5)")
    ap.add_argument("--sde-type", default="cps", choices=["cps", "sde"])
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per child process")
    ap.add_argument("child", nargs="*", help=argparse.SUPPRESS)
    args = ap.parse_args()
    iters = max(5, args.iters)
    if args.child:
        return child(args.child[0], args.sde_type, iters)
    out = {}
    for leg in LEGS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), leg, "--iters", str(iters),
               "--sde-type", args.sde_type]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                          # nothing more is started on the GPU after a failed leg
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"bench_cfg_rescale: leg {leg} ended with status {res.returncode}")
        out[leg] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps({"bench": "cfg_rescale", "shape": {"tensor": list(SHAPE), "dtype": "bf16", "sde_type": args.sde_type, "guidance": SCALE},
                      "unit": "host-inclusive us per call, median of %d intervals of %d calls" % (iters, INNER), **out,
                      "fwd_speedup": round(out["fwd_sequenced"]["us"] / out["fwd_fused"]["us"], 3),
                      "bwd_speedup": round(out["bwd_sequenced"]["us"] / out["bwd_fused"]["us"], 3)}))


if __name__ == "__main__":
    main()
