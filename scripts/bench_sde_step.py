"""The fused SDE step at BASELINE config 2's step shape ([8, 16, 64, 64] bf16, CFG, in-kernel Philox): Flow-CPS next to Flow-SDE.

  python scripts/bench_sde_step.py [--iters N]

Four legs -- sde_type cps / sde x the plain entry (8 rows) / the fan-out entry (1 row in, 8 copies out) -- each in a fresh child process
under its own `timeout`; the parent never opens the GPU.  A leg warms up, then reports the median over `--iters` (>= 5) timed intervals of
50 calls of sde_step_cfg each: host-inclusive microseconds per call (the output allocations and the two launches).  The kernel moves 3 MB at
this shape and is launch-latency bound, so the two steps are expected to be indistinguishable.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = [(t, e) for e in ("plain", "fan_out") for t in ("cps", "sde")]
B, INNER = 8, 50


def child(sde_type, entry, iters):
    import torch
    from adv_grpo_amd.diffusers_patch.sd3_sde_with_logprob import sde_step_cfg
    from adv_grpo_amd.scheduler import FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler(device=torch.device("cuda"))
    sch.set_timesteps(10, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(0)
    rows = B if entry == "plain" else 1
    vu, vt, x = (torch.randn(rows, 16, 64, 64, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    kw = dict(noise_level=0.8, seed=5, offset=1000, out_dtype=torch.bfloat16, want_mean=False, step_index=2, sde_type=sde_type,
              copies=None if entry == "plain" else B)

    def interval():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(INNER):
            out = sde_step_cfg(sch, vu, vt, 4.5, None, x, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / INNER * 1e6, out
    for _ in range(3):                                   # warm-up: code object, allocator
        _, out = interval()
    assert out[1].shape == (B, 16, 64, 64) and torch.isfinite(out[2]).all()
    times = [interval()[0] for _ in range(iters)]
    print(json.dumps({"us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7, help="timed intervals of 50 calls per leg (median reported; at least 5)")
    ap.add_argument("--timeout", type=int, default=120, help="seconds, per child process")
    ap.add_argument("child", nargs="*", help=argparse.SUPPRESS)
    args = ap.parse_args()
    iters = max(5, args.iters)
    if args.child:
        return child(args.child[0], args.child[1], iters)
    out = {}
    for sde_type, entry in LEGS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), sde_type, entry, "--iters", str(iters)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                          # nothing more is started on the GPU after a failed leg
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"bench_sde_step: leg {sde_type}/{entry} ended with status {res.returncode}")
        out[f"{entry}_{sde_type}"] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps({"bench": "sde_step", "shape": {"rows": B, "n": 16 * 64 * 64, "dtype": "bf16", "cfg": True, "mode": "philox"},
                      "unit": "host-inclusive us per sde_step_cfg call, median of %d intervals of %d calls" % (iters, INNER), **out}))


if __name__ == "__main__":
    main()
