"""Head-dim-128 attention forward and backward at config 5's shape (B = 16 incl. CFG, 24 heads, S = 4096 + 128) on three legs:
the plain entries; the per-sample-length entries with every length = S; the per-sample-length entries with the CFG pattern (half the
samples at 4096 + 8: the negative prompt, half at 4096 + 128).  Prints one JSON line (milliseconds, median of `iters` interleaved rounds).
Usage: bench_attention_varlen.py [iters]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import ops

B, H, D, NI, NT, NEG = 16, 24, 128, 4096, 128, 8


def main(iters):
    S, HD = NI + NT, H * D
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, S, 3 * HD, device="cuda", generator=g).to(torch.bfloat16)
    q, k, v = qkv[..., :HD], qkv[..., HD:2 * HD], qkv[..., 2 * HD:]
    d_o = torch.randn(B, S, HD, device="cuda", generator=g).to(torch.bfloat16)
    out = torch.empty(B, S, HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv[..., :HD], dqkv[..., HD:2 * HD], dqkv[..., 2 * HD:]
    legs = {"plain": None, "varlen_full": torch.full((B,), S, dtype=torch.int32, device="cuda"),
            "varlen_cfg": torch.tensor([NI + NEG] * (B // 2) + [S] * (B // 2), dtype=torch.int32, device="cuda")}
    times = {name: {"fwd": [], "bwd": []} for name in legs}
    for it in range(iters + 2):                      # two warm-up rounds; the legs are interleaved so that clock drift hits all alike
        for name, lens in legs.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            ops.attention(q, k, v, H, out=out, lse=lse, seq_lens=lens)
            ev[1].record()
            ops.attention_bwd(q, k, v, out, d_o, lse, H, dq, dk, dv, seq_lens=lens)
            ev[2].record()
            torch.cuda.synchronize()
            if it >= 2:
                times[name]["fwd"].append(ev[0].elapsed_time(ev[1]))
                times[name]["bwd"].append(ev[1].elapsed_time(ev[2]))
    res = {"bench": "attention_varlen", "B": B, "H": H, "S": S, "head_dim": D, "cfg_lengths": [NI + NEG, S], "iters": iters}
    for name in legs:
        for what in ("fwd", "bwd"):
            res[f"{name}_{what}_ms"] = round(statistics.median(times[name][what]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
