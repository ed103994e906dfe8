"""Time of the Qwen2.5-VL prompt encoder at the real width (28 layers of 3584, 28 query / 4 key-value heads of 128, SwiGLU 18944; random
weights, a 2000-row embedding table) on its three paths: the Python launch list (sequenced=True: the code of the commit before the entry,
unchanged), advgrpo_qwen_text_forward with the materialised attention, and with the fused grouped-query attention.

B = 2, T in {128, 512} for all three and T = 1058 (1024 prompt + 34 template tokens) for the fused path, the only one that takes it.  HIP
events around each call, the median of RUNS calls, the paths alternating in one process over ROUNDS rounds; the spread is that of the repeated
medians.  Prints one JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import synthetic, text_encoders as te                      # noqa: E402
from adv_grpo_amd.model_configs import QwenTextConfig                        # noqa: E402
from adv_grpo_amd.qwen_text_encoder import Qwen25VLTextEncoder               # noqa: E402

RUNS, ROUNDS, WARMUP = 7, 3, 2
LAYERS = int(os.environ.get("QWEN_TEXT_LAYERS", "28"))
cfg = QwenTextConfig(vocab_size=2000, num_layers=LAYERS)
with synthetic.on_device("cuda"):
    W = synthetic.qwen_text_weights(cfg, 9, dtype=torch.bfloat16)
mat = Qwen25VLTextEncoder(W, cfg, "cuda")
fused = Qwen25VLTextEncoder(W, cfg, "cuda", attention="fused")
fused.layers, fused.embed, fused.final_w = mat.layers, mat.embed, mat.final_w      # one copy of the weights


def timed(fn):
    """Median device milliseconds of RUNS calls (HIP events on the launch stream)."""
    ms = []
    for _ in range(RUNS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


result = {"bench": "qwen_text", "shape": f"{LAYERS} layers x 3584, 28/4 heads of 128, ff 18944, B=2", "runs_per_median": RUNS, "rounds": ROUNDS}
for T in (128, 512, 1058):
    ids = torch.randint(0, 2000, (2, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(T))
    paths = {"fused": lambda: fused(ids)}
    if T <= 512:
        paths = {"sequenced": lambda: mat(ids, sequenced=True), "materialised": lambda: mat(ids), **paths}
    outs = {}
    for _ in range(WARMUP):
        outs = {k: fn() for k, fn in paths.items()}
    assert all(bool(torch.isfinite(o.float()).all()) for o in outs.values())
    if T <= 512:
        assert torch.equal(outs["sequenced"], outs["materialised"])
        result[f"fused_vs_materialised_rel_T{T}"] = round(((outs["fused"].float() - outs["materialised"].float()).norm() /
                                                           outs["materialised"].float().norm()).item(), 5)
    med = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            med[k].append(timed(fn))
    for k, v in med.items():
        result[f"{k}_ms_T{T}"] = round(statistics.median(v), 3)
        result[f"{k}_spread_ms_T{T}"] = round(max(v) - min(v), 3)
result["bad_ids"] = te.bad_id_count()
print(json.dumps(result))
