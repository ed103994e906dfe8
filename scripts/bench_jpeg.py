"""jpeg_compressibility's size computation: the on-device encoder (jpeg.sizes, csrc/jpeg.hip) against the reference's host path
(adv_grpo/rewards.py:15-23: quantise, copy to the host, PIL save at quality 95), on the same noise images (the largest files).
Prints one JSON line per shape."""
import io
import json
import os
import sys
import time

import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adv_grpo_amd import jpeg  # noqa: E402


def host_sizes(x):
    a = (x * 255).round().clamp(0, 255).to(torch.uint8).cpu().numpy().transpose(0, 2, 3, 1)
    out = []
    for im in a:
        b = io.BytesIO()
        Image.fromarray(im).save(b, format="JPEG", quality=95)
        out.append(b.tell())
    return out


def bench(N, H, W, iters=20, host_iters=3):
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(0)).cuda()
    assert jpeg.sizes(x, 95).cpu().tolist() == host_sizes(x)
    for _ in range(3):
        jpeg.sizes(x, 95)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        jpeg.sizes(x, 95)
    e.record()
    torch.cuda.synchronize()
    dev_ms = s.elapsed_time(e) / iters
    host = []
    for _ in range(host_iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        host_sizes(x)
        host.append((time.perf_counter() - t) * 1e3)
    print(json.dumps({"shape": [N, 3, H, W], "quality": 95, "device_ms": round(dev_ms, 4), "host_ms": round(min(host), 2)}))


if __name__ == "__main__":
    bench(16, 512, 512)
    bench(16, 1024, 1024)
