"""CPU: the host half of the on-device JPEG encoder (adv_grpo_amd/jpeg.py, csrc/jpeg.hip) -- header and quantisation tables
against Pillow, the reward's registration, the C entry points' declarations and their refusals (which return before any
launch, so they run without a GPU), and the launcher's --reward-fn switch."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from adv_grpo_amd import jpeg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow(a, q):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="JPEG", quality=q)
    return b.getvalue()


def _lib():
    from adv_grpo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib, _lib.load()


@pytest.mark.parametrize("H,W,q", [(16, 16, 75), (48, 32, 1), (32, 48, 10), (512, 768, 95), (1024, 1024, 100), (64, 16, 50)])
def test_header_is_pillows_first_623_bytes(H, W, q):
    a = np.random.RandomState(H + W + q).randint(0, 256, (H, W, 3), dtype=np.uint8)
    h = jpeg.header(H, W, q)
    assert len(h) == jpeg.HEADER_BYTES == 623
    assert _pillow(a, q)[:623] == h


def test_quant_tables_match_pillow_for_every_quality():
    a = np.zeros((16, 16, 3), np.uint8)
    for q in range(1, 101):
        d = _pillow(a, q)
        luma, chroma = jpeg.quant_tables(q)
        # DQT payloads (zig-zag order) at the offsets of the 623-byte header: SOI + APP0 = 20 bytes, marker + length + id = 5
        assert list(d[25:89]) == [luma[jpeg.ZIGZAG[k]] for k in range(64)], q
        assert list(d[94:158]) == [chroma[jpeg.ZIGZAG[k]] for k in range(64)], q
    with pytest.raises(ValueError):
        jpeg.quant_tables(0)
    with pytest.raises(ValueError):
        jpeg.quant_tables(101)


def test_jpeg_compressibility_is_registered():
    from adv_grpo_amd import rewards
    assert "jpeg_compressibility" in rewards.score_functions
    assert "jpeg_compressibility" not in rewards._OUT_OF_SCOPE
    rewards.multi_score("cpu", {"jpeg_compressibility": 1})       # builds (the scorer touches no device until called)


def test_jpeg_symbols_are_declared_exported_and_typed():
    _l, lib = _lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advgrpo.h")).read(), flags=re.S)
    for n in ("advgrpo_jpeg_encode", "advgrpo_jpeg_workspace_bytes", "advgrpo_jpeg_max_file_bytes"):
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert hasattr(lib, n) and n in _l.SIGNATURES, n
    assert re.search(r"ADVGRPO_U8\s*=\s*3", txt)          # appended to the dtype enum
    assert lib.advgrpo_abi_version() == 1


def test_size_queries():
    _l, lib = _lib()
    for H, W in ((0, 16), (16, 0), (24, 16), (16, 40), (-16, 16)):
        assert lib.advgrpo_jpeg_max_file_bytes(H, W) == -1 and lib.advgrpo_jpeg_workspace_bytes(1, H, W) == -1
    assert lib.advgrpo_jpeg_workspace_bytes(0, 16, 16) == -1
    # bound: header + EOI + every entropy-coded byte stuffed, at <= 1697 bits per 8x8 block
    assert lib.advgrpo_jpeg_max_file_bytes(16, 16) == 623 + 2 + 2 * ((6 * 1697 + 7) // 8)
    assert lib.advgrpo_jpeg_workspace_bytes(4, 512, 512) > 4 * lib.advgrpo_jpeg_max_file_bytes(512, 512) // 2
    # the bound holds for the worst inputs Pillow sees: noise at quality 100
    a = np.random.RandomState(0).randint(0, 256, (64, 64, 3), dtype=np.uint8)
    assert len(_pillow(a, 100)) <= lib.advgrpo_jpeg_max_file_bytes(64, 64)


def test_encode_refusals_return_an_error_and_a_message():
    """Every refusal happens on the host before a launch (nothing here is dereferenced: the pointers are fake but aligned)."""
    _l, lib = _lib()
    P = 1 << 20
    N, H, W = 2, 32, 48
    ws = lib.advgrpo_jpeg_workspace_bytes(N, H, W)
    stride = lib.advgrpo_jpeg_max_file_bytes(H, W)
    ok = dict(images=P, dtype=_l.F32, layout=_l.JPEG_NCHW, N=N, H=H, W=W, quality=95, sizes=P, files=None, file_stride=0,
              workspace=P, workspace_bytes=ws, stream=None)
    bad = [dict(H=40), dict(W=24), dict(N=0), dict(H=0), dict(W=-16), dict(quality=0), dict(quality=101), dict(dtype=_l.F64),
           dict(dtype=7), dict(layout=2), dict(images=None), dict(sizes=None), dict(workspace=None), dict(workspace_bytes=ws - 1),
           dict(workspace=P + 16), dict(files=P, file_stride=stride - 1)]
    for over in bad:
        a = {**ok, **over}
        rc = lib.advgrpo_jpeg_encode(*a.values())
        msg = lib.advgrpo_last_error().decode()
        assert rc < 0 and "jpeg_encode" in msg, (over, rc, msg)


def test_launcher_reward_fn_switch():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train_sd3_fast
    finally:
        sys.path.pop(0)
    assert train_sd3_fast.parse_reward_fn("jpeg_compressibility=1") == {"jpeg_compressibility": 1}
    assert train_sd3_fast.parse_reward_fn("pickscore=0.5,ocr=0.5") == {"pickscore": 0.5, "ocr": 0.5}
    script = os.path.join(ROOT, "scripts", "train_sd3_fast.py")
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--reward-fn" in r.stdout
    cfg = os.path.join(ROOT, "config", "grpo.py") + ":pickscore_sd3_fast"
    for arg, needle in (("jpeg_compressibility", "NAME=W"), ("no_such_reward=1", "unknown reward"), ("aesthetic=1", "aesthetic")):
        r = subprocess.run([sys.executable, script, "--config", cfg, "--reward-fn", arg], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and needle in r.stderr, (arg, r.stderr[-2000:])
