"""On-device JPEG encoding, byte-exact with ``PIL.Image.save(format="JPEG", quality=q)``.

The reference's compressibility reward (adv_grpo/rewards.py:13-35) copies every image to the host, builds a PIL image
and saves it as a JPEG only to read the byte count.  ``advgrpo_jpeg_encode`` (csrc/jpeg.hip) computes the same file on
the device: the sizes stay there (no sync) and the files, when wanted, come back in one copy.

The header and the quality-scaled tables are also built here on the host (``header``, ``quant_tables``): they depend on
(H, W, quality) only and are what the tests hold against Pillow.
"""

import numpy as np
import torch

from . import _lib

HEADER_BYTES = 623
# ITU-T T.81 Annex K.1, natural order
LUMA_BASE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMA_BASE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zig-zag position -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# ITU-T T.81 Annex K.3: (table class << 4 | id, code counts per length 1..16, symbols)
_DC_VALS = tuple(range(12))
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), _DC_VALS),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), tuple(_AC_LUMA_VALS)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), _DC_VALS),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(_AC_CHROMA_VALS)),
)


def quant_tables(quality):
    """(luminance, chrominance) quantisation tables, natural order, for a quality 1..100 (IJG scaling, baseline-clamped)."""
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (LUMA_BASE, CHROMA_BASE))


def header(H, W, quality):
    """The 623 bytes before the entropy-coded segment: SOI, JFIF APP0, two DQT, SOF0 (4:2:0), four DHT, SOS."""
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t, q in enumerate(quant_tables(quality)):
        out += bytes((0xFF, 0xDB, 0, 67, t)) + bytes(q[ZIGZAG[k]] for k in range(64))
    out += bytes((0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))
    for tc, counts, vals in HUFFMAN_TABLES:
        n = 2 + 1 + 16 + len(vals)
        out += bytes((0xFF, 0xC4, n >> 8, n & 255, tc)) + bytes(counts) + bytes(vals)
    out += bytes((0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))
    assert len(out) == HEADER_BYTES
    return bytes(out)


def workspace_bytes(N, H, W):
    return _lib.load().advgrpo_jpeg_workspace_bytes(N, H, W)


def max_file_bytes(H, W):
    return _lib.load().advgrpo_jpeg_max_file_bytes(H, W)


def _device_images(images):
    """(tensor, dtype code, layout code): device NCHW f32 / bf16, device uint8 NHWC, or a host uint8 NHWC array."""
    if isinstance(images, np.ndarray):
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[-1] != 3:
            raise _lib.AdvGrpoError(f"jpeg: a host array must be uint8 [N,H,W,3] (got {images.dtype} {images.shape})")
        images = torch.from_numpy(np.ascontiguousarray(images)).to(torch.cuda.current_device())
    if not isinstance(images, torch.Tensor) or images.ndim != 4:
        raise _lib.AdvGrpoError("jpeg: images must be a 4-D tensor or array")
    images = images.contiguous()
    if images.dtype == torch.uint8:
        if images.shape[-1] != 3:
            raise _lib.AdvGrpoError(f"jpeg: uint8 images are NHWC [N,H,W,3] (got {tuple(images.shape)})")
        return images, _lib.U8, _lib.JPEG_NHWC
    if images.shape[1] != 3:
        raise _lib.AdvGrpoError(f"jpeg: float images are NCHW [N,3,H,W] (got {tuple(images.shape)})")
    return images, _lib.dtype_code(images.dtype), _lib.JPEG_NCHW


def _encode(images, quality, files):
    lib = _lib.load()
    x, dt, layout = _device_images(images)
    N, (H, W) = x.shape[0], (x.shape[1:3] if layout == _lib.JPEG_NHWC else x.shape[2:4])
    wsb = lib.advgrpo_jpeg_workspace_bytes(N, H, W)
    if wsb < 0:
        raise _lib.AdvGrpoError(f"jpeg: H and W must be positive multiples of 16 (got {H} x {W})")
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)        # current stream (caching allocator)
    sizes = torch.empty(N, dtype=torch.int64, device=x.device)
    stride = lib.advgrpo_jpeg_max_file_bytes(H, W) if files else 0
    buf = torch.empty(N, stride, dtype=torch.uint8, device=x.device) if files else None
    _lib.check(lib.advgrpo_jpeg_encode(_lib.ptr(x), dt, layout, N, H, W, int(quality), _lib.ptr(sizes), _lib.ptr(buf), stride,
                                       _lib.ptr(ws), wsb, _lib.stream_ptr()))
    return sizes, buf


def sizes(images, quality=95):
    """int64 device tensor [N]: the byte count of each image's JPEG file.  Asynchronous (no sync)."""
    return _encode(images, quality, False)[0]


def encode(images, quality=75):
    """list of N ``bytes``: each image's complete .jpg file (Pillow's default quality 75).  One synchronisation."""
    sz, buf = _encode(images, quality, True)
    host_sz = torch.empty(sz.shape, dtype=sz.dtype, pin_memory=True)
    host_buf = torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
    host_sz.copy_(sz, non_blocking=True)
    host_buf.copy_(buf, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    arr = host_buf.numpy()
    return [arr[i, :int(s)].tobytes() for i, s in enumerate(host_sz.tolist())]
