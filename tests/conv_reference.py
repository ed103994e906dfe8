"""Float64 reference of the 3x3 convolution family (csrc/conv_x3.hip, the implicit-conv loader of csrc/gemm.hip, gemm_epilogue_f32io and the
generic epilogue of gemm_device.hpp) in plain torch, the float32 emulation of the same arithmetic with named mutants, the bounds both are held
to, and the case lists (test helper, not a test module).

Written from the kernels' comments and the order of their epilogues; nothing here imports adv_grpo_amd.  tests/test_conv_reference_host.py pins
the reference against F.conv2d, measures C_CONV and runs the mutants; tests/test_gpu_conv_parity.py walks the same lists through the C entries
and compares element by element.  What gemm_reference.py already has (act_value, compare, SENTINEL, F32_TINY, U_BF16) is taken from there.

Forms and the products of one output element, from the pieces the kernel reads (x NHWC rows of three thirds, w [Cout, 9 taps, thirds]):
  bf16    x [C], w [9 C]                                   x w
  x3      x [hi | hi | lo] (generic tiles: the tripled K axis) or [hi | unread | lo] (dedicated kernel), w per tap [hi | lo | hi]
                                                            xh wh + xh wl + xl wh
  s2      x3 at stride 2 over an input of twice the size, zero row below and zero column to the right (F.pad (0, 1, 0, 1))
  f16x2   fp16 pair [hi | unread | lo] of prescale * x, one fp16 weight piece                   (xh + xl) w
  bf16x2  bf16 pair, one bf16 weight piece                                                      (xh + xl) w
  f16x1   the hi half of the fp16 pair only                                                     xh w
Order of one output element (gemm_epilogue_f32io; gemm_epilogue_rows / _frag for bf16):
  v = alpha * acc;  v += bias[n];  v = act(v);  v += residual[m, n];  store f32 | bf16 (round to nearest even) | fp16 pair of pair_prescale * v;
  gn_partial[m / 16, n / 4] = (sum, sum of squares) of the 16 x 4 stored values.
"""
import math
import zlib
from collections import namedtuple

import torch

from gemm_reference import F32_TINY, SENTINEL, U_BF16, act_value, bf16r, compare  # noqa: F401  (compare: re-exported for the two test modules)

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
F16 = torch.float16

# The float32 term of the bounds: |float32 evaluation - float64 evaluation| <= C_CONV * magnitude, the magnitude being the sum of the absolute
# values of the terms that are added to form the value (|alpha| sum |x||w| over every product of the form, + |bias|, carried through the
# activation, + |residual|).  Measured by test_conv_reference_host.py::test_float32_emulation_stays_within_c_conv over every narrow case of the
# list below (torch float32 on the CPU, nine taps x the form's products added one matrix product after the other, against float64):
# worst |f32 - f64| / magnitude = 8.38e-8 = 2^-23.5, set by `f16x1-x3-vec-bias_res` (C = 128, Cout = 132, bias + residual: one product per
# tap, so the fewest terms for a rounding to hide among; no activation case lies above it).  x 4 for what the emulation does not share with
# the kernels (the MFMA's summation order, __expf / v_rcp against libm) = 2^-21.5, rounded up to a power of two:
C_CONV = 2.0 ** -21
# Never above the order-independent worst case (K_eff + E) 2^-24 of K_eff products summed in any order plus E epilogue operations, at the
# largest K_eff of the list: three products x nine taps x 192 channels (the host test asserts it).  This is also as far as the constant may
# rise if a GPU path exceeds it without a fault in the kernel's code.
K_EFF_MAX = 3 * 9 * 192
N_EPI_OPS = 12        # alpha, bias, up to 8 operations of an activation, residual, pair scale

U_PAIR = 2.0 ** -22   # representation of a value by its fp16 pair: 22 significant bits
F16_SUB = 2.0 ** -25  # ... and where lo falls below fp16's normal range (2^-14) it is a multiple of 2^-24: half of that, in units of the scaled value
LO_UNIT = 2.0 ** -12  # the exact family's lo pieces: integers times this
GUARD = 8             # pixel rows of sentinel before and after every output
PAD = 2               # pixels / weight rows of NaN before and after every operand
GN_ROWS = 16          # pixels per gn_partial block (ADVGRPO_CONV_F16X2_STAT_ROWS); 4 channels per block

FORMS = ("bf16", "x3", "s2", "f16x2", "bf16x2", "f16x1")
PRODUCTS = {"bf16": 1, "x3": 3, "s2": 3, "f16x2": 2, "bf16x2": 2, "f16x1": 1}
X3_BM, X3_BN, WIDE_BN, WIDE_MIN_TILES = 192, 128, 256, 1024


# ------------------------------------------------------------------------------------------------------------------------------- cases
# form: see above.  tile: v5 (128x64) / v18 (128x128, 8 waves): the generic tiles with the implicit-conv loader; x3: the dedicated 192x128
#       kernel (for form s2 its strided instantiation); wide: its 192x256 instantiation.
# epi:  bf16 form: rows | frag_vec | frag_scalar (gemm_epilogue's three); every other form: vec | scalar | pair | gn (gemm_epilogue_f32io's
#       branches: float4, predicated scalars, fp16-pair output, float4 + block sums)
# H, W: the OUTPUT's height and width; ups: the input is [B, H/2, W/2] (fused nearest x2); form s2: the input is [B, 2H, 2W].
# route() below derives tile and epi from the conditions of gemm_variant, advgrpo_conv3x3_nhwc_x3, conv3x3_f16x2_launch and the epilogues.
Case = namedtuple("Case", "name form tile epi B H W C Cout ups family op bias act residual alpha prescale pair gn out_f32",
                  defaults=(False, "diffuse", "none", False, None, False, 1.0, 1.0, None, False, False))

OPS = {
    "none": dict(),
    "bias": dict(bias=True),
    "silu": dict(bias=True, act="silu"),
    "gelu_tanh": dict(bias=True, act="gelu_tanh"),
    "bias_res": dict(bias=True, residual=True),
    "full": dict(bias=True, act="silu", residual=True),
    "alpha": dict(bias=True, alpha=16.0, prescale=2.0 ** -4),
    "pair": dict(bias=True, pair=0.25),
    "gn": dict(bias=True, gn=True),
}
# geometry classes (B, Hout, Wout); the twin with the fused upsample keeps the output's shape where it is even and doubles it otherwise
GEOMETRIES = {
    "one": (1, 1, 1),            # a single pixel
    "w1": (2, 7, 1),             # W = 1: both column masks apply to every pixel
    "h1": (3, 1, 65),            # H = 1, 195 pixels: a tile boundary inside image 3
    "tiles": (2, 12, 16),        # two full tiles, the tile boundary on the image boundary: the halo pixel belongs to the previous image
    "tail3": (1, 13, 15),        # a last tile of 3 pixels, the tile boundary in the middle of a row
    "odd": (3, 9, 11),
}
UPS_ODD = (5, 6, 6)              # upsampled from (5, 3, 3): odd input width
S2_GEOMETRIES = {"s2one": (1, 1, 1), "s2w1": (2, 7, 1), "s2straddle": (3, 10, 13), "s2tile": (1, 12, 16)}     # inputs (1,2,2) (2,14,2) (3,20,26) (1,24,32)
# (form, tile) cells and the Cout values each walks through its geometries
CELLS = (("bf16", "v5", (3, 64)), ("bf16", "v18", (96, 136)), ("x3", "v5", (3, 64)), ("x3", "v18", (96,)), ("x3", "x3", (128, 132, 130, 256, 384)),
         ("f16x2", "x3", (128, 132, 130, 256, 384)), ("bf16x2", "x3", (132, 128, 384, 130, 256)), ("f16x1", "x3", (130, 256, 128, 384, 132)))
CHANNELS = (64, 128, 192)


def _epi(form, Cout, pair=None, gn=False):
    if form == "bf16":
        return "rows" if Cout % 8 == 0 else ("frag_vec" if Cout % 4 == 0 else "frag_scalar")
    if pair is not None:
        return "pair"
    if gn:
        return "gn"
    return "vec" if Cout % 4 == 0 else "scalar"


def _ups_shape(g):
    B, H, W = g
    return g if H % 2 == 0 and W % 2 == 0 else (B, 2 * H, 2 * W)


def _build_cases():
    cs = []

    def add(form, tile, g, C, Cout, tag, **kw):
        B, H, W = g
        op = kw.pop("op", "none")
        f = dict(OPS[op], op=op, **kw)
        epi = _epi(form, Cout, f.get("pair"), f.get("gn", False))
        cs.append(Case(f"{form}-{tile}-{epi}-{tag}", form, tile, epi, B, H, W, C, Cout, **f))

    # ---- the exact family carries the geometry: every (form x tile) cell through every class and its upsample twin; C and Cout rotate so
    # that 1, 2 and 3 slices per kernel row and every column-tile shape meet several geometries
    for form, tile, couts in CELLS:
        k = 0
        for gname, g in GEOMETRIES.items():
            for ups in (False, True):
                add(form, tile, _ups_shape(g) if ups else g, CHANNELS[k % 3], couts[k % len(couts)], gname + ("-ups" if ups else "") + "-exact",
                    ups=ups, family="exact", op="bias" if k % 2 else "none", out_f32=form == "bf16" and k % 4 >= 2)
                k += 1
        add(form, tile, UPS_ODD, CHANNELS[k % 3], couts[k % len(couts)], "upsodd-exact", ups=True, family="exact", op="bias_res")
    for k, (gname, g) in enumerate(S2_GEOMETRIES.items()):
        add("s2", "x3", g, CHANNELS[k % 3], (128, 132, 256, 384)[k], gname + "-exact", family="exact", op="bias" if k % 2 else "none")
    # exact pair output and block sums (tile boundary inside a row; gn needs 16 | H W)
    add("f16x2", "x3", (1, 13, 15), 64, 132, "tail3-exact", family="exact", op="pair")
    add("f16x1", "x3", (2, 12, 16), 128, 128, "tiles-exact", family="exact", op="pair", pair=4.0)
    add("f16x2", "x3", (2, 12, 16), 64, 132, "tiles-exact", family="exact", op="gn")
    # ---- the random family carries the epilogues, on the odd geometry (3, 9, 11) unless the operation needs another
    odd = GEOMETRIES["odd"]
    for Cout, tile in ((3, "v5"), (64, "v5"), (96, "v18")):
        for out_f32 in (False, True):
            for op in ("none", "bias", "silu", "gelu_tanh", "bias_res", "full"):
                if Cout == 64 and op in ("bias", "gelu_tanh"):
                    continue
                add("bf16", tile, odd, 64 if Cout != 96 else 128, Cout, op + ("-f32" if out_f32 else ""), op=op, out_f32=out_f32)
    add("bf16", "v18", odd, 192, 132, "full", op="full")                      # frag_vec: Cout % 8 == 4; two column tiles, the second of 4 columns
    for Cout, tile, ops in ((3, "v5", ("none", "full")), (64, "v5", ("bias", "silu")), (96, "v18", ("none", "bias", "silu", "gelu_tanh", "bias_res"))):
        for op in ops:
            add("x3", tile, odd, 64, Cout, op, op=op)
    for k, op in enumerate(("none", "bias", "silu", "gelu_tanh", "bias_res")):
        add("x3", "x3", odd, CHANNELS[(k + 2) % 3], (128, 132, 256, 384, 132)[k], op, op=op)
    add("x3", "x3", odd, 128, 130, "full", op="full")                         # the scalar branch of gemm_epilogue_f32io with every operation
    add("x3", "x3", _ups_shape(odd), 64, 132, "full-ups", op="full", ups=True)
    for gname, Cout, op in (("s2straddle", 128, "none"), ("s2straddle", 132, "bias"), ("s2tile", 256, "bias")):
        add("s2", "x3", S2_GEOMETRIES[gname], 192 if Cout == 256 else 64, Cout, f"{op}-{Cout}", op=op)
    for form in ("f16x2", "bf16x2", "f16x1"):
        for k, op in enumerate(("none", "bias", "silu", "gelu_tanh", "bias_res", "alpha")):
            add(form, "x3", odd, CHANNELS[k % 3], (128, 132, 256, 384, 132, 128)[k], op, op=op)
        add(form, "x3", odd, 128, 130, "full", op="full")
        add(form, "x3", (2, 12, 16), 64, 132 if form != "bf16x2" else 256, "gn", op="gn", act="silu", residual=True)
    add("f16x2", "x3", (3, 8, 16), 128, 128, "gn-b3", op="gn")               # image 1 = pixels 128..255 straddles the tile boundary at 192
    add("f16x2", "x3", (1, 13, 15), 64, 132, "pair", op="pair", act="silu", residual=True)
    add("f16x2", "x3", (2, 12, 16), 192, 256, "pair-ups", op="pair", ups=True, pair=1.0)
    add("f16x1", "x3", odd, 128, 128, "pair", op="pair", pair=4.0, alpha=16.0, prescale=2.0 ** -4)
    add("f16x1", "x3", (1, 13, 15), 64, 384, "pair-res", op="pair", residual=True)
    # ---- the wide tile: Cout % 256 == 0 and at least 1024 wide tiles (geometries below); C = 64 keeps the float64 reference cheap
    add("f16x2", "wide", WIDE_GN, 64, 256, "gn", op="gn")
    add("bf16x2", "wide", WIDE_UPS, 64, 256, "full-ups", op="full", ups=True)
    add("f16x1", "wide", WIDE_PAIR, 64, 256, "pair", op="pair")
    add("f16x2", "wide", WIDE_512, 64, 512, "pair-ups", op="pair", ups=True, pair=4.0)
    add("f16x1", "wide", WIDE_512, 64, 512, "ups-exact", family="exact", op="bias_res", ups=True)
    add("f16x2", "x3", BELOW_WIDE, 64, 256, "below-wide-exact", family="exact", op="bias")        # 1023 wide tiles: one short of the threshold
    return cs


# wide-tile geometries: ceil(M / 192) * (Cout / 256) >= 1024
WIDE_GN = (1, 464, 424)        # 196736 pixels = 1024 tiles + 128: 1025 tiles, the last one ragged; 16 | H W
WIDE_UPS = (2, 314, 314)       # 197192 pixels = 1027 tiles + 8, from a (2, 157, 157) input: odd input width
WIDE_PAIR = (3, 257, 255)      # 196605 pixels = 1023 tiles + 189: 1024 tiles, odd sizes, tile boundaries inside rows and across images
BELOW_WIDE = (1, 496, 396)     # 196416 pixels = 1023 tiles exactly: the narrow tile, two column tiles
WIDE_512 = (2, 222, 222)       # 98568 pixels = 513 tiles + 72, x 2 column tiles = 1028 wide tiles; input (2, 111, 111)

CASES = tuple(_build_cases())
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES), [n for n in CASE if sum(c.name == n for c in CASES) > 1]

# mutant of the float32 emulation -> the case on which it leaves the bound
MUTANTS = {
    "left_mask_dropped": "x3-x3-vec-odd-exact",
    "right_mask_dropped": "f16x1-x3-vec-w1-exact",
    "halo_from_previous_image": "bf16x2-x3-vec-tiles-exact",
    "taps_transposed": "bf16x2-x3-vec-odd-exact",
    "upsample_index_not_halved": "x3-x3-scalar-upsodd-exact",
    "stride2_pad_on_the_wrong_side": "s2-x3-vec-s2w1-exact",
    "xl_wh_dropped": "x3-x3-vec-none",
    "xl_wl_added": "x3-x3-vec-bias",
    "act_before_bias": "f16x2-x3-vec-silu",
    "alpha_after_bias": "f16x2-x3-vec-alpha",
    "residual_rounded_to_bf16": "x3-x3-vec-bias_res",
    "bf16_output_truncated": "bf16-v18-rows-bias",
    "last_column_tile_wrong_weight_row": "x3-x3-scalar-full",
    "pair_lo_from_unscaled_value": "f16x2-x3-pair-pair",
}


def k_eff(c):
    return PRODUCTS[c.form] * 9 * c.C


def in_shape(c):
    if c.form == "s2":
        return c.B, 2 * c.H, 2 * c.W
    return (c.B, c.H // 2, c.W // 2) if c.ups else (c.B, c.H, c.W)


def is_large(c):
    """The cases around the wide tile's threshold (about 100k and 200k pixels): evaluated on the GPU only."""
    return c.B * c.H * c.W >= 1 << 16


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def split_bf16(v):
    """hi = bf16(v), lo = bf16(v - hi): split8 of vae.hip."""
    hi = v.to(BF16)
    return hi, (v - hi.to(F32)).to(BF16)


def split_f16(v, prescale=1.0):
    """hi = f16(s v), lo = f16(s v - hi), saturated at the fp16 range: split8_f16 of vae.hip."""
    a = (v * prescale).clamp(-65504.0, 65504.0)
    hi = a.to(F16)
    return hi, (a - hi.to(F32)).to(F16)


def _nan_alloc(rows, cols, dtype):
    return torch.full((rows + 2 * PAD, cols), float("nan"), dtype=dtype)


def make(c, device="cpu"):
    """Every tensor of one case (generated on the CPU from the case's name, moved to `device`).  Returns a dict: x_alloc / w_alloc (NaN-filled,
    PAD pixels / weight rows on each side, the thirds the form does not read NaN as well) with the views x [pixels, thirds * C] and
    w [Cout, 9, thirds * C]; the pieces xh, xl, wh, wl as views of them (None where the form has none); bias, residual or None;
    out_alloc / pair_alloc / gn_alloc (sentinel-filled, GUARD pixel rows on each side) with the views out, pair_out, gn."""
    g = _gen(c.name)
    exact = c.family == "exact"
    B, Hin, Win = in_shape(c)
    P, M, C, N = B * Hin * Win, c.B * c.H * c.W, c.C, c.Cout
    f16 = c.form in ("f16x2", "f16x1")
    dt = F16 if f16 else BF16
    one_piece_w = c.form in ("bf16", "f16x2", "bf16x2", "f16x1")

    def ints(*shape, k=1):
        return torch.randint(-k, k + 1, shape, generator=g).to(F32)

    if exact:
        xh, xl = ints(P, C).to(dt), (ints(P, C) * LO_UNIT).to(dt)
        wh, wl = ints(N, 9, C).to(dt), (ints(N, 9, C) * LO_UNIT).to(dt)
    else:
        x = torch.randn(P, C, generator=g)
        w = torch.randn(N, 9, C, generator=g) * (1.5 / math.sqrt(9 * C)) * (1.0 + torch.arange(N)[:, None, None] / N)
        if one_piece_w:
            wh, wl = w.to(dt), None                                            # exact in the piece's format by construction
        else:
            wh, wl = split_bf16(w)
        xh, xl = split_f16(x, c.prescale) if f16 else split_bf16(x)
    if c.form == "bf16":
        x_alloc = _nan_alloc(P, C, dt)
        x_alloc[PAD:-PAD] = xh
    else:
        x_alloc = _nan_alloc(P, 3 * C, dt)
        v = x_alloc[PAD:-PAD]
        v[:, :C] = xh
        if c.form in ("x3", "s2") and c.tile in ("v5", "v18"):
            v[:, C:2 * C] = xh                                                 # order 0: the tripled K axis reads the middle third
        if c.form != "f16x1":
            v[:, 2 * C:] = xl
    if one_piece_w:
        w_alloc = _nan_alloc(N, 9 * C, dt)
        w_alloc[PAD:-PAD] = wh.reshape(N, 9 * C)
    else:
        w_alloc = _nan_alloc(N, 27 * C, dt)
        w_alloc[PAD:-PAD] = torch.cat([wh, wl, wh], dim=2).reshape(N, 27 * C)
    ep = BF16 if c.form == "bf16" else F32                                      # bias / residual travel in the activation's own width
    base = dict(x=x_alloc, w=w_alloc)
    if c.bias:
        base["bias"] = (ints(N, k=4) if exact else torch.randn(N, generator=g)).to(ep)
    if c.residual:
        base["residual"] = (ints(M, N, k=4) if exact else torch.randn(M, N, generator=g)).to(ep)
    if c.pair is None:
        base["out"] = torch.full((M + 2 * GUARD, N), SENTINEL, dtype=F32 if (c.out_f32 or c.form != "bf16") else BF16)
    else:
        base["pair"] = torch.full((M + 2 * GUARD, 3 * N), SENTINEL, dtype=F16)
    if c.gn:
        base["gn"] = torch.full((M // GN_ROWS + 2 * GUARD, N // 4 * 2), SENTINEL, dtype=F32)
    base = {k: t.to(device) for k, t in base.items()}
    xv = base["x"][PAD:-PAD]
    wv = base["w"][PAD:-PAD].view(N, 9, -1)
    inp = dict(case=c, x_alloc=base["x"], w_alloc=base["w"], x=xv, w=wv, bias=base.get("bias"), residual=base.get("residual"),
               out_alloc=base.get("out"), pair_alloc=base.get("pair"), gn_alloc=base.get("gn"), out=None, pair_out=None, gn=None)
    inp["xh"] = xv[:, :C]
    inp["xl"] = xv[:, 2 * C:] if c.form not in ("bf16", "f16x1") else None
    inp["wh"] = wv[:, :, :C]
    inp["wl"] = wv[:, :, C:2 * C] if not one_piece_w else None
    for key in ("out", "pair", "gn"):
        if base.get(key) is not None:
            inp["pair_out" if key == "pair" else key] = base[key][GUARD:-GUARD]
    return inp


# --------------------------------------------------------------------------------------------------------------------------- reference
Result = namedtuple("Result", "value mag stages")


def _coords(c, q):
    hw = c.H * c.W
    b = torch.div(q, hw, rounding_mode="floor")
    r = q - b * hw
    y = torch.div(r, c.W, rounding_mode="floor")
    return b, y, r - y * c.W


def tap_source(c, ky, kx, device="cpu", mutant=None):
    """(input pixel index [M], valid [M]) of tap (ky, kx) for every output pixel: the implicit-GEMM addressing.  Invalid taps read zero."""
    M = c.B * c.H * c.W
    _, Hin, Win = in_shape(c)
    m = torch.arange(M, device=device)
    b, y, x = _coords(c, m)
    if c.form == "s2":
        off = -1 if mutant == "stride2_pad_on_the_wrong_side" else 0           # F.pad (1, 0, 1, 0) instead of (0, 1, 0, 1)
        yy, xx = 2 * y + ky + off, 2 * x + kx + off
        valid = (yy >= 0) & (yy < Hin) & (xx >= 0) & (xx < Win)
        src = (b * Hin + yy) * Win + xx
        return src.clamp(0, c.B * Hin * Win - 1), valid

    def src_of(b, y, x, dy):
        """the dedicated kernel's pixel stage: output pixel (b, y, x) displaced by dy rows, its own column"""
        yy = y + dy
        ok = (yy >= 0) & (yy < c.H)
        if mutant == "halo_from_previous_image":                                # rows above the first one: the flat pixel one image row back
            prev = (yy < 0) & (b > 0)
            b, yy, ok = torch.where(prev, b - 1, b), torch.where(prev, yy + c.H, yy), ok | prev
        sy = yy.clamp(0, Hin - 1) if (mutant == "upsample_index_not_halved" and c.ups) else (yy >> 1 if c.ups else yy)
        sx = x >> 1 if c.ups else x
        return ((b * Hin + sy.clamp(0, Hin - 1)) * Win + sx).clamp(0, c.B * Hin * Win - 1), ok

    dy, dx = ky - 1, kx - 1
    xx = x + dx
    inside = (xx >= 0) & (xx < c.W)
    src, ok = src_of(b, y, xx.clamp(0, c.W - 1), dy)
    valid = ok & inside
    if (mutant == "left_mask_dropped" and dx < 0) or (mutant == "right_mask_dropped" and dx > 0):
        # the shifted LDS row holds flat pixel m + dx (clamped to the launch's pixels), displaced by dy: the neighbouring image row's pixel
        nb, ny, nx = _coords(c, (m + dx).clamp(0, M - 1))
        nsrc, nok = src_of(nb, ny, nx, dy)
        src, valid = torch.where(inside, src, nsrc), torch.where(inside, valid, nok)
    return src, valid


def _products(inp, mutant=None):
    """[(x piece, w piece)] in the order the kernels issue them."""
    c = inp["case"]
    xh, xl, wh, wl = inp["xh"], inp["xl"], inp["wh"], inp["wl"]
    if c.form in ("x3", "s2"):
        ps = [(xh, wl), (xl, wh), (xh, wh)]
        if mutant == "xl_wh_dropped":
            ps.pop(1)
        if mutant == "xl_wl_added":
            ps.append((xl, wl))
        return ps
    if c.form in ("f16x2", "bf16x2"):
        return [(xh, wh), (xl, wh)]
    return [(xh, wh)]


def accumulate(inp, dtype=F64, mutant=None, order=0, want_mag=True):
    """(acc, sum |x||w|) [M, Cout] as nine gathered matrix products per piece product.  order 1: another summation order (taps reversed, the
    products of a tap reversed) for the exact family's proof."""
    c = inp["case"]
    dev = inp["x"].device
    M, N = c.B * c.H * c.W, c.Cout
    acc = torch.zeros(M, N, dtype=dtype, device=dev)
    amag = torch.zeros(M, N, dtype=dtype, device=dev) if want_mag else None
    prods = _products(inp, mutant)
    rows = torch.arange(N, device=dev)
    if mutant == "last_column_tile_wrong_weight_row" and N % X3_BN:
        rows = torch.where(rows >= N - N % X3_BN, (rows + 1).clamp(max=N - 1), rows)       # the ragged tile's rows counted from one too far
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    if order:
        taps, prods = taps[::-1], prods[::-1]
    for ky, kx in taps:
        src, valid = tap_source(c, ky, kx, dev, mutant)
        t = kx * 3 + ky if mutant == "taps_transposed" else ky * 3 + kx
        keep = valid.to(dtype)[:, None]
        gathered = {}
        for xp, wp in prods:
            if id(xp) not in gathered:
                gathered[id(xp)] = xp[src].to(dtype) * keep
            X, Wt = gathered[id(xp)], wp[rows, t].to(dtype).T
            acc += X @ Wt
            if want_mag:
                amag += X.abs() @ Wt.abs()
    return acc, amag


def reference(inp, dtype=F64, mutant=None, order=0):
    """The whole epilogue of one case on make()'s tensors, on their device.  dtype float64: the reference; float32: the emulation of the
    kernels' arithmetic (`mutant` names a deliberate defect).  Returns Result: value / mag [M, Cout] (the unrounded output and the magnitude
    of its added terms; mag None for float32) and `stages`: the magnitude after every stage (for the exact family's 2^24 ceiling)."""
    c = inp["case"]
    want_mag = dtype == F64
    acc, amag = accumulate(inp, dtype, mutant, order, want_mag)
    alpha = float(c.alpha)
    v = alpha * acc
    mag = abs(alpha) * amag if want_mag else torch.zeros_like(v)
    stages = [amag, mag] if want_mag else []
    pre_act_done = False
    if inp["bias"] is not None:
        b = inp["bias"].to(dtype)
        if mutant == "alpha_after_bias":
            v = alpha * (acc + b)
        elif mutant == "act_before_bias":
            v = act_value(v, c.act)[0] + b
            pre_act_done = True
        else:
            v = v + b
        mag = mag + b.abs()
        stages.append(mag)
    if c.act is not None and not pre_act_done:
        y, dabs, emag = act_value(v, c.act)
        v, mag = y, dabs * mag + emag
        stages.append(mag)
    if inp["residual"] is not None:
        r = inp["residual"].to(dtype)
        v = v + (bf16r(r) if mutant == "residual_rounded_to_bf16" else r)
        mag = mag + r.abs()
        stages.append(mag)
    return Result(v, mag if want_mag else None, stages if want_mag else None)


def _bf16_truncate(t):
    return (t.to(F32).view(torch.int32) & -65536).view(F32).to(BF16)


def pair_of(v32, scale, mutant=None):
    """The fp16 pair of scale * v as the pair-output epilogue forms it (float32 in)."""
    hi, lo = split_f16(v32, scale)
    if mutant == "pair_lo_from_unscaled_value":
        lo = (v32.clamp(-65504.0, 65504.0) - hi.to(F32)).to(F16)
    return hi, lo


def gn_sums(stored, dtype=F64):
    """[M / 16, Cout / 4 * 2]: (sum, sum of squares) per block of 16 pixels x 4 channels of the stored output."""
    M, N = stored.shape
    v = stored.to(dtype).view(M // GN_ROWS, GN_ROWS, N // 4, 4)
    return torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1).reshape(M // GN_ROWS, N // 4 * 2)


def store(inp, res, mutant=None):
    """The allocations a kernel that computed `res` (float32) would leave: {"out" | "pair"[, "gn"]: tensor}, fresh copies of make()'s."""
    c = inp["case"]
    N = c.Cout
    v = res.value.to(F32)
    got = {}
    if c.pair is None:
        a = torch.full_like(inp["out_alloc"], SENTINEL)
        a[GUARD:-GUARD] = _bf16_truncate(v) if (mutant == "bf16_output_truncated" and a.dtype == BF16) else v.to(a.dtype)
        got["out"] = a
    else:
        a = torch.full_like(inp["pair_alloc"], SENTINEL)
        hi, lo = pair_of(v, c.pair, mutant)
        a[GUARD:-GUARD, :N], a[GUARD:-GUARD, 2 * N:] = hi, lo
        got["pair"] = a
    if c.gn:
        a = torch.full_like(inp["gn_alloc"], SENTINEL)
        a[GUARD:-GUARD] = gn_sums(got["out"][GUARD:-GUARD], F32)
        got["gn"] = a
    return got


def verify(inp, ref, got):
    """Compare whole allocations `got` ({"out" | "pair"[, "gn"]}) with the float64 reference `ref`: {key: (worst error / bound, elements outside
    their bound)}.  Guard rows and the unwritten third of pair rows have bound zero (they must hold the sentinel), and so has every element of
    the exact family."""
    c = inp["case"]
    N = c.Cout
    exact = c.family == "exact"
    val, mag = ref.value, ref.mag
    res = {}
    if c.pair is None:
        a = got["out"]
        want = torch.full(a.shape, SENTINEL, dtype=F64, device=a.device)
        bound = torch.zeros_like(want)
        is_bf16 = a.dtype == BF16
        want[GUARD:-GUARD] = bf16r(val) if (exact and is_bf16) else val
        if not exact:
            bound[GUARD:-GUARD] = C_CONV * mag + (U_BF16 * val.abs() if is_bf16 else 0.0) + F32_TINY
        res["out"] = compare(a, want, bound)
    else:
        a = got["pair"]
        bits = a.view(torch.int16)
        clean = torch.full_like(a, SENTINEL).view(torch.int16)
        outside = int((bits[:GUARD] != clean[:GUARD]).sum() + (bits[-GUARD:] != clean[-GUARD:]).sum() +
                      (bits[GUARD:-GUARD, N:2 * N] != clean[GUARD:-GUARD, N:2 * N]).sum())
        hi, lo = a[GUARD:-GUARD, :N], a[GUARD:-GUARD, 2 * N:]
        if exact:                                                               # the value is exact in float32: the pair's bits are determined
            wh, wl = pair_of(val.to(F32), c.pair)
            ratio, bad = 0.0, int((hi.view(torch.int16) != wh.view(torch.int16)).sum() + (lo.view(torch.int16) != wl.view(torch.int16)).sum())
        else:
            dec = (hi.to(F64) + lo.to(F64)) / c.pair
            ratio, bad = compare(dec, val, C_CONV * mag + U_PAIR * val.abs() + F16_SUB / c.pair + F32_TINY)
        res["pair"] = (ratio, bad + outside)
    if c.gn:
        a = got["gn"]
        stored = got["out"][GUARD:-GUARD].to(F64)
        want = torch.full(a.shape, SENTINEL, dtype=F64, device=a.device)
        bound = torch.zeros_like(want)
        want[GUARD:-GUARD] = gn_sums(stored)
        # order-independent: 64 values added in any order (63 additions); the squares one rounding each on top (and one for the pairing)
        mags = gn_sums(stored.abs())
        b = bound[GUARD:-GUARD].view(-1, N // 4, 2)
        b[..., 0] = 63 * 2.0 ** -24 * mags.view(-1, N // 4, 2)[..., 0] + F32_TINY
        b[..., 1] = 65 * 2.0 ** -24 * mags.view(-1, N // 4, 2)[..., 1] + F32_TINY
        res["gn"] = compare(a, want, bound)
    return res


# ------------------------------------------------------------------------------------------------------------------ which kernel a case reaches
def conv_variant(Cout):
    """gemm.hip's gemm_variant with conv = 1 (product build): the generic tile of a convolution."""
    return 5 if Cout <= 64 else 18


def route(c):
    """(tile, epilogue branch) of one case, or (None, "refuse") where the entry must refuse it: from the conditions of advgrpo_conv3x3_nhwc_x3 /
    _s2_nhwc_x3 / conv3x3_two_products (gemm.hip), conv3x3_f16x2_launch (conv_x3.hip), gemm_epilogue and gemm_epilogue_f32io.  Every pointer
    make() hands out is 16-byte aligned (PAD and GUARD are whole rows of at least 16 bytes times 8) and every pitch is the dense one."""
    M, N = c.B * c.H * c.W, c.Cout
    generic = "v%d" % conv_variant(N)
    if c.form == "bf16":
        rows_ok = N % 8 == 0                                                    # epilogue_rows_ok: ldc = ldr = N, aligned pointers
        return generic, "rows" if rows_ok else ("frag_vec" if N % 4 == 0 else "frag_scalar")
    vec = N % 4 == 0                                                            # gemm_epilogue_f32io: (ldc | ldr) % 4 == 0 and N % 4 == 0
    if c.form == "x3":
        if c.pair is not None or c.gn or c.alpha != 1.0:
            return None, "refuse"
        return (generic if N < 128 else "x3"), "vec" if vec else "scalar"
    if c.form == "s2":
        if N < 128 or not vec or c.act or c.residual or c.ups or c.pair is not None or c.gn:
            return None, "refuse"
        return "x3", "vec"
    if N < 128 or (c.pair is not None and (c.gn or not vec or c.form == "bf16x2")) or (c.gn and (c.H * c.W % GN_ROWS or not vec)):
        return None, "refuse"
    tiles_m = (M + X3_BM - 1) // X3_BM
    wide = N % WIDE_BN == 0 and tiles_m * (N // WIDE_BN) >= WIDE_MIN_TILES
    return "wide" if wide else "x3", "pair" if c.pair is not None else ("gn" if c.gn else ("vec" if vec else "scalar"))
