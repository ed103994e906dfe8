"""Float64 references of the transformer row kernels (csrc/norm.hip, csrc/train.hip) in plain torch, the error bounds the GPU parity
file holds them to, and the shape lists both test files walk (test helper, not a test module).

Every function is written from the comment at its kernel and the diffusers formula that comment cites; none calls adv_grpo_amd.
tests/test_row_kernel_reference_host.py pins the references against independent torch formulations and measures C_F32;
tests/test_gpu_row_kernels.py compares the kernels with them element by element.

The functions take a `dtype`: float64 is the reference, float32 is the emulation of the kernels' arithmetic that C_F32 is
measured with (same formulas, no bf16 roundings: `round_mid=False` where a formula has one inside).
"""
import math

import torch

F64 = torch.float64
BF16 = torch.bfloat16

# Unit roundoff of bfloat16: 8 significand bits, round to nearest even => |bf16(v) - v| <= 2^-8 |v|.
U_BF16 = 2.0 ** -8

# The float32 term of the bounds: |f32 evaluation - f64 evaluation| <= C_F32 * (sum of the magnitudes of the terms that are added to
# form the value).  Measured, not guessed: test_row_kernel_reference_host.py::test_float32_emulation_stays_within_c_f32 runs
# every formula below in torch float32 on the CPU over every shape list of this file and takes the worst ratio
# |f32 - f64| / magnitude.  Measured: 2.55e-7 = 2^-21.9 (rmsnorm_heads_bwd; the modulated norm 2.28e-7, its backward 1.99e-7, rmsnorm_heads
# 2.27e-7, rmsnorm_rows 2.24e-7, silu 1.28e-7 against (1 + |v|) |r|, its conditioning).  4 x 2^-21.9 = 2^-19.9, rounded up to a power of two:
C_F32 = 2.0 ** -19
# The factor 4 covers what the emulation does not share with the kernels: the summation order (64 lane partials and a shuffle tree
# against torch's vectorised sums) and rsqrtf / __expf against libm.  "Magnitudes of the terms" is taken literally: a mean is itself a
# sum, so it enters with mean|.| of its terms (its rounding error scales with those, not with the possibly cancelled result), and the
# normalised value (x - mean) * rstd enters as (|x| + mean|x|) * rstd -- which is what keeps the bound honest for rows whose mean is far
# from zero, where x - mean cancels.


def bf16r(t):
    """t rounded to bfloat16, back in t's dtype."""
    return t.to(BF16).to(t.dtype)


def mid_candidates(n):
    """The bf16 roundings of an intermediate n that the specification admits.  The kernels round the FLOAT32 value of n; where the
    float64 n lies within the float32 term of a rounding tie the two can fall to different neighbours, and both are correct.
    Returns (nominal, low, high); low and high differ from nominal only at such ties."""
    return bf16r(n), bf16r(n * (1.0 - C_F32)), bf16r(n * (1.0 + C_F32))


def batch_index(M, rows_per_batch):
    """Modulation / gate row of every token row: m // rows_per_batch, row 0 for all when rows_per_batch == 0."""
    if rows_per_batch <= 0:
        return torch.zeros(M, dtype=torch.long)
    return torch.arange(M) // rows_per_batch


def seg_rows(M, seg):
    """Buffer row of logical row m under seg = (rows, stride, off): (m // rows) * stride + off + m % rows."""
    m = torch.arange(M)
    if seg is None:
        return m
    r, s, o = seg
    return (m // r) * s + o + m % r


# ----------------------------------------------------------------------------------------------------------------- forward row ops
def layernorm_mod(x, w=None, b=None, scale=None, shift=None, scale2=None, shift2=None, rows_per_batch=0, eps=1e-6, dtype=F64):
    """(LN(x) [* w + b]) * (1 + scale[m // rows_per_batch]) + shift[...]; one output, or two when scale2 / shift2 are given.
    Returns (outs, mags): the unrounded values and the magnitudes of their added terms."""
    x = x.to(dtype)
    M = x.shape[0]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    n = d * rstd
    nmag = (x.abs() + x.abs().mean(-1, keepdim=True)) * rstd
    if w is not None:
        n, nmag = n * w.to(dtype), nmag * w.to(dtype).abs()
        if b is not None:
            n, nmag = n + b.to(dtype), nmag + b.to(dtype).abs()
    idx = batch_index(M, rows_per_batch)
    outs, mags = [], []
    for sc, sh in ((scale, shift), (scale2, shift2)):
        if sc is None:
            if not outs:
                outs.append(n), mags.append(nmag)
            continue
        s1, sh = 1.0 + sc.to(dtype)[idx], sh.to(dtype)[idx]
        outs.append(n * s1 + sh), mags.append(nmag * s1.abs() + sh.abs())
    return outs, mags


def rmsnorm_rows(x, w, eps=1e-6, dtype=F64, round_mid=True):
    """T5LayerNorm: bf16(x * rsqrt(mean x^2 + eps)) * w -- the value is cast to the weight dtype before the weight multiplies it.
    Returns the admissible values (nominal, low, high), see mid_candidates; one tensor three times when round_mid is False."""
    x, w = x.to(dtype), w.to(dtype)
    n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return tuple(c * w for c in (mid_candidates(n) if round_mid else (n, n, n)))


def rmsnorm_heads(buf, col0, nheads, w, heads_per_weight, eps=1e-6, seg=None, M=None, dtype=F64, round_mid=True):
    """Per 64-wide head: bf16(x * rsqrt(mean_64 x^2 + eps)) * w[head // heads_per_weight] on the heads at columns
    [col0, col0 + nheads * 64) of the rows seg maps.  Returns (rows, (nominal, low, high) each [M, nheads * 64], rs [M, nheads])."""
    M = buf.shape[0] if M is None else M
    rows = seg_rows(M, seg)
    x = buf[rows, col0:col0 + nheads * 64].to(dtype).reshape(M, nheads, 64)
    rs = torch.rsqrt((x * x).mean(-1) + eps)
    n = x * rs[..., None]
    wsel = w.to(dtype)[torch.arange(nheads) // heads_per_weight]          # [nheads, 64]
    cands = mid_candidates(n) if round_mid else (n, n, n)
    return rows, tuple((c * wsel).reshape(M, nheads * 64) for c in cands), rs


def timestep_embedding(t, dim, dtype=F64):
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0): [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(1e4) i / half)."""
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    a = t.to(dtype)[:, None] * f
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1)


def unary(x, act=None, x2=None, dtype=F64):
    """act(x [+ x2]); act None or "silu" (v / (1 + exp(-v))).  Returns (value, v)."""
    v = x.to(dtype)
    if x2 is not None:
        v = v + x2.to(dtype)
    if act in (None, "none"):
        return v, v
    assert act == "silu", act
    return v / (1.0 + torch.exp(-v)), v


def patchify(x):
    """[B, C, H, W] -> token rows [B * (H/2) * (W/2), C * 4], column = c * 4 + py * 2 + px (the Conv2d(C, D, k=2, s=2) weight flattened);
    values untouched, in x's dtype.  Index arithmetic, no reshape: the host test checks it against the reshape/permute form."""
    B, C, H, W = x.shape
    h, w = H // 2, W // 2
    tok = torch.arange(B * h * w)[:, None]
    col = torch.arange(C * 4)[None, :]
    return x[tok // (h * w), col // 4, 2 * ((tok // w) % h) + (col % 4) // 2, 2 * (tok % w) + col % 2]


def unpatchify(tokens, B, C, H, W):
    """Token rows [B * (H/2) * (W/2), 4 * C] with column = (py * 2 + px) * C + c (the order of proj_out's features) -> [B, C, H, W]."""
    w = W // 2
    b = torch.arange(B)[:, None, None, None]
    c = torch.arange(C)[None, :, None, None]
    y = torch.arange(H)[None, None, :, None]
    x = torch.arange(W)[None, None, None, :]
    return tokens[(b * (H // 2) + y // 2) * w + x // 2, ((y % 2) * 2 + x % 2) * C + c]


def gate_mul(x, gate, rows_per_batch, dtype=F64):
    """gate[m // rows_per_batch, :] * x[m, :] (unrounded: the product of two bf16 values is exact in f32 and f64)."""
    return x.to(dtype) * gate.to(dtype)[batch_index(x.shape[0], rows_per_batch)]


def transpose(x, R=None, seg=None, pad_to=64):
    """x [rows, C] -> [C, Rpad]: the R rows seg maps, transposed; columns [R, Rpad) zero."""
    R = x.shape[0] if R is None else R
    Rpad = (R + pad_to - 1) // pad_to * pad_to
    out = torch.zeros(x.shape[1], Rpad, dtype=x.dtype)
    out[:, :R] = x[seg_rows(R, seg)].t()
    return out


# ------------------------------------------------------------------------------------------------------------------- backward row ops
def layernorm_mod_bwd(x, dy0, scale0=None, dy1=None, scale1=None, dres=None, rows_per_batch=0, eps=1e-6):
    """dres + d/dx of sum(out0 * dy0 [+ out1 * dy1]) with out_k = LN(x) * (1 + scale_k[...]) + shift_k[...]: float64 autograd of the
    forward reference above (the shifts do not reach dx)."""
    xr = x.to(F64).requires_grad_(True)
    M, D = x.shape
    nb = int(batch_index(M, rows_per_batch).max()) + 1
    zero = torch.zeros(nb, D, dtype=F64)
    outs, _ = layernorm_mod(xr, scale=scale0 if scale0 is not None else zero, shift=zero, scale2=scale1 if dy1 is not None else None,
                            shift2=zero if dy1 is not None else None, rows_per_batch=rows_per_batch, eps=eps)
    loss = (outs[0] * dy0.to(F64)).sum()
    if dy1 is not None:
        loss = loss + (outs[1] * dy1.to(F64)).sum()
    (g,) = torch.autograd.grad(loss, xr)
    return g + (dres.to(F64) if dres is not None else 0.0)


def layernorm_mod_bwd_formula(x, dy0, scale0=None, dy1=None, scale1=None, dres=None, rows_per_batch=0, eps=1e-6, dtype=F64):
    """The closed form the kernel comment states: g = dy0 (1 + scale0) [+ dy1 (1 + scale1)], dx = rstd (g - mean g - xhat mean(g xhat)) + dres.
    Returns (dx, mag) with mag = rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dres|, |g| the sum over its two terms."""
    x = x.to(dtype)
    idx = batch_index(x.shape[0], rows_per_batch)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    g = dy0.to(dtype) * ((1.0 + scale0.to(dtype)[idx]) if scale0 is not None else 1.0)
    gabs = g.abs()
    if dy1 is not None:
        g1 = dy1.to(dtype) * (1.0 + scale1.to(dtype)[idx])
        g, gabs = g + g1, gabs + g1.abs()
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    mag = rstd * (gabs + gabs.mean(-1, keepdim=True) + xh.abs() * (gabs * xh.abs()).mean(-1, keepdim=True))
    if dres is not None:
        dx, mag = dx + dres.to(dtype), mag + dres.to(dtype).abs()
    return dx, mag


def rmsnorm_heads_bwd(x, dy, w, heads_per_weight, eps=1e-6):
    """Gradient w.r.t. x [M, nheads, 64] of sum(y * dy), y = x * rsqrt(mean_64 x^2 + eps) * w[head // heads_per_weight]: float64 autograd,
    the forward's bf16 rounding straight-through.  dy [M, nheads, 64]."""
    nheads = x.shape[1]
    xr = x.to(F64).requires_grad_(True)
    wsel = w.to(F64)[torch.arange(nheads) // heads_per_weight]
    y = xr * torch.rsqrt((xr * xr).mean(-1, keepdim=True) + eps) * wsel
    (g,) = torch.autograd.grad((y * dy.to(F64)).sum(), xr)
    return g


def rmsnorm_heads_bwd_formula(x, dy, w, heads_per_weight, eps=1e-6, dtype=F64):
    """Closed form at the kernel: g = dy w, dx = rs (g - xhat mean(g xhat)).  Returns (dx, mag_f32, mag_in):
    mag_f32 = rs (|g| + |xhat| mean|g xhat|), the magnitudes of the added terms;
    mag_in  = rs |xhat| (|mean(g xhat)| + mean|g xhat|), what one unit of relative error in xhat moves dx by.  The kernel does not see x: it
    recovers xhat as y / w from the forward's saved bf16 output y = bf16(bf16(x rs) w), two roundings, so its xhat carries a relative
    error d <= (1 + 2^-8)^2 - 1 once as the factor of the mean and once inside the mean."""
    nheads = x.shape[1]
    x, dy = x.to(dtype), dy.to(dtype)
    wsel = w.to(dtype)[torch.arange(nheads) // heads_per_weight]
    rs = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    xh, g = x * rs, dy * wsel
    mdot = (g * xh).mean(-1, keepdim=True)
    adot = (g * xh).abs().mean(-1, keepdim=True)
    return rs * (g - xh * mdot), rs * (g.abs() + xh.abs() * adot), rs * xh.abs() * (mdot.abs() + adot)


XHAT_IN_ERR = (1.0 + U_BF16) ** 2 - 1.0      # relative error of y / w against x rs (see rmsnorm_heads_bwd_formula)


# ----------------------------------------------------------------------------------------------------------------------- shape lists
LN_DS = (8, 504, 512, 520, 1536, 2048, 2056, 2432, 3072, 4096)        # <4> up to 2048, <8> above; partial chunks on both sides
LN_MS = (1, 3, 4, 5, 333)
LN_RPB = {1: 1, 3: 2, 4: 3, 5: 2, 333: 112}                            # rows_per_batch whose last batch is partial (M > 1)
LN_VARIANTS = ("table", "table_rpb0", "none", "affine", "w_only", "two", "xslice", "offset_mean")
RMS_ROWS_SHAPES = tuple((M, D) for D in (512, 4096) for M in (1, 77))
HEADS_NHEADS = (1, 7, 8, 9, 48, 76)
HEADS_COL0 = (0, 64)
HEADS_SEG = dict(B=2, Nt=5, S=13, Ni=3)                                 # seg = (Nt, S, Ni), M = B * Nt, buffer rows B * S
HEADS_BWD_NHEADS = (7, 8, 76)
LNB_DS = (256, 520, 1536, 2432, 3072, 4096)
LNB_MS = (5, 97)
LNB_RPB = {5: 2, 97: 33}
LNB_VARIANTS = ("scale0", "plain_dres", "two_dres", "two_strided", "gated1", "gated2_strided")
TS_T = (0.0, 1e-3, 1.0, 913.3488, 999.0, 1000.0)
TS_DIMS = (2, 256, 320)
UNARY_NS = (8, 2040, 2048 * 256 * 8 + 8)                                # the last: one chunk past a full grid => a second grid-stride trip
SILU_EDGES = (0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0)
PATCH_SHAPES = ((1, 16, 2, 2), (3, 16, 64, 64), (2, 16, 40, 24), (1, 64, 6, 10))
GATE_SHAPES = ((8, 7, 3), (1536, 37, 8), (2432, 11, 4))                # (D, M, rows_per_batch), M % rows_per_batch != 0
TR_RS = (1, 63, 64, 65, 205)
TR_CS = (8, 48, 64, 130)
TR_SEG = {1: (1, 4, 2), 63: (7, 11, 3), 64: (8, 8, 0), 65: (5, 9, 4), 205: (41, 50, 4)}   # R -> (rows, stride, off), R % rows == 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(*shape, g, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF16)


def ln_case(D, M, variant, device="cpu"):
    """Inputs of one layernorm_mod case as keyword arguments of ops.layernorm_mod / layernorm_mod above (tensors on `device`, views kept)."""
    g = _gen(1000 * D + 10 * M + LN_VARIANTS.index(variant))
    rpb = 0 if variant in ("table_rpb0", "none", "affine", "w_only") else LN_RPB[M]
    nb = (M + rpb - 1) // rpb if rpb else 1
    xw = _bf(M, D + 72, g=g, shift=100.0 if variant == "offset_mean" else 0.0).to(device)
    x = xw[:, 64:64 + D] if variant == "xslice" else xw[:, :D].clone(memory_format=torch.contiguous_format)
    kw = dict(x=x, rows_per_batch=rpb, eps=1e-6)
    if variant in ("affine", "w_only"):
        kw["w"] = _bf(D, g=g, scale=0.2, shift=1.0).to(device)
        if variant == "affine":
            kw["b"] = _bf(D, g=g, scale=0.2).to(device)
            kw["eps"] = 1e-5
    elif variant != "none":
        mods = _bf(nb, 6 * D, g=g, scale=0.5).to(device)                # the [B, 6 D] table: row pitch 6 D
        kw["shift"], kw["scale"] = mods[:, :D], mods[:, D:2 * D]
        if variant == "two":
            kw["shift2"], kw["scale2"] = mods[:, 3 * D:4 * D], mods[:, 4 * D:5 * D]
    return kw


def rms_rows_case(M, D, device="cpu"):
    g = _gen(7 * D + M)
    return dict(x=_bf(M, D, g=g, scale=3.0).to(device), w=_bf(D, g=g, scale=0.2, shift=1.0).to(device))


def heads_case(nheads, col0, seg, device="cpu"):
    """(buf, w, heads_per_weight, seg tuple or None, M): buf has one row and 72 columns more than the kernel may touch."""
    g = _gen(100 * nheads + col0 + (1 if seg else 0))
    s = HEADS_SEG
    M = s["B"] * s["Nt"]
    rows = s["B"] * s["S"] if seg else M + 1
    hpw = nheads // 2 if nheads % 2 == 0 else nheads
    buf = _bf(rows, col0 + nheads * 64 + 72, g=g, scale=2.0).to(device)
    w = _bf(nheads // hpw, 64, g=g, scale=0.1, shift=1.0).to(device)
    return buf, w, hpw, ((s["Nt"], s["S"], s["Ni"]) if seg else None), M


def lnb_case(D, M, variant, device="cpu"):
    """Keyword arguments of ops.layernorm_mod_bwd (without `out`); `gates` only for the gated variants.  The strided variants take x, dy0,
    dy1 and dres as column slices of wider buffers (dy0 | dy1 share a pitch, as the C entry requires)."""
    g = _gen(1000 * D + 10 * M + LNB_VARIANTS.index(variant) + 5)
    rpb = LNB_RPB[M]
    nb = (M + rpb - 1) // rpb
    strided = variant.endswith("strided")
    pad = 64 if strided else 0
    x = _bf(M, D + pad, g=g).to(device)[:, :D]
    dyw = _bf(M, 2 * D + pad, g=g).to(device)
    dy = _bf(M, D + pad, g=g).to(device)[:, :D]
    mods = _bf(nb, 6 * D, g=g, scale=0.5).to(device)
    kw = dict(x=x, dy0=dy, rows_per_batch=rpb)
    if variant != "plain_dres":
        kw["scale0"] = mods[:, D:2 * D]
    if variant in ("two_dres", "two_strided", "gated2_strided"):
        kw["dy0"], kw["dy1"], kw["scale1"] = dyw[:, :D], dyw[:, D:2 * D], mods[:, 4 * D:5 * D]
    if variant in ("plain_dres", "two_dres", "gated1", "gated2_strided"):
        kw["dres"] = _bf(M, D + pad, g=g).to(device)[:, :D]
    if variant == "gated1":
        kw["gates"] = [mods[:, 2 * D:3 * D]]
    if variant == "gated2_strided":
        kw["gates"] = [mods[:, 2 * D:3 * D], mods[:, 5 * D:6 * D]]
    return kw


def unary_case(n, device="cpu"):
    g = _gen(n % 9973)
    x = _bf(n, g=g, scale=4.0)
    e = torch.tensor(SILU_EDGES, dtype=BF16)
    x[:8] = e
    x[-8:] = e.flip(0)
    x2 = _bf(n, g=g)
    x2[:8] = 0          # the edge values stay what they are under x + x2: below v = -88.7 exp(-v) leaves the float32 range and
    x2[-8:] = 0         # v / (1 + exp(-v)) is -0 in float32 (torch's own float32 silu included) against -2e-37 in float64
    return x.to(device), x2.to(device)


def cpu(t):
    return None if t is None else t.detach().cpu()
