"""Float64 reference of the bf16 GEMM family's whole fused epilogue (csrc/gemm.hip, gemm_device.hpp, gemm8p*.hip) in plain torch, the
float32 emulation of the same arithmetic with named mutants, the bounds both are held to, and the case lists (test helper, not a test module).

Written from the kernels' comments and the order of their epilogues; nothing here imports adv_grpo_amd.  tests/test_gemm_reference_host.py
pins the reference against independent torch formulations, measures C_GEMM and runs the mutants; tests/test_gpu_gemm_parity.py walks the same
lists through the kernels and compares element by element.

Order of one output element, as in gemm_epilogue_rows / gemm_epilogue_frag / p8_epilogue:
  v = alpha * sum_k A[a_row(m), k] W[n, k];  v += bias[n];  aux_out[out_row(m), n] = bf16(v);  v = act(v)  or  v *= d(aux_in[out_row(m), n]);
  v *= gate[m // gate_rows, n];  v += residual[out_row(m), n];  C[out_row(m), n] = v   (bf16: round to nearest even; f32: as is).
accumulate: C += alpha * acc (f32, nothing else);  split-K: the same value, the partial sums added atomically in no fixed order.
f2bf (common.hpp) is round-to-nearest-even on both sides of its #if: the device side is the hardware conversion v_cvt_pk_bf16_f32, the host side
adds 0x7fff + lsb before the shift; torch's .to(bfloat16) is RNE as well, which is what the `exact` family compares with.
"""
import math
import zlib
from collections import namedtuple

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16

U_BF16 = 2.0 ** -8            # unit roundoff of bfloat16 (8 significand bits, round to nearest even)

# The float32 term of the bounds: |float32 evaluation - float64 evaluation| <= C_GEMM * magnitude, the magnitude being the sum of the absolute
# values of the terms that are added to form the value (|alpha| sum_k |a||w| + |bias|, carried through activation, gate and residual).
# Measured by test_gemm_reference_host.py::test_float32_emulation_stays_within_c_gemm over every case of the lists below (torch float32 on the
# CPU against float64): worst |f32 - f64| / magnitude = 2.17e-7 = 2^-22.1, set by the plain product of `v26-bmm2` (8192 x 1024 x 64, two
# batches: the largest number of elements; no activation case lies above it).  x 4 for what the emulation does not share with the kernels (the
# MFMA's summation order: 32-term dot products added to the accumulator K / 32 times; __expf / v_rcp / erff against libm) = 2^-20.1, rounded up
# to a power of two:
C_GEMM = 2.0 ** -20
# Never above the order-independent worst case (K + E) 2^-24 of K products summed in any order plus E epilogue operations, at the largest K of
# the lists (the host test asserts it).
K_MAX = 1536
N_EPI_OPS = 12        # alpha, bias, up to 8 operations of an activation, gate, residual

# Absolute floor of every bound: far below -88 the sigmoid of the tanh GELU leaves the normal range of float32 (exp overflows, the reciprocal is a
# denormal or zero) while float64 still has 1e-40; bounds relative to the value cannot cover that, 2^-100 does and is nothing otherwise.
F32_TINY = 2.0 ** -100

SENTINEL = -31744.0   # exact in bf16 and f32; fills every allocation around the views the kernels write

ACTS = ("gelu_tanh", "gelu", "silu", "quick_gelu")
D_ACTS = ("dgelu_tanh", "dgelu", "mul_aux")
_SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def bf16r(t):
    return t.to(BF16).to(t.dtype)


def seg_rows(M, seg, device="cpu"):
    """Buffer row of logical row m under seg = (rows, stride, off): (m // rows) * stride + off + m % rows."""
    m = torch.arange(M, device=device)
    if seg is None:
        return m
    r, s, o = seg
    return (m // r) * s + o + m % r


# ------------------------------------------------------------------------------------------------------------------------- activations
def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def act_value(x, act):
    """(act(x), |act'(x)|, magnitude of the terms added inside the evaluation of act at x)."""
    if act == "gelu_tanh":          # 0.5 x (1 + tanh e) written as the kernels evaluate it, x * sigmoid(2 e): no cancellation of 1 + tanh for x << 0
        e = _SQRT_2_OVER_PI * (x + 0.044715 * x ** 3)
        r = torch.sigmoid(2.0 * e)
        y = x * r
        d = r * (1.0 + (1.0 - r) * x * 2.0 * _SQRT_2_OVER_PI * (1.0 + 3 * 0.044715 * x * x))
        return y, d.abs(), (1.0 + 2.0 * e.abs()) * y.abs()          # the exponent's rounding is a relative error 2|e| u of the sigmoid
    if act == "gelu":
        er = torch.erf(x / math.sqrt(2.0))
        y = 0.5 * x * (1.0 + er)
        return y, (0.5 * (1.0 + er) + x * _phi(x)).abs(), 0.5 * x.abs() * (1.0 + er.abs())      # 1 + erf cancels for x << 0
    if act in ("silu", "quick_gelu"):
        s = 1.0 if act == "silu" else 1.702
        sg = torch.sigmoid(s * x)
        y = x * sg
        return y, (sg * (1.0 + s * x * (1.0 - sg))).abs(), (1.0 + s * x.abs()) * y.abs()
    raise KeyError(act)


def dact_value(z, act):
    """(f(z), magnitude of the terms added inside f) for the epilogues v *= f(aux_in)."""
    if act == "mul_aux":
        return z, torch.zeros_like(z)
    if act == "dgelu_tanh":         # r (1 + (1 - r) q), r = sigmoid(2 e), q = z (2c + 6ac z^2): the form of dgelu_tanh_f32; 1 - r has the terms 1 and r
        e = _SQRT_2_OVER_PI * (z + 0.044715 * z ** 3)
        r = torch.sigmoid(2.0 * e)
        q = z * 2.0 * _SQRT_2_OVER_PI * (1.0 + 3 * 0.044715 * z * z)
        return r * (1.0 + (1.0 - r) * q), (1.0 + 2.0 * e.abs()) * r * (1.0 + 2.0 * q.abs())
    if act == "dgelu":
        er = torch.erf(z / math.sqrt(2.0))
        cur = z * _phi(z)
        return 0.5 * (1.0 + er) + cur, 0.5 * (1.0 + er.abs()) + cur.abs() * (1.0 + 0.5 * z * z)
    raise KeyError(act)


# ------------------------------------------------------------------------------------------------------------------------------- cases
# kernel: the tile variant that runs (ids of gemm.hip: 0 = 128x128 4 waves, the split-K kernel; 1 = 128x64; 2 = 64x128; 15 = 128x128 8 waves;
#         26 = 192x128; 30 = the 256x256 eight-phase kernel)
# path:   rows | frag_vec | frag_scalar (gemm_epilogue's three), acc_vec | acc_scalar (fixed-order accumulate), splitk (atomics),
#         8p:<class> (epi_class of gemm8p.hip), refuse:<pitch> (stopped by gemm_prepare)
# route() below derives both from the conditions of gemm_variant, gemm_prepare, gemm8p_ok, epilogue_rows_ok, vec_ok and epi_class applied to
# the tensors make() builds; the host test asserts that every case reaches what it declares.
Case = namedtuple("Case", "name kernel path M N K family entry act bias alpha gate_rows residual inplace out_f32 seg a_seg pad bias_off "
                          "aux_out aux_pad res_pad gate_pad accumulate splitk batch confirm",
                  defaults=("diffuse", "gemm", None, False, 1.0, None, False, False, False, None, None, 0, 0, False, 0, 0, 0, False, 1, 1, True))
Pair = namedtuple("Pair", "name kernel first second")

# what an epilogue "operation" of the matrix means (fields of Case)
OPS = {
    "none": dict(),
    "bias": dict(bias=True, alpha=0.5),
    "gelu_tanh": dict(bias=True, act="gelu_tanh"),
    "gelu": dict(bias=True, act="gelu"),
    "silu": dict(bias=True, act="silu"),
    "quick_gelu": dict(bias=True, act="quick_gelu"),
    "aux": dict(bias=True, act="gelu_tanh", aux_out=True, entry="train"),
    "dgelu_tanh": dict(act="dgelu_tanh", entry="train"),
    "dgelu": dict(act="dgelu", entry="train", alpha=2.0),
    "mul_aux": dict(bias=True, act="mul_aux", entry="train"),
    "gate_res": dict(bias=True, gate_rows=50, residual=True, inplace=True),
    "f32": dict(bias=True, out_f32=True, alpha=2.0),
    "full": dict(bias=True, act="silu", alpha=0.5, gate_rows=16, residual=True, inplace=True),
}
ALL_OPS = ("none", "bias", "gelu_tanh", "gelu", "silu", "quick_gelu", "aux", "dgelu_tanh", "dgelu", "mul_aux", "gate_res", "f32")
FEW_OPS = ("none", "full", "f32")
# how a shape with N % 8 == 0 is steered onto each path: rows = every pitch and pointer 16-byte aligned; frag_vec = out / residual pitch N + 4
# (4 mod 8; the bias-only case instead views its bias 4 elements into a buffer: 8-byte aligned); frag_scalar = out / residual pitch N + 2 (2 mod 4)
PATH_PAD = {"rows": 0, "frag_vec": 4, "frag_scalar": 2}


def _matrix(tag, kernel, M, N, K, ops, paths=("rows", "frag_vec", "frag_scalar"), **kw):
    out = []
    for path in paths:
        for op in ops:
            f = dict(OPS[op], **kw)
            pad, boff, p = PATH_PAD[path], 0, path
            if path == "frag_vec" and op == "bias":
                pad, boff = 0, 4
            if path == "frag_scalar" and (f.get("aux_out") or f.get("act") in D_ACTS):
                p = "refuse:ldc"                     # the pitch 2 mod 4 with aux: refused by gemm_prepare, nothing is launched
            if N % 8:
                pad = 0                              # a ragged N is on the scalar path by itself
            out.append(Case(f"{tag}-{path}-{op}", kernel, p, M, N, K, pad=pad, bias_off=boff, **f))
    return out


def _exact(c, **kw):
    return c._replace(name=c.name + "-exact", family="exact", **kw)


def _build_cases():
    cs = []
    # ---- variant 15 (128x128, 8 waves): M > 64 < N, plain, below 8192 rows.  (130, 192, 64): two row tiles (the second 2 rows), two column
    # tiles (the second half full), ONE k-tile.  The whole operation list on all three paths.
    v15 = _matrix("v15", 15, 130, 192, 64, ALL_OPS)
    cs += v15
    cs += [_exact(c, alpha=a) for c, a in zip([c for c in v15 if c.name.endswith(("-none", "-mul_aux")) and not c.path.startswith("refuse")],
                                              (1.0, 0.5, 2.0, 1.0, 0.5))]
    cs += [c._replace(name=c.name + "-cancel", family="cancelling") for c in v15 if c.name.endswith("-none")]
    # (257, 136, 192): three row tiles (the last 1 row), a second column tile of 8 columns, THREE k-tiles (odd: the last one sits in buffer 0)
    cs += _matrix("v15b", 15, 257, 136, 192, ("full",))
    # row maps with segment / gate boundaries inside a 16-row slab: seg rows 21 and 50, gate_rows 50 and 16
    for path in ("rows", "frag_vec", "frag_scalar"):
        pad = PATH_PAD[path]
        cs.append(Case(f"v15-{path}-seg21", 15, path, 126, 192, 128, bias=True, gate_rows=50, residual=True, inplace=True, seg=(21, 30, 5), pad=pad))
        cs.append(Case(f"v15-{path}-seg50-aseg", 15, path, 150, 192, 64, bias=True, act="gelu_tanh", gate_rows=16, residual=True, seg=(50, 64, 7),
                       a_seg=(50, 61, 3), pad=pad, res_pad=pad))
    cs.append(_exact(cs[-2]))
    cs.append(Case("v15-rows-aseg21", 15, "rows", 126, 192, 64, a_seg=(21, 30, 5)))
    # refusals of the fix: aux or a d-activation with a residual / gate pitch that is 2 mod 4 (the output pitch is the matrix's refuse:ldc)
    cs.append(Case("v15-refuse-ldr", 15, "refuse:ldr", 130, 192, 64, entry="train", bias=True, act="gelu_tanh", aux_out=True, residual=True, res_pad=2))
    cs.append(Case("v15-refuse-gate", 15, "refuse:gate_stride", 130, 192, 64, entry="train", act="mul_aux", gate_rows=50, gate_pad=2))
    # ---- fixed-order accumulate into a non-zero f32 C (variant 15; gemm_epilogue_frag's first branch): float4 and scalar forms
    for path, pad in (("acc_vec", 4), ("acc_scalar", 2)):
        cs.append(Case(f"v15-{path}", 15, path, 130, 192, 192, entry="train", out_f32=True, accumulate=True, alpha=0.5, pad=pad))
        cs.append(_exact(cs[-1]))
    # ---- variant 1 (128x64): N <= 64
    cs += _matrix("v1", 1, 130, 64, 64, FEW_OPS)
    cs += [Case("v1-rows-m1-none", 1, "rows", 1, 8, 64), Case("v1-rows-m1-full", 1, "rows", 1, 8, 64, **OPS["full"])]
    cs += _matrix("v1r", 1, 77, 13, 192, FEW_OPS, paths=("frag_scalar",))          # N = 13: ragged quads, three k-tiles
    cs += [_exact(c) for c in cs if c.name in ("v1-rows-none", "v1r-frag_scalar-none")]
    cs.append(Case("v1-k1536-diffuse", 1, "frag_scalar", 77, 13, 1536, out_f32=True))
    cs.append(Case("v1-k1536-exact", 1, "frag_scalar", 77, 13, 1536, family="exact", bias=True, alpha=2.0))
    # ---- variant 2 (64x128): M <= 64 < N
    cs += _matrix("v2", 2, 48, 192, 128, FEW_OPS)
    cs += _matrix("v2m1", 2, 1, 200, 64, ("full",))
    cs += [_exact(c) for c in cs if c.name in ("v2-frag_vec-none",)]
    # ---- variant 0 (128x128, 4 waves): split-K only (gemm_variant's `plain` is false); 5 k-tiles over 2, 3 and 7 splits (7 > 5: two splits
    # get no k-tile and return before the first load).  C holds a running sum; atomics, no other epilogue.
    for sk in (2, 3, 7):
        cs.append(Case(f"v0-splitk{sk}", 0, "splitk", 130, 192, 320, entry="train", out_f32=True, splitk=sk, alpha=0.5, pad=2 if sk == 3 else 0, confirm=False))
    cs.append(_exact(cs[-1]))
    cs.append(cs[-3]._replace(name="v0-splitk3-cancel", family="cancelling"))
    # ---- variant 26 (192x128) at 8192 rows: where gemm8p_ok fails
    big = dict(M=8192, N=1024, K=64, confirm=False)
    cs.append(Case("v26-rows-seg8", 26, "rows", family="exact", bias=True, gate_rows=50, residual=True, inplace=True, seg=(8, 9, 1), **big))
    cs.append(Case("v26-rows-gate8", 26, "rows", bias=True, act="gelu_tanh", gate_rows=8, residual=True, **big))      # the fall-back from 30
    cs.append(Case("v26-frag_vec", 26, "frag_vec", pad=4, **OPS["full"], **big))
    cs.append(Case("v26-frag_scalar-n1026", 26, "frag_scalar", 8192, 1026, 64, family="exact", bias=True, alpha=0.5, confirm=False))
    cs.append(Case("v26-bmm2", 26, "rows", 8192, 1024, 64, entry="bmm", batch=2, alpha=0.25))
    # ---- variant 30 (eight-phase, 256x256): every epilogue class; (8192, 1024, 64) = 32 x 4 full tiles of ONE k-tile,
    # (8232, 1032, 192) = a 33rd row tile of 40 rows, a 5th column tile of 8 columns, THREE k-tiles
    e = dict(M=8192, N=1024, K=64)
    r = dict(M=8232, N=1032, K=192)
    cs.append(Case("v30-plain", 30, "8p:plain", family="exact", entry="desc", **e))
    cs.append(Case("v30-bias", 30, "8p:bias", bias=True, alpha=0.5, **e))
    cs.append(Case("v30-bias_gelu", 30, "8p:bias_gelu", bias=True, act="gelu_tanh", **e))
    cs.append(Case("v30-bias_gate_res", 30, "8p:bias_gate_res", bias=True, gate_rows=50, residual=True, inplace=True, **e))
    cs.append(Case("v30-bias_gelu_aux", 30, "8p:bias_gelu_aux", entry="train", bias=True, act="gelu_tanh", aux_out=True, **e))
    cs.append(Case("v30-dgelu", 30, "8p:dgelu", entry="train", act="dgelu_tanh", **e))
    cs.append(Case("v30-generic-f32-silu", 30, "8p:generic", bias=True, act="silu", out_f32=True, gate_rows=16, **e))
    cs.append(Case("v30-generic-mul_aux", 30, "8p:generic", family="exact", entry="desc", bias=True, act="mul_aux", residual=True, alpha=0.5, **e))
    cs.append(Case("v30r-plain", 30, "8p:plain", entry="desc", a_seg=(21, 30, 5), **r))
    cs.append(Case("v30r-bias_gate_res-seg21", 30, "8p:bias_gate_res", family="exact", bias=True, gate_rows=16, residual=True, inplace=True,
                   seg=(21, 30, 5), alpha=2.0, **r))
    cs.append(Case("v30r-generic-quick_gelu", 30, "8p:generic", bias=True, act="quick_gelu", residual=True, seg=(50, 64, 7),
                   **dict(r, M=8200)))                                                # 8200 = 164 segments of 50 rows
    return cs


CASES = tuple(_build_cases())
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# paired launches (gemm_grouped of two): the second problem differs in M, N, K and epilogue and runs on the FIRST problem's tile variant
PAIRS = (
    Pair("pair15", 15, CASE["v15-rows-gate_res"], Case("pair15-b", 15, "frag_scalar", 77, 200, 192, bias=True, act="silu", out_f32=True, pad=2)),
    Pair("pair26", 26, CASE["v26-frag_vec"], Case("pair26-b", 26, "rows", 130, 192, 128, bias=True, act="gelu", alpha=0.5)),
    # below 8192 rows and of another class than the first: the pair runs EPI_GENERIC
    Pair("pair30", 30, CASE["v30-bias_gelu"], Case("pair30-b", 30, "8p:bias_gate_res", 126, 192, 128, bias=True, gate_rows=50, residual=True,
                                                    inplace=True, seg=(21, 30, 5))),
)
# fused QK-norm against the unfused pair of kernels, bit for bit (its values are covered through rmsnorm_heads' own float64 test)
RMS_CASES = (("rms15", 15, 130, 192, 64, None), ("rms26", 26, 8192, 1024, 64, (8, 9, 1)), ("rms30", 30, 8192, 1024, 64, None))

# mutant of the float32 emulation -> the case on which it leaves the bound
MUTANTS = {
    "drop_last_substep": "v15b-rows-full",
    "double_substep": "v15-frag_vec-f32",
    "alpha_after_bias": "v15-rows-bias",
    "bias_next_column": "v1r-frag_scalar-f32",
    "act_before_bias": "v15-frag_scalar-silu",
    "gelu_swapped": "v15-rows-gelu_tanh",
    "aux_after_act": "v15-frag_vec-aux",
    "dact_skipped": "v15-rows-dgelu_tanh",
    "gate_row_plus_one": "v15-frag_vec-seg21",
    "residual_unsegmented": "v15-rows-seg21",
    "seg_off_dropped": "v15-frag_scalar-seg21",
    "a_seg_off_dropped": "v15-rows-aseg21",
    "batch_stride_c_for_a": "v26-bmm2",
    "accumulate_overwrites": "v15-acc_vec",
}


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _alloc(rows, cols, dtype, batch=1):
    return torch.full((batch, rows + 2, cols), SENTINEL, dtype=dtype)


def make(c, device="cpu"):
    """Every tensor of one case (generated on the CPU from the case's name, moved to `device`).  Returns a dict:
    a [B, rowsA, K] view of pitch K + 8, w [B, N, K], a_rows / out_rows (the two row maps), bias / gate / residual / aux_in views or None,
    out_alloc [B, rows + 2, pitch] with its initial contents (sentinel around the view; random data inside it for in-place, accumulate and
    split-K) and out = out_alloc[:, 1:-1, :N]; aux_alloc / aux likewise."""
    g = _gen(c.name)
    M, N, K, B = c.M, c.N, c.K, c.batch
    exact, cancel = c.family == "exact", c.family == "cancelling"

    def rnd(*shape, scale=1.0, lo=-8, hi=8):
        if exact:
            return torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        return torch.randn(*shape, generator=g) * scale

    a_rows, out_rows = seg_rows(M, c.a_seg), seg_rows(M, c.seg)
    rows_a, rows_o = int(a_rows.max()) + 2, int(out_rows.max()) + 2          # one spare row behind the last mapped one
    a_buf = rnd(B, rows_a, K + 8).to(BF16)
    wf = rnd(B, N, K, scale=1.5 / math.sqrt(K))
    if not exact:
        wf = wf * (1.0 + torch.arange(N)[None, :, None] / N)                   # asymmetric rows, as test_gemm_plain
    w = wf.to(BF16)
    if cancel:                                                                   # columns k and k + K/2 cancel exactly; column 0 carries the result
        h = K // 2
        a_buf[:, :, h:K] = a_buf[:, :, :h]
        w[:, :, h:] = -w[:, :, :h]
        a_buf[:, :, h] = 0
        a_buf[:, :, 0] = (torch.randn(B, rows_a, generator=g) * 2.0 ** -14).to(BF16)
    pitch = N + c.pad
    dt = F32 if c.out_f32 else BF16
    out_alloc = _alloc(rows_o, pitch, dt, B)
    view = out_alloc[:, 1:-1, :N]
    if c.inplace:
        view.copy_(rnd(B, rows_o, N).to(dt))
    if c.accumulate or c.splitk > 1:
        view.copy_(torch.zeros(B, rows_o, N) if cancel else rnd(B, rows_o, N, scale=4.0))
    # the buffers the views below are cut from; moved to the device whole so that pitches and offsets survive
    base = dict(a=a_buf, w=w, out=out_alloc)
    if c.bias:
        base["bias"] = rnd(c.bias_off + N + 8).to(BF16)
    if c.gate_rows is not None:
        G = (M - 1) // c.gate_rows + 2 if c.gate_rows else 1
        base["gate"] = rnd(G, N + c.gate_pad, lo=-4, hi=4).to(BF16)
    if c.residual and not c.inplace:
        base["residual"] = rnd(1, rows_o, N + c.res_pad).to(BF16)
    if c.act in D_ACTS:
        base["aux_in"] = rnd(1, rows_o, N + c.aux_pad, scale=1.5).to(BF16)
    if c.aux_out:
        base["aux"] = _alloc(rows_o, N + c.aux_pad, BF16)
    base = {k: v.to(device) for k, v in base.items()}
    inp = dict(case=c, a_buf=base["a"], a=base["a"][:, :, :K], w=base["w"], a_rows=a_rows.to(device), out_rows=out_rows.to(device),
               out_alloc=base["out"], out=base["out"][:, 1:-1, :N], bias=None, bias_next=None, gate=None, residual=None, aux_in=None,
               aux_alloc=base.get("aux"), aux=None)
    if c.bias:
        inp["bias"], inp["bias_next"] = base["bias"][c.bias_off:c.bias_off + N], base["bias"][c.bias_off + N]
    if c.gate_rows is not None:
        inp["gate"] = base["gate"][:, :N]
    if c.inplace:
        inp["residual"] = inp["out"]
    elif c.residual:
        inp["residual"] = base["residual"][:, :, :N]
    if c.act in D_ACTS:
        inp["aux_in"] = base["aux_in"][:, :, :N]
    if c.aux_out:
        inp["aux"] = base["aux"][:, 1:-1, :N]
    inp["init"] = inp["out_alloc"].clone()
    return inp


# --------------------------------------------------------------------------------------------------------------------------- reference
Result = namedtuple("Result", "value mag aux aux_mag out_rows stages")


def reference(inp, dtype=F64, mutant=None):
    """The whole epilogue of one case on make()'s tensors, on their device.  dtype float64: the reference; float32: the emulation of the
    kernels' arithmetic (no rounding to bf16 inside; `mutant` names a deliberate defect).  Returns Result: value / mag [B, M, N] (the unrounded
    output and the magnitude of its added terms), aux / aux_mag (the pre-activation) or None, out_rows, and `stages`: the magnitude after every
    epilogue stage (for the exact family's 2^24 ceiling)."""
    c = inp["case"]
    dev = inp["a"].device
    M, N, K, B = c.M, c.N, c.K, c.batch
    a_rows, out_rows = inp["a_rows"], inp["out_rows"]
    if mutant == "a_seg_off_dropped":
        a_rows = seg_rows(M, (c.a_seg[0], c.a_seg[1], 0), dev)
    if mutant == "seg_off_dropped":
        out_rows = seg_rows(M, (c.seg[0], c.seg[1], 0), dev)
    init = inp["init"][:, 1:-1, :N]
    A = inp["a"][:, a_rows].to(dtype)
    if mutant == "batch_stride_c_for_a":         # batch b's A read at b * strideC instead of b * strideA (wrapped into the allocation)
        flat = inp["a_buf"].reshape(-1)
        lda = inp["a"].stride(1)
        span = (int(a_rows.max()) + 1) * lda
        A = torch.stack([torch.as_strided(flat, (int(a_rows.max()) + 1, K), (lda, 1), (b * inp["out_alloc"].stride(0)) % (flat.numel() - span))[a_rows]
                         for b in range(B)]).to(dtype)
    W = inp["w"].to(dtype)
    acc = A @ W.transpose(1, 2)
    amag = A.abs() @ W.abs().transpose(1, 2)
    if mutant == "drop_last_substep":
        acc = acc - A[..., K - 32:] @ W[..., K - 32:].transpose(1, 2)
    if mutant == "double_substep":
        acc = acc + A[..., 32:64] @ W[..., 32:64].transpose(1, 2)
    alpha = float(c.alpha)
    stages = [amag]
    v, mag = alpha * acc, abs(alpha) * amag
    stages.append(mag)
    if c.accumulate or c.splitk > 1:
        c0 = init[:, out_rows].to(dtype)
        value = v if mutant == "accumulate_overwrites" else c0 + v
        mag = mag + c0.abs()
        stages.append(mag)
        return Result(value, mag, None, None, out_rows, stages)
    bias = inp["bias"]
    act = c.act
    if mutant == "gelu_swapped":
        act = {"gelu_tanh": "gelu", "gelu": "gelu_tanh"}[act]
    pre_act_done = False
    if bias is not None:
        b = bias.to(dtype).clone()
        if mutant == "bias_next_column":
            b[N - 1] = inp["bias_next"].to(dtype)
        if mutant == "alpha_after_bias":
            v = alpha * (acc + b)
        elif mutant == "act_before_bias":
            v = act_value(v, act)[0] + b
            pre_act_done = True
        else:
            v = v + b
        mag = mag + b.abs()
        stages.append(mag)
    aux, aux_mag = (v, mag) if c.aux_out else (None, None)
    if act in D_ACTS:
        z = inp["aux_in"][:, out_rows].to(dtype)
        if mutant != "dact_skipped":
            f, fmag = dact_value(z, act)
            v, mag = v * f, mag * f.abs() + v.abs() * fmag
    elif act is not None and not pre_act_done:
        y, dabs, emag = act_value(v, act)
        v, mag = y, dabs * mag + emag
    if mutant == "aux_after_act":
        aux = v
    stages.append(mag)
    if inp["gate"] is not None:
        m = torch.arange(M, device=dev) + (1 if mutant == "gate_row_plus_one" else 0)
        gi = m // c.gate_rows if c.gate_rows else torch.zeros_like(m)
        gt = inp["gate"].to(dtype)[gi]
        v, mag = v * gt, mag * gt.abs()
        stages.append(mag)
    if inp["residual"] is not None:
        rr = torch.arange(M, device=dev) if mutant == "residual_unsegmented" else out_rows
        rs = (init if c.inplace else inp["residual"])[:, rr].to(dtype)
        v, mag = v + rs, mag + rs.abs()
        stages.append(mag)
    return Result(v, mag, aux, aux_mag, out_rows, stages)


def expected(inp, ref):
    """The whole allocations a correct run leaves: (want, bound) per buffer, `want` the float64 contents (initial contents where nothing is
    written: guard rows, pad columns, rows no segment maps) and `bound` the admissible deviation (zero off the written elements and for the
    exact family).  Returns {"out": (want, bound)[, "aux": (want, bound)]}."""
    c = inp["case"]
    N = c.N
    res = {}
    for key, alloc, val, mag, is_bf16 in (("out", inp["init"], ref.value, ref.mag, not c.out_f32),
                                           ("aux", inp["aux_alloc"], ref.aux, ref.aux_mag, True)):
        if val is None or alloc is None:
            continue
        want = (inp["init"] if key == "out" else torch.full_like(alloc, SENTINEL)).to(F64)
        bound = torch.zeros_like(want)
        val = val.to(F64)
        if c.family == "exact":
            tol = torch.zeros_like(val)
            if is_bf16:
                val = bf16r(val)
        else:
            tol = C_GEMM * mag.to(F64) + (U_BF16 * val.abs() if is_bf16 else 0.0) + F32_TINY
        want[:, 1:-1, :N][:, ref.out_rows] = val
        bound[:, 1:-1, :N][:, ref.out_rows] = tol
        res[key] = (want, bound)
    return res


def compare(got, want, bound):
    """(worst error / bound over the elements with a bound, count of elements outside their bound) -- elements with bound zero must be equal."""
    got = got.to(F64)
    err = (got - want).abs()
    bad = ~(err <= bound)                       # (NaN counts)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    return ratio, int(bad.sum())


# ------------------------------------------------------------------------------------------------------------------ which branch a case reaches
def _a16(t):
    return t is None or (t.storage_offset() * t.element_size()) % 16 == 0


def gemm_variant(M, N, K, batch, plain):
    """gemm.hip's gemm_variant (product build, no convolution); batch includes the split-K factor."""
    if N <= 64:
        return 1
    if M <= 64:
        return 2
    if plain and M >= 8192 and N >= 1024:
        return 30 if batch == 1 else 26
    assert not (plain and batch == 1 and M >= 1024 and K >= 1024), "the reward towers' tile heuristic is outside these lists"
    return 15 if plain else 0


def route(inp, rms=False):
    """(kernel, path) of one problem launched alone, from the conditions in gemm_prepare, gemm8p_ok, epilogue_rows_ok, vec_ok and epi_class."""
    c = inp["case"]
    M, N, K = c.M, c.N, c.K
    out, res, gate, aux_in, aux = inp["out"], inp["residual"], inp["gate"], inp["aux_in"], inp["aux"]
    ldc, ldr = out.stride(1), res.stride(1) if res is not None else 0
    gs = gate.stride(0) if gate is not None else 0
    auxt = aux if aux is not None else aux_in
    ld_aux = auxt.stride(1) if auxt is not None else 0
    strideC = out.stride(0) if c.batch > 1 else 0
    has_aux = auxt is not None
    if has_aux and (ld_aux % 4 or N % 4):
        return None, "refuse:aux"
    if has_aux or c.act in D_ACTS:
        for name, p in (("ldc", ldc), ("ldr", ldr), ("gate_stride", gs)):
            if p % 4:
                return None, "refuse:" + name
    ptrs16 = all(_a16(t) for t in (out, inp["bias"], gate, res, aux, aux_in))
    v = gemm_variant(M, N, K, c.batch * c.splitk, c.splitk == 1)
    ok8 = (not (c.seg and c.seg[0] < 16) and not (gate is not None and 0 < (c.gate_rows or 0) < 16) and c.batch == 1 and c.splitk == 1 and
           not c.accumulate and N % 8 == 0 and (ldc | ldr | gs | ld_aux) % 8 == 0 and ptrs16)
    if v == 30 and c.accumulate:
        v = 15
    if v == 30 and not ok8:
        v = 26 if M >= 8192 and N >= 1024 else 15
    if rms and v == 1:
        v = 15
    if v == 30:
        return v, "8p:" + epi_class(c, rms)
    rows_ok = c.splitk == 1 and not c.accumulate and N % 8 == 0 and (ldc | ldr | gs | ld_aux | strideC) % 8 == 0 and ptrs16
    if rows_ok:
        return v, "rows"
    vec_ok = (ldc | ldr | gs) % 4 == 0 and N % 4 == 0
    if c.accumulate:
        return v, "acc_vec" if vec_ok and (out.storage_offset() * 4) % 16 == 0 else "acc_scalar"
    if c.splitk > 1:
        return v, "splitk"
    return v, "frag_vec" if vec_ok else "frag_scalar"


def epi_class(c, rms=False):
    """gemm8p.hip's epi_class, by name."""
    if c.out_f32:
        return "generic"
    f = []
    if c.bias:
        f.append("bias")
    if rms:
        f.append("rms")
    if c.act == "gelu_tanh":
        f.append("gelu")
    elif c.act == "dgelu_tanh":
        f.append("dgelu")
    elif c.act is not None:
        return "generic"
    has_gate, has_res = c.gate_rows is not None, c.residual
    if has_gate and has_res:
        f.append("gate_res")
    elif has_gate or has_res:
        return "generic"
    if c.aux_out:
        f.append("aux")
    name = "_".join(f) or "plain"
    return name if name in ("plain", "bias", "bias_rms", "bias_gelu", "bias_gate_res", "bias_gelu_aux", "dgelu") else "generic"


def pair_route(first, second):
    """(kernel, path of the first, path of the second) of gemm_grouped([first, second]): both problems run on the first one's tile variant;
    the eight-phase kernel runs the common class, or EPI_GENERIC when the two differ."""
    va, pa = route(first)
    vb, pb = route(second)
    if va == 30:
        cb = epi_class(second["case"])
        return va, pa, "8p:" + cb
    return va, pa, pb
