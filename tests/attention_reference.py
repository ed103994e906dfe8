"""Float64 references of the attention forward and backward (csrc/attention*.hip) in plain torch, the error bounds the GPU parity file
holds the kernels to, a float32 emulation of the kernels' stated arithmetic with a list of named mutants, and the input families and case
lists both test files walk (test helper, not a test module; never imports adv_grpo_amd).

tests/test_attention_reference_host.py pins the references against torch's scaled_dot_product_attention and its float64 autograd, runs the
emulation and the mutants against the bounds and measures C_ATT; tests/test_gpu_attention_parity.py compares the kernels element by element.

Layout everywhere: q [B, Sq, H * hd], k / v [B, Skv, H * hd] bf16 (column slices of one packed buffer); the references work on
[B, H, S, hd] float64 views and return [B, Sq, H * hd] / [B, H, Sq] like the entries.
"""
import math
import zlib

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)

# Unit roundoff of bfloat16: 8 significand bits, round to nearest even => |bf16(v) - v| <= 2^-8 |v|.
U_BF16 = 2.0 ** -8

# The float32 term of the bounds: |f32 evaluation - f64 evaluation| <= C_ATT * magnitude, the magnitudes being the ones written at each bound
# below.  Measured, not guessed: test_attention_reference_host.py::test_float32_evaluation_stays_within_c_att runs forward() and backward() of
# this file in torch float32 (no bf16 rounding inside) over every case list and family and takes the worst |f32 - f64| / magnitude.
# Measured: 1.14e-7 = 2^-23.1 (lse; out 8.4e-8, dv 6.0e-8, dq 5.0e-8, dk 4.1e-8).  4 x 2^-23.1 = 2^-21.1, rounded up to a power of two:
C_ATT = 2.0 ** -21
# The factor 4 covers what the float32 evaluation does not share with the kernels: the summation order (MFMA accumulation in 16- or
# 32-deep steps and lane partials against torch's blocked sums) and v_exp_f32 / v_log_f32 against libm.


def bf16r(t):
    return t.to(BF16).to(t.dtype)


def heads(x, H, dtype=F64):
    """[B, S, H * hd] -> [B, H, S, hd] in dtype."""
    B, S, HD = x.shape
    return x.to(dtype).view(B, S, H, HD // H).transpose(1, 2)


def unheads(x):
    B, H, S, D = x.shape
    return x.transpose(1, 2).reshape(B, S, H * D)


def default_scale(hd):
    return hd ** -0.5


def _live_mask(Sq, Skv, causal, bias):
    """Keys a query sees: causal hides keys > query index; a bias below -1000 is a mask (HF-style finite mask: exp of it is an exact zero in
    float32 and float64 alike, so such a key carries neither weight nor magnitude)."""
    live = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        live &= ~torch.ones(Sq, Skv, dtype=torch.bool).triu(1)
    if bias is not None:
        live = live[None] & (bias > -1000.0)
    return live


# ------------------------------------------------------------------------------------------------------------------------- forward
def forward(q, k, v, H, scale=None, bias=None, causal=False, dtype=F64):
    """w = softmax(scale q k^T [+ bias] [causal]); o = w v; lse2 = log2 sum_j exp2(log2e (scale s + bias)).
    Returns a dict: o [B, Sq, H hd], lse2 [B, H, Sq] (unrounded, in dtype), A = w |v| (same shape as o), T [B, H, Sq] the score magnitude
    of the row in base-2 units, max over the keys the row sees of log2e (scale sum_d |q_d k_jd| + |bias_ij|), and w itself."""
    hd = q.shape[-1] // H
    scale = default_scale(hd) if scale is None else scale
    qh, kh, vh = heads(q, H, dtype), heads(k, H, dtype), heads(v, H, dtype)
    Sq, Skv = qh.shape[2], kh.shape[2]
    t = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    tmag = (qh.abs() @ kh.abs().transpose(-1, -2)) * (scale * LOG2E)
    if bias is not None:
        t = t + bias.to(dtype)[None] * LOG2E
        tmag = tmag + bias.to(dtype).abs()[None] * LOG2E
    live = _live_mask(Sq, Skv, causal, bias)
    if causal:
        t = t.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool).triu(1), float("-inf"))
    m = t.amax(-1, keepdim=True)
    e = torch.exp2(t - m)
    l = e.sum(-1, keepdim=True)
    w = e / l
    return dict(o=unheads(w @ vh), lse2=(m + torch.log2(l)).squeeze(-1), A=unheads(w @ vh.abs()),
                T=tmag.masked_fill(~live, 0.0).amax(-1), w=w)


def forward_bounds(ref, H):
    """(out bound [B, Sq, H hd], lse bound [B, H, Sq]) for the arithmetic the kernel comments state: bf16 q, k, v; scores, exponentials, row
    maximum and row sum in float32; probabilities rounded to bf16 before P V; the quotient rounded to bf16.
      out:  |got - o| <= U |o|            the output rounding
                       + 2 U A            P V with each probability off by U relative (numerator: U sum_j w |v| = U A), and one more U A
                                          admitted for the row sum (l adds the unrounded exponentials in every kernel here, which makes this
                                          half slack; the issue's stated form is kept)
                       + C (1 + T) A      float32: a probability is exp2 of a float32 score whose absolute error scales with the score
                                          magnitude T (the dot product's terms, the scale, the bias), i.e. relative C T on the probability,
                                          and the sums over keys add C A
      lse2: |got - lse2| <= C (1 + T + |lse2|): the same score error moves log2 of the sum by as much; log2 and the final add are float32.
            No bf16 term: the row sum adds the exponentials before they are rounded (attention.hip: psum += e / ps2 += a ahead of the
            pack; attention_pipe.hip and attention_d128.hip: lsum in tile_probs ahead of att_cvt_pk)."""
    T = ref["T"]                                                        # [B, H, Sq]
    B, Sq, HD = ref["o"].shape
    Trow = T.transpose(1, 2)[..., None].expand(B, Sq, H, HD // H).reshape(B, Sq, HD)
    out = U_BF16 * ref["o"].abs() + 2 * U_BF16 * ref["A"] + C_ATT * (1.0 + Trow) * ref["A"]
    return out, C_ATT * (1.0 + T + ref["lse2"].abs())


def forward_f32_magnitudes(ref, H):
    """The magnitudes C_ATT multiplies (out, lse)."""
    T = ref["T"]
    B, Sq, HD = ref["o"].shape
    Trow = T.transpose(1, 2)[..., None].expand(B, Sq, H, HD // H).reshape(B, Sq, HD)
    return (1.0 + Trow) * ref["A"], 1.0 + T + ref["lse2"].abs()


# ------------------------------------------------------------------------------------------------------------------------ backward
def backward(q, k, v, o, d_o, lse2, H, scale=None, dtype=F64):
    """Defined on what the entry receives: P = exp2(log2e scale s - lse2), D = sum_d o d_o, dP = d_o v^T, dS = P (dP - D),
    dv = P^T d_o, dk = scale dS^T q, dq = scale dS k.  Returns a dict with dq, dk, dv ([B, S, H hd]) and the magnitudes:
    P, dS, G = sum_d |d_o| |v| [B, H, Sq, Skv], Hm = sum_d |o| |d_o| [B, H, Sq], T (score magnitude, base 2), and the sums
    PdO = sum_i P |d_o|, dSq = sum_i |dS| |q|, dSk = sum_j |dS| |k| (head-major [B, H, S, hd])."""
    hd = q.shape[-1] // H
    scale = default_scale(hd) if scale is None else scale
    qh, kh, vh, oh, gh = (heads(x, H, dtype) for x in (q, k, v, o, d_o))
    L = lse2.to(dtype)[..., None]
    s2 = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    P = torch.exp2(s2 - L)
    D = (oh * gh).sum(-1, keepdim=True)
    dP = gh @ vh.transpose(-1, -2)
    dS = P * (dP - D)
    res = dict(dv=unheads(P.transpose(-1, -2) @ gh), dk=unheads(dS.transpose(-1, -2) @ qh * scale), dq=unheads(dS @ kh * scale),
               P=P, dS=dS, G=gh.abs() @ vh.abs().transpose(-1, -2), Hm=(oh.abs() * gh.abs()).sum(-1),
               T=((qh.abs() @ kh.abs().transpose(-1, -2)) * (scale * LOG2E)).amax(-1),
               PdO=P.transpose(-1, -2) @ gh.abs(), dSq=dS.abs().transpose(-1, -2) @ qh.abs(), dSk=dS.abs() @ kh.abs(),
               scale=scale, lse2=lse2.to(dtype), qa=qh.abs(), ka=kh.abs(), ga=gh.abs())
    return res


def backward_bounds(r, c=None, dD=None, dL=None):
    """Bounds on dq, dk, dv ([B, S, H hd]) for the stated arithmetic: bf16 operands, float32 scores / exponentials / dP - D, P and dS rounded
    to bf16 before the second products, float32 accumulation, bf16 outputs.  With e_i = 1 + T_i + |lse2_i| (the magnitude of the exponent
    log2e scale s - lse2, formed in float32) a recomputed probability is off by C e_i relative:
      dv: U |dv| + sum_i (U + C e_i) P_ij |d_o_i|                   bf16(P) and the float32 error of P; the float32 sum adds C sum P |d_o|,
                                                                    which C e_i >= C covers
      dS: |bf16(dS) - dS| <= (U + C e_i) |dS_ij| + P_ij delta_ij,   delta_ij = C (G_ij + Hm_i) the float32 error of dP - D (two float32 dot
                                                                    products of magnitudes G and Hm)
      dq: U |dq| + scale sum_j dSerr_ij |k_j|,  dk: U |dk| + scale sum_i dSerr_ij |q_i|.
    The chained case (o and lse2 from the forward kernel, compared with the gradient at the exact o / lse2) passes the forward's own bounds:
    dD_i >= |D_i(got) - D_i| = sum_d (out bound) |d_o| moves dS by P dD; dL_i >= |lse2(got) - lse2| moves every P of the row, and with it dS
    and dv, by the factor 2^dL - 1."""
    c = C_ATT if c is None else c
    e = 1.0 + r["T"] + r["lse2"].abs()                                   # [B, H, Sq]
    relP = (U_BF16 + c * e)[..., None]                                   # [B, H, Sq, 1]
    P, dSa = r["P"], r["dS"].abs()
    dSerr = relP * dSa + P * c * (r["G"] + r["Hm"][..., None])
    dvx = relP * P
    if dD is not None:
        grow = torch.expm1(LN2 * dL)[..., None]
        dSerr = dSerr + P * dD[..., None] + grow * (dSa + P * dD[..., None])
        dvx = dvx + grow * P
    dv = U_BF16 * r["dv"].abs() + unheads(dvx.transpose(-1, -2) @ r["ga"])
    dq = U_BF16 * r["dq"].abs() + r["scale"] * unheads(dSerr @ r["ka"])
    dk = U_BF16 * r["dk"].abs() + r["scale"] * unheads(dSerr.transpose(-1, -2) @ r["qa"])
    return dict(dq=dq, dk=dk, dv=dv)


def backward_f32_magnitudes(r):
    """What C multiplies in backward_bounds: the bounds at U = 0, C = 1."""
    e = 1.0 + r["T"] + r["lse2"].abs()
    dSerr = e[..., None] * r["dS"].abs() + r["P"] * (r["G"] + r["Hm"][..., None])
    return dict(dv=unheads((e[..., None] * r["P"]).transpose(-1, -2) @ r["ga"]), dq=r["scale"] * unheads(dSerr @ r["ka"]),
                dk=r["scale"] * unheads(dSerr.transpose(-1, -2) @ r["qa"]))


def chained_extras(fref, d_o, H):
    """(dD, dL) of backward_bounds from the forward reference `fref`: the forward's own out bound carried through D = sum_d o d_o, and its
    lse bound."""
    ob, lb = forward_bounds(fref, H)
    return (heads(ob, H) * heads(d_o, H).abs()).sum(-1), lb


# --------------------------------------------------------------------------------------------- float32 emulation of the stated arithmetic
FWD_MUTANTS = ("scale_x1.005", "last_key_dropped", "v_pair_swapped", "causal_off_by_one", "bias_row_mod_128", "lse_missing_one_key")
BWD_MUTANTS = ("D_omitted", "dS_not_scaled", "dk_from_neighbour_query")


def emu_forward(q, k, v, H, scale=None, bias=None, causal=False, tile0=False, mutant=None):
    """The kernels' arithmetic in torch float32: float32 scores, exp2 relative to the row maximum (tile0: to the maximum over the first 64
    keys, never rescaled, as the two pipelined kernels do), float32 row sum of the UNROUNDED exponentials, bf16 probabilities into P V,
    float32 accumulation, bf16 quotient.  Returns (o bf16, lse2 f32, l f32 [B, H, Sq] the row sum relative to the maximum used)."""
    hd = q.shape[-1] // H
    c2 = (default_scale(hd) if scale is None else scale) * LOG2E
    if mutant == "scale_x1.005":
        c2 *= 1.005
    qh, kh, vh = heads(q, H, F32), heads(k, H, F32), heads(v, H, F32)
    Sq, Skv = qh.shape[2], kh.shape[2]
    t = (qh @ kh.transpose(-1, -2)) * c2
    if bias is not None:
        b = bias.to(F32)
        if mutant == "bias_row_mod_128":
            b = b[:, torch.arange(Sq) % 128]
        t = t + b[None] * LOG2E
    hide = torch.zeros(Sq, Skv, dtype=torch.bool)
    if causal:
        hide |= torch.ones(Sq, Skv, dtype=torch.bool).triu(2 if mutant == "causal_off_by_one" else 1)
    if mutant == "last_key_dropped" and Skv > 1:
        hide[:, Skv - 1] = True
    t = t.masked_fill(hide, float("-inf"))
    m = (t[..., :64] if tile0 else t).amax(-1, keepdim=True)
    e = torch.exp2(t - m)
    l = e.sum(-1, keepdim=True)
    if mutant == "v_pair_swapped":
        j = torch.arange(Skv) ^ 1
        j[j >= Skv] = Skv - 1
        vh = vh[:, :, j]
    o = (bf16r(e) @ vh) / l
    ll = l - e[..., -1:] if (mutant == "lse_missing_one_key" and Skv > 1) else l
    return unheads(o).to(BF16), (m + torch.log2(ll)).squeeze(-1), l.squeeze(-1)


def emu_backward(q, k, v, o, d_o, lse2, H, scale=None, mutant=None):
    """Float32 emulation of the backward: P and dS rounded to bf16 before the second products, bf16 outputs."""
    hd = q.shape[-1] // H
    scale = default_scale(hd) if scale is None else scale
    qh, kh, vh, oh, gh = (heads(x, H, F32) for x in (q, k, v, o, d_o))
    P = torch.exp2((qh @ kh.transpose(-1, -2)) * (scale * LOG2E) - lse2.to(F32)[..., None])
    D = (oh * gh).sum(-1, keepdim=True)
    if mutant == "D_omitted":
        D = torch.zeros_like(D)
    dS = bf16r(P * (gh @ vh.transpose(-1, -2) - D))
    sc = 1.0 if mutant == "dS_not_scaled" else scale
    qk = qh.roll(1, 2) if mutant == "dk_from_neighbour_query" else qh
    return dict(dv=unheads(bf16r(P).transpose(-1, -2) @ gh).to(BF16), dk=unheads(dS.transpose(-1, -2) @ qk * sc).to(BF16),
                dq=unheads(dS @ kh * sc).to(BF16))


WINDOW_LO, WINDOW_HI = 1e-30, 1e30            # attention_pipe.hip / attention_d128.hip: bad = !(l > 1e-30f && l < 1e30f)


def window_holds(l, margin=1.0):
    """Per row: the row sum relative to tile 0's maximum is finite and inside the kernels' window, shrunk by `margin` on both sides."""
    return torch.isfinite(l) & (l > WINDOW_LO * margin) & (l < WINDOW_HI / margin)


# -------------------------------------------------------------------------------------------------------------------------- inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _case(path, hd, Sq, Skv, family, B=2, H=3, causal=False, bias=None, scale=None, pitch4=False, probe=False, strength=200.0):
    name = f"{path}-{family}-{Sq}x{Skv}" + (f"-H{H}" if path.startswith("bwd") else "") + ("-causal" if causal else "") + (f"-bias_{bias}" if bias else "") + \
        (f"-scale{scale}" if scale is not None else "") + ("-probe" if probe else "") + (f"-x{strength:g}" if family == "outside_window" else "")
    return dict(name=name, path=path, hd=hd, B=B, H=H, Sq=Sq, Skv=Skv, family=family, causal=causal, bias=bias, scale=scale,
                pitch4=pitch4, probe=probe, strength=strength)


def peak_factor(hd):
    return 6.0 if hd == 128 else 4.0


def selector_target(Sq, Skv, causal, g):
    """Key index that query i selects: a permutation of the keys extended cyclically (every key is chosen when Sq >= Skv); under the causal
    mask a key the query may see, (7 i + 3) mod (min(i, Skv - 1) + 1)."""
    i = torch.arange(Sq)
    if causal:
        return (7 * i + 3) % (torch.minimum(i, torch.tensor(Skv - 1)) + 1)
    return torch.randperm(Skv, generator=g)[i % Skv]


def make_inputs(case):
    """q, k, v as column slices of one packed [B, S, 3 H hd] bf16 buffer (S = max(Sq, Skv)), bias [H, Sq, Skv] f32 or None; CPU tensors.
    Returns a dict of keyword arguments for forward() / emu_forward() plus 'target' for the selector family."""
    g = _gen(case["name"])
    B, H, hd, Sq, Skv, fam = case["B"], case["H"], case["hd"], case["Sq"], case["Skv"], case["family"]
    HD, S = H * hd, max(Sq, Skv)
    scale = default_scale(hd) if case["scale"] is None else case["scale"]
    x = torch.randn(B, S, 3 * HD, generator=g)
    target = None
    if fam == "peaked":
        x[..., :HD] *= peak_factor(hd)
    elif fam == "selector":
        # keys: +-1 sign vectors; query i = a * key target(i) with a hd scale = 32: the chosen key scores 32 nats, every other key
        # a * scale * (a sum of hd signs) ~ N(0, (32 / sqrt(hd))^2), at most ~16 nats => weight >= 0.999 on the chosen key
        kk = torch.where(torch.randn(B, Skv, H, hd, generator=g) >= 0, 1.0, -1.0)
        target = selector_target(Sq, Skv, case["causal"], g)
        a = torch.tensor(32.0 / (hd * scale)).to(BF16).float()
        x[:, :Skv, HD:2 * HD] = kk.reshape(B, Skv, HD)
        x[:, :Sq, :HD] = (a * kk[:, target]).reshape(B, Sq, HD)
        x[:, :Skv, 2 * HD:] = x[:, :Skv, 2 * HD:] * 0.5 + ((torch.arange(Skv) % 13).float() - 6.0)[None, :, None] * 0.5   # per-key distinct values
    elif fam == "outside_window":
        x[:, 64:, HD:2 * HD] *= case["strength"]                          # every key past tile 0: logits hundreds of octaves above it
    else:
        assert fam == "diffuse", fam
    x = x.to(BF16)
    q, k, v = x[:, :Sq, :HD], x[:, :Skv, HD:2 * HD], x[:, :Skv, 2 * HD:]
    if case["probe"]:                                                     # one probe query shared by the batch: q batch stride 0
        assert Sq == 1
        q = x[:1, :1, :HD].expand(B, 1, HD)
    bias = None
    if case["bias"]:
        bias = torch.randn(H, Sq, Skv, generator=g)
        if case["bias"] == "block":                                       # HF-style finite mask on a block: no row loses all its keys
            bias[:, Sq // 4:Sq // 2 + 1, Skv // 3:] = -1e4
            bias[:, Sq // 2 + 1:, 5:Skv // 2] = -1e4
    return dict(q=q, k=k, v=v, H=H, scale=scale, bias=bias, causal=case["causal"]), target, x


def to_device(kw, packed, device):
    """The same views on `device`: the packed buffer is moved once and re-sliced, so q | k | v stay column slices of one allocation."""
    xd = packed.to(device)
    HD = kw["q"].shape[-1]
    Sq, Skv = kw["q"].shape[1], kw["k"].shape[1]
    q = xd[:, :Sq, :HD]
    if kw["q"].stride(0) == 0:
        q = xd[:1, :1, :HD].expand(kw["q"].shape[0], 1, HD)
    return q, xd[:, :Skv, HD:2 * HD], xd[:, :Skv, 2 * HD:], (None if kw["bias"] is None else kw["bias"].to(device))


# ---------------------------------------------------------------------------------------------------------------------- case lists
# Dispatcher branch of attention_fwd each path reaches (read off attention.hip's attention_fwd):
#   hd64_pipe      head_dim == 64 && o16 && !bias && !causal            -> attention_fwd_pipe_launch        (attention_pipe.hip)
#   hd64_causal    head_dim == 64 && o16 && !bias, causal               -> attention_fwd_glds_kernel<false>
#   hd64_bias      head_dim == 64 && o16 && bias                        -> attention_fwd_glds_kernel<true>
#   hd64_tiled     head_dim == 64, output row pitch = 4 (mod 8)         -> attention_fwd_kernel<64>
#   hd72           head_dim == 72                                       -> attention_fwd_kernel<72>
#   hd80_resident  head_dim == 80, !causal, Skv <= 320 && Sq <= 512     -> attention_fwd_resident_launch
#   hd80_tiled     head_dim == 80, Skv > 320 or Sq > 512 or causal      -> attention_fwd_kernel<80>
#   hd128          head_dim == 128                                      -> attention_fwd_d128_launch        (attention_d128.hip)
FAMILIES = ("diffuse", "peaked", "selector")
PIPE_SKV = (1, 63, 64, 65, 128, 129, 193, 257, 321)        # 1, 2, 3, 4, 5, 6 key tiles of the 3-slot ring, ragged and full last tiles
PIPE_SQ = (1, 31, 33, 128, 129, 257)                        # part of a wave, a wave and one row, a full workgroup, one row more, three
CAUSAL_SHAPES = ((1, 1), (64, 64), (65, 65), (129, 129), (257, 257), (300, 300), (200, 300), (300, 200))
BIAS_SHAPES = ((1, 1), (100, 100), (129, 65), (257, 300))
TILED64_SHAPES = ((33, 65), (129, 193))
HD72_SHAPES = ((1, 193), (65, 65), (129, 257))
RES_SKV, RES_SQ = (1, 65, 257, 320), (1, 257, 512)
D128_SQ, D128_SKV = (1, 255, 257, 513), (1, 63, 65, 129, 193, 321)
BWD_PAIRS = tuple((s, s) for s in (1, 31, 33, 64, 65, 127, 129, 257)) + ((1, 257), (257, 1), (33, 129), (129, 33))
BWD_H = {64: (1, 3, 9), 128: (1, 3, 5)}                     # the delta kernels walk 8 (hd 64) / 4 (hd 128) heads per pass


def _fwd_cases():
    c = {}
    c["hd64_pipe"] = [_case("hd64_pipe", 64, sq, skv, f) for f in FAMILIES for sq in PIPE_SQ for skv in PIPE_SKV]
    c["hd64_pipe"] += [_case("hd64_pipe", 64, sq, skv, "outside_window", strength=st)
                       for (sq, skv, st) in ((129, 129, 200.0), (33, 321, 200.0), (257, 193, 60.0))]
    c["hd64_causal"] = [_case("hd64_causal", 64, sq, skv, f, causal=True) for f in FAMILIES for sq, skv in CAUSAL_SHAPES]
    bias = []
    for sc in (0.2, 1.0):
        for f in (FAMILIES if sc == 0.2 else ("diffuse", "selector")):
            bias += [_case("hd64_bias", 64, sq, skv, f, bias="randn", scale=sc) for sq, skv in BIAS_SHAPES]
    bias += [_case("hd64_bias", 64, 257, 300, f, bias="block", scale=0.2) for f in ("diffuse", "peaked")]
    bias += [_case("hd64_bias", 64, 257, 300, f, bias="randn", scale=0.2, causal=True) for f in ("diffuse", "peaked")]
    c["hd64_bias"] = bias
    c["hd64_tiled"] = [_case("hd64_tiled", 64, sq, skv, f, causal=ca, pitch4=True)
                       for f in FAMILIES for sq, skv in TILED64_SHAPES for ca in (False, True)]
    c["hd72"] = [_case("hd72", 72, sq, skv, f) for f in FAMILIES for sq, skv in HD72_SHAPES]
    c["hd72"] += [_case("hd72", 72, 1, 193, f, probe=True) for f in ("diffuse", "peaked")]
    c["hd80_resident"] = [_case("hd80_resident", 80, sq, skv, f) for f in FAMILIES for sq in RES_SQ for skv in RES_SKV]
    c["hd80_tiled"] = [_case("hd80_tiled", 80, sq, skv, f, causal=ca)
                       for f in FAMILIES for sq, skv, ca in ((257, 321, False), (513, 257, False), (129, 129, True))]
    c["hd128"] = [_case("hd128", 128, sq, skv, f, H=5) for f in FAMILIES for sq in D128_SQ for skv in D128_SKV]
    c["hd128"] += [_case("hd128", 128, sq, skv, "outside_window", H=5, strength=st) for (sq, skv, st) in ((257, 129, 200.0), (255, 321, 60.0))]
    return c


FWD_CASES = _fwd_cases()
FWD_PATHS = tuple(FWD_CASES)
TILE0_PATHS = ("hd64_pipe", "hd128")                       # the two pipelined kernels: every probability relative to tile 0's maximum
LSE_ONCE = {p: FWD_CASES[p][0]["name"] for p in FWD_PATHS}


def _bwd_cases():
    c = {}
    for hd in (64, 128):
        lst = []
        for n, (sq, skv) in enumerate(BWD_PAIRS):
            for f in FAMILIES:
                Hh = BWD_H[hd][(n + FAMILIES.index(f)) % 3]
                lst.append(_case(f"bwd{hd}", hd, sq, skv, f, H=Hh))
        for Hh in BWD_H[hd]:                                              # every head count at one ragged shape, for sure
            lst.append(_case(f"bwd{hd}", hd, 65, 129, "diffuse", H=Hh, scale=0.2 if hd == 64 else None))
        if hd == 64:
            lst += [_case("bwd64", 64, sq, skv, f, H=3, scale=0.2) for f in ("peaked", "selector") for sq, skv in ((129, 129), (33, 129))]
        c[f"bwd{hd}"] = lst
    return c


BWD_CASES = _bwd_cases()
CHAINED = {64: _case("chained64", 64, 129, 193, "peaked"), 128: _case("chained128", 128, 257, 129, "peaked", H=5)}


def make_backward_inputs(case, fref=None):
    """The forward inputs of `case`, d_o ~ N(0, 1) bf16 and the o (bf16) / lse2 (f32) the backward entry receives, taken from the float64
    forward reference (not from a kernel)."""
    kw, target, packed = make_inputs(case)
    fref = forward(**kw) if fref is None else fref
    g = _gen(case["name"] + "/d_o")
    d_o = torch.randn(kw["q"].shape, generator=g).to(BF16)
    return kw, packed, d_o, fref["o"].to(BF16), fref["lse2"].to(F32), fref
