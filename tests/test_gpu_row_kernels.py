"""GPU: the row kernels of csrc/norm.hip and csrc/train.hip against the float64 references of tests/row_kernel_reference.py, element by
element -- one wrong element fails -- with sentinel-filled padding around everything a kernel writes.

Bounds (derived in row_kernel_reference.py, never fitted to a kernel's output): data movement and single exactly-rounded products / sums
are bit-exact; everything else is |got - r| <= k * 2^-8 * |r| + a with k the bf16 roundings on the path and a = C_F32 * (sum of the
magnitudes of the added terms), C_F32 measured in tests/test_row_kernel_reference_host.py.  Each comparison prints its worst error / bound."""
import pytest
import torch

import row_kernel_reference as R

pytestmark = pytest.mark.gpu

U, C = R.U_BF16, R.C_F32
SENT16 = 0x5A5B           # sentinel bit patterns (a bf16 of ~2.4e16 / an f32 of ~1.5e16: nothing a kernel here computes)
SENT32 = 0x5A5B5C5D


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _is_sent(t):
    if t.dtype == torch.bfloat16:
        return bool((t.contiguous().view(torch.int16) == SENT16).all())
    return bool((t.contiguous().view(torch.int32) == SENT32).all())


def _bits(t):
    return t.contiguous().view(torch.int16)


def _within(got, ref, bound, what):
    """Elementwise |got - ref| <= bound; ref may be a tuple of admissible references (the nearer one counts).  NaN fails."""
    got = got.detach().cpu().double()
    refs = ref if isinstance(ref, tuple) else (ref,)
    err = torch.stack([(got - r).abs() for r in refs]).amin(0)
    ratio = err / bound.clamp_min(1e-300)
    print(f"{what}: worst |got - ref| / bound = {ratio.max().item():.3f} over {got.numel()} elements")
    bad = ~(err <= bound)
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements out of bound; first at flat index {i}: got "
                             f"{got.flatten()[i].item()!r}, ref {refs[0].flatten()[i].item()!r}, bound {bound.flatten()[i].item():.3e}")


def _guard(M, D, pad):
    """A sentinel-filled [M + 1, D + pad] bf16 buffer and its [M, D] view: what a kernel may write."""
    buf = _sent_bf16(M + 1, D + pad)
    return buf, buf[:M, :D]


def _guard_ok(buf, M, D):
    return _is_sent(buf[:, D:]) and _is_sent(buf[M:])


# ------------------------------------------------------------------------------------------------------------------------ layernorm_mod
@pytest.mark.parametrize("D", R.LN_DS)
def test_layernorm_mod_vs_float64(D):
    """k = 1 (the output rounding); a = C_F32 ((|x| + mean|x|) rstd [|w|] [+ |b|]) |1 + scale| + |shift|).  Every M, every modulation /
    affine variant, x as a column slice, a row mean of 100 (two-pass variance); output pitch D + 8 or D + 64 and one spare row."""
    from adv_grpo_amd import ops
    for M in R.LN_MS:
        for vi, variant in enumerate(R.LN_VARIANTS):
            kw = R.ln_case(D, M, variant, device="cuda")
            buf, out = _guard(M, D, 8 if vi % 2 else 64)
            res = ops.layernorm_mod(out=out, **kw)
            outs = list(res) if isinstance(res, tuple) else [res]
            refs, mags = R.layernorm_mod(**{k: (R.cpu(v) if torch.is_tensor(v) else v) for k, v in kw.items()})
            assert len(outs) == len(refs) and outs[0].data_ptr() == out.data_ptr()
            for j, (o, r, mg) in enumerate(zip(outs, refs, mags)):
                _within(o, r, U * r.abs() + C * mg, f"layernorm_mod D={D} M={M} {variant} out{j}")
            assert _guard_ok(buf, M, D), (D, M, variant)


@pytest.mark.parametrize("M,D", R.RMS_ROWS_SHAPES)
def test_rmsnorm_rows_vs_float64(M, D):
    """T5 form bf16(x rs) * w: k = 2 (the cast of the normalised value, the output), a = C_F32 |r|."""
    from adv_grpo_amd import ops
    kw = R.rms_rows_case(M, D, device="cuda")
    buf, out = _guard(M, D, 8)
    ops.rmsnorm_rows(kw["x"], kw["w"], out=out)
    ref = R.rmsnorm_rows(R.cpu(kw["x"]), R.cpu(kw["w"]))
    _within(out, ref, (2 * U + C) * ref[0].abs(), f"rmsnorm_rows M={M} D={D}")
    assert _guard_ok(buf, M, D)


# ------------------------------------------------------------------------------------------------------------------------ rmsnorm_heads
@pytest.mark.parametrize("nheads", R.HEADS_NHEADS)
def test_rmsnorm_heads_vs_float64(nheads):
    """bf16(x rs) * w[head // heads_per_weight] in place: k = 2, a = C_F32 |r|; rs_out relative 2^-20.  Columns outside
    [col0, col0 + nheads * 64), rows the seg map does not reach and their rs_out rows keep their bits."""
    from adv_grpo_amd import ops
    for col0 in R.HEADS_COL0:
        for seg in (False, True):
            for with_rs in (True, False):
                buf, w, hpw, sg, M = R.heads_case(nheads, col0, seg, device="cuda")
                before = buf.clone()
                rs = torch.full((buf.shape[0], nheads), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
                ops.rmsnorm_heads(buf, col0, nheads, w, hpw, seg=sg, M=M, rs_out=rs if with_rs else None)
                rows, ref, rs_ref = R.rmsnorm_heads(R.cpu(before), col0, nheads, R.cpu(w), hpw, seg=sg, M=M)
                what = f"rmsnorm_heads nheads={nheads} col0={col0} seg={sg} rs_out={with_rs}"
                _within(buf[rows.cuda(), col0:col0 + nheads * 64], ref, (2 * U + C) * ref[0].abs(), what)
                untouched = torch.ones(buf.shape, dtype=torch.bool)
                untouched[rows, col0:col0 + nheads * 64] = False
                assert torch.equal(_bits(buf).cpu()[untouched], _bits(before).cpu()[untouched]), what
                other = torch.ones(buf.shape[0], dtype=torch.bool)
                other[rows] = False
                assert other.any() and _is_sent(rs[other.cuda()]), what
                if with_rs:
                    _within(rs[rows.cuda()], rs_ref, 2.0 ** -20 * rs_ref, what + " rs")
                else:
                    assert _is_sent(rs), what


@pytest.mark.parametrize("nheads", R.HEADS_BWD_NHEADS)
def test_rmsnorm_heads_bwd_vs_float64_autograd(nheads):
    """dx = rs (g - xhat mean(g xhat)), g = dy w, against float64 autograd of x rs w (the forward's rounding straight-through).  The kernel's
    inputs are the reference forward's y (bf16) and rs (f32), not the forward kernel's.  k = 1; a = C_F32 rs (|g| + |xhat| mean|g xhat|); and the
    input term: the kernel has xhat only as y / w, two bf16 roundings off x rs, relative error d <= (1 + 2^-8)^2 - 1, which moves dx by at most
    (d + d^2) rs |xhat| (|mean(g xhat)| + mean|g xhat|).  dy and y have different pitches; everything outside the mapped heads keeps its bits."""
    from adv_grpo_amd import ops
    for col0 in R.HEADS_COL0:
        for seg in (False, True):
            buf, w, hpw, sg, M = R.heads_case(nheads, col0, seg, device="cpu")
            rows, (y_ref, _, _), rs_ref = R.rmsnorm_heads(buf, col0, nheads, w, hpw, seg=sg, M=M)
            y = buf.clone()
            y[rows, col0:col0 + nheads * 64] = y_ref.to(torch.bfloat16)
            rs = torch.zeros(buf.shape[0], nheads, dtype=torch.float32)
            rs[rows] = rs_ref.float()
            g = torch.Generator().manual_seed(nheads + col0)
            dy = torch.randn(buf.shape[0], buf.shape[1] + 64, generator=g).to(torch.bfloat16)       # a pitch of its own
            d_in = dy.cuda()
            ops.rmsnorm_heads_bwd(d_in, y.cuda(), rs.cuda(), col0, nheads, w.cuda(), hpw, seg=sg, M=M)
            x3 = buf[rows, col0:col0 + nheads * 64].reshape(M, nheads, 64)
            dy3 = dy[rows, col0:col0 + nheads * 64].reshape(M, nheads, 64)
            ref = R.rmsnorm_heads_bwd(x3, dy3, w, hpw)
            _, mag, mag_in = R.rmsnorm_heads_bwd_formula(x3, dy3, w, hpw)
            d = R.XHAT_IN_ERR
            what = f"rmsnorm_heads_bwd nheads={nheads} col0={col0} seg={sg}"
            _within(d_in[rows.cuda(), col0:col0 + nheads * 64].reshape(M, nheads, 64), ref, U * ref.abs() + C * mag + (d + d * d) * mag_in, what)
            untouched = torch.ones(dy.shape, dtype=torch.bool)
            untouched[rows, col0:col0 + nheads * 64] = False
            assert torch.equal(_bits(d_in).cpu()[untouched], _bits(dy)[untouched]), what


# -------------------------------------------------------------------------------------------------------------------- layernorm_mod_bwd
@pytest.mark.parametrize("D", R.LNB_DS)
def test_layernorm_mod_bwd_vs_float64_autograd(D):
    """k = 1; a = C_F32 (rstd (|g| + mean|g| + |xhat| mean|g xhat|) + |dres|).  The gated copies are single exact products of the stored
    bf16 dx and a bf16 gate: bit-equal to (dx.float() * gate.float()).bfloat16().  dx has pitch D + 8 / D + 64 and a spare row."""
    from adv_grpo_amd import ops
    for M in R.LNB_MS:
        for vi, variant in enumerate(R.LNB_VARIANTS):
            kw = R.lnb_case(D, M, variant, device="cuda")
            dres = kw.get("dres")                                       # (dres shares dx's pitch in the C entry)
            buf = _sent_bf16(M + 1, dres.stride(0) if dres is not None else D + (8 if vi % 2 else 64))
            out = buf[:M, :D]
            res = ops.layernorm_mod_bwd(out=out, **kw)
            dx, gouts = res if isinstance(res, tuple) else (res, [])
            ckw = {k: (R.cpu(v) if torch.is_tensor(v) else v) for k, v in kw.items() if k != "gates"}
            ref = R.layernorm_mod_bwd(**ckw)
            _, mag = R.layernorm_mod_bwd_formula(**ckw)
            what = f"layernorm_mod_bwd D={D} M={M} {variant}"
            _within(dx, ref, U * ref.abs() + C * mag, what)
            assert dx.data_ptr() == out.data_ptr() and _guard_ok(buf, M, D), what
            assert len(gouts) == len(kw.get("gates", []))
            for gate, go in zip(kw.get("gates", []), gouts):
                want = R.gate_mul(R.cpu(dx), R.cpu(gate), kw["rows_per_batch"]).to(torch.bfloat16)
                assert torch.equal(_bits(go).cpu(), _bits(want)), what + " gated copy"
                assert torch.equal(_bits(go), _bits(ops.gate_mul(dx.contiguous(), gate, kw["rows_per_batch"]))), what


# --------------------------------------------------------------------------------------------------- timestep_embedding, unary, gate_mul
def test_timestep_embedding_vs_float64():
    """k = 1 and the absolute term |t| 2^-20: the kernel forms the angle t f in float32, f = expf(-ln(1e4) i / half) with an exponent of
    magnitude <= 9.3 rounded three times (relative error of f <= ~2^-22 |exponent|, and |exponent| e^-|exponent| <= 1 / e), the product
    rounded once -- an angle error below |t| 2^-21 -- and cosf / sinf are 1-Lipschitz and good to a few 2^-24.  t = 0 must give exactly 1 | 0."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    t = torch.tensor(R.TS_T, dtype=torch.float32)
    B = t.numel()
    for dim in R.TS_DIMS:
        buf = _sent_bf16(B * dim + 64)
        _lib.check(lib.advgrpo_timestep_embedding(t.cuda().data_ptr(), buf.data_ptr(), B, dim, _lib.stream_ptr()))
        ref = R.timestep_embedding(t, dim)
        got = buf[:B * dim].view(B, dim)
        _within(got, ref, U * ref.abs() + t.double().abs()[:, None] * 2.0 ** -20, f"timestep_embedding dim={dim}")
        assert _is_sent(buf[B * dim:])
        assert torch.equal(got[0].cpu().float(), torch.cat([torch.ones(dim // 2), torch.zeros(dim // 2)]))
    from adv_grpo_amd import ops
    assert torch.equal(ops.timestep_embedding(t.cuda(), 256), _run_ts(lib, _lib, t, 256))


def _run_ts(lib, _lib, t, dim):
    out = torch.empty(t.numel(), dim, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.advgrpo_timestep_embedding(t.cuda().data_ptr(), out.data_ptr(), t.numel(), dim, _lib.stream_ptr()))
    return out


@pytest.mark.parametrize("n", R.UNARY_NS)
def test_unary_vs_float64(n):
    """none: a copy, bit for bit; none with x2: one exactly-rounded sum, bit-equal to (x.float() + x2.float()).bfloat16(); silu:
    k = 1, a = C_F32 (1 + |v|) |r| -- silu's relative condition number is below 1 + |v| (d ln(v sigmoid(v)) / d ln v = 1 + v (1 - sigmoid(v)))
    and __expf's argument reduction errs in proportion to |v| as well.  The edge values +-{0, 1e-3, 20, 88} sit at both ends."""
    from adv_grpo_amd import _lib, ops
    lib = _lib.load()
    x, x2 = R.unary_case(n, device="cuda")

    def run(act, second):
        buf = _sent_bf16(n + 64)
        _lib.check(lib.advgrpo_unary(x.data_ptr(), second.data_ptr() if second is not None else None, buf.data_ptr(), n, ops.ACT[act],
                                     _lib.stream_ptr()))
        assert _is_sent(buf[n:]), (act, second is not None)
        return buf[:n]

    assert torch.equal(_bits(run(None, None)), _bits(x))
    assert torch.equal(_bits(run(None, x2)), _bits((x.float() + x2.float()).bfloat16()))
    for second in (None, x2):
        ref, v = R.unary(R.cpu(x), "silu", R.cpu(second))
        got = run("silu", second)
        _within(got, ref, (U + C * (1 + v.abs())) * ref.abs(), f"silu n={n} x2={second is not None}")
        assert torch.equal(_bits(ops.unary(x, "silu", second)), _bits(got))


def test_unary_refuses_the_activations_it_does_not_implement():
    from adv_grpo_amd import _lib, ops
    x = torch.ones(64, dtype=torch.bfloat16, device="cuda")
    for act in ("gelu", "gelu_tanh", "quick_gelu", "gelu_erf", "gelu_new"):
        with pytest.raises(_lib.AdvGrpoError, match="0 none, 3 silu"):
            ops.unary(x, act)
    assert torch.equal(ops.unary(x, "none"), x)


@pytest.mark.parametrize("D,M,rpb", R.GATE_SHAPES)
def test_gate_mul_is_the_exactly_rounded_product(D, M, rpb):
    from adv_grpo_amd import ops
    g = torch.Generator().manual_seed(D + M)
    x = torch.randn(M, D, generator=g).bfloat16().cuda()
    table = torch.randn((M + rpb - 1) // rpb, 6 * D, generator=g).bfloat16().cuda()
    gate = table[:, 2 * D:3 * D]                                          # a strided view: pitch 6 D
    buf = _sent_bf16(M * D + 64)
    out = ops.gate_mul(x, gate, rpb, out=buf[:M * D].view(M, D))
    idx = torch.arange(M, device="cuda") // rpb
    assert torch.equal(_bits(out), _bits((x.float() * gate.float()[idx]).bfloat16()))
    assert torch.equal(_bits(out).cpu(), _bits(R.gate_mul(R.cpu(x), R.cpu(gate), rpb).to(torch.bfloat16)))
    assert _is_sent(buf[M * D:])


# ------------------------------------------------------------------------------------------------------- patchify, unpatchify, transpose
@pytest.mark.parametrize("shape", R.PATCH_SHAPES)
def test_patchify_and_unpatchify_are_exact_permutations(shape):
    """Bit-exact: patchify's columns are (c, py, px), unpatchify's (py, px, c) -- the two orders differ, and the round trip goes through the
    column permutation between them."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    B, C, H, W = shape
    T = B * (H // 2) * (W // 2)
    g = torch.Generator().manual_seed(H * W + C)
    x32 = torch.randn(B, C, H, W, generator=g)
    for x in (x32, x32.bfloat16()):
        buf = _sent_bf16(T * C * 4 + 64)
        xd = x.cuda()
        _lib.check(lib.advgrpo_patchify(xd.data_ptr(), _lib.dtype_code(x.dtype), buf.data_ptr(), B, C, H, W, _lib.stream_ptr()))
        got = buf[:T * C * 4].view(T, C * 4)
        assert torch.equal(_bits(got).cpu(), _bits(R.patchify(x).to(torch.bfloat16))), (shape, x.dtype)
        assert _is_sent(buf[T * C * 4:])
    tok = torch.randn(T, 4 * C, generator=g).bfloat16()
    want = R.unpatchify(tok, B, C, H, W)
    for dt, sent in ((torch.bfloat16, SENT16), (torch.float32, SENT32)):
        n = B * C * H * W
        buf = torch.full((n + 64,), sent, dtype=torch.int16 if dt == torch.bfloat16 else torch.int32, device="cuda").view(dt)
        _lib.check(lib.advgrpo_unpatchify(tok.cuda().data_ptr(), buf.data_ptr(), _lib.dtype_code(dt), B, C, H, W, _lib.stream_ptr()))
        got = buf[:n].view(B, C, H, W).cpu()
        assert got.dtype == dt and torch.equal(got, want.to(dt)), (shape, dt)            # (bf16 -> f32 is exact)
        assert _is_sent(buf[n:])
    from adv_grpo_amd import ops
    p = ops.patchify(x32.bfloat16().cuda())
    reordered = p.view(T, C, 4).transpose(1, 2).reshape(T, 4 * C).contiguous()
    assert torch.equal(ops.unpatchify(reordered, B, C, H, W).cpu(), x32.bfloat16())
    assert torch.equal(ops.unpatchify(reordered, B, C, H, W, out_dtype=torch.float32).cpu(), x32.bfloat16().float())


@pytest.mark.parametrize("Rr", R.TR_RS)
def test_transpose_is_exact_with_gather_and_zero_padding(Rr):
    from adv_grpo_amd import ops
    for Cc in R.TR_CS:
        for seg in (None, R.TR_SEG[Rr]):
            g = torch.Generator().manual_seed(Rr * 131 + Cc)
            rows = (Rr // seg[0]) * seg[1] if seg else Rr
            src = torch.randn(rows, Cc + 8, generator=g).bfloat16().cuda()[:, :Cc]          # input pitch C + 8
            Rpad = (Rr + 63) // 64 * 64
            buf = _sent_bf16(Cc + 1, Rpad + 8)
            out = ops.transpose(src, R=Rr, seg=seg, pad_to=64, out=buf[:Cc, :Rpad])
            assert torch.equal(_bits(out).cpu(), _bits(R.transpose(R.cpu(src), R=Rr, seg=seg, pad_to=64))), (Rr, Cc, seg)
            assert _guard_ok(buf, Cc, Rpad), (Rr, Cc, seg)


# --------------------------------------------------------------------------------------------------------------------- argument checks
def test_backward_and_gate_entries_refuse_bad_arguments_without_launching():
    """advgrpo_layernorm_mod_bwd, advgrpo_layernorm_mod_bwd_gated and advgrpo_gate_mul: D <= 0 and row, modulation and gate pitches that are
    not multiples of 8 (the kernels load 16 bytes per lane) come back as an error code with a message, before any launch.  Every call below
    is rejected by the entry's own checks; the buffers are valid and large enough for the good call that closes the test."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    M, D = 4, 64
    t = [torch.zeros(M, D, dtype=torch.bfloat16, device="cuda") for _ in range(8)]
    x, dy0, dy1, sc0, sc1, dres, dx, gate = (a.data_ptr() for a in t)
    gout = torch.zeros(M, D, dtype=torch.bfloat16, device="cuda")
    s = _lib.stream_ptr()

    def bwd(ldx=D, lddy=D, ms=D, lddx=D, D_=D):
        return lib.advgrpo_layernorm_mod_bwd(x, ldx, dy0, dy1, lddy, sc0, sc1, ms, 2, dres, dx, lddx, M, D_, 1e-6, s)

    def gated(ldx=D, lddy=D, ms=D, lddx=D, D_=D, gs=D):
        return lib.advgrpo_layernorm_mod_bwd_gated(x, ldx, dy0, dy1, lddy, sc0, sc1, ms, 2, dres, dx, lddx, M, D_, 1e-6, gate, gout.data_ptr(),
                                                   None, None, gs, s)

    def gmul(D_=D, gs=D):
        return lib.advgrpo_gate_mul(x, gate, gout.data_ptr(), M, D_, 2, gs, s)

    for fn, name in ((bwd, b"layernorm_mod_bwd:"), (gated, b"layernorm_mod_bwd_gated:")):
        for bad in (dict(D_=0), dict(D_=-8)):
            assert fn(**bad) != 0
            err = lib.advgrpo_last_error()
            assert name in err and b"D > 0" in err, err
        for bad in (dict(ldx=D + 4), dict(lddy=D + 4), dict(ms=D + 4), dict(lddx=D + 4)):
            assert fn(**bad) != 0
            err = lib.advgrpo_last_error()
            assert name in err and b"multiples of 8" in err, (bad, err)
    assert gated(gs=D + 4) != 0 and b"multiples of 8" in lib.advgrpo_last_error()
    for bad in (dict(D_=0), dict(D_=-8)):
        assert gmul(**bad) != 0 and b"D > 0" in lib.advgrpo_last_error()
    assert gmul(gs=D + 4) != 0 and b"gate pitch" in lib.advgrpo_last_error()
    assert bwd() == 0 and gated() == 0 and gmul() == 0
    torch.cuda.synchronize()
    assert not gout.any() and not t[6].any()


# ------------------------------------------------------------------------------------------------- flat LayerNorm entries against the pair entry
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("D", [64, 2056])
def test_layernorm_mod_flat_entries_equal_the_pair_entry(D, fp8):
    """ops.layernorm_mod / ops.layernorm_mod_fp8 against ops.layernorm_mod_pair on the same two problems, bit for bit: 5 rows with two
    outputs and 9 rows with one (a full and a partial four-row block each), both kernel widths, outputs as views of pitch D + 8 / D + 64 in
    sentinel-filled buffers whose padding must stay untouched."""
    from adv_grpo_amd import ops
    g = torch.Generator().manual_seed(D + fp8)
    probs = []
    for M, rpb, dual, pad in ((5, 3, True, 8), (9, 4, False, 64)):
        x = (torch.randn(M, D + 8, generator=g) * 2 + 1).bfloat16().cuda()[:, :D]
        mods = (torch.randn((M + rpb - 1) // rpb, 4 * D, generator=g) * 0.3).bfloat16().cuda()
        kw = dict(x=x, scale=mods[:, :D], shift=mods[:, D:2 * D], rows_per_batch=rpb)
        if dual:
            kw.update(scale2=mods[:, 2 * D:3 * D], shift2=mods[:, 3 * D:])
        probs.append((M, pad, dual, kw))

    def run(pair):
        bufs, kws = [], []
        for M, pad, dual, kw in probs:
            kw = dict(kw)
            b0, kw["out"] = _guard(M, D, pad)
            b1 = None
            if dual and (pair or fp8):              # (ops.layernorm_mod allocates its second output itself)
                b1, kw["out2"] = _guard(M, D, pad)
            if fp8:
                for name in ("q", "q2")[:2 if dual else 1]:
                    codes = torch.full((M + 1, D + 16), 0x5A, dtype=torch.uint8, device="cuda")
                    scales = torch.full((M + 1,), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
                    kw[name] = ops.Fp8Rows(codes[:M, :D], scales[:M])
                    bufs.append((codes, scales))
            bufs.append((b0, b1, M))
            kws.append(kw)
        if pair:
            rets = ops.layernorm_mod_pair(*kws)
        else:
            rets = []
            for kw in kws:
                kw = dict(kw)
                x = kw.pop("x")
                rets.append(ops.layernorm_mod_fp8(x, kw.pop("q"), **kw) if fp8 else ops.layernorm_mod(x, **kw))
        for b in bufs:
            if len(b) == 3:
                assert _guard_ok(b[0], b[2], D) and (b[1] is None or _guard_ok(b[1], b[2], D)), (pair, b[2])
            else:
                codes, scales = b
                M = codes.shape[0] - 1
                assert bool((codes[:, D:] == 0x5A).all()) and bool((codes[M:] == 0x5A).all()) and _is_sent(scales[M:]), (pair, M)
        return rets, kws

    (fa, fb), fkw = run(False)
    (pa, pb), pkw = run(True)
    assert isinstance(fa, tuple) and isinstance(pa, tuple) and len(fa) == len(pa) == 2
    assert torch.equal(fa[0], pa[0]) and torch.equal(fa[1], pa[1])
    if fp8:
        assert fb[1] is None and pb[1] is None and torch.equal(fb[0], pb[0])
        for f, p in zip(fkw, pkw):
            for name in ("q", "q2"):
                if name in f:
                    assert torch.equal(f[name].q, p[name].q) and torch.equal(f[name].scale, p[name].scale), name
                    assert f[name].q.any() and not _is_sent(f[name].scale)
    else:
        assert torch.is_tensor(fb) and torch.equal(fb, pb)
    assert not _is_sent(fa[0]) and not _is_sent(fa[1])
