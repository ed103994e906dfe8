"""CPU: the float64 references of tests/row_kernel_reference.py against independent torch formulations, every input of the GPU parity
file (tests/test_gpu_row_kernels.py) constructed once so that a typo in a shape or a stride fails here, and the float32 constant C_F32."""
import math

import pytest
import torch
import torch.nn.functional as F

import row_kernel_reference as R

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


def test_layernorm_mod_reference_matches_functional_layer_norm():
    for D, M, variant in [(8, 1, "none"), (520, 5, "table"), (2432, 4, "two"), (512, 3, "affine"), (504, 5, "w_only"), (1536, 5, "table_rpb0"),
                          (2056, 333, "offset_mean"), (520, 4, "xslice")]:
        kw = R.ln_case(D, M, variant)
        outs, mags = R.layernorm_mod(**kw)
        x = kw["x"].to(F64)
        w, b = kw.get("w"), kw.get("b")
        ln = F.layer_norm(x, (D,), None if w is None else w.to(F64), None if b is None else b.to(F64), kw["eps"])
        rpb = kw["rows_per_batch"]
        want = []
        for sc, sh in (("scale", "shift"), ("scale2", "shift2")):
            if kw.get(sc) is not None:
                rows = [kw[sc].to(F64)[(m // rpb) if rpb else 0] for m in range(M)]
                shr = [kw[sh].to(F64)[(m // rpb) if rpb else 0] for m in range(M)]
                want.append(ln * (1 + torch.stack(rows)) + torch.stack(shr))
        if not want:
            want = [ln]
        assert len(outs) == len(want) == len(mags)
        for o, wv, mg in zip(outs, want, mags):
            _close(o, wv, 1e-11 if variant == "offset_mean" else 1e-12)
            assert (mg >= o.abs() * (1 - 1e-12)).all()              # the magnitudes dominate the value they bound


def test_rmsnorm_references_match_vector_norm_form():
    kw = R.rms_rows_case(77, 512)
    x, w = kw["x"].to(F64), kw["w"].to(F64)
    n = x / torch.sqrt(torch.linalg.vector_norm(x, dim=-1, keepdim=True) ** 2 / 512 + 1e-6)
    nom, lo, hi = R.rmsnorm_rows(kw["x"], kw["w"])
    _close(nom, n.to(torch.bfloat16).to(F64) * w)
    assert (lo != hi).float().mean().item() < 1e-3                   # the tie candidates differ almost nowhere
    _close(R.rmsnorm_rows(kw["x"], kw["w"], round_mid=False)[0], n * w)
    for nheads, col0, seg in [(7, 64, True), (76, 0, False), (8, 64, False)]:
        buf, wq, hpw, sg, M = R.heads_case(nheads, col0, seg)
        rows, (nom, lo, hi), rs = R.rmsnorm_heads(buf, col0, nheads, wq, hpw, seg=sg, M=M)
        assert rows.tolist() == [((m // sg[0]) * sg[1] + sg[2] + m % sg[0]) if sg else m for m in range(M)]
        for i, r in enumerate(rows.tolist()):
            for h in (0, nheads // 2, nheads - 1):
                xh = buf[r, col0 + h * 64:col0 + (h + 1) * 64].to(F64)
                rr = 1.0 / math.sqrt(float((xh * xh).sum()) / 64 + 1e-6)
                assert abs(rs[i, h].item() - rr) <= 1e-12 * rr
                _close(nom[i, h * 64:(h + 1) * 64], (xh * rr).to(torch.bfloat16).to(F64) * wq[h // hpw].to(F64))


def test_timestep_embedding_reference_matches_the_diffusers_statement():
    t = torch.tensor(R.TS_T, dtype=torch.float32)
    for dim in R.TS_DIMS:
        half = dim // 2
        exponent = -math.log(10000) * torch.arange(0, half, dtype=F64) / (half - 0.0)      # downscale_freq_shift = 0
        emb = t.to(F64)[:, None] * torch.exp(exponent)[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)                            # flip_sin_to_cos
        _close(R.timestep_embedding(t, dim), emb)


def test_patch_references_match_reshape_permute():
    for B, C, H, W in R.PATCH_SHAPES:
        x = torch.arange(B * C * H * W, dtype=F64).reshape(B, C, H, W)
        h, w = H // 2, W // 2
        p = R.patchify(x)
        assert torch.equal(p, x.reshape(B, C, h, 2, w, 2).permute(0, 2, 4, 1, 3, 5).reshape(B * h * w, C * 4))
        tok = torch.arange(B * h * w * 4 * C, dtype=F64).reshape(B * h * w, 4 * C)
        u = R.unpatchify(tok, B, C, H, W)
        assert torch.equal(u, tok.reshape(B, h, w, 2, 2, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W))
        # the two column orders differ: (c, py, px) against (py, px, c); unpatchify inverts patchify after that column permutation
        reordered = p.reshape(-1, C, 4).transpose(1, 2).reshape(-1, 4 * C)
        assert torch.equal(R.unpatchify(reordered, B, C, H, W), x)
        if C > 1:
            assert not torch.equal(R.unpatchify(p, B, C, H, W), x)


def test_gate_mul_unary_and_transpose_references():
    for D, M, rpb in R.GATE_SHAPES:
        g = torch.Generator().manual_seed(D)
        x, gate = torch.randn(M, D, generator=g).bfloat16(), torch.randn((M + rpb - 1) // rpb, D, generator=g).bfloat16()
        want = torch.stack([x[m].double() * gate[m // rpb].double() for m in range(M)])
        assert torch.equal(R.gate_mul(x, gate, rpb), want)
        assert torch.equal(want.to(torch.bfloat16), (x.float() * gate.float()[torch.arange(M) // rpb]).bfloat16())   # exact in f32 too
    x, x2 = R.unary_case(2040)
    _close(R.unary(x, "silu", x2)[0], F.silu(x.double() + x2.double()))
    assert torch.equal(R.unary(x, None, x2)[0], x.double() + x2.double())
    for Rr in R.TR_RS:
        sr, ss, so = R.TR_SEG[Rr]
        assert Rr % sr == 0 and so + sr <= ss
        src = torch.randn((Rr // sr) * ss, 48).bfloat16()
        tr = R.transpose(src, R=Rr, seg=(sr, ss, so))
        assert tr.shape == (48, (Rr + 63) // 64 * 64)
        assert torch.equal(tr[:, :Rr], src.view(Rr // sr, ss, 48)[:, so:so + sr].reshape(Rr, 48).t()) and (tr[:, Rr:] == 0).all()


def _fd(f, x, h=1e-6):
    """Central finite differences of the scalar f at x (float64), one element at a time."""
    g = torch.zeros_like(x)
    for i in range(x.numel()):
        e = torch.zeros_like(x)
        e.view(-1)[i] = h
        g.view(-1)[i] = (f(x + e) - f(x - e)) / (2 * h)
    return g


def test_backward_references_match_finite_differences_and_the_closed_forms():
    g = torch.Generator().manual_seed(3)
    M, D, rpb = 3, 16, 2
    x, dy0, dy1, dres = (torch.randn(M, D, generator=g, dtype=F64) for _ in range(4))
    sc0, sc1, sh = (0.5 * torch.randn(2, D, generator=g, dtype=F64) for _ in range(3))
    for kw in (dict(scale0=sc0), dict(), dict(scale0=sc0, dy1=dy1, scale1=sc1, dres=dres), dict(dy1=dy1, scale1=sc1)):
        def loss(xx):
            outs, _ = R.layernorm_mod(xx, scale=kw.get("scale0", torch.zeros_like(sc0)), shift=sh, scale2=kw.get("scale1"),
                                      shift2=sh if "scale1" in kw else None, rows_per_batch=rpb)
            return ((outs[0] * dy0).sum() + ((outs[1] * dy1).sum() if "dy1" in kw else 0.0)).item()
        ref = R.layernorm_mod_bwd(x, dy0, rows_per_batch=rpb, **kw)
        _close(ref, _fd(loss, x) + kw.get("dres", 0.0), 1e-7)
        form, mag = R.layernorm_mod_bwd_formula(x, dy0, rows_per_batch=rpb, **kw)
        _close(form, ref, 1e-12)
        assert (mag >= form.abs() * (1 - 1e-12)).all()
    nh, hpw = 4, 2
    xh, dyh = torch.randn(3, nh, 64, generator=g, dtype=F64), torch.randn(3, nh, 64, generator=g, dtype=F64)
    w = 1 + 0.1 * torch.randn(nh // hpw, 64, generator=g, dtype=F64)
    wsel = w[torch.arange(nh) // hpw]
    ref = R.rmsnorm_heads_bwd(xh, dyh, w, hpw)
    _close(ref, _fd(lambda xx: (xx * torch.rsqrt((xx * xx).mean(-1, keepdim=True) + 1e-6) * wsel * dyh).sum().item(), xh), 1e-7)
    form, mag, mag_in = R.rmsnorm_heads_bwd_formula(xh, dyh, w, hpw)
    _close(form, ref, 1e-12)
    assert (mag >= form.abs() * (1 - 1e-12)).all() and (mag_in >= 0).all()


def _aligned(t):
    return t is None or (t.stride(-1) == 1 and (t.dim() < 2 or t.stride(0) % 8 == 0) and t.storage_offset() % 8 == 0)


def test_every_input_of_the_gpu_file_constructs():
    for D in R.LN_DS:
        for M in R.LN_MS:
            for v in R.LN_VARIANTS:
                kw = R.ln_case(D, M, v)
                assert kw["x"].shape == (M, D) and all(_aligned(t) for t in kw.values() if torch.is_tensor(t))
                rpb = kw["rows_per_batch"]
                if kw.get("scale") is not None:
                    nb = kw["scale"].shape[0]
                    assert kw["scale"].shape == kw["shift"].shape == (nb, D) and kw["scale"].stride(0) == kw["shift"].stride(0) == 6 * D
                    assert nb == ((M - 1) // rpb + 1 if rpb else 1)
                    if rpb and M > 1:
                        assert M % rpb != 0                          # the last batch is partial
                assert (v == "xslice") == (kw["x"].stride(0) != D)
    for M, D in R.RMS_ROWS_SHAPES:
        kw = R.rms_rows_case(M, D)
        assert kw["x"].shape == (M, D) and kw["w"].shape == (D,)
    for nheads in R.HEADS_NHEADS:
        for col0 in R.HEADS_COL0:
            for seg in (False, True):
                buf, w, hpw, sg, M = R.heads_case(nheads, col0, seg)
                assert nheads % hpw == 0 and w.shape == (nheads // hpw, 64) and _aligned(buf)
                rows = R.seg_rows(M, sg)
                assert rows.max().item() < buf.shape[0] and len(set(rows.tolist())) == M < buf.shape[0]
                assert col0 + nheads * 64 + 8 <= buf.shape[1]
    assert set(R.HEADS_BWD_NHEADS) <= set(R.HEADS_NHEADS)
    for D in R.LNB_DS:
        for M in R.LNB_MS:
            assert M % R.LNB_RPB[M] != 0
            for v in R.LNB_VARIANTS:
                kw = R.lnb_case(D, M, v)
                assert all(_aligned(t) for t in kw.values() if torch.is_tensor(t)) and all(_aligned(t) for t in kw.get("gates", []))
                assert kw["x"].shape == kw["dy0"].shape == (M, D)
                assert kw.get("dy1") is None or (kw["dy1"].stride(0) == kw["dy0"].stride(0) and kw["scale1"].stride(0) == 6 * D)
                assert (kw.get("dy1") is None) == (kw.get("scale1") is None)
                assert v.endswith("strided") == (kw["x"].stride(0) != D)
    for n in R.UNARY_NS:
        x, x2 = R.unary_case(n)
        assert x.shape == x2.shape == (n,) and n % 8 == 0
    assert R.UNARY_NS[-1] // 8 > 2048 * 256                          # more chunks than the largest grid has threads
    assert set(R.SILU_EDGES) == {0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0}
    for B, C, H, W in R.PATCH_SHAPES:
        assert H % 2 == 0 and W % 2 == 0
    for D, M, rpb in R.GATE_SHAPES:
        assert D % 8 == 0 and M % rpb != 0
    assert set(R.TR_SEG) == set(R.TR_RS)


def test_float32_emulation_stays_within_c_f32():
    """C_F32's derivation (row_kernel_reference.py): every formula in torch float32 against float64 over every shape list; the worst ratio
    |f32 - f64| / (magnitude of the added terms), times 4, rounded up to a power of two, is C_F32.  Asserted with a factor 2 to spare, so
    that another libm or vector width does not trip it; the figures are printed."""
    f32 = torch.float32
    worst = {}

    def note(name, a32, a64, mag):
        ok = mag > 0
        assert torch.equal(a32.double()[~ok], a64[~ok])
        r = ((a32.double() - a64).abs()[ok] / mag[ok]).max().item() if ok.any() else 0.0
        worst[name] = max(worst.get(name, 0.0), r)

    for D in R.LN_DS:
        for M in R.LN_MS:
            for v in R.LN_VARIANTS:
                kw = R.ln_case(D, M, v)
                o64, mags = R.layernorm_mod(**kw)
                o32, _ = R.layernorm_mod(**kw, dtype=f32)
                for a, b, m in zip(o32, o64, mags):
                    note("layernorm_mod", a, b, m)
    for M, D in R.RMS_ROWS_SHAPES:
        kw = R.rms_rows_case(M, D)
        b = R.rmsnorm_rows(**kw, round_mid=False)[0]
        note("rmsnorm_rows", R.rmsnorm_rows(**kw, round_mid=False, dtype=f32)[0], b, b.abs())
    for nheads in R.HEADS_NHEADS:
        for col0 in R.HEADS_COL0:
            for seg in (False, True):
                buf, w, hpw, sg, M = R.heads_case(nheads, col0, seg)
                _, (b, _, _), rs64 = R.rmsnorm_heads(buf, col0, nheads, w, hpw, seg=sg, M=M, round_mid=False)
                _, (a, _, _), rs32 = R.rmsnorm_heads(buf, col0, nheads, w, hpw, seg=sg, M=M, round_mid=False, dtype=f32)
                note("rmsnorm_heads", a, b, b.abs())
                note("rs", rs32, rs64, rs64.abs())
                if nheads in R.HEADS_BWD_NHEADS:
                    x = buf[R.seg_rows(M, sg), col0:col0 + nheads * 64].reshape(M, nheads, 64)
                    dy = torch.randn(M, nheads, 64, generator=torch.Generator().manual_seed(nheads)).bfloat16()
                    b, mag, _ = R.rmsnorm_heads_bwd_formula(x, dy, w, hpw)
                    note("rmsnorm_heads_bwd", R.rmsnorm_heads_bwd_formula(x, dy, w, hpw, dtype=f32)[0], b, mag)
    for D in R.LNB_DS:
        for M in R.LNB_MS:
            for v in R.LNB_VARIANTS:
                kw = R.lnb_case(D, M, v)
                kw.pop("gates", None)
                b, mag = R.layernorm_mod_bwd_formula(**kw)
                note("layernorm_mod_bwd", R.layernorm_mod_bwd_formula(**kw, dtype=f32)[0], b, mag)
    for n in R.UNARY_NS:
        x, x2 = R.unary_case(n)
        for second in (None, x2):
            b, v = R.unary(x, "silu", second)
            note("silu", R.unary(x, "silu", second, dtype=f32)[0], b, (1 + v.abs()) * b.abs())
    for k, r in sorted(worst.items()):
        print(f"float32 / float64 worst ratio {k:20s} {r:.3e} = 2^{math.log2(r) if r > 0 else float('-inf'):.2f}")
    top = max(worst.values())
    print(f"worst {top:.3e}; C_F32 = {R.C_F32:.3e} = {R.C_F32 / top:.1f} x worst")
    assert 2 * top <= R.C_F32
    assert R.C_F32 == 2.0 ** math.ceil(math.log2(R.C_F32))           # a power of two
