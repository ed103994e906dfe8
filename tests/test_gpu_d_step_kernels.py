"""GPU: the discriminator-step (D-step) kernels one by one against float64 references of the same bf16 inputs, at the shapes
where their loops and blocks change path, and the bitwise repeatability of both D-steps (no reduction on their path may
depend on the order in which workgroups finish: Adam turns last-bit noise on near-zero gradients into steps of +-lr).

Tolerances follow from the arithmetic, never from observed error:
  U8 = 2^-8   bf16 round-to-nearest of a result: |bf16(x) - x| <= 2^-8 |x| (8 significant bits);
  E  = 2^-24  f32 unit roundoff: a sum of k terms in any order is within (k - 1) E sum|terms| of the exact sum, every
              product / quotient / exp adds a few E relative.
Products of two bf16 values are exact in f32, so a dot product of bf16 inputs only carries the summation term."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U8 = 2.0 ** -8
E = 2.0 ** -24
f64, bf16, f32 = torch.float64, torch.bfloat16, torch.float32


def _lib():
    from adv_grpo_amd import _lib as L
    return L, L.load(), L.stream_ptr()


def _randn(g, *shape, scale=1.0, dtype=bf16):
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


def _assert_within(out, ref, tol, what):
    err = (out.double() - ref).abs()
    bad = err > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {err.numel()} outside the bound; worst excess "
                           f"{(err - tol).max().item():.3e}, max err {err.max().item():.3e}")


# ------------------------------------------------------------------ single-query (CLS) attention
ATTN_SHAPES = [(12, 16, 257, 80), (3, 4, 65, 64), (2, 2, 1, 64), (1, 3, 64, 80), (2, 2, 129, 128)]


def _cls_inputs(Bt, H, S, hd, seed, spike=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = H * hd
    qkv = _randn(g, Bt, S, 3 * D)
    if spike is not None:                       # one late key ~50x larger: the row maximum sits far behind the first 64 keys
        qkv[:, spike, D:2 * D] = (qkv[:, spike, D:2 * D].float() * 50).to(bf16)
    return qkv, g


def _cls_ref(qkv, H, hd, scale):
    Bt, S, _ = qkv.shape
    D = H * hd
    x = qkv.double()
    q = x[:, 0, :D].view(Bt, H, hd)
    k = x[:, :, D:2 * D].view(Bt, S, H, hd)
    v = x[:, :, 2 * D:].view(Bt, S, H, hd)
    s = torch.einsum("bhd,bshd->bhs", q * scale, k)
    p = torch.softmax(s, dim=-1)
    return q, k, v, s, p


@pytest.mark.parametrize("Bt,H,S,hd", ATTN_SHAPES)
def test_cls_attention_fwd(Bt, H, S, hd):
    _check_cls_fwd(Bt, H, S, hd, spike=None)


def test_cls_attention_fwd_late_maximum():
    _check_cls_fwd(2, 2, 129, 128, spike=100)
    _check_cls_fwd(3, 4, 257, 80, spike=250)


def _check_cls_fwd(Bt, H, S, hd, spike):
    L, lib, st = _lib()
    scale = hd ** -0.5
    D = H * hd
    qkv, g = _cls_inputs(Bt, H, S, hd, seed=Bt * 1000 + S + hd, spike=spike)
    o = torch.empty(Bt, D, dtype=bf16, device="cuda")
    probs = torch.empty(Bt, H, S, dtype=f32, device="cuda")
    L.check(lib.advgrpo_cls_attention_fwd(qkv.data_ptr(), o.data_ptr(), probs.data_ptr(), Bt, S, H, hd, scale, st))
    q, k, v, s, p = _cls_ref(qkv, H, hd, scale)
    # score error: q*scale is rounded once (E), the hd-term f32 dot adds (hd - 1) E sum|q k scale|
    ds = (hd + 1) * E * torch.einsum("bhd,bshd->bhs", (q * scale).abs(), k.abs())
    ds_max = ds.amax(dim=-1, keepdim=True)
    # p_k = exp(s_k - m) / sum: a shift of every score by <= ds_max moves p_k by <= 2 ds_max relative; __expf rounds its
    # argument times log2(e) (E |s - m|) and its result (2 E); the S-term sum, the reciprocal and the product add (S + 3) E
    arg = (s - s.amax(dim=-1, keepdim=True)).abs()
    # (x2: second-order terms; + 2^-126: f32 results below the smallest normal number are flushed to zero)
    tol_p = 2 * p * (2 * ds_max + 2 * E * (arg + 2) + (S + 3) * E) + 2.0 ** -126
    _assert_within(probs, p, tol_p, "probs")
    assert ((probs.double().sum(-1) - 1).abs() <= 2 * S * E + tol_p.sum(-1)).all()
    ref_o = torch.einsum("bhs,bshd->bhd", p, v).reshape(Bt, D)
    # o = bf16(sum_k p_k v_k): the probability errors times |v|, the S-term f32 sum, then one bf16 rounding
    pv = torch.einsum("bhs,bshd->bhd", tol_p, v.abs()).reshape(Bt, D)
    psum = torch.einsum("bhs,bshd->bhd", p, v.abs()).reshape(Bt, D)
    tol_o = U8 * ref_o.abs() + 2 * (pv + (S + 1) * E * psum)
    _assert_within(o, ref_o, tol_o, "o_cls")
    # only the CLS query row is read: other data in the query rows 1..S-1 changes nothing, bit for bit
    qkv2 = qkv.clone()
    qkv2[:, 1:, :D] = _randn(g, Bt, S - 1, D) if S > 1 else qkv2[:, 1:, :D]
    o2, probs2 = torch.empty_like(o), torch.empty_like(probs)
    L.check(lib.advgrpo_cls_attention_fwd(qkv2.data_ptr(), o2.data_ptr(), probs2.data_ptr(), Bt, S, H, hd, scale, st))
    assert torch.equal(o2, o) and torch.equal(probs2, probs)


@pytest.mark.parametrize("Bt,H,S,hd", ATTN_SHAPES)
def test_cls_attention_bwd(Bt, H, S, hd):
    L, lib, st = _lib()
    scale = hd ** -0.5
    D = H * hd
    qkv, g = _cls_inputs(Bt, H, S, hd, seed=7 + Bt * 1000 + S + hd)
    do = _randn(g, Bt, D)
    q, k, v, s, p = _cls_ref(qkv, H, hd, scale)
    probs = p.to(f32).contiguous()                 # the f32 probabilities the forward hands over (one rounding: E p)
    dqkv = torch.full((Bt, S, 3 * D), float("nan"), dtype=bf16, device="cuda")
    L.check(lib.advgrpo_cls_attention_bwd(qkv.data_ptr(), probs.data_ptr(), do.data_ptr(), dqkv.data_ptr(), Bt, S, H, hd, scale, st))
    assert not torch.isnan(dqkv.float()).any(), "part of a (b, h) slice was left unwritten"
    assert (dqkv[:, 1:, :D] == 0).all(), "dq of a non-CLS row must be exactly 0"
    # float64 autograd of single-query attention
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    pr = torch.softmax(torch.einsum("bhd,bshd->bhs", qr * scale, kr), dim=-1)
    out = torch.einsum("bhs,bshd->bhd", pr, vr)
    out.backward(do.double().view(Bt, H, hd))
    dO = do.double().view(Bt, H, hd)
    # dP_k = dO . v_k: hd-term f32 dot; delta = sum_k p_k dP_k: S-term sum of perturbed terms; dS_k = p_k (dP_k - delta)
    dp = torch.einsum("bhd,bshd->bhs", dO, v)
    e_dp = hd * E * torch.einsum("bhd,bshd->bhs", dO.abs(), v.abs())
    delta = (p * dp).sum(-1, keepdim=True)
    e_delta = (p * e_dp).sum(-1, keepdim=True) + (S + 2) * E * (p * dp.abs()).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    e_ds = p * (e_dp + e_delta) + 4 * E * p * (dp.abs() + delta.abs())
    # dk = bf16(scale dS_k q) ; dv = bf16(p_k dO) ; dq = bf16(scale sum_k dS_k k_k)
    ref_dk = kr.grad
    tol_dk = U8 * ref_dk.abs() + 2 * scale * q.abs().unsqueeze(1) * (e_ds + 3 * E * ds.abs()).permute(0, 2, 1).unsqueeze(-1)
    ref_dv = vr.grad
    tol_dv = U8 * ref_dv.abs() + 4 * E * ref_dv.abs()
    ref_dq = qr.grad.reshape(Bt, D)
    tol_dq = U8 * ref_dq.abs() + 2 * scale * (torch.einsum("bhs,bshd->bhd", e_ds, k.abs()) +
                                              (S + 2) * E * torch.einsum("bhs,bshd->bhd", ds.abs(), k.abs())).reshape(Bt, D)
    _assert_within(dqkv[:, :, D:2 * D].view(Bt, S, H, hd), ref_dk, tol_dk, "dk")
    _assert_within(dqkv[:, :, 2 * D:].view(Bt, S, H, hd), ref_dv, tol_dv, "dv")
    _assert_within(dqkv[:, 0, :D], ref_dq, tol_dq, "dq (CLS row)")


# ------------------------------------------------------------------ column sums and LayerNorm affine gradients
@pytest.mark.parametrize("R", [1, 63, 64, 65, 3084])
@pytest.mark.parametrize("C", [1, 8, 255, 256, 257, 3840])
def test_colsum_bf16(R, C):
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(R * 7 + C)
    full = _randn(g, R, C + 24)
    x = full[:, 5:5 + C]                                   # strided view: ld = C + 24 > C
    out0 = torch.randn(C, device="cuda", generator=g)
    out = out0.clone()
    L.check(lib.advgrpo_colsum_bf16(x.data_ptr(), x.stride(0), R, C, out.data_ptr(), st))
    ref = out0.double() + x.double().sum(0)
    # R partial sums plus the add into out: at most R + 17 roundings along any path of the fixed order
    tol = (R + 17) * E * (x.double().abs().sum(0) + out0.double().abs())
    _assert_within(out, ref, tol, "colsum")
    again = out0.clone()
    L.check(lib.advgrpo_colsum_bf16(x.data_ptr(), x.stride(0), R, C, again.data_ptr(), st))
    assert torch.equal(again, out), "colsum is not bitwise repeatable"


def _ln_affine(x, dy, gw, gb, eps):
    L, lib, st = _lib()
    M, D = x.shape
    ws = torch.empty(lib.advgrpo_ln_affine_grads_workspace_bytes(M) // 4, dtype=f32, device="cuda")
    L.check(lib.advgrpo_ln_affine_grads(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), M, D, eps, gw.data_ptr(),
                                        gb.data_ptr(), ws.data_ptr(), st))


@pytest.mark.parametrize("M", [1, 3, 12, 3084])
@pytest.mark.parametrize("D", [64, 80, 320, 1000, 1280])
def test_ln_affine_grads(M, D):
    g = torch.Generator(device="cuda").manual_seed(M * 11 + D)
    eps = 1e-5
    x = (torch.randn(M, D + 40, device="cuda", generator=g) + 30).to(bf16)[:, 8:8 + D]     # ldx = D + 40, mean ~ +30
    dy = _randn(g, M, D + 16)[:, :D]                                                    # lddy = D + 16
    gw0, gb0 = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
    gw, gb = gw0.clone(), gb0.clone()
    _ln_affine(x, dy, gw, gb, eps)
    xd, dyd = x.double(), dy.double()
    mu = xd.mean(1, keepdim=True)
    xc = xd - mu
    rstd = 1 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    xhat = xc * rstd
    ref_w, ref_b = gw0.double() + (dyd * xhat).sum(0), gb0.double() + dyd.sum(0)
    # mean: D-term sum -> |d mu| <= D E mean|x|; x - mu adds E |x - mu|; var: D-term sum of squares and rsqrtf -> rstd relative
    # (D / 2 + 4) E; each product dy * xhat adds 3 E; then the M-row sum (+16 wave partials + the add into gw): (M + 17) E
    d_mu = D * E * xd.abs().mean(1, keepdim=True)
    e_xhat = (d_mu + E * xc.abs()) * rstd + xhat.abs() * ((D / 2 + 4) * E)
    tol_w = 2 * ((dyd.abs() * (e_xhat + 3 * E * xhat.abs())).sum(0) + (M + 17) * E * ((dyd * xhat).abs().sum(0) + gw0.double().abs()))
    tol_b = (M + 17) * E * (dyd.abs().sum(0) + gb0.double().abs())
    _assert_within(gw, ref_w, tol_w, "ln grad_w")
    _assert_within(gb, ref_b, tol_b, "ln grad_b")
    gw2, gb2 = gw0.clone(), gb0.clone()
    _ln_affine(x, dy, gw2, gb2, eps)
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb), "ln_affine_grads is not bitwise repeatable"


# ------------------------------------------------------------------ DINO head
@pytest.mark.parametrize("D", [8, 520, 1024])
@pytest.mark.parametrize("n", [0, 5, 64])
def test_gather_rows(D, n):
    L, lib, st = _lib()
    B, T = 3, 37
    g = torch.Generator(device="cuda").manual_seed(D + n)
    feats = _randn(g, B, T, D)
    idx = torch.randint(0, T - 1, (B, n), device="cuda", generator=g)
    if n >= 3:
        idx[0, 0], idx[1, 1], idx[2, 2] = 0, T - 2, idx[2, 0]          # first / last patch, a repeated index
    out = torch.full((B * (1 + n), D), float("nan"), dtype=bf16, device="cuda")
    L.check(lib.advgrpo_gather_rows(feats.data_ptr(), idx.data_ptr() if n else None, out.data_ptr(), B, T, D, n, st))
    ref = torch.cat([feats[:, :1], torch.gather(feats[:, 1:], 1, idx[..., None].expand(B, n, D))], dim=1).reshape(-1, D)
    assert torch.equal(out, ref)


def _dino_weight(row, n, Breal, Btot, pw):
    b, j = divmod(row, 1 + n)
    real = b < Breal
    nb = Breal if real else Btot - Breal
    return real, j == 0, (0.5 / nb if j == 0 else pw * 0.5 / (nb * n))


@pytest.mark.parametrize("Hd", [16, 512, 520])
@pytest.mark.parametrize("Breal,Btot,n", [(3, 5, 4), (2, 3, 64), (4, 8, 6)])
def test_dino_head_loss(Hd, Breal, Btot, n):
    L, lib, st = _lib()
    R, pw = Btot * (1 + n), 0.3
    g = torch.Generator(device="cuda").manual_seed(Hd * 3 + R)
    h = _randn(g, R, Hd, scale=0.2)
    h[0] = 0                                          # real CLS row with logit = b2 = 1 exactly: margin 0, no gradient
    w2 = _randn(g, Hd, scale=0.2)
    b2 = torch.ones(1, dtype=bf16, device="cuda")
    logits, dl = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    stats = torch.full((4,), float("nan"), device="cuda")
    L.check(lib.advgrpo_dino_head_loss(h.data_ptr(), w2.data_ptr(), b2.data_ptr(), R, Hd, n, Breal, Btot, pw, logits.data_ptr(),
                                       dl.data_ptr(), stats.data_ptr(), st))
    ref = h.double() @ w2.double() + 1.0
    # the Hd-term f32 dot plus b2, then the bf16 rounding the kernel applies to the logit
    tol = U8 * ref.abs() + 2 * (Hd + 1) * E * ((h.double() * w2.double()).abs().sum(1) + 1.0)
    _assert_within(logits, ref, tol, "logits")
    assert torch.equal(logits, logits.to(bf16).float()), "logits must be bf16 values"
    assert logits[0].item() == 1.0 and dl[0].item() == 0.0
    lg = logits.double().cpu()
    exp_dl, loss, cr, cf = torch.zeros(R, dtype=f64), 0.0, 0, 0
    terms = []
    for r in range(R):
        real, cls, w = _dino_weight(r, n, Breal, Btot, pw)
        y = 1.0 if real else -1.0
        m = 1.0 - y * lg[r].item()
        exp_dl[r] = -y * w if m > 0 else 0.0
        terms.append(m * w if m > 0 else 0.0)
        if cls and y * lg[r].item() > 0:
            cr, cf = (cr + 1, cf) if real else (cr, cf + 1)
    # dl = -y * wgt: two f32 divisions / products -> 3 E relative
    _assert_within(dl.cpu(), exp_dl, 3 * E * exp_dl.abs(), "dlogits")
    s = stats.cpu().double()
    at = torch.tensor(terms, dtype=f64).abs().sum().item()
    assert abs(s[0].item() - sum(terms)) <= (R + 16) * E * at + 4 * E * at, (s[0].item(), sum(terms))
    assert (s[1].item(), s[2].item()) == (cr, cf)
    assert abs(s[3].item() - dl.double().sum().item()) <= (R + 16) * E * dl.double().abs().sum().item()
    # repeatable bit for bit
    stats2, l2, d2 = torch.empty_like(stats), torch.empty_like(logits), torch.empty_like(dl)
    L.check(lib.advgrpo_dino_head_loss(h.data_ptr(), w2.data_ptr(), b2.data_ptr(), R, Hd, n, Breal, Btot, pw, l2.data_ptr(),
                                       d2.data_ptr(), stats2.data_ptr(), st))
    assert torch.equal(stats2, stats) and torch.equal(l2, logits) and torch.equal(d2, dl)


@pytest.mark.parametrize("Hd", [16, 255, 256, 257, 512])
@pytest.mark.parametrize("R", [1, 31, 33, 130])
def test_dino_head_dpre(Hd, R):
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(Hd * 5 + R)
    pre = _randn(g, R, Hd, scale=2.0)
    h = _randn(g, R, Hd)
    w2 = _randn(g, Hd, scale=0.1)
    dl = torch.randn(R, device="cuda", generator=g) * 0.05
    dl[::3] = 0
    gw0, gb0 = torch.randn(Hd, device="cuda", generator=g), torch.randn(Hd, device="cuda", generator=g)
    gw, gb = gw0.clone(), gb0.clone()
    dpre = torch.full((R, Hd), float("nan"), dtype=bf16, device="cuda")
    L.check(lib.advgrpo_dino_head_dpre(pre.data_ptr(), h.data_ptr(), w2.data_ptr(), dl.data_ptr(), dpre.data_ptr(), gw.data_ptr(),
                                       gb.data_ptr(), R, Hd, st))
    u = pre.double()
    dgelu = 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    dw = dl.double()[:, None] * w2.double()[None, :]
    v = dw * dgelu
    # GELU'(u) in f32: erff (<= 2 ulp of a value <= 1) and __expf of -u^2/2 (argument rounding u^2 E, result 2 E), then
    # four products / sums (4 E); v = dl * w2 * GELU' adds 2 E.  dpre = bf16(v).
    e_dg = 4 * E + (u * torch.exp(-0.5 * u * u)).abs() / math.sqrt(2 * math.pi) * ((u * u + 4) * E) + 4 * E * dgelu.abs()
    e_v = dw.abs() * e_dg + 2 * E * v.abs()
    _assert_within(dpre, v, U8 * v.abs() + e_v, "dpre")
    # the column sums over R rows (+16 wave partials + the add into the buffer)
    ref_b = gb0.double() + v.sum(0)
    tol_b = e_v.sum(0) + (R + 17) * E * (v.abs().sum(0) + gb0.double().abs())
    _assert_within(gb, ref_b, tol_b, "grad_b1")
    dh = dl.double()[:, None] * h.double()
    ref_w = gw0.double() + dh.sum(0)
    tol_w = (R + 18) * E * (dh.abs().sum(0) + gw0.double().abs())
    _assert_within(gw, ref_w, tol_w, "grad_w2")
    gw2, gb2, dpre2 = gw0.clone(), gb0.clone(), torch.empty_like(dpre)
    L.check(lib.advgrpo_dino_head_dpre(pre.data_ptr(), h.data_ptr(), w2.data_ptr(), dl.data_ptr(), dpre2.data_ptr(), gw2.data_ptr(),
                                       gb2.data_ptr(), R, Hd, st))
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb) and torch.equal(dpre2, dpre)


# ------------------------------------------------------------------ weight-gradient GEMM as the D-steps call it
@pytest.mark.parametrize("tokens", [3084, 2 * 6 * 65])
@pytest.mark.parametrize("splitk", [1, 2, 16])
def test_weight_gradient_gemm(tokens, splitk):
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(tokens + splitk)
    n_out, n_in = 320, 200
    dy = _randn(g, tokens, n_out)
    x = _randn(g, tokens, n_in)
    acc0 = torch.randn(n_out, n_in, device="cuda", generator=g)
    acc = acc0.clone()
    T = ops.transpose
    ops.gemm_train(T(dy), T(x), out=acc, splitk=splitk)       # acc += dy^T x, contraction over the zero-padded token axis
    prod = dy.double().T @ x.double()
    ref = acc0.double() + prod
    # exact bf16 products, a K-term f32 sum (any order), splitk partials and the add into acc
    tol = (tokens + splitk + 2) * E * ((dy.double().abs().T @ x.double().abs()) + acc0.double().abs())
    _assert_within(acc, ref, tol, f"dW (splitk={splitk})")
    if splitk == 1:                     # the fixed-order accumulation the D-steps use: bit for bit repeatable
        again = acc0.clone()
        ops.gemm_train(T(dy), T(x), out=again)
        assert torch.equal(again, acc)


# ------------------------------------------------------------------ gradient norm and AdamW
@pytest.mark.parametrize("n", [1, 1023, 1025, 1024 * 1024 + 3, 5 * 1024 * 1024])
def test_sumsq_f32(n):
    L, lib, st = _lib()
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    x = torch.randn(n, device="cuda", generator=g)
    ws = torch.empty(lib.advgrpo_sumsq_workspace_bytes() // 4, dtype=f32, device="cuda")
    out = torch.full((1,), 3.0, device="cuda")
    L.check(lib.advgrpo_sumsq_f32(x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), st))
    ref = 3.0 + (x.double() ** 2).sum().item()
    # stage 1: <= ceil(n / (blocks * 256)) terms per thread, then a 256-lane tree (8 levels); stage 2: <= 4 partials per thread,
    # another tree, the add into out; each square adds one rounding: all terms are positive, so the bound is relative
    nb = min((n + 1023) // 1024, 1024)
    depth = -(-n // (nb * 256)) + 8 + 4 + 8 + 2
    assert abs(out.item() - ref) <= depth * E * ref, (out.item(), ref)
    out2 = torch.full((1,), 3.0, device="cuda")
    L.check(lib.advgrpo_sumsq_f32(x.data_ptr(), n, out2.data_ptr(), ws.data_ptr(), st))
    assert torch.equal(out2, out)


ADAM_SETUPS = {
    "g_step_clipped": dict(lr=3e-4, betas=(0.9, 0.999), wd=1e-4, clip=0.5, scale=1.0),
    "g_step_unclipped": dict(lr=3e-4, betas=(0.9, 0.999), wd=1e-4, clip=100.0, scale=1.0),
    "g_step_grad_scale": dict(lr=3e-4, betas=(0.9, 0.999), wd=1e-4, clip=0.5, scale=0.5),
    "d_step": dict(lr=1e-4, betas=(0.5, 0.999), wd=0.0, clip=None, scale=1.0),
}


@pytest.mark.parametrize("setup", list(ADAM_SETUPS) + ["d_step_at_1000"])
def test_adamw_step_vs_torch(setup):
    L, lib, st = _lib()
    c = ADAM_SETUPS["d_step" if setup == "d_step_at_1000" else setup]
    lr, (b1, b2), wd, eps = c["lr"], c["betas"], c["wd"], 1e-8
    n, steps = 4099, 5
    start = 999 if setup == "d_step_at_1000" else 0
    g = torch.Generator(device="cuda").manual_seed(len(setup))
    p32 = torch.randn(n, device="cuda", generator=g)
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    if start:                  # step 1000: moments carried in from step 999
        m = torch.randn(n, device="cuda", generator=g) * 0.01
        v = torch.rand(n, device="cuda", generator=g) * 1e-3 + 1e-4
    p16 = p32.to(bf16)
    ref = p32.double().clone().requires_grad_(True)
    opt = (torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False) if wd else
           torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps, foreach=False))
    if start:
        opt.state[ref] = {"step": torch.tensor(float(start), dtype=f64), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    ws = torch.empty(lib.advgrpo_sumsq_workspace_bytes() // 4, dtype=f32, device="cuda")
    grad = torch.empty(n, device="cuda")
    # Error bounds carried along in float64 (the kernel's arithmetic, step by step):
    #   clip factor: f32 sum of squares (<= 26 roundings deep for n = 4099, see test_sumsq_f32), sqrt, max_norm rounded to f32,
    #     one division -> dc <= 32 E relative (0 when clipping is off: fminf(1, .) returns 1 exactly; grad_scale 0.5 is exact);
    #   m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2: three roundings each, plus the clip factor's error on g (twice on g^2);
    #   update u = m^ / (sqrt(v^) + eps): the error of m^ over sqrt(v^), |u| (ev / 2v + 8 E) for v, the sqrt, the division, lr;
    #   the kernel takes beta1 / beta2 as f32: its (1 - beta) factors are off by |f32(beta) - beta| / (1 - beta) relative (for
    #     0.999: 1.3e-5, systematic) and its bias corrections 1 - beta^t by |f32(beta)^t - beta^t| (both exact, below);
    #   w: decayed, then stepped: 2 E |w| per step.  Everything x2 for second-order terms.
    bf1, bf2 = float(torch.tensor(b1, dtype=f32)), float(torch.tensor(b2, dtype=f32))
    dc = 32 * E if c["clip"] is not None and c["clip"] < 1 else 0.0
    r1, r2 = abs(bf1 - b1) / (1 - b1) + E, abs(bf2 - b2) / (1 - b2) + E
    em = torch.zeros(n, dtype=f64, device="cuda")
    ev = torch.zeros(n, dtype=f64, device="cuda")
    ep = torch.zeros(n, dtype=f64, device="cuda")
    for k in range(steps):
        t = start + k + 1
        gk = torch.randn(n, device="cuda", generator=g) * 0.05
        grad.copy_(gk)
        sumsq = torch.zeros(1, device="cuda")
        if c["clip"] is not None:
            L.check(lib.advgrpo_sumsq_f32(grad.data_ptr(), n, sumsq.data_ptr(), ws.data_ptr(), st))
            max_norm = c["clip"] * (gk.double().norm().item() * c["scale"])      # 0.5: clipping active; 100: inactive
        else:
            max_norm = 0.0
        L.check(lib.advgrpo_adamw_step(p32.data_ptr(), p16.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps,
                                       wd, t, sumsq.data_ptr() if c["clip"] is not None else None, max_norm, c["scale"], st))
        ref.grad = gk.double() * c["scale"]
        if c["clip"] is not None:
            torch.nn.utils.clip_grad_norm_([ref], max_norm)
        sref = opt.state.get(ref, {})
        m_prev = sref["exp_avg"].abs().clone() if "exp_avg" in sref else torch.zeros(n, dtype=f64, device="cuda")
        v_prev = sref["exp_avg_sq"].clone() if "exp_avg_sq" in sref else torch.zeros(n, dtype=f64, device="cuda")
        ge = ref.grad.abs()
        opt.step()
        m_ref, v_ref = opt.state[ref]["exp_avg"], opt.state[ref]["exp_avg_sq"]
        em = b1 * em + 3 * E * (b1 * m_prev + (1 - b1) * ge) + (1 - b1) * ge * (dc + r1) + abs(bf1 - b1) * m_prev
        ev = b2 * ev + 3 * E * (b2 * v_prev + (1 - b2) * ge * ge) + (1 - b2) * ge * ge * (2 * dc + 2 * E + r2) + abs(bf2 - b2) * v_prev
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        rb = abs(bf1 ** t - b1 ** t) / bc1 + 0.5 * abs(bf2 ** t - b2 ** t) / bc2
        den = (v_ref / bc2).sqrt() + eps
        u = (m_ref / bc1) / den
        du = (em / bc1) / den + u.abs() * (0.5 * ev / v_ref + 8 * E + rb)
        ep = ep + lr * du + 2 * E * ref.detach().abs()
    _assert_within(p32, ref.detach(), 2 * ep, f"AdamW params ({setup})")
    _assert_within(m, opt.state[ref]["exp_avg"], 2 * em, "exp_avg")
    _assert_within(v, opt.state[ref]["exp_avg_sq"], 2 * ev, "exp_avg_sq")
    assert torch.equal(p16, p32.to(bf16))
    assert (grad == 0).all()


# ------------------------------------------------------------------ bitwise repeatability of the D-steps
def _vit_h_clip(seed=12):
    from adv_grpo_amd import synthetic, vit
    from oracle import vit as o
    cfg = o.ClipConfig(v_hidden=1280, v_layers=2, v_heads=16, v_mlp=5120, image_size=224, t_hidden=256, t_layers=2, t_heads=4,
                       t_mlp=512, vocab=1000, proj=1024, eos_token_id=999)
    W = {k: v.to(torch.bfloat16) for k, v in synthetic.clip_weights(cfg, seed).items()}
    return vit.CLIPModel(W, cfg, "cuda"), cfg


def _clip_batch(cfg, B=6, seed=5):
    g = torch.Generator().manual_seed(seed)
    side, grid = cfg.image_size, cfg.image_size // 14
    px = torch.randn(2 * B, 3, side, side, generator=g).to(torch.bfloat16)
    ids = torch.randint(1, 990, (B, 77), generator=g)
    ids[:, 20] = 999
    patches = torch.zeros(2 * B * grid * grid, 640, dtype=torch.bfloat16)
    patches[:, :588] = px.view(2 * B, 3, grid, 14, grid, 14).permute(0, 2, 4, 1, 3, 5).reshape(2 * B * grid * grid, 588)
    l0 = torch.rand(B, generator=g)
    l0[0] = 0.5
    labels = (l0.cuda(), (1 - l0).cuda())                     # row 0: a tie (label_0 == label_1)
    return patches.cuda(), ids.cuda(), labels


def _state(tr):
    return {k: getattr(tr, k).clone() for k in ("params", "p16", "grads", "exp_avg", "exp_avg_sq")}, tr.opt_step


def _restore(tr, saved):
    s, step = saved
    for k, t in s.items():
        getattr(tr, k).copy_(t)                               # copy_: p16 stays the tensor the model's layers alias
    tr.opt_step = step


@pytest.mark.parametrize("kind", ["last_layer", "layers_-2"])
def test_pickscore_d_step_is_bitwise_repeatable(kind):
    from adv_grpo_amd.d_step_pickscore import ClipLastLayerTrainable, ClipLayersTrainable
    model, cfg = _vit_h_clip()
    tr = ClipLastLayerTrainable(model) if kind == "last_layer" else ClipLayersTrainable(model, -2)
    patches, ids, labels = _clip_batch(cfg)
    for lab in (None, labels):
        tr.grads.zero_()
        loss_a = tr.loss_and_grads(patches, ids, lab).clone()
        grads_a = tr.grads.clone()
        tr.grads.zero_()
        loss_b = tr.loss_and_grads(patches, ids, lab).clone()
        assert torch.isfinite(loss_a) and grads_a.abs().sum() > 0
        assert torch.equal(loss_a, loss_b), ("loss", lab is not None)
        assert torch.equal(grads_a, tr.grads), ("grads", lab is not None, int((grads_a != tr.grads).sum()))
    saved = _state(tr)
    tr.adam_step(1e-4)
    after = tr.params.clone()
    _restore(tr, saved)
    tr.adam_step(1e-4)
    assert not torch.equal(after, saved[0]["params"]) and torch.equal(tr.params, after)


def test_dino_head_d_step_is_bitwise_repeatable():
    from adv_grpo_amd.d_step import DinoHeadTrainable
    D, Hd, B, n, N = 1024, 512, 4, 64, 256
    head = DinoHeadTrainable(in_dim=D, hidden_dim=Hd, device="cuda", seed=3)
    g = torch.Generator(device="cuda").manual_seed(9)
    fr, ff = _randn(g, B, 1 + N, D), _randn(g, B, 1 + N, D, scale=1.3)
    ir = torch.randint(0, N, (B, n), device="cuda", generator=g)
    i_f = torch.randint(0, N, (B, n), device="cuda", generator=g)
    out = []
    for _ in range(2):
        head.grads.zero_()
        loss, acc = head.loss_and_grads(fr, ff, ir, i_f)
        out.append((loss.clone(), acc.clone(), head.grads.clone()))
    (la, aa, ga), (lb, ab, gb) = out
    assert ga.abs().sum() > 0
    assert torch.equal(la, lb) and torch.equal(aa, ab)
    assert torch.equal(ga, gb), int((ga != gb).sum())


def test_dino_trainer_d_step_after_resume_is_bitwise_identical(tmp_path):
    """A trainer restored from a checkpoint takes the SAME D-step as the original from the same samples: the head's parameters and
    both Adam moments agree bit for bit (train_dino draws its patch indices on the device: the generator is reseeded alike)."""
    from tests.test_gpu_trainer import _build
    tr_a, _, head_a = _build("dino", d_times=2, save_dir=str(tmp_path))
    tr_a.run_epoch()                                   # epoch 0: a D-step, so the head's Adam moments are non-zero
    path = tr_a.save_checkpoint()
    tr_b, _, head_b = _build("dino", d_times=2, save_dir=str(tmp_path))
    assert tr_b.load_checkpoint(path) is True
    samples = tr_a.sample_epoch()
    before = head_a.params.clone()
    for tr_ in (tr_a, tr_b):
        torch.cuda.manual_seed(1234)
        tr_.d_step(samples)
    assert not torch.equal(head_a.params, before)
    for f in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(head_a, f), getattr(head_b, f)), f
