"""GPU parity of the bf16 MFMA GEMM (through the C ABI) against a plain PyTorch fp32 reference of the
same op (computed on the bf16-rounded operands)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(a, w, bias=None, act=None, alpha=1.0, gate=None, gate_rows=0, residual=None):
    y = alpha * (a.float() @ w.float().T)
    if bias is not None:
        y = y + bias.float()
    if act == "gelu_tanh":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    elif act == "gelu":
        y = torch.nn.functional.gelu(y)
    elif act == "silu":
        y = torch.nn.functional.silu(y)
    if gate is not None:
        idx = torch.arange(a.shape[0], device=a.device) // gate_rows
        y = y * gate.float()[idx]
    if residual is not None:
        y = y + residual.float()
    return y


def _check(out, ref, K):
    # bf16 output: half-ulp 2^-9 relative to the result, plus f32 accumulation noise ~ sqrt(K) * 2^-24 * |a||w|
    err = (out.float() - ref).abs()
    tol = 2 ** -8 * ref.abs() + 1e-3 * ref.abs().mean()
    assert (err <= tol).all(), f"max err {err.max().item()} (ref scale {ref.abs().mean().item()})"


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 128), (1229, 1536, 1536), (3280, 4608, 1536),
                                   (16384, 1536, 1536), (100, 64, 1536), (77, 200, 192), (16, 13824, 1536),
                                   (2057, 3072, 768)])
def test_gemm_plain(M, N, K):
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    # asymmetric, non-identity operands (transposes / fragment swaps would show)
    w = (torch.randn(N, K, device="cuda", generator=g) * (1 + torch.arange(N, device="cuda")[:, None] / N)
         ).to(torch.bfloat16)
    out = ops.gemm(a, w)
    _check(out, _ref(a, w), K)
    out32 = ops.gemm(a, w, out_dtype=torch.float32)
    ref = _ref(a, w)
    assert (out32 - ref).abs().max() <= 2e-3 * ref.abs().max()


@pytest.mark.parametrize("act", [None, "gelu_tanh", "gelu", "silu"])
def test_gemm_epilogue(act):
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    B, S, K, N = 4, 333, 256, 520
    M = B * S
    a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
    gate = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
    out = ops.gemm(a, w, bias=bias, act=act, alpha=0.5, gate=gate, gate_rows=S, residual=res)
    _check(out, _ref(a, w, bias, act, 0.5, gate, S, res), K)


def test_gemm_row_segments_scatter_into_joint_buffer():
    """image tokens -> rows [b*S, b*S+Ni), text tokens -> rows [b*S+Ni, (b+1)*S) of one buffer."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(4)
    B, Ni, Nt, K, N = 3, 64, 21, 128, 192
    S = Ni + Nt
    xi = torch.randn(B * Ni, K, device="cuda", generator=g).to(torch.bfloat16)
    xt = torch.randn(B * Nt, K, device="cuda", generator=g).to(torch.bfloat16)
    wi = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
    wt = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
    joint = torch.zeros(B * S, N, dtype=torch.bfloat16, device="cuda")
    ops.gemm(xi, wi, out=joint, seg=(Ni, S, 0))
    ops.gemm(xt, wt, out=joint, seg=(Nt, S, Ni))
    ref = torch.cat([(xi.float() @ wi.float().T).view(B, Ni, N), (xt.float() @ wt.float().T).view(B, Nt, N)], 1)
    _check(joint.view(B, S, N), ref, K)


def test_bmm_nt():
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(5, 300, 512, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(5, 260, 512, device="cuda", generator=g).to(torch.bfloat16)
    out = ops.bmm_nt(a, w, alpha=0.25)
    _check(out, 0.25 * torch.einsum("bmk,bnk->bmn", a.float(), w.float()), 512)


@pytest.mark.parametrize("shape", [(3, 64, 21, 128, 384), (16, 1024, 205, 256, 4608)])
def test_gemm_grouped_pair_with_fused_qk_norm(shape):
    """One launch for the image- and text-stream QKV projections with the per-head RMSNorm in the epilogue ==
    two launches + the standalone rmsnorm_heads kernel (bit for bit), and == an fp32 torch reference."""
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(6)
    B, Ni, Nt, K, N = shape
    S, H = Ni + Nt, N // 3 // 64
    xi = torch.randn(B * Ni, K, device="cuda", generator=g).to(torch.bfloat16)
    xt = torch.randn(B * Nt, K, device="cuda", generator=g).to(torch.bfloat16)
    wi = (torch.randn(N, K, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    wt = (torch.randn(N, K, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    bi = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
    bt = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
    rw_i = (1 + 0.1 * torch.randn(2, 64, device="cuda", generator=g)).to(torch.bfloat16)
    rw_t = (1 + 0.1 * torch.randn(2, 64, device="cuda", generator=g)).to(torch.bfloat16)
    # unfused: two launches + two norm kernels
    ref = torch.zeros(B * S, N, dtype=torch.bfloat16, device="cuda")
    rs_ref = torch.zeros(B * S, 2 * H, dtype=torch.float32, device="cuda")
    ops.gemm(xi, wi, bias=bi, out=ref, seg=(Ni, S, 0))
    ops.gemm(xt, wt, bias=bt, out=ref, seg=(Nt, S, Ni))
    plain = ref.clone()
    ops.rmsnorm_heads(ref, 0, 2 * H, rw_i, H, seg=(Ni, S, 0), M=B * Ni, rs_out=rs_ref)
    ops.rmsnorm_heads(ref, 0, 2 * H, rw_t, H, seg=(Nt, S, Ni), M=B * Nt, rs_out=rs_ref)
    # fused + grouped
    out = torch.zeros(B * S, N, dtype=torch.bfloat16, device="cuda")
    rs = torch.zeros(B * S, 2 * H, dtype=torch.float32, device="cuda")
    ops.gemm_grouped([ops.gemm_desc(xi, wi, bias=bi, out=out, seg=(Ni, S, 0), rms=(rw_i, 2 * H, H, 1e-6, rs)),
                      ops.gemm_desc(xt, wt, bias=bt, out=out, seg=(Nt, S, Ni), rms=(rw_t, 2 * H, H, 1e-6, rs))])
    assert torch.equal(out, ref)
    assert torch.equal(rs, rs_ref)
    # fp32 reference of the norm on the bf16 projection
    q = plain.float().view(B, S, 3, H, 64)
    wsel = torch.cat([rw_i.float().view(1, 1, 2, 1, 64).expand(B, Ni, 2, H, 64),
                      rw_t.float().view(1, 1, 2, 1, 64).expand(B, Nt, 2, H, 64)], 1)
    qk = q[:, :, :2]
    normed = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + 1e-6)
    want = torch.cat([normed.to(torch.bfloat16).float() * wsel, q[:, :, 2:]], 2).reshape(B * S, N)
    assert (out.float() - want).abs().max().item() <= 2e-2 * want.abs().max().item()


def test_gemm_grouped_pair_gate_residual_matches_two_launches():
    from adv_grpo_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    B, Ni, Nt, K, N = 16, 1024, 205, 512, 1536
    xi = torch.randn(B * Ni, K, device="cuda", generator=g).to(torch.bfloat16)
    xt = torch.randn(B * Nt, K, device="cuda", generator=g).to(torch.bfloat16)
    wi = (torch.randn(N, K, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    wt = (torch.randn(N, K, device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    bi = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
    gi = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
    gt = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
    ri = torch.randn(B * Ni, N, device="cuda", generator=g).to(torch.bfloat16)
    rt = torch.randn(B * Nt, N, device="cuda", generator=g).to(torch.bfloat16)
    a = ops.gemm(xi, wi, bias=bi, gate=gi, gate_rows=Ni, residual=ri)
    b = ops.gemm(xt, wt, act="gelu_tanh", gate=gt, gate_rows=Nt, residual=rt)
    oa, ob = ops.gemm_grouped([ops.gemm_desc(xi, wi, bias=bi, gate=gi, gate_rows=Ni, residual=ri),
                               ops.gemm_desc(xt, wt, act="gelu_tanh", gate=gt, gate_rows=Nt, residual=rt)])
    assert torch.equal(oa, a) and torch.equal(ob, b)


# ------------------------------------------------------------------------------------- flat entries against the descriptor entry, bit for bit
# One shape per tile variant a Linear can get (both forms choose alike): 15 ragged in both directions, 2, 1, and the eight-phase kernel (30)
# at its smallest admissible size.
FLAT_VS_DESC = [(130, 192, 64, 15), (48, 192, 128, 2), (130, 64, 64, 1), (8192, 1024, 64, 30)]


def _flat_vs_desc_operands(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    a, w = rnd(M, K).to(torch.bfloat16), (rnd(N, K) * 0.2).to(torch.bfloat16)
    bias, res = rnd(N).to(torch.bfloat16), rnd(M, N).to(torch.bfloat16)
    rows = 50
    gate = rnd((M + rows - 1) // rows, N).to(torch.bfloat16)
    return a, w, bias, res, gate, rows


@pytest.mark.parametrize("M,N,K,variant", FLAT_VS_DESC)
def test_gemm_equals_its_descriptor_form(M, N, K, variant):
    """ops.gemm (advgrpo_gemm_bf16) == ops.gemm_grouped of one ops.gemm_desc: bias + gelu_tanh; gate + residual in place; a row scatter of the
    output with a row gather of the input."""
    from adv_grpo_amd import _lib, ops
    assert _lib.load().advgrpo_gemm_variant(M, N, K, 1, 0) == variant
    a, w, bias, res, gate, rows = _flat_vs_desc_operands(M, N, K)
    one = lambda **kw: ops.gemm_grouped([ops.gemm_desc(**kw)])[0]
    assert torch.equal(ops.gemm(a, w, bias=bias, act="gelu_tanh"), one(a=a, w=w, bias=bias, act="gelu_tanh"))
    assert torch.equal(ops.gemm(a, w, out_dtype=torch.float32, alpha=0.5), one(a=a, w=w, out_dtype=torch.float32, alpha=0.5))
    r1, r2 = res.clone(), res.clone()
    assert ops.gemm(a, w, gate=gate, gate_rows=rows, residual=r1, out=r1) is r1
    one(a=a, w=w, gate=gate, gate_rows=rows, residual=r2, out=r2)
    assert torch.equal(r1, r2) and not torch.equal(r1, res)
    # rows [b * sa + 10, b * sa + 10 + h) of a joint input -> rows [b * so + 7, b * so + 7 + h) of a joint output, b = 0, 1
    h = M // 2
    sa, so = h + 15, h + 25
    joint = torch.zeros(2 * sa, K, dtype=torch.bfloat16, device="cuda")
    joint.view(2, sa, K)[:, 10:10 + h] = a[:2 * h].view(2, h, K)
    outs = [torch.full((2 * so, N), 3.0, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    ops.gemm(joint, w, bias=bias, out=outs[0], seg=(h, so, 7), a_seg=(h, sa, 10), M=2 * h)
    one(a=joint, w=w, bias=bias, out=outs[1], seg=(h, so, 7), a_seg=(h, sa, 10), M=2 * h)
    assert torch.equal(outs[0], outs[1])
    _check(outs[0].view(2, so, N)[:, 7:7 + h].reshape(2 * h, N), _ref(a[:2 * h], w, bias), K)
    assert (outs[0].view(2, so, N)[:, :7] == 3.0).all() and (outs[0].view(2, so, N)[:, 7 + h:] == 3.0).all()


@pytest.mark.parametrize("M,N,K,variant", FLAT_VS_DESC)
def test_gemm_train_equals_its_descriptor_form(M, N, K, variant):
    """ops.gemm_train (advgrpo_gemm_bf16_train) == ops.gemm_grouped of one ops.gemm_desc: the epilogues above, the pre-activation copy
    (aux_out) and the d-activation on aux_in."""
    from adv_grpo_amd import ops
    a, w, bias, res, gate, rows = _flat_vs_desc_operands(M, N, K)
    one = lambda **kw: ops.gemm_grouped([ops.gemm_desc(**kw)])[0]
    assert torch.equal(ops.gemm_train(a, w, bias=bias, act="gelu_tanh"), one(a=a, w=w, bias=bias, act="gelu_tanh"))
    r1, r2 = res.clone(), res.clone()
    ops.gemm_train(a, w, gate=gate, gate_rows=rows, residual=r1, out=r1)
    one(a=a, w=w, gate=gate, gate_rows=rows, residual=r2, out=r2)
    assert torch.equal(r1, r2) and not torch.equal(r1, res)
    pre = [torch.zeros(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    assert torch.equal(ops.gemm_train(a, w, bias=bias, act="gelu_tanh", aux_out=pre[0]), one(a=a, w=w, bias=bias, act="gelu_tanh", aux_out=pre[1]))
    assert torch.equal(pre[0], pre[1]) and pre[0].any()
    assert torch.equal(ops.gemm_train(a, w, act="dgelu_tanh", aux_in=pre[0]), one(a=a, w=w, act="dgelu_tanh", aux_in=pre[0]))


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_bmm_nt_equals_per_batch_gemm(out_dtype):
    """The batch strides are what only the flat entry sets: operands and output are slices of larger buffers (batch stride != M x pitch)."""
    from adv_grpo_amd import ops
    B, M, N, K = 3, 70, 130, 64
    g = torch.Generator(device="cuda").manual_seed(12)
    a = torch.randn(B, M + 10, K, device="cuda", generator=g).to(torch.bfloat16)[:, :M]
    w = torch.randn(B, N + 6, K, device="cuda", generator=g).to(torch.bfloat16)[:, 6:]
    buf = torch.full((B, M + 2, N), 3.0, dtype=out_dtype, device="cuda")
    out = ops.bmm_nt(a, w, out=buf[:, :M], alpha=0.25)
    for b in range(B):
        assert torch.equal(out[b], ops.gemm(a[b], w[b], alpha=0.25, out_dtype=out_dtype)), b
    assert (buf[:, M:] == 3.0).all()
    assert torch.equal(ops.bmm_nt(a, w, out_dtype=out_dtype, alpha=0.25), out)
