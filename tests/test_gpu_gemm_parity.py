"""MI355X: every case of tests/gemm_reference.py through ops.gemm / gemm_grouped / gemm_train / bmm_nt against the float64 reference of the
whole epilogue, element by element, over the WHOLE allocation around each output (guard rows, pad columns and unmapped rows must keep
what they held).  The `exact` family is compared without a tolerance.  Cases that gemm_prepare must refuse assert the refusal's text and
that nothing was written.  One `PATH <kernel>:<path>: worst error / bound` line per path is printed at the end (pytest -s)."""
import pytest
import torch

import gemm_reference as G

pytestmark = pytest.mark.gpu

REFUSAL = {"refuse:ldc": "gemm: aux / d-activation needs ldc % 4 == 0 (ldc={})", "refuse:ldr": "gemm: aux / d-activation needs ldr % 4 == 0 (ldr={})",
           "refuse:gate_stride": "gemm: aux / d-activation needs gate_stride % 4 == 0 (gate_stride={})"}
_PATHS = {}


@pytest.fixture(scope="module", autouse=True)
def path_lines():
    yield
    print()
    for name, (r, n) in sorted(_PATHS.items()):
        print(f"PATH {name}: worst error / bound {r:.3f} over {n} cases")


def _sq(t):
    return None if t is None else t[0]


def _args(c, inp):
    return dict(bias=inp["bias"], act=c.act, alpha=c.alpha, gate=inp["gate"], gate_rows=c.gate_rows or 0, residual=_sq(inp["residual"]),
                out=inp["out"][0], M=c.M)


def _desc(ops, c, inp):
    return ops.gemm_desc(inp["a"][0], inp["w"][0], seg=c.seg, a_seg=c.a_seg, aux_out=_sq(inp["aux"]), aux_in=_sq(inp["aux_in"]), **_args(c, inp))


def _launch(ops, c, inp):
    a, w = inp["a"][0], inp["w"][0]
    if c.entry == "gemm":
        ops.gemm(a, w, seg=c.seg, a_seg=c.a_seg, **_args(c, inp))
    elif c.entry == "desc":
        ops.gemm_grouped([_desc(ops, c, inp)])
    elif c.entry == "train":
        assert c.seg is None and c.a_seg is None
        ops.gemm_train(a, w, aux_out=_sq(inp["aux"]), aux_in=_sq(inp["aux_in"]), splitk=c.splitk, **_args(c, inp))
    else:
        assert c.entry == "bmm"
        ops.bmm_nt(inp["a"][:, :c.M], inp["w"], out=inp["out"][:, :c.M], alpha=c.alpha)
    torch.cuda.synchronize()


def _check(c, inp, label):
    """Compare the allocations with the float64 reference; returns {"out": ..., "aux": ...} bounds for the callers that need them."""
    exp = G.expected(inp, G.reference(inp))
    worst = 0.0
    for key, (want, bound) in exp.items():
        got = inp["out_alloc"] if key == "out" else inp["aux_alloc"]
        ratio, bad = G.compare(got, want, bound)
        print(f"{c.name} [{label}] {key}: worst error / bound {ratio:.3f}, {bad} elements outside")
        assert bad == 0, (c.name, key, ratio)
        worst = max(worst, ratio)
    r, n = _PATHS.get(label, (0.0, 0))
    _PATHS[label] = (max(r, worst), n + 1)
    return exp


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_gemm_case_matches_float64_reference(name):
    from adv_grpo_amd import _lib, ops
    c = G.CASE[name]
    inp = G.make(c, "cuda")
    assert G.route(inp)[1] == c.path
    if c.confirm:
        assert _lib.load().advgrpo_gemm_variant(c.M, c.N, c.K, c.batch, 0) == c.kernel
    if c.path.startswith("refuse"):
        pitch = {"refuse:ldc": inp["out"].stride(1), "refuse:ldr": inp["residual"].stride(1) if inp["residual"] is not None else 0,
                 "refuse:gate_stride": inp["gate"].stride(0) if inp["gate"] is not None else 0}[c.path]
        with pytest.raises(_lib.AdvGrpoError) as e:
            _launch(ops, c, inp)
        assert str(e.value) == REFUSAL[c.path].format(pitch)
        assert torch.equal(inp["out_alloc"], inp["init"])                        # refused before any launch
        assert inp["aux_alloc"] is None or bool((inp["aux_alloc"] == G.SENTINEL).all())
        return
    _launch(ops, c, inp)
    exp = _check(c, inp, f"v{c.kernel}:{c.path}")
    if c.splitk > 1:                                                             # a second run: within the bound of the first, not bit for bit
        first = inp["out_alloc"].clone()
        inp["out_alloc"].copy_(inp["init"])
        _launch(ops, c, inp)
        _check(c, inp, f"v{c.kernel}:{c.path}")
        assert bool(((inp["out_alloc"].double() - first.double()).abs() <= exp["out"][1]).all())


@pytest.mark.parametrize("name", [p.name for p in G.PAIRS])
def test_paired_launch_matches_float64_reference(name):
    from adv_grpo_amd import ops
    p = {q.name: q for q in G.PAIRS}[name]
    ia, ib = G.make(p.first, "cuda"), G.make(p.second, "cuda")
    assert G.pair_route(ia, ib) == (p.kernel, p.first.path, p.second.path)
    ops.gemm_grouped([_desc(ops, p.first, ia), _desc(ops, p.second, ib)])
    torch.cuda.synchronize()
    _check(p.first, ia, f"pair v{p.kernel}:{p.first.path}")
    _check(p.second, ib, f"pair v{p.kernel}:{p.second.path}")


@pytest.mark.parametrize("name,kernel,M,N,K,seg", G.RMS_CASES)
def test_fused_qk_norm_equals_the_unfused_kernels(name, kernel, M, N, K, seg):
    """gemm with the per-head RMSNorm in its epilogue == gemm + rmsnorm_heads, bit for bit (the norm's values have their own float64 test)."""
    from adv_grpo_amd import ops
    c = G.Case(name, kernel, "rows" if kernel != 30 else "8p:bias_rms", M, N, K, bias=True, seg=seg, confirm=False)
    inp = G.make(c, "cuda")
    assert G.route(inp, rms=True) == (c.kernel, c.path)
    heads = N // 64
    nheads, hpw = (2, 1) if heads == 3 else (10, 5)                             # the last heads stay unnormalised (V of a fused QKV)
    g = torch.Generator().manual_seed(M + N)
    rw = (1 + 0.1 * torch.randn(nheads // hpw, 64, generator=g)).to(torch.bfloat16).cuda()
    rows = inp["out"].shape[1]
    rs = [torch.full((rows, nheads), G.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2)]
    fused, plain = inp["out_alloc"], inp["out_alloc"].clone()
    kw = dict(bias=inp["bias"], seg=c.seg, M=M)
    ops.gemm_grouped([ops.gemm_desc(inp["a"][0], inp["w"][0], out=fused[0, 1:-1, :N], rms=(rw, nheads, hpw, 1e-6, rs[0]), **kw)])
    ops.gemm(inp["a"][0], inp["w"][0], out=plain[0, 1:-1, :N], **kw)
    ops.rmsnorm_heads(plain[0, 1:-1, :N], 0, nheads, rw, hpw, seg=c.seg, M=M, rs_out=rs[1])
    torch.cuda.synchronize()
    assert torch.equal(fused, plain)
    assert torch.equal(rs[0], rs[1])
    assert bool((fused[0, 0] == G.SENTINEL).all()) and bool((fused[0, -1] == G.SENTINEL).all())
    assert bool((fused[0, 1:-1, :N][inp["out_rows"]] != G.SENTINEL).all())
