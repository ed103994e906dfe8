"""CPU: the float64 reference of tests/gemm_reference.py against independent torch formulations, the branch every case declares against
the dispatcher's conditions, the float32 constant C_GEMM, the emulation against every bound, every mutant on its named case, and the two
conditions of the `exact` and `cancelling` input families.  Every input of tests/test_gpu_gemm_parity.py is constructed here once."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_reference as G

F64 = torch.float64
BIG = 8192


@pytest.fixture(scope="module")
def runs():
    """name -> (inp, float64 Result, float32 Result) of every single case that is not a refusal; the references are computed once."""
    out = {}
    for c in G.CASES:
        if c.path.startswith("refuse"):
            continue
        inp = G.make(c)
        out[c.name] = (inp, G.reference(inp, F64), G.reference(inp, torch.float32))
    return out


def test_case_lists_stay_within_the_budget_and_reach_what_they_declare():
    assert len(G.CASES) + 2 * len(G.PAIRS) + len(G.RMS_CASES) <= 150
    big = sum(c.M >= BIG for c in G.CASES) + sum(p.first.M >= BIG for p in G.PAIRS) + sum(r[2] >= BIG for r in G.RMS_CASES)
    assert big <= 20
    assert all(c.K <= 320 for c in G.CASES if c.K != 1536) and sum(c.K == 1536 for c in G.CASES) == 2
    assert all(c.M <= 130 and c.N <= 200 for c in G.CASES if c.K == 1536)
    assert {c.K // 64 % 2 for c in G.CASES} == {0, 1}                            # odd and even k-tile counts
    for c in G.CASES:
        inp = G.make(c)
        v, path = G.route(inp)
        assert path == c.path and (v is None or v == c.kernel), (c.name, v, path)
        if c.confirm:                                                            # what advgrpo_gemm_variant(M, N, K, batch) answers by itself
            assert G.gemm_variant(c.M, c.N, c.K, c.batch, True) == c.kernel, c.name
    for p in G.PAIRS:
        v, pa, pb = G.pair_route(G.make(p.first), G.make(p.second))
        assert (v, pa, pb) == (p.kernel, p.first.path, p.second.path), p.name
        assert (p.first.M, p.first.N, p.first.K) != (p.second.M, p.second.N, p.second.K) and pa != pb
    # every kernel x path cell the issue lists is reached, every eight-phase class, and every mutant names a case
    cells = {(c.kernel, c.path) for c in G.CASES}
    for k in (1, 2, 15, 26):
        assert {(k, "rows"), (k, "frag_vec"), (k, "frag_scalar")} <= cells, k
    assert {(0, "splitk"), (15, "acc_vec"), (15, "acc_scalar")} <= cells
    assert {p for k, p in cells if k == 30} | {"8p:bias_rms"} == {"8p:" + n for n in ("plain", "bias", "bias_rms", "bias_gelu", "bias_gate_res",
                                                                                      "bias_gelu_aux", "dgelu", "generic")}
    assert {c.path for c in G.CASES if c.path.startswith("refuse")} == {"refuse:ldc", "refuse:ldr", "refuse:gate_stride"}
    assert set(G.MUTANTS.values()) <= set(G.CASE)


def test_reference_matches_functional_linear_and_activations():
    for name in ("v15-rows-bias", "v15-frag_vec-gelu_tanh", "v15-rows-gelu", "v15-frag_scalar-silu", "v15-rows-quick_gelu", "v1r-frag_scalar-full",
                 "v15-frag_vec-seg21", "v15-rows-seg50-aseg", "v2m1-rows-full", "v15-rows-aux"):
        c = G.CASE[name]
        inp = G.make(c)
        ref = G.reference(inp)
        a = torch.stack([inp["a"][0, int(r)] for r in inp["a_rows"]]).to(F64)
        y = F.linear(a, c.alpha * inp["w"][0].to(F64)) + (inp["bias"].to(F64) if c.bias else 0.0)
        if c.aux_out:
            assert (ref.aux[0] - y).abs().max() <= 1e-12 * y.abs().max()
        if c.act == "gelu_tanh":
            y = F.gelu(y, approximate="tanh")
        elif c.act == "gelu":
            y = F.gelu(y)
        elif c.act == "silu":
            y = F.silu(y)
        elif c.act == "quick_gelu":
            y = y * torch.sigmoid(1.702 * y)
        for m in range(c.M):
            row = y[m]
            if c.gate_rows is not None:
                row = row * inp["gate"][m // c.gate_rows if c.gate_rows else 0].to(F64)
            if c.residual:
                orow = (m // c.seg[0]) * c.seg[1] + c.seg[2] + m % c.seg[0] if c.seg else m
                assert int(ref.out_rows[m]) == orow
                row = row + (inp["init"][0, 1 + orow, :c.N] if c.inplace else inp["residual"][0, orow]).to(F64)
            assert (ref.value[0, m] - row).abs().max() <= 1e-12 * max(1.0, float(row.abs().max())), (name, m)
        assert (ref.mag >= ref.value.abs() * (1 - 1e-12)).all()                  # the magnitudes dominate the values they bound


def test_d_activations_match_autograd():
    z = torch.linspace(-9.0, 9.0, 2001, dtype=F64)
    for act, fwd in (("dgelu_tanh", lambda t: F.gelu(t, approximate="tanh")), ("dgelu", F.gelu), ("mul_aux", lambda t: 0.5 * t * t)):
        zr = z.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(fwd(zr).sum(), zr)
        f, fmag = G.dact_value(z, act)
        assert (f - g).abs().max() <= 1e-12
        assert (fmag >= f.abs() * (1 - 1e-12)).all() or act == "mul_aux"
    for act in G.ACTS:                                                           # |act'| of the magnitudes is autograd's derivative
        zr = z.clone().requires_grad_(True)
        y, dabs, emag = G.act_value(zr, act)
        (g,) = torch.autograd.grad(y.sum(), zr)
        assert (dabs.detach() - g.abs()).abs().max() <= 1e-12
        assert (emag.detach() >= y.detach().abs() * (1 - 1e-12)).all()
    # and the whole d-activation epilogue: value = (alpha acc + bias) * f(aux_in)
    for name in ("v15-rows-dgelu_tanh", "v15-frag_vec-dgelu", "v15-rows-mul_aux"):
        c = G.CASE[name]
        inp = G.make(c)
        ref = G.reference(inp)
        pre = F.linear(inp["a"][0, :c.M].to(F64), c.alpha * inp["w"][0].to(F64)) + (inp["bias"].to(F64) if c.bias else 0.0)
        want = pre * G.dact_value(inp["aux_in"][0, :c.M].to(F64), c.act)[0]
        assert (ref.value[0] - want).abs().max() <= 1e-12 * want.abs().max()


def test_batch_accumulate_and_splitk_references():
    c = G.CASE["v15-acc_scalar"]
    inp = G.make(c)
    ref = G.reference(inp)
    want = inp["init"][0, 1:1 + c.M, :c.N].to(F64) + c.alpha * (inp["a"][0, :c.M].to(F64) @ inp["w"][0].to(F64).T)
    assert (ref.value[0] - want).abs().max() <= 1e-12 * want.abs().max()
    assert float(inp["init"][0, 1:1 + c.M, :c.N].abs().mean()) > 1                    # a non-zero running sum
    for name in ("v0-splitk2", "v0-splitk7"):
        cs = G.CASE[name]
        i2 = G.make(cs)
        r2 = G.reference(i2)
        w2 = i2["init"][0, 1:1 + cs.M, :cs.N].to(F64) + cs.alpha * torch.einsum("mk,nk->mn", i2["a"][0, :cs.M].to(F64), i2["w"][0].to(F64))
        assert (r2.value[0] - w2).abs().max() <= 1e-12 * w2.abs().max()
        assert cs.K // 64 % cs.splitk != 0                                       # splitk does not divide the k-tile count


def test_bmm_reference(runs):
    inp, ref, _ = runs["v26-bmm2"]
    c = inp["case"]
    assert inp["out"].stride(0) != c.M * c.N and inp["a"].stride(0) != c.M * c.K                  # batch strides that are not the dense ones
    for b in range(c.batch):
        want = c.alpha * torch.einsum("mk,nk->mn", inp["a"][b, :c.M].to(F64), inp["w"][b].to(F64))
        assert (ref.value[b] - want).abs().max() <= 1e-12 * want.abs().max()


def test_c_gemm_stays_under_the_order_independent_worst_case():
    assert max(c.K for c in G.CASES) == G.K_MAX
    assert G.C_GEMM <= (G.K_MAX + G.N_EPI_OPS) * 2.0 ** -24
    assert math.log2(G.C_GEMM) == int(math.log2(G.C_GEMM))


def test_float32_emulation_stays_within_c_gemm(runs):
    """The measurement behind C_GEMM: worst |float32 - float64| / magnitude over every case (printed with the case that sets it), the
    constant at least 4 x and at most 16 x that figure."""
    worst, plain = (0.0, None), (0.0, None)
    for name, (inp, r64, r32) in runs.items():
        if inp["case"].family == "exact":
            assert torch.equal(r32.value.to(F64), r64.value), name                # integers below 2^24: float32 is exact
            continue
        for v32, v64, mag in ((r32.value, r64.value, r64.mag), (r32.aux, r64.aux, r64.aux_mag)):
            if v64 is None:
                continue
            q = float(((v32.to(F64) - v64).abs() / (mag + G.F32_TINY / G.C_GEMM)).max())
            if q > worst[0]:
                worst = (q, name)
            if inp["case"].act is None and q > plain[0]:
                plain = (q, name)
    print(f"\nC_GEMM measurement: worst |f32 - f64| / magnitude = {worst[0]:.3e} = 2^{math.log2(worst[0]):.1f} on {worst[1]}; "
          f"without activation {plain[0]:.3e} on {plain[1]}; C_GEMM = 2^{math.log2(G.C_GEMM):.0f}")
    assert 4.0 * worst[0] <= G.C_GEMM < 16.0 * worst[0]


def _ratios(inp, r64, got):
    exp = G.expected(inp, r64)
    out = {}
    for key, (want, bound) in exp.items():
        alloc = inp["init"].clone() if key == "out" else torch.full_like(inp["aux_alloc"], G.SENTINEL)
        val = got.value if key == "out" else got.aux
        alloc[:, 1:-1, :inp["case"].N][:, got.out_rows] = val.to(alloc.dtype)     # what a kernel computing `got` would leave in memory
        out[key] = G.compare(alloc, want, bound)
    return out


def test_emulation_meets_every_bound(runs):
    per = {}
    for name, (inp, r64, r32) in runs.items():
        c = inp["case"]
        for key, (ratio, bad) in _ratios(inp, r64, r32).items():
            assert bad == 0, (name, key, ratio)
            k = (c.family, f"v{c.kernel}:{c.path}" + (":aux" if key == "aux" else ""))
            per[k] = max(per.get(k, 0.0), ratio)
    print()
    for (fam, path), r in sorted(per.items()):
        print(f"EMULATION {fam} {path}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("mutant", sorted(G.MUTANTS))
def test_mutant_leaves_the_bound_on_its_named_case(runs, mutant):
    inp, r64, _ = runs[G.MUTANTS[mutant]]
    got = G.reference(inp, torch.float32, mutant=mutant)
    res = _ratios(inp, r64, got)
    bad = sum(b for _, b in res.values())
    print(f"\nMUTANT {mutant} on {G.MUTANTS[mutant]}: {bad} elements outside, worst error / bound {max(r for r, _ in res.values()):.3g}")
    assert bad > 0


def test_exact_family_stays_below_two_to_the_24(runs):
    n = 0
    for name, (inp, r64, _) in runs.items():
        c = inp["case"]
        if c.family != "exact":
            continue
        n += 1
        assert c.act in (None, "mul_aux") and c.alpha in (1.0, 0.5, 2.0) and c.K <= 1536
        for t in (inp["a"], inp["w"], inp["bias"], inp["residual"], inp["aux_in"]):
            assert t is None or (float(t.abs().max()) <= 8 and torch.equal(t.float(), t.float().round()))
        assert inp["gate"] is None or float(inp["gate"].abs().max()) <= 4
        unit = min(1.0, c.alpha)                                                 # every intermediate is a multiple of it
        for s in r64.stages:
            assert float(s.max()) / unit < 2.0 ** 24, name
        assert torch.equal(r64.value, (r64.value / unit).round() * unit)
        # rows and columns are distinguishable: no two rows of A and no two rows of W agree
        assert len({tuple(r.tolist()) for r in inp["a"][0, :min(c.M, 256)].short()}) == min(c.M, 256) or c.M == 1
        assert len({tuple(r.tolist()) for r in inp["w"][0, :256].short()}) == min(c.N, 256)
    assert n >= 12


def test_cancelling_family_makes_the_float32_term_dominate(runs):
    n = 0
    for name, (inp, r64, _) in runs.items():
        if inp["case"].family != "cancelling":
            continue
        n += 1
        init = inp["init"][:, 1:-1, :inp["case"].N][:, r64.out_rows].to(F64)
        assert float(init.abs().max()) == 0 or not (inp["case"].splitk > 1)
        assert (r64.value.abs() <= 2.0 ** -6 * r64.mag).all(), name
        assert (G.C_GEMM * r64.mag >= G.U_BF16 * r64.value.abs()).all(), name     # the float32 term is the larger one everywhere
    assert n >= 3
