"""CPU: the float64 reference of tests/conv_reference.py against F.conv2d (with F.interpolate and F.pad for the fused forms), the kernel and
epilogue branch every case declares against the dispatcher's conditions, the float32 constant C_CONV, the emulation against every bound,
every mutant on its named case, the proof that the `exact` family is exact, and the pair / block-sum references.  Every narrow input of
tests/test_gpu_conv_parity.py is constructed here once; the cases around the wide tile's threshold (about 100k and 200k pixels) are routed
but not evaluated."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_reference as R

F64 = torch.float64
NARROW = tuple(c for c in R.CASES if not R.is_large(c))
WIDE = tuple(c for c in R.CASES if c.tile == "wide")


@pytest.fixture(scope="module")
def runs():
    """name -> (inp, float64 Result, float32 Result) of every narrow case; the references are computed once."""
    out = {}
    for c in NARROW:
        inp = R.make(c)
        out[c.name] = (inp, R.reference(inp, F64), R.reference(inp, torch.float32))
    return out


def test_case_list_reaches_every_cell_it_declares():
    assert len(R.CASES) <= 200 and len(WIDE) <= 5 and sum(R.is_large(c) for c in R.CASES) == len(WIDE) + 1
    for c in R.CASES:
        assert R.route(c) == (c.tile, c.epi), (c.name, R.route(c))
        assert c.C in R.CHANNELS and R.k_eff(c) <= R.K_EFF_MAX
        assert not c.ups or (c.H % 2 == 0 and c.W % 2 == 0)
        assert not c.gn or (c.H * c.W) % R.GN_ROWS == 0
    assert max(R.k_eff(c) for c in NARROW) == R.K_EFF_MAX
    cells = [(f, t) for f, t, _ in R.CELLS]
    exact = [c for c in R.CASES if c.family == "exact" and not R.is_large(c)]
    # (form x tile x geometry): every stride-1 cell meets every class, plain and with the fused upsample, and the odd-width upsample
    for f, t in cells:
        mine = {c.name.split("-", 3)[3] for c in exact if (c.form, c.tile) == (f, t) and c.pair is None and not c.gn}
        assert mine == {g + u + "-exact" for g in R.GEOMETRIES for u in ("", "-ups")} | {"upsodd-exact"}, (f, t, mine)
        assert {c.C for c in exact if (c.form, c.tile) == (f, t)} == set(R.CHANNELS)
    s2 = {(c.B, c.H, c.W) for c in exact if c.form == "s2"}
    assert s2 == set(R.S2_GEOMETRIES.values()) and {R.in_shape(c) for c in exact if c.form == "s2"} == {(1, 2, 2), (2, 14, 2), (3, 20, 26), (1, 24, 32)}
    geo = {(c.B, c.H, c.W) for c in exact if c.form != "s2"}
    assert set(R.GEOMETRIES.values()) | {R.UPS_ODD} <= geo
    # the dedicated kernel's column tiles: full, ragged with the vec epilogue, ragged with the scalar epilogue, two and three tiles
    for f in ("x3", "f16x2", "bf16x2", "f16x1"):
        assert {c.Cout for c in R.CASES if (c.form, c.tile) == (f, "x3")} >= {128, 132, 130, 256, 384}, f
    assert {c.Cout for c in R.CASES if c.form == "bf16"} >= {3, 64, 96} and {c.Cout for c in R.CASES if c.form == "x3" and c.tile != "x3"} == {3, 64, 96}
    assert {(c.Cout, c.out_f32) for c in R.CASES if c.form == "bf16" and c.family != "exact"} >= {(n, o) for n in (3, 64, 96) for o in (False, True)}
    # (form x tile x epilogue) through the random family
    rnd = [c for c in R.CASES if c.family != "exact"]
    ops = lambda f, t: {c.op for c in rnd if (c.form, c.tile) == (f, t)}       # noqa: E731
    common = {"none", "bias", "silu", "gelu_tanh", "bias_res"}
    assert ops("bf16", "v5") >= common and ops("bf16", "v18") >= common | {"full"}
    assert ops("x3", "v5") | ops("x3", "v18") >= common and ops("x3", "x3") >= common | {"full"}
    for f in ("f16x2", "bf16x2", "f16x1"):
        assert ops(f, "x3") >= common | {"full", "alpha", "gn"}, f
    assert "pair" in ops("f16x2", "x3") and "pair" in ops("f16x1", "x3")
    assert {c.op for c in rnd if c.form == "s2"} == {"none", "bias"}
    # both branches of gemm_epilogue_f32io on every instantiation that can take them; the three of gemm_epilogue on the generic tiles
    for f in ("x3", "f16x2", "bf16x2", "f16x1"):
        assert {c.epi for c in rnd if (c.form, c.tile) == (f, "x3")} >= {"vec", "scalar"}, f
    assert {c.epi for c in rnd if c.form == "bf16"} == {"rows", "frag_vec", "frag_scalar"}
    # the wide tile: every one-piece form, pair output on both pair entries, block sums, the fused upsample, bias + activation + residual,
    # a ragged last pixel tile -- and a narrow case with the same C for each of them
    assert {c.form for c in WIDE} == {"f16x2", "bf16x2", "f16x1"} and {c.Cout for c in WIDE} == {256, 512}
    assert {(c.form, c.epi) for c in WIDE} >= {("f16x2", "gn"), ("f16x2", "pair"), ("f16x1", "pair"), ("bf16x2", "vec")}
    assert any(c.ups for c in WIDE) and any(c.op == "full" for c in WIDE) and all((c.B * c.H * c.W) % R.X3_BM for c in WIDE)
    for c in WIDE:
        assert any((n.form, n.C, n.epi) == (c.form, c.C, c.epi) for n in NARROW), c.name
    # exactly at the threshold, and one pixel tile short of it
    tiles = lambda c: -(-c.B * c.H * c.W // R.X3_BM) * (c.Cout // R.WIDE_BN)      # noqa: E731
    assert min(tiles(c) for c in WIDE) == R.WIDE_MIN_TILES
    assert [tiles(c) for c in R.CASES if R.is_large(c) and c.tile == "x3"] == [R.WIDE_MIN_TILES - 1]
    # every instantiation conv3x3_x3_launch and conv3x3_f16x2_launch dispatch in the product build: three products, strided, and the three
    # one-piece forms on the narrow and the wide tile
    assert {(c.form, c.tile) for c in R.CASES if c.tile in ("x3", "wide")} == {("x3", "x3"), ("s2", "x3")} | {(f, t) for f in ("f16x2", "bf16x2", "f16x1")
                                                                                                                  for t in ("x3", "wide")}
    assert set(R.MUTANTS.values()) <= {c.name for c in NARROW}


def test_generic_tile_matches_gemm_variant_of_the_library_source():
    """route()'s generic tiles are gemm.hip's gemm_variant(conv = 1) as gemm_reference re-derives the Linear ones: Cout <= 64 -> 5, else 18
    (the GPU suite confirms them against advgrpo_gemm_variant(..., conv=1))."""
    for c in R.CASES:
        if c.tile in ("v5", "v18"):
            assert c.tile == "v%d" % R.conv_variant(c.Cout) and (c.Cout <= 64) == (c.tile == "v5")
        else:
            assert c.Cout >= 128


def _conv2d(c, x, w):
    """F.conv2d form of one piece product: x [P, C], w [Cout, 9, C] float64 -> [M, Cout]."""
    B, Hin, Win = R.in_shape(c)
    xi = x.view(B, Hin, Win, c.C).permute(0, 3, 1, 2)
    wt = w.view(c.Cout, 3, 3, c.C).permute(0, 3, 1, 2)
    if c.form == "s2":
        y = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, stride=2)
    else:
        if c.ups:
            xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
        y = F.conv2d(xi, wt, padding=1)
    assert tuple(y.shape) == (c.B, c.Cout, c.H, c.W)
    return y.permute(0, 2, 3, 1).reshape(-1, c.Cout)


def test_reference_matches_functional_conv2d(runs):
    seen = set()
    for name, (inp, r64, _) in runs.items():
        c = inp["case"]
        key = (c.form, c.B, c.H, c.W, c.ups)
        if c.family != "exact" and key in seen:
            continue
        seen.add(key)
        acc = sum(_conv2d(c, xp.to(F64), wp.to(F64)) for xp, wp in R._products(inp))
        got, amag = R.accumulate(inp)
        scale = max(1.0, float(acc.abs().max()))
        assert (got - acc).abs().max() <= 1e-12 * scale, name
        mag = sum(_conv2d(c, xp.to(F64).abs(), wp.to(F64).abs()) for xp, wp in R._products(inp))
        assert (amag - mag).abs().max() <= 1e-12 * max(1.0, float(mag.abs().max())), name
        assert (r64.mag >= r64.value.abs() * (1 - 1e-12)).all(), name
    assert {k[0] for k in seen} == set(R.FORMS)


def test_reference_epilogue_order():
    for name in ("f16x2-x3-vec-alpha", "bf16x2-x3-scalar-full", "bf16-v18-rows-gelu_tanh", "x3-v18-vec-bias_res"):
        inp = R.make(R.CASE[name])
        c = inp["case"]
        acc, _ = R.accumulate(inp)
        y = c.alpha * acc + inp["bias"].to(F64)
        if c.act == "silu":
            y = F.silu(y)
        elif c.act == "gelu_tanh":
            y = F.gelu(y, approximate="tanh")
        if c.residual:
            y = y + inp["residual"].to(F64)
        ref = R.reference(inp)
        assert (ref.value - y).abs().max() <= 1e-12 * max(1.0, float(y.abs().max())), name


def test_operands_hold_nan_wherever_the_form_does_not_read():
    for name in ("x3-x3-vec-none", "x3-v18-vec-none", "f16x2-x3-vec-none", "f16x1-x3-vec-none", "bf16x2-x3-vec-none", "bf16-v5-rows-none", "s2-x3-vec-none-128"):
        inp = R.make(R.CASE[name])
        c = inp["case"]
        C = c.C
        xa, wa = inp["x_alloc"], inp["w_alloc"]
        assert bool(xa[:R.PAD].isnan().all()) and bool(xa[-R.PAD:].isnan().all()) and bool(wa[:R.PAD].isnan().all()) and bool(wa[-R.PAD:].isnan().all())
        assert not bool(inp["w"].isnan().any())
        if c.form == "bf16":
            assert not bool(inp["x"].isnan().any())
            continue
        mid, lo = inp["x"][:, C:2 * C], inp["x"][:, 2 * C:]
        assert not bool(inp["xh"].isnan().any())
        assert bool(mid.isnan().all()) == (c.tile == "x3")                     # the tripled K axis of the generic tiles reads [hi | hi | lo]
        assert bool(lo.isnan().all()) == (c.form == "f16x1")
        if c.tile != "x3":
            assert torch.equal(mid, inp["xh"])
        if c.form in ("x3", "s2"):                                               # per tap [hi | lo | hi]
            assert torch.equal(inp["w"][:, :, 2 * C:], inp["wh"]) and inp["w"].shape[2] == 3 * C
        # the random family's pieces are the split of one float32 value
    x = torch.randn(1000)
    hi, lo = R.split_bf16(x)
    assert ((hi.double() + lo.double()) - x.double()).abs().max() <= 2.0 ** -16 * x.abs().max()
    hi, lo = R.split_f16(x, 0.25)
    assert ((hi.double() + lo.double()) / 0.25 - x.double()).abs().max() <= R.U_PAIR * x.abs().max()


def test_c_conv_stays_under_the_order_independent_worst_case():
    assert R.C_CONV <= (R.K_EFF_MAX + R.N_EPI_OPS) * 2.0 ** -24
    assert math.log2(R.C_CONV) == int(math.log2(R.C_CONV))


def test_float32_emulation_stays_within_c_conv(runs):
    """The measurement behind C_CONV: worst |float32 - float64| / magnitude over every narrow case (printed with the case that sets it), the
    constant at least 4 x and at most 8 x that figure."""
    worst, plain = (0.0, None), (0.0, None)
    for name, (inp, r64, r32) in runs.items():
        c = inp["case"]
        if c.family == "exact":
            continue
        q = float(((r32.value.to(F64) - r64.value).abs() / (r64.mag + R.F32_TINY / R.C_CONV)).max())
        if q > worst[0]:
            worst = (q, name)
        if c.act is None and q > plain[0]:
            plain = (q, name)
    print(f"\nC_CONV measurement: worst |f32 - f64| / magnitude = {worst[0]:.3e} = 2^{math.log2(worst[0]):.1f} on {worst[1]}; "
          f"without activation {plain[0]:.3e} on {plain[1]}; C_CONV = 2^{math.log2(R.C_CONV):.0f}")
    assert 4.0 * worst[0] <= R.C_CONV < 8.0 * worst[0]


def test_emulation_meets_every_bound(runs):
    per = {}
    for name, (inp, r64, r32) in runs.items():
        c = inp["case"]
        for key, (ratio, bad) in R.verify(inp, r64, R.store(inp, r32)).items():
            assert bad == 0, (name, key, ratio)
            k = (c.family, f"{c.form}:{c.tile}:{c.epi}" + ("" if key in ("out", "pair") else ":" + key))
            per[k] = max(per.get(k, 0.0), ratio)
    print()
    for (fam, path), r in sorted(per.items()):
        print(f"EMULATION {fam} {path}: worst error / bound {r:.3f}")


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_mutant_leaves_the_bound_on_its_named_case(runs, mutant):
    inp, r64, _ = runs[R.MUTANTS[mutant]]
    got = R.reference(inp, torch.float32, mutant=mutant)
    res = R.verify(inp, r64, R.store(inp, got, mutant=mutant))
    bad = sum(b for _, b in res.values())
    print(f"\nMUTANT {mutant} on {R.MUTANTS[mutant]}: {bad} elements outside, worst error / bound {max(r for r, _ in res.values()):.3g}")
    assert bad > 0


def test_exact_family_is_exact(runs):
    """Every piece is an integer of {-1, 0, 1} times 1 (hi) or 2^-12 (lo), bias and residual integers up to 4: every partial sum is a multiple of
    2^-12 (2^-24 for nothing: no lo x lo product exists in any form) below 2^11, i.e. representable in float32's 24 bits -- checked on the
    magnitudes, and by evaluating float32 under two summation orders against float64, bit for bit."""
    n = 0
    for name, (inp, r64, r32) in runs.items():
        c = inp["case"]
        if c.family != "exact":
            continue
        n += 1
        assert c.act is None and c.alpha == 1.0
        for t, unit in ((inp["xh"], 1.0), (inp["wh"], 1.0), (inp["xl"], R.LO_UNIT), (inp["wl"], R.LO_UNIT), (inp["bias"], 1.0), (inp["residual"], 1.0)):
            if t is not None:
                q = t.to(F64) / unit
                assert torch.equal(q, q.round()) and float(q.abs().max()) <= (4 if unit == 1.0 and t is not inp["xh"] and t is not inp["wh"] else 1)
        for s in r64.stages:
            assert float(s.max()) / R.LO_UNIT < 2.0 ** 24, name
        assert torch.equal(r64.value, (r64.value / R.LO_UNIT).round() * R.LO_UNIT)
        assert torch.equal(r32.value.to(F64), r64.value), name
        assert torch.equal(R.reference(inp, torch.float32, order=1).value.to(F64), r64.value), name
        if c.form != "bf16" and c.form != "f16x1":
            assert float(inp["xl"].abs().max()) == R.LO_UNIT                    # the lo pieces take part
        if min(c.B * c.H * c.W, c.Cout) > 1:                                     # rows and columns are distinguishable
            assert len({tuple(r.tolist()) for r in inp["wh"].reshape(c.Cout, -1)[:256].to(torch.int16)}) == min(c.Cout, 256)
    assert n >= 100


def test_pair_and_block_sum_references(runs):
    # the pair of the reference's value decodes to it within 2^-22, its bits are split_f16's, and the saturation is split8_f16's
    inp, r64, r32 = runs["f16x2-x3-pair-pair"]
    c = inp["case"]
    got = R.store(inp, r32)["pair"]
    N = c.Cout
    hi, lo = got[R.GUARD:-R.GUARD, :N], got[R.GUARD:-R.GUARD, 2 * N:]
    assert ((hi.double() + lo.double()) / c.pair - r32.value.double()).abs().max() <= R.U_PAIR * r32.value.abs().max()
    assert bool((got[R.GUARD:-R.GUARD, N:2 * N] == R.SENTINEL).all()) and bool((got[:R.GUARD] == R.SENTINEL).all())
    assert torch.equal(hi, (r32.value * c.pair).to(torch.float16))
    h, l = R.pair_of(torch.tensor([1e6, -1e6, 3.0]), 1.0)
    assert h.tolist() == [65504.0, -65504.0, 3.0] and l.tolist() == [0.0, 0.0, 0.0]
    # a value written into the unwritten third, or a guard row, is counted
    for r, col in ((R.GUARD + 3, N + 5), (2, 7), (got.shape[0] - 1, 3 * N - 1)):
        dirty = got.clone()
        dirty[r, col] = 1.0
        assert R.verify(inp, r64, {"pair": dirty})["pair"][1] == 1
    # block sums: an independent loop over blocks, and the bound's two parts
    inp, r64, r32 = runs["f16x2-x3-gn-gn"]
    got = R.store(inp, r32)
    y = got["out"][R.GUARD:-R.GUARD].double()
    sums = R.gn_sums(y)
    for blk, ch in ((0, 0), (5, 17), (y.shape[0] // 16 - 1, inp["case"].Cout // 4 - 1)):
        tile = y[blk * 16:(blk + 1) * 16, ch * 4:(ch + 1) * 4]
        assert abs(float(sums[blk, 2 * ch] - tile.sum())) <= 1e-12 and abs(float(sums[blk, 2 * ch + 1] - (tile * tile).sum())) <= 1e-12
    assert R.verify(inp, r64, got)["gn"][1] == 0
    dirty = {k: v.clone() for k, v in got.items()}
    dirty["gn"][R.GUARD + 2, 9] *= 1.0 + 2.0 ** -12                               # a sum off by more than the order-independent bound
    dirty["gn"][1, 0] = 0.0                                                      # a store in front of the first block
    assert R.verify(inp, r64, dirty)["gn"][1] == 2
    # a batch of three: image 1's pixels are whole blocks of 16, and straddle the 192-pixel tile boundary
    c3 = R.CASE["f16x2-x3-gn-gn-b3"]
    hw = c3.H * c3.W
    assert c3.B == 3 and hw % R.GN_ROWS == 0 and hw < R.X3_BM < 2 * hw
