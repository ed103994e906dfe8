"""MI355X: every case of tests/conv_reference.py through the C entries of the 3x3 convolution family against the float64 reference of the
products and the whole epilogue, element by element, over the WHOLE allocation around each output (8 pixel rows of sentinel before and after
y, pair_out and gn_partial; the unwritten third of pair rows).  Operands sit inside NaN-filled allocations with the thirds a form does not
read NaN as well, so a read outside the pieces poisons the result.  The `exact` family is compared without a tolerance.  One
`PATH <form>:<tile>:<epilogue>: worst error / bound` line per path is printed at the end (pytest -s)."""
import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

_PATHS = {}


@pytest.fixture(scope="module", autouse=True)
def path_lines():
    yield
    print()
    for name, (r, n) in sorted(_PATHS.items()):
        print(f"PATH {name}: worst error / bound {r:.3f} over {n} cases")


def _launch(c, inp):
    """The entry of the case's form, called as adv_grpo_amd.ops does, but with outputs that are views inside guarded allocations."""
    from adv_grpo_amd import _lib, ops
    lib = _lib.load()
    p = _lib.ptr
    x, w = inp["x"], inp["w"]
    zp = ops.zero_page(x.device).data_ptr()
    geo = (c.B, c.H, c.W, x.shape[1], c.Cout)
    act, st = ops.ACT[c.act], _lib.stream_ptr()
    if c.form == "bf16":
        rc = lib.advgrpo_conv3x3_nhwc(p(x), p(w), p(inp["out"]), _lib.dtype_code(inp["out"].dtype), *geo, int(c.ups), p(inp["bias"]), act,
                                      p(inp["residual"]), zp, st)
    elif c.form == "x3":
        rc = lib.advgrpo_conv3x3_nhwc_x3(p(x), p(w), p(inp["out"]), *geo, int(c.ups), p(inp["bias"]), act, p(inp["residual"]), zp, st)
    elif c.form == "s2":
        rc = lib.advgrpo_conv3x3_s2_nhwc_x3(p(x), p(w), p(inp["out"]), *geo, p(inp["bias"]), zp, st)
    elif c.pair is not None:
        fn = {"f16x2": lib.advgrpo_conv3x3_nhwc_f16x2_pair, "f16x1": lib.advgrpo_conv3x3_nhwc_f16x1_pair}[c.form]
        rc = fn(p(x), p(w), p(inp["pair_out"]), float(c.pair), *geo, int(c.ups), p(inp["bias"]), act, p(inp["residual"]), zp, float(c.alpha), st)
    else:
        fn = {"f16x2": lib.advgrpo_conv3x3_nhwc_f16x2, "f16x1": lib.advgrpo_conv3x3_nhwc_f16x1, "bf16x2": lib.advgrpo_conv3x3_nhwc_bf16x2}[c.form]
        rc = fn(p(x), p(w), p(inp["out"]), *geo, int(c.ups), p(inp["bias"]), act, p(inp["residual"]), zp, float(c.alpha), p(inp["gn"]), st)
    _lib.check(rc)
    torch.cuda.synchronize()


def _got(inp):
    return {k: inp[k + "_alloc"] for k in ("out", "pair", "gn") if inp[k + "_alloc"] is not None}


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_conv_case_matches_float64_reference(name):
    from adv_grpo_amd import _lib
    c = R.CASE[name]
    assert R.route(c) == (c.tile, c.epi)
    if c.tile in ("v5", "v18"):
        K = 9 * c.C * (3 if c.form == "x3" else 1)
        assert "v%d" % _lib.load().advgrpo_gemm_variant(c.B * c.H * c.W, c.Cout, K, 1, 1) == c.tile
    inp = R.make(c, "cuda")
    _launch(c, inp)
    ref = R.reference(inp)
    label = f"{c.form}:{c.tile}:{c.epi}"
    worst = 0.0
    for key, (ratio, bad) in R.verify(inp, ref, _got(inp)).items():
        print(f"{c.name} [{label}] {key}: worst error / bound {ratio:.3f}, {bad} elements outside")
        assert bad == 0, (c.name, key, ratio)
        worst = max(worst, ratio)
    if c.family == "exact" and c.pair is None:
        a = inp["out_alloc"]
        want = torch.full_like(a, R.SENTINEL)
        want[R.GUARD:-R.GUARD] = ref.value.to(a.dtype)                            # (exact values: the cast is the round-to-nearest-even store)
        assert torch.equal(a, want)
    label += "" if c.family != "exact" else " (exact)"
    r, n = _PATHS.get(label, (0.0, 0))
    _PATHS[label] = (max(r, worst), n + 1)


def test_image_of_a_batch_gives_the_bits_and_sums_of_the_image_alone():
    """f16x2 with block sums over a batch of three: image 1 (pixels 128..255, across the tile boundary at 192) run alone leaves the same
    output bits and the same block sums."""
    c3 = R.CASE["f16x2-x3-gn-gn-b3"]
    inp = R.make(c3, "cuda")
    _launch(c3, inp)
    hw, C = c3.H * c3.W, c3.C
    c1 = c3._replace(name=c3.name + "-image1", B=1)
    one = R.make(c1, "cuda")
    one["x"].copy_(inp["x"][hw:2 * hw])
    one["w"].copy_(inp["w"])
    one["bias"].copy_(inp["bias"])
    _launch(c1, one)
    assert bool((one["out"] != R.SENTINEL).all())
    assert torch.equal(one["out"], inp["out"][hw:2 * hw])
    nb = hw // R.GN_ROWS
    assert torch.equal(one["gn"], inp["gn"][nb:2 * nb])
    for t in (one["out_alloc"], one["gn_alloc"]):
        assert bool((t[:R.GUARD] == R.SENTINEL).all()) and bool((t[-R.GUARD:] == R.SENTINEL).all())
    assert C == 128


def test_split_kernels_produce_the_bits_of_the_torch_construction():
    """ops.split_x3 (orders 0, 1, 2; with bias) and ops.split_f16x2 (with prescale; with bias) against split_bf16 / split_f16 of the helper,
    in every third they write."""
    from adv_grpo_amd import ops
    g = torch.Generator().manual_seed(7)
    K = 136
    x = (torch.randn(37, K, generator=g) * torch.logspace(-3, 3, 37)[:, None]).cuda()
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9])      # zeros, two ties of the bf16 rounding (to even: up, down)
    bias = torch.randn(K, generator=g).cuda()
    bits = lambda t: t.contiguous().view(torch.int16)                              # noqa: E731
    for b in (None, bias):
        v = x if b is None else x + b
        hi, lo = R.split_bf16(v)
        for order, thirds in ((0, (hi, hi, lo)), (1, (hi, lo, hi)), (2, (hi, None, lo))):
            out = ops.split_x3(x, order=order, bias=b)
            assert out.dtype == torch.bfloat16 and tuple(out.shape) == (37, 3 * K)
            for i, t in enumerate(thirds):
                if t is not None:
                    assert torch.equal(bits(out[:, i * K:(i + 1) * K]), bits(t)), (order, i, b is not None)
        for prescale in (1.0, 2.0 ** -4, 8.0):
            out = ops.split_f16x2(x, prescale=prescale, bias=b).view(torch.float16)
            hi, lo = R.split_f16(v, prescale)
            assert torch.equal(bits(out[:, :K]), bits(hi)) and torch.equal(bits(out[:, 2 * K:]), bits(lo)), (prescale, b is not None)
    big = torch.tensor([[1e6, -1e6, 65504.0, 70000.0] * 2]).cuda()               # saturation at the fp16 range
    out = ops.split_f16x2(big).view(torch.float16)
    hi, lo = R.split_f16(big)
    assert torch.equal(bits(out[:, :8]), bits(hi)) and torch.equal(bits(out[:, 16:]), bits(lo)) and not bool(out[:, :8].isinf().any())
