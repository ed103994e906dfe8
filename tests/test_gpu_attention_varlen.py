"""MI355X: the head-dim-128 attention with per-sample lengths (advgrpo_attention_fwd_varlen / _bwd_varlen, advgrpo_mask_to_seq_lens).

Semantics under test: with lengths L[b], sample b is computed exactly as if it had been launched alone at sequence length L[b] -- so the
first criterion is bit equality (torch.equal) with the plain entries launched per sample, and the second the float64 parity bounds of
tests/attention_reference.py at the sample's own length.  Rows at or beyond L[b] are never read (they hold NaN here) and come back as zeros.
"""
import pytest
import torch

import attention_reference as A
import attention_varlen_cases as V

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                  # sentinel elements on both sides of every output buffer
NAN = float("nan")


def _guarded(shape, dtype, sentinel):
    """A contiguous tensor of `shape` inside a larger allocation filled with `sentinel` (the view itself included): (view, whole)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n].view(*shape), whole


def _guards_intact(whole, sentinel, what):
    assert bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all()), f"{what}: guard elements overwritten"


def _lens_t(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _padded_with_nan(packed, lens):
    x = packed.to(DEV).clone()
    for b, L in enumerate(lens):
        x[b, L:] = NAN
    return x


def _views(x, HD):
    return x[:, :, :HD], x[:, :, HD:2 * HD], x[:, :, 2 * HD:]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _run_fwd_varlen(case, x, lens_t, want_lse=True):
    from adv_grpo_amd import ops
    B, S, Hh = case["B"], case["S"], case["H"]
    q, k, v = _views(x, Hh * V.HD)
    out, out_all = _guarded((B, S, Hh * V.HD), torch.bfloat16, 7.0)
    lse, lse_all = _guarded((B, Hh, S), torch.float32, 7.0)
    ops.attention(q, k, v, Hh, scale=case["scale"], out=out, lse=lse if want_lse else None, seq_lens=lens_t)
    torch.cuda.synchronize()
    _guards_intact(out_all, 7.0, case["name"] + " o")
    _guards_intact(lse_all, 7.0, case["name"] + " lse")
    return out, lse


def _run_fwd_alone(case, x, b, L):
    """The parent's entry on sample b alone at S = L."""
    from adv_grpo_amd import ops
    Hh = case["H"]
    q, k, v = _views(x[b:b + 1, :L], Hh * V.HD)
    lse = torch.empty(1, Hh, L, dtype=torch.float32, device=DEV)
    out = ops.attention(q, k, v, Hh, scale=case["scale"], lse=lse)
    return out, lse


def _within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    over = err > bound
    assert not bool(over.any()), f"{what}: {int(over.sum())} elements over the bound, worst ratio {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    return float((err / bound.clamp_min(1e-300)).max())


def _check_forward(case, expect_fallback):
    from adv_grpo_amd import ops
    kw, packed, refs = V.forward_case(case)
    lens = case["lens"]
    x = _padded_with_nan(packed, lens)
    x_before = x.clone()
    ops.attention_fallback_count(reset=True)
    out, lse = _run_fwd_varlen(case, x, _lens_t(lens))
    fallbacks = ops.attention_fallback_count(reset=True)
    assert _same_bits(x, x_before), "inputs modified"
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()), f"{case['name']}: padding was read (non-finite output)"
    worst = 0.0
    for b, L in enumerate(lens):
        o1, l1 = _run_fwd_alone(case, x, b, L)
        assert torch.equal(out[b, :L], o1[0]), f"{case['name']} sample {b} (L = {L}): o differs from the plain entry at S = L"
        assert torch.equal(lse[b, :, :L], l1[0]), f"{case['name']} sample {b} (L = {L}): lse differs from the plain entry at S = L"
        assert not bool(out[b, L:].any()) and not bool(lse[b, :, L:].any()), f"{case['name']} sample {b}: rows >= L are not zero"
        bo, bl = A.forward_bounds(refs[b], kw["H"])
        worst = max(worst, _within(out[b:b + 1, :L], refs[b]["o"], bo, f"{case['name']} sample {b} out"))
        worst = max(worst, _within(lse[b:b + 1, :, :L], refs[b]["lse2"], bl, f"{case['name']} sample {b} lse2"))
    print(f"VARLEN FWD {case['name']}: worst error / bound {worst:.3f}, fallbacks {fallbacks}")
    if expect_fallback:
        assert fallbacks > 0, "the fallback was not taken"
    else:
        assert fallbacks == 0, f"{fallbacks} workgroups took the fallback"
    ops.attention_fallback_count(reset=True)          # (the per-sample launches above counted too)


@pytest.mark.parametrize("case", V.FWD_CASES, ids=lambda c: c["name"])
def test_forward_equals_each_sample_launched_alone(case):
    """Bit identity with the plain entry per sample, zero rows beyond L, NaN padding never read, sentinel guards intact, float64 parity
    inside forward_bounds with no element left out."""
    _check_forward(case, expect_fallback=False)


def test_forward_fallback_with_ragged_lengths():
    """The running-maximum fallback is taken (the shared counter rises) and bit identity with the per-sample launches still holds."""
    _check_forward(V.FALLBACK_CASE, expect_fallback=True)


def test_forward_output_does_not_depend_on_the_lse_argument():
    case = V.FWD_CASES[-1]
    _, packed, _ = V.forward_case(case)
    x = _padded_with_nan(packed, case["lens"])
    a, _ = _run_fwd_varlen(case, x, _lens_t(case["lens"]), want_lse=True)
    b, _ = _run_fwd_varlen(case, x, _lens_t(case["lens"]), want_lse=False)
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", [V.FWD_CASES[0], V.FWD_CASES[-1]], ids=lambda c: c["name"])
def test_forward_full_lengths_equal_the_plain_entry(case):
    from adv_grpo_amd import ops
    _, packed, _ = V.forward_case(case)
    x = packed.to(DEV)
    B, S, Hh = case["B"], case["S"], case["H"]
    out, lse = _run_fwd_varlen(case, x, _lens_t([S] * B))
    q, k, v = _views(x, Hh * V.HD)
    lse0 = torch.empty(B, Hh, S, dtype=torch.float32, device=DEV)
    out0 = ops.attention(q, k, v, Hh, scale=case["scale"], lse=lse0)
    assert torch.equal(out, out0) and torch.equal(lse, lse0)


def test_forward_out_of_range_lengths_are_clamped():
    """0 behaves as 1 and S + 7 as S (the clamp the header documents)."""
    case = V.FWD_CASES[0]
    _, packed, _ = V.forward_case(case)
    x = packed.to(DEV)
    S = case["S"]
    got_o, got_l = _run_fwd_varlen(case, x, _lens_t([0, S + 7, -5, 2 ** 31 - 1]))
    ref_o, ref_l = _run_fwd_varlen(case, x, _lens_t([1, S, 1, S]))
    assert torch.equal(got_o, ref_o) and torch.equal(got_l, ref_l)


def test_graph_replay_reads_the_lengths_at_run_time():
    """One captured single-stream graph, replayed after seq_lens was overwritten on the device: the second replay matches the new lengths."""
    from adv_grpo_amd import ops
    case = V.FWD_CASES[-1]
    _, packed, _ = V.forward_case(case)
    x = packed.to(DEV)
    B, S, Hh = case["B"], case["S"], case["H"]
    q, k, v = _views(x, Hh * V.HD)
    first, second = list(case["lens"]), list(reversed(case["lens"]))
    assert first != second
    lens_t = _lens_t(first)
    out = torch.empty(B, S, Hh * V.HD, dtype=torch.bfloat16, device=DEV)
    lse = torch.empty(B, Hh, S, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention(q, k, v, Hh, scale=case["scale"], out=out, lse=lse, seq_lens=lens_t)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention(q, k, v, Hh, scale=case["scale"], out=out, lse=lse, seq_lens=lens_t)
    for lens in (first, second):
        lens_t.copy_(_lens_t(lens))
        out.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        want_o, want_l = _run_fwd_varlen(case, x, _lens_t(lens))
        assert torch.equal(out, want_o) and torch.equal(lse, want_l), f"replay with lengths {lens}"


# ---------------------------------------------------------------------------------------------------------------------- backward
def _run_bwd_varlen(case, x, d_o, o, lse, lens_t):
    from adv_grpo_amd import ops
    B, S, Hh = case["B"], case["S"], case["H"]
    HD = Hh * V.HD
    q, k, v = _views(x, HD)
    grads, grads_all = _guarded((B, S, 3 * HD), torch.bfloat16, 7.0)
    dq, dk, dv = _views(grads, HD)
    ops.attention_bwd(q, k, v, o, d_o, lse, Hh, dq, dk, dv, scale=case["scale"], seq_lens=lens_t)
    torch.cuda.synchronize()
    _guards_intact(grads_all, 7.0, case["name"] + " dq|dk|dv")
    return dq, dk, dv


@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c["name"])
def test_backward_equals_each_sample_launched_alone(case):
    """dq / dk / dv: bit identity with advgrpo_attention_bwd per sample at S = L, zero rows beyond L, NaN in the padding rows of q, k, v, o
    and d_o never read, guards intact, float64 parity inside backward_bounds."""
    from adv_grpo_amd import ops
    kw, packed, d_o_c, o_c, lse_c, refs = V.backward_case(case)
    lens, Hh = case["lens"], case["H"]
    HD = Hh * V.HD
    x = _padded_with_nan(packed, lens)
    d_o, o, lse = d_o_c.to(DEV).clone(), o_c.to(DEV).clone(), lse_c.to(DEV)
    for b, L in enumerate(lens):
        d_o[b, L:] = NAN
        o[b, L:] = NAN
    before = [t.clone() for t in (x, d_o, o, lse)]
    dq, dk, dv = _run_bwd_varlen(case, x, d_o, o, lse, _lens_t(lens))
    for t, t0, name in zip((x, d_o, o), before, ("q|k|v", "d_o", "o")):
        assert _same_bits(t, t0), f"{name} modified"
    assert torch.equal(lse, before[3])
    worst = 0.0
    for b, L in enumerate(lens):
        q1, k1, v1 = _views(x[b:b + 1, :L], HD)
        g1 = torch.empty(1, L, 3 * HD, dtype=torch.bfloat16, device=DEV)
        dq1, dk1, dv1 = _views(g1, HD)
        ops.attention_bwd(q1, k1, v1, o[b:b + 1, :L], d_o[b:b + 1, :L], lse[b:b + 1, :, :L].contiguous(), Hh, dq1, dk1, dv1, scale=case["scale"])
        bounds = A.backward_bounds(refs[b])
        for name, got, alone in (("dq", dq, dq1), ("dk", dk, dk1), ("dv", dv, dv1)):
            assert bool(torch.isfinite(got[b]).all()), f"{case['name']} sample {b} {name}: padding was read (non-finite)"
            assert torch.equal(got[b, :L], alone[0]), f"{case['name']} sample {b} (L = {L}): {name} differs from the plain entry at S = L"
            assert not bool(got[b, L:].any()), f"{case['name']} sample {b}: {name} rows >= L are not zero"
            worst = max(worst, _within(got[b:b + 1, :L], refs[b][name], bounds[name], f"{case['name']} sample {b} {name}"))
    print(f"VARLEN BWD {case['name']}: worst error / bound {worst:.3f}")


def test_backward_full_and_out_of_range_lengths():
    """Every length = S: the bits of the plain entry.  Lengths 0 and S + 7: the documented clamp."""
    from adv_grpo_amd import ops
    case = V.BWD_CASES[2]
    kw, packed, d_o_c, o_c, lse_c, _ = V.backward_case(case)
    B, S, Hh = case["B"], case["S"], case["H"]
    HD = Hh * V.HD
    x, d_o = packed.to(DEV), d_o_c.to(DEV)
    # o / lse of the full-length problem from the forward kernel itself (any consistent pair serves a bit comparison)
    q, k, v = _views(x, HD)
    lse = torch.empty(B, Hh, S, dtype=torch.float32, device=DEV)
    o = ops.attention(q, k, v, Hh, scale=case["scale"], lse=lse)
    got = _run_bwd_varlen(case, x, d_o, o, lse, _lens_t([S] * B))
    g0 = torch.empty(B, S, 3 * HD, dtype=torch.bfloat16, device=DEV)
    ref = ops.attention_bwd(q, k, v, o, d_o, lse, Hh, *_views(g0, HD), scale=case["scale"])
    for a, b_ in zip(got, ref):
        assert torch.equal(a, b_)
    lens = [0, S + 7, 1, S][:B]
    a3 = _run_bwd_varlen(case, x, d_o, o, lse, _lens_t(lens))
    b3 = _run_bwd_varlen(case, x, d_o, o, lse, _lens_t([1, S, 1, S][:B]))
    for a, b_ in zip(a3, b3):
        assert torch.equal(a, b_)


# ------------------------------------------------------------------------------------------------------------- mask_to_seq_lens
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int32, torch.int64], ids=str)
def test_mask_to_seq_lens_matches_the_restatement(dtype):
    from adv_grpo_amd import ops
    rows = torch.tensor([r for r, _ in V.MASK_ROWS])
    wide = torch.zeros(3, 200, dtype=torch.int64)              # rows longer than a wave: a prefix of 130, a full row, a hole at 70
    wide[0, :130] = 1
    wide[1] = 1
    wide[2, :150] = 1
    wide[2, 70] = 0
    ops.bad_count(reset=True)
    for m, base in ((rows, 256), (wide, 4096)):
        m = m.to(dtype)
        want, want_bad = V.mask_to_seq_lens(m, base)
        got = ops.mask_to_seq_lens(m.to(DEV), base)
        assert got.dtype == torch.int32 and got.tolist() == want
        assert ops.bad_count(reset=True) == want_bad
    assert sum(bad for _, bad in V.MASK_ROWS) == V.mask_to_seq_lens(rows, 0)[1]
