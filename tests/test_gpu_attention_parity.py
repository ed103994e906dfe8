"""GPU: every attention forward kernel behind ops.attention / ops.attention_bias and both backward families against the float64
references of tests/attention_reference.py, element by element -- one wrong element fails, NaN fails -- with sentinel-filled rows and
columns around everything a kernel writes.

Bounds (derived in attention_reference.py from the arithmetic the kernel comments state, never fitted to a kernel's output):
  out  U |o| + 2 U A + C (1 + T) A          lse2  C (1 + T + |lse2|)
  dv   U |dv| + sum_i (U + C e_i) P |d_o|    dq / dk  U |.| + scale sum ((U + C e_i) |dS| + P delta) |k| / |q|
with U = 2^-8, A = w |v|, T the row's score magnitude in base-2 units, e_i = 1 + T_i + |lse2_i|, delta the float32 error of dP - D and
C = C_ATT measured in tests/test_attention_reference_host.py.  The backward gets o (bf16) and lse2 (f32) from the float64 forward reference,
not from the forward kernel, so the two directions are judged independently; one chained case per head dim runs kernel into kernel.
Each comparison prints its worst error / bound; each path prints its worst over its case list."""
import functools

import pytest
import torch

import attention_reference as A

pytestmark = pytest.mark.gpu

SENT16 = 0x5A5B           # sentinel bit patterns (a bf16 of ~2.4e16 / an f32 of ~1.5e16: nothing a kernel here computes)
SENT32 = 0x5A5B5C5D


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _sent_f32(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_sent(t):
    if t.dtype == torch.bfloat16:
        return bool((t.contiguous().view(torch.int16) == SENT16).all())
    return bool((t.contiguous().view(torch.int32) == SENT32).all())


def _within(got, ref, bound, what):
    """Elementwise |got - ref| <= bound, no element excluded; NaN fails.  Returns the worst error / bound."""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst |got - ref| / bound = {ratio:.3f} over {got.numel()} elements")
    bad = ~(err <= bound)
    if bad.any():
        i = bad.flatten().nonzero()[0].item()
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements out of bound; first at {idx}: got "
                             f"{got.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, bound {bound.flatten()[i].item():.3e}")
    return ratio


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(case, inputs, packed buffer, float64 forward reference) of a named case, computed once and shared (never modified)."""
    pool = [c for p in A.FWD_PATHS for c in A.FWD_CASES[p]] + [c for p in A.BWD_CASES for c in A.BWD_CASES[p]] + list(A.CHAINED.values())
    case = next(c for c in pool if c["name"] == name)
    kw, _, packed = A.make_inputs(case)
    return case, kw, packed, A.forward(**kw)


def _run_forward(case, kw, packed, with_lse=True):
    """The kernel's output as a [B, Sq, H hd] column slice of a sentinel-filled buffer with one spare row per batch and 8 spare columns
    (12 for the cases that must miss the 16-byte row alignment), lse2 in front of 64 sentinel floats.  Returns (out, lse or None) after
    checking every guard."""
    from adv_grpo_amd import ops
    q, k, v, bias = A.to_device(kw, packed, "cuda")
    B, Sq, HD = q.shape
    H = kw["H"]
    buf = _sent_bf16(B, Sq + 1, HD + (12 if case["pitch4"] else 8))
    out = buf[:, :Sq, :HD]
    assert (out.stride(1) % 8 == 4) == case["pitch4"] and out.stride(1) % 4 == 0
    n = B * H * Sq
    lbuf = _sent_f32(n + 64)
    lse = lbuf[:n].view(B, H, Sq) if (with_lse and bias is None) else None
    if bias is not None:
        res = ops.attention_bias(q, k, v, H, bias, scale=kw["scale"], causal=kw["causal"], out=out)
    else:
        res = ops.attention(q, k, v, H, scale=case["scale"], causal=kw["causal"], out=out, lse=lse)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert _is_sent(buf[:, Sq:]) and _is_sent(buf[:, :, HD:]), f"{case['name']}: the kernel wrote next to its output"
    assert _is_sent(lbuf[n:]) and (lse is not None or _is_sent(lbuf)), f"{case['name']}: the kernel wrote next to (or without) lse"
    return out, lse


# ----------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("path", A.FWD_PATHS)
def test_attention_forward_path_vs_float64(path):
    """One dispatch branch of attention_fwd per path (the table at attention_reference.FWD_CASES), every case of its list.  The two pipelined
    kernels must stay on their fast path for the diffuse / peaked / selector families and must take the running-maximum fallback for
    outside_window."""
    from adv_grpo_amd import ops
    worst = {"out": 0.0, "lse": 0.0}
    for case in A.FWD_CASES[path]:
        _, kw, packed, ref = _reference(case["name"])
        ops.attention_fallback_count(reset=True)
        out, lse = _run_forward(case, kw, packed)
        fallbacks = ops.attention_fallback_count(reset=True)
        bo, bl = A.forward_bounds(ref, kw["H"])
        worst["out"] = max(worst["out"], _within(out, ref["o"], bo, case["name"] + " out"))
        if lse is not None:
            worst["lse"] = max(worst["lse"], _within(lse, ref["lse2"], bl, case["name"] + " lse2"))
        if case["family"] == "outside_window":
            assert fallbacks > 0, f"{case['name']}: the fallback was not taken"
        else:
            assert fallbacks == 0, f"{case['name']}: {fallbacks} workgroups took the fallback"
    print(f"PATH {path}: worst error / bound over {len(A.FWD_CASES[path])} cases: out {worst['out']:.3f} lse {worst['lse']:.3f}")


@pytest.mark.parametrize("path", [p for p in A.FWD_PATHS if p != "hd64_bias"])
def test_attention_output_does_not_depend_on_the_lse_argument(path):
    """lse=None and lse given: the same output bits, on the largest diffuse case of every forward kernel that has the argument."""
    case = max((c for c in A.FWD_CASES[path] if c["family"] == "diffuse"), key=lambda c: c["Sq"] * c["Skv"])
    _, kw, packed, _ = _reference(case["name"])
    with_lse, lse = _run_forward(case, kw, packed, with_lse=True)
    without, none = _run_forward(case, kw, packed, with_lse=False)
    assert lse is not None and none is None
    assert torch.equal(with_lse.contiguous().view(torch.int16), without.contiguous().view(torch.int16)), case["name"]


@pytest.mark.parametrize("skv", (257, 65, 320))
def test_resident_and_tiled_head_dim_80_kernels_agree_bitwise(skv):
    """attention_fwd_resident_kernel<80> and attention_fwd_kernel<80> share one tile step (csrc/attention.hpp): the same arithmetic in the
    same order, so the same bits.  257 queries over skv keys take the resident kernel; the same K / V under 513 queries (the first 257 rows
    the same) take the tiled one.  257 keys: a ragged fifth tile; 65: a ragged tile with one 16-key block; 320: five full tiles."""
    from adv_grpo_amd import ops
    B, H, hd, sq = 1, 2, 80, 257
    g = torch.Generator().manual_seed(8000 + skv)
    q = torch.randn(B, 513, H * hd, generator=g).to(torch.bfloat16).cuda()
    k = torch.randn(B, skv, H * hd, generator=g).to(torch.bfloat16).cuda()
    v = torch.randn(B, skv, H * hd, generator=g).to(torch.bfloat16).cuda()
    lse_res, lse_til = _sent_f32(B, H, sq), _sent_f32(B, H, 513)
    o_res = ops.attention(q[:, :sq], k, v, H, lse=lse_res)          # Sq <= 512 and Skv <= 320: resident
    o_til = ops.attention(q, k, v, H, lse=lse_til)                  # Sq > 512: tiled
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o_res.float()).all()) and bool(torch.isfinite(lse_res).all())
    assert torch.equal(o_res.view(torch.int16), o_til[:, :sq].contiguous().view(torch.int16)), "out"
    assert torch.equal(lse_res.view(torch.int32), lse_til[:, :, :sq].contiguous().view(torch.int32)), "lse"


# ---------------------------------------------------------------------------------------------------------------------- backward
def _run_backward(kw, packed, o, d_o, lse):
    """dq | dk | dv as column slices of ONE sentinel-filled packed buffer [B, S + 1, 3 H hd + 8]; o and d_o with a pitch of their own.
    Runs the entry twice into two such buffers: the bits must agree, and everything outside rows < Sq of dq and rows < Skv of dk / dv must
    still hold the sentinel."""
    from adv_grpo_amd import ops
    q, k, v, _ = A.to_device(kw, packed, "cuda")
    B, Sq, HD = q.shape
    Skv, H, S = k.shape[1], kw["H"], max(q.shape[1], k.shape[1])
    od = torch.zeros(B, Sq, HD + 8, dtype=torch.bfloat16, device="cuda")[:, :, :HD]
    gd = torch.zeros(B, Sq, HD + 64, dtype=torch.bfloat16, device="cuda")[:, :, :HD]
    od.copy_(o)
    gd.copy_(d_o)
    lse_d = lse.cuda()
    bufs = []
    for _ in range(2):
        buf = _sent_bf16(B, S + 1, 3 * HD + 8)
        dq, dk, dv = buf[:, :Sq, :HD], buf[:, :Skv, HD:2 * HD], buf[:, :Skv, 2 * HD:3 * HD]
        ops.attention_bwd(q, k, v, od, gd, lse_d, H, dq, dk, dv, scale=kw["scale"])
        torch.cuda.synchronize()
        bufs.append(buf)
    assert torch.equal(bufs[0].view(torch.int16), bufs[1].view(torch.int16)), "two backward launches on the same data differ"
    buf = bufs[0]
    written = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    written[:, :Sq, :HD] = True
    written[:, :Skv, HD:3 * HD] = True
    assert bool((buf.view(torch.int16)[~written] == SENT16).all()), "the backward wrote outside dq[:Sq] | dk[:Skv] | dv[:Skv]"
    return dict(dq=buf[:, :Sq, :HD], dk=buf[:, :Skv, HD:2 * HD], dv=buf[:, :Skv, 2 * HD:3 * HD])


@pytest.mark.parametrize("path", tuple(A.BWD_CASES))
def test_attention_backward_vs_float64(path):
    """attention_bwd_pipe_launch (bwd64) / attention_bwd_d128_launch (bwd128) on o and lse2 of the float64 forward reference."""
    worst = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
    for case in A.BWD_CASES[path]:
        _, kw, packed, fref = _reference(case["name"])
        _, _, d_o, o, lse, _ = A.make_backward_inputs(case, fref)
        r = A.backward(kw["q"], kw["k"], kw["v"], o, d_o, lse, kw["H"], kw["scale"])
        b = A.backward_bounds(r)
        got = _run_backward(kw, packed, o, d_o, lse)
        for n in ("dq", "dk", "dv"):
            worst[n] = max(worst[n], _within(got[n], r[n], b[n], f"{case['name']} {n}"))
    print(f"PATH {path}: worst error / bound over {len(A.BWD_CASES[path])} cases: " + " ".join(f"{n} {v:.3f}" for n, v in worst.items()))


@pytest.mark.parametrize("hd", tuple(A.CHAINED))
def test_attention_forward_into_backward_chained(hd):
    """Forward kernel -> backward kernel against the gradient at the exact o / lse2: the backward bound plus the forward's own bounds carried
    through D = sum_d o d_o and through P (attention_reference.backward_bounds; the host test shows every backward mutant leaving it)."""
    case = A.CHAINED[hd]
    _, kw, packed, fref = _reference(case["name"])
    _, _, d_o, _, _, _ = A.make_backward_inputs(case, fref)
    o_k, lse_k = _run_forward(case, kw, packed)
    r = A.backward(kw["q"], kw["k"], kw["v"], fref["o"], d_o, fref["lse2"], kw["H"], kw["scale"])
    dD, dL = A.chained_extras(fref, d_o, kw["H"])
    b = A.backward_bounds(r, dD=dD, dL=dL)
    got = _run_backward(kw, packed, o_k.cpu(), d_o, lse_k.cpu())
    for n in ("dq", "dk", "dv"):
        _within(got[n], r[n], b[n], f"{case['name']} {n}")
