"""CPU: the float64 attention references of tests/attention_reference.py against torch's scaled_dot_product_attention and its float64 autograd,
the float32 constant C_ATT, the float32 emulation of the kernels' stated arithmetic inside every bound on every case of the GPU parity file
(tests/test_gpu_attention_parity.py), every named mutant of the emulation outside a bound on a named case, and the window bookkeeping of the
input families."""
import functools
import math

import torch
import torch.nn.functional as F

import attention_reference as A

F64 = torch.float64
ALL_FWD = [c for p in A.FWD_PATHS for c in A.FWD_CASES[p]]
ALL_BWD = [c for p in A.BWD_CASES for c in A.BWD_CASES[p]]


@functools.lru_cache(maxsize=None)
def _fwd(name):
    case = next(c for c in ALL_FWD + ALL_BWD + list(A.CHAINED.values()) if c["name"] == name)
    kw, target, packed = A.make_inputs(case)
    return case, kw, target, A.forward(**kw)


@functools.lru_cache(maxsize=None)
def _bwd(name):
    case, kw, _, fref = _fwd(name)
    _, _, d_o, o, lse, _ = A.make_backward_inputs(case, fref)
    r = A.backward(kw["q"], kw["k"], kw["v"], o, d_o, lse, kw["H"], kw["scale"])
    return case, kw, d_o, o, lse, r


def _ratio(got, ref, bound):
    err = (got.double() - ref).abs()
    assert not torch.isnan(err).any()
    return (err / bound.clamp_min(1e-300)).max().item()


def test_case_names_are_unique_and_every_path_has_cases():
    names = [c["name"] for c in ALL_FWD + ALL_BWD]
    assert len(names) == len(set(names))
    assert all(A.FWD_CASES[p] for p in A.FWD_PATHS) and all(A.BWD_CASES[p] for p in A.BWD_CASES)
    assert all(c["B"] == 2 and c["H"] % 2 == 1 for c in ALL_FWD + ALL_BWD)


def test_forward_reference_matches_scaled_dot_product_attention():
    picks = [A.FWD_CASES[p][i] for p in A.FWD_PATHS for i in (0, len(A.FWD_CASES[p]) // 2, -1)]
    picks += [c for c in A.FWD_CASES["hd64_bias"] if c["bias"] == "block" or c["causal"]]
    for case in picks:
        _, kw, _, ref = _fwd(case["name"])
        H = kw["H"]
        qh, kh, vh = (A.heads(kw[n], H) for n in ("q", "k", "v"))
        Sq, Skv = qh.shape[2], kh.shape[2]
        mask = None
        if kw["bias"] is not None:
            mask = kw["bias"].to(F64)[None].clone()
            if kw["causal"]:
                mask = mask.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool).triu(1), float("-inf"))
        want = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, is_causal=kw["causal"] and mask is None, scale=kw["scale"])
        assert (ref["o"] - A.unheads(want)).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), case["name"]
        s = qh @ kh.transpose(-1, -2) * kw["scale"] + (0.0 if mask is None else mask)
        if kw["causal"]:
            s = s.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool).triu(1), float("-inf"))
        lse = torch.logsumexp(s, -1) * A.LOG2E
        assert (ref["lse2"] - lse).abs().max().item() <= 1e-12 * max(1.0, lse.abs().max().item()), case["name"]
        assert (ref["A"] >= ref["o"].abs() * (1 - 1e-12)).all()                  # the magnitude dominates the value it bounds
        assert (ref["w"].sum(-1) - 1).abs().max().item() < 1e-12


def test_backward_reference_matches_float64_autograd():
    """With the unrounded o and lse2 of the forward reference the stated formulas are the gradient: 1e-12 relative against autograd through
    scaled_dot_product_attention in float64."""
    picks = [c for p in A.BWD_CASES for c in A.BWD_CASES[p] if (c["Sq"], c["Skv"]) in ((33, 129), (129, 33), (1, 257), (65, 65), (129, 129))]
    assert len(picks) >= 12
    for case in picks:
        _, kw, _, fref = _fwd(case["name"])
        _, _, d_o, _, _, _ = _bwd(case["name"])
        H = kw["H"]
        r = A.backward(kw["q"], kw["k"], kw["v"], fref["o"], d_o, fref["lse2"], H, kw["scale"])
        leaves = [A.heads(kw[n], H).clone().requires_grad_(True) for n in ("q", "k", "v")]
        out = F.scaled_dot_product_attention(*leaves, scale=kw["scale"])
        grads = torch.autograd.grad((out * A.heads(d_o, H)).sum(), leaves)
        for name, g in zip(("dq", "dk", "dv"), grads):
            want = A.unheads(g)
            assert (r[name] - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), (case["name"], name)


def test_float32_evaluation_stays_within_c_att():
    """The measurement C_ATT comes from: the reference formulas in torch float32 (no bf16 rounding inside) against float64, relative to the
    magnitudes the bounds multiply C_ATT with, over every case."""
    worst = {}
    for case in ALL_FWD:
        _, kw, _, ref = _fwd(case["name"])
        f32 = A.forward(**kw, dtype=torch.float32)
        mo, ml = A.forward_f32_magnitudes(ref, kw["H"])
        worst["out"] = max(worst.get("out", 0.0), _ratio(f32["o"], ref["o"], mo))
        worst["lse"] = max(worst.get("lse", 0.0), _ratio(f32["lse2"], ref["lse2"], ml))
    for case in ALL_BWD:
        _, kw, d_o, o, lse, r = _bwd(case["name"])
        f32 = A.backward(kw["q"], kw["k"], kw["v"], o, d_o, lse, kw["H"], kw["scale"], dtype=torch.float32)
        mags = A.backward_f32_magnitudes(r)
        for n in ("dq", "dk", "dv"):
            worst[n] = max(worst.get(n, 0.0), _ratio(f32[n], r[n], mags[n]))
    top = max(worst.values())
    print("float32 / float64, worst |diff| / magnitude:", {k: f"{v:.3e}" for k, v in worst.items()},
          f"-> measured constant {top:.3e} = 2^{math.log2(top):.1f}; x 4, rounded up to a power of two: 2^{math.ceil(math.log2(4 * top))}")
    assert 2.0 ** math.ceil(math.log2(4 * top)) == A.C_ATT, (top, A.C_ATT)


def test_emulation_of_the_stated_arithmetic_stays_inside_every_bound():
    """No element excluded; prints the worst error / bound per family."""
    worst = {}
    for case in ALL_FWD:
        _, kw, _, ref = _fwd(case["name"])
        tile0 = case["path"] in A.TILE0_PATHS and case["family"] != "outside_window"
        o, lse, _ = A.emu_forward(**kw, tile0=tile0)
        bo, bl = A.forward_bounds(ref, kw["H"])
        for what, r_ in (("out", _ratio(o, ref["o"], bo)), ("lse", _ratio(lse, ref["lse2"], bl))):
            key = (case["family"], what)
            worst[key] = max(worst.get(key, 0.0), r_)
            assert r_ <= 1.0, (case["name"], what, r_)
    for case in ALL_BWD:
        _, kw, d_o, o, lse, r = _bwd(case["name"])
        got = A.emu_backward(kw["q"], kw["k"], kw["v"], o, d_o, lse, kw["H"], kw["scale"])
        b = A.backward_bounds(r)
        for n in ("dq", "dk", "dv"):
            r_ = _ratio(got[n], r[n], b[n])
            key = (case["family"], n)
            worst[key] = max(worst.get(key, 0.0), r_)
            assert r_ <= 1.0, (case["name"], n, r_)
    for key in sorted(worst):
        print(f"emulation, family {key[0]:15s} {key[1]:4s}: worst error / bound = {worst[key]:.3f}")


def test_chained_bound_holds_the_emulation_and_is_not_vacuous():
    """Forward emulation -> backward emulation against the gradient at the exact o / lse2, under the backward bound plus the forward's bounds
    carried through D and P.  Not vacuous: every backward mutant still leaves it (the widening against the unchained bound is printed)."""
    for hd, case in A.CHAINED.items():
        _, kw, _, fref = _fwd(case["name"])
        _, _, d_o, _, _, _ = A.make_backward_inputs(case, fref)
        o_k, lse_k, _ = A.emu_forward(**kw, tile0=True)
        r = A.backward(kw["q"], kw["k"], kw["v"], fref["o"], d_o, fref["lse2"], kw["H"], kw["scale"])
        dD, dL = A.chained_extras(fref, d_o, kw["H"])
        b, b0 = A.backward_bounds(r, dD=dD, dL=dL), A.backward_bounds(r)
        got = A.emu_backward(kw["q"], kw["k"], kw["v"], o_k, d_o, lse_k, kw["H"], kw["scale"])
        for n in ("dq", "dk", "dv"):
            ratio, widen = _ratio(got[n], r[n], b[n]), (b[n] / b0[n].clamp_min(1e-300)).median().item()
            print(f"chained hd {hd} {n}: worst error / bound = {ratio:.3f}; median chained / unchained bound = {widen:.2f}")
            assert ratio <= 1.0, (hd, n, ratio)
        for mutant in A.BWD_MUTANTS:
            bad = A.emu_backward(kw["q"], kw["k"], kw["v"], o_k, d_o, lse_k, kw["H"], kw["scale"], mutant=mutant)
            worst = max(_ratio(bad[n], r[n], b[n]) for n in ("dq", "dk", "dv"))
            print(f"chained hd {hd}: mutant {mutant} reaches {worst:.1f} x the chained bound")
            assert worst > 1.0, (hd, mutant, worst)


def _fwd_mutant_kills(mutant, cases):
    for case in cases:
        _, kw, _, ref = _fwd(case["name"])
        tile0 = case["path"] in A.TILE0_PATHS and case["family"] != "outside_window"
        o, lse, _ = A.emu_forward(**kw, tile0=tile0, mutant=mutant)
        bo, bl = A.forward_bounds(ref, kw["H"])
        ro, rl = _ratio(o, ref["o"], bo), _ratio(lse, ref["lse2"], bl)
        if max(ro, rl) > 1.0:
            return case["name"], ro, rl
    return None


def test_every_forward_mutant_is_killed_by_a_named_case():
    relevant = {"causal_off_by_one": [c for c in ALL_FWD if c["causal"]], "bias_row_mod_128": [c for c in ALL_FWD if c["bias"]]}
    for mutant in A.FWD_MUTANTS:
        killed = _fwd_mutant_kills(mutant, relevant.get(mutant, ALL_FWD))
        assert killed is not None, f"no case kills the forward mutant {mutant}"
        print(f"forward mutant {mutant:22s} killed by {killed[0]} (out error / bound {killed[1]:.2f}, lse {killed[2]:.2f})")
    # the 0.5 % scale error is caught by the values, not only by lse: on a peaked case the output alone leaves its bound
    hits = [c["name"] for c in ALL_FWD if c["family"] == "peaked" and c["Skv"] >= 128 and c["Sq"] >= 128 and
            _ratio(A.emu_forward(**_fwd(c["name"])[1], mutant="scale_x1.005")[0], _fwd(c["name"])[3]["o"],
                   A.forward_bounds(_fwd(c["name"])[3], c["H"])[0]) > 1.0]
    assert hits, "no peaked case sees a scale error in the output"
    print(f"scale_x1.005 leaves the OUT bound on {len(hits)} peaked cases, first {hits[0]}")
    # every path's own case list kills the addressing mutants that apply to it
    for path in A.FWD_PATHS:
        for mutant in ("last_key_dropped", "v_pair_swapped"):
            assert _fwd_mutant_kills(mutant, A.FWD_CASES[path]) is not None, (path, mutant)


def test_every_backward_mutant_is_killed_by_a_named_case():
    for path, cases in A.BWD_CASES.items():
        for mutant in A.BWD_MUTANTS:
            killed = None
            for case in cases:
                _, kw, d_o, o, lse, r = _bwd(case["name"])
                got = A.emu_backward(kw["q"], kw["k"], kw["v"], o, d_o, lse, kw["H"], kw["scale"], mutant=mutant)
                b = A.backward_bounds(r)
                ratios = {n: _ratio(got[n], r[n], b[n]) for n in ("dq", "dk", "dv")}
                if max(ratios.values()) > 1.0:
                    killed = (case["name"], ratios)
                    break
            assert killed is not None, f"no {path} case kills the backward mutant {mutant}"
            print(f"backward mutant {mutant:24s} killed by {killed[0]} " + " ".join(f"{n} {v:.2f}" for n, v in killed[1].items()))


def test_window_bookkeeping_of_the_families():
    """From the float32 emulation relative to tile 0's maximum: diffuse, peaked and selector keep every row sum inside the kernels' window
    (with five decades to spare on both sides, so no rounding difference flips it); every outside_window case has a row that leaves it."""
    for path in A.TILE0_PATHS:
        for case in A.FWD_CASES[path]:
            _, kw, _, _ = _fwd(case["name"])
            _, _, l = A.emu_forward(**kw, tile0=True)
            if case["family"] == "outside_window":
                assert (~A.window_holds(l)).any(), case["name"]
                assert (~A.window_holds(l, margin=1e-5)).any(), case["name"]       # ... and not by a hair
            else:
                assert A.window_holds(l, margin=1e5).all(), case["name"]
    assert sum(c["family"] == "outside_window" for c in A.FWD_CASES["hd64_pipe"]) >= 2
    assert sum(c["family"] == "outside_window" for c in A.FWD_CASES["hd128"]) >= 1


def test_selector_rows_put_their_weight_on_the_named_key():
    n = 0
    for case in ALL_FWD + ALL_BWD:
        if case["family"] != "selector" or case["bias"]:
            continue
        _, kw, target, ref = _fwd(case["name"])
        w = ref["w"]                                                          # [B, H, Sq, Skv]
        picked = w.gather(-1, target[None, None, :, None].expand(*w.shape[:3], 1)).squeeze(-1)
        assert picked.min().item() >= 0.999, (case["name"], picked.min().item())
        if case["Sq"] >= case["Skv"] and not case["causal"]:
            assert set(target.tolist()) == set(range(case["Skv"])), case["name"]
        n += 1
    assert n > 100
    # peaked: a handful of effective keys (1 / sum w^2), against ~Skv / 2.4 for the diffuse family
    _, _, _, ref = _fwd("hd64_pipe-peaked-257x321")
    neff = 1.0 / (ref["w"] ** 2).sum(-1)
    assert 1.5 < neff.median().item() < 6.0, neff.median().item()
