"""CPU: the per-sample-length attention entries without a device -- exports and signatures, the header as plain C, every refusal with its
text (all of them come before the first launch: the "pointers" are small integers that are never dereferenced), the test's own
construction (masked softmax over the padded batch == per-sample unpadded reference), the fairness of the chosen inputs (the float32
emulation of the kernels' arithmetic stays inside the bounds for every case and sample), and mask_to_seq_lens restated."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import attention_reference as A
import attention_varlen_cases as V
from adv_grpo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a 16-byte aligned non-null "pointer"; never dereferenced


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_exports_and_signatures(lib):
    c_int, c_int64, c_float, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "advgrpo_attention_fwd_varlen": [vp] * 4 + [c_int64] * 8 + [c_int] * 4 + [c_float, vp, vp, vp],
        "advgrpo_attention_bwd_varlen": [vp] * 10 + [c_int64] * 12 + [c_int] * 4 + [c_float, vp, vp],
        "advgrpo_mask_to_seq_lens": [vp, c_int, vp, c_int, c_int, c_int, vp, vp],
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        res, sig = _lib.SIGNATURES[name]
        assert res is c_int and list(sig) == args, name
    assert lib.advgrpo_abi_version() == 1
    assert (_lib.U8, _lib.I32, _lib.I64) == (3, 4, 5)


def test_header_declares_the_entries_and_compiles_as_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "varlen.c"
    src.write_text("""#include "advgrpo.h"
typedef int (*fwd_t)(const void*, const void*, const void*, void*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                     int, int, int, int, float, const int32_t*, float*, void*);
typedef int (*bwd_t)(const void*, const void*, const void*, const void*, const void*, const float*, float*, void*, void*, void*,
                     int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                     int, int, int, int, float, const int32_t*, void*);
typedef int (*m2l_t)(const void*, int, int32_t*, int, int, int, int*, void*);
int main(void) {
    fwd_t f = advgrpo_attention_fwd_varlen; bwd_t b = advgrpo_attention_bwd_varlen; m2l_t m = advgrpo_mask_to_seq_lens;
    return (f && b && m && ADVGRPO_I32 == 4 && ADVGRPO_I64 == 5 && ADVGRPO_ABI_VERSION == 1) ? 0 : 1;
}
""")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "varlen.o")],
                   check=True)


# --------------------------------------------------------------------------------------------------------------------------- refusals
FWD = dict(q=P, k=P, v=P, o=P, ldq=1152, ldk=1152, ldv=1152, ldo=384, bsq=0, bsk=0, bsv=0, bso=0, B=2, H=3, S=100, head_dim=128, scale=0.1,
           seq_lens=P, lse=None)
BWD = dict(q=P, k=P, v=P, o=P, d_o=P, lse=P, work=P, dq=P, dk=P, dv=P, ldq=1152, ldk=1152, ldv=1152, ldo=384, lddo=384, lddq=1152,
           bsq=0, bsk=0, bsv=0, bso=0, bsdo=0, bsdq=0, B=2, H=3, S=100, head_dim=128, scale=0.1, seq_lens=P)


def _fwd(lib, **over):
    a = dict(FWD, **over)
    return lib.advgrpo_attention_fwd_varlen(a["q"], a["k"], a["v"], a["o"], a["ldq"], a["ldk"], a["ldv"], a["ldo"], a["bsq"], a["bsk"], a["bsv"],
                                            a["bso"], a["B"], a["H"], a["S"], a["head_dim"], a["scale"], a["seq_lens"], a["lse"], None)


def _bwd(lib, **over):
    a = dict(BWD, **over)
    return lib.advgrpo_attention_bwd_varlen(a["q"], a["k"], a["v"], a["o"], a["d_o"], a["lse"], a["work"], a["dq"], a["dk"], a["dv"], a["ldq"],
                                            a["ldk"], a["ldv"], a["ldo"], a["lddo"], a["lddq"], a["bsq"], a["bsk"], a["bsv"], a["bso"], a["bsdo"],
                                            a["bsdq"], a["B"], a["H"], a["S"], a["head_dim"], a["scale"], a["seq_lens"], None)


FWD_REFUSALS = [
    (dict(head_dim=64), "attention_fwd_varlen: head_dim 64 not supported (128)"),
    (dict(seq_lens=None), "attention_fwd_varlen: null seq_lens"),
    (dict(q=None), "attention_fwd_varlen: null pointer (q, k, v or o)"),
    (dict(o=None), "attention_fwd_varlen: null pointer (q, k, v or o)"),
    (dict(S=0), "attention_fwd_varlen: bad shape (B=2 H=3 S=0)"),
    (dict(B=0), "attention_fwd_varlen: bad shape (B=0 H=3 S=100)"),
    (dict(ldk=1156), "attention_fwd_varlen: row pitches ldq, ldk, ldv must keep 16-byte alignment"),
    (dict(ldo=388), "attention_fwd_varlen: o, ldo and bso must keep 16-byte aligned output rows"),
    (dict(o=P + 8), "attention_fwd_varlen: o, ldo and bso must keep 16-byte aligned output rows"),
    (dict(ldk=1 << 24, S=1 << 10), "attention: row pitch too large"),
    (dict(head_dim=64, seq_lens=None, S=0), "attention_fwd_varlen: head_dim 64 not supported (128)"),        # the order of the checks
]
BWD_REFUSALS = [
    (dict(head_dim=64), "attention_bwd_varlen: head_dim 64 not supported (128)"),
    (dict(seq_lens=None), "attention_bwd_varlen: null seq_lens"),
    (dict(work=None), "attention_bwd_varlen: null pointer"),
    (dict(H=0), "attention_bwd_varlen: bad shape (B=2 H=0 S=100)"),
    (dict(lddq=1156), "attention_bwd_varlen: row and batch pitches must keep 16-byte alignment"),
    (dict(bsdo=4), "attention_bwd_varlen: row and batch pitches must keep 16-byte alignment"),
    (dict(dk=P + 2), "attention_bwd_varlen: pointers must be 16-byte aligned"),
    (dict(ldq=1 << 21, S=1 << 10), "attention_bwd (d128): rows * row stride must stay below 2^30 elements (32-bit byte offsets)"),
]
M2L_REFUSALS = [
    ((None, _lib.U8, P, 2, 8, 0, None), "mask_to_seq_lens: null pointer (mask or seq_lens)"),
    ((P, _lib.U8, None, 2, 8, 0, None), "mask_to_seq_lens: null pointer (mask or seq_lens)"),
    ((P, _lib.BF16, P, 2, 8, 0, None), "mask_to_seq_lens: mask_dtype 1 not supported (ADVGRPO_U8, ADVGRPO_I32, ADVGRPO_I64)"),
    ((P, _lib.I64, P, 0, 8, 0, None), "mask_to_seq_lens: bad shape (B=0 Nt=8 base=0)"),
    ((P, _lib.I64, P, 2, 8, -1, None), "mask_to_seq_lens: bad shape (B=2 Nt=8 base=-1)"),
]


def _refused(lib, rc, text):
    assert rc == -1, (rc, lib.advgrpo_last_error())            # -1: an argument check; a launch that failed would be -2
    assert lib.advgrpo_last_error().decode() == text


@pytest.mark.parametrize("over,text", FWD_REFUSALS, ids=[str(i) for i in range(len(FWD_REFUSALS))])
def test_forward_refusals(lib, over, text):
    _refused(lib, _fwd(lib, **over), text)


@pytest.mark.parametrize("over,text", BWD_REFUSALS, ids=[str(i) for i in range(len(BWD_REFUSALS))])
def test_backward_refusals(lib, over, text):
    _refused(lib, _bwd(lib, **over), text)


@pytest.mark.parametrize("args,text", M2L_REFUSALS, ids=[str(i) for i in range(len(M2L_REFUSALS))])
def test_mask_to_seq_lens_refusals(lib, args, text):
    _refused(lib, lib.advgrpo_mask_to_seq_lens(*args, None), text)


# -------------------------------------------------------------------------------------------------------- the test's own construction
def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())


ALL_FWD = V.FWD_CASES + [V.FALLBACK_CASE]


def test_case_list_covers_what_it_claims():
    lens = {L for c in ALL_FWD for L in c["lens"]}
    assert {1, 63, 64, 65}.issubset(lens)
    assert {1, 2, 4, 5, 6}.issubset({(L + 63) // 64 for L in lens})                               # key tiles against the 4-slot ring
    assert any(L <= 256 < c["S"] for c in V.FWD_CASES for L in c["lens"])                          # whole query blocks are padding
    assert any(L % 256 and L > 256 and L < c["S"] for c in V.FWD_CASES for L in c["lens"])         # a block straddles L
    assert any(c["S"] in c["lens"] for c in V.FWD_CASES)
    assert {L for c in V.BWD_CASES for L in c["lens"]} == set(V.BWD_LENGTHS)
    assert {c["S"] for c in V.BWD_CASES} == {257, 300} and {c["H"] for c in V.BWD_CASES} == set(A.BWD_H[128])
    assert {c["family"] for c in V.FWD_CASES} == {c["family"] for c in V.BWD_CASES} == set(V.FAMILIES)
    assert all(c["H"] == 3 and c["hd"] == 128 for c in ALL_FWD)


@pytest.mark.parametrize("case", V.FWD_CASES, ids=lambda c: c["name"])
def test_masked_softmax_over_the_padded_batch_is_the_per_sample_reference(case):
    kw, _, refs = V.forward_case(case)
    o, lse2 = V.masked_forward(kw, case["lens"])
    for b, L in enumerate(case["lens"]):
        assert torch.allclose(o[b, :L], refs[b]["o"][0], rtol=1e-12, atol=1e-13)
        assert torch.allclose(lse2[b, :, :L], refs[b]["lse2"][0], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c["name"])
def test_masked_backward_over_the_padded_batch_is_the_per_sample_reference(case):
    kw, _, d_o, o, lse2, refs = V.backward_case(case)
    got = V.masked_backward(kw, o, d_o, lse2, case["lens"])
    for b, L in enumerate(case["lens"]):
        for name in ("dq", "dk", "dv"):
            ref = refs[b][name][0]
            assert torch.allclose(got[name][b, :L], ref, rtol=1e-11, atol=1e-12 * max(1.0, float(ref.abs().max()))), (b, name)
            assert not bool(got[name][b, L:].any()), (b, name)                                  # padding rows carry exactly zero gradient


def test_emulated_forward_stays_inside_the_bounds_for_every_case_and_sample():
    for case in ALL_FWD:
        kw, _, refs = V.forward_case(case)
        for b, L in enumerate(case["lens"]):
            o, lse, _ = A.emu_forward(**V.sample_kw(kw, b, L), tile0=case["family"] != "outside_window")
            bo, bl = A.forward_bounds(refs[b], kw["H"])
            assert _ratio(o, refs[b]["o"], bo) <= 1.0 and _ratio(lse, refs[b]["lse2"], bl) <= 1.0, (case["name"], b)


def test_emulated_backward_stays_inside_the_bounds_for_every_case_and_sample():
    for case in V.BWD_CASES:
        kw, _, d_o, o, lse2, refs = V.backward_case(case)
        for b, L in enumerate(case["lens"]):
            s = V.sample_kw(kw, b, L)
            got = A.emu_backward(s["q"], s["k"], s["v"], o[b:b + 1, :L], d_o[b:b + 1, :L], lse2[b:b + 1, :, :L], kw["H"], kw["scale"])
            bounds = A.backward_bounds(refs[b])
            for name in ("dq", "dk", "dv"):
                assert _ratio(got[name], refs[b][name], bounds[name]) <= 1.0, (case["name"], b, name)


def test_fallback_case_leaves_the_window_and_the_others_do_not():
    for case in ALL_FWD:
        kw, _, _ = V.forward_case(case)
        left = False
        for b, L in enumerate(case["lens"]):
            _, _, l = A.emu_forward(**V.sample_kw(kw, b, L), tile0=True)
            if case["family"] == "outside_window":
                left |= bool((~A.window_holds(l, margin=1e-5)).any())
            else:
                assert A.window_holds(l, margin=1e5).all(), (case["name"], b)
        assert left == (case["family"] == "outside_window"), case["name"]


def test_mask_to_seq_lens_restated():
    rows = torch.tensor([r for r, _ in V.MASK_ROWS])
    lens, bad = V.mask_to_seq_lens(rows, 256)
    assert lens == [259, 263, 257, 256, 258, 256, 261, 258]
    assert bad == sum(b for _, b in V.MASK_ROWS) == 4
    for (row, is_bad) in V.MASK_ROWS:
        assert V.mask_to_seq_lens(torch.tensor([row]), 0)[1] == int(is_bad)
    assert V.mask_to_seq_lens(rows.bool(), 0) == ([l - 256 for l in lens], bad)
