"""CPU: the Qwen2.5-VL prompt-encoder entries (include/advgrpo.h "prompt encoding (Qwen-Image ...)") as far as they go without a device -- the
exports, the workspace size function, the refusals -- and a self-check of the inputs of the GPU parity test.

Every argument check of these entries runs on the host before anything is launched and the library loads without a device, so the
"pointers" below are small integers that are never dereferenced: every call to a launching entry in this file is refused."""
import ctypes
import os
import re

import pytest
import torch

import attention_reference as A
import qwen_gqa_cases as Q
from adv_grpo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a 256-byte aligned non-null "pointer"; never dereferenced
NEW = ["advgrpo_attention_fwd_gqa", "advgrpo_gqa_pack_heads", "advgrpo_gqa_unpack_heads", "advgrpo_qwen_prompt_embeds",
       "advgrpo_qwen_text_workspace_bytes", "advgrpo_qwen_text_forward"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _refused(lib, rc, fragment):
    assert rc == -1, (rc, lib.advgrpo_last_error())          # -1: an argument check (a launch that failed would be -2)
    with pytest.raises(_lib.AdvGrpoError) as e:
        _lib.check(rc)
    assert fragment in str(e.value), str(e.value)


# --------------------------------------------------------------------------------------------------------------------------- 1. exports
def test_library_exports_header_declares_and_signatures_list_the_new_entries(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advgrpo.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advgrpo_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/advgrpo.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
    assert lib.advgrpo_abi_version() == 1


# ----------------------------------------------------------------------------------------------------------------------- 2. size function
WS0 = dict(B=2, T=100, D=512, H=4, KV=2, hd=128, ff=1024)
SHAPES = (dict(), dict(B=1, T=1), dict(T=64), dict(T=65), dict(T=512), dict(B=2, T=512, D=3584, H=28, KV=4, ff=18944), dict(H=7, KV=1, D=896))


def _ws(lib, mode, **o):
    a = dict(WS0, **o)
    return lib.advgrpo_qwen_text_workspace_bytes(a["B"], a["T"], a["D"], a["H"], a["KV"], a["hd"], a["ff"], mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_size_function_grows_monotonically_and_returns_multiples_of_256(lib, mode):
    grow = [[dict(B=b) for b in (1, 2, 3, 8)], [dict(T=t) for t in (1, 23, 64, 65, 100, 128, 512)], [dict(D=d) for d in (64, 512, 3584, 4096)],
            [dict(ff=f) for f in (64, 1024, 18944)]]
    for steps in grow:
        sizes = [_ws(lib, mode, **o) for o in steps]
        assert all(s > 0 and s % 256 == 0 for s in sizes), (steps, sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (steps, sizes)


def test_the_fused_mode_never_needs_more_workspace_than_the_materialised_one(lib):
    for o in SHAPES:
        assert 0 < _ws(lib, 1, **o) <= _ws(lib, 0, **o), o
    assert _ws(lib, 1, T=1058) > 0                      # beyond the materialised cap the fused size is still defined
    assert _ws(lib, 2) == 0 and _ws(lib, -1) == 0       # an unknown mode has no size


# --------------------------------------------------------------------------------------------------------------------------- 3. refusals
WEIGHTS = (ctypes.c_void_p * 16)(*([P] * 16))
BIG = 1 << 40        # "enough" workspace bytes


def _fwd(lib, **o):
    a = dict(ids=P, emb=P, vocab=500, weights=WEIGHTS, n=2, final_w=P, cos_sin=P, B=2, T=100, D=512, H=4, KV=2, hd=128, ff=1024, mode=0, out=P,
             ws=P, ws_bytes=BIG)
    a.update(o)
    return lib.advgrpo_qwen_text_forward(a["ids"], a["emb"], a["vocab"], a["weights"], a["n"], a["final_w"], a["cos_sin"], a["B"], a["T"], a["D"],
                                         a["H"], a["KV"], a["hd"], a["ff"], 1e-6, a["mode"], a["out"], None, a["ws"], a["ws_bytes"], None)


def _gqa(lib, **o):
    a = dict(q=P, k=P, v=P, o=P, ldq=1024, ldk=1024, ldv=1024, ldo=512, B=2, Hq=4, Hkv=2, S=100, hd=128)
    a.update(o)
    return lib.advgrpo_attention_fwd_gqa(a["q"], a["k"], a["v"], a["o"], a["ldq"], a["ldk"], a["ldv"], a["ldo"], 100 * 1024, 100 * 1024, 100 * 1024,
                                         100 * 512, a["B"], a["Hq"], a["Hkv"], a["S"], a["hd"], 128 ** -0.5, 1, None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,label", [("ids", "ids"), ("emb", "emb"), ("weights", "weights"), ("final_w", "final_w"), ("cos_sin", "cos_sin"),
                                        ("out", "out"), ("ws", "workspace")])
def test_qwen_text_forward_refuses_null_pointers_by_name(lib, name, label, mode):
    _refused(lib, _fwd(lib, mode=mode, **{name: None}), f"qwen_text_forward: null pointer ({label})")


def test_qwen_text_forward_refuses_a_missing_layer_weight(lib):
    w = (ctypes.c_void_p * 16)(*([P] * 16))
    w[13] = None
    _refused(lib, _fwd(lib, weights=w), "qwen_text_forward: layer 1: weight 5 is missing")


@pytest.mark.parametrize("name", ["q", "k", "v", "o"])
def test_attention_fwd_gqa_refuses_null_pointers_by_name(lib, name):
    _refused(lib, _gqa(lib, **{name: None}), f"attention_fwd_gqa: null pointer ({name})")


def test_leaf_kernels_refuse_null_pointers(lib):
    for i in (0, 2, 3, 4):
        args = [P, 1024, P, P, P, 2, 37, 4, 2, 128, None]
        args[i] = None
        _refused(lib, lib.advgrpo_gqa_pack_heads(*args), "gqa_pack_heads: null pointer")
    _refused(lib, lib.advgrpo_gqa_unpack_heads(None, P, 2, 37, 4, 128, None), "gqa_unpack_heads: null pointer")
    _refused(lib, lib.advgrpo_gqa_unpack_heads(P, None, 2, 37, 4, 128, None), "gqa_unpack_heads: null pointer")
    for i in (0, 1, 2, 3):
        args = [P, P, P, P, 2, 60, 512, 20, 8, None, None]
        args[i] = None
        _refused(lib, lib.advgrpo_qwen_prompt_embeds(*args), "qwen_prompt_embeds: null pointer")
    _refused(lib, lib.advgrpo_qwen_prompt_embeds(P, P, P, P, 2, 60, 512, 20, 61, None, None), "qwen_prompt_embeds: bad shape")
    _refused(lib, lib.advgrpo_gqa_pack_heads(P, 1024, P, P, P, 2, 37, 4, 3, 128, None), "gqa_pack_heads: 4 query heads are not a multiple of 3")


@pytest.mark.parametrize("hd", [64, 96])
def test_head_dims_other_than_128_are_refused(lib, hd):
    _refused(lib, _gqa(lib, hd=hd), f"attention_fwd_gqa: head_dim {hd} not supported (128)")
    _refused(lib, _fwd(lib, mode=1, hd=hd), f"qwen_text_forward: head_dim {hd} not supported")


def test_query_heads_must_be_a_multiple_of_the_key_value_heads(lib):
    _refused(lib, _gqa(lib, Hq=4, Hkv=3), "attention_fwd_gqa: 4 query heads are not a multiple of 3 key/value heads")
    _refused(lib, _fwd(lib, H=4, KV=3), "qwen_text_forward: 4 query heads are not a multiple of 3 key/value heads")
    _refused(lib, _fwd(lib, mode=1, H=7, KV=2), "qwen_text_forward: 7 query heads are not a multiple of 2 key/value heads")


def test_the_materialised_mode_refuses_513_tokens_and_names_the_fused_mode(lib):
    _refused(lib, _fwd(lib, T=513), "up to 512 tokens (got 513); attention_mode 1 has no such cap")
    assert _fwd(lib, T=513, mode=1, ws_bytes=0) == -1 and b"workspace too small" in lib.advgrpo_last_error()      # mode 1 gets past the cap


@pytest.mark.parametrize("mode", [2, -1, 7])
def test_an_unknown_attention_mode_is_refused(lib, mode):
    _refused(lib, _fwd(lib, mode=mode), f"qwen_text_forward: unknown attention_mode {mode}")


@pytest.mark.parametrize("mode", [0, 1])
def test_misaligned_or_short_workspaces_are_refused(lib, mode):
    _refused(lib, _fwd(lib, mode=mode, ws=P + 128), "qwen_text_forward: workspace too small or not 256-byte aligned")
    _refused(lib, _fwd(lib, mode=mode, ws_bytes=_ws(lib, mode) - 1), "qwen_text_forward: workspace too small or not 256-byte aligned")


@pytest.mark.parametrize("name", ["ldq", "ldk", "ldv", "ldo"])
def test_attention_fwd_gqa_refuses_a_misaligned_row_pitch(lib, name):
    _refused(lib, _gqa(lib, **{name: 1028}), "attention_fwd_gqa: row and batch pitches must be multiples of 8 elements")


def test_attention_fwd_gqa_refuses_non_positive_sizes_and_misaligned_pointers(lib):
    for name in ("B", "Hq", "Hkv", "S"):
        _refused(lib, _gqa(lib, **{name: 0}), "attention_fwd_gqa: bad shape")
    _refused(lib, _gqa(lib, k=P + 8), "attention_fwd_gqa: q, k, v and o must be 16-byte aligned")
    _refused(lib, _gqa(lib, ldk=128), "attention_fwd_gqa: a row pitch is smaller than its heads")


# ------------------------------------------------------------------------------------------- 4. the GPU parity test's inputs, on the CPU
@pytest.mark.parametrize("S", Q.SEQ)
@pytest.mark.parametrize("Hq,Hkv", Q.HEADS)
def test_float32_emulation_of_every_parity_case_lies_inside_the_bound(Hq, Hkv, S):
    """For every case the GPU test runs: attention_reference.emu_forward (the stated arithmetic in float32) on K / V expanded to the query
    heads against the float64 reference and forward_bounds.  The inputs do not exceed the bound before any kernel has run."""
    worst = 0.0
    for c in (c for c in Q.CASES if (c["Hq"], c["Hkv"], c["S"]) == (Hq, Hkv, S)):
        _, packed, kw, ref = Q.reference(c["name"])
        assert packed.shape == (Q.B, S, (Hq + 2 * Hkv) * Q.HD) and kw["k"].shape[-1] == Hq * Q.HD
        G = Hq // Hkv
        kh = A.heads(kw["k"], Hq)
        assert all(torch.equal(kh[:, h], kh[:, h // G * G]) for h in range(Hq))       # the expansion: head h reads key/value head h / G
        got, _, _ = A.emu_forward(**kw)
        bound, _ = A.forward_bounds(ref, Hq)
        err = (got.double() - ref["o"]).abs()
        assert bool(torch.isfinite(got.float()).all()) and bool((err <= bound).all()), c["name"]
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
    print(f"gqa {Hq} over {Hkv}, S = {S}: worst emulation error / bound {worst:.3f}")
    assert worst <= 1.0
