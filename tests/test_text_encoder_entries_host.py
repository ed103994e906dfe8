"""CPU: the prompt-encoding entries (include/advgrpo.h "prompt encoding") as far as they go without a device -- the exports, the T5
relative-position bucket (a host function of the ABI), the workspace size functions and the refusals.

Every argument check of these entries runs on the host before anything is launched and the library loads without a device, so the
"pointers" below are small integers that are never dereferenced: every call to a launching entry in this file is refused."""
import ctypes
import math
import os
import re

import pytest
import torch

from adv_grpo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000          # a 256-byte aligned non-null "pointer"; never dereferenced
NEW = ["advgrpo_token_embed", "advgrpo_t5_bucket", "advgrpo_t5_position_bias", "advgrpo_clip_eos_pool", "advgrpo_prompt_embeds_assemble",
       "advgrpo_clip_text_forward", "advgrpo_t5_forward", "advgrpo_encode_prompt",
       "advgrpo_clip_text_workspace_bytes", "advgrpo_t5_workspace_bytes", "advgrpo_encode_prompt_workspace_bytes"]


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


# ---------------------------------------------------------------------------------------------------------------------------- 2. bucket
def _formula_bucket(rel, dtype):
    """The formula of T5Encoder.position_bias (transformers' _relative_position_bucket, bidirectional, 32 buckets, max distance 128)."""
    nb = 32 // 2
    ret = (rel > 0).long() * nb
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.to(dtype) / max_exact) / math.log(128 / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ret + torch.where(n < max_exact, n, large)


REL = torch.arange(-511, 512)


def test_t5_bucket_equals_the_float64_formula_over_the_whole_range(lib):
    got = torch.tensor([lib.advgrpo_t5_bucket(int(r), 32, 128) for r in REL])
    assert torch.equal(got, _formula_bucket(REL, torch.float64))
    assert got.min() == 0 and got.max() == 31


def test_t5_bucket_equals_transformers(lib):
    t5 = pytest.importorskip("transformers.models.t5.modeling_t5")
    want = t5.T5Attention._relative_position_bucket(REL, bidirectional=True, num_buckets=32, max_distance=128)
    got = torch.tensor([lib.advgrpo_t5_bucket(int(r), 32, 128) for r in REL])
    assert torch.equal(got, want)


# the logarithmic half starts at distance 8 with bucket 8 and climbs one bucket per factor sqrt(2): at a power of two the exact value of
# 2 log2(n / 8) is an integer, which is where a float log can land on either side.  Expected values worked out by hand:
#   n      7  8  9 | 15 16 17 | 31 32 33 | 63 64 65 | 127 128 129
#   bucket 7  8  8 |  9 10 10 | 11 12 12 | 13 14 14 |  15  15  15
BOUNDARY = {7: 7, 8: 8, 9: 8, 15: 9, 16: 10, 17: 10, 31: 11, 32: 12, 33: 12, 63: 13, 64: 14, 65: 14, 127: 15, 128: 15, 129: 15}


@pytest.mark.parametrize("n,bucket", sorted(BOUNDARY.items()))
def test_t5_bucket_at_the_power_of_two_distances_and_their_neighbours(lib, n, bucket):
    assert lib.advgrpo_t5_bucket(-n, 32, 128) == bucket            # keys before the query
    assert lib.advgrpo_t5_bucket(n, 32, 128) == 16 + bucket        # keys after it: the upper 16 buckets


@pytest.mark.parametrize("nb,md", [(16, 128), (32, 64), (64, 128), (32, 256), (0, 0)])
def test_unsupported_bucket_parameters_are_refused_not_misbucketed(lib, nb, md):
    _refused(lib, lib.advgrpo_t5_bucket(5, nb, md), "only (num_buckets, max_distance) = (32, 128)")
    _refused(lib, lib.advgrpo_t5_position_bias(P, P, 3, 77, nb, md, None), "only (num_buckets, max_distance) = (32, 128)")


# ----------------------------------------------------------------------------------------------------------------------- 3. size functions
CLIP0, T50 = dict(B=2, S=77, D=128, mlp=256), dict(B=2, S=100, D=384, H=3, ff=320)
PROMPT0 = dict(B=2, S=77, T=100, Dl=128, mlp_l=256, Dg=192, mlp_g=384, Dt=384, Ht=3, ff=320)


def _clip_ws(lib, **o):
    a = dict(CLIP0, **o)
    return lib.advgrpo_clip_text_workspace_bytes(a["B"], a["S"], a["D"], a["mlp"])


def _t5_ws(lib, **o):
    a = dict(T50, **o)
    return lib.advgrpo_t5_workspace_bytes(a["B"], a["S"], a["D"], a["H"], a["ff"])


def _prompt_ws(lib, **o):
    a = dict(PROMPT0, **o)
    return lib.advgrpo_encode_prompt_workspace_bytes(*[a[k] for k in ("B", "S", "T", "Dl", "mlp_l", "Dg", "mlp_g", "Dt", "Ht", "ff")])


def test_size_functions_grow_monotonically_and_return_multiples_of_256(lib):
    grow = [(_clip_ws, [dict(B=b) for b in (1, 2, 3, 8)]), (_clip_ws, [dict(S=s) for s in (1, 16, 77)]),
            (_clip_ws, [dict(D=d, mlp=4 * d) for d in (64, 128, 768, 1280)]), (_clip_ws, [dict(mlp=m) for m in (64, 256, 3072)]),
            (_t5_ws, [dict(B=b) for b in (1, 2, 8)]), (_t5_ws, [dict(S=s) for s in (1, 77, 100, 128, 512)]),
            (_t5_ws, [dict(D=d) for d in (64, 384, 4096)]), (_t5_ws, [dict(ff=f) for f in (64, 320, 10240)]), (_t5_ws, [dict(H=h) for h in (1, 3, 64)]),
            (_prompt_ws, [dict(B=b) for b in (1, 2, 8)]), (_prompt_ws, [dict(S=s) for s in (1, 40, 77)]), (_prompt_ws, [dict(T=t) for t in (1, 100, 128, 512)]),
            (_prompt_ws, [dict(Dl=d) for d in (64, 128, 192)]), (_prompt_ws, [dict(Dg=d) for d in (64, 192, 256)]),
            (_prompt_ws, [dict(Dt=d) for d in (384, 1024, 4096)])]
    for fn, steps in grow:
        sizes = [fn(lib, **o) for o in steps]
        assert all(s > 0 and s % 256 == 0 for s in sizes), (fn.__name__, steps, sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (fn.__name__, steps, sizes)


def test_encode_prompt_workspace_covers_the_largest_tower(lib):
    for o in (dict(), dict(B=8, T=128, Dl=768, mlp_l=3072, Dg=1280, mlp_g=5120, Dt=4096, Ht=64, ff=10240), dict(T=1, Dt=320, Ht=1, ff=64)):
        a = dict(PROMPT0, **o)
        towers = [lib.advgrpo_clip_text_workspace_bytes(a["B"], a["S"], a["Dl"], a["mlp_l"]),
                  lib.advgrpo_clip_text_workspace_bytes(a["B"], a["S"], a["Dg"], a["mlp_g"]),
                  lib.advgrpo_t5_workspace_bytes(a["B"], a["T"], a["Dt"], a["Ht"], a["ff"])]
        assert _prompt_ws(lib, **o) >= max(towers)
    assert _clip_ws(lib) >= lib.advgrpo_vit_workspace_bytes(2, 77, 128, 256)        # the tower's stack runs inside its workspace


# --------------------------------------------------------------------------------------------------------------------------- 4. refusals
LAYERS = (_lib.VitLayer * 2)()
T5_WEIGHTS = (ctypes.c_void_p * 14)(*([P] * 14))
BIG = 1 << 40        # "enough" workspace bytes


def _clip(lib, **o):
    a = dict(ids=P, tok=P, pos=P, vocab=99, layers=LAYERS, n=2, ln_w=P, ln_b=P, proj=P, B=2, S=77, D=128, H=2, mlp=256, Pj=64, act=4, eos=2,
             pen=P, emb=P, ld=64, ws=P, ws_bytes=BIG)
    a.update(o)
    return lib.advgrpo_clip_text_forward(a["ids"], a["tok"], a["pos"], a["vocab"], a["layers"], a["n"], a["ln_w"], a["ln_b"], a["proj"], a["B"], a["S"],
                                         a["D"], a["H"], a["mlp"], a["Pj"], a["act"], 1e-5, a["eos"], a["pen"], a["emb"], a["ld"], None, a["ws"],
                                         a["ws_bytes"], None)


def _t5(lib, **o):
    a = dict(ids=P, emb=P, vocab=120, rel=P, nb=32, md=128, weights=T5_WEIGHTS, n=2, ln_w=P, B=2, S=100, D=384, H=3, d_kv=64, ff=320, out=P, ws=P,
             ws_bytes=BIG)
    a.update(o)
    return lib.advgrpo_t5_forward(a["ids"], a["emb"], a["vocab"], a["rel"], a["nb"], a["md"], a["weights"], a["n"], a["ln_w"], a["B"], a["S"], a["D"],
                                  a["H"], a["d_kv"], a["ff"], 1e-6, a["out"], None, a["ws"], a["ws_bytes"], None)


def _prompt(lib, **o):
    a = dict(ids_l=P, ids_g=P, ids_t=P, Dl=128, Hl=2, Dg=192, Hg=3, Dt=384, d_kv=64, nb=32, out=P, pooled=P, ws=P, ws_bytes=BIG, g_tok=P, t_emb=P)
    a.update(o)
    return lib.advgrpo_encode_prompt(
        a["ids_l"], P, P, 99, LAYERS, 2, P, P, P, a["Dl"], a["Hl"], 256, 64, 4, 2,
        a["ids_g"], a["g_tok"], P, 99, LAYERS, 2, P, P, P, a["Dg"], a["Hg"], 384, 128, 2, 98, 1e-5,
        a["ids_t"], a["t_emb"], 120, P, a["nb"], 128, T5_WEIGHTS, 2, P, a["Dt"], 3, a["d_kv"], 320, 1e-6,
        2, 77, 100, a["out"], a["pooled"], None, a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("name", ["ids", "tok", "pos", "layers", "ln_w", "ln_b", "proj", "pen", "emb", "ws"])
def test_clip_text_forward_refuses_null_pointers(lib, name):
    _refused(lib, _clip(lib, **{name: None}), "clip_text_forward: null argument")


@pytest.mark.parametrize("name", ["ids", "emb", "rel", "weights", "ln_w", "out", "ws"])
def test_t5_forward_refuses_null_pointers(lib, name):
    _refused(lib, _t5(lib, **{name: None}), "t5_forward: null argument")


@pytest.mark.parametrize("name", ["ids_l", "ids_g", "ids_t", "g_tok", "t_emb", "out", "pooled", "ws"])
def test_encode_prompt_refuses_null_pointers(lib, name):
    _refused(lib, _prompt(lib, **{name: None}), "encode_prompt: null argument")


def test_leaf_kernels_refuse_null_pointers(lib):
    _refused(lib, lib.advgrpo_token_embed(None, P, P, P, 2, 77, 128, 99, None, None), "token_embed: null pointer")
    _refused(lib, lib.advgrpo_token_embed(P, None, P, P, 2, 77, 128, 99, None, None), "token_embed: null pointer")
    _refused(lib, lib.advgrpo_token_embed(P, P, None, None, 2, 77, 128, 99, None, None), "token_embed: null pointer")
    _refused(lib, lib.advgrpo_token_embed(P, P, P, P, 2, 77, 128, 0, None, None), "token_embed: bad shape")
    _refused(lib, lib.advgrpo_t5_position_bias(None, P, 3, 77, 32, 128, None), "t5_position_bias: null pointer")
    _refused(lib, lib.advgrpo_t5_position_bias(P, None, 3, 77, 32, 128, None), "t5_position_bias: null pointer")
    _refused(lib, lib.advgrpo_clip_eos_pool(None, P, P, 2, 77, 128, 2, None), "clip_eos_pool: null pointer")
    _refused(lib, lib.advgrpo_clip_eos_pool(P, P, None, 2, 77, 128, 2, None), "clip_eos_pool: null pointer")
    for i in (0, 2, 4, 5):
        args = [P, 128, P, 192, P, P, 2, 77, 100, 384, None]
        args[i] = None
        _refused(lib, lib.advgrpo_prompt_embeds_assemble(*args), "prompt_embeds_assemble: null pointer")


def test_clip_widths_beyond_the_t5_width_are_refused(lib):
    _refused(lib, lib.advgrpo_prompt_embeds_assemble(P, 128, P, 320, P, P, 2, 77, 100, 384, None),
             "prompt_embeds_assemble: the CLIP widths 128 + 320 exceed the T5 width 384")
    _refused(lib, _prompt(lib, Dt=256), "encode_prompt: the CLIP widths 128 + 192 exceed the T5 width 256")


def test_head_dims_other_than_64_are_refused(lib):
    _refused(lib, _clip(lib, D=160, H=2), "clip_text_forward: head dim 80")
    _refused(lib, _clip(lib, D=128, H=4), "clip_text_forward: head dim 32")
    _refused(lib, _t5(lib, d_kv=128), "t5_forward: head dim 128")
    _refused(lib, _t5(lib, d_kv=32), "t5_forward: head dim 32")
    _refused(lib, _prompt(lib, Hl=1), "encode_prompt: head dims 128, 64, 64")
    _refused(lib, _prompt(lib, Hg=2), "encode_prompt: head dims 64, 96, 64")
    _refused(lib, _prompt(lib, d_kv=80), "encode_prompt: head dims 64, 64, 80")
    _refused(lib, _prompt(lib, nb=16), "encode_prompt: only (num_buckets, max_distance) = (32, 128)")
    _refused(lib, _t5(lib, nb=16), "t5_forward: only (num_buckets, max_distance) = (32, 128)")


def test_misaligned_or_short_workspaces_are_refused(lib):
    _refused(lib, _clip(lib, ws=P + 128), "clip_text_forward: workspace too small or not 256-byte aligned")
    _refused(lib, _clip(lib, ws_bytes=_clip_ws(lib) - 1), "clip_text_forward: workspace too small or not 256-byte aligned")
    _refused(lib, _t5(lib, ws=P + 16), "t5_forward: workspace too small or not 256-byte aligned")
    _refused(lib, _t5(lib, ws_bytes=_t5_ws(lib) - 1), "t5_forward: workspace too small or not 256-byte aligned")
    _refused(lib, _prompt(lib, ws=P + 64), "encode_prompt: workspace too small or not 256-byte aligned")
    _refused(lib, _prompt(lib, ws_bytes=_prompt_ws(lib) - 1), "encode_prompt: workspace too small or not 256-byte aligned")
