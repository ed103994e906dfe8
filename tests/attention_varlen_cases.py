"""Shared case list of the head-dim-128 attention with per-sample lengths (test helper, not a test module; never imports adv_grpo_amd).

A case is one padded batch: B samples of padded length S, H = 3 heads of 128, lengths L[b].  The reference of a masked batch is the
per-sample reference of tests/attention_reference.py at the sample's own length: sample b, rows 0 .. L[b] - 1, launched alone.  No new
tolerance: bit equality with the plain entries, or attention_reference's forward_bounds / backward_bounds.
"""
import torch

import attention_reference as A

HD = 128
H = 3

# forward: every length class of attention_d128.hip in one batch --
#   a single key (1); the 64-key tile edges 63 / 64 / 65; nt = 1, 2, 4, 5, 6 tiles against the 4-slot ring (64, 65 -> 2, 129 -> 3, 256 -> 4,
#   257 -> 5, 321 and 330 -> 6, 600 -> 10); L < 256 < S so that whole 256-query blocks are padding (65 at 600, 257 leaves the third
#   block of 600 empty); a block straddling L (300 at 600, 257 at 600); L = S.
FWD_BATCHES = (
    (330, (1, 64, 65, 330)),
    (330, (63, 129, 256, 257, 321)),
    (600, (65, 257, 300, 600)),
)
# backward: BWD_PAIRS' diagonal mixed in batches; 257 and 300 are no multiple of the 128- / 64-row own blocks or the 32-row tiles
BWD_LENGTHS = tuple(s for s, t in A.BWD_PAIRS if s == t)
assert BWD_LENGTHS == (1, 31, 33, 64, 65, 127, 129, 257)
BWD_BATCHES = (
    (257, (1, 31, 33, 64, 65, 127, 129, 257), A.BWD_H[128][1]),
    (300, (257, 1, 129, 65), A.BWD_H[128][0]),
    (300, (33, 127, 64, 31), A.BWD_H[128][2]),
)
FAMILIES = ("diffuse", "peaked")
# the family the existing suite shows on the running-maximum fallback at head dim 128 is outside_window (test_gpu_attention_parity.py asserts
# that diffuse / peaked / selector stay on the fast path): keys past tile 0 carry logits far above it, here with ragged lengths
FALLBACK = (321, (65, 129, 257, 321), "outside_window", 200.0)


def _mk(kind, S, lens, family, Hh=H, strength=200.0):
    c = A._case("varlen_" + kind, HD, S, S, family, B=len(lens), H=Hh, strength=strength)
    c["name"] += "-L" + "_".join(str(l) for l in lens)
    c["lens"] = tuple(lens)
    c["S"] = S
    return c


FWD_CASES = [_mk("fwd", S, lens, f) for S, lens in FWD_BATCHES for f in FAMILIES]
FALLBACK_CASE = _mk("fwd", FALLBACK[0], FALLBACK[1], FALLBACK[2], strength=FALLBACK[3])
BWD_CASES = [_mk("bwd", S, lens, f, Hh) for S, lens, Hh in BWD_BATCHES for f in FAMILIES]


def sample_kw(kw, b, L):
    """The forward keyword arguments of sample b alone at length L (views of the padded batch)."""
    return dict(q=kw["q"][b:b + 1, :L], k=kw["k"][b:b + 1, :L], v=kw["v"][b:b + 1, :L], H=kw["H"], scale=kw["scale"], bias=None, causal=False)


_FWD, _BWD = {}, {}


def forward_case(case):
    """(kw, packed, refs): the padded inputs and the per-sample float64 forward references.  Computed once per case, never modified."""
    if case["name"] not in _FWD:
        kw, _, packed = A.make_inputs(case)
        _FWD[case["name"]] = (kw, packed, [A.forward(**sample_kw(kw, b, L)) for b, L in enumerate(case["lens"])])
    return _FWD[case["name"]]


def backward_case(case):
    """(kw, packed, d_o, o, lse2, refs): d_o ~ N(0, 1) bf16 [B, S, H hd]; o (bf16) and lse2 (f32, [B, H, S]) as the backward entry receives
    them, from the per-sample float64 forward, zero on the padding rows; refs: per-sample float64 backward dicts."""
    if case["name"] not in _BWD:
        kw, packed, frefs = forward_case(case)
        B, S, Hh = case["B"], case["S"], case["H"]
        d_o = torch.randn(B, S, Hh * HD, generator=A._gen(case["name"] + "/d_o")).to(A.BF16)
        o = torch.zeros(B, S, Hh * HD, dtype=A.BF16)
        lse2 = torch.zeros(B, Hh, S, dtype=A.F32)
        refs = []
        for b, L in enumerate(case["lens"]):
            o[b, :L] = frefs[b]["o"][0].to(A.BF16)
            lse2[b, :, :L] = frefs[b]["lse2"][0].to(A.F32)
            skw = sample_kw(kw, b, L)
            refs.append(A.backward(skw["q"], skw["k"], skw["v"], o[b:b + 1, :L], d_o[b:b + 1, :L], lse2[b:b + 1, :, :L], Hh, kw["scale"]))
        _BWD[case["name"]] = (kw, packed, d_o, o, lse2, refs)
    return _BWD[case["name"]]


def masked_forward(kw, lens, dtype=A.F64):
    """Float64 masked softmax over the PADDED batch: keys >= L[b] at -inf.  Returns o [B, S, H hd], lse2 [B, H, S] (rows >= L meaningless)."""
    Hh = kw["H"]
    qh, kh, vh = A.heads(kw["q"], Hh, dtype), A.heads(kw["k"], Hh, dtype), A.heads(kw["v"], Hh, dtype)
    S = qh.shape[2]
    t = (qh @ kh.transpose(-1, -2)) * (kw["scale"] * A.LOG2E)
    hide = torch.arange(S)[None, :] >= torch.tensor(lens)[:, None]                     # [B, S] keys
    t = t.masked_fill(hide[:, None, None, :], float("-inf"))
    m = t.amax(-1, keepdim=True)
    e = torch.exp2(t - m)
    l = e.sum(-1, keepdim=True)
    return A.unheads((e / l) @ vh), (m + torch.log2(l)).squeeze(-1)


def masked_backward(kw, o, d_o, lse2, lens, dtype=A.F64):
    """Float64 backward over the padded batch with keys AND queries >= L[b] masked out of P."""
    Hh = kw["H"]
    qh, kh, vh, oh, gh = (A.heads(x, Hh, dtype) for x in (kw["q"], kw["k"], kw["v"], o, d_o))
    S = qh.shape[2]
    live = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]                       # [B, S]
    pair = (live[:, :, None] & live[:, None, :])[:, None]                               # [B, 1, Sq, Skv]
    P = torch.exp2((qh @ kh.transpose(-1, -2)) * (kw["scale"] * A.LOG2E) - lse2.to(dtype)[..., None])
    P = torch.where(pair, P, torch.zeros_like(P))
    D = (oh * gh).sum(-1, keepdim=True)
    dS = P * (gh @ vh.transpose(-1, -2) - D)
    return dict(dv=A.unheads(P.transpose(-1, -2) @ gh), dk=A.unheads(dS.transpose(-1, -2) @ qh * kw["scale"]),
                dq=A.unheads(dS @ kh * kw["scale"]))


def mask_to_seq_lens(mask, base):
    """The semantics of advgrpo_mask_to_seq_lens restated: (lengths, number of bad rows).  length = base + the number of LEADING non-zero
    entries; a row is bad when it has a non-zero entry behind a zero, or no leading non-zero entry at all."""
    lens, bad = [], 0
    for row in (mask != 0).tolist():
        lead = row.index(False) if False in row else len(row)
        lens.append(base + lead)
        bad += int(lead == 0 or any(row[lead:]))
    return lens, bad


MASK_ROWS = (            # (row, is it bad)
    ([1, 1, 1, 0, 0, 0, 0], False),
    ([1, 1, 1, 1, 1, 1, 1], False),
    ([1, 0, 0, 0, 0, 0, 0], False),
    ([0, 0, 0, 0, 0, 0, 0], True),       # all zero
    ([1, 1, 0, 1, 0, 0, 0], True),       # a non-zero behind a zero
    ([0, 1, 1, 1, 1, 1, 1], True),       # starts with a zero
    ([1, 1, 1, 1, 1, 0, 7], True),
    ([5, 3, 0, 0, 0, 0, 0], False),      # any non-zero value counts
)
