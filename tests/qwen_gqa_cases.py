"""The cases and inputs of the grouped-query attention parity tests (test helper, not a test module; never imports adv_grpo_amd).

advgrpo_attention_fwd_gqa (csrc/attention_gqa.hip) is held to tests/attention_reference.py: the float64 reference `forward` on K / V expanded
to the query heads with repeat_interleave, and `forward_bounds`, the bound derived there from the stated arithmetic.  The input families are
that module's (diffuse, peaked, selector), built the way its make_inputs builds them but into ONE packed [B, S, (Hq + 2 Hkv) 128] buffer -- the
q | k | v GEMM output the kernel reads in place -- with the selector queries of head h pointing at keys of head h / (Hq / Hkv).

tests/test_qwen_text_entry_host.py shows on the CPU that the float32 emulation of the stated arithmetic lies inside the bound for every case
here; tests/test_gpu_qwen_text_entry.py compares the kernel element by element."""
import functools

import torch

import attention_reference as A

HD = 128
B = 2
HEADS = ((1, 1), (4, 2), (7, 1), (28, 4))            # (Hq, Hkv): plain multi-head, two per group, one group of seven, the real tower's
SEQ = (1, 63, 64, 65, 129, 257, 577)                 # one row; a ragged / full / one-over key tile; 3, 5 and 10 key tiles with ragged ends
FAMILIES = A.FAMILIES


def case(Hq, Hkv, S, family, causal):
    return dict(name=f"gqa-{family}-{Hq}over{Hkv}-{S}" + ("-causal" if causal else ""), Hq=Hq, Hkv=Hkv, S=S, family=family, causal=causal)


CASES = [case(hq, hkv, s, f, c) for hq, hkv in HEADS for s in SEQ for f in FAMILIES for c in (False, True)]


def expand(x, Hkv, G):
    """[B, S, Hkv hd] -> [B, S, Hkv G hd]: key/value head j repeated for its G query heads."""
    b, s, _ = x.shape
    return x.reshape(b, s, Hkv, HD).repeat_interleave(G, dim=2).reshape(b, s, Hkv * G * HD)


def views(packed, Hq, Hkv):
    """q, k, v as column slices of the packed buffer."""
    return packed[..., :Hq * HD], packed[..., Hq * HD:(Hq + Hkv) * HD], packed[..., (Hq + Hkv) * HD:]


def make_packed(c):
    """The packed bf16 buffer [B, S, (Hq + 2 Hkv) hd] of a case (CPU)."""
    g = A._gen(c["name"])
    Hq, Hkv, S, fam = c["Hq"], c["Hkv"], c["S"], c["family"]
    G, scale = Hq // Hkv, A.default_scale(HD)
    x = torch.randn(B, S, (Hq + 2 * Hkv) * HD, generator=g)
    if fam == "peaked":
        x[..., :Hq * HD] *= A.peak_factor(HD)
    elif fam == "selector":
        kk = torch.where(torch.randn(B, S, Hkv, HD, generator=g) >= 0, 1.0, -1.0)
        target = A.selector_target(S, S, c["causal"], g)
        a = torch.tensor(32.0 / (HD * scale)).to(A.BF16).float()
        x[..., Hq * HD:(Hq + Hkv) * HD] = kk.reshape(B, S, Hkv * HD)
        x[..., :Hq * HD] = (a * kk[:, target].repeat_interleave(G, dim=2)).reshape(B, S, Hq * HD)
        x[..., (Hq + Hkv) * HD:] = x[..., (Hq + Hkv) * HD:] * 0.5 + ((torch.arange(S) % 13).float() - 6.0)[None, :, None] * 0.5
    else:
        assert fam == "diffuse", fam
    return x.to(A.BF16)


@functools.lru_cache(maxsize=4)
def reference(name):
    """(case, packed buffer, keyword arguments of forward / emu_forward on the expanded K / V, float64 reference): computed once per case,
    shared, never modified."""
    c = next(c for c in CASES if c["name"] == name)
    packed = make_packed(c)
    q, k, v = views(packed, c["Hq"], c["Hkv"])
    G = c["Hq"] // c["Hkv"]
    kw = dict(q=q, k=expand(k, c["Hkv"], G), v=expand(v, c["Hkv"], G), H=c["Hq"], causal=c["causal"])
    return c, packed, kw, A.forward(**kw)
