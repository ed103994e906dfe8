"""GPU: the Qwen2.5-VL prompt encoder behind advgrpo_qwen_text_forward, its leaf kernels and the fused grouped-query attention
advgrpo_attention_fwd_gqa (csrc/attention_gqa.hip, csrc/qwen_text.hip, csrc/qwen_text_encoder.cpp).

 1. the fused kernel element by element against the float64 reference of tests/attention_reference.py on K / V expanded to the query heads,
    inside forward_bounds (the project's derived bound with its measured C_ATT; nothing fitted here), output in sentinel-filled buffers
 2. causality and independence, bitwise
 3. the non-causal result beside advgrpo_attention_fwd(head_dim 128): both inside the bound of the same reference
 4./5. pack / unpack / prompt_embeds bit-equal to the torch indexing they replace
 6. the entry in materialised mode equals the Python launch list bit for bit
 7./8. the fused mode against the fp32 oracle with the criterion of tests/test_gpu_qwen_text.py, also beyond 512 tokens
 9.-11. guards around outputs and workspaces, replay from a graph, out-of-vocabulary ids"""
import functools

import pytest
import torch

import attention_reference as A
import qwen_gqa_cases as Q

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
HD = Q.HD
SENT16 = 0x5A5B           # sentinel bit pattern (a bf16 of ~2.4e16: nothing a kernel here computes)
PAD, FILL = 4096, 0xA5


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(bf16)


def _is_sent(t):
    return bool((t.contiguous().view(torch.int16) == SENT16).all())


class Guards:
    """Buffers inside sentinel-filled allocations: alloc() hands out the middle, check() looks at both sides of every one."""

    def __init__(self):
        self.raw = []

    def alloc(self, shape, dtype):
        n = torch.empty(0, dtype=dtype).element_size()
        for d in shape:
            n *= d
        raw = torch.full((PAD + (n + 255) // 256 * 256 + PAD,), FILL, dtype=torch.uint8, device="cuda")
        self.raw.append((raw, n))
        return raw[PAD:PAD + n].view(dtype).view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for raw, n in self.raw:
            assert bool((raw[:PAD] == FILL).all()), "bytes in front of a buffer were written"
            assert bool((raw[PAD + n:] == FILL).all()), "bytes behind a buffer were written"


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


def _gqa(q, k, v, out, Hq, Hkv, causal):
    """advgrpo_attention_fwd_gqa on [B, S, heads * 128] views (any row / batch pitch)."""
    from adv_grpo_amd import _lib
    B, S, _ = q.shape
    _lib.check(_lib.load().advgrpo_attention_fwd_gqa(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q.stride(1), k.stride(1), v.stride(1),
                                                     out.stride(1), q.stride(0), k.stride(0), v.stride(0), out.stride(0), B, Hq, Hkv, S, HD,
                                                     float(HD ** -0.5), int(causal), _lib.stream_ptr()))
    return out


def _run_gqa(packed_dev, Hq, Hkv, causal):
    """The kernel's output as a [B, S, Hq hd] column slice of a sentinel-filled buffer with one spare row per batch and 8 spare columns;
    q | k | v are column slices of the one packed buffer.  Returns the output after checking the guards."""
    q, k, v = Q.views(packed_dev, Hq, Hkv)
    B, S, _ = q.shape
    buf = _sent_bf16(B, S + 1, Hq * HD + 8)
    out = _gqa(q, k, v, buf[:, :S, :Hq * HD], Hq, Hkv, causal)
    torch.cuda.synchronize()
    assert _is_sent(buf[:, S:]) and _is_sent(buf[:, :, Hq * HD:]), "the kernel wrote next to its output"
    return out


# ------------------------------------------------------------------------------------------------------- 1. parity of the fused kernel
@pytest.mark.parametrize("S", Q.SEQ)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Hq,Hkv", Q.HEADS)
def test_attention_fwd_gqa_vs_float64(Hq, Hkv, causal, S):
    from adv_grpo_amd import ops
    cases = [c for c in Q.CASES if (c["Hq"], c["Hkv"], c["S"], c["causal"]) == (Hq, Hkv, S, causal)]
    assert [c["family"] for c in cases] == list(Q.FAMILIES)
    ops.attention_fallback_count(reset=True)
    worst = 0.0
    for c in cases:
        _, packed, kw, ref = Q.reference(c["name"])
        out = _run_gqa(packed.cuda(), Hq, Hkv, causal)
        bound, _ = A.forward_bounds(ref, Hq)
        worst = max(worst, _within(out, ref["o"], bound, c["name"]))
    assert ops.attention_fallback_count(reset=True) == 0          # the kernel has no fallback path and leaves the counters alone
    print(f"gqa {Hq} over {Hkv}, S = {S}, causal = {causal}: worst error / bound {worst:.3f}")


# --------------------------------------------------------------------------------------------- 2. causality and independence, bitwise
def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _bitwise_base():
    c = Q.case(7, 1, 257, "diffuse", True)
    packed = Q.make_packed(c).cuda()
    return packed, _run_gqa(packed, 7, 1, True)


@pytest.mark.parametrize("t", [0, 63, 64, 200])
def test_keys_and_values_above_a_position_do_not_reach_the_rows_up_to_it(t):
    packed, base = _bitwise_base()
    g = torch.Generator(device="cuda").manual_seed(t)
    x = packed.clone()
    x[:, t + 1:, 7 * HD:] = (torch.randn(Q.B, 257 - t - 1, 2 * HD, device="cuda", generator=g) * 50).to(bf16)
    out = _run_gqa(x, 7, 1, True)
    assert torch.equal(_bits(out[:, :t + 1]), _bits(base[:, :t + 1]))
    assert not torch.equal(_bits(out[:, t + 1:]), _bits(base[:, t + 1:]))        # ... and the rows above it did see the change


def test_one_batch_does_not_reach_the_other():
    packed, base = _bitwise_base()
    x = packed.clone()
    x[1] = (torch.randn(257, 9 * HD, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 3).to(bf16)
    out = _run_gqa(x, 7, 1, True)
    assert torch.equal(_bits(out[0]), _bits(base[0])) and not torch.equal(_bits(out[1]), _bits(base[1]))


@pytest.mark.parametrize("causal", [False, True])
def test_the_seven_heads_of_a_group_equal_the_same_heads_run_one_at_a_time(causal):
    packed, base = _bitwise_base()
    if not causal:
        base = _run_gqa(packed, 7, 1, False)
    q, k, v = Q.views(packed, 7, 1)
    for h in range(7):
        buf = _sent_bf16(Q.B, 258, HD + 8)
        one = _gqa(q[..., h * HD:(h + 1) * HD], k, v, buf[:, :257, :HD], 1, 1, causal)
        torch.cuda.synchronize()
        assert _is_sent(buf[:, 257:]) and _is_sent(buf[:, :, HD:])
        assert torch.equal(_bits(one), _bits(base[..., h * HD:(h + 1) * HD])), h


# ------------------------------------------------------------------------------------- 3. beside the existing head-dim-128 kernel
@pytest.mark.parametrize("S", [129, 257])
def test_non_causal_multi_head_beside_attention_fwd(S):
    """Hq == Hkv, non-causal: advgrpo_attention_fwd_gqa and advgrpo_attention_fwd(head_dim 128) both inside the bound of the same
    float64 reference (bit equality is not asked for: the existing kernel takes every probability relative to tile 0's maximum)."""
    from adv_grpo_amd import ops
    H = 3
    packed = Q.make_packed(Q.case(H, H, S, "peaked", False))
    q, k, v = Q.views(packed, H, H)
    ref = A.forward(q, k, v, H)
    bound, _ = A.forward_bounds(ref, H)
    dev = packed.cuda()
    qd, kd, vd = Q.views(dev, H, H)
    _within(_run_gqa(dev, H, H, False), ref["o"], bound, f"gqa {H} over {H}, S = {S}")
    _within(ops.attention(qd, kd, vd, H), ref["o"], bound, f"attention_fwd hd 128, S = {S}")


# --------------------------------------------------------------------------------------------------------------- 4. pack and unpack
@pytest.mark.parametrize("B,T,H,KV", [(2, 37, 6, 2), (1, 64, 4, 4), (3, 100, 4, 2)])
def test_pack_and_unpack_heads_vs_torch_indexing(B, T, H, KV):
    from adv_grpo_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(T)
    Tp = (T + 63) // 64 * 64
    qkv = torch.randn(B * T, (H + 2 * KV) * HD, device="cuda", generator=g).to(bf16)
    x = qkv.view(B, T, H + 2 * KV, HD)                       # the indexing of Qwen25VLTextEncoder._attention
    q = torch.zeros(B * H, Tp, HD, dtype=bf16, device="cuda")
    q[:, :T] = x[:, :, :H].permute(0, 2, 1, 3).reshape(B * H, T, HD)
    k = torch.zeros(B * H, Tp, HD, dtype=bf16, device="cuda")
    k[:, :T] = x[:, :, H:H + KV].permute(0, 2, 1, 3).repeat_interleave(H // KV, dim=1).reshape(B * H, T, HD)
    vt = torch.zeros(B * H, HD, Tp, dtype=bf16, device="cuda")
    vt[:, :, :T] = x[:, :, H + KV:].permute(0, 2, 3, 1).repeat_interleave(H // KV, dim=1).reshape(B * H, HD, T)
    gd = Guards()
    gq, gk, gv = gd.alloc((B * H, Tp, HD), bf16), gd.alloc((B * H, Tp, HD), bf16), gd.alloc((B * H, HD, Tp), bf16)
    for t in (gq, gk, gv):
        t.view(torch.int16).fill_(0x7FC1)                    # a NaN pattern: the padding must be written by the kernel
    _lib.check(lib.advgrpo_gqa_pack_heads(qkv.data_ptr(), qkv.stride(0), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), B, T, H, KV, HD,
                                          _lib.stream_ptr()))
    gd.check()
    assert torch.equal(_bits(gq), _bits(q)) and torch.equal(_bits(gk), _bits(k)) and torch.equal(_bits(gv), _bits(vt))
    o = torch.randn(B * H, Tp, HD, device="cuda", generator=g).to(bf16)
    want = o[:, :T].reshape(B, H, T, HD).permute(0, 2, 1, 3).reshape(B * T, H * HD).contiguous()
    got = gd.alloc((B * T, H * HD), bf16)
    _lib.check(lib.advgrpo_gqa_unpack_heads(o.data_ptr(), got.data_ptr(), B, T, H, HD, _lib.stream_ptr()))
    gd.check()
    assert torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------------------------ 5. prompt embeds
def _loop(hs, lens, drop):
    L = max(n - drop for n in lens)
    emb = torch.zeros(hs.shape[0], L, hs.shape[2], dtype=hs.dtype, device=hs.device)
    msk = torch.zeros(hs.shape[0], L, dtype=torch.long, device=hs.device)
    for b, n in enumerate(lens):
        emb[b, :n - drop] = hs[b, drop:n]
        msk[b, :n - drop] = 1
    return emb, msk


@pytest.mark.parametrize("D", [512, 100])                   # 16-byte rows and the scalar path
@pytest.mark.parametrize("drop", [8, 34])
def test_prompt_embeds_kernel_vs_the_python_loop(drop, D):
    from adv_grpo_amd import _lib
    lib = _lib.load()
    B, T = 4, 60
    hs = torch.randn(B, T, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(drop)).to(bf16)
    lens = [T, T - 7, drop, drop + 1]                        # full, shorter, exactly the template (an all-zero sample), one token
    want, wmask = _loop(hs, lens, drop)
    L = want.shape[1]
    gd = Guards()
    emb, msk, bad = gd.alloc((B, L, D), bf16), gd.alloc((B, L), torch.int64), gd.alloc((1,), torch.int32)
    emb.view(torch.int16).fill_(0x7FC1)
    msk.fill_(-1)
    bad.zero_()
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    _lib.check(lib.advgrpo_qwen_prompt_embeds(hs.data_ptr(), dl.data_ptr(), emb.data_ptr(), msk.data_ptr(), B, T, D, L, drop, bad.data_ptr(),
                                              _lib.stream_ptr()))
    gd.check()
    assert torch.equal(_bits(emb), _bits(want)) and torch.equal(msk, wmask) and int(bad.item()) == 0
    assert bool((emb[2] == 0).all()) and int(msk[2].sum()) == 0
    # lengths outside [drop, T]: clamped (T + 5 -> T, drop - 3 -> drop, -1 -> drop) and counted, nothing read out of range
    dl = torch.tensor([T + 5, drop - 3, -1, T], dtype=torch.int32, device="cuda")
    want, wmask = _loop(hs, [T, drop, drop, T], drop)
    _lib.check(lib.advgrpo_qwen_prompt_embeds(hs.data_ptr(), dl.data_ptr(), emb.data_ptr(), msk.data_ptr(), B, T, D, L, drop, bad.data_ptr(),
                                              _lib.stream_ptr()))
    gd.check()
    assert torch.equal(_bits(emb), _bits(want)) and torch.equal(msk, wmask) and int(bad.item()) == 3


# ------------------------------------------------------------------------------------------------------------------------- the towers
def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


SMALL = dict(vocab_size=500, hidden_size=512, intermediate_size=1024, num_layers=3, num_heads=4, num_kv_heads=2)
REAL = dict(vocab_size=2000, num_layers=2)


@functools.lru_cache(maxsize=None)
def _tower(which):
    """(weights on the device in bf16, our config, the oracle's config) of the small tower / the real width on two layers, as in
    tests/test_gpu_qwen_text.py."""
    from adv_grpo_amd import synthetic
    from adv_grpo_amd.model_configs import QwenTextConfig
    from oracle import qwen_text as o
    kw = SMALL if which == "small" else REAL
    cfg = QwenTextConfig(**kw)
    if which == "small":
        W = {k: v.to(bf16).cuda() for k, v in synthetic.qwen_text_weights(cfg, 7).items()}
    else:
        with synthetic.on_device("cuda"):
            W = synthetic.qwen_text_weights(cfg, 9, dtype=bf16)
    return W, cfg, o.QwenTextConfig(**kw)


@functools.lru_cache(maxsize=None)
def _encoder(which, attention):
    from adv_grpo_amd.qwen_text_encoder import Qwen25VLTextEncoder
    W, cfg, _ = _tower(which)
    return Qwen25VLTextEncoder(W, cfg, "cuda", attention=attention)


CONFIGS = [("small", 3, 23), ("small", 2, 100), ("real", 2, 60)]


def _ids(which, B, T):
    vocab = (SMALL if which == "small" else REAL)["vocab_size"]
    return torch.randint(0, vocab, (B, T), generator=torch.Generator().manual_seed(T)).cuda()


@functools.lru_cache(maxsize=None)
def _oracle(which, B, T):
    """(fp32 oracle output, relative error of torch's own bf16 run of the oracle code): once per configuration."""
    from oracle import qwen_text as o
    W, _, ocfg = _tower(which)
    ids = _ids(which, B, T)
    ref = o.text_model_forward({k: v.float() for k, v in W.items()}, ocfg, ids)
    return ref, _rel(o.text_model_forward(W, ocfg, ids), ref)


# ----------------------------------------------------------------------------------------------- 6. the entry equals the launch list
@pytest.mark.parametrize("which,B,T", CONFIGS)
def test_materialised_entry_equals_the_python_sequencing_bit_for_bit(which, B, T):
    enc = _encoder(which, "materialised")
    ids = _ids(which, B, T)
    got, want = enc(ids), enc(ids, sequenced=True)
    assert got.shape == want.shape == (B, T, enc.cfg.hidden_size) and torch.equal(_bits(got), _bits(want))
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, T - 5:] = 0
    for drop in (8, 34) if T > 34 else (8,):
        emb, msk = enc.encode_prompt(ids, mask, drop_idx=drop)
        emb_s, msk_s = enc.encode_prompt(ids, mask, drop_idx=drop, sequenced=True)
        assert emb.shape == emb_s.shape and torch.equal(_bits(emb), _bits(emb_s)) and torch.equal(msk, msk_s)


# ------------------------------------------------------------------------------------------------------ 7. fused mode vs the oracle
@pytest.mark.parametrize("which,B,T", CONFIGS)
def test_fused_entry_vs_oracle(which, B, T):
    """The criterion of tests/test_gpu_qwen_text.py: within 2x of torch's own bf16 run of the oracle code (or 1e-2).  Prints the relative L2
    errors fused | materialised | torch-bf16 (the figures of deviation 19 in DESIGN.md section 3)."""
    ref, e_torch = _oracle(which, B, T)
    ids = _ids(which, B, T)
    e_fused, e_mat = _rel(_encoder(which, "fused")(ids), ref), _rel(_encoder(which, "materialised")(ids), ref)
    print(f"qwen text {which} B={B} T={T}: rel err fused {e_fused:.5f} materialised {e_mat:.5f} torch-bf16 {e_torch:.5f}")
    assert e_fused < max(2 * e_torch, 1e-2), (e_fused, e_torch)


# ------------------------------------------------------------------------------------------------------------ 8. the cap is lifted
def test_577_tokens_need_the_fused_mode_and_meet_the_oracle():
    ids = _ids("small", 1, 577)
    with pytest.raises(ValueError, match='attention="fused"'):
        _encoder("small", "materialised")(ids)
    with pytest.raises(ValueError, match='attention="fused"'):
        _encoder("small", "fused")(ids, sequenced=True)
    out = _encoder("small", "fused")(ids)
    assert out.shape == (1, 577, 512) and bool(torch.isfinite(out.float()).all())
    ref, e_torch = _oracle("small", 1, 577)
    e_fused = _rel(out, ref)
    print(f"qwen text small B=1 T=577: rel err fused {e_fused:.5f} torch-bf16 {e_torch:.5f}")
    assert e_fused < max(2 * e_torch, 1e-2), (e_fused, e_torch)


# --------------------------------------------------------------------------------------------------- 9. stays inside its buffers
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,T", [(3, 23), (2, 100)])
def test_entry_stays_inside_its_output_and_workspace(B, T, mode):
    """advgrpo_qwen_text_forward called directly on a guarded output and a guarded workspace of exactly the advertised size."""
    from adv_grpo_amd import _lib
    lib = _lib.load()
    enc = _encoder("small", "fused" if mode else "materialised")
    cfg = enc.cfg
    ids = _ids("small", B, T)
    D, H, KV, hd, ff = cfg.hidden_size, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.intermediate_size
    n = lib.advgrpo_qwen_text_workspace_bytes(B, T, D, H, KV, hd, ff, mode)
    gd = Guards()
    out, ws, bad = gd.alloc((B, T, D), bf16), gd.alloc((n,), torch.uint8), gd.alloc((1,), torch.int32)
    bad.zero_()
    _lib.check(lib.advgrpo_qwen_text_forward(ids.data_ptr(), *enc.tower_args(), enc._cos_sin(T).data_ptr(), B, T, D, H, KV, hd, ff, float(cfg.rms_eps),
                                             mode, out.data_ptr(), bad.data_ptr(), ws.data_ptr(), n, _lib.stream_ptr()))
    gd.check()
    assert torch.equal(_bits(out), _bits(enc(ids))) and int(bad.item()) == 0


# ------------------------------------------------------------------------------------------------------------- 10. capturability
def test_fused_entry_replays_from_a_graph():
    enc = _encoder("small", "fused")
    ids = _ids("small", 2, 100)
    mask = torch.ones(2, 100, dtype=torch.long)
    eager = enc(ids)                      # also: every lazy set-up (code objects, the rotary table, the counter) happens here
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):         # one stream, no parallel branches
        out = enc(ids, mask)
    out.view(torch.int16).fill_(0x7FC1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


# --------------------------------------------------------------------------------------------------------- 11. out-of-vocabulary ids
@pytest.mark.parametrize("attention", ["materialised", "fused"])
def test_out_of_vocabulary_ids_embed_as_zero_rows_and_are_counted(attention):
    """Ids -1 and vocab behave exactly like a token whose embedding row is zero: the same output bits as the tower run on a table with
    an all-zero row in place of the bad ids, and text_encoders.bad_id_count() reports two.  No device assert."""
    from adv_grpo_amd import text_encoders as te
    from adv_grpo_amd.qwen_text_encoder import Qwen25VLTextEncoder
    W, cfg, _ = _tower("small")
    ids = _ids("small", 2, 23)
    bad = ids.clone()
    bad[0, 5], bad[1, 22] = -1, cfg.vocab_size
    W0 = dict(W)
    W0["embed_tokens.weight"] = W["embed_tokens.weight"].clone()
    W0["embed_tokens.weight"][7] = 0
    zero = ids.clone()
    zero[0, 5] = zero[1, 22] = 7
    te.bad_id_count()
    got = _encoder("small", attention)(bad)
    assert te.bad_id_count() == 2 and te.bad_id_count() == 0
    want = Qwen25VLTextEncoder(W0, cfg, "cuda", attention=attention)(zero)
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(_bits(got), _bits(want))
