"""Prompt encoding on the gfx950 kernels: the three text encoders behind
``compute_text_embeddings`` (scripts/train_sd3_fast_pickscore.py:186-193) -> ``encode_prompt``
(adv_grpo/diffusers_patch/train_dreambooth_lora_sd3.py:98-144):

  CLIP-L and CLIP-G  (CLIPTextModelWithProjection: penultimate hidden state + projected pooled state)
  T5-XXL v1.1        (T5EncoderModel: RMSNorm, un-scaled attention + relative position bias, gated GELU)

Weights are given as transformers state dicts (same key names); token ids come from the caller (tokenizers are host
code outside the accelerated path).  Same GEMM / attention / norm kernels as the MMDiT; what is new for T5 is
``advgrpo_rmsnorm_rows``, the additive score bias of ``advgrpo_attention_fwd_bias`` and the ``mul_aux`` GEMM epilogue
(gate of the gated-GELU feed-forward)."""
import ctypes

import torch

from . import _lib, ops
from .vit import _bf, _Encoder, pack_clip_layers

_BAD_IDS = {}      # device -> int32 [1]: ids outside a vocabulary seen by advgrpo_token_embed (they embed as zero rows)


def _bad_ids(dev):
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _BAD_IDS:
        _BAD_IDS[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _BAD_IDS[dev]


def bad_id_count(device="cuda", reset=True):
    """Token ids outside their encoder's vocabulary since the last reset (each was embedded as a zero row, nothing was read out of
    range).  The encoders never look at the counter themselves; this call synchronises."""
    c = _bad_ids(device)
    n = int(c.item())
    if reset:
        c.zero_()
    return n


def _ids(input_ids, dev):
    return input_ids.to(device=dev, dtype=torch.int64).contiguous()


def _workspace(nbytes, dev):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)         # (torch's allocations are at least 512-byte aligned)


class CLIPTextEncoder:
    def __init__(self, sd, n_layers, heads, act, eos_token_id, device="cuda"):
        dev = torch.device(device)
        self.device, self.eos = dev, eos_token_id
        t = "text_model"
        layers = pack_clip_layers(sd, t, n_layers, dev)
        self.body = _Encoder(layers[:-1], heads, 1e-5, act, causal=True)
        self.last = _Encoder(layers[-1:], heads, 1e-5, act, causal=True)
        self.stack = _Encoder(layers, heads, 1e-5, act, causal=True)       # all layers: the host table advgrpo_clip_text_forward takes
        self.tok_emb = _bf(sd[f"{t}.embeddings.token_embedding.weight"], dev)
        self.pos = _bf(sd[f"{t}.embeddings.position_embedding.weight"], dev)
        self.final_ln = (_bf(sd[f"{t}.final_layer_norm.weight"], dev), _bf(sd[f"{t}.final_layer_norm.bias"], dev))
        self.proj = _bf(sd["text_projection.weight"], dev)
        self.D, self.P, self.mlp = self.tok_emb.shape[1], self.proj.shape[0], layers[0]["fc1.w"].shape[0]
        self._tower = None

    def tower_args(self):
        """The arguments of advgrpo_clip_text_forward behind `ids` that do not depend on the shape (_lib._CLIP_TOWER), built once: the
        weights are frozen, and the tensors the pointers name are held by this object."""
        if self._tower is None:
            tab = self.stack._table()
            self._tower = (self.tok_emb.data_ptr(), self.pos.data_ptr(), self.tok_emb.shape[0], ctypes.cast(tab, ctypes.POINTER(_lib.VitLayer)),
                           len(self.stack.layers), self.final_ln[0].data_ptr(), self.final_ln[1].data_ptr(), self.proj.data_ptr())
            self._keep = tab
        return self._tower

    @torch.no_grad()
    def __call__(self, input_ids, sequenced=False):
        """-> (hidden_states[-2] [B,S,D], text_embeds [B,P]) as _encode_prompt_with_clip takes them (TD3:84-88).  One call of
        advgrpo_clip_text_forward; sequenced=True: the launches one by one with torch indexing between them (the check)."""
        if sequenced:
            return self._call_sequenced(input_ids)
        lib = _lib.load()
        ids = _ids(input_ids, self.device)
        B, S = ids.shape
        assert S <= self.pos.shape[0]
        D, P = self.D, self.P
        pen = torch.empty(B, S, D, dtype=torch.bfloat16, device=self.device)
        emb = torch.empty(B, P, dtype=torch.bfloat16, device=self.device)
        ws = _workspace(lib.advgrpo_clip_text_workspace_bytes(B, S, D, self.mlp), self.device)
        _lib.check(lib.advgrpo_clip_text_forward(ids.data_ptr(), *self.tower_args(), B, S, D, self.stack.heads, self.mlp, P, ops.ACT[self.stack.act],
                                                 1e-5, self.eos, pen.data_ptr(), emb.data_ptr(), P, _bad_ids(self.device).data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return pen, emb

    def _call_sequenced(self, input_ids):
        ids = input_ids.to(self.device)
        B, S = ids.shape
        D = self.tok_emb.shape[1]
        x = (self.tok_emb[ids] + self.pos[:S][None]).reshape(B * S, D).contiguous()   # embedding gather: index plumbing
        x = self.body(x, B, S)
        pen = x.view(B, S, D).clone()
        x = self.last(x, B, S)
        eos = ids.int().argmax(dim=-1) if self.eos == 2 else (ids == self.eos).int().argmax(dim=-1)
        pooled = x.view(B, S, D)[torch.arange(B, device=self.device), eos].contiguous()
        pooled = ops.layernorm_mod(pooled, w=self.final_ln[0], b=self.final_ln[1], eps=1e-5)
        return pen, ops.gemm(pooled, self.proj)


class T5Encoder:
    _ORDER = ("ln1", "qkv", "o", "ln2", "wi0", "wi1", "wo")      # the order of a layer's seven pointers in advgrpo_t5_forward's `weights`

    def __init__(self, sd, n_layers, heads, d_kv=64, num_buckets=32, max_distance=128, device="cuda"):
        assert d_kv == 64, "the attention kernels serve head dim 64"
        dev = torch.device(device)
        self.device, self.H, self.nb, self.md = dev, heads, num_buckets, max_distance
        self.emb = _bf(sd["shared.weight"], dev)
        self.rel = sd["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"].to(dev, torch.bfloat16).float().contiguous()
        self.final_w = _bf(sd["encoder.final_layer_norm.weight"], dev)
        self.blocks = []
        for i in range(n_layers):
            p = f"encoder.block.{i}.layer"
            a, f = f"{p}.0.SelfAttention", f"{p}.1.DenseReluDense"
            self.blocks.append({
                "ln1": _bf(sd[f"{p}.0.layer_norm.weight"], dev), "ln2": _bf(sd[f"{p}.1.layer_norm.weight"], dev),
                "qkv": _bf(torch.cat([sd[f"{a}.q.weight"], sd[f"{a}.k.weight"], sd[f"{a}.v.weight"]]), dev),
                "o": _bf(sd[f"{a}.o.weight"], dev), "wi0": _bf(sd[f"{f}.wi_0.weight"], dev),
                "wi1": _bf(sd[f"{f}.wi_1.weight"], dev), "wo": _bf(sd[f"{f}.wo.weight"], dev)})
        self.D = self.emb.shape[1]
        self.ff = self.blocks[0]["wi0"].shape[0] if self.blocks else 64
        self._bias, self._bias_torch, self._tower, self._prompt = {}, {}, None, {}

    def tower_args(self):
        """The arguments of advgrpo_t5_forward behind `ids` that do not depend on the shape (_lib._T5_TOWER), built once."""
        if self._tower is None:
            tab = (ctypes.c_void_p * (7 * len(self.blocks)))(*[L[n].data_ptr() for L in self.blocks for n in self._ORDER])
            self._tower = (self.emb.data_ptr(), self.emb.shape[0], self.rel.data_ptr(), self.nb, self.md, tab, len(self.blocks),
                           self.final_w.data_ptr())
        return self._tower

    def position_bias(self, S):
        """[H,S,S] f32: T5Attention.compute_bias for the bidirectional encoder, by advgrpo_t5_position_bias; cached per S."""
        if S not in self._bias:
            bias = torch.empty(self.H, S, S, dtype=torch.float32, device=self.device)
            _lib.check(_lib.load().advgrpo_t5_position_bias(self.rel.data_ptr(), bias.data_ptr(), self.H, S, self.nb, self.md, _lib.stream_ptr()))
            self._bias[S] = bias
        return self._bias[S]

    def position_bias_torch(self, S):
        """The same table by torch indexing with a float log at the bucket boundaries: the check of position_bias."""
        if S not in self._bias_torch:
            import math
            rel = torch.arange(S, device=self.device)[None, :] - torch.arange(S, device=self.device)[:, None]
            nb = self.nb // 2
            ret = (rel > 0).long() * nb
            n = rel.abs()
            max_exact = nb // 2
            large = max_exact + (torch.log(n.float() / max_exact) / math.log(self.md / max_exact) * (nb - max_exact)).long()
            large = torch.min(large, torch.full_like(large, nb - 1))
            bucket = ret + torch.where(n < max_exact, n, large)
            self._bias_torch[S] = self.rel[bucket].permute(2, 0, 1).contiguous()
        return self._bias_torch[S]

    @torch.no_grad()
    def __call__(self, input_ids, sequenced=False):
        """-> last_hidden_state [B,S,D].  One call of advgrpo_t5_forward; sequenced=True: the launches one by one (the check)."""
        if sequenced:
            return self._call_sequenced(input_ids)
        lib = _lib.load()
        ids = _ids(input_ids, self.device)
        B, S = ids.shape
        out = torch.empty(B, S, self.D, dtype=torch.bfloat16, device=self.device)
        ws = _workspace(lib.advgrpo_t5_workspace_bytes(B, S, self.D, self.H, self.ff), self.device)
        _lib.check(lib.advgrpo_t5_forward(ids.data_ptr(), *self.tower_args(), B, S, self.D, self.H, 64, self.ff, 1e-6, out.data_ptr(),
                                          _bad_ids(self.device).data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
        return out

    def _call_sequenced(self, input_ids):
        ids = input_ids.to(self.device)
        B, S = ids.shape
        D = self.emb.shape[1]
        inner = self.H * 64
        x = self.emb[ids].reshape(B * S, D).contiguous()
        bias = self.position_bias_torch(S)
        for L in self.blocks:
            h = ops.rmsnorm_rows(x, L["ln1"])
            qkv = ops.gemm(h, L["qkv"]).view(B, S, 3 * inner)
            o = ops.attention_bias(qkv[:, :, :inner], qkv[:, :, inner:2 * inner], qkv[:, :, 2 * inner:], self.H, bias, scale=1.0)
            ops.gemm(o.view(B * S, inner), L["o"], residual=x, out=x)
            h = ops.rmsnorm_rows(x, L["ln2"])
            g = ops.gemm(h, L["wi0"], act="gelu_tanh")
            u = ops.gemm_train(h, L["wi1"], act="mul_aux", aux_in=g)                  # gelu(h W0^T) * (h W1^T)
            ops.gemm(u, L["wo"], residual=x, out=x)
        return ops.rmsnorm_rows(x, self.final_w).view(B, S, D)


def _clip_dims(c):
    return (c.D, c.stack.heads, c.mlp, c.P, ops.ACT[c.stack.act], c.eos)


@torch.no_grad()
def encode_prompt(clip_l, clip_g, t5, ids_l, ids_g, ids_t5, sequenced=False):
    """encode_prompt (TD3:98-144) from token ids: CLIP-L (+) CLIP-G penultimate states side by side, zero-padded to the T5
    width, followed by the T5 states along the sequence; pooled = the two projected pooled states side by side.  One call of
    advgrpo_encode_prompt; sequenced=True: the three towers launch by launch and the assembly by torch indexing (the check)."""
    if sequenced:
        return _encode_prompt_sequenced(clip_l, clip_g, t5, ids_l, ids_g, ids_t5)
    lib = _lib.load()
    dev = t5.device
    ids_l, ids_g, ids_t5 = _ids(ids_l, dev), _ids(ids_g, dev), _ids(ids_t5, dev)
    (B, S), T = ids_l.shape, ids_t5.shape[1]
    assert ids_g.shape == (B, S) and ids_t5.shape[0] == B and S <= min(clip_l.pos.shape[0], clip_g.pos.shape[0])
    key = (clip_l, clip_g, B, S, T)
    args = t5._prompt.get(key)
    if args is None:      # everything but the ids, the outputs, the workspace and the stream: once per shape
        nbytes = lib.advgrpo_encode_prompt_workspace_bytes(B, S, T, clip_l.D, clip_l.mlp, clip_g.D, clip_g.mlp, t5.D, t5.H, t5.ff)
        args = t5._prompt[key] = (clip_l.tower_args() + _clip_dims(clip_l), clip_g.tower_args() + _clip_dims(clip_g) + (1e-5,),
                                  t5.tower_args() + (t5.D, t5.H, 64, t5.ff, 1e-6, B, S, T), int(nbytes))
    a_l, a_g, a_t, nbytes = args
    out = torch.empty(B, S + T, t5.D, dtype=torch.bfloat16, device=dev)
    pooled = torch.empty(B, clip_l.P + clip_g.P, dtype=torch.bfloat16, device=dev)
    ws = _workspace(nbytes, dev)
    _lib.check(lib.advgrpo_encode_prompt(ids_l.data_ptr(), *a_l, ids_g.data_ptr(), *a_g, ids_t5.data_ptr(), *a_t, out.data_ptr(), pooled.data_ptr(),
                                         _bad_ids(dev).data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    return out, pooled


def _encode_prompt_sequenced(clip_l, clip_g, t5, ids_l, ids_g, ids_t5):
    pl, pooled_l = clip_l(ids_l, sequenced=True)
    pg, pooled_g = clip_g(ids_g, sequenced=True)
    t5e = t5(ids_t5, sequenced=True)
    B, S, _ = pl.shape
    out = torch.zeros(B, S + t5e.shape[1], t5e.shape[2], dtype=torch.bfloat16, device=t5e.device)
    out[:, :S, :pl.shape[2]] = pl
    out[:, :S, pl.shape[2]:pl.shape[2] + pg.shape[2]] = pg
    out[:, S:] = t5e
    return out, torch.cat([pooled_l, pooled_g], dim=-1)
