// text_encoders.cpp -- prompt encoding behind C-ABI entries: the CLIP text tower (CLIP-L, CLIP-G), the T5 v1.1 encoder, and encode_prompt
// over the three (adv_grpo/diffusers_patch/train_dreambooth_lora_sd3.py:98-144, reached from compute_text_embeddings,
// scripts/train_sd3_fast_pickscore.py:186-193).
//
// Until now the launch order of these towers lived in Python (adv_grpo_amd/text_encoders.py) and four of its steps were torch indexing;
// text_embed.hip has those steps as kernels and this file is the order in C++:
//   advgrpo_clip_text_forward   token + position embedding -> advgrpo_vit_forward over layers [0, n-1) -> copy-out of the penultimate state
//                               (hidden_states[-2]) -> advgrpo_vit_forward over the last layer -> EOS pooling -> final LayerNorm -> projection
//   advgrpo_t5_forward          token embedding, relative-position bias into the workspace, then per block: RMSNorm -> q|k|v GEMM ->
//                               attention with the additive bias (scale 1) -> out-proj + residual -> RMSNorm -> wi_0 with GELU(tanh) ->
//                               wi_1 times that gate (mul_aux epilogue) -> wo + residual; a final RMSNorm
//   advgrpo_encode_prompt       the two CLIP towers, T5, and the [B, S + T, Dt] assembly; the pooled pair side by side
// The same kernels, in the same order, with the same epilogues as the Python sequencing, which stays as the check: bit-identical
// (tests/test_gpu_text_encoder_entries.py).  No allocation, no synchronisation, no host <-> device copy: the entries can be captured in
// a graph.  Host-only code: it only calls this library's own C entries (and one device-to-device copy on the caller's stream).
#include "common.hpp"

using namespace advgrpo;

namespace {
inline int64_t piece(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
struct Carver {      // hands out 256-byte aligned pieces of the caller's workspace, in the order the size functions add them up
    char* w;
    char* take(int64_t bytes) { char* p = w; w += piece(bytes); return p; }
};
}  // namespace

// ----------------------------------------------------------------------------------------------------------------------- CLIP text tower
extern "C" int64_t advgrpo_clip_text_workspace_bytes(int B, int S, int D, int mlp) {
    const int64_t M = (int64_t)B * S;
    return piece(M * D * 2) + 2 * piece((int64_t)B * D * 2) + advgrpo_vit_workspace_bytes(B, S, D, mlp);
}

extern "C" int advgrpo_clip_text_forward(const int64_t* ids, const void* tok_emb, const void* pos_emb, int vocab, const advgrpo_vit_layer* layers,
                                         int n_layers, const void* final_ln_w, const void* final_ln_b, const void* proj_w, int B, int S, int D,
                                         int H, int mlp, int P, int act, float eps, int eos_token_id, void* penultimate, void* text_embeds,
                                         int64_t ld_text_embeds, int* bad_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    ADVGRPO_CHECK(ids && tok_emb && pos_emb && layers && final_ln_w && final_ln_b && proj_w && penultimate && text_embeds && workspace,
                  "clip_text_forward: null argument");
    ADVGRPO_CHECK(B > 0 && S > 0 && D > 0 && H > 0 && mlp > 0 && P > 0 && vocab > 0 && n_layers >= 1 && D % H == 0 && ld_text_embeds >= P,
                  "clip_text_forward: bad shape (B=%d S=%d D=%d H=%d mlp=%d P=%d vocab=%d layers=%d)", B, S, D, H, mlp, P, vocab, n_layers);
    ADVGRPO_CHECK(D / H == 64, "clip_text_forward: head dim %d (the CLIP text towers have 64)", D / H);
    ADVGRPO_CHECK(workspace_bytes >= advgrpo_clip_text_workspace_bytes(B, S, D, mlp) && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "clip_text_forward: workspace too small or not 256-byte aligned");
    const int64_t M = (int64_t)B * S;
    Carver c{reinterpret_cast<char*>(workspace)};
    char* x = c.take(M * D * 2);
    char* pooled = c.take((int64_t)B * D * 2);
    char* pooled_n = c.take((int64_t)B * D * 2);
    char* vit_ws = c.w;
    const int64_t vit_bytes = advgrpo_vit_workspace_bytes(B, S, D, mlp);
    int rc;
    if ((rc = advgrpo_token_embed(ids, tok_emb, pos_emb, x, B, S, D, vocab, bad_ids, stream)) != 0) return rc;
    advgrpo_vit_desc d{};
    d.B = B; d.S = S; d.D = D; d.H = H; d.mlp = mlp; d.act = act; d.causal = 1; d.eps = eps; d.x = x;
    d.layers = layers; d.n_layers = n_layers - 1;
    if (d.n_layers > 0 && (rc = advgrpo_vit_forward(&d, vit_ws, vit_bytes, stream)) != 0) return rc;
    // hidden_states[-2]: what the SD3 pipeline takes from a CLIP tower (device-to-device, asynchronous on the caller's stream)
    if (hipMemcpyAsync(penultimate, x, (size_t)(M * D * 2), hipMemcpyDeviceToDevice, as_stream(stream)) != hipSuccess) {
        set_error("clip_text_forward: the copy of the penultimate state failed");
        return -2;
    }
    d.layers = layers + (n_layers - 1); d.n_layers = 1;
    if ((rc = advgrpo_vit_forward(&d, vit_ws, vit_bytes, stream)) != 0) return rc;
    if ((rc = advgrpo_clip_eos_pool(ids, x, pooled, B, S, D, eos_token_id, stream)) != 0) return rc;
    if ((rc = advgrpo_layernorm_mod(pooled, D, pooled_n, nullptr, D, final_ln_w, final_ln_b, nullptr, nullptr, nullptr, nullptr, 0, 0, B, D, eps,
                                    stream)) != 0)
        return rc;
    return advgrpo_gemm_bf16(pooled_n, D, proj_w, D, text_embeds, ld_text_embeds, ADVGRPO_BF16, B, P, D, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, 0, 0,
                             0, 0, 0, 0, 0, 1, 0, 0, 0, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------- T5 encoder
extern "C" int64_t advgrpo_t5_workspace_bytes(int B, int S, int D, int H, int ff) {
    const int64_t M = (int64_t)B * S, inner = (int64_t)H * 64;
    return 2 * piece(M * D * 2) + piece(M * 3 * inner * 2) + piece(M * inner * 2) + 2 * piece(M * ff * 2) + piece((int64_t)H * S * S * 4);
}

extern "C" int advgrpo_t5_forward(const int64_t* ids, const void* emb, int vocab, const float* rel_table, int num_buckets, int max_distance,
                                  const void* const* weights, int n_layers, const void* final_ln_w, int B, int S, int D, int H, int d_kv, int ff,
                                  float eps, void* out, int* bad_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    ADVGRPO_CHECK(ids && emb && rel_table && (weights || n_layers == 0) && final_ln_w && out && workspace, "t5_forward: null argument");
    ADVGRPO_CHECK(B > 0 && S > 0 && D > 0 && H > 0 && ff > 0 && vocab > 0 && n_layers >= 0,
                  "t5_forward: bad shape (B=%d S=%d D=%d H=%d ff=%d vocab=%d layers=%d)", B, S, D, H, ff, vocab, n_layers);
    ADVGRPO_CHECK(d_kv == 64, "t5_forward: head dim %d (the attention with a score bias serves 64, T5 v1.1's d_kv)", d_kv);
    ADVGRPO_CHECK(num_buckets == 32 && max_distance == 128,
                  "t5_forward: only (num_buckets, max_distance) = (32, 128) is implemented, the T5 / T5 v1.1 encoders' (got %d, %d)", num_buckets,
                  max_distance);
    ADVGRPO_CHECK(workspace_bytes >= advgrpo_t5_workspace_bytes(B, S, D, H, ff) && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "t5_forward: workspace too small or not 256-byte aligned");
    const int M = B * S, inner = H * 64;
    Carver c{reinterpret_cast<char*>(workspace)};
    char* x = c.take((int64_t)M * D * 2);
    char* h = c.take((int64_t)M * D * 2);
    char* qkv = c.take((int64_t)M * 3 * inner * 2);
    char* o = c.take((int64_t)M * inner * 2);
    char* g = c.take((int64_t)M * ff * 2);
    char* u = c.take((int64_t)M * ff * 2);
    float* bias = reinterpret_cast<float*>(c.take((int64_t)H * S * S * 4));
    int rc;
    if ((rc = advgrpo_token_embed(ids, emb, nullptr, x, B, S, D, vocab, bad_ids, stream)) != 0) return rc;
    if ((rc = advgrpo_t5_position_bias(rel_table, bias, H, S, num_buckets, max_distance, stream)) != 0) return rc;
    const int64_t bs = (int64_t)S * 3 * inner;
    for (int l = 0; l < n_layers; ++l) {
        const void* const* W = weights + 7 * l;      // ln1, qkv, o, ln2, wi0, wi1, wo
        ADVGRPO_CHECK(W[0] && W[1] && W[2] && W[3] && W[4] && W[5] && W[6], "t5_forward: layer %d: a weight is missing", l);
        if ((rc = advgrpo_rmsnorm_rows(x, D, h, D, W[0], M, D, eps, stream)) != 0) return rc;
        if ((rc = advgrpo_gemm_bf16(h, D, W[1], D, qkv, 3 * inner, ADVGRPO_BF16, M, 3 * inner, D, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0,
                                    0, 0, 1, 0, 0, 0, stream)) != 0)
            return rc;
        if ((rc = advgrpo_attention_fwd_bias(qkv, qkv + (int64_t)inner * 2, qkv + (int64_t)2 * inner * 2, o, 3 * inner, 3 * inner, 3 * inner, inner, bs, bs,
                                             bs, (int64_t)S * inner, B, H, S, S, 64, 1.0f, 0, bias, stream)) != 0)
            return rc;
        if ((rc = advgrpo_gemm_bf16(o, inner, W[2], inner, x, D, ADVGRPO_BF16, M, D, inner, nullptr, 0, 1.0f, nullptr, 0, 0, x, D, 0, 0, 0, 0, 0, 0, 1, 0,
                                    0, 0, stream)) != 0)
            return rc;
        if ((rc = advgrpo_rmsnorm_rows(x, D, h, D, W[3], M, D, eps, stream)) != 0) return rc;
        if ((rc = advgrpo_gemm_bf16(h, D, W[4], D, g, ff, ADVGRPO_BF16, M, ff, D, nullptr, 1 /* GELU(tanh) */, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0,
                                    0, 0, 1, 0, 0, 0, stream)) != 0)
            return rc;
        if ((rc = advgrpo_gemm_bf16_train(h, D, W[5], D, u, ff, ADVGRPO_BF16, M, ff, D, nullptr, 7 /* mul_aux: y *= aux_in */, 1.0f, nullptr, 0, 0,
                                          nullptr, 0, nullptr, g, ff, 1, stream)) != 0)
            return rc;
        if ((rc = advgrpo_gemm_bf16(u, ff, W[6], ff, x, D, ADVGRPO_BF16, M, D, ff, nullptr, 0, 1.0f, nullptr, 0, 0, x, D, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0,
                                    stream)) != 0)
            return rc;
    }
    return advgrpo_rmsnorm_rows(x, D, out, D, final_ln_w, M, D, eps, stream);
}

// ------------------------------------------------------------------------------------------------------------------------- encode_prompt
extern "C" int64_t advgrpo_encode_prompt_workspace_bytes(int B, int S, int T, int Dl, int mlp_l, int Dg, int mlp_g, int Dt, int Ht, int ff) {
    const int64_t M = (int64_t)B * S;
    return piece(M * Dl * 2) + piece(M * Dg * 2) + piece((int64_t)B * T * Dt * 2) +
           max3(advgrpo_clip_text_workspace_bytes(B, S, Dl, mlp_l), advgrpo_clip_text_workspace_bytes(B, S, Dg, mlp_g),
                advgrpo_t5_workspace_bytes(B, T, Dt, Ht, ff));
}

extern "C" int advgrpo_encode_prompt(
    const int64_t* ids_l, const void* l_tok, const void* l_pos, int l_vocab, const advgrpo_vit_layer* l_layers, int l_n_layers, const void* l_ln_w,
    const void* l_ln_b, const void* l_proj, int Dl, int Hl, int mlp_l, int Pl, int act_l, int eos_l,
    const int64_t* ids_g, const void* g_tok, const void* g_pos, int g_vocab, const advgrpo_vit_layer* g_layers, int g_n_layers, const void* g_ln_w,
    const void* g_ln_b, const void* g_proj, int Dg, int Hg, int mlp_g, int Pg, int act_g, int eos_g, float clip_eps,
    const int64_t* ids_t5, const void* t_emb, int t_vocab, const float* rel_table, int num_buckets, int max_distance, const void* const* t_weights,
    int t_n_layers, const void* t_final_ln_w, int Dt, int Ht, int d_kv, int ff, float t5_eps,
    int B, int S, int T, void* prompt_embeds, void* pooled, int* bad_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    // everything the towers would refuse is refused here, before the first of them has launched anything
    ADVGRPO_CHECK(prompt_embeds && pooled && workspace && ids_l && l_tok && l_pos && l_layers && l_ln_w && l_ln_b && l_proj && ids_g && g_tok && g_pos &&
                      g_layers && g_ln_w && g_ln_b && g_proj && ids_t5 && t_emb && rel_table && (t_weights || t_n_layers == 0) && t_final_ln_w,
                  "encode_prompt: null argument");
    ADVGRPO_CHECK(B > 0 && S > 0 && T > 0 && Dl > 0 && Dg > 0 && Dt > 0 && Pl > 0 && Pg > 0 && Hl > 0 && Hg > 0 && Ht > 0 && mlp_l > 0 && mlp_g > 0 && ff > 0 &&
                      l_n_layers >= 1 && g_n_layers >= 1 && t_n_layers >= 0 && l_vocab > 0 && g_vocab > 0 && t_vocab > 0 && Dl % Hl == 0 && Dg % Hg == 0 && Pl % 8 == 0,
                  "encode_prompt: bad shape (B=%d S=%d T=%d Dl=%d Dg=%d Dt=%d Pl=%d Pg=%d)", B, S, T, Dl, Dg, Dt, Pl, Pg);
    ADVGRPO_CHECK(Dl / Hl == 64 && Dg / Hg == 64 && d_kv == 64, "encode_prompt: head dims %d, %d, %d (the three text towers have 64)", Dl / Hl, Dg / Hg,
                  d_kv);
    ADVGRPO_CHECK(num_buckets == 32 && max_distance == 128,
                  "encode_prompt: only (num_buckets, max_distance) = (32, 128) is implemented, the T5 / T5 v1.1 encoders' (got %d, %d)", num_buckets,
                  max_distance);
    ADVGRPO_CHECK(Dl + Dg <= Dt, "encode_prompt: the CLIP widths %d + %d exceed the T5 width %d", Dl, Dg, Dt);
    ADVGRPO_CHECK(workspace_bytes >= advgrpo_encode_prompt_workspace_bytes(B, S, T, Dl, mlp_l, Dg, mlp_g, Dt, Ht, ff) &&
                      (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "encode_prompt: workspace too small or not 256-byte aligned");
    const int64_t M = (int64_t)B * S;
    Carver c{reinterpret_cast<char*>(workspace)};
    char* pen_l = c.take(M * Dl * 2);
    char* pen_g = c.take(M * Dg * 2);
    char* t5 = c.take((int64_t)B * T * Dt * 2);
    char* tower_ws = c.w;                                   // the towers run one after the other on the stream and share it
    const int64_t tower_bytes = workspace_bytes - (tower_ws - reinterpret_cast<char*>(workspace));
    char* pooled_b = reinterpret_cast<char*>(pooled);       // [B, Pl + Pg]: each tower's projection writes its columns (pitch Pl + Pg)
    int rc;
    if ((rc = advgrpo_clip_text_forward(ids_l, l_tok, l_pos, l_vocab, l_layers, l_n_layers, l_ln_w, l_ln_b, l_proj, B, S, Dl, Hl, mlp_l, Pl, act_l,
                                        clip_eps, eos_l, pen_l, pooled_b, Pl + Pg, bad_ids, tower_ws, tower_bytes, stream)) != 0)
        return rc;
    if ((rc = advgrpo_clip_text_forward(ids_g, g_tok, g_pos, g_vocab, g_layers, g_n_layers, g_ln_w, g_ln_b, g_proj, B, S, Dg, Hg, mlp_g, Pg, act_g,
                                        clip_eps, eos_g, pen_g, pooled_b + (int64_t)Pl * 2, Pl + Pg, bad_ids, tower_ws, tower_bytes, stream)) != 0)
        return rc;
    if ((rc = advgrpo_t5_forward(ids_t5, t_emb, t_vocab, rel_table, num_buckets, max_distance, t_weights, t_n_layers, t_final_ln_w, B, T, Dt, Ht, d_kv,
                                 ff, t5_eps, t5, bad_ids, tower_ws, tower_bytes, stream)) != 0)
        return rc;
    return advgrpo_prompt_embeds_assemble(pen_l, Dl, pen_g, Dg, t5, prompt_embeds, B, S, T, Dt, stream);
}
