// qwen_text_encoder.cpp -- the Qwen2.5-VL language model on text-only input (the prompt encoder of Qwen-Image, BASELINE config 5) behind one
// C-ABI entry: what QwenImagePipeline._get_qwen_prompt_embeds computes after tokenisation, up to hidden_states[-1].
//
// Until now the launch order of this tower lived in Python (adv_grpo_amd/qwen_text_encoder.py) and its attention step was torch indexing
// around two batched GEMMs; qwen_text.hip has that indexing as kernels, attention_gqa.hip has the fused kernel, and this file is the order:
//   token embedding, then per layer: RMSNorm -> q | k | v GEMM with bias -> rotate_half rotary on the query and key heads in place ->
//   attention -> out-proj + residual -> RMSNorm -> gate with SiLU -> up times that gate (mul_aux epilogue) -> down + residual; final RMSNorm
// attention_mode 0 (materialised): pack -> scores (batched GEMM, f32) -> causal softmax rows -> P V (batched GEMM) -> unpack: the same
//   kernels, in the same order, with the same epilogues as the Python sequencing, which stays as the check -- bit-identical
//   (tests/test_gpu_qwen_text_entry.py).  T <= 512 (advgrpo_softmax_rows_causal).
// attention_mode 1 (fused): advgrpo_attention_fwd_gqa on the q | k | v buffer in place; head_dim 128 only.
// No allocation, no synchronisation, no host <-> device copy: the entry can be captured in a graph.  Host-only code.
#include <cmath>

#include "common.hpp"

using namespace advgrpo;

namespace {
inline int64_t piece(int64_t bytes) { return (bytes + 255) / 256 * 256; }
struct Carver {      // hands out 256-byte aligned pieces of the caller's workspace, in the order the size function adds them up
    char* w;
    char* take(int64_t bytes) { char* p = w; w += piece(bytes); return p; }
};
constexpr int QWEN_MAX_ROWS = 1 << 20;      // B * T of either mode: row counts and grids of every launch stay far inside 32 bits
}  // namespace

extern "C" int64_t advgrpo_qwen_text_workspace_bytes(int B, int T, int D, int H, int KV, int head_dim, int ff, int attention_mode) {
    if (B <= 0 || T <= 0 || D <= 0 || H <= 0 || KV <= 0 || head_dim <= 0 || ff <= 0 || (attention_mode != 0 && attention_mode != 1)) return 0;
    const int64_t M = (int64_t)B * T, inner = (int64_t)H * head_dim, W = (int64_t)(H + 2 * KV) * head_dim;
    int64_t n = 2 * piece(M * D * 2) + piece(M * W * 2) + piece(M * inner * 2) + 2 * piece(M * ff * 2);      // x, h, qkv, o, g, u
    if (attention_mode == 0) {
        const int64_t Tp = (T + 63) / 64 * 64, BH = (int64_t)B * H;
        n += 3 * piece(BH * Tp * head_dim * 2) + piece(BH * Tp * Tp * 4) + piece(BH * Tp * Tp * 2) + piece(BH * Tp * head_dim * 2);   // q, k, v^T, scores, P, o
    }
    return n;
}

extern "C" int advgrpo_qwen_text_forward(const int64_t* ids, const void* emb, int vocab, const void* const* weights, int n_layers, const void* final_w,
                                         const float* cos_sin, int B, int T, int D, int H, int KV, int head_dim, int ff, float eps, int attention_mode,
                                         void* out, int* bad_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    ADVGRPO_CHECK(ids, "qwen_text_forward: null pointer (ids)");
    ADVGRPO_CHECK(emb, "qwen_text_forward: null pointer (emb)");
    ADVGRPO_CHECK(weights || n_layers == 0, "qwen_text_forward: null pointer (weights)");
    ADVGRPO_CHECK(final_w, "qwen_text_forward: null pointer (final_w)");
    ADVGRPO_CHECK(cos_sin, "qwen_text_forward: null pointer (cos_sin)");
    ADVGRPO_CHECK(out, "qwen_text_forward: null pointer (out)");
    ADVGRPO_CHECK(workspace, "qwen_text_forward: null pointer (workspace)");
    ADVGRPO_CHECK(attention_mode == 0 || attention_mode == 1, "qwen_text_forward: unknown attention_mode %d (0 materialised, 1 fused)", attention_mode);
    ADVGRPO_CHECK(B > 0 && T > 0 && D > 0 && H > 0 && KV > 0 && head_dim > 0 && ff > 0 && vocab > 0 && n_layers >= 0,
                  "qwen_text_forward: bad shape (B=%d T=%d D=%d H=%d KV=%d head_dim=%d ff=%d vocab=%d layers=%d)", B, T, D, H, KV, head_dim, ff, vocab,
                  n_layers);
    ADVGRPO_CHECK(H % KV == 0, "qwen_text_forward: %d query heads are not a multiple of %d key/value heads", H, KV);
    ADVGRPO_CHECK(attention_mode == 1 ? head_dim == 128 : head_dim % 64 == 0,
                  "qwen_text_forward: head_dim %d not supported (fused: 128; materialised: a multiple of 64)", head_dim);
    ADVGRPO_CHECK(attention_mode == 1 || T <= 512, "qwen_text_forward: the materialised attention holds prompts of up to 512 tokens (got %d); attention_mode 1 has no such cap",
                  T);
    ADVGRPO_CHECK((int64_t)B * T <= QWEN_MAX_ROWS, "qwen_text_forward: B * T = %lld exceeds %d rows", (long long)B * T, QWEN_MAX_ROWS);
    ADVGRPO_CHECK(D % 64 == 0 && ff % 64 == 0 && D <= 4096, "qwen_text_forward: D and ff must be multiples of 64 and D <= 4096 (D=%d ff=%d)", D, ff);
    ADVGRPO_CHECK(workspace_bytes >= advgrpo_qwen_text_workspace_bytes(B, T, D, H, KV, head_dim, ff, attention_mode) &&
                      (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
                  "qwen_text_forward: workspace too small or not 256-byte aligned");
    for (int l = 0; l < n_layers; ++l)
        for (int i = 0; i < 8; ++i) ADVGRPO_CHECK(weights[8 * l + i], "qwen_text_forward: layer %d: weight %d is missing", l, i);

    const int M = B * T, inner = H * head_dim, W = (H + 2 * KV) * head_dim, Tp = (T + 63) / 64 * 64, BH = B * H;
    Carver c{reinterpret_cast<char*>(workspace)};
    char* x = c.take((int64_t)M * D * 2);
    char* h = c.take((int64_t)M * D * 2);
    char* qkv = c.take((int64_t)M * W * 2);
    char* o = c.take((int64_t)M * inner * 2);
    char* g = c.take((int64_t)M * ff * 2);
    char* u = c.take((int64_t)M * ff * 2);
    char *qh = nullptr, *kh = nullptr, *vt = nullptr, *sc = nullptr, *p16 = nullptr, *oh = nullptr;
    if (attention_mode == 0) {
        qh = c.take((int64_t)BH * Tp * head_dim * 2);
        kh = c.take((int64_t)BH * Tp * head_dim * 2);
        vt = c.take((int64_t)BH * Tp * head_dim * 2);
        sc = c.take((int64_t)BH * Tp * Tp * 4);
        p16 = c.take((int64_t)BH * Tp * Tp * 2);
        oh = c.take((int64_t)BH * Tp * head_dim * 2);
    }
    const float scale = (float)std::pow((double)head_dim, -0.5);
    int rc;
    if ((rc = advgrpo_token_embed(ids, emb, nullptr, x, B, T, D, vocab, bad_ids, stream)) != 0) return rc;
    for (int l = 0; l < n_layers; ++l) {
        const void* const* Wl = weights + 8 * l;      // ln1, qkv.w, qkv.b, o, ln2, gate, up, down
        if ((rc = advgrpo_rmsnorm_rows(x, D, h, D, Wl[0], M, D, eps, stream)) != 0) return rc;
        if ((rc = advgrpo_gemm_bf16(h, D, Wl[1], D, qkv, W, ADVGRPO_BF16, M, W, D, Wl[2], 0, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0,
                                    stream)) != 0)
            return rc;
        if ((rc = advgrpo_rope_half(qkv, W, M, T, 0, H + KV, head_dim, cos_sin, stream)) != 0) return rc;
        if (attention_mode == 0) {
            if ((rc = advgrpo_gqa_pack_heads(qkv, W, qh, kh, vt, B, T, H, KV, head_dim, stream)) != 0) return rc;
            if ((rc = advgrpo_gemm_bf16(qh, head_dim, kh, head_dim, sc, Tp, ADVGRPO_F32, Tp, Tp, head_dim, nullptr, 0, scale, nullptr, 0, 0, nullptr, 0, 0, 0,
                                        0, 0, 0, 0, BH, (int64_t)Tp * head_dim, (int64_t)Tp * head_dim, (int64_t)Tp * Tp, stream)) != 0)
                return rc;
            if ((rc = advgrpo_softmax_rows_causal(reinterpret_cast<const float*>(sc), p16, (int64_t)BH * Tp, Tp, stream)) != 0) return rc;
            if ((rc = advgrpo_gemm_bf16(p16, Tp, vt, Tp, oh, head_dim, ADVGRPO_BF16, Tp, head_dim, Tp, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0,
                                        0, 0, BH, (int64_t)Tp * Tp, (int64_t)head_dim * Tp, (int64_t)Tp * head_dim, stream)) != 0)
                return rc;
            if ((rc = advgrpo_gqa_unpack_heads(oh, o, B, T, H, head_dim, stream)) != 0) return rc;
        } else {
            if ((rc = advgrpo_attention_fwd_gqa(qkv, qkv + (int64_t)inner * 2, qkv + (int64_t)(inner + KV * head_dim) * 2, o, W, W, W, inner, (int64_t)T * W,
                                                (int64_t)T * W, (int64_t)T * W, (int64_t)T * inner, B, H, KV, T, head_dim, scale, 1, stream)) != 0)
                return rc;
        }
        if ((rc = advgrpo_gemm_bf16(o, inner, Wl[3], inner, x, D, ADVGRPO_BF16, M, D, inner, nullptr, 0, 1.0f, nullptr, 0, 0, x, D, 0, 0, 0, 0, 0, 0, 1, 0, 0,
                                    0, stream)) != 0)
            return rc;
        if ((rc = advgrpo_rmsnorm_rows(x, D, h, D, Wl[4], M, D, eps, stream)) != 0) return rc;
        if ((rc = advgrpo_gemm_bf16(h, D, Wl[5], D, g, ff, ADVGRPO_BF16, M, ff, D, nullptr, 3 /* SiLU */, 1.0f, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, 1,
                                    0, 0, 0, stream)) != 0)
            return rc;
        if ((rc = advgrpo_gemm_bf16_train(h, D, Wl[6], D, u, ff, ADVGRPO_BF16, M, ff, D, nullptr, 7 /* mul_aux: y *= aux_in */, 1.0f, nullptr, 0, 0, nullptr,
                                          0, nullptr, g, ff, 1, stream)) != 0)
            return rc;
        if ((rc = advgrpo_gemm_bf16(u, ff, Wl[7], ff, x, D, ADVGRPO_BF16, M, D, ff, nullptr, 0, 1.0f, nullptr, 0, 0, x, D, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0,
                                    stream)) != 0)
            return rc;
    }
    return advgrpo_rmsnorm_rows(x, D, out, D, final_w, M, D, eps, stream);
}
