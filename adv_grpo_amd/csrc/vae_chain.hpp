// vae_chain.hpp -- host sequencing shared by the VAE decoder (vae_decode.cpp) and encoder (vae_encode.cpp) chains: the mid block's
// single-head attention.  Host-only code: it only calls this library's own C entries.
#pragma once
#include <math.h>

#include "common.hpp"

namespace advgrpo {
namespace vae_chain {

inline int64_t piece(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// scratch bytes of vae_mid_attention without / with the score matrix
inline int64_t attn_rest_bytes(int64_t B, int64_t T, int64_t C) {
    return piece(B * T * 3 * C * 2) * 4          // h3, q3, k3, o3
           + piece(B * T * C * 4) * 4            // q, k, o, y
           + piece(B * C * T * 4) + piece(B * C * 3 * T * 2)   // vt, vt3
           + piece(B * T * 3 * T * 2);           // p3
}
inline int64_t attn_s_bytes(int64_t B, int64_t T) { return piece(B * T * T * 4); }

// Single-head attention over the T = H W pixels of x [B, H, W, C] f32 (diffusers' Attention of the VAE mid block: GroupNorm, q / k / v, softmax,
// out projection, + x), every product on split-bf16 operands, f32 in between (vae.py: _attn3_core).  `d` supplies attn_* and groups; `scratch`
// holds attn_rest_bytes (+ attn_s_bytes when `s` is null: the score matrix is then carved between vt3 and p3); out must not alias x.
inline int vae_mid_attention(const advgrpo_vae_decoder_desc& d, int B, int H, int W, int C, const float* x, float* out, char* scratch, float* s,
                             double* gn, void* stream) {
    int rc;
    const int G = d.groups;
    const int64_t T = (int64_t)H * W, M = B * T;
    char* a = scratch;
    auto tk = [&](int64_t bytes) { char* p = a; a += piece(bytes); return p; };
    char* h3 = tk(M * 3 * C * 2); char* q3 = tk(M * 3 * C * 2); char* k3 = tk(M * 3 * C * 2); char* o3 = tk(M * 3 * C * 2);
    float* q = reinterpret_cast<float*>(tk(M * C * 4)); float* k = reinterpret_cast<float*>(tk(M * C * 4));
    float* o = reinterpret_cast<float*>(tk(M * C * 4)); float* y = reinterpret_cast<float*>(tk(M * C * 4));
    float* vt = reinterpret_cast<float*>(tk((int64_t)B * C * T * 4)); char* vt3 = tk((int64_t)B * C * 3 * T * 2);
    if (!s) s = reinterpret_cast<float*>(tk((int64_t)B * T * T * 4));
    char* p3 = tk((int64_t)B * T * 3 * T * 2);
    auto gemm_f32 = [&](const void* A, int64_t lda, const void* Wt, int64_t ldw, float* Cc, int64_t ldc, int Mm, int N, int K, float alpha, int batch,
                        int64_t sA, int64_t sW, int64_t sC) {
        return advgrpo_gemm_bf16(A, lda, Wt, ldw, Cc, ldc, ADVGRPO_F32, Mm, N, K, nullptr, 0, alpha, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, batch, sA, sW, sC,
                                 stream);
    };
    if ((rc = advgrpo_groupnorm_nhwc_x3(x, h3, gn, d.attn_norm_w, d.attn_norm_b, B, (int)T, C, G, 1e-6f, 0, 0, stream)) != 0) return rc;
    if ((rc = gemm_f32(h3, 3 * C, d.attn_q_w, 3 * C, q, C, (int)M, C, 3 * C, 1.0f, 1, 0, 0, 0)) != 0) return rc;
    if ((rc = advgrpo_split_bf16x3(q, d.attn_q_b, q3, M, C, 0, stream)) != 0) return rc;
    if ((rc = gemm_f32(h3, 3 * C, d.attn_k_w, 3 * C, k, C, (int)M, C, 3 * C, 1.0f, 1, 0, 0, 0)) != 0) return rc;
    if ((rc = advgrpo_split_bf16x3(k, d.attn_k_b, k3, M, C, 1, stream)) != 0) return rc;
    // V^T[b] = Wv . h[b]^T (the bias is added after P . V: rows of P sum to one); the weight is the [hi | lo | hi] side
    if ((rc = gemm_f32(d.attn_v_w, 3 * C, h3, 3 * C, vt, T, C, (int)T, 3 * C, 1.0f, B, 0, T * 3 * C, (int64_t)C * T)) != 0) return rc;
    if ((rc = advgrpo_split_bf16x3(vt, nullptr, vt3, (int64_t)B * C, (int)T, 1, stream)) != 0) return rc;
    if ((rc = gemm_f32(q3, 3 * C, k3, 3 * C, s, T, (int)T, (int)T, 3 * C, (float)pow((double)C, -0.5), B, T * 3 * C, T * 3 * C, T * T)) != 0) return rc;
    if ((rc = advgrpo_softmax_rows_x3(s, p3, M, (int)T, stream)) != 0) return rc;
    if ((rc = gemm_f32(p3, 3 * T, vt3, 3 * T, o, C, (int)T, C, (int)(3 * T), 1.0f, B, T * 3 * T, (int64_t)C * 3 * T, T * C)) != 0) return rc;
    if ((rc = advgrpo_split_bf16x3(o, d.attn_v_b, o3, M, C, 0, stream)) != 0) return rc;
    if ((rc = gemm_f32(o3, 3 * C, d.attn_o_w, 3 * C, y, C, (int)M, C, 3 * C, 1.0f, 1, 0, 0, 0)) != 0) return rc;
    return advgrpo_add_rows_f32(y, x, d.attn_o_b, out, M, C, stream);
}

}  // namespace vae_chain
}  // namespace advgrpo
