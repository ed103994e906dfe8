// qwen_token.hpp -- the token layout of the Qwen-Image kernels on UNPACKED [B, 16, H, W] tensors, shared by qwen_sampler.hip (the
// deterministic true-CFG Euler step) and sde_step.hip (the norm-rescaled true CFG in front of the stochastic steps).
//
// A token is one 2 x 2 patch across the C = 16 channels: in NCHW 16 planes x 2 rows x 2 adjacent pixels.  Work split: lane = token
// (or two x-adjacent tokens when W % 4 == 0: 8 B per lane per bf16 load, 16 B per f32 load), wave w of the 4 in a block = channels
// 4w .. 4w+3.  So every load / store instruction of a wave covers 64 lanes x 2 (or 4) consecutive pixels of ONE row of ONE plane.
#pragma once
#include "common.hpp"

namespace advgrpo {

constexpr int QS_LANES = 64;                       // tokens (or token pairs) per block
constexpr int QS_WAVES = 4;
constexpr int QS_THREADS = QS_LANES * QS_WAVES;
constexpr int QS_CPW = 4;                          // channels per wave: C = 16

template <int N>   // N = 2 or 4 consecutive elements, aligned to their total size
__device__ __forceinline__ void qs_load(const void* p, int dt, int64_t i, float o[N]) {
    if (dt == ADVGRPO_BF16) {
        const bf16_t* q = reinterpret_cast<const bf16_t*>(p) + i;
        uint32_t w[N / 2];
        if constexpr (N == 2) {
            w[0] = *reinterpret_cast<const uint32_t*>(q);
        } else {
            const uint2 r = *reinterpret_cast<const uint2*>(q);
            w[0] = r.x; w[1] = r.y;
        }
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            o[2 * k] = bf2f((bf16_t)(w[k] & 0xffffu));
            o[2 * k + 1] = bf2f((bf16_t)(w[k] >> 16));
        }
    } else {
        const float* q = reinterpret_cast<const float*>(p) + i;
        if constexpr (N == 2) {
            const float2 r = *reinterpret_cast<const float2*>(q);
            o[0] = r.x; o[1] = r.y;
        } else {
            const float4 r = *reinterpret_cast<const float4*>(q);
            o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
        }
    }
}
template <int N>
__device__ __forceinline__ void qs_store(void* p, int dt, int64_t i, const float o[N]) {
    if (dt == ADVGRPO_BF16) {
        bf16_t* q = reinterpret_cast<bf16_t*>(p) + i;
        uint32_t w[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) w[k] = (uint32_t)f2bf(o[2 * k]) | ((uint32_t)f2bf(o[2 * k + 1]) << 16);
        if constexpr (N == 2) *reinterpret_cast<uint32_t*>(q) = w[0];
        else *reinterpret_cast<uint2*>(q) = make_uint2(w[0], w[1]);
    } else {
        float* q = reinterpret_cast<float*>(p) + i;
        if constexpr (N == 2) *reinterpret_cast<float2*>(q) = make_float2(o[0], o[1]);
        else *reinterpret_cast<float4*>(q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

}  // namespace advgrpo
