// qwen_sampler.hip -- Qwen-Image's norm-rescaled "true CFG" combine + the Euler ODE step of its flow-match scheduler (gfx950).
//
// Replaces the per-step tail of diffusers' QwenImagePipeline.__call__ (combine, two norms over the last axis of the packed
// [B, N_img, 64] latents, rescale) and FlowMatchEulerDiscreteScheduler.step (upcast, dt * v, add, cast back) -- about ten torch
// launches -- with one pass over HBM on the UNPACKED [B, C, H, W] tensors the transformer here returns.  PARITY UNPINNED: the
// rounding points are restated from the published pipeline (include/advgrpo.h has them), not checked against an installed diffusers
// (scripts/verify_against_diffusers.py does that where one exists).
//
// A token is one 2 x 2 patch across the C = 16 channels: in NCHW 16 planes x 2 rows x 2 adjacent pixels.  Work split: lane = token
// (or two x-adjacent tokens when W % 4 == 0: 8 B per lane per bf16 load, 16 B per f32 load), wave w of the 4 in a block = channels
// 4w .. 4w+3.  So every load / store instruction of a wave covers 64 lanes x 2 (or 4) consecutive pixels of ONE row of ONE plane:
// contiguous (up to the wrap at a row end).  The two sums of squares of a token are four lane-private partials (one per wave,
// 16 values each, added in the order channel, row, pixel) that meet in LDS and are added in wave order 0..3 by every wave: a
// fixed order, bit-reproducible run to run and the same in both lane layouts.  The combined prediction stays in registers between
// the norm and the step, so each input is read once.
//
// Built with -ffp-contract=off: every torch op of the restatement is one rounding here too.
#include "qwen_token.hpp"

namespace advgrpo {

// TPL = tokens per lane (1, or 2 x-adjacent ones).  `units` = B * (H/2) * (W/2 / TPL) lanes of work; x and out may alias.
template <int TPL>
__global__ __launch_bounds__(QS_THREADS) void qwen_cfg_euler_kernel(
    const void* __restrict__ v_neg, const void* __restrict__ v_pos, int v_dt, float scale, const void* x, int x_dt,
    const float* __restrict__ sigma, const float* __restrict__ sigma_next, int sigma_stride, void* out, int C, int H, int W,
    int64_t units) {
    constexpr int N = 2 * TPL;                      // elements per load: the row segment of TPL tokens
    __shared__ float part[2][QS_WAVES][QS_LANES * TPL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t u = (int64_t)blockIdx.x * QS_LANES + lane;
    const bool valid = u < units;
    const bool has_cfg = v_pos != nullptr, bf = v_dt == ADVGRPO_BF16;
    const int64_t plane = (int64_t)H * W;
    int64_t base = 0;
    float dt = 0.f;
    if (valid) {
        const int upr = (W / 2) / TPL, hh = H / 2;  // lanes per token row, token rows
        const int ux = (int)(u % upr);
        const int64_t r = u / upr;
        const int ty = (int)(r % hh), b = (int)(r / hh);
        base = (((int64_t)b * C + w * QS_CPW) * H + 2 * ty) * W + (int64_t)ux * N;
        dt = sigma_next[(int64_t)b * sigma_stride] - sigma[(int64_t)b * sigma_stride];
        if (bf) dt = round_bf16(dt);                // torch casts the 0-dim f32 dt to the tensor's dtype before it multiplies
    }
    float o[QS_CPW * 2][N];                         // the combined prediction, then the rescaled one
    float sp[TPL], sc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) sp[t] = sc[t] = 0.f;
    if (valid) {
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k) {      // k = channel * 2 + row
            const int64_t off = base + (k >> 1) * plane + (k & 1) * W;
            float ng[N], ps[N];
            qs_load<N>(v_neg, v_dt, off, ng);
            if (has_cfg) {
                qs_load<N>(v_pos, v_dt, off, ps);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    float d = ps[j] - ng[j];
                    if (bf) d = round_bf16(d);
                    float m = scale * d;
                    if (bf) m = round_bf16(m);
                    float c = ng[j] + m;
                    if (bf) c = round_bf16(c);
                    o[k][j] = c;
                    sp[j >> 1] += ps[j] * ps[j];
                    sc[j >> 1] += c * c;
                }
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) o[k][j] = ng[j];
            }
        }
    }
    if (has_cfg) {                                  // (uniform over the block: every wave reaches the barrier)
#pragma unroll
        for (int t = 0; t < TPL; ++t) {
            part[0][w][lane * TPL + t] = sp[t];
            part[1][w][lane * TPL + t] = sc[t];
        }
        __syncthreads();
        float ratio[TPL];
#pragma unroll
        for (int t = 0; t < TPL; ++t) {
            float p = 0.f, c = 0.f;
#pragma unroll
            for (int i = 0; i < QS_WAVES; ++i) {
                p += part[0][i][lane * TPL + t];
                c += part[1][i][lane * TPL + t];
            }
            float cn = sqrtf(p), nn = sqrtf(c);
            if (bf) { cn = round_bf16(cn); nn = round_bf16(nn); }
            float q = cn / nn;                      // no epsilon: an all-zero token is 0 * inf or 0 / 0 = NaN, as in the pipeline
            if (bf) q = round_bf16(q);
            ratio[t] = q;
        }
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float v = o[k][j] * ratio[j >> 1];
                if (bf) v = round_bf16(v);
                o[k][j] = v;
            }
    }
    if (valid) {
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k) {
            const int64_t off = base + (k >> 1) * plane + (k & 1) * W;
            float xs[N], nx[N];
            qs_load<N>(x, x_dt, off, xs);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float s = dt * o[k][j];             // ... and the product is a bf16 tensor
                if (bf) s = round_bf16(s);
                nx[j] = xs[j] + s;                  // the scheduler's f32 sample
            }
            qs_store<N>(out, x_dt, off, nx);
        }
    }
}

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_qwen_cfg_euler_step(const void* v_neg, const void* v_pos, int v_dtype, float true_cfg_scale,
                                           const void* sample, int sample_dtype, const float* sigma, const float* sigma_next,
                                           int sigma_stride, void* prev_sample, int B, int C, int H, int W, int patch_size,
                                           void* stream) {
    ADVGRPO_CHECK(v_dtype == ADVGRPO_F32 || v_dtype == ADVGRPO_BF16, "qwen_cfg_euler_step: bad v_dtype %d", v_dtype);
    ADVGRPO_CHECK(sample_dtype == ADVGRPO_F32 || sample_dtype == ADVGRPO_BF16, "qwen_cfg_euler_step: bad sample_dtype %d", sample_dtype);
    ADVGRPO_CHECK(v_neg && sample && sigma && sigma_next && prev_sample, "qwen_cfg_euler_step: null argument");
    ADVGRPO_CHECK(patch_size == 2 && C == QS_CPW * QS_WAVES, "qwen_cfg_euler_step: built for patch 2 and C = %d (patch=%d C=%d)",
                  QS_CPW * QS_WAVES, patch_size, C);
    ADVGRPO_CHECK(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && sigma_stride >= 0,
                  "qwen_cfg_euler_step: need B>0 and even H, W (B=%d H=%d W=%d)", B, H, W);
    const int vs = dtype_size(v_dtype), xs = dtype_size(sample_dtype);
    auto aligned = [&](int elems) {
        const uintptr_t v = (uintptr_t)v_neg | (uintptr_t)v_pos, s = (uintptr_t)sample | (uintptr_t)prev_sample;
        return v % (uintptr_t)(elems * vs) == 0 && s % (uintptr_t)(elems * xs) == 0;
    };
    ADVGRPO_CHECK(aligned(2), "qwen_cfg_euler_step: tensors must be aligned to two of their elements");
    const bool pair = W % 4 == 0 && aligned(4);
    const int64_t units = (int64_t)B * (H / 2) * (W / 2 / (pair ? 2 : 1));
    const int64_t blocks = (units + QS_LANES - 1) / QS_LANES;
    ADVGRPO_CHECK(blocks <= INT32_MAX, "qwen_cfg_euler_step: too many tokens");
    if (pair) {
        hipLaunchKernelGGL(qwen_cfg_euler_kernel<2>, dim3((unsigned)blocks), dim3(QS_THREADS), 0, as_stream(stream), v_neg, v_pos,
                           v_dtype, true_cfg_scale, sample, sample_dtype, sigma, sigma_next, sigma_stride, prev_sample, C, H, W, units);
    } else {
        hipLaunchKernelGGL(qwen_cfg_euler_kernel<1>, dim3((unsigned)blocks), dim3(QS_THREADS), 0, as_stream(stream), v_neg, v_pos,
                           v_dtype, true_cfg_scale, sample, sample_dtype, sigma, sigma_next, sigma_stride, prev_sample, C, H, W, units);
    }
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
