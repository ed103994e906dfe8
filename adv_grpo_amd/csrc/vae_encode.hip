// vae_encode.hip -- the two ends of the SD3 VAE encoder (gfx950): pixels -> conv_in's operand rows, moments -> latents.
//
// Stands in for `transforms.Normalize([0.5], [0.5])` + the layout change in front of `pipe.vae.encode(img)` and for
// `.latent_dist.sample() * scaling_factor` + `.to(bfloat16)` behind it (adv_grpo/diffusers_patch/sd3_pipeline_with_logprob_fast.py:691-705),
// and optionally for the forward noising of flux_to_sd3_denoise_random (:961-965) in the same launch.
//   image_to_nhwc_x3   [B,3,H,W] in [0,1] (f32 / bf16, NCHW) or uint8 [B,H,W,3] -> (x - 0.5) / 0.5 -> split-bf16 rows [B,H,W,3*Cpad]
//                      ([hi | unwritten | lo]; channels 3 .. Cpad-1 zero): the operand of conv_in on the 128-wide convolution kernel
//   vae_latent_tail    moments NHWC f32 [B,h,w,2C] -> mean, logvar = clamp(logvar, -30, 20), std = exp(0.5 logvar), z = mean + std * eps,
//                      z * scaling_factor, cast, NCHW; optionally mix = (1 - sigma) * bf16(z) + sigma * noise in bf16 arithmetic
// Built with -ffp-contract=off: every torch op of the reference is one f32 (or bf16) rounding here too.  The tail does NOT subtract
// shift_factor: image_to_latent does not (PF:704).
#include "common.hpp"

namespace advgrpo {

__global__ __launch_bounds__(256) void image_to_nhwc_x3_kernel(const void* __restrict__ img, int dt, bf16_t* __restrict__ out, int B, int H, int W,
                                                               int Cpad) {
    const int chunks = Cpad / 8;
    const int64_t total = (int64_t)B * H * W * chunks, hw = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / chunks;
        const int ch = (int)(i - pix * chunks);
        uint4 hi = make_uint4(0, 0, 0, 0), lo = hi;
        if (ch == 0) {
            const int64_t b = pix / hw, r = pix - b * hw;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x;
                if (dt == ADVGRPO_U8) x = (float)reinterpret_cast<const uint8_t*>(img)[pix * 3 + c] / 255.0f;     // ToTensor
                else if (dt == ADVGRPO_BF16) x = bf2f(reinterpret_cast<const bf16_t*>(img)[(b * 3 + c) * hw + r]);
                else x = reinterpret_cast<const float*>(img)[(b * 3 + c) * hw + r];
                v[c] = (x - 0.5f) / 0.5f;                                                                         // Normalize([0.5], [0.5])
            }
            uint16_t h[3], l[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                h[c] = f2bf(v[c]);
                l[c] = f2bf(v[c] - bf2f(h[c]));
            }
            hi.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16); hi.y = h[2];
            lo.x = (uint32_t)l[0] | ((uint32_t)l[1] << 16); lo.y = l[2];
        }
        bf16_t* row = out + pix * 3 * Cpad + ch * 8;
        *reinterpret_cast<uint4*>(row) = hi;
        *reinterpret_cast<uint4*>(row + 2 * Cpad) = lo;
    }
}

// one thread per four consecutive NCHW latent elements = one Philox block (the (seed, offset) convention of advgrpo_randn: element i takes
// value i % 4 of counter offset + i / 4)
__global__ __launch_bounds__(256) void vae_latent_tail_kernel(const float* __restrict__ mom, int B, int C, int h, int w, int mode,
                                                              const float* __restrict__ eps, uint64_t seed, uint64_t offset, float scaling,
                                                              void* __restrict__ z_out, int z_dt, int mix_mode, const void* __restrict__ noise,
                                                              int noise_dt, uint64_t mix_seed, uint64_t mix_offset,
                                                              const float* __restrict__ sigma, bf16_t* __restrict__ mix_out) {
    const int64_t n = (int64_t)B * C * h * w, groups = (n + 3) / 4;
    const Philox ph(seed), phm(mix_seed);
    float sg = 0.f, om = 0.f;
    if (mix_mode) {
        sg = round_bf16(sigma[0]);             // the scheduler's sigma in the latent dtype (get_sigmas(..., dtype=bf16))
        om = round_bf16(1.0f - sg);            // (1.0 - sigmas): one bf16 op
    }
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        float e[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (mode == 2) philox_normal4(ph, offset + (uint64_t)g, e);
        if (mix_mode == 2) philox_normal4(phm, mix_offset + (uint64_t)g, nz);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = g * 4 + k;
            if (i >= n) break;
            const int x = (int)(i % w);
            const int y = (int)((i / w) % h);
            const int c = (int)((i / ((int64_t)w * h)) % C);
            const int64_t b = i / ((int64_t)w * h * C);
            const float* m = mom + ((b * h + y) * w + x) * 2 * C;
            const float mean = m[c];
            float z = mean;
            if (mode != 0) {
                const float lv = fminf(fmaxf(m[C + c], -30.0f), 20.0f);
                const float sd = expf(0.5f * lv);
                const float ee = mode == 1 ? eps[i] : e[k];
                z = mean + sd * ee;
            }
            z = z * scaling;
            if (z_out) {
                if (z_dt == ADVGRPO_BF16) reinterpret_cast<bf16_t*>(z_out)[i] = f2bf(z);
                else reinterpret_cast<float*>(z_out)[i] = z;
            }
            if (mix_mode) {
                float nv = nz[k];
                if (mix_mode == 1) nv = noise_dt == ADVGRPO_BF16 ? bf2f(reinterpret_cast<const bf16_t*>(noise)[i]) : reinterpret_cast<const float*>(noise)[i];
                nv = round_bf16(nv);                                   // randn_like(bf16 latents)
                const float a = round_bf16(om * round_bf16(z));        // (1 - sigma) * latent
                const float bq = round_bf16(sg * nv);                  // sigma * noise
                mix_out[i] = f2bf(a + bq);
            }
        }
    }
}

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_image_to_nhwc_x3(const void* image, int image_dtype, void* out3, int B, int H, int W, int Cpad, void* stream) {
    ADVGRPO_CHECK(image && out3, "image_to_nhwc_x3: null pointer");
    ADVGRPO_CHECK(image_dtype == ADVGRPO_F32 || image_dtype == ADVGRPO_BF16 || image_dtype == ADVGRPO_U8, "image_to_nhwc_x3: bad dtype %d", image_dtype);
    ADVGRPO_CHECK(B > 0 && H > 0 && W > 0 && Cpad >= 8 && Cpad % 8 == 0, "image_to_nhwc_x3: bad shape (B=%d H=%d W=%d Cpad=%d)", B, H, W, Cpad);
    const int64_t total = (int64_t)B * H * W * (Cpad / 8);
    const int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(image_to_nhwc_x3_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), image, image_dtype, (bf16_t*)out3, B, H, W, Cpad);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_vae_latent_tail(const float* moments, int B, int C, int h, int w, int mode, const float* eps, uint64_t seed, uint64_t offset,
                                       float scaling_factor, void* z_out, int z_dtype, int mix_mode, const void* mix_noise, int mix_noise_dtype,
                                       uint64_t mix_seed, uint64_t mix_offset, const float* sigma, void* mix_out, void* stream) {
    ADVGRPO_CHECK(moments && (z_out || mix_out), "vae_latent_tail: null pointer");
    ADVGRPO_CHECK(B > 0 && C > 0 && h > 0 && w > 0, "vae_latent_tail: bad shape (B=%d C=%d h=%d w=%d)", B, C, h, w);
    ADVGRPO_CHECK(mode >= 0 && mode <= 2 && (mode != 1 || eps), "vae_latent_tail: mode must be 0 (mean), 1 (eps given) or 2 (Philox), got %d", mode);
    ADVGRPO_CHECK(!z_out || z_dtype == ADVGRPO_F32 || z_dtype == ADVGRPO_BF16, "vae_latent_tail: bad latent dtype %d", z_dtype);
    ADVGRPO_CHECK(mix_mode >= 0 && mix_mode <= 2, "vae_latent_tail: mix_mode must be 0 (none), 1 (noise given) or 2 (Philox), got %d", mix_mode);
    ADVGRPO_CHECK(!mix_mode || (sigma && mix_out && (mix_mode != 1 || (mix_noise && (mix_noise_dtype == ADVGRPO_F32 || mix_noise_dtype == ADVGRPO_BF16)))),
                  "vae_latent_tail: the noising needs sigma, an output and (mix_mode 1) f32 / bf16 noise");
    const int64_t groups = ((int64_t)B * C * h * w + 3) / 4;
    const int blocks = (int)std::min<int64_t>((groups + 255) / 256, 2048);
    hipLaunchKernelGGL(vae_latent_tail_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), moments, B, C, h, w, mode, eps, seed, offset, scaling_factor,
                       z_out, z_dtype, mix_mode, mix_noise, mix_noise_dtype, mix_seed, mix_offset, sigma, (bf16_t*)mix_out);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
