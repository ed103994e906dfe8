// preprocess.hip -- on-device image preprocessing and reward epilogues (gfx950).
//
// The reference moves every generated image GPU -> CPU -> PIL -> CLIPProcessor -> GPU before PickScore
// (adv_grpo/rewards.py:567-571, adv_grpo/pickscore_scorer.py:21-27) and runs F.interpolate + normalise as
// separate torch kernels before DINOv2 (adv_grpo/rewards.py:379-391).  Here both preprocessors run on the
// device and write the ViT patch-embedding im2col matrix directly (bf16 [B*P, 640], 3*14*14 = 588 real
// columns + zero pad to the GEMM's K granule), so the image is read once and no resized image is stored.
//
//   * CLIP path: bit-exact emulation of PIL's 8-bit antialiased bicubic resample (Pillow Resample.c:
//     horizontal then vertical pass, 22-bit fixed-point coefficients computed on the host in float64,
//     uint8 intermediate) after the reference's (x*255).round().clamp() quantisation.
//   * DINO path: torch's upsample_bicubic2d (A = -0.75, align_corners=False, no antialias) in f32 on
//     bf16 inputs, rounded to bf16, then (x - mean)/std in f32, rounded to bf16.
//   * SigLIP path: the same resize in the input's own dtype (no bf16 rounding of f32 / u8 inputs), (x - 0.5)/0.5 in f32, bf16.
//   * clipscore path: torchvision's tensor Resize (bilinear, antialias) + CenterCrop + Normalize, mirroring torch's GPU kernel.
//   * reward epilogues: gather + L2-normalise the CLS / sampled patch tokens, head second layer +
//     0.7/0.3 mix (rewards.py:399-421); PickScore exp(logit_scale) * cos / 26 (pickscore_scorer.py:40-52); the
//     aesthetic MLP head (aesthetic_scorer.py).
#include "common.hpp"

namespace advgrpo {

constexpr int PATCH = 14, PATCH_K = 3 * PATCH * PATCH, PATCH_KPAD = 640;

__device__ inline float ld_img(const void* img, int dt, int64_t i) {
    return dt == ADVGRPO_BF16 ? bf2f(reinterpret_cast<const bf16_t*>(img)[i]) : reinterpret_cast<const float*>(img)[i];
}

// ---- CLIP: quantise + horizontal PIL pass.  img [B,3,H,W] -> tmp u8 [B,3,H,OW]
__global__ void clip_resize_h_kernel(const void* __restrict__ img, int dt, uint8_t* __restrict__ tmp, int64_t rows, int W,
                                     int OW, const int* __restrict__ bounds, const int* __restrict__ coefs, int ksize,
                                     int trunc) {
    const int64_t total = rows * OW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = i % OW;
        const int64_t row = i / OW;
        const int xmin = bounds[2 * ox], cnt = bounds[2 * ox + 1];
        int ss = 1 << 21;  // 1 << (PRECISION_BITS - 1), PRECISION_BITS = 22
        for (int k = 0; k < cnt; ++k) {
            float v = ld_img(img, dt, row * W + xmin + k) * 255.0f;
            if (dt == ADVGRPO_BF16) v = round_bf16(v);   // the product is a bf16 torch op when images are bf16
            // (x*255).round().clamp(0,255).to(uint8) (rewards.py:567)  |  (x*255).astype(uint8) (tensor_to_pil_list, TD:135-149)
            const int q = (int)fminf(fmaxf(trunc ? truncf(v) : rintf(v), 0.f), 255.f);
            ss += q * coefs[ox * ksize + k];
        }
        ss >>= 22;
        tmp[i] = (uint8_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
    }
}

// ---- CLIP: vertical PIL pass + rescale/normalise + im2col.  tmp u8 [B,3,H,OW] -> patches bf16 [B*P, 640]
// X3: the normalised pixel stays f32 and leaves as the split-bf16 left operand [hi | hi | lo], row pitch 3 * 640 (x3.hip)
template <bool X3>
__global__ void clip_resize_v_patches_kernel(const uint8_t* __restrict__ tmp, bf16_t* __restrict__ patches, int B, int H,
                                             int OH, int OW, const int* __restrict__ bounds,
                                             const int* __restrict__ coefs, int ksize, float3 mean, float3 stdv) {
    const int gw = OW / PATCH;
    const int P = (OH / PATCH) * gw;
    const int64_t total = (int64_t)B * P * PATCH_KPAD;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = i % PATCH_KPAD;
        const int64_t prow = i / PATCH_KPAD;
        bf16_t* o3 = patches + prow * (3 * PATCH_KPAD) + col;
        if (col >= PATCH_K) {
            if (X3) { o3[0] = 0; o3[PATCH_KPAD] = 0; o3[2 * PATCH_KPAD] = 0; }
            else patches[i] = 0;
            continue;
        }
        const int p = prow % P, b = prow / P;
        const int c = col / (PATCH * PATCH), iy = (col / PATCH) % PATCH, ix = col % PATCH;
        const int oy = (p / gw) * PATCH + iy, ox = (p % gw) * PATCH + ix;
        const int ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
        const uint8_t* src = tmp + ((int64_t)(b * 3 + c) * H) * OW + ox;
        int ss = 1 << 21;
        for (int k = 0; k < cnt; ++k) ss += (int)src[(int64_t)(ymin + k) * OW] * coefs[oy * ksize + k];
        ss >>= 22;
        const int q = ss < 0 ? 0 : (ss > 255 ? 255 : ss);
        // CLIPImageProcessor: rescale (u8 * (1/255) in f32) then (x - mean) / std in f32
        const float m = c == 0 ? mean.x : (c == 1 ? mean.y : mean.z);
        const float s = c == 0 ? stdv.x : (c == 1 ? stdv.y : stdv.z);
        const float x = (float)q * 0.00392156862745098f;
        const float v = (x - m) / s;
        if (X3) {
            const bf16_t hi = f2bf(v);
            o3[0] = hi; o3[PATCH_KPAD] = hi; o3[2 * PATCH_KPAD] = f2bf(v - bf2f(hi));
        } else {
            patches[i] = f2bf(v);
        }
    }
}

// ---- DINO / SigLIP: torch's upsample_bicubic2d (A = -0.75, align_corners=False, no antialias) in f32 -> normalise -> im2col.
// Same tap formulas as torch; the f32 sums may round differently from torch's build (summation order / contraction), which moves
// a bf16 result by one ulp on a few 1e-5 of the pixels (tests/test_gpu_vit.py, tests/test_gpu_siglip.py).
__device__ inline void cubic_coeffs(float t, float c[4]) {
    const float A = -0.75f;
    const float x1 = t + 1.0f, x2 = t, x3 = 1.0f - t, x4 = 2.0f - t;
    c[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
    c[1] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[2] = ((A + 2.0f) * x3 - (A + 3.0f)) * x3 * x3 + 1.0f;
    c[3] = ((A * x4 - 5.0f * A) * x4 + 8.0f * A) * x4 - 4.0f * A;
}

// The three preprocessors share one resize body and differ in where they round to bf16:
//   DINO      (bf16 tower, rewards.py:379-391): inputs rounded to bf16 first (the reference casts images to bf16, TP:816), the resize
//             result rounded to bf16, (x - mean) / std in f32, bf16.
//   DINO_X3   (the fp32 tower of image_similarity_score, rewards.py:147-203): no bf16 rounding anywhere; the normalised pixel leaves as
//             the split-bf16 left operand [hi | hi | lo], row pitch 3 * 640.
//   SIGLIP    (siglip_image_similarity, rewards.py:87-115): F.interpolate in the input's dtype -- a bf16 input's resize result is
//             rounded to bf16, an f32 one is not; u8 inputs are x * (1 / 255) in f32 first (torch's division of a device tensor by a
//             python number) -- then (x - 0.5) / 0.5 in f32, bf16.  The image is resized to OH x OW = 384 x 384, but the 14/14 patch
//             conv reads only the top-left (384 / 14) * 14 rows and columns: those are the only pixels computed.
enum PreMode { PRE_DINO = 0, PRE_DINO_X3 = 1, PRE_SIGLIP = 2 };

__device__ inline float ld_img_u8(const void* img, int dt, int64_t i) {
    if (dt == ADVGRPO_U8) return (float)reinterpret_cast<const uint8_t*>(img)[i] * (1.0f / 255.0f);
    return ld_img(img, dt, i);
}

template <int MODE>
__global__ void bicubic_patches_kernel(const void* __restrict__ img, int dt, bf16_t* __restrict__ patches, int B, int H, int W, int OH,
                                       int OW, float3 mean, float3 stdv) {
    constexpr bool X3 = MODE == PRE_DINO_X3;
    const int gw = OW / PATCH;
    const int P = (OH / PATCH) * gw;
    const float sy = (float)H / (float)OH, sx = (float)W / (float)OW;
    const int64_t total = (int64_t)B * P * PATCH_KPAD;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = i % PATCH_KPAD;
        const int64_t prow = i / PATCH_KPAD;
        bf16_t* o3 = patches + prow * (3 * PATCH_KPAD) + col;
        if (col >= PATCH_K) {
            if (X3) { o3[0] = 0; o3[PATCH_KPAD] = 0; o3[2 * PATCH_KPAD] = 0; }
            else patches[i] = 0;
            continue;
        }
        const int p = prow % P, b = prow / P;
        const int c = col / (PATCH * PATCH), iy = (col / PATCH) % PATCH, ix = col % PATCH;
        const int oy = (p / gw) * PATCH + iy, ox = (p % gw) * PATCH + ix;
        const float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
        const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
        float cy[4], cx[4];
        cubic_coeffs(fy - (float)y0, cy);
        cubic_coeffs(fx - (float)x0, cx);
        const int64_t base = (int64_t)(b * 3 + c) * H * W;
        float acc = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int yy = min(max(y0 - 1 + a, 0), H - 1);
            float r = 0.f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int xx = min(max(x0 - 1 + d, 0), W - 1);
                float v;
                if constexpr (MODE == PRE_SIGLIP) {
                    v = ld_img_u8(img, dt, base + (int64_t)yy * W + xx);
                } else {
                    v = ld_img(img, dt, base + (int64_t)yy * W + xx);
                    if (!X3 && dt != ADVGRPO_BF16) v = round_bf16(v);
                }
                r += cx[d] * v;
            }
            acc += cy[a] * r;
        }
        const bool round_resized = MODE == PRE_DINO || (MODE == PRE_SIGLIP && dt == ADVGRPO_BF16);
        const float rb = round_resized ? round_bf16(acc) : acc;
        const float m = c == 0 ? mean.x : (c == 1 ? mean.y : mean.z);
        const float s = c == 0 ? stdv.x : (c == 1 ? stdv.y : stdv.z);
        const float v = (rb - m) / s;
        if (X3) {
            const bf16_t hi = f2bf(v);
            o3[0] = hi; o3[PATCH_KPAD] = hi; o3[2 * PATCH_KPAD] = f2bf(v - bf2f(hi));
        } else {
            patches[i] = f2bf(v);
        }
    }
}

// ---- rows: out[b*(1+n) + 0] = norm(feats[b,0]); out[b*(1+n)+1+j] = norm(feats[b, 1+idx[b,j]]);  x/(||x||+eps)
__global__ __launch_bounds__(256) void gather_l2norm_rows_kernel(const bf16_t* __restrict__ feats, const int64_t* __restrict__ idx,
                                                                 bf16_t* __restrict__ out, int B, int T, int D, int n,
                                                                 float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * (1 + n)) return;
    const int b = row / (1 + n), j = row % (1 + n);
    const int tok = j == 0 ? 0 : 1 + (int)idx[(int64_t)b * n + j - 1];
    const bf16_t* src = feats + ((int64_t)b * T + tok) * D;
    float sq = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = bf2f(src[d]); sq += v * v; }
    // torch: x / (x.norm() + 1e-6) on bf16 tensors: norm accumulates in f32 and rounds to bf16, add and divide in bf16
    const float nrm = round_bf16(round_bf16(sqrtf(wave_sum(sq))) + eps);
    for (int d = lane; d < D; d += 64) out[(int64_t)row * D + d] = f2bf(bf2f(src[d]) / nrm);
}

// ---- hidden [B*(1+n), Hd] bf16 (after Linear+GELU) . w2 + b2 -> cls/patch logits; hybrid = cw*cls + (1-cw)*mean
__global__ __launch_bounds__(256) void dino_head_combine_kernel(const bf16_t* __restrict__ hidden, const bf16_t* __restrict__ w2,
                                                                const bf16_t* __restrict__ b2, int Hd, int n, float cls_w,
                                                                float* __restrict__ hybrid, float* __restrict__ cls_out,
                                                                float* __restrict__ patch_out) {
    __shared__ float logits[1 + 256];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < 1 + n; r += 4) {
        const bf16_t* h = hidden + ((int64_t)b * (1 + n) + r) * Hd;
        float acc = 0.f;
        for (int d = lane; d < Hd; d += 64) acc += bf2f(h[d]) * bf2f(w2[d]);
        acc = wave_sum(acc);
        if (lane == 0) logits[r] = round_bf16(acc + bf2f(b2[0]));   // bf16 Linear output
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int j = 0; j < n; ++j) s += logits[1 + j];
        const float mean = round_bf16(s / (float)n);
        const float c = logits[0];
        // cls_weight * cls_score + (1 - cls_weight) * patch_score_mean, each op rounded to bf16
        hybrid[b] = round_bf16(round_bf16(cls_w * c) + round_bf16((float)(1.0 - (double)cls_w) * mean));
        cls_out[b] = c;
    }
    for (int j = threadIdx.x; j < n; j += blockDim.x) patch_out[(int64_t)b * n + j] = logits[1 + j];
}

// ---- PickScore: exp(logit_scale) * <t/|t|, i/|i|> / 26 per pair
__global__ __launch_bounds__(64) void pickscore_pairs_kernel(const bf16_t* __restrict__ img, const bf16_t* __restrict__ txt,
                                                             int P, float logit_scale_exp, float* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float ii = 0.f, tt = 0.f, it = 0.f;
    for (int d = lane; d < P; d += 64) {
        const float a = bf2f(img[(int64_t)b * P + d]), c = bf2f(txt[(int64_t)b * P + d]);
        ii += a * a; tt += c * c; it += a * c;
    }
    ii = wave_sum(ii); tt = wave_sum(tt); it = wave_sum(it);
    if (lane == 0) out[b] = logit_scale_exp * it / (sqrtf(ii) * sqrtf(tt)) / 26.0f;
}

// ---- torchvision T.Resize(shortest edge, bilinear, antialias) + T.CenterCrop + T.Normalize on a tensor (ClipScorer,
// adv_grpo/clip_scorer.py), computed only inside the crop window.  Mirrors torch's GPU upsample_bilinear2d_aa (UpSampleBilinear2d.cu
// upsample_gen2d_aa_out_frame + UpSample.cuh upsample_antialias::*) at scalar_t = accscalar_t = float: torchvision casts an input that
// is not f32 / f64 to f32 before F.interpolate and back after it.  Per output pixel: the x and y spans and weights in f32
// (center = scale (i + 0.5), xmin = max(int(center - support + 0.5), 0), triangle taps at (j + xmin - center + 0.5) / max(scale, 1),
// each divided by their f32 sum), the horizontal pass over the ysize input rows, then the vertical pass over those row results.
// Contraction is off in this code (`#pragma clang fp contract(off)`; fusing 1 - x * invscale in the filter moved 0.3 % of the outputs):
// the only fused multiply-adds are the explicit ones, one per tap after the first, which is how torch's build contracts
// `output += t * wts` (checked against torch's GPU kernel).
struct AaSpan {
    int xmin, xsize;
    float xmc, invscale, total;     // xmin - center, 1 / max(scale, 1), sum of the unnormalised taps
};

__device__ inline float aa_filter(float x) {
#pragma clang fp contract(off)
    if (x < 0.f) x = -x;
    return x < 1.f ? 1.f - x : 0.f;
}

__device__ inline float aa_tap(const AaSpan& a, int j) {
#pragma clang fp contract(off)
    return aa_filter(((float)j + a.xmc + 0.5f) * a.invscale);
}

__device__ inline AaSpan aa_span(int i, int in_size, float scale) {
#pragma clang fp contract(off)
    AaSpan a;
    const float support = scale >= 1.f ? scale : 1.f;                        // (interp_size / 2) * scale, interp_size = 2
    const float center = scale * ((float)i + 0.5f);         // scale * (i + 0.5): exact in double, rounded once
    // f32 (center -/+ support), then + 0.5 in double (a double literal in torch), truncated toward zero
    a.xmin = max((int)((double)(center - support) + 0.5), 0);
    a.xsize = min((int)((double)(center + support) + 0.5), in_size) - a.xmin;
    a.xmc = (float)a.xmin - center;
    a.invscale = scale >= 1.f ? 1.f / scale : 1.f;
    a.total = 0.f;
    for (int j = 0; j < a.xsize; ++j) a.total += aa_tap(a, j);
    return a;
}

__device__ inline float aa_weight(const AaSpan& a, int j) {
#pragma clang fp contract(off)
    const float w = aa_tap(a, j);
    return a.total != 0.f ? w / a.total : w;
}

__device__ inline float ld_img_tv(const void* img, int dt, int64_t i) {
#pragma clang fp contract(off)
    if (dt == ADVGRPO_U8) return (float)reinterpret_cast<const uint8_t*>(img)[i] / 255.0f;   // torch.tensor(u8) / 255.0
    return ld_img(img, dt, i);
}

// img [B,3,H,W] (F32 / BF16 / U8) resized to scale (H / RH, W / RW); the OS x OS window at (top, left) of the resized image is
// normalised and written as 14x14 patch rows.  bf16_ops (a bf16 input): the resize result, x - mean and the division are each rounded
// to bf16 (torch's bf16 elementwise ops), and mean / std arrive as bf16 values.
template <bool X3>
__global__ void tv_resize_patches_kernel(const void* __restrict__ img, int dt, bf16_t* __restrict__ patches, int B, int H, int W,
                                         float scale_h, float scale_w, int top, int left, int OS, float3 mean, float3 stdv,
                                         int bf16_ops) {
#pragma clang fp contract(off)
    const int gw = OS / PATCH;
    const int P = gw * gw;
    const int64_t total = (int64_t)B * P * PATCH_KPAD;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = i % PATCH_KPAD;
        const int64_t prow = i / PATCH_KPAD;
        bf16_t* o3 = patches + prow * (3 * PATCH_KPAD) + col;
        if (col >= PATCH_K) {
            if (X3) { o3[0] = 0; o3[PATCH_KPAD] = 0; o3[2 * PATCH_KPAD] = 0; }
            else patches[i] = 0;
            continue;
        }
        const int p = prow % P, b = prow / P;
        const int c = col / (PATCH * PATCH), iy = (col / PATCH) % PATCH, ix = col % PATCH;
        const int ry = top + (p / gw) * PATCH + iy, rx = left + (p % gw) * PATCH + ix;      // pixel of the resized image
        const AaSpan sx = aa_span(rx, W, scale_w), sy = aa_span(ry, H, scale_h);
        const int64_t base = (int64_t)(b * 3 + c) * H * W;
        float out = 0.f;
        for (int y = 0; y < sy.xsize; ++y) {
            const int64_t row = base + (int64_t)(sy.xmin + y) * W + sx.xmin;
            float h = ld_img_tv(img, dt, row) * aa_weight(sx, 0);
            for (int x = 1; x < sx.xsize; ++x) h = __fmaf_rn(ld_img_tv(img, dt, row + x), aa_weight(sx, x), h);
            const float wy = aa_weight(sy, y);
            out = y == 0 ? h * wy : __fmaf_rn(h, wy, out);
        }
        const float m = c == 0 ? mean.x : (c == 1 ? mean.y : mean.z);
        const float s = c == 0 ? stdv.x : (c == 1 ? stdv.y : stdv.z);
        float v;
        if (bf16_ops) v = round_bf16(round_bf16(round_bf16(out) - m) / s);
        else v = (out - m) / s;
        if (X3) {
            const bf16_t hi = f2bf(v);
            o3[0] = hi; o3[PATCH_KPAD] = hi; o3[2 * PATCH_KPAD] = f2bf(v - bf2f(hi));
        } else {
            patches[i] = f2bf(v);
        }
    }
}

// ---- LAION aesthetic predictor (adv_grpo/aesthetic_scorer.py): e / ||e|| -> Linear 768-1024-128-64-16-1 (no activations; dropout is
// inactive in eval).  One workgroup of 4 waves scores AES_ROWS rows; every value is f32.  Each output of a layer is one wave's dot
// product: lane l runs a fused multiply-add chain over k = l, l + 64, ... in increasing k, the 64 partial sums meet in the fixed DPP
// tree of wave_sum, and the bias is added last.  The squared norm is summed the same way.  A row's score therefore takes the same
// operations in the same order whatever the batch size and wherever the row sits in it.  No atomics.
constexpr int AES_D = 768, AES_ROWS = 4, AES_PITCH = 1024;      // input width, rows per workgroup, LDS row pitch (the widest layer)

struct AesWeights { const float* w[5]; const float* b[5]; };

// y[r, o] = sum_k w[o, k] x[r, k] + bias[o] for the AES_ROWS rows of the workgroup, one wave per output o
__device__ inline void aes_dense(const float* __restrict__ w, const float* __restrict__ bias, const float* xin, int K, float* yout, int N) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = wave; o < N; o += 4) {
        const float* wr = w + (int64_t)o * K;
        float acc[AES_ROWS];
#pragma unroll
        for (int r = 0; r < AES_ROWS; ++r) acc[r] = 0.f;
        for (int k = lane; k < K; k += 64) {
            const float wk = wr[k];
#pragma unroll
            for (int r = 0; r < AES_ROWS; ++r) acc[r] = __fmaf_rn(wk, xin[r * AES_PITCH + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < AES_ROWS; ++r) {
            const float t = wave_sum(acc[r]);
            if (lane == 0) yout[r * AES_PITCH + o] = t + bias[o];
        }
    }
}

__global__ __launch_bounds__(256) void aesthetic_head_kernel(const void* __restrict__ emb, int dt, int N, AesWeights wt,
                                                             float* __restrict__ scores) {
#pragma clang fp contract(off)
    __shared__ float bufA[AES_ROWS * AES_PITCH], bufB[AES_ROWS * AES_PITCH];
    const int row0 = blockIdx.x * AES_ROWS;
    const int rows = min(AES_ROWS, N - row0);               // rows past N are zeros, normalised to zeros, and never stored
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int idx = threadIdx.x; idx < AES_ROWS * AES_D; idx += blockDim.x) {
        const int r = idx / AES_D, k = idx % AES_D;
        bufB[r * AES_PITCH + k] = r < rows ? ld_img(emb, dt, (int64_t)(row0 + r) * AES_D + k) : 0.f;
    }
    __syncthreads();
    {                                                        // embed / torch.linalg.vector_norm(embed, dim=-1, keepdim=True): wave r, row r
        const float* e = bufB + wave * AES_PITCH;
        float sq = 0.f;
        for (int k = lane; k < AES_D; k += 64) sq = __fmaf_rn(e[k], e[k], sq);
        const float nrm = __fsqrt_rn(wave_sum(sq));
        for (int k = lane; k < AES_D; k += 64) bufA[wave * AES_PITCH + k] = wave < rows ? e[k] / nrm : 0.f;
    }
    __syncthreads();
    aes_dense(wt.w[0], wt.b[0], bufA, 768, bufB, 1024);
    __syncthreads();
    aes_dense(wt.w[1], wt.b[1], bufB, 1024, bufA, 128);
    __syncthreads();
    aes_dense(wt.w[2], wt.b[2], bufA, 128, bufB, 64);
    __syncthreads();
    aes_dense(wt.w[3], wt.b[3], bufB, 64, bufA, 16);
    __syncthreads();
    aes_dense(wt.w[4], wt.b[4], bufA, 16, bufB, 1);
    __syncthreads();
    if (threadIdx.x < rows) scores[row0 + threadIdx.x] = bufB[threadIdx.x * AES_PITCH];
}

}  // namespace advgrpo

using namespace advgrpo;

static int clip_preprocess_impl(bool x3, const void* image, int image_dtype, void* patches, uint8_t* tmp, int B, int H, int W,
                                int OH, int OW, const int* bounds_h, const int* coefs_h, int ksize_h, const int* bounds_v,
                                const int* coefs_v, int ksize_v, const float* mean3_host, const float* std3_host,
                                int quant_trunc, void* stream) {
    ADVGRPO_CHECK(image && patches && tmp && bounds_h && coefs_h && bounds_v && coefs_v && mean3_host && std3_host,
                  "clip_preprocess: null pointer");
    ADVGRPO_CHECK(OH % PATCH == 0 && OW % PATCH == 0 && B > 0, "clip_preprocess: output must be a multiple of 14");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(clip_resize_h_kernel, dim3(2048), dim3(256), 0, s, image, image_dtype, tmp, (int64_t)B * 3 * H, W,
                       OW, bounds_h, coefs_h, ksize_h, quant_trunc);
    ADVGRPO_LAUNCH_CHECK();
    const float3 m = make_float3(mean3_host[0], mean3_host[1], mean3_host[2]);
    const float3 sd = make_float3(std3_host[0], std3_host[1], std3_host[2]);
    if (x3)
        hipLaunchKernelGGL(clip_resize_v_patches_kernel<true>, dim3(2048), dim3(256), 0, s, tmp, (bf16_t*)patches, B, H, OH, OW,
                           bounds_v, coefs_v, ksize_v, m, sd);
    else
        hipLaunchKernelGGL(clip_resize_v_patches_kernel<false>, dim3(2048), dim3(256), 0, s, tmp, (bf16_t*)patches, B, H, OH, OW,
                           bounds_v, coefs_v, ksize_v, m, sd);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_clip_preprocess_patches(const void* image, int image_dtype, void* patches, uint8_t* tmp, int B,
                                               int H, int W, int OH, int OW, const int* bounds_h, const int* coefs_h,
                                               int ksize_h, const int* bounds_v, const int* coefs_v, int ksize_v,
                                               const float* mean3_host, const float* std3_host, int quant_trunc,
                                               void* stream) {
    return clip_preprocess_impl(false, image, image_dtype, patches, tmp, B, H, W, OH, OW, bounds_h, coefs_h, ksize_h, bounds_v,
                                coefs_v, ksize_v, mean3_host, std3_host, quant_trunc, stream);
}

/* the same with the normalised pixels kept in f32 and written as the split-bf16 left operand: patches3 [B*P, 3*640] */
extern "C" int advgrpo_clip_preprocess_patches_x3(const void* image, int image_dtype, void* patches3, uint8_t* tmp, int B,
                                                  int H, int W, int OH, int OW, const int* bounds_h, const int* coefs_h,
                                                  int ksize_h, const int* bounds_v, const int* coefs_v, int ksize_v,
                                                  const float* mean3_host, const float* std3_host, int quant_trunc,
                                                  void* stream) {
    return clip_preprocess_impl(true, image, image_dtype, patches3, tmp, B, H, W, OH, OW, bounds_h, coefs_h, ksize_h, bounds_v,
                                coefs_v, ksize_v, mean3_host, std3_host, quant_trunc, stream);
}

static int dino_preprocess_impl(bool x3, const void* image, int image_dtype, void* patches, int B, int H, int W, int OH, int OW,
                                const float* mean3_host, const float* std3_host, void* stream) {
    ADVGRPO_CHECK(image && patches && mean3_host && std3_host, "dino_preprocess: null pointer");
    ADVGRPO_CHECK(OH % PATCH == 0 && OW % PATCH == 0 && B > 0, "dino_preprocess: output must be a multiple of 14");
    const float3 m = make_float3(mean3_host[0], mean3_host[1], mean3_host[2]);
    const float3 sd = make_float3(std3_host[0], std3_host[1], std3_host[2]);
    if (x3)
        hipLaunchKernelGGL(bicubic_patches_kernel<PRE_DINO_X3>, dim3(4096), dim3(256), 0, as_stream(stream), image, image_dtype,
                           (bf16_t*)patches, B, H, W, OH, OW, m, sd);
    else
        hipLaunchKernelGGL(bicubic_patches_kernel<PRE_DINO>, dim3(4096), dim3(256), 0, as_stream(stream), image, image_dtype,
                           (bf16_t*)patches, B, H, W, OH, OW, m, sd);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_dino_preprocess_patches(const void* image, int image_dtype, void* patches, int B, int H, int W,
                                               int OH, int OW, const float* mean3_host, const float* std3_host,
                                               void* stream) {
    return dino_preprocess_impl(false, image, image_dtype, patches, B, H, W, OH, OW, mean3_host, std3_host, stream);
}

/* the fp32 pipeline of image_similarity_score (rewards.py:147-203): f32 bicubic, no bf16 rounding; patches3 [B*P, 3*640] */
extern "C" int advgrpo_dino_preprocess_patches_x3(const void* image, int image_dtype, void* patches3, int B, int H, int W,
                                                  int OH, int OW, const float* mean3_host, const float* std3_host,
                                                  void* stream) {
    return dino_preprocess_impl(true, image, image_dtype, patches3, B, H, W, OH, OW, mean3_host, std3_host, stream);
}

/* siglip_image_similarity's preprocessing (see the kernel): image [B,3,H,W] f32 / bf16 / u8 -> patches bf16 [B*P, 640], P = (OS/14)^2 */
extern "C" int advgrpo_siglip_preprocess_patches(const void* image, int image_dtype, void* patches, int B, int H, int W, int OS,
                                                 void* stream) {
    ADVGRPO_CHECK(image && patches, "siglip_preprocess: null pointer");
    ADVGRPO_CHECK(B > 0 && H > 0 && W > 0 && OS >= PATCH, "siglip_preprocess: bad shape (B=%d H=%d W=%d OS=%d)", B, H, W, OS);
    ADVGRPO_CHECK(image_dtype == ADVGRPO_F32 || image_dtype == ADVGRPO_BF16 || image_dtype == ADVGRPO_U8,
                  "siglip_preprocess: image dtype must be f32, bf16 or u8");
    hipLaunchKernelGGL(bicubic_patches_kernel<PRE_SIGLIP>, dim3(4096), dim3(256), 0, as_stream(stream), image, image_dtype,
                       (bf16_t*)patches, B, H, W, OS, OS, make_float3(0.5f, 0.5f, 0.5f), make_float3(0.5f, 0.5f, 0.5f));
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

/* clipscore's torchvision preprocessing (see the kernel): image [B,3,H,W] f32 / bf16 / u8 resized to RH x RW, the OS x OS window at
   (top, left) normalised and written as patch rows: bf16 [B*P, 640], or with x3 the split-bf16 [B*P, 3*640]; P = (OS/14)^2 */
extern "C" int advgrpo_tv_resize_patches(const void* image, int image_dtype, void* patches, int x3, int B, int H, int W, int RH, int RW,
                                         int top, int left, int OS, const float* mean3_host, const float* std3_host, void* stream) {
    ADVGRPO_CHECK(image && patches && mean3_host && std3_host, "tv_resize_patches: null pointer");
    ADVGRPO_CHECK(B > 0 && H > 0 && W > 0 && RH > 0 && RW > 0 && OS >= PATCH && OS % PATCH == 0,
                  "tv_resize_patches: bad shape (B=%d H=%d W=%d RH=%d RW=%d OS=%d)", B, H, W, RH, RW, OS);
    ADVGRPO_CHECK(top >= 0 && left >= 0 && top + OS <= RH && left + OS <= RW,
                  "tv_resize_patches: the %d x %d crop at (%d, %d) leaves the %d x %d resized image", OS, OS, top, left, RH, RW);
    ADVGRPO_CHECK(image_dtype == ADVGRPO_F32 || image_dtype == ADVGRPO_BF16 || image_dtype == ADVGRPO_U8,
                  "tv_resize_patches: image dtype must be f32, bf16 or u8");
    const float sh = (float)H / (float)RH, sw = (float)W / (float)RW;      // area_pixel_compute_scale<float>, align_corners = False
    const float3 m = make_float3(mean3_host[0], mean3_host[1], mean3_host[2]);
    const float3 sd = make_float3(std3_host[0], std3_host[1], std3_host[2]);
    const int bf16_ops = image_dtype == ADVGRPO_BF16;
    if (x3)
        hipLaunchKernelGGL(tv_resize_patches_kernel<true>, dim3(4096), dim3(256), 0, as_stream(stream), image, image_dtype,
                           (bf16_t*)patches, B, H, W, sh, sw, top, left, OS, m, sd, bf16_ops);
    else
        hipLaunchKernelGGL(tv_resize_patches_kernel<false>, dim3(4096), dim3(256), 0, as_stream(stream), image, image_dtype,
                           (bf16_t*)patches, B, H, W, sh, sw, top, left, OS, m, sd, bf16_ops);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

/* the aesthetic head: embeds f32 / bf16 [N, 768] -> scores f32 [N]; w0..w4 / b0..b4 f32, row-major [out, in] (see the kernel) */
extern "C" int advgrpo_aesthetic_head(const void* embeds, int embed_dtype, int N, const float* w0, const float* b0, const float* w1,
                                      const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const float* w4,
                                      const float* b4, float* scores, void* stream) {
    ADVGRPO_CHECK(embeds && scores && w0 && b0 && w1 && b1 && w2 && b2 && w3 && b3 && w4 && b4 && N > 0, "aesthetic_head: bad argument");
    ADVGRPO_CHECK(embed_dtype == ADVGRPO_F32 || embed_dtype == ADVGRPO_BF16, "aesthetic_head: embeds must be f32 or bf16");
    AesWeights wt = {{w0, w1, w2, w3, w4}, {b0, b1, b2, b3, b4}};
    hipLaunchKernelGGL(aesthetic_head_kernel, dim3((N + AES_ROWS - 1) / AES_ROWS), dim3(256), 0, as_stream(stream), embeds, embed_dtype,
                       N, wt, scores);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_gather_l2norm_rows(const void* feats, const int64_t* idx, void* out, int B, int T, int D, int n,
                                          float eps, void* stream) {
    ADVGRPO_CHECK(feats && out && (n == 0 || idx) && B > 0 && T > 0 && D > 0, "gather_l2norm_rows: bad argument");
    const int rows = B * (1 + n);
    hipLaunchKernelGGL(gather_l2norm_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream),
                       (const bf16_t*)feats, idx, (bf16_t*)out, B, T, D, n, eps);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_dino_head_combine(const void* hidden, const void* w2, const void* b2, int B, int Hd, int n,
                                         float cls_weight, float* hybrid, float* cls_score, float* patch_scores,
                                         void* stream) {
    ADVGRPO_CHECK(hidden && w2 && b2 && hybrid && cls_score && patch_scores && n >= 1 && n <= 256 && B > 0,
                  "dino_head_combine: bad argument");
    hipLaunchKernelGGL(dino_head_combine_kernel, dim3(B), dim3(256), 0, as_stream(stream), (const bf16_t*)hidden,
                       (const bf16_t*)w2, (const bf16_t*)b2, Hd, n, cls_weight, hybrid, cls_score, patch_scores);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_pickscore_pairs(const void* image_embs, const void* text_embs, int B, int P, float logit_scale_exp,
                                       float* scores, void* stream) {
    ADVGRPO_CHECK(image_embs && text_embs && scores && B > 0 && P > 0, "pickscore_pairs: bad argument");
    hipLaunchKernelGGL(pickscore_pairs_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const bf16_t*)image_embs,
                       (const bf16_t*)text_embs, P, logit_scale_exp, scores);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
