// sde_step.hip -- fused CFG combine + Flow-CPS or Flow-SDE step + per-sample Gaussian log-prob (gfx950).
//
// Replaces sd3_pipeline_with_logprob_fast.py:640-655 and sd3_sde_with_logprob.py:77-139 of the
// reference (six torch elementwise kernels, a randn, a .mean and two host syncs per step) with
// one HBM pass: 8 B (bf16 v_u, v_t, x in; bf16 x' out) to 12 B per latent element.  The kernel
// is launch-latency bound at 512^2 (0.5 MB per sample), so it is shaped for few, wide
// wavefronts: 16 B per lane per load, one block-level reduction, a tiny finalize launch.
//
// sde_step_branch_kernel is the fan-out form for the branch step of the shared-prefix rollouts: P rows in, P * G rows out, one read of the
// inputs and one evaluation of the mean per up to 8 copies, the bits of sde_step_kernel on the materialised repeat.
//
// Every kernel is a template over the step's arithmetic: CpsStep (Flow-CPS, SDE:117-134) or FlowStep (the original Flow-GRPO SDE with its
// full Gaussian log-density, SDE:44-67).  Loads, CFG combine, epsilon, stores and reductions are the same code for both.
//
// sde_step_rescaled_kernel / _bwd_kernel put Qwen-Image's norm-rescaled true CFG (v = comb * ||v_pos|| / ||comb|| per 2 x 2 x 16 token, the
// rounding points and summation order of qwen_sampler.hip) in front of the same two steps, on the unpacked [B, 16, H, W] tensors.
//
// Built with -ffp-contract=off: every reference torch op is one f32 rounding here too, so
// mean / next are bit-exact with the torch-CPU oracle; log_prob differs by summation order only.
#include <type_traits>

#include "common.hpp"
#include "qwen_token.hpp"

namespace advgrpo {

constexpr int SDE_THREADS = 256;
constexpr int SDE_VEC = 8;                       // elements per lane per iteration
constexpr int SDE_CHUNK = SDE_THREADS * SDE_VEC;  // 2048 elements per block iteration
constexpr int SDE_MAX_BLOCKS = 64;               // per sample
constexpr int SDE_BRANCH_COPIES = 8;             // sde_step_branch_kernel: copies of an input row per block

__device__ inline void load8(const void* p, int dt, int64_t i, float o[8]) {
    if (dt == ADVGRPO_BF16) {
        // (spelled out, not unpack8: through the shared helper sde_step_kernel<CpsStep> allocates its registers differently)
        const uint4 r = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(p) + i);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = bf2f((bf16_t)(w[k] & 0xffffu));
            o[2 * k + 1] = bf2f((bf16_t)(w[k] >> 16));
        }
    } else {
        ld8_f32(reinterpret_cast<const float*>(p) + i, o);
    }
}
__device__ inline void store8(void* p, int dt, int64_t i, const float o[8]) {
    if (dt == ADVGRPO_BF16) {
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p) + i) = pack8(o);
    } else {
        float* f = reinterpret_cast<float*>(p) + i;
        *reinterpret_cast<float4*>(f) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(f + 4) = make_float4(o[4], o[5], o[6], o[7]);
    }
}

struct SdeCoef {  // per-sample scalars, each one f32 rounding as in the reference
    float sigma, one_m_sigma, one_m_sigma_prev, sq, std;
};
__device__ inline SdeCoef sde_coef(const float* sigma, const float* sigma_prev, int stride, int b,
                                   float sin_coeff) {
    SdeCoef c;
    const float s = sigma[(int64_t)b * stride], sp = sigma_prev[(int64_t)b * stride];
    c.sigma = s;
    c.std = sp * sin_coeff;               // sd3_sde_with_logprob.py:118
    c.one_m_sigma = 1.0f - s;             // :120
    c.one_m_sigma_prev = 1.0f - sp;       // :121
    c.sq = sqrtf(sp * sp - c.std * c.std);  // :121
    return c;
}
// v after CFG (:640-642 of the pipeline); bf16 inputs => the three torch bf16 ops, each rounded
__device__ inline float cfg_v(float vu, float vt, bool has_cfg, bool bf, float g) {
    if (!has_cfg) return vu;
    float d = vt - vu;
    if (bf) d = round_bf16(d);
    float m = g * d;
    if (bf) m = round_bf16(m);
    float r = vu + m;
    if (bf) r = round_bf16(r);
    return r;
}

// Flow-CPS (SDE:117-134): x' = mean + std * eps, log_prob = mean_i -(x' - mean)^2
struct CpsStep {
    SdeCoef c;
    __device__ CpsStep(const float* sigma, const float* sigma_prev, int stride, int b, float sin_coeff, const float*)
        : c(sde_coef(sigma, sigma_prev, stride, b, sin_coeff)) {}
    __device__ float mean(float x, float v) const {
        const float x0 = x - c.sigma * v;                     // :119
        const float x1 = x + v * c.one_m_sigma;                // :120
        return x0 * c.one_m_sigma_prev + x1 * c.sq;            // :121
    }
    __device__ float noise() const { return c.std; }           // :131 the factor of eps
    __device__ float std() const { return c.std; }
    // d mean / d v, and grad_log_prob * d log_prob / d mean = grad_log_prob * 2 (prev - mean) / n
    __device__ float dmu_dv() const { return c.one_m_sigma * c.sq - c.sigma * c.one_m_sigma_prev; }
    __device__ float lp_scale(float glp, int64_t n) const { return glp * 2.0f / (float)n * dmu_dv(); }
};

// Flow-SDE (SDE:44-67), every scalar in f32 in the reference's operation order:
//   s = sqrt(sigma / (1 - (sigma == 1 ? sigma_max : sigma))) * noise_level ; dt = sigma_prev - sigma ; w = s * sqrt(-dt)
//   mean = x * (1 + s^2 / (2 sigma) * dt) + v * (1 + s^2 (1 - sigma) / (2 sigma)) * dt ; x' = mean + w * eps
//   log_prob = mean_i( -(x' - mean)^2 / (2 w^2) ) - log w - log sqrt(2 pi)         (flow_sde_finalize_kernel)
struct FlowStep {
    float cx, cv, dt, s, w;
    __device__ FlowStep(const float* sigma, const float* sigma_prev, int stride, int b, float noise_level,
                        const float* sigma_max) {
        const float sg = sigma[(int64_t)b * stride], sp = sigma_prev[(int64_t)b * stride];
        dt = sp - sg;                                                      // :47
        s = sqrtf(sg / (1.0f - (sg == 1.0f ? sigma_max[0] : sg))) * noise_level;   // :49
        const float s2 = s * s, two_sigma = 2.0f * sg;
        cx = 1.0f + s2 / two_sigma * dt;                                   // :53, the factor of x
        cv = 1.0f + s2 * (1.0f - sg) / two_sigma;                          // :53, the factor of v before `* dt`
        w = s * sqrtf(-1.0f * dt);                                         // :62
    }
    __device__ float mean(float x, float v) const { return x * cx + v * cv * dt; }   // :53
    __device__ float noise() const { return w; }                           // :62
    __device__ float std() const { return s; }                             // std_dev_t, without the sqrt(-dt)
    // d mean / d v, and grad_log_prob * d log_prob / d mean = grad_log_prob * (prev - mean) / (n w^2)
    __device__ float dmu_dv() const { return cv * dt; }
    __device__ float lp_scale(float glp, int64_t n) const { return glp / ((float)n * (w * w)) * dmu_dv(); }
};

template <class Step>
__global__ __launch_bounds__(SDE_THREADS) void sde_step_kernel(
    const void* __restrict__ v_u, const void* __restrict__ v_t, int v_dt, float guidance,
    const void* __restrict__ x, int x_dt, const float* __restrict__ sigma,
    const float* __restrict__ sigma_prev, int sigma_stride, float level, const float* __restrict__ sigma_max, int mode,
    const float* __restrict__ eps, uint64_t seed, uint64_t offset,
    const void* __restrict__ prev, int prev_dt, float* __restrict__ out_next,
    void* __restrict__ out_cast, int cast_dt, float* __restrict__ out_mean,
    float* __restrict__ partial, float* __restrict__ out_std, int64_t n) {
    __shared__ float red[SDE_THREADS / 64];
    const int b = blockIdx.y;
    const Step c(sigma, sigma_prev, sigma_stride, b, level, sigma_max);
    const bool has_cfg = v_t != nullptr, bf = v_dt == ADVGRPO_BF16;
    const int64_t base = (int64_t)b * n;
    const Philox ph(seed);
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * SDE_CHUNK + threadIdx.x * SDE_VEC; i < n;
         i += (int64_t)gridDim.x * SDE_CHUNK) {
        float vu[8], vt[8], xs[8], e[8], mean[8], nxt[8];
        load8(v_u, v_dt, base + i, vu);
        if (has_cfg) load8(v_t, v_dt, base + i, vt);
        load8(x, x_dt, base + i, xs);
        if (mode == ADVGRPO_SDE_EPS) {
            load8(eps, ADVGRPO_F32, base + i, e);
        } else if (mode == ADVGRPO_SDE_PHILOX) {
            philox_normal4(ph, offset + (uint64_t)((base + i) >> 2), e);
            philox_normal4(ph, offset + (uint64_t)((base + i) >> 2) + 1, e + 4);
        } else {
            load8(prev, prev_dt, base + i, e);  // e holds prev_sample
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = cfg_v(vu[k], vt[k], has_cfg, bf, guidance);
            mean[k] = c.mean(xs[k], v);
            nxt[k] = (mode == ADVGRPO_SDE_REPLAY) ? e[k] : mean[k] + c.noise() * e[k];
            const float d = nxt[k] - mean[k];
            acc += d * d;                                       // :134, :65 (sign and scale at finalize)
        }
        if (out_next && mode != ADVGRPO_SDE_REPLAY) store8(out_next, ADVGRPO_F32, base + i, nxt);
        if (out_cast && mode != ADVGRPO_SDE_REPLAY) store8(out_cast, cast_dt, base + i, nxt);
        if (out_mean) store8(out_mean, ADVGRPO_F32, base + i, mean);
    }
    const float tot = block_sum<SDE_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) {
        partial[b * gridDim.x + blockIdx.x] = tot;
        if (blockIdx.x == 0 && out_std) out_std[b] = c.std();
    }
}

// Fan-out form of sde_step_kernel for the branch step of the shared-prefix rollouts (sd3_pipeline_with_logprob_fast.py:163, :385: the
// latents are repeated G times and every copy takes its own epsilon).  v_u / v_t / x hold P rows; output row j = g * P + p (torch's
// .repeat tiling) reads input row p.  A block owns the chunks sde_step_kernel's block (blockIdx.x, j) would own and runs the same f32
// operations in the same order on them, so every output -- the block partials of log_prob included -- has the bits of sde_step_kernel on
// the materialised repeat.  The 16 B of v_u, v_t and x per lane are loaded, and the mean is computed, once per chunk for up to
// SDE_BRANCH_COPIES copies; the copies' running sums live in lane-private LDS slots (a runtime-indexed register array would go to scratch).
template <class Step>
__global__ __launch_bounds__(SDE_THREADS) void sde_step_branch_kernel(
    const void* __restrict__ v_u, const void* __restrict__ v_t, int v_dt, float guidance,
    const void* __restrict__ x, int x_dt, const float* __restrict__ sigma,
    const float* __restrict__ sigma_prev, int sigma_stride, float level, const float* __restrict__ sigma_max, int mode,
    const float* __restrict__ eps, uint64_t seed, uint64_t offset,
    const void* __restrict__ prev, int prev_dt, float* __restrict__ out_next,
    void* __restrict__ out_cast, int cast_dt, float* __restrict__ out_mean,
    float* __restrict__ partial, float* __restrict__ out_std, int P, int G, int64_t n) {
    __shared__ float red[SDE_THREADS / 64];
    __shared__ float accs[SDE_BRANCH_COPIES][SDE_THREADS];
    const int p = blockIdx.y;
    const int g0 = blockIdx.z * SDE_BRANCH_COPIES;
    const int ng = G - g0 < SDE_BRANCH_COPIES ? G - g0 : SDE_BRANCH_COPIES;
    const Step c(sigma, sigma_prev, sigma_stride, p, level, sigma_max);
    const bool has_cfg = v_t != nullptr, bf = v_dt == ADVGRPO_BF16;
    const int64_t in_base = (int64_t)p * n;
    const Philox ph(seed);
    for (int gg = 0; gg < ng; ++gg) accs[gg][threadIdx.x] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * SDE_CHUNK + threadIdx.x * SDE_VEC; i < n;
         i += (int64_t)gridDim.x * SDE_CHUNK) {
        float vu[8], vt[8], xs[8], mean[8];
        load8(v_u, v_dt, in_base + i, vu);
        if (has_cfg) load8(v_t, v_dt, in_base + i, vt);
        load8(x, x_dt, in_base + i, xs);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = cfg_v(vu[k], vt[k], has_cfg, bf, guidance);
            mean[k] = c.mean(xs[k], v);
        }
        for (int gg = 0; gg < ng; ++gg) {
            const int64_t o = ((int64_t)(g0 + gg) * P + p) * n + i;   // element (j, i) of the P * G-row outputs
            float e[8], nxt[8];
            if (mode == ADVGRPO_SDE_EPS) {
                load8(eps, ADVGRPO_F32, o, e);
            } else if (mode == ADVGRPO_SDE_PHILOX) {
                philox_normal4(ph, offset + (uint64_t)(o >> 2), e);
                philox_normal4(ph, offset + (uint64_t)(o >> 2) + 1, e + 4);
            } else {
                load8(prev, prev_dt, o, e);  // e holds prev_sample
            }
            float acc = accs[gg][threadIdx.x];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                nxt[k] = (mode == ADVGRPO_SDE_REPLAY) ? e[k] : mean[k] + c.noise() * e[k];
                const float d = nxt[k] - mean[k];
                acc += d * d;                                       // :134, :65 (sign and scale at finalize)
            }
            accs[gg][threadIdx.x] = acc;
            if (out_next && mode != ADVGRPO_SDE_REPLAY) store8(out_next, ADVGRPO_F32, o, nxt);
            if (out_cast && mode != ADVGRPO_SDE_REPLAY) store8(out_cast, cast_dt, o, nxt);
            if (out_mean) store8(out_mean, ADVGRPO_F32, o, mean);
        }
    }
    for (int gg = 0; gg < ng; ++gg) {
        const float tot = block_sum<SDE_THREADS / 64>(accs[gg][threadIdx.x], red);
        if (threadIdx.x == 0) {
            const int64_t j = (int64_t)(g0 + gg) * P + p;
            partial[j * gridDim.x + blockIdx.x] = tot;
            if (blockIdx.x == 0 && out_std) out_std[j] = c.std();
        }
    }
}

// log_prob[b] = -(sum of block partials)/n ; partials summed in fixed order in f64
__global__ void sde_finalize_kernel(const float* __restrict__ partial, int nblk, int64_t n,
                                    float* __restrict__ out_log_prob, int B, float sign = -1.0f) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += (double)partial[b * nblk + i];
    out_log_prob[b] = (float)((double)sign * (s / (double)n));
}

// Flow-SDE: log_prob[b] = -(sum of block partials) / (n * 2 w^2) - log w - log sqrt(2 pi)   (SDE:64-71); row b takes the schedule row b % P.
// noise_level == 0: w == 0 and the sum is 0, so this is 0/0 - log 0 = NaN, as in the reference.
__global__ void flow_sde_finalize_kernel(const float* __restrict__ partial, int nblk, int64_t n, float* __restrict__ out_log_prob, int B,
                                         const float* __restrict__ sigma, const float* __restrict__ sigma_prev, int sigma_stride, int P,
                                         float noise_level, const float* __restrict__ sigma_max) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const FlowStep c(sigma, sigma_prev, sigma_stride, b % P, noise_level, sigma_max);
    double s = 0.0;
    for (int i = 0; i < nblk; ++i) s += (double)partial[b * nblk + i];
    const double two_w2 = (double)(2.0f * (c.w * c.w));                    // :65, the reference's f32 denominator
    out_log_prob[b] = (float)(-(s / (double)n) / two_w2 - log((double)c.w) - 0.91893853320467274178);
}

template <class Step>
__global__ __launch_bounds__(SDE_THREADS) void sde_step_bwd_kernel(
    const void* __restrict__ v_u, const void* __restrict__ v_t, int v_dt, float guidance,
    const void* __restrict__ x, int x_dt, const float* __restrict__ sigma,
    const float* __restrict__ sigma_prev, int sigma_stride, float level, const float* __restrict__ sigma_max,
    const void* __restrict__ prev, int prev_dt, const float* __restrict__ grad_lp,
    void* __restrict__ g_u, void* __restrict__ g_t, int64_t n,
    const float* __restrict__ mean_ref, float kl_weight, int B, float* __restrict__ kl_partial) {
    __shared__ float red[SDE_THREADS / 64];
    const int b = blockIdx.y;
    const Step c(sigma, sigma_prev, sigma_stride, b, level, sigma_max);
    const bool has_cfg = v_t != nullptr, bf = v_dt == ADVGRPO_BF16;
    const int64_t base = (int64_t)b * n;
    const float dmu_dv = c.dmu_dv();
    const float scale = c.lp_scale(grad_lp[b], n);
    // KL term (TP:1105-1108,1126-1130): loss += beta * mean_b mean_elem (mean - mean_ref)^2, mean_ref = the same step's mean
    // under the adapter-free transformer; d/d mean = beta * 2 (mean - mean_ref) / (n B), then the same d mean / d v
    const float kl_scale = mean_ref ? kl_weight * 2.0f / ((float)n * (float)B) * dmu_dv : 0.f;
    float kl_acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * SDE_CHUNK + threadIdx.x * SDE_VEC; i < n;
         i += (int64_t)gridDim.x * SDE_CHUNK) {
        float vu[8], vt[8], xs[8], pv[8], gu[8], gt[8], mr[8];
        if (mean_ref) load8(mean_ref, ADVGRPO_F32, base + i, mr);
        load8(v_u, v_dt, base + i, vu);
        if (has_cfg) load8(v_t, v_dt, base + i, vt);
        load8(x, x_dt, base + i, xs);
        load8(prev, prev_dt, base + i, pv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float v = cfg_v(vu[k], vt[k], has_cfg, bf, guidance);
            const float mean = c.mean(xs[k], v);
            float gv = scale * (pv[k] - mean);
            if (mean_ref) {
                const float d = mean - mr[k];
                gv += kl_scale * d;
                kl_acc += d * d;
            }
            if (bf) gv = round_bf16(gv);  // autograd hands the (summed) f32 grad back through .float()
            gu[k] = has_cfg ? (1.0f - guidance) * gv : gv;
            gt[k] = guidance * gv;
        }
        store8(g_u, v_dt, base + i, gu);
        if (has_cfg) store8(g_t, v_dt, base + i, gt);
    }
    if (mean_ref) {      // per-sample KL value: block partials, summed in fixed order by sde_finalize_kernel
        const float tot = block_sum<SDE_THREADS / 64>(kl_acc, red);
        if (threadIdx.x == 0) kl_partial[b * gridDim.x + blockIdx.x] = tot;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Qwen-Image's norm-rescaled true CFG in front of the same steps: v = comb * ||v_pos|| / ||comb|| over each 2 x 2 x 16 token, with
// the rounding points and the fixed summation order of qwen_cfg_euler_kernel (qwen_sampler.hip; the layout is qwen_token.hpp's),
// then Step::mean on the rescaled v held in registers.  Unlike that kernel a block never leaves its sample (grid = blocks per
// sample x B), so a block's partial of log_prob -- and a NaN from an all-zero token -- stays inside one sample.
//
// rs_rescaled_v: every thread of the block calls it (it holds a barrier when there is a second prediction).  In: this lane's row
// segments of v_neg / v_pos.  Out: o = the rescaled prediction (v_neg itself without v_pos), cmb = the combined one, pos = v_pos,
// and per token the forward's cn = ||pos||, nn = ||comb|| and ratio = cn / nn, each rounded to bf16 on bf16 predictions.
template <int TPL, bool KEEP>
__device__ __forceinline__ void rs_rescaled_v(const void* __restrict__ v_neg, const void* __restrict__ v_pos, int v_dt, float scale,
                                              bool valid, int64_t base, int64_t plane, int W, int lane, int w,
                                              float (*part)[QS_WAVES][QS_LANES * TPL], float (&o)[QS_CPW * 2][2 * TPL],
                                              float (&cmb)[KEEP ? QS_CPW * 2 : 1][2 * TPL], float (&pos)[KEEP ? QS_CPW * 2 : 1][2 * TPL],
                                              float (&cn)[TPL], float (&nn)[TPL], float (&ratio)[TPL]) {
    constexpr int N = 2 * TPL;
    const bool has_cfg = v_pos != nullptr, bf = v_dt == ADVGRPO_BF16;
    float sp[TPL], sc[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) sp[t] = sc[t] = 0.f;
#pragma unroll
    for (int k = 0; k < QS_CPW * 2; ++k)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            o[k][j] = 0.f;
            if constexpr (KEEP) cmb[k][j] = pos[k][j] = 0.f;
        }
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
                    const float c = cfg_v(ng[j], ps[j], true, bf, scale);
                    o[k][j] = c;
                    if constexpr (KEEP) { cmb[k][j] = c; pos[k][j] = ps[j]; }
                    sp[j >> 1] += ps[j] * ps[j];
                    sc[j >> 1] += c * c;
                }
            } else {
#pragma unroll
                for (int j = 0; j < N; ++j) o[k][j] = ng[j];
            }
        }
    }
    if (!has_cfg) return;                           // (uniform over the block: every wave reaches the barrier or none does)
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        part[0][w][lane * TPL + t] = sp[t];
        part[1][w][lane * TPL + t] = sc[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        float p = 0.f, c = 0.f;
#pragma unroll
        for (int i = 0; i < QS_WAVES; ++i) {
            p += part[0][i][lane * TPL + t];
            c += part[1][i][lane * TPL + t];
        }
        cn[t] = sqrtf(p);
        nn[t] = sqrtf(c);
        if (bf) { cn[t] = round_bf16(cn[t]); nn[t] = round_bf16(nn[t]); }
        float q = cn[t] / nn[t];                    // no epsilon: an all-zero token is 0 / 0 = NaN, as in the pipeline
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

// lane -> (token row, first pixel) of sample blockIdx.y; false past the sample's last token
template <int TPL>
__device__ __forceinline__ bool rs_lane_base(int C, int H, int W, int lane, int w, int64_t& base) {
    const int upr = (W / 2) / TPL;                  // lanes per token row
    const int64_t u = (int64_t)blockIdx.x * QS_LANES + lane;
    base = 0;
    if (u >= (int64_t)(H / 2) * upr) return false;
    const int ux = (int)(u % upr), ty = (int)(u / upr);
    base = (((int64_t)blockIdx.y * C + w * QS_CPW) * H + 2 * ty) * W + (int64_t)ux * (2 * TPL);
    return true;
}

template <class Step, int TPL>
__global__ __launch_bounds__(QS_THREADS) void sde_step_rescaled_kernel(
    const void* __restrict__ v_u, const void* __restrict__ v_t, int v_dt, float guidance,
    const void* __restrict__ x, int x_dt, const float* __restrict__ sigma,
    const float* __restrict__ sigma_prev, int sigma_stride, float level, const float* __restrict__ sigma_max, int mode,
    const float* __restrict__ eps, uint64_t seed, uint64_t offset,
    const void* __restrict__ prev, int prev_dt, float* __restrict__ out_next,
    void* __restrict__ out_cast, int cast_dt, float* __restrict__ out_mean,
    float* __restrict__ partial, float* __restrict__ out_std, int C, int H, int W) {
    constexpr int N = 2 * TPL;
    __shared__ float part[2][QS_WAVES][QS_LANES * TPL];
    __shared__ float red[QS_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const Step c(sigma, sigma_prev, sigma_stride, b, level, sigma_max);
    const int64_t plane = (int64_t)H * W;
    int64_t base;
    const bool valid = rs_lane_base<TPL>(C, H, W, lane, w, base);
    float v[QS_CPW * 2][N], unused[1][N], cn[TPL], nn[TPL], ratio[TPL];
    rs_rescaled_v<TPL, false>(v_u, v_t, v_dt, guidance, valid, base, plane, W, lane, w, part, v, unused, unused, cn, nn, ratio);
    const Philox ph(seed);
    float acc = 0.f;
    if (valid) {
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k) {
            const int64_t off = base + (k >> 1) * plane + (k & 1) * W;   // = b * n + i: the element index of advgrpo_sde_step
            float xs[N], e[N], mean[N], nxt[N];
            qs_load<N>(x, x_dt, off, xs);
            if (mode == ADVGRPO_SDE_EPS) {
                qs_load<N>(eps, ADVGRPO_F32, off, e);
            } else if (mode == ADVGRPO_SDE_PHILOX) {
                float z[4];                          // the N elements lie in one Philox block: off % N == 0
                philox_normal4(ph, offset + (uint64_t)(off >> 2), z);
                if constexpr (N == 4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[j] = z[j];
                } else {
                    const bool hi = (off & 2) != 0;
                    e[0] = hi ? z[2] : z[0];
                    e[1] = hi ? z[3] : z[1];
                }
            } else {
                qs_load<N>(prev, prev_dt, off, e);  // e holds prev_sample
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                mean[j] = c.mean(xs[j], v[k][j]);
                nxt[j] = (mode == ADVGRPO_SDE_REPLAY) ? e[j] : mean[j] + c.noise() * e[j];
                const float d = nxt[j] - mean[j];
                acc += d * d;
            }
            if (out_next && mode != ADVGRPO_SDE_REPLAY) qs_store<N>(out_next, ADVGRPO_F32, off, nxt);
            if (out_cast && mode != ADVGRPO_SDE_REPLAY) qs_store<N>(out_cast, cast_dt, off, nxt);
            if (out_mean) qs_store<N>(out_mean, ADVGRPO_F32, off, mean);
        }
    }
    const float tot = block_sum<QS_WAVES>(acc, red);
    if (threadIdx.x == 0) {
        partial[b * gridDim.x + blockIdx.x] = tot;
        if (blockIdx.x == 0 && out_std) out_std[b] = c.std();
    }
}

// Backward of the replay-mode rescaled step.  Per token, with p = v_pos, n = v_neg, c = n + s (p - n), a = ||p||, b = ||c||, r = a / b
// and g = dL/dv = lp_scale (prev - mean) [+ kl_scale (mean - mean_ref)] (mean recomputed from the forward's rounded v):
//   dL/dc = r (g - (c.g) / b^2 c) ;  dL/dp = s dL/dc + (c.g) / (a b) p ;  dL/dn = (1 - s) dL/dc
// the gradient of the unrounded formula at the forward's c, a, b and r (what autograd's straight-through casts give).  c.g is a second
// per-token reduction in the order of the norms; everything f32, one rounding to the prediction dtype at the store.
template <class Step, int TPL>
__global__ __launch_bounds__(QS_THREADS) void sde_step_rescaled_bwd_kernel(
    const void* __restrict__ v_u, const void* __restrict__ v_t, int v_dt, float guidance,
    const void* __restrict__ x, int x_dt, const float* __restrict__ sigma,
    const float* __restrict__ sigma_prev, int sigma_stride, float level, const float* __restrict__ sigma_max,
    const void* __restrict__ prev, int prev_dt, const float* __restrict__ grad_lp,
    void* __restrict__ g_u, void* __restrict__ g_t, int C, int H, int W,
    const float* __restrict__ mean_ref, float kl_weight, int B, float* __restrict__ kl_partial) {
    constexpr int N = 2 * TPL;
    __shared__ float part[2][QS_WAVES][QS_LANES * TPL];
    __shared__ float dots[QS_WAVES][QS_LANES * TPL];
    __shared__ float red[QS_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
    const Step c(sigma, sigma_prev, sigma_stride, b, level, sigma_max);
    const bool has_cfg = v_t != nullptr;
    const int64_t plane = (int64_t)H * W, n = (int64_t)C * plane;
    const float dmu_dv = c.dmu_dv();
    const float scale = c.lp_scale(grad_lp[b], n);
    const float kl_scale = mean_ref ? kl_weight * 2.0f / ((float)n * (float)B) * dmu_dv : 0.f;
    int64_t base;
    const bool valid = rs_lane_base<TPL>(C, H, W, lane, w, base);
    float v[QS_CPW * 2][N], cmb[QS_CPW * 2][N], pos[QS_CPW * 2][N], cn[TPL], nn[TPL], ratio[TPL];
    rs_rescaled_v<TPL, true>(v_u, v_t, v_dt, guidance, valid, base, plane, W, lane, w, part, v, cmb, pos, cn, nn, ratio);
    float kl_acc = 0.f, cg[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) cg[t] = 0.f;
    if (valid) {
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k) {      // v[k][j] becomes g
            const int64_t off = base + (k >> 1) * plane + (k & 1) * W;
            float xs[N], pv[N], mr[N];
            qs_load<N>(x, x_dt, off, xs);
            qs_load<N>(prev, prev_dt, off, pv);
            if (mean_ref) qs_load<N>(mean_ref, ADVGRPO_F32, off, mr);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float mean = c.mean(xs[j], v[k][j]);
                float gv = scale * (pv[j] - mean);
                if (mean_ref) {
                    const float d = mean - mr[j];
                    gv += kl_scale * d;
                    kl_acc += d * d;
                }
                v[k][j] = gv;
                if (has_cfg) cg[j >> 1] += cmb[k][j] * gv;
            }
        }
    }
    if (has_cfg) {
#pragma unroll
        for (int t = 0; t < TPL; ++t) dots[w][lane * TPL + t] = cg[t];
        __syncthreads();
        float k_c[TPL], k_p[TPL];                   // (c.g) / b^2 and (c.g) / (a b)
#pragma unroll
        for (int t = 0; t < TPL; ++t) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < QS_WAVES; ++i) d += dots[i][lane * TPL + t];
            k_c[t] = d / (nn[t] * nn[t]);
            k_p[t] = d / (cn[t] * nn[t]);
        }
        if (valid) {
#pragma unroll
            for (int k = 0; k < QS_CPW * 2; ++k) {
                const int64_t off = base + (k >> 1) * plane + (k & 1) * W;
                float gu[N], gt[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float dc = ratio[j >> 1] * (v[k][j] - k_c[j >> 1] * cmb[k][j]);
                    gu[j] = (1.0f - guidance) * dc;
                    gt[j] = guidance * dc + k_p[j >> 1] * pos[k][j];
                }
                qs_store<N>(g_u, v_dt, off, gu);
                qs_store<N>(g_t, v_dt, off, gt);
            }
        }
    } else if (valid) {
#pragma unroll
        for (int k = 0; k < QS_CPW * 2; ++k) qs_store<N>(g_u, v_dt, base + (k >> 1) * plane + (k & 1) * W, v[k]);
    }
    if (mean_ref) {      // per-sample KL value: block partials, summed in fixed order by sde_finalize_kernel
        const float tot = block_sum<QS_WAVES>(kl_acc, red);
        if (threadIdx.x == 0) kl_partial[b * gridDim.x + blockIdx.x] = tot;
    }
}

__global__ __launch_bounds__(256) void randn_kernel(void* __restrict__ out, int dt, int64_t n,
                                                    uint64_t seed, uint64_t offset) {
    const Philox ph(seed);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g * 4 < n;
         g += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal4(ph, offset + (uint64_t)g, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = g * 4 + k;
            if (i < n) {
                if (dt == ADVGRPO_BF16) reinterpret_cast<bf16_t*>(out)[i] = f2bf(z[k]);
                else reinterpret_cast<float*>(out)[i] = z[k];
            }
        }
    }
}

static int sde_blocks(int64_t n) {
    int64_t nb = (n + SDE_CHUNK - 1) / SDE_CHUNK;
    return (int)(nb < 1 ? 1 : (nb > SDE_MAX_BLOCKS ? SDE_MAX_BLOCKS : nb));
}

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int64_t advgrpo_sde_step_workspace_bytes(int B, int64_t n) {
    return (int64_t)B * sde_blocks(n) * sizeof(float);
}

static int check_common(int v_dtype, int x_dtype, int B, int64_t n) {
    ADVGRPO_CHECK(v_dtype == ADVGRPO_F32 || v_dtype == ADVGRPO_BF16, "sde_step: bad v_dtype %d", v_dtype);
    ADVGRPO_CHECK(x_dtype == ADVGRPO_F32 || x_dtype == ADVGRPO_BF16, "sde_step: bad x_dtype %d", x_dtype);
    ADVGRPO_CHECK(B > 0 && n > 0 && n % SDE_VEC == 0, "sde_step: need B>0 and n %% 8 == 0 (B=%d n=%lld)", B,
                  (long long)n);
    return 0;
}

// The four entry shapes, once for both steps.  Step = CpsStep: level = sin_coeff, sigma_max unused (NULL); Step = FlowStep: level =
// noise_level, sigma_max required.  `what` names the entry in error messages.
template <class Step>
static int step_finalize(const float* ws, int nb, int64_t n, float* out_log_prob, int B, const float* sigma, const float* sigma_prev,
                         int sigma_stride, int P, float level, const float* sigma_max, void* stream) {
    if constexpr (std::is_same_v<Step, FlowStep>) {
        hipLaunchKernelGGL(flow_sde_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), ws, nb, n, out_log_prob, B,
                           sigma, sigma_prev, sigma_stride, P, level, sigma_max);
    } else {
        hipLaunchKernelGGL(sde_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), ws, nb, n, out_log_prob, B, -1.0f);
    }
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

template <class Step>
static int step_fwd(const char* what, const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                    int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float level,
                    const float* sigma_max, int mode, const float* eps, uint64_t seed, uint64_t offset, const void* prev_sample,
                    int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype, float* out_mean,
                    float* out_log_prob, float* out_std, void* workspace, int B, int64_t n, void* stream) {
    if (check_common(v_dtype, x_dtype, B, n)) return -1;
    ADVGRPO_CHECK(v_uncond && x && sigma && sigma_prev && out_log_prob && workspace, "%s: null argument", what);
    ADVGRPO_CHECK((!std::is_same_v<Step, FlowStep>) || sigma_max, "%s: null sigma_max", what);
    ADVGRPO_CHECK(mode >= 0 && mode <= 2, "%s: bad mode %d", what, mode);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_EPS || eps, "%s: mode EPS needs eps", what);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_REPLAY || prev_sample, "%s: mode REPLAY needs prev_sample", what);
    const int nb = sde_blocks(n);
    hipLaunchKernelGGL(sde_step_kernel<Step>, dim3(nb, B), dim3(SDE_THREADS), 0, as_stream(stream), v_uncond, v_text,
                       v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride, level, sigma_max, mode, eps,
                       seed, offset, prev_sample, prev_dtype, out_next_f32, out_next_cast, out_cast_dtype, out_mean,
                       (float*)workspace, out_std, n);
    ADVGRPO_LAUNCH_CHECK();
    return step_finalize<Step>((const float*)workspace, nb, n, out_log_prob, B, sigma, sigma_prev, sigma_stride, B, level, sigma_max,
                               stream);
}

template <class Step>
static int step_branch(const char* what, const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                       int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float level,
                       const float* sigma_max, int mode, const float* eps, uint64_t seed, uint64_t offset,
                       const void* prev_sample, int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype,
                       float* out_mean, float* out_log_prob, float* out_std, void* workspace, int P, int G, int64_t n,
                       void* stream) {
    ADVGRPO_CHECK(P > 0 && G > 0, "%s: need P>0 and G>0 (P=%d G=%d)", what, P, G);
    if (check_common(v_dtype, x_dtype, P, n)) return -1;
    const int gz = (G + SDE_BRANCH_COPIES - 1) / SDE_BRANCH_COPIES;
    ADVGRPO_CHECK(P <= 65535 && gz <= 65535 && (int64_t)P * G <= INT32_MAX, "%s: P=%d G=%d too large", what, P, G);
    ADVGRPO_CHECK(v_uncond && x && sigma && sigma_prev && out_log_prob && workspace, "%s: null argument", what);
    ADVGRPO_CHECK((!std::is_same_v<Step, FlowStep>) || sigma_max, "%s: null sigma_max", what);
    ADVGRPO_CHECK(mode >= 0 && mode <= 2, "%s: bad mode %d", what, mode);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_EPS || eps, "%s: mode EPS needs eps", what);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_REPLAY || prev_sample, "%s: mode REPLAY needs prev_sample", what);
    const int nb = sde_blocks(n), B = P * G;
    hipLaunchKernelGGL(sde_step_branch_kernel<Step>, dim3(nb, P, gz), dim3(SDE_THREADS), 0, as_stream(stream), v_uncond, v_text,
                       v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride, level, sigma_max, mode, eps,
                       seed, offset, prev_sample, prev_dtype, out_next_f32, out_next_cast, out_cast_dtype, out_mean,
                       (float*)workspace, out_std, P, G, n);
    ADVGRPO_LAUNCH_CHECK();
    return step_finalize<Step>((const float*)workspace, nb, n, out_log_prob, B, sigma, sigma_prev, sigma_stride, P, level, sigma_max,
                               stream);
}

// mean_ref == NULL: the policy-only backward (kl_weight, kl_out and workspace unused)
template <class Step>
static int step_bwd(const char* what, const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                    int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float level,
                    const float* sigma_max, const void* prev_sample, int prev_dtype, const float* grad_log_prob, bool with_kl,
                    const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text, float* kl_out, void* workspace,
                    int B, int64_t n, void* stream) {
    if (check_common(v_dtype, x_dtype, B, n)) return -1;
    ADVGRPO_CHECK(v_uncond && x && sigma && sigma_prev && prev_sample && grad_log_prob && grad_v_uncond &&
                      (!with_kl || (mean_ref && kl_out && workspace)), "%s: null argument", what);
    ADVGRPO_CHECK((!std::is_same_v<Step, FlowStep>) || sigma_max, "%s: null sigma_max", what);
    ADVGRPO_CHECK(!v_text || grad_v_text, "%s: CFG needs grad_v_text", what);
    const int nb = sde_blocks(n);
    hipLaunchKernelGGL(sde_step_bwd_kernel<Step>, dim3(nb, B), dim3(SDE_THREADS), 0, as_stream(stream), v_uncond, v_text,
                       v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride, level, sigma_max, prev_sample,
                       prev_dtype, grad_log_prob, grad_v_uncond, grad_v_text, n, with_kl ? mean_ref : (const float*)nullptr,
                       with_kl ? kl_weight : 0.f, B, with_kl ? (float*)workspace : (float*)nullptr);
    ADVGRPO_LAUNCH_CHECK();
    if (with_kl) {
        hipLaunchKernelGGL(sde_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream),
                           (const float*)workspace, nb, n, kl_out, B, 1.0f);
        ADVGRPO_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int advgrpo_sde_step(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                int sigma_stride, float sin_coeff, int mode, const float* eps, uint64_t seed,
                                uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                float* out_std, void* workspace, int B, int64_t n, void* stream) {
    return step_fwd<CpsStep>("sde_step", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride,
                             sin_coeff, nullptr, mode, eps, seed, offset, prev_sample, prev_dtype, out_next_f32, out_next_cast,
                             out_cast_dtype, out_mean, out_log_prob, out_std, workspace, B, n, stream);
}

extern "C" int advgrpo_sde_step_branch(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                       const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                       int sigma_stride, float sin_coeff, int mode, const float* eps, uint64_t seed,
                                       uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                       void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                       float* out_std, void* workspace, int P, int G, int64_t n, void* stream) {
    return step_branch<CpsStep>("sde_step_branch", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                                sigma_stride, sin_coeff, nullptr, mode, eps, seed, offset, prev_sample, prev_dtype, out_next_f32,
                                out_next_cast, out_cast_dtype, out_mean, out_log_prob, out_std, workspace, P, G, n, stream);
}

extern "C" int advgrpo_sde_step_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                    const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                    int sigma_stride, float sin_coeff, const void* prev_sample, int prev_dtype,
                                    const float* grad_log_prob, void* grad_v_uncond, void* grad_v_text, int B,
                                    int64_t n, void* stream) {
    return step_bwd<CpsStep>("sde_step_bwd", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride,
                             sin_coeff, nullptr, prev_sample, prev_dtype, grad_log_prob, false, nullptr, 0.f, grad_v_uncond,
                             grad_v_text, nullptr, nullptr, B, n, stream);
}

extern "C" int advgrpo_sde_step_bwd_kl(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                       const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                       int sigma_stride, float sin_coeff, const void* prev_sample, int prev_dtype,
                                       const float* grad_log_prob, const float* mean_ref, float kl_weight,
                                       void* grad_v_uncond, void* grad_v_text, float* kl_out, void* workspace, int B,
                                       int64_t n, void* stream) {
    return step_bwd<CpsStep>("sde_step_bwd_kl", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                             sigma_stride, sin_coeff, nullptr, prev_sample, prev_dtype, grad_log_prob, true, mean_ref, kl_weight,
                             grad_v_uncond, grad_v_text, kl_out, workspace, B, n, stream);
}

extern "C" int advgrpo_flow_sde_step(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                     const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                     int sigma_stride, float noise_level, const float* sigma_max, int mode, const float* eps,
                                     uint64_t seed, uint64_t offset, const void* prev_sample, int prev_dtype,
                                     float* out_next_f32, void* out_next_cast, int out_cast_dtype, float* out_mean,
                                     float* out_log_prob, float* out_std, void* workspace, int B, int64_t n, void* stream) {
    return step_fwd<FlowStep>("flow_sde_step", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev, sigma_stride,
                              noise_level, sigma_max, mode, eps, seed, offset, prev_sample, prev_dtype, out_next_f32, out_next_cast,
                              out_cast_dtype, out_mean, out_log_prob, out_std, workspace, B, n, stream);
}

extern "C" int advgrpo_flow_sde_step_branch(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                            const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                            int sigma_stride, float noise_level, const float* sigma_max, int mode,
                                            const float* eps, uint64_t seed, uint64_t offset, const void* prev_sample,
                                            int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype,
                                            float* out_mean, float* out_log_prob, float* out_std, void* workspace, int P, int G,
                                            int64_t n, void* stream) {
    return step_branch<FlowStep>("flow_sde_step_branch", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                                 sigma_stride, noise_level, sigma_max, mode, eps, seed, offset, prev_sample, prev_dtype,
                                 out_next_f32, out_next_cast, out_cast_dtype, out_mean, out_log_prob, out_std, workspace, P, G, n,
                                 stream);
}

extern "C" int advgrpo_flow_sde_step_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                         const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                         int sigma_stride, float noise_level, const float* sigma_max, const void* prev_sample,
                                         int prev_dtype, const float* grad_log_prob, void* grad_v_uncond, void* grad_v_text,
                                         int B, int64_t n, void* stream) {
    return step_bwd<FlowStep>("flow_sde_step_bwd", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                              sigma_stride, noise_level, sigma_max, prev_sample, prev_dtype, grad_log_prob, false, nullptr, 0.f,
                              grad_v_uncond, grad_v_text, nullptr, nullptr, B, n, stream);
}

extern "C" int advgrpo_flow_sde_step_bwd_kl(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                            const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                            int sigma_stride, float noise_level, const float* sigma_max,
                                            const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                            const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                            float* kl_out, void* workspace, int B, int64_t n, void* stream) {
    return step_bwd<FlowStep>("flow_sde_step_bwd_kl", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                              sigma_stride, noise_level, sigma_max, prev_sample, prev_dtype, grad_log_prob, true, mean_ref,
                              kl_weight, grad_v_uncond, grad_v_text, kl_out, workspace, B, n, stream);
}

// ---- the norm-rescaled true-CFG forms: shape checks, layout choice and grid, once for the four entries
struct RsLaunch {
    bool pair;      // two tokens per lane
    int nb;         // blocks per sample
    int64_t n;      // elements per sample
};
static int64_t rs_blocks(int H, int W, int tpl) {
    const int64_t units = (int64_t)(H / 2) * ((W / 2) / tpl);
    return (units + QS_LANES - 1) / QS_LANES;
}
static int rs_shape(const char* what, int v_dtype, int x_dtype, int B, int C, int H, int W, int patch_size, int sigma_stride) {
    ADVGRPO_CHECK(v_dtype == ADVGRPO_F32 || v_dtype == ADVGRPO_BF16, "%s: bad v_dtype %d", what, v_dtype);
    ADVGRPO_CHECK(x_dtype == ADVGRPO_F32 || x_dtype == ADVGRPO_BF16, "%s: bad x_dtype %d", what, x_dtype);
    ADVGRPO_CHECK(patch_size == 2 && C == QS_CPW * QS_WAVES, "%s: built for patch 2 and C = %d (patch=%d C=%d)", what,
                  QS_CPW * QS_WAVES, patch_size, C);
    ADVGRPO_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && sigma_stride >= 0,
                  "%s: need 0 < B <= 65535 and even H, W (B=%d H=%d W=%d)", what, B, H, W);
    ADVGRPO_CHECK(rs_blocks(H, W, 1) <= INT32_MAX / B, "%s: too many tokens", what);
    return 0;
}
// ptrs / sizes: every tensor the kernel reads or writes N elements at a time, with its element size (NULL entries are skipped)
static int rs_layout(const char* what, const void* const* ptrs, const int* sizes, int count, int C, int H, int W, RsLaunch* L) {
    auto aligned = [&](int elems) {
        for (int i = 0; i < count; ++i)
            if (ptrs[i] && (uintptr_t)ptrs[i] % (uintptr_t)(elems * sizes[i]) != 0) return false;
        return true;
    };
    ADVGRPO_CHECK(aligned(2), "%s: tensors must be aligned to two of their elements", what);
    L->pair = W % 4 == 0 && aligned(4);
    L->nb = (int)rs_blocks(H, W, L->pair ? 2 : 1);
    L->n = (int64_t)C * H * W;
    return 0;
}

extern "C" int64_t advgrpo_sde_step_rescaled_workspace_bytes(int B, int C, int H, int W, int patch_size) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * rs_blocks(H, W, 1) * sizeof(float);   // the one-token-per-lane grid: the larger of the two layouts
}

template <class Step>
static int step_rescaled_fwd(const char* what, const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                             int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float level,
                             const float* sigma_max, int mode, const float* eps, uint64_t seed, uint64_t offset,
                             const void* prev_sample, int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype,
                             float* out_mean, float* out_log_prob, float* out_std, void* workspace, int B, int C, int H, int W,
                             int patch_size, void* stream) {
    if (rs_shape(what, v_dtype, x_dtype, B, C, H, W, patch_size, sigma_stride)) return -1;
    ADVGRPO_CHECK(v_uncond && x && sigma && sigma_prev && out_log_prob && workspace, "%s: null argument", what);
    ADVGRPO_CHECK((!std::is_same_v<Step, FlowStep>) || sigma_max, "%s: null sigma_max", what);
    ADVGRPO_CHECK(mode >= 0 && mode <= 2, "%s: bad mode %d", what, mode);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_EPS || eps, "%s: mode EPS needs eps", what);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_REPLAY || prev_sample, "%s: mode REPLAY needs prev_sample", what);
    ADVGRPO_CHECK(mode != ADVGRPO_SDE_REPLAY || prev_dtype == ADVGRPO_F32 || prev_dtype == ADVGRPO_BF16, "%s: bad prev_dtype %d", what,
                  prev_dtype);
    ADVGRPO_CHECK(!out_next_cast || mode == ADVGRPO_SDE_REPLAY || out_cast_dtype == ADVGRPO_F32 || out_cast_dtype == ADVGRPO_BF16,
                  "%s: bad out_cast_dtype %d", what, out_cast_dtype);
    const bool replay = mode == ADVGRPO_SDE_REPLAY;
    const void* ptrs[] = {v_uncond, v_text, x, mode == ADVGRPO_SDE_EPS ? eps : nullptr, replay ? prev_sample : nullptr,
                          replay ? nullptr : out_next_f32, replay ? nullptr : out_next_cast, out_mean};
    const int sizes[] = {dtype_size(v_dtype), dtype_size(v_dtype), dtype_size(x_dtype), 4, dtype_size(prev_dtype), 4,
                         dtype_size(out_cast_dtype), 4};
    RsLaunch L;
    if (rs_layout(what, ptrs, sizes, 8, C, H, W, &L)) return -1;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(L.nb, B), dim3(QS_THREADS), 0, as_stream(stream), v_uncond, v_text, v_dtype, guidance_scale, x,
                           x_dtype, sigma, sigma_prev, sigma_stride, level, sigma_max, mode, eps, seed, offset, prev_sample, prev_dtype,
                           out_next_f32, out_next_cast, out_cast_dtype, out_mean, (float*)workspace, out_std, C, H, W);
    };
    if (L.pair) launch(sde_step_rescaled_kernel<Step, 2>);
    else launch(sde_step_rescaled_kernel<Step, 1>);
    ADVGRPO_LAUNCH_CHECK();
    return step_finalize<Step>((const float*)workspace, L.nb, L.n, out_log_prob, B, sigma, sigma_prev, sigma_stride, B, level, sigma_max,
                               stream);
}

// mean_ref == NULL: the policy-only backward (kl_weight, kl_out and workspace unused)
template <class Step>
static int step_rescaled_bwd(const char* what, const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                             const void* x, int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float level,
                             const float* sigma_max, const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                             const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text, float* kl_out,
                             void* workspace, int B, int C, int H, int W, int patch_size, void* stream) {
    if (rs_shape(what, v_dtype, x_dtype, B, C, H, W, patch_size, sigma_stride)) return -1;
    ADVGRPO_CHECK(v_uncond && x && sigma && sigma_prev && prev_sample && grad_log_prob && grad_v_uncond &&
                      (!mean_ref || (kl_out && workspace)), "%s: null argument", what);
    ADVGRPO_CHECK((!std::is_same_v<Step, FlowStep>) || sigma_max, "%s: null sigma_max", what);
    ADVGRPO_CHECK(prev_dtype == ADVGRPO_F32 || prev_dtype == ADVGRPO_BF16, "%s: bad prev_dtype %d", what, prev_dtype);
    ADVGRPO_CHECK(!v_text || grad_v_text, "%s: CFG needs grad_v_text", what);
    const void* ptrs[] = {v_uncond, v_text, x, prev_sample, mean_ref, grad_v_uncond, v_text ? grad_v_text : nullptr};
    const int sizes[] = {dtype_size(v_dtype), dtype_size(v_dtype), dtype_size(x_dtype), dtype_size(prev_dtype), 4, dtype_size(v_dtype),
                         dtype_size(v_dtype)};
    RsLaunch L;
    if (rs_layout(what, ptrs, sizes, 7, C, H, W, &L)) return -1;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(L.nb, B), dim3(QS_THREADS), 0, as_stream(stream), v_uncond, v_text, v_dtype, guidance_scale, x,
                           x_dtype, sigma, sigma_prev, sigma_stride, level, sigma_max, prev_sample, prev_dtype, grad_log_prob,
                           grad_v_uncond, grad_v_text, C, H, W, mean_ref, mean_ref ? kl_weight : 0.f, B,
                           mean_ref ? (float*)workspace : (float*)nullptr);
    };
    if (L.pair) launch(sde_step_rescaled_bwd_kernel<Step, 2>);
    else launch(sde_step_rescaled_bwd_kernel<Step, 1>);
    ADVGRPO_LAUNCH_CHECK();
    if (mean_ref) {
        hipLaunchKernelGGL(sde_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), (const float*)workspace, L.nb, L.n,
                           kl_out, B, 1.0f);
        ADVGRPO_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int advgrpo_sde_step_rescaled(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                         int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float sin_coeff,
                                         int mode, const float* eps, uint64_t seed, uint64_t offset, const void* prev_sample,
                                         int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype, float* out_mean,
                                         float* out_log_prob, float* out_std, void* workspace, int B, int C, int H, int W,
                                         int patch_size, void* stream) {
    return step_rescaled_fwd<CpsStep>("sde_step_rescaled", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                                      sigma_stride, sin_coeff, nullptr, mode, eps, seed, offset, prev_sample, prev_dtype, out_next_f32,
                                      out_next_cast, out_cast_dtype, out_mean, out_log_prob, out_std, workspace, B, C, H, W, patch_size,
                                      stream);
}

extern "C" int advgrpo_flow_sde_step_rescaled(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                              int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride,
                                              float noise_level, const float* sigma_max, int mode, const float* eps, uint64_t seed,
                                              uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                              void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                              float* out_std, void* workspace, int B, int C, int H, int W, int patch_size,
                                              void* stream) {
    return step_rescaled_fwd<FlowStep>("flow_sde_step_rescaled", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                                       sigma_stride, noise_level, sigma_max, mode, eps, seed, offset, prev_sample, prev_dtype,
                                       out_next_f32, out_next_cast, out_cast_dtype, out_mean, out_log_prob, out_std, workspace, B, C, H,
                                       W, patch_size, stream);
}

extern "C" int advgrpo_sde_step_rescaled_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                             int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride,
                                             float sin_coeff, const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                             const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                             float* kl_out, void* workspace, int B, int C, int H, int W, int patch_size,
                                             void* stream) {
    return step_rescaled_bwd<CpsStep>("sde_step_rescaled_bwd", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma, sigma_prev,
                                      sigma_stride, sin_coeff, nullptr, prev_sample, prev_dtype, grad_log_prob, mean_ref, kl_weight,
                                      grad_v_uncond, grad_v_text, kl_out, workspace, B, C, H, W, patch_size, stream);
}

extern "C" int advgrpo_flow_sde_step_rescaled_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                                  const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                                  int sigma_stride, float noise_level, const float* sigma_max,
                                                  const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                                  const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                                  float* kl_out, void* workspace, int B, int C, int H, int W, int patch_size,
                                                  void* stream) {
    return step_rescaled_bwd<FlowStep>("flow_sde_step_rescaled_bwd", v_uncond, v_text, v_dtype, guidance_scale, x, x_dtype, sigma,
                                       sigma_prev, sigma_stride, noise_level, sigma_max, prev_sample, prev_dtype, grad_log_prob,
                                       mean_ref, kl_weight, grad_v_uncond, grad_v_text, kl_out, workspace, B, C, H, W, patch_size,
                                       stream);
}

extern "C" int advgrpo_randn(void* out, int out_dtype, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    ADVGRPO_CHECK(out && n >= 0, "randn: bad argument");
    ADVGRPO_CHECK(out_dtype == ADVGRPO_F32 || out_dtype == ADVGRPO_BF16, "randn: bad dtype %d", out_dtype);
    if (n == 0) return 0;
    int64_t groups = (n + 3) / 4;
    int blocks = (int)((groups + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(randn_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), out, out_dtype, n, seed, offset);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
