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

// ---- the twelve step entries: one call block, one forward and one backward routine under them ------------------------------------
// What any of advgrpo_{,flow_}sde_step{,_branch,_bwd,_bwd_kl} and advgrpo_{,flow_}sde_step_rescaled{,_bwd} receives.  An entry fills
// it BY NAME (STEP_CALL and the macros after it: the entries spell their parameters alike, so no list is handed on by position) and
// calls step_forward or step_backward.  Where the entries' checks differ, a field below says so; none of the differences is resolved.
enum StepShape { STEP_FLAT, STEP_FAN, STEP_TOKENS };
struct StepCall {
    const char* what;           // the entry's name in error texts
    const char* common_what;    // ... in the dtype and B / n checks: "sde_step" under all eight flat and fan-out entries
    bool flow;                  // Flow-SDE: level = noise_level, sigma_max required; else Flow-CPS: level = sin_coeff, sigma_max NULL
    const float* sigma_max;
    // shared inputs
    const void *v_uncond, *v_text, *x;
    int v_dtype, x_dtype, sigma_stride;
    float guidance_scale, level;
    const float *sigma, *sigma_prev;
    // forward
    int mode, prev_dtype, out_cast_dtype;   // (prev_sample / prev_dtype: the backward's too)
    const float* eps;
    uint64_t seed, offset;
    const void* prev_sample;
    void* out_next_cast;
    float *out_next_f32, *out_mean, *out_log_prob, *out_std;
    // backward; mean_ref == NULL: the policy-only backward (kl_weight, kl_out and workspace unused)
    const float *grad_log_prob, *mean_ref;
    float kl_weight;
    void *grad_v_uncond, *grad_v_text;
    float* kl_out;
    bool need_mean_ref;         // *_bwd_kl refuse a NULL mean_ref; under *_rescaled_bwd it selects the policy-only backward
    void *workspace, *stream;
    // the shape, in one of three forms
    StepShape shape;
    bool io_dtypes;             // refuse a bad prev_dtype / out_cast_dtype: the rescaled entries only
    int B, G;                   // input rows (the fan-out entries' P) and copies per row (1 except there): B * G output rows
    int64_t n;                  // elements per row (STEP_TOKENS: from rs_layout)
    int C, H, W, patch_size;
    StepCall& flat(int B_, int64_t n_) { return shape = STEP_FLAT, common_what = "sde_step", io_dtypes = false, B = B_, G = 1, n = n_, *this; }
    StepCall& fan(int P_, int G_, int64_t n_) { return shape = STEP_FAN, common_what = "sde_step", io_dtypes = false, B = P_, G = G_, n = n_, *this; }
    StepCall& tokens(int B_, int C_, int H_, int W_, int patch_) {
        return shape = STEP_TOKENS, common_what = what, io_dtypes = true, B = B_, G = 1, n = 0, C = C_, H = H_, W = W_, patch_size = patch_, *this;
    }
};
#define STEP_CALL(c, NAME, FLOW, LEVEL, SIGMA_MAX)                                                                                  \
    StepCall c{};                                                                                                                   \
    c.what = NAME, c.flow = FLOW, c.level = LEVEL, c.sigma_max = SIGMA_MAX, c.v_uncond = v_uncond, c.v_text = v_text,               \
    c.v_dtype = v_dtype, c.guidance_scale = guidance_scale, c.x = x, c.x_dtype = x_dtype, c.sigma = sigma, c.sigma_prev = sigma_prev, \
    c.sigma_stride = sigma_stride, c.stream = stream
#define STEP_FORWARD(c)                                                                                                             \
    c.mode = mode, c.eps = eps, c.seed = seed, c.offset = offset, c.prev_sample = prev_sample, c.prev_dtype = prev_dtype,           \
    c.out_next_f32 = out_next_f32, c.out_next_cast = out_next_cast, c.out_cast_dtype = out_cast_dtype, c.out_mean = out_mean,       \
    c.out_log_prob = out_log_prob, c.out_std = out_std, c.workspace = workspace
#define STEP_BACKWARD(c)                                                                                                            \
    c.prev_sample = prev_sample, c.prev_dtype = prev_dtype, c.grad_log_prob = grad_log_prob, c.grad_v_uncond = grad_v_uncond,       \
    c.grad_v_text = grad_v_text
#define STEP_KL(c, NEED_MEAN_REF)                                                                                                   \
    c.mean_ref = mean_ref, c.kl_weight = kl_weight, c.kl_out = kl_out, c.workspace = workspace, c.need_mean_ref = NEED_MEAN_REF

struct StepGrid {
    bool pair;      // STEP_TOKENS: two tokens per lane
    int nb;         // blocks per sample
    int64_t n;      // elements per sample
};
static int fan_blocks(int G) { return (G + SDE_BRANCH_COPIES - 1) / SDE_BRANCH_COPIES; }
static int64_t rs_blocks(int H, int W, int tpl) {
    const int64_t units = (int64_t)(H / 2) * ((W / 2) / tpl);
    return (units + QS_LANES - 1) / QS_LANES;
}
static int rs_shape(const char* what, int B, int C, int H, int W, int patch_size, int sigma_stride) {
    ADVGRPO_CHECK(patch_size == 2 && C == QS_CPW * QS_WAVES, "%s: built for patch 2 and C = %d (patch=%d C=%d)", what,
                  QS_CPW * QS_WAVES, patch_size, C);
    ADVGRPO_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0 && sigma_stride >= 0,
                  "%s: need 0 < B <= 65535 and even H, W (B=%d H=%d W=%d)", what, B, H, W);
    ADVGRPO_CHECK(rs_blocks(H, W, 1) <= INT32_MAX / B, "%s: too many tokens", what);
    return 0;
}
// ptrs / sizes: every tensor the kernel reads or writes N elements at a time, with its element size (NULL entries are skipped)
static int rs_layout(const char* what, const void* const* ptrs, const int* sizes, int count, int C, int H, int W, StepGrid* L) {
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

// The checks that come before the pointers.  The fan-out entries look at P, G first, so a bad n under them reports P as "B=".
static int step_shape(const StepCall& c) {
    if (c.shape == STEP_FAN) ADVGRPO_CHECK(c.B > 0 && c.G > 0, "%s: need P>0 and G>0 (P=%d G=%d)", c.what, c.B, c.G);
    ADVGRPO_CHECK(c.v_dtype == ADVGRPO_F32 || c.v_dtype == ADVGRPO_BF16, "%s: bad v_dtype %d", c.common_what, c.v_dtype);
    ADVGRPO_CHECK(c.x_dtype == ADVGRPO_F32 || c.x_dtype == ADVGRPO_BF16, "%s: bad x_dtype %d", c.common_what, c.x_dtype);
    if (c.shape == STEP_TOKENS) return rs_shape(c.what, c.B, c.C, c.H, c.W, c.patch_size, c.sigma_stride);
    ADVGRPO_CHECK(c.B > 0 && c.n > 0 && c.n % SDE_VEC == 0, "%s: need B>0 and n %% 8 == 0 (B=%d n=%lld)", c.common_what, c.B,
                  (long long)c.n);
    if (c.shape == STEP_FAN)
        ADVGRPO_CHECK(c.B <= 65535 && fan_blocks(c.G) <= 65535 && (int64_t)c.B * c.G <= INT32_MAX, "%s: P=%d G=%d too large", c.what,
                      c.B, c.G);
    return 0;
}

template <class Step>
static int launch_forward(const StepCall& c, const StepGrid& g) {
    auto launch = [&](auto kernel, dim3 grid, int threads, auto... shape) {
        hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, as_stream(c.stream), c.v_uncond, c.v_text, c.v_dtype, c.guidance_scale, c.x,
                           c.x_dtype, c.sigma, c.sigma_prev, c.sigma_stride, c.level, c.sigma_max, c.mode, c.eps, c.seed, c.offset,
                           c.prev_sample, c.prev_dtype, c.out_next_f32, c.out_next_cast, c.out_cast_dtype, c.out_mean,
                           (float*)c.workspace, c.out_std, shape...);
    };
    if (c.shape == STEP_FLAT) launch(sde_step_kernel<Step>, dim3(g.nb, c.B), SDE_THREADS, g.n);
    else if (c.shape == STEP_FAN) launch(sde_step_branch_kernel<Step>, dim3(g.nb, c.B, fan_blocks(c.G)), SDE_THREADS, c.B, c.G, g.n);
    else if (g.pair) launch(sde_step_rescaled_kernel<Step, 2>, dim3(g.nb, c.B), QS_THREADS, c.C, c.H, c.W);
    else launch(sde_step_rescaled_kernel<Step, 1>, dim3(g.nb, c.B), QS_THREADS, c.C, c.H, c.W);
    ADVGRPO_LAUNCH_CHECK();
    const int rows = c.B * c.G;                     // output row j takes the schedule row j % B
    if (c.flow)
        hipLaunchKernelGGL(flow_sde_finalize_kernel, dim3((rows + 63) / 64), dim3(64), 0, as_stream(c.stream),
                           (const float*)c.workspace, g.nb, g.n, c.out_log_prob, rows, c.sigma, c.sigma_prev, c.sigma_stride, c.B, c.level,
                           c.sigma_max);
    else
        hipLaunchKernelGGL(sde_finalize_kernel, dim3((rows + 63) / 64), dim3(64), 0, as_stream(c.stream), (const float*)c.workspace,
                           g.nb, g.n, c.out_log_prob, rows, -1.0f);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

static int step_forward(const StepCall& c) {
    if (step_shape(c)) return -1;
    ADVGRPO_CHECK(c.v_uncond && c.x && c.sigma && c.sigma_prev && c.out_log_prob && c.workspace, "%s: null argument", c.what);
    ADVGRPO_CHECK(!c.flow || c.sigma_max, "%s: null sigma_max", c.what);
    ADVGRPO_CHECK(c.mode >= 0 && c.mode <= 2, "%s: bad mode %d", c.what, c.mode);
    ADVGRPO_CHECK(c.mode != ADVGRPO_SDE_EPS || c.eps, "%s: mode EPS needs eps", c.what);
    const bool replay = c.mode == ADVGRPO_SDE_REPLAY;
    ADVGRPO_CHECK(!replay || c.prev_sample, "%s: mode REPLAY needs prev_sample", c.what);
    if (c.io_dtypes) {
        ADVGRPO_CHECK(!replay || c.prev_dtype == ADVGRPO_F32 || c.prev_dtype == ADVGRPO_BF16, "%s: bad prev_dtype %d", c.what,
                      c.prev_dtype);
        ADVGRPO_CHECK(!c.out_next_cast || replay || c.out_cast_dtype == ADVGRPO_F32 || c.out_cast_dtype == ADVGRPO_BF16,
                      "%s: bad out_cast_dtype %d", c.what, c.out_cast_dtype);
    }
    StepGrid g{false, sde_blocks(c.n), c.n};
    if (c.shape == STEP_TOKENS) {
        const void* ptrs[] = {c.v_uncond, c.v_text, c.x, c.mode == ADVGRPO_SDE_EPS ? c.eps : nullptr, replay ? c.prev_sample : nullptr,
                              replay ? nullptr : c.out_next_f32, replay ? nullptr : c.out_next_cast, c.out_mean};
        const int sizes[] = {dtype_size(c.v_dtype), dtype_size(c.v_dtype), dtype_size(c.x_dtype), 4, dtype_size(c.prev_dtype), 4,
                             dtype_size(c.out_cast_dtype), 4};
        if (rs_layout(c.what, ptrs, sizes, 8, c.C, c.H, c.W, &g)) return -1;
    }
    return c.flow ? launch_forward<FlowStep>(c, g) : launch_forward<CpsStep>(c, g);
}

template <class Step>
static int launch_backward(const StepCall& c, const StepGrid& g) {
    const float kl_weight = c.mean_ref ? c.kl_weight : 0.f;
    float* kl_partial = c.mean_ref ? (float*)c.workspace : nullptr;
    if (c.shape == STEP_TOKENS) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(g.nb, c.B), dim3(QS_THREADS), 0, as_stream(c.stream), c.v_uncond, c.v_text, c.v_dtype,
                               c.guidance_scale, c.x, c.x_dtype, c.sigma, c.sigma_prev, c.sigma_stride, c.level, c.sigma_max, c.prev_sample,
                               c.prev_dtype, c.grad_log_prob, c.grad_v_uncond, c.grad_v_text, c.C, c.H, c.W, c.mean_ref, kl_weight, c.B,
                               kl_partial);
        };
        if (g.pair) launch(sde_step_rescaled_bwd_kernel<Step, 2>);
        else launch(sde_step_rescaled_bwd_kernel<Step, 1>);
    } else {
        hipLaunchKernelGGL(sde_step_bwd_kernel<Step>, dim3(g.nb, c.B), dim3(SDE_THREADS), 0, as_stream(c.stream), c.v_uncond, c.v_text,
                           c.v_dtype, c.guidance_scale, c.x, c.x_dtype, c.sigma, c.sigma_prev, c.sigma_stride, c.level, c.sigma_max,
                           c.prev_sample, c.prev_dtype, c.grad_log_prob, c.grad_v_uncond, c.grad_v_text, g.n, c.mean_ref, kl_weight, c.B,
                           kl_partial);
    }
    ADVGRPO_LAUNCH_CHECK();
    if (c.mean_ref) {       // the per-sample KL values from the block partials
        hipLaunchKernelGGL(sde_finalize_kernel, dim3((c.B + 63) / 64), dim3(64), 0, as_stream(c.stream), (const float*)c.workspace, g.nb,
                           g.n, c.kl_out, c.B, 1.0f);
        ADVGRPO_LAUNCH_CHECK();
    }
    return 0;
}

static int step_backward(const StepCall& c) {
    if (step_shape(c)) return -1;
    ADVGRPO_CHECK(c.v_uncond && c.x && c.sigma && c.sigma_prev && c.prev_sample && c.grad_log_prob && c.grad_v_uncond &&
                      (!c.need_mean_ref || c.mean_ref) && (!c.mean_ref || (c.kl_out && c.workspace)), "%s: null argument", c.what);
    ADVGRPO_CHECK(!c.flow || c.sigma_max, "%s: null sigma_max", c.what);
    if (c.io_dtypes) ADVGRPO_CHECK(c.prev_dtype == ADVGRPO_F32 || c.prev_dtype == ADVGRPO_BF16, "%s: bad prev_dtype %d", c.what, c.prev_dtype);
    ADVGRPO_CHECK(!c.v_text || c.grad_v_text, "%s: CFG needs grad_v_text", c.what);
    StepGrid g{false, sde_blocks(c.n), c.n};
    if (c.shape == STEP_TOKENS) {
        const void* ptrs[] = {c.v_uncond, c.v_text, c.x, c.prev_sample, c.mean_ref, c.grad_v_uncond, c.v_text ? c.grad_v_text : nullptr};
        const int sizes[] = {dtype_size(c.v_dtype), dtype_size(c.v_dtype), dtype_size(c.x_dtype), dtype_size(c.prev_dtype), 4,
                             dtype_size(c.v_dtype), dtype_size(c.v_dtype)};
        if (rs_layout(c.what, ptrs, sizes, 7, c.C, c.H, c.W, &g)) return -1;
    }
    return c.flow ? launch_backward<FlowStep>(c, g) : launch_backward<CpsStep>(c, g);
}

extern "C" int advgrpo_sde_step(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                int sigma_stride, float sin_coeff, int mode, const float* eps, uint64_t seed,
                                uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                float* out_std, void* workspace, int B, int64_t n, void* stream) {
    STEP_CALL(c, "sde_step", false, sin_coeff, nullptr);
    STEP_FORWARD(c);
    return step_forward(c.flat(B, n));
}

extern "C" int advgrpo_sde_step_branch(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                       const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                       int sigma_stride, float sin_coeff, int mode, const float* eps, uint64_t seed,
                                       uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                       void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                       float* out_std, void* workspace, int P, int G, int64_t n, void* stream) {
    STEP_CALL(c, "sde_step_branch", false, sin_coeff, nullptr);
    STEP_FORWARD(c);
    return step_forward(c.fan(P, G, n));
}

extern "C" int advgrpo_sde_step_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                    const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                    int sigma_stride, float sin_coeff, const void* prev_sample, int prev_dtype,
                                    const float* grad_log_prob, void* grad_v_uncond, void* grad_v_text, int B,
                                    int64_t n, void* stream) {
    STEP_CALL(c, "sde_step_bwd", false, sin_coeff, nullptr);
    STEP_BACKWARD(c);
    return step_backward(c.flat(B, n));
}

extern "C" int advgrpo_sde_step_bwd_kl(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                       const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                       int sigma_stride, float sin_coeff, const void* prev_sample, int prev_dtype,
                                       const float* grad_log_prob, const float* mean_ref, float kl_weight,
                                       void* grad_v_uncond, void* grad_v_text, float* kl_out, void* workspace, int B,
                                       int64_t n, void* stream) {
    STEP_CALL(c, "sde_step_bwd_kl", false, sin_coeff, nullptr);
    STEP_BACKWARD(c);
    STEP_KL(c, true);
    return step_backward(c.flat(B, n));
}

extern "C" int advgrpo_flow_sde_step(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                     const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                     int sigma_stride, float noise_level, const float* sigma_max, int mode, const float* eps,
                                     uint64_t seed, uint64_t offset, const void* prev_sample, int prev_dtype,
                                     float* out_next_f32, void* out_next_cast, int out_cast_dtype, float* out_mean,
                                     float* out_log_prob, float* out_std, void* workspace, int B, int64_t n, void* stream) {
    STEP_CALL(c, "flow_sde_step", true, noise_level, sigma_max);
    STEP_FORWARD(c);
    return step_forward(c.flat(B, n));
}

extern "C" int advgrpo_flow_sde_step_branch(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                            const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                            int sigma_stride, float noise_level, const float* sigma_max, int mode,
                                            const float* eps, uint64_t seed, uint64_t offset, const void* prev_sample,
                                            int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype,
                                            float* out_mean, float* out_log_prob, float* out_std, void* workspace, int P, int G,
                                            int64_t n, void* stream) {
    STEP_CALL(c, "flow_sde_step_branch", true, noise_level, sigma_max);
    STEP_FORWARD(c);
    return step_forward(c.fan(P, G, n));
}

extern "C" int advgrpo_flow_sde_step_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                         const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                         int sigma_stride, float noise_level, const float* sigma_max, const void* prev_sample,
                                         int prev_dtype, const float* grad_log_prob, void* grad_v_uncond, void* grad_v_text,
                                         int B, int64_t n, void* stream) {
    STEP_CALL(c, "flow_sde_step_bwd", true, noise_level, sigma_max);
    STEP_BACKWARD(c);
    return step_backward(c.flat(B, n));
}

extern "C" int advgrpo_flow_sde_step_bwd_kl(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                            const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                            int sigma_stride, float noise_level, const float* sigma_max,
                                            const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                            const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                            float* kl_out, void* workspace, int B, int64_t n, void* stream) {
    STEP_CALL(c, "flow_sde_step_bwd_kl", true, noise_level, sigma_max);
    STEP_BACKWARD(c);
    STEP_KL(c, true);
    return step_backward(c.flat(B, n));
}

extern "C" int advgrpo_sde_step_rescaled(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                         int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride, float sin_coeff,
                                         int mode, const float* eps, uint64_t seed, uint64_t offset, const void* prev_sample,
                                         int prev_dtype, float* out_next_f32, void* out_next_cast, int out_cast_dtype, float* out_mean,
                                         float* out_log_prob, float* out_std, void* workspace, int B, int C, int H, int W,
                                         int patch_size, void* stream) {
    STEP_CALL(c, "sde_step_rescaled", false, sin_coeff, nullptr);
    STEP_FORWARD(c);
    return step_forward(c.tokens(B, C, H, W, patch_size));
}

extern "C" int advgrpo_flow_sde_step_rescaled(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                              int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride,
                                              float noise_level, const float* sigma_max, int mode, const float* eps, uint64_t seed,
                                              uint64_t offset, const void* prev_sample, int prev_dtype, float* out_next_f32,
                                              void* out_next_cast, int out_cast_dtype, float* out_mean, float* out_log_prob,
                                              float* out_std, void* workspace, int B, int C, int H, int W, int patch_size,
                                              void* stream) {
    STEP_CALL(c, "flow_sde_step_rescaled", true, noise_level, sigma_max);
    STEP_FORWARD(c);
    return step_forward(c.tokens(B, C, H, W, patch_size));
}

extern "C" int advgrpo_sde_step_rescaled_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale, const void* x,
                                             int x_dtype, const float* sigma, const float* sigma_prev, int sigma_stride,
                                             float sin_coeff, const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                             const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                             float* kl_out, void* workspace, int B, int C, int H, int W, int patch_size,
                                             void* stream) {
    STEP_CALL(c, "sde_step_rescaled_bwd", false, sin_coeff, nullptr);
    STEP_BACKWARD(c);
    STEP_KL(c, false);
    return step_backward(c.tokens(B, C, H, W, patch_size));
}

extern "C" int advgrpo_flow_sde_step_rescaled_bwd(const void* v_uncond, const void* v_text, int v_dtype, float guidance_scale,
                                                  const void* x, int x_dtype, const float* sigma, const float* sigma_prev,
                                                  int sigma_stride, float noise_level, const float* sigma_max,
                                                  const void* prev_sample, int prev_dtype, const float* grad_log_prob,
                                                  const float* mean_ref, float kl_weight, void* grad_v_uncond, void* grad_v_text,
                                                  float* kl_out, void* workspace, int B, int C, int H, int W, int patch_size,
                                                  void* stream) {
    STEP_CALL(c, "flow_sde_step_rescaled_bwd", true, noise_level, sigma_max);
    STEP_BACKWARD(c);
    STEP_KL(c, false);
    return step_backward(c.tokens(B, C, H, W, patch_size));
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
