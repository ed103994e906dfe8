// attention_gqa.hip -- fused causal grouped-query self-attention at head dim 128 for gfx950: o = softmax(scale q k^T [causal]) v with Hq query
// heads over Hkv key/value heads (query head h reads key/value head h / (Hq / Hkv)), bf16 in/out, f32 scores / exponentials / row maximum /
// row sum, probabilities rounded to bf16 before P V, the quotient rounded to bf16.
//
// Serves the Qwen2.5-VL language model behind Qwen-Image's encode_prompt (28 query heads over 4 key/value heads of 128; the prompt encoder
// of BASELINE config 5, adv_grpo_amd/qwen_text_encoder.py): the packed q | k | v GEMM output is read in place, no head-major copies, no
// repeat_interleave of K / V, no materialised scores -- and no 512-token cap.
//
// Mapping (wave64, v_mfma_f32_16x16x32_bf16; the fragment layouts and the tile step -- mask, online softmax, P V, epilogue -- are attention.hpp's):
//   * a workgroup (4 waves) serves one (batch, key/value head, chunk of up to 8 query heads of the group, block of query positions) and
//     stages each 64-key K and V tile in LDS ONCE for all of them: with 7 query heads per key/value head a K / V byte is fetched once
//     where the materialised path made 7 copies.
//   * the work is cut into 8 units of 32 rows (one query head x 32 positions); wave w owns units w and w + 4.  With g = min(Hq / Hkv, 8)
//     heads in the chunk a workgroup covers 8 / g blocks of 32 positions (g = 1: 256 positions of one head, g = 7: 32 positions of 7 heads,
//     one unit idle).
//   * both LDS tiles use a 272-byte row pitch (an odd multiple of 16 bytes).
//   * ordinary online softmax: a running maximum with a rescale of O and of the row sum per tile.  No first-tile-maximum shortcut, hence
//     no fallback path and no fallback counter.
//   * causal: key tiles above the workgroup's last query position are never staged, a unit skips the tiles above its own last position,
//     and the diagonal and the ragged last tile are masked before the row maximum.
//   * K / V tiles are register staged: the next tile's global loads are issued before the current tile's MFMAs and written to LDS
//     afterwards (single LDS buffer of 34 KiB, two barriers per tile).  Two units per wave cost about 440 registers per lane: one workgroup
//     per CU.  Prompt encoding runs once per prompt; the kernel is written for the shared K / V tile and for having no cap, not for peak speed.
// Every offset into q / k / v / o is 64-bit.
#include "attention.hpp"

namespace advgrpo {

struct GqaParams {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int64_t ldq, ldk, ldv, ldo;   // row pitch (elements)
    int64_t bsq, bsk, bsv, bso;   // batch pitch (elements)
    int Hq, Hkv, S;
    float scale_log2e;            // softmax scale * log2(e)
    int causal;
    int gc;                       // query heads of a group per workgroup (<= 8)
    int nchunk;                   // workgroups per group along the heads: ceil((Hq / Hkv) / gc)
    int psb;                      // blocks of 32 query positions per workgroup: 8 / gc
    int npb;                      // workgroups along the positions: ceil(S / (32 psb))
};

constexpr int GQA_HD = 128;
constexpr int GQA_UNITS = 8;      // 32-row units per workgroup
constexpr int GQA_UPW = 2;        // units per wave
constexpr int GQA_QP = 32;        // query positions per unit

__global__ __launch_bounds__(256) void attention_fwd_gqa_kernel(const GqaParams p) {
    constexpr int HD = GQA_HD, KS = HD / 32, DB = HD / 16;
    constexpr int PITCH = HD + 8;                   // LDS row pitch in elements: 272 bytes
    constexpr int CPR = HD / 8;                     // 16-byte chunks per row
    constexpr int NCH = ATT_KB * CPR / 256;         // staging chunks per thread (4)
    constexpr int TILE = ATT_KB * PITCH;
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * TILE];      // K, V
    bf16_t* Ks = smem;
    bf16_t* Vs = smem + TILE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, t = lane & 15;
    const int G = p.Hq / p.Hkv;
    int idx = blockIdx.x;
    const int pblk = idx % p.npb; idx /= p.npb;
    const int chunk = idx % p.nchunk; idx /= p.nchunk;
    const int kvh = idx % p.Hkv;
    const int b = idx / p.Hkv;

    const bf16_t* kp = p.k + (int64_t)b * p.bsk + kvh * HD;
    const bf16_t* vp = p.v + (int64_t)b * p.bsv + kvh * HD;

    // ---- this wave's units: (query head, first position); a unit past the group's heads or past the sequence idles (wave-uniform)
    bool active[GQA_UPW];
    int head[GQA_UPW], q0[GQA_UPW];
    bf16x8_t qf[GQA_UPW][2][KS];     // B operand: lane = query t, 8 consecutive d at ks*32 + g*8
#pragma unroll
    for (int j = 0; j < GQA_UPW; ++j) {
        const int u = wave + 4 * j;
        const int hic = chunk * p.gc + u % p.gc, sub = u / p.gc;
        head[j] = kvh * G + hic;
        q0[j] = (pblk * p.psb + sub) * GQA_QP;
        active[j] = sub < p.psb && hic < G && q0[j] < p.S;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) qf[j][qb][ks] = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
        if (active[j]) {
            const bf16_t* qp = p.q + (int64_t)b * p.bsq + head[j] * HD;
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                int qr = q0[j] + qb * 16 + t;
                qr = qr < p.S ? qr : p.S - 1;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    qf[j][qb][ks] = *reinterpret_cast<const bf16x8_t*>(qp + (int64_t)qr * p.ldq + ks * 32 + g * 8);
            }
        }
    }

    // ---- staging: 64 rows x 16 chunks of 16 bytes per tile, 4 per thread for K and for V (rows past the sequence re-read the last row)
    // (named values, not arrays: across the tile's MFMAs the compiler keeps staging ARRAYS in scratch)
    static_assert(NCH == 4, "the staging below is written out for 4 chunks per thread");
    uint4 k0, k1, k2, k3, v0, v1, v2, v3;
    auto src = [&](const bf16_t* base, int64_t ld, int kv0, int i) {
        const int c = tid + i * 256;
        int r = kv0 + c / CPR;
        r = r < p.S ? r : p.S - 1;
        return *reinterpret_cast<const uint4*>(base + (int64_t)r * ld + (c % CPR) * 8);
    };
    auto dst = [&](bf16_t* base, int i, const uint4& val) {
        const int c = tid + i * 256;
        *reinterpret_cast<uint4*>(base + (c / CPR) * PITCH + (c % CPR) * 8) = val;
    };
#define GQA_ISSUE(kv0)                                                                                          \
    k0 = src(kp, p.ldk, kv0, 0); k1 = src(kp, p.ldk, kv0, 1); k2 = src(kp, p.ldk, kv0, 2); k3 = src(kp, p.ldk, kv0, 3); \
    v0 = src(vp, p.ldv, kv0, 0); v1 = src(vp, p.ldv, kv0, 1); v2 = src(vp, p.ldv, kv0, 2); v3 = src(vp, p.ldv, kv0, 3);
#define GQA_COMMIT()                                                          \
    dst(Ks, 0, k0); dst(Ks, 1, k1); dst(Ks, 2, k2); dst(Ks, 3, k3);           \
    dst(Vs, 0, v0); dst(Vs, 1, v1); dst(Vs, 2, v2); dst(Vs, 3, v3);

    f32x4 o[GQA_UPW][DB][2];
    float m_run[GQA_UPW][2], l_run[GQA_UPW][2];
#pragma unroll
    for (int j = 0; j < GQA_UPW; ++j) {
#pragma unroll
        for (int i = 0; i < DB; ++i)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) o[j][i][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) { m_run[j][qb] = -INFINITY; l_run[j][qb] = 0.f; }
    }

    int kv_end = p.S;
    if (p.causal) kv_end = min(kv_end, (pblk + 1) * p.psb * GQA_QP);      // keys <= the last query position of the workgroup
    const int nt = (kv_end + ATT_KB - 1) / ATT_KB;

    GQA_ISSUE(0)
    GQA_COMMIT()
    __syncthreads();
    for (int it = 0; it < nt; ++it) {
        const int kv0 = it * ATT_KB;
        if (it + 1 < nt) { GQA_ISSUE(kv0 + ATT_KB) }
#pragma unroll
        for (int j = 0; j < GQA_UPW; ++j) {
            if (!active[j]) continue;                                     // wave-uniform
            if (p.causal && kv0 > q0[j] + GQA_QP - 1) continue;           // the whole tile lies above this unit's last query
            // ---- S^T[key][q] = K Q^T
            f32x4 s[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb) s[i][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8_t kf[4];
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) kf[kb] = *reinterpret_cast<const bf16x8_t*>(Ks + (kb * 16 + t) * PITCH + ks * 32 + g * 8);
#pragma unroll
                for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        s[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb], qf[j][qb][ks], s[kb][qb], 0, 0, 0);
            }
            // lane holds S[key = kv0 + kb*16 + g*4 + r][query = q0 + qb*16 + t]
            const bool edge = (kv0 + ATT_KB > p.S) || (p.causal && kv0 + ATT_KB - 1 > q0[j]);
            if (edge) ADVGRPO_MASK_SCORES(s, 2, kv0, q0[j], p.S, p.causal, g, t);
            // ordinary online softmax with a running maximum (no first-tile-maximum shortcut)
            bf16x8_t pf[2][2];  // [qb][key pair]
            ADVGRPO_SOFTMAX_TILE(s, 2, DB, m_run[j], l_run[j], o[j], p.scale_log2e, pf);
            ADVGRPO_PV_TILE(Vs, PITCH, 2, DB, pf, o[j], 4, g, t);
        }
        __syncthreads();                 // every wave has read the tile
        if (it + 1 < nt) { GQA_COMMIT() }
        __syncthreads();
    }

#undef GQA_ISSUE
#undef GQA_COMMIT

#pragma unroll
    for (int j = 0; j < GQA_UPW; ++j) {
        if (!active[j]) continue;
        ADVGRPO_STORE_ROWS(HD, 2, DB, o[j], l_run[j], m_run[j], p.o + (int64_t)b * p.bso, p.ldo, head[j] * HD, (float*)nullptr, 0, q0[j], p.S, g, t);
    }
}

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_attention_fwd_gqa(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                         int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, int B, int Hq, int Hkv, int S, int head_dim,
                                         float scale, int causal, void* stream) {
    ADVGRPO_CHECK(q, "attention_fwd_gqa: null pointer (q)");
    ADVGRPO_CHECK(k, "attention_fwd_gqa: null pointer (k)");
    ADVGRPO_CHECK(v, "attention_fwd_gqa: null pointer (v)");
    ADVGRPO_CHECK(o, "attention_fwd_gqa: null pointer (o)");
    ADVGRPO_CHECK(head_dim == GQA_HD, "attention_fwd_gqa: head_dim %d not supported (128)", head_dim);
    ADVGRPO_CHECK(B > 0 && Hq > 0 && Hkv > 0 && S > 0, "attention_fwd_gqa: bad shape (B=%d Hq=%d Hkv=%d S=%d)", B, Hq, Hkv, S);
    ADVGRPO_CHECK(Hq % Hkv == 0, "attention_fwd_gqa: %d query heads are not a multiple of %d key/value heads", Hq, Hkv);
    ADVGRPO_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && bsq % 8 == 0 && bsk % 8 == 0 && bsv % 8 == 0 && bso % 8 == 0,
                  "attention_fwd_gqa: row and batch pitches must be multiples of 8 elements (16-byte rows)");
    ADVGRPO_CHECK(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o)) & 15) == 0,
                  "attention_fwd_gqa: q, k, v and o must be 16-byte aligned");
    ADVGRPO_CHECK(ldq >= (int64_t)Hq * GQA_HD && ldo >= (int64_t)Hq * GQA_HD && ldk >= (int64_t)Hkv * GQA_HD && ldv >= (int64_t)Hkv * GQA_HD,
                  "attention_fwd_gqa: a row pitch is smaller than its heads");
    GqaParams p{};
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso;
    p.Hq = Hq; p.Hkv = Hkv; p.S = S;
    p.scale_log2e = scale * 1.4426950408889634f;
    p.causal = causal != 0;
    const int G = Hq / Hkv;
    p.gc = G < GQA_UNITS ? G : GQA_UNITS;
    p.nchunk = (G + p.gc - 1) / p.gc;
    p.psb = GQA_UNITS / p.gc;
    p.npb = (S + p.psb * GQA_QP - 1) / (p.psb * GQA_QP);
    const int64_t nwg = (int64_t)B * Hkv * p.nchunk * p.npb;
    ADVGRPO_CHECK(nwg < (1ll << 31), "attention_fwd_gqa: grid too large");
    hipLaunchKernelGGL(attention_fwd_gqa_kernel, dim3((unsigned)nwg), dim3(256), 0, as_stream(stream), p);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
