// attention.hpp -- parameter block, lane-swap helpers and the online-softmax tile step shared by the attention forward kernels.
#pragma once
#include "common.hpp"
#include "gemm.hpp"

namespace advgrpo {

struct AttnParams {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int64_t ldq, ldk, ldv, ldo;   // row pitch (elements)
    int64_t bsq, bsk, bsv, bso;   // batch pitch (elements)
    int H, Sq, Skv;
    float scale_log2e;            // softmax scale * log2(e)
    int causal;
    float* lse;                   // optional [B,H,Sq]: base-2 log-sum-exp of the scaled scores (for backward)
    const float* bias;            // optional additive score bias [H,Sq,Skv] f32 (T5 relative position bias), head dim 64 only
    int nqb, nwg, xcd_local;      // query blocks per (b,h); workgroups in the 1-D grid; XCD-local block order (common.hpp)
};

// the head-dim-128 kernel with per-sample lengths: the same block + the lengths (int32 [B] on the device)
struct AttnVarlenParams : AttnParams {
    const int* seq_lens;
};

constexpr int ATT_QB = 128;   // queries per workgroup
constexpr int ATT_KB = 64;    // keys per tile

// xor-16 / xor-32 lane exchanges on the VALU (gfx950 v_permlane{16,32}_swap) instead of ds_bpermute.
// v_permlane32_swap d, s: d[32..63] <-> s[0..31]; with d = s = v the pair (d, s) afterwards holds, in every lane,
// the lane's value and its xor-32 partner's (16: odd 16-lane rows of d <-> even rows of s).
// (inline asm with two read-write operands: given the same value twice the builtin form is folded onto ONE
// register and returns the swap of a register with itself -- checked with scripts/probes/permlane_probe.hip)
#define ADVGRPO_SWAP16(a, b) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b))
#define ADVGRPO_SWAP32(a, b) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b))
__device__ __forceinline__ float xor16_max(float v) { float a = v, b = v; ADVGRPO_SWAP16(a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xor32_max(float v) { float a = v, b = v; ADVGRPO_SWAP32(a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xor16_add(float v) { float a = v, b = v; ADVGRPO_SWAP16(a, b); return a + b; }
__device__ __forceinline__ float xor32_add(float v) { float a = v, b = v; ADVGRPO_SWAP32(a, b); return a + b; }

// ------------------------------------------------------------------------------------------------------------
// The tile step of the running-maximum forward kernels (attention_fwd_kernel, attention_fwd_resident_kernel, attention_fwd_gqa_kernel;
// attention_fwd_glds_kernel uses the mask only): one 64-key tile against NQB blocks of 16 queries of one wave.
//
// Layout (wave64, v_mfma_f32_16x16x32_bf16, lane = (g, t) = (lane >> 4, lane & 15)):
//   * S^T = K Q^T is computed with K as the MFMA A operand, so a lane holds scores of ONE query (column t) for 16 keys:
//     s[kb][qb][r] = S[key = kv0 + kb*16 + g*4 + r][query = q0 + qb*16 + t].  Row max / row sum are in-lane plus two cross-lane
//     steps, and the probabilities are already in the B-operand layout of the P V product -- no LDS round trip and no permutes
//     between the two MFMAs.
//   * pf[qb][kpair] packs key blocks 2 kpair and 2 kpair + 1 into one 32-deep B fragment; the V^T fragment of the same step is
//     read (ds_read_b64_tr_b16, hardware transpose of the row-major V tile) from rows (2 kpair)*16 + g*4 + .. and 16 rows further
//     on: the key order inside a 32-deep MFMA step is permuted consistently on the P and the V side, which a sum over keys does
//     not see.
//   * O is kept transposed in the accumulators, o[db][qb][r] = O[query = q0 + qb*16 + t][d = db*16 + g*4 + r]: the online-softmax
//     rescale is a per-lane scalar and the epilogue is an 8-byte bf16x4 store per lane.
// The four pieces are statement macros, not function templates: the compiler optimises an always-inline function on its own before
// it inlines it, and every kernel came out of that with other branches and register counts than with the step written out (LABNOTES,
// "One online-softmax tile step"); as macros the kernels' device code is unchanged, instruction for instruction.  Arguments are
// evaluated more than once and the bodies declare short local names (kb, qb, r, db, kpair, key, qi, l, v, ...): pass array names,
// parameter fields and plain index expressions.

// -inf where key >= Skv or (causal) key > query.  Goes under the kernel's own wave-uniform "this tile has an edge" test.
#define ADVGRPO_MASK_SCORES(s, NQB, kv0, q0, Skv, causal, g, t)                                                                   \
    _Pragma("unroll") for (int kb = 0; kb < 4; ++kb)                                                                             \
    _Pragma("unroll") for (int qb = 0; qb < (NQB); ++qb)                                                                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                              \
        const int key = (kv0) + kb * 16 + (g) * 4 + r;                                                                           \
        const int qi = (q0) + qb * 16 + (t);                                                                                     \
        if (key >= (Skv) || ((causal) && key > qi)) s[kb][qb][r] = -INFINITY;                                                    \
    }

// online softmax (base-2), per query block: the new running maximum, l_run and O rescaled by alpha, p = exp2(s * scale - m) added to
// l_run (per lane: the cross-lane sum waits for the epilogue) and packed into pf, the two B fragments of P V
#define ADVGRPO_SOFTMAX_TILE(s, NQB, DB, m_run, l_run, o, scale_log2e, pf)                                                        \
    _Pragma("unroll") for (int qb = 0; qb < (NQB); ++qb) {                                                                       \
        float mx = -INFINITY;                                                                                                    \
        _Pragma("unroll") for (int kb = 0; kb < 4; ++kb)                                                                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kb][qb][r]);                                              \
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));                                                                                  \
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                                                                                  \
        const float m_new = fmaxf(m_run[qb], mx * (scale_log2e));                                                                \
        const float m_use = (m_new == -INFINITY) ? 0.f : m_new; /* fully masked so far */                                        \
        const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_use);                                                           \
        m_run[qb] = m_new;                                                                                                       \
        float psum = 0.f;                                                                                                        \
        float pv[4][4];                                                                                                          \
        _Pragma("unroll") for (int kb = 0; kb < 4; ++kb)                                                                         \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                          \
            const float e = __builtin_amdgcn_exp2f(s[kb][qb][r] * (scale_log2e) - m_use);                                        \
            pv[kb][r] = e;                                                                                                       \
            psum += e;                                                                                                           \
        }                                                                                                                        \
        l_run[qb] = l_run[qb] * alpha + psum;                                                                                    \
        _Pragma("unroll") for (int db = 0; db < (DB); ++db) o[db][qb] *= alpha;                                                  \
        _Pragma("unroll") for (int kpair = 0; kpair < 2; ++kpair) {                                                              \
            bf16x8_t f;                                                                                                          \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                      \
                f[r] = (__bf16)pv[2 * kpair][r];                                                                                 \
                f[4 + r] = (__bf16)pv[2 * kpair + 1][r];                                                                         \
            }                                                                                                                    \
            pf[qb][kpair] = f;                                                                                                   \
        }                                                                                                                        \
    }

// O^T[d][q] += V^T P^T over the row-major V tile at Vt (row pitch in elements).  nkb = 16-key blocks of the tile that hold a key
// (wave-uniform): a pair of blocks behind them is skipped, it would add zeros.  A literal 4 folds the test away.
#define ADVGRPO_PV_TILE(Vt, pitch, NQB, DB, pf, o, nkb, g, t)                                                                     \
    _Pragma("unroll") for (int kpair = 0; kpair < 2; ++kpair) {                                                                  \
        if (2 * kpair < (nkb)) {                                                                                                 \
            _Pragma("unroll") for (int db = 0; db < (DB); ++db) {                                                                \
                const bf16_t* a0 = (Vt) + ((2 * kpair) * 16 + (g) * 4 + ((t) >> 2)) * (pitch) + db * 16 + ((t) & 3) * 4;         \
                const bf16x8_t vf = ld_tr_frag(a0, a0 + 16 * (pitch));                                                           \
                _Pragma("unroll") for (int qb = 0; qb < (NQB); ++qb)                                                             \
                    o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb][kpair], o[db][qb], 0, 0, 0);                  \
            }                                                                                                                    \
        }                                                                                                                        \
    }

// epilogue: normalise and store bf16x4 (query q0 + qb*16 + t, d = db*16 + g*4 .. +3) at obase + query * ldo + col0, col0 the head's
// first column.  Of a head whose HD is no multiple of 16 (72) the last block's padding columns are not stored: the output is packed
// [.., H * HD], so a wider store would overwrite the next head.  lse (a float*, may be null): lse[lse_row + query] = m + log2(l).
#define ADVGRPO_STORE_ROWS(HD, NQB, DB, o, l_run, m_run, obase, ldo, col0, lse, lse_row, q0, Sq, g, t)                            \
    _Pragma("unroll") for (int qb = 0; qb < (NQB); ++qb) {                                                                       \
        float l = l_run[qb];                                                                                                     \
        l += __shfl_xor(l, 16, 64);                                                                                              \
        l += __shfl_xor(l, 32, 64);                                                                                              \
        const float inv = l > 0.f ? 1.0f / l : 0.f;                                                                              \
        const int qi = (q0) + qb * 16 + (t);                                                                                     \
        if (qi >= (Sq)) continue;                                                                                                \
        if ((lse) && (g) == 0) (lse)[(lse_row) + qi] = m_run[qb] + __builtin_amdgcn_logf(l);                                     \
        bf16_t* op = (obase) + (int64_t)qi * (ldo) + (col0) + (g) * 4;                                                           \
        _Pragma("unroll") for (int db = 0; db < (DB); ++db) {                                                                    \
            if (db * 16 + (g) * 4 >= (HD)) continue; /* HD = 72: lanes g >= 2 of the last block hold padding columns */          \
            const f32x4 v = o[db][qb] * inv;                                                                                     \
            *reinterpret_cast<uint2*>(op + db * 16) = pack4(v[0], v[1], v[2], v[3]);                                             \
        }                                                                                                                        \
    }

// the software-pipelined head-dim-64 forward (attention_pipe.hip): non-causal, no score bias, 16-byte aligned output rows
int attention_fwd_pipe_launch(const AttnParams& p, hipStream_t s);
// head dim 128 (attention_d128.hip): 8-wave workgroups of 256 queries, non-causal, no score bias, 16-byte aligned output rows
int attention_fwd_d128_launch(const AttnParams& p, int B, hipStream_t s);
// the same with per-sample lengths read from a device array (self-attention, p.Sq == p.Skv = the padded length): sample b is computed as
// if launched alone at seq_lens[b] (clamped into [1, S]); the rows beyond it are written as zeros
int attention_fwd_d128_varlen_launch(const AttnParams& p, int B, const int* seq_lens, hipStream_t s);
// workgroups of the two kernels above that took their running-maximum fallback since the last reset (host call, synchronises)
int attention_pipe_fallbacks(unsigned long long* out, int reset);
int attention_d128_fallbacks(unsigned long long* out, int reset);

}  // namespace advgrpo
