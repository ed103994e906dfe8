// attention_varlen.hip -- the C entries of the head-dim-128 attention with per-sample lengths, and the kernel that turns a prompt mask
// into those lengths.
//
// The Qwen-Image MMDiT attends over [image rows ; text rows] with right-padded prompts: the valid rows of sample b are the prefix
// 0 .. L[b] - 1, L[b] = N_img + text_len[b].  diffusers' QwenImagePipeline masks the padding keys (encoder_hidden_states_mask); here the
// kernels of attention_d128.hip / attention_bwd_d128.hip read L[b] from a device array and compute sample b exactly as if it had been
// launched alone at that length.  The lengths are read on the device at run time: no host sync, and a captured graph follows them.
#include "attention_bwd.hpp"

namespace advgrpo {

namespace {

// one wave per mask row: lead = index of the first zero (Nt when there is none), bad = a non-zero behind it, or lead == 0
template <typename T>
__global__ __launch_bounds__(256) void mask_to_seq_lens_kernel(const T* __restrict__ mask, int* __restrict__ seq_lens, int B, int Nt, int base,
                                                               int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const T* row = mask + (int64_t)b * Nt;
    int first_zero = Nt, last_set = -1;
    for (int i = lane; i < Nt; i += 64) {
        if (row[i] != (T)0) last_set = i;                   // (ascending per lane: the last hit is the lane's largest)
        else if (first_zero == Nt) first_zero = i;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        first_zero = min(first_zero, __shfl_xor(first_zero, m, 64));
        last_set = max(last_set, __shfl_xor(last_set, m, 64));
    }
    if (lane == 0) {
        seq_lens[b] = base + first_zero;
        if (bad && (first_zero == 0 || last_set > first_zero)) atomicAdd(bad, 1);
    }
}

}  // namespace

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_mask_to_seq_lens(const void* mask, int mask_dtype, int* seq_lens, int B, int Nt, int base, int* bad, void* stream) {
    ADVGRPO_CHECK(mask && seq_lens, "mask_to_seq_lens: null pointer (mask or seq_lens)");
    ADVGRPO_CHECK(mask_dtype == ADVGRPO_U8 || mask_dtype == ADVGRPO_I32 || mask_dtype == ADVGRPO_I64,
                  "mask_to_seq_lens: mask_dtype %d not supported (ADVGRPO_U8, ADVGRPO_I32, ADVGRPO_I64)", mask_dtype);
    ADVGRPO_CHECK(B > 0 && Nt > 0 && base >= 0 && (int64_t)base + Nt < (1ll << 31), "mask_to_seq_lens: bad shape (B=%d Nt=%d base=%d)", B, Nt, base);
    const dim3 grid((unsigned)((B + 3) / 4));
    hipStream_t s = as_stream(stream);
    if (mask_dtype == ADVGRPO_U8) hipLaunchKernelGGL(mask_to_seq_lens_kernel<uint8_t>, grid, dim3(256), 0, s, (const uint8_t*)mask, seq_lens, B, Nt, base, bad);
    else if (mask_dtype == ADVGRPO_I32) hipLaunchKernelGGL(mask_to_seq_lens_kernel<int32_t>, grid, dim3(256), 0, s, (const int32_t*)mask, seq_lens, B, Nt, base, bad);
    else hipLaunchKernelGGL(mask_to_seq_lens_kernel<int64_t>, grid, dim3(256), 0, s, (const int64_t*)mask, seq_lens, B, Nt, base, bad);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_attention_fwd_varlen(const void* q, const void* k, const void* v, void* o, int64_t ldq, int64_t ldk, int64_t ldv,
                                            int64_t ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, int B, int H, int S, int head_dim,
                                            float scale, const int32_t* seq_lens, float* lse, void* stream) {
    ADVGRPO_CHECK(head_dim == 128, "attention_fwd_varlen: head_dim %d not supported (128)", head_dim);
    ADVGRPO_CHECK(seq_lens, "attention_fwd_varlen: null seq_lens");
    ADVGRPO_CHECK(q && k && v && o, "attention_fwd_varlen: null pointer (q, k, v or o)");
    ADVGRPO_CHECK(B > 0 && H > 0 && S > 0, "attention_fwd_varlen: bad shape (B=%d H=%d S=%d)", B, H, S);
    ADVGRPO_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0, "attention_fwd_varlen: row pitches ldq, ldk, ldv must keep 16-byte alignment");
    ADVGRPO_CHECK(ldo % 8 == 0 && bso % 8 == 0 && (reinterpret_cast<uintptr_t>(o) & 15) == 0,
                  "attention_fwd_varlen: o, ldo and bso must keep 16-byte aligned output rows");
    AttnParams p{};
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (bf16_t*)o;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso;
    p.H = H; p.Sq = S; p.Skv = S;
    p.scale_log2e = scale * 1.4426950408889634f;
    p.lse = lse;
    p.xcd_local = 1;
    return attention_fwd_d128_varlen_launch(p, B, seq_lens, as_stream(stream));
}

extern "C" int advgrpo_attention_bwd_varlen(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                                            float* work, void* dq, void* dk, void* dv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                                            int64_t lddo, int64_t lddq, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso, int64_t bsdo,
                                            int64_t bsdq, int B, int H, int S, int head_dim, float scale, const int32_t* seq_lens, void* stream) {
    ADVGRPO_CHECK(head_dim == 128, "attention_bwd_varlen: head_dim %d not supported (128)", head_dim);
    ADVGRPO_CHECK(seq_lens, "attention_bwd_varlen: null seq_lens");
    ADVGRPO_CHECK(q && k && v && o && d_o && lse && work && dq && dk && dv, "attention_bwd_varlen: null pointer");
    ADVGRPO_CHECK(B > 0 && H > 0 && S > 0, "attention_bwd_varlen: bad shape (B=%d H=%d S=%d)", B, H, S);
    ADVGRPO_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && lddo % 8 == 0 && lddq % 8 == 0 &&
                      bsq % 8 == 0 && bsk % 8 == 0 && bsv % 8 == 0 && bso % 8 == 0 && bsdo % 8 == 0 && bsdq % 8 == 0,
                  "attention_bwd_varlen: row and batch pitches must keep 16-byte alignment");
    ADVGRPO_CHECK(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dq | (uintptr_t)dk |
                   (uintptr_t)dv) % 16 == 0, "attention_bwd_varlen: pointers must be 16-byte aligned");
    AttnBwdParams p{};
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v; p.o = (const bf16_t*)o;
    p.d_o = (const bf16_t*)d_o; p.lse = lse; p.vec = work;
    p.dq = (bf16_t*)dq; p.dk = (bf16_t*)dk; p.dv = (bf16_t*)dv;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.lddo = lddo; p.lddq = lddq;
    p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso; p.bsdo = bsdo; p.bsdq = bsdq;
    p.H = H; p.Sq = S; p.Skv = S; p.nb32 = (S + 31) / 32; p.scale = scale; p.scale_log2e = scale * 1.4426950408889634f;
    p.xcd_local = 1;
    return attention_bwd_d128_varlen_launch(p, B, seq_lens, as_stream(stream));
}
