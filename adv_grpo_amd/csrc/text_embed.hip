// text_embed.hip -- the index plumbing of prompt encoding as kernels (gfx950): what adv_grpo_amd/text_encoders.py did with torch indexing
// around the CLIP-L / CLIP-G text towers and the T5-XXL v1.1 encoder behind encode_prompt (adv_grpo/diffusers_patch/
// train_dreambooth_lora_sd3.py:98-144).  A caller that binds include/advgrpo.h directly gets prompt_embeds / pooled_prompt_embeds
// without torch:
//   advgrpo_token_embed             rows tok[id] (+ pos[s]) with a guard on the id (zero row + a counter, no assert, no trap)
//   advgrpo_t5_bucket               T5's bidirectional relative-position bucket, host function; the kernel below uses the same routine
//   advgrpo_t5_position_bias        bias[h, i, j] = rel_table[bucket(j - i), h]: the operand of advgrpo_attention_fwd_bias
//   advgrpo_clip_eos_pool           the pooled row of CLIPTextTransformer (first position of the maximum id / of the eos id)
//   advgrpo_prompt_embeds_assemble  [B, S + T, Dt]: CLIP-L | CLIP-G | zeros over the first S rows, the T5 states behind them
// All are bandwidth-bound row kernels: one 64-lane wave per row, four rows per workgroup, 16-byte accesses where the row pitch allows
// them (a scalar path otherwise), no LDS.
#include "common.hpp"

namespace advgrpo {

// ------------------------------------------------------------------------------------------------------------------ token embedding
__global__ __launch_bounds__(256) void token_embed_kernel(const int64_t* __restrict__ ids, const bf16_t* __restrict__ tok,
                                                          const bf16_t* __restrict__ pos, bf16_t* __restrict__ out, int rows, int S, int D,
                                                          int vocab, int* __restrict__ bad_ids, int vec) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t id = ids[r];
    const bool ok = id >= 0 && id < (int64_t)vocab;          // wave-uniform: an id outside the table reads nothing from it
    if (!ok && bad_ids && lane == 0) atomicAdd(bad_ids, 1);
    const bf16_t* t = tok + (ok ? id : 0) * (int64_t)D;
    const bf16_t* p = pos ? pos + (int64_t)(r % S) * D : nullptr;
    bf16_t* o = out + (int64_t)r * D;
    if (vec) {
        for (int c = lane * 8; c < D; c += 64 * 8) {
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) {
                v = *reinterpret_cast<const bf16x8*>(t + c);
                if (p) {
                    const bf16x8 q = *reinterpret_cast<const bf16x8*>(p + c);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = (short)f2bf(bf2f((uint16_t)v[k]) + bf2f((uint16_t)q[k]));
                }
            }
            *reinterpret_cast<bf16x8*>(o + c) = v;
        }
    } else {
        for (int c = lane; c < D; c += 64) o[c] = !ok ? (bf16_t)0 : (p ? f2bf(bf2f(t[c]) + bf2f(p[c])) : t[c]);
    }
}

// ------------------------------------------------------------------------------------------------- T5 relative-position bucket + bias
// transformers' T5Attention._relative_position_bucket(bidirectional=True) for (num_buckets, max_distance) = (32, 128), the parameters
// of every released T5 / T5 v1.1 encoder.  16 buckets per sign; distances below 8 have a bucket each; above, the reference takes
// 8 + int(log(n / 8) / log(128 / 8) * 8) = 8 + int(2 log2(n) - 6), capped at 15.  floor(2 log2 n) = floor(log2 n^2) for an integer n,
// so the boundary (n = 16, 32, 64: where a float log may land on either side) is decided in integer arithmetic.
__host__ __device__ inline int t5_bucket_32_128(int rel) {
    const int side = rel > 0 ? 16 : 0;
    const unsigned n = rel < 0 ? 0u - (unsigned)rel : (unsigned)rel;
    if (n < 8) return side + (int)n;
    if (n >= 128) return side + 15;
    const int large = 8 + (31 - __builtin_clz(n * n)) - 6;      // n * n < 2^14
    return side + (large < 15 ? large : 15);
}

__global__ __launch_bounds__(256) void t5_position_bias_kernel(const float* __restrict__ rel_table, float* __restrict__ bias, int H, int S,
                                                               int vec) {
    const int64_t total = (int64_t)H * S * S;
    if (vec) {      // S % 4 == 0: four consecutive keys of one (h, i) per lane, one 16-byte store
        const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
        if (e >= total) return;
        const int j = (int)(e % S), i = (int)((e / S) % S), h = (int)(e / ((int64_t)S * S));
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = rel_table[t5_bucket_32_128(j + k - i) * H + h];
        *reinterpret_cast<f32x4*>(bias + e) = v;
    } else {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= total) return;
        const int j = (int)(e % S), i = (int)((e / S) % S), h = (int)(e / ((int64_t)S * S));
        bias[e] = rel_table[t5_bucket_32_128(j - i) * H + h];
    }
}

// ---------------------------------------------------------------------------------------------------------------------- EOS pooling
// One wave per prompt: every lane scans the positions lane, lane + 64, .. and keeps its best (value, position); the butterfly keeps the
// larger value and, on a tie, the smaller position -- "first" as torch.argmax defines it.  argmax_mode: value = the id itself (the legacy
// eos_token_id == 2 configs); otherwise value = 1 at the eos id and 0 elsewhere, so a prompt without eos pools position 0.
__global__ __launch_bounds__(64) void clip_eos_pool_kernel(const int64_t* __restrict__ ids, const bf16_t* __restrict__ x,
                                                           bf16_t* __restrict__ pooled, int S, int D, int64_t eos, int argmax_mode, int vec) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int64_t* row = ids + (int64_t)b * S;
    long long best = 0;
    int at = S;                                  // S = "no candidate yet" (lanes past the end of a short row)
    for (int s = lane; s < S; s += 64) {
        const long long v = argmax_mode ? (long long)row[s] : (long long)(row[s] == eos);
        if (at == S || v > best) { best = v; at = s; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const long long ov = __shfl_xor(best, m, 64);
        const int oa = __shfl_xor(at, m, 64);
        if (oa < S && (at == S || ov > best || (ov == best && oa < at))) { best = ov; at = oa; }
    }
    const bf16_t* src = x + ((int64_t)b * S + at) * D;       // at < S: lane 0 always holds position 0 (S > 0)
    bf16_t* dst = pooled + (int64_t)b * D;
    if (vec) {
        for (int c = lane * 8; c < D; c += 64 * 8) *reinterpret_cast<bf16x8*>(dst + c) = *reinterpret_cast<const bf16x8*>(src + c);
    } else {
        for (int c = lane; c < D; c += 64) dst[c] = src[c];
    }
}

// ------------------------------------------------------------------------------------------------------------ prompt_embeds assembly
// Every element of out [B, S + T, Dt] is written exactly once by this one launch (no memset in front): rows p < S take
// pen_l[b, p] | pen_g[b, p] | zeros, rows p >= S take t5[b, p - S].
__global__ __launch_bounds__(256) void prompt_embeds_assemble_kernel(const bf16_t* __restrict__ pen_l, int Dl, const bf16_t* __restrict__ pen_g,
                                                                     int Dg, const bf16_t* __restrict__ t5, bf16_t* __restrict__ out, int rows,
                                                                     int S, int T, int Dt, int vec) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = r / (S + T), p = r % (S + T);
    bf16_t* o = out + (int64_t)r * Dt;
    if (p >= S) {
        const bf16_t* src = t5 + ((int64_t)b * T + (p - S)) * Dt;
        if (vec) {
            for (int c = lane * 8; c < Dt; c += 64 * 8) *reinterpret_cast<bf16x8*>(o + c) = *reinterpret_cast<const bf16x8*>(src + c);
        } else {
            for (int c = lane; c < Dt; c += 64) o[c] = src[c];
        }
        return;
    }
    const bf16_t* l = pen_l + ((int64_t)b * S + p) * Dl;
    const bf16_t* g = pen_g + ((int64_t)b * S + p) * Dg;
    if (vec) {      // Dl, Dg, Dt % 8 == 0: a chunk of 8 columns lies in one of the three regions
        for (int c = lane * 8; c < Dt; c += 64 * 8) {
            bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c < Dl) v = *reinterpret_cast<const bf16x8*>(l + c);
            else if (c < Dl + Dg) v = *reinterpret_cast<const bf16x8*>(g + (c - Dl));
            *reinterpret_cast<bf16x8*>(o + c) = v;
        }
    } else {
        for (int c = lane; c < Dt; c += 64) o[c] = c < Dl ? l[c] : (c < Dl + Dg ? g[c - Dl] : (bf16_t)0);
    }
}

static inline bool host_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_token_embed(const int64_t* ids, const void* tok, const void* pos, void* out, int B, int S, int D, int vocab, int* bad_ids,
                                   void* stream) {
    ADVGRPO_CHECK(ids && tok && out, "token_embed: null pointer");
    ADVGRPO_CHECK(B > 0 && S > 0 && D > 0 && vocab > 0 && (int64_t)B * S < (1ll << 31) - 4, "token_embed: bad shape (B=%d S=%d D=%d vocab=%d)", B, S, D,
                  vocab);
    const int rows = B * S;
    const int vec = D % 8 == 0 && host_aligned16(tok) && host_aligned16(out) && (!pos || host_aligned16(pos));
    hipLaunchKernelGGL(token_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), ids, (const bf16_t*)tok, (const bf16_t*)pos,
                       (bf16_t*)out, rows, S, D, vocab, bad_ids, vec);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_t5_bucket(int rel, int num_buckets, int max_distance) {
    ADVGRPO_CHECK(num_buckets == 32 && max_distance == 128,
                  "t5_bucket: only (num_buckets, max_distance) = (32, 128) is implemented, the T5 / T5 v1.1 encoders' (got %d, %d)", num_buckets,
                  max_distance);
    return t5_bucket_32_128(rel);
}

extern "C" int advgrpo_t5_position_bias(const float* rel_table, float* bias, int H, int S, int num_buckets, int max_distance, void* stream) {
    ADVGRPO_CHECK(rel_table && bias, "t5_position_bias: null pointer");
    ADVGRPO_CHECK(num_buckets == 32 && max_distance == 128,
                  "t5_position_bias: only (num_buckets, max_distance) = (32, 128) is implemented, the T5 / T5 v1.1 encoders' (got %d, %d)", num_buckets,
                  max_distance);
    ADVGRPO_CHECK(H > 0 && S > 0 && (int64_t)H * S * S < (1ll << 38), "t5_position_bias: bad shape (H=%d S=%d)", H, S);
    const int64_t total = (int64_t)H * S * S;
    const int vec = S % 4 == 0 && host_aligned16(bias);
    const int64_t threads = vec ? total / 4 : total;
    hipLaunchKernelGGL(t5_position_bias_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(stream), rel_table, bias, H, S, vec);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_clip_eos_pool(const int64_t* ids, const void* x, void* pooled, int B, int S, int D, int eos_token_id, void* stream) {
    ADVGRPO_CHECK(ids && x && pooled, "clip_eos_pool: null pointer");
    ADVGRPO_CHECK(B > 0 && S > 0 && D > 0, "clip_eos_pool: bad shape (B=%d S=%d D=%d)", B, S, D);
    const int vec = D % 8 == 0 && host_aligned16(x) && host_aligned16(pooled);
    hipLaunchKernelGGL(clip_eos_pool_kernel, dim3(B), dim3(64), 0, as_stream(stream), ids, (const bf16_t*)x, (bf16_t*)pooled, S, D,
                       (int64_t)eos_token_id, eos_token_id == 2, vec);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_prompt_embeds_assemble(const void* pen_l, int Dl, const void* pen_g, int Dg, const void* t5, void* out, int B, int S, int T,
                                              int Dt, void* stream) {
    ADVGRPO_CHECK(pen_l && pen_g && t5 && out, "prompt_embeds_assemble: null pointer");
    ADVGRPO_CHECK(B > 0 && S > 0 && T > 0 && Dl > 0 && Dg > 0 && Dt > 0 && (int64_t)B * (S + (int64_t)T) < (1ll << 31) - 4,
                  "prompt_embeds_assemble: bad shape (B=%d S=%d T=%d Dl=%d Dg=%d Dt=%d)", B, S, T, Dl, Dg, Dt);
    ADVGRPO_CHECK(Dl + Dg <= Dt, "prompt_embeds_assemble: the CLIP widths %d + %d exceed the T5 width %d", Dl, Dg, Dt);
    const int rows = B * (S + T);
    const int vec = Dl % 8 == 0 && Dg % 8 == 0 && Dt % 8 == 0 && host_aligned16(pen_l) && host_aligned16(pen_g) && host_aligned16(t5) &&
                    host_aligned16(out);
    hipLaunchKernelGGL(prompt_embeds_assemble_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), (const bf16_t*)pen_l, Dl,
                       (const bf16_t*)pen_g, Dg, (const bf16_t*)t5, (bf16_t*)out, rows, S, T, Dt, vec);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
