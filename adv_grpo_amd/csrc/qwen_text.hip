// qwen_text.hip -- the index plumbing of the Qwen2.5-VL prompt encoder as kernels (gfx950): what adv_grpo_amd/qwen_text_encoder.py did with
// torch indexing around its materialised attention and behind the tower (QwenImagePipeline._get_qwen_prompt_embeds; BASELINE config 5):
//   advgrpo_gqa_pack_heads       packed q | k | v rows [B T, (H + 2 KV) hd] -> q [B H, Tp, hd], k [B H, Tp, hd] (each key/value head written
//                                for its H / KV query heads), v^T [B H, hd, Tp]; Tp = ceil(T / 64) 64, the padding written as zeros
//   advgrpo_gqa_unpack_heads     o [B H, Tp, hd] -> [B T, H hd]
//   advgrpo_qwen_prompt_embeds   hidden [B, T, D] + per-sample lengths -> emb [B, L, D] (template prefix dropped, right-padded with
//                                zeros) and mask [B, L] int64
// Bandwidth-bound copies with 16-byte accesses; the transpose of V goes through a 64 x 64 LDS tile.
#include "common.hpp"

namespace advgrpo {

// One workgroup per (b, h, 64 positions, 64 head columns): q and k are row copies; v is read row-major (16 bytes along d), written to an
// LDS tile and read back column-wise so that v^T leaves in 16-byte pieces along the positions.
__global__ __launch_bounds__(256) void gqa_pack_heads_kernel(const bf16_t* __restrict__ qkv, int64_t ld, bf16_t* __restrict__ q,
                                                             bf16_t* __restrict__ k, bf16_t* __restrict__ vt, int T, int Tp, int H, int KV,
                                                             int hd, int ndt) {
    constexpr int TP = 64 + 2;                                   // tile pitch in elements
    __shared__ bf16_t tile[64 * TP];
    int idx = blockIdx.x;
    const int dt = idx % ndt; idx /= ndt;
    const int tt = idx % (Tp / 64); idx /= (Tp / 64);
    const int h = idx % H, b = idx / H;
    const int kvh = h / (H / KV);
    const int64_t bh = (int64_t)b * H + h;
    for (int c = threadIdx.x; c < 64 * 8; c += 256) {
        const int r = c >> 3, d = dt * 64 + (c & 7) * 8;         // position tt*64 + r, head columns d .. d + 7
        const int pos = tt * 64 + r;
        if (d >= hd) continue;
        uint4 vq = {0, 0, 0, 0}, vk = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
        if (pos < T) {
            const bf16_t* row = qkv + ((int64_t)b * T + pos) * ld;
            vq = *reinterpret_cast<const uint4*>(row + (int64_t)h * hd + d);
            vk = *reinterpret_cast<const uint4*>(row + (int64_t)(H + kvh) * hd + d);
            vv = *reinterpret_cast<const uint4*>(row + (int64_t)(H + KV + kvh) * hd + d);
        }
        *reinterpret_cast<uint4*>(q + (bh * Tp + pos) * hd + d) = vq;
        *reinterpret_cast<uint4*>(k + (bh * Tp + pos) * hd + d) = vk;
        const bf16_t* e = reinterpret_cast<const bf16_t*>(&vv);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[r * TP + (c & 7) * 8 + i] = e[i];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 64 * 8; c += 256) {
        const int dl = c >> 3, r0 = (c & 7) * 8;                 // head column dt*64 + dl, positions tt*64 + r0 .. + 7
        const int d = dt * 64 + dl;
        if (d >= hd) continue;
        uint4 out;
        bf16_t* e = reinterpret_cast<bf16_t*>(&out);
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = tile[(r0 + i) * TP + dl];
        *reinterpret_cast<uint4*>(vt + (bh * hd + d) * Tp + tt * 64 + r0) = out;
    }
}

__global__ __launch_bounds__(256) void gqa_unpack_heads_kernel(const bf16_t* __restrict__ o, bf16_t* __restrict__ out, int64_t total, int T, int Tp,
                                                               int H, int hd) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;   // 16-byte chunk of out [B T, H hd]
    if (c >= total) return;
    const int cpr = H * hd / 8;
    const int64_t row = c / cpr;
    const int col = (int)(c % cpr) * 8;
    const int h = col / hd, d = col % hd;
    const int64_t b = row / T;
    const int t = (int)(row % T);
    *reinterpret_cast<uint4*>(out + row * ((int64_t)H * hd) + col) = *reinterpret_cast<const uint4*>(o + ((b * H + h) * Tp + t) * hd + d);
}

// One wave per output row (b, l), four rows per workgroup.  Every element of emb and mask is written by this one launch.
__global__ __launch_bounds__(256) void qwen_prompt_embeds_kernel(const bf16_t* __restrict__ hidden, const int* __restrict__ lens,
                                                                 bf16_t* __restrict__ emb, int64_t* __restrict__ mask, int rows, int T, int D,
                                                                 int L, int drop, int* __restrict__ bad, int vec) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = r / L, l = r % L;
    const int n = lens[b];
    const int len = n < drop ? drop : (n > T ? T : n);            // a length outside [drop, T] is clamped ...
    if (n != len && bad && l == 0 && lane == 0) atomicAdd(bad, 1);  // ... and counted, once per sample
    const bool live = l < len - drop;                            // wave-uniform; then drop + l < len <= T
    const bf16_t* src = hidden + ((int64_t)b * T + drop + (live ? l : 0)) * D;
    bf16_t* dst = emb + (int64_t)r * D;
    if (lane == 0) mask[r] = live ? 1 : 0;
    if (vec) {
        for (int c = lane * 8; c < D; c += 64 * 8)
            *reinterpret_cast<uint4*>(dst + c) = live ? *reinterpret_cast<const uint4*>(src + c) : uint4{0, 0, 0, 0};
    } else {
        for (int c = lane; c < D; c += 64) dst[c] = live ? src[c] : (bf16_t)0;
    }
}

static inline bool host_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace advgrpo

using namespace advgrpo;

extern "C" int advgrpo_gqa_pack_heads(const void* qkv, int64_t ld, void* q, void* k, void* vt, int B, int T, int H, int KV, int head_dim,
                                      void* stream) {
    ADVGRPO_CHECK(qkv && q && k && vt, "gqa_pack_heads: null pointer");
    ADVGRPO_CHECK(B > 0 && T > 0 && H > 0 && KV > 0 && head_dim > 0 && head_dim % 8 == 0, "gqa_pack_heads: bad shape (B=%d T=%d H=%d KV=%d head_dim=%d)",
                  B, T, H, KV, head_dim);
    ADVGRPO_CHECK(H % KV == 0, "gqa_pack_heads: %d query heads are not a multiple of %d key/value heads", H, KV);
    ADVGRPO_CHECK(ld % 8 == 0 && ld >= (int64_t)(H + 2 * KV) * head_dim && host_aligned16(qkv) && host_aligned16(q) && host_aligned16(k) &&
                      host_aligned16(vt),
                  "gqa_pack_heads: 16-byte aligned pointers and a row pitch that is a multiple of 8 and holds the heads");
    const int Tp = (T + 63) / 64 * 64, ndt = (head_dim + 63) / 64;
    const int64_t nwg = (int64_t)B * H * (Tp / 64) * ndt;
    ADVGRPO_CHECK(nwg < (1ll << 31), "gqa_pack_heads: grid too large");
    hipLaunchKernelGGL(gqa_pack_heads_kernel, dim3((unsigned)nwg), dim3(256), 0, as_stream(stream), (const bf16_t*)qkv, ld, (bf16_t*)q, (bf16_t*)k,
                       (bf16_t*)vt, T, Tp, H, KV, head_dim, ndt);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_gqa_unpack_heads(const void* o, void* out, int B, int T, int H, int head_dim, void* stream) {
    ADVGRPO_CHECK(o && out, "gqa_unpack_heads: null pointer");
    ADVGRPO_CHECK(B > 0 && T > 0 && H > 0 && head_dim > 0 && head_dim % 8 == 0, "gqa_unpack_heads: bad shape (B=%d T=%d H=%d head_dim=%d)", B, T, H,
                  head_dim);
    ADVGRPO_CHECK(host_aligned16(o) && host_aligned16(out), "gqa_unpack_heads: pointers must be 16-byte aligned");
    const int Tp = (T + 63) / 64 * 64;
    const int64_t total = (int64_t)B * T * H * head_dim / 8;
    ADVGRPO_CHECK((total + 255) / 256 < (1ll << 31), "gqa_unpack_heads: grid too large");
    hipLaunchKernelGGL(gqa_unpack_heads_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), (const bf16_t*)o, (bf16_t*)out,
                       total, T, Tp, H, head_dim);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

extern "C" int advgrpo_qwen_prompt_embeds(const void* hidden, const int* lens, void* emb, int64_t* mask, int B, int T, int D, int L, int drop_idx,
                                          int* bad, void* stream) {
    ADVGRPO_CHECK(hidden && lens && emb && mask, "qwen_prompt_embeds: null pointer");
    ADVGRPO_CHECK(B > 0 && T > 0 && D > 0 && L > 0 && drop_idx >= 0 && drop_idx <= T && (int64_t)B * L < (1ll << 31) - 4,
                  "qwen_prompt_embeds: bad shape (B=%d T=%d D=%d L=%d drop_idx=%d)", B, T, D, L, drop_idx);
    const int rows = B * L;
    const int vec = D % 8 == 0 && host_aligned16(hidden) && host_aligned16(emb);
    hipLaunchKernelGGL(qwen_prompt_embeds_kernel, dim3((rows + 3) / 4), dim3(256), 0, as_stream(stream), (const bf16_t*)hidden, lens, (bf16_t*)emb, mask,
                       rows, T, D, L, drop_idx, bad, vec);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}
