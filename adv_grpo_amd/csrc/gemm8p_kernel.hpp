// gemm8p_kernel.hpp -- device code of the 256 x 256 eight-phase persistent GEMM (see gemm8p.hip for the description) and the
// launch helper shared by the translation units that instantiate its epilogue classes (gemm8p.hip: rollout classes,
// gemm8p_train.hip: G-step classes -- two files so that the instantiations compile in parallel).
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "gemm_device.hpp"

namespace advgrpo {

namespace {

constexpr int P8_BM = 256, P8_BN = 256, P8_BK = 64;
constexpr int P8_HALF = 128 * P8_BK * 2;          // one ring item: 128 rows x 128 B
constexpr int P8_BUF = 4 * P8_HALF;               // one k-tile buffer: A sub 0, A sub 1, W sub 0, W sub 1
constexpr int P8_LDS = 2 * P8_BUF;                // 128 KiB
constexpr int P8_SCRATCH = 2 * 16 * 64 * 4;       // per-wave epilogue scratch: 2 slabs of 16 rows x 64 f32, inside buffer 1

// The lane id, re-derived where it is needed (two VALU instructions) instead of kept live: held across the k loop it was
// spilled, and each reload at the tile boundary was a scratch-memory load followed by s_waitcnt vmcnt(0) -- 18 serialised
// memory round trips made up most of the ~2.5-3.5k cycles a wave spent between two tiles.
__device__ __forceinline__ int p8_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// wait until at most `allowed` ring items (2 DMA instructions each) of this wave are still in flight
__device__ __forceinline__ void p8_wait_inflight(int allowed) {
    if (allowed >= 5) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (allowed == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (allowed == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (allowed == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (allowed == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// What a workgroup needs to stream one output tile: the problem, the tile origin and the per-lane DMA sources.  A ring
// item is what every wave reads in ONE phase: item "A sub s" = rows {s*64 .. s*64+63} of both 128-row wave-row halves,
// item "W sub s" = columns {s*32 .. s*32+31} of the four 64-wide wave columns; slot row r of the 128-row item image belongs
// to wave row r >> 6 (A) / wave column r >> 5 (W).  Sources are 32-bit byte offsets from the uniform operand bases (the
// DMA takes "SGPR base + VGPR offset").
struct P8Tile {
    bool second;                     // problem b of a paired launch
    int m0, n0, nk;
    const char* a_bytes;             // operand bases (uniform)
    const char* w_bytes;
    uint32_t a_off[2][2], b_off[2][2];
};

__device__ __forceinline__ void p8_setup(P8Tile& t, const GemmParams& pr, int id, int wave) {
    const GemmParams* p = &pr;
    const int lane = p8_lane();
    const int tiles_n = (p->N + P8_BN - 1) / P8_BN, tiles_m = (p->M + P8_BM - 1) / P8_BM;
    int tile_m, tile_n;
    tile_coords(id, tiles_m, tiles_n, 4, tile_m, tile_n);
    t.a_bytes = reinterpret_cast<const char*>(p->A);
    t.w_bytes = reinterpret_cast<const char*>(p->W);
    t.m0 = tile_m * P8_BM;
    t.n0 = tile_n * P8_BN;
    const int es = p->fp8 ? 1 : 2;                 // operand element size: a k-tile is 128 BYTES per row either way (64 bf16 / 128 fp8)
    t.nk = p->K * es / (P8_BK * 2);
    const int lrow = lane >> 3;                   // row inside an 8-row DMA instruction
    const int schunk = (lane & 7) ^ lrow;         // pre-swizzled source chunk of this lane's LDS slot
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int sr = (wave + it * 8) * 8 + lrow;                    // slot row of this lane's 16 bytes
            int r = t.m0 + (sr >> 6) * 128 + sub * 64 + (sr & 63);
            r = r < p->M ? r : p->M - 1;
            const int64_t ar = seg_row(r, p->a_seg_rows, p->a_seg_stride, p->a_seg_off);
            t.a_off[sub][it] = (uint32_t)(ar * p->lda * es + schunk * 16);
            int n = t.n0 + (sr >> 5) * 64 + sub * 32 + (sr & 31);
            n = n < p->N ? n : p->N - 1;
            t.b_off[sub][it] = (uint32_t)((int64_t)n * p->ldw * es + schunk * 16);
        }
}

// which = 0,1: A sub 0 / 1; 2,3: W sub 0 / 1
__device__ __forceinline__ void p8_stage(const P8Tile& t, char* smem, int wave, int buf, int which, int kt) {
    if (kt >= t.nk) return;
    char* base = smem + buf * P8_BUF + which * P8_HALF;
    const char* src = (which < 2 ? t.a_bytes : t.w_bytes) + kt * (P8_BK * 2);   // uniform
    const uint32_t* off = which < 2 ? t.a_off[which] : t.b_off[which - 2];
#pragma unroll
    for (int it = 0; it < 2; ++it) lds_dma16(src, off[it], lds_addr(base + (wave + it * 8) * 1024));
}

// Fused epilogue.  Same arithmetic, in the same order, as gemm_epilogue_rows (gemm_device.hpp) -- results are bit-identical to
// the other tile variants.  With one workgroup per CU nothing overlaps the epilogue, so every cycle in it is exposed (the
// first version spent 16 us per tile here, 30 us being the whole k loop).  What it is built from, and why:
//   * eight 16-row slabs in four STATIC rounds of two: accumulators may only be indexed statically (a runtime-indexed
//     accumulator array goes to scratch memory); a round writes two slabs to the wave's private 8 KiB of LDS, then a
//     static loop over the two slabs reads them back row-wise.  (A runtime round loop with the accumulators rotated down
//     by `v_mov` cost ~190 v_mov_b64 per tile; fully unrolling every OPTION as well gave 100k instructions and 29 us of
//     instruction fetch per tile -- the options are compile-time classes instead, below.)
//   * LDS bounce: f32 rows of 256 B, 16-byte chunk c of row r at slot c ^ (r & 7) -- conflict-free for the ds_write_b128
//     of the accumulator layout (8 lanes = 8 rows, one chunk) and for the ds_read_b128 of the row layout (a lane ends
//     with 8 consecutive columns of one row: 16-byte loads of bias / gate / residual / aux, 16-byte stores);
//   * no integer division per row and no branches: the output-row map (row-segment scatter) and the gate index advance as
//     wave-uniform (segment, remainder) pairs from slab to slab with scalar selects; a lane adds the segment jump / next
//     gate vector by comparison masks (segments and gate groups are at least a slab long: gemm8p_ok);
//   * 32-bit element offsets from the uniform operand bases (host-checked), 24-bit multiplies;
//   * residual rows and gate vectors are requested P8_EPI_AHEAD slabs ahead with UNCONDITIONAL loads (edge rows read
//     element 0): a load inside a branch makes the compiler wait with vmcnt(0), which also waits for the prefetch just issued;
//   * the problem description is selected once per tile into pinned scalar registers (P8EpiArgs), the lane id is
//     re-derived (p8_lane): anything kept live across the k loop is spilled, and a spill reload is a memory operation
//     whose vmcnt(0) drains the prefetches (VGPR) or hundreds of v_readlane (SGPR);
//   * arithmetic on explicit column pairs (v_pk_mul / v_pk_add / v_pk_fma_f32, one v_cvt_pk_bf16_f32 per output dword);
//   * streaming (nt) stores of the output tile;
//   * specialised at compile time for the epilogues of the rollout and the G-step (EPI_*): skipping the unused options with
//     wave-uniform branches cost more than the arithmetic (a taken branch is an instruction-fetch bubble; the generic
//     code took 22-28k cycles per tile, 55k being the k loop).
// A class is a set of features fixed at compile time (EPI_GENERIC: everything decided at run time).
enum { EPI_GENERIC = -1, F_BIAS = 1, F_RMS = 2 /* per-head QK RMSNorm */, F_GELU = 4 /* gelu_tanh */, F_GATE_RES = 8 /* * gate + residual */,
       F_AUX_OUT = 16 /* keep the pre-activation (training forward) */, F_DGELU = 32 /* y *= gelu_tanh'(aux_in) (training backward) */,
       F_SCALE = 64 /* acc *= a_scale[m] * w_scale[n]: the per-token / per-channel scales of fp8 operands */ };
enum { EPI_PLAIN = 0, EPI_BIAS = F_BIAS, EPI_BIAS_RMS = F_BIAS | F_RMS, EPI_BIAS_GELU = F_BIAS | F_GELU, EPI_BIAS_GATE_RES = F_BIAS | F_GATE_RES,
       EPI_BIAS_GELU_AUX = F_BIAS | F_GELU | F_AUX_OUT, EPI_DGELU = F_DGELU };

// which classes write their output tile with streaming (nt) stores: 0 all (product), 1 all but gate + residual (its output is the next
// LayerNorm's input), 2 none  -- A/B knob of scripts/probes/rollout_ab_inprocess.py builds
#ifndef P8_NT_MODE
#define P8_NT_MODE 0
#endif
#ifndef P8_EPI_AHEAD
#define P8_EPI_AHEAD 3
#endif

typedef const __attribute__((address_space(1))) char* p8_gcptr;
typedef __attribute__((address_space(1))) char* p8_gptr;
__device__ __forceinline__ uint4 p8_gld16(p8_gcptr base, uint32_t byte_off) {
    const u32x4 v = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(base + byte_off);
    return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void p8_gst16(p8_gptr base, size_t byte_off, const uint4& v) {
    *reinterpret_cast<__attribute__((address_space(1))) u32x4*>(base + byte_off) = u32x4{v.x, v.y, v.z, v.w};
}
// streaming (non-temporal) store: the output tile is not read again by this kernel
__device__ __forceinline__ void p8_gst16_nt(p8_gptr base, size_t byte_off, const uint4& v) {
    __builtin_nontemporal_store(u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<__attribute__((address_space(1))) u32x4*>(base + byte_off));
}
// a value pinned into scalar registers (opaque to the optimiser from here on)
template <class T>
__device__ __forceinline__ T p8_sgpr(T v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ float p8_sgpr(float v) { return __builtin_bit_cast(float, p8_sgpr(__builtin_bit_cast(int, v))); }

// The epilogue's own copy of the problem description, chosen ONCE per tile.  Reading the fields through
// "second ? pp.b : pp.a" the compiler kept BOTH problems of a paired launch in scalar registers and selected at every use:
// the ~120 SGPRs that needs were spilled to VGPR lanes, and the gate + residual / QK-norm epilogues executed 400-500
// v_readlane (plus their hazard wait states) per tile.  32-bit copies of what is 64-bit on the host side (pitches, segment
// strides: all host-checked to fit) halve the register count again.
struct P8EpiArgs {
    int M, N, act, out_dtype;
    float alpha, rms_eps;
    // (explicitly GLOBAL pointers: a pointer that went through the register pin has lost the address space the compiler
    // infers for kernel arguments and would be accessed with flat_load / flat_store)
    p8_gcptr bias, gate, residual, rms_w, aux_in, a_scale, w_scale;
    p8_gptr aux_out, C, rms_rs_out;
    int rms_nheads, rms_hpw, gate_rows, seg_rows, seg_stride, seg_off;
    uint32_t gate_stride, ldc, ldr, ld_aux;
};
template <int EPI>
__device__ __forceinline__ P8EpiArgs p8_epi_args(const GemmParams& g) {
    constexpr bool G = EPI == EPI_GENERIC;
    constexpr bool BIAS = G || (EPI & F_BIAS), RMS = G || (EPI & F_RMS), GR = G || (EPI & F_GATE_RES), AUXO = G || (EPI & F_AUX_OUT),
                   AUXI = G || (EPI & F_DGELU);
    P8EpiArgs e{};
    e.M = p8_sgpr(g.M); e.N = p8_sgpr(g.N);
    e.alpha = p8_sgpr(g.alpha);
    e.C = (p8_gptr)p8_sgpr((uintptr_t)g.C); e.ldc = p8_sgpr((uint32_t)g.ldc);
    e.seg_rows = p8_sgpr(g.seg_rows); e.seg_stride = p8_sgpr((int)g.seg_stride); e.seg_off = p8_sgpr((int)g.seg_off);
    if constexpr (G) { e.act = p8_sgpr(g.act); e.out_dtype = p8_sgpr(g.out_dtype); }
    if constexpr (BIAS) e.bias = (p8_gcptr)p8_sgpr((uintptr_t)g.bias);
    if constexpr (RMS) {
        e.rms_w = (p8_gcptr)p8_sgpr((uintptr_t)g.rms_w); e.rms_rs_out = (p8_gptr)p8_sgpr((uintptr_t)g.rms_rs_out); e.rms_nheads = p8_sgpr(g.rms_nheads);
        e.rms_hpw = p8_sgpr(g.rms_hpw); e.rms_eps = p8_sgpr(g.rms_eps);
    }
    if constexpr (GR) {
        e.gate = (p8_gcptr)p8_sgpr((uintptr_t)g.gate); e.gate_stride = p8_sgpr((uint32_t)g.gate_stride); e.gate_rows = p8_sgpr(g.gate_rows);
        e.residual = (p8_gcptr)p8_sgpr((uintptr_t)g.residual); e.ldr = p8_sgpr((uint32_t)g.ldr);
    }
    if constexpr (AUXO) e.aux_out = (p8_gptr)p8_sgpr((uintptr_t)g.aux_out);
    if constexpr (AUXI) e.aux_in = (p8_gcptr)p8_sgpr((uintptr_t)g.aux_in);
    if constexpr (AUXO || AUXI) e.ld_aux = p8_sgpr((uint32_t)g.ld_aux);
    if constexpr (!G && (EPI & F_SCALE)) { e.a_scale = (p8_gcptr)p8_sgpr((uintptr_t)g.a_scale); e.w_scale = (p8_gcptr)p8_sgpr((uintptr_t)g.w_scale); }
    return e;
}

template <int EPI>
__device__ __forceinline__ void p8_epilogue(const GemmParams& p_in, f32x4 (&acc)[8][4], int mw0, int nw0, char* scratch) {
    const int lane = p8_lane();
    constexpr bool G = EPI == EPI_GENERIC;
    const P8EpiArgs p = p8_epi_args<EPI>(p_in);
    // features: compile-time constants in the specialised classes (bf16 output, alpha = 1 is NOT assumed)
    const bool has_bias = G ? p.bias != nullptr : (EPI & F_BIAS) != 0;
    const bool has_rms = G ? p.rms_w != nullptr : (EPI & F_RMS) != 0;
    const bool has_gate = G ? p.gate != nullptr : (EPI & F_GATE_RES) != 0;
    const bool has_res = G ? p.residual != nullptr : (EPI & F_GATE_RES) != 0;
    const bool has_aux_out = G ? p.aux_out != nullptr : (EPI & F_AUX_OUT) != 0;
    const bool has_scale = G ? false : (EPI & F_SCALE) != 0;   // (fp8 operands run on specialised classes only)
    const bool out_bf16 = G ? p.out_dtype == ADVGRPO_BF16 : true;
    const int mrow = lane & 15, q = lane >> 4;
    const int orow_l = lane >> 3, c8 = (lane & 7) * 8;
    const int n = nw0 + c8;
    const bool n_ok = n < p.N;
    // bf16 pair in a dword -> two f32 (shift / mask), and back with the hardware conversion (round-to-nearest-even)
    auto up2 = [](uint32_t w) __attribute__((always_inline)) {
        return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
    };
    auto unpack4 = [&](const uint4& q4, f32x2 (&f)[4]) __attribute__((always_inline)) {
        f[0] = up2(q4.x); f[1] = up2(q4.y); f[2] = up2(q4.z); f[3] = up2(q4.w);
    };
    auto pack4 = [&](const f32x2 (&x)[4]) __attribute__((always_inline)) {
        return uint4{cvt_pk_bf16(x[0]), cvt_pk_bf16(x[1]), cvt_pk_bf16(x[2]), cvt_pk_bf16(x[3])};
    };
    auto ld16 = [](p8_gcptr base, uint32_t elem) __attribute__((always_inline)) { return p8_gld16(base, elem * 2u); };
    // alpha as ONE scalar register for the whole epilogue: left to the compiler the two problems' alphas of a paired launch
    // sat in VGPRs, were spilled, and every pass reloaded both from scratch memory -- a memory operation whose
    // s_waitcnt vmcnt(0) also drained the residual prefetch
    const float alpha = p.alpha;
    // QK-norm: the wave tile's 64 columns are ONE head -- its weight vector and whether it is normalised at all (q / k heads
    // yes, v heads no) are fixed for the tile: loaded once here, not once per pass (a load + full wait 16 times per tile)
    f32x2 rms_w2[4];
    bool rms_on = false;
    if (has_rms) {
        const int hh = n >> 6;
        rms_on = hh < p.rms_nheads && n_ok;
        if (rms_on) unpack4(ld16(p.rms_w, (uint32_t)((hh / p.rms_hpw) * 64 + c8)), rms_w2);
    }
    f32x2 bias2[4];
    if (has_bias && n_ok) unpack4(ld16(p.bias, (uint32_t)n), bias2);
    f32x2 wsc2[4];                               // fp8 operands: the eight per-output-channel scales of this lane's columns (f32)
    if (has_scale && n_ok) {
        const uint4 s0 = p8_gld16(p.w_scale, (uint32_t)n * 4u), s1 = p8_gld16(p.w_scale, (uint32_t)n * 4u + 16u);
        wsc2[0] = f32x2{__builtin_bit_cast(float, s0.x), __builtin_bit_cast(float, s0.y)};
        wsc2[1] = f32x2{__builtin_bit_cast(float, s0.z), __builtin_bit_cast(float, s0.w)};
        wsc2[2] = f32x2{__builtin_bit_cast(float, s1.x), __builtin_bit_cast(float, s1.y)};
        wsc2[3] = f32x2{__builtin_bit_cast(float, s1.z), __builtin_bit_cast(float, s1.w)};
    }
    // wave-uniform bookkeeping of the slab's first row m_s: output row = seg_b * seg_stride + seg_off + seg_r (identity map:
    // seg_rows = 0 -> one segment as long as M), gate vector = gate_b
    const int seg_rows = p.seg_rows > 0 ? p.seg_rows : 0x7fffffff;
    const int gate_rows = p.gate_rows > 0 ? p.gate_rows : 0x7fffffff;
    const int seg_jump = p.seg_rows > 0 ? (int)p.seg_stride - p.seg_rows : 0;   // added to the row when it wraps
    struct Cur { int seg_b, seg_r, gate_b, gate_r; };
    auto start = [&](int m) __attribute__((always_inline)) {
        Cur c;
        c.seg_b = m / seg_rows; c.seg_r = m - c.seg_b * seg_rows;
        c.gate_b = m / gate_rows; c.gate_r = m - c.gate_b * gate_rows;
        return c;
    };
    // 16 rows further; segments / gate groups are at least 16 rows (gemm8p_ok): at most one wrap, done with scalar selects
    // (as loops these were four real branches per slab, and a taken branch is an instruction-fetch bubble)
    auto advance = [&](Cur& c) __attribute__((always_inline)) {
        c.seg_r += 16;
        const int ws = c.seg_r >= seg_rows ? 1 : 0;
        c.seg_r -= ws ? seg_rows : 0;
        c.seg_b += ws;
        c.gate_r += 16;
        const int wg = c.gate_r >= gate_rows ? 1 : 0;
        c.gate_r -= wg ? gate_rows : 0;
        c.gate_b += wg;
    };
    // output row of (slab cursor, row inside the slab)
    // (segments and gate groups are at least a slab long, gemm8p_ok: a slab crosses at most one boundary)
    auto out_row = [&](const Cur& c, int row) __attribute__((always_inline)) -> uint32_t {
        const int base = p.seg_rows > 0 ? c.seg_b * (int)p.seg_stride + (int)p.seg_off + c.seg_r : c.seg_r;
        return (uint32_t)(base + row + (seg_jump & -(int)(c.seg_r + row >= seg_rows)));
    };
    // what a slab needs from memory: its residual rows (two passes of 8 rows) and the gate vector of its first row.
    // The loads are UNCONDITIONAL (rows / columns past the edge read element 0 instead): with a load inside a branch the
    // compiler can no longer count the younger memory operations and waits with vmcnt(0) -- which also waits for the
    // prefetch it has just issued for the slab after next, so every slab paid a full memory latency (measured: 32 k
    // cycles for the gate + residual epilogue against 15 k for bias + GELU).
    struct Pre { uint4 r[2]; uint4 g[2]; float sa[2]; };     // (g[ps]: the gate vector of THIS lane's row in pass ps -- no reload branch; sa: its fp8 row scale)
    auto prefetch = [&](const Cur& c, int i, Pre& f) __attribute__((always_inline)) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int row = ps * 8 + orow_l;
            f.r[ps] = uint4{0u, 0u, 0u, 0u};
            if (has_res) {
                const bool ok = mw0 + i * 16 + row < p.M && n_ok;
                f.r[ps] = ld16(p.residual, (__umul24(out_row(c, row), (uint32_t)p.ldr) + n) & (0u - (uint32_t)ok));
            }
        }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {         // per-token scale of the INPUT row (unconditional: rows past the end read row M - 1)
            f.sa[ps] = 1.0f;
            if (has_scale) {
                const int m_in = min(mw0 + i * 16 + ps * 8 + orow_l, p.M - 1);
                f.sa[ps] = *reinterpret_cast<const __attribute__((address_space(1))) float*>(p.a_scale + (uint32_t)m_in * 4u);
            }
        }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int row = ps * 8 + orow_l;
            f.g[ps] = uint4{0u, 0u, 0u, 0u};
            if (has_gate) {     // (a row past the last one has no gate vector)
                const bool ok = mw0 + i * 16 + row < p.M && n_ok;
                const uint32_t gb = (uint32_t)(c.gate_b + (int)(c.gate_r + row >= gate_rows));
                f.g[ps] = ld16(p.gate, (__umul24(gb, (uint32_t)p.gate_stride) + n) & (0u - (uint32_t)ok));
            }
        }
    };
    Cur cur = start(__builtin_amdgcn_readfirstlane(mw0)), cpre = cur;
    constexpr int AHEAD = P8_EPI_AHEAD;       // slabs requested ahead of the one being written out
    Pre f[AHEAD + 1];
    prefetch(cpre, 0, f[0]);
#pragma unroll
    for (int a = 1; a < AHEAD; ++a) {
        advance(cpre);
        prefetch(cpre, a, f[a]);
    }
    const int w_off = mrow * 256, w_sw = mrow & 7;
    const int act = G ? p.act : ((EPI & F_GELU) ? (int)ACT_GELU_TANH : ((EPI & F_DGELU) ? (int)ACT_DGELU_TANH : (int)ACT_NONE));
    static_for<4>([&](auto rdc) {
        constexpr int rd = decltype(rdc)::value;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<f32x4*>(scratch + sl * 4096 + w_off + (((j * 4 + q) ^ w_sw) << 4)) = acc[rd * 2 + sl][j];
        static_for<2>([&](auto slc) {
            constexpr int sl = decltype(slc)::value;
            constexpr int i = rd * 2 + sl;
            const char* slab = scratch + sl * 4096;
            const Pre& f0 = f[i % (AHEAD + 1)];
            const Cur c0 = cur;
            if constexpr (i + AHEAD < 8) {
                advance(cpre);
                prefetch(cpre, i + AHEAD, f[(i + AHEAD) % (AHEAD + 1)]);
            }
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int row = ps * 8 + orow_l;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(slab + row * 256 + ((((lane & 7) * 2) ^ (row & 7)) << 4));
                const f32x4 hi = *reinterpret_cast<const f32x4*>(slab + row * 256 + ((((lane & 7) * 2 + 1) ^ (row & 7)) << 4));
                if (mw0 + i * 16 + row >= p.M || !n_ok) continue;   // (unrolled: skips to the next pass)
                const uint32_t orow = out_row(c0, row);
                // (contraction off for the scale / bias / gate / residual steps: where a specialised class makes two of them
                // unconditional the compiler would fuse them into an fma and the classes would stop agreeing bit for bit)
                // The arithmetic is written on explicit PAIRS (columns 2k, 2k+1 of the lane's eight): v_pk_mul / v_pk_add_f32
                // on the register pairs the LDS read delivers and one v_cvt_pk_bf16_f32 per output dword.  Left to the
                // auto-vectoriser the same code paired columns (0,2), (1,3) and re-interleaved them with 14 moves / and / or
                // per pass (a third of the bias-only epilogue).
                f32x2 v[4] = {f32x2{lo[0], lo[1]}, f32x2{lo[2], lo[3]}, f32x2{hi[0], hi[1]}, f32x2{hi[2], hi[3]}};
                {
#pragma clang fp contract(off)
                    if (has_scale) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = (v[k] * f0.sa[ps]) * wsc2[k];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = v[k] * alpha;
                    if (has_bias) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = v[k] + bias2[k];
                    }
                }
                if (has_rms) {   // QK-norm: the wave tile's 64 columns are one head, its row sits in 8 adjacent lanes
                    const int hh = n >> 6;
                    float sq = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = up2(cvt_pk_bf16(v[k]));             // the Linear's bf16 output is what gets normalised
                        sq += v[k].x * v[k].x;
                        sq += v[k].y * v[k].y;
                    }
                    sq = group8_sum(sq);
                    if (rms_on) {
                        const float rs = rsqrtf(sq * (1.0f / 64.0f) + p.rms_eps);
                        if (p.rms_rs_out && (lane & 7) == 0)
                            *reinterpret_cast<__attribute__((address_space(1))) float*>(p.rms_rs_out + ((size_t)orow * p.rms_nheads + hh) * 4) = rs;
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = up2(cvt_pk_bf16(v[k] * rs)) * rms_w2[k];
                    }
                }
                const uint32_t o_aux = __umul24(orow, (uint32_t)p.ld_aux) + n;
                if (has_aux_out) p8_gst16(p.aux_out, (size_t)(o_aux * 2u), pack4(v));
                if ((G || (EPI & F_DGELU)) && act >= ACT_DGELU_TANH) {
                    f32x2 z[4];
                    unpack4(ld16(p.aux_in, o_aux), z);
                    if (act == ACT_DGELU_TANH) {
                        dgelu_tanh_mul_pk4(v, z);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = f32x2{v[k].x * dact_fn(z[k].x, act), v[k].y * dact_fn(z[k].y, act)};
                    }
                } else if (act == ACT_GELU_TANH) {
                    gelu_tanh_pk4(v);
                } else if (act != ACT_NONE) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = f32x2{act_fn(v[k].x, act), act_fn(v[k].y, act)};
                }
                if (has_gate) {
                    f32x2 g[4];
                    unpack4(f0.g[ps], g);
                    {
#pragma clang fp contract(off)
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = v[k] * g[k];
                    }
                }
                if (has_res) {
                    f32x2 r[4];
                    unpack4(f0.r[ps], r);
                    {
#pragma clang fp contract(off)
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = v[k] + r[k];
                    }
                }
                const uint32_t o = __umul24(orow, (uint32_t)p.ldc) + n;
                if (out_bf16) {
                    if constexpr (P8_NT_MODE == 0 || (P8_NT_MODE == 1 && !G && !(EPI & F_GATE_RES))) p8_gst16_nt(p.C, (size_t)(o * 2u), pack4(v));
                    else p8_gst16(p.C, (size_t)(o * 2u), pack4(v));
                } else {
                    p8_gst16(p.C, (size_t)o * 4u, __builtin_bit_cast(uint4, make_float4(v[0].x, v[0].y, v[1].x, v[1].y)));
                    p8_gst16(p.C, (size_t)o * 4u + 16, __builtin_bit_cast(uint4, make_float4(v[2].x, v[2].y, v[3].x, v[3].y)));
                }
            }
            advance(cur);
        });
    });
}

}  // namespace

struct P8Sched { int tiles_a, tiles_total; unsigned long long* stamps; };   // stamps: experiment (ADVGRPO_P8_STAMPS)

typedef int p8_v4i __attribute__((ext_vector_type(4)));
typedef int p8_v8i __attribute__((ext_vector_type(8)));
// fp8 operands: the two 16-byte fragments a lane reads per row and k-tile (chunks kgrp and 4 + kgrp of the 128-byte row) are
// the 32 fp8 of ONE v_mfma_f32_16x16x128_f8f6f4 operand.  Which 32 of the row's 128 k positions a lane holds does not matter
// for a dot product as long as both operands agree, and they do (same fragment reads for A and W), so the LDS image, the DMA
// and the reads are the bf16 kernel's, byte for byte.  The UNSCALED form of the instruction (both scale operands the
// constant 0: no v_mfma_ld_scale prefix, block scales 2^0; measured identical to unit scales in a register and at the same
// rate, scripts/probes/mfma_fp8_probe.hip -- and with scale VGPRs this kernel spilled inside the k loop): the per-token /
// per-channel scales are applied in the epilogue (F_SCALE), the instruction is used for its K = 128 rate (2x bf16).
__device__ __forceinline__ p8_v8i p8_cat(const bf16x8_t& lo, const bf16x8_t& hi) {
    return __builtin_shufflevector(__builtin_bit_cast(p8_v4i, lo), __builtin_bit_cast(p8_v4i, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}

template <bool PAIR, int EPI, bool FP8 = false>
__global__ __launch_bounds__(512, 2) void gemm8p_kernel(const GemmPair pp, const P8Sched sc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;      // wave row (group) / wave column
    // this wave's fragment bases inside a k-tile buffer
    const int a_base = wr * 64 * 128;                     // + sub * P8_HALF + i * 16 * 128
    const int b_base = 2 * P8_HALF + wc * 32 * 128;       // + sub * P8_HALF + j * 16 * 128
    const int nwg = gridDim.x;

    // tile -> (problem, tile id): every round of nwg tiles is dealt XCD-contiguously
    auto locate = [&](int tile, P8Tile& t) __attribute__((always_inline)) {
        const int round0 = tile - (int)blockIdx.x;
        const int in_round = min(nwg, sc.tiles_total - round0);
        int id = round0 + xcd_remap(blockIdx.x, in_round);
        const bool second = PAIR && id >= sc.tiles_a;
        if (second) id -= sc.tiles_a;
        t.second = second;
        if (second) p8_setup(t, pp.b, id, wave);
        else p8_setup(t, pp.a, id, wave);
    };
    // the seven items the steady state would have issued before phase 0 of k-tile 0, in its order: A0 W0 W1 A1 of
    // k-tile 0 (buffer 0), then A0 W0 W1 of k-tile 1 (buffer 1)
    auto issue_first = [&](const P8Tile& t) __attribute__((always_inline)) {
        p8_stage(t, smem, wave, 0, 0, 0); p8_stage(t, smem, wave, 0, 2, 0); p8_stage(t, smem, wave, 0, 3, 0); p8_stage(t, smem, wave, 0, 1, 0);
    };
    auto issue_second = [&](const P8Tile& t) __attribute__((always_inline)) {
        p8_stage(t, smem, wave, 1, 0, 1); p8_stage(t, smem, wave, 1, 2, 1); p8_stage(t, smem, wave, 1, 3, 1);
    };

    // experiment: s_memtime at the tile milestones, wave 0 of every workgroup, 8 stamps per tile
    [[maybe_unused]] int stamp_i = 0;
    auto stamp = [&](int k) __attribute__((always_inline)) {
#ifdef ADVGRPO_EXPERIMENTS
        if (sc.stamps && wave == 0 && stamp_i < 8) {
            const unsigned long long tm = __builtin_readcyclecounter();
            if (p8_lane() == 0) sc.stamps[((size_t)blockIdx.x * 8 + stamp_i) * 8 + k] = tm;
        }
#else
        (void)k;
#endif
    };
    P8Tile t;
    locate(blockIdx.x, t);
    issue_first(t);
    issue_second(t);
    for (int tile = blockIdx.x; tile < sc.tiles_total; tile += nwg) {
        const int nk = t.nk;
        const int n_items = 4 * nk;                       // ring items of this output tile, in issue (= first-read) order
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        // per-lane fragment offsets, recomputed per tile from an opaque copy of the lane id: kept live across the epilogue
        // they were spilled, and the reload's conservative s_waitcnt vmcnt(0) ended up INSIDE the k loop (draining the DMA)
        int frag_off[2];
        {
            const int l = p8_lane();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) frag_off[ks] = (l & 15) * 128 + (((ks * 4 + (l >> 4)) ^ (l & 7)) << 4);
        }
        // the first two items must have landed for the first reads
        stamp(0);
        p8_wait_inflight(min(7, n_items) - 2);
        __builtin_amdgcn_s_barrier();
        stamp(1);
        if (wr == 1) __builtin_amdgcn_s_barrier();       // stagger: group 1 runs one barrier behind

        bf16x8_t af0[2][4], af1[2][4], b0[2][2], b1[2][2];
        auto read_a = [&](const char* buf, int sub, bf16x8_t (&a)[2][4]) __attribute__((always_inline)) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[ks][i] = *reinterpret_cast<const bf16x8_t*>(buf + a_base + sub * P8_HALF + i * 16 * 128 + frag_off[ks]);
        };
        auto read_b = [&](const char* buf, int sub, bf16x8_t (&b)[2][2]) __attribute__((always_inline)) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    b[ks][j] = *reinterpret_cast<const bf16x8_t*>(buf + b_base + sub * P8_HALF + j * 16 * 128 + frag_off[ks]);
        };
        // end of a load segment at global phase g (= 4 kt + ph): everything first read in phase g + 1 must have landed
        // (items 0 .. g + 2 of the issue order); 8 + g items have been issued (capped by n_items)
        auto close_load = [&](int g, bool steady) __attribute__((always_inline)) {
            if (steady) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            else p8_wait_inflight(min(8 + g, n_items) - min(g + 3, n_items));
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
#define P8_COMPUTE(MH, NH, AF, BF)                                                                                      \
        do {                                                                                                            \
            __builtin_amdgcn_s_setprio(1);                                                                              \
            if constexpr (FP8) {                                                                                        \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                           \
                    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                       \
                        acc[(MH) * 4 + i][(NH) * 2 + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(            \
                            p8_cat(BF[0][j], BF[1][j]), p8_cat(AF[0][i], AF[1][i]), acc[(MH) * 4 + i][(NH) * 2 + j],    \
                            0, 0, 0, 0, 0, 0);                                                                          \
            } else {                                                                                                    \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                            \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                           \
                    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                       \
                        acc[(MH) * 4 + i][(NH) * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                      \
                            BF[ks][j], AF[ks][i], acc[(MH) * 4 + i][(NH) * 2 + j], 0, 0, 0);                            \
            }                                                                                                           \
            __builtin_amdgcn_s_setprio(0);                                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                                          \
            __builtin_amdgcn_s_barrier();                                                                               \
            __builtin_amdgcn_sched_barrier(0);                                                                          \
        } while (0)

        // Phases of k-tile kt (buffer cur), fragments kept in registers:
        //   ph0  read W sub 0            fill A1(kt+1)   compute (A0, W0)        [A sub 0 was read in ph3 of kt-1]
        //   ph1  read W sub 1            fill A0(kt+2)   compute (A0, W1)
        //   ph2  read A sub 1            fill W0(kt+2)   compute (A1, W1)
        //   ph3  read A sub 0 of kt+1    fill W1(kt+2)   compute (A1, W0)
        auto ktile = [&](int cur, int kt, bool steady) __attribute__((always_inline)) {
            const char* buf = smem + cur * P8_BUF;
            const char* nxt = smem + (cur ^ 1) * P8_BUF;
            const int g = 4 * kt;
            read_b(buf, 0, b0);
            p8_stage(t, smem, wave, cur ^ 1, 1, kt + 1);
            close_load(g, steady);
            P8_COMPUTE(0, 0, af0, b0);
            read_b(buf, 1, b1);
            p8_stage(t, smem, wave, cur, 0, kt + 2);
            close_load(g + 1, steady);
            P8_COMPUTE(0, 1, af0, b1);
            read_a(buf, 1, af1);
            p8_stage(t, smem, wave, cur, 2, kt + 2);
            close_load(g + 2, steady);
            P8_COMPUTE(1, 1, af1, b1);
            if (kt + 1 < nk) read_a(nxt, 0, af0);
            p8_stage(t, smem, wave, cur, 3, kt + 2);
            close_load(g + 3, steady);
            P8_COMPUTE(1, 0, af1, b0);
        };
        read_a(smem, 0, af0);
        int kt = 0;
        for (; kt + 3 < nk; kt += 2) {                   // both k-tiles issue all of their re-fills: constant waits
            ktile(0, kt, true);
            ktile(1, kt + 1, true);
        }
        for (; kt < nk; kt += 2) {
            ktile(0, kt, false);
            if (kt + 1 < nk) ktile(1, kt + 1, false);
        }
#undef P8_COMPUTE
        if (wr == 0) __builtin_amdgcn_s_barrier();       // matches group 1's stagger barrier: every ring read is complete
        stamp(2);

        // ---- tile boundary: request the next tile's first k-tile (buffer 0), run the epilogue through buffer 1, then
        // request the rest of the next tile's pipeline fill
        const bool cur_second = t.second;
        const int mw0 = t.m0 + wr * 128, nw0 = t.n0 + wc * 64;
        const bool more = tile + nwg < sc.tiles_total;
        if (more) {
            locate(tile + nwg, t);
            issue_first(t);
        }
        stamp(3);
        {
            const GemmParams& p = (PAIR && cur_second) ? pp.b : pp.a;
            p8_epilogue<EPI>(p, acc, mw0, nw0, smem + P8_BUF + wave * P8_SCRATCH);
        }
        stamp(4);
        if (more) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                 // every wave is done with its scratch in buffer 1
            stamp(5);
            issue_second(t);
        }
        ++stamp_i;
    }
}

// experiment only: device buffer of the s_memtime stamps of the last launch (ADVGRPO_P8_STAMPS=1)
extern unsigned long long* g_p8_stamps;

template <int EPI, bool FP8 = false>
int launch8p(const GemmPair& pp, const P8Sched& sc, hipStream_t s) {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
            set_error("gemm8p: cannot query the device");
            return -2;
        }
        cus = prop.multiProcessorCount;
    }
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm8p_kernel<true, EPI, FP8>), hipFuncAttributeMaxDynamicSharedMemorySize, P8_LDS);
        attr_set = true;
    }
    const int grid = sc.tiles_total < cus ? sc.tiles_total : cus;
    P8Sched sc2 = sc;
#ifdef ADVGRPO_EXPERIMENTS
    {
        static unsigned long long* stamps = nullptr;
        static int want = -1;
        if (want < 0) { const char* e = getenv("ADVGRPO_P8_STAMPS"); want = (e && atoi(e)) ? 1 : 0; }
        if (want && !stamps) { (void)hipMalloc((void**)&stamps, 256 * 8 * 8 * 8); }
        if (want) { (void)hipMemsetAsync(stamps, 0, 256 * 8 * 8 * 8, s); g_p8_stamps = stamps; }
        sc2.stamps = want ? stamps : nullptr;
    }
#endif
    hipLaunchKernelGGL((gemm8p_kernel<true, EPI, FP8>), dim3(grid), dim3(512), P8_LDS, s, pp, sc2);   // a single problem is a pair with an empty second half
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}


}  // namespace advgrpo
