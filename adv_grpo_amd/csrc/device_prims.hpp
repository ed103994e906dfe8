// device_prims.hpp -- the small device primitives every kernel file needs: vector / address-space types, bf16 x 8 / x 4 packing,
// the packed convert, the transpose-read MFMA operand, the hand-written LDS-DMA instruction, counted waits, compile-time loops and tags, the segmented row
// map and the scheduling macros.  One definition each, with the reason it is written the way it is; included through
// common.hpp (which it needs for bf2f / f2bf).  A kernel file keeps only its own experiment knobs as thin wrappers.
#pragma once
#include <type_traits>
#include <utility>

namespace advgrpo {

// ---- vector and address-space types
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;    // one ds_read_tr16_b64
typedef __attribute__((ext_vector_type(8))) short s16x8;    // two of them: an MFMA fragment before the bit cast
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;   // ... and after it: one bf16 MFMA A / B operand
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;

// ---- compile-time indices, tags and loops
template <int N>
using int_c = std::integral_constant<int, N>;
typedef std::integral_constant<bool, true> true_c;      // e.g. "first tile" / "last tile" arguments of a pipeline step
typedef std::integral_constant<bool, false> false_c;
template <int N0, class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(int_c<N0 + Is>{}), ...);
}
// f(int_c<0>{}), ..., f(int_c<N - 1>{}): indices stay compile-time constants, so accumulators never leave the register file
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl<0>(f, std::make_integer_sequence<int, N>{});
}
// f(int_c<N0>{}), ..., f(int_c<N1 - 1>{})
template <int N0, int N1, class F>
__device__ __forceinline__ void static_for_range(F&& f) {
    static_for_impl<N0>(f, std::make_integer_sequence<int, N1 - N0>{});
}

// ---- 8 bf16 in a uint4 <-> 8 f32 (the 16-byte lane access of the row kernels)
__device__ __forceinline__ void unpack8(const uint4& r, float o[8]) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[2 * k] = bf2f((bf16_t)(w[k] & 0xffffu));
        o[2 * k + 1] = bf2f((bf16_t)(w[k] >> 16));
    }
}
__device__ __forceinline__ uint4 pack8(const float o[8]) {
    uint4 r;
    r.x = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
    r.y = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
    r.z = (uint32_t)f2bf(o[4]) | ((uint32_t)f2bf(o[5]) << 16);
    r.w = (uint32_t)f2bf(o[6]) | ((uint32_t)f2bf(o[7]) << 16);
    return r;
}
// four f32 -> 4 bf16 in a uint2 (the 8-byte lane store of an MFMA accumulator row)
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
    uint2 r;
    r.x = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
    r.y = (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16);
    return r;
}
// 8 consecutive f32 (two 16-byte loads)
__device__ __forceinline__ void ld8_f32(const float* q, float o[8]) {
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// ---- two f32 -> packed bf16 (v_cvt_pk_bf16_f32, round-to-nearest-even; lo in bits 0..15).  Through the compiler, NOT
// inline asm: in the attention pipelines the packed probabilities are written into registers that MFMAs issued a slot
// earlier may still be reading as their B operand, and the hazard recogniser only pads instructions it knows (an asm
// statement there produced wrong probabilities for half of the query lanes).
__device__ __forceinline__ uint32_t cvt_pk_bf16(f32x2 v) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) { return cvt_pk_bf16(f32x2{lo, hi}); }
// (through the compiler as well, which fuses the pair into v_max3_f32: as an asm statement its reads of the score
// accumulators were not padded against the MFMAs that had just written them, and the reference maximum of the attention
// forward came out of half-written registers)
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// ---- a 16 x 32 bf16 MFMA operand out of a row-major LDS tile through the hardware transpose: two ds_read_b64_tr_b16, the second
// 16 rows further on (lo -> elements 0..3, hi -> 4..7).  ld_tr_s16x8 is the fragment before the bit cast, for a caller that
// zeroes elements of it (the ragged chunks of gemm_tn.hip).
__device__ __forceinline__ s16x8 ld_tr_s16x8(const void* lo_ptr, const void* hi_ptr) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_ptr));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_ptr));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8_t ld_tr_frag(const void* lo_ptr, const void* hi_ptr) {
    return __builtin_bit_cast(bf16x8_t, ld_tr_s16x8(lo_ptr, hi_ptr));
}

// ---- LDS-DMA: one instruction, 64 lanes x 16 bytes -> LDS [lds, lds + 1 KiB), lane-linear.
// Hand-written (m0 = the LDS address, the s_nop between the write of m0 and its use, the memory clobber), not
// __builtin_amdgcn_global_load_lds, for two reasons on record:
//   * issued through the builtin the compiler treats the DMA as a possible alias of every later ds_read and puts
//     s_waitcnt vmcnt(0) in front of the first fragment read of the SAME iteration (head-dim-64 attention ring);
//   * the builtin form keeps every per-lane source as a 64-bit VGPR pair and re-adds the k offset on the VALU: in the
//     eight-phase GEMM 24 VGPRs and 8 v_lshl_add_u64 per k-tile more than the SGPR-base form, enough to spill inside the
//     main loop.
// Ring hazards (a slot overwritten while it is still read, a slot read before it has arrived) are the caller's: a counted
// wait (wait_vm) + barrier.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char*)(p));
}
// source = uniform (SGPR) base + 32-bit per-lane byte offset
__device__ __forceinline__ void lds_dma16(const void* base, uint32_t off, uint32_t lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(lds) : "memory");
}
// source = a 64-bit pointer per lane
__device__ __forceinline__ void lds_dma16_ptr(const void* src, const char* lds) {
    const uint32_t l = lds_addr(lds);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(l) : "memory");
}

// ---- wait until at most N of this wave's vector-memory operations (DMA instructions included) are outstanding
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- row of token m through the (seg_rows, seg_stride, seg_off) map of the GEMM family:
// (m / seg_rows) * seg_stride + seg_off + m % seg_rows; seg_rows = 0: identity
__device__ __forceinline__ int64_t seg_row(int m, int seg_rows, int64_t seg_stride, int64_t seg_off) {
    int64_t row = m;
    if (seg_rows > 0) {
        const int b = m / seg_rows;
        row = (int64_t)b * seg_stride + seg_off + (m - b * seg_rows);
    }
    return row;
}

// ---- scheduling of the hand-pipelined kernels (one MFMA slot = one MFMA + the VALU / LDS / DMA work in its shadow)
// a fence the compiler's scheduler moves nothing across
#define ADVGRPO_SB() __builtin_amdgcn_sched_barrier(0)
// keeps a value (and the instructions that made it) in the slot where it was written: without it e.g. the row-sum adds of
// the attention forward are sunk out of the iteration (their result is only read at the very end) and all 32 probabilities
// stay live across it
#define ADVGRPO_PIN(x) asm volatile("" : "+v"(x))
#define ADVGRPO_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

}  // namespace advgrpo
