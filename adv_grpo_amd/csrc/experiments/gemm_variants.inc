// Experimental GEMM tile variants (NOT part of the product library): the BK = 32 ring kernel (variants 11 / 17) and the
// ping-pong kernel (20 / 21 / 23) that the eight-phase kernel of gemm8p_kernel.hpp superseded.  Compiled only with
// `make EXPERIMENTS=1` (-DADVGRPO_EXPERIMENTS -> libadvgrpo_experiments.so), textually included into gemm.hip inside
// namespace advgrpo after the two-stage kernel.  Measurements: DESIGN.md section 6.
// ------------------------------------------------------------------------------------------------------------
// Deep-pipelined variant for short-K problems (the MMDiT's K = 1536 Linears): BK = 32, a 4-slot LDS ring, LDS-DMA
// for three tiles kept in flight ACROSS the workgroup barrier (counted s_waitcnt vmcnt + raw s_barrier, guide
// section 5 "Pipelining across barriers").  The 2-stage kernel above drains the DMA queue before every barrier
// (hipcc's __syncthreads), which exposes the HBM/L2 latency of each 64-deep tile once per iteration; here a tile
// is requested three iterations before it is consumed.  Same fragment layout, swizzle idea and epilogue.
//   LDS tile image: rows of 32 k = 64 B = 4 chunks; one DMA instruction (1 KiB) covers 16 rows; chunk c of row r
//   sits at slot c ^ ((-(r >> 2)) & 3), which spreads each ds_read_b128 service group over all 16 bank slots.
template <int BM, int BN, int NS, int WM, int WN>
__device__ __forceinline__ void gemm_bf16_pipe_body(const GemmParams& p, const int bid, const int by, char* smem) {
    constexpr int BK = 32, AHEAD = NS - 2;   // tiles kept in flight beyond the one being consumed
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INST = BM / 16 / NW, B_INST = BN / 16 / NW;     // 16-row DMA instructions per wave
    static_assert(A_INST >= 1 && B_INST >= 1, "tile too small for the wave count");
    constexpr int LOADS = A_INST + B_INST;                        // per wave per tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int swz = xcd_remap(bid, tiles_m * tiles_n);
    int tile_m, tile_n;
    tile_coords(swz, tiles_m, tiles_n, (p.debug >> 8) ? (p.debug >> 8) : 4, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int bz = by;
    const bf16_t* __restrict__ A = p.A + (int64_t)bz * p.strideA;
    const bf16_t* __restrict__ W = p.W + (int64_t)bz * p.strideW;

    const int lrow = lane >> 2;                           // row inside the 16-row instruction
    // chunk c of row r sits at slot c ^ h(r), h = (-(r >> 2)) & 3: with ds_read_b128's 16-lane service groups
    // ({0-3,12-15,20-27}, ...) every group then touches 16 distinct 16-byte bank slots
    const int schunk = (lane & 3) ^ ((0 - (lrow >> 2)) & 3);
    const bf16_t* a_src[A_INST];
    const bf16_t* b_src[B_INST];
#pragma unroll
    for (int it = 0; it < A_INST; ++it) {
        int r = m0 + (wave + it * NW) * 16 + lrow;
        r = r < p.M ? r : p.M - 1;
        const int64_t ar = seg_row(r, p.a_seg_rows, p.a_seg_stride, p.a_seg_off);
        a_src[it] = A + ar * p.lda + schunk * 8;
    }
#pragma unroll
    for (int it = 0; it < B_INST; ++it) {
        int r = n0 + (wave + it * NW) * 16 + lrow;
        r = r < p.N ? r : p.N - 1;
        b_src[it] = W + (int64_t)r * p.ldw + schunk * 8;
    }
    auto stage = [&](int slot, int kt) __attribute__((always_inline)) {
        char* base = smem + slot * STAGE;
#pragma unroll
        for (int it = 0; it < A_INST; ++it)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[it] + kt * BK), (lds_ptr_t)(base + (wave + it * NW) * 1024), 16, 0, 0);
#pragma unroll
        for (int it = 0; it < B_INST; ++it)
            __builtin_amdgcn_global_load_lds((gptr_t)(b_src[it] + kt * BK),
                                             (lds_ptr_t)(base + A_BYTES + (wave + it * NW) * 1024), 16, 0, 0);
    };
    // fragment byte offset inside a tile: row (lane&15) * 64 B + swizzled chunk (lane>>4)
    const int frow = lane & 15;
    const int frag_off = frow * 64 + ((((lane >> 4)) ^ ((0 - (frow >> 2)) & 3)) << 4);

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / BK;
    // prologue: NS-1 tiles in flight
#pragma unroll
    for (int t = 0; t < NS - 1; ++t)
        if (t < nk) stage(t, t);
    int slot = 0;                      // slot of tile kt
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt must have landed: allow the younger tiles (at most AHEAD) to stay in flight
        const int ahead = min(nk - 1 - kt, AHEAD);
        if (ahead >= 2) wait_vm<2 * LOADS>();
        else if (ahead == 1) wait_vm<LOADS>();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // the slot of tile kt-1 is free now (every wave passed the barrier after reading it): refill it
        const int fill = slot == 0 ? NS - 1 : slot - 1;
        if (kt + NS - 1 < nk) stage(fill, kt + NS - 1);
        const char* ta = smem + slot * STAGE + wm * TM * 64;
        const char* tb = smem + slot * STAGE + A_BYTES + wn * TN * 64;
        slot = slot == NS - 1 ? 0 : slot + 1;
        bf16x8_t af[FM], bf[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(ta + i * 1024 + frag_off);
#pragma unroll
        for (int j = 0; j < FN; ++j) bf[j] = *reinterpret_cast<const bf16x8_t*>(tb + j * 1024 + frag_off);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);
    }
    gemm_epilogue<FM, FN, TM, TN>(p, acc, m0, n0, wm, wn, bz, lane, smem, wave);
}

template <int BM, int BN, int NS, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_bf16_pipe_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gemm_bf16_pipe_body<BM, BN, NS, WM, WN>(p, blockIdx.x, blockIdx.y, smem);
}

template <int BM, int BN, int NS, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_bf16_pipe_pair_kernel(const GemmPair pp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bid = blockIdx.x;
    if (bid < pp.tiles_a) gemm_bf16_pipe_body<BM, BN, NS, WM, WN>(pp.a, bid, 0, smem);
    else gemm_bf16_pipe_body<BM, BN, NS, WM, WN>(pp.b, bid - pp.tiles_a, 0, smem);
}

template <int BM, int BN, int NS, int WM, int WN>
static int launch_pipe(const GemmParams& p, hipStream_t s) {
    constexpr int lds = NS * (BM + BN) * 32 * 2;
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_pipe_kernel<BM, BN, NS, WM, WN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_bf16_pipe_kernel<BM, BN, NS, WM, WN>), dim3(tiles, p.batch), dim3(WM * WN * 64), lds, s, p);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// Ping-pong variant: 8 waves in two groups of four that run half a phase apart, so that while one group is in its
// MFMA segment the other is in its LDS-read + DMA-issue segment (one wave of each group per SIMD: the matrix pipe
// and the LDS/VMEM paths are busy at the same time instead of taking turns behind a common barrier).
//   * BK = 32 tiles in a 4-slot LDS ring; the DMA for tile t+2 is issued in the load segment of tile t and waited
//     for (counted s_waitcnt vmcnt) in the segment just before the barrier that precedes its first read, so a
//     tile has two full compute segments to arrive and every LDS hazard (read-after-DMA, DMA-after-read) is
//     separated by at least one workgroup barrier -- no placement or timing assumption.
//   * segment structure per tile and wave:  [ds_read fragments of tile t, issue DMA of tile t+2] s_barrier
//     [s_waitcnt lgkmcnt(0); MFMAs] s_barrier ; group 1 executes one extra barrier up front (stagger) and group 0
//     one extra at the end, so both groups arrive at every barrier.
template <int BM, int BN, int NS, int WM, int WN>
__global__ __launch_bounds__(512) void gemm_bf16_pp_kernel(const GemmParams p) {
    constexpr int BK = 32, NW = 8;
    static_assert(NS == 3 || NS == 4, "ring depth");
    static_assert(WM * WN == NW, "eight waves");
    constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INST = BM / 16 / NW, B_INST = BN / 16 / NW;
    constexpr int LOADS = A_INST + B_INST;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                       // waves w and w+4 share a SIMD: one of each group per SIMD
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int swz = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    int tile_m, tile_n;
    tile_coords(swz, tiles_m, tiles_n, (p.debug >> 8) ? (p.debug >> 8) : 4, tile_m, tile_n);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int bz = blockIdx.y;
    const bf16_t* __restrict__ A = p.A + (int64_t)bz * p.strideA;
    const bf16_t* __restrict__ W = p.W + (int64_t)bz * p.strideW;
    const int lrow = lane >> 2;
    const int schunk = (lane & 3) ^ ((0 - (lrow >> 2)) & 3);
    const bf16_t* a_src[A_INST];
    const bf16_t* b_src[B_INST];
#pragma unroll
    for (int it = 0; it < A_INST; ++it) {
        int r = m0 + (wave + it * NW) * 16 + lrow;
        r = r < p.M ? r : p.M - 1;
        const int64_t ar = seg_row(r, p.a_seg_rows, p.a_seg_stride, p.a_seg_off);
        a_src[it] = A + ar * p.lda + schunk * 8;
    }
#pragma unroll
    for (int it = 0; it < B_INST; ++it) {
        int r = n0 + (wave + it * NW) * 16 + lrow;
        r = r < p.N ? r : p.N - 1;
        b_src[it] = W + (int64_t)r * p.ldw + schunk * 8;
    }
    auto stage = [&](int slot, int kt) __attribute__((always_inline)) {
        char* base = smem + slot * STAGE;
#pragma unroll
        for (int it = 0; it < A_INST; ++it)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[it] + kt * BK), (lds_ptr_t)(base + (wave + it * NW) * 1024), 16, 0, 0);
#pragma unroll
        for (int it = 0; it < B_INST; ++it)
            __builtin_amdgcn_global_load_lds((gptr_t)(b_src[it] + kt * BK),
                                             (lds_ptr_t)(base + A_BYTES + (wave + it * NW) * 1024), 16, 0, 0);
    };
    const int frow = lane & 15;
    const int frag_off = frow * 64 + ((((lane >> 4)) ^ ((0 - (frow >> 2)) & 3)) << 4);
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = (p.debug & 8) ? 2 : p.K / BK;
    stage(0, 0);
    if (nk > 1) stage(1, 1);
    if (nk > 1) wait_vm<LOADS>();
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                     // tile 0 is complete for everybody
    if (grp == 1) __builtin_amdgcn_s_barrier();       // stagger: group 1 runs one segment behind
    int slot = 0, slot2 = 2;                          // ring slots of tile kt and tile kt+2
    for (int kt = 0; kt < nk; ++kt) {
        // ---- load segment: fragments of tile kt, DMA of tile kt+2
        const char* ta = smem + slot * STAGE + wm * TM * 64;
        const char* tb = smem + slot * STAGE + A_BYTES + wn * TN * 64;
        bf16x8_t af[FM], bf[FN];
        if (!(p.debug & 2) || kt == 0) {
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(ta + i * 1024 + frag_off);
#pragma unroll
            for (int j = 0; j < FN; ++j) bf[j] = *reinterpret_cast<const bf16x8_t*>(tb + j * 1024 + frag_off);
        }
        if (kt + 2 < nk && !(p.debug & 1)) stage(slot2, kt + 2);
        slot = slot + 1 == NS ? 0 : slot + 1;
        slot2 = slot2 + 1 == NS ? 0 : slot2 + 1;
        if (grp == 1) {   // tile kt+1 is first read right after the next barrier (by group 0)
            if (kt + 2 < nk) wait_vm<LOADS>();
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // with a 3-slot ring group 0 refills the slot of tile kt (= slot of tile kt+3) right after the next
            // barrier: this group's fragment reads of it must have completed, not just been issued
            if (NS == 3) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // ---- compute segment
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[j], af[i], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        if (grp == 0) {
            if (kt + 2 < nk) wait_vm<LOADS>();
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();       // matches group 1's stagger barrier
    if (p.debug & 4) { if (acc[0][0][0] != 12345.678f) return; }
    gemm_epilogue<FM, FN, TM, TN>(p, acc, m0, n0, wm, wn, bz, lane, smem, wave);
}

template <int BM, int BN, int NS, int WM, int WN>
static int launch_pp(const GemmParams& p, hipStream_t s) {
    constexpr int lds = NS * (BM + BN) * 32 * 2;
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_pp_kernel<BM, BN, NS, WM, WN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_bf16_pp_kernel<BM, BN, NS, WM, WN>), dim3(tiles, p.batch), dim3(512), lds, s, p);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

template <int BM, int BN, int NS, int WM, int WN>
static int launch_pipe_pair(const GemmParams& a, const GemmParams& b, hipStream_t s) {
    constexpr int lds = NS * (BM + BN) * 32 * 2;
    GemmPair pp{a, b, ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN)};
    const int tiles_b = ((b.M + BM - 1) / BM) * ((b.N + BN - 1) / BN);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_pipe_pair_kernel<BM, BN, NS, WM, WN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_bf16_pipe_pair_kernel<BM, BN, NS, WM, WN>), dim3(pp.tiles_a + tiles_b), dim3(WM * WN * 64), lds,
                       s, pp);
    ADVGRPO_LAUNCH_CHECK();
    return 0;
}

