// Body of the 8-wave 256x256 kernels, included by gemm.hip into big::gemm256_kernel<SWIGLU, ROPE> and big::gemm256d_kernel: the
// prologue, the DMA staging, the hand-dealt K-step schedule and the stream-K slab store, once.  The including kernel provides
//     GemmArgs p                      its argument
//     constexpr bool SWIGLU, ROPE     the epilogue variant
//     constexpr bool PERMUTED_W       the layout of the W tile: false = rows in order, swizzled by row & 7 like X, LDS-staged epilogue;
//                                     true = the 4-wave kernel's W-row permutation (w4_* in gemm.hip) and its register-direct epilogue
// and every place where the two layouts differ is an `if constexpr (PERMUTED_W)` whose arms hold each variant's own expressions.
// This is an included text and not a function template on purpose: a device function is optimized on its own before it is inlined into
// the kernel that calls it, and the kernel then comes out with commuted operands and renumbered registers -- as a text, both kernels
// compile to the instructions they had as two copies (profiles/gemm_refactor_isa.txt).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 3, wm = wave >> 2;
    const TileRaster t = raster256(p);
    const int bid = t.bid, slice = t.slice, bm = t.bm, bn = t.bn;
    const bool split = t.split;
    const int m0 = bm * BM, n0 = bn * BN;
    const int nk_total = p.K / BK;
    const bool w_tiled = p.flags & EPI_W_TILED, x_tiled = p.flags & EPI_X_TILED;

    // DMA: a 1-KiB piece = 8 rows x 128 B; wave w stages pieces 4w..4w+3 of X and of W.
    const int srow = lane >> 3;
    const int schunk = (lane & 7) ^ srow;
    const elem_t* xsrc[4];
    const elem_t* wsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (wave * 4 + i) * 8 + srow;
        xsrc[i] = x_tiled ? p.X + (((long)bm * nk_total) * BM + r) * BK + schunk * 8
                          : p.X + (long)min(m0 + r, p.M - 1) * p.ldx + schunk * 8;
        if constexpr (PERMUTED_W) {
            const int wchunk = (lane & 7) ^ w4_row_swizzle<false>(r);           // permuted W rows: the W tile's own swizzle
            wsrc[i] = w_tiled ? p.W + (((long)bn * nk_total) * BN + r) * BK + wchunk * 8
                              : p.W + (long)min(n0 + r, p.N - 1) * p.ldw + wchunk * 8;
        } else {
            wsrc[i] = w_tiled ? p.W + (((long)bn * nk_total) * BN + r) * BK + schunk * 8
                              : p.W + (long)min(n0 + r, p.N - 1) * p.ldw + schunk * 8;
        }
    }
    const long xstep = x_tiled ? BM * BK : BK, wstep = w_tiled ? BN * BK : BK;    // elements between consecutive K-tiles
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
    const uint32_t piece_off = wave * 4 * 1024;
    auto stage = [&](int kt) {
        const uint32_t bx = lds_base + (kt & 1) * SLOT_BYTES + piece_off;
        const long kox = (long)kt * xstep, kow = (long)kt * wstep;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            glds16(xsrc[i] + kox, bx + i * 1024);
            glds16(wsrc[i] + kow, bx + OP_BYTES + i * 1024);
        }
    };

    const int fr = lane & 15, fg = lane >> 4;
    int swz[2];
    swz[0] = ((0 + fg) ^ (lane & 7)) << 4;
    swz[1] = ((4 + fg) ^ (lane & 7)) << 4;
    int wswz[2];                                      // PERMUTED_W: swizzle = fr >> 1 for the reading lane (see w4_row_swizzle)
    wswz[0] = ((0 + fg) ^ (fr >> 1)) << 4;
    wswz[1] = ((4 + fg) ^ (fr >> 1)) << 4;
    const int xoff = (wm * 128 + fr) * (BK * 2);
    const int woff = OP_BYTES + (wn * 64 + (PERMUTED_W ? w4_lane_row<false>(fr) : fr)) * (BK * 2);
    // fragment r of half step kk of tile kt: r < 4 -> W fragment r, else X fragment r - 4
    auto read1 = [&](int kt, int kk, Frags& f, int r) {
        if constexpr (PERMUTED_W) {
            const char* base = smem + (kt & 1) * SLOT_BYTES;
            if (r < 4) f.w[r] = *(const uint4*)(base + wswz[kk] + woff + w4_frag_row<false>(r) * (BK * 2));
            else f.x[r - 4] = *(const uint4*)(base + swz[kk] + xoff + (r - 4) * 16 * (BK * 2));
        } else {
            const char* base = smem + (kt & 1) * SLOT_BYTES + swz[kk];
            if (r < 4) f.w[r] = *(const uint4*)(base + woff + r * 16 * (BK * 2));
            else f.x[r - 4] = *(const uint4*)(base + xoff + (r - 4) * 16 * (BK * 2));
        }
    };

    f32x4_t acc[1][4][8];                             // ([1]: the shape w4_direct_epilogue takes for one 64-column half)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[0][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int nk = p.K / BK;                                // >= 2 (host dispatch, also per K-slice)
    if (split) {
        const int kt0 = (int)((long)nk * slice / p.sk), kt1 = (int)((long)nk * (slice + 1) / p.sk);
#pragma unroll
        for (int i = 0; i < 4; ++i) { xsrc[i] += (long)kt0 * xstep; wsrc[i] += (long)kt0 * wstep; }
        nk = kt1 - kt0;
    }
    // Same step schedule as the 4-wave kernel (see there), 64 MFMA slots per wave and step: the 12 fragment reads of the tile's second
    // half first, barrier A, the 8 DMA pieces of tile kt+2 dealt out one per 6 slots (a burst of all 64 pieces of a CU right behind
    // the barrier measured 3-7 % slower end to end: the memory pipe wants an even stream), barrier B with the newest pieces still in
    // flight, then the first-half fragments of tile kt+1.  The last two steps re-fetch the last tile into a 16-KiB dump.
    // (W8_BAR_A, W8_DMA_STRIDE, W8_BAR_B, W8_FA_STRIDE: gemm.hip)
    constexpr int USE_ORDER[12] = {0, 4, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11};    // w0, x0, w1..w3, x1..x7
    auto mma1 = [&](const Frags& f, int s) {
        const int j = s >> 2, i = s & 3;
        acc[0][i][j] = mfma16(f.w[i], f.x[j], acc[0][i][j]);
    };
    stage(0);
    stage(1);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile 0 landed, tile 1 in flight
    __builtin_amdgcn_s_barrier();
    Frags fa, fb;                                     // fa: half 0 of the current tile, fb: half 1
#pragma unroll
    for (int r = 0; r < 12; ++r) read1(0, 0, fa, r);
    const uint32_t dump = lds_base + LDS_BYTES;
#pragma clang loop unroll(disable)
    for (int kt = 0; kt < nk; ++kt) {
        const bool with_dma = kt + 2 < nk;
        const int ktd = with_dma ? kt + 2 : nk - 1;
        const long kox = (long)ktd * xstep, kow = (long)ktd * wstep;
        const uint32_t bx = with_dma ? lds_base + (kt & 1) * SLOT_BYTES + piece_off : dump;
        const uint32_t bw = with_dma ? bx + OP_BYTES : dump + 4096;
#pragma clang loop unroll(full)
        for (int s = 0; s < 64; ++s) {
            if (s == W8_BAR_A) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            if (s == W8_BAR_B) {
                asm volatile("s_waitcnt vmcnt(%0)" :: "n"(W8_INFLIGHT) : "memory");
                __builtin_amdgcn_s_barrier();
            }
            if (s < 12) read1(kt, 1, fb, s);
            if (s >= W8_BAR_B && (s - W8_BAR_B) % W8_FA_STRIDE == 0 && (s - W8_BAR_B) / W8_FA_STRIDE < 12)
                read1(kt + 1, 0, fa, USE_ORDER[(s - W8_BAR_B) / W8_FA_STRIDE]);
            if (s >= W8_BAR_A && (s - W8_BAR_A) % W8_DMA_STRIDE == 0 && (s - W8_BAR_A) / W8_DMA_STRIDE < 8) {
                const int pc = (s - W8_BAR_A) / W8_DMA_STRIDE;
                if (pc < 4) glds16(xsrc[pc] + kox, bx + pc * 1024);
                else glds16(wsrc[pc - 4] + kow, bw + (pc - 4) * 1024);
            }
            mma1(s < 32 ? fa : fb, s & 31);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // (the dump's pieces may still be landing: they touch nothing the epilogue uses, and s_endpgm waits for them)

    // ---- epilogue: acc[0][i][j][r] = D[n][m = m0 + wm*128 + j*16 + fr] with n = n0 + wn*64 + i*16 + 4*fg + r, resp. (PERMUTED_W)
    // the physical W row n0 + wn*64 + w4_acc_row(0, i, fg) + r ----------
    if (split) {
        float* slab = p.ws + ((long)(bid - p.t_full) * p.sk + slice) * (BM * BN);
#pragma clang loop unroll(full)
        for (int j = 0; j < 8; ++j)
#pragma clang loop unroll(full)
            for (int i = 0; i < 4; ++i) {
                if constexpr (PERMUTED_W) *(f32x4_t*)(slab + (wm * 128 + j * 16 + fr) * BN + wn * 64 + w4_acc_row<false>(0, i, fg)) = acc[0][i][j];
                else *(f32x4_t*)(slab + (wm * 128 + j * 16 + fr) * BN + wn * 64 + i * 16 + fg * 4) = acc[0][i][j];
            }
        return;
    }
    if constexpr (PERMUTED_W) {
        // 16-bit output, 16-byte-aligned rows, whole groups of 8 columns, no activation with a residual: straight from the accumulators
        static_assert(!SWIGLU && !ROPE, "one 64-column half per wave: SwiGLU and RoPE pair columns across two");
        const int fl = p.flags;
        const bool direct = !(fl & (EPI_OUT_F32 | EPI_BIAS_ROUNDED)) && (!(fl & EPI_ACT_MASK) || !(fl & EPI_RESID)) && (p.ldc & 7) == 0 && (p.N & 7) == 0 &&
                            (!(fl & EPI_RESID) || (p.ldr & 7) == 0) && !(fl & ULL_W4_FORCE_STAGED);
        if (direct) {
            w4_direct_epilogue<false, false, 1>(p, acc, lane, m0 + wm * 128, n0 + wn * 64);
            return;
        }
        __builtin_amdgcn_s_barrier();                          // every wave has consumed the last K-tile: LDS is free
        staged_epilogue<false, 8, false, 0, false, 2, false, 1>(p, acc[0], smem + wave * (128 * 144), lane, m0 + wm * 128, n0 + wn * 64);
    } else {
        __builtin_amdgcn_s_barrier();                          // every wave has consumed the last K-tile: LDS is free
        staged_epilogue<SWIGLU, 8, ROPE>(p, acc[0], smem + wave * (128 * 144), lane, m0 + wm * 128, n0 + wn * 64, smem + (wave ^ 1) * (128 * 144));
    }
