// What sam_global_kernel and sam_global_exact_kernel (attention.hip) share, from the LDS declaration down to the score epilogue: the Q
// fragments, the rel-pos tables built on the MFMA, the DMA piece offsets and issue_k / issue_v, the fragment addresses, the accumulators
// with the running maximum, the S tile (qk) and its score epilogue (scores).  Included at the top of each kernel's body, with the
// argument block named `p`; the kernel's own tile loops follow.
// It is a TEXT and not a __device__ function: a function is optimized on its own before it is inlined and its caller a second time, which
// changed sam_global_kernel's register allocation; the same statements compiled directly as the kernel give the instructions they gave
// when they stood in both kernels (mechanism and evidence: profiles/gemm_refactor_isa.txt, profiles/attention_refactor_isa.txt).
    extern __shared__ __attribute__((aligned(256))) char smem[];
    constexpr int NWV = 4, NG = 2, BQ = 16 * NG * NWV, HDP = 128, hd = 80;
    constexpr int KROW = HDP * 2, NKS = 3 /* 96 = 3 x 32 >= hd */, NDS = 5 /* 80 = 5 x 16 */;
    constexpr int TILE = 64 * KROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int nq = p.Sq / BQ;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int head = (slot / nq) * 8 + xcd;
    if (head >= p.B * p.H) return;
    const int qt = slot % nq;
    const int b = head / p.H, h = head % p.H;
    const int q0 = qt * BQ + wave * 16 * NG;                   // this wave's first query; its 32 queries share the grid row qy
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem);
    elem_t* ghl = (elem_t*)(smem + 4 * TILE) + wave * (64 * 16 * NG);     // [64 key rows][32 queries]: rel_h, 16-bit (a tile's read = 64 B)

    uint4 qf[NG][NKS];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const elem_t* qp = p.Q + (long)b * p.q_bs + (long)h * p.q_hs + (long)(q0 + g * 16 + fr) * p.q_ss;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = ks * 32 + fg * 8;
            qf[g][ks] = d < hd ? *(const uint4*)(qp + d) : make_uint4(0, 0, 0, 0);
        }
    }
    // G[q][t] = 16-bit(q . rel_pos[t]) on the MFMA (A = table rows, B = the UNSCALED query fragments): rel_w[q][kw] = Gw[q][qx - kw + 63],
    // rel_h[q][kh] = Gh[q][qy - kh + 63].  Gw: all 127 rows -> this wave's pad (aliases the tile slots, not in use yet) -> 16 registers per
    // group; Gh: the 64 rows qy - kh + 63 -> the wave's LDS table.
    float rw[NG][16];
    {
        elem_t* gw = (elem_t*)(smem + wave * (NG * 4096));      // [group][16 queries][128]
        const int qy = q0 >> 6;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll 2
            for (int st = 0; st < 8; ++st) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                const elem_t* tr = p.rel_w + (long)min(st * 16 + fr, 126) * hd + fg * 8;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const uint4 a = (ks * 32 + fg * 8 < hd) ? *(const uint4*)(tr + ks * 32) : make_uint4(0, 0, 0, 0);
                    acc = mfma16(a, qf[g][ks], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) gw[g * 2048 + fr * 128 + st * 16 + fg * 4 + r] = f2e(acc[r]);   // G[t = st*16 + 4*fg + r][query fr]
            }
#pragma unroll 2
            for (int st = 0; st < 4; ++st) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                const elem_t* tr = p.rel_h + (long)(qy - (st * 16 + fr) + 63) * hd + fg * 8;               // row of key-grid row kh = st*16 + fr
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const uint4 a = (ks * 32 + fg * 8 < hd) ? *(const uint4*)(tr + ks * 32) : make_uint4(0, 0, 0, 0);
                    acc = mfma16(a, qf[g][ks], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) ghl[(st * 16 + fg * 4 + r) * (16 * NG) + g * 16 + fr] = f2e(acc[r]);  // Gh[kh = st*16 + 4*fg + r][query fr]
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // own pad only
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int qx = (q0 + g * 16 + fr) & 63;
#pragma unroll
            for (int i = 0; i < 16; ++i) rw[g][i] = e2f(gw[g * 2048 + fr * 128 + qx - ((i >> 2) * 16 + fg * 4 + (i & 3)) + 63]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (p.q_scale != 1.0f) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) qf[g][ks] = scale_q8(qf[g][ks], p.q_scale);
    }
    __builtin_amdgcn_s_barrier();                              // every wave is done with its pad before tile 0 is DMA'd over it

    // LDS: K ring [2][64 x 256 B] at 0, V ring [2][64 x 256 B] at 2 TILE, rel_h tables behind.  DMA: a tile is 16 pieces of 1 KiB (4 key rows x
    // 16 chunks); a wave issues 4 K + 4 V pieces per step.  The per-lane byte offset of every piece is the same for all 64 tiles; the six
    // chunks of a row that are head-dim padding are not transferred: chunks 10 / 11 of every K row (dims 80..95, read by the last QK k-step)
    // are zeroed once per buffer, the rest is never read.
    const elem_t* kbase = p.K + (long)b * p.k_bs + (long)h * p.k_hs;
    const elem_t* vbase = p.Vt + (long)b * p.vt_bs + (long)h * p.vt_hs;
    uint32_t dko[4], dvo[4];
    bool dk_real[4], dv_real[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = wave + j * NWV, row = i * 4 + (lane >> 4), cpos = lane & 15;
        const int ck = cpos ^ (row & 15), cv = ((((cpos >> 1) ^ (row & 7)) << 1) | (cpos & 1));
        dko[j] = (uint32_t)(((long)row * p.k_ss + ck * 8) * 2);
        dvo[j] = (uint32_t)(((long)row * p.vt_ds + cv * 8) * 2);
        dk_real[j] = ck * 8 < hd;
        dv_real[j] = cv * 8 < hd;
    }
    for (int t = tid; t < 2 * 64 * 2; t += 64 * NWV) {
        const int sl = t >> 7, row = (t & 127) >> 1, c = 10 + (t & 1);
        *(uint4*)(smem + sl * TILE + row * KROW + ((c ^ (row & 15)) << 4)) = make_uint4(0, 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // (the first barrier below orders these writes before every read)
    auto issue_k = [&](int kt) {
        if (kt >= 64) return;
        const uint32_t dst = lds_base + (kt & 1) * TILE;
        const elem_t* tk = kbase + (long)kt * KT * p.k_ss;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (dk_real[j]) glds16s(tk, dko[j], dst + (wave + j * NWV) * 1024);
    };
    auto issue_v = [&](int kt) {
        if (kt >= 64) return;
        const uint32_t dst = lds_base + (2 + (kt & 1)) * TILE;
        const elem_t* tv = vbase + (long)kt * KT * p.vt_ds;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (dv_real[j]) glds16s(tv, dvo[j], dst + (wave + j * NWV) * 1024);
    };
    // LDS fragment addresses, per lane and once: K fragment of k-step ks in rows fr, fr + 16, ... (the swizzle term of row 16 ns + fr is fr);
    // V fragment base of the transposing reads (see attn_reg_kernel)
    uint32_t kfo[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) kfo[ks] = fr * KROW + (((ks * 4 + fg) ^ fr) << 4);
    const int swr = 4 * (fg & 1) + (fr >> 2);
    const uint32_t vfo = 2 * TILE + (4 * fg + (fr >> 2)) * KROW + ((fr & 2) << 3) + ((fr & 1) << 3);

    f32x4_t oacc[NG][NDS];
    float m[NG], mn[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        m[g] = -INFINITY;
#pragma unroll
        for (int ds = 0; ds < NDS; ++ds) oacc[g][ds] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    // S tile kt on the matrix pipe: 4 x 3 K fragments, each into both groups' chains (24 MFMAs)
    auto qk = [&](int kt, f32x4_t (&acc)[NG][4]) {
        const char* tb = smem + (kt & 1) * TILE;
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g][ns] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const uint4 kf = *(const uint4*)(tb + ns * 16 * KROW + kfo[ks]);
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][ns] = mfma16(kf, qf[g][ks], acc[g][ns]);
            }
        }
    };
    // score epilogue of tile kt: rnd(rnd(rnd(acc) + rel_h) + rel_w) as 16-bit pairs sq[g][2 ns + half] (keys 16 ns + 4 fg + {0,1 | 2,3}), the
    // tile maximum folded into mn[g] = the row maximum including tile kt; returns whether some query of the wave saw a new maximum
    auto scores = [&](int kt, const f32x4_t (&acc)[NG][4], uint32_t (&sq)[NG][8]) -> bool {
        bool grew = false;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float rh = e2f(ghl[kt * (16 * NG) + g * 16 + fr]);
            float tm = -INFINITY;
#pragma unroll
            for (int ns = 0; ns < 4; ++ns)
                score_quad_win(acc[g][ns], rh, f32x2_t{rw[g][ns * 4], rw[g][ns * 4 + 1]}, f32x2_t{rw[g][ns * 4 + 2], rw[g][ns * 4 + 3]}, sq[g][ns * 2],
                               sq[g][ns * 2 + 1], tm);
            tm = rnd(tm);
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            mn[g] = fmaxf(m[g], tm);                           // finite from tile 0 on
            grew = grew || mn[g] > m[g];
        }
        return __builtin_amdgcn_ballot_w64(grew) != 0;
    };
