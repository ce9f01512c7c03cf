// W4A8 for batched decode steps on gfx950 (bf16 build only): MXFP8 activations x resident MXFP4 weights at M <= 32, streamed from the resident
// codes and scale bytes.
//
// ull_gemm_skinny_w4a8_bf16 is skinny_a8w8_kernel (a8_decode.hip) with the operands of gemm128_w4a8_kernel (gemm.hip): a block of 8 waves owns
// 16 output features (SwiGLU: 16 gate + 16 up rows of the interleave), the waves split K, and one v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = 4:
// e2m1 first operand, blgp = 0: e4m3 second operand) consumes 16 weight rows x 128 codes with both E8M0 scales applied by the instruction, so
// nothing is left to the epilogue but the rounding points.  The operand lane maps are gemm128_w4a8_kernel's (measured:
// tools/probes/mfma_scale_lane_map.hip, tools/probes/mfma_scale_w4a8_lane_map.hip; nothing else is relied on): lane l = (row fr = l & 15, group
// fg = l >> 4) feeds the 32 e2m1 codes of block fg of the K-tile in the first four registers of the first operand, the e4m3 codes
// k = 64 (byte >> 4) + 16 fg + (byte & 15) in the second, and the scale byte of (row, block fg) of either operand.
// The resident layout is what makes the weight streamable: for super tile (b, t) of whole superblock b (2048 elements) the lane's fragments of
// the four K-tiles at element b * 2048 + g * 512 + t * 128, g = 0 .. 3, are the 64 contiguous row bytes at b * 1024 + (16 t + 4 fg) * 16 --
// component g of each 16-byte piece is tile g's -- and their four scale bytes are the aligned dword at scale byte b * 64 + (4 t + fg) * 4, picked
// by the instruction's byte select; the activation scale row (ull_quantize_rows_mxfp8_bf16's order) holds the same dword.  K-tiles after the
// last whole superblock are in standard order: 16 code bytes at kt * 64 + fg * 16, scale byte kt * 4 + fg.  The activation codes (M x K bytes,
// L2-resident) are in standard K order; rows >= M repeat the last row and are never stored; M in 17 .. 32 is a second activation fragment and
// a second accumulator against the same weight fragment.
//
// Summation order: a function of K alone (never of M, N, the row or the grid).  The UNITS are the super tiles (b, t) in ull_gemm_w4a8_bf16's
// visit order (b, then t ascending), then the tail K-tiles ascending; inside a super tile g = 0 .. 3 ascending, one matrix instruction per
// K-tile, from zero.  With nkt = K / 128 K-tiles, unit u starts at K-tile position p(u) = 4 u (a super tile) or 4 nsup + (u - nsup) (a tail
// tile); wave w (w = 0 .. 7) takes the units with nkt w / 8 <= p(u) < nkt (w + 1) / 8 (integer division), i.e. contiguous runs of units of about
// equal K-tile count (K = 4096: one super tile per wave; K = 11008, 20 super tiles + 6 tail tiles: 3, 3, 2, 3, 3, 2, 3 super tiles and
// 1 super tile + 6 tail tiles), a wave without a unit contributes exact zeros, and the eight partial sums are added w = 0 .. 7 ascending.
//
// ull_rmsnorm_quantize_rows_mxfp8_bf16 is ull_quantize_rows_mxfp8_bf16(ull_rmsnorm_bf16(x)) in one launch, bit for bit: the operations of
// rownorm_kernel<., 0> (norm.hip) and quantize_rows_mxfp8_kernel (gemm.hip) in their order, without the normed rows going to memory.
#include <type_traits>

#include "ull_common.h"

namespace {

constexpr int EPI_RESID = ULL_EPI_RESID, EPI_SWIGLU = ULL_EPI_SWIGLU, EPI_OUT_F32 = ULL_EPI_OUT_F32;
constexpr int BK8 = ULL_A8W8_BK;                       // codes per K-tile: one matrix instruction
constexpr int MAXM = ULL_W4A8_SKINNY_MAX_M;

using i32x8_t = __attribute__((ext_vector_type(8))) int;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// the weight stream is read once, by one CU: non-temporal, as the GEMV's (gemv.hip w_load16)
ULL_DEV u32x4_t nt_load16(const uint8_t* p) { return __builtin_nontemporal_load((const u32x4_t*)p); }
ULL_DEV i32x8_t xfrag(const uint8_t* p) {              // the e4m3 operand of one K-tile: the 16-byte chunks fg and 4 + fg (p points at chunk fg)
    const uint4 lo = *(const uint4*)p, hi = *(const uint4*)(p + 64);
    return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

struct W4A8SkinnyArgs {
    const uint8_t* Xq; const uint8_t* xs;              // e4m3 codes [M, ldxq], E8M0 bytes [M, ldxs] (mx_scale_pos order)
    const uint8_t* Wq; const uint8_t* ws;              // resident e2m1 codes [N, ldq], E8M0 bytes [N, lds]
    void* C; const elem_t* R;
    long ldxq, ldxs, ldq, lds, ldc, ldr;
    int M, N, K, flags, n_out;
};

// first unit of wave w: the number of units that start before K-tile position nkt * w / 8
ULL_DEV int first_unit(int w, int nkt, int nsup) {
    const int T = (int)((long)nkt * w / 8);
    return T <= 4 * nsup ? (T + 3) >> 2 : nsup + (T - 4 * nsup);
}

// SW: SwiGLU on the gate|up interleave; MF: activation fragments of 16 rows (1: M <= 16, 2: M <= 32)
template <bool SW, int MF>
__global__ __launch_bounds__(512) void skinny_w4a8_kernel(W4A8SkinnyArgs p) {
    __shared__ f32x4_t part[SW ? 2 : 1][MF][8][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 15, fg = lane >> 4;
    const int o0 = blockIdx.x * 16;                              // first output feature of the block
    // weight row of first-operand row fr: plain: o0 + fr (past N: the last row, never stored); SwiGLU pack: gate rows (o0/16)*32 + fr, up rows 16 below
    const int wr0 = SW ? (o0 >> 4) * 32 + fr : min(o0 + fr, p.N - 1);
    const uint8_t* w0 = p.Wq + (long)wr0 * p.ldq;
    const uint8_t* w1 = w0 + 16 * p.ldq;
    const uint8_t* s0 = p.ws + (long)wr0 * p.lds;
    const uint8_t* s1 = s0 + 16 * p.lds;
    const uint8_t* xr[MF];
    const uint8_t* xsr[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) {                               // rows >= M repeat the last row
        const long m = min(fr + 16 * f, p.M - 1);
        xr[f] = p.Xq + m * p.ldxq + fg * 16;
        xsr[f] = p.xs + m * p.ldxs;
    }
    const int nkt = p.K / BK8, nsup = (p.K >> 11) * 4;
    const int u0 = first_unit(wave, nkt, nsup), u1 = first_unit(wave + 1, nkt, nsup);
    f32x4_t a0[MF], a1[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) a0[f] = a1[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // ---- the wave's super tiles: 64 contiguous weight bytes and one scale dword per lane and row, requested one unit ahead ----
    const int se = min(u1, nsup);
    u32x4_t wq[4], uq[4];
    uint32_t wsc = 0, usc = 0;
    auto load_w = [&](int u, u32x4_t (&a)[4], u32x4_t (&b)[4], uint32_t& sa, uint32_t& sb) {
        const long wo = (long)(u >> 2) * 1024 + ((u & 3) * 16 + fg * 4) * 16, so = (long)(u >> 2) * 64 + ((u & 3) * 4 + fg) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = nt_load16(w0 + wo + c * 16);
            if constexpr (SW) b[c] = nt_load16(w1 + wo + c * 16);
        }
        sa = *(const uint32_t*)(s0 + so);
        if constexpr (SW) sb = *(const uint32_t*)(s1 + so);
    };
    if (u0 < se) load_w(u0, wq, uq, wsc, usc);
    for (int u = u0; u < se; ++u) {
        u32x4_t wn[4], un[4];
        uint32_t wsn = 0, usn = 0;
        if (u + 1 < se) load_w(u + 1, wn, un, wsn, usn);         // wave-uniform
        const long so = (long)(u >> 2) * 64 + ((u & 3) * 4 + fg) * 4;
        uint32_t xsc[MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) xsc[f] = *(const uint32_t*)(xsr[f] + so);
        const int kt0 = (u >> 2) * 16 + (u & 3);                 // K-tile of step g: b * 16 + g * 4 + t
        auto step = [&](auto G) {
            constexpr int g = decltype(G)::value;
            const long ko = (long)(kt0 + g * 4) * BK8;
            const i32x8_t wf{(int)wq[0][g], (int)wq[1][g], (int)wq[2][g], (int)wq[3][g], 0, 0, 0, 0};
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const i32x8_t xf = xfrag(xr[f] + ko);
                // cbsz = 4: e2m1 A; blgp = 0: e4m3 B; scale byte g of both registers
                a0[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, xf, a0[f], 4, 0, g, (int)wsc, g, (int)xsc[f]);
                if constexpr (SW) {
                    const i32x8_t uf{(int)uq[0][g], (int)uq[1][g], (int)uq[2][g], (int)uq[3][g], 0, 0, 0, 0};
                    a1[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(uf, xf, a1[f], 4, 0, g, (int)usc, g, (int)xsc[f]);
                }
            }
        };
        step(std::integral_constant<int, 0>{});
        step(std::integral_constant<int, 1>{});
        step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{});
        if (u + 1 < se) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { wq[c] = wn[c]; uq[c] = un[c]; }
            wsc = wsn; usc = usn;
        }
    }

    // ---- the wave's tail K-tiles (standard order): 16 weight bytes and one scale byte per lane and row ----
    const int kt_end = 4 * nsup + (u1 - nsup);                   // (only read when the wave has tail tiles: u1 > nsup)
    constexpr int U = 4;                                         // K-tiles per batch: all of a batch's loads are issued before its first MFMA
    for (int k0 = 4 * nsup + (max(u0, nsup) - nsup); u1 > nsup && k0 < kt_end; k0 += U) {
        u32x4_t tw[U], tu[U];
        uint32_t tws[U], tus[U], txs[U][MF];
        i32x8_t tx[U][MF];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int kt = min(k0 + i, kt_end - 1);              // past the end: a repeated, unused fragment
            tw[i] = nt_load16(w0 + (long)kt * 64 + fg * 16);
            tws[i] = s0[kt * 4 + fg];
            if constexpr (SW) {
                tu[i] = nt_load16(w1 + (long)kt * 64 + fg * 16);
                tus[i] = s1[kt * 4 + fg];
            }
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                tx[i][f] = xfrag(xr[f] + (long)kt * BK8);
                txs[i][f] = xsr[f][kt * 4 + fg];
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (k0 + i < kt_end) {
                const i32x8_t wf{(int)tw[i][0], (int)tw[i][1], (int)tw[i][2], (int)tw[i][3], 0, 0, 0, 0};
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    a0[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, tx[i][f], a0[f], 4, 0, 0, (int)tws[i], 0, (int)txs[i][f]);
                    if constexpr (SW) {
                        const i32x8_t uf{(int)tu[i][0], (int)tu[i][1], (int)tu[i][2], (int)tu[i][3], 0, 0, 0, 0};
                        a1[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(uf, tx[i][f], a1[f], 4, 0, 0, (int)tus[i], 0, (int)txs[i][f]);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int f = 0; f < MF; ++f) {
        part[0][f][wave][lane] = a0[f];
        if constexpr (SW) part[1][f][wave][lane] = a1[f];
    }
    __syncthreads();
    if (wave >= MF) return;
    // wave f finishes activation fragment f: the partial sums in wave order (from wave 0's, whichever wave adds them)
    const int f = wave;
    f32x4_t y0 = part[0][f][0][lane], y1 = y0;
    if constexpr (SW) y1 = part[1][f][0][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) {
        y0 += part[0][f][w][lane];
        if constexpr (SW) y1 += part[1][f][w][lane];
    }
    // y0[r] = y[m, o] for m = 16 f + fr, o = o0 + 4 fg + r, both scales applied by the instruction
    const int m = 16 * f + fr;
    if (m >= p.M) return;
    float t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + fg * 4 + r;
        float v;
        if constexpr (SW) {
            v = rnd(rnd(act_silu(rnd(y0[r]))) * rnd(y1[r]));
        } else {
            v = y0[r];
            if (!(p.flags & EPI_OUT_F32) || (p.flags & EPI_RESID)) v = rnd(v);
        }
        if ((p.flags & EPI_RESID) && o < p.n_out) v = rnd(e2f(p.R[(long)m * p.ldr + o]) + v);
        t[r] = v;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + fg * 4 + r;
        if (o < p.n_out) {
            if (p.flags & EPI_OUT_F32) ((float*)p.C)[(long)m * p.ldc + o] = t[r];
            else ((elem_t*)p.C)[(long)m * p.ldc + o] = f2e(t[r]);
        }
    }
}

// One row per block of one wave.  Lane l owns the 8-element chunks l, l + 64, ... -- rownorm_kernel's assignment for a row (its sub-wave
// groups of narrower rows add the same terms: the lanes past the row hold zeros here).  First walk: the sum of squares; second walk (the row
// stays in the L1): the normed chunk, then quantize_rows_mxfp8_kernel's steps on it -- the four lanes of a 32-block share its amax through two
// xor-shuffles, each lane writes its 8 codes, the first of the four the scale byte.
__global__ __launch_bounds__(64) void rmsnorm_quantize_rows_mxfp8_kernel(const elem_t* __restrict__ X, long ldx, const elem_t* __restrict__ W, float eps,
                                                                          int K, uint8_t* __restrict__ codes, long ldq, uint8_t* __restrict__ scales,
                                                                          long lds) {
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    const elem_t* x = X + row * ldx;
    const int nchunk = K >> 3, nsb = K >> 11;
    float s2 = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
        float v[8];
        unpack8(*(const uint4*)(x + c * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s2 += v[j] * v[j];
    }
    const float invD = 1.0f / (float)K;
    s2 = group_sum(s2, 64);
    const float rstd = rsqrtf(s2 * invD + eps);
    uint8_t* q = codes + row * ldq;
    uint8_t* sc = scales + row * lds;
    for (int c0 = 0; c0 < nchunk; c0 += 64) {              // K % 32 == 0: the four lanes of a block are in or out together
        const int c = c0 + lane;
        const bool on = c < nchunk;
        float v[8], wv[8];
        unpack8(on ? *(const uint4*)(x + c * 8) : make_uint4(0, 0, 0, 0), v);
        unpack8(on ? *(const uint4*)(W + c * 8) : make_uint4(0, 0, 0, 0), wv);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = rnd(wv[j] * rnd(v[j] * rstd));          // the normed row as ull_rmsnorm_bf16 stores it: bf16(w * bf16(x * rstd))
            amax = fmaxf(amax, fabsf(v[j]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        if (!on) continue;
        const int t = min(max(fp8_scale_exp(amax), -127), 127);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ldexpf(v[j], -t);     // exact; |v| <= 448: the conversion cannot overflow
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
        *(uint2*)(q + c * 8) = make_uint2((uint32_t)lo, (uint32_t)hi);
        if ((c & 3) == 0) sc[mx_scale_pos(c >> 2, nsb)] = (uint8_t)(t + 127);
    }
}

}  // namespace

// W4A8 Linear at 1 <= M <= 32 (batched decode steps): ull_gemm_w4a8_bf16's operands and flags, the skinny kernel's shape and epilogue
// (include/ullava_hip.h).  Everything is checked before any launch.
extern "C" int ull_gemm_skinny_w4a8_bf16(const void* Xq, int64_t ldxq, const void* x_scales, int64_t ldxs, const void* Q, int64_t ldq,
                                         const void* w_scales, int64_t lds, void* C, int64_t ldc, const void* R, int64_t ldr, int64_t M, int64_t N,
                                         int64_t K, int flags, void* stream) {
    if (!Xq || !x_scales || !Q || !w_scales || !C || M <= 0 || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if (const int rc = ull_a8_epilogue_check(flags, R, N, ldc, ldr)) return rc;
    if (M > MAXM || N > (1 << 30) || K > (1 << 30)) return ULL_ERR_SHAPE;
    if (K % BK8 != 0 || (ldxq & 15) || (ldq & 15) || ldxq < K || ldq < K / 2 || (((uintptr_t)Xq | (uintptr_t)Q) & 15)) return ULL_ERR_SHAPE;   // 16-byte pieces
    if ((ldxs & 3) || (lds & 3) || ldxs < K / 32 || lds < K / 32 || (((uintptr_t)x_scales | (uintptr_t)w_scales) & 3)) return ULL_ERR_SHAPE;   // 4-byte scale loads
    const int64_t n_out = (flags & EPI_SWIGLU) ? N / 2 : N;
    const W4A8SkinnyArgs a{(const uint8_t*)Xq, (const uint8_t*)x_scales, (const uint8_t*)Q, (const uint8_t*)w_scales, C, (const elem_t*)R,
                           (long)ldxq, (long)ldxs, (long)ldq, (long)lds, (long)ldc, (long)ldr, (int)M, (int)N, (int)K, flags, (int)n_out};
    const dim3 grid((unsigned)((n_out + 15) / 16));
    hipStream_t st = (hipStream_t)stream;
    if (flags & EPI_SWIGLU) {
        if (M <= 16) hipLaunchKernelGGL((skinny_w4a8_kernel<true, 1>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((skinny_w4a8_kernel<true, 2>), grid, dim3(512), 0, st, a);
    } else {
        if (M <= 16) hipLaunchKernelGGL((skinny_w4a8_kernel<false, 1>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((skinny_w4a8_kernel<false, 2>), grid, dim3(512), 0, st, a);
    }
    return ull_check_launch();
}

// codes, scales = ull_quantize_rows_mxfp8_bf16(ull_rmsnorm_bf16(X; rms_w, eps)) without the normed rows: X [M, K] bf16 (row pitch ldx), codes
// [M, K] (row pitch ldq bytes), scale bytes [M, lds] in the W4A8 pair's order.  Any M; K % 32 == 0.
extern "C" int ull_rmsnorm_quantize_rows_mxfp8_bf16(const void* X, int64_t ldx, const void* rms_w, float eps, int64_t M, int64_t K, void* codes,
                                                    int64_t ldq, void* scales, int64_t lds, void* stream) {
    if (!X || !rms_w || !codes || !scales || M <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 31) || (ldx & 7) || ldx < K || (ldq & 7) || ldq < K || lds < K / 32 || (lds & 3) || M > (1 << 30) || K > (1 << 30) ||
        (((uintptr_t)X | (uintptr_t)rms_w) & 15) || ((uintptr_t)codes & 7) || ((uintptr_t)scales & 3))
        return ULL_ERR_SHAPE;
    hipLaunchKernelGGL(rmsnorm_quantize_rows_mxfp8_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, (const elem_t*)X, (long)ldx,
                       (const elem_t*)rms_w, eps, (int)K, (uint8_t*)codes, (long)ldq, (uint8_t*)scales, (long)lds);
    return ull_check_launch();
}
