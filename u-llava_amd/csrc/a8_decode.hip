// W8A8 for batched decode steps on gfx950 (bf16 build only): e4m3 activations x e4m3 weights at M <= 32, streamed from the resident codes.
//
// ull_gemm_skinny_a8w8_bf16 is the skinny kernel of gemv.hip (skinny_gemm_kernel<SW, WF_FP8>) with the block-scaled matrix instruction in
// place of convert + 16x16x32 MFMA: a block of 8 waves owns 16 output features (SwiGLU: 16 gate + 16 up rows of the interleave), every
// wave one contiguous eighth of the 128-code K-tiles, and one v_mfma_scale_f32_16x16x128_f8f6f4 consumes 16 weight rows x 128 codes -- 32
// contiguous bytes per lane, straight from HBM into the first operand, no conversion.  Lane l holds row (l & 15) and the codes
// [32 (l >> 4), +32) of the K-tile for BOTH operands (the pairing tools/probes/mfma_scale_lane_map.hip measured; nothing else is relied
// on); the scale operands are the constant 127 (2^0), cbsz = blgp = 0 (e4m3 x e4m3).  The activation codes (M x K bytes, L2-resident) are
// loaded the same way; rows >= M repeat the last row and are never stored; M in 17 .. 32 is a second activation fragment and a second
// accumulator against the same weight fragment.  Partial sums go through LDS and are added in wave order, so the fp32 summation order of an
// output is a function of K alone: K-tiles [nkt w / 8, nkt (w + 1) / 8) ascending inside wave w, then waves 0 .. 7 ascending.
//
// ull_rmsnorm_quantize_rows_fp8_bf16 is ull_quantize_rows_fp8_bf16(ull_rmsnorm_bf16(x)) in one launch, bit for bit: the operations of
// rownorm_kernel<., 0> (norm.hip) and quantize_rows_fp8_kernel (gemv.hip) in their order, without the normed rows going to memory.
#include "ull_common.h"

namespace {

constexpr int EPI_RESID = ULL_EPI_RESID, EPI_SWIGLU = ULL_EPI_SWIGLU, EPI_OUT_F32 = ULL_EPI_OUT_F32;
constexpr int BK8 = 128;                               // codes per K-tile: one matrix instruction
constexpr int MAXM8 = 32;

using i32x8_t = __attribute__((ext_vector_type(8))) int;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// the weight stream is read once, by one CU: non-temporal, as the GEMV's (gemv.hip w_load16)
ULL_DEV uint4 nt_load16(const uint8_t* p) {
    const u32x4_t v = __builtin_nontemporal_load((const u32x4_t*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
ULL_DEV i32x8_t frag32(const uint4& lo, const uint4& hi) {
    return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

struct A8SkinnyArgs {
    const uint8_t* Xq; const uint8_t* Wq;              // codes [M, ldxq], [N, ldq]
    const float* xs; const float* ws;                  // 2^t_m [M], 2^s_n [N]
    void* C; const elem_t* R;
    long ldxq, ldq, ldc, ldr;
    int M, N, K, flags, n_out;
};

// SW: SwiGLU on the gate|up interleave; MF: activation fragments of 16 rows (1: M <= 16, 2: M <= 32)
template <bool SW, int MF>
__global__ __launch_bounds__(512) void skinny_a8w8_kernel(A8SkinnyArgs p) {
    __shared__ f32x4_t part[SW ? 2 : 1][MF][8][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 15, fg = lane >> 4;
    const int o0 = blockIdx.x * 16;                              // first output feature of the block
    // weight row of first-operand row fr: plain: o0 + fr (past N: the last row, never stored); SwiGLU pack: gate rows (o0/16)*32 + fr, up rows 16 below
    const int wr0 = SW ? (o0 >> 4) * 32 + fr : min(o0 + fr, p.N - 1);
    const uint8_t* w0 = p.Wq + (long)wr0 * p.ldq + fg * 32;
    const uint8_t* w1 = w0 + 16 * p.ldq;
    const uint8_t* xr[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) xr[f] = p.Xq + (long)min(fr + 16 * f, p.M - 1) * p.ldxq + fg * 32;   // rows >= M repeat the last row
    const int nkt = p.K / BK8;
    const int kt0 = (int)((long)nkt * wave / 8), kt1 = (int)((long)nkt * (wave + 1) / 8);
    f32x4_t a0[MF], a1[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) a0[f] = a1[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                               // K-tiles per batch: all of a batch's loads are issued before its first MFMA
    for (int k0 = kt0; k0 < kt1; k0 += U) {
        uint4 wq[U][2], uq[U][2], xq[U][MF][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long ko = (long)min(k0 + u, kt1 - 1) * BK8;    // past the end: a repeated, unused fragment
            wq[u][0] = nt_load16(w0 + ko);
            wq[u][1] = nt_load16(w0 + ko + 16);
            if constexpr (SW) {
                uq[u][0] = nt_load16(w1 + ko);
                uq[u][1] = nt_load16(w1 + ko + 16);
            }
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                xq[u][f][0] = *(const uint4*)(xr[f] + ko);
                xq[u][f][1] = *(const uint4*)(xr[f] + ko + 16);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < kt1) {
                const i32x8_t wf = frag32(wq[u][0], wq[u][1]);
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const i32x8_t xf = frag32(xq[u][f][0], xq[u][f][1]);
                    // cbsz = blgp = 0: e4m3 A and B; scale bytes 127 = 2^0
                    a0[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, xf, a0[f], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
                    if constexpr (SW)
                        a1[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag32(uq[u][0], uq[u][1]), xf, a1[f], 0, 0, 0, 0x7f7f7f7f, 0,
                                                                                 0x7f7f7f7f);
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
    f32x4_t s0 = part[0][f][0][lane], s1 = s0;
    if constexpr (SW) s1 = part[1][f][0][lane];
#pragma unroll
    for (int w = 1; w < 8; ++w) {
        s0 += part[0][f][w][lane];
        if constexpr (SW) s1 += part[1][f][w][lane];
    }
    // s0[r] = sum_k xq[m, k] * wq[o, k] for m = 16 f + fr, o = o0 + 4 fg + r: times 2^(t_m + s_n), one exact ldexp
    const int m = 16 * f + fr;
    if (m >= p.M) return;
    const int ex = ilogbf(p.xs[m]);
    float t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + fg * 4 + r;
        float v;
        if constexpr (SW) {
            const int wr = (o0 >> 4) * 32 + fg * 4 + r;
            const float g = ldexpf(s0[r], ilogbf(p.ws[wr]) + ex), u = ldexpf(s1[r], ilogbf(p.ws[wr + 16]) + ex);
            v = rnd(rnd(act_silu(rnd(g))) * rnd(u));
        } else {
            v = ldexpf(s0[r], ilogbf(p.ws[min(o, p.N - 1)]) + ex);
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
// groups of narrower rows add the same terms: the lanes past the row hold zeros here) -- and walks them three times (the row stays in the
// L1): sum of squares, amax of the normed row, codes.
__global__ __launch_bounds__(64) void rmsnorm_quantize_rows_fp8_kernel(const elem_t* __restrict__ X, long ldx, const elem_t* __restrict__ W, float eps,
                                                                        int K, uint8_t* __restrict__ codes, long ldq, float* __restrict__ scales) {
    const int lane = threadIdx.x;
    const long row = blockIdx.x;
    const elem_t* x = X + row * ldx;
    const int nchunk = K >> 3;
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
    // the normed row as ull_rmsnorm_bf16 stores it: bf16(w * bf16(x * rstd))
    auto normed = [&](int c, float* o) {
        float v[8], wv[8];
        unpack8(*(const uint4*)(x + c * 8), v);
        unpack8(*(const uint4*)(W + c * 8), wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rnd(wv[j] * rnd(v[j] * rstd));
    };
    float amax = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
        float o[8];
        normed(c, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(o[j]));
    }
    amax = wave_max(amax);
    const int s = fp8_scale_exp(amax);
    if (lane == 0) scales[row] = ldexpf(1.f, s);
    uint8_t* q = codes + row * ldq;
    for (int c = lane; c < nchunk; c += 64) {
        float o[8];
        normed(c, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = ldexpf(o[j], -s);     // exact; |o| <= 448: the conversion cannot overflow
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(o[0], o[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(o[2], o[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(o[4], o[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(o[6], o[7], hi, true);
        *(uint2*)(q + c * 8) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
}

}  // namespace

// W8A8 Linear at 1 <= M <= 32 (batched decode steps): ull_gemm_a8w8_bf16's operands and flags, the skinny kernel's shape and epilogue
// (include/ullava_hip.h).  Everything is checked before any launch.
extern "C" int ull_gemm_skinny_a8w8_bf16(const void* Xq, int64_t ldxq, const void* x_scales, const void* Q, int64_t ldq, const void* w_scales, void* C,
                                         int64_t ldc, const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    if (!Xq || !x_scales || !Q || !w_scales || !C || M <= 0 || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if (const int rc = ull_a8_epilogue_check(flags, R, N, ldc, ldr)) return rc;
    if (M > MAXM8 || K % BK8 != 0 || (ldxq & 15) || (ldq & 15) || ldxq < K || ldq < K || (((uintptr_t)Xq | (uintptr_t)Q) & 15)) return ULL_ERR_SHAPE;
    if (N > (1 << 30) || K > (1 << 30)) return ULL_ERR_SHAPE;
    const int64_t n_out = (flags & EPI_SWIGLU) ? N / 2 : N;
    const A8SkinnyArgs a{(const uint8_t*)Xq, (const uint8_t*)Q, (const float*)x_scales, (const float*)w_scales, C, (const elem_t*)R,
                         (long)ldxq, (long)ldq, (long)ldc, (long)ldr, (int)M, (int)N, (int)K, flags, (int)n_out};
    const dim3 grid((unsigned)((n_out + 15) / 16));
    hipStream_t st = (hipStream_t)stream;
    if (flags & EPI_SWIGLU) {
        if (M <= 16) hipLaunchKernelGGL((skinny_a8w8_kernel<true, 1>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((skinny_a8w8_kernel<true, 2>), grid, dim3(512), 0, st, a);
    } else {
        if (M <= 16) hipLaunchKernelGGL((skinny_a8w8_kernel<false, 1>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((skinny_a8w8_kernel<false, 2>), grid, dim3(512), 0, st, a);
    }
    return ull_check_launch();
}

// codes, scales = ull_quantize_rows_fp8_bf16(ull_rmsnorm_bf16(X; rms_w, eps)) without the normed rows: X [M, K] bf16 (row pitch ldx), codes
// [M, K] (row pitch ldq bytes), scales fp32 [M].  Any M; K % 8 == 0.
extern "C" int ull_rmsnorm_quantize_rows_fp8_bf16(const void* X, int64_t ldx, const void* rms_w, float eps, int64_t M, int64_t K, void* codes,
                                                  int64_t ldq, void* scales, void* stream) {
    if (!X || !rms_w || !codes || !scales || M <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 7) || (ldx & 7) || ldx < K || (ldq & 7) || ldq < K || M > (1 << 30) || K > (1 << 30) ||
        (((uintptr_t)X | (uintptr_t)rms_w) & 15) || ((uintptr_t)codes & 7))
        return ULL_ERR_SHAPE;
    hipLaunchKernelGGL(rmsnorm_quantize_rows_fp8_kernel, dim3((unsigned)M), dim3(64), 0, (hipStream_t)stream, (const elem_t*)X, (long)ldx,
                       (const elem_t*)rms_w, eps, (int)K, (uint8_t*)codes, (long)ldq, (float*)scales);
    return ull_check_launch();
}
