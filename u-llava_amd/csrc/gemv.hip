// Decode-shape Linear for gfx950: C[M,N] = epilogue(X[M,K] * W[N,K]^T) with M <= 4 (token-by-token generation).
//
// reference: the same nn.Linear modules as gemm_bf16.hip, reached from `generate()` steps after the prefill
// (models/ullava_core.py:357-395 prepare_inputs_for_generation keeps only the last token when a KV cache exists).
//
// At M <= 4 the op is a pure weight stream (LLaMA-7B: 13.5 GB per token), so there is no LDS staging and no MFMA: one wave
// owns one output feature at a time, its 64 lanes stream that weight row with 16-byte loads (1 KiB per wave-instruction,
// read exactly once), X comes from L1/L2, fp32 accumulation, wave reduction, same epilogues/rounding points as the GEMM.
#include <type_traits>

#include "linear_route.h"
#include "ull_common.h"

namespace {

// short names for the header's ULL_EPI_* (the activation field's shift and mask have no name there)
constexpr int EPI_BIAS = ULL_EPI_BIAS, EPI_ACT_SHIFT = 1, EPI_ACT_MASK = 3 << 1, EPI_RESID = ULL_EPI_RESID, EPI_SWIGLU = ULL_EPI_SWIGLU,
              EPI_OUT_F32 = ULL_EPI_OUT_F32;
constexpr int EPI_BIAS_ROUNDED = ULL_EPI_BIAS_ROUNDED;     // bias added to the already rounded product (at::linear's unfused matmul + add_ path)
constexpr int EPI_ROPE_APPEND = 1 << 20;  // (internal) q|k|v projection of a decode step: RoPE + KV-cache append in the epilogue, see RopeAppend
constexpr int MAXM = 4;

// Decode-step q|k|v projection (hf LlamaAttention.forward: q/k/v_proj, apply_rotary_pos_emb, cache update) in ONE launch: a wave owns the
// output pair (i, i + hd/2) of one head -- the two elements a rotation mixes -- so after the dot products
//   q: both rotated elements go to the query buffer;  k: to row `past + s` of the K cache;  v (no rotation): to its V^T cache columns,
// with exactly the operations of rope_append_kernel on the rounded projection outputs (same bits), from the cos / sin table of the
// step's positions (rope_table: one launch per step instead of 32 x 16 lanes evaluating sinf / cosf per layer).
struct RopeAppend {
    const elem_t* cs; const elem_t* sn;      // [tokens][hd / 2], 16-bit rounded
    elem_t* kc; elem_t* vtc;                 // K cache [B, H, smax, hd]; V^T cache [B, H, hd, smax] (32-key permutation of transpose_v_kernel)
    int S, H, hd, smax, past;
};

typedef uint32_t gv_u32x4_t __attribute__((ext_vector_type(4)));
// The weight stream is read exactly once per token, by exactly one CU: non-temporal loads (global_load_dwordx4 ... nt; MI355X_MICROARCH.md
// "nt-weights") keep it from evicting X and the KV cache from the L2.  Measured (tools/gemv_bw.py, tools/decode_bench.py): 1-GB stream
// 5.82 -> 6.29 TB/s, decode step 3.77 -> 3.61 ms.  (Software-pipelining the batches of a wave across output rows was also tried: 168
// registers, 3 waves per SIMD instead of 4, 3.85 TB/s on the q|k|v shape against 4.9 -- not shipped.  Requesting the wave's first weight
// batch before the activations are staged -- the weights do not depend on them -- was tried in two forms in the decode loop: held in the
// real buffers across the staging code (151 registers, the fourth wave per SIMD gone: 3.79 vs 3.38 ms per token) and as loads into one
// scratch register quad that only warm the L2 (3.40 vs 3.37): neither shipped; the launch's first memory round trip is not what a
// 20-us GEMV loses against the 1-GB stream rate.)
ULL_DEV uint4 w_load16(const elem_t* p) {
    const gv_u32x4_t v = __builtin_nontemporal_load((const gv_u32x4_t*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// Weight formats of the decode kernels.  WF_ELEM: 16-bit rows (the model dtype).  WF_FP8 (bf16 build only): e4m3 code rows plus one fp32
// power-of-two scale per row (ull_quantize_rows_fp8_bf16); a lane turns 8 codes into the 8 floats float(q) * 2^s -- exactly the bf16
// values of the dequantized weight -- and feeds them to the same FMAs / MFMAs in the same order, so the result equals the 16-bit
// kernel's on dequant(W) bit for bit.  The format is a template parameter: for WF_ELEM the pointer type below is the plain weight pointer,
// so the existing instantiations keep their arguments and code.
// WF_MXFP4 (bf16 build only): e2m1 code rows with one E8M0 scale per 32 elements, in the resident layout of ull_common.h (mx_code_pos): a lane's four
// chunks of a superblock arrive in one 16-byte load, their four scale bytes in one 4-byte load, and v_cvt_scalef32_pk_f32_fp4 turns each chunk
// into the 8 floats e2m1 * 2^s -- again exactly the bf16 values of the dequantized weight, multiplied in the order of the 16-bit kernel.
constexpr int WF_ELEM = ULL_WF_ELEM, WF_FP8 = ULL_WF_FP8, WF_MXFP4 = ULL_WF_MXFP4;

struct W8Rows {
    const uint8_t* codes;                    // [N][ldw] e4m3fn bytes
    const float* scales;                     // [N] 2^s
};
template <int WF> struct WFmt {
    typedef const elem_t* __restrict__ ptr_t;
    typedef elem_t w_t;
    ULL_DEV static const elem_t* rows(ptr_t W) { return W; }
};
template <> struct WFmt<WF_FP8> {
    typedef W8Rows ptr_t;
    typedef uint8_t w_t;
    ULL_DEV static const uint8_t* rows(const W8Rows& W) { return W.codes; }
};

struct W4Rows {
    const uint8_t* codes;                    // [N][ldw] bytes: two e2m1 codes each, resident layout
    const uint8_t* scales;                   // [N][lds] E8M0 bytes, resident layout
    long lds;
};
template <> struct WFmt<WF_MXFP4> {
    typedef W4Rows ptr_t;
    typedef uint8_t w_t;
    ULL_DEV static const uint8_t* rows(const W4Rows& W) { return W.codes; }
};

typedef uint32_t gv_u32x2_t __attribute__((ext_vector_type(2)));
ULL_DEV uint2 w_load8(const uint8_t* p) {
    const gv_u32x2_t v = __builtin_nontemporal_load((const gv_u32x2_t*)p);
    return make_uint2(v.x, v.y);
}

// (unpack8_w8, fp8_scale_exp, unpack8_w4, mx_code_pos, mx_scale_pos: ull_common.h)

// One weight chunk (8 elements) of a GEMV lane against the M activation rows: the FMAs of gemv_kernel's 16-bit loop, in its order.
template <int M>
ULL_DEV void gemv_fma_chunk(const float* wv, const float* uv, bool swiglu, const elem_t* __restrict__ X, long ldx, const elem_t* xs, int K, int staged,
                            int c, float* a0, float* a1) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        float xv[8];
        if (staged) unpack8(*(const uint4*)(xs + (long)m * K + c * 8), xv);
        else unpack8(*(const uint4*)(X + (long)m * ldx + c * 8), xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            a0[m] += wv[j] * xv[j];
            if (swiglu) a1[m] += uv[j] * xv[j];
        }
    }
}

// X (optionally RMS-normalised) is staged in LDS when its M * K * 2 bytes fit ull_route::GEMV_STAGE_BYTES (ull_route::gemv_stages, which the
// routing rule reads too: a Linear whose RMSNorm does not fit here gets it as a launch of its own).
// X staged in LDS (`staged`): every block first copies -- or, with norm_w, RMS-normalises (transformers LlamaRMSNorm:
// w * bf16(x * rsqrt(mean(x^2) + eps)), the op that precedes the q/k/v and gate/up projections) -- the M activation rows,
// which removes one tiny latency-bound kernel per projection from the decode step.  The weight stream keeps U 16-byte loads
// per lane in flight (U KiB per wave); WF_FP8: U 8-byte loads of 8 codes, the same 8 elements per lane and chunk as the 16-byte form.
template <int M, int U, int WF = WF_ELEM>
__global__ __launch_bounds__(256) void gemv_kernel(const elem_t* __restrict__ X, long ldx, typename WFmt<WF>::ptr_t W, long ldw, void* C,
                                                   long ldc, const elem_t* __restrict__ bias, const elem_t* __restrict__ R, long ldr, int N, int K,
                                                   int flags, int n_out, const elem_t* __restrict__ norm_w, float eps, int staged, RopeAppend ra) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    elem_t* xs = (elem_t*)smem;                                   // [M][K] when staged
    __shared__ float red[4][MAXM];
    const int lane = threadIdx.x & 63, wv_id = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wv_id;                        // global wave id
    const int nwaves = gridDim.x * 4;
    const bool rope = flags & EPI_ROPE_APPEND;
    const bool swiglu = (flags & EPI_SWIGLU) || rope;             // two weight rows per output unit
    const int act = (flags & EPI_ACT_MASK) >> EPI_ACT_SHIFT;
    const int nchunk = K >> 3;
    if (staged) {
        float rstd[M];
#pragma unroll
        for (int m = 0; m < M; ++m) rstd[m] = 1.f;
        if (norm_w != nullptr) {
            float ss[M];
#pragma unroll
            for (int m = 0; m < M; ++m) ss[m] = 0.f;
            for (int c = threadIdx.x; c < nchunk; c += 256) {
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    float xv[8];
                    unpack8(*(const uint4*)(X + (long)m * ldx + c * 8), xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) ss[m] += xv[j] * xv[j];
                }
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
                ss[m] = wave_sum(ss[m]);
                if (lane == 0) red[wv_id][m] = ss[m];
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < M; ++m) rstd[m] = rsqrtf((red[0][m] + red[1][m] + red[2][m] + red[3][m]) / (float)K + eps);
        }
        for (int c = threadIdx.x; c < nchunk; c += 256) {
            float wn[8];
            if (norm_w != nullptr) unpack8(*(const uint4*)(norm_w + c * 8), wn);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                uint4 raw = *(const uint4*)(X + (long)m * ldx + c * 8);
                if (norm_w != nullptr) {
                    float xv[8];
                    unpack8(raw, xv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[j] = wn[j] * rnd(xv[j] * rstd[m]);
                    raw = pack8(xv);
                }
                *(uint4*)(xs + (long)m * K + c * 8) = raw;
            }
        }
        __syncthreads();
    }
    for (int o = gw; o < n_out; o += nwaves) {
        // SwiGLU pack: output o <- gate row (o/16)*32 + o%16 and up row 16 below it
        int row0 = swiglu ? (o >> 4) * 32 + (o & 15) : o;
        int row1_off = 16;
        int r_sec = 0, r_head = 0, r_i = 0;                       // RoPE unit o -> section (q / k / v), head, element i < hd / 2
        if (rope) {
            const int half = ra.hd >> 1, per_sec = ra.H * half;
            r_sec = o / per_sec;
            const int rem = o - r_sec * per_sec;
            r_head = rem / half;
            r_i = rem - r_head * half;
            row0 = (r_sec * ra.H + r_head) * ra.hd + r_i;
            row1_off = half;
        }
        const typename WFmt<WF>::w_t* w0 = WFmt<WF>::rows(W) + (long)row0 * ldw;
        const typename WFmt<WF>::w_t* w1 = w0 + (long)row1_off * ldw;
        float s0 = 1.f, s1 = 1.f;                                 // (WF_FP8) the two rows' scales
        if constexpr (WF == WF_FP8) {
            s0 = W.scales[row0];
            if (swiglu) s1 = W.scales[row0 + row1_off];
        }
        float a0[M], a1[M];
#pragma unroll
        for (int m = 0; m < M; ++m) a0[m] = a1[m] = 0.f;
        if constexpr (WF == WF_MXFP4) {
            // whole superblocks: U 16-byte loads per lane in flight, each the lane's chunks b * 256 + g * 64 + lane, g = 0 .. 3 -- ascending K,
            // the order in which the 16-bit kernel's lane meets them; then the standard-order chunks after the last whole superblock
            const uint8_t* sc0 = W.scales + (long)row0 * W.lds;
            const uint8_t* sc1 = sc0 + (long)row1_off * W.lds;
            const int nsb = nchunk >> 8;
            for (int b0 = 0; b0 < nsb; b0 += U) {
                uint4 wq[U], uq[U];
                uint32_t ws[U], us[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int b = min(b0 + u, nsb - 1);                       // past the end: a repeated, unused superblock
                    wq[u] = w_load16((const elem_t*)(w0 + (long)b * 1024 + lane * 16));
                    ws[u] = *(const uint32_t*)(sc0 + b * 64 + (lane >> 2) * 4);
                    if (swiglu) {
                        uq[u] = w_load16((const elem_t*)(w1 + (long)b * 1024 + lane * 16));
                        us[u] = *(const uint32_t*)(sc1 + b * 64 + (lane >> 2) * 4);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (b0 + u < nsb) {
                        const uint32_t* wc = (const uint32_t*)&wq[u];
                        const uint32_t* uc = (const uint32_t*)&uq[u];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            float wv[8], uv[8];
                            unpack8_w4(wc[g], mx_scale_f32(ws[u] >> (8 * g)), wv);
                            if (swiglu) unpack8_w4(uc[g], mx_scale_f32(us[u] >> (8 * g)), uv);
                            gemv_fma_chunk<M>(wv, uv, swiglu, X, ldx, xs, K, staged, (b0 + u) * 256 + g * 64 + lane, a0, a1);
                        }
                    }
                }
            }
            for (int c = nsb * 256 + lane; c < nchunk; c += 64) {
                float wv[8], uv[8];
                unpack8_w4(*(const uint32_t*)(w0 + (long)c * 4), mx_scale_f32(sc0[c >> 2]), wv);
                if (swiglu) unpack8_w4(*(const uint32_t*)(w1 + (long)c * 4), mx_scale_f32(sc1[c >> 2]), uv);
                gemv_fma_chunk<M>(wv, uv, swiglu, X, ldx, xs, K, staged, c, a0, a1);
            }
        } else {
            for (int c0 = lane; c0 < nchunk; c0 += 64 * U) {
                typename std::conditional<WF == WF_FP8, uint2, uint4>::type wq[U], uq[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int c = c0 + 64 * u;
                    if constexpr (WF == WF_FP8) {
                        wq[u] = c < nchunk ? w_load8(w0 + c * 8) : make_uint2(0, 0);
                        if (swiglu) uq[u] = c < nchunk ? w_load8(w1 + c * 8) : make_uint2(0, 0);
                    } else {
                        wq[u] = c < nchunk ? w_load16(w0 + c * 8) : make_uint4(0, 0, 0, 0);
                        if (swiglu) uq[u] = c < nchunk ? w_load16(w1 + c * 8) : make_uint4(0, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int c = c0 + 64 * u;
                    if (c < nchunk) {
                        float wv[8], uv[8];
                        if constexpr (WF == WF_FP8) {
                            unpack8_w8(wq[u], s0, wv);
                            if (swiglu) unpack8_w8(uq[u], s1, uv);
                        } else {
                            unpack8(wq[u], wv);
                            if (swiglu) unpack8(uq[u], uv);
                        }
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            float xv[8];
                            if (staged) unpack8(*(const uint4*)(xs + (long)m * K + c * 8), xv);
                            else unpack8(*(const uint4*)(X + (long)m * ldx + c * 8), xv);
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                a0[m] += wv[j] * xv[j];
                                if (swiglu) a1[m] += uv[j] * xv[j];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            a0[m] = wave_sum(a0[m]);
            if (swiglu) a1[m] = wave_sum(a1[m]);
        }
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float t;
                if (rope) {
                    const int half = ra.hd >> 1;
                    const float x0 = rnd(a0[m]), x1 = rnd(a1[m]);              // what the q | k | v buffer would hold
                    const int b = m / ra.S, slot = ra.past + (m - b * ra.S);
                    if (r_sec < 2) {
                        const float cs = e2f(ra.cs[(long)m * half + r_i]), sn = e2f(ra.sn[(long)m * half + r_i]);
                        const float o1 = rnd(rnd(x0 * cs) + rnd(-x1 * sn)), o2 = rnd(rnd(x1 * cs) + rnd(x0 * sn));
                        elem_t* dst = r_sec == 0 ? (elem_t*)C + (long)m * ldc + r_head * ra.hd + r_i
                                                 : ra.kc + (((long)b * ra.H + r_head) * ra.smax + slot) * ra.hd + r_i;
                        dst[0] = f2e(o1);
                        dst[half] = f2e(o2);
                    } else {
                        const int w = slot & 31;
                        const int slot_v = (slot & ~31) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3);
                        elem_t* dst = ra.vtc + (((long)b * ra.H + r_head) * ra.hd + r_i) * ra.smax + slot_v;
                        dst[0] = f2e(x0);
                        dst[(long)half * ra.smax] = f2e(x1);
                    }
                    continue;
                }
                if (swiglu) {
                    t = rnd(rnd(act_silu(rnd(a0[m]))) * rnd(a1[m]));
                } else {
                    t = a0[m];
                    if ((flags & EPI_BIAS) && (flags & EPI_BIAS_ROUNDED)) t = rnd(t);
                    if (flags & EPI_BIAS) t += e2f(bias[o]);
                    if (!(flags & EPI_OUT_F32) || act || (flags & EPI_RESID)) t = rnd(t);
                    if (act == 1) t = act_quick_gelu_e(t);
                    else if (act == 2) t = rnd(act_gelu_erf(t));
                    else if (act == 3) t = fmaxf(t, 0.f);
                }
                if (flags & EPI_RESID) t = rnd(e2f(R[(long)m * ldr + o]) + t);
                if (flags & EPI_OUT_F32) ((float*)C)[(long)m * ldc + o] = t;
                else ((elem_t*)C)[(long)m * ldc + o] = f2e(t);
            }
        }
    }
}

// ---- 2 <= M <= 16 (batched decode steps): the same weight stream on the matrix cores -------------------------------------------------
// At M = 4 the GEMV above already spends more time on its 4 x 8 FMAs per weight chunk than on the stream (2.2 TB/s), and M > 4 fell
// to the 128 x 128 GEMM whose grid is a few dozen blocks.  Here 16 output features x 16 (padded) rows of X are one 16x16x32 MFMA per
// 64 bytes of each weight row: a block of 8 waves owns 16 features (SwiGLU: 16 gate + 16 up rows), every wave one eighth of K,
// weight fragments straight from HBM (8 in flight per lane), X fragments from L2 (M x K x 2 bytes, shared by every block), partial
// sums through LDS, then the GEMV's epilogue (same flags, same rounding points).  MFMA work is 16 / M times the useful flops and
// still far below the stream's time.  WF_FP8: 8 code bytes per lane and fragment, turned into the exact bf16 fragment of dequant(W).
// WF_MXFP4: 4 code bytes and the block's scale byte per lane and fragment (a 32-wide k-step is one scale block), at their resident positions;
// v_cvt_scalef32_pk_bf16_fp4 yields the bf16 fragment of dequant(W) directly.
template <bool SW, int WF = WF_ELEM>
__global__ __launch_bounds__(512) void skinny_gemm_kernel(const elem_t* __restrict__ X, long ldx, typename WFmt<WF>::ptr_t W, long ldw, void* C,
                                                          long ldc, const elem_t* __restrict__ bias, const elem_t* __restrict__ R, long ldr, int M,
                                                          int N, int K, int flags, int n_out) {
    __shared__ f32x4_t part[SW ? 2 : 1][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fg = lane >> 4;
    const int o0 = blockIdx.x * 16;                              // first output feature of the block
    // weight row of A-operand row fr: plain: o0 + fr; SwiGLU pack: gate rows (o0/16)*32 + fr, up rows 16 below
    const int wr0 = SW ? (o0 >> 4) * 32 + fr : min(o0 + fr, N - 1);
    const typename WFmt<WF>::w_t* w0 = WFmt<WF>::rows(W) + (long)wr0 * ldw + (WF == WF_MXFP4 ? 0 : fg * 8);   // (mxfp4: see mx_code_pos below)
    const typename WFmt<WF>::w_t* w1 = w0 + 16 * ldw;
    float s0 = 1.f, s1 = 1.f;                                    // (WF_FP8) the scales of rows wr0 and wr0 + 16
    if constexpr (WF == WF_FP8) {
        s0 = W.scales[wr0];
        if constexpr (SW) s1 = W.scales[wr0 + 16];
    }
    const elem_t* xr = X + (long)min(fr, M - 1) * ldx + fg * 8;  // rows >= M repeat the last row: those accumulator columns are not stored
    const int nks = K >> 5;                                      // 32-wide k-steps
    const uint8_t *sc0 = nullptr, *sc1 = nullptr;                // (WF_MXFP4) the scale rows of wr0 and wr0 + 16
    if constexpr (WF == WF_MXFP4) {
        sc0 = W.scales + (long)wr0 * W.lds;
        sc1 = sc0 + 16 * W.lds;
    }
    const int nsb = K >> 11;                                     // (WF_MXFP4) whole superblocks of the resident layout
    const int ks0 = (int)((long)nks * wave / 8), ks1 = (int)((long)nks * (wave + 1) / 8);
    f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    constexpr int U = SW ? 4 : 8;              // (SwiGLU streams two weight rows per fragment: 8 would cost the second block per CU its registers)
    for (int k0 = ks0; k0 < ks1; k0 += U) {
        typename std::conditional<WF == WF_FP8, uint2, typename std::conditional<WF == WF_MXFP4, uint32_t, uint4>::type>::type wq[U], uq[U];
        uint32_t wsc[U], usc[U];                                 // (WF_MXFP4) the k-steps' scale bytes
        uint4 xq[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ks = min(k0 + u, ks1 - 1);                 // past the end: a repeated, unused fragment
            if constexpr (WF == WF_MXFP4) {
                const long cp = mx_code_pos(ks * 4 + fg, nsb), sp = mx_scale_pos(ks, nsb);
                wq[u] = *(const uint32_t*)(w0 + cp);
                wsc[u] = sc0[sp];
                if constexpr (SW) {
                    uq[u] = *(const uint32_t*)(w1 + cp);
                    usc[u] = sc1[sp];
                }
            } else if constexpr (WF == WF_FP8) {
                wq[u] = *(const uint2*)(w0 + ks * 32);
                if constexpr (SW) uq[u] = *(const uint2*)(w1 + ks * 32);
            } else {
                wq[u] = *(const uint4*)(w0 + ks * 32);
                if constexpr (SW) uq[u] = *(const uint4*)(w1 + ks * 32);
            }
            xq[u] = *(const uint4*)(xr + ks * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + u < ks1) {
                if constexpr (WF == WF_MXFP4) {
                    a0 = mfma16(unpack8_w4_bf16(wq[u], mx_scale_f32(wsc[u])), xq[u], a0);
                    if constexpr (SW) a1 = mfma16(unpack8_w4_bf16(uq[u], mx_scale_f32(usc[u])), xq[u], a1);
                } else if constexpr (WF == WF_FP8) {
                    float f[8];
                    unpack8_w8(wq[u], s0, f);
                    a0 = mfma16(pack8(f), xq[u], a0);
                    if constexpr (SW) {
                        unpack8_w8(uq[u], s1, f);
                        a1 = mfma16(pack8(f), xq[u], a1);
                    }
                } else {
                    a0 = mfma16(wq[u], xq[u], a0);
                    if constexpr (SW) a1 = mfma16(uq[u], xq[u], a1);
                }
            }
        }
    }
    part[0][wave][lane] = a0;
    if constexpr (SW) part[1][wave][lane] = a1;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < 8; ++w) {
        a0 += part[0][w][lane];
        if constexpr (SW) a1 += part[1][w][lane];
    }
    // a0[r] = (x_m . w_o) for m = fr, o = o0 + 4 fg + r
    const int m = fr;
    if (m >= M) return;
    const int act = (flags & EPI_ACT_MASK) >> EPI_ACT_SHIFT;
    float t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + fg * 4 + r;
        float v;
        if constexpr (SW) {
            v = rnd(rnd(act_silu(rnd(a0[r]))) * rnd(a1[r]));
        } else {
            v = a0[r];
            if (o < n_out) {
                if ((flags & EPI_BIAS) && (flags & EPI_BIAS_ROUNDED)) v = rnd(v);
                if (flags & EPI_BIAS) v += e2f(bias[o]);
                if (!(flags & EPI_OUT_F32) || act || (flags & EPI_RESID)) v = rnd(v);
                if (act == 1) v = act_quick_gelu_e(v);
                else if (act == 2) v = rnd(act_gelu_erf(v));
                else if (act == 3) v = fmaxf(v, 0.f);
            }
        }
        if ((flags & EPI_RESID) && o < n_out) v = rnd(e2f(R[(long)m * ldr + o]) + v);
        t[r] = v;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + fg * 4 + r;
        if (o < n_out) {
            if (flags & EPI_OUT_F32) ((float*)C)[(long)m * ldc + o] = t[r];
            else ((elem_t*)C)[(long)m * ldc + o] = f2e(t[r]);
        }
    }
}

// ---- host side: one weight descriptor, one launcher per kernel family ---------------------------------------------------------------
// A decode-shape weight as the entries hand it to the launchers: its format, the rows the kernel streams (16-bit elements, or code bytes) with
// their pitch, and for a quantized format the scales (WF_FP8: fp32 [N], lds unused; WF_MXFP4: E8M0 bytes, row pitch lds; both bf16 build only).
struct Weight {
    int fmt;
    const void* rows; int64_t ld;
    const void* scales; int64_t lds;
};

// the kernel argument of a weight in format WF (WFmt<WF>::ptr_t)
template <int WF> inline auto kernel_weight(const Weight& w) {
    if constexpr (WF == WF_FP8) return W8Rows{(const uint8_t*)w.rows, (const float*)w.scales};
    else if constexpr (WF == WF_MXFP4) return W4Rows{(const uint8_t*)w.rows, (const uint8_t*)w.scales, (long)w.lds};
    else return (const elem_t*)w.rows;
}

// a format this build has kernels for, with the pointers it needs
inline bool weight_ok(const Weight& w) {
#ifndef ULL_ELEM_F16
    if (w.fmt == WF_FP8 || w.fmt == WF_MXFP4) return w.rows && w.scales;
#endif
    return w.fmt == WF_ELEM && w.rows;
}
// the row pitches an mxfp4 weight needs: whole rows, 16-byte aligned code rows, 4-byte aligned scale rows
inline bool w4_pitch_ok(int64_t K, int64_t ldw, int64_t lds) { return !(K & 31) && ldw >= K / 2 && !(ldw & 15) && lds >= K / 32 && !(lds & 3); }

// Launch shape of the GEMV per format: U[M - 1] weight loads per lane in flight, BLOCKS the grid cap where every block pays the X staging.
template <int WF> struct GemvShape {                 // 16-bit rows: 16-byte loads; ~2 blocks per CU, several output rows per wave
    static constexpr int U[MAXM] = {8, 4, 4, 4}, BLOCKS = 1024;
};
// Half the bytes per row make a row's latency, not the stream, the limit: more waves in flight (a 1536-block grid where the 16-bit form has
// 1024) and fewer registers per wave (4 loads per lane in flight at M = 1) -- measured on the LLaMA-7B decode step (tools/fp8_decode_bench.py,
// batch 1): U = 16 / 1024 blocks 3.06 ms, U = 8 / 2048 blocks 2.66, U = 4 / 2048 2.56, U = 4 / 1536 2.46, U = 4 / 1280 2.45, U = 4 / 1024 2.51,
// U = 2 / 2048 2.60 (bf16: 3.37).
template <> struct GemvShape<WF_FP8> {
    static constexpr int U[MAXM] = {4, 8, 8, 8}, BLOCKS = 1536;
};
// A quarter of the bytes per row: a K = 4096 row is two 16-byte loads per lane.  The constants are the sweep's choice (profiles/mxfp4_decode.txt,
// batch-1 decode ms per step: U = 1 / 2 / 4 at 1536 blocks 2.58 / 2.50 / 2.92; U = 2 at 1024 / 1536 / 2048 / 3072 / 4096 blocks 2.55 / 2.50 / 2.59 /
// 2.66 / 2.66).  A build with -DULL_W4_TUNE (make HIPCC="/opt/rocm/bin/hipcc -DULL_W4_TUNE"; tools/ only, not part of the ABI in
// include/ullava_hip.h) adds U = 1, 2, 4 instantiations and a process-wide run-time switch, ull_gemv_w4_tune_bf16(u, blocks), which
// tools/mxfp4_decode_bench.py --sweep drives.
constexpr int W4_U = 2, W4_BLOCKS = 1536;
template <> struct GemvShape<WF_MXFP4> {
    static constexpr int U[MAXM] = {W4_U, W4_U, W4_U, W4_U}, BLOCKS = W4_BLOCKS;
};
#ifdef ULL_W4_TUNE
struct W4Tune { int u, blocks; };
W4Tune g_w4_tune = {W4_U, W4_BLOCKS};
#endif
template <int V> using Int = std::integral_constant<int, V>;

template <int WF>
int launch_skinny_as(const void* X, int64_t ldx, const Weight& w, void* C, int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M,
                     int64_t N, int64_t K, int flags, int n_out, hipStream_t st) {
    const auto wk = kernel_weight<WF>(w);
    const unsigned blocks = (unsigned)((n_out + 15) / 16);
    if (flags & EPI_SWIGLU)
        hipLaunchKernelGGL((skinny_gemm_kernel<true, WF>), dim3(blocks), dim3(512), 0, st, (const elem_t*)X, ldx, wk, w.ld, C, ldc, (const elem_t*)bias,
                           (const elem_t*)R, ldr, (int)M, (int)N, (int)K, flags, n_out);
    else
        hipLaunchKernelGGL((skinny_gemm_kernel<false, WF>), dim3(blocks), dim3(512), 0, st, (const elem_t*)X, ldx, wk, w.ld, C, ldc, (const elem_t*)bias,
                           (const elem_t*)R, ldr, (int)M, (int)N, (int)K, flags, n_out);
    return ull_check_launch();
}

int launch_skinny(const void* X, int64_t ldx, const Weight& w, void* C, int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N,
                  int64_t K, int flags, void* stream) {
    if (!X || !weight_ok(w) || !C || M <= 0 || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if (M > 16 || (K & 31) || (ldx & 7) || (w.ld & 7)) return ULL_ERR_SHAPE;
    if (w.fmt == WF_MXFP4 && !w4_pitch_ok(K, w.ld, w.lds)) return ULL_ERR_SHAPE;
    if ((flags & EPI_BIAS) && !bias) return ULL_ERR_ARG;
    if ((flags & EPI_RESID) && !R) return ULL_ERR_ARG;
    if ((flags & EPI_SWIGLU) && ((N & 31) || (flags & (EPI_BIAS | EPI_ACT_MASK)))) return ULL_ERR_SHAPE;
    const int n_out = (int)((flags & EPI_SWIGLU) ? N / 2 : N);
    hipStream_t st = (hipStream_t)stream;
    switch (w.fmt) {
#ifndef ULL_ELEM_F16
        case WF_FP8: return launch_skinny_as<WF_FP8>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, st);
        case WF_MXFP4: return launch_skinny_as<WF_MXFP4>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, st);
#endif
        default: return launch_skinny_as<WF_ELEM>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, st);
    }
}

template <int WF>
int launch_gemv_as(const void* X, int64_t ldx, const Weight& w, void* C, int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N,
                   int64_t K, int flags, int n_out, const void* norm_w, float eps, int staged, const RopeAppend& ra, hipStream_t st) {
    typedef GemvShape<WF> Shape;
    const auto wk = kernel_weight<WF>(w);
    const int lds = staged ? (int)(M * K * 2) : 0;
    int cap = Shape::BLOCKS;
#ifdef ULL_W4_TUNE
    if constexpr (WF == WF_MXFP4) cap = g_w4_tune.blocks;
#endif
    int blocks = (n_out + 3) / 4;
    if (staged && blocks > cap) blocks = cap;
    if (blocks > 8192) blocks = 8192;
    const auto go = [&](auto m, auto u) {
        hipLaunchKernelGGL((gemv_kernel<decltype(m)::value, decltype(u)::value, WF>), dim3(blocks), dim3(256), lds, st, (const elem_t*)X, ldx, wk, w.ld, C,
                           ldc, (const elem_t*)bias, (const elem_t*)R, ldr, (int)N, (int)K, flags, n_out, (const elem_t*)norm_w, eps, staged, ra);
    };
    const auto go_m = [&](auto m) {
#ifdef ULL_W4_TUNE
        if constexpr (WF == WF_MXFP4) {
            if (g_w4_tune.u == 1) return go(m, Int<1>{});
            if (g_w4_tune.u == 4) return go(m, Int<4>{});
            return go(m, Int<2>{});
        } else
#endif
            return go(m, Int<Shape::U[decltype(m)::value - 1]>{});
    };
    switch ((int)M) {
        case 1: go_m(Int<1>{}); break;
        case 2: go_m(Int<2>{}); break;
        case 3: go_m(Int<3>{}); break;
        default: go_m(Int<4>{}); break;
    }
    return ull_check_launch();
}

int launch_gemv(const void* X, int64_t ldx, const Weight& w, void* C, int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N,
                int64_t K, int flags, const void* norm_w, float eps, void* stream, const RopeAppend* rope = nullptr) {
    if (!X || !weight_ok(w) || !C || M <= 0 || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((flags & EPI_ROPE_APPEND) && (!rope || flags != EPI_ROPE_APPEND || (N & 1))) return ULL_ERR_ARG;   // (not part of the public flags)
    const RopeAppend ra = rope ? *rope : RopeAppend{};
    if (M > MAXM || (K & 7) || (ldx & 7) || (w.ld & 7)) return ULL_ERR_SHAPE;
    if (w.fmt == WF_MXFP4 && !w4_pitch_ok(K, w.ld, w.lds)) return ULL_ERR_SHAPE;
    if ((flags & EPI_BIAS) && !bias) return ULL_ERR_ARG;
    if ((flags & EPI_RESID) && !R) return ULL_ERR_ARG;
    if ((flags & EPI_SWIGLU) && ((N & 31) || (flags & (EPI_BIAS | EPI_ACT_MASK)))) return ULL_ERR_SHAPE;
    const int staged = ull_route::gemv_stages(M, K);
    if (norm_w && !staged) return ULL_ERR_SHAPE;
    const int n_out = (int)((flags & (EPI_SWIGLU | EPI_ROPE_APPEND)) ? N / 2 : N);
    hipStream_t st = (hipStream_t)stream;
    switch (w.fmt) {
#ifndef ULL_ELEM_F16
        case WF_FP8: return launch_gemv_as<WF_FP8>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, norm_w, eps, staged, ra, st);
        case WF_MXFP4: return launch_gemv_as<WF_MXFP4>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, norm_w, eps, staged, ra, st);
#endif
        default: return launch_gemv_as<WF_ELEM>(X, ldx, w, C, ldc, bias, R, ldr, M, N, K, flags, n_out, norm_w, eps, staged, ra, st);
    }
}

// The q | k | v projection with RoPE and the cache append (see RopeAppend) on a weight of any format: the checks of its arguments, then the GEMV.
int launch_qkv_rope_append(const void* X, int64_t ldx, const void* norm_w, float eps, const Weight& w, void* Q_out, int64_t ldq, const void* cos_tab,
                           const void* sin_tab, void* k_cache, void* vt_cache, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t K, int64_t smax,
                           int64_t past, void* stream) {
    if (!cos_tab || !sin_tab || !k_cache || !vt_cache || B <= 0 || S <= 0 || H <= 0) return ULL_ERR_ARG;
    if (hd <= 0 || (hd & 1) || past < 0 || past + S > smax || ldq < H * hd) return ULL_ERR_SHAPE;
    RopeAppend ra;
    ra.cs = (const elem_t*)cos_tab; ra.sn = (const elem_t*)sin_tab; ra.kc = (elem_t*)k_cache; ra.vtc = (elem_t*)vt_cache;
    ra.S = (int)S; ra.H = (int)H; ra.hd = (int)hd; ra.smax = (int)smax; ra.past = (int)past;
    return launch_gemv(X, ldx, w, Q_out, ldq, nullptr, nullptr, 0, B * S, 3 * H * hd, K, EPI_ROPE_APPEND, norm_w, norm_w ? eps : 0.f, stream, &ra);
}

}  // namespace

// Same contract as ull_gemm_bf16 (flags, layouts) for M <= 4; K % 8 == 0.
extern "C" int ULL_FN(ull_gemv_)(const void* X, int64_t ldx, const void* W, int64_t ldw, void* C, int64_t ldc, const void* bias, const void* R,
                             int64_t ldr, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    return launch_gemv(X, ldx, Weight{WF_ELEM, W, ldw}, C, ldc, bias, R, ldr, M, N, K, flags, nullptr, 0.f, stream);
}

// The same with the preceding LlamaRMSNorm fused in: C = epilogue(rmsnorm(X; norm_w, eps) * W^T), where gemv_stages(M, K).
extern "C" int ULL_FN(ull_gemv_rmsnorm_)(const void* X, int64_t ldx, const void* norm_w, float eps, const void* W, int64_t ldw, void* C,
                                     int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int flags,
                                     void* stream) {
    if (!norm_w) return ULL_ERR_ARG;
    return launch_gemv(X, ldx, Weight{WF_ELEM, W, ldw}, C, ldc, bias, R, ldr, M, N, K, flags, norm_w, eps, stream);
}

// Decode-step q | k | v projection with RoPE and the KV-cache append in its epilogue (see RopeAppend): W = [3 * H * hd, K] (q | k | v rows),
// M = B * S tokens (<= 4), optional fused RMSNorm (norm_w may be null).  Q_out [M, H * hd] receives the rotated queries; the rotated keys
// go to k_cache[b, h, past + s, :], the values to vt_cache[b, h, :, slot(past + s)].  Same bits as ull_gemv_rmsnorm_ + ull_rope_append_.
extern "C" int ULL_FN(ull_gemv_qkv_rope_append_)(const void* X, int64_t ldx, const void* norm_w, float eps, const void* W, int64_t ldw, void* Q_out,
                                             int64_t ldq, const void* cos_tab, const void* sin_tab, void* k_cache, void* vt_cache, int64_t B,
                                             int64_t S, int64_t H, int64_t hd, int64_t K, int64_t smax, int64_t past, void* stream) {
    return launch_qkv_rope_append(X, ldx, norm_w, eps, Weight{WF_ELEM, W, ldw}, Q_out, ldq, cos_tab, sin_tab, k_cache, vt_cache, B, S, H, hd, K, smax, past,
                                  stream);
}

// The same contract for 2 <= M <= 16 on the matrix cores (batched decode steps); K % 32 == 0.
extern "C" int ULL_FN(ull_gemm_skinny_)(const void* X, int64_t ldx, const void* W, int64_t ldw, void* C, int64_t ldc, const void* bias, const void* R,
                                    int64_t ldr, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    return launch_skinny(X, ldx, Weight{WF_ELEM, W, ldw}, C, ldc, bias, R, ldr, M, N, K, flags, stream);
}

#ifndef ULL_ELEM_F16
// The four entries above on a weight of format wfmt (ULL_WF_*): Q = its rows (row pitch ldq: 16-bit elements, or code bytes), scales / lds as the
// format has them (the two sections below).  Same contract and bits as the bf16 entry on dequant(Q).  bf16 build only.
extern "C" int ull_gemv_wq_bf16(const void* X, int64_t ldx, int wfmt, const void* Q, int64_t ldq, const void* scales, int64_t lds, void* C, int64_t ldc,
                                const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int flags, void* stream) {
    return launch_gemv(X, ldx, Weight{wfmt, Q, ldq, scales, lds}, C, ldc, bias, R, ldr, M, N, K, flags, nullptr, 0.f, stream);
}

extern "C" int ull_gemv_rmsnorm_wq_bf16(const void* X, int64_t ldx, const void* norm_w, float eps, int wfmt, const void* Q, int64_t ldq,
                                        const void* scales, int64_t lds, void* C, int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M,
                                        int64_t N, int64_t K, int flags, void* stream) {
    if (!norm_w) return ULL_ERR_ARG;
    return launch_gemv(X, ldx, Weight{wfmt, Q, ldq, scales, lds}, C, ldc, bias, R, ldr, M, N, K, flags, norm_w, eps, stream);
}

extern "C" int ull_gemv_qkv_rope_append_wq_bf16(const void* X, int64_t ldx, const void* norm_w, float eps, int wfmt, const void* Q, int64_t ldq,
                                                const void* scales, int64_t lds, void* Q_out, int64_t ldq_out, const void* cos_tab,
                                                const void* sin_tab, void* k_cache, void* vt_cache, int64_t B, int64_t S, int64_t H, int64_t hd,
                                                int64_t K, int64_t smax, int64_t past, void* stream) {
    return launch_qkv_rope_append(X, ldx, norm_w, eps, Weight{wfmt, Q, ldq, scales, lds}, Q_out, ldq_out, cos_tab, sin_tab, k_cache, vt_cache, B, S, H, hd,
                                  K, smax, past, stream);
}

extern "C" int ull_gemm_skinny_wq_bf16(const void* X, int64_t ldx, int wfmt, const void* Q, int64_t ldq, const void* scales, int64_t lds, void* C,
                                       int64_t ldc, const void* bias, const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int flags,
                                       void* stream) {
    return launch_skinny(X, ldx, Weight{wfmt, Q, ldq, scales, lds}, C, ldc, bias, R, ldr, M, N, K, flags, stream);
}
#endif  // !ULL_ELEM_F16

// ---- FP8 (e4m3) weight-only decode: bf16 build only ------------------------------------------------------------------------------
// A weight W [N, K] is stored as e4m3fn codes q [N, K] plus one fp32 scale 2^s per row, s the smallest integer with amax|w| * 2^-s <= 448
// (all-zero row: s = 0), q = e4m3fn(w * 2^-s) rounded to nearest even.  dequant(q) = float(q) * 2^s is exactly representable in bf16, so
// the fp8 kernels above compute exactly what the 16-bit kernels compute on dequant(W).
#ifndef ULL_ELEM_F16
namespace {

// one row per wave: amax, the power-of-two scale, then the codes (8 per lane and chunk, like the GEMV's weight chunks)
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const elem_t* __restrict__ W, long ldw, int N, int K, uint8_t* __restrict__ codes,
                                                                float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const elem_t* w = W + (long)row * ldw;
    const int nchunk = K >> 3;
    float amax = 0.f;
    for (int c = lane; c < nchunk; c += 64) {
        float v[8];
        unpack8(*(const uint4*)(w + c * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    amax = wave_max(amax);
    const int s = fp8_scale_exp(amax);
    if (lane == 0) scales[row] = ldexpf(1.f, s);
    uint8_t* q = codes + (long)row * K;
    for (int c = lane; c < nchunk; c += 64) {
        float v[8];
        unpack8(*(const uint4*)(w + c * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ldexpf(v[j], -s);     // exact; |v| <= 448: the conversion cannot overflow
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
        *(uint2*)(q + c * 8) = make_uint2((uint32_t)lo, (uint32_t)hi);
    }
}

// codes -> dequant(W) in bf16, row-major [N, K] or (tiled) the ULL_EPI_W_TILED layout [ceil(N/256)][K/64][256][64] of ull_gemm_bf16
// with the padding rows zeroed.  One thread per 8 elements.
__global__ __launch_bounds__(256) void dequantize_rows_fp8_kernel(const uint8_t* __restrict__ codes, long ldq, const float* __restrict__ scales,
                                                                  int N, int K, elem_t* __restrict__ out, int tiled, long total) {
    const int g8 = K >> 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / g8), k = (int)(i - (long)n * g8) * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (n < N) {
            float f[8];
            unpack8_w8(*(const uint2*)(codes + (long)n * ldq + k), scales[n], f);
            v = pack8(f);
        }
        const long o = tiled ? (((long)(n >> 8) * (K >> 6) + (k >> 6)) * 256 + (n & 255)) * 64 + (k & 63) : (long)n * K + k;
        *(uint4*)(out + o) = v;
    }
}

}  // namespace

// Per-row e4m3 quantization (see above) of a bf16 weight W [N, K] (row pitch ldw): codes [N, K] (pitch K bytes), scales [N] fp32.
// Bit-identical to torch's CPU cast (w.float() * 2^-s).to(torch.float8_e4m3fn).  K % 8 == 0.
extern "C" int ULL_FN(ull_quantize_rows_fp8_)(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, void* scales, void* stream) {
    if (!W || !codes || !scales || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 7) || (ldw & 7) || ldw < K || N > (1 << 28)) return ULL_ERR_SHAPE;
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const elem_t*)W, (long)ldw,
                       (int)N, (int)K, (uint8_t*)codes, (float*)scales);
    return ull_check_launch();
}

// dequant(codes) into a bf16 buffer: tiled = 0: row-major [N, K]; tiled = 1: ull_gemm_bf16's ULL_EPI_W_TILED layout (K % 64 == 0;
// out holds ceil(N / 256) * 256 * K elements).  The prefill path of an fp8 weight: this, then the unchanged 16-bit GEMM.
extern "C" int ULL_FN(ull_dequantize_rows_fp8_)(const void* codes, int64_t ldq, const void* scales, int64_t N, int64_t K, void* out, int tiled,
                                                void* stream) {
    if (!codes || !scales || !out || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 7) || (ldq & 7) || ldq < K || (tiled && (K & 63))) return ULL_ERR_SHAPE;
    const long rows = tiled ? (N + 255) / 256 * 256 : N;
    const long total = rows * (K >> 3);
    const long blocks = std::min<long>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(dequantize_rows_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, (long)ldq,
                       (const float*)scales, (int)N, (int)K, (elem_t*)out, tiled, total);
    return ull_check_launch();
}

#endif  // !ULL_ELEM_F16

// ---- MXFP4 weight-only decode: bf16 build only -------------------------------------------------------------------------------------
// A weight W [N, K], K % 32 == 0, is stored as e2m1 codes (two per byte, element 2i in the low nibble: [N, K / 2] bytes) plus one E8M0 scale
// byte s + 127 per row and block of 32 consecutive K elements ([N, K / 32]); s is the smallest integer with amax|block| * 2^-s <= 6 (all-zero
// block: s = 0) clamped to [-125, 126], a code is e2m1(w * 2^-s) rounded to nearest, ties to the even code, sign in bit 3 (ull_common.h).
// dequant = e2m1 * 2^s is exactly a bf16 value, so the mxfp4 kernels above compute exactly what the 16-bit kernels compute on dequant(W).
// `resident` selects the byte order within a row: 0 the standard layout just described, 1 the resident layout the decode kernels read
// (mx_code_pos / mx_scale_pos: a permutation of the standard layout's bytes within the row).
#ifndef ULL_ELEM_F16
namespace {

// one row per wave; a lane owns chunks of 8 elements, four neighbouring lanes one scale block
__global__ __launch_bounds__(256) void quantize_rows_mxfp4_kernel(const elem_t* __restrict__ W, long ldw, int N, int K, uint8_t* __restrict__ codes,
                                                                  long ldq, uint8_t* __restrict__ scales, long lds, int resident) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const elem_t* w = W + (long)row * ldw;
    const int nchunk = K >> 3, nsb = resident ? nchunk >> 8 : 0;
    uint8_t* q = codes + (long)row * ldq;
    uint8_t* sc = scales + (long)row * lds;
    for (int c0 = 0; c0 < nchunk; c0 += 64) {                    // (nchunk % 4 == 0: the four lanes of a block are in or out together)
        const int c = c0 + lane;
        float v[8];
        if (c < nchunk) unpack8(*(const uint4*)(w + c * 8), v);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
        amax = group_max(amax, 4);
        const int s = mxfp4_scale_exp(amax);
        if (c < nchunk) {
            uint32_t code = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) code |= mxfp4_code(ldexpf(v[j], -s), s == 126 ? 5u : 7u) << (4 * j);     // exact, or below a quarter of the smallest step
            *(uint32_t*)(q + mx_code_pos(c, nsb)) = code;
            if ((lane & 3) == 0) sc[mx_scale_pos(c >> 2, nsb)] = (uint8_t)(s + 127);
        }
    }
}

// codes -> dequant(W) in bf16, row-major [N, K] or (tiled) the ULL_EPI_W_TILED layout of ull_gemm_bf16 with the padding rows zeroed.
// One thread per 8 elements.
__global__ __launch_bounds__(256) void dequantize_rows_mxfp4_kernel(const uint8_t* __restrict__ codes, long ldq, const uint8_t* __restrict__ scales,
                                                                    long lds, int N, int K, elem_t* __restrict__ out, int tiled, int resident,
                                                                    long total) {
    const int g8 = K >> 3, nsb = resident ? g8 >> 8 : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / g8), c = (int)(i - (long)n * g8), k = c * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (n < N)
            v = unpack8_w4_bf16(*(const uint32_t*)(codes + (long)n * ldq + mx_code_pos(c, nsb)),
                                mx_scale_f32(scales[(long)n * lds + mx_scale_pos(c >> 2, nsb)]));
        const long o = tiled ? (((long)(n >> 8) * (K >> 6) + (k >> 6)) * 256 + (n & 255)) * 64 + (k & 63) : (long)n * K + k;
        *(uint4*)(out + o) = v;
    }
}

}  // namespace

// MXFP4 quantization (see above) of a bf16 weight W [N, K] (row pitch ldw elements): codes [N, K / 2] bytes (row pitch ldq), scales
// [N, K / 32] bytes (row pitch lds).  K % 32 == 0.
extern "C" int ULL_FN(ull_quantize_rows_mxfp4_)(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldq, void* scales, int64_t lds,
                                                int resident, void* stream) {
    if (!W || !codes || !scales || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 31) || (ldw & 7) || ldw < K || (ldq & 3) || ldq < K / 2 || lds < K / 32 || N > (1 << 28)) return ULL_ERR_SHAPE;
    hipLaunchKernelGGL(quantize_rows_mxfp4_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const elem_t*)W, (long)ldw,
                       (int)N, (int)K, (uint8_t*)codes, (long)ldq, (uint8_t*)scales, (long)lds, resident ? 1 : 0);
    return ull_check_launch();
}

// dequant(codes) into a bf16 buffer: tiled = 0: row-major [N, K]; tiled = 1: ull_gemm_bf16's ULL_EPI_W_TILED layout (K % 64 == 0; out holds
// ceil(N / 256) * 256 * K elements).  The prefill path of an mxfp4 weight: this, then the unchanged 16-bit GEMM.
extern "C" int ULL_FN(ull_dequantize_rows_mxfp4_)(const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t N, int64_t K, void* out,
                                                  int tiled, int resident, void* stream) {
    if (!codes || !scales || !out || N <= 0 || K <= 0) return ULL_ERR_ARG;
    if ((K & 31) || (ldq & 3) || ldq < K / 2 || lds < K / 32 || (tiled && (K & 63))) return ULL_ERR_SHAPE;
    const long rows = tiled ? (N + 255) / 256 * 256 : N;
    const long total = rows * (K >> 3);
    const long blocks = std::min<long>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(dequantize_rows_mxfp4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)codes, (long)ldq,
                       (const uint8_t*)scales, (long)lds, (int)N, (int)K, (elem_t*)out, tiled, resident ? 1 : 0, total);
    return ull_check_launch();
}

#ifdef ULL_W4_TUNE
// (ULL_W4_TUNE builds only) the launch shape of the mxfp4 GEMV for the sweep of tools/mxfp4_decode_bench.py: u = 1, 2 or 4, blocks = 256 .. 8192.
extern "C" int ull_gemv_w4_tune_bf16(int u, int blocks) {
    if ((u != 1 && u != 2 && u != 4) || blocks < 256 || blocks > 8192) return ULL_ERR_ARG;
    g_w4_tune = W4Tune{u, blocks};
    return ULL_OK;
}
#endif
#endif  // !ULL_ELEM_F16
