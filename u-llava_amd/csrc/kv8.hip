// FP8 (e4m3) KV cache for KV-cached LLaMA decoding, bf16 build only (compiled once): the decode attention that reads the cache's codes,
// and the kernels that quantize positions into it and dequantize them out of it.
//
// attn_fewq_kv8_kernel is compiled from the same text as attention.hip's attn_fewq_kernel, attn_fewq_body.inc (<= 16 queries, the keys
// split over the waves of one block per head); the text's fp8 arms build the cached keys' K / V^T fragments from codes: each lane turns
// its 8 codes into exactly the bf16 operand the 16-bit kernel loads from the dequantized cache.  The Sq new keys come from a bf16 staging
// window.  MFMAs, lane mapping, rounding points and reduction order exist once, so the result equals attn_fewq_kernel's on the
// dequantized cache bit for bit.  After the attention the block quantizes the new keys' K rows and V columns (staging -> codes and
// scales): a block owns its (batch, head) and never reads the cache at the positions it writes.
#ifdef ULL_ELEM_F16
#error "kv8.hip is bf16 only"
#endif
#include "attention_common.h"
#include <algorithm>

namespace {

// ---------------------------------------------------------------------------------------------
// FP8 (e4m3) KV cache (bf16 build only; ull_attention_kv8 / ull_kv8_quantize / ull_kv8_dequantize).  Per layer: K codes [B, H, smax, hd]
// and V^T codes [B, H, hd, smax] in the key-permuted slot order of transpose_v, one fp32 power-of-two scale per (batch, head, position)
// for the K row (ks [B, H, smax], indexed by key) and one for the V column (vs [B, H, smax], indexed by V^T slot).  The scale and code
// rule is the fp8-weight rule of ull_common.h (fp8_scale_exp), so dequant = float(code) * 2^s is a bf16 value.
struct Kv8Args {
    uint8_t* k8; uint8_t* vt8;          // codes
    float* ks; float* vs;               // scales
    int smax;                           // cache pitch (positions), multiple of 64
};
// V^T slot of key k (32-key blocks: slot 8g + 4a + r holds key 16a + 4g + r)
ULL_DEV int kv8_slot(int k) {
    const int w = k & 31;
    return (k & ~31) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3);
}
// the 8 slots slot0 .. slot0 + 7 (slot0 % 8 == 0) hold keys klo + 0..3 (elements 0..3) and klo + 16 + 0..3 (elements 4..7)
ULL_DEV int kv8_klo(int slot0) { return (slot0 & ~31) + 4 * ((slot0 & 31) >> 3); }
ULL_DEV void kv8_load_vsc(const Kv8Args& kv, long bh, int slot0, int past, float* sc) {
    if (kv8_klo(slot0) < past) {
        const float4 a = *(const float4*)(kv.vs + bh * kv.smax + slot0), b = *(const float4*)(kv.vs + bh * kv.smax + slot0 + 4);
        sc[0] = a.x; sc[1] = a.y; sc[2] = a.z; sc[3] = a.w; sc[4] = b.x; sc[5] = b.y; sc[6] = b.z; sc[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) sc[e] = 0.f;
    }
}
ULL_DEV uint2 kv8_load_vcode(const Kv8Args& kv, long bh, int hd, int d, int slot0, int past) {
    return kv8_klo(slot0) < past ? *(const uint2*)(kv.vt8 + (bh * hd + d) * kv.smax + slot0) : make_uint2(0, 0);
}
// One 8-slot V^T fragment: element e from the codes (float(q) * its slot's scale) where its key is < past, from the bf16 row `stg` where
// past <= key < end, zero for keys >= end.  (Keys >= end carry probability 0, but a stale staging value there could be non-finite: the
// zero keeps P * V exact whatever the staging window held before.)  stg is read only when some key of the fragment is in [past, end).
ULL_DEV uint4 kv8_vfrag(uint2 q, const float* sc, int slot0, int past, int end, const elem_t* stg) {
    const int klo = kv8_klo(slot0);
    float f[8];
    unpack8_w8(q, 1.0f, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] *= sc[e];
    if (klo + 19 >= past) {
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (stg && klo < end) unpack8(*(const uint4*)stg, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = klo + (e >> 2) * 16 + (e & 3);
            if (key >= past) f[e] = key < end ? g[e] : 0.f;
        }
    }
    return pack8(f);
}
// One wave quantizes one vector of hd <= 128 bf16 values (element i at src[i * sstride]) into codes dst[i * dstride] and its scale.
ULL_DEV void kv8_quant_vec(const elem_t* src, long sstride, int hd, uint8_t* dst, long dstride, float* scale, int lane) {
    const float x0 = lane < hd ? e2f(src[lane * sstride]) : 0.f;
    const float x1 = lane + 64 < hd ? e2f(src[(lane + 64) * sstride]) : 0.f;
    const int s = fp8_scale_exp(wave_max(fmaxf(fabsf(x0), fabsf(x1))));
    if (lane == 0) *scale = ldexpf(1.f, s);
    const int c = __builtin_amdgcn_cvt_pk_fp8_f32(ldexpf(x0, -s), ldexpf(x1, -s), 0, false);     // exact scaling; |x| <= 448
    if (lane < hd) dst[lane * dstride] = (uint8_t)(c & 0xff);
    if (lane + 64 < hd) dst[(lane + 64) * dstride] = (uint8_t)((c >> 8) & 0xff);
}

template <int HDP, int FL, int TPW>
__global__ __launch_bounds__(1024) void attn_fewq_kv8_kernel(AttnArgs p, Kv8Args kv) {
#define ULL_FEWQ_KV8
#include "attn_fewq_body.inc"
#undef ULL_FEWQ_KV8
}

// the block shape and TPW of the 16-bit launch it replaces: the same rule (launch_fewq_as)
template <int HDP, int FL>
int launch_fewq_kv8(const AttnArgs& a, const Kv8Args& kv, hipStream_t st) {
    return launch_fewq_as<attn_fewq_kv8_kernel<HDP, FL, 1>, attn_fewq_kv8_kernel<HDP, FL, 4>, HDP>(a, st, kv);
}

// positions p0 .. p0 + n - 1 into the cache: block (s, b * H + h), wave 0 quantizes the K row, wave 1 the V column of position p0 + s.
// Source position src_p0 + s: K rows by (k_bs, k_hs, k_ss); V rows by (v_bs, v_hs, v_ss) or (v_image) a V^T image [.., hd, pitch v_ss]
// in the permuted slot order.
__global__ __launch_bounds__(128) void kv8_quantize_kernel(const elem_t* __restrict__ K, long k_bs, long k_hs, long k_ss, const elem_t* __restrict__ V,
                                                           long v_bs, long v_hs, long v_ss, int v_image, int src_p0, Kv8Args kv, int H, int hd, int p0) {
    const int s = blockIdx.x;
    const long bh = blockIdx.y;
    const int b = (int)(bh / H), h = (int)(bh % H);
    const int lane = threadIdx.x & 63;
    const int key = p0 + s, sk = src_p0 + s;
    if (threadIdx.x < 64) {
        kv8_quant_vec(K + b * k_bs + h * k_hs + sk * k_ss, 1, hd, kv.k8 + (bh * kv.smax + key) * hd, 1, kv.ks + bh * kv.smax + key, lane);
    } else {
        const int slot = kv8_slot(key);
        const elem_t* src = V + b * v_bs + h * v_hs + (v_image ? (long)kv8_slot(sk) : (long)sk * v_ss);
        kv8_quant_vec(src, v_image ? v_ss : 1, hd, kv.vt8 + bh * hd * kv.smax + slot, kv.smax, kv.vs + bh * kv.smax + slot, lane);
    }
}

// positions [0, n) of the cache -> bf16 K [B, H, k_pitch, hd] and V^T [B, H, hd, vt_pitch] (slots [0, round_up(n, 64)); keys >= n zero).
// The same conversions as the fp8 attention's operands.  One thread per 8 elements: first the K chunks, then the V^T chunks.
__global__ __launch_bounds__(256) void kv8_dequantize_kernel(Kv8Args kv, int hd, int n, elem_t* __restrict__ Ko, long k_pitch, elem_t* __restrict__ Vo,
                                                             long vt_pitch, long nk, long total) {
    const int c8 = hd >> 3, nv8 = ((n + 63) & ~63) >> 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < nk) {
            const long bh = i / ((long)n * c8);
            const long r = i - bh * n * c8;
            const int pos = (int)(r / c8), c = (int)(r - (long)pos * c8) * 8;
            float f[8];
            unpack8_w8(*(const uint2*)(kv.k8 + (bh * kv.smax + pos) * hd + c), kv.ks[bh * kv.smax + pos], f);
            *(uint4*)(Ko + (bh * k_pitch + pos) * hd + c) = pack8(f);
        } else {
            const long j = i - nk;
            const long bh = j / ((long)hd * nv8);
            const long r = j - bh * hd * nv8;
            const int d = (int)(r / nv8), slot0 = (int)(r - (long)d * nv8) * 8;
            float sc[8];
            kv8_load_vsc(kv, bh, slot0, n, sc);
            *(uint4*)(Vo + (bh * hd + d) * vt_pitch + slot0) = kv8_vfrag(kv8_load_vcode(kv, bh, hd, d, slot0, n), sc, slot0, n, n, nullptr);
        }
    }
}

}  // namespace

// ---- FP8 (e4m3) KV cache, bf16 build only (see Kv8Args) ----------------------------------------------------------------------------
static bool kv8_cache_ok(const void* k8, const void* vt8, const void* ks, const void* vs, int64_t B, int64_t H, int64_t hd, int64_t smax) {
    return k8 && vt8 && ks && vs && B > 0 && H > 0 && hd > 0 && hd <= 128 && (hd & 15) == 0 && smax > 0 && (smax & 63) == 0 &&
           B * H * smax * hd < (1L << 40);
}

// KV-cached decode attention over an fp8 cache (scale_mode 1, causal: the LLaMA decode call).  Keys < past = Sk - Sq from the cache
// (k8 / vt8 / k_scale / vt_scale, pitch smax); the Sq new keys from the bf16 staging window: K rows k_stage [B, H, 128, hd] and V^T
// vt_stage [B, H, hd, 128] (permuted slots) hold key k at row / slot k - w0, w0 = past rounded down to a multiple of 64 -- where the
// decode appenders put them when called on the staging buffers with smax = 128 and past - w0.  The kernel then stores the new keys'
// codes and scales into the cache.  Equals ull_attention_bf16 on the dequantized cache (ull_kv8_dequantize) with the new keys appended,
// bit for bit.  1 <= Sq <= 16, 2 <= ceil(Sk / 64) <= 64 (other shapes: ULL_ERR_SHAPE, nothing launched).
extern "C" int ull_attention_kv8_bf16(const void* Q, int64_t q_bs, int64_t q_hs, int64_t q_ss, const void* k_stage, const void* vt_stage,
                                      const void* k8, const void* vt8, const void* k_scale, const void* vt_scale, int64_t smax, void* O, int64_t o_bs,
                                      int64_t o_hs, int64_t o_ss, const void* key_mask, int64_t B, int64_t H, int64_t Sq, int64_t Sk, int64_t hd,
                                      float scale, const void* zeros, void* stream) {
    if (!Q || !k_stage || !vt_stage || !O || !zeros || !kv8_cache_ok(k8, vt8, k_scale, vt_scale, B, H, hd, smax)) return ULL_ERR_ARG;
    const int64_t nt = (Sk + KT - 1) / KT;
    if (Sq < 1 || Sq > 16 || Sk <= Sq || Sk > smax || nt < 2 || nt > 64) return ULL_ERR_SHAPE;
    if ((q_ss & 7) || (q_hs & 7) || (q_bs & 7) || (o_ss & 3) || (o_hs & 3) || (o_bs & 3)) return ULL_ERR_SHAPE;
    AttnArgs a = attn_args({Q, q_bs, q_hs, q_ss}, {k_stage, H * 128 * hd, 128 * hd, hd}, {vt_stage, H * hd * 128, hd * 128, 128},
                           {O, o_bs, o_hs, o_ss}, B, H, Sq, Sk, hd);
    a.key_mask = (const int32_t*)key_mask;
    a.vt_len = 128;
    a.causal = 1; a.scale_mode = 1; a.scale = scale;
    a.zeros = (const elem_t*)zeros;
    Kv8Args kv;
    kv.k8 = (uint8_t*)k8; kv.vt8 = (uint8_t*)vt8; kv.ks = (float*)k_scale; kv.vs = (float*)vt_scale; kv.smax = (int)smax;
    hipStream_t st = (hipStream_t)stream;
    // the kernel ull_attention_bf16 picks for these arguments (dispatch_nt: FL_LLAMA at head_dim 128, the run-time flavor otherwise)
    if (hd <= 32) return launch_fewq_kv8<32, FL_RUNTIME>(a, kv, st);
    if (hd <= 64) return launch_fewq_kv8<64, FL_RUNTIME>(a, kv, st);
    if (hd == 128) return launch_fewq_kv8<128, FL_LLAMA>(a, kv, st);
    return launch_fewq_kv8<128, FL_RUNTIME>(a, kv, st);
}

// Quantize positions p0 .. p0 + n - 1 of one layer's cache from bf16 sources (source position src_p0 + s): K rows K + b k_bs + h k_hs +
// pos k_ss; V rows V + b v_bs + h v_hs + pos v_ss (v_image = 0) or a V^T image in the permuted slot order, d stride v_ss (v_image = 1).
extern "C" int ull_kv8_quantize_bf16(const void* K, int64_t k_bs, int64_t k_hs, int64_t k_ss, const void* V, int64_t v_bs, int64_t v_hs, int64_t v_ss,
                                     int v_image, int64_t src_p0, void* k8, void* vt8, void* k_scale, void* vt_scale, int64_t B, int64_t H, int64_t hd,
                                     int64_t smax, int64_t p0, int64_t n, void* stream) {
    if (!K || !V || !kv8_cache_ok(k8, vt8, k_scale, vt_scale, B, H, hd, smax) || n <= 0) return ULL_ERR_ARG;
    if (p0 < 0 || src_p0 < 0 || p0 + n > smax || (v_image != 0 && v_image != 1) || B * H > 0x7fffffff) return ULL_ERR_SHAPE;
    Kv8Args kv;
    kv.k8 = (uint8_t*)k8; kv.vt8 = (uint8_t*)vt8; kv.ks = (float*)k_scale; kv.vs = (float*)vt_scale; kv.smax = (int)smax;
    hipLaunchKernelGGL(kv8_quantize_kernel, dim3((unsigned)n, (unsigned)(B * H)), dim3(128), 0, (hipStream_t)stream, (const elem_t*)K, (long)k_bs,
                       (long)k_hs, (long)k_ss, (const elem_t*)V, (long)v_bs, (long)v_hs, (long)v_ss, v_image, (int)src_p0, kv, (int)H, (int)hd, (int)p0);
    return ull_check_launch();
}

// Dequantize positions [0, n) of one layer's cache: K_out [B, H, k_pitch, hd] rows 0 .. n - 1 and Vt_out [B, H, hd, vt_pitch] slots
// 0 .. round_up(n, 64) - 1 (keys >= n zero), either may be null.  dequant = float(code) * 2^s, exactly the operands ull_attention_kv8 reads.
extern "C" int ull_kv8_dequantize_bf16(const void* k8, const void* vt8, const void* k_scale, const void* vt_scale, int64_t B, int64_t H, int64_t hd,
                                       int64_t smax, int64_t n, void* K_out, int64_t k_pitch, void* Vt_out, int64_t vt_pitch, void* stream) {
    if (!kv8_cache_ok(k8, vt8, k_scale, vt_scale, B, H, hd, smax) || n <= 0 || (!K_out && !Vt_out)) return ULL_ERR_ARG;
    const int64_t nv = (n + 63) & ~63;
    if (n > smax || (K_out && k_pitch < n) || (Vt_out && ((vt_pitch & 7) || vt_pitch < nv))) return ULL_ERR_SHAPE;
    Kv8Args kv;
    kv.k8 = (uint8_t*)k8; kv.vt8 = (uint8_t*)vt8; kv.ks = (float*)k_scale; kv.vs = (float*)vt_scale; kv.smax = (int)smax;
    const long nk = K_out ? (long)(B * H * n * (hd >> 3)) : 0;
    const long total = nk + (Vt_out ? (long)(B * H * hd * (nv >> 3)) : 0);
    const long blocks = std::min<long>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(kv8_dequantize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, kv, (int)hd, (int)n, (elem_t*)K_out,
                       (long)k_pitch, (elem_t*)Vt_out, (long)vt_pitch, nk, total);
    return ull_check_launch();
}

