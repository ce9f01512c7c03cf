// Coarse C-ABI entries: ONE call enqueues a whole stack of transformer layers on the stream (round 6).
//
// Host code only -- no kernel lives here.  Every function below calls the per-op entry points of this library (the same kernels, picked by the
// same dispatch rule, linear_route.h, that u-llava_amd/ops.py reads call by call), so the results are bit-identical to the per-op path; what changes is the host
// cost: a ctypes round trip + Python argument marshalling per LAUNCH (~15 us, profiles/r05_decode.txt) becomes one per FORWARD.  With eight
// Python ranks sharing one host that is the margin the >= 6x target has.
//
// Reference lines replaced: hf LlamaModel.forward's layer loop (modeling_llama.py:347-419 through models/ullava_core.py:312-322), hf
// CLIPEncoder.forward's layer loop (modeling_clip.py:353-384 through models/ullava_core.py:146-158), ImageEncoderViT.forward's block loop
// (models/segment_anything/modeling/image_encoder.py:110-116, Block.forward :165-193).
#include <stdint.h>
#include <math.h>

#include "linear_route.h"

#ifdef ULL_ELEM_F16
#define FN(base) base##f16
#else
#define FN(base) base##bf16
#endif
#define TRY(call)                 \
    do {                          \
        const int rc_ = (call);   \
        if (rc_ != ULL_OK) return rc_; \
    } while (0)

namespace {

struct SK {                      // the caller's stream-K policy (ops.streamk_policy) and workspace
    void* ws;
    int64_t bytes;
    int64_t min_k;               // < 0: never split
};

// How the tiled GEMM runs a Linear at M rows (ull_route::is_big / gemm_split): a "big" shape takes the tile-major weight where there is one, and
// the workspace where the rule splits K (the small-M split-K mode is never on here: the host takes the per-op path while it is).
struct Tiled {
    const void* w;
    int64_t ldw;
    int flags;
    void* ws;
    int64_t wsb;
};
inline Tiled tiled(const ull_linear* L, int64_t M, const SK& sk) {
    const bool big = ull_route::is_big(M, L->n, L->k);
    Tiled t{L->w, L->ldw, 0, nullptr, 0};
    if (big && L->w_tiled) { t.w = L->w_tiled; t.ldw = L->k; t.flags = ULL_EPI_W_TILED; }
    if (ull_route::gemm_split(big, M, L->n, L->k, sk.min_k, false, false)) { t.ws = sk.ws; t.wsb = sk.bytes; }
    return t;
}

// ops.linear on a 16-bit weight where the rule says GEMM (K % 64 == 0): the tiled GEMM.  The entries below admit no other shape.
inline int lin(const void* x, int64_t ldx, const ull_linear* L, void* out, int64_t ldc, const void* R, int64_t ldr, int64_t M, int flags,
               const SK& sk, void* stream) {
    if (ull_route::route_of(M, L->n, L->k, L->ldw, ULL_WF_ELEM, ULL_AF_NONE, false, 0).kind != ULL_ROUTE_GEMM) return ULL_ERR_SHAPE;
    const Tiled t = tiled(L, M, sk);
    if (L->bias) flags |= ULL_EPI_BIAS;
    if (R) flags |= ULL_EPI_RESID;
    return FN(ull_gemm_)(x, ldx, t.w, t.ldw, out, ldc, L->bias, R, ldr, M, L->n, L->k, flags | t.flags, t.ws, t.wsb, stream);
}

// A decode-shape Linear in any weight format (ull_linear.format): a quantized one (bf16 build only) has no bias and goes to the *_wq_bf16 form of
// the entry, which takes the format as an argument.  format_ok: a format this build's entries take; has_weight: its pointers are there;
// pitch_ok: the rows are whole; ldw_of: the row pitch the routing rule (ull_route::route_of) sees.
inline bool quantized(const ull_linear* L) { return L->format != ULL_WF_ELEM; }
inline bool format_ok(const ull_linear* L) {
#ifndef ULL_ELEM_F16
    if (L->format == ULL_WF_FP8 || L->format == ULL_WF_MXFP4) return true;
#endif
    return !quantized(L);
}
inline bool has_weight(const ull_linear* L) { return L->w && (!quantized(L) || L->scales); }
inline bool pitch_ok(const ull_linear* L) {
    if (L->format == ULL_WF_MXFP4) return L->k % 32 == 0 && L->ldw >= L->k / 2 && L->ldw % 16 == 0 && L->lds >= L->k / 32 && L->lds % 4 == 0;
    return L->ldw >= L->k;
}
inline const void* bias_of(const ull_linear* L) { return quantized(L) ? nullptr : L->bias; }
// (ops.linear passes K for an Mxfp4Weight: its rows are always whole)
inline int64_t ldw_of(const ull_linear* L) { return L->format == ULL_WF_MXFP4 ? L->k : L->ldw; }
inline int gemm_skinny(const void* x, int64_t ldx, const ull_linear* L, void* out, int64_t ldc, const void* R, int64_t ldr, int64_t M, int flags,
                       void* stream) {
#ifndef ULL_ELEM_F16
    if (quantized(L))
        return ull_gemm_skinny_wq_bf16(x, ldx, L->format, L->w, L->ldw, L->scales, L->lds, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags, stream);
#endif
    return FN(ull_gemm_skinny_)(x, ldx, L->w, L->ldw, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags, stream);
}
inline int gemv(const void* x, int64_t ldx, const ull_linear* L, void* out, int64_t ldc, const void* R, int64_t ldr, int64_t M, int flags, void* stream) {
#ifndef ULL_ELEM_F16
    if (quantized(L)) return ull_gemv_wq_bf16(x, ldx, L->format, L->w, L->ldw, L->scales, L->lds, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags, stream);
#endif
    return FN(ull_gemv_)(x, ldx, L->w, L->ldw, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags, stream);
}
inline int gemv_rmsnorm(const void* x, int64_t ldx, const void* rms_w, float eps, const ull_linear* L, void* out, int64_t ldc, const void* R,
                        int64_t ldr, int64_t M, int flags, void* stream) {
#ifndef ULL_ELEM_F16
    if (quantized(L))
        return ull_gemv_rmsnorm_wq_bf16(x, ldx, rms_w, eps, L->format, L->w, L->ldw, L->scales, L->lds, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags,
                                        stream);
#endif
    return FN(ull_gemv_rmsnorm_)(x, ldx, rms_w, eps, L->w, L->ldw, out, ldc, bias_of(L), R, ldr, M, L->n, L->k, flags, stream);
}
inline int gemv_qkv_rope_append(const void* x, int64_t ldx, const void* rms_w, float eps, const ull_linear* L, void* q, int64_t ldq, const void* cs,
                                const void* sn, void* kc, void* vtc, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t smax, int64_t past,
                                void* stream) {
#ifndef ULL_ELEM_F16
    if (quantized(L))
        return ull_gemv_qkv_rope_append_wq_bf16(x, ldx, rms_w, eps, L->format, L->w, L->ldw, L->scales, L->lds, q, ldq, cs, sn, kc, vtc, B, S, H, hd, L->k,
                                                smax, past, stream);
#endif
    return FN(ull_gemv_qkv_rope_append_)(x, ldx, rms_w, eps, L->w, L->ldw, q, ldq, cs, sn, kc, vtc, B, S, H, hd, L->k, smax, past, stream);
}

// ops.linear at the decode steps' shapes (weight-only: these entries never quantize activations): the rule's skinny MFMA GEMM or weight-streaming
// GEMV; a preceding LlamaRMSNorm is fused into the GEMV or a launch of its own, as the rule says.
inline int lin_decode(const void* x, int64_t ldx, const void* rms_w, float eps, void* xn_scratch, const ull_linear* L, void* out, int64_t ldc,
                      const void* R, int64_t ldr, int64_t M, int flags, void* stream) {
    const ull_route::Route route = ull_route::route_of(M, L->n, L->k, ldw_of(L), L->format, ULL_AF_NONE, false, 0);
    const bool skinny = route.kind == ULL_ROUTE_SKINNY;
    if (!skinny && route.kind != ULL_ROUTE_GEMV) return ULL_ERR_SHAPE;
    if (bias_of(L)) flags |= ULL_EPI_BIAS;
    if (R) flags |= ULL_EPI_RESID;
    if (rms_w && route.rms_first) {
        TRY(FN(ull_rmsnorm_)(x, ldx, rms_w, xn_scratch, L->k, M, L->k, eps, stream));
        x = xn_scratch;
        ldx = L->k;
        rms_w = nullptr;
    }
    if (skinny) return gemm_skinny(x, ldx, L, out, ldc, R, ldr, M, flags, stream);
    if (rms_w) return gemv_rmsnorm(x, ldx, rms_w, eps, L, out, ldc, R, ldr, M, flags, stream);
    return gemv(x, ldx, L, out, ldc, R, ldr, M, flags, stream);
}

}  // namespace

extern "C" int FN(ull_llama_prefill_layers_)(const ull_llama_layer* layers, int64_t n_layers, const void* x_in, void* const* x_out, void* x_mid,
                                             void* xn, void* qkv, void* att, void* act, const void* rope_cos, const void* rope_sin,
                                             const void* key_mask, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t I, float eps, void* ws,
                                             int64_t ws_bytes, int64_t sk_min_k, const void* zeros, void* stream) {
    if (!layers || !x_in || !x_out || !x_mid || !xn || !qkv || !att || !act || !rope_cos || !rope_sin || !zeros || n_layers <= 0) return ULL_ERR_ARG;
    const int64_t D = H * hd, T = B * S;
    if (hd != 128 || T <= 16 || S <= 16 || S > 1024 || D % 64 || I % 64) return ULL_ERR_SHAPE;       // the fused-RoPE prefill form only
    const SK sk{ws, ws_bytes, sk_min_k};
    const float scale = 1.0f / sqrtf((float)hd);
    const char* q = (const char*)qkv;
    const void* x = x_in;
    for (int64_t l = 0; l < n_layers; ++l) {
        const ull_llama_layer& w = layers[l];
        if (w.qkv.n != 3 * D || w.qkv.k != D || w.o.n != D || w.o.k != D || w.gu.n != 2 * I || w.gu.k != D || w.down.n != D || w.down.k != I || !x_out[l] ||
            quantized(&w.qkv) || quantized(&w.o) || quantized(&w.gu) || quantized(&w.down))       // (a quantized model's prefill: the per-op path)
            return ULL_ERR_ARG;
        TRY(FN(ull_rmsnorm_)(x, D, w.ln1, xn, D, T, D, eps, stream));                                   // input_layernorm
        {                                                                                               // q|k|v projection + RoPE epilogue
            const Tiled t = tiled(&w.qkv, T, sk);
            TRY(FN(ull_gemm_qkv_rope_)(xn, D, t.w, t.ldw, qkv, 3 * D, T, 3 * D, D, rope_cos, rope_sin, 2 * D, hd, t.flags, t.ws, t.wsb, stream));
        }
        // causal attention, V read as rows of the fused q|k|v buffer (vt_len = 0)
        TRY(FN(ull_attention_)(q, S * 3 * D, hd, 3 * D, q + D * 2, S * 3 * D, hd, 3 * D, q + 2 * D * 2, S * 3 * D, hd, 3 * D, 0, att, S * D, hd, D, key_mask,
                               B, H, S, S, hd, 1, 1, scale, 1.0f, nullptr, nullptr, 0, 0, 0, zeros, stream));
        TRY(lin(att, D, &w.o, x_mid, D, x, D, T, 0, sk, stream));                                       // o_proj + residual
        TRY(FN(ull_rmsnorm_)(x_mid, D, w.ln2, xn, D, T, D, eps, stream));                               // post_attention_layernorm
        TRY(lin(xn, D, &w.gu, act, I, nullptr, 0, T, ULL_EPI_SWIGLU, sk, stream));                      // gate|up + SwiGLU
        TRY(lin(act, I, &w.down, x_out[l], D, x_mid, D, T, 0, sk, stream));                             // down_proj + residual
        x = x_out[l];
    }
    return ULL_OK;
}

namespace {

// The KV-cache formats of a decode step.  BfCache: the model-dtype K / V^T buffers per layer, appended to in place.  Kv8Cache (bf16 build):
// the fp8 cache (csrc/kv8.hip) -- per-layer codes and scales plus ONE bf16 staging window shared by the layers: the appender writes the
// step's keys into the window (pitch 128, first new key at past mod 64), ull_attention_kv8 reads the cached keys from the codes and the new
// ones from the window, then quantizes the new keys into the layer's cache.  The same launches per layer in both formats.
struct BfCache {
    void* const* k; void* const* vt;
};
inline bool cache_layer_ok(const BfCache& c, int64_t l) { return c.k[l] && c.vt[l]; }
inline bool cache_shape_ok(const BfCache& c, int64_t, int64_t) { return c.k && c.vt; }
inline int append_and_attend(const BfCache& c, int64_t l, const void* x, int64_t D, const void* ln1, float eps, const ull_linear* qkv, void* q, const void* cs,
                             const void* sn, void* att, const void* key_mask, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t smax, int64_t past,
                             float scale, const void* zeros, void* stream) {
    TRY(gemv_qkv_rope_append(x, D, ln1, eps, qkv, q, D, cs, sn, c.k[l], c.vt[l], B, S, H, hd, smax, past, stream));
    return FN(ull_attention_)(q, S * D, hd, D, c.k[l], H * smax * hd, smax * hd, hd, c.vt[l], H * hd * smax, hd * smax, smax, smax, att, S * D, hd, D,
                              key_mask, B, H, S, past + S, hd, 1, 1, scale, 1.0f, nullptr, nullptr, 0, 0, 0, zeros, stream);
}

#ifndef ULL_ELEM_F16
struct Kv8Cache {
    void* const* k8; void* const* vt8; void* const* ks; void* const* vs;
    void* k_stage; void* vt_stage;
};
inline bool cache_layer_ok(const Kv8Cache& c, int64_t l) { return c.k8[l] && c.vt8[l] && c.ks[l] && c.vs[l]; }
// the shapes ull_attention_kv8 takes (the model routes other calls through the dequantized per-op path)
inline bool cache_shape_ok(const Kv8Cache& c, int64_t S, int64_t past) {
    return c.k8 && c.vt8 && c.ks && c.vs && c.k_stage && c.vt_stage && S <= 16 && past + S > 64 && past + S <= 4096;
}
inline int append_and_attend(const Kv8Cache& c, int64_t l, const void* x, int64_t D, const void* ln1, float eps, const ull_linear* qkv, void* q, const void* cs,
                             const void* sn, void* att, const void* key_mask, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t smax, int64_t past,
                             float scale, const void* zeros, void* stream) {
    TRY(gemv_qkv_rope_append(x, D, ln1, eps, qkv, q, D, cs, sn, c.k_stage, c.vt_stage, B, S, H, hd, 128, past & 63, stream));
    return ull_attention_kv8_bf16(q, S * D, hd, D, c.k_stage, c.vt_stage, c.k8[l], c.vt8[l], c.ks[l], c.vs[l], smax, att, S * D, hd, D, key_mask, B, H, S,
                                  past + S, hd, scale, zeros, stream);
}
#endif  // !ULL_ELEM_F16

// The decode-step layer loop over either cache format.  Every layer is checked before anything is enqueued.
template <class Cache>
int llama_decode_layers(const ull_llama_layer* layers, int64_t n_layers, const void* x_in, void* const* x_out, void* x_mid, void* xn, void* q, void* att, void* act,
                        const void* rope_cos, const void* rope_sin, const void* key_mask, const Cache& cache, int64_t B, int64_t S, int64_t H,
                        int64_t hd, int64_t I, int64_t smax, int64_t past, float eps, const void* zeros, void* stream) {
    if (!layers || !x_in || !x_out || !x_mid || !xn || !q || !att || !act || !rope_cos || !rope_sin || !zeros || n_layers <= 0) return ULL_ERR_ARG;
    const int64_t D = H * hd, T = B * S;
    if (T <= 0 || past <= 0 || !ull_route::decode_step_fused(T, D, hd) || I <= 0 || I % 8 || past + S > smax) return ULL_ERR_SHAPE;
    if (!cache_shape_ok(cache, S, past)) return ULL_ERR_ARG;
    for (int64_t l = 0; l < n_layers; ++l) {
        const ull_llama_layer& w = layers[l];
        if (w.qkv.n != 3 * D || w.qkv.k != D || w.o.n != D || w.o.k != D || w.gu.n != 2 * I || w.gu.k != D || w.down.n != D || w.down.k != I)
            return ULL_ERR_SHAPE;
        for (const auto* L : {&w.qkv, &w.o, &w.gu, &w.down})
            if (!format_ok(L) || !has_weight(L) || !pitch_ok(L)) return ULL_ERR_ARG;
        if (!w.ln1 || !w.ln2 || !cache_layer_ok(cache, l) || !x_out[l]) return ULL_ERR_ARG;
    }
    const float scale = 1.0f / sqrtf((float)hd);
    const void* x = x_in;
    for (int64_t l = 0; l < n_layers; ++l) {
        const ull_llama_layer& w = layers[l];
        TRY(append_and_attend(cache, l, x, D, w.ln1, eps, &w.qkv, q, rope_cos, rope_sin, att, key_mask, B, S, H, hd, smax, past, scale, zeros, stream));
        TRY(lin_decode(att, D, nullptr, 0.f, xn, &w.o, x_mid, D, x, D, T, 0, stream));
        TRY(lin_decode(x_mid, D, w.ln2, eps, xn, &w.gu, act, I, nullptr, 0, T, ULL_EPI_SWIGLU, stream));
        TRY(lin_decode(act, I, nullptr, 0.f, xn, &w.down, x_out[l], D, x_mid, D, T, 0, stream));
        x = x_out[l];
    }
    return ULL_OK;
}

}  // namespace

extern "C" int FN(ull_llama_decode_layers_)(const ull_llama_layer* layers, int64_t n_layers, const void* x_in, void* const* x_out, void* x_mid,
                                            void* xn, void* q, void* att, void* act, const void* rope_cos, const void* rope_sin,
                                            const void* key_mask, void* const* k_cache, void* const* vt_cache, int64_t B, int64_t S, int64_t H,
                                            int64_t hd, int64_t I, int64_t smax, int64_t past, float eps, const void* zeros, void* stream) {
    return llama_decode_layers(layers, n_layers, x_in, x_out, x_mid, xn, q, att, act, rope_cos, rope_sin, key_mask, BfCache{k_cache, vt_cache}, B, S, H,
                               hd, I, smax, past, eps, zeros, stream);
}

#ifndef ULL_ELEM_F16
extern "C" int ull_llama_decode_layers_kv8_bf16(const ull_llama_layer* layers, int64_t n_layers, const void* x_in, void* const* x_out, void* x_mid,
                                                void* xn, void* q, void* att, void* act, const void* rope_cos, const void* rope_sin,
                                                const void* key_mask, void* const* k8, void* const* vt8, void* const* k_scale, void* const* vt_scale,
                                                void* k_stage, void* vt_stage, int64_t B, int64_t S, int64_t H, int64_t hd, int64_t I, int64_t smax,
                                                int64_t past, float eps, const void* zeros, void* stream) {
    return llama_decode_layers(layers, n_layers, x_in, x_out, x_mid, xn, q, att, act, rope_cos, rope_sin, key_mask,
                               Kv8Cache{k8, vt8, k_scale, vt_scale, k_stage, vt_stage}, B, S, H, hd, I, smax, past, eps, zeros, stream);
}

#endif  // !ULL_ELEM_F16

extern "C" int FN(ull_clip_layers_)(const ull_clip_layer* layers, int64_t n_layers, void* h, void* h_mid, void* y, void* qkv, void* att, void* f,
                                    int64_t n_img, int64_t S, int64_t H, int64_t hd, int64_t I, float eps, void* ws, int64_t ws_bytes,
                                    int64_t sk_min_k, const void* zeros, void* stream) {
    if (!layers || !h || !h_mid || !y || !qkv || !att || !f || !zeros || n_layers < 0) return ULL_ERR_ARG;
    const int64_t D = H * hd, T = n_img * S;
    if (hd != 64 || T <= 16 || S <= 16 || S > 704 || D % 64 || I % 64) return ULL_ERR_SHAPE;
    const SK sk{ws, ws_bytes, sk_min_k};
    const float scale = 1.0f / sqrtf((float)hd);
    const char* q = (const char*)qkv;
    for (int64_t l = 0; l < n_layers; ++l) {
        const ull_clip_layer& w = layers[l];
        if (w.qkv.n != 3 * D || w.qkv.k != D || w.out.n != D || w.out.k != D || w.fc1.n != I || w.fc1.k != D || w.fc2.n != D || w.fc2.k != I ||
            quantized(&w.qkv) || quantized(&w.out) || quantized(&w.fc1) || quantized(&w.fc2))
            return ULL_ERR_ARG;
        TRY(FN(ull_layernorm_)(h, D, w.ln1_w, w.ln1_b, y, D, T, D, eps, stream));
        TRY(lin(y, D, &w.qkv, qkv, 3 * D, nullptr, 0, T, 0, sk, stream));
        TRY(FN(ull_attention_)(q, S * 3 * D, hd, 3 * D, q + D * 2, S * 3 * D, hd, 3 * D, q + 2 * D * 2, S * 3 * D, hd, 3 * D, 0, att, S * D, hd, D, nullptr,
                               n_img, H, S, S, hd, 0, 1, scale, 1.0f, nullptr, nullptr, 0, 0, 0, zeros, stream));
        TRY(lin(att, D, &w.out, h_mid, D, h, D, T, 0, sk, stream));
        TRY(FN(ull_layernorm_)(h_mid, D, w.ln2_w, w.ln2_b, y, D, T, D, eps, stream));
        TRY(lin(y, D, &w.fc1, f, I, nullptr, 0, T, ULL_EPI_ACT_QUICK_GELU, sk, stream));
        TRY(lin(f, I, &w.fc2, h, D, h_mid, D, T, 0, sk, stream));
    }
    return ULL_OK;
}

extern "C" int FN(ull_sam_blocks_)(const ull_sam_block* blocks, int64_t n_blocks, void* x, void* x_mid, void* y, void* qkv, void* att, void* f,
                                   int64_t B, int64_t g, int64_t nH, int64_t hd, int64_t I, float eps, void* ws, int64_t ws_bytes, int64_t sk_min_k,
                                   const void* zeros, void* stream) {
    if (!blocks || !x || !x_mid || !y || !qkv || !att || !f || !zeros || n_blocks <= 0) return ULL_ERR_ARG;
    const int64_t C = nH * hd, T = B * g * g, S = g * g;
    if (hd != 80 || g != 64 || C % 64 || I % 64) return ULL_ERR_SHAPE;                                  // SAM ViT-H / L / B at 1024 x 1024
    const SK sk{ws, ws_bytes, sk_min_k};
    const float q_scale = 1.0f / sqrtf((float)hd);
    const char* q = (const char*)qkv;
    for (int64_t i = 0; i < n_blocks; ++i) {
        const ull_sam_block& w = blocks[i];
        if (w.qkv.n != 3 * C || w.qkv.k != C || !w.qkv.bias || w.proj.n != C || w.proj.k != C || w.lin1.n != I || w.lin1.k != C || w.lin2.n != C ||
            w.lin2.k != I || !w.rel_pos_h || !w.rel_pos_w || (w.window != 0 && w.window != 14) || quantized(&w.qkv) || quantized(&w.proj) || quantized(&w.lin1) ||
            quantized(&w.lin2))
            return ULL_ERR_ARG;
        TRY(FN(ull_layernorm_)(x, C, w.n1_w, w.n1_b, y, C, T, C, eps, stream));
        TRY(lin(y, C, &w.qkv, qkv, 3 * C, nullptr, 0, T, 0, sk, stream));
        if (w.window)          // 14 x 14 windows on image-order tokens; the padded positions' q|k|v = the qkv bias
            TRY(FN(ull_sam_window_attention_)(qkv, 3 * C, w.qkv.bias, w.rel_pos_h, w.rel_pos_w, att, C, B, g, g, nH, hd, w.window, q_scale, zeros, stream));
        else                   // global attention over the 64 x 64 grid, rel-pos tables built in the kernel (rel_mode 2), V rows read in place
            TRY(FN(ull_attention_)(q, S * 3 * C, hd, 3 * C, q + C * 2, S * 3 * C, hd, 3 * C, q + 2 * C * 2, S * 3 * C, hd, 3 * C, 0, att, S * C, hd, C,
                                   nullptr, B, nH, S, S, hd, 0, 0, 1.0f, q_scale, w.rel_pos_h, w.rel_pos_w, g, g, 2, zeros, stream));
        TRY(lin(att, C, &w.proj, x_mid, C, x, C, T, 0, sk, stream));
        TRY(FN(ull_layernorm_)(x_mid, C, w.n2_w, w.n2_b, y, C, T, C, eps, stream));
        TRY(lin(y, C, &w.lin1, f, I, nullptr, 0, T, ULL_EPI_ACT_GELU, sk, stream));
        TRY(lin(f, I, &w.lin2, x, C, x_mid, C, T, 0, sk, stream));
    }
    return ULL_OK;
}
