// The Linear dispatch rule: which kernel a Linear x [M, K] @ w.T (w [N, K], row pitch ldw) takes, what becomes of a LlamaRMSNorm in front of it,
// how the tiled GEMM runs it, and when a decode step takes the fused q|k|v + RoPE + cache-append GEMV.  This is the ONE definition: the kernels'
// launchers (gemv.hip, gemm.hip), the coarse entries (layers.hip) and -- through ull_linear_route / ull_gemm_plan / ull_decode_step_fused
// (linear_route.hip) -- u-llava_amd/ops.py and modeling_core.py all read it, so the coarse entries and the per-op path cannot disagree on a shape.
// Host-only, plain C++17.
#ifndef ULL_LINEAR_ROUTE_H
#define ULL_LINEAR_ROUTE_H
#include <stdint.h>

#include "../../include/ullava_hip.h"

namespace ull_route {

constexpr int64_t GEMV_MAX_M = 4;                      // rows the weight-streaming GEMV takes (decode steps; no padding, no MFMA)
constexpr int64_t GEMV_STAGE_BYTES = 32 * 1024;        // the GEMV stages (and, asked to, RMS-normalises) its M x K 16-bit activations in this much LDS
constexpr int64_t SKINNY_MIN_M = 3, SKINNY_MAX_M = 16; // batched decode steps on the matrix cores: the GEMV is FMA-bound from M = 4 on and measured
                                                       // slower from M = 3 on (decode step at batch 3: 4.47 vs 4.24 ms; at batch 2 it wins, 4.00 vs 4.08)
constexpr int64_t SKINNY_K_STEP = 32;                  // one 16x16x32 MFMA
constexpr int64_t LARGE_WEIGHT = (int64_t)1 << 22;     // N * K of a LLaMA-sized weight (8 MB of 16-bit elements): smaller ones stay on the GEMV / tiled GEMM
constexpr int64_t BIG_MIN_M = 1024, BIG_MIN_N = 512, BIG_MIN_K = 128;      // the 256 x 256 GEMM kernel (at least two K-steps of 64)
constexpr int64_t SPLIT_K_MIN_K = 1024, SPLIT_K_MIN_M = 128, SPLIT_K_MAX_TILES = 256;     // small-M split-K: a long K, few 128 x 128 tiles

struct Route {
    int kind;            // ULL_ROUTE_*
    bool rms_first;      // a requested RMSNorm is a launch of its own ahead of the Linear (false: the route's kernel fuses it)
};

// The GEMV's LDS staging holds the activations; a fused RMSNorm needs it.
constexpr bool gemv_stages(int64_t M, int64_t K) { return M * K * 2 <= GEMV_STAGE_BYTES; }

// wfmt: ULL_WF_*; afmt: ULL_AF_*; a_decode: the ULL_AF_* code of the activations at the batched decode shapes (0: none); tune: the
// ULL_GEMM_TUNE_* bits of the call (a forced GEMM form keeps the Linear off the skinny kernels; the GEMV does not read it).
// An activation format on the weight format it pairs with (fp8 + per-token fp8, mxfp4 + mxfp8 or mxfp4; any other pair is weight-only) quantizes the
// activations wherever the weight-only rule says GEMM.  a_decode == ULL_AF_FP8 on fp8 weights with afmt == ULL_AF_FP8 adds A8W8_SKINNY ahead of
// everything else: the skinny size rule, starting above the rows the fused q|k|v + RoPE + cache-append GEMV takes and extended to that kernel's
// 32 rows (so at 17 .. 32 rows it replaces A8W8), with K a whole number of 128-code K-tiles; it fuses the RMSNorm into its row quantization.
// a_decode == ULL_AF_MXFP8 on mxfp4 weights, whatever afmt is, adds W4A8_SKINNY the same way (at 17 .. 32 rows it replaces W4A8 / W4A4 / the
// dequantizing GEMM); it acts on no other weight format, and ULL_AF_FP8 acts on no mxfp4 weight.
constexpr Route route_of(int64_t M, int64_t N, int64_t K, int64_t ldw, int wfmt, int afmt, int a_decode, int tune) {
    const int a8 = wfmt == ULL_WF_FP8 && afmt == ULL_AF_FP8     ? ULL_ROUTE_A8W8
                   : wfmt == ULL_WF_MXFP4 && afmt == ULL_AF_MXFP8 ? ULL_ROUTE_W4A8
                   : wfmt == ULL_WF_MXFP4 && afmt == ULL_AF_MXFP4 ? ULL_ROUTE_W4A4
                                                                  : ULL_ROUTE_GEMM;
    const bool streams_large_weight = N * K >= LARGE_WEIGHT && ldw % 8 == 0 && tune == 0;
    if (a8 == ULL_ROUTE_A8W8 && a_decode == ULL_AF_FP8 && M > GEMV_MAX_M && M <= ULL_A8W8_SKINNY_MAX_M && K % ULL_A8W8_BK == 0 &&
        streams_large_weight)
        return {ULL_ROUTE_A8W8_SKINNY, false};
    if (wfmt == ULL_WF_MXFP4 && a_decode == ULL_AF_MXFP8 && M > GEMV_MAX_M && M <= ULL_W4A8_SKINNY_MAX_M && K % ULL_A8W8_BK == 0 &&
        streams_large_weight)
        return {ULL_ROUTE_W4A8_SKINNY, false};
    if (M >= SKINNY_MIN_M && M <= SKINNY_MAX_M && K % SKINNY_K_STEP == 0 && streams_large_weight) return {ULL_ROUTE_SKINNY, true};
    if (M <= GEMV_MAX_M && K % 8 == 0) return {ULL_ROUTE_GEMV, !gemv_stages(M, K)};
    return {a8, true};
}

// The tiled GEMM takes its 256 x 256 kernel and the weight's tile-major copy where there is one.
constexpr bool is_big(int64_t M, int64_t N, int64_t K) { return M >= BIG_MIN_M && N >= BIG_MIN_N && K >= BIG_MIN_K; }

// Whether the tiled GEMM gets a workspace to split K into: the stream-K tail of a big one from K >= min_k on (min_k < 0: never), or -- small_m:
// the kernel has the split; small_m_split_k: the opt-in latency mode is on -- the split-K of a small-M one against a large weight (single-image
// prefill: o_proj / down_proj, CLIP's fc2: 376 -> 256 us per LLaMA layer at M = 323).
constexpr bool gemm_split(bool big, int64_t M, int64_t N, int64_t K, int64_t min_k, bool small_m, bool small_m_split_k) {
    if (min_k < 0) return false;
    if (big) return K >= min_k;
    return small_m && small_m_split_k && K >= SPLIT_K_MIN_K && M >= SPLIT_K_MIN_M && N * K >= LARGE_WEIGHT &&
           ((M + 127) / 128) * ((N + 127) / 128) <= SPLIT_K_MAX_TILES;
}

// A decode step of T = B * S tokens at width D = H * hd runs RoPE and the cache append in the q|k|v GEMV's epilogue: GEMV rows, rotation pairs,
// 16-byte loads, and the T x D activations in the GEMV's staging (LLaMA-7B at T = 4 is exactly the limit).
constexpr bool decode_step_fused(int64_t T, int64_t D, int64_t hd) { return T <= GEMV_MAX_M && hd % 2 == 0 && D % 8 == 0 && gemv_stages(T, D); }

}  // namespace ull_route
#endif
