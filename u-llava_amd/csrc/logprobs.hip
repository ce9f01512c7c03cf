// The log-probability of one chosen token per row of logits: out[r] = log_softmax(float(logits[r]))[ids[r]], the number HF users take from
// `output_scores` + `compute_transition_scores`.  torch spells it log_softmax(logits.float(), -1).gather(...): an fp32 [R, V] tensor and half
// a dozen launches; here it is one launch that reads the row and writes four bytes per row.
//
// Compiled once; the logits' dtype is a run-time code (ULL_DT_*).  One 1024-thread block per row (the blocks stride over the rows, so any R fits):
//   1. max_r over the row (16-byte chunks, four in flight per thread, when the row base is 16-byte aligned; element-wise otherwise);
//   2. sum_r = sum_i exp(float(logit_i) - max_r), on the same chunks: the first round of them (4096 chunks: a 32 064-entry 16-bit row) is still
//      in registers, later rounds are read again.  The element-wise path gives every thread the elements the chunk path gives it, in the
//      same order, so a row's result does not depend on its alignment;
//   3. out = float(logit[id]) - max_r - log(sum_r), all in fp32.
// A row whose id is outside [0, V) (-100, the loss's ignore index, included) or whose row_mask is 0 writes 0.0f and reads no logit.
// -inf entries add exp(-inf) = 0; a NaN entry, or a maximum of -inf / +inf (x - max = NaN), makes the sum and so the result NaN, as
// torch.log_softmax does.  Both reductions run in a fixed order (xor tree inside a wave, the sixteen wave partials left to right; no
// floating-point atomics): the same inputs give the same bits on every run.
#include "ull_common.h"
#include "select.h"
#include "logsumexp.h"

namespace {

constexpr int LP_MAX_GRID = 1 << 16;

template <int DT>
__global__ __launch_bounds__(LP_THREADS) void token_logprobs_kernel(const void* __restrict__ logits, long row_stride, long R, int V,
                                                                    const int64_t* __restrict__ ids, long ids_stride,
                                                                    const int32_t* __restrict__ row_mask, float* __restrict__ out, long out_stride) {
    __shared__ LpScratch sc;
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2;
    const int tid = threadIdx.x;
    for (long r = blockIdx.x; r < R; r += gridDim.x) {             // (every branch below is uniform over the block)
        const int64_t id = ids[r * ids_stride];
        if (id < 0 || id >= (int64_t)V || (row_mask && row_mask[r] == 0)) {
            if (tid == 0) out[r * out_stride] = 0.f;
            continue;
        }
        const char* row = (const char*)logits + r * row_stride * ESZ;
        float m, s;
        lp_row_max_sum<DT>(row, V, sc, m, s);              // (logsumexp.h: the beam step takes the same two numbers)

        // ---- 3. the chosen token's entry (id was checked against [0, V) above)
        if (tid == 0) out[r * out_stride] = load_dt<DT>(row, (long)id) - m - logf(s);      // (the next row's reductions start with a barrier)
    }
}

template <int DT>
int launch_token_logprobs(const void* logits, int64_t row_stride, int64_t R, int64_t V, const void* ids, int64_t ids_stride, const void* row_mask,
                          void* out, int64_t out_stride, hipStream_t st) {
    const unsigned grid = (unsigned)(R < LP_MAX_GRID ? R : LP_MAX_GRID);
    hipLaunchKernelGGL(token_logprobs_kernel<DT>, dim3(grid), dim3(LP_THREADS), 0, st, logits, (long)row_stride, (long)R, (int)V, (const int64_t*)ids,
                       (long)ids_stride, (const int32_t*)row_mask, (float*)out, (long)out_stride);
    return ull_check_launch();
}

}  // namespace

extern "C" int ull_token_logprobs(const void* logits, int logits_dtype, int64_t row_stride, int64_t R, int64_t V, const void* ids, int64_t ids_stride,
                                  const void* row_mask, void* out, int64_t out_stride, void* stream) {
    if (!logits || !ids || !out || R < 0 || V <= 0 || V > 0x7fffffff || logits_dtype < 0 || logits_dtype > 2 || row_stride < 0 || ids_stride < 0 ||
        out_stride < 0 || (R > 1 && out_stride == 0))
        return ULL_ERR_ARG;
    if (R == 0) return ULL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == ULL_DT_BF16) return launch_token_logprobs<ULL_DT_BF16>(logits, row_stride, R, V, ids, ids_stride, row_mask, out, out_stride, st);
    if (logits_dtype == ULL_DT_F16) return launch_token_logprobs<ULL_DT_F16>(logits, row_stride, R, V, ids, ids_stride, row_mask, out, out_stride, st);
    return launch_token_logprobs<ULL_DT_F32>(logits, row_stride, R, V, ids, ids_stride, row_mask, out, out_stride, st);
}
