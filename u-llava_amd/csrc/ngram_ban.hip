// HF's NoRepeatNGramLogitsProcessor on the device: out[r] = logits[r] bit for bit, except -inf at every token that would complete an n-gram
// the row already holds (`generation.no_repeat_ngram_banned_tokens`, which stays the definition).  The host path spells it seq.tolist(), a
// Python loop over every position of every row and one indexed store per row; here it is one launch that never leaves the device, so the
// fused decode loop can keep the ban.
//
// Compiled once; the dtype is a run-time code (ULL_DT_*) and only decides the element size and the bits of -inf: nothing is converted, so
// NaN payloads and infinities travel unchanged.  One 1024-thread block per row (the blocks stride over the rows, so any R fits):
//   1. copy the row: 16-byte chunks, four in flight per thread, where BOTH the source and the destination row are 16-byte aligned (the
//      source is `out.logits[:, -1]`: rows S*V elements apart, starting anywhere), the elements behind the last whole chunk one by one;
//      element by element otherwise;
//   2. a block barrier (the -inf stores of step 3 land on elements other threads copied);
//   3. the threads stride over the windows i = 0 .. cur_len - ngram; where ids[i .. i+ngram-2] equals the row's last ngram - 1 ids, the
//      id behind the window, t = ids[i+ngram-1], gets -inf -- if 0 <= t < V: no address is formed from an unchecked id.  Several threads
//      may store the same value to the same element.
// Nothing is staged in LDS: V has no limit.  The ids are read-only and only their first cur_len entries per row are touched.
#include "ull_common.h"

namespace {

constexpr int NB_THREADS = 1024;
constexpr int NB_MAX_GRID = 1 << 16;

template <typename E>    // E: uint16_t (bf16 / fp16) or uint32_t (fp32) -- the raw bits of one element
__global__ __launch_bounds__(NB_THREADS) void ngram_ban_kernel(const E* __restrict__ logits, long row_stride, long R, long V,
                                                               const int64_t* __restrict__ ids, long ids_ld, long cur_len, long ngram,
                                                               E* __restrict__ out, long out_ld, E neg_inf) {
    constexpr long EPC = 16 / sizeof(E);
    const int tid = threadIdx.x;
    for (long r = blockIdx.x; r < R; r += gridDim.x) {             // (every branch on r below is uniform over the block)
        const E* src = logits + r * row_stride;
        E* dst = out + r * out_ld;

        // ---- 1. the copy
        const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
        const long nchunk = vec ? V / EPC : 0;
        for (long c0 = tid; c0 < nchunk; c0 += 4 * NB_THREADS) {
            uint4 q[4];                                            // (a chunk past the end reads the last chunk again and is not stored)
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = ((const uint4*)src)[min(c0 + u * NB_THREADS, nchunk - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c0 + u * NB_THREADS < nchunk) ((uint4*)dst)[c0 + u * NB_THREADS] = q[u];
        }
        for (long c = nchunk * EPC + tid; c < V; c += NB_THREADS) dst[c] = src[c];

        // ---- 2. every element of the row is written before any -inf lands on it
        __syncthreads();

        // ---- 3. the ban.  cur_len + 1 < ngram: no window fits.  Window i reads ids[i .. i+ngram-1], i + ngram - 1 <= cur_len - 1, and the
        // row's tail ids[cur_len-ngram+1 .. cur_len-1], cur_len - ngram + 1 >= 0: every index is inside the first cur_len entries.
        if (cur_len + 1 < ngram) continue;
        const int64_t* row = ids + r * ids_ld;
        const int64_t* tail = row + (cur_len - ngram + 1);
        for (long i = tid; i <= cur_len - ngram; i += NB_THREADS) {
            bool same = true;
            for (long j = 0; same && j < ngram - 1; ++j) same = row[i + j] == tail[j];
            if (!same) continue;
            const int64_t t = row[i + ngram - 1];
            if (t >= 0 && t < (int64_t)V) dst[t] = neg_inf;
        }
        // (the next row of this block is another row of `out`: no barrier is needed between rows)
    }
}

template <typename E>
int launch_ngram_ban(const void* logits, int64_t row_stride, int64_t R, int64_t V, const void* ids, int64_t ids_ld, int64_t cur_len, int64_t ngram,
                     void* out, int64_t out_ld, E neg_inf, hipStream_t st) {
    const unsigned grid = (unsigned)(R < NB_MAX_GRID ? R : NB_MAX_GRID);
    hipLaunchKernelGGL(ngram_ban_kernel<E>, dim3(grid), dim3(NB_THREADS), 0, st, (const E*)logits, (long)row_stride, (long)R, (long)V,
                       (const int64_t*)ids, (long)ids_ld, (long)cur_len, (long)ngram, (E*)out, (long)out_ld, neg_inf);
    return ull_check_launch();
}

}  // namespace

extern "C" int ull_ngram_ban(const void* logits, int logits_dtype, int64_t row_stride, int64_t R, int64_t V, const void* ids, int64_t ids_ld,
                             int64_t cur_len, int64_t ngram, void* out, int64_t out_ld, void* stream) {
    if (!logits || (!ids && cur_len > 0) || !out || R < 0 || V < 1 || ngram < 1 || cur_len < 0 || logits_dtype < 0 || logits_dtype > 2 ||
        row_stride < 0 || ids_ld < 0)
        return ULL_ERR_ARG;
    if (out_ld < V) return ULL_ERR_SHAPE;                          // the rows of `out` would overlap
    if (R == 0) return ULL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == ULL_DT_F32)
        return launch_ngram_ban<uint32_t>(logits, row_stride, R, V, ids, ids_ld, cur_len, ngram, out, out_ld, 0xFF800000u, st);
    return launch_ngram_ban<uint16_t>(logits, row_stride, R, V, ids, ids_ld, cur_len, ngram, out, out_ld,
                                      (uint16_t)(logits_dtype == ULL_DT_BF16 ? 0xFF80 : 0xFC00), st);
}
