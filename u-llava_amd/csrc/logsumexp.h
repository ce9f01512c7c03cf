// The two reductions of a row's log-softmax as device functions: max_r over the row and sum_r = sum_i exp(float(x_i) - max_r), by one
// 1024-thread block, in a fixed order.  Shared by token_logprobs_kernel (logprobs.hip) and the beam step (beam.hip), so that
// float(x_j) - max_r - logf(sum_r) has the same bits wherever it is computed -- the way select.h shares greedy_pick.
#pragma once
#include "ull_common.h"
#include "select.h"

constexpr int LP_THREADS = 1024;

struct LpScratch {
    float f[16];
};

ULL_DEV float lp_block_max(float v, LpScratch& sc) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sc.f[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) t = fmaxf(t, sc.f[w]);
    return t;
}
ULL_DEV float lp_block_sum(float v, LpScratch& sc) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += sc.f[w];
    return t;
}

// row: V elements of dtype DT.  Called by all LP_THREADS threads of the block; m and s are valid in every thread.
// The sum gives every element to the same thread on either load path -- element i of the nfull whole chunks to thread (i / EPC) % 1024,
// element i of the tail behind them to thread (i - nfull * EPC) % 1024 -- and every thread adds its elements in increasing order, chunks
// before tail: the sum's bits depend on the row's values alone, not on where the row lies (a verify step's odd rows against the plain
// loop's aligned ones).  The maximum needs no such care.  The element-wise loops count in long: V + 1023 may pass 2^31.
template <int DT> ULL_DEV void lp_row_max_sum(const char* __restrict__ row, int V, LpScratch& sc, float& m_out, float& s_out) {
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2, EPC = 16 / ESZ;
    const int tid = threadIdx.x;
    const bool vec = ((uintptr_t)row & 15) == 0;
    const int nfull = V / EPC, nchunk = vec ? nfull : 0;

    // ---- 1. the maximum; q0 keeps the first round of chunks for step 2
    uint4 q0[4] = {};
    float m = -INFINITY;
    for (int c0 = tid; c0 < nchunk; c0 += 4 * LP_THREADS) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = c0 + u * LP_THREADS < nchunk ? *(const uint4*)(row + (long)(c0 + u * LP_THREADS) * 16) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 == tid) q0[u] = q[u];
            if (c0 + u * LP_THREADS < nchunk) {
                float f[EPC];
                unpack_chunk<DT>(q[u], f);
#pragma unroll
                for (int j = 0; j < EPC; ++j) m = fmaxf(m, f[j]);
            }
        }
    }
    for (long c = (vec ? (long)nfull * EPC : 0) + tid; c < V; c += LP_THREADS) m = fmaxf(m, load_dt<DT>(row, c));
    m = lp_block_max(m, sc);

    // ---- 2. the sum of exp(x - max)
    float s = 0.f;
    for (int c0 = tid; c0 < nchunk; c0 += 4 * LP_THREADS) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 == tid) q[u] = q0[u];
            else q[u] = c0 + u * LP_THREADS < nchunk ? *(const uint4*)(row + (long)(c0 + u * LP_THREADS) * 16) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u * LP_THREADS < nchunk) {
                float f[EPC];
                unpack_chunk<DT>(q[u], f);
#pragma unroll
                for (int j = 0; j < EPC; ++j) s += expf(f[j] - m);
            }
        }
    }
    if (!vec)
        for (int c = tid; c < nfull; c += LP_THREADS)
#pragma unroll
            for (int j = 0; j < EPC; ++j) s += expf(load_dt<DT>(row, (long)c * EPC + j) - m);
    for (long c = (long)nfull * EPC + tid; c < V; c += LP_THREADS) s += expf(load_dt<DT>(row, c) - m);
    s = lp_block_sum(s, sc);
    m_out = m;
    s_out = s;
}
