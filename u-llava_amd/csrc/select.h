// The greedy selection rule of a decoding step as a device function: one 1024-thread block picks argmax(row) with the lowest index on ties
// (torch.argmax).  Shared by greedy_step_kernel (vision.hip, both 16-bit builds), greedy_step_f32_kernel (f32.hip) and the speculative
// step's spec_pick_kernel (sampling.hip), so that every path that says "the greedy token" runs the same code.
#pragma once
#include "ull_common.h"

template <int DT> ULL_DEV void unpack_chunk(const uint4& q, float* f) {       // 16 bytes = 4 fp32 or 8 16-bit elements
    if constexpr (DT == ULL_DT_F32) {
        f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y); f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
    } else {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (DT == ULL_DT_BF16) { f[2 * j] = __uint_as_float(w[j] << 16); f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u); }
            else { f[2 * j] = f16_bits_to_f32((uint16_t)(w[j] & 0xffffu)); f[2 * j + 1] = f16_bits_to_f32((uint16_t)(w[j] >> 16)); }
        }
    }
}

// row: V elements of dtype DT (ULL_DT_*); bv / bi: 16 words of LDS each.  Called by all 1024 threads of the block; the result is valid in
// thread 0 only.  A row of NaNs gives index 0 (torch returns the first NaN).
// 16-byte chunks, four of them in flight per thread (a 32 064-entry bf16 row is 4 008 chunks: one round of 1024 threads); the scalar form
// of this loop -- 125 dependent 2-byte loads per thread -- took 39 us per token
template <int DT> ULL_DEV int greedy_pick(const void* __restrict__ rowp, int V, float* bv, int* bi) {
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2, EPC = 16 / ESZ;
    const char* row = (const char*)rowp;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    const int nchunk = (((uintptr_t)row & 15) == 0) ? V / EPC : 0;
    for (int c0 = threadIdx.x; c0 < nchunk; c0 += 4 * 1024) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = c0 + u * 1024 < nchunk ? *(const uint4*)(row + (long)(c0 + u * 1024) * 16) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u * 1024 < nchunk) {
                float f[EPC];
                unpack_chunk<DT>(q[u], f);
#pragma unroll
                for (int j = 0; j < EPC; ++j)
                    if (f[j] > best) { best = f[j]; idx = (c0 + u * 1024) * EPC + j; }    // increasing index per thread: the first maximum stays
            }
        }
    }
    for (int c = nchunk * EPC + threadIdx.x; c < V; c += 1024) {
        const float v = load_dt<DT>(row, c);
        if (v > best || (v == best && c < idx)) { best = v; idx = c; }
    }
    if (idx == 0x7fffffff) idx = threadIdx.x < V ? threadIdx.x : 0;   // a row of NaNs: any valid index
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 16; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    return idx;
}
