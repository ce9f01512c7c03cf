// What a continued generate() call needs beside the decode kernels: the prefix check of the ids against the ids a KV cache was filled with,
// and the copy of an fp8 cache's positions into buffers of another (or the same) capacity.  Byte and integer work, compiled once.
//
// ull_ids_common_prefix: one 256-thread block per row (the blocks stride over the rows, so any R fits).  The threads stride over the
// positions i = 0 .. n - 1 in ascending order; a thread stops at its first mismatch and the block takes the minimum over the threads
// through one LDS word (start value n).  The ids are only compared, never used as an address.
//
// ull_kv8_copy_positions: positions [0, n) of the K codes [B, H, smax, hd], the V^T codes [B, H, hd, smax] (key-permuted slots inside
// 32-key blocks, see kv8.hip), the K scales [B, H, smax] (by key) and the V scales [B, H, smax] (by slot), for up to 32 layers per launch.
// The whole 32-key blocks below n are contiguous runs in every one of the four arrays and move in 16-byte chunks (every run starts on a
// 16-byte boundary: smax is a multiple of 32 and the bases are checked); the keys of the last, partial block move one code / one scale at a
// time to their slots, so nothing at or beyond position n is written.  The bf16 staging window (k_stage / vt_stage) is NOT part of the
// state that travels: every forward call that uses it (layers.hip's append_and_attend in the coarse decode stack, the callers of
// KVCache._kv8_decode_buffers on the per-op path) writes the call's new keys into the window before ull_attention_kv8 reads them, and
// that kernel reads the window only at keys >= past (kv8_vfrag: `key >= past`, K rows likewise), i.e. at what the same call has just
// written.
#include "ull_common.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_MAX_GRID = 1 << 16;

__global__ __launch_bounds__(CP_THREADS) void ids_common_prefix_kernel(const int64_t* __restrict__ a, long lda, const int64_t* __restrict__ b, long ldb,
                                                                       long R, int n, int32_t* __restrict__ out) {
    __shared__ int first;
    const int tid = threadIdx.x;
    for (long r = blockIdx.x; r < R; r += gridDim.x) {             // (uniform over the block)
        if (tid == 0) first = n;
        __syncthreads();
        const int64_t* ra = a + r * lda;
        const int64_t* rb = b + r * ldb;
        for (int i = tid; i < n; i += CP_THREADS) {
            if (ra[i] != rb[i]) {
                atomicMin(&first, i);                              // (LDS; a thread's later mismatches are larger)
                break;
            }
        }
        __syncthreads();
        if (tid == 0) out[r] = first;
        __syncthreads();                                           // `first` is reset for the block's next row only after it was read
    }
}

constexpr int K8_MAX_LAYERS = 32;                                  // per launch: the pointers travel as kernel arguments

struct Kv8CopyPtrs {
    const char* s[4][K8_MAX_LAYERS];                               // 0: K codes, 1: V^T codes, 2: K scales, 3: V scales
    char* d[4][K8_MAX_LAYERS];
};

// V^T slot of key k inside its 32-key block (kv8.hip's kv8_slot)
ULL_DEV long cp_slot(long k) {
    const long w = k & 31;
    return (k & ~31L) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3);
}

// grid: x strides over the units of one (batch, head), y = batch * H + head, z = 4 * layer + array.
__global__ __launch_bounds__(CP_THREADS) void kv8_copy_positions_kernel(const Kv8CopyPtrs P, int hd, long ss, long ds, long n) {
    const int l = blockIdx.z >> 2, part = blockIdx.z & 3;
    const long bh = blockIdx.y;
    const long step = (long)gridDim.x * CP_THREADS, u0 = (long)blockIdx.x * CP_THREADS + threadIdx.x;
    const char* src = P.s[part][l];
    char* dst = P.d[part][l];
    const long nb = n & ~31L, rem = n - nb;                        // keys in whole 32-key blocks; keys of the partial block
    if (part == 0) {                                               // K codes: n rows of hd bytes, one run
        src += bh * ss * hd; dst += bh * ds * hd;
        const long bytes = n * hd, chunks = bytes >> 4;
        for (long u = u0; u < chunks; u += step) ((uint4*)dst)[u] = ((const uint4*)src)[u];
        for (long u = (chunks << 4) + u0; u < bytes; u += step) dst[u] = src[u];
    } else if (part == 2) {                                        // K scales: n floats, one run
        src += bh * ss * 4; dst += bh * ds * 4;
        const long chunks = n >> 2;
        for (long u = u0; u < chunks; u += step) ((uint4*)dst)[u] = ((const uint4*)src)[u];
        for (long u = (chunks << 2) + u0; u < n; u += step) ((float*)dst)[u] = ((const float*)src)[u];
    } else if (part == 1) {                                        // V^T codes: hd lines of nb bytes, then rem single slots per line
        src += bh * hd * ss; dst += bh * hd * ds;
        const long cpl = nb >> 4;
        for (long u = u0; u < hd * cpl; u += step) {
            const long d = u / cpl, c = u % cpl;
            ((uint4*)(dst + d * ds))[c] = ((const uint4*)(src + d * ss))[c];
        }
        for (long u = u0; u < hd * rem; u += step) {
            const long d = u / rem, s = cp_slot(nb + u % rem);     // nb <= s < nb + 32 <= both pitches
            dst[d * ds + s] = src[d * ss + s];
        }
    } else {                                                       // V scales: nb floats, then rem single slots
        src += bh * ss * 4; dst += bh * ds * 4;
        const long chunks = nb >> 2;
        for (long u = u0; u < chunks; u += step) ((uint4*)dst)[u] = ((const uint4*)src)[u];
        for (long u = u0; u < rem; u += step) {
            const long s = cp_slot(nb + u);
            ((float*)dst)[s] = ((const float*)src)[s];
        }
    }
}

}  // namespace

extern "C" int ull_ids_common_prefix(const void* ids_a, int64_t lda, const void* ids_b, int64_t ldb, int64_t R, int64_t n, void* out, void* stream) {
    if (R < 0 || n < 0 || n > 0x7fffffff || lda < 0 || ldb < 0 || (R > 0 && !out) || (R > 0 && n > 0 && (!ids_a || !ids_b))) return ULL_ERR_ARG;
    if (R > 1 && n > 0 && (lda < n || ldb < n)) return ULL_ERR_SHAPE;      // the rows would overlap
    if (R == 0) return ULL_OK;
    const unsigned grid = (unsigned)(R < CP_MAX_GRID ? R : CP_MAX_GRID);
    hipLaunchKernelGGL(ids_common_prefix_kernel, dim3(grid), dim3(CP_THREADS), 0, (hipStream_t)stream, (const int64_t*)ids_a, (long)lda,
                       (const int64_t*)ids_b, (long)ldb, (long)R, (int)n, (int32_t*)out);
    return ull_check_launch();
}

extern "C" int ull_kv8_copy_positions(const void* const* src_k8, const void* const* src_vt8, const void* const* src_k_scale,
                                      const void* const* src_vt_scale, void* const* dst_k8, void* const* dst_vt8, void* const* dst_k_scale,
                                      void* const* dst_vt_scale, int64_t n_layers, int64_t B, int64_t H, int64_t hd, int64_t src_smax, int64_t dst_smax,
                                      int64_t n, void* stream) {
    if (!src_k8 || !src_vt8 || !src_k_scale || !src_vt_scale || !dst_k8 || !dst_vt8 || !dst_k_scale || !dst_vt_scale || n_layers < 0 || B < 1 ||
        H < 1 || hd < 1 || hd > (1 << 20) || n < 0 || src_smax < 1 || dst_smax < 1)
        return ULL_ERR_ARG;
    if ((src_smax & 31) || (dst_smax & 31) || n > src_smax || n > dst_smax || B * H > 65535) return ULL_ERR_SHAPE;
    const void* const* srcs[4] = {src_k8, src_vt8, src_k_scale, src_vt_scale};
    void* const* dsts[4] = {dst_k8, dst_vt8, dst_k_scale, dst_vt_scale};
    for (int64_t l = 0; l < n_layers; ++l)
        for (int a = 0; a < 4; ++a) {
            if (!srcs[a][l] || !dsts[a][l] || srcs[a][l] == dsts[a][l]) return ULL_ERR_ARG;
            if (((uintptr_t)srcs[a][l] | (uintptr_t)dsts[a][l]) & 15) return ULL_ERR_SHAPE;
        }
    if (n == 0 || n_layers == 0) return ULL_OK;
    const long units = (n * hd + 15) / 16 + 32 * hd;               // the largest array's chunks, plus a partial block's single codes
    const unsigned gx = (unsigned)((units + CP_THREADS - 1) / CP_THREADS < 64 ? (units + CP_THREADS - 1) / CP_THREADS : 64);
    for (int64_t l0 = 0; l0 < n_layers; l0 += K8_MAX_LAYERS) {
        const int nl = (int)(n_layers - l0 < K8_MAX_LAYERS ? n_layers - l0 : K8_MAX_LAYERS);
        Kv8CopyPtrs P = {};
        for (int a = 0; a < 4; ++a)
            for (int l = 0; l < nl; ++l) {
                P.s[a][l] = (const char*)srcs[a][l0 + l];
                P.d[a][l] = (char*)dsts[a][l0 + l];
            }
        hipLaunchKernelGGL(kv8_copy_positions_kernel, dim3(gx, (unsigned)(B * H), (unsigned)(4 * nl)), dim3(CP_THREADS), 0, (hipStream_t)stream, P,
                           (int)hd, (long)src_smax, (long)dst_smax, (long)n);
        if (ull_check_launch() != ULL_OK) return ULL_ERR_LAUNCH;
    }
    return ULL_OK;
}
