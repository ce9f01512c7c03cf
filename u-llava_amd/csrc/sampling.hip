// One SAMPLED decoding step of HF `generate` (GenerationMixin._sample: TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on
// fp32 scores, softmax, torch.multinomial) with the bookkeeping of greedy_step_kernel (vision.hip), in one launch per token.
//
// reference: the callers of the inherited `generate` all sample (inference_ullava_core.py:73-80 do_sample=True, temperature=0.2;
// models/ullava.py:350-361 evaluate; top_k = 50 from GenerationConfig).  Host form: modeling_core.sampling_probs + torch.multinomial,
// some twenty torch launches and a device -> host read per token.
//
// Compiled once; the logits' dtype is a run-time code (ULL_DT_*).  One 1024-thread block per batch row:
//   1. the row is read once (16-byte chunks, four in flight per thread), s_i = float(logit_i) / temperature (IEEE division) is turned into
//      an order-preserving 32-bit key and staged in LDS (V = 32 064: 125.3 KiB);
//   2. top-k: the key of the k-th largest by radix select (12 + 10 + 10 bits, integer histograms in LDS); survivors are key >= that key,
//      so ties with the threshold stay (the host's `scores < kth`);
//   3. top-p: survivors are removed in ascending order while their cumulative softmax is <= 1 - top_p, the largest is kept.
//      Up to SS_CAP survivors (HF's top_k = 50: a few dozen) are compacted into LDS, ranked by (key, index) and scanned;
//      more (top-k off) are handled on the whole row by a bit-wise search for the boundary key on the probability mass below it;
//   4. token = argmax over the kept i of exp(s_i - max) / noise_i, the lowest index on exact ties: torch.multinomial(probs, 1) is
//      argmax(probs / exponential noise), and the common factor 1 / sum does not move an argmax;
//   5. pad fill / EOS / alive bookkeeping as greedy_step_kernel.
// Every sum is taken in a fixed order (no floating-point atomics): the same inputs give the same token on every run.
#include "ull_common.h"
#include "select.h"

namespace {

constexpr int SS_THREADS = 1024;
constexpr int SS_MAXPT = 36;                       // elements per thread (element i belongs to thread i % 1024)
constexpr int SS_HIST = 4096;                      // histogram words of the first radix pass; also the four SS_CAP-word lists of the compact path
constexpr int SS_CAP = 1024;                       // survivors the compact path takes
constexpr int SS_STATIC = 1024;                    // static LDS of the kernel is below this
constexpr int SS_MAX_V = (160 * 1024 - SS_STATIC - SS_HIST * 4) / 4;      // 36 608
static_assert(SS_MAX_V <= SS_THREADS * SS_MAXPT, "a thread holds SS_MAXPT elements");
static_assert(SS_MAX_V == ULL_SAMPLE_MAX_V, "include/ullava_hip.h names the limit");

ULL_DEV uint32_t f2key(float s) {                  // increasing in s; -0.0 and +0.0 share a key, as they compare equal
    if (s == 0.f) s = 0.f;
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ULL_DEV float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct Scratch {
    float f[16];
    int i[16];
    uint32_t u[16];
    uint32_t sel_digit, sel_rem;
    int count;
};

// sums in a fixed order: xor tree inside a wave, the sixteen wave sums left to right
ULL_DEV float block_sum(float v, Scratch& sc) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += sc.f[w];
    return t;
}
ULL_DEV uint32_t block_max_u(uint32_t v, Scratch& sc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc.u[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t = sc.u[w] > t ? sc.u[w] : t;
    return t;
}
// exclusive prefix over the threads in thread order, and the total
ULL_DEV int block_scan_i(int v, Scratch& sc, int& total) {
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(inc, o, 64); if ((int)(threadIdx.x & 63) >= o) inc += x; }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) sc.i[threadIdx.x >> 6] = inc;
    __syncthreads();
    int base = 0, t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { if (w < (int)(threadIdx.x >> 6)) base += sc.i[w]; t += sc.i[w]; }
    total = t;
    return base + inc - v;
}
ULL_DEV float block_scan_f(float v, Scratch& sc, float& total) {      // INCLUSIVE prefix (fixed order) and the total
    float inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float x = __shfl_up(inc, o, 64); if ((int)(threadIdx.x & 63) >= o) inc += x; }
    __syncthreads();
    if ((threadIdx.x & 63) == 63) sc.f[threadIdx.x >> 6] = inc;
    __syncthreads();
    float base = 0.f, t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) { if (w == (int)(threadIdx.x >> 6)) base = t; t += sc.f[w]; }
    total = t;
    return base + inc;
}
// the largest value, the lowest index among equal ones; idx 0x7fffffff = no candidate
ULL_DEV int block_argmax(float best, int idx, Scratch& sc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sc.f[threadIdx.x >> 6] = best; sc.i[threadIdx.x >> 6] = idx; }
    __syncthreads();
    best = sc.f[0]; idx = sc.i[0];
#pragma unroll
    for (int w = 1; w < 16; ++w)
        if (sc.f[w] > best || (sc.f[w] == best && sc.i[w] < idx)) { best = sc.f[w]; idx = sc.i[w]; }
    return idx;
}

// The sampled selection rule (steps 1-4 above) for one row, by one SS_THREADS block: `row` the logits of the row, nz its noise, lds the block's
// dynamic LDS ([V] keys + SS_HIST words).  Every thread returns the token index (outside [0, V) only for a row of NaNs).  Shared by
// sample_step_kernel and the speculative step's spec_pick_kernel.
template <int DT>
ULL_DEV int sample_pick(const char* __restrict__ row, int V, const float* __restrict__ nz, float temperature, int top_k, float top_p,
                        uint32_t* lds, Scratch& sc) {
    uint32_t* keys = lds;                              // [V]
    uint32_t* hist = lds + ((V + 3) & ~3);             // [SS_HIST]
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2, EPC = 16 / ESZ;
    const int tid = threadIdx.x;

    // ---- 1. stage the row as keys of s = logit / temperature
    uint32_t kmax = 0;
    const int nchunk = (((uintptr_t)row & 15) == 0) ? V / EPC : 0;
    for (int c0 = tid; c0 < nchunk; c0 += 4 * SS_THREADS) {
        uint4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = c0 + u * SS_THREADS < nchunk ? *(const uint4*)(row + (long)(c0 + u * SS_THREADS) * 16) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u * SS_THREADS < nchunk) {
                float f[EPC];
                unpack_chunk<DT>(q[u], f);
                uint32_t k[EPC];
#pragma unroll
                for (int j = 0; j < EPC; ++j) { k[j] = f2key(__fdiv_rn(f[j], temperature)); kmax = k[j] > kmax ? k[j] : kmax; }
                uint32_t* d = keys + (c0 + u * SS_THREADS) * EPC;
                *(uint4*)d = make_uint4(k[0], k[1], k[2], k[3]);
                if constexpr (EPC == 8) *(uint4*)(d + 4) = make_uint4(k[4], k[5], k[6], k[7]);
            }
        }
    }
    for (int c = nchunk * EPC + tid; c < V; c += SS_THREADS) {
        const uint32_t k = f2key(__fdiv_rn(load_dt<DT>(row, c), temperature));
        keys[c] = k;
        kmax = k > kmax ? k : kmax;
    }
    kmax = block_max_u(kmax, sc);                      // (its barriers also publish the keys)
    const float smax = key2f(kmax);
    const bool nucleus = top_p < 1.0f;
    const float p_cut = (float)(1.0 - (double)top_p);  // remove while cumulative <= p_cut

    // ---- 2. top-k: thr = key of the k-th largest
    uint32_t thr = 0;
    const bool topk = top_k > 0 && top_k < V;
    if (topk) {
        uint32_t prefix = 0, mask = 0;
        uint32_t rem = (uint32_t)top_k;
#pragma unroll 1
        for (int pass = 0; pass < 3; ++pass) {
            const int bits = pass == 0 ? 12 : 10, shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
            const int nb = 1 << bits, per = nb / SS_THREADS;
            for (int i = tid; i < nb; i += SS_THREADS) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += SS_THREADS) {
                const uint32_t k = keys[i];
                if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & (nb - 1)], 1u);
            }
            __syncthreads();
            // thread t owns the buckets nb-1 - (t*per + q): a prefix over the threads counts the keys in higher buckets
            int mine = 0;
            for (int q = 0; q < per; ++q) mine += (int)hist[nb - 1 - (tid * per + q)];
            int total;
            int above = block_scan_i(mine, sc, total);
            for (int q = 0; q < per; ++q) {
                const int d = nb - 1 - (tid * per + q), c = (int)hist[d];
                if ((uint32_t)above < rem && rem <= (uint32_t)(above + c)) { sc.sel_digit = (uint32_t)d; sc.sel_rem = rem - (uint32_t)above; }
                above += c;
            }
            __syncthreads();
            prefix |= sc.sel_digit << shift;
            mask |= (uint32_t)(nb - 1) << shift;
            rem = sc.sel_rem;
            __syncthreads();
        }
        thr = prefix;
    }

    // ---- 3a. few survivors: compact them
    uint32_t* ck = hist;                               // key
    uint32_t* ci = hist + SS_CAP;                      // index
    float* ce = (float*)(hist + 2 * SS_CAP);           // exp(s - max) in ascending (key, index) order
    uint32_t* cr = hist + 3 * SS_CAP;                  // removed, by rank
    int n_surv = V;
    if (topk) {
        if (tid == 0) sc.count = 0;
        __syncthreads();
        for (int i = tid; i < V; i += SS_THREADS) {
            const uint32_t k = keys[i];
            if (k >= thr) {
                const int slot = atomicAdd(&sc.count, 1);         // slot order varies from run to run; nothing below depends on it
                if (slot < SS_CAP) { ck[slot] = k; ci[slot] = (uint32_t)i; }
            }
        }
        __syncthreads();
        n_surv = sc.count;
    }

    float best = -1.f;
    int idx = 0x7fffffff;
    if (topk && n_surv <= SS_CAP) {                   // (top-k off: nothing was compacted, whatever V is)
        const bool have = tid < n_surv;
        const uint32_t k = have ? ck[tid] : 0u;
        const int i = have ? (int)ci[tid] : 0;
        const float e = have ? expf(key2f(k) - smax) : 0.f;
        bool kept = have;
        if (nucleus) {
            int rank = 0;
            if (have)
                for (int j = 0; j < n_surv; ++j) {
                    const uint32_t kj = ck[j], ij = ci[j];
                    rank += (kj < k || (kj == k && ij < (uint32_t)i)) ? 1 : 0;
                }
            if (have) ce[rank] = e;
            __syncthreads();
            float total;
            const float cum = block_scan_f(have ? ce[tid] : 0.f, sc, total);
            if (have) cr[tid] = (tid != n_surv - 1 && __fdiv_rn(cum, total) <= p_cut) ? 1u : 0u;
            __syncthreads();
            kept = have && !cr[rank];
        }
        if (kept) { best = __fdiv_rn(e, nz[i]); idx = i; }
    } else {
        // ---- 3b. the whole row (top-k off, or more than SS_CAP survivors)
        float er[SS_MAXPT];
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < SS_MAXPT; ++j) {
            const int i = tid + j * SS_THREADS;
            er[j] = -1.f;                              // < 0: not a candidate
            if (i < V) {
                const uint32_t k = keys[i];
                if (k >= thr) { er[j] = expf(key2f(k) - smax); part += er[j]; }
            }
        }
        if (nucleus) {
            const float total = block_sum(part, sc);
            // u = the largest key with mass(key < u) / total <= p_cut: every key below u is removed, every key above it stays
            uint32_t u = 0;
            float m_u = 0.f;
#pragma unroll 1
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = u | (1u << bit);
                float m = 0.f;
#pragma unroll
                for (int j = 0; j < SS_MAXPT; ++j) {
                    const int i = tid + j * SS_THREADS;
                    if (i < V && er[j] >= 0.f && keys[i] < cand) m += er[j];
                }
                m = block_sum(m, sc);
                if (cand <= kmax && __fdiv_rn(m, total) <= p_cut) { u = cand; m_u = m; }      // u <= kmax: the largest key stays
            }
            // the keys equal to u, in thread order then element order: the j-th of them goes while (m_u + j * e_u) / total <= p_cut
            int mine = 0;
#pragma unroll
            for (int j = 0; j < SS_MAXPT; ++j) {
                const int i = tid + j * SS_THREADS;
                if (i < V && er[j] >= 0.f && keys[i] == u) ++mine;
            }
            int n_tie;
            int ord = block_scan_i(mine, sc, n_tie);
            const float e_u = expf(key2f(u) - smax);
#pragma unroll
            for (int j = 0; j < SS_MAXPT; ++j) {
                const int i = tid + j * SS_THREADS;
                if (i < V && er[j] >= 0.f) {
                    const uint32_t k = keys[i];
                    if (k < u) er[j] = -1.f;
                    else if (k == u) {
                        ++ord;
                        const bool last = u == kmax && ord == n_tie;          // min_tokens_to_keep = 1
                        if (!last && __fdiv_rn(m_u + (float)ord * e_u, total) <= p_cut) er[j] = -1.f;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < SS_MAXPT; ++j) {
            const int i = tid + j * SS_THREADS;
            if (i < V && er[j] >= 0.f) {
                const float r = __fdiv_rn(er[j], nz[i]);
                if (r > best) { best = r; idx = i; }   // increasing index per thread: the first maximum stays
            }
        }
    }

    // ---- 4. the race
    return block_argmax(best, idx, sc);
}

template <int DT>
__global__ __launch_bounds__(SS_THREADS) void sample_step_kernel(const void* __restrict__ logits, long row_stride, int V, const float* __restrict__ noise,
                                                                 float temperature, int top_k, float top_p, int32_t* __restrict__ unfinished,
                                                                 const int64_t* __restrict__ eos, int n_eos, long pad, int has_pad,
                                                                 int64_t* __restrict__ seq, long seq_ld, int pos, int32_t* __restrict__ alive) {
    extern __shared__ uint32_t lds[];
    __shared__ Scratch sc;
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2;
    const int b = blockIdx.x;
    int idx = sample_pick<DT>((const char*)logits + (long)b * row_stride * ESZ, V, noise + (long)b * V, temperature, top_k, top_p, lds, sc);
    // ---- 5. bookkeeping (greedy_step_kernel's)
    if (threadIdx.x == 0) {
        if (idx < 0 || idx >= V) idx = 0;              // a row of NaNs: any valid index
        int live = unfinished[b];
        long tok = idx;
        if (!live && has_pad) tok = pad;
        seq[(long)b * seq_ld + pos] = tok;
        if (live) {
            for (int e = 0; e < n_eos; ++e)
                if (eos[e] == tok) live = 0;
            unfinished[b] = live;
        }
        if (live) atomicAdd(alive, 1);
    }
}

template <int DT>
int launch_sample_step(const void* logits, int64_t row_stride, int64_t B, int64_t V, const void* noise, float temperature, int64_t top_k, float top_p,
                       void* unfinished, const void* eos, int64_t n_eos, int64_t pad, int has_pad, void* seq, int64_t seq_ld, int64_t pos,
                       void* alive, hipStream_t st) {
    const int lds = (((int)V + 3) & ~3) * 4 + SS_HIST * 4;
    static UllOncePerDevice once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)sample_step_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - SS_STATIC);
    hipLaunchKernelGGL(sample_step_kernel<DT>, dim3((unsigned)B), dim3(SS_THREADS), lds, st, logits, (long)row_stride, (int)V, (const float*)noise,
                       temperature, (int)(top_k > V ? V : top_k), top_p, (int32_t*)unfinished, (const int64_t*)eos, (int)n_eos, (long)pad, has_pad,
                       (int64_t*)seq, (long)seq_ld, (int)pos, (int32_t*)alive);
    return ull_check_launch();
}

// ---- one step of prompt-lookup speculative decoding (batch 1), two launches ---------------------------------------------------------
// The forward ran on buf[n - 1 : n + d] (the last valid id and the d drafts that already sit in buf[n : n + d]) and left 1 + d rows of logits.
// spec_pick_kernel: one block per row picks that row's token t_i by the plain loop's rule (greedy_pick, or sample_pick on the row's noise).
// spec_accept_kernel (one block): a = the leading i < d with t_i == buf[n + i]; t_0 .. t_a are emitted into buf[n ...], cut at n_max valid ids
// and after the first EOS id (finished); then the next step's drafts are looked up (modeling_core.prompt_lookup_candidates restated) over the
// n' valid ids and written to buf[n' : n' + d'], and record = (emitted, finished, d').  No block waits on another; every loop is bounded by
// an argument of the launch.
template <int DT>
__global__ __launch_bounds__(SS_THREADS) void spec_pick_kernel(const void* __restrict__ logits, long row_stride, int V, const float* __restrict__ noise,
                                                               float temperature, int top_k, float top_p, int32_t* __restrict__ picks) {
    extern __shared__ uint32_t lds[];
    __shared__ Scratch sc;
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2;
    const int b = blockIdx.x;
    const char* row = (const char*)logits + (long)b * row_stride * ESZ;
    int idx;
    if (noise) {
        idx = sample_pick<DT>(row, V, noise + (long)b * V, temperature, top_k, top_p, lds, sc);
        if (idx < 0 || idx >= V) idx = 0;              // a row of NaNs: any valid index
    } else {
        idx = greedy_pick<DT>(row, V, sc.f, sc.i);
    }
    if (threadIdx.x == 0) picks[b] = idx;
}

ULL_DEV bool is_eos(int64_t tok, const int64_t* __restrict__ eos, int n_eos) {
    for (int e = 0; e < n_eos; ++e)
        if (eos[e] == tok) return true;
    return false;
}

__global__ __launch_bounds__(SS_THREADS) void spec_accept_kernel(const int32_t* __restrict__ picks, int64_t* buf, int n, int d, int n_max,
                                                                 const int64_t* __restrict__ eos, int n_eos, int num_tokens, int max_ngram,
                                                                 int32_t* __restrict__ record) {
    __shared__ int s_emit, s_fin, s_min[16];
    const int tid = threadIdx.x;
    if (tid == 0) {
        int a = 0;
        while (a < d && (int64_t)picks[a] == buf[n + a]) ++a;
        int m = min(a + 1, n_max - n), fin = 0;
        for (int j = 0; j < m; ++j)
            if (is_eos(picks[j], eos, n_eos)) { m = j + 1; fin = 1; break; }
        for (int j = 0; j < m; ++j) buf[n + j] = picks[j];
        s_emit = m;
        s_fin = fin;
    }
    __syncthreads();                                   // (also orders thread 0's stores to buf before the scan's loads)
    const int emitted = s_emit, fin = s_fin, n2 = n + emitted;
    const int limit = n_max - n2 - 1;                  // a step never proposes more than it may emit
    int d2 = 0;
    if (!fin && limit > 0) {
        const int want = min(num_tokens, limit);
#pragma unroll 1
        for (int ng = min(max_ngram, n2 - 1); ng >= 1; --ng) {
            // the earliest window [s, s + ng) equal to the trailing ng ids with a non-empty continuation: s <= n2 - ng - 1
            const int64_t* tail = buf + (n2 - ng);
            int first = 0x7fffffff;
            for (int s = tid; s <= n2 - ng - 1; s += SS_THREADS) {       // any history length: the last round is partial
                bool eq = true;
                for (int j = 0; j < ng && eq; ++j) eq = buf[s + j] == tail[j];
                if (eq) { first = s; break; }          // increasing s per thread: its earliest
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
            __syncthreads();
            if ((tid & 63) == 0) s_min[tid >> 6] = first;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 16; ++w) first = min(first, s_min[w]);
            if (first != 0x7fffffff) {                 // (the same value in every thread)
                const int start = first + ng, end = min(start + want, n2);
                if (tid == 0)
                    for (int c = start; c < end; ++c) {              // cut before the first EOS id
                        const int64_t tok = buf[c];
                        if (is_eos(tok, eos, n_eos)) break;
                        buf[n2 + d2++] = tok;
                    }
                break;
            }
        }
    }
    if (tid == 0) { record[0] = emitted; record[1] = fin; record[2] = d2; }
}

template <int DT>
int launch_spec_pick(const void* logits, int64_t row_stride, int64_t R, int64_t V, const void* noise, float temperature, int64_t top_k, float top_p,
                     void* picks, hipStream_t st) {
    const int lds = noise ? (((int)V + 3) & ~3) * 4 + SS_HIST * 4 : 0;
    static UllOncePerDevice once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)spec_pick_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - SS_STATIC);
    hipLaunchKernelGGL(spec_pick_kernel<DT>, dim3((unsigned)R), dim3(SS_THREADS), lds, st, logits, (long)row_stride, (int)V, (const float*)noise,
                       temperature, (int)(top_k > V ? V : top_k), top_p, (int32_t*)picks);
    return ull_check_launch();
}

}  // namespace

extern "C" int ull_spec_step(const void* logits, int logits_dtype, int64_t row_stride, int64_t V, const void* noise, float temperature, int64_t top_k,
                             float top_p, void* buf, int64_t buf_len, int64_t n, int64_t d, int64_t n_max, const void* eos, int64_t n_eos,
                             int64_t num_tokens, int64_t max_ngram, void* picks, void* record, void* stream) {
    if (!logits || !buf || !picks || !record || V <= 0 || (n_eos > 0 && !eos) || n_eos < 0 || logits_dtype < 0 || logits_dtype > 2 || top_k < 0 ||
        !(top_p == top_p) || (noise && !(temperature > 0.f)))
        return ULL_ERR_ARG;
    // n valid ids, d drafts behind them, at most n_max valid ids in the end: the kernels read buf[0, max(n + d, n_max)) and write buf[n, n_max)
    if (n < 1 || d < 0 || d > ULL_SPEC_MAX_DRAFT || num_tokens < 1 || num_tokens > ULL_SPEC_MAX_DRAFT || max_ngram < 1 || n >= n_max || n + d > buf_len ||
        n_max > buf_len || n_max > 0x7fffffff)
        return ULL_ERR_ARG;
    if (noise && V > SS_MAX_V) return ULL_ERR_SHAPE;  // the sampled pick stages the row in LDS as 4-byte keys
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (logits_dtype == ULL_DT_BF16) rc = launch_spec_pick<ULL_DT_BF16>(logits, row_stride, 1 + d, V, noise, temperature, top_k, top_p, picks, st);
    else if (logits_dtype == ULL_DT_F16) rc = launch_spec_pick<ULL_DT_F16>(logits, row_stride, 1 + d, V, noise, temperature, top_k, top_p, picks, st);
    else rc = launch_spec_pick<ULL_DT_F32>(logits, row_stride, 1 + d, V, noise, temperature, top_k, top_p, picks, st);
    if (rc != ULL_OK) return rc;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(SS_THREADS), 0, st, (const int32_t*)picks, (int64_t*)buf, (int)n, (int)d, (int)n_max,
                       (const int64_t*)eos, (int)n_eos, (int)num_tokens, (int)max_ngram, (int32_t*)record);
    return ull_check_launch();
}

extern "C" int ull_sample_step(const void* logits, int logits_dtype, int64_t row_stride, int64_t B, int64_t V, const void* noise, float temperature,
                               int64_t top_k, float top_p, void* unfinished, const void* eos, int64_t n_eos, int64_t pad, int has_pad, void* seq,
                               int64_t seq_ld, int64_t pos, void* alive, void* stream) {
    if (!logits || !noise || !unfinished || !seq || !alive || B <= 0 || V <= 0 || pos < 0 || pos >= seq_ld || (n_eos > 0 && !eos) ||
        logits_dtype < 0 || logits_dtype > 2 || !(temperature > 0.f) || top_k < 0 || !(top_p == top_p))
        return ULL_ERR_ARG;
    if (V > SS_MAX_V) return ULL_ERR_SHAPE;           // the row is staged in LDS as 4-byte keys
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == ULL_DT_BF16)
        return launch_sample_step<ULL_DT_BF16>(logits, row_stride, B, V, noise, temperature, top_k, top_p, unfinished, eos, n_eos, pad, has_pad, seq, seq_ld, pos, alive, st);
    if (logits_dtype == ULL_DT_F16)
        return launch_sample_step<ULL_DT_F16>(logits, row_stride, B, V, noise, temperature, top_k, top_p, unfinished, eos, n_eos, pad, has_pad, seq, seq_ld, pos, alive, st);
    return launch_sample_step<ULL_DT_F32>(logits, row_stride, B, V, noise, temperature, top_k, top_p, unfinished, eos, n_eos, pad, has_pad, seq, seq_ld, pos, alive, st);
}
