// Beam search on the device: one step of HF `GenerationMixin._beam_search` (do_sample=False) for the whole batch -- the rule is written out in
// `generation.beam_search_reference`, which stays the definition -- and the reorder of the KV cache by the step's `parent`.
//
// ull_beam_step, two launches (compiled once; the logits' dtype is a run-time code, ULL_DT_*):
//   1. beam_rows_kernel, one 1024-thread block per (item, beam): max_r and sum_r of the raw row exactly as token_logprobs_kernel takes them
//      (logsumexp.h), then the row's first nc = min(KK, V) candidates in (acc descending, token ascending), acc_j = (float(pick_j) - max_r
//      - logf(sum_r)) + run_sc -- by acc, not by the logit: two logits can round to one acc.  Every thread keeps the best of its own
//      elements (j = tid mod 1024); a round takes the block's best (xor tree inside a wave, the sixteen wave partials left to right) and only
//      its owner looks for its next one: one pass over the row plus nc short rescans.  A NaN acc is never a candidate; a row that runs out
//      of candidates (NaN logits) fills up with -inf at tokens t mod V.
//   2. beam_merge_kernel, ONE block that walks the items: ranks the K * nc candidates of an item by (acc descending, flat index k * V + j
//      ascending) by counting, keeps the first KK, and does the rule's steps 3-7 on them -- tiny, so the "loop goes on" word, which spans all
//      items, needs no second pass.  The id rows are gathered from the *_in into the *_out buffers (a gather in place would read rows it has
//      overwritten); the per-beam scalars are read into LDS before they are written, so they update in place.
// No floating-point atomics, every reduction in a fixed order: the same inputs give the same bits.
//
// ull_kv_gather_rows, one launch for up to 64 layers: positions of row map[r] of one set of K / V^T buffers copied to row r of another.
#include "ull_common.h"
#include "select.h"
#include "logsumexp.h"

namespace {

constexpr int BM_THREADS = 1024;
constexpr int BM_SLOTS = ULL_BEAM_MAX_CAND;     // candidate slots per (item, beam) in the scratch
constexpr int BM_MAX_K = ULL_BEAM_MAX_K;
constexpr float BM_NEG = -1.0e9f;

// (av, ai) comes before (bv, bi): larger value, then lower index; an index < 0 is "no candidate".  Values are never NaN here.
ULL_DEV bool cand_before(float av, long ai, float bv, long bi) { return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi)); }

template <int DT>
__global__ __launch_bounds__(BM_THREADS) void beam_rows_kernel(const void* __restrict__ logits, long row_stride, const void* __restrict__ pick,
                                                               long pick_stride, int Kin, int K, int V, int nc, const float* __restrict__ run_sc,
                                                               float* __restrict__ cand_v, int32_t* __restrict__ cand_t) {
    __shared__ LpScratch sc;
    __shared__ float wv[16];
    __shared__ int wi[16];
    constexpr int ESZ = DT == ULL_DT_F32 ? 4 : 2;
    const int tid = threadIdx.x;
    const long bk = blockIdx.x, b = bk / K;
    const long src = b * Kin + (Kin == 1 ? 0 : bk % K);            // Kin == 1: every beam of the item reads the item's one row
    const char* raw = (const char*)logits + src * row_stride * ESZ;
    const char* prow = pick ? (const char*)pick + src * pick_stride * ESZ : raw;
    float m, s;
    lp_row_max_sum<DT>(raw, V, sc, m, s);
    const float ls = logf(s), base = run_sc[bk];

    // the best of this thread's elements strictly behind (pv, pi) in the order; pi < 0: of all of them
    auto scan = [&](float pv, int pi, float& bv, int& bi) {
        bv = 0.f;
        bi = -1;
        for (long j = tid; j < V; j += BM_THREADS) {
            const float v = (load_dt<DT>(prow, j) - m - ls) + base;
            if (!(v == v)) continue;
            if (pi >= 0 && !(v < pv || (v == pv && j > pi))) continue;
            if (bi < 0 || v > bv) { bv = v; bi = (int)j; }        // increasing j: the first of equal values stays
        }
    };
    float bv;
    int bi;
    scan(0.f, -1, bv, bi);
    for (int t = 0; t < nc; ++t) {
        float v = bv;
        int i = bi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (cand_before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        __syncthreads();                                           // (the previous round's reads of wv / wi)
        if ((tid & 63) == 0) { wv[tid >> 6] = v; wi[tid >> 6] = i; }
        __syncthreads();
        v = wv[0];
        i = wi[0];
#pragma unroll
        for (int w = 1; w < 16; ++w)
            if (cand_before(wv[w], wi[w], v, i)) { v = wv[w]; i = wi[w]; }
        if (tid == 0) {
            cand_v[bk * BM_SLOTS + t] = i >= 0 ? v : -INFINITY;
            cand_t[bk * BM_SLOTS + t] = i >= 0 ? i : t % V;
        }
        if (i >= 0 && (i & (BM_THREADS - 1)) == tid) scan(v, i, bv, bi);
    }
}

struct BeamArgs {
    const float* cand_v;
    const int32_t* cand_t;
    const int64_t *run_in, *pool_in, *eos;
    int64_t *run_out, *pool_out;
    float *run_sc, *pool_sc;
    int32_t *pool_len, *fin, *open, *parent, *go;
    long V, Lmax, L0, cur, pad;
    int B, K, KK, nc, n_eos, es;
    float pow_fin, pow_hyp;
};

__global__ __launch_bounds__(BM_THREADS) void beam_merge_kernel(const BeamArgs a) {
    __shared__ float sv[BM_THREADS];
    __shared__ long sf[BM_THREADS];
    __shared__ float tv[BM_SLOTS], rv[BM_SLOTS], pv[BM_MAX_K + BM_SLOTS], o_rsc[BM_MAX_K], o_psc[BM_MAX_K];
    __shared__ int tp[BM_SLOTS], tt[BM_SLOTS], hit[BM_SLOTS], selr[BM_MAX_K], selp[BM_MAX_K], o_plen[BM_MAX_K], o_fin[BM_MAX_K];
    const int tid = threadIdx.x, K = a.K, KK = a.KK, N = a.K * a.nc;
    const long Lmax = a.Lmax, cur = a.cur;
    bool any_open = false, all_fin = true, all_hit = true;         // (thread 0's, over the items)
    for (int b = 0; b < a.B; ++b) {
        const long r0 = (long)b * K;
        // ---- the item's K * nc candidates, ranked by counting; the first KK in order
        int k = 0, tok = 0;
        if (tid < N) {
            k = tid / a.nc;
            tok = a.cand_t[(r0 + k) * BM_SLOTS + tid % a.nc];
            tok = tok < 0 ? 0 : tok >= a.V ? (int)(a.V - 1) : tok;
            sv[tid] = a.cand_v[(r0 + k) * BM_SLOTS + tid % a.nc];
            sf[tid] = (long)k * a.V + tok;
        }
        if (tid < KK) { tv[tid] = -INFINITY; tp[tid] = 0; tt[tid] = 0; }
        __syncthreads();
        if (tid < N) {
            const float v = sv[tid];
            const long f = sf[tid];
            int rank = 0;
            for (int j = 0; j < N; ++j) rank += sv[j] > v || (sv[j] == v && (sf[j] < f || (sf[j] == f && j < tid)));
            if (rank < KK) { tv[rank] = v; tp[rank] = k; tt[rank] = tok; }
        }
        __syncthreads();
        // ---- steps 3-5: which candidates hit; the running scores; the finished scores behind the pool's
        if (tid < KK) {
            bool h = cur + 1 == Lmax;
            for (int e = 0; e < a.n_eos; ++e) h = h || a.eos[e] == (int64_t)tt[tid];
            hit[tid] = h;
            rv[tid] = h ? tv[tid] + BM_NEG : tv[tid];
            bool full = a.es == 1;
            for (int j = 0; j < K; ++j) full = full && a.fin[r0 + j] != 0;
            const bool pen = full || a.open[b] == 0 || !(h && tid < K);
            const float fv = tv[tid] / a.pow_fin;
            pv[K + tid] = pen ? fv + BM_NEG : fv;
        }
        if (tid < K) { pv[tid] = a.pool_sc[r0 + tid]; selr[tid] = tid; selp[tid] = tid; }
        __syncthreads();
        if (tid < KK) {
            int rank = 0;
            for (int j = 0; j < KK; ++j) rank += rv[j] > rv[tid] || (rv[j] == rv[tid] && j < tid);
            if (rank < K) selr[rank] = tid;
        }
        if (tid < K + KK) {
            int rank = 0;
            for (int j = 0; j < K + KK; ++j) rank += pv[j] > pv[tid] || (pv[j] == pv[tid] && j < tid);
            if (rank < K) selp[rank] = tid;
        }
        __syncthreads();
        if (tid < K) {
            const int i = selr[tid], e = selp[tid];
            o_rsc[tid] = rv[i];
            a.parent[r0 + tid] = (int32_t)(r0 + tp[i]);
            o_psc[tid] = pv[e];
            o_plen[tid] = e < K ? a.pool_len[r0 + e] : (int32_t)(cur + 1 - a.L0);
            o_fin[tid] = e < K ? a.fin[r0 + e] : (hit[e - K] && e - K < K);
        }
        __syncthreads();
        // ---- the id rows: a candidate is its parent's ids, its token at `cur`, the pad id behind
        for (long x = tid; x < 2 * K * Lmax; x += BM_THREADS) {
            const bool pool = x >= K * Lmax;
            const long y = pool ? x - K * Lmax : x, j = y / Lmax, p = y % Lmax;
            const int e = pool ? selp[j] : K + selr[j];
            int64_t id;
            if (e < K) id = a.pool_in[(r0 + e) * Lmax + p];
            else id = p < cur ? a.run_in[(r0 + tp[e - K]) * Lmax + p] : p == cur ? (int64_t)tt[e - K] : (int64_t)a.pad;
            (pool ? a.pool_out : a.run_out)[(r0 + j) * Lmax + p] = id;
        }
        if (tid < K) {
            a.run_sc[r0 + tid] = o_rsc[tid];
            a.pool_sc[r0 + tid] = o_psc[tid];
            a.pool_len[r0 + tid] = o_plen[tid];
            a.fin[r0 + tid] = o_fin[tid];
        }
        // ---- step 6: can the best running beam still beat the worst finished one
        if (tid == 0) {
            const float best = o_rsc[0] / a.pow_hyp;
            float worst = o_psc[0];
            bool fin_all = true, hit_all = true, better = false;
            for (int j = 1; j < K; ++j) worst = fminf(worst, o_psc[j]);
            for (int j = 0; j < K; ++j) {
                better = better || best > (o_fin[j] ? worst : BM_NEG);
                fin_all = fin_all && o_fin[j];
            }
            for (int j = 0; j < KK; ++j) hit_all = hit_all && hit[j];
            const bool open = a.open[b] != 0 && better;
            a.open[b] = open;
            any_open = any_open || open;
            all_fin = all_fin && fin_all;
            all_hit = all_hit && hit_all;
        }
        __syncthreads();                                           // (the next item reuses the LDS)
    }
    if (tid == 0) a.go[0] = any_open && !(a.es == 1 && all_fin) && !all_hit;
}

template <int DT>
void launch_beam_rows(const void* logits, long row_stride, const void* pick, long pick_stride, int B, int Kin, int K, int V, int nc, const float* run_sc,
                      float* cand_v, int32_t* cand_t, hipStream_t st) {
    hipLaunchKernelGGL(beam_rows_kernel<DT>, dim3((unsigned)(B * K)), dim3(BM_THREADS), 0, st, logits, row_stride, pick, pick_stride, Kin, K, V, nc, run_sc,
                       cand_v, cand_t);
}

// ---------------------------------------------------------------- the KV rows
constexpr int KV_THREADS = 256;
constexpr int KV_MAX_LAYERS = 64;                                  // per launch: the pointers travel as kernel arguments

struct KvPtrs {
    const char* sk[KV_MAX_LAYERS];
    const char* sv[KV_MAX_LAYERS];
    char* dk[KV_MAX_LAYERS];
    char* dv[KV_MAX_LAYERS];
};

// grid: x strides over the 16-byte units of one (row, head), y = destination row * H + head, z = 2 * layer + (0: K, 1: V^T).
// K [rows, H, smax, hd]: n whole rows of hd elements from position p0.  V^T [rows, H, hd, smax]: for each of the hd lines the whole 32-key
// blocks that [p0, p0 + n) touches (source and destination positions agree mod 32, so a key keeps its slot inside its block).
__global__ __launch_bounds__(KV_THREADS) void kv_rows_kernel(const KvPtrs P, const int32_t* __restrict__ row_map, const int32_t* __restrict__ skip, long src_rows,
                                                             int H, int hd, int esz, long src_smax, long dst_smax, long src_p0, long dst_p0, long n) {
    const int l = blockIdx.z >> 1;
    const long r = blockIdx.y / H, h = blockIdx.y % H;
    if (skip && skip[r] == r) return;                              // (uniform over the block)
    const long sr = row_map ? (long)row_map[r] : r;
    if (sr < 0 || sr >= src_rows) return;                          // no address is formed from an unchecked row
    const long step = (long)gridDim.x * KV_THREADS, u0 = (long)blockIdx.x * KV_THREADS + threadIdx.x;
    if ((blockIdx.z & 1) == 0) {
        const uint4* src = (const uint4*)(P.sk[l] + ((sr * H + h) * src_smax + src_p0) * hd * esz);
        uint4* dst = (uint4*)(P.dk[l] + ((r * H + h) * dst_smax + dst_p0) * hd * esz);
        const long units = n * hd * esz / 16;
        for (long u = u0; u < units; u += step) dst[u] = src[u];
    } else {
        const long sq0 = src_p0 & ~31L, dq0 = dst_p0 & ~31L, W = ((src_p0 + n + 31) & ~31L) - sq0, line = W * esz / 16;
        for (long u = u0; u < hd * line; u += step) {
            const long d = u / line, c = u % line;
            const uint4* src = (const uint4*)(P.sv[l] + (((sr * H + h) * hd + d) * src_smax + sq0) * esz);
            uint4* dst = (uint4*)(P.dv[l] + (((r * H + h) * hd + d) * dst_smax + dq0) * esz);
            dst[c] = src[c];
        }
    }
}

}  // namespace

extern "C" int ull_beam_step(const void* logits, int logits_dtype, int64_t row_stride, const void* pick, int64_t pick_stride, int64_t B, int64_t Kin,
                             int64_t K, int64_t V, const void* run_in, void* run_out, const void* pool_in, void* pool_out, void* run_sc, void* pool_sc,
                             void* pool_len, void* fin, void* open, const void* eos, int64_t n_eos, int64_t pad, int64_t Lmax, int64_t L0, int64_t cur,
                             float pow_fin, float pow_hyp, int early_stopping, void* cand_v, void* cand_t, void* parent, void* go, void* stream) {
    if (!logits || !run_in || !run_out || !pool_in || !pool_out || !run_sc || !pool_sc || !pool_len || !fin || !open || !cand_v || !cand_t || !parent ||
        !go || (!eos && n_eos > 0) || logits_dtype < 0 || logits_dtype > 2 || row_stride < 0 || pick_stride < 0 || B < 1 || B > (1 << 20) || K < 1 ||
        K > BM_MAX_K || (Kin != 1 && Kin != K) || V < 1 || V > 0x7fffffff || n_eos < 0 || L0 < 0 || cur < L0 || cur >= Lmax || early_stopping < 0 ||
        early_stopping > 2 || run_in == run_out || pool_in == pool_out)
        return ULL_ERR_ARG;
    if ((1 + n_eos) * K > BM_SLOTS) return ULL_ERR_SHAPE;
    const int64_t KK = (n_eos + 1 > 2 ? n_eos + 1 : 2) * K;
    if (K * V < KK) return ULL_ERR_SHAPE;
    const int nc = (int)(V < KK ? V : KK);
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == ULL_DT_BF16)
        launch_beam_rows<ULL_DT_BF16>(logits, row_stride, pick, pick_stride, (int)B, (int)Kin, (int)K, (int)V, nc, (const float*)run_sc, (float*)cand_v, (int32_t*)cand_t, st);
    else if (logits_dtype == ULL_DT_F16)
        launch_beam_rows<ULL_DT_F16>(logits, row_stride, pick, pick_stride, (int)B, (int)Kin, (int)K, (int)V, nc, (const float*)run_sc, (float*)cand_v, (int32_t*)cand_t, st);
    else
        launch_beam_rows<ULL_DT_F32>(logits, row_stride, pick, pick_stride, (int)B, (int)Kin, (int)K, (int)V, nc, (const float*)run_sc, (float*)cand_v, (int32_t*)cand_t, st);
    if (ull_check_launch() != ULL_OK) return ULL_ERR_LAUNCH;
    BeamArgs a;
    a.cand_v = (const float*)cand_v; a.cand_t = (const int32_t*)cand_t;
    a.run_in = (const int64_t*)run_in; a.pool_in = (const int64_t*)pool_in; a.eos = (const int64_t*)eos;
    a.run_out = (int64_t*)run_out; a.pool_out = (int64_t*)pool_out;
    a.run_sc = (float*)run_sc; a.pool_sc = (float*)pool_sc;
    a.pool_len = (int32_t*)pool_len; a.fin = (int32_t*)fin; a.open = (int32_t*)open; a.parent = (int32_t*)parent; a.go = (int32_t*)go;
    a.V = V; a.Lmax = Lmax; a.L0 = L0; a.cur = cur; a.pad = pad;
    a.B = (int)B; a.K = (int)K; a.KK = (int)KK; a.nc = nc; a.n_eos = (int)n_eos; a.es = early_stopping;
    a.pow_fin = pow_fin; a.pow_hyp = pow_hyp;
    hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(BM_THREADS), 0, st, a);
    return ull_check_launch();
}

extern "C" int ull_kv_gather_rows(const void* const* src_k, const void* const* src_vt, void* const* dst_k, void* const* dst_vt, int64_t n_layers,
                                  int64_t src_rows, int64_t dst_rows, int64_t H, int64_t hd, int64_t elem_size, int64_t src_smax, int64_t dst_smax,
                                  int64_t src_p0, int64_t dst_p0, int64_t n, const void* row_map, const void* skip, void* stream) {
    if (!src_k || !src_vt || !dst_k || !dst_vt || n_layers < 0 || src_rows < 1 || dst_rows < 1 || H < 1 || hd < 1 || (elem_size != 2 && elem_size != 4) ||
        src_p0 < 0 || dst_p0 < 0 || n < 0)
        return ULL_ERR_ARG;
    if ((src_smax & 31) || (dst_smax & 31) || src_p0 + n > src_smax || dst_p0 + n > dst_smax || ((src_p0 ^ dst_p0) & 31) || (hd * elem_size) % 16 ||
        dst_rows * H > 65535)
        return ULL_ERR_SHAPE;
    for (int64_t l = 0; l < n_layers; ++l) {
        if (!src_k[l] || !src_vt[l] || !dst_k[l] || !dst_vt[l]) return ULL_ERR_ARG;
        if (((uintptr_t)src_k[l] | (uintptr_t)src_vt[l] | (uintptr_t)dst_k[l] | (uintptr_t)dst_vt[l]) & 15) return ULL_ERR_SHAPE;
    }
    if (n == 0 || n_layers == 0) return ULL_OK;
    const long W = ((src_p0 + n + 31) & ~31L) - (src_p0 & ~31L);
    const long units_k = n * hd * elem_size / 16, units_v = hd * (W * elem_size / 16), units = units_k > units_v ? units_k : units_v;
    const unsigned gx = (unsigned)((units + KV_THREADS - 1) / KV_THREADS < 64 ? (units + KV_THREADS - 1) / KV_THREADS : 64);
    for (int64_t l0 = 0; l0 < n_layers; l0 += KV_MAX_LAYERS) {
        const int nl = (int)(n_layers - l0 < KV_MAX_LAYERS ? n_layers - l0 : KV_MAX_LAYERS);
        KvPtrs P = {};
        for (int l = 0; l < nl; ++l) {
            P.sk[l] = (const char*)src_k[l0 + l]; P.sv[l] = (const char*)src_vt[l0 + l];
            P.dk[l] = (char*)dst_k[l0 + l]; P.dv[l] = (char*)dst_vt[l0 + l];
        }
        hipLaunchKernelGGL(kv_rows_kernel, dim3(gx, (unsigned)(dst_rows * H), (unsigned)(2 * nl)), dim3(KV_THREADS), 0, (hipStream_t)stream, P,
                           (const int32_t*)row_map, (const int32_t*)skip, (long)src_rows, (int)H, (int)hd, (int)elem_size, (long)src_smax, (long)dst_smax,
                           (long)src_p0, (long)dst_p0, (long)n);
        if (ull_check_launch() != ULL_OK) return ULL_ERR_LAUNCH;
    }
    return ULL_OK;
}
