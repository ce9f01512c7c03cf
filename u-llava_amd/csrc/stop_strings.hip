// generate(stop_strings=): the per-row stop on TEXT, decided on the device (`generation.stop_strings_reference`, which stays the definition).
// The host criterion the reference's callers pass reads the ids after every step and decodes all generated tokens again; here the step is
// one launch that never leaves the device, so the fused decode loop keeps looking at the host every 8 steps only.
//
// Compiled once; there is no dtype: only ids and bytes are read.  The text of a row is the concatenation of the table bytes of its
// generated ids (tok_bytes[tok_off[id] .. tok_off[id+1]) for 0 <= id < V, nothing otherwise), and a step only has to decide whether a stop
// string ENDS inside the bytes of the last token, ids[r, cur_len-1]: earlier ends were decided by earlier steps.  One 64-thread block (one
// wave) per row:
//   0. the block copies the stop strings into LDS (at most ULL_STOP_MAX_STRINGS * ULL_STOP_MAX_BYTES bytes; their offsets arrive by value);
//   1. the row's last token has n_last bytes (0: no string can end in it, done); need = n_last + longest stop string - 1 bytes decide;
//   2. the walk back: lane j takes column cur_len-1-j (never below L0), looks its id's length up -- if 0 <= id < V: no address is formed
//      from an unchecked id -- and a wave prefix sum gives every token its distance from the end of the text; each lane copies those of
//      its token's bytes that lie within `need` into the row's LDS window.  64 columns per round, until `need` bytes are there or column L0
//      is passed: zero-byte tokens (special ids, ids outside the table) cost a lane and nothing else;
//   3. the lanes stride over the (stop string, end byte inside the last token) pairs and compare backwards through the window; a match
//      may not begin before the first byte the walk found, so text before L0 never counts;
//   4. any pair matched: lane 0 sets live[r] = 0 and takes the row out of alive[0] with one vector atomic, so the result does not depend
//      on the order of the rows.  Rows that come in with live == 0 are not touched.
// Every length read from the table is clamped to [0, ULL_STOP_MAX_TOKEN_BYTES] and every byte offset to the table's size, so a table that
// breaks its own contract gives a wrong answer, never an address outside it.
#include "ull_common.h"

namespace {

constexpr int ST_THREADS = 64;                                     // one wave: the prefix sum of step 2 is a wave scan
constexpr int ST_WIN = ULL_STOP_MAX_WINDOW;
static_assert(ST_WIN >= ULL_STOP_MAX_TOKEN_BYTES + ULL_STOP_MAX_BYTES - 1, "the window holds the last token and the longest string's head");

struct StopOffsets {
    int32_t off[ULL_STOP_MAX_STRINGS + 1];                         // validated by the entry: off[0] = 0, 1 <= off[s+1] - off[s] <= ULL_STOP_MAX_BYTES
};

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(ST_THREADS) void stop_strings_kernel(const int64_t* __restrict__ ids, long ids_ld, long L0, long cur_len,
                                                                   const int32_t* __restrict__ tok_off, const uint8_t* __restrict__ tok_bytes,
                                                                   long V, long n_tok_bytes, StopOffsets so, const uint8_t* __restrict__ stop_bytes,
                                                                   int S, int max_stop, int32_t* __restrict__ live, int32_t* __restrict__ alive) {
    __shared__ uint8_t s_stop[ULL_STOP_MAX_STRINGS * ULL_STOP_MAX_BYTES];
    __shared__ int32_t s_off[ULL_STOP_MAX_STRINGS + 1];
    __shared__ uint8_t win[ST_WIN];
    const int tid = threadIdx.x, lane = tid;

    // ---- 0. the stop strings (so.off[S] <= ULL_STOP_MAX_STRINGS * ULL_STOP_MAX_BYTES by the entry's checks)
    for (int i = tid; i <= S; i += ST_THREADS) s_off[i] = so.off[i];
    for (int i = tid; i < so.off[S]; i += ST_THREADS) s_stop[i] = stop_bytes[i];
    __syncthreads();

    const int r = blockIdx.x;                                      // (every branch on r below is uniform over the block)
    if (live[r] == 0) return;
    const int64_t* row = ids + (long)r * ids_ld;

    // the bytes of the id at column c: (offset, length), (0, 0) for a column before L0 and for an id outside the table
    auto token = [&](long c, long& off) -> int {
        off = 0;
        if (c < L0) return 0;
        const int64_t id = row[c];
        if (id < 0 || id >= (int64_t)V) return 0;
        long a = tok_off[id], b = tok_off[id + 1];
        a = min(max(a, 0l), n_tok_bytes);
        b = min(max(b, a), n_tok_bytes);
        off = a;
        return (int)min(b - a, (long)ULL_STOP_MAX_TOKEN_BYTES);
    };

    // ---- 1. the last token
    long off_last;
    const int n_last = token(cur_len - 1, off_last);
    if (n_last == 0) return;
    const int need = n_last + max_stop - 1;                        // <= ST_WIN: the window's bytes sit at win[ST_WIN - need .. ST_WIN)

    // ---- 2. the walk back.  `have` bytes of text lie behind (later than) this round's columns
    int have = 0;
    for (long c0 = cur_len - 1; c0 >= L0 && have < need; c0 -= 64) {
        long off;
        const int len = token(c0 - lane, off);
        const int incl = wave_inclusive_sum(len, lane);
        const int end = have + incl - len;                         // distance of this token's last byte from the end of the text
        for (int b = 0; b < len; ++b) {
            const int fe = end + (len - 1 - b);                    // ... and of its byte b
            if (fe < need) win[ST_WIN - 1 - fe] = tok_bytes[off + b];
        }
        have += __shfl(incl, 63, 64);
    }
    const int n_have = min(have, need);                            // the window's valid bytes: win[ST_WIN - n_have .. ST_WIN)
    __syncthreads();                                               // the window's bytes of every lane have landed

    // ---- 3. a stop string s ends at byte e of the last token (e = 0 .. n_last - 1): the window index of that byte is ST_WIN - n_last + e
    bool hit = false;
    for (int p = lane; p < S * n_last && !hit; p += 64) {
        const int s = p / n_last, e = p - s * n_last;
        const int a = s_off[s], slen = s_off[s + 1] - a;
        const int last = ST_WIN - n_last + e, first = last - slen + 1;
        if (first < ST_WIN - n_have) continue;                     // it would begin before column L0 (or before the text)
        bool same = true;
        for (int j = 0; same && j < slen; ++j) same = win[first + j] == s_stop[a + j];
        hit = same;
    }

    // ---- 4. the row stops
    if (__any(hit) && lane == 0) {
        live[r] = 0;
        atomicSub(alive, 1);
    }
}

}  // namespace

extern "C" int ull_stop_strings(const void* ids, int64_t ids_ld, int64_t R, int64_t L0, int64_t cur_len, const void* tok_off, const void* tok_bytes,
                                int64_t V, int64_t n_tok_bytes, int64_t max_token_bytes, const void* stop_off, const void* stop_bytes, int64_t S,
                                void* live, void* alive, void* stream) {
    if (!ids || !tok_off || !stop_off || !stop_bytes || !live || !alive || R < 0 || ids_ld < 0 || L0 < 0 || cur_len <= L0 || cur_len > ids_ld ||
        V < 1 || n_tok_bytes < 0 || (n_tok_bytes > 0 && !tok_bytes) || max_token_bytes < 0 || S < 1 || R > INT32_MAX)
        return ULL_ERR_ARG;
    if (S > ULL_STOP_MAX_STRINGS || max_token_bytes > ULL_STOP_MAX_TOKEN_BYTES) return ULL_ERR_SHAPE;
    // the offsets are HOST memory: checked here, before any launch, and handed to the kernel by value
    StopOffsets so = {};
    const int32_t* off = (const int32_t*)stop_off;
    if (off[0] != 0) return ULL_ERR_ARG;
    int max_stop = 0;
    for (int s = 0; s < (int)S; ++s) {
        const int64_t len = (int64_t)off[s + 1] - off[s];
        if (len < 1) return ULL_ERR_ARG;                           // (an empty string would stop every row at once)
        if (len > ULL_STOP_MAX_BYTES) return ULL_ERR_SHAPE;
        max_stop = len > max_stop ? (int)len : max_stop;
    }
    for (int s = 0; s <= (int)S; ++s) so.off[s] = off[s];
    if (R == 0) return ULL_OK;
    hipLaunchKernelGGL(stop_strings_kernel, dim3((unsigned)R), dim3(ST_THREADS), 0, (hipStream_t)stream, (const int64_t*)ids, (long)ids_ld, (long)L0,
                       (long)cur_len, (const int32_t*)tok_off, (const uint8_t*)tok_bytes, (long)V, (long)n_tok_bytes, so, (const uint8_t*)stop_bytes,
                       (int)S, max_stop, (int32_t*)live, (int32_t*)alive);
    return ull_check_launch();
}
