// The query entries of the Linear dispatch rule (linear_route.h): how the Python host reads the rule the C callers apply.  Host code only.
#include "linear_route.h"

extern "C" int64_t ull_linear_route(int64_t M, int64_t N, int64_t K, int64_t ldw, int wfmt, int afmt, int a_decode, int tune) {
    const ull_route::Route r = ull_route::route_of(M, N, K, ldw, wfmt, afmt, a_decode, tune);
    return r.kind | (r.rms_first ? 1 << 8 : 0);
}

extern "C" int64_t ull_gemm_plan(int64_t M, int64_t N, int64_t K, int64_t min_k, int small_m, int small_m_split_k) {
    const bool big = ull_route::is_big(M, N, K);
    return (big ? 1 : 0) | (ull_route::gemm_split(big, M, N, K, min_k, small_m != 0, small_m_split_k != 0) ? 2 : 0);
}

extern "C" int64_t ull_decode_step_fused(int64_t T, int64_t D, int64_t hd) { return ull_route::decode_step_fused(T, D, hd) ? 1 : 0; }
