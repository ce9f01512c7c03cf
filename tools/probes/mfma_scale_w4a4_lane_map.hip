// Operand, nibble and scale-byte map of v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1 for BOTH operands (cbsz = 4, blgp = 4), found with exact
// integer data, plus the issue rate of e2m1 x e2m1 against the mixed and the e4m3 x e4m3 form.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mfma_scale_w4a4_lane_map.hip -o tools/probes/mfma_scale_w4a4_lane_map && tools/probes/mfma_scale_w4a4_lane_map
// A lane holds 32 e2m1 codes of A and 32 of B (16 bytes each: VGPRs 0..3 of the 8-register operands; 4..7 hold junk, 0x77 = 6.0, to show
// that they are ignored for both).
//   pass 1  every A slot (lane la, nibble na) in turn holds e2m1 1.0 (code 2), the rest 0, against four B images whose nibble (lb, nb) holds
//           the small integer 1 + (lb >> 4), 1 + (nb & 3), 1 + ((nb >> 2) & 3), 1 + (nb >> 4): the row of D that lights up is the slot's row,
//           the values name the B slot it pairs with.  The images are asymmetric: A is one-hot, B is dense.
//   pass 2  the mirror: every B slot one-hot against the four dense A images: the column, and the A slot it pairs with.
//   pass 3  scales: a one-hot A slot (la, nibble 0) against all-ones B, A's scale register of lane l holding the bytes 100 + (l & 15) + 16 b
//           and then 100 + (l >> 4) + 4 b (b = 0..3): the exponent of D names the lane and the byte that the select value picked.  The same
//           for B's scale register with a one-hot B slot (lb, nibble 0).
// Prints the table and whether it is the map csrc/gemm.hip (gemm128_w4a4_kernel) relies on, k the position in the 128-deep product:
//   A slot (l, n): row l & 15, k = 32 (l >> 4) + n;  B slot (l, n): column l & 15, k = 32 (l >> 4) + n; nibble n = low (n even) / high (n odd)
//   half of byte n >> 1;  scale of (row or column r, block j = k >> 5): byte `select` of the scale register of lane r + 16 j, for A and for B.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>

using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ uint8_t code_of(int v) {          // e2m1 codes of 1 .. 4
    const uint8_t t[5] = {0, 2, 4, 5, 6};
    return t[v];
}

__device__ int wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ i32x8 pack(const uint8_t* a) {
    i32x8 v;
    for (int i = 0; i < 8; ++i) v[i] = (int)(a[4 * i] | (a[4 * i + 1] << 8) | (a[4 * i + 2] << 16) | ((uint32_t)a[4 * i + 3] << 24));
    return v;
}

template <int CB, int BL, int SA, int SB>
__device__ f32x4 mm(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, CB, BL, SA, sa, SB, sb);
}

__device__ f32x4 mm_sel(i32x8 a, i32x8 b, int sel_a, int sa, int sel_b, int sb) {
    const f32x4 z{0.f, 0.f, 0.f, 0.f};
    if (sel_b == 0) {
        if (sel_a == 0) return mm<4, 4, 0, 0>(a, b, z, sa, sb);
        if (sel_a == 1) return mm<4, 4, 1, 0>(a, b, z, sa, sb);
        if (sel_a == 2) return mm<4, 4, 2, 0>(a, b, z, sa, sb);
        return mm<4, 4, 3, 0>(a, b, z, sa, sb);
    }
    if (sel_b == 1) return mm<4, 4, 0, 1>(a, b, z, sa, sb);
    if (sel_b == 2) return mm<4, 4, 0, 2>(a, b, z, sa, sb);
    return mm<4, 4, 0, 3>(a, b, z, sa, sb);
}

// a one-hot nibble: bytes 0..15 carry the 32 codes, bytes 16..31 junk
__device__ void onehot(uint8_t* a, bool mine, int nib) {
    for (int i = 0; i < 16; ++i) a[i] = 0;
    for (int i = 16; i < 32; ++i) a[i] = 0x77;
    if (mine) a[nib >> 1] = (uint8_t)(2 << (4 * (nib & 1)));
}

// the dense image of pass `pass`: nibble n of lane `lane` holds the integer 1 + (lane >> 4), 1 + (n & 3), 1 + ((n >> 2) & 3), 1 + (n >> 4)
__device__ void dense(uint8_t* b, int lane, int pass) {
    for (int i = 0; i < 16; ++i) {
        uint8_t v = 0;
        for (int h = 0; h < 2; ++h) {
            const int n = 2 * i + h;
            v |= (uint8_t)(code_of(1 + (pass == 0 ? (lane >> 4) : pass == 1 ? (n & 3) : pass == 2 ? ((n >> 2) & 3) : (n >> 4))) << (4 * h));
        }
        b[i] = v;
    }
    for (int i = 16; i < 32; ++i) b[i] = 0x77;
}

// out[(side * 2048 + slot) * 5 + 0..4]: row (side 0: one-hot A) / column (side 1: one-hot B), then the paired slot's lane group, nibble & 3,
// (nibble >> 2) & 3, nibble >> 4;  out[4096 * 5 + (sel * 64 + l) * 4 + 0..1]: A-scale exponents e1, e2 of A slot (l, 0) under select sel;
// + 2..3: the same for B's scale with B slot (l, 0)
__global__ __launch_bounds__(64) void probe(int* out) {
    const int lane = threadIdx.x;
    uint8_t a[32], b[32];
    const int one = 0x7f7f7f7f;
    for (int side = 0; side < 2; ++side)
        for (int slot = 0; slot < 2048; ++slot) {
            const int sl = slot >> 5, sn = slot & 31;
            int res[5] = {-1, -1, -1, -1, -1};
            for (int pass = 0; pass < 4; ++pass) {
                if (side == 0) { onehot(a, lane == sl, sn); dense(b, lane, pass); }
                else { onehot(b, lane == sl, sn); dense(a, lane, pass); }
                const f32x4 d = mm_sel(pack(a), pack(b), 0, one, 0, one);            // D[row 4 (lane >> 4) + r][col lane & 15]
                if (side == 0) {                                                     // a row lights up: read it in column 0
                    for (int r = 0; r < 4; ++r)
                        if (d[r] != 0.f && (lane & 15) == 0) { res[0] = 4 * (lane >> 4) + r; res[1 + pass] = (int)d[r] - 1; }
                } else {                                                             // a column lights up: read it in row 0
                    if (d[0] != 0.f && (lane >> 4) == 0) { res[0] = lane & 15; res[1 + pass] = (int)d[0] - 1; }
                }
            }
            for (int i = 0; i < 5; ++i) {
                const int v = wave_max_i(res[i]);
                if (lane == 0) out[(side * 2048 + slot) * 5 + i] = v;
            }
        }
    for (int sel = 0; sel < 4; ++sel)
        for (int l = 0; l < 64; ++l)
            for (int side = 0; side < 2; ++side)
                for (int pass = 0; pass < 2; ++pass) {
                    int sc = 0;
                    for (int bt = 3; bt >= 0; --bt) sc = (sc << 8) | (pass == 0 ? 100 + (lane & 15) + 16 * bt : 100 + (lane >> 4) + 4 * bt);
                    if (side == 0) {
                        onehot(a, lane == l, 0);
                        for (int i = 0; i < 32; ++i) b[i] = i < 16 ? 0x22 : 0x77;
                    } else {
                        onehot(b, lane == l, 0);
                        for (int i = 0; i < 32; ++i) a[i] = i < 16 ? 0x22 : 0x77;
                    }
                    const f32x4 d = side == 0 ? mm_sel(pack(a), pack(b), sel, sc, 0, one) : mm_sel(pack(a), pack(b), 0, one, sel, sc);
                    int e = -1000;
                    for (int r = 0; r < 4; ++r)
                        if (d[r] != 0.f) e = ilogbf(d[r]) + 127;
                    e = wave_max_i(e);
                    if (lane == 0) out[4096 * 5 + (sel * 64 + l) * 4 + side * 2 + pass] = e;
                }
}

// issue rate: 4 waves per block, 16 independent accumulators per wave, one block per CU slot
template <int CB, int BL>
__global__ __launch_bounds__(256) void rate(float* out, int iters) {
    i32x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = CB == 4 ? 0x22222222 : 0x38383838; b[i] = BL == 4 ? 0x22222222 : 0x38383838; }
    f32x4 acc[16];
    for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sc = 0x7f7f7f7f - (int)(threadIdx.x & 1);
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = mm<CB, BL, 0, 0>(a, b, acc[i], sc, 0x7f7f7f7f);
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.f) out[0] = s;
}

template <int CB, int BL>
static double time_rate(float* d, int blocks, int iters) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((rate<CB, BL>), dim3(blocks), dim3(256), 0, 0, d, iters);
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL((rate<CB, BL>), dim3(blocks), dim3(256), 0, 0, d, iters);
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 2.0 * 16 * 16 * 128 * 16.0 * iters * 4.0 * blocks / (best * 1e-3) * 1e-12;   // TFLOP/s
}

int main() {
    int* d;
    std::vector<int> h(4096 * 5 + 256 * 4, -2);
    if (hipMalloc(&d, h.size() * sizeof(int)) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h.data(), d, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    const char* name[2] = {"A", "B"};
    for (int side = 0; side < 2; ++side) {
        printf("%s (e2m1) slot (lane l, nibble n) -> %s, paired %s slot (lane group, nibble); first lane of each group, then every slot that differs "
               "from the map\n", name[side], side ? "column" : "row", name[side ^ 1]);
        for (int slot = 0; slot < 2048; ++slot) {
            const int l = slot >> 5, n = slot & 31;
            const int* r = &h[(side * 2048 + slot) * 5];
            const int rc = r[0], grp = r[1], nib = r[2] + 4 * r[3] + 16 * r[4];
            const bool ok = rc == (l & 15) && grp == (l >> 4) && nib == n;     // both operands: k = 32 (l >> 4) + n
            if ((l & 15) == 0 && (n & 7) == 0)
                printf("  lane %2d nibbles %2d..%2d (byte %2d low first): %s %d, %s group %d, %s nibbles %d..\n", l, n, n + 7, n >> 1,
                       side ? "column" : "row", rc, name[side ^ 1], grp, name[side ^ 1], nib);
            if (!ok && bad++ < 32)
                printf("  DIFFERS %s slot (lane %d, nibble %d): %s %d, pairs with %s group %d nibble %d\n", name[side], l, n, side ? "column" : "row", rc,
                       name[side ^ 1], grp, nib);
        }
    }
    printf("A slot (l, n): row l & 15, k = 32 (l >> 4) + n; B slot (l, n): column l & 15, k = 32 (l >> 4) + n; low nibble first, VGPRs 4..7 of both "
           "ignored -- %s (%d of 4096 slots differ)\n", bad ? "NOT the map found" : "confirmed for all 2048 slots of A and of B", bad);
    int sbad = 0;
    const char* what[2] = {"A slot (l, nibble 0)", "B slot (l, nibble 0)"};
    for (int sel = 0; sel < 4; ++sel)
        for (int side = 0; side < 2; ++side) {
            int ok = 0, byte_seen = -1;
            for (int l = 0; l < 64; ++l) {
                const int* e = &h[4096 * 5 + (sel * 64 + l) * 4 + side * 2];
                const int e1 = e[0] - 100, e2 = e[1] - 100;
                const int src_lane = (e1 & 15) + 16 * (e2 & 3), b1 = e1 >> 4, b2 = e2 >> 2;
                if (src_lane == l && b1 == b2 && b1 == sel) ++ok;              // k = 32 (l >> 4): block l >> 4, lane (l & 15) + 16 (l >> 4) = l
                else if (sbad++ < 32) printf("  DIFFERS select %d, %s, l = %d: scale of lane %d, byte %d / %d\n", sel, what[side], l, src_lane, b1, b2);
                byte_seen = b1;
            }
            printf("scale byte select %d, %s: byte %d of the scale register of lane (l & 15) + 16 (k >> 5) for %d of 64 lanes\n", sel, what[side],
                   byte_seen, ok);
        }
    printf("scale of (row / column r, block j = k >> 5): byte `select` of the scale register of lane r + 16 j -- %s\n",
           sbad ? "NOT the map found" : "confirmed");

    int n_cu = 0;
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, 0);
    float* o;
    hipMalloc(&o, 16);
    const int blocks = n_cu * 2, iters = 4000;
    const double r88 = time_rate<0, 0>(o, blocks, iters), r48 = time_rate<4, 0>(o, blocks, iters), r44 = time_rate<4, 4>(o, blocks, iters);
    printf("issue rate, %d CUs, 8 waves per CU, 16 accumulators per wave: e4m3 x e4m3 %.0f TF/s, e2m1 x e4m3 %.0f TF/s, e2m1 x e2m1 %.0f TF/s\n", n_cu,
           r88, r48, r44);
    hipFree(o);
    hipFree(d);
    return (bad || sbad) ? 1 : 0;
}
