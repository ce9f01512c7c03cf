// Operand, nibble and scale-byte map of v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 A operand (cbsz = 4) against an e4m3 B operand
// (blgp = 0), found with exact integer data, plus the issue rate of the mixed form against e4m3 x e4m3 and e2m1 x e2m1.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mfma_scale_w4a8_lane_map.hip -o tools/probes/mfma_scale_w4a8_lane_map && tools/probes/mfma_scale_w4a8_lane_map
// A lane holds 32 e2m1 codes of A (16 bytes: VGPRs 0..3 of the 8-register operand, 4..7 ignored) and 32 e4m3 code bytes of B.
//   pass 1  every A slot (lane la, nibble na) in turn holds e2m1 1.0 (code 2), the rest 0, against three B images whose byte (lb, bb) holds the
//           small integer (lb >> 4), (bb & 7), (bb >> 3): the row of D that lights up is the slot's row, the values name the B slot it pairs with.
//           VGPRs 4..7 of A hold junk (0x77 = 6.0 everywhere) to show that they are ignored.
//   pass 2  every B slot in turn holds e4m3 1.0 against an all-ones A: the column that lights up.
//   pass 3  scales: a one-hot A slot (la, nibble 0) against all-ones B, A's scale register of lane l holding the bytes 100 + (l & 15) + 16 b
//           and then 100 + (l >> 4) + 4 b (b = 0..3): the exponent of D names the lane and the byte that the select value picked.  The same for
//           B's scale register with a one-hot B slot at byte 0 and at byte 16.
// Prints the table and whether it is the map csrc/gemm.hip (gemm128_w4a8_kernel) relies on, k the position in the 128-deep product:
//   A slot (l, n): row l & 15, k = 32 (l >> 4) + n, nibble n = low (n even) / high (n odd) half of byte n >> 1;
//   B slot (l, b): column l & 15, k = 64 (b >> 4) + 16 (l >> 4) + (b & 15) -- the 8-bit operand interleaves 16-byte pieces over the lane groups;
//   scale of (row or column r, block j = k >> 5): byte `select` of the scale register of lane r + 16 j, for A and for B.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>

using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ uint8_t code_of(int v) {          // e4m3fn codes of 0 .. 8
    const uint8_t t[9] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50};
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
        if (sel_a == 0) return mm<4, 0, 0, 0>(a, b, z, sa, sb);
        if (sel_a == 1) return mm<4, 0, 1, 0>(a, b, z, sa, sb);
        if (sel_a == 2) return mm<4, 0, 2, 0>(a, b, z, sa, sb);
        return mm<4, 0, 3, 0>(a, b, z, sa, sb);
    }
    if (sel_b == 1) return mm<4, 0, 0, 1>(a, b, z, sa, sb);
    if (sel_b == 2) return mm<4, 0, 0, 2>(a, b, z, sa, sb);
    return mm<4, 0, 0, 3>(a, b, z, sa, sb);
}

// the A image of a one-hot nibble: bytes 0..15 carry the 32 codes, bytes 16..31 junk
__device__ void a_onehot(uint8_t* a, bool mine, int nib) {
    for (int i = 0; i < 16; ++i) a[i] = 0;
    for (int i = 16; i < 32; ++i) a[i] = 0x77;
    if (mine) a[nib >> 1] = (uint8_t)(2 << (4 * (nib & 1)));
}

// out[slot * 4 + 0..3]: A pass: row, paired group, paired byte & 7, paired byte >> 3;  out[(2048 + slot) * 4]: column of the B slot;
// out[4096 * 4 + (sel * 64 + l) * 6 + 0..1]: A-scale exponents e1, e2 of A slot (l, 0) under select sel; + 2..3 / 4..5: the same for B's scale
// with B slot (l, byte 0) / (l, byte 16)
__global__ __launch_bounds__(64) void probe(int* out) {
    const int lane = threadIdx.x;
    uint8_t a[32], b[32];
    const int one = 0x7f7f7f7f;
    for (int slot = 0; slot < 2048; ++slot) {
        const int sl = slot >> 5, sb = slot & 31;
        a_onehot(a, lane == sl, sb);
        int res[4] = {-1, -1, -1, -1};
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < 32; ++i) b[i] = code_of(1 + (pass == 0 ? (lane >> 4) : pass == 1 ? (i & 7) : (i >> 3)));
            const f32x4 d = mm_sel(pack(a), pack(b), 0, one, 0, one);            // D[row 4 (lane >> 4) + r][col lane & 15]
            for (int r = 0; r < 4; ++r)
                if (d[r] != 0.f && (lane & 15) == 0) { res[0] = 4 * (lane >> 4) + r; res[1 + pass] = (int)d[r] - 1; }
        }
        for (int i = 0; i < 4; ++i) {
            const int v = wave_max_i(res[i]);
            if (lane == 0) out[slot * 4 + i] = v;
        }
        for (int i = 0; i < 32; ++i) { b[i] = (lane == sl && i == sb) ? 0x38 : 0; a[i] = i < 16 ? 0x22 : 0x77; }
        const f32x4 d = mm_sel(pack(a), pack(b), 0, one, 0, one);
        int col = -1;
        for (int r = 0; r < 4; ++r)
            if (d[r] != 0.f) col = lane & 15;
        col = wave_max_i(col);
        if (lane == 0) out[(2048 + slot) * 4] = col;
    }
    for (int sel = 0; sel < 4; ++sel)
        for (int l = 0; l < 64; ++l)
            for (int side = 0; side < 3; ++side)
                for (int pass = 0; pass < 2; ++pass) {
                    int sc = 0;
                    for (int bt = 3; bt >= 0; --bt) sc = (sc << 8) | (pass == 0 ? 100 + (lane & 15) + 16 * bt : 100 + (lane >> 4) + 4 * bt);
                    if (side == 0) {
                        a_onehot(a, lane == l, 0);
                        for (int i = 0; i < 32; ++i) b[i] = 0x38;
                    } else {
                        for (int i = 0; i < 32; ++i) { b[i] = (lane == l && i == (side == 2 ? 16 : 0)) ? 0x38 : 0; a[i] = i < 16 ? 0x22 : 0x77; }
                    }
                    const f32x4 d = side == 0 ? mm_sel(pack(a), pack(b), sel, sc, 0, one) : mm_sel(pack(a), pack(b), 0, one, sel, sc);
                    int e = -1000;
                    for (int r = 0; r < 4; ++r)
                        if (d[r] != 0.f) e = ilogbf(d[r]) + 127;
                    e = wave_max_i(e);
                    if (lane == 0) out[4096 * 4 + (sel * 64 + l) * 6 + side * 2 + pass] = e;
                }
}

// issue rate: 4 waves per block, 16 independent accumulators per wave, one block per CU slot
template <int CB, int BL>
__global__ __launch_bounds__(256) void rate(float* out, int iters) {
    i32x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = 0x22222222; b[i] = CB == BL ? 0x22222222 : 0x38383838; }
    if (CB == 0) for (int i = 0; i < 8; ++i) a[i] = 0x38383838;
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
    std::vector<int> h(4096 * 4 + 256 * 6, -2);
    if (hipMalloc(&d, h.size() * sizeof(int)) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h.data(), d, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    printf("A (e2m1) slot (lane l, nibble n) -> row, paired B (e4m3) slot (lane group, byte); first lane of each group, then every slot that differs "
           "from the map\n");
    for (int slot = 0; slot < 2048; ++slot) {
        const int l = slot >> 5, n = slot & 31;
        const int row = h[slot * 4], grp = h[slot * 4 + 1], byte = h[slot * 4 + 2] + 8 * h[slot * 4 + 3], col = h[(2048 + slot) * 4];
        const int k = 32 * (l >> 4) + n;                      // the A slot's k; the B slot of that k is (group (k >> 4) & 3, byte (k & 15) + 16 (k >> 6))
        const bool ok = row == (l & 15) && grp == ((k >> 4) & 3) && byte == (k & 15) + 16 * (k >> 6) && col == (l & 15);
        if ((l & 15) == 0 && (n & 7) == 0)
            printf("  lane %2d nibbles %2d..%2d (byte %2d low first): row %d, B group %d, B bytes %d..\n", l, n, n + 7, n >> 1, row, grp, byte);
        if (!ok && bad++ < 32) printf("  DIFFERS slot (lane %d, nibble %d): A row %d, pairs with B group %d byte %d; B column %d\n", l, n, row, grp, byte, col);
    }
    printf("A slot (l, n): row l & 15, k = 32 (l >> 4) + n, low nibble first, VGPRs 4..7 ignored; B slot (l, b): column l & 15, "
           "k = 64 (b >> 4) + 16 (l >> 4) + (b & 15) -- %s (%d of 2048 slots differ)\n", bad ? "NOT the map found" : "confirmed for all 2048 slots", bad);
    int sbad = 0;
    const char* what[3] = {"A slot (l, nibble 0)", "B slot (l, byte 0)", "B slot (l, byte 16)"};
    for (int sel = 0; sel < 4; ++sel)
        for (int side = 0; side < 3; ++side) {
            int ok = 0, byte_seen = -1;
            for (int l = 0; l < 64; ++l) {
                const int* e = &h[4096 * 4 + (sel * 64 + l) * 6 + side * 2];
                const int e1 = e[0] - 100, e2 = e[1] - 100;
                const int src_lane = (e1 & 15) + 16 * (e2 & 3), b1 = e1 >> 4, b2 = e2 >> 2;
                const int k = side == 0 ? 32 * (l >> 4) : 16 * (l >> 4) + (side == 2 ? 64 : 0);
                if (src_lane == (l & 15) + 16 * (k >> 5) && b1 == b2 && b1 == sel) ++ok;
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
