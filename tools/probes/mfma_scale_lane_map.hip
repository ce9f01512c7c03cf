// A/B operand lane map of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 A and B and unit block scales, found with exact integer data.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mfma_scale_lane_map.hip -o tools/probes/mfma_scale_lane_map && tools/probes/mfma_scale_lane_map
// A lane holds 32 code bytes (8 VGPRs) of A and of B.  For every A slot (lane la, byte ba) one launch-free pass puts e4m3 1.0 there and
// zeros elsewhere, and multiplies by three B images whose byte (lb, bb) holds a small integer code of (lb >> 4), (bb & 7) and (bb >> 3):
// the row of D that lights up is the slot's row, and the three values name the B slot group / byte it is paired with (the same k).
// A second pass does the same for the columns of B slots.  Prints the map and whether it is the one csrc/gemm.hip relies on:
//   A slot (l, b): row l & 15; B slot (l, b): column l & 15; A slot (l, b) pairs with the B slots (l' with l' >> 4 == l >> 4, b).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
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

__device__ f32x4 mm(const uint8_t* a, const uint8_t* b) {
    i32x8 av, bv;
    for (int i = 0; i < 8; ++i) {
        av[i] = (int)(a[4 * i] | (a[4 * i + 1] << 8) | (a[4 * i + 2] << 16) | ((uint32_t)a[4 * i + 3] << 24));
        bv[i] = (int)(b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24));
    }
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

// out[slot][0..3]: A pass: row, paired group, paired byte & 7, paired byte >> 3;  out[2048 + slot][0]: column of the B slot
__global__ __launch_bounds__(64) void probe(int* out) {
    const int lane = threadIdx.x;
    uint8_t a[32], b[32];
    for (int slot = 0; slot < 2048; ++slot) {
        const int sl = slot >> 5, sb = slot & 31;
        for (int i = 0; i < 32; ++i) a[i] = (lane == sl && i == sb) ? 0x38 : 0;
        int res[4] = {-1, -1, -1, -1};
        for (int pass = 0; pass < 3; ++pass) {
            for (int i = 0; i < 32; ++i) b[i] = code_of(1 + (pass == 0 ? (lane >> 4) : pass == 1 ? (i & 7) : (i >> 3)));
            const f32x4 d = mm(a, b);                                      // D[row 4 (lane >> 4) + r][col lane & 15]
            for (int r = 0; r < 4; ++r)
                if (d[r] != 0.f && (lane & 15) == 0) { res[0] = 4 * (lane >> 4) + r; res[1 + pass] = (int)d[r] - 1; }
        }
        for (int i = 0; i < 4; ++i) {
            const int v = wave_max_i(res[i]);
            if (lane == 0) out[slot * 4 + i] = v;
        }
        // B slot: A all ones -> the column that lights up
        for (int i = 0; i < 32; ++i) { b[i] = (lane == sl && i == sb) ? 0x38 : 0; a[i] = 0x38; }
        const f32x4 d = mm(a, b);
        int col = -1;
        for (int r = 0; r < 4; ++r)
            if (d[r] != 0.f) col = lane & 15;
        col = wave_max_i(col);
        if (lane == 0) out[(2048 + slot) * 4] = col;
    }
}

int main() {
    int* d;
    std::vector<int> h(4096 * 4, -2);
    if (hipMalloc(&d, h.size() * sizeof(int)) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h.data(), d, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int bad = 0;
    for (int slot = 0; slot < 2048; ++slot) {
        const int l = slot >> 5, b = slot & 31;
        const int row = h[slot * 4], grp = h[slot * 4 + 1], byte = h[slot * 4 + 2] + 8 * h[slot * 4 + 3], col = h[(2048 + slot) * 4];
        if (row != (l & 15) || grp != (l >> 4) || byte != b || col != (l & 15)) {
            if (bad++ < 16) printf("slot (lane %d, byte %d): A row %d, pairs with B group %d byte %d; B column %d\n", l, b, row, grp, byte, col);
        }
    }
    printf("A slot (l, b): row l & 15, paired with B slots (l >> 4, b); B slot (l, b): column l & 15 -- %s (%d of 2048 slots differ)\n",
           bad ? "NOT the map found" : "confirmed for all 2048 slots", bad);
    hipFree(d);
    return bad ? 1 : 0;
}
