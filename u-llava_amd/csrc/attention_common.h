// Declarations shared by the attention kernels (attention.hip) and the fp8 KV-cache attention (kv8.hip): the argument block, the score
// flavors and their rounding chain, and the small operand helpers.  Everything is internal to the translation unit that includes it.
#pragma once
#include "ull_common.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int KT = 64;                 // keys per tile

struct AttnArgs {
    const elem_t* Q; const elem_t* K; const elem_t* Vt; elem_t* O;
    const int32_t* key_mask;            // [B, Sk] nonzero = may be attended, or null
    long q_bs, q_hs, q_ss, k_bs, k_hs, k_ss, vt_bs, vt_hs, vt_ds, o_bs, o_hs, o_ss;
    int B, H, Sq, Sk, hd, vt_len;
    int causal, scale_mode;
    float scale;
    const elem_t* zeros;                // >= 16 readable zero bytes (source of the head-dim padding chunks)
    // SAM decomposed relative-position bias (image_encoder.py:354-392): S += rel_h[q, key / KW]; S += rel_w[q, key % KW]
    const elem_t* rel_h; const elem_t* rel_w;   // [B*H, Sq, KH] / [B*H, Sq, KW] or null
    int KH, KW;
    int rel_mode;                       // 1: rel_h/rel_w are per-query tables [B*H,Sq,KH|KW]; 2: they are the raw rel_pos_h/w parameters
    int win16;                          // ull_sam_window_attention: sam_window_kernel, see below
    uint32_t mg_h, mg_nwx, mg_nwy, mg_nw;   // win16: ceil(2^32 / d) for d = H, nwx, nwy, nwx * nwy (udiv_magic: no run-time integer division in the kernel)
    int v_rows;                         // Vt is V itself, [B,H,S,hd] by (vt_bs, vt_hs, vt_ds = token stride): kernels with a VROW form
                                        //    [2KH-1,hd] / [2KW-1,hd] and the tables are built in the kernel prologue on the MFMA
    float inv_kw;                       // 1 / KW
    float q_scale;                      // != 1: Q is consumed as bf16(q * q_scale)  (SAM: (q * scale) @ k^T)
    // win16 (ull_sam_window_attention): Q / K / V / O rows are tokens of [img, img_h, img_w] grids in image order, "batch" b is
    // window (img, wy, wx) of the 14 x 14 partition, Vt points at the V part of the rows (same strides as K), and window positions
    // outside the grid are the reference's zero padding (image_encoder.py:262-289 pads AFTER norm1, so a padded token's q|k|v is
    // the qkv bias): K / V rows of such keys come from k_pad / v_pad.
    int img_h, img_w, nwy, nwx;
    const elem_t* k_pad; const elem_t* v_pad;   // K / V part of the pad token's row (+ h * k_hs)
};
#define ULL_ATT_ACC(slot, t0) ((void)0)

// The argument block of a C entry point: the four tensors with their (batch, head, row) strides in elements and the shape; every other
// field zero / null (no mask, not causal, scale_mode 0, no rel-pos bias, V^T form with vt_len 0, no windows) except scale = q_scale = 1.
// The entry sets what it uses on top.
struct AttnTensor { const void* ptr; int64_t bs, hs, ss; };
inline AttnArgs attn_args(AttnTensor q, AttnTensor k, AttnTensor vt, AttnTensor o, int64_t B, int64_t H, int64_t Sq, int64_t Sk, int64_t hd) {
    AttnArgs a{};
    a.Q = (const elem_t*)q.ptr; a.K = (const elem_t*)k.ptr; a.Vt = (const elem_t*)vt.ptr; a.O = (elem_t*)o.ptr;
    a.q_bs = q.bs; a.q_hs = q.hs; a.q_ss = q.ss; a.k_bs = k.bs; a.k_hs = k.hs; a.k_ss = k.ss;
    a.vt_bs = vt.bs; a.vt_hs = vt.hs; a.vt_ds = vt.ss; a.o_bs = o.bs; a.o_hs = o.hs; a.o_ss = o.ss;
    a.B = (int)B; a.H = (int)H; a.Sq = (int)Sq; a.Sk = (int)Sk; a.hd = (int)hd;
    a.scale = a.q_scale = 1.0f;
    return a;
}

// ull_sam_window_attention: window b = (img * nwy + wy) * nwx + wx -> (image, first token row, first token column).  The divisors are
// run-time values; a / d goes through the host-computed m = ceil(2^32 / d): exact while a * d < 2^32 (the dispatcher checks), m = 0
// encodes d = 1.  (As three integer divisions, ~30 scalar instructions each and repeated per DMA piece, this was ~1200 scalar
// instructions in every wave's prologue.)
struct WinOrigin { int img, iy0, ix0; };
ULL_DEV int udiv_magic(int a, uint32_t m) { return m ? (int)__umulhi((uint32_t)a, m) : a; }
ULL_DEV WinOrigin win_origin(const AttnArgs& p, int b, int ws) {
    const int t = udiv_magic(b, p.mg_nwx), wx = b - t * p.nwx;
    const int img = udiv_magic(b, p.mg_nw), wy = t - img * p.nwy;
    return WinOrigin{img, wy * ws, wx * ws};
}

// Compile-time "flavors" of the score epilogue.  The runtime-flag version (FL_RUNTIME) costs ~6 wave-uniform branches per
// score element, which fragments the schedule (measured: SAM global attention 12 ms -> see profiles/); the hot callers
// get straight-line code instead.
constexpr int FL_RUNTIME = -1;   // every switch read from AttnArgs at run time (any combination)
constexpr int FL_LLAMA = 0;      // S*scale, causal + key-padding mask            (hf llama eager_attention_forward)
constexpr int FL_CLIP = 1;       // S*scale                                        (hf clip eager_attention_forward)
constexpr int FL_SAM_ENC = 2;    // (q*scale) pre-scaled, + rel_h, + rel_w         (SAM image_encoder.py Attention)
constexpr int FL_SAM_DEC = 3;    // S / sqrt(hd)                                   (SAM transformer.py Attention)

// One lane's 4 consecutive scores of one query -> the reference's rounding chain -> two packed bf16 pairs.
//   acc[r] = raw fp32 dot product for key j0 + r;  mk = 4 mask bytes (1 attend, 0 masked, 2 out of range)
//   brow   = this query's bias row in LDS, rel_h(kh) = brow[bh_off - kh], rel_w(kw) = brow[bw_off - kw]; or null
template <int FL>
ULL_DEV void score_quad(const AttnArgs& p, const f32x4_t& acc, int j0, uint32_t mk, int qi, int koff, const elem_t* brow, int bh_off,
                        int bw_off, uint32_t& lo, uint32_t& hi, float* row_max = nullptr) {
    const bool do_mul = FL == FL_RUNTIME ? p.scale_mode == 1 : (FL == FL_LLAMA || FL == FL_CLIP);
    const bool do_div = FL == FL_RUNTIME ? p.scale_mode == 2 : (FL == FL_SAM_DEC);
    const bool do_bias = FL == FL_RUNTIME ? brow != nullptr : (FL == FL_SAM_ENC);
    const bool do_causal = FL == FL_RUNTIME ? p.causal != 0 : (FL == FL_LLAMA);
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + r;
        float sv = rnd(acc[r]);
        if (do_mul) sv = rnd(sv * p.scale);
        if (do_div) sv = rnd(sv / p.scale);
        if (do_bias) {
            // j / KW without the integer-division sequence: exact for j < 2^16, KW <= 256 (|err| << 0.5 / KW)
            const int kh = min((int)(((float)j + 0.5f) * p.inv_kw), p.KH - 1), kw = j - kh * p.KW;
            sv = rnd(rnd(sv + e2f(brow[bh_off - kh])) + e2f(brow[bw_off - kw]));
        }
        const uint32_t mb = (mk >> (8 * r)) & 0xff;
        const bool allowed = (mb == 1) && (!do_causal || j <= qi + koff);
        o[r] = (mb == 2) ? -INFINITY : (allowed ? sv : ELEM_MIN_F);   // -inf / finfo(bf16).min, exact in bf16
    }
    if (row_max) *row_max = fmaxf(fmaxf(*row_max, fmaxf(o[0], o[1])), fmaxf(o[2], o[3]));   // values are already 16-bit exact
    lo = pack2e(o[0], o[1]);
    hi = pack2e(o[2], o[3]);
}

// The same for a quad whose four keys are all attendable for every lane of the wave (no padding, below the causal diagonal, no
// bias): only the scale + the two roundings remain.  ~85 % of the LLaMA / CLIP score quads take this path.
// LLaMA / CLIP (S * scale): rnd(acc) two at a time through one packed convert, the scale as one packed multiply, and -- rounding to 16
// bits is monotone, so max_i rnd(x_i) = rnd(max_i x_i) -- the row maximum is fed with the UNROUNDED products (one v_max3 per pair instead
// of two unpacks and two v_max); the caller rounds the row maximum once.  11 vector instructions per quad instead of 26, same bits.
template <int FL>
ULL_DEV void score_quad_clean(const AttnArgs& p, const f32x4_t& acc, uint32_t& lo, uint32_t& hi, float* row_max = nullptr) {
    if constexpr (FL == FL_LLAMA || FL == FL_CLIP) {
        // (the packed pairs are made opaque: seeing through pack -> unpack, the compiler converts every value on its own again --
        //  4 single conversions + 4 shifts instead of 2 packed conversions + 2 shifts + 2 ands; census in profiles/r05_attn_prefill_census.txt)
        uint32_t a01 = pack2e(acc[0], acc[1]), a23 = pack2e(acc[2], acc[3]);
        asm volatile("" : "+v"(a01), "+v"(a23));
        const f32x2_t x01 = f32x2_t{pk_lo(a01), pk_hi(a01)} * p.scale, x23 = f32x2_t{pk_lo(a23), pk_hi(a23)} * p.scale;
        if (row_max) *row_max = fmaxf(fmaxf(fmaxf(*row_max, x01.x), x01.y), fmaxf(x23.x, x23.y));
        lo = pack2e(x01.x, x01.y);
        hi = pack2e(x23.x, x23.y);
        return;
    }
    const bool do_mul = FL == FL_RUNTIME ? p.scale_mode == 1 : false;
    const bool do_div = FL == FL_RUNTIME ? p.scale_mode == 2 : (FL == FL_SAM_DEC);
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float sv = rnd(acc[r]);
        if (do_mul) sv = rnd(sv * p.scale);
        if (do_div) sv = rnd(sv / p.scale);
        o[r] = sv;
    }
    if (row_max) *row_max = fmaxf(fmaxf(*row_max, fmaxf(o[0], o[1])), fmaxf(o[2], o[3]));
    lo = pack2e(o[0], o[1]);
    hi = pack2e(o[2], o[3]);
}


// SAM 14 x 14 windows (sam_window_kernel): one lane's scores of window row kh for its four window columns kw = 4 fg + r:
// rnd(rnd(rnd(acc) + rel_h[kh]) + rel_w[kw]), the reference's three roundings, two values at a time: one packed convert rounds a pair, the
// two adds are one packed add, the third rounding IS the packed pair that is kept, and the row maximum takes the unrounded sums (rounding
// is monotone; the caller rounds the maximum once).  wv23 = -inf in the lanes whose columns are the padding slots kw = 14, 15.
// 21 vector instructions per window row instead of 45, same bits (the kernel is bound by its vector-issue slots: docs/experiments.md).
ULL_DEV void score_quad_win(const f32x4_t& acc, float hb, const f32x2_t& wv01, const f32x2_t& wv23, uint32_t& lo, uint32_t& hi, float& row_max) {
    // (the packed pairs are made opaque: seeing through pack -> unpack, the compiler converts every value on its own again)
    uint32_t a01 = pack2e(acc[0], acc[1]), a23 = pack2e(acc[2], acc[3]);
    asm volatile("" : "+v"(a01), "+v"(a23));
    const f32x2_t x01 = f32x2_t{pk_lo(a01), pk_hi(a01)} + hb, x23 = f32x2_t{pk_lo(a23), pk_hi(a23)} + hb;
    uint32_t b01 = pack2e(x01.x, x01.y), b23 = pack2e(x23.x, x23.y);
    asm volatile("" : "+v"(b01), "+v"(b23));
    const f32x2_t y01 = f32x2_t{pk_lo(b01), pk_hi(b01)} + wv01, y23 = f32x2_t{pk_lo(b23), pk_hi(b23)} + wv23;
    row_max = fmaxf(fmaxf(fmaxf(row_max, y01.x), y01.y), fmaxf(y23.x, y23.y));
    lo = pack2e(y01.x, y01.y);
    hi = pack2e(y23.x, y23.y);
    asm volatile("" : "+v"(lo), "+v"(hi));
}

// ... and the exact fp32 softmax over the lane's 56 scores (14 window rows x 4 columns; the row's other 168 sit in the lanes fr, fr + 16,
// fr + 32, fr + 48): every exponential is evaluated once and kept, subtraction / log2(e) / normalisation are packed fp32 operations.
// mrow = the lane's running maximum from score_quad_win.  P = 16-bit softmax, in place.
ULL_DEV void softmax_win(uint32_t (&sp)[4][8], float mrow) {
    float m = rnd(mrow);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
    f32x2_t e[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) {
        const f32x2_t t = (f32x2_t{pk_lo(sp[i / 8][i % 8]), pk_hi(sp[i / 8][i % 8])} - m) * 1.4426950408889634f;   // __expf(x) = exp2(x * log2 e)
        e[i] = f32x2_t{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
        sum += e[i].x;
        sum += e[i].y;
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 28; ++i) {
        const f32x2_t q = e[i] * inv;
        sp[i / 8][i % 8] = pack2e(q.x, q.y);
    }
}

// Stage this wave's 16 relative-position bias rows in LDS (`dst`, row pitch `bp` elements, see bias_pitch()).
//   rel_mode 1: copy the precomputed per-query tables (stored reversed so both modes index the same way);
//   rel_mode 2: build them here: G[q][t] = bf16(q . rel_pos[t]) for every table row t on the MFMA (the reference's
//               einsum("bhwc,hkc->bhwk") is a Toeplitz slice of exactly this product: rel_h[q][kh] = Gh[q][qy - kh + KH - 1]).
// qf0 = the wave's UNSCALED query fragments.  Returns the two lookup offsets of this lane's query.
template <int NKS>
ULL_DEV void stage_rel_bias(const AttnArgs& p, elem_t* dst, int bp, const uint4 (&qf0)[NKS], int q_first, long head, int lane,
                            int& bh_off, int& bw_off, int hd) {
    const int fr = lane & 15, fg = lane >> 4;
    const int qi = min(q_first + fr, p.Sq - 1);
    if (p.rel_mode == 1) {
        const int bw = p.KH + p.KW;
        for (int i = lane; i < 16 * bw; i += 64) {
            const int r = i / bw, c = i % bw;
            const long row = head * p.Sq + min(q_first + r, p.Sq - 1);
            if (c < p.KH) dst[r * bp + (p.KH - 1 - c)] = p.rel_h[row * p.KH + c];
            else dst[r * bp + p.KH + (p.KW - 1 - (c - p.KH))] = p.rel_w[row * p.KW + (c - p.KH)];
        }
        bh_off = p.KH - 1;
        bw_off = p.KH + p.KW - 1;
    } else {
        const int nth = 2 * p.KH - 1, ntw = 2 * p.KW - 1;
        if (nth <= 32 && ntw <= 32) {
            // window-sized tables (14 x 14 -> 27 rows each): all 4 x NKS table fragments are requested before the first MFMA, so the
            // block pays one memory round trip here instead of four dependent ones (this prologue was ~1/4 of a window block's time)
            uint4 a[2][2][NKS];
#pragma unroll
            for (int which = 0; which < 2; ++which)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const elem_t* tab = which ? p.rel_w : p.rel_h;
                    const int nt = which ? ntw : nth;
                    const int t = min(st * 16 + fr, nt - 1);
#pragma unroll
                    for (int ks = 0; ks < NKS; ++ks) {
                        const int d = ks * 32 + fg * 8;
                        a[which][st][ks] = (d < hd) ? *(const uint4*)(tab + (long)t * hd + d) : make_uint4(0, 0, 0, 0);
                    }
                }
#pragma unroll
            for (int which = 0; which < 2; ++which)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const int nt = which ? ntw : nth, base = which ? nth : 0;
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < NKS; ++ks)
                        if (ks * 32 < hd) acc = mfma16(a[which][st][ks], qf0[ks], acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int tt = st * 16 + fg * 4 + r;
                        if (tt < nt) dst[fr * bp + base + tt] = f2e(acc[r]);
                    }
                }
        } else
#pragma unroll 1
        for (int which = 0; which < 2; ++which) {
            const elem_t* tab = which ? p.rel_w : p.rel_h;
            const int nt = which ? ntw : nth, base = which ? nth : 0;
            for (int st = 0; st * 16 < nt; ++st) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                const int t = min(st * 16 + fr, nt - 1);
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const int d = ks * 32 + fg * 8;
                    if (ks * 32 < hd) {
                        const uint4 a = (d < hd) ? *(const uint4*)(tab + (long)t * hd + d) : make_uint4(0, 0, 0, 0);
                        acc = mfma16(a, qf0[ks], acc);
                    }
                }
                // acc[r] = G[t = st*16 + 4*fg + r][query fr]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tt = st * 16 + fg * 4 + r;
                    if (tt < nt) dst[fr * bp + base + tt] = f2e(acc[r]);
                }
            }
        }
        bh_off = qi / p.KW + p.KH - 1;
        bw_off = nth + qi % p.KW + p.KW - 1;
    }
}

__host__ ULL_DEV int bias_pitch(const AttnArgs& p) {       // elements; odd so the 16 query rows start in different LDS banks
    const int n = p.rel_mode == 2 ? (2 * p.KH - 1) + (2 * p.KW - 1) : p.KH + p.KW;
    return n | 1;
}
// ... and the LDS bytes the launcher adds for them: 16 rows per wave (+ 16: the rows start at the next 16-byte boundary)
inline int rel_bias_lds_bytes(const AttnArgs& a, int nwv) { return a.rel_h ? nwv * 16 * bias_pitch(a) * 2 + 16 : 0; }

// Launch of the few-query kernels (attn_fewq_kernel; attn_fewq_kv8_kernel with extra = its Kv8Args), one block per (batch, head): one
// wave per key tile up to 16 waves, which then hold TPW = 1 tile each in registers (KERNEL_TPW1); beyond 16 tiles 16 waves with TPW = 4
// (KERNEL_TPW4, <= 64 tiles).  LDS: the two reductions' [16 waves][16 queries] floats and one partial O per wave.
template <auto KERNEL, int HDP, typename... Extra>
int launch_fewq_block(const AttnArgs& a, int nwv, hipStream_t st, const Extra&... extra) {
    const int lds = 2 * 16 * 16 * 4 + nwv * HDP * 16 * 4;
    static UllOncePerDevice once;                               // (one per kernel: KERNEL is a template argument)
    if (once.first()) (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(KERNEL, dim3(a.B * a.H), dim3(nwv * 64), lds, st, a, extra...);
    return ull_check_launch();
}
template <auto KERNEL_TPW1, auto KERNEL_TPW4, int HDP, typename... Extra>
int launch_fewq_as(const AttnArgs& a, hipStream_t st, const Extra&... extra) {
    const int nt = (a.Sk + KT - 1) / KT;
    const int nwv = nt < 16 ? nt : 16;
    return nt <= 16 ? launch_fewq_block<KERNEL_TPW1, HDP>(a, nwv, st, extra...) : launch_fewq_block<KERNEL_TPW4, HDP>(a, nwv, st, extra...);
}

ULL_DEV uint4 scale_q8(const uint4& v, float sc) {
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= sc;
    return pack8(f);
}

// LDS-DMA of 64 x 16 B (see gemm_bf16.hip: issued via inline asm so hipcc does not drain it before the next ds_read).
// the same with a wave-uniform base and a 32-bit per-lane byte offset (saddr form): the per-lane part is computed once per kernel
ULL_DEV void glds16s(const void* sbase /* wave-uniform */, uint32_t voff, uint32_t lds_byte_addr /* wave-uniform */) {
    uint32_t keep;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);   // make uniformity provable to the compiler
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(dst) : "memory");
}
ULL_DEV void glds16(const void* gsrc, uint32_t lds_byte_addr /* wave-uniform */) {
    uint32_t keep;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);   // make uniformity provable to the compiler
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

// XOR swizzle of the 16-byte chunk index inside an LDS tile row (CPR chunks per row): chosen so that the 16 rows a
// ds_read_b128 lane group touches land on 16 different bank slots.
template <int CPR>
ULL_DEV int swz(int row) { return CPR >= 16 ? (row & 15) : CPR == 8 ? (row & 7) : ((row >> 2) & 3); }

// Head dim as a compile-time constant where the flavor pins it (flavor_of() checks the argument): the `ks * 32 < hd` /
// `ds * 16 < hd` tests that skip pure-padding MFMAs then fold away.  With a run-time hd every MFMA sits in its own basic
// block behind an s_waitcnt (seen in the ISA of the first version of these kernels).
template <int HDP, int FL>
ULL_DEV int head_dim_of(const AttnArgs& p) {
    if constexpr (FL == FL_LLAMA || FL == FL_CLIP) return HDP;
    else if constexpr (FL == FL_SAM_ENC && HDP == 128) return 80;
    else return p.hd;
}

}  // namespace
