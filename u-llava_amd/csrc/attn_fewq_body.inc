// The body of the few-query attention, compiled into attn_fewq_kernel<HDP, FL, TPW>(AttnArgs p) in attention.hip and, with
// ULL_FEWQ_KV8 defined around the include, into attn_fewq_kv8_kernel<HDP, FL, TPW>(AttnArgs p, Kv8Args kv) in kv8.hip.  The two differ
// only where a K or V^T fragment is fetched (16-bit cache: loaded; fp8 cache: built from codes, the Sq new keys from the staging window)
// and in the fp8 form's tail, which quantizes the new keys; those places are the #ifdef arms below.  Lane mapping, MFMAs, rounding points
// and the reduction order are one text, which is what makes the fp8 form equal the 16-bit kernel on the dequantized cache bit for bit.
// A text and not a function for the reason given in sam_global_prologue.inc; and `kv` does not exist in the 16-bit kernel.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NKS = HDP / 32, NDS = HDP / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int hd = head_dim_of<HDP, FL>(p);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwv = blockDim.x >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int head = blockIdx.x;
    const int b = head / p.H, h = head % p.H;
    const int koff = p.Sk - p.Sq;
    const int nkt = (p.Sk + KT - 1) / KT;
#ifdef ULL_FEWQ_KV8
    const int w0 = koff & ~(KT - 1);                            // staging row / slot of key k >= koff: k - w0
    const long bh = head;                                       // = b * H + h
#endif
    float* red = (float*)smem;                                  // [2][16 waves][16 queries]
    float* obuf = red + 2 * 16 * 16;                            // [nwv][NDS * 4][64 lanes]

    uint4 qf[NKS];
    const int qi = fr;
    {
        const elem_t* qp = p.Q + (long)b * p.q_bs + (long)h * p.q_hs + (long)qi * p.q_ss;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = ks * 32 + fg * 8;
            qf[ks] = (qi < p.Sq && d < hd) ? *(const uint4*)(qp + d) : make_uint4(0, 0, 0, 0);
        }
        if (p.q_scale != 1.0f) {
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) qf[ks] = scale_q8(qf[ks], p.q_scale);
        }
    }
    const elem_t* kbase = p.K + (long)b * p.k_bs + (long)h * p.k_hs;
    const elem_t* vbase = p.Vt + (long)b * p.vt_bs + (long)h * p.vt_hs;

    // ---- scores of this wave's tiles -> registers (packed bf16), running max -------------------------------
    uint32_t sp[TPW][8];
    float m = -INFINITY;
#pragma clang loop unroll(full)
    for (int t = 0; t < TPW; ++t) {
        const int kt = wave + t * nwv;
        if (kt < nkt) {
#pragma unroll
            for (int ns = 0; ns < 4; ++ns) {
                const int key = min(kt * KT + ns * 16 + fr, p.Sk - 1);
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#ifdef ULL_FEWQ_KV8
                const bool old = key < koff;                    // cached key: codes; new key: staging row key - w0
                const elem_t* kp = kbase + (long)(old ? 0 : key - w0) * p.k_ss + fg * 8;
                const uint8_t* kq = kv.k8 + (bh * kv.smax + key) * hd + fg * 8;
                const float ksc = old ? kv.ks[bh * kv.smax + key] : 0.f;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    if (ks * 32 < hd) {
                        uint4 kf = make_uint4(0, 0, 0, 0);
                        if (ks * 32 + fg * 8 < hd) {
                            if (old) {
                                float f[8];
                                unpack8_w8(*(const uint2*)(kq + ks * 32), ksc, f);
                                kf = pack8(f);
                            } else {
                                kf = *(const uint4*)(kp + ks * 32);
                            }
                        }
                        acc = mfma16(kf, qf[ks], acc);
                    }
                }
#else
                const elem_t* kp = kbase + (long)key * p.k_ss + fg * 8;
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    if (ks * 32 < hd) {
                        const uint4 kf = (ks * 32 + fg * 8 < hd) ? *(const uint4*)(kp + ks * 32) : make_uint4(0, 0, 0, 0);
                        acc = mfma16(kf, qf[ks], acc);
                    }
                }
#endif
                const int j0 = kt * KT + ns * 16 + fg * 4;
                uint32_t mk = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = j0 + r;
                    uint32_t mb = 2;
                    if (j < p.Sk) mb = (p.key_mask == nullptr || p.key_mask[(long)b * p.Sk + j] != 0) ? 1 : 0;
                    mk |= mb << (8 * r);
                }
                score_quad<FL>(p, acc, j0, mk, qi, koff, nullptr, 0, 0, sp[t][ns * 2], sp[t][ns * 2 + 1]);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                m = fmaxf(m, pk_lo(sp[t][i]));
                m = fmaxf(m, pk_hi(sp[t][i]));
            }
        }
    }
    // TPW == 1: this wave's V^T operands are requested here, in flight across the barriers
#ifdef ULL_FEWQ_KV8
    uint2 vq[2][NDS];                                           // the codes and the 8 slots' scales (converted at use)
    float vsc[2][8];
    if constexpr (TPW == 1) {
        if (wave < nkt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int slot0 = wave * KT + (kk * 4 + fg) * 8;
                kv8_load_vsc(kv, bh, slot0, koff, vsc[kk]);
#pragma unroll
                for (int ds = 0; ds < NDS; ++ds)
                    if (ds * 16 < hd) vq[kk][ds] = kv8_load_vcode(kv, bh, hd, ds * 16 + fr, slot0, koff);
            }
        }
    }
#else
    uint4 vpre[2][NDS];                                         // the fragments
    if constexpr (TPW == 1) {
        if (wave < nkt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int ds = 0; ds < NDS; ++ds)
                    if (ds * 16 < hd) vpre[kk][ds] = *(const uint4*)(vbase + (long)(ds * 16 + fr) * p.vt_ds + wave * KT + (kk * 4 + fg) * 8);
        }
    }
#endif
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    if (fg == 0) red[wave * 16 + fr] = m;
    __syncthreads();
    for (int w = 0; w < nwv; ++w) m = fmaxf(m, red[w * 16 + fr]);

    // ---- exact fp32 softmax over the bf16 scores of ALL waves ----------------------------------------------
    float sum = 0.f;
#pragma clang loop unroll(full)
    for (int t = 0; t < TPW; ++t)
        if (wave + t * nwv < nkt) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                sum += __expf(pk_lo(sp[t][i]) - m);
                sum += __expf(pk_hi(sp[t][i]) - m);
            }
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (fg == 0) red[256 + wave * 16 + fr] = sum;
    __syncthreads();
    sum = 0.f;
    for (int w = 0; w < nwv; ++w) sum += red[256 + w * 16 + fr];
    const float inv = 1.0f / sum;

    // ---- partial O^T = V^T P^T over this wave's tiles --------------------------------------------------------
    f32x4_t oacc[NDS];
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) oacc[ds] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma clang loop unroll(full)
    for (int t = 0; t < TPW; ++t) {
        const int kt = wave + t * nwv;
        if (kt < nkt) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float lo = __expf(pk_lo(sp[t][i]) - m) * inv;
                const float hi = __expf(pk_hi(sp[t][i]) - m) * inv;
                sp[t][i] = pack2e(lo, hi);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const uint4 pf = make_uint4(sp[t][4 * kk], sp[t][4 * kk + 1], sp[t][4 * kk + 2], sp[t][4 * kk + 3]);
#pragma unroll
                for (int ds = 0; ds < NDS; ++ds) {
                    if (ds * 16 < hd) {
                        uint4 vf;
#ifdef ULL_FEWQ_KV8
                        const int slot0 = kt * KT + (kk * 4 + fg) * 8;
                        const elem_t* stg = vbase + (long)(ds * 16 + fr) * p.vt_ds + slot0 - w0;
                        if constexpr (TPW == 1) {
                            vf = kv8_vfrag(vq[kk][ds], vsc[kk], slot0, koff, p.Sk, stg);
                        } else {
                            if (ds == 0) kv8_load_vsc(kv, bh, slot0, koff, vsc[0]);
                            vf = kv8_vfrag(kv8_load_vcode(kv, bh, hd, ds * 16 + fr, slot0, koff), vsc[0], slot0, koff, p.Sk, stg);
                        }
#else
                        if constexpr (TPW == 1) vf = vpre[kk][ds];
                        else vf = *(const uint4*)(vbase + (long)(ds * 16 + fr) * p.vt_ds + kt * KT + (kk * 4 + fg) * 8);
#endif
                        oacc[ds] = mfma16(vf, pf, oacc[ds]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds)
#pragma unroll
        for (int r = 0; r < 4; ++r) obuf[(wave * NDS * 4 + ds * 4 + r) * 64 + lane] = oacc[ds][r];
    __syncthreads();
    // element e = (ds*4 + r)*64 + lane  <->  O[query lane & 15][d = ds*16 + 4*(lane >> 4) + r]
    for (int e = tid; e < NDS * 4 * 64; e += blockDim.x) {
        float acc = 0.f;
        for (int w = 0; w < nwv; ++w) acc += obuf[w * NDS * 4 * 64 + e];
        const int reg = e >> 6, ln = e & 63;
        const int q = ln & 15, d = (reg >> 2) * 16 + (ln >> 4) * 4 + (reg & 3);
        if (q < p.Sq && d < hd) p.O[(long)b * p.o_bs + (long)h * p.o_hs + (long)q * p.o_ss + d] = f2e(acc);
    }
#ifdef ULL_FEWQ_KV8
    // the new keys into the cache: vector 2i = K row of key koff + i, 2i + 1 = its V column; one wave per vector
    for (int v = wave; v < 2 * p.Sq; v += nwv) {
        const int key = koff + (v >> 1);
        if ((v & 1) == 0) {
            kv8_quant_vec(kbase + (long)(key - w0) * p.k_ss, 1, hd, kv.k8 + (bh * kv.smax + key) * hd, 1, kv.ks + bh * kv.smax + key, lane);
        } else {
            const int slot = kv8_slot(key);
            kv8_quant_vec(vbase + (slot - w0), p.vt_ds, hd, kv.vt8 + bh * hd * kv.smax + slot, kv.smax, kv.vs + bh * kv.smax + slot, lane);
        }
    }
#endif
