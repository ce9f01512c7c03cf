"""GPU: MXFP8 activations in batched decode steps on mxfp4 weights (ops.linear_w4a8_skinny / ull_gemm_skinny_w4a8_bf16,
ops.rmsnorm_quantize_rows_mxfp8 / ull_rmsnorm_quantize_rows_mxfp8_bf16, quantize_weights("mxfp4", decode_activations="mxfp8_e4m3"), DESIGN f20).

  1. the fused norm + quantize equals the composition of the existing ops, codes and scale bytes, bit for bit;
  2. the GEMM kernel equals the 128 x 128 W4A8 GEMM and the W4A16 Linear bit for bit on data where every fp32 partial sum is exact
     (tests/test_w4a8_gpu.py `_act` x `_wgt`: the summation order cannot matter), 3. with SwiGLU, 4. on strided operands;
  5. on Gaussian data a row / a column block does not depend on M, N or the other rows (the order is a function of K alone);
  6. on Gaussian data it is within the any-order fp32 accumulation bound of the fp64 restatement (tests/test_w4a8_cpu.py `w4a8_exact`);
  7. model level, on a seeded random-init core whose layer Linears are on the routing rule (N * K >= 2^22).
"""
import pytest
import torch

from helpers import load_fixture, pkg
from test_a8_decode_gpu import HEADS, HID, INTER, LAYERS, PROMPT, VOCAB, _ids, _spy, _steps
from test_w4a8_cpu import w4a8_exact
from test_w4a8_gpu import _act, _dequant_rows, _wgt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
MS = (1, 5, 16, 17, 32)


def _quant(ops, x):
    """(codes, scale bytes) as the W4A8 kernels read them."""
    return ops._quantize_rows_mxfp8(x, x.shape[-1])


# ---- 1. fused RMSNorm + row quantization ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["gauss", "zeros"])
@pytest.mark.parametrize("M,K", [(1, 128), (5, 4096), (32, 4096), (7, 11008), (9, 2816)])
def test_fused_norm_quantize_equals_the_composition(M, K, data):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(100 * M + K)
    x = torch.randn(M, K, generator=g) * 3.0
    x[:, ::501] *= 40.0                                            # activation outliers
    w = 1.0 + 0.1 * torch.randn(K, generator=g)
    w[K // 3] = 56.0
    if data == "zeros":
        x[0, 32:64] = 0                                            # an all-zero block
        x[-1, K - 32:] = 0
        if M >= 5:
            x[1] = 0                                               # an all-zero row
    eps = 1e-6
    xw = torch.zeros(M, K + 72, dtype=BF)
    xw[:, :K] = x.to(BF)
    xw, w = xw.to(DEV), w.to(BF).to(DEV)
    for xs_ in (xw[:, :K].contiguous(), xw[:, :K]):                # contiguous, and rows of a wider buffer (ldx = K + 72)
        want_c, want_s = _quant(ops, ops.rmsnorm(xs_, w, eps))
        got_c, got_s = ops.rmsnorm_quantize_rows_mxfp8(xs_, w, eps)
        assert got_c.shape == (M, K) and got_c.dtype == torch.uint8 and got_s.shape == want_s.shape == (M, K // 32) and got_s.dtype == torch.uint8
        assert torch.equal(got_s, want_s), f"scale bytes: {int((got_s != want_s).sum())} of {got_s.numel()} differ"
        assert torch.equal(got_c, want_c), f"codes: {int((got_c != want_c).sum())} of {got_c.numel()} differ"
        assert bool(got_c.any()) and len(set(got_s.flatten().tolist())) > 1
        if data == "zeros":
            assert not bool(got_c[0, 32:64].any()) and int(got_s[0, ops._mx_perm(K, DEV)[1][1]]) == 127, "the all-zero block: scale 2^0, zero codes"
            if M >= 5:
                assert not bool(got_c[1].any()) and bool((got_s[1] == 127).all()), "the all-zero row"


# ---- 2. the GEMM kernel, bit for bit on exactly summable data ----------------------------------------------------------------------------
# (N, K): tail only, seven idle waves / a partial block / one superblock, four units over eight waves / a superblock plus one tail tile /
# one superblock + six tail tiles / five superblocks + six tail tiles / the full grid, one super tile per wave
@pytest.mark.parametrize("N,K", [(16, 128), (40, 384), (200, 2048), (48, 2176), (48, 2816), (48, 11008), (4096, 4096)])
def test_kernel_equals_existing_paths_bit_for_bit(N, K):
    ops = pkg("ops")
    w = _wgt(N, K, 2000 + N)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize(q), w), "the weights are exact in MXFP4"
    for M in MS:
        x = _act(M, K, 1000 + M, special=True)
        xd = _dequant_rows(ops, x)
        assert torch.equal(xd, x), "the activations are exact in MXFP8"
        xq, xsc = _quant(ops, x)
        assert K < 256 or len(set(xsc.flatten().tolist())) > 2, "block scales vary"
        r = _act(M, N - N % 32 + 32, 3000 + M)[:, :N].contiguous()
        with torch.no_grad():
            for kw, what in ((dict(), "no epilogue"), (dict(residual=r), "residual"), (dict(out_f32=True), "fp32 output")):
                got = ops.linear_w4a8_skinny(xq, xsc, q, **kw)
                assert got.shape == (M, N) and got.dtype == (torch.float32 if kw.get("out_f32") else BF)
                assert torch.equal(got, ops.linear_w4a8(x, q, **kw)), f"M = {M}, {what}: against the 128 x 128 W4A8 GEMM"
                assert torch.equal(got, ops.linear(xd, q, **kw)), f"M = {M}, {what}: against the W4A16 Linear on the dequantized rows"
            out = ops.linear_w4a8_skinny(xq, xsc, q)
            assert bool(out.float().abs().sum() > 0)
            if M > 5:
                assert not bool(out[3].any()), "the all-zero row gives zeros"


# ---- 3. SwiGLU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 128), (288, 2176), (320, 4096)])
def test_kernel_swiglu_equals_existing_paths_bit_for_bit(N, K):
    ops = pkg("ops")
    # |gate| stays below 80 (the shared SiLU code returns NaN where exp(-gate) overflows): |x| <= 2^9, |w| <= 12 * 2^(3 - 22), K <= 4096:
    # |gate| <= 4096 * 2^9 * 12 * 2^-19 = 48 whatever the signs
    q = ops.quantize_mxfp4(_wgt(N, K, 5000 + N, mag=-22))
    for M in MS:
        x = _act(M, K, 4000 + M, special=True)
        assert torch.equal(_dequant_rows(ops, x), x), "the activations are exact in MXFP8: ops.linear on x is the W4A16 path"
        with torch.no_grad():
            a = ops.linear_w4a8_skinny(*_quant(ops, x), q, swiglu=True)
            assert bool(torch.isfinite(a.float()).all()) and float(ops.linear(x, q).float().abs().max()) < 80.0
            assert a.shape == (M, N // 2) and torch.equal(a, ops.linear_w4a8(x, q, swiglu=True)), f"M = {M}: against the W4A8 GEMM"
            assert torch.equal(a, ops.linear(x, q, swiglu=True)), f"M = {M}: against the W4A16 Linear"
            assert bool(a.float().abs().sum() > 0)


# ---- 4. strided operands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [5, 16, 17, 32])
def test_kernel_strided_codes_scales_output_and_residual(M):
    ops = pkg("ops")
    N, K = 200, 384
    x = _act(M, K, 6000 + M)
    q = ops.quantize_mxfp4(_wgt(N, K, 6001))
    xq, xsc = _quant(ops, x)
    wide = torch.full((M, K + 64), 0x7e, device=DEV, dtype=torch.uint8)            # (0x7e = 448: garbage the kernel must not read into the sum)
    wide[:, :K] = xq
    wsc = torch.full((M, K // 32 + 8), 0xfe, device=DEV, dtype=torch.uint8)        # (0xfe = 2^127 beyond the row's K / 32 scale bytes)
    wsc[:, :K // 32] = xsc
    want = ops.linear(x, q)
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_w4a8_skinny(wide[:, :K], wsc[:, :K // 32], q, out=outw[:, :N])      # ldxq = K + 64, ldxs = K / 32 + 8, ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"
    r = _act(M, N + 24, 6002)[:, :N]                                               # a strided residual
    assert torch.equal(ops.linear_w4a8_skinny(wide[:, :K], wsc[:, :K // 32], q, residual=r), ops.linear(x, q, residual=r.contiguous()))
    o32 = torch.full((M, N + 8), 7.0, device=DEV, dtype=torch.float32)
    ops.linear_w4a8_skinny(wide[:, :K], wsc[:, :K // 32], q, out=o32[:, :N], out_f32=True)
    assert torch.equal(o32[:, :N], ops.linear(x, q, out_f32=True)) and bool((o32[:, N:] == 7.0).all())


# ---- 5. the summation order is a function of K alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4096, 11008])
def test_result_does_not_depend_on_m_n_or_the_other_rows(K):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(32, K, generator=g).to(BF).to(DEV)
    q = ops.quantize_mxfp4((torch.randn(200, K, generator=g) * 0.02).to(BF).to(DEV))
    xq, xsc = _quant(ops, x)
    full = ops.linear_w4a8_skinny(xq, xsc, q, out_f32=True)
    part = ops.linear_w4a8_skinny(xq[3:8], xsc[3:8], q, out_f32=True)              # the second fragment's kernel against the first's
    assert torch.equal(full[3:8], part), "rows 3 .. 7 of an M = 32 call against an M = 5 call"
    cols = ops.linear_w4a8_skinny(xq, xsc, ops.Mxfp4Weight(q.codes[16:32], q.scales[16:32], K), out_f32=True)
    assert cols.shape == (32, 16) and torch.equal(full[:, 16:32], cols), "column block 16 .. 31 of N = 200 against N = 16"
    assert torch.equal(ops.linear_w4a8_skinny(xq, xsc, q)[3:8], ops.linear_w4a8_skinny(xq[3:8], xsc[3:8], q))
    assert bool(full.abs().sum() > 0)


# ---- 6. Gaussian data against the fp64 restatement -------------------------------------------------------------------------------------------
def test_kernel_random_data_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 32, 520, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02)
    w[::97] *= 8.0
    q = ops.quantize_mxfp4(w.to(BF).to(DEV))
    wc, ws = (t.cpu() for t in q.to_standard())
    xq, xsc = _quant(ops, x.to(DEV))
    out = ops.linear_w4a8_skinny(xq, xsc, q).cpu().double()
    y, absum = w4a8_exact(x, wc, ws)
    # K * 2^-23 * sum |terms|: fp32 accumulation in any order; 2^-8 |y|: the final rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -8 * y.abs()
    err = (out - y).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y| = {float(y.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"
    f32 = ops.linear_w4a8_skinny(xq, xsc, q, out_f32=True).cpu().double()
    e32 = (f32 - y).abs()
    print(f"fp32 output: max err / accumulation bound = {float((e32 / (K * 2.0 ** -23 * absum).clamp_min(1e-300)).max()):.4f}")
    assert bool((e32 <= K * 2.0 ** -23 * absum).all()), "fp32 output: the accumulation bound alone"


# ---- 7. model level -----------------------------------------------------------------------------------------------------------------------
def _core(activations=None, decode_activations=None):
    """test_a8_decode_gpu's seeded random-init core (about 70 M weights) quantized to mxfp4: the same weights for every mode."""
    C, M = pkg("configuration"), pkg("modeling_core")
    cd = load_fixture("g1_core_tiny_bf16.pt")["cfg"]
    cfg = C.UllavaCoreConfig(vision_config=cd["vision_config"], vision_hidden_layer=-2, mm_token_ids=cd["mm_token_ids"], vocab_size=VOCAB,
                             hidden_size=HID, intermediate_size=INTER, num_hidden_layers=LAYERS, num_attention_heads=HEADS)
    model = M.UllavaCoreForCausalLM(cfg, device=DEV)
    g = torch.Generator().manual_seed(1234)
    for name, p in sorted(model.named_parameters()):
        if p.dim() == 1 and ("norm" in name or "ln" in name) and "bias" not in name:
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        elif p.dim() == 1:
            v = 0.02 * torch.randn(p.shape, generator=g)
        else:
            v = 0.03 * torch.randn(p.shape, generator=g)
        p.data.copy_(v.to(BF))
    model.quantize_weights("mxfp4", activations=activations, decode_activations=decode_activations)
    return model


NEW = "mxfp8_e4m3"


@pytest.fixture(scope="module")
def models():
    with torch.no_grad():
        m = dict(w4=_core(), a8=_core("mxfp8_e4m3"), d8=_core(), a4d8=_core("mxfp4_e2m1", NEW))
        assert m["d8"].decode_activation_quantization is None
        assert m["d8"].quantize_weights("mxfp4", decode_activations=NEW) is m["d8"]        # switched on for an already quantized model
    assert m["w4"].decode_activation_quantization is None and m["a8"].decode_activation_quantization is None
    assert m["d8"].decode_activation_quantization == NEW and m["d8"].activation_quantization is None
    assert m["a4d8"].decode_activation_quantization == NEW and m["a4d8"].activation_quantization == "mxfp4_e2m1"
    assert all(v.weight_quantization == "mxfp4" and v.activation_scope == "prefill" for v in m.values())
    ops = pkg("ops")
    for a, b in zip(m["w4"]._packed["llama"], m["d8"]._packed["llama"]):
        for k in ("w_qkv", "w_o", "w_gu", "w_down"):
            assert torch.equal(a[k].codes, b[k].codes) and torch.equal(a[k].scales, b[k].scales), "no weight change"
            assert all(ops.linear_route(B, b[k], ops.ActQuant(None, False, NEW)) == "w4a8_skinny" for B in (8, 32)), "the layer Linears are on the rule"
    return m


def _filled_caches(models, B, n):
    """n identical KV caches, each filled by the W4A16 model's prefill of the same prompts, and the next token of every row."""
    pf = [models["w4"](input_ids=_ids(B), use_cache=True) for _ in range(n)]
    assert all(torch.equal(pf[0].logits, p.logits) for p in pf[1:])
    return [p.past_key_values for p in pf], pf[0].logits[:, -1].argmax(-1, keepdim=True)


GEMM, NORMQ, ROWQ = "ull_gemm_skinny_w4a8_bf16", "ull_rmsnorm_quantize_rows_mxfp8_bf16", "ull_quantize_rows_mxfp8_bf16"
SKINNY, GEMM128, GEMM128_A4 = "ull_gemm_skinny_wq_bf16", "ull_gemm_w4a8_bf16", "ull_gemm_w4a4_bf16"


@pytest.mark.parametrize("B", [8, 32])
def test_decode_step_takes_the_new_entries_only_under_the_new_mode(models, monkeypatch, B):
    with torch.no_grad():
        caches, tok = _filled_caches(models, B, 4)
        names = _spy(monkeypatch)
        for i, which in enumerate(("d8", "a4d8")):
            del names[:]
            models[which](input_ids=tok, past_key_values=caches[i], use_cache=True)
            assert names.count(GEMM) == 4 * LAYERS and names.count(NORMQ) == 2 * LAYERS, which
            assert names.count(ROWQ) == 2 * LAYERS, "o_proj and down_proj quantize their inputs in a launch of their own"
            assert names.count(SKINNY) == 0 and names.count(GEMM128) == 0 and names.count(GEMM128_A4) == 0, which
            assert names.count("ull_rmsnorm_bf16") == 1, "(the final norm)"
            assert names.count("ull_gemm_bf16") <= 1, "lm_head alone may take the tiled GEMM"
        for i, which in enumerate(("w4", "a8")):
            del names[:]
            models[which](input_ids=tok, past_key_values=caches[2 + i], use_cache=True)
            assert names.count(GEMM) == 0 and names.count(NORMQ) == 0, "without the keyword neither new entry is called"
        assert names.count(SKINNY if B <= 16 else GEMM128) == 4 * LAYERS


def test_steps_at_batch_4_equal_the_weight_only_model(models):
    """The new mode at batch 4 (the fused-append GEMV steps): every step bit-identical to the weight-only model from an identical cache."""
    with torch.no_grad():
        caches, tok = _filled_caches(models, 4, 2)
        for step, (oa, ob) in enumerate(zip(_steps(models["w4"], caches[0], tok, 3), _steps(models["d8"], caches[1], tok, 3))):
            assert torch.equal(oa.logits, ob.logits), f"decode step {step}"
            assert torch.equal(oa.hidden_states[-1], ob.hidden_states[-1]), f"decode step {step}"
        assert caches[0].length == caches[1].length == PROMPT + 3


def test_prefill_of_the_decode_only_mode_equals_the_weight_only_model(models, monkeypatch):
    with torch.no_grad():
        ids = _ids(1, n=40, seed=3)
        want = models["w4"](input_ids=ids, use_cache=True).logits
        names = _spy(monkeypatch)
        got = models["d8"](input_ids=ids, use_cache=True).logits
    assert names.count(GEMM) == 0 and names.count(NORMQ) == 0 and names.count(ROWQ) == 0
    assert torch.equal(got, want), "a 40-token prefill stays W4A16, bit for bit"


def _emulation(xq, xsc, w, residual=None, swiglu=False, out=None, out_f32=False):
    """ops.linear_w4a8_skinny out of existing kernels: dequantize the codes it is handed, then the W4A16 Linear."""
    ops = pkg("ops")
    M, K = xq.shape
    sc = xsc[:, ops._mx_perm(K, xq.device)[1]]                     # the scale bytes back in block order
    xd = (xq.view(torch.float8_e4m3fn).float().view(M, K // 32, 32) * torch.pow(2.0, sc.float() - 127)[..., None]).view(M, K).to(BF)
    return ops.linear(xd, w, residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)


@pytest.mark.parametrize("B", [8, 32])
def test_model_error_against_the_emulation(models, monkeypatch, B):
    """Truth: the weight-only model's logits from the same cache.  The new path's error may be at most 1.5 x the error of the same model with
    ops.linear_w4a8_skinny replaced by the emulation (same math, another accumulation order)."""
    ops = pkg("ops")
    with torch.no_grad():
        caches, tok = _filled_caches(models, B, 3)
        truth = models["w4"](input_ids=tok, past_key_values=caches[0], use_cache=True).logits.float()
        new = models["d8"](input_ids=tok, past_key_values=caches[1], use_cache=True).logits.float()
        monkeypatch.setattr(ops, "linear_w4a8_skinny", _emulation)
        emu = models["d8"](input_ids=tok, past_key_values=caches[2], use_cache=True).logits.float()
    e_new, e_emu = (new - truth).abs(), (emu - truth).abs()
    print(f"batch {B}: logit error vs W4A16: new max {float(e_new.max()):.5f} mean {float(e_new.mean()):.6f}; "
          f"emulation max {float(e_emu.max()):.5f} mean {float(e_emu.mean()):.6f}; max|truth| {float(truth.abs().max()):.3f}")
    assert float(e_emu.max()) > 0, "the emulation is an MXFP8-activation model too: it cannot equal the W4A16 model"
    assert float(e_new.max()) <= 1.5 * float(e_emu.max())
    assert float(e_new.mean()) <= 1.5 * float(e_emu.mean())


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_generate_at_batch_8(models, kv):
    m = models["d8"]
    prompt = _ids(8)
    kw = dict(input_ids=prompt, max_new_tokens=6, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    with torch.no_grad():
        a = m.generate(do_sample=False, **kw)
        assert a.shape == (8, PROMPT + 6) and torch.equal(a[:, :PROMPT], prompt)
        assert torch.equal(a, m.generate(do_sample=False, **kw)), "greedy is deterministic"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, sampler="device", **kw)
        assert s.shape == a.shape and int(s.min()) >= 0 and int(s.max()) < VOCAB


def test_beam_search_at_eight_rows_runs(models, monkeypatch):
    prompt = _ids(2)
    names = _spy(monkeypatch)
    with torch.no_grad():
        b = models["d8"].generate(input_ids=prompt, max_new_tokens=6, use_cache=True, eos_token_id=-1, pad_token_id=0, num_beams=4)
    assert names.count(GEMM) > 0, "2 x 4 beams: the steps are on the new route"
    assert b.shape == (2, PROMPT + 6) and torch.equal(b[:, :PROMPT], prompt) and int(b.min()) >= 0 and int(b.max()) < VOCAB
