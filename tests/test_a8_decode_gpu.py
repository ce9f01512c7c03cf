"""GPU: FP8 activations in batched decode steps (ops.linear_a8w8_skinny / ull_gemm_skinny_a8w8_bf16, ops.rmsnorm_quantize_rows_fp8 /
ull_rmsnorm_quantize_rows_fp8_bf16, quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="prefill+decode"), DESIGN f10).

  1. the fused norm + quantize equals the composition of the existing ops, codes and scales, bit for bit;
  2. the GEMM kernel equals the existing W8A8 GEMM and the W8A16 Linear bit for bit on data where every fp32 partial sum is exact
     (tests/test_a8w8_gpu.py `_int_rows`: the summation order cannot matter);
  3. on Gaussian data a row / a column block does not depend on M, N or the other rows (the order is a function of K alone);
  4. on Gaussian data it is within the any-order fp32 accumulation bound of the fp64 restatement (tests/test_a8w8_cpu.py `a8w8_exact`);
  5. model level, on a seeded random-init core whose layer Linears are on the routing rule (N * K >= 2^22).
"""
import pytest
import torch

from helpers import load_fixture, pkg
from test_a8w8_cpu import a8w8_exact
from test_a8w8_gpu import _int_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
MS = (1, 5, 15, 16, 17, 31, 32)


# ---- 1. fused RMSNorm + row quantization ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["gauss", "int"])
@pytest.mark.parametrize("M,K", [(1, 128), (5, 4096), (32, 4096), (7, 11008)])
def test_fused_norm_quantize_equals_the_composition(M, K, data):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(100 * M + K)
    x = torch.randn(M, K, generator=g) * 3.0 if data == "gauss" else torch.randint(-8, 9, (M, K), generator=g).float()
    if data == "gauss":
        x[:, ::501] *= 40.0                                        # activation outliers
    w = 1.0 + 0.1 * torch.randn(K, generator=g)
    w[K // 3] = 56.0                                               # 448 * 2^-3: the largest norm weight
    if M >= 5:
        x[1] = 0                                                   # an all-zero row
        # a row of +-1: mean(x^2) = 1, bf16(x * rsqrt(1 + eps)) = +-1, so the normed row is +-w and its amax exactly 448 * 2^-3
        x[2] = torch.randint(0, 2, (K,), generator=g).float() * 2 - 1
    eps = 1e-6
    xw = torch.zeros(M, K + 72, dtype=BF)
    xw[:, :K] = x.to(BF)
    xw, w = xw.to(DEV), w.to(BF).to(DEV)
    for xs_ in (xw[:, :K].contiguous(), xw[:, :K]):                # contiguous, and rows of a wider buffer (ldx = K + 72)
        normed = ops.rmsnorm(xs_, w, eps)
        want_c, want_s = ops.quantize_rows_fp8(normed)
        got_c, got_s = ops.rmsnorm_quantize_rows_fp8(xs_, w, eps)
        assert got_c.shape == (M, K) and got_c.dtype == torch.uint8 and got_s.shape == (M,) and got_s.dtype == torch.float32
        assert torch.equal(got_s, want_s), "scales"
        assert torch.equal(got_c, want_c), f"codes: {int((got_c != want_c).sum())} of {got_c.numel()} differ"
        if M >= 5:
            assert float(got_s[1]) == 1.0 and not bool(got_c[1].any()), "the all-zero row: scale 2^0, zero codes"
            assert float(normed[2].float().abs().max()) == 56.0 and float(got_s[2]) == 2.0 ** -3, "amax exactly 448 * 2^-3"
        assert bool(got_c.any())


# ---- 2. the GEMM kernel, bit for bit on exactly summable data ----------------------------------------------------------------------------
def _skinny(ops, x, q, **kw):
    return ops.linear_a8w8_skinny(*ops.quantize_rows_fp8(x), q, **kw)


@pytest.mark.parametrize("N,K", [(16, 128), (40, 384), (200, 1024), (48, 11008), (4096, 4096)])
def test_kernel_equals_existing_paths_bit_for_bit(N, K):
    ops = pkg("ops")
    q = ops.quantize_fp8(_int_rows(N, K, 2000 + N))
    assert len(set(q.scales.tolist())) > 1 and bool((q.scales < 1).any())             # s_n varies, some negative
    for M in MS:
        x = _int_rows(M, K, 1000 + M, special=True)
        xq, xs = ops.quantize_rows_fp8(x)
        assert bool((xs < 1).any()) and (M == 1 or len(set(xs.tolist())) > 1)         # t_m varies, some negative
        xd = ops.dequantize(ops.Fp8Weight(xq, xs)).view(x.shape)
        assert torch.equal(xd, x), "the integer rows are exact in e4m3"
        r = _int_rows(M, N, 3000 + M)
        with torch.no_grad():
            for kw, what in ((dict(), "no epilogue"), (dict(residual=r), "residual"), (dict(out_f32=True), "fp32 output")):
                got = ops.linear_a8w8_skinny(xq, xs, q, **kw)
                assert got.shape == (M, N) and got.dtype == (torch.float32 if kw.get("out_f32") else BF)
                assert torch.equal(got, ops.linear_a8w8(x, q, **kw)), f"M = {M}, {what}: against the 128 x 128 W8A8 GEMM"
                assert torch.equal(got, ops.linear(xd, q, **kw)), f"M = {M}, {what}: against the W8A16 Linear on the dequantized rows"
            out = ops.linear_a8w8_skinny(xq, xs, q)
            assert bool(out.float().abs().sum() > 0)
            if M > 5:
                assert float(xs[3]) == 1.0 and not bool(out[3].any()), "the all-zero row gives zeros"


@pytest.mark.parametrize("N,K", [(64, 128), (288, 256), (320, 4096)])
def test_kernel_swiglu_equals_existing_paths_bit_for_bit(N, K):
    ops = pkg("ops")
    # gate / up rows interleaved in groups of 16, scaled so that |gate| stays below 80 (the shared SiLU code returns NaN where exp(-gate)
    # overflows, and NaN != NaN would hide what this test compares): |x| <= 128, |w| <= 2^-7 at K <= 256, 2^-10 at K = 4096
    q = ops.quantize_fp8((_int_rows(N, K, 5000 + N).float() * 2.0 ** (-14 if K <= 256 else -17)).to(BF))
    for M in MS:
        x = _int_rows(M, K, 4000 + M, special=True)
        with torch.no_grad():
            a = _skinny(ops, x, q, swiglu=True)
            assert bool(torch.isfinite(a.float()).all()) and float(ops.linear(x, q).float().abs().max()) < 80.0
            assert a.shape == (M, N // 2) and torch.equal(a, ops.linear_a8w8(x, q, swiglu=True)), f"M = {M}: against the W8A8 GEMM"
            assert torch.equal(a, ops.linear(x, q, swiglu=True)), f"M = {M}: against the W8A16 Linear"
            assert bool(a.float().abs().sum() > 0)


@pytest.mark.parametrize("M", [5, 16, 17, 32])
def test_kernel_strided_codes_and_output(M):
    ops = pkg("ops")
    N, K = 200, 384
    x = _int_rows(M, K, 6000 + M)
    q = ops.quantize_fp8(_int_rows(N, K, 6001))
    xq, xs = ops.quantize_rows_fp8(x)
    wide = torch.full((M, K + 64), 0x7e, device=DEV, dtype=torch.uint8)            # (0x7e = 448: garbage the kernel must not read into the sum)
    wide[:, :K] = xq
    want = ops.linear(x, q)
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_a8w8_skinny(wide[:, :K], xs, q, out=outw[:, :N])             # ldxq = K + 64, ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"
    r = _int_rows(M, N + 8, 6002)[:, :N]                                           # a strided residual
    assert torch.equal(ops.linear_a8w8_skinny(wide[:, :K], xs, q, residual=r), ops.linear(x, q, residual=r.contiguous()))


# ---- 3. the summation order is a function of K alone ----------------------------------------------------------------------------------------
def test_result_does_not_depend_on_m_n_or_the_other_rows():
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    K = 4096
    x = torch.randn(32, K, generator=g).to(BF).to(DEV)
    q = ops.quantize_fp8((torch.randn(200, K, generator=g) * 0.02).to(BF).to(DEV))
    xq, xs = ops.quantize_rows_fp8(x)
    full = ops.linear_a8w8_skinny(xq, xs, q, out_f32=True)
    part = ops.linear_a8w8_skinny(xq[3:8], xs[3:8], q, out_f32=True)              # the second fragment's kernel against the first's
    assert torch.equal(full[3:8], part), "rows 3 .. 7 of an M = 32 call against an M = 5 call"
    cols = ops.linear_a8w8_skinny(xq, xs, ops.Fp8Weight(q.codes[16:32], q.scales[16:32]), out_f32=True)
    assert cols.shape == (32, 16) and torch.equal(full[:, 16:32], cols), "column block 16 .. 31 of N = 200 against N = 16"
    assert torch.equal(ops.linear_a8w8_skinny(xq, xs, q)[3:8], ops.linear_a8w8_skinny(xq[3:8], xs[3:8], q))


# ---- 4. Gaussian data against the fp64 restatement -------------------------------------------------------------------------------------------
def test_kernel_random_data_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 32, 520, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02)
    w[::97] *= 8.0
    q = ops.quantize_fp8(w.to(BF).to(DEV))
    out = _skinny(ops, x.to(DEV), q).cpu().double()
    y, absum = a8w8_exact(x, q.codes, q.scales)
    # K * 2^-23 * 2^(t_m + s_n) * sum_k |xq wq|: fp32 accumulation in any order; 2^-8 |y|: the final rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -8 * y.abs()
    err = (out - y).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y| = {float(y.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"
    f32 = _skinny(ops, x.to(DEV), q, out_f32=True).cpu().double()
    e32 = (f32 - y).abs()
    print(f"fp32 output: max err / accumulation bound = {float((e32 / (K * 2.0 ** -23 * absum).clamp_min(1e-300)).max()):.4f}")
    assert bool((e32 <= K * 2.0 ** -23 * absum).all()), "fp32 output: the accumulation bound alone"


# ---- 5. model level -----------------------------------------------------------------------------------------------------------------------
HID, HEADS, INTER, LAYERS, VOCAB = 2048, 16, 2816, 2, 1024      # q|k|v 6144 x 2048, o 2048 x 2048 (= 2^22), gate|up 5632 x 2048, down 2048 x 2816
PROMPT = 12


def _core(activations=None, scope="prefill"):
    """A seeded random-init core (about 70 M weights) quantized to fp8: the same weights for every (activations, scope)."""
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
    model.quantize_weights("fp8_e4m3", activations=activations, activation_scope=scope)
    return model


@pytest.fixture(scope="module")
def models():
    with torch.no_grad():
        m = dict(w8=_core(), a8=_core("fp8_e4m3"), a8d=_core("fp8_e4m3", "prefill+decode"))
    assert m["w8"].activation_scope == m["a8"].activation_scope == "prefill" and m["a8d"].activation_scope == "prefill+decode"
    assert m["a8d"].activation_quantization == "fp8_e4m3"
    ops = pkg("ops")
    for w in m["a8d"]._packed["llama"]:
        for k in ("w_qkv", "w_o", "w_gu", "w_down"):
            assert all(ops.linear_route(B, w[k], ops.ActQuant("fp8_e4m3", decode=True)) == "a8w8_skinny" for B in (8, 32)), "the layer Linears are on the rule"
    return m


def _ids(B, n=PROMPT, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randint(3, 80, (B, n), generator=g).to(DEV)       # (below the fixture's multimodal token ids, 90 .. 95)


def _filled_caches(models, B, n):
    """n identical KV caches, each filled by the W8A16 model's prefill of the same prompts, and the next token of every row."""
    pf = [models["w8"](input_ids=_ids(B), use_cache=True) for _ in range(n)]
    assert all(torch.equal(pf[0].logits, p.logits) for p in pf[1:])
    return [p.past_key_values for p in pf], pf[0].logits[:, -1].argmax(-1, keepdim=True)


def _spy(monkeypatch):
    L = pkg("_lib")
    names, real = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *a: names.append(name) or real(name, *a))
    return names


GEMM, NORMQ = "ull_gemm_skinny_a8w8_bf16", "ull_rmsnorm_quantize_rows_fp8_bf16"
SKINNY, GEMM128 = "ull_gemm_skinny_wq_bf16", "ull_gemm_a8w8_bf16"


@pytest.mark.parametrize("B", [8, 32])
def test_decode_step_takes_the_new_entries_only_under_the_new_scope(models, monkeypatch, B):
    with torch.no_grad():
        caches, tok = _filled_caches(models, B, 2)
        names = _spy(monkeypatch)
        models["a8d"](input_ids=tok, past_key_values=caches[0], use_cache=True)
        assert names.count(GEMM) == 4 * LAYERS and names.count(NORMQ) == 2 * LAYERS
        assert names.count("ull_quantize_rows_fp8_bf16") == 2 * LAYERS, "o_proj and down_proj quantize their inputs in a launch of their own"
        assert names.count(SKINNY) == 0 and names.count(GEMM128) == 0 and names.count("ull_rmsnorm_bf16") == 1, "(the final norm)"
        assert names.count("ull_gemm_bf16") <= 1, "lm_head alone may take the tiled GEMM"
        del names[:]
        models["a8"](input_ids=tok, past_key_values=caches[1], use_cache=True)
        assert names.count(GEMM) == 0 and names.count(NORMQ) == 0, "the default scope calls neither new entry"
        assert names.count(SKINNY if B <= 16 else GEMM128) == 4 * LAYERS


def _steps(model, cache, tok, n):
    outs = []
    for _ in range(n):
        o = model(input_ids=tok, past_key_values=cache, use_cache=True, output_hidden_states=True)
        outs.append(o)
        tok = o.logits[:, -1].argmax(-1, keepdim=True)
    return outs


@pytest.mark.parametrize("which,B", [("a8", 8), ("a8d", 4)])
def test_steps_outside_the_new_path_equal_the_w8a16_model(models, which, B):
    """Default scope at a skinny batch (8), and the new scope at batch 4 (the fused-append GEMV steps): every step bit-identical to the
    weight-only model from an identical cache."""
    with torch.no_grad():
        caches, tok = _filled_caches(models, B, 2)
        for step, (oa, ob) in enumerate(zip(_steps(models["w8"], caches[0], tok, 3), _steps(models[which], caches[1], tok, 3))):
            assert torch.equal(oa.logits, ob.logits), f"decode step {step}"
            assert torch.equal(oa.hidden_states[-1], ob.hidden_states[-1]), f"decode step {step}"
        assert caches[0].length == caches[1].length == PROMPT + 3


def _emulation(xq, xs, w, residual=None, swiglu=False, out=None, out_f32=False):
    """ops.linear_a8w8_skinny out of existing kernels: dequantize the codes it is handed, then the W8A16 Linear."""
    ops = pkg("ops")
    return ops.linear(ops.dequantize(ops.Fp8Weight(xq, xs)), w, residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)


@pytest.mark.parametrize("B", [8, 32])
def test_model_error_against_the_emulation(models, monkeypatch, B):
    """Truth: the W8A16 model's logits from the same cache.  The new path's error may be at most 1.5 x the error of the same model with
    ops.linear_a8w8_skinny replaced by the emulation (same math, another accumulation order)."""
    ops = pkg("ops")
    with torch.no_grad():
        caches, tok = _filled_caches(models, B, 3)
        truth = models["w8"](input_ids=tok, past_key_values=caches[0], use_cache=True).logits.float()
        new = models["a8d"](input_ids=tok, past_key_values=caches[1], use_cache=True).logits.float()
        monkeypatch.setattr(ops, "linear_a8w8_skinny", _emulation)
        emu = models["a8d"](input_ids=tok, past_key_values=caches[2], use_cache=True).logits.float()
    e_new, e_emu = (new - truth).abs(), (emu - truth).abs()
    print(f"batch {B}: logit error vs W8A16: new max {float(e_new.max()):.5f} mean {float(e_new.mean()):.6f}; "
          f"emulation max {float(e_emu.max()):.5f} mean {float(e_emu.mean()):.6f}; max|truth| {float(truth.abs().max()):.3f}")
    assert float(e_emu.max()) > 0, "the emulation is an fp8-activation model too: it cannot equal the W8A16 model"
    assert float(e_new.max()) <= 1.5 * float(e_emu.max())
    assert float(e_new.mean()) <= 1.5 * float(e_emu.mean())


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_generate_at_batch_8(models, kv):
    m = models["a8d"]
    prompt = _ids(8)
    kw = dict(input_ids=prompt, max_new_tokens=6, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    with torch.no_grad():
        a = m.generate(do_sample=False, **kw)
        assert a.shape == (8, PROMPT + 6) and torch.equal(a[:, :PROMPT], prompt)
        assert torch.equal(a, m.generate(do_sample=False, **kw)), "greedy is deterministic"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, sampler="device", **kw)
        assert s.shape == a.shape and int(s.min()) >= 0 and int(s.max()) < VOCAB
