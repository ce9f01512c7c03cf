"""GPU: FP8 activations on FP8 weights (ops.linear_a8w8 / ull_gemm_a8w8_bf16, quantize_weights("fp8_e4m3", activations="fp8_e4m3")).

The kernel is pinned to the definition in tests/test_a8w8_cpu.py three ways:
  * bit for bit against the existing path on data where every fp32 partial sum is exact (integers of magnitude <= 8 times one power of
    two per row: exact in e4m3 under any power-of-two scale, every product under one (m, n) shares one power-of-two factor, and
    64 * K < 2^24 for K <= 11008 -- so the summation order cannot matter, in the new kernel or in the bf16 GEMM);
  * against the fp64 restatement on Gaussian data, within the fp32 accumulation bound for ANY summation order plus one bf16 ulp;
  * at model level against the emulation built from existing kernels (quantize rows -> dequantize -> W8A16 Linear).
"""
import pytest
import torch

from helpers import core_model_from_fixture, load_fixture, pkg
from test_a8w8_cpu import a8w8_exact
from test_fp8_weights_cpu import fp8_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16


def _dequant_rows(ops, x):
    """dequant(quantize_rows(x)) with the existing kernels: the bf16 activations the W8A8 Linear really multiplies."""
    codes, scales = ops.quantize_rows_fp8(x)
    return ops.dequantize(ops.Fp8Weight(codes, scales)).view(x.shape)


def emulation(x, w, residual=None, swiglu=False, out=None, out_f32=False):
    """ops.linear_a8w8 out of existing kernels: the W8A16 Linear (dequantize + bf16 GEMM) on the quantize-dequantized activations."""
    ops = pkg("ops")
    return ops.linear(_dequant_rows(ops, x), w, residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)


# ---- 1. the kernel, bit for bit -------------------------------------------------------------------------------------------------------
def _int_rows(rows, K, seed, special=False):
    """bf16 [rows, K]: integers in [-8, 8] times 2^e_row, e_row in [-4, 4]; special: row 3 all zero, row 5 with amax exactly 448 * 2^-3
    (integers in [-7, 7] times 64 * 2^-3, one of them 7)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, (rows, K), generator=g).float()
    e = (torch.arange(rows) * 7 % 9 - 4).float()
    v = v * torch.pow(2.0, e)[:, None]
    if special and rows > 5:
        v[3] = 0
        v[5] = torch.randint(-7, 8, (K,), generator=g).float() * 8.0
        v[5, K // 2] = 56.0                      # 448 * 2^-3
    return v.to(BF).to(DEV)


# (M, N, K): the kernel's tile is 128 x 128 with a K-tile of 128 codes; "gemm" starts at M = 17 against LLaMA-sized weights
INT_SHAPES = [(127, 127, 128), (128, 128, 256), (129, 129, 384), (17, 200, 128), (40, 136, 192), (33, 48, 64), (40, 144, 11008),
              (300, 264, 512)]


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_kernel_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x = _int_rows(M, K, 1000 + M, special=True)
    q = ops.quantize_fp8(_int_rows(N, K, 2000 + N))
    assert len(set(q.scales.tolist())) > 1 and bool((q.scales < 1).any())             # s_n varies, some negative
    xs = ops.quantize_rows_fp8(x)[1]
    assert len(set(xs.tolist())) > 1 and bool((xs < 1).any()) and float(xs[3]) == 1.0 and float(xs[5]) == 2.0 ** -3
    xd = _dequant_rows(ops, x)
    assert torch.equal(xd, x), "the integer rows are exact in e4m3"
    r = _int_rows(M, N, 3000 + M)
    with torch.no_grad():
        assert torch.equal(ops.linear_a8w8(x, q), ops.linear(xd, q)), "no epilogue"
        assert torch.equal(ops.linear_a8w8(x, q, residual=r), ops.linear(xd, q, residual=r)), "residual"
        assert torch.equal(ops.linear_a8w8(x, q, out_f32=True), ops.linear(xd, q, out_f32=True)), "fp32 output"
        out = ops.linear_a8w8(x, q)
        assert bool(out.float().abs().sum() > 0) and not bool(out[3].any()), "the all-zero row gives zeros"


@pytest.mark.parametrize("M,N,K", [(129, 320, 256), (17, 64, 128), (200, 2 * 144, 192)])
def test_kernel_swiglu_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x = _int_rows(M, K, 4000 + M, special=True)
    # gate / up rows interleaved in groups of 16, scaled so that |gate| stays far below 88 (the shared SiLU code returns NaN where
    # exp(-gate) overflows, and NaN != NaN would hide what this test compares): |x| <= 128, |w| <= 2^-7, K <= 256 random-sign terms
    q = ops.quantize_fp8((_int_rows(N, K, 5000 + N).float() * 2.0 ** -14).to(BF))
    with torch.no_grad():
        a, b = ops.linear_a8w8(x, q, swiglu=True), ops.linear(x, q, swiglu=True)
    assert bool(torch.isfinite(b.float()).all()) and float(ops.linear(x, q).float().abs().max()) < 80.0
    assert a.shape == (M, N // 2) and torch.equal(a, b)
    assert bool(a.float().abs().sum() > 0)


def test_kernel_strided_input_and_output():
    ops = pkg("ops")
    M, N, K = 70, 200, 256
    xw = _int_rows(M, K + 64, 6000)
    x = xw[:, :K]                                                  # ldx = K + 64
    q = ops.quantize_fp8(_int_rows(N, K, 6001))
    want = ops.linear(x.contiguous(), q)
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_a8w8(x, q, out=outw[:, :N])                   # ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"
    # 3-D activations [B, S, K] and a 3-D residual
    x3 = x.contiguous().view(2, 35, K)
    r3 = _int_rows(M, N, 6002).view(2, 35, N)
    assert torch.equal(ops.linear_a8w8(x3, q, residual=r3), ops.linear(x3, q, residual=r3))


def test_result_does_not_depend_on_the_rows_sharing_a_tile():
    """Gaussian data: row m of a [300, K] product equals the same row computed alone among other rows, at another M, bit for bit."""
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 1024, generator=g).to(BF).to(DEV)
    q = ops.quantize_fp8((torch.randn(264, 1024, generator=g) * 0.02).to(BF).to(DEV))
    full = ops.linear_a8w8(x, q)
    part = ops.linear_a8w8(x[131:160].contiguous(), q)             # 29 rows, another place in the tile, another grid
    assert torch.equal(full[131:160], part)


# ---- 2. the kernel on random data against the fp64 restatement -------------------------------------------------------------------------
def test_kernel_random_data_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 300, 520, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02)
    w[::97] *= 8.0
    q = ops.quantize_fp8(w.to(BF).to(DEV))
    out = ops.linear_a8w8(x.to(DEV), q).cpu().double()
    y, absum = a8w8_exact(x, q.codes, q.scales)
    # K * 2^-23 * 2^(t_m + s_n) * sum_k |xq wq|: fp32 accumulation in any order (truncation inside the instruction allowed);
    # 2^-8 |y|: the final rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -8 * y.abs()
    err = (out - y).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y| = {float(y.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"
    f32 = ops.linear_a8w8(x.to(DEV), q, out_f32=True).cpu().double()
    assert bool(((f32 - y).abs() <= K * 2.0 ** -23 * absum).all()), "fp32 output: the accumulation bound alone"


# ---- 3. activation quantization ------------------------------------------------------------------------------------------------------
def test_quantize_rows_on_activations_equals_torch_cast():
    ops = pkg("ops")
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(17, 4096, generator=g) * 3.0)
    x[:, ::501] *= 40.0                                            # activation outliers
    x[4] = 0
    x = x.to(BF)
    codes, scales = ops.quantize_rows_fp8(x.to(DEV))
    rc, rs = fp8_reference(x)
    assert torch.equal(codes.cpu(), rc) and torch.equal(scales.cpu(), rs)
    # rows of a wider buffer, viewed [B, S, K]
    wide = torch.zeros(17, 4096 + 128, dtype=BF)
    wide[:, :4096] = x
    c2, s2 = ops.quantize_rows_fp8(wide.to(DEV)[:, :4096])
    assert torch.equal(c2.cpu(), rc) and torch.equal(s2.cpu(), rs)


# ---- 4. tiny models --------------------------------------------------------------------------------------------------------------------
def _tiny(activations=None):
    fx = load_fixture("g1_core_tiny_bf16.pt")
    model, _ = core_model_from_fixture(fx, DEV)
    model.quantize_weights("fp8_e4m3", activations=activations)
    return fx, model


def _inputs(fx):
    return dict(input_ids=fx["input_ids"].to(DEV), attention_mask=fx["attention_mask"].to(DEV), images=fx["images"].to(DEV))


def test_mode_switch_and_attribute():
    fx, m = _tiny()
    assert m.weight_quantization == "fp8_e4m3" and m.activation_quantization is None
    codes = m._packed["llama"][0]["w_o"].codes
    assert m.quantize_weights("fp8_e4m3", activations="fp8_e4m3") is m             # switching the mode on: no weight changes
    assert m.activation_quantization == "fp8_e4m3" and m._packed["llama"][0]["w_o"].codes is codes
    assert m.quantize_weights("fp8_e4m3") is m and m.activation_quantization == "fp8_e4m3"
    with pytest.raises(NotImplementedError):
        m.quantize_weights("mxfp4", activations="fp8_e4m3")


def test_model_takes_the_new_entry_only_at_gemm_shapes(monkeypatch):
    ops = pkg("ops")
    fx, m = _tiny("fp8_e4m3")
    calls = []
    real = ops.linear_a8w8
    monkeypatch.setattr(ops, "linear_a8w8", lambda x, w, **kw: calls.append((x.shape[0], tuple(w.shape))) or real(x, w, **kw))
    L = len(m.model.layers)
    with torch.no_grad():
        m(**_inputs(fx))
        assert len(calls) == 4 * L and {c[0] for c in calls} == {26}, "q|k|v, o_proj, gate|up, down_proj of every layer at T = 26"
        del calls[:]
        out = m(input_ids=fx["greedy_prompt"].to(DEV), images=fx["images"][:1].to(DEV), use_cache=True)
        assert len(calls) == 4 * L
        del calls[:]
        m(input_ids=torch.tensor([[5]], device=DEV), past_key_values=out.past_key_values, use_cache=True)
        assert calls == [], "a decode step stays W8A16"


def test_batch_invariance():
    """Sample b of a batch equals the single-sample run bit for bit (both at prefill shapes)."""
    fx, m = _tiny("fp8_e4m3")
    inp = _inputs(fx)
    with torch.no_grad():
        both = m(**inp, output_hidden_states=True)
        for b in range(2):
            one = m(**{k: v[b:b + 1] for k, v in inp.items()}, output_hidden_states=True)
            assert torch.equal(both.logits[b:b + 1], one.logits), f"logits of sample {b}"
            for i, (hb, h1) in enumerate(zip(both.hidden_states, one.hidden_states)):
                assert torch.equal(hb[b:b + 1], h1), f"hidden state {i} of sample {b}"


def test_model_error_against_the_emulation(monkeypatch):
    """The same model with ops.linear_a8w8 replaced by the emulation out of existing kernels: the new path's logit error against the
    fixture's reference logits may be at most 1.5 x the emulation's (same math, another rounding order)."""
    ops = pkg("ops")
    fx, m = _tiny("fp8_e4m3")
    ref = fx["logits"].float()
    with torch.no_grad():
        new = m(**_inputs(fx)).logits.float().cpu()
        monkeypatch.setattr(ops, "linear_a8w8", emulation)
        emu = m(**_inputs(fx)).logits.float().cpu()
    valid = fx["attention_mask"].bool()
    e_new, e_emu = (new - ref)[valid].abs(), (emu - ref)[valid].abs()
    print(f"logit error vs reference: new max {float(e_new.max()):.5f} mean {float(e_new.mean()):.6f}; "
          f"emulation max {float(e_emu.max()):.5f} mean {float(e_emu.mean()):.6f}; max|ref| {float(ref.abs().max()):.3f}")
    assert float(e_emu.max()) > 0, "the emulation is an fp8-activation model too: it cannot equal the bf16 reference"
    assert float(e_new.max()) <= 1.5 * float(e_emu.max())
    assert float(e_new.mean()) <= 1.5 * float(e_emu.mean())


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_generate_runs_with_every_option(kv):
    fx, m = _tiny("fp8_e4m3")
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    kw = dict(input_ids=prompt, images=images, max_new_tokens=8, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    with torch.no_grad():
        a = m.generate(do_sample=False, **kw)
        assert a.shape == (1, prompt.shape[1] + 8) and torch.equal(a[:, :prompt.shape[1]], prompt)
        assert torch.equal(a, m.generate(do_sample=False, **kw)), "deterministic"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, sampler="device", **kw)
        assert s.shape == a.shape and int(s.min()) >= 0 and int(s.max()) < m.config.vocab_size
        if kv is None:
            nc = m.generate(do_sample=False, **dict(kw, use_cache=False, kv_cache_dtype=None))
            assert nc.shape == a.shape                     # (may differ from `a`: the cached run decodes in W8A16)


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_evaluate_runs(kv):
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    assert model.quantize_weights("fp8_e4m3", activations="fp8_e4m3") is model and model.activation_quantization == "fp8_e4m3"
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    torch.manual_seed(77)
    ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9, kv_cache_dtype=kv, sampler="device")
    assert ids.dim() == 2 and ids.shape[0] == 1 and ids.numel() > 0
    assert all(bool(torch.isfinite(t.float()).all()) for t in list(masks) + list(boxes))


def test_decode_steps_equal_the_w8a16_model_from_the_same_cache():
    """Both models continue from identical KV caches built by the W8A16 prefill: every single-token step is bit-identical."""
    fx, w8 = _tiny()
    _, a8 = _tiny("fp8_e4m3")
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    with torch.no_grad():
        pf = [w8(input_ids=prompt, images=images, use_cache=True) for _ in range(2)]
        assert torch.equal(pf[0].logits, pf[1].logits)
        caches = [p.past_key_values for p in pf]
        tok = pf[0].logits[:, -1].argmax(-1, keepdim=True)
        for step in range(4):
            oa = w8(input_ids=tok, past_key_values=caches[0], use_cache=True, output_hidden_states=True)
            ob = a8(input_ids=tok, past_key_values=caches[1], use_cache=True, output_hidden_states=True)
            assert torch.equal(oa.logits, ob.logits), f"decode step {step}"
            assert torch.equal(oa.hidden_states[-1], ob.hidden_states[-1]), f"decode step {step}"
            tok = oa.logits[:, -1].argmax(-1, keepdim=True)
        assert caches[0].length == caches[1].length == prompt.shape[1] + 4
        # ... while the A8 prefill itself is a different computation
        assert not torch.equal(a8(input_ids=prompt, images=images).logits, pf[0].logits)


def test_without_activations_the_model_still_equals_its_twin():
    """activation_quantization None: today's bits (the twin assertion of tests/test_fp8_weights_gpu.py)."""
    from test_fp8_weights_gpu import _tiny_core_pair
    fx, twin, fp8 = _tiny_core_pair()
    assert fp8.activation_quantization is None
    with torch.no_grad():
        a, b = (m(**_inputs(fx), output_hidden_states=True) for m in (twin, fp8))
        assert torch.equal(a.logits, b.logits)
        for i, (x, y) in enumerate(zip(a.hidden_states, b.hidden_states)):
            assert torch.equal(x, y), f"hidden state {i}"
