"""GPU: MXFP8 activations on MXFP4 weights (ops.linear_w4a8 / ull_gemm_w4a8_bf16, quantize_weights("mxfp4", activations="mxfp8_e4m3")).

The kernels are pinned to the definition in tests/test_w4a8_cpu.py:
  * the activation quantizer bit for bit against the torch restatement;
  * the operand layout (nibble order, resident permutation, scale bytes) with one-hot activations: the product IS dequant(w).T;
  * bit for bit against the existing path (dequantize + bf16 GEMM) on data where every fp32 partial sum is exact in any order:
    activations = integers |v| <= 8 times 2^e_row times a per-block 2^{0,1,2}, weights = e2m1 values (multiples of 0.5 up to 6, a 6 in every
    block) times 2^e_row times a per-block 2^{0,1}: with the row factors taken out a term is at most 32 * 12 = 768 half-units and
    768 * 11008 < 2^24;
  * against the fp64 restatement on Gaussian data within the any-order fp32 accumulation bound plus one bf16 rounding;
  * at model level against the emulation built from existing kernels.
"""
import pytest
import torch

from helpers import core_model_from_fixture, load_fixture, pkg
from test_w4a8_cpu import mxfp8_reference, special_rows, w4a8_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


# ---- 1. the activation quantizer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("K", [32, 96, 4096])
def test_quantize_rows_mxfp8_equals_restatement(M, K):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(M * 10000 + K)
    x = torch.randn(M, K, generator=g) * 3.0
    x[:, ::37] *= 40.0                                            # outliers
    x *= torch.pow(2.0, torch.randint(-12, 13, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
    x[M // 2, :32] = 0
    x = x.to(BF)
    codes, scales = ops.quantize_rows_mxfp8(x.to(DEV))
    rc, rs = mxfp8_reference(x)
    assert codes.shape == (M, K) and scales.shape == (M, K // 32)
    assert torch.equal(codes.cpu(), rc) and torch.equal(scales.cpu(), rs)


def test_quantize_rows_mxfp8_special_blocks_and_strided_rows():
    ops = pkg("ops")
    x = special_rows()
    rc, rs = mxfp8_reference(x)
    codes, scales = ops.quantize_rows_mxfp8(x.to(DEV))
    assert torch.equal(codes.cpu(), rc) and torch.equal(scales.cpu(), rs)
    wide = torch.full((8, 96 + 40), 9.0, dtype=BF)
    wide[:, :96] = x
    c2, s2 = ops.quantize_rows_mxfp8(wide.to(DEV)[:, :96])        # ldx = 136
    assert torch.equal(c2.cpu(), rc) and torch.equal(s2.cpu(), rs)
    c3, s3 = ops.quantize_rows_mxfp8(x.to(DEV).view(2, 4, 96))    # [B, S, K]
    assert torch.equal(c3.cpu(), rc) and torch.equal(s3.cpu(), rs)


# ---- 2. layout ------------------------------------------------------------------------------------------------------------------------
def _varied_weight(N, K, seed):
    """bf16 [N, K] of exact MXFP4 values: every e2m1 magnitude and both signs, a 6 in every block, block scales 2^[-6, 6] all different
    between neighbours."""
    g = torch.Generator().manual_seed(seed)
    v = E2M1[torch.randint(0, 8, (N, K), generator=g)] * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1).float()
    v.view(N, K // 32, 32)[:, :, 0] = 6.0
    v.view(N, K // 32, 32)[:, :, 0] *= (torch.arange(K // 32) % 2 * 2 - 1).float()
    e = ((torch.arange(N)[:, None] * 5 + torch.arange(K // 32)[None, :] * 3) % 13 - 6).float()
    return (v * torch.pow(2.0, e).repeat_interleave(32, 1)).to(BF)


@pytest.mark.parametrize("K", [128, 2048 + 384])
def test_one_hot_activations_give_the_dequantized_weight(K):
    """x = the identity: y[m, n] = dequant(w)[n, m] exactly -- pins the nibble order, the resident permutation (one superblock plus three
    tail tiles at K = 2432) and the scale byte of every k."""
    ops = pkg("ops")
    N = 48
    w = _varied_weight(N, K, 70 + K).to(DEV)
    q = ops.quantize_mxfp4(w)
    wd = ops.dequantize(q)
    assert torch.equal(wd, w), "the weight is exact in MXFP4"
    x = torch.eye(K, device=DEV, dtype=BF)
    got = ops.linear_w4a8(x, q, out_f32=True)
    assert got.dtype == torch.float32 and torch.equal(got, wd.float().T)
    # asymmetric activations too: row m = 2^(m % 5) at k = m
    x2 = (torch.eye(K) * torch.pow(2.0, (torch.arange(K) % 5).float())[:, None]).to(BF).to(DEV)
    assert torch.equal(ops.linear_w4a8(x2, q, out_f32=True), wd.float().T * torch.pow(2.0, (torch.arange(K, device=DEV) % 5).float())[:, None])


# ---- 3. bit for bit against the existing path -------------------------------------------------------------------------------------------
def _act(rows, K, seed, special=False):
    """bf16 [rows, K]: integers in [-8, 8] with an 8 in every block, times 2^e_row (e_row in [-4, 4]) times a per-block 2^{0,1,2}."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, (rows, K), generator=g).float()
    v.view(rows, K // 32, 32)[:, :, 1] = 8.0
    v *= torch.pow(2.0, torch.randint(0, 3, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
    v *= torch.pow(2.0, (torch.arange(rows) * 7 % 9 - 4).float())[:, None]
    if special and rows > 5:
        v[3] = 0
    return v.to(BF).to(DEV)


def _wgt(rows, K, seed, mag=0):
    """bf16 [rows, K]: e2m1 values with a 6 in every block, times 2^e_row (e_row in [-3, 3] + mag) times a per-block 2^{0,1}."""
    g = torch.Generator().manual_seed(seed)
    v = E2M1[torch.randint(0, 8, (rows, K), generator=g)] * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float()
    v.view(rows, K // 32, 32)[:, :, 2] = -6.0
    v *= torch.pow(2.0, torch.randint(0, 2, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
    v *= torch.pow(2.0, (torch.arange(rows) * 5 % 7 - 3 + mag).float())[:, None]
    return v.to(BF).to(DEV)


def _dequant_rows(ops, x):
    """dequant(quantize_rows_mxfp8(x)) as bf16: the activations the W4A8 Linear really multiplies (4 significant bits: exact in bf16)."""
    codes, scales = ops.quantize_rows_mxfp8(x)
    v = codes.view(torch.float8_e4m3fn).float().view(codes.shape[0], -1, 32) * torch.pow(2.0, scales.float() - 127)[..., None]
    return v.view(codes.shape).to(BF).view(x.shape)


def emulation(x, w, residual=None, swiglu=False, out=None, out_f32=False):
    """ops.linear_w4a8 out of existing kernels: the W4A16 Linear (dequantize + bf16 GEMM) on the quantize-dequantized activations."""
    ops = pkg("ops")
    return ops.linear(_dequant_rows(ops, x), w, residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)


# (M, N, K): 128 x 128 tile, K-tile of 128 codes, superblocks of 2048: none / exactly one / one + a tail tile / two / five + six tail tiles
INT_SHAPES = [(127, 127, 128), (128, 128, 256), (129, 129, 384), (17, 200, 128), (33, 48, 64), (40, 136, 2048), (40, 144, 2176), (40, 144, 4096),
              (40, 144, 11008), (300, 264, 512)]


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_kernel_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x = _act(M, K, 1000 + M, special=True)
    w = _wgt(N, K, 2000 + N)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize(q), w), "the weights are exact in MXFP4"
    xd = _dequant_rows(ops, x)
    assert torch.equal(xd, x), "the activations are exact in MXFP8"
    sc = ops.quantize_rows_mxfp8(x)[1]
    assert len(set(sc.flatten().tolist())) > 2, "block scales vary"
    r = _act(M, N - N % 32 + 32, 3000 + M)[:, :N].contiguous()
    with torch.no_grad():
        assert torch.equal(ops.linear_w4a8(x, q), ops.linear(xd, q)), "no epilogue"
        assert torch.equal(ops.linear_w4a8(x, q, residual=r), ops.linear(xd, q, residual=r)), "residual"
        assert torch.equal(ops.linear_w4a8(x, q, out_f32=True), ops.linear(xd, q, out_f32=True)), "fp32 output"
        out = ops.linear_w4a8(x, q)
        assert bool(out.float().abs().sum() > 0) and not bool(out[3].any()), "the all-zero row gives zeros"


@pytest.mark.parametrize("K", [4096, 2048 + 128])
def test_kernel_full_grid_equals_existing_path_bit_for_bit(K):
    """The superblock loop with two blocks on every CU (16 x 32 tiles of 128 x 128), at a K that is whole superblocks only (no tail tile
    follows the last super tile: the staging schedule's last steps differ) and at one with a tail: memory latency under a full grid is
    what a counted wait has to survive."""
    ops = pkg("ops")
    M, N = 2048, 4096
    x = _act(M, K, 7000 + K)
    w = _wgt(N, K, 7001 + K)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize(q), w) and torch.equal(_dequant_rows(ops, x), x)
    with torch.no_grad():
        want = ops.linear(x, q, out_f32=True)
        for _ in range(3):
            assert torch.equal(ops.linear_w4a8(x, q, out_f32=True), want)


@pytest.mark.parametrize("M,N,K", [(129, 320, 256), (17, 64, 128), (40, 2 * 144, 2176)])
def test_kernel_swiglu_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x = _act(M, K, 4000 + M, special=True)
    # |gate| far below 88 (the shared SiLU code returns NaN where exp(-gate) overflows): |x| <= 2^9, |w| <= 12 * 2^(3 - 22), K <= 2176
    # random-sign terms
    q = ops.quantize_mxfp4(_wgt(N, K, 5000 + N, mag=-22))
    assert torch.equal(_dequant_rows(ops, x), x), "the activations are exact in MXFP8: ops.linear on x is the existing path"
    with torch.no_grad():
        a, b = ops.linear_w4a8(x, q, swiglu=True), ops.linear(x, q, swiglu=True)
        assert bool(torch.isfinite(b.float()).all()) and float(ops.linear(x, q).float().abs().max()) < 80.0
    assert a.shape == (M, N // 2) and torch.equal(a, b)
    assert bool(a.float().abs().sum() > 0)


def test_kernel_strided_input_and_output():
    ops = pkg("ops")
    M, N, K = 70, 200, 256
    xw = _act(M, K + 64, 6000)
    x = xw[:, :K]                                                  # ldx = K + 64
    q = ops.quantize_mxfp4(_wgt(N, K, 6001))
    want = ops.linear(x.contiguous(), q)
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_w4a8(x, q, out=outw[:, :N])                   # ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"
    x3 = x.contiguous().view(2, 35, K)                             # 3-D activations [B, S, K] and a 3-D residual
    r3 = _act(M, 224, 6002)[:, :N].contiguous().view(2, 35, N)
    assert torch.equal(ops.linear_w4a8(x3, q, residual=r3), ops.linear(x3, q, residual=r3))


# ---- 4. tile independence, 5. Gaussian accuracy -------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_rows_sharing_a_tile():
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 4096, generator=g).to(BF).to(DEV)
    q = ops.quantize_mxfp4((torch.randn(264, 4096, generator=g) * 0.02).to(BF).to(DEV))
    full = ops.linear_w4a8(x, q)
    assert torch.equal(full[131:132], ops.linear_w4a8(x[131:132].contiguous(), q)), "a row computed alone"
    assert torch.equal(full[131:160], ops.linear_w4a8(x[131:160].contiguous(), q)), "29 rows, another place in the tile, another grid"


def test_kernel_random_data_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 300, 520, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02)
    w[::97] *= 8.0
    q = ops.quantize_mxfp4(w.to(BF).to(DEV))
    wc, ws = (t.cpu() for t in q.to_standard())
    out = ops.linear_w4a8(x.to(DEV), q).cpu().double()
    y, absum = w4a8_exact(x, wc, ws)
    # K * 2^-23 * sum |terms|: fp32 accumulation in any order (truncation inside the instruction allowed); 2^-8 |y|: the rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -8 * y.abs()
    err = (out - y).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y| = {float(y.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"
    f32 = ops.linear_w4a8(x.to(DEV), q, out_f32=True).cpu().double()
    assert bool(((f32 - y).abs() <= K * 2.0 ** -23 * absum).all()), "fp32 output: the accumulation bound alone"


# ---- 6. tiny models (K < 2048: the standard-order phase only; the kernel tests above cover superblocks) --------------------------------------
def _tiny(activations=None):
    fx = load_fixture("g1_core_tiny_bf16.pt")
    model, _ = core_model_from_fixture(fx, DEV)
    model.quantize_weights("mxfp4", activations=activations)
    return fx, model


def _inputs(fx):
    return dict(input_ids=fx["input_ids"].to(DEV), attention_mask=fx["attention_mask"].to(DEV), images=fx["images"].to(DEV))


def test_mode_switch_and_attribute():
    fx, m = _tiny()
    assert m.weight_quantization == "mxfp4" and m.activation_quantization is None
    codes = m._packed["llama"][0]["w_o"].codes
    assert m.quantize_weights("mxfp4", activations="mxfp8_e4m3") is m             # switching the mode on: no weight changes
    assert m.activation_quantization == "mxfp8_e4m3" and m._packed["llama"][0]["w_o"].codes is codes
    assert m.quantize_weights("mxfp4") is m and m.activation_quantization == "mxfp8_e4m3"
    with pytest.raises(NotImplementedError):
        m.quantize_weights("mxfp4", activations="fp8_e4m3")
    _, fresh = _tiny("mxfp8_e4m3")
    assert fresh.weight_quantization == "mxfp4" and fresh.activation_quantization == "mxfp8_e4m3"


def test_model_takes_the_new_entry_only_at_gemm_shapes(monkeypatch):
    ops, L_ = pkg("ops"), pkg("_lib")
    fx, m = _tiny("mxfp8_e4m3")
    calls, entries = [], []
    real, real_call = ops.linear_w4a8, L_.call
    monkeypatch.setattr(ops, "linear_w4a8", lambda x, w, **kw: calls.append((x.shape[0], tuple(w.shape))) or real(x, w, **kw))
    monkeypatch.setattr(L_, "call", lambda name, *a: (entries.append(name) if name == "ull_gemm_w4a8_bf16" else None) or real_call(name, *a))
    L = len(m.model.layers)
    with torch.no_grad():
        m(**_inputs(fx))
        assert len(calls) == 4 * L and len(entries) == 4 * L and {c[0] for c in calls} == {26}, "q|k|v, o_proj, gate|up, down_proj of every layer"
        del calls[:], entries[:]
        out = m(input_ids=fx["greedy_prompt"].to(DEV), images=fx["images"][:1].to(DEV), use_cache=True)
        assert len(calls) == 4 * L and len(entries) == 4 * L
        del calls[:], entries[:]
        m(input_ids=torch.tensor([[5]], device=DEV), past_key_values=out.past_key_values, use_cache=True)
        assert calls == [] and entries == [], "a decode step stays W4A16"


def test_batch_invariance():
    fx, m = _tiny("mxfp8_e4m3")
    inp = _inputs(fx)
    with torch.no_grad():
        both = m(**inp, output_hidden_states=True)
        for b in range(2):
            one = m(**{k: v[b:b + 1] for k, v in inp.items()}, output_hidden_states=True)
            assert torch.equal(both.logits[b:b + 1], one.logits), f"logits of sample {b}"
            for i, (hb, h1) in enumerate(zip(both.hidden_states, one.hidden_states)):
                assert torch.equal(hb[b:b + 1], h1), f"hidden state {i} of sample {b}"


def test_model_error_against_the_emulation(monkeypatch):
    """The new path's logit error against the fixture's reference logits may be at most 1.5 x that of the same model with ops.linear_w4a8
    replaced by the emulation out of existing kernels (same math, another rounding order): the rule of tests/test_a8w8_gpu.py."""
    ops = pkg("ops")
    fx, m = _tiny("mxfp8_e4m3")
    ref = fx["logits"].float()
    with torch.no_grad():
        new = m(**_inputs(fx)).logits.float().cpu()
        monkeypatch.setattr(ops, "linear_w4a8", emulation)
        emu = m(**_inputs(fx)).logits.float().cpu()
    valid = fx["attention_mask"].bool()
    e_new, e_emu = (new - ref)[valid].abs(), (emu - ref)[valid].abs()
    print(f"logit error vs reference: new max {float(e_new.max()):.5f} mean {float(e_new.mean()):.6f}; "
          f"emulation max {float(e_emu.max()):.5f} mean {float(e_emu.mean()):.6f}; max|ref| {float(ref.abs().max()):.3f}")
    assert float(e_emu.max()) > 0
    assert float(e_new.max()) <= 1.5 * float(e_emu.max())
    assert float(e_new.mean()) <= 1.5 * float(e_emu.mean())


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_generate_runs_with_every_option(kv):
    fx, m = _tiny("mxfp8_e4m3")
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    kw = dict(input_ids=prompt, images=images, max_new_tokens=8, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    with torch.no_grad():
        a = m.generate(do_sample=False, **kw)
        assert a.shape == (1, prompt.shape[1] + 8) and torch.equal(a[:, :prompt.shape[1]], prompt)
        assert torch.equal(a, m.generate(do_sample=False, **kw)), "deterministic"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, **kw)
        assert s.shape == a.shape
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, sampler="device", **kw)
        assert s.shape == a.shape and int(s.min()) >= 0 and int(s.max()) < m.config.vocab_size
        # (no use_cache=False run here: it re-embeds the generated ids, and this random tiny model generates an image-start id in A8, which
        # the model's own start / end token check refuses before the LLaMA layers are reached)


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_evaluate_runs(kv):
    from test_mxfp4_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    assert model.quantize_weights("mxfp4", activations="mxfp8_e4m3") is model and model.activation_quantization == "mxfp8_e4m3"
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    torch.manual_seed(77)
    ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9, kv_cache_dtype=kv, sampler="device")
    assert ids.dim() == 2 and ids.shape[0] == 1 and ids.numel() > 0
    assert all(bool(torch.isfinite(t.float()).all()) for t in list(masks) + list(boxes))


def test_decode_steps_equal_the_w4a16_model_from_the_same_cache():
    fx, w4 = _tiny()
    _, a8 = _tiny("mxfp8_e4m3")
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    with torch.no_grad():
        pf = [w4(input_ids=prompt, images=images, use_cache=True) for _ in range(2)]
        assert torch.equal(pf[0].logits, pf[1].logits)
        caches = [p.past_key_values for p in pf]
        tok = pf[0].logits[:, -1].argmax(-1, keepdim=True)
        for step in range(4):
            oa = w4(input_ids=tok, past_key_values=caches[0], use_cache=True, output_hidden_states=True)
            ob = a8(input_ids=tok, past_key_values=caches[1], use_cache=True, output_hidden_states=True)
            assert torch.equal(oa.logits, ob.logits), f"decode step {step}"
            assert torch.equal(oa.hidden_states[-1], ob.hidden_states[-1]), f"decode step {step}"
            tok = oa.logits[:, -1].argmax(-1, keepdim=True)
        assert caches[0].length == caches[1].length == prompt.shape[1] + 4
        assert not torch.equal(a8(input_ids=prompt, images=images).logits, pf[0].logits), "the A8 prefill is a different computation"


def test_without_activations_the_model_still_equals_its_twin():
    from test_mxfp4_weights_gpu import _tiny_core_pair
    fx, twin, mx = _tiny_core_pair()
    assert mx.activation_quantization is None
    with torch.no_grad():
        a, b = (m(**_inputs(fx), output_hidden_states=True) for m in (twin, mx))
        assert torch.equal(a.logits, b.logits)
        for i, (x, y) in enumerate(zip(a.hidden_states, b.hidden_states)):
            assert torch.equal(x, y), f"hidden state {i}"
