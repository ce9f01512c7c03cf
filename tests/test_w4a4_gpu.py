"""GPU: MXFP4 activations on MXFP4 weights (ops.linear_w4a4 / ull_gemm_w4a4_bf16, quantize_weights("mxfp4", activations="mxfp4_e2m1")).

The kernels are pinned to the definition in tests/test_w4a4_cpu.py:
  * the activation quantizer bit for bit against the weights' quantizer and the float64 restatement, over every finite bf16 bit pattern;
  * the operand layout of BOTH sides with one-hot data: one-hot activations give dequant(w).T, one-hot weights give dequant(xq) -- the
    second pins the activation nibble order, the private K-tile order and every activation scale byte;
  * bit for bit against the existing path (dequantize + bf16 GEMM) on data where every fp32 partial sum is exact in any order: both sides
    e2m1 values with a +-6 in every block, times a per-block 2^{0,1}, times a per-row 2^[-3, 3]: with the row factors taken out a term is a
    multiple of 0.25 and at most 6 * 6 * 4 = 576 quarters, and 576 * 11008 < 2^24 (the tests compute the real sum of |terms| and assert it);
  * against the float64 restatement on Gaussian data within the any-order fp32 accumulation bound plus one bf16 rounding;
  * at model level against the emulation built from existing kernels.
"""
import pytest
import torch

from helpers import core_model_from_fixture, load_fixture, pkg
from test_w4a4_cpu import mxfp4_rows_reference, special_rows, w4a4_exact
from test_w4a8_gpu import INT_SHAPES, _inputs, _varied_weight

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _same_as_both(ops, x_cpu, x_dev):
    """ops.quantize_rows_mxfp4(x_dev) against the weights' quantizer on the same rows and against the restatement; returns the codes."""
    codes, scales = ops.quantize_rows_mxfp4(x_dev)
    M, K = x_cpu.shape
    assert codes.shape == (M, K // 2) and scales.shape == (M, K // 32) and codes.dtype == scales.dtype == torch.uint8
    wc, ws = ops.quantize_mxfp4(x_dev.reshape(M, K).contiguous()).to_standard()
    assert torch.equal(codes, wc) and torch.equal(scales, ws), "the weights' own rule, bit for bit"
    rc, rs = mxfp4_rows_reference(x_cpu)
    assert torch.equal(codes.cpu(), rc) and torch.equal(scales.cpu(), rs), "the restatement, bit for bit"
    return codes


# ---- 1. the activation quantizer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 130])
@pytest.mark.parametrize("K", [32, 96, 4096, 2048 + 384])
def test_quantize_rows_mxfp4_equals_weight_rule_and_restatement(M, K):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(M * 10000 + K)
    x = torch.randn(M, K, generator=g) * 3.0
    x[:, ::37] *= 40.0                                            # outliers
    x *= torch.pow(2.0, torch.randint(-12, 13, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
    x[M // 2, :32] = 0
    x = x.to(BF)
    _same_as_both(ops, x, x.to(DEV))


def test_quantize_rows_mxfp4_special_blocks_and_strided_rows():
    ops = pkg("ops")
    x = special_rows()
    rc = _same_as_both(ops, x, x.to(DEV))
    wide = torch.full((x.shape[0], 96 + 64), 9.0, dtype=BF)
    wide[:, :96] = x
    c2, s2 = ops.quantize_rows_mxfp4(wide.to(DEV)[:, :96])        # ldx = K + 64
    assert torch.equal(c2, rc) and torch.equal(s2.cpu(), mxfp4_rows_reference(x)[1])
    x3 = x[:8].contiguous()
    c3, _ = ops.quantize_rows_mxfp4(x3.to(DEV).view(2, 4, 96))    # [B, S, K]
    assert torch.equal(c3, rc[:8])


@pytest.mark.parametrize("holder", [6 * 2.0 ** -3, 6.0, 6 * 2.0 ** 5, 4.0, 8.0])
def test_quantizer_sweep_over_every_finite_bf16_pattern(holder):
    """Every bf16 bit pattern except the NaN / Inf ones (exponent field all ones: 2 * 128 = 256 patterns, the only ones left out) as element 0
    of a block whose element 1 holds the scale (6 * 2^j: the pattern is rounded on the grid of step 2^j up to the block maximum; 4 * 2^j:
    the maximum is not the largest code).  A pattern larger than the holder sets the scale itself; the restatement covers that too."""
    ops = pkg("ops")
    bits = torch.arange(65536, dtype=torch.int32)
    finite = (bits & 0x7F80) != 0x7F80
    assert int((~finite).sum()) == 256
    pat = bits[finite].to(torch.int16).view(BF)                    # 65280 values
    n = pat.numel()
    rows = -(-n // 128)
    x = torch.zeros(rows * 128, 32, dtype=BF)
    x[:n, 0] = pat
    x[:, 1] = holder
    x = x.view(rows, 128 * 32)
    codes, scales = ops.quantize_rows_mxfp4(x.to(DEV))
    rc, rs = mxfp4_rows_reference(x)
    assert torch.equal(scales.cpu(), rs)
    bad = (codes.cpu() != rc).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} code bytes differ, first at {bad[0].tolist()}"
    assert torch.equal(codes, ops.quantize_mxfp4(x.to(DEV)).to_standard()[0])


# ---- 2. layout: one-hot, both sides -----------------------------------------------------------------------------------------------------
def _dequant_rows(ops, x):
    """dequant(quantize_rows_mxfp4(x)) as bf16: the activations the W4A4 Linear really multiplies (2 significant bits: exact in bf16)."""
    codes, scales = ops.quantize_rows_mxfp4(x)
    M = codes.shape[0]
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).view(M, -1).long()
    v = E2M1.to(x.device)[nib & 7] * torch.where((nib & 8) != 0, -1.0, 1.0)
    v = v.view(M, -1, 32) * torch.pow(2.0, scales.float() - 127)[..., None]
    return v.view(M, -1).to(BF).view(x.shape)


@pytest.mark.parametrize("K", [128, 2048 + 384])
def test_one_hot_activations_give_the_dequantized_weight(K):
    """x = the identity: y[m, n] = dequant(w)[n, m] exactly -- the weight side as the W4A8 test pins it (one superblock plus three tail tiles at
    K = 2432), now against an e2m1 second operand."""
    ops = pkg("ops")
    N = 48
    w = _varied_weight(N, K, 70 + K).to(DEV)
    q = ops.quantize_mxfp4(w)
    wd = ops.dequantize(q)
    assert torch.equal(wd, w), "the weight is exact in MXFP4"
    x = torch.eye(K, device=DEV, dtype=BF)
    got = ops.linear_w4a4(x, q, out_f32=True)
    assert got.dtype == torch.float32 and torch.equal(got, wd.float().T)
    # asymmetric activations too: row m = 2^(m % 5) at k = m
    x2 = (torch.eye(K) * torch.pow(2.0, (torch.arange(K) % 5).float())[:, None]).to(BF).to(DEV)
    assert torch.equal(_dequant_rows(ops, x2), x2)
    assert torch.equal(ops.linear_w4a4(x2, q, out_f32=True), wd.float().T * torch.pow(2.0, (torch.arange(K, device=DEV) % 5).float())[:, None])


@pytest.mark.parametrize("K", [128, 2048 + 384])
def test_one_hot_weights_give_the_dequantized_activations(K):
    """The mirror: w = the identity (1.0 is exact in MXFP4), activations carrying every e2m1 magnitude, both signs and block scales that differ
    between neighbours: y[m, n] = dequant(xq)[m, n] exactly -- the activation nibble order, the private K-tile order and the scale byte of every
    (row, block)."""
    ops = pkg("ops")
    M = 40
    x = _varied_weight(M, K, 90 + K).to(DEV)
    xd = _dequant_rows(ops, x)
    assert torch.equal(xd, x), "the activations are exact in MXFP4"
    sc = ops.quantize_rows_mxfp4(x)[1]
    assert bool((sc[:, 1:] != sc[:, :-1]).all()), "neighbouring block scales all differ"
    nib = ops.quantize_rows_mxfp4(x)[0]
    assert set((nib & 15).flatten().tolist()) | set((nib >> 4).flatten().tolist()) >= set(range(1, 8)) | set(range(9, 16)), "every magnitude, both signs"
    q = ops.quantize_mxfp4(torch.eye(K, device=DEV, dtype=BF))
    got = ops.linear_w4a4(x, q, out_f32=True)
    assert torch.equal(got, xd.float())
    assert torch.equal(ops.linear_w4a4(x, q), xd)


# ---- 3. bit for bit against the existing path -------------------------------------------------------------------------------------------
def _rows(rows, K, seed, mag=0, slot=2, zero_row=False):
    """(bf16 [rows, K] on the GPU, per-row exponent): e2m1 values with a +-6 in every block, times a per-block 2^{0,1}, times 2^e_row,
    e_row in [-3, 3] + mag."""
    g = torch.Generator().manual_seed(seed)
    v = E2M1[torch.randint(0, 8, (rows, K), generator=g)] * (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float()
    v.view(rows, K // 32, 32)[:, :, slot] = 6.0 * (torch.arange(K // 32) % 2 * 2 - 1).float()
    v *= torch.pow(2.0, torch.randint(0, 2, (rows, K // 32), generator=g).float()).repeat_interleave(32, 1)
    e = (torch.arange(rows) * 5 % 7 - 3 + mag).float()
    v *= torch.pow(2.0, e)[:, None]
    if zero_row and rows > 5:
        v[3] = 0
    return v.to(BF).to(DEV), e


def _assert_exactly_summable(x, ex, w, ew):
    """sum |terms| of every output, in units of its quantum 0.25 * 2^(e_m + e_n), stays below 2^24: every fp32 partial sum is exact."""
    absum = x.cpu().double().abs() @ w.cpu().double().abs().T
    quanta = absum / (0.25 * torch.pow(2.0, ex.double())[:, None] * torch.pow(2.0, ew.double())[None, :])
    assert float(quanta.max()) < 2 ** 24, float(quanta.max())
    assert float(quanta.max()) <= 576 * x.shape[1]


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_kernel_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x, ex = _rows(M, K, 1000 + M, slot=1, zero_row=True)
    w, ew = _rows(N, K, 2000 + N)
    _assert_exactly_summable(x, ex, w, ew)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize(q), w), "the weights are exact in MXFP4"
    assert torch.equal(_dequant_rows(ops, x), x), "the activations are exact in MXFP4: ops.linear on x is the existing path"
    sc = ops.quantize_rows_mxfp4(x)[1]
    assert len(set(sc.flatten().tolist())) > 2, "block scales vary"
    r = _rows(M, N - N % 32 + 32, 3000 + M)[0][:, :N].contiguous()
    with torch.no_grad():
        assert torch.equal(ops.linear_w4a4(x, q), ops.linear(x, q)), "no epilogue"
        assert torch.equal(ops.linear_w4a4(x, q, residual=r), ops.linear(x, q, residual=r)), "residual"
        assert torch.equal(ops.linear_w4a4(x, q, out_f32=True), ops.linear(x, q, out_f32=True)), "fp32 output"
        out = ops.linear_w4a4(x, q)
        assert bool(out.float().abs().sum() > 0)
        if M > 5:
            assert not bool(out[3].any()), "the all-zero row gives zeros"


@pytest.mark.parametrize("K", [4096, 2048 + 128])
def test_kernel_full_grid_equals_existing_path_bit_for_bit(K):
    """The superblock loop with two blocks on every CU (16 x 32 tiles of 128 x 128), at a K that is whole superblocks only (no tail tile
    follows the last super tile: the staging schedule's last steps differ) and at one with a tail: memory latency under a full grid is
    what a counted wait has to survive."""
    ops = pkg("ops")
    M, N = 2048, 4096
    x, ex = _rows(M, K, 7000 + K, slot=1)
    w, ew = _rows(N, K, 7001 + K)
    _assert_exactly_summable(x, ex, w, ew)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(ops.dequantize(q), w) and torch.equal(_dequant_rows(ops, x), x)
    with torch.no_grad():
        want = ops.linear(x, q, out_f32=True)
        for _ in range(3):
            assert torch.equal(ops.linear_w4a4(x, q, out_f32=True), want)


@pytest.mark.parametrize("M,N,K", [(129, 320, 256), (17, 64, 128), (40, 2 * 144, 2176)])
def test_kernel_swiglu_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x, ex = _rows(M, K, 4000 + M, slot=1, zero_row=True)
    # |gate| far below 88 (the shared SiLU code returns NaN where exp(-gate) overflows): |x| <= 96, |w| <= 12 * 2^(3 - 22), K <= 2176
    w, ew = _rows(N, K, 5000 + N, mag=-22)
    _assert_exactly_summable(x, ex, w, ew)
    q = ops.quantize_mxfp4(w)
    assert torch.equal(_dequant_rows(ops, x), x), "the activations are exact in MXFP4: ops.linear on x is the existing path"
    with torch.no_grad():
        a, b = ops.linear_w4a4(x, q, swiglu=True), ops.linear(x, q, swiglu=True)
        assert bool(torch.isfinite(b.float()).all()) and float(ops.linear(x, q).float().abs().max()) < 80.0
    assert a.shape == (M, N // 2) and torch.equal(a, b)
    assert bool(a.float().abs().sum() > 0)


def test_kernel_strided_input_and_output():
    ops = pkg("ops")
    M, N, K = 70, 200, 256
    xw = _rows(M, K + 64, 6000)[0]
    x = xw[:, :K]                                                  # ldx = K + 64
    q = ops.quantize_mxfp4(_rows(N, K, 6001)[0])
    want = ops.linear(x.contiguous(), q)
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_w4a4(x, q, out=outw[:, :N])                   # ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"
    x3 = x.contiguous().view(2, 35, K)                             # 3-D activations [B, S, K] and a 3-D residual
    r3 = _rows(M, 224, 6002)[0][:, :N].contiguous().view(2, 35, N)
    assert torch.equal(ops.linear_w4a4(x3, q, residual=r3), ops.linear(x3, q, residual=r3))


# ---- 4. tile independence, 5. Gaussian accuracy -------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_rows_sharing_a_tile():
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 4096, generator=g).to(BF).to(DEV)
    q = ops.quantize_mxfp4((torch.randn(264, 4096, generator=g) * 0.02).to(BF).to(DEV))
    full = ops.linear_w4a4(x, q)
    assert torch.equal(full[131:132], ops.linear_w4a4(x[131:132].contiguous(), q)), "a row computed alone"
    assert torch.equal(full[131:160], ops.linear_w4a4(x[131:160].contiguous(), q)), "29 rows, another place in the tile, another grid"


def test_kernel_random_data_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 300, 520, 4096
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * 0.02)
    w[::97] *= 8.0
    q = ops.quantize_mxfp4(w.to(BF).to(DEV))
    wc, ws = (t.cpu() for t in q.to_standard())
    out = ops.linear_w4a4(x.to(DEV), q).cpu().double()
    y, absum = w4a4_exact(x, wc, ws)
    # K * 2^-23 * sum |terms|: fp32 accumulation in any order (truncation inside the instruction allowed); 2^-8 |y|: the rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -8 * y.abs()
    err = (out - y).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y| = {float(y.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"
    f32 = ops.linear_w4a4(x.to(DEV), q, out_f32=True).cpu().double()
    e32 = (f32 - y).abs()
    print(f"fp32 output: max err / bound = {float((e32 / (K * 2.0 ** -23 * absum).clamp_min(1e-300)).max()):.4f}")
    assert bool((e32 <= K * 2.0 ** -23 * absum).all()), "fp32 output: the accumulation bound alone"


# ---- 6. tiny models (K < 2048: the standard-order phase only; the kernel tests above cover superblocks) --------------------------------------
MODE = "mxfp4_e2m1"


def _tiny(activations=None):
    fx = load_fixture("g1_core_tiny_bf16.pt")
    model, _ = core_model_from_fixture(fx, DEV)
    model.quantize_weights("mxfp4", activations=activations)
    return fx, model


def emulation(x, w, residual=None, swiglu=False, out=None, out_f32=False):
    """ops.linear_w4a4 out of existing kernels: the W4A16 Linear (dequantize + bf16 GEMM) on the quantize-dequantized activations."""
    ops = pkg("ops")
    return ops.linear(_dequant_rows(ops, x), w, residual=residual, swiglu=swiglu, out=out, out_f32=out_f32)


def test_mode_switch_and_attribute():
    fx, m = _tiny()
    assert m.weight_quantization == "mxfp4" and m.activation_quantization is None
    codes = m._packed["llama"][0]["w_o"].codes
    assert m.quantize_weights("mxfp4", activations=MODE) is m                       # switching the mode on: no weight changes
    assert m.activation_quantization == MODE and m._packed["llama"][0]["w_o"].codes is codes
    assert m.quantize_weights("mxfp4") is m and m.activation_quantization == MODE
    with pytest.raises(NotImplementedError):
        m.quantize_weights("mxfp4", activations=MODE, activation_scope="prefill+decode")
    _, fresh = _tiny(MODE)
    assert fresh.weight_quantization == "mxfp4" and fresh.activation_quantization == MODE


def test_model_takes_the_new_entry_only_at_gemm_shapes(monkeypatch):
    ops, L_ = pkg("ops"), pkg("_lib")
    fx, m = _tiny(MODE)
    calls, entries = [], []
    real, real_call = ops.linear_w4a4, L_.call
    monkeypatch.setattr(ops, "linear_w4a4", lambda x, w, **kw: calls.append((x.shape[0], tuple(w.shape))) or real(x, w, **kw))
    monkeypatch.setattr(L_, "call", lambda name, *a: (entries.append(name) if name in ("ull_gemm_w4a4_bf16", "ull_gemm_w4a8_bf16") else None) or real_call(name, *a))
    L = len(m.model.layers)
    with torch.no_grad():
        m(**_inputs(fx))
        assert len(calls) == 4 * L and entries == ["ull_gemm_w4a4_bf16"] * (4 * L) and {c[0] for c in calls} == {26}, "q|k|v, o_proj, gate|up, down_proj of every layer"
        del calls[:], entries[:]
        out = m(input_ids=fx["greedy_prompt"].to(DEV), images=fx["images"][:1].to(DEV), use_cache=True)
        assert len(calls) == 4 * L and len(entries) == 4 * L
        del calls[:], entries[:]
        m(input_ids=torch.tensor([[5]], device=DEV), past_key_values=out.past_key_values, use_cache=True)
        assert calls == [] and entries == [], "a decode step stays W4A16"


def test_batch_invariance():
    fx, m = _tiny(MODE)
    inp = _inputs(fx)
    with torch.no_grad():
        both = m(**inp, output_hidden_states=True)
        for b in range(2):
            one = m(**{k: v[b:b + 1] for k, v in inp.items()}, output_hidden_states=True)
            assert torch.equal(both.logits[b:b + 1], one.logits), f"logits of sample {b}"
            for i, (hb, h1) in enumerate(zip(both.hidden_states, one.hidden_states)):
                assert torch.equal(hb[b:b + 1], h1), f"hidden state {i} of sample {b}"


def test_model_error_against_the_emulation(monkeypatch):
    """The new path's logit error against the fixture's reference logits may be at most 1.5 x that of the same model with ops.linear_w4a4
    replaced by the emulation out of existing kernels (same math, another rounding order; both sides share the 4-bit loss): the rule of
    tests/test_a8w8_gpu.py."""
    ops = pkg("ops")
    fx, m = _tiny(MODE)
    ref = fx["logits"].float()
    with torch.no_grad():
        new = m(**_inputs(fx)).logits.float().cpu()
        monkeypatch.setattr(ops, "linear_w4a4", emulation)
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
    fx, m = _tiny(MODE)
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    kw = dict(input_ids=prompt, images=images, max_new_tokens=8, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    with torch.no_grad():
        a = m.generate(do_sample=False, **kw)
        assert a.shape == (1, prompt.shape[1] + 8) and torch.equal(a[:, :prompt.shape[1]], prompt)
        assert torch.equal(a, m.generate(do_sample=False, **kw)), "deterministic"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, **kw)
        torch.manual_seed(3)
        assert s.shape == a.shape and torch.equal(s, m.generate(do_sample=True, temperature=0.7, top_p=0.9, **kw)), "deterministic under a seed"
        torch.manual_seed(3)
        s = m.generate(do_sample=True, temperature=0.7, top_p=0.9, sampler="device", **kw)
        assert s.shape == a.shape and int(s.min()) >= 0 and int(s.max()) < m.config.vocab_size


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_evaluate_runs(kv):
    from test_mxfp4_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    assert model.quantize_weights("mxfp4", activations=MODE) is model and model.activation_quantization == MODE
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9, kv_cache_dtype=kv, sampler="device")
        assert ids.dim() == 2 and ids.shape[0] == 1 and ids.numel() > 0
        assert all(bool(torch.isfinite(t.float()).all()) for t in list(masks) + list(boxes))
        runs.append(ids)
    assert torch.equal(runs[0], runs[1]), "deterministic under a seed"


def test_decode_steps_equal_the_w4a16_model_from_the_same_cache():
    fx, w4 = _tiny()
    _, a4 = _tiny(MODE)
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    with torch.no_grad():
        pf = [w4(input_ids=prompt, images=images, use_cache=True) for _ in range(2)]
        assert torch.equal(pf[0].logits, pf[1].logits)
        caches = [p.past_key_values for p in pf]
        tok = pf[0].logits[:, -1].argmax(-1, keepdim=True)
        for step in range(4):
            oa = w4(input_ids=tok, past_key_values=caches[0], use_cache=True, output_hidden_states=True)
            ob = a4(input_ids=tok, past_key_values=caches[1], use_cache=True, output_hidden_states=True)
            assert torch.equal(oa.logits, ob.logits), f"decode step {step}"
            assert torch.equal(oa.hidden_states[-1], ob.hidden_states[-1]), f"decode step {step}"
            tok = oa.logits[:, -1].argmax(-1, keepdim=True)
        assert caches[0].length == caches[1].length == prompt.shape[1] + 4
        assert not torch.equal(a4(input_ids=prompt, images=images).logits, pf[0].logits), "the A4 prefill is a different computation"


def test_without_activations_the_model_still_equals_its_twin():
    from test_mxfp4_weights_gpu import _tiny_core_pair
    fx, twin, mx = _tiny_core_pair()
    assert mx.activation_quantization is None
    with torch.no_grad():
        a, b = (m(**_inputs(fx), output_hidden_states=True) for m in (twin, mx))
        assert torch.equal(a.logits, b.logits)
        for i, (x, y) in enumerate(zip(a.hidden_states, b.hidden_states)):
            assert torch.equal(x, y), f"hidden state {i}"
