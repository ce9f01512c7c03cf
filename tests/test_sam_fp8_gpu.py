"""GPU: the opt-in FP8 (W8A8) Linears of the SAM image encoder (ops.layernorm_quantize_rows_fp8 / ull_layernorm_quantize_rows_fp8_bf16,
ops.linear_a8w8_rows / ull_gemm_a8w8_epi_bf16, SamEngine.linear_precision = "fp8_e4m3", DESIGN f12).

  * the fused norm + quantize launch is pinned bit for bit to the two launches it replaces;
  * the GEMM entry is pinned as tests/test_a8w8_gpu.py pins ull_gemm_a8w8_bf16: bit for bit against the existing path on data where every fp32
    partial sum is exact (every epilogue the entry adds), against the fp64 restatement on Gaussian data, and row by row;
  * the encoder is compared with its emulation out of existing kernels (quantize rows -> dequantize -> W8A16 Linear), and the default path
    with itself.
"""
import pytest
import torch

from helpers import fixture_sd, load_fixture, pkg
from test_a8w8_cpu import a8w8_exact
from test_a8w8_gpu import _int_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16


# ---- 1. fused LayerNorm + row quantization ----------------------------------------------------------------------------------------------
def _ln_params(K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, generator=g) * 0.2 + 1.0).to(BF).to(DEV), (torch.randn(K, generator=g) * 0.1).to(BF).to(DEV)


def _both(ops, x, w, b, eps=1e-6):
    """(fused, unfused) = ((codes, scales), (codes, scales))"""
    return ops.layernorm_quantize_rows_fp8(x, w, b, eps), ops.quantize_rows_fp8(ops.layernorm(x, w, b, eps))


# (M, K): one row, fewer rows than a block's four, more than one block; K = 1280 / 5120 (ViT-H: 3 and 10 chunks per lane), 64 (8 lanes hold the
# row) and 160 (20 chunks: a partly filled wave)
@pytest.mark.parametrize("M,K", [(1, 1280), (5, 1280), (130, 1280), (9, 5120), (7, 64), (33, 160)])
def test_fused_norm_quantize_equals_the_two_launches(M, K):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(100 + M + K)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    w, b = _ln_params(K, 7 + K)
    (c, s), (rc, rs) = _both(ops, x, w, b)
    assert c.dtype == torch.uint8 and c.shape == (M, K) and s.dtype == torch.float32 and s.shape == (M,)
    assert torch.equal(s, rs) and torch.equal(c, rc)
    assert bool(c.any()), "codes were written"
    # rows with outliers: a few columns x 40 move the mean, the variance and the scale
    xo = x.clone()
    xo[:, ::max(K // 5, 1)] *= 40.0
    (c, s), (rc, rs) = _both(ops, xo, w, b)
    assert torch.equal(s, rs) and torch.equal(c, rc)
    # rows of a wider buffer (ldx > K)
    wide = torch.full((M, K + 72), 3.0, dtype=BF, device=DEV)
    wide[:, :K] = x
    (c, s), (rc, rs) = _both(ops, wide[:, :K], w, b)
    want = ops.quantize_rows_fp8(ops.layernorm(x, w, b, 1e-6))
    assert torch.equal(c, rc) and torch.equal(s, rs) and torch.equal(c, want[0]) and torch.equal(s, want[1])


@pytest.mark.parametrize("K", [64, 1280])
def test_fused_norm_quantize_constant_row_with_zero_bias(K):
    """x = 1 everywhere: the fp32 mean is exactly 1 (K a power of two; K = 1280: 1280 * fl(1 / 1280) rounds to 1), so the normed row is all zero
    whatever the gain -- scale 2^0, codes 0 -- next to ordinary rows."""
    ops = pkg("ops")
    x = torch.randn(6, K, generator=torch.Generator().manual_seed(3)).to(BF).to(DEV)
    x[2] = 1.0
    w, _ = _ln_params(K, 11)
    b = torch.zeros(K, dtype=BF, device=DEV)
    (c, s), (rc, rs) = _both(ops, x, w, b)
    assert torch.equal(c, rc) and torch.equal(s, rs)
    assert float(s[2]) == 1.0 and not bool(c[2].any()) and bool(c[1].any())


# ---- 2. the GEMM entry, bit for bit -------------------------------------------------------------------------------------------------------
# (M, N, K): the kernel's tile is 128 x 128 with a K-tile of 128 codes; (33, 48, 64) pads K; (40, 144, 5120) is lin2's K; (1100, 520, 256) sends
# the bf16 comparison through the 256 x 256 kernel
INT_SHAPES = [(127, 127, 128), (129, 129, 384), (17, 200, 128), (5, 136, 256), (33, 48, 64), (40, 144, 5120), (1100, 520, 256)]


def _int_bias(N, seed):
    """bf16 [N]: integers in [-6, 6] times 2^-2"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-6, 7, (N,), generator=g).float() * 0.25).to(BF).to(DEV)


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_gemm_equals_existing_path_bit_for_bit(M, N, K):
    ops = pkg("ops")
    x = _int_rows(M, K, 1000 + M, special=True)
    q = ops.quantize_fp8(_int_rows(N, K, 2000 + N))
    bias = _int_bias(N, 3000 + N)
    r = _int_rows(M, N, 4000 + M)
    xq, xs = ops.quantize_rows_fp8(x)
    assert torch.equal(ops.dequantize(ops.Fp8Weight(xq, xs)), x), "the integer rows are exact in e4m3"
    new = lambda **kw: ops.linear_a8w8_rows(xq, xs, q, **kw)
    old = lambda bias=None, **kw: ops.linear(x, q, bias, **kw)
    with torch.no_grad():
        assert torch.equal(new(bias=bias), old(bias=bias)), "bias"
        assert torch.equal(new(bias=bias, act="gelu"), old(bias=bias, act="gelu")), "bias + gelu"
        # QuickGELU: the shared sigmoid code returns NaN where exp(1.702 |t|) overflows (t below about -52; these products reach thousands), and
        # NaN != NaN: compared as bit patterns here, and once more on weights 2^-16 smaller, where every output is finite
        a, b = new(bias=bias, act="quick_gelu"), old(bias=bias, act="quick_gelu")
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "bias + quick_gelu"
        qs = ops.quantize_fp8((_int_rows(N, K, 2000 + N).float() * 2.0 ** -16).to(BF))
        a, b = ops.linear_a8w8_rows(xq, xs, qs, bias=bias, act="quick_gelu"), ops.linear(x, qs, bias, act="quick_gelu")
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), "bias + quick_gelu, finite"
        assert torch.equal(new(bias=bias, residual=r), old(bias=bias, residual=r)), "bias + residual"
        f = new(bias=bias, out_f32=True)
        assert f.dtype == torch.float32 and torch.equal(f, old(bias=bias, out_f32=True)), "bias + fp32 output"
        assert torch.equal(new(), old()) and torch.equal(new(), ops.linear_a8w8(x, q)), "no bias"
        plain = new(bias=bias)
        assert bool(plain.float().abs().sum() > 0) and (M <= 5 or torch.equal(plain[3], bias)), "the all-zero row gives the bias"
        assert not torch.equal(new(bias=bias, act="gelu"), plain) and not torch.equal(new(), plain)


def test_gemm_strided_output():
    ops = pkg("ops")
    M, N, K = 70, 200, 256
    x = _int_rows(M, K, 6000)
    q = ops.quantize_fp8(_int_rows(N, K, 6001))
    bias = _int_bias(N, 6002)
    xq, xs = ops.quantize_rows_fp8(x)
    want = ops.linear(x, q, bias, act="gelu")
    outw = torch.full((M, N + 56), 7.0, device=DEV, dtype=BF)
    got = ops.linear_a8w8_rows(xq, xs, q, bias=bias, act="gelu", out=outw[:, :N])      # ldc = N + 56
    assert got.data_ptr() == outw.data_ptr() and torch.equal(outw[:, :N], want)
    assert bool((outw[:, N:] == 7.0).all()), "nothing is written beyond N"


# ---- 3. Gaussian data against the fp64 restatement ----------------------------------------------------------------------------------------
def test_gemm_random_data_with_bias_within_the_fp32_accumulation_bound():
    ops = pkg("ops")
    M, N, K = 300, 520, 1280
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(BF)
    w = torch.randn(N, K, generator=g) * 0.02
    w[::97] *= 8.0
    bias = (torch.randn(N, generator=g) * 0.5).to(BF)
    q = ops.quantize_fp8(w.to(BF).to(DEV))
    out = ops.linear_a8w8_rows(*ops.quantize_rows_fp8(x.to(DEV)), q, bias=bias.to(DEV)).cpu().double()
    y, absum = a8w8_exact(x, q.codes, q.scales)
    yb = y + bias.double()[None, :]
    # K * 2^-23 * absum: fp32 accumulation in any order; 2^-23 |y + b|: the fp32 bias add; 2^-8 |y + b|: the final rounding to bf16
    bound = K * 2.0 ** -23 * absum + 2.0 ** -23 * yb.abs() + 2.0 ** -8 * yb.abs()
    err = (out - yb).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.4f}; max |y + b| = {float(yb.abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements beyond the bound"


# ---- 4. row independence -----------------------------------------------------------------------------------------------------------------
def test_gemm_rows_do_not_depend_on_the_rows_sharing_a_tile():
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 1280, generator=g).to(BF).to(DEV)
    q = ops.quantize_fp8((torch.randn(264, 1280, generator=g) * 0.02).to(BF).to(DEV))
    bias = (torch.randn(264, generator=g) * 0.5).to(BF).to(DEV)
    xq, xs = ops.quantize_rows_fp8(x)
    full = ops.linear_a8w8_rows(xq, xs, q, bias=bias, act="gelu")
    part = ops.linear_a8w8_rows(xq[131:160].contiguous(), xs[131:160].contiguous(), q, bias=bias, act="gelu")   # another place in the tile, another grid
    assert torch.equal(full[131:160], part) and bool(part.any())


# ---- 5. / 6. the encoder at ViT-H width --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g9():
    """One windowed + one global ViT-H block (d = 1280) on one 1024 x 1024 image, as tests/test_sam_gpu.py builds it; the bf16 encode of the
    default engine is computed once and shared."""
    C, S = pkg("configuration"), pkg("sam")
    fx = load_fixture("g9_sam_blocks_bf16.pt")
    cfg = C.SamConfig(depth=2, global_attn_indexes=[1])
    holder = S.build_sam_holder(cfg, device=DEV, dtype=BF)
    sd = {k[len("visual_model."):]: v for k, v in fixture_sd(fx, BF).items()}
    assert not holder.load_state_dict(sd, strict=False).unexpected_keys
    img = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(fx["image_seed"])).to(BF).to(DEV)
    base = S.SamEngine(holder, cfg).encode(img)
    return dict(fx=fx, cfg=cfg, holder=holder, img=img, base=base, S=S)


def _sample_err(fx, out):
    got = out.cpu().view(1, 64, 64, 256).permute(0, 3, 1, 2)[:, ::2, ::2, ::2].float()
    e = (got - fx["embedding_sample"].float()).abs()
    return float(e.max()), float(e.mean())


def _emulate(monkeypatch, ops):
    """the two new wrappers as compositions of existing kernels"""
    def lnq(x, w, b, eps):
        return ops.quantize_rows_fp8(ops.layernorm(x, w, b, eps))

    def rows(xq, xs, w, bias=None, act=None, residual=None, out=None, out_f32=False):
        return ops.linear(ops.dequantize(ops.Fp8Weight(xq, xs)), w, bias, act=act, residual=residual, out=out, out_f32=out_f32)
    monkeypatch.setattr(ops, "layernorm_quantize_rows_fp8", lnq)
    monkeypatch.setattr(ops, "linear_a8w8_rows", rows)


def _count(monkeypatch, ops, *names):
    n = {k: 0 for k in names}
    for k in names:
        real = getattr(ops, k)

        def spy(*a, _k=k, _real=real, **kw):
            n[_k] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, k, spy)
    return n


def test_encoder_error_against_the_emulation(g9, monkeypatch):
    """The fp8 encode's error against the fixture's reference output may be at most 1.5 x the error of the same engine with the two new
    wrappers replaced by existing kernels (same math, another rounding order) -- the rule of test_model_error_against_the_emulation."""
    ops = pkg("ops")
    eng = g9["S"].SamEngine(g9["holder"], g9["cfg"])
    eng.linear_precision = "fp8_e4m3"
    n = _count(monkeypatch, ops, "linear_a8w8_rows", "layernorm_quantize_rows_fp8", "quantize_rows_fp8", "sam_blocks", "linear_a8w8")
    new = eng.encode(g9["img"])
    depth = g9["cfg"].depth
    assert n["linear_a8w8_rows"] == 4 * depth, "qkv, proj, lin1, lin2 of every block"
    assert n["layernorm_quantize_rows_fp8"] == 2 * depth, "norm1 -> qkv (image-order window path, global block) and norm2 -> lin1"
    assert n["quantize_rows_fp8"] == 2 * depth, "attention -> proj and GELU -> lin2"
    assert n["sam_blocks"] == 0 and n["linear_a8w8"] == 0
    assert "_fp8" in eng._pk and len(eng._pk["_fp8"][0]) == depth
    monkeypatch.undo()
    _emulate(monkeypatch, ops)
    emu = eng.encode(g9["img"])
    monkeypatch.undo()
    (new_max, new_mean), (emu_max, emu_mean), (bf_max, bf_mean) = (_sample_err(g9["fx"], t) for t in (new, emu, g9["base"]))
    print(f"encoder error vs the reference fixture: fp8 max {new_max:.5f} mean {new_mean:.6f}; emulation max {emu_max:.5f} mean {emu_mean:.6f}; "
          f"bf16 max {bf_max:.5f} mean {bf_mean:.6f}; max|ref| {g9['fx']['embedding_max']:.3f}")
    assert bool(torch.isfinite(new.float()).all()) and new.dtype == BF and new.shape == g9["base"].shape
    assert emu_max > 0, "the emulation is an fp8 encoder too: it cannot equal the bf16 reference"
    assert new_max <= 1.5 * emu_max and new_mean <= 1.5 * emu_mean
    assert not torch.equal(new, g9["base"]), "the fp8 mode changed nothing"


def test_default_is_untouched_and_the_packs_go_with_invalidate(g9):
    ops = pkg("ops")
    eng = g9["S"].SamEngine(g9["holder"], g9["cfg"])
    assert eng.linear_precision is None and torch.equal(eng.encode(g9["img"]), g9["base"])
    assert "_fp8" not in eng._pk, "no fp8 codes without the switch"
    eng.linear_precision = "fp8_e4m3"
    a = eng.encode(g9["img"])
    packs = eng._pk["_fp8"][0]
    assert isinstance(packs[0][0], ops.Fp8Weight) and tuple(packs[0][0].shape) == (3 * 1280, 1280) and tuple(packs[1][3].shape) == (1280, 5120)
    assert torch.equal(eng.encode(g9["img"]), a) and eng._pk["_fp8"][0] is packs, "deterministic; the codes are made once"
    eng.linear_precision = None
    assert torch.equal(eng.encode(g9["img"]), g9["base"]), "switched back: the same bits as an engine never switched"
    with ops.per_op_layers():
        assert torch.equal(eng.encode(g9["img"]), g9["base"]), "... on the per-op loop as well"
    eng.invalidate()
    assert eng._pk is None
    assert torch.equal(eng.encode(g9["img"]), g9["base"]) and "_fp8" not in eng._pk
    # the bf16 parameters are where they were
    assert all(p.dtype == BF for p in g9["holder"].parameters())


def test_encoder_combines_with_the_exact_global_attention(g9, monkeypatch):
    ops = pkg("ops")
    eng = g9["S"].SamEngine(g9["holder"], g9["cfg"])
    eng.linear_precision = "fp8_e4m3"
    a = eng.encode(g9["img"])
    eng.global_attention = "exact"
    n = _count(monkeypatch, ops, "linear_a8w8_rows", "sam_global_attention_exact", "sam_blocks")
    b = eng.encode(g9["img"])
    assert n == {"linear_a8w8_rows": 4 * g9["cfg"].depth, "sam_global_attention_exact": 1, "sam_blocks": 0}
    assert bool(torch.isfinite(b.float()).all()) and not torch.equal(a, b)


# ---- 7. the generic (partitioned) path and evaluate ------------------------------------------------------------------------------------------
def _eval_args(fx):
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF).to(DEV)
    return images_sam, (images_sam[:1], fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])


def _finite(masks, boxes):
    return all(bool(torch.isfinite(t.float()).all()) for t in list(masks) + list(boxes))


def test_tiny_model_generic_path_and_evaluate(monkeypatch):
    """g8's SAM has embed 64, head dim 32, K = 64 / 256: windows are partitioned (norm1 stays a launch of its own there), K = 64 is padded."""
    from test_fp8_weights_gpu import _tiny_full
    ops = pkg("ops")
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    images_sam, args = _eval_args(fx)
    base = model._sam.encode(images_sam)
    assert model.set_sam_precision("fp8_e4m3") is model and model.sam_precision == "fp8_e4m3"
    n = _count(monkeypatch, ops, "linear_a8w8_rows", "layernorm_quantize_rows_fp8", "sam_blocks")
    both = model._sam.encode(images_sam)
    depth = len(model.visual_model.image_encoder.blocks)
    assert n == {"linear_a8w8_rows": 4 * depth, "layernorm_quantize_rows_fp8": 2 * depth - 1, "sam_blocks": 0}, "block 0 partitions its normed rows"
    monkeypatch.undo()
    assert bool(torch.isfinite(both.float()).all()) and not torch.equal(both, base)
    # batch invariance: sample b of the 2-image encode equals its single-image encode
    for b in range(2):
        assert torch.equal(model._sam.encode(images_sam[b:b + 1]), both[b:b + 1]), f"sample {b}"
    torch.manual_seed(77)
    ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9)
    assert ids.dim() == 2 and ids.shape[0] == 1 and _finite(masks, boxes)
    # ... together with fp8 weights and activations in the language model
    assert model.quantize_weights("fp8_e4m3", activations="fp8_e4m3") is model and model.sam_precision == "fp8_e4m3"
    torch.manual_seed(77)
    ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9)
    assert ids.dim() == 2 and ids.shape[0] == 1 and _finite(masks, boxes)


def test_evaluate_with_the_exact_global_attention():
    """set_sam_attention("exact") refuses g8's own SAM (head dim 32 has no exact kernel, and the streamed form is never substituted), so this
    model keeps g8's language model, heads and mask decoder and gets a seeded image encoder of head dim 80 (embed 160: K = 160 / 640, both
    padded to whole K-tiles; block 0 on the image-order window path, block 1 on the exact global kernel)."""
    C, M = pkg("configuration"), pkg("modeling_ullava")
    fx = load_fixture("g8_full_tiny_bf16.pt")
    cfg, cd = fx["cfg"], fx["cfg"]["llm"]
    ucfg = C.UllavaConfig(llm_config=dict(vision_config=cd["vision_config"], vision_hidden_layer=cd["vision_hidden_layer"], projector_type="mlp",
                                          projector_from_scratch=bool(cd.get("projector_from_scratch", False)), mm_token_ids=cd["mm_token_ids"],
                                          vocab_size=cd["vocab_size"], hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"],
                                          num_hidden_layers=cd["num_hidden_layers"], num_attention_heads=cd["num_attention_heads"]),
                          seg_token_idx=cfg["seg_token_idx"], loc_token_idx=cfg["loc_token_idx"], sam_config=dict(cfg["sam"], embed_dim=160, num_heads=2))
    model = M.UllavaForCausalLM(ucfg, device=DEV)
    res = model.load_state_dict({k: v for k, v in fixture_sd(fx, BF).items() if not k.startswith("visual_model.image_encoder.")}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("visual_model.image_encoder.") for k in res.missing_keys)
    g = torch.Generator(device="cuda").manual_seed(51)
    with torch.no_grad():
        for name, p in model.visual_model.image_encoder.named_parameters():
            if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name in ("neck.1.weight", "neck.3.weight"):
                p.fill_(1.0)
            else:
                p.copy_((torch.randn(p.shape, device=DEV, generator=g) * (0.05 if p.dim() > 1 else 0.1)).to(BF))
    _, args = _eval_args(fx)
    model.set_sam_precision("fp8_e4m3").set_sam_attention("exact")
    torch.manual_seed(77)
    ids, masks, boxes = model.evaluate(*args, max_new_tokens=6, temperature=0.2, top_p=0.9)
    assert ids.dim() == 2 and ids.shape[0] == 1 and _finite(masks, boxes)
    a = model._sam.encode(args[0])
    model.set_sam_precision(None)
    b = model._sam.encode(args[0])
    assert bool(torch.isfinite(a.float()).all()) and not torch.equal(a, b)
