"""GPU: FP8 (e4m3) weight-only inference (UllavaCoreForCausalLM.quantize_weights).

The contract is bit-identity with the TWIN: the same bf16 model whose LLaMA Linear weights (and lm_head) are replaced by dequant(Q(W)) =
float(code) * 2^s, which is exactly representable in bf16.  Every fp8 path (GEMV, RMSNorm-GEMV, q|k|v + RoPE + cache append, skinny MFMA,
dequantize + GEMM at prefill shapes, the coarse decode entry) feeds its FMAs / MFMAs the values the bf16 kernel it mirrors reads from the
twin's weight, in the same order -- so every comparison below is torch.equal.
"""
import ctypes
import os
import sys

import pytest
import torch

from helpers import fixture_sd, load_fixture, pkg
from test_fp8_weights_cpu import dequant_reference, edge_rows, fp8_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rand(*shape, sc=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * sc).to(BF)


def _weight(N, K, seed):
    """N(0, 0.02) with a few outlier rows / elements, as trained weights have."""
    w = _rand(N, K, sc=0.02, seed=seed).float()
    w[::97] *= 8.0
    w[:, ::331] *= 3.0
    return w.to(BF)


def _twin_weight(w):
    ops = pkg("ops")
    return ops.dequantize_fp8(ops.quantize_fp8(w))


def _llama_linears(core):
    for l in core.model.layers:
        a, m = l.self_attn, l.mlp
        yield from (a.q_proj, a.k_proj, a.v_proj, a.o_proj, m.gate_proj, m.up_proj, m.down_proj)
    yield core.lm_head


def _make_twin_(core):
    """In place: every LLaMA Linear weight and lm_head := dequant(Q(W)) (the bf16 twin)."""
    with torch.no_grad():
        for mod in _llama_linears(core):
            mod.weight.copy_(_twin_weight(mod.weight))
    core._packed = None
    return core


# ---- 1. the quantize kernel ----------------------------------------------------------------------------------------------------
def test_quantize_kernel_edge_rows_equal_torch_cast():
    ops = pkg("ops")
    for K in (64, 4096):
        w = edge_rows(K)
        q = ops.quantize_fp8(w.to(DEV))
        codes, scales = fp8_reference(w)
        assert torch.equal(q.codes.cpu(), codes), f"codes differ from torch's cast (K = {K})"
        assert torch.equal(q.scales.cpu(), scales), f"scales differ (K = {K})"


@pytest.mark.parametrize("N,K", [(4096, 4096), (22016, 4096), (4096, 11008), (32011, 4096)])
def test_quantize_kernel_real_shapes_equal_torch_cast(N, K):
    ops, MC = pkg("ops"), pkg("modeling_core")
    if N == 22016:            # gate|up interleave: quantizing the pack row by row == interleaving the per-Linear codes and scales
        gate, up = _weight(N // 2, K, 1), _weight(N // 2, K, 2)
        w = MC.interleave_gate_up(gate, up)
        qg, qu = ops.quantize_fp8(gate), ops.quantize_fp8(up)
        q = ops.quantize_fp8(w)
        assert torch.equal(q.codes, MC.interleave_gate_up(qg.codes, qu.codes))
        assert torch.equal(q.scales, MC.interleave_gate_up(qg.scales[:, None], qu.scales[:, None]).view(-1))
    else:
        w = _weight(N, K, N + K)
        q = ops.quantize_fp8(w)
    codes, scales = fp8_reference(w.cpu())
    assert torch.equal(q.codes.cpu(), codes)
    assert torch.equal(q.scales.cpu(), scales)


def test_dequantize_kernel_row_major_and_tile_major():
    ops = pkg("ops")
    for N, K in ((1000, 4096), (32011, 4096), (48, 64)):
        q = ops.quantize_fp8(_weight(N, K, 5))
        ref = dequant_reference(q.codes.cpu(), q.scales.cpu())
        assert torch.equal(ops.dequantize_fp8(q).cpu(), ref)
        if K % 64 == 0:
            assert torch.equal(ops.dequantize_fp8(q, tiled=True), ops.tile_major(ref.to(DEV)))


# ---- 2. every fp8 linear path == ops.linear on the dequantized weight -------------------------------------------------------------
def _pair(N, K, seed, register=False):
    ops = pkg("ops")
    w = _weight(N, K, seed)
    q = ops.quantize_fp8(w)
    wd = ops.dequantize_fp8(q).contiguous()
    if register:
        ops.register_tiled(wd)                # what pack_weights does for the twin's weights
    return q, wd


@pytest.mark.parametrize("M", [1, 2, 4])
def test_gemv_forms_equal_twin(M):
    ops = pkg("ops")
    with torch.no_grad():
        for N, K in ((4096, 4096), (1000, 11008), (512, 2048)):        # (the last is below the skinny kernel's size at M = 3, 4)
            q, wd = _pair(N, K, 10 + M)
            x = _rand(M, K, seed=M)
            r = _rand(M, N, seed=7)
            nw = (_rand(K, sc=0.1, seed=3).float() + 1).to(BF)
            assert torch.equal(ops.linear(x, q), ops.linear(x, wd))
            assert torch.equal(ops.linear(x, q, residual=r), ops.linear(x, wd, residual=r))
            assert torch.equal(ops.linear(x, q, out_f32=True), ops.linear(x, wd, out_f32=True))
            if M * K <= 16384:
                assert torch.equal(ops.linear(x, q, rms_w=nw, rms_eps=1e-6), ops.linear(x, wd, rms_w=nw, rms_eps=1e-6))
        # SwiGLU on the interleaved gate|up pack, with and without the fused RMSNorm prologue
        q, wd = _pair(2 * 2048, 4096, 20 + M)
        x = _rand(M, 4096, seed=M + 1)
        nw = (_rand(4096, sc=0.1, seed=4).float() + 1).to(BF)
        assert torch.equal(ops.linear(x, q, swiglu=True), ops.linear(x, wd, swiglu=True))
        assert torch.equal(ops.linear(x, q, swiglu=True, rms_w=nw, rms_eps=1e-6), ops.linear(x, wd, swiglu=True, rms_w=nw, rms_eps=1e-6))


@pytest.mark.parametrize("B,S", [(1, 1), (2, 2), (4, 1)])
def test_qkv_rope_append_equal_twin(B, S):
    ops = pkg("ops")
    H, hd, smax, past = 32, 128, 256, 37
    D = H * hd
    T = B * S
    q8, wd = _pair(3 * D, D, 30 + T)
    x = _rand(T, D, seed=T)
    nw = (_rand(D, sc=0.1, seed=9).float() + 1).to(BF)
    pos = torch.arange(past, past + S, device=DEV).repeat(B)
    inv = (1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))).to(DEV)
    cs, sn = ops.rope_table(pos, inv, BF)
    outs = []
    with torch.no_grad():
        for w in (q8, wd):
            kc = torch.zeros(B, H, smax, hd, device=DEV, dtype=BF)
            vt = torch.zeros(B, H, hd, smax, device=DEV, dtype=BF)
            qo = ops.linear_qkv_rope_append(x, w, cs, sn, B, S, H, hd, kc, vt, smax, past, rms_w=nw, rms_eps=1e-6)
            outs.append((qo, kc, vt))
    (qa, ka, va), (qb, kb, vb) = outs
    assert torch.equal(qa, qb), "query output"
    assert torch.equal(ka, kb), "K cache rows"
    assert torch.equal(va, vb), "V^T cache columns"
    assert bool(ka[:, :, past:past + S].abs().sum() > 0)


@pytest.mark.parametrize("M", [3, 8, 16])
def test_skinny_equal_twin(M):
    ops = pkg("ops")
    with torch.no_grad():
        q, wd = _pair(4096, 4096, 40 + M)
        x = _rand(M, 4096, seed=M)
        r = _rand(M, 4096, seed=M + 2)
        assert torch.equal(ops.linear(x, q), ops.linear(x, wd))
        assert torch.equal(ops.linear(x, q, residual=r), ops.linear(x, wd, residual=r))
        q, wd = _pair(2 * 11008, 4096, 50 + M)
        assert torch.equal(ops.linear(x, q, swiglu=True), ops.linear(x, wd, swiglu=True))
        q, wd = _pair(4096, 11008, 60 + M)
        xa = _rand(M, 11008, seed=M + 3)
        assert torch.equal(ops.linear(xa, q, residual=r), ops.linear(xa, wd, residual=r))


@pytest.mark.parametrize("M", [323, 1024, 1286])
def test_prefill_equal_twin(M):
    """M = 323: the 128 x 128 kernel on the row-major dequantized weight; M >= 1024: the 256 x 256 kernel on the tile-major copy with the
    stream-K tail (K = 4096 >= the split threshold); lm_head's N = 32011 among the shapes."""
    ops = pkg("ops")
    with torch.no_grad():
        for N, K, kw in ((4096, 4096, dict(residual=True)), (32011, 4096, {}), (2 * 11008, 4096, dict(swiglu=True)), (4096, 11008, {})):
            q, wd = _pair(N, K, N + M, register=True)
            x = _rand(M, K, seed=M)
            args = {}
            if kw.get("residual"):
                args["residual"] = _rand(M, N, seed=M + 1)
            if kw.get("swiglu"):
                args["swiglu"] = True
            assert torch.equal(ops.linear(x, q, **args), ops.linear(x, wd, **args)), (N, K, kw)
        # the fused q|k|v + RoPE prefill GEMM
        q, wd = _pair(3 * 4096, 4096, 70 + M, register=True)
        x = _rand(M, 4096, seed=M + 5)
        pos = torch.arange(M, device=DEV)
        inv = (1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float) / 128))).to(DEV)
        cs, sn = ops.rope_table(pos, inv, BF)
        assert torch.equal(ops.linear_qkv_rope(x, q, cs, sn, 2 * 4096, 128), ops.linear_qkv_rope(x, wd, cs, sn, 2 * 4096, 128))


# ---- 3. tiny models against their twin ---------------------------------------------------------------------------------------------
def _tiny_core_pair():
    from helpers import core_model_from_fixture
    fx = load_fixture("g1_core_tiny_bf16.pt")
    twin, _ = core_model_from_fixture(fx, DEV)
    _make_twin_(twin)
    fp8, _ = core_model_from_fixture(fx, DEV)
    with torch.no_grad():
        for a, b in zip(_llama_linears(fp8), _llama_linears(twin)):
            a.weight.copy_(b.weight)
    fp8.quantize_weights("fp8_e4m3")
    assert fp8.weight_quantization == "fp8_e4m3" and twin.weight_quantization is None
    return fx, twin, fp8


@pytest.mark.parametrize("per_op", [False, True])
def test_tiny_core_forward_and_generate_equal_twin(per_op):
    ops = pkg("ops")
    fx, twin, fp8 = _tiny_core_pair()
    ids, mask, images = fx["input_ids"].to(DEV), fx["attention_mask"].to(DEV), fx["images"].to(DEV)
    prompt = fx["greedy_prompt"].to(DEV)
    with torch.no_grad(), ops.per_op_layers(per_op):
        outs = [m(input_ids=ids, attention_mask=mask, images=images, output_hidden_states=True) for m in (twin, fp8)]
        assert torch.equal(outs[0].logits, outs[1].logits)
        assert len(outs[0].hidden_states) == len(outs[1].hidden_states)
        for i, (a, b) in enumerate(zip(outs[0].hidden_states, outs[1].hidden_states)):
            assert torch.equal(a, b), f"hidden state {i}"
        for use_cache in (False, True):
            kw = dict(input_ids=prompt, images=images[:1], max_new_tokens=8, do_sample=False, use_cache=use_cache, eos_token_id=-1,
                      output_hidden_states=True, return_dict_in_generate=True)
            a, b = twin.generate(**kw), fp8.generate(**kw)
            assert torch.equal(a.sequences, b.sequences), use_cache
            assert torch.equal(a.hidden_states[-1][-1], b.hidden_states[-1][-1]), use_cache
        # left-padded batch of 2: the fixture's left-padded prompt beside a longer, unpadded one (the greedy prompt + 3 text tokens)
        lp, lm = fx["leftpad_ids"].to(DEV), fx["leftpad_mask"].to(DEV)
        gp = fx["greedy_prompt"].to(DEV)
        ids2 = torch.cat([lp, torch.cat([gp, torch.tensor([[20, 21, 22][:lp.shape[1] - gp.shape[1]]], device=DEV)], dim=1)])
        mask2 = torch.cat([lm, torch.ones_like(lm)])
        img2 = images[:1].expand(2, -1, -1, -1).contiguous()
        for use_cache in (False, True):
            kw = dict(input_ids=ids2, attention_mask=mask2, images=img2, max_new_tokens=6, do_sample=False, use_cache=use_cache, eos_token_id=-1)
            assert torch.equal(twin.generate(**kw), fp8.generate(**kw)), use_cache
        # seeded sampling
        seqs = []
        for m in (twin, fp8):
            torch.manual_seed(1234)
            seqs.append(m.generate(input_ids=ids2, attention_mask=mask2, images=img2, max_new_tokens=8, do_sample=True, temperature=0.2,
                                   top_p=0.9, use_cache=True, eos_token_id=-1))
        assert torch.equal(seqs[0], seqs[1])


def test_tiny_core_quantize_and_generate_under_inference_mode():
    """quantize_weights() called, and the first forward run, under torch.inference_mode() (the reference wraps generation in it)."""
    from helpers import core_model_from_fixture
    fx = load_fixture("g1_core_tiny_bf16.pt")
    twin, _ = core_model_from_fixture(fx, DEV)
    _make_twin_(twin)
    fp8, _ = core_model_from_fixture(fx, DEV)
    with torch.no_grad():
        for a, b in zip(_llama_linears(fp8), _llama_linears(twin)):
            a.weight.copy_(b.weight)
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"][:1].to(DEV)
    kw = dict(input_ids=prompt, images=images, max_new_tokens=8, do_sample=False, use_cache=True, eos_token_id=-1)
    with torch.no_grad():
        ref = twin.generate(**kw)
    with torch.inference_mode():
        fp8.quantize_weights()
        got = fp8.generate(**kw)
        got_nc = fp8.generate(**dict(kw, use_cache=False))
    assert torch.equal(ref, got) and torch.equal(ref, got_nc)


def _tiny_full(fx):
    C, M = pkg("configuration"), pkg("modeling_ullava")
    cfg, cd = fx["cfg"], fx["cfg"]["llm"]
    ucfg = C.UllavaConfig(llm_config=dict(vision_config=cd["vision_config"], vision_hidden_layer=cd["vision_hidden_layer"], projector_type="mlp",
                                          projector_from_scratch=bool(cd.get("projector_from_scratch", False)), mm_token_ids=cd["mm_token_ids"],
                                          vocab_size=cd["vocab_size"], hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"],
                                          num_hidden_layers=cd["num_hidden_layers"], num_attention_heads=cd["num_attention_heads"]),
                          seg_token_idx=cfg["seg_token_idx"], loc_token_idx=cfg["loc_token_idx"], sam_config=dict(cfg["sam"]))
    model = M.UllavaForCausalLM(ucfg, device=DEV)
    model.load_state_dict(fixture_sd(fx, BF), strict=True)
    return model


@pytest.mark.parametrize("temperature", [0, 0.2])
def test_tiny_evaluate_equal_twin(temperature):
    fx = load_fixture("g8_full_tiny_bf16.pt")
    twin, fp8 = _tiny_full(fx), _tiny_full(fx)
    _make_twin_(twin.llm)
    with torch.no_grad():
        for a, b in zip(_llama_linears(fp8.llm), _llama_linears(twin.llm)):
            a.weight.copy_(b.weight)
    assert fp8.quantize_weights() is fp8 and fp8.weight_quantization == "fp8_e4m3"
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    res = []
    for m in (twin, fp8):
        torch.manual_seed(77)
        res.append(m.evaluate(*args, max_new_tokens=6, temperature=temperature, top_p=0.9 if temperature else None))
    (sa, ma, ba), (sb, mb, bb) = res
    assert torch.equal(sa, sb)
    assert len(ma) == len(mb) and all(torch.equal(x, y) for x, y in zip(ma, mb))
    assert len(ba) == len(bb) and all(torch.equal(x, y) for x, y in zip(ba, bb))


# ---- 4. full width and depth (LLaMA-7B, random init) -----------------------------------------------------------------------------
def test_full_depth_c1_prefill_and_decode_equal_twin_and_memory():
    import bench
    ops = pkg("ops")
    model, cfg = bench.build_model(336, DEV, seed=3)
    _make_twin_(model)
    vis, ids, mask = bench.make_inputs(cfg, 1, 64, DEV, 0)
    vis4, ids4, _ = bench.make_inputs(cfg, 4, 64, DEV, 1)

    def run(m):
        with torch.no_grad():
            out = m.forward(input_ids=ids, attention_mask=mask, images=vis, output_hidden_states=True)
            g1 = m.generate(input_ids=ids, images=vis, max_new_tokens=16, do_sample=False, use_cache=True, eos_token_id=-1,
                            output_hidden_states=True, return_dict_in_generate=True)
            g4 = m.generate(input_ids=ids4, images=vis4, max_new_tokens=16, do_sample=False, use_cache=True, eos_token_id=-1,
                            output_hidden_states=True, return_dict_in_generate=True)
        return out.logits, out.hidden_states, g1, g4

    a = run(model)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    P = sum(mod.weight.numel() for mod in _llama_linears(model))
    assert P > 6.4e9
    with torch.no_grad():
        model.quantize_weights()
    b = run(model)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(DEV)
    print(f"memory allocated: {before / 2**30:.2f} GiB before, {after / 2**30:.2f} GiB after quantize_weights (P = {P / 1e9:.2f} G weights)")
    assert torch.equal(a[0], b[0]), "prefill logits"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"prefill hidden state {i}"
    for ga, gb, what in ((a[2], b[2], "batch 1 (GEMV)"), (a[3], b[3], "batch 4 (skinny)")):
        assert torch.equal(ga.sequences, gb.sequences), what
        assert torch.equal(ga.hidden_states[-1][-1], gb.hidden_states[-1][-1]), what
    assert before - after >= 2 * P, (before, after, P)
    assert ops.coarse_ok()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_quantized_model_refuses_training_lora_save_and_cast(tmp_path):
    fx, twin, fp8 = _tiny_core_pair()
    ids, mask, images = fx["input_ids"].to(DEV), fx["attention_mask"].to(DEV), fx["images"].to(DEV)
    fp8.model.norm.weight.requires_grad_(True)                  # a trainable LLaMA parameter: forward(labels=...) would build a graph
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="fp8_e4m3"):
        fp8.forward(input_ids=ids, attention_mask=mask, images=images, labels=ids)
    fp8.model.norm.weight.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        fp8.add_lora(r=4)
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        fp8.save_pretrained(str(tmp_path / "ckpt"))
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        fp8.state_dict()
    with pytest.raises(NotImplementedError, match="fp8_e4m3"):
        fp8.to(torch.float16)
    assert fp8.dtype == BF and not os.path.exists(tmp_path / "ckpt" / "config.json")
    # a no-op move is allowed, and the model still equals its twin afterwards
    fp8.to(DEV)
    with torch.no_grad():
        assert torch.equal(fp8(input_ids=ids, attention_mask=mask, images=images).logits, twin(input_ids=ids, attention_mask=mask, images=images).logits)


@pytest.mark.parametrize("fmt", ["fp8", "bf16"])
def test_coarse_decode_entry_validates_shapes_without_launching(fmt):
    """The coarse decode entry checks every layer (fp8 and bf16 weights) before the first launch: an inconsistent layer or intermediate
    size is refused with the output untouched."""
    L, ops = pkg("_lib"), pkg("ops")
    w8 = fmt == "fp8"
    H, hd, I, T = 4, 16, 128, 1
    D = H * hd
    ws = {n: _weight(r, c, i) for i, (n, r, c) in enumerate((("qkv", 3 * D, D), ("o", D, D), ("gu", 2 * I, D), ("down", D, I)))}
    q = {n: ops.quantize_fp8(w) for n, w in ws.items()} if w8 else ws
    Layer = L.LlamaLayer
    ln = torch.ones(D, device=DEV, dtype=BF)

    def lin(w, n=None):
        if w8:
            return L.Linear(w.codes.data_ptr(), None, None, n or w.shape[0], w.shape[1], w.codes.stride(0), L.WF_FP8, w.scales.data_ptr(), 0)
        return L.Linear(w.data_ptr(), None, None, n or w.shape[0], w.shape[1], w.stride(0))

    def call(layer, I_):
        x = torch.zeros(T, D, device=DEV, dtype=BF)
        out = torch.full((T, D), 7.0, device=DEV, dtype=BF)
        x_mid, xn, qb, att, act = (torch.zeros(T, n, device=DEV, dtype=BF) for n in (D, max(D, I), D, D, I))
        kc = torch.zeros(1, H, 64, hd, device=DEV, dtype=BF)
        vt = torch.zeros(1, H, hd, 64, device=DEV, dtype=BF)
        cs = torch.ones(T, hd // 2, device=DEV, dtype=BF)
        arr = (Layer * 1)(layer)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        ptrs = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
        fn = L.load().ull_llama_decode_layers_bf16
        rc = fn(arr, 1, p(x), ptrs(out), p(x_mid), p(xn), p(qb), p(att), p(act), p(cs), p(cs), None, ptrs(kc), ptrs(vt),
                1, 1, H, hd, I_, 64, 5, 1e-6, ops._zeros(DEV).data_ptr(), ops._stream())
        torch.cuda.synchronize()
        return rc, out

    good = Layer(ln.data_ptr(), ln.data_ptr(), lin(q["qkv"]), lin(q["o"]), lin(q["gu"]), lin(q["down"]))
    rc, out = call(good, I)
    assert rc == 0 and not bool((out == 7.0).all())
    bad_gu = Layer(ln.data_ptr(), ln.data_ptr(), lin(q["qkv"]), lin(q["o"]), lin(q["gu"], n=2 * I - 32), lin(q["down"]))
    rc, out = call(bad_gu, I)
    assert rc in (-1, -2) and bool((out == 7.0).all()), "inconsistent gu.n must be refused before any launch"
    rc, out = call(good, I - 3)
    assert rc in (-1, -2) and bool((out == 7.0).all()), "an odd intermediate size must be refused before any launch"
