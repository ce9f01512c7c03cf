"""GPU: the FP8 (e4m3) KV cache (KVCache(kv_dtype="fp8_e4m3"), generate(kv_cache_dtype=...)).

The contract is bit-identity with the TWIN: the same model with a bf16 KVCache whose positions < past hold dequant(Q(.)) of the fp8 cache
(`KVCache.dequantized()`).  An attention reads the K / V of its own forward call at full bf16 precision and the earlier positions
dequantized, and the fp8 decode attention feeds its MFMAs exactly the bf16 operands the bf16 kernel reads from the twin -- so every
comparison below is torch.equal.
"""
import os
import sys

import pytest
import torch

from helpers import core_model_from_fixture, load_fixture, pkg
from test_fp8_weights_cpu import dequant_reference, edge_rows, fp8_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rand(*shape, sc=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * sc).to(BF)


def _slots(n):
    """V^T slot of every key 0 .. n - 1 (KVCache.vt_slot)."""
    MC = pkg("modeling_core")
    return torch.tensor([MC.KVCache.vt_slot(p) for p in range(n)], device=DEV)


def _cache(B, H, hd, smax, n_layers=1):
    return pkg("modeling_core").KVCache(n_layers, B, H, hd, smax, DEV, kv_dtype="fp8_e4m3")


# ---- 1, 2. quantize into / dequantize out of the cache ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 32])
def test_quantize_and_dequantize_equal_torch(B):
    ops = pkg("ops")
    H, hd, S = (1, 128, 21) if B == 1 else (32, 128, 70)
    if B == 1:                                   # the edge vectors as K rows and as V columns (reversed, so the two differ)
        k = edge_rows(hd).to(DEV)[:S].view(1, 1, -1, hd)
        S = k.shape[2]
        v = k.flip(2).contiguous()
    else:
        k = (_rand(B, H, S, hd, seed=1).float() * torch.logspace(-3, 3, S, device=DEV)[None, None, :, None]).to(BF)
        v = _rand(B, H, S, hd, seed=2)
        v[0, 0, 3] = 0                           # an all-zero vector: scale 1
    c = _cache(B, H, hd, S + 40)
    p0 = 5
    ops.quantize_kv(k, k.stride()[:3], v, v.stride()[:3], *c.kv8_layer(0), p0, S)
    kc, ks = fp8_reference(k.reshape(-1, hd).cpu())
    vc, vs = fp8_reference(v.reshape(-1, hd).cpu())
    sl = _slots(p0 + S)[p0:]
    assert torch.equal(c.k8[0][:, :, p0:p0 + S].reshape(-1, hd).cpu(), kc)
    assert torch.equal(c.k_scale[0][:, :, p0:p0 + S].reshape(-1).cpu(), ks)
    assert torch.equal(c.vt8[0][..., sl].transpose(-1, -2).reshape(-1, hd).cpu(), vc)
    assert torch.equal(c.vt_scale[0][..., sl].reshape(-1).cpu(), vs)
    # dequantize: float(code) * 2^s at positions < n, zero V^T columns for keys >= n
    n = p0 + S
    ko = torch.full((B, H, n + 3, hd), 7.0, device=DEV, dtype=BF)
    vo = torch.full((B, H, hd, c.smax), 7.0, device=DEV, dtype=BF)
    ops.dequantize_kv(*c.kv8_layer(0), n, k_out=ko, vt_out=vo)
    assert torch.equal(ko[:, :, p0:n].reshape(-1, hd).cpu(), dequant_reference(kc, ks))
    assert torch.equal(vo[..., sl].transpose(-1, -2).reshape(-1, hd).cpu(), dequant_reference(vc, vs))
    assert torch.equal(ko[:, :, :p0].float().abs().sum().cpu(), torch.tensor(0.0))            # never written: zero codes
    nv = -(-n // 64) * 64
    tail = torch.ones(nv, dtype=torch.bool, device=DEV)
    tail[_slots(n)] = False
    assert not vo[..., :nv][..., tail].any()
    assert torch.equal(ko[:, :, n:], torch.full_like(ko[:, :, n:], 7.0)) and (vo[..., nv:] == 7.0).all()


# ---- 3. the fp8 decode attention against the bf16 attention on the twin -------------------------------------------------------------
# (<= 64 keys take the bf16 path's single-tile kernel: the model routes such calls through the dequantized scratch, not this kernel)
@pytest.mark.parametrize("Sq,past", [(sq, p) for sq in (1, 2, 4, 16) for p in (1, 31, 63, 64, 700, 1023, 2040) if sq + p > 64])
@pytest.mark.parametrize("B,masked", [(1, False), (4, True)])
def test_decode_attention_equals_twin(Sq, past, B, masked):
    ops = pkg("ops")
    H, hd = (32, 128) if B == 1 else (8, 128)
    Sk = past + Sq
    smax = -(-(Sk + 5) // 64) * 64
    D = H * hd
    kf = (_rand(B, H, Sk, hd, seed=past).float() * torch.logspace(-2, 1, Sk, device=DEV)[None, None, :, None]).to(BF)
    vf = _rand(B, H, Sk, hd, seed=past + 1)
    q = _rand(B * Sq, D, seed=past + 2)
    mask = None
    if masked:
        mask = torch.ones(B, Sk, device=DEV, dtype=torch.int32)
        mask[1, :past // 2] = 0
        mask[3, 1:past:3] = 0
    c = _cache(B, H, hd, smax)
    ops.quantize_kv(kf, kf.stride()[:3], vf, vf.stride()[:3], *c.kv8_layer(0), 0, past)
    w0 = past & ~63
    sl = _slots(Sk)
    c.k_stage[:, :, past - w0:Sk - w0] = kf[:, :, past:]
    c.vt_stage[..., sl[past:] - w0] = vf[:, :, past:].transpose(-1, -2)
    kt = torch.zeros(B, H, smax, hd, device=DEV, dtype=BF)
    vt = torch.zeros(B, H, hd, smax, device=DEV, dtype=BF)
    ops.dequantize_kv(*c.kv8_layer(0), past, k_out=kt, vt_out=vt)
    kt[:, :, past:Sk] = kf[:, :, past:]
    vt[..., sl[past:]] = vf[:, :, past:].transpose(-1, -2)
    ref = torch.empty(B * Sq, D, device=DEV, dtype=BF)
    ops.attention(q, kt, vt, ref, B, H, Sq, Sk, hd, (Sq * D, hd, D), (H * smax * hd, smax * hd, hd), (Sq * D, hd, D), mask, causal=True,
                  scale_mode=1, scale=hd ** -0.5)
    got = torch.empty_like(ref)
    ops.attention_kv8(q, (Sq * D, hd, D), c.k_stage, c.vt_stage, *c.kv8_layer(0), got, (Sq * D, hd, D), B, H, Sq, Sk, hd, mask, hd ** -0.5)
    assert torch.equal(got, ref)
    # the new keys' codes and scales = Q(staging)
    kc, ks = fp8_reference(kf[:, :, past:].reshape(-1, hd).cpu())
    vc, vs = fp8_reference(vf[:, :, past:].reshape(-1, hd).cpu())
    assert torch.equal(c.k8[0][:, :, past:Sk].reshape(-1, hd).cpu(), kc)
    assert torch.equal(c.k_scale[0][:, :, past:Sk].reshape(-1).cpu(), ks)
    assert torch.equal(c.vt8[0][..., sl[past:]].transpose(-1, -2).reshape(-1, hd).cpu(), vc)
    assert torch.equal(c.vt_scale[0][..., sl[past:]].reshape(-1).cpu(), vs)


def test_decode_attention_entry_rejects_bad_shapes():
    ops, lib = pkg("ops"), pkg("_lib")
    B, H, hd, Sq = 1, 2, 128, 1
    c = _cache(B, H, hd, 128)
    q = _rand(Sq, H * hd)
    o = torch.empty_like(q)
    k8, vt8, ks, vs = c.kv8_layer(0)
    base = [q.data_ptr(), Sq * H * hd, hd, H * hd, c.k_stage.data_ptr(), c.vt_stage.data_ptr(), k8.data_ptr(), vt8.data_ptr(), ks.data_ptr(),
            vs.data_ptr(), c.smax, o.data_ptr(), Sq * H * hd, hd, H * hd, None, B, H, Sq, 100, hd, 0.1, ops._zeros(DEV).data_ptr(),
            torch.cuda.current_stream().cuda_stream]
    assert lib.query("ull_attention_kv8_bf16", *base) == 0
    for i, bad in ((19, 64), (19, 129), (18, 17), (18, 0), (20, 136), (10, 100), (6, None)):
        args = list(base)
        args[i] = bad
        assert lib.query("ull_attention_kv8_bf16", *args) != 0, (i, bad)
    torch.cuda.synchronize()


# ---- 5, 6. tiny models step by step against the twin -------------------------------------------------------------------------------
def _tiny(fp8_weights=False):
    fx = load_fixture("g1_core_tiny_bf16.pt")
    m, _ = core_model_from_fixture(fx, DEV)
    if fp8_weights:
        m.quantize_weights("fp8_e4m3")
    return fx, m


def _step_twin(m, seq, mask, n_steps, tokens_per_step=1, smax=None, images=None, sample=None, hidden=None):
    """Greedy decoding with an fp8 cache where every forward is checked against the twin (the same model on c8.dequantized()).
    Returns the ids.  tokens_per_step > 1: continuation calls of that many (greedy-repeated) tokens.  sample = (temperature, top_p): draw
    each token from the twin's logits as generate() does (one torch.multinomial per step).  hidden: a list that receives the twin's
    last-layer hidden states of every call."""
    MC = pkg("modeling_core")
    cfg = m.config
    B = seq.shape[0]
    H, hd = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    smax = smax or seq.shape[1] + n_steps * tokens_per_step + 64
    c8 = MC.KVCache(cfg.num_hidden_layers, B, H, hd, smax, DEV, kv_dtype="fp8_e4m3")
    for step in range(n_steps + 1):
        m8 = None if mask is None else torch.cat([mask, mask.new_ones(B, seq.shape[1] - mask.shape[1])], dim=1)
        tw = c8.dequantized() if c8 else MC.KVCache(cfg.num_hidden_layers, B, H, hd, smax, DEV)
        outs = []
        for cache in (tw, c8):
            inp = m.prepare_inputs_for_generation(input_ids=seq, attention_mask=m8, images=images if step == 0 else None,
                                                  past_key_values=cache, use_cache=True)
            if cache and tokens_per_step > 1:
                inp["input_ids"] = seq[:, -tokens_per_step:]
                if inp["position_ids"] is not None:
                    inp["position_ids"] = (m8.long().cumsum(-1) - 1)[:, -tokens_per_step:]
            outs.append(m(**inp, output_hidden_states=True))
        a, b = outs
        assert torch.equal(a.logits, b.logits), f"step {step}: logits"
        for i, (x, y) in enumerate(zip(a.hidden_states, b.hidden_states)):
            assert torch.equal(x, y), f"step {step}: hidden state {i}"
        assert torch.equal(tw.last_hidden[-1], c8.last_hidden[-1])
        assert c8.length == tw.length
        if hidden is not None:
            hidden.append(a.hidden_states[-1])
        if step == n_steps:
            break
        if sample is not None:
            nxt = torch.multinomial(MC.sampling_probs(a.logits[:, -1].float(), sample[0], 50, sample[1]), 1)
        else:
            nxt = a.logits[:, -1].argmax(-1, keepdim=True)
        if tokens_per_step > 1:
            nxt = nxt.remainder(90)                  # a multi-token call must not carry an unmatched multimodal id
        seq = torch.cat([seq] + [nxt] * tokens_per_step, dim=1)
    return seq


def _long_ids(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 90, (B, L), generator=g).to(DEV)             # (text ids: below the fixture's multimodal ids 90 .. 95)


@pytest.mark.parametrize("fp8_weights", [False, True])
def test_tiny_prefill_and_decode_equal_twin(fp8_weights):
    fx, m = _tiny(fp8_weights)
    with torch.no_grad():
        # image prompt (< 64 positions: the scratch route), then a text prompt that crosses the 64- and 128-key tiles (fp8 decode attention)
        _step_twin(m, fx["greedy_prompt"].to(DEV), None, 6, images=fx["images"][:1].to(DEV))
        _step_twin(m, _long_ids(1, 58, 1), None, 80)
        # T = B * S > 4: the unfused decode route; left-padded batch with a key mask
        ids = _long_ids(6, 70, 2)
        mask = torch.ones_like(ids)
        mask[1, :9] = 0
        mask[4, :33] = 0
        _step_twin(m, ids, mask, 5)
        # continuations: 3 tokens per call at batch 2 (T = 6), 20 tokens per call (> 16: dequantize + bf16 path + quantize)
        _step_twin(m, _long_ids(2, 61, 3), None, 4, tokens_per_step=3)
        _step_twin(m, _long_ids(1, 70, 4), None, 3, tokens_per_step=20)


@pytest.mark.parametrize("fp8_weights", [False, True])
def test_tiny_generate_greedy_and_sampling_use_the_fp8_cache(fp8_weights):
    fx, m = _tiny(fp8_weights)
    ids = _long_ids(1, 60, 5)
    lp = torch.cat([torch.zeros(1, 7, dtype=torch.long, device=DEV), _long_ids(1, 60, 6)], dim=1)
    ids2 = torch.cat([lp, _long_ids(1, 67, 7)])
    mask2 = torch.ones_like(ids2)
    mask2[0, :7] = 0
    with torch.no_grad():
        for seq, mask in ((ids, None), (ids2, mask2)):
            want = _step_twin(m, seq, mask, 12)
            got = m.generate(input_ids=seq, attention_mask=mask, max_new_tokens=12, do_sample=False, use_cache=True, eos_token_id=-1,
                             kv_cache_dtype="fp8_e4m3")
            assert torch.equal(got, want)
            ref = m.generate(input_ids=seq, attention_mask=mask, max_new_tokens=12, do_sample=False, use_cache=True, eos_token_id=-1)
            assert got.shape == ref.shape
        # seeded sampling: generate() with the fp8 cache draws the tokens the twin's logits give with the same seed
        torch.manual_seed(1234)
        want = _step_twin(m, ids2, mask2, 8, sample=(0.7, 0.9))
        torch.manual_seed(1234)
        got = m.generate(input_ids=ids2, attention_mask=mask2, max_new_tokens=8, do_sample=True, temperature=0.7, top_p=0.9, use_cache=True,
                         eos_token_id=-1, kv_cache_dtype="fp8_e4m3")
        assert torch.equal(got, want)
        MC = pkg("modeling_core")
        cfg = m.config
        c8 = MC.KVCache(cfg.num_hidden_layers, 1, cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads, 128, DEV,
                        kv_dtype="fp8_e4m3")
        out = m(input_ids=ids, past_key_values=c8, use_cache=True)
        assert out.past_key_values is c8 and c8.length == ids.shape[1]
        tw = MC.KVCache(cfg.num_hidden_layers, 1, cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads, 128, DEV)
        assert torch.equal(m(input_ids=ids, past_key_values=tw, use_cache=True).logits, out.logits)      # 6. prefill == bf16-cache prefill


def test_tiny_evaluate_with_fp8_cache_equals_twin():
    """evaluate(kv_cache_dtype=...): ids, masks and boxes equal what evaluate computes from the twin's decoding (ids and last-layer hidden
    states of the twin loop, then evaluate's own [SEG] / [LOC] heads)."""
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    images, ids0 = fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV)
    raw, resize = [fx["size_list"][0]], [fx["resize_list"][0]]
    with torch.no_grad():
        ids, masks, boxes = model.evaluate(images_sam, images, ids0, raw, resize, max_new_tokens=6, temperature=0, kv_cache_dtype="fp8_e4m3")
        hid = []
        want = _step_twin(model.llm, ids0, None, 6, images=images, hidden=hid)
        assert torch.equal(ids, want[:, :ids.shape[1]])
        last = torch.cat(hid, dim=1)[:, :ids.shape[1] - 1]
        L1 = last.shape[1]
        pe = model._select(last, (ids[:, 1:] == model.config.seg_token_idx)[:, :L1], model.seg_projector)
        pl = model._select(last, (ids[:, 1:] == model.config.loc_token_idx)[:, :L1], model.det_projector)
        masks_w = model._decode(model._visual_embs_tm(images_sam), pe, resize, raw)
        boxes_w = [model._run_mlp(model.det_decoder, e) if e.shape[0] else e.new_empty(0, 4) for e in pl]
    assert len(masks) == len(masks_w) and all(torch.equal(x, y) for x, y in zip(masks, masks_w))
    assert len(boxes) == len(boxes_w) and all(torch.equal(x, y) for x, y in zip(boxes, boxes_w))
    with pytest.raises(ValueError):
        model.evaluate(images_sam, images, ids0, raw, resize, max_new_tokens=2, temperature=0, kv_cache_dtype="fp8")


# ---- 7. HF views ---------------------------------------------------------------------------------------------------------------------
def test_from_hf_and_legacy_views_equal_dequant():
    MC = pkg("modeling_core")
    B, H, S, hd = 2, 4, 77, 64
    past = [(_rand(B, H, S, hd, seed=10 + i), _rand(B, H, S, hd, sc=3.0, seed=20 + i)) for i in range(3)]
    c = MC.KVCache.from_hf(past, headroom=16, kv_dtype="fp8_e4m3")
    assert c.kv_dtype == "fp8_e4m3" and c.length == S and len(c) == 3
    legacy = c.to_legacy_cache()
    for li, ((k, v), (k2, v2)) in enumerate(zip(past, legacy)):
        for x, y in ((k, k2), (v, v2)):
            codes, scales = fp8_reference(x.reshape(-1, hd).cpu())
            assert torch.equal(y.reshape(-1, hd).cpu(), dequant_reference(codes, scales)), li
        gk, gv = c[li]
        assert torch.equal(gk, k2) and torch.equal(gv, v2)
    tw = c.dequantized()
    assert tw.kv_dtype is None and tw.length == S
    for (a, b), (x, y) in zip(tw.to_legacy_cache(), legacy):
        assert torch.equal(a, x) and torch.equal(b, y)


# ---- 8. full width and depth (LLaMA-7B, random init) -----------------------------------------------------------------------------
def test_full_depth_decode_equals_twin_and_memory():
    """LLaMA-7B (random init): an fp8 cache filled by a forward prefill holds <= 0.53x the bytes of the bf16 cache the same prefill makes --
    every device byte the cache keeps, checked against the allocator too -- and a few decode steps equal the twin at batch 1 and 4."""
    import bench
    MC = pkg("modeling_core")
    model, cfg = bench.build_model(336, DEV, seed=3)
    for B in (1, 4):
        vis, ids, _ = bench.make_inputs(cfg, B, 64, DEV, B)
        with torch.no_grad():
            bf = model(input_ids=ids, images=vis, use_cache=True).past_key_values
            S = bf.length
            c8 = MC.KVCache(len(bf), B, 32, 128, bf.smax, DEV, kv_dtype="fp8_e4m3")
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated(DEV)
            pf = model(input_ids=ids, images=vis, past_key_values=c8, use_cache=True)
            del pf
            torch.cuda.synchronize()
            grown = torch.cuda.memory_allocated(DEV) - before
            hidden = sum(t.numel() * t.element_size() for t in c8.last_hidden)
            assert grown <= hidden + (1 << 20), ("the prefill left device memory behind", grown, hidden)
            assert c8.length == S and c8.nbytes() <= 0.53 * bf.nbytes(), (c8.nbytes(), bf.nbytes())
            del bf
            tok = ids[:, -1:]
            for step in range(3):
                tw = c8.dequantized()
                a = model(input_ids=tok, past_key_values=tw, use_cache=True, output_hidden_states=True)
                b = model(input_ids=tok, past_key_values=c8, use_cache=True, output_hidden_states=True)
                assert torch.equal(a.logits, b.logits), (B, step)
                assert torch.equal(a.hidden_states[-1], b.hidden_states[-1]), (B, step)
                assert c8.length == S + step + 1
                tok = b.logits[:, -1].argmax(-1, keepdim=True)
                del tw, a, b
            torch.cuda.synchronize()
            assert torch.cuda.memory_allocated(DEV) - before <= sum(t.numel() * t.element_size() for t in c8.last_hidden) + (1 << 20)


# ---- 4. the coarse fp8-cache decode entries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8_weights", [False, True])
def test_coarse_kv8_decode_equals_per_op(fp8_weights, monkeypatch):
    """T <= 4 decode steps over an fp8 cache through ull_llama_decode_layers[_w8]_kv8_bf16 (one C call per step) equal the per-op path bit
    for bit: logits, hidden states and the codes / scales stored."""
    ops, MC = pkg("ops"), pkg("modeling_core")
    fx, m = _tiny(fp8_weights)
    cfg = m.config
    H, hd = cfg.num_attention_heads, cfg.hidden_size // cfg.num_attention_heads
    calls = []
    real = ops.llama_decode_layers
    monkeypatch.setattr(ops, "llama_decode_layers", lambda *a, **k: (calls.append(k.get("kv8") is not None), real(*a, **k))[1])
    for B in (1, 4):
        ids = _long_ids(B, 63, 10 + B)
        runs = []
        for per_op in (False, True):
            c8 = MC.KVCache(cfg.num_hidden_layers, B, H, hd, 128, DEV, kv_dtype="fp8_e4m3")
            outs, seq = [], ids
            with torch.no_grad(), ops.per_op_layers(per_op):
                for step in range(6):                    # past 63 .. 68: the first step has 64 keys (per-op scratch route), then the entry
                    inp = seq if step == 0 else seq[:, -1:]
                    o = m(input_ids=inp, past_key_values=c8, use_cache=True, output_hidden_states=True)
                    outs.append(o)
                    seq = torch.cat([seq, o.logits[:, -1].argmax(-1, keepdim=True)], dim=1)
            runs.append((outs, c8))
        (oa, ca), (ob, cb) = runs
        for a, b in zip(oa, ob):
            assert torch.equal(a.logits, b.logits)
            assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states))
        for t in ("k8", "vt8", "k_scale", "vt_scale"):
            assert all(torch.equal(x, y) for x, y in zip(getattr(ca, t), getattr(cb, t))), t
    assert calls.count(True) == 2 * 4, calls             # steps 2 .. 5 (65 .. 68 keys) of the coarse runs at both batch sizes


@pytest.mark.parametrize("fmt", ["bf16", "fp8"])
def test_coarse_kv8_decode_entry_validates_without_launching(fmt):
    """The fp8-cache decode entry checks every layer (bf16 and fp8 weights), the cache pointers and the shapes ull_attention_kv8 takes before
    the first launch."""
    import ctypes
    L, ops = pkg("_lib"), pkg("ops")
    w8 = fmt == "fp8"
    H, hd, I, T = 4, 16, 128, 1
    D = H * hd
    ws = {n: _rand(r, c, sc=0.02, seed=i) for i, (n, r, c) in enumerate((("qkv", 3 * D, D), ("o", D, D), ("gu", 2 * I, D), ("down", D, I)))}
    q = {n: ops.quantize_fp8(w) for n, w in ws.items()} if w8 else ws
    Layer = L.LlamaLayer
    ln = torch.ones(D, device=DEV, dtype=BF)

    def lin(w, n=None):
        if w8:
            return L.Linear(w.codes.data_ptr(), None, None, n or w.shape[0], w.shape[1], w.codes.stride(0), L.WF_FP8, w.scales.data_ptr(), 0)
        return L.Linear(w.data_ptr(), None, None, n or w.shape[0], w.shape[1], w.stride(0))

    def call(layer, I_=I, past=70, stage=True, k8_null=False):
        x = torch.zeros(T, D, device=DEV, dtype=BF)
        out = torch.full((T, D), 7.0, device=DEV, dtype=BF)
        x_mid, xn, qb, att, act = (torch.zeros(T, n, device=DEV, dtype=BF) for n in (D, max(D, I), D, D, I))
        c = _cache(1, H, hd, 128)
        cs = torch.ones(T, hd // 2, device=DEV, dtype=BF)
        arr = (Layer * 1)(layer)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        ptrs = lambda t: (ctypes.c_void_p * 1)(None if t is None else t.data_ptr())
        fn = L.load().ull_llama_decode_layers_kv8_bf16
        rc = fn(arr, 1, p(x), ptrs(out), p(x_mid), p(xn), p(qb), p(att), p(act), p(cs), p(cs), None, ptrs(None if k8_null else c.k8[0]),
                ptrs(c.vt8[0]), ptrs(c.k_scale[0]), ptrs(c.vt_scale[0]), p(c.k_stage) if stage else None, p(c.vt_stage), 1, 1, H, hd, I_, 128, past,
                1e-6, ops._zeros(DEV).data_ptr(), ops._stream())
        torch.cuda.synchronize()
        return rc, out, c

    good = Layer(ln.data_ptr(), ln.data_ptr(), lin(q["qkv"]), lin(q["o"]), lin(q["gu"]), lin(q["down"]))
    rc, out, c = call(good)
    assert rc == 0 and not bool((out == 7.0).all()) and bool(c.k_scale[0][0, :, 70].ne(0).all())
    bad_gu = Layer(ln.data_ptr(), ln.data_ptr(), lin(q["qkv"]), lin(q["o"]), lin(q["gu"], n=2 * I - 32), lin(q["down"]))
    for kw in (dict(layer=bad_gu), dict(layer=good, I_=I - 3), dict(layer=good, past=40), dict(layer=good, past=128),
               dict(layer=good, stage=False), dict(layer=good, k8_null=True)):
        rc, out, c = call(**kw)
        assert rc in (-1, -2) and bool((out == 7.0).all()) and not bool(c.k_scale[0].any()), f"{kw} must be refused before any launch"


def test_kv8_c_ptrs_follow_a_rebound_layer():
    c = _cache(1, 2, 16, 64, n_layers=2)
    a = c.c_ptrs()
    assert [a[0][i] for i in range(2)] == [t.data_ptr() for t in c.k8]
    c.k8[1] = c.k8[1].clone()
    b = c.c_ptrs()
    assert b[0][1] == c.k8[1].data_ptr() and b[1][0] == c.vt8[0].data_ptr() and b[4] is c.k_stage
