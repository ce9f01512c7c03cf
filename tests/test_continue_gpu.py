"""generate() / evaluate() continuing an earlier call's KV cache (`past_key_values`): the two kernels alone, the continued call against a
hand-written loop over model.forward on a copy of the cache (same kernels, so the same bits), against the one-shot call (the rule of
test_attention_cached_gpu.py::test_continuation_equals_one_shot_prefill), the prefix check, growth and fork, a padded batch, evaluate() and
the plain call.  The models are the g1 `tiny` fixture model and a seeded 2-layer model with head_dim 128, built once per module."""
import pytest
import torch
import torch.nn.functional as F

from helpers import fixture_sd, load_fixture, pkg, rel_err
from oracle import ullava_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
KV8 = "fp8_e4m3"

_MM = dict(IMG_START=90, IMG_END=91, IMG_PATCH=92, VID_START=93, VID_END=94, VID_PATCH=95)
_HD128 = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=100, rms_norm_eps=1e-6,
              rope_theta=10000.0, vision_hidden_layer=-2, projector_type="mlp", mm_token_ids=_MM,
              vision_config=dict(hidden_size=32, num_hidden_layers=3, num_attention_heads=2, intermediate_size=64, image_size=28, patch_size=14,
                                 num_channels=3, layer_norm_eps=1e-5))
_MODELS = {}


def _model(which):
    """("tiny": the g1_core_tiny fixture model, head_dim 16 | "hd128": a seeded 2-layer config with head_dim 128), bf16 -> (model, sd, cfg dict)"""
    if which in _MODELS:
        return _MODELS[which]
    C, M, W = pkg("configuration"), pkg("modeling_core"), pkg("weights")
    if which == "tiny":
        fx = load_fixture("g1_core_tiny_bf16.pt")
        cd = dict(fx["cfg"])
    else:
        cd = dict(_HD128)
    model = M.UllavaCoreForCausalLM(C.UllavaCoreConfig(**cd, projector_from_scratch=False), device=DEV, dtype=BF)
    if which == "tiny":
        sd = fixture_sd(fx, BF)
    else:
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = {k: v.to(BF) for k, v in W.seeded_state_dict(shapes, 4242, torch.float32).items()}
    model.load_state_dict(sd, strict=True)
    _MODELS[which] = (model, sd, cd)
    return _MODELS[which]


def _ids(B, L, seed, hi=90):
    return torch.randint(3, hi, (B, L), generator=torch.Generator().manual_seed(seed)).to(DEV)     # text ids: below the multimodal ids


def _vt_slot(pos):
    w = pos & 31
    return (pos & ~31) + 8 * ((w >> 2) & 3) + 4 * (w >> 4) + (w & 3)


def _buffers(c):
    return (c.k + c.vt) if c.kv_dtype is None else (c.k8 + c.vt8 + c.k_scale + c.vt_scale)


def _clone(c, smax=None, length=None):
    """a copy of cache c made with torch alone (no kernel of this feature): same state, capacity smax (>= the positions kept)."""
    MC = pkg("modeling_core")
    n_layers, B, H, hd, dev, dt = c._geom
    n = c.length if length is None else length
    d = MC.KVCache(n_layers, B, H, hd, c.smax if smax is None else smax, dev, dt, kv_dtype=c.kv_dtype)
    w = min(c.smax, d.smax)
    assert ((n + 31) & ~31) <= w
    names = ("k", "vt") if c.kv_dtype is None else ("k8", "vt8", "k_scale", "vt_scale")
    for name in names:
        for s, t in zip(getattr(c, name), getattr(d, name)):
            if name in ("vt", "vt8"):                                  # V^T images: positions last
                t[..., :w].copy_(s[..., :w])
            else:
                t[:, :, :w].copy_(s[:, :, :w])
    d.length = c.length
    d.last_hidden = list(c.last_hidden)
    d._id_chunks = None if c.ids is None else [(c.ids.clone(), True)]
    d.mask = c.mask
    if n < c.length:
        d.truncate(n)
    return d


def _hand(model, cache, seq, n_new, mask=None, eos=None, pad=None, sample=None):
    """The loop generate() has to equal, written on forward() alone: the ids behind the cache's positions in one call, then one token per
    step; argmax (or ops.sample_step on torch's noise, sample = (temperature, top_k, top_p)); rows that emitted `eos` get `pad`.
    -> (ids [B, L + n_new], logprobs fp32 [B, n_new])"""
    ops = pkg("ops")
    B, L = seq.shape
    buf = torch.zeros(B, L + n_new, dtype=torch.int64, device=DEV)
    buf[:, :L] = seq
    live = torch.ones(B, dtype=torch.int32, device=DEV)
    alive = torch.zeros(1, dtype=torch.int32, device=DEV)
    eos_ids = None if eos is None else torch.tensor([eos], dtype=torch.int64, device=DEV)
    lps = []
    for step in range(n_new):
        cur = L + step
        lo = cache.length if step == 0 else cur - 1
        m = pos = None
        if mask is not None:
            m = torch.cat([mask, mask.new_ones(B, cur - mask.shape[1])], dim=1)
            pos = (m.long().cumsum(-1) - 1).masked_fill(m == 0, 1)[:, lo:cur]
        with torch.no_grad():
            last = model.forward(input_ids=buf[:, lo:cur], attention_mask=m, position_ids=pos, past_key_values=cache, use_cache=True).logits[:, -1]
        before = live.clone()
        if sample is None:
            nxt = last.float().argmax(-1)
            if pad is not None:
                nxt = torch.where(live.bool(), nxt, torch.full_like(nxt, pad))
            buf[:, cur] = nxt
            if eos is not None:
                live = live * (nxt != eos).to(torch.int32)
        else:
            noise = torch.empty(last.shape, dtype=torch.float32, device=DEV).exponential_()
            ops.sample_step(last, noise, sample[0], sample[1], sample[2], live, eos_ids, pad, buf, cur, alive)
        lps.append(ops.token_logprobs(last, buf[:, cur], before))
    return buf, torch.stack(lps, dim=1)


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 1030])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1500])
def test_ids_common_prefix_against_a_loop(R, n):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(1000 * R + n)
    a = torch.randint(0, 1 << 40, (R, n + 7), generator=g)             # pitches n + 7 and n + 3: they differ
    b = torch.zeros(R, n + 3, dtype=torch.int64)
    b[:, :n] = a[:, :n]
    b[:, n:] = -5                                                      # (what lies behind n must not be read as a match or a mismatch)
    want = torch.full((R,), n, dtype=torch.int32)
    for r in range(R):
        kind = r % 4                                                   # none, position 0, position n - 1, somewhere (two mismatches: the first counts)
        if n and kind == 1:
            b[r, 0] += 1; want[r] = 0
        elif n and kind == 2:
            b[r, n - 1] ^= 1 << 35; want[r] = n - 1                    # (a high bit: all 64 bits are compared)
        elif n > 2 and kind == 3:
            m = int(torch.randint(0, n - 1, (1,), generator=g))
            b[r, m] += 1; b[r, n - 1] += 1; want[r] = m
    for r in range(min(R, 8)):                                         # the rule, spelled as a loop, on the rows a loop can afford
        i = 0
        while i < n and int(a[r, i]) == int(b[r, i]):
            i += 1
        assert i == int(want[r])
    got = ops.ids_common_prefix(a.to(DEV)[:, :n], b.to(DEV)[:, :n], n)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)


def _kv8_buffers(nl, B, H, hd, smax, g=None):
    """random codes and power-of-two scales (g) or sentinels: (k8 list, vt8 list, k_scale list, vt_scale list) on the device"""
    out = ([], [], [], [])
    for _ in range(nl):
        for i, shp in enumerate(((B, H, smax, hd), (B, H, hd, smax))):
            out[i].append((torch.randint(0, 256, shp, generator=g, dtype=torch.uint8) if g else torch.full(shp, 0xAB, dtype=torch.uint8)).to(DEV))
        for i in (2, 3):
            sc = torch.ldexp(torch.ones(B, H, smax), torch.randint(-12, 4, (B, H, smax), generator=g)) if g else torch.full((B, H, smax), 123.0)
            out[i].append(sc.to(DEV))
    return out


@pytest.mark.parametrize("hd", [128, 24])
@pytest.mark.parametrize("smax_pair", [(64, 64), (128, 256), (256, 128)])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 64, 65, 200])
def test_kv8_copy_positions_moves_exactly_the_positions_below_n(n, smax_pair, hd):
    ops = pkg("ops")
    s_smax, d_smax = smax_pair
    if n > min(s_smax, d_smax):
        with pytest.raises(ValueError):
            ops.kv8_copy_positions(_kv8_buffers(1, 1, 1, hd, s_smax), _kv8_buffers(1, 1, 1, hd, d_smax), n)
        return
    nl, B, H = 2, 2, 3
    g = torch.Generator().manual_seed(n * 7 + s_smax + hd)
    src, dst = _kv8_buffers(nl, B, H, hd, s_smax, g), _kv8_buffers(nl, B, H, hd, d_smax)
    before = [[t.clone() for t in l] for l in dst]
    ops.kv8_copy_positions(src, dst, n)
    torch.cuda.synchronize()
    keys = torch.arange(n, device=DEV)
    slots = torch.tensor([_vt_slot(p) for p in range(n)], dtype=torch.int64, device=DEV)
    for li in range(nl):
        for a, idx, dim in ((0, keys, 2), (1, slots, 3), (2, keys, 2), (3, slots, 2)):
            s, d, b = src[a][li], dst[a][li], before[a][li]
            raw = lambda t: t if t.dtype == torch.uint8 else t.view(torch.int32)              # raw bytes, NaN-proof
            assert torch.equal(raw(d).index_select(dim, idx), raw(s).index_select(dim, idx)), f"layer {li} array {a}: positions < {n}"
            rest = torch.ones(d.shape[dim], dtype=torch.bool, device=DEV)
            rest[idx] = False
            rest = rest.nonzero().squeeze(-1)
            assert torch.equal(raw(d).index_select(dim, rest), raw(b).index_select(dim, rest)), f"layer {li} array {a}: bytes outside the positions"
        if hd == 128 and n:
            outs = []
            for bufs, smax in ((src, s_smax), (dst, d_smax)):
                k = torch.zeros(B, H, n, hd, device=DEV, dtype=BF)
                vt = torch.zeros(B, H, hd, (n + 63) & ~63, device=DEV, dtype=BF)
                ops.dequantize_kv(bufs[0][li], bufs[1][li], bufs[2][li], bufs[3][li], n, k_out=k, vt_out=vt)
                outs.append((k.view(torch.int16), vt.view(torch.int16)))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), f"layer {li}: dequantized positions"


# ---- 2. same kernels, same bits --------------------------------------------------------------------------------------------------------
_TURN1 = {}


def _turn1(which, P0, kv, n_new=6):
    """generate() for a first turn of P0 prompt ids into an EMPTY cache -> (cache, sequences); made once, handed out as copies"""
    key = (which, P0, kv, n_new)
    if key not in _TURN1:
        model, _, cd = _model(which)
        mm = torch.tensor(sorted(cd["mm_token_ids"].values()), device=DEV)
        for seed in range(60):                                          # a prompt after which the model emits no image / video placeholder id
            c = model.new_kv_cache(1, 64, kv_cache_dtype=kv)
            assert c.length == 0 and not c and c.ids.shape == (1, 0)
            out = model.generate(input_ids=_ids(1, P0, 5 * P0 + 1 + 1000 * seed), max_new_tokens=n_new, eos_token_id=-1, past_key_values=c,
                                 return_dict_in_generate=True)
            if not bool(torch.isin(out.sequences, mm).any()):
                break
        else:
            pytest.fail("every prompt tried leads to a placeholder id")
        assert out.past_key_values is c and out.sequences.shape[1] == P0 + n_new
        assert c.length == P0 + n_new - 1 and torch.equal(c.ids, out.sequences[:, :-1])
        _TURN1[key] = (c, out.sequences)
    c, seq = _TURN1[key]
    return _clone(c, smax=c.smax + 64), seq                           # (room for the hand-written loops, which grow nothing)


_SHAPES = [(P0, u) for P0 in (60, 64, 65) for u in (1, 4, 5, 16, 17, 40)] + [(690, 17), (698, 5), (698, 1)]    # (P + |u| crosses 64; 704 / 705)


@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("P0,u", _SHAPES)
def test_second_turn_equals_the_hand_written_loop(P0, u, kv):
    model = _model("hd128")[0]
    c_gen, seq1 = _turn1("hd128", P0, kv)
    c_hand, _ = _turn1("hd128", P0, kv)
    seq2 = torch.cat([seq1, _ids(1, u, 3 * P0 + u)], dim=1)
    want, want_lp = _hand(model, c_hand, seq2, 6)
    out = model.generate(input_ids=seq2, max_new_tokens=6, eos_token_id=-1, past_key_values=c_gen, return_dict_in_generate=True, output_logprobs=True,
                         output_hidden_states=True)
    assert torch.equal(out.sequences, want), "ids"
    assert torch.equal(out.logprobs, want_lp), "logprobs"
    assert set(out.keys()) == {"sequences", "hidden_states", "logprobs", "past_key_values"} and out.past_key_values is c_gen
    assert c_gen.length == want.shape[1] - 1 and torch.equal(c_gen.ids, want[:, :-1])
    hs = out.hidden_states[-1][-1]
    assert hs.shape[1] == c_gen.length and torch.equal(hs, torch.cat(c_hand.last_hidden, dim=1)), "hidden states of ALL positions"


@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("which,P0,u", [("tiny", 60, 5), ("hd128", 60, 17)])
def test_second_turn_with_the_device_sampler_and_the_host_loop(which, P0, u, kv):
    model = _model(which)[0]
    seq1 = _turn1(which, P0, kv)[1]
    seq2 = torch.cat([seq1, _ids(1, u, 11 * P0 + u)], dim=1)
    kw = dict(input_ids=seq2, max_new_tokens=6, eos_token_id=-1, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, return_dict_in_generate=True,
              output_logprobs=True)
    torch.manual_seed(1234)
    want, want_lp = _hand(model, _turn1(which, P0, kv)[0], seq2, 6, sample=(0.7, 20, 0.9))
    torch.manual_seed(1234)
    dev = model.generate(**kw, sampler="device", past_key_values=_turn1(which, P0, kv)[0])
    assert torch.equal(dev.sequences, want) and torch.equal(dev.logprobs, want_lp)
    torch.manual_seed(1234)
    host = model.generate(**kw, past_key_values=_turn1(which, P0, kv)[0])           # host_loop: the same forwards; its own draw
    assert host.sequences.shape == want.shape and torch.equal(host.sequences[:, :seq2.shape[1]], seq2)
    greedy_host = model.generate(input_ids=seq2, max_new_tokens=6, eos_token_id=-1, no_repeat_ngram_size=50, past_key_values=_turn1(which, P0, kv)[0])
    assert torch.equal(greedy_host, _hand(model, _turn1(which, P0, kv)[0], seq2, 6)[0]), "host loop (a ban that never fires), greedy"


@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
def test_second_turn_under_prompt_lookup(kv):
    """against the same call on a cache prepared by hand to the same state; a repeating suffix, so that drafts are made and accepted"""
    model = _model("hd128")[0]
    c_gen, seq1 = _turn1("hd128", 60, kv)
    rep = _ids(1, 6, 99)
    seq2 = torch.cat([seq1, rep, rep, rep[:, :3]], dim=1)
    P = c_gen.length
    hand = model.new_kv_cache(1, 256, kv_cache_dtype=kv)                         # the same state, by hand: the prompt, then one token per call
    with torch.no_grad():
        model.forward(input_ids=seq1[:, :60], past_key_values=hand, use_cache=True)
        for j in range(60, P):
            model.forward(input_ids=seq1[:, j:j + 1], past_key_values=hand, use_cache=True)
    kw = dict(input_ids=seq2, max_new_tokens=12, eos_token_id=-1, prompt_lookup_num_tokens=4, return_dict_in_generate=True, output_logprobs=True)
    a = model.generate(**kw, past_key_values=c_gen)
    b = model.generate(**kw, past_key_values=hand)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs)
    assert c_gen.length == hand.length == a.sequences.shape[1] - 1 and torch.equal(c_gen.ids, a.sequences[:, :-1])


# ---- 3. against the one-shot call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,P0,u", [("tiny", 60, 5), ("hd128", 60, 17), ("hd128", 64, 40), ("hd128", 698, 16)])
def test_second_turn_logits_against_the_one_shot_forward(which, P0, u):
    """the rule of test_continuation_equals_one_shot_prefill: the error of the fed ids' logits against the oracle's fp32 LLaMA stack on the
    same weights is at most max(1.5 x the no-cache HIP forward's, 2^-7)."""
    model, sd, cd = _model(which)
    c, seq1 = _turn1(which, P0, None)
    seq2 = torch.cat([seq1, _ids(1, u, 17 * P0 + u)], dim=1)
    P = c.length
    with torch.no_grad():
        cont = model.forward(input_ids=seq2[:, P:], past_key_values=c, use_cache=True).logits
        nocache = model.forward(input_ids=seq2).logits[:, P:]
    sd32 = {k: v.float() for k, v in sd.items()}
    ids = seq2.cpu()
    mask = torch.ones_like(ids)
    hs, _ = O.llama_model(sd32, cd, F.embedding(ids, sd32["model.embed_tokens.weight"]), mask, (mask.cumsum(-1) - 1))
    truth = F.linear(hs[-1], sd32["lm_head.weight"])[:, P:]
    e_cont, e_nc = rel_err(cont.cpu(), truth), rel_err(nocache.cpu(), truth)
    print(f"second turn {which} P={P} fed={seq2.shape[1] - P}: logits err vs fp32 -- continuation {e_cont:.5f}, no-cache {e_nc:.5f}")
    assert e_cont <= max(1.5 * e_nc, 2.0 ** -7)


# ---- 4. the prefix check ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("m", [0, 1, "P-1", None, "L==P"])
def test_prefix_check_cuts_the_cache_to_the_common_prefix(m, kv):
    model = _model("hd128")[0]
    c, seq1 = _turn1("hd128", 60, kv)
    P = c.length
    if m == "L==P":
        seq2, keep = c.ids.clone(), P - 1                              # nothing new: the last token is fed again
    else:
        seq2 = torch.cat([seq1, _ids(1, 5, 77)], dim=1)
        keep = P if m is None else P - 1 if m == "P-1" else m
        if m is not None:
            seq2[0, keep] = (seq2[0, keep] + 1) % 90
    by_hand = _clone(c, length=keep)
    kw = dict(input_ids=seq2, max_new_tokens=5, eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True, output_hidden_states=True)
    a = model.generate(**kw, past_key_values=c)
    b = model.generate(**kw, past_key_values=by_hand)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs)
    assert torch.equal(a.hidden_states[-1][-1], b.hidden_states[-1][-1])
    assert torch.equal(a.sequences[:, :seq2.shape[1]], seq2)
    assert c.length == a.sequences.shape[1] - 1 and torch.equal(c.ids, a.sequences[:, :-1]), "the cache describes the new sequence"


def test_refusals_that_need_the_device():
    model = _model("hd128")[0]
    c, seq1 = _turn1("hd128", 60, None)
    bad = torch.cat([seq1, torch.tensor([[5, _MM["IMG_START"], 7]], device=DEV)], dim=1)
    bad[0, 50] = (bad[0, 50] + 1) % 90                                  # (the cache would also be cut to 50 positions)
    P, ids_before = c.length, c.ids.clone()
    with pytest.raises(NotImplementedError, match="placeholder"):
        model.generate(input_ids=bad, max_new_tokens=2, past_key_values=c)
    assert c.length == P and torch.equal(c.ids, ids_before) and sum(h.shape[1] for h in c.last_hidden) == P, "a refused call leaves the cache as it was"
    hf = _turn1("hd128", 60, None)[0].to_legacy_cache()                  # an HF tuple: ids unknown, the caller is trusted
    seq2 = torch.cat([seq1, _ids(1, 4, 3)], dim=1)
    got = model.generate(input_ids=seq2, max_new_tokens=4, eos_token_id=-1, past_key_values=hf, return_dict_in_generate=True)
    assert got.past_key_values.ids is None and got.past_key_values.length == seq2.shape[1] + 3
    with pytest.raises(ValueError, match="hidden"):
        model.generate(input_ids=seq2, max_new_tokens=4, past_key_values=hf, return_dict_in_generate=True, output_hidden_states=True)
    with pytest.raises(TypeError):
        model.generate(input_ids=seq2, max_new_tokens=4, past_key_values=_turn1("hd128", 60, None)[0], repetition_penalty=1.1)


# ---- 5. growth and fork ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
def test_a_cache_of_capacity_exactly_P_is_grown_by_the_call(kv):
    model = _model("hd128")[0]
    big, seq1 = _turn1("hd128", 59, kv)                                 # 59 + 6 - 1 = 64 positions
    assert big.length == 64 and big.smax > 64
    small = _clone(big, smax=64)
    assert small.smax == 64
    seq2 = torch.cat([seq1, _ids(1, 17, 8)], dim=1)
    kw = dict(input_ids=seq2, max_new_tokens=6, eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True)
    a = model.generate(**kw, past_key_values=small)
    b = model.generate(**kw, past_key_values=big)
    assert small.smax >= seq2.shape[1] + 7
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs)


def test_grow_leaves_the_vt_columns_beyond_the_sequence_zero():
    c, _ = _turn1("hd128", 60, None)
    c.truncate(40)                                                      # (stale columns 40 .. 64 in the old buffers)
    k_before = [t[:, :, :40].clone() for t in c.k]
    with pytest.raises(ValueError):
        c.grow(39)
    c.grow(200)
    assert c.smax == 256 and c.length == 40 and c.k[0].shape[2] == 256
    old = torch.tensor([_vt_slot(p) for p in range(40)], device=DEV)
    tail = torch.tensor(sorted(set(range(c.smax)) - {_vt_slot(p) for p in range(40)}), device=DEV)
    ref = _turn1("hd128", 60, None)[0]
    for li in range(len(c.k)):
        assert torch.equal(c.k[li][:, :, :40], k_before[li]) and torch.equal(c.vt[li][..., old], ref.vt[li][..., old])
        assert not bool(c.vt[li][..., tail].any()), f"layer {li}: V^T columns beyond the sequence must be zero"


@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
def test_fork_gives_independent_caches(kv):
    model = _model("hd128")[0]
    c, seq1 = _turn1("hd128", 65, kv)
    before = [t.clone() for t in _buffers(c)]
    ids_before, n_before = c.ids.clone(), c.length
    with pytest.raises(ValueError):
        c.grow(c.length - 1)
    for seed in (1, 2):
        seq2 = torch.cat([seq1, _ids(1, 9, seed)], dim=1)
        kw = dict(input_ids=seq2, max_new_tokens=6, eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True)
        f = c.fork()
        assert f is not c and f.smax == c.smax and f.length == c.length and torch.equal(f.ids, c.ids)
        a = model.generate(**kw, past_key_values=f)
        b = model.generate(**kw, past_key_values=_turn1("hd128", 65, kv)[0])
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs), f"suffix {seed}"
    assert c.length == n_before and torch.equal(c.ids, ids_before)
    assert all(torch.equal(x, y) for x, y in zip(_buffers(c), before)), "the original cache is untouched"


@pytest.mark.parametrize("kv", [None, KV8], ids=["bf16", "fp8"])
def test_the_cache_after_fused_loop_trimmed_an_overrun(kv):
    """EOS at the second new token: the device loop looks at the host every 8 steps, runs past the end and trims.  The cache then covers
    sequences.shape[1] - 1 positions, ids and hidden states alike, and a third turn on it equals the hand-written loop."""
    model = _model("hd128")[0]
    c, seq1 = _turn1("hd128", 60, kv)
    mm = set(_MM.values())
    for seed in range(21, 61):                                          # a suffix whose first two new tokens differ and are no placeholder ids
        seq2 = torch.cat([seq1, _ids(1, 5, seed)], dim=1)
        L = seq2.shape[1]
        dry, _ = _hand(model, _turn1("hd128", 60, kv)[0], seq2, 10)
        first, eos = int(dry[0, L]), int(dry[0, L + 1])
        if eos != first and not {first, eos} & mm:
            break
    else:
        pytest.fail("no suffix tried gives the EOS pattern")
    out = model.generate(input_ids=seq2, max_new_tokens=10, eos_token_id=eos, past_key_values=c, return_dict_in_generate=True, output_hidden_states=True)
    assert torch.equal(out.sequences, dry[:, :L + 2])
    assert c.length == L + 1 and torch.equal(c.ids, out.sequences[:, :-1]) and out.hidden_states[-1][-1].shape[1] == L + 1
    by_hand = _turn1("hd128", 60, kv)[0]
    _hand(model, by_hand, seq2, 2)                                      # the same state without an overrun: L + 1 positions
    assert by_hand.length == L + 1
    seq3 = torch.cat([out.sequences, _ids(1, 3, 22)], dim=1)
    want, want_lp = _hand(model, by_hand, seq3, 4)
    got = model.generate(input_ids=seq3, max_new_tokens=4, eos_token_id=-1, past_key_values=c, return_dict_in_generate=True, output_logprobs=True)
    assert torch.equal(got.sequences, want) and torch.equal(got.logprobs, want_lp)


# ---- 6. a padded batch -----------------------------------------------------------------------------------------------------------------
def test_padded_batch_second_turn():
    model = _model("tiny")[0]
    L0, pad_n = 20, 7
    mask1 = torch.ones(2, L0, dtype=torch.long, device=DEV)
    mask1[1, :pad_n] = 0                                                # left-padded
    for seed in range(40):                                              # a prompt whose row 0 can end after 2 tokens while row 1 runs all 6
        ids1 = _ids(2, L0, 500 + seed)
        dry = model.generate(input_ids=ids1, attention_mask=mask1, max_new_tokens=6, eos_token_id=-1, use_cache=True)
        eos = int(dry[0, L0 + 1])
        if eos != int(dry[0, L0]) and eos not in dry[1, L0:].tolist():
            break
    else:
        pytest.fail("no seed gives the EOS pattern")
    c = model.new_kv_cache(2, 64)
    out = model.generate(input_ids=ids1, attention_mask=mask1, max_new_tokens=6, eos_token_id=eos, pad_token_id=0, past_key_values=c,
                         return_dict_in_generate=True)
    seq1 = out.sequences
    assert seq1.shape[1] == L0 + 6 and seq1[0, L0 + 2:].tolist() == [0] * 4 and c.length == L0 + 5
    seq2 = torch.cat([seq1, _ids(2, 5, 9)], dim=1)
    mask2 = torch.ones_like(seq2)
    mask2[1, :pad_n] = 0
    mask2[0, L0 + 2:L0 + 6] = 0                                         # row 0's pad fill behind its EOS
    want, want_lp = _hand(model, _clone(c), seq2, 6, mask=mask2, eos=eos, pad=0)
    bad = mask2.clone()
    bad[1, pad_n + 3] = 0                                               # a visible cached position in the middle
    with pytest.raises(ValueError, match="attention_mask"):
        model.generate(input_ids=seq2, attention_mask=bad, max_new_tokens=6, eos_token_id=eos, pad_token_id=0, past_key_values=_clone(c))
    got = model.generate(input_ids=seq2, attention_mask=mask2, max_new_tokens=6, eos_token_id=eos, pad_token_id=0, past_key_values=c,
                         return_dict_in_generate=True, output_logprobs=True)
    n = got.sequences.shape[1]
    assert torch.equal(got.sequences, want[:, :n]) and torch.equal(got.logprobs, want_lp[:, :n - seq2.shape[1]])
    if n < want.shape[1]:                                               # (both rows ended early: the hand loop went on with pad fill)
        assert bool((want[:, n:] == 0).all())
    # the cache covers every position fed, also where fused_loop trimmed steps that ran past the end
    assert c.length == n - 1 and torch.equal(c.ids, got.sequences[:, :-1]) and c.mask.shape == (2, n - 1)
    assert sum(h.shape[1] for h in c.last_hidden) == n - 1


# ---- 7. evaluate() on the tiny full model ----------------------------------------------------------------------------------------------
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


def _same_lists(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_evaluate_two_turns_on_one_cache_and_the_plain_call():
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    model.llm.strict_checks = False
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    images, ids1 = fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV)
    sizes, resizes = [fx["size_list"][0]], [fx["resize_list"][0]]
    mm = set(fx["cfg"]["llm"]["mm_token_ids"].values())
    calls = []
    enc = model._visual_embs_tm
    model._visual_embs_tm = lambda x: (calls.append(1), enc(x))[1]

    def by_hand(cache, ids, n_new, emb):
        """llm.generate on the prepared cache, then _select / _decode: what evaluate() does behind its SAM encoder"""
        out = model.llm.generate(input_ids=ids, images=images, max_new_tokens=n_new, do_sample=False, temperature=0.0, output_hidden_states=True,
                                 return_dict_in_generate=True, keep_last_step_only=True, past_key_values=cache)
        seq, last = out.sequences, out.hidden_states[-1][-1]
        assert last.shape[1] == seq.shape[1] - 1, "hidden states cover all positions"
        L1 = last.shape[1]
        seg = model._select(last, (seq[:, 1:] == model.config.seg_token_idx)[:, :L1], model.seg_projector)
        loc = model._select(last, (seq[:, 1:] == model.config.loc_token_idx)[:, :L1], model.det_projector)
        return seq, model._decode(emb, seg, resizes, sizes), [model._run_mlp(model.det_decoder, e) if e.shape[0] else e.new_empty(0, 4) for e in loc]

    # a cache of another geometry is refused before the SAM encoder starts, and nothing is kept on it
    foreign = pkg("modeling_core").KVCache(model.llm.config.num_hidden_layers + 1, 1, model.llm.config.num_attention_heads, 16, 64, DEV)
    with pytest.raises(ValueError, match="layers, heads, head_dim"):
        model.evaluate(images_sam, images, ids1, sizes, resizes, max_new_tokens=4, temperature=0.0, past_key_values=foreign)
    assert calls == [] and foreign.side == {}
    for n1 in range(4, 9):                                              # (the last token of turn 1 is fed by turn 2: it must not be a placeholder id)
        c = model.new_kv_cache(1, 64)
        seq1, masks1, boxes1 = model.evaluate(images_sam, images, ids1, sizes, resizes, max_new_tokens=n1, temperature=0.0, past_key_values=c)
        if int(seq1[0, -1]) not in mm:
            break
    emb = c.side["sam_image_embeddings"]
    h = model.new_kv_cache(1, 64)
    hs1, hm1, hb1 = by_hand(h, ids1, n1, emb)
    assert torch.equal(seq1, hs1) and _same_lists(masks1, hm1) and _same_lists(boxes1, hb1)
    # the plain call (no cache), same arguments: its ids, masks and boxes are those of the call that fills an empty cache, and so of the
    # hand-driven run
    del calls[:]
    plain = model.evaluate(images_sam, images, ids1, sizes, resizes, max_new_tokens=n1, temperature=0.0)
    assert len(plain) == 3 and calls == [1]
    assert torch.equal(plain[0], seq1) and _same_lists(plain[1], masks1) and _same_lists(plain[2], boxes1)
    assert torch.equal(plain[0], hs1) and _same_lists(plain[1], hm1) and _same_lists(plain[2], hb1)
    seg_or_loc = torch.tensor([[7, model.config.seg_token_idx, 9, model.config.loc_token_idx, 11]], device=DEV)
    ids2 = torch.cat([seq1, seg_or_loc], dim=1)
    del calls[:]
    seq2, masks2, boxes2 = model.evaluate(images_sam, images, ids2, sizes, resizes, max_new_tokens=5, temperature=0.0, past_key_values=c)
    assert calls == [], "the second call must not run the SAM encoder"
    hs2, hm2, hb2 = by_hand(h, ids2, 5, emb)
    assert torch.equal(seq2, hs2) and _same_lists(masks2, hm2) and _same_lists(boxes2, hb2)
    assert len(masks2[0]) >= 1 and len(boxes2[0]) >= 1                  # (the [SEG] and [LOC] of the second turn's prompt are decoded)
    assert c.length == seq2.shape[1] - 1 and torch.equal(c.ids, seq2[:, :-1])


# ---- 8. a plain call is unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny", "hd128"])
def test_a_plain_generate_call_is_unchanged(which):
    """without `past_key_values`: the ids of the prefill + one-token loop written on forward() alone, and exactly the old dict keys"""
    model = _model(which)[0]
    ids = _ids(1, 37, 4)
    want, want_lp = _hand(model, model.new_kv_cache(1, 64), ids, 6)
    out = model.generate(input_ids=ids, max_new_tokens=6, eos_token_id=-1, use_cache=True, return_dict_in_generate=True, output_hidden_states=True)
    assert torch.equal(out.sequences, want) and set(out.keys()) == {"sequences", "hidden_states"}
    out = model.generate(input_ids=ids, max_new_tokens=6, eos_token_id=-1, use_cache=True, return_dict_in_generate=True, output_logprobs=True)
    assert torch.equal(out.logprobs, want_lp) and set(out.keys()) == {"sequences", "hidden_states", "logprobs"}
