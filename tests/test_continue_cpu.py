"""generate(past_key_values=) / evaluate(past_key_values=) without a GPU: where the keyword stands, every refusal of check_generate_args in
its documented order, the C ABI of the two new entry points, and the host-side bookkeeping of KVCache (ids, truncate, grow, fork)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"ull_ids_common_prefix": 8, "ull_kv8_copy_positions": 16}
IDS = torch.zeros(1, 8, dtype=torch.int64)


def _cache(B=1, n_layers=2, H=2, hd=16, smax=64, **kw):
    return pkg("kv_cache").KVCache(n_layers, B, H, hd, smax, "cpu", **kw)


def test_where_the_keyword_stands():
    """evaluate(): a named parameter between `ngram_ban` and `prompt_lookup_num_tokens`, default None; its pinned first seven and last four
    parameters stay.  generate(): `output_logprobs` is pinned as the LAST named parameter (tests/test_logprobs_cpu.py), so the keyword
    behind it is read from **kwargs -- by keyword, default None -- and every other unknown keyword keeps raising TypeError."""
    MC, MU = pkg("modeling_core"), pkg("modeling_ullava")
    ev = inspect.signature(MU.UllavaForCausalLM.evaluate).parameters
    names = list(ev)
    assert names[:7] == ["self", "images_sam", "images", "input_ids", "raw_size_list", "resize_list", "max_new_tokens"]
    assert names[-4:] == ["prompt_lookup_num_tokens", "max_matching_ngram_size", "output_logprobs", "sampler"]
    i = names.index("past_key_values")
    assert names[i - 1] == "ngram_ban" and names[i + 1] == "prompt_lookup_num_tokens" and ev["past_key_values"].default is None
    gen = inspect.signature(MC.UllavaCoreForCausalLM.generate).parameters
    assert list(gen)[-2:] == ["output_logprobs", "kwargs"] and gen["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "past_key_values" in MC.UllavaCoreForCausalLM.generate.__doc__
    for cls in (MC.UllavaCoreForCausalLM, MU.UllavaForCausalLM):
        assert list(inspect.signature(cls.new_kv_cache).parameters) == ["self", "batch_size", "capacity", "kv_cache_dtype"]


def test_generate_takes_past_key_values_and_still_refuses_unknown_keywords():
    """the test that fails without the feature: the parent commit answers `past_key_values` with the TypeError of an unknown keyword.
    Here the keyword reaches check_generate_args, whose last refusal (CPU tensors) is the one a well-formed CPU call meets."""
    model = _tiny_core()
    cfg = model.config
    H = cfg.num_attention_heads
    c = _cache(n_layers=cfg.num_hidden_layers, H=H, hd=cfg.hidden_size // H)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        model.generate(input_ids=IDS, max_new_tokens=2, past_key_values=c)
    with pytest.raises(ValueError, match="layers, heads, head_dim"):
        model.generate(input_ids=IDS, max_new_tokens=2, past_key_values=_cache(n_layers=cfg.num_hidden_layers + 1, H=H, hd=cfg.hidden_size // H))
    for name in ("repetition_penalty", "output_scores", "prompt_lookup_tokens"):
        with pytest.raises(TypeError, match=name):
            model.generate(input_ids=IDS, max_new_tokens=2, past_key_values=c, **{name: 1})
        with pytest.raises(TypeError, match=name):
            model.generate(input_ids=IDS, max_new_tokens=2, **{name: 1})
    made = model.new_kv_cache(3, 100, None)
    assert made._geom[:4] == (cfg.num_hidden_layers, 3, H, cfg.hidden_size // H) and made.smax == 128 and made.length == 0


def test_refusals_in_the_documented_order():
    """use_cache=False; batch; layers / heads / head_dim; kv_cache_dtype; hidden states of an HF cache; num_beams; CPU tensors -- each call
    below is wrong in everything from its own refusal on, so the one raised is the first of them."""
    G = pkg("generation")
    shape = (2, 2, 16)
    c = _cache()
    c8 = _cache(kv_dtype="fp8_e4m3")
    hf = tuple((torch.zeros(1, 2, 5, 16), torch.zeros(1, 2, 5, 16)) for _ in range(2))
    chk = lambda ids=IDS, **kw: G.check_generate_args(ids, cache_shape=shape, dtype=torch.bfloat16, **kw)          # noqa: E731
    with pytest.raises(ValueError, match="use_cache=True"):
        chk(past_key_values=_cache(B=2), use_cache=False, kv_cache_dtype="fp8_e4m3", num_beams=2)
    with pytest.raises(ValueError, match="2 rows"):
        chk(past_key_values=_cache(B=2, H=4), kv_cache_dtype="fp8_e4m3", num_beams=2)
    for wrong in (dict(n_layers=3), dict(H=4), dict(hd=32)):
        with pytest.raises(ValueError, match="layers, heads, head_dim"):
            chk(past_key_values=_cache(**wrong), kv_cache_dtype="fp8_e4m3", num_beams=2)
    with pytest.raises(ValueError, match="contradicts"):
        chk(past_key_values=c, kv_cache_dtype="fp8_e4m3", num_beams=2)
    with pytest.raises(ValueError, match="hidden"):
        chk(past_key_values=hf, output_hidden_states=True, num_beams=2)
    with pytest.raises(NotImplementedError, match="num_beams=2"):
        chk(past_key_values=c, num_beams=2)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        chk(past_key_values=c)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        chk(past_key_values=c8)                                       # (kv_cache_dtype unset: the cache's own dtype decides)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        chk(past_key_values=c8, kv_cache_dtype="fp8_e4m3", output_hidden_states=True)        # an EMPTY KVCache has no hidden states to miss
    with pytest.raises(RuntimeError, match="GPU tensors"):
        G.check_generate_args(IDS, past_key_values=hf)                # (an HF tuple, the model's shape not known)
    with pytest.raises(TypeError, match="KVCache"):
        chk(past_key_values=7)
    # evaluate() runs the same function before it starts the SAM encoder, and without a cache nothing changes
    assert G.check_generate_args(IDS, config_use_cache=False)[3] is False


def test_the_new_entry_points_are_declared_bound_and_exported():
    L = pkg("_lib")
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name, n_args in NEW_ENTRIES.items():
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, header)) == 1, name
        assert len(L.SIGNATURES[name]) == n_args and L.RESTYPES[name] is ctypes.c_int, name
        assert getattr(lib, name) is not None, name
    assert L.SIGNATURES["ull_ids_common_prefix"] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                     ctypes.c_void_p, ctypes.c_void_p]
    assert L.SIGNATURES["ull_kv8_copy_positions"] == [ctypes.c_void_p] * 8 + [ctypes.c_int64] * 7 + [ctypes.c_void_p]
    mk = open(os.path.join(ROOT, "u-llava_amd", "csrc", "Makefile")).read()
    assert "kv_continue.hip" in re.search(r"^ONCE_SRCS\s*=(.*)$", mk, flags=re.M).group(1)
    # argument checks that launch nothing: they answer without a GPU
    fn = getattr(L.load(), "ull_ids_common_prefix")
    assert fn(None, 0, None, 0, 0, 0, None, None) == 0                                                           # R == 0: nothing to do
    assert fn(None, 0, None, 0, 0, -1, None, None) == L.DEFINES["ULL_ERR_ARG"]
    assert fn(None, 4, None, 4, 2, 3, None, None) == L.DEFINES["ULL_ERR_ARG"]                                    # null pointers that would be used


def test_the_cache_remembers_its_ids_and_truncate_trims_them():
    c = _cache(B=2)
    assert c.ids.shape == (2, 0) and c.ids.dtype == torch.int64 and c.mask is None and c.side == {}
    a, b = torch.arange(10).view(2, 5), torch.arange(10, 16).view(2, 3)
    c.length = 5; c.note_fed(a, 5)
    c.length = 8; c.note_fed(b, 3)
    assert torch.equal(c.ids, torch.cat([a, b], dim=1))
    a[0, 0] = 99                                                        # the joined ids are the cache's own tensor, no view of the caller's
    assert int(c.ids[0, 0]) == 0
    c.last_hidden = [torch.zeros(2, 5, 4), torch.ones(2, 3, 4)]
    c.truncate(6)
    assert c.length == 6 and c.ids.shape == (2, 6) and torch.equal(c.ids[:, 5:], b[:, :1]) and sum(h.shape[1] for h in c.last_hidden) == 6
    c.length = 7; c.note_fed(None, 1)                                   # fed as embeddings: unknown from here on
    assert c.ids is None
    c.truncate(3)
    assert c.ids is None and c.length == 3
    c.truncate(0)
    assert c.ids.shape == (2, 0), "an empty cache knows its ids again"
    m = torch.ones(2, 4, dtype=torch.long)
    c.length = 4; c.note_fed(torch.zeros(2, 4, dtype=torch.int64), 4, m)
    assert torch.equal(c.mask, m) and c.mask is not m, "the cache keeps copies: the caller may reuse its tensors"
    c.length = 5; c.note_fed(torch.zeros(2, 1, dtype=torch.int64), 1, None)
    assert c.mask.shape == (2, 5) and bool(c.mask.all())
    c.truncate(2)
    assert c.mask.shape == (2, 2)
    # inside generate() (borrow_ids) the loops' tensors are noted as they come, and own_ids() joins them into the cache's own before it returns
    c.truncate(0)
    c.borrow_ids = True
    x, m2 = torch.arange(6).view(2, 3), torch.ones(2, 3, dtype=torch.long)
    c.length = 3; c.note_fed(x, 3, m2)
    assert c._id_chunks[0][0] is x and c.mask is m2
    c.borrow_ids = False
    c.own_ids()
    x[0, 0], m2[0, 0] = 77, 0
    assert int(c.ids[0, 0]) == 0 and int(c.mask[0, 0]) == 1
    for j in range(40):                                                 # one-token steps: the copies are joined every 32 calls
        c.length += 1; c.note_fed(torch.full((2, 1), j), 1)
    assert len(c._id_chunks) <= 32 and c.ids.shape == (2, 43) and c.ids[0, 3:].tolist() == list(range(40))


@pytest.mark.parametrize("kv", [None, "fp8_e4m3"])
def test_grow_and_fork_on_the_host_side(kv):
    c = _cache(kv_dtype=kv)
    c.length = 10
    with pytest.raises(ValueError, match="holds 10"):
        c.grow(9)
    c.length = 0                                                        # (nothing to copy: the host side alone)
    c.side["x"] = 1
    bufs = lambda t: (t.k + t.vt) if kv is None else (t.k8 + t.vt8 + t.k_scale + t.vt_scale)          # noqa: E731
    old = [b.data_ptr() for b in bufs(c)]
    c.c_ptrs()
    c.grow(64)
    assert c.smax == 64 and [b.data_ptr() for b in bufs(c)] == old, "a capacity the cache has changes nothing"
    c.grow(65)
    assert c.smax == 128 and all(b.shape[3 if b.dim() == 4 and b.shape[2] == 16 else 2] == 128 for b in bufs(c))
    assert getattr(c, "_c_ptrs", None) is None and getattr(c, "_kv8_ptrs", None) is None and getattr(c, "_gather_scratch", None) is None
    if kv is None:
        assert not any(bool(t.any()) for t in c.vt)
    f = c.fork()
    assert f is not c and f.smax == 128 and f.kv_dtype == kv and f.length == 0 and f.side == {"x": 1} and f.side is not c.side
    assert not set(b.data_ptr() for b in bufs(f)) & set(b.data_ptr() for b in bufs(c))
    # replicated / gather_rows keep refusing the fp8 cache
    if kv is not None:
        with pytest.raises(NotImplementedError):
            c.replicated(2)
        with pytest.raises(NotImplementedError):
            c.gather_rows(None, 0, 1)
