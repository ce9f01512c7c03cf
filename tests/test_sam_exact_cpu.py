"""No GPU: the opt-in reference-rounding SAM global attention (SamEngine.global_attention = "exact", DESIGN f11) -- the two exported
entries and their refusals, the routing predicate ops.sam_global_exact_takes, the mode validation of UllavaForCausalLM.set_sam_attention,
and the kernel's five-operation quotient against the IEEE division it stands for.  The GPU tests are in tests/test_sam_exact_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ull_sam_global_attention_exact_bf16", "ull_sam_global_attention_exact_f16")


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_both_entries_without_an_f32_twin():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for entry in ENTRIES:
        assert re.search(r"^int " + entry + r"\(", header, flags=re.M), entry
        assert entry in L.SIGNATURES and hasattr(lib, entry), entry
    twin = "ull_sam_global_attention_exact_f32"
    assert twin not in header and twin not in L.SIGNATURES and not hasattr(lib, twin), "the fp32 build's attention is exact already"


def test_header_entry_list_equals_the_bound_signatures():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    declared = set(re.findall(r"\bint(?:64_t)? (ull_[a-z0-9_]+)\(", header))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    # the declaration's parameter count is the bound one's
    for entry in ENTRIES:
        params = re.search(r"^int " + entry + r"\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(params.split(",")) == len(L.SIGNATURES[entry]) == 24, entry


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2
_C = 2 * 80
_LD = 3 * _C


def _rc(entry, Q=_ADDR, q_st=(4096 * _LD, 80, _LD), K=_ADDR, k_st=(4096 * _LD, 80, _LD), V=_ADDR, v_st=(4096 * _LD, 80, _LD), rel_h=_ADDR,
        rel_w=_ADDR, B=1, H=2, side=64, hd=80, q_scale=80 ** -0.5, O=_ADDR, o_st=(4096 * _C, 80, _C)):
    return getattr(pkg("_lib").load(), entry)(Q, *q_st, K, *k_st, V, *v_st, rel_h, rel_w, B, H, side, hd, q_scale, O, *o_st, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_refuses_bad_arguments_without_launching(entry):
    for null in ("Q", "K", "V", "rel_h", "rel_w", "O"):
        assert _rc(entry, **{null: None}) == ERR_ARG, null
    assert _rc(entry, B=0) == ERR_ARG and _rc(entry, H=0) == ERR_ARG and _rc(entry, B=-1) == ERR_ARG
    assert _rc(entry, side=63) == ERR_SHAPE and _rc(entry, side=32) == ERR_SHAPE and _rc(entry, side=128) == ERR_SHAPE, "the 64 x 64 grid only"
    assert _rc(entry, hd=64) == ERR_SHAPE and _rc(entry, hd=128) == ERR_SHAPE and _rc(entry, hd=0) == ERR_SHAPE, "head dim 80 only"
    for which in ("q_st", "k_st", "v_st", "o_st"):
        base = (4096 * _C, 80, _C) if which == "o_st" else (4096 * _LD, 80, _LD)
        for i in range(3):
            for delta in (1, 4):                                   # an odd stride; a stride that is a multiple of 8 bytes but not of 16
                st = list(base)
                st[i] += delta
                assert _rc(entry, **{which: tuple(st)}) == ERR_SHAPE, (which, i, delta)
        st = list(base)
        st[2] = 72                                                 # rows that overlap (token stride below the head dim)
        assert _rc(entry, **{which: tuple(st)}) == ERR_SHAPE, which
    for which in ("Q", "K", "V", "rel_h", "rel_w", "O"):
        for off in (2, 8):
            assert _rc(entry, **{which: _ADDR + off}) == ERR_SHAPE, (which, off)
    # 32-bit per-lane offsets of the DMA pieces inside a 64-key tile: 128 * stride bytes stay below 2^31
    big = 1 << 24
    assert _rc(entry, k_st=(4096 * big, 80, big)) == ERR_SHAPE and _rc(entry, v_st=(4096 * big, 80, big)) == ERR_SHAPE
    assert _rc(entry, B=1 << 20, H=2) == ERR_SHAPE, "the grid's block count stays in 32 bits"


# ---- routing ------------------------------------------------------------------------------------------------------------------------------
def test_routing_predicate_truth_table():
    takes = pkg("ops").sam_global_exact_takes
    for dt in (torch.bfloat16, torch.float16):
        assert takes(64, 80, dt)
        for side, hd in ((63, 80), (32, 80), (48, 80), (14, 80), (128, 80), (64, 64), (64, 32), (64, 128), (64, 96)):
            assert not takes(side, hd, dt), (side, hd)
    assert not takes(64, 80, torch.float32), "the fp32 build has no such kernel and needs none"


def _tiny_model():
    C, M = pkg("configuration"), pkg("modeling_ullava")
    cfg = C.UllavaConfig(llm_config=dict(vision_config=dict(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64, image_size=28,
                                                            patch_size=14), vocab_size=120, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                         num_attention_heads=4), seg_token_idx=101, loc_token_idx=102, out_dim=256,
                         sam_config=dict(embed_dim=32, depth=2, num_heads=2, global_attn_indexes=[1]))
    return M.UllavaForCausalLM(cfg)


def test_mode_validation_on_a_tiny_model():
    S = pkg("sam")
    m = _tiny_model()
    assert m.sam_attention == "streamed" and m._sam.global_attention == "streamed" and S.SamEngine.global_attention == "streamed"
    for bad in ("Exact", "two-pass", "", None, 1):
        with pytest.raises(ValueError, match="sam attention mode"):
            m.set_sam_attention(bad)
        assert m.sam_attention == "streamed", "a refused mode changes nothing"
    assert m.set_sam_attention("exact") is m
    assert m.sam_attention == "exact" and m._sam.global_attention == "exact"
    assert _tiny_model().sam_attention == "streamed", "the mode belongs to one model"
    assert m.set_sam_attention("streamed") is m and m.sam_attention == "streamed"
    # an engine whose attribute was set to nonsense directly refuses to encode (before it touches the GPU)
    m._sam.global_attention = "fast"
    with pytest.raises(ValueError, match="global_attention"):
        m._sam.encode(torch.zeros(1, 3, 1024, 1024, dtype=torch.bfloat16))


# ---- the kernel's quotient ----------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """RN32(a * b + c) for float32 arrays.  The product of two float32 is exact in float64; where the float64 sum is not exact it still rounds
    to the same float32 unless it lands within 2^-29 of a float32 rounding boundary (double rounding) -- the callers below stay clear of
    that: their sums either cancel (exact) or add a term far below the other's last float64 bit only in the sticky position."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _div5(e, l):
    """sam_global_exact_kernel's quotient: y = RN(1 / l) once per query; per key q0 = RN(e y), q1 = fma(fma(-q0, l, e), y, q0),
    q = fma(fma(-q1, l, e), y, q1)."""
    y = (np.float32(1.0) / l).astype(np.float32)
    q0 = (e * y).astype(np.float32)
    q1 = _fma32(_fma32(-q0, l, e), y, q0)
    r = _fma32(-q1, l, e)
    assert np.array_equal(r.astype(np.float64), e.astype(np.float64) - q1.astype(np.float64) * l.astype(np.float64)), "the last remainder is exact"
    return _fma32(r, y, q1)


def test_five_operation_quotient_is_the_ieee_division():
    """P = r16(e / l) with e = exp(s - m) in [2^-100, 1] (there the last bit of the remainder e - q1 l, 2^-47 e, is in the fp32 range and one
    fma holds it exactly; a smaller e is a probability below 2^-100 of the row's largest) and l in [1, 4096]: the kernel's mul + 4 fma give the
    correctly rounded quotient (Markstein's theorem), bit for bit what `e / l` gives -- on 6e6 random pairs, on sums next to powers of two,
    and on numerators next to powers of two."""
    rng = np.random.default_rng(0)
    n = 2_000_000
    l = rng.uniform(1.0, 4096.0, n).astype(np.float32)
    cases = [(np.exp(rng.uniform(-69.0, 0.0, n)).astype(np.float32), l),
             (rng.uniform(0.0, 1.0, n).astype(np.float32) + np.float32(2.0 ** -100), l),
             (np.exp(rng.uniform(-20.0, 0.0, n)).astype(np.float32), np.exp2(rng.uniform(0.0, 12.0, n)).astype(np.float32))]
    # sums within 64 ulps of a power of two (all-ones significands included), numerators likewise
    edge_l = np.concatenate([np.float32(2.0 ** k) + np.arange(-64, 65, dtype=np.float32) * np.float32(2.0 ** (k - 23)) for k in range(1, 13)])
    edge_l = edge_l[(edge_l >= 1.0) & (edge_l <= 4096.0)]
    edge_e = np.concatenate([np.float32(2.0 ** -k) + np.arange(-64, 65, dtype=np.float32) * np.float32(2.0 ** (-k - 24)) for k in range(0, 97, 3)])
    edge_e = edge_e[edge_e <= 1.0]
    ee, ll = np.meshgrid(edge_e, edge_l)
    cases.append((ee.ravel().astype(np.float32), ll.ravel().astype(np.float32)))
    for e, l_ in cases:
        want = (e / l_).astype(np.float32)
        got = _div5(e, l_)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
