"""No GPU: the FP8 (e4m3) KV cache's C entry points (declared and exported) and its argument refusals, which come before any device work."""
import ctypes
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV8_ENTRIES = ("ull_attention_kv8_bf16", "ull_kv8_quantize_bf16", "ull_kv8_dequantize_bf16", "ull_llama_decode_layers_kv8_bf16")


def test_kv8_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib = pkg("_lib")
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in KV8_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} not declared in include/ullava_hip.h"
        assert name in lib.SIGNATURES, f"{name} not bound in _lib.py"
        assert hasattr(so, name), f"{name} not exported by {lib.LIB_PATH}"
    assert not hasattr(so, "ull_attention_kv8_f16"), "the fp8 KV cache is a bf16-only feature"


def test_kv_cache_constructor_refusals():
    MC = pkg("modeling_core")
    with pytest.raises(ValueError, match="unknown KV cache dtype"):
        MC.KVCache(2, 1, 2, 16, 64, "cpu", kv_dtype="fp8_e5m2")
    with pytest.raises(ValueError, match="unknown KV cache dtype"):
        MC.KVCache(2, 1, 2, 16, 64, "cpu", kv_dtype=torch.float8_e4m3fn)
    for dt in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="bf16 model"):
            MC.KVCache(2, 1, 2, 16, 64, "cpu", dtype=dt, kv_dtype="fp8_e4m3")


def test_fp8_cache_layout_and_bytes():
    MC = pkg("modeling_core")
    c = MC.KVCache(3, 2, 4, 32, 100, "cpu", kv_dtype="fp8_e4m3")
    ref = MC.KVCache(3, 2, 4, 32, 100, "cpu")
    assert c.smax == ref.smax == 128 and len(c) == len(ref) == 3 and not c
    assert c.k8[0].shape == (2, 4, 128, 32) and c.k8[0].dtype == torch.uint8
    assert c.vt8[0].shape == (2, 4, 32, 128) and c.k_scale[0].shape == c.vt_scale[0].shape == (2, 4, 128)
    assert c.k_stage.shape == (2, 4, 128, 32) and c.vt_stage.shape == (2, 4, 32, 128)
    assert ref.kv_dtype is None and ref.dequantized() is ref
    # codes + scales + one staging window shared by the layers against the bf16 K and V^T
    assert c.nbytes() == 3 * 2 * (2 * 4 * 128 * 32 + 2 * 4 * 128 * 4) + 2 * 2 * (2 * 4 * 128 * 32)
    assert ref.nbytes() == 3 * 2 * 2 * (2 * 4 * 128 * 32)


def test_generate_refuses_bad_kv_cache_dtype_before_device_work():
    m = _tiny_core()
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="unknown KV cache dtype"):
        m.generate(input_ids=ids, max_new_tokens=2, use_cache=True, kv_cache_dtype="int8")
    with pytest.raises(ValueError, match="use_cache=True"):
        m.generate(input_ids=ids, max_new_tokens=2, use_cache=False, kv_cache_dtype="fp8_e4m3")
    for dt in (torch.float16, torch.float32):
        with pytest.raises(NotImplementedError, match="bf16 model"):
            _tiny_core(dt).generate(input_ids=ids, max_new_tokens=2, use_cache=True, kv_cache_dtype="fp8_e4m3")
