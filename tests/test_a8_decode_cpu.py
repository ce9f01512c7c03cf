"""No GPU: FP8 activations in batched decode steps (quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="prefill+decode"),
DESIGN f10) -- the two exported entries and their refusals, the "a8w8_skinny" route of the dispatch rule (ops.linear_route), and the argument validation of
activation_scope.  The arithmetic is the definition restated in tests/test_a8w8_cpu.py (a8w8_exact / a8w8_reference); the GPU tests are in
tests/test_a8_decode_gpu.py."""
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
GEMM, NORMQ = "ull_gemm_skinny_a8w8_bf16", "ull_rmsnorm_quantize_rows_fp8_bf16"


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_both_entries_without_an_f16_twin():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for entry in (GEMM, NORMQ):
        assert re.search(r"^int " + entry + r"\(", header, flags=re.M), entry
        assert entry in L.SIGNATURES and hasattr(lib, entry), entry
        twin = entry[:-4] + "f16"
        assert twin not in header and twin not in L.SIGNATURES and not hasattr(lib, twin), "fp8 activations are a bf16-only feature"
    assert "a8_decode.hip" in open(os.path.join(ROOT, "u-llava_amd", "csrc", "Makefile")).read()


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=128, xs=_ADDR, Q=_ADDR, ldq=128, ws=_ADDR, C=_ADDR, ldc=64, R=None, ldr=0, M=16, N=64, K=128, flags=0):
    return getattr(pkg("_lib").load(), GEMM)(Xq, ldxq, xs, Q, ldq, ws, C, ldc, R, ldr, M, N, K, flags, None)


def test_gemm_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(M=33) == ERR_SHAPE, "two 16-row activation fragments at the most"
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_BIAS, ops.EPI_QGELU, ops.EPI_GELU, ops.EPI_RELU, ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    assert _rc(K=192, ldxq=192, ldq=192) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=64, ldxq=64, ldq=64) == ERR_SHAPE
    assert _rc(ldxq=129) == ERR_SHAPE and _rc(ldq=129) == ERR_SHAPE, "an odd row pitch"
    assert _rc(ldxq=136) == ERR_SHAPE and _rc(ldq=136) == ERR_SHAPE, "row pitches are multiples of 16 bytes"
    assert _rc(ldxq=112) == ERR_SHAPE and _rc(ldq=112) == ERR_SHAPE, "a row pitch below K"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"


def _rcn(X=_ADDR, ldx=128, w=_ADDR, eps=1e-6, M=4, K=128, codes=_ADDR, ldq=128, scales=_ADDR):
    return getattr(pkg("_lib").load(), NORMQ)(X, ldx, w, eps, M, K, codes, ldq, scales, None)


def test_norm_quantize_entry_refuses_bad_arguments_without_launching():
    for null in ("X", "w", "codes", "scales"):
        assert _rcn(**{null: None}) == ERR_ARG, null
    assert _rcn(M=0) == ERR_ARG and _rcn(K=0) == ERR_ARG
    assert _rcn(K=124, ldx=128) == ERR_SHAPE, "K must be a multiple of 8"
    assert _rcn(ldx=129) == ERR_SHAPE and _rcn(ldq=129) == ERR_SHAPE, "an odd row pitch"
    assert _rcn(ldx=120) == ERR_SHAPE and _rcn(ldq=120) == ERR_SHAPE, "a row pitch below K"
    assert _rcn(X=_ADDR + 2) == ERR_SHAPE and _rcn(codes=_ADDR + 4) == ERR_SHAPE, "aligned rows"


# ---- the routing rule -----------------------------------------------------------------------------------------------------------------
def _fp8(N, K, pitch=None):
    ops = pkg("ops")
    codes = torch.empty(N, pitch or K, dtype=torch.uint8, device="meta")[:, :K]
    return ops.Fp8Weight(codes, torch.empty(N, dtype=torch.float32, device="meta"))


def test_truth_table_of_a8w8_decode_takes():
    ops = pkg("ops")

    def a8w8_decode_takes(M, N, K, w):                           # the one rule's answer under activation_scope="prefill+decode"
        assert tuple(w.shape) == (N, K)
        return ops.linear_route(M, w, ops.ActQuant("fp8_e4m3", decode=True)) == "a8w8_skinny"

    def a8w8_takes(M, N, K, w):                                  # ... and under the default scope
        assert tuple(w.shape) == (N, K)
        return ops.linear_route(M, w, ops.ActQuant("fp8_e4m3")) == "a8w8"

    w = _fp8(4096, 4096)
    assert [a8w8_decode_takes(M, 4096, 4096, w) for M in (4, 5, 16, 17, 32, 33)] == [False, True, True, True, True, False]
    assert [M for M in range(0, 70) if a8w8_decode_takes(M, 4096, 4096, w)] == list(range(5, 33))
    # N * K just below and at 2^22
    assert not a8w8_decode_takes(8, 2047, 2048, _fp8(2047, 2048))
    assert a8w8_decode_takes(8, 2048, 2048, _fp8(2048, 2048))
    assert not a8w8_decode_takes(8, 32768 - 256, 128, _fp8(32768 - 256, 128)) and a8w8_decode_takes(8, 32768, 128, _fp8(32768, 128))
    # K = 4096 + 64: a multiple of 32 (the W8A16 skinny kernel takes it) but no whole number of 128-code K-tiles
    K = 4096 + 64
    assert ops._linear_route(8, 4096, K, K, 0)[0] == "skinny" and not a8w8_decode_takes(8, 4096, K, _fp8(4096, K))
    # a row pitch the kernels cannot stream
    assert not a8w8_decode_takes(8, 4096, 4096, _fp8(4096, 4096, pitch=4100)) and a8w8_decode_takes(8, 4096, 4096, _fp8(4096, 4096, pitch=4104))
    # only fp8 weights
    assert not a8w8_decode_takes(8, 4096, 4096, torch.empty(4096, 4096, dtype=BF, device="meta"))
    mx = ops.Mxfp4Weight(torch.empty(4096, 2048, dtype=torch.uint8, device="meta"),
                         torch.empty(4096, ops.Mxfp4Weight.scale_pitch(4096), dtype=torch.uint8, device="meta"), 4096)
    assert not a8w8_decode_takes(8, 4096, 4096, mx) and ops.linear_route(8, mx, ops.ActQuant("mxfp8_e4m3", decode=True)) == "skinny"
    # the LLaMA-7B layer Linears are all on the rule, and it mirrors the skinny route at 5 .. 16 rows
    for N, K in ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)):
        for M in (5, 8, 16):
            assert ops._linear_route(M, N, K, K, 0)[0] == "skinny" and a8w8_decode_takes(M, N, K, _fp8(N, K))
        for M in (17, 32):
            assert a8w8_takes(M, N, K, _fp8(N, K)) and a8w8_decode_takes(M, N, K, _fp8(N, K))


# ---- activation_scope: argument validation (before any device work) -------------------------------------------------------------------------
def test_default_scope_and_signature():
    M, U = pkg("modeling_core"), pkg("modeling_ullava")
    for cls in (M.UllavaCoreForCausalLM, U.UllavaForCausalLM):
        params = inspect.signature(cls.quantize_weights).parameters
        assert params["activation_scope"].default == "prefill" and params["activations"].default is None
        assert list(params)[:4] == ["self", "fmt", "activations", "activation_scope"]
    assert _tiny_core().activation_scope == "prefill"


def test_unknown_scope_is_refused():
    model = _tiny_core()
    with pytest.raises(ValueError, match="scope"):
        model.quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="decode")
    assert model.weight_quantization is None and model.activation_quantization is None and model.activation_scope == "prefill"


def test_decode_scope_without_activations_is_refused():
    model = _tiny_core()
    with pytest.raises(ValueError, match="activations"):
        model.quantize_weights("fp8_e4m3", activation_scope="prefill+decode")
    assert model.weight_quantization is None and model.activation_scope == "prefill"


def test_decode_scope_on_mxfp4_is_refused_by_name():
    model = _tiny_core()
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3", activation_scope="prefill+decode")
    assert model.weight_quantization is None and model.activation_quantization is None and model.activation_scope == "prefill"
