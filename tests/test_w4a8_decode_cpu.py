"""No GPU: MXFP8 activations in batched decode steps on mxfp4 weights (quantize_weights("mxfp4", decode_activations="mxfp8_e4m3"), DESIGN f20)
-- the two exported entries and their refusals, the "w4a8_skinny" route of the dispatch rule (ops.linear_route under
ActQuant(decode_fmt="mxfp8_e4m3")), and the argument validation of decode_activations.  The arithmetic is the definition restated in
tests/test_w4a8_cpu.py (w4a8_exact); the GPU tests are in tests/test_w4a8_decode_gpu.py."""
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core
from test_host_cpu import RULE_MS, RULE_NK, _written_linear_route
from test_w4a8_cpu import _meta_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
GEMM, NORMQ = "ull_gemm_skinny_w4a8_bf16", "ull_rmsnorm_quantize_rows_mxfp8_bf16"
LLAMA_7B = ((12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008))     # q|k|v, o_proj, gate|up, down_proj


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_both_entries_without_an_f16_twin():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for entry in (GEMM, NORMQ):
        assert re.search(r"^int " + entry + r"\(", header, flags=re.M), entry
        assert entry in L.SIGNATURES and hasattr(lib, entry), entry
        twin = entry[:-4] + "f16"
        assert twin not in header and twin not in L.SIGNATURES and not hasattr(lib, twin), "W4A8 is a bf16-only feature"
    assert "w4a8_decode.hip" in open(os.path.join(ROOT, "u-llava_amd", "csrc", "Makefile")).read()
    assert L.DEFINES["ULL_ROUTE_W4A8_SKINNY"] == 7 and L.DEFINES["ULL_W4A8_SKINNY_MAX_M"] == 32
    assert re.search(r"^#define ULL_ROUTE_W4A8_SKINNY 7\b", header, flags=re.M)


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=128, xs=_ADDR, ldxs=4, Q=_ADDR, ldq=64, ws=_ADDR, lds=4, C=_ADDR, ldc=64, R=None, ldr=0, M=16, N=64, K=128, flags=0):
    return getattr(pkg("_lib").load(), GEMM)(Xq, ldxq, xs, ldxs, Q, ldq, ws, lds, C, ldc, R, ldr, M, N, K, flags, None)


def test_gemm_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(M=33) == ERR_SHAPE, "two 16-row activation fragments at the most"
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_BIAS, ops.EPI_QGELU, ops.EPI_GELU, ops.EPI_RELU, ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    assert _rc(K=64, ldxq=64, ldq=32) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=192, ldxq=192, ldq=96, ldxs=8, lds=8) == ERR_SHAPE
    assert _rc(ldxq=136) == ERR_SHAPE and _rc(ldq=72) == ERR_SHAPE, "code pitches are multiples of 16 bytes"
    assert _rc(ldxq=112) == ERR_SHAPE and _rc(ldq=48) == ERR_SHAPE, "a code pitch below the row"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(ldxs=6) == ERR_SHAPE and _rc(lds=5) == ERR_SHAPE and _rc(xs=_ADDR + 2) == ERR_SHAPE and _rc(ws=_ADDR + 1) == ERR_SHAPE
    assert _rc(K=256, ldxq=256, ldq=128, ldxs=4, lds=8) == ERR_SHAPE and _rc(K=256, ldxq=256, ldq=128, ldxs=8, lds=4) == ERR_SHAPE, \
        "a scale pitch below K / 32"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"


def _rcn(X=_ADDR, ldx=128, w=_ADDR, eps=1e-6, M=4, K=128, codes=_ADDR, ldq=128, scales=_ADDR, lds=4):
    return getattr(pkg("_lib").load(), NORMQ)(X, ldx, w, eps, M, K, codes, ldq, scales, lds, None)


def test_norm_quantize_entry_refuses_bad_arguments_without_launching():
    for null in ("X", "w", "codes", "scales"):
        assert _rcn(**{null: None}) == ERR_ARG, null
    assert _rcn(M=0) == ERR_ARG and _rcn(K=0) == ERR_ARG
    assert _rcn(K=120, ldx=128) == ERR_SHAPE and _rcn(K=48, ldx=48, ldq=48) == ERR_SHAPE, "K must be a multiple of 32"
    assert _rcn(ldx=129) == ERR_SHAPE and _rcn(ldq=129) == ERR_SHAPE, "an odd row pitch"
    assert _rcn(ldx=120) == ERR_SHAPE and _rcn(ldq=120) == ERR_SHAPE, "a row pitch below K"
    assert _rcn(lds=0) == ERR_SHAPE and _rcn(K=256, ldx=256, ldq=256, lds=4) == ERR_SHAPE, "a scale pitch below K / 32"
    assert _rcn(lds=6) == ERR_SHAPE and _rcn(lds=5) == ERR_SHAPE, "the scale rows are what the GEMM reads: pitch % 4"
    assert _rcn(X=_ADDR + 2) == ERR_SHAPE and _rcn(codes=_ADDR + 4) == ERR_SHAPE and _rcn(scales=_ADDR + 2) == ERR_SHAPE, "aligned rows"


# ---- the routing rule -----------------------------------------------------------------------------------------------------------------
def _modes(ops):
    """Every ActQuant that carries decode_fmt="mxfp8_e4m3": any prefill format, either value of the fp8 scope flag."""
    return [ops.ActQuant(fmt, dec, "mxfp8_e4m3") for fmt in (None, "mxfp8_e4m3", "mxfp4_e2m1") for dec in (False, True)]


def test_truth_table_of_the_w4a8_skinny_route():
    ops = pkg("ops")
    assert "w4a8_skinny" in ops.A8_ROUTES and "w4a8_skinny" in ops._ROUTES.values()
    assert ops.ActQuant("mxfp8_e4m3").decode_fmt is None and ops.ActQuant._fields == ("fmt", "decode", "decode_fmt")
    w = _meta_mx(4096, 4096)
    for aq in _modes(ops):
        assert [M for M in range(0, 70) if ops.linear_route(M, w, aq) == "w4a8_skinny"] == list(range(5, 33)), aq
        assert all(ops._linear_route(M, 4096, 4096, w.route_pitch, 0, "mxfp4", aq) == ("w4a8_skinny", False) for M in range(5, 33)), \
            "the route fuses the norm"
        for N, K in LLAMA_7B:
            q = _meta_mx(N, K)
            assert [M for M in range(0, 70) if ops.linear_route(M, q, aq) == "w4a8_skinny"] == list(range(5, 33)), (aq, N, K)
        # outside 5 .. 32 rows the answer is the one without the decode format
        plain = None if aq.fmt is None else ops.ActQuant(aq.fmt, aq.decode)
        for M in list(range(0, 5)) + list(range(33, 70)):
            assert ops.linear_route(M, w, aq) == ops.linear_route(M, w, plain), (aq, M)
    aq = ops.ActQuant(None, False, "mxfp8_e4m3")
    assert ops.w4a8_decode_takes(8, 4096, 4096, w) and not ops.w4a8_decode_takes(4, 4096, 4096, w)
    # N * K just below and at 2^22
    assert ops.linear_route(8, _meta_mx(2047, 2048), aq) != "w4a8_skinny" and ops.linear_route(8, _meta_mx(2048, 2048), aq) == "w4a8_skinny"
    assert ops.linear_route(8, _meta_mx(32768 - 256, 128), aq) != "w4a8_skinny" and ops.linear_route(8, _meta_mx(32768, 128), aq) == "w4a8_skinny"
    # K = 4096 + 64: a multiple of 32 (the W4A16 skinny kernel takes it) but no whole number of 128-code K-tiles
    assert ops.linear_route(8, _meta_mx(4096, 4096 + 64), aq) == "skinny"
    assert ops.linear_route(20, _meta_mx(4096, 4096 + 64), aq) == "gemm"
    # a forced GEMM form keeps the Linear off the route
    assert ops._linear_route(8, 4096, 4096, w.route_pitch, ops.GEMM_TUNE_WAVES8, "mxfp4", aq)[0] != "w4a8_skinny"
    # only mxfp4 weights: an fp8 or a 16-bit weight never takes it
    f8 = ops.Fp8Weight(torch.empty(4096, 4096, dtype=torch.uint8, device="meta"), torch.empty(4096, dtype=torch.float32, device="meta"))
    bf = torch.empty(4096, 4096, dtype=BF, device="meta")
    for mode in _modes(ops):
        for M in range(0, 70):
            assert ops.linear_route(M, f8, mode) == ops.linear_route(M, f8, ops.ActQuant(mode.fmt, mode.decode)) != "w4a8_skinny"
            assert ops.linear_route(M, bf, mode) == ops.linear_route(M, bf) != "w4a8_skinny"
    assert all(ops.linear_route(M, f8, ops.ActQuant("fp8_e4m3", False, "mxfp8_e4m3")) in ("gemv", "skinny", "a8w8") for M in range(0, 70))


def test_every_answer_without_a_decode_format_is_unchanged():
    """decode_fmt=None: the rule as it was (tests/test_host_cpu.py's written form), over that file's shapes, with the three-field ActQuant."""
    ops = pkg("ops")
    modes = (None, ops.ActQuant("fp8_e4m3"), ops.ActQuant("fp8_e4m3", True), ops.ActQuant("mxfp8_e4m3"), ops.ActQuant("mxfp8_e4m3", True),
             ops.ActQuant("mxfp8_e4m3", True, None), ops.ActQuant("fp8_e4m3", True, None))
    for N, K in RULE_NK:
        for M in RULE_MS:
            for ldw in (K, K + 8, K + 4):
                for wfmt in (None, "fp8", "mxfp4"):
                    for aq in modes:
                        got = ops._linear_route(M, N, K, ldw, 0, wfmt, aq)
                        assert got == _written_linear_route(M, N, K, ldw, 0, wfmt, aq), (M, N, K, ldw, wfmt, aq)
                        assert got[0] != "w4a8_skinny"


# ---- decode_activations: signature and argument validation (before any device work) ---------------------------------------------------------
def test_signature_and_default_attribute():
    M, U, ops = pkg("modeling_core"), pkg("modeling_ullava"), pkg("ops")
    for cls in (M.UllavaCoreForCausalLM, U.UllavaForCausalLM):
        params = inspect.signature(cls.quantize_weights).parameters
        assert list(params) == ["self", "fmt", "activations", "activation_scope", "decode_activations"]
        assert params["decode_activations"].default is None and params["activation_scope"].default == "prefill"
        assert "decode_activations" in cls.quantize_weights.__doc__
    assert _tiny_core().decode_activation_quantization is None
    p = inspect.signature(ops.linear_w4a8_skinny).parameters
    assert list(p) == ["xq", "xsc", "w", "residual", "swiglu", "out", "out_f32"]
    assert p["residual"].default is None and p["swiglu"].default is False and p["out"].default is None and p["out_f32"].default is False
    assert list(inspect.signature(ops.rmsnorm_quantize_rows_mxfp8).parameters) == ["x", "w", "eps"]


def _untouched(model):
    return (model.weight_quantization is None and model.activation_quantization is None and model.activation_scope == "prefill"
            and model.decode_activation_quantization is None)


def test_unknown_decode_format_is_refused():
    model = _tiny_core()
    for bad in ("fp8_e4m3", "mxfp4_e2m1", "int8", True):
        with pytest.raises(ValueError, match="decode activation"):
            model.quantize_weights("mxfp4", decode_activations=bad)
    assert _untouched(model)


def test_decode_activations_on_fp8_weights_name_fp8s_spelling():
    model = _tiny_core()
    with pytest.raises(ValueError, match=r'activation_scope="prefill\+decode"'):
        model.quantize_weights("fp8_e4m3", decode_activations="mxfp8_e4m3")
    with pytest.raises(ValueError, match=r'activation_scope="prefill\+decode"'):
        model.quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="prefill+decode", decode_activations="mxfp8_e4m3")
    assert _untouched(model)


def test_mxfp4_scope_refusal_points_to_the_new_keyword():
    model = _tiny_core()
    with pytest.raises(NotImplementedError, match="mxfp4") as e:
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3", activation_scope="prefill+decode")
    assert "decode_activations='mxfp8_e4m3'" in str(e.value)
    assert _untouched(model)


def test_k_that_cannot_be_tiled_or_padded_is_refused_before_device_work():
    model = _tiny_core()
    model.config.hidden_size = 4096 + 64                        # (only the check reads it: the model never reaches the device)
    with pytest.raises(NotImplementedError, match="128"):
        model.quantize_weights("mxfp4", decode_activations="mxfp8_e4m3")
    assert _untouched(model)


@pytest.mark.parametrize("activations", [None, "mxfp8_e4m3", "mxfp4_e2m1"])
def test_mxfp4_with_decode_activations_passes_the_format_checks(activations):
    model = _tiny_core()
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        model.quantize_weights("mxfp4", activations=activations, decode_activations="mxfp8_e4m3")
    assert _untouched(model)
