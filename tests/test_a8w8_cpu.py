"""No GPU: FP8 activations on FP8 weights (quantize_weights("fp8_e4m3", activations="fp8_e4m3"), DESIGN f8) -- argument validation, the
routing rule, the exported entry and its refusals, and the test's own fp64 restatement of the arithmetic that the GPU tests hold the
kernel to:

    xq, 2^t_m = per-row e4m3 quantization of x (the weights' rule: t the smallest integer with amax|x_m| * 2^-t <= 448, 0 for a zero row)
    acc[m, n] = sum_k float(xq[m, k]) * float(wq[n, k])
    y[m, n]   = acc[m, n] * 2^(t_m + s_n)
    then ull_gemm_bf16's epilogue on y (none / residual / SwiGLU on the gate|up interleave / fp32 output).
"""
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core, fp8_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
ENTRY = "ull_gemm_a8w8_bf16"


# ---- the fp64 restatement (the reference of tests/test_a8w8_gpu.py) ---------------------------------------------------------------------
def a8w8_exact(x: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor):
    """(y, bound_sum) in fp64 on the CPU for bf16 x [M, K] and an fp8 weight (codes uint8 [N, K], scales fp32 [N]):
    y = 2^(t_m + s_n) * sum_k xq * wq exactly as defined above, bound_sum = 2^(t_m + s_n) * sum_k |xq * wq| (for the accumulation bound)."""
    x_codes, x_scales = fp8_reference(x.cpu())
    xq = x_codes.view(torch.float8_e4m3fn).double()
    wq = w_codes.cpu().view(torch.float8_e4m3fn).double()
    sc = x_scales.double()[:, None] * w_scales.cpu().double()[None, :]
    return (xq @ wq.T) * sc, (xq.abs() @ wq.abs().T) * sc


def _rnd(t: torch.Tensor) -> torch.Tensor:
    return t.to(BF).double()


def a8w8_reference(x, w_codes, w_scales, residual=None, swiglu=False, out_f32=False) -> torch.Tensor:
    """The restatement with the epilogue's rounding points, computed from the exact y (so it is the result of a kernel whose fp32
    accumulation happens to be exact): bf16(y); residual: bf16(R + bf16(y)); swiglu (rows in 16-row gate / up groups):
    bf16(bf16(silu(bf16(gate))) * bf16(up)); out_f32 with no other flag: y itself as fp32."""
    y, _ = a8w8_exact(x, w_codes, w_scales)
    if swiglu:
        M, N = y.shape
        g = y.view(M, N // 32, 2, 16)
        gate, up = _rnd(g[:, :, 0].reshape(M, N // 2)), _rnd(g[:, :, 1].reshape(M, N // 2))
        y = _rnd(_rnd(gate * torch.sigmoid(gate)) * up)
    elif not (out_f32 and residual is None):
        y = _rnd(y)
    if residual is not None:
        y = _rnd(residual.cpu().double() + y)
    return y.float() if out_f32 else y.to(BF)


def test_restatement_on_hand_computed_2x2_cases():
    # row 0: amax 3 -> t = -7 (3 * 128 = 384 <= 448 < 768), codes 384, -128; row 1 all zero -> t = 0
    x = torch.tensor([[3.0, -1.0], [0.0, 0.0]]).to(BF)
    # row 0: amax 0.5 -> s = -9 (codes 256, 128); row 1: amax 1792 = 448 * 4 -> s = 2 (codes 448, 0)
    w = torch.tensor([[0.5, 0.25], [1792.0, 0.0]]).to(BF)
    wc, ws = fp8_reference(w)
    xc, xs = fp8_reference(x)
    assert xs.tolist() == [2.0 ** -7, 1.0] and ws.tolist() == [2.0 ** -9, 4.0]
    assert xc.view(torch.float8_e4m3fn).float().tolist() == [[384.0, -128.0], [0.0, 0.0]]
    y, ab = a8w8_exact(x, wc, ws)
    assert y.tolist() == [[3 * 0.5 - 0.25, 3 * 1792.0], [0.0, 0.0]]
    assert ab.tolist() == [[3 * 0.5 + 0.25, 3 * 1792.0], [0.0, 0.0]]
    assert a8w8_reference(x, wc, ws).tolist() == [[1.25, 5376.0], [0.0, 0.0]]
    r = torch.tensor([[0.5, 1.0], [2.0, -3.0]]).to(BF)
    assert a8w8_reference(x, wc, ws, residual=r).tolist() == [[1.75, 5376.0], [2.0, -3.0]]       # 5377 is not a bf16 value: ties to 5376
    assert a8w8_reference(x, wc, ws, out_f32=True).dtype == torch.float32
    # the activation cast rounds: 1.0625 is halfway between the e4m3 values 1.0 and 1.125 -> 1.0 (even), so y = 1 + 448, not 449.0625
    x2 = torch.tensor([[1.0625, 448.0], [448.0, 447.0]]).to(BF)                                  # (447 -> 448: bf16 has 8 significant bits)
    w2 = torch.tensor([[1.0, 1.0], [1.0, -1.0]]).to(BF)
    wc2, ws2 = fp8_reference(w2)
    assert ws2.tolist() == [2.0 ** -8, 2.0 ** -8]
    y2, _ = a8w8_exact(x2, wc2, ws2)
    assert y2.tolist() == [[449.0, -447.0], [896.0, 0.0]]
    assert a8w8_reference(x2, wc2, ws2, out_f32=True).tolist() == [[449.0, -447.0], [896.0, 0.0]]
    assert a8w8_reference(x2, wc2, ws2).tolist() == [[448.0, -448.0], [896.0, 0.0]]              # bf16(449) = 448 (tie to even), bf16(-447) = -448


def test_restatement_swiglu_interleave():
    """N = 32: rows 0..15 are gate rows, 16..31 up rows; output column c = silu(gate_c) * up_c with the three roundings."""
    K = 8
    x = torch.zeros(1, K)
    x[0, 0] = 1.0
    w = torch.zeros(32, K)
    w[:16, 0] = torch.arange(16.0) - 8          # gate_c = c - 8
    w[16:, 0] = 2.0                             # up_c = 2
    wc, ws = fp8_reference(w.to(BF))
    out = a8w8_reference(x.to(BF), wc, ws, swiglu=True)
    g = (torch.arange(16.0) - 8).double()
    want = ((g * torch.sigmoid(g)).to(BF).double() * 2.0).to(BF)
    assert out.shape == (1, 16) and torch.equal(out[0], want)


# ---- argument validation (before any device work) -------------------------------------------------------------------------------------
def test_default_is_off_and_signature():
    M, U = pkg("modeling_core"), pkg("modeling_ullava")
    for cls in (M.UllavaCoreForCausalLM, U.UllavaForCausalLM):
        assert inspect.signature(cls.quantize_weights).parameters["activations"].default is None
    assert _tiny_core().activation_quantization is None


def test_unknown_activation_format():
    model = _tiny_core()
    with pytest.raises(ValueError, match="activation"):
        model.quantize_weights("fp8_e4m3", activations="int8")
    assert model.weight_quantization is None and model.activation_quantization is None


def test_mxfp4_with_fp8_activations_is_refused():
    model = _tiny_core()
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("mxfp4", activations="fp8_e4m3")
    assert model.weight_quantization is None and model.activation_quantization is None


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_non_bf16_model_is_refused(dtype):
    model = _tiny_core(dtype)
    with pytest.raises(NotImplementedError, match="bf16"):
        model.quantize_weights("fp8_e4m3", activations="fp8_e4m3")
    assert model.weight_quantization is None and model.activation_quantization is None


# ---- the routing rule -----------------------------------------------------------------------------------------------------------------
def test_a8_is_taken_exactly_on_the_gemm_route():
    ops = pkg("ops")

    def a8w8_takes(M, N, K, w):                                  # the one rule's answer for an fp8-activation model (prefill scope)
        assert tuple(w.shape) == (N, K)
        return ops.linear_route(M, w, ops.ActQuant("fp8_e4m3")) == "a8w8"
    shapes = [(N, K) for N, K in ((4096, 4096), (12288, 4096), (22016, 4096), (4096, 11008), (192, 64), (64, 128), (1000, 2048))]
    seen = set()
    for N, K in shapes:
        w = ops.Fp8Weight(torch.empty(N, K, dtype=torch.uint8, device="meta"), torch.empty(N, dtype=torch.float32, device="meta"))
        for M in (1, 2, 3, 4, 5, 8, 16, 17, 26, 128, 643, 20576):
            route = ops._linear_route(M, N, K, w.route_pitch, 0)[0]
            seen.add(route)
            assert a8w8_takes(M, N, K, w) == (route == "gemm"), (M, N, K, route)
    assert seen == {"gemv", "skinny", "gemm"}
    # the LLaMA-7B shapes: decode steps never, 17 rows and more always
    w = ops.Fp8Weight(torch.empty(4096, 4096, dtype=torch.uint8, device="meta"), torch.empty(4096, dtype=torch.float32, device="meta"))
    assert [M for M in range(1, 40) if a8w8_takes(M, 4096, 4096, w)] == list(range(17, 40))
    # only fp8 weights: a bf16 tensor or an mxfp4 weight never takes it
    assert not a8w8_takes(643, 4096, 4096, torch.empty(4096, 4096, dtype=BF, device="meta"))


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_entry_without_an_f16_twin():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    assert re.search(r"^int " + ENTRY + r"\(", header, flags=re.M)
    assert "ull_gemm_a8w8_f16" not in header
    L = pkg("_lib")
    lib = L.load()
    assert ENTRY in L.SIGNATURES and hasattr(lib, ENTRY)
    assert not hasattr(lib, "ull_gemm_a8w8_f16"), "fp8 activations are a bf16-only feature"
    gen = open(os.path.join(ROOT, "tools", "gen_header_f16.py")).read()
    assert "a8w8" in gen, "the header generator must know the entry has no fp16 twin"


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=128, xs=_ADDR, Q=_ADDR, ldq=128, ws=_ADDR, C=_ADDR, ldc=64, R=None, ldr=0, M=32, N=64, K=128, flags=0):
    return getattr(pkg("_lib").load(), ENTRY)(Xq, ldxq, xs, Q, ldq, ws, C, ldc, R, ldr, M, N, K, flags, None)


def test_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_BIAS, ops.EPI_QGELU, ops.EPI_GELU, ops.EPI_RELU, ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    assert _rc(K=64, ldxq=64, ldq=64) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=192, ldxq=192, ldq=192) == ERR_SHAPE
    assert _rc(ldxq=136) == ERR_SHAPE and _rc(ldq=136) == ERR_SHAPE, "row pitches are multiples of 16 bytes"
    assert _rc(ldxq=112) == ERR_SHAPE and _rc(ldq=112) == ERR_SHAPE, "a row pitch below K"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"
