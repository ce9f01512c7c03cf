"""CPU: MXFP8 activations on MXFP4 weights (quantize_weights("mxfp4", activations="mxfp8_e4m3"), ops.linear_w4a8 / ull_gemm_w4a8_bf16).

The definition of include/ullava_hip.h restated with torch on the CPU, for x [M, K] @ w.T on an MXFP4 weight (codes e2m1, scales 2^s[n, j],
j the blocks of 32 consecutive K elements):
  1. t[m, j] = the smallest integer with amax|x[m, block j]| * 2^-t <= 448 (all-zero block: 0), clamped to [-127, 127], stored as t + 127;
     xq = e4m3fn(x * 2^-t), round to nearest even (torch's CPU cast)                                       -- mxfp8_reference
  2. y[m, n] = sum_j 2^(t[m, j] + s[n, j]) * sum_{k in j} float(xq[m, k]) * e2m1(wq[n, k])                 -- w4a8_exact (fp64)
  3. the bf16 GEMM's epilogue on y.
"""
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core
from test_mxfp4_weights_cpu import mxfp4_dequant_reference, mxfp4_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
ENTRIES = ("ull_quantize_rows_mxfp8_bf16", "ull_gemm_w4a8_bf16")


def mxfp8_reference(x: torch.Tensor):
    """(codes uint8 [M, K], E8M0 bytes uint8 [M, K / 32]) of bf16 rows x [M, K], K % 32 == 0."""
    M, K = x.shape
    b = x.double().view(M, K // 32, 32)
    amax = b.abs().amax(-1)
    t = torch.zeros_like(amax)
    nz = amax > 0
    t[nz] = torch.ceil(torch.log2(amax[nz] / 448.0))
    for _ in range(2):                                   # settle the rounding of log2 exactly
        t = torch.where(nz & (amax > 448.0 * torch.pow(2.0, t)), t + 1, t)
        t = torch.where(nz & (amax <= 448.0 * torch.pow(2.0, t - 1)), t - 1, t)
    t = t.clamp(-127, 127)
    codes = (b * torch.pow(2.0, -t)[..., None]).float().to(torch.float8_e4m3fn).view(torch.uint8).view(M, K)
    return codes, (t + 127).to(torch.uint8)


def mxfp8_dequant(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """float64 [M, K]: float(code) * 2^(byte - 127) per block."""
    M, K = codes.shape
    v = codes.view(torch.float8_e4m3fn).double().view(M, K // 32, 32)
    return (v * torch.pow(2.0, scales.double() - 127)[..., None]).view(M, K)


def w4a8_exact(x: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor):
    """(y, sum of |terms|) in float64 for bf16 x [M, K] and an MXFP4 weight in the STANDARD layout (codes [N, K / 2], scales [N, K / 32]).
    Every term 2^(t + s) * xq * wq is exact in float64, so y is the definition's value whatever the order."""
    xd = mxfp8_dequant(*mxfp8_reference(x))
    wd = mxfp4_dequant_reference(w_codes, w_scales).double()
    return xd @ wd.T, xd.abs() @ wd.abs().T


# ---- the activation quantizer -----------------------------------------------------------------------------------------------------------
def special_rows() -> torch.Tensor:
    """bf16 [8, 96]: three blocks per row with the edge cases of the scale rule."""
    x = torch.zeros(8, 96)
    g = torch.Generator().manual_seed(3)
    x[0] = torch.randn(96, generator=g)
    x[1, 32:64] = torch.randn(32, generator=g) * 100.0           # blocks 0 and 2 all zero
    x[2, :32] = torch.randn(32, generator=g).clamp(-1, 1) * 448.0
    x[2, 5] = 448.0                                               # amax exactly 448: t = 0
    x[2, 32:64] = torch.randn(32, generator=g).clamp(-1, 1) * 448.0 * 8
    x[2, 40] = -448.0 * 8                                         # amax exactly 448 * 2^3: t = 3
    x[2, 64:] = torch.randn(32, generator=g).clamp(-1, 1) * 448.0 / 16
    x[2, 70] = 448.0 / 16                                         # amax exactly 448 * 2^-4: t = -4
    x[3, 17] = 3.0                                                # one element in the block
    x[3, 95] = -2.0 ** -20
    x[4, :32] = 449.0                                             # (bf16: 448) just the boundary again after rounding to bf16
    x[4, 32:64] = 452.0                                           # bf16 452 -> above 448: t = 1
    x[5] = torch.randn(96, generator=g) * 2.0 ** -100
    x[6] = torch.randn(96, generator=g) * 2.0 ** 100
    x[7, ::2] = 0.07
    return x.to(BF)


def test_quantizer_restatement_on_special_blocks():
    x = special_rows()
    codes, sc = mxfp8_reference(x)
    t = sc.int() - 127
    assert t[1].tolist()[0] == 0 and t[1].tolist()[2] == 0, "an all-zero block gets t = 0"
    assert not bool(codes[1, :32].any()) and not bool(codes[1, 64:].any())
    assert t[2].tolist() == [0, 3, -4], "amax exactly 448 * 2^j gives t = j"
    assert codes[2, 5] == 0x7E and codes[2, 40] == 0xFE and codes[2, 70] == 0x7E, "... and the code of 448"
    assert t[3].tolist() == [-7, 0, -28], "3 * 2^7 = 384 <= 448 < 768; 2^-20 * 2^28 = 256 <= 448 < 512"
    assert codes[3, 17] == 0x7C and codes[3, 95] == 0xF8                      # 384 = 1.5 * 2^8, -256
    assert t[4].tolist()[:2] == [0, 1]
    # every block: amax * 2^-t <= 448 < amax * 2^-(t - 1) unless all zero, and the dequantized value is within half an e4m3 ulp
    b = x.double().view(8, 3, 32)
    amax = b.abs().amax(-1)
    nz = amax > 0
    assert bool((amax * torch.pow(2.0, -t.double()) <= 448)[nz].all()) and bool((amax * torch.pow(2.0, -(t.double() - 1)) > 448)[nz].all())
    d = mxfp8_dequant(codes, sc)
    assert bool(((d - x.double()).abs() <= x.double().abs() * 2.0 ** -4 + torch.pow(2.0, t.double() - 10).repeat_interleave(32, 1)).all())
    # the same codes as the per-row fp8 rule applied to one block as a row
    from test_fp8_weights_cpu import fp8_reference
    rc, rs = fp8_reference(x.view(24, 32))
    assert torch.equal(rc.view(8, 96), codes) and torch.equal(torch.log2(rs).view(8, 3).int(), t)


def test_restatement_on_a_hand_checked_product():
    """K = 64: two blocks with different scales on both sides."""
    x = torch.zeros(2, 64)
    x[0, 0], x[0, 1], x[0, 33] = 448.0, 1.0, 3.0            # block 0: t = 0, codes 448 and 1; block 1: t = -7, 3 * 128 = 384
    x[1, 40] = -896.0                                        # block 1: t = 1, code -448
    w = torch.zeros(3, 64)
    w[0, 0], w[0, 1], w[0, 33] = 6.0, 0.5, 1.5               # block 0: s = 0; block 1: 1.5 -> s = -2, code 6
    w[1, 40], w[1, 33] = 12.0, 1.0                           # block 1: s = 1: codes 6 and 0.5
    w[2, 1] = -0.25                                          # block 0: s = -4 (0.25 * 16 = 4 <= 6 < 8), code of -4
    wc, ws = mxfp4_reference(w.to(BF))
    assert (ws.int() - 127).tolist() == [[0, -2], [0, 1], [-4, 0]]
    y, absum = w4a8_exact(x.to(BF), wc, ws)
    want = torch.tensor([[448 * 6 + 0.5 + 3 * 1.5, 3 * 1.0, -0.25], [0.0, -896.0 * 12, 0.0]], dtype=torch.float64)
    assert torch.equal(y, want)
    assert torch.equal(absum, want.abs())
    xq, xt = mxfp8_reference(x.to(BF))
    assert (xt.int() - 127).tolist() == [[0, -7], [0, 1]]


# ---- argument validation (before any device work) -------------------------------------------------------------------------------------
def test_signature_defaults_unchanged():
    M, U, ops = pkg("modeling_core"), pkg("modeling_ullava"), pkg("ops")
    for cls in (M.UllavaCoreForCausalLM, U.UllavaForCausalLM):
        p = inspect.signature(cls.quantize_weights).parameters
        assert p["activations"].default is None and p["fmt"].default == "fp8_e4m3"
    assert _tiny_core().activation_quantization is None
    p = inspect.signature(ops.linear_w4a8).parameters
    assert list(p) == ["x", "w", "residual", "swiglu", "out", "out_f32"]
    assert p["residual"].default is None and p["swiglu"].default is False and p["out"].default is None and p["out_f32"].default is False


def test_mxfp4_with_mxfp8_activations_passes_the_format_checks():
    model = _tiny_core()
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3")
    assert model.weight_quantization is None and model.activation_quantization is None


def test_fp8_weights_with_mxfp8_activations_are_refused():
    model = _tiny_core()
    with pytest.raises(NotImplementedError, match="mxfp8_e4m3"):
        model.quantize_weights("fp8_e4m3", activations="mxfp8_e4m3")
    assert model.weight_quantization is None and model.activation_quantization is None


def test_other_values_keep_their_errors():
    model = _tiny_core()
    with pytest.raises(ValueError, match="activation"):
        model.quantize_weights("mxfp4", activations="int8")
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("mxfp4", activations="fp8_e4m3")
    with pytest.raises(NotImplementedError, match="bf16"):
        _tiny_core(torch.float16).quantize_weights("mxfp4", activations="mxfp8_e4m3")
    assert model.weight_quantization is None and model.activation_quantization is None


def test_k_that_cannot_be_tiled_or_padded_is_refused_before_device_work():
    ops = pkg("ops")
    assert all(ops.w4a8_k_ok(K) for K in (32, 64, 96, 128, 192, 1920, 2048, 4096, 11008, 2048 + 384))
    assert not any(ops.w4a8_k_ok(K) for K in (1952, 2016, 2048 + 32, 4096 + 64, 11008 + 96))
    model = _tiny_core()
    model.config.hidden_size = 4096 + 64                        # (only the check reads it: the model never reaches the device)
    with pytest.raises(NotImplementedError, match="128"):
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3")


# ---- the routing rule -----------------------------------------------------------------------------------------------------------------
def _meta_mx(N, K):
    ops = pkg("ops")
    return ops.Mxfp4Weight(torch.empty(N, K // 2, dtype=torch.uint8, device="meta"),
                           torch.empty(N, ops.Mxfp4Weight.scale_pitch(K), dtype=torch.uint8, device="meta"), K)


def test_w4a8_is_taken_exactly_on_the_gemm_route():
    ops = pkg("ops")

    def w4a8_takes(M, N, K, w):                                  # the one rule's answers for the two activation formats (prefill scope)
        assert tuple(w.shape) == (N, K)
        return ops.linear_route(M, w, ops.ActQuant("mxfp8_e4m3")) == "w4a8"

    def a8w8_takes(M, N, K, w):                                  # (asked about a weight of another format: its own N, K)
        return ops.linear_route(M, w, ops.ActQuant("fp8_e4m3")) == "a8w8"
    seen = set()
    for N, K in ((4096, 4096), (12288, 4096), (22016, 4096), (4096, 11008), (192, 64), (64, 128), (1000, 2048)):
        w = _meta_mx(N, K)
        for M in (1, 2, 3, 4, 5, 8, 16, 17, 26, 128, 643, 20576):
            route = ops._linear_route(M, N, K, w.route_pitch, 0)[0]
            seen.add(route)
            assert w4a8_takes(M, N, K, w) == (route == "gemm"), (M, N, K, route)
    assert seen == {"gemv", "skinny", "gemm"}
    w = _meta_mx(4096, 4096)                                     # LLaMA-7B: decode steps (M <= 16) never, 17 rows and more always
    assert [M for M in range(1, 40) if w4a8_takes(M, 4096, 4096, w)] == list(range(17, 40))
    w = _meta_mx(192, 64)                                        # a small weight: the GEMV up to 4 rows, the GEMM from 5 on
    assert [M for M in range(1, 20) if w4a8_takes(M, 192, 64, w)] == list(range(5, 20))
    # only mxfp4 weights: a bf16 tensor or an fp8 weight never takes it
    assert not w4a8_takes(643, 4096, 4096, torch.empty(4096, 4096, dtype=BF, device="meta"))
    f8 = ops.Fp8Weight(torch.empty(4096, 4096, dtype=torch.uint8, device="meta"), torch.empty(4096, dtype=torch.float32, device="meta"))
    assert not w4a8_takes(643, 4096, 4096, f8) and not a8w8_takes(643, 4096, 4096, w)


# ---- the C entries --------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_entries_without_f16_twins():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for e in ENTRIES:
        assert re.search(r"^int " + e + r"\(", header, flags=re.M)
        assert e.replace("_bf16", "_f16") not in header
        assert e in L.SIGNATURES and hasattr(lib, e) and not hasattr(lib, e.replace("_bf16", "_f16"))
    assert "normal floats or zero" in header, "the header says which inputs the definition covers"
    gen = open(os.path.join(ROOT, "tools", "gen_header_f16.py")).read()
    assert "w4a8" in gen, "the header generator must know the entry has no fp16 twin"


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=128, xs=_ADDR, ldxs=4, Q=_ADDR, ldq=64, ws=_ADDR, lds=4, C=_ADDR, ldc=64, R=None, ldr=0, M=32, N=64, K=128, flags=0):
    return pkg("_lib").load().ull_gemm_w4a8_bf16(Xq, ldxq, xs, ldxs, Q, ldq, ws, lds, C, ldc, R, ldr, M, N, K, flags, None)


def test_gemm_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_BIAS, ops.EPI_QGELU, ops.EPI_GELU, ops.EPI_RELU, ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    assert _rc(K=64, ldxq=64, ldq=32) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=192, ldxq=192, ldq=96, ldxs=8, lds=8) == ERR_SHAPE
    assert _rc(ldxq=136) == ERR_SHAPE and _rc(ldq=72) == ERR_SHAPE, "code pitches are multiples of 16 bytes"
    assert _rc(ldxq=112) == ERR_SHAPE and _rc(ldq=48) == ERR_SHAPE, "a code pitch below the row"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(ldxs=6) == ERR_SHAPE and _rc(lds=5) == ERR_SHAPE and _rc(xs=_ADDR + 2) == ERR_SHAPE and _rc(ws=_ADDR + 1) == ERR_SHAPE
    assert _rc(K=256, ldxq=256, ldq=128, ldxs=4) == ERR_SHAPE and _rc(K=256, ldxq=256, ldq=128, ldxs=8, lds=4) == ERR_SHAPE, "a scale pitch below K / 32"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"
    assert _rc(M=1 << 20, K=4096, ldxq=4096, ldq=2048, ldxs=128, lds=128) == ERR_SHAPE, "operands of 2 GiB and more"


def test_quantizer_entry_refuses_bad_arguments_without_launching():
    f = pkg("_lib").load().ull_quantize_rows_mxfp8_bf16
    ok = dict(X=_ADDR, ldx=64, M=4, K=64, codes=_ADDR, ldq=64, scales=_ADDR, lds=4)

    def rc(**kw):
        a = dict(ok, **kw)
        return f(a["X"], a["ldx"], a["M"], a["K"], a["codes"], a["ldq"], a["scales"], a["lds"], None)
    for null in ("X", "codes", "scales"):
        assert rc(**{null: None}) == ERR_ARG
    assert rc(M=0) == ERR_ARG and rc(K=0) == ERR_ARG
    assert rc(K=48, ldx=48, ldq=48) == ERR_SHAPE, "K % 32"
    assert rc(ldx=60) == ERR_SHAPE and rc(ldx=56) == ERR_SHAPE and rc(ldq=56) == ERR_SHAPE and rc(ldq=68) == ERR_SHAPE and rc(lds=1) == ERR_SHAPE
    assert rc(lds=2) == ERR_SHAPE and rc(lds=6) == ERR_SHAPE and rc(scales=_ADDR + 2) == ERR_SHAPE, "the scale rows are what the GEMM reads: pitch % 4, 4-byte aligned"
    assert rc(X=_ADDR + 2) == ERR_SHAPE and rc(codes=_ADDR + 4) == ERR_SHAPE
