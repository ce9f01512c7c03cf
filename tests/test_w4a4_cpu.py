"""CPU: MXFP4 activations on MXFP4 weights (quantize_weights("mxfp4", activations="mxfp4_e2m1"), ops.linear_w4a4 / ull_gemm_w4a4_bf16).

The definition of include/ullava_hip.h restated in float64 on the CPU, for x [M, K] @ w.T on an MXFP4 weight (codes e2m1, scales 2^s[n, j],
j the blocks of 32 consecutive K elements):
  1. t[m, j] = the smallest integer with amax|x[m, block j]| * 2^-t <= 6 (all-zero block: 0), clamped to [-125, 126], stored as t + 127;
     xq = e2m1(x * 2^-t), round to nearest, ties to the even code (at t = 126 saturating at the code of 3)     -- mxfp4_rows_reference
  2. y[m, n] = sum_j 2^(t[m, j] + s[n, j]) * sum_{k in j} e2m1(xq[m, k]) * e2m1(wq[n, k])                      -- w4a4_exact (fp64)
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
from test_w4a8_cpu import _meta_mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
ENTRIES = ("ull_quantize_act_rows_mxfp4_bf16", "ull_gemm_w4a4_bf16")
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def mxfp4_rows_reference(x: torch.Tensor):
    """(codes uint8 [M, K / 2], E8M0 bytes uint8 [M, K / 32]) of bf16 rows x [M, K], K % 32 == 0, standard layout.  Written from the rule
    itself, not from the weights' restatement: t by exact comparison against 6 * 2^t, the code as the nearest of the eight e2m1 values in
    float64 with a tie going to the even code."""
    M, K = x.shape
    b = x.double().view(M, K // 32, 32)
    amax = b.abs().amax(-1)
    t = torch.zeros_like(amax)
    nz = amax > 0
    t[nz] = torch.ceil(torch.log2(amax[nz] / 6.0))
    for _ in range(2):                                   # settle the rounding of log2 exactly
        t = torch.where(nz & (amax > 6.0 * torch.pow(2.0, t)), t + 1, t)
        t = torch.where(nz & (amax <= 6.0 * torch.pow(2.0, t - 1)), t - 1, t)
    t = t.clamp(-125, 126)
    a = (b * torch.pow(2.0, -t)[..., None]).abs()        # exact: a power of two times a bf16 value
    d = (a[..., None] - E2M1).abs()                      # distance to each e2m1 value: exact in float64
    best = d.amin(-1, keepdim=True)
    cand = d == best                                     # one code, or the two neighbours of a tie
    idx = torch.arange(8)
    lo = torch.where(cand, idx, 8).amin(-1)
    hi = torch.where(cand, idx, -1).amax(-1)
    mag = torch.where(lo % 2 == 0, lo, hi)               # neighbours differ by one: exactly one of them is even
    mag = torch.where(t[..., None] == 126, mag.clamp(max=5), mag)
    sign = torch.signbit(x.float()).view(M, K // 32, 32).long()
    code = (mag | (sign << 3)).view(M, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), (t + 127).to(torch.uint8)


def w4a4_exact(x: torch.Tensor, w_codes: torch.Tensor, w_scales: torch.Tensor):
    """(y, sum of |terms|) in float64 for bf16 x [M, K] and an MXFP4 weight in the STANDARD layout (codes [N, K / 2], scales [N, K / 32]).
    Every term 2^(t + s) * xq * wq is exact in float64, so y is the definition's value whatever the order."""
    xd = mxfp4_dequant_reference(*mxfp4_rows_reference(x)).double()
    wd = mxfp4_dequant_reference(w_codes, w_scales).double()
    return xd @ wd.T, xd.abs() @ wd.abs().T


def _nibbles(codes: torch.Tensor) -> torch.Tensor:
    return torch.stack((codes & 15, codes >> 4), dim=-1).view(codes.shape[0], -1)


# ---- the activation quantizer -----------------------------------------------------------------------------------------------------------
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
TIES_TO_CODE = [0, 2, 2, 4, 4, 6, 6]                      # each tie goes to the even code: 0, 1, 1, 2, 2, 4, 4


def special_rows() -> torch.Tensor:
    """bf16 [9, 96]: three blocks per row with the edge cases of the rule."""
    x = torch.zeros(9, 96)
    g = torch.Generator().manual_seed(3)
    x[0] = torch.randn(96, generator=g)
    x[1, 32:64] = torch.randn(32, generator=g) * 100.0           # blocks 0 and 2 all zero
    x[2, :32] = torch.randn(32, generator=g).clamp(-1, 1) * 6.0
    x[2, 5] = 6.0                                                 # amax exactly 6: t = 0
    x[2, 32:64] = torch.randn(32, generator=g).clamp(-1, 1) * 48.0
    x[2, 40] = -48.0                                              # amax exactly 6 * 2^3: t = 3
    x[2, 64:] = torch.randn(32, generator=g).clamp(-1, 1) * 6.0 / 16
    x[2, 70] = 6.0 / 16                                           # amax exactly 6 * 2^-4: t = -4
    x[3, 17] = 3.0                                                # one element in the block: 3 = 6 * 2^-1
    x[3, 95] = -2.0 ** -20                                        # 2^-20 = 4 * 2^-22: t = -22, code of -4
    x[4, 0] = 6.0 * (1 + 2.0 ** -7)                               # the next bf16 above 6: t = 1
    x[4, 32] = 48.0 * (1 + 2.0 ** -7)                             # ... above 6 * 2^3: t = 4
    x[4, 64] = 6.0 / 16 * (1 + 2.0 ** -7)                         # ... above 6 * 2^-4: t = -3
    x[5, 0] = 6.0                                                 # every tie and its negative beside a 6 (t = 0), a negative zero
    x[5, 1:8] = torch.tensor(TIES)
    x[5, 8:15] = -torch.tensor(TIES)
    x[5, 15] = -0.0
    x[5, 16] = -0.125                                             # rounds to -0
    x[5, 32] = 12.0                                               # the same ties one scale up (t = 1)
    x[5, 33:40] = 2 * torch.tensor(TIES)
    x[6, 0] = 2.0 ** -130                                         # bf16 subnormals under the clamp: t = -125
    x[6, 1] = -(2.0 ** -127)                                      # 0.25 at t = -125: a tie, to -0
    x[6, 2] = 2.0 ** -126                                         # 0.5
    x[6, 3] = 3 * 2.0 ** -128                                     # 0.375 -> 0.5
    x[6, 32] = 2.0 ** -133                                        # the smallest bf16 subnormal alone
    x[7] = torch.randn(96, generator=g) * 2.0 ** 100
    x[7, 0] = torch.finfo(BF).max                                 # the largest bf16 value: t = 126, saturating at the code of 3
    x[7, 1] = 2.0 ** 127
    x[7, 40] = -torch.finfo(BF).max
    x[8, ::2] = 0.07
    return x.to(BF)


def test_quantizer_restatement_on_special_blocks():
    x = special_rows()
    codes, sc = mxfp4_rows_reference(x)
    nib, t = _nibbles(codes), sc.int() - 127
    assert t[1].tolist()[0] == 0 and t[1].tolist()[2] == 0, "an all-zero block gets t = 0"
    assert not bool(nib[1, :32].any()) and not bool(nib[1, 64:].any())
    assert t[2].tolist() == [0, 3, -4], "amax exactly 6 * 2^j gives t = j"
    assert nib[2, 5] == 7 and nib[2, 40] == 15 and nib[2, 70] == 7, "... and the code of 6"
    assert t[3].tolist() == [-1, 0, -22] and nib[3, 17] == 7 and nib[3, 95] == 8 + 6 and int(nib[3].ne(0).sum()) == 2, "one element"
    assert t[4].tolist() == [1, 4, -3], "amax just above 6 * 2^j gives t = j + 1"
    assert nib[4, 0] == 5 and nib[4, 32] == 5 and nib[4, 64] == 5, "... where it rounds to 3"
    assert t[5].tolist()[:2] == [0, 1]
    assert nib[5, 1:8].tolist() == TIES_TO_CODE and nib[5, 8:15].tolist() == [8 + c for c in TIES_TO_CODE], "ties go to the even code"
    assert nib[5, 33:40].tolist() == TIES_TO_CODE
    assert nib[5, 15] == 8 and nib[5, 16] == 8, "negative zero keeps its sign, and -0.125 rounds to it"
    assert t[6].tolist() == [-125, -125, 0] and nib[6, :4].tolist() == [0, 8, 1, 1] and nib[6, 32] == 0, "subnormals under the clamp"
    assert t[7].tolist()[0] == 126 and nib[7, 0] == 5 and nib[7, 1] == 4 and t[7].tolist()[1] == 126 and nib[7, 40] == 8 + 5, "the largest bf16 value"
    # every block: amax * 2^-t <= 6 < amax * 2^-(t - 1) unless all zero or clamped, and the dequantized value is finite and within half a step
    b = x.double().view(9, 3, 32)
    amax = b.abs().amax(-1)
    free = (amax > 0) & (t > -125) & (t < 126)
    assert bool((amax * torch.pow(2.0, -t.double()) <= 6)[free].all()) and bool((amax * torch.pow(2.0, -(t.double() - 1)) > 6)[free].all())
    d = mxfp4_dequant_reference(codes, sc).double()
    assert bool(torch.isfinite(d).all())
    step = torch.pow(2.0, t.double()).repeat_interleave(32, 1)
    ok = (d - x.double()).abs() <= step
    ok[7] = True                                                   # (the saturating row)
    assert bool(ok.all())
    # the weights' restatement gives the same bytes: one rule for both operands
    wc, ws = mxfp4_reference(x)
    assert torch.equal(wc, codes) and torch.equal(ws, sc)
    g = torch.Generator().manual_seed(9)
    r = (torch.randn(64, 256, generator=g) * torch.pow(2.0, torch.randint(-20, 20, (64, 8), generator=g).float()).repeat_interleave(32, 1)).to(BF)
    assert all(torch.equal(a, b_) for a, b_ in zip(mxfp4_rows_reference(r), mxfp4_reference(r)))


def test_restatement_on_a_hand_checked_product():
    """K = 64: two blocks with different scales on both sides."""
    x = torch.zeros(2, 64)
    x[0, 0], x[0, 1], x[0, 33] = 6.0, 1.0, 3.0              # block 0: t = 0, codes 6 and 1; block 1: t = -1, code 6
    x[1, 40], x[1, 41] = -24.0, 5.0                          # block 1: t = 2: codes -6 and 1.25 -> 1 (a tie, to the even code): 4
    w = torch.zeros(3, 64)
    w[0, 0], w[0, 1], w[0, 33] = 6.0, 0.5, 1.5               # block 0: s = 0; block 1: 1.5 -> s = -2, code 6
    w[1, 40], w[1, 33], w[1, 41] = 12.0, 1.0, 2.0            # block 1: s = 1: codes 6, 0.5 and 1
    w[2, 1] = -0.25                                          # block 0: s = -4 (0.25 * 16 = 4 <= 6 < 8), code of -4
    wc, ws = mxfp4_reference(w.to(BF))
    assert (ws.int() - 127).tolist() == [[0, -2], [0, 1], [-4, 0]]
    xq, xt = mxfp4_rows_reference(x.to(BF))
    assert (xt.int() - 127).tolist() == [[0, -1], [0, 2]]
    assert _nibbles(xq)[0, [0, 1, 33]].tolist() == [7, 2, 7] and _nibbles(xq)[1, [40, 41]].tolist() == [15, 2]
    y, absum = w4a4_exact(x.to(BF), wc, ws)
    want = torch.tensor([[6 * 6 + 0.5 + 3 * 1.5, 3 * 1.0, -0.25], [0.0, -24.0 * 12 + 4.0 * 2, 0.0]], dtype=torch.float64)
    assert torch.equal(y, want)
    assert torch.equal(absum, torch.tensor([[41.0, 3.0, 0.25], [0.0, 296.0, 0.0]], dtype=torch.float64))


# ---- argument validation (before any device work) -------------------------------------------------------------------------------------
def test_signature_defaults_unchanged():
    M, U, ops = pkg("modeling_core"), pkg("modeling_ullava"), pkg("ops")
    for cls in (M.UllavaCoreForCausalLM, U.UllavaForCausalLM):
        p = inspect.signature(cls.quantize_weights).parameters
        assert p["activations"].default is None and p["fmt"].default == "fp8_e4m3" and p["activation_scope"].default == "prefill"
    assert _tiny_core().activation_quantization is None
    p = inspect.signature(ops.linear_w4a4).parameters
    assert list(p) == ["x", "w", "residual", "swiglu", "out", "out_f32"]
    assert p["residual"].default is None and p["swiglu"].default is False and p["out"].default is None and p["out_f32"].default is False
    assert list(inspect.signature(ops.quantize_rows_mxfp4).parameters) == ["x"]


def _untouched(model):
    return model.weight_quantization is None and model.activation_quantization is None


def test_mxfp4_with_mxfp4_activations_passes_the_format_checks():
    model = _tiny_core()
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        model.quantize_weights("mxfp4", activations="mxfp4_e2m1")
    assert _untouched(model)


def test_refusals_keep_their_errors_and_leave_the_model_alone():
    model = _tiny_core()
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("fp8_e4m3", activations="mxfp4_e2m1")
    assert _untouched(model)
    with pytest.raises(ValueError, match="activation.*mxfp4_e2m1"):
        model.quantize_weights("mxfp4", activations="int8")
    assert _untouched(model)
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("mxfp4", activations="mxfp4_e2m1", activation_scope="prefill+decode")
    assert _untouched(model)
    f16 = _tiny_core(torch.float16)
    with pytest.raises(NotImplementedError, match="bf16"):
        f16.quantize_weights("mxfp4", activations="mxfp4_e2m1")
    assert _untouched(f16)
    # the existing modes answer as before
    with pytest.raises(NotImplementedError, match="mxfp8_e4m3"):
        model.quantize_weights("fp8_e4m3", activations="mxfp8_e4m3")
    with pytest.raises(NotImplementedError, match="mxfp4"):
        model.quantize_weights("mxfp4", activations="fp8_e4m3")
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3")
    assert _untouched(model)


def test_k_that_cannot_be_tiled_or_padded_is_refused_before_device_work():
    model = _tiny_core()
    model.config.hidden_size = 4096 + 64                        # (only the check reads it: the model never reaches the device)
    with pytest.raises(NotImplementedError, match="128"):
        model.quantize_weights("mxfp4", activations="mxfp4_e2m1")
    assert _untouched(model)


# ---- the routing rule -----------------------------------------------------------------------------------------------------------------
def test_w4a4_is_taken_exactly_on_the_gemm_route():
    ops = pkg("ops")
    aq4, aq8 = ops.ActQuant("mxfp4_e2m1"), ops.ActQuant("mxfp8_e4m3")
    seen = set()
    for N, K in ((4096, 4096), (12288, 4096), (22016, 4096), (4096, 11008), (192, 64), (64, 128), (1000, 2048)):
        w = _meta_mx(N, K)
        for M in (1, 2, 3, 4, 5, 8, 16, 17, 26, 128, 643, 20576):
            route = ops._linear_route(M, N, K, w.route_pitch, 0)[0]          # the five-argument rule: the weight-only answer
            seen.add(route)
            got = ops.linear_route(M, w, aq4)
            assert (got == "w4a4") == (route == "gemm") and ops.w4a4_takes(M, N, K, w) == (route == "gemm"), (M, N, K, route, got)
            assert got == ("w4a4" if route == "gemm" else route), "elsewhere the weight-only answer"
            assert (ops.linear_route(M, w, aq8) == "w4a8") == (route == "gemm"), "MXFP8 activations on the same weight still answer w4a8"
            assert ops._linear_route(M, N, K, w.route_pitch, 0, "mxfp4", aq4)[1] == ops._linear_route(M, N, K, w.route_pitch, 0, "mxfp4", aq8)[1]
    assert seen == {"gemv", "skinny", "gemm"}
    bf = torch.empty(4096, 4096, dtype=BF, device="meta")
    f8 = ops.Fp8Weight(torch.empty(4096, 4096, dtype=torch.uint8, device="meta"), torch.empty(4096, dtype=torch.float32, device="meta"))
    for M in (1, 5, 17, 643, 20576):                             # only mxfp4 weights: a bf16 tensor or an fp8 weight never takes it
        assert ops.linear_route(M, bf, aq4) == ops.linear_route(M, bf) and ops.linear_route(M, f8, aq4) == ops.linear_route(M, f8)
        assert not ops.w4a4_takes(M, 4096, 4096, bf) and not ops.w4a4_takes(M, 4096, 4096, f8)
    assert "w4a4" in ops.A8_ROUTES and ops.linear_route(643, _meta_mx(4096, 4096), ops.ActQuant("mxfp4_e2m1", True)) == "w4a4"


# ---- the C entries --------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_entries_without_f16_twins():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    L = pkg("_lib")
    lib = L.load()
    for e in ENTRIES:
        assert re.search(r"^int " + e + r"\(", header, flags=re.M)
        assert e.replace("_bf16", "_f16") not in header
        assert e in L.SIGNATURES and hasattr(lib, e) and not hasattr(lib, e.replace("_bf16", "_f16"))
    assert re.search(r"^#define ULL_AF_MXFP4 3\b", header, flags=re.M) and re.search(r"^#define ULL_ROUTE_W4A4 6\b", header, flags=re.M)
    gen = open(os.path.join(ROOT, "tools", "gen_header_f16.py")).read()
    assert "w4a4" in gen, "the header generator must know the entry has no fp16 twin"


_ADDR = 0x10000                 # a non-null, 16-byte aligned address that is never dereferenced: every call returns from its argument checks
ERR_ARG, ERR_SHAPE = -1, -2


def _rc(Xq=_ADDR, ldxq=64, xs=_ADDR, ldxs=4, Q=_ADDR, ldq=64, ws=_ADDR, lds=4, C=_ADDR, ldc=64, R=None, ldr=0, M=32, N=64, K=128, flags=0):
    return pkg("_lib").load().ull_gemm_w4a4_bf16(Xq, ldxq, xs, ldxs, Q, ldq, ws, lds, C, ldc, R, ldr, M, N, K, flags, None)


def test_gemm_entry_refuses_bad_arguments_without_launching():
    ops = pkg("ops")
    for null in ("Xq", "xs", "Q", "ws", "C"):
        assert _rc(**{null: None}) == ERR_ARG, null
    assert _rc(M=0) == ERR_ARG and _rc(N=0) == ERR_ARG and _rc(K=0) == ERR_ARG
    assert _rc(flags=ops.EPI_RESID) == ERR_ARG, "residual flag without a residual"
    for bad in (ops.EPI_BIAS, ops.EPI_QGELU, ops.EPI_GELU, ops.EPI_RELU, ops.EPI_W_TILED, 128, ops.EPI_BIAS_ROUNDED, 1 << 20):
        assert _rc(flags=bad) == ERR_ARG, f"flag {bad} is not part of the contract"
    assert _rc(K=64, ldxq=32, ldq=32) == ERR_SHAPE, "K must be a multiple of 128"
    assert _rc(K=192, ldxq=96, ldq=96, ldxs=8, lds=8) == ERR_SHAPE
    assert _rc(ldxq=72) == ERR_SHAPE and _rc(ldq=72) == ERR_SHAPE, "code pitches are multiples of 16 bytes"
    assert _rc(ldxq=48) == ERR_SHAPE and _rc(ldq=48) == ERR_SHAPE, "a code pitch below the row"
    assert _rc(Xq=_ADDR + 8) == ERR_SHAPE and _rc(Q=_ADDR + 4) == ERR_SHAPE, "16-byte aligned codes"
    assert _rc(ldxs=6) == ERR_SHAPE and _rc(lds=5) == ERR_SHAPE and _rc(xs=_ADDR + 2) == ERR_SHAPE and _rc(ws=_ADDR + 1) == ERR_SHAPE
    assert _rc(K=256, ldxq=128, ldq=128, ldxs=4) == ERR_SHAPE and _rc(K=256, ldxq=128, ldq=128, ldxs=8, lds=4) == ERR_SHAPE, "a scale pitch below K / 32"
    assert _rc(flags=ops.EPI_SWIGLU, N=48) == ERR_SHAPE, "SwiGLU needs whole 32-row gate|up groups"
    assert _rc(ldc=63) == ERR_SHAPE and _rc(flags=ops.EPI_RESID, R=_ADDR, ldr=8) == ERR_SHAPE, "output / residual rows shorter than N"
    assert _rc(M=1 << 20, K=4096, ldxq=2048, ldq=2048, ldxs=128, lds=128) == ERR_SHAPE, "an activation operand of 2 GiB"
    assert _rc(N=1 << 20, K=4096, ldxq=2048, ldq=2048, ldxs=128, lds=128, ldc=1 << 20) == ERR_SHAPE, "a weight operand of 2 GiB"


def test_quantizer_entry_refuses_bad_arguments_without_launching():
    f = pkg("_lib").load().ull_quantize_act_rows_mxfp4_bf16
    ok = dict(X=_ADDR, ldx=64, M=4, K=64, codes=_ADDR, ldq=32, scales=_ADDR, lds=4, layout=1)

    def rc(**kw):
        a = dict(ok, **kw)
        return f(a["X"], a["ldx"], a["M"], a["K"], a["codes"], a["ldq"], a["scales"], a["lds"], a["layout"], None)
    for null in ("X", "codes", "scales"):
        assert rc(**{null: None}) == ERR_ARG
    assert rc(M=0) == ERR_ARG and rc(K=0) == ERR_ARG and rc(layout=2) == ERR_ARG and rc(layout=-1) == ERR_ARG
    assert rc(K=48, ldx=48, ldq=24) == ERR_SHAPE, "K % 32"
    assert rc(ldx=60) == ERR_SHAPE and rc(ldx=56) == ERR_SHAPE, "row pitch: 16-byte aligned rows, at least K"
    assert rc(ldq=28) == ERR_SHAPE and rc(ldq=34) == ERR_SHAPE and rc(lds=1) == ERR_SHAPE
    assert rc(X=_ADDR + 2) == ERR_SHAPE and rc(codes=_ADDR + 2) == ERR_SHAPE
