"""GPU: ops.linear(..., act_quant=) carries out what the dispatch rule decides -- at the smallest shapes that reach each activation-quantized
route it equals the direct calls of the per-kernel wrappers (ops.linear_a8w8 / ops.linear_w4a8 / ops.linear_a8w8_skinny) bit for bit, with
the same launches; outside those routes it is ops.linear without act_quant; arguments no A8 kernel has are refused by name."""
import pytest
import torch

from helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
EPS = 1e-6


def _data(M, N, K, seed):
    """x [M, K], a weight [N, K] small enough that SiLU of a gate column stays finite, an RMSNorm weight [K], residuals [M, N] and [M, N / 2]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(BF).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(DEV)
    rms = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF).to(DEV)
    return x, w, rms, torch.randn(M, N, generator=g).to(BF).to(DEV), torch.randn(M, N // 2, generator=g).to(BF).to(DEV)


def _names(monkeypatch):
    L = pkg("_lib")
    names, real = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *a: names.append(name) or real(name, *a))
    return names


def _same(names, got_fn, want_fn):
    """Both calls give the same bits through the same launches."""
    del names[:]
    got = got_fn()
    n_got = list(names)
    del names[:]
    want = want_fn()
    assert n_got == names, (n_got, names)
    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    assert bool(torch.isfinite(got.float()).all()) and bool(got.float().abs().sum() > 0)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_gemm_routes_equal_the_direct_call(monkeypatch, fmt):
    """M = 26, N = 192, K = 64: the A8 GEMM of the weight's format, K padded to 128 (the copy kept on the weight, padded scale bytes for mxfp4)."""
    ops = pkg("ops")
    M, N, K = 26, 192, 64
    x, w, rms, r, r2 = _data(M, N, K, 1)
    if fmt == "fp8":
        q, aq, route, direct = ops.quantize_fp8(w), ops.ActQuant("fp8_e4m3"), "a8w8", ops.linear_a8w8
    else:
        q, aq, route, direct = ops.quantize_mxfp4(w), ops.ActQuant("mxfp8_e4m3"), "w4a8", ops.linear_w4a8
    assert ops.linear_route(M, q, aq) == route and ops.linear_route(M, q, None) == "gemm"
    names = _names(monkeypatch)
    with torch.no_grad():
        _same(names, lambda: ops.linear(x, q, act_quant=aq), lambda: direct(x, q))
        assert q._kpad is not None
        _same(names, lambda: ops.linear(x, q, rms_w=rms, rms_eps=EPS, act_quant=aq), lambda: direct(ops.rmsnorm(x, rms, EPS), q))
        _same(names, lambda: ops.linear(x, q, residual=r, act_quant=aq), lambda: direct(x, q, residual=r))
        _same(names, lambda: ops.linear(x, q, swiglu=True, act_quant=aq), lambda: direct(x, q, swiglu=True))       # (the rows as a gate|up pack)
        _same(names, lambda: ops.linear(x, q, rms_w=rms, rms_eps=EPS, residual=r2, swiglu=True, out_f32=True, act_quant=aq),
              lambda: direct(ops.rmsnorm(x, rms, EPS), q, residual=r2, swiglu=True, out_f32=True))
        out = torch.empty(M, N, device=DEV, dtype=BF)
        assert ops.linear(x, q, out=out, act_quant=aq).data_ptr() == out.data_ptr() and torch.equal(out, direct(x, q))
        # the other format's mode is no pair for this weight: weight-only
        other = ops.ActQuant("mxfp8_e4m3" if fmt == "fp8" else "fp8_e4m3")
        _same(names, lambda: ops.linear(x, q, rms_w=rms, rms_eps=EPS, act_quant=other), lambda: ops.linear(x, q, rms_w=rms, rms_eps=EPS))


def test_decode_scope_routes_equal_the_direct_calls(monkeypatch):
    """N = K = 2048 (N * K = 2^22) under decode=True: 8 and 32 rows take the W8A8 skinny kernel with the RMSNorm inside the row quantization;
    4 rows are the weight-only Linear, 33 rows the W8A8 GEMM."""
    ops = pkg("ops")
    N = K = 2048
    x, w, rms, r, r2 = _data(33, N, K, 2)
    q = ops.quantize_fp8(w)
    aq = ops.ActQuant("fp8_e4m3", decode=True)
    assert [ops.linear_route(M, q, aq) for M in (4, 8, 32, 33)] == ["skinny", "a8w8_skinny", "a8w8_skinny", "a8w8"]
    names = _names(monkeypatch)
    with torch.no_grad():
        for M in (8, 32):
            xm, rm, rm2 = x[:M], r[:M], r2[:M]
            _same(names, lambda: ops.linear(xm, q, rms_w=rms, rms_eps=EPS, act_quant=aq),
                  lambda: ops.linear_a8w8_skinny(*ops.rmsnorm_quantize_rows_fp8(xm, rms, EPS), q))
            assert names == ["ull_rmsnorm_quantize_rows_fp8_bf16", "ull_gemm_skinny_a8w8_bf16"]
            _same(names, lambda: ops.linear(xm, q, act_quant=aq), lambda: ops.linear_a8w8_skinny(*ops.quantize_rows_fp8(xm), q))
            assert names == ["ull_quantize_rows_fp8_bf16", "ull_gemm_skinny_a8w8_bf16"]
            _same(names, lambda: ops.linear(xm, q, residual=rm, act_quant=aq), lambda: ops.linear_a8w8_skinny(*ops.quantize_rows_fp8(xm), q, residual=rm))
            _same(names, lambda: ops.linear(xm, q, rms_w=rms, rms_eps=EPS, residual=rm2, swiglu=True, out_f32=True, act_quant=aq),
                  lambda: ops.linear_a8w8_skinny(*ops.rmsnorm_quantize_rows_fp8(xm, rms, EPS), q, residual=rm2, swiglu=True, out_f32=True))
            x3 = xm.view(2, M // 2, K)                                                      # leading dims are kept
            assert torch.equal(ops.linear(x3, q, act_quant=aq), ops.linear(xm, q, act_quant=aq).view(2, M // 2, N))
        for kw in (dict(), dict(rms_w=rms, rms_eps=EPS), dict(residual=r[:4])):
            _same(names, lambda: ops.linear(x[:4], q, act_quant=aq, **kw), lambda: ops.linear(x[:4], q, **kw))
            assert "ull_gemm_skinny_wq_bf16" in names
        _same(names, lambda: ops.linear(x, q, act_quant=aq), lambda: ops.linear_a8w8(x, q))
        _same(names, lambda: ops.linear(x, q, rms_w=rms, rms_eps=EPS, residual=r, act_quant=aq), lambda: ops.linear_a8w8(ops.rmsnorm(x, rms, EPS), q, residual=r))
        # without decode: 8 rows stay W8A16, 32 rows are the W8A8 GEMM
        pre = ops.ActQuant("fp8_e4m3")
        _same(names, lambda: ops.linear(x[:8], q, act_quant=pre), lambda: ops.linear(x[:8], q))
        _same(names, lambda: ops.linear(x[:32], q, act_quant=pre), lambda: ops.linear_a8w8(x[:32], q))


def test_the_wrappers_are_reached_through_the_module(monkeypatch):
    """A test that replaces one of the three wrappers intercepts ops.linear's calls."""
    ops = pkg("ops")
    x, w, rms, r, _ = _data(8, 2048, 2048, 3)
    q, seen = ops.quantize_fp8(w), []
    for name in ("linear_a8w8", "linear_a8w8_skinny", "linear_w4a8"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **kw: seen.append((_n, sorted(kw))) or _r(*a, **kw))
    with torch.no_grad():
        ops.linear(x, q, residual=r, act_quant=ops.ActQuant("fp8_e4m3", decode=True))
        x26, w26 = _data(26, 192, 64, 4)[:2]
        ops.linear(x26, ops.quantize_fp8(w26), act_quant=ops.ActQuant("fp8_e4m3"))
        ops.linear(x26, ops.quantize_mxfp4(w26), act_quant=ops.ActQuant("mxfp8_e4m3"))
    kws = ["out", "out_f32", "residual", "swiglu"]
    assert seen == [("linear_a8w8_skinny", kws), ("linear_a8w8", kws), ("linear_w4a8", kws)]


def test_arguments_no_a8_kernel_has_are_refused_by_name(monkeypatch):
    ops = pkg("ops")
    M, N, K = 26, 192, 64
    x, w, rms, r, _ = _data(M, N, K, 5)
    bias = torch.zeros(N, device=DEV, dtype=BF)
    names = _names(monkeypatch)
    for q, aq in ((ops.quantize_fp8(w), ops.ActQuant("fp8_e4m3")), (ops.quantize_mxfp4(w), ops.ActQuant("mxfp8_e4m3"))):
        for kw, name in ((dict(bias=bias), "bias"), (dict(act="gelu"), "act"), (dict(bias=bias, bias_after_rounding=True), "bias"),
                         (dict(bias_after_rounding=True), "bias_after_rounding"), (dict(tune=ops.GEMM_TUNE_WAVES8), "tune")):
            with pytest.raises(RuntimeError, match=f"`{name}`"):
                ops.linear(x, q, act_quant=aq, **kw)
    x8, w8 = _data(8, 2048, 2048, 6)[:2]
    with pytest.raises(RuntimeError, match="`bias`"):
        ops.linear(x8, ops.quantize_fp8(w8), bias=torch.zeros(2048, device=DEV, dtype=BF), act_quant=ops.ActQuant("fp8_e4m3", decode=True))
    assert names == [n for n in names if n.startswith("ull_quantize_rows_")], "nothing is launched before a refusal (the weights' quantization aside)"
    with torch.no_grad():                                                                   # off the A8 routes the arguments are the Linear's own
        q = ops.quantize_fp8(w)
        assert torch.equal(ops.linear(x[:4], q, bias=bias, act="gelu", act_quant=ops.ActQuant("fp8_e4m3")), ops.linear(x[:4], q, bias=bias, act="gelu"))
