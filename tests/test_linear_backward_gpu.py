"""GPU: the Linear backward (autograd_ops._Linear / _LinearPacked: dX = linear(dY, W^T), dW = linear(dY^T, X^T), db = colsum(dY)) on every
GEMM route a training step takes, element by element against explicit fp64 matmuls on the CPU.

Two input families per case, run in this order on one stream with every tensor of the first kept alive during the second (a stale
stream-K / split-K workspace or a stale padding buffer then shows in the exact run):

* Gaussian: randn scaled as in test_kernels_gpu.test_gemm_plain; the project's elementwise rule of a once-rounded GEMM,
  |got - ref| <= 2 ulp * max(|ref|, 2 % of max|ref|) with one ulp = 2^-7 (bf16: helpers.assert_close_bf16) or 2^-10 (fp16: the rule of
  test_fp16_gpu.assert_close_f16, restated here).  The worst observed ratio to that bound is printed (docs/experiments.md keeps a record).
* exact: every operand a random integer in {-2 .. 2}.  Every product and every fp32 partial sum is then an integer of magnitude
  <= 4 * 4096 < 2^24 however the reduction is ordered, split, padded or tailed, so the accumulator holds the exact value and the output
  is that value rounded once: it must be torch.equal to the fp64 result cast to the dtype.  (All reduction lengths here are <= 4096; fp16
  cannot overflow: 16384 < 65504.)

The route of each of the two backward GEMMs is asserted twice: predicted from ops._linear_route / _big / _gemm_ws on the GEMM's own shape
(so a later change of the dispatch rule fails here instead of silently moving a case onto an already covered route), and observed on the
C-ABI call the backward really makes (entry point, M / N / padded K, workspace pointer).

Notes on the cases (M tokens x N out-features x K in-features of the forward Linear):
* case 2 (300, 2011, 512): its dW GEMM has 2011 rows, 512 columns and a reduction of 300 -> 320, which `_big` sends to the 256 x 256 kernel
  (no workspace); the dX GEMM stays on the 128-tile kernel.
* fp32 (cases 1 and 2): an fp32 dot product of length K is bounded by K * 2^-24 * sum_i |a_i b_i| (the classic worst case), NOT by
  K * 2^-24 * |sum_i a_i b_i|: where the terms cancel no fp32 summation meets the latter.  torch's own fp32 matmul on the CPU misses it on
  0.2 to 1.5 per cent of the elements of these four GEMMs (and, at reduction 37, still by 1.2x on elements above 2 % of max|ref|), while
  staying under 0.09 of the magnitude-sum bound.  The Gaussian fp32 check is therefore |got - ref| <= K * 2^-24 * (|A| @ |B|) elementwise:
  torch.allclose's rtol = K * 2^-24 taken against the magnitude sum of each dot product.  The share of elements beyond rtol * |ref| is
  printed.
"""
import contextlib
import functools

import pytest
import torch

from helpers import pkg, assert_close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, H, F32 = torch.bfloat16, torch.float16, torch.float32
ULP = {BF: 2.0 ** -7, H: 2.0 ** -10}
NAME = {BF: "bf16", H: "f16", F32: "f32"}
KEEP = []          # device tensors of the Gaussian run, held until the exact run of the same case is over


# ---- inputs and references (CPU, computed once per shape and shared: never modified) ------------------------------------------------------
def _ints(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g).double()


@functools.lru_cache(maxsize=None)
def _exact(M, N, K):
    """integer x, w, dy, bias, residual as float64 (exact in every dtype here) and the fp64 dX, dW, db."""
    x, w, dy, b, r = _ints(M, K, seed=11), _ints(N, K, seed=12), _ints(M, N, seed=13), _ints(N, seed=14), _ints(M, N, seed=15)
    return dict(x=x, w=w, dy=dy, b=b, r=r, dx=dy @ w, dw=dy.t() @ x, db=dy.sum(0))


def _gauss(M, N, K, dt):
    g = torch.Generator().manual_seed(1000 + M)
    x, w, dy = torch.randn(M, K, generator=g).to(dt), (torch.randn(N, K, generator=g) * K ** -0.5).to(dt), torch.randn(M, N, generator=g).to(dt)
    return dict(x=x, w=w, dy=dy, dx=dy.double() @ w.double(), dw=dy.double().t() @ x.double())


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def _assert_exact(got, ref64, what):
    got = got.detach().cpu()
    ref = ref64.to(got.dtype).reshape(got.shape)
    if torch.equal(got, ref):
        return
    g2, r2 = got.reshape(-1, got.shape[-1]), ref.reshape(-1, got.shape[-1])
    bad = g2 != r2
    r, c = (int(v) for v in bad.nonzero()[0])
    raise AssertionError(f"{what}: {int(bad.sum())} elements differ in {int(bad.any(1).sum())} of {g2.shape[0]} rows and "
                         f"{int(bad.any(0).sum())} of {g2.shape[1]} columns; first at (row {r}, column {c}): got {float(g2[r, c])}, "
                         f"exact {float(ref64.reshape(r2.shape)[r, c])} -> {float(r2[r, c])}")


def _assert_close(got, ref64, what):
    """the Gaussian family's check in the 16-bit types."""
    dt = got.dtype
    a, b = got.detach().cpu().double(), ref64
    fl = float(b.abs().max()) * 0.02
    ratio = float(((a - b).abs() / (ULP[dt] * torch.maximum(b.abs(), torch.full_like(b, fl)))).max())
    print(f"[linear-bwd] {what}: worst |d| / (ulp * max(|ref|, floor)) = {ratio:.3f} (bound 2.0)")
    if dt == BF:
        return assert_close_bf16(got, ref64, ulps=2.0, what=what)
    a, b = got.detach().float().cpu(), ref64.float()                 # fp16: test_fp16_gpu.assert_close_f16's rule
    fl = float(b.abs().max()) * 0.02
    bad = (a - b).abs() > 2.0 * 2.0 ** -10 * torch.maximum(b.abs(), torch.full_like(b, fl))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off; max|d|={float((a - b).abs().max()):.4g} max|ref|={float(b.abs().max()):.4g}"


def _assert_close_f32(got, ref64, mag64, what, red):
    """|got - ref| <= red * 2^-24 * (|A| @ |B|): the worst-case bound of an fp32 dot product of length `red` (module docstring)."""
    a = got.detach().cpu().double()
    rtol = red * 2.0 ** -24
    err = (a - ref64).abs()
    print(f"[linear-bwd] {what}: worst |d| / (K 2^-24 |A||B|) = {float((err / (rtol * mag64)).max()):.4f} (bound 1.0); "
          f"{float((err > rtol * ref64.abs()).double().mean()):.2e} of the elements beyond K 2^-24 |ref|")
    bad = err > rtol * mag64
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements beyond the fp32 dot-product bound"


# ---- routes: predicted from the dispatch predicates, observed on the C-ABI --------------------------------------------------------------
def _predict(M, N, K, ldw, dt):
    """(route, 256 x 256 kernel, K-split workspace, K zero-padded) of ops.linear(x [M, K], w [N, K] of row pitch ldw)."""
    ops = pkg("ops")
    if dt == F32:
        return ("f32", None, None, None)
    route, _ = ops._linear_route(M, N, K, ldw, 0)
    if route != "gemm":
        return (route, None, None, None)
    Kp = -(-K // 64) * 64
    big = ops._big(M, N, Kp)
    ws, _ = ops._gemm_ws(torch.device(DEV), torch.cuda.current_stream().cuda_stream, big, M, N, Kp, small_m=True)
    return ("gemm", big, ws is not None, Kp != K)


@contextlib.contextmanager
def _spy():
    """record (entry point, arguments) of every C-ABI call made inside the block."""
    L = pkg("_lib")
    calls, real = [], L.call

    def call(name, *args):
        calls.append((name, args))
        return real(name, *args)

    L.call = call
    try:
        yield calls
    finally:
        L.call = real


def _gemms(calls):
    return [(n, a) for n, a in calls if n.startswith(("ull_gemm_", "ull_gemv_"))]


def _n_transposes(calls):
    return sum(n.startswith("ull_transpose2d_") for n, _ in calls)


def _check_call(call, M, N, K, want, dt, what):
    """the observed call of one backward GEMM [M, K] x [N, K]^T against the predicted route `want`."""
    name, a = call
    route, big, ws, padded = want
    entry = {"f32": "ull_gemm_f32", "gemm": "ull_gemm_" + NAME[dt], "gemv": "ull_gemv_" + NAME[dt], "skinny": "ull_gemm_skinny_" + NAME[dt]}[route]
    assert name == entry, f"{what}: ran {name}, expected {entry}"
    if route == "gemm":
        Kp = -(-K // 64) * 64
        assert (a[9], a[10], a[11]) == (M, N, Kp) and (Kp != K) == padded, f"{what}: M, N, K = {a[9:12]}, expected {(M, N, Kp)}"
        assert (a[13] is not None) == ws, f"{what}: workspace {'passed' if a[13] is not None else 'missing'}"
        # row-major operands fresh from the transpose / the zero pad: no tile-major copy of a transposed operand is ever registered
        assert not a[12] & pkg("ops").EPI_W_TILED and (a[1], a[3]) == (Kp, Kp), f"{what}: flags {a[12]}, ldx {a[1]}, ldw {a[3]}"
    else:
        assert (a[9], a[10], a[11]) == (M, N, K) and (a[1], a[3]) == (K, K), f"{what}: M, N, K = {a[9:12]}, ldx {a[1]}, ldw {a[3]}"


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
G, GEMV, SKINNY = "gemm", ("gemv", None, None, None), ("skinny", None, None, None)
#         M,    N,    K      dX = [M, N] x [K, N]^T            dW = [N, M] x [K, M]^T        (route, 256 kernel, workspace, K padded)
CASES = {
    "c1": (37, 200, 192, (G, False, False, True), (G, False, False, True)),        # reductions 200 -> 256 and 37 -> 64, odd pitches
    "c2": (300, 2011, 512, (G, False, False, True), (G, True, False, True)),        # odd out-features (lm_head): 2011 -> 2048, dW has 2011 rows
    "c3": (1929, 1280, 512, (G, True, False, False), (G, True, False, True)),       # both on the 256 kernel, 1929 -> 1984 < streamk_min_k
    "c4": (2123, 1536, 512, (G, True, False, False), (G, True, True, True)),        # dW: 256 kernel + stream-K workspace on 2123 -> 2176
    "c5-1": (1, 1024, 512, GEMV, (G, False, False, True)),                          # dX: GEMV on W^T; dW reduction 1 .. 4 -> 64
    "c5-2": (2, 1024, 512, GEMV, (G, False, False, True)),
    "c5-4": (4, 1024, 512, GEMV, (G, False, False, True)),
    "c6-3": (3, 2048, 2048, SKINNY, (G, False, False, True)),                       # dX: skinny MFMA GEMM on W^T (3 tokens: not the GEMV)
    "c6-8": (8, 2048, 2048, SKINNY, (G, False, False, True)),
    "c6-16": (16, 2048, 2048, SKINNY, (G, False, False, True)),
}
C7 = (256, 1024, 4096)          # dX [256, 1024] x [4096, 1024]^T: split-K of the 128-tile kernel under ops.small_m_split_k(True)


def _backward(dt, data, tag):
    """one plain Linear forward + backward on the device; returns (dx, dw, the C-ABI calls of the backward)."""
    A = pkg("autograd_ops")
    x, w = data["x"].to(dt).to(DEV).requires_grad_(True), data["w"].to(dt).to(DEV).requires_grad_(True)
    dy = data["dy"].to(dt).to(DEV)
    y = A.linear(x, w)
    with _spy() as calls:
        y.backward(dy)
    torch.cuda.synchronize()
    KEEP.extend((x, w, dy, y, x.grad, w.grad))
    assert x.grad.dtype == dt and w.grad.dtype == dt and x.grad.shape == x.shape and w.grad.shape == w.shape, tag
    return x.grad, w.grad, calls


def _run_case(dt, M, N, K, want_dx, want_dw, tag):
    assert max(M, N) <= 4096                                    # the two reduction lengths: the exactness argument needs <= 4096
    if dt == F32:
        want_dx = want_dw = ("f32", None, None, None)
    assert _predict(M, K, N, N, dt) == want_dx, f"{tag}: dX route {_predict(M, K, N, N, dt)}"
    assert _predict(N, K, M, M, dt) == want_dw, f"{tag}: dW route {_predict(N, K, M, M, dt)}"
    try:
        for family in ("gauss", "exact"):
            data = _gauss(M, N, K, dt) if family == "gauss" else _exact(M, N, K)
            dx, dw, calls = _backward(dt, data, tag)
            gemms = _gemms(calls)
            assert len(gemms) == 2, [n for n, _ in gemms]
            _check_call(gemms[0], M, K, N, want_dx, dt, f"{tag} dX")
            _check_call(gemms[1], N, K, M, want_dw, dt, f"{tag} dW")
            what = f"{tag} {NAME[dt]} {family}"
            if family == "exact":
                _assert_exact(dx, data["dx"], what + " dX")
                _assert_exact(dw, data["dw"], what + " dW")
            elif dt == F32:
                xa, wa, ga = (data[k].double().abs() for k in ("x", "w", "dy"))
                _assert_close_f32(dx, data["dx"], ga @ wa, what + " dX", N)
                _assert_close_f32(dw, data["dw"], ga.t() @ xa, what + " dW", M)
            else:
                _assert_close(dx, data["dx"], what + " dX")
                _assert_close(dw, data["dw"], what + " dW")
    finally:
        KEEP.clear()


@pytest.mark.parametrize("dt", [BF, H], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", list(CASES))
def test_linear_backward_routes(case, dt):
    M, N, K, want_dx, want_dw = CASES[case]
    _run_case(dt, M, N, K, want_dx, want_dw, case)


@pytest.mark.parametrize("case", ["c1", "c2"])
def test_linear_backward_fp32(case):
    """the fp32 build: ull_gemm_f32 (any M / N / K / strides) on operands from the fp32 transpose."""
    M, N, K, want_dx, want_dw = CASES[case]
    _run_case(F32, M, N, K, want_dx, want_dw, case)


@pytest.mark.parametrize("dt", [BF, H], ids=["bf16", "f16"])
def test_linear_backward_small_m_split_k(dt):
    """case 7: dX through the split-K of the 128-tile kernel (opt-in), dW on the 256 kernel; with the context off the same shapes run
    unsplit.  Both are exact on integers and within 2 ulp on Gaussian inputs."""
    ops = pkg("ops")
    M, N, K = C7
    for on in (True, False):
        with ops.small_m_split_k(on):
            _run_case(dt, M, N, K, (G, False, on, False), (G, True, False, False), f"c7 split-K {'on' if on else 'off'}")


# ---- operand forms of the training path (exact family, cases 1 and 3) -------------------------------------------------------------------
FORM_CASES = {"c1": (37, 200, 192, 1, (96, 72, 32)), "c3": (1929, 1280, 512, 3, (1024, 128, 128))}     # M, N, K, batch B (M = B * S), packed rows
forms = pytest.mark.parametrize("dt", [BF, H], ids=["bf16", "f16"])
form_cases = pytest.mark.parametrize("case", list(FORM_CASES))


def _dev(t, dt, grad=False):
    return t.to(dt).to(DEV).requires_grad_(grad)


@forms
@form_cases
def test_strided_3d_x_and_sliced_dy(case, dt):
    """x is a [B, S, K] view of a wider buffer (row pitch K + 24), dy a column slice of a wider tensor."""
    A = pkg("autograd_ops")
    M, N, K, B, _ = FORM_CASES[case]
    e = _exact(M, N, K)
    xbuf = torch.full((B, M // B, K + 24), 7.0, dtype=dt, device=DEV)
    xbuf[..., :K] = e["x"].to(dt).view(B, M // B, K)
    x = xbuf[..., :K].requires_grad_(True)
    assert not x.is_contiguous() and x.stride(1) == K + 24
    w = _dev(e["w"], dt, True)
    dybuf = torch.full((B, M // B, N + 13), 7.0, dtype=dt, device=DEV)
    dybuf[..., 5:5 + N] = e["dy"].to(dt).view(B, M // B, N)
    dy = dybuf[..., 5:5 + N]
    assert not dy.is_contiguous()
    A.linear(x, w).backward(dy)
    assert x.grad.shape == x.shape
    _assert_exact(x.grad, e["dx"], f"{case} strided dX")
    _assert_exact(w.grad, e["dw"], f"{case} strided dW")


@forms
@form_cases
def test_bias_and_residual(case, dt):
    A = pkg("autograd_ops")
    M, N, K, _, _ = FORM_CASES[case]
    e = _exact(M, N, K)
    x, w, b, r = (_dev(e[k], dt, True) for k in ("x", "w", "b", "r"))
    dy = _dev(e["dy"], dt)
    A.linear(x, w, b, residual=r).backward(dy)
    _assert_exact(x.grad, e["dx"], f"{case} bias+residual dX")
    _assert_exact(w.grad, e["dw"], f"{case} bias+residual dW")
    assert b.grad.dtype == dt
    _assert_exact(b.grad, e["db"], f"{case} db")
    assert torch.equal(r.grad, dy), "dres must be dy itself"


@forms
@form_cases
def test_relu(case, dt):
    """the mask is the sign of the y the HIP forward returned (the tensor saved for backward), not a recomputed forward."""
    A = pkg("autograd_ops")
    M, N, K, _, _ = FORM_CASES[case]
    e = _exact(M, N, K)
    x, w, b = (_dev(e[k], dt, True) for k in ("x", "w", "b"))
    y = A.linear(x, w, b, relu=True)
    y.backward(_dev(e["dy"], dt))
    yc = y.detach().cpu().double()
    assert bool((yc >= 0).all()) and 0.2 < float((yc > 0).double().mean()) < 0.8
    g = e["dy"] * (yc > 0)
    _assert_exact(x.grad, g @ e["w"], f"{case} relu dX")
    _assert_exact(w.grad, g.t() @ e["x"], f"{case} relu dW")
    _assert_exact(b.grad, g.sum(0), f"{case} relu db")


@forms
@form_cases
def test_requires_grad_subsets(case, dt):
    A = pkg("autograd_ops")
    M, N, K, _, _ = FORM_CASES[case]
    e = _exact(M, N, K)
    dy = _dev(e["dy"], dt)
    # only x: the frozen weight's transpose is made once, reused, and re-made after an in-place update of the weight
    x, w = _dev(e["x"], dt, True), _dev(e["w"], dt)
    with _spy() as calls:
        A.linear(x, w).backward(dy)
    assert _n_transposes(calls) == 1 and len(_gemms(calls)) == 2 and w.grad is None       # forward GEMM + dX GEMM
    _assert_exact(x.grad, e["dx"], f"{case} frozen-w dX")
    kept = A._T_CACHE[id(w)][2]
    x.grad = None
    with _spy() as calls:
        A.linear(x, w).backward(dy)
    assert _n_transposes(calls) == 0 and A._T_CACHE[id(w)][2] is kept, "the kept W^T was not reused"
    _assert_exact(x.grad, e["dx"], f"{case} frozen-w dX, second backward")
    w.add_(1)
    x.grad = None
    with _spy() as calls:
        A.linear(x, w).backward(dy)
    _assert_exact(x.grad, e["dy"] @ (e["w"] + 1), f"{case} frozen-w dX after w.add_(1)")
    assert _n_transposes(calls) == 1, "the kept W^T was not refreshed after w.add_(1)"
    # only w
    x, w = _dev(e["x"], dt), _dev(e["w"], dt, True)
    with _spy() as calls:
        A.linear(x, w).backward(dy)
    assert x.grad is None and _n_transposes(calls) == 2 and len(_gemms(calls)) == 2       # forward GEMM + dW GEMM
    _assert_exact(w.grad, e["dw"], f"{case} only-w dW")


@forms
@form_cases
def test_linear_packed(case, dt):
    """three row-slice parameters of one buffer: their gradients are the row slices of the one dW; dX with all trainable (fresh W^T) and
    all frozen (kept W^T)."""
    A = pkg("autograd_ops")
    M, N, K, _, rows = FORM_CASES[case]
    assert sum(rows) == N
    e = _exact(M, N, K)
    dy = _dev(e["dy"], dt)
    for train in (True, False):
        packed = _dev(e["w"], dt)
        offs = [sum(rows[:i]) for i in range(len(rows))]
        ws = [torch.nn.Parameter(packed[o:o + n], requires_grad=train) for o, n in zip(offs, rows)]
        assert all(p.data_ptr() == packed.data_ptr() + o * K * 2 for p, o in zip(ws, offs))
        x = _dev(e["x"], dt, True)
        A.linear_packed(x, packed, *ws).backward(dy)
        _assert_exact(x.grad, e["dx"], f"{case} packed dX ({'trainable' if train else 'frozen'})")
        for i, (p, o, n) in enumerate(zip(ws, offs, rows)):
            if train:
                assert p.grad.shape == p.shape
                _assert_exact(p.grad, e["dw"][o:o + n], f"{case} packed dW[{i}] rows {o}..{o + n}")
            else:
                assert p.grad is None
        if not train:
            assert A._T_CACHE[id(packed)][0]() is packed


@forms
def test_colsum_exact(dt):
    """ops.colsum directly: one row, around the 4-wave / 64-row steps, strided rows, many columns.  Integers: the fp32 sum is exact."""
    ops = pkg("ops")
    for rows, cols, pad in ((1, 200, 0), (255, 130, 0), (256, 130, 0), (257, 130, 0), (4100, 96, 40), (37, 2011, 0)):
        v = _ints(rows, cols + pad, seed=rows + cols)
        got = ops.colsum(v.to(dt).to(DEV)[:, :cols])
        assert got.dtype == torch.float32 and got.shape == (cols,)
        _assert_exact(got, v[:, :cols].sum(0), f"colsum {rows} x {cols} (+{pad})")


def test_transpose2d_fp32_strided_and_ragged():
    """ull_transpose2d_f32 on its own: rows of a padded pitch, shapes that are no multiple of the 64 x 64 tile, one row, one column."""
    ops = pkg("ops")
    for R, C, pad in ((1, 200, 0), (200, 1, 3), (37, 192, 24), (64, 64, 8), (65, 129, 0), (300, 2011, 5)):
        g = torch.Generator().manual_seed(R * 7 + C)
        v = torch.randn(R, C + pad, generator=g)
        got = ops.transpose2d(v.to(DEV)[:, :C])
        assert got.shape == (C, R) and got.is_contiguous() and got.dtype == F32
        assert torch.equal(got.cpu(), v[:, :C].t()), f"transpose2d fp32 {R} x {C} (+{pad})"


@forms
def test_folded_3d_view_outside_linear(dt):
    """ops._rows folds a [B, S, D] view of a wider buffer onto rows of one pitch for every op that takes a row pitch: rmsnorm on such a
    view gives the bits it gives on the contiguous copy."""
    ops = pkg("ops")
    g = torch.Generator().manual_seed(5)
    buf = (torch.randn(3, 37, 256 + 24, generator=g) * 1.5).to(dt).to(DEV)
    w = (torch.randn(256, generator=g) * 0.1 + 1.0).to(dt).to(DEV)
    view = buf[..., :256]
    assert not view.is_contiguous()
    got = ops.rmsnorm(view, w, 1e-6)
    assert got.shape == view.shape and torch.equal(got, ops.rmsnorm(view.contiguous(), w, 1e-6))
    with pytest.raises(RuntimeError, match="one common pitch"):
        ops.rmsnorm(buf[:, ::2, :256], w, 1e-6)


def test_fp32_backward_pieces_without_a_kernel_say_so():
    """the fp32 build has the Linear's dX and dW only: a bias gradient or a relu mask in fp32 is refused by name, before any launch."""
    A = pkg("autograd_ops")
    e = _exact(37, 200, 192)
    x, w, b = (_dev(e[k], F32, True) for k in ("x", "w", "b"))
    for kw in (dict(bias=b), dict(relu=True)):
        y = A.linear(x, w, **kw)
        with pytest.raises(RuntimeError, match="fp32 Linear backward"):
            y.backward(_dev(e["dy"], F32))
