"""GPU: SiLU (SwiGLU) and QuickGELU over every finite 16-bit input on every kernel path that evaluates them, against float64 references.

The pre-activation is planted exactly: the activation rows are one-hot (x[m] = e_k) and column k of the weight carries the 16-bit values,
so the fp32 accumulator holds exactly that value (every other term is 0 * finite; non-finite patterns are replaced by 0; -0.0 arrives as
+0.0, helpers.planted).  The expected values come from helpers.swiglu_ref / quick_gelu_ref / swiglu_bwd_ref (float64, rounded where the
reference rounds), never from a kernel of this project.  helpers.sweep_compare asserts for every finite planted input: (a) never NaN,
(b) an infinity of the reference (fp16 overflow) is matched, (c) at most one 16-bit ulp off (floor 2^-24 in fp16, 2^-100 in bf16),
(d) the number of inputs that differ bitwise from the reference is capped (MEASURED).

Tier A: every finite pattern of bf16 and fp16 on ops.swiglu_fwd / swiglu_bwd (both column layouts), the 128-tile GEMM, the three forms of
the 256-tile GEMM, the skinny GEMM and the GEMV; SwiGLU with up == 1 and up == -3, QuickGELU with N = I, and QuickGELU with a zero
residual, which is what takes the staged epilogue off its inline activation loop and onto the general finish (big_finish8, the only place
that evaluates QuickGELU there).  The fp32 build (true division) is swept once as a control.
Tier B: a fixed edge list, periodic in the weight, on the routes that cannot carry arbitrary patterns or that only some tiles take: the
stream-K and split-K finalize, fp8 / mxfp4 weights on the GEMV and the skinny GEMM, a8w8, w4a8 and the a8w8 decode step.  Quantization
makes the planted value inexact there, so the oracle is the route's own output without activation on the gate rows (and the up rows), to
which the float64 reference activation is applied.

Before rcp_newton (csrc/ull_common.h) took the median of its result with 0 and 1, every case here but the fp32 control failed (a): NaN for
SiLU inputs <= -89 and QuickGELU inputs <= -52.25 on every path listed above.
"""
import contextlib
import functools

import pytest
import torch

from helpers import (pkg, all_patterns, planted, swiglu_ref, quick_gelu_ref, swiglu_bwd_ref, sweep_compare, QGELU_SCALE)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, H, F32 = torch.bfloat16, torch.float16, torch.float32
DTS = [BF, H]
NAME = {BF: "bf16", H: "f16"}
UPS = [1.0, -3.0]

# (d) inputs that may differ bitwise from the float64 reference: twice the count measured on the MI355X, never above 0.1 % of the inputs.
# Every site evaluates the same three helpers, and the counts were the same on every route.  Measured, of 65 280 bf16 / 63 488 fp16 inputs:
#   SwiGLU, up = 1 and up = -3     20 / 0    bf16: the 20 gates -97 .. -87.5, all below the floor: the reference is a bf16 subnormal or a
#                                            normal below 6e-37 where the kernel has -0.0 (fp32 1 + exp(-g) has overflowed from -89 down,
#                                            as in torch's own kernel; above, its reciprocal is an fp32 denormal); fp16: bit for bit
#   QuickGELU                      12 / 4    bf16: the 12 inputs -54.25 .. -51.5, the same tail of the sigmoid (|ref| < 6e-37); fp16: four
#                                            one-ulp results in 8e-4 < |x| < 7e-3, the inputs at which torch's CPU kernel differs too
#   QuickGELU + zero residual      12 / 4    the same inputs (the residual add turns -0.0 into +0.0 on both sides)
#   swiglu_bwd, da = 1             d_gate 23 / 7, d_up 20 / 2
#   swiglu_bwd, varied da          d_gate 21 / 5, d_up 53 / 3 (bf16 d_up: twice the count is above 0.1 %, which then is the cap: 65)
# On the parent of the fix 769 276 of the 3 932 160 tier-A outputs were NaN; the other 3 162 884 have the same bits before and after.
MEASURED = {("swiglu", 1.0): {BF: 20, H: 0}, ("swiglu", -3.0): {BF: 20, H: 0}, "quick_gelu": {BF: 12, H: 4}, "quick_gelu_resid": {BF: 12, H: 4},
            ("bwd", "ones", "d_gate"): {BF: 23, H: 7}, ("bwd", "ones", "d_up"): {BF: 20, H: 2},
            ("bwd", "varied", "d_gate"): {BF: 21, H: 5}, ("bwd", "varied", "d_up"): {BF: 53, H: 3}}
N_FINITE = {BF: 65280, H: 63488}


def _cap(key, dt):
    return min(2 * MEASURED[key][dt], N_FINITE[dt] // 1000)


# ---- planting ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _patterns(dt):
    return all_patterns(dt)


def _one_hot(M, K, P, dt):
    """x [M, K] with x[m] = e_(m % P)."""
    x = torch.zeros(M, K, dtype=dt)
    x[torch.arange(M), torch.arange(M) % P] = 1
    return x


def _pattern_weight(I, K, P, dt):
    """w [I, K] whose first P columns hold all 65 536 patterns (I * P of them, non-finite -> 0), repeated over the other columns (which
    only ever meet zeros of x), and the finite mask of the first P columns."""
    pat, fin = _patterns(dt)
    assert I * P == 65536 and K % P == 0
    return pat.view(I, P).repeat(1, K // P).contiguous(), fin.view(I, P)


def _read_out(w, M, P):
    """what row m of the one-hot x reads from w [I, K]: [M, I] = planted(w[:, m % P])."""
    return planted(w[:, torch.arange(M) % P].t().contiguous())


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


def _linears(calls):
    return [(n, a) for n, a in calls if n.startswith(("ull_gemm_", "ull_gemv_"))]


def _first_copy(y, M, P, what):
    """rows m and m + P planted the same values: all copies must agree bit for bit; the first one is compared with the reference."""
    y = y.cpu()
    if M > P:
        v = y.view(torch.int16).view(M // P, P, -1)
        assert bool((v == v[:1]).all()), f"{what}: rows that planted the same values differ"
    return y[:P]


# ---- Tier A: the Linear routes ------------------------------------------------------------------------------------------------------
W8, W4 = "waves8", "waves4"
#          name        M     K     I    route     256-tile kernel, forced form (None: the dispatch's own choice)
ROUTES = [("gemm128", 64, 64, 1024, "gemm", False, None),
          ("gemm256-w8", 1024, 128, 512, "gemm", True, W8),            # LDS-staged epilogue
          ("gemm256-w4", 1024, 128, 512, "gemm", True, W4),            # register-direct epilogue of the 4-wave kernel
          ("gemm256", 1024, 128, 512, "gemm", True, None),             # QuickGELU: the 8-wave kernel with the register-direct epilogue
          ("skinny", 16, 1024, 4096, "skinny", False, None),
          ("gemv", 4, 64, 16384, "gemv", False, None)]


def _run_route(case, dt, w, swiglu, act, zero_residual=False):
    """ops.linear on the planted operands of one ROUTES case, with the predicted route asserted on the dispatch rule and on the C-ABI call."""
    ops = pkg("ops")
    name, M, K, I, route, big, form = case
    N, P = w.shape[0], min(M, K)
    tune = {None: 0, W8: ops.GEMM_TUNE_WAVES8, W4: ops.GEMM_TUNE_WAVES4}[form]
    assert ops._linear_route(M, N, K, K, tune)[0] == route and (route != "gemm" or ops._big(M, N, K) == big), (name, N)
    wd = w.to(DEV)
    if big:
        ops.register_tiled(wd)               # what pack_weights does: without the tile-major copy a K this short stays on the 128-tile kernel
    x = _one_hot(M, K, P, dt).to(DEV)
    res = torch.zeros(M, N // 2 if swiglu else N, dtype=dt, device=DEV) if zero_residual else None
    with _spy() as calls:
        y = ops.linear(x, wd, swiglu=swiglu, act=act, residual=res, tune=tune)
    torch.cuda.synchronize()
    (entry, a), = _linears(calls)
    assert bool(a[12] & ops.EPI_RESID) == zero_residual, (name, a[12])
    assert entry == {"gemm": "ull_gemm_", "skinny": "ull_gemm_skinny_", "gemv": "ull_gemv_"}[route] + NAME[dt], (name, entry)
    assert (a[9], a[10], a[11]) == (M, N, K), (name, a[9:12])
    if route == "gemm":
        assert bool(a[12] & ops.EPI_W_TILED) == big and a[13] is None, (name, a[12], a[13])        # no K split at these K
    return _first_copy(y, M, P, name)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("case", ROUTES[:3] + ROUTES[4:], ids=lambda c: c[0])
def test_swiglu_over_every_16_bit_gate(case, dt):
    M_ = pkg("modeling_core")
    name, M, K, I, *_ = case
    P = min(M, K)
    wg, fin = _pattern_weight(I, K, P, dt)
    g = _read_out(wg, P, P)
    for up in UPS:
        wu = torch.full_like(wg, up)
        got = _run_route(case, dt, M_.interleave_gate_up(wg, wu), True, None)
        ref = swiglu_ref(g, torch.full_like(g, up), dt)
        sweep_compare(got, ref, dt, _cap(("swiglu", up), dt), f"swiglu {name} {NAME[dt]} up={up}", fin.t())


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c[0])
def test_quick_gelu_over_every_16_bit_input(case, dt):
    name, M, K, I, *_ = case
    P = min(M, K)
    w, fin = _pattern_weight(I, K, P, dt)
    got = _run_route(case, dt, w, False, "quick_gelu")
    sweep_compare(got, quick_gelu_ref(_read_out(w, P, P), dt), dt, _cap("quick_gelu", dt), f"quick_gelu {name} {NAME[dt]}", fin.t())


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("case", ROUTES[:2], ids=lambda c: c[0])
def test_quick_gelu_on_the_general_finish_path_over_every_16_bit_input(case, dt):
    """An activation together with a residual is the one combination that leaves the staged epilogue's inline activation loop (128-tile and
    8-wave 256-tile kernel) for the general finish, big_finish8, which evaluates QuickGELU itself.  The residual is zero: the expected value
    is rnd(0 + quick_gelu), which differs from quick_gelu only in that -0.0 becomes +0.0."""
    name, M, K, I, *_ = case
    P = min(M, K)
    w, fin = _pattern_weight(I, K, P, dt)
    got = _run_route(case, dt, w, False, "quick_gelu", zero_residual=True)
    ref = (quick_gelu_ref(_read_out(w, P, P), dt).double() + 0.0).to(dt)
    sweep_compare(got, ref, dt, _cap("quick_gelu_resid", dt), f"quick_gelu + zero residual {name} {NAME[dt]}", fin.t())


# ---- Tier A: the training path's elementwise kernels ----------------------------------------------------------------------------------
def _columns(gate, up, halves):
    """[M, 2I] in the layout swiglu_fwd / swiglu_bwd read: [gate | up] halves, or the 16-column interleave of the inference pack."""
    if halves:
        return torch.cat([gate, up], dim=1).contiguous()
    return pkg("modeling_core").interleave_gate_up(gate.t().contiguous(), up.t().contiguous()).t().contiguous()


def _split(dgu, I, halves):
    if halves:
        return dgu[:, :I], dgu[:, I:]
    v = dgu.view(dgu.shape[0], I // 16, 2, 16)
    return v[:, :, 0].reshape(-1, I), v[:, :, 1].reshape(-1, I)


ELT_M, ELT_I = 2048, 32        # 65 536 gates; I = 32 is the smallest width at which the two column layouts differ


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("halves", [False, True], ids=["interleaved", "halves"])
def test_swiglu_fwd_kernel_over_every_16_bit_gate(halves, dt):
    ops = pkg("ops")
    pat, fin = _patterns(dt)
    g = pat.view(ELT_M, ELT_I)                                   # read directly: -0.0 stays -0.0 here
    for up in UPS:
        u = torch.full_like(g, up)
        got = ops.swiglu_fwd(_columns(g, u, halves).to(DEV), halves=halves).cpu()
        sweep_compare(got, swiglu_ref(g, u, dt), dt, _cap(("swiglu", up), dt), f"swiglu_fwd {'halves' if halves else 'interleaved'} {NAME[dt]} up={up}", fin)


def _varied(shape, dt):
    """incoming gradients / up values that vary from element to element: both signs, some large, some small, none zero, and every one with
    the last mantissa bit of the type set.  A value of few significant bits (3.0, 0.75) times a gate is an exact tie of the 16-bit grid
    for a quarter of the gates, and wherever the sigmoid is 1/2 or 1 to within fp32 (|g| < 1e-4, g > 16.6) any fp32 evaluation then rounds
    the tie to even while the float64 value sits a hair beside it: the count (d) would measure the test's inputs, not the kernel (525 of
    65 280 in bf16 with such values).  With the last bit set only gates of one or two significant bits can still produce a tie."""
    vals = torch.tensor([0.5, -2.0, 3.0, -0.75, 1.25, -1.0, 96.0, -0.0078125], dtype=torch.float64).to(dt)
    vals = (vals.view(torch.int16) | 1).view(dt)
    n = shape[0] * shape[1]
    return vals[(torch.arange(n) * 5 + torch.arange(n) // 8) % 8].view(shape)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("halves", [False, True], ids=["interleaved", "halves"])
def test_swiglu_bwd_kernel_over_every_16_bit_gate(halves, dt):
    ops = pkg("ops")
    pat, fin = _patterns(dt)
    g = pat.view(ELT_M, ELT_I)
    for kind in ("ones", "varied"):
        da = torch.ones_like(g) if kind == "ones" else _varied(g.shape, dt)
        u = torch.full_like(g, -3.0) if kind == "ones" else _varied(g.shape, dt).flip(1)
        dgu = ops.swiglu_bwd(_columns(g, u, halves).to(DEV), da.to(DEV), halves=halves).cpu()
        dg, du = _split(dgu, ELT_I, halves)
        rg, ru = swiglu_bwd_ref(g, u, da, dt)
        what = f"swiglu_bwd {'halves' if halves else 'interleaved'} {NAME[dt]} da={kind}"
        sweep_compare(dg.contiguous(), rg, dt, _cap(("bwd", kind, "d_gate"), dt), what + " d_gate", fin)
        sweep_compare(du.contiguous(), ru, dt, _cap(("bwd", kind, "d_up"), dt), what + " d_up", fin)


# ---- control: the fp32 build divides (csrc/f32.hip sigmoid32) and was never affected -------------------------------------------------
def test_fp32_build_control_on_the_128_tile_shape():
    ops, M_ = pkg("ops"), pkg("modeling_core")
    name, M, K, I, *_ = ROUTES[0]
    wg, fin = _pattern_weight(I, K, K, BF)
    g = _read_out(wg, M, K).double()
    x = _one_hot(M, K, K, F32).to(DEV)
    y = ops.linear(x, M_.interleave_gate_up(wg, torch.full_like(wg, -3.0)).float().to(DEV), swiglu=True).cpu().double()
    q = ops.linear(x, wg.float().to(DEV), act="quick_gelu").cpu().double()
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    for what, got, ref in (("swiglu", y, g * sig(g) * -3.0), ("quick_gelu", q, g * sig(QGELU_SCALE * g))):
        assert not bool(torch.isnan(got).any()), f"fp32 {what}: NaN"
        ref = ref.float().double()                               # an fp32 result: overflow and underflow as fp32 has them
        inf = torch.isinf(ref)
        assert torch.equal(got[inf], ref[inf]), f"fp32 {what}: overflow"
        # fp32 roundings of expf's argument (up to 89 of its ulps in the result), expf, the division and two products; 1e-30 floor
        tol = 2e-5 * ref.abs() + 2.0 ** -100
        bad = ((got - ref).abs() > tol)[fin.t() & ~inf]
        assert not bool(bad.any()), f"fp32 {what}: {int(bad.sum())} off"


# ---- Tier B: the edge list on the quantized and the K-split routes ----------------------------------------------------------------------
def _edges():
    """+-0, +-2^e (e = -20 .. 15) and +-{52, 52.5, 60, 87, 88, 88.5, 89, 96, 128, 448, 1000, 30000}, ordered by magnitude so that the 32
    consecutive entries of an mxfp4 block have neighbouring magnitudes (a block then keeps more than its largest element)."""
    mags = sorted([0.0] + [2.0 ** e for e in range(-20, 16)] + [52, 52.5, 60, 87, 88, 88.5, 89, 96, 128, 448, 1000, 30000])
    return torch.tensor([s * m for m in mags for s in (1.0, -1.0)], dtype=torch.float64)


def _edge_weight(N, K, shift=0):
    """w[n, k] = list[(n + k + shift) % L] in bf16 (every entry but 30000 -> 29952 is exact): every output tile sees the whole list."""
    e = _edges()
    idx = (torch.arange(N)[:, None] + torch.arange(K)[None, :] + shift) % e.numel()
    return e[idx].to(BF)


def _edge_case(run, M, K, I, dt, what, acts=("swiglu",), reach=-89.0, quant=None):
    """One Tier-B route.  run(x, w, swiglu, act) is the route on the device operands; its plain output on the gate rows (and on the up rows)
    is the oracle's pre-activation.  `reach`: the oracle must itself contain gates at or below it, or the case tests nothing."""
    M_ = pkg("modeling_core")
    quant = quant or (lambda w: w)
    wg, wu = _edge_weight(I, K).to(dt), _edge_weight(I, K, shift=37).to(dt)
    x = _one_hot(M, K, min(M, K), dt).to(DEV)
    pg, pu = run(x, quant(wg.to(DEV)), False, None).cpu(), run(x, quant(wu.to(DEV)), False, None).cpu()
    assert pg.dtype == dt and pg.shape == (M, I)
    fin = torch.isfinite(pg) & torch.isfinite(pu)
    assert bool((pg[fin].float() <= reach).any()) and bool((pg[fin].float() >= 8).any()), f"{what}: the oracle misses the far tails"
    for act in acts:
        if act == "swiglu":
            got = run(x, quant(M_.interleave_gate_up(wg, wu).to(DEV)), True, None)
            ref = swiglu_ref(pg, pu, dt)
        else:
            got = run(x, quant(wg.to(DEV)), False, act)
            ref = quick_gelu_ref(pg, dt)
        torch.cuda.synchronize()
        sweep_compare(got.cpu(), ref, dt, None, f"{what} {act}", fin)          # (a) to (c): the list repeats its few inputs, a count says nothing


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_stream_k_finalize_on_the_edge_list(dt):
    """the swiglu shape of test_gemm_streamk_tail, with the tile-major weight copy and a K threshold that let the 256-tile kernel split its
    partial last round at this K: the finalize kernel evaluates the activation of those tiles."""
    ops = pkg("ops")
    M, K, I = 256 * 9 + 3, 256, 256 * 15

    def run(x, w, swiglu, act):
        N = w.shape[0]
        ops.register_tiled(w)
        with ops.streamk_policy(128), _spy() as calls:
            y = ops.linear(x, w, swiglu=swiglu, act=act)
        (entry, a), = _linears(calls)
        assert entry == "ull_gemm_" + NAME[dt] and a[12] & ops.EPI_W_TILED and a[13] is not None, (entry, a[12], a[13])
        if swiglu or act:                    # these launches must end in the finalize: more tiles than CUs and a partial round of at most half of them
            T, cu = -(-M // 256) * -(-N // 256), _n_cu()
            assert T > cu and 0 < T % cu <= cu // 2, (T, cu)
        return y

    _edge_case(run, M, K, I, dt, f"stream-K finalize {NAME[dt]}", acts=("swiglu",))
    M, K, N = 256 * 9 + 3, 256, 256 * 30
    _edge_case(run, M, K, N, dt, f"stream-K finalize {NAME[dt]}", acts=("quick_gelu",), reach=-52.25)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_split_k_finalize_on_the_edge_list(dt):
    """the swiglu shape of test_small_m_gemm_split_k_matches_reference_and_unsplit under small_m_split_k: every tile goes through the finalize."""
    ops = pkg("ops")
    M, K = 323, 1024

    def run(x, w, swiglu, act):
        with ops.small_m_split_k(True), _spy() as calls:
            y = ops.linear(x, w, swiglu=swiglu, act=act)
        (entry, a), = _linears(calls)
        assert entry == "ull_gemm_" + NAME[dt] and not a[12] & ops.EPI_W_TILED, (entry, a[12])
        if swiglu or act:
            assert a[13] is not None, "no split-K workspace passed"
        return y

    _edge_case(run, M, K, 2048, dt, f"split-K finalize {NAME[dt]}", acts=("swiglu",))
    _edge_case(run, M, K, 4096, dt, f"split-K finalize {NAME[dt]}", acts=("quick_gelu",), reach=-52.25)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
@pytest.mark.parametrize("route,M,K,I", [("gemv", 4, 256, 512), ("skinny", 16, 1024, 4096)])
def test_quantized_weights_on_the_edge_list(route, M, K, I, fmt):
    ops = pkg("ops")
    quant = ops.quantize_fp8 if fmt == "fp8" else ops.quantize_mxfp4

    def run(x, w, swiglu, act):
        assert ops.linear_route(M, w) == route, (ops.linear_route(M, w), w.shape)
        with _spy() as calls:
            y = ops.linear(x, w, swiglu=swiglu, act=act)
        (entry, a), = _linears(calls)
        assert entry == {"gemv": "ull_gemv_wq_bf16", "skinny": "ull_gemm_skinny_wq_bf16"}[route], entry
        return y

    _edge_case(run, M, K, I, BF, f"{fmt} {route}", acts=("swiglu", "quick_gelu"), quant=quant)


@pytest.mark.parametrize("route,M,K,I", [("a8w8", 128, 128, 256), ("w4a8", 128, 128, 256), ("a8w8_skinny", 24, 1024, 4096)])
def test_quantized_activations_on_the_edge_list(route, M, K, I):
    ops = pkg("ops")
    quant = ops.quantize_mxfp4 if route == "w4a8" else ops.quantize_fp8
    aq = {"a8w8": ops.ActQuant("fp8_e4m3"), "w4a8": ops.ActQuant("mxfp8_e4m3"), "a8w8_skinny": ops.ActQuant("fp8_e4m3", True)}[route]
    entry_of = {"a8w8": "ull_gemm_a8w8_bf16", "w4a8": "ull_gemm_w4a8_bf16", "a8w8_skinny": "ull_gemm_skinny_a8w8_bf16"}

    def run(x, w, swiglu, act):
        assert ops.linear_route(M, w, aq) == route, (ops.linear_route(M, w, aq), w.shape)
        with _spy() as calls:
            y = ops.linear(x, w, swiglu=swiglu, act_quant=aq)
        (entry, a), = _linears(calls)
        assert entry == entry_of[route], entry
        return y

    _edge_case(run, M, K, I, BF, route, acts=("swiglu",), quant=quant)
