"""The row kernels of a training step -- RMSNorm, LayerNorm and LayerNorm2d(+GELU) backward (csrc/backward.hip) and the shifted cross
entropy forward / backward (csrc/norm.hip, csrc/backward.hip) -- row by row and column by column against fp64, in bf16 and fp16.
(tests/test_backward_gpu.py holds the same kernels to one relative-L2 figure per tensor at one or two shapes; attention and Linear backward
have files of their own.)

The kernels are called directly (ops.rmsnorm_bwd, layernorm_bwd, layernorm2d_cl_bwd, shifted_cross_entropy_stats / _bwd), not through
autograd_ops: no forward kernel takes part, and widths the forward refuses (D % 8 != 0) reach the backward block kernel.  The launch of
every call is asserted on the C-ABI arguments (`_spy` of test_linear_backward_gpu.py) against `rms_launch`, a restatement of the dispatch
conditions of ull_rmsnorm_bwd_*, and against the table of rows one grid pass reaches (PASS, itself held to the grid clamps in the source of
csrc/backward.hip by a CPU test), so that a changed dispatch rule fails here
instead of emptying a row of the grid:
    wave_dw  rmsnorm_bwd_wave_kernel<true>   D <= 4096, D % 8 == 0, every pitch % 8 == 0, dw asked for: 512 blocks x 4 waves = 2048 rows
    wave     rmsnorm_bwd_wave_kernel<false>  the same without dw: 2048 blocks x 4 waves = 8192 rows
    block    rmsnorm_bwd_kernel              anything else up to D = 8192: 1024 rows
    ln       layernorm_bwd_kernel            D <= 2048: 2048 rows;      ln2d  layernorm2d_cl_bwd_kernel  C <= 512: 4096 x 4 = 16384 rows

Reference: the formula in the comment above each kernel, evaluated in fp64 from the same 16-bit inputs, with the kernel's documented
rounding points (RMSNorm: dw sums dy * rnd(xh), the 16-bit value the forward stored); 16-bit outputs rounded once (helpers.rnd16).

Rules (no new tolerance):
* 16-bit outputs (dx, dlogits): EVERY element |d| <= 2 ulp * max(|ref|, 2 % of max|ref| OF ITS ROW), one ulp = 2^-7 (bf16) / 2^-10 (fp16):
  the suite's 2-ulp rule (helpers.assert_close_bf16, test_fp16_gpu.assert_close_f16) with the floor per row -- the rows carry scales from
  2^-6 to 2^3 and a per-tensor floor would exempt the small ones.  No outlier share.  A row whose reference is zero must be exactly zero.
* fp32 outputs (dw, db): every column |d| <= (n + c) * 2^-24 * sum_r |term[r, c]|, the worst case of an fp32 sum of n terms in any order
  (per-thread partial sums, LDS and global atomics), the terms taken from the fp64 reference; n = the rows whose dy is not zero (all of
  them but in the spike kind: adding an exact 0.0 rounds nothing, and n = rows would let one of four spike terms hide in 2049 roundings).
  c counts the roundings a term has behind it when it enters the sum:
    RMSNorm dw   c = C_SUM = 8.  The kernel's own count is 3: the product dy * rnd(xh) (xh itself is rounded to 16 bits: its fp32 error
                 vanishes, see below), one for the zero-initialised LDS / global atomic stages, one for the second-order terms.  But the
                 spike kind sums n = 4 terms, and the worst case of ANY fp32 evaluation of 4 terms, (3 additions + 1 product) 2^-24,
                 is 2/3 of (4 + 2) 2^-24: no reference can sit at a third of that (CPU check (b)).  c = 8 is the smallest c with n <= (n + c) / 3 at n = 4.  A lost spike term is 1/4 of its column
                 against 12 * 2^-24;
    LN / LN2d db the same c = 8 without GELU (dy enters unrounded).  dw: c = C_STAT = 40, the longest chain of roundings behind dy * xh:
                 the mean's row sum of depth 8 + 6 + 3 = 17 (per-thread loop, wave butterfly, wave partials), 1 / D and its product (2),
                 x - mean (1); rstd at half the relative error of the variance -- d * d (3), the same sum (17), 1 / D, eps, then sqrt
                 and the division: (22 / 2) + 2 = 13; the products (x - mean) rstd and dy xh (2): 35, and the second-order terms.
                 With GELU (dw and db): c = C_GELU = 64 -- w xh + b (2), erff and __expf at a few ulp each, the products of gelu'.
  For dw of LN / LN2d `term` is |dy| (|x - mean| + |mean|) rstd (|gelu'| + ...), not |dy xh| = |dy| |x - mean| rstd: xh inherits the fp32
  error of the mean, 2^-24 |mean|, which is 26 x |x - mean| in the offset kind -- the fp32 recipe of the CPU check below misses the bound
  on |dy xh| there by 2.5 x at D = 255 and 11 x at D = 1280, as any fp32 evaluation must.  In the random and spike kinds |mean| is
  ~ D^-1/2 of |x - mean|: there the bound IS the one on |dy xh|; only the offset kinds are held to the wider term.
  RMSNorm dw, one derived addition: the kernel's fp32 xh can round to the other 16-bit neighbour than the fp64 xh.  An element whose fp64
  xh lies within 8 * 2^-24 relative of a 16-bit rounding boundary (rnd16(xh (1 +- 8 * 2^-24)) != rnd16(xh)) adds |dy| times that step to
  its column's bound.  Nothing else.
* stats[1], the counted tokens: exact.
* stats[0], the loss sum, passes through the fast exp / log intrinsics, whose error is neither derivable nor documented by the project.
  LOSS_SUM_BOUND is 4 x the worst relative deviation |stats[0] - fp64| / fp64 measured over the whole grid on an MI355X (the factor covers
  the atomic order of another run) and must stay <= 2^-12: the largest case counts 40 tokens, one dropped token is 100 x outside.
  MEASURED: 2.7416e-06 (V = 2, one scored token, fp16, random: the token's loss 0.023 is the residue of m + log(s) - logit at 0.68, so
  the fp32 roundings of the three count 30-fold; the fp32 recipe on the CPU deviates by the same 2.742e-06 there), the bound 1.0966e-05.

Kinds of input:
  random  Gaussian x and dy with a power-of-two scale per row: x at 2^-2 .. 2^2, dy at 2^-6 .. 2^3 times the row's x scale, so that the rows
          of dx ~ dy / rms(x) span 2^-6 .. 2^3 (independent scales put whole fp16 dx rows among the subnormals, whose fixed 2^-24 grid is
          0.4 of the rule by itself; LN2d, whose GELU derivative shrinks rows of 8 further, at 2^-3 .. 2^6); the second half of the columns of x doubled, so that a statistic over the first columns only is a
          different number; w = 1 + 0.2 randn, b = 0.1 randn.  Two conditioning limits of the operation itself (CPU check (b)): at D <= 8 |x| is clipped to [0.5, 2] times its scale -- a row in which one
          element carries the whole mean square has dx = g (1 - xh_c^2 / D) ~ 0, a cancellation residue; RMSNorm at D = 1 is that case
          always, dx = g w eps / (x^2 + eps)^1.5, and keeps x at 2^-6, where eps still counts.
  offset1k (LN, LN2d, fp16 only: bf16 has no such values) x = 2000 + k, |k| <= 3 where D is a power of two (1 / D, and with it any fp32
          mean, is exact) and 1024 + k, |k| <= 8 elsewhere (an fp32 mean is off by up to 2^-24 |mean|; further out the fp32 recipe itself
          leaves a third of the rule): the mean 200 .. 1000 deviations away, where a one-pass fp32 variance is off by 0.3 .. 6 %.
  offset  (LN, LN2d) x = 64 + k / 2, integer |k| <= 8 (exact in both types), mean ~ 26 x the deviation: a mean over the wrong count or a
          variance around the wrong mean is grossly off.  dy at 2^-3 .. 2^6 per row (dx ~ dy / 2.5 and less at C = 8: at 2^-6 whole fp16 rows
          of dx are subnormal again); at D <= 8, |k| >= 4 (no lone outlier among near-equal values, the conditioning limit above).
  spike   dy zero except in the first row, the last row of the first grid pass, the first of the second and the last row: dw / db are the
          sum of <= four known terms, dx of every other row exactly zero -- which rows the loop visits.
  edge / edge0 (cross entropy) labels cycle over the columns 0, 63, 64, 255, 256, V - 1 (those below V); every row's maximum is a +40 spike
          over logits of order 1, at column V - 1 (edge) or 0 (edge0), moved to the other end where it would sit on the label (p_label = 1
          leaves dlogits ~ e^-40 relative: a cancellation residue, not a test); one row all-equal logits, one sample all -100, one label
          >= V -- the kernels IGNORE it (pinned here); torch raises IndexError there.
  ignored (cross entropy) every label -100: stats = (0, 0), the loss 0 / 0 = NaN as torch's mean reduction gives, dlogits all zero.
Padded views carry NaN in the pad columns of x and dy / of the logits: a kernel that reads them poisons a row statistic.

The GPU tests carry `@gpu` one by one; the CPU checks at the bottom run under `-m "not gpu"`.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close_bf16, pkg, rnd16
from oracle import ullava_oracle as O
from test_attention_cached_gpu import BF, DTS, FP16, _dtname
from test_fp16_gpu import assert_close_f16
from test_linear_backward_gpu import _spy

gpu = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
ULP = {BF: 2.0 ** -7, FP16: 2.0 ** -10}
U32 = 2.0 ** -24
SFX = {BF: "bf16", FP16: "f16"}
EPS = {"rms": 1e-6, "ln": 1e-5, "ln2d": 1e-6}            # LlamaRMSNorm, torch.nn.LayerNorm, SAM's LayerNorm2d
PASS = {"wave_dw": 2048, "wave": 8192, "block": 1024, "ln": 2048, "ln2d": 16384}      # rows one grid pass reaches (module docstring)
STRIDE = {"wave_dw": 512, "wave": 512, "block": 256, "ln": 256, "ln2d": 64}           # columns the first stride of a row loop covers
C_SUM, C_STAT, C_GELU = 8, 40, 64
NEAR = 8 * U32
LOSS_SUM_MEASURED = 2.7416e-06                 # worst |stats[0] - fp64| / fp64 over the 720 calls of the grid on an MI355X (bf16 and fp16)
LOSS_SUM_BOUND = 4 * LOSS_SUM_MEASURED         # 1.0966e-05 = 2^-16.5
assert LOSS_SUM_BOUND <= 2.0 ** -12


def rms_launch(D, ldx, lddy, lddx, need_dw):
    """the launch ull_rmsnorm_bwd_* picks (csrc/backward.hip; w is a fresh allocation, 16-byte aligned)."""
    if D > 8192:
        return "refused"
    if D <= 4096 and D % 8 == 0 and ldx % 8 == 0 and lddy % 8 == 0 and lddx % 8 == 0:
        return "wave_dw" if need_dw else "wave"
    return "block"


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
# RMSNorm: (rows, D, pad of x, pad of dy, dw asked for, launch)
RMS_CASES = [(r, D, 0, 0, True, "wave_dw") for D in (8, 64) for r in (1, 3, 4, 5, 2047, 2048, 2049, 4100)] + \
            [(r, D, 0, 0, True, "wave_dw") for D in (72, 520, 4088, 4096) for r in (5, 2049)] + \
            [(5, 72, 8, 64, True, "wave_dw"), (2049, 64, 64, 8, True, "wave_dw"), (5, 4096, 8, 64, True, "wave_dw")] + \
            [(8192, 8, 0, 0, False, "wave"), (8193, 8, 0, 0, False, "wave"), (300, 4096, 0, 0, False, "wave"), (5, 72, 64, 8, False, "wave")] + \
            [(3, D, 0, 0, True, "block") for D in (1, 7, 255, 257, 4104, 8191, 8192)] + [(3, 1000, 1, 1, True, "block")] + \
            [(r, 7, 0, 0, True, "block") for r in (1024, 1025, 2049)] + [(1025, 7, 0, 0, False, "block"), (3, 64, 4, 0, True, "block")]
# LayerNorm: (rows, D, pad of x, pad of dy, dw / db asked for)
LN_CASES = [(5, D, 0, 0, True) for D in (1, 8, 255, 256, 257, 1280, 2047, 2048)] + \
           [(r, D, 0, 0, True) for D in (8, 257) for r in (1, 2048, 2049, 4097)] + \
           [(5, 257, 0, 0, False), (2049, 8, 0, 0, False), (5, 1280, 8, 3, True), (2049, 257, 3, 8, True), (5, 256, 1, 0, False)]
# LayerNorm2d: (rows, C, GELU)
LN2D_CASES = [(50, C, g) for C in (8, 64, 72, 128, 256, 504, 512) for g in (False, True)] + \
             [(r, C, g) for C in (8, 64) for r in (1, 5, 16384, 16385, 32771) for g in (False, True)]
CE_V = [2, 50, 63, 64, 65, 255, 256, 257, 1000, 32011]
CE_BS = [(1, 2), (2, 9), (3, 5)]
CE_PAD = 22
CE_GOUT = [1.0, 0.37]
CE_KINDS = ["random", "edge", "edge0", "ignored"]


def _nid(case):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case)


def norm_cases(op):
    return {"rms": RMS_CASES, "ln": LN_CASES, "ln2d": LN2D_CASES}[op]


def launch_of(op, case):
    return case[5] if op == "rms" else op


def kinds_of(op, dt=None):
    """offset1k needs the 11 significant bits of fp16 (1024 + k is not a bf16 value)."""
    return ["random", "spike"] if op == "rms" else ["random", "offset", "spike"] + (["offset1k"] if dt == FP16 else [])


def spike_rows(rows, npass):
    return sorted({0, npass - 1, npass, rows - 1} & set(range(rows)))


# ---- inputs (CPU, shared, never modified) -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def norm_inputs(op, rows, D, dt, kind, npass):
    g = torch.Generator().manual_seed(100003 * rows + 17 * D + {"random": 1, "offset": 2, "spike": 3, "offset1k": 4}[kind] + (5 if op == "ln2d" else 0))
    sx = 2.0 ** torch.randint(-2, 3, (rows, 1), generator=g).float()          # x rows at 2^-2 .. 2^2
    lo = -3 if op == "ln2d" else -6                                           # (LN2d: the GELU's derivative shrinks dx rows of C = 8 further)
    sy = 2.0 ** torch.randint(lo, lo + 10, (rows, 1), generator=g).float()    # dy rows at 2^-6 .. 2^3 times the row's x scale: dx rows at 2^-6 .. 2^3
    if kind == "offset":
        k = torch.randint(-8, 9, (rows, D), generator=g).float()
        if D <= 8:                                                # (no lone outlier among near-equal values: see the docstring on D <= 8)
            k = torch.where(k.abs() < 4, torch.sign(k + 0.5) * (k.abs() + 4), k)
        x = 64.0 + k / 2
    elif kind == "offset1k":
        # D a power of two: 1 / D and with it the fp32 mean are exact: 2000 + k, |k| <= 3 (mean ~ 1000 deviations); any other D: the fp32
        # mean is off by up to 2^-24 |mean|, which 1024 + k, |k| <= 8 (mean ~ 200 deviations) keeps inside a third of the rule (CPU check (b))
        base, K = (2000.0, 3) if D & (D - 1) == 0 else (1024.0, 8)
        k = torch.randint(-K, K + 1, (rows, D), generator=g).float()
        if D <= 8:                                                # (the same: magnitudes 2 .. 3; never all equal -- rstd = eps^-1/2 overflows fp16)
            k = torch.where(k.abs() < 2, torch.sign(k + 0.5) * (k.abs() + 2), k)
            if D > 1:
                k[:, 0], k[:, 1] = 3.0, -2.0
        x = base + k
    else:
        x = torch.randn(rows, D, generator=g)
        if D <= 8:
            x = torch.sign(x) * x.abs().clamp(0.5, 2.0)
        if (op, D) == ("rms", 1):
            sx = torch.full_like(sx, 2.0 ** -6)
        x = x * sx * (1.0 + (2 * torch.arange(D) >= D).float())
    dy = torch.randn(rows, D, generator=g)
    if kind == "spike":
        keep = torch.zeros(rows, 1)
        keep[spike_rows(rows, npass)] = 1.0
        dy = dy * keep
    else:
        dy = dy * sy * (8.0 if kind.startswith("offset") else sx)           # offset: rms(x - mean) ~ 2.5, and at C = 8 the projection and the GELU shrink dx further
    w, b = 1.0 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    return dict(x=x.to(dt), dy=dy.to(dt), w=w.to(dt), b=b.to(dt))


def _rnd(t, dt):
    """the element type's rounding inside a recipe: once from fp64, torch's own cast from fp32."""
    return (rnd16(t, dt) if t.dtype == F64 else t.to(dt)).to(t.dtype)


def _wrong_stats(t, wrong, stride, rules=("stats",)):
    """the columns a row statistic is taken over: all, or (wrong rule) the first stride of the loop only."""
    return t[:, :stride] if wrong in rules and t.shape[1] > stride else t


def _gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def norm_recipe(op, i, dt, ft=F64, wrong=None, npass=None, stride=None, gelu=False):
    """-> dict(dx unrounded, tw / tb: the terms of dw / db [rows, D], mw / mb: their operand magnitudes) in `ft`.
    wrong: None | skip_rows (rows beyond the first grid pass not visited) | drop_dw (the dw / db partial sums of the second pass lost) |
           stats (row statistics over the first stride only) | onepass (variance as E[x^2] - mean^2 in fp32) | count (the mean's sum over
           the first stride, divided by D)."""
    x, dy, w, b = (i[n].to(ft) for n in ("x", "dy", "w", "b"))
    rows, D = x.shape
    eps = EPS[op]
    if op == "rms":
        xs = _wrong_stats(x, wrong, stride, ("stats", "count"))
        r = torch.rsqrt((xs * xs).sum(-1, keepdim=True) / (D if wrong == "count" else xs.shape[1]) + eps)
        xh = x * r
        g = dy * w
        dot = _wrong_stats(g * xh, wrong, stride).mean(-1, keepdim=True)
        dx = r * (g - xh * dot)
        tw = dy * _rnd(xh, dt)
        out = dict(dx=dx, tw=tw, mw=tw.abs(), xh=xh)
    else:
        xs = _wrong_stats(x, wrong, stride, ("stats", "count"))
        mean = xs.sum(-1, keepdim=True) / (D if wrong == "count" else xs.shape[1])
        if wrong == "onepass":
            x32 = x.to(F32)
            var = ((x32 * x32).mean(-1, keepdim=True) - x32.mean(-1, keepdim=True) ** 2).to(ft)
        else:
            var = ((_wrong_stats(x, wrong, stride) - mean) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        xh = (x - mean) * rstd
        mxh = ((x - mean).abs() + mean.abs()) * rstd
        if gelu:
            z = w * xh + b
            gp = _gelu_grad(z)
            zz = z.double()
            mgp = (0.5 * (1.0 + torch.erf(zz * math.sqrt(0.5)).abs()) + zz.abs() * torch.exp(-0.5 * zz * zz) / math.sqrt(2.0 * math.pi)
                   + 0.8 * (w.double().abs() * mxh.double() + b.double().abs())).to(ft)       # |gelu''| <= 0.8: the error of z carried through
            g0 = dy * gp
        else:
            g0, mgp = dy, None
        g = g0 * w
        a = _wrong_stats(g, wrong, stride).mean(-1, keepdim=True)
        bs = _wrong_stats(g * xh, wrong, stride).mean(-1, keepdim=True)
        dx = rstd * (g - a - xh * bs)
        tw, tb = g0 * xh, g0
        if gelu:
            mb = dy.abs() * mgp
            mw = dy.abs() * (mgp * xh.abs() + gp.abs() * mxh)
        else:
            mb, mw = tb.abs(), dy.abs() * mxh
        out = dict(dx=dx, tw=tw, tb=tb, mw=mw, mb=mb)
    if wrong == "skip_rows":
        for n in ("dx", "tw", "tb"):
            if n in out:
                out[n] = out[n].clone()
                out[n][npass:] = 0.0
    if wrong == "drop_dw":
        for n in ("tw", "tb"):
            if n in out:
                out[n] = out[n].clone()
                out[n][npass:2 * npass] = 0.0
    return out


def _nnz(term, dy=None):
    """n of the bound per column: the rows whose term is not an exact zero (dy == 0: the kernel adds an exact 0.0, which rounds nothing)."""
    return ((term if dy is None else dy) != 0).sum(0).double()


@functools.lru_cache(maxsize=3)
def norm_reference(op, case, dt, kind):
    """-> dict(dx: fp64 rounded once to dt, dw / db fp64 [D], bw / bb: their bounds [D])."""
    rows, D = case[0], case[1]
    launch = launch_of(op, case)
    gelu = op == "ln2d" and case[2]
    i = norm_inputs(op, rows, D, dt, kind, PASS[launch])
    r = norm_recipe(op, i, dt, gelu=gelu)
    ref = dict(dx=rnd16(r["dx"], dt).double(), dw=r["tw"].sum(0))
    if op == "rms":
        bw = (_nnz(r["tw"]) + C_SUM) * U32 * r["mw"].sum(0)
        xh, q0 = r["xh"], rnd16(r["xh"], dt).double()
        step = torch.maximum((rnd16(xh * (1.0 + NEAR), dt).double() - q0).abs(), (rnd16(xh * (1.0 - NEAR), dt).double() - q0).abs())
        ref["bw"] = bw + (i["dy"].double().abs() * step).sum(0)
        ref["bw0"], ref["near"], ref["q0"] = bw, step > 0, q0.float()
    else:
        ref["bw"] = (_nnz(r["tw"], dy=i["dy"]) + (C_GELU if gelu else C_STAT)) * U32 * r["mw"].sum(0)
        ref["db"] = r["tb"].sum(0)
        ref["bb"] = (_nnz(r["tb"]) + (C_GELU if gelu else C_SUM)) * U32 * r["mb"].sum(0)
    return ref


# ---- the rules as numbers ---------------------------------------------------------------------------------------------------------------
def _ratio(err, tol):
    """err / tol elementwise; a zero tolerance admits a zero error only."""
    return torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def rule16(got, ref, dt):
    """[rows, D] doubles -> (worst |d| / tol, [rows] 'an element of this row is beyond the rule'); NaN counts as beyond."""
    fl = 0.02 * ref.abs().amax(-1, keepdim=True)
    q = _ratio((got - ref).abs(), 2.0 * ULP[dt] * torch.maximum(ref.abs(), fl))
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max()), (q > 1.0).any(-1)


def rule32(got, ref, bound):
    """[D] doubles -> (worst |d| / bound, [D] 'this column is beyond its bound')."""
    q = _ratio((got.double() - ref).abs(), bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max()), q > 1.0


def assert_rule16(got, ref, dt, what):
    worst, rows = rule16(got.double(), ref, dt)
    print(f"[row-bwd] {what}: worst |d| / (2 ulp max(|ref|, row floor)) = {worst:.3f}")
    assert not bool(rows.any()), f"{what}: {int(rows.sum())} of {rows.numel()} rows hold an element beyond the rule (worst {worst:.3f}); first row {int(rows.nonzero()[0])}"


def assert_rule32(got, ref, bound, what):
    assert got.dtype == F32 and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    worst, cols = rule32(got, ref, bound)
    print(f"[row-bwd] {what}: worst |d| / bound = {worst:.3f}")
    assert not bool(cols.any()), f"{what}: {int(cols.sum())} of {cols.numel()} columns beyond the fp32 bound (worst {worst:.3f}); first column {int(cols.nonzero()[0])}"


# ---- running the norm kernels -----------------------------------------------------------------------------------------------------------
def _padded(t, pad):
    """the [rows, D] tensor as a view of NaN-padded rows on the device."""
    if pad == 0:
        return t.to(DEV)
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    v = buf.to(DEV)[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + pad
    return v


def run_norm(op, case, i):
    """-> (dx, dw, db) on the CPU (None where not asked for); asserts the launch on the C-ABI arguments."""
    ops = pkg("ops")
    rows, D = case[0], case[1]
    dt = i["x"].dtype
    w, b = i["w"].to(DEV), i["b"].to(DEV)
    with _spy() as calls:
        if op == "rms":
            x, dy = _padded(i["x"], case[2]), _padded(i["dy"], case[3])
            dx, dw = ops.rmsnorm_bwd(x, w, dy, EPS[op], need_dw=case[4])
            db, need = None, case[4]
        elif op == "ln":
            x, dy = _padded(i["x"], case[2]), _padded(i["dy"], case[3])
            dx, dw, db = ops.layernorm_bwd(x, w, dy, EPS[op], need_wb=case[4])
            need = case[4]
        else:
            dx, dw, db = ops.layernorm2d_cl_bwd(i["x"].to(DEV), w, b, i["dy"].to(DEV), EPS[op], case[2])
            need = True
    torch.cuda.synchronize()
    entry = {"rms": "ull_rmsnorm_bwd_", "ln": "ull_layernorm_bwd_", "ln2d": "ull_layernorm2d_cl_bwd_"}[op] + SFX[dt]
    assert [n for n, _ in calls] == [entry], [n for n, _ in calls]
    a = calls[0][1]
    if op == "ln2d":
        assert (a[7], a[8], a[10]) == (rows, D, int(case[2])) and a[5] is not None and a[6] is not None, a
    else:
        assert (a[1], a[4], a[6]) == (D + case[2], D + case[3], D), f"pitches {a[1]}, {a[4]}, {a[6]}"
        assert (a[7] is not None) == need and ((a[9], a[10]) == (rows, D) if op == "ln" else (a[8], a[9]) == (rows, D)), a
        if op == "ln":
            assert (a[8] is not None) == need
        else:
            assert rms_launch(D, a[1], a[4], a[6], a[7] is not None) == case[5], f"{_nid(case)}: laid out for the {case[5]} launch"
    assert dx.dtype == dt and tuple(dx.shape) == (rows, D)
    assert (dw is not None) == need and (db is not None) == (need and op != "rms")
    return dx.cpu(), None if dw is None else dw.cpu(), None if db is None else db.cpu()


def _check_norm(op, case, dt):
    rows, D = case[0], case[1]
    launch = launch_of(op, case)
    for kind in kinds_of(op, dt):
        i = norm_inputs(op, rows, D, dt, kind, PASS[launch])
        ref = norm_reference(op, case, dt, kind)
        dx, dw, db = run_norm(op, case, i)
        what = f"{op} {_nid(case)} {_dtname(dt)} {kind}"
        assert_rule16(dx, ref["dx"], dt, what + " dx")
        if kind == "spike":
            quiet = torch.ones(rows, dtype=torch.bool)
            quiet[spike_rows(rows, PASS[launch])] = False
            assert not bool(dx[quiet].float().abs().sum() != 0), f"{what}: dx of a row with dy = 0 must be exactly zero"
        if dw is not None:
            assert_rule32(dw, ref["dw"], ref["bw"], what + " dw")
        if db is not None:
            assert_rule32(db, ref["db"], ref["bb"], what + " db")


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", RMS_CASES, ids=_nid)
def test_rmsnorm_backward(case, dt):
    """all three launches: rows around the 4 waves of a block and around one and two grid passes, widths around the 64-lane chunk stride,
    the 4096 limit of the wave kernels and the 8192 limit of the block kernel, NaN-padded pitches, with and without dw."""
    _check_norm("rms", case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", LN_CASES, ids=_nid)
def test_layernorm_backward(case, dt):
    """1 to 8 columns per thread with ragged last strides, rows around one and two grid passes, NaN-padded pitches, with and without dw / db."""
    _check_norm("ln", case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", LN2D_CASES, ids=_nid)
def test_layernorm2d_backward(case, dt):
    """1 to 8 columns per lane, rows around the 4 waves of a block and around one and two grid passes, with and without the GELU."""
    _check_norm("ln2d", case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_widths_beyond_the_kernels_are_refused(dt):
    """D = 8193 (RMSNorm), 2049 (LayerNorm) and C = 520 (LayerNorm2d) raise the library's shape error; the entry returns before any launch."""
    ops = pkg("ops")
    mk = lambda *s: torch.ones(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):
        ops.rmsnorm_bwd(mk(3, 8193), mk(8193), mk(3, 8193), 1e-6)
    assert rms_launch(8193, 8193, 8193, 8193, True) == "refused"
    with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):
        ops.layernorm_bwd(mk(3, 2049), mk(2049), mk(3, 2049), 1e-5)
    with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):
        ops.layernorm2d_cl_bwd(mk(3, 520), mk(520), mk(520), mk(3, 520), 1e-6, True)
    torch.cuda.synchronize()


@gpu
def test_the_rule_is_the_suites_rule():
    """on a single-scale tensor the per-row rule implies helpers.assert_close_bf16 / test_fp16_gpu.assert_close_f16 (their floor is per
    tensor, hence larger): one plain case through the suite's own assertions."""
    case = (5, 256, 0, 0, True)
    for dt in DTS:
        i = norm_inputs("ln", 5, 256, dt, "offset", PASS["ln"])
        dx, _, _ = run_norm("ln", case, i)
        (assert_close_bf16 if dt == BF else assert_close_f16)(dx, norm_reference("ln", case, dt, "offset")["dx"], ulps=2.0, what=f"ln offset {_dtname(dt)}")


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------------
def _edge_cols(V):
    return [c for c in (0, 63, 64, 255, 256) if c < V - 1] + [V - 1]


@functools.lru_cache(maxsize=8)
def ce_inputs(V, B, S, dt, kind):
    """-> (logits [B, S, V] of dt, labels [B, S] int64).  Row (b, t) is scored against labels[b, t + 1]."""
    g = torch.Generator().manual_seed(7919 * V + 31 * B + S + {"random": 0, "edge": 1, "edge0": 2, "ignored": 3}[kind])
    logits = torch.randn(B, S, V, generator=g) * (2.0 if kind == "random" else 1.0)
    labels = torch.randint(0, V, (B, S), generator=g)
    if kind == "random":
        if B * S > 4:
            labels[0, :3] = -100
    elif kind == "ignored":
        labels[:] = -100
    else:
        cols = _edge_cols(V)
        n = 0
        for b in range(B):
            for t in range(S - 1):
                lab = cols[n % len(cols)]
                spike = V - 1 if (kind == "edge") else 0
                if spike == lab:
                    spike = V - 1 - spike
                logits[b, t, spike] += 40.0
                labels[b, t + 1] = lab
                n += 1
        if B * (S - 1) >= 8:
            logits[0, S - 2] = 0.5                               # all-equal logits: loss log V, dlogits 1 / V off the label
            labels[B - 1, :] = -100                              # one sample without a counted token
            labels[0, 2] = V + 3                                 # a label >= V: ignored by the kernels
    return logits.to(dt), labels


def _ce_short(t, wrong, stride):
    """the columns a row loop covers: all, or (wrong rule) those before the ragged last stride."""
    V = t.shape[-1]
    return t[..., :V // stride * stride] if wrong == "short" and V > stride and V % stride else t


def ce_recipe(logits, labels, gout, ft=F64, wrong=None):
    """-> dict(tok: the counted per-token losses [B, S-1] (zero where not counted), n: counted tokens, dl: dlogits [B, S, V] unrounded).
    wrong = "short": the sum of exponentials misses the ragged last stride (64 lanes forward, 256 threads backward).  A maximum that
    misses it changes nothing by itself (the softmax is shift invariant; e^40 does not overflow)."""
    B, S, V = logits.shape
    l = logits.to(ft)[:, :-1]
    lab = labels[:, 1:]
    counted = (lab >= 0) & (lab < V)
    m = l.amax(-1, keepdim=True)
    e = torch.exp(l - m)
    lse_f = m[..., 0] + torch.log(_ce_short(e, wrong, 64).sum(-1))
    tok = (lse_f - l.gather(-1, lab.clamp(0, V - 1)[..., None])[..., 0]) * counted
    n = int(counted.sum())
    p = e / _ce_short(e, wrong, 256).sum(-1, keepdim=True)
    onehot = F.one_hot(lab.clamp(0, V - 1), V).to(ft)
    dl = torch.zeros(B, S, V, dtype=ft)
    if n:
        dl[:, :-1] = (p - onehot) * (gout / n) * counted[..., None]
    return dict(tok=tok, n=n, dl=dl)


def _ce_view(logits, pad):
    B, S, V = logits.shape
    if pad == 0:
        return logits.to(DEV)
    buf = torch.full((B, S, V + pad), float("nan"), dtype=logits.dtype)
    buf[..., :V] = logits
    v = buf.to(DEV)[..., :V]
    assert not v.is_contiguous() and v.stride() == (S * (V + pad), V + pad, 1)
    return v


def _check_ce(V, dt):
    ops = pkg("ops")
    for B, S in CE_BS:
        for kind in CE_KINDS:
            logits, labels = ce_inputs(V, B, S, dt, kind)
            for pad in (0, CE_PAD):
                lg, lb = _ce_view(logits, pad), labels.to(DEV)
                for gout in CE_GOUT:
                    what = f"ce V{V} b{B}s{S} {_dtname(dt)} {kind} pitch {V + pad} gout {gout}"
                    ref = ce_recipe(logits, labels, gout)
                    with _spy() as calls:
                        st = ops.shifted_cross_entropy_stats(lg, lb)
                        dl = ops.shifted_cross_entropy_bwd(lg, lb, st, torch.tensor([gout], device=DEV))
                    torch.cuda.synchronize()
                    assert [n for n, _ in calls] == ["ull_shifted_cross_entropy_" + SFX[dt], "ull_shifted_cross_entropy_bwd_" + SFX[dt]]
                    for _, a in calls:
                        assert (a[1], a[3], a[4], a[5]) == (V + pad, B, S, V), a
                    assert dl.dtype == dt and tuple(dl.shape) == (B, S, V) and dl.stride() == (S * (V + pad), V + pad, 1), dl.stride()
                    st = st.cpu()
                    assert st.dtype == F32 and float(st[1]) == ref["n"], f"{what}: counted {float(st[1])}, expected {ref['n']}"
                    s64 = float(ref["tok"].sum())
                    if ref["n"] == 0:
                        assert float(st[0]) == 0.0
                        assert bool(torch.isnan(ops.shifted_cross_entropy(lg, lb))), f"{what}: the loss of no counted token is 0 / 0"
                    else:
                        dev = abs(float(st[0]) - s64) / s64
                        print(f"[row-bwd] {what}: |stats[0] - fp64| / fp64 = {dev:.3e} (bound {LOSS_SUM_BOUND:.3e})")
                        assert dev <= LOSS_SUM_BOUND, f"{what}: loss sum {float(st[0])!r}, fp64 {s64!r}: {dev:.3e} relative"
                        loss = ops.shifted_cross_entropy(lg, lb)
                        assert loss.dtype == dt and loss.dim() == 0
                        assert_rule16(loss.cpu().reshape(1, 1), torch.tensor([[s64 / ref["n"]]], dtype=F64), dt, what + " loss")
                    got = dl.cpu()
                    assert bool(torch.isfinite(got.float()).all()), f"{what}: dlogits holds unwritten or non-finite elements"
                    assert_rule16(got.reshape(B * S, V), rnd16(ref["dl"], dt).double().reshape(B * S, V), dt, what + " dlogits")
                    if ref["n"] == 0:
                        assert not bool(got.float().abs().sum() != 0)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("V", CE_V, ids=lambda v: f"V{v}")
def test_shifted_cross_entropy_forward_and_backward(V, dt):
    """widths around the 64-lane stride of the forward and the 256-thread stride of the backward, the real model's ragged 32011; 1 to 16
    scored rows (the forward's 4 rows per block); exact and padded pitch; two upstream gradients; every kind."""
    _check_ce(V, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_shifted_cross_entropy_refuses_rows_of_two_pitches(dt):
    """a [B, :S] view of longer sequences has a batch stride that is not S row pitches: the kernels would read other rows; all three
    wrappers refuse it by ops._rows' message before any launch."""
    ops = pkg("ops")
    B, S, V = 2, 5, 50
    buf = torch.zeros(B, S + 1, V, dtype=dt, device=DEV)
    lb = torch.zeros(B, S, dtype=torch.int64, device=DEV)
    view = buf[:, :S]
    assert not view.is_contiguous()
    st, one = torch.ones(2, device=DEV), torch.ones(1, device=DEV)
    with _spy() as calls:
        for fn in (lambda: ops.shifted_cross_entropy_stats(view, lb), lambda: ops.shifted_cross_entropy(view, lb),
                   lambda: ops.shifted_cross_entropy_bwd(view, lb, st, one)):
            with pytest.raises(RuntimeError, match="one common pitch"):
                fn()
    assert calls == []


# ---- CPU: the recipes, the bounds and the inputs themselves -----------------------------------------------------------------------------
_BIG = {"rms-2049x4088": (2049, 4088), "rms-2049x4096": (2049, 4096)}        # a few seconds each: tests of their own
NORM_PARTS = ["rms", *_BIG, "ln", "ln2d"]


def part_cases(part):
    """-> (op, its cases of that part); "rms": every RMSNorm case but the two big ones."""
    op = part.split("-")[0]
    return op, [c for c in norm_cases(op) if (c[:2] == _BIG[part] if part in _BIG else c[:2] not in _BIG.values())]


def test_the_grid_tables_are_the_kernels_grids():
    """PASS restates the launch grids of csrc/backward.hip: the clamps are looked up in the source, so that a changed grid fails here
    instead of silently moving the 'second pass' cases into the first."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "u-llava_amd", "csrc", "backward.hip")).read()
    for launch, clamp, per_block in (("wave_dw", "dim3(wb < 512 ? wb : 512)", 4), ("wave", "(rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048", 4),
                                     ("block", "rows < 1024 ? rows : 1024", 1), ("ln", "rows < 2048 ? rows : 2048", 1),
                                     ("ln2d", "want < 4096 ? want : 4096", 4)):
        assert clamp in src, f"{launch}: the grid clamp `{clamp}` is gone from backward.hip"
        assert PASS[launch] == int(clamp.rsplit(" ", 1)[1].rstrip(")")) * per_block
    assert "constexpr int RN_MAXC = 32;" in src and "constexpr int LN_MAXC = 8;" in src and "constexpr int NCH = 8;" in src


def _autograd_norm(op, i, gelu):
    """torch autograd in fp64 of the forward each kernel differentiates -> (dx, dw, db or None).  RMSNorm: the oracle's rms_norm formula in
    fp64 (O.rms_norm itself computes in fp32 and rounds xh to the input type: held against this on one shape below)."""
    x, w, b = (i[n].double().requires_grad_(True) for n in ("x", "w", "b"))
    D = x.shape[1]
    if op == "rms":
        y = w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS[op]))
    elif op == "ln":
        y = F.layer_norm(x, (D,), w, b, EPS[op])
    else:
        y = F.layer_norm(x, (D,), w, b, EPS[op])
        y = F.gelu(y) if gelu else y
    y.backward(i["dy"].double())
    return x.grad, w.grad, None if op == "rms" else b.grad


def _close64(a, b, what, rtol=1e-9, atol=1e-300):
    scale = b.abs().amax(-1, keepdim=True) if b.dim() == 2 else b.abs().max()
    assert bool(((a - b).abs() <= rtol * scale + atol).all()), f"{what}: {float(((a - b).abs() / (scale + 1e-300)).max()):.3e}"


@pytest.mark.parametrize("part", NORM_PARTS)
def test_the_fp64_recipes_are_torch_autograd(part):
    """(a) the formula itself: the fp64 recipe against torch autograd in fp64 on every shape (bf16 inputs; RMSNorm's dw with xh unrounded --
    the rounding of xh is the forward's storage format, not part of the derivative).  D = 1 RMSNorm: dx is a cancellation residue of
    relative size eps / x^2, held to 1e-6 of itself."""
    seen = set()
    op, cases = part_cases(part)
    for case in cases:
        rows, D = case[0], case[1]
        gelu = op == "ln2d" and case[2]
        if (rows, D, gelu) in seen:
            continue
        seen.add((rows, D, gelu))
        for kind in kinds_of(op, FP16):
            dt = FP16 if kind == "offset1k" else BF
            i = norm_inputs(op, rows, D, dt, kind, PASS[launch_of(op, case)])
            r = norm_recipe(op, i, dt, gelu=gelu)
            dx, dw, db = _autograd_norm(op, i, gelu)
            what = f"{op} {_nid(case)} {kind}"
            # (atol: the fp64 rounding of g rstd where dx is zero by identity -- LayerNorm at D = 1)
            _close64(r["dx"], dx, what + " dx", rtol=1e-6 if (op, D) == ("rms", 1) else 1e-9, atol=1e-13 * float(i["dy"].double().abs().max()) * EPS[op] ** -0.5)
            if op == "rms":
                _close64((i["dy"].double() * r["xh"]).sum(0), dw, what + " dw")
                assert bool(((r["tw"] - i["dy"].double() * r["xh"]).abs() <= ULP[BF] * (i["dy"].double() * r["xh"]).abs()).all())
            else:
                _close64(r["tw"].sum(0), dw, what + " dw", atol=1e-12 * float(r["mw"].sum(0).max()))
                _close64(r["tb"].sum(0), db, what + " db")


def test_the_rmsnorm_recipe_is_the_oracles_rms_norm():
    """O.rms_norm (fp32 arithmetic, xh rounded to the input type before the weight) differentiated by torch on bf16 inputs: dw is the sum of
    dy * rnd(xh) -- the recipe's rounding point -- up to fp32."""
    i = norm_inputs("rms", 5, 72, BF, "random", PASS["wave_dw"])
    x, w = i["x"].clone().requires_grad_(True), i["w"].float().requires_grad_(True)
    O.rms_norm(x, w, EPS["rms"]).backward(i["dy"].float())
    r = norm_recipe("rms", i, BF)
    assert bool(((w.grad.double() - r["tw"].sum(0)).abs() <= 8 * U32 * r["mw"].sum(0) + ULP[BF] * r["mw"].amax(0)).all())


def test_the_cross_entropy_recipe_is_torch_autograd():
    """(a) for the cross entropy: F.cross_entropy on the shifted slices in fp64, every shape and kind.  torch raises on a label >= V (checked);
    the kernels ignore it, so it is -100 for torch.  All ignored: torch gives loss NaN and a zero gradient -- what the kernels are pinned to."""
    for V in CE_V:
        for B, S in CE_BS:
            for kind in CE_KINDS:
                logits, labels = ce_inputs(V, B, S, BF, kind)
                if bool((labels[:, 1:] >= V).any()):
                    with pytest.raises(IndexError):
                        F.cross_entropy(logits.double()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1))
                lab = torch.where(labels >= V, torch.full_like(labels, -100), labels)
                ls = logits.double().requires_grad_(True)
                loss = F.cross_entropy(ls[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1))
                (loss * 0.37).backward()
                r = ce_recipe(logits, labels, 0.37)
                what = f"ce V{V} b{B}s{S} {kind}"
                if r["n"] == 0:
                    assert bool(torch.isnan(loss)) and not bool(ls.grad.abs().sum() != 0) and not bool(r["dl"].abs().sum() != 0), what
                else:
                    assert abs(float(r["tok"].sum()) / r["n"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach())), what
                    _close64(r["dl"].reshape(B * S, V), ls.grad.reshape(B * S, V), what + " dlogits", rtol=1e-12)


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("part", NORM_PARTS + ["ce"])
def test_the_fp32_recipes_stay_inside_a_third_of_every_bound(part, dt):
    """(b) the bounds are conditions the reference meets on its own, not measurements of the kernels: the same recipes with every operation
    in fp32 (torch on the CPU), taken before their 16-bit outputs are rounded, stay within a third of the rule in every element of dx /
    dlogits and within a third of the bound in every column of dw / db, on every case and kind.  The loss sum in fp32 is printed against
    LOSS_SUM_BOUND; that bound is a measurement of the intrinsics by construction (module docstring) and is asserted at full size here."""
    top = {}
    for op, cases in [part_cases(part)] if part != "ce" else []:
        for case in cases:
            rows, D = case[0], case[1]
            gelu = op == "ln2d" and case[2]
            for kind in kinds_of(op, dt):
                i = norm_inputs(op, rows, D, dt, kind, PASS[launch_of(op, case)])
                ref = norm_reference(op, case, dt, kind)
                r = norm_recipe(op, i, dt, ft=F32, gelu=gelu)
                fig = {"dx": rule16(r["dx"].double(), ref["dx"], dt)[0]}
                if op == "rms":
                    # a flipped rnd(xh) is all or nothing (|dy| times the step, the whole allowance of that element): the fp32 recipe may flip
                    # only inside the window (its xh error is printed as a share of the window: torch's fp32 x * rsqrt(mean) uses 0.42 of it);
                    # with the fp64 roundings put back, the sum stays within a third of the bound proper
                    q32 = r["xh"].to(dt).float()
                    assert not bool(((q32 != ref["q0"]) & ~ref["near"]).any()), (op, _nid(case), kind, "rnd(xh) flipped outside the window")
                    x64 = norm_recipe(op, i, dt)["xh"]
                    fig["xh"] = float(((r["xh"].double() - x64).abs() / x64.abs().clamp_min(1e-300)).max()) / NEAR
                    fig["dw"] = rule32((i["dy"].float() * ref["q0"]).sum(0), ref["dw"], ref["bw0"])[0]
                    assert rule32(r["tw"].sum(0), ref["dw"], ref["bw"])[0] <= 1.0
                else:
                    fig["dw"] = rule32(r["tw"].sum(0), ref["dw"], ref["bw"])[0]
                    fig["db"] = rule32(r["tb"].sum(0), ref["db"], ref["bb"])[0]
                for n, v in fig.items():
                    top[(op, n)] = max(top.get((op, n), 0.0), v)
                    assert v <= (1.0 if n == "xh" else 1 / 3), (op, _nid(case), kind, n, v)     # xh: the share of the window's half width used
    worst_loss = 0.0
    for V in CE_V if part == "ce" else []:
        for B, S in CE_BS:
            for kind in CE_KINDS:
                logits, labels = ce_inputs(V, B, S, dt, kind)
                ref, r = ce_recipe(logits, labels, 0.37), ce_recipe(logits, labels, 0.37, ft=F32)
                v = rule16(r["dl"].double().reshape(B * S, V), rnd16(ref["dl"], dt).double().reshape(B * S, V), dt)[0]
                top[("ce", "dlogits")] = max(top.get(("ce", "dlogits"), 0.0), v)
                assert v <= 1 / 3, (V, B, S, kind, v)
                if ref["n"]:
                    s64 = float(ref["tok"].sum())
                    worst_loss = max(worst_loss, abs(float(r["tok"].sum()) - s64) / s64)
    for key, v in sorted(top.items()):
        print(f"[row-bwd] {_dtname(dt)} fp32 recipe against fp64, {key[0]} {key[1]}: worst |d| / bound {v:.3f}")
    if part == "ce":
        print(f"[row-bwd] {_dtname(dt)} fp32 recipe, loss sum: worst relative deviation {worst_loss:.3e} (bound {LOSS_SUM_BOUND:.3e})")
        assert worst_loss <= LOSS_SUM_BOUND


def _exposed(op, case, dt, wrong):
    """union over the kinds -> ([rows] dx rows, [D] dw columns, [D] db columns or None) that leave the rule under the wrong recipe."""
    rows, D = case[0], case[1]
    launch = launch_of(op, case)
    gelu = op == "ln2d" and case[2]
    rx, cw, cb = torch.zeros(rows, dtype=torch.bool), torch.zeros(D, dtype=torch.bool), torch.zeros(D, dtype=torch.bool)
    for kind in kinds_of(op, dt):
        i = norm_inputs(op, rows, D, dt, kind, PASS[launch])
        ref = norm_reference(op, case, dt, kind)
        r = norm_recipe(op, i, dt, wrong=wrong, npass=PASS[launch], stride=STRIDE[launch], gelu=gelu)
        rx |= rule16(rnd16(r["dx"], dt).double(), ref["dx"], dt)[1]
        cw |= rule32(r["tw"].sum(0), ref["dw"], ref["bw"])[1]
        if op != "rms":
            cb |= rule32(r["tb"].sum(0), ref["db"], ref["bb"])[1]
    return rx, cw, cb


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("part", NORM_PARTS + ["ce"])
def test_the_inputs_expose_wrong_row_loops_and_wrong_statistics(part, dt):
    """(c) guards the inputs and the rules, not the kernels: the fp64 recipe run with a deliberately wrong rule must leave the rule in every
    row / column the error touches, the kinds taken together, on every shape that reaches the path:
      skip_rows  rows beyond the first grid pass not visited (rows > one pass): every such dx row, every dw / db column;
      drop_dw    the dw / db partial sums of the second pass lost (rows > one pass): every dw / db column (dx untouched);
      stats      row statistics over the first stride only (D > 512 wave, 256 block / ln, 64 ln2d): where the stride is at most half the
                 row, every dx row and every dw column; below that, caught in some row or column (one Gaussian column of 257 moves r by
                 0.2 %, a fifth of a bf16 ulp, and RMSNorm's dw sums the ROUNDED xh: most elements cannot show it and need not);
      count      LN / LN2d: the mean's sum over the first stride divided by D: every dw column and some dx row (the offset kind.  dx is
                 nearly blind to a shifted mean: the shift enters through mean(g) and mean(g xh), both ~ D^-1/2 of g);
      short      cross entropy: the sum of exponentials misses the ragged last stride: every scored row whose maximum sits there (edge),
                 and the loss sum.
      onepass    LN / LN2d: the variance as E[x^2] - mean^2 in fp32.  The cancellation costs about 2^-24 (mean / deviation)^2 of the variance.
                 fp16 (11 significant bits) can put the mean 200 .. 1000 deviations away: the offset1k kind, on which some dx row of every
                 fp16 shape with D > 1 and at least 5 rows must leave the rule (three quarters of all rows do; a shape of a single row is
                 a single draw and is only counted).  bf16 (8 bits) cannot put it further than ~2^7 deviations: at most 2^-10 of the
                 variance, below the bf16 rule, so for bf16 the count is printed and nothing is required -- a limit of bf16 inputs."""
    gaps, onepass = [], [0, 0]
    for op, cases in [part_cases(part)] if part != "ce" else []:
        for case in cases:
            rows, D = case[0], case[1]
            launch = launch_of(op, case)
            has_w = case[4] if op != "ln2d" else True
            npass, stride = PASS[launch], STRIDE[launch]
            tag = f"{op} {_nid(case)} {_dtname(dt)}"
            if rows > npass:
                rx, cw, cb = _exposed(op, case, dt, "skip_rows")
                if not bool(rx[npass:].all()):
                    gaps.append(f"{tag} skip_rows: {int((~rx[npass:]).sum())} dx rows")
                if has_w and not (bool(cw.all()) and (op == "rms" or bool(cb.all()))):
                    gaps.append(f"{tag} skip_rows: {int((~cw).sum())} dw, {int((~cb).sum())} db columns")
                rx, cw, cb = _exposed(op, case, dt, "drop_dw")
                if has_w and not (bool(cw.all()) and (op == "rms" or bool(cb.all()))):
                    gaps.append(f"{tag} drop_dw: {int((~cw).sum())} dw, {int((~cb).sum())} db columns")
            if D > stride:
                rx, cw, cb = _exposed(op, case, dt, "stats")
                if D >= 2 * stride:
                    if not bool(rx.all()) or (has_w and not bool(cw.all())):
                        gaps.append(f"{tag} stats: {int((~rx).sum())} dx rows, {int((~cw).sum())} dw columns")
                elif not (bool(rx.any()) or (has_w and bool(cw.any()))):
                    gaps.append(f"{tag} stats: not caught")
                if op != "rms":
                    rx, cw, cb = _exposed(op, case, dt, "count")
                    if (has_w and not bool(cw.all())) or not bool(rx.any()):
                        gaps.append(f"{tag} count: {int((~rx).sum())} dx rows, {int((~cw).sum())} dw columns")
            if op != "rms" and D > 1:
                kind = "offset1k" if dt == FP16 else "offset"
                i = norm_inputs(op, rows, D, dt, kind, npass)
                r = norm_recipe(op, i, dt, wrong="onepass", gelu=op == "ln2d" and case[2])
                hit = rule16(rnd16(r["dx"], dt).double(), norm_reference(op, case, dt, kind)["dx"], dt)[1]
                onepass[0] += int(hit.sum())
                onepass[1] += rows
                if dt == FP16 and rows >= 5 and not bool(hit.any()):
                    gaps.append(f"{tag} onepass: no dx row of {rows}")
    print(f"[row-bwd] {_dtname(dt)} {part} one-pass fp32 variance, {'offset1k' if dt == FP16 else 'offset'} kind: {onepass[0]} of {onepass[1]} dx rows leave the rule")
    for V in CE_V if part == "ce" else []:
        for B, S in CE_BS:
            logits, labels = ce_inputs(V, B, S, dt, "edge")
            ref, bad = ce_recipe(logits, labels, 1.0), ce_recipe(logits, labels, 1.0, wrong="short")
            scored = (ref["tok"] != 0).reshape(-1)
            spike_last = (logits[:, :-1].float().argmax(-1) == V - 1).reshape(-1) & scored
            if V > 256 and V % 256:
                rows = rule16(rnd16(bad["dl"], dt).double()[:, :-1].reshape(-1, V), rnd16(ref["dl"], dt).double()[:, :-1].reshape(-1, V), dt)[1]
                if not bool(spike_last.any()) or not bool(rows[spike_last].all()):
                    gaps.append(f"ce V{V} b{B}s{S} short: {int((spike_last & ~rows).sum())} of {int(spike_last.sum())} dlogits rows")
            if V > 64 and V % 64:
                s64 = float(ref["tok"].sum())
                if not bool(spike_last.any()) or abs(float(bad["tok"].sum()) - s64) / s64 <= 2.0 ** -12:
                    gaps.append(f"ce V{V} b{B}s{S} short: the loss sum stays inside 2^-12")
    assert not gaps, f"{len(gaps)} gaps ({_dtname(dt)}):\n" + "\n".join(gaps[:40])
