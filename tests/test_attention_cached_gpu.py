"""Cached attention with many new queries: the causal offset koff = Sk - Sq, key masks and the dispatch edges of `ull_attention_*`,
the RoPE + cache append with many rows, and a continuation `forward()` against the one-shot prefill.

A continuation (a second chat turn, a prompt fed in pieces) calls the attention with Sq = S new tokens, Sk = past + S keys, causal, K and
the V^T image read from the cache at cache strides.  Every kernel offsets the causal diagonal by koff and derives from it how many key
tiles a block / a wave streams; a one-key error there yields plausible text, and random inputs hide it (one key carries ~1/Sk of a row).
So every shape runs with three kinds of input:
  a. "random":  randn q, k, v -- the rule the existing attention tests use;
  b. "needle":  q_i a multiple of the LAST ALLOWED key of row i (its diagonal key i + koff, or the last unmasked one below it): that key
                carries >= 0.9999 of the softmax, the row must come out as that key's V row.  A kernel that drops the key (diagonal short
                by one, a tile not streamed, a wave stopping a tile early) returns something else;
  c. "forbid":  q_i a multiple of the FIRST FORBIDDEN key i + koff + 1 (on a left-padded sample: of a masked key below the diagonal): the
                reference ignores it, a kernel that leaks it returns that key's V row.
The needle keys are +-1 vectors and the multiple a power of two, so Q K^T is an exact integer in any summation order and the kernel and
the reference round the very same scores; `test_needle_inputs_expose_a_shifted_diagonal_a_dropped_tile_and_an_ignored_mask` (CPU) shows
on the reference itself that each of those errors moves every affected row outside the tolerance.

The GPU tests carry `@gpu` (= pytest.mark.gpu) one by one instead of a module-wide `pytestmark`: the two CPU checks of the inputs at the
bottom must run under `-m "not gpu"`.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close_bf16, fixture_sd, load_fixture, pkg, rel_err
from oracle import ullava_oracle as O
from test_fp16_gpu import assert_close_f16

gpu = pytest.mark.gpu
DEV = "cuda:0"
BF, FP16 = torch.bfloat16, torch.float16
DTS = [BF, FP16]
KINDS = ["random", "needle", "forbid"]
KT = 64                                  # keys per tile (csrc/attention.hip)
W_NEEDLE, W_FORBID = 0.9999, 0.99        # softmax weight of the needle key in the reference (b) / if it leaked (c)


# ---- which launch dispatch_nt (csrc/attention.hip) picks for a causal scale_mode-1 call with a V^T image ---------------------------------
def family(Sq, Sk, hd):
    nt = (Sk + KT - 1) // KT
    if Sq <= 16 and 2 <= nt <= 64:
        return "fewq_tpw1" if nt <= 16 else "fewq_tpw4"                # launch_fewq_t<.., 1> / <.., 4>
    if hd == 128:                                                      # FL_LLAMA
        return "llama_11x4w" if nt <= 11 else "llama_16x8w" if nt <= 16 else "long"
    if hd <= 64 and nt <= 5:                                           # FL_RUNTIME register kernels (no <128, 5> instantiation: hd 80)
        return "runtime_5"
    return "runtime_11" if nt <= 11 else "runtime_16" if nt <= 16 else "long"


# (B, H, Sq, Sk, hd, mask, family).  mask: None | ("right", n) | ("left", n) -- n keys of the LAST sample masked at the end / the start.
def _c(B, H, Sq, Sk, fam, hd=128, mask=None):
    return (B, H, Sq, Sk, hd, mask, fam)


GRID_128 = [
    # <= 704 keys: launch_attn<128, 11, FL_LLAMA, 4> (64-query blocks, 4 waves)
    _c(1, 2, 17, 18, "llama_11x4w"), _c(2, 4, 17, 32, "llama_11x4w"), _c(1, 3, 63, 64, "llama_11x4w"), _c(1, 2, 63, 127, "llama_11x4w"),
    _c(2, 2, 64, 65, "llama_11x4w"), _c(1, 2, 64, 128, "llama_11x4w"), _c(1, 2, 64, 129, "llama_11x4w"), _c(3, 4, 65, 128, "llama_11x4w"),
    _c(1, 2, 65, 81, "llama_11x4w"), _c(1, 2, 127, 144, "llama_11x4w"), _c(1, 2, 127, 191, "llama_11x4w"), _c(1, 2, 128, 193, "llama_11x4w"),
    _c(2, 8, 128, 192, "llama_11x4w"), _c(1, 2, 129, 192, "llama_11x4w"), _c(1, 2, 129, 629, "llama_11x4w"), _c(1, 2, 200, 700, "llama_11x4w"),
    _c(1, 2, 200, 704, "llama_11x4w"), _c(1, 2, 640, 641, "llama_11x4w"), _c(1, 2, 689, 704, "llama_11x4w"),
    # 705 .. 1024 keys: launch_attn<128, 16, FL_LLAMA> (128-query blocks, 8 waves)
    _c(1, 2, 200, 705, "llama_16x8w"), _c(1, 2, 17, 1024, "llama_16x8w"), _c(2, 8, 128, 1024, "llama_16x8w"), _c(1, 2, 129, 1023, "llama_16x8w"),
    _c(1, 3, 65, 769, "llama_16x8w"), _c(1, 2, 63, 767, "llama_16x8w"), _c(1, 2, 524, 1024, "llama_16x8w"), _c(1, 2, 689, 705, "llama_16x8w"),
    _c(1, 2, 1007, 1024, "llama_16x8w"), _c(1, 2, 961, 1024, "llama_16x8w"), _c(1, 1, 960, 1024, "llama_16x8w"),
    _c(1, 2, 127, 832, "llama_16x8w"),
    # > 1024 keys: launch_long<128, FL_RUNTIME> (two passes)
    _c(1, 2, 17, 1025, "long"), _c(1, 2, 64, 1025, "long"), _c(1, 2, 1024, 1025, "long"), _c(2, 8, 129, 1089, "long"),
    _c(1, 2, 1010, 1025, "long"), _c(1, 2, 1100, 1165, "long"), _c(1, 2, 200, 3000, "long"), _c(1, 1, 2500, 3000, "long"),
    _c(1, 2, 128, 1152, "long"),
]
GRID_SMALL_HD = [
    _c(2, 2, 70, 200, "runtime_5", hd=64), _c(1, 3, 100, 600, "runtime_11", hd=64), _c(1, 2, 70, 200, "runtime_11", hd=80),
    _c(1, 2, 40, 1100, "long", hd=80), _c(2, 4, 40, 100, "runtime_5", hd=32), _c(1, 2, 65, 900, "runtime_16", hd=32),
    _c(2, 4, 40, 100, "runtime_5", hd=16), _c(1, 8, 33, 1500, "long", hd=16),
]
_FEWQ_FAM = {1: "llama_11x4w", 2: "llama_11x4w", 63: "llama_11x4w", 64: "llama_11x4w", 65: "fewq_tpw1", 1024: "fewq_tpw1", 1025: "fewq_tpw4",
             1088: "fewq_tpw4", 1089: "fewq_tpw4", 4096: "fewq_tpw4", 4097: "long", 5000: "long"}
# Heads per few-query case: rule (a) caps a SHARE of elements, and one score whose bf16 rounding falls the other way under another fp32
# summation order (Q K^T has 128 terms) moves, for a key of large weight, every near-zero element of its row -- the ~6 % of a row's 128
# elements below 2 % of max|ref|, 8 or 9 elements.  A cap of 2e-3 admits one or two such events from 6000 / 12000 elements on, so every
# case compares B * H * Sq >= 96 rows (Sq = 1: LLaMA-7B's 32 heads at batch 4); 3072 elements would admit 6 elements, less than one event.
_FEWQ_BH = {1: (4, 32), 4: (2, 16), 16: (2, 3)}
GRID_FEWQ = [_c(_FEWQ_BH[Sq][0], _FEWQ_BH[Sq][1] + (2 if Sk == 1089 else 0), Sq, Sk, fam)
             for Sq in (1, 4, 16) for Sk, fam in _FEWQ_FAM.items() if Sk >= Sq]
_MASK_SHAPES = [(2, 4, 17, 200, 128, "llama_11x4w"), (2, 2, 65, 128, 128, "llama_11x4w"), (2, 2, 129, 705, 128, "llama_16x8w"),
                (2, 2, 200, 1100, 128, "long"), (2, 3, 4, 200, 128, "fewq_tpw1"), (2, 3, 16, 1025, 128, "fewq_tpw4"), (2, 2, 70, 200, 64, "runtime_5")]
GRID_MASKED = [_c(B, H, Sq, Sk, fam, hd=hd, mask=m) for (B, H, Sq, Sk, hd, fam) in _MASK_SHAPES
               for m in (("right", Sk // 3), ("left", 1), ("left", 63), ("left", 64), ("left", 65))]
ALL_CASES = GRID_128 + GRID_SMALL_HD + GRID_FEWQ + GRID_MASKED


def _id(case):
    B, H, Sq, Sk, hd, mask, fam = case
    return f"{fam}-b{B}h{H}-{Sq}x{Sk}-hd{hd}" + ("" if mask is None else f"-{mask[0]}{mask[1]}")


def _dtname(dt):
    return "bf16" if dt == BF else "fp16"


def outlier_cap(Sq):
    """the shares the existing tests admit: test_attention (prefill kernels) 1e-3, test_attention_decode_step_shapes (<= 16 queries) 2e-3."""
    return 2e-3 if Sq <= 16 else 1e-3


# ---- reference -------------------------------------------------------------------------------------------------------------------------
def _allowed(B, Sq, Sk, km, shift=0, drop_last_tile=False, ignore_mask=False):
    """[B, 1, Sq, Sk] bool: key j visible to query i -- j <= i + (Sk - Sq) and key_mask[b, j] != 0.  The other arguments build the WRONG
    rules the CPU check of the inputs runs: the diagonal shifted, the tile that holds a row's diagonal key not streamed, the mask ignored."""
    qi, kj = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    a = kj <= qi + (Sk - Sq) + shift
    if drop_last_tile:
        a = a & (kj // KT != (qi + (Sk - Sq)) // KT)
    a = a[None, None].expand(B, 1, Sq, Sk)
    if km is not None and not ignore_mask:
        a = a & (km[:, None, None, :] != 0)
    return a


def _attn_ref(q, k, v, scale, km, f64=False, **wrong):
    """eager attention on 16-bit tensors q [B,H,Sq,hd], k / v [B,H,Sk,hd] with the kernels' rounding points (`_attn_ref` of
    test_kernels_gpu.py / test_attention_fp16, on the element type of q): S = dt(dt(Q K^T) * scale) + additive mask, softmax in fp32 -> dt,
    P V -> dt.  f64: the same operation with every sum in double -- Q K^T exact, the softmax and P V in double, rounded to dt at the points
    that define the operation (scores twice, P once) and not at the end: what is left is the reference's own fp32 summation, the score /
    probability roundings that flip because of it, and its rounded output."""
    dt = q.dtype
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    w = (q.double() @ k.double().transpose(2, 3)).to(dt) if f64 else torch.matmul(q, k.transpose(2, 3))
    w = w * scale
    w = w + torch.where(_allowed(B, Sq, Sk, km, **wrong), torch.zeros((), dtype=dt), torch.full((), torch.finfo(dt).min, dtype=dt))
    if f64:
        return torch.matmul(F.softmax(w.double(), dim=-1).to(dt).double(), v.double())
    return torch.matmul(F.softmax(w, dim=-1, dtype=torch.float32).to(dt), v)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _key_mask(B, Sk, mask):
    if mask is None:
        return None
    km = torch.ones(B, Sk, dtype=torch.int32)
    if mask[0] == "right":
        km[-1, Sk - mask[1]:] = 0
    else:
        km[-1, :mask[1]] = 0
    return km


def _valid_rows(B, Sq, Sk, km):
    """[B, Sq] bool: queries whose own key i + koff is unmasked (the rows test_attention compares)."""
    if km is None:
        return torch.ones(B, Sq, dtype=torch.bool)
    return km[:, Sk - Sq:] != 0


def _pm1(B, H, Sk, hd, g):
    """+-1 keys, all rows of a head distinct (hd = 16: the bits of distinct 16-bit numbers)."""
    if hd == 16:
        codes = torch.stack([torch.randperm(1 << 16, generator=g)[:Sk] for _ in range(B * H)]).view(B, H, Sk, 1)
        bits = (codes >> torch.arange(16)) & 1
    else:
        bits = torch.randint(0, 2, (B, H, Sk, hd), generator=g)
    return (bits * 2 - 1).float()


def _targets(B, Sq, Sk, km, mask, kind):
    """[B, Sq] key index each row's query points at, and [B, Sq] bool: the row carries the kind's own needle (else, kind "forbid" only: no
    such key exists, the row points at its last allowed key like kind "needle")."""
    koff = Sk - Sq
    al = _allowed(B, Sq, Sk, km)[:, 0]                                                  # [B, Sq, Sk]
    last = (al * torch.arange(1, Sk + 1)).amax(-1) - 1                                  # last allowed key, -1: none
    if kind == "needle":
        return last.clamp_min(0), last >= 0
    forb = (torch.arange(Sq) + koff + 1)[None].repeat(B, 1)
    if mask is not None and mask[0] == "left":                                          # last sample: masked keys just below the boundary
        n = mask[1]
        forb[-1] = torch.minimum((n - 1 - torch.arange(Sq) % min(n, 4)).clamp_min(0), torch.arange(Sq) + koff)
    has = forb < Sk
    return torch.where(has, forb, last.clamp_min(0)), has


def make_inputs(case, dt, kind):
    """-> dict(q, k, v [B,H,S,hd] of dt, km, valid [B,Sq], tgt [B,Sq], has [B,Sq], mult)"""
    B, H, Sq, Sk, hd, mask, _ = case
    g = torch.Generator().manual_seed(1000 * Sq + Sk + hd + (0 if mask is None else 7 * mask[1] + (1 if mask[0] == "left" else 2)))
    km = _key_mask(B, Sk, mask)
    valid = _valid_rows(B, Sq, Sk, km)
    v = torch.randn(B, H, Sk, hd, generator=g).to(dt)
    if kind == "random":
        q, k = torch.randn(B, H, Sq, hd, generator=g).to(dt), torch.randn(B, H, Sk, hd, generator=g).to(dt)
        return dict(q=q, k=k, v=v, km=km, valid=valid, tgt=None, has=None, mult=None)
    k = _pm1(B, H, Sk, hd, g)
    tgt, has = _targets(B, Sq, Sk, km, mask, kind)
    qdir = k.gather(2, tgt[:, None, :, None].expand(B, H, Sq, hd))
    dots = qdir @ k.transpose(2, 3)                                                      # exact integers
    al = _allowed(B, Sq, Sk, km)
    if kind == "forbid":                                                                 # the weight the forbidden key would take if it leaked
        al = al | (F.one_hot(tgt, Sk).bool() & has[..., None])[:, None]
    rows = valid if kind == "needle" else valid & has
    scale = hd ** -0.5
    for mult in (1, 2, 4, 8, 16, 32, 64, 128):
        s = ((dots * mult).to(dt) * scale).double()
        wt = F.softmax(s.masked_fill(~al, float("-inf")), dim=-1).gather(3, tgt[:, None, :, None].expand(B, H, Sq, 1))[..., 0]
        need = W_NEEDLE if kind == "needle" else W_FORBID
        if not bool(rows.any()) or float(wt.transpose(1, 2)[rows].min()) >= need:
            break
    else:
        raise AssertionError(f"{_id(case)} {kind}: no multiple gives the needle key the weight {need}")
    assert mult * hd < 60000                                                             # Q K^T stays finite in fp16
    return dict(q=(qdir * mult).to(dt), k=k.to(dt), v=v, km=km, valid=valid, tgt=tgt, has=has, mult=mult)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def _rows(x, valid):
    """[B,H,Sq,hd] -> the compared rows [n, H, hd]"""
    return x.transpose(1, 2)[valid]


def assert_rule(got, ref, dt, vmax, cap, what):
    """rule (a): bf16 -- test_attention's; fp16 -- test_attention_fp16's."""
    if dt == BF:
        assert_close_bf16(got, ref, ulps=2.0, what=what, outlier_frac=cap, outlier_floor=vmax)
    else:
        assert_close_f16(got, ref, ulps=2.0, floor=vmax * 0.5, what=what)


def rule_figures(got, ref, dt, vmax):
    """the same rule as numbers: (share of elements beyond the tight bound, worst |d| / the bound every element must meet, per-row
    'an element of this row is beyond that bound')."""
    a, b = got.double(), ref.double()
    d = (a - b).abs()
    if dt == BF:
        tight = 2.0 * 2.0 ** -7 * torch.maximum(b.abs(), torch.full_like(b, float(b.abs().max()) * 0.02))
        loose = 2.0 * 2.0 ** -7 * torch.maximum(b.abs(), torch.full_like(b, vmax))
    else:
        tight = loose = 2.0 * 2.0 ** -10 * torch.maximum(b.abs(), torch.full_like(b, vmax * 0.5))
    return float((d > tight).double().mean()), float((d / loose).max()), (d > loose).flatten(1).any(-1)


def rule_holds(got, ref, dt, vmax, cap):
    share, worst, _ = rule_figures(got, ref, dt, vmax)
    return worst <= 1.0 and (dt != BF or share <= cap)


# ---- 1. kernel level -------------------------------------------------------------------------------------------------------------------
def _run_kernel(q, k, v, km, fused_q):
    """ops.attention the way the `decode` branch of modeling_core._llama calls it: K from a cache [B,H,smax,hd] (smax > Sk, rows >= Sk hold
    other values), V^T from transpose_v(pitch=smax), Q as rows of a fused q|k|v buffer or as a plain [B*Sq, D] tensor."""
    ops = pkg("ops")
    dt = q.dtype
    B, H, Sq, hd = q.shape
    Sk, D = k.shape[2], H * hd
    smax = ((Sk + 63) // 64) * 64 + 64
    g = torch.Generator().manual_seed(Sk)
    kc = (torch.randn(B, H, smax, hd, generator=g) * 3.0).to(dt)
    kc[:, :, :Sk] = k
    vtc = ops.transpose_v(v.transpose(1, 2).reshape(B * Sk, D).to(DEV), Sk * D, D, B, Sk, H, hd, pitch=smax)
    qrows = q.transpose(1, 2).reshape(B * Sq, D)
    if fused_q:
        buf = torch.randn(B * Sq, 3 * D, generator=g).to(dt)
        buf[:, :D] = qrows
        qd, qs = buf.to(DEV), (Sq * 3 * D, hd, 3 * D)
    else:
        qd, qs = qrows.contiguous().to(DEV), (Sq * D, hd, D)
    out = torch.full((B * Sq, D), float("nan"), device=DEV, dtype=dt)
    ops.attention(qd, kc.to(DEV), vtc, out, B, H, Sq, Sk, hd, qs, (H * smax * hd, smax * hd, hd), (Sq * D, hd, D),
                  None if km is None else km.to(DEV), causal=True, scale_mode=1, scale=hd ** -0.5)
    return out.cpu().view(B, Sq, H, hd).transpose(1, 2)


def _check_case(case, dt, kind):
    B, H, Sq, Sk, hd, mask, fam = case
    assert Sk >= Sq and family(Sq, Sk, hd) == fam, "the dispatch table this grid was laid out for has changed"
    x = make_inputs(case, dt, kind)
    q, k, v, km, valid = x["q"], x["k"], x["v"], x["km"], x["valid"]
    ref = _attn_ref(q, k, v, hd ** -0.5, km)
    got = _run_kernel(q, k, v, km, fused_q=True)
    plain = _run_kernel(q, k, v, km, fused_q=False)
    what = f"{_id(case)} {_dtname(dt)} {kind}"
    vmax, cap = float(v.float().abs().max()), outlier_cap(Sq)
    g_, r_ = _rows(got, valid), _rows(ref, valid)
    share, worst, _ = rule_figures(g_, r_, dt, vmax)
    print(f"{what}: share beyond the tight bound {share:.2e} (cap {cap:.0e}), worst |d| / bound {worst:.3f}")
    assert torch.equal(_rows(plain, valid), g_), f"{what}: Q as plain rows and Q inside the fused q|k|v buffer differ"
    assert_rule(g_, r_, dt, vmax, cap, what)
    if kind == "random":
        return
    tv = v.gather(2, x["tgt"][:, None, :, None].expand(B, H, Sq, hd))                  # the V row of each row's needle key
    if kind == "needle":
        assert_rule(g_, _rows(tv, valid), dt, vmax, cap, what + " against V[last allowed key]")
    else:
        rows = valid & x["has"]
        g2, r2, t2 = _rows(got, rows).float(), _rows(ref, rows).float(), _rows(tv, rows).float()
        d_ref, d_forb = (g2 - r2).flatten(1).norm(dim=1), (g2 - t2).flatten(1).norm(dim=1)
        assert bool((d_forb > d_ref).all()), f"{what}: {int((d_forb <= d_ref).sum())} rows are closer to the forbidden key's V row than to the reference"


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_128, ids=_id)
def test_cached_attention_hd128_grid(case, dt, kind):
    """hd 128 (FL_LLAMA): Sq around the 64- / 128-query blocks, koff from 1 to 2800, Sk at tile multiples +- 1 and at the 704 / 705 and
    1024 / 1025 switches of the dispatch table, B * H below and above the 8 XCDs."""
    _check_case(case, dt, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_SMALL_HD, ids=_id)
def test_cached_attention_small_head_dims(case, dt, kind):
    """hd 64, 80, 32, 16: a causal call there takes the FL_RUNTIME register kernels / the long kernel."""
    _check_case(case, dt, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_FEWQ, ids=_id)
def test_cached_attention_few_query_edges(case, dt, kind):
    """Sq <= 16: one tile (nt == 1: falls through to the register kernel), the few-query kernel with 1 and 4 tiles per wave (switch at
    nt == 16 / 17), more than 64 tiles (two-pass long kernel)."""
    _check_case(case, dt, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_MASKED, ids=_id)
def test_cached_attention_key_masks(case, dt, kind):
    """right padding and left padding of 1 / 63 / 64 / 65 keys on the last sample; rows of unmasked queries are compared."""
    _check_case(case, dt, kind)


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("Sk", [100, 1024, 1100, 4096])
def test_cached_attention_16_against_17_queries(Sk, dt, kind):
    """Sq = 16 takes the few-query kernel (the long kernel beyond 4096 keys), Sq = 17 at the same Sk a register / long kernel.  Under the
    causal rule a row sees the keys <= i + Sk - Sq, so the same query sees the same keys in both calls
      * as row i of the 16 and row i + 1 of the 17 at the same Sk (the 16 queries are the last 16 of the 17), and
      * as row i of both when the 17-query call has one key more (the same first 16 queries; the extra key is above their diagonals).
    Both pairs are compared with each other under the rule used against the reference (different kernels: no bit equality)."""
    B, H, hd = 2, 3, 128
    x = make_inputs(_c(B, H, 17, Sk, family(17, Sk, hd)), dt, kind)
    q, k, v = x["q"], x["k"], x["v"]
    vmax, cap = float(v.float().abs().max()), outlier_cap(16)
    assert family(16, Sk, hd) != family(17, Sk, hd)
    a17 = _run_kernel(q, k, v, None, fused_q=True)
    a16 = _run_kernel(q[:, :, 1:].contiguous(), k, v, None, fused_q=True)
    ref = _attn_ref(q, k, v, hd ** -0.5, None)
    what = f"16 vs 17 x {Sk} {_dtname(dt)} {kind}"
    assert_rule(a17, ref, dt, vmax, cap, what + ": 17 vs reference")
    assert_rule(a16, ref[:, :, 1:], dt, vmax, cap, what + ": 16 vs reference")
    assert_rule(a16, a17[:, :, 1:], dt, vmax, cap, what + ": last 16 of 17 vs 16")
    # the same first 16 queries: 16 x (Sk - 1) against 17 x Sk (for row i both diagonals sit at key i + Sk - 17)
    b16 = _run_kernel(q[:, :, :16].contiguous(), k[:, :, :Sk - 1].contiguous(), v[:, :, :Sk - 1].contiguous(), None, fused_q=False)
    assert_rule(b16, ref[:, :, :16], dt, vmax, cap, what + ": first 16 vs reference")
    assert_rule(b16, a17[:, :, :16], dt, vmax, cap, what + ": first 16 of 17 vs 16")


# ---- 2. rope_append with many new tokens -----------------------------------------------------------------------------------------------
def _vt_slot(pos):
    """V^T column of key pos: inside its 32-key block, slot 8g + 4a + r <- key 16a + 4g + r."""
    w = pos % 32
    a, g, r = w // 16, (w // 4) % 4, w % 4
    return pos - w + 8 * g + 4 * a + r


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [5, 17, 40])
def test_rope_append_many_new_tokens(S, B, hd, dt):
    """ull_rope_append_* with B * S rows (a continuation longer than 4 tokens skips the fused GEMV epilogue): the new positions cross a
    32-key permutation block and a 64-key tile.  q / k bit-equal to rope_inplace, the K rows and V^T columns copied to their places in a
    cache built on the CPU, everything else in the caches untouched -- torch.equal on the whole buffers."""
    ops, M_ = pkg("ops"), pkg("modeling_core")
    H = 4
    D = H * hd
    inv = (1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))).to(DEV)
    for past in (0, 27, 31, 60, 63, 100):
        smax = ((past + S + 63) // 64) * 64 + 64
        g = torch.Generator().manual_seed(S * 1000 + past + hd)
        qkv = torch.randn(B * S, 3 * D, generator=g).to(dt)
        pos = (torch.arange(S)[None] + past + 5 * torch.arange(B)[:, None]).reshape(-1)        # (RoPE positions need not be the cache slots)
        a = qkv.to(DEV)
        ops.rope_inplace(a, 3 * D, pos.to(DEV), inv, B * S, 2 * H, hd)
        a = a.cpu()
        want_k = torch.full((B, H, smax, hd), 7.0, dtype=dt)
        want_vt = torch.full((B, H, hd, smax), 7.0, dtype=dt)
        ar = a.view(B, S, 3, H, hd)
        for t in range(S):
            assert _vt_slot(past + t) == M_.KVCache.vt_slot(past + t)
            want_k[:, :, past + t] = ar[:, t, 1]
            want_vt[:, :, :, _vt_slot(past + t)] = ar[:, t, 2]
        b = qkv.to(DEV)
        kc = torch.full((B, H, smax, hd), 7.0, device=DEV, dtype=dt)
        vtc = torch.full((B, H, hd, smax), 7.0, device=DEV, dtype=dt)
        ops.rope_append(b, 3 * D, pos.to(DEV), inv, B, S, H, hd, kc, vtc, smax, past)
        b = b.cpu()
        assert torch.equal(b[:, :D], a[:, :D]), f"past {past}: rotated q"            # (the rotated k goes to the cache only)
        assert torch.equal(b[:, 2 * D:], qkv[:, 2 * D:]), f"past {past}: v rows must stay"
        assert torch.equal(kc.cpu(), want_k), f"past {past}: K cache"
        assert torch.equal(vtc.cpu(), want_vt), f"past {past}: V^T cache"


# ---- 3. model level: a continuation equals the one-shot prefill ------------------------------------------------------------------------
_MM = dict(IMG_START=90, IMG_END=91, IMG_PATCH=92, VID_START=93, VID_END=94, VID_PATCH=95)
_HD128 = dict(hidden_size=256, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=100, rms_norm_eps=1e-6,
              rope_theta=10000.0, vision_hidden_layer=-2, projector_type="mlp", mm_token_ids=_MM,
              vision_config=dict(hidden_size=32, num_hidden_layers=3, num_attention_heads=2, intermediate_size=64, image_size=28, patch_size=14,
                                 num_channels=3, layer_norm_eps=1e-5))
_MODELS = {}


def _model(which, dt):
    """("tiny": the g1_core_tiny fixture model, head_dim 16 | "hd128": a seeded 2-layer config with head_dim 128) in dt -> (model, sd, cfg dict)"""
    if (which, dt) in _MODELS:
        return _MODELS[(which, dt)]
    C, M, W = pkg("configuration"), pkg("modeling_core"), pkg("weights")
    if which == "tiny":
        fx = load_fixture("g1_core_tiny_bf16.pt")
        cd = dict(fx["cfg"])
    else:
        cd = dict(_HD128)
    cfg = C.UllavaCoreConfig(**cd, projector_from_scratch=False)
    model = M.UllavaCoreForCausalLM(cfg, device=DEV, dtype=dt)
    if which == "tiny":
        sd = fixture_sd(fx, dt)
    else:
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        sd = {k: v.to(dt) for k, v in W.seeded_state_dict(shapes, 4242, torch.float32).items()}
    model.load_state_dict(sd, strict=True)
    _MODELS[(which, dt)] = (model, sd, cd)
    return _MODELS[(which, dt)]


def _text(B, L, left_pad, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 90, (B, L), generator=g)                    # text ids: below the multimodal ids 90 .. 95
    mask = torch.ones(B, L, dtype=torch.long)
    if left_pad:
        mask[-1, :left_pad] = 0
    pos = (mask.cumsum(-1) - 1).clamp_min(0)
    return ids, mask, pos


# (B, P, chunk, left padding of the last sample): past + chunk crosses 64 in every case
_CONT = [(1, 60, 5, 0), (1, 50, 17, 0), (1, 30, 70, 0), (1, 64, 17, 0), (2, 61, 17, 9), (2, 40, 70, 33), (2, 62, 5, 63)]


@gpu
@pytest.mark.parametrize("per_op", [False, True], ids=["coarse", "per_op"])
@pytest.mark.parametrize("B,P,chunk,left_pad", _CONT)
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("which", ["tiny", "hd128"])
def test_continuation_equals_one_shot_prefill(which, dt, B, P, chunk, left_pad, per_op):
    """prefill P tokens into a KVCache, then forward() the next `chunk` tokens on it (rope_append with B * chunk rows, attention with
    Sq = chunk, Sk = P + chunk at cache strides) -- against a no-cache forward over the whole sequence and a one-shot cached prefill.
    Different kernels on the two sides, so the rule of test_c1_kv_cached_generate_returns_the_no_cache_last_step_states_full_depth: the
    error against the oracle's fp32 forward with the same weights is at most 1.5 x the other HIP run's (floor 2^-7), for the chunk's
    logits and for every layer's cached K / V.  The cached K rows / V^T columns of the positions < P are bit-identical before and after."""
    ops, MC = pkg("ops"), pkg("modeling_core")
    model, sd, cd = _model(which, dt)
    L = P + chunk
    H, hd, nl = cd["num_attention_heads"], cd["hidden_size"] // cd["num_attention_heads"], cd["num_hidden_layers"]
    ids, mask, pos = _text(B, L, left_pad, 31 * P + chunk)
    idg, mg, pg = ids.to(DEV), mask.to(DEV), pos.to(DEV)
    new = lambda: MC.KVCache(nl, B, H, hd, L + 30, DEV, dtype=dt)
    with torch.no_grad(), ops.per_op_layers(per_op):
        nocache = model(input_ids=idg, attention_mask=mg, position_ids=pg).logits
        c1 = new()
        oneshot = model(input_ids=idg, attention_mask=mg, position_ids=pg, past_key_values=c1, use_cache=True).logits
        c2 = new()
        model(input_ids=idg[:, :P], attention_mask=mg[:, :P], position_ids=pg[:, :P], past_key_values=c2, use_cache=True)
        assert c2.length == P
        k_before, vt_before = [t.clone() for t in c2.k], [t.clone() for t in c2.vt]
        cont = model(input_ids=idg[:, P:], attention_mask=mg, position_ids=pg[:, P:], past_key_values=c2, use_cache=True).logits
    assert c1.length == c2.length == L and tuple(cont.shape) == (B, chunk, cd["vocab_size"])
    old = torch.tensor([_vt_slot(p) for p in range(P)], device=DEV)
    for li in range(nl):
        assert torch.equal(c2.k[li][:, :, :P], k_before[li][:, :, :P]), f"layer {li}: K rows of the prefill changed"
        assert torch.equal(c2.vt[li][..., old], vt_before[li][..., old]), f"layer {li}: V^T columns of the prefill changed"
        tail = torch.tensor(sorted(set(range(c2.smax)) - {_vt_slot(p) for p in range(L)}), device=DEV)
        assert not bool(c2.vt[li][..., tail].any()), f"layer {li}: V^T columns beyond the sequence must stay zero"
    sd32 = {k: v.float() for k, v in sd.items()}                   # the oracle's LLaMA stack in fp32 on the same weights (text-only ids)
    hs, past32 = O.llama_model(sd32, cd, F.embedding(ids, sd32["model.embed_tokens.weight"]), mask, pos)
    truth = dict(logits=F.linear(hs[-1], sd32["lm_head.weight"]), past=past32)
    valid = mask.bool()
    vc = valid[:, P:]
    t_chunk = truth["logits"][:, P:][vc]
    e_cont, e_nc, e_os = (rel_err(x.cpu()[vc], t_chunk) for x in (cont, nocache[:, P:], oneshot[:, P:]))
    print(f"continuation {which} {_dtname(dt)} B={B} P={P} chunk={chunk} pad={left_pad}: logits err vs fp32 -- continuation {e_cont:.5f}, "
          f"no-cache {e_nc:.5f}, one-shot prefill {e_os:.5f}")
    assert e_cont <= max(1.5 * e_nc, 2.0 ** -7) and e_cont <= max(1.5 * e_os, 2.0 ** -7)
    kv1, kv2 = c1.to_legacy_cache(), c2.to_legacy_cache()
    for li in range(nl):
        for j, name in ((0, "K"), (1, "V")):
            t = truth["past"][li][j].transpose(1, 2)[valid]                              # [B,H,L,hd] -> the valid positions [n, H, hd]
            e2, e1 = rel_err(kv2[li][j].cpu().transpose(1, 2)[valid], t), rel_err(kv1[li][j].cpu().transpose(1, 2)[valid], t)
            assert e2 <= max(1.5 * e1, 2.0 ** -7), f"layer {li} cached {name}: continuation {e2:.5f} vs one-shot prefill {e1:.5f}"


@gpu
@pytest.mark.parametrize("B,P,chunk,left_pad", [(1, 70, 17, 0), (2, 61, 20, 9), (1, 30, 40, 0)])
@pytest.mark.parametrize("which", ["tiny", "hd128"])
def test_continuation_on_fp8_cache_equals_twin(which, B, P, chunk, left_pad):
    """more than 16 new tokens on an fp8 KV cache: the fp8 decode attention declines, every layer is dequantized into the bf16 scratch,
    runs the bf16 path and quantizes its new positions back (_kv8_decode_buffers).  The rule of test_kv8_cache_gpu.py: bit-identical to the
    same call on the bf16 twin `cache.dequantized()`."""
    MC = pkg("modeling_core")
    model, sd, cd = _model(which, BF)
    L = P + chunk
    H, hd, nl = cd["num_attention_heads"], cd["hidden_size"] // cd["num_attention_heads"], cd["num_hidden_layers"]
    ids, mask, pos = (t.to(DEV) for t in _text(B, L, left_pad, 77 * P + chunk))
    with torch.no_grad():
        c8 = MC.KVCache(nl, B, H, hd, L + 30, DEV, kv_dtype="fp8_e4m3")
        model(input_ids=ids[:, :P], attention_mask=mask[:, :P], position_ids=pos[:, :P], past_key_values=c8, use_cache=True)
        tw = c8.dequantized()
        a = model(input_ids=ids[:, P:], attention_mask=mask, position_ids=pos[:, P:], past_key_values=tw, use_cache=True, output_hidden_states=True)
        b = model(input_ids=ids[:, P:], attention_mask=mask, position_ids=pos[:, P:], past_key_values=c8, use_cache=True, output_hidden_states=True)
        assert c8.length == tw.length == L
        assert torch.equal(a.logits, b.logits), "logits"
        assert all(torch.equal(x, y) for x, y in zip(a.hidden_states, b.hidden_states)), "hidden states"
        tw2 = c8.dequantized()
        for li in range(nl):                     # the old positions keep their codes
            assert torch.equal(tw2.k[li][:, :, :P], tw.k[li][:, :, :P]), f"layer {li}: dequantized K of the prefill changed"


# ---- CPU: the inputs themselves ---------------------------------------------------------------------------------------------------------
def _cpu_cases():
    return ALL_CASES


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_needle_inputs_expose_a_shifted_diagonal_a_dropped_tile_and_an_ignored_mask(dt):
    """Guards the design of inputs (b) and (c), not the kernels: the reference run with a deliberately wrong rule must leave rule (a) in
    EVERY row the error touches --
      * diagonal short by one key (j <= i + koff - 1)            on "needle": every row whose last allowed key is its diagonal key;
      * the tile holding the row's diagonal key not streamed     on "needle": every row (that still sees a key);
      * diagonal long by one key (j <= i + koff + 1)             on "forbid": every row that has an unmasked key i + koff + 1;
      * the key mask ignored                                     on "forbid": every row of a left-padded sample;
    and the right rule gives, on "needle", the V row of the needle key itself."""
    for case in _cpu_cases():
        B, H, Sq, Sk, hd, mask, fam = case
        assert family(Sq, Sk, hd) == fam
        koff, scale, cap = Sk - Sq, hd ** -0.5, outlier_cap(Sq)
        x = make_inputs(case, dt, "needle")
        q, k, v, km, valid, tgt = x["q"], x["k"], x["v"], x["km"], x["valid"], x["tgt"]
        vmax = float(v.float().abs().max())
        ref = _attn_ref(q, k, v, scale, km)
        tv = v.gather(2, tgt[:, None, :, None].expand(B, H, Sq, hd))
        assert rule_holds(_rows(ref, valid), _rows(tv, valid), dt, vmax, cap), _id(case)
        diag = torch.arange(Sq)[None] + koff
        n_allowed = _allowed(B, Sq, Sk, km)[:, 0].sum(-1)
        for wrong, rows in ((dict(shift=-1), valid & (tgt == diag) & (n_allowed > 1)),
                            (dict(drop_last_tile=True), valid & (tgt // KT == diag // KT) & (_allowed(B, Sq, Sk, km, drop_last_tile=True)[:, 0].any(-1)))):
            if not bool(rows.any()):
                assert Sk <= KT or Sk == 1, (_id(case), wrong)
                continue
            bad = rule_figures(_rows(_attn_ref(q, k, v, scale, km, **wrong), rows), _rows(ref, rows), dt, vmax)[2]
            assert bool(bad.all()), (_id(case), wrong, int((~bad).sum()))
        x = make_inputs(case, dt, "forbid")
        q, k, v, km, tgt, has = x["q"], x["k"], x["v"], x["km"], x["tgt"], x["has"]
        ref = _attn_ref(q, k, v, scale, km)
        unmasked = torch.ones_like(has) if km is None else km.gather(1, tgt) != 0
        left = mask is not None and mask[0] == "left"
        sample_last = torch.zeros_like(has)
        sample_last[-1] = left
        for wrong, rows in ((dict(shift=1), valid & has & (tgt == diag + 1) & unmasked), (dict(ignore_mask=True), valid & has & sample_last)):
            if not bool(rows.any()):
                assert Sq == 1 or "ignore_mask" in wrong, (_id(case), wrong)
                continue
            leak = _attn_ref(q, k, v, scale, km, **wrong)
            bad = rule_figures(_rows(leak, rows), _rows(ref, rows), dt, vmax)[2]
            assert bool(bad.all()), (_id(case), wrong, int((~bad).sum()))
            tv = _rows(v.gather(2, tgt[:, None, :, None].expand(B, H, Sq, hd)), rows).float()
            lk, rf = _rows(leak, rows).float(), _rows(ref, rows).float()
            assert bool(((lk - tv).flatten(1).norm(dim=1) < (lk - rf).flatten(1).norm(dim=1)).all()), (_id(case), wrong)
        if left:
            assert bool((valid & has & sample_last).any()), _id(case)


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_the_16_bit_reference_stays_inside_the_caps_against_fp64(dt):
    """The outlier share of rule (a) is a cap, not a measurement: for the seeds and shapes of this module the 16-bit reference itself, held
    against the same operation evaluated in double, stays inside it (all three kinds of input)."""
    worst_share, worst = 0.0, 0.0
    for case in _cpu_cases():
        B, H, Sq, Sk, hd, mask, fam = case
        for kind in KINDS:
            x = make_inputs(case, dt, kind)
            ref = _rows(_attn_ref(x["q"], x["k"], x["v"], hd ** -0.5, x["km"]), x["valid"])
            f64 = _rows(_attn_ref(x["q"], x["k"], x["v"], hd ** -0.5, x["km"], f64=True), x["valid"])
            vmax = float(x["v"].float().abs().max())
            share, w, _ = rule_figures(ref, f64, dt, vmax)
            worst_share, worst = max(worst_share, share / outlier_cap(Sq)), max(worst, w)
            assert rule_holds(ref, f64, dt, vmax, outlier_cap(Sq)), (_id(case), kind, share, w)
    print(f"{_dtname(dt)} reference against fp64: worst share / cap {worst_share:.3f}, worst |d| / bound {worst:.3f}")
