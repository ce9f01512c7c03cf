"""The attention backward (`ops.attention_bwd`: six kernels of csrc/backward.hip in three families) key by key: dQ, dK and dV each held
element by element against an fp64 reference, in bf16 and fp16, at the tile / wave / 32-block / diagonal edges of every family.

Families (asserted per call on the C-ABI entry point the call really makes, like test_linear_backward_gpu.py observes its routes):
  scalar    ull_attention_bwd_*        any head dim <= 128, any strides: 8 query rows / 8 keys per block, whole score rows in the LDS,
                                       P and dS stay fp32;
  mfma64    ull_attention_bwd_mfma_*   hd 64, head stride == hd: 64-row blocks, fragments from global memory, transposed operands as
                                       transpose_v images; P and dS rounded to the element type before the second product;
  tiles128  ull_attention_bwd_mfma_*   hd 128, same conditions: 64-row tiles by LDS-DMA, double-buffered; same rounding points.

The kernels are called directly with O as an INPUT (the fp64 forward rounded to the element type: a forward-kernel deviation must not
leak into delta = rowsum(dO * O)), dq / dk / dv pre-filled with NaN and with slack behind / beside them that must stay NaN.  Layouts:
  (a) fused [B*S, 3D (+ 8 unused columns)] q|k|v rows with the strides of autograd_ops._SelfAttention.backward (Sq == Sk only);
  (b) separate [n*S (+ a guard row), H*hd] tensors with the strides of autograd_ops._Attention.backward;
  (c) contiguous [B, H, S, hd]: head stride S * hd != hd, which routes hd 64 / 128 to the scalar kernels -- the scalar and the matrix
      kernels then run on identical data, and the scalar dK/dV kernel reaches its limit of four outputs per thread (8 * 128 = 1024).

Kinds of input (random cannot see one key: a boundary key carries ~1/S of a row):
  random   Gaussian q, k, v, dO;
  needle   the forward grid's: +-1 keys, q_i a power-of-two multiple of the row's LAST ALLOWED key (weight >= 0.9999), dO small integers:
           dV routes dO rows one to one, dS ~ 0;
  forbid   the forward grid's: q_i a multiple of the FIRST FORBIDDEN key (one past the diagonal / a masked key; weight >= 0.99 had it
           leaked);
  pair     hd >= 64: q_i a multiple of (last allowed key + first allowed key).  The two tie exactly, P = (1/2, 1/2), and with +-1 value
           rows and dO_i = c_i (v_a - v_b) + {-1, 0, 1}, c_i = +-1, dS = +-(dP_a - dP_b) mult / 4 is large in every row: dQ = dS_a (k_a - k_b)
           and dK of the two keys carry it, so one key dropped from / added to the dS products changes the row grossly;
  pairf    hd >= 64: the same with (last allowed key + first forbidden key): the reference gives the allowed key everything (dS ~ 0, dK of
           the forbidden key unchanged), a leak gives the tie -- the only kind that shows a leaked key in dK.
Below hd 64 random +-1 keys tie with third keys, so pair / pairf are built from hd 64 on; the scalar kernels take hd as a runtime
parameter and get both kinds through layout (c).  The builder asserts every weight; no row is dropped.

Rule: the suite's elementwise 2-ulp rule, no new tolerance: |d| <= 2 * 2^-7 (bf16) / 2 * 2^-10 (fp16) * max(|ref|, 2 % of max|ref| of
the tensor).  scalar: every element.  mfma64 / tiles128: a share of at most `outlier_cap` (test_attention_cached_gpu: 1e-3, 2e-3 at <= 16
rows) may miss it, every element meets the same bound with the floor raised to max|ref| (P and dS are rounded to 16 bits: a score whose
rounding falls the other way moves one term by an ulp, which a near-zero output feels).  The reference rounds P and dS for the matrix
families and not for scalar.  `test_the_backward_reference_stays_inside_the_caps_against_fp64` (CPU) holds the same recipe in fp32
against fp64 to a third of every cap on every case.  One addition, for dQ and dK of the kinds whose dS is ~ 0 by construction (needle,
forbid, pairf) and nowhere else: the worst-case fp32 dot-product bound is taken off |d| first -- see `allowances` for why the rule
alone cannot hold a tensor that is the residue of a cancellation.

FULLY MASKED query rows (left padding under `causal`): this file pins the KERNELS' rule, which is not the reference project's.  All six
kernels give such a row P = 0 (lse = INFINITY, or l == 0), so its dQ is exactly zero and dK / dV do not depend on its dO; the reference
project's additive finfo.min mask gives a uniform row there instead, whose dO is zero in any real loss.  dO and O of these rows hold
ordinary random values here; every output must be finite, dQ of the row exactly zero, dK / dV equal to the reference with P = 0 there.

The GPU tests carry `@gpu` one by one: the two CPU checks at the bottom run under `-m "not gpu"`.
"""
import functools

import pytest
import torch

from helpers import assert_close_bf16, pkg
from test_attention_cached_gpu import BF, DTS, FP16, KT, W_FORBID, W_NEEDLE, _allowed, _dtname, _key_mask, _pm1, _targets, outlier_cap, rule_figures
from test_fp16_gpu import assert_close_f16
from test_linear_backward_gpu import _spy

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("dQ", "dK", "dV")
AB_R, AB_LDS_MAX = 8, 160 * 1024 - 256            # csrc/backward.hip: rows per block of the scalar kernels, their dynamic LDS limit


# ---- the grid: (B, H, Sq, Sk, hd, causal, mask).  mask: None | ("right", n) | ("left", n) on the LAST sample -------------------------------
def _c(B, H, Sq, Sk, hd, causal=True, mask=None):
    return (B, H, Sq, Sk, hd, causal, mask)


def _bh(rows):
    """B, H by the smaller row count: few rows get more heads, so that one rounding event stays a small share (cap check below).  One
    row: 4 x 32 like the forward grid's single-query cases -- a dS that rounds the other way moves the near-zero elements of its row (~6 %
    of hd), and a cap of 2e-3 admits that only from ~4000 elements on."""
    return (4, 32) if rows == 1 else (2, 4) if rows <= 33 else (2, 2) if rows <= 129 else (1, 2)


_SELF = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 643]
_KOFF, _OFF_SQ = [1, 15, 16, 17, 63, 64, 65, 100, 192], [1, 17, 64, 65, 129]
_NONCAUSAL = [(7, 300), (300, 7), (65, 129), (129, 65), (64, 64), (1, 65)]
_SCALAR_S, _SCALAR_KOFF = [1, 7, 8, 9, 31, 32, 33, 255, 256, 257], [0, 1, 9, 33]
_MASKS = lambda Sk: [("right", Sk // 3), ("left", 1), ("left", 63), ("left", 64), ("left", 65)]

# (Sq, Sk, hd) whose fp16 random case at the heads of _bh left the fp32 recipe above a third of a cap against fp64 (the CPU check at the
# bottom; shares of 3.4e-4 .. 1.1e-3 on 4000 .. 30000 elements, one worst |d| of 0.45): more heads, same shape, same caps
_MORE_HEADS = {(64, 64, 64): 4, (193, 193, 128): 4, (17, 18, 64): 3, (64, 81, 64): 4, (17, 81, 64): 4, (17, 82, 64): 4, (17, 117, 64): 4, (64, 80, 64): 4,
               (65, 129, 64): 4, (64, 127, 128): 4, (65, 257, 128): 4, (7, 300, 64): 4, (300, 7, 64): 4, (129, 65, 128): 4}


def _m(Sq, Sk, hd, causal=True):
    B, H = _bh(min(Sq, Sk))
    return _c(B, H * _MORE_HEADS.get((Sq, Sk, hd), 1), Sq, Sk, hd, causal)


GRID_MATRIX_SELF = [_m(S, S, hd) for hd in (64, 128) for S in _SELF]
GRID_MATRIX_OFFSET = [_m(Sq, Sq + koff, hd) for hd in (64, 128) for Sq in _OFF_SQ for koff in _KOFF]
GRID_MATRIX_NONCAUSAL = [_m(Sq, Sk, hd, causal=False) for hd in (64, 128) for Sq, Sk in _NONCAUSAL]
GRID_SCALAR = [_c(*_bh(Sq), Sq, Sq + koff, hd) for hd in (16, 32, 80, 64, 128) for Sq in _SCALAR_S for koff in _SCALAR_KOFF]
GRID_SCALAR_NONCAUSAL = [_c(2, 4, 7, 4096, 16, causal=False), _c(2, 4, 4096, 7, 16, causal=False), _c(2, 4, 7, 7, 16, causal=False),
                         _c(2, 4, 7, 7, 80, causal=False)]
# masks on every family: a causal self shape, a causal offset shape (qbeg == 0 for the first key blocks) and a non-causal one
_MASK_SHAPES = [(129, 129, hd, True) for hd in (64, 128)] + [(65, 165, hd, True) for hd in (64, 128)] + [(65, 129, hd, False) for hd in (64, 128)] + \
               [(70, 100, 16, True), (100, 100, 32, True), (9, 74, 80, True), (70, 100, 16, False)]
# 65 x 165 at hd 128: 2 x 8 heads.  In `pair` a dS that rounds the other way moves the hd / 2 elements of its dQ row where k_a == k_b (zero
# in the reference) by an ulp of dS; one such event is 1 / (2 B H Sq) of dQ, 1.9e-3 at 2 x 2 x 65 rows and 4.8e-4 at 2 x 8 x 65 (cap 1e-3).
# The MI355X run met one at 2 x 2 (left padding 64, fp16: 53 elements, 1.6e-3); same shape, same cap, more heads.
GRID_MASKED = [_c(2, 8 if (Sq, Sk, hd) == (65, 165, 128) else 2, Sq, Sk, hd, causal, m) for Sq, Sk, hd, causal in _MASK_SHAPES for m in _MASKS(Sk)]
# scalar against matrix on the same values (layouts (b) and (c)): two shapes per head dim
GRID_TWINS = [_c(2, 2, 129, 129, hd) for hd in (64, 128)] + [_c(2, 2, 65, 165, hd) for hd in (64, 128)]
ALL_CASES = GRID_MATRIX_SELF + GRID_MATRIX_OFFSET + GRID_MATRIX_NONCAUSAL + GRID_SCALAR + GRID_SCALAR_NONCAUSAL + GRID_MASKED


def _id(case):
    B, H, Sq, Sk, hd, causal, mask = case
    return f"b{B}h{H}-{Sq}x{Sk}-hd{hd}-{'causal' if causal else 'full'}" + ("" if mask is None else f"-{mask[0]}{mask[1]}")


def kinds_of(case):
    """pair / pairf from hd 64 on (module docstring); pairf where a forbidden key can exist: under a diagonal or a mask."""
    B, H, Sq, Sk, hd, causal, mask = case
    return ["random", "needle", "forbid"] + (["pair"] if hd >= 64 else []) + (["pairf"] if hd >= 64 and (causal or mask is not None) else [])


def layouts_of(case, scalar_only=False):
    """the scalar grid's hd 64 / 128 cases are there for layout (c) alone (their other layouts belong to the matrix grids)."""
    B, H, Sq, Sk, hd, causal, mask = case
    if scalar_only and hd >= 64:
        return ["c"]
    return (["a"] if Sq == Sk else []) + ["b", "c"]


def family_of(case, layout):
    """the family the case was laid out for in that layout."""
    B, H, Sq, Sk, hd, causal, mask = case
    if hd not in (64, 128) or (layout == "c" and not Sq == Sk == 1):       # (c): head stride S * hd; one row makes it hd again
        return "scalar"
    return "tiles128" if hd == 128 else "mfma64"


def assert_scalar_fits(case):
    B, H, Sq, Sk, hd, causal, mask = case
    assert (AB_R * Sk + 2 * AB_R * hd + 4 * AB_R) * 4 <= AB_LDS_MAX, _id(case)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def allowed(case, km, shift=0, drop_last_tile=False, ignore_mask=False):
    """[B, 1, Sq, Sk] bool.  causal: test_attention_cached_gpu._allowed, with its wrong rules.  Not causal: every unmasked key; the wrong
    rules there are `shift` < 0: the last -shift keys not seen, `drop_last_tile`: the last key tile not streamed."""
    B, H, Sq, Sk, hd, causal, mask = case
    if causal:
        return _allowed(B, Sq, Sk, km, shift=shift, drop_last_tile=drop_last_tile, ignore_mask=ignore_mask)
    a = _allowed(B, Sq, Sk, km, shift=Sq + Sk, ignore_mask=ignore_mask)
    kj = torch.arange(Sk)
    if shift < 0:
        a = a & (kj < Sk + shift)
    if drop_last_tile:
        a = a & (kj // KT != (Sk - 1) // KT)
    return a


def tile_kept(case):
    """[Sq, Sk] bool: False on the key tile the wrong rule 'a tile dropped from the dS products' leaves out for that row."""
    B, H, Sq, Sk, hd, causal, mask = case
    qi, kj = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    return kj // KT != ((qi + (Sk - Sq)) // KT if causal else torch.full_like(qi, (Sk - 1) // KT))


def _nth(flags, n):
    """flags [B, Sq, Sk] bool, n [B, Sq]: index of the n-th True of each row (ascending)."""
    order = torch.argsort(flags.int(), dim=-1, descending=True, stable=True)
    return order.gather(-1, n[..., None])[..., 0]


def targets(case, km, kind):
    """-> (tgt [B, Sq], has [B, Sq]) like test_attention_cached_gpu._targets.  Not causal: "needle" walks down from the last allowed key
    (row i points at the (i mod n)-th allowed key from the end: every key, the last tile's edge included, is some row's needle as far as
    the rows reach), "forbid" walks over the masked keys (no mask: no forbidden key exists, has = False)."""
    B, H, Sq, Sk, hd, causal, mask = case
    if causal:
        return _targets(B, Sq, Sk, km, mask, kind)
    al = allowed(case, km)[:, 0]
    n = al.sum(-1)
    need = _nth(al, (n - 1 - torch.arange(Sq)[None] % n.clamp_min(1)).clamp_min(0))
    if kind == "needle":
        return need, n > 0
    masked = ~al
    nm = masked.sum(-1)
    return torch.where(nm > 0, _nth(masked, torch.arange(Sq)[None] % nm.clamp_min(1)), need), nm > 0


def _gather(x, idx):
    """x [B, H, Sk, hd], idx [B, Sq] -> [B, H, Sq, hd]"""
    B, H, _, hd = x.shape
    return x.gather(2, idx[:, None, :, None].expand(B, H, idx.shape[1], hd))


@functools.lru_cache(maxsize=8)
def make_inputs(case, dt, kind):
    """-> dict(q, do, o [B,H,Sq,hd], k, v [B,H,Sk,hd] of dt; km; live [B,Sq]: the row sees a key; mult).  Shared, never modified."""
    B, H, Sq, Sk, hd, causal, mask = case
    g = torch.Generator().manual_seed(1000 * Sq + Sk + hd + (0 if mask is None else 7 * mask[1] + (1 if mask[0] == "left" else 2)) + 3 * causal)
    km = _key_mask(B, Sk, mask)
    al = allowed(case, km)
    live = al[:, 0].any(-1)
    scale = hd ** -0.5
    v = torch.randn(B, H, Sk, hd, generator=g)
    if kind == "random":
        q, k, do = torch.randn(B, H, Sq, hd, generator=g), torch.randn(B, H, Sk, hd, generator=g), torch.randn(B, H, Sq, hd, generator=g)
    else:
        k = _pm1(B, H, Sk, hd, g)
        do = torch.randint(-3, 4, (B, H, Sq, hd), generator=g).float()
        if kind in ("needle", "forbid"):
            tgt, has = targets(case, km, kind)
            qdir = _gather(k, tgt)
            rows, need = (live, W_NEEDLE) if kind == "needle" else (has, W_FORBID)
            if kind == "forbid":                                       # the weight the forbidden key would take if it leaked
                al = al | (torch.nn.functional.one_hot(tgt, Sk).bool() & has[..., None])[:, None]
        else:
            a, _ = targets(case, km, "needle")
            if kind == "pair":
                b = al[:, 0].int().argmax(-1)                          # first allowed key
                rows = live & (a != b)                                 # (a row with a single allowed key has no pair)
            else:
                b, has = targets(case, km, "forbid")
                rows = live & has & (a != b)
                al_leak = al | (torch.nn.functional.one_hot(b, Sk).bool() & rows[..., None])[:, None]
            b = torch.where(rows, b, a)
            qdir = _gather(k, a) + _gather(k, b)
            v = _pm1(B, H, Sk, hd, g)
            va, vb, ka, kb = _gather(v, a), _gather(v, b), _gather(k, a), _gather(k, b)
            # the sign c_i of each row: dK of a key that many rows pair with (the first allowed one) is the sum of -c_i n_i (k_a + k_b) / 2
            # over those rows, a random walk under random signs that would set max|dK| and with it the floor of every other key row;
            # taking each sign against the running sum keeps that key's row the size of the others
            walk = (0.5 * (va - vb).abs().sum(-1, keepdim=True) * (ka + kb)).transpose(0, 2)          # [Sq, H, B, hd]
            c, run = torch.ones(Sq, H, B, 1), torch.zeros(H, B, hd)
            for i in range(Sq):
                c[i] = torch.where((run * walk[i]).sum(-1, keepdim=True) > 0, -1.0, 1.0)
                run = run + c[i] * walk[i]
            do = c.transpose(0, 2) * (va - vb) + torch.randint(-1, 2, (B, H, Sq, hd), generator=g).float()
            tgt, need = a, W_NEEDLE
        dots = qdir @ k.transpose(2, 3)                                # exact integers
        pick = lambda w, idx: w.gather(3, idx[:, None, :, None].expand(B, H, Sq, 1))[..., 0].transpose(1, 2)
        for mult in (1, 2, 4, 8, 16, 32, 64, 128):
            s = (dots * mult).double() * scale
            w = torch.softmax(s.masked_fill(~al, float("-inf")), dim=-1)
            wt = pick(w, tgt) + (pick(w, b) * (a != b)[..., None] if kind == "pair" else 0.0)
            if not bool(rows.any()) or float(wt[rows].min()) >= need:
                break
        else:
            raise AssertionError(f"{_id(case)} {kind}: no multiple gives the {kind} key(s) the weight {need}")
        if kind == "pair" and bool(rows.any()):
            assert torch.equal(pick(w, a)[rows], pick(w, b)[rows]), f"{_id(case)}: the pair does not tie exactly"
        if kind == "pairf" and bool(rows.any()):                       # had the forbidden key leaked: an exact tie that takes >= 0.99 together
            w = torch.softmax(s.masked_fill(~al_leak, float("-inf")), dim=-1)
            assert torch.equal(pick(w, a)[rows], pick(w, b)[rows]) and float((pick(w, a) + pick(w, b))[rows].min()) >= W_FORBID, _id(case)
        assert 2 * mult * hd < 60000
        q = qdir * mult
    q, k, v, do = q.to(dt), k.to(dt), v.to(dt), do.to(dt)
    p = _softmax(q.double() @ k.double().transpose(2, 3) * scale, allowed(case, km))
    o = (p @ v.double()).to(dt)
    dead = ~live[:, None, :, None].expand(B, H, Sq, hd)
    o = torch.where(dead, torch.randn(B, H, Sq, hd, generator=g).to(dt), o)          # ordinary values where no key is seen
    return dict(q=q, k=k, v=v, do=do, o=o, km=km, live=live, mult=scale)


# ---- reference --------------------------------------------------------------------------------------------------------------------------
def _softmax(s, al):
    """softmax over the allowed keys; a row without one gets P = 0 (the kernels' rule, module docstring)."""
    s = s.masked_fill(~al, float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    return e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)


def bwd_ref(case, x, dt, rounded, ft=torch.float64, drop_ds_tile=False, round_out=True, **wrong):
    """the operation the kernels define, every sum in `ft`: S = mult Q K^T over the allowed keys, P = softmax, delta = rowsum(dO * O) with
    the given 16-bit O, dS = P (dO V^T - delta) mult, dQ = dS K, dK = dS^T Q, dV = P^T dO; `rounded` (matrix families): P and dS rounded
    to the element type before the three output products.  Outputs rounded to the element type.  wrong / drop_ds_tile: the deliberately
    wrong rules of the CPU check of the inputs (drop_ds_tile: a key tile left out of dS K and dS^T Q only, the statistics correct)."""
    q, k, v, do, o = (x[n].to(ft) for n in ("q", "k", "v", "do", "o"))
    p = _softmax(q @ k.transpose(2, 3) * x["mult"], allowed(case, x["km"], **wrong))
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(2, 3) - delta) * x["mult"]
    if rounded:
        p, ds = p.to(dt).to(ft), ds.to(dt).to(ft)
    dsk = ds * tile_kept(case) if drop_ds_tile else ds
    out = (dsk @ k, dsk.transpose(2, 3) @ q, p.transpose(2, 3) @ do)
    return tuple(t.to(dt) for t in out) if round_out else out


@functools.lru_cache(maxsize=8)
def reference(case, dt, kind, rounded):
    """-> ((dQ, dK, dV), their allowances)"""
    x = make_inputs(case, dt, kind)
    ref = bwd_ref(case, x, dt, rounded)
    return ref, allowances(case, x, kind, ref)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def allowances(case, x, kind, ref):
    """an elementwise allowance beside the rule for dQ / dK / dV, None wherever the rule stands alone: dV always; dQ and dK of random and
    pair, the kinds that hold these two tensors to single keys.
    Where dS ~ 0 BY CONSTRUCTION (needle, forbid, pairf: one key takes the whole row, dP - delta cancels to nothing and dQ / dK are the
    residue of that cancellation; likewise a tensor that is zero because no row sees two keys) max|ref| of the tensor is no scale: the
    recipe in fp32 itself sits 10^3 .. 10^5 bounds away from fp64 there, and in fp16 such a tensor lies among the subnormals.  What any
    fp32 evaluation can promise is the worst-case bound of a dot product, n 2^-24 sum|terms| (the bound test_linear_backward_gpu.py uses
    for fp32), on the same expression with magnitudes: dS~ = P (|dO| |V|^T + |dO| . |O|) mult, dQ~ = dS~ |K|, dK~ = dS~^T |Q|, with
    n = 2 hd + 64 + the keys / queries summed over (dP and delta, the exponential's argument, the output product); in fp16 plus one
    step of the subnormal grid, 2^-24.  These kinds hold dV and the softmax statistics to single keys."""
    own = [float(r.double().abs().max()) for r in ref]
    if kind in ("random", "pair") and own[0] > 0.0 and own[1] > 0.0:
        return None, None, None
    B, H, Sq, Sk, hd, causal, mask = case
    q, k, v, do, o = (x[n].double() for n in ("q", "k", "v", "do", "o"))
    p = _softmax(q @ k.transpose(2, 3) * x["mult"], allowed(case, x["km"]))
    dsm = p * (do.abs() @ v.abs().transpose(2, 3) + (do * o).abs().sum(-1, keepdim=True)) * x["mult"]
    sub = 2.0 ** -24 if x["q"].dtype == FP16 else 0.0
    return ((2 * hd + 64 + Sk) * 2.0 ** -24 * (dsm @ k.abs()) + sub, (2 * hd + 64 + Sq) * 2.0 ** -24 * (dsm.transpose(2, 3) @ q.abs()) + sub, None)


def figures(got, ref, dt, fam, allow=None):
    """test_attention_cached_gpu.rule_figures on one of dQ / dK / dV [B,H,S,hd] with this file's floors: 2 % of max|ref| for the tight
    bound, max|ref| for the one every element of a matrix family must meet; `allow` (see allowances) is taken off |d| first
    -> (share of elements beyond the tight bound, worst |d| / the bound every element must meet, [B*H,S] 'an element of this row is
    beyond that bound')."""
    shape = ref.shape[:3]
    got, ref = got.double().flatten(0, 2), ref.double().flatten(0, 2)
    if allow is not None:
        d = got - ref
        got = ref + torch.sign(d) * (d.abs() - allow.flatten(0, 2)).clamp_min(0.0)
    vmax = max(float(ref.abs().max()), 1e-300)
    two = 1.0 if dt == BF else 2.0                                     # (rule_figures halves its floor in fp16)
    share = rule_figures(got, ref, dt, 0.02 * two * vmax)[0]
    _, worst, rows = rule_figures(got, ref, dt, (0.02 if fam == "scalar" else 1.0) * two * vmax)
    return share, worst, rows.view(shape[0] * shape[1], shape[2])


def cap_of(fam, rows):
    return 0.0 if fam == "scalar" else outlier_cap(rows)


def assert_rule(got, ref, fl, dt, fam, what, record=None):
    B, H = ref[0].shape[:2]
    for name, g_, r_, allow in zip(NAMES, got, ref, fl):
        share, worst, rows = figures(g_, r_, dt, fam, allow)
        cap = cap_of(fam, r_.shape[2])
        print(f"[attn-bwd] {what} {name}: share beyond the tight bound {share:.2e} (cap {cap:.0e}), worst |d| / bound {worst:.3f}")
        if record is not None:
            record.append((fam, _dtname(dt), name, share, worst))
        if bool(rows.any()):
            bh, r = (int(t) for t in rows.nonzero()[0])
            raise AssertionError(f"{what} {name}: {int(rows.sum())} of {rows.numel()} rows hold an element beyond the bound (worst |d| / bound "
                                 f"{worst:.3f}); first at (sample {bh // H}, head {bh % H}, row {r})")
        assert share <= cap, f"{what} {name}: {share:.2e} of the elements beyond the tight bound, cap {cap:.0e}"


# ---- running the kernels ----------------------------------------------------------------------------------------------------------------
def _rows(t):
    """[B,H,S,hd] -> [B*S, H*hd]"""
    B, H, S, hd = t.shape
    return t.transpose(1, 2).reshape(B * S, H * hd)


def _unrows(t, B, H, S, hd):
    return t.view(B, S, H, hd).transpose(1, 2)


def run_kernels(case, x, layout, v_pad=0):
    """-> (family observed, (dq, dk, dv) as [B,H,S,hd] on the CPU); asserts every output finite and the slack untouched.
    v_pad: layout (b) with the V rows (H * (hd + v_pad) wide) at a head stride of hd + v_pad."""
    ops = pkg("ops")
    B, H, Sq, Sk, hd, causal, mask = case
    D, dt = H * hd, x["q"].dtype
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=dt)
    km = None if x["km"] is None else x["km"].to(DEV)
    if layout == "a":
        W = 3 * D + 8                                                 # 8 unused columns behind q|k|v
        buf = torch.zeros(B * Sq, W, dtype=dt)
        buf[:, :D], buf[:, D:2 * D], buf[:, 2 * D:3 * D] = _rows(x["q"]), _rows(x["k"]), _rows(x["v"])
        buf, dbuf = buf.to(DEV), nan(B * Sq, W)
        s3, s1 = (Sq * W, hd, W), (Sq * D, hd, D)
        ins = (buf, buf[:, D:], buf[:, 2 * D:], _rows(x["o"]).contiguous().to(DEV), _rows(x["do"]).contiguous().to(DEV))
        outs, strides = (dbuf, dbuf[:, D:], dbuf[:, 2 * D:]), (s3, s3, s3, s1, s1, s3, s3, s3)
        read = lambda: tuple(_unrows(dbuf[:, i * D:(i + 1) * D].cpu().contiguous(), B, H, Sq, hd) for i in range(3))
        slack = lambda: dbuf[:, 3 * D:]
    elif layout == "b":
        Dv = H * (hd + v_pad)
        vrows = torch.zeros(B * Sk, H, hd + v_pad, dtype=dt)
        vrows[..., :hd] = _rows(x["v"]).view(B * Sk, H, hd)
        ins = tuple(t.contiguous().to(DEV) for t in (_rows(x["q"]), _rows(x["k"]), vrows.view(B * Sk, Dv), _rows(x["o"]), _rows(x["do"])))
        outs = (nan(B * Sq + 1, D), nan(B * Sk + 1, D), nan(B * Sk + 1, D))      # a guard row behind each
        sq, sk, sv = (Sq * D, hd, D), (Sk * D, hd, D), (Sk * Dv, hd + v_pad, Dv)
        strides = (sq, sk, sv, sq, sq, sq, sk, sk)
        read = lambda: tuple(_unrows(t[:-1].cpu(), B, H, S, hd) for t, S in zip(outs, (Sq, Sk, Sk)))
        slack = lambda: torch.cat([t[-1] for t in outs])
    else:
        ins = tuple(x[n].contiguous().to(DEV) for n in ("q", "k", "v", "o", "do"))
        outs = tuple(nan(B * H * S * hd + hd) for S in (Sq, Sk, Sk))
        sq, sk = (H * Sq * hd, Sq * hd, hd), (H * Sk * hd, Sk * hd, hd)
        strides = (sq, sk, sk, sq, sq, sq, sk, sk)
        read = lambda: tuple(t[:-hd].cpu().view(B, H, S, hd) for t, S in zip(outs, (Sq, Sk, Sk)))
        slack = lambda: torch.cat([t[-hd:] for t in outs])
    with _spy() as calls:
        ops.attention_bwd(*ins, *outs, strides, km, B, H, Sq, Sk, hd, causal, x["mult"])
    calls = [(n, a) for n, a in calls if n.startswith("ull_attention_bwd_")]
    assert len(calls) == 1, [n for n, _ in calls]
    name, a = calls[0]
    matrix = name.startswith("ull_attention_bwd_mfma_")
    assert int(a[18 if matrix else 14]) == hd
    fam = ("tiles128" if hd == 128 else "mfma64") if matrix else "scalar"
    got = read()
    assert bool(torch.isnan(slack()).all()), f"{_id(case)} layout ({layout}): the slack beside / behind the outputs was written"
    for name, t in zip(NAMES, got):
        assert bool(torch.isfinite(t.float()).all()), f"{_id(case)} layout ({layout}): {name} holds unwritten or non-finite elements"
    return fam, got


RECORD = []                # (family, dtype, tensor, share, worst |d| / bound) of every comparison of this session, summed up at the end


def _check_case(case, dt, scalar_only=False):
    B, H, Sq, Sk, hd, causal, mask = case
    assert max(Sq, Sk) <= 643 or (min(Sq, Sk) == 7 and max(Sq, Sk) == 4096)
    for kind in kinds_of(case):
        x = make_inputs(case, dt, kind)
        for layout in layouts_of(case, scalar_only):
            want = family_of(case, layout)
            if want == "scalar":
                assert_scalar_fits(case)
            fam, got = run_kernels(case, x, layout)
            what = f"{_id(case)} {_dtname(dt)} {kind} ({layout}) {fam}"
            assert fam == want, f"{what}: laid out for the {want} kernels"
            assert_rule(got, *reference(case, dt, kind, fam != "scalar"), dt, fam, what, RECORD)
            dead = ~x["live"][:, None].expand(B, H, Sq)
            assert not bool(got[0][dead].any()), f"{what}: dQ of a fully masked query row must be exactly zero"


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_MATRIX_SELF, ids=_id)
def test_attention_backward_causal_self(case, dt):
    """hd 64 / 128, Sq = Sk: 1 to 11 tiles on both double-buffer parities, tails of 1 and of 63 rows, the wave boundary (16) and the
    permuted 32-key block; layouts (a), (b) on the matrix kernels and (c) on the scalar ones."""
    _check_case(case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_MATRIX_OFFSET, ids=_id)
def test_attention_backward_causal_offset(case, dt):
    """koff = Sk - Sq from 1 to 192: moves kend / nkt of the dQ kernels, qbeg / qt0 of the dK/dV kernels and the tiles kernel's buffer
    parity (qt - qt0) & 1; first key blocks visible to every query (qbeg == 0), last key block starting beyond qt0 * 64."""
    _check_case(case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_MATRIX_NONCAUSAL, ids=_id)
def test_attention_backward_noncausal(case, dt):
    """Sq != Sk without a diagonal, on the matrix kernels (b) and the scalar ones (c)."""
    _check_case(case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_SCALAR + GRID_SCALAR_NONCAUSAL, ids=_id)
def test_attention_backward_scalar_family(case, dt):
    """the scalar kernels: hd 16 / 32 / 80 in every layout, hd 64 / 128 through layout (c); Sq around the 8-row blocks, the 32 staged
    queries and the 256 threads that stride the keys; the SAM decoder's 7 x 4096 / 4096 x 7 at hd 16."""
    _check_case(case, dt, scalar_only=True)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_MASKED, ids=_id)
def test_attention_backward_key_masks(case, dt):
    """right padding of Sk / 3 keys and left padding of 1 / 63 / 64 / 65 keys on the last sample, on every family.  Left padding under
    `causal` makes fully masked query rows: finite outputs, dQ exactly zero, dK / dV as with P = 0 in those rows (module docstring)."""
    B, H, Sq, Sk, hd, causal, mask = case
    if causal and mask[0] == "left" and mask[1] > Sk - Sq:
        assert not bool(make_inputs(case, dt, "random")["live"].all())
    _check_case(case, dt)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
@pytest.mark.parametrize("case", GRID_TWINS, ids=_id)
def test_attention_backward_scalar_against_matrix(case, dt):
    """layouts (b) (matrix kernels) and (c) (scalar kernels) on the same values: both meet the rule against their reference; their mutual
    worst |d| is printed in the rule's units and not asserted (the rounding points differ)."""
    for kind in kinds_of(case):
        x = make_inputs(case, dt, kind)
        fam_b, got_b = run_kernels(case, x, "b")
        fam_c, got_c = run_kernels(case, x, "c")
        what = f"{_id(case)} {_dtname(dt)} {kind}"
        assert (fam_b, fam_c) == (family_of(case, "b"), "scalar"), what
        assert_rule(got_b, *reference(case, dt, kind, True), dt, fam_b, what + " (b)")
        assert_rule(got_c, *reference(case, dt, kind, False), dt, fam_c, what + " (c)")
        for name, b_, c_, allow in zip(NAMES, got_b, got_c, reference(case, dt, kind, False)[1]):
            share, worst, _ = figures(b_, c_, dt, fam_b, allow)
            print(f"[attn-bwd] {what} {name}: {fam_b} against scalar: share beyond the tight bound {share:.2e}, worst |d| / loose bound {worst:.3f}")


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_attention_backward_unaligned_value_head_stride_takes_the_scalar_kernels(dt):
    """hd 128 with the V rows at a head stride of hd + 4 (8-byte but not 16-byte aligned; the token stride still 16-byte aligned): legal
    for the scalar kernels only -- the LDS-DMA of the tiles kernels copies 16-byte chunks and ull_attention_bwd_mfma_ refuses the layout.
    ops.attention_bwd routes by what the C entry requires instead of raising."""
    case = _c(2, 2, 65, 129, 128)
    for kind in ("random", "pair"):
        x = make_inputs(case, dt, kind)
        fam, got = run_kernels(case, x, "b", v_pad=4)
        assert fam == "scalar", f"ran the {fam} kernels"
        assert_rule(got, *reference(case, dt, kind, False), dt, fam, f"{_id(case)} {_dtname(dt)} {kind} V head stride 132")


@gpu
@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_attention_backward_scalar_lds_limit(dt):
    """hd 16: 5076 keys are the last that fit (8 * Sk + 16 * hd + 32 floats <= 160 KiB - 256); 5077 must raise the library's LDS error
    and launch nothing (the outputs keep their NaN fill)."""
    ops = pkg("ops")
    B, H, Sq, Sk, hd = 1, 1, 7, 5077, 16
    assert (AB_R * Sk + 2 * AB_R * hd + 4 * AB_R) * 4 > AB_LDS_MAX >= (AB_R * (Sk - 1) + 2 * AB_R * hd + 4 * AB_R) * 4
    g = torch.Generator().manual_seed(5)
    q, o, do = (torch.randn(Sq, hd, generator=g).to(dt).to(DEV) for _ in range(3))
    k, v = (torch.randn(Sk, hd, generator=g).to(dt).to(DEV) for _ in range(2))
    dq, dk, dv = (torch.full((S, hd), float("nan"), device=DEV, dtype=dt) for S in (Sq, Sk, Sk))
    sq, sk = (Sq * hd, hd, hd), (Sk * hd, hd, hd)
    with pytest.raises(RuntimeError, match="ULL_ERR_LDS"):
        ops.attention_bwd(q, k, v, o, do, dq, dk, dv, (sq, sk, sk, sq, sq, sq, sk, sk), None, B, H, Sq, Sk, hd, False, hd ** -0.5)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dq, dk, dv)), "a kernel ran"


@gpu
def test_attention_backward_summary():
    """prints the worst figures per family, dtype and tensor of the comparisons above (docs/experiments.md keeps a record); the 2-ulp rule
    against one plain tensor, so that helpers' own assertions stay the yardstick of `figures`."""
    worst = {}
    for fam, dtn, name, share, w in RECORD:
        s0, w0, n0 = worst.get((fam, dtn, name), (0.0, 0.0, 0))
        worst[(fam, dtn, name)] = (max(s0, share), max(w0, w), n0 + 1)
    for key in sorted(worst):
        s, w, n = worst[key]
        print(f"[attn-bwd] summary {key[0]} {key[1]} {key[2]}: {n} comparisons, worst share {s:.2e}, worst |d| / bound {w:.3f}")
    case = _c(2, 2, 33, 33, 32)
    for dt in DTS:
        x = make_inputs(case, dt, "random")
        fam, got = run_kernels(case, x, "b")
        for g_, r_ in zip(got, reference(case, dt, "random", False)[0]):
            (assert_close_bf16 if dt == BF else assert_close_f16)(g_, r_.double(), ulps=2.0, what=f"{_id(case)} {_dtname(dt)}")


# ---- CPU: the reference and the inputs themselves ----------------------------------------------------------------------------------------
def _ref_family(case):
    """the rounding points of the family the case's layouts (a) / (b) run on (the scalar grid's hd 64 / 128 cases: layout (c))."""
    return family_of(case, "b") if case not in GRID_SCALAR else "scalar"


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_the_backward_reference_stays_inside_the_caps_against_fp64(dt):
    """The caps are a condition, not a measurement: the same recipe with every sum in fp32, held against the fp64 reference at equal
    rounding points over the whole grid and all kinds, stays within a third of the cap (share) and a third of the bound every element
    must meet -- for both sets of rounding points wherever a case runs on a matrix and on the scalar family.  The fp32 recipe is taken
    BEFORE its outputs are rounded to the element type (a kernel's accumulators): rounding them too adds one flip of the last bit against
    the rounded fp64 value, 0.25 .. 0.5 of the bound wherever the tensor's largest elements sit low in their binade, whatever the
    recipe does (printed as the second figure); unrounded it is the half ulp of the reference's own rounding, <= 0.25, plus the recipe's
    error.  A case that missed a third was given more heads, never a wider cap."""
    top = {}
    for case in ALL_CASES:
        fams = {_ref_family(case)} | ({"scalar"} if case[4] >= 64 else set())
        for kind in kinds_of(case):
            x = make_inputs(case, dt, kind)
            for fam in sorted(fams):
                ref = bwd_ref(case, x, dt, fam != "scalar")
                fl = allowances(case, x, kind, ref)
                f32 = bwd_ref(case, x, dt, fam != "scalar", ft=torch.float32, round_out=False)
                for name, a, b, vmax in zip(NAMES, f32, ref, fl):
                    share, worst, _ = figures(a, b, dt, fam, vmax)
                    _, flip, _ = figures(a.to(dt), b, dt, fam, vmax)
                    cap = cap_of(fam, b.shape[2])
                    s0, w0, f0 = top.get(fam, (0.0, 0.0, 0.0))
                    top[fam] = (max(s0, share / cap if cap else share), max(w0, worst), max(f0, flip))
                    assert share <= cap / 3 and worst <= 1 / 3, (_id(case), kind, fam, name, share, worst)
    for fam, (s, w, f) in sorted(top.items()):
        print(f"[attn-bwd] {_dtname(dt)} fp32 recipe against fp64, {fam} rounding points: worst share / cap {s:.3f}, worst |d| / bound {w:.3f} "
              f"(outputs rounded: {f:.3f})")


@pytest.mark.parametrize("dt", DTS, ids=_dtname)
def test_backward_inputs_expose_a_shifted_diagonal_a_dropped_tile_and_an_ignored_mask(dt):
    """Guards the inputs, not the kernels: the reference run with a deliberately wrong rule must leave the rule in EVERY row the error
    touches, separately for dQ, dK and dV, with the kinds taken together (a row counts as exposed when one kind shows it):
      * shift -1   the diagonal one key short (not causal: the last key not seen);
      * tile       the tile holding a row's diagonal key (not causal: the last key tile) not streamed at all;
      * ds_tile    that tile left out of dS K and dS^T Q only, statistics and dV correct (a parameter of the reference);
      * shift +1   the diagonal one key long (causal only);
      * mask       the key mask ignored (left padding).
    A (query, key) pair counts as touched when the wrong rule changes its visibility and some kind gives it weight by construction: the
    row's last allowed key (needle, pair), its first forbidden key (forbid, pairf).  Touched rows: dQ -- the query of such a pair, if it
    sees more than one key under either rule (a single visible key has dS = 0); dV -- the key of such a pair; dK -- the key of such a pair
    whose query sees more than one key.  Below hd 64 there is no pair / pairf, needle and forbid have dS ~ 0, and only dV is required."""
    gaps = []
    for case in ALL_CASES:
        B, H, Sq, Sk, hd, causal, mask = case
        fam = _ref_family(case)
        kinds = kinds_of(case)
        xs = {kind: make_inputs(case, dt, kind) for kind in kinds}
        km = xs["random"]["km"]
        refs = {kind: bwd_ref(case, xs[kind], dt, fam != "scalar") for kind in kinds}
        fls = {kind: allowances(case, xs[kind], kind, refs[kind]) for kind in kinds}
        ok = allowed(case, km)[:, 0]                                                    # [B, Sq, Sk]
        last, _ = targets(case, km, "needle")
        forb, has = targets(case, km, "forbid")
        onehot = lambda idx, rows: torch.nn.functional.one_hot(idx, Sk).bool() & rows[..., None]
        live = ok.any(-1)
        rules = [("shift -1", dict(shift=-1)), ("tile", dict(drop_last_tile=True)), ("ds_tile", dict(drop_ds_tile=True))]
        if causal:
            rules.append(("shift +1", dict(shift=1)))
        if mask is not None and mask[0] == "left":
            rules.append(("mask", dict(ignore_mask=True)))
        for rule, wrong in rules:
            if rule == "ds_tile":
                bad_al = ok & tile_kept(case)
            else:
                bad_al = allowed(case, km, **wrong)[:, 0]
            changed = ok != bad_al
            pairs = changed & (onehot(last, live) | onehot(forb, has))                  # touched (query, key) pairs
            many = (ok.sum(-1) > 1) | ((bad_al.sum(-1) > 1) & (rule != "ds_tile"))
            touched = (pairs.any(-1) & many, (pairs & many[..., None]).any(1), pairs.any(1))      # dQ [B,Sq], dK [B,Sk], dV [B,Sk]
            exposed = [torch.zeros(B * H, n, dtype=torch.bool) for n in (Sq, Sk, Sk)]
            for kind in kinds:
                out = bwd_ref(case, xs[kind], dt, fam != "scalar", **wrong)
                for i in range(3):
                    exposed[i] |= figures(out[i], refs[kind][i], dt, fam, fls[kind][i])[2]
            for i, name in enumerate(NAMES):
                if hd < 64 and name != "dV" or rule == "ds_tile" and name == "dV":
                    continue
                miss = touched[i][:, None] & ~exposed[i].view(B, H, -1)
                if bool(miss.any()):
                    gaps.append(f"{_id(case)} rule '{rule}' {name}: {int(miss.sum())} of {int(touched[i].sum()) * H} touched rows stay inside the "
                                f"rule; first (sample, head, row) {tuple(int(t) for t in miss.nonzero()[0])}")
    assert not gaps, f"{len(gaps)} gaps in the inputs ({_dtname(dt)}):\n" + "\n".join(gaps[:40])
