"""CPU: the float64 references and the comparator of the activation sweeps (tests/test_activation_sweep_gpu.py), checked without a GPU.

* the references against torch's own CPU kernels of the same dtype over every finite 16-bit input: they may differ only where torch's fp32
  evaluation and the float64 one round differently -- counts measured here and pinned, all far below 0.1 % of the inputs, none NaN;
* where the references round: float64 -> fp32 -> 16 bits, and what a single rounding from float64 would change (nine fp16 inputs);
* the comparator rejects one planted NaN, a deviation of two ulps, gate and up swapped, and one output row shifted by one;
* the planting: one-hot activation rows recover every finite pattern exactly through an fp32 matmul.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import (all_patterns, planted, quick_gelu_ref, rnd16, silu_ref, sweep_compare, swiglu_bwd_ref, swiglu_ref, ulp16, SWEEP_FLOOR)

BF, H = torch.bfloat16, torch.float16
DTS = [BF, H]
N_FINITE = {BF: 65280, H: 63488}
# inputs whose float64 reference differs bitwise from torch's CPU kernel of the dtype (measured)
#   SiLU bf16: the 17 gates -97 .. -89 -- torch's fp32 exp(-x) has overflowed (silu = -0.0) where x * e^x is still a bf16 subnormal or small normal
#   SiLU fp16: one input (-2.7246) where torch's fp32 kernel rounds the other way; this depends on the host's kernel
# (bf16: pinned, the 17 are a property of fp32 overflow; fp16: capped at twice the measurement, like the QuickGELU counts)
SILU_VS_TORCH = {BF: 17, H: 1}
#   QuickGELU bf16: 9 inputs in [-54.25, -52.25] -- the same overflow, of the sigmoid of 1.702 x in [-92.5, -89]
#   QuickGELU fp16: 4 inputs in 8e-4 < |x| < 7e-3 where torch's vectorised fp32 sigmoid rounds the other way (one ulp of the sigmoid)
# the QuickGELU counts depend on the host's sigmoid kernel, so they are capped at twice the measurement (the rule of the GPU sweep's caps)
QGELU_VS_TORCH = {BF: 9, H: 4}


def _finite(dt):
    x, fin = all_patterns(dt)
    assert int(fin.sum()) == N_FINITE[dt]
    return x[fin].contiguous()


@pytest.mark.parametrize("dt", DTS)
def test_rnd16_rounds_once(dt):
    """rnd16 is the identity on 16-bit values, rounds ties to even, does not round twice, and overflows to the infinity."""
    x = _finite(dt)
    assert torch.equal(rnd16(x.double(), dt).view(torch.int16), x.view(torch.int16))
    one_ulp = 2.0 ** -7 if dt == BF else 2.0 ** -10
    # 1 + ulp/2 is a tie (-> 1, even); a hair above it goes up, although float32 would first round the hair away (the double rounding)
    t = torch.tensor([1.0 + one_ulp / 2, 1.0 + one_ulp / 2 + 2.0 ** -40, 1.0 + 3 * one_ulp / 2, 1e39, -1e39, 1e-60], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + one_ulp, 1.0 + 2 * one_ulp, float("inf"), float("-inf"), 0.0], dtype=torch.float64)
    assert torch.equal(rnd16(t, dt).double(), want)
    assert float(ulp16(torch.tensor([1.0]), dt)) == one_ulp and float(ulp16(torch.tensor([0.0]), dt)) == 2.0 ** (-133 if dt == BF else -24)


@pytest.mark.parametrize("dt", DTS)
def test_silu_reference_against_torch(dt):
    x = _finite(dt)
    ref, tor = silu_ref(x, dt), F.silu(x)
    assert not bool(torch.isnan(ref).any()) and not bool(torch.isnan(tor).any())
    diff = ref.view(torch.int16) != tor.view(torch.int16)
    n = int(diff.sum())
    print(f"SiLU {dt}: float64 reference differs from torch CPU in {n} of {x.numel()} inputs: {sorted(x[diff].float().tolist())[:20]}")
    assert (n == SILU_VS_TORCH[dt] if dt == BF else n <= 2 * SILU_VS_TORCH[dt]) and n < 1e-3 * x.numel()
    # and where they differ, by no more than the comparator's own bound
    assert bool(((ref.double() - tor.double()).abs() <= torch.clamp(ulp16(ref, dt), min=SWEEP_FLOOR[dt])).all())


@pytest.mark.parametrize("dt", DTS)
def test_quick_gelu_reference_against_torch(dt):
    x = _finite(dt)
    ref, tor = quick_gelu_ref(x, dt), x * torch.sigmoid(1.702 * x)
    assert not bool(torch.isnan(ref).any()) and not bool(torch.isnan(tor).any())
    diff = ref.view(torch.int16) != tor.view(torch.int16)
    n = int(diff.sum())
    print(f"QuickGELU {dt}: float64 reference differs from torch CPU in {n} of {x.numel()} inputs: {sorted(x[diff].float().tolist())[:20]}")
    assert n <= 2 * QGELU_VS_TORCH[dt] and n < 1e-3 * x.numel()
    # one ulp of the 16-bit sigmoid is up to two of the product
    assert bool(((ref.double() - tor.double()).abs() <= torch.clamp(2 * ulp16(ref, dt), min=SWEEP_FLOOR[dt])).all())


def test_the_fp32_step_of_the_references_matters_only_at_fp32_ties():
    """The references cast the float64 value to fp32 and then to 16 bits, as the reference's fp32 evaluation does (helpers.rnd32_16).  Rounded
    once from float64 instead, bf16 gives the same bits everywhere; fp16 differs in 2 SiLU inputs (2^-24: silu = 2^-25 (1 + 2^-26), and
    -2.7246) and 7 QuickGELU inputs with |x| < 7e-3, where sigmoid(u) = 1/2 + u/4 - u^3/48 is an fp16 tie to within fp32 -- there by up to
    two ulps of the product, which no fp32 evaluation, torch's included, can follow."""
    for dt, n_silu, n_q in ((BF, 0, 0), (H, 2, 7)):
        x = _finite(dt)
        d = silu_ref(x, dt).view(torch.int16) != silu_ref(x, dt, rnd=rnd16).view(torch.int16)
        assert int(d.sum()) == n_silu, (dt, x[d].tolist())
        q1, q2 = quick_gelu_ref(x, dt), quick_gelu_ref(x, dt, rnd=rnd16)
        d = q1.view(torch.int16) != q2.view(torch.int16)
        assert int(d.sum()) == n_q and (n_q == 0 or float(x[d].float().abs().max()) < 7e-3), (dt, x[d].tolist())
        assert bool(((q1.double() - q2.double()).abs() <= 2 * ulp16(q2, dt)).all())


@pytest.mark.parametrize("dt", DTS)
def test_swiglu_references_at_the_edges(dt):
    """far negative gates give -0.0 (never NaN), the product with up = -3 flips the sign, and fp16 overflows to the reference's infinity."""
    g = torch.tensor([-60000.0, -1000.0, -100.0 if dt == H else -200.0, 0.0, 32768.0], dtype=torch.float64).to(dt)
    one, m3 = torch.ones_like(g), torch.full_like(g, -3.0)
    assert swiglu_ref(g, one, dt).tolist() == [-0.0, -0.0, -0.0, 0.0, 32768.0] and str(float(swiglu_ref(g, one, dt)[0])) == "-0.0"
    want = [0.0, 0.0, 0.0, -0.0, float("-inf") if dt == H else -98304.0]
    assert swiglu_ref(g, m3, dt).tolist() == want and str(float(swiglu_ref(g, m3, dt)[3])) == "-0.0"
    dg, du = swiglu_bwd_ref(g, m3, one, dt)
    assert dg.tolist()[:3] == [0.0, 0.0, 0.0] and float(dg[3]) == -1.5 and float(dg[4]) == -3.0 and float(du[3]) == 0.0 and float(du[4]) == 32768.0


@pytest.mark.parametrize("dt", DTS)
def test_comparator_rejects_what_it_must(dt):
    x = _finite(dt)
    I, K = 64, x.numel() // 64
    g = x[: I * K].view(I, K)
    u = torch.full_like(g, -3.0)
    ref = swiglu_ref(g, u, dt)
    assert sweep_compare(ref.clone(), ref, dt, 0, "identity") == 0
    # one ulp on one element passes (c) and is counted by (d)
    up1 = ref.clone().view(-1)
    i = int((ref.view(-1).float() == 1.5).nonzero()[0]) if bool((ref.view(-1).float() == 1.5).any()) else int((ref.view(-1).float().abs() > 1).nonzero()[0])
    up1.view(torch.int16)[i] += 1
    assert sweep_compare(up1, ref, dt, 1, "one ulp") == 1
    with pytest.raises(AssertionError, match="differ bitwise"):
        sweep_compare(up1, ref, dt, 0, "one ulp, cap 0")
    # a single NaN
    bad = ref.clone().view(-1)
    bad[12345] = float("nan")
    with pytest.raises(AssertionError, match="NaN"):
        sweep_compare(bad, ref, dt, 10 ** 6, "one NaN")
    # two ulps on one element
    bad = ref.clone().view(-1)
    bad.view(torch.int16)[i] += 2
    with pytest.raises(AssertionError, match="beyond one ulp"):
        sweep_compare(bad, ref, dt, 10 ** 6, "two ulps")
    # gate and up swapped
    with pytest.raises(AssertionError):
        sweep_compare(swiglu_ref(u, g, dt), ref, dt, 10 ** 6, "swapped")
    # one output row shifted by one
    bad = ref.clone()
    bad[7] = torch.roll(ref[7], 1)
    with pytest.raises(AssertionError):
        sweep_compare(bad, ref, dt, 10 ** 6, "row shifted")
    # a finite value where the reference overflowed, and an infinity where it did not
    if dt == H:
        assert bool(torch.isinf(ref).any())
        bad = ref.clone().view(-1)
        bad[int(torch.isinf(ref.view(-1)).nonzero()[0])] = 65504.0
        with pytest.raises(AssertionError, match="infinities"):
            sweep_compare(bad, ref, dt, 10 ** 6, "inf missed")
    bad = ref.clone().view(-1)
    bad[i] = float("inf")
    with pytest.raises(AssertionError, match="beyond one ulp"):
        sweep_compare(bad, ref, dt, 10 ** 6, "spurious inf")
    # `valid` takes elements out of every check
    bad = ref.clone().view(-1)
    bad[12345] = float("nan")
    keep = torch.ones(bad.numel(), dtype=torch.bool)
    keep[12345] = False
    assert sweep_compare(bad, ref, dt, 0, "masked NaN", valid=keep) == 0


@pytest.mark.parametrize("dt", DTS)
def test_one_hot_rows_plant_every_pattern_exactly(dt):
    """x[m] = e_m against a weight whose first columns carry the patterns: the fp32 matmul returns each of them bit for bit (every other term
    is 0 * finite), whatever finite values the other columns hold."""
    pat, fin = all_patterns(dt)
    M, K, I = 16, 64, 4096
    w = pat.view(I, M).repeat(1, K // M)
    x = torch.zeros(M, K, dtype=dt)
    x[torch.arange(M), torch.arange(M)] = 1
    y = x.float() @ w.float().t()                                   # [M, I]
    got = y.t().reshape(-1)
    assert torch.equal(got, pat.float())                            # exact in fp32 already, not only after the rounding
    # bit for bit too, except the one pattern an accumulator cannot hold: -0.0 arrives as +0.0 (0 + -0 = +0), see planted()
    assert torch.equal(got.to(dt).view(torch.int16)[fin], planted(pat).view(torch.int16)[fin])
    assert int((planted(pat).view(torch.int16) != pat.view(torch.int16)).sum()) == 1
