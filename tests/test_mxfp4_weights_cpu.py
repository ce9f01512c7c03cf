"""No GPU: UllavaCoreForCausalLM.quantize_weights("mxfp4") (MXFP4 weight-only inference) -- its refusals, which come before any device work,
the test's own torch restatement of the format (the GPU tests hold the quantize / dequantize kernels to it), and the resident layout's round
trip through the standard layout.

The format: per row and per block of 32 consecutive K elements one scale 2^s, s the smallest integer with amax * 2^-s <= 6 (all-zero block:
s = 0), clamped to [-125, 126], stored as the E8M0 byte s + 127; elements e2m1(w * 2^-s) -- 0, 0.5, 1, 1.5, 2, 3, 4, 6 as codes 0 .. 7, sign
in bit 3 -- rounded to nearest with ties to the even code (at s = 126 saturating at 3, the largest finite value there); standard layout: codes [N, K / 2] with element 2i in the low nibble, scales [N, K / 32].
"""
import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def mxfp4_reference(w: torch.Tensor):
    """(codes uint8 [N, K / 2], scales uint8 [N, K / 32]) in the standard layout, on the CPU."""
    N, K = w.shape
    wb = w.double().view(N, K // 32, 32)                       # (bf16 -> double is exact, and so is every product with 2^-s below)
    amax = wb.abs().amax(dim=2)
    s = torch.zeros_like(amax, dtype=torch.int64)
    nz = amax > 0
    s[nz] = torch.ceil(torch.log2(amax[nz] / 6.0)).long()
    # settle the float log2 exactly: 6 * 2^s >= amax > 6 * 2^(s - 1)
    s = torch.where(nz & (amax > 6.0 * torch.pow(2.0, s.double())), s + 1, s)
    s = torch.where(nz & (amax <= 6.0 * torch.pow(2.0, (s - 1).double())), s - 1, s)
    s = s.clamp(-125, 126)
    a = (wb * torch.pow(2.0, -s.double())[..., None]).abs()
    # explicit midpoints between neighbouring e2m1 values; a tie goes to the even code
    mag = ((a > 0.25).long() + (a >= 0.75).long() + (a > 1.25).long() + (a >= 1.75).long() + (a > 2.5).long() + (a >= 3.5).long() + (a > 5.0).long())
    # 4 * 2^126 and 6 * 2^126 are 2^128 and above, which no float holds: at s = 126 the magnitude saturates at the code of 3
    mag = torch.where(s[..., None] == 126, mag.clamp(max=5), mag)
    sign = torch.signbit(w.float()).view(N, K // 32, 32).long()
    code = (mag | (sign << 3)).view(N, K // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return codes, (s + 127).to(torch.uint8)


def mxfp4_dequant_reference(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K]: e2m1 * 2^(scale - 127), every product exact."""
    N = codes.shape[0]
    c = torch.stack((codes & 15, codes >> 4), dim=-1).view(N, -1).long()
    v = E2M1[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)
    sc = torch.pow(2.0, scales.double() - 127.0).float()
    return (v.view(N, -1, 32) * sc[..., None]).view(N, -1)


TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
TIES_TO = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]


def edge_blocks(K: int = 32) -> torch.Tensor:
    """bf16 rows, every block of 32 filled alike: all zeros; amax exactly 6 * 2^k and the next bf16 above it, k in (-10, 0, 3); every tie
    between two e2m1 values and its negative (next to a 6, so that s = 0); a block under the s clamp; a Gaussian block."""
    rows = [torch.zeros(32)]
    for k in (-10, 0, 3):
        r = torch.linspace(-1, 1, 32) * 6 * 2.0 ** k
        r[5] = 6 * 2.0 ** k
        rows.append(r)
        r = r.clone()
        r[7] = torch.tensor(6 * 2.0 ** k).bfloat16().float().nextafter(torch.tensor(float("inf"))).bfloat16().float().item()
        if r[7] <= 6 * 2.0 ** k:                                   # (nextafter in fp32 rounds back down in bf16: step one bf16 ulp instead)
            r[7] = 6 * 2.0 ** k * (1 + 2.0 ** -7)
        rows.append(r)
    t = torch.zeros(32)
    t[0] = 6.0
    t[1:8] = torch.tensor(TIES)
    t[8:15] = -torch.tensor(TIES)
    t[15] = -0.0
    t[16] = -0.125                                                 # rounds to -0
    rows.append(t)
    u = torch.zeros(32)                                            # under the clamp: amax = 2^-130 would give s = -132
    u[0] = 2.0 ** -130
    u[1] = -(2.0 ** -127)                                          # 0.25 at s = -125: a tie, to 0
    u[2] = 2.0 ** -126                                             # 0.5 at s = -125
    u[3] = 3 * 2.0 ** -128                                         # 0.375 -> 0.5
    rows.append(u)
    g = torch.Generator().manual_seed(3)
    rows.append(torch.randn(32, generator=g) * 0.02)
    return torch.stack(rows).bfloat16().repeat(1, K // 32)


def test_quantize_weights_mxfp4_refuses_non_bf16():
    for dtype in (torch.float16, torch.float32):
        model = _tiny_core(dtype)
        with pytest.raises(NotImplementedError, match="bf16"):
            model.quantize_weights("mxfp4")
        assert model.weight_quantization is None


def test_quantize_weights_mxfp4_refuses_lora_adapters():
    model = _tiny_core()
    model.add_lora(r=4)
    with pytest.raises(NotImplementedError, match="merge_lora"):
        model.quantize_weights("mxfp4")
    assert model.weight_quantization is None


def test_quantize_weights_unknown_format_lists_both():
    with pytest.raises(ValueError, match="fp8_e4m3.*mxfp4"):
        _tiny_core().quantize_weights("int4")


def test_quantize_weights_mxfp4_refuses_k_not_multiple_of_32_before_device_work():
    ops = pkg("ops")
    model = _tiny_core()                                           # on the CPU: anything that reached the device path would raise RuntimeError
    model.config.intermediate_size = model.config.intermediate_size + 16
    with pytest.raises(NotImplementedError, match="32"):
        model.quantize_weights("mxfp4")
    assert model.weight_quantization is None
    with pytest.raises(NotImplementedError, match="32"):
        ops.quantize_mxfp4(torch.zeros(4, 48, dtype=torch.bfloat16))


def test_format_restatement_on_edge_blocks():
    w = edge_blocks()
    codes, scales = mxfp4_reference(w)
    s = scales.long()[:, 0] - 127
    deq = mxfp4_dequant_reference(codes, scales)
    assert int(s[0]) == 0 and int(codes[0].sum()) == 0                               # all-zero block: s = 0
    # rows 1, 3, 5: amax exactly 6 * 2^k -> s = k and the largest code (7) at the max; rows 2, 4, 6: the next bf16 above -> s = k + 1
    for i, k in ((1, -10), (3, 0), (5, 3)):
        assert int(s[i]) == k and int(codes[i, 2] >> 4) == 7                         # element 5: high nibble of byte 2
        assert int(s[i + 1]) == k + 1
    amax = w.float().abs().amax(dim=1)
    fit = slice(1, 8)
    assert bool((amax[fit] <= 6.0 * torch.pow(2.0, s[fit].float())).all()) and bool((amax[fit] > 3.0 * torch.pow(2.0, s[fit].float())).all())
    # ties go to the even code, on both signs; -0 stays -0, and -0.125 rounds to -0
    t = deq[7]
    assert int(s[7]) == 0
    assert t[1:8].tolist() == TIES_TO and t[8:15].tolist() == [-x for x in TIES_TO]
    assert int(codes[7, 7] >> 4) == 8 and int(codes[7, 8] & 15) == 8                 # elements 15 and 16: code 8 = -0
    assert int(codes[7, 0] >> 4) == 0                                                # element 1 (0.25): +0, no sign bit
    # under the clamp: s = -125, and everything at or below a quarter of 2^-125 is 0
    assert int(s[8]) == -125
    assert deq[8, :4].tolist() == [0.0, -0.0, 2.0 ** -126, 2.0 ** -126]
    nzv = deq[deq != 0].abs()
    assert bool((nzv >= 2.0 ** -126).all()), "every non-zero dequantized value is a normal float"
    # the Gaussian block: each element is within half of the widest step (2 * 2^s) of its value, and the block's amax -- in (3, 6] * 2^s by
    # the scale rule -- maps to 3, 4 or 6
    gq, gw = deq[9, :32], w[9, :32].float()
    assert float(gq.abs().max()) in tuple(m * 2.0 ** int(s[9]) for m in (3.0, 4.0, 6.0))
    assert bool(((gq - gw).abs() <= 2.0 ** int(s[9])).all())


def huge_blocks() -> torch.Tensor:
    """bf16 rows of one block each whose amax is above 3 * 2^126, up to the bf16 maximum: s = 126, where only the codes up to 3 are finite."""
    big = torch.tensor(torch.finfo(torch.bfloat16).max)
    rows = []
    for top in (big, -big, torch.tensor(3.5 * 2.0 ** 126), torch.tensor(3.25 * 2.0 ** 126)):
        r = torch.linspace(-1, 1, 32) * 2.0 ** 126
        r[3] = top
        r[4] = 2.0 ** 127                                          # 2 at s = 126
        rows.append(r)
    return torch.stack(rows).bfloat16()


def test_restatement_saturates_at_the_largest_finite_value():
    w = huge_blocks()
    codes, scales = mxfp4_reference(w)
    assert scales[:, 0].tolist() == [253, 253, 253, 253]                              # s = 126
    deq = mxfp4_dequant_reference(codes, scales)
    assert bool(torch.isfinite(deq).all())
    assert deq[:, 3].tolist() == [3 * 2.0 ** 126, -3 * 2.0 ** 126, 3 * 2.0 ** 126, 3 * 2.0 ** 126]
    assert deq[:, 4].tolist() == [2.0 ** 127] * 4
    assert torch.equal(deq.bfloat16().float(), deq)


def test_restatement_dequantization_is_exact_in_bf16():
    g = torch.Generator().manual_seed(5)
    w = torch.cat([edge_blocks(64), (torch.randn(16, 64, generator=g) * 0.02).bfloat16()])
    codes, scales = mxfp4_reference(w)
    deq = mxfp4_dequant_reference(codes, scales)
    assert torch.equal(deq.bfloat16().float(), deq)                                  # two significant bits, normal exponents: bf16 holds it
    # and quantizing the dequantized weight again changes nothing (the twin is a fixed point)
    c2, s2 = mxfp4_reference(deq.bfloat16())
    d2 = mxfp4_dequant_reference(c2, s2)
    assert torch.equal(d2, deq)


@pytest.mark.parametrize("K", [32, 96, 2048, 4096, 2048 + 96, 11008])
def test_resident_layout_round_trip(K):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(K)
    N = 5
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(2, 254, (N, K // 32), generator=g, dtype=torch.uint8)
    q = ops.Mxfp4Weight.from_standard(codes, scales)
    assert tuple(q.shape) == (N, K) and q.codes.shape == (N, K // 2) and q.scales.shape[1] % 4 == 0
    c2, s2 = q.to_standard()
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # a permutation of the bytes within each row
    assert torch.equal(q.codes.sort(dim=1).values, codes.sort(dim=1).values)
    nsb = K // 2048
    if nsb:
        # inside a whole superblock the chunks lane, lane + 64, lane + 128, lane + 192 of a GEMV lane are 16 adjacent bytes, and the scale
        # bytes of their four blocks are 4 adjacent bytes
        lane, b = 37, nsb - 1
        for gq in range(4):
            c = b * 256 + gq * 64 + lane
            assert torch.equal(q.codes[:, b * 1024 + lane * 16 + gq * 4:b * 1024 + lane * 16 + gq * 4 + 4], codes[:, c * 4:c * 4 + 4])
            assert torch.equal(q.scales[:, b * 64 + (lane // 4) * 4 + gq], scales[:, c // 4])
    # after the last whole superblock: the standard order
    assert torch.equal(q.codes[:, nsb * 1024:], codes[:, nsb * 1024:])
    assert torch.equal(q.scales[:, nsb * 64:K // 32], scales[:, nsb * 64:])
