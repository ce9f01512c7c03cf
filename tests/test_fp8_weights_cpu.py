"""No GPU: UllavaCoreForCausalLM.quantize_weights (FP8 e4m3 weight-only inference) -- its refusals, which come before any device work, and
the test's own torch restatement of the per-row scale rule that the GPU tests hold the quantize kernel to."""
import pytest
import torch

from helpers import load_fixture, pkg


def fp8_reference(w: torch.Tensor):
    """(codes uint8 [N, K], scales fp32 [N]) on the CPU: s = the smallest integer with amax|w_row| * 2^-s <= 448 (all-zero row: 0),
    codes = e4m3fn(w * 2^-s) rounded to nearest even (torch's CPU cast), scale = 2^s."""
    wf = w.float()
    amax = wf.abs().amax(dim=1).double()
    s = torch.zeros_like(amax, dtype=torch.int64)
    nz = amax > 0
    s[nz] = torch.ceil(torch.log2(amax[nz] / 448.0)).long()
    # settle the float log2 exactly: 448 * 2^s >= amax > 448 * 2^(s - 1)
    s = torch.where(nz & (amax > 448.0 * torch.pow(2.0, s.double())), s + 1, s)
    s = torch.where(nz & (amax <= 448.0 * torch.pow(2.0, (s - 1).double())), s - 1, s)
    scale = torch.pow(2.0, s.double()).float()
    codes = (wf * torch.pow(2.0, -s.double()).float()[:, None]).to(torch.float8_e4m3fn)
    return codes.view(torch.uint8), scale


def dequant_reference(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    return (codes.view(torch.float8_e4m3fn).float() * scales[:, None]).to(torch.bfloat16)


def edge_rows(K: int = 64) -> torch.Tensor:
    """bf16 rows that exercise the scale rule and the rounding: all zeros, amax exactly 448 * 2^k, just above it, ties between two e4m3
    values, and values in e4m3's subnormal range next to a large one."""
    rows = [torch.zeros(K)]
    for k in (-10, 0, 3):
        r = torch.linspace(-1, 1, K) * 448 * 2.0 ** k
        r[5] = 448 * 2.0 ** k
        rows.append(r)
        r = r.clone()
        r[7] = torch.tensor(448 * 2.0 ** k).bfloat16().float().nextafter(torch.tensor(float("inf"))).item() * 1.01
        rows.append(r)
    t = torch.full((K,), 0.0)
    t[0] = 448.0
    t[1:9] = torch.tensor([1.0625, 1.1875, 17.0, 19.0, -1.0625, 9.5, 0.017578125, 0.005859375])   # halfway cases at 4 significant bits
    rows.append(t)
    sub = torch.full((K,), 2.0 ** -9)                                                             # smallest e4m3 subnormal at scale 1
    sub[0] = 448.0
    sub[1:6] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -8 + 2.0 ** -10, -(2.0 ** -7), 2.0 ** -11])
    rows.append(sub)
    g = torch.Generator().manual_seed(3)
    rows.append(torch.randn(K, generator=g) * 0.02)
    return torch.stack(rows).bfloat16()


def _tiny_core(dtype=torch.bfloat16):
    fx = load_fixture("g1_core_tiny_bf16.pt")
    C, M = pkg("configuration"), pkg("modeling_core")
    cd = fx["cfg"]
    cfg = C.UllavaCoreConfig(vision_config=cd["vision_config"], vision_hidden_layer=-2, mm_token_ids=cd["mm_token_ids"], vocab_size=cd["vocab_size"],
                             hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"], num_hidden_layers=cd["num_hidden_layers"],
                             num_attention_heads=cd["num_attention_heads"])
    return M.UllavaCoreForCausalLM(cfg, dtype=dtype)


def test_quantize_weights_exists():
    M, U = pkg("modeling_core"), pkg("modeling_ullava")
    assert callable(M.UllavaCoreForCausalLM.quantize_weights)
    assert callable(U.UllavaForCausalLM.quantize_weights)
    assert _tiny_core().weight_quantization is None


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_quantize_weights_refuses_non_bf16(dtype):
    model = _tiny_core(dtype)
    with pytest.raises(NotImplementedError, match="bf16"):
        model.quantize_weights("fp8_e4m3")
    assert model.weight_quantization is None


def test_quantize_weights_refuses_lora_adapters():
    model = _tiny_core()
    model.add_lora(r=4)
    with pytest.raises(NotImplementedError, match="merge_lora"):
        model.quantize_weights()
    assert model.weight_quantization is None


def test_quantize_weights_unknown_format():
    with pytest.raises(ValueError):
        _tiny_core().quantize_weights("int4")


def test_scale_rule_restatement_on_edge_rows():
    w = edge_rows()
    codes, scales = fp8_reference(w)
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = torch.log2(scales).round()
    assert torch.equal(torch.pow(2.0, s), scales)                                     # powers of two
    assert scales[0] == 1.0 and int(codes[0].sum()) == 0                             # all-zero row: s = 0
    nz = amax > 0
    assert bool((amax[nz] <= 448.0 * scales[nz]).all())                              # fits
    assert bool((amax[nz] > 224.0 * scales[nz]).all())                               # and s is the smallest that fits
    # rows 1, 3, 5: amax exactly 448 * 2^k -> scale 2^k and the largest code (0x7e) at the max; rows 2, 4, 6: just above -> 2^(k+1)
    for i, k in ((1, -10), (3, 0), (5, 3)):
        assert scales[i] == 2.0 ** k and int(codes[i, 5]) == 0x7E
        assert scales[i + 1] == 2.0 ** (k + 1)
    deq = dequant_reference(codes, scales).float()
    assert bool((deq.abs() <= 448.0 * scales[:, None]).all())
    # ties round to even (4 significant bits); scale 1 on the tie row
    t = deq[7]
    assert scales[7] == 1.0
    assert t[1:9].tolist() == [1.0, 1.25, 16.0, 20.0, -1.0, 10.0, 0.017578125, 0.005859375]
    # e4m3 subnormals at scale 1: multiples of 2^-9, ties to even
    sub = deq[8]
    assert scales[8] == 1.0
    assert sub[1:6].tolist() == [0.0, 2.0 ** -8, 2.0 ** -8, -(2.0 ** -7), 0.0]
    assert float(sub[6]) == 2.0 ** -9
    # the dequantized weight is exact in bf16: the restatement's dequantize equals the fp32 product
    assert torch.equal(deq, codes.view(torch.float8_e4m3fn).float() * scales[:, None])
