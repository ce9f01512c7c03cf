"""Shared test plumbing: build the HIP-backed model from a golden fixture and compare with the reference
outputs stored in the fixture and with the CPU oracle.  (Imports `oracle/` -- tests only.)"""
import importlib
import os

import torch

from oracle import ullava_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pkg(sub=""):
    return importlib.import_module("u-llava_amd" + ("." + sub if sub else ""))


def load_fixture(name):
    return torch.load(os.path.join(GOLDEN, name), map_location="cpu", weights_only=True)


def fixture_sd(fx, dtype=None):
    W = pkg("weights")
    dt = dtype or getattr(torch, fx["dtype"].split(".")[-1])
    return {k: v.to(dt) for k, v in W.seeded_state_dict(fx["shapes"], fx["seed"], torch.float32).items()}


def rel_err(a, b):
    """max |a-b| / max |b| in fp32."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def assert_close_bf16(a, b, ulps=2.0, floor=None, what="", outlier_frac=0.0, outlier_floor=None):
    """See below; with `outlier_frac` > 0 that fraction of elements may miss the tight bound as long as ALL elements meet the
    same bound evaluated with `outlier_floor` as the absolute floor (e.g. attention: one bf16 flip of a dominant probability
    p ~ 0.5 moves the output by 2^-9 * max|v| whatever the output's own magnitude)."""
    if outlier_frac > 0.0:
        a_, b_ = a.detach().float().cpu(), b.detach().float().cpu()
        fl = float(b_.abs().max()) * 0.02 if floor is None else floor
        bad = (a_ - b_).abs() > ulps * 2.0 ** -7 * torch.maximum(b_.abs(), torch.full_like(b_, fl))
        print(f"{what}: {float(bad.float().mean()):.2e} of the elements beyond the tight bound (allowed {outlier_frac:.1e})")
        assert float(bad.float().mean()) <= outlier_frac, f"{what}: {int(bad.sum())}/{bad.numel()} elements beyond the tight bound"
        return assert_close_bf16(a, b, ulps, outlier_floor, what)
    """|a-b| <= ulps * 2^-7 * max(|b|, floor).  One bf16 ulp is between 2^-8 and 2^-7 of the value, so `ulps=1` admits a
    single rounding flip anywhere; `floor` (default 2% of max|b|) sets the absolute tolerance for near-zero entries."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    fl = float(b.abs().max()) * 0.02 if floor is None else floor
    tol = ulps * 2.0 ** -7 * torch.maximum(b.abs(), torch.full_like(b, fl))
    bad = (a - b).abs() > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} elements off; max|d|={float((a - b).abs().max()):.4g} " \
                                f"max|ref|={float(b.abs().max()):.4g}"


def core_model_from_fixture(fx, device):
    M = pkg("modeling_core")
    C = pkg("configuration")
    cd = fx["cfg"]
    cfg = C.UllavaCoreConfig(vision_config=cd["vision_config"], vision_hidden_layer=cd["vision_hidden_layer"],
                             projector_type=cd["projector_type"], projector_from_scratch=bool(cd.get("projector_from_scratch", False)),
                             mm_token_ids=cd["mm_token_ids"],
                             vocab_size=cd["vocab_size"], hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"],
                             num_hidden_layers=cd["num_hidden_layers"], num_attention_heads=cd["num_attention_heads"],
                             rms_norm_eps=cd["rms_norm_eps"], rope_theta=cd["rope_theta"])
    model = M.UllavaCoreForCausalLM(cfg, device=device)
    sd = fixture_sd(fx, torch.bfloat16)
    missing = model.load_state_dict(sd, strict=True)
    return model, sd


def run_core_fixture(name, device="cuda:0"):
    """HIP forward on a G1-style fixture -> error statistics (used by smoke() and the gpu tests)."""
    fx = load_fixture(name)
    model, sd = core_model_from_fixture(fx, device)
    ids, mask, images = fx["input_ids"].to(device), fx["attention_mask"].to(device), fx["images"].to(device)
    out = model(input_ids=ids, attention_mask=mask, images=images, output_hidden_states=True)
    torch.cuda.synchronize()
    # fp32 "truth": same bf16-rounded weights/inputs, fp32 arithmetic
    sd32 = {k: v.float() for k, v in sd.items()}
    truth = O.core_forward(sd32, fx["cfg"], fx["input_ids"], fx["attention_mask"], fx["images"].float())
    e_ref = rel_err(fx["logits"], truth["logits"])
    e_hip = rel_err(out.logits, truth["logits"])
    stats = dict(logits_err_vs_ref=rel_err(out.logits, fx["logits"]), ref_err_vs_fp32=e_ref, hip_err_vs_fp32=e_hip,
                 hidden_err_vs_ref=[round(rel_err(h, r), 5) for h, r in zip(out.hidden_states, fx["hidden_states"])],
                 tol=max(1.5 * e_ref, 2.0 ** -6))
    if "greedy_prompt" in fx:
        seq = model.generate(input_ids=fx["greedy_prompt"].to(device), images=images[:1], max_new_tokens=8, do_sample=False)
        stats["greedy_equal"] = bool(torch.equal(seq.cpu(), fx["greedy_sequences"]))
        stats["greedy"] = seq[0, fx["greedy_prompt"].shape[1]:].tolist()
    return stats


def per_op_inputs(seed, dtype):
    """Seeded inputs / weights of the G6 ops (shared with the tests: they regenerate these, the fixture only holds outputs)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dtype)
    return dict(rms_x=r(96, 4096, sc=1.5), rms_w=(torch.randn(4096, generator=g) * 0.1 + 1.0).to(dtype),
                rope_q=r(1, 2, 1024, 128), rope_k=r(1, 2, 1024, 128),
                gate=r(160, 1024, sc=2.0), up=r(160, 1024), act_x=r(160, 1024, sc=2.5),
                px224=r(2, 3, 224, 224), px336=r(1, 3, 336, 336),
                patch_w=r(1024, 3, 14, 14, sc=0.02), cls=r(1024, sc=0.02), pos224=r(257, 1024, sc=0.02), pos336=r(577, 1024, sc=0.02),
                ln_w=(torch.randn(1024, generator=g) * 0.1 + 1.0).to(dtype), ln_b=r(1024, sc=0.1))


def digest_matches(t, d):
    """Does tensor t reproduce a gen_golden._digest record bit for bit?  (sha256 of the raw bytes)"""
    import hashlib
    flat = t.detach().cpu().contiguous().view(-1)
    raw = flat.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().tobytes()
    return tuple(t.shape) == tuple(d["shape"]) and hashlib.sha256(raw).hexdigest() == d["sha256"]


# ---- activation sweeps (tests/test_activation_sweep_{cpu,gpu}.py): float64 references rounded where the reference rounds, and the comparator --
SWEEP_MANT = {torch.bfloat16: 7, torch.float16: 10}               # stored mantissa bits
SWEEP_MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}        # exponent of the smallest normal
SWEEP_FLOOR = {torch.bfloat16: 2.0 ** -100, torch.float16: 2.0 ** -24}
QGELU_SCALE = 1.7020000219345093                                  # float32(1.702): torch multiplies a 16-bit tensor by a Python scalar in fp32


def all_patterns(dt):
    """(values, finite): all 65 536 bit patterns of the 16-bit type in bit order with the non-finite ones replaced by 0, and which were finite
    (65 280 in bf16, 63 488 in fp16)."""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    finite = torch.isfinite(x)
    return torch.where(finite, x, torch.zeros_like(x)), finite


def planted(w):
    """What a one-hot activation row reads out of the weight column w through an fp32 accumulator: w itself, bit for bit, except that -0.0
    arrives as +0.0 (the sum of one -0 and zeros is +0)."""
    return torch.where(w == 0, torch.zeros_like(w), w)


def _rnd32_odd(x64):
    """float64 -> float32 rounded to odd: truncate, and set the last bit where that was inexact.  Rounding this to a 16-bit type (nearest
    even) gives the float64 value rounded ONCE -- a plain float64 -> float32 -> 16-bit cast rounds twice."""
    f = x64.to(torch.float32)
    bits = f.view(torch.int32).clone()
    fin = torch.isfinite(x64)
    inexact = fin & (f.double() != x64)
    bits = torch.where(inexact & (f.double().abs() > x64.abs()), bits - 1, bits)         # back towards zero (also from an overflow to inf)
    return torch.where(inexact, bits | 1, bits).view(torch.float32)


def rnd16(x64, dt):
    """float64 -> dt with a single round-to-nearest-even (overflow gives the infinity, as the casts of the reference do)."""
    return _rnd32_odd(x64).to(dt)


def rnd32_16(x64, dt):
    """float64 -> float32 -> dt, both to nearest even: where the reference rounds the result of an fp32 evaluation on a 16-bit tensor (torch
    computes the activations of a bf16 / fp16 tensor in fp32 and casts).  The fp32 step matters: sigmoid(u) = 1/2 + u/4 - u^3/48 and
    silu(2^-24) = 2^-25 (1 + 2^-26) lie closer to a 16-bit rounding boundary than fp32 resolves for a dozen fp16 inputs, so an fp32
    result -- torch's own included -- is the tie there and goes to even, while the float64 value rounded once goes the other way, and the
    product with the input (or with up = -3) turns that one ulp into two or three."""
    return x64.to(torch.float32).to(dt)


def _sigmoid64(x64):
    return 1.0 / (1.0 + torch.exp(-x64))          # exp overflows to inf in float64 only below -709: 1 / inf = 0, no NaN


def silu_ref(g, dt, rnd=rnd32_16):
    """torch's F.silu on a 16-bit tensor: the fp32 result cast to 16 bits; here from float64."""
    g64 = g.double()
    return rnd(g64 * _sigmoid64(g64), dt)


def swiglu_ref(g, u, dt):
    """LlamaMLP's act_fn(gate) * up on 16-bit tensors: rnd16(rnd16(silu(g)) * u) (the product of two 16-bit values is exact in fp32)."""
    return rnd16(silu_ref(g, dt).double() * u.double(), dt)


def quick_gelu_ref(t, dt, rnd=rnd32_16):
    """transformers' QuickGELUActivation on a 16-bit tensor, input * sigmoid(1.702 * input): three 16-bit roundings.  The scaled input is the
    fp32 product with float32(1.702) cast to 16 bits (that is what the reference computes; its sigmoid is so steep in the negative tail
    that another rounding of its argument would be another function); the last product is exact in fp32."""
    t64 = t.double()
    u = rnd32_16(t64 * QGELU_SCALE, dt)
    s = rnd(_sigmoid64(u.double()), dt)
    return rnd16(t64 * s.double(), dt)


def swiglu_bwd_ref(g, u, da, dt):
    """(d_gate, d_up) of a = silu(g) * u for the incoming da, in float64, each rounded once."""
    g64, u64, d64 = g.double(), u.double(), da.double()
    s = _sigmoid64(g64)
    return rnd16(d64 * u64 * s * (1.0 + g64 * (1.0 - s)), dt), rnd16(d64 * g64 * s, dt)


def ulp16(ref, dt):
    """float64 spacing of the 16-bit type at each |ref| (the subnormal spacing below the smallest normal; inf at inf)."""
    a = ref.double().abs()
    e = torch.frexp(a)[1].double() - 1.0                          # floor(log2 |ref|); frexp(0) = (0, 0)
    e = torch.where(a == 0, torch.full_like(e, SWEEP_MIN_EXP[dt]), torch.clamp(e, min=float(SWEEP_MIN_EXP[dt])))
    return torch.where(torch.isfinite(a), torch.pow(torch.tensor(2.0, dtype=torch.float64), e - SWEEP_MANT[dt]), a)


def sweep_compare(got, ref, dt, cap, what, valid=None):
    """The sweep's comparator over the elements where `valid` (default: all): (a) no NaN, (b) a non-finite reference value is matched exactly,
    (c) |got - ref| <= max(one 16-bit ulp of ref, SWEEP_FLOOR), (d) at most `cap` elements differ from ref bitwise (None: not capped).  Returns that count."""
    got, ref = got.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    assert got.dtype == dt and ref.dtype == dt and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    if valid is not None:
        valid = valid.detach().cpu().reshape(-1)
        got, ref = got[valid], ref[valid]
    assert not bool(torch.isnan(ref).any()), f"{what}: the reference itself has NaN"
    g64, r64 = got.double(), ref.double()
    nan = torch.isnan(got)
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} NaN outputs of {got.numel()}, first at element {int(nan.nonzero()[0])} (reference {float(r64[nan][0])})"
    inf = torch.isinf(ref)
    assert bool((g64[inf] == r64[inf]).all()), f"{what}: {int((g64[inf] != r64[inf]).sum())} infinities of the reference not matched"
    err = (g64 - r64).abs()[~inf]
    tol = torch.clamp(ulp16(ref, dt)[~inf], min=SWEEP_FLOOR[dt])
    bad = err > tol
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} beyond one ulp; first: got {float(g64[~inf][i])!r}, reference {float(r64[~inf][i])!r}")
    ndiff = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
    print(f"[act-sweep] {what}: {ndiff} of {got.numel()} differ bitwise from the reference (cap {cap})")
    assert cap is None or ndiff <= cap, f"{what}: {ndiff} of {got.numel()} differ bitwise from the reference, cap {cap}"
    return ndiff
