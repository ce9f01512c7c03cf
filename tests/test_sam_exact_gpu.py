"""GPU: the opt-in reference-rounding SAM global attention (ops.sam_global_attention_exact, SamEngine.global_attention = "exact", DESIGN f11)
against the CPU oracle, against closed forms, against itself across batch shapes and strides, and at engine level.  One image, 2 heads of
4096 x 4096 is the workload's own smallest unit (the kernel takes the 64 x 64 grid only)."""
import pytest
import torch
import torch.nn.functional as F

from helpers import pkg, assert_close_bf16
from oracle import ullava_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16 = torch.bfloat16, torch.float16
SIDE, HD = 64, 80
S = SIDE * SIDE
ULP = {BF: 2.0 ** -7, F16: 2.0 ** -10}          # the bound's unit: one ulp is between half of it and all of it, relative to the value


def _rand(*shape, seed=0, scale=1.0, dt=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _share(a, b, dt, ulps=2.0, floor=None):
    """Share of the elements of a beyond ulps * unit * max(|b|, floor) of b (floor: 2 % of max |b|, the rule of helpers.assert_close_bf16)."""
    a_, b_ = a.detach().float().cpu(), b.detach().float().cpu()
    fl = float(b_.abs().max()) * 0.02 if floor is None else floor
    bad = (a_ - b_).abs() > ulps * ULP[dt] * torch.maximum(b_.abs(), torch.full_like(b_, fl))
    return float(bad.float().mean())


def _assert_close_f16(a, b, what, outlier_frac, outlier_floor):
    """helpers.assert_close_bf16 with the bound in fp16 ulps (2 x 2^-10)."""
    sh = _share(a, b, F16)
    print(f"{what}: {sh:.2e} of the elements beyond the tight bound (allowed {outlier_frac:.1e})")
    assert sh <= outlier_frac, f"{what}: share {sh:.3e} beyond the tight bound"
    assert _share(a, b, F16, floor=outlier_floor) == 0.0, f"{what}: elements beyond the bound at the outlier floor"


def _streamed(ops, qkv, rph, rpw, NB, nH, out=None):
    """The default route for the same operands: ops.attention, raw tables, V as rows -> sam_global_kernel."""
    C = nH * HD
    st = (S * 3 * C, HD, 3 * C)
    att = torch.empty(NB * S, C, device=DEV, dtype=qkv.dtype) if out is None else out
    ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], att, NB, nH, S, S, HD, st, st, (S * C, HD, C), None, causal=False, scale_mode=0,
                  q_scale=HD ** -0.5, rel_h=rph, rel_w=rpw, rel_pos_hw=(SIDE, SIDE), v_strides=st)
    return att


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16])
def test_parity_with_the_oracle(dt):
    """The inputs of test_sam_gpu.py::test_sam_encoder_attention for (side 64, hd 80, nH 2, NB 1), seeds 6-10.  Share of the outputs beyond
    the 2-ulp bound against oracle.sam_attention: the fp64-sum restatement of the reference's rounding points (another accumulation order)
    sits at 0 in bf16 and 4.5e-4 in fp16, the streamed form's restatement at 3.9e-3 / 4.5e-3; caps 5e-4 (bf16) and 1.5e-3 (fp16)."""
    ops = pkg("ops")
    nH, NB = 2, 1
    C = nH * HD
    x = _rand(NB, SIDE, SIDE, C, seed=6, dt=dt)
    sd = {"qkv.weight": _rand(3 * C, C, seed=7, scale=C ** -0.5, dt=dt), "qkv.bias": _rand(3 * C, seed=8, scale=0.1, dt=dt),
          "proj.weight": torch.eye(C).to(dt), "proj.bias": torch.zeros(C).to(dt),
          "rel_pos_h": _rand(2 * SIDE - 1, HD, seed=9, scale=0.3, dt=dt), "rel_pos_w": _rand(2 * SIDE - 1, HD, seed=10, scale=0.3, dt=dt)}
    ref = O.sam_attention(sd, "", x, nH).reshape(NB * S, C)           # proj = identity -> the attention output itself
    qkv = F.linear(x.reshape(-1, C), sd["qkv.weight"], sd["qkv.bias"]).to(DEV)
    rph, rpw = sd["rel_pos_h"].to(DEV), sd["rel_pos_w"].to(DEV)
    vmax = float(qkv[:, 2 * C:].float().abs().max())
    new = ops.sam_global_attention_exact(qkv, rph, rpw, NB, nH, SIDE, HD)
    old = _streamed(ops, qkv, rph, rpw, NB, nH)
    cap = 5e-4 if dt == BF else 1.5e-3
    sh_new, sh_old = _share(new, ref, dt), _share(old, ref, dt)
    print(f"{dt}: share beyond 2 ulp of the oracle: exact {sh_new:.3e}, streamed {sh_old:.3e} (cap {cap:.1e})")
    if dt == BF:
        assert_close_bf16(new, ref, ulps=2.0, what="exact sam global attention", outlier_frac=cap, outlier_floor=vmax)
    else:
        _assert_close_f16(new, ref, "exact sam global attention (fp16)", cap, vmax)
    assert sh_old > cap, f"the streamed kernel's share {sh_old:.3e} is not above the cap: the test cannot tell the two forms apart"
    truth = O.sam_attention({k: v.float() for k, v in sd.items()}, "", x.float(), nH).reshape(NB * S, C)
    e_new = float((new.float().cpu() - truth).pow(2).mean().sqrt())
    e_ref = float((ref.float() - truth).pow(2).mean().sqrt())
    print(f"{dt}: rms error vs fp32 truth: exact kernel {e_new:.4g}, reference 16-bit path {e_ref:.4g}")
    assert e_new <= 1.15 * e_ref, f"rms error vs fp32 truth: kernel {e_new:.4g}, reference 16-bit path {e_ref:.4g}"


# ---- 2. closed-form rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16])
def test_closed_form_rows(dt):
    """q = 0: every score is 0, l = 4096 exactly, P = 2^-12 and O = r16(mean of v).  One dominant key (its score more than 100 above every
    other): P is one-hot and O is that V row.  V holds multiples of 1/8 up to 2, so every partial sum of P v is exact in fp32 whatever its
    order, and both rows are compared bit for bit."""
    ops = pkg("ops")
    nH, NB = 2, 1
    C = nH * HD
    g = torch.Generator().manual_seed(21)
    qkv = (0.5 * torch.randn(S, 3 * C, generator=g)).to(dt)
    qkv[:, 2 * C:] = (torch.randint(-16, 17, (S, C), generator=g).float() / 8).to(dt)
    zero_q = [0, 1, 17, 63, 64, 2047, 2100, 4095]                    # first / last rows, both 16-query groups of a wave, several blocks
    for h in range(nH):
        for qi in zero_q:
            qkv[qi, h * HD:(h + 1) * HD] = 0
    hot = {0: (5, 3000), 1: (4090, 7)}                               # head -> (query, its key)
    sign = (torch.randint(0, 2, (HD,), generator=g) * 2 - 1).float()
    for h, (qi, kj) in hot.items():
        qkv[qi, h * HD:(h + 1) * HD] = (16 * sign).to(dt)            # score of key kj: 80 * 256 * 80^-0.5 ~ 2290; any other: |s| < 60
        qkv[kj, C + h * HD:C + (h + 1) * HD] = (16 * sign).to(dt)
    rph = _rand(2 * SIDE - 1, HD, seed=22, scale=0.01, dt=dt)         # |q . rel_pos| stays below 16 * 80 * 0.05 = 64 in the hot rows
    rpw = _rand(2 * SIDE - 1, HD, seed=23, scale=0.01, dt=dt)
    # the margin the closed form needs, checked on the CPU in fp32
    for h, (qi, kj) in hot.items():
        q = qkv[qi, h * HD:(h + 1) * HD].float()
        s = (q * HD ** -0.5) @ qkv[:, C + h * HD:C + (h + 1) * HD].float().T
        bias = q @ O.get_rel_pos(SIDE, SIDE, rph.float())[qi // SIDE].T, q @ O.get_rel_pos(SIDE, SIDE, rpw.float())[qi % SIDE].T
        s = (s.view(SIDE, SIDE) + bias[0][:, None] + bias[1][None, :]).view(-1)
        others = torch.cat([s[:kj], s[kj + 1:]])
        assert float(s[kj] - others.max()) > 120, "the dominant key's margin"
    out = ops.sam_global_attention_exact(qkv.to(DEV), rph.to(DEV), rpw.to(DEV), NB, nH, SIDE, HD).cpu()
    for h in range(nH):
        v = qkv[:, 2 * C + h * HD:2 * C + (h + 1) * HD]
        mean = (v.double().sum(0) / 4096).to(dt)
        for qi in zero_q:
            assert torch.equal(out[qi, h * HD:(h + 1) * HD].view(torch.int16), mean.view(torch.int16)), (h, qi)
        qi, kj = hot[h]
        assert torch.equal(out[qi, h * HD:(h + 1) * HD].view(torch.int16), v[kj].view(torch.int16)), (h, qi, kj)
    assert bool(torch.isfinite(out.float()).all())


# ---- 3. independence of the batch ---------------------------------------------------------------------------------------------------------
def test_heads_do_not_depend_on_the_batch():
    """Nine heads (B 3 x H 3: the second round of 8 XCD slots holds one head) against one-head calls on the same q | k | v: equal bits."""
    ops = pkg("ops")
    NB, nH = 3, 3
    C = nH * HD
    qkv = _rand(NB * S, 3 * C, seed=31, scale=0.5)
    rph, rpw = _rand(2 * SIDE - 1, HD, seed=32, scale=0.3).to(DEV), _rand(2 * SIDE - 1, HD, seed=33, scale=0.3).to(DEV)
    out9 = ops.sam_global_attention_exact(qkv.to(DEV), rph, rpw, NB, nH, SIDE, HD).cpu()
    for i in (0, 7, 8):
        b, h = divmod(i, nH)
        rows = qkv[b * S:(b + 1) * S]
        one = torch.cat([rows[:, j * C + h * HD:j * C + (h + 1) * HD] for j in range(3)], dim=1).contiguous()
        out1 = ops.sam_global_attention_exact(one.to(DEV), rph, rpw, 1, 1, SIDE, HD).cpu()
        assert torch.equal(out9[b * S:(b + 1) * S, h * HD:(h + 1) * HD].contiguous().view(torch.int16), out1.view(torch.int16)), f"head {i}"


# ---- 4. strides ---------------------------------------------------------------------------------------------------------------------------
def test_wider_row_pitches_and_nothing_written_outside_out():
    ops = pkg("ops")
    NB, nH = 1, 2
    C = nH * HD
    qkv = _rand(NB * S, 3 * C, seed=41, scale=0.5).to(DEV)
    rph, rpw = _rand(2 * SIDE - 1, HD, seed=42, scale=0.3).to(DEV), _rand(2 * SIDE - 1, HD, seed=43, scale=0.3).to(DEV)
    want = ops.sam_global_attention_exact(qkv, rph, rpw, NB, nH, SIDE, HD)
    wide = torch.full((NB * S, 3 * C + 8), float("nan"), device=DEV, dtype=BF)
    wide[:, :3 * C] = qkv
    sentinel = -1234.0
    obuf = torch.full((NB * S + 2, C + 16), sentinel, device=DEV, dtype=BF)
    out = obuf[1:-1, 8:8 + C]
    got = ops.sam_global_attention_exact(wide[:, :3 * C], rph, rpw, NB, nH, SIDE, HD, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out.contiguous().view(torch.int16), want.view(torch.int16))
    guard = obuf.clone()
    guard[1:-1, 8:8 + C] = sentinel
    assert bool((guard == sentinel).all()), "something outside `out` was written"
    # what the wrapper refuses: another dtype for out, a shape that is not [B * S, C], a grid without a kernel
    with pytest.raises(RuntimeError):
        ops.sam_global_attention_exact(qkv, rph, rpw, NB, nH, SIDE, HD, out=torch.empty(NB * S, C, device=DEV, dtype=F16))
    with pytest.raises(ValueError):
        ops.sam_global_attention_exact(qkv, rph, rpw, NB, nH, SIDE, HD, out=torch.empty(NB * S, C + 8, device=DEV, dtype=BF))
    with pytest.raises(NotImplementedError, match="48 x 48"):
        ops.sam_global_attention_exact(qkv[:48 * 48], rph, rpw, NB, nH, 48, HD)


# ---- 5. engine level ----------------------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    L = pkg("_lib")
    names = []
    call, query = L.call, L.query

    def spy_call(name, *a):
        names.append(name)
        return call(name, *a)

    def spy_query(name, *a):
        names.append(name)
        return query(name, *a)
    monkeypatch.setattr(L, "call", spy_call)
    monkeypatch.setattr(L, "query", spy_query)
    return names


def test_engine_mode_routes_the_global_blocks(monkeypatch):
    """A two-block encoder at ViT-H width (one window block, one global block, seeded weights as test_sam_gpu.py's full-width encoder) on
    one 1024 x 1024 image."""
    ops, C, Sm, W = pkg("ops"), pkg("configuration"), pkg("sam"), pkg("weights")
    cfg = C.SamConfig(depth=2, global_attn_indexes=[1])
    holder = Sm.build_sam_holder(cfg, device=DEV, dtype=BF)
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items() if k.startswith("image_encoder.")}
    sd = {k: v.to(BF) for k, v in W.seeded_state_dict(shapes, 91, torch.float32).items()}
    assert not holder.load_state_dict(sd, strict=False).unexpected_keys
    eng = Sm.SamEngine(holder, cfg)
    img = torch.randn(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(92)).to(BF).to(DEV)
    names = _spy(monkeypatch)
    entry = "ull_sam_global_attention_exact_bf16"
    assert eng.global_attention == "streamed"
    a = eng.encode(img)
    assert entry not in names and "ull_sam_blocks_bf16" in names
    with ops.per_op_layers():
        b = eng.encode(img)
    assert entry not in names and torch.equal(a, b), "default mode: coarse entry != per-op path"
    del names[:]
    eng.global_attention = "exact"
    c = eng.encode(img)
    assert names.count(entry) == 1 and not any(n.startswith("ull_sam_blocks") for n in names), names
    assert names.count("ull_sam_window_attention_bf16") == 1 and "ull_attention_bf16" not in names
    assert not torch.equal(a, c), "the exact mode changed nothing"
    scfg = dict(patch_size=16, depth=2, global_attn_indexes=[1], window_size=14, num_heads=16)
    torch.set_num_threads(min(64, __import__("os").cpu_count()))
    ref = O.sam_image_encoder({"visual_model." + k: v for k, v in sd.items()}, scfg, img.cpu())
    nchw = lambda t: t.cpu().view(1, 64, 64, 256).permute(0, 3, 1, 2)
    sh_def, sh_exact = _share(nchw(a), ref, BF), _share(nchw(c), ref, BF)
    print(f"encoder output beyond 2 ulp of oracle.sam_image_encoder: default {sh_def:.3e}, exact {sh_exact:.3e}")
    assert sh_exact <= sh_def
    eng.global_attention = "streamed"
    assert torch.equal(eng.encode(img), a), "back to the default: the same bits"


def test_engine_refuses_a_global_block_without_an_exact_kernel():
    """48 x 48 grid (2304 keys > 1024), head dim 80: the exact mode raises."""
    C, Sm = pkg("configuration"), pkg("sam")
    cfg = C.SamConfig(embed_dim=160, depth=1, num_heads=2, global_attn_indexes=[0], img_size=768)
    holder = Sm.build_sam_holder(cfg, device=DEV, dtype=BF)
    g = torch.Generator(device="cuda").manual_seed(51)
    with torch.no_grad():
        for n, p in list(holder.named_parameters()) + list(holder.named_buffers()):
            p.copy_((torch.randn(p.shape, device=DEV, generator=g) * (0.02 if p.dim() > 1 else 0.1)).to(BF))
    eng = Sm.SamEngine(holder, cfg)
    img = torch.randn(1, 3, 768, 768, device=DEV, generator=g).to(BF)
    eng.global_attention = "exact"
    with pytest.raises(NotImplementedError, match="48 x 48 grid with head dim 80"):
        eng.encode(img)
