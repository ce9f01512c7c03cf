"""A/B of two builds of the SAM global attention (64 x 64 grid, 4096 keys, decomposed rel-pos, V as rows: attn_stream_kernel) at the RES
shape (8 images, 16 heads, hd 80): the first run dumps its output, later runs compare with that dump.
usage: ULL_LIB_PATH=<other libullava_hip.so> python tools/global_attn_ab.py <dump.pt>;  python tools/global_attn_ab.py <dump.pt>
       python tools/global_attn_ab.py --three-forms [out.txt]: one process, B = 8, H = 16, the same operands through the three forms of this
       attention -- streamed (sam_global_kernel, the default), exact (sam_global_exact_kernel, SamEngine.global_attention = "exact") and the
       generic exact route (attn_long_kernel: per-query bias tables from sam_relpos, a V^T image and an all-ones key mask make the call a
       run-time-flag one, which ends in launch_long) -- arms interleaved, device events, median / min / max of 7 rounds of 4 calls."""
import importlib, sys, os, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ops = importlib.import_module("u-llava_amd.ops")
dev = "cuda"
nH, side, hd = 16, 64, 80
S, C = side * side, nH * hd


def three_forms(out_path):
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)
    for dt in (torch.bfloat16, torch.float16):
        NB = 8
        gen = torch.Generator().manual_seed(NB)
        qkv = (0.5 * torch.randn(NB * S, 3 * C, generator=gen)).to(dt).to(dev)
        rph = (0.3 * torch.randn(2 * side - 1, hd, generator=gen)).to(dt).to(dev)
        rpw = (0.3 * torch.randn(2 * side - 1, hd, generator=gen)).to(dt).to(dev)
        st = (S * 3 * C, hd, 3 * C)
        o = [torch.empty(NB * S, C, device=dev, dtype=dt) for _ in range(3)]
        rel_h, rel_w = ops.sam_relpos(qkv, st, rph, rpw, NB, nH, side, side, hd)
        vt = ops.transpose_v(qkv[:, 2 * C:], S * 3 * C, 3 * C, NB, S, nH, hd)
        ones = torch.ones(NB, S, device=dev, dtype=torch.int32)
        arms = [
            ("streamed (sam_global_kernel)", lambda: ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], o[0], NB, nH, S, S, hd, st, st, (S * C, hd, C), None,
                                                                   causal=False, scale_mode=0, q_scale=hd ** -0.5, rel_h=rph, rel_w=rpw,
                                                                   rel_pos_hw=(side, side), v_strides=st)),
            ("exact (sam_global_exact_kernel)", lambda: ops.sam_global_attention_exact(qkv, rph, rpw, NB, nH, side, hd, out=o[1])),
            ("generic exact route (attn_long_kernel)", lambda: ops.attention(qkv, qkv[:, C:], vt, o[2], NB, nH, S, S, hd, st, st, (S * C, hd, C), ones,
                                                                            causal=False, scale_mode=0, q_scale=hd ** -0.5, rel_h=rel_h, rel_w=rel_w)),
        ]
        for _, fn in arms:                                    # warm-up: code objects, attribute calls
            fn(); fn()
        torch.cuda.synchronize()
        ts = [[] for _ in arms]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rnd in range(7):
            for i, (_, fn) in enumerate(arms):
                e0.record()
                for _ in range(4):
                    fn()
                e1.record(); torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1) / 4 * 1e3)
        say(f"{str(dt)[6:]}  B = {NB}, H = {nH}, 4096 x 4096, hd 80: us per call, median [min .. max] of 7 interleaved rounds of 4 calls")
        med = [sorted(t)[3] for t in ts]
        for (name, _), t, m in zip(arms, ts, med):
            say(f"   {name:42s} {m:8.1f}  [{min(t):8.1f} .. {max(t):8.1f}]   {m / med[0]:5.2f} x streamed")
        d = [(o[1].float() - o[j].float()).abs() for j in (0, 2)]
        say(f"   exact vs streamed: {float((d[0] > 0).float().mean()):.4f} of the outputs differ (max |d| {float(d[0].max()):.3g}); exact vs generic exact route: "
            f"{float((d[1] > 0).float().mean()):.2e} differ (max |d| {float(d[1].max()):.3g}; fp32 summation order only)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "--three-forms":
    three_forms(sys.argv[2] if len(sys.argv) > 2 else None)
    sys.exit(0)
outs = {}
CASES = ((8, torch.bfloat16), (1, torch.bfloat16), (8, torch.float16))
if os.environ.get('ONLY_FIRST'):
    CASES = CASES[:1]
for (NB, dt) in CASES:
    gen = torch.Generator().manual_seed(NB)
    qkv = (0.5 * torch.randn(NB * S, 3 * C, generator=gen)).to(dt).to(dev)
    rph = (0.3 * torch.randn(2 * side - 1, hd, generator=gen)).to(dt).to(dev)
    rpw = (0.3 * torch.randn(2 * side - 1, hd, generator=gen)).to(dt).to(dev)
    strides = (S * 3 * C, hd, 3 * C)
    att = torch.empty(NB * S, C, device=dev, dtype=dt)
    fn = lambda: ops.attention(qkv, qkv[:, C:], qkv[:, 2 * C:], att, NB, nH, S, S, hd, strides, strides, (S * C, hd, C), None, causal=False,
                               scale_mode=0, q_scale=hd ** -0.5, rel_h=rph, rel_w=rpw, rel_pos_hw=(side, side), v_strides=strides)
    fn(); torch.cuda.synchronize()
    outs[(NB, str(dt))] = att.cpu().clone()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for rep in range(3):
        torch.cuda.synchronize(); e0.record()
        for _ in range(10):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 10 * 1e3)
    print(f"{os.path.basename(os.environ.get('ULL_LIB_PATH', 'libullava_hip.so'))}  {str(dt)[6:]} NB={NB}: " + " ".join(f"{t:.1f}" for t in ts) + " us", flush=True)
path = sys.argv[1]
if os.path.exists(path):
    ref = torch.load(path)
    for k, o in outs.items():
        same = torch.equal(o.view(torch.int16), ref[k].view(torch.int16))
        print(f"   {k}: bit-identical to the first run: {same}  (max |diff| {(o.float() - ref[k].float()).abs().max().item():.3g}, finite {bool(torch.isfinite(o.float()).all())})")
else:
    torch.save(outs, path)
