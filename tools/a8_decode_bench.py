#!/usr/bin/env python
"""FP8 activations in batched decode steps (quantize_weights(..., activation_scope="prefill+decode"), DESIGN f10) against the routes the
parent takes, in ONE process on the same random-init LLaMA-7B weights (bench.build_model).  Arms, interleaved round by round:

    bf16       the bf16 model
    w8a16      quantize_weights("fp8_e4m3")
    a8         ... activations="fp8_e4m3" (scope "prefill": W8A16 skinny kernel at 5 .. 16 rows, the 128 x 128 W8A8 GEMM from 17 rows on)
    a8+decode  ... activation_scope="prefill+decode" (ops.linear_a8w8_skinny at 5 .. 32 rows)

Measured: one whole decode step (embedding, 32 layers, final norm, lm_head) from a KV cache holding 643 positions at batch 4 (control:
the fused-append GEMV steps, untouched), 8, 16 and 32; and per launch at M = 8 / 16 / 32 the four LLaMA-layer Linears on the parent's route
and the new one, each as TB/s of weight bytes, plus the two row-quantization launches and the fused norm + quantize.  The per-launch loops
rotate over weight copies of more than 512 MB in total so that no launch finds its weight in a cache.  Times are device-event medians over
--reps rounds after --warmup rounds, with min and max.  Also, ungated: greedy-token agreement with the W8A16 model over 32 steps at batch 8
on the bench prompt.

    python tools/a8_decode_bench.py [--reps 7] [--warmup 2] > profiles/a8_decode.txt
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--past", type=int, default=643, help="positions in the KV cache before the timed step")
ap.add_argument("--skip-launches", action="store_true")
ap.add_argument("--skip-steps", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("a8_decode_bench: needs the GPU (nothing is measured without one)")
dev = torch.device("cuda:0")
ops = importlib.import_module("u-llava_amd.ops")
BF = torch.bfloat16
STREAM = 4.65                  # TB/s the fp8 GEMV stream reaches (profiles/fp8_decode.txt)


def timed(fns, reps, warmup):
    """{name: (median, min, max) ms} of the callables in `fns`, run interleaved: one call of each per round."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def fmt(t, div=1.0, unit="ms"):
    return f"{t[0] / div:8.3f} {unit} (min {t[1] / div:.3f}, max {t[2] / div:.3f})"


def random_fp8(N, K, g):
    """An Fp8Weight of random finite codes (|code| < 0x78) and scales 2^-7 .. 2^-9: timing only."""
    codes = torch.randint(0, 0x78, (N, K), device=dev, generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (N, K), device=dev, generator=g,
                                                                                                       dtype=torch.uint8) << 7)
    return ops.Fp8Weight(codes, torch.pow(2.0, -7.0 - torch.arange(N, device=dev) % 3).float())


def layer_launches(M):
    D, I = 4096, 11008
    g = torch.Generator(device="cuda").manual_seed(M)
    print(f"-- LLaMA-layer launches at M = {M} rows; per launch, rotating over weight copies of > 512 MB; TB/s = weight code bytes / time "
          f"(the fp8 GEMV stream: {STREAM} TB/s)")
    for name, N, K, kw in (("q|k|v", 3 * D, D, {}), ("o_proj + residual", D, D, dict(residual=True)),
                           ("gate|up + SwiGLU", 2 * I, D, dict(swiglu=True)), ("down_proj + residual", D, I, dict(residual=True))):
        n = -(-(1 << 29) // (N * K)) + 1
        qs = [random_fp8(N, K, g) for _ in range(n)]
        x = torch.randn(M, K, device=dev, generator=g).to(BF)
        xq, xs = ops.quantize_rows_fp8(x)
        args = dict(swiglu=True) if kw.get("swiglu") else {}
        if kw.get("residual"):
            args["residual"] = torch.randn(M, N, device=dev, generator=g).to(BF)
        out = torch.empty(M, N // 2 if kw.get("swiglu") else N, device=dev, dtype=BF)
        parent = (lambda q: ops.linear(x, q, out=out, **args)) if M <= 16 else (lambda q: ops.linear_a8w8(x, q, out=out, **args))
        pname = "W8A16 skinny kernel" if M <= 16 else "128 x 128 W8A8 GEMM incl. its row quantization"

        def loop(f):
            def run():
                for q in qs:
                    f(q)
            return run
        with torch.no_grad():
            r = timed({"parent": loop(parent), "new": loop(lambda q: ops.linear_a8w8_skinny(xq, xs, q, out=out, **args))}, a.reps, a.warmup)
        gb = N * K / 1e9
        print(f"{name:22s} [{M} x {K}] @ [{N} x {K}]^T, {n} copies")
        for k, what in (("parent", pname), ("new", "W8A8 skinny kernel (codes in)")):
            us = r[k][0] / n * 1e3
            print(f"    {k:6s} {fmt(r[k], n / 1e3, 'us')}  {gb / us * 1e3:5.2f} TB/s = {gb / us * 1e3 / STREAM * 100:5.1f} % of the stream   {what}")
        print(f"    new / parent = {r['new'][0] / r['parent'][0]:.3f}")
        del qs, out, args, x, xq, xs
        torch.cuda.empty_cache()
    for K in (D, I):
        x = torch.randn(M, K, device=dev, generator=g).to(BF)
        w = torch.ones(K, device=dev, dtype=BF)
        n = 16
        fns = {"quantize_rows_fp8": lambda: [ops.quantize_rows_fp8(x) for _ in range(n)]}
        if K == D:
            fns["rmsnorm"] = lambda: [ops.rmsnorm(x, w, 1e-6) for _ in range(n)]
            fns["rmsnorm_quantize_rows_fp8"] = lambda: [ops.rmsnorm_quantize_rows_fp8(x, w, 1e-6) for _ in range(n)]
        with torch.no_grad():
            r = timed(fns, a.reps, a.warmup)
        for k, t in r.items():
            print(f"    {k + f' [{M} x {K}]':40s} {fmt(t, n / 1e3, 'us')}  (incl. the output allocations)")


def decode_steps(m16, m8, B):
    g = torch.Generator(device="cuda").manual_seed(B)
    prompt = torch.randint(5, 32000, (B, a.past), device=dev, generator=g)
    tok = torch.randint(5, 32000, (B, 1), device=dev, generator=g)
    with torch.no_grad():
        caches = {id(m): m(input_ids=prompt, use_cache=True).past_key_values for m in (m16, m8)}

    def arm(m, act, scope):
        cache = caches[id(m)]

        def f():
            m.activation_quantization, m.activation_scope = act, scope
            with torch.no_grad():
                m(input_ids=tok, past_key_values=cache, use_cache=True)
            cache.length = a.past                  # the next timed step rewrites the same position
            del cache.last_hidden[1:]
        return f
    r = timed({"bf16": arm(m16, None, "prefill"), "w8a16": arm(m8, None, "prefill"), "a8": arm(m8, "fp8_e4m3", "prefill"),
               "a8+decode": arm(m8, "fp8_e4m3", "prefill+decode")}, a.reps, a.warmup + 1)
    m8.activation_quantization, m8.activation_scope = None, "prefill"
    print(f"-- decode step at batch {B} from a cache of {a.past} positions")
    for k in r:
        print(f"    {k:10s} {fmt(r[k])}")
    print(f"    a8+decode / a8 (the parent's behaviour) = {r['a8+decode'][0] / r['a8'][0]:.3f};  a8+decode / w8a16 = "
          f"{r['a8+decode'][0] / r['w8a16'][0]:.3f};  spread of the parent's arm (max - min) / median = "
          f"{(r['a8'][2] - r['a8'][1]) / r['a8'][0]:.3f}")
    del caches
    torch.cuda.empty_cache()


def agreement(m8, cfg):
    images, ids, _ = bench.make_inputs(cfg, 8, 64, dev, 8)
    kw = dict(input_ids=ids, images=images, max_new_tokens=32, do_sample=False, use_cache=True, eos_token_id=-1)
    outs = {}
    with torch.no_grad():
        for name, act, scope in (("w8a16", None, "prefill"), ("a8", "fp8_e4m3", "prefill"), ("a8+decode", "fp8_e4m3", "prefill+decode")):
            m8.activation_quantization, m8.activation_scope = act, scope
            outs[name] = m8.generate(**kw)[:, ids.shape[1]:]
    m8.activation_quantization, m8.activation_scope = None, "prefill"
    print("-- greedy-token agreement with the W8A16 model, batch 8 x 32 new tokens on the bench prompt (336 x 336 image + 64 tokens), random-init "
          "weights (their logit margins are far smaller than a trained model's); ungated")
    for name in ("a8", "a8+decode"):
        same = (outs[name] == outs["w8a16"])
        first = [int((~row).nonzero()[0]) if not bool(row.all()) else 32 for row in same]
        print(f"    {name:10s} {float(same.float().mean()) * 100:6.2f} % of {same.numel()} tokens; first differing step per row: {first}")
    print("    (task accuracy on real checkpoints is unmeasured)")


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; times from device events, arms interleaved per round")
if not a.skip_launches:
    for M in (8, 16, 32):
        layer_launches(M)
if not a.skip_steps:
    m16, cfg = bench.build_model(336, dev)
    m8, _ = bench.build_model(336, dev)                    # the same seed: the same weights
    with torch.no_grad():
        m8.quantize_weights("fp8_e4m3")
    for B in (4, 8, 16, 32):
        decode_steps(m16, m8, B)
    del m16
    torch.cuda.empty_cache()
    agreement(m8, cfg)
