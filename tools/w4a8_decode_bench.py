#!/usr/bin/env python
"""MXFP8 activations in batched decode steps on mxfp4 weights (quantize_weights("mxfp4", decode_activations="mxfp8_e4m3"), DESIGN f20) against
the routes the parent takes, in ONE process on the same random-init LLaMA-7B weights (bench.build_model) -- the mxfp4 sibling of
tools/a8_decode_bench.py.  Arms, interleaved round by round:

    bf16          the bf16 model
    w4a16         quantize_weights("mxfp4") (W4A16 skinny kernel at 5 .. 16 rows, dequantize + bf16 GEMM from 17 rows on)
    w4a8          ... activations="mxfp8_e4m3" (W4A16 skinny kernel at 5 .. 16 rows, the 128 x 128 W4A8 GEMM from 17 rows on)
    w4a8+decode   ... decode_activations="mxfp8_e4m3" (ops.linear_w4a8_skinny at 5 .. 32 rows)
    fp8 a8+decode quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="prefill+decode"): the cross-format yardstick

Measured: one whole decode step (embedding, 32 layers, final norm, lm_head) from a KV cache holding 643 positions at batch 4 (control:
the fused-append GEMV steps, untouched), 8, 16 and 32; and per launch at M = 8 / 16 / 32 the four LLaMA-layer Linears on the parent's route
and the new one, each as TB/s of code + scale bytes beside the mxfp4 GEMV (M = 1) on the same weights in the same loop, plus the row
quantizer, the norm and the fused norm + quantize.  The per-launch loops rotate over weight copies of more than 512 MB in total so that no
launch finds its weight in a cache.  Times are device-event medians over --reps rounds after --warmup rounds, with min and max.  Also,
ungated: greedy-token agreement with the W4A16 model over 32 steps at batch 8 on the bench prompt.

    python tools/w4a8_decode_bench.py [--reps 7] [--warmup 2] > profiles/w4a8_decode.txt
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
    sys.exit("w4a8_decode_bench: needs the GPU (nothing is measured without one)")
dev = torch.device("cuda:0")
ops = importlib.import_module("u-llava_amd.ops")
BF = torch.bfloat16
NEW = "mxfp8_e4m3"


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


def random_mxfp4(N, K, g):
    """An Mxfp4Weight of random codes (every e2m1 nibble is finite) and block scales 2^-7 .. 2^-10: timing only."""
    codes = torch.randint(0, 256, (N, K // 2), device=dev, generator=g, dtype=torch.uint8)
    scales = torch.randint(117, 121, (N, ops.Mxfp4Weight.scale_pitch(K)), device=dev, generator=g, dtype=torch.uint8)
    return ops.Mxfp4Weight(codes, scales, K)


def layer_launches(M):
    D, I = 4096, 11008
    g = torch.Generator(device="cuda").manual_seed(M)
    print(f"-- LLaMA-layer launches at M = {M} rows; per launch, rotating over weight copies of > 512 MB; TB/s = weight code + scale bytes / time")
    for name, N, K, kw in (("q|k|v", 3 * D, D, {}), ("o_proj + residual", D, D, dict(residual=True)),
                           ("gate|up + SwiGLU", 2 * I, D, dict(swiglu=True)), ("down_proj + residual", D, I, dict(residual=True))):
        n = -(-(1 << 29) // (N * K // 2 + N * K // 32)) + 1
        qs = [random_mxfp4(N, K, g) for _ in range(n)]
        x = torch.randn(M, K, device=dev, generator=g).to(BF)
        x1 = x[:1].contiguous()
        xq, xsc = ops._quantize_rows_mxfp8(x, K)
        args = dict(swiglu=True) if kw.get("swiglu") else {}
        args1 = dict(args)
        if kw.get("residual"):
            args["residual"] = torch.randn(M, N, device=dev, generator=g).to(BF)
            args1["residual"] = args["residual"][:1].contiguous()
        out = torch.empty(M, N // 2 if kw.get("swiglu") else N, device=dev, dtype=BF)
        out1 = torch.empty(1, out.shape[1], device=dev, dtype=BF)
        parent = (lambda q: ops.linear(x, q, out=out, **args)) if M <= 16 else (lambda q: ops.linear_w4a8(x, q, out=out, **args))
        pname = "W4A16 skinny kernel" if M <= 16 else "128 x 128 W4A8 GEMM incl. its row quantization"

        def loop(f):
            def run():
                for q in qs:
                    f(q)
            return run
        with torch.no_grad():
            r = timed({"gemv": loop(lambda q: ops.linear(x1, q, out=out1, **args1)), "parent": loop(parent),
                       "new": loop(lambda q: ops.linear_w4a8_skinny(xq, xsc, q, out=out, **args))}, a.reps, a.warmup)
        gb = (N * K // 2 + N * K // 32) / 1e9
        stream = gb / (r["gemv"][0] / n * 1e3) * 1e3
        print(f"{name:22s} [{M} x {K}] @ [{N} x {K}]^T, {n} copies")
        for k, what in (("gemv", "the mxfp4 GEMV stream: M = 1 on the same weights"), ("parent", pname), ("new", "W4A8 skinny kernel (codes in)")):
            us = r[k][0] / n * 1e3
            print(f"    {k:6s} {fmt(r[k], n / 1e3, 'us')}  {gb / us * 1e3:5.2f} TB/s = {gb / us * 1e3 / stream * 100:5.1f} % of the stream   {what}")
        print(f"    new / parent = {r['new'][0] / r['parent'][0]:.3f};  spread of the parent's arm (max - min) / median = "
              f"{(r['parent'][2] - r['parent'][1]) / r['parent'][0]:.3f}")
        del qs, out, args, x, xq, xsc
        torch.cuda.empty_cache()
    for K in (D, I):
        x = torch.randn(M, K, device=dev, generator=g).to(BF)
        w = torch.ones(K, device=dev, dtype=BF)
        n = 16
        fns = {"quantize_rows_mxfp8": lambda: [ops._quantize_rows_mxfp8(x, K) for _ in range(n)]}
        if K == D:
            fns["rmsnorm"] = lambda: [ops.rmsnorm(x, w, 1e-6) for _ in range(n)]
            fns["rmsnorm_quantize_rows_mxfp8"] = lambda: [ops.rmsnorm_quantize_rows_mxfp8(x, w, 1e-6) for _ in range(n)]
        with torch.no_grad():
            r = timed(fns, a.reps, a.warmup)
        for k, t in r.items():
            print(f"    {k + f' [{M} x {K}]':40s} {fmt(t, n / 1e3, 'us')}  (incl. the output allocations)")


def _mode(m, act, dec):
    m.activation_quantization, m.decode_activation_quantization = act, dec


def decode_steps(m16, m4, m8, B):
    g = torch.Generator(device="cuda").manual_seed(B)
    prompt = torch.randint(5, 32000, (B, a.past), device=dev, generator=g)
    tok = torch.randint(5, 32000, (B, 1), device=dev, generator=g)
    with torch.no_grad():
        caches = {id(m): m(input_ids=prompt, use_cache=True).past_key_values for m in (m16, m4, m8)}

    def arm(m, act, dec):
        cache = caches[id(m)]

        def f():
            if m is m4:
                _mode(m, act, dec)
            with torch.no_grad():
                m(input_ids=tok, past_key_values=cache, use_cache=True)
            cache.length = a.past                  # the next timed step rewrites the same position
            del cache.last_hidden[1:]
        return f
    r = timed({"bf16": arm(m16, None, None), "w4a16": arm(m4, None, None), "w4a8": arm(m4, NEW, None), "w4a8+decode": arm(m4, None, NEW),
               "fp8 a8+decode": arm(m8, None, None)}, a.reps, a.warmup + 1)
    _mode(m4, None, None)
    print(f"-- decode step at batch {B} from a cache of {a.past} positions")
    for k in r:
        print(f"    {k:14s} {fmt(r[k])}")
    new = r["w4a8+decode"][0]
    print(f"    w4a8+decode / w4a16 = {new / r['w4a16'][0]:.3f} (spread of that parent arm (max - min) / median = "
          f"{(r['w4a16'][2] - r['w4a16'][1]) / r['w4a16'][0]:.3f});  w4a8+decode / w4a8 = {new / r['w4a8'][0]:.3f} (spread "
          f"{(r['w4a8'][2] - r['w4a8'][1]) / r['w4a8'][0]:.3f});  w4a8+decode / fp8 a8+decode = {new / r['fp8 a8+decode'][0]:.3f}")
    del caches
    torch.cuda.empty_cache()


def agreement(m4, cfg):
    images, ids, _ = bench.make_inputs(cfg, 8, 64, dev, 8)
    kw = dict(input_ids=ids, images=images, max_new_tokens=32, do_sample=False, use_cache=True, eos_token_id=-1)
    outs = {}
    with torch.no_grad():
        for name, act, dec in (("w4a16", None, None), ("w4a8", NEW, None), ("w4a16+decode", None, NEW), ("w4a8+decode", NEW, NEW)):
            _mode(m4, act, dec)
            outs[name] = m4.generate(**kw)[:, ids.shape[1]:]
    _mode(m4, None, None)
    print("-- greedy-token agreement with the W4A16 model, batch 8 x 32 new tokens on the bench prompt (336 x 336 image + 64 tokens), random-init "
          "weights (their logit margins are far smaller than a trained model's); ungated")
    for name in ("w4a8", "w4a16+decode", "w4a8+decode"):
        same = (outs[name] == outs["w4a16"])
        first = [int((~row).nonzero()[0]) if not bool(row.all()) else 32 for row in same]
        print(f"    {name:13s} {float(same.float().mean()) * 100:6.2f} % of {same.numel()} tokens; first differing step per row: {first}")
    print("    (task accuracy on real checkpoints is unmeasured)")


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; times from device events, arms interleaved per round")
if not a.skip_launches:
    for M in (8, 16, 32):
        layer_launches(M)
if not a.skip_steps:
    m16, cfg = bench.build_model(336, dev)
    m4, _ = bench.build_model(336, dev)                    # the same seed: the same weights
    m8, _ = bench.build_model(336, dev)
    with torch.no_grad():
        m4.quantize_weights("mxfp4")
        m8.quantize_weights("fp8_e4m3", activations="fp8_e4m3", activation_scope="prefill+decode")
    for B in (4, 8, 16, 32):
        decode_steps(m16, m4, m8, B)
    del m16, m8
    torch.cuda.empty_cache()
    agreement(m4, cfg)
