#!/usr/bin/env python
"""FP8 (e4m3) KV cache against the bf16 cache, in ONE process on the same model: ViT-L/14-336 + LLaMA-7B (random init), a 336 x 336 image +
64-token prompt (S = 643), KV-cached greedy decoding at batch 1, 4, 16 and 32, with bf16 weights and then with quantize_weights("fp8_e4m3").
Prints per (weights, cache, batch): prefill + first token, ms per decode step, tokens/s and the resident bytes of the cache generate()
allocates (S + --new + 1 positions, rounded up to 64).

    python tools/kv8_decode_bench.py [--new 33] [--reps 3] [--batches 1,4,16,32] [--weights bf16,fp8] [--caches bf16,fp8]

For a kernel trace of one configuration (`rocprofv3 --kernel-trace --stats -- python tools/kv8_decode_bench.py --batches 1 --weights bf16
--caches fp8 --reps 1`), pick a single batch / weight format / cache format.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--new", type=int, default=33, help="tokens generated in the timed run (the first one is the prefill's)")
ap.add_argument("--reps", type=int, default=3, help="timed runs per configuration; the median is reported")
ap.add_argument("--batches", default="1,4,16,32")
ap.add_argument("--weights", default="bf16,fp8")
ap.add_argument("--caches", default="bf16,fp8")
a = ap.parse_args()
dev = "cuda:0"
batches = [int(b) for b in a.batches.split(",")]
caches = {"bf16": None, "fp8": "fp8_e4m3"}


def time_decode(model, ids, images, kv):
    """(prefill + 1 token in ms, ms per decode step): median over --reps of generate(1) and generate(--new)."""
    kw = dict(input_ids=ids, images=images, do_sample=False, use_cache=True, eos_token_id=-1, kv_cache_dtype=kv)
    pre, step = [], []
    with torch.no_grad():
        model.generate(max_new_tokens=2, **kw)                                   # warm-up
        for _ in range(a.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.generate(max_new_tokens=1, **kw)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            model.generate(max_new_tokens=a.new, **kw)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            pre.append(t1 - t0)
            step.append(((t2 - t1) - (t1 - t0)) / (a.new - 1))
    return sorted(pre)[len(pre) // 2] * 1e3, sorted(step)[len(step) // 2] * 1e3


def cache_bytes(model, B, S, kv):
    from importlib import import_module
    MC = import_module("u-llava_amd.modeling_core")
    c = model.config
    cache = MC.KVCache(c.num_hidden_layers, B, c.num_attention_heads, c.hidden_size // c.num_attention_heads, S + a.new + 1, dev, kv_dtype=kv)
    n = cache.nbytes()
    del cache
    return n


model, cfg = bench.build_model(336, dev)
inputs = {b: bench.make_inputs(cfg, b, 64, dev, b) for b in batches}
with torch.no_grad():
    S = model(input_ids=inputs[batches[0]][1][:1], images=inputs[batches[0]][0][:1], use_cache=True).past_key_values.length
res = {}
for w in a.weights.split(","):
    if w == "fp8":
        with torch.no_grad():
            model.quantize_weights("fp8_e4m3")
        torch.cuda.synchronize()
    for b in batches:
        images, ids, _ = inputs[b]
        for c in a.caches.split(","):
            res[(w, c, b)] = time_decode(model, ids, images, caches[c])
            torch.cuda.empty_cache()

print(f"prompt length S = {S} positions (336 x 336 image + 64 text tokens); cache of generate(--new {a.new}): S + {a.new + 1} positions")
for w in a.weights.split(","):
    for b in batches:
        for c in a.caches.split(","):
            pre, st = res[(w, c, b)]
            print(f"weights {w:4s} cache {c:4s} batch {b:2d}: prefill + 1 token {pre:8.2f} ms; decode {st:7.3f} ms/step = {b / st * 1e3:8.1f} "
                  f"tokens/s; cache {cache_bytes(model, b, S, caches[c]) / 2**30:6.3f} GiB")
    if "bf16" in a.caches and "fp8" in a.caches:
        for b in batches:
            r8, r16 = res[(w, "fp8", b)], res[(w, "bf16", b)]
            print(f"weights {w:4s} batch {b:2d}: fp8 / bf16 cache: decode {r8[1] / r16[1]:.3f}x, prefill + 1 token {r8[0] / r16[0]:.3f}x")
