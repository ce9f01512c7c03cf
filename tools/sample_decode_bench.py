#!/usr/bin/env python
"""What the SAMPLED decode step costs, host sampler against the on-device sampler against greedy, in ONE process on the same model:
ViT-L/14-336 + LLaMA-7B (random init), a 336 x 336 image + 64-token prompt (S = 643), KV-cached decoding at batch 1, 4 and 16, with bf16
and then fp8 (e4m3) weights.  Sampling settings are the reference callers': temperature 0.2, top_k 50, top_p None and 0.7.

Per configuration: decode ms per token = (generate(--new) - generate(1)) / (--new - 1), eos off so that every run makes every step.  The
modes of one configuration are timed alternately, --reps rounds; the median is printed.  `sampler=None` is timed in three such series of its
own (host#1..#3): it is the code path that existed before the device sampler, and the spread between its three medians is the run-to-run
noise every difference below has to be read against.

    python tools/sample_decode_bench.py [--new 33] [--reps 3] [--batches 1,4,16]
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
ap.add_argument("--reps", type=int, default=3, help="timed rounds per configuration; the median is reported")
ap.add_argument("--batches", default="1,4,16")
a = ap.parse_args()
dev = "cuda:0"
if not torch.cuda.is_available():
    sys.exit("sample_decode_bench needs the GPU (a CPU run measures nothing)")


def one(model, ids, images, n, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(input_ids=ids, images=images, max_new_tokens=n, use_cache=True, eos_token_id=-1, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(v):
    return sorted(v)[len(v) // 2]


model, cfg = bench.build_model(336, dev)
batches = [int(b) for b in a.batches.split(",")]
inputs = {b: bench.make_inputs(cfg, b, 64, dev, b) for b in batches}
print(f"decode ms/token, median of {a.reps} alternating rounds; generate({a.new}) - generate(1) over {a.new - 1} steps; temperature 0.2, top_k 50")
for fmt in ("bf16", "fp8"):
    if fmt == "fp8":
        with torch.no_grad():
            model.quantize_weights("fp8_e4m3")
        torch.cuda.synchronize()
    for b in batches:
        images, ids, _ = inputs[b]
        for top_p in (None, 0.7):
            s = dict(do_sample=True, temperature=0.2, top_k=50, top_p=top_p)
            modes = {"greedy": dict(do_sample=False), "host#1": dict(s, sampler=None), "device": dict(s, sampler="device"),
                     "host#2": dict(s, sampler=None), "host#3": dict(s, sampler=None)}
            t = {m: [] for m in modes}
            with torch.no_grad():
                torch.manual_seed(0)
                for kw in modes.values():                       # warm-up of every mode's kernels and allocations
                    one(model, ids, images, 2, kw)
                for _ in range(a.reps):
                    for m, kw in modes.items():
                        t1 = one(model, ids, images, 1, kw)
                        tn = one(model, ids, images, a.new, kw)
                        t[m].append((tn - t1) / (a.new - 1) * 1e3)
            r = {m: med(v) for m, v in t.items()}
            host = [r["host#1"], r["host#2"], r["host#3"]]
            print(f"weights {fmt:4s} batch {b:2d} top_p {str(top_p):4s}: greedy {r['greedy']:.3f}  device {r['device']:.3f}  host {host[0]:.3f} {host[1]:.3f} "
                  f"{host[2]:.3f} (spread {max(host) - min(host):.3f});  device - greedy {r['device'] - r['greedy']:+.3f} ms, "
                  f"device - host {r['device'] - med(host):+.3f} ms ({(r['device'] / med(host) - 1) * 100:+.1f} %)", flush=True)
