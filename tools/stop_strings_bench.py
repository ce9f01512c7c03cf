#!/usr/bin/env python
"""Stop strings on the device (generate(stop_strings=, tokenizer=), DESIGN f18): what a token costs with no criterion, with the reference
callers' KeywordsStoppingCriteria on the host, and with the on-device stop, in ONE process on random-init LLaMA-7B weights (bench.build_model),
bf16, on the bench prompt (S = 643): batch 1 and 16, 64 and 512 new tokens, greedy and sampler="device", eos_token_id=-1.

The stop string is one no run ever spells ("§§never§§": its bytes could only come from byte-fallback tokens drawn in exactly that order), so
every run goes to max_new_tokens -- asserted.  The tokenizer is the LLaMA-shaped one of tests/stop_tokenizer.py, built in-process with a
vocabulary of the model's size; only its byte table and its decode are exercised.  Arms, interleaved per round:
  (a)  no criterion                                   (a2) the same again: the run-to-run spread of (a) in this process
  (b)  stopping_criteria=[KeywordsStoppingCriteria]   the status quo: a host read per step and a decode of all generated tokens of row 0
  (c)  stop_strings=[...], tokenizer=...              one more launch per step, the host looks every 8 steps
Times are wall clock between synchronizes around whole generate() calls (they read the host themselves), medians over --reps rounds after
--warmup rounds, per token (prefill included in every arm alike).

  --plain   arm (a) alone, with no new option: runs on a checkout of the parent commit too, for the flag-off comparison.

    python tools/stop_strings_bench.py [--reps 5] [--warmup 1] > profiles/stop_strings_decode.txt
"""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--plain", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("stop_strings_bench: needs the GPU (nothing is measured without one)")
dev = torch.device("cuda:0")
STOP = "§§never§§"


def wall(fns, reps, warmup):
    """{name: (median, min, max) ms} of whole generate() calls, one call of each arm per round: wall clock between synchronizes."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


def per_token(t, n):
    return f"{t[0] / n:7.4f} ms/token (min {t[1] / n:.4f}, max {t[2] / n:.4f})"


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; arms interleaved per round; library "
      f"{os.environ.get('ULL_LIB_PATH', 'as built')}")
model, cfg = bench.build_model(336, dev)
tok = None
if not a.plain:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stop_tokenizer import build_tokenizer
    T = importlib.import_module("u-llava_amd.tools")
    tok = build_tokenizer(vocab_size=model.config.vocab_size)
    t0 = time.perf_counter()
    G = importlib.import_module("u-llava_amd.generation")
    G.stop_table(model, tok, dev)
    print(f"token byte table of {model.config.vocab_size} ids: built and copied in {(time.perf_counter() - t0) * 1e3:.0f} ms (once per tokenizer)")

for B in (1, 16):
    images, ids, _ = bench.make_inputs(cfg, B, 64, dev, 1)
    for new in (64, 512):
        for name, pick in (("greedy", dict(do_sample=False)), ('sampler="device"', dict(do_sample=True, temperature=0.7, top_k=50, sampler="device"))):
            kw = dict(input_ids=ids, images=images, max_new_tokens=new, use_cache=True, eos_token_id=-1, **pick)
            L = ids.shape[1] + new

            def run(**more):
                with torch.no_grad():
                    out = model.generate(**kw, **more)
                assert out.shape[1] == L, (out.shape, L)             # no run stops early
            fns = {"(a)  no criterion": run}
            if not a.plain:
                fns["(a2) no criterion, again"] = run
                fns["(b)  KeywordsStoppingCriteria"] = lambda: run(stopping_criteria=[T.KeywordsStoppingCriteria([STOP], tok, ids)])
                fns["(c)  stop_strings"] = lambda: run(stop_strings=[STOP], tokenizer=tok)
            r = wall(fns, a.reps, a.warmup)
            print(f"-- batch {B}, {new} new tokens, {name}")
            for k, t in r.items():
                print(f"    {k:32s} {per_token(t, new)}")
            if not a.plain:
                ta, ta2, tb, tc = (r[k][0] / new * 1e3 for k in fns)
                print(f"    per token: spread of (a) {abs(ta2 - ta):.1f} us; (c) - (a) = {tc - ta:+.1f} us; (b) - (a) = {tb - ta:+.1f} us; (b) - (c) = {tb - tc:+.1f} us")
