#!/usr/bin/env python
"""FP8 (e4m3) weight-only decode against bf16, in ONE process on the same model: ViT-L/14-336 + LLaMA-7B (random init), a 336 x 336 image +
64-token prompt (S = 643), KV-cached greedy decoding at batch 1 (GEMV) and batch 4 (skinny MFMA GEMM).  Times the bf16 model, then calls
quantize_weights() and times the same steps again.  Prints per batch: prefill + first token, ms per decode step, and the effective weight
stream rate (resident LLaMA-Linear + lm_head bytes / step time); plus the resident weight bytes before and after.

    python tools/fp8_decode_bench.py [--new 33] [--reps 3]
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
a = ap.parse_args()
dev = "cuda:0"


def llama_linears(core):
    for l in core.model.layers:
        yield from (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj,
                    l.mlp.down_proj)
    yield core.lm_head


def time_decode(model, ids, images):
    """(prefill + 1 token in ms, ms per decode step): median over --reps of generate(1) and generate(--new)."""
    pre, step = [], []
    with torch.no_grad():
        model.generate(input_ids=ids, images=images, max_new_tokens=2, do_sample=False, use_cache=True, eos_token_id=-1)   # warm-up
        for _ in range(a.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.generate(input_ids=ids, images=images, max_new_tokens=1, do_sample=False, use_cache=True, eos_token_id=-1)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            model.generate(input_ids=ids, images=images, max_new_tokens=a.new, do_sample=False, use_cache=True, eos_token_id=-1)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            pre.append(t1 - t0)
            step.append(((t2 - t1) - (t1 - t0)) / (a.new - 1))
    return sorted(pre)[len(pre) // 2] * 1e3, sorted(step)[len(step) // 2] * 1e3


model, cfg = bench.build_model(336, dev)
inputs = {b: bench.make_inputs(cfg, b, 64, dev, b) for b in (1, 4)}
n_w = sum(m.weight.numel() for m in llama_linears(model))
res = {}
bytes_ = {"bf16": 2 * n_w, "fp8": n_w + 4 * sum(m.weight.shape[0] for m in llama_linears(model))}
for fmt in ("bf16", "fp8"):
    if fmt == "fp8":
        with torch.no_grad():
            model.quantize_weights("fp8_e4m3")
        torch.cuda.synchronize()
    for b in (1, 4):
        images, ids, _ = inputs[b]
        res[(fmt, b)] = time_decode(model, ids, images)
    torch.cuda.synchronize()
    res[(fmt, "mem")] = torch.cuda.memory_allocated(dev)

print(f"LLaMA-7B Linear + lm_head weights: {n_w / 1e9:.3f} G elements; streamed per decode step: bf16 {bytes_['bf16'] / 1e9:.2f} GB, "
      f"fp8 {bytes_['fp8'] / 1e9:.2f} GB (codes + row scales)")
print(f"torch.cuda.memory_allocated after the runs: bf16 {res[('bf16', 'mem')] / 2**30:.2f} GiB, fp8 {res[('fp8', 'mem')] / 2**30:.2f} GiB "
      "(bf16: parameters + packs + tile-major copies; fp8: codes + scales + one dequantize scratch)")
for b in (1, 4):
    for fmt in ("bf16", "fp8"):
        pre, st = res[(fmt, b)]
        print(f"batch {b} {fmt:4s}: prefill + 1 token {pre:7.2f} ms; decode {st:.3f} ms/step = {b / st * 1e3:7.1f} tokens/s; "
              f"{bytes_[fmt] / (st * 1e-3) / 1e12:.2f} TB/s effective")
    print(f"batch {b} fp8 / bf16: decode {res[('fp8', b)][1] / res[('bf16', b)][1]:.3f}x, prefill + 1 token "
          f"{res[('fp8', b)][0] / res[('bf16', b)][0]:.3f}x ({res[('fp8', b)][0] - res[('bf16', b)][0]:+.2f} ms)")
