#!/usr/bin/env python
"""MXFP4 weight-only decode against bf16 and FP8 (e4m3), in ONE process on the same random-init model: ViT-L/14-336 + LLaMA-7B, a 336 x 336
image + 64-token prompt (S = 643), KV-cached greedy decoding at batch 1 (GEMV), 4 and 16 (skinny MFMA GEMM).  Times the bf16 model, calls
quantize_weights("fp8_e4m3") and times the same steps, then rebuilds the model from the same seed, calls quantize_weights("mxfp4") and times
them again.  Prints per batch and format: prefill + first token, ms per decode step (median and the spread of --reps runs), the effective
weight stream rate, torch.cuda.memory_allocated; and the relative Frobenius error of both formats' dequantized weights (computed on the
device).  --sweep adds the launch-shape sweep of the mxfp4 GEMV at batch 1; it needs a library built with the tuning switch
(`make -C u-llava_amd/csrc clean`, then `make -C u-llava_amd/csrc HIPCC="/opt/rocm/bin/hipcc -DULL_W4_TUNE"`, or ULL_LIB_PATH pointing at
such a build), which the shipped build leaves out.

    python tools/mxfp4_decode_bench.py [--new 33] [--reps 3] [--sweep]
    python tools/mxfp4_decode_bench.py --prefill-only        # an mxfp4 model's prefill + 1 token, twice: the run to put under a kernel trace
"""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--new", type=int, default=33, help="tokens generated in the timed run (the first one is the prefill's)")
ap.add_argument("--reps", type=int, default=3, help="timed runs per configuration; the median is reported")
ap.add_argument("--sweep", action="store_true", help="also sweep the mxfp4 GEMV's launch shape at batch 1 (needs a -DULL_W4_TUNE build)")
ap.add_argument("--prefill-only", action="store_true")
a = ap.parse_args()
dev = "cuda:0"
BATCHES = (1, 4, 16)


def llama_linears(core):
    for l in core.model.layers:
        yield from (l.self_attn.q_proj, l.self_attn.k_proj, l.self_attn.v_proj, l.self_attn.o_proj, l.mlp.gate_proj, l.mlp.up_proj,
                    l.mlp.down_proj)
    yield core.lm_head


def time_decode(model, ids, images, reps):
    """((prefill + 1 token in ms: median), (ms per decode step: median, min, max)) over `reps` of generate(1) and generate(--new)."""
    pre, step = [], []
    with torch.no_grad():
        model.generate(input_ids=ids, images=images, max_new_tokens=2, do_sample=False, use_cache=True, eos_token_id=-1)   # warm-up
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            model.generate(input_ids=ids, images=images, max_new_tokens=1, do_sample=False, use_cache=True, eos_token_id=-1)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            model.generate(input_ids=ids, images=images, max_new_tokens=a.new, do_sample=False, use_cache=True, eos_token_id=-1)
            torch.cuda.synchronize(); t2 = time.perf_counter()
            pre.append(t1 - t0)
            step.append(((t2 - t1) - (t1 - t0)) / (a.new - 1))
    step.sort()
    return sorted(pre)[len(pre) // 2] * 1e3, (step[len(step) // 2] * 1e3, step[0] * 1e3, step[-1] * 1e3)


model, cfg = bench.build_model(336, dev)
ops, _lib = importlib.import_module("u-llava_amd.ops"), importlib.import_module("u-llava_amd._lib")
inputs = {b: bench.make_inputs(cfg, b, 64, dev, b) for b in BATCHES}

if a.prefill_only:
    with torch.no_grad():
        model.quantize_weights("mxfp4")
        for _ in range(2):
            model.generate(input_ids=inputs[1][1], images=inputs[1][0], max_new_tokens=1, do_sample=False, use_cache=True, eos_token_id=-1)
    torch.cuda.synchronize()
    sys.exit(0)

lin = list(llama_linears(model))
n_w = sum(m.weight.numel() for m in lin)
bytes_ = {"bf16": 2 * n_w, "fp8": n_w + 4 * sum(m.weight.shape[0] for m in lin), "mxfp4": n_w // 2 + n_w // 32}
del lin


def frob():
    num = {"fp8": 0.0, "mxfp4": 0.0}
    den = 0.0
    with torch.no_grad():
        for m in llama_linears(model):
            w = m.weight.detach().contiguous()
            wf = w.double()
            den += float((wf * wf).sum())
            for fmt, q, dq in (("fp8", ops.quantize_fp8, ops.dequantize_fp8), ("mxfp4", ops.quantize_mxfp4, ops.dequantize_mxfp4)):
                d = dq(q(w)).double() - wf
                num[fmt] += float((d * d).sum())
    return {k: (v / den) ** 0.5 for k, v in num.items()}


err = frob()
res = {}
for fmt in ("bf16", "fp8", "mxfp4"):
    if fmt == "mxfp4":
        del model
        torch.cuda.empty_cache()
        model, cfg = bench.build_model(336, dev)            # the same seed: the same weights
    if fmt != "bf16":
        with torch.no_grad():
            model.quantize_weights("fp8_e4m3" if fmt == "fp8" else "mxfp4")
        torch.cuda.synchronize()
    for b in BATCHES:
        images, ids, _ = inputs[b]
        res[(fmt, b)] = time_decode(model, ids, images, a.reps)
    torch.cuda.synchronize()
    res[(fmt, "mem")] = torch.cuda.memory_allocated(dev)

print(f"LLaMA-7B Linear + lm_head weights: {n_w / 1e9:.3f} G elements; streamed per decode step: bf16 {bytes_['bf16'] / 1e9:.2f} GB, "
      f"fp8 {bytes_['fp8'] / 1e9:.2f} GB (codes + row scales), mxfp4 {bytes_['mxfp4'] / 1e9:.2f} GB (codes + block scales)")
print("torch.cuda.memory_allocated after the runs: " + ", ".join(f"{f} {res[(f, 'mem')] / 2**30:.2f} GiB" for f in ("bf16", "fp8", "mxfp4")))
print(f"relative Frobenius error of dequant(Q(W)) over these weights (N(0, 0.02) random init, round-to-nearest, no calibration): "
      f"fp8 {err['fp8']:.4e}, mxfp4 {err['mxfp4']:.4e}")
for b in BATCHES:
    for fmt in ("bf16", "fp8", "mxfp4"):
        pre, (st, lo, hi) = res[(fmt, b)]
        print(f"batch {b:2d} {fmt:5s}: prefill + 1 token {pre:7.2f} ms; decode {st:.3f} ms/step (min {lo:.3f}, max {hi:.3f}) = "
              f"{b / st * 1e3:7.1f} tokens/s; {bytes_[fmt] / (st * 1e-3) / 1e12:.2f} TB/s effective")
    m4, f8, bf = res[("mxfp4", b)], res[("fp8", b)], res[("bf16", b)]
    spread = max(f8[1][2] - f8[1][1], m4[1][2] - m4[1][1])
    print(f"batch {b:2d} mxfp4 / bf16: decode {m4[1][0] / bf[1][0]:.3f}x; mxfp4 / fp8: decode {m4[1][0] / f8[1][0]:.3f}x "
          f"({m4[1][0] - f8[1][0]:+.3f} ms; run-to-run spread {spread:.3f} ms); prefill + 1 token mxfp4 - bf16 {m4[0] - bf[0]:+.2f} ms, "
          f"mxfp4 - fp8 {m4[0] - f8[0]:+.2f} ms")

if a.sweep:
    tune = getattr(_lib.load(), "ull_gemv_w4_tune_bf16", None)
    if tune is None:
        sys.exit("--sweep needs a library built with -DULL_W4_TUNE (see the docstring)")
    images, ids, _ = inputs[1]
    print("launch-shape sweep of the mxfp4 GEMV (batch 1 decode ms/step, median of --reps; u = 16-byte loads per lane in flight):")
    for u in (1, 2, 4):
        row = []
        for blocks in (1024, 1536, 2048, 3072, 4096):
            assert tune(u, blocks) == 0
            row.append(f"{blocks}: {time_decode(model, ids, images, a.reps)[1][0]:.3f}")
        print(f"  u = {u}:  " + "   ".join(row))
