#!/usr/bin/env python
"""FP8 (W8A8) Linears of the SAM ViT-H image encoder (UllavaForCausalLM.set_sam_precision("fp8_e4m3"), DESIGN f12) against the bf16 path, in
ONE process on the same random-init weights (bench.py's model).  Arms are interleaved round by round; times are device-event medians over
--reps rounds after --warmup rounds, with min and max.

  1. the four launches of a ViT-H block (qkv, proj + residual, lin1 + GELU, lin2 + residual; every one with its bias) at M = 4096 B tokens,
     B = 1 and 8:  bf16 as shipped | fp8 with what produces its codes (the fused LayerNorm + quantize for qkv / lin1 -- against LayerNorm +
     bf16 Linear --, the row quantization for proj / lin2) | the fp8 GEMM alone on ready codes;
  2. the fused LayerNorm + quantize launch against layernorm followed by quantize_rows_fp8;
  3. the whole 32-block encoder (patch embed .. neck) at B = 1 and 8: fp8 (per-op loop) against the default (coarse entry, bf16) and the bf16
     per-op loop;
  4. one RES step as `bench.py --full` runs it (batch 8, 3 [SEG] / [LOC] per image), the switch off and on;
  5. the deviation fp8 - bf16 on the same input: encoder output and mask logits of that step, as max / p99 / mean of |d| (random-init
     weights: N(0, 0.02) matrices).

    python tools/sam_fp8_bench.py [--reps 9] [--warmup 3] > profiles/sam_fp8.txt
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--skip-model", action="store_true", help="parts 1 and 2 only")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sam_fp8_bench: needs the GPU (nothing is measured without one)")
dev = torch.device("cuda:0")
ops = importlib.import_module("u-llava_amd.ops")
BF = torch.bfloat16


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


def fmt(t):
    return f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def block_launches(B):
    C, I, M = 1280, 5120, 4096 * B
    g = torch.Generator(device="cuda").manual_seed(B)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(BF)
    nw, nb = (rnd(C, sc=0.1).float() + 1.0).to(BF), rnd(C, sc=0.1)
    print(f"-- ViT-H block launches at M = {M} tokens (B = {B}; Gaussian activations, N(0, 0.02) weights, every Linear with its bias)")
    for name, N, K, normed, kw in (("qkv", 3 * C, C, True, {}), ("proj + residual", C, C, False, dict(residual=True)),
                                   ("lin1 + GELU", I, C, True, dict(act="gelu")), ("lin2 + residual", C, I, False, dict(residual=True))):
        w, bias, x = rnd(N, K, sc=0.02), rnd(N, sc=0.02), rnd(M, K)
        ops.register_tiled(w)
        q = ops.quantize_fp8(w)
        args = {k: v for k, v in kw.items() if k != "residual"}
        if kw.get("residual"):
            args["residual"] = rnd(M, N)
        out = torch.empty(M, N, device=dev, dtype=BF)
        xq, xs = ops.quantize_rows_fp8(x)
        fns = {"bf16": lambda: ops.linear(x, w, bias, out=out, **args), "fp8 gemm": lambda: ops.linear_a8w8_rows(xq, xs, q, bias=bias, out=out, **args)}
        if normed:
            fns["bf16 incl"] = lambda: ops.linear(ops.layernorm(x, nw, nb, 1e-6), w, bias, out=out, **args)
            fns["fp8 incl"] = lambda: ops.linear_a8w8_rows(*ops.layernorm_quantize_rows_fp8(x, nw, nb, 1e-6), q, bias=bias, out=out, **args)
        else:
            fns["fp8 incl"] = lambda: ops.linear_a8w8_rows(*ops.quantize_rows_fp8(x), q, bias=bias, out=out, **args)
        with torch.no_grad():
            r = timed(fns, a.reps, a.warmup)
        flop = 2.0 * M * N * K
        print(f"{name:16s} [{M} x {K}] @ [{N} x {K}]^T")
        print(f"    bf16 Linear                          {fmt(r['bf16'])}  {flop / r['bf16'][0] / 1e9:7.1f} TFLOP/s")
        print(f"    fp8 GEMM alone (ready codes)         {fmt(r['fp8 gemm'])}  {flop / r['fp8 gemm'][0] / 1e9:7.1f} TFLOP/s   fp8 / bf16 = {r['fp8 gemm'][0] / r['bf16'][0]:.3f}")
        if normed:
            print(f"    LayerNorm + bf16 Linear              {fmt(r['bf16 incl'])}")
            print(f"    fused LayerNorm-quantize + fp8 GEMM  {fmt(r['fp8 incl'])}   fp8 / bf16 = {r['fp8 incl'][0] / r['bf16 incl'][0]:.3f}")
        else:
            print(f"    row quantization + fp8 GEMM          {fmt(r['fp8 incl'])}   fp8 / bf16 = {r['fp8 incl'][0] / r['bf16'][0]:.3f}")
        ops.unregister_tiled(w)
        del w, q, x, out, args, xq, xs, fns


def norm_quantize(M, K=1280):
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, K, device=dev, generator=g).to(BF)
    nw, nb = (torch.randn(K, device=dev, generator=g) * 0.1 + 1.0).to(BF), (torch.randn(K, device=dev, generator=g) * 0.1).to(BF)
    with torch.no_grad():
        r = timed({"fused": lambda: ops.layernorm_quantize_rows_fp8(x, nw, nb, 1e-6), "two": lambda: ops.quantize_rows_fp8(ops.layernorm(x, nw, nb, 1e-6)),
                   "layernorm": lambda: ops.layernorm(x, nw, nb, 1e-6), "quantize": lambda: ops.quantize_rows_fp8(x)}, a.reps, a.warmup)
    print(f"[{M} x {K}]  fused {fmt(r['fused'])} | layernorm then quantize_rows_fp8 {fmt(r['two'])} | layernorm alone {fmt(r['layernorm'])} | "
          f"quantize_rows_fp8 alone {fmt(r['quantize'])}   fused / two launches = {r['fused'][0] / r['two'][0]:.3f}")


def stats(d):
    d = d.float().abs().flatten()
    k = max(int(d.numel() * 0.99), 1)
    return f"max {float(d.max()):.3e}  p99 {float(d.kthvalue(k).values):.3e}  mean {float(d.mean()):.3e}"


def encoder_and_res(model, cfg):
    eng = model._sam

    def enc(mode, per_op=False):
        def f():
            eng.linear_precision = mode
            with torch.no_grad():
                if per_op:
                    with ops.per_op_layers():
                        return eng.encode(img)
                return eng.encode(img)
        return f
    for B in (1, 8):
        img = torch.randn(B, 3, 1024, 1024, device=dev, generator=torch.Generator(device="cuda").manual_seed(40 + B)).to(BF)
        r = timed({"bf16": enc(None), "bf16 per-op": enc(None, True), "fp8": enc("fp8_e4m3")}, a.reps, a.warmup)
        print(f"-- whole SAM ViT-H encoder (patch embed, 32 blocks, neck), B = {B}")
        print(f"    bf16, default (coarse entry)   {fmt(r['bf16'])}  {B / r['bf16'][0] * 1e3:7.1f} images/s")
        print(f"    bf16, per-op loop              {fmt(r['bf16 per-op'])}  {B / r['bf16 per-op'][0] * 1e3:7.1f} images/s")
        print(f"    fp8 Linears (per-op loop)      {fmt(r['fp8'])}  {B / r['fp8'][0] * 1e3:7.1f} images/s   fp8 / bf16 default = {r['fp8'][0] / r['bf16'][0]:.3f}")
        ref, new = enc(None)(), enc("fp8_e4m3")()
        print(f"    encoder output, |fp8 - bf16|: {stats(new - ref)}   (max |bf16| {float(ref.float().abs().max()):.3e}, mean |bf16| {float(ref.float().abs().mean()):.3e})")
        del img, ref, new
    # the RES step of `bench.py --full`: batch 8, three rounds "... [SEG] ... [LOC]" per sample
    _, prompt, batch, _ = bench.WORKLOADS["res"]
    vis, ids, mask = bench.make_inputs(cfg, batch, prompt, dev, 0)
    S = ids.shape[1]
    for rr in range(3):
        ids[:, S - 10 - 40 * rr] = bench.SEG
        ids[:, S - 5 - 40 * rr] = bench.LOC
    images_sam = torch.randn(batch, 3, 1024, 1024, device=dev, generator=torch.Generator(device="cuda").manual_seed(2000)).to(BF)
    sizes, resizes = [(480, 640)] * batch, [(768, 1024)] * batch

    def step(mode):
        def f():
            model.set_sam_precision(mode)
            with torch.no_grad():
                return model.forward(images_sam=images_sam, images=vis, input_ids=ids, labels=None, attention_mask=mask, mask_list=[None] * batch,
                                     size_list=sizes, resize_list=resizes, bbox_list=[None] * batch, inference=True)
        return f
    r = timed({"off": step(None), "on": step("fp8_e4m3")}, a.reps, a.warmup)
    print(f"-- one RES step (bench.py's C3: ViT-L/14-224 + LLaMA-7B + SAM ViT-H + mask decoder, batch {batch}, S = {S})")
    print(f"    set_sam_precision(None)        {fmt(r['off'])}  {batch / r['off'][0] * 1e3:7.1f} images/s")
    print(f"    set_sam_precision('fp8_e4m3')  {fmt(r['on'])}  {batch / r['on'][0] * 1e3:7.1f} images/s   on / off = {r['on'][0] / r['off'][0]:.3f}")
    o0, o1 = step(None)(), step("fp8_e4m3")()
    torch.cuda.synchronize()
    m0, m1 = torch.cat([m.flatten() for m in o0["pred_masks"]]), torch.cat([m.flatten() for m in o1["pred_masks"]])
    print(f"    mask logits, |fp8 - bf16|: {stats(m1 - m0)}   (max |bf16| {float(m0.abs().max()):.3e}, mean |bf16| {float(m0.abs().mean()):.3e}; "
          f"sign agreement {float(((m0 > 0) == (m1 > 0)).float().mean()) * 100:.3f} %)")
    model.set_sam_precision(None)


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; times from device events, arms interleaved per round")
for B in (1, 8):
    block_launches(B)
print("-- LayerNorm + per-token e4m3 quantization: one launch against two")
for M in (4096, 32768):
    norm_quantize(M)
if not a.skip_model:
    model, cfg = bench.build_model(bench.WORKLOADS["res"][0], dev, with_sam=True)
    encoder_and_res(model, cfg)
