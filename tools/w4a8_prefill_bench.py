#!/usr/bin/env python
"""MXFP8-activation (W4A8) and MXFP4-activation (W4A4) prefill on MXFP4 weights against the bf16 model, the weight-only mxfp4 model (dequantize + bf16 GEMM: the yardstick)
and the W8A8 Linear, in ONE process on the same random-init LLaMA-7B weights.  Arms, interleaved round by round:

    bf16   the bf16 model
    w4a16  quantize_weights("mxfp4"): every prefill Linear dequantizes its weight into a scratch and runs the bf16 GEMM
    w8a8   ops.linear_a8w8 on the fp8-quantized weight (layer launches only)
    w4a8   quantize_weights("mxfp4", activations="mxfp8_e4m3"): ops.linear_w4a8 (block quantization + the block-scaled matrix instruction)
    w4a4   quantize_weights("mxfp4", activations="mxfp4_e2m1"): ops.linear_w4a4 (the same with e2m1 activations; its yardstick is w4a8)

Measured: the four LLaMA-layer launches (q|k|v, o_proj + residual, gate|up + SwiGLU, down_proj + residual) and the whole 32-layer LLaMA
prefill (`_llama` on random embeddings: no CLIP, no lm_head), at the C4 shape (batch 32, S = 643) and at batch 1, and the memory the mxfp4
model holds.  The w4a8 launch time is given with the activation quantization included (what the model pays) and excluded (included minus
the separately timed quantize launch); the same for w4a4.  Times are device-event medians over --reps rounds after --warmup rounds, with min and max.
Decode: ms per greedy decode step of the whole model (64-token prompt + one image, batch 1 and 16) with the mode off (the parent's mxfp4
model) and on, interleaved; the decode launches are the same W4A16 kernels in both.

    python tools/w4a8_prefill_bench.py [--reps 7] [--warmup 2] [--accuracy] > profiles/w4a4_prefill.txt

--accuracy adds, on the committed full-depth samples (tests/golden/g15_c1_full_depth_bf16.pt), the logit error against the reference and the
greedy-token agreement at the margin-gated positions for bf16 / w4a16 / w4a8 / w4a4 (builds the fixture's seeded weights on the host first: minutes).
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--accuracy", action="store_true")
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--new", type=int, default=33, help="tokens generated in the timed decode run (the first one is the prefill's)")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("w4a8_prefill_bench: needs the GPU (nothing is measured without one)")
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


def layer_launches(M):
    D, I = 4096, 11008
    g = torch.Generator(device="cuda").manual_seed(M)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(BF)
    print(f"-- LLaMA-layer launches at M = {M} tokens (Gaussian activations, N(0, 0.02) weights)")
    for name, N, K, kw in (("q|k|v", 3 * D, D, {}), ("o_proj + residual", D, D, dict(residual=True)),
                           ("gate|up + SwiGLU", 2 * I, D, dict(swiglu=True)), ("down_proj + residual", D, I, dict(residual=True))):
        w = rnd(N, K, sc=0.02)
        ops.register_tiled(w)
        q8, q4 = ops.quantize_fp8(w), ops.quantize_mxfp4(w)
        x = rnd(M, K)
        args = dict(swiglu=True) if kw.get("swiglu") else {}
        if kw.get("residual"):
            args["residual"] = rnd(M, N)
        out = torch.empty(M, N // 2 if kw.get("swiglu") else N, device=dev, dtype=BF)
        with torch.no_grad():
            r = timed({"bf16": lambda: ops.linear(x, w, out=out, **args), "w4a16": lambda: ops.linear(x, q4, out=out, **args),
                       "w8a8": lambda: ops.linear_a8w8(x, q8, out=out, **args), "w4a8": lambda: ops.linear_w4a8(x, q4, out=out, **args),
                       "quantize": lambda: ops._quantize_rows_mxfp8(x, K), "w4a4": lambda: ops.linear_w4a4(x, q4, out=out, **args),
                       "quantize4": lambda: ops._quantize_rows_mxfp4(x, K, 1)}, a.reps, a.warmup)
        flop = 2.0 * M * N * K
        excl = r["w4a8"][0] - r["quantize"][0]
        excl4 = r["w4a4"][0] - r["quantize4"][0]
        print(f"{name:22s} [{M} x {K}] @ [{N} x {K}]^T")
        for k in ("bf16", "w4a16", "w8a8", "w4a8", "w4a4"):
            print(f"    {k:6s} {fmt(r[k])}  {flop / r[k][0] / 1e9:7.1f} TFLOP/s")
        print(f"    w4a8 without the activation quantization ({r['quantize'][0]:.3f} ms): {excl:8.3f} ms  {flop / excl / 1e9:7.1f} TFLOP/s;"
              f"  w4a8 / bf16 = {r['w4a8'][0] / r['bf16'][0]:.3f} (incl.), {excl / r['bf16'][0]:.3f} (excl.);  w4a8 / w4a16 = {r['w4a8'][0] / r['w4a16'][0]:.3f};"
              f"  w4a8 / w8a8 = {r['w4a8'][0] / r['w8a8'][0]:.3f}")
        gain = "faster, ranges apart" if r["w4a4"][2] < r["w4a8"][1] else "slower, ranges apart" if r["w4a4"][1] > r["w4a8"][2] else "ranges overlap"
        print(f"    w4a4 without the activation quantization ({r['quantize4'][0]:.3f} ms): {excl4:8.3f} ms  {flop / excl4 / 1e9:7.1f} TFLOP/s;"
              f"  w4a4 / w4a8 = {r['w4a4'][0] / r['w4a8'][0]:.3f} (incl.: {gain}), {excl4 / excl:.3f} (excl.);  w4a4 / bf16 = {r['w4a4'][0] / r['bf16'][0]:.3f}")
        ops.unregister_tiled(w)
        del w, q8, q4, x, out, args


def whole_prefill(models, B, S=643):
    g = torch.Generator(device="cuda").manual_seed(B)
    emb = (torch.randn(B, S, 4096, device=dev, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, S, device=dev, dtype=torch.int64)
    m16, m4 = models

    def arm(m, act):
        def f():
            m.activation_quantization = act
            with torch.no_grad():
                m._llama(emb, mask, None, False)
        return f
    r = timed({"bf16": arm(m16, None), "w4a16": arm(m4, None), "w4a8": arm(m4, "mxfp8_e4m3"), "w4a4": arm(m4, "mxfp4_e2m1")}, a.reps, a.warmup)
    m4.activation_quantization = None
    print(f"-- whole LLaMA prefill (32 layers + final norm), batch {B} x S = {S}  ({B * S} tokens)")
    for k in ("bf16", "w4a16", "w4a8", "w4a4"):
        print(f"    {k:6s} {fmt(r[k])}  {B * S / r[k][0]:9.1f} tokens/ms")
    print(f"    w4a8 / bf16 = {r['w4a8'][0] / r['bf16'][0]:.3f};  w4a8 / w4a16 = {r['w4a8'][0] / r['w4a16'][0]:.3f};  "
          f"w4a4 / w4a8 = {r['w4a4'][0] / r['w4a8'][0]:.3f};  w4a4 / bf16 = {r['w4a4'][0] / r['bf16'][0]:.3f}")


def accuracy():
    """bf16 / w4a16 / w4a8 / w4a4 on the G15 samples: max logit error / max|truth| on the committed rows, and token agreement where the fp32 margin
    clears 4 sigma of the reference's own 16-bit noise."""
    from concurrent.futures import ThreadPoolExecutor
    C, MC, W = importlib.import_module("u-llava_amd.configuration"), importlib.import_module("u-llava_amd.modeling_core"), \
        importlib.import_module("u-llava_amd.weights")
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "g15_c1_full_depth_bf16.pt"), map_location="cpu", weights_only=True)
    cfg = C.UllavaCoreConfig(vision_config=dict(image_size=224, patch_size=14), vision_hidden_layer=-2, projector_type="mlp",
                             projector_from_scratch=False, mm_token_ids=dict(bench.MM), vocab_size=32011)
    with torch.no_grad():
        model = MC.UllavaCoreForCausalLM(cfg, device=dev, dtype=BF)
        model.strict_checks = False
        sd = model.state_dict(keep_vars=True)
        shapes = {k: tuple(v) for k, v in fx["shapes"].items()}
        keys = [k for k in shapes if k in sd]
        assert len(keys) == len(sd), "state-dict keys differ from the fixture's"

        def gen(k):
            return k, W.seeded_tensor(k, shapes[k], fx["seed"], torch.float32, hf_init=True)
        with ThreadPoolExecutor(max_workers=16) as ex:
            for i in range(0, len(keys), 48):
                for k, t in ex.map(gen, keys[i:i + 48]):
                    sd[k].data.copy_(t.to(BF))
        model._packed = None
        inp = dict(input_ids=fx["input_ids"].to(dev), attention_mask=fx["attention_mask"].to(dev), images=fx["images"].to(dev))
        rec = fx["logits"]
        gap = rec["truth_top_values"][:, 0] - rec["truth_top_values"][:, 1]
        gated = gap > 4.0 * rec["sigma"]
        print(f"-- accuracy on the committed full-depth samples (G15, bf16): {int(gated.sum())} of {gap.numel()} positions are margin-gated")

        def report(name):
            lg = model(**inp).logits[0].float().cpu()
            rows = rec["rows"]
            d = lg[rows] - rec["truth_rows"].float()
            dr = rec["ref_rows"].float() - rec["truth_rows"].float()
            am = lg.argmax(-1)
            agree = float((am == rec["truth_argmax"].long())[gated].float().mean())
            print(f"    {name:6s} logit error vs the reference's fp32 run: max {float(d.abs().max()) / rec['truth_absmax']:.5f} rms {float(d.pow(2).mean().sqrt()):.5f}"
                  f"  (the reference's own bf16 run: max {float(dr.abs().max()) / rec['truth_absmax']:.5f} rms {float(dr.pow(2).mean().sqrt()):.5f});"
                  f"  greedy-token agreement at the gated positions: {agree * 100:.2f} %  ({int((am != rec['truth_argmax'].long())[gated].sum())} differ)")
        report("bf16")
        model.quantize_weights("mxfp4")
        report("w4a16")
        model.quantize_weights("mxfp4", activations="mxfp8_e4m3")
        report("w4a8")
        model.quantize_weights("mxfp4", activations="mxfp4_e2m1")
        report("w4a4")
    del model
    torch.cuda.empty_cache()


def decode(m4, cfg):
    """ms per greedy decode step (generate(--new) minus generate(1), per extra token) with the mode off and on, interleaved."""
    print(f"-- decode, whole model, 64-token prompt + one image, {a.new - 1} timed steps; off = the weight-only mxfp4 model")
    for B in (1, 16):
        images, ids = bench.make_inputs(cfg, B, 64, dev, B)[:2]
        kw = dict(input_ids=ids, images=images, do_sample=False, use_cache=True, eos_token_id=-1)
        ts = {None: [], "mxfp8_e4m3": [], "mxfp4_e2m1": []}
        with torch.no_grad():
            for act in ts:
                m4.activation_quantization = act
                m4.generate(max_new_tokens=2, **kw)
            for _ in range(a.reps):
                for act in ts:
                    m4.activation_quantization = act
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    m4.generate(max_new_tokens=1, **kw)
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    m4.generate(max_new_tokens=a.new, **kw)
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    ts[act].append((((t2 - t1) - (t1 - t0)) / (a.new - 1) * 1e3, (t1 - t0) * 1e3))
        m4.activation_quantization = None
        for act, v in ts.items():
            st, pre = sorted(x[0] for x in v), sorted(x[1] for x in v)
            print(f"    batch {B:2d}  activations={str(act):12s} {st[len(st) // 2]:7.3f} ms per token (min {st[0]:.3f}, max {st[-1]:.3f});"
                  f"  prefill + first token {pre[len(pre) // 2]:8.3f} ms")


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; times from device events, arms interleaved per round")
if not a.skip_timing:
    for M in (32 * 643, 643):
        layer_launches(M)
    m16, _ = bench.build_model(336, dev)
    m4, _cfg = bench.build_model(336, dev)                       # the same seed: the same weights
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        m4.quantize_weights("mxfp4")
    torch.cuda.empty_cache()
    print(f"-- memory_allocated: both models {before / 2**30:.2f} GiB, after quantize_weights('mxfp4') on one {torch.cuda.memory_allocated() / 2**30:.2f} GiB "
          f"(the mode adds no weight copy: the activation codes and scale bytes of one Linear are transient)")
    for B in (32, 1):
        whole_prefill((m16, m4), B)
    decode(m4, _cfg)
    print(f"-- memory_allocated after the prefills and decodes: {torch.cuda.memory_allocated() / 2**30:.2f} GiB")
    del m16, m4
    torch.cuda.empty_cache()
if a.accuracy:
    accuracy()
