#!/usr/bin/env python
"""FP8-activation (W8A8) prefill against the bf16 model and the weight-only fp8 model (dequantize + bf16 GEMM), in ONE process on the same
random-init LLaMA-7B weights.  Three arms, interleaved round by round:

    bf16   the bf16 model
    w8a16  quantize_weights("fp8_e4m3"): every prefill Linear dequantizes its weight into a scratch and runs the bf16 GEMM
    w8a8   quantize_weights("fp8_e4m3", activations="fp8_e4m3"): ops.linear_a8w8 (row quantization + the fp8 matrix instruction)

Measured: the four LLaMA-layer launches (q|k|v, o_proj + residual, gate|up + SwiGLU, down_proj + residual) and the whole 32-layer LLaMA
prefill (`_llama` on random embeddings: no CLIP, no lm_head), at the C4 shape (batch 32, S = 643) and at batch 1.  The w8a8 launch time is
given with the activation quantization included (what the model pays) and excluded (included minus the separately timed quantize launch).
Times are device-event medians over --reps rounds after --warmup rounds, with min and max.

    python tools/a8w8_prefill_bench.py [--reps 7] [--warmup 2] [--accuracy] > profiles/a8w8_prefill.txt

--accuracy adds, on the committed full-depth samples (tests/golden/g15_c1_full_depth_bf16.pt), the logit error against the reference and the
greedy-token agreement at the margin-gated positions for the three arms (builds the fixture's seeded weights on the host first: minutes).
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
ap.add_argument("--accuracy", action="store_true")
ap.add_argument("--skip-timing", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("a8w8_prefill_bench: needs the GPU (nothing is measured without one)")
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
        q = ops.quantize_fp8(w)
        x = rnd(M, K)
        args = dict(swiglu=True) if kw.get("swiglu") else {}
        if kw.get("residual"):
            args["residual"] = rnd(M, N)
        out = torch.empty(M, N // 2 if kw.get("swiglu") else N, device=dev, dtype=BF)
        with torch.no_grad():
            r = timed({"bf16": lambda: ops.linear(x, w, out=out, **args), "w8a16": lambda: ops.linear(x, q, out=out, **args),
                       "w8a8": lambda: ops.linear_a8w8(x, q, out=out, **args), "quantize": lambda: ops.quantize_rows_fp8(x)}, a.reps, a.warmup)
        flop = 2.0 * M * N * K
        excl = r["w8a8"][0] - r["quantize"][0]
        print(f"{name:22s} [{M} x {K}] @ [{N} x {K}]^T")
        for k in ("bf16", "w8a16", "w8a8"):
            print(f"    {k:6s} {fmt(r[k])}  {flop / r[k][0] / 1e9:7.1f} TFLOP/s")
        print(f"    w8a8 without the activation quantization ({r['quantize'][0]:.3f} ms): {excl:8.3f} ms  {flop / excl / 1e9:7.1f} TFLOP/s;"
              f"  w8a8 / bf16 = {r['w8a8'][0] / r['bf16'][0]:.3f} (incl.), {excl / r['bf16'][0]:.3f} (excl.);  w8a8 / w8a16 = {r['w8a8'][0] / r['w8a16'][0]:.3f}")
        ops.unregister_tiled(w)
        del w, q, x, out, args


def whole_prefill(models, B, S=643):
    g = torch.Generator(device="cuda").manual_seed(B)
    emb = (torch.randn(B, S, 4096, device=dev, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, S, device=dev, dtype=torch.int64)
    m16, m8 = models

    def arm(m, act):
        def f():
            m.activation_quantization = act
            with torch.no_grad():
                m._llama(emb, mask, None, False)
        return f
    r = timed({"bf16": arm(m16, None), "w8a16": arm(m8, None), "w8a8": arm(m8, "fp8_e4m3")}, a.reps, a.warmup)
    m8.activation_quantization = None
    print(f"-- whole LLaMA prefill (32 layers + final norm), batch {B} x S = {S}  ({B * S} tokens)")
    for k in ("bf16", "w8a16", "w8a8"):
        print(f"    {k:6s} {fmt(r[k])}  {B * S / r[k][0]:9.1f} tokens/ms")
    print(f"    w8a8 / bf16 = {r['w8a8'][0] / r['bf16'][0]:.3f};  w8a8 / w8a16 = {r['w8a8'][0] / r['w8a16'][0]:.3f}")


def accuracy():
    """The three arms on the G15 samples: max logit error / max|truth| on the committed rows, and token agreement where the fp32 margin
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
        model.quantize_weights("fp8_e4m3")
        report("w8a16")
        model.quantize_weights("fp8_e4m3", activations="fp8_e4m3")
        report("w8a8")
    del model
    torch.cuda.empty_cache()


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; times from device events, arms interleaved per round")
if not a.skip_timing:
    for M in (32 * 643, 643):
        layer_launches(M)
    m16, _ = bench.build_model(336, dev)
    m8, _ = bench.build_model(336, dev)                    # the same seed: the same weights
    with torch.no_grad():
        m8.quantize_weights("fp8_e4m3")
    for B in (32, 1):
        whole_prefill((m16, m8), B)
    del m16, m8
    torch.cuda.empty_cache()
if a.accuracy:
    accuracy()
