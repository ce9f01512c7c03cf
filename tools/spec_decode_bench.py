#!/usr/bin/env python
"""Prompt-lookup speculative decoding (generate(prompt_lookup_num_tokens=), DESIGN f13): what a verify step costs, what the per-step host read
costs, and what the loop gives on two prompts, in ONE process on random-init LLaMA-7B weights (bench.build_model).

  --tiny    the tiny fixture model only: the largest |logit difference| between the one-token path and the multi-token path (chunks of
            2 .. 16 new tokens over the same cached prefix) on the plain greedy run of the prompt tests/test_prompt_lookup_gpu.py uses; its
            TAU is 1.5 times this figure.
  --plain   plain generate() only (no new option): 64 greedy tokens on the bench prompt, for an A/B of two builds of the library (ULL_LIB_PATH).
  default   1. one verify step at B = 1 with S = 1, 2, 4, 5, 8, 16 new tokens from a cache of --past positions, for the bf16, the fp8-weight
               and the A8 "prefill+decode" model, arms interleaved per round; S = 1 is the plain decode step.  step(S) / step(1) is the
               break-even number of tokens per step.
            2. plain greedy generate() with the 8-step host check against a per-step check (a stopping criterion that never fires).
            3. tokens per second and acceptance rate of the speculative loop against the plain loop on two prompts.
Times are device-event medians over --reps rounds after --warmup rounds, with min and max (whole generate() calls: wall clock around a
synchronize).

    python tools/spec_decode_bench.py [--reps 7] [--warmup 2] > profiles/spec_decode.txt
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
ap.add_argument("--past", type=int, default=643, help="positions in the KV cache before the timed step")
ap.add_argument("--tiny", action="store_true")
ap.add_argument("--plain", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("spec_decode_bench: needs the GPU (nothing is measured without one)")
dev = torch.device("cuda:0")
ops = importlib.import_module("u-llava_amd.ops")
MC = importlib.import_module("u-llava_amd.modeling_core")
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


def wall(fns, reps, warmup):
    """the same for whole generate() calls, which read the host themselves: wall clock between synchronizes."""
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


def fmt(t, div=1.0, unit="ms"):
    return f"{t[0] / div:8.3f} {unit} (min {t[1] / div:.3f}, max {t[2] / div:.3f})"


def tiny_path_diff():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import fixture_sd, load_fixture
    C = importlib.import_module("u-llava_amd.configuration")
    fx = load_fixture("g1_core_tiny_bf16.pt")
    cd = fx["cfg"]
    cfg = C.UllavaCoreConfig(vision_config=cd["vision_config"], vision_hidden_layer=cd["vision_hidden_layer"], projector_type=cd["projector_type"],
                             mm_token_ids=None, vocab_size=cd["vocab_size"], hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"],
                             num_hidden_layers=cd["num_hidden_layers"], num_attention_heads=cd["num_attention_heads"], rms_norm_eps=cd["rms_norm_eps"],
                             rope_theta=cd["rope_theta"])
    m = MC.UllavaCoreForCausalLM(cfg, device=dev, dtype=BF)
    m.load_state_dict(fixture_sd(fx, BF), strict=True)
    g = torch.Generator().manual_seed(3)
    phrase = torch.randint(3, 90, (11,), generator=g).tolist()
    ids = torch.tensor([phrase * 6 + phrase[:3]], device=dev)
    L0, NEW = ids.shape[1], 32

    def cache():
        c = m.config
        return MC.KVCache(c.num_hidden_layers, 1, c.num_attention_heads, c.hidden_size // c.num_attention_heads, L0 + NEW + 17, dev, BF)
    with torch.no_grad():
        plain = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=-1)
        kc = cache()
        one = [m.forward(input_ids=ids, past_key_values=kc, use_cache=True).logits[0, -1].float()]
        for t in range(NEW - 1):
            one.append(m.forward(input_ids=plain[:, L0 + t:L0 + t + 1], past_key_values=kc, use_cache=True).logits[0, -1].float())
        one = torch.stack(one)                                   # row t: the logits that pick token t of the plain run
        assert torch.equal(one.argmax(-1), plain[0, L0:])
        worst = 0.0
        for S in range(2, 17):
            kc = cache()
            m.forward(input_ids=ids, past_key_values=kc, use_cache=True)
            diff, t = 0.0, 0
            while t < NEW - 1:
                n = min(S, NEW - 1 - t)
                lg = m.forward(input_ids=plain[:, L0 + t:L0 + t + n], past_key_values=kc, use_cache=True).logits[0].float()
                diff = max(diff, float((lg - one[t + 1:t + 1 + n]).abs().max()))
                t += n
            print(f"    chunks of {S:2d} new tokens: max |logit difference| to the one-token path {diff:.6f}")
            worst = max(worst, diff)
    top2 = one.topk(2, dim=-1)[0]
    gaps = (top2[:, 0] - top2[:, 1]).tolist()
    tau = 1.5 * worst
    n_cmp = next((t for t, gp in enumerate(gaps) if gp < tau), NEW)
    print(f"-- tiny fixture model (bf16), prompt of {L0} ids, {NEW} plain greedy tokens; logits reach |{float(one.abs().max()):.3f}|")
    print(f"    MEASURED_PATH_DIFF = {worst!r}    tau = 1.5 x = {tau!r}")
    print(f"    top-two gaps of the plain run: min {min(gaps):.6f}, median {sorted(gaps)[len(gaps) // 2]:.6f}; first gap below tau at position {n_cmp} of {NEW}")


def plain_generate(model, cfg):
    images, ids, _ = bench.make_inputs(cfg, 1, 64, dev, 1)
    kw = dict(input_ids=ids, images=images, max_new_tokens=64, do_sample=False, use_cache=True, eos_token_id=-1)
    with torch.no_grad():
        r = wall({"plain": lambda: model.generate(**kw)}, a.reps, a.warmup)
    print(f"-- plain greedy generate(), no new option: 64 tokens at batch 1 on the bench prompt, library {os.environ.get('ULL_LIB_PATH', 'as built')}")
    print(f"    {fmt(r['plain'])}   = {r['plain'][0] / 64:.3f} ms per token incl. the prefill")


def verify_steps(m16, m8):
    g = torch.Generator(device="cuda").manual_seed(1)
    prompt = torch.randint(5, 32000, (1, a.past), device=dev, generator=g)
    toks = torch.randint(5, 32000, (1, 16), device=dev, generator=g)
    with torch.no_grad():
        caches = {id(m): m(input_ids=prompt, use_cache=True).past_key_values for m in (m16, m8)}

    def arm(m, act, scope, S):
        cache = caches[id(m)]

        def f():
            m.activation_quantization, m.activation_scope = act, scope
            with torch.no_grad():
                m(input_ids=toks[:, :S], past_key_values=cache, use_cache=True)
            cache.truncate(a.past)                               # the next timed step rewrites the same positions
        return f
    res = {}
    for S in (1, 2, 4, 5, 8, 16):
        res[S] = timed({"bf16": arm(m16, None, "prefill", S), "fp8 weights": arm(m8, None, "prefill", S),
                        "A8 prefill+decode": arm(m8, "fp8_e4m3", "prefill+decode", S)}, a.reps, a.warmup + 1)
    m8.activation_quantization, m8.activation_scope = None, "prefill"
    print(f"-- one forward at B = 1 over S new tokens from a cache of {a.past} positions (embedding, 32 layers, final norm, lm_head on S rows); "
          "S = 1 is the plain decode step")
    for k in ("bf16", "fp8 weights", "A8 prefill+decode"):
        for S, r in res.items():
            print(f"    {k:18s} S = {S:2d}  {fmt(r[k])}   step(S) / step(1) = {r[k][0] / res[1][k][0]:.3f}")
    del caches
    torch.cuda.empty_cache()


def host_read_cost(m16, cfg):
    images, ids, _ = bench.make_inputs(cfg, 1, 64, dev, 1)
    kw = dict(input_ids=ids, images=images, max_new_tokens=64, do_sample=False, use_cache=True, eos_token_id=-1)
    never = lambda seq, scores: torch.tensor(False)              # forces generate()'s per-step check (and per-step device -> host read)
    with torch.no_grad():
        r = wall({"check every 8 steps": lambda: m16.generate(**kw), "check every step": lambda: m16.generate(stopping_criteria=[never], **kw)},
                 a.reps, a.warmup)
    print("-- the per-step host read: plain greedy generate(), bf16, 64 tokens at batch 1 on the bench prompt")
    for k, t in r.items():
        print(f"    {k:20s} {fmt(t)}")
    d = (r["check every step"][0] - r["check every 8 steps"][0]) / 64
    print(f"    per-step check costs {d * 1e3:.1f} us per token ({d / (r['check every 8 steps'][0] / 64) * 100:.2f} % of a token)")


def loops(m16, cfg):
    images, ids, _ = bench.make_inputs(cfg, 1, 64, dev, 1)
    g = torch.Generator().manual_seed(7)
    phrase = torch.randint(5, 32000, (24,), generator=g)
    rep = phrase.repeat(16)[None].to(dev)                        # a phrase of 24 ids sixteen times: 384 text ids, no image
    print("-- the loop, bf16, greedy, 64 new tokens at batch 1, k = prompt_lookup_num_tokens (n-gram size 2).  RANDOM-INIT weights: the acceptance "
          "rate of these runs says nothing about real checkpoints, where it depends on how much of the answer repeats the prompt")
    for name, kw in (("bench prompt (336 x 336 image + 64 random ids)", dict(input_ids=ids, images=images)),
                     ("repetitive text prompt (24 ids x 16)", dict(input_ids=rep))):
        kw = dict(max_new_tokens=64, do_sample=False, use_cache=True, eos_token_id=-1, **kw)
        L0 = kw["input_ids"].shape[1]
        fns = {"plain": lambda kw=kw: m16.generate(**kw)}
        for k in (4, 10):
            fns[f"k = {k}"] = lambda kw=kw, k=k: m16.generate(prompt_lookup_num_tokens=k, **kw)
        with torch.no_grad():
            r = wall(fns, a.reps, a.warmup)
            plain = m16.generate(**kw)
        print(f"    {name}")
        for key, t in r.items():
            line = f"        {key:8s} {fmt(t)}   {64 / t[0] * 1e3:7.1f} tokens/s incl. the prefill"
            if key != "plain":
                k = int(key.split()[-1])
                stats, orig = [], ops.spec_step

                def counting(*args, _o=orig, _s=stats):          # (an untimed run: the extra read of the record is not in the times above)
                    _o(*args)
                    _s.append((args[7], args[-1].tolist()[0]))   # (drafts verified, tokens emitted)
                ops.spec_step = counting
                try:
                    with torch.no_grad():
                        out = m16.generate(prompt_lookup_num_tokens=k, **kw)
                finally:
                    ops.spec_step = orig
                drafted, accepted = sum(d for d, e in stats), sum(e - 1 for d, e in stats)
                same = int((out[0, L0:] == plain[0, L0:]).sum())
                line += (f"; {len(stats)} forwards, {drafted} drafts, {accepted} accepted ({100.0 * accepted / max(drafted, 1):.0f} %), "
                         f"{64 / len(stats):.2f} tokens per forward; {same} of 64 ids equal the plain run's")
            print(line)


print(f"device: {torch.cuda.get_device_name(0)}; reps {a.reps}, warm-up {a.warmup}; arms interleaved per round")
if a.tiny:
    tiny_path_diff()
    sys.exit(0)
m16, cfg = bench.build_model(336, dev)
if a.plain:
    plain_generate(m16, cfg)
    sys.exit(0)
m8, _ = bench.build_model(336, dev)                              # the same seed: the same weights
with torch.no_grad():
    m8.quantize_weights("fp8_e4m3")
verify_steps(m16, m8)
del m8
torch.cuda.empty_cache()
host_read_cost(m16, cfg)
loops(m16, cfg)
