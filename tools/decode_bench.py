#!/usr/bin/env python
"""KV-cached greedy decoding: prefill a 336x336 image + 64-token prompt (S = 643), then time the
token-by-token steps.  At batch <= 4 a step is one pass over the 13.5 GB of LLaMA-7B weights through the GEMV kernels, so the
roofline is HBM: 13.48 GB / 8 TB/s = 1.69 ms per step.
--sample: sampler="device" at temperature 0.2 / top_k 50 in place of greedy; --logprobs: generate(output_logprobs=True) (one more launch per
step).
--rounds N (the table of profiles/logprobs_decode.txt): one process times every arm -- greedy and sampler="device", each with
output_logprobs off and on where this tree's generate() has the flag -- interleaved per round, N timed rounds after a warm-up round, for
every batch of --batches, with eos_token_id=-1 so that no row ends early.  --tree DIR imports bench.py and the package from another built
checkout (the parent commit, for an A/B by the same method); run the two trees' processes alternately.
--ngram N with --rounds (the table of profiles/ngram_ban_decode.txt): the arms are instead, for greedy decoding and for sampling at temperature
0.2 / top_k 50, "plain" (no ban: the fused loop; sampling with sampler="device"), "host-ban" (no_repeat_ngram_size=N with the list rule on
the host: the per-step host loop, and for sampling the host sampler, the only sampler that rule combines with) and, where this tree's
generate() has `ngram_ban`, "dev-ban" (the same N with ngram_ban="device": the fused loop, sampling with sampler="device")."""
import argparse, importlib, inspect, os, statistics, sys, time
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--new", type=int, default=33)
ap.add_argument("--sample", action="store_true")
ap.add_argument("--logprobs", action="store_true")
ap.add_argument("--rounds", type=int, default=0)
ap.add_argument("--ngram", type=int, default=0)
ap.add_argument("--batches", type=str, default="1,16")
ap.add_argument("--tree", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
a = ap.parse_args()
root = os.path.abspath(a.tree)
sys.path.insert(0, root)
import bench
assert os.path.dirname(os.path.abspath(bench.__file__)) == root, bench.__file__
dev = "cuda:0"
model, cfg = bench.build_model(336, dev)
SAMPLE = dict(do_sample=True, temperature=0.2, top_k=50, sampler="device")
LOGPROBS = dict(output_logprobs=True, return_dict_in_generate=True)


def timed(ids, images, n, kw):
    """(seconds of prefill + 1 token, seconds per further token) from a 1-token and an n-token generate()."""
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.generate(input_ids=ids, images=images, max_new_tokens=1, use_cache=True, **kw)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    model.generate(input_ids=ids, images=images, max_new_tokens=n, use_cache=True, **kw)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    return t1 - t0, ((t2 - t1) - (t1 - t0)) / max(n - 1, 1)


if a.rounds > 0:
    gen = importlib.import_module("u-llava_amd.modeling_core").UllavaCoreForCausalLM.generate
    arms = [("greedy", dict(do_sample=False)), ("device", SAMPLE)]
    if a.ngram > 0:
        ban = dict(no_repeat_ngram_size=a.ngram)
        arms = [("greedy/plain", dict(do_sample=False)), ("greedy/host-ban", dict(do_sample=False, **ban)),
                ("sample/plain", SAMPLE), ("sample/host-ban", dict(SAMPLE, sampler=None, **ban))]
        if "ngram_ban" in inspect.signature(gen).parameters:
            arms[2:2] = [("greedy/dev-ban", dict(do_sample=False, ngram_ban="device", **ban))]
            arms.append(("sample/dev-ban", dict(SAMPLE, ngram_ban="device", **ban)))
    elif "output_logprobs" in inspect.signature(gen).parameters:
        arms = [(name + sfx, dict(kw, **extra)) for name, kw in arms for sfx, extra in (("/off", {}), ("/on", LOGPROBS))]
    with torch.no_grad():
        for batch in (int(b) for b in a.batches.split(",")):
            images, ids, mask = bench.make_inputs(cfg, batch, 64, dev, 0)
            res = {name: [] for name, _ in arms}
            for rnd in range(a.rounds + 1):        # round 0: warm-up (allocator, packed weights)
                for name, kw in arms:
                    torch.manual_seed(1)
                    t = timed(ids, images, a.new, dict(kw, eos_token_id=-1))[1] * 1e3
                    if rnd:
                        res[name].append(t)
            for name, _ in arms:
                print(f"batch {batch:2d} {name:15s}: " + " ".join(f"{x:.3f}" for x in res[name]) +
                      f"  median {statistics.median(res[name]):.3f} ms/token", flush=True)
    sys.exit(0)

images, ids, mask = bench.make_inputs(cfg, a.batch, 64, dev, 0)
kw = dict(SAMPLE) if a.sample else dict(do_sample=False)
if a.logprobs:
    kw.update(LOGPROBS)
with torch.no_grad():
    for n in (2, a.new):            # warm-up (allocator, packed weights), then the timed run
        prefill, per_tok = timed(ids, images, n, kw)
wbytes = sum(p.numel() * p.element_size() for n_, p in model.named_parameters() if "vision" not in n_)
print(f"batch {a.batch}{' sampler=device' if a.sample else ' greedy'}{' output_logprobs' if a.logprobs else ''}: prefill+1 token {prefill * 1e3:.1f} ms; decode {per_tok * 1e3:.3f} ms/step = {a.batch / per_tok:.1f} tokens/s; "
      f"weights {wbytes / 1e9:.2f} GB -> {wbytes / per_tok / 1e12:.2f} TB/s ({wbytes / per_tok / 8e12 * 100:.1f} % of 8 TB/s)")
