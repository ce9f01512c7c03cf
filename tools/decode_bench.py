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
generate() has `ngram_ban`, "dev-ban" (the same N with ngram_ban="device": the fused loop, sampling with sampler="device").
--num-beams K with --rounds (the table of profiles/beam_decode.txt): for every batch B of --batches the arms are "greedy@B*K" (plain greedy
decoding at batch B * K: the same rows through the same GEMVs, the yardstick) and "beam" (generate(num_beams=K) at batch B), interleaved per
round; then the stand-alone times of ops.beam_step and KVCache.gather_rows (every row moving) at 8 and 64 generated tokens."""
import argparse, importlib, inspect, os, statistics, sys, time
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--new", type=int, default=33)
ap.add_argument("--sample", action="store_true")
ap.add_argument("--logprobs", action="store_true")
ap.add_argument("--rounds", type=int, default=0)
ap.add_argument("--ngram", type=int, default=0)
ap.add_argument("--num-beams", type=int, default=1)
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


def event_ms(fn, reps):
    """milliseconds per call of fn() from a pair of events around `reps` back-to-back calls, after three warm-up calls."""
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


if a.rounds > 0 and a.num_beams > 1:
    pk = importlib.import_module("u-llava_amd")
    G, ops, KV = (importlib.import_module("u-llava_amd." + n) for n in ("generation", "ops", "kv_cache"))
    K = a.num_beams
    with torch.no_grad():
        for batch in (int(b) for b in a.batches.split(",")):
            arms = [(f"greedy@{batch * K}", bench.make_inputs(cfg, batch * K, 64, dev, 0), dict(do_sample=False)),
                    (f"beam K={K}", bench.make_inputs(cfg, batch, 64, dev, 0), dict(num_beams=K))]
            res = {name: [] for name, _, _ in arms}
            for rnd in range(a.rounds + 1):        # round 0: warm-up
                for name, (images, ids, mask), kw in arms:
                    t = timed(ids, images, a.new, dict(kw, eos_token_id=-1))[1] * 1e3
                    if rnd:
                        res[name].append(t)
            for name, _, _ in arms:
                print(f"batch {batch:2d} {name:12s}: " + " ".join(f"{x:.3f}" for x in res[name]) + f"  median {statistics.median(res[name]):.3f} ms/step",
                      flush=True)
            # the two new launches on their own, at the decode loop's shapes -- and greedy_step, which the yardstick runs and beams do not
            L0, H = 643, cfg.num_attention_heads
            V = cfg.vocab_size
            logits = torch.randn(batch, K, V, device=dev).to(model.dtype)
            live, alive = torch.ones(batch * K, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
            buf = torch.zeros(batch * K, L0 + a.new, dtype=torch.int64, device=dev)
            greedy = lambda: ops.greedy_step(logits.view(batch * K, V), live, None, 0, buf, L0 + 8, alive)   # noqa: E731
            # one more beam run that records every step's parents: the share of rows a step really moves
            moved_rows, inner = [], KV.KVCache.gather_rows
            KV.KVCache.gather_rows = lambda c, parent, p0, p1: (moved_rows.append((parent.clone(), p1 - p0)), inner(c, parent, p0, p1))[1]
            model.generate(input_ids=arms[1][1][1], images=arms[1][1][0], max_new_tokens=a.new, use_cache=True, num_beams=K, eos_token_id=-1)
            KV.KVCache.gather_rows = inner
            # ... the same gathers again on their own (the exact stand-alone cost of the run's reorders), and the run without them
            # (wrong ids, the same launches otherwise): what the gathers cost inside the loop
            replay_cache = KV.KVCache(cfg.num_hidden_layers, batch * K, H, cfg.hidden_size // H, L0 + a.new + 2, dev, model.dtype)
            replay = event_ms(lambda: [replay_cache.gather_rows(p, L0, L0 + n) for p, n in moved_rows], 5) / max(a.new - 1, 1)
            del replay_cache
            KV.KVCache.gather_rows = lambda c, parent, p0, p1: None
            nog = statistics.median(timed(arms[1][1][1], arms[1][1][0], a.new, dict(num_beams=K, eos_token_id=-1))[1] * 1e3 for _ in range(3))
            KV.KVCache.gather_rows = inner
            print(f"batch {batch:2d} K {K}: the run's own gathers replayed stand-alone {replay:.4f} ms/step; beam without the gathers {nog:.3f} ms/step", flush=True)
            ident = torch.arange(batch * K, dtype=torch.int32, device=dev)
            share = [(float((p != ident).float().mean()), n) for p, n in moved_rows]
            print(f"batch {batch:2d} K {K}: greedy_step {event_ms(greedy, 50):.4f} ms; the beam run of {a.new} tokens gathered at {len(share)} steps, "
                  f"mean share of rows moved {statistics.mean(x for x, _ in share):.3f}, mean of share * generated positions "
                  f"{statistics.mean(x * n for x, n in share):.2f}", flush=True)
            for gen_tok in (8, 64):
                st = G.BeamState(torch.zeros(batch, L0, dtype=torch.int64, device=dev), K, a.new + 64, 0)
                st.run_sc.copy_(-torch.rand(batch, K, device=dev).cumsum(1))
                out, pout = torch.empty_like(st.run), torch.empty_like(st.pool)
                cv = torch.empty(batch * K * ops.BEAM_MAX_CAND, device=dev)
                ct, par, go = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (batch * K * ops.BEAM_MAX_CAND, batch * K, 1))
                eos = torch.tensor([2], device=dev)
                step = lambda: ops.beam_step(logits, None, st.run, out, st.pool, pout, st.run_sc, st.pool_sc, st.pool_len, st.fin, st.open, eos, 0, L0,  # noqa: E731
                                             L0 + gen_tok, 1.0, 1.0, False, cv, ct, par, go)
                cache = KV.KVCache(cfg.num_hidden_layers, batch * K, H, cfg.hidden_size // H, L0 + 66, dev, model.dtype)
                cycle = torch.tensor([b * K + (k + 1) % K for b in range(batch) for k in range(K)], dtype=torch.int32, device=dev)
                gather = lambda: cache.gather_rows(cycle, L0, L0 + gen_tok)                             # noqa: E731
                moved = 2 * cfg.num_hidden_layers * batch * K * cfg.hidden_size * gen_tok * cache.k[0].element_size()
                print(f"batch {batch:2d} K {K} at {gen_tok:2d} generated tokens: beam_step {event_ms(step, 50):.4f} ms; gather_rows (every row moves, "
                      f"{moved / 1e6:.0f} MB of K rows + V^T blocks each way, through the scratch) {event_ms(gather, 20):.4f} ms", flush=True)
                del cache
    sys.exit(0)

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
