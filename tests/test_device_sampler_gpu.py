"""GPU: the on-device sampler (ops.sample_step, generate(sampler="device"), evaluate(sampler="device")).

The yardstick is always the host path -- `sampling_probs` + `torch.multinomial` on the same logits with the same seed -- never the new
kernel.  Tokens must be equal on every row the gate of test_device_sampler_cpu.robust_rows calls robust (an fp64 restatement decides
that from the logits and the noise alone), and at most 5 % of the rows of a setting may be non-robust."""
import os
import sys

import pytest
import torch

from helpers import fixture_sd, load_fixture, pkg
from test_device_sampler_cpu import MAX_NON_ROBUST, SETTINGS, gate_logits, robust_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # bench.py (the LLaMA-7B builder)


def _noise(shape, seed):
    torch.manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32, device=DEV).exponential_()


def _host_tokens(logits_d, T, k, p, seed):
    """What generate()'s host path draws from these last-step logits under this seed."""
    MC = pkg("modeling_core")
    torch.manual_seed(seed)
    return torch.multinomial(MC.sampling_probs(logits_d.float(), T, k, p), 1).squeeze(1)


def _device_tokens(logits_d, T, k, p, seed):
    ops = pkg("ops")
    B = logits_d.shape[0]
    live = torch.ones(B, dtype=torch.int32, device=DEV)
    seq = torch.full((B, 2), -1, dtype=torch.int64, device=DEV)
    alive = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.sample_step(logits_d, _noise(tuple(logits_d.shape), seed), T, k, p, live, None, None, seq, 1, alive)
    assert int(alive) == B and bool((seq[:, 0] == -1).all())
    return seq[:, 1]


def _check_against_host(logits_d, T, k, p, seed, what):
    want = _host_tokens(logits_d, T, k, p, seed).cpu()
    got = _device_tokens(logits_d, T, k, p, seed).cpu()
    ok, tok64 = robust_rows(logits_d.float().cpu(), _noise(tuple(logits_d.shape), seed).cpu(), T, k, p)
    R = logits_d.shape[0]
    print(f"{what} T={T} top_k={k} top_p={p}: {int((~ok).sum())} of {R} rows non-robust; host != fp64 on {int((want != tok64)[ok].sum())} robust rows, "
          f"device != host on {int((got != want)[ok].sum())} robust rows and {int((got != want).sum())} of all rows")
    assert bool(((got >= 0) & (got < logits_d.shape[1])).all())
    assert float((~ok).float().mean()) <= MAX_NON_ROBUST, "too many non-robust rows"
    assert torch.equal(want[ok], tok64[ok]), "the host path disagrees with its fp64 restatement on robust rows"
    assert torch.equal(got[ok], want[ok]), "the device sampler draws other tokens than the host path on robust rows"


def test_multinomial_is_argmax_of_probs_over_exponential_noise_on_the_gpu():
    """The kernel's step 4 rests on this: with one sample per row torch.multinomial draws exponential noise of the probabilities' shape
    from the generator and returns argmax(probs / noise).  A torch upgrade that changes it must be noticed here."""
    torch.manual_seed(0)
    p = torch.rand(4, 32064, device=DEV).softmax(-1)
    torch.manual_seed(5)
    a = torch.multinomial(p, 1).squeeze(1)
    b = (p / _noise((4, 32064), 5)).argmax(-1)
    assert torch.equal(a, b)
    torch.manual_seed(6)                                         # two draws in a row: the second starts where the first noise ended
    a1, a2 = torch.multinomial(p, 1).squeeze(1), torch.multinomial(p, 1).squeeze(1)
    torch.manual_seed(6)
    q1 = torch.empty(4, 32064, device=DEV).exponential_()
    q2 = torch.empty(4, 32064, device=DEV).exponential_()
    assert torch.equal(a1, (p / q1).argmax(-1)) and torch.equal(a2, (p / q2).argmax(-1))


@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_kernel_draws_the_host_paths_tokens_bf16_rows(T, k, p):
    logits = gate_logits(512, 32064, 1).to(DEV)
    _check_against_host(logits, T, k, p, 21, "bf16")
    again = _device_tokens(logits, T, k, p, 21)
    assert torch.equal(again, _device_tokens(logits, T, k, p, 21)), "two launches on the same inputs drew different tokens"


@pytest.mark.parametrize("T,k,p", [(0.2, 50, 0.7), (1.0, 0, 0.9), (0.7, 0, None)])
def test_kernel_other_dtypes_strided_rows_and_odd_vocabulary(T, k, p):
    R = 128
    _check_against_host(gate_logits(R, 32064, 2, torch.float16).to(DEV), T, k, p, 22, "fp16")
    _check_against_host(gate_logits(R, 32064, 3, torch.float32).to(DEV), T, k, p, 23, "fp32")
    three = gate_logits(R * 3, 32064, 4).to(DEV).view(R, 3, 32064)
    _check_against_host(three[:, -1], T, k, p, 24, "bf16 strided rows")              # out.logits[:, -1] of a prefill
    for V in (32011, 1003, 100):                                                    # not multiples of 8: rows off the 16-byte grid, scalar tails
        for dt in (BF, torch.float32):
            _check_against_host(gate_logits(R, V, 5, dt).to(DEV), T, k, p, 25, f"{dt} V={V}")


def test_kernel_ties_at_the_top_k_threshold_stay():
    """`scores < kth` keeps every score equal to the k-th largest: with 80 tokens tied at the top and top_k = 50 all 80 stay in the race."""
    V = 32064
    logits = torch.full((64, V), -4.0)
    cols = torch.arange(80) * 397 + 5
    logits[:, cols] = 3.0
    ld = logits.to(BF).to(DEV)
    want, got = _host_tokens(ld, 1.0, 50, None, 31).cpu(), _device_tokens(ld, 1.0, 50, None, 31).cpu()
    assert torch.equal(got, want) and bool(torch.isin(got, cols).all())
    assert len(set(got.tolist())) > 20 and bool((got > int(cols[49])).any())       # tokens beyond the 50th tied column are drawn too


def test_kernel_bookkeeping_matches_torch():
    """Pad fill of finished rows, EOS tracking, append, the unfinished-row counter: as test_greedy_step_kernel_matches_torch_bookkeeping,
    with top_k = 1 so that the drawn token is the row's maximum."""
    ops = pkg("ops")
    g = torch.Generator().manual_seed(9)
    B, V, L = 7, 32011, 12
    for dt in (BF, torch.float16, torch.float32):
        logits = (torch.randn(B, 3, V, generator=g) * 2).to(dt)
        winners = torch.tensor([100, 2, 7, 31000, 32010, 0, 555])
        logits[torch.arange(B), -1, winners] = 40.0
        eos = torch.tensor([2, 100], dtype=torch.int64)
        unfinished = torch.tensor([1, 1, 0, 1, 1, 0, 1], dtype=torch.int32)
        seq = torch.full((B, L), -7, dtype=torch.int64)
        pad = 31999
        want_tok = torch.where(unfinished.bool(), winners, torch.full_like(winners, pad))
        want_unf = unfinished.bool() & ~torch.isin(want_tok, eos)
        ld = logits.to(DEV)
        noise = _noise((B, V), 3)
        u_d, s_d, alive = unfinished.to(DEV), seq.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.sample_step(ld[:, -1], noise, 0.7, 1, 0.9, u_d, eos.to(DEV), pad, s_d, 4, alive)
        assert torch.equal(s_d[:, 4].cpu(), want_tok) and torch.equal(u_d.cpu().bool(), want_unf) and int(alive) == int(want_unf.sum()) == 3
        assert bool((s_d.cpu()[:, :4] == -7).all()) and bool((s_d.cpu()[:, 5:] == -7).all())       # only column `pos` is written
        # no pad id: finished rows keep their draw; no EOS list: nothing finishes
        u2, s2, a2 = unfinished.to(DEV), seq.to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.sample_step(ld[:, -1], noise, 0.7, 1, None, u2, None, None, s2, 0, a2)
        assert torch.equal(s2[:, 0].cpu(), winners) and torch.equal(u2.cpu(), unfinished) and int(a2) == int(unfinished.sum())


def test_kernel_entry_refusals():
    ops = pkg("ops")
    B = 2
    live, seq, alive = torch.ones(B, dtype=torch.int32, device=DEV), torch.zeros(B, 4, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    V = ops.SAMPLE_MAX_V + 8
    with pytest.raises(RuntimeError, match="ull_sample_step failed"):              # ULL_ERR_SHAPE: the row does not fit the LDS
        ops.sample_step(torch.zeros(B, V, dtype=BF, device=DEV), torch.ones(B, V, device=DEV), 1.0, 50, None, live, None, None, seq, 0, alive)
    lg = torch.zeros(B, 128, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="noise"):
        ops.sample_step(lg, torch.ones(B, 127, device=DEV), 1.0, 50, None, live, None, None, seq, 0, alive)
    with pytest.raises(RuntimeError, match="noise"):
        ops.sample_step(lg, torch.ones(B, 128, device=DEV, dtype=torch.float64), 1.0, 50, None, live, None, None, seq, 0, alive)
    with pytest.raises(ValueError, match="temperature"):
        ops.sample_step(lg, torch.ones(B, 128, device=DEV), 0.0, 50, None, live, None, None, seq, 0, alive)
    assert int(alive) == 0 and bool((seq == 0).all())


# ---- model level ------------------------------------------------------------------------------------------------------------------------
class _Tally:
    compared = 0
    total = 0


class _Total(_Tally):
    def add(self, what, tally):
        print(f"{what}: {tally.compared} of {tally.total} row-steps compared ({100.0 * tally.compared / tally.total:.1f} %)")
        self.compared += tally.compared
        self.total += tally.total


def _host_and_device(m, seed, tally, **kw):
    """generate(sampler=None) and generate(sampler="device") under the same seed.  The host run's per-step logits are captured by wrapping
    `sampling_probs`, its noise is regenerated from the same seed, and every row's ids are compared up to the first step at which that row
    is non-robust (from there on the two runs may feed it different prefixes; the rows of a batch do not see each other, and a step draws
    B x V noise values whatever was drawn before).  Returns (host ids, device ids, fully compared)."""
    MC = pkg("modeling_core")
    rec, orig = [], MC.sampling_probs

    def wrap(logits, *a, **k):
        rec.append(logits.detach().float().cpu())
        return orig(logits, *a, **k)

    MC.sampling_probs = wrap
    try:
        torch.manual_seed(seed)
        host = m.generate(sampler=None, **kw)
    finally:
        MC.sampling_probs = orig
    torch.manual_seed(seed)
    dev = m.generate(sampler="device", **kw)
    hs, ds = (host.sequences, dev.sequences) if kw.get("return_dict_in_generate") else (host, dev)
    L0 = kw["input_ids"].shape[1]
    n = hs.shape[1] - L0
    assert len(rec) == n
    eos = kw.get("eos_token_id", m.config.eos_token_id)
    eos = [] if eos is None else ([eos] if isinstance(eos, int) else list(eos))
    torch.manual_seed(seed)
    B = hs.shape[0]
    first_bad = [n] * B
    for t in range(n):
        q = torch.empty(rec[t].shape, dtype=torch.float32, device=DEV).exponential_().cpu()
        ok, _ = robust_rows(rec[t], q, kw.get("temperature", 1.0), kw.get("top_k", 50), kw.get("top_p"))
        for b in range(B):
            live = not any(int(x) in eos for x in hs[b, L0:L0 + t])
            if live and not bool(ok[b]) and first_bad[b] == n:
                first_bad[b] = t
    for b in range(B):
        fb = min(first_bad[b], ds.shape[1] - L0)                # (a row that went its own way may end the device run at another length)
        tally.total += n
        tally.compared += fb
        assert torch.equal(hs[b, :L0 + fb], ds[b, :L0 + fb]), (seed, b, fb, hs.tolist(), ds.tolist())
    full = all(f == n for f in first_bad)
    if full:
        assert torch.equal(hs, ds), (seed, hs.tolist(), ds.tolist())
    return host, dev, full


def _tiny_core_on_gpu(dt, text_only=False):
    """text_only: no multimodal ids in the config, so that a SAMPLED id in 90 .. 95 is an ordinary token (with them, a drawn image-start id
    without its end trips the reference's start / end count assert when use_cache=False embeds the whole sequence again)."""
    fx = load_fixture("g1_core_tiny_bf16.pt")
    C, M = pkg("configuration"), pkg("modeling_core")
    cd = fx["cfg"]
    cfg = C.UllavaCoreConfig(vision_config=cd["vision_config"], vision_hidden_layer=cd["vision_hidden_layer"], projector_type=cd["projector_type"],
                             projector_from_scratch=bool(cd.get("projector_from_scratch", False)),
                             mm_token_ids=None if text_only else cd["mm_token_ids"],
                             vocab_size=cd["vocab_size"], hidden_size=cd["hidden_size"], intermediate_size=cd["intermediate_size"],
                             num_hidden_layers=cd["num_hidden_layers"], num_attention_heads=cd["num_attention_heads"],
                             rms_norm_eps=cd["rms_norm_eps"], rope_theta=cd["rope_theta"])
    m = M.UllavaCoreForCausalLM(cfg, device=DEV, dtype=dt)
    m.load_state_dict(fixture_sd(fx, dt), strict=True)
    return fx, m


def _text_ids(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, 90, (B, L), generator=g).to(DEV)     # text ids: below the fixture's multimodal ids


def _case_tiny_generate(dt, use_cache, total):
    """A left-padded batch whose rows hit EOS at different steps, a stopping criterion, max_new_tokens off the 8-step check grid."""
    fx, m = _tiny_core_on_gpu(dt, text_only=True)
    tally = _Tally()
    ids = torch.cat([torch.cat([torch.zeros(1, 5, dtype=torch.long, device=DEV), _text_ids(1, 9, 1)], dim=1), _text_ids(2, 14, 2)])
    mask = torch.ones_like(ids)
    mask[0, :5] = 0
    for seed in (1, 2, 3, 4):
        for T, k, p in ((0.2, 50, 0.7), (1.0, 50, 0.9), (0.7, 0, None)):
            kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=13, do_sample=True, temperature=T, top_k=k, top_p=p, use_cache=use_cache,
                      eos_token_id=-1)
            host, _, _ = _host_and_device(m, seed, tally, **kw)
            # rows that finish at different steps: the tokens the host run drew for row 0 at step 2 and row 1 at step 6 become EOS ids
            L0 = ids.shape[1]
            kw["eos_token_id"] = [int(host[0, L0 + 2]), int(host[1, L0 + 6])]
            kw["pad_token_id"] = 0
            _host_and_device(m, seed, tally, **kw)
    # a stopping criterion (checked every step)
    stop = lambda seq, scores: torch.tensor(seq.shape[1] >= ids.shape[1] + 5)
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=11, do_sample=True, temperature=0.2, top_p=0.7, use_cache=use_cache, eos_token_id=-1,
              stopping_criteria=[stop])
    host, dev, _ = _host_and_device(m, 5, tally, **kw)
    assert host.shape[1] == dev.shape[1] == ids.shape[1] + 5
    total.add(f"tiny {dt} use_cache={use_cache}", tally)
    # determinism, and temperature 0 / do_sample=False are the greedy fused path whatever the sampler
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=13, do_sample=True, temperature=1.0, top_p=0.9, use_cache=use_cache, eos_token_id=-1,
              sampler="device")
    torch.manual_seed(9)
    a = m.generate(**kw)
    torch.manual_seed(9)
    assert torch.equal(a, m.generate(**kw))
    g = dict(input_ids=ids, attention_mask=mask, max_new_tokens=6, use_cache=use_cache, eos_token_id=-1)
    want = m.generate(do_sample=False, **g)
    assert torch.equal(want, m.generate(do_sample=False, sampler="device", **g))
    assert torch.equal(want, m.generate(do_sample=True, temperature=0, sampler="device", **g))


def _case_tiny_fp8(fp8_weights, fp8_cache, total):
    fx, m = _tiny_core_on_gpu(BF)
    if fp8_weights:
        m.quantize_weights("fp8_e4m3")
    tally = _Tally()
    ids = torch.cat([torch.cat([torch.zeros(1, 7, dtype=torch.long, device=DEV), _text_ids(1, 60, 6)], dim=1), _text_ids(1, 67, 7)])
    mask = torch.ones_like(ids)
    mask[0, :7] = 0
    for seed in (1, 2, 3):
        for T, k, p in ((0.2, 50, 0.7), (1.0, 50, 0.9)):
            kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=11, do_sample=True, temperature=T, top_k=k, top_p=p, use_cache=True,
                      eos_token_id=-1)
            if fp8_cache:
                kw["kv_cache_dtype"] = "fp8_e4m3"
            _host_and_device(m, seed, tally, **kw)
    total.add(f"tiny fp8 weights {fp8_weights}, fp8 cache {fp8_cache}", tally)


def _case_tiny_evaluate(total):
    """evaluate(sampler="device"): ids, masks and boxes equal evaluate(sampler=None) under the same seed."""
    from test_fp8_weights_gpu import _tiny_full
    MC = pkg("modeling_core")
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    L0 = fx["input_ids"].shape[1]
    full, tally = 0, _Tally()
    for seed in (1, 2, 3, 4):
        rec, orig = [], MC.sampling_probs

        def wrap(logits, *a, **k):
            rec.append(logits.detach().float().cpu())
            return orig(logits, *a, **k)

        MC.sampling_probs = wrap
        try:
            torch.manual_seed(seed)
            ids_h, masks_h, boxes_h = model.evaluate(*args, max_new_tokens=7, temperature=0.2, top_p=0.7)
        finally:
            MC.sampling_probs = orig
        torch.manual_seed(seed)
        ids_d, masks_d, boxes_d = model.evaluate(*args, max_new_tokens=7, temperature=0.2, top_p=0.7, sampler="device")
        torch.manual_seed(seed)
        first_bad = len(rec)
        for t, lg in enumerate(rec):
            q = torch.empty(lg.shape, dtype=torch.float32, device=DEV).exponential_().cpu()
            if not bool(robust_rows(lg, q, 0.2, 50, 0.7)[0].all()):
                first_bad = t
                break
        tally.total += len(rec)
        tally.compared += first_bad
        assert torch.equal(ids_h[:, :L0 + first_bad], ids_d[:, :L0 + first_bad])
        if first_bad == len(rec):
            full += 1
            assert torch.equal(ids_h, ids_d)
            assert len(masks_h) == len(masks_d) and all(torch.equal(x, y) for x, y in zip(masks_h, masks_d))
            assert len(boxes_h) == len(boxes_d) and all(torch.equal(x, y) for x, y in zip(boxes_h, boxes_d))
    total.add(f"tiny evaluate ({full} of 4 runs in full)", tally)
    assert full >= 1, "no evaluate run was robust at every step: masks and boxes were never compared"


def _case_llama7b(total):
    """LLaMA-7B (random init), the reference's settings (temperature 0.2, top_k 50, top_p 0.7), 16 tokens at batch 1 and batch 4."""
    import bench
    model, cfg = bench.build_model(336, DEV, seed=3)
    tally = _Tally()
    for B in (1, 4):
        vis, ids, _ = bench.make_inputs(cfg, B, 64, DEV, B)
        kw = dict(input_ids=ids, images=vis, max_new_tokens=16, do_sample=True, temperature=0.2, top_k=50, top_p=0.7, use_cache=True, eos_token_id=-1)
        for seed in (17, 18, 19):
            _host_and_device(model, seed, tally, **kw)
        torch.manual_seed(5)
        a = model.generate(sampler="device", **kw)
        torch.manual_seed(5)
        assert torch.equal(a, model.generate(sampler="device", **kw))
    total.add("LLaMA-7B", tally)


def test_generate_and_evaluate_device_sampler_equals_host_sampler():
    """Model level: sampler="device" against sampler=None under the same seed -- tiny models in bf16 / fp16 / fp32 with and without cache
    (left-padded batch, rows that hit EOS at different steps, a stopping criterion, 13 and 11 new tokens), fp8 weights and the fp8 KV cache,
    `evaluate` ids / masks / boxes, and LLaMA-7B at full depth.  Every row is compared up to its first non-robust host step, and at least
    90 % of all row-steps of all these runs must be compared.

    The bar is on the pool, not on each case.  What is compared depends on the host run and the gate alone, never on the device sampler:
    measured on the host path over 24-40 seeds per case, 1.25 % of the tiny fp8 model's steps at 0.2 / 50 / 0.7 and 1.5-2.1 % of LLaMA-7B's
    are non-robust (tie groups of bf16 scores on the nucleus boundary), so an n-step row is compared over (1 - (1 - r)^n) / (n r) of its
    steps on average: 93 % at n = 11, r = 1.25 %; 86-89 % at n = 16, r = 1.5-2.1 % (measured: 89 % and 83-90 %).  The 16-token LLaMA-7B
    case therefore sits below 90 % on its own whatever the sampler does; each case's own count is printed."""
    total = _Total()
    for use_cache in (False, True):
        for dt in (BF, torch.float16, torch.float32):
            _case_tiny_generate(dt, use_cache, total)
    for fp8_weights, fp8_cache in ((True, False), (False, True), (True, True)):
        _case_tiny_fp8(fp8_weights, fp8_cache, total)
    _case_tiny_evaluate(total)
    _case_llama7b(total)
    print(f"model level: {total.compared} of {total.total} row-steps compared")
    assert total.compared >= 0.9 * total.total
