"""GPU: prompt-lookup speculative decoding -- ops.spec_step against the host restatement (`prompt_lookup_candidates`, torch argmax,
`sampling_probs`), and generate(prompt_lookup_num_tokens=) on the tiny fixture model against a host-driven loop written here.

The yardstick is never the new kernel: the expected ids and record of a step are worked out on the host from the same logits.  Sampled
rows are compared under the gate of test_device_sampler_cpu.robust_rows (the device and the host sampler sum in different fp32 orders), as
tests/test_device_sampler_gpu.py does."""
import pytest
import torch

from helpers import pkg
from test_device_sampler_cpu import robust_rows
from test_device_sampler_gpu import _tiny_core_on_gpu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16


# ---- the host restatement of one step -------------------------------------------------------------------------------------------------
def host_step(row, drafts, tokens, n_max, k, ng, eos):
    """row: the valid ids; drafts: this step's drafts; tokens: the 1 + d picks -> (new row, record (emitted, finished, d'), next drafts)."""
    MC = pkg("modeling_core")
    a = 0
    while a < len(drafts) and tokens[a] == drafts[a]:
        a += 1
    emit = tokens[:a + 1][:n_max - len(row)]
    fin = 0
    for j, t in enumerate(emit):
        if t in eos:
            emit, fin = emit[:j + 1], 1
            break
    row = row + emit
    nxt = [] if fin else MC.prompt_lookup_candidates(row, k, ng, eos, n_max - len(row) - 1)
    return row, (len(emit), fin, len(nxt)), nxt, a


def run_step(logits, row, drafts, n_max, k, ng, eos, noise=None, T=1.0, top_k=None, top_p=None):
    """ops.spec_step on a fresh buffer of n_max + k ids, -1 where nothing was put -> (the buffer as a list, record, picks)."""
    ops = pkg("ops")
    L = n_max + k
    buf = torch.full((1, L), -1, dtype=torch.int64, device=DEV)
    buf[0, :len(row) + len(drafts)] = torch.tensor(row + drafts)
    picks = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    rec = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    eos_t = torch.tensor(eos, dtype=torch.int64, device=DEV) if eos else None
    ops.spec_step(logits, noise, T, top_k, top_p, buf, len(row), len(drafts), n_max, eos_t, k, ng, picks, rec)
    return buf[0].tolist(), tuple(rec.tolist()), picks.tolist()


def check_step(logits, row, drafts, n_max, k, ng, eos, what, tokens=None):
    tokens = logits.float().argmax(-1).tolist() if tokens is None else tokens
    want_row, want_rec, want_next, a = host_step(row, drafts, tokens, n_max, k, ng, eos)
    buf, rec, picks = run_step(logits, row, drafts, n_max, k, ng, eos)
    print(f"{what}: n={len(row)} d={len(drafts)} accepted={a} record={rec} want={want_rec}")
    assert picks[:1 + len(drafts)] == tokens, what
    assert rec == want_rec, (what, rec, want_rec)
    n2 = len(want_row)
    assert buf[:n2] == want_row and buf[n2:n2 + len(want_next)] == want_next, (what, buf[:n2 + 16], want_row, want_next)
    assert all(x == -1 for x in buf[max(n2 + len(want_next), len(row) + len(drafts)):]), what      # nothing else is written
    return a, rec


def peaked(R, V, winners, dtype, seed=0):
    """[R, V] random logits whose row i has its maximum at winners[i]."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(R, V, generator=g) * 2
    lg[torch.arange(R), torch.tensor(winners)] = 30.0
    return lg.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [BF, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V", [50, 32003])
def test_step_acceptance_cases(dtype, V):
    """d = 0 / 15 accepted / none / up to the middle, on a history that holds a match for the next draft."""
    ops = pkg("ops")
    g = torch.Generator().manual_seed(V)
    hist = torch.randint(3, 40, (70,), generator=g).tolist()
    row = hist + hist[:20]                                       # the trailing ids occurred before: the next lookup finds a draft
    # d = 0: the token is greedy_step's
    lg = (torch.randn(1, V, generator=g) * 3).to(dtype).to(DEV)
    a, rec = check_step(lg, row, [], 400, 15, 2, [], "d=0")
    seq = torch.full((1, 2), -1, dtype=torch.int64, device=DEV)
    ops.greedy_step(lg, torch.ones(1, dtype=torch.int32, device=DEV), None, None, seq, 0, torch.zeros(1, dtype=torch.int32, device=DEV))
    buf, _, _ = run_step(lg, row, [], 400, 15, 2, [])
    assert buf[len(row)] == int(seq[0, 0]) and rec[0] == 1
    # 15 drafts, all accepted: 16 tokens emitted (the bonus token continues the repetition, so the next draft is found again)
    drafts = hist[20:35]
    a, rec = check_step(peaked(16, V, drafts + [hist[35]], dtype), row, drafts, 400, 15, 2, [], "all accepted")
    assert a == 15 and rec[0] == 16 and rec[2] == 15
    # none accepted
    a, rec = check_step(peaked(16, V, [41] * 16, dtype), row, drafts, 400, 15, 2, [], "none accepted")
    assert a == 0 and rec[0] == 1
    # accepted up to the middle (the pick at row 7 differs from draft 7)
    win = drafts[:7] + [42] + drafts[8:] + [hist[35]]
    a, rec = check_step(peaked(16, V, win, dtype), row, drafts, 400, 15, 2, [], "middle")
    assert a == 7 and rec[0] == 8
    # rows of a larger logits tensor, 1 + d rows from its end (what generate() hands over)
    big = peaked(20, V, [0] * 4 + win, dtype)
    check_step(big[-16:], row, drafts, 400, 15, 2, [], "strided view")
    # random logits, nothing arranged
    check_step((torch.randn(6, V, generator=g) * 3).to(dtype).to(DEV), row, hist[20:25], 400, 5, 3, [7], "random")


def test_step_three_way_tie_takes_the_lowest_index():
    for V, cols in ((50, [44, 9, 30]), (32003, [32002, 31999, 17])):
        for dtype in (BF, torch.float16, torch.float32):
            lg = torch.full((3, V), -1.0)
            lg[:, cols] = 2.5
            lg[2, 5] = 2.5                                       # row 2: four-way, 5 is the lowest
            a, rec = check_step(lg.to(dtype).to(DEV), [1, 2, 3], [min(cols), min(cols)], 64, 4, 2, [], f"tie V={V}", tokens=[min(cols)] * 2 + [5])
            assert a == 2 and rec[0] == 3


def test_step_eos_and_max_new_tokens():
    V = 50
    row = [5, 6, 7, 8, 5, 6]
    drafts = [7, 8, 5, 6]
    # EOS at an accepted position: emission is cut after it, the row is finished, no further drafts
    a, rec = check_step(peaked(5, V, [7, 8, 5, 6, 9], BF), row, drafts, 64, 4, 2, [8], "EOS accepted")
    assert a == 4 and rec == (2, 1, 0)
    # EOS as the bonus token
    a, rec = check_step(peaked(5, V, [7, 8, 5, 6, 9], BF), row, drafts, 64, 4, 2, [3, 9], "EOS bonus")
    assert a == 4 and rec == (5, 1, 0)
    # EOS as the token that rejects a draft
    a, rec = check_step(peaked(5, V, [7, 9, 5, 6, 9], BF), row, drafts, 64, 4, 2, [9], "EOS rejecting")
    assert a == 1 and rec == (2, 1, 0)
    # an EOS id in the history cuts the next draft: [5, 6] -> 7, 8 with 8 an EOS id... (picks never emit it here)
    a, rec = check_step(peaked(1, V, [5], BF), [5, 6, 7, 8, 5, 6, 4], [], 64, 4, 1, [8], "EOS in the draft")
    assert rec == (1, 0, 2)                                      # trailing [5] -> continuation 6, 7, (8)
    # max_new_tokens cuts the emission: 2 ids of room, 5 picked; the EOS id behind the cut does not finish the row
    a, rec = check_step(peaked(5, V, [7, 8, 5, 6, 9], BF), row, drafts, len(row) + 2, 4, 2, [5], "max_new_tokens")
    assert a == 4 and rec == (2, 0, 0)
    # one id of room left after the step: limit = 0, no draft; two ids: a draft of one
    assert check_step(peaked(1, V, [7], BF), row, [], len(row) + 2, 4, 2, [], "limit 0")[1] == (1, 0, 0)
    assert check_step(peaked(1, V, [7], BF), row, [], len(row) + 3, 4, 2, [], "limit 1")[1] == (1, 0, 1)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025])
def test_step_lookup_over_history_lengths(n):
    """The block-wide scan at history lengths around the block size (n valid ids before the step; the scan runs over n + 1): the only
    match sits at the very start, at the very end, or nowhere."""
    V = 50
    for where in ("start", "end", "none", "random"):
        g = torch.Generator().manual_seed(n)
        if where == "random":
            row = torch.randint(0, 6, (n,), generator=g).tolist()
            tok = int(torch.randint(0, 6, (1,), generator=g))
        else:
            row = [10 + (i % 30) for i in range(n)]              # period 30: ids 10 .. 39
            tok = 45
            if where == "start":
                row[0] = 45
            elif where == "end" and n >= 2:
                row[n - 2] = 45
        for ng in (1, 2, 3):
            a, rec = check_step(peaked(1, V, [tok], BF), row, [], n + 40, 6, ng, [], f"n={n} {where} ng={ng}")
            if where == "start" and ng == 1 and n > 1:
                assert rec[2] == min(6, n)


SAMPLED = [(0.2, 50, 0.7), (1.0, 50, 0.7), (1.0, 0, None)]


@pytest.mark.parametrize("T,top_k,top_p", SAMPLED)
def test_step_sampled_form_against_sampling_probs(T, top_k, top_p):
    """noise fixed; the expected picks are argmax(sampling_probs / noise) row by row.  A step is compared when every row the outcome rests
    on is robust under the gate.  The gate admits up to 5 % non-robust rows (MAX_NON_ROBUST), so at least 0.95^16 = 44 % of 16-row steps
    and 0.95^4 = 81 % of 4-row steps are comparable; the bar below is the smaller one over the pool."""
    MC = pkg("modeling_core")
    compared = total = 0
    for V, dtype in ((50, BF), (32003, BF), (32003, torch.float16), (32003, torch.float32)):
        for seed, d in ((1, 0), (2, 3), (3, 3), (4, 15), (5, 15)):
            g = torch.Generator().manual_seed(100 * seed + V)
            lg = (torch.randn(1 + d, V, generator=g) * 2.5).to(dtype).to(DEV)
            torch.manual_seed(seed)
            noise = torch.empty((1 + d, V), dtype=torch.float32, device=DEV).exponential_()
            tokens = (MC.sampling_probs(lg.float(), T, top_k, top_p) / noise).argmax(-1).tolist()
            ok, _ = robust_rows(lg.float().cpu(), noise.cpu(), T, top_k, top_p)
            hist = torch.randint(3, 40, (90,), generator=g).tolist()
            drafts = [t if i % 5 != 4 else (t + 1) % V for i, t in enumerate(tokens[:d])]       # every fifth draft is wrong
            want_row, want_rec, want_next, a = host_step(hist, drafts, tokens, 300, 15, 2, [])
            total += 1
            if not bool(ok[:a + 1].all()):                       # rows behind the first rejection do not matter
                continue
            compared += 1
            buf, rec, picks = run_step(lg, hist, drafts, 300, 15, 2, [], noise=noise, T=T, top_k=top_k, top_p=top_p)
            assert picks[:a + 1] == tokens[:a + 1] and rec == want_rec, (V, dtype, seed, d, picks, tokens)
            assert buf[:len(want_row)] == want_row and buf[len(want_row):len(want_row) + len(want_next)] == want_next
    print(f"T={T} top_k={top_k} top_p={top_p}: {compared} of {total} steps compared")
    assert compared >= 0.44 * total


def test_step_entry_refusals():
    ops = pkg("ops")
    lg = torch.zeros(2, 64, dtype=BF, device=DEV)
    buf = torch.zeros(1, 32, dtype=torch.int64, device=DEV)
    picks, rec = torch.zeros(16, dtype=torch.int32, device=DEV), torch.full((3,), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="1 \\+ d"):
        ops.spec_step(lg, None, 1.0, None, None, buf, 4, 2, 20, None, 4, 2, picks, rec)
    lg3 = torch.zeros(3, 64, dtype=BF, device=DEV)
    for n, d, n_max, k, ng in ((0, 1, 20, 4, 2), (20, 1, 20, 4, 2), (31, 2, 32, 4, 2), (4, 1, 33, 4, 2), (4, 1, 20, 16, 2), (4, 1, 20, 4, 0)):
        with pytest.raises(RuntimeError, match="ull_spec_step failed"):
            ops.spec_step(lg if d == 1 else lg3, None, 1.0, None, None, buf, n, d, n_max, None, k, ng, picks, rec)
    with pytest.raises(RuntimeError, match="noise"):
        ops.spec_step(lg, torch.ones(2, 63, device=DEV), 1.0, None, None, buf, 4, 1, 20, None, 4, 2, picks, rec)
    assert rec.tolist() == [-1, -1, -1] and bool((buf == 0).all())


# ---- end to end on the tiny fixture model -------------------------------------------------------------------------------------------------
K, NG, NEW = 4, 2, 48


def _prompt():
    """A repetitive prompt of text ids: a random phrase of 11 ids, six times, and three more of its ids (69 ids: more than 64 cached
    positions from the first verify step on, so the fp8 cache's few-query attention runs)."""
    g = torch.Generator().manual_seed(3)
    phrase = torch.randint(3, 90, (11,), generator=g).tolist()
    return torch.tensor([phrase * 6 + phrase[:3]], device=DEV)


def _new_cache(m, L0, max_new, k, kv_dtype):
    """the cache generate() makes for this run."""
    MC = pkg("modeling_core")
    c = m.config
    return MC.KVCache(c.num_hidden_layers, 1, c.num_attention_heads, c.hidden_size // c.num_attention_heads, max(L0 + max_new + k + 1, 64), DEV,
                      m.dtype, kv_dtype=kv_dtype)


def host_loop(m, ids, max_new, k, ng, eos=(), kv_dtype=None, sample=None):
    """The speculative loop driven from the host: model.forward on the same chunks, torch argmax (or sampling_probs and the step's noise),
    the host restatement of the lookup, KVCache.truncate.  -> (ids, [(d, accepted)] per step, last-layer hidden states, robust per step)"""
    MC = pkg("modeling_core")
    row, L0 = ids[0].tolist(), ids.shape[1]
    n_max = L0 + max_new
    cache = _new_cache(m, L0, max_new, k, kv_dtype)
    drafts, steps, robust = [], [], []
    first = True
    while len(row) < n_max:
        chunk = torch.tensor([row if first else row[-1:] + drafts], device=DEV)
        out = m.forward(input_ids=chunk, past_key_values=cache, use_cache=True)
        first = False
        lg = out.logits[0, -(1 + len(drafts)):]
        if sample is None:
            tokens = lg.float().argmax(-1).tolist()
            ok = True
        else:
            T, top_k, top_p = sample
            noise = torch.empty(lg.shape, dtype=torch.float32, device=DEV).exponential_()
            tokens = (MC.sampling_probs(lg.float(), T, top_k, top_p) / noise).argmax(-1).tolist()
            ok = robust_rows(lg.float().cpu(), noise.cpu(), T, top_k, top_p)[0]
        row, rec, nxt, a = host_step(row, drafts, tokens, n_max, k, ng, list(eos))
        robust.append(True if sample is None else bool(ok[:a + 1].all()))
        steps.append((len(drafts), a))
        cache.truncate(len(row) - 1)
        drafts = nxt
        if rec[1]:
            break
    return row, steps, torch.cat(cache.last_hidden, dim=1), robust


_MODELS = {}


def _model(quant=None):
    if quant not in _MODELS:
        _, m = _tiny_core_on_gpu(BF, text_only=True)
        if quant:
            m.quantize_weights(quant)
        _MODELS[quant] = m
    return _MODELS[quant]


@pytest.mark.parametrize("kv_dtype,quant", [(None, None), ("fp8_e4m3", None), (None, "fp8_e4m3")], ids=["bf16", "fp8-cache", "fp8-weights"])
def test_generate_equals_the_host_driven_loop(kv_dtype, quant):
    m = _model(quant)
    ids = _prompt()
    want, steps, hidden, _ = host_loop(m, ids, NEW, K, NG, kv_dtype=kv_dtype)
    print("steps (drafts, accepted):", steps)
    assert any(a > 0 for d, a in steps), "no step of the host-driven loop accepted a draft"
    assert any(a < d for d, a in steps), "no step of the host-driven loop rejected a draft"
    out = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=K, kv_cache_dtype=kv_dtype,
                     output_hidden_states=True, return_dict_in_generate=True)
    assert out.sequences[0].tolist() == want and out.sequences.shape == (1, ids.shape[1] + NEW)
    # e. hidden states: the accepted positions only, equal to the host loop's
    h = out.hidden_states[-1][-1]
    assert h.shape[1] == out.sequences.shape[1] - 1 and torch.equal(h, hidden)
    assert torch.equal(m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=K,
                                  kv_cache_dtype=kv_dtype), out.sequences)


def test_generate_eos_list_stopping_criteria_and_ngram_size():
    m = _model()
    ids = _prompt()
    L0 = ids.shape[1]
    base, _, _, _ = host_loop(m, ids, NEW, K, NG)
    eos = [int(base[L0 + 9]), int(base[L0 + 20])]                # an EOS list: the run ends at the first of them it emits
    want, steps, _, _ = host_loop(m, ids, NEW, K, NG, eos=eos)
    got = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=eos, prompt_lookup_num_tokens=K)
    assert got[0].tolist() == want and want[-1] in eos and not any(t in eos for t in want[L0:-1]) and len(want) <= L0 + 10
    # a stopping criterion is asked once per step, on the valid ids: it fires at the end of the step that passes its mark
    seen = []

    def stop(seq, scores):
        seen.append(seq.shape[1])
        return torch.tensor(seq.shape[1] >= L0 + 12)

    got = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=K, stopping_criteria=[stop])
    assert got[0].tolist() == base[:got.shape[1]] and L0 + 12 <= got.shape[1] <= L0 + 12 + K and seen[-1] == got.shape[1]
    assert all(b - a <= K + 1 for a, b in zip(seen, seen[1:]))
    # another draft length and n-gram size
    want, _, _, _ = host_loop(m, ids, 21, 15, 3)
    assert m.generate(input_ids=ids, max_new_tokens=21, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=15,
                      max_matching_ngram_size=3)[0].tolist() == want


@pytest.mark.parametrize("T", [0.2, 1.0])
def test_generate_sampled_equals_the_host_driven_loop(T):
    """sampler="device", top_k 50, top_p 0.7, a seeded generator: the host loop draws the same noise in the same order.  Compared up to the
    first step that the gate calls non-robust (from there on the two runs may go different ways).  What is compared depends on the host
    loop and the gate alone.  The gate admits up to 5 % non-robust rows; a 48-token run is then compared over (1 - 0.95^48) / (48 * 0.05)
    = 38 % of its tokens on average, which is the bar on the pool of runs."""
    m = _model()
    ids = _prompt()
    L0 = ids.shape[1]
    compared = total = 0
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        want, steps, _, robust = host_loop(m, ids, NEW, K, NG, sample=(T, 50, 0.7))
        torch.manual_seed(seed)
        got = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=K, do_sample=True,
                         temperature=T, top_k=50, top_p=0.7, sampler="device")[0].tolist()
        n_ok = L0
        for (d, a), ok in zip(steps, robust):
            if not ok:
                break
            n_ok += a + 1
        n_ok = min(n_ok, len(want))
        total += len(want) - L0
        compared += n_ok - L0
        assert got[:n_ok] == want[:n_ok], (seed, steps, robust)
        if n_ok == len(want):
            assert got == want
    print(f"T={T}: {compared} of {total} tokens compared")
    assert compared >= 0.38 * total


@pytest.mark.parametrize("kv_dtype", [None, "fp8_e4m3"], ids=["bf16", "fp8-cache"])
def test_rejected_positions_never_reach_a_result(kv_dtype):
    """The poison test: the same verify chunk with two different sets of drafts, all rejected; after truncate() one more token gives
    bit-identical logits on both caches."""
    m = _model()
    ids = _prompt()
    L0 = ids.shape[1]
    assert L0 > 64
    probe = _new_cache(m, L0, 40, 15, kv_dtype)
    t0 = int(m.forward(input_ids=ids, past_key_values=probe, use_cache=True).logits[0, -1].float().argmax())
    rows, toks = [], []
    for drafts in ([(t0 + 1 + i) % 90 for i in range(15)], [(t0 + 40 + 2 * i) % 90 for i in range(15)]):      # neither starts with t0
        cache = _new_cache(m, L0, 40, 15, kv_dtype)
        m.forward(input_ids=ids, past_key_values=cache, use_cache=True)
        cache.truncate(L0 - 1)
        out = m.forward(input_ids=torch.tensor([[int(ids[0, -1])] + drafts], device=DEV), past_key_values=cache, use_cache=True)
        assert cache.length == L0 + len(drafts)
        tok = int(out.logits[0, 0].float().argmax())
        assert tok != drafts[0]                                  # the first draft is rejected, and with it all of them
        cache.truncate(L0)
        assert cache.length == L0 and sum(h.shape[1] for h in cache.last_hidden) == L0
        toks.append(tok)
        rows.append(m.forward(input_ids=torch.tensor([[tok]], device=DEV), past_key_values=cache, use_cache=True).logits[0, -1])
    assert toks[0] == toks[1]
    assert torch.equal(rows[0], rows[1])


# The largest |logit difference| between the one-token path and the multi-token path (chunks of 2 .. 16 new tokens over the same cached
# prefix) on this prompt's plain greedy run, measured by tools/spec_decode_bench.py --tiny in the session that wrote
# profiles/spec_decode.txt: MEASURED_PATH_DIFF.  TAU is 1.5 times that.  Measured: 0.0 at every chunk length -- at this model's width the
# one-token and the multi-token forward take the same kernels, so their logits are bit-identical (logits reach 3.7; the plain run's
# smallest top-two gap is 0.0078, its median 0.25).  With TAU = 0 no gap is below it and all 32 positions are compared.  (At LLaMA-7B's
# width the two paths differ -- GEMV against skinny GEMM -- and the ids can part at near-ties: recorded in the same profile.)
MEASURED_PATH_DIFF = 0.0
TAU = 1.5 * MEASURED_PATH_DIFF


def test_generate_against_plain_greedy_generate():
    m = _model()
    ids = _prompt()
    L0 = ids.shape[1]
    plain = m.generate(input_ids=ids, max_new_tokens=32, use_cache=True, eos_token_id=-1)
    spec = m.generate(input_ids=ids, max_new_tokens=32, use_cache=True, eos_token_id=-1, prompt_lookup_num_tokens=K)
    # the plain run's own logits, one token at a time over the cache (the launches of generate()'s plain loop)
    cache = _new_cache(m, L0, 32, 0, None)
    lg = [m.forward(input_ids=ids, past_key_values=cache, use_cache=True).logits[0, -1]]
    for t in range(31):
        lg.append(m.forward(input_ids=plain[:, L0 + t:L0 + t + 1], past_key_values=cache, use_cache=True).logits[0, -1])
    top2 = torch.stack(lg).float().topk(2, dim=-1)[0]
    assert torch.equal(torch.stack(lg).float().argmax(-1), plain[0, L0:])
    gaps = (top2[:, 0] - top2[:, 1]).tolist()
    n_cmp = next((t for t, gp in enumerate(gaps) if gp < TAU), 32)
    print(f"tau = {TAU}: {n_cmp} of 32 positions compared; smallest gap {min(gaps):.4f}")
    assert n_cmp >= 16
    assert torch.equal(spec[0, :L0 + n_cmp], plain[0, :L0 + n_cmp])


def test_evaluate_passes_the_option_through():
    """evaluate(prompt_lookup_num_tokens=) on the tiny full model, greedy: ids, masks and boxes equal the plain evaluate's (this model's
    one-token and multi-token forwards are bit-identical, see TAU), so the [SEG] / [LOC] rows were read at the accepted positions."""
    from helpers import load_fixture
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    ids_p, masks_p, boxes_p = model.evaluate(*args, max_new_tokens=12, temperature=0.0)
    calls, ops = [], pkg("ops")
    orig = ops.spec_step

    def spy(*a, **k):
        calls.append(a[7])
        return orig(*a, **k)

    ops.spec_step = spy
    try:
        ids_s, masks_s, boxes_s = model.evaluate(*args, max_new_tokens=12, temperature=0.0, prompt_lookup_num_tokens=4)
    finally:
        ops.spec_step = orig
    assert calls and len(calls) <= 12
    assert torch.equal(ids_p, ids_s)
    assert len(masks_p) == len(masks_s) and all(torch.equal(x, y) for x, y in zip(masks_p, masks_s))
    assert len(boxes_p) == len(boxes_s) and all(torch.equal(x, y) for x, y in zip(boxes_p, boxes_s))
