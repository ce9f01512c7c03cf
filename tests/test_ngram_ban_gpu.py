"""The on-device n-gram ban on the GPU: the kernel (ops.ngram_ban / ull_ngram_ban) against the host rule
`generation.no_repeat_ngram_banned_tokens`, then generate(ngram_ban="device") / evaluate(ngram_ban="device") against the same call with the
host ban on tiny models.  Everything is exact: logits are compared as bit patterns (NaN and -inf included), ids with torch.equal; there is
no tolerance anywhere."""
import pytest
import torch

from helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NINF = float("-inf")
NGRAMS = (1, 2, 3, 5)
KINDS = ("one", "period3", "many", "edges", "random")
TRAP = 6            # an id only the "edges" rows at V = 7 hold: it stands behind every row's end, where reading it would ban it


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
def crafted_row(kind, r, L, V):
    """L ids of row r.  one: a single token (every window overlaps the tail); period3: 1 2 4 1 2 4 ...; many: 5 2 5 2 ... (one token banned by
    every second window); edges: 0 and V - 1 alternate (the banned token is the first or the last entry of the logits row); random: a
    4-symbol alphabet, seeded by the row.  Rows of one batch differ by a shift."""
    if kind == "one":
        return [3] * L
    if kind == "period3":
        return [(1, 2, 4)[(i + r) % 3] for i in range(L)]
    if kind == "many":
        return [(5, 2)[(i + r) % 2] for i in range(L)]
    if kind == "edges":
        return [(0, V - 1)[(i + r) % 2] for i in range(L)]
    g = torch.Generator().manual_seed(100 + r)
    return torch.randint(0, 4, (L,), generator=g).tolist()


_RULE = {}


def host_rule(row, n):
    """generation.no_repeat_ngram_banned_tokens of one row, computed once per (row, n) for the whole module."""
    key = (tuple(row), n)
    if key not in _RULE:
        _RULE[key] = pkg("generation").no_repeat_ngram_banned_tokens([list(row)], n)[0]
    return _RULE[key]


def cur_lens(n):
    return sorted({c for c in (0, n - 2, n - 1, n, 9, 1500) if c >= 0})


def expected(logits, rows, n, V):
    """-> (a clone of logits with -inf at the host rule's tokens inside [0, V), whether the rule banned anything at all in some row)."""
    mask = torch.zeros(len(rows), V, dtype=torch.bool)
    any_ban = False
    for r, row in enumerate(rows):
        banned = host_rule(row, n)
        any_ban |= bool(banned)
        for t in set(banned):
            if 0 <= t < V:
                mask[r, t] = True
    return logits.clone().masked_fill(mask.to(logits.device), NINF), any_ban


def make_logits(R, V, dtype, seed):
    """x[:, -1] of a [R, 3, V] tensor: rows 3 V elements apart, so odd V gives row bases at every 2-byte (4-byte) alignment; NaN, +inf and -inf
    are sprinkled in, one of each in every 11 entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, 3, V, generator=g)
    flat = x.view(-1)
    flat[0::11] = float("nan")
    flat[3::11] = float("inf")
    flat[7::11] = NINF
    return x.to(dtype).to(DEV)[:, -1]


def wide_ids(rows, L, n):
    """[R, L + n + 6] int64 on the device, the rows in the first L columns; behind them the row's trailing n - 1 ids again and TRAP -- a
    kernel that read past cur_len would find one more window and ban TRAP -- then more of the alphabet."""
    R = len(rows)
    wide = torch.empty(R, L + n + 6, dtype=torch.int64)
    for r, row in enumerate(rows):
        tail = row[L - (n - 1):] if n > 1 and L >= n - 1 else []
        rest = tail + [TRAP] + [1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3]
        wide[r] = torch.tensor(row + rest[:n + 6])
    return wide.to(DEV)


@pytest.mark.parametrize("V", [1, 7, 8, 97, 4099])
@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "fp16", "fp32"])
def test_kernel_against_the_host_rule(dtype, V):
    ops = pkg("ops")
    n_cases = n_long = n_long_banned = n_in_range = 0
    for R in (1, 3, 70):
        logits = make_logits(R, V, dtype, seed=1000 * R + V)
        assert logits.stride(0) == 3 * V and logits.stride(1) == 1
        f = logits.float()
        assert V < 97 or (bool(f.isnan().any()) and bool((f == NINF).any()) and bool((f == float("inf")).any()))
        pad = torch.full((R, V + 9), 1.5, dtype=dtype, device=DEV)
        for n in NGRAMS:
            for L in cur_lens(n):
                for kind in KINDS:
                    rows = [crafted_row(kind, r, L, V) for r in range(R)]
                    want, any_ban = expected(logits, rows, n, V)
                    ids = wide_ids(rows, L, n)[:, :L]              # a column-prefix view: ids_ld > cur_len
                    assert ids.shape == (R, L) and ids.stride(0) == L + n + 6
                    if n_cases % 2 == 0:
                        got = ops.ngram_ban(logits, ids, L, n)
                        assert got.dtype == dtype and got.shape == (R, V) and got.is_contiguous()
                    else:
                        # rows that start one element behind the allocation's base: source and destination alignments differ
                        out = pad[:, 1:1 + V]
                        got = ops.ngram_ban(logits, ids, L, n, out=out)
                        assert got.data_ptr() == out.data_ptr()
                    assert torch.equal(bits(got), bits(want)), (R, n, L, kind)
                    n_cases += 1
                    n_in_range += int((bits(want) != bits(logits)).sum())
                    if L >= n:
                        n_long += 1
                        n_long_banned += any_ban
        assert bool((pad[:, 0] == 1.5).all()) and bool((pad[:, 1 + V:] == 1.5).all())
    print(f"{dtype} V={V}: {n_cases} cases; the host rule bans something in {n_long_banned} of the {n_long} with cur_len >= ngram; "
          f"{n_in_range} logits changed by in-range bans")
    assert 2 * n_long_banned >= n_long and n_in_range > 0


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_kernel_vocabulary_sized_rows(dtype):
    """V = 32064 (the LLaMA vocabulary: every thread of the block copies several 16-byte chunks) on aligned rows, every id of a 4-symbol row
    banned under ngram 1."""
    ops = pkg("ops")
    V, R, L = 32064, 2, 40
    logits = make_logits(R, V, dtype, seed=5)
    rows = [crafted_row("random", r, L, V) for r in range(R)]
    want, any_ban = expected(logits, rows, 1, V)
    got = ops.ngram_ban(logits, wide_ids(rows, L, 1)[:, :L], L, 1)
    assert any_ban and torch.equal(bits(got), bits(want))


def test_kernel_more_rows_than_one_grid_pass():
    """70 001 rows on a grid of 65 536 blocks: the first 4 465 blocks take a second row."""
    ops = pkg("ops")
    R, V, L, n = 70001, 7, 4, 2
    logits = make_logits(R, V, BF, seed=9)
    rows = [crafted_row("many", r, L, V) for r in range(R)]
    want, any_ban = expected(logits, rows, n, V)
    got = ops.ngram_ban(logits, torch.tensor(rows, device=DEV), L, n)
    assert any_ban and torch.equal(bits(got), bits(want))
    assert int((bits(want[65536:]) != bits(logits[65536:])).sum()) > 0


@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V", [7, 97])
def test_kernel_skips_out_of_range_ids(dtype, V):
    """The continuations of the trailing id are -1, V and V + 3 (skipped: a store through one of them would land in the sentinels around
    `out`) and 2 (banned)."""
    ops = pkg("ops")
    a = 4
    row = [a, 2, a, -1, a, V, a, V + 3, a]
    R, L = 3, len(row)
    rows = [row] * R
    assert sorted(host_rule(row, 2)) == sorted([2, -1, V, V + 3])
    logits = make_logits(R, V, dtype, seed=V)
    want, _ = expected(logits, rows, 2, V)
    assert int((bits(want) != bits(logits)).sum()) >= 1            # token 2 of some row was not -inf before
    big = torch.full((R + 2, V + 10), 2.5, dtype=dtype, device=DEV)
    out = big[1:1 + R, 5:5 + V]
    ops.ngram_ban(logits, torch.tensor(rows, device=DEV), L, 2, out=out)
    assert torch.equal(bits(out), bits(want))
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:1 + R, 5:5 + V] = False
    assert bool((big[keep] == 2.5).all())
    # ngram 1: the row's own ids, the out-of-range ones among them
    want1, _ = expected(logits, rows, 1, V)
    big.fill_(2.5)
    ops.ngram_ban(logits, torch.tensor(rows, device=DEV), L, 1, out=out)
    assert torch.equal(bits(out), bits(want1)) and bool((big[keep] == 2.5).all())


def test_op_refusals():
    ops = pkg("ops")
    lg = torch.zeros(2, 8, dtype=BF, device=DEV)
    ids = torch.zeros(2, 5, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.ngram_ban(lg, ids, 5, 2, out=lg)
    with pytest.raises(RuntimeError, match="must be torch.int64"):
        ops.ngram_ban(lg, ids.int(), 5, 2)
    with pytest.raises(RuntimeError, match="ids must be"):
        ops.ngram_ban(lg, ids, 6, 2)
    with pytest.raises(ValueError, match="ngram must be >= 1"):
        ops.ngram_ban(lg, ids, 5, 0)
    with pytest.raises(RuntimeError, match="out"):
        ops.ngram_ban(lg, ids, 5, 2, out=torch.zeros(2, 8, dtype=F16, device=DEV))
    assert ops.ngram_ban(lg[:0], ids[:0], 5, 2).shape == (0, 8)


# ---- generate() on the tiny model -----------------------------------------------------------------------------------------------------------
def _model(dtype=BF):
    from test_logprobs_gpu import _model as tiny
    return tiny(dtype)


def _prompt():
    """two rows of a repetitive prompt: greedy decoding wants to go on repeating, which the ban forbids."""
    return torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6, 7, 5, 6], [9, 9, 9, 9, 8, 9, 9, 9, 9, 8, 9]], device=DEV)


def _same_nested(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and len(a) == len(b) and all(_same_nested(x, y) for x, y in zip(a, b))


def _steps_where_the_ban_bit(m, seq, L0, n):
    """Over the emitted positions of every row: how often the argmax of the RAW logits (the model's own forward over the ids so far) was a
    token the host rule bans there."""
    G = pkg("generation")
    bit = 0
    with torch.no_grad():
        for j in range(seq.shape[1] - L0):
            raw = m.forward(input_ids=seq[:, :L0 + j]).logits[:, -1].float().argmax(-1).tolist()
            banned = G.no_repeat_ngram_banned_tokens(seq[:, :L0 + j].tolist(), n)
            bit += sum(raw[b] in banned[b] for b in range(seq.shape[0]))
    return bit


def _two_ends(free, L0, new):
    """EOS ids from the free run with which the two rows finish at different steps, both before step 7 (the fused loop first looks at the
    host after step 8, so it pad-fills a finished row under the ban and trims its overrun)."""
    for j0 in range(1, 7):
        for j1 in range(1, 7):
            eos = [int(free[0, L0 + j0]), int(free[1, L0 + j1])]
            ends = [min((j for j in range(new) if int(free[b, L0 + j]) in eos), default=new) for b in range(2)]
            if ends[0] != ends[1] and max(ends) < 7:
                return eos, ends
    raise AssertionError(f"no usable pair of EOS ids in the free run {free[:, L0:].tolist()}")


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("cached", [True, False], ids=["kv_cache", "no_cache_keep_last_step"])
def test_generate_greedy_fused_loop_with_device_ban_equals_host_loop_with_host_ban(cached, n):
    m = _model()
    ids = _prompt()
    L0, new = ids.shape[1], 12
    kw = dict(input_ids=ids, max_new_tokens=new, do_sample=False, no_repeat_ngram_size=n, output_hidden_states=True, return_dict_in_generate=True,
              output_logprobs=True, **(dict(use_cache=True) if cached else dict(use_cache=False, keep_last_step_only=True)))
    host = m.generate(eos_token_id=-1, **kw)
    dev = m.generate(eos_token_id=-1, ngram_ban="device", **kw)
    assert host.sequences.shape == (2, L0 + new) and torch.equal(dev.sequences, host.sequences)
    assert torch.equal(dev.logprobs, host.logprobs) and _same_nested(dev.hidden_states, host.hidden_states)
    bit = _steps_where_the_ban_bit(m, host.sequences, L0, n)
    plain = m.generate(eos_token_id=-1, **dict(kw, no_repeat_ngram_size=None)).sequences
    print(f"ngram {n}: the raw argmax was banned at {bit} of {2 * new} steps; ids differ from the run without a ban: {not torch.equal(plain, host.sequences)}")
    assert bit >= 1

    # two rows that end at different steps, both before the fused loop's first look at the host
    eos, ends = _two_ends(host.sequences, L0, new)
    host_e = m.generate(eos_token_id=eos, **kw)
    dev_e = m.generate(eos_token_id=eos, ngram_ban="device", **kw)
    n_tok = max(ends) + 1
    assert host_e.sequences.shape[1] == L0 + n_tok, (ends, host_e.sequences[:, L0:].tolist())
    assert torch.equal(dev_e.sequences, host_e.sequences)
    assert torch.equal(dev_e.logprobs, host_e.logprobs) and tuple(dev_e.logprobs.shape) == (2, n_tok)
    assert bool((dev_e.logprobs[ends.index(min(ends)), min(ends) + 1:] == 0).all())
    assert _same_nested(dev_e.hidden_states, host_e.hidden_states)
    assert dev_e.hidden_states[-1][-1].shape[1] == L0 + n_tok - 1


SAMPLE_SEED = 3


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("cached", [True, False], ids=["kv_cache", "no_cache_keep_last_step"])
def test_generate_device_sampler_with_device_ban_equals_host_sampler_with_host_ban(cached, n):
    """One seed, the same noise: sampler="device" draws the host sampler's token wherever the draw is not a near-tie between the two
    samplers' arithmetic (tests/test_device_sampler_gpu.py measures that gate); on this prompt none of the seeds 0 .. 11 meets one in any
    of the four cases, SAMPLE_SEED is one of them.  No row finishes early: the fused loop's overrun would advance the generator further,
    as documented."""
    m = _model()
    ids = _prompt()
    L0, new = ids.shape[1], 12
    kw = dict(input_ids=ids, max_new_tokens=new, do_sample=True, temperature=0.7, top_k=50, no_repeat_ngram_size=n, eos_token_id=-1,
              output_hidden_states=True, return_dict_in_generate=True, output_logprobs=True,
              **(dict(use_cache=True) if cached else dict(use_cache=False, keep_last_step_only=True)))
    torch.manual_seed(SAMPLE_SEED)
    host = m.generate(**kw)
    torch.manual_seed(SAMPLE_SEED)
    dev = m.generate(sampler="device", ngram_ban="device", **kw)
    assert torch.equal(dev.sequences, host.sequences), (host.sequences[:, L0:].tolist(), dev.sequences[:, L0:].tolist())
    assert torch.equal(dev.logprobs, host.logprobs) and _same_nested(dev.hidden_states, host.hidden_states)
    # the ban held: no n-gram of the new tokens repeats one the row already had
    G = pkg("generation")
    for j in range(new):
        banned = G.no_repeat_ngram_banned_tokens(dev.sequences[:, :L0 + j].tolist(), n)
        assert all(int(dev.sequences[b, L0 + j]) not in banned[b] for b in range(2)), j


@pytest.mark.parametrize("n", [1, 2])
def test_generate_host_sampler_device_ban_equals_host_ban(n):
    m = _model()
    ids = _prompt()
    kw = dict(input_ids=ids, max_new_tokens=12, do_sample=True, temperature=0.7, top_k=50, no_repeat_ngram_size=n, eos_token_id=-1, use_cache=True,
              return_dict_in_generate=True, output_logprobs=True)
    torch.manual_seed(11)
    a = m.generate(**kw)
    state_a = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(11)
    b = m.generate(ngram_ban="device", **kw)
    state_b = torch.cuda.get_rng_state(DEV)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs)
    assert torch.equal(state_a, state_b)
    torch.manual_seed(11)
    c = m.generate(ngram_ban="host", **kw)
    assert torch.equal(a.sequences, c.sequences)


def test_the_option_decides_which_code_runs():
    """ngram_ban="device": ops.greedy_step and ops.ngram_ban run, the list rule does not; the default: the reverse."""
    G, ops = pkg("generation"), pkg("ops")
    m = _model()
    calls = []
    orig = dict(rule=G.no_repeat_ngram_banned_tokens, greedy=ops.greedy_step, ban=ops.ngram_ban)

    def spy(name):
        def f(*a, **k):
            calls.append(name)
            return orig[name](*a, **k)
        return f

    G.no_repeat_ngram_banned_tokens, ops.greedy_step, ops.ngram_ban = spy("rule"), spy("greedy"), spy("ban")
    try:
        kw = dict(input_ids=_prompt(), max_new_tokens=4, no_repeat_ngram_size=2, eos_token_id=-1, use_cache=True)
        m.generate(ngram_ban="device", **kw)
        assert calls.count("greedy") == 4 and calls.count("ban") == 4 and "rule" not in calls, calls
        del calls[:]
        m.generate(**kw)
        assert calls == ["rule"] * 4, calls
        del calls[:]
        # the host sampler keeps the host loop and only swaps the ban
        torch.manual_seed(0)
        m.generate(ngram_ban="device", do_sample=True, temperature=0.7, **kw)
        assert calls == ["ban"] * 4, calls
        del calls[:]
        # without a ban nothing of this runs
        m.generate(**dict(kw, no_repeat_ngram_size=None))
        assert calls == ["greedy"] * 4, calls
    finally:
        G.no_repeat_ngram_banned_tokens, ops.greedy_step, ops.ngram_ban = orig["rule"], orig["greedy"], orig["ban"]


def test_evaluate_with_the_device_ban_returns_the_host_bans_ids():
    from helpers import load_fixture
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    model.llm.strict_checks = False     # (random weights under a ban may emit an image start id without its end; both runs feed the same ids)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    ids_h, masks_h, boxes_h = model.evaluate(*args, max_new_tokens=8, no_repeat_ngram_size=2, temperature=0.0)
    ids_d, masks_d, boxes_d = model.evaluate(*args, max_new_tokens=8, no_repeat_ngram_size=2, ngram_ban="device", temperature=0.0)
    assert torch.equal(ids_h, ids_d)
    assert len(masks_h) == len(masks_d) and all(torch.equal(x, y) for x, y in zip(masks_h, masks_d))
    assert len(boxes_h) == len(boxes_d) and all(torch.equal(x, y) for x, y in zip(boxes_h, boxes_d))
