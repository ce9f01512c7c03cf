"""ops.stop_strings / generate(stop_strings=) / evaluate(stop_strings=) on the GPU.  The kernel is held against the host rule
(`generation.stop_strings_reference`) with exact integer equality of `live` and `alive`, case by case and step by step; generate() against
its own run without stop strings, row by row, on every loop the option reaches."""
import random

import pytest
import torch

from helpers import pkg
from stop_tokenizer import FIRST_PIECE, N_SPECIAL, PIECES, build_tokenizer, byte_id, piece_id, random_row, utf8_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
_S = {}


def _setup():
    """the helper tokenizer and its table on the host (for the rule); V = len(tokenizer) + 5 = 317.  Nothing here touches the device: the
    case list below is built from it while the tests are collected, also where there is no GPU."""
    if not _S:
        tok = build_tokenizer()
        _S.update(tok=tok, host=pkg("generation").token_byte_table(tok, len(tok) + 5), V=len(tok) + 5)
    return _S


def _dev_table():
    """the same table on the device (for the kernel), made at the first launch."""
    if "dev" not in _S:
        _S["dev"] = pkg("ops").StopTable(*_setup()["host"], DEV)
    return _S["dev"]


def _launch(rows, L0, stops, live_in, alive_in=7, table=None, pitch_pad=0):
    """rows: equal-length id lists, prompt included -> (live, alive) after one ops.stop_strings over all of them.  pitch_pad > 0: the rows
    are cut from a wider buffer of `#` pieces (pitch != cur_len, a column offset, ids behind cur_len that would complete a string)."""
    ops = pkg("ops")
    cur = len(rows[0])
    wide = torch.full((len(rows), cur + 2 * pitch_pad), piece_id("#"), dtype=torch.int64)
    wide[:, pitch_pad:pitch_pad + cur] = torch.tensor(rows, dtype=torch.int64)
    ids = wide.to(DEV)[:, pitch_pad:pitch_pad + cur]
    live = torch.tensor(live_in, dtype=torch.int32, device=DEV)
    alive = torch.tensor([alive_in], dtype=torch.int32, device=DEV)
    ops.stop_strings(ids, L0, cur, _dev_table() if table is None else table, ops.StopStrings([s.encode() if isinstance(s, str) else s for s in stops], DEV),
                     live, alive)
    return live.tolist(), int(alive)


def _expected(rows, L0, stops, live_in, alive_in=7, host=None):
    """the rule, asked about the LAST token only: a live row stops now iff the rule's n is the number of generated ids."""
    ref = pkg("generation").stop_strings_reference
    host = _setup()["host"] if host is None else host
    fires = []
    for r, l in zip(rows, live_in):
        # a row whose earlier tokens had not stopped it (what a decode loop hands in): the rule's n itself; a row that had (and is live
        # all the same): the rule from the last token's first byte on, which is the rule over the last token alone plus the bytes before it
        n, before = ref(r, L0, host, stops), ref(r[:-1], L0, host, stops)
        if before is None:
            now = n == len(r) - L0
        else:
            text = b"".join(_pieces(host, r[L0:-1]))
            last = _pieces(host, r[-1:])[0]
            now = bool(last) and any((text + last).find(s.encode() if isinstance(s, str) else s, max(0, len(text) - len(s.encode() if isinstance(s, str) else s) + 1)) >= 0
                                     for s in stops)
        fires.append(bool(l) and now)
    return [0 if f else l for f, l in zip(fires, live_in)], alive_in - sum(fires), fires


# name -> (stop strings, generated ids, whether the last token stops the row)
def _cases():
    V = _setup()["V"]
    p = piece_id
    return {
        "completed exactly at the last byte of the last token": (["###"], [p("z"), p("#"), p("##")], True),
        "ends in the middle of the last token (overhang)": (["#x"], [p("z"), p("#"), p("x##y")], True),
        "wholly inside the last token": (["##"], [p("z"), p("x##y")], True),
        "spans three tokens with zero-byte special ids between them": (["a#b"], [p("a"), 2, p("#"), 0, p("b")], True),
        "longer than all generated text": (["zzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzzz###"], [p("#"), p("##")], False),
        "would have to begin before L0": (["###"], [p("#"), p("#")], False),
        "two strings fire in the same step": (["##", "x#"], [p("z"), p("x"), p("##")], True),
        "an id of -100 and ids >= V in the walk back": (["###"], [p("#"), -100, V, V + 7, 2 ** 40, p("##")], True),
        "a multi-byte character assembled from byte tokens": (["日"], [p("z")] + utf8_ids("日"), True),
        "the character's first bytes alone": (["日"], [p("z")] + utf8_ids("日")[:2], False),
        "the string ended one token ago": (["###"], [p("###"), p("z")], False),
        "a last token of no bytes": (["###"], [p("###"), 1], False),
        "nothing occurs": (["###", "the"], [p("z"), p("a"), p("b")], False),
    }


def _fit(gen, n):
    """the last n generated ids of a case, filled up in front with a piece no stop string holds."""
    return ([piece_id("y")] * n + gen)[-n:]


@pytest.mark.parametrize("name", list(_cases()), ids=lambda s: s.replace(" ", "_"))
def test_kernel_case_by_case(name):
    """Every case at R = 1, 3, 5 (5: cut from a wider buffer), L0 = 0, 1, 7 (the prompt is all `#`: counted, it would complete `###`) and
    1, 2, 9 generated ids.  In a launch, row 1 comes in dead and row 2 holds filler; the others hold the case."""
    stops, gen, fires_at_full_length = _cases()[name]
    assert _expected([[piece_id("#")] * 7 + gen], 7, stops, [1])[2] == [fires_at_full_length]         # the case is what its name says
    for R in (1, 3, 5):
        for L0 in (0, 1, 7):
            for n in (1, 2, 9):
                rows = [[piece_id("#")] * L0 + (_fit([piece_id("y")], n) if r % 3 == 2 else _fit(gen, n)) for r in range(R)]
                live_in = [0 if r == 1 else 1 + (r == 3) for r in range(R)]                           # (a live row may hold any non-zero word)
                want_live, want_alive, fires = _expected(rows, L0, stops, live_in)
                got = _launch(rows, L0, stops, live_in, pitch_pad=3 if R == 5 else 0)
                assert got == (want_live, want_alive), (name, R, L0, n, rows, got, want_live, want_alive)
                if R > 1:
                    assert got[0][1] == 0 and not fires[1]                                            # dead rows stay dead and are not counted
    # the natural length once more, alone
    rows = [[piece_id("#")] * 7 + gen]
    assert _launch(rows, 7, stops, [1]) == (([0], 6) if fires_at_full_length else ([1], 7))


def test_kernel_all_rows_dead_changes_nothing():
    rows = [[piece_id("#"), piece_id("##")]] * 4
    assert _launch(rows, 0, ["###"], [0, 0, 0, 0]) == ([0, 0, 0, 0], 7)
    assert _launch(rows, 0, ["###"], [1, 0, 1, 1]) == ([0, 0, 0, 0], 4)


def test_kernel_at_its_limits():
    """The largest number of strings and the longest string are taken; one more of either is refused by ops.StopStrings, and by the entry
    itself before any launch: nothing is written.  A table at the longest token and a window filled to its last byte."""
    ops, lib, G = pkg("ops"), pkg("_lib"), pkg("generation")
    S, B, T = ops.STOP_MAX_STRINGS, ops.STOP_MAX_BYTES, ops.STOP_MAX_TOKEN_BYTES
    ab = piece_id("ab")
    many = [f"q{i:02d}" for i in range(S - 1)] + ["ab" * (B // 2)]                                      # the one that occurs is the LAST of S, B bytes long
    for n_tok, fires in ((B // 2, True), (B // 2 - 1, False)):
        rows = [[piece_id("#")] * 2 + [ab] * n_tok, [piece_id("#")] * 2 + [piece_id("y")] * n_tok]
        assert _launch(rows, 2, many, [1, 1]) == _expected(rows, 2, many, [1, 1])[:2] == (([0, 1], 6) if fires else ([1, 1], 7))
    with pytest.raises(ValueError, match="ULL_STOP_MAX_STRINGS"):
        ops.StopStrings([b"q"] * (S + 1), DEV)
    with pytest.raises(ValueError, match="ULL_STOP_MAX_BYTES"):
        ops.StopStrings([b"q" * (B + 1)], DEV)
    # ... and the entry's own refusal, under an object that skipped the host check
    table = _dev_table()
    ids = torch.tensor([[piece_id("#"), piece_id("##")]], dtype=torch.int64, device=DEV)
    for lens in ([1] * (S + 1), [B + 1]):
        over = object.__new__(ops.StopStrings)
        over.stops = [b"#" * n for n in lens]
        over.offsets = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
        over.bytes = torch.full((sum(lens),), ord("#"), dtype=torch.uint8, device=DEV)
        live, alive = torch.ones(1, dtype=torch.int32, device=DEV), torch.full((1,), 7, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):
            ops.stop_strings(ids, 0, 2, table, over, live, alive)
        assert live.tolist() == [1] and int(alive) == 7
    # a table of its own: id 0 = `#` and T - 1 times `y` (the longest token allowed), id 1 = `x`; the stop string is B - 1 times `x` and `#`:
    # it ends on the FIRST byte of the longest token, so the window holds T + B - 1 bytes
    host = (torch.tensor([0, T, T + 1], dtype=torch.int32), torch.tensor(list(b"#" + b"y" * (T - 1) + b"x"), dtype=torch.uint8))
    dev = ops.StopTable(*host, DEV)
    assert dev.max_token_bytes == T and T + B - 1 <= ops.STOP_MAX_WINDOW
    stop = [b"x" * (B - 1) + b"#"]
    for n_x, fires in ((B - 1, True), (B - 2, False), (B + 5, True)):
        rows = [[0] * 3 + [1] * n_x + [0]]
        want = _expected(rows, 3, stop, [1], host=host)
        assert want[2] == [fires] and _launch(rows, 3, stop, [1], table=dev) == want[:2], n_x
    assert G.stop_strings_reference([1] * (B - 1) + [0], 0, host, stop) == B
    # a walk back of more than one round of 64 columns: seventy ids of no bytes between `#` and `##`
    for L0, fires in ((0, True), (1, False)):
        rows = [[piece_id("#")] + [2] * 70 + [piece_id("##")]]
        assert _launch(rows, L0, ["###"], [1]) == _expected(rows, L0, ["###"], [1])[:2] == (([0], 6) if fires else ([1], 7))


def _stepwise_rows():
    """the crafted cases and seeded random rows, each 12 generated ids long (filled up behind with <unk>: no bytes) behind a prompt of 3."""
    rng = random.Random(7)
    gens = [gen for stops, gen, _ in _cases().values() if len(gen) <= 12]
    gens += [random_row(rng, rng.randint(1, 12)) for _ in range(80)]
    gens += [[rng.choice([piece_id(x) for x in ("a", "b", "c", "▁cat", "s", "é", "\n", "y")]) for _ in range(12)] for _ in range(30)]
    return [[piece_id("#")] * 3 + g + [0] * (12 - len(g)) for g in gens]


def test_kernel_step_by_step():
    """The ids of 120-odd rows are fed one column at a time, as a decode loop does: the step at which `live` drops is the rule's n for
    every row, the step's counter loses exactly the rows that dropped, and a row that has dropped is never touched again."""
    G, ops = pkg("generation"), pkg("ops")
    s = _setup()
    stops = ["###", "#x", "日", "the", "a#b"]
    rows = _stepwise_rows()
    want = [G.stop_strings_reference(r, 3, s["host"], stops) for r in rows]
    never = sum(w is None for w in want)
    assert never >= len(rows) // 3 and len(rows) - never >= len(rows) // 4 and len({w for w in want}) >= 8, (never, len(rows))
    ids = torch.tensor(rows, dtype=torch.int64, device=DEV)
    live = torch.ones(len(rows), dtype=torch.int32, device=DEV)
    alive = torch.zeros(12, dtype=torch.int32, device=DEV)
    dev_stops = ops.StopStrings([x.encode() for x in stops], DEV)
    history = []
    for j in range(12):
        ops.stop_strings(ids, 3, 3 + j + 1, _dev_table(), dev_stops, live, alive[j:j + 1])
        history.append(live.clone())
    history = torch.stack(history).cpu()                               # [step, row]
    got = [next((j + 1 for j in range(12) if history[j, r] == 0), None) for r in range(len(rows))]
    assert got == want, [(r, g, w) for r, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    assert alive.tolist() == [-sum(w == j + 1 for w in want) for j in range(12)]
    for r, w in enumerate(want):                                       # dropped once, for good
        assert history[:, r].tolist() == [1] * (12 if w is None else w - 1) + [0] * (0 if w is None else 12 - w + 1)


# ---- generate() on the tiny model -----------------------------------------------------------------------------------------------------------
NEW, PAD = 12, 0


def _model():
    from test_logprobs_gpu import _model as tiny
    return tiny(BF)


def _gen_setup():
    """the tokenizer the tiny model (vocab 100) speaks: the pieces stand before the byte tokens, so its ids are pieces of several bytes."""
    if "gtok" not in _S:
        tok = build_tokenizer(pieces_first=True)
        _S.update(gtok=tok, ghost=pkg("generation").token_byte_table(tok, 100))
    return _S["gtok"], _S["ghost"]


def _pieces(host, gen):
    off, data = host[0].tolist(), bytes(host[1].tolist())
    return [data[off[t]:off[t + 1]] if 0 <= t < len(off) - 1 else b"" for t in gen]


def _as_text(b):
    try:
        s = b.decode("utf-8")
    except UnicodeDecodeError:
        return None
    return s if s and "\ufffd" not in s else None


def _ending_at(pieces, j, cut, width):
    """a string of up to `width` bytes that ends `cut` bytes into token j of a row (cut = len(pieces[j]): at its end), or None."""
    end = sum(len(p) for p in pieces[:j]) + cut
    text = b"".join(pieces)
    for w in range(width, 0, -1):
        s = _as_text(text[max(0, end - w):end])
        if s is not None and end - w >= 0:
            return s
    return None


def _pick_two(host, gens):
    """(A, B, n): A ends in the MIDDLE of a token of row 0, B is completed at the END of a late token of row 1, row 0 and row 1 stop at
    different steps strictly before NEW and row 2 does not stop -- all by the rule."""
    ref = pkg("generation").stop_strings_reference
    pcs = [_pieces(host, g) for g in gens]
    for j0 in range(1, NEW - 1):
        if len(pcs[0][j0]) < 2:
            continue
        A = _ending_at(pcs[0], j0, 1, 5)
        for j1 in range(NEW - 2, 1, -1):
            B = _ending_at(pcs[1], j1, len(pcs[1][j1]), 5) if pcs[1][j1] else None
            if A is None or B is None:
                continue
            n = [ref(g, 0, host, [A, B]) for g in gens]
            if n[0] is not None and n[1] is not None and n[0] < n[1] < NEW and n[2] is None and n[0] == j0 + 1:
                return A, B, n
    return None


def _pick_all(host, gens):
    """stop strings under which EVERY row stops within 6 tokens, not all at the same step (the fused loop first looks at the host after
    step 8: it overruns and trims), or None."""
    ref = pkg("generation").stop_strings_reference
    pcs = [_pieces(host, g) for g in gens]
    for base in (1, 2, 0):
        stops = [_ending_at(p, base + r, len(p[base + r]), 3) if p[base + r] else None for r, p in enumerate(pcs)]
        if any(s is None for s in stops):
            continue
        n = [ref(g, 0, host, stops) for g in gens]
        if all(x is not None for x in n) and max(n) <= 6 and len(set(n)) > 1:
            return stops, n
    return None


PATHS = {
    "greedy fused": dict(),
    "device sampler": dict(do_sample=True, temperature=0.7, top_k=50, sampler="device"),
    "device n-gram ban": dict(no_repeat_ngram_size=2, ngram_ban="device"),
    "host sampler": dict(do_sample=True, temperature=0.7, top_k=50),
    "host sampler, device ban": dict(do_sample=True, temperature=0.7, top_k=50, no_repeat_ngram_size=2, ngram_ban="device"),
    "fp8 kv cache": dict(kv_cache_dtype="fp8_e4m3"),
}


def _check_rows(out, free, L0, n, n_tok):
    """every row equals the run without stop strings up to and including its stopping token, then pad; log-probabilities and hidden states alike."""
    assert out.sequences.shape[1] == L0 + n_tok and tuple(out.logprobs.shape) == (out.sequences.shape[0], n_tok)
    hid, hid_free = out.hidden_states[-1][-1], free.hidden_states[-1][-1]
    assert hid.shape[1] == L0 + n_tok - 1
    for r, n_r in enumerate(n):
        k = n_tok if n_r is None else n_r
        assert out.sequences[r, :L0 + k].tolist() == free.sequences[r, :L0 + k].tolist(), (r, n)
        assert out.sequences[r, L0 + k:].tolist() == [PAD] * (n_tok - k), (r, n, out.sequences[r].tolist())
        assert torch.equal(out.logprobs[r, :k], free.logprobs[r, :k]) and bool((out.logprobs[r, k:] == 0).all()), (r, n)
        assert torch.equal(hid[r, :L0 + k - 1], hid_free[r, :L0 + k - 1]), (r, n)


@pytest.mark.parametrize("path", list(PATHS), ids=lambda s: s.replace(" ", "_").replace(",", ""))
def test_generate_stops_each_row_on_text(path):
    from test_device_sampler_gpu import _text_ids
    G = pkg("generation")
    m = _model()
    tok, host = _gen_setup()
    kw = dict(max_new_tokens=NEW, eos_token_id=-1, pad_token_id=PAD, use_cache=True, return_dict_in_generate=True, output_logprobs=True,
              output_hidden_states=True, **PATHS[path])

    def run(ids, **more):
        torch.manual_seed(5)
        return m.generate(input_ids=ids, **kw, **more)

    two = every = None
    for seed in range(40, 52):                                     # (a prompt whose free run offers the strings: the rule picks, nothing is tuned)
        ids = _text_ids(3, 9, seed)
        free = run(ids)
        gens = free.sequences[:, 9:].tolist()
        found = (None if two else _pick_two(host, gens)), (None if every else _pick_all(host, gens))
        two = two or (found[0] and (ids, free) + found[0])
        every = every or (found[1] and (ids, free) + found[1])
        if two and every:
            break
    assert two and every, "no prompt of twelve offered the stop strings the test needs"
    calls = []
    MC = pkg("modeling_core")                                      # (generate() calls the loops by the names it imported)
    saved = MC.fused_loop, MC.host_loop
    MC.fused_loop = lambda d, *a, **k: (calls.append(("fused", d)), saved[0](d, *a, **k))[1]
    MC.host_loop = lambda d, *a, **k: (calls.append(("host", d)), saved[1](d, *a, **k))[1]
    try:
        ids, free, A, B, n = two
        out = run(ids, stop_strings=[A, B], tokenizer=tok)
        print(f"{path}: {A!r} stops row 0 at {n[0]}, {B!r} row 1 at {n[1]}, row 2 runs to {NEW}")
        _check_rows(out, free, 9, n, NEW)                          # the last row never stops: the full length
        ids, free, stops, n = every
        out = run(ids, stop_strings=stops, tokenizer=tok)
        print(f"{path}: {stops!r} stop the rows at {n}")
        _check_rows(out, free, 9, n, max(n))                       # ... the length of the last row to finish
    finally:
        MC.fused_loop, MC.host_loop = saved
    want = "host" if path.startswith("host sampler") else "fused"
    assert [c[0] for c in calls] == [want, want]
    if want == "fused":
        assert all(d.check == 8 and d.stops is not None for _, d in calls)


def test_generate_second_turn_ignores_the_text_of_earlier_turns():
    """Turn 2 continues turn 1's cache; its input_ids are the whole conversation.  One stop string lies wholly in turn 1's answer, the
    other begins in the conversation's last tokens and ends on the first byte turn 2 generates: counted from any earlier column than this
    call's input_ids.shape[1] it fires at once.  It does not."""
    from test_device_sampler_gpu import _text_ids
    G = pkg("generation")
    m = _model()
    tok, host = _gen_setup()
    kw = dict(max_new_tokens=8, eos_token_id=-1, pad_token_id=PAD, return_dict_in_generate=True)
    for seed in range(60, 72):
        ids = _text_ids(1, 9, seed)
        cache = m.new_kv_cache(1, 64, None)
        turn1 = m.generate(input_ids=ids, past_key_values=cache, **kw).sequences
        conv = torch.cat([turn1, _text_ids(1, 2, seed + 100)], dim=1)
        L0 = conv.shape[1]
        free = m.generate(input_ids=conv, past_key_values=cache.fork(), **kw).sequences
        pcs = _pieces(host, free[0].tolist())
        inside = _ending_at(pcs, 12, len(pcs[12]), 4) if pcs[12] else None                   # ends in turn 1's answer (columns 9 .. 16)
        across = _ending_at(pcs, L0, 1, 4) if pcs[L0] and sum(len(p) for p in pcs[L0 - 2:L0]) >= 3 else None
        if inside is None or across is None or len(across.encode()) < 2:
            continue
        stops = [inside, across]
        n = G.stop_strings_reference(free[0].tolist(), L0, host, stops)
        if G.stop_strings_reference(free[0].tolist(), 9, host, stops) is None or n == 1:
            continue
        out = m.generate(input_ids=conv, past_key_values=cache.fork(), stop_strings=stops, tokenizer=tok, **kw)
        assert out.sequences[0].tolist() == free[0, :L0 + (8 if n is None else n)].tolist() and out.past_key_values.length == out.sequences.shape[1] - 1
        return
    raise AssertionError("no prompt of twelve offered the stop strings the test needs")


def test_batch_one_equals_a_host_criterion_and_reads_the_host_every_eight_steps():
    from test_device_sampler_gpu import _text_ids
    G = pkg("generation")
    m = _model()
    tok, host = _gen_setup()
    kw = dict(max_new_tokens=16, eos_token_id=-1, pad_token_id=PAD, use_cache=True, return_dict_in_generate=True, output_logprobs=True, output_hidden_states=True)
    picked = None
    for seed in range(80, 92):
        ids = _text_ids(1, 9, seed)
        free = m.generate(input_ids=ids, **kw)
        pcs = _pieces(host, free.sequences[0, 9:].tolist())
        for j in range(9, 2, -1):
            S = _ending_at(pcs, j, len(pcs[j]), 4) if pcs[j] else None
            n = None if S is None else G.stop_strings_reference(free.sequences[0].tolist(), 9, host, [S])
            if n is not None and 2 <= n <= 10:
                picked = picked or (ids, S, n)
        if picked:
            break
    assert picked, "no prompt of twelve offered the stop string the test needs"
    ids, S, n = picked
    seen = []
    MC = pkg("modeling_core")
    orig = MC.fused_loop
    MC.fused_loop = lambda d, *a, **k: (seen.append(d), orig(d, *a, **k))[1]
    reads = []
    cpu = torch.Tensor.cpu
    torch.Tensor.cpu = lambda t, *a, **k: (reads.append(tuple(t.shape)) if t.dtype == torch.int32 and t.is_cuda and t.dim() == 1 else None, cpu(t, *a, **k))[1]
    try:
        crit = lambda out_ids, scores: G.stop_strings_reference(out_ids[0].tolist(), 9, host, [S]) is not None          # noqa: E731
        by_host = m.generate(input_ids=ids, stopping_criteria=[crit], **kw)
        del reads[:]
        by_dev = m.generate(input_ids=ids, stop_strings=S, tokenizer=tok, **kw)
        reads_stopping = list(reads)
        del reads[:]
        unstopped = m.generate(input_ids=ids, stop_strings="\x7f never \x7f", tokenizer=tok, **kw)
        reads_full = list(reads)
    finally:
        MC.fused_loop = orig
        torch.Tensor.cpu = cpu
    assert by_host.sequences.shape[1] == 9 + n and torch.equal(by_dev.sequences, by_host.sequences)
    assert torch.equal(by_dev.logprobs, by_host.logprobs) and torch.equal(by_dev.hidden_states[-1][-1], by_host.hidden_states[-1][-1])
    assert [d.check for d in seen] == [1, 8, 8] and seen[0].stops is None and seen[1].stops is not None
    # the loop's only device -> host read is `alive[:n_done].cpu()`, the int32 vector of the step counters: once after step 8 and, for a run
    # that has not stopped by then, once after step 16 (the prefill's own read of the multimodal spans is a [B, 4] matrix, once per call)
    assert unstopped.sequences.shape[1] == 9 + 16 and reads_full == [(8,), (16,)], reads_full
    assert reads_stopping == ([(8,)] if n <= 8 else [(8,), (16,)]), (n, reads_stopping)


def test_batch_needs_a_pad_id():
    from test_device_sampler_gpu import _text_ids
    m = _model()
    tok, _ = _gen_setup()
    eos, m.config.eos_token_id = m.config.eos_token_id, None      # (a model without an EOS id and without a pad id)
    try:
        with pytest.raises(ValueError, match="pad_token_id"):
            m.generate(input_ids=_text_ids(2, 9, 1), max_new_tokens=2, stop_strings="#", tokenizer=tok)
    finally:
        m.config.eos_token_id = eos
    assert m.generate(input_ids=_text_ids(1, 9, 1), max_new_tokens=2, eos_token_id=-1, stop_strings="\x7f\x7f", tokenizer=tok).shape == (1, 11)


def test_evaluate_stops_on_text():
    from helpers import load_fixture
    from test_fp8_weights_gpu import _tiny_full
    G = pkg("generation")
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    model.llm.strict_checks = False     # (random weights may emit an image start id without its end; both runs feed the same ids)
    V = model.llm.config.vocab_size
    tok = build_tokenizer(vocab_size=V, pieces_first=True)
    host = G.token_byte_table(tok, V)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    L0 = args[2].shape[1]
    ids_f, masks_f, boxes_f = model.evaluate(*args, max_new_tokens=8, temperature=0.0)
    pcs = _pieces(host, ids_f[0, L0:].tolist())
    picked = None
    for j in range(6, 0, -1):
        S = _ending_at(pcs, j, len(pcs[j]), 4) if pcs[j] else None
        n = None if S is None else G.stop_strings_reference(ids_f[0].tolist(), L0, host, [S])
        if n is not None and 2 <= n <= 7:
            picked = (S, n)
            break
    assert picked, (ids_f[0, L0:].tolist(), pcs)
    S, n = picked
    ids_s, masks_s, boxes_s = model.evaluate(*args, max_new_tokens=8, temperature=0.0, stop_strings=[S], tokenizer=tok)
    assert ids_s.shape[1] == L0 + n and torch.equal(ids_s, ids_f[:, :L0 + n])
    assert len(masks_s) == 1 and len(boxes_s) == 1
