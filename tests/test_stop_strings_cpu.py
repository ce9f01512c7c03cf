"""generate(stop_strings=, tokenizer=) / evaluate(...) / ops.stop_strings / ull_stop_strings: what can be checked without a GPU -- the C ABI,
where the keywords stand, every refusal before device work, the token byte table, and the rule (`generation.stop_strings_reference`) against
the project's KeywordsStoppingCriteria and against transformers' StopStringCriteria on a LLaMA-shaped tokenizer built in-process."""
import ctypes
import inspect
import os
import random
import re

import pytest
import torch

from helpers import pkg
from stop_tokenizer import FIRST_PIECE, N_SPECIAL, PIECES, build_tokenizer, byte_id, piece_id, random_row, utf8_ids
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = torch.tensor([[1, 5, 6, 7, 5, 6]])
_TOK = {}


def _tok():
    if not _TOK:
        t = build_tokenizer()
        _TOK["tok"], _TOK["table"] = t, pkg("generation").token_byte_table(t, len(t) + 5)       # (5 padded embedding rows behind the tokenizer)
    return _TOK["tok"], _TOK["table"]


def _bytes(table, i):
    off, data = table
    return bytes(data[int(off[i]):int(off[i + 1])].tolist())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib, ops = pkg("_lib"), pkg("ops")
    so = ctypes.CDLL(lib.LIB_PATH)
    m = re.search(r"\bint ull_stop_strings\(([^;]*)\);", header)
    assert m, "ull_stop_strings not declared in include/ullava_hip.h"
    assert "ull_stop_strings" in lib.SIGNATURES and hasattr(so, "ull_stop_strings")
    assert len(m.group(1).split(",")) == len(lib.SIGNATURES["ull_stop_strings"]) == 16 and lib.RESTYPES["ull_stop_strings"] is ctypes.c_int
    assert not any(n.startswith("ull_stop_strings_") for n in lib.SIGNATURES)              # compiled once: no per-dtype twins
    # the limits are the header's, exported like SAMPLE_MAX_V, and hold "###"-class strings with a wide margin
    assert (ops.STOP_MAX_STRINGS, ops.STOP_MAX_BYTES, ops.STOP_MAX_TOKEN_BYTES, ops.STOP_MAX_WINDOW) == tuple(
        lib.DEFINES["ULL_STOP_MAX_" + n] for n in ("STRINGS", "BYTES", "TOKEN_BYTES", "WINDOW"))
    assert ops.STOP_MAX_STRINGS >= 24 and ops.STOP_MAX_BYTES >= 64 and ops.STOP_MAX_WINDOW >= ops.STOP_MAX_TOKEN_BYTES + ops.STOP_MAX_BYTES - 1


def test_entry_refuses_bad_arguments_before_any_launch():
    """Null pointers, sizes out of range, an empty stop string: ULL_ERR_ARG; more strings, a longer string or a longer token than the limits:
    ULL_ERR_SHAPE; R == 0: ULL_OK.  The stop offsets are host memory and are really read; no device pointer is dereferenced on these paths
    (no device exists here)."""
    lib = pkg("_lib")
    fn = getattr(lib.load(), "ull_stop_strings")
    D = lib.DEFINES
    ARG, SHAPE = D["ULL_ERR_ARG"], D["ULL_ERR_SHAPE"]
    S_MAX, B_MAX, T_MAX = D["ULL_STOP_MAX_STRINGS"], D["ULL_STOP_MAX_BYTES"], D["ULL_STOP_MAX_TOKEN_BYTES"]
    p = 4096                                                       # any non-null address

    def offsets(lens):
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        return (ctypes.c_int32 * len(off))(*off)

    good = dict(ids=p, ids_ld=16, R=2, L0=3, cur_len=5, tok_off=p, tok_bytes=p, V=100, n_tok_bytes=400, max_tok=8, lens=[3, 4], stop_bytes=p, live=p,
                alive=p)

    def call(**kw):
        a = dict(good, **kw)
        off = a.get("stop_off", offsets(a["lens"]))
        return fn(a["ids"], a["ids_ld"], a["R"], a["L0"], a["cur_len"], a["tok_off"], a["tok_bytes"], a["V"], a["n_tok_bytes"], a["max_tok"],
                  None if off is None else ctypes.cast(off, ctypes.c_void_p), a["stop_bytes"], a.get("S", len(a["lens"])), a["live"], a["alive"], None)

    for bad in (dict(ids=None), dict(tok_off=None), dict(tok_bytes=None), dict(stop_off=None), dict(stop_bytes=None), dict(live=None),
                dict(alive=None), dict(R=-1), dict(ids_ld=-1), dict(L0=-1), dict(cur_len=3), dict(cur_len=2), dict(cur_len=17), dict(V=0),
                dict(n_tok_bytes=-1), dict(max_tok=-1), dict(S=0), dict(lens=[3, 0]), dict(lens=[0]),
                dict(stop_off=(ctypes.c_int32 * 3)(1, 4, 8))):
        assert call(R=0, **bad) == ARG if "R" not in bad else call(**bad) == ARG, bad
    for bad in (dict(lens=[1] * (S_MAX + 1)), dict(lens=[3, B_MAX + 1]), dict(max_tok=T_MAX + 1)):
        assert call(R=0, **bad) == SHAPE, bad
    # the largest of each is taken (R == 0: the checks pass, nothing is launched)
    assert call(R=0) == 0 and call(R=0, lens=[B_MAX] * S_MAX, max_tok=T_MAX) == 0


# ---- the public surface ---------------------------------------------------------------------------------------------------------------------
def test_where_the_keywords_stand():
    """evaluate(): two named parameters in front of `ngram_ban` (its first seven and everything from `ngram_ban` on are pinned by earlier
    tests), default None.  generate(): read from **kwargs by keyword, like `past_key_values` (`output_logprobs` stays the last named one)."""
    MC, MU, G = pkg("modeling_core"), pkg("modeling_ullava"), pkg("generation")
    names = list(inspect.signature(MU.UllavaForCausalLM.evaluate).parameters)
    i = names.index("stop_strings")
    assert names[i:i + 3] == ["stop_strings", "tokenizer", "ngram_ban"] and names[i - 1] == "kv_cache_dtype"
    ev = inspect.signature(MU.UllavaForCausalLM.evaluate).parameters
    assert ev["stop_strings"].default is None and ev["tokenizer"].default is None
    assert "stop_strings" in MC.UllavaCoreForCausalLM.generate.__doc__ and "stop_strings" in MU.UllavaForCausalLM.evaluate.__doc__
    cg = inspect.signature(G.check_generate_args).parameters
    assert cg["stop_strings"].default is None and cg["tokenizer"].default is None
    src = inspect.getsource(MU.UllavaForCausalLM.evaluate)
    assert src.index("stop_strings") < src.index("check_generate_args(") < src.index("_visual_embs_tm(")


class _FakeTok:
    """stands for a tokenizer where only its presence matters (the refusals come before it is used)."""


LONG = "x" * 65
REFUSALS = [
    ("no tokenizer", dict(stop_strings="###"), ValueError, "tokenizer"),
    ("not a string", dict(stop_strings=3, tokenizer=_FakeTok()), ValueError, "str or a non-empty list of str"),
    ("a list with a non-string", dict(stop_strings=["###", 3], tokenizer=_FakeTok()), ValueError, "str or a non-empty list of str"),
    ("an empty list", dict(stop_strings=[], tokenizer=_FakeTok()), ValueError, "str or a non-empty list of str"),
    ("an empty string", dict(stop_strings=["###", ""], tokenizer=_FakeTok()), ValueError, "empty string"),
    ("U+FFFD", dict(stop_strings="a\ufffdb", tokenizer=_FakeTok()), ValueError, "U\\+FFFD"),
    ("too many strings", dict(stop_strings=[f"s{i}" for i in range(33)], tokenizer=_FakeTok()), ValueError, "ULL_STOP_MAX_STRINGS"),
    ("too long a string", dict(stop_strings=["###", LONG], tokenizer=_FakeTok()), ValueError, "ULL_STOP_MAX_BYTES"),
    ("too long in UTF-8", dict(stop_strings=["日" * 22], tokenizer=_FakeTok()), ValueError, "limit of 64"),
    ("beam search", dict(stop_strings="###", tokenizer=_FakeTok(), num_beams=2), ValueError, "num_beams=2 does not combine with `stop_strings`"),
    ("prompt lookup", dict(stop_strings="###", tokenizer=_FakeTok(), prompt_lookup_num_tokens=4, use_cache=True), ValueError,
     "does not combine with prompt-lookup"),
    ("CPU ids", dict(stop_strings="###", tokenizer=_FakeTok()), RuntimeError, "`stop_strings` needs GPU tensors"),
    ("CPU ids, next to a criterion", dict(stop_strings=["###"], tokenizer=_FakeTok(), stopping_criteria=[lambda ids, scores: False]), RuntimeError,
     "`stop_strings` needs GPU tensors"),
]


@pytest.mark.parametrize("what,kw,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_generate_refuses_before_any_device_work(what, kw, exc, match):
    """A CPU model and CPU ids: anything that got past the checks would fail with another error (no CPU path exists).  On the parent commit
    every one of these is the TypeError of an unknown keyword."""
    with pytest.raises(exc, match=match):
        _tiny_core().generate(input_ids=IDS, max_new_tokens=2, **kw)


@pytest.mark.parametrize("what,kw,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_generate_args_is_where_the_refusals_live(what, kw, exc, match):
    G = pkg("generation")
    with pytest.raises(exc, match=match):
        G.check_generate_args(IDS, return_dict_in_generate=True, config_use_cache=False, **kw)


def test_refusals_keep_their_order_and_unknown_keywords_still_raise():
    G = pkg("generation")
    both = dict(stop_strings="###", tokenizer=_FakeTok(), num_beams=2, prompt_lookup_num_tokens=4, use_cache=True)
    with pytest.raises(ValueError, match="num_beams=2 does not combine with `stop_strings`"):      # beams before prompt lookup
        G.check_generate_args(IDS, config_use_cache=True, **both)
    with pytest.raises(ValueError, match="tokenizer"):                                             # the strings themselves before either
        G.check_generate_args(IDS, config_use_cache=True, **dict(both, tokenizer=None))
    with pytest.raises(ValueError, match="unknown sampler"):                                       # ... and behind the older options' refusals
        G.check_generate_args(IDS, config_use_cache=True, sampler="nonsense", stop_strings="")
    # a tokenizer alone switches nothing on; off is off
    assert G.check_generate_args(IDS, config_use_cache=False, tokenizer=_FakeTok()) == G.check_generate_args(IDS, config_use_cache=False)
    assert G.check_stop_strings(None, None) is None and G.check_stop_strings("é#", _FakeTok()) == ["é#".encode()]
    for name in ("stop_string", "stop", "repetition_penalty"):
        with pytest.raises(TypeError, match=name):
            _tiny_core().generate(input_ids=IDS, max_new_tokens=2, stop_strings="###", tokenizer=_FakeTok(), **{name: 1})


def test_evaluate_forwards_both_keywords_to_the_checks():
    MU = pkg("modeling_ullava")
    self = object.__new__(MU.UllavaForCausalLM)                    # the refusals come before the model is touched
    with pytest.raises(ValueError, match="tokenizer"):
        MU.UllavaForCausalLM.evaluate(self, None, None, None, None, None, stop_strings="###")
    with pytest.raises(ValueError, match="empty string"):
        MU.UllavaForCausalLM.evaluate(self, None, None, None, None, None, stop_strings=[""], tokenizer=_FakeTok())
    with pytest.raises(ValueError, match="does not combine with `stop_strings`"):
        MU.UllavaForCausalLM.evaluate(self, None, None, None, None, None, stop_strings="###", tokenizer=_FakeTok(), num_beams=2)


def test_ops_refusals_before_device_work():
    ops = pkg("ops")
    off, data = torch.tensor([0, 1, 3], dtype=torch.int32), torch.tensor([65, 66, 67], dtype=torch.uint8)
    table = ops.StopTable(off, data, "cpu")
    assert (table.V, table.n_bytes, table.max_token_bytes) == (2, 3, 2)
    stops = ops.StopStrings([b"###"], "cpu")
    assert stops.offsets.tolist() == [0, 3] and stops.offsets.dtype == torch.int32 and not stops.offsets.is_cuda
    ids, live, alive = torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.stop_strings(ids, 1, 3, table, stops, live, alive)
    for bad, match in (([b"x"] * (ops.STOP_MAX_STRINGS + 1), "ULL_STOP_MAX_STRINGS"), ([b"x" * (ops.STOP_MAX_BYTES + 1)], "ULL_STOP_MAX_BYTES"),
                       ([b"ab", b""], "none of them empty"), ([], "at least one")):
        with pytest.raises(ValueError, match=match):
            ops.StopStrings(bad, "cpu")
    assert len(ops.StopStrings([b"x" * ops.STOP_MAX_BYTES] * ops.STOP_MAX_STRINGS, "cpu").stops) == ops.STOP_MAX_STRINGS
    n = ops.STOP_MAX_TOKEN_BYTES + 1
    with pytest.raises(ValueError, match="ULL_STOP_MAX_TOKEN_BYTES"):
        ops.StopTable(torch.tensor([0, n], dtype=torch.int32), torch.zeros(n, dtype=torch.uint8), "cpu")
    ops.StopTable(torch.tensor([0, n - 1], dtype=torch.int32), torch.zeros(n - 1, dtype=torch.uint8), "cpu")
    for o, d in ((off.long(), data), (off, data.long()), (torch.tensor([1, 3], dtype=torch.int32), data), (torch.tensor([0, 2, 1, 3], dtype=torch.int32), data),
                 (torch.tensor([0, 2], dtype=torch.int32), data)):
        with pytest.raises(RuntimeError, match="StopTable"):
            ops.StopTable(o, d, "cpu")


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_token_byte_table_entries():
    tok, table = _tok()
    off, data = table
    V = len(tok) + 5
    assert off.dtype == torch.int32 and tuple(off.shape) == (V + 1,) and data.dtype == torch.uint8 and int(off[0]) == 0 and int(off[-1]) == data.numel()
    assert sorted(tok.all_special_ids) == [0, 1, 2] and all(_bytes(table, i) == b"" for i in (0, 1, 2))          # <unk> <s> </s>
    assert all(_bytes(table, i) == b"" for i in range(len(tok), V))                                             # padded embedding rows
    assert all(_bytes(table, byte_id(b)) == bytes([b]) for b in range(256))                                     # <0xXX>: that one raw byte
    # a piece in context: `▁` is a space and nothing is stripped; a multi-byte character is its UTF-8
    for piece in PIECES:
        assert _bytes(table, piece_id(piece)) == piece.replace("▁", " ").encode("utf-8"), piece
    assert _bytes(table, piece_id("▁###")) == b" ###" and _bytes(table, piece_id("日")) == "日".encode() == bytes(_bytes(table, i)[0] for i in utf8_ids("日"))
    # a smaller V cuts the table, a tokenizer flagged-special added token gives nothing
    G = pkg("generation")
    small = G.token_byte_table(tok, 10)
    assert tuple(small[0].shape) == (11,) and small[0].tolist() == off[:11].tolist()
    grown = build_tokenizer()
    grown.add_tokens(["[SEG]"], special_tokens=True)
    grown.add_tokens(["plain"])
    t2 = G.token_byte_table(grown, len(grown))
    assert _bytes(t2, len(grown) - 2) == b"" and _bytes(t2, len(grown) - 1) == b"plain"


def test_token_byte_table_spells_what_decode_spells():
    """On random rows of valid text the table's bytes are tokenizer.decode(row, skip_special_tokens=True), up to the ONE leading space that
    decode strips from the whole text."""
    tok, table = _tok()
    rng = random.Random(5)
    stripped = 0
    for _ in range(400):
        row = random_row(rng, rng.randint(1, 12), valid_text=True)
        mine = b"".join(_bytes(table, i) for i in row)
        ref = tok.decode(row, skip_special_tokens=True).encode("utf-8")
        assert mine in (ref, b" " + ref), (row, mine, ref)
        stripped += mine != ref
    assert stripped >= 10


def test_stop_table_is_kept_per_tokenizer_and_rebuilt_when_a_size_changes():
    G = pkg("generation")
    model = _tiny_core()
    tok, other = build_tokenizer(), build_tokenizer()
    a = G.stop_table(model, tok, "cpu")
    assert G.stop_table(model, tok, "cpu") is a and a.V == model.config.vocab_size
    assert G.stop_table(model, other, "cpu") is not a and G.stop_table(model, tok, "cpu") is a
    assert type(model._stop_tables) is dict and len(model._stop_tables) == 2
    tok.add_tokens(["[NEW]"])
    b = G.stop_table(model, tok, "cpu")
    assert b is not a and G.stop_table(model, tok, "cpu") is b
    model.config.vocab_size += 8                                   # (what resize_token_embeddings leaves behind)
    c = G.stop_table(model, tok, "cpu")
    assert c is not b and c.V == model.config.vocab_size and len(model._stop_tables) == 2


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------
STOP_SETS = [["#"], ["###"], ["#x#"], ["# #"], ["é"], ["##x", "the"]]      # one byte, "###", spanning three tokens, a space inside, multi-byte, two


def _keywords_stop(crit_cls, tok, stops, row):
    """the reference criterion run step by step on a batch-1 row behind a 4-id prompt -> the number of generated tokens at which it fires."""
    prompt = torch.full((1, 4), piece_id("###"), dtype=torch.int64)            # (a prompt that holds a stop string: it never counts)
    crit = crit_cls(stops, tok, prompt)
    for j in range(1, len(row) + 1):
        if crit(torch.cat([prompt, torch.tensor([row[:j]])], 1), None):
            return j
    return None


def test_rule_against_keywords_stopping_criteria():
    """3000 seeded rows of 1-12 ids, invalid byte runs included, six stop sets.  The stop position is the reference criterion's in every
    case but one kind: the criterion's first call only records the prompt length, so a string wholly inside the FIRST generated token
    stops there by this rule (n = 1) and one token later (or, on a one-token row, never) by the criterion."""
    G, T = pkg("generation"), pkg("tools")
    tok, table = _tok()
    rng = random.Random(0)
    n_rows, stopped, corner, invalid = 3000, 0, 0, 0
    for k in range(n_rows):
        row = random_row(rng, rng.randint(1, 12))
        stops = STOP_SETS[k % len(STOP_SETS)]
        mine = G.stop_strings_reference([piece_id("###")] * 4 + row, 4, table, stops)
        theirs = _keywords_stop(T.KeywordsStoppingCriteria, tok, stops, row)
        stopped += mine is not None
        invalid += "\ufffd" in tok.decode(row, skip_special_tokens=True)
        if mine != theirs:
            corner += 1
            assert mine == 1 and G.stop_strings_reference(row[:1], 0, table, stops) == 1, (row, stops, mine, theirs)
            assert theirs == (2 if len(row) > 1 else None), (row, stops, mine, theirs)
    print(f"{n_rows} rows: {stopped} stop ({100 * stopped / n_rows:.0f} %), {corner} first-token differences, {invalid} rows with bytes that are no UTF-8")
    assert corner >= 1 and stopped >= n_rows // 5 and invalid >= 100


def test_the_documented_differences_from_the_reference_criterion():
    """Beside the first-token corner: (1) decode strips one leading space of the WHOLE text, so a stop string that begins with a space can
    match here at the very start where the criterion sees no space; (2) the decoder judges a run of byte tokens as a whole and turns all
    of it into U+FFFD when it is not valid UTF-8 -- a good character spelled in byte tokens next to a bad byte (or next to a character
    still being assembled) is text here and is lost there."""
    G, T = pkg("generation"), pkg("tools")
    tok, table = _tok()
    row = [piece_id("a"), piece_id("▁###"), piece_id("a"), piece_id("b")]
    assert G.stop_strings_reference(row, 0, table, [" ###"]) == 2 == _keywords_stop(T.KeywordsStoppingCriteria, tok, [" ###"], row)
    lead = [piece_id("▁###"), piece_id("a"), piece_id("▁###"), piece_id("b")]
    assert G.stop_strings_reference(lead, 0, table, [" ###"]) == 1 and _keywords_stop(T.KeywordsStoppingCriteria, tok, [" ###"], lead) == 3
    bad_run = [piece_id("a"), piece_id("b"), byte_id(0xF2)] + utf8_ids("é") + [piece_id("a")]
    assert G.stop_strings_reference(bad_run, 0, table, ["é"]) == 5 and _keywords_stop(T.KeywordsStoppingCriteria, tok, ["é"], bad_run) is None
    assembling = [byte_id(0x23)] + utf8_ids("日") + [piece_id("a")]           # (the first-token corner, drawn out until the character is whole)
    assert G.stop_strings_reference(assembling, 0, table, ["#"]) == 1 and _keywords_stop(T.KeywordsStoppingCriteria, tok, ["#"], assembling) == 4


def test_rule_against_hf_stop_string_criteria():
    """transformers' StopStringCriteria knows no prompt (L0 = 0), keeps the text of special tokens and sees a byte token as a string of its
    own, so the two definitions are held together where both speak of the same text: rows of pieces and ASCII byte tokens."""
    from transformers.generation.stopping_criteria import StopStringCriteria
    G = pkg("generation")
    tok, table = _tok()
    crits = [StopStringCriteria(tok, stops) for stops in STOP_SETS]
    rng = random.Random(1)
    n = stopped = 0
    for k in range(600):
        row = [t for t in random_row(rng, rng.randint(1, 12), valid_text=True) if t >= FIRST_PIECE or N_SPECIAL <= t < N_SPECIAL + 0x80]
        if not row:
            continue
        mine = G.stop_strings_reference(row, 0, table, STOP_SETS[k % len(STOP_SETS)])
        theirs = next((j for j in range(1, len(row) + 1) if bool(crits[k % len(STOP_SETS)](torch.tensor([row[:j]]), None)[0])), None)
        assert mine == theirs, (row, STOP_SETS[k % len(STOP_SETS)], mine, theirs)
        n, stopped = n + 1, stopped + (mine is not None)
    assert n >= 500 and stopped >= n // 5


def test_rule_details():
    G = pkg("generation")
    tok, table = _tok()
    h, hh, x = piece_id("#"), piece_id("##"), piece_id("x")
    ref = lambda row, L0, stops: G.stop_strings_reference(row, L0, table, stops)               # noqa: E731
    assert ref([h, h, h], 0, ["###"]) == 3 and ref([h, hh, x], 0, ["###"]) == 2 and ref([x, piece_id("x##y")], 0, ["x#"]) == 2
    assert ref([h, h, h], 1, ["###"]) is None and ref([h, h, h, h], 1, ["###"]) == 3          # text before L0 never counts
    assert ref([h, 1, -100, 10 ** 6, hh], 0, ["###"]) == 5                                     # zero-byte ids are stepped over
    assert ref([x, x], 0, ["###", "x"]) == 1 and ref([], 0, ["x"]) is None and ref([x], 1, ["x"]) is None
    assert ref([h, hh], 0, [b"###"]) == 2                                                      # bytes are taken as they are
