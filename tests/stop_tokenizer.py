"""A LLaMA-shaped tokenizer built in-process for the stop-string tests (nothing is downloaded): BPE with byte fallback, the specials
<unk> <s> </s>, the 256 byte tokens <0x00> .. <0xFF>, then a few dozen pieces, and LLaMA's decoder -- Replace("▁", " "), ByteFallback, Fuse,
Strip(" ", 1, 0) -- wrapped in PreTrainedTokenizerFast with clean_up_tokenization_spaces=False.  Only decoding is exercised (and the
one-token encodings KeywordsStoppingCriteria asks for), so there are no merges.  Not a conftest: the tests import it by name."""
import random

PIECES = ["#", "##", "###", "▁###", "▁", "a", "b", "c", "d", "e", "f", "ab", "abc", "▁a", "▁ab", "▁the", "the", "▁cat", "cat", "s", "▁s", ".", "▁.", ",",
          "\n", "\n\n", "#\n", "é", "▁é", "né", "日", "本", "▁日本", "€", "x#", "#x", "##x", "x##y", "▁x", "x", "y", "z", "stop", "▁stop", "st", "op",
          "HUMAN", "▁HUMAN", ":", "▁:", "a#", "#a#", "ASSISTANT"]
N_SPECIAL, N_BYTES = 3, 256
FIRST_PIECE = N_SPECIAL + N_BYTES


def build_tokenizer(vocab_size=None, pieces_first=False):
    """-> PreTrainedTokenizerFast.  vocab_size: pad the vocabulary with filler pieces `<fill_i>` up to that many ids (for a model whose
    vocabulary is larger); None: specials + bytes + PIECES.  pieces_first: the pieces stand before the byte tokens, so that a model with
    a vocabulary of a hundred ids emits pieces of several bytes (byte_id / piece_id below speak of the default order only)."""
    from tokenizers import Tokenizer, decoders, models, normalizers
    from transformers import PreTrainedTokenizerFast
    byte_tokens = [f"<0x{b:02X}>" for b in range(N_BYTES)]
    tokens = ["<unk>", "<s>", "</s>"] + (PIECES + byte_tokens if pieces_first else byte_tokens + PIECES)
    if vocab_size is not None:
        tokens += [f"<fill_{i}>" for i in range(len(tokens), vocab_size)]
    vocab = {t: i for i, t in enumerate(tokens)}
    assert len(vocab) == len(tokens)
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[], unk_token="<unk>", byte_fallback=True, fuse_unk=True))
    tok.normalizer = normalizers.Replace(" ", "▁")
    tok.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse(), decoders.Strip(" ", 1, 0)])
    return PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", bos_token="<s>", eos_token="</s>", clean_up_tokenization_spaces=False)


def byte_id(b: int) -> int:
    return N_SPECIAL + b


def piece_id(piece: str) -> int:
    return FIRST_PIECE + PIECES.index(piece)


def utf8_ids(text: str):
    """the byte tokens that spell `text` (a multi-byte character as byte tokens)."""
    return [byte_id(b) for b in text.encode("utf-8")]


def random_row(rng: random.Random, n_ids: int, valid_text: bool = False):
    """n_ids random ids: mostly pieces (the `#` family often, so that stop strings occur), now and then a special id, and runs of byte
    tokens -- a whole character (ASCII or multi-byte) or, unless valid_text, one or two bytes that are no UTF-8.  Every byte run stands
    alone: a piece follows it before the next one.  (The decoder judges a run of byte tokens as a whole and turns ALL of it into U+FFFD
    when it is not valid UTF-8, so a good character next to a bad byte is lost there; test_stop_strings_cpu.py shows that difference on
    rows of its own.)  The cut at n_ids may leave a character's first bytes at the end: an invalid run as well."""
    row, piece_since_run = [], True
    while len(row) < n_ids:
        u = rng.random()
        if u < 0.35:
            row.append(piece_id(rng.choice(["#", "##", "###", "▁###", "x#", "#x", "##x", "a#", "#a#", "#\n", "x##y"])))
            piece_since_run = True
        elif u < 0.75 or not piece_since_run:
            row.append(rng.randrange(FIRST_PIECE, FIRST_PIECE + len(PIECES)))
            piece_since_run = True
        elif u < 0.93:
            if valid_text or u < 0.86:
                row.extend(utf8_ids(rng.choice(["é", "日", "€", "#", " ", "a"])))
            else:
                row.extend(byte_id(rng.choice([0x80, 0xA9, 0xBF, 0xF8, 0xFF])) for _ in range(rng.randint(1, 2)))
            piece_since_run = False
        else:
            row.append(rng.randrange(N_SPECIAL))
    del row[n_ids:]
    if valid_text:
        while row and N_SPECIAL + 0x80 <= row[-1] < FIRST_PIECE:     # a character cut by the length limit is no valid text
            row.pop()
    return row
