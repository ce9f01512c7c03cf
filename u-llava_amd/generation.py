"""Decoding for UllavaCoreForCausalLM.generate(): the HF rules restated on the host (sampling warpers, n-gram ban, prompt-lookup draft), every
refusal of generate()'s / evaluate()'s arguments in one function, and the three decode loops -- host per-step, fused on the device, prompt-lookup
-- over what they share (`Decoding`: the step's forward, the stopping test, the result).  The loops take the model; no model class is imported."""
import re
from typing import Optional

import torch

from . import ops
from .kv_cache import KVCache, _check_kv_dtype


class GenerateOutput(dict):
    __getattr__ = dict.__getitem__


def no_repeat_ngram_banned_tokens(rows, ngram_size: int):
    """transformers' NoRepeatNGramLogitsProcessor rule (generation/logits_process.py `_calc_banned_ngram_tokens`; reference
    models/ullava.py:360 forwards `no_repeat_ngram_size` to HF generate): for every row (list of ids so far, prompt included), the tokens
    that followed an earlier occurrence of the row's last ngram_size - 1 tokens.  Host-side integer bookkeeping, like HF's."""
    out = []
    for toks in rows:
        cur = len(toks)
        if ngram_size <= 0 or cur + 1 < ngram_size:
            out.append([])
            continue
        prefix = tuple(toks[cur + 1 - ngram_size:cur])
        banned = []
        for i in range(cur - ngram_size + 1):
            if tuple(toks[i:i + ngram_size - 1]) == prefix:
                banned.append(toks[i + ngram_size - 1])
        out.append(banned)
    return out


_BYTE_TOKEN = re.compile(r"<0x([0-9A-Fa-f]{2})>")


def token_byte_table(tokenizer, vocab_size: int):
    """The bytes every id contributes to the decoded text -> (offsets int32 [V + 1], bytes uint8 [n]), V = vocab_size: id t gives
    bytes[offsets[t]:offsets[t + 1]].  A regular token gives the UTF-8 of its string IN CONTEXT, by the trick of transformers'
    StopStringCriteria (generation/stopping_criteria.py, `clean_tokenizer_vocab`): convert_tokens_to_string(prefix tokens + [token]) minus
    what the prefix alone gives, so a LLaMA piece's `▁` becomes a space and the decoder's strip of the text's first space does not reach it.
    A byte-fallback token `<0xXX>` gives that one raw byte (two of them may form a character no single one decodes to).  A special id
    (tokenizer.all_special_ids, and added tokens flagged special) gives nothing -- the `skip_special_tokens=True` of the reference's
    criterion (models/tools.py:28) -- and so does an id >= len(tokenizer): the padded rows of a resized embedding."""
    V = int(vocab_size)
    special = {int(i) for i in tokenizer.all_special_ids}
    special |= {int(i) for i, t in getattr(tokenizer, "added_tokens_decoder", {}).items() if getattr(t, "special", False)}
    prefix = tokenizer.convert_ids_to_tokens(tokenizer("abcdef", add_special_tokens=False)["input_ids"])
    head = tokenizer.convert_tokens_to_string(prefix)
    pieces = []
    for t, tok in enumerate(tokenizer.convert_ids_to_tokens(list(range(min(V, len(tokenizer)))))):
        m = None if tok is None else _BYTE_TOKEN.fullmatch(tok)
        if tok is None or t in special:
            pieces.append(b"")
        elif m:
            pieces.append(bytes([int(m.group(1), 16)]))
        else:
            text = tokenizer.convert_tokens_to_string(prefix + [tok])
            if not text.startswith(head):
                raise ValueError(f"token_byte_table: token {t} ({tok!r}) changes the text in front of it: its bytes in context are not defined")
            pieces.append(text[len(head):].encode("utf-8"))
    pieces += [b""] * (V - len(pieces))
    offsets = torch.zeros(V + 1, dtype=torch.int32)
    offsets[1:] = torch.tensor([len(p) for p in pieces], dtype=torch.int64).cumsum(0).to(torch.int32)
    return offsets, torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8) if offsets[-1] else torch.zeros(0, dtype=torch.uint8)


def stop_strings_reference(ids_row, L0: int, table, stops):
    """generate(stop_strings=)'s rule on one row, on the host: the definition ops.stop_strings is held against.  ids_row: the row's ids,
    prompt included; only ids_row[L0:], the generated ones, count (as in the reference's criterion and its `outputs.endswith(stop_str)`
    clean-up).  table: token_byte_table's pair; stops: str or bytes.  The row's text is the concatenation of the table bytes of its
    generated ids (an id outside [0, V) gives nothing).  -> n (1-based), the first generated token for which some stop string occurs in
    the text with its LAST byte inside token n's bytes -- the token that completes the string is kept, as HF and the reference keep
    it -- or None.  Checked from the first generated token on."""
    offsets, data = table
    offsets, data = offsets.tolist(), bytes(data.tolist())
    V = len(offsets) - 1
    stops = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in stops]
    text = b""
    for n, t in enumerate(list(ids_row)[L0:], 1):
        t = int(t)
        start = len(text)
        if 0 <= t < V:
            text += data[offsets[t]:offsets[t + 1]]
        for s in stops:
            # an occurrence that ends behind `start`: it begins at start - len(s) + 1 or later
            if len(text) > start and text.find(s, max(0, start - len(s) + 1)) >= 0:
                return n
    return None


def check_stop_strings(stop_strings, tokenizer):
    """generate()'s `stop_strings` / `tokenizer` (HF's names and HF's errors) -> the UTF-8 of the strings, or None when the feature is off."""
    if stop_strings is None:
        return None
    if tokenizer is None:
        raise ValueError("`stop_strings` needs the `tokenizer` the ids come from: pass `tokenizer=` to generate() (a stop string is text, "
                         "and only the tokenizer knows the text of a token)")
    strings = [stop_strings] if isinstance(stop_strings, str) else list(stop_strings) if isinstance(stop_strings, (list, tuple)) else None
    if not strings or not all(isinstance(s, str) for s in strings):
        raise ValueError(f"`stop_strings` has to be a str or a non-empty list of str, but is {stop_strings!r}")
    if any(s == "" or "\ufffd" in s for s in strings):
        raise ValueError("`stop_strings` must not hold an empty string (it would stop every row at once) or U+FFFD (the replacement "
                         "character stands for bytes that are not text: no token sequence spells it)")
    stops = [s.encode("utf-8") for s in strings]
    if len(stops) > ops.STOP_MAX_STRINGS:
        raise ValueError(f"`stop_strings` holds {len(stops)} strings, above the limit of {ops.STOP_MAX_STRINGS} (ULL_STOP_MAX_STRINGS)")
    if max(len(s) for s in stops) > ops.STOP_MAX_BYTES:
        raise ValueError(f"a stop string of {max(len(s) for s in stops)} bytes (UTF-8) is above the limit of {ops.STOP_MAX_BYTES} (ULL_STOP_MAX_BYTES)")
    return stops


def _tokenizer_size(tokenizer):
    """What changes whenever len(tokenizer) does.  A tokenizer grows through added tokens only, and on a fast tokenizer of 32 000 ids
    len() itself costs 4-5 ms (measured, transformers 5.15: the backend counts the whole vocabulary), which a 64-token batch-1 call would pay
    as 60 us per token; the base size and the number of added tokens cost microseconds."""
    added = getattr(tokenizer, "added_tokens_decoder", None)
    return len(tokenizer) if added is None else (tokenizer.vocab_size, len(added))


def stop_table(model, tokenizer, device):
    """The ops.StopTable of `tokenizer` on `device`, built on first use and kept on the model under the tokenizer's identity; rebuilt when
    len(tokenizer) (`_tokenizer_size`) or the model's vocabulary size has changed since (the resize helpers of tools.py grow both).  One
    plain dict."""
    tables = model.__dict__.setdefault("_stop_tables", {})
    key = (_tokenizer_size(tokenizer), int(model.config.vocab_size), torch.device(device))
    held = tables.get(id(tokenizer))
    if held is None or held[0] is not tokenizer or held[1] != key:
        held = tables[id(tokenizer)] = (tokenizer, key, ops.StopTable(*token_byte_table(tokenizer, key[1]), device))
    return held[2]


def prompt_lookup_candidates(row, num_tokens: int, max_ngram: int, eos_ids, limit: int):
    """The draft of prompt-lookup decoding (transformers generation/candidate_generator.py, PromptLookupCandidateGenerator: what HF
    `generate(prompt_lookup_num_tokens=, max_matching_ngram_size=)` proposes), restated on a plain list; the reference of the device lookup in
    ops.spec_step.  row: the ids so far, prompt included.  For n = min(max_ngram, len(row) - 1) down to 1: the earliest window equal to the
    row's trailing n ids whose continuation is non-empty wins; the continuation is the next min(num_tokens, limit) ids, cut at the end of the
    row and before the first id in eos_ids (what is left may be empty, and is the draft all the same).  No window at any n: no draft.
    limit = max_new_tokens - tokens generated so far - 1: a step never proposes more than it may emit."""
    row = list(row)
    L = len(row)
    want = min(int(num_tokens), int(limit))
    if want <= 0:
        return []
    eos = set() if eos_ids is None else {int(e) for e in eos_ids}
    for n in range(min(int(max_ngram), L - 1), 0, -1):
        tail = row[L - n:]
        for s in range(L - n):                                   # s + n < L: the continuation has at least one id
            if row[s:s + n] == tail:
                out = []
                for tok in row[s + n:min(s + n + want, L)]:
                    if tok in eos:
                        break
                    out.append(tok)
                return out
    return []


def check_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size):
    """generate()'s `prompt_lookup_num_tokens` / `max_matching_ngram_size` -> (k, n-gram size), or None when the feature is off."""
    if prompt_lookup_num_tokens is None:
        if max_matching_ngram_size is not None:
            raise ValueError("`max_matching_ngram_size` is an option of prompt-lookup decoding: it needs `prompt_lookup_num_tokens`")
        return None
    k = int(prompt_lookup_num_tokens)
    if k != prompt_lookup_num_tokens or not 1 <= k <= ops.SPEC_MAX_DRAFT:
        raise ValueError(f"`prompt_lookup_num_tokens` has to be an integer in 1..{ops.SPEC_MAX_DRAFT} (a verify step takes at most "
                         f"{ops.SPEC_MAX_DRAFT + 1} new tokens), but is {prompt_lookup_num_tokens}")
    g = 2 if max_matching_ngram_size is None else int(max_matching_ngram_size)
    if (max_matching_ngram_size is not None and g != max_matching_ngram_size) or g < 1:
        raise ValueError(f"`max_matching_ngram_size` has to be an integer >= 1, but is {max_matching_ngram_size}")
    return k, g


def sampling_probs(logits: torch.Tensor, temperature: float, top_k: Optional[int] = 50, top_p: Optional[float] = None) -> torch.Tensor:
    """The distribution HF `GenerationMixin._sample` draws from, in its own arithmetic and order (transformers generation/logits_process.py:
    TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on fp32 scores, then softmax): the reference's callers pass `temperature`
    (and optionally `top_p`) and inherit `top_k = 50` from GenerationConfig's defaults (models/ullava.py:350-361, inference_ullava_core.py:73-80).
    One `torch.multinomial(probs, 1)` per step on these probabilities consumes the RNG exactly as HF does, so a seeded run draws HF's tokens
    from the same logits.  Integer / fp32 bookkeeping on [B, V] scores (the logits themselves come from the HIP lm_head)."""
    scores = logits.float()
    if temperature is not None and temperature != 1.0:
        scores = scores / temperature
    if top_k is not None and top_k > 0:
        k = min(int(top_k), scores.size(-1))
        scores = scores.masked_fill(scores < torch.topk(scores, k)[0][..., -1, None], float("-inf"))
    if top_p is not None and top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cumulative = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cumulative <= (1 - top_p)
        remove[..., -1:] = 0                                     # min_tokens_to_keep = 1
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), float("-inf"))
    return torch.softmax(scores, dim=-1)


def check_sampler(sampler) -> bool:
    """generate()'s `sampler`: None / "host" = torch's sampling path, "device" = ops.sample_step in the fused loop (True)."""
    if sampler not in (None, "host", "device"):
        raise ValueError(f'unknown sampler {sampler!r} (None / "host": the torch path; "device": one HIP launch per token)')
    return sampler == "device"


def check_ngram_ban(ngram_ban) -> bool:
    """generate()'s `ngram_ban`: None / "host" = the Python rule on seq.tolist() in the host loop, "device" = ops.ngram_ban (True)."""
    if ngram_ban not in (None, "host", "device"):
        raise ValueError(f'unknown ngram_ban {ngram_ban!r} (None / "host": the list rule on the host; "device": one HIP launch per step)')
    return ngram_ban == "device"


def check_num_beams(num_beams, length_penalty=1.0, early_stopping=False, num_return_sequences=1) -> int:
    """generate()'s `num_beams` and the three options that belong to it -> the number of beams (1: no beam search)."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= ops.BEAM_MAX_K:
        raise ValueError(f"`num_beams` has to be an integer in 1..{ops.BEAM_MAX_K}, but is {num_beams!r}")
    if not (early_stopping is False or early_stopping is True or early_stopping == "never"):
        raise ValueError(f'`early_stopping` has to be False, True or "never", but is {early_stopping!r}')
    if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or num_return_sequences < 1:
        raise ValueError(f"`num_return_sequences` has to be a positive integer, but is {num_return_sequences!r}")
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)):
        raise ValueError(f"`length_penalty` has to be a number, but is {length_penalty!r}")
    if num_beams == 1:
        for name, value, default in (("length_penalty", length_penalty, 1.0), ("early_stopping", early_stopping, False),
                                     ("num_return_sequences", num_return_sequences, 1)):
            if value is not default and value != default or isinstance(value, str):
                raise ValueError(f"`{name}={value!r}` is an option of beam search: it needs `num_beams` > 1")
    elif num_return_sequences > num_beams:
        raise ValueError(f"`num_return_sequences` ({num_return_sequences}) has to be at most `num_beams` ({num_beams})")
    return num_beams


def _past_geometry(past):
    """(layers, batch, heads, head_dim, kv_dtype, on the GPU, holds the hidden states of its positions) of generate()'s `past_key_values`:
    a KVCache, or what KVCache.from_hf takes (kv_dtype then None: it is converted to whatever the call asks for).  Host-side reads only."""
    if isinstance(past, KVCache):
        n_layers, B, H, hd, dev, _ = past._geom
        return n_layers, B, H, hd, past.kv_dtype, dev.type == "cuda", sum(h.shape[1] for h in past.last_hidden) == past.length
    if hasattr(past, "key_cache") and hasattr(past, "value_cache"):
        keys = list(past.key_cache)
    elif hasattr(past, "layers"):
        keys = [l.keys for l in past.layers]
    else:
        try:
            keys = [kv[0] for kv in past]
        except TypeError:
            raise TypeError(f"`past_key_values` has to be a KVCache, an HF legacy tuple of (key, value) pairs or a Cache object, not {type(past).__name__}")
    if not keys or not torch.is_tensor(keys[0]) or keys[0].dim() != 4:
        raise ValueError("`past_key_values` entries must be [batch, heads, seq, head_dim] tensors (an empty HF cache: pass an empty KVCache)")
    B, H, _, hd = keys[0].shape
    return len(keys), B, H, hd, None, keys[0].is_cuda, False


def check_past_key_values(past, input_ids, cache_shape=None, kv_cache_dtype=None, output_hidden_states=False, num_beams=1):
    """The refusals of generate(past_key_values=) after `use_cache=False`, in check_generate_args' documented order; no device work."""
    n_layers, B, H, hd, kv_dtype, on_gpu, has_hidden = _past_geometry(past)
    if input_ids is None or input_ids.dim() != 2:
        raise ValueError("`past_key_values` needs `input_ids` [batch, length]: the whole conversation so far, the cached positions included")
    if input_ids.shape[0] != B:
        raise ValueError(f"`past_key_values` holds {B} rows and `input_ids` has {input_ids.shape[0]}")
    if cache_shape is not None and tuple(cache_shape) != (n_layers, H, hd):
        raise ValueError(f"`past_key_values` has (layers, heads, head_dim) = {(n_layers, H, hd)}, the model {tuple(cache_shape)}")
    if isinstance(past, KVCache) and kv_cache_dtype is not None and kv_cache_dtype != kv_dtype:
        raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r} contradicts the cache handed in, which is "
                         f"{'in the model dtype' if kv_dtype is None else repr(kv_dtype)} (leave `kv_cache_dtype` unset)")
    if output_hidden_states and not has_hidden and not (isinstance(past, KVCache) and past.length == 0):
        raise ValueError("output_hidden_states=True needs a cache that holds the last-layer states of its positions; one built from an HF "
                         "cache (KVCache.from_hf) does not")
    if num_beams > 1:
        raise NotImplementedError(f"num_beams={num_beams} does not continue a cache (`past_key_values`): beam search replicates and reorders its own")
    if not input_ids.is_cuda or not on_gpu:
        raise RuntimeError("`past_key_values` needs GPU tensors (no CPU path exists)")


def enter_cache(cache: KVCache, seq, attention_mask, no_pad: bool, need: int, mm_ids=None) -> None:
    """generate()'s entry with a cache handed in (HF's rule: `seq` [B, L] is the whole conversation, the cache covers its first positions):
    the cache is cut to the longest prefix it shares with every row of `seq` (ops.ids_common_prefix against `cache.ids`, one launch and one
    int32 per row read by the host; ids unknown: the caller is trusted), and to L - 1 at most, so that at least one token is fed; the mask
    is held against the one the cache was filled under (one more flag read by the host, only where either mask has a zero); the ids to
    feed must not hold image / video placeholders (one flag, only on models with placeholder ids); and the cache is grown to `need`
    positions.  Up to three small host reads, then; the cache is touched only after the last refusal.  The images are not looked at."""
    B, L = seq.shape
    P = cache.length
    if P:
        ids = cache.ids
        if ids is not None:
            keep = min(ops.ids_common_prefix(seq, ids, min(P, L)).tolist())
        elif P > L:
            raise ValueError(f"`past_key_values` covers {P} positions and `input_ids` has {L} (pass the whole conversation)")
        else:
            keep = P
        keep = min(keep, L - 1)
        if keep > 0 and not (no_pad and cache.mask is None):
            # the kept positions' keys carry the RoPE positions of the mask they were filled under.  A new mask may only clear positions
            # behind a row's last visible kept one (the pad fill behind its EOS): cumsum(mask) - 1 of every key still visible is unchanged
            new = seq.new_ones(B, keep, dtype=torch.bool) if attention_mask is None else attention_mask[:, :keep].ne(0)
            rec = new.new_ones(B, keep) if cache.mask is None else cache.mask[:, :keep].ne(0)
            tail = new.flip(1).cumsum(1).flip(1) == 0
            if bool(((new != rec) & ~tail).any()):
                raise ValueError("`attention_mask` differs from the mask the cache was filled under at a cached position that stays visible "
                                 "(only the pad fill behind a row's last visible cached position may be cleared)")
        if keep and mm_ids:
            mm = torch.as_tensor(sorted(set(int(v) for v in mm_ids)), dtype=seq.dtype, device=seq.device)
            if bool(torch.isin(seq[:, keep:], mm).any()):
                raise NotImplementedError("the ids to feed behind the cached positions hold image / video placeholder ids: images and videos "
                                          "inside a continuation are not implemented (start a new cache)")
        if keep < P:
            cache.truncate(keep)                                 # (behind every refusal: a refused call leaves the cache as it was)
    if need > cache.smax:
        cache.grow(need)


def check_generate_args(input_ids, attention_mask=None, *, do_sample=False, temperature=1.0, num_beams=1, no_repeat_ngram_size=None,
                        use_cache=None, kv_cache_dtype=None, sampler=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=None,
                        output_logprobs=False, return_dict_in_generate=False, unknown=None, dtype=None, vocab_size=None, config_use_cache=None,
                        ngram_ban=None, length_penalty=1.0, early_stopping=False, num_return_sequences=1, stopping_criteria=None,
                        output_hidden_states=False, n_eos=None, past_key_values=None, cache_shape=None, stop_strings=None, tokenizer=None):
    """Every refusal of generate()'s arguments that needs no device work, in generate()'s order; evaluate() calls it too, before it starts
    the SAM encoder on the side stream.  No model is needed: what the model decides comes in as plain values, each read only when the
    option it belongs to is set -- `dtype` with kv_cache_dtype, `vocab_size` with sampler="device" (None: the caller does not know it
    and leaves that one refusal to generate(), which always passes it), `config_use_cache` where use_cache is None.  `unknown`: generate()'s
    **kwargs.  -> (n-gram size or 0, tokens are sampled, on the device, use_cache with the config's default filled in, (k, n-gram size) or None);
    whether the ban runs on the device is check_ngram_ban(ngram_ban), checked here against the other options.  Beam search (num_beams > 1;
    check_num_beams for the option values) is refused with everything its loop does not define -- stopping_criteria, output_hidden_states and
    the number of EOS ids `n_eos` (None: not known) come in for that alone -- and on tensors that are not on the GPU.
    past_key_values (a KVCache, or an HF legacy tuple / Cache object): the call continues an earlier one's cache, which implies use_cache=True;
    refused, in this order: use_cache=False; a cache whose batch is not input_ids', or whose (layers, heads, head_dim) are not the model's
    `cache_shape` (None: not known, left to generate()); a kv_cache_dtype other than the cache's own; output_hidden_states=True on a cache
    that does not hold the hidden states of its positions (from_hf); num_beams > 1; tensors that are not on the GPU.
    stop_strings / tokenizer (check_stop_strings: a str or a list of str with its tokenizer, no empty string, no U+FFFD, within ops.STOP_MAX_STRINGS
    and ops.STOP_MAX_BYTES), behind the refusals of prompt lookup; then refused, in this order: with num_beams > 1; with prompt_lookup_num_tokens
    (a verify step emits several tokens and would have to be cut in the middle); and, last of all, on tensors that are not on the GPU."""
    beams = check_num_beams(num_beams, length_penalty, early_stopping, num_return_sequences)
    if unknown:
        # HF generate() validates its model kwargs and raises on unknown ones; options this loop does not implement must not be
        # swallowed (a silently ignored `repetition_penalty` changes the ids)
        raise TypeError(f"generate() got unsupported keyword arguments {sorted(unknown)} (supported: greedy / sampling with temperature, "
                        "top_k, top_p, no_repeat_ngram_size, stopping_criteria, eos_token_id, pad_token_id, max_new_tokens)")
    if output_logprobs and not return_dict_in_generate:
        raise ValueError("`output_logprobs=True` needs `return_dict_in_generate=True`: the log-probabilities travel in the returned dict")
    ngram = int(no_repeat_ngram_size) if no_repeat_ngram_size else 0
    if ngram < 0:
        raise ValueError(f"`no_repeat_ngram_size` has to be a positive integer, but is {no_repeat_ngram_size}")
    sampling = bool(do_sample and temperature and temperature > 0)
    device_sampler = check_sampler(sampler)
    device_ban = check_ngram_ban(ngram_ban)
    if device_ban and not ngram:
        raise ValueError('ngram_ban="device" is an option of the n-gram ban: it needs `no_repeat_ngram_size` >= 1')
    if device_sampler and ngram and not device_ban:
        raise ValueError('sampler="device" does not combine with `no_repeat_ngram_size` while the n-gram ban is host-side list work '
                         '(use sampler=None, or ngram_ban="device": the ban in one launch, inside the device loop)')
    if device_sampler and sampling and vocab_size is not None and vocab_size > ops.SAMPLE_MAX_V:
        raise ValueError(f'sampler="device" stages a row of logits in LDS: vocab_size {vocab_size} is above its limit of '
                         f"{ops.SAMPLE_MAX_V} (use sampler=None)")
    if past_key_values is not None:
        if use_cache is not None and not use_cache:
            raise ValueError("`past_key_values` needs use_cache=True: the call continues a KV cache (leave `use_cache` unset)")
        use_cache = True                                         # (whatever the config's default is)
        check_past_key_values(past_key_values, input_ids, cache_shape, kv_cache_dtype, output_hidden_states, beams)
    use_cache = config_use_cache if use_cache is None else use_cache
    lookup = check_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size)
    if lookup is not None:
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("prompt-lookup decoding takes a batch of one row (as HF's assisted decoding does), got "
                             f"{None if input_ids is None else tuple(input_ids.shape)}")
        if not use_cache:
            raise ValueError("prompt-lookup decoding needs use_cache=True: a verify step runs over a filled KV cache")
        if ngram:
            # (on the host or on the device alike)
            raise ValueError("prompt-lookup decoding does not combine with `no_repeat_ngram_size`: a draft is the continuation of a repeated "
                             "n-gram, so its first token is what the ban forbids (max_matching_ngram_size >= no_repeat_ngram_size - 1) and "
                             "the pair could only reject drafts")
        if attention_mask is not None and not bool(attention_mask.ne(0).all()):
            raise ValueError("prompt-lookup decoding does not take a padded attention mask (one unpadded row)")
        if sampling and not device_sampler:
            raise ValueError('prompt-lookup decoding with do_sample=True needs sampler="device": its loop picks the tokens on the device')
    if check_stop_strings(stop_strings, tokenizer) is not None:
        if beams > 1:
            raise ValueError(f"num_beams={beams} does not combine with `stop_strings` (a beam is not a row that stops: use `eos_token_id`, or "
                             "num_beams=1)")
        if lookup is not None:
            raise ValueError("`stop_strings` does not combine with prompt-lookup decoding: a verify step emits several tokens and the stop may "
                             "fall between them (drop `prompt_lookup_num_tokens`, or pass a host `stopping_criteria`)")
    if kv_cache_dtype is not None:
        _check_kv_dtype(kv_cache_dtype, dtype)
        if not use_cache:
            raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r} needs use_cache=True: without a KV cache there is nothing to quantize")
    if beams > 1:
        # beam search (beam_loop): deterministic, in its own device loop; what it does not define is refused, with the way out
        for on, what in ((sampling, "do_sample=True with temperature > 0 (beam sampling is not implemented: use do_sample=False)"),
                         (device_sampler, 'sampler="device" (beam search picks by score: leave `sampler` unset)'),
                         (lookup is not None, "prompt-lookup decoding (drop `prompt_lookup_num_tokens`: the beams already share one forward)"),
                         (bool(stopping_criteria), "`stopping_criteria` (HF calls them per candidate row and the reference's criterion answers "
                                                   "with one bool: use `eos_token_id`)"),
                         (output_logprobs, "output_logprobs=True (read `sequences_scores`, or score the result with score())"),
                         (kv_cache_dtype is not None, f"kv_cache_dtype={kv_cache_dtype!r} (the fp8 cache is not reordered: leave it unset)"),
                         (bool(ngram) and not device_ban, '`no_repeat_ngram_size` with the host ban (pass ngram_ban="device")')):
            if on:
                raise ValueError(f"num_beams={beams} does not combine with {what}")
        if output_hidden_states:
            raise NotImplementedError(f"num_beams={beams} does not return hidden states (the rows of a step are reordered by the next one; "
                                      "evaluate() therefore decodes with num_beams=1)")
        kk = ops.beam_candidates(beams, 1 if n_eos is None else n_eos)
        if n_eos is not None and (1 + n_eos) * beams > ops.BEAM_MAX_CAND:
            raise ValueError(f"num_beams={beams} with {n_eos} EOS ids: a step keeps (1 + EOS ids) * num_beams <= {ops.BEAM_MAX_CAND} candidates "
                             "(pass fewer EOS ids or fewer beams)")
        if vocab_size is not None and vocab_size * beams < kk:
            raise ValueError(f"num_beams={beams} needs {kk} candidates per step and vocab_size * num_beams = {vocab_size * beams} is fewer "
                             "(use fewer beams)")
        if input_ids is None or not input_ids.is_cuda:
            raise NotImplementedError("beam search needs GPU tensors (no CPU path exists)")
    for on, what in ((lookup is not None, "prompt-lookup decoding"), (device_sampler and sampling, 'sampler="device"'), (output_logprobs, "output_logprobs"),
                     (device_ban, 'ngram_ban="device"'), (stop_strings is not None, "`stop_strings`")):
        if on and input_ids is not None and not input_ids.is_cuda:
            raise RuntimeError(f"{what} needs GPU tensors (no CPU path exists)")
    return ngram, sampling, device_sampler, use_cache, lookup


class Decoding:
    """One generate() call as its loop sees it: the model, the inputs beside the ids, the KV cache generate() made (None: use_cache off),
    how a token is picked, when to stop, what to return -- and the hidden states collected where there is no cache."""

    def __init__(self, model, images, videos, attention_mask, no_pad, cache, max_new_tokens, sampling, temperature, top_k, top_p, eos_ids, pad,
                 crit, output_hidden_states, keep_last_step_only, output_logprobs):
        self.model, self.images, self.videos, self.attention_mask, self.no_pad, self.cache = model, images, videos, attention_mask, no_pad, cache
        self.sampling, self.temperature, self.top_k, self.top_p = sampling, temperature, top_k, top_p
        self.max_new_tokens, self.eos_ids, self.pad, self.crit = max_new_tokens, eos_ids, pad, crit
        self.output_hidden_states, self.keep_last_step_only, self.output_logprobs = output_hidden_states, keep_last_step_only, output_logprobs
        self.steps_hidden = []
        self.return_cache = False                                # the cache came from the caller (past_key_values): the result names it
        self.continued = bool(cache)                             # ... and held positions at entry: step 0 feeds what lies behind them
        self.stops = None                                        # generate(stop_strings=): (ops.StopTable, ops.StopStrings) on the ids' device

    def forward(self, seq, step: int):
        """The forward of decode step `step` over the ids so far, through prepare_inputs_for_generation.  With a cache:
        step 0 is the prefill that fills it, later steps feed one token and vision does not run again.  Without one (the reference's
        released checkpoints: use_cache=False) every step re-runs the multimodal prefill, and its hidden states are kept when asked for."""
        m = self.attention_mask
        mask = None if self.no_pad else torch.cat([m, m.new_ones(seq.shape[0], seq.shape[1] - m.shape[1])], dim=1)
        if step == 0 and self.continued:
            # a cache handed in with P positions: the ids behind them in one call, many new tokens over a filled cache (no `[:, -1:]` cut,
            # no vision inputs, as in the later steps); the positions come from the full mask, as prepare_inputs_for_generation takes them
            P = self.cache.length
            pos = None
            if mask is not None:
                pos = mask.long().cumsum(-1) - 1
                pos.masked_fill_(mask == 0, 1)
                pos = pos[:, P:]
            return self.model.forward(input_ids=seq[:, P:], attention_mask=mask, position_ids=pos, past_key_values=self.cache, use_cache=True)
        inputs = self.model.prepare_inputs_for_generation(input_ids=seq, attention_mask=mask, images=self.images, videos=self.videos,
                                                          past_key_values=self.cache, use_cache=self.cache is not None)
        if self.cache is not None:
            if step > 0:
                inputs["images"] = inputs["videos"] = None
            return self.model.forward(**inputs)
        out = self.model.forward(**inputs, output_hidden_states=self.output_hidden_states)
        if self.output_hidden_states:
            if self.keep_last_step_only:
                self.steps_hidden.clear()                        # evaluate() only reads hidden_states[-1] (the last step)
            self.steps_hidden.append(out.hidden_states)
        return out

    def stopped(self, ids) -> bool:
        """whether a stopping criterion fires on the ids so far (each criterion reads them on the host)."""
        return any(bool(torch.as_tensor(c(ids, None)).all()) for c in self.crit)

    def result(self, seq, logprobs, return_dict: bool):
        """what generate() returns.  hidden_states with a cache: the tensor the no-cache path returns at its last step -- last-layer states of
        ALL positions fed so far, joined once; without one: every step's (the last step's alone under keep_last_step_only)."""
        if not return_dict:
            return seq
        hidden = None
        if self.output_hidden_states:
            hidden = tuple(self.steps_hidden) if self.cache is None else ((torch.cat(self.cache.last_hidden, dim=1),),) if self.cache else ()
        return GenerateOutput(sequences=seq, hidden_states=hidden, **({} if logprobs is None else dict(logprobs=logprobs)),
                              **(dict(past_key_values=self.cache) if self.return_cache else {}))


def host_loop(d: Decoding, seq, ngram: int, probs=sampling_probs, device_ban: bool = False):
    """One token per step, picked by torch on the host's schedule: the n-gram ban, torch.multinomial on sampling_probs (or argmax), pad fill
    and EOS bookkeeping per row, one host read per step.  probs: generate() hands in the `sampling_probs` of its own module, so that a
    wrapper installed there (the tests record the logits that way) is the one that runs.  device_ban: the ban is ops.ngram_ban on the
    model-dtype logits (-inf where the list rule puts it, the same fp32 values after .float()) instead of tolist() + the Python rule + one
    indexed store per row.  d.stops (stop_strings): ops.stop_strings on the ids after the token is appended, folded into `unfinished`.
    -> (ids, logprobs or None)"""
    B, L0 = seq.shape
    unfinished = torch.ones(B, dtype=torch.bool, device=seq.device)
    stop_count = torch.zeros(1, dtype=torch.int32, device=seq.device) if d.stops is not None else None      # (the kernel's counter: not read here)
    lp_cols = []
    for step in range(d.max_new_tokens):
        out = d.forward(seq, step)
        if ngram > 0 and device_ban:
            # the processor below in one launch, into a new tensor: the scored logits stay raw
            logits = ops.ngram_ban(out.logits[:, -1], seq, seq.shape[1], ngram).float()
        else:
            logits = out.logits[:, -1].float()
            if d.output_logprobs and ngram > 0 and logits.dtype == out.logits.dtype:
                logits = logits.clone()                          # an fp32 model: .float() is a view, and the ban must not reach the scored logits
            if ngram > 0:
                # HF NoRepeatNGramLogitsProcessor (logits processors run before the sampling warpers): tokens that would complete an
                # n-gram already present in the row (prompt included) get -inf
                for b_, banned in enumerate(no_repeat_ngram_banned_tokens(seq.tolist(), ngram)):
                    if banned:
                        logits[b_, torch.as_tensor(banned, device=logits.device)] = float("-inf")
        nxt = torch.multinomial(probs(logits, d.temperature, d.top_k, d.top_p), 1) if d.sampling else logits.argmax(-1, keepdim=True)
        if d.pad is not None:
            nxt = torch.where(unfinished.unsqueeze(1), nxt, torch.full_like(nxt, d.pad))      # finished rows: pad fill
        seq = torch.cat([seq, nxt], dim=1)
        if d.output_logprobs:
            # the raw logits (before the n-gram ban and the warpers), masked by `unfinished` as it stood before this step
            lp_cols.append(ops.token_logprobs(out.logits[:, -1], nxt.squeeze(1), unfinished.to(torch.int32)))
        if d.eos_ids is not None:
            unfinished = unfinished & ~torch.isin(nxt.squeeze(1), d.eos_ids)
        if d.stops is not None:
            live = unfinished.to(torch.int32)
            ops.stop_strings(seq, L0, seq.shape[1], d.stops[0], d.stops[1], live, stop_count)
            unfinished = live.bool()
        if (d.eos_ids is not None or d.stops is not None) and not bool(unfinished.any()):
            break
        if d.stopped(seq):
            break
    if not d.output_logprobs:
        return seq, None
    return seq, torch.stack(lp_cols, dim=1) if lp_cols else torch.zeros(B, 0, dtype=torch.float32, device=seq.device)


def fused_loop(d: Decoding, seq, ngram: int = 0):
    """Greedy decoding, or sampler="device", with the whole step on the device: the tokens land in a pre-sized [B, L0 + max_new_tokens]
    buffer, the pick / pad-fill / EOS bookkeeping is ONE kernel (ops.greedy_step / ops.sample_step), and the host looks at the "rows still
    unfinished" counters only every `check` steps (every step when a stopping criterion needs the ids on the host anyway).  Steps that run
    past the point where every row had finished only produce pad tokens; ids, cache and hidden states are trimmed to what a per-step check
    returns.  ngram > 0 (ngram_ban="device"): one more launch per step, ops.ngram_ban, copies the last-position logits into a [B, V] scratch
    with the banned tokens at -inf -- it reads the ids in `buf`, pad fill included, as HF's processor does -- and the pick runs on the
    scratch; the log-probabilities keep scoring the raw logits.  d.stops (stop_strings): one more launch per step behind the pick,
    ops.stop_strings, clears `live` of the rows whose text now holds a stop string and takes them out of the step's counter; the next
    step pad-fills them as it does a row behind its EOS.  -> (ids, logprobs or None)"""
    B, L0 = seq.shape
    n_max, dev = d.max_new_tokens, seq.device
    buf = torch.empty(B, L0 + n_max, dtype=torch.int64, device=dev)
    buf[:, :L0] = seq
    live = torch.ones(B, dtype=torch.int32, device=dev)
    alive = torch.zeros(n_max, dtype=torch.int32, device=dev)
    lp = live_before = None
    if d.output_logprobs:
        # the step kernels update `live` in place and the score needs it as it stood BEFORE the step: a snapshot per step
        lp = torch.zeros(B, n_max, dtype=torch.float32, device=dev)
        live_before = torch.empty_like(live)
    banned = None                                                # the step's logits under the n-gram ban: allocated once, at the first step
    check = d.check = 1 if d.crit else 8                         # (kept on `d`: the tests read how often this call looked at the host)
    n_done = n_tok = 0                                           # tokens appended so far; tokens after which every row had finished
    for step in range(n_max):
        last = d.forward(buf[:, :L0 + step], step).logits[:, -1]
        if lp is not None:
            live_before.copy_(live)
        pick = last
        if ngram > 0:
            if banned is None:
                banned = torch.empty(last.shape, dtype=last.dtype, device=dev)
            pick = ops.ngram_ban(last, buf, L0 + step, ngram, out=banned)
        if d.sampling:
            # torch's noise, drawn as torch.multinomial draws it: the generator moves as it does on the host path
            noise = torch.empty(last.shape, dtype=torch.float32, device=last.device).exponential_()
            ops.sample_step(pick, noise, d.temperature, d.top_k, d.top_p, live, d.eos_ids, d.pad, buf, L0 + step, alive[step:step + 1])
        else:
            ops.greedy_step(pick, live, d.eos_ids, d.pad, buf, L0 + step, alive[step:step + 1])
        if d.stops is not None:
            ops.stop_strings(buf, L0, L0 + step + 1, d.stops[0], d.stops[1], live, alive[step:step + 1])
        if lp is not None:
            ops.token_logprobs(last, buf[:, L0 + step], live_before, out=lp[:, step])
        n_done = n_tok = step + 1
        if d.stopped(buf[:, :L0 + n_done]):
            break
        if (d.eos_ids is not None or d.stops is not None) and (n_done % check == 0 or n_done == n_max):
            dead = (alive[:n_done].cpu() == 0).nonzero()         # the only device -> host read: every `check` steps
            if dead.numel():
                n_tok = int(dead[0]) + 1
                break
    if n_tok < n_done:
        # steps that ran after every row had finished (at most check - 1): drop their states so that the outputs equal a per-step check's
        if d.cache is not None:
            d.cache.truncate(L0 + n_tok - 1)
        if d.steps_hidden and d.keep_last_step_only:
            # the kept step saw L0 + n_done - 1 positions; the reference's last step L0 + n_tok - 1
            d.steps_hidden = [tuple(h[:, :L0 + n_tok - 1] for h in d.steps_hidden[0])]
        else:
            del d.steps_hidden[n_tok:]
    # (the log-probability columns of the steps that ran past the end go as their ids went)
    return buf[:, :L0 + n_tok].contiguous(), None if lp is None else lp[:, :n_tok].clone()


def prompt_lookup_loop(d: Decoding, seq, lookup):
    """generate()'s loop under prompt_lookup_num_tokens (batch 1, KV cache, arguments already checked).  The ids live in one device
    buffer: n valid ids, then the dn drafts of the next step.  A step is one forward over buf[n-1 : n+dn] and ops.spec_step, which emits,
    drafts again and leaves (emitted, finished, dn') for the one host read of the step -- the next forward's length depends on it.
    output_logprobs: after the step, its 1 + dn verify rows are scored against buf[0, n : n+1+dn] into columns n-L0 ... of a buffer with
    buf's k columns of slack; only the first `emitted` are valid, the next step overwrites the rest, and the result is cut at n.  -> (ids, logprobs or None)"""
    k, max_ngram = lookup
    L0 = seq.shape[1]
    n_max, dev = L0 + d.max_new_tokens, seq.device
    buf = torch.empty(1, n_max + k, dtype=torch.int64, device=dev)
    buf[:, :L0] = seq
    picks = torch.empty(16, dtype=torch.int32, device=dev)
    record = torch.empty(3, dtype=torch.int32, device=dev)
    lp = torch.zeros(d.max_new_tokens + k, dtype=torch.float32, device=dev) if d.output_logprobs else None
    n, dn = L0, 0
    first = True
    while n < n_max:
        # the prefill (or, on a cache handed in, the ids behind its positions) through the step forward every loop shares; then the last
        # valid id and the drafts over the filled cache
        out = d.forward(buf[:, :L0], 0) if first else d.model.forward(input_ids=buf[:, n - 1:n + dn], past_key_values=d.cache, use_cache=True)
        first = False
        logits = out.logits[0, -(1 + dn):]
        # torch's noise, one row per verified position, drawn in one call per step
        noise = torch.empty(logits.shape, dtype=torch.float32, device=dev).exponential_() if d.sampling else None
        ops.spec_step(logits, noise, d.temperature, d.top_k, d.top_p, buf, n, dn, n_max, d.eos_ids, k, max_ngram, picks, record)
        if lp is not None:
            # rows 0 .. emitted-1 hold the emitted tokens (a row past them is scored against whatever id sits there: never returned)
            ops.token_logprobs(logits, buf[0, n:n + 1 + dn], out=lp[n - L0:n - L0 + 1 + dn])
        emitted, finished, dn = record.tolist()                  # the step's device -> host read
        n += emitted
        d.cache.truncate(n - 1)                                  # the rejected drafts' positions (and the states of the token not yet fed)
        if finished or d.stopped(buf[:, :n]):
            break
    return buf[:, :n].contiguous(), None if lp is None else lp[:n - L0].unsqueeze(0).clone()


# ------------------------------------------------------------------------------------------------------------------ beam search
BEAM_NEG = -1.0e9


class BeamState:
    """The state of deterministic beam search (HF `GenerationMixin._beam_search`, do_sample=False) for B items of K beams, as tensors on
    `device`: the running ids run [B, K, Lmax] (Lmax = L0 + max_new_tokens, the pad id behind the prompt) with scores run_sc [B, K] =
    [0, -1e9, ...]; the pool of finished hypotheses pool [B, K, Lmax] (copies of the padded prompt), pool_sc = -1e9, pool_len = 0, fin = 0
    (int32); open [B] = 1 (int32): the item's best running beam can still beat its worst finished one."""

    def __init__(self, input_ids, num_beams: int, max_new_tokens: int, pad: int, device=None):
        dev = input_ids.device if device is None else device
        B, L0 = input_ids.shape
        K = num_beams
        self.B, self.K, self.L0, self.Lmax, self.pad = B, K, L0, L0 + max_new_tokens, int(pad)
        self.run = torch.full((B, K, self.Lmax), int(pad), dtype=torch.int64, device=dev)
        self.run[:, :, :L0] = input_ids.to(dev).unsqueeze(1)
        self.pool = self.run.clone()
        self.run_sc = torch.full((B, K), BEAM_NEG, dtype=torch.float32, device=dev)
        self.run_sc[:, 0] = 0.0
        self.pool_sc = torch.full((B, K), BEAM_NEG, dtype=torch.float32, device=dev)
        self.pool_len = torch.zeros(B, K, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(B, K, dtype=torch.int32, device=dev)
        self.open = torch.ones(B, dtype=torch.int32, device=dev)

    def result(self, num_return_sequences: int):
        """(sequences [B * n, L0 + longest returned hypothesis], sequences_scores fp32 [B * n]): the first n pool rows of every item."""
        n = num_return_sequences
        longest = int(self.pool_len[:, :n].max()) if self.pool_len.numel() else 0
        return (self.pool[:, :n, :self.L0 + longest].reshape(self.B * n, -1).contiguous(), self.pool_sc[:, :n].reshape(-1).clone())


def beam_powers(cur: int, L0: int, Lmax: int, length_penalty, early_stopping):
    """The two powers of the length penalty at a step that starts with `cur` valid ids, computed in Python double (the step's kernels and
    the host rule round each to fp32 once and divide by it): the one a hypothesis finished at this step is divided by, and the one the
    best running beam is divided by after the step."""
    hyp = Lmax - L0 if (early_stopping == "never" and length_penalty > 0) else cur + 1 - L0
    return float((cur + 1 - L0) ** length_penalty), float(hyp ** length_penalty)


def _first_k(values, k: int):
    """indices of the k largest entries of a 1-D CPU tensor, descending, the lowest index first among equals (torch.topk leaves that open)."""
    return torch.sort(values, descending=True, stable=True).indices[:k]


def beam_step_reference(st: BeamState, lp, cur: int, eos_ids, length_penalty=1.0, early_stopping=False) -> tuple:
    """One step of the beam-search rule on a BeamState of CPU tensors, in fp32 -- the written form of what ops.beam_step does.
    lp: fp32 [B, K, V], log_softmax of the step's logits per beam row with the n-gram ban's -inf already on it; cur: valid ids per row.
    With n_eos EOS ids, KK = max(2, 1 + n_eos) * K.
      1. acc[k, j] = lp[k, j] + run_sc[k].
      2. The KK largest acc over the flat index k * V + j, ties to the lowest flat index -> (tv, parent, tok), descending; a candidate
         is run[parent] with tok at `cur`.
      3. hit = tok in eos or cur + 1 == Lmax.
      4. rv = tv + (-1e9 where hit); the K largest rv (same tie rule) become run / run_sc.
      5. fv = tv / fp32((cur + 1 - L0) ** length_penalty), plus -1e9 where (early_stopping is True and all of fin) or not open or the
         candidate is not (hit and among the first K); [pool ; candidates], pool first, keep the K largest; a finished candidate's
         length is cur + 1 - L0.
      6. best = run_sc[0] / fp32(hyp ** length_penalty), hyp = Lmax - L0 if early_stopping == "never" and length_penalty > 0 else
         cur + 1 - L0; worst_k = min(pool_sc) if fin[k] else -1e9; open &= any_k(best > worst_k).
      7. The loop goes on while any item is open, not (early_stopping is True and every fin of every item), and not every candidate hit.
    Both divisions are IEEE fp32 divisions on CPU tensors.  -> (parent int32 [B * K] with the batch offset, as HF's beam_idx; goes on)."""
    B, K, L0, Lmax = st.B, st.K, st.L0, st.Lmax
    V = lp.shape[-1]
    f32 = torch.float32
    eos = torch.as_tensor([] if eos_ids is None else [int(e) for e in eos_ids], dtype=torch.int64)
    KK = ops.beam_candidates(K, eos.numel())
    neg = torch.tensor(BEAM_NEG, dtype=f32)
    p_fin, p_hyp = (torch.tensor(p, dtype=f32) for p in beam_powers(cur, L0, Lmax, length_penalty, early_stopping))
    parents = torch.empty(B * K, dtype=torch.int32)
    every_hit = True
    for b in range(B):
        acc = (lp[b].to(f32) + st.run_sc[b].unsqueeze(1)).reshape(-1)
        idx = _first_k(acc, KK)
        tv, parent, tok = acc[idx], idx // V, idx % V
        hit = torch.isin(tok, eos) | (cur + 1 == Lmax)
        cand = st.run[b, parent].clone()
        cand[:, cur] = tok
        every_hit = every_hit and bool(hit.all())
        rv = torch.where(hit, tv + neg, tv)
        sel = _first_k(rv, K)
        fv = tv / p_fin
        first_k = torch.arange(KK) < K
        pen = (early_stopping is True and bool(st.fin[b].all())) or not bool(st.open[b])
        fv = torch.where(~(hit & first_k) | pen, fv + neg, fv)
        e = _first_k(torch.cat([st.pool_sc[b], fv]), K)
        st.pool[b] = torch.cat([st.pool[b], cand])[e]
        st.pool_sc[b] = torch.cat([st.pool_sc[b], fv])[e]
        st.pool_len[b] = torch.cat([st.pool_len[b], torch.full((KK,), cur + 1 - L0, dtype=torch.int32)])[e]
        st.fin[b] = torch.cat([st.fin[b], (hit & first_k).to(torch.int32)])[e]
        st.run[b], st.run_sc[b] = cand[sel], rv[sel]
        parents[b * K:(b + 1) * K] = (b * K + parent[sel]).to(torch.int32)
        best = st.run_sc[b, 0] / p_hyp
        worst = torch.where(st.fin[b].bool(), st.pool_sc[b].min(), neg)
        st.open[b] = int(bool(st.open[b]) and bool((best > worst).any()))
    go = bool(st.open.any()) and not (early_stopping is True and bool(st.fin.all())) and not every_hit
    return parents, go


def beam_search_reference(logits_fn, input_ids, num_beams: int, max_new_tokens: int, eos_ids=None, pad: int = 0, length_penalty=1.0,
                          early_stopping=False, num_return_sequences: int = 1, no_repeat_ngram_size: int = 0, log_probs=None,
                          extra_steps: int = 0, trace=None):
    """generate(num_beams=K)'s rule on the host: HF `GenerationMixin._beam_search` with do_sample=False, restated step by step
    (beam_step_reference) with the one thing HF leaves open fixed -- ties go to the lowest flat index.  The reference of the device loop.
    logits_fn(ids int64 [R, cur]) -> the last-position logits [R, V] of those rows: the first step hands it the B prompts (only beam 0
    of an item exists: the K rows would be equal), every later one the B * K running rows.  log_probs(logits [R, V]) -> fp32 [R, V]:
    the log-softmax (default: torch's on the fp32 logits; the GPU tests hand in ops.token_logprobs' bits).  The n-gram ban puts -inf on the
    log-probabilities, after the softmax (HF's processor order).  extra_steps: steps to run on after the rule has stopped (they must
    change nothing).  trace: a list that receives one dict per step (logits, lp, parent, goes on, the running rows and scores before the step, the rows after).
    -> GenerateOutput(sequences [B * n, <= Lmax], sequences_scores fp32 [B * n], steps = the forwards up to the stop)."""
    if log_probs is None:
        log_probs = lambda x: torch.log_softmax(x.float(), dim=-1)                                      # noqa: E731
    ids = input_ids.cpu()
    B, K = ids.shape[0], num_beams
    st = BeamState(ids, K, max_new_tokens, pad, device="cpu")
    steps, extra = None, 0
    for step in range(max_new_tokens):
        cur = st.L0 + step
        rows = st.run[:, 0, :cur] if step == 0 else st.run[:, :, :cur].reshape(B * K, cur)
        logits = logits_fn(rows.to(input_ids.device))
        lp = log_probs(logits).float().cpu().view(B, -1, logits.shape[-1]).expand(B, K, -1).clone()
        if no_repeat_ngram_size:
            for r, banned in enumerate(no_repeat_ngram_banned_tokens(st.run[:, :, :cur].reshape(B * K, cur).tolist(), no_repeat_ngram_size)):
                lp[r // K, r % K, [t for t in banned if 0 <= t < lp.shape[-1]]] = float("-inf")
        before = (st.run.clone(), st.run_sc.clone()) if trace is not None else None
        parent, go = beam_step_reference(st, lp, cur, eos_ids, length_penalty, early_stopping)
        if trace is not None:
            trace.append(dict(cur=cur, logits=logits, lp=lp, parent=parent, go=go, run_before=before[0], run_sc_before=before[1], run_after=st.run.clone(),
                              stopped=steps is not None))
        if steps is not None:
            extra += 1
        elif not go:
            steps = step + 1
        if steps is not None and extra >= extra_steps:
            break
    seqs, scores = st.result(num_return_sequences)
    return GenerateOutput(sequences=seqs, sequences_scores=scores, steps=max_new_tokens if steps is None else steps)


def beam_loop(d: Decoding, seq, num_beams: int, ngram: int = 0, length_penalty=1.0, early_stopping=False, num_return_sequences: int = 1):
    """generate(num_beams=K): deterministic beam search (`beam_search_reference` is the rule) with the state on the device, after the
    pattern of fused_loop.  The prefill runs once per item (B rows, vision tower included); its cache is replicated to B * K rows and every
    later forward takes the B * K running rows.  A step is the forward, ops.ngram_ban if asked (a copy of the rows with -inf at the banned
    tokens; the normalizer keeps reading the raw rows), ops.beam_step (two launches: the new state, `parent`, and the step's "the loop goes
    on" word) and, with a cache, KVCache.gather_rows by `parent` over the generated positions only (the beams of an item share the prompt's
    K / V).  The host reads the go-on words every 8 steps; steps past the stop change neither the pool nor its scores, so nothing is trimmed.
    Without a cache every step re-runs the rows and nothing is gathered.  -> (ids [B * n, <= Lmax], sequences_scores fp32 [B * n])"""
    B, L0 = seq.shape
    K, n_max, dev = num_beams, d.max_new_tokens, seq.device
    st = BeamState(seq, K, n_max, 0 if d.pad is None else d.pad)
    run = [st.run, torch.empty_like(st.run)]
    pool = [st.pool, torch.empty_like(st.pool)]
    cand_v = torch.empty(B * K * ops.BEAM_MAX_CAND, dtype=torch.float32, device=dev)
    cand_t = torch.empty(B * K * ops.BEAM_MAX_CAND, dtype=torch.int32, device=dev)
    parent = torch.empty(B * K, dtype=torch.int32, device=dev)
    go = torch.zeros(max(n_max, 1), dtype=torch.int32, device=dev)
    banned = None
    n_done = 0
    for step in range(n_max):
        cur, a, b_ = L0 + step, step & 1, (step + 1) & 1
        if step == 0:
            last = d.forward(seq, 0).logits[:, -1]                                   # [B, V]: the prefill
            rows = run[a][:, 0]                                                      # beam 0 of every item (a view: rows K * Lmax apart)
            # from here on the rows are the beams: cache, mask and vision inputs K times, item by item
            if d.cache is not None:
                d.cache = d.cache.replicated(K)
            if d.attention_mask is not None:
                d.attention_mask = d.attention_mask.repeat_interleave(K, 0)
            if d.cache is None:
                d.images, d.videos = (None if t is None else t.repeat_interleave(K, 0) if torch.is_tensor(t) else [x for x in t for _ in range(K)]
                                      for t in (d.images, d.videos))
        else:
            rows = run[a].view(B * K, -1)
            last = d.forward(rows[:, :cur], step).logits[:, -1]                      # [B * K, V]
        pick = None
        if ngram > 0:
            if banned is None or banned.shape != last.shape:
                banned = torch.empty(last.shape, dtype=last.dtype, device=dev)
            pick = ops.ngram_ban(last, rows, cur, ngram, out=banned)
        p_fin, p_hyp = beam_powers(cur, L0, st.Lmax, length_penalty, early_stopping)
        ops.beam_step(last.view(B, -1, last.shape[-1]) if step else last.unsqueeze(1), pick, run[a], run[b_], pool[a], pool[b_], st.run_sc, st.pool_sc,
                      st.pool_len, st.fin, st.open, d.eos_ids, st.pad, L0, cur, p_fin, p_hyp, early_stopping, cand_v, cand_t, parent, go[step:step + 1])
        if d.cache is not None and step > 0 and step + 1 < n_max:
            d.cache.gather_rows(parent, L0, cur)                                     # (step 0: every row continues beam 0's prefill)
        n_done = step + 1
        if n_done % 8 == 0 or n_done == n_max:
            if bool((go[:n_done] == 0).any()):                                       # the only device -> host read: every 8 steps
                break
    st.run, st.pool = run[n_done & 1], pool[n_done & 1]                              # (step s wrote the buffers (s + 1) & 1)
    return st.result(num_return_sequences)
