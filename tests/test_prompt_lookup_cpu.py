"""No GPU: the `prompt_lookup_num_tokens` / `max_matching_ngram_size` arguments of generate() / evaluate() (every refusal comes before any
device work), the C entry point of the speculative step, KVCache.truncate's bookkeeping, and the host restatement of the lookup
(`prompt_lookup_candidates`) against transformers' PromptLookupCandidateGenerator."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hf_candidates(row, num_tokens, max_ngram, eos_ids, limit):
    """The same draft from transformers' own generator.  HF caps the continuation's END INDEX by its `max_length`; the contract here is a
    cap on the draft's length, so the cap goes in through num_output_tokens and max_length is out of the way."""
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    want = min(num_tokens, limit)
    if want <= 0:
        return []
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos_ids) if eos_ids else None, num_output_tokens=want,
                                         max_matching_ngram_size=max_ngram, max_length=10 ** 9)
    ids = torch.tensor([row])
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(row):].tolist()


def test_lookup_equals_transformers_on_random_rows():
    MC = pkg("modeling_core")
    g = torch.Generator().manual_seed(5)
    n_nonempty = 0
    for i in range(400):
        L = int(torch.randint(1, 40, (1,), generator=g))
        vocab = (3, 5, 9)[i % 3]                                 # small: matches are common
        row = torch.randint(0, vocab, (L,), generator=g).tolist()
        k = int(torch.randint(1, 16, (1,), generator=g))
        ng = int(torch.randint(1, 5, (1,), generator=g))
        eos = ([], [0], [1, 2])[i % 3]
        limit = int(torch.randint(0, 20, (1,), generator=g))
        got = MC.prompt_lookup_candidates(row, k, ng, eos, limit)
        assert got == hf_candidates(row, k, ng, eos, limit), (row, k, ng, eos, limit)
        assert len(got) <= min(k, limit)
        n_nonempty += bool(got)
    assert n_nonempty >= 100


CRAFTED = [
    # (what, row, num_tokens, max_ngram, eos, limit, expected)
    ("several matches, the earliest wins", [7, 8, 1, 7, 8, 2, 7, 8, 3, 7, 8], 1, 2, [], 9, [1]),
    ("a longer n-gram matching later beats a shorter one matching earlier", [8, 5, 6, 7, 8, 9, 4, 7, 8], 1, 2, [], 9, [9]),
    ("only the trailing n-gram itself matches at n = 2: falls through to n = 1", [3, 9, 4, 5, 9], 2, 2, [], 9, [4, 5]),
    ("continuation cut by the row's end", [1, 2, 3, 1, 2], 10, 2, [], 99, [3, 1, 2]),
    ("an EOS id inside the continuation", [1, 2, 3, 0, 4, 1, 2], 5, 2, [0], 99, [3]),
    ("an EOS id first in the continuation: an empty draft, no fall-through", [2, 1, 2, 0, 4, 1, 2], 5, 2, [0], 99, []),
    ("a row shorter than the n-gram size", [4, 4], 3, 5, [], 9, [4]),
    ("a row of one id", [4], 3, 2, [], 9, []),
    ("no match at all", [1, 2, 3, 4, 5], 3, 2, [], 9, []),
    ("the limit cuts the draft", [1, 2, 3, 4, 5, 1, 2], 5, 2, [], 2, [3, 4]),
    ("limit 0: nothing may be proposed", [1, 2, 3, 1, 2], 5, 2, [], 0, []),
]


@pytest.mark.parametrize("case", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_lookup_on_crafted_rows(case):
    _, row, k, ng, eos, limit, want = case
    assert pkg("modeling_core").prompt_lookup_candidates(row, k, ng, eos, limit) == want
    assert hf_candidates(row, k, ng, eos, limit) == want


def test_spec_step_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib, ops = pkg("_lib"), pkg("ops")
    so = ctypes.CDLL(lib.LIB_PATH)
    assert re.search(r"\bint ull_spec_step\(", header), "ull_spec_step not declared in include/ullava_hip.h"
    assert "ull_spec_step" in lib.SIGNATURES and hasattr(so, "ull_spec_step")
    n_args = len(re.search(r"\bint ull_spec_step\(([^;]*)\);", header).group(1).split(","))
    assert n_args == len(lib.SIGNATURES["ull_spec_step"])
    m = re.search(r"#define ULL_SPEC_MAX_DRAFT (\d+)", header)
    assert m and int(m.group(1)) == ops.SPEC_MAX_DRAFT == 15
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.spec_step(torch.zeros(1, 8), None, 1.0, 0, None, torch.zeros(1, 8, dtype=torch.int64), 1, 0, 4, None, 4, 2,
                      torch.zeros(16, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


def test_generate_takes_the_two_arguments_by_name():
    for cls, fn in ((pkg("modeling_core").UllavaCoreForCausalLM, "generate"), (pkg("modeling_ullava").UllavaForCausalLM, "evaluate")):
        p = inspect.signature(getattr(cls, fn)).parameters
        for name in ("prompt_lookup_num_tokens", "max_matching_ngram_size"):
            assert p[name].default is None and p[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, (fn, name)
    with pytest.raises(TypeError, match="unsupported keyword"):   # **kwargs keeps raising on unknown options
        _tiny_core().generate(input_ids=torch.tensor([[1, 2, 3]]), max_new_tokens=2, prompt_lookup_tokens=3)


REFUSALS = [
    ("a batch of more than one row", dict(input_ids=torch.tensor([[1, 2, 3], [4, 5, 6]])), "one row"),
    ("use_cache false", dict(use_cache=False), "use_cache"),
    ("no_repeat_ngram_size", dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"),
    ("a padded attention mask", dict(attention_mask=torch.tensor([[0, 1, 1]])), "padded"),
    ("sampling on the host sampler", dict(do_sample=True, temperature=0.2), 'sampler="device"'),
    ("sampling with sampler='host'", dict(do_sample=True, temperature=1.0, sampler="host"), 'sampler="device"'),
    ("k = 0", dict(prompt_lookup_num_tokens=0), "1..15"),
    ("k = 16", dict(prompt_lookup_num_tokens=16), "1..15"),
    ("k = 2.5", dict(prompt_lookup_num_tokens=2.5), "1..15"),
    ("n-gram size 0", dict(max_matching_ngram_size=0), ">= 1"),
    ("the n-gram size alone", dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=2), "needs `prompt_lookup_num_tokens`"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_generate_refusals_come_before_any_device_work(case):
    _, extra, match = case
    kw = dict(input_ids=torch.tensor([[1, 2, 3]]), max_new_tokens=4, use_cache=True, prompt_lookup_num_tokens=4)
    kw.update(extra)
    with pytest.raises(ValueError, match=match):
        _tiny_core().generate(**kw)                              # CPU tensors: any device work would raise something else


def test_generate_accepts_the_settings_then_asks_for_the_gpu():
    """do_sample with temperature 0 is greedy, an all-ones mask is no padding, sampler="device" may sample: these pass every check and
    stop at the first device work (no CPU path, no fall-back to the plain loop)."""
    ids = torch.tensor([[1, 2, 3]])
    for extra in (dict(), dict(do_sample=True, temperature=0.0), dict(attention_mask=torch.ones(1, 3, dtype=torch.long)),
                  dict(do_sample=True, temperature=0.2, sampler="device"), dict(max_matching_ngram_size=3, kv_cache_dtype="fp8_e4m3")):
        with pytest.raises(RuntimeError, match="GPU tensors"):
            _tiny_core().generate(input_ids=ids, max_new_tokens=4, use_cache=True, prompt_lookup_num_tokens=4, **extra)


def test_evaluate_refusals_come_before_the_model_is_touched():
    MU = pkg("modeling_ullava")
    self = object.__new__(MU.UllavaForCausalLM)
    ev = MU.UllavaForCausalLM.evaluate
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="1..15"):
        ev(self, None, None, ids, None, None, prompt_lookup_num_tokens=16, sampler="device")
    with pytest.raises(ValueError, match="needs `prompt_lookup_num_tokens`"):
        ev(self, None, None, ids, None, None, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match='sampler="device"'):
        ev(self, None, None, ids, None, None, prompt_lookup_num_tokens=4)            # evaluate's default temperature is 0.2
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        ev(self, None, None, ids, None, None, prompt_lookup_num_tokens=4, temperature=0.0, no_repeat_ngram_size=3)
    with pytest.raises(ValueError, match="one row"):
        ev(self, None, None, torch.tensor([[1, 2], [3, 4]]), None, None, prompt_lookup_num_tokens=4, temperature=0.0)


def test_truncate_keeps_exactly_n_positions_of_hidden_states():
    MC = pkg("modeling_core")
    c = object.__new__(MC.KVCache)                               # bookkeeping only: no device buffers
    h = [torch.arange(5.0).view(1, 5, 1), torch.arange(5.0, 9.0).view(1, 4, 1), torch.arange(9.0, 10.0).view(1, 1, 1)]
    for n in (10, 9, 8, 6, 5, 3, 0):
        c.length, c.last_hidden = 10, list(h)
        c.truncate(n)
        assert c.length == n
        got = torch.cat(c.last_hidden, dim=1) if c.last_hidden else torch.empty(1, 0, 1)
        assert torch.equal(got, torch.arange(float(n)).view(1, n, 1)), n
    c.length, c.last_hidden = 10, list(h)
    for bad in (11, -1):
        with pytest.raises(ValueError, match="truncate"):
            c.truncate(bad)
    c.length, c.last_hidden = 7, []                              # a cache made from an HF past: no hidden states to trim
    c.truncate(4)
    assert c.length == 4 and c.last_hidden == []
