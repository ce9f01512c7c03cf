"""Per-token log-probabilities (generate(output_logprobs=True), evaluate(output_logprobs=True), score(), ops.token_logprobs,
ull_token_logprobs): what can be checked without a GPU -- signatures, the refusals that come before any device work, the C ABI."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_PARAMS = ["self", "input_ids", "attention_mask", "images", "videos", "labels"]


def test_generate_and_evaluate_take_output_logprobs():
    """The core model generates, the full model evaluates (through the core's generate).  generate: output_logprobs=False is the last named
    parameter.  evaluate: tests/test_device_sampler_cpu.py pins `sampler` as its last parameter, so the flag stands right before it, behind
    every parameter that is older than `sampler`; it is meant to be passed by keyword."""
    MC, MU = pkg("modeling_core"), pkg("modeling_ullava")
    gen = [p for p in inspect.signature(MC.UllavaCoreForCausalLM.generate).parameters.values() if p.kind is not inspect.Parameter.VAR_KEYWORD]
    assert [p.name for p in gen][-3:] == ["prompt_lookup_num_tokens", "max_matching_ngram_size", "output_logprobs"]
    assert gen[-1].default is False
    ev = inspect.signature(MU.UllavaForCausalLM.evaluate).parameters
    assert list(ev)[-4:] == ["prompt_lookup_num_tokens", "max_matching_ngram_size", "output_logprobs", "sampler"]
    assert ev["output_logprobs"].default is False and ev["sampler"].default is None
    assert list(ev)[:7] == ["self", "images_sam", "images", "input_ids", "raw_size_list", "resize_list", "max_new_tokens"]


def test_score_exists_on_both_classes_with_one_signature():
    MC, MU = pkg("modeling_core"), pkg("modeling_ullava")
    for cls in (MC.UllavaCoreForCausalLM, MU.UllavaForCausalLM):
        ps = inspect.signature(cls.score).parameters
        assert list(ps) == SCORE_PARAMS, cls
        assert all(ps[n].default is None for n in SCORE_PARAMS[2:]) and ps["input_ids"].default is inspect.Parameter.empty


def test_generate_validates_before_any_device_work():
    m = _tiny_core()
    ids = torch.tensor([[1, 5, 6, 7]])
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        m.generate(input_ids=ids, max_new_tokens=2, output_logprobs=True)
    with pytest.raises(TypeError, match="repetition_penalty"):
        m.generate(input_ids=ids, max_new_tokens=2, repetition_penalty=1.2)
    with pytest.raises(TypeError, match="output_scores"):          # HF's spelling stays refused: this project's is output_logprobs
        m.generate(input_ids=ids, max_new_tokens=2, output_scores=True, return_dict_in_generate=True)


def test_token_logprobs_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib = pkg("_lib")
    so = ctypes.CDLL(lib.LIB_PATH)
    assert re.search(r"\bint ull_token_logprobs\(", header), "ull_token_logprobs not declared in include/ullava_hip.h"
    assert "ull_token_logprobs" in lib.SIGNATURES and hasattr(so, "ull_token_logprobs")
    assert len(lib.SIGNATURES["ull_token_logprobs"]) == 11 and lib.RESTYPES["ull_token_logprobs"] is ctypes.c_int
    # compiled once, with a run-time dtype code: no per-dtype twins
    assert not any(n.startswith("ull_token_logprobs_") for n in lib.SIGNATURES)


def test_token_logprobs_refuses_cpu_tensors():
    ops = pkg("ops")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.token_logprobs(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64))
