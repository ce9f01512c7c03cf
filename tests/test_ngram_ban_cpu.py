"""The on-device n-gram ban (generate(ngram_ban="device"), evaluate(ngram_ban="device"), ops.ngram_ban, ull_ngram_ban): what can be checked
without a GPU -- the C ABI, the signatures and the refusals that come before any device work."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = torch.tensor([[1, 5, 6, 7, 5, 6]])


def test_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib = pkg("_lib")
    so = ctypes.CDLL(lib.LIB_PATH)
    m = re.search(r"\bint ull_ngram_ban\(([^;]*)\);", header)
    assert m, "ull_ngram_ban not declared in include/ullava_hip.h"
    assert "ull_ngram_ban" in lib.SIGNATURES and hasattr(so, "ull_ngram_ban")
    assert len(m.group(1).split(",")) == len(lib.SIGNATURES["ull_ngram_ban"]) == 12 and lib.RESTYPES["ull_ngram_ban"] is ctypes.c_int
    # compiled once, with a run-time dtype code: no per-dtype twins
    assert not any(n.startswith("ull_ngram_ban_") for n in lib.SIGNATURES)


def test_entry_refuses_bad_arguments_before_any_launch():
    """ngram < 1, cur_len < 0, V < 1, a null pointer: ULL_ERR_ARG; rows of `out` that would overlap: ULL_ERR_SHAPE; R == 0: ULL_OK.  The
    pointers are never dereferenced on these paths (no device exists here)."""
    lib = pkg("_lib")
    fn = getattr(lib.load(), "ull_ngram_ban")
    ARG, SHAPE = lib.DEFINES["ULL_ERR_ARG"], lib.DEFINES["ULL_ERR_SHAPE"]
    p = 4096                                                       # any non-null address
    good = dict(logits=p, dt=1, row_stride=8, R=1, V=8, ids=p, ids_ld=4, cur_len=4, ngram=2, out=p, out_ld=8)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["logits"], a["dt"], a["row_stride"], a["R"], a["V"], a["ids"], a["ids_ld"], a["cur_len"], a["ngram"], a["out"], a["out_ld"], None)

    for bad in (dict(ngram=0), dict(ngram=-1), dict(cur_len=-1), dict(V=0), dict(logits=None), dict(ids=None), dict(out=None), dict(dt=3),
                dict(R=-1), dict(row_stride=-8), dict(ids_ld=-1)):
        assert call(**bad) == ARG, bad
    assert call(out_ld=7) == SHAPE
    assert call(R=0) == 0


def test_ngram_ban_defaults_to_none_and_keeps_the_pinned_positions():
    MC, MU = pkg("modeling_core"), pkg("modeling_ullava")
    gen = inspect.signature(MC.UllavaCoreForCausalLM.generate).parameters
    ev = inspect.signature(MU.UllavaForCausalLM.evaluate).parameters
    for p in (gen, ev):
        assert p["ngram_ban"].default is None and p["ngram_ban"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert list(ev)[-1] == "sampler" and list(ev).index("ngram_ban") < list(ev).index("sampler")
    assert inspect.signature(pkg("generation").check_generate_args).parameters["ngram_ban"].default is None


def test_ops_ngram_ban_refuses_cpu_tensors_and_bad_sizes():
    ops = pkg("ops")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.ngram_ban(torch.zeros(2, 8), torch.zeros(2, 4, dtype=torch.int64), 4, 2)


REFUSALS = [
    ("device ban without a size", dict(ngram_ban="device"), ValueError, "no_repeat_ngram_size"),
    ("device ban with size 0", dict(ngram_ban="device", no_repeat_ngram_size=0), ValueError, "no_repeat_ngram_size"),
    ("an unknown value", dict(ngram_ban="gpu", no_repeat_ngram_size=2), ValueError, "unknown ngram_ban"),
    ("CPU ids", dict(ngram_ban="device", no_repeat_ngram_size=2), RuntimeError, "needs GPU tensors"),
    ("CPU ids, device sampler", dict(ngram_ban="device", no_repeat_ngram_size=2, sampler="device", do_sample=True, temperature=0.7), RuntimeError,
     "needs GPU tensors"),
    ("prompt lookup with the device ban", dict(ngram_ban="device", no_repeat_ngram_size=3, prompt_lookup_num_tokens=4, use_cache=True), ValueError,
     "no_repeat_ngram_size"),
    ("prompt lookup with the host ban", dict(ngram_ban="host", no_repeat_ngram_size=3, prompt_lookup_num_tokens=4, use_cache=True), ValueError,
     "no_repeat_ngram_size"),
    ("device sampler, default ban", dict(sampler="device", no_repeat_ngram_size=3), ValueError, "no_repeat_ngram_size"),
    ("device sampler, host ban", dict(sampler="device", no_repeat_ngram_size=3, ngram_ban="host", do_sample=True, temperature=0.7), ValueError,
     "no_repeat_ngram_size"),
]


@pytest.mark.parametrize("what,kw,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_generate_refuses_before_any_device_work(what, kw, exc, match):
    """A CPU model and CPU ids: anything that got past the checks would fail with another error (no CPU path exists)."""
    with pytest.raises(exc, match=match):
        _tiny_core().generate(input_ids=IDS, max_new_tokens=2, **kw)


@pytest.mark.parametrize("what,kw,exc,match", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_generate_args_is_where_the_refusals_live(what, kw, exc, match):
    """evaluate() calls check_generate_args before it starts the SAM encoder: every refusal above comes from there."""
    G = pkg("generation")
    with pytest.raises(exc, match=match):
        G.check_generate_args(IDS, return_dict_in_generate=True, config_use_cache=False, **kw)


def test_evaluate_forwards_ngram_ban_to_the_checks():
    src = inspect.getsource(pkg("modeling_ullava").UllavaForCausalLM.evaluate)
    assert "ngram_ban=ngram_ban" in src and src.index("check_generate_args(") < src.index("_visual_embs_tm(")


def test_prompt_lookup_refusal_says_why():
    with pytest.raises(ValueError, match="draft"):
        _tiny_core().generate(input_ids=IDS, max_new_tokens=2, no_repeat_ngram_size=3, ngram_ban="device", prompt_lookup_num_tokens=4, use_cache=True)
