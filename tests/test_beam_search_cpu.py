"""Beam search (generate(num_beams=K), generation.beam_search_reference / beam_loop, ops.beam_step, ops.kv_gather_rows): what can be checked
without a GPU -- the host rule against transformers' own beam search, that running it past its stop changes nothing, every refusal that
comes before any device work, and the C ABI."""
import ctypes
import inspect
import itertools
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW, L0, PAD = 12, 5, 15
# (K, length_penalty, early_stopping) x (EOS ids, use_cache); num_return_sequences alternates between 1 and K
GRID = [(K, lp, es, eos, uc, K if i & 1 else 1)
        for i, (K, lp, es) in enumerate(itertools.product((2, 3, 4), (0.0, 1.0, 2.0), (False, True, "never")))
        for eos, uc in (([1], True), ([1, 2], False))]


@pytest.fixture(scope="module")
def hf():
    """A tiny random LlamaForCausalLM (V = 16; lm_head scaled so that the distributions are peaked and EOS ends some beams early), two
    prompts, and the rule's result and trace for every case of GRID, computed once."""
    from transformers import LlamaConfig, LlamaForCausalLM
    gen = pkg("generation")
    with torch.no_grad():
        torch.manual_seed(2)
        model = LlamaForCausalLM(LlamaConfig(vocab_size=16, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                             max_position_embeddings=64)).eval()
        model.lm_head.weight.mul_(8.0)
        torch.manual_seed(102)
        ids = torch.randint(3, 16, (2, L0))
        fwd = lambda x: model(x).logits[:, -1]                                                          # noqa: E731
        ours = []
        for K, lp, es, eos, uc, nret in GRID:
            trace = []
            ours.append((gen.beam_search_reference(fwd, ids, K, NEW, eos, PAD, lp, es, nret, trace=trace), trace))
    return model, ids, fwd, ours


def test_rule_equals_transformers_beam_search(hf):
    """ids equal, scores within 1e-5, on all 54 cases; a non-zero pad (HF turns pad id 0 into EOS) and an all-ones mask (HF would infer one
    from pad ids in the prompt).  At least 5 cases end before Lmax."""
    model, ids, _, ours = hf
    early = 0
    with torch.no_grad():
        for (K, lp, es, eos, uc, nret), (r, _) in zip(GRID, ours):
            ref = model.generate(ids, attention_mask=torch.ones_like(ids), num_beams=K, do_sample=False, max_new_tokens=NEW, length_penalty=lp,
                                 early_stopping=es, eos_token_id=eos, pad_token_id=PAD, num_return_sequences=nret, return_dict_in_generate=True,
                                 output_scores=True, use_cache=uc)
            case = (K, lp, es, eos, uc, nret)
            assert tuple(r.sequences.shape) == tuple(ref.sequences.shape) and torch.equal(r.sequences, ref.sequences), case
            assert r.sequences_scores.dtype == torch.float32 and tuple(r.sequences_scores.shape) == (2 * nret,)
            assert float((r.sequences_scores - ref.sequences_scores).abs().max()) <= 1e-5, case
            early += r.steps < NEW
    assert early >= 5, early


def test_no_case_depends_on_the_tie_order(hf):
    """torch.topk leaves the order of equal scores open and the rule fixes it: the comparison above must not lean on either.  No step of
    any case has two equal values among its KK + 1 largest accumulated scores."""
    for (K, lp, es, eos, uc, nret), (_, trace) in zip(GRID, hf[3]):
        KK = max(2, 1 + len(eos)) * K
        for t in trace:
            acc = (t["lp"] + t["run_sc_before"].unsqueeze(-1)).flatten(1)
            top = acc.sort(dim=1, descending=True).values[:, :KK + 1]
            assert not bool((top[:, 1:] == top[:, :-1]).any()), (K, lp, es, eos, t["cur"])


def test_steps_past_the_stop_change_nothing(hf):
    """the device loop looks at the host every 8 steps: up to 7 steps run after the rule has stopped."""
    gen = pkg("generation")
    _, ids, fwd, ours = hf
    ran_past = 0
    with torch.no_grad():
        for (K, lp, es, eos, uc, nret), (r, _) in list(zip(GRID, ours))[::3]:
            trace = []
            more = gen.beam_search_reference(fwd, ids, K, NEW, eos, PAD, lp, es, nret, extra_steps=7, trace=trace)
            ran_past += len(trace) > r.steps
            assert more.steps == r.steps and torch.equal(more.sequences, r.sequences)
            assert torch.equal(more.sequences_scores.view(torch.int32), r.sequences_scores.view(torch.int32))
    assert ran_past >= 2, ran_past


def test_ties_go_to_the_lowest_flat_index():
    """two beams with equal scores and equal rows: the candidates come beam 0 first, and inside a beam the lowest token first."""
    gen = pkg("generation")
    st = gen.BeamState(torch.tensor([[3, 4]]), 2, 2, PAD)
    st.run_sc[:] = -1.0
    lp = torch.log_softmax(torch.tensor([0.0, 2.0, 2.0, 1.0, 0.0]), -1).expand(1, 2, 5).clone()
    parent, go = gen.beam_step_reference(st, lp, 2, None)
    assert parent.tolist() == [0, 0] and st.run[0, :, 2].tolist() == [1, 2] and go


def test_generate_signature_and_defaults():
    core = pkg("modeling_core")
    sig = inspect.signature(core.UllavaCoreForCausalLM.generate).parameters
    assert (sig["num_beams"].default, sig["length_penalty"].default, sig["early_stopping"].default, sig["num_return_sequences"].default) == (1, 1.0, False, 1)


IDS = torch.tensor([[1, 5, 6, 7, 5, 6]])


class _OnGpu:
    """stands in for a GPU tensor where only the placement is asked for"""
    is_cuda = True
    shape = (1, 6)

    def dim(self):
        return 2


@pytest.mark.parametrize("kw, match", [
    (dict(do_sample=True, temperature=0.7), "do_sample=False"),
    (dict(sampler="device"), "sampler"),
    (dict(prompt_lookup_num_tokens=4, use_cache=True), "prompt_lookup_num_tokens"),
    (dict(stopping_criteria=[lambda ids, scores: False]), "eos_token_id"),
    (dict(output_logprobs=True, return_dict_in_generate=True), "sequences_scores"),
    (dict(kv_cache_dtype="fp8_e4m3", use_cache=True, dtype=torch.bfloat16), "kv_cache_dtype"),
    (dict(no_repeat_ngram_size=2), 'ngram_ban="device"'),
    (dict(no_repeat_ngram_size=2, ngram_ban="host"), 'ngram_ban="device"'),
    (dict(num_return_sequences=5), "num_return_sequences"),
    (dict(vocab_size=1), "vocab_size"),
    (dict(n_eos=16), "EOS ids"),
])
def test_beam_refusals_name_the_way_out(kw, match):
    gen = pkg("generation")
    with pytest.raises(ValueError, match=match):
        gen.check_generate_args(_OnGpu(), num_beams=4, **kw)


def test_beam_refusals_other():
    gen = pkg("generation")
    for bad in (0, 17, -1, 2.0, True, "4"):
        with pytest.raises(ValueError, match="num_beams"):
            gen.check_generate_args(IDS, num_beams=bad)
    with pytest.raises(ValueError, match="early_stopping"):
        gen.check_generate_args(_OnGpu(), num_beams=2, early_stopping="always")
    # hidden states: what evaluate() needs, so evaluate(num_beams > 1) keeps raising
    with pytest.raises(NotImplementedError, match="hidden states"):
        gen.check_generate_args(_OnGpu(), num_beams=2, output_hidden_states=True)
    # no CPU path
    with pytest.raises(NotImplementedError, match="GPU"):
        gen.check_generate_args(IDS, num_beams=4)
    with pytest.raises(NotImplementedError, match="GPU"):
        _tiny_core().generate(input_ids=IDS, num_beams=2, max_new_tokens=2)
    # the beam options without beams
    for kw in (dict(length_penalty=2.0), dict(early_stopping=True), dict(early_stopping="never"), dict(num_return_sequences=2)):
        with pytest.raises(ValueError, match="num_beams"):
            gen.check_generate_args(IDS, **kw)
        with pytest.raises(ValueError, match="num_beams"):
            _tiny_core().generate(input_ids=IDS, max_new_tokens=2, **kw)
    # what passes: every supported combination reaches the end of the checks
    assert gen.check_generate_args(_OnGpu(), num_beams=4, length_penalty=0.5, early_stopping="never", num_return_sequences=4, no_repeat_ngram_size=2,
                                   ngram_ban="device", use_cache=True, return_dict_in_generate=True, vocab_size=32064, n_eos=2)[0] == 2
    assert gen.check_generate_args(IDS, num_beams=1, length_penalty=1, early_stopping=False, num_return_sequences=1)[0] == 0


def test_entries_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib = pkg("_lib")
    so = ctypes.CDLL(lib.LIB_PATH)
    for name, n_args in (("ull_beam_step", 32), ("ull_kv_gather_rows", 18)):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, f"{name} not declared in include/ullava_hip.h"
        assert name in lib.SIGNATURES and hasattr(so, name)
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name]) == n_args and lib.RESTYPES[name] is ctypes.c_int
        assert not any(n.startswith(name + "_") for n in lib.SIGNATURES)         # compiled once: no per-dtype twins
    ops = pkg("ops")
    assert (ops.BEAM_MAX_K, ops.BEAM_MAX_CAND) == (16, 64)


def test_entries_refuse_bad_arguments_before_any_launch():
    """the pointers are never dereferenced on these paths (no device exists here)."""
    lib = pkg("_lib")
    ARG, SHAPE = lib.DEFINES["ULL_ERR_ARG"], lib.DEFINES["ULL_ERR_SHAPE"]
    p, q = 4096, 8192                                              # any non-null addresses
    good = dict(logits=p, dt=1, row_stride=32, pick=None, pick_stride=0, B=1, Kin=4, K=4, V=32, run_in=p, run_out=q, pool_in=p, pool_out=q, run_sc=p,
                pool_sc=p, pool_len=p, fin=p, open=p, eos=p, n_eos=1, pad=0, Lmax=10, L0=4, cur=5, pow_fin=1.0, pow_hyp=1.0, es=0, cand_v=p, cand_t=p,
                parent=p, go=p, stream=None)
    step = getattr(lib.load(), "ull_beam_step")
    for kw, rc in ((dict(K=17, Kin=17), ARG), (dict(Kin=2), ARG), (dict(cur=10), ARG), (dict(cur=3), ARG), (dict(run_out=p), ARG), (dict(go=None), ARG),
                   (dict(es=3), ARG), (dict(dt=3), ARG), (dict(eos=None), ARG), (dict(V=1), SHAPE), (dict(n_eos=16), SHAPE)):
        assert step(*dict(good, **kw).values()) == rc, kw
    arr = (ctypes.c_void_p * 1)(p)
    good = dict(sk=arr, sv=arr, dk=arr, dv=arr, n_layers=1, src_rows=2, dst_rows=2, H=2, hd=8, esz=2, src_smax=128, dst_smax=64, src_p0=33, dst_p0=1, n=4,
                row_map=None, skip=None, stream=None)
    rows = getattr(lib.load(), "ull_kv_gather_rows")
    for kw, rc in ((dict(esz=3), ARG), (dict(n=-1), ARG), (dict(sk=None), ARG), (dict(dst_p0=2), SHAPE), (dict(n=100), SHAPE), (dict(n=64), SHAPE),
                   (dict(src_smax=100), SHAPE), (dict(hd=4), SHAPE), (dict(dst_rows=40000), SHAPE), (dict(n=0), 0), (dict(n_layers=0), 0)):
        assert rows(*dict(good, **kw).values()) == rc, kw
