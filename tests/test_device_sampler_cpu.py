"""No GPU: the `sampler=` keyword of generate() / evaluate() (its refusals come before any device work), the C entry point of the on-device
sampler, and the robustness gate the GPU tests use (`robust_rows`), checked here against the host path on the CPU.

The gate.  The device sampler and the host path (`sampling_probs` + `torch.multinomial`) compute the same thing in different fp32 orders, so
they may differ on a row where rounding decides: a token whose cumulative mass sits on the nucleus boundary 1 - top_p, or two race values
exp(s - max) / noise that are almost equal.  `robust_rows` restates a row in fp64 and calls it robust when
  * the fp64 winner is the same with every UNCERTAIN token kept and with every uncertain token removed.  Uncertain: cumulative mass within
    n_kept * 2^-22 of 1 - top_p (n_kept fp32 additions of values <= 1, each off by at most 2^-24 of the running sum, with a factor 4 for the
    softmax denominators), plus every token tied in score with one of those or with a tie group that straddles the boundary (the order
    among equal scores is free);
  * the best race value exceeds the second best by a factor above 1 + 2^-18 (a few ulps of exp's argument at |s - max| <= 64 move
    exp(s - max) by up to 64 * 2^-24 = 2^-18).
Tokens are compared on robust rows only, and at most 5 % of the rows of a setting may be non-robust."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import pkg
from test_fp8_weights_cpu import _tiny_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(0.2, 50, None), (0.2, 50, 0.7), (1.0, 50, 0.9), (1.0, 0, 0.9), (0.7, 0, None), (1.0, 1000, 0.95)]
MAX_NON_ROBUST = 0.05


def robust_rows(logits, q, T, k, p):
    """logits fp32 [R, V] (CPU), q fp32 [R, V] the exponential noise of the draw -> (robust bool [R], the fp64 restatement's tokens [R])."""
    logits, q = logits.float().cpu(), q.float().cpu()
    R, V = logits.shape
    s32 = logits / T if T != 1.0 else logits                    # the scores are fp32 on both paths; everything after them is fp64 here
    keep = torch.ones_like(s32, dtype=torch.bool)
    topk_keep = keep.clone()
    if k and k > 0:
        thr = torch.topk(s32, min(k, V))[0][:, -1:]
        topk_keep = s32 >= thr
        keep = topk_keep.clone()
    nk = keep.sum(-1)
    robust = torch.ones(R, dtype=torch.bool)
    if p is not None and p < 1.0:
        sm = s32.double().masked_fill(~keep, float("-inf"))
        so, si = torch.sort(sm, descending=False)
        cum = so.softmax(-1).cumsum(-1)
        rem = cum <= (1 - p)
        rem[:, -1] = False
        keep = keep & ~rem.scatter(1, si, rem)
        eps = nk.double()[:, None] * 2.0 ** -22
        unc_sorted = ((cum - (1 - p)).abs() <= eps) & (so > float("-inf"))
        first_kept = (cum > (1 - p)).int().argmax(-1, keepdim=True)
        last_rem = (first_kept - 1).clamp(min=0)
        edge = torch.zeros_like(unc_sorted)
        edge.scatter_(1, first_kept, True)
        edge.scatter_(1, last_rem, True)
        straddle = (so.gather(1, first_kept) == so.gather(1, last_rem)) & (first_kept > 0)
        unc_sorted = unc_sorted | (edge & straddle)
        for r_ in range(R):                                      # every token tied in score with an uncertain one
            if bool(unc_sorted[r_].any()):
                unc_sorted[r_] |= torch.isin(so[r_], so[r_][unc_sorted[r_]].unique())
        unc = torch.zeros_like(unc_sorted).scatter(1, si, unc_sorted)
        base = (s32.double() - s32.double().max(-1, keepdim=True)[0]).exp() / q.double()
        hi = base.masked_fill(~((keep | unc) & topk_keep), -1).argmax(-1)
        lo = base.masked_fill(~(keep & ~unc), -1).argmax(-1)
        robust = hi == lo
    r = s32.double().masked_fill(~keep, float("-inf")).softmax(-1) / q.double()
    top2 = torch.topk(r, 2)[0]
    robust = robust & (top2[:, 0] > top2[:, 1] * (1 + 2.0 ** -18))
    return robust, r.argmax(-1)


def gate_logits(R, V, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * 2.5).to(dtype)


@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_gate_agrees_with_the_host_path_on_the_cpu(T, k, p):
    """On the gate's robust rows the fp64 restatement, `sampling_probs` + the spelled-out multinomial, and torch.multinomial itself draw
    the same tokens from the same seed; few rows are non-robust."""
    MC = pkg("modeling_core")
    R, V = 64, 32064
    logits = gate_logits(R, V, 1).float()
    probs = MC.sampling_probs(logits, T, k, p)
    g = torch.Generator().manual_seed(11)
    q = torch.empty_like(probs).exponential_(1, generator=g)
    spelled = (probs / q).argmax(-1)
    g = torch.Generator().manual_seed(11)
    drawn = torch.multinomial(probs, 1, generator=g).squeeze(1)
    assert torch.equal(spelled, drawn), "torch.multinomial(probs, 1) is no longer argmax(probs / exponential noise) on the CPU"
    ok, tok64 = robust_rows(logits, q, T, k, p)
    print(f"T={T} top_k={k} top_p={p}: {int((~ok).sum())} of {R} rows non-robust")
    assert float((~ok).float().mean()) <= MAX_NON_ROBUST
    assert torch.equal(tok64[ok], spelled[ok])


def test_sample_step_entry_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ullava_hip.h")).read()
    lib, ops = pkg("_lib"), pkg("ops")
    so = ctypes.CDLL(lib.LIB_PATH)
    assert re.search(r"\bint ull_sample_step\(", header), "ull_sample_step not declared in include/ullava_hip.h"
    assert "ull_sample_step" in lib.SIGNATURES and hasattr(so, "ull_sample_step")
    m = re.search(r"#define ULL_SAMPLE_MAX_V (\d+)", header)
    assert m and int(m.group(1)) == ops.SAMPLE_MAX_V and 32064 <= ops.SAMPLE_MAX_V       # the LLaMA vocabulary fits
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.sample_step(torch.zeros(1, 8), torch.ones(1, 8), 1.0, 0, None, torch.ones(1, dtype=torch.int32), None, None,
                        torch.zeros(1, 4, dtype=torch.int64), 0, torch.zeros(1, dtype=torch.int32))


def test_generate_refuses_unknown_sampler_and_the_ngram_ban():
    m = _tiny_core()
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="unknown sampler"):
        m.generate(input_ids=ids, max_new_tokens=2, sampler="nonsense")
    with pytest.raises(ValueError, match="unknown sampler"):
        m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, temperature=0.2, sampler="gpu")
    for do_sample in (False, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            m.generate(input_ids=ids, max_new_tokens=2, do_sample=do_sample, temperature=0.2, sampler="device", no_repeat_ngram_size=3)
    with pytest.raises(RuntimeError, match="GPU tensors"):        # no CPU path and no fallback to the host sampler
        m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, temperature=0.2, sampler="device")


def test_generate_refuses_a_vocabulary_beyond_the_lds_row_before_the_first_step():
    C, M, ops = pkg("configuration"), pkg("modeling_core"), pkg("ops")
    cfg = _tiny_core().config
    big = C.UllavaCoreConfig(vision_config=cfg.vision_config.to_dict() if hasattr(cfg.vision_config, "to_dict") else cfg.vision_config,
                             vision_hidden_layer=-2, mm_token_ids=cfg.mm_token_ids, vocab_size=ops.SAMPLE_MAX_V + 1, hidden_size=cfg.hidden_size,
                             intermediate_size=cfg.intermediate_size, num_hidden_layers=1, num_attention_heads=cfg.num_attention_heads)
    m = M.UllavaCoreForCausalLM(big)
    with pytest.raises(ValueError, match="LDS"):
        m.generate(input_ids=torch.tensor([[1, 2, 3]]), max_new_tokens=2, do_sample=True, temperature=0.2, sampler="device")


def test_evaluate_refuses_unknown_sampler_and_the_ngram_ban():
    MU = pkg("modeling_ullava")
    sig = inspect.signature(MU.UllavaForCausalLM.evaluate)
    assert list(sig.parameters)[-1] == "sampler" and sig.parameters["sampler"].default is None
    assert inspect.signature(pkg("modeling_core").UllavaCoreForCausalLM.generate).parameters["sampler"].default is None
    self = object.__new__(MU.UllavaForCausalLM)                  # the refusals come before the model is touched
    with pytest.raises(ValueError, match="unknown sampler"):
        MU.UllavaForCausalLM.evaluate(self, None, None, None, None, None, sampler="nonsense")
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        MU.UllavaForCausalLM.evaluate(self, None, None, None, None, None, sampler="device", no_repeat_ngram_size=3)


def test_reference_signatures_still_match():
    import test_host_cpu
    test_host_cpu.test_public_signatures_match_reference_fixture()
