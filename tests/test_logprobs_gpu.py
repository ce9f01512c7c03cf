"""Per-token log-probabilities on the GPU: the kernel (ops.token_logprobs / ull_token_logprobs) against a float64 log-softmax, then
generate(output_logprobs=True) in its three loops, score() and the fp8 twin on tiny models.

Tolerance of every comparison with float64 (`tol`): nothing fixed in advance.  torch's own fp32 log_softmax(rows.float()) is compared with
the float64 log-softmax of the same rows, and its largest error over the finite entries of the rows of the comparison is taken; the kernel
may be off by twice that plus one fp32 ulp of the result -- both sides sum V fp32 terms in different orders.  (The maximum is taken over the
comparison's rows, not row by row: where torch's error on one short row happens to be next to nothing the bound collapses to one ulp, which
three rounded operations do not promise -- 1 of 70 001 five-entry rows was at 1.17 of such a per-row bound.)  The measured |error| / tol of
every case is printed; the largest, 0.47, and the rest are recorded in profiles/logprobs_decode.txt.  Masked and out-of-range rows are
compared with `== 0.0`, NaN rows with isnan, runs with each other bit for bit."""
import pytest
import torch

from helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NINF = float("-inf")


def ulp32(x):
    """one fp32 ulp at |x| (x float64); the smallest subnormal at 0."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.where(x == 0, torch.full_like(x, 2.0 ** -149), torch.exp2(torch.floor(torch.log2(a)) - 23))


def reference(rows, ids):
    """-> (float64 log-softmax at ids, the tolerance of each described in the module docstring).  rows [R, V], ids [R] in [0, V)."""
    ref_all = torch.log_softmax(rows.double(), -1)
    t32 = torch.log_softmax(rows.float(), -1).double()
    fin = torch.isfinite(ref_all)
    err = torch.where(fin, (t32 - ref_all).abs(), torch.zeros_like(ref_all)).max()
    ref = ref_all.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    return ref, 2 * err + ulp32(ref)


def assert_close(got, rows, ids, what):
    ref, tol = reference(rows, ids)
    diff = (got.double() - ref).abs()
    ratio = float((diff / tol).max())
    print(f"{what}: max |err| {float(diff.max()):.3e}, largest |err| / tol {ratio:.3f}")
    assert bool((diff <= tol).all()), (what, diff.tolist(), tol.tolist())
    return ratio


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def make_rows(R, V, dtype, seed):
    """x[:, -1] of a [R, 3, V] tensor: rows 3 V elements apart (unaligned row bases for odd V in 16 bit); row 0 is N(0, 1), the later rows
    are scaled by 10 r and, from V = 7 on, carry +80 and -80 (exp overflows there without the max subtraction) and three -inf entries.
    -> (rows, ids): the ids avoid the -inf entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, 3, V, generator=g)
    ids = torch.randint(0, V, (R,), generator=g)
    for r in range(R):
        x[r] *= max(1, 10 * r)
        if V >= 7 and r % 2 == 0:
            x[r, :, (int(ids[r]) + 1) % V] = 80.0
            x[r, :, (int(ids[r]) + 2) % V] = -80.0
        if V >= 7:
            for off in (3, 4, V - 1):
                x[r, :, (int(ids[r]) + off) % V] = NINF
    return x.to(dtype).to(DEV)[:, -1], ids.to(DEV)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("V", [1, 7, 257, 4099, 32064])
@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "fp16", "fp32"])
def test_kernel_against_float64(dtype, V, R):
    ops = pkg("ops")
    rows, ids = make_rows(R, V, dtype, seed=1000 * R + V)
    assert rows.stride(0) == 3 * V and rows.stride(1) == 1
    got = ops.token_logprobs(rows, ids)
    assert got.dtype == F32 and got.shape == (R,)
    assert_close(got, rows, ids, f"{dtype} V={V} R={R}")
    if V >= 7:
        fin = rows.float()[torch.isfinite(rows.float())]
        assert float(fin.max()) >= 80.0 and float(fin.min()) <= -80.0 and bool(torch.isinf(rows.float()).any())

    # a second call on the same inputs: equal bits
    assert torch.equal(bits(ops.token_logprobs(rows, ids)), bits(got))

    # the same values on a 16-byte aligned row base and on one that is 2 or 4 bytes off it: the load path changes, the bits do not
    flat = torch.zeros(R, V + 16, dtype=dtype, device=DEV)
    for off in (0, 1):
        view = flat[:, 8 + off:8 + off + V]
        view.copy_(rows)
        assert (view.data_ptr() % 16 == 0) == (off == 0)          # (row 0's base; the later rows' bases fall as V has it)
        assert torch.equal(bits(ops.token_logprobs(view, ids)), bits(got)), off

    # ids as a column of a wider int64 tensor (the generate buffer's `buf[:, pos]`), out as a column of a wider fp32 tensor
    wide = torch.full((R, 6), 10 ** 12, dtype=torch.int64, device=DEV)
    wide[:, 4] = ids
    out = torch.full((R, 3), 7.0, device=DEV)
    ret = ops.token_logprobs(rows, wide[:, 4], out=out[:, 1])
    assert ret.data_ptr() == out[:, 1].data_ptr() and torch.equal(bits(out[:, 1]), bits(got))
    assert bool((out[:, 0] == 7.0).all()) and bool((out[:, 2] == 7.0).all())

    # one id -100, one id V, one row_mask zero: exactly 0.0 there, the other rows unchanged
    for what, bad in (("-100", -100), ("V", V), ("2^40", 2 ** 40)):
        ids2 = ids.clone()
        ids2[R // 2] = bad
        g2 = ops.token_logprobs(rows, ids2)
        assert int(bits(g2[R // 2:R // 2 + 1])) == 0, what                     # +0.0
        keep = torch.arange(R, device=DEV) != R // 2
        assert torch.equal(bits(g2[keep]), bits(got[keep])), what
    mask = torch.ones(R, dtype=torch.int32, device=DEV)
    mask[R - 1] = 0
    g3 = ops.token_logprobs(rows, ids, mask)
    assert float(g3[R - 1]) == 0.0
    assert torch.equal(bits(g3[:R - 1]), bits(got[:R - 1]))


@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("V", [7, 4099, 32064])
def test_kernel_all_minus_inf_and_nan_rows_give_nan(dtype, V):
    ops = pkg("ops")
    g = torch.Generator().manual_seed(V)
    x = torch.randn(4, 3, V, generator=g)
    x[0] = NINF                                     # the maximum is -inf
    x[1, :, V - 1] = float("nan")                   # a NaN in the element-wise tail / the last chunk
    x[2, :, 0] = float("nan")
    rows = x.to(dtype).to(DEV)[:, -1]
    ids = torch.tensor([0, 1, 2, 3], device=DEV)
    got = ops.token_logprobs(rows, ids)
    want = torch.log_softmax(rows.float(), -1).gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    assert torch.isnan(want[:3]).all(), "torch.log_softmax no longer gives NaN for these rows"
    assert torch.isnan(got[:3]).all() and not bool(torch.isnan(got[3]))
    assert_close(got[3:], rows[3:], ids[3:], f"finite row beside NaN rows, {dtype} V={V}")


def test_kernel_more_rows_than_one_grid_pass():
    """R = 70 001 rows (above the 65 536 blocks one launch starts): the blocks stride over the rows; contiguous fp32 rows of 5."""
    ops = pkg("ops")
    R, V = 70001, 5
    g = torch.Generator().manual_seed(5)
    rows = (torch.randn(R, V, generator=g) * 3).to(DEV)
    ids = torch.randint(0, V, (R,), generator=g).to(DEV)
    ids[-1] = -100
    got = ops.token_logprobs(rows, ids)
    assert float(got[-1]) == 0.0
    assert_close(got[:-1], rows[:-1], ids[:-1], "R = 70001")


def test_op_refusals():
    ops = pkg("ops")
    rows = torch.zeros(2, 3, 8, device=DEV, dtype=BF)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous in its last dim"):
        ops.token_logprobs(rows[:, :, 0], ids)
    with pytest.raises(RuntimeError, match="int64"):
        ops.token_logprobs(rows[:, -1], ids.int())
    with pytest.raises(RuntimeError, match=r"\[R, V\]"):
        ops.token_logprobs(rows, ids)
    with pytest.raises(RuntimeError, match="row_mask"):
        ops.token_logprobs(rows[:, -1], ids, torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.token_logprobs(rows[:, -1], ids.cpu())
    with pytest.raises(RuntimeError, match="out must be"):
        ops.token_logprobs(rows[:, -1], ids, out=torch.zeros(3, device=DEV))


# ---- generate() on the tiny model ---------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(dtype=BF):
    """2 layers, hidden 64, vocab 100, the seeded weights of the g1 fixture, text ids only."""
    from test_device_sampler_gpu import _tiny_core_on_gpu
    if dtype not in _MODELS:
        _MODELS[dtype] = _tiny_core_on_gpu(dtype, text_only=True)[1]
    return _MODELS[dtype]


def _leftpad_batch():
    """B = 3, L0 = 9: row 0 left-padded by 3, row 1 by 1, row 2 full."""
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, 90, (3, 9), generator=g)
    mask = torch.ones(3, 9, dtype=torch.int64)
    mask[0, :3] = 0
    mask[1, :1] = 0
    ids[mask == 0] = 0
    return ids.to(DEV), mask.to(DEV)


def _first(row, tok):
    row = row.tolist()
    return row.index(tok) if tok in row else None


def _pick_eos(new):
    """An id whose first occurrence among the dry run's new tokens [B, n] is at step >= 1 in some row and at least two steps later (or
    never) in another: that row finishes mid-way while the loop goes on."""
    n = new.shape[1]
    for r in range(new.shape[0]):
        for j in range(1, n - 2):
            tok = int(new[r, j])
            firsts = [_first(new[b], tok) for b in range(new.shape[0])]
            firsts = [n if f is None else f for f in firsts]
            if min(firsts) >= 1 and max(firsts) >= min(firsts) + 2:
                return tok
    raise AssertionError(f"no usable EOS id in the dry run {new.tolist()}")


def test_generate_without_cache_against_the_models_own_forward():
    m = _model()
    ids = torch.tensor([[1, 17, 33, 5, 61, 8, 29]], device=DEV)
    L0 = ids.shape[1]
    out = m.generate(input_ids=ids, max_new_tokens=6, use_cache=False, eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True)
    assert out.sequences.shape == (1, L0 + 6) and out.logprobs.shape == (1, 6) and out.logprobs.dtype == F32
    with torch.no_grad():
        rows = torch.cat([m.forward(input_ids=out.sequences[:, :L0 + j]).logits[:, -1] for j in range(6)])
    assert_close(out.logprobs[0], rows, out.sequences[0, L0:], "use_cache=False, greedy")
    assert bool((out.logprobs < 0).all())
    # the flag changes nothing else, and without it the result carries no such entry
    plain = m.generate(input_ids=ids, max_new_tokens=6, use_cache=False, eos_token_id=-1, return_dict_in_generate=True)
    assert torch.equal(plain.sequences, out.sequences) and "logprobs" not in plain


@pytest.mark.parametrize("use_cache", [False, True])
def test_generate_finished_rows_get_zero_and_eos_its_real_value(use_cache):
    m = _model()
    ids, mask = _leftpad_batch()
    L0, NEW = ids.shape[1], 12
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, use_cache=use_cache, return_dict_in_generate=True, output_logprobs=True)
    dry = m.generate(**kw, eos_token_id=-1)
    assert dry.logprobs.shape == (3, NEW) and bool((dry.logprobs < 0).all())
    eos = _pick_eos(dry.sequences[:, L0:])
    out = m.generate(**kw, eos_token_id=eos)
    new = out.sequences[:, L0:]
    n_new = new.shape[1]
    assert out.logprobs.shape == (3, n_new)
    firsts = [_first(new[b], eos) for b in range(3)]
    assert any(f is not None and f < n_new - 1 for f in firsts), (firsts, n_new)
    for b, f in enumerate(firsts):
        end = n_new if f is None else f + 1
        assert bool((out.logprobs[b, :end] < 0).all()), (b, out.logprobs[b].tolist())        # the EOS column included
        assert bool((out.logprobs[b, end:] == 0.0).all()), (b, out.logprobs[b].tolist())
        assert bool((new[b, end:] == eos).all())                                               # (pad fill = the EOS id)
        # the live columns are the dry run's: the same tokens from the same logits
        assert torch.equal(bits(out.logprobs[b, :end]), bits(dry.logprobs[b, :end]))


@pytest.mark.parametrize("sample", [False, True], ids=["greedy-ngram-ban", "host-sampler"])
def test_generate_host_loop_finished_rows_get_zero_and_eos_its_real_value(sample):
    """The per-step host loop (reached through no_repeat_ngram_size, or through the host sampler) with an EOS id that one row meets mid-way:
    its mask is `unfinished` as it stood BEFORE the step, so the EOS column is scored and only the columns behind it are 0.0."""
    m = _model()
    ids, mask = _leftpad_batch()
    L0, NEW = ids.shape[1], 12
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, use_cache=True, return_dict_in_generate=True, output_logprobs=True)
    kw.update(dict(do_sample=True, temperature=0.7, top_k=50) if sample else dict(no_repeat_ngram_size=3))
    torch.manual_seed(7)
    dry = m.generate(**kw, eos_token_id=-1)
    eos = _pick_eos(dry.sequences[:, L0:])
    torch.manual_seed(7)
    out = m.generate(**kw, eos_token_id=eos)
    new = out.sequences[:, L0:]
    n_new = new.shape[1]
    assert out.logprobs.shape == (3, n_new)
    firsts = [_first(new[b], eos) for b in range(3)]
    assert any(f is not None and f < n_new - 1 for f in firsts), (firsts, n_new)
    for b, f in enumerate(firsts):
        end = n_new if f is None else f + 1
        assert bool((out.logprobs[b, :end] < 0).all()), (b, out.logprobs[b].tolist())        # the EOS column included
        assert bool((out.logprobs[b, end:] == 0.0).all()), (b, out.logprobs[b].tolist())
        if not sample:                                  # (a sampled run draws every row's noise from one stream: only greedy repeats the dry run)
            assert torch.equal(bits(out.logprobs[b, :end]), bits(dry.logprobs[b, :end]))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_generate_ngram_ban_does_not_reach_the_logprobs(dtype):
    """no_repeat_ngram_size=2 on a repetitive prompt: the ban writes -inf into the scores the token is picked from, and the log-probabilities
    still come from the raw logits -- float64 log-softmax of the model's own forward, not of the banned scores (on an fp32 model the fp32
    scores are a view of the logits; the loop bans on a copy)."""
    MC = pkg("modeling_core")
    m = _model(dtype)
    ids = torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6]], device=DEV)
    L0, NEW = ids.shape[1], 8
    out = m.generate(input_ids=ids, max_new_tokens=NEW, use_cache=False, eos_token_id=-1, no_repeat_ngram_size=2, return_dict_in_generate=True,
                     output_logprobs=True)
    seq = out.sequences
    assert seq.shape == (1, L0 + NEW) and out.logprobs.shape == (1, NEW)
    with torch.no_grad():
        rows = torch.cat([m.forward(input_ids=seq[:, :L0 + j]).logits[:, -1] for j in range(NEW)])
    banned_rows = rows.double().clone()
    n_banned = 0
    for j in range(NEW):
        banned = MC.no_repeat_ngram_banned_tokens(seq[:, :L0 + j].tolist(), 2)[0]
        n_banned += len(banned)
        if banned:
            banned_rows[j, torch.as_tensor(banned, device=DEV)] = NINF
    new = seq[0, L0:]
    assert_close(out.logprobs[0], rows, new, f"n-gram ban, {dtype}")
    # the check tells the two apart: scored on the banned rows, some step would be off by far more than the tolerance
    ref, tol = reference(rows, new)
    post = torch.log_softmax(banned_rows, -1).gather(-1, new.unsqueeze(-1)).squeeze(-1)
    print(f"banned ids over the {NEW} steps: {n_banned}; largest raw / banned difference {float((post - ref).abs().max()):.3e}, tol {float(tol.max()):.3e}")
    assert n_banned > 0 and float(((post - ref).abs() - tol).max()) > 1e-3


def test_generate_fused_loop_overrun_is_trimmed():
    """B = 1, the row finishes within three steps while the fused loop looks at the host after eight: five or more columns go."""
    m = _model()
    ids = torch.tensor([[1, 17, 33, 5, 61, 8, 29]], device=DEV)
    L0 = ids.shape[1]
    kw = dict(input_ids=ids, max_new_tokens=16, use_cache=True, return_dict_in_generate=True, output_logprobs=True)
    dry = m.generate(**kw, eos_token_id=-1)
    eos = int(dry.sequences[0, L0 + 2])
    out = m.generate(**kw, eos_token_id=eos)
    n_new = out.sequences.shape[1] - L0
    assert 1 <= n_new <= 3 and out.logprobs.shape == (1, n_new)
    assert torch.equal(bits(out.logprobs), bits(dry.logprobs[:, :n_new])) and bool((out.logprobs < 0).all())


def test_generate_fused_loop_equals_the_per_step_check():
    """A stopping criterion that never fires makes the fused loop look at the host after every step (no overrun, no trim)."""
    m = _model()
    ids, mask = _leftpad_batch()
    L0 = ids.shape[1]
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=12, use_cache=True, return_dict_in_generate=True, output_logprobs=True)
    dry = m.generate(**kw, eos_token_id=-1)
    eos = _pick_eos(dry.sequences[:, L0:])
    a = m.generate(**kw, eos_token_id=eos)
    calls = []

    def never(seq, scores):
        calls.append(seq.shape[1])
        return False

    b = m.generate(**kw, eos_token_id=eos, stopping_criteria=[never])
    assert calls and torch.equal(a.sequences, b.sequences)
    assert torch.equal(bits(a.logprobs), bits(b.logprobs))


def test_generate_host_sampler_equals_device_sampler():
    """One seed, the host loop (torch.multinomial) against sampler="device": the same noise, so the same ids wherever the draw is not a
    near-tie (tests/test_device_sampler_gpu.py measures that gate); column j of a row is compared while the row's ids agree up to j, and
    nearly all columns must be.  The log-probabilities come from the same kernel on the same logits: equal bits."""
    m = _model()
    ids, mask = _leftpad_batch()
    L0 = ids.shape[1]
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=12, use_cache=True, do_sample=True, temperature=0.7, top_k=50, top_p=0.9,
              eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True)
    compared = total = 0
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        host = m.generate(**kw)
        torch.manual_seed(seed)
        dev = m.generate(**kw, sampler="device")
        assert host.logprobs.shape == dev.logprobs.shape == (3, 12)
        for b in range(3):
            same = (host.sequences[b, L0:] == dev.sequences[b, L0:]).int().cumprod(0)
            n = int(same.sum())
            assert torch.equal(bits(host.logprobs[b, :n]), bits(dev.logprobs[b, :n])), (seed, b)
            compared += n
            total += 12
    print(f"host against device sampler: {compared} of {total} columns compared")
    assert compared >= 0.9 * total
    # raw distribution: the sampled token's log-probability is not the warped one (temperature 0.7 would sharpen it)
    assert bool((host.logprobs < 0).all())


# Prompt-lookup: a verify step's multi-token forward against the plain loop's one-token forwards.  Measured on this fixture with the kernels
# of the commit before this feature (profiles/logprobs_decode.txt): the largest |logit difference| over the 32 positions is 0.0 -- this tiny
# model's two paths are bit-identical, as tests/test_prompt_lookup_gpu.py records (MEASURED_PATH_DIFF).  A logit difference of at most d moves a
# log-probability by at most 2 d (d on the token's own logit, d on the log-sum-exp); twice that is allowed.
SPEC_LOGIT_DIFF = 0.0
SPEC_LOGPROB_TOL = 2 * (2 * SPEC_LOGIT_DIFF)


def test_generate_prompt_lookup_against_the_plain_loop():
    from test_prompt_lookup_gpu import K, _prompt
    ops = pkg("ops")
    m = _model()
    ids = _prompt()
    L0 = ids.shape[1]
    kw = dict(input_ids=ids, use_cache=True, eos_token_id=-1, return_dict_in_generate=True, output_logprobs=True)
    plain = m.generate(**kw, max_new_tokens=32)
    drafts, orig = [], ops.spec_step

    def spy(*a, **k):
        drafts.append(a[7])
        return orig(*a, **k)

    ops.spec_step = spy
    try:
        spec = m.generate(**kw, max_new_tokens=32, prompt_lookup_num_tokens=K)
        assert any(d > 0 for d in drafts) and len(drafts) < 32, drafts       # drafts were offered, and fewer forwards than tokens: some accepted
        # 30 new tokens: the last step is cut by max_new_tokens inside its accepted drafts or right after them
        spec30 = m.generate(**kw, max_new_tokens=30, prompt_lookup_num_tokens=K)
    finally:
        ops.spec_step = orig
    assert torch.equal(spec.sequences, plain.sequences)
    assert spec.logprobs.shape == plain.logprobs.shape == (1, 32)
    diff = float((spec.logprobs.double() - plain.logprobs.double()).abs().max())
    print(f"prompt lookup against the plain loop: max |log-probability difference| {diff:.3e} (allowed {SPEC_LOGPROB_TOL:.3e})")
    assert diff <= SPEC_LOGPROB_TOL
    # nothing behind the last valid token leaks: the shorter run is the longer run's prefix, and it has exactly 30 columns
    assert spec30.sequences.shape == (1, L0 + 30) and spec30.logprobs.shape == (1, 30)
    assert float((spec30.logprobs.double() - plain.logprobs[:, :30].double()).abs().max()) <= SPEC_LOGPROB_TOL
    # EOS inside the run: the result ends with the EOS token's own (non-zero) entry
    eos = int(plain.sequences[0, L0 + 9])
    cut = m.generate(input_ids=ids, use_cache=True, eos_token_id=eos, return_dict_in_generate=True, output_logprobs=True, max_new_tokens=32,
                     prompt_lookup_num_tokens=K)
    n_new = cut.sequences.shape[1] - L0
    assert n_new <= 10 and int(cut.sequences[0, -1]) == eos and cut.logprobs.shape == (1, n_new)
    assert float((cut.logprobs.double() - plain.logprobs[:, :n_new].double()).abs().max()) <= SPEC_LOGPROB_TOL and float(cut.logprobs[0, -1]) < 0


def test_generate_fp8_weights_equal_the_dequantized_twin():
    from test_fp8_weights_gpu import _tiny_core_pair
    fx, twin, fp8 = _tiny_core_pair()
    prompt, images = fx["greedy_prompt"].to(DEV), fx["images"].to(DEV)
    for use_cache in (False, True):
        kw = dict(input_ids=prompt, images=images[:1], max_new_tokens=8, use_cache=use_cache, eos_token_id=-1, return_dict_in_generate=True,
                  output_logprobs=True)
        a, b = twin.generate(**kw), fp8.generate(**kw)
        assert torch.equal(a.sequences, b.sequences), use_cache
        assert a.logprobs.shape == (1, 8) and bool((a.logprobs < 0).all())
        assert torch.equal(bits(a.logprobs), bits(b.logprobs)), use_cache


def test_evaluate_returns_the_logprobs_as_a_fourth_value():
    from helpers import load_fixture
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    g = torch.Generator().manual_seed(fx["images_sam_seed"])
    _ = torch.randn(2, 3, 28, 28, generator=g)
    images_sam = torch.randn(2, 3, 1024, 1024, generator=g).to(BF)[:1].to(DEV)
    args = (images_sam, fx["images"][:1].to(DEV), fx["input_ids"][:1].to(DEV), [fx["size_list"][0]], [fx["resize_list"][0]])
    ids_p, masks_p, boxes_p = model.evaluate(*args, max_new_tokens=6, temperature=0.0)
    ids_l, masks_l, boxes_l, lp = model.evaluate(*args, max_new_tokens=6, temperature=0.0, output_logprobs=True)
    assert torch.equal(ids_p, ids_l)
    assert len(masks_p) == len(masks_l) and all(torch.equal(x, y) for x, y in zip(masks_p, masks_l))
    assert len(boxes_p) == len(boxes_l) and all(torch.equal(x, y) for x, y in zip(boxes_p, boxes_l))
    assert lp.dtype == F32 and lp.shape == (1, ids_l.shape[1] - args[2].shape[1])


# ---- score() ------------------------------------------------------------------------------------------------------------------------------
def _score_batch():
    """B = 2, L = 12; row 0 left-padded by 2; labels -100 over the first 5 positions (the prompt) and wherever the mask is 0."""
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(3, 90, (2, 12), generator=g)
    mask = torch.ones(2, 12, dtype=torch.int64)
    mask[0, :2] = 0
    ids[mask == 0] = 0
    labels = ids.clone()
    labels[:, :5] = -100
    return ids.to(DEV), mask.to(DEV), labels.to(DEV)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_score_against_the_models_own_forward(dtype):
    m = _model(dtype)
    ids, mask, labels = _score_batch()
    out = m.score(ids, attention_mask=mask, labels=labels)
    assert set(out) == {"token_logprobs", "sequence_logprob", "num_tokens"}
    lp = out.token_logprobs
    assert lp.dtype == F32 and lp.shape == (2, 11)
    with torch.no_grad():
        logits = m.forward(input_ids=ids, attention_mask=mask).logits
    tgt = labels[:, 1:]
    scored = tgt != -100
    assert bool((lp[~scored] == 0.0).all()) and bool((lp[scored] < 0).all())
    assert_close(lp[scored], logits[:, :-1][scored], tgt[scored], f"score {dtype}")
    assert out.num_tokens.tolist() == [7, 7] == scored.sum(-1).tolist()
    assert torch.equal(bits(out.sequence_logprob), bits(lp.sum(-1)))

    # labels default to input_ids: every position whose target is attended counts; the padded targets give exactly 0.0
    dflt = m.score(ids, attention_mask=mask)
    assert dflt.num_tokens.tolist() == [10, 11]
    assert bool((dflt.token_logprobs[0, :1] == 0.0).all()) and bool((dflt.token_logprobs[0, 1:] < 0).all())
    assert torch.equal(bits(dflt.token_logprobs[:, 4:]), bits(lp[:, 4:]))


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_score_agrees_with_the_training_loss(dtype):
    """-sum(sequence_logprob) / sum(num_tokens) against forward(labels=...).loss.  Both are means of the same N = 14 per-token values, each
    within `tol` of float64 (the kernel tolerance; the loss kernel's fp32 log-softmax is held to the same), summed in fp32 in two orders
    (N - 1 additions, each off by at most half an ulp of a partial sum <= N |loss|) and divided once.  forward() returns the loss in the
    model's dtype, so a bf16 model adds half a bf16 ulp of the loss.  Measured on an MI355X (profiles/logprobs_decode.txt):
    fp32 model |difference| 4.8e-07 of 2.1e-05 allowed; bf16 model 1.8e-03 of 1.0e-02 (the bf16 rounding of the loss is nearly all of it)."""
    m = _model(dtype)
    ids, mask, labels = _score_batch()
    out = m.score(ids, attention_mask=mask, labels=labels)
    with torch.no_grad():
        fw = m.forward(input_ids=ids, attention_mask=mask, labels=labels)
    mine = -out.sequence_logprob.sum() / out.num_tokens.sum()
    scored = labels[:, 1:] != -100
    ref, tol = reference(fw.logits[:, :-1][scored], labels[:, 1:][scored])
    N = int(scored.sum())
    ref_loss = float(-ref.sum() / N)
    margin = 2 * (float(tol.max()) + N * 2.0 ** -23 * abs(ref_loss))
    if dtype == BF:
        margin += 2.0 ** -9 * abs(ref_loss)
    diff = abs(float(mine) - float(fw.loss.float()))
    print(f"loss consistency {dtype}: score {float(mine):.7f} forward {float(fw.loss):.7f} float64 {ref_loss:.7f}; "
          f"|difference| {diff:.3e}, allowed {margin:.3e}")
    assert N == 14 and diff <= margin
    assert abs(float(mine) - ref_loss) <= float(tol.max()) + N * 2.0 ** -23 * abs(ref_loss)      # score()'s own half of the margin


def test_score_of_the_full_model_delegates_to_the_language_model():
    from helpers import load_fixture
    from test_fp8_weights_gpu import _tiny_full
    fx = load_fixture("g8_full_tiny_bf16.pt")
    model = _tiny_full(fx)
    ids = fx["input_ids"][:1].to(DEV)
    images = fx["images"][:1].to(DEV)
    a = model.score(ids, images=images)
    b = model.llm.score(ids, images=images)
    assert set(a) == set(b) == {"token_logprobs", "sequence_logprob", "num_tokens"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
