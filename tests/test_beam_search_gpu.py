"""Beam search on the GPU: ops.beam_step against the host rule (generation.beam_step_reference) bit for bit, KVCache.gather_rows /
replicated against index_select on the cache's logical view, and generate(num_beams=K) end to end on the tiny model against
generation.beam_search_reference driven by the same model's forwards.  The host rule is fed the device's own log-probabilities
(ops.token_logprobs over a whole row: row_stride 0, R = V, ids = arange(V)), which the beam step must reproduce bit for bit."""
import itertools

import pytest
import torch

from helpers import pkg, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF, F16, F32], ids=["bf16", "fp16", "fp32"])
GUARD, SENT = 16, -77


def bits(t):
    return t.contiguous().view(torch.int32)


def row_logprobs(logits):
    """[R, V] -> fp32 [R, V] on the CPU: every entry of every row through ops.token_logprobs."""
    ops = pkg("ops")
    R, V = logits.shape
    ids = torch.arange(V, device=DEV)
    return torch.stack([ops.token_logprobs(logits[r].unsqueeze(0).expand(V, V), ids) for r in range(R)]).cpu()


def guarded(t):
    """a device copy of `t` inside a buffer with sentinel words on both sides -> (the view, the whole buffer)."""
    big = torch.full((t.numel() + 2 * GUARD,), SENT, dtype=t.dtype, device=DEV)
    view = big[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, big


def guards_intact(big):
    return bool((big[:GUARD] == SENT).all()) and bool((big[-GUARD:] == SENT).all())


def random_state(B, K, L0, Lmax, cur, V, seed, first_step=False, pool="empty"):
    """a BeamState on the CPU in the middle of a search: random ids up to `cur`, decreasing running scores, and a pool that is empty,
    half full or full (fin set on the filled rows)."""
    G = pkg("generation")
    g = torch.Generator().manual_seed(seed)
    st = G.BeamState(torch.randint(0, V, (B, L0), generator=g), K, Lmax - L0, pad=V - 1)
    if not first_step:
        st.run[:, :, L0:cur] = torch.randint(0, V, (B, K, cur - L0), generator=g)
        st.run_sc[:] = -torch.rand(B, K, generator=g).cumsum(1) * 3
    n_fin = dict(empty=0, half=(K + 1) // 2, full=K)[pool]
    if n_fin and cur > L0:
        st.pool_sc[:, :n_fin] = -torch.rand(B, n_fin, generator=g).cumsum(1) * 2
        st.pool_len[:, :n_fin] = torch.randint(1, cur - L0 + 1, (B, n_fin), generator=g, dtype=torch.int32)
        st.fin[:, :n_fin] = 1
        st.pool[:, :n_fin, L0:cur] = torch.randint(0, V, (B, n_fin, cur - L0), generator=g)
    return st


def check_step(logits, st, cur, eos, length_penalty=1.0, early_stopping=False, pick=None, what=""):
    """one ops.beam_step on guarded device copies of `st` against beam_step_reference on `st` itself: everything exact."""
    ops, G = pkg("ops"), pkg("generation")
    B, Kin, V = logits.shape
    K, L0, Lmax = st.K, st.L0, st.Lmax
    lp = row_logprobs(logits.reshape(B * Kin, V)).view(B, Kin, V)
    if pick is not None:
        lp = torch.where(torch.isneginf(pick.float().cpu()), torch.tensor(float("-inf")), lp)
    lp = lp.expand(B, K, V).clone()
    dev = {n: guarded(getattr(st, n)) for n in ("run", "pool", "run_sc", "pool_sc", "pool_len", "fin", "open")}
    run_out, pool_out = guarded(torch.full_like(st.run, SENT + 1)), guarded(torch.full_like(st.pool, SENT + 1))
    parent = guarded(torch.full((B * K,), SENT + 1, dtype=torch.int32))
    go = guarded(torch.full((1,), SENT + 1, dtype=torch.int32))
    cand_v = guarded(torch.zeros(B * K * ops.BEAM_MAX_CAND, dtype=F32))
    cand_t = guarded(torch.zeros(B * K * ops.BEAM_MAX_CAND, dtype=torch.int32))
    eos_dev = None if not eos else torch.tensor(eos, device=DEV)
    p_fin, p_hyp = G.beam_powers(cur, L0, Lmax, length_penalty, early_stopping)
    run_in, pool_in = st.run.clone(), st.pool.clone()
    ops.beam_step(logits, pick, dev["run"][0], run_out[0], dev["pool"][0], pool_out[0], dev["run_sc"][0], dev["pool_sc"][0], dev["pool_len"][0],
                  dev["fin"][0], dev["open"][0], eos_dev, st.pad, L0, cur, p_fin, p_hyp, early_stopping, cand_v[0], cand_t[0], parent[0], go[0])
    torch.cuda.synchronize()
    want_parent, want_go = G.beam_step_reference(st, lp, cur, eos, length_penalty, early_stopping)
    tag = (what, tuple(logits.shape), str(logits.dtype), K, cur, eos, length_penalty, early_stopping)
    assert torch.equal(parent[0].cpu(), want_parent), (tag, parent[0].tolist(), want_parent.tolist())
    assert torch.equal(run_out[0].cpu(), st.run), tag
    assert torch.equal(bits(dev["run_sc"][0].cpu()), bits(st.run_sc)), (tag, dev["run_sc"][0].tolist(), st.run_sc.tolist())
    assert torch.equal(pool_out[0].cpu(), st.pool), tag
    assert torch.equal(bits(dev["pool_sc"][0].cpu()), bits(st.pool_sc)), (tag, dev["pool_sc"][0].tolist(), st.pool_sc.tolist())
    assert torch.equal(dev["pool_len"][0].cpu(), st.pool_len) and torch.equal(dev["fin"][0].cpu(), st.fin), tag
    assert torch.equal(dev["open"][0].cpu(), st.open) and int(go[0]) == int(want_go), (tag, int(go[0]), want_go)
    # the inputs of the double buffers stay, and nothing is written past any end
    assert torch.equal(dev["run"][0].cpu(), run_in) and torch.equal(dev["pool"][0].cpu(), pool_in), tag
    for _, big in list(dev.values()) + [run_out, pool_out, parent, go, cand_v, cand_t]:
        assert guards_intact(big), tag
    assert 0 <= int(st.run[:, :, cur].min()) and int(st.run[:, :, cur].max()) < V
    return want_parent, want_go


def make_logits(B, Kin, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Kin, V, generator=g) * 3).to(dtype).to(DEV)


def eos_for(logits, n_eos, seed):
    """EOS ids that matter: the best token of the first row, then random ones."""
    V = logits.shape[-1]
    g = torch.Generator().manual_seed(seed)
    ids = [int(logits[0, 0].float().argmax())]
    while len(ids) < n_eos:
        t = int(torch.randint(0, V, (1,), generator=g))
        if t not in ids:
            ids.append(t)
    return ids[:n_eos]


SHAPES = list(itertools.product((2, 3, 5, 16), (1, 3), (0, 1, 2), ("one", "K")))


@DTYPES
@pytest.mark.parametrize("V", [7, 33, 4097])
def test_step_against_the_host_rule(dtype, V):
    """odd and unaligned rows, more than one round of the 16-byte-chunk loop (4097 fp32), every K x B x n_eos x Kin; Kin == 1 is the
    prefill step with its [0, -1e9, ...] scores.  Rows sit at an odd element offset for half of the cases (the element-wise load path)."""
    for i, (K, B, n_eos, kin) in enumerate(SHAPES):
        Kin = 1 if kin == "one" else K
        L0, Lmax = 3, 9
        cur = L0 if Kin == 1 else 5
        wide = make_logits(B, Kin, V + 3, dtype, 100 + i)
        logits = wide[:, :, 1:V + 1] if i & 1 else wide[:, :, :V].contiguous()
        st = random_state(B, K, L0, Lmax, cur, V, 200 + i, first_step=Kin == 1, pool=("empty", "half", "full")[i % 3] if Kin != 1 else "empty")
        check_step(logits, st, cur, eos_for(logits, n_eos, i), length_penalty=(0.0, 1.0, 2.0)[i % 3], early_stopping=(False, True, "never")[(i // 3) % 3])


@DTYPES
@pytest.mark.parametrize("K, B, n_eos, kin", [(2, 1, 0, "K"), (3, 3, 2, "K"), (5, 1, 1, "one"), (16, 3, 1, "K"), (16, 1, 2, "one"), (4, 3, 0, "K")])
def test_step_vocabulary_sized_rows(dtype, K, B, n_eos, kin):
    V, L0, Lmax = 32064, 3, 9
    Kin = 1 if kin == "one" else K
    cur = L0 if Kin == 1 else 6
    logits = make_logits(B, Kin, V, dtype, 7 * K + B)
    st = random_state(B, K, L0, Lmax, cur, V, K + B, first_step=Kin == 1, pool="half" if Kin != 1 else "empty")
    check_step(logits, st, cur, eos_for(logits, n_eos, K), length_penalty=2.0, early_stopping=K == 3)


@DTYPES
def test_step_ties_across_beams_and_inside_a_row(dtype):
    """two beams with identical rows and identical scores (the flat index decides across beams), duplicated values inside a row, and
    different logits that round to one accumulated score next to a large running score."""
    B, K, V, L0, Lmax, cur = 1, 3, 33, 3, 9, 5
    row = (torch.arange(V) % 5).float()
    logits = row.expand(B, K, V).clone().to(dtype).to(DEV)
    st = random_state(B, K, L0, Lmax, cur, V, 1)
    st.run_sc[:] = torch.tensor([-1.5, -1.5, -1.5])
    parent, _ = check_step(logits, st, cur, [4], what="equal beams")
    assert parent.tolist() == [0, 0, 0]
    st = random_state(B, K, L0, Lmax, cur, V, 2)
    st.run_sc[:] = torch.tensor([-3.0e4, -3.0e4, -3.0e4 - 0.25])                       # ulp(3e4) = 2^-9 * 2^... : small logit steps vanish
    fine = torch.linspace(0, 0.01, V).expand(B, K, V).clone().to(dtype).to(DEV)
    check_step(fine, st, cur, [1, 2], what="absorbed")


@DTYPES
def test_step_minus_infinity_rows_and_a_banned_top_token(dtype):
    B, K, V, L0, Lmax, cur = 3, 2, 33, 3, 9, 4
    logits = make_logits(B, K, V, dtype, 5)
    sparse = torch.full_like(logits, float("-inf"))
    sparse[..., [3, 17, 32]] = logits[..., [3, 17, 32]]
    check_step(sparse, random_state(B, K, L0, Lmax, cur, V, 3), cur, [17], what="three finite entries")
    # the pick copy ops.ngram_ban writes: the top token of every row at -inf; the normalizer keeps reading the raw row
    pick = logits.clone()
    pick.scatter_(-1, logits.float().argmax(-1, keepdim=True), float("-inf"))
    st = random_state(B, K, L0, Lmax, cur, V, 4)
    parent, _ = check_step(logits, st, cur, [5], pick=pick, what="banned top")
    tops = logits.float().argmax(-1).cpu().view(-1)
    assert all(int(st.run.view(B * K, -1)[r, cur]) != int(tops[int(parent[r])]) for r in range(B * K))
    first = pkg("generation").BeamState(torch.zeros(B, L0, dtype=torch.int64), K, Lmax - L0, pad=V - 1)
    check_step(logits[:, :1], first, L0, [5], pick=pick[:, :1], what="banned top, Kin = 1")
    assert all(int(first.run[b, 0, L0]) != int(tops[b * K]) for b in range(B))


@DTYPES
def test_step_candidates_from_the_minus_1e9_beams(dtype):
    """V = 7, K = 5 at the prefill step: KK = 10 > V, so candidates come from the beams at -1e9, where the log-probability is absorbed and
    everything ties."""
    G = pkg("generation")
    for n_eos, Kin in ((0, 1), (1, 1), (2, 5), (1, 5)):
        logits = make_logits(2, Kin, 7, dtype, 9 + n_eos)
        st = G.BeamState(torch.tensor([[1, 2, 3], [4, 5, 6]]), 5, 4, pad=6)
        check_step(logits, st, 3, eos_for(logits, n_eos, 1), what="absorbed beams")


@DTYPES
def test_step_last_position_and_full_pool(dtype):
    """cur + 1 == Lmax: every candidate hits; a pool that is already full under each early_stopping, open and closed items."""
    B, K, V, L0, Lmax = 3, 4, 33, 3, 7
    for es in (False, True, "never"):
        for lp in (0.0, 1.0, 2.0):
            logits = make_logits(B, K, V, dtype, 11)
            st = random_state(B, K, L0, Lmax, Lmax - 1, V, 12, pool="full")
            _, go = check_step(logits, st, Lmax - 1, [2], lp, es, what="last position")
            assert not go
            for cur in (4, 5):
                st = random_state(B, K, L0, Lmax, cur, V, 13 + cur, pool="full")
                st.open[1] = 0
                if es == "never":
                    st.pool_sc[:] -= 40.0                                            # a pool the running beams can still beat
                check_step(logits, st, cur, eos_for(logits, 2, 3), lp, es, what="full pool")


def test_step_refusals():
    ops, G = pkg("ops"), pkg("generation")
    st = G.BeamState(torch.zeros(1, 3, dtype=torch.int64, device=DEV), 4, 4, pad=0)
    out, pout = torch.empty_like(st.run), torch.empty_like(st.pool)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)                                       # noqa: E731
    args = lambda lg, eos, ro=out: (lg, None, st.run, ro, st.pool, pout, st.run_sc, st.pool_sc, st.pool_len, st.fin, st.open, eos, 0, 3, 3, 1.0, 1.0,  # noqa: E731
                                    False, torch.zeros(256, device=DEV), i32(256), i32(4), i32(1))
    with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):                            # K * V < KK
        ops.beam_step(torch.zeros(1, 4, 1, dtype=BF, device=DEV), None, *args(None, None)[2:])
    with pytest.raises(RuntimeError, match="ULL_ERR_SHAPE"):                            # (1 + n_eos) * K > 64
        ops.beam_step(*args(torch.zeros(1, 4, 64, dtype=BF, device=DEV), torch.arange(16, device=DEV)))
    with pytest.raises(RuntimeError, match="double-buffered"):
        ops.beam_step(*args(torch.zeros(1, 4, 64, dtype=BF, device=DEV), None, st.run))
    with pytest.raises(ValueError, match="Kin"):
        ops.beam_step(*args(torch.zeros(1, 2, 64, dtype=BF, device=DEV), None))


# ---- the KV rows --------------------------------------------------------------------------------------------------------------------------
PARENTS = dict(identity=[0, 1, 2, 3, 4, 5], all_zero=[0, 0, 0, 3, 3, 3], swap=[1, 0, 2, 3, 5, 4], cycle=[1, 2, 0, 5, 3, 4])


def filled_cache(dtype, rows, per_item, p0, length, seed, layers=2, H=2, hd=8, smax=128):
    """random K and V^T everywhere (every slot of the buffers), the rows of an item equal below p0 -- what a replicated prefill leaves."""
    ops, KV = pkg("ops"), pkg("kv_cache")
    g = torch.Generator().manual_seed(seed)
    c = KV.KVCache(layers, rows, H, hd, smax, DEV, dtype)
    slot = ops.vt_unpermute_index(c.smax)[:p0].to(DEV)
    for li in range(layers):
        c.k[li].copy_(torch.randn(c.k[li].shape, generator=g).to(dtype))
        c.vt[li].copy_(torch.randn(c.vt[li].shape, generator=g).to(dtype))
        for r in range(rows):
            first = r - r % per_item
            c.k[li][r, :, :p0] = c.k[li][first, :, :p0]
            c.vt[li][r][..., slot] = c.vt[li][first][..., slot]
    c.length = length
    return c


@DTYPES
@pytest.mark.parametrize("kind", list(PARENTS))
def test_kv_gather_rows_equals_index_select(dtype, kind):
    parent = torch.tensor(PARENTS[kind], dtype=torch.int32, device=DEV)
    for p0, n in itertools.product((1, 31, 32, 33, 65), (1, 2, 31, 33)):
        p1 = p0 + n
        c = filled_cache(dtype, 6, 3, p0, p1, 1000 * p0 + n)
        before_k, before_vt = [t.clone() for t in c.k], [t.clone() for t in c.vt]
        want = [(k.index_select(0, parent.long()), v.index_select(0, parent.long())) for k, v in c.to_legacy_cache()]
        c.gather_rows(parent, p0, p1)
        got = c.to_legacy_cache()
        q0, q1 = p0 & ~31, (p1 + 31) & ~31
        for li in range(len(c)):
            assert torch.equal(got[li][0], want[li][0]) and torch.equal(got[li][1], want[li][1]), (kind, p0, n, li)
            k, vt = c.k[li], c.vt[li]
            # nothing outside the range (K) / outside the touched 32-key blocks (V^T), and nothing at all in a row that stays
            assert torch.equal(k[:, :, :p0], before_k[li][:, :, :p0]) and torch.equal(k[:, :, p1:], before_k[li][:, :, p1:]), (kind, p0, n)
            assert torch.equal(vt[..., :q0], before_vt[li][..., :q0]) and torch.equal(vt[..., q1:], before_vt[li][..., q1:]), (kind, p0, n)
            for r, p in enumerate(PARENTS[kind]):
                src = before_k[li][p] if p != r else before_k[li][r]
                assert torch.equal(k[r, :, p0:p1], src[:, p0:p1])
                if p == r:
                    assert torch.equal(k[r], before_k[li][r]) and torch.equal(vt[r], before_vt[li][r]), (kind, p0, n, r)
                else:
                    assert torch.equal(vt[r][..., q0:q1], before_vt[li][p][..., q0:q1]), (kind, p0, n, r)


@DTYPES
def test_kv_cache_replicated(dtype):
    c = filled_cache(dtype, 2, 1, 0, 37, 5)
    rep = c.replicated(3)
    assert rep.length == 37 and len(rep) == len(c) and rep.k[0].shape[0] == 6 and rep.smax == c.smax
    for (k, v), (rk, rv) in zip(c.to_legacy_cache(), rep.to_legacy_cache()):
        assert torch.equal(rk, k.repeat_interleave(3, 0)) and torch.equal(rv, v.repeat_interleave(3, 0))
    with pytest.raises(ValueError):
        c.gather_rows(torch.zeros(2, dtype=torch.int32, device=DEV), 5, 4)


# ---- generate(num_beams=K) on the tiny model ----------------------------------------------------------------------------------------------
def _model(dtype=BF):
    from test_logprobs_gpu import _model as tiny
    return tiny(dtype)


def _batch():
    """B = 2, L0 = 9, row 0 left-padded by 3."""
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, 90, (2, 9), generator=g)
    mask = torch.ones(2, 9, dtype=torch.int64)
    mask[0, :3] = 0
    ids[mask == 0] = 0
    return ids.to(DEV), mask.to(DEV)


NEW, PAD = 12, 99


def _no_cache_logits(m, mask, K):
    """logits_fn of the host rule: the model's own no-cache forward of the rows, through prepare_inputs_for_generation as generate() does."""
    def fn(rows):
        mk = mask if rows.shape[0] == mask.shape[0] else mask.repeat_interleave(K, 0)
        mk = torch.cat([mk, mk.new_ones(rows.shape[0], rows.shape[1] - mk.shape[1])], dim=1)
        with torch.no_grad():
            return m.forward(**m.prepare_inputs_for_generation(input_ids=rows, attention_mask=mk, images=None, videos=None, past_key_values=None,
                                                               use_cache=False)).logits[:, -1]
    return fn


class _Recorder:
    """wraps model.forward: the batch of every call and a copy of its last-position logits."""

    def __init__(self, m):
        self.m, self.inner, self.batches, self.logits = m, m.forward, [], []

    def __enter__(self):
        def forward(*a, **kw):
            out = self.inner(*a, **kw)
            self.batches.append(out.logits.shape[0])
            self.logits.append(out.logits[:, -1].clone())
            return out
        self.m.forward = forward
        return self

    def __exit__(self, *exc):
        del self.m.forward


@pytest.fixture(scope="module")
def eos_pair():
    """two EOS ids with which beam search ends early on this model and batch: tokens of the best hypotheses of a free 2-beam run, the
    first pair with which the host rule under early_stopping=True stops well before the last step for 2 and for 4 beams."""
    G = pkg("generation")
    m = _model()
    ids, mask = _batch()
    L0 = ids.shape[1]
    free = G.beam_search_reference(_no_cache_logits(m, mask, 2), ids, 2, NEW, [], PAD).sequences
    for j0, j1 in itertools.product(range(4), range(4)):
        eos = [int(free[0, L0 + j0]), int(free[1, L0 + j1])]
        if eos[0] != eos[1] and all(G.beam_search_reference(_no_cache_logits(m, mask, K), ids, K, NEW, eos, PAD, early_stopping=True).steps <= NEW - 3
                                    for K in (2, 4)):
            return eos
    raise AssertionError(f"no pair of EOS ids from the free run {free[:, L0:].tolist()} ends the search early")


@pytest.mark.parametrize("es", [False, True, "never"], ids=["es_false", "es_true", "es_never"])
@pytest.mark.parametrize("K", [2, 4])
def test_generate_without_cache_equals_the_host_rule(K, es, eos_pair):
    G = pkg("generation")
    m = _model()
    ids, mask = _batch()
    early = 0
    for lp, nret in itertools.product((0.0, 1.0, 2.0), (1, K)):
        want = G.beam_search_reference(_no_cache_logits(m, mask, K), ids, K, NEW, eos_pair, PAD, lp, es, nret, log_probs=row_logprobs)
        with _Recorder(m) as rec:
            got = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, num_beams=K, length_penalty=lp, early_stopping=es,
                             num_return_sequences=nret, eos_token_id=eos_pair, pad_token_id=PAD, use_cache=False, return_dict_in_generate=True)
        case = (K, es, lp, nret, want.steps)
        assert tuple(got.sequences.shape) == tuple(want.sequences.shape) and torch.equal(got.sequences.cpu(), want.sequences), case
        assert got.sequences_scores.dtype == F32 and torch.equal(bits(got.sequences_scores.cpu()), bits(want.sequences_scores)), case
        assert rec.batches[0] == 2 and all(b == 2 * K for b in rec.batches[1:]), rec.batches
        assert len(rec.batches) <= min(want.steps + 7, NEW), (case, len(rec.batches))
        early += want.steps < NEW
        plain = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, num_beams=K, length_penalty=lp, early_stopping=es,
                           num_return_sequences=nret, eos_token_id=eos_pair, pad_token_id=PAD, use_cache=False)
        assert torch.equal(plain, got.sequences)
    print(f"K {K} early_stopping {es}: {early} of 6 runs ended before {NEW} steps")
    if es is True:
        assert early >= 1


@pytest.mark.parametrize("K", [2, 4])
def test_generate_with_cache_replays_its_own_logits_and_gathers_the_cache(K, eos_pair):
    G = pkg("generation")
    m = _model()
    ids, mask = _batch()
    L0 = ids.shape[1]
    with _Recorder(m) as rec:
        got = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, num_beams=K, num_return_sequences=K, eos_token_id=[eos_pair[0]],
                         pad_token_id=PAD, use_cache=True, return_dict_in_generate=True)
    assert rec.batches[0] == 2 and all(b == 2 * K for b in rec.batches[1:])                # the prefill ran once per item
    steps = iter(rec.logits)
    stop = G.beam_search_reference(lambda rows: next(steps), ids, K, NEW, [eos_pair[0]], PAD, num_return_sequences=K, log_probs=row_logprobs).steps
    assert stop <= len(rec.logits) <= min(stop + 7, NEW)
    steps = iter(rec.logits)
    trace = []
    want = G.beam_search_reference(lambda rows: next(steps), ids, K, NEW, [eos_pair[0]], PAD, num_return_sequences=K, log_probs=row_logprobs,
                                   extra_steps=len(rec.logits) - stop, trace=trace)
    assert len(trace) == len(rec.logits)
    assert torch.equal(got.sequences.cpu(), want.sequences) and torch.equal(bits(got.sequences_scores.cpu()), bits(want.sequences_scores))
    # each step's logits against a fresh no-cache forward of the rule's running rows; where the step before reordered the rows, the row
    # the cache row held BEFORE the reorder (with the new token behind it) must miss the same bound: a wrong gather would show
    fresh = _no_cache_logits(m, mask, K)
    ident = torch.arange(2 * K, dtype=torch.int32)
    reordered = detected = 0
    for s in range(1, len(trace)):
        t, prev = trace[s], trace[s - 1]
        cur = t["cur"]
        rows = t["run_before"][:, :, :cur].reshape(2 * K, cur).to(DEV)
        e = rel_err(rec.logits[s], fresh(rows))
        assert e < 0.03, (s, e)
        moved = [r for r in range(2 * K) if int(prev["parent"][r]) != r]
        if s >= 2 and moved and not torch.equal(prev["parent"], ident):
            reordered += 1
            stale = prev["run_before"].reshape(2 * K, -1)[:, :cur].clone().to(DEV)       # what row r held before the reorder ...
            stale[:, cur - 1] = rows[:, cur - 1]                                         # ... and the token that was fed
            differs = [r for r in moved if not torch.equal(stale[r], rows[r])]
            if differs:
                wrong = fresh(stale)
                detected += max(rel_err(rec.logits[s][r], wrong[r]) for r in differs) > 0.03
    print(f"K {K}: {len(trace)} steps, {reordered} with a reorder of generated positions, {detected} where the stale row misses the bound")
    assert reordered >= 1 and detected >= 1


def test_generate_with_the_device_ngram_ban():
    G = pkg("generation")
    m = _model()
    ids = torch.tensor([[5, 6, 7, 5, 6, 7, 5, 6, 7, 5, 6], [9, 9, 9, 9, 8, 9, 9, 9, 9, 8, 9]], device=DEV)
    mask = torch.ones_like(ids)
    for cached in (False, True):
        with _Recorder(m) as rec:
            got = m.generate(input_ids=ids, max_new_tokens=8, num_beams=3, no_repeat_ngram_size=2, ngram_ban="device", eos_token_id=-1, pad_token_id=PAD,
                             use_cache=cached, return_dict_in_generate=True)
        steps = iter(rec.logits)
        trace = []
        want = G.beam_search_reference((lambda rows: next(steps)) if cached else _no_cache_logits(m, mask, 3), ids, 3, 8, [-1], PAD,
                                       no_repeat_ngram_size=2, log_probs=row_logprobs, trace=trace)
        assert torch.equal(got.sequences.cpu(), want.sequences) and torch.equal(bits(got.sequences_scores.cpu()), bits(want.sequences_scores))
        # some step banned what the best beam wanted most
        bit = sum(bool(torch.isneginf(t["lp"][b, 0, int(t["logits"].view(2, -1, t["lp"].shape[-1])[b, 0].float().argmax())])) for t in trace for b in range(2))
        assert bit >= 1
        free = m.generate(input_ids=ids, max_new_tokens=8, num_beams=3, eos_token_id=-1, pad_token_id=PAD, use_cache=cached)
        assert not torch.equal(free, got.sequences)


def test_one_beam_is_the_decoding_it_was(monkeypatch):
    G, core = pkg("generation"), pkg("modeling_core")
    m = _model()
    ids, mask = _batch()

    def never(*a, **kw):
        raise AssertionError("num_beams=1 reached the beam loop")
    monkeypatch.setattr(core, "beam_loop", never)
    ran = []
    fused = core.fused_loop
    monkeypatch.setattr(core, "fused_loop", lambda *a, **kw: ran.append(1) or fused(*a, **kw))
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=6, use_cache=True, return_dict_in_generate=True, output_logprobs=True)
    a = m.generate(**kw)
    b = m.generate(num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1, **kw)
    assert len(ran) == 2 and torch.equal(a.sequences, b.sequences) and torch.equal(a.logprobs, b.logprobs) and set(a) == set(b) == {"sequences", "hidden_states", "logprobs"}
