"""What the model-level batch calls of SLIM (rtrec_amd/models/slim.py) promise for the users a device pass does not serve, as
identities between the calls: explain_batch, rerank_batch, rank_items_batch, recommend_diverse_batch, recommend_blended_batch,
recommend_factor_batch, recommend_hybrid_batch and recommend_quality split a batch into regular users (a row of X), cold users
(nobody the model knows) and users outside the matrix (a negative integer id; an id known only through register_user_feature),
fill the lists of the latter two on the host, pad the outputs and map them back to raw ids.  No recorded outputs: every
expectation is another call of the same model (recommend_batch, recommend, the same call on one user alone) or the padding the
docstrings state.  Runs through the CPU stand-in; tests/test_gpu_api.py runs check_mix on the device."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_audience_host import AudienceOracleBackend
from tests.test_explain_host import ExplainOracleBackend
from tests.test_factor_host import FactorOracleBackend
from tests.test_ranks_host import RanksOracleBackend

N_USERS, N_ITEMS = 12, 24
TOP_K, POOL = 5, 8
WIDE = dict(top_k=30, pool=40)          # top_k beyond the catalogue: the lists come back narrower than top_k
KINDS = ("int", "str", "mixed")         # integer ids (SPARSE); string ids (DENSE); integer users with string items (DENSE)


class EveryCallBackend(RanksOracleBackend, ExplainOracleBackend, AudienceOracleBackend, FactorOracleBackend):
    """The CPU stand-ins of the request kernels in one backend (TEST-ONLY, like its bases)."""


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=EveryCallBackend())
    return m


def build_case(kind, make=cpu_slim):
    """A fitted 12 x 24 model of `kind` with vectors attached for every user but one, and what the checks need to know of it."""
    rng = np.random.default_rng(17)
    user = (lambda u: f"u{u:02d}") if kind == "str" else int
    item = (lambda i: f"i{i:02d}") if kind != "int" else int
    pairs = {(i % N_USERS, i) for i in range(N_ITEMS)} | {(N_USERS - 1, N_ITEMS - 1)}       # every user and every item is seen
    for u in range(N_USERS):
        pairs |= {(u, int(i)) for i in rng.choice(N_ITEMS, size=int(rng.integers(3, 7)), replace=False)}
    pairs = sorted(pairs)
    batch = [(user(u), item(i), 1.7e9 + p, float(rng.integers(1, 6))) for p, (u, i) in enumerate(pairs)]
    m = make(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    assert m.interactions.shape[0] == N_USERS and m.model.n_items_fitted == N_ITEMS
    users, items = [user(u) for u in range(N_USERS)], [item(i) for i in range(N_ITEMS)]
    no_vector = users[5]
    fu, fi = [u for u in users if u != no_vector], [i for i in items if i not in (items[2], items[20])]
    m.attach_factors(fu, rng.standard_normal((len(fu), 6)).astype(np.float32), fi, rng.standard_normal((len(fi), 6)).astype(np.float32))
    cold = ["nobody", "no one"] if kind == "str" else [40, 41]
    unknown_item = 10 ** 7 if kind == "int" else "never seen"
    if kind == "str":
        mixes = {"mix": [users[3], cold[0], users[5]]}
    else:       # -1 wraps to the last row of X, which is populated only if that user is in the batch
        mixes = {"mix with the last user": [3, cold[0], 3, N_USERS - 1, -1], "mix without the last user": [3, cold[0], 3, -1],
                 "odd alone": [-1]}
    mixes.update({name + " reversed": mix[::-1] for name, mix in list(mixes.items()) if len(mix) > 1})
    mixes.update({"regular alone": [users[3]], "cold alone": cold[:1], "all regular": [users[0], users[5], users[7], users[3]],
                  "all cold": cold, "empty": []})
    return types.SimpleNamespace(m=m, kind=kind, users=users, items=items, no_vector=no_vector, cold=cold, unknown_item=unknown_item,
                                 mixes=mixes, item_type=int if kind == "int" else str, user_type=str if kind == "str" else int,
                                 is_cold=lambda u: u in cold, is_regular=lambda u: u in users)


_CASES = {}


def case(kind):
    if kind not in _CASES:
        _CASES[kind] = build_case(kind)
    return _CASES[kind]


def brought(c, B, seed=5):
    """One list of raw item ids per user -- seven known items in a seeded order, an unknown one inside -- and descending scores."""
    rng = np.random.default_rng(seed)
    lists = []
    for _ in range(B):
        row = [c.items[j] for j in rng.permutation(N_ITEMS)[:7]]
        row.insert(3, c.unknown_item)
        lists.append(row)
    return lists, [[float(8 - p) for p in range(8)] for _ in range(B)]


def same(a, b):
    """== for the summaries, where a NaN equals a NaN."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def padded(n, ids, *others):
    """Everything behind counts[b] = n is -1 in `ids`; -inf in the float arrays and 0 in the integer arrays of `others`."""
    return (ids[n:] == -1).all() and all((np.isneginf(a[n:]) if a.dtype.kind == "f" else a[n:] == 0).all() for a in others)


def check_mix(c, users, top_k=TOP_K, pool=POOL):
    """Every identity of this file's docstring for one batch `users` of the case `c`."""
    from rtrec_amd.utils.metrics import gini
    m, B = c.m, len(users)
    get = m.item_ids.get
    reg, cold = [c.is_regular(u) for u in users], [c.is_cold(u) for u in users]
    plain = m.recommend_batch(list(users), top_k=top_k)
    cold_list = m.recommend_batch(c.cold[:1], top_k=top_k)[0]
    width = min(top_k, N_ITEMS)
    assert len(plain) == B and all(len(row) <= width for row in plain) and len(cold_list) > 0
    py = lambda rows, t: all(type(x) is t for row in rows for x in row)

    # ---- explain_batch(items=None): recommend_batch's lists; no reasons for a user without a row
    m_ = min(3, 32)
    got = m.explain_batch(users, top_k=top_k, top_m=m_)
    ids, cnt, r_ids, contrib, support = m.explain_batch(users, top_k=top_k, top_m=m_, as_arrays=True)
    assert ids.shape == support.shape == (B, top_k) and r_ids.shape == contrib.shape == (B, top_k, m_) and cnt.shape == (B,)
    assert [[i for i, _ in row] for row in got] == plain
    assert py([[i for i, _ in row] for row in got], c.item_type)
    assert py([[r for _, rs in row for r, _ in rs] for row in got], c.item_type) and py([[v for _, rs in row for _, v in rs] for row in got], float)
    for b in range(B):
        n = int(cnt[b])
        if reg[b]:
            assert got[b] == m.explain_batch([users[b]], top_k=top_k, top_m=m_)[0]
        else:
            assert all(reasons == [] for _, reasons in got[b]) and (support[b] == 0).all()
        assert [get(int(i)) for i in ids[b, :n]] == [i for i, _ in got[b]] and padded(n, ids[b], support[b])
        assert (r_ids[b, n:] == -1).all() and np.isneginf(contrib[b, n:]).all()
        for p, (_, reasons) in enumerate(got[b]):
            k = min(int(support[b, p]), m_)
            assert [(get(int(i)), float(v)) for i, v in zip(r_ids[b, p, :k], contrib[b, p, :k])] == reasons
            assert padded(k, r_ids[b, p], contrib[b, p])

    # ---- recommend_diverse_batch: recommend_batch's lists with scores 0.0 for a user without a row; diversity 0 for everybody
    got = m.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=0.6, ret_scores=True)
    ids, sc, cnt, val, pen = m.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=0.6, as_arrays=True)
    assert ids.shape == sc.shape == val.shape == pen.shape == (B, top_k) and cnt.shape == (B,)
    assert m.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=0.6) == [[i for i, _ in row] for row in got]
    assert m.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=0.0) == plain
    assert py([[i for i, _ in row] for row in got], c.item_type) and py([[s for _, s in row] for row in got], float)
    for b in range(B):
        n = int(cnt[b])
        if reg[b]:
            assert got[b] == m.recommend_diverse_batch([users[b]], top_k=top_k, pool=pool, diversity=0.6, ret_scores=True)[0]
        else:
            assert got[b] == [(i, 0.0) for i in plain[b]] and np.isneginf(val[b]).all() and np.isneginf(pen[b]).all()
        assert [(get(int(i)), float(s)) for i, s in zip(ids[b, :n], sc[b, :n])] == got[b] and padded(n, ids[b], sc[b], val[b], pen[b])

    # ---- recommend_quality: the measured lists are recommend_batch's (diversity 0) / recommend_diverse_batch's
    from rtrec_amd.utils import metrics
    seen, summarise = [], metrics.quality_summary
    metrics.quality_summary = lambda *a: (seen.append(np.asarray(a[4]).copy()), summarise(*a))[1]    # keeps the exposure it is given
    try:
        summary, frame = m.recommend_quality(users, top_k=top_k, per_user=True)
    finally:
        metrics.quality_summary = summarise
    assert same(m.recommend_quality(users, top_k=top_k), summary)
    assert frame["n"].tolist() == [len(row) for row in plain] and list(frame.index) == list(users)
    hist = np.bincount([m.item_ids.get_id(i) for row in plain for i in row], minlength=N_ITEMS)
    assert len(seen) == 1 and seen[0].tolist() == hist.tolist()          # the exposure IS the histogram of the lists
    assert summary["n_lists"] == B and summary["distinct_items"] == int(np.count_nonzero(hist))
    assert same(summary["gini"], gini(hist)) and same(summary["coverage"], np.count_nonzero(hist) / N_ITEMS)
    _, frame = m.recommend_quality(users, top_k=top_k, pool=pool, diversity=0.6, per_user=True)
    for b in range(B):
        if reg[b]:
            alone = m.recommend_quality([users[b]], top_k=top_k, pool=pool, diversity=0.6, per_user=True)[1]
            assert all(same(float(frame[col].iloc[b]), float(alone[col].iloc[0])) for col in frame.columns)
        else:
            assert frame["n"].iloc[b] == len(plain[b])

    # ---- recommend_factor_batch: the cold-start list, scores 0, for whoever has no row or no vector
    got = m.recommend_factor_batch(users, top_k=top_k)
    ids, sc, cnt = m.recommend_factor_batch(users, top_k=top_k, as_arrays=True)
    assert ids.shape == sc.shape == (B, top_k) and py(got, c.item_type)
    for b in range(B):
        n = int(cnt[b])
        if reg[b] and users[b] != c.no_vector:
            assert got[b] == m.recommend_factor_batch([users[b]], top_k=top_k)[0] and len(got[b]) > 0
        else:
            assert got[b] == cold_list and (sc[b, :n] == 0.0).all()
        assert [get(int(i)) for i in ids[b, :n]] == got[b] and padded(n, ids[b], sc[b])

    # ---- rerank_batch: a cold user gets recommend()'s answer for their own candidates, as recommend returns it
    cands, cand_scores = brought(c, B)
    got = m.rerank_batch(users, cands, top_k=top_k, ret_scores=True)
    ids, sc, cnt = m.rerank_batch(users, cands, top_k=top_k, as_arrays=True)
    assert ids.shape == sc.shape == (B, min(top_k, 7) if B else 0)
    assert m.rerank_batch(users, cands, top_k=top_k) == [[i for i, _ in row] for row in got]
    assert py([[s for _, s in row] for row in got], float)
    for b in range(B):
        n = int(cnt[b])
        if cold[b]:
            assert got[b] == [(i, 0.0) for i in m.recommend(users[b], candidate_items=cands[b], top_k=top_k)]
            assert ids[b, :n].tolist() == [i for i, _ in got[b]]            # (unmapped, as recommend leaves them)
        else:
            assert [get(int(i)) for i in ids[b, :n]] == [i for i, _ in got[b]] and py([[i for i, _ in got[b]]], c.item_type)
        if reg[b]:
            assert got[b] == m.rerank_batch([users[b]], [cands[b]], top_k=top_k, ret_scores=True)[0] and len(got[b]) == min(top_k, 7)
        assert [float(s) for s in sc[b, :n]] == [s for _, s in got[b]] and padded(n, ids[b], sc[b])

    # ---- rank_items_batch: nothing competes for a cold user
    got = m.rank_items_batch(users, cands)
    ptr, above, tied, score, competing = m.rank_items_batch(users, cands, as_arrays=True)
    assert ptr.tolist() == [8 * b for b in range(B + 1)] and competing.shape == (B,)
    for b in range(B):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        assert got[b] == {"items": cands[b], "above": above[lo:hi].tolist(), "tied": tied[lo:hi].tolist(), "score": score[lo:hi].tolist(),
                          "competing": int(competing[b])}
        assert type(got[b]["competing"]) is int and py([got[b]["above"], got[b]["tied"]], int) and py([got[b]["score"]], float)
        if cold[b]:
            assert got[b]["above"] == [-1] * 8 and got[b]["tied"] == [0] * 8 and got[b]["score"] == [-np.inf] * 8 and got[b]["competing"] == 0
        if reg[b]:
            assert got[b] == m.rank_items_batch([users[b]], [cands[b]])[0] and got[b]["competing"] > 0

    # ---- recommend_blended_batch: a user without a row has an empty SLIM side: the brought list alone
    got = m.recommend_blended_batch(users, cands, cand_scores, top_k=top_k, pool=pool, weighting=0.5)
    ids, val, src, cnt = m.recommend_blended_batch(users, cands, cand_scores, top_k=top_k, pool=pool, weighting=0.5, as_arrays=True)
    assert ids.shape == val.shape == src.shape == (B, top_k) and py(got, c.item_type)
    for b in range(B):
        n = int(cnt[b])
        if reg[b]:
            assert got[b] == m.recommend_blended_batch([users[b]], [cands[b]], [cand_scores[b]], top_k=top_k, pool=pool, weighting=0.5)[0]
        else:
            assert got[b] == [i for i in cands[b] if i != c.unknown_item][:top_k] and (src[b, :n] == 1).all()
        assert [get(int(i)) for i in ids[b, :n]] == got[b] and padded(n, ids[b], val[b], src[b]) and (src[b, :n] > 0).all()

    # ---- recommend_hybrid_batch: a user without a row has no side at all; one without a vector has SLIM's side alone
    got = m.recommend_hybrid_batch(users, top_k=top_k, pool=pool, weighting=0.5)
    ids, val, src, cnt = m.recommend_hybrid_batch(users, top_k=top_k, pool=pool, weighting=0.5, as_arrays=True)
    assert ids.shape == val.shape == src.shape == (B, top_k) and py(got, c.item_type)
    for b in range(B):
        n = int(cnt[b])
        if reg[b]:
            assert got[b] == m.recommend_hybrid_batch([users[b]], top_k=top_k, pool=pool, weighting=0.5)[0]
            if users[b] == c.no_vector:
                assert (src[b, :n] == 2).all() and set(got[b]) <= set(m.recommend_batch([users[b]], top_k=pool)[0]) and n > 0
        else:
            assert got[b] == [] and n == 0
        assert [get(int(i)) for i in ids[b, :n]] == got[b] and padded(n, ids[b], val[b], src[b])


@pytest.mark.parametrize("kind", KINDS)
def test_every_mix_of_regular_cold_and_odd_users(kind):
    c = case(kind)
    for name, users in c.mixes.items():
        check_mix(c, users)
    if kind != "str":      # the wrap-around is what recommend_batch does: the last user's list where they are in the batch, else none
        a = c.m.recommend_diverse_batch(c.mixes["mix with the last user"], top_k=TOP_K, pool=POOL)
        b = c.m.recommend_diverse_batch(c.mixes["mix without the last user"], top_k=TOP_K, pool=POOL)
        assert a[4] == c.m.recommend_batch([N_USERS - 1], top_k=TOP_K)[0] and len(a[4]) > 0
        # integer items: nothing stored, nothing listed; string items: an all-zero row ranks the highest internal ids first
        assert b[3] == ([] if kind == "int" else [c.m.item_ids.get(j) for j in range(N_ITEMS - 1, N_ITEMS - 1 - TOP_K, -1)])


@pytest.mark.parametrize("kind", KINDS)
def test_lists_narrower_than_top_k(kind):
    c = case(kind)
    mix = next(iter(c.mixes.values()))
    check_mix(c, mix, **WIDE)
    check_mix(c, [], **WIDE)
    ids, _, cnt, _, _ = c.m.recommend_diverse_batch(mix, as_arrays=True, **WIDE)
    assert ids.shape == (len(mix), 30) and cnt.max() <= N_ITEMS and (ids[:, N_ITEMS:] == -1).all()


def test_a_user_beyond_the_matrix_raises_index_error_from_every_call_that_lists_for_them():
    c = build_case("str")
    m = c.m
    m.register_user_feature("ghost", ["tag"])
    assert m._known_user_id("ghost") == N_USERS
    for users in (["ghost"], [c.users[3], "ghost"], ["nobody", "ghost", c.users[3]]):
        for call in (lambda: m.recommend_batch(users, top_k=TOP_K),
                     lambda: m.explain_batch(users, top_k=TOP_K),
                     lambda: m.recommend_diverse_batch(users, top_k=TOP_K, pool=POOL),
                     lambda: m.recommend_quality(users, top_k=TOP_K),
                     lambda: m.recommend_quality(users, top_k=TOP_K, pool=POOL, diversity=0.5)):
            with pytest.raises(IndexError) as e:
                call()
            assert str(e.value) == f"index ({N_USERS}) out of range"
    # the calls that serve such a user as one without a row still do
    lists, scores = brought(c, 2)
    assert m.explain_batch(["ghost"], items=[lists[0]]) == [[(i, []) for i in lists[0]]]
    assert m.recommend_factor_batch(["ghost"], top_k=TOP_K) == m.recommend_batch(["nobody"], top_k=TOP_K)
    assert m.recommend_hybrid_batch(["ghost"], top_k=TOP_K) == [[]]
    assert m.recommend_blended_batch(["ghost"], lists[:1], scores[:1], top_k=TOP_K, weighting=1.0) == [[i for i in lists[0] if i != c.unknown_item][:TOP_K]]
    assert m.rank_items_batch(["ghost"], lists[:1])[0]["competing"] > 0 and len(m.rerank_batch(["ghost"], lists[:1])[0]) == 7


@pytest.mark.parametrize("kind", ["int", "str"])
def test_explain_batch_with_brought_items_fills_nothing_and_returns_the_callers_values(kind):
    c = case(kind)
    m = c.m
    users = c.mixes["mix with the last user" if kind == "int" else "mix"]
    lists, _ = brought(c, len(users))
    got = m.explain_batch(users, items=lists, top_m=2)
    ids, cnt, r_ids, contrib, support = m.explain_batch(users, items=lists, top_m=2, as_arrays=True)
    assert [[i for i, _ in row] for row in got] == lists and cnt.tolist() == [8] * len(users) and ids.shape == (len(users), 8)
    for b, u in enumerate(users):
        assert ids[b].tolist() == [-1 if i == c.unknown_item else m.item_ids.get_id(i) for i in lists[b]]
        if c.is_regular(u):
            assert got[b] == m.explain_batch([u], items=[lists[b]], top_m=2)[0] and support[b].max() > 0
        else:
            assert all(reasons == [] for _, reasons in got[b]) and (support[b] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_the_list_tails_of_the_calls_without_users_hold_python_values(kind):
    c = case(kind)
    m = c.m
    a, sa = brought(c, 3, seed=1)
    b, sb = brought(c, 3, seed=2)
    got = m.blend_batch(a, sa, b, sb, top_k=6, weight=0.7)
    A, Bl = m._brought_lists("blend_batch", a, sa), m._brought_lists("blend_batch", b, sb, 3)
    ids, value, _, count = m.model.engine.blend_lists(A[0], A[1], Bl[0], Bl[1], A[2], Bl[2], keep=6, weight_b=0.7, mnz=False)
    assert got == [[(m.item_ids.get(int(i)), float(v)) for i, v in zip(ids[r, :count[r]], value[r, :count[r]])] for r in range(3)]
    assert all(type(i) is c.item_type and type(v) is float for row in got for i, v in row) and all(len(row) == 6 for row in got)
    assert m.blend_batch([], [], [], []) == []
    items = c.items[:4] + [c.unknown_item]
    pairs = m.recommend_users_batch(items, top_n=4, ret_scores=True)
    users, scores, counts, _ = m.recommend_users_batch(items, top_n=4, as_arrays=True)
    assert m.recommend_users_batch(items, top_n=4) == [[u for u, _ in row] for row in pairs] and pairs[-1] == [] and any(pairs)
    assert all(type(u) is c.user_type and type(s) is float for row in pairs for u, s in row)
    for r, row in enumerate(pairs):
        n = int(counts[r])
        assert [(m.user_ids.get(int(u)), float(s)) for u, s in zip(users[r, :n], scores[r, :n])] == row and padded(n, users[r], scores[r])


def test_arguments_wrong_in_two_ways_are_refused_for_the_first_reason():
    """Per call: arguments that are wrong in more than one way, and the one refusal they get (type and full text)."""
    fresh = cpu_slim()                                                  # not fitted, no vectors
    c = build_case("int")
    fitted = c.m
    bare = build_case("int").m.detach_factors()                         # fitted, no vectors
    two, one = [0, 1], [[1, 2]]
    R, V = RuntimeError, ValueError
    not_fitted = "Model must be fitted before calling {}."
    hybrid_range = ("recommend_hybrid_batch needs top_k >= 1 and 1 <= pool <= 128, got top_k=0 and pool=0: the factor kernel keeps each "
                    "user's candidates in LDS and selects at most 128 per user")
    weighting = '{}: weighting must be "contacts" or a non-negative number, got \'x\''
    tags = "{}: users_tags needs the per-feature tables of attach_feature_factors(): no factor model is attached"
    table = [
        (lambda: fresh.explain_batch(two, top_k=0), R, not_fitted.format("explain_batch")),
        (lambda: fresh.explain_batch(two, items=one), R, not_fitted.format("explain_batch")),
        (lambda: fitted.explain_batch(two, items=one, top_m=0), V, "items must hold one list per user: 1 lists for 2 users"),
        (lambda: fresh.rerank_batch(two, one), R, not_fitted.format("rerank_batch")),
        (lambda: fitted.rerank_batch(two, [list(range(2000))]), V, "candidates must hold one list per user: 1 lists for 2 users"),
        (lambda: fresh.rank_items_batch(two, one), R, not_fitted.format("rank_items_batch")),
        (lambda: fitted.rank_items_batch(two, one), V, "items must hold one list per user: 1 lists for 2 users"),
        (lambda: fresh.recommend_diverse_batch(two, top_k=0, diversity=2), V,
         "recommend_diverse_batch needs 1 <= top_k <= pool <= 1024, got top_k=0 and pool=50"),
        (lambda: fresh.recommend_diverse_batch(two, diversity=2), V, "recommend_diverse_batch: diversity must lie in [0, 1], got 2"),
        (lambda: fresh.recommend_diverse_batch([1, "x"]), R, not_fitted.format("recommend_diverse_batch")),
        (lambda: fresh.recommend_blended_batch(two, one, [[1.0]], top_k=0, weighting="x"), V,
         "recommend_blended_batch needs top_k >= 1 and 1 <= pool <= 1024, got top_k=0 and pool=0"),
        (lambda: fresh.recommend_blended_batch(two, one, [[1.0]], weighting="x", similarity_weight_factor=-1), V,
         weighting.format("recommend_blended_batch")),
        (lambda: fresh.recommend_blended_batch(two, one, [[1.0]], similarity_weight_factor=-1), V,
         "recommend_blended_batch: similarity_weight_factor must not be negative or NaN, got -1"),
        (lambda: fresh.recommend_blended_batch(two, one, [[1.0]]), R, not_fitted.format("recommend_blended_batch")),
        (lambda: fitted.recommend_blended_batch(two, one, [[1.0, 2.0]], pool=1024), V,
         "recommend_blended_batch: one list of items is needed per user, got 1 for 2 users"),
        (lambda: fresh.recommend_factor_batch(two, top_k=0, users_tags=[["t"], ["t"]]), V,
         "recommend_factor_batch needs 1 <= top_k <= 128 (what the factor kernel selects), got 0"),
        (lambda: fresh.recommend_factor_batch(two, users_tags=[["t"], ["t"]]), V, tags.format("recommend_factor_batch")),
        (lambda: fresh.recommend_factor_batch(two), R, not_fitted.format("recommend_factor_batch")),
        (lambda: bare.recommend_factor_batch([1, "x"]), R, "attach_factors() must be called before recommend_factor_batch."),
        (lambda: fresh.recommend_hybrid_batch(two, top_k=0, weighting="x"), V, hybrid_range),
        (lambda: fresh.recommend_hybrid_batch(two, weighting="x", similarity_weight_factor=-1), V, weighting.format("recommend_hybrid_batch")),
        (lambda: fresh.recommend_hybrid_batch(two, similarity_weight_factor=float("nan"), users_tags=[["t"], ["t"]]), V,
         "recommend_hybrid_batch: similarity_weight_factor must not be negative or NaN, got nan"),
        (lambda: fresh.recommend_hybrid_batch(two, users_tags=[["t"], ["t"]]), V, tags.format("recommend_hybrid_batch")),
        (lambda: fresh.recommend_hybrid_batch(two), R, not_fitted.format("recommend_hybrid_batch")),
        (lambda: bare.recommend_hybrid_batch(two, pool=128), R, "attach_factors() must be called before recommend_hybrid_batch."),
        (lambda: fresh.recommend_quality(two, top_k=0), V, "recommend_quality needs 1 <= top_k <= 1024, got top_k=0"),
        (lambda: fresh.recommend_quality(two), R, not_fitted.format("recommend_quality")),
        (lambda: fresh.recommend_quality(two, top_k=0, diversity=2), V, "recommend_quality needs 1 <= top_k <= pool <= 1024, got top_k=0 and pool=50"),
        (lambda: fresh.recommend_quality(two, diversity=2), V, "recommend_quality: diversity must lie in [0, 1], got 2"),
        (lambda: fresh.recommend_quality(two, diversity=0.5), R, not_fitted.format("recommend_quality")),
    ]
    for n, (call, exc, text) in enumerate(table):
        with pytest.raises(exc) as e:
            call()
        assert type(e.value) is exc and str(e.value) == text, (n, str(e.value))
    # an empty batch asks nothing of W -- except in recommend_quality, which checks W and the pool whatever the batch holds
    lossy = sp.csc_matrix(fitted.model.item_similarity, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    W, fitted.model.item_similarity = fitted.model.item_similarity, lossy
    try:
        assert fitted.explain_batch([]) == fitted.rerank_batch([], []) == fitted.recommend_diverse_batch([]) == []
        assert fitted.recommend_blended_batch([], [], []) == fitted.recommend_hybrid_batch([]) == fitted.recommend_factor_batch([]) == []
        for call in (lambda: fitted.recommend_quality([]), lambda: fitted.recommend_diverse_batch([0]), lambda: fitted.explain_batch([40])):
            with pytest.raises(ValueError, match="not float32 numbers"):
                call()
    finally:
        fitted.model.item_similarity = W
