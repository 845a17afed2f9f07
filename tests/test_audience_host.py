"""The audience of an item (SLIM.recommend_users_batch, csrc/audience.hip) without a GPU: the definition as a numpy host model,
pinned to the reference's scores on the golden fixture; the model / facade / serving layers end to end through the CPU stand-in
backend with `audience_topk` supplied by the host model; the registration of the op and the C entry point's host-side checks.
The kernel itself is in tests/test_gpu_audience.py.

The definition (include/rtrec_amd.h, "AUDIENCE OF AN ITEM"): score(u, i) is the float32 sum of fl32(x_uj * w_ji) over the j stored
in both row u of X and column i of W, added from 0.0f in ascending j; eligible are the users with at least one such j, not stored
in column i of X (filter_interacted), inside the candidate set; the audience is the top_n of them by score descending, the lower
user row first among equal scores.  A user whose score is NaN counts in eligible and is never listed; +-inf are numbers.  The
value-edge cases (`edge_case`) and the mutated models that show they bite follow the definition's tests;
tests/test_gpu_audience.py runs the same cases on the kernels."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.cpu_backend import OracleBackend
from tests.test_explain_host import INF, NNAN, PNAN, bits, golden, ordered_sum, p2, pair_contributions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------------------------------------- the host model
def accumulate(Xc: sp.csc_matrix, W: sp.csc_matrix, i: int):
    """(acc float32[U], touched bool[U]) of query item i: W's column applied to X's columns in ascending j."""
    acc, touched = np.zeros(Xc.shape[0], np.float32), np.zeros(Xc.shape[0], bool)
    for p in range(W.indptr[i], W.indptr[i + 1]):
        j, w = int(W.indices[p]), np.float32(W.data[p])
        s, e = Xc.indptr[j], Xc.indptr[j + 1]
        r = Xc.indices[s:e]
        with np.errstate(all="ignore"):                                  # inf * 0, inf - inf, underflow: the values under test
            acc[r] = acc[r] + Xc.data[s:e].astype(np.float32) * w        # one rounded multiply, one rounded add
        touched[r] = True
    return acc, touched


def host_model(Xc, W, items, top_n, filter_interacted=True, candidates=None):
    """THE DEFINITION: (users[n, top_n] int32, scores[n, top_n] float32, count[n], eligible[n]), -1 / -inf padded.  Xc / W are
    CSC with sorted indices; `candidates` a bool array over the user rows or None; an item outside [0, n_items) is empty.  A
    user whose score is NaN counts in eligible (support is structural) and is never listed: count = min(top_n, the eligible
    users whose score is a number); +-inf are numbers."""
    n, rows = len(items), np.arange(Xc.shape[0])
    users, scores = np.full((n, top_n), -1, np.int32), np.full((n, top_n), -np.inf, np.float32)
    count, eligible = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for b, i in enumerate(int(x) for x in items):
        if not 0 <= i < W.shape[1]:
            continue
        acc, ok = accumulate(Xc, W, i)
        if filter_interacted:
            ok[Xc.indices[Xc.indptr[i]:Xc.indptr[i + 1]]] = False
        if candidates is not None:
            ok &= candidates
        el = rows[ok]
        eligible[b] = len(el)                                            # NaN scores included
        el = el[~np.isnan(acc[el])]
        order = el[np.lexsort((el, -acc[el]))][:top_n]                   # score descending, then the lower user row
        count[b] = len(order)
        users[b, :len(order)], scores[b, :len(order)] = order, acc[order]
    return users, scores, count, eligible


def golden_csc():
    X, W, users, ids, scores = golden()
    Xc = X.tocsc()
    Xc.sort_indices()
    return X, Xc, W, users, ids, scores


class AudienceOracleBackend(OracleBackend):
    """The CPU stand-in plus audience_topk from the host model (TEST-ONLY, like its base)."""

    def audience_topk(self, items, n_users, X, W, top_n, filter_interacted, user_mask, users, scores, count, eligible):
        import torch
        n_items = W["cptr"].numel() - 1
        Xc = sp.csc_matrix((X[2].numpy(), X[1].numpy(), X[0].numpy()), shape=(n_users, n_items))
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        cand = None
        if user_mask is not None:
            cand = np.unpackbits(user_mask.numpy().view(np.uint8), bitorder="little")[:n_users].astype(bool)
        out = host_model(Xc, Wc, items.numpy(), top_n, filter_interacted, cand)
        for dst, src in zip((users, scores, count, eligible), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=AudienceOracleBackend())
    return m


# ---------------------------------------------------------------------------------------------- the definition
def test_accumulators_reproduce_every_reference_score_bit_for_bit():
    """All 2,400 (user, item, score) triples of the fixture generated from the real reference: the accumulator of the item's
    walk holds the reference's score for the user, and the user is touched."""
    _, Xc, W, users, ids, scores = golden_csc()
    assert ids.shape == (240, 10) and (ids >= 0).all()
    distinct = np.unique(ids)
    assert len(distinct) == 145
    acc_of = {int(i): accumulate(Xc, W, int(i)) for i in distinct}
    n = 0
    for b, u in enumerate(users.tolist()):
        for p in range(10):
            acc, touched = acc_of[int(ids[b, p])]
            assert touched[u] and bits(acc[u]) == bits(np.float32(scores[b, p])), (u, p)
            n += 1
    assert n == 2400


def test_accumulator_model_is_the_per_pair_definition():
    """A sample of golden pairs, and of pairs the reference never listed: the accumulator equals the ordered float32 sum of
    the pair's contributions (explain's invariant read the other way round), touched equals support >= 1."""
    X, Xc, W, users, ids, _ = golden_csc()
    rng = np.random.default_rng(7)
    pairs = [(int(users[b]), int(ids[b, p])) for b, p in zip(rng.integers(0, 240, 150), rng.integers(0, 10, 150))]
    pairs += [(int(u), int(i)) for u, i in zip(rng.integers(0, X.shape[0], 150), rng.integers(0, W.shape[1], 150))]
    hit = 0
    for u, i in pairs:
        acc, touched = accumulate(Xc, W, i)
        j, c = pair_contributions(X, W, u, i)
        assert touched[u] == (len(j) >= 1)
        assert bits(acc[u]) == bits(ordered_sum(c)), (u, i)
        hit += len(j) >= 1
    assert hit >= 150


def test_tie_rule_lower_user_row_first_zero_and_negative_scores_take_part():
    # items 0..3; the query is item 3, W[:, 3] = {0: 1.0, 1: -1.0, 2: 0.5}
    X = sp.csr_matrix(np.array([[2, 0, 0, 0],       # 2.0
                                [0, 0, 4, 0],       # 2.0: ties with user 0, the lower row first
                                [1, 1, 0, 0],       # exactly 0 with support 2: eligible
                                [0, 3, 0, 0],       # -3.0: negative, eligible
                                [2, 0, 0, 5],       # 2.0 but interacted with item 3: removed by the filter
                                [0, 0, 0, 1],       # no support (and interacted)
                                [0, 0, 0, 0],       # no support
                                [0, 0, 4, 0]],      # 2.0: the third of the tie
                               dtype=np.float32))
    W = sp.csc_matrix(np.array([[0, 0, 0, 1.0], [0, 0, 0, -1.0], [0, 0, 0, 0.5], [0, 0, 0, 0]], dtype=np.float32))
    Xc = X.tocsc()
    users, scores, count, eligible = host_model(Xc, W, [3], 8)
    assert users[0].tolist() == [0, 1, 7, 2, 3, -1, -1, -1] and count[0] == 5 and eligible[0] == 5
    assert scores[0].tolist() == [2.0, 2.0, 2.0, 0.0, -3.0, -np.inf, -np.inf, -np.inf]
    users, scores, count, eligible = host_model(Xc, W, [3], 2)            # the boundary cuts the tie: rows 0 and 1
    assert users[0].tolist() == [0, 1] and count[0] == 2 and eligible[0] == 5
    users, _, count, eligible = host_model(Xc, W, [3], 8, filter_interacted=False)
    assert users[0].tolist() == [0, 1, 4, 7, 2, 3, -1, -1] and eligible[0] == 6
    cand = np.array([0, 0, 1, 1, 1, 1, 1, 1], bool)
    users, _, count, eligible = host_model(Xc, W, [3, 0, -1, 4], 3, candidates=cand)
    assert users.tolist() == [[7, 2, 3], [-1] * 3, [-1] * 3, [-1] * 3] and count.tolist() == [3, 0, 0, 0] and eligible.tolist() == [3, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the value edges: the cases
E = "E"                # a row token: ("E", d) is row edge + d, edge = the last row of the first tile when there are two tiles
o = None                # not stored
D = p2(-100)           # times the weight 2^-40: the denormal 2^-140

# name -> (the three weights of the query column's active entries in ascending item id,
#          {user row: its three ratings on those items}, the rows that interacted with the query item itself).
# Every 0.0 below is a STORED zero.
SCORE_SETS = {
    "nan_rating": ((1, 1, 1), {1: (2, o, o), 2: (PNAN, 1, o), 3: (1, o, o), 4: (NNAN, o, 1), 5: (3, o, o), 6: (o, o, NNAN), 7: (1, PNAN, 1),
                               (E, -1): (5, o, o), (E, 0): (PNAN, o, o), (E, 1): (5, o, o), (E, 2): (o, NNAN, o)}, {2, (E, 0)}),
    "inf_minus_inf": ((1, -1, 1), {2: (INF, INF, 7), 4: (INF, o, 7), 6: (o, INF, 7), 8: (1, 1, 1), 9: (2, o, o), 10: (-3, o, o),
                                   (E, -2): (INF, INF, 1), (E, -1): (o, INF, o), (E, 0): (INF, o, o), (E, 1): (INF, o, 1), (E, 2): (o, INF, 3),
                                   (E, 3): (INF, INF, o)}, {2}),
    "inf_times_zero": ((0.0, 1, 2), {1: (INF, 1, o), 2: (-INF, o, 1), 3: (5, 1, o), 4: (o, 2, o), 5: (o, o, -1), (E, 0): (INF, o, o),
                                     (E, 1): (7, o, o)}, {1}),
    "zero_times_inf": ((INF, 1, 1), {1: (0.0, 1, o), 2: (1, o, o), 3: (-1, o, o), 4: (o, 1, 1), (E, 0): (0.0, o, o), (E, 1): (2, o, o)}, set()),
    # 11 eligible, 3 of them numbers: with top_n = 5 there is no fifth key to find
    "few_numbers": ((1, 1, 1), {1: (PNAN, o, o), 2: (NNAN, o, o), 3: (PNAN, 1, o), 4: (o, NNAN, o), 5: (1, o, PNAN), 6: (1, o, o), 7: (NNAN, o, o),
                                8: (PNAN, o, o), (E, 0): (2, o, o), (E, 1): (2, o, o), (E, 2): (PNAN, o, o)}, {7}),
    "all_nan": ((1, NNAN, 1), {3: (o, 1, o), 5: (1, 1, 1), (E, 0): (o, 2, o), (E, 1): (o, 1, o)}, set()),
    # -1 * 0 = -0.0 alone in its sum: 0 + -0 = +0.0, tying with 1 - 1 and with 1 * 0
    "signed_zero": ((0.0, 1, -1), {2: (o, 2, o), 3: (o, 1, 1), 5: (-1, o, o), 7: (1, o, o), 9: (o, o, 2), (E, 0): (-2, o, o), (E, 1): (o, 3, 3)}, set()),
    # the zero-score users sit on lower rows than the positive denormal and on higher rows than the negative one
    "denormals": ((p2(-40), p2(-40), 1), {1: (o, o, 0.0), 2: (o, o, 0.0), 3: (D, D, o), 4: (D, o, o), 6: (-D, o, o), 7: (-D, -D, o), 8: (o, o, 0.0),
                                          (E, -1): (o, o, 0.0), (E, 0): (D, o, o), (E, 1): (D, o, o), (E, 2): (-D, o, 0.0)}, set()),
}
# the users the definition lists, whole (top_n = 1024), per set: e = edge
EXPECTED_USERS = {
    "nan_rating": lambda e: [e - 1, e + 1, 5, 1, 3], "inf_minus_inf": lambda e: [4, e, e + 1, 9, 8, 10, 6, e - 1, e + 2],
    "inf_times_zero": lambda e: [4, 3, e + 1, 5], "zero_times_inf": lambda e: [2, e + 1, 4, 3], "few_numbers": lambda e: [e, e + 1, 6],
    "all_nan": lambda e: [], "signed_zero": lambda e: [2, 3, 5, 7, e, e + 1, 9], "denormals": lambda e: [3, 4, e, e + 1, 1, 2, 8, e - 1, 6, e + 2, 7],
}
EDGE_TOP_N = (1, 5, 1024)
MANY_NANS = (100, 1130)           # the rows of the "many_nans" item: 1,030 NaN scores in one tile (as many as there are users)


def edge_case(two_tiles):
    """(Xc csc, W csc, query items, mask, cases) from raw (data, indices, indptr) arrays, so that stored zeros survive: 300 users
    (one tile) or 8,192 + 300 (two; the edge rows 8,191 and 8,192 then carry the tied and the NaN scores, so the merge kernel
    sees them from different tiles).  Every score set is asked about twice: through a column of W of its 3 active entries, and
    through one of 60 entries -- 55 fillers, a stored-zero product of every user of the set at position 55 (the last of the
    first round of 56 columns), one more filler, the active entries at positions 57..59: the accumulator crosses a round and
    arrives as +0.0, so both columns give the set's users the same scores.  Rows 60..89 rate the fillers only.  "many_nans" has
    more NaN users than top_n = 1024 can be (in the two-tile matrix) beside ten numbers.  mask: a candidate set that leaves out
    NaN users, numbers and the edge row.  cases[name] = (query item with 3 entries, with 60, the set's expected users)."""
    U = 8192 + 300 if two_tiles else 300
    edge = 8191 if two_tiles else 255
    row = lambda t: t if isinstance(t, int) else edge + t[1]
    sets = dict(SCORE_SETS)
    nan_rows = range(MANY_NANS[0], min(MANY_NANS[1], U))
    sets["many_nans"] = ((1, 1, 1), {**{r: ((PNAN, NNAN)[r & 1], o, o) for r in nan_rows}, **{20 + k: (k - 4, o, o) for k in range(10)}}, set())
    n_fill, S = 56, len(sets)
    first_gate, second_filler, first_active, first_query = 55, 55 + S, 56 + S, 56 + 4 * S
    I = first_query + 2 * S
    cols = {j: {} for j in range(I)}                                      # X by column: {row: value}
    rng = np.random.default_rng(23)
    for j in list(range(55)) + [second_filler]:
        for r in rng.choice(np.arange(60, 90), 6, replace=False):
            cols[j][int(r)] = np.float32(rng.integers(-4, 5))
    wcols, items, cases = {}, [], {}
    for s, (name, (w, users, interacted)) in enumerate(sets.items()):
        gate, act = first_gate + s, [first_active + 3 * s + t for t in range(3)]
        q3, q60 = first_query + 2 * s, first_query + 2 * s + 1
        for t, x in users.items():
            cols[gate][row(t)] = np.float32(0.0)
            for a, v in zip(act, x):
                if v is not None:
                    cols[a][row(t)] = np.float32(v)
        for t in interacted:
            cols[q3][row(t)] = cols[q60][row(t)] = np.float32(1.0)
        wcols[q3] = [(a, np.float32(v)) for a, v in zip(act, w)]
        wcols[q60] = [(j, np.float32(1 + j % 3)) for j in range(55)] + [(gate, np.float32(1.0)), (second_filler, np.float32(-2.0))] + wcols[q3]
        assert len(wcols[q60]) == 60 and [j for j, _ in wcols[q60]] == sorted(j for j, _ in wcols[q60])
        items += [q3, q60]
        want = (lambda e: list(range(29, 19, -1))) if name == "many_nans" else EXPECTED_USERS[name]
        cases[name] = (q3, q60, want(edge))
    xptr = np.zeros(I + 1, np.int64)
    xptr[1:] = np.cumsum([len(cols[j]) for j in range(I)])
    xrow = np.array([r for j in range(I) for r in sorted(cols[j])], np.int32)
    xval = np.array([cols[j][r] for j in range(I) for r in sorted(cols[j])], np.float32)
    Xc = sp.csc_matrix((xval, xrow, xptr.astype(np.int32)), shape=(U, I))
    wptr = np.zeros(I + 1, np.int64)
    wptr[1:] = np.cumsum([len(wcols.get(j, ())) for j in range(I)])
    W = sp.csc_matrix((np.array([v for j in range(I) for _, v in wcols.get(j, ())], np.float32),
                       np.array([i for j in range(I) for i, _ in wcols.get(j, ())], np.int32), wptr.astype(np.int32)), shape=(I, I))
    assert Xc.nnz == len(xval) and W.nnz == 63 * S and Xc.has_sorted_indices and W.has_sorted_indices      # no zero was dropped
    mask = np.ones(U, bool)
    mask[[2, 4, 5, edge, 101, 22]] = False
    return Xc, W, np.array(items, np.int32), mask, cases


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("two_tiles", [False, True])
def test_edge_cases_give_the_expected_audiences_under_the_definition(two_tiles):
    Xc, W, items, mask, cases = edge_case(two_tiles)
    X = Xc.tocsr()                                                       # (scipy keeps the stored zeros)
    assert X.nnz == Xc.nnz and np.isnan(Xc.data).any() and np.isinf(Xc.data).any() and (Xc.data == 0).any() and (W.data == 0).any()
    users, scores, count, eligible = host_model(Xc, W, items, 1024, filter_interacted=False)
    assert not np.isnan(scores).any()                                    # under the rule no output holds a NaN
    edge = 8191 if two_tiles else 255
    for name, (q3, q60, want) in cases.items():
        a, b = int(np.flatnonzero(items == q3)[0]), int(np.flatnonzero(items == q60)[0])
        assert users[a, :count[a]].tolist() == want and (users[a, count[a]:] == -1).all(), name
        n_set = eligible[a]
        assert eligible[b] == n_set + 30 and count[b] == count[a] + 30    # the 60-entry column adds the 30 filler users ...
        of_set = ~np.isin(users[b, :count[b]], np.arange(60, 90))
        assert users[b, :count[b]][of_set].tolist() == want, name         # ... and gives the set's users the same order and scores
        assert np.array_equal(bits(scores[b, :count[b]][of_set]), bits(scores[a, :count[a]]))
    q = lambda name: int(np.flatnonzero(items == cases[name][0])[0])
    assert (eligible[q("few_numbers")], count[q("few_numbers")]) == (11, 3) and (eligible[q("all_nan")], count[q("all_nan")]) == (4, 0)
    n_nan = min(MANY_NANS[1], Xc.shape[0]) - MANY_NANS[0]
    assert (eligible[q("many_nans")], count[q("many_nans")]) == (n_nan + 10, 10) and (n_nan > 1024) == two_tiles
    assert bits(scores[q("signed_zero"), 1:6]).tolist() == [0] * 5        # -0.0 alone, 1 - 1 and 1 * 0: all +0.0
    assert bits(scores[q("denormals"), :11]).tolist() == [0x400, 0x200, 0x200, 0x200, 0, 0, 0, 0, 0x80000200, 0x80000200, 0x80000400]
    assert scores[q("inf_minus_inf"), :9].tolist() == [np.inf] * 3 + [2, 1, -3] + [-np.inf] * 3
    # the accumulator model is the per-pair definition on these values too: the ordered float32 sum of the pair's products
    for name, (q3, q60, _) in cases.items():
        for item in (q3, q60):
            acc, touched = accumulate(Xc, W, item)
            for u in np.flatnonzero(touched)[:40]:
                j, c = pair_contributions(X, W, int(u), item)
                with np.errstate(all="ignore"):
                    s = ordered_sum(c)
                assert len(j) >= 1 and (np.isnan(s) and np.isnan(acc[u]) or bits(s) == bits(acc[u])), (name, item, u)
    # the filter, the candidate set and top_n change what they should
    f = host_model(Xc, W, items, 5)
    m = host_model(Xc, W, items, 5, False, mask)
    assert f[3][q("nan_rating")] == eligible[q("nan_rating")] - 2 and f[3][q("few_numbers")] == 10 and f[2][q("few_numbers")] == 3
    assert m[3][q("nan_rating")] == eligible[q("nan_rating")] - 4 and m[0][q("nan_rating"), :3].tolist() == [edge - 1, edge + 1, 1]


def test_existing_fixtures_hold_no_nan_and_keep_their_answers_under_the_rule():
    _, Xc, W, _, _, _ = golden_csc()
    assert np.isfinite(Xc.data).all() and np.isfinite(W.data).all()
    old = mutant_model(Xc, W, np.arange(W.shape[1]), 1024, "nan_listed_last")       # the definition before the rule
    assert same(old, host_model(Xc, W, np.arange(W.shape[1]), 1024))


# ---------------------------------------------------------------------------------------------- mutated models: the cases bite
DEFECTS = ("nan_listed_last", "nan_by_sign_bit", "denormals_flushed", "ties_to_the_higher_row", "nan_dropped_from_eligible")


def _flush(v):
    return np.where(np.abs(v) < p2(-126), np.copysign(np.float32(0), v), v).astype(np.float32)


def mutant_model(Xc, W, items, top_n, defect, filter_interacted=True, candidates=None):
    """host_model with one defect built in."""
    assert defect in DEFECTS
    n, rows = len(items), np.arange(Xc.shape[0])
    users, scores = np.full((n, top_n), -1, np.int32), np.full((n, top_n), -np.inf, np.float32)
    count, eligible = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for b, i in enumerate(int(x) for x in items):
        if not 0 <= i < W.shape[1]:
            continue
        if defect == "denormals_flushed":                                # every product and every sum
            acc, ok = np.zeros(Xc.shape[0], np.float32), np.zeros(Xc.shape[0], bool)
            for p in range(W.indptr[i], W.indptr[i + 1]):
                j, w = int(W.indices[p]), np.float32(W.data[p])
                r = Xc.indices[Xc.indptr[j]:Xc.indptr[j + 1]]
                with np.errstate(all="ignore"):
                    acc[r] = _flush(acc[r] + _flush(Xc.data[Xc.indptr[j]:Xc.indptr[j + 1]].astype(np.float32) * w))
                ok[r] = True
        else:
            acc, ok = accumulate(Xc, W, i)
        if filter_interacted:
            ok[Xc.indices[Xc.indptr[i]:Xc.indptr[i + 1]]] = False
        if candidates is not None:
            ok &= candidates
        el = rows[ok]
        eligible[b] = len(el)
        if defect == "nan_dropped_from_eligible":
            eligible[b] = int((~np.isnan(acc[el])).sum())
        if defect == "nan_by_sign_bit":                                  # the kernel's key before the rule: the raw bits, order-preserving
            u = bits(acc[el]).astype(np.int64)
            u[u == 0x80000000] = 0
            order = el[np.lexsort((el, -np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000)))][:top_n]
        else:
            if defect != "nan_listed_last":
                el = el[~np.isnan(acc[el])]
            order = el[np.lexsort((-el if defect == "ties_to_the_higher_row" else el, -acc[el]))][:top_n]
        count[b] = len(order)
        users[b, :len(order)], scores[b, :len(order)] = order, acc[order]
    return users, scores, count, eligible


# defect -> (a score set, its 3- or 60-entry column, the matrix) that must tell it from the definition
CAUGHT_BY = {
    "nan_listed_last": ("few_numbers", 3, False), "nan_by_sign_bit": ("nan_rating", 60, True), "denormals_flushed": ("denormals", 60, False),
    "ties_to_the_higher_row": ("inf_minus_inf", 3, True), "nan_dropped_from_eligible": ("all_nan", 3, True),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_told_from_the_definition_by_a_named_case(defect):
    name, length, two_tiles = CAUGHT_BY[defect]
    Xc, W, items, mask, cases = edge_case(two_tiles)
    seen = set()
    for top_n in EDGE_TOP_N:
        want, got = host_model(Xc, W, items, top_n), mutant_model(Xc, W, items, top_n, defect)
        for set_name, (q3, q60, _) in cases.items():
            for L, item in ((3, q3), (60, q60)):
                b = int(np.flatnonzero(items == item)[0])
                if not same(tuple(a[b:b + 1] for a in want), tuple(a[b:b + 1] for a in got)):
                    seen.add((set_name, L, top_n))
    print(f"{defect}: seen by {sorted(seen)}")
    assert any(s[:2] == (name, length) for s in seen)
    if defect == "ties_to_the_higher_row":                               # the tie that straddles the two tiles decides top_n = 5
        assert ("inf_minus_inf", 3, 5) in seen


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _batch(strings=False):
    z = np.load(os.path.join(G, "partial_fit.npz"))
    a, b = z["A"][0], z["C"][1]
    if strings:
        return [(f"u{x}", f"i{y}", float(t), float(r)) for x, y, t, r in zip(z["u"][a:b], z["i"][a:b], z["ts"][a:b], z["v"][a:b])]
    return [(int(x), int(y), float(t), float(r)) for x, y, t, r in zip(z["u"][a:b], z["i"][a:b], z["ts"][a:b], z["v"][a:b])]


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    return m, batch


def _want(m, items, top_n, filter_interacted=True, candidates=None):
    """The host model on the model's own X and W for internal item ids."""
    Xc, W = m.interactions.to_csc(), m.model.item_similarity.tocsc()
    Xc.sort_indices(); W.sort_indices()
    Xc.resize((Xc.shape[0], max(Xc.shape[1], W.shape[1])))
    return host_model(Xc, W, items, top_n, filter_interacted, candidates)


def test_recommend_users_batch_integer_ids():
    from rtrec_amd.recommender import Recommender
    m, batch = _model()
    items = sorted({i for _, i, _, _ in batch})
    query = items[:30] + [items[3], 10 ** 7, "no such item", items[3]]     # duplicates, an unknown id, an id of the other kind
    q = [i if isinstance(i, int) and i < 10 ** 7 else -1 for i in query]
    want = _want(m, q, 7)
    got = m.recommend_users_batch(query, top_n=7, as_arrays=True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
    assert want[3].max() > 7 and (want[2] > 0).sum() >= 20 and want[2][-3:].tolist() == [0, 0, int(want[2][3])]
    lists = m.recommend_users_batch(query, top_n=7)
    pairs = m.recommend_users_batch(query, top_n=7, ret_scores=True)
    for b in range(len(query)):
        c = int(want[2][b])
        assert lists[b] == want[0][b, :c].tolist() and [u for u, _ in pairs[b]] == lists[b]
        assert all(isinstance(s, float) for _, s in pairs[b]) and np.array_equal(bits([s for _, s in pairs[b]]), bits(want[1][b, :c]))
    assert lists[-2] == [] and lists[-3] == [] and lists[-1] == lists[3] and lists[3]
    assert m.recommend_users(query[0], top_n=7) == lists[0] and m.recommend_users(query[0], top_n=7, ret_scores=True) == pairs[0]
    # filter_interacted: nobody listed has the item with it, somebody has without it
    X = m.interactions.to_csr()
    assert all(X[u, i] == 0 for i, row in zip(query[:30], lists) for u in row)
    nof = m.recommend_users_batch(query[:30], top_n=7, filter_interacted=False, as_arrays=True)
    w2 = _want(m, q[:30], 7, filter_interacted=False)
    assert np.array_equal(nof[0], w2[0]) and np.array_equal(bits(nof[1]), bits(w2[1])) and np.array_equal(nof[3], w2[3])
    assert (nof[3] >= got[3][:30]).all() and (nof[3] > got[3][:30]).any()
    assert any(X[u, i] != 0 for i, row, c in zip(query[:30], nof[0], nof[2]) for u in row[:c])
    # candidate users: raw ids, unknown ones ignored, an empty list leaves nobody
    all_users = sorted({u for u, _, _, _ in batch})
    cands = all_users[::2] + [10 ** 8, "nobody"]
    mask = np.zeros(m.interactions.shape[0], bool)
    mask[all_users[::2]] = True
    gc = m.recommend_users_batch(query[:30], top_n=7, candidate_users=cands, as_arrays=True)
    wc = _want(m, q[:30], 7, candidates=mask)
    assert np.array_equal(gc[0], wc[0]) and np.array_equal(bits(gc[1]), bits(wc[1])) and np.array_equal(gc[2], wc[2]) and np.array_equal(gc[3], wc[3])
    assert wc[3].sum() > 0 and (wc[3] < want[3][:30]).any() and set(gc[0][gc[0] >= 0].tolist()) <= set(all_users[::2])
    none = m.recommend_users_batch(query[:5], top_n=7, candidate_users=[], as_arrays=True)
    assert (none[0] == -1).all() and np.isneginf(none[1]).all() and (none[2] == 0).all() and (none[3] == 0).all()
    assert m.recommend_users_batch(query[:5], top_n=7, candidate_users=[]) == [[]] * 5
    # the facade passes everything through
    rec = Recommender(m)
    assert rec.recommend_users_batch(query, top_n=7) == lists and rec.recommend_users(query[1], top_n=7, ret_scores=True) == pairs[1]
    assert rec.recommend_users_batch(query[:30], top_n=7, candidate_users=cands) == [row[:c].tolist() for row, c in zip(gc[0], gc[2])]
    # no items, parameter ranges
    assert m.recommend_users_batch([], top_n=7) == []
    e = m.recommend_users_batch([], top_n=7, as_arrays=True)
    assert e[0].shape == (0, 7) and e[1].shape == (0, 7) and e[2].shape == (0,) and e[3].shape == (0,)
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match="top_n in 1..1024"):
            m.recommend_users_batch(query[:2], top_n=bad)
    m.recommend_users_batch(query[:2], top_n=1024)
    # the existing calls are untouched by the CSC side that was attached
    assert m.model.engine.has_csc()
    assert m.recommend_batch(all_users[:10], top_k=5) == _model()[0].recommend_batch(all_users[:10], top_k=5)


def test_recommend_users_batch_string_ids_and_an_item_the_fit_never_reached():
    m, batch = _model(strings=True)
    items = sorted({i for _, i, _, _ in batch})[:25]
    q = [m.item_ids.get_id(i) for i in items]
    want = _want(m, q, 6)
    users, scores, counts, eligible = m.recommend_users_batch(items, top_n=6, as_arrays=True)
    assert np.array_equal(users, want[0]) and np.array_equal(bits(scores), bits(want[1])) and np.array_equal(eligible, want[3])
    lists = m.recommend_users_batch(items + ["never seen", 3], top_n=6, ret_scores=True)
    get = m.user_ids.get                                                  # string ids: the arrays hold internal ids
    for b in range(len(items)):
        assert lists[b] == [(get(int(u)), float(s)) for u, s in zip(users[b, :counts[b]], scores[b, :counts[b]])]
    assert all(isinstance(u, str) for row in lists for u, _ in row) and sum(len(r) for r in lists) > 50 and lists[-2:] == [[], []]
    known = sorted({u for u, _, _, _ in batch})[:40]
    sub = m.recommend_users_batch(items, top_n=6, candidate_users=known + ["nobody", 17])
    assert set(u for row in sub for u in row) <= set(known) and any(sub)
    # an item that arrives after the fit is in the store but not in W: an empty audience, and X's new column does no harm
    m.add_interactions([(known[0], "brand new", 2.0e9, 3.0)])
    after = m.recommend_users_batch(["brand new", items[0]], top_n=6)
    assert after[0] == [] and len(after[1]) == 6


def test_scores_are_those_of_the_decayed_matrix_recommend_serves_from():
    batch = _batch()
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5, decay_in_days=30)
    m.fit(batch, progress_bar=False)
    items = sorted({i for _, i, _, _ in batch})[:10]
    before = m.recommend_users_batch(items, top_n=5, as_arrays=True)
    u0 = batch[0][0]
    m.add_interactions([(u0, items[0], max(t for _, _, t, _ in batch) + 40 * 86400.0, 4.0)])      # max_timestamp moves on
    after = m.recommend_users_batch(items, top_n=5, as_arrays=True)
    want = _want(m, items, 5)
    assert np.array_equal(after[0], want[0]) and np.array_equal(bits(after[1]), bits(want[1])) and np.array_equal(after[3], want[3])
    assert not np.array_equal(bits(after[1]), bits(before[1]))


def test_not_fitted_lossy_and_sharded_weights_are_refused():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    fresh = cpu_slim()
    with pytest.raises(RuntimeError, match="Model must be fitted before calling recommend_users_batch"):
        fresh.recommend_users_batch([1])
    with pytest.raises(RuntimeError, match="Model must be fitted before calling recommend_users_batch"):
        fresh.model.recommend_users_batch([1], 5)
    with pytest.raises(RuntimeError, match="Model must be fitted"):
        SlimEngine(backend=AudienceOracleBackend()).audience_items([1], 5)
    m, batch = _model()
    items = sorted({i for _, i, _, _ in batch})[:8]
    W = m.model.item_similarity
    base = m.recommend_users_batch(items, top_n=5, ret_scores=True)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)         # float64 W holding float32 numbers: the float32 model's scores
    assert m.recommend_users_batch(items, top_n=5, ret_scores=True) == base and any(base)
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.recommend_users_batch(items, top_n=5)
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.recommend_users_batch([], top_n=5)
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=AudienceOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
        eng.audience_items([1], 5)
    # the engine boundary of SLIMElastic: the resident X, internal ids; an X without its CSC side is an error, not a guess
    X = m.interactions.to_csr()
    se = SLIMElastic({"nn_feature_selection": 5}, engine=SlimEngine(backend=AudienceOracleBackend()))
    se.item_similarity = W
    se.engine.set_interactions(None, X, need_csc=False)
    with pytest.raises(RuntimeError, match="CSC orientation"):
        se.recommend_users_batch(items, 5)
    se.engine.set_interactions(X.tocsc(), X)
    got = se.recommend_users_batch(items + [-1, 10 ** 6, 2 ** 40], 5, filter_interacted=False, candidate_rows=[0, 1, 2, 3, 5, 8, -4, 10 ** 9])
    cand = np.zeros(X.shape[0], bool)
    cand[[0, 1, 2, 3, 5, 8]] = True
    Xc, Wc = X.tocsc(), W.tocsc()
    Xc.sort_indices(); Wc.sort_indices()
    want = host_model(Xc, Wc, items + [-1, -1, -1], 5, False, cand)
    assert all(np.array_equal(g.view(np.int32), w.view(np.int32)) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="top_n in 1..1024"):
        se.recommend_users_batch(items, 1025)


# ---------------------------------------------------------------------------------------------- serving
def test_recommend_users_route_token_payload_and_failure():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = _model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    item = batch[0][1]
    r = client.post("/recommend_users", json={"item": item, "top_n": 4}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/recommend_users", json={"item": item, "top_n": 4}, headers=ok)
    want = m.recommend_users(item, top_n=4, ret_scores=True)
    assert r.status_code == 200 and len(want) == 4
    assert r.json() == {"item": item, "users": [{"user": u, "score": s} for u, s in want]}
    cands = [u for u, _ in want[1:3]] + [10 ** 8]
    r = client.post("/recommend_users", json={"item": item, "top_n": 4, "filter_interacted": False, "candidate_users": cands}, headers=ok)
    assert r.status_code == 200
    assert r.json()["users"] == [{"user": u, "score": s} for u, s in m.recommend_users(item, 4, False, cands, ret_scores=True)]
    assert len(r.json()["users"]) == 2
    r = client.post("/recommend_users", json={"item": 10 ** 7}, headers=ok)
    assert r.status_code == 200 and r.json() == {"item": 10 ** 7, "users": []}
    r = client.post("/recommend_users", json={"item": item, "top_n": 5000}, headers=ok)      # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Audience failed"}
    r = client.post("/recommend", json={"user": batch[0][0], "top_k": 4}, headers=ok)         # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(batch[0][0], top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def test_audience_topk_is_registered_declared_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    assert "audience_topk" in ops.OPS and ops.EXPORT_OF["audience_topk"] == "rtrec_slim_audience_topk"
    schema = str(torch.ops.rtrec_amd.audience_topk.default._schema)
    for name in ("users", "scores", "count", "eligible", "ws"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("items", "xc_ptr", "xc_row", "xc_val", "wc_ptr", "wc_row", "wc_val"):
        assert f"Tensor {name}" in schema, schema
    assert "Tensor? user_mask" in schema and "int top_n" in schema and "bool filter_interacted" in schema and "int n_users" in schema
    header = open(os.path.join(ROOT, "include", "rtrec_amd.h")).read()
    assert re.search(r"\bint rtrec_slim_audience_topk\s*\(", header) and re.search(r"\bsize_t rtrec_slim_audience_workspace_bytes\s*\(", header)
    assert "rtrec_slim_audience_topk" in _native.EXPORTS and "rtrec_slim_audience_workspace_bytes" in _native.EXPORTS
    assert "audience.hip" in build.SOURCES
    assert callable(getattr(HipBackend, "audience_topk")) and callable(getattr(SlimEngine, "audience_device"))
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.audience_topk(i32(1), 4, i32(4), i32(1), torch.zeros(1), i32(4), i32(1), torch.zeros(1), 2, True, None,
                                              i32(1, 2), torch.zeros(1, 2), i32(1), i32(1), torch.zeros(64, dtype=torch.uint8))


def test_c_entry_point_checks_its_arguments_before_touching_a_device():
    from rtrec_amd import _native
    L = _native.load()
    size = L.rtrec_slim_audience_workspace_bytes
    tiles = lambda U: max(1, -(-U // 8192))
    assert size(1200, 400, 10) == 400 * tiles(1200) * (10 * 8 + 8)
    assert size(138_493, 64, 1024) == 64 * tiles(138_493) * (1024 * 8 + 8)
    one = tiles(138_493) * (1024 * 8 + 8)
    assert size(138_493, 100_000, 1024) == 256 << 20 and (256 << 20) >= one       # capped: the call works through the items in passes
    assert size(2 ** 31 - 1, 5, 1024) == tiles(2 ** 31 - 1) * (1024 * 8 + 8)       # one item needs more than the cap
    assert size(1200, 0, 10) == 0 and size(1200, 4, 0) == 0 and size(1200, 4, 1025) == 0 and size(-1, 4, 10) == 0
    fn = L.rtrec_slim_audience_topk
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_q=1, top_n=10, n_users=100, n_items=5, xnnz=0, wnnz=0, items=one, users=one, scores=one, count=one, eligible=one, ws=one, ws_bytes=1 << 20: (
        n_q, items, n_users, n_items, one, one, one, xnnz, one, one, one, wnnz, top_n, 1, None, users, scores, count, eligible, ws, ws_bytes, None)
    for kw in (dict(top_n=0), dict(top_n=1025), dict(top_n=-1), dict(xnnz=2 ** 31), dict(wnnz=2 ** 31)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_q=-1), dict(n_users=-1), dict(n_items=-1), dict(xnnz=-1), dict(wnnz=-1), dict(items=None), dict(users=None),
               dict(scores=None), dict(count=None), dict(eligible=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_q=0)) == 0 and fn(*args(n_q=0, users=None, ws=None, ws_bytes=0)) == 0
    for kw in (dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=10 * 8 + 7)):
        assert fn(*args(**kw)) == -3, kw
