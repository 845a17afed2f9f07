"""Rerank of per-user candidate lists (SLIM.rerank_batch / score_pairs, csrc/score_pairs.hip) without a GPU: the definition as a
numpy host model, pinned to the reference's own outputs on the golden fixture; the model / facade / serving layers end to end
through the CPU stand-in backend with `score_pairs` supplied by the host model; the registration of the op and the C entry
point's host-side checks.  The kernel itself is in tests/test_gpu_rerank.py.

The definition (include/rtrec_amd.h, "RERANK PER-USER CANDIDATE LISTS"): score(u, i) is the float32 sum of fl32(x_uj * w_ji)
over the j stored in both row u of X and column i of W, added from +0.0f in ascending j; support is their number; a list
position at or beyond counts[r] or with an item outside [0, n_items) is empty (score 0, support -1, never competes); a row
outside X is an empty row (score 0, support 0); NaN scores and -- with filter_interacted -- items stored in the row do not
compete; position p beats q if score[p] > score[q], or the scores are == and p > q."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.cpu_backend import OracleBackend
from tests.test_explain_host import bits, golden, ordered_sum, pair_contributions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------------------------------------- the host model
def host_model(X, W, rows, ids, counts, top_k, filter_interacted=False):
    """THE DEFINITION: (scores[B, k] float32, support[B, k] int32, order[B, top_k] int32, count[B] int32); X csr / W csc with
    sorted indices."""
    ids = np.asarray(ids)
    B, k = ids.shape
    U, I = X.shape[0], W.shape[1]
    scores, support = np.zeros((B, k), np.float32), np.full((B, k), -1, np.int32)
    order, count = np.full((B, top_k), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        u = int(rows[b])
        own = set(X.indices[X.indptr[u]:X.indptr[u + 1]].tolist()) if 0 <= u < U else set()
        competing = []
        for p in range(min(max(int(counts[b]), 0), k)):
            item = int(ids[b, p])
            if not 0 <= item < I:
                continue
            j, c = pair_contributions(X, W, u, item)
            scores[b, p], support[b, p] = ordered_sum(c), len(j)
            if not np.isnan(scores[b, p]) and not (filter_interacted and item in own):
                competing.append(p)
        # p beats q: the larger score, among == scores the LATER position
        ranked = sorted(competing, key=lambda p: (-float(scores[b, p]), -p))[:top_k]
        order[b, :len(ranked)], count[b] = ranked, len(ranked)
    return scores, support, order, count


def host_model_vectorised(X, W, rows, ids, counts, top_k, filter_interacted=False, chunk=4096):
    """The same function without a Python loop per pair: what the larger GPU tests and tools/rerank_bench.py compare against."""
    ids, rows, counts = np.asarray(ids), np.asarray(rows, dtype=np.int64), np.asarray(counts)
    B, k = ids.shape
    U, I = X.shape[0], W.shape[1]
    scores, support = np.zeros((B, k), np.float32), np.full((B, k), -1, np.int32)
    order, count = np.full((B, top_k), -1, np.int32), np.zeros(B, np.int32)
    xkey = np.repeat(np.arange(U, dtype=np.int64), np.diff(X.indptr)) * I + X.indices        # ascending: X is a sorted CSR
    xval = X.data.astype(np.float32)
    wptr, wlen = W.indptr.astype(np.int64), np.diff(W.indptr).astype(np.int64)

    def stored(key):
        if len(xkey) == 0:
            return np.zeros(len(key), np.int64), np.zeros(len(key), bool)
        pos = np.minimum(np.searchsorted(xkey, key), len(xkey) - 1)
        return pos, xkey[pos] == key

    for s in range(0, B, chunk):
        sub, r = ids[s:s + chunk], rows[s:s + chunk]
        valid = (np.arange(k)[None, :] < counts[s:s + chunk, None]) & (sub >= 0) & (sub < I)
        pb, pp = np.nonzero(valid)
        item = sub[pb, pp].astype(np.int64)
        in_x = (r[pb] >= 0) & (r[pb] < U)
        n = np.where(in_x, wlen[item], 0)
        pair = np.repeat(np.arange(len(item)), n)
        off = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(wptr[item], n)
        pos, hit = stored(r[pb][pair] * I + W.indices[off].astype(np.int64))
        pair, c = pair[hit], xval[pos[hit]] * W.data[off[hit]].astype(np.float32)            # pair-major, ascending j inside a pair
        sup = np.bincount(pair, minlength=len(item))
        term = np.arange(len(pair)) - (np.cumsum(sup) - sup)[pair]                            # the term's place in its pair's sum
        by_term = np.argsort(term, kind="stable")
        ends = np.cumsum(np.bincount(term, minlength=1))
        acc = np.zeros(len(item), np.float32)
        with np.errstate(invalid="ignore"):                                                  # inf - inf is a NaN score, not an error
            for t in range(len(ends)):                                                       # one rounded add per term, in order
                sel = by_term[(ends[t - 1] if t else 0):ends[t]]
                acc[pair[sel]] = acc[pair[sel]] + c[sel]
        scores[s + pb, pp], support[s + pb, pp] = acc, sup
        competes = ~np.isnan(acc)
        if filter_interacted:
            competes &= ~(in_x & stored(np.where(in_x, r[pb], 0) * I + item)[1])
        cb, cp, cs = pb[competes], pp[competes], acc[competes]
        by_rank = np.lexsort((-cp, -cs, cb))                                                 # row, score descending, later position
        cb, cp = cb[by_rank], cp[by_rank]
        per_row = np.bincount(cb, minlength=len(sub))
        rank = np.arange(len(cb)) - (np.cumsum(per_row) - per_row)[cb]
        keep = rank < top_k
        order[s + cb[keep], rank[keep]] = cp[keep]
        count[s:s + chunk] = np.minimum(per_row, top_k)
    return scores, support, order, count


PAIRS_TRIP_LENGTHS = [0, 1, 128, 129, 2048, 2049] * 2     # rows of X on both sides of the kernel's two staging limits (128 and 2,048 entries)


def pairs_trip_case(seed=29):
    """More list rows than the list stage's grid (65,536): the 509 patterns of a 65,536 + 3 row call (row r carries pattern
    r % 509; tests/test_factor_host.py).  X has 12 rows of PAIRS_TRIP_LENGTHS entries over 4,000 items, W 40 stored columns of 30
    weights (every column stores rows 0 .. 9, which every non-empty row of X holds some of); a pattern is a row of X, a list of 5
    ids (some of them empty columns, -1 or beyond the catalogue) and a count of 0 .. 5.  Across the cap: row 0 is an unstaged row
    (2,049 entries) and row 65,536 a staged one of one entry, rows 1 / 65,537 the reverse, row 2 a full list and row 65,538 an
    empty one.  (X, W, rows, ids, counts) per pattern, list_k 5."""
    rng = np.random.default_rng(seed)
    I, P = 4000, 509
    xi = [np.sort(np.r_[rng.choice(10, min(L, 1 + L // 256), replace=False), 10 + rng.choice(I - 10, L - min(L, 1 + L // 256), replace=False)])
          for L in PAIRS_TRIP_LENGTHS]
    X = sp.csr_matrix((rng.standard_normal(sum(PAIRS_TRIP_LENGTHS)).astype(np.float32), np.concatenate(xi).astype(np.int32),
                       np.cumsum([0] + PAIRS_TRIP_LENGTHS)), shape=(len(PAIRS_TRIP_LENGTHS), I))
    wi = [np.sort(np.r_[np.arange(10), 10 + rng.choice(I - 10, 20, replace=False)]) for _ in range(40)]
    wptr = np.zeros(I + 1, np.int64)
    wptr[1:41] = np.cumsum([len(w) for w in wi])
    wptr[41:] = wptr[40]
    W = sp.csc_matrix((rng.standard_normal(40 * 30).astype(np.float32), np.concatenate(wi).astype(np.int32), wptr), shape=(I, I))
    rows = rng.integers(0, 12, P).astype(np.int32)
    rows[::31] = rng.choice(np.array([-1, 12], np.int32), len(rows[::31]))
    ids = rng.integers(0, 46, (P, 5)).astype(np.int32)
    ids[rng.random((P, 5)) < 0.05] = -1
    ids[rng.random((P, 5)) < 0.05] = I
    counts = rng.integers(0, 6, P).astype(np.int32)
    rows[[0, 1, 2]], rows[[384, 385, 386]] = [5, 7, 3], [1, 11, 2]
    counts[[0, 1, 2]], counts[[384, 385, 386]] = [5, 5, 5], [5, 5, 0]
    ids[[0, 1, 2, 384, 385, 386]] = np.stack([rng.permutation(40)[:5] for _ in range(6)])
    return X, W, rows, ids, counts


def test_pairs_trip_case_is_the_definition_and_crosses_the_staging_limits_across_the_cap():
    X, W, rows, ids, counts = pairs_trip_case()
    want = host_model_vectorised(X, W, rows, ids, counts, 3, True)
    assert_same(want, host_model(X, W, rows, ids, counts, 3, True), "patterns")
    lens = np.diff(X.indptr)
    assert lens.tolist() == PAIRS_TRIP_LENGTHS and 65536 % 509 == 384
    row_len = np.where((rows >= 0) & (rows < 12), lens[np.clip(rows, 0, 11)], 0)
    assert set(row_len.tolist()) == set(PAIRS_TRIP_LENGTHS)
    for limit in (128, 2048):                       # both launch widths: an unstaged row and a one-entry row share a workgroup, in both orders
        assert row_len[0] > limit and row_len[384] == 1 and row_len[1] == 1 and row_len[385] > limit
    assert counts[2] == 5 and counts[386] == 0 and want[3][2] == 3 and want[3][386] == 0
    assert (want[1][[0, 1, 384, 385]] > 0).all() and (want[0][[0, 1, 384, 385]] != 0).all()      # every pair of those rows has support
    filtered = sum(int(((want[1][x] >= 0) & np.isin(ids[x], X.indices[X.indptr[rows[x]]:X.indptr[rows[x] + 1]])).sum())
                   for x in range(509) if 0 <= rows[x] < 12)
    assert filtered > 50 and (want[3] < np.minimum(counts, 3)).any()                             # the filter decides lists


def assert_same(got, want, what=""):
    names = ("scores", "support", "order", "count")
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the host model {w.shape}"
        bad = np.flatnonzero((bits(g) != bits(w)).ravel() if name == "scores" else (g != w).ravel())
        assert bad.size == 0, f"{what}: {bad.size} {name} differ from the host model, first at flat index {int(bad[0])}: {g.ravel()[bad[0]]} != {w.ravel()[bad[0]]}"


def golden_scoring():
    return np.load(os.path.join(G, "scoring.npz"))


def golden_permuted_lists():
    """All 240 users of golden(), each with a seeded permutation of all 400 items as its list."""
    X, W, users, ids, scores = golden()
    rng = np.random.default_rng(29)
    lists = np.stack([rng.permutation(W.shape[1]) for _ in users]).astype(np.int32)
    return X, W, users, lists, ids, scores


class PairsOracleBackend(OracleBackend):
    """The CPU stand-in plus score_pairs from the host model (TEST-ONLY, like its base)."""

    def score_pairs(self, row_ids, xb, n_items, W, ids, counts, list_k, top_k, filter_interacted, scores, support, order, count,
                    waves_per_row=0):
        import torch
        ptr, col, val = (t.numpy() for t in xb)
        X = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, n_items))
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        rows = row_ids.numpy() if row_ids is not None else np.arange(ids.shape[0])
        out = host_model_vectorised(X, Wc, rows, ids.numpy()[:, :list_k], counts.numpy(), top_k, filter_interacted)
        for dst, src in zip((scores, support, order, count), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=PairsOracleBackend())
    return m


# ---------------------------------------------------------------------------------------------- the definition
def test_scores_reproduce_the_reference_predict_files_bit_for_bit():
    X, W, _, _, _ = golden()
    z = golden_scoring()
    users, cands = z["predict_users"], z["cands"]
    I = W.shape[1]
    assert I == 400 and z["predict_dense"].shape == (4, 400) and z["predict_selected"].shape == (4, len(cands))
    every = np.tile(np.arange(I, dtype=np.int32), (len(users), 1))
    for model in (host_model, host_model_vectorised):
        sc, su, order, count = model(X, W, users, every, np.full(len(users), I), 0)
        assert np.array_equal(bits(sc), bits(z["predict_dense"])) and su.min() >= 0 and su.max() > 3
        assert order.shape == (4, 0) and (count == 0).all()
        sel = model(X, W, users, np.tile(cands.astype(np.int32), (len(users), 1)), np.full(len(users), len(cands)), 0)[0]
        assert np.array_equal(bits(sel), bits(z["predict_selected"]))


def test_ranking_reproduces_the_reference_top10_of_all_240_users():
    X, W, users, lists, ids, scores = golden_permuted_lists()
    assert ids.shape == (240, 10) and lists.shape == (240, 400)
    for model in (host_model, host_model_vectorised):
        sc, su, order, count = model(X, W, users, lists, np.full(240, 400), 10, True)
        assert (count == 10).all()
        # no tied neighbours among the first 11 of any list: the tie rule cannot hide a difference
        full = model(X, W, users, lists, np.full(240, 400), 11, True)[2]
        top11 = np.take_along_axis(sc, full, axis=1)
        assert (top11[:, 1:] < top11[:, :-1]).all()
        assert np.array_equal(np.take_along_axis(lists, order, axis=1), ids)
        assert np.array_equal(bits(np.take_along_axis(sc, order, axis=1)), bits(scores.astype(np.float32)))


def test_vectorised_model_is_the_definition():
    X, W, users, lists, _, _ = golden_permuted_lists()
    rng = np.random.default_rng(6)
    ids = lists[:, :37].copy()
    ids[rng.random(ids.shape) < 0.05] = -1
    ids[3, 4], ids[7, 0] = W.shape[1], W.shape[1] + 7
    ids[:, 20] = ids[:, 2]                                               # duplicates
    counts = rng.integers(-2, 41, len(users)).astype(np.int32)
    rows = users.copy()
    rows[5], rows[9] = -1, X.shape[0]
    for filt in (False, True):
        for top_k in (0, 1, 10, 37):
            a = host_model(X, W, rows, ids, counts, top_k, filt)
            assert_same(host_model_vectorised(X, W, rows, ids, counts, top_k, filt, chunk=41), a, f"filter={filt} k={top_k}")
    assert (a[1][5][:counts[5]][ids[5, :max(counts[5], 0)] >= 0] == 0).all() and a[1].max() > 3


def test_hand_written_cases():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    # items 0..7; user 0 holds items 0 (1.0), 1 (2.0), 5 (inf), 6 (1.0); user 1 holds nothing
    X = sp.csr_matrix((np.array([1.0, 2.0, inf, 1.0], np.float32), np.array([0, 1, 5, 6]), np.array([0, 4, 4])), shape=(2, 8))
    W = sp.lil_matrix((8, 8), dtype=np.float32)
    W[0, 2] = 3.0                      # score(0, 2) = 3
    W[1, 3] = 1.5                      # score(0, 3) = 3: ties with item 2
    W[0, 4], W[1, 4] = 1.0, 1.0        # score(0, 4) = 3 too (1 + 2)
    W[5, 1] = 1.0                      # score(0, 1) = +inf, and item 1 is interacted
    W[5, 0] = -1.0                     # score(0, 0) = -inf, interacted
    W[5, 7], W[0, 7] = 1.0, 0.0        # an explicit zero is dropped by lil: column 7 holds j = 5 alone -> inf
    W[6, 6] = 1.0
    W = W.tocsc()
    Xn = sp.csr_matrix((np.array([inf, inf], np.float32), np.array([0, 1]), np.array([0, 2])), shape=(1, 3))
    Wn = sp.csc_matrix((np.array([1.0, -1.0], np.float32), np.array([0, 1]), np.array([0, 0, 0, 2])), shape=(3, 3))
    ids = np.array([[2, 3, 4, 2, 1, 0, 7, -1, 8, 3]], np.int32)
    for model in (host_model, host_model_vectorised):
        sc, su, order, count = model(X, W, [0], ids, [10], 10, False)
        assert sc[0].tolist() == [3.0, 3.0, 3.0, 3.0, inf, -inf, inf, 0.0, 0.0, 3.0]
        assert su[0].tolist() == [1, 1, 2, 1, 1, 1, 1, -1, -1, 1]
        # inf first (the later of the two), the five 3.0 from the last position backwards (duplicates are positions), -inf last
        assert order[0].tolist() == [6, 4, 9, 3, 2, 1, 0, 5, -1, -1] and count[0] == 8
        sc2, su2, order2, count2 = model(X, W, [0], ids, [10], 3, True)
        assert np.array_equal(bits(sc2), bits(sc)) and np.array_equal(su2, su)       # filtered scores are still written
        assert order2[0].tolist() == [6, 9, 3] and count2[0] == 3                  # items 1 and 0 are stored in the row
        # beyond counts: empty; a row outside X: support 0, every valid position competes with 0.0, the later first
        sc3, su3, order3, count3 = model(X, W, [0, 2, -1], np.tile(ids, (3, 1)), [4, 10, 10], 10, False)
        assert su3[0].tolist() == [1, 1, 2, 1] + [-1] * 6 and order3[0].tolist() == [3, 2, 1, 0] + [-1] * 6
        for b in (1, 2):
            assert su3[b].tolist() == [0, 0, 0, 0, 0, 0, 0, -1, -1, 0] and not sc3[b].any()
            assert order3[b].tolist() == [9, 6, 5, 4, 3, 2, 1, 0, -1, -1] and count3[b] == 8
        # two inf ratings against weights of both signs: inf - inf = NaN -- written, never listed
        scn, sun, ordern, countn = model(Xn, Wn, [0], np.array([[2, 0]], np.int32), [2], 2, False)
        assert np.isnan(scn[0, 0]) and scn[0, 1] == 0.0 and sun[0].tolist() == [2, 0]
        assert ordern[0].tolist() == [1, -1] and countn[0] == 1
    # the -0.0-only pair: 0 + -0 = +0, support 1
    Xz = sp.csr_matrix((np.array([-1.0], np.float32), np.array([0]), np.array([0, 1])), shape=(1, 2))
    Wz = sp.csc_matrix((np.array([0.0], np.float32), np.array([0]), np.array([0, 0, 1])), shape=(2, 2))
    assert Wz.nnz == 1 and np.signbit(np.float32(-1.0) * Wz.data[0])
    for model in (host_model, host_model_vectorised):
        sc, su, _, _ = model(Xz, Wz, [0], np.array([[1]], np.int32), [1], 0)
        assert su[0, 0] == 1 and bits(sc)[0, 0] == 0


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _batch(strings=False):
    z = np.load(os.path.join(G, "partial_fit.npz"))
    a, b = z["A"][0], z["C"][1]
    name = (lambda p, x: f"{p}{x}") if strings else (lambda p, x: int(x))
    return [(name("u", x), name("i", y), float(t), float(r)) for x, y, t, r in zip(z["u"][a:b], z["i"][a:b], z["ts"][a:b], z["v"][a:b])]


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)      # the contract is the float32 model's
    return m, batch


@pytest.mark.parametrize("strings", [False, True])
def test_rerank_batch_is_recommend_with_the_users_own_candidates(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    rng = np.random.default_rng(8)
    known_users = sorted({u for u, _, _, _ in batch}, key=str)
    known_items = sorted({i for _, i, _, _ in batch}, key=str)
    unknown_item = "never seen" if strings else 10 ** 7
    cold = "nobody" if strings else max(known_users) + 1000
    users = known_users[:30] + [cold, known_users[3], cold, cold]
    cands = []
    for b in range(len(users)):
        n = int(rng.integers(1, 40))
        if b % 2:                                                        # drawn with replacement: duplicated candidates
            c = [known_items[j] for j in rng.integers(0, len(known_items), n)]
        else:
            c = [known_items[j] for j in rng.permutation(len(known_items))[:n]]
        c.insert(int(rng.integers(0, n + 1)), unknown_item)
        cands.append(c)
    cands[32] = known_items[:]                                          # a cold user whose list holds every hot item
    cands[33] = known_items[:6] + [unknown_item] + known_items[:3]      # ... and one with duplicates
    dup = [len(set(c)) < len(c) for c in cands]
    assert sum(dup) >= 10 and sum(not d for d in dup) >= 10 and not dup[30] and not dup[32] and dup[33]

    def first_of_each(row):                                             # a ranked list with every item at its best entry only
        return [x for p, x in enumerate(row) if x not in row[:p]]

    for top_k in (1, 5, 1000):
        got = m.rerank_batch(users, cands, top_k=top_k)
        for b, (u, c) in enumerate(zip(users, cands)):
            # the contract.  The CPU stand-in ranks a candidate list through the engine's rank array (one rank per column of
            # W), which keeps ONE entry per item, the last; the reference's X[u] @ W[:, candidates] and the request kernel of
            # the device (tests/test_gpu_rerank.py holds the contract there) keep every entry.  So a list with duplicates is
            # compared whole: its ranking with every item at its best entry -- the later one -- is the stand-in's answer
            if not dup[b]:
                assert got[b] == m.recommend(u, candidate_items=c, top_k=top_k), (b, top_k)
                assert u == cold or len(got[b]) == min(top_k, len(c) - 1)
            elif top_k == 1000:
                assert first_of_each(got[b]) == m.recommend(u, candidate_items=c, top_k=top_k), b
                assert u == cold or sorted(got[b], key=str) == sorted(c[:c.index(unknown_item)] + c[c.index(unknown_item) + 1:], key=str)
    assert got[32] and got[33] and got[30] != got[32]
    # top_k=None ranks the whole list; rerank is the single-user form; Recommender passes everything through
    whole = m.rerank_batch(users, cands)
    assert whole == m.rerank_batch(users, cands, top_k=1000)
    assert all(whole[b] == m.recommend(users[b], candidate_items=cands[b], top_k=1000) for b in range(len(users)) if not dup[b])
    assert m.rerank(users[2], cands[2]) == whole[2] and m.rerank(users[2], cands[2], top_k=3) == whole[2][:3]
    rec = Recommender(m)
    assert rec.rerank_batch(users, cands, top_k=5) == m.rerank_batch(users, cands, top_k=5) and rec.rerank(users[1], cands[1]) == whole[1]
    # the documented exception: a list that is empty after mapping yields [], where recommend ranks the whole catalogue
    assert m.rerank_batch([users[0], cold], [[unknown_item], []], top_k=5) == [[], []]
    assert len(m.recommend(users[0], candidate_items=[unknown_item], top_k=5)) == 5
    assert m.rerank_batch([], []) == [] and m.rerank_batch(users[:2], cands[:2], top_k=0) == [[], []]
    with pytest.raises(ValueError, match="one list per user"):
        m.rerank_batch(users[:2], cands[:1])
    # ret_scores and as_arrays say the same as the lists, with the host model's scores
    pairs = m.rerank_batch(users, cands, top_k=5, ret_scores=True)
    assert [[i for i, _ in row] for row in pairs] == m.rerank_batch(users, cands, top_k=5)
    assert all(isinstance(s, float) for row in pairs for _, s in row)
    ids, sc, counts = m.rerank_batch(users, cands, top_k=5, as_arrays=True)
    assert ids.shape == sc.shape == (len(users), 5) and counts.shape == (len(users),)
    X, W = m.interactions.to_csr(), m.model.item_similarity.tocsc()
    X.sort_indices(); W.sort_indices()
    raw_of = m.item_ids.get
    for b, row in enumerate(pairs):
        n = int(counts[b])
        assert n == len(row) and (ids[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all()
        if users[b] == cold:
            assert ids[b, :n].tolist() == [i for i, _ in row] and not sc[b, :n].any()
            continue
        assert [raw_of(int(i)) for i in ids[b, :n]] == [i for i, _ in row]
        assert np.array_equal(bits(sc[b, :n]), bits([s for _, s in row]))
        uid = m._known_user_id(users[b])
        for i, s in zip(ids[b, :n].tolist(), sc[b, :n]):
            assert bits(s) == bits(ordered_sum(pair_contributions(X, W, uid, i)[1]))
    assert rec.rerank_batch(users, cands, top_k=5, as_arrays=True)[2].tolist() == counts.tolist()
    # integer ids: one [B, k] array of candidates is the B lists
    if not strings:
        block = rng.integers(0, max(known_items) + 40, (len(users), 12))
        assert (block > m.interactions.max_item_id).any()
        for kw in (dict(top_k=4), dict(ret_scores=True), dict(top_k=6, as_arrays=True, filter_interacted=True)):
            a, b = m.rerank_batch(np.asarray(users), block, **kw), m.rerank_batch(users, block.tolist(), **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) if kw.get("as_arrays") else a == b, kw
    # filter_interacted leaves out what the user's row stores
    u0 = users[0]
    seen = [i for u, i, _, _ in batch if u == u0]
    mixed = seen[:3] + [i for i in known_items if i not in seen][:4]
    kept = m.rerank(u0, mixed, filter_interacted=True)
    assert sorted(kept, key=str) == sorted(mixed[3:], key=str) and len(m.rerank(u0, mixed)) == 7


def test_score_pairs_against_the_host_model_with_unknowns_and_chunking():
    from rtrec_amd.recommender import Recommender
    m, batch = _model()
    X, W = m.interactions.to_csr(), m.model.item_similarity.tocsc()
    X.sort_indices(); W.sort_indices()
    rng = np.random.default_rng(9)
    known_users = sorted({u for u, _, _, _ in batch})
    known_items = sorted({i for _, i, _, _ in batch})
    n = 3000
    users = [known_users[j] for j in rng.integers(0, len(known_users), n)]
    items = [known_items[j] for j in rng.integers(0, len(known_items), n)]
    heavy = known_users[4]
    users[200:1500] = [heavy] * 1300                                     # more than 1024 pairs of one user: two kernel rows
    users[7], items[11], users[13], items[13] = max(known_users) + 99, 10 ** 7, "who", "what"
    scores, support = m.score_pairs(users, items, as_arrays=True)
    assert scores.dtype == np.float32 and scores.shape == support.shape == (n,)
    unknown = {7, 11, 13}
    for p in range(n):
        if p in unknown:
            assert scores[p] == 0.0 and support[p] == -1
            continue
        j, c = pair_contributions(X, W, users[p], items[p])
        assert support[p] == len(j) and bits(scores[p]) == bits(ordered_sum(c)), p
    assert (support == 0).any() and support.max() >= 3 and users.count(heavy) > 1024
    assert np.array_equal(bits(m.score_pairs(users, items)), bits(scores))
    assert np.array_equal(bits(Recommender(m).score_pairs(np.asarray(users[20:40]), np.asarray(items[20:40]))), bits(scores[20:40]))
    assert m.score_pairs([], []).shape == (0,)
    with pytest.raises(ValueError, match="one length"):
        m.score_pairs(users[:3], items[:2])
    # SLIMElastic's host-CSR boundary and the engine's column chunks
    se = m.model
    lists = [[3, 1, 10 ** 6], [], [2, 2]]
    rows = known_users[:3]
    got = se.score_pairs_batch(rows, X, lists, top_k=2, filter_interacted=True)
    ids = np.array([[3, 1, -1], [-1, -1, -1], [2, 2, -1]], np.int32)
    assert_same(got, host_model(X, W, rows, ids, [3, 0, 2], 2, True), "score_pairs_batch")
    wide = rng.integers(-1, W.shape[1] + 2, (3, 2500)).astype(np.int32)
    counts = np.array([2500, 1024, 1500], np.int32)
    got = se.engine.score_pairs_rows(rows, wide, counts, xb=se.engine._upload_csr(X))
    assert_same(got, host_model_vectorised(X, W, rows, wide, counts, 0), "chunked lists")


def test_unservable_weights_and_long_lists_are_refused():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    fresh = cpu_slim()
    for call in (lambda: fresh.rerank_batch([1], [[1]]), lambda: fresh.score_pairs([1], [1]),
                 lambda: fresh.model.score_pairs_batch([0], sp.csr_matrix((1, 3), dtype=np.float32), [[1]])):
        with pytest.raises(RuntimeError, match="Model must be fitted"):
            call()
    m, batch = _model()
    users = sorted({u for u, _, _, _ in batch})[:4]
    items = sorted({i for _, i, _, _ in batch})
    W = m.model.item_similarity
    want = m.rerank_batch(users, [items[:30]] * 4, top_k=8, ret_scores=True)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)         # float64 W holding float32 numbers: served with them
    assert m.rerank_batch(users, [items[:30]] * 4, top_k=8, ret_scores=True) == want
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.rerank_batch(users, [items[:30]] * 4)
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.score_pairs(users, items[:4])
    m.model.item_similarity = W
    # a list longer than 1024 with ranking; without ranking the engine works through it in chunks (tested above)
    long_list = [items[j % len(items)] for j in range(1025)]
    with pytest.raises(ValueError, match="1024"):
        m.rerank_batch(users[:1], [long_list])
    assert len(m.rerank(users[0], long_list[:1024], top_k=3)) == 3
    with pytest.raises(ValueError, match="1024"):
        m.model.engine.score_pairs_rows([0], np.zeros((1, 1025), np.int32), top_k=5)
    with pytest.raises(ValueError, match="top_k"):
        m.model.engine.score_pairs_rows([0], np.zeros((1, 4), np.int32), top_k=5)
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=PairsOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
        eng.score_pairs_rows([0], np.array([[1]], np.int32))


# ---------------------------------------------------------------------------------------------- serving
def test_rerank_route_token_payload_and_failure():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = _model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = batch[0][0]
    items = sorted({i for _, i, _, _ in batch})[:25] + [10 ** 7]
    r = client.post("/rerank", json={"user": user, "items": items, "top_k": 4}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/rerank", json={"user": user, "items": items, "top_k": 4}, headers=ok)
    want = m.rerank(user, items, top_k=4, ret_scores=True)
    assert r.status_code == 200 and len(want) == 4
    assert r.json() == {"user": user, "items": [{"item": i, "score": s} for i, s in want]}
    r = client.post("/rerank", json={"user": user, "items": items}, headers=ok)               # top_k absent: the whole list
    assert r.status_code == 200 and [e["item"] for e in r.json()["items"]] == m.rerank(user, items) and len(r.json()["items"]) == 25
    r = client.post("/rerank", json={"user": user, "items": items, "filter_interacted": True}, headers=ok)
    assert [e["item"] for e in r.json()["items"]] == m.rerank(user, items, filter_interacted=True) != m.rerank(user, items)
    r = client.post("/rerank", json={"user": user, "items": (items[:25] * 41)[:1025]}, headers=ok)   # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Rerank failed"}
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)                # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(user, top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def test_score_pairs_is_registered_declared_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    assert "score_pairs" in ops.OPS and ops.EXPORT_OF["score_pairs"] == "rtrec_slim_score_pairs" and len(ops.OPS) == 22
    schema = str(torch.ops.rtrec_amd.score_pairs.default._schema)
    for name in ("scores", "support", "order", "count"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("xb_ptr", "xb_col", "xb_val", "wc_ptr", "wc_row", "wc_val", "ids", "counts"):
        assert f"Tensor {name}" in schema, schema
    assert "Tensor? row_ids" in schema and "int list_k" in schema and "int top_k" in schema and "int waves_per_row" in schema
    header = open(os.path.join(ROOT, "include", "rtrec_amd.h")).read()
    assert re.search(r"\bint rtrec_slim_score_pairs\s*\(", header)
    assert "rtrec_slim_score_pairs" in _native.EXPORTS and "score_pairs.hip" in build.SOURCES
    L = _native.load()
    # the host-side argument checks run before anything touches a device
    fn = L.rtrec_slim_score_pairs
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_rows=1, list_k=10, top_k=3, ids=one, stride=10, n_items=5, nnz=0, waves=0, order=one, scores=one: (
        n_rows, None, one, one, one, 4, nnz, n_items, one, one, one, 0, ids, stride, list_k, one, top_k, 0, waves, scores, one, order, one, None)
    for kw in (dict(list_k=0), dict(list_k=1025, stride=1025), dict(top_k=-1), dict(top_k=11), dict(waves=2), dict(waves=-1)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_rows=-1), dict(n_items=-1), dict(nnz=-1), dict(stride=9), dict(ids=None), dict(scores=None), dict(order=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, ids=None, scores=None)) == 0
    for name in ("score_pairs_device", "score_pairs_rows"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "score_pairs"))
    if not torch.cuda.is_available():
        with pytest.raises((NotImplementedError, RuntimeError)):
            i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
            torch.ops.rtrec_amd.score_pairs(None, i32(2), i32(1), torch.zeros(1), 3, i32(4), i32(1), torch.zeros(1), i32(1, 2), i32(1), 2, 1,
                                            False, 0, torch.zeros(1, 2), i32(1, 2), i32(1, 1), i32(1))
