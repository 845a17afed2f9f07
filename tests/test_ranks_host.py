"""Full-catalogue ranks of held-out items (SLIM.rank_items_batch / Recommender.evaluate_catalogue, csrc/catalogue_ranks.hip)
without a GPU: the definition as a plain-Python host model and a vectorised one, pinned to the reference's own lists on the
golden fixture; hand-written rows for what the fixture cannot exercise; the pure summary function on hand-computed cases; the
model / facade / serving layers end to end through the CPU stand-in backend with `catalogue_ranks` supplied by the host model;
the registration of the op and the C entry point's host-side checks.  The kernel itself is in tests/test_gpu_ranks.py.

The definition (include/rtrec_amd_ext.h, "CATALOGUE RANKS"), for row r with scores s[c]: own = the in-range columns stored in
X's row (filter_interacted only; a row id outside X has none); competes(c) = s[c] is not NaN, c is not in own, and the mode is
DENSE or s[c] != 0; a target i that is in range and competes has above = |{c != i : competes(c), s[c] > s[i]}| and tied = the
same with ==; any other target has -1 / 0; score = (double) s[i] for i in range, else -inf; competing = |{c : competes(c)}|."""
import math
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.cpu_backend import OracleBackend
from tests.test_rerank_host import _batch, golden, golden_scoring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE, DENSE = 0, 1


# ---------------------------------------------------------------------------------------------- the host models
def host_model(S, n_items, rows, X, filter_interacted, mode, tg_ptr, tg_items):
    """THE DEFINITION, one Python step per column: (above[n_tg] int32, tied[n_tg] int32, score[n_tg] float64, competing[n_rows]
    int32) for the score block S [n_rows, >= n_items]; rows = the row of X (csr) per score row, None = row r."""
    n_rows, n_tg = S.shape[0], len(tg_items)
    above, tied = np.full(n_tg, -1, np.int32), np.zeros(n_tg, np.int32)
    score, competing = np.full(n_tg, -np.inf, np.float64), np.zeros(n_rows, np.int32)
    for r in range(n_rows):
        s = S[r]
        own = set()
        u = r if rows is None else int(rows[r])
        if filter_interacted and 0 <= u < X.shape[0]:
            own = {int(c) for c in X.indices[X.indptr[u]:X.indptr[u + 1]] if 0 <= c < n_items}
        comp = [not math.isnan(s[c]) and c not in own and (mode == DENSE or s[c] != 0) for c in range(n_items)]
        competing[r] = sum(comp)
        for t in range(int(tg_ptr[r]), int(tg_ptr[r + 1])):
            i = int(tg_items[t])
            if not 0 <= i < n_items:
                continue
            score[t] = float(s[i])
            if comp[i]:
                above[t] = sum(1 for c in range(n_items) if c != i and comp[c] and s[c] > s[i])
                tied[t] = sum(1 for c in range(n_items) if c != i and comp[c] and s[c] == s[i])
    return above, tied, score, competing


def host_model_vectorised(S, n_items, rows, X, filter_interacted, mode, tg_ptr, tg_items):
    """The same function with numpy inside a row: what the larger GPU tests, the CPU stand-in and tools/ranks_bench.py use."""
    S, tg_items = np.asarray(S), np.asarray(tg_items, dtype=np.int64)
    n_rows, n_tg = S.shape[0], len(tg_items)
    above, tied = np.full(n_tg, -1, np.int32), np.zeros(n_tg, np.int32)
    score, competing = np.full(n_tg, -np.inf, np.float64), np.zeros(n_rows, np.int32)
    for r in range(n_rows):
        s = S[r, :n_items]
        comp = ~np.isnan(s)
        if mode != DENSE:
            comp &= s != 0
        u = r if rows is None else int(rows[r])
        if filter_interacted and 0 <= u < X.shape[0]:
            own = X.indices[X.indptr[u]:X.indptr[u + 1]]
            comp[own[(own >= 0) & (own < n_items)]] = False
        competing[r] = comp.sum()
        t0, t1 = int(tg_ptr[r]), int(tg_ptr[r + 1])
        items = tg_items[t0:t1]
        ok = (items >= 0) & (items < n_items)
        if not ok.any():
            continue
        si = s[items[ok]]
        score[t0:t1][ok] = si.astype(np.float64)
        live = comp[items[ok]]
        sc = s[comp]
        with np.errstate(invalid="ignore"):
            a = (sc[None, :] > si[:, None]).sum(axis=1)
            e = (sc[None, :] == si[:, None]).sum(axis=1) - 1          # (the target's own hit; only used where it competes)
        above[t0:t1][ok] = np.where(live, a, -1)
        tied[t0:t1][ok] = np.where(live, e, 0)
    return above, tied, score, competing


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what=""):
    for name, g, w in zip(("above", "tied", "score", "competing"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {name} is {g.dtype}{g.shape}, the host model {w.dtype}{w.shape}"
        bad = np.flatnonzero(bits64(g) != bits64(w) if name == "score" else g != w)
        assert bad.size == 0, f"{what}: {bad.size} {name} differ from the host model, first at {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}"


def golden_block(dtype):
    """(X, users, S): the score rows of the 240 fixture users over the 400 items, as scipy's product in `dtype` gives them --
    the numbers the reference ranked."""
    X, W, users, _, _ = golden()
    S = np.asarray((X[users].astype(dtype) @ W.astype(dtype).tocsr()).toarray())
    return X, users, np.ascontiguousarray(S)


def every_pair(n_rows, n_items):
    return np.arange(n_rows + 1, dtype=np.int64) * n_items, np.tile(np.arange(n_items, dtype=np.int32), n_rows)


def hand_case():
    """Seven hand-written rows over 8 items (float32 values; the block is 11 wide with garbage beyond the items) and the X
    they filter by: (S, n_items, rows, X, tg_ptr, tg_items)."""
    nan, inf = np.nan, np.inf
    rows_ = [
        [3, 1, 3, 3, 0, -2, 1, 5],                   # A: a three-way tie, a pair, a zero, a negative
        [0.0, -0.0, -1, 2, -0.0, 0.0, -3, -1],       # B: +0 / -0 and negatives: a zero outranks them only in DENSE
        [nan, inf, -inf, 1, inf, nan, 0, 2],         # C: NaN and +-inf
        [5, 4, 3, 2, 1, 6, 7, 8],                    # D: row 0 of X stores 1 (twice), 5 and the out-of-range 9
        [1, 1, 0, 0, 2, 0, 0, 0],                    # E: no targets; row 1 of X stores column 0 with the value 0
        [1, 2, 0, 0, 0, 0, 0, 0],                    # F: a row id beyond X
        [1, 2, 0, 0, 0, 0, 0, 0],                    # G: a negative row id
    ]
    S = np.full((7, 11), 1e30, np.float32)
    S[:, 8], S[:, 9] = np.nan, 3.0
    S[:, :8] = np.array(rows_, np.float32)
    X = sp.csr_matrix((np.array([1, 1, 0, 2, 0], np.float32), np.array([1, 1, 5, 9, 0]), np.array([0, 4, 5, 5])), shape=(3, 12))
    rows = np.array([2, 2, 2, 0, 1, 7, -1], np.int32)
    targets = [[0, 2, 3, 1, 6, 7, 4, 5], [0, 1, 2, 3, 6, 7], [0, 1, 2, 3, 4], [1, 0, 4, 4, -1, 8, 2], [], [0], [1, 0]]
    tg_ptr = np.zeros(8, np.int64)
    np.cumsum([len(t) for t in targets], out=tg_ptr[1:])
    return S, 8, rows, X, tg_ptr, np.array([i for t in targets for i in t], np.int32)


class RanksOracleBackend(OracleBackend):
    """The CPU stand-in plus catalogue_ranks from the host model, and a score_rows that honours row_ids (TEST-ONLY, like its base)."""

    def score_rows(self, n_rows, row_ids, xb, n_items, col_lo, lay, acc_f64, out):
        import torch
        Wr = self._shard_w(n_items, col_lo, lay)
        ptr, col, val = (t.numpy() for t in xb)
        Xall = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, n_items))
        rsel = row_ids.numpy().astype(np.int64) if row_ids is not None else np.arange(n_rows)
        has = (rsel >= 0) & (rsel < Xall.shape[0])
        dt = np.float64 if acc_f64 else np.float32
        S = np.zeros((n_rows, lay["n_cols"]), dt)
        S[has] = (Xall[rsel[has]].astype(dt) @ Wr.astype(dt)).toarray()[:, col_lo:col_lo + lay["n_cols"]]
        out[:n_rows, :lay["n_cols"]] = torch.from_numpy(S)

    def catalogue_ranks(self, n_items, scores, row_ids, xb, filter_interacted, mode, tg_ptr, tg_items, above, tied, score, competing):
        import torch
        ptr, col, _ = (t.numpy() for t in xb)
        X = sp.csr_matrix((np.ones(len(col), np.float32), col, ptr), shape=(len(ptr) - 1, max(n_items, int(col.max()) + 1 if len(col) else 0)))
        rows = row_ids.numpy() if row_ids is not None else None
        out = host_model_vectorised(scores.numpy(), n_items, rows, X, filter_interacted, mode, tg_ptr.numpy(), tg_items.numpy())
        for dst, src in zip((above, tied, score, competing), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=RanksOracleBackend())
    return m


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


# ---------------------------------------------------------------------------------------------- the definition
def test_the_two_host_models_agree():
    S, n_items, rows, X, tg_ptr, tg_items = hand_case()
    for mode in (SPARSE, DENSE):
        for filt in (False, True):
            for r in (rows, None):
                a = host_model(S, n_items, r, X, filt, mode, tg_ptr, tg_items)
                assert_same(host_model_vectorised(S, n_items, r, X, filt, mode, tg_ptr, tg_items), a, f"mode={mode} filter={filt}")
    X2, users, S2 = golden_block(np.float32)
    rng = np.random.default_rng(3)
    n = rng.integers(0, 9, len(users))
    tg_ptr = np.r_[0, np.cumsum(n)].astype(np.int64)
    tg_items = rng.integers(-2, 403, int(n.sum())).astype(np.int32)
    for mode in (SPARSE, DENSE):
        a = host_model(S2, 400, users, X2, True, mode, tg_ptr, tg_items)
        assert_same(host_model_vectorised(S2, 400, users, X2, True, mode, tg_ptr, tg_items), a, f"fixture mode={mode}")
        assert (a[0] >= 0).sum() > 100 and (a[0] == -1).sum() > 10


@pytest.mark.parametrize("w", ["f32", "f64"])
def test_the_item_the_reference_lists_at_position_p_has_p_items_above(w):
    """All eight recorded variants: 2,400 of 2,400 positions each.  The fixture holds no tie and no negative score among its
    competing pairs (82,790 for f32 / sparse / filter), so `tied` and the sign handling are left to the hand-written rows."""
    X, users, S = golden_block(np.float32 if w == "f32" else np.float64)
    zs = golden_scoring()
    tg_ptr = np.arange(241, dtype=np.int64) * 10
    for mode, mname in ((SPARSE, "sparse"), (DENSE, "dense")):
        for filt in (True, False):
            ids = zs[f"ids_{w}_{mname}_{'filter' if filt else 'nofilter'}"]
            assert ids.shape == (240, 10) and (ids >= 0).all()
            above, tied, score, competing = host_model_vectorised(S, 400, users, X, filt, mode, tg_ptr, ids.ravel())
            assert np.array_equal(above.reshape(240, 10), np.tile(np.arange(10), (240, 1))), (w, mname, filt)
            assert (tied == 0).all() and (competing >= 10).all()
            assert np.array_equal(score.reshape(240, 10), np.take_along_axis(S, ids, axis=1).astype(np.float64))
    ptr, items = every_pair(240, 400)
    a, t, _, c = host_model_vectorised(S, 400, users, X, True, SPARSE, ptr, items)
    if w == "f32":
        assert int(c.sum()) == 82790 == int((a >= 0).sum())
    live = a.reshape(240, 400) >= 0
    assert (t == 0).all() and not (S[live] < 0).any()
    # every competing item has a position of its own: the positions of a row are 0 .. competing - 1
    for r in range(240):
        assert np.array_equal(np.sort(a.reshape(240, 400)[r][live[r]]), np.arange(c[r]))


def test_hand_written_rows():
    S, n_items, rows, X, tg_ptr, tg_items = hand_case()
    inf = np.inf
    for model in (host_model, host_model_vectorised):
        out = {(m, f): model(S, n_items, rows, X, f, m, tg_ptr, tg_items) for m in (SPARSE, DENSE) for f in (False, True)}
        row = lambda res, r: [x[tg_ptr[r]:tg_ptr[r + 1]].tolist() for x in res[:3]]
        # A: targets 0, 2, 3 (score 3, a three-way tie below the 5), 1 and 6 (score 1, a pair), 7 (the best), 4 (a zero), 5 (-2)
        a, t, s = row(out[SPARSE, True], 0)
        assert a == [1, 1, 1, 4, 4, 0, -1, 6] and t == [2, 2, 2, 1, 1, 0, 0, 0] and s == [3, 3, 3, 1, 1, 5, 0, -2]
        a, t, _ = row(out[DENSE, True], 0)
        assert a == [1, 1, 1, 4, 4, 0, 6, 7] and t == [2, 2, 2, 1, 1, 0, 0, 0]
        assert out[SPARSE, True][3][0] == 7 and out[DENSE, True][3][0] == 8
        # B: targets 0 (+0), 1 (-0), 2 (-1), 3 (2), 6 (-3), 7 (-1)
        a, t, s = row(out[SPARSE, False], 1)
        assert a == [-1, -1, 1, 0, 3, 1] and t == [0, 0, 1, 0, 0, 1]
        assert np.signbit(s[1]) and not np.signbit(s[0]) and s[:2] == [0.0, 0.0]          # the score keeps its sign bit
        a, t, _ = row(out[DENSE, False], 1)
        assert a == [1, 1, 5, 0, 7, 5] and t == [3, 3, 1, 0, 0, 1]                          # +0 ties with -0; a zero outranks -1
        assert out[SPARSE, False][3][1] == 4 and out[DENSE, False][3][1] == 8
        # C: targets 0 (NaN), 1 (inf), 2 (-inf), 3 (1), 4 (inf)
        a, t, s = row(out[SPARSE, False], 2)
        assert a == [-1, 0, 4, 3, 0] and t == [0, 1, 0, 0, 1] and math.isnan(s[0]) and s[1:] == [inf, -inf, 1, inf]
        a, t, _ = row(out[DENSE, False], 2)
        assert a == [-1, 0, 5, 3, 0] and t == [0, 1, 0, 0, 1]
        assert out[SPARSE, False][3][2] == 5 and out[DENSE, False][3][2] == 6
        # D: own = {1, 5}; targets 1 (in own), 0, 4 twice, -1 and 8 (out of range), 2
        a, t, s = row(out[SPARSE, True], 3)
        assert a == [-1, 2, 5, 5, -1, -1, 3] and t == [0] * 7 and s == [4, 5, 1, 1, -inf, -inf, 3]
        a, t, _ = row(out[SPARSE, False], 3)
        assert a == [4, 3, 7, 7, -1, -1, 5] and t == [0] * 7
        assert out[SPARSE, True][3][3] == 6 and out[SPARSE, False][3][3] == 8
        # E: no targets; a stored explicit zero is in own whatever its value
        assert tg_ptr[4] == tg_ptr[5]
        assert [out[k][3][4] for k in ((SPARSE, True), (SPARSE, False), (DENSE, True), (DENSE, False))] == [2, 3, 7, 8]
        # F, G: a row id outside X has no own
        for r in (5, 6):
            assert out[DENSE, True][3][r] == 8 and out[SPARSE, True][3][r] == 2
        assert row(out[SPARSE, True], 5)[0] == [1] and row(out[SPARSE, True], 6)[0] == [0, 1]


# ---------------------------------------------------------------------------------------------- the summary
def test_summary_on_hand_computed_users():
    from rtrec_amd.utils.metrics import catalogue_rank_summary
    # user 0 "perfect": 2 targets at ranks 0 and 1 of 10 competing.  user 1 "reversed": 2 targets at the last two ranks of 10.
    # user 2 "all tied": 2 targets and 3 negatives, all with one score.  user 3: one listed target (rank 3 of 6 competing) and
    # one never listed.  user 4: its 2 targets are everything that competes (no negative: no auc).  user 5: no target (skipped)
    tg_ptr = np.array([0, 2, 4, 6, 8, 10, 10])
    above = np.array([0, 1, 8, 9, 0, 0, 3, -1, 0, 1])
    tied = np.array([0, 0, 0, 0, 4, 4, 0, 0, 0, 0])
    score = np.array([9.0, 8.0, 0.2, 0.1, 1.0, 1.0, 4.0, 0.0, 2.0, 1.0])
    competing = np.array([10, 10, 5, 6, 2, 77])
    out, cols = catalogue_rank_summary(tg_ptr, above, tied, score, competing, ks=(1, 2, 5), unknown_items=3, skipped_users=1)
    assert out["n_users"] == 5 and out["n_targets"] == 10 and out["skipped_users"] == 2 and out["unknown_items"] == 3
    assert out["never_listed"] == 1 and out["tied_targets"] == 2 and out["auc_users"] == 4
    auc = cols["auc"].tolist()
    assert auc[:3] == [1.0, 0.0, 0.5] and auc[3] == (5 - 3) / (2 * 5) and math.isnan(auc[4])
    assert out["auc"] == math.fsum([1.0, 0.0, 0.5, 0.2]) / 4
    # percentile ranks: 0, 0 | 1, 1 | .5, .5 | 3/5, 1 (never listed) | 0, 0 (listed, no negative)
    assert out["mean_percentile_rank"] == math.fsum([0, 0, 1, 1, .5, .5, .6, 1, 0, 0]) / 10
    assert cols["mean_percentile_rank"].tolist() == [0.0, 1.0, 0.5, 0.8, 0.0]
    # pessimistic ranks: 0, 1 | 8, 9 | 4, 4 | 3, never | 0, 1
    assert cols["best_rank"].tolist() == [0, 8, 4, 3, 0] and cols["never_listed"].tolist() == [0, 0, 0, 1, 0]
    assert cols["mrr"].tolist() == [1.0, 1 / 9, 1 / 5, 1 / 4, 1.0] and out["mrr"] == math.fsum(cols["mrr"].tolist()) / 5
    assert cols["recall@1"].tolist() == [0.5, 0, 0, 0, 0.5] and cols["recall@2"].tolist() == [1, 0, 0, 0, 1]
    assert cols["recall@5"].tolist() == [1, 0, 1, 0.5, 1] and cols["hit_rate@5"].tolist() == [1, 0, 1, 1, 1]
    d = lambda rank: 1.0 / math.log2(rank + 2)
    assert cols["ndcg@5"].tolist() == [1.0, 0.0, (d(4) + d(4)) / (d(0) + d(1)), d(3) / (d(0) + d(1)), 1.0]
    assert cols["ndcg@1"].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]
    assert out["recall@5"] == math.fsum([1, 0, 1, 0.5, 1]) / 5 and out["hit_rate@1"] == 2 / 5
    assert list(out)[:9] == ["recall@1", "hit_rate@1", "ndcg@1", "recall@2", "hit_rate@2", "ndcg@2", "recall@5", "hit_rate@5", "ndcg@5"]
    # a listed positive above another listed positive is no negative: 3 targets at above 0, 1, 2 of 4 competing -> auc 1
    out, cols = catalogue_rank_summary([0, 3], [0, 1, 2], [0, 0, 0], [3.0, 2.0, 1.0], [4], ks=(1,))
    assert cols["auc"].tolist() == [1.0] and out["mean_percentile_rank"] == 0.0
    # ... and one tied with another listed positive is no tied negative: both above the single negative
    out, cols = catalogue_rank_summary([0, 2], [0, 0], [1, 1], [2.0, 2.0], [3], ks=(1,))
    assert cols["auc"].tolist() == [1.0] and cols["best_rank"].tolist() == [1] and out["tied_targets"] == 2
    # nothing at all
    out, cols = catalogue_rank_summary([0], [], [], [], [], ks=(1,))
    assert out["n_users"] == 0 and math.isnan(out["auc"]) and math.isnan(out["recall@1"]) and len(cols["auc"]) == 0
    with pytest.raises(ValueError, match="at least 1"):
        catalogue_rank_summary([0], [], [], [], [], ks=(0,))


# ---------------------------------------------------------------------------------------------- the layers, on the stand-in
@pytest.mark.parametrize("strings", [False, True])
def test_rank_items_batch_is_the_position_in_recommend(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    known_users = sorted({u for u, _, _, _ in batch}, key=str)
    known_items = sorted({i for _, i, _, _ in batch}, key=str)
    unknown_item = "never seen" if strings else 10 ** 7
    cold = "nobody" if strings else max(known_users) + 1000
    users = known_users[:25] + [cold, known_users[3]]
    lists = [known_items + [unknown_item] for _ in users]
    lists[-1] = [known_items[5], unknown_item, known_items[5], known_items[0]]
    for filt in (True, False):
        got = m.rank_items_batch(users, lists, filter_interacted=filt)
        full = [m.recommend(u, top_k=len(known_items), filter_interacted=filt) for u in users]
        for b, u in enumerate(users):
            g = got[b]
            assert g["items"] == lists[b] and len(g["above"]) == len(g["tied"]) == len(g["score"]) == len(lists[b])
            if u == cold:
                assert g["competing"] == 0 and set(g["above"]) == {-1} and set(g["tied"]) == {0} and set(g["score"]) == {-np.inf}
                continue
            assert g["above"][lists[b].index(unknown_item)] == -1 and g["score"][lists[b].index(unknown_item)] == -np.inf
            if b == len(users) - 1:
                assert g["above"][0] == g["above"][2] and g["score"][0] == g["score"][2]
                continue
            assert g["competing"] == len(full[b])
            for p, item in enumerate(full[b]):                             # the list `recommend` gives IS the ranking
                q = lists[b].index(item)
                assert g["above"][q] <= p <= g["above"][q] + g["tied"][q] and math.isfinite(g["score"][q])
            listed = set(full[b])
            assert all((g["above"][q] >= 0) == (item in listed) for q, item in enumerate(lists[b]))
    assert sum(len(f) for f in full) > 100
    one = m.rank_items(users[0], lists[0], filter_interacted=False)
    assert one == got[0] and Recommender(m).rank_items(users[0], lists[0], filter_interacted=False) == one
    assert Recommender(m).rank_items_batch(users, lists, filter_interacted=False) == got
    ptr, above, tied, score, competing = m.rank_items_batch(users, lists, filter_interacted=False, as_arrays=True)
    assert ptr.tolist() == np.r_[0, np.cumsum([len(c) for c in lists])].tolist() and above.dtype == tied.dtype == competing.dtype == np.int32
    assert above.tolist() == [a for g in got for a in g["above"]] and competing.tolist() == [g["competing"] for g in got]
    assert score.dtype == np.float64 and m.rank_items_batch([], []) == []
    with pytest.raises(ValueError, match="one list per user"):
        m.rank_items_batch(users, lists[:-1])


def test_several_passes_equal_one_and_unservable_weights_are_refused():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    fresh = cpu_slim()
    with pytest.raises(RuntimeError, match="Model must be fitted"):
        fresh.rank_items_batch([1], [[1]])
    m, batch = _model()
    eng = m.model.engine
    known_items = sorted({i for _, i, _, _ in batch})
    m.rank_items(batch[0][0], known_items[:3])                              # (syncs W and X into the engine)
    rng = np.random.default_rng(12)
    rows = np.r_[rng.permutation(eng.n_users)[:40], -1, eng.n_users + 5, 0, 0]
    n = rng.integers(0, 7, len(rows))
    ptr = np.r_[0, np.cumsum(n)].astype(np.int64)
    tg = rng.integers(-1, m.model.n_items_fitted + 2, int(n.sum()))
    for mode in (SPARSE, DENSE):
        one = eng.catalogue_ranks_rows(rows, ptr, tg, True, mode)
        assert (one[0] >= 0).any() and (one[0] == -1).any() and one[3].max() > 0
        for block_bytes in (1, 4 * m.model.n_items_fitted * 3, 4 * m.model.n_items_fitted * 43):    # 1, 3 and 43 rows a pass
            assert_same(eng.catalogue_ranks_rows(rows, ptr, tg, True, mode, block_bytes=block_bytes), one, f"block_bytes={block_bytes}")
    assert eng.catalogue_ranks_rows([], [0], [])[3].shape == (0,)
    for bad_ptr in ([0, 1], np.r_[1, ptr[1:]], np.r_[ptr[:-1], ptr[-1] + 1], np.r_[0, 5, 2, ptr[3:]]):
        with pytest.raises(ValueError, match="targets_ptr"):
            eng.catalogue_ranks_rows(rows, bad_ptr, tg)
    with pytest.raises(ValueError, match="mode"):
        eng.catalogue_ranks_rows(rows, ptr, tg, True, 2)
    # a float64 W is served from its float64 scores, one whose values are no float32 numbers included
    W = m.model.item_similarity
    users = sorted({u for u, _, _, _ in batch})[:6]
    want = m.rank_items_batch(users, [known_items] * 6)
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    got = m.rank_items_batch(users, [known_items] * 6)
    assert [g["above"] for g in got] == [g["above"] for g in want] and [g["competing"] for g in got] == [g["competing"] for g in want]
    m.model.item_similarity = W
    # a column-sharded W: the error names the way out
    eng2 = SlimEngine(backend=RanksOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng2.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng2.set_weights(dw)
    with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
        eng2.catalogue_ranks_rows([0], [0, 1], [1])


@pytest.mark.parametrize("score_shard", ["columns", "rows"])
def test_every_rank_that_holds_the_whole_w_counts_over_the_whole_catalogue(score_shard):
    """Two ranks, W replicated (shard_w off).  With column shards a rank's score layouts cover its own column block only; the
    rank call must still count over all columns: both ranks answer what a single rank answers, float32 and float64."""
    from rtrec_amd.engine import SlimEngine
    X, W, users, _, _ = golden()
    rng = np.random.default_rng(5)
    rows = np.r_[users[:30], -1, X.shape[0] + 3]
    n = rng.integers(0, 6, len(rows))
    ptr = np.r_[0, np.cumsum(n)].astype(np.int64)
    tg = rng.integers(-1, 402, int(n.sum()))
    for dtype in (np.float32, np.float64):
        Wd = sp.csc_matrix(W, dtype=dtype)
        want = {}
        for world, rank in ((1, 0), (2, 0), (2, 1)):
            eng = SlimEngine(backend=RanksOracleBackend(), rank=rank, world_size=world, score_shard=score_shard, shard_w=False)
            eng.set_weights(Wd)
            eng.set_interactions(None, X, need_csc=False)
            assert world == 1 or score_shard == "rows" or eng._W["col_hi"] - eng._W["col_lo"] == 200
            for mode in (SPARSE, DENSE):
                got = eng.catalogue_ranks_rows(rows, ptr, tg, True, mode, block_bytes=7 * 400 * 4)
                if world == 1:
                    want[mode] = got
                    S = np.asarray((X[users[:30]].astype(dtype) @ Wd.tocsr()).toarray())
                    S = np.vstack([S, np.zeros((2, 400), dtype)])
                    assert_same(got, host_model_vectorised(S, 400, rows, X, True, mode, ptr, tg), f"one rank {dtype.__name__} mode={mode}")
                    assert (got[0] > 200).any() and got[3][:30].min() > 10
                else:
                    assert_same(got, want[mode], f"rank {rank} of 2, {score_shard}, {dtype.__name__}, mode={mode}")


def test_evaluate_catalogue_agrees_with_evaluate_inside_the_list():
    import pandas as pd
    from rtrec_amd.recommender import Recommender
    from rtrec_amd.utils.metrics import catalogue_rank_summary
    m, batch = _model()
    rec = Recommender(m)
    known_users = sorted({u for u, _, _, _ in batch})
    known_items = sorted({i for _, i, _, _ in batch})
    rng = np.random.default_rng(21)
    pairs = []
    for u in known_users:                                                   # held out: some of what the user would be shown, some not
        shown = m.recommend(u, top_k=12)
        mine = set(rng.permutation(shown)[:int(rng.integers(0, 4))].tolist()) | set(rng.permutation(known_items)[:int(rng.integers(1, 4))].tolist())
        pairs += [(u, i) for i in sorted(mine)]
    frame = pd.DataFrame(pairs, columns=["user", "item"]).sample(frac=1.0, random_state=4)
    assert len(known_users) <= 240 and not frame.duplicated().any()
    out, per_user = rec.evaluate_catalogue(frame, ks=(1, 5, 10), per_user=True)
    assert out["n_users"] == len(known_users) == len(per_user) and out["n_targets"] == len(frame) and out["unknown_items"] == 0
    assert out["skipped_users"] == 0 and per_user.index.tolist() == known_users and per_user.index.name == "user"
    hits = 0
    for k in (1, 5, 10):
        ref = rec.evaluate(frame, recommend_size=k)
        for name in ("recall", "hit_rate", "ndcg"):
            assert abs(out[f"{name}@{k}"] - ref[name]) <= 1e-12, (name, k, out[f"{name}@{k}"], ref[name])
        hits += ref["tp"]
    assert hits > 50 and 0.0 < out["recall@1"] < out["recall@10"] < 1.0
    assert 0.5 < out["auc"] <= 1.0 and 0.0 <= out["mean_percentile_rank"] < 0.5 and out["mrr"] > 0.0
    assert rec.evaluate_catalogue(frame, ks=(1, 5, 10)) == out
    # the same figures from the ranks themselves
    users = per_user.index.tolist()
    lists = [sorted(frame.loc[frame["user"] == u, "item"].tolist()) for u in users]
    ptr, above, tied, score, competing = m.rank_items_batch(users, lists, as_arrays=True)
    assert catalogue_rank_summary(ptr, above, tied, score, competing, ks=(1, 5, 10))[0] == out
    # unknown items are dropped and counted, unknown users and users left without a target skipped and counted, duplicates merged
    extra = pd.DataFrame([(known_users[0], 10 ** 7), (10 ** 6, known_items[0]), (10 ** 6 + 1, 10 ** 7), pairs[0], pairs[0]],
                         columns=["user", "item"])
    out2 = rec.evaluate_catalogue(pd.concat([frame, extra]), ks=(1, 5, 10))
    assert out2["unknown_items"] == 2 and out2["skipped_users"] == 2
    assert {k: v for k, v in out2.items() if k not in ("unknown_items", "skipped_users")} == \
           {k: v for k, v in out.items() if k not in ("unknown_items", "skipped_users")}
    nothing = rec.evaluate_catalogue(frame.iloc[:0], ks=(3,))
    assert nothing["n_users"] == 0 and math.isnan(nothing["recall@3"])


# ---------------------------------------------------------------------------------------------- serving
def test_rank_items_route_token_payload_and_failure():
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
    r = client.post("/rank_items", json={"user": user, "items": items}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/rank_items", json={"user": user, "items": items}, headers=ok)
    want = m.rank_items(user, items)
    assert r.status_code == 200 and want["above"][-1] == -1 and max(want["above"]) > 0
    assert r.json() == {"user": user, "competing": want["competing"],
                        "items": [{"item": i, "above": a, "tied": t, "score": s if math.isfinite(s) else None}
                                  for i, a, t, s in zip(items, want["above"], want["tied"], want["score"])]}
    assert r.json()["items"][-1]["score"] is None
    r = client.post("/rank_items", json={"user": user, "items": items, "filter_interacted": False}, headers=ok)
    assert [e["above"] for e in r.json()["items"]] == m.rank_items(user, items, filter_interacted=False)["above"] != want["above"]
    assert client.post("/rank_items", json={"user": user}, headers=ok).status_code == 422       # items are required
    unfitted = FastAPI()
    unfitted.include_router(build_router(ModelGate(cpu_slim())))
    r = TestClient(unfitted).post("/rank_items", json={"user": user, "items": items}, headers=ok)   # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Rank items failed"}
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)                 # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(user, top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def test_catalogue_ranks_is_registered_declared_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    assert "catalogue_ranks" in ops.EXT_OPS and ops.EXT_EXPORT_OF["catalogue_ranks"] == "rtrec_slim_catalogue_ranks"
    assert "catalogue_ranks" not in ops.OPS and "rtrec_slim_catalogue_ranks" not in _native.EXPORTS
    assert "rtrec_slim_catalogue_ranks" in _native.EXT_EXPORTS and "catalogue_ranks.hip" in build.SOURCES
    schema = str(torch.ops.rtrec_amd.catalogue_ranks.default._schema)
    for name in ("above", "tied", "score", "competing"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("scores", "xb_ptr", "xb_col", "tg_ptr", "tg_items"):
        assert f"Tensor {name}" in schema, schema
    assert "Tensor? row_ids" in schema and "int mode" in schema and "bool filter_interacted" in schema
    ext = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    core = open(os.path.join(ROOT, "include", "rtrec_amd.h")).read()
    assert re.search(r"\bint rtrec_slim_catalogue_ranks\s*\(", ext) and "rtrec_slim_catalogue_ranks" not in core
    assert "catalogue_ranks_kernel" in open(os.path.join(ROOT, "rtrec_amd", "csrc", "catalogue_ranks.hip")).read()
    fn = _native.load().rtrec_slim_catalogue_ranks
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_rows=1, n_items=5, scores=one, stride=5, f64=0, n_x=3, nnz=4, filt=1, mode=0, tg_ptr=one, n_tg=2, above=one, comp=one, xb=one: (
        n_rows, n_items, scores, stride, f64, None, xb, xb, n_x, nnz, filt, mode, tg_ptr, one, n_tg, above, one, one, comp, None)
    for kw in (dict(mode=2), dict(mode=-1), dict(mode=3, n_rows=0)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_rows=-1), dict(n_items=-1), dict(nnz=-1), dict(n_x=-1), dict(n_tg=-1), dict(stride=4), dict(scores=None),
               dict(tg_ptr=None), dict(above=None), dict(comp=None), dict(xb=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, scores=None, tg_ptr=None, comp=None)) == 0
    for name in ("catalogue_ranks_device", "catalogue_ranks_rows"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "catalogue_ranks"))
    if not torch.cuda.is_available():
        with pytest.raises((NotImplementedError, RuntimeError)):
            i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
            torch.ops.rtrec_amd.catalogue_ranks(torch.zeros(1, 4), 4, None, i32(2), i32(1), True, 0, torch.zeros(2, dtype=torch.int64), i32(1),
                                                i32(1), i32(1), torch.zeros(1, dtype=torch.float64), i32(1))
