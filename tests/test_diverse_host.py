"""Diversified lists (SLIM.recommend_diverse_batch / diversify_batch, csrc/diversify.hip) without a GPU: the definition as a
plain-Python host model and a vectorised one, their properties on the golden fixture, hand-written cases; the model / facade /
serving layers end to end through the CPU stand-in backend with `diversify_lists` supplied by the host model; the rules of the
extension surface (include/rtrec_amd_ext.h) and the C entry point's host-side checks.  The kernel is in tests/test_gpu_diverse.py.

The definition (include/rtrec_amd_ext.h, "DIVERSIFIED LISTS"): a position competes when it lies below counts[r], its id lies
in [0, n_items), its score is finite and no chosen position holds its item; sim(a, b) = fmax(|W[a, b]|, |W[b, a]|); every step
takes the largest v = fl(fl(lambda * score) - fl((1 - lambda) * pen)), the earlier position among == values, skipping NaN values;
afterwards pen = fmax(pen, sim(item, winner)) for every other competing position."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_explain_host import bits, golden
from tests.test_rerank_host import PairsOracleBackend, _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---------------------------------------------------------------------------------------------- the host models
def host_model(W, ids, scores, counts, keep, lam, ties=None):
    """THE DEFINITION, written for clarity: (order[B, keep] int32, value[B, keep] float32, penalty[B, keep] float32, count[B]
    int32); W csc with sorted, distinct rows per column.  `ties` (a list) collects (row, step) of every step whose best value
    is shared by two competing positions."""
    ids, scores = np.asarray(ids), np.asarray(scores, dtype=F32)
    B, k = ids.shape
    I = W.shape[1]
    lam = F32(lam)
    oml = F32(F32(1.0) - lam)
    stored = {(int(j), int(i)): F32(v) for i in range(I) for j, v in zip(W.indices[W.indptr[i]:W.indptr[i + 1]],
                                                                          W.data[W.indptr[i]:W.indptr[i + 1]])}

    def sim(a, b):
        return np.fmax(np.abs(stored.get((a, b), F32(0.0))), np.abs(stored.get((b, a), F32(0.0))))

    order = np.full((B, keep), -1, np.int32)
    value = np.full((B, keep), -np.inf, F32)
    penalty = np.full((B, keep), -np.inf, F32)
    count = np.zeros(B, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            alive = [p for p in range(min(max(int(counts[b]), 0), k)) if 0 <= ids[b, p] < I and np.isfinite(scores[b, p])]
            pen = {p: F32(0.0) for p in alive}
            for t in range(keep):
                best, best_v, shared = None, None, False
                for p in alive:                                              # ascending: > keeps the earlier position
                    v = F32(F32(lam * scores[b, p]) - F32(oml * pen[p]))
                    if np.isnan(v):
                        continue
                    if best is None or v > best_v:
                        best, best_v, shared = p, v, False
                    elif v == best_v:
                        shared = True
                if best is None:
                    break
                if shared and ties is not None:
                    ties.append((b, t))
                order[b, t], value[b, t], penalty[b, t], count[b] = best, best_v, pen[best], t + 1
                c = int(ids[b, best])
                alive = [p for p in alive if ids[b, p] != c]                 # the winner and its duplicates leave
                for p in alive:
                    pen[p] = np.fmax(pen[p], sim(int(ids[b, p]), c))
    return order, value, penalty, count


def host_model_vectorised(W, ids, scores, counts, keep, lam):
    """The same function with numpy over rows and positions, the similarities looked up in one sparse matrix: what the larger
    GPU cases and tools/diverse_bench.py compare against."""
    ids, scores, counts = np.asarray(ids), np.asarray(scores, dtype=F32), np.asarray(counts)
    B, k = ids.shape
    I = W.shape[1]
    lam = F32(lam)
    oml = F32(F32(1.0) - lam)
    A = sp.csr_matrix(abs(sp.csc_matrix(W, dtype=F32)))
    A.data[np.isnan(A.data)] = 0.0                                           # fmax ignores a NaN weight: it counts like none (|w| >= 0)
    S = A.maximum(A.T).tocsr()
    S.sort_indices()
    alive = (np.arange(k)[None, :] < counts[:, None]) & (ids >= 0) & (ids < I) & np.isfinite(scores)
    safe = np.where(alive, ids, 0)
    pen = np.zeros((B, k), F32)
    order = np.full((B, keep), -1, np.int32)
    value = np.full((B, keep), -np.inf, F32)
    penalty = np.full((B, keep), -np.inf, F32)
    count = np.zeros(B, np.int32)
    rows = np.arange(B)
    with np.errstate(invalid="ignore", over="ignore"):
        ls = (lam * scores).astype(F32)
        for t in range(keep):
            v = (ls - (oml * pen).astype(F32)).astype(F32)
            valid = alive & ~np.isnan(v)
            top = np.where(valid, v, -np.inf).max(axis=1) if k else np.zeros(B, F32)
            cand = valid & (v == top[:, None])
            has = cand.any(axis=1)
            if not has.any():
                break
            c = cand.argmax(axis=1)                                          # the first of the == values
            r = rows[has]
            order[r, t], value[r, t], penalty[r, t] = c[has], v[r, c[has]], pen[r, c[has]]
            count[r] = t + 1
            idc = safe[rows, c]
            alive &= ~(has[:, None] & (ids == idc[:, None]))
            alive &= has[:, None]                                            # a list that has ended stays ended
            sim = np.asarray(S[safe, np.broadcast_to(idc[:, None], safe.shape)].todense(), dtype=F32).reshape(B, k)
            pen = np.where(alive, np.fmax(pen, sim), pen)
    return order, value, penalty, count


def assert_same(got, want, what=""):
    for name, g, w in zip(("order", "value", "penalty", "count"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the host model {w.shape}"
        bad = np.flatnonzero((bits(g) != bits(w)).ravel() if name in ("value", "penalty") else (g != w).ravel())
        assert bad.size == 0, f"{what}: {bad.size} {name} differ from the host model, first at flat index {int(bad[0])}: {g.ravel()[bad[0]]} != {w.ravel()[bad[0]]}"


_POOLS = {}


def fixture_pools(pool=50):
    """(W, ids[240, pool] int32, scores[240, pool] float32, counts[240], the reference's top-10 ids): per fixture user the
    `pool` best items of the float32 dense product, interacted and zero scores removed, best first.  Computed once."""
    if pool not in _POOLS:
        X, W, users, ref_ids, ref_scores = golden()
        S = (X[users].astype(F32) @ sp.csc_matrix(W, dtype=F32)).toarray().astype(F32)
        S[X[users].toarray() != 0] = 0.0
        ids = np.full((len(users), pool), -1, np.int32)
        scores = np.zeros((len(users), pool), F32)
        counts = np.zeros(len(users), np.int32)
        for b in range(len(users)):
            nz = np.flatnonzero(S[b])
            best = nz[np.lexsort((-nz, -S[b, nz]))][:pool]                   # score descending, the higher id first (DESIGN D1)
            ids[b, :len(best)], scores[b, :len(best)], counts[b] = best, S[b, best], len(best)
        for a in (ids, scores, counts):
            a.setflags(write=False)
        _POOLS[pool] = (W, ids, scores, counts, ref_ids, ref_scores)
    return _POOLS[pool]


def csc_of(entries, n):
    """W[j, i] = v for every ((j, i), v) of `entries`, as a float32 CSC with sorted rows (explicit zeros, inf and NaN kept)."""
    keys = sorted(entries, key=lambda ji: (ji[1], ji[0]))
    ptr = np.zeros(n + 1, np.int32)
    for _, i in keys:
        ptr[i + 1] += 1
    return sp.csc_matrix((np.array([entries[ji] for ji in keys], F32), np.array([j for j, _ in keys], np.int32), np.cumsum(ptr).astype(np.int32)),
                         shape=(n, n))


def hand_cases():
    """(name, W, ids, scores, counts, keep, lam, order, value, penalty, count) of the hand-written cases; None = not pinned."""
    inf, nan = float("inf"), float("nan")
    # sim(0, 1) = 2 stored only as W[0, 1]; sim(0, 2) = 1 only as W[2, 0]; sim(0, 3) = 3: W[0, 3] = 0.25 against W[3, 0] = -3 (both sides,
    # the negative one larger in magnitude); sim(2, 3) = 0.125; W[5, 0] = inf; W[4, 0] = NaN against W[0, 4] = 0.5; items 6, 7 unlinked
    W = csc_of({(0, 1): 2.0, (2, 0): 1.0, (0, 3): 0.25, (3, 0): -3.0, (2, 3): 0.125, (5, 0): inf, (4, 0): nan, (0, 4): 0.5}, 8)
    i32 = lambda *rows: np.array(rows, np.int32)
    f32 = lambda *rows: np.array(rows, F32)
    return [
        # lambda 0.5: v = s / 2 - pen / 2.  Step 1: positions 1 and 2 tie at 3.5 exactly -> the lower position
        ("asymmetry, sign and an exact tie", W, i32([0, 1, 2, 3, 6]), f32([10, 9, 8, 9.5, 2]), [5], 5, 0.5,
         [[0, 1, 2, 3, 4]], [[5.0, 3.5, 3.5, 3.25, 1.0]], [[0.0, 2.0, 1.0, 3.0, 0.0]], [5]),
        ("the NaN weight is ignored, the other side counts", W, i32([0, 4, 6]), f32([4, 3, 2.25]), [3], 3, 0.5,
         [[0, 1, 2]], [[2.0, 1.25, 1.125]], [[0.0, 0.5, 0.0]], [3]),
        # lambda 0: v = 0 * s - pen: step 0 is all zeros (-0.0 for the negative score: it ties with +0.0 and is earlier)
        ("lambda 0: position 0, then by penalty only", W, i32([0, 1, 2, 3]), f32([-1, 5, 7, 9]), [4], 4, 0.0,
         [[0, 2, 1, 3]], [[-0.0, -1.0, -2.0, -3.0]], [[0.0, 1.0, 2.0, 3.0]], [4]),
        ("-0.0 against +0.0 is a tie", W, i32([6, 7], [7, 6]), f32([-1, 1], [1, -1]), [2, 2], 2, 0.0,
         [[0, 1], [0, 1]], [[-0.0, 0.0], [0.0, -0.0]], [[0.0, 0.0], [0.0, 0.0]], [2, 2]),
        ("duplicated ids are shown once", W, i32([0, 0, 6, 6, 0]), f32([3, 2.5, 2, 1, 0.5]), [5], 4, 0.75,
         [[0, 2, -1, -1]], [[2.25, 1.5, -inf, -inf]], [[0.0, 0.0, -inf, -inf]], [2]),
        # lambda 1: oml = 0, 0 * inf = NaN: item 5 is skipped in every step after item 0 is chosen, and the list ends short
        ("an inf weight with lambda 1 ends the list short", W, i32([0, 5, 6]), f32([3, 2, 1]), [3], 3, 1.0,
         [[0, 2, -1]], [[3.0, 1.0, -inf]], [[0.0, 0.0, -inf]], [2]),
        ("an inf weight with lambda 0.5 is a -inf value that still competes", W, i32([0, 5, 6]), f32([3, 2, 1]), [3], 3, 0.5,
         [[0, 2, 1]], [[1.5, 0.5, -inf]], [[0.0, 0.0, inf]], [3]),
        ("non-finite scores, foreign ids and counts", W, i32([0, 1, 2, 6, 8, -1, 7], [0, 1, 2, 3, 6, 7, 7]), f32([inf, nan, -inf, 1, 9, 9, 0.5], [7, 6, 5, 4, 3, 2, 1]),
         [7, 0], 3, 0.5, [[3, 6, -1], [-1, -1, -1]], [[0.5, 0.25, -inf], [-inf] * 3], [[0.0, 0.0, -inf], [-inf] * 3], [2, 0]),
    ]


class DiverseOracleBackend(PairsOracleBackend):
    """The CPU stand-in (tests.cpu_backend.OracleBackend, with score_pairs from the rerank host model) plus diversify_lists
    from the host model (TEST-ONLY, like its bases)."""

    def diversify_lists(self, n_items, W, ids, scores, counts, list_k, keep, lam, order, value, penalty, count, waves_per_row=0):
        import torch
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        out = host_model_vectorised(Wc, ids.numpy()[:, :list_k], scores.numpy()[:, :list_k], counts.numpy(), keep, lam)
        for dst, src in zip((order, value, penalty, count), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=DiverseOracleBackend())
    return m


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


# ---------------------------------------------------------------------------------------------- the definition
def test_vectorised_model_is_the_definition_on_a_mutilated_fixture():
    W, ids, scores, counts, _, _ = fixture_pools()
    rng = np.random.default_rng(41)
    ids, scores = ids.copy(), scores.copy()
    ids[rng.random(ids.shape) < 0.05] = -1
    ids[3, 4], ids[7, 0] = W.shape[1], W.shape[1] + 7
    ids[:, 20] = ids[:, 2]                                               # duplicates, one of them in front
    ids[:, 1] = ids[:, 30]
    scores[rng.random(scores.shape) < 0.02] = np.nan
    scores[5, 0], scores[6, 3] = np.inf, -np.inf
    counts = rng.integers(-2, ids.shape[1] + 4, len(ids)).astype(np.int32)
    for lam in (1.0, 0.7, 0.0):
        for keep in (1, 10, 50):
            a = host_model(W, ids, scores, counts, keep, F32(lam))
            assert_same(host_model_vectorised(W, ids, scores, counts, keep, F32(lam)), a, f"lambda={lam} keep={keep}")
    assert a[3].min() == 0 and a[3].max() > 30 and (a[0] >= 0).sum() == a[3].sum()


def test_lambda_one_is_the_identity_and_the_reference_top10():
    W, ids, scores, counts, ref_ids, ref_scores = fixture_pools()
    assert ids.shape == (240, 50) and (counts >= 11).all()
    for model in (host_model, host_model_vectorised):
        order, value, pen, count = model(W, ids, scores, counts, 10, F32(1.0))
        assert (count == 10).all() and (order == np.arange(10)[None, :]).all()
        assert np.array_equal(np.take_along_axis(ids, order, axis=1), ref_ids)
        assert np.array_equal(bits(value), bits(ref_scores.astype(F32))) and np.array_equal(bits(value), bits(scores[:, :10]))


def test_diversity_changes_most_fixture_lists_without_a_single_tie():
    W, ids, scores, counts, _, _ = fixture_pools()
    changed = {}
    for lam in (1.0, 0.7, 0.5, 0.3):
        ties = []
        order, value, pen, count = host_model(W, ids, scores, counts, 10, F32(lam), ties=ties)
        assert ties == [], f"lambda={lam}: the tie rule decides steps {ties[:5]}"
        assert_same(host_model_vectorised(W, ids, scores, counts, 10, F32(lam)), (order, value, pen, count), f"lambda={lam}")
        changed[lam] = int((order != np.arange(10)[None, :]).any(axis=1).sum())
        assert (count == 10).all() and (order[:, 0] == 0).all() and not pen[:, 0].any()
        chosen = np.take_along_axis(ids, order, axis=1)
        assert all(len(set(row)) == 10 for row in chosen.tolist())             # duplicate-free subsets of the pools
        assert all(set(row) <= set(ids[b, :counts[b]].tolist()) for b, row in enumerate(chosen.tolist()))
        assert (pen >= 0).all() and (np.diff(value, axis=1) <= 0).all() if lam == 1.0 else (pen >= 0).all()
    assert changed[1.0] == 0 and changed[0.7] > 120 and changed[0.7] <= changed[0.5] <= changed[0.3] <= 240, changed


def test_the_second_choice_maximises_the_value_over_all_remaining_positions():
    W, ids, scores, counts, _, _ = fixture_pools()
    A = np.abs(W.toarray().astype(F32))
    for lam in (F32(0.7), F32(0.3)):
        oml = F32(F32(1.0) - lam)
        for model in (host_model, host_model_vectorised):
            order, value, pen, count = model(W, ids, scores, counts, 2, lam)
            for b in range(len(ids)):
                n, first = int(counts[b]), int(ids[b, 0])
                sim = np.maximum(A[ids[b, 1:n], first], A[first, ids[b, 1:n]])
                v = (lam * scores[b, 1:n]).astype(F32) - (oml * sim).astype(F32)
                assert order[b].tolist() == [0, 1 + int(np.argmax(v))] and bits(value[b, 1]) == bits(v.max())
                assert bits(pen[b, 1]) == bits(sim[int(np.argmax(v))])


def test_hand_written_cases():
    for name, W, ids, scores, counts, keep, lam, order, value, penalty, count in hand_cases():
        for model in (host_model, host_model_vectorised):
            got = model(W, ids, scores, counts, keep, F32(lam))
            assert_same(got, (np.array(order, np.int32), np.array(value, F32), np.array(penalty, F32), np.array(count, np.int32)), name)
    # the tie of the first case is a tie: the plain model reports it
    ties = []
    name, W, ids, scores, counts, keep, lam = hand_cases()[0][:7]
    host_model(W, ids, scores, counts, keep, F32(lam), ties=ties)
    assert (0, 1) in ties


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _expected(m, users, top_k, pool, diversity, filter_interacted=True):
    """recommend_diverse_batch from its parts: recommend_batch's pool, score_pairs' scores, the plain host model."""
    W = m.model.item_similarity.tocsc()
    W.sort_indices()
    out = []
    for u in users:
        items = m.recommend_batch([u], top_k=pool, filter_interacted=filter_interacted)[0]
        sc = m.score_pairs([u] * len(items), items)
        ids = np.array([[m.item_ids.get_id(i) for i in items]], np.int32).reshape(1, -1)
        keep = min(top_k, max(len(items), 1))
        if not len(items):
            out.append([])
            continue
        order, _, _, count = host_model(W, ids, sc[None, :], [len(items)], keep, F32(1.0 - diversity))
        out.append([(items[p], float(sc[p])) for p in order[0, :count[0]].tolist()])
    return out


@pytest.mark.parametrize("strings", [False, True])
def test_recommend_diverse_batch_end_to_end(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    known = sorted({u for u, _, _, _ in batch}, key=str)
    cold = "nobody" if strings else max(known) + 1000
    users = known[:25] + [cold, known[3], cold]
    hot = [b for b, u in enumerate(users) if u != cold]
    got = m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6, ret_scores=True)
    want = _expected(m, [users[b] for b in hot], 6, 30, 0.6)
    plain = m.recommend_batch(users, top_k=6)
    assert [got[b] for b in hot] == want
    assert sum([i for i, _ in got[b]] != plain[b] for b in hot) >= 3            # the stage is not cosmetic on this model either
    for b, u in enumerate(users):
        if u == cold:                                                        # the cold-start list, unchanged, without scores
            assert [i for i, _ in got[b]] == plain[b][:6] and not any(s for _, s in got[b]) and len(got[b]) > 0
    lists = m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6)
    assert lists == [[i for i, _ in row] for row in got]
    # diversity 0 is recommend_batch; filter_interacted reaches the scoring pass
    assert m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.0) == plain
    assert m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.0, filter_interacted=False) == m.recommend_batch(users, top_k=6, filter_interacted=False)
    assert [m.recommend_diverse_batch([users[b] for b in hot[:4]], top_k=3, pool=9, diversity=0.5, filter_interacted=False, ret_scores=True)[j]
            for j in range(4)] == _expected(m, [users[b] for b in hot[:4]], 3, 9, 0.5, filter_interacted=False)
    # as_arrays: rerank_batch's triple plus value and penalty
    ids, sc, cnt, val, pen = m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6, as_arrays=True)
    assert ids.shape == sc.shape == val.shape == pen.shape == (len(users), 6) and cnt.shape == (len(users),)
    lam, oml = F32(1.0 - 0.6), F32(F32(1.0) - F32(1.0 - 0.6))
    for b, row in enumerate(got):
        n = int(cnt[b])
        assert n == len(row) and (ids[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all()
        assert [m.item_ids.get(int(i)) for i in ids[b, :n]] == [i for i, _ in row]
        assert np.array_equal(bits(sc[b, :n]), bits([s for _, s in row]))
        if users[b] == cold:
            assert np.isneginf(val[b]).all() and np.isneginf(pen[b]).all()
        else:
            assert pen[b, 0] == 0 and (pen[b, :n] >= 0).all()
            assert np.array_equal(bits(val[b, :n]), bits((lam * sc[b, :n]).astype(F32) - (oml * pen[b, :n]).astype(F32)))
    # one user; the facade passes everything through
    assert m.recommend_diverse(users[2], top_k=6, pool=30, diversity=0.6) == lists[2]
    assert m.recommend_diverse(users[2], top_k=6, pool=30, diversity=0.6, ret_scores=True) == got[2]
    rec = Recommender(m)
    assert rec.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6) == lists
    assert rec.recommend_diverse(users[1], top_k=6, pool=30, diversity=0.6, ret_scores=True) == got[1]
    assert rec.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6, as_arrays=True)[2].tolist() == cnt.tolist()
    assert m.recommend_diverse_batch([], top_k=3, pool=5) == []


def test_diversify_batch_takes_raw_ids_and_needs_no_user():
    from rtrec_amd.recommender import Recommender
    for strings in (False, True):
        m, batch = _model(strings)
        W = m.model.item_similarity.tocsc()
        W.sort_indices()
        rng = np.random.default_rng(12)
        known = sorted({i for _, i, _, _ in batch}, key=str)
        unknown = "never seen" if strings else 10 ** 7
        items, scores = [], []
        for b in range(12):
            row = [known[j] for j in rng.permutation(len(known))[:int(rng.integers(1, 40))]]
            row.insert(int(rng.integers(0, len(row) + 1)), unknown)
            if b % 3 == 0:
                row.append(row[0])                                           # an item listed twice
            items.append(row)
            scores.append(np.sort(rng.random(len(row)).astype(F32))[::-1].tolist())
        items.append([]); scores.append([])
        k = max(len(r) for r in items)
        ids = np.full((len(items), k), -1, np.int32)
        sc = np.zeros((len(items), k), F32)
        for b, row in enumerate(items):
            ids[b, :len(row)] = [-1 if i == unknown else m.item_ids.get_id(i) for i in row]
            sc[b, :len(row)] = scores[b]
        want = host_model(W, ids, sc, [len(r) for r in items], 7, F32(1.0 - 0.45))
        got = m.diversify_batch(items, scores, top_k=7, diversity=0.45, as_arrays=True)
        assert_same(got, want, f"diversify_batch strings={strings}")
        pairs = m.diversify_batch(items, scores, top_k=7, diversity=0.45)
        for b, row in enumerate(pairs):
            assert row == [(items[b][p], float(F32(scores[b][p]))) for p in want[0][b, :want[3][b]].tolist()]
            assert unknown not in [i for i, _ in row] and len({i for i, _ in row}) == len(row)
        assert pairs[-1] == [] and Recommender(m).diversify_batch(items, scores, top_k=7, diversity=0.45) == pairs
        assert_same(m.model.diversify_batch(ids.tolist(), sc.tolist(), top_k=7, lam=F32(1.0 - 0.45)), want, "SLIMElastic.diversify_batch")
    with pytest.raises(ValueError, match="one score per item"):
        m.diversify_batch([[known[0], known[1]]], [[1.0]])
    with pytest.raises(ValueError, match="1024"):
        m.diversify_batch([[known[j % len(known)] for j in range(1025)]], [[1.0] * 1025])
    with pytest.raises(ValueError, match="top_k"):
        m.diversify_batch([[known[0]]], [[1.0]], top_k=0)
    with pytest.raises(ValueError, match="diversity"):
        m.diversify_batch([[known[0]]], [[1.0]], diversity=1.5)


def test_every_refusal_of_the_public_calls():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    fresh = cpu_slim()
    for call in (lambda: fresh.recommend_diverse_batch([1]), lambda: fresh.diversify_batch([[1]], [[1.0]]),
                 lambda: fresh.model.diversify_batch([[1]], [[1.0]])):
        with pytest.raises(RuntimeError, match="Model must be fitted"):
            call()
    m, batch = _model()
    users = sorted({u for u, _, _, _ in batch})[:4]
    for kw in (dict(top_k=0), dict(top_k=11, pool=10), dict(pool=1025, top_k=10), dict(top_k=-1), dict(pool=0, top_k=0)):
        with pytest.raises(ValueError, match="top_k <= pool <= 1024"):
            m.recommend_diverse_batch(users, **kw)
    for d in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"diversity must lie in \[0, 1\]"):
            m.recommend_diverse_batch(users, diversity=d)
    assert len(m.recommend_diverse_batch(users, top_k=1, pool=1)[0]) == 1 and m.recommend_diverse_batch(users, diversity=1.0)
    # a pool the fused top-k kernels refuse for this model
    eng = m.model.engine
    eng.topk_supported = lambda top_k, mode: top_k < 40
    assert m.recommend_diverse_batch(users, top_k=5, pool=39)
    with pytest.raises(ValueError, match="do not serve lists of pool=40 .* smaller pool"):
        m.recommend_diverse_batch(users, top_k=5, pool=40)
    del eng.topk_supported
    # the fused kernels rank lists of at most MAX_TOP_K: a wider pool is refused with that reason (a catalogue that wide is needed)
    wide = eng.MAX_TOP_K
    eng.MAX_TOP_K = 30
    try:
        assert m.recommend_diverse_batch(users, top_k=5, pool=30)
        with pytest.raises(ValueError, match="at most 30 .* smaller pool"):
            m.recommend_diverse_batch(users, top_k=5, pool=31)
    finally:
        eng.MAX_TOP_K = wide
    # a float64 W holding float32 numbers is served with them; one holding other numbers is refused
    W = m.model.item_similarity
    want = m.recommend_diverse_batch(users, top_k=5, pool=20, ret_scores=True)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)
    got = m.recommend_diverse_batch(users, top_k=5, pool=20, ret_scores=True)      # (its scoring pass adds in double: last bits)
    assert [[i for i, _ in row] for row in got] == [[i for i, _ in row] for row in want]
    assert np.allclose([[s for _, s in row] for row in got], [[s for _, s in row] for row in want], rtol=1e-6, atol=0)
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.recommend_diverse_batch(users)
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.diversify_batch([[1, 2]], [[2.0, 1.0]])
    m.model.item_similarity = W
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=DiverseOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
        eng.diversify_lists(np.array([[1, 2]], np.int32), np.array([[2.0, 1.0]], F32), keep=1)
    mine = m.model._engine
    m.model._engine = eng                                                # ... through the public calls too
    m.model._sync_weights = lambda: None
    try:
        with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
            m.recommend_diverse_batch(users)
        with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
            m.diversify_batch([[1, 2]], [[2.0, 1.0]])
    finally:
        del m.model._sync_weights
        m.model._engine = mine
    # the engine's own ranges
    m.model._sync_weights()
    eng = m.model.engine
    for kw in (dict(keep=0), dict(keep=3), dict(lam=1.5), dict(lam=float("nan"))):
        with pytest.raises(ValueError, match="diversify"):
            eng.diversify_lists(np.array([[1, 2]], np.int32), np.array([[2.0, 1.0]], F32), **kw)
    with pytest.raises(ValueError, match="one shape"):
        eng.diversify_lists(np.array([[1, 2]], np.int32), np.array([[2.0]], F32))


# ---------------------------------------------------------------------------------------------- serving
def test_recommend_diverse_route_token_payload_and_failure():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = _model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = batch[0][0]
    body = {"user": user, "top_k": 4, "pool": 20, "diversity": 0.6}
    r = client.post("/recommend_diverse", json=body, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/recommend_diverse", json=body, headers=ok)
    want = m.recommend_diverse(user, top_k=4, pool=20, diversity=0.6, ret_scores=True)
    assert r.status_code == 200 and len(want) == 4
    assert r.json() == {"user": user, "items": [{"item": i, "score": s} for i, s in want]}
    r = client.post("/recommend_diverse", json={"user": user}, headers=ok)                    # the defaults: top 10 of 50 at 0.3
    assert r.status_code == 200 and [e["item"] for e in r.json()["items"]] == m.recommend_diverse(user)
    r = client.post("/recommend_diverse", json={"user": user, "top_k": 5, "pool": 4}, headers=ok)   # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Recommend diverse failed"}
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)                # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(user, top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def ext_declared_symbols():
    text = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rtrec_[a-z0-9_]+)\s*\(", text)))


def test_the_extension_surface_follows_the_rules_of_the_core():
    import ctypes
    import torch
    from rtrec_amd import _native, build, ops
    # the header declares exactly EXT_EXPORTS; the core surface did not grow
    assert ext_declared_symbols() == sorted(_native.EXT_EXPORTS) and "rtrec_slim_diversify_lists" in _native.EXT_EXPORTS
    assert not set(_native.EXT_EXPORTS) & set(_native.EXPORTS)
    assert "diversify.hip" in build.SOURCES
    ext = os.path.join("..", "..", "include", "rtrec_amd_ext.h")
    assert ext in build.HEADERS[:-1] and build.HEADERS[-1].endswith("rtrec_amd.h") and build.EXT_HEADER == ext
    # every launching symbol is behind exactly one op
    assert ops.EXT_EXPORT_OF["diversify_lists"] == "rtrec_slim_diversify_lists" and sorted(ops.EXT_EXPORT_OF) == sorted(ops.EXT_OPS)
    assert len(set(ops.EXT_EXPORT_OF.values())) == len(ops.EXT_OPS)
    assert sorted(ops.EXT_EXPORT_OF.values()) == sorted(_native.EXT_EXPORTS) and not set(ops.EXT_OPS) & set(ops.OPS)
    # the library exports them, and the loaded binding knows them
    lib = ctypes.CDLL(build.LIB_PATH)
    L = _native.load()
    for name in _native.EXT_EXPORTS:
        assert hasattr(lib, name), f"{name} is declared in include/rtrec_amd_ext.h but not exported"
        assert getattr(L, name).argtypes is not None
    # no Python file of the package calls them by raw ctypes
    call = re.compile(r"\.(rtrec_[a-z0-9_]+)\(")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):
        for f in files:
            if f.endswith(".py") and f != "_native.py":
                for name in call.findall(open(os.path.join(dirpath, f)).read()):
                    assert name not in _native.EXT_EXPORTS, f"{f} calls {name} by ctypes"
    # the op: outputs declared as mutated, inputs not
    for name in ops.EXT_OPS:
        schema = str(getattr(torch.ops.rtrec_amd, name).default._schema)
        assert schema.startswith(f"rtrec_amd::{name}(") and "!" in schema, f"{name} declares no mutated argument"
    schema = str(torch.ops.rtrec_amd.diversify_lists.default._schema)
    assert schema.endswith("-> ()")
    for name in ("order", "value", "penalty", "count"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("wc_ptr", "wc_row", "wc_val", "ids", "scores", "counts"):
        assert f"Tensor {name}" in schema, schema
    assert "int list_k" in schema and "int keep" in schema and "float lam" in schema and "int waves_per_row" in schema
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.diversify_lists(i32(4), i32(1), torch.zeros(1), 3, i32(1, 2), torch.zeros(1, 2), i32(1), 2, 1, 0.5, 0,
                                                i32(1, 1), torch.zeros(1, 1), torch.zeros(1, 1), i32(1))


def test_the_entry_point_checks_its_arguments_on_the_host():
    from rtrec_amd import _native
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    fn = _native.load().rtrec_slim_diversify_lists
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_rows=1, n_items=5, wptr=one, wrow=one, wval=one, nnz=0, ids=one, istride=10, scores=one, sstride=10, list_k=10, counts=one, keep=3, lam=0.5, \
        waves=0, order=one, value=one, penalty=one, count=one: (
        n_rows, n_items, wptr, wrow, wval, nnz, ids, istride, scores, sstride, list_k, counts, keep, lam, waves, order, value, penalty, count, None)
    for kw in (dict(list_k=0), dict(list_k=1025, istride=1025, sstride=1025), dict(keep=0), dict(keep=11), dict(keep=-1), dict(waves=2),
               dict(waves=-1), dict(waves=8)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(lam=-0.5), dict(lam=1.5), dict(lam=float("nan")), dict(n_rows=-1), dict(n_items=-1), dict(nnz=-1), dict(istride=9),
               dict(sstride=9), dict(ids=None), dict(scores=None), dict(counts=None), dict(order=None), dict(value=None),
               dict(penalty=None), dict(count=None), dict(wptr=None), dict(nnz=3, wrow=None), dict(nnz=3, wval=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_items=0, wptr=None, wrow=None, wval=None, n_rows=0)) == 0          # an empty W needs no arrays
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, ids=None, scores=None, order=None)) == 0
    for name in ("diversify_device", "diversify_lists"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "diversify_lists"))
