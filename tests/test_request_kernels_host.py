"""Host checks that go with tests/test_gpu_request_kernels.py.  Two kinds:

  * the numpy / Python models of that module against independent references, on the very inputs the GPU tests use: scipy's
    csr_matmat product for the candidates and export models, the oracle's dense mode for the dense-fill model, this
    repository's UserItemInteractions.add_interaction (and numpy_fold of tests/test_host_logic.py) for the ingest fold;
  * sensitivity: each plausible defect of a kernel is applied to a copy of its MODEL, and the mutated model must differ from
    the true one on at least one of the GPU test's inputs -- the inputs discriminate, and no wrong kernel ever runs on a GPU.
"""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import test_gpu_request_kernels as rk


def same_or_both_nan(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.dtype == b.dtype and bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


# ---- 1. candidates ----------------------------------------------------------------------------------------------------
def all_cands_cases():
    """Every (data, row ids, candidates, top_k, f64) the GPU tests run, the short ones first."""
    for name, f64 in itertools.product(rk.CD_EXTRA, (False, True)):
        yield rk.cands_extra_case(name) + (f64,)
    for n, f64 in itertools.product(rk.CD_SIZES, (False, True)):
        for case in rk.cands_cases(n, f64):
            yield case + (f64,)
    for n, f64 in ((8192, False), (6144, True)):
        for case in rk.cands_cases(n, f64):
            yield case + (f64,)


def test_candidates_inputs_reach_every_branch():
    X, W = rk.cands_data()
    lens = np.diff(X.indptr)
    assert {0, 1, rk.CD_STAGED - 1, rk.CD_STAGED, rk.CD_STAGED + 1, rk.CD_ITEMS} <= set(lens.tolist())
    col_len = np.diff(W.indptr)
    assert all(col_len[c] == n for n, c in rk.CD_EXACT_COLS.items()) and col_len[rk.CD_FULL_COL] == rk.CD_ITEMS
    assert (W.data > 0).any() and (W.data < 0).any() and (X.data < 0).any()
    z = X.data[X.indptr[rk.CD_ROW["zeros"]]:X.indptr[rk.CD_ROW["zeros"] + 1]]
    assert (np.signbit(z) & (z == 0)).any() and ((z != 0) & (np.abs(z) < np.finfo(np.float32).tiny)).any()
    # launch widths: 64 threads up to 64 candidates, 128 up to 128, 256 beyond; the ABI limits of both forms
    assert {1, 64, 65, 128, 129, 257} <= set(rk.CD_SIZES)
    sizes = {(len(c), f64) for _, _, c, _, f64 in all_cands_cases()}
    assert (8192, False) in sizes and (6144, True) in sizes
    for n in rk.CD_SIZES[1:]:
        c = rk.cands_list(n)
        assert len(c) == n and len(np.unique(c)) < n and not np.array_equal(c, np.sort(c))
    rid = rk.cd_row_subset()
    assert -1 in rid and X.shape[0] in rid


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_candidates_model_equals_the_scipy_product(f64):
    """X @ W[:, cands] by scipy (csr_matmat: the order the contract cites), bit for bit, for every list of the GPU tests."""
    X, W = rk.cands_data()
    dt = np.float64 if f64 else np.float32
    Xd, Wr = X.astype(dt), W.tocsr().astype(dt)
    lists = [rk.cands_list(n) for n in rk.CD_SIZES + [6144 if f64 else 8192]]
    lists += [rk.cands_extra_case(n)[2] for n in ("pad200", "nan_some", "nan_all")]
    for c in lists:
        S = (Xd @ Wr[:, c]).toarray()
        M = np.array([[rk.cand_score("main", u, int(j), f64) for j in c] for u in range(X.shape[0])], dtype=dt)
        assert same_or_both_nan(S, M), f"{len(c)} candidates"
        assert not np.isnan(M[:rk.CD_FINITE_ROWS]).any() and (np.isnan(M[rk.CD_ROW["inf"]]).any() or len(c) == 3)
    Xh, Wh = rk.cands_data("hand")
    for c in ([0, 1], [2, 4, 3, 5, 2]):
        S = (Xh.astype(dt) @ Wh.tocsr().astype(dt)[:, c]).toarray()
        assert same_or_both_nan(S, np.array([[rk.cand_score("hand", 0, j, f64) for j in c]], dtype=dt))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_candidates_model_ranks_like_a_stable_argsort(f64):
    """The reference's rule (DESIGN D1): argsort(scores, stable)[-k:][::-1] -- on the rows without NaN scores."""
    X, W = rk.cands_data()
    dt = np.float64 if f64 else np.float32
    for n in (1, 65, 257):
        c = rk.cands_list(n)
        S = (X.astype(dt) @ W.tocsr().astype(dt)[:, c]).toarray()
        for k in (1, 10, n):
            rows = np.arange(rk.CD_FINITE_ROWS, dtype=np.int32)
            ids, sc, sc64, cnt = rk.cands_model("main", rows, c, k, f64)
            for u in rows:
                o = np.argsort(S[u], kind="stable")[-k:][::-1]
                assert cnt[u] == len(o) and ids[u, :len(o)].tolist() == c[o].tolist()
                assert np.array_equal(rk.bits(sc[u, :len(o)]), rk.bits(S[u, o].astype(np.float32)))
                assert (ids[u, len(o):] == -1).all() and (sc[u, len(o):] == -np.inf).all()


def test_float64_pair_is_below_float32_resolution():
    a32, b32 = rk.cand_score("hand", 0, 0, False), rk.cand_score("hand", 0, 1, False)
    a64, b64 = rk.cand_score("hand", 0, 0, True), rk.cand_score("hand", 0, 1, True)
    assert a32 == b32 == np.float32(1.0) and (a64, b64) == (1.0 + 2.0 ** -30, 1.0) and np.float32(a64) == np.float32(b64)


def overstaged_score(data, xrow, c, f64, **mut):
    """The staging threshold one too high: a row of 2,049 items is staged into the 2,048 slots, its last column id lands on
    the slot of the first rating (which then reads as that integer's bit pattern) and its last rating is lost."""
    X, W = rk.cands_data(data)
    if not (0 <= xrow < X.shape[0] and 0 <= c < W.shape[1]) or X.indptr[xrow + 1] - X.indptr[xrow] != rk.CD_STAGED + 1:
        return rk.cand_score(data, xrow, c, f64, **mut)
    a, b, s, e = X.indptr[xrow], X.indptr[xrow + 1], W.indptr[c], W.indptr[c + 1]
    vals = np.array(X.data[a:b])
    vals[0], vals[-1] = X.indices[b - 1:b].view(np.float32)[0], 0.0
    return rk.fold_column(X.indices[a:b], vals, W.indices[s:e], W.data[s:e], f64, **mut)


CANDS_MUTANTS = {
    "tie rule p < bp": (dict(tie_low=True), None),
    "staging threshold off by one": (dict(x_of=overstaged_score), None),
    "tail of the four-at-a-time loop dropped": (dict(drop_tail=4), None),
    "fused multiply-add": (dict(fma=True), False),                      # (exact products: no difference in float64)
    "descending item order": (dict(descending=True), None),
    "float32 comparison in the float64 form": (dict(compare_f32=True), True),
}


def lists_differ(a, b):
    return any(x is not None and not same_or_both_nan(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CANDS_MUTANTS))
def test_candidates_inputs_detect(name):
    mut, only_f64 = CANDS_MUTANTS[name]
    for data, rows, c, k, f64 in all_cands_cases():
        if only_f64 is not None and f64 != only_f64:
            continue
        if lists_differ(rk.cands_model(data, rows, c, k, f64, **mut), rk.cands_model(data, rows, c, k, f64)):
            return
    pytest.fail(f"no case of the GPU test tells the mutant '{name}' from the model")


# ---- 2. dense fill ----------------------------------------------------------------------------------------------------
def all_fill_cases():
    """(X structure, row ids, col_lo, col_hi, top_k, filter, lists, flagged) of every GPU call, the small shards first."""
    for (lo, span, beyond), k in itertools.product(rk.FILL_SHARDS, rk.FILL_TOP_K):
        xptr, xcol, ids, sc, cnt, flagged = rk.fill_case(lo, span, beyond, k)
        rid, pptr, pcol = rk.fill_permuted(xptr, xcol, len(cnt))
        for filt in (True, False):
            yield xptr, xcol, None, lo, lo + span, k, filt, ids, sc, cnt, flagged
            yield pptr, pcol, rid, lo, lo + span, k, filt, ids, sc, cnt, flagged


def fill_outputs(case, **mut):
    xptr, xcol, rid, lo, hi, k, filt, ids, sc, cnt, flagged = case
    aux = np.full(ids.shape, rk.SENTINEL_AUX, dtype=np.int32)
    return rk.fill_model(xptr, xcol, rid, lo, hi, k, filt, ids, sc, aux, cnt, flagged, **mut)


def fill_differ(a, b):
    return any(not np.array_equal(np.asarray(x).view(np.int32) if np.asarray(x).dtype == np.float32 else np.asarray(x),
                                  np.asarray(y).view(np.int32) if np.asarray(y).dtype == np.float32 else np.asarray(y))
               for x, y in zip(a, b))


def test_dense_fill_inputs_reach_every_branch():
    spans = {s for _, s, _ in rk.FILL_SHARDS}
    assert {31, 2048, 2049, 2048 + 33, 4097} == spans and {0, 37} == {lo for lo, _, _ in rk.FILL_SHARDS}
    assert any(b for _, _, b in rk.FILL_SHARDS) and rk.FILL_TOP_K == [1, 8, 63, 64]
    xptr, xcol, ids, sc, cnt, flagged = rk.fill_case(37, 2048 + 33, 60, 8)
    assert 70 <= len(cnt) <= 100 and len(flagged) < len(cnt) and xcol.max() >= 37 + 2048 + 33
    inside = [sc[r, :cnt[r]] for r in flagged]
    for probe in (lambda s: (s == 0).any() and not np.signbit(s[s == 0]).any(), lambda s: (np.signbit(s) & (s == 0)).any(),
                  lambda s: (s < 0).any(), lambda s: np.isnan(s).any(), lambda s: len(s) > 1 and s[0] == s[1],
                  lambda s: len(s) > 1 and s[-1] == s[-2], lambda s: ((s > 0) & (s < np.finfo(np.float32).tiny)).any()):
        assert any(probe(s) for s in inside)
    assert (cnt[flagged] == 8).any() and (cnt[flagged] == 7).any() and (cnt[flagged] == 0).any()
    rid = rk.fill_permuted(xptr, xcol, len(cnt))[0]
    assert -1 in rid and len(cnt) in rid
    assert len(rk.fill_many_rows()[4]) > 8192


def test_dense_fill_windowed_model_equals_the_plain_walk():
    """The statement of the contract (walk the ids downwards) and its restatement in windows of 2,048 ids, which carries the
    mutations below, agree on every GPU case; and the cases are not trivial."""
    completed = crossed = 0
    for case in all_fill_cases():
        plain, windowed = fill_outputs(case), fill_outputs(case, window=rk.FILL_WINDOW)
        assert not fill_differ(plain, windowed)
        ids, cnt, k, hi = plain[0], plain[3], case[5], case[4]
        grew = np.flatnonzero(cnt > case[9])
        completed += len(grew)
        crossed += sum(int(ids[r, case[9][r]:cnt[r]].min() < hi - rk.FILL_WINDOW <= ids[r, case[9][r]:cnt[r]].max()) for r in grew)
    assert completed > 1000 and crossed > 50


def test_dense_fill_model_equals_the_oracle_dense_mode(oracle):
    """A small positive model: the oracle's DENSE lists, cut down to their positive scores and fed to the model, come back
    whole -- ids, score bits and counts -- for every user whose positive list has no equal neighbours."""
    rng = np.random.default_rng(77)
    n_users, n_items = 120, 90
    X = sp.random(n_users, n_items, density=0.03, format="csr", dtype=np.float32, random_state=3,
                  data_rvs=lambda n: rng.uniform(0.5, 5.0, n).astype(np.float32))
    W = sp.random(n_items, n_items, density=0.02, format="csr", dtype=np.float32, random_state=4,
                  data_rvs=lambda n: rng.uniform(0.01, 1.0, n).astype(np.float32))
    X.sort_indices(); W.sort_indices()
    xptr, xcol = X.indptr.astype(np.int32), X.indices.astype(np.int32)
    for k, filt in itertools.product((1, 8, 63, 64), (True, False)):
        o_ids, o_sc, o_cnt = oracle.recommend_batch(X, W, top_k=k, filter_interacted=filt, dense=True)
        n_pos = np.array([int((o_sc[u, :o_cnt[u]] > 0).sum()) for u in range(n_users)], dtype=np.int32)
        ids = np.where(np.arange(k)[None, :] < n_pos[:, None], o_ids, rk.SENTINEL_ID).astype(np.int32)
        sc = np.where(np.arange(k)[None, :] < n_pos[:, None], o_sc, np.float32(rk.SENTINEL_SCORE)).astype(np.float32)
        rows = np.arange(n_users, dtype=np.int32)
        m_ids, m_sc, _, m_cnt, handed = rk.fill_model(xptr, xcol, None, 0, n_items, k, filt, ids, sc, None, n_pos, rows)
        done = np.setdiff1d(rows, handed)
        assert len(done) > (n_users // 2 if k >= 8 else 0) and (n_pos[done] < k).all() and (m_cnt[done] > n_pos[done]).any()
        for u in handed:
            s = sc[u, :n_pos[u]]
            assert n_pos[u] == k or (s[1:] == s[:-1]).any()
        for u in done:
            assert m_cnt[u] == o_cnt[u] and np.array_equal(m_ids[u, :o_cnt[u]], o_ids[u, :o_cnt[u]])
            assert np.array_equal(rk.bits(m_sc[u, :o_cnt[u]]), rk.bits(o_sc[u, :o_cnt[u]]))


FILL_MUTANTS = {
    "have not carried into the second window": dict(carry=False),
    "partial-word mask off by one": dict(mask_slack=1),
    "listed id not masked": dict(mask_listed=False),
    "user's items not masked in later windows": dict(mask_items_later=False),
    ">= instead of > in the positivity test": dict(nonneg_ok=True),
}


@pytest.mark.parametrize("name", list(FILL_MUTANTS))
def test_dense_fill_inputs_detect(name):
    for case in all_fill_cases():
        if fill_differ(fill_outputs(case, window=rk.FILL_WINDOW, **FILL_MUTANTS[name]), fill_outputs(case)):
            return
    pytest.fail(f"no case of the GPU test tells the mutant '{name}' from the model")


# ---- 3. score-vector export --------------------------------------------------------------------------------------------
def test_export_inputs_reach_every_branch():
    from rtrec_amd.layouts import build_tiled_w
    X, W = rk.export_data()
    assert X.indices.max() >= rk.EX_ITEMS and 0 in np.diff(X.indptr)
    wide = W.tocsr()[rk.EX_WIDE_ROW].indices
    assert set(range(256, 512)) <= set(wide.tolist())                  # more than 64 entries of one tile in one row of W
    assert any(rk.EX_WIDE_ROW in X.indices[X.indptr[u]:X.indptr[u + 1]] for u in range(3))
    tiles = {name: build_tiled_w(W, lo, hi, rk.EX_TILE) for name, (lo, hi) in rk.EX_LAYOUTS.items()}
    assert [(t.n_tiles, t.n_cols - (t.n_tiles - 1) * rk.EX_TILE) for t in tiles.values()] == [(3, 188), (1, 256), (2, 1)]
    for t in tiles.values():
        assert t.tile_cols == rk.EX_TILE and {0, 255 if t.n_cols >= 256 else 0} <= set(t.w_col.tolist())
    jobs = {n * t.n_tiles for n in rk.EX_ROWS for t in tiles.values()}
    assert {3, 9, 15, 33} <= jobs and any(j % 8 for j in jobs)
    for n in rk.EX_ROWS[1:]:
        rid = rk.export_row_ids(n)
        assert -1 in rid and len(set(rid.tolist())) < n


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_export_model_equals_the_scipy_product(f64):
    X, W = rk.export_data()
    dt = np.float64 if f64 else np.float32
    S = rk.export_scores(f64)
    Xd, Wr = X[:, :rk.EX_ITEMS].astype(dt), W.tocsr().astype(dt)
    for layout, (lo, hi) in rk.EX_LAYOUTS.items():
        P = (Xd @ Wr[:, lo:hi]).toarray()
        assert rk.same_bits(np.ascontiguousarray(P), np.ascontiguousarray(S[:X.shape[0], lo:hi]))
        for n_rows, rid, stride in rk.export_cases(layout):
            img = rk.export_image(layout, n_rows, rid, stride, f64, tail=64)
            body = img[:n_rows * stride].reshape(n_rows, stride)
            rows = np.arange(n_rows) if rid is None else rid
            want = np.where((rows >= 0)[:, None], P[np.maximum(rows, 0)], 0).astype(dt)
            assert rk.same_bits(np.ascontiguousarray(body[:, :hi - lo]), want)
            assert (body[:, hi - lo:] == rk.SENTINEL_SCORE).all() and (img[n_rows * stride:] == rk.SENTINEL_SCORE).all()
    assert (S != 0).mean() > 0.2 and (S < 0).any()


EXPORT_MUTANTS = {"t0 missing from the output address": dict(no_t0=True), "col_offset ignored": dict(no_col_offset=True),
                  "ncol taken as tile_cols in the last tile": dict(full_last_tile=True)}


@pytest.mark.parametrize("name", list(EXPORT_MUTANTS))
def test_export_inputs_detect(name):
    hits = gap_hits = 0
    for layout, f64 in itertools.product(rk.EX_LAYOUTS, (False, True)):
        n_cols = rk.EX_LAYOUTS[layout][1] - rk.EX_LAYOUTS[layout][0]
        for n_rows, rid, stride in rk.export_cases(layout):
            a = rk.export_image(layout, n_rows, rid, stride, f64, tail=64)
            b = rk.export_image(layout, n_rows, rid, stride, f64, tail=64, **EXPORT_MUTANTS[name])
            diff = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
            hits += bool(diff.size)
            gap_hits += bool(((diff % stride >= n_cols) | (diff >= n_rows * stride)).any())
    assert hits > 0, f"no case of the GPU test tells the mutant '{name}' from the model"
    if "ncol" in name:
        assert gap_hits > 0                    # caught by the sentinels of the gap words and behind the last row


# ---- 4. ingest fold ----------------------------------------------------------------------------------------------------
FOLD_COMBOS = [(lo, hi, with_old, upsert) for (lo, hi) in rk.FOLD_BOUNDS for with_old in (False, True) for upsert in (False, True)]


def test_fold_inputs_reach_every_branch():
    order, start, delta, tstamp, old = rk.fold_batch()
    lens = np.diff(start)
    assert set(rk.FOLD_RUNS) == set(lens.tolist()) and {7, 8, 9, 15, 16, 17} <= set(lens.tolist())
    assert np.isnan(delta).any() and (delta == np.inf).any() and (delta == -np.inf).any() and (delta == 1e308).sum() >= 2
    assert (np.signbit(delta) & (delta == 0)).any() and (np.abs(delta) == 2.0 ** 24 + 1).any()
    assert np.isnan(old).any() and (old > 10).any() and (old < -3).any() and (np.signbit(old) & (old == 0)).any()
    assert sorted(order.tolist()) == list(range(len(delta))) and not np.array_equal(order, np.arange(len(delta)))
    for g in range(len(lens)):
        assert (np.diff(order[start[g]:start[g + 1]]) > 0).all()           # a pair's occurrences in arrival order
    # inf + -inf really happens, and the overflow really overflows, under the unbounded store
    val = rk.fold_model(order, start, delta, tstamp, None, -np.inf, np.inf, False)[0]
    assert (val == -np.inf).any() and (val == np.inf).any()
    v32 = rk.fold_model(order, start, delta, tstamp, None, -np.inf, np.inf, False)[2]
    assert ((v32.astype(np.float64) != val) & np.isfinite(val)).any()      # a value float32 cannot hold


@pytest.mark.parametrize("lo,hi,with_old,upsert", FOLD_COMBOS)
def test_fold_model_equals_numpy_fold(lo, hi, with_old, upsert):
    import torch
    from tests.test_host_logic import numpy_fold
    order, start, delta, tstamp, old = rk.fold_batch()
    old = old if with_old else None
    t = [torch.from_numpy(np.array(a)) for a in (order, start, delta, tstamp)]
    with np.errstate(all="ignore"):
        val, ts, v32 = numpy_fold(torch)(*t, None if old is None else np.array(old), lo, hi, upsert)
    m_val, m_ts, m_v32 = rk.fold_model(order, start, delta, tstamp, old, lo, hi, upsert)
    assert same_or_both_nan(val.numpy(), m_val) and np.array_equal(ts.numpy(), m_ts) and same_or_both_nan(v32.numpy(), m_v32)


@pytest.mark.parametrize("upsert", [False, True], ids=["add", "upsert"])
@pytest.mark.parametrize("with_old", [False, True], ids=["empty_store", "stored"])
@pytest.mark.parametrize("lo,hi", [(-3.0, 10.0), (-np.inf, np.inf)], ids=["-3..10", "unbounded"])
def test_fold_model_equals_the_store_pair_by_pair(lo, hi, with_old, upsert):
    """UserItemInteractions.add_interaction, one call per occurrence in arrival order.  (The store needs max_value >
    min_value, so the bounds (0, 0) are left to numpy_fold; it adds `0.0 + delta`, which turns a -0.0 delta into +0.0 -- the
    one visible difference, a stored -0.0 that only meets -0.0 deltas, is compared as a number, not by its sign bit.)"""
    from rtrec_amd.utils.interactions import UserItemInteractions
    order, start, delta, tstamp, old = rk.fold_batch()
    g = len(start) - 1
    st = UserItemInteractions(min_value=lo, max_value=hi)
    if with_old:
        for k in range(g):
            st.add_interaction(k, 0, 1.6e9, float(old[k]), upsert=True)
    group_of = np.empty(len(delta), dtype=np.int64)
    group_of[order] = np.repeat(np.arange(g), np.diff(start))
    with np.errstate(all="ignore"):
        for i in range(len(delta)):                          # arrival order
            st.add_interaction(int(group_of[i]), 0, float(tstamp[i]), float(delta[i]), upsert=upsert)
    blk = st._compact()
    assert np.array_equal(blk.key >> 32, np.arange(g))
    m_val, m_ts, _ = rk.fold_model(order, start, delta, tstamp, old if with_old else None, lo, hi, upsert)
    neg_zero = np.signbit(m_val) & (m_val == 0) & (blk.val == 0) & ~np.signbit(blk.val)
    assert same_or_both_nan(np.where(neg_zero, 0.0, blk.val), np.where(neg_zero, 0.0, m_val)) and neg_zero.sum() <= 5 * (not upsert)
    assert np.array_equal(blk.ts, m_ts)


FOLD_MUTANTS = {"clip order swapped": dict(clip_swapped=True), "tail of the eight-block dropped": dict(drop_tail=True),
                "d_old ignored": dict(no_old=True)}


@pytest.mark.parametrize("name", list(FOLD_MUTANTS))
def test_fold_inputs_detect(name):
    order, start, delta, tstamp, old = rk.fold_batch()
    mut = dict(FOLD_MUTANTS[name])
    no_old = mut.pop("no_old", False)
    for lo, hi, with_old, upsert in FOLD_COMBOS:
        o = old if with_old else None
        a = rk.fold_model(order, start, delta, tstamp, o, lo, hi, upsert)
        b = rk.fold_model(order, start, delta, tstamp, None if no_old else o, lo, hi, upsert, **mut)
        if any(not same_or_both_nan(x, y) for x, y in zip(a, b)):
            return
    pytest.fail(f"no case of the GPU test tells the mutant '{name}' from the model")


# ---- 5. float64 refine ------------------------------------------------------------------------------------------------
def test_refine_inputs_reach_both_searches():
    X, W = rk.refine_data()
    lens = np.diff(X.indptr)
    assert lens.tolist() == rk.RF_ROW_LENS and 0 < np.diff(W.indptr).max() <= rk.RF_COL_MAX and (np.diff(W.indptr) == 0).any()
    assert (X.data > 0).all() and (W.data > 0).all()
    for top_k, staged in rk.RF_STAGED.items():
        P = 2
        while P < top_k + 1:
            P *= 2
        assert staged == 1024 // (64 // P)                          # kRfItems over the rows of a wave
        assert {0, 1, staged - 1, staged, staged + 1, 600} <= set(lens.tolist())
        row_ids, in_ids, in_count = rk.refine_case(top_k)
        assert len(row_ids) > 4 * (64 // P)                         # more than one workgroup of four waves
        assert set(range(X.shape[0])) <= set(row_ids.tolist()) and row_ids[rk.RF_FOREIGN] == X.shape[0]
        assert ((row_ids < 0) | (row_ids >= X.shape[0])).sum() == 1
        assert {0, 1, top_k - 1, top_k, top_k + 1} <= set(in_count.tolist())
        assert all(len(set(r)) == top_k + 1 for r in in_ids.tolist()) and in_ids.min() >= 0 and in_ids.max() < rk.RF_ITEMS
        # in every wave a row searched in global memory works next to rows searched in LDS
        long_row = lens[np.clip(row_ids, 0, X.shape[0] - 1)] > staged
        long_row[rk.RF_FOREIGN] = False
        waves = [long_row[i:i + 64 // P] for i in range(0, len(row_ids) - 64 // P + 1, 64 // P)]
        assert any(w.any() and not w.all() for w in waves)


@pytest.mark.parametrize("top_k", sorted(rk.RF_STAGED))
def test_refine_model_equals_the_scipy_product_and_a_stable_sort(top_k):
    """float64 X @ W by scipy (csr_matmat adds a column's terms in ascending item order), bit for bit, ranked by a stable
    argsort of the negated scores: score descending, list position ascending."""
    X, W = rk.refine_data()
    row_ids, in_ids, in_count = rk.refine_case(top_k)
    ids, sc, sc64, cnt = rk.refine_model(top_k)
    S = (X.astype(np.float64) @ W.tocsr().astype(np.float64)).toarray()
    S = np.vstack([S, np.zeros((1, rk.RF_ITEMS))])                  # the foreign row id: an empty row
    n_tied = 0
    for r in range(len(row_ids)):
        n = min(int(in_count[r]), top_k + 1)
        s = S[row_ids[r], in_ids[r, :n]]
        o = np.argsort(-s, kind="stable")[:top_k]
        assert cnt[r] == len(o) and ids[r, :len(o)].tolist() == in_ids[r, o].tolist()
        assert same_or_both_nan(sc64[r, :len(o)], s[o]) and same_or_both_nan(sc[r, :len(o)], s[o].astype(np.float32))
        assert (ids[r, len(o):] == -1).all() and np.isneginf(sc[r, len(o):]).all() and np.isneginf(sc64[r, len(o):]).all()
        n_tied += len(set(s.tolist())) < n
    assert n_tied >= 2                                              # zero scores tie (the empty row at least): position decides


@pytest.mark.parametrize("top_k", sorted(rk.RF_STAGED))
def test_refine_inputs_tell_wrong_searches_from_the_right_one(top_k):
    want = rk.refine_model(top_k)
    staged = rk.RF_STAGED[top_k]
    differs = lambda got: any(not same_or_both_nan(g, w) for g, w in zip(got, want))
    assert differs(rk.refine_model(top_k, cap=staged))              # longer rows staged anyway: their tail is lost
    assert not differs(rk.refine_model(top_k, cap=600))
    assert differs(rk.refine_model(top_k, descending=True))         # the sum's order shows in the float64 bits
    # a row of exactly `staged` items searched in global memory or in LDS gives one answer; one too few slots does not
    assert differs(rk.refine_model(top_k, cap=staged - 1))

