"""Rerank of per-user candidate lists on the GPU (csrc/score_pairs.hip, torch.ops.rtrec_amd.score_pairs, SLIM.rerank_batch /
score_pairs) against the numpy host model of tests/test_rerank_host.py: score bits, support, order and count with ==.  The
output buffers are poisoned before every call (every slot must be written); both thread counts per row (waves_per_row 1 and 4)
are forced where the kernel's paths differ."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from tests.test_explain_host import bits, golden
from tests.test_gpu_explain import LENGTHS, tie_case
from tests.test_rerank_host import (assert_same, cpu_slim, golden_permuted_lists, golden_scoring, host_model, host_model_vectorised,
                                    pairs_trip_case, _batch)

pytestmark = pytest.mark.gpu

WAVES = [1, 4]
ROW_LIMITS = [128, 2048]                 # rows staged in LDS up to here with 1 / 4 waves per row (csrc/score_pairs.hip)


def run_op(X, W, rows, ids, counts, list_k, top_k, filter_interacted=False, waves=0):
    """torch.ops.rtrec_amd.score_pairs on host matrices: X csr, W csc (sorted), rows None = identity, ids [n, >= list_k]."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")
    n = ids.shape[0]
    scores = torch.full((n, list_k), 7.0, dtype=torch.float32, device="cuda:0")             # poisoned: every slot must be written
    support = torch.full((n, list_k), -7, dtype=torch.int32, device="cuda:0")
    order = torch.full((n, top_k), 12345, dtype=torch.int32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.ops.rtrec_amd.score_pairs(None if rows is None else up(rows, np.int32), up(X.indptr, np.int32), up(X.indices, np.int32),
                                    up(X.data, np.float32), W.shape[1], up(W.indptr, np.int32), up(W.indices, np.int32),
                                    up(W.data, np.float32), up(ids, np.int32), up(counts, np.int32), list_k, top_k, bool(filter_interacted),
                                    waves, scores, support, order, count)
    torch.cuda.synchronize()
    return scores.cpu().numpy(), support.cpu().numpy(), order.cpu().numpy(), count.cpu().numpy()


def cut(want, top_k):
    """The host model's answer at a smaller top_k: the head of the order (ranks do not depend on top_k)."""
    return want[0], want[1], want[2][:, :top_k], np.minimum(want[3], top_k)


# ---------------------------------------------------------------------------------------------- the reference's own files
@pytest.fixture(scope="module")
def golden_want():
    X, W, users, lists, ids, scores = golden_permuted_lists()
    return X, W, users, lists, ids, scores, host_model_vectorised(X, W, users, lists, np.full(240, 400), 10, True)


@pytest.mark.parametrize("waves", WAVES)
def test_golden_fixture_scores_and_top10_equal_the_reference(golden_want, waves):
    X, W, users, lists, ids, scores, want = golden_want
    z = golden_scoring()
    pu, cands = z["predict_users"], z["cands"].astype(np.int32)
    every = np.tile(np.arange(400, dtype=np.int32), (len(pu), 1))
    sc, su, order, count = run_op(X, W, pu, every, np.full(len(pu), 400), 400, 0, waves=waves)
    assert np.array_equal(bits(sc), bits(z["predict_dense"])) and su.min() >= 0 and order.shape == (4, 0) and (count == 0).all()
    sel = run_op(X, W, pu, np.tile(cands, (len(pu), 1)), np.full(len(pu), len(cands)), len(cands), 0, waves=waves)[0]
    assert np.array_equal(bits(sel), bits(z["predict_selected"]))
    got = run_op(X, W, users, lists, np.full(240, 400), 400, 10, True, waves=waves)
    assert np.array_equal(np.take_along_axis(lists, got[2], axis=1), ids)
    assert np.array_equal(bits(np.take_along_axis(got[0], got[2], axis=1)), bits(scores.astype(np.float32)))
    assert_same(got, want, "golden")


# ---------------------------------------------------------------------------------------------- every length
ROW_LENGTHS = LENGTHS + [L + d for L in ROW_LIMITS for d in (-1, 0, 1)]
N_ORDINARY = 1500


def length_case():
    """The construction of length_case() in tests/test_gpu_explain.py -- a catalogue of 40,000 items, user r rates
    ROW_LENGTHS[r] items, column c < 8 of W stores LENGTHS[c] weights (the last one all 40,000: a K=None column), signed values,
    short rows / columns drawn from a pool of 200 so that they intersect -- with rows at the LDS staging limits added and
    N_ORDINARY ordinary columns (20 weights each, half of them from the pool) behind the special ones."""
    rng = np.random.default_rng(11)
    I, n_c = 40000, len(LENGTHS)
    pool = lambda L: 200 if L <= 130 else I
    xi = [np.sort(rng.choice(pool(L), L, replace=False)) for L in ROW_LENGTHS]
    X = sp.csr_matrix((rng.standard_normal(sum(ROW_LENGTHS)).astype(np.float32), np.concatenate(xi), np.cumsum([0] + ROW_LENGTHS)),
                      shape=(len(ROW_LENGTHS), I))
    wi = [np.sort(rng.choice(pool(L), L, replace=False)) for L in LENGTHS]
    wi += [np.unique(np.r_[rng.choice(200, 10, replace=False), rng.choice(I, 10, replace=False)]) for _ in range(N_ORDINARY)]
    lens = np.array([len(w) for w in wi])
    wptr = np.zeros(I + 1, np.int64)
    wptr[1:len(wi) + 1] = np.cumsum(lens)
    wptr[len(wi) + 1:] = wptr[len(wi)]
    W = sp.csc_matrix((rng.standard_normal(int(lens.sum())).astype(np.float32), np.concatenate(wi), wptr), shape=(I, I))
    return X, W


@pytest.fixture(scope="module")
def lengths():
    return length_case()


@pytest.mark.parametrize("list_k", [1, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_rows_columns_and_lists_of_every_length(lengths, list_k):
    """Every user x every special column, in lists of `list_k` padded with ordinary columns; top_k = list_k and 1, both
    thread counts."""
    X, W = lengths
    rng = np.random.default_rng(list_k)
    n_u, n_c = len(ROW_LENGTHS), len(LENGTHS)
    if list_k >= n_c:                    # one list per user, the special columns at seeded places in it
        rows = np.arange(n_u)
        ids = rng.integers(n_c, n_c + N_ORDINARY, (n_u, list_k)).astype(np.int32)
        for b in range(n_u):
            ids[b, rng.permutation(list_k)[:n_c]] = np.arange(n_c)
    else:                                # one list per (user, special column)
        rows = np.repeat(np.arange(n_u), n_c)
        ids = np.tile(np.arange(n_c, dtype=np.int32), n_u)[:, None]
    counts = np.full(len(rows), list_k, np.int32)
    want = host_model_vectorised(X, W, rows, ids, counts, list_k)
    su = want[1][np.arange(len(rows))[:, None], np.argsort(ids, axis=1, kind="stable")[:, :min(n_c, list_k)]].reshape(n_u, -1)
    assert su[7, 7] == 40000 and su[6, 7] == 5000 and su[1, 7] == 1 and (su[0] == 0).all() and su[6, 6] > 32       # (user, special column)
    assert all(su[r, c] > 5 for r in list(range(2, 6)) + list(range(8, 11)) for c in range(2, 6))
    for waves in WAVES:
        assert_same(run_op(X, W, rows, ids, counts, list_k, list_k, waves=waves), want, f"lengths k={list_k} waves={waves}")
        assert_same(run_op(X, W, rows, ids, counts, list_k, 1, True, waves=waves),
                    cut(host_model_vectorised(X, W, rows, ids, counts, 1, True), 1), f"lengths k={list_k} top 1 waves={waves}")


def test_vectorised_host_model_is_the_definition_on_the_length_case(lengths):
    X, W = lengths
    n_u, n_c = len(ROW_LENGTHS), 6                                       # the definition itself where it is cheap
    ids = np.tile(np.arange(n_c, dtype=np.int32), (n_u, 1))
    assert_same(host_model_vectorised(X, W, np.arange(n_u), ids, np.full(n_u, n_c), n_c), host_model(X, W, np.arange(n_u), ids, np.full(n_u, n_c), n_c),
                "host models")


# ---------------------------------------------------------------------------------------------- ties and duplicates
@pytest.mark.parametrize("waves", WAVES)
def test_tied_scores_and_duplicated_candidates(waves):
    X, W, _, _ = tie_case()
    rng = np.random.default_rng(4)
    U, I = X.shape
    ids = rng.integers(0, I, (U, 100)).astype(np.int32)                  # drawn with replacement
    counts = np.full(U, 100, np.int32)
    want = host_model_vectorised(X, W, np.arange(U), ids, counts, 11)
    top = np.take_along_axis(want[0], want[2], axis=1)
    tied = (top[:, 1:] == top[:, :-1]).any(axis=1)
    assert tied.mean() >= 0.5, f"only {tied.mean():.2f} of the rows have equal neighbouring scores among their first 11"
    assert (np.sort(ids, axis=1)[:, 1:] == np.sort(ids, axis=1)[:, :-1]).any(axis=1).all()
    assert_same(run_op(X, W, None, ids, counts, 100, 10, waves=waves), cut(want, 10), "ties")
    sample = np.arange(0, U, 16)
    assert_same(cut(tuple(w[sample] for w in want), 10), host_model(X, W, sample, ids[sample], counts[sample], 10), "host models")


# ---------------------------------------------------------------------------------------------- filter and specials
@pytest.mark.parametrize("waves", WAVES)
def test_filter_row_ids_counts_strides_and_empty_lists(waves):
    X, W, _, _, _ = golden()
    rng = np.random.default_rng(2)
    n, I = 500, W.shape[1]
    rows = rng.integers(0, 1200, n).astype(np.int32)
    rows[:40] = rows[40:80]                                              # repeats
    rows[[3, 50, 77]] = [-1, 1200, 2 ** 31 - 1]                          # users without a row
    ids = rng.integers(0, I, (n, 45)).astype(np.int32)                   # stride 45, list_k 40: the last columns are not the list's
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[5, 2], ids[6, 0], ids[7, 9] = I, I + 1000, -5
    ids[9] = -1                                                          # an all-empty list
    counts = rng.integers(-2, 46, n).astype(np.int32)                    # 0, negative and > list_k: clamped
    counts[:3] = [0, -1, 45]
    for filt in (False, True):
        want = host_model_vectorised(X, W, rows.astype(np.int64), ids[:, :40], counts, 40, filt)
        assert_same(run_op(X, W, rows, ids, counts, 40, 40, filt, waves=waves), want, f"filter={filt}")
        assert_same(run_op(X, W, rows, ids, counts, 40, 7, filt, waves=waves), cut(want, 7), f"filter={filt} top 7")
    assert (want[1][[3, 50, 77]] <= 0).all() and (want[3][[0, 1, 9]] == 0).all() and (want[1][9] == -1).all() and want[1].max() > 4
    nofilt = host_model_vectorised(X, W, rows.astype(np.int64), ids[:, :40], counts, 40, False)
    assert nofilt[3].sum() > want[3].sum()                               # the filter removed something
    assert_same(run_op(X[:n], W, None, ids, counts, 40, 40, True, waves=waves),
                host_model_vectorised(X, W, np.arange(n), ids[:, :40], counts, 40, True), "identity rows")
    # no rows at all: nothing is launched, nothing is written
    empty = run_op(X, W, np.empty(0, np.int32), np.empty((0, 40), np.int32), np.empty(0, np.int32), 40, 5, waves=waves)
    assert empty[0].shape == (0, 40) and empty[2].shape == (0, 5) and empty[3].shape == (0,)


def test_nan_and_infinite_scores():
    inf = np.float32(np.inf)
    # user 0: two inf ratings; user 1: one inf rating; columns: 2 = (+1, -1) on both, 3 = +1 on item 0, 4 = -1 on item 0, 5 = nothing
    X = sp.csr_matrix((np.array([inf, inf, inf, 2.0], np.float32), np.array([0, 1, 0, 1]), np.array([0, 2, 4])), shape=(2, 6))
    W = sp.csc_matrix((np.array([1.0, -1.0, 1.0, -1.0], np.float32), np.array([0, 1, 0, 0]), np.array([0, 0, 0, 2, 3, 4, 4])), shape=(6, 6))
    ids = np.array([[2, 3, 4, 5, 3], [2, 3, 4, 5, 3]], np.int32)
    want = host_model(X, W, [0, 1], ids, [5, 5], 5)
    assert np.isnan(want[0][0, 0]) and want[0][0, 1:].tolist() == [inf, -inf, 0.0, inf] and want[2][0].tolist() == [4, 1, 3, 2, -1]
    assert want[0][1].tolist() == [inf, inf, -inf, 0.0, inf] and want[2][1].tolist() == [4, 1, 0, 3, 2]
    for waves in WAVES:
        assert_same(run_op(X, W, None, ids, np.array([5, 5]), 5, 5, waves=waves), want, "nan / inf")


# ---------------------------------------------------------------------------------------------- more rows than the grid
@pytest.mark.parametrize("waves", WAVES)
def test_more_list_rows_than_the_grid(waves):
    """65,536 + 3 list rows onto 12 rows of X through row_ids: the grid is capped at 65,536 workgroups, so the last three rows are
    second trips, and across the cap an unstaged row of X meets a staged one of one entry in both orders and a full list an empty
    one (tests/test_rerank_host.py, pairs_trip_case): the staged row, the choice between LDS and global memory and the wave
    counts' slots of a workgroup's first row must not reach its second.  list_k 5, top_k 3, filter_interacted."""
    X, W, rows, ids, counts = pairs_trip_case()
    want = host_model_vectorised(X, W, rows, ids, counts, 3, True)
    at = np.arange(65536 + 3) % len(rows)
    got = run_op(X, W, rows[at], ids[at], counts[at], 5, 3, True, waves=waves)
    assert_same(got, tuple(w[at] for w in want), f"second trip, {waves} wave(s)")


# ---------------------------------------------------------------------------------------------- CANDIDATES mode
@pytest.mark.parametrize("n_rows", [1200, 3])
def test_a_shared_list_gives_what_candidates_mode_gives(engine, n_rows):
    X, W, _, _, _ = golden()
    engine.set_interactions(None, X, need_csc=False)
    engine.set_weights(W)
    rng = np.random.default_rng(12)
    c = rng.permutation(W.shape[1])[:300].astype(np.int32)
    rows = np.arange(1200) if n_rows == 1200 else np.array([5, 700, 1199])
    e_ids, e_sc, e_cnt = engine.recommend_rows(rows, 10, mode=_native.TOPK_CANDIDATES, candidates=c)
    ids = np.tile(c, (n_rows, 1))
    for waves in WAVES:
        sc, _, order, count = run_op(X, W, rows, ids, np.full(n_rows, 300), 300, 10, waves=waves)
        assert np.array_equal(count, e_cnt) and (count == 10).all()
        assert np.array_equal(np.take_along_axis(ids, order, axis=1), e_ids)
        assert np.array_equal(bits(np.take_along_axis(sc, order, axis=1)), bits(e_sc))
    got = engine.score_pairs_rows(rows, ids, top_k=10)                   # the engine's own call, on the resident X
    assert np.array_equal(np.take_along_axis(ids, got[2], axis=1), e_ids) and np.array_equal(got[3], e_cnt)


# ---------------------------------------------------------------------------------------------- the API on the device
@pytest.mark.parametrize("strings", [False, True])
def test_rerank_batch_and_score_pairs_equal_the_cpu_stand_in_model(strings):
    from rtrec_amd import SLIM
    batch = _batch(strings)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    W = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    m.model.item_similarity = W
    ref = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    ref.add_interactions(batch)
    ref.model.item_similarity = W
    rng = np.random.default_rng(8)
    known_users = sorted({u for u, _, _, _ in batch}, key=str)
    known_items = sorted({i for _, i, _, _ in batch}, key=str)
    unknown_item, cold = ("never seen", "nobody") if strings else (10 ** 7, max(known_users) + 1000)
    users = known_users[:40] + [cold, known_users[3], cold]
    cands = [[known_items[j] for j in rng.integers(0, len(known_items), int(rng.integers(1, 60)))] + [unknown_item] for _ in users]
    cands[-1] = known_items[:]
    for kw in (dict(top_k=5), dict(), dict(top_k=5, filter_interacted=True), dict(top_k=7, ret_scores=True)):
        assert m.rerank_batch(users, cands, **kw) == ref.rerank_batch(users, cands, **kw), kw
    # the contract, duplicates included: the request kernel of CANDIDATES mode keeps every entry of a list
    got = m.rerank_batch(users, cands, top_k=5)
    assert got == [m.recommend(u, candidate_items=c, top_k=5) for u, c in zip(users, cands)]
    assert any(len(set(c)) < len(c) for c in cands) and got[-1]
    # as_arrays is the list form
    ids, sc, counts = m.rerank_batch(users, cands, top_k=7, as_arrays=True)
    pairs = m.rerank_batch(users, cands, top_k=7, ret_scores=True)
    r_ids, r_sc, r_counts = ref.rerank_batch(users, cands, top_k=7, as_arrays=True)
    assert np.array_equal(ids, r_ids) and np.array_equal(bits(sc), bits(r_sc)) and np.array_equal(counts, r_counts)
    raw_of = m.item_ids.get
    for b, row in enumerate(pairs):
        n = int(counts[b])
        assert n == len(row) and (ids[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all()
        assert [i if users[b] == cold else raw_of(int(i)) for i in ids[b, :n].tolist()] == [i for i, _ in row]
        assert np.array_equal(bits(sc[b, :n]), bits([s for _, s in row]))
    # pair scores, with unknown ids and a user with more than 1024 pairs
    n = 2500
    pu = [known_users[j] for j in rng.integers(0, len(known_users), n)]
    pi = [known_items[j] for j in rng.integers(0, len(known_items), n)]
    pu[100:1300] = [known_users[4]] * 1200
    pu[7], pi[11] = cold, unknown_item
    a, b = m.score_pairs(pu, pi, as_arrays=True), ref.score_pairs(pu, pi, as_arrays=True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[1][7] == a[1][11] == -1 and a[1].max() >= 3


# ---------------------------------------------------------------------------------------------- mid-size
def test_mid_size_structured_matrix_equals_the_vectorised_host_model():
    import torch
    from rtrec_amd.engine import SlimEngine, coefficients_to_updates, merge_coefficients
    from rtrec_amd.synth import structured_matrix
    U, I, K = 20000, 5000, 50
    X = structured_matrix(U, I, 1_500_000, seed=7)
    Xc = X.tocsc()
    Xc.sort_indices()
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(Xc, X)
    W = merge_coefficients(None, I, *coefficients_to_updates(*eng.fit_columns(np.arange(I), nn_feature_selection=K)[:4]))
    W.sort_indices()
    eng.set_weights(W)
    rng = np.random.default_rng(3)
    rows = rng.permutation(U)[:2000]
    ids = rng.integers(0, I, (2000, 100)).astype(np.int32)
    want = host_model_vectorised(X, W, rows, ids, np.full(2000, 100), 10, True)
    assert np.diff(X.indptr)[rows].max() > ROW_LIMITS[0] and want[1].max() > 10 and (want[3] == 10).all()
    for waves in WAVES:
        d = eng.be.to_dev
        out = eng.score_pairs_device(d(rows.astype(np.int32)), 2000, None, d(ids), d(np.full(2000, 100, np.int32)), 10, True, waves_per_row=waves)
        torch.cuda.synchronize()
        assert_same(tuple(t.cpu().numpy() for t in out), want, f"mid-size waves={waves}")


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    op = torch.ops.rtrec_amd.score_pairs
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(list_k=2, top_k=2, waves=0, **kw):
        a = dict(row_ids=None, xb_ptr=i32(4), xb_col=i32(5), xb_val=f32(5), wc_ptr=i32(7), wc_row=i32(3), wc_val=f32(3), ids=i32(3, list_k),
                 counts=i32(3), scores=f32(3, list_k), support=i32(3, list_k), order=i32(3, max(top_k, 0)), count=i32(3))
        a.update(kw)
        op(a["row_ids"], a["xb_ptr"], a["xb_col"], a["xb_val"], 6, a["wc_ptr"], a["wc_row"], a["wc_val"], a["ids"], a["counts"], list_k, top_k,
           False, waves, a["scores"], a["support"], a["order"], a["count"])

    call()                                                               # the well-formed calls run
    call(list_k=1024, top_k=1024, waves=4)
    call(top_k=0, count=i32(0))
    for kw in (dict(list_k=0, top_k=0), dict(list_k=1025), dict(top_k=-1), dict(top_k=3), dict(waves=2)):
        with pytest.raises(RuntimeError, match="must lie in|must be 0, 1 or 4"):
            call(**kw)
    bad = [dict(ids=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(xb_val=torch.zeros(5, dtype=torch.float64, device=dev)),
           dict(wc_val=torch.zeros(3, dtype=torch.float16, device=dev)), dict(scores=torch.zeros((3, 2), dtype=torch.float64, device=dev)),
           dict(row_ids=torch.zeros(3, dtype=torch.int64, device=dev)), dict(counts=torch.zeros(3, dtype=torch.int32)),
           dict(order=torch.zeros((3, 2), dtype=torch.int32)), dict(ids=i32(3, 4)[:, ::2]), dict(ids=i32(3, 1)), dict(counts=i32(2)),
           dict(support=i32(3, 3)), dict(order=i32(3, 3)), dict(count=i32(2)), dict(wc_ptr=i32(6)), dict(xb_val=f32(4)), dict(row_ids=i32(2))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()
