"""Catalogue ranks on the GPU (csrc/catalogue_ranks.hip, torch.ops.rtrec_amd.catalogue_ranks, SLIM.rank_items_batch,
Recommender.evaluate_catalogue) against the host models of tests/test_ranks_host.py: above, tied and competing with ==, score
by its bits.  The output buffers are poisoned before every call: every slot must be written."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from rtrec_amd.utils.metrics import catalogue_rank_summary
from tests.test_ranks_host import (DENSE, SPARSE, assert_same, every_pair, golden_block, hand_case, host_model, host_model_vectorised)
from tests.test_rerank_host import _batch

pytestmark = pytest.mark.gpu

GRID_CAP = 2048                          # kRanksMaxGrid of csrc/catalogue_ranks.hip: workgroups per launch


def run_op(S, n_items, rows, X, filter_interacted, mode, tg_ptr, tg_items):
    """torch.ops.rtrec_amd.catalogue_ranks on host arrays: S [n_rows, >= n_items] float32 or float64, X csr (its values are
    not read), rows int32 or None.  Returns the four arrays of the host models."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to("cuda:0")        # (a copy: the shared fixture arrays are read-only)
    n_rows, n_tg = S.shape[0], len(tg_items)
    above = torch.full((n_tg,), -7, dtype=torch.int32, device="cuda:0")            # poisoned: every slot must be written
    tied = torch.full((n_tg,), -7, dtype=torch.int32, device="cuda:0")
    score = torch.full((n_tg,), 7.0, dtype=torch.float64, device="cuda:0")
    competing = torch.full((n_rows,), -7, dtype=torch.int32, device="cuda:0")
    torch.ops.rtrec_amd.catalogue_ranks(up(S, S.dtype), n_items, None if rows is None else up(rows, np.int32), up(X.indptr, np.int32),
                                        up(X.indices, np.int32), bool(filter_interacted), mode, up(tg_ptr, np.int64), up(tg_items, np.int32),
                                        above, tied, score, competing)
    torch.cuda.synchronize()
    return above.cpu().numpy(), tied.cpu().numpy(), score.cpu().numpy(), competing.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module", params=["f32", "f64"])
def fixture_block(request):
    """Every (user, item) of the 240 x 400 fixture as a target, with the host model's answers for both modes and both filter
    settings (computed once, shared, never changed)."""
    X, users, S = golden_block(np.float32 if request.param == "f32" else np.float64)
    ptr, items = every_pair(240, 400)
    want = {(mode, filt): host_model_vectorised(S, 400, users, X, filt, mode, ptr, items) for mode in (SPARSE, DENSE) for filt in (True, False)}
    return request.param, X, users, S, ptr, items, want


@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("mode", [SPARSE, DENSE])
def test_every_pair_of_the_fixture_equals_the_host_model(fixture_block, mode, filt):
    w, X, users, S, ptr, items, want = fixture_block
    got = run_op(S, 400, users, X, filt, mode, ptr, items)
    assert_same(got, want[mode, filt], f"fixture {w} mode={mode} filter={filt}")
    assert (got[0] >= 0).sum() == got[3].sum() > 80000 and (got[0] == -1).sum() == 96000 - got[3].sum()


# ---------------------------------------------------------------------------------------------- hand-written rows
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_written_rows(dtype):
    S, n_items, rows, X, tg_ptr, tg_items = hand_case()
    S = S.astype(dtype)
    for mode in (SPARSE, DENSE):
        for filt in (True, False):
            want = host_model(S, n_items, rows, X, filt, mode, tg_ptr, tg_items)
            assert_same(run_op(S, n_items, rows, X, filt, mode, tg_ptr, tg_items), want, f"hand-written mode={mode} filter={filt}")
    assert want[1].max() == 3 and np.isnan(want[2]).sum() == 1 and np.isinf(want[2]).sum() == 5


# ---------------------------------------------------------------------------------------------- every size
def random_block(rng, n_rows, n_items, stride, dtype, n_x_rows=None):
    """Score rows drawn from a few values (ties, zeros of both signs, negatives, a NaN and an inf now and then) with garbage
    beyond n_items, and an X whose rows store a tenth of the columns."""
    values = np.array([0.0, -0.0, 1.0, 2.0, -1.0, 0.5, 3.0, np.nan, np.inf, -np.inf], dtype)
    p = np.array([0.3, 0.05, 0.15, 0.1, 0.1, 0.1, 0.1, 0.04, 0.03, 0.03])
    S = rng.choice(values, size=(n_rows, stride), p=p)
    S[:, n_items:] = 9.0
    n_x_rows = n_rows if n_x_rows is None else n_x_rows
    X = sp.random(n_x_rows, n_items, density=0.1, format="csr", dtype=np.float32, random_state=int(rng.integers(1 << 30)))
    X.sort_indices()
    return np.ascontiguousarray(S), X


@pytest.mark.parametrize("n_targets", [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_target_counts_across_every_group_size(n_targets):
    """Four rows of 300 items: the row under test with `n_targets` targets, a row without any before and after it, and one
    with three; targets in any order, repeated, some out of range."""
    rng = np.random.default_rng(n_targets)
    S, X = random_block(rng, 4, 300, 300, np.float32)
    counts = [0, n_targets, 0, 3]
    tg_ptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    tg_items = rng.integers(-1, 302, int(tg_ptr[-1])).astype(np.int32)
    for mode in (SPARSE, DENSE):
        want = host_model_vectorised(S, 300, None, X, True, mode, tg_ptr, tg_items)
        assert_same(run_op(S, 300, None, X, True, mode, tg_ptr, tg_items), want, f"n_targets={n_targets} mode={mode}")
    assert want[3].min() > 100


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_items", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_row_lengths_across_the_vector_load_tails(n_items, dtype):
    """Five rows of `n_items` scores in a block three wider (so the rows start at every alignment), garbage beyond the items;
    five targets a row; d_row_ids given and NULL."""
    rng = np.random.default_rng(n_items)
    S, X = random_block(rng, 5, n_items, n_items + 3, dtype, n_x_rows=9)
    tg_ptr = np.arange(6, dtype=np.int64) * 5
    tg_items = rng.integers(-1, n_items + 1, 25).astype(np.int32)
    rows = np.array([8, 0, -1, 3, 9], np.int32)
    for mode in (SPARSE, DENSE):
        for r in (rows, None):
            want = host_model_vectorised(S, n_items, r, X, True, mode, tg_ptr, tg_items)
            if n_items <= 65:
                assert_same(host_model(S, n_items, r, X, True, mode, tg_ptr, tg_items), want, "host models")
            assert_same(run_op(S, n_items, r, X, True, mode, tg_ptr, tg_items), want, f"n_items={n_items} mode={mode} rows={r is not None}")
    assert n_items < 63 or (want[0] >= 0).any()


def test_three_rows_more_than_the_grid():
    rng = np.random.default_rng(GRID_CAP + 3)
    n = GRID_CAP + 3
    S, X = random_block(rng, n, 8, 8, np.float32)
    counts = rng.integers(0, 4, n)
    counts[GRID_CAP:] = 3                                                   # the rows a second trip of the grid reaches
    tg_ptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    tg_items = rng.integers(0, 8, int(tg_ptr[-1])).astype(np.int32)
    want = host_model_vectorised(S, 8, None, X, True, SPARSE, tg_ptr, tg_items)
    assert_same(run_op(S, 8, None, X, True, SPARSE, tg_ptr, tg_items), want, "more rows than workgroups")
    assert (want[0] >= 0).sum() > n // 4 and want[3][GRID_CAP:].max() > 0


def test_slots_no_row_covers_are_written_too():
    """tg_ptr need not start at 0 or end at n_tg: the slots in front of and behind the rows' spans get -1 / 0 / -inf."""
    S, n_items, rows, X, tg_ptr, tg_items = hand_case()
    shifted = tg_ptr + 3
    items = np.r_[[0, 1, 2], tg_items, [3, 4]].astype(np.int32)
    got = run_op(S, n_items, rows, X, True, SPARSE, shifted, items)
    want = host_model(S, n_items, rows, X, True, SPARSE, tg_ptr, tg_items)
    pad = lambda a, v, n: np.full(n, v, a.dtype)
    assert_same(got, (np.r_[pad(want[0], -1, 3), want[0], pad(want[0], -1, 2)], np.r_[pad(want[1], 0, 3), want[1], pad(want[1], 0, 2)],
                      np.r_[pad(want[2], -np.inf, 3), want[2], pad(want[2], -np.inf, 2)], want[3]), "uncovered slots")


# ---------------------------------------------------------------------------------------------- the API on the device
@pytest.fixture(scope="module")
def fitted():
    from rtrec_amd import SLIM
    batch = _batch(False)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    known = sorted({u for u, _, _, _ in batch})
    return m, batch, known, max(known) + 1000


def test_rank_items_batch_is_the_position_in_recommend_batch(fitted):
    m, batch, known, cold = fitted
    items = sorted({i for _, i, _, _ in batch})
    users = known + [cold, known[3]]
    lists = [items + [10 ** 7] for _ in users]
    for filt in (True, False):
        got = m.rank_items_batch(users, lists, filter_interacted=filt)
        full = m.recommend_batch(users, top_k=400, filter_interacted=filt)
        n_listed = 0
        for b, u in enumerate(users):
            g = got[b]
            if u == cold:
                assert g["competing"] == 0 and set(g["above"]) == {-1} and set(g["score"]) == {-np.inf}
                continue
            assert g["competing"] == len(full[b]) and g["above"][-1] == -1 and g["score"][-1] == -np.inf
            for p, item in enumerate(full[b]):
                q = lists[b].index(item)
                assert g["above"][q] <= p <= g["above"][q] + g["tied"][q], (u, item, p)
                assert g["tied"][q] > 0 or g["above"][q] == p
            assert sum(a >= 0 for a in g["above"]) == len(full[b])
            n_listed += len(full[b])
        assert n_listed > 1000
    assert got[-1] == got[3]
    # a float64 W is ranked by its float64 scores
    W = m.model.item_similarity
    try:
        m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)
        got64 = m.rank_items_batch(known[:20], [items] * 20)
        full = m.recommend_batch(known[:20], top_k=400)
        for b in range(20):
            for p, item in enumerate(full[b]):
                q = items.index(item)
                assert got64[b]["above"][q] <= p <= got64[b]["above"][q] + got64[b]["tied"][q]
    finally:
        m.model.item_similarity = W


def test_evaluate_catalogue_and_one_pass_against_many(fitted):
    from rtrec_amd.recommender import Recommender
    m, batch, known, cold = fitted
    rec = Recommender(m)
    rng = np.random.default_rng(8)
    items = sorted({i for _, i, _, _ in batch})
    held = [(u, items[int(j)]) for u in known + [cold] for j in rng.integers(0, len(items), 3)] + [(known[0], 10 ** 7)]
    test = pd.DataFrame({"user": [u for u, _ in held], "item": [i for _, i in held]})
    got, frame = rec.evaluate_catalogue(test, ks=(1, 5, 10, 100), per_user=True)
    truth = test[test["item"] != 10 ** 7].groupby("user")["item"].apply(lambda s: sorted(set(s))).to_dict()
    users = [u for u in truth if u != cold]
    ptr, above, tied, score, competing = m.rank_items_batch(users, [truth[u] for u in users], as_arrays=True)
    eng = m.model.engine
    n_items = m.model.n_items_fitted
    want, cols = catalogue_rank_summary(ptr, above, tied, score, competing, ks=(1, 5, 10, 100), unknown_items=1, skipped_users=1)
    assert got == want and frame.index.tolist() == users
    assert all(np.array_equal(frame[c].to_numpy(), cols[c], equal_nan=True) for c in cols)
    assert got["n_users"] == len(known) and got["auc_users"] > 0 and 0.0 < got["auc"] <= 1.0 and got["recall@100"] >= got["recall@10"]
    # one pass against many: 1, 3 and 43 rows a pass
    flat = np.concatenate([np.asarray(truth[u], np.int64) for u in users])
    one = eng.catalogue_ranks_rows(np.asarray(users), ptr, flat, True, SPARSE)
    assert_same(one, (above, tied, score, competing), "the model's call")
    for rows_per_pass in (1, 3, 43):
        assert_same(eng.catalogue_ranks_rows(np.asarray(users), ptr, flat, True, SPARSE, block_bytes=4 * n_items * rows_per_pass), one,
                    f"{rows_per_pass} rows a pass")


def test_rows_outside_x_through_the_reused_block(fitted):
    """A -1 and an n_users + 5 row id between real users, through the real score_rows and a block that earlier passes filled:
    such a row scores 0 everywhere whatever the block held (the block is not zeroed again between passes)."""
    m, batch, known, cold = fitted
    items = sorted({i for _, i, _, _ in batch})
    m.rank_items(known[0], items[:3])                                       # (syncs W and X into the engine)
    eng, n_items = m.model.engine, m.model.n_items_fitted
    rows = np.array(known[:7] + [-1] + known[7:12] + [eng.n_users + 5] + known[12:15] + [-1, known[0]], np.int64)
    outside = np.flatnonzero((rows < 0) | (rows >= eng.n_users))
    ptr = np.arange(len(rows) + 1, dtype=np.int64) * 4
    tg = np.tile(np.array(items[:3] + [10 ** 7], np.int64), len(rows))
    for mode in (SPARSE, DENSE):
        one = eng.catalogue_ranks_rows(rows, ptr, tg, True, mode)
        for rows_per_pass in (1, 2, 3, 5):
            assert_same(eng.catalogue_ranks_rows(rows, ptr, tg, True, mode, block_bytes=4 * n_items * rows_per_pass), one,
                        f"mode={mode}, {rows_per_pass} rows a pass")
        above, tied, score, competing = (a.reshape(len(rows), -1) if a.ndim == 1 and len(a) == 4 * len(rows) else a for a in one)
        assert (score[outside, :3] == 0.0).all() and (score[:, 3] == -np.inf).all() and (above[:, 3] == -1).all()
        if mode == SPARSE:                                                  # nothing but zeros: nothing competes
            assert (competing[outside] == 0).all() and (above[outside] == -1).all() and (tied[outside] == 0).all()
        else:                                                               # every column competes, all tied at 0
            assert (competing[outside] == n_items).all() and (above[outside, :3] == 0).all() and (tied[outside, :3] == n_items - 1).all()
        assert (competing[np.setdiff1d(np.arange(len(rows)), outside)] > 0).all() and np.array_equal(competing[0], competing[-1])


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    op = torch.ops.rtrec_amd.catalogue_ranks
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)

    def call(n_items=6, mode=0, **kw):
        a = dict(scores=f32(3, 6), row_ids=i32(3), xb_ptr=i32(5), xb_col=i32(2), tg_ptr=i64(4), tg_items=i32(2), above=i32(2), tied=i32(2),
                 score=f64(2), competing=i32(3))
        a.update(kw)
        op(a["scores"], n_items, a["row_ids"], a["xb_ptr"], a["xb_col"], True, mode, a["tg_ptr"], a["tg_items"], a["above"], a["tied"],
           a["score"], a["competing"])

    call()                                                               # the well-formed calls run
    call(mode=1, scores=f64(3, 6), row_ids=None)
    call(scores=f32(3, 9))
    call(n_items=0)
    for kw in (dict(mode=2), dict(mode=-1)):
        with pytest.raises(RuntimeError, match="mode must be"):
            call(**kw)
    bad = [dict(scores=torch.zeros((3, 6), dtype=torch.float16, device=dev)), dict(scores=f32(3, 5)), dict(scores=f32(18)), dict(n_items=-1),
           dict(scores=f32(3, 12)[:, ::2]), dict(scores=torch.zeros((3, 6), dtype=torch.float32)), dict(row_ids=i64(3)), dict(row_ids=i32(2)),
           dict(row_ids=torch.zeros(3, dtype=torch.int32)), dict(xb_ptr=i64(5)), dict(xb_ptr=i32(0)), dict(xb_col=i64(2)),
           dict(xb_col=torch.zeros(2, dtype=torch.int32)), dict(tg_ptr=i32(4)), dict(tg_ptr=i64(3)), dict(tg_items=i64(2)), dict(above=i32(3)),
           dict(above=i64(2)), dict(tied=i32(1)), dict(tied=f32(2)), dict(score=f32(2)), dict(score=f64(3)), dict(competing=i32(2)),
           dict(competing=i64(3)), dict(competing=torch.zeros(3, dtype=torch.int32))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
