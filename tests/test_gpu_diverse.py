"""Diversified lists on the GPU (csrc/diversify.hip, torch.ops.rtrec_amd.diversify_lists, SLIM.recommend_diverse_batch) against
the host models of tests/test_diverse_host.py: order and count with ==, value and penalty by their bits.  The output buffers are
poisoned before every call (every slot must be written); both thread counts per row (waves_per_row 1 and 4) are forced, and 0
(the library's choice) runs beside them."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_diverse_host import (F32, assert_same, cpu_slim, fixture_pools, hand_cases, host_model, host_model_vectorised)
from tests.test_explain_host import bits
from tests.test_rerank_host import _batch

pytestmark = pytest.mark.gpu

WAVES = [1, 4]
STAGE = 128                              # kDivStage of csrc/diversify.hip: entries of the winner's column staged in LDS per step
GRID_CAP = 65536                         # kListMaxGrid: workgroups per launch


def run_op(W, ids, scores, counts, list_k, keep, lam, waves=0):
    """torch.ops.rtrec_amd.diversify_lists on host arrays: W csc (sorted), ids / scores [n, >= list_k]."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to("cuda:0")        # (a copy: the shared fixture arrays are read-only)
    n = np.asarray(ids).shape[0]
    order = torch.full((n, keep), 12345, dtype=torch.int32, device="cuda:0")              # poisoned: every slot must be written
    value = torch.full((n, keep), 7.0, dtype=torch.float32, device="cuda:0")
    penalty = torch.full((n, keep), 7.0, dtype=torch.float32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    torch.ops.rtrec_amd.diversify_lists(up(W.indptr, np.int32), up(W.indices, np.int32), up(W.data, np.float32), W.shape[1], up(ids, np.int32),
                                        up(scores, np.float32), up(counts, np.int32), list_k, keep, float(F32(lam)), waves, order, value,
                                        penalty, count)
    torch.cuda.synchronize()
    return order.cpu().numpy(), value.cpu().numpy(), penalty.cpu().numpy(), count.cpu().numpy()


def cut(want, keep):
    """The host model's answer at a smaller keep: the head of the selection (a step does not depend on the steps behind it)."""
    return want[0][:, :keep], want[1][:, :keep], want[2][:, :keep], np.minimum(want[3], keep)


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def fixture_want():
    W, ids, scores, counts, ref_ids, _ = fixture_pools()
    return W, ids, scores, counts, ref_ids, {lam: host_model_vectorised(W, ids, scores, counts, 10, F32(lam)) for lam in (1.0, 0.7, 0.3)}


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("lam", [1.0, 0.7, 0.3])
def test_fixture_lists_equal_the_host_model(fixture_want, lam, waves):
    W, ids, scores, counts, ref_ids, want = fixture_want
    got = run_op(W, ids, scores, counts, 50, 10, lam, waves=waves)
    assert_same(got, want[lam], f"fixture lambda={lam} waves={waves}")
    if lam == 1.0:
        assert (got[0] == np.arange(10)[None, :]).all() and np.array_equal(np.take_along_axis(ids, got[0], axis=1), ref_ids)
        assert np.array_equal(bits(got[1]), bits(scores[:, :10]))
    else:
        assert (got[0] != np.arange(10)[None, :]).any(axis=1).sum() > 120 and not got[2][:, 0].any()


# ---------------------------------------------------------------------------------------------- every length
N_ITEMS = 3000
SPECIAL = [0, 1, STAGE - 1, STAGE, STAGE + 1, 1000, N_ITEMS]      # lengths of columns 0..6 of W; the others hold 20 weights


def length_case():
    """W over 3,000 items: column c < 7 stores SPECIAL[c] weights (none, one, around the staging limit, and every row: a
    K=None column), the others 20 each; signed values of magnitude in (0, 1)."""
    rng = np.random.default_rng(17)
    lens = np.array(SPECIAL + [20] * (N_ITEMS - len(SPECIAL)))
    rows = np.concatenate([np.sort(rng.choice(N_ITEMS, L, replace=False)) for L in lens])
    vals = (rng.random(len(rows)) * rng.choice([-1.0, 1.0], len(rows))).astype(F32)
    return sp.csc_matrix((vals, rows.astype(np.int32), np.r_[0, np.cumsum(lens)].astype(np.int32)), shape=(N_ITEMS, N_ITEMS))


@pytest.fixture(scope="module")
def lengths():
    return length_case()


@pytest.mark.parametrize("list_k", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_lists_and_columns_of_every_length(lengths, list_k):
    """Six (three of the longest) lists of `list_k` distinct items with the special columns at seeded places (where the list has room), scores
    descending; keep = 1, list_k and one value between; strides wider than the list; all three wave settings."""
    W = lengths
    rng = np.random.default_rng(list_k)
    n = 6 if list_k <= 257 else 3                                      # (the host model's time goes with rows x steps)
    ids = np.stack([rng.permutation(np.arange(len(SPECIAL), N_ITEMS))[:list_k] for _ in range(n)]).astype(np.int32)
    for b in range(n):
        where = rng.permutation(list_k)[:len(SPECIAL)]
        ids[b, where] = np.arange(len(SPECIAL))[:len(where)]
    scores = -np.sort(-rng.random((n, list_k)).astype(F32), axis=1)
    counts = np.full(n, list_k, np.int32)
    counts[n - 1] = max(list_k - 3, 0)
    wide_ids = np.concatenate([ids, rng.integers(0, N_ITEMS, (n, 3)).astype(np.int32)], axis=1)       # ids_stride = list_k + 3
    wide_sc = np.concatenate([scores, np.full((n, 7), 9.0, F32)], axis=1)                             # scores_stride = list_k + 7
    whole = host_model_vectorised(W, ids, scores, counts, list_k, F32(0.5))
    if list_k >= 63:
        assert whole[3][0] == list_k and (whole[2][:, 1:] > 0).any() and (whole[0] != np.arange(list_k)[None, :]).any()
    if list_k <= 65:                      # the head of a longer selection is the shorter selection
        assert_same(host_model_vectorised(W, ids, scores, counts, (list_k + 1) // 2, F32(0.5)), cut(whole, (list_k + 1) // 2), "cut")
    for keep in sorted({1, (list_k + 1) // 2, list_k}):
        want = cut(whole, keep)
        for waves in WAVES + [0]:
            assert_same(run_op(W, wide_ids, wide_sc, counts, list_k, keep, 0.5, waves=waves), want, f"lengths k={list_k} keep={keep} waves={waves}")


def test_host_models_agree_on_the_length_case(lengths):
    W = lengths
    rng = np.random.default_rng(2)
    ids = np.stack([rng.permutation(N_ITEMS)[:40] for _ in range(4)]).astype(np.int32)
    ids[:, :len(SPECIAL)] = np.arange(len(SPECIAL))
    scores = -np.sort(-rng.random((4, 40)).astype(F32), axis=1)
    assert_same(host_model_vectorised(W, ids, scores, np.full(4, 40), 40, F32(0.5)), host_model(W, ids, scores, np.full(4, 40), 40, F32(0.5)), "host models")


# ---------------------------------------------------------------------------------------------- hand-written cases
@pytest.mark.parametrize("waves", WAVES)
def test_hand_written_cases(waves):
    for name, W, ids, scores, counts, keep, lam, order, value, penalty, count in hand_cases():
        want = (np.array(order, np.int32), np.array(value, F32), np.array(penalty, F32), np.array(count, np.int32))
        assert_same(run_op(W, ids, scores, np.array(counts, np.int32), ids.shape[1], keep, lam, waves=waves), want, f"{name} waves={waves}")


@pytest.mark.parametrize("waves", WAVES)
def test_exact_ties_in_long_lists(waves):
    """Small-integer scores and power-of-two weights: most steps are decided by the tie rule, in lists that span every wave."""
    rng = np.random.default_rng(5)
    I = 300
    rows, cols = rng.integers(0, I, 4000), rng.integers(0, I, 4000)
    keep_ = rows != cols
    W = sp.csc_matrix((np.ones(int(keep_.sum()), F32), (rows[keep_], cols[keep_])), shape=(I, I))
    W.sum_duplicates()
    W.data[:] = rng.choice([0.25, 0.5, 1.0, 2.0], W.nnz) * rng.choice([-1.0, 1.0], W.nnz)
    W.sort_indices()
    ids = rng.integers(0, I, (40, 300)).astype(np.int32)                 # drawn with replacement: duplicates
    scores = -np.sort(-rng.integers(0, 6, (40, 300)).astype(F32), axis=1)
    counts = rng.integers(250, 301, 40).astype(np.int32)
    want = host_model_vectorised(W, ids, scores, counts, 60, F32(0.5))
    assert_same(host_model(W, ids[:3], scores[:3], counts[:3], 60, F32(0.5)), tuple(a[:3] for a in want), "host models")
    assert (np.diff(want[1], axis=1) == 0).sum() > 500
    assert_same(run_op(W, ids, scores, counts, 300, 60, 0.5, waves=waves), want, f"ties waves={waves}")


# ---------------------------------------------------------------------------------------------- more rows than workgroups
def test_one_row_more_than_the_grid():
    W, _, _, _, _, _ = fixture_pools()
    rng = np.random.default_rng(65537)
    n = GRID_CAP + 1
    ids = rng.integers(-1, W.shape[1] + 1, (n, 2)).astype(np.int32)
    scores = rng.random((n, 2)).astype(F32)
    counts = rng.integers(0, 3, n).astype(np.int32)
    want = host_model_vectorised(W, ids, scores, counts, 2, F32(0.25))
    assert want[3][-1] > 0 or want[3][GRID_CAP - 1] > 0
    assert sorted(np.unique(want[3]).tolist()) == [0, 1, 2] and (want[0][:, 0] == 1).any()
    assert_same(run_op(W, ids, scores, counts, 2, 2, 0.25), want, "65,537 rows")


# ---------------------------------------------------------------------------------------------- the API on the device
@pytest.mark.parametrize("strings", [False, True])
def test_recommend_diverse_batch_equals_the_cpu_stand_in_model(strings):
    from rtrec_amd import SLIM
    batch = _batch(strings)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    W = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    m.model.item_similarity = W
    ref = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    ref.add_interactions(batch)
    ref.model.item_similarity = W
    known = sorted({u for u, _, _, _ in batch}, key=str)
    cold = "nobody" if strings else max(known) + 1000
    users = known[:40] + [cold, known[3], cold]
    for kw in (dict(), dict(top_k=6, pool=30, diversity=0.6), dict(top_k=6, pool=30, diversity=0.6, ret_scores=True),
               dict(top_k=5, pool=12, diversity=1.0, filter_interacted=False), dict(top_k=4, pool=4, diversity=0.0)):
        assert m.recommend_diverse_batch(users, **kw) == ref.recommend_diverse_batch(users, **kw), kw
    assert m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.0) == m.recommend_batch(users, top_k=6)
    assert m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6) != m.recommend_batch(users, top_k=6)
    got, want = (x.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.6, as_arrays=True) for x in (m, ref))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    for g, w in zip((got[1], got[3], got[4]), (want[1], want[3], want[4])):
        assert np.array_equal(bits(g), bits(w))
    assert m.recommend_diverse(users[2], top_k=6, pool=30, diversity=0.6) == ref.recommend_diverse(users[2], top_k=6, pool=30, diversity=0.6)
    items = sorted({i for _, i, _, _ in batch}, key=str)
    lists = [items[:30], items[5:9] + ["never seen" if strings else 10 ** 7] + items[5:7], []]
    sc = [np.linspace(3, 1, len(r)).tolist() for r in lists]
    assert m.diversify_batch(lists, sc, top_k=8, diversity=0.5) == ref.diversify_batch(lists, sc, top_k=8, diversity=0.5)


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    op = torch.ops.rtrec_amd.diversify_lists
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(list_k=2, keep=2, lam=0.5, waves=0, **kw):
        a = dict(wc_ptr=i32(7), wc_row=i32(3), wc_val=f32(3), ids=i32(3, list_k), scores=f32(3, list_k), counts=i32(3),
                 order=i32(3, max(keep, 0)), value=f32(3, max(keep, 0)), penalty=f32(3, max(keep, 0)), count=i32(3))
        a.update(kw)
        op(a["wc_ptr"], a["wc_row"], a["wc_val"], 6, a["ids"], a["scores"], a["counts"], list_k, keep, lam, waves, a["order"], a["value"],
           a["penalty"], a["count"])

    call()                                                               # the well-formed calls run
    call(list_k=1024, keep=1024, waves=4)
    call(list_k=1024, keep=1, waves=1, lam=1.0)
    call(ids=i32(3, 5), scores=f32(3, 4), lam=0.0)
    for kw in (dict(list_k=0, keep=0), dict(list_k=1025), dict(keep=0), dict(keep=-1), dict(keep=3), dict(waves=2), dict(lam=-0.1),
               dict(lam=1.1), dict(lam=float("nan"))):
        with pytest.raises(RuntimeError, match="must lie in|must be 0, 1 or 4"):
            call(**kw)
    bad = [dict(ids=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(scores=torch.zeros((3, 2), dtype=torch.float64, device=dev)),
           dict(wc_val=torch.zeros(3, dtype=torch.float16, device=dev)), dict(value=torch.zeros((3, 2), dtype=torch.float64, device=dev)),
           dict(order=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(counts=torch.zeros(3, dtype=torch.int32)),
           dict(order=torch.zeros((3, 2), dtype=torch.int32)), dict(ids=i32(3, 4)[:, ::2]), dict(ids=i32(3, 1)), dict(scores=f32(3, 1)),
           dict(scores=f32(2, 2)), dict(counts=i32(2)), dict(order=i32(3, 3)), dict(penalty=f32(3, 1)), dict(count=i32(2)), dict(wc_ptr=i32(6)),
           dict(wc_val=f32(4))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()
