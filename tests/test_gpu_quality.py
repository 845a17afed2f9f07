"""List quality on the GPU (csrc/list_quality.hip, torch.ops.rtrec_amd.list_quality, SLIM.recommend_quality,
Recommender.evaluate(list_quality=True)) against the host models of tests/test_quality_host.py: n, linked and exposure with ==,
sim_sum and weight_sum by their bits.  The output buffers are poisoned before every call (every slot must be written); both
thread counts per row (waves_per_row 1 and 4) are forced, and 0 (the library's choice) runs beside them."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from rtrec_amd.utils.metrics import QUALITY_COLUMNS, QUALITY_KEYS, compute_scores, quality_frame_columns, quality_summary
from tests.test_diverse_host import fixture_pools
from tests.test_explain_host import bits
from tests.test_quality_host import (F32, HAND_WEIGHT, assert_same, expected_summary, fixture_lists, fixture_want, hand_batch, host_model,
                                     host_model_vectorised, same_dict)
from tests.test_rerank_host import _batch

pytestmark = pytest.mark.gpu

WAVES = [1, 4]
GRID_CAP = 65536                         # kListMaxGrid of csrc/list_stage.hip.h: workgroups per launch


def run_op(W, ids, counts, list_k, weight=None, exposure=True, waves=0):
    """torch.ops.rtrec_amd.list_quality on host arrays: W csc (sorted), ids [n, >= list_k]; `exposure`: True = a zeroed array,
    an int32 array = its start values, None = not kept.  Returns the five arrays of the host models (exposure None if not kept)."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to("cuda:0")        # (a copy: the shared fixture arrays are read-only)
    rows = np.asarray(ids).shape[0]
    n = torch.full((rows,), -7, dtype=torch.int32, device="cuda:0")                # poisoned: every slot must be written
    sim_sum = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda:0")
    linked = torch.full((rows,), -7, dtype=torch.int32, device="cuda:0")
    weight_sum = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda:0")
    d_exp = None if exposure is None else up(np.zeros(W.shape[1]) if exposure is True else exposure, np.int32)
    torch.ops.rtrec_amd.list_quality(up(W.indptr, np.int32), up(W.indices, np.int32), up(W.data, np.float32), W.shape[1], up(ids, np.int32),
                                     up(counts, np.int32), list_k, None if weight is None else up(weight, np.float32), waves, n, sim_sum,
                                     linked, weight_sum, d_exp)
    torch.cuda.synchronize()
    return (n.cpu().numpy(), sim_sum.cpu().numpy(), linked.cpu().numpy(), weight_sum.cpu().numpy(),
            None if d_exp is None else d_exp.cpu().numpy())


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("waves", WAVES + [0])
@pytest.mark.parametrize("lam", [1.0, 0.7, 0.3])
def test_fixture_lists_equal_the_host_model(lam, waves):
    W, ids, counts, weight = fixture_lists(lam)
    want = fixture_want(lam)
    assert (want[0] == 10).all() and (want[2] >= 1).all() and want[4].sum() == 2400
    assert_same(run_op(W, ids, counts, 10, weight, waves=waves), want, f"fixture lambda={lam} waves={waves}")


# ---------------------------------------------------------------------------------------------- every length
N_ITEMS = 3000
SPECIAL = [0, 1, 127, 128, 129, 1000, N_ITEMS]       # lengths of columns 0..6 of W; the others hold 20 weights


@pytest.fixture(scope="module")
def lengths():
    """W over 3,000 items: column c < 7 stores SPECIAL[c] weights (none, one, some hundred, and every row), the others 20 each;
    signed values of magnitude in (0, 1).  With it a weight per item."""
    rng = np.random.default_rng(17)
    lens = np.array(SPECIAL + [20] * (N_ITEMS - len(SPECIAL)))
    rows = np.concatenate([np.sort(rng.choice(N_ITEMS, L, replace=False)) for L in lens])
    vals = (rng.random(len(rows)) * rng.choice([-1.0, 1.0], len(rows))).astype(F32)
    W = sp.csc_matrix((vals, rows.astype(np.int32), np.r_[0, np.cumsum(lens)].astype(np.int32)), shape=(N_ITEMS, N_ITEMS))
    return W, (rng.random(N_ITEMS) * 12).astype(F32)


@pytest.mark.parametrize("list_k", [1, 2, 10, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_lists_and_columns_of_every_length(lengths, list_k):
    """Six (three of the longest) lists of `list_k` items with the special columns and a few duplicates at seeded places (where
    the list has room); a stride wider than the list; one short count; all three wave settings."""
    W, weight = lengths
    rng = np.random.default_rng(list_k)
    n = 6 if list_k <= 257 else 3
    ids = np.stack([rng.permutation(np.arange(len(SPECIAL), N_ITEMS))[:list_k] for _ in range(n)]).astype(np.int32)
    for b in range(n):
        where = rng.permutation(list_k)[:len(SPECIAL)]
        ids[b, where] = np.arange(len(SPECIAL))[:len(where)]
        if list_k >= 10:
            twice = rng.permutation(list_k)[:4]
            ids[b, twice[:2]] = ids[b, twice[2:]]                            # two items shown twice
    ids[0, list_k // 2] = -1
    ids[n - 1, 0] = N_ITEMS
    counts = np.full(n, list_k, np.int32)
    counts[n - 2] = max(list_k - 3, 0)
    wide = np.concatenate([ids, rng.integers(0, N_ITEMS, (n, 3)).astype(np.int32)], axis=1)           # ids_stride = list_k + 3
    want = host_model_vectorised(W, ids, counts, weight)
    if list_k <= 65:
        assert_same(host_model(W, ids, counts, weight), want, "host models")
    if list_k >= 63:
        assert want[2].sum() > 0 and (want[0] < counts).any() and want[0].max() >= list_k - 3
    for waves in WAVES + [0]:
        assert_same(run_op(W, wide, counts, list_k, weight, waves=waves), want, f"lengths k={list_k} waves={waves}")


# ---------------------------------------------------------------------------------------------- hand-written cases
@pytest.mark.parametrize("waves", WAVES)
def test_hand_written_cases(waves):
    W, ids, counts, want = hand_batch()
    assert_same(run_op(W, ids, counts, ids.shape[1], HAND_WEIGHT, waves=waves), want, f"hand-written waves={waves}")
    assert np.isinf(want[1]).sum() == 2 and (want[0] == 0).sum() == 2 and (want[0] == 1).sum() == 2


# ---------------------------------------------------------------------------------------------- more rows than workgroups
def test_three_rows_more_than_the_grid():
    W, _, _, weight = fixture_lists(1.0)
    rng = np.random.default_rng(65539)
    n = GRID_CAP + 3
    ids = rng.integers(-1, W.shape[1] + 1, (n, 2)).astype(np.int32)
    ids[::7, 1] = ids[::7, 0]                                                # some lists show one item twice
    counts = rng.integers(0, 3, n).astype(np.int32)
    ids[-3:], counts[-3:] = [[5, 9], [9, 5], [7, 7]], 2                      # the rows beyond the cap do count
    want = host_model_vectorised(W, ids, counts, weight)
    assert sorted(np.unique(want[0]).tolist()) == [0, 1, 2] and want[2].sum() > 100 and want[0][-3:].tolist() == [2, 2, 1]
    assert_same(run_op(W, ids, counts, 2, weight), want, "65,539 rows")


# ---------------------------------------------------------------------------------------------- optional operands
def test_exposure_accumulates_and_both_optional_operands_may_be_absent():
    W, ids, counts, weight = fixture_lists(0.7)
    want = fixture_want(0.7)
    start = np.arange(W.shape[1], dtype=np.int32) % 5
    once = run_op(W, ids, counts, 10, weight, exposure=start)
    assert_same(once[:4], want[:4], "a start value")
    assert np.array_equal(once[4], start + want[4])                          # added to, not zeroed ...
    twice = run_op(W, ids[:100], counts[:100], 10, weight, exposure=once[4])
    assert np.array_equal(twice[4], start + want[4] + host_model_vectorised(W, ids[:100], counts[:100])[4])   # ... over two calls
    bare = run_op(W, ids, counts, 10, None, exposure=None)
    assert bare[4] is None
    assert_same(bare[:3], want[:3], "no weight, no exposure")
    assert (bits(bare[3]) == 0).all()                                        # +0.0f, sign included
    assert_same(run_op(W, ids, counts, 10, None), want[:3] + (bare[3], want[4]), "no weight")
    assert_same(run_op(W, ids, counts, 10, weight, exposure=None)[:4], want[:4], "no exposure")


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


def test_recommend_quality_equals_the_host_aggregation_of_the_served_lists(fitted):
    m, batch, known, cold = fitted
    users = known[:40] + [cold, known[3], cold]
    plain, _ = expected_summary(m, m.recommend_batch(users, top_k=6))
    same_dict(m.recommend_quality(users, top_k=6), plain)
    diverse, raw = expected_summary(m, m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.3))
    got, frame = m.recommend_quality(users, top_k=6, pool=30, diversity=0.3, per_user=True)
    same_dict(got, diverse)
    assert list(got) == list(QUALITY_KEYS) and got["n_lists"] == len(users) and got["intra_list_similarity"] < plain["intra_list_similarity"]
    cols = quality_frame_columns(*raw[:4])
    assert frame.index.tolist() == users and all(np.array_equal(frame[c].to_numpy(), cols[c], equal_nan=True) for c in QUALITY_COLUMNS)
    items = sorted({i for _, i, _, _ in batch})
    lists = [items[:30], items[5:9] + [10 ** 7] + items[5:7], [], items[::3]]
    assert_same(m.list_quality_batch(lists, as_arrays=True), expected_summary(m, lists)[1], "list_quality_batch")


def test_evaluate_prices_the_knob_and_the_defaults_keep_the_host_paths_dict(fitted):
    from rtrec_amd.recommender import Recommender
    m, batch, known, cold = fitted
    rec = Recommender(m)
    rng = np.random.default_rng(8)
    items = sorted({i for _, i, _, _ in batch})
    held = [(u, items[int(j)]) for u in known[:50] + [cold] for j in rng.integers(0, len(items), 3)]
    test = pd.DataFrame({"user": [u for u, _ in held], "item": [i for _, i in held]})
    truth = test.groupby("user")["item"].apply(list).to_dict()
    users = list(truth)
    lists = m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.3)
    want = dict(compute_scores(zip(lists, (truth[u] for u in users)), 6))
    quality, raw = expected_summary(m, lists)
    want.update(quality)
    got, frame = rec.evaluate(test, recommend_size=6, on_device=True, diversity=0.3, pool=30, list_quality=True, per_user=True)
    same_dict(got, want)
    same_dict(rec.evaluate(test, recommend_size=6, on_device=True, diversity=0.3, pool=30, list_quality=True), want)
    cols = quality_frame_columns(*raw[:4])
    assert frame.index.tolist() == users and all(np.array_equal(frame[c].to_numpy(), cols[c], equal_nan=True) for c in QUALITY_COLUMNS)
    # either argument alone
    only_diverse = rec.evaluate(test, recommend_size=6, on_device=True, diversity=0.3, pool=30)
    same_dict(only_diverse, {key: want[key] for key in only_diverse})
    assert len(only_diverse) == 9 and lists != m.recommend_batch(users, top_k=6)
    plain = dict(rec.evaluate(test, recommend_size=6))
    plain.update(expected_summary(m, m.recommend_batch(users, top_k=6))[0])
    same_dict(rec.evaluate(test, recommend_size=6, on_device=True, list_quality=True), plain)
    # the defaults: today's path, today's dict
    host = rec.evaluate(test, recommend_size=6)
    same_dict(rec.evaluate(test, recommend_size=6, on_device=True), host)
    same_dict(rec.evaluate(test, recommend_size=6, on_device=True, diversity=0.0, pool=3, list_quality=False), host)


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    op = torch.ops.rtrec_amd.list_quality
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(list_k=2, waves=0, **kw):
        a = dict(wc_ptr=i32(7), wc_row=i32(3), wc_val=f32(3), ids=i32(3, list_k), counts=i32(3), item_weight=f32(6), exposure=i32(6),
                 n=i32(3), sim_sum=f32(3), linked=i32(3), weight_sum=f32(3))
        a.update(kw)
        op(a["wc_ptr"], a["wc_row"], a["wc_val"], 6, a["ids"], a["counts"], list_k, a["item_weight"], waves, a["n"], a["sim_sum"], a["linked"],
           a["weight_sum"], a["exposure"])

    call()                                                               # the well-formed calls run
    call(list_k=1024, waves=4)
    call(list_k=1024, waves=1, item_weight=None, exposure=None)
    call(ids=i32(3, 5))
    for kw in (dict(list_k=0), dict(list_k=1025), dict(waves=2), dict(waves=-1)):
        with pytest.raises(RuntimeError, match="must lie in|must be 0, 1 or 4"):
            call(**kw)
    bad = [dict(ids=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(wc_val=torch.zeros(3, dtype=torch.float16, device=dev)),
           dict(sim_sum=torch.zeros(3, dtype=torch.float64, device=dev)), dict(n=torch.zeros(3, dtype=torch.int64, device=dev)),
           dict(item_weight=torch.zeros(6, dtype=torch.float64, device=dev)), dict(exposure=torch.zeros(6, dtype=torch.int64, device=dev)),
           dict(counts=torch.zeros(3, dtype=torch.int32)), dict(exposure=torch.zeros(6, dtype=torch.int32)), dict(ids=i32(3, 4)[:, ::2]),
           dict(ids=i32(3, 1)), dict(counts=i32(2)), dict(n=i32(2)), dict(weight_sum=f32(4)), dict(item_weight=f32(5)), dict(exposure=i32(7)),
           dict(wc_ptr=i32(6)), dict(wc_val=f32(4))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()
