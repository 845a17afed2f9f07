"""Host side of Recommender.evaluate(on_device=True): the ground truth as CSR, the discount tables, the sequential means,
the registration of the rank_metrics op and what the facade refuses -- everything that needs no GPU.  The kernel and the
end-to-end path are in tests/test_gpu_evaluate.py."""
import os
import re
from math import log2

import numpy as np
import pandas as pd
import pytest

from rtrec_amd.utils import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(seed, n_rows, n_users, n_items, strings):
    """Unsorted rows with duplicated (user, item) pairs; users / items beyond the `known` ranges are unknown to the index
    functions below."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, n_users, n_rows)
    i = rng.integers(0, n_items, n_rows)
    dup = rng.integers(0, n_rows, n_rows // 3)                   # a third of the rows once more, somewhere else
    u, i = np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])
    order = rng.permutation(len(u))
    u, i = u[order], i[order]
    if strings:
        return pd.DataFrame({"user": np.array([f"u{x}" for x in u], dtype=object),
                             "item": np.array([f"i{x}" for x in i], dtype=object)})
    return pd.DataFrame({"user": u, "item": i})


@pytest.mark.parametrize("strings", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ground_truth_csr_is_the_groupby_dict(seed, strings):
    n_users, n_items, known_users, known_items = 60, 50, 45, 35
    df = _frame(seed, 700, n_users, n_items, strings)
    truth = df.groupby("user")["item"].apply(list).to_dict()
    if strings:
        u_map = {f"u{x}": x for x in range(known_users)}
        i_map = {f"i{x}": (x * 7) % known_items for x in range(known_items)}        # internal ids in another order than the names
        user_index = lambda v: np.array([u_map.get(x, -1) for x in v.tolist()], dtype=np.int64)
        item_index = lambda v: np.array([i_map.get(x, -1) for x in v.tolist()], dtype=np.int64)
        known = lambda lst: sorted({i_map[x] for x in lst if x in i_map})
        row_of = lambda k: u_map.get(k, -1)
    else:
        user_index = lambda v: np.where(v < known_users, v, -1)
        item_index = lambda v: np.where(v < known_items, v, -1)
        known = lambda lst: sorted({int(x) for x in lst if x < known_items})
        row_of = lambda k: k if k < known_users else -1
    users, rows, ptr, items, length = metrics.ground_truth_csr(df["user"].to_numpy(), df["item"].to_numpy(), user_index, item_index)
    assert users.tolist() == list(truth)                                      # same users, same (sorted) order
    assert ptr.dtype == np.int64 and items.dtype == np.int32 and length.dtype == np.int32 and len(ptr) == len(users) + 1
    assert ptr[0] == 0 and ptr[-1] == len(items)
    seen_dup = seen_unknown = False
    for j, k in enumerate(users.tolist()):
        lst = truth[k]
        assert length[j] == len(lst)
        assert items[ptr[j]:ptr[j + 1]].tolist() == known(lst)
        assert rows[j] == row_of(k)
        seen_dup |= len(set(lst)) < len(lst)
        seen_unknown |= len(known(lst)) < len(set(lst))
    assert seen_dup and seen_unknown and (rows < 0).any()                     # the frame really holds the cases named above


def test_ground_truth_csr_drops_missing_users_and_handles_empty_frames():
    df = pd.DataFrame({"user": np.array(["b", None, "a", float("nan"), "a"], dtype=object),
                       "item": np.array(["x", "x", "y", "y", None], dtype=object)})
    truth = df.groupby("user")["item"].apply(list).to_dict()
    ident = lambda v: np.arange(len(v), dtype=np.int64)
    users, rows, ptr, items, length = metrics.ground_truth_csr(df["user"].to_numpy(), df["item"].to_numpy(), ident, ident)
    assert users.tolist() == list(truth) == ["a", "b"]
    assert length.tolist() == [len(truth["a"]), len(truth["b"])] == [2, 1]     # the missing item counts in the length ...
    assert ptr.tolist() == [0, 1, 2]                                           # ... but is no member
    users, rows, ptr, items, length = metrics.ground_truth_csr(np.empty(0, np.int64), np.empty(0, np.int64), ident, ident)
    assert len(users) == 0 and ptr.tolist() == [0] and len(items) == 0 and len(length) == 0


@pytest.mark.parametrize("size", [1, 5, 10, 50, 64])
def test_discount_tables_are_the_reference_expressions(size):
    discount, ideal = metrics.discount_tables(size)
    assert discount.dtype == np.float64 and ideal.dtype == np.float64 and len(discount) == size and len(ideal) == size + 1
    for pos in range(size):
        assert discount[pos] == 1.0 / log2(pos + 2)
    for n in range(size + 1):
        assert ideal[n] == sum(1.0 / log2(pos + 2) for pos in range(n))


def test_sequential_sum_is_the_python_loop_where_numpy_sum_is_not():
    values = np.random.default_rng(7).random(100_000)
    total = 0.0
    for v in values.tolist():
        total += v
    assert metrics.sequential_sum(values) == total
    assert float(np.sum(values)) != total                # pairwise summation: why the helper exists
    assert metrics.sequential_sum(np.empty(0)) == 0.0


def test_scores_from_columns_equals_compute_scores():
    rng = np.random.default_rng(3)
    pairs = []
    for _ in range(300):
        ranked = rng.permutation(40)[:rng.integers(0, 12)].tolist()
        truth = rng.integers(0, 40, rng.integers(0, 9)).tolist()
        pairs.append((ranked, truth))
    for size in (1, 5, 10):
        rows = [metrics._query_metrics(r, t, size) for r, t in pairs]
        cols = np.array([[row[c] for c in metrics.METRIC_COLUMNS] for row in rows], dtype=np.float64)
        tp = np.array([row["tp"] for row in rows])
        got, want = metrics.scores_from_columns(cols, tp), metrics.compute_scores(iter(pairs), size)
        assert list(got) == list(want) and got == want and isinstance(got["tp"], int)
    empty = metrics.scores_from_columns(np.empty((0, 8)), np.empty(0, np.int32))
    assert empty == metrics.compute_scores(iter([]), 5) and empty["precision"] == 0.0


def test_rank_metrics_is_registered_declared_and_exported():
    import torch
    from rtrec_amd import _native, ops
    assert "rank_metrics" in ops.OPS and ops.EXPORT_OF["rank_metrics"] == "rtrec_rank_metrics"
    schema = str(torch.ops.rtrec_amd.rank_metrics.default._schema)
    for name in ("metrics", "tp", "rel"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("ids", "counts", "truth_ptr", "truth_items", "truth_len", "discount", "ideal"):
        assert f"Tensor {name}" in schema, schema
    header = open(os.path.join(ROOT, "include", "rtrec_amd.h")).read()
    assert re.search(r"\bint rtrec_rank_metrics\s*\(", header)
    assert "rtrec_rank_metrics" in _native.EXPORTS
    assert hasattr(_native.load(), "rtrec_rank_metrics")
    assert "rank_metrics.hip" in __import__("rtrec_amd.build", fromlist=["SOURCES"]).SOURCES


def _cpu_recommender():
    from tests.test_pipeline_cpu import cpu_slim
    from rtrec_amd.recommender import Recommender
    rng = np.random.default_rng(11)
    n = 1500
    train = pd.DataFrame({"user": rng.integers(0, 80, n), "item": rng.integers(0, 60, n),
                          "tstamp": 1.7e9 + np.arange(n, dtype=np.float64), "rating": rng.integers(1, 6, n).astype(np.float64)})
    test = pd.DataFrame({"user": rng.integers(0, 90, 400), "item": rng.integers(0, 70, 400)})
    rec = Recommender(cpu_slim(nn_feature_selection=6, min_value=0, max_value=15))
    rec.fit(train, batch_size=500, parallel=False)
    return rec, test


def test_on_device_is_refused_where_it_cannot_run_and_per_user_works_on_the_host():
    rec, test = _cpu_recommender()
    with pytest.raises(ValueError, match="on_device evaluation needs the HIP backend"):
        rec.evaluate(test, on_device=True)                                     # the CPU stand-in scores through another backend
    with pytest.raises(ValueError, match="user_tags"):
        rec.evaluate(test, user_tags={1: ["a"]}, on_device=True)
    for size in (0, 65, 2.5):
        with pytest.raises(ValueError, match="recommend_size"):
            rec.evaluate(test, recommend_size=size, on_device=True)

    class NoHook:
        pass
    from rtrec_amd.recommender import Recommender
    with pytest.raises(ValueError, match="no device evaluation hook"):
        Recommender(NoHook()).evaluate(test, on_device=True)

    plain = rec.evaluate(test, recommend_size=5)
    scores, frame = rec.evaluate(test, recommend_size=5, per_user=True)
    assert scores == plain and list(scores) == list(plain)
    assert list(frame.columns) == list(metrics.RESULT_KEYS) and frame.index.name == "user"
    assert frame.index.tolist() == sorted(set(test["user"].tolist()))
    n = len(frame)
    for name in metrics.METRIC_COLUMNS:
        assert metrics.sequential_sum(frame[name].to_numpy()) / n == plain[name], name
    assert int(frame["tp"].sum()) == plain["tp"]
    assert plain["hit_rate"] > 0.0                                             # not a frame of zeros
    empty_scores, empty_frame = rec.evaluate(test.iloc[:0], per_user=True)
    assert empty_scores == rec.evaluate(test.iloc[:0]) and len(empty_frame) == 0


def test_the_hook_refuses_float_id_columns_before_it_touches_the_device():
    """`3 in [3.0]` is True in the reference: a float item column is not guessed at.  (Checked on the model directly with a
    stand-in for the backend check, since the refusal must not depend on the GPU.)"""
    from rtrec_amd import SLIM
    from rtrec_amd.backend import HipBackend

    class FakeEngine:
        be = object.__new__(HipBackend)
    m = SLIM()
    m.model._engine = FakeEngine()
    with pytest.raises(ValueError, match="item column is float64"):
        m._evaluate_device(np.arange(4), np.arange(4, dtype=np.float64), 10, True)
    with pytest.raises(ValueError, match="recommend_size 1..64"):
        m._evaluate_device(np.arange(4), np.arange(4), 65, True)
