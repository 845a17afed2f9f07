"""Recommender.evaluate(on_device=True) on the GPU: rank_metrics_kernel (csrc/rank_metrics.hip) against the reference's
per-pair figures (tests/golden/evaluate.json) and against utils.metrics._query_metrics, the op's argument checks, and the
one-pass path end to end against the host path -- all with `==`: the kernel performs the same IEEE float64 operations in
the same order as CPython, so there is no tolerance to grant."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from rtrec_amd.utils import metrics

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"

# column of rank_metrics_kernel's output for every metric name of the fixture ("true_positives" is the tp array)
GOLDEN_COLUMN = {"precision": 0, "recall": 1, "f1_score": 2, "ndcg": 3, "hit": 4, "reciprocal_rank": 5, "average_precision": 6,
                 "auc": 7}


def run_op(pairs, size, known=None):
    """(metrics[n, 8], tp[n], rel[n] uint64) of the op for (ranked list, ground truth list) pairs of item ids.  `known`:
    ids the model knows (None: all); the others count in truth_len only, like items Recommender.evaluate cannot map."""
    import torch
    from rtrec_amd import ops as _registered        # noqa: F401
    n = len(pairs)
    stride = max([size] + [len(r) for r, _ in pairs])
    ids = np.full((n, stride), -1, dtype=np.int32)
    counts = np.zeros(n, dtype=np.int32)
    ptr = np.zeros(n + 1, dtype=np.int64)
    items = []
    length = np.zeros(n, dtype=np.int32)
    for j, (ranked, truth) in enumerate(pairs):
        ids[j, :len(ranked)] = ranked
        counts[j] = len(ranked)
        members = sorted(x for x in set(truth) if known is None or x in known)
        items.extend(members)
        ptr[j + 1] = len(items)
        length[j] = len(truth)
    discount, ideal = metrics.discount_tables(size)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = torch.full((n, 8), float("nan"), dtype=torch.float64, device=DEV)
    tp = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    rel = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    torch.ops.rtrec_amd.rank_metrics(up(ids), up(counts), up(ptr), up(np.asarray(items, dtype=np.int32)), up(length), up(discount),
                                     up(ideal), size, out, tp, rel)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tp.cpu().numpy(), rel.cpu().numpy().view(np.uint64)


def check_pairs(pairs, size, known=None):
    """Every pair, every figure, `==` against _query_metrics (and the relevance word against the list itself)."""
    got, tp, rel = run_op(pairs, size, known)
    bad = []
    for j, (ranked, truth) in enumerate(pairs):
        want = metrics._query_metrics(ranked, truth, size)
        for c, name in enumerate(metrics.METRIC_COLUMNS):
            if not got[j, c] == want[name]:
                bad.append((j, name, got[j, c], want[name], ranked, truth))
        if tp[j] != want["tp"]:
            bad.append((j, "tp", tp[j], want["tp"], ranked, truth))
        word = sum(1 << p for p, item in enumerate(ranked[:size]) if item in set(truth))
        if int(rel[j]) != word:
            bad.append((j, "rel", int(rel[j]), word, ranked, truth))
    assert not bad, (size, len(bad), bad[:5])
    return got, tp


def test_kernel_reproduces_the_reference_per_pair_figures_and_means():
    g = json.load(open(os.path.join(G, "evaluate.json")))
    pairs = [(r, t) for r, t in g["pairs"]]
    assert len(pairs) == 156
    for size in (1, 5, 10):
        got, tp, _ = run_op(pairs, size)
        bad = []
        for j, want in enumerate(g["per_pair"][str(size)]):
            for name, value in zip(g["metric_names"], want):
                mine = tp[j] if name == "true_positives" else got[j, GOLDEN_COLUMN[name]]
                if not mine == value:
                    bad.append((j, name, float(mine), value, pairs[j]))
        assert not bad, (size, len(bad), bad[:5])
        scores = metrics.scores_from_columns(got, tp)
        ref = g["aggregate"][str(size)]
        assert set(scores) == set(ref)
        for name in ref:
            assert scores[name] == ref[name], (size, name, scores[name], ref[name])
        check_pairs(pairs, size)                           # and the host code of this package says the same


def _seeded_pairs(seed, n, n_known, n_items, max_ranked, max_truth):
    """Ranked lists of distinct KNOWN items (what a model can recommend), truth lists with duplicated entries and with
    items >= n_known the model has never seen; empty lists on both sides."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        ranked = rng.permutation(n_known)[:rng.integers(0, max_ranked + 1)].tolist()
        truth = rng.integers(0, n_items, rng.integers(0, max_truth + 1)).tolist()
        if truth and rng.random() < 0.5:
            truth += [truth[k] for k in rng.integers(0, len(truth), rng.integers(1, 4))]      # duplicated rows of the test frame
        if ranked and rng.random() < 0.3:
            truth += ranked[:rng.integers(1, len(ranked) + 1)]                                 # some lists that hit a lot
        if ranked and rng.random() < 0.05:
            truth = list(ranked)                                                               # tp == k
        pairs.append((ranked, truth))
    pairs += [([], []), ([], [1, 2, 2]), ([3, 4], []), ([5], [5]), ([5], [5, 5, n_known + 1]), (list(range(64)), list(range(64))),
              (list(range(70)), [0, 69, 63, 64]), (list(range(64)), [63]), (list(range(64)), [n_known + 3] * 5)]
    return pairs


@pytest.mark.parametrize("size", [1, 2, 3, 5, 10, 16, 17, 33, 50, 64])
def test_kernel_equals_query_metrics_on_seeded_pairs(size):
    n_known = 90
    pairs = _seeded_pairs(100 + size, 700, n_known, 120, 80, 30)       # ranked lists shorter than, equal to and longer than size
    assert any(len(r) > size for r, _ in pairs) and any(0 < len(r) < size for r, _ in pairs) or size == 1
    assert any(len(r) == 0 for r, _ in pairs) and any(len(set(t)) < len(t) for _, t in pairs)
    assert any(x >= n_known for _, t in pairs for x in t)
    got, tp = check_pairs(pairs, size, known=set(range(n_known)))
    assert tp.sum() > 0 and (got[:, 7] > 0).any()                     # not a trivial batch
    assert size < 3 or ((got[:, 7] > 0) & (got[:, 7] < 1)).any()      # (a fractional auc needs a hit and a miss behind it)


def test_kernel_tiles_rows_beyond_one_grid_pass():
    """More tiles of 64 users than the launch has workgroups: the grid-stride loop serves them all."""
    known = set(range(90))
    pairs = _seeded_pairs(5, 300, 90, 120, 12, 6)
    reps = (64 * 16384 + 64 * 40) // len(pairs) + 1
    big = pairs * reps
    got, tp, rel = run_op(big, 10, known=known)
    one, tp1, rel1 = run_op(pairs, 10, known=known)
    check_pairs(pairs, 10, known=known)
    assert np.array_equal(got, np.tile(one, (reps, 1))) and np.array_equal(tp, np.tile(tp1, reps)) and np.array_equal(rel, np.tile(rel1, reps))


def test_rank_metrics_op_refuses_mistyped_tensors():
    import torch
    from rtrec_amd import ops as _registered        # noqa: F401
    op = torch.ops.rtrec_amd.rank_metrics
    z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=DEV)
    i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64

    def args(size=10, n=4, **over):
        disc, ideal = metrics.discount_tables(min(max(size, 1), 64))
        a = dict(ids=z(i32, n, 12), counts=z(i32, n), truth_ptr=z(i64, n + 1), truth_items=z(i32, 3), truth_len=z(i32, n),
                 discount=torch.from_numpy(disc).to(DEV), ideal=torch.from_numpy(ideal).to(DEV), size=size,
                 metrics=z(f64, n, 8), tp=z(i32, n), rel=z(i64, n))
        a.update(over)
        return list(a.values())
    bad_calls = [
        lambda: op(*args(ids=z(i64, 4, 12))),                     # ids int32
        lambda: op(*args(counts=z(i64, 4))),
        lambda: op(*args(truth_ptr=z(i32, 5))),                   # truth_ptr int64
        lambda: op(*args(truth_items=z(i64, 3))),
        lambda: op(*args(truth_len=z(i64, 4))),
        lambda: op(*args(discount=z(f32, 10))),                   # tables float64
        lambda: op(*args(metrics=z(f32, 4, 8))),
        lambda: op(*args(tp=z(i64, 4))),
        lambda: op(*args(rel=z(i32, 4))),
        lambda: op(*args(ids=z(i32, 4, 24)[:, ::2])),             # strided view
        lambda: op(*args(counts=z(i32, 8)[::2])),
        lambda: op(*args(truth_len=z(i32, 4).cpu())),             # host tensor
        lambda: op(*args(metrics=z(f64, 4, 8).cpu())),
        lambda: op(*args(size=0)),                                # size outside 1..64
        lambda: op(*args(size=65)),
        lambda: op(*args(size=13)),                               # ids.size(1) < size (and tables of another size)
        lambda: op(*args(ids=z(i32, 4, 8))),
        lambda: op(*args(truth_ptr=z(i64, 4))),                   # truth_ptr of the wrong length
        lambda: op(*args(truth_ptr=z(i64, 6))),
        lambda: op(*args(metrics=z(f64, 4, 7))),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
            pytest.fail(f"bad call {k} went through")
    a = args()
    op(*a)                                                        # a well-typed call goes through
    torch.cuda.synchronize()
    want = metrics._query_metrics([], [], 10)                     # four rows of "nothing recommended, nothing held out"
    assert a[-3].cpu().numpy().tolist() == [[want[c] for c in metrics.METRIC_COLUMNS]] * 4
    assert a[-2].cpu().numpy().tolist() == [0] * 4 and a[-1].cpu().numpy().tolist() == [0] * 4
    empty = args(n=0)
    op(*empty)                                                    # and so does an empty one
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- end to end

def _golden_frames():
    g = json.load(open(os.path.join(G, "evaluate.json")))["e2e"]
    cols = ("user", "item", "tstamp", "rating")
    return g, pd.DataFrame(dict(zip(cols, g["train"]))), pd.DataFrame(dict(zip(cols, g["test"])))


def _assert_same(rec, test, size, filter_interacted, recheck=True):
    """device == host: the dicts key for key (order included) and the per-user frames cell for cell."""
    host, host_frame = rec.evaluate(test, recommend_size=size, filter_interacted=filter_interacted, per_user=True)
    dev, dev_frame = rec.evaluate(test, recommend_size=size, filter_interacted=filter_interacted, on_device=True, per_user=True)
    assert list(dev) == list(host)
    for name in host:
        assert dev[name] == host[name], (size, filter_interacted, name, dev[name], host[name])
    assert isinstance(dev["tp"], int)
    assert dev == rec.evaluate(test, recommend_size=size, filter_interacted=filter_interacted, on_device=True)
    if recheck:           # per_user changes nothing about the dict
        assert host == rec.evaluate(test, recommend_size=size, filter_interacted=filter_interacted)
    pd.testing.assert_frame_equal(dev_frame, host_frame, check_exact=True)
    return host, dev


def test_evaluate_on_device_equals_the_host_path_and_the_reference_on_the_golden_model():
    """The recipe of tests/test_pipeline_cpu.py::_evaluate_against_golden (same frames, model_kwargs and fit call)."""
    from rtrec_amd import SLIM
    from rtrec_amd.recommender import Recommender
    g, train, test = _golden_frames()
    rec = Recommender(SLIM(**g["model_kwargs"]))
    rec.fit(train, batch_size=1000, parallel=False)
    assert rec.recommend_batch(g["users"], top_k=10) == g["recommend_top10"]
    for key, ref in g["evaluate"].items():
        size, fi = key.split("_")
        host, dev = _assert_same(rec, test, int(size), bool(int(fi)))
        assert set(dev) == set(ref) and dev["tp"] == ref["tp"] and host["tp"] == ref["tp"]
        for name in ref:
            assert dev[name] == pytest.approx(ref[name], rel=1e-12), (key, name)
            assert host[name] == pytest.approx(ref[name], rel=1e-12), (key, name)
    # a frame that adds never-seen users and items (cold-start lists; items that only count in len(ground_truth))
    rng = np.random.default_rng(4)
    top_u, top_i = int(train["user"].max()), int(train["item"].max())
    extra = pd.DataFrame({"user": rng.integers(top_u + 1, top_u + 40, 120), "item": rng.integers(0, top_i + 30, 120),
                          "tstamp": 0.0, "rating": 1.0})
    known_users_new_items = pd.DataFrame({"user": rng.integers(0, top_u + 1, 80), "item": rng.integers(top_i + 1, top_i + 30, 80),
                                          "tstamp": 0.0, "rating": 1.0})
    wider = pd.concat([test, extra, known_users_new_items], ignore_index=True).sample(frac=1.0, random_state=1)
    for size, fi in ((5, True), (10, False), (64, True)):
        host, dev = _assert_same(rec, wider, size, fi)
    assert host["tp"] > 0
    # the relevance words on request: bit i = the i-th recommendation is in the user's held-out list
    users, cols, tp, rel = rec.model._evaluate_device(wider["user"].to_numpy(), wider["item"].to_numpy(), 10, True, want_rel=True)
    truth = wider.groupby("user")["item"].apply(list).to_dict()
    lists = rec.recommend_batch(users.tolist(), top_k=10)
    assert users.tolist() == list(truth) and rel.dtype == np.uint64
    for u, word, hits, ranked in zip(users.tolist(), rel.tolist(), tp.tolist(), lists):
        assert word == sum(1 << p for p, item in enumerate(ranked) if item in truth[u]) and bin(word).count("1") == hits
    empty = rec.evaluate(test.iloc[:0], on_device=True)
    assert empty == rec.evaluate(test.iloc[:0]) and empty["ndcg"] == 0.0
    with pytest.raises(ValueError, match="negative integer user ids"):
        rec.evaluate(pd.DataFrame({"user": [-3, 1], "item": [1, 2]}), on_device=True)
    with pytest.raises(ValueError, match="item column is float64"):
        rec.evaluate(pd.DataFrame({"user": [1, 2], "item": [1.0, 2.0]}), on_device=True)
    with pytest.raises(ValueError, match="user_tags"):
        rec.evaluate(test, user_tags={1: ["x"]}, on_device=True)


def test_evaluate_on_device_with_string_ids_takes_the_dense_mode():
    from rtrec_amd import SLIM
    from rtrec_amd.recommender import Recommender
    g, train, test = _golden_frames()
    as_str = lambda df: df.assign(user=["u%d" % x for x in df["user"]], item=["i%d" % x for x in df["item"]])
    train, test = as_str(train), as_str(test)
    rec = Recommender(SLIM(**g["model_kwargs"]))
    rec.fit(train, batch_size=1000, parallel=False)
    assert rec.model.item_ids.pass_through is False
    for key in g["evaluate"]:
        size, fi = key.split("_")
        host, _ = _assert_same(rec, test, int(size), bool(int(fi)))
        assert host["tp"] > 0
    extra = pd.DataFrame({"user": ["nobody%d" % (x % 7) for x in range(40)], "item": ["i%d" % x for x in range(40)],
                          "tstamp": 0.0, "rating": 1.0})
    unseen_items = test.head(60).assign(item=["never%d" % x for x in range(60)])
    wider = pd.concat([test, extra, unseen_items], ignore_index=True).sample(frac=1.0, random_state=2)
    for size, fi in ((5, True), (10, False), (64, True)):      # 64 is more than the catalogue in dense mode is asked to rank short of
        _assert_same(rec, wider, size, fi)


def test_evaluate_on_device_at_size():
    """24,000 users, all named by a seeded held-out frame; sizes 10 (feature-row lists) and 50 (beyond them), filtering
    both ways: the dict and every user's nine figures equal the host path's."""
    from rtrec_amd import SLIM, synth
    from rtrec_amd.recommender import Recommender
    n_users, n_items = 24_000, 3_000
    X = synth.interaction_matrix(n_users, n_items, 700_000, seed=31).tocoo()
    rng = np.random.default_rng(32)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=12)
    m.add_interactions_columns(X.row.astype(np.int64), X.col.astype(np.int64), 1.7e9 + np.arange(X.nnz, dtype=np.float64),
                               X.data.astype(np.float64))
    m.bulk_fit(parallel=True, progress_bar=False)
    rec = Recommender(m)
    # every user once with a popular item (so there are hits), plus random rows, duplicates included
    pop = np.argsort(-np.bincount(X.col, minlength=n_items))[:200]
    users = np.concatenate([np.arange(n_users), rng.integers(0, n_users, 60_000)])
    items = np.concatenate([pop[rng.integers(0, len(pop), n_users)], rng.integers(0, n_items, 60_000)])
    order = rng.permutation(len(users))
    test = pd.DataFrame({"user": users[order], "item": items[order]})
    assert test["user"].nunique() == n_users
    for size in (10, 50):
        for fi in (True, False):
            host, dev = _assert_same(rec, test, size, fi, recheck=False)
            assert host["tp"] > 0 and 0.0 < host["auc"] < 1.0
