"""List quality (SLIM.list_quality_batch / recommend_quality, Recommender.evaluate(list_quality=True), csrc/list_quality.hip)
without a GPU: the definition as a plain-Python host model and a vectorised one, their properties on the golden fixture,
hand-written cases, the aggregators of utils/metrics.py; the model / facade layers end to end through the CPU stand-in backend
with `list_quality` supplied by the host model; the registration on the extension surface (include/rtrec_amd_ext.h) and the C
entry point's host-side checks.  The kernel is in tests/test_gpu_quality.py.

The definition (include/rtrec_amd_ext.h, "LIST QUALITY"): a position is counted when it lies below counts[r], its id lies in
[0, n_items) and no earlier counted position holds its id; sim(a, b) = fmax(|W[a, b]|, |W[b, a]|); s_p = the float32 sum from +0
of sim(id_p, id_q) over the counted q < p in ascending q, sim_sum = the float32 sum from +0 of the s_p in ascending p; linked = the
pairs with sim > 0; weight_sum = the float32 sum from +0 of item_weight[id_p]; every counted position adds 1 to exposure[id]."""
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from rtrec_amd.utils.metrics import (QUALITY_COLUMNS, QUALITY_KEYS, fsum_mean, gini, list_quality_figures, novelty_weights,
                                     quality_frame_columns, quality_summary)
from tests.test_diverse_host import DiverseOracleBackend, csc_of, fixture_pools, hand_cases
from tests.test_diverse_host import host_model_vectorised as mmr_model
from tests.test_explain_host import bits, golden
from tests.test_rerank_host import _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LAMBDAS = (1.0, 0.7, 0.5, 0.3)


# ---------------------------------------------------------------------------------------------- the host models
def host_model(W, ids, counts, item_weight=None):
    """THE DEFINITION, written for clarity: (n[B] int32, sim_sum[B] float32, linked[B] int32, weight_sum[B] float32,
    exposure[n_items] int32); W csc with sorted, distinct rows per column."""
    ids = np.asarray(ids)
    B, k = ids.shape
    I = W.shape[1]
    stored = {(int(j), int(i)): F32(v) for i in range(I) for j, v in zip(W.indices[W.indptr[i]:W.indptr[i + 1]],
                                                                          W.data[W.indptr[i]:W.indptr[i + 1]])}

    def sim(a, b):
        return np.fmax(np.abs(stored.get((a, b), F32(0.0))), np.abs(stored.get((b, a), F32(0.0))))

    n, linked = np.zeros(B, np.int32), np.zeros(B, np.int32)
    sim_sum, weight_sum = np.zeros(B, F32), np.zeros(B, F32)
    exposure = np.zeros(I, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            counted = []
            for p in range(min(max(int(counts[b]), 0), k)):
                i = int(ids[b, p])
                if 0 <= i < I and i not in counted:
                    counted.append(i)                                        # an item shown twice is judged once, at its first place
            total, wsum = F32(0.0), F32(0.0)
            for at, a in enumerate(counted):
                s = F32(0.0)
                for c in counted[:at]:                                       # ascending q: one rounded add each
                    v = sim(a, c)
                    s = F32(s + v)
                    linked[b] += bool(v > 0)
                total = F32(total + s)
                if item_weight is not None:
                    wsum = F32(wsum + F32(item_weight[a]))
                exposure[a] += 1
            n[b], sim_sum[b], weight_sum[b] = len(counted), total, wsum
    return n, sim_sum, linked, weight_sum, exposure


def similarity_matrix(W):
    """max(|W|, |W|^T) with NaN weights ignored, as a float32 CSR."""
    A = sp.csr_matrix(abs(sp.csc_matrix(W, dtype=F32)))
    A.data[np.isnan(A.data)] = 0.0
    S = A.maximum(A.T).tocsr()
    S.sort_indices()
    return S


def host_model_vectorised(W, ids, counts, item_weight=None, chunk=1 << 22):
    """The same function with numpy over rows and pairs: the pairs' similarities gathered into [rows, k, k], the ordered float32
    sums as np.cumsum (which adds one element after the other; a masked pair adds +0.0, which changes no non-negative sum).
    What the larger GPU cases and tools/quality_bench.py compare against."""
    ids, counts = np.asarray(ids), np.asarray(counts)
    B, k = ids.shape
    I = W.shape[1]
    S = similarity_matrix(W)
    dense = S.toarray() if I <= 4096 else None
    lower = np.tri(k, k, -1, dtype=bool)                                     # [p, q]: q < p
    n, linked = np.zeros(B, np.int32), np.zeros(B, np.int32)
    sim_sum, weight_sum = np.zeros(B, F32), np.zeros(B, F32)
    exposure = np.zeros(I, np.int64)
    step = max(1, chunk // max(k * k, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, B, step):
            rows = ids[lo:lo + step]
            valid = (np.arange(k)[None, :] < np.clip(counts[lo:lo + step], 0, k)[:, None]) & (rows >= 0) & (rows < I)
            same = (rows[:, :, None] == rows[:, None, :]) & valid[:, :, None] & valid[:, None, :] & lower[None]
            counted = valid & ~same.any(axis=2)
            safe = np.where(counted, rows, 0)
            a, c = np.broadcast_arrays(safe[:, :, None], safe[:, None, :])
            sims = dense[a, c] if dense is not None else np.asarray(S[a.ravel(), c.ravel()], dtype=F32).reshape(a.shape)
            M = np.where(counted[:, :, None] & counted[:, None, :] & lower[None], sims.astype(F32), F32(0.0))
            s = np.cumsum(M, axis=2, dtype=F32)[:, :, -1]
            sim_sum[lo:lo + step] = np.cumsum(s, axis=1, dtype=F32)[:, -1]
            linked[lo:lo + step] = (M > 0).sum(axis=(1, 2))
            n[lo:lo + step] = counted.sum(axis=1)
            if item_weight is not None:
                w = np.where(counted, np.asarray(item_weight, dtype=F32)[safe], F32(0.0))
                weight_sum[lo:lo + step] = np.cumsum(w, axis=1, dtype=F32)[:, -1]
            exposure += np.bincount(rows[counted], minlength=I)
    return n, sim_sum, linked, weight_sum, exposure.astype(np.int32)


NAMES = ("n", "sim_sum", "linked", "weight_sum", "exposure")


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the host model {w.shape}"
        bad = np.flatnonzero((bits(g) != bits(w)).ravel() if name in ("sim_sum", "weight_sum") else (g != w).ravel())
        assert bad.size == 0, f"{what}: {bad.size} {name} differ from the host model, first at flat index {int(bad[0])}: {g.ravel()[bad[0]]} != {w.ravel()[bad[0]]}"


_LISTS = {}


def fixture_lists(lam):
    """(W, ids[240, 10] int32, counts[240], novelty[400] float32): the 240 fixture users' top-10 of their pool of 50 at `lam`
    (tests.test_diverse_host.host_model_vectorised), and the novelty table of the fixture's X.  Computed once per lambda."""
    if lam not in _LISTS:
        W, pool_ids, scores, counts, _, _ = fixture_pools()
        order, _, _, count = mmr_model(W, pool_ids, scores, counts, 10, F32(lam))
        ids = np.where(order >= 0, np.take_along_axis(pool_ids, np.maximum(order, 0), axis=1), -1).astype(np.int32)
        X = golden()[0]
        weight = novelty_weights(np.diff(sp.csc_matrix(X).indptr), X.shape[0], W.shape[1])
        for a in (ids, count, weight):
            a.setflags(write=False)
        _LISTS[lam] = (W, ids, count, weight)
    return _LISTS[lam]


_WANT = {}


def fixture_want(lam):
    """The vectorised host model's answer on fixture_lists(lam), computed once and shared."""
    if lam not in _WANT:
        W, ids, counts, weight = fixture_lists(lam)
        _WANT[lam] = host_model_vectorised(W, ids, counts, weight)
        for a in _WANT[lam]:
            a.setflags(write=False)
    return _WANT[lam]


def hand_w():
    """The W of tests.test_diverse_host.hand_cases() -- sim(0, 1) = 2 stored on one side, sim(0, 2) = 1 on the other, sim(0, 3) = 3
    from W[0, 3] = 0.25 against W[3, 0] = -3, sim(2, 3) = 0.125, W[5, 0] = inf, W[4, 0] = NaN against W[0, 4] = 0.5 -- plus two
    explicit zeros between items 6 and 7 (a positive and a negative one)."""
    W = hand_cases()[0][1]
    entries = {(int(j), i): W.data[p] for i in range(W.shape[1]) for p, j in zip(range(W.indptr[i], W.indptr[i + 1]), W.indices[W.indptr[i]:W.indptr[i + 1]])}
    entries.update({(6, 7): 0.0, (7, 6): -0.0})
    return csc_of(entries, 8)


HAND_WEIGHT = (0.25 + 0.5 * np.arange(8)).astype(F32)                        # item i weighs 0.25 + i / 2: every sum below is exact


def hand_quality_cases():
    """(name, ids row, count, n, sim_sum, linked, weight_sum) over hand_w() and HAND_WEIGHT."""
    inf = float("inf")
    return [
        ("similarity stored as W[0, 1] only", [0, 1], 2, 2, 2.0, 1, 1.0),
        ("similarity stored as W[2, 0] only", [0, 2], 2, 2, 1.0, 1, 1.5),
        ("the same pair in the other order", [2, 0], 2, 2, 1.0, 1, 1.5),
        ("both sides stored, the negative one larger", [0, 3], 2, 2, 3.0, 1, 2.0),
        ("a NaN weight is ignored, the other side counts", [0, 4], 2, 2, 0.5, 1, 2.5),
        ("a count of 1 leaves one item and no pair", [4, 0, 6], 1, 1, 0.0, 0, 2.25),
        ("an inf weight", [0, 5], 2, 2, inf, 1, 3.0),
        ("an inf weight stays inf under the later adds", [0, 5, 1], 3, 3, inf, 2, 3.75),
        ("explicit zeros on both sides are not a link", [6, 7], 2, 2, 0.0, 0, 7.0),
        ("four items: s = 0, 2, 1, 3.125", [0, 1, 2, 3], 4, 4, 6.125, 4, 4.0),
        ("duplicated ids are counted once, at their first place", [0, 1, 0, 1, 3, 3], 6, 3, 5.0, 2, 2.75),
        ("ids -1 and n_items are not counted", [-1, 0, 8, 3, 9], 5, 2, 3.0, 1, 2.0),
        ("a count below 0", [0, 1, 2], -3, 0, 0.0, 0, 0.0),
        ("a count above list_k", [0, 1, 2], 99, 3, 3.0, 2, 2.25),
        ("a count that cuts the list", [0, 1, 2], 2, 2, 2.0, 1, 1.0),
        ("m = 0", [-1, 8, -5], 3, 0, 0.0, 0, 0.0),
        ("m = 1", [3, 3, 3], 3, 1, 0.0, 0, 1.75),
    ]


def hand_batch():
    """The hand-written cases as one batch: (W, ids[B, 6], counts[B], want in NAMES order)."""
    cases = hand_quality_cases()
    ids = np.full((len(cases), 6), -1, np.int32)
    for b, case in enumerate(cases):
        ids[b, :len(case[1])] = case[1]
    counts = np.array([c[2] for c in cases], np.int32)
    exposure = np.zeros(8, np.int32)
    for case in cases:
        seen = []
        for i in case[1][:max(case[2], 0)]:
            if 0 <= i < 8 and i not in seen:
                seen.append(i)
        exposure[seen] += 1
    want = (np.array([c[3] for c in cases], np.int32), np.array([c[4] for c in cases], F32), np.array([c[5] for c in cases], np.int32),
            np.array([c[6] for c in cases], F32), exposure)
    return hand_w(), ids, counts, want


class QualityOracleBackend(DiverseOracleBackend):
    """The CPU stand-in (with score_pairs and diversify_lists from their host models) plus list_quality from the host model
    (TEST-ONLY, like its bases)."""

    def list_quality(self, n_items, W, ids, counts, list_k, item_weight, exposure, n, sim_sum, linked, weight_sum, waves_per_row=0):
        import torch
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        out = host_model_vectorised(Wc, ids.numpy()[:, :list_k], counts.numpy(), None if item_weight is None else item_weight.numpy())
        for dst, src in zip((n, sim_sum, linked, weight_sum), out):
            dst.copy_(torch.from_numpy(src))
        if exposure is not None:
            exposure += torch.from_numpy(out[4])                             # added to, never zeroed


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=QualityOracleBackend())
    return m


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


def model_parts(m):
    """(W csc sorted, the novelty table of the model's X) from the host copies."""
    W = m.model.item_similarity.tocsc()
    W.sort_indices()
    X = sp.csc_matrix(m.interactions.to_csr())
    return W, novelty_weights(np.diff(X.indptr), X.shape[0], W.shape[1])


def expected_summary(m, lists):
    """quality_summary (and the raw arrays) of `lists` (raw item ids per list) from the host copies and the plain host model."""
    W, weight = model_parts(m)
    k = max([len(r) for r in lists] + [1])
    ids = np.full((len(lists), k), -1, np.int32)
    for b, row in enumerate(lists):
        ids[b, :len(row)] = [-1 if (i := m.item_ids.get_id(x)) is None else i for x in row]
    raw = host_model(W, ids, [len(r) for r in lists], weight)
    return quality_summary(*raw), raw


def same_dict(got, want):
    """== key for key, in order, with NaN equal to NaN."""
    assert list(got) == list(want), (list(got), list(want))
    for key in want:
        g, w = got[key], want[key]
        assert (g == w) or (isinstance(w, float) and math.isnan(w) and math.isnan(g)), f"{key}: {g!r} != {w!r}"


# ---------------------------------------------------------------------------------------------- the definition
def test_vectorised_model_is_the_definition_on_a_mutilated_fixture():
    W, ids, _, weight = fixture_lists(0.7)
    pool = fixture_pools()[1]
    rng = np.random.default_rng(43)
    for rows in (ids.copy(), pool[:60].copy()):                              # lists of 10, and of 50 (pairs that are linked and not)
        rows[rng.random(rows.shape) < 0.05] = -1
        rows[3, 4], rows[7, 0] = W.shape[1], W.shape[1] + 7
        rows[:, 8] = rows[:, 2]                                              # duplicates, one of them in front
        rows[:, 1] = rows[:, 6]
        counts = rng.integers(-2, rows.shape[1] + 4, len(rows)).astype(np.int32)
        want = host_model(W, rows, counts, weight)
        assert_same(host_model_vectorised(W, rows, counts, weight), want, f"lists of {rows.shape[1]}")
        assert_same(host_model_vectorised(W, rows, counts, weight, chunk=1), want, "row by row")
        assert want[0].min() == 0 and want[0].max() >= 8 and want[4].sum() == want[0].sum()
        none = host_model_vectorised(W, rows, counts)
        assert_same(none, host_model(W, rows, counts), "no weight")
        assert not none[3].any() and not np.signbit(none[3]).any()


def test_fixture_properties_along_the_diversity_curve():
    mean_ils, distinct = [], []
    for lam in LAMBDAS:
        W, ids, counts, weight = fixture_lists(lam)
        n, sim_sum, linked, weight_sum, exposure = fixture_want(lam)
        assert ids.shape == (240, 10) and (counts == 10).all() and (n == 10).all()
        assert (linked >= 1).all(), f"lambda={lam}: a list without a linked pair"
        ils, share, nov = list_quality_figures(n, sim_sum, linked, weight_sum)
        assert np.isfinite(ils).all() and (share > 0).all() and (share <= 1).all() and np.isfinite(nov).all() and (nov >= 0).all()
        summary = quality_summary(n, sim_sum, linked, weight_sum, exposure)
        assert summary["n_lists"] == summary["n_lists_pairs"] == 240 and summary["mean_length"] == 10.0
        assert summary["distinct_items"] == int((exposure > 0).sum()) and summary["coverage"] == summary["distinct_items"] / 400
        assert exposure.sum() == 2400 and 0.0 < summary["gini"] < 1.0
        mean_ils.append(summary["intra_list_similarity"])
        distinct.append(summary["distinct_items"])
    assert all(a > b for a, b in zip(mean_ils, mean_ils[1:])), mean_ils      # diversity lowers the intra-list similarity ...
    assert all(a < b for a, b in zip(distinct, distinct[1:])), distinct      # ... and widens what the lists show of the catalogue
    assert [round(v, 6) for v in mean_ils] == [0.025108, 0.023737, 0.021347, 0.016256] and distinct == [145, 159, 190, 233]
    assert_same(host_model(*fixture_lists(0.5)), fixture_want(0.5), "lambda=0.5")


def test_the_order_of_the_float32_additions_has_teeth_on_the_fixture():
    W, ids, counts, _ = fixture_lists(1.0)
    S = similarity_matrix(W).toarray().astype(np.float64)
    sim_sum = fixture_want(1.0)[1]
    once = np.array([F32(math.fsum(S[a, c] for at, a in enumerate(row) for c in row[:at])) for row in ids.tolist()])
    differ = int((bits(sim_sum) != bits(once)).sum())
    assert differ > 50, differ                                               # a kernel that adds in another order cannot pass by bits
    assert np.allclose(sim_sum, once, rtol=1e-5, atol=0)


def test_hand_written_cases():
    W, ids, counts, want = hand_batch()
    assert np.isnan(W[4, 0]) and np.isinf(W[5, 0]) and W.nnz == 10 and (W.data == 0).sum() == 2
    for model in (host_model, host_model_vectorised):
        assert_same(model(W, ids, counts, HAND_WEIGHT), want, model.__name__)
        got = model(W, ids, counts)
        assert_same(got[:3], want[:3], "no weight")
        assert not got[3].any() and np.array_equal(got[4], want[4])
    for b, (name, row, count, n, sim_sum, linked, weight_sum) in enumerate(hand_quality_cases()):   # ... and one list at a time
        got = host_model(W, np.array([row], np.int32), [count], HAND_WEIGHT)
        assert (int(got[0][0]), float(got[1][0]), int(got[2][0]), float(got[3][0])) == (n, sim_sum, linked, weight_sum), name


# ---------------------------------------------------------------------------------------------- the aggregators
def test_gini_of_uniform_and_one_hot_exposures():
    for n in (1, 2, 7, 400):
        assert gini(np.full(n, 3)) == 0.0
        one = np.zeros(n, np.int32)
        one[n // 2] = 5
        assert gini(one) == (n - 1) / n
    assert math.isnan(gini(np.zeros(9, np.int32))) and math.isnan(gini(np.zeros(0, np.int32)))
    assert gini([1, 2, 3, 4]) == (-3 * 1 - 1 * 2 + 1 * 3 + 3 * 4) / (4 * 10) and gini([4, 1, 3, 2]) == gini([1, 2, 3, 4])
    big = np.array([2 ** 40, 2 ** 41, 0, 2 ** 42], np.int64)                # beyond what int64 holds once multiplied: exact all the same
    assert gini(np.tile(big, 1 << 10)) == gini(big) == ((-3 * 0 - 2 ** 40 + 2 ** 41 + 3 * 2 ** 42) / (4 * 7 * 2 ** 40))


def test_nan_rules_and_fsum_means():
    n = np.array([0, 1, 2, 3, 10], np.int32)
    sim_sum = np.array([0, 0, 0.5, 1.5, np.inf], F32)
    linked = np.array([0, 0, 1, 2, 45], np.int32)
    weight_sum = np.array([0, 2.5, 3, 1, 5], F32)
    ils, share, nov = list_quality_figures(n, sim_sum, linked, weight_sum)
    assert np.isnan(ils[:2]).all() and ils[2:].tolist() == [0.5, 0.5, np.inf]
    assert np.isnan(share[:2]).all() and share[2:].tolist() == [1.0, 2 / 3, 1.0]
    assert np.isnan(nov[0]) and nov[1:].tolist() == [2.5, 1.5, 1 / 3, 0.5]
    assert ils.dtype == share.dtype == nov.dtype == np.float64
    s = quality_summary(n[:4], sim_sum[:4], linked[:4], weight_sum[:4], np.array([0, 3, 0, 1, 2]))
    assert list(s) == list(QUALITY_KEYS)
    assert (s["n_lists"], s["n_lists_nonempty"], s["n_lists_pairs"], s["mean_length"]) == (4, 3, 2, 1.5)
    assert s["intra_list_similarity"] == 0.5 and s["linked_share"] == math.fsum([1.0, 2 / 3]) / 2 and s["novelty"] == math.fsum([2.5, 1.5, 1 / 3]) / 3
    assert (s["distinct_items"], s["coverage"]) == (3, 0.6) and s["gini"] == gini([0, 3, 0, 1, 2])
    empty = quality_summary(n[:1], sim_sum[:1], linked[:1], weight_sum[:1], np.zeros(5, np.int32))
    assert empty["n_lists"] == 1 and empty["n_lists_pairs"] == 0 and empty["mean_length"] == 0.0 and empty["distinct_items"] == 0 and empty["coverage"] == 0.0
    assert all(math.isnan(empty[key]) for key in ("intra_list_similarity", "linked_share", "novelty", "gini"))
    nothing = quality_summary(n[:0], sim_sum[:0], linked[:0], weight_sum[:0], np.zeros(0, np.int32))
    assert nothing["n_lists"] == 0 and all(math.isnan(nothing[key]) for key in ("mean_length", "coverage", "gini", "novelty"))
    # the mean is the exactly rounded sum over the count: no order changes it, where a running sum does
    values = np.array([1e16, 1.0, -1e16, 1.0, 3.0, 1e-3] * 50)
    rng = np.random.default_rng(3)
    means = {fsum_mean(rng.permutation(values)) for _ in range(20)}
    assert means == {math.fsum(values.tolist()) / len(values)} and len({float(np.cumsum(rng.permutation(values))[-1]) for _ in range(20)}) > 1
    assert math.isnan(fsum_mean(np.zeros(0))) and fsum_mean([np.inf, 1.0]) == np.inf and math.isnan(fsum_mean([np.inf, -np.inf]))
    cols = quality_frame_columns(n, sim_sum, linked, weight_sum)
    assert list(cols) == list(QUALITY_COLUMNS) and cols["n"].dtype == cols["linked_pairs"].dtype == np.int64


def test_novelty_table_is_rounded_once_and_follows_the_width_of_w():
    pop = np.array([0, 1, 2, 3, 8, 5])
    w = novelty_weights(pop, 8, 6)
    assert w.dtype == F32 and w.tolist() == [3.0, 3.0, 2.0, float(F32(3.0 - math.log2(3))), 0.0, float(F32(3.0 - math.log2(5)))]
    assert bits(novelty_weights(pop, 8, 4)).tolist() == bits(w[:4]).tolist()             # cut to W's items ...
    assert novelty_weights(pop, 8, 9).tolist() == w.tolist() + [3.0] * 3                  # ... or padded: never seen weighs like seen once
    big = novelty_weights(np.array([3]), 138493, 1)
    assert bits(big)[0] == bits(F32(math.log2(138493) - math.log2(3))) and novelty_weights(pop, 0, 2).tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _some_lists(m, batch, strings):
    rng = np.random.default_rng(14)
    known = sorted({i for _, i, _, _ in batch}, key=str)
    unknown = "never seen" if strings else 10 ** 7
    lists = []
    for b in range(12):
        row = [known[j] for j in rng.permutation(len(known))[:int(rng.integers(1, 40))]]
        row.insert(int(rng.integers(0, len(row) + 1)), unknown)
        if b % 3 == 0:
            row.append(row[0])                                               # an item listed twice
        lists.append(row)
    return lists + [[], [unknown], [known[0]], [known[0], known[0]]], known, unknown


@pytest.mark.parametrize("strings", [False, True])
def test_list_quality_batch_takes_raw_ids_and_needs_no_user(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    lists, known, unknown = _some_lists(m, batch, strings)
    summary, raw = expected_summary(m, lists)
    got = m.list_quality_batch(lists, as_arrays=True)
    assert len(got) == 5 and got[4].shape == (m.model.n_items_fitted,)
    assert_same(got, raw, f"list_quality_batch strings={strings}")
    assert raw[2].sum() > 10 and raw[0][-4:].tolist() == [0, 0, 1, 1] and raw[0][0] == len(set(lists[0])) - 1
    dicts = m.list_quality_batch(lists)
    ils, _, nov = list_quality_figures(*raw[:4])
    for b, d in enumerate(dicts):
        assert list(d) == list(QUALITY_COLUMNS) and d["n"] == raw[0][b] and d["linked_pairs"] == raw[2][b]
        same_dict(d, {"n": int(raw[0][b]), "intra_list_similarity": float(ils[b]), "linked_pairs": int(raw[2][b]), "novelty": float(nov[b])})
    assert math.isnan(dicts[-4]["novelty"]) and math.isnan(dicts[-2]["intra_list_similarity"]) and dicts[-2]["novelty"] >= 0
    same_dict(m.list_quality(lists[1]), dicts[1])
    rec = Recommender(m)
    same_dict(rec.list_quality(lists[2]), dicts[2])
    assert_same(rec.list_quality_batch(lists, as_arrays=True), raw, "Recommender.list_quality_batch")
    assert m.list_quality_batch([]) == [] and m.list_quality_batch([], as_arrays=True)[0].shape == (0,)
    # the engine's forms: host arrays with a weight of the caller's, or none, and no exposure
    eng = m.model.engine
    W, weight = model_parts(m)
    ids = np.array([[m.item_ids.get_id(known[j]) for j in (0, 1, 2, 3)], [m.item_ids.get_id(known[j]) for j in (4, 5, 6, 6)]], np.int32)
    mine = np.arange(W.shape[1], dtype=F32)
    assert_same(eng.list_quality_lists(ids, item_weight=mine), host_model(W, ids, [4, 4], mine), "a weight of the caller's")
    out = eng.list_quality_lists(ids, counts=np.array([2, 9]), with_exposure=False)
    assert out[4] is None and not out[3].any()
    assert_same(out[:4], host_model(W, ids, [2, 9])[:4], "no weight, no exposure")
    # the novelty table is built once per X and dropped with it
    table = eng.item_novelty_device()
    assert eng.item_novelty_device() is table and bits(table.numpy()).tolist() == bits(weight).tolist()
    eng.set_interactions(None, m.interactions.to_csr(), need_csc=True)       # (the CSC orientation resident: col_nnz instead of a count)
    assert eng.item_novelty_device() is not table and bits(eng.item_novelty_device().numpy()).tolist() == bits(weight).tolist()


@pytest.mark.parametrize("strings", [False, True])
def test_recommend_quality_is_composed_of_the_lists_the_users_are_served(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    known = sorted({u for u, _, _, _ in batch}, key=str)
    cold = "nobody" if strings else max(known) + 1000
    users = known[:25] + [cold, known[3], cold]
    rec = Recommender(m)
    plain = m.recommend_batch(users, top_k=6)
    want, raw = expected_summary(m, plain)
    got, frame = m.recommend_quality(users, top_k=6, per_user=True)
    same_dict(got, want)
    assert got["n_lists"] == len(users) and 5.0 < got["mean_length"] <= 6.0 and 0 < got["coverage"] < 1 and got["intra_list_similarity"] > 0
    same_dict(m.recommend_quality(users, top_k=6), want)
    same_dict(m.recommend_quality(users, top_k=6, diversity=0.0, pool=3), want)          # (pool is not read without diversity)
    assert list(frame.columns) == list(QUALITY_COLUMNS) and frame.index.name == "user" and frame.index.tolist() == users
    cols = quality_frame_columns(*raw[:4])
    for name in QUALITY_COLUMNS:
        assert np.array_equal(frame[name].to_numpy(), cols[name], equal_nan=True), name
    # diversity: recommend_diverse_batch's lists, through its as_arrays form (internal ids) and through its raw lists
    ids, _, cnt, _, _ = m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.5, as_arrays=True)
    W, weight = model_parts(m)
    arrays = host_model(W, ids, cnt, weight)
    diverse, _ = expected_summary(m, m.recommend_diverse_batch(users, top_k=6, pool=30, diversity=0.5))
    same_dict(diverse, quality_summary(*arrays))
    got = m.recommend_quality(users, top_k=6, diversity=0.5, pool=30)
    same_dict(got, diverse)
    assert got["intra_list_similarity"] < want["intra_list_similarity"]                  # the knob does what it says on this model too
    same_dict(rec.recommend_quality(users, top_k=6, diversity=0.5, pool=30), diverse)
    same_dict(rec.recommend_quality(users, top_k=6, diversity=0.5, pool=30, per_user=True)[0], diverse)
    # filter_interacted reaches the scoring pass
    unfiltered, _ = expected_summary(m, m.recommend_batch(users, top_k=6, filter_interacted=False))
    same_dict(m.recommend_quality(users, top_k=6, filter_interacted=False), unfiltered)
    assert unfiltered != want
    unfiltered, _ = expected_summary(m, m.recommend_diverse_batch(users, top_k=4, pool=9, diversity=0.3, filter_interacted=False))
    same_dict(m.recommend_quality(users, top_k=4, pool=9, diversity=0.3, filter_interacted=False), unfiltered)
    # only unknown users; nobody
    same_dict(m.recommend_quality([cold, cold], top_k=6), expected_summary(m, m.recommend_batch([cold, cold], top_k=6))[0])
    none = m.recommend_quality([], top_k=6)
    assert none["n_lists"] == 0 and none["distinct_items"] == 0 and math.isnan(none["gini"]) and math.isnan(none["mean_length"])


def test_every_refusal_of_the_public_calls():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.recommender import Recommender
    fresh = cpu_slim()
    for call in (lambda: fresh.list_quality_batch([[1]]), lambda: fresh.list_quality([1]), lambda: fresh.recommend_quality([1]),
                 lambda: fresh.recommend_quality([1], diversity=0.3)):
        with pytest.raises(RuntimeError, match="Model must be fitted"):
            call()
    m, batch = _model()
    users = sorted({u for u, _, _, _ in batch})[:4]
    items = sorted({i for _, i, _, _ in batch})
    with pytest.raises(ValueError, match="up to 1024 items, got a list of 1025"):
        m.list_quality_batch([[items[j % len(items)] for j in range(1025)]])
    assert m.list_quality_batch([[items[j % len(items)] for j in range(1024)]])[0]["n"] == len(items)
    # recommend_quality: recommend_diverse_batch's refusals once diversity is asked for
    for kw in (dict(top_k=0), dict(top_k=11, pool=10), dict(pool=1025, top_k=10), dict(top_k=-1), dict(pool=0, top_k=0)):
        with pytest.raises(ValueError, match="recommend_quality needs 1 <= top_k <= pool <= 1024"):
            m.recommend_quality(users, diversity=0.3, **kw)
        with pytest.raises(ValueError, match="needs 1 <= top_k <= pool <= 1024"):
            m.recommend_diverse_batch(users, **kw)
    for d in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"recommend_quality: diversity must lie in \[0, 1\]"):
            m.recommend_quality(users, diversity=d)
    for top_k in (0, -1, 1025):
        with pytest.raises(ValueError, match="recommend_quality needs 1 <= top_k <= 1024"):
            m.recommend_quality(users, top_k=top_k)
    assert m.recommend_quality(users, top_k=1, pool=1, diversity=1.0)["mean_length"] == 1.0
    eng = m.model.engine
    eng.topk_supported = lambda top_k, mode: top_k < 40
    try:
        assert m.recommend_quality(users, top_k=5, pool=39, diversity=0.3) and m.recommend_quality(users, top_k=39)
        with pytest.raises(ValueError, match="recommend_quality: .* do not serve lists of pool=40 .* smaller pool"):
            m.recommend_quality(users, top_k=5, pool=40, diversity=0.3)
        with pytest.raises(ValueError, match="recommend_quality: .* do not serve lists of top_k=40"):
            m.recommend_quality(users, top_k=40)
    finally:
        del eng.topk_supported
    # a float64 W holding float32 numbers is served with them; one holding other numbers is refused
    W = m.model.item_similarity
    lists = [items[:8], items[4:20]]
    want = m.list_quality_batch(lists, as_arrays=True)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)
    assert_same(m.list_quality_batch(lists, as_arrays=True), want, "a float64 W of float32 numbers")
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    for call in (lambda: m.list_quality_batch(lists), lambda: m.recommend_quality(users), lambda: m.recommend_quality(users, diversity=0.3)):
        with pytest.raises(ValueError, match="not float32 numbers"):
            call()
    m.model.item_similarity = W
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=QualityOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    with pytest.raises(ValueError, match=r"list quality needs the whole of W .* gather_item_similarity\(\)"):
        eng.list_quality_lists(np.array([[1, 2]], np.int32))
    mine = m.model._engine
    m.model._engine = eng
    m.model._sync_weights = lambda: None
    try:
        for call in (lambda: m.list_quality_batch(lists), lambda: m.recommend_quality(users), lambda: m.recommend_quality(users, diversity=0.3)):
            with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
                call()
    finally:
        del m.model._sync_weights
        m.model._engine = mine
    # the engine's own ranges
    m.model._sync_weights()
    eng = m.model.engine
    n_w = m.model.n_items_fitted
    with pytest.raises(ValueError, match="lists of 1..1024 items"):
        eng.list_quality_lists(np.zeros((2, 0), np.int32))
    with pytest.raises(ValueError, match="lists of 1..1024 items"):
        eng.list_quality_lists(np.zeros((1, 1025), np.int32))
    with pytest.raises(ValueError, match=r"\[B, k\]"):
        eng.list_quality_lists(np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="one entry per row"):
        eng.list_quality_lists(np.zeros((2, 3), np.int32), counts=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="item_weight must hold one entry per item"):
        eng.list_quality_lists(np.zeros((2, 3), np.int32), item_weight=np.zeros(n_w + 1, F32))
    with pytest.raises(ValueError, match="not both"):
        eng.list_quality_lists(np.zeros((2, 3), np.int32), item_weight=np.zeros(n_w, F32), novelty=True)
    with pytest.raises(ValueError, match="exposure must hold one entry per item"):
        eng.list_quality_device(eng._up(np.zeros((2, 3), np.int32)), eng._up(np.zeros(2, np.int32)), exposure=eng._up(np.zeros(n_w - 1, np.int32)))
    # evaluate: the new arguments belong to the device path, and that path needs the device
    rec = Recommender(m)
    test = pd.DataFrame({"user": [u for u, _, _, _ in batch[:40]], "item": [i for _, i, _, _ in batch[:40]]})
    before = rec.evaluate(test)
    for kw in (dict(diversity=0.3), dict(list_quality=True), dict(diversity=0.3, list_quality=True, per_user=True)):
        with pytest.raises(ValueError, match="on_device=True"):
            rec.evaluate(test, **kw)
        with pytest.raises(ValueError, match="needs the HIP backend"):
            rec.evaluate(test, on_device=True, **kw)
    assert rec.evaluate(test, diversity=0.0, pool=7, list_quality=False) == before


# ---------------------------------------------------------------------------------------------- registration
def test_list_quality_is_declared_registered_and_exported():
    import ctypes
    import torch
    from rtrec_amd import _native, build, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read(), flags=re.S)
    assert "rtrec_slim_list_quality" in re.findall(r"\b(rtrec_[a-z0-9_]+)\s*\(", text)
    core = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtrec_amd.h")).read(), flags=re.S)
    assert "list_quality" not in core and "rtrec_slim_list_quality" not in _native.EXPORTS
    assert "rtrec_slim_list_quality" in _native.EXT_EXPORTS and "list_quality.hip" in build.SOURCES
    assert "list_quality" in ops.EXT_OPS and "list_quality" not in ops.OPS and ops.EXT_EXPORT_OF["list_quality"] == "rtrec_slim_list_quality"
    assert hasattr(ctypes.CDLL(build.LIB_PATH), "rtrec_slim_list_quality")
    assert len(_native.load().rtrec_slim_list_quality.argtypes) == 18
    schema = str(torch.ops.rtrec_amd.list_quality.default._schema)
    assert schema.startswith("rtrec_amd::list_quality(") and schema.endswith("-> ()")
    for name in ("n", "sim_sum", "linked", "weight_sum"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    assert re.search(r"Tensor\([a-z]!\)\? exposure\b", schema), schema
    for name in ("wc_ptr", "wc_row", "wc_val", "ids", "counts"):
        assert f"Tensor {name}" in schema, schema
    assert "Tensor? item_weight" in schema and "int list_k" in schema and "int waves_per_row" in schema and "int n_items" in schema
    assert schema.count("!") == 5
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.list_quality(i32(4), i32(1), torch.zeros(1), 3, i32(1, 2), i32(1), 2, None, 0, i32(1), torch.zeros(1), i32(1),
                                             torch.zeros(1), None)
    # no Python file of the package calls the symbol by raw ctypes
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):
        for f in files:
            if f.endswith(".py") and f != "_native.py":
                assert ".rtrec_slim_list_quality(" not in open(os.path.join(dirpath, f)).read(), f


def test_the_entry_point_checks_its_arguments_on_the_host():
    from rtrec_amd import _native
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    fn = _native.load().rtrec_slim_list_quality
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_rows=1, n_items=5, wptr=one, wrow=one, wval=one, nnz=0, ids=one, istride=10, list_k=10, counts=one, weight=one, exposure=one, \
        waves=0, n=one, sim_sum=one, linked=one, weight_sum=one: (
        n_rows, n_items, wptr, wrow, wval, nnz, ids, istride, list_k, counts, weight, exposure, waves, n, sim_sum, linked, weight_sum, None)
    for kw in (dict(list_k=0), dict(list_k=-1), dict(list_k=1025, istride=1025), dict(waves=2), dict(waves=-1), dict(waves=8)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_rows=-1), dict(n_items=-1), dict(nnz=-1), dict(istride=9), dict(ids=None), dict(counts=None), dict(n=None),
               dict(sim_sum=None), dict(linked=None), dict(weight_sum=None), dict(wptr=None), dict(nnz=3, wrow=None), dict(nnz=3, wval=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_items=0, wptr=None, wrow=None, wval=None, n_rows=0)) == 0          # an empty W needs no arrays
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, ids=None, counts=None, n=None, weight=None, exposure=None)) == 0
    for name in ("list_quality_device", "list_quality_lists", "item_novelty_device"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "list_quality"))
