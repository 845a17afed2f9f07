"""Explanations (SLIM.explain_batch, csrc/explain.hip) without a GPU: the definition as a numpy host model, pinned to the
reference's scores on the golden fixture; the model / facade / serving layers end to end through the CPU stand-in backend
with `explain_topk` supplied by the host model; the registration of the op.  The kernel itself is in tests/test_gpu_explain.py.

The definition (include/rtrec_amd.h, "EXPLANATIONS"): for a user row u and an item i the contributing items are the j stored in
both row u of X and column i of W, c(j) = float32(x_uj) * float32(w_ji) in float32, support = their number, reasons = the top_m
by c descending, the lower item id first among equal c.  A NaN contribution counts in support and is never a reason; +-inf
are numbers; +0.0 and -0.0 are equal and each keeps its sign bit.  The value-edge cases (`edge_case`) and the mutated models
that show they bite are at the end of the definition's section; tests/test_gpu_explain.py runs the same cases on the kernel."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.cpu_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------------------------------------- the host model
def pair_contributions(X: sp.csr_matrix, W: sp.csc_matrix, row: int, item: int):
    """(j ascending, c float32) of one (user row, item) pair; X / W with sorted indices."""
    if not (0 <= row < X.shape[0] and 0 <= item < W.shape[1]):
        return np.empty(0, np.int64), np.empty(0, np.float32)
    xs, xv = X.indices[X.indptr[row]:X.indptr[row + 1]], X.data[X.indptr[row]:X.indptr[row + 1]].astype(np.float32)
    wj, ww = W.indices[W.indptr[item]:W.indptr[item + 1]], W.data[W.indptr[item]:W.indptr[item + 1]].astype(np.float32)
    common, xi, wi = np.intersect1d(xs, wj, assume_unique=True, return_indices=True)
    with np.errstate(all="ignore"):                                     # inf * 0, overflow, underflow: the values under test
        return common.astype(np.int64), xv[xi] * ww[wi]                 # float32 * float32: one rounding


def host_model(X, W, rows, ids, counts, top_m):
    """THE DEFINITION: (reason_items[B, k, top_m] int32, contributions[B, k, top_m] float32, support[B, k] int32), -1 / -inf
    padded.  A slot at or beyond counts[b], an item outside [0, n_items) and a row outside [0, n_users) are empty.  A NaN
    contribution counts in support and is never a reason: the reasons are ranked among the contributions that are numbers
    (+-inf included; +0.0 == -0.0, so the two go by item id), and the slots from their number on are padding."""
    ids = np.asarray(ids)
    B, k = ids.shape
    items = np.full((B, k, top_m), -1, np.int32)
    contrib = np.full((B, k, top_m), -np.inf, np.float32)
    support = np.zeros((B, k), np.int32)
    for b in range(B):
        for p in range(min(max(int(counts[b]), 0), k)):
            j, c = pair_contributions(X, W, int(rows[b]), int(ids[b, p]))
            support[b, p] = len(j)                                      # NaN contributions included
            j, c = j[~np.isnan(c)], c[~np.isnan(c)]
            order = np.lexsort((j, -c))[:top_m]                         # c descending, then the lower item id
            items[b, p, :len(order)], contrib[b, p, :len(order)] = j[order], c[order]
    return items, contrib, support


def host_model_vectorised(X, W, rows, ids, counts, top_m, chunk=8192):
    """The same function without a Python loop per pair (scipy / numpy over all pairs of a chunk of users): what the full-size
    GPU test and tools/explain_bench.py compare and time the kernel against."""
    ids, rows, counts = np.asarray(ids), np.asarray(rows, dtype=np.int64), np.asarray(counts)
    B, k = ids.shape
    U, I = X.shape[0], W.shape[1]
    items = np.full((B, k, top_m), -1, np.int32)
    contrib = np.full((B, k, top_m), -np.inf, np.float32)
    support = np.zeros((B, k), np.int32)
    xkey = np.repeat(np.arange(U, dtype=np.int64), np.diff(X.indptr)) * I + X.indices        # ascending: X is a sorted CSR
    xval = X.data.astype(np.float32)
    wptr, wlen = W.indptr.astype(np.int64), np.diff(W.indptr).astype(np.int64)
    if len(xkey) == 0:
        return items, contrib, support
    for s in range(0, B, chunk):
        sub, r = ids[s:s + chunk], rows[s:s + chunk]
        valid = ((np.arange(k)[None, :] < counts[s:s + chunk, None]) & (sub >= 0) & (sub < I) & (r[:, None] >= 0) & (r[:, None] < U))
        pb, pp = np.nonzero(valid)
        item = sub[pb, pp].astype(np.int64)
        n = wlen[item]
        pair = np.repeat(np.arange(len(item)), n)
        off = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(wptr[item], n)
        j = W.indices[off].astype(np.int64)
        key = r[pb][pair] * I + j
        pos = np.minimum(np.searchsorted(xkey, key), len(xkey) - 1)
        hit = xkey[pos] == key
        with np.errstate(all="ignore"):
            pair, j, c = pair[hit], j[hit], xval[pos[hit]] * W.data[off[hit]].astype(np.float32)
        sup = np.bincount(pair, minlength=len(item))                    # NaN contributions included
        number = ~np.isnan(c)
        pair, j, c = pair[number], j[number], c[number]
        numbers = np.bincount(pair, minlength=len(item))
        order = np.lexsort((j, -c, pair))
        pair, j, c = pair[order], j[order], c[order]
        rank = np.arange(len(pair)) - (np.cumsum(numbers) - numbers)[pair]
        keep = rank < top_m
        items[s + pb[pair[keep]], pp[pair[keep]], rank[keep]] = j[keep]
        contrib[s + pb[pair[keep]], pp[pair[keep]], rank[keep]] = c[keep]
        support[s + pb, pp] = sup
    return items, contrib, support


def ordered_sum(c):
    """Left to right in float32 from 0.0f: scipy's csr_matmat order for one output entry."""
    acc = np.float32(0.0)
    for v in np.asarray(c, dtype=np.float32):
        acc = np.float32(acc + v)
    return acc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def load(z, prefix, fmt=sp.csc_matrix):
    return fmt((z[f"{prefix}_data"], z[f"{prefix}_indices"], z[f"{prefix}_indptr"]), shape=tuple(z[f"{prefix}_shape"]))


def golden():
    z, zs = np.load(os.path.join(G, "models.npz")), np.load(os.path.join(G, "scoring.npz"))
    X = load(z, "X2").tocsr()
    X.sort_indices()
    W = load(z, "W2_k50")
    W.sort_indices()
    return X, W, zs["users"], zs["ids_f32_sparse_filter"], zs["scores_f32_sparse_filter"]


class ExplainOracleBackend(OracleBackend):
    """The CPU stand-in plus explain_topk from the host model (TEST-ONLY, like its base)."""

    def explain_topk(self, row_ids, xb, n_items, W, ids, counts, list_k, top_m, items, contrib, support):
        import torch
        ptr, col, val = (t.numpy() for t in xb)
        X = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, n_items))
        Wc = sp.csc_matrix((W["cval"].numpy(), W["crow"].numpy(), W["cptr"].numpy()), shape=(n_items, n_items))
        rows = row_ids.numpy() if row_ids is not None else np.arange(ids.shape[0])
        r, c, s = host_model(X, Wc, rows, ids.numpy()[:, :list_k], counts.numpy(), top_m)
        items.copy_(torch.from_numpy(r)); contrib.copy_(torch.from_numpy(c)); support.copy_(torch.from_numpy(s))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=ExplainOracleBackend())
    return m


# ---------------------------------------------------------------------------------------------- the definition
def test_ordered_sum_of_the_contributions_is_the_reference_score_bit_for_bit():
    """All 240 x 10 pairs of the fixture generated from the real reference: no pair left out."""
    X, W, users, ids, scores = golden()
    assert ids.shape == (240, 10) and (ids >= 0).all()
    sizes = []
    for b, u in enumerate(users.tolist()):
        for p in range(10):
            j, c = pair_contributions(X, W, u, int(ids[b, p]))
            assert c.dtype == np.float32 and np.all(j[1:] > j[:-1])
            assert bits(ordered_sum(c)) == bits(np.float32(scores[b, p])), (u, p)
            sizes.append(len(j))
    assert len(sizes) == 2400 and min(sizes) == 1 and max(sizes) == 30 and int(np.median(sizes)) == 6


@pytest.mark.parametrize("top_m", [1, 3, 32])
def test_vectorised_model_is_the_definition(top_m):
    X, W, users, ids, _ = golden()
    rng = np.random.default_rng(5)
    ids = ids.astype(np.int32).copy()
    ids[rng.random(ids.shape) < 0.05] = -1                               # holes inside lists
    ids[3, 4], ids[7, 0] = W.shape[1], W.shape[1] + 7                    # ids beyond the catalogue
    counts = rng.integers(0, 11, len(users)).astype(np.int32)
    rows = users.copy()
    rows[5], rows[9] = -1, X.shape[0]                                    # users without a row
    a, b = host_model(X, W, rows, ids, counts, top_m), host_model_vectorised(X, W, rows, ids, counts, top_m, chunk=37)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    assert (a[2][5] == 0).all() and (a[2][9] == 0).all() and a[2].max() > 3
    live = np.arange(10)[None, :] < counts[:, None]
    assert (a[2][~live] == 0).all() and (a[0][~live] == -1).all() and np.isneginf(a[1][~live]).all()


def test_tie_rule_lower_item_id_first_and_negative_contributions_take_part():
    X = sp.csr_matrix(np.array([[2, 1, 2, 4, 0, 1]], dtype=np.float32))
    W = sp.csc_matrix(np.array([[0.5], [1.0], [0.5], [-1.0], [9.0], [1.0]], dtype=np.float32))
    for model in (host_model, host_model_vectorised):
        items, contrib, support = model(X, W, [0], np.array([[0]], np.int32), [1], 6)
        assert support.tolist() == [[5]]
        assert items[0, 0].tolist() == [0, 1, 2, 5, 3, -1]                  # 1.0 four times (ids ascending), then -4.0
        assert contrib[0, 0].tolist() == [1.0, 1.0, 1.0, 1.0, -4.0, -np.inf]


# ---------------------------------------------------------------------------------------------- the value edges: the cases
PNAN, NNAN = (np.float32(v) for v in np.array([0x7fc00000, 0xffc00000], np.uint32).view(np.float32))     # the two default quiet NaNs
INF = np.float32(np.inf)


def p2(e):
    return np.float32(2.0 ** e)


# name -> the (x_uj, w_ji) of the contributing items in ascending item id.  Every zero below is a STORED zero.
VALUE_SETS = {
    "nan_lowest": [(PNAN, 1), (1, 2), (1, 1), (1, .5), (1, 3), (1, -2)],
    "nan_middle": [(1, 2), (1, 1), (1, NNAN), (1, .5), (1, 3), (1, -2)],
    "nan_highest": [(1, 2), (1, 1), (1, .5), (1, 3), (1, -2), (NNAN, 1)],
    "two_nans": [(PNAN, 1), (1, 2), (1, 1), (1, 0), (PNAN, 1), (1, 3), (1, -2)],       # c = nan 2 1 0 nan 3 -2: the butterfly's smallest failure
    "two_nans_adjacent": [(1, 3), (PNAN, 1), (1, NNAN), (1, 1), (1, 5)],
    "all_nan": [(PNAN, 1), (1, NNAN), (INF, 0)],
    "made_and_given_nans": [(INF, 0), (1, 2), (PNAN, 1), (1, -1), (NNAN, 1), (-INF, 0), (1, 5), (0, INF), (1, PNAN), (0, -INF), (-4, 1)],
    "infinities": [(1, 1), (INF, 1), (INF, -1), (1, 2), (1, INF), (1, -3), (-INF, 2), (1, 0)],   # c = 1 inf -inf 2 inf -3 -inf 0
    "signed_zeros_minus_first": [(-1, 0), (1, 0), (1, 1)],                             # c = -0 +0 1
    "signed_zeros_plus_first": [(1, 0), (-1, 0), (1, -1)],                             # c = +0 -0 -1
    "denormals": [(p2(-100), p2(-60)), (p2(-100), p2(-40)), (1, 0), (-p2(-100), p2(-40)), (-p2(-100), p2(-60)), (1, -1)],
    "overflow_ties_inf": [(p2(100), p2(100)), (INF, 1), (1, 3), (INF, 2), (p2(100), p2(100))],   # c = inf inf 3 inf inf
}
# what the definition says about them, item ids as positions in the value set (top_m = 32: the whole list)
EXPECTED_ORDER = {
    "nan_lowest": [4, 1, 2, 3, 5], "nan_middle": [4, 0, 1, 3, 5], "nan_highest": [3, 0, 1, 2, 4], "two_nans": [5, 1, 2, 3, 6],
    "two_nans_adjacent": [4, 0, 3], "all_nan": [], "made_and_given_nans": [6, 1, 3, 10], "infinities": [1, 4, 3, 0, 7, 5, 2, 6],
    "signed_zeros_minus_first": [2, 0, 1], "signed_zeros_plus_first": [0, 1, 2], "denormals": [1, 0, 2, 4, 3, 5],
    "overflow_ties_inf": [0, 1, 3, 4, 2],
}
EDGE_ITEMS = 400
ISSUE_J = [0, 1, 2, 9, 11, 17, 21]                                      # the "two_nans" values on these literal ids: a 7-lane column


def _spread(m, residue):
    """m distinct item ids = residue (mod 3) spread evenly over [0, EDGE_ITEMS)."""
    return (3 * np.round(np.linspace(0, 132, m)).astype(np.int64) + residue) if m else np.empty(0, np.int64)


def _sorted_entries(j_a, v_a, j_b, v_b):
    j, v = np.concatenate([j_a, j_b]), np.concatenate([np.asarray(v_a, np.float32), np.asarray(v_b, np.float32)])
    order = np.argsort(j, kind="stable")
    assert len(np.unique(j)) == len(j)
    return j[order], v[order]


def edge_case():
    """(X csr, W csc, rows, ids[n, 4], counts, cases): one matrix pair from raw (data, indices, indptr) arrays -- stored zeros
    survive -- that runs every value set through the kernel's four search paths.  Per value set of n contributing items
    (ids = 0 mod 3, the first 0 and the last 396) there is a row of X of 64 and one of 65 entries (search in registers /
    in memory; the other entries have ids = 1 mod 3) and a column of W of 64, 65 and 130 entries (one probe / a probe per
    round; the other entries have ids = 2 mod 3, so they never meet the row's): the contributing items are exactly the
    value set's, in the first and the last lane of a probe and, for the 130-entry column, in all three probes.  The sets of
    three values also get a row and a column of 3 entries.  Row r explains its set's columns: ids[r], counts[r].
    cases[(name, row_len, col_len)] = (r, slot, the contributing ids)."""
    x_rows, w_cols, lists, cases = [], [], [], {}
    for name, pairs in VALUE_SETS.items():
        n = len(pairs)
        J = _spread(n, 0)
        col_lens = ([3] if n == 3 else []) + [64, 65, 130]
        cols = []
        for L in col_lens:
            j, v = _sorted_entries(J, [w for _, w in pairs], _spread(L - n, 2), np.full(L - n, 0.75))
            if L == 130:
                at = np.flatnonzero(np.isin(j, J))
                assert at[0] == 0 and ((at >= 64) & (at < 128)).any() and (at >= 128).any(), (name, at)
            cols.append(len(w_cols))
            w_cols.append((j, v))
        for L in ([3] if n == 3 else []) + [64, 65]:
            for slot, Lc in enumerate(col_lens):
                cases[(name, L, Lc)] = (len(x_rows), slot, J)
            x_rows.append(_sorted_entries(J, [x for x, _ in pairs], _spread(L - n, 1), np.full(L - n, 1.5)))
            lists.append(cols)
    J = np.array(ISSUE_J, np.int64)
    cases[("two_nans_literal", 7, 7)] = (len(x_rows), 0, J)
    x_rows.append((J, np.array([x for x, _ in VALUE_SETS["two_nans"]], np.float32)))
    lists.append([len(w_cols)])
    w_cols.append((J, np.array([w for _, w in VALUE_SETS["two_nans"]], np.float32)))

    def raw(entries, n_major):
        ptr = np.zeros(n_major + 1, np.int64)
        ptr[1:len(entries) + 1] = np.cumsum([len(j) for j, _ in entries])
        ptr[len(entries) + 1:] = ptr[len(entries)]
        return np.concatenate([v for _, v in entries]), np.concatenate([j for j, _ in entries]).astype(np.int32), ptr.astype(np.int32)

    X = sp.csr_matrix(raw(x_rows, len(x_rows)), shape=(len(x_rows), EDGE_ITEMS))
    W = sp.csc_matrix(raw(w_cols, EDGE_ITEMS), shape=(EDGE_ITEMS, EDGE_ITEMS))
    assert len(w_cols) <= EDGE_ITEMS and X.has_sorted_indices and W.has_sorted_indices
    assert X.nnz == sum(len(j) for j, _ in x_rows) and W.nnz == sum(len(j) for j, _ in w_cols)          # no zero was dropped
    ids = np.full((len(x_rows), 4), -1, np.int32)
    for r, cols in enumerate(lists):
        ids[r, :len(cols)] = cols
    return X, W, np.arange(len(x_rows)), ids, np.array([len(c) for c in lists], np.int32), cases


EDGE_TOP_M = (1, 4, 32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def test_edge_cases_definition_vectorised_model_and_the_expected_lists():
    X, W, rows, ids, counts, cases = edge_case()
    assert X.shape[0] < 40 and len(cases) > 60 and sorted({k[1] for k in cases}) == [3, 7, 64, 65] and sorted({k[2] for k in cases}) == [3, 7, 64, 65, 130]
    assert np.isnan(X.data).any() and np.isnan(W.data).any() and np.isinf(X.data).any() and (W.data == 0).any() and (X.data == 0).any()
    for top_m in EDGE_TOP_M:
        a, b = host_model(X, W, rows, ids, counts, top_m), host_model_vectorised(X, W, rows, ids, counts, top_m, chunk=5)
        assert same(a, b)
        assert not np.isnan(a[1]).any()                                  # under the rule no output holds a NaN
        assert np.isneginf(a[1][a[0] < 0]).all() and (np.sort(a[0] < 0, axis=2) == (a[0] < 0)).all()      # padding is -inf and trails
    items, contrib, support = a                                          # top_m = 32
    for (name, Lr, Lc), (r, slot, J) in cases.items():
        pairs = VALUE_SETS[name.replace("_literal", "")]
        want = EXPECTED_ORDER[name.replace("_literal", "")]
        assert support[r, slot] == len(pairs), (name, Lr, Lc)
        assert items[r, slot, :len(want)].tolist() == J[want].tolist() and (items[r, slot, len(want):] == -1).all(), (name, Lr, Lc)
        with np.errstate(all="ignore"):
            c = np.array([np.float32(x) * np.float32(w) for x, w in pairs], np.float32)
        assert np.array_equal(bits(contrib[r, slot, :len(want)]), bits(c[want])) and np.isneginf(contrib[r, slot, len(want):]).all()
    r, slot, _ = cases[("signed_zeros_minus_first", 3, 3)]
    assert bits(contrib[r, slot, :3]).tolist() == [0x3f800000, 0x80000000, 0x00000000]           # each zero keeps its sign bit
    r, slot, _ = cases[("denormals", 64, 130)]
    assert bits(contrib[r, slot, :6]).tolist() == [0x00000200, 0, 0, 0x80000000, 0x80000200, 0xbf800000]   # 2^-140 is kept, 2^-160 is 0
    r, slot, _ = cases[("infinities", 65, 65)]
    assert contrib[r, slot, :8].tolist() == [np.inf, np.inf, 2, 1, 0, -3, -np.inf, -np.inf] and (items[r, slot, 6:8] >= 0).all()


def test_existing_fixtures_hold_no_nan_and_keep_their_answers_under_the_rule():
    X, W, users, ids, _ = golden()
    z = np.load(os.path.join(G, "partial_fit.npz"))
    assert np.isfinite(X.data).all() and np.isfinite(W.data).all() and np.isfinite(z["v"]).all()
    old = mutant_model(X, W, users, ids, np.full(len(users), 10), 32, "nan_listed_last")      # the definition before the rule
    assert same(old, host_model(X, W, users, ids, np.full(len(users), 10), 32))


# ---------------------------------------------------------------------------------------------- mutated models: the cases bite
def _better(a, b):
    """cand_better of csrc/common.hip.h on (score, aux, id) triples: a NaN score is neither above nor below."""
    if a[2] < 0:
        return False
    if b[2] < 0:
        return True
    if a[0] > b[0]:
        return True
    if a[0] < b[0]:
        return False
    if a[1] != b[1]:
        return a[1] > b[1]
    return a[2] > b[2]


def butterfly_pair(col_j, col_c, top_m):
    """The kernel BEFORE the rule re-enacted lane by lane on one pair: col_j / col_c are the column's entries in storage order
    (j = -1: not in the row), a NaN product is a candidate like any other.  64 lanes, the xor butterfly of wave_best, each
    lane keeping its own view of the last winner; lane m's view of round m is what is written."""
    none = (-np.inf, 0, -1)
    cands = [(float(c), 0xffffffff - int(j), int(j)) if j >= 0 else none for j, c in zip(col_j, col_c)]
    support = sum(j >= 0 for j in col_j)
    one = len(cands) <= 64
    last, live = [none] * 64, [True] * 64
    out_j, out_c = [-1] * top_m, [np.float32(-np.inf)] * top_m
    for m in range(min(top_m, support)):
        b = [none] * 64
        for lane in range(64):
            if not live[lane]:
                continue
            for base in range(0, len(cands), 64):
                x = cands[base + lane] if base + lane < len(cands) else none
                if last[lane][2] >= 0 and not _better(last[lane], x):
                    continue
                if one:
                    b[lane] = x
                elif _better(x, b[lane]):
                    b[lane] = x
        for step in (32, 16, 8, 4, 2, 1):
            b = [b[l ^ step] if _better(b[l ^ step], b[l]) else b[l] for l in range(64)]
        for lane in range(64):
            if live[lane] and b[lane][2] < 0:
                live[lane] = False
            elif live[lane]:
                last[lane] = b[lane]
        if live[m]:
            out_j[m], out_c[m] = b[m][2], np.float32(b[m][0])
    return out_j, out_c, support


DEFECTS = ("nan_listed_last", "nan_by_sign_bit", "nan_equal_to_everything", "denormals_flushed", "minus_zero_written_as_plus_zero",
           "ties_to_the_higher_id", "nan_dropped_from_support")


def mutant_model(X, W, rows, ids, counts, top_m, defect):
    """host_model with one defect built in."""
    assert defect in DEFECTS
    ids = np.asarray(ids)
    B, k = ids.shape
    items = np.full((B, k, top_m), -1, np.int32)
    contrib = np.full((B, k, top_m), -np.inf, np.float32)
    support = np.zeros((B, k), np.int32)
    for b in range(B):
        for p in range(min(max(int(counts[b]), 0), k)):
            j, c = pair_contributions(X, W, int(rows[b]), int(ids[b, p]))
            support[b, p] = len(j)
            if defect == "nan_equal_to_everything":
                item = int(ids[b, p])
                if not 0 <= item < W.shape[1]:
                    continue
                col = W.indices[W.indptr[item]:W.indptr[item + 1]].astype(np.int64)
                full = np.full(len(col), np.float32(0))
                full[np.isin(col, j)] = c
                r, v, _ = butterfly_pair(np.where(np.isin(col, j), col, -1), full, top_m)
                items[b, p], contrib[b, p] = r, v
                continue
            if defect == "denormals_flushed":
                c = np.where(np.abs(c) < p2(-126), np.copysign(np.float32(0), c), c).astype(np.float32)
            if defect == "nan_dropped_from_support":
                support[b, p] = int((~np.isnan(c)).sum())
            if defect == "nan_by_sign_bit":                             # the order-preserving key of the raw bits
                u = bits(c).astype(np.int64)
                key = np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000)
                order = np.lexsort((j, -key))[:top_m]
            else:
                if defect != "nan_listed_last":
                    j, c = j[~np.isnan(c)], c[~np.isnan(c)]
                order = np.lexsort((-j if defect == "ties_to_the_higher_id" else j, -c))[:top_m]
            items[b, p, :len(order)], contrib[b, p, :len(order)] = j[order], c[order]
            if defect == "minus_zero_written_as_plus_zero":
                contrib[b, p][contrib[b, p] == 0] = 0.0
    return items, contrib, support


# defect -> a case that must tell it from the definition (every defect is also run over all cases: which ones see it is printed)
CAUGHT_BY = {
    "nan_listed_last": ("nan_lowest", 64, 64), "nan_by_sign_bit": ("made_and_given_nans", 65, 130),
    "nan_equal_to_everything": ("two_nans_literal", 7, 7), "denormals_flushed": ("denormals", 64, 65),
    "minus_zero_written_as_plus_zero": ("signed_zeros_minus_first", 3, 3), "ties_to_the_higher_id": ("infinities", 65, 64),
    "nan_dropped_from_support": ("all_nan", 3, 130),
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_defect_is_told_from_the_definition_by_a_named_case(defect):
    X, W, rows, ids, counts, cases = edge_case()
    top_m = 32
    if defect == "nan_equal_to_everything":                              # the lane-by-lane re-enactment: one-probe columns only
        keep = sorted({r for (_, _, Lc), (r, _, _) in cases.items() if Lc <= 7} | {cases[k][0] for k in cases if k[2] == 64})
        rows, ids, counts = rows[keep], ids[keep].copy(), counts[keep]
        ids[W.indptr[np.maximum(ids, 0) + 1] - W.indptr[np.maximum(ids, 0)] > 64] = -1
        cases = {k: (keep.index(r), slot, J) for k, (r, slot, J) in cases.items() if r in keep and ids[keep.index(r), slot] >= 0}
    want, got = host_model(X, W, rows, ids, counts, top_m), mutant_model(X, W, rows, ids, counts, top_m, defect)
    seen = sorted(k for k, (r, slot, _) in cases.items()
                  if not (np.array_equal(want[0][r, slot], got[0][r, slot]) and np.array_equal(bits(want[1][r, slot]), bits(got[1][r, slot]))
                          and want[2][r, slot] == got[2][r, slot]))
    print(f"{defect}: seen by {len(seen)} of {len(cases)} cases, value sets {sorted({k[0] for k in seen})}")
    assert CAUGHT_BY[defect] in seen
    if defect == "nan_equal_to_everything":                              # the failure the rule was written for: item 17 twice, 21 lost
        r, slot, _ = cases[("two_nans_literal", 7, 7)]
        assert got[0][r, slot, :7].tolist() == [0, 17, 1, 2, 9, 11, 17] and want[0][r, slot, :7].tolist() == [17, 1, 2, 9, 21, -1, -1]


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _int_model():
    z = np.load(os.path.join(G, "partial_fit.npz"))
    a, b = z["A"][0], z["C"][1]
    batch = [(int(x), int(y), float(t), float(r)) for x, y, t, r in zip(z["u"][a:b], z["i"][a:b], z["ts"][a:b], z["v"][a:b])]
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    return m, batch


def _check_against_definition(m, users, got, items_given=None, top_m=3):
    """`got` (the list form) against the host model on the model's own X and W, raw ids mapped by hand."""
    X, W = m.interactions.to_csr(), m.model.item_similarity.tocsc()
    X.sort_indices(); W.sort_indices()
    assert len(got) == len(users)
    n_reasons = 0
    for u, row in zip(users, got):
        uid = m._known_user_id(u)
        for item, reasons in row:
            try:
                iid = m.item_ids.get_id(item)
            except ValueError:
                iid = None
            j, c = pair_contributions(X, W, -1 if uid is None else uid, -1 if iid is None else iid)
            order = np.lexsort((j, -c))[:top_m]
            assert [r for r, _ in reasons] == [m.item_ids.get(int(x)) for x in j[order]], (u, item)
            assert all(isinstance(v, float) for _, v in reasons)
            assert np.array_equal(bits([v for _, v in reasons]), bits(c[order])), (u, item)
            n_reasons += len(reasons)
    return n_reasons


def test_slim_explain_batch_sparse_mode_integer_ids():
    from rtrec_amd.recommender import Recommender
    m, batch = _int_model()
    users = sorted({u for u, _, _, _ in batch})[:40]
    cold = max(u for u, _, _, _ in batch) + 1000
    recs = m.recommend_batch(users + [cold], top_k=5)
    got = m.explain_batch(users + [cold], top_k=5, top_m=3)
    assert [[item for item, _ in row] for row in got] == recs            # the lists are recommend_batch's
    assert _check_against_definition(m, users, got[:-1]) > 50
    assert recs[-1] and all(reasons == [] for _, reasons in got[-1])     # the cold-start list, no reasons
    # given lists: the ones served above reproduce the one-pass answer; an unknown item has no explanation
    assert m.explain_batch(users + [cold], items=recs, top_m=3) == got
    odd = [[recs[0][0], 10 ** 7, "no such item"], [], recs[2][:1]]
    got2 = m.explain_batch(users[:3], items=odd, top_m=2)
    assert [[item for item, _ in row] for row in got2] == odd
    assert got2[0][0][1] == got[0][0][1][:2] and got2[0][1][1] == [] and got2[0][2][1] == [] and got2[1] == []
    assert m.explain(users[0], top_k=5) == got[0] and m.explain(users[0], items=recs[0]) == got[0]
    # as_arrays is the list form
    ids, counts, r_ids, contrib, support = m.explain_batch(users + [cold], top_k=5, top_m=3, as_arrays=True)
    assert ids.shape == (41, 5) and r_ids.shape == contrib.shape == (41, 5, 3) and support.shape == (41, 5)
    for b, row in enumerate(got):
        assert ids[b, :counts[b]].tolist() == [item for item, _ in row] and (ids[b, counts[b]:] == -1).all()
        for p, (_, reasons) in enumerate(row):
            n = min(int(support[b, p]), 3)
            assert list(zip(r_ids[b, p, :n].tolist(), contrib[b, p, :n].tolist())) == reasons
            assert (r_ids[b, p, n:] == -1).all() and np.isneginf(contrib[b, p, n:]).all()
    assert (support[-1] == 0).all() and support.max() >= 3
    # filter_interacted is the list's, and the facade passes everything through
    rec = Recommender(m)
    nof = rec.explain_batch(users, top_k=5, top_m=3, filter_interacted=False)
    assert [[item for item, _ in row] for row in nof] == m.recommend_batch(users, top_k=5, filter_interacted=False) and nof != got[:-1]
    assert rec.explain_batch(users + [cold], top_k=5, top_m=3) == got and rec.explain(users[1], top_k=5) == got[1]
    assert rec.explain_batch(users, items=recs[:-1], top_m=1) == [[(i, r[:1]) for i, r in row] for row in got[:-1]]
    # empty batch, users beyond the matrix, parameter ranges
    assert m.explain_batch([], top_k=5) == [] and m.explain_batch([], items=[]) == []
    e = m.explain_batch([], top_k=5, top_m=2, as_arrays=True)
    assert e[0].shape == (0, 5) and e[2].shape == (0, 5, 2) and e[4].shape == (0, 5)
    neg = m.explain_batch([users[0], -1], top_k=5)                       # _recommend_odd_ids' rule: nothing to wrap around to
    assert neg[0] == got[0] and neg[1] == []
    for kw in (dict(top_k=0), dict(top_k=65), dict(top_m=0), dict(top_m=33)):
        with pytest.raises(ValueError, match="1..64 items and top_m in 1..32"):
            m.explain_batch(users[:2], **kw)
    with pytest.raises(ValueError, match="one list per user"):
        m.explain_batch(users[:2], items=[[1]])


def test_explain_batch_list_form_counts_the_reasons_present_when_a_contribution_is_nan():
    m, batch = _int_model()
    users = sorted({u for u, _, _, _ in batch})[:40]
    recs = m.recommend_batch(users, top_k=5)
    ids, counts, r_ids, contrib, support = m.explain_batch(users, items=recs, top_m=3, as_arrays=True)
    b, p = next((b, p) for b in range(len(users)) for p in range(counts[b]) if 2 <= support[b, p] <= 3)
    before = m.explain_batch([users[b]], items=[[recs[b][p]]], top_m=3)[0][0][1]
    assert len(before) == support[b, p]
    W = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    W[int(r_ids[b, p, 0]), int(ids[b, p])] = np.nan                      # the strongest reason's weight: its contribution is NaN
    assert W.nnz == m.model.item_similarity.nnz
    m.model.item_similarity = W
    after = m.explain_batch([users[b]], items=[[recs[b][p]]], top_m=3)
    assert after == [[(recs[b][p], before[1:])]]                         # one reason fewer, no padding slot read as a reason
    a = m.explain_batch([users[b]], items=[[recs[b][p]]], top_m=3, as_arrays=True)
    assert a[4][0, 0] == support[b, p] and (a[2][0, 0] >= 0).sum() == support[b, p] - 1 and not np.isnan(a[3]).any()


def test_slim_explain_batch_dense_mode_string_ids():
    z = np.load(os.path.join(G, "partial_fit.npz"))
    a, b = z["A"][0], z["C"][1]
    batch = [(f"u{x}", f"i{y}", float(t), float(r)) for x, y, t, r in zip(z["u"][a:b], z["i"][a:b], z["ts"][a:b], z["v"][a:b])]
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    users = sorted({u for u, _, _, _ in batch})[:30] + ["nobody"]
    recs = m.recommend_batch(users, top_k=6)
    got = m.explain_batch(users, top_k=6, top_m=4)
    assert [[item for item, _ in row] for row in got] == recs and all(isinstance(i, str) for row in recs for i in row)
    assert _check_against_definition(m, users[:-1], got[:-1], top_m=4) > 50
    assert all(isinstance(r, str) for row in got for _, reasons in row for r, _ in reasons)
    assert all(reasons == [] for _, reasons in got[-1])
    assert m.explain_batch(users, items=recs, top_m=4) == got
    assert m.explain_batch(users[:1], items=[[recs[0][0], "never seen", 3]], top_m=4)[0][1:] == [("never seen", []), (3, [])]
    ids, counts, r_ids, contrib, support = m.explain_batch(users, top_k=6, top_m=4, as_arrays=True)
    get = m.item_ids.get                                                 # DENSE models: the arrays hold internal ids
    for b, row in enumerate(got):
        assert [get(int(i)) for i in ids[b, :counts[b]]] == [item for item, _ in row]
        for p, (_, reasons) in enumerate(row):
            n = min(int(support[b, p]), 4)
            assert [(get(int(i)), float(c)) for i, c in zip(r_ids[b, p, :n], contrib[b, p, :n])] == reasons


def test_not_fitted_lossy_and_sharded_weights_are_refused():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    fresh = cpu_slim()
    with pytest.raises(RuntimeError, match="Model must be fitted before calling explain_batch"):
        fresh.explain_batch([1])
    with pytest.raises(RuntimeError, match="Model must be fitted before calling explain_batch"):
        fresh.model.explain_batch([0], sp.csr_matrix((1, 3), dtype=np.float32), [[1]])
    m, batch = _int_model()
    users = sorted({u for u, _, _, _ in batch})[:4]
    W = m.model.item_similarity
    recs = m.recommend_batch(users, top_k=5)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)         # float64 W holding float32 numbers: same answer
    got64 = m.explain_batch(users, items=recs)
    m.model.item_similarity = W
    assert got64 == m.explain_batch(users, items=recs) and any(reasons for row in got64 for _, reasons in row)
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.explain_batch(users, top_k=5)
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.explain_batch(users, items=[[1]] * 4)
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=ExplainOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
        eng.explain_rows([0], np.array([[1]], np.int32), top_m=1)
    # the host-CSR boundary of SLIMElastic
    X = m.interactions.to_csr()
    se = SLIMElastic({"nn_feature_selection": 5}, engine=SlimEngine(backend=ExplainOracleBackend()))
    se.item_similarity = W
    lists = [[3, 1, 10 ** 6], [], [2]]
    r, c, s = se.explain_batch([users[0], users[1], users[2]], X, lists, top_m=2)
    ids = np.array([[3, 1, -1], [-1, -1, -1], [2, -1, -1]], np.int32)
    want = host_model(X, W.tocsc(), [users[0], users[1], users[2]], ids, [3, 0, 1], 2)
    assert np.array_equal(r, want[0]) and np.array_equal(bits(c), bits(want[1])) and np.array_equal(s, want[2])
    with pytest.raises(ValueError, match="1..64"):
        se.explain_batch([users[0]], X, [[1]], top_m=40)


# ---------------------------------------------------------------------------------------------- serving
def test_explain_route_token_payload_and_failure():
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    from fastapi import FastAPI
    m, batch = _int_model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = batch[0][0]
    r = client.post("/explain", json={"user": user, "top_k": 4, "top_m": 2}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/explain", json={"user": user, "top_k": 4, "top_m": 2}, headers=ok)
    want = m.explain(user, top_k=4, top_m=2)
    assert r.status_code == 200 and want and any(reasons for _, reasons in want)
    assert r.json() == {"user": user, "explanations": [{"item": i, "reasons": [{"item": j, "contribution": c} for j, c in rs]}
                                                       for i, rs in want]}
    served = [i for i, _ in want]
    r = client.post("/explain", json={"user": user, "items": served + [10 ** 7], "top_m": 2, "filter_interacted": False}, headers=ok)
    assert r.status_code == 200
    assert r.json()["explanations"][:-1] == client.post("/explain", json={"user": user, "top_k": 4, "top_m": 2}, headers=ok).json()["explanations"]
    assert r.json()["explanations"][-1] == {"item": 10 ** 7, "reasons": []}
    r = client.post("/explain", json={"user": user, "top_m": 99}, headers=ok)      # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Explanation failed"}
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)     # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == [i for i, _ in m.explain(user, top_k=4)]


# ---------------------------------------------------------------------------------------------- registration
def test_explain_topk_is_registered_declared_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    assert "explain_topk" in ops.OPS and ops.EXPORT_OF["explain_topk"] == "rtrec_slim_explain_topk"
    schema = str(torch.ops.rtrec_amd.explain_topk.default._schema)
    for name in ("items", "contrib", "support"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("xb_ptr", "xb_col", "xb_val", "wc_ptr", "wc_row", "wc_val", "ids", "counts"):
        assert f"Tensor {name}" in schema, schema
    assert "Tensor? row_ids" in schema and "int list_k" in schema and "int top_m" in schema
    header = open(os.path.join(ROOT, "include", "rtrec_amd.h")).read()
    assert re.search(r"\bint rtrec_slim_explain_topk\s*\(", header)
    assert "rtrec_slim_explain_topk" in _native.EXPORTS and "explain.hip" in build.SOURCES
    L = _native.load()
    # the host-side argument checks run before anything touches a device
    fn = L.rtrec_slim_explain_topk
    one = 1                                                             # any non-NULL address: never dereferenced on these paths
    args = lambda n_rows=1, list_k=10, top_m=3, ids=one, stride=10, n_items=5, nnz=0: (
        n_rows, None, one, one, one, 4, nnz, n_items, one, one, one, 0, ids, stride, list_k, one, top_m, one, one, one, None)
    for kw in (dict(list_k=0), dict(list_k=65, stride=65), dict(top_m=0), dict(top_m=33)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_rows=-1), dict(n_items=-1), dict(nnz=-1), dict(stride=9), dict(ids=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, ids=None)) == 0
    assert callable(getattr(HipBackend, "explain_topk")) and callable(getattr(SlimEngine, "explain_device"))
    if not torch.cuda.is_available():
        with pytest.raises((NotImplementedError, RuntimeError)):
            i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
            torch.ops.rtrec_amd.explain_topk(None, i32(2), i32(1), torch.zeros(1), 3, i32(4), i32(1), torch.zeros(1), i32(1, 2), i32(1), 2, 1,
                                             i32(1, 2, 1), torch.zeros(1, 2, 1), i32(1, 2))
