"""The hybrid's similar_items (SLIM.similar_items_factor_batch / similar_items_hybrid_batch; csrc/factor_norms.hip,
factor_similar.hip, similar_blend.hip) without a GPU: each of the three definitions as a plain-Python host model, one step at a
time, and as a vectorised one that reuses the exact fused step of tests/test_factor_host.py; what the roundings the contract
fixes are worth (pinning tests); the blend against what the reference's own HybridSlimFM._similar_items answered
(tests/golden/similar_blend.json, written by tools/gen_golden_similar.py); the contract's edges; the rules of the extension
surface and the ValueError paths of the API that need no device.  The kernels are in
tests/test_gpu_similar.py.

The definitions (include/rtrec_amd_ext.h, "FACTOR NORMS", "FACTOR SIMILAR TOP-K", "SIMILAR BLEND"):
  norm   n2 = +0, then n2 = fmaf(v[c], v[c], n2) for ascending c; sqrt(n2) correctly rounded to float32
  s1     dot = the fmaf chain of rtrec_factor_topk; s1 = fl(dot / norm_i), one correctly rounded division; item i competes when
         i != q, the mask admits it and s1 is not NaN; the larger s1 first, the lower id among == ones
  blend  each list cut on its raw scores, the query taken out, A divided by the query norm, each list min-max normalised in
         float32, the union by first appearance, a float64 sum per id over EVERY occurrence (A's first), a stable descending sort"""
import base64
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from tests.test_factor_host import F32, bits, fma32, fmaf, host_scores, rounding_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "similar_blend.json")
FLT_MAX = float(np.finfo(np.float32).max)


def f32div(a, b):
    """One correctly rounded float32 division, through float64: the quotient of two float32 numbers rounded to 53 bits and then to
    24 is the correctly rounded float32 quotient (53 >= 2 * 24 + 2), and float64 has the range for every float32 quotient."""
    a, b = float(a), float(b)
    if b == 0.0:
        if a != a or a == 0.0:
            return F32(np.nan)
        return F32(math.copysign(math.inf, a) * math.copysign(1.0, b))
    return F32(a / b)


def dbits(a):
    """The bit patterns of float64 values after adding +0.0 (the sign of a zero is not part of the contract)."""
    return (np.asarray(a, np.float64) + 0.0).view(np.int64)


# ---------------------------------------------------------------------------------------------- norms
def host_norms_plain(V):
    """THE DEFINITION, one fmaf at a time: V [n, dim] -> norms [n] float32."""
    V = np.asarray(V, F32)
    out = np.zeros(len(V), F32)
    for r in range(len(V)):
        n2 = F32(0.0)
        for c in range(V.shape[1]):
            n2 = fmaf(V[r, c], V[r, c], n2)
        out[r] = F32(math.sqrt(float(n2))) if n2 == n2 and n2 >= 0 else F32(np.nan)
    return out


def host_norms_fast(V):
    """host_norms_plain, vectorised: the chain through fma32, the root in float64 rounded once more."""
    V = np.asarray(V, F32)
    n2 = np.zeros(len(V), F32)
    for c in range(V.shape[1]):
        n2 = fma32(V[:, c], V[:, c], n2)
    with np.errstate(all="ignore"):
        return np.sqrt(n2.astype(np.float64)).astype(F32)


# ---------------------------------------------------------------------------------------------- cosine top-k
def _query_vectors(Q, norms, queries, P, p_norms):
    """(vector per job or None, norm per job, excluded id per job)."""
    n_items = len(Q)
    R = len(P) if P is not None else len(queries)
    q = np.full(R, -1, np.int64) if queries is None else np.asarray(queries, np.int64)
    vec, qn = [], np.zeros(R, F32)
    for r in range(R):
        if P is not None:
            vec.append(np.asarray(P[r], F32)); qn[r] = p_norms[r]
        elif 0 <= q[r] < n_items:
            vec.append(Q[q[r]]); qn[r] = norms[q[r]]
        else:
            vec.append(None)
    return vec, qn, q


def _finish(cands, top_k, qn, write_cosine, ids, scores, count, r, divide):
    """cands: (id, s1) in the strict order; writes job r."""
    if write_cosine and not qn > 0:
        return
    n = min(top_k, len(cands))
    count[r] = n
    for t in range(n):
        ids[r, t] = cands[t][0]
        scores[r, t] = divide(cands[t][1], qn) if write_cosine else cands[t][1]


def host_similar_plain(Q, norms, queries, top_k, P=None, p_norms=None, mask=None, write_cosine=False):
    """THE DEFINITION, one step at a time: (ids[R, top_k] int32, scores[R, top_k] float32, count[R] int32, div[R] float32).
    Q [n_items, dim] the targets, norms [n_items] their divisors, `queries` the item per job (None with P: nothing excluded);
    P [R, dim] / p_norms [R]: brought query vectors."""
    Q, norms = np.asarray(Q, F32), np.asarray(norms, F32)
    vec, qn, q = _query_vectors(Q, norms, queries, P, p_norms)
    R = len(vec)
    ids = np.full((R, top_k), -1, np.int32)
    scores = np.full((R, top_k), -np.inf, F32)
    count = np.zeros(R, np.int32)
    for r in range(R):
        if vec[r] is None:
            continue
        cands = []
        for i in range(len(Q)):
            if i == q[r] or (mask is not None and not mask[i]):
                continue
            dot = F32(0.0)
            for c in range(Q.shape[1]):
                dot = fmaf(vec[r][c], Q[i, c], dot)
            s1 = f32div(dot, norms[i])
            if s1 == s1:
                cands.append((i, s1))
        cands.sort(key=lambda t: (-float(t[1]), t[0]))
        _finish(cands, top_k, qn[r], write_cosine, ids, scores, count, r, f32div)
    return ids, scores, count, qn


def host_s1(V, Q, norms):
    """The s1 block [len(V), len(Q)] by the vectorised chain and numpy's float32 division (IEEE: correctly rounded)."""
    with np.errstate(all="ignore"):
        return host_scores(V, Q) / np.asarray(norms, F32)[None, :]


def host_similar_fast(Q, norms, queries, top_k, P=None, p_norms=None, mask=None, write_cosine=False):
    """host_similar_plain, vectorised: host_scores of tests/test_factor_host.py, numpy's float32 division, a lexsort."""
    Q, norms = np.asarray(Q, F32), np.asarray(norms, F32)
    vec, qn, q = _query_vectors(Q, norms, queries, P, p_norms)
    R = len(vec)
    ids = np.full((R, top_k), -1, np.int32)
    scores = np.full((R, top_k), -np.inf, F32)
    count = np.zeros(R, np.int32)
    live = [r for r in range(R) if vec[r] is not None]
    if not live or not len(Q):
        return ids, scores, count, qn
    S = host_s1(np.stack([vec[r] for r in live]), Q, norms)
    ok = ~np.isnan(S)
    if mask is not None:
        ok &= (np.asarray(mask) != 0)[None, :]
    for a, r in enumerate(live):
        if 0 <= q[r] < len(Q):
            ok[a, q[r]] = False
        c = np.flatnonzero(ok[a])
        s = S[a, c] + F32(0.0)
        order = np.lexsort((c, -s.astype(np.float64)))[:top_k]
        with np.errstate(all="ignore"):
            _finish([(c[o], S[a, c[o]]) for o in order], top_k, qn[r], write_cosine, ids, scores, count, r, lambda x, y: F32(x) / F32(y))
    return ids, scores, count, qn


def assert_same_lists(got, want, what=""):
    g_ids, g_sc, g_cnt = [np.asarray(a) for a in got[:3]]
    w_ids, w_sc, w_cnt = [np.asarray(a) for a in want[:3]]
    assert np.array_equal(g_cnt, w_cnt), (what, "counts", np.flatnonzero(g_cnt != w_cnt)[:5])
    assert np.array_equal(g_ids, w_ids), (what, "ids", np.argwhere(g_ids != w_ids)[:5])
    assert np.array_equal(bits(g_sc), bits(w_sc)), (what, "scores", np.argwhere(bits(g_sc) != bits(w_sc))[:5])


# ---------------------------------------------------------------------------------------------- the blend
def _cut(ids, scores, count, n_items):
    n = max(0, min(int(count), len(ids)))
    for p in range(n):
        s = float(scores[p])
        if not (0 <= int(ids[p]) < n_items) or not math.isfinite(s) or s <= -FLT_MAX:
            return p
    return n


def blend_row_plain(n_items, a_ids, a_scores, a_count, a_div, b_ids, b_scores, b_count, exclude, sum_dtype=np.float64):
    """THE DEFINITION for one row, one step at a time: [(id, value, source)] of the whole union in order.  `sum_dtype`
    float32 is what the contract does NOT do (the pinning tests)."""
    lists = []
    for which, (ids, sc, cnt) in enumerate(((a_ids, a_scores, a_count), (b_ids, b_scores, b_count))):
        n = _cut(ids, sc, cnt, n_items)
        kept = [(int(ids[p]), F32(sc[p])) for p in range(n) if exclude is None or int(ids[p]) != int(exclude)]
        if which == 0 and a_div is not None:
            kept = [(i, f32div(s, a_div)) for i, s in kept] if a_div > 0 else []
        if kept:
            mn, mx = kept[0][1], kept[0][1]
            for _, s in kept:
                mn, mx = (s if s < mn else mn), (s if s > mx else mx)
            with np.errstate(all="ignore"):
                den = F32(F32(mx - mn) + F32(1e-8))
                kept = [(i, F32(F32(s - mn) / den)) for i, s in kept]
        lists.append(kept)
    total, order = {}, []
    for kept in lists:                                   # comb_sum: a defaultdict(float), A first, += per occurrence
        for i, s in kept:
            if i not in total:
                total[i] = sum_dtype(0.0)
                order.append(i)
            with np.errstate(all="ignore"):
                total[i] = sum_dtype(total[i] + sum_dtype(s))
    in_a, in_b = {i for i, _ in lists[0]}, {i for i, _ in lists[1]}
    entries = [(i, total[i], (1 if i in in_a else 0) + (2 if i in in_b else 0)) for i in order if total[i] == total[i]]
    return sorted(entries, key=lambda e: float(e[1]), reverse=True)           # (stable: equal values keep the union's order)


def blend_row_fast(n_items, a_ids, a_scores, a_count, a_div, b_ids, b_scores, b_count, exclude, sum_dtype=np.float64):
    """blend_row_plain on arrays: the cut by a cumulative test, the normalisation as array expressions, the k-th occurrences of
    all ids added together (so every id sees its occurrences in order), a stable argsort."""
    parts = []
    with np.errstate(all="ignore"):
        for which, (ids, sc, cnt) in enumerate(((a_ids, a_scores, a_count), (b_ids, b_scores, b_count))):
            ids, sc = np.asarray(ids, np.int64), np.asarray(sc, F32)
            n = max(0, min(int(cnt), len(ids)))
            ok = (ids[:n] >= 0) & (ids[:n] < n_items) & np.isfinite(sc[:n]) & (sc[:n] > F32(-FLT_MAX))
            n = int(np.argmin(ok)) if not ok.all() else n
            keep = np.ones(n, bool) if exclude is None else ids[:n] != int(exclude)
            ids, sc = ids[:n][keep], sc[:n][keep]
            if which == 0 and a_div is not None:
                if a_div > 0:
                    sc = sc / F32(a_div)
                else:
                    ids, sc = ids[:0], sc[:0]
            if len(sc):
                mn, mx = sc.min(), sc.max()
                sc = (sc - mn) / F32(F32(mx - mn) + F32(1e-8))
            parts.append((ids, sc))
        ids = np.concatenate([parts[0][0], parts[1][0]])
        terms = np.concatenate([parts[0][1], parts[1][1]]).astype(sum_dtype)
        if not len(ids):
            return []
        uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
        occ = np.zeros(len(ids), np.int64)                  # the how-manieth occurrence of its id
        seen = np.zeros(len(uniq), np.int64)
        for e in range(len(ids)):
            occ[e] = seen[inv[e]]; seen[inv[e]] += 1
        value = np.zeros(len(uniq), sum_dtype)
        for k in range(int(occ.max()) + 1):
            at = occ == k
            value[inv[at]] = (value[inv[at]] + terms[at]).astype(sum_dtype)
    src = np.isin(uniq, parts[0][0]).astype(int) + 2 * np.isin(uniq, parts[1][0]).astype(int)
    by_first = np.argsort(first, kind="stable")
    uniq, value, src = uniq[by_first], value[by_first], src[by_first]
    live = ~np.isnan(value)
    uniq, value, src = uniq[live], value[live], src[live]
    order = np.argsort(-(value.astype(np.float64) + 0.0), kind="stable")
    return [(int(uniq[o]), value[o], int(src[o])) for o in order]


def host_blend(n_items, A, B, keep, a_div=None, exclude=None, row_fn=blend_row_fast, sum_dtype=np.float64):
    """(ids[R, keep] int32, value[R, keep] float64, source[R, keep] int32, count[R] int32) for A = (ids[R, ka], scores[R, ka],
    counts[R]) and B in the same form."""
    R = len(A[0])
    ids = np.full((R, keep), -1, np.int32)
    value = np.full((R, keep), -np.inf, np.float64)
    source = np.zeros((R, keep), np.int32)
    count = np.zeros(R, np.int32)
    for r in range(R):
        row = row_fn(n_items, A[0][r], A[1][r], A[2][r], None if a_div is None else F32(a_div[r]), B[0][r], B[1][r], B[2][r],
                     None if exclude is None else exclude[r], sum_dtype=sum_dtype)[:keep]
        count[r] = len(row)
        for t, (i, v, s) in enumerate(row):
            ids[r, t], value[r, t], source[r, t] = i, float(v), s
    return ids, value, source, count


def assert_same_blend(got, want, what=""):
    g_ids, g_val, g_src, g_cnt = [np.asarray(a) for a in got]
    w_ids, w_val, w_src, w_cnt = [np.asarray(a) for a in want]
    assert np.array_equal(g_cnt, w_cnt), (what, "counts", np.flatnonzero(g_cnt != w_cnt)[:5])
    assert np.array_equal(g_ids, w_ids), (what, "ids", np.argwhere(g_ids != w_ids)[:5])
    assert np.array_equal(g_src, w_src), (what, "source", np.argwhere(g_src != w_src)[:5])
    assert np.array_equal(dbits(g_val), dbits(w_val)), (what, "values", np.argwhere(dbits(g_val) != dbits(w_val))[:5])


def pad(rows, width, fill, dtype):
    out = np.full((len(rows), width), fill, dtype)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out


def lists_of(rows_ids, rows_scores, width=None):
    """(ids[R, width] int32, scores[R, width] float32, counts[R] int32) of ragged lists."""
    width = max([1] + [len(r) for r in rows_ids]) if width is None else width
    return (pad(rows_ids, width, -1, np.int32), pad(rows_scores, width, 0.0, F32), np.array([len(r) for r in rows_ids], np.int32))


def host_slim_similar(W, q, top_k):
    """rtrec_slim_similar_topk for one query: the stored entries of W's column q, q itself dropped, the larger value first,
    the lower row among equal ones: (ids, float32 scores)."""
    W = W.tocsc()
    lo, hi = W.indptr[q], W.indptr[q + 1]
    rows, vals = W.indices[lo:hi], W.data[lo:hi].astype(F32)
    keep = rows != q
    rows, vals = rows[keep], vals[keep]
    order = np.lexsort((rows, -vals.astype(np.float64)))[:top_k]
    return rows[order].astype(np.int64), vals[order]


# ---------------------------------------------------------------------------------------------- the two models of each agree
def special_vectors(n, dim, seed):
    """Vectors with zero, denormal, near-overflow and ordinary rows, and rounding-sensitive ones between them."""
    V = rounding_vectors(n, 1, dim, seed)[0]
    rng = np.random.default_rng(seed)
    V[1 % n] = 0.0
    V[2 % n] = F32(2.0 ** -140) * rng.integers(1, 200, dim).astype(F32)          # squares underflow to denormals or zero
    V[3 % n] = F32(2.0 ** -80) * rng.integers(64, 256, dim).astype(F32)          # every square and n2 itself are denormals
    V[4 % n] = F32(1.5e19) * rng.choice(np.array([1, -1], F32), dim)             # n2 is near FLT_MAX for small dims, inf beyond
    V[5 % n] = F32(3.0e38)                                                       # n2 overflows
    return V


@pytest.mark.parametrize("dim", [1, 2, 3, 13, 64, 256])
def test_both_norm_models_agree(dim):
    V = special_vectors(40, dim, seed=dim)
    plain, fast = host_norms_plain(V), host_norms_fast(V)
    assert np.array_equal(plain.view(np.int32), fast.view(np.int32))
    assert plain[1] == 0 and np.isinf(plain[5]) and (plain[3] > 0)
    # the norm is the root of rtrec_factor_topk's score of the vector with itself
    own = np.array([host_scores(V[r:r + 1], V[r:r + 1])[0, 0] for r in range(len(V))], F32)
    with np.errstate(all="ignore"):
        assert np.array_equal(np.sqrt(own.astype(np.float64)).astype(F32).view(np.int32), plain.view(np.int32))


@pytest.mark.parametrize("dim", [1, 2, 3, 12, 13, 64])
def test_both_similar_models_agree_on_rounding_sensitive_vectors(dim):
    P, Q = rounding_vectors(6, 18, dim, seed=100 + dim)
    Q[3] = 0.0                                                                   # a zero vector: 0 / 0 never competes
    norms = host_norms_fast(Q)
    queries = [0, 3, 17, -1, 18, 5]
    mask = (np.arange(18) % 5 != 4).astype(np.uint8)
    for kw in (dict(), dict(mask=mask), dict(write_cosine=True), dict(P=P, p_norms=host_norms_fast(P)),
               dict(P=P, p_norms=host_norms_fast(P), write_cosine=True, mask=mask)):
        plain = host_similar_plain(Q, norms, queries, 17, **kw)
        fast = host_similar_fast(Q, norms, queries, 17, **kw)
        assert_same_lists(fast, plain, f"dim {dim} {sorted(kw)}")
        assert np.array_equal(plain[3].view(np.int32), fast[3].view(np.int32))
        ids, sc, cnt, div = plain
        for r, q in enumerate(queries):
            assert q not in ids[r, :cnt[r]].tolist() and 3 not in ids[r, :cnt[r]].tolist()
            if "P" not in kw and not 0 <= q < 18:
                assert cnt[r] == 0 and div[r] == 0
        if "P" not in kw and kw.get("write_cosine"):
            assert cnt[1] == 0 and div[1] == 0                                   # the zero vector as a query: its norm is not > 0


def test_both_similar_models_agree_on_long_chains_and_ties():
    P, Q = rounding_vectors(2, 7, 256, seed=9)
    norms = host_norms_fast(Q)
    assert_same_lists(host_similar_fast(Q, norms, [0, 6], 6), host_similar_plain(Q, norms, [0, 6], 6), "dim 256")
    Q = np.tile(np.array([[1.0, 2.0, 2.0]], F32), (9, 1))                        # all scores equal: ties go to the lower id
    norms = host_norms_fast(Q)
    for model in (host_similar_plain, host_similar_fast):
        ids, sc, cnt, _ = model(Q, norms, [4, 0], 5, write_cosine=True)
        assert ids.tolist() == [[0, 1, 2, 3, 5], [1, 2, 3, 4, 5]] and cnt.tolist() == [5, 5] and (sc == 1.0).all()
        ids, sc, cnt, _ = model(Q, norms, None, 20, P=Q[:1], p_norms=norms[:1])
        assert cnt[0] == 9 and ids[0, :9].tolist() == list(range(9)) and (ids[0, 9:] == -1).all() and np.isneginf(sc[0, 9:]).all()


_ONE_SCAN = []


def one_scan_cases():
    """[(name, P, Q, p_norms, {top_k: host_model_fast's answer})] on which rtrec_factor_similar_topk with item norms of 1.0f, no
    queries, no mask and no cosine must BE rtrec_factor_topk without a filter (x / 1.0f is exact): 33 jobs (a second workgroup with
    one live lane) x 161 items (five whole tiles and one item) at dim 13 (odd: a zero-padded k-step), once on rounding_vectors and
    once with small-integer scores that rise with the item id (exact in float32, so every item beats the threshold and a 64-entry
    buffer compacts several times within 161 items at top_k 10).  Computed once; tests/test_gpu_similar.py runs both ops on them."""
    from tests.test_factor_host import host_model_fast
    if not _ONE_SCAN:
        rng = np.random.default_rng(131)
        P, Q = rounding_vectors(33, 161, 13, seed=131)
        P2 = rng.integers(1, 5, (33, 13)).astype(F32)
        Q2 = (np.arange(161)[:, None] * (1 + np.arange(13)[None, :] % 3)).astype(F32)
        for name, p, q in (("rounding", P, Q), ("rising", P2, Q2)):
            p_norms = (rng.random(33) * 9 + 0.5).astype(F32)                      # any positive values: they are not read for s1
            _ONE_SCAN.append((name, p, q, p_norms, {k: host_model_fast(p, q, k) for k in (10, 128)}))
    return _ONE_SCAN


def test_similar_with_unit_norms_is_the_factor_model():
    """The premise of the one-scan GPU test, shown with the two host models: with unit item norms and nothing excluded,
    host_similar_fast equals host_model_fast, ids, counts and score bits."""
    for name, P, Q, p_norms, want in one_scan_cases():
        ones = np.ones(len(Q), F32)
        for top_k in (10, 128):
            ids, sc, cnt, div = host_similar_fast(Q, ones, None, top_k, P=P, p_norms=p_norms)
            w_ids, w_sc, w_cnt = want[top_k]
            assert np.array_equal(ids, w_ids) and np.array_equal(cnt, w_cnt) and (cnt == top_k).all(), (name, top_k)
            assert np.array_equal(sc.view(np.int32), w_sc.view(np.int32)) and np.array_equal(div, p_norms), (name, top_k)
        if name == "rising":
            assert (want[10][0] == np.arange(160, 150, -1)).all() and (np.diff(host_scores(P, Q), axis=1) > 0).all()


# ---------------------------------------------------------------------------------------------- cases for the device tests
def same_or_both_nan(got, want, what=""):
    """assert_same_lists for lists that may hold a NaN SCORE (fl(+-inf / +inf) with write_cosine and an infinite query norm): ids
    and counts with ==, a score by its bits, a NaN by being one -- its sign and payload are not part of the contract (x86's
    default NaN is negative, the device's positive)."""
    g_ids, g_sc, g_cnt = [np.asarray(a) for a in got[:3]]
    w_ids, w_sc, w_cnt = [np.asarray(a) for a in want[:3]]
    assert np.array_equal(g_cnt, w_cnt), (what, "counts", g_cnt, w_cnt)
    assert np.array_equal(g_ids, w_ids), (what, "ids", np.argwhere(g_ids != w_ids)[:5])
    ok = (bits(g_sc) == bits(w_sc)) | (np.isnan(g_sc) & np.isnan(w_sc))
    assert ok.all(), (what, "scores", np.argwhere(~ok)[:5])
    if len(got) > 3 and got[3] is not None:
        g, w = np.asarray(got[3], F32), np.asarray(want[3], F32)
        assert ((g.view(np.int32) == w.view(np.int32)) | (np.isnan(g) & np.isnan(w))).all(), (what, "div")


def similar_class_case(dim):
    """tests/test_factor_host.py's class_edge_case as a similar-items call: 200 items, the first 40 as queries."""
    from tests.test_factor_host import class_edge_case
    _, Q = class_edge_case(dim)
    Q[:, dim - 1] = F32(8.0) * np.where(np.arange(200) % 3 == 0, -1, 1).astype(F32)
    return Q, host_norms_fast(Q), np.arange(40, dtype=np.int32)


def similar_operand_case(dim):
    """test_operand_map_on_an_asymmetric_integer_matrix of tests/test_gpu_similar.py at any dim."""
    n_items = 40
    i, c = np.meshgrid(np.arange(n_items), np.arange(dim), indexing="ij")
    Q = (i * 37 + c * 3 + (i * c) % 5 - 400).astype(F32)
    return Q, host_norms_fast(Q), np.r_[np.arange(n_items), [3]].astype(np.int32)


ODD_NORMS = (np.nan, np.inf, None, 1e-45, -np.inf, -0.0)            # None: the item's own norm, negated


def caller_norms_case(seed=12):
    """The norms are the caller's: 100 items of dim 6 whose computed norms are overwritten at six items with NaN, +inf, a negated
    value, a denormal (1e-45), -inf and -0.0; the queries are an ordinary item, those six and another ordinary one.  As a DIVISOR
    of s1 they make NaN (never competes), +-0, a sign flip, +-inf (competes as a number: it leads or ends the list) and -+0; as a
    QUERY norm with write_cosine only +inf and the denormal are > 0.  (Q, norms, queries, odd items)."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((100, 6)).astype(F32)
    norms = host_norms_fast(Q)
    odd = np.array([11, 23, 37, 52, 68, 90])
    for i, v in zip(odd, ODD_NORMS):
        norms[i] = -norms[i] if v is None else F32(v)
    return Q, norms, np.r_[[3], odd, [77]].astype(np.int32), odd


def query_norms_case(seed=12):
    """caller_norms_case with brought vectors whose norms are the caller's too: NaN, +inf, a negative value, -0.0, a denormal and
    two ordinary ones.  (Q, norms, P, p_norms)."""
    Q, norms, _, _ = caller_norms_case(seed)
    rng = np.random.default_rng(seed + 1)
    P = rng.standard_normal((7, 6)).astype(F32)
    p_norms = host_norms_fast(P)
    p_norms[:5] = [np.nan, np.inf, -p_norms[2], -0.0, 1e-45]
    return Q, norms, P, p_norms


def similar_trip_case(seed=17, extra=40):
    """More jobs than the similar merge kernel's grid (65,536): 65,536 + 40 jobs over 64 items (two chunks of one tile), dim 2,
    top_k 3, write_cosine.  A pattern's query is a live item, the zero-norm item 7 (an empty cosine list) or outside the
    catalogue (no vector); the brought vectors of the second form are ordinary or zero (norm 0).  Norms are zero or ordinary
    here: the odd ones have caller_norms_case.  Returns a dict."""
    from tests.test_factor_host import GRID_CAP, PATTERNS, pattern_of
    rng = np.random.default_rng(seed)
    n_rows = GRID_CAP + extra
    Q = rng.standard_normal((64, 2)).astype(F32)
    Q[7] = 0.0
    norms = host_norms_fast(Q)
    kind = rng.integers(0, 3, PATTERNS)                                 # 0 live, 1 the zero-norm item, 2 outside the catalogue
    kind[:6], kind[384:390] = [0, 1, 0, 2, 1, 2], [1, 0, 2, 0, 0, 1]
    live = rng.integers(0, 64, PATTERNS)
    live[live == 7] = 8
    outside = rng.choice(np.array([-1, 64, 2 ** 31 - 1, -2 ** 31]), PATTERNS)
    queries = np.where(kind == 0, live, np.where(kind == 1, 7, outside)).astype(np.int32)
    P = rng.standard_normal((PATTERNS, 2)).astype(F32)
    P[kind != 0] = 0.0
    return dict(Q=Q, norms=norms, queries=queries, P=P, p_norms=host_norms_fast(P), kind=kind, at=pattern_of(n_rows), n_rows=n_rows, top_k=3,
                splits=2)


def blend_trip_case(seed=23, extra=3):
    """More rows than the list stage's grid (65,536): 65,536 + 3 rows of ka = kb = 4, keep 5, ids below 30.  The patterns: 0 full
    lists with an id repeated in A, one shared with B and one of A's ids excluded (a hole); 1 an empty A; 2 an empty B; 3 a divisor
    that is not > 0; 4 A cut at position 1 by a non-finite score.  Returns (n_items, A, B, a_div, exclude, kind), per pattern."""
    from tests.test_factor_host import PATTERNS
    rng = np.random.default_rng(seed)
    n_items = 30
    kind = rng.integers(0, 5, PATTERNS)
    kind[:3], kind[384:387] = [0, 4, 3], [1, 0, 0]
    both = np.stack([rng.permutation(n_items)[:8] for _ in range(PATTERNS)]).astype(np.int32)        # (disjoint before the repeats are made)
    a_ids, b_ids = both[:, :4].copy(), both[:, 4:].copy()
    a_ids[:, 2] = a_ids[:, 0]                                            # A repeats its first id
    b_ids[:, 1] = a_ids[:, 1]                                            # ... and shares its second with B
    desc = lambda: (-np.sort(-rng.standard_normal((PATTERNS, 4)), axis=1)).astype(F32)
    a_sc, b_sc = desc(), desc()
    a_cnt, b_cnt = np.full(PATTERNS, 4, np.int32), np.full(PATTERNS, 4, np.int32)
    a_cnt[kind == 1], b_cnt[kind == 2], b_cnt[kind == 4] = 0, 0, 2
    a_div = (0.5 + rng.random(PATTERNS)).astype(F32)
    bad = np.flatnonzero(kind == 3)
    a_div[bad] = np.array([0.0, -2.0, np.nan, -0.0], F32)[np.arange(len(bad)) % 4]
    cut = np.flatnonzero(kind == 4)
    a_sc[cut, 1] = np.array([np.inf, np.nan, -np.inf, -FLT_MAX], F32)[np.arange(len(cut)) % 4]
    exclude = np.where(kind == 0, a_ids[:, 3], np.where(rng.random(PATTERNS) < 0.5, -1, b_ids[:, 0])).astype(np.int32)
    return n_items, (a_ids, a_sc, a_cnt), (b_ids, b_sc, b_cnt), a_div, exclude, kind


@pytest.mark.parametrize("dim", [15, 16, 17, 31, 32, 33, 63, 65, 129])
def test_both_similar_models_agree_on_the_class_edge_dims(dim):
    """The device rounding test's own case at the dims around the scan's class rules: the plain definition on 12 of its 96
    queries, and the last component moves bits of s1 for most queries."""
    _, Q = rounding_vectors(1, 96, dim, seed=dim)
    Q[5] = 0.0
    norms = host_norms_fast(Q)
    some = np.arange(0, 96, 8, dtype=np.int32)
    for cosine in (False, True):
        fast = host_similar_fast(Q, norms, np.arange(96, dtype=np.int32), 95, write_cosine=cosine)
        plain = host_similar_plain(Q, norms, some, 95, write_cosine=cosine)
        assert_same_lists([a[some] for a in fast[:3]], plain, (dim, cosine))
    with np.errstate(all="ignore"):
        full, less = host_s1(Q, Q, norms), host_s1(Q[:, :dim - 1], Q[:, :dim - 1], norms)
    assert int((bits(full) != bits(less)).any(axis=1).sum()) > 48


@pytest.mark.parametrize("dim", [17, 65])
def test_similar_class_case_hangs_on_its_last_component(dim):
    Q, norms, queries = similar_class_case(dim)
    want = host_similar_fast(Q, norms, queries, 65, write_cosine=True)
    assert_same_lists(want, host_similar_plain(Q, norms, queries, 65, write_cosine=True), dim)
    assert (want[2] == 65).all()
    less = host_similar_fast(Q[:, :dim - 1], host_norms_fast(Q), queries, 17)
    assert (less[0] != want[0][:, :17]).any(axis=1).all()


@pytest.mark.parametrize("dim", [13, 33])
def test_similar_operand_case_at_odd_dims(dim):
    Q, norms, queries = similar_operand_case(dim)
    want = host_similar_fast(Q, norms, queries, 40)
    assert_same_lists(want, host_similar_plain(Q, norms, queries, 40), dim)
    assert (want[2] == 39).all() and np.array_equal(want[3], norms[queries])


def test_caller_norms_cases_are_the_definition_and_stay_odd():
    Q, norms, queries, odd = caller_norms_case()
    assert np.isnan(norms[odd[0]]) and np.isposinf(norms[odd[1]]) and norms[odd[2]] < 0 and 0 < norms[odd[3]] < 2.0 ** -126
    assert np.isneginf(norms[odd[4]]) and norms[odd[5]] == 0 and np.signbit(norms[odd[5]])
    for top_k in (20, 99):
        for cosine in (False, True):
            want = host_similar_fast(Q, norms, queries, top_k, write_cosine=cosine)
            with np.errstate(over="ignore"):
                same_or_both_nan(want, host_similar_plain(Q, norms, queries, top_k, write_cosine=cosine), (top_k, cosine))
            listed = want[1][np.arange(top_k)[None, :] < want[2][:, None]]
            assert np.isinf(listed).any(), "infinite scores must be listed"
            if top_k == 20:                                                 # (fl(inf / inf) of the +inf query norm: two NaN scores)
                assert (int(np.isinf(listed).sum()), int(np.isnan(listed).sum())) == ((23, 2) if cosine else (9, 0))
            # nobody lists the NaN-norm item; the two items whose norm is a zero or a denormal lead or end every other live list
            assert not (want[0] == odd[0]).any()
            n = min(top_k, 98)                                              # 100 items less the query and the NaN-norm item
            assert want[2].tolist() == ([n, 0, n, 0, n, 0, 0, n] if cosine else [n, min(top_k, 99), n, n, n, n, n, n])
    Q, norms, P, p_norms = query_norms_case()
    for cosine in (False, True):
        want = host_similar_fast(Q, norms, None, 20, P=P, p_norms=p_norms, write_cosine=cosine)
        with np.errstate(over="ignore"):
            same_or_both_nan(want, host_similar_plain(Q, norms, None, 20, P=P, p_norms=p_norms, write_cosine=cosine), cosine)
        assert want[2].tolist() == ([0, 20, 0, 0, 20, 20, 20] if cosine else [20] * 7)
        assert np.array_equal(want[3].view(np.int32), p_norms.view(np.int32))


def test_similar_trip_case_is_the_definition_and_sets_live_against_dead_across_the_cap():
    from tests.test_factor_host import GRID_CAP, PATTERNS
    case = similar_trip_case()
    Q, norms, kind, at = case["Q"], case["norms"], case["kind"], case["at"]
    want = host_similar_fast(Q, norms, case["queries"], 3, write_cosine=True)
    assert_same_lists(want, host_similar_plain(Q, norms, case["queries"], 3, write_cosine=True), "queries")
    assert np.array_equal(want[2], np.where(kind == 0, 3, 0))
    brought = host_similar_fast(Q, norms, case["queries"], 3, P=case["P"], p_norms=case["p_norms"], write_cosine=True)
    assert_same_lists(brought, host_similar_plain(Q, norms, case["queries"], 3, P=case["P"], p_norms=case["p_norms"], write_cosine=True), "brought")
    assert np.array_equal(brought[2], np.where(kind == 0, 3, 0)) and len(kind) == PATTERNS
    early, late = kind[at[:case["n_rows"] - GRID_CAP]] == 0, kind[at[GRID_CAP:]] == 0
    assert (early & ~late).any() and (~early & late).any() and (early & late).any()
    assert {1, 2} <= set(kind[at[GRID_CAP:]].tolist()) and {1, 2} <= set(kind[at[:40]].tolist())


def test_blend_trip_case_is_the_definition_and_changes_the_unions_length_across_the_cap():
    n_items, A, B, a_div, exclude, kind = blend_trip_case()
    want = host_blend(n_items, A, B, 5, a_div=a_div, exclude=exclude)
    assert_same_blend(want, host_blend(n_items, A, B, 5, a_div=a_div, exclude=exclude, row_fn=blend_row_plain), "patterns")
    union = host_blend(n_items, A, B, 8, a_div=a_div, exclude=exclude)[3]
    assert set(kind.tolist()) == {0, 1, 2, 3, 4}
    assert (union[kind == 0] == 5).all() and (union[kind == 1] <= 4).all() and (union[kind == 3] <= 4).all() and (union[kind == 4] <= 3).all()
    assert (want[2][kind == 0] == 3).any(), "an id of both lists"
    early, late = union[:3], union[384:387]                             # rows 0 .. 2 and 65,536 .. 65,538 share their workgroups
    assert (early != late).all() and (early > late).any() and (early < late).any()


# ---------------------------------------------------------------------------------------------- pinning: what the roundings are worth
def test_other_ways_to_divide_change_bits_of_s1():
    rng = np.random.default_rng(12)
    Q = rng.standard_normal((300, 12)).astype(F32)
    norms = host_norms_fast(Q)
    V = Q[:20]
    dot = host_scores(V, Q)
    s1 = host_s1(V, Q, norms)
    cos = s1 / norms[:20, None]                                                  # the contract: two divisions, the item's first
    with np.errstate(all="ignore"):
        at_once = dot / (norms[None, :] * norms[:20, None])                      # one division by the product of the norms
        recip = dot * (F32(1.0) / norms)[None, :]                                # a reciprocal and a multiply
        n2 = np.zeros(len(Q), F32)
        for c in range(12):
            n2 = fma32(Q[:, c], Q[:, c], n2)
        wide = (dot.astype(np.float64) / np.sqrt(n2.astype(np.float64))[None, :]).astype(F32)    # the divisor never rounded to float32
    counts = {"product of the norms": int((bits(at_once) != bits(cos)).sum()), "reciprocal": int((bits(recip) != bits(s1)).sum()),
              "float64 divisor": int((bits(wide) != bits(s1)).sum())}
    print("s1 bits changed out of", s1.size, counts)
    assert all(n > 0 for n in counts.values()), counts


def test_numpys_norm_differs_from_the_chain_on_some_vectors():
    rng = np.random.default_rng(13)
    changed = {}
    for dim in (12, 64):
        V = rng.standard_normal((3000, dim)).astype(F32)
        changed[dim] = int((np.linalg.norm(V, axis=1).view(np.int32) != host_norms_fast(V).view(np.int32)).sum())
    print("norms that differ from np.linalg.norm out of 3000:", changed)
    assert all(n > 0 for n in changed.values()), changed


def order_case():
    """Two entries of A tie at the maximum and the later one also stands in B with a normalised score of 1e-9: 1 + 1e-9 is 1 in
    float32 and more than 1 in float64, so only the float64 sum puts the later one first."""
    A = lists_of([[7, 3, 5]], [[2.0, 2.0, 1.0]])
    B = lists_of([[9, 3, 11]], [[1.0, 1e-9, 0.0]])
    return 24, A, B


def test_float32_addition_changes_values_and_in_the_crafted_case_the_order():
    n_items, A, B = order_case()
    for row_fn in (blend_row_plain, blend_row_fast):
        ids64, val64, src64, cnt64 = host_blend(n_items, A, B, 6, row_fn=row_fn)
        ids32, val32, _, _ = host_blend(n_items, A, B, 6, row_fn=row_fn, sum_dtype=np.float32)
        assert ids64[0, :5].tolist() == [3, 7, 9, 5, 11] and ids32[0, :5].tolist() == [7, 3, 9, 5, 11] and cnt64[0] == 5
        assert val64[0, 0] > 1.0 and val32[0, 0] == val32[0, 1] == 1.0 and src64[0, :5].tolist() == [3, 1, 2, 1, 2]
    cases = golden_cases()[1]
    changed = 0
    for c in cases:
        A, B = lists_of([c["a_ids"]], [c["a_scores"]]), lists_of([c["b_ids"]], [c["b_scores"]])
        kw = dict(a_div=[c["query_norm"]], exclude=[c["query"]])
        v64 = host_blend(c["n_items"], A, B, c["top_k"], **kw)[1]
        v32 = host_blend(c["n_items"], A, B, c["top_k"], sum_dtype=np.float32, **kw)[1]
        changed += int((dbits(v64) != dbits(v32)).any())
    print("golden cases whose value bits a float32 comb_sum changes:", changed, "of", len(cases))
    assert changed > 0


# ---------------------------------------------------------------------------------------------- the reference's answers
def golden_cases():
    """(the file's header, its cases as dicts by `case_fields`): lists are stored as base64 of their little-endian bytes (int16
    ids, float32 scores and norm, float64 answers), so every bit survives."""
    g = json.load(open(GOLDEN))
    un = lambda t, dt: np.frombuffer(base64.b64decode(t), dt).astype(np.float64).tolist()
    cases = [dict(zip(g["case_fields"], c)) for c in g["cases"]]
    for c in cases:
        c["query_norm"], c["a_scores"], c["b_scores"] = un(c["query_norm"], "<f4")[0], un(c["a_scores"], "<f4"), un(c["b_scores"], "<f4")
        c["values"] = un(c["values"], "<f8")
        for key in ("a_ids", "b_ids", "ids"):
            c[key] = np.frombuffer(base64.b64decode(c[key]), "<i2").astype(int).tolist()
    return g, cases


def golden_inputs(cases):
    """The golden cases as one batch per list: (A, B, a_div, exclude, keep per case)."""
    A = lists_of([c["a_ids"] for c in cases], [c["a_scores"] for c in cases])
    B = lists_of([c["b_ids"] for c in cases], [c["b_scores"] for c in cases])
    return A, B, np.array([c["query_norm"] for c in cases], F32), np.array([c["query"] for c in cases], np.int32)


def golden_answer(c):
    return [int(i) for i in c["ids"]], c["values"]


@pytest.mark.parametrize("row_fn", [blend_row_plain, blend_row_fast])
def test_both_blend_models_reproduce_the_reference(row_fn):
    g, cases = golden_cases()
    assert len(cases) == g["n_fixture"] + g["n_small"] and g["n_fixture"] == 400 and g["n_small"] == 60
    cond = g["conditions"]
    assert cond["share_an_item"] >= 100 and cond["value_not_float32"] >= 50 and cond["order_float32_would_change"] >= 1
    for n, c in enumerate(cases):
        A, B = lists_of([c["a_ids"]], [c["a_scores"]]), lists_of([c["b_ids"]], [c["b_scores"]])
        assert F32(c["query_norm"]) == c["query_norm"] and all(F32(s) == s for s in c["a_scores"] + c["b_scores"])
        ids, value, source, count = host_blend(c["n_items"], A, B, c["top_k"], a_div=[c["query_norm"]], exclude=[c["query"]], row_fn=row_fn)
        w_ids, w_val = golden_answer(c)
        assert ids[0, :count[0]].tolist() == w_ids, n
        assert np.array_equal(dbits(value[0, :count[0]]), dbits(w_val)), n
    # the recorded conditions are true of the file
    share = sum(bool(set(c["a_ids"]) & set(c["b_ids"])) for c in cases[:400])
    wide = sum(any(float(F32(v)) != v for v in golden_answer(c)[1]) for c in cases[:400])
    assert share == cond["share_an_item"] and wide == cond["value_not_float32"]


def test_both_blend_models_agree_on_seeded_lists_with_repeats():
    rng = np.random.default_rng(21)
    rows_a, sc_a, rows_b, sc_b = [], [], [], []
    for r in range(120):
        la, lb = int(rng.integers(0, 14)), int(rng.integers(0, 14))
        rows_a.append(rng.integers(0, 16, la).tolist()); rows_b.append(rng.integers(0, 16, lb).tolist())
        sc_a.append((-np.sort(-rng.standard_normal(la))).astype(F32).tolist())
        sc_b.append((np.full(lb, 0.25) if r % 7 == 0 else -np.sort(-rng.standard_normal(lb))).astype(F32).tolist())
    A, B = lists_of(rows_a, sc_a), lists_of(rows_b, sc_b)
    div = np.abs(rng.standard_normal(120)).astype(F32) + F32(0.1)
    div[5], div[6], div[7] = 0.0, -1.0, np.nan
    ex = rng.integers(-1, 16, 120).astype(np.int32)
    want = host_blend(16, A, B, 20, a_div=div, exclude=ex, row_fn=blend_row_plain)
    assert_same_blend(host_blend(16, A, B, 20, a_div=div, exclude=ex, row_fn=blend_row_fast), want)
    assert (want[2][5:8] != 1).all() and (want[2][5:8] != 3).all()               # a divisor that is not > 0 empties A
    assert (want[0][ex >= 0] != ex[ex >= 0, None]).all() and (ex == -1).any()


# ---------------------------------------------------------------------------------------------- the contract's edges
@pytest.mark.parametrize("row_fn", [blend_row_plain, blend_row_fast])
def test_blend_contract_edges(row_fn):
    run = lambda A, B, keep, **kw: host_blend(24, A, B, keep, row_fn=row_fn, **kw)
    none = lists_of([[]], [[]])
    one = lists_of([[4, 6, 2]], [[3.0, 2.0, 1.0]])
    # both lists empty, or one: the reference raises ValueError there; an empty list contributes nothing
    ids, value, source, count = run(none, none, 2)
    assert count[0] == 0 and (ids == -1).all() and np.isneginf(value).all() and (source == 0).all()
    ids, value, source, count = run(one, none, 4)
    assert ids[0].tolist() == [4, 6, 2, -1] and source[0].tolist() == [1, 1, 1, 0] and count[0] == 3
    assert value[0, 0] == float(F32(2.0) / F32(F32(2.0) + F32(1e-8))) and value[0, 2] == 0.0
    ids, value, source, count = run(none, one, 3)
    assert ids[0].tolist() == [4, 6, 2] and source[0].tolist() == [2, 2, 2]
    # an all-equal list normalises to zeros: the union's order decides
    flat = lists_of([[8, 1, 5]], [[0.7, 0.7, 0.7]])
    ids, value, _, count = run(flat, flat, 6)
    assert ids[0, :3].tolist() == [8, 1, 5] and (value[0, :3] == 0).all() and count[0] == 3
    # repeated ids add once per occurrence, in A and in B (NOT blend_lists' "the last score of A")
    A = lists_of([[3, 3, 9]], [[4.0, 2.0, 0.0]])
    B = lists_of([[9, 9, 3]], [[1.0, 0.5, 0.0]])
    ids, value, source, count = run(A, B, 6)
    na = [float(F32(F32(s) / F32(F32(4.0) + F32(1e-8)))) for s in (4.0, 2.0)]
    nb = [float(F32(F32(s) / F32(F32(1.0) + F32(1e-8)))) for s in (1.0, 0.5)]
    assert ids[0, :2].tolist() == [3, 9] and source[0, :2].tolist() == [3, 3] and count[0] == 2
    assert value[0, 0] == (na[0] + na[1]) + 0.0 and value[0, 1] == (0.0 + nb[0]) + nb[1]
    # the query id is taken out of both lists, before the extremes are taken
    A = lists_of([[5, 2, 7]], [[9.0, 2.0, 1.0]])
    B = lists_of([[7, 5, 1]], [[3.0, 2.0, 1.0]])
    ids, value, source, count = run(A, B, 6, exclude=[5])
    # A is left with 2 (2.0) and 7 (1.0): 1 and 0; B with 7 (3.0) and 1 (1.0): 1 and 0; 2 and 7 tie at 1, the union's order decides
    assert 5 not in ids[0].tolist() and count[0] == 3 and value[0, :3].tolist() == [1.0, 1.0, 0.0]
    assert ids[0, :3].tolist() == [2, 7, 1] and source[0, :3].tolist() == [1, 3, 2]
    # a divisor of 0, a negative one and NaN empty A; a positive one divides before the normalisation
    for d in (0.0, -2.0, np.nan):
        ids, value, source, count = run(A, B, 6, a_div=[d])
        assert ids[0, :3].tolist() == [7, 5, 1] and (source[0, :3] == 2).all() and count[0] == 3
    assert_same_blend(run(A, B, 6, a_div=[4.0]), run(lists_of([[5, 2, 7]], [[2.25, 0.5, 0.25]]), B, 6))
    # the cut: -FLT_MAX, inf, NaN and an id outside the catalogue end a list (judged on the RAW score), a short count too
    A = lists_of([[5, 2, 7, 8]], [[9.0, 2.0, -FLT_MAX, 1.0]])
    B = lists_of([[7, 24, 1]], [[3.0, 2.0, 1.0]])
    ids, _, source, count = run(A, B, 6, a_div=[1e-30])
    assert sorted(ids[0, :3].tolist()) == [2, 5, 7] and count[0] == 3
    A = (A[0], A[1], np.array([1], np.int32))
    assert run(A, B, 6)[0][0, :2].tolist() == [5, 7]
    # NaN values are never listed: inf - inf in a normalisation
    A = lists_of([[5, 2]], [[3.0e38, -3.0e38]])
    ids, value, _, count = run(A, none, 4)
    assert not np.isnan(value[0, :count[0]]).any() and (ids[0, count[0]:] == -1).all()
    # keep larger than the union
    ids, value, source, count = run(one, one, 6)
    assert count[0] == 3 and (ids[0, 3:] == -1).all() and np.isneginf(value[0, 3:]).all() and (source[0, 3:] == 0).all()


# ---------------------------------------------------------------------------------------------- registration
NEW = {"factor_norms": ("rtrec_factor_norms", "factor_norms.hip", 7),
       "factor_similar_topk": ("rtrec_factor_similar_topk", "factor_similar.hip", 21),
       "similar_blend": ("rtrec_similar_blend", "similar_blend.hip", 23)}


def test_the_three_calls_are_declared_registered_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    from tests.test_diverse_host import ext_declared_symbols
    assert ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    assert len(ops.OPS) == 22                                                    # the core surface did not grow
    lib = ctypes.CDLL(build.LIB_PATH)
    for op, (symbol, source, n_args) in NEW.items():
        assert symbol in ext_declared_symbols() and symbol in _native.EXT_EXPORTS and symbol not in _native.EXPORTS
        assert op in ops.EXT_OPS and op not in ops.OPS and ops.EXT_EXPORT_OF[op] == symbol and source in build.SOURCES
        assert hasattr(lib, symbol) and len(getattr(_native.load(), symbol).argtypes) == n_args
        assert callable(getattr(HipBackend, op))
        for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):      # called through the op only, never by ctypes
            for f in files:
                if f.endswith(".py") and f != "_native.py":
                    assert f".{symbol}(" not in open(os.path.join(dirpath, f)).read(), f
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert all(t in header for t in ("FACTOR NORMS", "FACTOR SIMILAR TOP-K", "SIMILAR BLEND"))
    schema = {op: str(getattr(torch.ops.rtrec_amd, op).default._schema) for op in NEW}
    for op, mutated in (("factor_norms", ("out",)), ("factor_similar_topk", ("ids", "scores", "count")),
                        ("similar_blend", ("ids", "value", "source", "count"))):
        assert schema[op].startswith(f"rtrec_amd::{op}(") and schema[op].endswith("-> ()")
        for name in mutated:
            assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema[op]), schema[op]
    for name in ("div", "workspace"):
        assert re.search(rf"Tensor\([a-z]!\)\? {name}\b", schema["factor_similar_topk"])
    for name in ("queries", "p", "p_norms", "item_mask"):
        assert f"Tensor? {name}" in schema["factor_similar_topk"]
    assert "Tensor? a_div" in schema["similar_blend"] and "Tensor? exclude" in schema["similar_blend"]
    for name in ("similar_items_device", "item_norms_device", "similar_factor_device", "similar_blend_device", "similar_hybrid_device"):
        assert callable(getattr(SlimEngine, name))
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.factor_norms(torch.zeros(3, 4), 3, 4, 4, 1, torch.zeros(3))
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.factor_similar_topk(i32(2), None, None, torch.zeros(4, 5), 5, 4, torch.zeros(5), None, 3, 1, False,
                                                    i32(2, 3), torch.zeros(2, 3), i32(2), None, None)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.similar_blend(5, i32(2, 3), torch.zeros(2, 3), i32(2), 3, None, i32(2, 3), torch.zeros(2, 3), i32(2), 3, None,
                                              4, 0, i32(2, 4), torch.zeros(2, 4, dtype=torch.float64), i32(2, 4), i32(2))


# ---------------------------------------------------------------------------------------------- the API's refusals
def test_the_api_refuses_what_it_cannot_serve_without_touching_a_device():
    from tests.test_factor_host import fitted_model, seeded_factors
    m, batch = fitted_model()
    f = seeded_factors(batch)
    items = f["all_items"][:3]
    for call in (m.similar_items_factor_batch, m.similar_items_hybrid_batch):
        with pytest.raises(RuntimeError, match="attach_factors"):
            call(items)
        with pytest.raises(ValueError, match="attach_feature_factors"):                # no factor model at all
            call(items, query_items_tags=[["a"]] * 3)
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    for call in (m.similar_items_factor_batch, m.similar_items_hybrid_batch):
        for kw in (dict(top_k=0), dict(first_component=-1), dict(first_component=12)):
            with pytest.raises(ValueError):
                call(items, **kw)
        with pytest.raises(ValueError, match="attach_feature_factors"):                # finished vectors: a tag cannot change them
            call(items, query_items_tags=[["a"]] * 3)
        assert call([]) == []
    for kw in (dict(top_k=129), ):
        with pytest.raises(ValueError):
            m.similar_items_factor_batch(items, **kw)
    for kw in (dict(pool=0), dict(pool=129), dict(top_k=5, pool=200)):
        with pytest.raises(ValueError, match="128"):
            m.similar_items_hybrid_batch(items, **kw)
    # the whole of W on one rank: several ranks, a column-sharded W and a lossy W are refused before any device call
    m.recommend_batch([batch[0][0]])
    eng = m.model.engine
    dw = eng._W["dw"]
    eng.world_size = 2
    for call in (m.similar_items_hybrid_batch, m.similar_items_factor_batch):
        with pytest.raises(ValueError, match="gather_item_similarity"):
            call(items)
    dw.shard = (0, 1)
    with pytest.raises(ValueError, match="gather_item_similarity"):
        eng.similar_hybrid_device([0, 1])
    dw.shard, eng.world_size, dw.lossy = None, 1, True
    with pytest.raises(ValueError, match="float32"):
        eng.similar_hybrid_device([0, 1])
    dw.lossy = False
    for kw in (dict(top_k=0), dict(pool=0), dict(pool=129)):
        with pytest.raises(ValueError):
            eng.similar_hybrid_device([0, 1], **kw)
    # tags against tables: a string instead of a list, the wrong number of lists
    from tests.test_feature_repr_host import attach_tables, seeded_tables
    attach_tables(m, seeded_tables(batch))
    for call in (m.similar_items_factor_batch, m.similar_items_hybrid_batch):
        with pytest.raises(ValueError, match="LIST"):
            call(items, query_items_tags=["a", "b", "c"])
        with pytest.raises(ValueError, match="one list of tags per query item"):
            call(items, query_items_tags=[["a"]])
        for fc in (-1, 99):
            with pytest.raises(ValueError, match="first_component"):
                call(items, first_component=fc)


# ---------------------------------------------------------------------------------------------- the API check tests/test_gpu_similar.py runs
def host_hybrid(m, Q, has, first, queries, top_k, pool, vectors=None):
    """Host top-k -> host SLIM similar -> host blend over internal ids: (factor lists with cosines at top_k, the blend).
    Q [n_items, dim] the full-width item vectors (zero rows without one), `has` who has one, `queries` internal ids (-1:
    unknown), `vectors` [len(queries), dim] brought full-width query vectors or None."""
    import scipy.sparse as sp
    n_items = len(Q)
    T = np.ascontiguousarray(Q[:, first:])
    norms = host_norms_fast(T)
    kw = dict(mask=has.astype(np.uint8))
    if vectors is not None:
        kw.update(P=np.ascontiguousarray(vectors[:, first:]), p_norms=host_norms_fast(vectors[:, first:]))
    cosine = host_similar_fast(T, norms, queries, top_k, write_cosine=True, **kw)
    a_ids, a_s1, a_cnt, div = host_similar_fast(T, norms, queries, pool, **kw)
    W = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    W.sort_indices()
    rows = [host_slim_similar(W, q, pool) if 0 <= q < n_items else (np.zeros(0, np.int64), np.zeros(0, F32)) for q in queries]
    B = lists_of([r[0] for r in rows], [r[1] for r in rows], pool)
    return cosine, host_blend(n_items, (a_ids, a_s1, a_cnt), B, min(top_k, 2 * pool), a_div=div, exclude=np.asarray(queries, np.int32))


def _check_against_host(m, Q, has, first, raw_queries, top_k, pool, tags=None, vectors=None, first_arg=None):
    n_items = m.model.n_items_fitted
    qid = np.array([(-1 if m.item_ids.get_id(q) is None or m.item_ids.get_id(q) >= n_items else m.item_ids.get_id(q)) for q in raw_queries])
    cosine, blend = host_hybrid(m, Q, has, first, qid, top_k, pool, vectors)
    kw = dict(first_component=first_arg)
    if tags is not None:
        kw["query_items_tags"] = tags
    ids, sc, cnt = m.similar_items_factor_batch(raw_queries, top_k=top_k, as_arrays=True, **kw)
    assert ids.dtype == np.int64 and sc.dtype == np.float32 and ids.shape == sc.shape == (len(raw_queries), top_k)
    assert_same_lists((ids, sc, cnt), cosine, "factor")
    pairs = m.similar_items_factor_batch(raw_queries, top_k=top_k, **kw)
    for b in range(len(raw_queries)):
        assert pairs[b] == [(m.item_ids.get(int(i)), float(s)) for i, s in zip(ids[b, :cnt[b]], sc[b, :cnt[b]])]
        assert raw_queries[b] not in [i for i, _ in pairs[b]]
    got = m.similar_items_hybrid_batch(raw_queries, top_k=top_k, pool=pool, as_arrays=True, **kw)
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == (len(raw_queries), top_k)
    keep = min(top_k, 2 * pool)
    assert_same_blend([a[:, :keep] if a.ndim == 2 else a for a in got], blend, "hybrid")
    assert (got[0][:, keep:] == -1).all() and np.isneginf(got[1][:, keep:]).all() and (got[2][:, keep:] == 0).all()
    pairs = m.similar_items_hybrid_batch(raw_queries, top_k=top_k, pool=None if pool == top_k else pool, **kw)
    for b in range(len(raw_queries)):
        n = int(got[3][b])
        assert pairs[b] == [(m.item_ids.get(int(i)), float(v)) for i, v in zip(got[0][b, :n], got[1][b, :n])]
        assert all(isinstance(v, float) for _, v in pairs[b]) and raw_queries[b] not in [i for i, _ in pairs[b]]
    return qid, got


def check_similar_api(m, batch, strings=False):
    """The API checks shared with tests/test_gpu_similar.py (there `m` runs on the device): every item of the fixture as a
    query against host top-k -> host SLIM similar -> host blend, with finished vectors and with feature tables, with and
    without biases; query_items_tags; an unknown item; an item without a vector; pool > top_k; as_arrays."""
    from tests.test_factor_host import seeded_factors
    from tests.test_feature_repr_host import attach_tables, host_vectors, seeded_tables
    n_items = m.model.n_items_fitted
    # ---- finished vectors (attach_factors): stack_bias's [1, b, e...]; first_component None = 0, and 1 as a caller passes it
    f = seeded_factors(batch, strings=strings)
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    Q, has = np.zeros((n_items, f["Q"].shape[1]), F32), np.zeros(n_items, bool)
    for j, i in enumerate(f["items"]):
        if i in f["all_items"]:
            Q[m.item_ids.get_id(i)], has[m.item_ids.get_id(i)] = f["Q"][j], True
    unknown = "never heard of" if strings else 10 ** 9
    queries = f["all_items"][:50] + [unknown] + f["all_items"][50:]
    for first_arg, first, top_k, pool in ((None, 0, 10, 10), (1, 1, 7, 20), (1, 1, 128, 3)):
        qid, got = _check_against_host(m, Q, has, first, queries, top_k, pool, first_arg=first_arg)
        ids, value, source, cnt = got
        assert cnt[50] == 0 and m.similar_items_hybrid_batch([unknown]) == [[]] and m.similar_items_factor_batch([unknown]) == [[]]
        for raw in f["no_vec_items"]:                      # no vector: SLIM's list alone
            b = queries.index(raw)
            assert cnt[b] > 0 and (source[b, :cnt[b]] == 2).all()
            assert m.similar_items_factor_batch([raw]) == [[]]
        assert any((source[b, :cnt[b]] == 3).any() for b in range(len(queries))) and any((source[b, :cnt[b]] == 1).any() for b in range(len(queries)))
        for raw in f["no_vec_items"]:                      # ... and never listed by the factor side
            assert not ((ids == m.item_ids.get_id(raw)) & (source == 1)).any()
    assert m.similar_items_hybrid(queries[3], top_k=6, pool=9) == m.similar_items_hybrid_batch(queries, top_k=6, pool=9)[3]
    assert m.similar_items_factor(queries[3], top_k=6) == m.similar_items_factor_batch(queries, top_k=6)[3]
    before = m.similar_items_batch(queries[:5], top_k=5, ret_scores=True)
    # ---- feature tables (attach_feature_factors), with and without biases: first_component None = 1 / 0
    for bias in (True, False):
        t = seeded_tables(batch, strings=strings, bias=bias)
        for raw, tags in t["item_reg"]:
            m.register_item_feature(raw, tags)
        attach_tables(m, t)
        Qf, hf = host_vectors(m, t, "item", t["all_items"])
        Q, has = np.zeros((n_items, Qf.shape[1]), F32), np.zeros(n_items, bool)
        for j, i in enumerate(t["all_items"]):
            Q[m.item_ids.get_id(i)], has[m.item_ids.get_id(i)] = Qf[j], bool(hf[j])
        first = 1 if bias else 0
        queries = t["all_items"][:50] + [unknown] + t["all_items"][50:]
        qid, got = _check_against_host(m, Q, has, first, queries, 10, 10)
        assert got[3][50] == 0
        _check_against_host(m, Q, has, first, queries[40:60], 5, 12)
        # query_items_tags replace the registered tags; an unknown item with tags the table knows gets its tag-only vector
        qs = [t["all_items"][0], t["all_items"][1], unknown, unknown, t["all_items"][30], t["all_items"][7]]
        tags = [["comedy"], [], ["drama", "live"], ["nothing the table knows"], ["classic", "short"], None]
        entities = [q if q != unknown else None for q in qs]
        vec, vh = host_vectors(m, t, "item", entities, [tg or [] for tg in tags])
        vec = np.where(vh[:, None] != 0, vec, F32(0.0))
        qid, got = _check_against_host(m, Q, has, first, qs, 8, 8, tags=tags, vectors=vec)
        assert got[3][2] > 0 and (got[2][2, :got[3][2]] == 1).all()                 # unknown with known tags: the factor list alone
        assert got[3][3] == 0 and m.similar_items_hybrid(unknown, query_item_tags=["nothing the table knows"]) == []
        assert m.similar_items_hybrid(qs[0], top_k=8, query_item_tags=tags[0]) == m.similar_items_hybrid_batch(qs, top_k=8, query_items_tags=tags)[0]
        assert m.similar_items_hybrid(qs[0], top_k=8, query_item_tags=tags[0]) != m.similar_items_hybrid(qs[0], top_k=8)
    assert m.similar_items_batch(queries[:5], top_k=5, ret_scores=True) == before      # SLIM.similar_items did not change
    return queries


def check_serving_and_facade(m, item, queries):
    """POST /similar_items_hybrid and the Recommender pass-throughs against the model's own answers (tests/test_gpu_similar.py
    runs it on the device; `m` has feature tables attached)."""
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.recommender import Recommender
    from rtrec_amd.serving.app import ModelGate, build_router
    rec = Recommender(m)
    assert rec.similar_items_hybrid_batch(queries, top_k=6, pool=8) == m.similar_items_hybrid_batch(queries, top_k=6, pool=8)
    assert rec.similar_items_hybrid(item, top_k=6, query_item_tags=["drama"]) == m.similar_items_hybrid(item, top_k=6, query_item_tags=["drama"])
    assert rec.similar_items_factor_batch(queries, top_k=6, first_component=0) == m.similar_items_factor_batch(queries, top_k=6, first_component=0)
    assert rec.similar_items_factor(item) == m.similar_items_factor(item)
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    want = m.similar_items_hybrid_batch([item], top_k=6, pool=20)[0]
    r = client.post("/similar_items_hybrid", json={"item": item, "top_k": 6, "pool": 20}, headers=ok)
    assert r.status_code == 200 and len(want) == 6 and r.json() == {"item": item, "items": [{"item": i, "score": v} for i, v in want]}
    r = client.post("/similar_items_hybrid", json={"item": item, "item_tags": ["drama", "short"], "first_component": 0}, headers=ok)
    want = m.similar_items_hybrid_batch([item], query_items_tags=[["drama", "short"]], first_component=0)[0]
    assert r.status_code == 200 and r.json()["items"] == [{"item": i, "score": v} for i, v in want]
    assert client.post("/similar_items_hybrid", json={"item": item, "pool": 500}, headers=ok).status_code == 500


def test_the_serving_route_and_the_facade_without_a_device():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    import rtrec_amd.serving.app as app_mod
    from rtrec_amd.recommender import Recommender
    from tests.test_factor_host import fitted_model
    assert "POST /similar_items_hybrid" in app_mod.__doc__
    m, batch = fitted_model()
    rec, item = Recommender(m), batch[0][1]
    for call in (rec.similar_items_hybrid, rec.similar_items_factor):
        with pytest.raises(RuntimeError, match="attach_factors"):
            call(item)
    with pytest.raises(ValueError):
        rec.similar_items_hybrid_batch([item], pool=0)
    with pytest.raises(ValueError):
        rec.similar_items_factor_batch([item], top_k=129)
    app = FastAPI()
    app.include_router(app_mod.build_router(app_mod.ModelGate(m)))
    client = TestClient(app)
    r = client.post("/similar_items_hybrid", json={"item": item}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/similar_items_hybrid", json={"item": item}, headers={"X-Token": "fake_secret_token"})   # no vectors: the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Similar items hybrid failed"}
    assert client.post("/similar_items_hybrid", json={"top_k": 4}, headers={"X-Token": "fake_secret_token"}).status_code == 422
