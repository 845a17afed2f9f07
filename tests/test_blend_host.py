"""Blended lists (SLIM.recommend_blended_batch / blend_batch, csrc/blend.hip) without a GPU: the definition as a plain-Python host
model and a vectorised one, both pinned to the reference's own HybridSlimFM._ensemble_by_scores on the golden fixture
(tests/golden/blend.json, written by tools/gen_golden_blend.py); hand-written cases for every rule; the model / facade / serving
layers end to end through the CPU stand-in backend with `blend_lists` supplied by the host model; the rules of the extension
surface and the C entry point's host-side checks.  The kernel is in tests/test_gpu_blend.py.

The definition (include/rtrec_amd_ext.h, "BLENDED LISTS"), with A the other scorer's list and B SLIM's: a list is cut at its
first position behind its count, with an id outside [0, n_items) or a score that is not finite or <= -FLT_MAX; each list is
min-max normalised in float32, norm = fl(fl(s - mn) / fl(fl(mx - mn) + 1e-8f)); the union holds A's distinct ids by first appearance
(with the normalised score of their LAST appearance), then the ids only B holds; every B position adds fl(w * normB) to its item's
entry in ascending position; w is a constant or (float32)((2.0 * n) / (n + k)) with n the user's contacts with the item; with mnz
an entry of both lists doubles; entries are ranked by value, the earlier entry first among == values, NaN never."""
import json
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.engine import SlimEngine
from tests.test_explain_host import bits
from tests.test_quality_host import QualityOracleBackend
from tests.test_rerank_host import _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
EPS = F32(1e-8)
MAX_LIST = SlimEngine.BLEND_MAX_LIST     # positions either list may hold (1024: the kernel's LDS arrays)


# ---------------------------------------------------------------------------------------------- the host models
def contact_weight(n, k):
    """(float32)((2.0 * n) / (n + k)) in float64; n <= 0 gives +0."""
    return F32(0.0) if n <= 0 else F32((2.0 * float(n)) / (float(n) + float(k)))


def _rows_of(contacts, B):
    rows = contacts.get("rows")
    return np.arange(B, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)


def host_model(n_items, A, B, keep, weight_b=1.0, contacts=None, k=2.0, mnz=False, ties=None):
    """THE DEFINITION, written the way the reference writes it (a dict per row, a stable sort): (ids[R, keep] int32,
    value[R, keep] float32, source[R, keep] int32, count[R] int32).  A and B are (ids[R, ka], scores[R, ka], counts[R]).
    `contacts` None: every B position weighs float32(weight_b); else a dict with "X" (csr over the catalogue: which items a row
    stores), "C" (csr of int counts, or None) and "rows" (the row of X / C per list row, None: row r).  `ties` (a list)
    collects the rows whose listed entries -- and the first one left out -- hold two == values next to each other."""
    R = len(A[0])
    ids = np.full((R, keep), -1, np.int32)
    value = np.full((R, keep), -np.inf, F32)
    source = np.zeros((R, keep), np.int32)
    count = np.zeros(R, np.int32)
    rows = _rows_of(contacts, R) if contacts is not None else None

    def cut(lst, r):
        li, ls, lc = np.asarray(lst[0])[r], np.asarray(lst[1], dtype=F32)[r], int(np.asarray(lst[2])[r])
        out_i, out_s = [], []
        for p in range(min(max(lc, 0), len(li))):
            if not 0 <= li[p] < n_items or not np.isfinite(ls[p]) or ls[p] <= -FLT_MAX:
                break
            out_i.append(int(li[p])); out_s.append(F32(ls[p]))
        return out_i, out_s

    def normalise(s):
        mn, mx = min(s), max(s)
        den = F32(F32(mx - mn) + EPS)
        return [F32(F32(v - mn) / den) for v in s]

    def weight(r, item):
        if contacts is None:
            return F32(weight_b)
        u = int(rows[r])
        X, C = contacts["X"], contacts.get("C")
        if not 0 <= u < X.shape[0]:
            return F32(0.0)
        n = None
        if C is not None:
            lo, hi = C.indptr[u], C.indptr[u + 1]
            hit = np.flatnonzero(C.indices[lo:hi] == item)
            if hit.size:
                n = int(C.data[lo + hit[0]])
        if n is None:
            n = 1 if item in X.indices[X.indptr[u]:X.indptr[u + 1]] else 0
        return contact_weight(n, k)

    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for r in range(R):
            ai, as_ = cut(A, r)
            bi, bs = cut(B, r)
            combined = {}
            if ai:
                combined = dict(zip(ai, normalise(as_)))                 # the first position, the LAST value
            if bi:
                nb = normalise(bs)
                for q, item in enumerate(bi):
                    term = F32(weight(r, item) * nb[q])
                    combined[item] = F32(combined.get(item, F32(0.0)) + term)
            in_a, in_b = set(ai), set(bi)
            if mnz:
                combined = {i: (F32(v * F32(2.0)) if i in in_a and i in in_b else v) for i, v in combined.items()}
            ranked = sorted(((i, v) for i, v in combined.items() if not np.isnan(v)), key=lambda x: x[1], reverse=True)
            if ties is not None and any(ranked[t][1] == ranked[t + 1][1] for t in range(min(keep, len(ranked) - 1))):
                ties.append(r)
            ranked = ranked[:keep]
            for t, (i, v) in enumerate(ranked):
                ids[r, t], value[r, t], source[r, t] = i, v, (1 if i in in_a else 0) + (2 if i in in_b else 0)
            count[r] = len(ranked)
    return ids, value, source, count


def host_model_vectorised(n_items, A, B, keep, weight_b=1.0, contacts=None, k=2.0, mnz=False, chunk=None):
    """The same function with numpy over rows and positions (the B terms are added in a loop over q, all rows at once): what the
    larger GPU cases and tools/blend_bench.py compare against."""
    a_ids, a_sc, a_cnt = np.asarray(A[0]), np.asarray(A[1], dtype=F32), np.asarray(A[2])
    b_ids, b_sc, b_cnt = np.asarray(B[0]), np.asarray(B[1], dtype=F32), np.asarray(B[2])
    R, ka, kb = a_ids.shape[0], a_ids.shape[1], b_ids.shape[1]
    K = ka + kb
    if chunk is None:
        chunk = max(1, (1 << 24) // (K * K))
    if R > chunk:
        parts = []
        for s in range(0, R, chunk):
            sub = None if contacts is None else dict(contacts, rows=_rows_of(contacts, R)[s:s + chunk])
            parts.append(host_model_vectorised(n_items, (a_ids[s:s + chunk], a_sc[s:s + chunk], a_cnt[s:s + chunk]),
                                               (b_ids[s:s + chunk], b_sc[s:s + chunk], b_cnt[s:s + chunk]), keep, weight_b, sub, k, mnz, chunk))
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(4))

    def effective(ids, sc, cnt):
        ok = (np.arange(ids.shape[1])[None, :] < cnt[:, None]) & (ids >= 0) & (ids < n_items) & np.isfinite(sc) & (sc > -FLT_MAX)
        return np.cumprod(ok, axis=1).astype(bool)

    def normalise(sc, eff):
        mn = np.where(eff, sc, np.inf).min(axis=1, initial=np.inf).astype(F32)
        mx = np.where(eff, sc, -np.inf).max(axis=1, initial=-np.inf).astype(F32)
        den = ((mx - mn).astype(F32) + EPS).astype(F32)
        return ((sc - mn[:, None]).astype(F32) / den[:, None]).astype(F32)

    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        ea, eb = effective(a_ids, a_sc, a_cnt), effective(b_ids, b_sc, b_cnt)
        na_, nb_ = normalise(a_sc, ea), normalise(b_sc, eb)
        eff = np.concatenate([ea, eb], axis=1)
        ids_all = np.where(eff, np.concatenate([a_ids, b_ids], axis=1), -1).astype(np.int64)
        eq = (ids_all[:, :, None] == ids_all[:, None, :]) & eff[:, :, None] & eff[:, None, :]        # [R, K, K]
        owner = eq.argmax(axis=2)                                            # the first position that holds the id (e itself at least)
        entry = eff & (owner == np.arange(K)[None, :])
        last_a = (ka - 1) - eq[:, :, :ka][:, :, ::-1].argmax(axis=2) if ka else np.zeros((R, K), np.int64)
        in_a, in_b = eq[:, :, :ka].any(axis=2), eq[:, :, ka:].any(axis=2)
        val = np.zeros((R, K), F32)                                          # by e: A's positions, then B's
        val[:, :ka] = np.where(entry[:, :ka], np.take_along_axis(na_, last_a[:, :ka], axis=1), F32(0.0))
        # the weight per B position
        if contacts is None:
            w = np.full((R, kb), F32(weight_b), F32)
        else:
            rows = _rows_of(contacts, R)
            X, C = contacts["X"], contacts.get("C")
            U = X.shape[0]
            in_x = (rows >= 0) & (rows < U)
            key = np.where(in_x, rows, 0)[:, None] * n_items + np.where(eb, b_ids, 0).astype(np.int64)

            def stored(M):
                mkey = np.repeat(np.arange(U, dtype=np.int64), np.diff(M.indptr)) * n_items + M.indices
                if len(mkey) == 0:
                    return np.zeros(key.shape, np.int64), np.zeros(key.shape, bool)
                pos = np.minimum(np.searchsorted(mkey, key), len(mkey) - 1)      # (left: the first of equal columns)
                return pos, mkey[pos] == key

            n = stored(X)[1].astype(np.int64)
            if C is not None:
                pos, hit = stored(C)
                n = np.where(hit, np.asarray(C.data)[pos] if C.nnz else 0, n)
            n = np.where(in_x[:, None] & eb, n, 0)
            w = np.where(n > 0, ((2.0 * n) / (np.maximum(n, 1) + float(k))), 0.0).astype(F32)
        rr = np.arange(R)
        for q in range(kb):
            live = eb[:, q]
            if not live.any():
                continue
            o = owner[:, ka + q]
            term = (w[:, q] * nb_[:, q]).astype(F32)
            val[rr[live], o[live]] = (val[rr[live], o[live]] + term[live]).astype(F32)
        both = in_a & in_b
        if mnz:
            val = np.where(entry & both, (val * F32(2.0)).astype(F32), val)
        listed = entry & ~np.isnan(val)
        order = np.argsort(np.where(listed, -val, np.inf), axis=1, kind="stable")[:, :keep]
        n_listed = listed.sum(axis=1)
        count = np.minimum(n_listed, keep).astype(np.int32)
        if order.shape[1] < keep:
            order = np.concatenate([order, np.zeros((R, keep - order.shape[1]), np.int64)], axis=1)
        live = np.arange(keep)[None, :] < count[:, None]
        ids = np.where(live, np.take_along_axis(ids_all, order, axis=1), -1).astype(np.int32)
        value = np.where(live, np.take_along_axis(val, order, axis=1), -np.inf).astype(F32)
        src = (in_a.astype(np.int32) + 2 * in_b.astype(np.int32))
        source = np.where(live, np.take_along_axis(src, order, axis=1), 0).astype(np.int32)
    return ids, value, source, count


def value_bits(v):
    """The bits of a value after adding +0.0f: the sign of a zero is not part of the contract."""
    return bits(np.asarray(v, dtype=F32) + F32(0.0))


def assert_same(got, want, what=""):
    for name, g, w in zip(("ids", "value", "source", "count"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the host model {w.shape}"
        bad = np.flatnonzero((value_bits(g) != value_bits(w)).ravel() if name == "value" else (g != w).ravel())
        assert bad.size == 0, f"{what}: {bad.size} {name} differ from the host model, first at flat index {int(bad[0])}: {g.ravel()[bad[0]]} != {w.ravel()[bad[0]]}"


def pad_lists(lists, width=None, fill=-1, dtype=np.int32):
    """[R, width] array of the ragged `lists`, `fill` behind each, and their lengths."""
    width = max([len(r) for r in lists] + [1]) if width is None else width
    out = np.full((len(lists), width), fill, dtype)
    for r, row in enumerate(lists):
        out[r, :len(row)] = row
    return out, np.array([len(r) for r in lists], np.int32)


def csr_of_rows(rows, n_cols, values=None):
    """A CSR with sorted columns from one list of columns per row (and a dict column -> value per row for `values`)."""
    ptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    cols = np.array([c for r in rows for c in sorted(r)], np.int32)
    data = np.ones(len(cols), np.int32) if values is None else np.array([values[i][c] for i, r in enumerate(rows) for c in sorted(r)], np.int32)
    return sp.csr_matrix((data, cols, ptr), shape=(len(rows), n_cols))


_FIXTURE = {}


def fixture():
    """tests/golden/blend.json as arrays, once: dict(n_items, A, B, X, C, k[R], want[R] (the reference's ids, the whole union),
    users (the first 240 rows), small (the rest), meta)."""
    if not _FIXTURE:
        z = json.load(open(os.path.join(G, "blend.json")))
        cases = z["cases"]
        a_ids, a_cnt = pad_lists([c["a_ids"] for c in cases])
        b_ids, b_cnt = pad_lists([c["b_ids"] for c in cases])
        a_sc, _ = pad_lists([c["a_scores"] for c in cases], a_ids.shape[1], 0.0, F32)
        b_sc, _ = pad_lists([c["b_scores"] for c in cases], b_ids.shape[1], 0.0, F32)
        n_items = z["n_items"]
        X = csr_of_rows([c["x_items"] for c in cases], n_items)
        counted = [{int(i): n for i, n in c["counts"]} for c in cases]
        C = csr_of_rows([list(d) for d in counted], n_items, counted)
        for a in (a_ids, a_cnt, b_ids, b_cnt, a_sc, b_sc):
            a.setflags(write=False)
        _FIXTURE.update(n_items=n_items, A=(a_ids, a_sc, a_cnt), B=(b_ids, b_sc, b_cnt), X=X, C=C, k=np.array([c["k"] for c in cases]),
                        want=[c["ids"] for c in cases], n_users=z["n_users"], meta=z)
    return _FIXTURE


def fixture_by_k(model, keep, **kw):
    """`model` over the whole fixture, the rows of each k in one call: (ids, value, source, count) in fixture order."""
    f = fixture()
    R = len(f["k"])
    out = (np.full((R, keep), -1, np.int32), np.full((R, keep), -np.inf, F32), np.zeros((R, keep), np.int32), np.zeros(R, np.int32))
    for k in np.unique(f["k"]):
        sel = np.flatnonzero(f["k"] == k)
        got = model(f["n_items"], tuple(a[sel] for a in f["A"]), tuple(b[sel] for b in f["B"]), keep,
                    contacts=dict(X=f["X"], C=f["C"], rows=sel), k=float(k), **kw)
        for dst, src in zip(out, got):
            dst[sel] = src
    return out


class BlendOracleBackend(QualityOracleBackend):
    """The CPU stand-in (tests.cpu_backend.OracleBackend with the request calls of the earlier host models) plus blend_lists
    from the host model (TEST-ONLY, like its bases)."""

    def blend_lists(self, n_items, a_ids, a_scores, a_counts, ka, b_ids, b_scores, b_counts, kb, keep, weight_b, contacts, k, mnz,
                    row_ids, xb, cn, out_ids, value, source, count, waves_per_row=0):
        import torch
        con = None
        if contacts:
            ptr, col = xb[0].numpy(), xb[1].numpy()
            X = sp.csr_matrix((np.ones(len(col), np.int32), col, ptr), shape=(len(ptr) - 1, n_items))
            C = None if cn is None else sp.csr_matrix((cn[2].numpy(), cn[1].numpy(), cn[0].numpy()), shape=(len(ptr) - 1, n_items))
            con = dict(X=X, C=C, rows=None if row_ids is None else row_ids.numpy())
        out = host_model_vectorised(n_items, (a_ids.numpy()[:, :ka], a_scores.numpy()[:, :ka], a_counts.numpy()),
                                    (b_ids.numpy()[:, :kb], b_scores.numpy()[:, :kb], b_counts.numpy()), keep, weight_b, con, k, mnz)
        for dst, src in zip((out_ids, value, source, count), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=BlendOracleBackend())
    return m


def _model(strings=False):
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


def random_lists(rng, R, ka, kb, n_items, id_hi=None):
    """Seeded lists with everything that can go wrong: ids drawn with replacement from a small range (duplicates inside and
    across the lists), invalid ids and scores at seeded places, counts from -2 to beyond the width."""
    id_hi = n_items if id_hi is None else id_hi
    out = []
    for k_ in (ka, kb):
        ids = rng.integers(0, id_hi, (R, k_)).astype(np.int32)
        sc = -np.sort(-rng.standard_normal((R, k_)).astype(F32), axis=1)
        bad = rng.random((R, k_)) < 0.02
        ids[bad] = rng.choice([-1, n_items, n_items + 5], int(bad.sum()))
        worse = rng.random((R, k_)) < 0.02
        sc[worse] = rng.choice([np.nan, np.inf, -np.inf, -FLT_MAX], int(worse.sum())).astype(F32)
        cnt = rng.integers(-2, k_ + 3, R).astype(np.int32)
        cnt[rng.random(R) < 0.5] = k_
        out.append((ids, sc, cnt))
    return out[0], out[1]


def random_contacts(rng, R, n_rows_x, n_items, with_counts=True):
    """dict(X, C, rows) over `n_rows_x` rows of X: about a third of the items stored per row, counts 0..6 on half of those and
    on a few items the row does not store; list row r -> a seeded row, some outside X."""
    xs, cs = [], []
    for _ in range(n_rows_x):
        own = np.flatnonzero(rng.random(n_items) < 0.3)
        xs.append(own.tolist())
        counted = {int(i): int(rng.integers(0, 7)) for i in own if rng.random() < 0.5}
        counted.update({int(i): int(rng.integers(1, 4)) for i in rng.integers(0, n_items, 2)})
        cs.append(counted)
    rows = rng.integers(-1, n_rows_x + 1, R)
    return dict(X=csr_of_rows(xs, n_items), C=csr_of_rows([list(d) for d in cs], n_items, cs) if with_counts else None, rows=rows)


# ---------------------------------------------------------------------------------------------- the definition
def test_both_models_reproduce_the_reference_on_every_fixture_case():
    f = fixture()
    assert f["meta"]["numpy_version"].split(".")[0] == "2", "the fixture's float32 arithmetic is numpy 2's (NEP 50)"
    R, U = len(f["want"]), f["n_users"]
    assert U == 240 and R == 300
    keep = f["A"][0].shape[1] + f["B"][0].shape[1]
    plain = fixture_by_k(host_model, keep)
    fast = fixture_by_k(host_model_vectorised, keep)
    assert_same(fast, plain, "fixture")
    for r in range(R):
        assert plain[0][r, :plain[3][r]].tolist() == f["want"][r], f"case {r}: the host model's order is not the reference's"
        assert fast[0][r, :fast[3][r]].tolist() == f["want"][r]
    # the recorded conditions hold, and are what the host model finds
    top = fixture_by_k(host_model, 10)
    a_ids = f["A"][0]
    differs = sum(top[0][r].tolist() != a_ids[r, :10].tolist() for r in range(U))
    b_only = int((top[2][:U] == 2).any(axis=1).sum())
    ties = 0
    for r in range(U):
        v = plain[1][r, :plain[3][r]]
        ties += bool((v[1:] == v[:-1]).any())
    cond = f["meta"]["conditions"]
    assert (differs, ties, b_only) == (cond["order_differs_from_a"], cond["tie_decided_by_position"], cond["lists_an_item_only_b_holds"])
    assert differs >= 100 and ties >= 100 and b_only >= 50
    small = range(U, R)
    assert f["meta"]["small_cases_with_repeated_ids"] >= 30 and {1, 12} <= {int(f["A"][2][r]) for r in small} | {int(f["B"][2][r]) for r in small}
    assert set(f["k"].tolist()) == {2.0, 0.5}


@pytest.mark.parametrize("mode", ["constant", "contacts", "membership", "mnz"])
def test_vectorised_model_is_the_definition_on_mutilated_lists(mode):
    rng = np.random.default_rng({"constant": 1, "contacts": 2, "membership": 3, "mnz": 4}[mode])
    n_items = 40
    for ka, kb, keep in ((1, 1, 2), (7, 12, 5), (12, 7, 19), (30, 30, 60)):
        A, B = random_lists(rng, 60, ka, kb, n_items, id_hi=16)
        kw = dict(weight_b=0.75) if mode == "constant" else dict(weight_b=1.5, mnz=True) if mode == "mnz" else \
            dict(contacts=random_contacts(rng, 60, 9, n_items, with_counts=mode == "contacts"), k=0.5 if ka == 7 else 2.0)
        want = host_model(n_items, A, B, keep, **kw)
        assert_same(host_model_vectorised(n_items, A, B, keep, **kw), want, f"{mode} ka={ka} kb={kb}")
        assert_same(host_model_vectorised(n_items, A, B, keep, chunk=7, **kw), want, f"{mode} ka={ka} kb={kb} in chunks")
        if ka == 30:
            assert want[3].min() < want[3].max() and {1, 2, 3} <= set(np.unique(want[2]).tolist())


def _one(a_ids, a_sc, b_ids, b_sc, keep, n_items=8, a_cnt=None, b_cnt=None, **kw):
    A = (np.array([a_ids], np.int32), np.array([a_sc], F32), [len(a_ids) if a_cnt is None else a_cnt])
    B = (np.array([b_ids], np.int32), np.array([b_sc], F32), [len(b_ids) if b_cnt is None else b_cnt])
    outs = [model(n_items, A, B, keep, **kw) for model in (host_model, host_model_vectorised)]
    assert_same(outs[1], outs[0], "hand-written")
    ids, value, source, count = outs[0]
    n = int(count[0])
    assert (ids[0, n:] == -1).all() and np.isneginf(value[0, n:]).all() and (source[0, n:] == 0).all()
    return ids[0, :n].tolist(), value[0, :n], source[0, :n].tolist()


def norm_of(s):
    s = np.asarray(s, F32)
    return ((s - s.min()).astype(F32) / F32(F32(s.max() - s.min()) + EPS)).astype(F32)


def test_hand_written_cases_cover_each_rule():
    half = norm_of([3, 2, 1])[1]
    # normalisation: the minimum is 0, the maximum fl(2 / fl(2 + 1e-8)) = 1; an all-equal list is all zeros and keeps A's order
    ids, v, src = _one([1, 2, 3], [3, 2, 1], [0], [0.0], 4, b_cnt=0)
    assert ids == [1, 2, 3] and src == [1, 1, 1] and np.array_equal(bits(v), bits([1.0, half, 0.0])) and half == F32(0.5)
    ids, v, src = _one([3, 4, 1], [2, 2, 2], [0], [0.0], 3, b_cnt=0)
    assert ids == [3, 4, 1] and not v.any()
    # an id repeated inside A stands at its FIRST position with the value of its LAST one
    ids, v, src = _one([1, 2, 1], [3, 2, 1], [0], [0.0], 3, b_cnt=0)
    assert ids == [2, 1] and np.array_equal(bits(v), bits([half, 0.0]))
    # an id repeated inside B adds once per occurrence; the items only B holds follow A's, in B's order
    ids, v, src = _one([1], [1.0], [5, 6, 5], [3, 2, 1], 3, weight_b=1.0)
    assert ids == [5, 6, 1] and src == [2, 2, 1] and np.array_equal(bits(v), bits([F32(F32(1.0) + F32(0.0)), half, 0.0]))
    ids, v, src = _one([1], [1.0], [5, 6, 5], [3, 2, 1], 3, weight_b=0.0)
    assert ids == [1, 5, 6] and not v.any()                              # every value 0: the union's own order decides
    # separate roundings: fl(w * norm) then fl(value + term)
    w, nb = F32(0.3), norm_of([7, 3, 1])
    ids, v, src = _one([4, 2], [5, 1], [2, 4, 3], [7, 3, 1], 3, weight_b=0.3)
    assert ids == [4, 2, 3] and src == [3, 3, 2]
    assert np.array_equal(bits(v), bits([F32(F32(1.0) + F32(w * nb[1])), F32(F32(0.0) + F32(w * nb[0])), F32(w * nb[2])]))
    # mnz doubles what stands in both lists, once, at the end
    ids2, v2, _ = _one([4, 2], [5, 1], [2, 4, 3], [7, 3, 1], 3, weight_b=0.3, mnz=True)
    assert ids2 == [4, 2, 3] and np.array_equal(bits(v2), bits([v[0] * 2, v[1] * 2, v[2]]))
    # contacts: a stored count wins over membership (a stored 0 too), membership is one contact, anything else none
    X = csr_of_rows([[1, 2, 3]], 8)
    C = csr_of_rows([[2, 3, 5]], 8, [{2: 4, 3: 0, 5: 2}])
    for k in (2.0, 0.5):
        ids, v, src = _one([0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], 6, contacts=dict(X=X, C=C, rows=None), k=k)
        one = F32(F32(4.0) / F32(F32(4.0) + EPS))
        want = {1: F32(contact_weight(1, k) * one), 2: F32(contact_weight(4, k) * one), 3: F32(0.0), 5: F32(contact_weight(2, k) * one), 6: F32(0.0), 0: F32(0.0)}
        assert sorted(ids) == [0, 1, 2, 3, 5, 6] and all(bits(x) == bits(want[i]) for i, x in zip(ids, v))
        assert ids == ([2, 5, 1, 0, 3, 6] if k == 2.0 else [2, 5, 1, 0, 3, 6])
        assert contact_weight(1, 2.0) == F32(2.0 / 3.0) and contact_weight(4, 2.0) == F32(8.0 / 6.0) and contact_weight(1, 0.5) == F32(2.0 / 1.5)
        no_counts = _one([0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], 6, contacts=dict(X=X, C=None, rows=None), k=k)
        assert no_counts[0] == [1, 2, 3, 0, 5, 6]                        # membership only: 1, 2, 3 weigh the same, 5 and 6 nothing
        outside = _one([0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], 6, contacts=dict(X=X, C=C, rows=[7]), k=k)
        assert outside[0] == [0, 1, 2, 3, 5, 6] and not outside[1].any()  # a row outside X has no contacts
    # a list is cut at its first invalid position: its count, a foreign id, a score that is NaN, infinite or <= -FLT_MAX
    for bad_id, bad_sc in ((8, 1.0), (-1, 1.0), (2, np.nan), (2, np.inf), (2, -np.inf), (2, -FLT_MAX)):
        ids, v, src = _one([1, bad_id, 3], [3, bad_sc, 0.5], [5], [1.0], 4, weight_b=1.0)
        assert ids == [1, 5] and not v.any()                             # (one position left on each side: both normalise to 0)
    ids, v, src = _one([1, 2, 3], [3, 2, 1], [5, 6], [2, 1], 5, a_cnt=2, b_cnt=0)
    assert ids == [1, 2] and np.array_equal(bits(v), bits([F32(F32(1.0) / F32(F32(1.0) + EPS)), 0.0]))
    ids, v, src = _one([1, 2], [3, np.nextafter(-FLT_MAX, F32(0))], [5], [1.0], 3, b_cnt=0)
    assert ids == [1, 2]                                                 # just above the cut: kept
    # two empty lists; keep beyond the union
    assert _one([9], [1.0], [9], [1.0], 2)[0] == []
    # equal values: the earlier entry of the union wins, -0.0 == +0.0
    ids, v, src = _one([1, 2], [-0.0, 0.0], [3], [1.0], 3, weight_b=0.0)
    assert ids == [1, 2, 3]
    # one denormal apart: the difference is not flushed, the division is correctly rounded
    d = np.float32(1e-45)
    ids, v, src = _one([1, 2], [2 * d, d], [0], [0.0], 2, b_cnt=0)
    assert ids == [1, 2] and v[0] > 0 and bits(v[0]) == bits(F32(d / F32(d + EPS))) and v[1] == 0
    # a range that overflows: the maximum's value is inf / inf = NaN and is never listed
    ids, v, src = _one([1, 2, 3], [3e38, 0.0, -3e38], [0], [0.0], 3, b_cnt=0)
    assert ids == [2, 3] and not v.any()


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _expected(m, users, others, other_scores, top_k, pool, contact_counts=None, k=2.0, weighting="contacts", mnz=False,
              filter_interacted=True):
    """recommend_blended_batch from its parts: recommend_batch's list, score_pairs' scores, the plain host model."""
    n_items = m.model.n_items_fitted
    X = sp.csr_matrix(m.interactions.to_csr())
    X.sort_indices()
    out = []
    for u, items, sc in zip(users, others, other_scores):
        row = m._known_user_id(u) if not isinstance(u, float) else None
        own = m.recommend_batch([u], top_k=pool, filter_interacted=filter_interacted)[0] if row is not None else []
        own_sc = m.score_pairs([u] * len(own), own) if own else np.zeros(0, F32)
        known = [(m.item_ids.get_id(i), s) for i, s in zip(items, sc) if _known(m, i)]
        A = pad_lists([[i for i, _ in known]])[0], pad_lists([[s for _, s in known]], None, 0.0, F32)[0], [len(known)]
        B = pad_lists([[m.item_ids.get_id(i) for i in own]])[0], pad_lists([list(own_sc)], None, 0.0, F32)[0], [len(own)]
        kw = dict(weight_b=weighting) if weighting != "contacts" else None
        if kw is None:
            cnt = {}
            for cu, ci, n in (contact_counts or []):
                if cu == u and _known(m, ci):
                    cnt[m.item_ids.get_id(ci)] = int(n)
            C = sp.csr_matrix((X.shape[0], n_items), dtype=np.int32).tolil()
            kw = dict(contacts=dict(X=sp.csr_matrix((np.ones(X.nnz, np.int32), X.indices, X.indptr), shape=(X.shape[0], n_items)),
                                    C=csr_of_rows([list(cnt) if r == row else [] for r in range(X.shape[0])], n_items,
                                                  [cnt if r == row else {} for r in range(X.shape[0])]) if contact_counts is not None else None,
                                    rows=[-1 if row is None else row]), k=k)
        ids, value, source, count = host_model(n_items, A, B, min(top_k, A[0].shape[1] + B[0].shape[1]), mnz=mnz, **kw)
        out.append(([m.item_ids.get(int(i)) for i in ids[0, :count[0]]], value[0, :count[0]], source[0, :count[0]].tolist()))
    return out


def _known(m, item):
    try:
        return m.item_ids.get_id(item) is not None and 0 <= m.item_ids.get_id(item) < m.model.n_items_fitted
    except (ValueError, TypeError, KeyError):
        return False


@pytest.mark.parametrize("strings", [False, True])
def test_recommend_blended_batch_end_to_end(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = _model(strings)
    rng = np.random.default_rng(8)
    known_users = sorted({u for u, _, _, _ in batch}, key=str)
    known_items = sorted({i for _, i, _, _ in batch}, key=str)
    cold = "nobody" if strings else max(known_users) + 1000
    unknown = "never seen" if strings else 10 ** 7
    users = known_users[:20] + [cold, known_users[3]]
    plain = m.recommend_batch(users, top_k=8)
    others, other_scores = [], []
    for b, u in enumerate(users):
        mine = plain[b][:4] if plain[b] else []
        row = list(mine) + [known_items[j] for j in rng.permutation(len(known_items))[:6]] + [unknown]
        row = [row[j] for j in rng.permutation(len(row))]
        others.append(row)
        other_scores.append((-np.sort(-rng.random(len(row)))).astype(F32).tolist())
    seen = {}
    for u, i, _, _ in batch:
        seen.setdefault(u, []).append(i)
    counts = [(u, plain[b][j], int(rng.integers(1, 5))) for b, u in enumerate(users[:20]) for j in range(0, len(plain[b]), 2)]
    counts += [(cold, known_items[0], 3), (known_users[0], unknown, 2), (known_users[1], seen[known_users[1]][0], 3)]
    for kw in (dict(top_k=8), dict(top_k=8, contact_counts=counts), dict(top_k=5, pool=12, contact_counts=counts, similarity_weight_factor=0.5),
               dict(top_k=8, weighting=0.6), dict(top_k=8, weighting=1.0, mnz=True), dict(top_k=6, contact_counts=counts, filter_interacted=False),
               dict(top_k=40, pool=9, weighting=2.0)):
        got = m.recommend_blended_batch(users, others, other_scores, **kw)
        arrays = m.recommend_blended_batch(users, others, other_scores, as_arrays=True, **kw)
        want = _expected(m, users, others, other_scores, kw["top_k"], kw.get("pool", kw["top_k"]), kw.get("contact_counts"),
                         kw.get("similarity_weight_factor", 2.0), kw.get("weighting", "contacts"), kw.get("mnz", False),
                         kw.get("filter_interacted", True))
        assert got == [w[0] for w in want], kw
        ids, value, source, cnt = arrays
        assert ids.shape == value.shape == source.shape == (len(users), kw["top_k"]) and ids.dtype == np.int64
        for b, (w_ids, w_val, w_src) in enumerate(want):
            n = int(cnt[b])
            assert n == len(w_ids) and [m.item_ids.get(int(i)) for i in ids[b, :n]] == w_ids and source[b, :n].tolist() == w_src
            assert np.array_equal(value_bits(value[b, :n]), value_bits(w_val))
            assert (ids[b, n:] == -1).all() and np.isneginf(value[b, n:]).all() and (source[b, n:] == 0).all()
            assert unknown not in got[b]
        assert all(s == 1 for s in want[20][2]) and got[20] == [i for i in others[20] if i != unknown][:kw["top_k"]] or kw["top_k"] < 8
    # contacts without counts and with the filter: SLIM's items weigh nothing, so only the other scorer's items have a value
    base = m.recommend_blended_batch(users, others, other_scores, top_k=8)
    _, value, source, _ = m.recommend_blended_batch(users, others, other_scores, top_k=8, as_arrays=True)
    assert (value > 0).any() and (source[value > 0] != 2).all()
    assert m.recommend_blended_batch(users, others, other_scores, top_k=8, contact_counts=counts) != base     # the counts have teeth
    assert m.recommend_blended_batch(users, others, other_scores, top_k=8, weighting=0.6) != base
    one = m.recommend_blended(users[2], others[2], other_scores[2], top_k=8, contact_counts=counts)
    assert one == m.recommend_blended_batch(users, others, other_scores, top_k=8, contact_counts=counts)[2]
    rec = Recommender(m)
    assert rec.recommend_blended_batch(users, others, other_scores, top_k=8, weighting=0.6) == m.recommend_blended_batch(users, others, other_scores, top_k=8, weighting=0.6)
    assert rec.recommend_blended(users[2], others[2], other_scores[2], top_k=8, contact_counts=counts) == one
    assert m.recommend_blended_batch([], [], []) == []
    if not strings:                                                      # integer ids may come as two [B, K] arrays: the same answer
        width = max(len(r) for r in others)
        oi = np.array([r + [unknown] * (width - len(r)) for r in others], np.int64)
        osc = np.array([r + [0.0] * (width - len(r)) for r in other_scores], F32)
        for kw in (dict(top_k=8, contact_counts=counts), dict(top_k=5, pool=12, weighting=0.6)):
            assert m.recommend_blended_batch(users, oi, osc, **kw) == m.recommend_blended_batch(users, others, other_scores, **kw)
    # two brought lists, no user
    la, lb = others[:6], [plain[b] + [unknown] for b in range(6)]
    sa, sb = other_scores[:6], [np.linspace(2, 1, len(r)).tolist() for r in lb]
    pairs = m.blend_batch(la, sa, lb, sb, top_k=7, weight=0.8, mnz=True)
    for b in range(6):
        ka_ = [(m.item_ids.get_id(i), s) for i, s in zip(la[b], sa[b]) if i != unknown]
        kb_ = [(m.item_ids.get_id(i), s) for i, s in zip(lb[b], sb[b]) if i != unknown]
        A = pad_lists([[i for i, _ in ka_]])[0], pad_lists([[s for _, s in ka_]], None, 0.0, F32)[0], [len(ka_)]
        B = pad_lists([[i for i, _ in kb_]])[0], pad_lists([[s for _, s in kb_]], None, 0.0, F32)[0], [len(kb_)]
        ids, value, _, count = host_model(m.model.n_items_fitted, A, B, min(7, A[0].shape[1] + B[0].shape[1]), weight_b=0.8, mnz=True)
        assert [i for i, _ in pairs[b]] == [m.item_ids.get(int(i)) for i in ids[0, :count[0]]]
        assert np.array_equal(value_bits([v for _, v in pairs[b]]), value_bits(value[0, :count[0]]))
    assert rec.blend_batch(la, sa, lb, sb, top_k=7, weight=0.8, mnz=True) == pairs and m.blend_batch([], [], [], []) == []


def test_every_refusal_of_the_public_calls():
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    fresh = cpu_slim()
    for call in (lambda: fresh.recommend_blended_batch([1], [[1]], [[1.0]]), lambda: fresh.blend_batch([[1]], [[1.0]], [[1]], [[1.0]])):
        with pytest.raises(RuntimeError, match="Model must be fitted"):
            call()
    m, batch = _model()
    users = sorted({u for u, _, _, _ in batch})[:3]
    items = sorted({i for _, i, _, _ in batch})
    oi, osc = [items[:4]] * 3, [[4.0, 3.0, 2.0, 1.0]] * 3
    assert m.recommend_blended_batch(users, oi, osc, top_k=1, pool=1)
    for kw in (dict(top_k=0), dict(top_k=-1), dict(pool=0), dict(pool=1025)):
        with pytest.raises(ValueError, match="top_k >= 1 and 1 <= pool <= 1024"):
            m.recommend_blended_batch(users, oi, osc, **kw)
    for w in ("contact", "", -0.5, float("nan")):
        with pytest.raises(ValueError, match='"contacts" or a non-negative number'):
            m.recommend_blended_batch(users, oi, osc, weighting=w)
    for k in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="similarity_weight_factor"):
            m.recommend_blended_batch(users, oi, osc, similarity_weight_factor=k)
    with pytest.raises(ValueError, match="one score per item"):
        m.recommend_blended_batch(users, oi, [[1.0]] * 3)
    with pytest.raises(ValueError, match="per user"):
        m.recommend_blended_batch(users, oi[:2], osc[:2])
    with pytest.raises(ValueError, match="up to 1024"):
        m.recommend_blended_batch(users[:1], [[items[j % len(items)] for j in range(MAX_LIST + 1)]], [[1.0] * (MAX_LIST + 1)])
    for kw in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight="contacts"), dict(top_k=0)):
        with pytest.raises(ValueError, match="constant non-negative weight|non-negative number"):
            m.blend_batch(oi, osc, oi, osc, **kw)
    with pytest.raises(ValueError, match="one score per item"):
        m.blend_batch(oi, osc, oi, [[1.0]] * 3)
    with pytest.raises(ValueError, match="per user"):
        m.blend_batch(oi, osc, oi[:1], osc[:1])
    # a pool the fused top-k kernels refuse for this model
    eng = m.model.engine
    eng.topk_supported = lambda top_k, mode: top_k < 40
    assert m.recommend_blended_batch(users, oi, osc, top_k=5, pool=39)
    with pytest.raises(ValueError, match="do not serve lists of pool=40 .* smaller pool"):
        m.recommend_blended_batch(users, oi, osc, top_k=5, pool=40)
    with pytest.raises(ValueError, match="do not serve lists of pool=45"):
        m.recommend_blended_batch(users, oi, osc, top_k=45)                # (pool defaults to top_k)
    del eng.topk_supported
    # a float64 W holding float32 numbers is served with its float32 scores; one holding other numbers is refused
    W = m.model.item_similarity
    want = m.recommend_blended_batch(users, oi, osc, top_k=6, weighting=0.5)
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)
    assert m.recommend_blended_batch(users, oi, osc, top_k=6, weighting=0.5) == want
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.recommend_blended_batch(users, oi, osc)
    m.model.item_similarity = W
    # a column-sharded W: the error names the way out
    eng = SlimEngine(backend=BlendOracleBackend(), rank=0, world_size=2, shard_w=True)
    dw = eng.upload_weights(W.tocsc())
    assert isinstance(dw, DeviceWeights)
    dw.shard = (0, 2)
    eng.set_weights(dw)
    mine = m.model._engine
    m.model._engine = eng
    m.model._sync_weights = lambda: None
    try:
        with pytest.raises(ValueError, match=r"gather_item_similarity\(\)"):
            m.recommend_blended_batch(users, oi, osc)
    finally:
        del m.model._sync_weights
        m.model._engine = mine
    # the engine's own ranges
    m.model._sync_weights()
    eng = m.model.engine
    i2, f2 = np.array([[1, 2]], np.int32), np.array([[2.0, 1.0]], F32)
    assert eng.blend_lists(i2, f2, i2, f2, keep=4)[3].tolist() == [2]
    for kw in (dict(keep=0), dict(keep=5), dict(weight_b=-1.0), dict(weight_b=float("nan")), dict(k=-2.0, row_ids=[0])):
        with pytest.raises(ValueError, match="blend"):
            eng.blend_lists(i2, f2, i2, f2, **kw)
    with pytest.raises(ValueError, match="one shape"):
        eng.blend_lists(i2, f2[:, :1], i2, f2)
    with pytest.raises(ValueError, match="one row per row"):
        eng.blend_lists(i2, f2, np.repeat(i2, 2, axis=0), np.repeat(f2, 2, axis=0))
    with pytest.raises(ValueError, match="row_ids"):
        eng.blend_lists(i2, f2, i2, f2, row_ids=[0, 1])
    with pytest.raises(ValueError, match="contact_counts"):
        eng.blend_lists(i2, f2, i2, f2, row_ids=[0], contact_counts=sp.csr_matrix((3, 5), dtype=np.int32))
    with pytest.raises(RuntimeError, match="fitted"):
        SlimEngine(backend=BlendOracleBackend()).blend_lists(i2, f2, i2, f2)


# ---------------------------------------------------------------------------------------------- serving
def test_recommend_blended_route_token_payload_and_failure():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = _model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = batch[0][0]
    mine = m.recommend(user, top_k=6)
    items = [mine[1], mine[4]] + sorted({i for _, i, _, _ in batch})[:5]
    scores = np.linspace(3, 1, len(items)).tolist()
    body = {"user": user, "items": items, "scores": scores, "top_k": 6, "contact_counts": [[mine[0], 3], [mine[1], 1]], "similarity_weight_factor": 0.5}
    r = client.post("/recommend_blended", json=body, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/recommend_blended", json=body, headers=ok)
    want = m.recommend_blended(user, items, scores, top_k=6, contact_counts=[(user, mine[0], 3), (user, mine[1], 1)], similarity_weight_factor=0.5)
    assert r.status_code == 200 and r.json() == {"user": user, "items": want} and len(want) == 6 and mine[0] in want
    r = client.post("/recommend_blended", json={"user": user, "items": items, "scores": scores, "weighting": 0.7, "mnz": True, "pool": 20}, headers=ok)
    assert r.status_code == 200 and r.json()["items"] == m.recommend_blended(user, items, scores, weighting=0.7, mnz=True, pool=20)
    r = client.post("/recommend_blended", json={"user": user, "items": items, "scores": scores[:2]}, headers=ok)      # a model error is the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Recommend blended failed"}
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)                # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(user, top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def test_blend_lists_is_declared_registered_and_exported():
    import ctypes
    import torch
    from rtrec_amd import _native, build, ops
    from tests.test_diverse_host import ext_declared_symbols
    assert "rtrec_slim_blend_lists" in ext_declared_symbols() and ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    assert "rtrec_slim_blend_lists" in _native.EXT_EXPORTS and "rtrec_slim_blend_lists" not in _native.EXPORTS and "blend.hip" in build.SOURCES
    assert "blend_lists" in ops.EXT_OPS and "blend_lists" not in ops.OPS and ops.EXT_EXPORT_OF["blend_lists"] == "rtrec_slim_blend_lists"
    assert (_native.BLEND_CONSTANT, _native.BLEND_CONTACTS) == (0, 1)
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert re.search(r"#define RTREC_BLEND_CONSTANT 0\n#define RTREC_BLEND_CONTACTS 1\n", header)
    assert hasattr(ctypes.CDLL(build.LIB_PATH), "rtrec_slim_blend_lists") and len(_native.load().rtrec_slim_blend_lists.argtypes) == 34
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):      # called through the op only, never by ctypes
        for f in files:
            if f.endswith(".py") and f != "_native.py":
                assert ".rtrec_slim_blend_lists(" not in open(os.path.join(dirpath, f)).read(), f
    schema = str(torch.ops.rtrec_amd.blend_lists.default._schema)
    assert schema.startswith("rtrec_amd::blend_lists(") and schema.endswith("-> ()")
    for name in ("ids", "value", "source", "count"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    for name in ("a_ids", "a_scores", "a_counts", "b_ids", "b_scores", "b_counts"):
        assert f"Tensor {name}" in schema, schema
    for name in ("row_ids", "xb_ptr", "xb_col", "cn_ptr", "cn_col", "cn_val"):
        assert f"Tensor? {name}" in schema, schema
    for arg in ("int ka", "int kb", "int keep", "float weight_b", "bool contacts", "float k", "bool mnz", "int waves_per_row"):
        assert arg in schema, schema
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.blend_lists(5, i32(1, 2), torch.zeros(1, 2), i32(1), 2, i32(1, 2), torch.zeros(1, 2), i32(1), 2, 2, 1.0, False, 2.0,
                                            False, None, None, None, None, None, None, 0, i32(1, 2), torch.zeros(1, 2), i32(1, 2), i32(1))


def test_the_entry_point_checks_its_arguments_on_the_host():
    from rtrec_amd import _native
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    fn = _native.load().rtrec_slim_blend_lists
    one = 1                                                              # any non-NULL address: never dereferenced on these paths

    def args(n_rows=1, n_items=5, a_ids=one, ais=10, a_sc=one, ass=10, a_cnt=one, ka=10, b_ids=one, bis=7, b_sc=one, bss=7, b_cnt=one, kb=7,
             keep=3, weight_b=1.0, mode=0, k=2.0, mnz=0, rows=one, xptr=one, xcol=one, n_x=4, xnnz=3, cptr=one, ccol=one, cval=one, cnnz=2,
             waves=0, ids=one, value=one, source=one, count=one):
        return (n_rows, n_items, a_ids, ais, a_sc, ass, a_cnt, ka, b_ids, bis, b_sc, bss, b_cnt, kb, keep, weight_b, mode, k, mnz, rows, xptr,
                xcol, n_x, xnnz, cptr, ccol, cval, cnnz, waves, ids, value, source, count, None)

    for kw in (dict(ka=0), dict(ka=1025, ais=1025, ass=1025), dict(kb=0), dict(kb=1025, bis=1025, bss=1025), dict(keep=0), dict(keep=18),
               dict(keep=-1), dict(waves=2), dict(waves=-1), dict(waves=8), dict(mode=2), dict(mode=-1)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(weight_b=-0.5), dict(weight_b=float("nan")), dict(k=-0.5), dict(k=float("nan")), dict(n_rows=-1), dict(n_items=-1),
               dict(n_x=-1), dict(xnnz=-1), dict(cnnz=-1), dict(ais=9), dict(ass=9), dict(bis=6), dict(bss=6), dict(a_ids=None),
               dict(a_sc=None), dict(a_cnt=None), dict(b_ids=None), dict(b_sc=None), dict(b_cnt=None), dict(ids=None), dict(value=None),
               dict(source=None), dict(count=None), dict(mode=1, xptr=None), dict(mode=1, xcol=None), dict(mode=1, ccol=None),
               dict(mode=1, cval=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, a_ids=None, b_sc=None, ids=None, mode=1, xptr=None)) == 0
    assert fn(*args(n_rows=0, keep=17)) == 0                             # keep = ka + kb is served
    for name in ("blend_device", "blend_lists"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "blend_lists"))
