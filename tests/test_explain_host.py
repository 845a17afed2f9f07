"""Explanations (SLIM.explain_batch, csrc/explain.hip) without a GPU: the definition as a numpy host model, pinned to the
reference's scores on the golden fixture; the model / facade / serving layers end to end through the CPU stand-in backend
with `explain_topk` supplied by the host model; the registration of the op.  The kernel itself is in tests/test_gpu_explain.py.

The definition (include/rtrec_amd.h, "EXPLANATIONS"): for a user row u and an item i the contributing items are the j stored in
both row u of X and column i of W, c(j) = float32(x_uj) * float32(w_ji) in float32, support = their number, reasons = the top_m
by c descending, the lower item id first among equal c."""
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
    return common.astype(np.int64), xv[xi] * ww[wi]                     # float32 * float32: one rounding


def host_model(X, W, rows, ids, counts, top_m):
    """THE DEFINITION: (reason_items[B, k, top_m] int32, contributions[B, k, top_m] float32, support[B, k] int32), -1 / -inf
    padded.  A slot at or beyond counts[b], an item outside [0, n_items) and a row outside [0, n_users) are empty."""
    ids = np.asarray(ids)
    B, k = ids.shape
    items = np.full((B, k, top_m), -1, np.int32)
    contrib = np.full((B, k, top_m), -np.inf, np.float32)
    support = np.zeros((B, k), np.int32)
    for b in range(B):
        for p in range(min(max(int(counts[b]), 0), k)):
            j, c = pair_contributions(X, W, int(rows[b]), int(ids[b, p]))
            order = np.lexsort((j, -c))[:top_m]                         # c descending, then the lower item id
            support[b, p] = len(j)
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
        pair, j, c = pair[hit], j[hit], xval[pos[hit]] * W.data[off[hit]].astype(np.float32)
        sup = np.bincount(pair, minlength=len(item))
        order = np.lexsort((j, -c, pair))
        pair, j, c = pair[order], j[order], c[order]
        rank = np.arange(len(pair)) - (np.cumsum(sup) - sup)[pair]
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
