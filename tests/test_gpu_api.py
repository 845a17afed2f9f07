"""Drop-in API on the real GPU path: rtrec_amd.SLIM / Recommender vs golden outputs of the
reference (tests/golden/, tools/gen_golden.py)."""
import io
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def load_csc(z, prefix):
    return sp.csc_matrix((z[f"{prefix}_data"], z[f"{prefix}_indices"], z[f"{prefix}_indptr"]),
                         shape=tuple(z[f"{prefix}_shape"]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_matrix(A, B):
    A, B = A.tocsc(), B.tocsc()
    A.sort_indices(); B.sort_indices()
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


def test_reference_unit_test_scenarios():
    from rtrec_amd import SLIM
    api = json.load(open(os.path.join(G, "api.json")))
    m = SLIM()
    m.fit([tuple(x) for x in api["similar_items"]["interactions"]])
    assert m.similar_items("item_1", top_k=5) == ["item_4", "item_3"] == api["similar_items"]["similar_item_1"]
    got = m.similar_items("item_1", top_k=5, ret_scores=True)
    ref = api["similar_items"]["similar_item_1_scores"]
    assert [a for a, _ in got] == [a for a, _ in ref]
    assert np.array_equal(bits([b for _, b in got]), bits([b for _, b in ref]))
    assert m.recommend("user_2", top_k=5) == api["similar_items"]["recommend_user_2"]

    m = SLIM()
    inter = [tuple(x) for x in api["fit_and_recommend"]["interactions"]]
    m.fit(inter)
    m.fit(iter(inter))            # generator input, additive re-ingest
    assert m.recommend("user_1", top_k=5) == ["item_4", "item_2"] == api["fit_and_recommend"]["recommend_user_1"]
    assert m.interactions.get_user_item_rating(0, 0) == api["fit_and_recommend"]["rating_u1_i1"]

    m = SLIM()
    m.fit([tuple(x) for x in api["recommend_batch"]["interactions"]])
    users = ["user_1", "user_2", "user_3"]
    ref = api["recommend_batch"]
    assert m.recommend_batch(users, top_k=2) == ref["top2"]
    assert m.recommend_batch(users, candidate_items=["item_1", "item_2", "item_3"], top_k=2) == ref["cands"]
    assert m.recommend_batch(["user_1"], top_k=3, filter_interacted=False) == ref["nofilter_u1"]
    assert m.recommend_batch(["user_1", "nobody"], top_k=2) == ref["cold"]
    assert m.recommend_batch([], top_k=2) == []

    m = SLIM()
    m.fit([tuple(x) for x in api["int_ids"]["interactions"]])
    assert m.recommend_batch([1, 2, 3, 4], top_k=3) == api["int_ids"]["top3"]
    assert m.recommend_batch([1, 2, 3, 4], top_k=3, filter_interacted=False) == api["int_ids"]["nofilter"]
    assert m.recommend(99, top_k=3) == api["int_ids"]["cold_99"]
    assert m.similar_items(10, top_k=3) == api["int_ids"]["similar_10"]
    buf = io.BytesIO()
    m.save(buf)
    m2 = SLIM.loads(buf.getvalue())
    assert m2.recommend_batch([1, 2, 3, 4], top_k=3) == api["int_ids"]["top3"]


@pytest.mark.parametrize("name,kw", [("k5", {"nn_feature_selection": 5}), ("all", {}),
                                     ("k5_decay", {"nn_feature_selection": 5, "decay_in_days": 30})])
def test_incremental_fit_sequence_on_gpu(name, kw):
    from rtrec_amd import SLIM
    z = np.load(os.path.join(G, "partial_fit.npz"))
    u, i, v, ts = z["u"], z["i"], z["v"], z["ts"]
    m = SLIM(min_value=0, max_value=15, **kw)
    for label, key, upsert in (("A", "A", False), ("B", "B", False), ("C_add", "C", False), ("C_upsert", "C", True)):
        a, b = z[key]
        batch = [(int(x), int(y), float(t), float(r)) for x, y, t, r in zip(u[a:b], i[a:b], ts[a:b], v[a:b])]
        m.fit(batch, update_interaction=upsert, progress_bar=False)
        assert same_matrix(m.model.item_similarity, load_csc(z, f"W_{name}_{label}")), f"{name} after {label}"
    users = z[f"rec_users_{name}"].tolist()
    assert m.recommend_batch(users, top_k=5) == [[x for x in row.tolist() if x >= 0] for row in z[f"rec_{name}"]]


def test_slimelastic_matches_reference_models_and_scores():
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    z = np.load(os.path.join(G, "models.npz"))
    zs = np.load(os.path.join(G, "scoring.npz"))
    X = load_csc(z, "X")
    assert same_matrix(SLIMElastic({}).fit(X.copy()).item_similarity, load_csc(z, "W_serial_all"))
    assert same_matrix(SLIMElastic({"nn_feature_selection": 8}).fit(X.copy(), parallel=True).item_similarity,
                       load_csc(z, "W_parallel_k8"))
    assert same_matrix(SLIMElastic({"nn_feature_selection": 8, "positive_only": False})
                       .partial_fit_items(X.copy(), list(range(60))).item_similarity, load_csc(z, "W_nonpos_k8"))
    X2 = load_csc(z, "X2")
    m = SLIMElastic({"nn_feature_selection": 50}).partial_fit_items(X2.copy(), list(range(400)))
    assert same_matrix(m.item_similarity, load_csc(z, "W2_k50"))
    users = zs["users"].tolist()
    Xr = X2.tocsr()
    for wname in ("f32", "f64"):
        if wname == "f64":
            m.item_similarity = sp.csc_matrix(m.item_similarity, dtype=np.float64)
        for filt in (True, False):
            out = m.recommend_batch(users, Xr, top_k=10, filter_interacted=filt, dense_output=False, ret_scores=True)
            key = f"{wname}_sparse_{'filter' if filt else 'nofilter'}"
            for r, (ids, sc) in enumerate(out):
                ref = [x for x in zs[f"ids_{key}"][r].tolist() if x >= 0]
                assert ids == ref
                assert np.array_equal(bits(sc), bits(zs[f"scores_{key}"][r, :len(ref)]))
    m.item_similarity = load_csc(z, "W2_k50")
    out = m.recommend_batch(users, Xr, candidate_item_ids=zs["cands"].tolist(), top_k=5, ret_scores=True)
    for r, (ids, sc) in enumerate(out):
        g = zs["scores_cands"][r]
        n = next((k for k in range(4) if g[k] == g[k + 1]), 5)       # untied prefix (D1)
        assert ids[:n] == zs["ids_cands"][r, :n].tolist()
        assert np.array_equal(bits(sc[:n]), bits(g[:n]))
    for j in range(0, 400, 7):
        ids, sc = m.similar_items(j, top_k=6, ret_ndarrays=True)
        g = zs["similar_scores"][j]
        fin = int(np.sum(np.isfinite(g)))
        n = next((k for k in range(fin - 1) if g[k] == g[k + 1]), fin)
        assert ids[:n].tolist() == zs["similar_ids"][j, :n].tolist()


def test_predict_score_vectors_on_gpu():
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    z = np.load(os.path.join(G, "models.npz"))
    zs = np.load(os.path.join(G, "scoring.npz"))
    X2 = load_csc(z, "X2").tocsr()
    m = SLIMElastic({"nn_feature_selection": 50})
    m.item_similarity = load_csc(z, "W2_k50")
    users, cands = zs["predict_users"].tolist(), zs["cands"].tolist()
    for r, u in enumerate(users):
        assert np.array_equal(bits(m.predict(u, X2).ravel()), bits(zs["predict_dense"][r]))
        assert np.array_equal(bits(m.predict(u, X2, dense_output=False).toarray().ravel()), bits(zs["predict_sparse_as_dense"][r]))
        assert np.array_equal(bits(m.predict_selected(u, cands, X2).ravel()), bits(zs["predict_selected"][r]))
    assert np.array_equal(bits(m.predict_all(X2[:40])), bits(zs["predict_all_head"]))
    m.item_similarity = sp.csc_matrix(m.item_similarity, dtype=np.float64)
    for r, u in enumerate(users):
        d64 = m.predict(u, X2)
        assert d64.dtype == np.float64 and np.array_equal(d64.ravel(), zs["predict_dense_f64"][r])


def test_reference_written_model_file_serves_on_gpu():
    from rtrec_amd import SLIM
    exp = json.load(open(os.path.join(G, "ref_pickles.json")))
    m = SLIM.loads(open(os.path.join(G, "ref_slim_int.pkl"), "rb").read())
    assert m.recommend_batch(exp["int"]["users"], top_k=5) == exp["int"]["recs"]
    assert m.similar_items(3, top_k=4) == exp["int"]["similar_3"]
    s = SLIM.loads(open(os.path.join(G, "ref_slim_str.pkl"), "rb").read())
    assert s.similar_items("item_1", top_k=5) == exp["str"]["similar_item_1"]
    assert s.recommend("user_2", top_k=5) == exp["str"]["rec_user_2"]


@pytest.mark.parametrize("session", ["str", "int"])
def test_serving_shell_on_the_gpu_replays_the_reference_transcript(session):
    """The HTTP shell with its default model (GPU engine) against the transcript of the reference's
    FastAPI app (tests/golden/serving.json)."""
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import create_app
    steps = json.load(open(os.path.join(G, "serving.json")))[session]
    client = TestClient(create_app())
    for st in steps:
        r = client.get(st["path"]) if st["method"] == "GET" else client.post(st["path"], json=st["json"], headers=st["headers"])
        assert r.status_code == st["status"], st
        assert r.json() == st["response"], st


def test_large_top_k_through_the_api():
    """top_k beyond one wave's lanes (the reference accepts any k): ids and order vs the oracle."""
    from oracle import slim_oracle as so
    from rtrec_amd import SLIM
    from rtrec_amd.synth import interaction_matrix
    X = interaction_matrix(400, 900, 30000, seed=12)
    coo = X.tocoo()
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=40)
    m.fit(list(zip(coo.row.tolist(), coo.col.tolist(), (1.7e9 + np.arange(coo.nnz)).tolist(), coo.data.astype(float).tolist())),
          progress_bar=False)
    users = list(range(0, 400, 7))
    W = m.model.item_similarity.tocsr()
    Xs = m.interactions.to_csr()
    for k in (100, 300):
        got = m.recommend_batch(users, top_k=k)
        o_ids, _, o_cnt = so.recommend_batch(Xs[users], W, top_k=k, filter_interacted=True)
        assert got == [o_ids[r, :o_cnt[r]].tolist() for r in range(len(users))]


@pytest.mark.parametrize("decay", [None, 30])
def test_streaming_through_the_device_resident_store_equals_host_exports(decay, monkeypatch):
    """SLIM.fit mini-batches served from the device-resident X (utils/device_store.py: bulk_fit's upload
    adopted, every batch merged on the GPU, touched-columns matrix gathered there) give the same W,
    bit for bit, and the same recommendations as the host-export path (RTREC_AMD_DEVICE_STORE=0),
    including new users / items and re-rated pairs -- also for a store with time decay, whose every value moves
    with max_timestamp at every batch and is re-evaluated by the device decay kernel."""
    from rtrec_amd import SLIM
    rng = np.random.default_rng(11)
    U, I, n = 1500, 300, 40_000
    u, i = rng.integers(0, U, n), rng.zipf(1.3, n) % I
    r = (rng.integers(1, 6, n) * np.exp(-rng.random(n))).astype(float)
    ts = 1.7e9 + np.arange(n, dtype=float) * (600.0 if decay else 1.0)          # with decay: ~9 months of history
    n_bulk = n - 6 * 400

    def run(device_store):
        monkeypatch.setenv("RTREC_AMD_DEVICE_STORE", "1" if device_store else "0")
        m = SLIM(min_value=0, max_value=15, nn_feature_selection=8, **({"decay_in_days": decay} if decay else {}))
        m.add_interactions(list(zip(u[:n_bulk].tolist(), i[:n_bulk].tolist(), ts[:n_bulk].tolist(), r[:n_bulk].tolist())))
        m.bulk_fit(parallel=True, progress_bar=False)
        assert (m._dev_x is not None and m._dev_x.version == m._store_tag()) == device_store
        out = []
        for k in range(6):
            a = n_bulk + 400 * k
            uu, ii = u[a:a + 400] + (30 * k if k % 2 else 0), i[a:a + 400] + (7 * k if k % 3 == 0 else 0)   # some new ids
            m.fit(list(zip(uu.tolist(), ii.tolist(), ts[a:a + 400].tolist(), r[a:a + 400].tolist())), progress_bar=False)
            if device_store:
                assert m._dev_x.version == m._store_tag() and m._dev_x.nnz == m.interactions.nnz
            out.append((m.model.item_similarity.copy(), m.recommend_batch(list(range(0, 200, 3)), top_k=7)))
        # incremental Recommender.fit on a numeric DataFrame: the columnar ingest advances the mirror too
        import contextlib, io
        import pandas as pd
        from rtrec_amd import Recommender
        df = pd.DataFrame({"user": u[:300] + 5, "item": i[:300], "tstamp": ts[-1] + 1.0 + np.arange(300), "rating": r[:300]})
        loads = []
        if device_store:
            orig = m._dev_x.load_store
            m._dev_x.load_store = lambda *a, **k: (loads.append(1), orig(*a, **k))[1]
        with contextlib.redirect_stdout(io.StringIO()):
            Recommender(m).fit(df)
        assert not loads                                   # advanced incrementally, never rebuilt from a host export
        if device_store:
            assert m._dev_x.version == m._store_tag() and m._dev_x.nnz == m.interactions.nnz
        out.append((m.model.item_similarity.copy(), m.recommend_batch(list(range(0, 200, 3)), top_k=7)))
        return out

    dev, host = run(True), run(False)
    for (Wd, rd), (Wh, rh) in zip(dev, host):
        assert same_matrix(Wd, Wh)
        assert rd == rh


@pytest.mark.parametrize("parallel,decay", [(False, None), (True, None), (True, 30)])
def test_bulk_fit_from_the_device_resident_store_equals_host_export(parallel, decay, monkeypatch):
    """SLIM.bulk_fit takes X from the resident store (host CSR keys, CSC order by a device sort): same W
    bits and dtype (float64 after a serial fit, float32 after a parallel one) as through to_csc() -- also for
    a store with time decay, whose resident values are re-evaluated on the device (csrc/store_device.hip)."""
    from rtrec_amd import SLIM
    rng = np.random.default_rng(5)
    U, I, n = 900, 200, 20_000
    rows = list(zip(rng.integers(0, U, n).tolist(), (rng.zipf(1.3, n) % I).tolist(),
                    (1.7e9 + np.arange(n)).tolist(), (rng.integers(1, 6, n) * np.exp(-rng.random(n))).tolist()))

    def run(device_store):
        monkeypatch.setenv("RTREC_AMD_DEVICE_STORE", "1" if device_store else "0")
        kw = {"decay_in_days": decay} if decay else {}
        m = SLIM(min_value=0, max_value=15, nn_feature_selection=8, **kw)
        m.add_interactions(rows)
        m.bulk_fit(parallel=parallel, progress_bar=False)
        assert (m._dev_x is not None and m._dev_x.version == m._store_tag()) == device_store
        return m.model.item_similarity, m.recommend_batch(list(range(0, 300, 7)), top_k=5)

    (Wd, rd), (Wh, rh) = run(True), run(False)
    assert Wd.dtype == Wh.dtype == (np.float32 if parallel else np.float64)
    assert Wd.shape == Wh.shape and np.array_equal(Wd.indptr, Wh.indptr) and np.array_equal(Wd.indices, Wh.indices)
    assert np.array_equal(Wd.data.view(np.uint8), Wh.data.view(np.uint8))
    assert rd == rh


@pytest.mark.parametrize("upsert", [False, True])
def test_device_bulk_ingest_equals_the_host_store(upsert, monkeypatch):
    """Bulk batches are sorted, cut into runs of equal pairs and folded on the GPU (DeviceInteractions.ingest ->
    rtrec_store_fold_device): the store, the hot items and the resident matrix must equal the host path's, for a batch into
    an empty store (the mirror adopts the folded block), a second batch on top of it (merged into the mirror on the device),
    a pair repeated 50,000 times, NaN ratings and clipping at both ends; then the same through Recommender.bulk_fit."""
    import pandas as pd
    from rtrec_amd import SLIM, Recommender
    from rtrec_amd.utils import interactions as mod
    from tests.test_host_logic import bits64, bulk_batches
    monkeypatch.setattr(mod, "_DEVICE_FOLD_MIN", 1000)
    u, i, ts, r = bulk_batches(n=400_000, n_users=9000, n_items=700)
    u[::8], i[::8] = 5, 3                  # one long run: the kernel's eight-at-a-time loop
    cut = 250_000

    def run(device):
        monkeypatch.setenv("RTREC_AMD_DEVICE_INGEST", "1" if device else "0")
        m = SLIM(min_value=-3, max_value=10, nn_feature_selection=8)
        m.add_interactions_columns(u[:cut], i[:cut], ts[:cut], r[:cut], update_interaction=upsert)
        in_step = m._dev_x is not None and m._dev_x.version == m._store_tag()
        m.add_interactions_columns(u[cut:], i[cut:], ts[cut:], r[cut:], update_interaction=upsert)
        in_step = in_step and m._dev_x.version == m._store_tag()
        return m, in_step

    (md, dev_in_step), (mh, host_in_step) = run(True), run(False)
    assert dev_in_step and not host_in_step
    a, b = md.interactions._compact(), mh.interactions._compact()
    assert np.array_equal(a.key, b.key) and np.array_equal(a.ts, b.ts) and np.array_equal(bits64(a.val), bits64(b.val))
    assert md.interactions.max_timestamp == mh.interactions.max_timestamp and md.interactions.shape == mh.interactions.shape
    assert md.interactions.all_item_ids == mh.interactions.all_item_ids
    assert list(md.interactions.hot_items.data.items()) == list(mh.interactions.hot_items.data.items())
    X, H = md._dev_x.full(), mh.interactions.to_csr()
    assert np.array_equal(X["rptr"].cpu().numpy(), H.indptr) and np.array_equal(X["rcol"].cpu().numpy(), H.indices)
    assert np.array_equal(bits(X["rval"].cpu().numpy()), bits(H.data))

    # Recommender.bulk_fit on a DataFrame: one device-folded chunk, then the fit from the adopted mirror
    ok = ~np.isnan(r)
    df = pd.DataFrame({"user": u[ok], "item": i[ok], "tstamp": ts[ok], "rating": np.abs(r[ok])})
    recs = []
    for device in (True, False):
        monkeypatch.setenv("RTREC_AMD_DEVICE_INGEST", "1" if device else "0")
        rec = Recommender(SLIM(min_value=0, max_value=15, nn_feature_selection=8))
        rec.bulk_fit(df, update_interaction=upsert)
        recs.append((rec.model.model.item_similarity, rec.recommend_batch(list(range(0, 400, 9)), top_k=5)))
    (Wd, rd), (Wh, rh) = recs
    assert same_matrix(Wd, Wh) and rd == rh


_RCCL_ONE_RANK = r"""
import os, sys, numpy as np, scipy.sparse as sp, torch, torch.distributed as dist
G = sys.argv[1]
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
from rtrec_amd.engine import SlimEngine
from rtrec_amd.models.internal.slim_elastic import SLIMElastic
z, zs = np.load(os.path.join(G, "models.npz")), np.load(os.path.join(G, "scoring.npz"))
load = lambda p: sp.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(z[p + "_shape"]))
X, users = load("X2").tocsr(), zs["users"].tolist()
for mode in ("columns", "rows"):
    eng = SlimEngine(device="cuda:0", rank=0, world_size=1, score_shard=mode)
    eng.force_exchange = True
    eng.row_chunk_rows = eng.gather_chunk_rows = 7                       # several chunks: several asynchronous exchanges in flight
    m = SLIMElastic({"nn_feature_selection": 50}, engine=eng)
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        m.item_similarity = sp.csc_matrix(load("W2_k50"), dtype=dtype)
        out = m.recommend_batch(users, X, top_k=10, filter_interacted=True, dense_output=False)
        assert out == [[x for x in row.tolist() if x >= 0] for row in zs[f"ids_{tag}_sparse_filter"]], (mode, tag, "sparse")
        out = m.recommend_batch(users, X, top_k=10, filter_interacted=False, dense_output=True)
        assert out == [[x for x in row.tolist() if x >= 0] for row in zs[f"ids_{tag}_dense_nofilter"]], (mode, tag, "dense")
torch.cuda.synchronize()
dist.destroy_process_group()
print("RCCL-EXCHANGE-OK")
"""


def test_exchange_path_over_rccl_with_one_rank():
    """The multi-GPU exchange of the scoring path (all_to_all_single of per-shard lists, strided merge of the
    received block, all_gather_into_tensor of the final lists; row-shard mode too) pushed through RCCL
    itself: a 1-rank NCCL group on this box's GPU, in a child process, against the reference goldens."""
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", _RCCL_ONE_RANK, G], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RCCL-EXCHANGE-OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _small_int_model(n_users=300, n_items=1800, seed=9, **kw):
    from rtrec_amd import SLIM
    rng = np.random.default_rng(seed)
    n = 12000
    u, i = rng.integers(0, n_users, n), (rng.zipf(1.25, n) - 1) % n_items
    r = rng.integers(1, 6, n).astype(float) + rng.random(n)
    ts = 1.7e9 + np.arange(n, dtype=float)
    m = SLIM(nn_feature_selection=20, **kw)
    m.add_interactions(list(zip(u.tolist(), i.tolist(), ts.tolist(), r.tolist())))
    m.bulk_fit(progress_bar=False)
    return m


def test_user_ids_outside_the_matrix_never_reach_the_device():
    """internal user ids outside [0, n_users) used to be read out of bounds by the
    resident-X kernels.  They now get the reference's scipy semantics (slim.py:93, slim_elastic.py:707):
    IndexError beyond the matrix, and a negative id wraps to a row that is empty unless it is in the batch."""
    from rtrec_amd.engine import SlimEngine
    m = _small_int_model()
    n_users = m.interactions.shape[0]
    ok = m.recommend_batch([0, 1, 2], top_k=5)
    assert m._recommend_hot_batch([0, -1, 2], top_k=5) == [ok[0], [], ok[2]]
    last = m._recommend_hot_batch([n_users - 1], top_k=5)[0]
    assert m._recommend_hot_batch([-1, n_users - 1], top_k=5) == [last, last]      # -1 IS the last row here
    assert m.recommend(-1, top_k=5) == []
    with pytest.raises(IndexError):
        m._recommend_hot_batch([n_users], top_k=5)
    with pytest.raises(IndexError):
        m._recommend_hot_batch([-n_users - 1], top_k=5)
    with pytest.raises(IndexError):
        m.model.engine.recommend_rows([0, n_users], top_k=5)
    with pytest.raises(IndexError):
        m.model.engine.recommend_rows([-1], top_k=5)
    # a user known only through register_user_feature has no row: string ids -> internal id >= n_users
    from rtrec_amd import SLIM
    s = SLIM()
    s.fit([("a", "x", 1.7e9, 1.0), ("b", "y", 1.7e9, 2.0), ("a", "y", 1.7e9, 1.0)], progress_bar=False)
    s.recommend_batch(["a", "b"], top_k=2)
    s.register_user_feature("ghost", ["tag"])
    with pytest.raises(IndexError):
        s.recommend("ghost", top_k=2)


@pytest.mark.parametrize("dense", [False, True])
def test_top_k_beyond_the_kernel_limit_is_served_from_device_scores(dense, oracle):
    """top_k > 1023 (rtrec_slim_score_topk's limit; the reference accepts any top_k): score rows from the
    device, selection on the host in the reference's orders -- equal to the oracle, and equal to the fused
    kernel's answer on the prefix it can produce."""
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    m = _small_int_model()
    W = m.model.item_similarity
    X = m.interactions.to_csr()
    users = list(range(0, 300, 7))
    el = SLIMElastic({"nn_feature_selection": 20})
    el.item_similarity = W
    big = el.recommend_batch(users, X, top_k=1500, dense_output=dense, ret_scores=True)
    o_ids, o_sc, o_cnt = oracle.recommend_batch(X[users], W.tocsr(), top_k=1500, dense=dense, use_f64=(W.dtype == np.float64))
    for (ids, sc), oi, os_, oc in zip(big, o_ids, o_sc, o_cnt):
        assert ids == oi[:oc].tolist()
        assert np.array_equal(bits(sc), bits(os_[:oc]))
    small = el.recommend_batch(users, X, top_k=50, dense_output=dense)
    assert [ids[:50] for ids, _ in big] == small
    # candidates: the whole candidate list, ranked
    cands = list(range(5, 1700))
    got = el.recommend_batch(users[:5], X, candidate_item_ids=cands, top_k=1400)
    ref = el.recommend_batch(users[:5], X, candidate_item_ids=cands, top_k=1000)
    assert [g[:1000] for g in got] == ref and all(len(g) == 1400 for g in got)


def test_evaluate_matches_the_reference_end_to_end_on_gpu():
    """N3: Recommender.fit + evaluate (ndcg@k, recall, map, auc ...) on the GPU path equal the reference's run."""
    from rtrec_amd import SLIM
    from tests.test_pipeline_cpu import _evaluate_against_golden
    _evaluate_against_golden(SLIM)


def test_api_randomised_parity():
    """tools/fuzz_api.py: random interaction streams (bulk fit, mini-batches with repeats and upserts, time decay, negative
    ratings, int or str ids, K or every item) through rtrec_amd.SLIM on the GPU and on the oracle backend -- W bits,
    recommend_batch and similar_items after every step (1,500 scenarios run clean after the -0.0 product fix it led to;
    40 run here)."""
    from tools.fuzz_api import run
    messages = []
    assert run(40, seed=3, log=messages.append) == 0, messages


def test_hybrid_slimfm_call_sequence_on_the_gpu():
    """HybridSlimFM's calls on its SLIM half (hybrid.py:122,151,196,217,225,267,381,409,477) replayed on the product path against the
    real SLIMElastic's answers (tests/golden/hybrid_calls.json)."""
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    from tests.hybrid_replay import replay
    replay(lambda cfg: SLIMElastic(cfg))


def test_model_level_batch_calls_serve_cold_and_odd_users_on_the_gpu():
    """The identities of tests/test_user_batch_host.py (who gets recommend_batch's list, the padding, the list tails) for the
    integer-id and the string-id mix of regular, cold and out-of-matrix users, through the real backend."""
    from rtrec_amd import SLIM
    from tests.test_user_batch_host import build_case, check_mix
    for kind in ("int", "str"):
        c = build_case(kind, make=SLIM)
        for name in ("mix with the last user", "mix without the last user") if kind == "int" else ("mix",):
            check_mix(c, c.mixes[name])


def test_custom_ops_refuse_mistyped_tensors():
    """csrc/torch_ops.cpp checks every pointer it hands to the C-ABI: a tensor of another dtype, a strided view or a host
    tensor raises instead of becoming an out-of-bounds access on the GPU -- for the ops added in round 5 as for the old ones."""
    import torch
    from rtrec_amd import ops as _registered        # noqa: F401  (importing it loads and binds the ops library)
    ops = torch.ops.rtrec_amd
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    ptr2 = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    bad_calls = [
        lambda: ops.store_decay_device(f32(4), f64(4), 0.9, 1.0, f32(4), i32(8), i32(1)),                        # raw must be float64
        lambda: ops.store_fold_device(i32(4), i64(2), f64(4), f64(4), None, 0.0, 5.0, False, f64(1), f64(1), f32(1)),   # order int64
        lambda: ops.first_touch_aux(None, ptr2, i64(1), 1, 4, ptr2, i32(1), 2, i32(1, 2), i32(1), i32(1, 2)),    # xb_col int32
        lambda: ops.dense_fill(None, ptr2, i32(1), 1, 0, 4, 2, True, i64(1, 2), f32(1, 2), i32(1, 2), i32(1), i32(2), i32(2)),
        lambda: ops.refine_topk_f64(None, ptr2, i32(1), f64(1), 1, 4, ptr2, i32(1), f32(1), 2, i32(1, 3), f32(1, 3), i32(1), 1e-6, None,
                                    i32(1, 2), f32(1, 2), f64(1, 2), i32(1), i32(2)),                               # xb_val float32
        lambda: ops.score_candidates(None, ptr2, i32(1), f32(1), 1, 4, ptr2, i32(1), f32(1), i64(2), 2, False, i32(1, 2), f32(1, 2), None, i32(1)),
        lambda: ops.seg_plan(i32(4), i64(4), 8, 0, 8, i64(8), torch.zeros(64, dtype=torch.uint8, device=dev)),     # rows int64
        lambda: ops.ordered_sums(f64(8), i64(2), 0, f32(1)),                                                      # values float32
        lambda: ops.ordered_sums(f32(8).cpu(), i64(2), 0, f32(1)),                                                # host tensor
        lambda: ops.ordered_sums(f32(16)[::2], i64(2), 0, f32(1)),                                                # strided view
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
    # fit_sgd_epochs: every tensor slot in turn with another dtype and as a host tensor, and a cap outside 1..256 -- each a
    # RuntimeError before anything is launched.  The well-typed call is a 2 x 2 matrix, one target, one feature, one epoch.
    def sgd_args():
        return [torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), i32(1, 2), f32(1, 2), i32(1), torch.ones(1, 1, dtype=torch.int32, device=dev),
                torch.ones(1, dtype=torch.int32, device=dev), 2, 2, 2, 1, 0, 1, 1, 1e-4, f64(2), torch.ones(2, dtype=torch.float64, device=dev),
                torch.ones(2, dtype=torch.float64, device=dev), f64(2), i32(3), f32(1), f32(1, 1), f32(1, 1),
                torch.full((1,), float("inf"), dtype=torch.float64, device=dev), i32(1), i32(1), i32(1)]
    tensor_slots = [k for k, a in enumerate(sgd_args()) if isinstance(a, torch.Tensor)]
    assert len(tensor_slots) == 18
    other = {torch.int32: torch.float32, torch.float32: torch.int32, torch.float64: torch.float32}
    for k in tensor_slots:
        for spoil in (lambda t: t.to(other[t.dtype]), lambda t: t.cpu()):
            args = sgd_args()
            args[k] = spoil(args[k])
            with pytest.raises(RuntimeError):
                ops.fit_sgd_epochs(*args)
    for cap in (257, 0):
        args = sgd_args()
        args[9] = cap
        with pytest.raises(RuntimeError):
            ops.fit_sgd_epochs(*args)
    args = sgd_args()
    ops.fit_sgd_epochs(*args)
    torch.cuda.synchronize()
    assert int(args[-2].item()) == 1 and int(args[-1].item()) == 0          # max_iter = 1 reached, nobody unfinished
    # and a well-typed call goes through
    vals = torch.arange(8, dtype=torch.float32, device=dev)
    out = f32(1)
    ops.ordered_sums(vals, torch.tensor([0, 8], dtype=torch.int64, device=dev), 0, out)
    assert float(out.item()) == 28.0
