"""explain_topk_kernel (csrc/explain.hip) on the GPU against the host model of tests/test_explain_host.py -- `==` on reason ids,
contribution bits and support for every pair -- and SLIM.explain_batch end to end: the ordered float32 sum of a pair's
contributions is the score the scoring kernels report for it."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from tests.test_explain_host import EDGE_TOP_M, bits, edge_case, golden, host_model, host_model_vectorised, ordered_sum

pytestmark = pytest.mark.gpu


def run_op(X, W, rows, ids, counts, list_k, top_m):
    """torch.ops.rtrec_amd.explain_topk on host matrices: X csr, W csc (sorted), rows None = identity, ids [n, >= list_k]."""
    import torch
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")
    n = ids.shape[0]
    items = torch.full((n, list_k, top_m), 12345, dtype=torch.int32, device="cuda:0")       # poisoned: every slot must be written
    contrib = torch.full((n, list_k, top_m), 7.0, dtype=torch.float32, device="cuda:0")
    support = torch.full((n, list_k), -7, dtype=torch.int32, device="cuda:0")
    torch.ops.rtrec_amd.explain_topk(None if rows is None else up(rows, np.int32), up(X.indptr, np.int32), up(X.indices, np.int32),
                                     up(X.data, np.float32), W.shape[1], up(W.indptr, np.int32), up(W.indices, np.int32),
                                     up(W.data, np.float32), up(ids, np.int32), up(counts, np.int32), list_k, top_m, items, contrib, support)
    torch.cuda.synchronize()
    return items.cpu().numpy(), contrib.cpu().numpy(), support.cpu().numpy()


def assert_same(got, want, what=""):
    bad = np.flatnonzero((got[0] != want[0]).any(axis=2).ravel() | (bits(got[1]) != bits(want[1])).any(axis=2).ravel()
                         | (got[2] != want[2]).ravel())
    assert bad.size == 0, f"{what}: {bad.size} pairs differ from the host model, first (row, slot) {divmod(int(bad[0]), got[2].shape[1])}"


@pytest.fixture(scope="module")
def golden_lists(engine):
    """The golden fixture's X / W and, for ALL 1,200 users, the lists the scoring kernels give at k = 1, 10, 64."""
    X, W, _, _, _ = golden()
    assert X.shape[0] == 1200
    engine.set_interactions(None, X, need_csc=False)
    engine.set_weights(W)
    lists = {k: engine.recommend_rows(np.arange(1200), top_k=k) for k in (1, 10, 64)}
    return X, W, lists


@pytest.mark.parametrize("list_k", [1, 10, 64])
@pytest.mark.parametrize("top_m", [1, 3, 32])
def test_op_equals_the_definition_on_the_golden_fixture(golden_lists, list_k, top_m):
    X, W, lists = golden_lists
    ids, _, counts = lists[list_k]
    want = host_model(X, W, np.arange(1200), ids, counts, top_m)
    assert 3 < want[2].max() <= 32                                       # top_m = 32 exceeds it: whole lists are compared
    assert_same(run_op(X, W, None, ids, counts, list_k, top_m), want, f"k={list_k} m={top_m}")


def tie_case(seed=3, U=400, I=150):
    """Integer ratings 1..5 and a W drawn from four distinct values: products collide."""
    rng = np.random.default_rng(seed)
    X = sp.random(U, I, density=0.25, random_state=rng, format="csr", dtype=np.float32)
    X.data[:] = rng.integers(1, 6, X.nnz).astype(np.float32)
    W = sp.random(I, I, density=0.2, random_state=rng, format="csc", dtype=np.float32)
    W.data[:] = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), W.nnz)
    X.sort_indices(); W.sort_indices()
    ids = np.stack([rng.permutation(I)[:10] for _ in range(U)]).astype(np.int32)
    return X, W, ids, np.full(U, 10, np.int32)


@pytest.mark.parametrize("top_m", [3, 8])
def test_tied_contributions_go_to_the_lower_item_id(top_m):
    X, W, ids, counts = tie_case()
    want = host_model(X, W, np.arange(X.shape[0]), ids, counts, top_m)
    c = want[1]
    tied = ((c[:, :, 1:] == c[:, :, :-1]) & np.isfinite(c[:, :, 1:])).any(axis=2)
    assert tied.mean() >= 0.1, f"only {tied.mean():.3f} of the pairs have a tie among their first {top_m}"
    first = np.argmax((c[:, :, 1:] == c[:, :, :-1]) & np.isfinite(c[:, :, 1:]), axis=2)
    b, p = np.nonzero(tied)
    assert (want[0][b, p, first[b, p]] < want[0][b, p, first[b, p] + 1]).all()           # the model itself: lower id first
    assert_same(run_op(X, W, None, ids, counts, 10, top_m), want, "ties")


LENGTHS = [0, 1, 63, 64, 65, 130, 5000, 40000]


def length_case():
    """Rows and columns of every length in LENGTHS over a catalogue of 40,000 items: user r rates LENGTHS[r] items, column
    c of W stores LENGTHS[c] weights (the last one all n_items, a K=None column); signed values."""
    rng = np.random.default_rng(11)
    I = 40000
    n = len(LENGTHS)
    pool = lambda L: 200 if L <= 130 else I                              # short rows / columns share a small pool: they intersect
    xi = [np.sort(rng.choice(pool(L), L, replace=False)) for L in LENGTHS]
    X = sp.csr_matrix((rng.standard_normal(sum(LENGTHS)).astype(np.float32), np.concatenate(xi), np.cumsum([0] + LENGTHS)), shape=(n, I))
    wi = [np.sort(rng.choice(pool(L), L, replace=False)) for L in LENGTHS]
    wptr = np.zeros(I + 1, np.int64)
    wptr[1:n + 1] = np.cumsum(LENGTHS)
    wptr[n + 1:] = wptr[n]
    W = sp.csc_matrix((rng.standard_normal(sum(LENGTHS)).astype(np.float32), np.concatenate(wi), wptr), shape=(I, I))
    return X, W


@pytest.mark.parametrize("top_m", [1, 5, 32])
def test_rows_and_columns_of_every_length(top_m):
    X, W = length_case()
    n = len(LENGTHS)
    ids = np.tile(np.arange(n, dtype=np.int32), (n, 1))                  # every user x every special column
    counts = np.full(n, n, np.int32)
    want = host_model_vectorised(X, W, np.arange(n), ids, counts, top_m)
    assert want[2][n - 1, n - 1] == 40000 and want[2][n - 2, n - 1] == 5000 and want[2][1, n - 1] == 1 and (want[2][0] == 0).all()
    assert all(want[2][r, c] > 5 for r in range(2, 6) for c in range(2, 6)) and want[2][6, 6] > 32
    assert_same(run_op(X, W, None, ids, counts, n, top_m), want, f"lengths m={top_m}")
    small = host_model(X, W, np.arange(n), ids[:, :6], np.full(n, 6, np.int32), top_m)        # the definition itself where it is cheap
    assert_same(run_op(X, W, None, ids[:, :6].copy(), np.full(n, 6, np.int32), 6, top_m), small, "lengths, definition")


def test_row_ids_padding_holes_and_strides():
    X, W, _, _, _ = golden()
    rng = np.random.default_rng(2)
    n, I = 500, W.shape[1]
    rows = rng.integers(0, 1200, n).astype(np.int32)
    rows[[3, 50, 77]] = [-1, 1200, 2 ** 31 - 1]                          # users without a row
    ids = rng.integers(0, I, (n, 12)).astype(np.int32)                   # stride 12, list_k 10: the last two columns are not the list's
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[5, 2], ids[6, 0], ids[7, 9] = I, I + 1000, -5
    counts = rng.integers(-1, 13, n).astype(np.int32)                    # short lists, and counts the kernel has to clamp
    want = host_model(X, W, rows.astype(np.int64), ids[:, :10], np.clip(counts, 0, 10), 4)
    assert_same(run_op(X, W, rows, ids, counts, 10, 4), want, "row ids")
    assert (want[2][[3, 50, 77]] == 0).all() and want[2].max() > 4
    ident = host_model(X, W, np.arange(n), ids[:, :10], np.clip(counts, 0, 10), 4)
    assert_same(run_op(X[:n], W, None, ids, counts, 10, 4), ident, "identity rows")
    # no rows at all: nothing is launched, nothing is written
    empty = run_op(X, W, np.empty(0, np.int32), np.empty((0, 10), np.int32), np.empty(0, np.int32), 10, 4)
    assert empty[0].shape == (0, 10, 4) and empty[2].shape == (0, 10)


# ---------------------------------------------------------------------------------------------- the value edges
@pytest.fixture(scope="module")
def edges():
    return edge_case()


def differing_cases(got, want, cases):
    return sorted(k for k, (r, slot, _) in cases.items()
                  if not (np.array_equal(got[0][r, slot], want[0][r, slot]) and np.array_equal(bits(got[1][r, slot]), bits(want[1][r, slot]))
                          and got[2][r, slot] == want[2][r, slot]))


@pytest.mark.parametrize("top_m", EDGE_TOP_M)
def test_nan_inf_signed_zero_and_denormal_contributions_on_all_four_search_paths(edges, top_m):
    """tests/test_explain_host.py's edge_case: every value set through rows of 3 / 64 / 65 entries (search in registers / in
    memory) and columns of 3 / 64 / 65 / 130 entries (one probe / a probe per round, hits in all three probes).  A NaN
    contribution counts in support and is never a reason; +-inf are numbers; each zero keeps its sign bit; 2^-140 is kept."""
    X, W, rows, ids, counts, cases = edges
    want = host_model(X, W, rows, ids, counts, top_m)
    got = run_op(X, W, None, ids, counts, 4, top_m)
    bad = differing_cases(got, want, cases)
    print(f"top_m={top_m}: {len(bad)} of {len(cases)} cases differ: {bad}")
    assert not bad, f"top_m={top_m}: {len(bad)} of {len(cases)} cases differ from the definition: {bad}"
    assert_same(got, want, f"edges m={top_m}")
    assert not np.isnan(got[1]).any()                                    # under the rule no output holds a NaN
    back = np.arange(len(rows))[::-1].copy()                             # the same pairs through row ids, the last row first
    assert_same(run_op(X, W, back, ids[back], counts[back], 4, top_m), tuple(a[back] for a in want), f"edges by row id m={top_m}")


def test_engine_explain_rows_lists_infinite_contributions_as_numbers():
    from rtrec_amd.engine import SlimEngine
    rng = np.random.default_rng(31)
    U, I = 60, 48
    X = sp.random(U, I, density=0.4, random_state=rng, format="csr", dtype=np.float32)
    X.data[:] = rng.integers(1, 6, X.nnz).astype(np.float32)
    X.data[rng.choice(X.nnz, 40, replace=False)] = np.repeat(np.array([np.inf, -np.inf], np.float32), 20)     # infinite ratings
    W = sp.random(I, I, density=0.3, random_state=rng, format="csc", dtype=np.float32)
    W.data[:] = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0, 2.0], np.float32), W.nnz)
    X.sort_indices(); W.sort_indices()
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(X.tocsc(), X)
    eng.set_weights(W)
    ids = np.stack([rng.permutation(I)[:8] for _ in range(U)]).astype(np.int32)
    want = host_model(X, W, np.arange(U), ids, np.full(U, 8), 32)
    listed = want[0] >= 0
    assert (np.isposinf(want[1]) & listed).sum() > 10 and (np.isneginf(want[1]) & listed).sum() > 10      # -inf with an id: a reason, not padding
    got = eng.explain_rows(np.arange(U), ids, None, 32)
    assert_same(got, want, "engine, infinite ratings")
    assert not np.isnan(got[1]).any()


def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    op = torch.ops.rtrec_amd.explain_topk
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(list_k=2, top_m=2, **kw):
        a = dict(row_ids=None, xb_ptr=i32(4), xb_col=i32(5), xb_val=f32(5), wc_ptr=i32(7), wc_row=i32(3), wc_val=f32(3), ids=i32(3, list_k),
                 counts=i32(3), items=i32(3, list_k, top_m), contrib=f32(3, list_k, top_m), support=i32(3, list_k))
        a.update(kw)
        op(a["row_ids"], a["xb_ptr"], a["xb_col"], a["xb_val"], 6, a["wc_ptr"], a["wc_row"], a["wc_val"], a["ids"], a["counts"], list_k, top_m,
           a["items"], a["contrib"], a["support"])

    call()                                                               # the well-formed call runs
    call(list_k=64, top_m=32)
    for kw in (dict(list_k=0), dict(list_k=65), dict(top_m=0), dict(top_m=33)):
        with pytest.raises(RuntimeError, match="must lie in"):
            call(**kw)
    bad = [dict(ids=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(xb_val=torch.zeros(5, dtype=torch.float64, device=dev)),
           dict(wc_val=torch.zeros(3, dtype=torch.float16, device=dev)), dict(contrib=torch.zeros((3, 2, 2), dtype=torch.float64, device=dev)),
           dict(row_ids=torch.zeros(3, dtype=torch.int64, device=dev)), dict(counts=torch.zeros(3, dtype=torch.int32)),
           dict(items=torch.zeros((3, 2, 2), dtype=torch.int32)), dict(ids=i32(3, 4)[:, ::2]), dict(ids=i32(3, 1)), dict(counts=i32(2)),
           dict(support=i32(3, 3)), dict(wc_ptr=i32(6)), dict(xb_val=f32(4)), dict(row_ids=i32(2))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- end to end
def _golden_model(string_ids=False, **kw):
    from rtrec_amd import SLIM
    X, W, _, _, _ = golden()
    coo = X.tocoo()
    m = SLIM(min_value=-100, max_value=100, nn_feature_selection=50, **kw)
    ts = 1.7e9 + np.arange(coo.nnz, dtype=np.float64)
    if string_ids:
        m.add_interactions([(f"u{u}", f"i{i}", float(t), float(r)) for u, i, t, r in zip(coo.row.tolist(), coo.col.tolist(), ts.tolist(), coo.data.tolist())])
    else:
        m.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64), ts, coo.data.astype(np.float64))
    return m, X, W


def test_explain_batch_contributions_add_up_to_the_reported_scores():
    """A float32 model: for every pair of every user's top-10 the ordered float32 sum of explain_batch(top_m=32)'s contributions
    is the score of the same list entry, bit for bit."""
    m, X, W = _golden_model()
    m.model.item_similarity = W
    users = np.arange(1200)
    ids, counts, r_ids, contrib, support = m.explain_batch(users, top_k=10, top_m=32, as_arrays=True)
    Xm = m.interactions.to_csr()
    Xm.sort_indices()
    assert np.array_equal(Xm.indices, X.indices) and np.array_equal(bits(Xm.data), bits(X.data))
    e_ids, e_sc, e_cnt = m.model.engine.recommend_rows(users, top_k=10)
    assert np.array_equal(ids, e_ids) and np.array_equal(counts, e_cnt)
    live = np.arange(10)[None, :] < counts[:, None]
    assert (support[live] >= 1).all() and support.max() <= 32, "support <= 32 must cover every pair of the fixture"
    assert (support[~live] == 0).all()
    n = 0
    for b, p in zip(*np.nonzero(live)):
        s = support[b, p]
        order = np.argsort(r_ids[b, p, :s], kind="stable")               # back to ascending item order
        assert bits(ordered_sum(contrib[b, p, :s][order])) == bits(e_sc[b, p]), (b, p)
        assert (r_ids[b, p, s:] == -1).all() and np.isneginf(contrib[b, p, s:]).all()
        n += 1
    assert n == int(counts.sum()) and n > 11000
    # the list form, the given-lists form and the single-user form say the same
    got = m.explain_batch(users[:50].tolist(), top_k=10, top_m=3)
    assert got == m.explain_batch(users[:50].tolist(), items=[[i for i, _ in row] for row in got], top_m=3)
    assert got[7] == m.explain(7, top_k=10, top_m=3)
    want = host_model(X, W, users[:50], ids[:50], counts[:50], 3)
    for b, row in enumerate(got):
        assert [i for i, _ in row] == ids[b, :counts[b]].tolist()
        for p, (_, reasons) in enumerate(row):
            k = min(int(want[2][b, p]), 3)
            assert [j for j, _ in reasons] == want[0][b, p, :k].tolist()
            assert np.array_equal(bits([c for _, c in reasons]), bits(want[1][b, p, :k]))


def test_explain_batch_float64_w_and_dense_mode_equal_the_host_model():
    m, X, W = _golden_model()
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)         # the serial fit's dtype; the values are float32 numbers
    users = np.arange(1200)
    ids, counts, r_ids, contrib, support = m.explain_batch(users, top_k=10, top_m=5, as_arrays=True)
    assert m.model.engine.weights.f64 and not m.model.engine.weights.lossy
    e_ids, _, e_cnt = m.model.engine.recommend_rows(users, top_k=10)
    assert np.array_equal(ids, e_ids) and np.array_equal(counts, e_cnt)
    assert_same((r_ids, contrib, support), host_model(X, W, users, ids, counts, 5), "float64 W")
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.explain_batch(users[:5], top_k=10)
    # DENSE mode: string ids, a W fitted on the device in the model's own id order, zero-score items in the lists
    s, _, _ = _golden_model(string_ids=True)
    s.bulk_fit(parallel=True, progress_bar=False)
    names = [f"u{u}" for u in range(0, 1200, 3)] + ["nobody"]
    ids, counts, r_ids, contrib, support = s.explain_batch(names, top_k=12, top_m=4, as_arrays=True)
    recs = s.recommend_batch(names, top_k=12)
    assert [[s.item_ids.get(int(i)) for i in ids[b, :counts[b]]] for b in range(len(names))] == recs
    Xs, Ws = s.interactions.to_csr(), s.model.item_similarity.tocsc()
    Xs.sort_indices(); Ws.sort_indices()
    rows = np.array([s.user_ids.get_id(u) for u in names[:-1]] + [-1])
    assert_same((r_ids, contrib, support), host_model(Xs, Ws, rows, ids, counts, 4), "dense mode")
    assert (support[-1] == 0).all() and counts[-1] > 0 and support.max() > 4
    lists = s.explain_batch(names, top_k=12, top_m=4)
    assert [[i for i, _ in row] for row in lists] == recs
    assert all(isinstance(j, str) and isinstance(c, float) for row in lists for _, reasons in row for j, c in reasons)


# ---------------------------------------------------------------------------------------------- full size
C3S = dict(U=138_493, I=26_744, draws=46_000_000, K=50, gen="clustered", clusters=80, p_in=0.85)


def test_c3s_all_users_top10_equal_the_vectorised_host_model():
    """The structured MovieLens-20M shape (rows of more than 4,096 items included): every user's top-10 explained in one pass
    on lists that stay in HBM, all 1.38 M pairs against the scipy-vectorised host model: ids, contribution bits, support."""
    import torch
    from rtrec_amd.engine import SlimEngine, coefficients_to_updates, merge_coefficients
    from rtrec_amd.synth import workload_matrix
    U, I, K = C3S["U"], C3S["I"], C3S["K"]
    X = workload_matrix(C3S)
    Xc = X.tocsc()
    Xc.sort_indices()
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(Xc, X)
    W = merge_coefficients(None, I, *coefficients_to_updates(*eng.fit_columns(np.arange(I), nn_feature_selection=K)[:4]))
    W.sort_indices()
    eng.set_weights(W)
    d_rows = eng.be.to_dev(np.arange(U, dtype=np.int32))
    d_ids, d_sc, d_cnt = eng.score_topk_device(None, U, 10, True, _native.TOPK_SPARSE, d_rows=d_rows)
    out = eng.explain_device(d_rows, U, None, d_ids, d_cnt, 3)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in out)
    ids, counts, scores = d_ids.cpu().numpy(), d_cnt.cpu().numpy(), d_sc.cpu().numpy()
    assert np.diff(X.indptr).max() > 4096 and counts.min() >= 0
    t0 = time.perf_counter()
    want = host_model_vectorised(X, W, np.arange(U), ids, counts, 3, chunk=16384)
    print(f"host model, {U} users x 10: {time.perf_counter() - t0:.1f} s; support 1..{want[2].max()}, median "
          f"{int(np.median(want[2][want[2] > 0]))}")
    assert_same(got, want, "c3s")
    live = np.arange(10)[None, :] < counts[:, None]
    assert (want[2][live] >= 1).all() and live.sum() > 1_300_000
    # the invariant at full size: with top_m = 32 a pair of at most 32 contributing items is listed whole, and its ordered
    # float32 sum is the score of the list entry (a fixed-seed sample of 20,000 such pairs)
    items32, contrib32, support32 = (t.cpu().numpy() for t in eng.explain_device(d_rows, U, None, d_ids, d_cnt, 32))
    assert np.array_equal(support32, want[2]) and np.array_equal(items32[:, :, :3], got[0]) and np.array_equal(bits(contrib32[:, :, :3]), bits(got[1]))
    b, p = np.nonzero(live & (support32 <= 32))
    assert len(b) > 500_000
    sel = np.random.default_rng(1).choice(len(b), 20000, replace=False)
    for bb, pp in zip(b[sel], p[sel]):
        s = support32[bb, pp]
        order = np.argsort(items32[bb, pp, :s], kind="stable")
        assert bits(ordered_sum(contrib32[bb, pp, :s][order])) == bits(scores[bb, pp]), (bb, pp)
    del eng
    torch.cuda.empty_cache()
