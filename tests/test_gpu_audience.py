"""audience_tile_kernel / audience_merge_kernel (csrc/audience.hip) on the GPU against the host model of
tests/test_audience_host.py -- `==` on user ids, score bits, counts and eligible for every slot -- and SLIM.recommend_users_batch
end to end: the score an audience lists for a (user, item) pair is, bit for bit, the score the forward candidates path reports."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from rtrec_amd import ops as _ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
from tests.test_audience_host import EDGE_TOP_N, edge_case, golden_csc, host_model
from tests.test_explain_host import bits

pytestmark = pytest.mark.gpu


def run_op(Xc, W, items, top_n, filter_interacted=True, mask=None, ws_bytes=None, ws_out=None):
    """torch.ops.rtrec_amd.audience_topk on host matrices: Xc / W csc (sorted), mask a bool array over the users or None.  The
    outputs are poisoned first: every slot must be written."""
    import torch
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")
    U, n = Xc.shape[0], len(items)
    users = torch.full((n, top_n), 12345, dtype=torch.int32, device="cuda:0")
    scores = torch.full((n, top_n), 7.0, dtype=torch.float32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    eligible = torch.full((n,), -9, dtype=torch.int32, device="cuda:0")
    d_mask = None
    if mask is not None:
        padded = np.zeros(((U + 31) // 32) * 32, np.uint8)
        padded[:U] = mask
        d_mask = up(np.packbits(padded, bitorder="little").view(np.int32), np.int32)
    if ws_bytes is None:
        ws_bytes = max(int(_native.load().rtrec_slim_audience_workspace_bytes(U, max(n, 1), top_n)), 8)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.ops.rtrec_amd.audience_topk(up(items, np.int32), U, up(Xc.indptr, np.int32), up(Xc.indices, np.int32), up(Xc.data, np.float32),
                                      up(W.indptr, np.int32), up(W.indices, np.int32), up(W.data, np.float32), top_n, bool(filter_interacted),
                                      d_mask, users, scores, count, eligible, ws)
    torch.cuda.synchronize()
    if ws_out is not None:
        ws_out.append(ws.cpu().numpy())
    return users.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), eligible.cpu().numpy()


def assert_same(got, want, what=""):
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (bits(got[1]) != bits(want[1])).any(axis=1) | (got[2] != want[2]) | (got[3] != want[3]))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want[2])} query items differ from the host model, first {int(bad[0])}: "
                           f"count {got[2][bad[0]]} / {want[2][bad[0]]}, eligible {got[3][bad[0]]} / {want[3][bad[0]]}")


def prefix(want, top_n):
    """The host model's answer for a smaller top_n: the order is a prefix of the longer one."""
    return want[0][:, :top_n], want[1][:, :top_n], np.minimum(want[2], top_n).astype(np.int32), want[3]


# ---------------------------------------------------------------------------------------------- 1. the golden fixture
@pytest.fixture(scope="module")
def golden_want():
    """The host model on all 400 items at top_n = 1024, per (filter, mask)."""
    _, Xc, W, _, _, _ = golden_csc()
    assert Xc.shape == (1200, 400)
    mask = np.random.default_rng(17).random(1200) < 0.5
    want = {(f, m): host_model(Xc, W, np.arange(400), 1024, f, mask if m else None) for f in (True, False) for m in (False, True)}
    el = want[(True, False)][3]
    assert el.min() == 226 and el.max() == 1164
    return Xc, W, mask, want


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("filter_interacted", [True, False])
@pytest.mark.parametrize("top_n", [1, 10, 1024])
def test_op_equals_the_definition_on_the_golden_fixture(golden_want, top_n, filter_interacted, masked):
    Xc, W, mask, want = golden_want
    got = run_op(Xc, W, np.arange(400), top_n, filter_interacted, mask if masked else None)
    assert_same(got, prefix(want[(filter_interacted, masked)], top_n), f"golden n={top_n} filter={filter_interacted} mask={masked}")
    live = np.arange(top_n)[None, :] < got[2][:, None]
    assert (got[0][~live] == -1).all() and np.isneginf(got[1][~live]).all()


# ---------------------------------------------------------------------------------------------- 2. ties
def tie_case(seed=3, U=4000, I=150):
    """Integer ratings 1..5 and a W drawn from six signed values: scores collide, cancel to exactly 0 and go negative."""
    rng = np.random.default_rng(seed)
    X = sp.random(U, I, density=0.25, random_state=rng, format="csr", dtype=np.float32)
    X.data[:] = rng.integers(1, 6, X.nnz).astype(np.float32)
    W = sp.random(I, I, density=0.2, random_state=rng, format="csc", dtype=np.float32)
    W.data[:] = rng.choice(np.array([-1.0, -0.5, 0.25, 0.5, 1.0, 2.0], np.float32), W.nnz)
    Xc = X.tocsc()
    Xc.sort_indices(); W.sort_indices()
    return Xc, W


def test_ties_at_the_boundary_go_to_the_lower_user_row():
    Xc, W = tie_case()
    U, I = Xc.shape
    full = host_model(Xc, W, np.arange(I), U)                            # every eligible user, in order
    sc, el = full[1], full[3]
    assert (el > 1024).all()
    for top_n, share in ((10, 0.25), (100, 0.8), (1024, 0.8)):
        tied = sc[:, top_n - 1] == sc[:, top_n]                          # the cut runs through a group of equal scores
        print(f"top_n={top_n}: {int(tied.sum())} of {I} items have a tie at the boundary")
        assert tied.mean() >= share, f"only {tied.mean():.3f} of the items have a tie at the top_n={top_n} boundary"
    listed = np.arange(U)[None, :] < el[:, None]
    assert ((sc < 0) & listed).any(axis=1).all() and ((sc == 0) & listed).any(axis=1).all()     # negative and exactly-zero scores everywhere
    for top_n in (10, 100, 1024):
        for f in (True, False):
            want = prefix(full, top_n) if f else host_model(Xc, W, np.arange(I), top_n, False)
            assert_same(run_op(Xc, W, np.arange(I), top_n, f), want, f"ties n={top_n} filter={f}")


# ---------------------------------------------------------------------------------------------- 2b. the value edges
@pytest.fixture(scope="module", params=[False, True], ids=["one_tile", "two_tiles"])
def edges(request):
    return edge_case(request.param)


@pytest.mark.parametrize("top_n", EDGE_TOP_N)
def test_nan_inf_signed_zero_and_denormal_scores(edges, top_n):
    """tests/test_audience_host.py's edge_case, every score set through a column of W of 3 and of 60 entries: a NaN score counts
    in eligible and is never listed, however it was made and whatever its sign bit; +-inf are numbers and tie by row across
    the tile boundary; -0.0 alone in its sum scores +0.0; denormal sums keep their place.  Then with the filter and the
    candidate set removing NaN users, and through a workspace that holds one query item per pass."""
    Xc, W, items, mask, cases = edges
    one = int(_native.load().rtrec_slim_audience_workspace_bytes(Xc.shape[0], 1, top_n))
    for what, f, m, ws_bytes in (("no filter", False, None, None), ("filter", True, None, None), ("candidates", False, mask, None),
                                 ("filter and candidates", True, mask, None), ("one item per pass", True, None, one)):
        want = host_model(Xc, W, items, top_n, f, m)
        got = run_op(Xc, W, items, top_n, f, m, ws_bytes=ws_bytes)
        bad = sorted((name, L) for name, (q3, q60, _) in cases.items() for L, q in ((3, q3), (60, q60))
                     for b in np.flatnonzero(items == q)
                     if not (np.array_equal(got[0][b], want[0][b]) and np.array_equal(bits(got[1][b]), bits(want[1][b]))
                             and got[2][b] == want[2][b] and got[3][b] == want[3][b]))
        print(f"top_n={top_n}, {what}: {len(bad)} of {len(items)} query items differ: {bad}")
        assert not bad, f"top_n={top_n}, {what}: these (score set, column length) differ from the definition: {bad}"
        assert_same(got, want, f"edges n={top_n} {what}")
        assert not np.isnan(got[1]).any()                                # under the rule no output holds a NaN
    assert (want[3] > want[2]).any() and (want[2] < min(top_n, 3)).any()


def test_engine_audience_items_counts_but_never_lists_a_nan_score_from_infinite_ratings():
    from rtrec_amd.engine import SlimEngine
    rng = np.random.default_rng(37)
    U, I = 9000, 48                                                      # two tiles
    X = sp.random(U, I, density=0.3, random_state=rng, format="csr", dtype=np.float32)
    X.data[:] = rng.integers(1, 6, X.nnz).astype(np.float32)
    X.data[rng.choice(X.nnz, 4000, replace=False)] = np.repeat(np.array([np.inf, -np.inf], np.float32), 2000)   # infinite ratings
    W = sp.random(I, I, density=0.3, random_state=rng, format="csc", dtype=np.float32)
    W.data[:] = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0, 2.0], np.float32), W.nnz)
    Xc = X.tocsc()
    Xc.sort_indices(); X.sort_indices(); W.sort_indices()
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(Xc, X)
    eng.set_weights(W)
    for top_n, f in ((1, True), (40, True), (1024, False)):
        want = host_model(Xc, W, np.arange(I), top_n, f)
        got = eng.audience_items(np.arange(I), top_n, f)
        assert_same(got, want, f"engine, infinite ratings n={top_n}")
        assert not np.isnan(got[1]).any()
    cand = np.zeros(U, bool)                                             # 1,000 candidates around the tile boundary: whole audiences fit
    cand[7700:8700] = True                                               # into top_n, so a listed NaN could not hide behind the cut
    want = host_model(Xc, W, np.arange(I), 1024, False, cand)
    got = eng.audience_items(np.arange(I), 1024, False, candidate_rows=np.flatnonzero(cand))
    assert_same(got, want, "engine, infinite ratings, candidates")
    assert not np.isnan(got[1]).any() and (want[3] < 1024).all() and (want[2] < want[3]).sum() > I // 2
    full = host_model(Xc, W, np.arange(I), U, False)
    assert ((full[3] - full[2]) > 10).sum() > I // 2                     # inf - inf happened: NaN scores, eligible and not listed
    assert np.isposinf(full[1][:, 1]).sum() > I // 2 and np.isneginf(full[1][np.arange(I), full[2] - 1]).sum() > I // 2   # inf ties at both ends


# ---------------------------------------------------------------------------------------------- 3. lengths
X_LENGTHS = [0, 1, 63, 64, 65, 5000, None]      # None: all U
W_LENGTHS = [0, 1, 50, 65, None]                # None: all items


def length_case(U=300_000, I=400):
    """300,000 users (37 tiles, rows beyond 2^16): X columns 0..6 have the lengths of X_LENGTHS, the others 200 entries each;
    the query columns 0..4 of W have the lengths of W_LENGTHS, each starting with X's special columns; signed values."""
    rng = np.random.default_rng(11)
    x_len = [U if L is None else L for L in X_LENGTHS] + [200] * (I - len(X_LENGTHS))
    rows = [np.sort(rng.choice(U, L, replace=False)) if L < U else np.arange(U) for L in x_len]
    ptr = np.zeros(I + 1, np.int64)
    ptr[1:] = np.cumsum(x_len)
    Xc = sp.csc_matrix((rng.standard_normal(int(ptr[-1])).astype(np.float32), np.concatenate(rows).astype(np.int32), ptr), shape=(U, I))
    w_len = [I if L is None else L for L in W_LENGTHS]
    w_rows = [np.arange(L) if L >= 7 or L == 0 else np.array([6]) for L in w_len]          # the single entry: the all-U column
    wptr = np.zeros(I + 1, np.int64)
    wptr[1:len(w_len) + 1] = np.cumsum(w_len)
    wptr[len(w_len) + 1:] = wptr[len(w_len)]
    W = sp.csc_matrix((rng.standard_normal(sum(w_len)).astype(np.float32), np.concatenate(w_rows).astype(np.int32), wptr), shape=(I, I))
    return Xc, W


@pytest.mark.parametrize("top_n", [1, 1024])
def test_columns_of_every_length_over_300000_users(top_n):
    Xc, W = length_case()
    U = Xc.shape[0]
    assert U >= 300_000 and np.diff(Xc.indptr)[:7].tolist() == [0, 1, 63, 64, 65, 5000, U]
    assert np.diff(W.indptr)[:5].tolist() == [0, 1, 50, 65, 400] and (W.data < 0).any() and (Xc.data < 0).any()
    items = np.arange(8)                                                 # the five special columns and three empty ones
    for f, mask in ((True, None), (False, None), (True, np.random.default_rng(5).random(U) < 0.5)):
        want = host_model(Xc, W, items, top_n, f, mask)
        if mask is None:
            assert want[3][1] >= U - 1 and (want[3][2:5] >= U - 65).all() and (want[3][5:] == 0).all()
        assert_same(run_op(Xc, W, items, top_n, f, mask), want, f"lengths n={top_n} filter={f} mask={mask is not None}")


# ---------------------------------------------------------------------------------------------- 4. bad input
def test_query_ids_outside_the_catalogue_duplicates_and_an_empty_list():
    _, Xc, W, _, _, _ = golden_csc()
    items = np.array([5, -1, 400, 2 ** 31 - 1, 5, 17, 5, -2 ** 31], dtype=np.int64).astype(np.int32)
    want = host_model(Xc, W, items, 20)
    got = run_op(Xc, W, items, 20)
    assert_same(got, want, "odd ids")
    assert got[2].tolist()[1:4] == [0, 0, 0] and got[3].tolist()[1:4] == [0, 0, 0] and got[2][7] == 0
    assert np.array_equal(got[0][0], got[0][4]) and np.array_equal(got[0][0], got[0][6]) and got[2][0] == 20
    ws = []                                                              # an empty list: nothing is launched, so the workspace
    empty = run_op(Xc, W, np.empty(0, np.int32), 20, ws_bytes=4096, ws_out=ws)      # keeps the pattern it was filled with
    assert empty[0].shape == (0, 20) and empty[1].shape == (0, 20) and empty[2].shape == (0,) and empty[3].shape == (0,)
    assert ws[0].shape == (4096,) and (ws[0] == 0xA5).all()
    ws = []
    run_op(Xc, W, items[:1], 20, ws_bytes=4096, ws_out=ws)               # the same workspace IS written by a call with one item
    assert (ws[0] != 0xA5).any()


@pytest.mark.parametrize("case", ["golden", "lengths"])
def test_a_small_workspace_is_worked_through_in_passes(case):
    """A workspace of one or two query items' worth for ten or eleven items: the entry point reuses it pass after pass and
    every pass writes its own slice of the outputs."""
    if case == "golden":
        _, Xc, W, _, _, _ = golden_csc()
        items = np.array([7, 399, 7, -1, 120, 33, 400, 250, 8, 9, 310], np.int32)
    else:
        Xc, W = length_case()
        items = np.array([4, 2, 3, 1, 0, 4, 7, 2, -1, 3], np.int32)
    size = _native.load().rtrec_slim_audience_workspace_bytes
    for top_n in (1, 10, 1024):
        one = int(size(Xc.shape[0], 1, top_n))
        assert int(size(Xc.shape[0], len(items), top_n)) == len(items) * one
        want = host_model(Xc, W, items, top_n)
        for ws_bytes in (one, 2 * one, 3 * one - 1):                     # 1, 2 and 2 items a pass (the odd item last)
            assert_same(run_op(Xc, W, items, top_n, ws_bytes=ws_bytes), want, f"{case} n={top_n} ws={ws_bytes}")


def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    op = torch.ops.rtrec_amd.audience_topk
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(top_n=2, n_users=40, **kw):
        a = dict(items=i32(3), xc_ptr=i32(7), xc_row=i32(5), xc_val=f32(5), wc_ptr=i32(7), wc_row=i32(3), wc_val=f32(3), user_mask=None,
                 users=i32(3, top_n), scores=f32(3, top_n), count=i32(3), eligible=i32(3),
                 ws=torch.zeros(1 << 16, dtype=torch.uint8, device=dev))
        a.update(kw)
        op(a["items"], n_users, a["xc_ptr"], a["xc_row"], a["xc_val"], a["wc_ptr"], a["wc_row"], a["wc_val"], top_n, True, a["user_mask"],
           a["users"], a["scores"], a["count"], a["eligible"], a["ws"])

    call()                                                               # the well-formed call runs
    call(top_n=1024, ws=torch.zeros(3 * (1024 * 8 + 8), dtype=torch.uint8, device=dev))
    call(user_mask=i32(2))
    for kw in (dict(top_n=0), dict(top_n=1025)):
        with pytest.raises(RuntimeError, match="must lie in"):
            call(**kw)
    with pytest.raises(RuntimeError, match="workspace too small"):
        call(ws=torch.zeros(16, dtype=torch.uint8, device=dev))
    bad = [dict(items=torch.zeros(3, dtype=torch.int64, device=dev)), dict(xc_val=torch.zeros(5, dtype=torch.float64, device=dev)),
           dict(wc_val=torch.zeros(3, dtype=torch.float16, device=dev)), dict(scores=torch.zeros((3, 2), dtype=torch.float64, device=dev)),
           dict(user_mask=torch.zeros(2, dtype=torch.int64, device=dev)), dict(count=torch.zeros(3, dtype=torch.int32)),
           dict(users=torch.zeros((3, 2), dtype=torch.int32)), dict(items=i32(6)[::2]), dict(users=i32(3, 4)[:, ::2]), dict(users=i32(3, 1)),
           dict(count=i32(2)), dict(eligible=i32(4)), dict(xc_ptr=i32(6)), dict(xc_val=f32(4)), dict(wc_row=i32(4)), dict(user_mask=i32(3)),
           dict(items=i32(3, 1)), dict(n_users=-1), dict(ws=torch.zeros(1 << 16, dtype=torch.uint8))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. the invariant, end to end
def _golden_model(string_ids=False, **kw):
    from rtrec_amd import SLIM
    X, _, W, _, _, _ = golden_csc()
    coo = X.tocoo()
    m = SLIM(min_value=-100, max_value=100, nn_feature_selection=50, **kw)
    ts = 1.7e9 + np.arange(coo.nnz, dtype=np.float64)
    if string_ids:
        m.add_interactions([(f"u{u}", f"i{i}", float(t), float(r)) for u, i, t, r in zip(coo.row.tolist(), coo.col.tolist(), ts.tolist(), coo.data.tolist())])
    else:
        m.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64), ts, coo.data.astype(np.float64))
    return m, X, W


def forward_scores(eng, users, cands):
    """{(user, item): score} from the existing candidates path: every user of `users` against the items `cands`."""
    ids, sc, cnt = eng.recommend_rows(users, top_k=len(cands), filter_interacted=False, mode=_native.TOPK_CANDIDATES,
                                      candidates=np.asarray(cands))
    return ids, sc, cnt


def assert_invariant(eng, items, a_users, a_scores, a_counts):
    """Every (user, item) pair the audiences list: the audience score is the forward score of the pair, bit for bit."""
    listed = np.unique(np.concatenate([a_users[b, :a_counts[b]] for b in range(len(items))] + [np.empty(0, np.int32)]))
    assert len(listed) > 0
    ids, sc, cnt = forward_scores(eng, listed, items)
    n = 0
    for b, i in enumerate(items):
        rows = np.searchsorted(listed, a_users[b, :a_counts[b]])
        hit = ids[rows] == i                                              # where the forward list of each listed user holds item i
        hit &= np.arange(ids.shape[1])[None, :] < cnt[rows][:, None]
        assert (hit.sum(axis=1) == 1).all(), f"item {i}: a listed user's forward list does not hold the item exactly once"
        fwd = sc[rows][hit]
        assert np.array_equal(bits(fwd), bits(a_scores[b, :a_counts[b]])), f"item {i}"
        n += len(rows)
    return n


def test_audience_scores_are_the_forward_kernels_scores_bit_for_bit():
    m, X, W = _golden_model()
    m.model.item_similarity = W
    items = np.random.default_rng(4).choice(400, 32, replace=False)
    items.sort()
    for f in (True, False):
        users, scores, counts, eligible = m.recommend_users_batch(items.tolist(), top_n=200, filter_interacted=f, as_arrays=True)
        Xc = X.tocsc()
        Xc.sort_indices()
        assert_same((users, scores, counts, eligible), host_model(Xc, W, items, 200, f), f"SLIM filter={f}")
        assert assert_invariant(m.model.engine, items.tolist(), users, scores, counts) == int(counts.sum()) > 6000
    # the list forms say the same
    lists = m.recommend_users_batch(items.tolist(), top_n=200, filter_interacted=False, ret_scores=True)
    for b in range(32):
        assert [u for u, _ in lists[b]] == users[b, :counts[b]].tolist() and np.array_equal(bits([s for _, s in lists[b]]), bits(scores[b, :counts[b]]))
    assert m.recommend_users(int(items[3]), top_n=200, filter_interacted=False, ret_scores=True) == lists[3]
    # candidate users through the bitmap
    cands = list(range(0, 1200, 3))
    mask = np.zeros(1200, bool)
    mask[cands] = True
    got = m.recommend_users_batch(items.tolist(), top_n=50, candidate_users=cands + [10 ** 7], as_arrays=True)
    assert_same(got, host_model(Xc, W, items, 50, True, mask), "SLIM candidates")


def test_string_ids_float64_w_and_lossy_w():
    m, X, W = _golden_model()
    Xc = X.tocsc()
    Xc.sort_indices()
    m.model.item_similarity = sp.csc_matrix(W, dtype=np.float64)         # the serial fit's dtype; the values are float32 numbers
    items = list(range(0, 400, 7))
    got = m.recommend_users_batch(items, top_n=64, as_arrays=True)
    assert m.model.engine.weights.f64 and not m.model.engine.weights.lossy
    assert_same(got, host_model(Xc, W, items, 64), "float64 W")           # the float32 model's scores
    lossy = sp.csc_matrix(W, dtype=np.float64)
    lossy.data[:] = lossy.data * (1.0 + 2.0 ** -40)
    m.model.item_similarity = lossy
    with pytest.raises(ValueError, match="not float32 numbers"):
        m.recommend_users_batch(items, top_n=64)
    # string ids end to end: a W fitted on the device in the model's own id order, raw user ids out
    s, _, _ = _golden_model(string_ids=True)
    s.bulk_fit(parallel=True, progress_bar=False)
    names = [f"i{i}" for i in range(0, 400, 9)] + ["never seen"]
    users, scores, counts, eligible = s.recommend_users_batch(names, top_n=30, as_arrays=True)
    Xs, Ws = s.interactions.to_csc(), s.model.item_similarity.tocsc()
    Xs.sort_indices(); Ws.sort_indices()
    q = [s.item_ids.get_id(n) for n in names[:-1]] + [-1]
    assert_same((users, scores, counts, eligible), host_model(Xs, Ws, q, 30), "string ids")
    lists = s.recommend_users_batch(names, top_n=30, ret_scores=True)
    assert lists[-1] == [] and counts[-1] == 0 and counts[:-1].min() > 0
    for b in range(len(names)):
        assert lists[b] == [(s.user_ids.get(int(u)), float(v)) for u, v in zip(users[b, :counts[b]], scores[b, :counts[b]])]
    assert all(isinstance(u, str) and u.startswith("u") for row in lists for u, _ in row)
    assert_invariant(s.model.engine, q[:-1], users[:-1], scores[:-1], counts[:-1])


# ---------------------------------------------------------------------------------------------- 6. full size
C3S = dict(U=138_493, I=26_744, draws=46_000_000, K=50, gen="clustered", clusters=80, p_in=0.85)


def test_c3s_256_items_equal_the_host_model_and_the_forward_scores():
    """The structured MovieLens-20M shape with all 138,493 users resident: the 64 query items with the most work (the sum over
    W[:, i]'s rows of nnz(X[:, j])), the 64 with the least non-zero work and 128 drawn with a fixed seed, at top_n = 10 and
    1024 against the host model; then the invariant on all listed users, one forward candidates call per 64 items."""
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
    col_nnz = np.diff(Xc.indptr).astype(np.int64)
    pattern = sp.csc_matrix((np.ones(W.nnz, np.int64), W.indices, W.indptr), shape=W.shape)
    work = np.asarray(pattern.T @ col_nnz).ravel()
    order = np.argsort(-work, kind="stable")
    nonzero = order[work[order] > 0]
    heavy, light = nonzero[:64], nonzero[-64:][::-1]
    rest = np.setdiff1d(np.arange(I), np.concatenate([heavy, light]))
    drawn = np.random.default_rng(20).choice(rest, 128, replace=False)
    items = np.concatenate([heavy, light, drawn]).astype(np.int32)
    assert len(np.unique(items)) == 256
    t0 = time.perf_counter()
    want = host_model(Xc, W, items, 1024)
    print(f"host model, 256 items x {U} users: {time.perf_counter() - t0:.1f} s; work {work[items].min()}..{work[items].max()}, "
          f"eligible {want[3].min()}..{want[3].max()}")
    assert want[3].max() > 100_000 and (want[3] < 10).any() and (want[3] > 1024).sum() > 64      # not a trivial sample
    up = eng.be.to_dev
    got = {}
    for top_n in (10, 1024):
        out = eng.audience_device(up(items), 256, top_n, True)
        torch.cuda.synchronize()
        got[top_n] = tuple(t.cpu().numpy() for t in out)
        assert_same(got[top_n], prefix(want, top_n), f"c3s n={top_n}")
    nof = tuple(t.cpu().numpy() for t in eng.audience_device(up(items), 256, 1024, False))
    assert_same(nof, host_model(Xc, W, items, 1024, False), "c3s unfiltered")
    users, scores, counts, _ = got[1024]
    n = 0
    for g in range(0, 256, 64):
        n += assert_invariant(eng, items[g:g + 64].tolist(), users[g:g + 64], scores[g:g + 64], counts[g:g + 64])
    assert n == int(counts.sum()) > 64 * 1024
    del eng
    torch.cuda.empty_cache()
