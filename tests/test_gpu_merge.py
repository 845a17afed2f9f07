"""The cross-shard list merge (merge_topk_kernel through rtrec_slim_merge_topk / rtrec_slim_merge_topk_strided) and the
cross-shard tie key (rtrec_slim_first_touch_aux) against plain numpy models of their contracts in include/rtrec_amd.h,
at every slot-count variant of the kernel (NS = 1, 2, 4, 16: n_lists * top_k up to 64, 128, 256, 1024), for float32 and
float64 scores, through the contiguous ABI and through the strided views of the exchange's record buffer.

Bar: ids, score bits and counts equal the model's.  The inputs stay inside the documented precondition of the merge (ids
distinct across the lists of a row, no NaN score).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
# ties dominate: ten levels, among them both zeros, a float32 denormal, the largest float and a VALID -inf
SCORE_POOL = np.array([0.0, -0.0, 1e-40, -1.5, -3.0, 0.5, 1.0, 2.75, FLT_MAX, -np.inf], dtype=np.float32)
# doubles that round to a float32 of the pool without being equal to it (or to each other): their order follows the double
SCORE_POOL_F64 = np.concatenate([SCORE_POOL.astype(np.float64),
                                 [1.0 + 2.0 ** -30, 1.0 - 2.0 ** -31, 2.75 + 2.0 ** -28, 0.5 - 2.0 ** -40, -1.5 - 2.0 ** -30,
                                  -1.5 + 2.0 ** -30]])
AUX_POOL = np.array([0, 1, 7, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32)    # a signed comparison misorders these
SENTINEL_ID, SENTINEL_CNT, SENTINEL_SCORE = -777, -555, 12345.5
RTREC_OK, RTREC_ERR_INVALID_ARG, RTREC_ERR_UNSUPPORTED = 0, -1, -2          # include/rtrec_amd.h

# (n_lists, top_k): every variant of launch_merge_topk and both sides of each of its cuts (64, 128, 256)
MERGE_CASES = [(1, 1), (2, 10), (8, 8),                   # NS = 1
               (5, 13), (8, 10), (8, 16),                 # NS = 2
               (3, 43), (4, 64),                          # NS = 4
               (8, 33), (8, 50), (16, 64), (1, 1024)]     # NS = 16


def variant(n_lists, top_k):
    total = n_lists * top_k
    return 1 if total <= 64 else 2 if total <= 128 else 4 if total <= 256 else 16


def case_id(n_lists, top_k):
    return f"{n_lists}x{top_k}={n_lists * top_k}-NS{variant(n_lists, top_k)}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _order(score, aux, ids):
    """Indices by score descending, then aux descending as unsigned 32-bit, then id descending."""
    return np.lexsort((-ids.astype(np.int64), -aux.astype(np.uint32).astype(np.int64), -score.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def make_lists(n_lists, top_k, f64, n_rows=257, pad_rows=0):
    """Seeded lists [n_lists, n_rows, top_k]: (ids int32, scores float32, scores float64 or None, aux uint32, counts).
    Rows 0.. are special: 0 every list empty, 1 every list full, 2 and 3 only the last list has entries (3: full); the last
    `pad_rows` rows are the all-zero records with count 0 that the exchange pads a chunk with.  Every slot at or beyond a
    list's count is poison (score +inf, aux 0xffffffff, a plausible id): a merge that reads past the count fails.  The valid
    prefix of a list is in the merge's own order, as a shard's list is."""
    L, R, K = n_lists, n_rows, top_k
    rng = np.random.default_rng([L, K, int(f64), R])
    sc64 = rng.choice(SCORE_POOL_F64 if f64 else SCORE_POOL.astype(np.float64), (L, R, K))
    aux = rng.choice(AUX_POOL, (L, R, K))
    # ids: distinct within a row across all lists, half of them just below 2**31
    span = max(2 * L * K, 64)
    ids = np.empty((L, R, K), dtype=np.int64)
    for r in range(R):
        p = rng.permutation(span)[:L * K]
        if r == 1 and span - 1 not in p:
            p[0] = span - 1                       # the full row holds id 2**31 - 1
        ids[:, r, :] = np.where(p < span // 2, p, 2 ** 31 - span + p).reshape(L, K)
    cnt = rng.integers(0, K + 1, (L, R)).astype(np.int32)
    cnt[:, 0] = 0
    cnt[:, 1] = K
    cnt[:, 2:4] = 0
    cnt[L - 1, 2], cnt[L - 1, 3] = (K + 1) // 2, K
    if pad_rows == 0:
        cnt[:, R - 1] = K                         # ... and the last row is full as well
    for l in range(L):
        for r in range(R):
            c = cnt[l, r]
            o = _order(sc64[l, r, :c], aux[l, r, :c], ids[l, r, :c])
            sc64[l, r, :c], aux[l, r, :c], ids[l, r, :c] = sc64[l, r, :c][o], aux[l, r, :c][o], ids[l, r, :c][o]
    beyond = np.arange(K)[None, None, :] >= cnt[:, :, None]
    sc64[beyond] = np.inf
    aux[beyond] = 0xffffffff
    if pad_rows:
        cnt[:, R - pad_rows:] = 0
        sc64[:, R - pad_rows:], aux[:, R - pad_rows:], ids[:, R - pad_rows:] = 0.0, 0, 0
    assert ids.max() == 2 ** 31 - 1 or L * K == 1
    out = (ids.astype(np.int32), sc64.astype(np.float32), sc64 if f64 else None, aux.astype(np.uint32), cnt)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def merge_model(ids, sc, sc64, aux, cnt, top_k):
    """The contract of rtrec_slim_merge_topk in numpy: per row the first count[l, row] entries of every list, ordered by score
    descending (the doubles when given), then aux descending as unsigned 32-bit, then id descending; the leading top_k, padded
    with id -1 / score -inf; count = min(valid, top_k); the returned score is float32(double) when doubles are given."""
    L, R, K = ids.shape
    key = sc64 if sc64 is not None else sc
    o_ids = np.full((R, top_k), -1, dtype=np.int32)
    o_sc = np.full((R, top_k), -np.inf, dtype=np.float32)
    o_cnt = np.zeros(R, dtype=np.int32)
    for r in range(R):
        valid = np.arange(K)[None, :] < cnt[:, r, None]                   # [L, K]
        c_id, c_key, c_aux = ids[:, r, :][valid], key[:, r, :][valid], aux[:, r, :][valid]
        o = _order(c_key, c_aux, c_id)[:top_k]
        o_cnt[r] = len(o)
        o_ids[r, :len(o)] = c_id[o]
        o_sc[r, :len(o)] = c_key[o].astype(np.float32)
    return o_ids, o_sc, o_cnt


@functools.lru_cache(maxsize=None)
def expected(n_lists, top_k, f64, n_rows=257, pad_rows=0):
    ids, sc, sc64, aux, cnt = make_lists(n_lists, top_k, f64, n_rows, pad_rows)
    return merge_model(ids, sc, sc64, aux, cnt, top_k)


def assert_lists_equal(got, want, what):
    (g_ids, g_sc, g_cnt), (w_ids, w_sc, w_cnt) = got, want
    assert np.array_equal(g_cnt, w_cnt), f"{what}: counts differ on rows {np.flatnonzero(g_cnt != w_cnt)[:8]}"
    bad = np.flatnonzero((g_ids != w_ids).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ on {bad.size} rows, first {bad[0]}: {g_ids[bad[0]]} vs {w_ids[bad[0]]}"
    bad = np.flatnonzero((bits(g_sc) != bits(w_sc)).any(axis=1))
    assert bad.size == 0, f"{what}: score bits differ on {bad.size} rows, first {bad[0]}: {g_sc[bad[0]]} vs {w_sc[bad[0]]}"
    # padding and count on every row (the model pads with -1 / -inf; said once more on the kernel's own output)
    k = g_ids.shape[1]
    pad = np.arange(k)[None, :] >= g_cnt[:, None]
    assert (g_ids[pad] == -1).all() and (bits(g_sc)[pad] == bits(np.float32(-np.inf))).all(), f"{what}: padding"
    assert (g_ids[~pad] >= 0).all(), f"{what}: an id inside the count is negative"


def dev(be, a):
    """A device copy of a shared (read-only) host array."""
    return be.to_dev(np.array(a))


def sentinel_outputs(be, n_rows, top_k):
    import torch
    return (torch.full((n_rows, top_k), SENTINEL_ID, dtype=torch.int32, device=be.device),
            torch.full((n_rows, top_k), SENTINEL_SCORE, dtype=torch.float32, device=be.device),
            torch.full((max(n_rows, 1),), SENTINEL_CNT, dtype=torch.int32, device=be.device))


def untouched(outs):
    o_ids, o_sc, o_cnt = (t.cpu().numpy() for t in outs)
    return (o_ids == SENTINEL_ID).all() and (o_sc == np.float32(SENTINEL_SCORE)).all() and (o_cnt == SENTINEL_CNT).all()


def merge_contiguous(be, lists, top_k, n_rows=None, n_lists=None):
    """rtrec_slim_merge_topk on contiguous [n_lists][n_rows][top_k] device copies of `lists`: (status, outputs on the host)."""
    ids, sc, sc64, aux, cnt = lists
    L, R, _ = ids.shape
    d = [dev(be, a) if a is not None else None for a in (ids, sc, sc64, aux.view(np.int32), cnt)]
    outs = sentinel_outputs(be, R, top_k)
    rc = be.lib.rtrec_slim_merge_topk(R if n_rows is None else n_rows, L if n_lists is None else n_lists, top_k, be.ptr(d[0]),
                                      be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]), be.ptr(d[4]), be.ptr(outs[0]), be.ptr(outs[1]),
                                      be.ptr(outs[2]), be.stream())
    be.synchronize()
    return rc, outs


# ---- (a) synthetic lists, contiguous ABI ------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n_lists,top_k", MERGE_CASES, ids=[case_id(*c) for c in MERGE_CASES])
def test_merge_contiguous_equals_model(engine, n_lists, top_k, f64):
    be = engine.be
    lists = make_lists(n_lists, top_k, f64)
    rc, outs = merge_contiguous(be, lists, top_k)
    assert rc == RTREC_OK
    got = tuple(t.cpu().numpy() for t in outs)
    assert_lists_equal(got, expected(n_lists, top_k, f64), case_id(n_lists, top_k))


def test_merge_slot_variants_are_all_reached():
    assert sorted({variant(*c) for c in MERGE_CASES}) == [1, 2, 4, 16]
    totals = sorted(l * k for l, k in MERGE_CASES)
    for cut in (64, 128, 256):          # both sides of every cut, and the largest supported merge
        assert cut in totals and any(cut < t <= cut + 8 for t in totals)
    assert totals[-1] == 1024


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_merge_argument_checks_leave_outputs_alone(engine, f64):
    be = engine.be
    lists = make_lists(5, 205, f64, 4)
    rc, outs = merge_contiguous(be, lists, 205, n_rows=0)
    assert rc == RTREC_OK and untouched(outs)
    rc, outs = merge_contiguous(be, lists, 205)                               # 5 x 205 = 1025 candidates
    assert rc == RTREC_ERR_UNSUPPORTED and untouched(outs)
    rc, outs = merge_contiguous(be, lists, 205, n_lists=0)
    assert rc == RTREC_ERR_INVALID_ARG and untouched(outs)
    rc, outs = merge_contiguous(be, make_lists(2, 10, f64, 4), 0)
    assert rc == RTREC_ERR_INVALID_ARG


# ---- (b) the same lists through the exchange's record layout -----------------------------------------------------------
POISON_WORD = 0x7f800000      # +inf as a float32 score, ~1e306 as half of a float64 one, a plausible id, a huge count


def record_buffer(be, lists, G, q, k, f64, list_perm=None):
    """`lists` written into a [G * q, width] int32 record buffer through the engine's own views (list l at position
    list_perm[l]); the pad word and a guard region on either side of the buffer hold poison.  The guards are long enough that a
    merge which confused any list stride with a row stride would still read poison, not memory outside the allocation."""
    import torch
    from rtrec_amd.engine import exchange_record_layout, exchange_record_views
    width = exchange_record_layout(k, f64)["width"]
    n, front = G * q * width, 2 * width
    back = (q + G) * q * width
    whole = torch.full((front + n + back,), POISON_WORD, dtype=torch.int32, device=be.device)
    recv = whole[front:front + n].view(G * q, width)
    views = exchange_record_views(torch, recv, G, q, k, f64)
    ids, sc, sc64, aux, cnt = lists
    perm = torch.as_tensor(np.arange(G) if list_perm is None else list_perm, device=be.device)
    for v, a in zip(views, (ids, sc, sc64, aux.view(np.int32), cnt)):
        if a is not None:
            v[perm] = dev(be, a)
    return whole, recv, views


EXCHANGE_Q = 37        # rows a rank merges: no multiple of 2, 3 or 8; the last three are the exchange's zero padding


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("G,k", [(G, k) for G in (2, 3, 8) for k in (10, 50)],
                         ids=[case_id(G, k) for G in (2, 3, 8) for k in (10, 50)])
def test_merge_record_views_equal_model_and_contiguous(engine, G, k, f64):
    from rtrec_amd.engine import exchange_record_layout
    be, q = engine.be, EXCHANGE_Q
    lists = make_lists(G, k, f64, q, 3)
    want = expected(G, k, f64, q, 3)
    # the views first: their buffer has guards, so a merge that mixed up two strides fails here, on poison, before anything else runs
    perms = [None] + ([np.roll(np.arange(G), 1)] if (G, k) in ((3, 50), (8, 10)) else [])
    results = []
    for perm in perms:
        whole, recv, views = record_buffer(be, lists, G, q, k, f64, perm)
        before = whole.clone()
        outs = sentinel_outputs(be, q, k)
        be.merge_topk(q, G, k, *views, *outs)
        be.synchronize()
        got = tuple(t.cpu().numpy() for t in outs)
        what = f"record views{'' if perm is None else ' (lists permuted)'}"
        assert_lists_equal(got, want, what)
        results.append((what, got))
        assert bool((whole == before).all()), "the merge wrote to its input buffer or the guards"
        L = exchange_record_layout(k, f64)
        if L["o_cnt"] + 1 < L["width"]:
            assert bool((recv[:, L["o_cnt"] + 1:] == POISON_WORD).all())      # the pad word was poison throughout
    rc, outs = merge_contiguous(be, lists, k)
    assert rc == RTREC_OK
    flat = tuple(t.cpu().numpy() for t in outs)
    assert_lists_equal(flat, want, "contiguous")
    for what, got in results:
        for g, f in zip(got, flat):
            assert np.array_equal(g.view(np.int32), f.view(np.int32)), f"{what} differ from the contiguous call"


# ---- (c) real shards against the unsharded oracle ----------------------------------------------------------------------
U_SHARDS, I_SHARDS = 300, 800


@functools.lru_cache(maxsize=None)
def tie_model(shape):
    """The recipe of test_column_shards_order_cross_shard_ties_like_the_reference (tests/test_gpu_kernels.py): the right half of W
    copies the left half, integer weights and ratings, so columns j and j + 400 score bit-equal for every user."""
    rng = np.random.default_rng(12)
    I, U, half = I_SHARDS, U_SHARDS, I_SHARDS // 2
    R = 60 if shape == "feature_rows" else 300
    rows_w = np.sort(rng.choice(I, R, replace=False))
    nnz = 4000 if shape == "feature_rows" else 2500
    r, c = rng.choice(rows_w, nnz), rng.integers(0, half, nnz)
    v = rng.integers(1, 4, nnz).astype(np.float32)
    A = sp.csc_matrix((v, (r, c)), shape=(I, half), dtype=np.float32)
    A.sum_duplicates()
    W = sp.hstack([A, A], format="csc").astype(np.float32)
    W.sort_indices()
    ur = np.repeat(np.arange(U), rng.integers(1, 40, U))
    ui = np.where(rng.random(len(ur)) < 0.6, rng.choice(rows_w, len(ur)), rng.integers(0, I, len(ur)))
    X = sp.csr_matrix((rng.integers(1, 6, len(ur)).astype(np.float32), (ur, ui)), shape=(U, I), dtype=np.float32)
    X.sum_duplicates(); X.sort_indices()
    return X, W


@functools.lru_cache(maxsize=None)
def oracle_lists(shape, k, filt, dense, f64):
    from oracle import slim_oracle
    X, W = tie_model(shape)
    out = slim_oracle.recommend_batch(X, W.tocsr(), top_k=k, filter_interacted=filt, dense=dense, use_f64=f64)
    for a in out:
        a.setflags(write=False)
    return out


def cross_shard_tie_rows(o_ids, o_sc, o_cnt, G):
    """Rows of the oracle's lists that hold two ADJACENT equal scores whose columns belong to different shards."""
    from rtrec_amd.engine import shard_bounds
    hi = np.array([shard_bounds(I_SHARDS, G, r)[1] for r in range(G)])
    shard = np.searchsorted(hi, o_ids, side="right")
    inside = np.arange(1, o_ids.shape[1])[None, :] < o_cnt[:, None]
    return int(((o_sc[:, 1:] == o_sc[:, :-1]) & (shard[:, 1:] != shard[:, :-1]) & inside).any(axis=1).sum())


SHARD_CASES = [(8, 10), (16, 10), (8, 50), (3, 64), (16, 64)]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", ["feature_rows", "general"])
@pytest.mark.parametrize("G,k", SHARD_CASES, ids=[case_id(*c) for c in SHARD_CASES])
def test_real_shards_merge_to_the_unsharded_oracle(engine, G, k, shape, f64):
    """G column shards of one W on one GPU (SlimEngine(rank=r, world_size=G)._local_topk, first-touch keys completed), stacked
    and merged, against the oracle on the whole W: SPARSE with and without the filter, DENSE for the float32 W.

    The inputs cannot pass vacuously: at least half of the 300 rows must hold, in the oracle's own SPARSE lists, two adjacent
    equal scores from different shards (shard_bounds of the engine).  Measured, float32 and float64 oracle scores alike, with
    and without the filter, at every (G, k) here: 297 rows for the general shape (mean list length 9.9 / 47.3 / 59.5 at
    k = 10 / 50 / 64, so short lists are present), 298 rows for the feature_rows shape (9.9 / 49.7 / 63.6)."""
    import torch
    from rtrec_amd import _native
    from rtrec_amd.engine import SlimEngine
    X, W = tie_model(shape)
    U, be = U_SHARDS, engine.be
    ties = cross_shard_tie_rows(*oracle_lists(shape, k, True, False, f64), G)
    print(f"cross-shard tie rows: {ties} of {U} ({shape}, G={G}, k={k}, f64={f64})")
    assert ties >= U // 2
    d_rows = be.to_dev(np.arange(U, dtype=np.int32))
    shards = []
    for r in range(G):
        e = SlimEngine(device="cuda:0", rank=r, world_size=G, backend=be)
        e.set_interactions(None, X, need_csc=False)
        if f64:
            e.set_weights(W.astype(np.float64), acc_f64=True)
        else:
            e.set_weights(W)
        shards.append(e)
    modes = [(_native.TOPK_SPARSE, True), (_native.TOPK_SPARSE, False)] + ([] if f64 else [(_native.TOPK_DENSE, True)])
    for mode, filt in modes:
        want = oracle_lists(shape, k, filt, mode == _native.TOPK_DENSE, f64)
        parts = []
        for e in shards:
            xb = (e._X["rptr"], e._X["rcol"], e._X["rval"])
            parts.append(e._local_topk(d_rows, U, xb, k, filt, mode, None))
        assert (parts[0][2] is not None) == f64
        g = [torch.stack([p[j] for p in parts]).contiguous() if parts[0][j] is not None else None for j in range(5)]
        outs = sentinel_outputs(be, U, k)
        _native.check(be.lib.rtrec_slim_merge_topk(U, G, k, be.ptr(g[0]), be.ptr(g[1]), be.ptr(g[2]), be.ptr(g[3]), be.ptr(g[4]),
                                                   be.ptr(outs[0]), be.ptr(outs[1]), be.ptr(outs[2]), be.stream()), "merge")
        be.synchronize()
        m_ids, m_sc, m_cnt = (t.cpu().numpy() for t in outs)
        assert_lists_equal((m_ids, m_sc, m_cnt), (want[0], want[1], want[2]), f"mode {mode} filter {filt}")


# ---- (d) the cross-shard tie key ------------------------------------------------------------------------------------
def first_touch_model(row_ids, x_ptr, x_col, n_items, wc_ptr, wc_row, ids, cnt):
    """The rule at the top of csrc/score_first_touch.hip: for entry (row, slot) inside the count whose id c is a column of W, the
    position in the user's row of X of the LOWEST item that stores a weight in column c; 0 where there is none, where the row id
    is no row of X, where the id is no column, and for every slot at or beyond the count."""
    n_rows, k = ids.shape
    n_x = len(x_ptr) - 1
    aux = np.zeros((n_rows, k), dtype=np.uint32)
    for r in range(n_rows):
        xr = int(row_ids[r]) if row_ids is not None else r
        if not 0 <= xr < n_x:
            continue
        items = x_col[x_ptr[xr]:x_ptr[xr + 1]]
        for s in range(min(int(cnt[r]), k)):
            c = int(ids[r, s])
            if 0 <= c < n_items:
                common = np.intersect1d(items, wc_row[wc_ptr[c]:wc_ptr[c + 1]])
                if common.size:
                    aux[r, s] = int(np.flatnonzero(items == common.min())[0])
    return aux


def first_touch_case(top_k, with_row_ids):
    """(row_ids or None, X, W, n_rows, ids, counts, slots beyond the count, expected keys)"""
    rng = np.random.default_rng([top_k, int(with_row_ids)])
    n_items, n_x, n_rows = 500, 260, 300
    X = sp.random(n_x, n_items, density=0.08, format="csr", dtype=np.float32, random_state=3)
    X = X.tolil(); X[7, :] = 0; X[n_x - 1, :] = 0                      # users with an empty row
    X = X.tocsr(); X.eliminate_zeros(); X.sort_indices()
    Wc = sp.random(n_items, n_items, density=0.03, format="csc", dtype=np.float32, random_state=4).tolil()
    Wc[:, 11] = 0; Wc[:, n_items - 1] = 0                              # columns without a stored weight
    Wc = Wc.tocsc(); Wc.eliminate_zeros(); Wc.sort_indices()
    if with_row_ids:
        row_ids = rng.integers(0, n_x, n_rows).astype(np.int32)
        row_ids[[3, 50, 299]] = [-1, n_x, 2 ** 31 - 1]                 # no rows of X
        row_ids[[4, 51]] = [7, n_x - 1]
    else:
        row_ids, n_rows = None, n_x
    ids = rng.integers(0, n_items, (n_rows, top_k)).astype(np.int32)
    ids[rng.random((n_rows, top_k)) < 0.1] = 11
    ids[rng.random((n_rows, top_k)) < 0.05] = n_items - 1
    ids[rng.random((n_rows, top_k)) < 0.05] = -1                       # no columns of W, inside the count
    ids[rng.random((n_rows, top_k)) < 0.05] = n_items
    ids[rng.random((n_rows, top_k)) < 0.02] = 2 ** 31 - 1
    cnt = rng.integers(0, top_k + 1, n_rows).astype(np.int32)
    cnt[:8] = top_k
    beyond = np.arange(top_k)[None, :] >= cnt[:, None]
    ids[beyond] = rng.choice(np.array([-1, n_items + 5, -2 ** 31, 2 ** 31 - 1], dtype=np.int32), int(beyond.sum()))   # poison
    want = first_touch_model(row_ids, X.indptr, X.indices, n_items, Wc.indptr, Wc.indices, ids, cnt)
    assert (want != 0).sum() > want.size // 10                        # the key is not trivially zero
    return row_ids, X, Wc, n_rows, ids, cnt, beyond, want


@pytest.mark.parametrize("with_row_ids", [True, False], ids=["row_ids", "rows_in_order"])
@pytest.mark.parametrize("top_k", [1, 64])
def test_first_touch_aux_equals_model(engine, top_k, with_row_ids):
    import torch
    be = engine.be
    row_ids, X, Wc, n_rows, ids, cnt, beyond, want = first_touch_case(top_k, with_row_ids)
    n_x, n_items = X.shape
    d = [be.to_dev(np.asarray(a, dtype=np.int32)) if a is not None else None
         for a in (row_ids, X.indptr, X.indices, Wc.indptr, Wc.indices, ids, cnt)]
    aux = torch.full((n_rows, top_k), 0x5a5a5a5a, dtype=torch.int32, device=be.device)
    rc = be.lib.rtrec_slim_first_touch_aux(n_rows, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), n_x, n_items, be.ptr(d[3]),
                                           be.ptr(d[4]), top_k, be.ptr(d[5]), be.ptr(d[6]), be.ptr(aux), be.stream())
    be.synchronize()
    assert rc == RTREC_OK
    got = aux.cpu().numpy().view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} keys differ, first (row, slot) {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    assert (got[beyond] == 0).all()
