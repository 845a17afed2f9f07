"""Five small kernels called directly -- through the C ABI (be.lib), the last one through its custom op -- and compared with
plain numpy / Python models written from their contracts in include/rtrec_amd.h:

  1. rtrec_slim_score_candidates  (csrc/score_cands.hip)      ranking of a given candidate list
  2. rtrec_slim_dense_fill        (csrc/score_dense_fill.hip) zero-score columns behind a short DENSE list
  3. rtrec_slim_score_rows        (csrc/score.hip)            score-vector export (predict*)
  4. rtrec_store_fold_device      (csrc/store_device.hip)     per-pair fold of a bulk ingest
  5. rtrec_slim_refine_topk_f64   (csrc/score_refine.hip)     float64 scores and order of a fast pass's lists

Bar: exact equality -- ids, counts, float32 / float64 bit patterns, and the bytes of memory outside the contract (every
output buffer starts as sentinels and carries a guard region behind its last row).  tests/test_request_kernels_host.py checks
the models of this module against independent references and shows, model against mutated model, that these inputs tell a
wrong kernel from a right one.

Not covered: the grid cap of the ingest fold (65,536 blocks of 256 pairs) is reached only beyond 16 million pairs; no case
here is that large, so its grid-stride loop always runs exactly once per thread.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

RTREC_OK, RTREC_ERR_INVALID_ARG, RTREC_ERR_UNSUPPORTED = 0, -1, -2          # include/rtrec_amd.h
SENTINEL_ID, SENTINEL_CNT, SENTINEL_SCORE, SENTINEL_AUX = -777, -555, 12345.5, 0x5a5a5a5a
GUARD_ROWS = 2                 # rows of sentinels behind the last row of every output


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def writable(M):
    """A copy of a shared sparse matrix that an engine may take over."""
    return M.copy()


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def dev(be, a, dtype=None):
    """A device copy of a shared (read-only) host array; None stays None (a NULL pointer)."""
    if a is None:
        return None
    return be.to_dev(np.array(a, dtype=dtype))


# ======================================================================================================================
# 1. candidates kernel
# ======================================================================================================================
CD_ITEMS = 2600
CD_STAGED = 2048               # kCdItems: items of a row staged in LDS
CD_FULL_COL = 1234             # the column that stores all 2,600 rows
CD_EXACT_COLS = {0: 7, 1: 8, 3: 9, 4: 10, 5: 11, 8: 12, 9: 13}      # entries -> column: the four-at-a-time loop and its tail
CD_ROW = {"empty": 0, "one": 1, "n2047": 2, "n2048": 3, "n2049": 4, "n2600": 5, "zeros": 18, "inf": 19}
CD_FINITE_ROWS = 19            # rows 0..18 hold finite ratings; row 19 rates half the catalogue with +inf


def _signed_weights(rng, n):
    """float32 weights of both signs with exponents spread over 2^-20 .. 2^20: the order of a sum changes its bits."""
    return (rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-20, 21, n)) * rng.uniform(1.0, 2.0, n)).astype(np.float32)


def _signed_ratings(rng, n):
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 5.0, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cands_data(name="main"):
    """(X csr float32, W csc float32) for the candidates kernel.  "main": the seeded 2,600-item model of the module
    docstring; "hand": six items made by hand (a float64 pair below float32 resolution, a row of negative and zero scores)."""
    if name == "hand":
        # column 0 (A): 1 * 1 + 1 * 2^-30; column 1 (B): 1 * 1; columns 2, 3: negative; columns 4, 5: empty
        W = sp.csc_matrix((np.array([1.0, 2.0 ** -30, 1.0, -1.0, -2.0], dtype=np.float32),
                           (np.array([0, 1, 0, 0, 1]), np.array([0, 0, 1, 2, 3]))), shape=(6, 6))
        X = sp.csr_matrix((np.array([1.0, 1.0], dtype=np.float32), np.array([0, 1]), np.array([0, 2])), shape=(1, 6))
    else:
        rng = np.random.default_rng(2600)
        I = CD_ITEMS
        n_ent = rng.integers(2, 11, I)
        for n, c in CD_EXACT_COLS.items():
            n_ent[c] = n
        n_ent[CD_FULL_COL] = I
        rows = np.concatenate([np.sort(rng.choice(I, n, replace=False)) for n in n_ent])
        cptr = np.concatenate([[0], np.cumsum(n_ent)])
        W = sp.csc_matrix((_signed_weights(rng, len(rows)), rows, cptr), shape=(I, I))
        lens = [0, 1, 2047, 2048, 2049, 2600] + [int(n) for n in rng.integers(20, 41, 13)] + [1300]
        cols = [np.sort(rng.choice(I, n, replace=False)) for n in lens]
        vals = [_signed_ratings(rng, n) for n in lens]
        z = CD_ROW["zeros"]
        vals[z][[0, 3, 7]] = [-0.0, 1e-40, -3e-39]                    # a -0.0 rating and two denormal ones
        vals[CD_ROW["inf"]][:] = np.inf
        X = sp.csr_matrix((np.concatenate(vals), np.concatenate(cols), np.concatenate([[0], np.cumsum(lens)])),
                          shape=(len(lens), I))
    X.indices, X.indptr = X.indices.astype(np.int32), X.indptr.astype(np.int32)
    W.indices, W.indptr = W.indices.astype(np.int32), W.indptr.astype(np.int32)
    assert X.has_canonical_format and W.has_canonical_format and X.dtype == W.dtype == np.float32
    frozen(X.data, X.indices, X.indptr, W.data, W.indices, W.indptr)
    return X, W


def fold_column(items, vals, w_rows, w_vals, f64, descending=False, drop_tail=0, fma=False):
    """sum_i x_i * w_i over the entries (w_rows ascending, w_vals) of one column of W whose row is among `items` (ascending,
    ratings `vals`): acc = fl(acc + fl(x * w)) from acc = +0 in entry order -- np.float32 arithmetic, or Python floats
    (float64) over the float32 inputs when f64.  The keyword arguments are the mutations of the host file: entries summed in
    descending order, the last len % drop_tail entries left out, one fused multiply-add per entry (float32 form)."""
    n = len(w_rows)
    if drop_tail:
        n -= n % drop_tail
    if n == 0 or len(items) == 0:
        return 0.0 if f64 else np.float32(0.0)
    pos = np.minimum(np.searchsorted(items, w_rows[:n]), len(items) - 1)
    hit = items[pos] == w_rows[:n]
    xs, ws = vals[pos[hit]], w_vals[:n][hit]
    if descending:
        xs, ws = xs[::-1], ws[::-1]
    with np.errstate(all="ignore"):
        if f64:
            acc = 0.0
            for x, w in zip(xs.tolist(), ws.tolist()):
                acc = acc + x * w
            return acc
        acc = np.float32(0.0)
        for x, w in zip(xs, ws):
            acc = np.float32(float(acc) + float(x) * float(w)) if fma else np.float32(acc + np.float32(x * w))
        return acc


_score_cache = {}


def cand_score(data, xrow, c, f64, **mut):
    """The score of candidate id c for row xrow of X (anything that is no row of X scores as an empty row, an id that is no
    column of W scores 0)."""
    key = (data, xrow, c, f64, tuple(sorted(mut.items())))
    if key not in _score_cache:
        X, W = cands_data(data)
        if not (0 <= xrow < X.shape[0] and 0 <= c < W.shape[1]):
            _score_cache[key] = 0.0 if f64 else np.float32(0.0)
        else:
            a, b, s, e = X.indptr[xrow], X.indptr[xrow + 1], W.indptr[c], W.indptr[c + 1]
            _score_cache[key] = fold_column(X.indices[a:b], X.data[a:b], W.indices[s:e], W.data[s:e], f64, **mut)
    return _score_cache[key]


def cands_model(data, row_ids, cands, top_k, f64, tie_low=False, compare_f32=False, x_of=None, **mut):
    """The contract of rtrec_slim_score_candidates: (ids [R, top_k], float32 scores, float64 scores or None, counts).  Per
    row the candidates by (score descending, position descending), a NaN score never listed; output id = cands[p], float32
    score = the cast; slots beyond the count hold -1 / -inf.  Mutations: tie_low (the earlier position wins a tie),
    compare_f32 (the float64 form orders by the float32 casts), x_of (a function replacing cand_score), **mut (fold_column)."""
    X, _ = cands_data(data)
    rows = list(range(X.shape[0])) if row_ids is None else [int(r) for r in row_ids]
    R = len(rows)
    o_ids = np.full((R, top_k), -1, dtype=np.int32)
    o_sc = np.full((R, top_k), -np.inf, dtype=np.float32)
    o_sc64 = np.full((R, top_k), -np.inf, dtype=np.float64) if f64 else None
    o_cnt = np.zeros(R, dtype=np.int32)
    score = x_of or cand_score
    for r, xr in enumerate(rows):
        sc = [score(data, xr, int(c), f64, **mut) for c in cands]
        with np.errstate(all="ignore"):
            key = [float(np.float32(s)) if compare_f32 else float(s) for s in sc]
        valid = [p for p in range(len(cands)) if key[p] == key[p]]
        valid.sort(key=lambda p: (-key[p], p if tie_low else -p))
        best = valid[:top_k]
        o_cnt[r] = len(best)
        for j, p in enumerate(best):
            o_ids[r, j] = cands[p]
            with np.errstate(all="ignore"):
                o_sc[r, j] = np.float32(sc[p])
            if f64:
                o_sc64[r, j] = sc[p]
    return o_ids, o_sc, o_sc64, o_cnt


def cands_list(n_cands, seed=0):
    """n_cands ids in random order: the special columns first in line, at least one duplicate from two ids on."""
    rng = np.random.default_rng([n_cands, seed])
    special = [CD_FULL_COL] + [CD_EXACT_COLS[n] for n in (9, 5, 3, 1, 0, 8, 4)] + [0, CD_ITEMS - 1]
    c = np.concatenate([special, rng.integers(0, CD_ITEMS, max(n_cands - len(special), 0))])[:n_cands]
    if n_cands >= 2:
        c[-1] = c[0]
    if n_cands >= 64:
        c[rng.integers(10, n_cands - 1, n_cands // 16)] = c[rng.integers(0, 10, n_cands // 16)]
    return rng.permutation(c).astype(np.int32)


def cd_row_subset():
    """A permuted subset of the rows of X with two ids that are no rows: both score as an empty row."""
    n_x = cands_data()[0].shape[0]
    return np.array([CD_ROW["n2049"], -1, 9, CD_ROW["zeros"], n_x, CD_ROW["n2048"], CD_ROW["n2600"], 6, CD_ROW["empty"],
                     CD_ROW["n2047"], CD_ROW["one"], 9], dtype=np.int32)


CD_SIZES = [1, 63, 64, 65, 128, 129, 256, 257]         # both sides of the 64 / 128-thread cuts, more than one pass at 256


def cands_cases(n_cands, f64):
    """[(data, row_ids or None, cands, top_k)] of one parametrised GPU case."""
    if n_cands in CD_SIZES:
        c = cands_list(n_cands)
        finite = np.arange(CD_FINITE_ROWS, dtype=np.int32)
        return [("main", rows, c, k) for rows in (None, finite, cd_row_subset()) for k in sorted({1, 10, n_cands})]
    # the long lists: 4 rows, top_k <= 300 (the selection costs top_k * n_cands / 64 steps per row)
    rows = np.array([CD_ROW["n2600"], 7, CD_ROW["n2049"], CD_ROW["zeros"]], dtype=np.int32)
    return [("main", rows, cands_list(n_cands), k) for k in (65, 300)]


CD_EXTRA = {
    # top_k above 64 with a short list: the padding loop runs more than one pass
    "pad200": ("main", np.arange(CD_FINITE_ROWS, dtype=np.int32), np.array([CD_FULL_COL, 40, CD_FULL_COL], dtype=np.int32), 200),
    # ids that are no columns of W score 0 and compete with the id as given
    "foreign_ids": ("main", cd_row_subset(),
                    np.array([-5, CD_FULL_COL, CD_ITEMS, 13, 2 ** 31 - 1, -2 ** 31, 12, CD_ITEMS + 7], dtype=np.int32), 8),
    # an inf rating against weights of both signs: NaN scores are never listed, +-inf scores are
    "nan_some": ("main", np.array([CD_ROW["inf"], 6, CD_ROW["inf"]], dtype=np.int32), None, 70),
    "nan_pad200": ("main", np.array([CD_ROW["inf"]], dtype=np.int32), None, 200),
    "nan_all": ("main", None, None, 5),
    # the float64 pair below float32 resolution, and the row of negative and zero scores
    "pair": ("hand", None, np.array([0, 1], dtype=np.int32), 2),
    "pair_swapped": ("hand", None, np.array([1, 0], dtype=np.int32), 2),
    "zeros_lead": ("hand", None, np.array([2, 4, 3, 5, 2], dtype=np.int32), 5),
}


def cands_extra_case(name, f64=False):
    data, rows, c, k = CD_EXTRA[name]
    if c is None:
        X, W = cands_data("main")
        rated = X.indices[X.indptr[CD_ROW["inf"]]:X.indptr[CD_ROW["inf"] + 1]]
        kind = {}
        for col in range(CD_ITEMS):
            w = W.data[W.indptr[col]:W.indptr[col + 1]][np.isin(W.indices[W.indptr[col]:W.indptr[col + 1]], rated)]
            kind.setdefault("empty" if len(w) == 0 else "pos" if (w > 0).all() else "neg" if (w < 0).all() else "mixed", []).append(col)
        assert all(len(kind[t]) >= 8 for t in ("empty", "pos", "neg", "mixed"))
        if name == "nan_all":
            c, rows = np.array(kind["mixed"][:40], dtype=np.int32), np.array([CD_ROW["inf"], CD_ROW["inf"]], dtype=np.int32)
        else:
            c = np.array(kind["mixed"][:30] + kind["pos"][:8] + kind["empty"][:8] + kind["neg"][:8] + kind["mixed"][30:50], dtype=np.int32)
            c = np.random.default_rng(5).permutation(c)
    return data, rows, c, k


def run_cands(be, data, row_ids, cands, top_k, f64, n_rows=None, n_cands=None, with_sc64=True):
    """(status, ids, float32 scores, float64 scores, counts) of one call; the outputs have GUARD_ROWS rows more than the call
    may write and start as sentinels."""
    import torch
    X, W = cands_data(data)
    R = X.shape[0] if row_ids is None else len(row_ids)
    d = [dev(be, a) for a in (row_ids, X.indptr, X.indices, X.data, W.indptr, W.indices, W.data, cands)]
    o_ids = torch.full((R + GUARD_ROWS, top_k), SENTINEL_ID, dtype=torch.int32, device=be.device)
    o_sc = torch.full((R + GUARD_ROWS, top_k), SENTINEL_SCORE, dtype=torch.float32, device=be.device)
    o_sc64 = torch.full((R + GUARD_ROWS, top_k), SENTINEL_SCORE, dtype=torch.float64, device=be.device)
    o_cnt = torch.full((R + GUARD_ROWS,), SENTINEL_CNT, dtype=torch.int32, device=be.device)
    rc = be.lib.rtrec_slim_score_candidates(R if n_rows is None else n_rows, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]),
                                            X.shape[0], W.shape[1], be.ptr(d[4]), be.ptr(d[5]), be.ptr(d[6]), be.ptr(d[7]),
                                            len(cands) if n_cands is None else n_cands, top_k, int(f64), be.ptr(o_ids), be.ptr(o_sc),
                                            be.ptr(o_sc64 if with_sc64 else None), be.ptr(o_cnt), be.stream())
    be.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_ids, o_sc, o_sc64, o_cnt))


def all_sentinels(o_ids, o_sc, o_sc64, o_cnt):
    return bool((o_ids == SENTINEL_ID).all() and (o_sc == np.float32(SENTINEL_SCORE)).all() and (o_sc64 == SENTINEL_SCORE).all()
                and (o_cnt == SENTINEL_CNT).all())


def assert_cands_equal(got, want, f64, what):
    rc, g_ids, g_sc, g_sc64, g_cnt = got
    w_ids, w_sc, w_sc64, w_cnt = want
    R = len(w_cnt)
    assert rc == RTREC_OK, what
    assert all_sentinels(g_ids[R:], g_sc[R:], g_sc64[R:], g_cnt[R:]), f"{what}: written behind the last row"
    assert np.array_equal(g_cnt[:R], w_cnt), f"{what}: counts {g_cnt[:R]} vs {w_cnt}"
    bad = np.flatnonzero((g_ids[:R] != w_ids).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ on rows {bad[:8]}, first: {g_ids[bad[0]][:12]} vs {w_ids[bad[0]][:12]}"
    bad = np.flatnonzero((bits(g_sc[:R]) != bits(w_sc)).any(axis=1))
    assert bad.size == 0, f"{what}: score bits differ on rows {bad[:8]}, first: {g_sc[bad[0]][:12]} vs {w_sc[bad[0]][:12]}"
    if f64:
        bad = np.flatnonzero((bits64(g_sc64[:R]) != bits64(w_sc64)).any(axis=1))
        assert bad.size == 0, f"{what}: float64 bits differ on rows {bad[:8]}, first: {g_sc64[bad[0]][:6]} vs {w_sc64[bad[0]][:6]}"
    else:
        assert (g_sc64 == SENTINEL_SCORE).all(), f"{what}: the float32 form wrote float64 scores"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n_cands", CD_SIZES + ["longest"])
def test_candidates_equal_model(engine, n_cands, f64):
    """Every launch width (64 / 128 / 256 threads), rows on both sides of the LDS staging limit of 2,048 items, lists up to
    the ABI limit (8,192 candidates in float32, 6,144 in float64: beyond the engine's CANDS_DIRECT_MAX), duplicates, signed
    scores whose bits depend on the summation order, rows that are no rows of X."""
    if n_cands == "longest":
        n_cands = 6144 if f64 else 8192
    for data, rows, c, k in cands_cases(n_cands, f64):
        got = run_cands(engine.be, data, rows, c, k, f64)
        what = f"{n_cands} candidates, top_k {k}, rows {'in order' if rows is None else list(rows[:4])}"
        assert_cands_equal(got, cands_model(data, rows, c, k, f64), f64, what)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["pad200", "foreign_ids", "nan_some", "nan_pad200", "nan_all", "zeros_lead"])
def test_candidates_edge_lists_equal_model(engine, name, f64):
    data, rows, c, k = cands_extra_case(name)
    want = cands_model(data, rows, c, k, f64)
    assert_cands_equal(run_cands(engine.be, data, rows, c, k, f64), want, f64, name)
    n_valid = min(k, len(c))
    if name == "nan_all":
        assert (want[3] == 0).all() and (want[0] == -1).all()
    elif name.startswith("nan"):
        assert 0 < want[3][0] < n_valid and np.isinf(want[1][0, :want[3][0]]).any()     # NaN left out, +-inf listed
    elif name == "zeros_lead":
        assert want[0].tolist() == [[5, 4, 2, 2, 3]] and want[1].tolist() == [[0.0, 0.0, -1.0, -1.0, -2.0]]
    elif name == "foreign_ids":
        assert (want[3] == n_valid).all() and -5 in want[0][1] and 2 ** 31 - 1 in want[0][1]


def test_candidates_float64_order_below_float32_resolution(engine):
    """Candidate A scores 1 + 2^-30 in float64 and exactly 1.0 in float32, candidate B exactly 1.0: the float32 form sees a
    tie (the later position first), the float64 form puts A first whatever its position -- with equal float32 casts."""
    be = engine.be
    for name, later_first, a_first in (("pair", [1, 0], [0, 1]), ("pair_swapped", [0, 1], [0, 1])):
        data, rows, c, k = cands_extra_case(name)
        for f64 in (False, True):
            got = run_cands(be, data, rows, c, k, f64)
            assert_cands_equal(got, cands_model(data, rows, c, k, f64), f64, name)
            assert got[1][0].tolist() == (a_first if f64 else later_first)
            assert got[2][0].tolist() == [1.0, 1.0]
            if f64:
                assert got[3][0].tolist() == [1.0 + 2.0 ** -30, 1.0]


def test_candidates_argument_checks_leave_outputs_alone(engine):
    be = engine.be
    c = cands_list(8192)
    rows = np.array([6, 7], dtype=np.int32)
    for f64, n_cands, with_sc64, n_rows, want in ((False, 8193, True, None, RTREC_ERR_INVALID_ARG),
                                                  (True, 6145, True, None, RTREC_ERR_UNSUPPORTED),
                                                  (True, 64, False, None, RTREC_ERR_INVALID_ARG),
                                                  (False, 64, True, 0, RTREC_OK), (True, 64, True, 0, RTREC_OK)):
        cc = np.concatenate([c, c[:1]]) if n_cands > len(c) else c
        got = run_cands(be, "main", rows, cc, 10, f64, n_rows=n_rows, n_cands=n_cands, with_sc64=with_sc64)
        assert got[0] == want and all_sentinels(*got[1:]), (f64, n_cands, with_sc64, n_rows)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_engine_candidates_for_rows_beyond_the_staging_limit(f64):
    """recommend_rows(candidates=...) for the users of 2,049 and 2,600 items takes the direct kernel and equals the model."""
    from rtrec_amd import _native
    from rtrec_amd.engine import SlimEngine
    X, W = cands_data()
    Xe, W = writable(X[:CD_ROW["n2600"] + 1]), writable(W)
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(None, Xe, need_csc=False)
    eng.set_weights(W.astype(np.float64) if f64 else W, acc_f64=f64)
    rows, c = np.array([CD_ROW["n2049"], CD_ROW["n2600"]]), cands_list(257)
    ids, sc, cnt = eng.recommend_rows(rows, top_k=10, mode=_native.TOPK_CANDIDATES, candidates=c)
    assert eng.last_score_path == "candidates_direct"
    w_ids, w_sc, _, w_cnt = cands_model("main", rows, c, 10, f64)
    assert np.array_equal(ids, w_ids) and np.array_equal(bits(sc), bits(w_sc)) and np.array_equal(cnt, w_cnt)


# ======================================================================================================================
# 2. dense fill
# ======================================================================================================================
FILL_WINDOW = 2048             # kFillWindow: column ids per step
# (col_lo, span, ids of X beyond col_hi): spans around the window, a shard that starts at 37, one that ends below the catalogue
FILL_SHARDS = [(lo, span, 0) for span in (31, 2048, 2049, 2048 + 33, 4097) for lo in (0, 37)] + [(37, 2048 + 33, 60)]
FILL_TOP_K = [1, 8, 63, 64]


@functools.lru_cache(maxsize=None)
def fill_case(col_lo, span, beyond, top_k):
    """Hand-made lists for one shard: (X csr structure, ids, scores, counts, flagged rows).  One row of X per list row; the
    last two users rate everything (with row ids given they are addressed as -1 and n_x_rows, where no filter applies)."""
    rng = np.random.default_rng([col_lo, span, beyond, top_k])
    hi, K = col_lo + span, top_k
    n_items = hi + beyond
    w_lo = max(col_lo, hi - FILL_WINDOW)                       # the first window is [w_lo, hi)
    first = np.arange(w_lo, hi)
    everything = np.arange(n_items)
    rows = []                                                  # (user's items, listed ids, listed scores, flagged)

    def some_items(n=30):
        return np.unique(np.concatenate([rng.integers(0, n_items, n), rng.integers(max(hi - 50, 0), hi, 6)]))

    def pos_scores(n):
        return np.sort(rng.uniform(0.5, 9.0, n).astype(np.float32))[::-1] * np.float32(1.0) if n else np.empty(0, np.float32)

    def listed(n, where=None):
        pool = np.arange(col_lo, hi) if where is None else where
        return rng.choice(pool, min(n, len(pool)), replace=False).astype(np.int64)

    def add(items, ids, scores=None, flagged=True):
        ids = np.asarray(ids, dtype=np.int64)[:K]
        scores = pos_scores(len(ids)) if scores is None else np.asarray(scores, dtype=np.float32)[:K]
        assert len(scores) == len(ids) and len(np.unique(ids)) == len(ids)
        rows.append((np.asarray(items, dtype=np.int64), ids, scores, flagged))

    for _ in range(12):
        add(some_items(), [])                                                   # count 0
        add(some_items(), listed(K - 1))                                        # count top_k - 1
        add(some_items(), listed(K))                                            # count top_k: handed on
        add(some_items(), listed(int(rng.integers(0, K))))                      # anything below
    add([], [])
    add(first, [])                                             # the whole first window rated: the fill starts in the second
    add(first, listed(min(2, K - 1)))
    for c in sorted({0, min(2, K - 1), K // 2}):               # all of the first window but top_k - count - 1 ids: crosses mid-list
        keep = rng.choice(first, min(max(K - c - 1, 0), len(first)), replace=False)
        add(np.setdiff1d(first, keep), listed(c, np.setdiff1d(np.arange(col_lo, hi), keep)))
    add(first[1:], [])                                         # only the lowest id of the first window is free
    add(first[:-1], listed(min(1, K - 1), np.arange(col_lo, hi - 1)))
    add(everything, [])                                        # everything rated: the count stays
    add(everything, listed(K // 2))
    add(np.setdiff1d(everything, [col_lo]), [])                # the catalogue runs out at its lowest id
    add(np.setdiff1d(everything, [col_lo, col_lo + 1, hi - 1]), listed(min(1, K - 1), [col_lo + 1]))
    # listed ids at the top of the first window, at the top of the second (reached when the first is rated), outside the shard
    top1 = [hi - 1, hi - 3, hi - 2 - 32]
    top2 = [i for i in (w_lo - 1, w_lo - 3, w_lo - 33, w_lo - 64) if i >= col_lo]
    outside = [i for i in (col_lo - 1, col_lo - 30) if i >= 0] + [hi, hi + 5, hi + FILL_WINDOW]
    add(some_items(), top1[:K - 1])
    add(first, top2[:K - 1])
    add(first, (top1 + top2)[:K - 1])
    add(some_items(), (outside + top1)[:K - 1])
    add(first, (outside[:2] + top2)[:K - 1])
    # hand-over rules: an entry that is not positive, equal neighbours
    if K >= 2:
        for bad in (0.0, -0.0, -1.5, np.nan, -np.inf):
            n = min(3, K - 1)
            s = pos_scores(n)
            s[int(rng.integers(0, n))] = bad
            add(some_items(), listed(n), s)
        add(some_items(), listed(1), [1e-40])                  # a positive denormal: completed
        add(some_items(), listed(1), [np.inf])
    if K >= 8:
        for at in (0, 3):                                      # a tie in the first two and in the last two of five slots
            s = pos_scores(5)
            s[at + 1] = s[at]
            add(some_items(), listed(5), s)
        s = pos_scores(5)
        s[4] = s[0]                                            # equal, but no neighbours: completed
        add(some_items(), listed(5), s)
    for _ in range(4):                                         # not flagged: nothing may change
        add(some_items(), listed(int(rng.integers(0, K))), flagged=False)
    add(everything, [])                                        # the two users that row ids address as -1 and n_x_rows
    add(everything, listed(K // 3))
    R = len(rows)
    ids = np.full((R, K), SENTINEL_ID, dtype=np.int32)
    sc = np.full((R, K), SENTINEL_SCORE, dtype=np.float32)
    cnt = np.zeros(R, dtype=np.int32)
    for r, (_, i, s, _) in enumerate(rows):
        ids[r, :len(i)], sc[r, :len(i)], cnt[r] = i, s, len(i)
    xptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
    xcol = np.concatenate([r[0] for r in rows]).astype(np.int32)
    flagged = rng.permutation(np.flatnonzero([r[3] for r in rows])).astype(np.int32)
    return frozen(xptr, xcol, ids, sc, cnt, flagged)


def fill_permuted(xptr, xcol, n_rows):
    """(row ids, X structure): X with its rows permuted so that list row r still meets its own user through the row ids --
    except the last two list rows, whose ids -1 and n_x_rows are no rows of X."""
    rid = np.random.default_rng(n_rows).permutation(n_rows).astype(np.int32)
    lens = np.diff(xptr)
    inv = np.argsort(rid)                                      # X' row j = old row inv[j]
    pptr = np.concatenate([[0], np.cumsum(lens[inv])]).astype(np.int32)
    pcol = np.concatenate([xcol[xptr[j]:xptr[j + 1]] for j in inv]).astype(np.int32)
    rid[n_rows - 2], rid[n_rows - 1] = -1, n_rows
    return rid, pptr, pcol


def fill_model(xptr, xcol, row_ids, col_lo, col_hi, top_k, filt, ids, sc, aux, cnt, flagged, *, window=None, carry=True,
               mask_slack=0, mask_listed=True, mask_items_later=True, nonneg_ok=False):
    """The contract of rtrec_slim_dense_fill on copies of the lists: (ids, scores, aux, counts, sorted rows handed on).
    window=None is the plain statement (walk the ids downwards); window=2048 is the same walk cut into the kernel's windows,
    which the mutations of the host file need: carry (the running count enters the next window), mask_slack (ids below
    col_lo admitted by the last window's partial word), mask_listed, mask_items_later, nonneg_ok (>= 0 passes as positive)."""
    ids, sc, cnt = ids.copy(), sc.copy(), cnt.copy()
    aux = None if aux is None else aux.copy()
    n_x = len(xptr) - 1
    handed = []
    for row in flagged:
        c = int(cnt[row])
        s = sc[row, :c]
        with np.errstate(invalid="ignore"):
            positive = bool((s >= 0).all()) if nonneg_ok else bool((s > 0).all())
            ok = c < top_k and positive and not bool((s[1:] == s[:-1]).any())
        if not ok:
            handed.append(int(row))
            continue
        xr = int(row) if row_ids is None else int(row_ids[row])
        mine = set(xcol[xptr[xr]:xptr[xr + 1]].tolist()) if filt and 0 <= xr < n_x else set()
        listed = set(ids[row, :c].tolist()) if mask_listed else set()
        have = c
        if window is None:
            for col in range(col_hi - 1, col_lo - 1, -1):
                if have >= top_k:
                    break
                if col not in listed and col not in mine:
                    ids[row, have], sc[row, have] = col, 0.0
                    if aux is not None:
                        aux[row, have] = 0
                    have += 1
        else:
            hi = col_hi
            while have < top_k and hi > col_lo:
                lo = max(hi - window, col_lo)
                low = lo - mask_slack if (hi - lo) % 32 else lo
                free = [col for col in range(hi - 1, low - 1, -1)
                        if col < lo or (col not in listed and not (col in mine and (mask_items_later or hi == col_hi)))]
                pos = have if carry else c
                for col in free[:max(top_k - pos, 0)]:
                    ids[row, pos], sc[row, pos] = col, 0.0
                    if aux is not None:
                        aux[row, pos] = 0
                    pos += 1
                have = min((have if carry else c) + len(free), top_k)
                hi = lo
        cnt[row] = have
    return ids, sc, aux, cnt, sorted(handed)


def run_fill(be, xptr, xcol, row_ids, col_lo, col_hi, top_k, filt, ids, sc, cnt, flagged, with_aux, n_rows=None):
    """One call on sentinel-guarded device copies: (status, ids, scores, aux or None, counts, flag_out)."""
    import torch
    R = len(cnt)
    guard_i = np.full((GUARD_ROWS, top_k), SENTINEL_ID, dtype=np.int32)
    guard_s = np.full((GUARD_ROWS, top_k), SENTINEL_SCORE, dtype=np.float32)
    d_ids = dev(be, np.concatenate([ids, guard_i]))
    d_sc = dev(be, np.concatenate([sc, guard_s]))
    d_cnt = dev(be, np.concatenate([cnt, np.full(GUARD_ROWS, SENTINEL_CNT, dtype=np.int32)]))
    d_aux = torch.full((R + GUARD_ROWS, top_k), SENTINEL_AUX, dtype=torch.int32, device=be.device) if with_aux else None
    d_in = dev(be, np.concatenate([[len(flagged)], flagged, np.full(R + 1 - len(flagged), SENTINEL_ID)]).astype(np.int32))
    d_out = torch.full((R + 1 + GUARD_ROWS,), SENTINEL_ID, dtype=torch.int32, device=be.device)
    d_x = [dev(be, a) for a in (row_ids, xptr, xcol)]
    rc = be.lib.rtrec_slim_dense_fill(R if n_rows is None else n_rows, be.ptr(d_x[0]), be.ptr(d_x[1]), be.ptr(d_x[2]), len(xptr) - 1,
                                      col_lo, col_hi, top_k, int(filt), be.ptr(d_ids), be.ptr(d_sc), be.ptr(d_aux), be.ptr(d_cnt),
                                      be.ptr(d_in), be.ptr(d_out), be.stream())
    be.synchronize()
    return (rc,) + tuple(None if t is None else t.cpu().numpy() for t in (d_ids, d_sc, d_aux, d_cnt, d_out))


def assert_fill_equal(got, want, R, top_k, what):
    rc, g_ids, g_sc, g_aux, g_cnt, g_out = got
    w_ids, w_sc, w_aux, w_cnt, w_handed = want
    assert rc == RTREC_OK, what
    assert (g_ids[R:] == SENTINEL_ID).all() and (g_sc[R:] == np.float32(SENTINEL_SCORE)).all() and (g_cnt[R:] == SENTINEL_CNT).all(), what
    assert np.array_equal(g_cnt[:R], w_cnt), f"{what}: counts differ on rows {np.flatnonzero(g_cnt[:R] != w_cnt)[:8]}"
    bad = np.flatnonzero((g_ids[:R] != w_ids).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ on rows {bad[:8]}, first: {g_ids[bad[0]][:10]} vs {w_ids[bad[0]][:10]}"
    assert np.array_equal(bits(g_sc[:R]), bits(w_sc)), f"{what}: score bits differ"
    if w_aux is not None:
        assert np.array_equal(g_aux[:R], w_aux) and (g_aux[R:] == SENTINEL_AUX).all(), f"{what}: aux differs"
    n = len(w_handed)
    assert g_out[0] == n and sorted(g_out[1:1 + n].tolist()) == w_handed, f"{what}: rows handed on {g_out[:n + 1]} vs {w_handed}"
    assert (g_out[1 + n:] == SENTINEL_ID).all(), f"{what}: flag list written beyond its count"


@pytest.mark.parametrize("top_k", FILL_TOP_K)
@pytest.mark.parametrize("shard", FILL_SHARDS, ids=[f"lo{s[0]}-span{s[1]}{'-below' if s[2] else ''}" for s in FILL_SHARDS])
def test_dense_fill_equals_model(engine, shard, top_k):
    """Shards of one window, one window and a partial word, two windows and a rest; users whose rated ids push the fill into
    the later windows; every hand-over rule at its edge values; rows that are not flagged; row ids that are no rows of X."""
    be = engine.be
    col_lo, span, beyond = shard
    xptr, xcol, ids, sc, cnt, flagged = fill_case(col_lo, span, beyond, top_k)
    R = len(cnt)
    aux0 = np.full((R, top_k), SENTINEL_AUX, dtype=np.int32)
    rid, pptr, pcol = fill_permuted(xptr, xcol, R)
    for filt in (True, False):
        for row_ids, xp, xc, with_aux in ((None, xptr, xcol, False), (rid, pptr, pcol, True)):
            got = run_fill(be, xp, xc, row_ids, col_lo, col_lo + span, top_k, filt, ids, sc, cnt, flagged, with_aux)
            want = fill_model(xp, xc, row_ids, col_lo, col_lo + span, top_k, filt, ids, sc, aux0 if with_aux else None, cnt, flagged)
            assert_fill_equal(got, want, R, top_k, f"filter {filt}, row ids {row_ids is not None}")
    # an empty flag list: nothing moves
    none = np.empty(0, dtype=np.int32)
    got = run_fill(be, xptr, xcol, None, col_lo, col_lo + span, top_k, True, ids, sc, cnt, none, True)
    assert_fill_equal(got, (ids, sc, aux0, cnt, []), R, top_k, "empty flag list")


@functools.lru_cache(maxsize=None)
def fill_many_rows(n_rows=9000, top_k=4, n_items=300):
    rng = np.random.default_rng(9000)
    lens = rng.integers(0, 12, n_rows)
    lens[::50] = 0
    xcol = np.concatenate([np.sort(rng.choice(np.arange(n_items - 16, n_items), n, replace=False)) for n in lens]).astype(np.int32)
    xptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cnt = rng.integers(0, top_k + 1, n_rows).astype(np.int32)
    ids = np.full((n_rows, top_k), SENTINEL_ID, dtype=np.int32)
    sc = np.full((n_rows, top_k), SENTINEL_SCORE, dtype=np.float32)
    for r in range(n_rows):
        ids[r, :cnt[r]] = rng.choice(np.arange(n_items - 12, n_items), cnt[r], replace=False)
        sc[r, :cnt[r]] = np.float32(9.0) - np.arange(cnt[r], dtype=np.float32)
    sc[rng.random(n_rows) < 0.05, 0] = 0.0                    # some rows are handed on (where the count is not 0)
    return frozen(xptr, xcol, ids, sc, cnt, rng.permutation(n_rows).astype(np.int32))


def test_dense_fill_more_rows_than_the_grid(engine):
    """9,000 flagged rows: the grid is capped at 8,192 workgroups, so the first 808 take a second row."""
    xptr, xcol, ids, sc, cnt, flagged = fill_many_rows()
    R, K = ids.shape
    got = run_fill(engine.be, xptr, xcol, None, 0, 300, K, True, ids, sc, cnt, flagged, False)
    want = fill_model(xptr, xcol, None, 0, 300, K, True, ids, sc, None, cnt, flagged)
    assert 100 < len(want[4]) < R - 100 and not np.array_equal(want[3], cnt)
    assert_fill_equal(got, want, R, K, "9000 rows")


# ======================================================================================================================
# 3. score-vector export
# ======================================================================================================================
EX_ITEMS, EX_TILE = 700, 256
EX_WIDE_ROW = 5                                     # the row of W that stores all 256 columns of tile 1 of the whole W
EX_LAYOUTS = {"whole": (0, 700), "one_tile": (130, 386), "tile_of_one": (130, 387)}
EX_ROWS = [1, 3, 5, 8, 11]
EX_GAP = 5


@functools.lru_cache(maxsize=None)
def export_data():
    """(X csr float32 with one id beyond the items of W, W csc float32 700 x 700, signed)."""
    rng = np.random.default_rng(700)
    I = EX_ITEMS
    r, c = rng.integers(0, I, 9000), rng.integers(0, I, 9000)
    r = np.concatenate([r, np.full(256, EX_WIDE_ROW), rng.integers(0, I, 40)])
    c = np.concatenate([c, np.arange(256, 512), np.repeat([0, 255, 256, 511, 512, 130, 385, 386, 699, 129], 4)])
    keep = np.unique(r * I + c, return_index=True)[1]
    r, c = r[keep], c[keep]
    W = sp.csc_matrix((_signed_weights(rng, len(r)), (r, c)), shape=(I, I))
    W.sort_indices()
    lens = [45, 30, 0, 60, 1, 25, 40, 33, 52, 28, 37, 44, 31]
    cols = [np.sort(rng.choice(I, n, replace=False)) for n in lens]
    for k in (0, 3, 6, 9):
        if EX_WIDE_ROW not in cols[k]:
            cols[k] = np.sort(np.concatenate([cols[k][1:], [EX_WIDE_ROW]]))
    cols[1] = np.concatenate([cols[1], [I + 5]])             # an item newer than W: ignored
    cols[3] = np.concatenate([cols[3], [I, I + 5]])
    lens = [len(x) for x in cols]
    X = sp.csr_matrix((_signed_ratings(rng, sum(lens)), np.concatenate(cols), np.concatenate([[0], np.cumsum(lens)])),
                      shape=(len(lens), I + 6))
    X.indices, X.indptr = X.indices.astype(np.int32), X.indptr.astype(np.int32)
    W.indices, W.indptr = W.indices.astype(np.int32), W.indptr.astype(np.int32)
    assert X.has_canonical_format and W.has_canonical_format and len(np.unique(cols[0])) == len(cols[0])
    frozen(X.data, X.indices, X.indptr, W.data, W.indices, W.indptr)
    return X, W


@functools.lru_cache(maxsize=None)
def export_scores(f64):
    """S[x row, column of W]: the sequential fold of section 1 over all rows of W; the last row is the zero row that a row id
    of -1 stands for."""
    X, W = export_data()
    S = np.zeros((X.shape[0] + 1, EX_ITEMS), dtype=np.float64 if f64 else np.float32)
    for u in range(X.shape[0]):
        a, b = X.indptr[u], X.indptr[u + 1]
        for c in range(EX_ITEMS):
            s, e = W.indptr[c], W.indptr[c + 1]
            S[u, c] = fold_column(X.indices[a:b], X.data[a:b], W.indices[s:e], W.data[s:e], f64)
    return frozen(S)[0]


def export_row_ids(n_rows):
    """A subset of the rows of X with repeats and -1 (a zero row)."""
    rid = np.random.default_rng(n_rows).integers(0, export_data()[0].shape[0], n_rows).astype(np.int32)
    if n_rows >= 3:
        rid[1], rid[n_rows - 1] = -1, rid[0]
    return rid


def export_image(layout, n_rows, row_ids, stride, f64, tail, no_t0=False, no_col_offset=False, full_last_tile=False):
    """What the output buffer of rtrec_slim_score_rows must hold, sentinels included: n_rows * stride words and `tail` more.
    The keyword arguments are the mutations of the host file."""
    lo, hi = EX_LAYOUTS[layout]
    n_cols, S = hi - lo, export_scores(f64)
    img = np.full(n_rows * stride + tail, SENTINEL_SCORE, dtype=S.dtype)
    for row in range(n_rows):
        xr = row if row_ids is None else int(row_ids[row])
        for t0 in range(0, n_cols, EX_TILE):
            ncol = min(EX_TILE, n_cols - t0)
            at = row * stride + (0 if no_t0 else t0)
            if full_last_tile and ncol < EX_TILE:           # the accumulators behind the last column hold +0
                spill = img[at + ncol:at + EX_TILE]
                own = (np.arange(at + ncol, at + ncol + len(spill)) % stride) < n_cols
                spill[~own | (spill == SENTINEL_SCORE)] = 0.0
            first = t0 if no_col_offset else lo + t0
            img[at:at + ncol] = S[xr, first:first + ncol]
    return img


def run_export(be, layout, n_rows, row_ids, stride, f64, tail, tile_cols=None, n_tiles=None):
    import torch
    from rtrec_amd.layouts import build_tiled_w
    X, W = export_data()
    lo, hi = EX_LAYOUTS[layout]
    T = build_tiled_w(W, lo, hi, EX_TILE)
    assert (T.tile_cols, T.n_cols, T.n_tiles) == (EX_TILE, hi - lo, -(-(hi - lo) // EX_TILE)) and T.dense_idx is None
    d = [dev(be, a) for a in (row_ids, X.indptr, X.indices, X.data, T.tile_ptr, T.w_col.view(np.int16), T.w_val)]
    out = torch.full((n_rows * stride + tail,), SENTINEL_SCORE, dtype=torch.float64 if f64 else torch.float32, device=be.device)
    rc = be.lib.rtrec_slim_score_rows(n_rows, be.ptr(d[0]), be.ptr(d[1]), be.ptr(d[2]), be.ptr(d[3]), EX_ITEMS, T.n_cols, lo,
                                      T.tile_cols if tile_cols is None else tile_cols, T.n_tiles if n_tiles is None else n_tiles,
                                      be.ptr(d[4]), be.ptr(d[5]), be.ptr(d[6]), int(f64), be.ptr(out), stride, be.stream())
    be.synchronize()
    return rc, out.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                 b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


def export_cases(layout):
    lo, hi = EX_LAYOUTS[layout]
    return [(n, rid, (hi - lo) + gap) for n in EX_ROWS for rid in (None, export_row_ids(n)) for gap in (0, EX_GAP)]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", list(EX_LAYOUTS))
def test_score_rows_equal_model(engine, layout, f64):
    """Three tiles with a ragged last one, exactly one tile, a last tile of one column; a column shard (col_offset 130); job
    counts that are no multiple of 8; an output stride beyond n_cols whose gap words must survive; row ids with repeats and
    -1; a user item beyond the rows of W; a row of W with more than 64 entries in one tile."""
    for n_rows, rid, stride in export_cases(layout):
        rc, out = run_export(engine.be, layout, n_rows, rid, stride, f64, tail=64)
        assert rc == RTREC_OK
        want = export_image(layout, n_rows, rid, stride, f64, tail=64)
        bad = np.flatnonzero(out.view(np.uint8).reshape(len(out), -1) != want.view(np.uint8).reshape(len(want), -1))
        assert same_bits(out, want), (f"{n_rows} rows, stride {stride}, row ids {rid}: {bad.size} bytes differ, first at word "
                                      f"{bad[0] // out.itemsize}: {out[bad[0] // out.itemsize]} vs {want[bad[0] // out.itemsize]}")


def test_score_rows_argument_checks_leave_the_output_alone(engine):
    be = engine.be
    n_cols = 700
    for kw, stride, want in ((dict(tile_cols=128), n_cols, RTREC_ERR_UNSUPPORTED), (dict(tile_cols=300), n_cols, RTREC_ERR_UNSUPPORTED),
                             (dict(n_tiles=2), n_cols, RTREC_ERR_INVALID_ARG), (dict(n_tiles=4), n_cols, RTREC_ERR_INVALID_ARG),
                             (dict(), n_cols - 1, RTREC_ERR_INVALID_ARG)):
        rc, out = run_export(be, "whole", 3, None, stride, False, tail=64, **kw)
        assert rc == want and (out == np.float32(SENTINEL_SCORE)).all(), (kw, stride)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_engine_predict_over_three_tiles(f64):
    """SlimEngine(tile_cols=256).predict_csr on the 700-item W: the multi-tile plumbing of _layout(compact=False)."""
    from rtrec_amd.engine import SlimEngine
    X, W = export_data()
    W = writable(W)
    eng = SlimEngine(device="cuda:0", tile_cols=EX_TILE)
    eng.set_weights(W.astype(np.float64) if f64 else W, acc_f64=f64)
    got = eng.predict_csr(X[:, :EX_ITEMS].tocsr())
    assert same_bits(np.ascontiguousarray(got), np.ascontiguousarray(export_scores(f64)[:X.shape[0]]))


# ======================================================================================================================
# 4. ingest fold
# ======================================================================================================================
FOLD_RUNS = [1, 2, 7, 8, 9, 15, 16, 17, 64, 1000]           # both sides of the eight-at-a-time loop, and a long run
FOLD_BOUNDS = [(-3.0, 10.0), (0.0, 0.0), (-np.inf, np.inf)]
FOLD_FLAVOURS = ["ints", "nan", "infs", "negzero", "overflow", "f32edge", "fractions"]
FOLD_OLD = [1.5, 50.0, -20.0, np.nan, -0.0, 10.0, -3.0, 0.25, np.inf, 2.0 ** 24]      # stored values, some outside every bound


@functools.lru_cache(maxsize=None)
def fold_batch():
    """(order, start, delta, tstamp, old): one pair per (run length, flavour); the arrival order is a random interleaving."""
    rng = np.random.default_rng(8)
    runs = []
    for n in FOLD_RUNS:
        for fl in FOLD_FLAVOURS:
            d = rng.integers(-4, 9, n).astype(np.float64)
            if fl == "nan":
                d[rng.random(n) < 0.3] = np.nan
                d[-1] = np.nan if n % 2 else d[-1]
            elif fl == "infs" and n >= 2:
                k = int(rng.integers(0, n - 1))
                d[k], d[k + 1] = np.inf, -np.inf                # adjacent: with infinite bounds the sum is NaN and ends as lo
                d[0 if k else n - 1] = -np.inf if n % 2 else np.inf
            elif fl == "negzero":
                d[:] = -0.0
            elif fl == "overflow":
                d = d * 1e300
                d[[0, -1]] = 1e308
                if n >= 2:
                    d[1] = 1e308                                # 1e308 twice: the sum overflows
            elif fl == "f32edge":
                d = rng.choice([2.0 ** 24 + 1, -(2.0 ** 24 + 1), 2.0 ** 24 + 3, 1.0, 2.0 ** -30, 2.0 ** 25 + 2], n)
            elif fl == "fractions":
                d = rng.uniform(-2, 3, n)
            runs.append(d)
    lens = np.array([len(d) for d in runs])
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(start[-1])
    slots = rng.permutation(N)
    order = np.concatenate([np.sort(slots[start[g]:start[g + 1]]) for g in range(len(runs))]).astype(np.int64)
    delta = np.empty(N)
    delta[order] = np.concatenate(runs)
    tstamp = 1.7e9 + rng.permutation(N).astype(np.float64)
    old = np.array([FOLD_OLD[(g * 3 + g // len(FOLD_FLAVOURS)) % len(FOLD_OLD)] for g in range(len(runs))])
    neg = [g for g in range(len(runs)) if FOLD_FLAVOURS[g % len(FOLD_FLAVOURS)] == "negzero"]
    old[neg[::2]] = -0.0                                        # (-0) + (-0) stays -0
    return frozen(order, start, delta, tstamp, old)


def fold_model(order, start, delta, tstamp, old, lo, hi, upsert, clip_swapped=False, drop_tail=False):
    """numpy_fold of tests/test_host_logic.py (the reference's own line max(lo, min(v + d, hi)) per occurrence) as arrays:
    (float64 values, timestamps, float32 values).  Mutations: clip_swapped (a NaN sum ends as hi), drop_tail (the occurrences
    behind the last whole eight are left out)."""
    g = len(start) - 1
    val, ts = np.zeros(g), np.zeros(g)
    for k in range(g):
        v = 0.0 if old is None else float(old[k])
        q1 = int(start[k + 1])
        if drop_tail:
            q1 -= (q1 - int(start[k])) % 8
        for q in range(int(start[k]), q1):
            d = float(delta[order[q]])
            if upsert:
                v = d
            elif clip_swapped:
                v = min(hi, max(v + d, lo))
            else:
                v = max(lo, min(v + d, hi))
        if upsert:
            v = float(delta[order[start[k + 1] - 1]])
        val[k], ts[k] = v, tstamp[order[start[k + 1] - 1]]
    with np.errstate(all="ignore"):
        return val, ts, val.astype(np.float32)


def run_fold(be, order, start, delta, tstamp, old, lo, hi, upsert, with_v32, n_groups=None):
    import torch
    g = len(start) - 1
    d = [dev(be, a) for a in (order, start, delta, tstamp, old)]
    o_val = torch.full((g + GUARD_ROWS,), SENTINEL_SCORE, dtype=torch.float64, device=be.device)
    o_ts = torch.full((g + GUARD_ROWS,), SENTINEL_SCORE, dtype=torch.float64, device=be.device)
    o_v32 = torch.full((g + GUARD_ROWS,), SENTINEL_SCORE, dtype=torch.float32, device=be.device)
    rc = be.lib.rtrec_store_fold_device(be.ptr(d[0]), be.ptr(d[1]), g if n_groups is None else n_groups, be.ptr(d[2]), be.ptr(d[3]),
                                        be.ptr(d[4]), lo, hi, int(upsert), be.ptr(o_val), be.ptr(o_ts),
                                        be.ptr(o_v32 if with_v32 else None), be.stream())
    be.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (o_val, o_ts, o_v32))


@pytest.mark.parametrize("upsert", [False, True], ids=["add", "upsert"])
@pytest.mark.parametrize("with_old", [False, True], ids=["empty_store", "stored"])
@pytest.mark.parametrize("lo,hi", FOLD_BOUNDS, ids=["-3..10", "0..0", "unbounded"])
def test_ingest_fold_equals_model(engine, lo, hi, with_old, upsert):
    """Runs on both sides of the eight-at-a-time loop; NaN, +-inf (inf + -inf included), -0.0, a sum that overflows, values
    that float32 cannot hold; stored values outside the bounds; upsert keeps the last delta unclipped."""
    order, start, delta, tstamp, old = fold_batch()
    old = old if with_old else None
    g = len(start) - 1
    w_val, w_ts, w_v32 = fold_model(order, start, delta, tstamp, old, lo, hi, upsert)
    for with_v32 in (True, False):
        rc, val, ts, v32 = run_fold(engine.be, order, start, delta, tstamp, old, lo, hi, upsert, with_v32)
        assert rc == RTREC_OK
        assert (val[g:] == SENTINEL_SCORE).all() and (ts[g:] == SENTINEL_SCORE).all() and (v32[g:] == np.float32(SENTINEL_SCORE)).all()
        bad = np.flatnonzero(bits64(val[:g]) != bits64(w_val))
        assert bad.size == 0, f"values differ on pairs {bad[:8]}: {val[bad[:8]]} vs {w_val[bad[:8]]}"
        assert np.array_equal(bits64(ts[:g]), bits64(w_ts))
        if with_v32:
            bad = np.flatnonzero(bits(v32[:g]) != bits(w_v32))
            assert bad.size == 0, f"float32 values differ on pairs {bad[:8]}: {v32[bad[:8]]} vs {w_v32[bad[:8]]}"
        else:
            assert (v32 == np.float32(SENTINEL_SCORE)).all()


def test_ingest_fold_without_pairs(engine):
    order, start, delta, tstamp, old = fold_batch()
    rc, val, ts, v32 = run_fold(engine.be, order, start, delta, tstamp, old, -3.0, 10.0, False, True, n_groups=0)
    assert rc == RTREC_OK
    assert (val == SENTINEL_SCORE).all() and (ts == SENTINEL_SCORE).all() and (v32 == np.float32(SENTINEL_SCORE)).all()


# ======================================================================================================================
# 5. float64 refine: rows on both sides of the staging limit (kRfItems / rows per wave), searched in LDS or in global memory
# ======================================================================================================================
RF_ITEMS = 700
RF_COL_MAX = 30                # stored weights per column of W, at most
RF_STAGED = {10: 256, 3: 64}   # top_k -> staged items per row: 1,024 slots per wave over 64 / P rows, P = 16 and 4 lanes per row
RF_ROW_LENS = [0, 1, 63, 64, 65, 255, 256, 257, 600, 5, 17, 30]
RF_ROWS = 70                   # list rows per call: five workgroups at top_k 10 (16 rows each), two at top_k 3 (64 rows each)
RF_FOREIGN = 23                # the list row whose row id is no row of X


@functools.lru_cache(maxsize=None)
def refine_data():
    """(X [12, 700] CSR, W [700, 700] CSC), float32, continuous positive values: no two float64 sums tie unless both are 0."""
    rng = np.random.default_rng(41)
    cols = [np.sort(rng.choice(RF_ITEMS, n, replace=False)) for n in RF_ROW_LENS]
    ptr = np.concatenate([[0], np.cumsum(RF_ROW_LENS)])
    X = sp.csr_matrix((rng.uniform(0.5, 5.0, ptr[-1]).astype(np.float32), np.concatenate(cols).astype(np.int32), ptr.astype(np.int32)),
                      shape=(len(RF_ROW_LENS), RF_ITEMS))
    col_len = rng.integers(0, RF_COL_MAX + 1, RF_ITEMS)
    wrows = [np.sort(rng.choice(RF_ITEMS, n, replace=False)) for n in col_len]
    wptr = np.concatenate([[0], np.cumsum(col_len)])
    W = sp.csc_matrix((rng.uniform(0.01, 1.0, wptr[-1]).astype(np.float32), np.concatenate(wrows).astype(np.int32), wptr.astype(np.int32)),
                      shape=(RF_ITEMS, RF_ITEMS))
    frozen(X.data, X.indices, X.indptr, W.data, W.indices, W.indptr)
    return X, W


@functools.lru_cache(maxsize=None)
def refine_case(top_k):
    """(row_ids [70], in_ids [70, top_k + 1], in_count [70]): every row of X several times, neighbours of a wave on different
    sides of the staging limit, one row id outside the matrix; top_k + 1 distinct columns per list in no order, and lists that
    are empty, hold one entry, top_k - 1 or top_k entries instead of all top_k + 1."""
    rng = np.random.default_rng([43, top_k])
    n_x, kin = len(RF_ROW_LENS), top_k + 1
    row_ids = np.concatenate([rng.permutation(n_x) for _ in range(RF_ROWS // n_x + 1)])[:RF_ROWS].astype(np.int32)
    row_ids[RF_FOREIGN] = n_x
    in_ids = np.stack([rng.choice(RF_ITEMS, kin, replace=False) for _ in range(RF_ROWS)]).astype(np.int32)
    in_count = np.full(RF_ROWS, kin, dtype=np.int32)
    in_count[[3, 18, 37, 52, 66]] = [0, 1, top_k - 1, top_k, 2]
    return frozen(row_ids, in_ids, in_count)


def refine_model(top_k, cap=None, **mut):
    """The lists rtrec_slim_refine_topk_f64 writes: (ids [R, top_k], float32 scores, float64 scores, counts).  Per list entry the
    float64 sum of double(x) * double(w) over the column's entries in ascending order (fold_column), the entries by (score
    descending, list position ascending), slots behind the count -1 / -inf.  Mutations of the host file: cap (only the first
    `cap` items of a longer row are seen), **mut (fold_column)."""
    X, W = refine_data()
    row_ids, in_ids, in_count = refine_case(top_k)
    R = len(row_ids)
    o_ids = np.full((R, top_k), -1, dtype=np.int32)
    o_sc = np.full((R, top_k), -np.inf, dtype=np.float32)
    o_sc64 = np.full((R, top_k), -np.inf, dtype=np.float64)
    o_cnt = np.zeros(R, dtype=np.int32)
    for r, xr in enumerate(row_ids.tolist()):
        a, b = (X.indptr[xr], X.indptr[xr + 1]) if 0 <= xr < X.shape[0] else (0, 0)
        if cap is not None and b - a > cap:
            b = a + cap
        n = min(int(in_count[r]), top_k + 1)
        sc = [fold_column(X.indices[a:b], X.data[a:b], W.indices[W.indptr[c]:W.indptr[c + 1]], W.data[W.indptr[c]:W.indptr[c + 1]], True,
                          **mut) for c in in_ids[r, :n].tolist()]
        best = sorted(range(n), key=lambda p: (-sc[p], p))[:top_k]
        o_cnt[r] = len(best)
        for j, p in enumerate(best):
            o_ids[r, j], o_sc[r, j], o_sc64[r, j] = in_ids[r, p], np.float32(sc[p]), sc[p]
    return o_ids, o_sc, o_sc64, o_cnt


def run_refine(be, top_k):
    """(ids, float32 scores, float64 scores, counts) of one call of the op; the outputs have GUARD_ROWS rows more than the call
    may write and start as sentinels."""
    import torch
    X, W = refine_data()
    row_ids, in_ids, in_count = refine_case(top_k)
    R = len(row_ids)
    d = [dev(be, a) for a in (row_ids, X.indptr, X.indices, X.data, W.indptr, W.indices, W.data, in_ids, in_count)]
    in_sc = torch.zeros((R, top_k + 1), dtype=torch.float32, device=be.device)      # read by the margin test only (not asserted)
    o_ids = torch.full((R + GUARD_ROWS, top_k), SENTINEL_ID, dtype=torch.int32, device=be.device)
    o_sc = torch.full((R + GUARD_ROWS, top_k), SENTINEL_SCORE, dtype=torch.float32, device=be.device)
    o_sc64 = torch.full((R + GUARD_ROWS, top_k), SENTINEL_SCORE, dtype=torch.float64, device=be.device)
    o_cnt = torch.full((R + GUARD_ROWS,), SENTINEL_CNT, dtype=torch.int32, device=be.device)
    flagged = torch.zeros((R + 1,), dtype=torch.int32, device=be.device)            # [0]: the counter; a slot for every row
    be.ops.refine_topk_f64(d[0], d[1], d[2], d[3], R, RF_ITEMS, d[4], d[5], d[6], top_k, d[7], in_sc, d[8], 2.0 ** -20, None,
                           o_ids, o_sc, o_sc64, o_cnt, flagged)
    be.synchronize()
    return tuple(t.cpu().numpy() for t in (o_ids, o_sc, o_sc64, o_cnt))


@pytest.mark.parametrize("top_k", sorted(RF_STAGED, reverse=True))
def test_refine_equals_model_on_both_sides_of_the_staging_limit(engine, top_k):
    """Rows of 0 .. 600 items with 64 (top_k 3) or 256 (top_k 10) staged items per row: the longer ones are searched in global
    memory, the others in LDS, side by side in one wave.  ids, float32 and float64 score bits and counts equal the model; what
    the call flags is the margin test's business (tests/test_gpu_seg.py) and not looked at."""
    g_ids, g_sc, g_sc64, g_cnt = run_refine(engine.be, top_k)
    w_ids, w_sc, w_sc64, w_cnt = refine_model(top_k)
    R = len(w_cnt)
    assert all_sentinels(g_ids[R:], g_sc[R:], g_sc64[R:], g_cnt[R:]), "written behind the last row"
    assert np.array_equal(g_cnt[:R], w_cnt), f"counts {g_cnt[:R]} vs {w_cnt}"
    bad = np.flatnonzero((g_ids[:R] != w_ids).any(axis=1))
    assert bad.size == 0, f"ids differ on rows {bad[:8]}, first: {g_ids[bad[0]]} vs {w_ids[bad[0]]}"
    bad = np.flatnonzero((bits64(g_sc64[:R]) != bits64(w_sc64)).any(axis=1))
    assert bad.size == 0, f"float64 bits differ on rows {bad[:8]}, first: {g_sc64[bad[0]]} vs {w_sc64[bad[0]]}"
    bad = np.flatnonzero((bits(g_sc[:R]) != bits(w_sc)).any(axis=1))
    assert bad.size == 0, f"float32 bits differ on rows {bad[:8]}, first: {g_sc[bad[0]]} vs {w_sc[bad[0]]}"

