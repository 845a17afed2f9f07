"""The hybrid's similar_items on the GPU (csrc/factor_norms.hip, factor_similar.hip, similar_blend.hip; torch.ops.rtrec_amd.
factor_norms / factor_similar_topk / similar_blend; SLIM.similar_items_factor_batch / similar_items_hybrid_batch) against the host
models of tests/test_similar_host.py: ids, sources and counts with ==, float32 scores and float64 values by their bits after
adding +0.0 (the sign of a zero is not part of the contract).  The output buffers are poisoned before every call (every slot
must be written)."""
import numpy as np
import pytest

from tests.test_factor_host import CLASS_DIMS, F32, GRID_CAP, PATTERNS, pattern_of, rounding_vectors, tiled
from tests.test_similar_host import (FLT_MAX, assert_same_blend, assert_same_lists, blend_trip_case, caller_norms_case, check_serving_and_facade,
                                     check_similar_api, golden_answer, golden_cases, golden_inputs, host_blend, host_norms_fast,
                                     host_norms_plain, host_similar_fast, lists_of, one_scan_cases, query_norms_case, same_or_both_nan,
                                     similar_class_case, similar_operand_case, similar_trip_case, special_vectors, dbits)

pytestmark = pytest.mark.gpu


def _up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")


# ---------------------------------------------------------------------------------------------- 1. norms
def run_norms(V, component_major, pad, seed=0):
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    V = np.asarray(V, F32)
    n, dim = V.shape
    rng = np.random.default_rng(seed)
    if component_major:
        M = (rng.standard_normal((dim, n + pad)) * 100).astype(F32)
        M[:, :n] = V.T
        rs, cs = 1, n + pad
    else:
        M = (rng.standard_normal((n, dim + pad)) * 100).astype(F32)
        M[:, :dim] = V
        rs, cs = dim + pad, 1
    out = torch.full((n,), 7.0, dtype=torch.float32, device="cuda:0")
    torch.ops.rtrec_amd.factor_norms(_up(M, np.float32), n, dim, rs, cs, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dim", [1, 2, 3, 13, 64, 256])
def test_norms_are_the_chain_and_a_correctly_rounded_root_bit_for_bit(dim):
    V = special_vectors(97, dim, seed=dim)
    want = host_norms_fast(V)
    assert np.array_equal(want[:12].view(np.int32), host_norms_plain(V[:12]).view(np.int32))
    assert want[1] == 0 and 0 < want[3] and np.isinf(want[5])
    with np.errstate(all="ignore"):
        n2 = (V[3].astype(np.float64) ** 2).sum()
    assert 0 < n2 < 2.0 ** -126, "vector 3 must have a denormal sum of squares"
    for component_major in (False, True):
        for pad in (0, 5):
            got = run_norms(V, component_major, pad)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (dim, component_major, pad, np.flatnonzero(got != want)[:5])


# ---------------------------------------------------------------------------------------------- 2. the cosine top-k
def run_similar(Q, norms, queries, top_k, P=None, p_norms=None, mask=None, write_cosine=False, splits=0, pad=0, want_div=True, seed=0,
                pad_value=None):
    """torch.ops.rtrec_amd.factor_similar_topk on host arrays, as the host models take them.  `pad` > 0: the strides are wider
    than the widths (and qt has rows beyond dim), with seeded values behind them, or `pad_value` in all three places (qt's rows
    beyond dim, qt's columns beyond n_items, p's columns beyond dim)."""
    import torch
    from rtrec_amd import ops  # noqa: F401
    Q = np.asarray(Q, F32)
    n_items, dim = Q.shape
    rng = np.random.default_rng(seed)
    behind = lambda *shape: rng.standard_normal(shape).astype(F32) * 100 if pad_value is None else np.full(shape, pad_value, F32)
    Qt = np.ascontiguousarray(Q.T)
    if pad:
        Qt = np.concatenate([Qt, behind(dim, pad)], axis=1)
        Qt = np.concatenate([Qt, behind(pad, n_items + pad)], axis=0)
    n = len(P) if P is not None else len(queries)
    ids = torch.full((n, top_k), 12345, dtype=torch.int32, device="cuda:0")               # poisoned: every slot must be written
    scores = torch.full((n, top_k), 7.0, dtype=torch.float32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    div = torch.full((n,), -7.0, dtype=torch.float32, device="cuda:0") if want_div else None
    s_eff = splits if splits else 64
    ws = torch.empty((n * s_eff * (top_k * 8 + 4),), dtype=torch.uint8, device="cuda:0") if s_eff > 1 else None
    d_p = d_pn = None
    if P is not None:
        Pd = np.asarray(P, F32)
        if pad:
            Pd = np.concatenate([Pd, behind(n, pad)], axis=1)
        d_p, d_pn = _up(Pd, np.float32), _up(p_norms, np.float32)
    torch.ops.rtrec_amd.factor_similar_topk(None if queries is None else _up(queries, np.int32), d_p, d_pn, _up(Qt, np.float32), n_items, dim,
                                            _up(norms, np.float32), None if mask is None else _up(np.asarray(mask) != 0, np.uint8), top_k,
                                            splits, bool(write_cosine), ids, scores, count, div, ws)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy(), None if div is None else div.cpu().numpy()


def same(got, want, what):
    assert_same_lists(got, want, what)
    if got[3] is not None:
        assert np.array_equal(got[3].view(np.int32), np.asarray(want[3], F32).view(np.int32)), (what, "div")


def test_operand_map_on_an_asymmetric_integer_matrix():
    """A swapped row / column of the tile, a permuted k or a norm taken from the wrong item would show: the integer matrix is not
    symmetric in any pair of its indices; the queries read from qt's columns and the same vectors brought as p give the same bits."""
    dim, n_items = 32, 40
    i, c = np.meshgrid(np.arange(n_items), np.arange(dim), indexing="ij")
    Q = (i * 37 + c * 3 + (i * c) % 5 - 400).astype(F32)
    norms = host_norms_fast(Q)
    queries = np.r_[np.arange(n_items), [3]].astype(np.int32)                 # 41 jobs: two workgroups
    want = host_similar_fast(Q, norms, queries, n_items)
    assert (want[2] == n_items - 1).all()
    for splits in (1, 2):
        got = run_similar(Q, norms, queries, n_items, splits=splits)
        same(got, want, f"columns, {splits} chunk(s)")
        brought = run_similar(Q, norms, queries, n_items, P=Q[queries], p_norms=norms[queries], splits=splits, pad=3)
        same(brought, want, f"brought, {splits} chunk(s)")
    for r, q in enumerate(queries):
        assert q not in got[0][r].tolist() and got[0][r, -1] == -1 and np.isneginf(got[1][r, -1])


@pytest.mark.parametrize("dim", [1, 2, 3, 12, 13, 64, 255, 256] + CLASS_DIMS)
def test_every_s1_is_the_chain_and_one_division_bit_for_bit(dim):
    """Every s1 of 96 x 95 pairs must carry the bits of fl(chain / norm) on vectors where another order, an unfused multiply, a
    reciprocal or a wider accumulator changes them (tests/test_similar_host.py counts how often they do)."""
    _, Q = rounding_vectors(1, 96, dim, seed=dim)
    Q[5] = 0.0                                                                # a zero vector: never listed, and as a query empty with write_cosine
    norms = host_norms_fast(Q)
    queries = np.arange(96, dtype=np.int32)
    want = host_similar_fast(Q, norms, queries, 95)
    got = run_similar(Q, norms, queries, 95, splits=1)
    same(got, want, f"dim {dim}")
    assert not (got[0] == 5).any()
    cos = run_similar(Q, norms, queries, 95, splits=1, write_cosine=True)
    same(cos, host_similar_fast(Q, norms, queries, 95, write_cosine=True), f"dim {dim} cosine")
    assert cos[2][5] == 0 and (cos[0][5] == -1).all()


def test_s1_bits_beyond_one_compaction():
    """130 items: at top_k 64 the 128-entry buffer is compacted before the last tile."""
    _, Q = rounding_vectors(1, 130, 12, seed=77)
    norms = host_norms_fast(Q)
    queries = np.arange(130, dtype=np.int32)
    for top_k in (64, 128):
        want = host_similar_fast(Q, norms, queries, top_k)
        for splits in (1, 3):
            same(run_similar(Q, norms, queries, top_k, splits=splits), want, (top_k, splits))


@pytest.fixture(scope="module")
def selection_case():
    rng = np.random.default_rng(55)
    Q = rng.standard_normal((2100, 9)).astype(F32)
    Q[[4, 700, 2099]] = 0.0                                                   # zero-norm items
    norms = host_norms_fast(Q)
    mask = (rng.random(2100) < 0.8).astype(np.uint8)
    return Q, norms, mask


@pytest.mark.parametrize("n_items", [70, 2100])
def test_selection_chunks_mask_query_and_every_top_k(selection_case, n_items):
    """33 queries (two workgroups) over 70 and 2,100 items -- more than 64 tiles, so item_splits = 0 really chunks; item_splits
    1, 2 and 0 give identical outputs; the query is never listed; a mask; zero-norm items; top_k beyond n_items - 1."""
    Q, norms, mask = selection_case[0][:n_items], selection_case[1][:n_items], selection_case[2][:n_items]
    queries = np.r_[np.arange(0, n_items, max(1, n_items // 31))[:31], [4, n_items - 1]].astype(np.int32)
    assert len(queries) == 33
    for kw in (dict(), dict(mask=mask), dict(write_cosine=True)):
        want = host_similar_fast(Q, norms, queries, 128, **kw)
        for top_k in ((1, 10, 16, 17, 64, 65, 128) if not kw else (10, 128)):
            w = (want[0][:, :top_k], want[1][:, :top_k], np.minimum(want[2], top_k), want[3])
            base = None
            for splits in (1, 2, 0):
                got = run_similar(Q, norms, queries, top_k, splits=splits, pad=2 if splits == 2 else 0, **kw)
                same(got, w, (n_items, top_k, splits, sorted(kw)))
                base = got if base is None else base
                assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[:3], base[:3]))
            for r, q in enumerate(queries):
                assert q not in got[0][r].tolist()
            assert not np.isin(got[0], [4, 700, 2099]).any()
    if n_items == 70:
        assert (want[2][np.flatnonzero(queries != 4)] <= 69).all() and want[2].max() < 128      # top_k beyond n_items - 1


def test_ties_unknown_queries_and_the_two_ways_to_divide():
    Q = np.tile(np.array([[1.0, 2.0, 2.0]], F32), (3000, 1))                  # every s1 is equal: ids 0 .. top_k-1 without the query
    norms = host_norms_fast(Q)
    queries = np.array([0, 5, 2999, -1, 3000, 17], np.int32)
    for top_k, splits in ((128, 0), (128, 1), (10, 3)):
        want = host_similar_fast(Q, norms, queries, top_k, write_cosine=True)
        got = run_similar(Q, norms, queries, top_k, write_cosine=True, splits=splits)
        same(got, want, (top_k, splits))
        assert got[0][1, :6].tolist() == [0, 1, 2, 3, 4, 6] and got[2].tolist() == [top_k, top_k, top_k, 0, 0, top_k] and (got[1][0] == 1.0).all()
    # q = -1 with brought vectors excludes nothing; no queries at all with brought vectors
    rng = np.random.default_rng(8)
    Q = rng.standard_normal((200, 6)).astype(F32)
    norms = host_norms_fast(Q)
    P = rng.standard_normal((5, 6)).astype(F32)
    P[3] = 0.0
    pn = host_norms_fast(P)
    for queries in (np.array([-1, 7, -1, 9, 200], np.int32), None):
        for cosine in (False, True):
            want = host_similar_fast(Q, norms, queries, 12, P=P, p_norms=pn, write_cosine=cosine)
            same(run_similar(Q, norms, queries, 12, P=P, p_norms=pn, write_cosine=cosine, splits=2), want, (queries is None, cosine))
            assert want[2][0] == 12 and (want[2][3] == (0 if cosine else 12))
    # write_cosine against d_out_div: the same lists, the written score divided by what out_div reports
    queries = np.arange(40, dtype=np.int32)
    s1 = run_similar(Q, norms, queries, 10, splits=1)
    cos = run_similar(Q, norms, queries, 10, write_cosine=True, splits=4)
    assert np.array_equal(s1[0], cos[0]) and np.array_equal(s1[3], norms[:40]) and np.array_equal(cos[3], norms[:40])
    assert np.array_equal((s1[1] / s1[3][:, None]).view(np.int32), cos[1].view(np.int32))


def test_the_two_entry_points_run_the_same_scan():
    """The two kernels are one scan written twice (csrc/factor_scan.hip.h says why).  Unit item norms, no queries, no mask, no
    cosine: factor_similar_topk must return factor_topk's ids, counts and score bits (x / 1.0f is exact), and both the host
    model's (tests/test_similar_host.py, one_scan_cases, shows the premise on the host)."""
    from tests.test_factor_host import assert_same
    from tests.test_gpu_factor import run_op
    for name, P, Q, p_norms, want in one_scan_cases():
        ones = np.ones(len(Q), F32)
        for top_k in (10, 128):
            for splits in (1, 3):
                sim = run_similar(Q, ones, None, top_k, P=P, p_norms=p_norms, splits=splits)
                top = run_op(P, Q, top_k, splits=splits)
                what = (name, top_k, splits)
                assert np.array_equal(sim[0], top[0]) and np.array_equal(sim[2], top[2]), what
                assert np.array_equal(sim[1].view(np.int32), top[1].view(np.int32)) and np.array_equal(sim[3], p_norms), what
                assert_same(top, want[top_k], what)
                assert_same(sim[:3], want[top_k], what)


# ---------------------------------------------------------------------------------------------- 2b. class edges, padding, norms, second trips
@pytest.mark.parametrize("dim", [17, 65])
def test_both_class_choices_change_in_one_similar_call(dim):
    """200 items, 40 queries one past a dim class at top_k one past a k class, in one chunk and in three, with the cosine
    division; the last component decides every list (tests/test_similar_host.py)."""
    Q, norms, queries = similar_class_case(dim)
    for cosine in (False, True):
        want = host_similar_fast(Q, norms, queries, 65, write_cosine=cosine)
        for top_k in (17, 65):
            w = (want[0][:, :top_k], want[1][:, :top_k], np.minimum(want[2], top_k), want[3])
            for splits in (1, 3):
                same(run_similar(Q, norms, queries, top_k, write_cosine=cosine, splits=splits), w, (dim, top_k, splits, cosine))


@pytest.mark.parametrize("dim", [13, 33])
def test_nan_padding_is_never_read_into_an_s1(dim):
    """The operand-map case with NaN in qt's rows beyond dim, in qt's columns beyond n_items and in the brought vectors' columns
    beyond dim (tests/test_gpu_factor.py says why NaN, why odd dims and why 32 rows); the expected answer is the unpadded one."""
    from tests.test_gpu_factor import NAN_PAD
    Q, norms, queries = similar_operand_case(dim)
    want = host_similar_fast(Q, norms, queries, 40)
    for splits in (1, 2):
        same(run_similar(Q, norms, queries, 40, splits=splits, pad=NAN_PAD, pad_value=np.nan), want, ("columns", splits))
        same(run_similar(Q, norms, queries, 40, P=Q[queries], p_norms=norms[queries], splits=splits, pad=NAN_PAD, pad_value=np.nan), want,
             ("brought", splits))


def test_the_similar_merge_serves_more_jobs_than_its_grid():
    """65,536 + 40 jobs in two chunks with write_cosine: the merge's grid is capped at 65,536 workgroups, and across the cap live
    queries meet zero-norm and unknown ones in both orders (tests/test_similar_host.py, similar_trip_case) -- `live` and `total`
    of a workgroup's first job must not reach its second.  Once with the queries' own columns, once with brought vectors."""
    case = similar_trip_case()
    Q, norms, at, n_rows = case["Q"], case["norms"], case["at"], case["n_rows"]
    assert n_rows > GRID_CAP
    want = host_similar_fast(Q, norms, case["queries"], 3, write_cosine=True)
    same(run_similar(Q, norms, case["queries"][at], 3, write_cosine=True, splits=2), tiled(want, n_rows), "queries")
    want = host_similar_fast(Q, norms, case["queries"], 3, P=case["P"], p_norms=case["p_norms"], write_cosine=True)
    got = run_similar(Q, norms, case["queries"][at], 3, P=case["P"][at], p_norms=case["p_norms"][at], write_cosine=True, splits=2)
    same(got, tiled(want, n_rows), "brought")


@pytest.mark.parametrize("splits", [1, 3])
def test_item_and_query_norms_are_the_callers(splits):
    """NaN, +-inf, negative, -0.0 and denormal norms as divisors of s1 and as query norms (tests/test_similar_host.py,
    caller_norms_case / query_norms_case): "s1 is not NaN" decides who competes and "a norm that is not > 0 empties a cosine list"
    -- in the scan's epilogue (one chunk) and in the merge (three), which must agree with the host and so with each other."""
    Q, norms, queries, _ = caller_norms_case()
    for top_k in (20, 99):
        for cosine in (False, True):
            want = host_similar_fast(Q, norms, queries, top_k, write_cosine=cosine)
            same_or_both_nan(run_similar(Q, norms, queries, top_k, write_cosine=cosine, splits=splits), want, (top_k, cosine))
    Q, norms, P, p_norms = query_norms_case()
    for cosine in (False, True):
        want = host_similar_fast(Q, norms, None, 20, P=P, p_norms=p_norms, write_cosine=cosine)
        same_or_both_nan(run_similar(Q, norms, None, 20, P=P, p_norms=p_norms, write_cosine=cosine, splits=splits), want, ("brought", cosine))


@pytest.mark.parametrize("component_major", [False, True])
def test_norms_of_more_vectors_than_one_trip_of_the_grid(component_major):
    """65,536 workgroups x 256 threads + 300 vectors of dim 1: the last 300 are second trips.  The vectors repeat 509 patterns
    of special_vectors (zero, denormal squares, overflow), so vector r and vector r + 16,777,216 differ."""
    n = GRID_CAP * 256 + 300
    V = special_vectors(PATTERNS, 1, seed=1)
    want = host_norms_fast(V)
    assert want[1] == 0 and np.isinf(want[5]) and (GRID_CAP * 256) % PATTERNS != 0
    at = pattern_of(n)
    got = run_norms(V[at], component_major, 0)
    assert np.array_equal(got.view(np.int32), want[at].view(np.int32)), np.flatnonzero(got != want[at])[:5]


# ---------------------------------------------------------------------------------------------- 3. the blend
def run_blend(n_items, A, B, keep, a_div=None, exclude=None, waves=0, pad=0):
    import torch
    from rtrec_amd import ops  # noqa: F401
    R, ka, kb = len(A[0]), A[0].shape[1], B[0].shape[1]

    def wide(a, fill):
        return np.concatenate([a, np.full((R, pad), fill, a.dtype)], axis=1) if pad else a

    ids = torch.full((R, keep), 12345, dtype=torch.int32, device="cuda:0")               # poisoned: every slot must be written
    value = torch.full((R, keep), 7.0, dtype=torch.float64, device="cuda:0")
    source = torch.full((R, keep), 9, dtype=torch.int32, device="cuda:0")
    count = torch.full((R,), -7, dtype=torch.int32, device="cuda:0")
    torch.ops.rtrec_amd.similar_blend(n_items, _up(wide(A[0], 3), np.int32), _up(wide(A[1], F32(9.0)), np.float32), _up(A[2], np.int32), ka,
                                      None if a_div is None else _up(a_div, np.float32), _up(wide(B[0], 3), np.int32),
                                      _up(wide(B[1], F32(9.0)), np.float32), _up(B[2], np.int32), kb,
                                      None if exclude is None else _up(exclude, np.int32), keep, waves, ids, value, source, count)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), value.cpu().numpy(), source.cpu().numpy(), count.cpu().numpy()


def test_the_whole_golden_file_equals_the_reference():
    """One launch per (ka, kb) class: the 400 fixture queries (10 x 10) and the 60 small cases (up to 15 x 12), both wave counts."""
    g, cases = golden_cases()
    for lo, hi in ((0, g["n_fixture"]), (g["n_fixture"], len(cases))):
        part = cases[lo:hi]
        A, B, div, ex = golden_inputs(part)
        keep = max(c["top_k"] for c in part)
        n_items = part[0]["n_items"]
        want = host_blend(n_items, A, B, keep, a_div=div, exclude=ex)
        got = {w: run_blend(n_items, A, B, keep, a_div=div, exclude=ex, waves=w, pad=w) for w in (1, 4)}
        assert_same_blend(got[1], want, "golden, one wave")
        assert_same_blend(got[4], got[1], "golden, four waves")
        for r, c in enumerate(part):                       # ... and what the reference itself returned
            w_ids, w_val = golden_answer(c)
            n = len(w_ids)
            assert n == min(c["top_k"], got[1][3][r]) and got[1][0][r, :n].tolist() == w_ids, (lo + r)
            assert np.array_equal(dbits(got[1][1][r, :n]), dbits(w_val)), (lo + r)


@pytest.mark.parametrize("width", [1, 64, 65, 256, 257, 1024])
def test_blend_of_every_list_class_with_seeded_repeats(width):
    rng = np.random.default_rng(width)
    R, n_items = 6, max(8, width // 2)                      # ids drawn from half the width: every list repeats ids
    rows_a = [rng.integers(0, n_items, width).tolist() for _ in range(R)]
    rows_b = [rng.integers(0, n_items, max(1, width - r)).tolist() for r in range(R)]
    sc = lambda n: (-np.sort(-rng.standard_normal(n))).astype(F32).tolist()
    A = lists_of(rows_a, [sc(len(r)) for r in rows_a], width)
    B = lists_of(rows_b, [sc(len(r)) for r in rows_b], width)
    div = (np.abs(rng.standard_normal(R)) + 0.5).astype(F32)
    ex = rng.integers(-1, n_items, R).astype(np.int32)
    keep = min(2 * width, n_items + 3)
    want = host_blend(n_items, A, B, keep, a_div=div, exclude=ex)
    one = run_blend(n_items, A, B, keep, a_div=div, exclude=ex, waves=1)
    assert_same_blend(one, want, f"width {width}")
    assert_same_blend(run_blend(n_items, A, B, keep, a_div=div, exclude=ex, waves=4, pad=2), one, f"width {width}, four waves")
    assert_same_blend(run_blend(n_items, A, B, keep, a_div=div, exclude=ex, waves=0), one, f"width {width}, the library's choice")


def test_blend_contract_edges_on_the_device():
    none = lists_of([[]], [[]])
    one = lists_of([[4, 6, 2]], [[3.0, 2.0, 1.0]])
    flat = lists_of([[8, 1, 5]], [[0.7, 0.7, 0.7]])
    rep_a, rep_b = lists_of([[3, 3, 9]], [[4.0, 2.0, 0.0]]), lists_of([[9, 9, 3]], [[1.0, 0.5, 0.0]])
    A, B = lists_of([[5, 2, 7]], [[9.0, 2.0, 1.0]]), lists_of([[7, 5, 1]], [[3.0, 2.0, 1.0]])
    cut_a, cut_b = lists_of([[5, 2, 7, 8]], [[9.0, 2.0, -FLT_MAX, 1.0]]), lists_of([[7, 24, 1]], [[3.0, 2.0, 1.0]])
    big = lists_of([[5, 2]], [[3.0e38, -3.0e38]])
    for waves in (1, 4):
        for a, b, keep, kw in ((none, none, 2, {}), (one, none, 4, {}), (none, one, 3, {}), (flat, flat, 6, {}), (rep_a, rep_b, 6, {}),
                               (A, B, 6, dict(exclude=np.array([5], np.int32))), (A, B, 6, dict(exclude=np.array([-1], np.int32))),
                               (A, B, 6, dict(a_div=np.array([0.0], F32))), (A, B, 6, dict(a_div=np.array([-2.0], F32))),
                               (A, B, 6, dict(a_div=np.array([np.nan], F32))), (A, B, 6, dict(a_div=np.array([4.0], F32))),
                               (cut_a, cut_b, 6, dict(a_div=np.array([1e-30], F32))), ((cut_a[0], cut_a[1], np.array([1], np.int32)), cut_b, 6, {}),
                               ((cut_a[0], cut_a[1], np.array([-3], np.int32)), (cut_b[0], cut_b[1], np.array([99], np.int32)), 6, {}),
                               (big, none, 3, {}), (one, one, 6, {})):
            want = host_blend(24, a, b, keep, **kw)
            got = run_blend(24, a, b, keep, waves=waves, **kw)
            assert_same_blend(got, want, (waves, keep, sorted(kw)))
            assert not np.isnan(got[1]).any()


@pytest.mark.parametrize("waves", [1, 4])
def test_the_blend_serves_more_rows_than_its_grid(waves):
    """65,536 + 3 rows: the list stage's grid is capped at 65,536 workgroups, so the last three rows are second trips, and
    across the cap a long union follows a short one and the reverse (tests/test_similar_host.py, blend_trip_case): holes, values
    and lengths of a workgroup's first row must not reach its second."""
    n_items, A, B, a_div, exclude, _ = blend_trip_case()
    want = host_blend(n_items, A, B, 5, a_div=a_div, exclude=exclude)
    n_rows = GRID_CAP + 3
    at = pattern_of(n_rows)
    got = run_blend(n_items, tuple(a[at] for a in A), tuple(b[at] for b in B), 5, a_div=a_div[at], exclude=exclude[at], waves=waves)
    assert_same_blend(got, tiled(want, n_rows), f"second trip, {waves} wave(s)")


# ---------------------------------------------------------------------------------------------- 4. the API on the device
def gpu_model(strings=False):
    from tests.test_factor_host import fitted_model
    return fitted_model(strings, cpu=False)


@pytest.mark.parametrize("strings", [False, True])
def test_similar_items_factor_and_hybrid_batch_equal_the_host_path(strings):
    """Every item of the golden fixture model as a query: host top-k -> host SLIM similar -> host blend, with finished vectors and
    with feature tables, with and without biases; query_items_tags, an unknown item, an item without a vector, pool > top_k."""
    m, batch = gpu_model(strings)
    queries = check_similar_api(m, batch, strings)
    eng = m.model.engine
    known = [q for q in queries if m.item_ids.get_id(q) is not None]
    qid = np.array([m.item_ids.get_id(q) for q in known])
    base = [t.cpu().numpy() for t in eng.similar_factor_device(qid, 20, 0)[:3]]
    for splits in (1, 2, 9):
        got = [t.cpu().numpy() for t in eng.similar_factor_device(qid, 20, 0, item_splits=splits)[:3]]
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), splits
    # the norms are taken with the vectors, stand beside them, and a rebuild or clear_factors drops them
    rng = np.random.default_rng(3)
    P, Q = rng.standard_normal((eng.n_users, 6)).astype(F32), rng.standard_normal((m.model.n_items_fitted, 6)).astype(F32)
    eng.set_factors(P, Q)
    assert set(eng._F["norms"]) == {0}
    n0 = eng.item_norms_device(0)
    assert eng.item_norms_device(0) is n0 and np.array_equal(n0.cpu().numpy().view(np.int32), host_norms_fast(Q).view(np.int32))
    assert np.array_equal(eng.item_norms_device(2).cpu().numpy().view(np.int32), host_norms_fast(Q[:, 2:]).view(np.int32))
    eng.set_factors(P, Q * F32(3.0))
    assert set(eng._F["norms"]) == {0} and eng.item_norms_device(0) is not n0
    assert np.array_equal(eng.item_norms_device(0).cpu().numpy().view(np.int32), host_norms_fast(Q * F32(3.0)).view(np.int32))
    m.detach_factors()
    assert not eng.has_factors() and "norms" not in eng._F


def test_the_serving_route_and_the_recommender_on_the_device():
    from tests.test_feature_repr_host import attach_tables, seeded_tables
    m, batch = gpu_model()
    t = seeded_tables(batch)
    attach_tables(m, t)
    assert set(m.similar_items_hybrid(t["all_items"][4])) and set(m.model.engine._F["norms"]) == {1}      # biased tables: [b, e...]
    check_serving_and_facade(m, t["all_items"][4], t["all_items"][:9])
