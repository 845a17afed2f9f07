"""Training the factor scorer on the GPU (csrc/factor_gram.hip, csrc/factor_als.hip, torch.ops.rtrec_amd.factor_gram /
factor_als_solve, SLIM.fit_factors) against the host models of tests/test_als_host.py: the status with ==, every Gram element and
every solved vector by its bits after adding +0.0f (the sign of a zero is not part of the contract).  Both kernels build their
matrices with the f32-input MFMA; these tests are what says that it is the fmaf chain of the contract, bit for bit.  The output
buffers carry a sentinel before every call: what a call must not touch keeps it."""
import numpy as np
import pytest

from tests.test_als_host import (BLOCK_SEED, BLOCK_USABLE, BREAK_ALPHA, BREAK_GRID, BREAK_KINDS, BREAK_LENGTHS, BREAK_T, F32, OUTSIDE,
                                 STRIDE_CASES, STRIDE_GRID, STRIDE_PAIRS, STRIDE_SECOND, als_block_case, als_case, als_inf_case,
                                 als_rounding_case, als_stride_case, als_tiny_case, bits, block_data, break_reference, counts_of,
                                 gram_fast, half_step, host_fit, solve_fast, stride_classes)
from tests.test_factor_host import rounding_vectors

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")


def run_gram(V, reg, pad=0, n=None):
    """torch.ops.rtrec_amd.factor_gram on a host matrix; `pad` > 0: the stride is wider than dim, with NaN behind it; `n`: n_v,
    where the matrix handed in has more rows than the call may read."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    V = np.asarray(V, F32)
    rows, dim = V.shape
    n = rows if n is None else n
    Vd = np.concatenate([V, np.full((rows, pad), np.nan, F32)], axis=1) if pad else V
    gram = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda:0")
    chunks = (n + 1023) // 1024
    ws = torch.full((chunks * dim * dim,), np.nan, dtype=torch.float32, device="cuda:0") if chunks else None
    torch.ops.rtrec_amd.factor_gram(up(Vd, np.float32) if n else torch.zeros((0, dim + pad), device="cuda:0"), n, dim, float(reg), gram, ws)
    torch.cuda.synchronize()
    return gram.cpu().numpy()


def run_solve(ptr, idx, val, V, G, alpha, jobs=None, pad=0, n_v=None):
    """torch.ops.rtrec_amd.factor_als_solve on host arrays: (status[n_jobs], out[n_rows, dim + pad]) with the sentinel wherever
    the call wrote nothing; `pad` > 0 widens both strides (NaN behind V's components); `n_v` where V has more rows than the
    call may name."""
    import torch
    from rtrec_amd import ops  # noqa: F401
    V = np.asarray(V, F32)
    rows, dim = V.shape
    n_v = rows if n_v is None else n_v
    n_rows = len(ptr) - 1
    Vd = np.concatenate([V, np.full((rows, pad), np.nan, F32)], axis=1) if pad else V
    n_jobs = n_rows if jobs is None else len(jobs)
    out = torch.full((n_rows, dim + pad), SENTINEL, dtype=torch.float32, device="cuda:0")
    status = torch.full((n_jobs,), 9, dtype=torch.uint8, device="cuda:0")
    torch.ops.rtrec_amd.factor_als_solve(None if jobs is None else up(jobs, np.int32), n_jobs, up(ptr, np.int32), up(idx, np.int32),
                                         up(val, np.float32), up(Vd, np.float32), n_v, dim, up(G, np.float32), float(alpha), out, status)
    torch.cuda.synchronize()
    return status.cpu().numpy(), out.cpu().numpy()


def host_solve(ptr, idx, val, V, G, alpha, jobs=None, pad=0):
    out = np.full((len(ptr) - 1, V.shape[1] + pad), SENTINEL, F32)
    return solve_fast(ptr, idx, val, V, G, alpha, out, jobs), out


def assert_solved(got, want, what):
    (gs, go), (ws, wo) = got, want
    assert np.array_equal(gs, ws), (what, "status", np.flatnonzero(gs != ws)[:5], gs[gs != ws][:5], ws[gs != ws][:5])
    same = bits(go) == bits(wo)
    assert same.all(), (what, "vectors", np.argwhere(~same)[:5], go[~same][:3], wo[~same][:3])


# ---------------------------------------------------------------------------------------------- 1. the Gram matrix
@pytest.mark.parametrize("dim", [1, 7, 32, 33, 48, 63, 64])
def test_gram_is_the_chunked_fmaf_chain_bit_for_bit(dim):
    """Cancelling 2^24 terms, midpoint products and denormals (rounding_vectors): another order of the rows, an unfused multiply,
    a wider accumulator or another chunk size changes bits.  1023 / 1024 / 1025 and 2048 / 2049 rows stand on both sides of a
    chunk, 2 / 3 and 15 .. 18 rows around the group of 16 rows whose loads are issued together."""
    for n in (1, 2, 3, 15, 16, 17, 18, 1023, 1024, 1025, 2048, 2049, 3000):
        V = rounding_vectors(n, 1, dim, seed=n + dim)[0]
        pad = 3 if n == 1025 else 0
        got, want = run_gram(V, 0.37, pad), gram_fast(V, 0.37)
        same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (n, dim, np.argwhere(~same)[:5])
        assert np.array_equal(got.view(np.int32), got.T.view(np.int32)), (n, dim, "not symmetric")
    assert np.array_equal(run_gram(np.zeros((0, dim), F32), 0.25), np.eye(dim, dtype=F32) * F32(0.25))
    # the inputs have teeth: a float64 accumulation gives other bits (not at dim 1: one sum of squares, ruled by its 2^48 terms)
    V = rounding_vectors(3000, 1, dim, seed=3000 + dim)[0]
    with np.errstate(all="ignore"):
        wide = (V.astype(np.float64).T @ V.astype(np.float64)).astype(F32) + np.eye(dim, dtype=F32) * F32(0.37)
    assert dim == 1 or (bits(wide) != bits(gram_fast(V, 0.37))).any()


# ---------------------------------------------------------------------------------------------- 2. the solve
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 300)


@pytest.mark.parametrize("dim", [1, 2, 31, 32, 33, 64])
def test_solve_equals_the_host_model_bit_for_bit(dim):
    """96 jobs over rows of 0 .. 300 entries in a shuffled explicit order, two job rows outside R, four rows of R no job names;
    values 0, negative and NaN, columns outside V and a NaN row of V reachable only through skipped entries (als_case)."""
    ptr, idx, val, V = als_case(100, 400, dim, seed=dim, lengths=LENGTHS, scale=0.3)
    G = gram_fast(np.nan_to_num(V), 0.1)
    rng = np.random.default_rng(dim)
    jobs = np.r_[rng.permutation(100)[:96], -1, 100]
    jobs = jobs[rng.permutation(len(jobs))]
    got, want = run_solve(ptr, idx, val, V, G, 0.7, jobs, pad=2), host_solve(ptr, idx, val, V, G, 0.7, jobs, pad=2)
    assert_solved(got, want, f"dim {dim}")
    status, out = got
    named = np.zeros(100, bool)
    named[jobs[(jobs >= 0) & (jobs < 100)]] = True
    assert (out[~named] == SENTINEL).all() and (out[:, dim:] == SENTINEL).all()
    assert sorted(set(status.tolist())) == [0, 1] and (status == 0).sum() >= 80
    # without a job list job r is row r
    assert_solved(run_solve(ptr, idx, val, V, G, 0.7), host_solve(ptr, idx, val, V, G, 0.7), f"dim {dim}, no job list")


def test_fit_factors_on_the_device_equals_the_host_stack():
    """The block-structured case of tests/test_als_host.py through SLIM.fit_factors: after 2 iterations P and Q carry the host
    model's bits, and the factor and hybrid lists are those of the CPU stand-in stack with the host model's vectors attached
    (and the device model's W, so that SLIM's side is the same on both)."""
    import scipy.sparse as sp
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    from tests.test_als_host import als_backend, attach_host_vectors, resident_x
    X = block_data(0).tocoo()
    batch = [(int(u), int(i), 1000.0, float(v)) for u, i, v in zip(X.row, X.col, X.data)]
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=F32)
    kw = dict(dim=8, iterations=2, regularization=0.01, alpha=1.0, seed=0)
    assert m.fit_factors(**kw) is m and m.has_factors()
    P, Q, su, si = host_fit(resident_x(m), 8, 2, 0.01, 1.0, 0)
    assert (su == 0).all() and (si == 0).all()
    F = m._factors
    assert np.array_equal(F["user_rows"], np.arange(200)) and np.array_equal(F["item_rows"], np.arange(120))
    assert np.array_equal(bits(F["user_vectors"]), bits(P)) and np.array_equal(bits(F["item_vectors"]), bits(Q))
    ref = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    ref.model._engine = SlimEngine(backend=als_backend())
    ref.fit(batch, progress_bar=False)
    ref.model.item_similarity = m.model.item_similarity.copy()
    attach_host_vectors(ref, P, su, Q, si)
    users = list(range(0, 200, 3)) + [10 ** 6]
    assert m.recommend_factor_batch(users, top_k=5) == ref.recommend_factor_batch(users, top_k=5)
    got, want = m.recommend_factor_batch(users, top_k=5, as_arrays=True), ref.recommend_factor_batch(users, top_k=5, as_arrays=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
    for h in (dict(top_k=6), dict(top_k=5, pool=12, weighting=0.5)):
        assert m.recommend_hybrid_batch(users, **h) == ref.recommend_hybrid_batch(users, **h), h
    # the online step: new interactions, then the named rows alone are solved again
    m.fit([(3, 40, 1001.0, 5.0), (777, 95, 1001.0, 4.0), (777, 100, 1001.0, 2.0)], progress_bar=False)
    ref.fit([(3, 40, 1001.0, 5.0), (777, 95, 1001.0, 4.0), (777, 100, 1001.0, 2.0)], progress_bar=False)
    m.update_factors([3, 777])
    ref.update_factors([3, 777])
    for key in ("user_rows", "item_rows"):
        assert np.array_equal(m._factors[key], ref._factors[key]), key
    for key in ("user_vectors", "item_vectors"):
        assert np.array_equal(bits(m._factors[key]), bits(ref._factors[key])), key
    assert len(m._factors["user_rows"]) == 201 and m.recommend_factor_batch([777], top_k=5)[0]


def test_breakdown_is_a_status_never_a_fault():
    for dim in (3, 40):
        ptr, idx, val, _ = als_case(12, 50, dim, seed=1, lengths=(2, 5, 0))
        Z = np.zeros((50, dim), F32)
        st, out = run_solve(ptr, idx, val, Z, np.zeros((dim, dim), F32), 1.0)                   # reg = 0, V = 0: d = 0 at once
        hs, ho = host_solve(ptr, idx, val, Z, np.zeros((dim, dim), F32), 1.0)
        assert np.array_equal(st, hs) and set(st.tolist()) == {1, 2} and (out == 0).all() and (ho == 0).all()
        V = np.random.default_rng(2).standard_normal((50, dim)).astype(F32)
        G = gram_fast(V, 0.1)
        G[dim - 1, 0] = np.nan
        assert_solved(run_solve(ptr, idx, val, V, G, 1.0), host_solve(ptr, idx, val, V, G, 1.0), "NaN in G")
        assert (run_solve(ptr, idx, val, V, G, 1.0)[0] != 0).all()
        # offsets far beyond nnz and below zero: clamped, so the answer is the clamped matrix's
        G = gram_fast(V, 0.1)
        bad = ptr.astype(np.int64).copy()
        bad[3], bad[7], bad[-1] = 2 ** 31 - 1, -5, 10 ** 9
        bad = bad.astype(np.int32)
        assert_solved(run_solve(bad, idx, val, V, G, 1.0), host_solve(bad, idx, val, V, G, 1.0), "offsets out of range")


# ---------------------------------------------------------------------------------------------- 3. a workgroup's second job
@pytest.mark.parametrize("dim, c", STRIDE_CASES)
def test_a_second_job_on_the_same_workgroup_starts_clean(dim, c):
    """2^18 + 300 jobs (als_stride_case): more than a launch has workgroups, so workgroups 0 .. 299 run job b and then job
    b + 2^18 -- the only place where LDS `A`, the accumulators, rhs and the flags of a job meet those of the job before.  The
    job list lays every pair of STRIDE_PAIRS on one workgroup: a solve, a breakdown and an empty row after a solved job, after
    one that broke in the middle of its factorisation (A half overwritten), after a row without a usable entry and after a row
    outside R.  Every status, every vector and the sentinel in the rows no job names and behind dim are compared; the
    expectation is the 64 templates expanded (a job's result depends on its row alone).  Without a job list job r is row r and
    workgroup b runs the same template twice."""
    ptr, idx, val, V, G, jobs, t_st, t_out = als_stride_case(dim, c)
    n_rows = len(ptr) - 1
    assert len(jobs) > STRIDE_GRID and min(counts_of(t_st)) >= 5
    cls = stride_classes(jobs, n_rows, t_st)
    second = np.arange(STRIDE_GRID, STRIDE_GRID + STRIDE_SECOND)
    pairs = set(zip(cls[second - STRIDE_GRID].tolist(), cls[second].tolist()))
    assert pairs == set(STRIDE_PAIRS) and {(0, 0), (2, 0), (1, 0), (OUTSIDE, 0), (0, 2)} <= pairs
    named = jobs[cls != OUTSIDE].astype(np.int64)
    want = np.full((n_rows, dim + 2), SENTINEL, F32)
    want[named, :dim] = t_out[named % 64]
    assert n_rows - len(named) >= 100
    got = run_solve(ptr, idx, val, V, G, BREAK_ALPHA, jobs, pad=2)
    assert_solved(got, (np.where(cls == OUTSIDE, 1, cls).astype(np.uint8), want), f"dim {dim}, {len(jobs)} jobs")
    want[:, :dim] = np.tile(t_out, (n_rows // 64 + 1, 1))[:n_rows]
    got = run_solve(ptr, idx, val, V, G, BREAK_ALPHA, pad=2)
    assert_solved(got, (np.tile(t_st, n_rows // 64 + 1)[:n_rows], want), f"dim {dim}, one job per row")


# ---------------------------------------------------------------------------------------------- 4. blocks of 64 entries
@pytest.mark.parametrize("dim", [1, 32, 33, 48, 63, 64])
def test_blocks_without_a_usable_entry_and_the_block_edges(dim):
    """als_block_case: whole blocks of skipped entries before, between and after the usable ones, a block's only usable entry
    in lane 0, in lane 63 or in the odd last slot, rows of exactly 127 .. 129 and 191 .. 193 usable entries -- with a shuffled
    job list that also names two rows outside R, and without one; strides wider than dim."""
    ptr, idx, val, V = als_block_case(260, dim, BLOCK_SEED.get(dim, dim))
    G = gram_fast(np.nan_to_num(V), 0.1)
    n = len(BLOCK_USABLE)
    jobs = np.r_[np.arange(n), -1, n][np.random.default_rng(dim).permutation(n + 2)]
    want = host_solve(ptr, idx, val, V, G, 0.7, jobs, pad=2)
    assert want[0].tolist() == [1 if x in (-1, n) or not BLOCK_USABLE[x] else 0 for x in jobs]
    assert_solved(run_solve(ptr, idx, val, V, G, 0.7, jobs, pad=2), want, f"dim {dim}")
    want = host_solve(ptr, idx, val, V, G, 0.7, pad=2)
    assert want[0].tolist() == [0 if u else 1 for u in BLOCK_USABLE]
    assert_solved(run_solve(ptr, idx, val, V, G, 0.7, pad=2), want, f"dim {dim}, no job list")


# ---------------------------------------------------------------------------------------------- 5. breakdown at every column
@pytest.mark.parametrize("kind", BREAK_KINDS)
@pytest.mark.parametrize("dim, c", BREAK_GRID)
def test_breakdown_at_a_middle_pivot(dim, c, kind):
    """als_break_case: G doctored at pivot c -- the first, the second and the last column, and for dim > 32 the columns 31, 32
    and 33 where the factorisation leaves tile (0, 0) -- by a negative diagonal (rows break or survive by their length: both
    must occur, but at dim 64, c = 32, where no t leaves a survivor, BREAK_T), by +inf on the diagonal and by a NaN in the
    middle of row c.  One launch: solved and broken jobs side by side, broken rows all zero."""
    (ptr, idx, val, V, G), st, out = break_reference(dim, c, kind)
    n0, n1, n2 = counts_of(st)
    if kind == "neg" and BREAK_T.get((dim, c), 0.5) is not None:
        assert n0 >= 1 and n1 == 6 and n2 >= 1, (n0, n1, n2)
    else:
        assert (n0, n1, n2) == (0, 6, 42)
    assert (out[st != 0] == 0).all()
    got = run_solve(ptr, idx, val, V, G, BREAK_ALPHA)
    assert_solved(got, (st, out), f"dim {dim}, c {c}, {kind}")
    assert (got[1][got[0] != 0] == 0).all()


# ---------------------------------------------------------------------------------------------- 6. denormals, rounding, inf
@pytest.mark.parametrize("dim, g, alpha, mix", [(1, 1e-38, 1e-39, [42, 6, 0]), (5, 1e-38, 1e-39, [42, 6, 0]), (40, 1e-38, 1e-39, [38, 6, 4]),
                                               (1, 1e-40, 1e-40, [7, 6, 35])])
def test_denormals_are_kept_in_every_stage_of_the_solve(dim, g, alpha, mix):
    """als_tiny_case: w, fl(w * y), the pivots and the quotients are float32 denormals and the solved components reach 3e38; a
    kernel that flushes any of them gives other statuses (tests/test_als_host.py).  g = alpha = 1e-40: the factorisation
    succeeds and the component overflows -- status 2 by the test after the substitutions."""
    ptr, idx, val, V, G, alpha = als_tiny_case(dim, g, alpha)
    want = host_solve(ptr, idx, val, V, G, alpha)
    assert counts_of(want[0]) == mix
    assert_solved(run_solve(ptr, idx, val, V, G, alpha), want, f"dim {dim}, g {g}")


@pytest.mark.parametrize("dim", [7, 32, 40, 64])
def test_the_build_is_the_fmaf_chain_on_rounding_sensitive_vectors(dim):
    """als_rounding_case: 2^24-sized cancelling terms, midpoint products and denormals in V; all 42 non-empty rows are solved,
    and an unfused or reordered build changes their bits (tests/test_als_host.py)."""
    for side in (0, 1):
        ptr, idx, val, V, G = als_rounding_case(dim, side)
        want = host_solve(ptr, idx, val, V, G, 0.7)
        assert counts_of(want[0]) == [42, 6, 0]
        assert_solved(run_solve(ptr, idx, val, V, G, 0.7), want, f"dim {dim}, side {side}")


@pytest.mark.parametrize("dim", [5, 33, 64])
def test_one_infinite_value_breaks_its_row_alone(dim):
    ptr, idx, val, V, G, row = als_inf_case(dim)
    want = host_solve(ptr, idx, val, V, G, BREAK_ALPHA)
    assert counts_of(want[0]) == [41, 6, 1] and want[0][row] == 2 and (want[1][row] == 0).all()
    assert_solved(run_solve(ptr, idx, val, V, G, BREAK_ALPHA), want, f"dim {dim}")


# ---------------------------------------------------------------------------------------------- 7. n_v below the tensor's rows
@pytest.mark.parametrize("dim", [5, 40])
def test_rows_of_v_behind_n_v_are_never_read(dim):
    """V as handed in has 40 NaN rows behind n_v.  The solve skips every entry that names one (a fifth of the usable entries
    are moved there) and equals the host model on V[:n_v]; the Gram matrix is that of V[:n_v], with n_v in the middle of a
    group of 16 rows, at a chunk edge and one behind it."""
    ptr, idx, val, V = als_case(48, 200, dim, seed=dim, lengths=BREAK_LENGTHS, scale=0.3)
    rng = np.random.default_rng(dim)
    idx = idx.copy()
    move = np.flatnonzero((val > 0) & (idx >= 0) & (idx < 199) & (rng.random(len(idx)) < 0.2))
    idx[move] = 200 + rng.integers(0, 40, len(move))
    big = np.concatenate([V, np.full((40, dim), np.nan, F32)])
    G = gram_fast(np.nan_to_num(V), 0.1)
    want = host_solve(ptr, idx, val, V, G, 0.7, pad=2)
    assert len(move) > 300 and counts_of(want[0])[0] >= 36 and counts_of(want[0])[2] == 0      # (a short row may lose every entry)
    assert_solved(run_solve(ptr, idx, val, big, G, 0.7, pad=2, n_v=200), want, f"dim {dim}")
    for n in (17, 1024, 1025):
        Vn = np.concatenate([rounding_vectors(n, 1, dim, seed=n + dim)[0], np.full((40, dim), np.nan, F32)])
        got, want_g = run_gram(Vn, 0.37, pad=1, n=n), gram_fast(Vn[:n], 0.37)
        assert np.isfinite(want_g).all() and np.array_equal(bits(got), bits(want_g)), (dim, n)


# ---------------------------------------------------------------------------------------------- 8. end to end, larger
def larger_end_to_end(eng):
    """The body of the test below on an engine (the CPU stand-in of tests/test_als_host.py runs it too)."""
    X = block_data(0, clusters=4, items_per=30, users_per=275, rated=8)
    item_lens = np.diff(X.tocsc().indptr)
    assert X.shape == (1100, 120) and item_lens.min() >= 50 and (item_lens > 64).sum() >= 60      # two chunks of P; two entry blocks
    eng.set_interactions(X.tocsc())
    counts = eng.fit_factors(dim=40, iterations=2, regularization=0.01, alpha=1.0, seed=0)
    P, Q, su, si = host_fit(X, 40, 2, 0.01, 1.0, 0)
    assert (su == 0).all() and (si == 0).all()
    gP, gsu, gQ, gsi = eng.als_vectors()
    assert counts == {"user": {0: 1100, 1: 0, 2: 0}, "item": {0: 120, 1: 0, 2: 0}}
    assert np.array_equal(gsu, su) and np.array_equal(gsi, si)
    assert np.array_equal(bits(gP), bits(P)) and np.array_equal(bits(gQ), bits(Q))
    # a half-step over named rows: duplicates and rows outside the side are dropped, the rest solved in ascending order
    want = P.copy()
    st = half_step(X, Q, 0.01, 1.0, want, job_rows=[5, 17, 900])
    changed = (bits(want) != bits(P)).any(axis=1)
    assert st.tolist() == [0, 0, 0] and np.flatnonzero(changed).tolist() == [5, 17, 900]
    assert eng.als_half_step("user", rows=[5, 5, 900, -3, 10 ** 6, 17]) == {0: 3, 1: 0, 2: 0}
    hP, hsu, hQ, hsi = eng.als_vectors()
    assert np.array_equal(bits(hP), bits(want)) and np.array_equal(bits(hP[~changed]), bits(gP[~changed]))
    assert np.array_equal(bits(hQ), bits(gQ)) and np.array_equal(hsu, su) and np.array_equal(hsi, si)


def test_fit_factors_with_two_gram_chunks_and_two_entry_blocks():
    """1,100 users x 120 items at dim 40 through SlimEngine.fit_factors: the item half-step's Gram matrix has two chunks, an
    item's row 60 .. 90 entries (two blocks), the three lower tiles are live.  P, Q and the statuses equal host_fit's; then
    als_half_step("user", rows=[5, 5, 900, -3, 10**6, 17]) equals the host half-step over rows 5, 17 and 900, every other row
    keeps its bits, and the counts are returned."""
    from rtrec_amd.engine import SlimEngine
    larger_end_to_end(SlimEngine(device="cuda:0"))
