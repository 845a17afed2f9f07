"""Training the factor scorer by conjugate gradient on the GPU (csrc/factor_als_cg.hip, the wide kernel of csrc/factor_gram.hip,
torch.ops.rtrec_amd.factor_gram_wide / factor_als_cg, SLIM.fit_factors(solver="cg")) against the host models of
tests/test_als_cg_host.py and tests/test_als_host.py: the status with ==, every Gram element, every vector and every residual
norm by its bits after adding +0.0f (the sign of a zero is not part of the contract).  The output buffers carry a sentinel
before every call: what a call must not touch keeps it."""
import functools

import numpy as np
import pytest

from tests.test_als_host import BLOCK_SEED, BLOCK_USABLE, F32, als_block_case, block_data, counts_of, gram_fast
from tests.test_als_cg_host import (OUTSIDE, STATUS_ALPHA, STRIDE_GRID, STRIDE_PAIRS, STRIDE_SECOND, STRIDE_STEPS, STRIDE_TEMPLATES,
                                    bits, cg_case, cg_fast, cg_half_step, cg_stride_case, early_stop_case, host_fit_cg, run,
                                    small_residual_case, status_case, stride_classes, tiny_case, warm_vectors)
from tests.test_factor_host import rounding_vectors

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")


def run_gram(V, reg, pad=0, n=None, op="factor_gram_wide"):
    """torch.ops.rtrec_amd.factor_gram_wide (or `op`) on a host matrix; `pad` > 0: the stride is wider than dim, with NaN behind
    it; `n`: n_v, where the matrix handed in has more rows than the call may read."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    V = np.asarray(V, F32)
    rows, dim = V.shape
    n = rows if n is None else n
    Vd = np.concatenate([V, np.full((rows, pad), np.nan, F32)], axis=1) if pad else V
    gram = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda:0")
    chunks = (n + 1023) // 1024
    ws = torch.full((chunks * dim * dim,), np.nan, dtype=torch.float32, device="cuda:0") if chunks else None
    getattr(torch.ops.rtrec_amd, op)(up(Vd, np.float32) if rows else torch.zeros((0, dim + pad), device="cuda:0"), n, dim, float(reg), gram, ws)
    torch.cuda.synchronize()
    return gram.cpu().numpy()


def run_cg(case, alpha, cg_steps=3, warm=None, jobs=None, pad=0, n_v=None, want_rs=True):
    """torch.ops.rtrec_amd.factor_als_cg on host arrays: (status[n_jobs], rs[n_jobs], out[n_rows, dim + pad]).  `warm`
    [n_rows, dim]: the start vectors (None: warm_start = 0 and `out` holds the sentinel); `pad` > 0 widens both strides (NaN
    behind V's components, the sentinel behind out's); rs is the sentinel where the call wrote none, and None without want_rs."""
    import torch
    from rtrec_amd import ops  # noqa: F401
    ptr, idx, val, V, G = case[:5]
    V = np.asarray(V, F32)
    rows, dim = V.shape
    n_v = rows if n_v is None else n_v
    n_rows = len(ptr) - 1
    Vd = np.concatenate([V, np.full((rows, pad), np.nan, F32)], axis=1) if pad else V
    n_jobs = n_rows if jobs is None else len(jobs)
    start = np.full((n_rows, dim + pad), SENTINEL, F32)
    if warm is not None:
        start[:, :dim] = warm
    out = up(start, np.float32)
    status = torch.full((n_jobs,), 9, dtype=torch.uint8, device="cuda:0")
    rs = torch.full((n_jobs,), SENTINEL, dtype=torch.float32, device="cuda:0") if want_rs else None
    torch.ops.rtrec_amd.factor_als_cg(None if jobs is None else up(jobs, np.int32), n_jobs, up(ptr, np.int32), up(idx, np.int32),
                                      up(val, np.float32), up(Vd, np.float32), n_v, dim, up(G, np.float32), float(alpha), int(cg_steps),
                                      warm is not None, out, status, rs)
    torch.cuda.synchronize()
    return status.cpu().numpy(), None if rs is None else rs.cpu().numpy(), out.cpu().numpy()


def host_cg(case, alpha, cg_steps=3, warm=None, jobs=None, pad=0):
    ptr, idx, val, V, G = case[:5]
    out = np.full((len(ptr) - 1, V.shape[1] + pad), SENTINEL, F32)
    if warm is not None:
        out[:, :V.shape[1]] = warm
    st, rs = cg_fast(ptr, idx, val, V, G, alpha, out, jobs, cg_steps, warm is not None)
    return st, rs, out


def assert_same(got, want, what):
    (gs, gr, go), (ws, wr, wo) = got, want
    assert np.array_equal(gs, ws), (what, "status", np.flatnonzero(gs != ws)[:5], gs[gs != ws][:5], ws[gs != ws][:5])
    same = bits(go) == bits(wo)
    assert same.all(), (what, "vectors", int((~same).sum()), np.argwhere(~same)[:5], go[~same][:3], wo[~same][:3])
    if gr is not None:
        same = (bits(gr) == bits(wr)) | (np.isnan(gr) & np.isnan(wr))
        assert same.all(), (what, "rs", np.flatnonzero(~same)[:5], gr[~same][:3], wr[~same][:3])


# ---------------------------------------------------------------------------------------------- 1. the wide Gram matrix
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("dim", [1, 32, 33, 64, 65, 96, 97, 128, 255, 256])
def test_gram_wide_is_the_chunked_fmaf_chain_bit_for_bit(dim, n):
    """Cancelling 2^24 terms, midpoint products and denormals (rounding_vectors) on both sides of a chunk and of every 32-wide
    tile: another order of the rows, an unfused multiply, a wider accumulator or a tile written to the wrong place changes
    bits.  Up to 64 components the narrow call gives the same bits; 1025 rows are read through a wider stride and with n_v below
    the tensor's rows."""
    V = rounding_vectors(n, 1, dim, seed=n + dim)[0]
    want = gram_fast(V, 0.37)
    if n == 1025:
        Vd = np.concatenate([V, np.full((40, dim), np.nan, F32)])               # rows the call may not read
        got = run_gram(Vd, 0.37, pad=3, n=n)
    else:
        got = run_gram(V, 0.37)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (n, dim, int((~same).sum()), np.argwhere(~same)[:5])
    assert np.array_equal(got.view(np.int32), got.T.view(np.int32)), (n, dim, "not symmetric")
    if dim <= 64:
        narrow = run_gram(V, 0.37, op="factor_gram")
        assert np.array_equal(got.view(np.int32), narrow.view(np.int32)) or n == 1025 and np.array_equal(bits(got), bits(narrow))
    if n == 1:
        assert np.array_equal(run_gram(np.zeros((0, dim), F32), 0.25), np.eye(dim, dtype=F32) * F32(0.25))


# ---------------------------------------------------------------------------------------------- 2. the conjugate-gradient call
@pytest.mark.parametrize("dim", [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256])
def test_cg_equals_the_host_model_bit_for_bit(dim):
    """27 rows of 0 / 1 / 2 / 3 / 63 / 64 / 65 / 129 / 300 entries (cg_case: values 0, negative and NaN, columns outside V and a NaN
    row of V reachable only through skipped entries) at every power-of-two edge of `tree` and every wave count.  Cold, three
    steps, a shuffled job list with two rows outside R and two rows no job names, wider strides, rs wanted; then warm, two
    steps, without a job list and without rs, from finite vectors, from zeros (rows 5 and 6) and from vectors with one NaN
    component (rows 7 and 8: the cold start of those rows)."""
    case = cg_case(dim)
    st_h = run(case, 0.7, 3)[0]
    assert counts_of(st_h) == [24, 3, 0]                 # the builder on the host model alone: all finished but the empty rows
    rng = np.random.default_rng(dim)
    jobs = np.r_[rng.permutation(27)[:25], -1, 27]
    jobs = jobs[rng.permutation(len(jobs))]
    got, want = run_cg(case, 0.7, 3, None, jobs, pad=2), host_cg(case, 0.7, 3, None, jobs, pad=2)
    assert_same(got, want, f"dim {dim} cold")
    status, rs, out = got
    named = np.zeros(27, bool)
    named[jobs[(jobs >= 0) & (jobs < 27)]] = True
    assert (out[~named] == SENTINEL).all() and (out[:, dim:] == SENTINEL).all()
    assert (rs[(jobs < 0) | (jobs >= 27)] == 0).all() and (rs[status == 1] == 0).all() and (rs[status == 0] > 0).all()
    warm = warm_vectors(27, dim, dim + 1, nan_rows=(7, 8))
    warm[[5, 6]] = 0
    got, want = run_cg(case, 0.7, 2, warm, want_rs=False), host_cg(case, 0.7, 2, warm)
    assert_same(got, want, f"dim {dim} warm")
    cold = host_cg(case, 0.7, 2)
    assert np.array_equal(bits(got[2][[5, 6, 7, 8]]), bits(cold[2][[5, 6, 7, 8]]))
    assert dim == 1 or not np.array_equal(bits(got[2][[9, 17]]), bits(cold[2][[9, 17]]))


@pytest.mark.parametrize("dim", [5, 70, 200])
def test_whole_blocks_of_skipped_entries(dim):
    """als_block_case: whole 64-entry blocks of skipped entries before, between and behind usable ones, a block's only usable
    entry in its first or last slot, rows that end at, one before and one behind the second and third block edge."""
    ptr, idx, val, V = als_block_case(260, dim, BLOCK_SEED.get(dim, dim))
    case = (ptr, idx, val, V, gram_fast(np.nan_to_num(V), 0.1))
    want = host_cg(case, 0.7, 3)
    assert want[0].tolist() == [0 if n else 1 for n in BLOCK_USABLE]
    assert_same(run_cg(case, 0.7, 3), want, f"dim {dim}")
    warm = warm_vectors(len(ptr) - 1, dim, 2)
    assert_same(run_cg(case, 0.7, 1, warm), host_cg(case, 0.7, 1, warm), f"dim {dim} warm")


def test_the_threshold_stops_a_job_early():
    """The dim-2 case whose rows fall below rn < 1e-20f after one, two and three steps: 1, 3 and 64 steps."""
    case = early_stop_case()
    results = {}
    for steps in (1, 3, 64):
        results[steps] = run_cg(case, 1.0, steps)
        assert_same(results[steps], host_cg(case, 1.0, steps), f"{steps} steps")
    assert np.array_equal(bits(results[3][2]), bits(results[64][2])) and not np.array_equal(bits(results[1][2]), bits(results[3][2]))


# ---------------------------------------------------------------------------------------------- 3. status
@pytest.mark.parametrize("dim", [5, 40, 70])
def test_breakdown_is_a_status_never_a_fault(dim):
    """Finished and broken jobs side by side in one launch: G negative so that den <= 0 at step 1, and at step 2 only; a NaN and
    a +inf in G (symmetric); denormal w and products with components that overflow; a start residual below the threshold, from
    zero and from a small start.  tests/test_als_cg_host.py says from the host model alone that each case holds what it claims
    and that a flushing kernel would show on the denormal one."""
    for kind, steps in (("neg1", 1), ("neg1", 3), ("neg2", 2), ("nan", 3), ("inf", 3)):
        case = status_case(dim, kind)
        want = host_cg(case, STATUS_ALPHA, steps)
        assert counts_of(want[0])[2] >= 3, (kind, counts_of(want[0]))
        assert_same(run_cg(case, STATUS_ALPHA, steps), want, f"dim {dim} {kind}")
    if dim <= 40:
        *case, alpha = tiny_case(dim)
        want = host_cg(case, alpha, 3)
        assert counts_of(want[0])[0] >= 20 and counts_of(want[0])[2] >= 5
        assert_same(run_cg(case, alpha, 3), want, f"dim {dim} denormal")
        flushed = run(case, alpha, 3, variant="flush")
        assert not np.array_equal(flushed[0], want[0])
    case = small_residual_case(dim)
    for warm in (None, warm_vectors(18, dim, 1) * F32(1e-11)):
        want = host_cg(case, 1.0, 3, warm)
        assert counts_of(want[0]) == [16, 2, 0] and (want[1][want[0] == 0] < 1e-20).all()
        assert_same(run_cg(case, 1.0, 3, warm), want, f"dim {dim} small residual")
    # offsets far beyond nnz and below zero: clamped, so the answer is the clamped matrix's
    ptr, idx, val, V, G = cg_case(dim, n_rows=18, n_v=80, lengths=(2, 5, 0, 70))
    bad = ptr.astype(np.int64).copy()
    bad[3], bad[7], bad[-1] = 2 ** 31 - 1, -5, 10 ** 9
    case = (bad.astype(np.int32), idx, val, V, G)
    assert_same(run_cg(case, 1.0, 2), host_cg(case, 1.0, 2), "offsets out of range")


# ---------------------------------------------------------------------------------------------- 4. a workgroup's second job
@pytest.mark.parametrize("dim", [5, 70])
def test_a_second_job_on_the_same_workgroup_starts_clean(dim):
    """2^14 + 300 jobs (cg_stride_case): more than a launch has workgroups, so workgroups 0 .. 299 run job b and then job
    b + 2^14 -- the only place where the LDS vectors, the staged rows and the flags of a job meet those of the job before.  The
    job list lays every pair of STRIDE_PAIRS on one workgroup: a finished, a broken and an empty job after a finished one, after
    one that broke, after a row without a usable entry and after a row outside R.  Every status, vector and residual norm and
    the sentinel in the rows no job names and behind dim are compared; the expectation is the 509 templates expanded."""
    ptr, idx, val, V, G, jobs, t_st, t_rs, t_out = cg_stride_case(dim)
    n_rows = len(ptr) - 1
    assert len(jobs) > STRIDE_GRID and min(counts_of(t_st)) >= 50
    cls = stride_classes(jobs, n_rows, t_st)
    second = np.arange(STRIDE_GRID, STRIDE_GRID + STRIDE_SECOND)
    assert set(zip(cls[second - STRIDE_GRID].tolist(), cls[second].tolist())) == set(STRIDE_PAIRS)
    inside = cls != OUTSIDE
    named = jobs[inside].astype(np.int64)
    want_out = np.full((n_rows, dim + 2), SENTINEL, F32)
    want_out[named, :dim] = t_out[named % STRIDE_TEMPLATES]
    want_st = np.where(inside, cls, 1).astype(np.uint8)
    want_rs = np.zeros(len(jobs), F32)
    want_rs[inside] = t_rs[named % STRIDE_TEMPLATES]
    got = run_cg((ptr, idx, val, V, G), STATUS_ALPHA, STRIDE_STEPS, None, jobs, pad=2)
    assert_same(got, (want_st, want_rs, want_out), f"dim {dim}")


# ---------------------------------------------------------------------------------------------- 5. through the engine
ENGINE_FIT = dict(iterations=2, regularization=0.01, alpha=1.0, seed=0)


@functools.lru_cache(maxsize=None)
def engine_reference(dim):
    """(X, P, Q, user status, item status) of host_fit_cg on 1,100 users x 120 items, computed once and read-only."""
    X = block_data(0, users_per=275)
    P, Q, su, si = host_fit_cg(X, dim, 2, 0.01, 1.0, 0, cg_steps=3)
    for a in (P, Q, su, si):
        a.setflags(write=False)
    return X, P, Q, su, si


@pytest.mark.parametrize("dim", [40, 96])
def test_fit_factors_cg_on_the_device_equals_the_host_stack(dim):
    """1,100 users of 8 items each in 4 clusters of 30 items: the item half-step's Gram matrix has two chunks and its rows about
    73 entries (two blocks); dim 40 takes the narrow Gram call, dim 96 the wide one and two waves.  After 2 iterations P and Q
    carry the host model's bits, the factor and hybrid lists are those of the CPU stand-in stack with the host model's vectors
    attached (and the device model's W), and a half-step over named rows equals the host model's."""
    import scipy.sparse as sp
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    from tests.test_als_cg_host import als_cg_backend
    from tests.test_als_host import attach_host_vectors, resident_x
    X, P, Q, su, si = engine_reference(dim)
    assert (su == 0).all() and (si == 0).all() and np.diff(X.tocsc().indptr).max() > 64
    coo = X.tocoo()
    batch = [(int(u), int(i), 1000.0, float(v)) for u, i, v in zip(coo.row, coo.col, coo.data)]
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=F32)
    assert m.fit_factors(dim=dim, solver="cg", cg_steps=3, **ENGINE_FIT) is m and m.has_factors()
    assert (resident_x(m) != X).nnz == 0
    F = m._factors
    assert np.array_equal(F["user_rows"], np.arange(1100)) and np.array_equal(F["item_rows"], np.arange(120))
    assert np.array_equal(bits(F["user_vectors"]), bits(P)) and np.array_equal(bits(F["item_vectors"]), bits(Q))
    ref = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    ref.model._engine = SlimEngine(backend=als_cg_backend())
    ref.fit(batch, progress_bar=False)
    ref.model.item_similarity = m.model.item_similarity.copy()
    attach_host_vectors(ref, P, su, Q, si)
    users = list(range(0, 1100, 7)) + [10 ** 6]
    assert m.recommend_factor_batch(users, top_k=5) == ref.recommend_factor_batch(users, top_k=5)
    for h in (dict(top_k=6), dict(top_k=5, pool=12, weighting=0.5)):
        assert m.recommend_hybrid_batch(users, **h) == ref.recommend_hybrid_batch(users, **h), h
    # a half-step over named rows, warm-started from the trained vectors
    eng = m.model.engine
    rows = [3, 1099, 500, 64]
    counts = eng.als_half_step("user", rows=rows)
    assert counts == {0: 4, 1: 0, 2: 0}
    Ph = np.array(P)
    st = cg_half_step(X, np.array(Q), 0.01, 1.0, Ph, job_rows=np.array(sorted(rows)), cg_steps=3)
    assert (st == 0).all() and not np.array_equal(bits(Ph[rows]), bits(P[rows]))
    got = eng.als_vectors()[0]
    assert np.array_equal(bits(got), bits(Ph))
    # the online call through the model: the named users alone
    m.update_factors([3, 64])
    ref._factor_training = dict(m._factor_training)
    ref.update_factors([3, 64])
    assert np.array_equal(bits(m._factors["user_vectors"]), bits(ref._factors["user_vectors"]))
