"""Training the factor scorer on the GPU (csrc/factor_gram.hip, csrc/factor_als.hip, torch.ops.rtrec_amd.factor_gram /
factor_als_solve, SLIM.fit_factors) against the host models of tests/test_als_host.py: the status with ==, every Gram element and
every solved vector by its bits after adding +0.0f (the sign of a zero is not part of the contract).  Both kernels build their
matrices with the f32-input MFMA; these tests are what says that it is the fmaf chain of the contract, bit for bit.  The output
buffers carry a sentinel before every call: what a call must not touch keeps it."""
import numpy as np
import pytest

from tests.test_als_host import F32, als_case, bits, block_data, gram_fast, host_fit, solve_fast
from tests.test_factor_host import rounding_vectors

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


def up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")


def run_gram(V, reg, pad=0):
    """torch.ops.rtrec_amd.factor_gram on a host matrix; `pad` > 0: the stride is wider than dim, with NaN behind it."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    V = np.asarray(V, F32)
    n, dim = V.shape
    Vd = np.concatenate([V, np.full((n, pad), np.nan, F32)], axis=1) if pad else V
    gram = torch.full((dim, dim), SENTINEL, dtype=torch.float32, device="cuda:0")
    chunks = (n + 1023) // 1024
    ws = torch.full((chunks * dim * dim,), np.nan, dtype=torch.float32, device="cuda:0") if chunks else None
    torch.ops.rtrec_amd.factor_gram(up(Vd, np.float32) if n else torch.zeros((0, dim + pad), device="cuda:0"), n, dim, float(reg), gram, ws)
    torch.cuda.synchronize()
    return gram.cpu().numpy()


def run_solve(ptr, idx, val, V, G, alpha, jobs=None, pad=0):
    """torch.ops.rtrec_amd.factor_als_solve on host arrays: (status[n_jobs], out[n_rows, dim + pad]) with the sentinel wherever
    the call wrote nothing; `pad` > 0 widens both strides (NaN behind V's components)."""
    import torch
    from rtrec_amd import ops  # noqa: F401
    V = np.asarray(V, F32)
    n_v, dim = V.shape
    n_rows = len(ptr) - 1
    Vd = np.concatenate([V, np.full((n_v, pad), np.nan, F32)], axis=1) if pad else V
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
@pytest.mark.parametrize("dim", [1, 7, 32, 33, 64])
def test_gram_is_the_chunked_fmaf_chain_bit_for_bit(dim):
    """Cancelling 2^24 terms, midpoint products and denormals (rounding_vectors): another order of the rows, an unfused multiply,
    a wider accumulator or another chunk size changes bits.  1023 / 1024 / 1025 rows stand on both sides of the chunk."""
    for n in (1, 1023, 1024, 1025, 3000):
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
