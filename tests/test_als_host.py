"""Training the factor scorer (SLIM.fit_factors / update_factors, csrc/factor_gram.hip, csrc/factor_als.hip) without a GPU: the
definition of an implicit-feedback ALS half-step as a plain-Python host model, one libm fmaf at a time, and a vectorised one
(fma32 over the jobs, np.sqrt and / on float32); that each pinned operation is visible in the bits; the accuracy of the solve
against float64; descent and sense on block-structured data; the model / facade / serving layers through the CPU stand-in
backend with `factor_gram` / `factor_als_solve` supplied by the host model; the rules of the extension surface and the C entry
points' host-side checks.  The kernels are in tests/test_gpu_als.py.

The definition (include/rtrec_amd_ext.h, "FACTOR GRAM" and "FACTOR ALS SOLVE"): G = the sum over chunks of 1024 rows, in
ascending order, of the fmaf chains v_r[a] * v_r[b] over the chunk's rows, plus reg on the diagonal.  A job names row x of the
CSR R; an entry (i, val) is usable when 0 <= i < n_v and w = fl(alpha * val) > 0; A = G, then fmaf(fl(w * y_i[a]), y_i[b], A[a][b])
over the usable entries in storage order (lower triangle), rhs = fmaf(fl(1 + w), y_i[a], rhs[a]); a left-looking Cholesky whose
every element is one fmaf chain over ascending k, a forward and a backward substitution, one division per component."""
import ctypes
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_factor_host import bits, fma32, fmaf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24
CHUNK = 1024                                     # rows of V per partial Gram: a constant of the contract


# ---------------------------------------------------------------------------------------------- the host models
def gram_plain(V, reg):
    """THE DEFINITION of rtrec_factor_gram, one fmaf at a time: G[dim, dim] float32."""
    V = np.asarray(V, F32)
    n, dim = V.shape
    G = np.zeros((dim, dim), F32)
    for c0 in range(0, n, CHUNK):
        part = np.zeros((dim, dim), F32)
        for r in range(c0, min(n, c0 + CHUNK)):
            for a in range(dim):
                for b in range(dim):
                    part[a, b] = fmaf(V[r, a], V[r, b], part[a, b])
        for a in range(dim):
            for b in range(dim):
                G[a, b] = F32(G[a, b] + part[a, b])
    for a in range(dim):
        G[a, a] = F32(G[a, a] + F32(reg))
    return G


def gram_fast(V, reg):
    """gram_plain, vectorised: all chunks side by side, one fma32 per position inside a chunk."""
    V = np.asarray(V, F32)
    n, dim = V.shape
    n_chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((n_chunks * CHUNK, dim), F32)          # (a zero row adds fmaf(0, 0, p) = p)
    pad[:n] = V
    pad = pad.reshape(n_chunks, CHUNK, dim)
    part = np.zeros((n_chunks, dim, dim), F32)
    for t in range(min(CHUNK, n)):
        live = min(n_chunks, (n - t + CHUNK - 1) // CHUNK)             # chunks that hold a row at position t
        v = pad[:live, t]
        part[:live] = fma32(v[:, :, None], v[:, None, :], part[:live])
    G = np.zeros((dim, dim), F32)
    with np.errstate(all="ignore"):
        for c in range(n_chunks):
            G = G + part[c]
        G[np.arange(dim), np.arange(dim)] += F32(reg)
    return G


def _row_entries(ptr, idx, val, x, n_v, alpha):
    """(columns, w) of the usable entries of row x in storage order; offsets clamped to [0, nnz]."""
    nnz = len(idx)
    s, e = int(np.clip(ptr[x], 0, nnz)), int(np.clip(ptr[x + 1], 0, nnz))
    ii = np.asarray(idx[s:e], np.int64)
    with np.errstate(all="ignore"):
        w = F32(alpha) * np.asarray(val[s:e], F32)
        ok = (ii >= 0) & (ii < n_v) & (w > 0)
    return ii[ok], w[ok]


def solve_plain(ptr, idx, val, V, G, alpha, out, job_rows=None):
    """THE DEFINITION of rtrec_factor_als_solve, one fmaf at a time: writes the vectors into `out` [n_rows, >= dim] in place and
    returns status[n_jobs] uint8."""
    V, G = np.asarray(V, F32), np.asarray(G, F32)
    n_v, dim = V.shape
    n_rows = len(ptr) - 1
    jobs = np.arange(n_rows) if job_rows is None else np.asarray(job_rows, np.int64)
    status = np.zeros(len(jobs), np.uint8)
    zero = F32(0.0)
    for r, x in enumerate(jobs):
        if not 0 <= x < n_rows:
            status[r] = 1
            continue
        cols, ws = _row_entries(ptr, idx, val, x, n_v, alpha)
        if not len(cols):
            status[r] = 1
            out[x, :dim] = 0
            continue
        A = [[G[a, b] for b in range(dim)] for a in range(dim)]
        rhs = [zero] * dim
        with np.errstate(all="ignore"):
            for i, w in zip(cols, ws):
                y = V[i]
                c = F32(F32(1.0) + w)
                for a in range(dim):
                    wy = F32(w * y[a])
                    for b in range(a + 1):
                        A[a][b] = fmaf(wy, y[b], A[a][b])
                    rhs[a] = fmaf(c, y[a], rhs[a])
            L = [[zero] * dim for _ in range(dim)]
            broken = False
            for j in range(dim):
                d = A[j][j]
                for k in range(j):
                    d = fmaf(-L[j][k], L[j][k], d)
                if not (d > 0) or not np.isfinite(d):
                    broken = True
                    break
                L[j][j] = F32(np.sqrt(F32(d)))
                for i in range(j + 1, dim):
                    s = A[i][j]
                    for k in range(j):
                        s = fmaf(-L[i][k], L[j][k], s)
                    L[i][j] = F32(s / L[j][j])
            x_out = [zero] * dim
            if not broken:
                z = [zero] * dim
                for j in range(dim):
                    s = rhs[j]
                    for k in range(j):
                        s = fmaf(-L[j][k], z[k], s)
                    z[j] = F32(s / L[j][j])
                for j in range(dim - 1, -1, -1):
                    s = z[j]
                    for k in range(dim - 1, j, -1):
                        s = fmaf(-L[k][j], x_out[k], s)
                    x_out[j] = F32(s / L[j][j])
                broken = not np.isfinite(np.array(x_out, F32)).all()
        status[r] = 2 if broken else 0
        out[x, :dim] = 0 if broken else np.array(x_out, F32)
    return status


VARIANTS = ("unfused", "reverse", "right_looking", "float64", "w_other")


def solve_fast(ptr, idx, val, V, G, alpha, out, job_rows=None, variant=None):
    """solve_plain, vectorised over the jobs (sorted by length, so that the jobs still building are a prefix): every fused step
    through fma32, np.sqrt and / on float32.  `variant` swaps ONE pinned operation for what another implementation might do
    (test_each_pinned_operation_shows_in_the_bits): "unfused" rounds the build's product and sum separately; "reverse" takes the
    entries last first; "right_looking" is the textbook outer-product Cholesky in float32 (A -= l l^T, a rounded product and a
    rounded difference: with fused updates the right-looking order gives the very chains of the left-looking one, element by
    element); "float64" builds A and rhs in a float64 accumulator and rounds once; "w_other" scales the other operand,
    fmaf(y[a], fl(w * y[b]), A)."""
    assert variant is None or variant in VARIANTS
    V, G = np.asarray(V, F32), np.asarray(G, F32)
    n_v, dim = V.shape
    n_rows = len(ptr) - 1
    jobs = np.arange(n_rows) if job_rows is None else np.asarray(job_rows, np.int64)
    status = np.zeros(len(jobs), np.uint8)
    entries = {}
    for r, x in enumerate(jobs):
        if not 0 <= x < n_rows:
            status[r] = 1
            continue
        cols, ws = _row_entries(ptr, idx, val, x, n_v, alpha)
        if not len(cols):
            status[r] = 1
            out[x, :dim] = 0
            continue
        entries[r] = (cols[::-1], ws[::-1]) if variant == "reverse" else (cols, ws)
    if not entries:
        return status
    live = sorted(entries, key=lambda r: -len(entries[r][0]))
    J, longest = len(live), len(entries[live[0]][0])
    lens = np.array([len(entries[r][0]) for r in live])
    cols = np.zeros((J, longest), np.int64)
    ws = np.zeros((J, longest), F32)
    for a, r in enumerate(live):
        cols[a, :lens[a]], ws[a, :lens[a]] = entries[r]
    wide = variant == "float64"
    with np.errstate(all="ignore"):
        A = np.broadcast_to(G, (J, dim, dim)).astype(np.float64 if wide else F32)
        rhs = np.zeros((J, dim), np.float64 if wide else F32)
        for t in range(longest):
            n = int((lens > t).sum())
            y, w = V[cols[:n, t]], ws[:n, t]
            wy = w[:, None] * y
            c = (F32(1.0) + w)[:, None]
            if wide:
                A[:n] += wy.astype(np.float64)[:, :, None] * y.astype(np.float64)[:, None, :]
                rhs[:n] += c.astype(np.float64) * y.astype(np.float64)
            elif variant == "unfused":
                A[:n] = A[:n] + wy[:, :, None] * y[:, None, :]
                rhs[:n] = fma32(c, y, rhs[:n])
            elif variant == "w_other":
                A[:n] = fma32(y[:, :, None], wy[:, None, :], A[:n])
                rhs[:n] = fma32(c, y, rhs[:n])
            else:
                A[:n] = fma32(wy[:, :, None], y[:, None, :], A[:n])
                rhs[:n] = fma32(c, y, rhs[:n])
        A, rhs = A.astype(F32), rhs.astype(F32)
        L = np.zeros((J, dim, dim), F32)
        broken = np.zeros(J, bool)
        for j in range(dim):
            s = A[:, j:, j].copy()
            if variant != "right_looking":
                for k in range(j):
                    s = fma32(-L[:, j:, k], L[:, j, k][:, None], s)
            d = s[:, 0]
            broken |= ~((d > 0) & np.isfinite(d))
            root = np.sqrt(d)
            L[:, j, j] = root
            L[:, j + 1:, j] = s[:, 1:] / root[:, None]
            if variant == "right_looking":
                l = L[:, j + 1:, j]
                A[:, j + 1:, j + 1:] = A[:, j + 1:, j + 1:] - l[:, :, None] * l[:, None, :]
        diag = L[:, np.arange(dim), np.arange(dim)]
        s = rhs.copy()
        for k in range(dim):                          # forward: component k is final once the columns below k are applied
            s[:, k] = s[:, k] / diag[:, k]
            s[:, k + 1:] = fma32(-L[:, k + 1:, k], s[:, k][:, None], s[:, k + 1:])
        for k in range(dim - 1, -1, -1):              # backward: every component takes x[k] for k descending
            s[:, k] = s[:, k] / diag[:, k]
            s[:, :k] = fma32(-L[:, k, :k], s[:, k][:, None], s[:, :k])
        broken |= ~np.isfinite(s).all(axis=1)
    for a, r in enumerate(live):
        status[r] = 2 if broken[a] else 0
        out[jobs[r], :dim] = 0 if broken[a] else s[a]
    return status


def half_step(R, V, reg, alpha, out, job_rows=None, fast=True):
    """One half-step by the host model: the Gram of V, then the solve of R's rows (a scipy CSR, float32 values) into `out`."""
    G = (gram_fast if fast else gram_plain)(V, reg)
    return (solve_fast if fast else solve_plain)(R.indptr, R.indices, R.data, V, G, alpha, out, job_rows)


def host_fit(X, dim, iterations, reg, alpha, seed, trace=None):
    """SlimEngine.fit_factors by the host model: (P, Q, user status, item status).  Only the item matrix is initialised; the user
    half-step runs first.  `trace(P, Q)` is called after every half-step."""
    X = sp.csr_matrix(X, dtype=F32)
    X.sort_indices()
    Xt = sp.csr_matrix(X.T.tocsr(), dtype=F32)
    Xt.sort_indices()
    n_users, n_items = X.shape
    Q = np.random.default_rng(seed).standard_normal((n_items, dim)).astype(F32) * F32(0.01)
    P = np.zeros((n_users, dim), F32)
    su, si = np.ones(n_users, np.uint8), np.ones(n_items, np.uint8)
    for _ in range(iterations):
        su = half_step(X, Q, reg, alpha, P)
        if trace:
            trace(P, Q)
        si = half_step(Xt, P, reg, alpha, Q)
        if trace:
            trace(P, Q)
    return P, Q, su, si


# ---------------------------------------------------------------------------------------------- inputs
def als_case(n_rows, n_v, dim, seed, lengths=(0, 1, 2, 3, 40), scale=1.0):
    """A CSR R [n_rows, n_v] whose rows have the given lengths in turn (columns in a shuffled order: storage order is the
    contract, not column order), with skipped entries -- zero, negative and NaN values, columns outside [0, n_v) -- among them,
    and a row of V that is NaN but reachable only through a skipped entry.  Returns (ptr, idx, val, V)."""
    rng = np.random.default_rng(seed)
    V = (rng.standard_normal((n_v, dim)) * scale).astype(F32)
    poisoned = n_v - 1
    V[poisoned] = np.nan
    ptr, idx, val = [0], [], []
    for r in range(n_rows):
        n = lengths[r % len(lengths)]
        cols = rng.choice(n_v - 1, size=min(n, n_v - 1), replace=False) if n else np.zeros(0, np.int64)
        vals = rng.integers(1, 6, len(cols)).astype(F32) * F32(0.5)
        extra_c = [poisoned, poisoned, poisoned, -1, n_v, n_v + 7]
        extra_v = [0.0, -2.0, np.nan, 1.0, 2.0, 3.0]
        k = int(rng.integers(0, 4)) if r % 3 else 0
        for _ in range(k):
            at, e = int(rng.integers(0, len(cols) + 1)), int(rng.integers(0, len(extra_c)))
            cols, vals = np.insert(cols, at, extra_c[e]), np.insert(vals, at, F32(extra_v[e]))
        idx += cols.tolist()
        val += vals.tolist()
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, F32), V


def block_data(seed=0, clusters=4, items_per=30, users_per=50, rated=8):
    """The block-structured interactions of the descent test: every user rates `rated` items of its own cluster with 1..5."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for u in range(clusters * users_per):
        c = u // users_per
        rows += [u] * rated
        cols += (c * items_per + rng.choice(items_per, rated, replace=False)).tolist()
        vals += rng.integers(1, 6, rated).tolist()
    X = sp.csr_matrix((np.array(vals, F32), (rows, cols)), shape=(clusters * users_per, clusters * items_per))
    X.sort_indices()
    return X


def als_loss(X, P, Q, reg, alpha):
    """sum_ui c_ui (p_ui - x_u . y_i)^2 + reg (|P|^2 + |Q|^2) over ALL pairs in float64, c = 1 + alpha r, p = [r > 0]."""
    Xd = np.asarray(X.todense(), np.float64)
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    c = 1.0 + alpha * np.where(Xd > 0, Xd, 0.0)
    return float((c * ((Xd > 0) - P @ Q.T) ** 2).sum() + reg * ((P ** 2).sum() + (Q ** 2).sum()))


# ---------------------------------------------------------------------------------------------- the two models agree
@pytest.mark.parametrize("dim", [1, 2, 5, 33])
def test_both_models_agree_bit_for_bit(dim):
    n_v = 1030 if dim <= 2 else 37                       # (dim 1 and 2 cross the chunk of 1024 rows in the plain model too)
    ptr, idx, val, V = als_case(23, n_v, dim, seed=dim)
    Vg = np.nan_to_num(V)                                # (the Gram reads every row)
    Gp, Gf = gram_plain(Vg, 0.05), gram_fast(Vg, 0.05)
    assert np.array_equal(bits(Gp), bits(Gf)) and np.array_equal(bits(Gp), bits(Gp.T))
    jobs = np.r_[np.random.default_rng(dim).permutation(23), -1, 23]
    outs = []
    for solve in (solve_plain, solve_fast):
        out = np.full((23, dim + 2), 7.0, F32)
        outs.append((solve(ptr, idx, val, V, Gp, 0.7, out, jobs), out))
    (sp_, op), (sf, of) = outs
    assert np.array_equal(sp_, sf) and np.array_equal(bits(op), bits(of))
    assert (op[:, dim:] == 7).all() and sp_[-1] == 1 and sp_[-2] == 1
    lengths = np.array([(0, 1, 2, 3, 40)[x % 5] for x in jobs[:-2]])
    assert (sp_[:-2][lengths == 0] == 1).all() and (op[jobs[:-2][lengths == 0], :dim] == 0).all()
    assert (sp_[:-2][lengths > 0] == 0).all() and np.isfinite(op[:, :dim]).all()


def test_gram_of_nothing_and_breakdowns():
    assert np.array_equal(gram_fast(np.zeros((0, 3), F32), 0.25), np.eye(3, dtype=F32) * F32(0.25))
    assert np.array_equal(gram_plain(np.zeros((0, 3), F32), 0.25), np.eye(3, dtype=F32) * F32(0.25))
    ptr, idx, val = np.array([0, 2, 2], np.int32), np.array([0, 1], np.int32), np.array([1, 1], F32)
    for solve in (solve_plain, solve_fast):
        out = np.full((2, 3), 7.0, F32)
        st = solve(ptr, idx, val, np.zeros((2, 3), F32), np.zeros((3, 3), F32), 1.0, out)       # reg = 0 and V = 0: d = 0
        assert st.tolist() == [2, 1] and (out == 0).all()
        G = np.eye(3, dtype=F32)
        G[2, 1] = np.nan
        out = np.full((2, 3), 7.0, F32)
        assert solve(ptr, idx, val, np.ones((2, 3), F32), G, 1.0, out).tolist() == [2, 1] and (out == 0).all()
        out = np.full((2, 3), 7.0, F32)                                                      # offsets beyond nnz are clamped
        assert solve(np.array([0, 9, -4], np.int32), idx, val, np.ones((2, 3), F32), np.eye(3, dtype=F32), 1.0, out).tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------- every pinned operation shows
def test_each_pinned_operation_shows_in_the_bits():
    """One seeded case (200 rows of 1 .. 90 entries, dim 12, all solved): the number of the 2,400 output components whose bits
    change when ONE operation of the definition is swapped for what another implementation might do (solve_fast's variants).
    Measured with this host model: unfused build 609, entries in reverse order 1378, textbook right-looking Cholesky 253,
    float64 accumulator 1506, w on the other operand 393.  A kernel that took any of these liberties could not equal the host
    model in tests/test_gpu_als.py."""
    ptr, idx, val, V = als_case(200, 300, 12, seed=12, lengths=(1, 2, 3, 7, 20, 40, 90), scale=0.5)
    G = gram_fast(np.nan_to_num(V), 0.01)
    base = np.zeros((200, 12), F32)
    assert (solve_fast(ptr, idx, val, V, G, 1.0, base) == 0).all()
    counts = {}
    for variant in VARIANTS:
        out = np.zeros((200, 12), F32)
        solve_fast(ptr, idx, val, V, G, 1.0, out, variant=variant)
        counts[variant] = int((bits(out) != bits(base)).sum())
    print(counts)
    assert all(counts[v] > 0 for v in VARIANTS), counts


# ---------------------------------------------------------------------------------------------- accuracy
ACCURACY_MEASURED = 5.93        # the largest err / (2^-24 cond_2(A)) of the host model on the cases below (dim 8, reg 1)
ACCURACY_BOUND = 4 * ACCURACY_MEASURED


@pytest.mark.parametrize("dim", [8, 32, 64])
@pytest.mark.parametrize("reg", [0.01, 1.0])
def test_the_solve_is_as_accurate_as_the_conditioning_allows(dim, reg):
    """Against np.linalg.solve of the same system built in float64: err / (2^-24 * cond_2(A)) per row, err the relative 2-norm
    error.  Measured with the host model on these cases: 5.83 / 5.92 (dim 8, reg 0.01 / 1), 4.68 / 3.55 (dim 32), 3.07 / 3.29
    (dim 64); the bound is 4 times the largest.  The margin covers other seeds (7.9 was seen on seed 1), not the kernel: the
    kernel must equal the host model exactly."""
    ptr, idx, val, V = als_case(60, 500, dim, seed=0, lengths=(1, 3, 10, 40, 150), scale=0.3)
    V = np.nan_to_num(V)
    out = np.zeros((60, dim), F32)
    status = solve_fast(ptr, idx, val, V, gram_fast(V, reg), 1.0, out)
    V64 = V.astype(np.float64)
    G64 = V64.T @ V64 + reg * np.eye(dim)
    worst = 0.0
    for x in np.flatnonzero(status == 0):
        cols, ws = _row_entries(ptr, idx, val, x, len(V), 1.0)
        Y, w = V64[cols], ws.astype(np.float64)
        A = G64 + (Y * w[:, None]).T @ Y
        ref = np.linalg.solve(A, ((1.0 + w)[:, None] * Y).sum(axis=0))
        err = np.linalg.norm(out[x] - ref) / np.linalg.norm(ref)
        worst = max(worst, err / (U * np.linalg.cond(A, 2)))
    print(f"dim {dim} reg {reg}: worst ratio {worst:.3f} (bound {ACCURACY_BOUND:.2f})")
    assert (status == 0).sum() == 60 and 0 < worst <= ACCURACY_BOUND


# ---------------------------------------------------------------------------------------------- descent and sense
def test_every_half_step_descends_and_the_lists_stay_in_the_cluster():
    """4 clusters of 30 items, 50 users each rating 8 items of their own cluster: each of the 16 half-steps lowers the float64
    loss by more than 1e-3 relative (the smallest decrease measured with this host model on seed 0: 3.10e-3; 3.34e-3 and 3.31e-3
    on seeds 1 and 2), and after 8 iterations every user's factor top-5, interacted items filtered, lies inside its cluster."""
    X = block_data(0)
    losses = []
    P, Q, su, si = host_fit(X, 8, 8, 0.01, 1.0, 0, trace=lambda P, Q: losses.append(als_loss(X, P, Q, 0.01, 1.0)))
    assert len(losses) == 16 and (su == 0).all() and (si == 0).all()
    Q0 = np.random.default_rng(0).standard_normal((120, 8)).astype(F32) * F32(0.01)
    losses = [als_loss(X, np.zeros((200, 8), F32), Q0, 0.01, 1.0)] + losses
    rel = [(a - b) / a for a, b in zip(losses[:-1], losses[1:])]
    print("smallest relative decrease", min(rel))
    assert min(rel) > 1e-3, rel
    from tests.test_factor_host import host_model_fast
    ids, _, cnt = host_model_fast(P, Q, 5, X=X, filter_interacted=True)
    assert (cnt == 5).all() and (ids // 30 == (np.arange(200) // 50)[:, None]).all()


# ---------------------------------------------------------------------------------------------- model / facade, end to end
def _csr_of(t3):
    ptr, idx, val = [t.numpy() for t in t3]
    return ptr, idx, val


def als_backend():
    from tests.test_factor_host import FactorOracleBackend

    class AlsOracleBackend(FactorOracleBackend):
        """The CPU stand-in with factor_gram / factor_als_solve from the host model (TEST-ONLY, like its bases)."""

        def factor_gram(self, v, n_v, dim, reg, gram):
            import torch
            gram.copy_(torch.from_numpy(gram_fast(v.numpy()[:n_v, :dim], reg)))

        def factor_als_solve(self, job_rows, n_jobs, r_csr, v, n_v, dim, gram, alpha, out, status):
            import torch
            ptr, idx, val = _csr_of(r_csr)
            jobs = np.arange(n_jobs) if job_rows is None else job_rows.numpy()
            o = out.numpy()                                   # (shares the tensor's memory: written in place)
            status.copy_(torch.from_numpy(solve_fast(ptr, idx, val, v.numpy()[:n_v, :dim], gram.numpy(), alpha, o, jobs)))

    return AlsOracleBackend()


def als_model(extra=()):
    """The golden fixture model of tests/test_factor_host.py on the stand-in above; `extra` interactions join the batch."""
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    from tests.test_rerank_host import _batch
    batch = _batch(False) + list(extra)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.model._engine = SlimEngine(backend=als_backend())
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=F32)
    return m, batch


def resident_x(m):
    X = sp.csr_matrix(m.interactions.to_csr(), dtype=F32)
    X.sort_indices()
    return X


def attach_host_vectors(ref, P, su, Q, si):
    """attach_factors of the host model's vectors through raw ids, in ascending internal id."""
    urows, irows = np.flatnonzero(su == 0), np.flatnonzero(si == 0)
    return ref.attach_factors([ref.user_ids.get(int(r)) for r in urows], P[urows], [ref.item_ids.get(int(i)) for i in irows], Q[irows])


FIT = dict(dim=6, iterations=2, regularization=0.05, alpha=0.5, seed=3)


def test_fit_factors_equals_attach_factors_of_the_host_models_vectors():
    from rtrec_amd.recommender import Recommender
    m, batch = als_model()
    users = sorted({u for u, _, _, _ in batch})
    assert not m.has_factors() and m.fit_factors(**FIT) is m and m.has_factors()
    P, Q, su, si = host_fit(resident_x(m), FIT["dim"], FIT["iterations"], FIT["regularization"], FIT["alpha"], FIT["seed"])
    assert (su == 0).sum() > 100 and (si == 0).sum() > 30
    ref, _ = als_model()
    attach_host_vectors(ref, P, su, Q, si)
    for key in ("user_rows", "user_vectors", "item_rows", "item_vectors"):
        a, b = m._factors[key], ref._factors[key]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a) if a.dtype == F32 else a, bits(b) if b.dtype == F32 else b), key
    assert sorted(m._serialize()) == sorted(ref._serialize()) and sorted(m._serialize()["factors"]) == sorted(ref._serialize()["factors"])
    ask = users[:40] + [max(users) + 1000] + users[40:]
    assert m.recommend_factor_batch(ask, top_k=7) == ref.recommend_factor_batch(ask, top_k=7)
    got, want = m.recommend_factor_batch(ask, top_k=7, as_arrays=True), ref.recommend_factor_batch(ask, top_k=7, as_arrays=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for kw in (dict(top_k=8), dict(top_k=6, weighting=0.6), dict(top_k=5, pool=12, filter_interacted=False)):
        assert m.recommend_hybrid_batch(ask, **kw) == ref.recommend_hybrid_batch(ask, **kw), kw
    # the engine holds what set_factors would hold: P row-major, Q component-major, -1 / 0 where there is no vector
    E = m.model.engine._F
    assert tuple(E["p"].shape) == (len(su), 6) and tuple(E["qt"].shape) == (6, m.model.n_items_fitted) and E["dim"] == 6
    assert np.array_equal(E["index"].numpy() >= 0, su == 0) and np.array_equal(E["mask"].numpy() != 0, si[:m.model.n_items_fitted] == 0)
    assert np.array_equal(bits(E["qt"].numpy().T), bits(Q[:m.model.n_items_fitted]))
    # a pickle carries the vectors, and the facade passes through
    buf = io.BytesIO()
    m.save(buf)
    from rtrec_amd.engine import SlimEngine
    back = type(m).loads(buf.getvalue())
    back.model._engine = SlimEngine(backend=als_backend())
    assert back.has_factors() and back.recommend_factor_batch(ask, top_k=7) == m.recommend_factor_batch(ask, top_k=7)
    rec = Recommender(als_model()[0])
    assert rec.fit_factors(**FIT) is rec and rec.recommend_factor_batch(ask, top_k=7) == m.recommend_factor_batch(ask, top_k=7)
    assert rec.update_factors(users[:3]) is rec


def test_a_user_without_positive_interactions_gets_the_cold_start_list():
    m, batch = als_model()
    users = sorted({u for u, _, _, _ in batch})
    m.fit_factors(**FIT)
    X = resident_x(m)
    # no row of the fixture is empty, so one is made: the user's vector is taken away as a failed solve would
    row = m._known_user_id(users[4])
    keep = m._factors["user_rows"] != row
    m._factors = dict(m._factors, user_rows=m._factors["user_rows"][keep], user_vectors=m._factors["user_vectors"][keep])
    m._factors_on_device = None
    cold = m.recommend_batch([max(users) + 1000], top_k=6)[0]
    assert m.recommend_factor_batch([users[4]], top_k=6)[0] == cold[:6]
    # and the host model gives such a row status 1 and no vector
    Xz = X.copy().tolil()
    Xz[row, :] = 0
    Xz = sp.csr_matrix(Xz.tocsr(), dtype=F32)
    P, Q, su, si = host_fit(Xz, 6, 1, 0.05, 0.5, 3)
    assert su[row] == 1 and (P[row] == 0).all() and (np.delete(su, row) == 0).all()


def test_update_factors_is_a_user_half_step_on_the_named_rows():
    m, batch = als_model()
    users = sorted({u for u, _, _, _ in batch})
    items = sorted({i for _, i, _, _ in batch})
    m.fit_factors(**FIT)
    before = {k: v.copy() for k, v in m._factors.items()}
    a, newcomer = users[7], max(users) + 5
    t = max(ts for _, _, ts, _ in batch) + 1.0
    m.fit([(a, items[3], t, 4.0), (a, items[11], t, 2.0), (newcomer, items[3], t, 5.0), (newcomer, items[20], t, 3.0)],
          progress_bar=False)                        # (SLIM.fit is incremental: it ingests and refits the items touched)
    assert m.update_factors([a, newcomer, max(users) + 999]) is m
    X = resident_x(m)
    n_users, dim = X.shape[0], FIT["dim"]
    P = np.zeros((n_users, dim), F32)
    P[before["user_rows"]] = before["user_vectors"]
    Q = np.zeros((X.shape[1], dim), F32)
    Q[before["item_rows"]] = before["item_vectors"]
    rows = [m._known_user_id(a), m._known_user_id(newcomer)]
    st = half_step(X, Q, FIT["regularization"], FIT["alpha"], P, job_rows=np.array(sorted(rows)))
    assert (st == 0).all() and rows[1] not in before["user_rows"]
    after = m._factors
    assert np.array_equal(after["item_rows"], before["item_rows"]) and np.array_equal(bits(after["item_vectors"]), bits(before["item_vectors"]))
    assert sorted(after["user_rows"].tolist()) == sorted(before["user_rows"].tolist() + [rows[1]])
    for r, vec in zip(after["user_rows"], after["user_vectors"]):
        assert np.array_equal(bits(vec), bits(P[r])), r
    changed = [r for r, vec in zip(before["user_rows"], before["user_vectors"]) if not np.array_equal(bits(vec), bits(P[r]))]
    assert changed == [rows[0]]
    assert m.recommend_factor_batch([newcomer], top_k=5)[0] and items[3] not in m.recommend_factor_batch([newcomer], top_k=5)[0]


def test_refusals():
    from rtrec_amd.models.slim import SLIM
    m, batch = als_model()
    users = sorted({u for u, _, _, _ in batch})
    with pytest.raises(RuntimeError, match="fit_factors"):
        m.update_factors(users[:2])
    for kw in (dict(dim=0), dict(dim=65), dict(iterations=0), dict(regularization=-1.0), dict(alpha=0.0), dict(alpha=float("nan"))):
        with pytest.raises(ValueError):
            m.fit_factors(**kw)
    m.recommend_batch(users[:1])
    eng = m.model.engine
    m._sync_interactions_csc()
    eng.world_size = 2                                     # several ranks: as the other factor calls
    try:
        with pytest.raises(ValueError, match="rank"):
            eng.fit_factors(dim=4, iterations=1)
    finally:
        eng.world_size = 1
    dw = eng._W["dw"]
    had = getattr(dw, "shard", None)
    dw.shard = (0, 1)                                      # a column-sharded W
    try:
        with pytest.raises(ValueError, match="column-sharded"):
            eng.fit_factors(dim=4, iterations=1)
    finally:
        dw.shard = had
    with pytest.raises(RuntimeError, match="als_begin"):
        eng.als_half_step("user")
    eng.fit_factors(dim=4, iterations=1)
    with pytest.raises(ValueError, match="side"):
        eng.als_half_step("both")
    counts = eng.als_half_step("item", rows=[0, 1, 2, 10 ** 6, -1])
    assert sum(counts.values()) == 3 and set(counts) == {0, 1, 2}
    assert SLIM.fit_factors.__defaults__ == (32, 15, 0.01, 1.0, 0)


def test_fit_factors_route():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = als_model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    r = client.post("/fit_factors", json={"dim": 4}, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and not m.has_factors()
    r = client.post("/fit_factors", json={"dim": 4, "iterations": 1, "seed": 2}, headers=ok)
    assert r.status_code == 200 and r.json() == {"message": "Factor training successful"} and m.has_factors()
    want, _ = als_model()
    want.fit_factors(dim=4, iterations=1, seed=2)
    user = batch[0][0]
    r = client.post("/recommend_hybrid", json={"user": user, "top_k": 5}, headers=ok)
    assert r.status_code == 200 and r.json()["items"] == want.recommend_hybrid(user, top_k=5)
    assert client.post("/fit_factors", json={"dim": 65}, headers=ok).status_code == 500


# ---------------------------------------------------------------------------------------------- registration
def test_the_two_calls_are_declared_registered_and_exported():
    import re
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from rtrec_amd.engine import SlimEngine
    from tests.test_diverse_host import ext_declared_symbols
    assert ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert "#define RTREC_FACTOR_GRAM_WORKSPACE_BYTES(n_v, dim)" in header and "FACTOR GRAM" in header and "FACTOR ALS SOLVE" in header
    for sym, op, src, n_args in (("rtrec_factor_gram", "factor_gram", "factor_gram.hip", 9),
                                 ("rtrec_factor_als_solve", "factor_als_solve", "factor_als.hip", 17)):
        assert sym in _native.EXT_EXPORTS and sym not in _native.EXPORTS and src in build.SOURCES
        assert op in ops.EXT_OPS and op not in ops.OPS and ops.EXT_EXPORT_OF[op] == sym
        assert hasattr(ctypes.CDLL(build.LIB_PATH), sym) and len(getattr(_native.load(), sym).argtypes) == n_args
        schema = str(getattr(torch.ops.rtrec_amd, op).default._schema)
        assert schema.startswith(f"rtrec_amd::{op}(") and schema.endswith("-> ()")
        for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):      # called through the op only, never by ctypes
            for f in files:
                if f.endswith(".py") and f != "_native.py":
                    assert f".{sym}(" not in open(os.path.join(dirpath, f)).read(), f
        assert callable(getattr(HipBackend, op))
    assert len(ops.OPS) == 22 and len(ops.EXT_OPS) == len(_native.EXT_EXPORTS)
    schema = str(torch.ops.rtrec_amd.factor_als_solve.default._schema)
    for name in ("out", "status"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    assert re.search(r"Tensor\([a-z]!\) gram\b", str(torch.ops.rtrec_amd.factor_gram.default._schema))
    for name in ("als_begin", "als_half_step", "als_install", "fit_factors"):
        assert callable(getattr(SlimEngine, name))
    if not torch.cuda.is_available():
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.factor_gram(torch.zeros(2, 4), 2, 4, 0.1, torch.zeros(4, 4), torch.zeros(64))


def test_the_entry_points_check_their_arguments_on_the_host():
    from rtrec_amd import _native
    gram, solve = _native.load().rtrec_factor_gram, _native.load().rtrec_factor_als_solve
    one = 1                                                              # any non-NULL address: never dereferenced on these paths

    def g(n_v=2000, v=one, vs=8, dim=8, reg=0.1, out=one, ws=one, ws_bytes=2 * 8 * 8 * 4):
        return (n_v, v, vs, dim, reg, out, ws, ws_bytes, None)

    for kw in (dict(dim=0), dict(dim=65, vs=65)):
        assert gram(*g(**kw)) == -2, kw
    for kw in (dict(n_v=-1), dict(vs=7), dict(reg=-0.5), dict(reg=float("nan")), dict(out=None), dict(v=None), dict(ws=None)):
        assert gram(*g(**kw)) == -1, kw
    assert gram(*g(ws_bytes=2 * 8 * 8 * 4 - 1)) == -3 and gram(*g(n_v=2049)) == -3      # RTREC_FACTOR_GRAM_WORKSPACE_BYTES(2049, 8)

    def s(n_jobs=3, jobs=one, n_rows=5, ptr=one, idx=one, val=one, nnz=9, v=one, vs=8, n_v=7, dim=8, gram_=one, alpha=1.0, out=one,
          os_=8, status=one):
        return (n_jobs, jobs, n_rows, ptr, idx, val, nnz, v, vs, n_v, dim, gram_, alpha, out, os_, status, None)

    for kw in (dict(dim=0), dict(dim=65, vs=65, os_=65)):
        assert solve(*s(**kw)) == -2, kw
    for kw in (dict(n_jobs=-1), dict(n_rows=-1), dict(n_v=-1), dict(nnz=-1), dict(vs=7), dict(os_=7), dict(alpha=-1.0), dict(alpha=float("nan")),
               dict(ptr=None), dict(idx=None), dict(val=None), dict(v=None), dict(gram_=None), dict(out=None), dict(status=None)):
        assert solve(*s(**kw)) == -1, kw
    assert solve(*s(n_jobs=0)) == 0 and solve(*s(n_jobs=0, ptr=None, v=None, gram_=None, out=None, status=None)) == 0
    assert solve(*s(n_jobs=0, dim=64, vs=64, os_=64)) == 0               # the limit itself is served
