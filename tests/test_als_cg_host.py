"""Training the factor scorer by conjugate gradient (SLIM.fit_factors(solver="cg"), csrc/factor_als_cg.hip, and the wide Gram
call of csrc/factor_gram.hip) without a GPU: the definition of rtrec_factor_als_cg as a plain-Python host model, one libm fmaf at a
time and `tree` level by level, and a vectorised one over the jobs; that each pinned operation is visible in the bits; that
the start residual is the Cholesky contract's rhs; descent of the quadratic and sense on block-structured data, with the
Cholesky solver as the yardstick; the model / facade / serving layers through the CPU stand-in backend; the rules of the extension
surface and the C entry points' host-side checks.  The kernels are in tests/test_gpu_als_cg.py.

The definition (include/rtrec_amd_ext.h, "FACTOR ALS CG"): with A = G + sum w y y^T and b = sum (1 + w) y over the usable entries
of the row in storage order, chain = the fmaf chain over ascending components, tree = rounded products, then q[c] += q[c + h] for
h = D/2 .. 1, mat = G v by one fmaf chain per component: r = -mat(x), then fmaf(fl(fl(1 + w) - fl(w chain(y, x))), y, r) per entry;
p = r, rs = tree(r, r); per step Ap = mat(p), then fmaf(fl(w chain(y, p)), y, Ap) per entry, den = tree(p, Ap), al = fl(rs / den),
x = fmaf(al, p, x), r = fmaf(-al, Ap, r), rn = tree(r, r), be = fl(rn / rs), p = fmaf(be, p, r)."""
import ctypes
import io
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_factor_host import bits, fma32, fmaf
from tests.test_als_host import (BREAK_LENGTHS, F32, ROOT, TINY, _row_entries, als_backend, als_case, als_loss, als_model,
                                 block_data, counts_of, gram_fast, gram_plain, resident_x, solve_plain)

EPS = F32(1e-20)                                 # the stopping threshold of the contract, compared in float32
WIDE_MAX_DIM, MAX_STEPS = 256, 64


# ---------------------------------------------------------------------------------------------- the host models
def pow2_at_least(dim):
    D = 1
    while D < dim:
        D *= 2
    return D


def chain_plain(u, v, dim):
    s = F32(0.0)
    for c in range(dim):
        s = fmaf(u[c], v[c], s)
    return s


def tree_plain(u, v, dim):
    D = pow2_at_least(dim)
    q = [F32(F32(u[c]) * F32(v[c])) for c in range(dim)] + [F32(0.0)] * (D - dim)
    h = D // 2
    while h >= 1:
        for c in range(h):
            q[c] = F32(q[c] + q[c + h])
        h //= 2
    return q[0]


def mat_plain(G, v, dim):
    out = []
    for a in range(dim):
        s = F32(0.0)
        for b in range(dim):
            s = fmaf(G[a, b], v[b], s)
        out.append(s)
    return out


def residual_plain(cols, ws, V, G, x, dim):
    """The start residual of the contract for one row: r = -mat(x), then one fused update per usable entry."""
    r = [F32(-s) for s in mat_plain(G, x, dim)]
    for i, w in zip(cols, ws):
        y = V[i]
        t = chain_plain(y, x, dim)
        coef = F32(F32(F32(1.0) + w) - F32(w * t))
        for a in range(dim):
            r[a] = fmaf(coef, y[a], r[a])
    return r


def cg_plain(ptr, idx, val, V, G, alpha, out, job_rows=None, cg_steps=3, warm_start=True):
    """THE DEFINITION of rtrec_factor_als_cg, one fmaf at a time: writes the vectors into `out` [n_rows, >= dim] in place and
    returns (status[n_jobs] uint8, rs[n_jobs] float32)."""
    V, G = np.asarray(V, F32), np.asarray(G, F32)
    n_v, dim = V.shape
    n_rows = len(ptr) - 1
    jobs = np.arange(n_rows) if job_rows is None else np.asarray(job_rows, np.int64)
    status, rs_out = np.zeros(len(jobs), np.uint8), np.zeros(len(jobs), F32)
    zero = F32(0.0)
    for j, row in enumerate(jobs):
        if not 0 <= row < n_rows:
            status[j] = 1
            continue
        cols, ws = _row_entries(ptr, idx, val, row, n_v, alpha)
        if not len(cols):
            status[j] = 1
            out[row, :dim] = 0
            continue
        with np.errstate(all="ignore"):
            x = [F32(c) for c in out[row, :dim]] if warm_start else [zero] * dim
            if not np.isfinite(np.array(x, F32)).all():
                x = [zero] * dim
            r = residual_plain(cols, ws, V, G, x, dim)
            p = list(r)
            rs = last = tree_plain(r, r, dim)
            broken = False
            if not rs < EPS:
                for _ in range(cg_steps):
                    Ap = mat_plain(G, p, dim)
                    for i, w in zip(cols, ws):
                        y = V[i]
                        wt = F32(w * chain_plain(y, p, dim))
                        for a in range(dim):
                            Ap[a] = fmaf(wt, y[a], Ap[a])
                    den = tree_plain(p, Ap, dim)
                    if not den > 0 or not np.isfinite(den):
                        broken = True
                        break
                    al = F32(rs / den)
                    for a in range(dim):
                        x[a] = fmaf(al, p[a], x[a])
                        r[a] = fmaf(-al, Ap[a], r[a])
                    rn = last = tree_plain(r, r, dim)
                    if rn < EPS:
                        break
                    be = F32(rn / rs)
                    for a in range(dim):
                        p[a] = fmaf(be, p[a], r[a])
                    rs = rn
            broken = broken or not np.isfinite(np.array(x, F32)).all()
        status[j] = 2 if broken else 0
        out[row, :dim] = 0 if broken else np.array(x, F32)
        rs_out[j] = last
    return status, rs_out


VARIANTS = ("tree_as_chain", "chain_as_tree", "unfused", "reverse", "coef_other", "float64", "reciprocal")
GROUP_ELEMENTS = 1 << 21                         # jobs are taken in groups whose staged rows of V hold at most this many floats


def _tree_fast(u, v, dim):
    D = pow2_at_least(dim)
    q = np.zeros(u.shape[:-1] + (D,), F32)
    q[..., :dim] = u * v
    h = D // 2
    while h >= 1:
        q[..., :h] = q[..., :h] + q[..., h:2 * h]
        h //= 2
    return q[..., 0].copy()


def _chain_fast(u, v, dim):
    s = np.zeros(np.broadcast(u[..., 0], v[..., 0]).shape, F32)
    for c in range(dim):
        s = fma32(u[..., c], v[..., c], s)
    return s


def _cg_group(cols, ws, lens, x, V, G, dim, cg_steps, variant):
    """One group of jobs (sorted by length, longest first): cols / ws [J, L] padded, x [J, dim] the start.  Returns (x, rs, broken)."""
    flush = variant == "flush"

    def z(a):
        return np.where(np.abs(a) < TINY, F32(0.0), a).astype(F32) if flush else a

    J, L = cols.shape
    Y, Gz = z(V[cols]), z(G)                              # [J, L, dim]; a padded slot holds row 0 and is never applied
    tree = (lambda u, v: _chain_fast(u, v, dim)) if variant == "tree_as_chain" else (lambda u, v: z(_tree_fast(z(u), z(v), dim)))

    def entry_dots(vec):                                 # t [J, L] = chain(y, vec) per entry
        if variant == "chain_as_tree":
            return _tree_fast(Y, np.broadcast_to(vec[:, None, :], Y.shape), dim)
        t = np.zeros((J, L), F32)
        for c in range(dim):
            t = z(fma32(Y[:, :, c], vec[:, c][:, None], t))
        return t

    def mat(vec):
        s = np.zeros((J, dim), F32)
        for b in range(dim):
            s = z(fma32(Gz[:, b][None, :], vec[:, b][:, None], s))
        return s

    def apply(acc, coef):                                # the entries in storage order, the jobs that still have one a prefix
        if variant == "float64":
            acc = acc.astype(np.float64)
        for t in range(L):
            n = int((lens > t).sum())
            c, y = coef[:n, t][:, None], Y[:n, t]
            if variant == "float64":
                acc[:n] += c.astype(np.float64) * y.astype(np.float64)
            elif variant == "unfused":
                acc[:n] = acc[:n] + c * y
            else:
                acc[:n] = z(fma32(c, y, acc[:n]))
        return acc.astype(F32)

    def axpy(a, u, v):
        return v + a[:, None] * u if variant == "unfused" else z(fma32(a[:, None], u, v))

    one = F32(1.0)
    t = entry_dots(x)
    coef = one + ws * (one - t) if variant == "coef_other" else z((one + ws) - z(ws * t))
    r = apply(-mat(x), coef)
    p = r.copy()
    rs = tree(r, r)
    last = rs.copy()
    active = ~(rs < EPS)
    broken = np.zeros(J, bool)
    for _ in range(cg_steps):
        if not active.any():
            break
        Ap = apply(mat(p), z(ws * entry_dots(p)))
        den = tree(p, Ap)
        fails = active & ~((den > 0) & np.isfinite(den))
        broken |= fails
        active &= ~fails
        al = z(rs * (one / den) if variant == "reciprocal" else rs / den)
        keep = active[:, None]
        x = np.where(keep, axpy(al, p, x), x)
        r = np.where(keep, axpy(-al, Ap, r) if variant != "unfused" else z(fma32(-al[:, None], Ap, r)), r)
        rn = tree(r, r)
        last = np.where(active, rn, last)
        active &= ~(rn < EPS)
        be = z(rn / rs)
        p = np.where(active[:, None], z(fma32(be[:, None], p, r)), p)
        rs = np.where(active, rn, rs)
    return x, last, broken | ~np.isfinite(x).all(axis=1)


def cg_fast(ptr, idx, val, V, G, alpha, out, job_rows=None, cg_steps=3, warm_start=True, variant=None):
    """cg_plain, vectorised over the jobs (sorted by length, in groups): every fused step through fma32, the products, sums and
    quotients of `tree`, al and be on float32.  `variant` swaps ONE pinned operation for what another implementation might do
    (test_each_pinned_operation_shows_in_the_bits): "tree_as_chain" reduces rs, den and rn by the fmaf chain; "chain_as_tree"
    takes every entry's t by the tree; "unfused" rounds product and sum of the updates of r / Ap (per entry) and x separately;
    "reverse" takes the entries last first; "coef_other" is fl(1 + fl(w * fl(1 - t))); "float64" accumulates the entries' terms
    of r and Ap in float64 and rounds once; "reciprocal" is al = fl(rs * fl(1 / den)).  "flush" (not one of VARIANTS) is a
    kernel in flush-to-zero mode: denormal operands and results become zero and an entry whose w flushes is not usable."""
    assert variant is None or variant in VARIANTS or variant == "flush"
    V, G = np.asarray(V, F32), np.asarray(G, F32)
    n_v, dim = V.shape
    n_rows = len(ptr) - 1
    jobs = np.arange(n_rows) if job_rows is None else np.asarray(job_rows, np.int64)
    status, rs_out = np.zeros(len(jobs), np.uint8), np.zeros(len(jobs), F32)
    entries = {}
    for j, row in enumerate(jobs):
        if not 0 <= row < n_rows:
            status[j] = 1
            continue
        cols, ws = _row_entries(ptr, idx, val, row, n_v, alpha)
        if variant == "flush":
            cols, ws = cols[ws >= TINY], ws[ws >= TINY]
        if not len(cols):
            status[j] = 1
            out[row, :dim] = 0
            continue
        entries[j] = (cols[::-1], ws[::-1]) if variant == "reverse" else (cols, ws)
    live = sorted(entries, key=lambda j: -len(entries[j][0]))
    at = 0
    with np.errstate(all="ignore"):
        while at < len(live):
            L = len(entries[live[at]][0])
            J = max(1, min(len(live) - at, GROUP_ELEMENTS // (L * dim)))
            grp = live[at:at + J]
            at += J
            lens = np.array([len(entries[j][0]) for j in grp])
            cols, ws = np.zeros((J, L), np.int64), np.zeros((J, L), F32)
            for a, j in enumerate(grp):
                cols[a, :lens[a]], ws[a, :lens[a]] = entries[j]
            rows = jobs[grp]
            x = np.array(out[rows, :dim], F32) if warm_start else np.zeros((J, dim), F32)
            x[~np.isfinite(x).all(axis=1)] = 0
            x, rs, bad = _cg_group(cols, ws, lens, x, V, G, dim, cg_steps, variant)
            out[rows, :dim] = np.where(bad[:, None], F32(0.0), x)
            status[grp] = np.where(bad, 2, 0)
            rs_out[grp] = rs
    return status, rs_out


def cg_half_step(R, V, reg, alpha, out, job_rows=None, cg_steps=3, warm_start=True):
    """One half-step by the host model: the Gram of V, then cg_fast of R's rows (a scipy CSR, float32 values) into `out`."""
    return cg_fast(R.indptr, R.indices, R.data, V, gram_fast(V, reg), alpha, out, job_rows, cg_steps, warm_start)[0]


def host_fit_cg(X, dim, iterations, reg, alpha, seed, cg_steps=3, trace=None):
    """SlimEngine.fit_factors(solver="cg") by the host model: (P, Q, user status, item status).  P starts as zeros, every
    half-step is warm-started from what the matrix holds."""
    X = sp.csr_matrix(X, dtype=F32)
    X.sort_indices()
    Xt = sp.csr_matrix(X.T.tocsr(), dtype=F32)
    Xt.sort_indices()
    n_users, n_items = X.shape
    Q = np.random.default_rng(seed).standard_normal((n_items, dim)).astype(F32) * F32(0.01)
    P = np.zeros((n_users, dim), F32)
    su, si = np.ones(n_users, np.uint8), np.ones(n_items, np.uint8)
    for _ in range(iterations):
        su = cg_half_step(X, Q, reg, alpha, P, cg_steps=cg_steps)
        if trace:
            trace(P, Q)
        si = cg_half_step(Xt, P, reg, alpha, Q, cg_steps=cg_steps)
        if trace:
            trace(P, Q)
    return P, Q, su, si


def run(case, alpha, cg_steps=3, warm=None, jobs=None, variant=None, plain=False):
    """(status, rs, out) of the host model on (ptr, idx, val, V, G); `warm` [n_rows, dim] is the start (None: cold, `out`
    starts as 7.0)."""
    ptr, idx, val, V, G = case[:5]
    out = np.full((len(ptr) - 1, V.shape[1]), 7.0, F32) if warm is None else np.array(warm, F32)
    if plain:
        st, rs = cg_plain(ptr, idx, val, V, G, alpha, out, jobs, cg_steps, warm is not None)
    else:
        st, rs = cg_fast(ptr, idx, val, V, G, alpha, out, jobs, cg_steps, warm is not None, variant=variant)
    return st, rs, out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))


# ---------------------------------------------------------------------------------------------- inputs
def cg_case(dim, n_rows=27, n_v=400, lengths=(0, 1, 2, 3, 63, 64, 65, 129, 300), seed=None, scale=0.3, reg=0.1):
    """als_case's rows (skipped entries of every kind among the usable ones, a NaN row of V behind skipped entries) with the
    entry counts that cross one, two and four 64-entry blocks, and the honest Gram matrix.  Returns (ptr, idx, val, V, G)."""
    ptr, idx, val, V = als_case(n_rows, n_v, dim, seed=dim if seed is None else seed, lengths=lengths, scale=scale)
    return ptr, idx, val, V, gram_fast(np.nan_to_num(V), reg)


def warm_vectors(n_rows, dim, seed, nan_rows=()):
    """Finite start vectors, with one NaN component in each of `nan_rows` (the contract then starts those from zero)."""
    W = (np.random.default_rng(seed).standard_normal((n_rows, dim)) * 0.1).astype(F32)
    for k, r in enumerate(nan_rows):
        W[r, (3 * k + dim // 2) % dim] = np.nan
    return W


def early_stop_case():
    """dim 2: rows whose system CG solves within one, two or three steps, so that rn < 1e-20f stops the job before `cg_steps`
    run out: V is 1e-3 times the unit vectors, (1, 1) and (0.5, -1), G = 1e-6 I, so that the start residual is about 1e-6 squared
    and its 2^-24-sized remainder falls below the threshold.  Returns (ptr, idx, val, V, G)."""
    V = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, -1.0]], F32) * F32(1e-3)
    ptr, idx, val = [0], [], []
    for row in ([0], [1], [0, 1], [2], [2, 3], [0, 1, 2, 3], []):
        idx += row
        val += [1.0 + 0.5 * k for k in range(len(row))]
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.int32), np.array(val, F32), V, np.eye(2, dtype=F32) * F32(1e-6)


STATUS_ALPHA = 0.7


def status_case(dim, kind):
    """cg_case's rows with G doctored SYMMETRICALLY (the contract wants a symmetric matrix), to be run with STATUS_ALPHA:
    "neg1"  G = -dim / 10 I: den <= 0 at step 1 for the short rows (a long row's own entries outweigh it);
    "neg2"  the last diagonal element -dim / 2: den > 0 at step 1 for every row, <= 0 at step 2 for some;
    "nan"   a NaN at G[c][c // 2] and its mirror;  "inf"  +inf at G[c][c], c = dim - 1.
    Returns (ptr, idx, val, V, G)."""
    ptr, idx, val, V, G = cg_case(dim, n_rows=48, n_v=200, lengths=BREAK_LENGTHS)
    G = G.copy()
    c = dim - 1
    if kind == "neg1":
        G = (-0.1 * dim * np.eye(dim)).astype(F32)
    elif kind == "neg2":
        G[c, c] = -0.5 * dim
    elif kind == "nan":
        G[c, c // 2] = G[c // 2, c] = np.nan
    else:
        assert kind == "inf"
        G[c, c] = np.inf
    return ptr, idx, val, V, G


def tiny_case(dim, g=1e-38, alpha=1e-39):
    """Denormal w and products, and components that overflow (als_tiny_case's recipe): every usable value 1, G = g I, and an
    alpha so small that w = fl(alpha * 1) and fl(w * t) are float32 denormals.  den is about 1e-38 |p|^2, so al = fl(rs / den) is
    about 1e38 and fmaf(al, p, x) overflows in the rows where it is larger: status 2 by the finite check, not by den.
    Returns (ptr, idx, val, V, G, alpha)."""
    ptr, idx, val, V = als_case(48, 200, dim, seed=3, lengths=BREAK_LENGTHS)
    with np.errstate(invalid="ignore"):
        val = np.where(val > 0, F32(1.0), val).astype(F32)
    return ptr, idx, val, V, np.eye(dim, dtype=F32) * F32(g), alpha


def small_residual_case(dim):
    """cg_case's rows on vectors of about 1e-12: the start residual b has a squared norm below 1e-20f, so every job with a usable
    entry is done before the first step (status 0, x as it was), from zero and from a start of about 1e-12."""
    ptr, idx, val, V, _ = cg_case(dim, n_rows=18, n_v=200)
    with np.errstate(invalid="ignore"):
        V = (V * F32(1e-13)).astype(F32)
    return ptr, idx, val, V, np.eye(dim, dtype=F32) * F32(0.1)


STRIDE_GRID = 1 << 14                 # the workgroups of the largest launch (csrc/factor_als_cg.hip, kCgMaxGrid): job b + 2^14 is
STRIDE_SECOND = 300                   # the SECOND job of workgroup b; this many jobs have one
STRIDE_TEMPLATES = 509                # pattern rows (a prime: no template meets a fixed residue of the workgroup index)
STRIDE_LENGTHS = (0, 1, 2, 3, 5, 65)
OUTSIDE = 3                           # the class of a job whose row lies outside R; the other classes are the status
# (class of workgroup b's first job, class of its second one), in turn over b
STRIDE_PAIRS = ((0, 0), (2, 0), (1, 0), (OUTSIDE, 0), (0, 2), (2, 2), (1, 2), (OUTSIDE, 2), (0, 1), (2, 1), (1, 1), (OUTSIDE, 1),
                (0, OUTSIDE), (2, OUTSIDE))
STRIDE_STEPS = 2


def cg_stride_case(dim):
    """2^14 + 300 jobs over DISTINCT rows, more than one launch has workgroups for, so that 300 workgroups run a second job.
    R has 2^14 + 400 rows and row x is template x % 509: the rows of status_case(dim, "neg1") with STRIDE_LENGTHS, whose
    negative G leaves finished, empty and broken templates.  A job's result depends on its row alone, so the host model runs
    the templates once (STRIDE_STEPS steps from zero, STATUS_ALPHA).  The job list puts the pairs of STRIDE_PAIRS on workgroups
    0 .. 299 (job b, then job b + 2^14), fills the other slots with the remaining rows in a shuffled order and leaves about 100
    rows unnamed.  Returns (ptr, idx, val, V, G, jobs, template status, template rs, template vectors)."""
    tp, ti, tv, V, _ = cg_case(dim, n_rows=STRIDE_TEMPLATES, n_v=200, lengths=STRIDE_LENGTHS)
    G = (-0.1 * dim * np.eye(dim)).astype(F32)
    t_st, t_rs, t_out = run((tp, ti, tv, V, G), STATUS_ALPHA, STRIDE_STEPS)
    T = STRIDE_TEMPLATES
    n_jobs = STRIDE_GRID + STRIDE_SECOND
    n_rows = n_jobs + 100
    reps = -(-n_rows // T)
    ptr = np.r_[0, np.cumsum(np.tile(np.diff(tp), reps)[:n_rows])]
    idx, val = np.tile(ti, reps)[:ptr[-1]], np.tile(tv, reps)[:ptr[-1]]
    order = np.random.default_rng(dim).permutation(n_rows)
    pools = [iter(order[t_st[order % T] == k].tolist()) for k in range(3)]
    outside = iter([-1, n_rows] * STRIDE_SECOND)
    jobs = np.full(n_jobs, -7, np.int64)
    for b in range(STRIDE_SECOND):
        first, second = STRIDE_PAIRS[b % len(STRIDE_PAIRS)]
        jobs[b] = next(outside) if first == OUTSIDE else next(pools[first])
        jobs[b + STRIDE_GRID] = next(outside) if second == OUTSIDE else next(pools[second])
    taken = np.zeros(n_rows, bool)
    taken[jobs[(jobs >= 0) & (jobs < n_rows)]] = True
    rest = order[~taken[order]]
    jobs[jobs == -7] = rest[:(jobs == -7).sum()]
    return ptr.astype(np.int32), idx, val, V, G, jobs.astype(np.int32), t_st, t_rs, t_out


def stride_classes(jobs, n_rows, t_st):
    """The class per job of cg_stride_case: its status by the templates, or OUTSIDE."""
    jobs = np.asarray(jobs, np.int64)
    inside = (jobs >= 0) & (jobs < n_rows)
    return np.where(inside, t_st[np.where(inside, jobs, 0) % STRIDE_TEMPLATES], OUTSIDE)


# ---------------------------------------------------------------------------------------------- the two models agree
@pytest.mark.parametrize("dim", [1, 2, 3, 5, 12])
def test_both_models_agree_bit_for_bit(dim):
    case = cg_case(dim, n_rows=18, n_v=80, lengths=(0, 1, 2, 3, 9, 70))
    jobs = np.r_[np.random.default_rng(dim).permutation(18), -1, 18]
    warm = warm_vectors(18, dim, dim, nan_rows=(3, 4))
    for steps in (1, 3):
        for w in (None, warm):
            a, b = run(case, 0.7, steps, w, jobs, plain=True), run(case, 0.7, steps, w, jobs)
            assert same(a, b), (dim, steps, w is None)
            st, rs, out = b
            assert st[-1] == 1 and st[-2] == 1 and rs[-1] == 0 and rs[-2] == 0
            lengths = np.array([(0, 1, 2, 3, 9, 70)[x % 6] for x in jobs[:-2]])
            assert (st[:-2][lengths == 0] == 1).all() and (out[jobs[:-2][lengths == 0]] == 0).all()
            assert (st[:-2][lengths > 0] == 0).all() and np.isfinite(out).all()
    # a start with a NaN component is the cold start of that row
    cold = run(case, 0.7, 3, None, [3, 4])
    got = run(case, 0.7, 3, warm, [3, 4])
    assert np.array_equal(bits(cold[2][[3, 4]]), bits(got[2][[3, 4]])) and np.array_equal(bits(cold[1]), bits(got[1]))
    # and a finite start is not
    other = run(case, 0.7, 3, warm, [5, 11])
    assert not np.array_equal(bits(run(case, 0.7, 3, None, [5, 11])[2][[5, 11]]), bits(other[2][[5, 11]]))


def test_models_agree_on_the_status_cases():
    for kind in ("neg1", "neg2", "nan", "inf"):
        case = status_case(5, kind)
        assert same(run(case, STATUS_ALPHA, 3, plain=True), run(case, STATUS_ALPHA, 3)), kind
    *case, alpha = tiny_case(5)
    assert same(run(case, alpha, 3, plain=True), run(case, alpha, 3))
    case = early_stop_case()
    for steps in (1, 3, 64):
        assert same(run(case, 1.0, steps, plain=True), run(case, 1.0, steps)), steps
    case = small_residual_case(5)
    assert same(run(case, 1.0, 3, plain=True), run(case, 1.0, 3))


def test_the_status_cases_hold_what_they_claim():
    """From the host model alone: solved and broken jobs side by side for a G that is negative (den <= 0 at step 1), for one
    that breaks at step 2 only, every non-empty row broken by a NaN or +inf in G, overflowing components, a start residual
    below the threshold, and the denormal case on which a flushing kernel shows."""
    for dim in (5, 40, 70):
        # den <= 0 at step 1: with one step only, exactly the same rows break
        case = status_case(dim, "neg1")
        st1, st3 = run(case, STATUS_ALPHA, 1)[0], run(case, STATUS_ALPHA, 3)[0]
        assert counts_of(st1)[1] == 6 and counts_of(st1)[2] >= 8 and counts_of(st1)[0] >= 8, (dim, counts_of(st1))
        assert (st3[st1 == 2] == 2).all() and counts_of(st3)[2] >= counts_of(st1)[2]
        # ... at step 2: rows that one step finishes break with two
        case = status_case(dim, "neg2")
        st1, st2 = run(case, STATUS_ALPHA, 1)[0], run(case, STATUS_ALPHA, 2)[0]
        assert counts_of(st1) == [42, 6, 0] and ((st1 == 0) & (st2 == 2)).sum() >= 3 and (st2 == 0).sum() >= 10, (dim, counts_of(st2))
        for kind in ("nan", "inf"):
            st, rs, out = run(status_case(dim, kind), STATUS_ALPHA, 3)
            assert counts_of(st) == [0, 6, 42] and (out == 0).all(), (dim, kind, counts_of(st))
    for dim in (5, 70):
        case = small_residual_case(dim)
        warm = warm_vectors(18, dim, 1) * F32(1e-11)          # (A x is then as small as b)
        st, rs, out = run(case, 1.0, 3, warm)
        solved = st == 0
        assert solved.sum() == 16 and (rs[solved] < EPS).all() and (rs[solved] > 0).all()
        assert np.array_equal(bits(out[solved]), bits(warm[solved])) and (out[~solved] == 0).all()
    for dim in (5, 40):
        *case, alpha = tiny_case(dim)
        assert 0 < F32(alpha) * F32(1.0) < TINY
        base, flushed = run(case, alpha, 3), run(case, alpha, 3, variant="flush")
        changed = (base[0] != flushed[0]) | (bits(base[2]) != bits(flushed[2])).any(axis=1)
        assert counts_of(base[0])[0] >= 20 and counts_of(base[0])[2] >= 5 and changed.sum() == 42, (dim, counts_of(base[0]))
        assert np.abs(base[2]).max() > 1e38 and counts_of(flushed[0]) == [0, 48, 0]      # (a flushed w leaves no usable entry)
        # the broken rows overflow: one step fewer leaves them finished, with components beyond 1e37
        fewer = run(case, alpha, 1)
        assert (fewer[0][base[0] == 2] == 0).any() or (run(case, alpha, 2)[0][base[0] == 2] == 0).any()
    # ordinary inputs do not show a flush
    case = cg_case(5, n_rows=18, n_v=80)
    assert same(run(case, 0.7), run(case, 0.7, variant="flush"))


def test_early_stop_case_stops_on_the_threshold():
    """The dim-2 case: with 64 steps allowed every row stops on rn < 1e-20f after at most three, so 3 and 64 steps give the
    same bits; rows stop after the first, the second and the third step (measured: rows 0, 1 / 2, 3, 4 / 5)."""
    case = early_stop_case()
    one, two, three, many = (run(case, 1.0, k) for k in (1, 2, 3, 64))
    assert counts_of(many[0]) == [6, 1, 0] and (many[1][:6] < EPS).all()
    assert same(three, many) and not same(one, two) and not same(two, three)
    assert ((one[1][:6] < EPS).sum(), (two[1][:6] < EPS).sum()) == (2, 5)


# ---------------------------------------------------------------------------------------------- every pinned operation shows
def test_each_pinned_operation_shows_in_the_bits():
    """One seeded case (200 rows of 1 .. 90 entries, dim 12, all finished, cg_steps 3 from zero): the number of the 2,400
    output components whose bits change when ONE operation of the definition is swapped for what another implementation
    might do (cg_fast's variants), from zero and from finite start vectors.  Measured with this host model, cold / warm: tree
    replaced by chain 1054 / 1408, chain replaced by tree for t 748 / 1119, unfused updates of r, Ap and x 1432 / 1976, entries in
    reverse order 1510 / 1612, coef as 1 + w (1 - t) 0 / 1060 (from zero t is 0 and both forms are fl(1 + w): the warm start is
    the case for it), float64 accumulator 1553 / 1770, al by a reciprocal 567 / 730.  A kernel that
    took any of these liberties could not equal the host model in tests/test_gpu_als_cg.py."""
    ptr, idx, val, V = als_case(200, 300, 12, seed=12, lengths=(1, 2, 3, 7, 20, 40, 90), scale=0.5)
    case = (ptr, idx, val, V, gram_fast(np.nan_to_num(V), 0.01))
    warm = warm_vectors(200, 12, 12)
    counts = {}
    for name, w in (("cold", None), ("warm", warm)):
        base = run(case, 1.0, 3, w)
        assert (base[0] == 0).all()
        for variant in VARIANTS:
            got = run(case, 1.0, 3, w, variant=variant)
            counts[name, variant] = int((bits(got[2]) != bits(base[2])).sum())
    print(counts)
    assert all(counts["warm", v] > 0 for v in VARIANTS), counts
    assert all(counts["cold", v] > 0 for v in VARIANTS if v != "coef_other"), counts


# ---------------------------------------------------------------------------------------------- residual, objective
@pytest.mark.parametrize("dim", [1, 5, 12])
def test_from_zero_the_residual_is_the_cholesky_contracts_rhs(dim):
    """r from x = 0 against the rhs of solve_plain's definition, fmaf(fl(1 + w), y[a], rhs[a]) over the usable entries: mat(0) is
    zero, chain(y, 0) is zero and fl(fl(1 + w) - fl(w * 0)) is fl(1 + w)."""
    ptr, idx, val, V, G = cg_case(dim, n_rows=18, n_v=80, lengths=(1, 2, 3, 9, 70))
    for row in range(18):
        cols, ws = _row_entries(ptr, idx, val, row, 80, 0.7)
        rhs = [F32(0.0)] * dim
        for i, w in zip(cols, ws):
            c = F32(F32(1.0) + w)
            for a in range(dim):
                rhs[a] = fmaf(c, V[i][a], rhs[a])
        r = residual_plain(cols, ws, V, G, [F32(0.0)] * dim, dim)
        assert np.array_equal(bits(np.array(r, F32)), bits(np.array(rhs, F32))), row
    # and solve_plain's solution of the same rows has a residual that is small against rhs (the two contracts share the system)
    out = np.zeros((18, dim), F32)
    assert (solve_plain(ptr, idx, val, V, G, 0.7, out) == 0).all()
    for row in range(18):
        cols, ws = _row_entries(ptr, idx, val, row, 80, 0.7)
        r0 = np.array(residual_plain(cols, ws, V, G, [F32(0.0)] * dim, dim), np.float64)
        r1 = np.array(residual_plain(cols, ws, V, G, list(out[row]), dim), np.float64)
        assert np.linalg.norm(r1) <= 1e-4 * np.linalg.norm(r0), row


@pytest.mark.parametrize("dim", [8, 32, 96])
def test_three_steps_lower_the_quadratic_and_stay_above_its_minimum(dim):
    """f(x) = x^T A x / 2 - b^T x in float64 from the same float32 inputs, for every finished job of als_case's rows: lower after
    cg_steps = 3 than at the start (cold: f = 0; warm: f of the start vector), and not below f at np.linalg.solve's solution --
    beyond 1e-6 |f_min|, the rounding of a float32 x in a float64 evaluation."""
    ptr, idx, val, V = als_case(60, 500, dim, seed=0, lengths=(1, 3, 10, 40, 150), scale=0.3)
    V = np.nan_to_num(V)
    G = gram_fast(V, 0.01)
    V64 = V.astype(np.float64)
    G64 = G.astype(np.float64)
    warm = warm_vectors(60, dim, 5)
    for start in (None, warm):
        st, rs, out = run((ptr, idx, val, V, G), 1.0, 3, start)
        assert (st == 0).sum() == 60
        for row in range(60):
            cols, ws = _row_entries(ptr, idx, val, row, len(V), 1.0)
            Y, w = V64[cols], ws.astype(np.float64)
            A = G64 + (Y * w[:, None]).T @ Y
            b = ((1.0 + w)[:, None] * Y).sum(axis=0)
            f = lambda x: 0.5 * x @ A @ x - b @ x
            x0 = np.zeros(dim) if start is None else start[row].astype(np.float64)
            f_min = f(np.linalg.solve(A, b))
            f_x = f(out[row].astype(np.float64))
            assert f_x < f(x0), (dim, row)
            assert f_x >= f_min - 1e-6 * abs(f_min), (dim, row, f_x, f_min)


# ---------------------------------------------------------------------------------------------- the stand-in backend
def _csr_of(t3):
    return [t.numpy() for t in t3]


def als_cg_backend():
    class AlsCgOracleBackend(type(als_backend())):
        """The CPU stand-in with factor_gram_wide / factor_als_cg from the host model (TEST-ONLY, like its bases)."""

        def factor_gram_wide(self, v, n_v, dim, reg, gram):
            import torch
            gram.copy_(torch.from_numpy(gram_fast(v.numpy()[:n_v, :dim], reg)))

        def factor_als_cg(self, job_rows, n_jobs, r_csr, v, n_v, dim, gram, alpha, cg_steps, warm_start, out, status, rs=None):
            import torch
            ptr, idx, val = _csr_of(r_csr)
            jobs = np.arange(n_jobs) if job_rows is None else job_rows.numpy()
            o = out.numpy()                                   # (shares the tensor's memory: written in place)
            st, r = cg_fast(ptr, idx, val, v.numpy()[:n_v, :dim], gram.numpy(), alpha, o, jobs, cg_steps, warm_start)
            status.copy_(torch.from_numpy(st))
            if rs is not None:
                rs.copy_(torch.from_numpy(r))

    return AlsCgOracleBackend()


def cg_model(extra=()):
    """als_model on the stand-in above."""
    from rtrec_amd.engine import SlimEngine
    m, batch = als_model(extra)
    m.model._engine = SlimEngine(backend=als_cg_backend())
    return m, batch


def test_gram_wide_model_and_stand_in():
    """The wide Gram call shares rtrec_factor_gram's definition: the plain model equals gram_fast at widths on both sides of
    every tile and wave edge (rows across the chunk edge at the narrow ones, where the plain model is quick), gram_fast is
    symmetric bit for bit at every dim in 1..256, and the stand-in's wide call equals its narrow one up to 64."""
    import torch
    rng = np.random.default_rng(0)
    for dim, n in ((1, 1030), (2, 1025), (33, 5), (65, 3), (97, 2), (129, 2), (256, 1)):
        V = rng.standard_normal((n, dim)).astype(F32)
        assert np.array_equal(bits(gram_plain(V, 0.05)), bits(gram_fast(V, 0.05))), dim
    V = rng.standard_normal((7, 256)).astype(F32)
    for dim in range(1, 257):
        G = gram_fast(V[:, :dim], 0.05)
        assert G.shape == (dim, dim) and np.array_equal(bits(G), bits(G.T)), dim
    be = als_cg_backend()
    for dim in (1, 32, 33, 64):
        v = torch.from_numpy(rng.standard_normal((1100, dim + 2)).astype(F32))
        a, b = torch.zeros(dim, dim), torch.zeros(dim, dim)
        be.factor_gram(v, 1090, dim, 0.1, a)
        be.factor_gram_wide(v, 1090, dim, 0.1, b)
        assert np.array_equal(bits(a.numpy()), bits(b.numpy())) and a.abs().sum() > 0


# ---------------------------------------------------------------------------------------------- training quality
CG_EXCESS_MEASURED = 1.2449e-05     # (loss_cg - loss_cholesky) / loss_cholesky of the test below, measured with the host models


def test_cg_training_keeps_the_lists_in_the_cluster_and_its_loss_near_choleskys():
    """4 clusters of 30 items, 50 users each rating 8 items of their own cluster, dim 8, 16 iterations, reg 0.01, alpha 1, seed 0
    by the host models (the stand-in stack runs them: test_fit_factors_cg_...): with solver="cg", cg_steps=3 every user's factor top-5 (interacted items
    filtered) lies inside its cluster, and the final float64 als_loss is measured against the Cholesky solver's on the same
    data.  Measured with the host models: Cholesky 2227.235454, CG 2227.263181, a relative excess of 1.2449e-05; the test
    allows twice that.  A swapped operation that still converges to another point cannot hide behind the bound."""
    from tests.test_factor_host import host_model_fast
    from tests.test_als_host import host_fit
    X = block_data(0)
    P, Q, su, si = host_fit_cg(X, 8, 16, 0.01, 1.0, 0, cg_steps=3)
    assert (su == 0).all() and (si == 0).all()
    ids, _, cnt = host_model_fast(P, Q, 5, X=X, filter_interacted=True)
    assert (cnt == 5).all() and (ids // 30 == (np.arange(200) // 50)[:, None]).all()
    Pc, Qc, _, _ = host_fit(X, 8, 16, 0.01, 1.0, 0)
    loss_cg, loss_ch = als_loss(X, P, Q, 0.01, 1.0), als_loss(X, Pc, Qc, 0.01, 1.0)
    excess = (loss_cg - loss_ch) / loss_ch
    print(f"cholesky {loss_ch:.6f} cg {loss_cg:.6f} relative excess {excess:.3e}")
    assert excess <= 2 * CG_EXCESS_MEASURED, (loss_ch, loss_cg, excess)


# ---------------------------------------------------------------------------------------------- model / facade, end to end
FIT = dict(dim=6, iterations=2, regularization=0.05, alpha=0.5, seed=3)


def test_fit_factors_cg_equals_attach_factors_of_the_host_models_vectors():
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.recommender import Recommender
    from tests.test_als_host import attach_host_vectors
    m, batch = cg_model()
    users = sorted({u for u, _, _, _ in batch})
    assert not m.has_factors() and m.fit_factors(**FIT, solver="cg", cg_steps=2) is m and m.has_factors()
    P, Q, su, si = host_fit_cg(resident_x(m), FIT["dim"], FIT["iterations"], FIT["regularization"], FIT["alpha"], FIT["seed"], cg_steps=2)
    assert (su == 0).sum() > 100 and (si == 0).sum() > 30
    ref, _ = cg_model()
    attach_host_vectors(ref, P, su, Q, si)
    for key in ("user_rows", "user_vectors", "item_rows", "item_vectors"):
        a, b = m._factors[key], ref._factors[key]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a) if a.dtype == F32 else a, bits(b) if b.dtype == F32 else b), key
    assert m._factor_training == {"regularization": 0.05, "alpha": 0.5, "solver": "cg", "cg_steps": 2}
    ask = users[:40] + [max(users) + 1000] + users[40:]
    assert m.recommend_factor_batch(ask, top_k=7) == ref.recommend_factor_batch(ask, top_k=7)
    for kw in (dict(top_k=8), dict(top_k=6, weighting=0.6)):
        assert m.recommend_hybrid_batch(ask, **kw) == ref.recommend_hybrid_batch(ask, **kw), kw
    # the default solver gives other vectors, and records no solver (a dict without one means Cholesky)
    ch, _ = cg_model()
    ch.fit_factors(**FIT)
    assert ch._factor_training == {"regularization": 0.05, "alpha": 0.5}
    assert not np.array_equal(bits(ch._factors["user_vectors"]), bits(m._factors["user_vectors"]))
    assert sorted(ch._serialize()) == sorted(ref._serialize())
    # a pickle carries the vectors AND the solver; the facade passes both keywords through
    buf = io.BytesIO()
    m.save(buf)
    back = type(m).loads(buf.getvalue())
    back.model._engine = SlimEngine(backend=als_cg_backend())
    assert back.has_factors() and back._factor_training == m._factor_training
    assert back.recommend_factor_batch(ask, top_k=7) == m.recommend_factor_batch(ask, top_k=7)
    back.update_factors(users[:3])
    m.update_factors(users[:3])
    assert np.array_equal(bits(back._factors["user_vectors"]), bits(m._factors["user_vectors"]))
    rec = Recommender(cg_model()[0])
    assert rec.fit_factors(**FIT, solver="cg", cg_steps=2) is rec
    assert rec.recommend_factor_batch(ask, top_k=7) == ref.recommend_factor_batch(ask, top_k=7)
    assert rec.update_factors(users[:3], solver="cg", cg_steps=1) is rec


def test_fit_factors_cg_trains_what_cholesky_cannot():
    """dim 96 through the stand-in stack: the wide Gram call and the CG call, the host model's P and Q bit for bit."""
    m, batch = cg_model()
    calls = []
    be = m.model.engine.be
    wide, narrow = be.factor_gram_wide, be.factor_gram
    be.factor_gram_wide = lambda *a: (calls.append("wide"), wide(*a))[1]
    be.factor_gram = lambda *a: (calls.append("narrow"), narrow(*a))[1]
    with pytest.raises(ValueError):
        m.fit_factors(dim=96, iterations=1)
    m.fit_factors(dim=96, iterations=1, solver="cg")
    assert calls == ["wide", "wide"]
    P, Q, su, si = host_fit_cg(resident_x(m), 96, 1, 0.01, 1.0, 0)
    assert np.array_equal(bits(m._factors["user_vectors"]), bits(P[su == 0])) and np.array_equal(bits(m._factors["item_vectors"]), bits(Q[si == 0]))
    m.fit_factors(dim=64, iterations=1, solver="cg", cg_steps=1)
    assert calls == ["wide", "wide", "narrow", "narrow"]


def test_update_factors_cg_resolves_an_attached_wide_model_and_touches_only_the_named_users():
    m, batch = cg_model()
    users = sorted({u for u, _, _, _ in batch})
    items = sorted({i for _, i, _, _ in batch})
    rng = np.random.default_rng(4)
    P0 = (rng.standard_normal((len(users), 96)) * 0.1).astype(F32)
    Q0 = (rng.standard_normal((len(items), 96)) * 0.1).astype(F32)
    m.attach_factors(users, P0, items, Q0)
    before = {k: v.copy() for k, v in m._factors.items()}
    with pytest.raises(ValueError, match="64"):                      # today's refusal stays: no recorded solver means Cholesky
        m.update_factors(users[:2])
    for kw in (dict(solver="lu"), dict(solver="cg", cg_steps=0), dict(solver="cg", cg_steps=65)):
        with pytest.raises(ValueError):
            m.update_factors(users[:2], **kw)
    named = [users[7], users[2], max(users) + 999]
    assert m.update_factors(named, solver="cg", cg_steps=2) is m
    X = resident_x(m)
    n_users = X.shape[0]
    P = np.zeros((n_users, 96), F32)
    P[before["user_rows"]] = before["user_vectors"]
    Q = np.zeros((X.shape[1], 96), F32)
    Q[before["item_rows"]] = before["item_vectors"]
    rows = sorted(m._known_user_id(u) for u in named[:2])
    st = cg_half_step(X, Q, 0.01, 1.0, P, job_rows=np.array(rows), cg_steps=2, warm_start=True)
    assert (st == 0).all()
    after = m._factors
    assert np.array_equal(after["item_rows"], before["item_rows"]) and np.array_equal(bits(after["item_vectors"]), bits(before["item_vectors"]))
    assert np.array_equal(after["user_rows"], before["user_rows"])
    for r, vec in zip(after["user_rows"], after["user_vectors"]):
        assert np.array_equal(bits(vec), bits(P[r])), r
    changed = [int(r) for r, a, b in zip(before["user_rows"], before["user_vectors"], after["user_vectors"]) if not np.array_equal(bits(a), bits(b))]
    assert changed == rows
    # warm-started: from zero the same two steps end elsewhere
    Pz = np.zeros((n_users, 96), F32)
    cg_half_step(X, Q, 0.01, 1.0, Pz, job_rows=np.array(rows), cg_steps=2, warm_start=False)
    assert not np.array_equal(bits(Pz[rows]), bits(P[rows]))


def test_refusals_and_defaults():
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.slim import SLIM
    from rtrec_amd.recommender import Recommender
    m, batch = cg_model()
    for kw in (dict(solver="lu"), dict(solver="cg", cg_steps=0), dict(solver="cg", cg_steps=65), dict(solver="cg", dim=257),
               dict(solver="cg", dim=0), dict(dim=65), dict(dim=65, solver="cholesky"), dict(solver="cg", iterations=0)):
        with pytest.raises(ValueError):
            m.fit_factors(**kw)
    assert not m.has_factors()
    m.recommend_batch([batch[0][0]])
    m._sync_interactions_csc()
    eng = m.model.engine
    Q0 = np.zeros((eng.n_items, 70), F32)
    with pytest.raises(ValueError, match="1..64"):
        eng.als_begin(70, 0.01, 1.0, Q0)
    for kw in (dict(solver="lu"), dict(solver="cg", cg_steps=0), dict(solver="cg", cg_steps=65)):
        with pytest.raises(ValueError):
            eng.als_begin(70, 0.01, 1.0, Q0, **kw)
        with pytest.raises(ValueError):
            eng.fit_factors(dim=70, iterations=1, **kw)
    with pytest.raises(ValueError):
        eng.als_begin(257, 0.01, 1.0, np.zeros((eng.n_items, 257), F32), solver="cg")
    eng.als_begin(70, 0.01, 1.0, Q0, solver="cg", cg_steps=64)
    assert eng._als["solver"] == "cg" and eng._als["cg_steps"] == 64
    eng.als_begin(8, 0.01, 1.0, Q0[:, :8])
    assert eng._als["solver"] == "cholesky"
    eng.world_size = 2
    try:
        with pytest.raises(ValueError, match="rank"):
            eng.fit_factors(dim=4, iterations=1, solver="cg")
    finally:
        eng.world_size = 1
    assert SlimEngine.ALS_MAX_DIM == 64 and SLIM.FACTOR_TRAIN_MAX_DIM == 64
    for f in (SLIM.fit_factors, SlimEngine.fit_factors, Recommender.fit_factors):
        assert f.__defaults__ == (32, 15, 0.01, 1.0, 0) and f.__kwdefaults__ == {"solver": "cholesky", "cg_steps": 3}
    assert SlimEngine.als_begin.__kwdefaults__ == {"solver": "cholesky", "cg_steps": 3}
    assert SLIM.update_factors.__kwdefaults__ == {"solver": None, "cg_steps": None}


def test_fit_factors_route_takes_the_solver():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = cg_model()
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    assert client.post("/fit_factors", json={"dim": 65}, headers=ok).status_code == 500 and not m.has_factors()
    assert client.post("/fit_factors", json={"dim": 65, "solver": "lu"}, headers=ok).status_code == 500
    assert client.post("/fit_factors", json={"dim": 65, "solver": "cg", "cg_steps": 0}, headers=ok).status_code == 500
    r = client.post("/fit_factors", json={"dim": 65, "iterations": 1, "seed": 2, "solver": "cg", "cg_steps": 2}, headers=ok)
    assert r.status_code == 200 and r.json() == {"message": "Factor training successful"} and m.has_factors()
    want, _ = cg_model()
    want.fit_factors(dim=65, iterations=1, seed=2, solver="cg", cg_steps=2)
    user = batch[0][0]
    r = client.post("/recommend_hybrid", json={"user": user, "top_k": 5}, headers=ok)
    assert r.status_code == 200 and r.json()["items"] == want.recommend_hybrid(user, top_k=5)


# ---------------------------------------------------------------------------------------------- registration
def test_the_two_calls_are_declared_registered_and_exported():
    import re
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from tests.test_diverse_host import ext_declared_symbols
    assert ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert "FACTOR GRAM WIDE" in header and "FACTOR ALS CG" in header
    for sym, op, src, n_args in (("rtrec_factor_gram_wide", "factor_gram_wide", "factor_gram.hip", 9),
                                 ("rtrec_factor_als_cg", "factor_als_cg", "factor_als_cg.hip", 20)):
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
    assert len(ops.OPS) == 22 and len(ops.EXT_OPS) == len(_native.EXT_EXPORTS) == len(set(ops.EXT_EXPORT_OF.values()))
    schema = str(torch.ops.rtrec_amd.factor_als_cg.default._schema)
    for name in ("out", "status"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    assert re.search(r"Tensor\([a-z]!\)\? rs\b", schema) and "int cg_steps" in schema and "bool warm_start" in schema
    assert re.search(r"Tensor\([a-z]!\) gram\b", str(torch.ops.rtrec_amd.factor_gram_wide.default._schema))
    if not torch.cuda.is_available():
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.factor_gram_wide(torch.zeros(2, 96), 2, 96, 0.1, torch.zeros(96, 96), torch.zeros(96 * 96))


def test_the_entry_points_check_their_arguments_on_the_host():
    from rtrec_amd import _native
    gram, cg = _native.load().rtrec_factor_gram_wide, _native.load().rtrec_factor_als_cg
    one = 1                                                              # any non-NULL address: never dereferenced on these paths

    def g(n_v=2000, v=one, vs=8, dim=8, reg=0.1, out=one, ws=one, ws_bytes=2 * 8 * 8 * 4):
        return (n_v, v, vs, dim, reg, out, ws, ws_bytes, None)

    for kw in (dict(dim=0), dict(dim=257, vs=257), dict(dim=-1)):
        assert gram(*g(**kw)) == -2, kw
    for kw in (dict(n_v=-1), dict(vs=7), dict(reg=-0.5), dict(reg=float("nan")), dict(out=None), dict(v=None), dict(ws=None)):
        assert gram(*g(**kw)) == -1, kw
    assert gram(*g(ws_bytes=2 * 8 * 8 * 4 - 1)) == -3 and gram(*g(n_v=2049)) == -3      # RTREC_FACTOR_GRAM_WORKSPACE_BYTES(2049, 8)
    assert gram(*g(dim=256, vs=255)) == -1 and gram(*g(dim=256, vs=256, ws_bytes=2 * 256 * 256 * 4 - 1)) == -3   # 256 is served
    assert gram(*g(dim=65, vs=65, ws_bytes=0)) == -3                     # ... and so is 65, which rtrec_factor_gram refuses
    assert _native.load().rtrec_factor_gram(*g(dim=65, vs=65)) == -2

    def s(n_jobs=3, jobs=one, n_rows=5, ptr=one, idx=one, val=one, nnz=9, v=one, vs=8, n_v=7, dim=8, gram_=one, alpha=1.0, steps=3,
          warm=1, out=one, os_=8, status=one, rs=one):
        return (n_jobs, jobs, n_rows, ptr, idx, val, nnz, v, vs, n_v, dim, gram_, alpha, steps, warm, out, os_, status, rs, None)

    for kw in (dict(dim=0), dict(dim=257, vs=257, os_=257), dict(steps=0), dict(steps=65), dict(steps=-3), dict(n_jobs=0, steps=0),
               dict(n_jobs=0, dim=257, vs=257, os_=257)):
        assert cg(*s(**kw)) == -2, kw
    for kw in (dict(n_jobs=-1), dict(n_rows=-1), dict(n_v=-1), dict(nnz=-1), dict(vs=7), dict(os_=7), dict(alpha=-1.0), dict(alpha=float("nan")),
               dict(ptr=None), dict(idx=None), dict(val=None), dict(v=None), dict(gram_=None), dict(out=None), dict(status=None)):
        assert cg(*s(**kw)) == -1, kw
    assert cg(*s(n_jobs=0)) == 0 and cg(*s(n_jobs=0, ptr=None, v=None, gram_=None, out=None, status=None, rs=None)) == 0
    assert cg(*s(n_jobs=0, dim=256, vs=256, os_=256, steps=64)) == 0     # the limits themselves are served
    assert cg(*s(n_jobs=0, dim=256, vs=255, os_=256)) == -1 and cg(*s(n_jobs=0, dim=65, vs=65, os_=65, steps=1, warm=0)) == 0


@pytest.mark.parametrize("dim", [5, 70])
def test_stride_case_puts_every_pair_on_one_workgroup(dim):
    """cg_stride_case from the host model alone: the templates hold all three statuses, the rows named are distinct, every
    pair of STRIDE_PAIRS occurs as (job b, job b + 2^14), and running the tiled R itself for those 600 jobs gives what the
    templates expand to."""
    ptr, idx, val, V, G, jobs, t_st, t_rs, t_out = cg_stride_case(dim)
    n_rows, jobs = len(ptr) - 1, jobs.astype(np.int64)
    assert len(jobs) == STRIDE_GRID + STRIDE_SECOND and min(counts_of(t_st)) >= 50, counts_of(t_st)
    inside = jobs[(jobs >= 0) & (jobs < n_rows)]
    assert len(np.unique(inside)) == len(inside) and 0 < len(jobs) - len(inside) < 150 and n_rows - len(inside) >= 100
    cls = stride_classes(jobs, n_rows, t_st)
    second = np.arange(STRIDE_GRID, STRIDE_GRID + STRIDE_SECOND)
    assert set(zip(cls[second - STRIDE_GRID].tolist(), cls[second].tolist())) == set(STRIDE_PAIRS)
    sel = np.r_[second - STRIDE_GRID, second]
    st, rs, out = run((ptr, idx, val, V, G), STATUS_ALPHA, STRIDE_STEPS, jobs=jobs[sel])
    assert np.array_equal(st, np.where(cls[sel] == OUTSIDE, 1, cls[sel]))
    named = jobs[sel][cls[sel] != OUTSIDE]
    assert np.array_equal(bits(out[named]), bits(t_out[named % STRIDE_TEMPLATES])) and (np.delete(out, named, axis=0) == 7.0).all()
    assert np.array_equal(bits(rs[cls[sel] != OUTSIDE]), bits(t_rs[named % STRIDE_TEMPLATES])) and (rs[cls[sel] == OUTSIDE] == 0).all()
