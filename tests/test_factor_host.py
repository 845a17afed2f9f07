"""The factor scorer (SLIM.recommend_factor_batch / recommend_hybrid_batch, csrc/factor_topk.hip) without a GPU: the definition
as a plain-Python host model whose fmaf is libm's and a vectorised one whose fused step is exact by construction; the accuracy
bound of the chain; the model / facade / serving layers end to end through the CPU stand-in backend with `factor_topk` supplied
by the host model; the rules of the extension surface and the C entry point's host-side checks.  The kernel is in
tests/test_gpu_factor.py.

The definition (include/rtrec_amd_ext.h, "FACTOR TOP-K"): job r names row x of X; its vector is row p_index[x] of P; the score
of item i is s = +0, then s = fmaf(p[c], q[c], s) for ascending c; item i competes when the mask admits it, X's row does not
store it (with filter_interacted) and its score is not NaN; the larger score first, the lower id among == scores."""
import ctypes
import ctypes.util
import io
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.engine import SlimEngine
from tests.test_blend_host import BlendOracleBackend, _expected, value_bits
from tests.test_rerank_host import _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24                                   # the unit roundoff of float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]


def fmaf(a, b, c):
    """libm's correctly rounded float32 fused multiply-add."""
    return F32(_libm.fmaf(float(a), float(b), float(c)))


def fma32(a, b, c):
    """fmaf on float32 arrays, exact by construction: the product of two float32 is exact in float64 (48 bits); the float64 sum
    with c is rounded to odd (TwoSum gives the error, nextafter moves an even inexact result to its odd neighbour), and a value
    rounded to odd at 53 bits rounds to float32 as the exact value does (53 >= 2 * 24 + 2)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where((err > 0), np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F32)


def bits(a):
    """The bit patterns of float32 values after adding +0.0f (the sign of a zero is not part of the contract)."""
    return (np.asarray(a, F32) + F32(0.0)).view(np.int32)


# ---------------------------------------------------------------------------------------------- the host models
def _job_vectors(P, rows, p_index, n_x_rows):
    """(x per job, vector row per job or -1)."""
    P = np.asarray(P, F32)
    R = len(rows)
    x = np.asarray(rows, np.int64)
    vec = np.full(R, -1, np.int64)
    for r in range(R):
        if 0 <= x[r] < n_x_rows:
            v = int(p_index[x[r]]) if p_index is not None else int(x[r])
            if 0 <= v < len(P):
                vec[r] = v
    return x, vec


def host_model_plain(P, Q, top_k, rows=None, p_index=None, n_x_rows=None, X=None, mask=None, filter_interacted=False):
    """THE DEFINITION, one fmaf at a time: (ids[R, top_k] int32, scores[R, top_k] float32, count[R] int32).  P [n_p, dim], Q
    [n_items, dim]; `rows` the row of X per job (None: 0 .. len(P)-1), `p_index` the vector per row of X (None: row x), X a csr
    over the items, `mask` one entry per item."""
    P, Q = np.asarray(P, F32), np.asarray(Q, F32)
    rows = np.arange(len(P)) if rows is None else rows
    n_x_rows = (X.shape[0] if X is not None else len(P)) if n_x_rows is None else n_x_rows
    x, vec = _job_vectors(P, rows, p_index, n_x_rows)
    R, I = len(rows), len(Q)
    ids = np.full((R, top_k), -1, np.int32)
    scores = np.full((R, top_k), -np.inf, F32)
    count = np.zeros(R, np.int32)
    for r in range(R):
        if vec[r] < 0:
            continue
        seen = set(X.indices[X.indptr[x[r]]:X.indptr[x[r] + 1]].tolist()) if filter_interacted else set()
        cands = []
        for i in range(I):
            if (mask is not None and not mask[i]) or i in seen:
                continue
            s = F32(0.0)
            for c in range(P.shape[1]):
                s = fmaf(P[vec[r], c], Q[i, c], s)
            if s == s:
                cands.append((-float(s), i, s))
        cands.sort(key=lambda t: (t[0], t[1]))
        n = min(top_k, len(cands))
        count[r] = n
        ids[r, :n] = [t[1] for t in cands[:n]]
        scores[r, :n] = [t[2] for t in cands[:n]]
    return ids, scores, count


def host_scores(P, Q):
    """The score block [len(P), len(Q)] by the vectorised chain."""
    P, Q = np.asarray(P, F32), np.asarray(Q, F32)
    s = np.zeros((len(P), len(Q)), F32)
    for c in range(P.shape[1]):
        s = fma32(P[:, c][:, None], Q[:, c][None, :], s)
    return s


def host_model_fast(P, Q, top_k, rows=None, p_index=None, n_x_rows=None, X=None, mask=None, filter_interacted=False):
    """host_model_plain, vectorised: the chain through fma32, the order by a lexsort on (-score, id)."""
    P, Q = np.asarray(P, F32), np.asarray(Q, F32)
    rows = np.arange(len(P)) if rows is None else rows
    n_x_rows = (X.shape[0] if X is not None else len(P)) if n_x_rows is None else n_x_rows
    x, vec = _job_vectors(P, rows, p_index, n_x_rows)
    R, I = len(rows), len(Q)
    ids = np.full((R, top_k), -1, np.int32)
    scores = np.full((R, top_k), -np.inf, F32)
    count = np.zeros(R, np.int32)
    live = np.flatnonzero(vec >= 0)
    if not len(live) or not I:
        return ids, scores, count
    S = host_scores(P[vec[live]], Q)
    ok = ~np.isnan(S)
    if mask is not None:
        ok &= (np.asarray(mask) != 0)[None, :]
    if filter_interacted:
        for a, r in enumerate(live):
            ok[a, X.indices[X.indptr[x[r]]:X.indptr[x[r] + 1]]] = False
    for a, r in enumerate(live):
        c = np.flatnonzero(ok[a])
        s = S[a, c] + F32(0.0)
        order = np.lexsort((c, -s.astype(np.float64)))[:top_k]
        n = len(order)
        count[r] = n
        ids[r, :n], scores[r, :n] = c[order], S[a, c[order]]
    return ids, scores, count


def assert_same(got, want, what=""):
    g_ids, g_sc, g_cnt = [np.asarray(a) for a in got]
    w_ids, w_sc, w_cnt = [np.asarray(a) for a in want]
    assert np.array_equal(g_cnt, w_cnt), (what, "counts", np.flatnonzero(g_cnt != w_cnt)[:5])
    assert np.array_equal(g_ids, w_ids), (what, "ids", np.argwhere(g_ids != w_ids)[:5])
    same = (bits(g_sc) == bits(w_sc)) | (np.isnan(g_sc) & np.isnan(w_sc))
    assert same.all(), (what, "scores", np.argwhere(~same)[:5])


# ---------------------------------------------------------------------------------------------- inputs that tell roundings apart
def rounding_vectors(n_users, n_items, dim, seed):
    """P [n_users, dim], Q [n_items, dim] on which any other summation order, an unfused multiply or a wider accumulator
    changes bits: products that cancel a 2^24-sized partial sum, products that are float32 midpoints (1 + 2^-12)^2-style,
    products in the denormal range, and ordinary normals between them."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n_users, dim)).astype(F32)
    Q = rng.standard_normal((n_items, dim)).astype(F32)
    kind = rng.integers(0, 5, (n_users, dim))
    big = F32(2.0 ** 24) * rng.choice(np.array([1, -1, 3, -3], F32), (n_users, dim))
    P = np.where(kind == 0, big, P)
    P = np.where(kind == 1, F32(1.0) + F32(2.0 ** -12) * rng.integers(1, 64, (n_users, dim)).astype(F32), P)
    P = np.where(kind == 2, F32(2.0 ** -75) * rng.integers(1, 2 ** 20, (n_users, dim)).astype(F32), P)
    qkind = rng.integers(0, 5, (n_items, dim))
    Q = np.where(qkind == 0, rng.choice(np.array([1, -1, 0.5, -1], F32), (n_items, dim)), Q)
    Q = np.where(qkind == 1, F32(1.0) + F32(2.0 ** -12) * rng.integers(1, 64, (n_items, dim)).astype(F32), Q)
    Q = np.where(qkind == 2, F32(2.0 ** -74) * rng.integers(1, 2 ** 20, (n_items, dim)).astype(F32), Q)
    if dim >= 4:            # the issue's pattern, verbatim, on the first user and item: 2^24, 1, -2^24, 2^-12
        P[0, :4] = [2.0 ** 24, 1.0, -2.0 ** 24, 2.0 ** -12]
        Q[0, :4] = 1.0
    return np.ascontiguousarray(P.astype(F32)), np.ascontiguousarray(Q.astype(F32))


def test_fma32_is_libms_fmaf_on_adversarial_triples():
    rng = np.random.default_rng(1)
    n = 400_000
    a = (F32(1.0) + F32(2.0 ** -12) * rng.integers(0, 4096, n).astype(F32)) * F32(2.0) ** rng.integers(-70, 20, n).astype(F32)
    b = (F32(1.0) + F32(2.0 ** -12) * rng.integers(0, 4096, n).astype(F32)) * rng.choice(np.array([1, -1], F32), n)
    b *= F32(2.0) ** rng.integers(-70, 20, n).astype(F32)
    with np.errstate(all="ignore"):
        c = np.where(rng.random(n) < 0.5, -(a * b) * (F32(1.0) + F32(2.0 ** -23) * rng.integers(-3, 4, n).astype(F32)),
                     rng.standard_normal(n).astype(F32) * F32(2.0) ** rng.integers(-140, 30, n).astype(F32)).astype(F32)
        unfused = a * b + c
    got = fma32(a, b, c)
    want = np.array([_libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert int((unfused.view(np.int32) != want.view(np.int32)).sum()) > n // 10, "the triples do not tell fused from unfused"
    # specials go through as IEEE says
    sp_ = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, 2.0 ** -149, 3.0e38], F32)
    A, B, C = [g.ravel() for g in np.meshgrid(sp_, sp_, sp_)]
    want = np.array([_libm.fmaf(x, y, z) for x, y, z in zip(A.tolist(), B.tolist(), C.tolist())], F32)
    got = fma32(A, B, C)
    assert (np.isnan(got) == np.isnan(want)).all() and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


@pytest.mark.parametrize("dim", [1, 2, 3, 12, 13, 64])
def test_both_models_agree_on_rounding_sensitive_vectors(dim):
    P, Q = rounding_vectors(10, 14, dim, seed=dim)
    plain = host_model_plain(P, Q, 14)
    fast = host_model_fast(P, Q, 14)
    assert_same(fast, plain, f"dim {dim}")
    if dim >= 4:            # 2^24 + 1 - 2^24 + 2^-12: the chain loses the 1, any reassociation keeps it
        s = host_scores(P[:1], Q[:1])[0, 0]
        tail = F32(0.0)
        for c in range(4, dim):
            tail = fmaf(P[0, c], Q[0, c], tail)
        first4 = F32(0.0)
        for c in range(4):
            first4 = fmaf(P[0, c], Q[0, c], first4)
        assert first4 == F32(2.0 ** -12) and (dim > 4 or s == first4)
    # the vectors have teeth: the unfused float32 expression and a float64 accumulation both give other bits somewhere
    with np.errstate(all="ignore"):
        unfused = np.zeros((len(P), len(Q)), F32)
        for c in range(dim):
            unfused = unfused + P[:, c][:, None] * Q[:, c][None, :]
        wide = (P.astype(np.float64) @ Q.astype(np.float64).T).astype(F32)
    S = host_scores(P, Q)
    if dim >= 2:
        assert (bits(unfused) != bits(S)).any() and (bits(wide) != bits(S)).any()


def test_both_models_agree_on_long_chains_filters_and_ties():
    P, Q = rounding_vectors(3, 5, 256, seed=5)
    assert_same(host_model_fast(P, Q, 5), host_model_plain(P, Q, 5), "dim 256")
    assert_same(host_model_fast(P[:, :255], Q[:, :255], 3), host_model_plain(P[:, :255], Q[:, :255], 3), "dim 255")
    rng = np.random.default_rng(2)
    P = rng.integers(-2, 3, (9, 4)).astype(F32)
    Q = rng.integers(-2, 3, (40, 4)).astype(F32)
    Q[7, 0], P[2, 1], Q[9, 2], P[4, 0] = np.nan, np.inf, -np.inf, np.nan
    X = sp.random(7, 40, density=0.3, random_state=3, format="csr", dtype=F32)
    X.sort_indices()
    mask = (rng.random(40) < 0.7).astype(np.uint8)
    kw = dict(rows=[0, 1, -1, 7, 3, 4, 5, 6], p_index=np.array([1, -1, 2, 8, 9, 4, 0]), n_x_rows=7, X=X, mask=mask, filter_interacted=True)
    plain = host_model_plain(P, Q, 12, **kw)
    assert_same(host_model_fast(P, Q, 12, **kw), plain, "filters")
    ids, sc, cnt = plain
    assert cnt[2] == 0 and cnt[3] == 0 and (ids[2] == -1).all() and np.isneginf(sc[2]).all()      # row -1, row 7 = n_x_rows
    assert cnt[1] == 0 and cnt[5] == 0                                                             # vector index -1, and 9 = n_p
    assert cnt[6] == 0 and cnt[0] > 0 and cnt[4] > 0 and cnt[7] > 0                                # vector 4 holds a NaN: every score is one
    for r in range(len(cnt)):
        s, i = sc[r, :cnt[r]], ids[r, :cnt[r]]
        assert not np.isnan(s).any() and all(s[t] > s[t + 1] or (s[t] == s[t + 1] and i[t] < i[t + 1]) for t in range(len(s) - 1))
        if cnt[r]:
            assert mask[i].all() and not set(i.tolist()) & set(X.indices[X.indptr[kw["rows"][r]]:X.indptr[kw["rows"][r] + 1]].tolist())


def test_every_score_is_within_the_bound_of_a_chain_of_d_roundings():
    """|s - exact| <= gamma_d * sum_c |p_c q_c| with gamma_d = d u / (1 - d u), u = 2^-24: the standard bound for d roundings
    (each fmaf rounds once; the product is not rounded).  Finite, well-scaled vectors: no overflow, no denormal result."""
    rng = np.random.default_rng(4)
    for dim in (1, 12, 64, 256):
        P = rng.standard_normal((20, dim)).astype(F32)
        Q = (rng.standard_normal((30, dim)) * 10.0 ** rng.integers(-3, 4, (30, dim))).astype(F32)
        S = host_scores(P, Q).astype(np.float64)
        exact = P.astype(np.float64) @ Q.astype(np.float64).T
        mag = np.abs(P.astype(np.float64)) @ np.abs(Q.astype(np.float64)).T
        gamma = dim * U / (1.0 - dim * U)
        # float64's own error in `exact` and `mag` is 2^-29 of float32's: one part in 10^8 of the bound
        assert (np.abs(S - exact) <= gamma * mag * (1.0 + 1e-6)).all(), dim


# ---------------------------------------------------------------------------------------------- cases for the device tests
# The scan is instantiated per class of dim (8 / 32 / 128 B registers for dim <= 16 / 64 / 256) and of top_k (64 / 128 / 224 buffer
# entries for top_k <= 16 / 64 / 128); its A operands are loaded 16 k-steps at a time.  These are the dims on both sides of a class
# rule, and dims whose ceil(dim / 2) leaves the last group of 16 partly filled in the two larger classes.
CLASS_DIMS = [15, 16, 17, 31, 32, 33, 63, 65, 129]
# A case of more rows than a grid cap is built from 509 distinct pattern rows, row r carrying pattern r % 509: 65,536 % 509 = 384,
# so the rows r and r + 65,536 that one workgroup serves never carry the same pattern, and the host model runs on 509 rows.
PATTERNS = 509
GRID_CAP = 65536


def pattern_of(n_rows):
    return np.arange(n_rows) % PATTERNS


def tiled(want, n_rows):
    """The answer for n_rows rows from the answer for the patterns."""
    at = pattern_of(n_rows)
    return tuple(None if a is None else np.asarray(a)[at] for a in want)


def class_edge_case(dim, seed=0):
    """40 jobs x 200 items whose LAST component decides the lists: a class rule one too generous drops exactly that one."""
    rng = np.random.default_rng(900 + dim + seed)
    P = rng.standard_normal((40, dim)).astype(F32)
    Q = rng.standard_normal((200, dim)).astype(F32)
    P[:, dim - 1] = F32(8.0) * rng.choice(np.array([1, -1], F32), 40)
    return P, Q


def operand_case(dim):
    """test_identity_vectors_against_an_asymmetric_integer_matrix of tests/test_gpu_factor.py at any dim: P = unit vectors makes
    score(u, i) = Q[i, u % dim], so every component -- the last one, behind which the padding begins, included -- is somebody's
    whole score, and the transposed roles."""
    n_items, n_users = 40, max(33, dim + 1)
    i, c = np.meshgrid(np.arange(n_items), np.arange(dim), indexing="ij")
    Q = (i * 37 + c * 3 + (i * c) % 5 - 400).astype(F32)
    P = np.zeros((n_users, dim), F32)
    P[np.arange(n_users), np.arange(n_users) % dim] = 1
    u, c = np.meshgrid(np.arange(n_users), np.arange(dim), indexing="ij")
    P2 = (u * 29 - c * 7 + (u * c) % 3).astype(F32)
    Q2 = np.zeros((n_items, dim), F32)
    Q2[np.arange(n_items), np.arange(n_items) % dim] = 1
    return P, Q, P2, Q2


def filter_case(dim, seed=66):
    """The inputs of test_filter_mask_rows_strides_and_specials (tests/test_gpu_factor.py) at any dim >= 4: (P, Q, keyword
    arguments, x_rows)."""
    rng = np.random.default_rng(seed)
    n_items, n_x = 300, 8
    P = rng.standard_normal((6, dim)).astype(F32)
    Q = rng.standard_normal((n_items, dim)).astype(F32)
    P[4, 2], P[5, 1] = np.inf, np.nan
    Q[10, 2], Q[11, 2], Q[12, 0], Q[13, 3], Q[14, 2] = 0.0, -2.0, np.nan, np.inf, -np.inf
    p_index = np.array([0, 1, 2, 3, -1, 4, 5, 6])
    free = host_model_fast(P, Q, 40, rows=np.arange(n_x), p_index=p_index, n_x_rows=n_x)
    x_rows = [sorted(free[0][0, :30].tolist()), list(range(n_items)), [], sorted(rng.choice(n_items, 50, replace=False).tolist()), [],
              sorted(rng.choice(n_items, 20, replace=False).tolist()), [3], []]
    X = sp.csr_matrix((np.ones(sum(map(len, x_rows)), F32), np.concatenate([np.array(r, np.int64) for r in x_rows]),
                       np.r_[0, np.cumsum([len(r) for r in x_rows])]), shape=(n_x, n_items))
    rows = [0, 1, 2, 3, 4, 5, 6, 7, -1, n_x, 0, 3]
    return P, Q, dict(rows=rows, p_index=p_index, n_x_rows=n_x, X=X, filter_interacted=True), x_rows


MERGE_KINDS = ("chunk 0", "chunk 1", "short", "no vector", "both chunks")


def merge_kind(ids, count, top_k, has_vector):
    if not has_vector:
        return 3
    if count < top_k:
        return 2
    return 0 if (ids < 32).all() else 1 if (ids >= 32).all() else 4


def merge_trip_case(seed=7, extra=40):
    """More jobs than the merge kernel's grid (65,536 workgroups, one job per trip): 65,536 + 40 jobs over 64 items in two chunks
    of one tile, dim 2, top_k 3.  The items of chunk 0 have a positive first component and those of chunk 1 a negative one, the
    second component is 0 but at two admitted items (one per chunk).  A pattern's vector makes its merge take every entry from
    chunk 0 ((a, 0), a > 0), every entry from chunk 1 ((-a, 0)), fewer than top_k entries in total ((0, +-inf): NaN against every 0,
    +-inf against the two others; (NaN, 0): nothing), entries of both chunks (an ordinary vector), or it has no vector at all
    (p_index -1).  Returns a dict: P, Q, mask, p_index, rows, n_x_rows, top_k, splits, kind (designed, per pattern)."""
    rng = np.random.default_rng(seed)
    n_rows, top_k = GRID_CAP + extra, 3
    Q = np.zeros((64, 2), F32)
    Q[:32, 0] = (1 + rng.random(32)).astype(F32)
    Q[32:, 0] = -(1 + rng.random(32)).astype(F32)
    Q[5, 1], Q[40, 1] = 1.0, 2.0
    mask = (rng.random(64) < 0.6).astype(np.uint8)
    mask[[5, 40, 0, 1, 2, 33, 34, 35]] = 1
    kind = rng.integers(0, 5, PATTERNS)
    kind[:5], kind[384:389] = [0, 1, 2, 3, 4], [3, 4, 1, 0, 2]
    P = np.zeros((PATTERNS, 2), F32)
    a = (0.5 + rng.random(PATTERNS)).astype(F32)
    P[kind == 0, 0] = a[kind == 0]
    P[kind == 1, 0] = -a[kind == 1]
    short = np.flatnonzero(kind == 2)
    P[short, 1] = rng.choice(np.array([np.inf, -np.inf], F32), len(short))
    P[short[::3], 0], P[short[::3], 1] = np.nan, 0.0
    both = kind == 4
    P[both] = np.stack([rng.choice(np.array([0.25, -0.25], F32), both.sum()), F32(4.0) * a[both]], axis=1)       # items 40 and 5 lead
    P[kind == 3] = a[kind == 3][:, None]                                    # (a vector nobody may read)
    p_index = np.where(kind == 3, -1, np.arange(PATTERNS)).astype(np.int32)
    return dict(P=P, Q=Q, mask=mask, p_index=p_index, rows=pattern_of(n_rows).astype(np.int32), n_x_rows=PATTERNS, top_k=top_k, splits=2,
                kind=kind, n_rows=n_rows)


def merge_trip_answer(case):
    """(the host model's answer for the patterns, the kind of each pattern's answer)."""
    want = host_model_fast(case["P"], case["Q"], case["top_k"], rows=np.arange(PATTERNS), p_index=case["p_index"], n_x_rows=PATTERNS,
                           mask=case["mask"])
    kinds = np.array([merge_kind(want[0][x, :want[2][x]], want[2][x], case["top_k"], case["p_index"][x] >= 0) for x in range(PATTERNS)])
    return want, kinds


@pytest.mark.parametrize("dim", CLASS_DIMS)
def test_both_models_agree_on_the_class_edge_dims(dim):
    """The rounding test's own shape (64 x 96) on the dims around the class rules: the fast model is the definition, every one
    of the 6,144 scores is listed (none is NaN), and the last component -- the one a class rule one too generous drops -- moves
    score bits in more than half of the rows."""
    P, Q = rounding_vectors(64, 96, dim, seed=dim)
    fast = host_model_fast(P, Q, 96)
    assert_same(fast, host_model_plain(P, Q, 96), f"dim {dim}")
    assert int(fast[2].sum()) == 64 * 96
    S, less = host_scores(P, Q), host_scores(P[:, :dim - 1], Q[:, :dim - 1])
    assert int((bits(S) != bits(less)).any(axis=1).sum()) > 32               # (a row whose last component is a denormal may keep its bits)


@pytest.mark.parametrize("dim", [17, 65])
def test_class_edge_case_is_the_definition_and_hangs_on_its_last_component(dim):
    P, Q = class_edge_case(dim)
    want = host_model_fast(P, Q, 65)
    assert_same(want, host_model_plain(P, Q, 65), f"dim {dim}")
    assert (want[2] == 65).all()
    less = host_model_fast(P[:, :dim - 1], Q[:, :dim - 1], 17)
    assert (less[0] != want[0][:, :17]).any(axis=1).all(), "dropping the last component must change every job's list"


@pytest.mark.parametrize("dim", [13, 33])
def test_operand_and_filter_cases_at_odd_dims(dim):
    """Odd dims: the k-step of the last component has a zero half, behind which the padding begins."""
    P, Q, P2, Q2 = operand_case(dim)
    n_items = len(Q)
    want = host_model_fast(P, Q, n_items)
    assert_same(want, host_model_plain(P, Q, n_items), "P = I")
    assert_same(host_model_fast(P2, Q2, n_items), host_model_plain(P2, Q2, n_items), "Q = I")
    for u in range(len(P)):
        assert np.array_equal(np.sort(want[1][u]), np.sort(Q[:, u % dim]))
    assert len(P) > dim and dim % 2 == 1
    P, Q, kw, x_rows = filter_case(dim)
    want = host_model_plain(P, Q, 10, **kw)
    assert_same(host_model_fast(P, Q, 10, **kw), want, "filter")
    assert want[2].tolist() == [10, 0, 10, 10, 0, 10, 0, 0, 0, 0, 10, 10]
    assert not set(want[0][0].tolist()) & set(x_rows[0]) and np.isposinf(want[1][5]).any()


def test_merge_trip_case_is_the_definition_and_mixes_its_kinds_across_the_cap():
    case = merge_trip_case()
    want, kinds = merge_trip_answer(case)
    kw = dict(rows=np.arange(PATTERNS), p_index=case["p_index"], n_x_rows=PATTERNS, mask=case["mask"])
    assert_same(want, host_model_plain(case["P"], case["Q"], case["top_k"], **kw), "patterns")
    assert np.array_equal(kinds, case["kind"]), "every pattern's answer is of the kind it was built for"
    n_rows, at = case["n_rows"], case["rows"]
    assert n_rows == GRID_CAP + 40 and GRID_CAP % PATTERNS == 384 and np.array_equal(at, np.arange(n_rows) % PATTERNS)
    late, early = kinds[at[GRID_CAP:]], kinds[at[:n_rows - GRID_CAP]]
    for k in (0, 1, 2, 3):                                                  # among the rows past the cap and among their partners
        assert (late == k).any() and (early == k).any(), MERGE_KINDS[k]
    assert int((late != early).sum()) >= 10
    short = want[2][(kinds == 2)]
    assert set(short.tolist()) == {0, 2}                                    # (NaN, 0): nothing; (0, +-inf): the two items with a second component
    full = tiled(want, n_rows)
    assert full[0].shape == (n_rows, 3) and np.array_equal(full[0][GRID_CAP + 3], want[0][387])


# ---------------------------------------------------------------------------------------------- stack_bias
def test_stack_bias_is_the_references_hstack():
    from rtrec_amd.utils.factors import stack_bias
    rng = np.random.default_rng(6)
    user_biases, user_embeddings = rng.standard_normal(7), rng.standard_normal((7, 10))
    item_biases, item_embeddings = rng.standard_normal(5).astype(F32), rng.standard_normal((5, 10)).astype(F32)
    # the expressions of the reference's hybrid model (its lines 236 and 238)
    user_vector = np.hstack((user_biases[:, np.newaxis], np.ones((user_biases.size, 1)), user_embeddings), dtype=np.float32)
    item_vector = np.hstack((np.ones((item_biases.size, 1)), item_biases[:, np.newaxis], item_embeddings), dtype=np.float32)
    got_u, got_i = stack_bias(user_biases, user_embeddings, item_biases, item_embeddings)
    assert got_u.dtype == got_i.dtype == np.float32 and got_u.flags.c_contiguous and got_i.flags.c_contiguous
    assert np.array_equal(got_u, user_vector) and np.array_equal(got_i, item_vector) and got_u.shape == (7, 12)
    # the dot product of two stacked rows is b_u + b_i + e_u . e_i
    assert np.allclose(got_u @ got_i.T, user_biases[:, None] + item_biases[None, :] + user_embeddings @ item_embeddings.T, atol=1e-4)
    with pytest.raises(ValueError):
        stack_bias(user_biases, user_embeddings, item_biases, item_embeddings[:, :9])
    with pytest.raises(ValueError):
        stack_bias(user_biases[:6], user_embeddings, item_biases, item_embeddings)


# ---------------------------------------------------------------------------------------------- model / facade, end to end
class FactorOracleBackend(BlendOracleBackend):
    """The CPU stand-in with factor_topk from the host model (TEST-ONLY, like its bases)."""

    def factor_topk(self, row_ids, p_index, n_x_rows, p, qt, n_items, dim, item_mask, xb, filter_interacted, top_k, ids, scores,
                    count, item_splits=0):
        import torch
        n_rows = int(count.numel())
        X = None
        if filter_interacted:
            ptr, col = xb[0].numpy(), xb[1].numpy()
            X = sp.csr_matrix((np.ones(len(col), np.int32), col, ptr), shape=(len(ptr) - 1, max(n_items, int(col.max()) + 1 if len(col) else 0)))
        out = host_model_fast(p.numpy()[:, :dim], qt.numpy()[:dim, :n_items].T, top_k,
                              rows=np.arange(n_rows) if row_ids is None else row_ids.numpy(),
                              p_index=None if p_index is None else p_index.numpy(), n_x_rows=n_x_rows, X=X,
                              mask=None if item_mask is None else item_mask.numpy(), filter_interacted=filter_interacted)
        for dst, src in zip((ids, scores, count), out):
            dst.copy_(torch.from_numpy(src))


def cpu_slim(**kw):
    from rtrec_amd.models.slim import SLIM
    m = SLIM(**kw)
    m.model._engine = SlimEngine(backend=FactorOracleBackend())
    return m


def fitted_model(strings=False, cpu=True):
    """The golden fixture model (tests/golden/partial_fit.npz through _batch) as a float32 model."""
    from rtrec_amd.models.slim import SLIM
    batch = _batch(strings)
    m = cpu_slim(min_value=0, max_value=15, nn_feature_selection=5) if cpu else SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


def seeded_factors(batch, dim=12, seed=11, strings=False):
    """Seeded vectors for the fixture's users and items (dim 12: the reference's default 10 components plus the two bias slots),
    with two users and three items left without a vector and one id on each side the model does not know."""
    from rtrec_amd.utils.factors import stack_bias
    rng = np.random.default_rng(seed)
    users = sorted({u for u, _, _, _ in batch}, key=str)
    items = sorted({i for _, i, _, _ in batch}, key=str)
    no_vec_users, no_vec_items = [users[5], users[17]], [items[2], items[30], items[31]]
    fu = [u for u in users if u not in no_vec_users] + ["a stranger" if strings else 10 ** 8]
    fi = [i for i in items if i not in no_vec_items] + ["never seen" if strings else 10 ** 7]
    fu = [fu[j] for j in rng.permutation(len(fu))]
    fi = [fi[j] for j in rng.permutation(len(fi))]
    P, Q = stack_bias(rng.standard_normal(len(fu)) * 0.3, rng.standard_normal((len(fu), dim - 2)),
                      rng.standard_normal(len(fi)) * 0.3, rng.standard_normal((len(fi), dim - 2)))
    return dict(users=fu, P=P, items=fi, Q=Q, no_vec_users=no_vec_users, no_vec_items=no_vec_items, all_users=users, all_items=items)


def host_factor_lists(m, f, users, top_k, filter_interacted=True, candidate_items=None):
    """What the factor scorer owes the known users of `users` that have a vector, by the plain definition over raw ids:
    {position in users: (raw item ids, float32 scores)}."""
    n_items = m.model.n_items_fitted
    X = sp.csr_matrix(m.interactions.to_csr())
    X.sort_indices()
    vec_of = {u: f["P"][j] for j, u in enumerate(f["users"])}
    Q = np.zeros((n_items, f["P"].shape[1]), F32)
    mask = np.zeros(n_items, np.uint8)
    for j, i in enumerate(f["items"]):
        if i in f["all_items"]:
            Q[m.item_ids.get_id(i)], mask[m.item_ids.get_id(i)] = f["Q"][j], 1
    if candidate_items is not None:
        allowed = np.zeros(n_items, np.uint8)
        allowed[[m.item_ids.get_id(i) for i in candidate_items if i in f["all_items"]]] = 1
        mask &= allowed
    out = {}
    for b, u in enumerate(users):
        if u in f["all_users"] and u in vec_of:
            row = m._known_user_id(u)
            ids, sc, cnt = host_model_fast(vec_of[u][None, :], Q, top_k, rows=[0], p_index=None, n_x_rows=1,
                                           X=X[row:row + 1], mask=mask, filter_interacted=filter_interacted)
            out[b] = ([m.item_ids.get(int(i)) for i in ids[0, :cnt[0]]], sc[0, :cnt[0]])
    return out


HYBRID_CASES = (dict(top_k=10), dict(top_k=8, contact_counts=True), dict(top_k=5, pool=12, contact_counts=True, similarity_weight_factor=0.5),
                dict(top_k=8, weighting=0.6), dict(top_k=8, weighting=1.0, mnz=True), dict(top_k=6, contact_counts=True, filter_interacted=False))


def check_factor_and_hybrid(m, batch, strings, cases=HYBRID_CASES):
    """The API checks shared with tests/test_gpu_factor.py (there `m` runs on the device): every user of the fixture, two cold
    ones, users and items without a vector, ids the model does not know."""
    f = seeded_factors(batch, strings=strings)
    assert m.attach_factors(f["users"], f["P"], f["items"], f["Q"]) is m and m.has_factors()
    cold = ["nobody", "no one"] if strings else [max(f["all_users"]) + 1000, max(f["all_users"]) + 1001]
    users = f["all_users"][:120] + cold[:1] + f["all_users"][120:] + cold[1:]
    cold_list = m.recommend_batch(cold[:1], top_k=10)[0]
    # the second scorer alone
    for kw in (dict(top_k=10), dict(top_k=7, filter_interacted=False), dict(top_k=12, candidate_items=f["all_items"][::3] + f["items"][-1:])):
        want = host_factor_lists(m, f, users, kw["top_k"], kw.get("filter_interacted", True), kw.get("candidate_items"))
        got = m.recommend_factor_batch(users, **kw)
        ids, sc, cnt = m.recommend_factor_batch(users, as_arrays=True, **kw)
        assert ids.shape == sc.shape == (len(users), kw["top_k"]) and ids.dtype == np.int64 and len(want) == len(f["all_users"]) - 2
        for b, u in enumerate(users):
            n = int(cnt[b])
            assert [m.item_ids.get(int(i)) for i in ids[b, :n]] == got[b] and (ids[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all()
            if b in want:
                assert got[b] == want[b][0] and np.array_equal(bits(sc[b, :n]), bits(want[b][1])), (kw, b)
                assert not set(got[b]) & set(f["no_vec_items"])
            elif "candidate_items" not in kw:             # cold, or no vector: recommend_batch's cold-start list
                assert got[b] == cold_list[:kw["top_k"]] and (sc[b, :n] == 0).all(), (kw, b)
    assert m.recommend_factor(users[3], top_k=10) == m.recommend_factor_batch(users, top_k=10)[3]
    # the hybrid: the factor lists and SLIM's, blended by the host model of tests/test_blend_host.py
    counts = [(u, i, int(n)) for (u, i, _, _), n in zip(batch[::7], np.random.default_rng(3).integers(1, 5, len(batch)))]
    for kw in cases:
        kw = dict(kw, contact_counts=counts) if kw.get("contact_counts") else dict(kw)
        pool = kw.get("pool", kw["top_k"])
        lists = host_factor_lists(m, f, users, pool, kw.get("filter_interacted", True))
        others = [lists[b][0] if b in lists else [] for b in range(len(users))]
        other_scores = [lists[b][1].tolist() if b in lists else [] for b in range(len(users))]
        want = _expected(m, users, others, other_scores, kw["top_k"], pool, kw.get("contact_counts"), kw.get("similarity_weight_factor", 2.0),
                         kw.get("weighting", "contacts"), kw.get("mnz", False), kw.get("filter_interacted", True))
        got = m.recommend_hybrid_batch(users, **kw)
        ids, value, source, cnt = m.recommend_hybrid_batch(users, as_arrays=True, **kw)
        assert got == [w[0] for w in want], kw
        assert ids.shape == value.shape == source.shape == (len(users), kw["top_k"])
        for b, (w_ids, w_val, w_src) in enumerate(want):
            n = int(cnt[b])
            assert n == len(w_ids) and source[b, :n].tolist() == w_src and np.array_equal(value_bits(value[b, :n]), value_bits(w_val)), (kw, b)
        for b, u in enumerate(users):
            if u in cold:
                assert got[b] == []
            elif u in f["no_vec_users"]:
                assert all(s == 2 for s in want[b][2]) and len(got[b]) > 0       # SLIM's side alone
        assert any(3 in w[2] for w in want) and any(1 in w[2] for w in want)
    assert m.recommend_hybrid(users[3], top_k=8, contact_counts=counts) == m.recommend_hybrid_batch(users, top_k=8, contact_counts=counts)[3]
    assert m.recommend_hybrid_batch([]) == [] and m.recommend_factor_batch([]) == []
    return f, users


@pytest.mark.parametrize("strings", [False, True])
def test_recommend_factor_and_hybrid_batch_end_to_end(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = fitted_model(strings)
    f, users = check_factor_and_hybrid(m, batch, strings)
    rec = Recommender(m)
    assert rec.recommend_hybrid_batch(users[:9], top_k=6, weighting=0.4) == m.recommend_hybrid_batch(users[:9], top_k=6, weighting=0.4)
    assert rec.recommend_hybrid(users[2], top_k=6) == m.recommend_hybrid(users[2], top_k=6)
    assert rec.recommend_factor_batch(users[:9], top_k=6) == m.recommend_factor_batch(users[:9], top_k=6)
    assert rec.recommend_factor(users[2]) == m.recommend_factor(users[2])
    # refusals
    for kw in (dict(top_k=0), dict(pool=129), dict(top_k=129), dict(pool=0), dict(weighting="votes"), dict(weighting=-1.0),
               dict(similarity_weight_factor=-2.0)):
        with pytest.raises(ValueError):
            m.recommend_hybrid_batch(users[:3], **kw)
    with pytest.raises(ValueError, match="128"):
        m.recommend_hybrid_batch(users[:3], top_k=5, pool=200)
    assert m.recommend_hybrid_batch(users[:3], top_k=200, pool=128)                       # top_k is only a cut
    for kw in (dict(top_k=0), dict(top_k=129)):
        with pytest.raises(ValueError):
            m.recommend_factor_batch(users[:3], **kw)
    assert rec.detach_factors() is rec and not m.has_factors() and not m.model.engine.has_factors()
    for call in (lambda: m.recommend_hybrid_batch(users[:3]), lambda: m.recommend_factor_batch(users[:3])):
        with pytest.raises(RuntimeError, match="attach_factors"):
            call()
    with pytest.raises(ValueError):
        m.attach_factors(f["users"], f["P"][:, :5], f["items"], f["Q"])
    with pytest.raises(ValueError):
        m.attach_factors(f["users"][:-1], f["P"], f["items"], f["Q"])
    with pytest.raises(ValueError, match="float32"):
        m.attach_factors(f["users"], f["P"].astype(np.float64) + 1e-12, f["items"], f["Q"])
    rec.attach_factors(f["users"], f["P"].astype(np.float64), f["items"], f["Q"])      # float64 holding float32 numbers is served
    assert m.recommend_factor(users[2]) == rec.recommend_factor(users[2])


def test_attach_factors_maps_raw_ids_and_drops_unknown_ones():
    m, batch = fitted_model(True)
    f = seeded_factors(batch, strings=True)
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    F = m._factors
    assert len(F["user_rows"]) == len(f["users"]) - 1 and len(F["item_rows"]) == len(f["items"]) - 1
    for j, u in enumerate(f["users"]):
        if u != "a stranger":
            at = int(np.flatnonzero(F["user_rows"] == m._known_user_id(u))[0])
            assert np.array_equal(F["user_vectors"][at], f["P"][j])
    for j, i in enumerate(f["items"]):
        if i != "never seen":
            at = int(np.flatnonzero(F["item_rows"] == m.item_ids.get_id(i))[0])
            assert np.array_equal(F["item_vectors"][at], f["Q"][j])
    # what the engine receives: an index over X's rows (-1 without a vector), the items without a vector masked out
    m.recommend_factor_batch(f["all_users"][:2])
    E = m.model.engine._F
    index, mask = E["index"].numpy(), E["mask"].numpy()
    assert len(index) == m.model.engine.n_users and len(mask) == m.model.n_items_fitted == E["n_items"] and E["dim"] == 12
    assert sorted(np.flatnonzero(index < 0).tolist()) == sorted(m._known_user_id(u) for u in f["no_vec_users"])
    assert sorted(np.flatnonzero(mask == 0).tolist()) == sorted(m.item_ids.get_id(i) for i in f["no_vec_items"])
    assert tuple(E["qt"].shape) == (12, m.model.n_items_fitted) and np.array_equal(E["p"].numpy(), F["user_vectors"])


def test_engine_set_factors_checks_shapes_and_values():
    m, batch = fitted_model()
    m.recommend_batch([batch[0][0]])
    eng = m.model.engine
    n_items, n_users = m.model.n_items_fitted, eng.n_users
    rng = np.random.default_rng(0)
    P, Q = rng.standard_normal((n_users, 6)).astype(F32), rng.standard_normal((n_items, 6)).astype(F32)
    assert not eng.has_factors()
    eng.set_factors(P, Q)
    assert eng.has_factors()
    rows = [0, 3, n_users, -1, 5]
    got = eng.factor_topk_rows(rows, top_k=9)
    X = sp.csr_matrix(m.interactions.to_csr())
    X.sort_indices()
    assert_same(got, host_model_plain(P, Q, 9, rows=rows, n_x_rows=n_users, X=X, filter_interacted=True), "engine rows")
    mask = (rng.random(n_items) < 0.5)
    assert_same(eng.factor_topk_rows(rows, top_k=4, filter_interacted=False, item_mask=mask, item_splits=3),
                host_model_plain(P, Q, 4, rows=rows, n_x_rows=n_users, mask=mask), "engine mask")
    for bad in (lambda: eng.set_factors(P, Q[:-1]), lambda: eng.set_factors(P[:, :5], Q), lambda: eng.set_factors(P, Q, user_index=np.zeros(3)),
                lambda: eng.set_factors(P, Q, item_mask=np.ones(3)), lambda: eng.set_factors(np.zeros((2, 257), F32), np.zeros((n_items, 257), F32)),
                lambda: eng.set_factors(P.astype(np.float64) * 1.1, Q), lambda: eng.factor_topk_rows(rows, top_k=0),
                lambda: eng.factor_topk_rows(rows, top_k=129), lambda: eng.factor_topk_rows(rows, item_splits=65),
                lambda: eng.factor_topk_rows(rows, item_mask=np.ones(3))):
        with pytest.raises(ValueError):
            bad()
    eng.clear_factors()
    with pytest.raises(RuntimeError, match="set_factors"):
        eng.factor_topk_rows(rows)


def test_pickle_carries_the_vectors_only_when_attached():
    from rtrec_amd.models.slim import SLIM
    m, batch = fitted_model()

    def saved(model):
        buf = io.BytesIO()
        model.save(buf)
        return buf.getvalue()

    m.recommend_batch([batch[0][0]], top_k=5)          # (the first scoring call settles the flags scipy keeps on W)
    before = saved(m)
    assert saved(m) == before and sorted(m._serialize()) == ["feature_store", "interactions", "item_ids", "model", "user_ids"]
    f = seeded_factors(batch)
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    m.detach_factors()
    assert saved(m) == before, "a model without vectors must serialise exactly as it always did"
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    with_vectors = saved(m)
    assert "factors" in m._serialize() and len(with_vectors) > len(before) + f["P"].nbytes // 2
    want = m.recommend_hybrid_batch(f["all_users"][:6], top_k=5, weighting=0.5)
    back = SLIM.loads(with_vectors)
    back.model._engine = SlimEngine(backend=FactorOracleBackend())
    assert back.has_factors() and back.recommend_hybrid_batch(f["all_users"][:6], top_k=5, weighting=0.5) == want
    for key in ("user_rows", "user_vectors", "item_rows", "item_vectors"):
        assert np.array_equal(back._factors[key], m._factors[key])
    m.detach_factors()
    assert b"factors" not in saved(m) and b"factors" in with_vectors and sorted(m._serialize()) == sorted(SLIM.loads(before)._serialize())
    plain = SLIM.loads(before)
    assert not plain.has_factors()


# ---------------------------------------------------------------------------------------------- serving
def test_recommend_hybrid_route_token_payload_and_failure():
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    m, batch = fitted_model()
    f = seeded_factors(batch)
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = f["all_users"][0]
    r = client.post("/recommend_hybrid", json={"user": user}, headers=ok)                     # no vectors attached: the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Recommend hybrid failed"}
    m.attach_factors(f["users"], f["P"], f["items"], f["Q"])
    mine = m.recommend(user, top_k=6)
    body = {"user": user, "top_k": 6, "pool": 20, "contact_counts": [[mine[0], 3], [mine[1], 1]], "similarity_weight_factor": 0.5}
    r = client.post("/recommend_hybrid", json=body, headers={"X-Token": "wrong"})
    assert r.status_code == 400 and r.json() == {"detail": "Invalid X-Token header"}
    r = client.post("/recommend_hybrid", json=body, headers=ok)
    want = m.recommend_hybrid(user, top_k=6, pool=20, contact_counts=[(user, mine[0], 3), (user, mine[1], 1)], similarity_weight_factor=0.5)
    assert r.status_code == 200 and r.json() == {"user": user, "items": want} and len(want) == 6
    r = client.post("/recommend_hybrid", json={"user": user, "weighting": 0.7, "mnz": True}, headers=ok)
    assert r.status_code == 200 and r.json()["items"] == m.recommend_hybrid(user, weighting=0.7, mnz=True)
    r = client.post("/recommend_hybrid", json={"user": user, "pool": 500}, headers=ok)
    assert r.status_code == 500
    r = client.post("/recommend", json={"user": user, "top_k": 4}, headers=ok)                # the existing routes are untouched
    assert r.status_code == 200 and r.json()["recommendations"] == m.recommend(user, top_k=4)


# ---------------------------------------------------------------------------------------------- registration
def test_factor_topk_is_declared_registered_and_exported():
    import torch
    from rtrec_amd import _native, build, ops
    from tests.test_diverse_host import ext_declared_symbols
    assert "rtrec_factor_topk" in ext_declared_symbols() and ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    assert "rtrec_factor_topk" in _native.EXT_EXPORTS and "rtrec_factor_topk" not in _native.EXPORTS and "factor_topk.hip" in build.SOURCES
    assert "factor_topk" in ops.EXT_OPS and "factor_topk" not in ops.OPS and ops.EXT_EXPORT_OF["factor_topk"] == "rtrec_factor_topk"
    assert len(ops.OPS) == 22 and not any("factor" in name for name in _native.EXPORTS)      # the core surface did not grow
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert "FACTOR TOP-K" in header and "#define RTREC_FACTOR_TOPK_WORKSPACE_BYTES(n_rows, top_k, item_splits)" in header
    assert hasattr(ctypes.CDLL(build.LIB_PATH), "rtrec_factor_topk") and len(_native.load().rtrec_factor_topk.argtypes) == 24
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rtrec_amd")):      # called through the op only, never by ctypes
        for f in files:
            if f.endswith(".py") and f != "_native.py":
                assert ".rtrec_factor_topk(" not in open(os.path.join(dirpath, f)).read(), f
    schema = str(torch.ops.rtrec_amd.factor_topk.default._schema)
    assert schema.startswith("rtrec_amd::factor_topk(") and schema.endswith("-> ()")
    for name in ("ids", "scores", "count"):
        assert re.search(rf"Tensor\([a-z]!\) {name}\b", schema), schema
    assert re.search(r"Tensor\([a-z]!\)\? workspace\b", schema), schema
    for name in ("p", "qt"):
        assert f"Tensor {name}" in schema, schema
    for name in ("row_ids", "p_index", "item_mask", "xb_ptr", "xb_col"):
        assert f"Tensor? {name}" in schema, schema
    for arg in ("int n_x_rows", "int n_items", "int dim", "bool filter_interacted", "int top_k", "int item_splits"):
        assert arg in schema, schema
    if not torch.cuda.is_available():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
        with pytest.raises((NotImplementedError, RuntimeError)):
            torch.ops.rtrec_amd.factor_topk(None, None, 2, torch.zeros(2, 4), torch.zeros(4, 5), 5, 4, None, None, None, False, 3, 1,
                                            i32(2, 3), torch.zeros(2, 3), i32(2), None)
    from rtrec_amd.backend import HipBackend
    for name in ("set_factors", "has_factors", "factor_topk_device", "factor_topk_rows"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "factor_topk"))
    # the backend's own choice of chunks: the rule of the kernel file, never more chunks than tiles
    be = HipBackend.__new__(HipBackend)
    assert [be.factor_splits(n, 26744) for n in (1, 32, 33, 1000, 32768, 138493)] == [64, 64, 64, 32, 1, 1]
    assert be.factor_splits(1, 40) == 2 and be.factor_splits(1, 0) == 1 and be.factor_splits(5, 1000, 7) == 7 and be.factor_splits(5, 33, 7) == 2


def test_the_entry_point_checks_its_arguments_on_the_host():
    from rtrec_amd import _native
    fn = _native.load().rtrec_factor_topk
    one = 1                                                              # any non-NULL address: never dereferenced on these paths

    def args(n_rows=2, rows=one, pidx=one, n_x=4, p=one, ps=12, n_p=4, qt=one, qs=50, n_items=50, dim=12, mask=one, xptr=one, xcol=one,
             xnnz=3, filt=1, top_k=10, splits=1, ids=one, scores=one, count=one, ws=None, ws_bytes=0):
        return (n_rows, rows, pidx, n_x, p, ps, n_p, qt, qs, n_items, dim, mask, xptr, xcol, xnnz, filt, top_k, splits, ids, scores, count,
                ws, ws_bytes, None)

    for kw in (dict(dim=0), dict(dim=257, ps=257), dict(top_k=0), dict(top_k=129), dict(splits=-1), dict(splits=65)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_rows=-1), dict(n_x=-1), dict(n_p=-1), dict(n_items=-1), dict(xnnz=-1), dict(ps=11), dict(qs=49), dict(p=None),
               dict(qt=None), dict(ids=None), dict(scores=None), dict(count=None), dict(xptr=None), dict(xcol=None),
               dict(splits=2, ws=None, ws_bytes=1 << 20)):
        assert fn(*args(**kw)) == -1, kw
    need = 2 * 4 * (10 * 8 + 4)                                          # RTREC_FACTOR_TOPK_WORKSPACE_BYTES(2, 10, 4)
    assert fn(*args(splits=4, ws=one, ws_bytes=need - 1)) == -3
    assert fn(*args(n_rows=0)) == 0 and fn(*args(n_rows=0, p=None, qt=None, ids=None, xptr=None, splits=9)) == 0
    assert fn(*args(n_rows=0, dim=256, ps=256, top_k=128, splits=64)) == 0     # the limits themselves are served
