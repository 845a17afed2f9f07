"""rtrec_slim_score_topk at the value edges: a plain numpy definition of the call with the rule for NaN, +-inf and overflow
(include/rtrec_amd.h), builders of twelve named value sets, and the CPU checks of both.

The definition is held to the oracle (oracle.recommend_batch, the restated reference) bit for bit wherever the oracle is defined --
no NaN score -- and the builders assert, from the definition alone, that their rows hold what their names claim.  Mutated copies
of the definition show which value set catches which defect (MUTANTS).  The CPU paths -- the tests' stand-in backend and
SLIMElastic._topk_host -- are held to the rule on the value sets.  The device runs the same sets against the same definition
in tests/test_gpu_score_values.py (the tiled kernel follows the rule; the engine keeps such calls off the fast kernels), and
tests/test_score_selection_host.py holds a host model of the tiled selection to it.

The rule: a column whose score is NaN is never listed, takes no slot and is not counted; +inf is a number and is listed first, ties
by the mode's tie rule; -inf is never listed (`minus_inf_listed=False`) although the reference's SPARSE `sorted` lists it last
(`minus_inf_listed=True`, the form that is compared with the oracle): -inf is the kernels' mark of "no candidate"; DENSE mode drops
-inf in the reference as well.  A finite sum that overflows is +-inf and ranks as such.
"""
import numpy as np
import pytest
import scipy.sparse as sp

F32, F64 = np.float32, np.float64
SPARSE, DENSE = 0, 1
N_USERS, N_ITEMS, TILE = 40, 640, 256          # three tiles of 256 columns: 256 + 256 + 128
TOP_KS = (1, 10, 63, 64, 200)
HEAVY_ROWS = (5, 17, 300, 630)                 # rows of W dense enough for the compacted layout's dense blocks
PINF, NINF = F32(np.inf), F32(-np.inf)
NAN_POS, NAN_NEG = np.array([0x7fc00000, 0xffc00000], np.uint32).view(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.uint64)


class Case:
    """Raw CSR arrays of X (n_users x n_items) and W (n_items x n_items), both with ascending indices; stored zeros survive."""

    def __init__(self, name, xp, xi, xv, wp, wi, wv):
        self.name, self.xp, self.xi, self.xv, self.wp, self.wi, self.wv = name, xp, xi, xv, wp, wi, wv
        self.n_users, self.n_items = len(xp) - 1, len(wp) - 1
        self._sums = {}

    def X(self):
        return sp.csr_matrix((self.xv, self.xi, self.xp), shape=(self.n_users, self.n_items))

    def W(self):
        return sp.csr_matrix((self.wv, self.wi, self.wp), shape=(self.n_items, self.n_items))

    def w_coo_by_column(self):
        """(rows, cols, vals) sorted by (column, row): the order of DeviceWeights and of a CSC matrix."""
        rows = np.repeat(np.arange(self.n_items, dtype=np.int64), np.diff(self.wp))
        o = np.lexsort((rows, self.wi))
        return rows[o], self.wi[o].astype(np.int64), self.wv[o]

    def sums(self, f64, mutant=None):
        key = (bool(f64), mutant)
        if key not in self._sums:
            self._sums[key] = [raw_sums(self, u, F64 if f64 else F32, mutant) for u in range(self.n_users)]
        return self._sums[key]


# ---------------------------------------------------------------------------------------------- the definition
def raw_sums(case, u, dt, mutant=None):
    """Row u: the stored ratings in ascending item order, each rating's row of W in stored order, one rounded multiply and one
    rounded add per entry in `dt`.  Returns (acc[n_items], ft[n_items], order): the sums (+0 where nothing was added), the
    position in the user's row of the first rating that touched the column (-1: untouched), the touched columns in
    first-touch order."""
    acc = np.zeros(case.n_items, dt)
    ft = np.full(case.n_items, -1, np.int64)
    order = []
    s, e = int(case.xp[u]), int(case.xp[u + 1])
    items = case.xi[s:e]
    assert np.all(items[1:] > items[:-1])
    pos = 0
    with np.errstate(all="ignore"):
        for p in range(e - s):
            i, x = int(items[p]), dt(case.xv[s + p])
            a, b = int(case.wp[i]), int(case.wp[i + 1])
            cols, w = case.wi[a:b], case.wv[a:b].astype(dt)
            acc[cols] = acc[cols] + x * w                    # the columns of one row of W are distinct
            if mutant == "zero_times_inf" and b > a and not np.isfinite(x):
                rest = np.setdiff1d(np.arange(case.n_items), cols)          # a dense slice holds 0 where W stores nothing
                acc[rest] = acc[rest] + x * dt(0)
            new = cols[ft[cols] < 0]
            ft[new] = pos if mutant == "nan_shifts_first_touch" else p
            order.extend(new.tolist())
            if not (mutant == "nan_shifts_first_touch" and np.isnan(x)):
                pos += 1
        if mutant == "zero_times_inf":
            # ... and a user who does not rate a row has x = 0 for it: 0 * inf for every infinite weight of W
            rated = np.zeros(case.n_items, bool)
            rated[items] = True
            rows = np.repeat(np.arange(case.n_items), np.diff(case.wp))
            hit = ~np.isfinite(case.wv) & ~rated[rows]
            acc[case.wi[hit]] = acc[case.wi[hit]] + dt(0) * case.wv[hit].astype(dt)
    return acc, ft, np.asarray(order, np.int64)


def rank_row(case, u, mode, f64, filter_interacted, minus_inf_listed=False, mutant=None):
    """The whole ranked list of row u: (ids, scores in the accumulator's type, aux)."""
    acc, ft, order = case.sums(f64, mutant)[u]
    own = case.xi[int(case.xp[u]):int(case.xp[u + 1])]
    if mode == SPARSE:
        cand = order[::-1]                                   # scipy's product lists the touched columns last touched first
        cand = cand[acc[cand] != 0]                          # ... and drops the zero sums (NaN != 0: a NaN sum is kept so far)
        if filter_interacted:
            cand = cand[~np.isin(cand, own)]
        if not minus_inf_listed:
            cand = cand[acc[cand] != -np.inf]
        sc = acc[cand]
        nan = np.isnan(sc)
        nan_key = {"nan_listed_last": np.full(len(sc), -np.inf), "nan_listed_first": np.full(len(sc), np.inf),
                   "nan_by_sign_bit": np.where(np.signbit(sc), -np.inf, np.inf)}.get(mutant)
        if nan_key is not None:                              # mutants: a NaN competes, with the key an implementation might give it
            o = np.argsort(-np.where(nan, nan_key, sc), kind="stable")
            return cand[o], sc[o], ft[cand[o]]
        cand, sc = cand[~nan], sc[~nan]
        o = np.argsort(-sc, kind="stable")                   # Python's sorted(reverse=True) is stable: ties keep list order
        if mutant == "inf_ties_wrong_side":
            o = np.lexsort((-np.arange(len(sc)), -sc))       # (ties in the opposite order)
        return cand[o], sc[o], ft[cand[o]]
    sc = acc.copy()
    if filter_interacted:
        sc[own] = -np.inf
    idx = np.arange(case.n_items)
    nan = np.isnan(sc)
    nan_key = {"nan_listed_last": np.full(len(sc), -np.inf), "nan_listed_first": np.full(len(sc), np.inf),
               "nan_by_sign_bit": np.where(np.signbit(sc), -np.inf, np.inf)}.get(mutant)
    if nan_key is not None:
        o = np.lexsort((-idx, -np.where(nan, nan_key, sc)))
        o = o[sc[o] != -np.inf]                              # (NaN != -inf: the NaN columns stay)
        return idx[o], sc[o], np.zeros(len(o), np.int64)
    keep = ~nan & ((sc != -np.inf) | (mutant == "minus_inf_listed_dense"))
    idx, sc = idx[keep], sc[keep]
    o = np.lexsort((idx, -sc)) if mutant == "inf_ties_wrong_side" else np.lexsort((-idx, -sc))   # ties: the higher id first
    return idx[o], sc[o], np.zeros(len(o), np.int64)


def definition(case, rows, top_k, mode, f64, filter_interacted, minus_inf_listed=False, mutant=None):
    """(ids int32 [R, k], scores float32, scores float64 or None, aux uint32, counts int32) with the call's padding:
    id -1, score -inf, aux 0."""
    R = len(rows)
    ids = np.full((R, top_k), -1, np.int32)
    sc = np.full((R, top_k), -np.inf, F32)
    sc64 = np.full((R, top_k), -np.inf, F64) if f64 else None
    aux = np.zeros((R, top_k), np.uint32)
    cnt = np.zeros(R, np.int32)
    for r, u in enumerate(np.asarray(rows).tolist()):
        i, s, a = rank_row(case, u, mode, f64, filter_interacted, minus_inf_listed, mutant)
        n = min(len(i), top_k)
        if mutant == "nan_counted":
            acc = case.sums(f64)[u][0]
            n = min(top_k, n + int(np.isnan(acc).sum()))
            i, s, a = (np.concatenate([v, np.zeros(top_k, v.dtype)]) for v in (i, s, a))
        ids[r, :n], aux[r, :n], cnt[r] = i[:n], a[:n], n
        with np.errstate(over="ignore"):
            sc[r, :n] = s[:n].astype(F32)                    # float64 accumulations are rounded on output
        if f64:
            sc64[r, :n] = s[:n]
    return ids, sc, sc64, aux, cnt


def same(got, want, what=""):
    """`==` on ids, counts and aux, bits on scores (float64 ones too where both sides carry them)."""
    names = ("ids", "scores", "scores64", "aux", "count")
    for n, g, w in zip(names, got, want):
        if g is None or w is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        if n == "scores":
            g, w = bits(g), bits(w)
        elif n == "scores64":
            g, w = bits64(g), bits64(w)
        elif n == "aux":
            g, w = g.view(np.uint32) if g.dtype == np.int32 else g, w
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
            return f"{what}: {n} differ in {bad.size} of {len(w)} rows, first row {int(bad[0])}: got {g[bad[0]].tolist()[:12]} want {w[bad[0]].tolist()[:12]}"
    return ""


# ---------------------------------------------------------------------------------------------- the value sets
def _base(seed):
    """Dense work copies (value, stored mask) of a seeded X and W: users of 6-12 ratings in 0.5 .. 5, a W of 12 % signed weights
    with four rows 60 % full (dense blocks in every tile), every column stored at least once, no diagonal."""
    rng = np.random.default_rng(seed)
    Xv, Xm = np.zeros((N_USERS, N_ITEMS), F32), np.zeros((N_USERS, N_ITEMS), bool)
    for u in range(N_USERS):
        its = rng.choice(N_ITEMS, size=int(rng.integers(6, 13)), replace=False)
        Xm[u, its] = True
        Xv[u, its] = rng.choice(np.arange(0.5, 5.5, 0.5), size=len(its)).astype(F32)
    Wm = rng.random((N_ITEMS, N_ITEMS)) < 0.12
    for h in HEAVY_ROWS:
        Wm[h] = rng.random(N_ITEMS) < 0.6
    Wm[rng.integers(0, N_ITEMS, N_ITEMS), np.arange(N_ITEMS)] = True
    np.fill_diagonal(Wm, False)
    Wv = np.where(Wm, rng.uniform(-1.0, 1.0, Wm.shape), 0.0).astype(F32)
    Wv[Wm & (Wv == 0)] = F32(0.25)
    return rng, Xv, Xm, Wv, Wm


def _csr(v, m):
    ptr = np.zeros(m.shape[0] + 1, np.int32)
    np.cumsum(m.sum(axis=1), out=ptr[1:])
    r, c = np.nonzero(m)                                     # row-major, ascending columns
    return ptr, c.astype(np.int32), np.ascontiguousarray(v[r, c], F32)


def _rate(Xv, Xm, u, item, value):
    Xm[u, item], Xv[u, item] = True, value


def _store(Wv, Wm, row, col, value):
    Wm[row, col], Wv[row, col] = True, value


SPREAD = (3, 130, 250, 260, 400, 511, 520, 600, 639)        # columns in all three tiles, at tile edges


def build(name):
    rng, Xv, Xm, Wv, Wm = _base({n: k for k, n in enumerate(VALUE_SETS)}[name] + 100)
    light = [i for i in range(40, 80)]                       # ordinary rows of W (12 % full)
    if name == "nan_rating":
        for u in range(N_USERS):                             # the NaN is the user's middle rating: ratings come before and after it
            its = np.flatnonzero(Xm[u])
            if u % 2:
                Xv[u, its[len(its) // 2]] = NAN_POS if u % 4 == 1 else NAN_NEG
            else:                                            # ... or sits on a row of W with dense blocks
                _rate(Xv, Xm, u, HEAVY_ROWS[(u // 2) % 4], NAN_POS)
    elif name == "nan_weight":
        with np.errstate(invalid="ignore"):
            nan_from_inf = PINF - PINF
        assert np.isnan(nan_from_inf)
        vals = [NAN_POS, NAN_NEG, nan_from_inf, -nan_from_inf]
        for k in range(120):
            _store(Wv, Wm, int(rng.choice(HEAVY_ROWS + tuple(light))), int(rng.integers(0, N_ITEMS)), vals[k % 4])
        for u in range(N_USERS):
            _rate(Xv, Xm, u, HEAVY_ROWS[u % 4], F32(2.0))
        np.fill_diagonal(Wm, False)
    elif name == "inf_rating_mixed":
        for u in range(N_USERS):                             # two +inf ratings: +inf, -inf and (+inf) + (-inf) = NaN columns
            _rate(Xv, Xm, u, HEAVY_ROWS[u % 4], PINF)
            _rate(Xv, Xm, u, light[u % len(light)], PINF)
    elif name == "inf_times_stored_zero":
        z = HEAVY_ROWS[1]
        for c in SPREAD:
            _store(Wv, Wm, z, c, F32(0.0) if c % 2 else F32(-0.0))
        _store(Wv, Wm, light[0], 77, PINF)                   # ... and a stored zero RATING against an infinite weight
        for u in range(N_USERS):
            if u % 3 != 2:
                _rate(Xv, Xm, u, z, PINF)
            if u % 3 != 0:
                _rate(Xv, Xm, u, light[0], F32(0.0))
    elif name == "inf_weight":
        _store(Wv, Wm, HEAVY_ROWS[2], 411, PINF)
        Xm[:, 411] = False                                   # (nobody owns the column)
        for u in range(N_USERS):
            Xm[u, HEAVY_ROWS[2]] = False
            if u % 3 == 0:
                _rate(Xv, Xm, u, HEAVY_ROWS[2], F32(1.5) if u % 2 else F32(-1.5))
    elif name in ("plus_inf_ties", "minus_inf"):
        v = PINF if name == "plus_inf_ties" else NINF
        for c in SPREAD:
            _store(Wv, Wm, HEAVY_ROWS[0], c, v)
        for c in SPREAD[1::2]:
            _store(Wv, Wm, light[3], c + 1, v)               # a second row: ties across first-touch positions
        if name == "minus_inf":                              # ... and a row that leaves 40 columns above -inf: lists run into them
            for c in range(N_ITEMS):
                if c % 16 and c != light[4]:
                    _store(Wv, Wm, light[4], c, v)
        for u in range(N_USERS):
            Xm[u, HEAVY_ROWS[0]] = Xm[u, light[3]] = Xm[u, light[4]] = False
            if name == "minus_inf" and u % 8 == 0:
                _rate(Xv, Xm, u, light[4], F32(0.5))
            if u % 4 != 3:
                _rate(Xv, Xm, u, HEAVY_ROWS[0], F32(1.0))
            if u % 2:
                _rate(Xv, Xm, u, light[3], F32(2.0))
    elif name == "overflow_finite":
        Wv[HEAVY_ROWS[3]] = np.where(Wm[HEAVY_ROWS[3]], np.where(rng.random(N_ITEMS) < 0.5, 10.0, -10.0), 0.0).astype(F32)
        for u in range(N_USERS):
            Xm[u, HEAVY_ROWS[3]] = False
            if u % 4 != 3:
                _rate(Xv, Xm, u, HEAVY_ROWS[3], F32(3e38))
    elif name == "overflow_cancel":
        a, b = HEAVY_ROWS[0], HEAVY_ROWS[3]
        both = Wm[a] & Wm[b]
        Wv[a] = np.where(Wm[a], 10.0, 0.0).astype(F32)
        Wv[b] = np.where(Wm[b], np.where(both & (np.arange(N_ITEMS) % 2 == 0), -10.0, 10.0), 0.0).astype(F32)
        for u in range(N_USERS):
            _rate(Xv, Xm, u, a, F32(3e38))
            _rate(Xv, Xm, u, b, F32(3e38))
    elif name == "all_nan":
        for u in range(0, N_USERS, 2):                       # one NaN rating and nothing else
            Xm[u] = False
            _rate(Xv, Xm, u, HEAVY_ROWS[u % 4] if u % 4 else light[u % 7], NAN_POS)
    elif name == "few_numbers":
        Wm[light[5]] = False
        for c in SPREAD[:5]:
            _store(Wv, Wm, light[5], c + 2, F32(0.5 + c / 1000.0))
        for u in range(N_USERS):
            if u % 5 == 0:                                   # (some rows with numbers enough to fill a list of 200)
                _rate(Xv, Xm, u, light[6], NAN_NEG)
                continue
            Xm[u] = False
            _rate(Xv, Xm, u, light[5], F32(1.0 + u))
            _rate(Xv, Xm, u, HEAVY_ROWS[u % 4], NAN_NEG)
    elif name == "nan_is_own":
        Xm[:, 100:100 + N_USERS] = False
        for u in range(N_USERS):                             # item 100 + u is rated by user u alone; its row of W holds the NaN
            its = np.flatnonzero(Xm[u])
            _rate(Xv, Xm, u, 100 + u, F32(1.0))
            _store(Wv, Wm, 100 + u, int(its[-1] if its[-1] != 100 + u else its[0]), NAN_POS if u % 2 else NAN_NEG)
    else:
        raise KeyError(name)
    return Case(name, *_csr(Xv, Xm), *_csr(Wv, Wm))


VALUE_SETS = ("nan_rating", "nan_weight", "inf_rating_mixed", "inf_times_stored_zero", "inf_weight", "plus_inf_ties", "minus_inf",
              "overflow_finite", "overflow_cancel", "all_nan", "few_numbers", "nan_is_own")
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = build(name)
    return _CASES[name]


def competing(c, u, f64=False, filt=True):
    """(numeric, NaN, +inf, -inf) counts among row u's competing SPARSE columns."""
    acc, ft, order = c.sums(f64)[u]
    cand = order[acc[order] != 0]
    if filt:
        cand = cand[~np.isin(cand, c.xi[int(c.xp[u]):int(c.xp[u + 1])])]
    s = acc[cand]
    return int(np.isfinite(s).sum()), int(np.isnan(s).sum()), int(np.isposinf(s).sum()), int(np.isneginf(s).sum())


def tiles_of(cols):
    return set((np.asarray(cols) // TILE).tolist())


# ---------------------------------------------------------------------------------------------- the builders keep their promises
@pytest.mark.parametrize("name", VALUE_SETS)
def test_value_set_holds_what_its_name_claims(name):
    c = case(name)
    assert (c.n_users, c.n_items) == (N_USERS, N_ITEMS) and -(-N_ITEMS // TILE) >= 3
    assert np.all(np.diff(c.wp) >= 0) and all(np.all(np.diff(c.wi[c.wp[i]:c.wp[i + 1]]) > 0) for i in range(N_ITEMS))
    assert len(np.unique(c.wi)) == N_ITEMS                   # every column is stored: the compacted layout has all three tiles
    comp = np.array([competing(c, u) for u in range(N_USERS)])
    comp64 = np.array([competing(c, u, f64=True) for u in range(N_USERS)])
    total = comp.sum(axis=1)
    num, nan, pinf, ninf = comp.T
    assert (num + pinf >= 200).sum() >= 8, "rows that list at least 200 columns: top_k 64 and 200 fill"
    if name in ("nan_rating", "nan_weight", "inf_rating_mixed", "inf_times_stored_zero"):
        assert ((nan > 0) & (num + pinf >= 200)).sum() >= 8  # NaN scores in rows that also list 200 numbers
    if name == "nan_rating":
        # a listed column whose first touch lies BEHIND the NaN rating, in a row whose NaN is not the last rating
        seen = 0
        for u in range(N_USERS):
            xv = c.xv[c.xp[u]:c.xp[u + 1]]
            p = int(np.flatnonzero(np.isnan(xv))[0])
            acc, ft, order = c.sums(False)[u]
            seen += int(((ft > p) & ~np.isnan(acc) & (acc != 0)).sum() > 0)
        assert seen >= 20
        assert {bool(np.signbit(v)) for v in c.xv[np.isnan(c.xv)]} == {False, True}
    if name == "nan_weight":
        assert {bool(np.signbit(v)) for v in c.wv[np.isnan(c.wv)]} == {False, True} and np.isnan(c.wv).sum() >= 100
    if name == "inf_rating_mixed":
        assert ((nan > 0) & (pinf > 0) & (ninf > 0)).all()  # inf - inf in the middle of a sum, beside both infinities
        assert (np.isposinf(c.xv).sum() == 2 * N_USERS) and (comp64[:, 1] > 0).all()
    if name == "inf_times_stored_zero":
        assert (c.wv == 0).sum() == len(SPREAD) and np.signbit(c.wv[c.wv == 0]).any() and (c.xv == 0).any()
        rated = [u for u in range(N_USERS) if u % 3 != 2]
        for u in rated:                                      # every stored zero of the row is a NaN column (own items aside)
            acc = c.sums(False)[u][0]
            assert np.isnan(acc[list(SPREAD)]).all()
        assert tiles_of(SPREAD) == {0, 1, 2}
        assert all(np.isnan(c.sums(False)[u][0][77]) for u in range(N_USERS) if u % 3 != 0)     # 0 (stored) * inf
    if name == "inf_weight":
        r = np.array([u % 3 == 0 for u in range(N_USERS)])
        assert (nan == 0).all() and ((pinf + ninf)[r] == 1).all() and ((pinf + ninf)[~r] == 0).all() and pinf.sum() and ninf.sum()
    if name == "plus_inf_ties":
        assert (nan == 0).all() and (pinf >= 5).sum() >= 20 and (ninf == 0).all()
        u = int(np.argmax(pinf))
        acc = c.sums(False)[u][0]
        assert tiles_of(np.flatnonzero(np.isposinf(acc))) == {0, 1, 2} and len(set(c.sums(False)[u][1][np.isposinf(acc)].tolist())) == 2
    if name == "minus_inf":
        assert (nan == 0).all() and (ninf >= 5).sum() >= 20 and (pinf == 0).all()
        assert tiles_of(np.flatnonzero(np.isneginf(c.sums(False)[int(np.argmax(ninf))][0]))) == {0, 1, 2}
    if name == "overflow_finite":
        assert np.isfinite(c.xv).all() and np.isfinite(c.wv).all() and (nan == 0).all()
        assert (pinf > 50).sum() >= 20 and (ninf > 50).sum() >= 20
        assert (comp64[:, 2] == 0).all() and (comp64[:, 3] == 0).all()          # finite in float64: +-inf only when rounded on output
    if name == "overflow_cancel":
        assert np.isfinite(c.xv).all() and np.isfinite(c.wv).all()
        assert (nan > 20).all() and (pinf > 20).all() and (comp64[:, 1:] == 0).all()
    if name == "all_nan":
        assert ((total > 0) & (num + pinf + ninf == 0)).sum() == N_USERS // 2
    if name == "few_numbers":
        few = (num > 0) & (num < 10) & (nan > 200)
        assert few.sum() >= 30 and (num >= 200).sum() >= 8
    if name == "nan_is_own":
        assert (nan == 0).all()                              # with the filter the NaN column is gone anyway ...
        assert (np.array([competing(c, u, filt=False)[1] for u in range(N_USERS)]) == 1).all()      # ... without it, it competes


# ---------------------------------------------------------------------------------------------- the definition is the oracle's
def _oracle_same(oracle, c, rows, top_k, mode, f64, filt):
    X, W = c.X(), c.W()
    o_ids, o_sc, o_cnt = oracle.recommend_batch(X[rows], W, top_k=top_k, filter_interacted=filt, dense=(mode == DENSE), use_f64=f64)
    d = definition(c, rows, top_k, mode, f64, filt, minus_inf_listed=True)
    return same((o_ids, o_sc, None, None, o_cnt), d, f"{c.name} k={top_k} mode={mode} f64={f64} filter={filt}")


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("mode", [SPARSE, DENSE])
def test_definition_is_the_oracle_on_every_value_set_without_a_nan(oracle, mode, f64):
    """Bit for bit, with and without the filter, at top_k 1, 10, 63, 64 and 200 (63 and 64: the two sides of the kernels' threshold filter); the compared inputs hold +inf and -inf
    scores (checked), which the reference's SPARSE sorted() lists first and last."""
    compared, seen_pinf, seen_ninf = [], 0, 0
    for name in VALUE_SETS:
        c = case(name)
        rows = [u for u in range(N_USERS) if not np.isnan(c.sums(f64)[u][0]).any()]
        if len(rows) < N_USERS // 2:
            continue
        compared.append(name)
        for filt in (True, False):
            for k in TOP_KS:
                msg = _oracle_same(oracle, c, rows, k, mode, f64, filt)
                assert not msg, msg
        got = definition(c, rows, 200, SPARSE, f64, True, minus_inf_listed=True)[1]
        seen_pinf += int(np.isposinf(got).sum())
        live = np.arange(200)[None, :] < definition(c, rows, 200, SPARSE, f64, True, minus_inf_listed=True)[4][:, None]
        seen_ninf += int((np.isneginf(got) & live).sum())
    assert {"inf_weight", "plus_inf_ties", "minus_inf", "overflow_finite"} <= set(compared)
    assert "overflow_cancel" in compared or not f64          # float64: 3e39 - 3e39 is 0, not NaN
    assert seen_pinf > 100 and seen_ninf > 100


@pytest.mark.parametrize("key", [f"{w}_{m}_{f}" for w in ("f32", "f64") for m in ("sparse", "dense") for f in ("filter", "nofilter")])
def test_definition_is_the_oracle_on_the_golden_scoring_fixture(oracle, key):
    import os
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    zm, zs = np.load(os.path.join(G, "models.npz")), np.load(os.path.join(G, "scoring.npz"))
    ld = lambda p: sp.csc_matrix((zm[f"{p}_data"], zm[f"{p}_indices"], zm[f"{p}_indptr"]), shape=tuple(zm[f"{p}_shape"]))
    X, W = ld("X2").tocsr(), ld("W2_k50").tocsr()
    X.sort_indices(); W.sort_indices()
    c = Case("golden", X.indptr, X.indices, X.data.astype(F32), W.indptr, W.indices, W.data.astype(F32))
    w, m, f = key.split("_")
    users = zs["users"]
    msg = _oracle_same(oracle, c, users.tolist(), 10, DENSE if m == "dense" else SPARSE, w == "f64", f == "filter")
    assert not msg, msg
    if m == "sparse":                                        # ... and the fixture itself (generated by the real reference)
        d = definition(c, users.tolist(), 10, SPARSE, w == "f64", f == "filter")
        assert np.array_equal(d[0], zs[f"ids_{key}"]) and np.array_equal(bits(d[1]), bits(zs[f"scores_{key}"]))


# ---------------------------------------------------------------------------------------------- mutants
# defect -> the value sets that must catch it (mode, accumulator, filter of the catching call)
MUTANTS = {
    "nan_listed_last": ("few_numbers", SPARSE, False, True, (10, 200)),
    "nan_listed_first": ("nan_rating", SPARSE, False, True, (1, 10, 200)),
    "nan_by_sign_bit": ("nan_weight", DENSE, False, True, (1, 10, 200)),
    "nan_counted": ("all_nan", SPARSE, False, True, (1, 10, 200)),
    "nan_shifts_first_touch": ("nan_rating", SPARSE, False, True, (10, 200)),
    "minus_inf_listed_dense": ("minus_inf", DENSE, False, True, (63, 64, 200)),      # (40 columns stay above -inf)
    "inf_ties_wrong_side": ("plus_inf_ties", SPARSE, False, True, (10, 200)),
    "zero_times_inf": ("inf_weight", SPARSE, False, True, (64, 200)),
}


def _differs(name, mutant, mode, f64, filt, top_k):
    c = case(name)
    rows = list(range(N_USERS))
    return bool(same(definition(c, rows, top_k, mode, f64, filt, mutant=mutant), definition(c, rows, top_k, mode, f64, filt)))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_each_defect_is_caught_by_its_named_value_set(mutant):
    name, mode, f64, filt, top_ks = MUTANTS[mutant]
    for k in top_ks:
        assert _differs(name, mutant, mode, f64, filt, k), f"{mutant} is not caught by {name} at top_k {k}"


def test_mutant_table():
    """Which value set catches which defect (SPARSE and DENSE, float32, top_k 200): every defect by its named set, and the
    zero-times-infinity defect also by both sets that rate a row with +inf."""
    table = {m: [n for n in VALUE_SETS if _differs(n, m, SPARSE, False, True, 200) or _differs(n, m, DENSE, False, True, 200)]
             for m in sorted(MUTANTS)}
    for m, (name, *_rest) in MUTANTS.items():
        assert name in table[m], (m, table[m])
    assert {"inf_rating_mixed", "inf_times_stored_zero", "inf_weight"} <= set(table["zero_times_inf"])
    print("\n".join(f"{m:26s} {', '.join(v)}" for m, v in table.items()))


# ---------------------------------------------------------------------------------------------- the CPU paths follow the rule
def cpu_engine(c, f64=False, **kw):
    """A SlimEngine on the tests' CPU stand-in holding the value set; W as DeviceWeights, so that stored zeros survive."""
    import torch
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    from tests.cpu_backend import OracleBackend
    eng = SlimEngine(backend=OracleBackend(), **kw)
    eng.set_interactions(None, c.X(), need_csc=False)
    r, cc, v = c.w_coo_by_column()
    eng.set_weights(DeviceWeights(torch.from_numpy(r), torch.from_numpy(cc), torch.from_numpy(v.copy()), c.n_items, f64))
    return eng


@pytest.mark.parametrize("name", VALUE_SETS)
def test_cpu_stand_in_follows_the_rule(name):
    c = case(name)
    rows = np.array([3, 0, 7, 7, 39, 12, 20, 21, 8], np.int64)
    with np.errstate(all="ignore"):                          # float32: the stand-in leaves the oracle for its own selection
        assert not np.isfinite((c.X() @ c.W()).data).all()
    for f64 in (False, True):
        eng = cpu_engine(c, f64)
        for mode, filt, k in ((SPARSE, True, 10), (SPARSE, False, 200), (DENSE, True, 64), (DENSE, False, 10)):
            ids, sc, cnt = eng.recommend_rows(rows, top_k=k, filter_interacted=filt, mode=mode)
            want = definition(c, rows, k, mode, f64, filt)
            msg = same((ids, sc, None, None, cnt), want, f"{name} mode={mode} f64={f64} filter={filt} k={k}")
            assert not msg, msg
            assert not np.isnan(sc).any()


@pytest.mark.parametrize("name", ["nan_rating", "inf_rating_mixed", "minus_inf", "overflow_cancel", "all_nan"])
def test_large_k_host_selection_follows_the_rule(name):
    """SLIMElastic._topk_host (top_k beyond the fused kernel): score rows from the backend, selection in numpy."""
    from rtrec_amd import _native
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.models.internal.slim_elastic import SLIMElastic
    from tests.cpu_backend import OracleBackend
    c = case(name)
    se = SLIMElastic({"nn_feature_selection": 5}, engine=SlimEngine(backend=OracleBackend()))
    W = sp.csc_matrix(c.W())
    W.sort_indices()
    se.item_similarity = W
    se._sync_weights()                                        # (what _topk does before it hands over to _topk_host)
    Xb = c.X()
    zero_w = Case(c.name, c.xp, c.xi, c.xv, *(lambda m: (m.indptr, m.indices, m.data))(_without_zeros(c.W())))    # (an assigned W keeps no stored zero)
    for mode, filt in ((_native.TOPK_SPARSE, True), (_native.TOPK_SPARSE, False), (_native.TOPK_DENSE, True)):
        ids, sc, cnt = se._topk_host(Xb, None, N_ITEMS, filt, mode)
        want = definition(zero_w, range(N_USERS), N_ITEMS, mode, False, filt)
        msg = same((ids, sc, None, None, cnt), want, f"{name} mode={mode} filter={filt}")
        assert not msg, msg


def _without_zeros(m):
    m = sp.csr_matrix(m)
    keep = m.data != 0
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))[keep]
    out = sp.csr_matrix((m.data[keep], (rows, m.indices[keep])), shape=m.shape)
    out.sort_indices()
    return out
