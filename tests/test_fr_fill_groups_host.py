"""Host model of score_frows_kernel's first fill over STRIDED groups (rtrec_amd.layouts.fr_first_fill_model with
strided=True): group g holds register r of the lane 64 // regs * r places below g, so `regs` neighbouring columns fall into
`regs` different groups.  The list it leaves must hold the values of "the admissible non-zero sums, sorted descending,
the first kk"; equal values may come in any order (the kernel's emit sends such rows to the tie passes), so columns
are compared where a value is the only one of its size.  A run of strong neighbouring columns must leave (next to) no
extras, where the lane grouping leaves most of the run to merge()."""
import numpy as np
import pytest

from rtrec_amd.layouts import fr_fill_group_columns, fr_first_fill_model

NINF = np.float32(-np.inf)


def expected(sums, adm, kk):
    sums = np.asarray(sums, dtype=np.float32)
    idx = np.flatnonzero(np.asarray(adm, dtype=bool) & (sums != 0))
    order = idx[np.argsort(-sums[idx].astype(np.float64), kind="stable")]
    vals = np.full(kk, NINF, dtype=np.float32)
    cols = np.full(kk, -1, dtype=np.int64)
    n = min(kk, len(order))
    vals[:n], cols[:n] = sums[order[:n]], order[:n]
    return vals, cols, sums[order]


def check(sums, adm, kk):
    sums = np.asarray(sums, dtype=np.float32)
    m = fr_first_fill_model(sums, adm, kk, strided=True)
    vals, cols, all_sorted = expected(sums, adm, kk)
    assert np.array_equal(m["values"].view(np.uint32), vals.view(np.uint32))
    filled = m["cols"] >= 0
    assert np.array_equal(filled, vals > NINF) and len(set(m["cols"][filled].tolist())) == int(filled.sum())
    assert np.array_equal(sums[m["cols"][filled]], vals[filled]) and np.asarray(adm, dtype=bool)[m["cols"][filled]].all()
    distinct = np.array([(all_sorted == v).sum() == 1 for v in vals]) & filled
    assert np.array_equal(m["cols"][distinct], cols[distinct])
    assert m["n_inserted"] <= m["n_extras"]
    return m


def test_group_columns():
    for regs in (2, 4):
        for strided in (False, True):
            g = fr_fill_group_columns(regs, strided)
            assert g.shape == (64, regs) and np.array_equal(np.sort(g.ravel()), np.arange(64 * regs))
            assert (g % regs == np.arange(regs)).all()                      # register r holds the columns = r mod regs
        s = fr_fill_group_columns(regs, True)
        where = np.empty(64 * regs, dtype=np.int64)
        where[s.ravel()] = np.repeat(np.arange(64), regs)
        assert (np.diff(where.reshape(64, regs), axis=1) % 64 == 64 // regs).all()      # a lane's columns: regs different groups
        a = 5
        assert where[regs * a] == where[regs * ((a - 64 // regs) % 64) + 1] == a         # two columns of one group


@pytest.mark.parametrize("regs", [2, 4])
@pytest.mark.parametrize("kk", [2, 11, 16])
def test_random_tiles(regs, kk):
    rng = np.random.default_rng(1200 + 10 * regs + kk)
    tc = 64 * regs
    n_short = n_ties = 0
    for i in range(400):
        kind = i % 5
        if kind == 0:       # dense float sums
            sums = rng.normal(0, 1, tc)
        elif kind == 1:     # few distinct values: ties everywhere, across and inside groups
            sums = rng.integers(-3, 6, tc).astype(np.float32) * 0.25
        elif kind == 2:     # sparse: most sums zero, fewer than kk values now and then
            sums = np.where(rng.random(tc) < rng.uniform(0, 0.15), rng.uniform(0.1, 1, tc), 0)
        elif kind == 3:     # all negative
            sums = -rng.uniform(0.1, 1, tc)
        else:               # a few strided groups hold all the large values
            sums = rng.uniform(0, 0.1, tc)
            for g in rng.choice(64, 3, replace=False):
                sums[fr_fill_group_columns(regs, True)[g]] = rng.integers(5, 9, regs)
        adm = rng.random(tc) >= rng.choice([0.0, 0.1, 0.6])
        m = check(sums.astype(np.float32), adm, kk)
        n_short += int(m["values"][kk - 1] == NINF)
        n_ties += int(len(set(m["values"].tolist())) < kk)
    assert n_short > 0 and n_ties > 50


@pytest.mark.parametrize("regs", [2, 4])
@pytest.mark.parametrize("kk", [2, 11, 16])
def test_runs_of_neighbours(regs, kk):
    """A run of 12-20 strong neighbouring columns over a weak background: the lane grouping hands most of the run to merge(),
    the strided grouping none of it (a run shorter than 64 // regs * regs + 1 columns never meets itself in a group)."""
    rng = np.random.default_rng(1300 + 10 * regs + kk)
    tc = 64 * regs
    lane = strided = 0
    for _ in range(200):
        n = int(rng.integers(max(12, kk), 21))              # (at least kk: the whole list comes from the run)
        start = int(rng.integers(0, tc - n + 1))
        sums = rng.uniform(0.001, 0.01, tc).astype(np.float32)
        sums[start:start + n] = rng.permutation(n).astype(np.float32) + 1
        adm = np.ones(tc, dtype=bool)
        ms = check(sums, adm, kk)
        ml = fr_first_fill_model(sums, adm, kk)
        assert np.array_equal(ml["values"], ms["values"])
        assert ms["n_extras"] == 0
        lane += ml["n_extras"]
        strided += ms["n_extras"]
    # kk >= 11: a run of n <= 20 columns has at most ceil(n / regs) + 1 <= 11 lane maxima, so the kk-th lane maximum is at
    # most the run's smallest one, and every other sum of the run is an extra: n - ceil(n / regs) - 1 >= 4 of them per tile
    assert lane >= (1 if kk == 2 else 200 * 4) and strided == 0


@pytest.mark.parametrize("regs", [2, 4])
@pytest.mark.parametrize("kk", [2, 11, 16])
def test_extras_that_are_left(regs, kk):
    """Columns regs * a and regs * ((a - 64 // regs) % 64) + 1 share strided group a: the smaller of the two is an extra."""
    tc = 64 * regs
    all_ok = np.ones(tc, dtype=bool)
    for a in (0, 7, 64 // regs, 63):                    # (the first two: the partner lane wraps)
        c0, c1 = regs * a, regs * ((a - 64 // regs) % 64) + 1
        low = np.zeros(tc, dtype=np.float32)
        low[np.arange(64) * regs] = np.linspace(0.01, 0.02, 64)
        for v0, v1 in ((5.0, 4.0), (4.0, 5.0), (5.0, 5.0)):
            s = low.copy(); s[c0], s[c1] = v0, v1
            m = check(s, all_ok, kk)
            assert m["n_extras"] >= 1 and m["n_inserted"] >= 1
            assert set(m["cols"][:2].tolist()) == {c0, c1}
            if v0 == v1:                            # merge() puts the higher column first (c1 > c0 where the partner lane wraps)
                assert m["cols"][0] == max(c0, c1)
            else:
                assert m["cols"][0] == (c0 if v0 > v1 else c1)
        # the group's maximum is interacted: its second sum is ranked, nothing is left over
        s = low.copy(); s[c0], s[c1] = 5.0, 4.0
        adm = all_ok.copy(); adm[c0] = False
        m = check(s, adm, kk)
        assert m["cols"][0] == c1 and m["n_extras"] == 0
    # all of one group's registers above everything else, nothing else in the tile: regs - 1 extras while the list is short
    s = np.zeros(tc, dtype=np.float32)
    s[fr_fill_group_columns(regs, True)[9]] = np.arange(1, regs + 1)
    m = check(s, all_ok, kk)
    assert m["n_ranked"] == 1 and m["n_extras"] == regs - 1 == m["n_inserted"]
    # none at all; all interacted
    m = check(np.zeros(tc, np.float32), all_ok, kk)
    assert m["n_ranked"] == 0 and (m["cols"] == -1).all()
    check(np.ones(tc, np.float32), ~all_ok, kk)
    # exactly kk and kk - 1 neighbouring columns: kk different groups, no extras
    for n in (kk, kk - 1):
        s = np.zeros(tc, dtype=np.float32); s[3:3 + n] = np.linspace(1, 2, n)
        m = check(s, all_ok, kk)
        assert m["n_extras"] == 0 and m["n_ranked"] == n and (m["values"][kk - 1] > NINF) == (n == kk)
