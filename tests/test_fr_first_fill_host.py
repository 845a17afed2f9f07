"""Host model of score_frows_kernel's first fill (rtrec_amd.layouts.fr_first_fill_model: rank, place, extras): the list it
leaves must be "the admissible non-zero sums sorted by (score descending, column descending), the first kk of them".
Where the kk-th and the (kk+1)-th sum are equal, which of the equal columns stays is open (the row is re-scored by the
exact pass): only the values have to match there."""
import numpy as np
import pytest

from rtrec_amd.layouts import fr_first_fill_model

NINF = np.float32(-np.inf)


def expected(sums, adm, kk):
    sums = np.asarray(sums, dtype=np.float32)
    idx = np.flatnonzero(np.asarray(adm, dtype=bool) & (sums != 0))
    order = idx[np.lexsort((-idx, -sums[idx].astype(np.float64)))]            # score descending, then column descending
    vals = np.full(kk, NINF, dtype=np.float32)
    cols = np.full(kk, -1, dtype=np.int64)
    n = min(kk, len(order))
    vals[:n], cols[:n] = sums[order[:n]], order[:n]
    open_tie = len(order) > kk and sums[order[kk]] == sums[order[kk - 1]]
    return vals, cols, open_tie


def check(sums, adm, kk):
    m = fr_first_fill_model(sums, adm, kk)
    vals, cols, open_tie = expected(sums, adm, kk)
    assert np.array_equal(m["values"].view(np.uint32), vals.view(np.uint32))
    if open_tie:                # the columns above the tie group are settled all the same
        above = vals > vals[kk - 1]
        assert np.array_equal(m["cols"][above], cols[above])
        s = np.asarray(sums, dtype=np.float32)
        assert (s[m["cols"][~above]] == vals[kk - 1]).all() and len(set(m["cols"].tolist())) == kk
    else:
        assert np.array_equal(m["cols"], cols)
    return m


@pytest.mark.parametrize("regs", [2, 4])
def test_random_tiles(regs):
    rng = np.random.default_rng(100 + regs)
    n_extras = n_ties = 0
    for i in range(1500):
        kk = int(rng.integers(2, 17))
        tc = 64 * regs
        kind = i % 5
        if kind == 0:       # dense float sums
            sums = rng.normal(0, 1, tc)
        elif kind == 1:     # few distinct values: ties everywhere, across and inside lanes
            sums = rng.integers(-3, 6, tc).astype(np.float32) * 0.25
        elif kind == 2:     # sparse: most sums zero, fewer than kk values now and then
            sums = np.where(rng.random(tc) < rng.uniform(0, 0.15), rng.uniform(0.1, 1, tc), 0)
        elif kind == 3:     # all negative
            sums = -rng.uniform(0.1, 1, tc)
        else:               # a few lanes hold all the large values
            sums = rng.uniform(0, 0.1, tc)
            hot = rng.choice(64, 3, replace=False)
            for lane in hot:
                sums[lane * regs:(lane + 1) * regs] = rng.integers(5, 9, regs)
        adm = rng.random(tc) >= rng.choice([0.0, 0.1, 0.6])
        m = check(sums.astype(np.float32), adm, kk)
        n_extras += m["n_inserted"]
        n_ties += int(expected(sums.astype(np.float32), adm, kk)[2])
    assert n_extras > 100 and n_ties > 50           # both rare paths were exercised


@pytest.mark.parametrize("regs", [2, 4])
@pytest.mark.parametrize("kk", [2, 11, 16])
def test_constructed_tiles(regs, kk):
    tc = 64 * regs
    all_ok = np.ones(tc, dtype=bool)
    z = np.zeros(tc, dtype=np.float32)

    def low():                  # one small sum per lane, in its first register
        s = z.copy(); s[np.arange(64) * regs] = np.linspace(0.01, 0.02, 64)
        return s
    # none at all; all interacted; all zero
    m = check(z, all_ok, kk)
    assert m["n_ranked"] == 0 and (m["cols"] == -1).all()
    check(np.ones(tc, np.float32), ~all_ok, kk)
    # fewer than kk values, in different lanes and in one lane
    s = z.copy(); s[[3 * regs, 40 * regs + 1][:kk - 1]] = [0.5, 0.25][:kk - 1]
    m = check(s, all_ok, kk)
    assert m["values"][kk - 1] == NINF
    s = z.copy(); s[7 * regs:8 * regs] = np.arange(1, regs + 1)
    m = check(s, all_ok, kk)
    assert m["n_ranked"] == 1 and m["n_extras"] == regs - 1 == m["n_inserted"]      # (ascending: each beats the last)
    # exactly kk and kk - 1 values in distinct lanes
    for n in (kk, kk - 1):
        s = z.copy(); s[np.arange(n) * 3 * regs % tc] = np.linspace(1, 2, n)
        m = check(s, all_ok, kk)
        assert m["n_extras"] == 0 and (m["values"][kk - 1] > NINF) == (n == kk)
    # ties inside the top k: equal sums in different lanes, the higher column first
    s = low(); s[[5 * regs, 50 * regs, 20 * regs + 1]] = 3.0
    m = check(s, all_ok, kk)
    assert m["cols"][0] == 50 * regs and (kk < 3 or m["cols"][2] == 5 * regs)
    # more than one top value in one lane: the lane's other registers are extras
    s = low(); s[9 * regs:10 * regs] = 5.0 + np.arange(regs); s[30 * regs] = 4.0
    m = check(s, all_ok, kk)
    assert m["n_extras"] == m["n_inserted"] == regs - 1 and m["cols"][0] == 10 * regs - 1
    # ... equal ones
    s = low(); s[9 * regs:10 * regs] = 5.0
    m = check(s, all_ok, kk)
    assert m["cols"][0] == 10 * regs - 1
    # negative values only, some interacted: the largest raw sums are masked
    s = -np.linspace(1, 2, tc).astype(np.float32)
    adm = all_ok.copy(); adm[:5] = False
    m = check(s, adm, kk)
    assert m["cols"][0] == 5 and (m["values"] < 0).all()
    # a tie group across kk | kk + 1: values only
    s = z.copy(); s[np.arange(kk + 2) * regs] = [2.0] * (kk - 1) + [1.0] * 3
    check(s, all_ok, kk)
