"""rtrec_slim_score_topk on the device at the value edges: the twelve value sets of tests/test_score_values_host.py, held to
the same numpy `definition` as the CPU paths -- ids, counts and tie keys with `==`, score bits with `==` (the float64 outputs
too), no NaN in any output, padding -1 / -inf / 0.

The tiled form is forced (feature rows and segments off) and every path a test believes it covers is asserted: the path the
engine reports, the dense blocks of the compacted layout, the rows the exact-tie pass re-scored.  With the engine's default
settings the value sets must come out the same through the routing (score_plan.values_ordinary sends them to the tiled
kernel), ordinary data must keep its fast path, and changing a rating or the weights must switch the path.  Every mutant of
the definition is shown absent on the device by its named set.

These sets ran on a device only after select_topk's admission was `key > -inf` and the host model of the selection
(tests/test_score_selection_host.py) agreed with the definition: with the admission before that, a NaN score could make the
kernel read result slots nobody wrote.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_score_values_host import (DENSE, F32, HEAVY_ROWS, MUTANTS, N_ITEMS, N_USERS, NAN_POS, PINF, SPARSE, TILE, TOP_KS,
                                          VALUE_SETS, Case, _base, _csr, bits, case, definition, same)

pytestmark = pytest.mark.gpu

ROW_LIST = [3, 0, 7, 7, 39, 12, 20, 21, 8]                  # shuffled, with a repeat


def expected(c, rows, top_k, mode, f64, filt, mutant=None):
    """The definition's answer as the device hands it out, and the number of rows its exact-tie pass re-scores.  The tie key
    (aux) of an entry is its first-touch position only in the rows that pass re-scored: SPARSE mode, rows whose leading
    top_k + 1 scores -- in the accumulator's type -- hold an exact tie; everywhere else the key is 0."""
    ids, sc, sc64, aux, cnt = definition(c, rows, top_k, mode, f64, filt, mutant=mutant)
    n_flag = 0
    if mode == SPARSE:
        _i, s1, s1_64, _a, c1 = definition(c, rows, top_k + 1, mode, f64, filt, mutant=mutant)
        s = s1_64 if f64 else s1
        live = np.arange(top_k + 1)[None, :] < c1[:, None]
        tie = ((s[:, 1:] == s[:, :-1]) & live[:, 1:]).any(axis=1)
        aux = np.where(tie[:, None], aux, 0).astype(np.uint32)
        n_flag = int(tie.sum())
    else:
        aux = np.zeros_like(aux)
    return (ids, sc, sc64, aux, cnt), n_flag


class Dev:
    """One value set on the device: X resident, W as DeviceWeights from the raw (column, row) triples, so that stored zeros
    survive."""

    def __init__(self, c, f64, forced_tiled):
        import torch
        from rtrec_amd.engine import SlimEngine
        self.torch, self.c, self.f64 = torch, c, f64
        self.eng = SlimEngine(device="cuda:0")
        if forced_tiled:
            self.eng.use_feature_rows = False
            self.eng.use_seg_layout = False
        self.eng.rescored = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        self.set_x(c)
        self.set_w(c)

    def set_x(self, c):
        self.eng.set_interactions(None, c.X(), need_csc=False)

    def set_w(self, c):
        torch = self.torch
        from rtrec_amd.backend import DeviceWeights
        r, cc, v = c.w_coo_by_column()
        dev = "cuda:0"
        self.eng.set_weights(DeviceWeights(torch.from_numpy(r).to(dev), torch.from_numpy(cc).to(dev), torch.from_numpy(v.copy()).to(dev),
                                           c.n_items, self.f64))

    def run(self, rows, top_k, mode, filt):
        """(ids, scores, float64 scores or None, tie keys, counts) as numpy, and the rows the exact-tie pass re-scored."""
        torch, eng = self.torch, self.eng
        d_rows = torch.tensor(rows, dtype=torch.int32, device="cuda:0")
        eng.rescored.fill_(-1)
        out = eng._local_topk(d_rows, len(rows), eng._x_csr(), top_k, filt, mode, None)
        torch.cuda.synchronize()
        got = tuple(None if t is None else t.cpu().numpy() for t in out)
        return got, int(eng.rescored.item())


def check_outputs(got, want, what, top_k):
    msg = same(got, want, what)
    assert not msg, msg
    ids, sc, sc64, aux, cnt = got
    assert not np.isnan(sc).any() and (sc64 is None or not np.isnan(sc64).any()), what
    pad = np.arange(top_k)[None, :] >= cnt[:, None]
    assert (ids[pad] == -1).all() and np.isneginf(sc[pad]).all() and (aux[pad] == 0).all(), what
    assert sc64 is None or np.isneginf(sc64[pad]).all(), what
    listed = sc64 if sc64 is not None else sc                # (a finite float64 score may round to -inf on output)
    assert (ids[~pad] >= 0).all() and not np.isneginf(listed[~pad]).any(), what


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", VALUE_SETS)
def test_tiled_form_follows_the_value_rule(name, f64):
    """Feature rows and segments off: SPARSE and DENSE, with and without the filter, top_k 1 / 10 / 63 / 64 / 200 (quad maxima,
    lane bests, both sides of the threshold filter, successive scans), tiles of 256 (three tiles and the merge kernel) and
    one tile (direct emit), all 40 rows and a shuffled row list with a repeat."""
    c = case(name)
    d = Dev(c, f64, forced_tiled=True)
    rescored_total = 0
    for tile_cols in (256, 1024):
        d.eng.tile_cols = tile_cols
        lay = d.eng._layout(True, 10)
        assert lay["n_tiles"] == (3 if tile_cols == 256 else 1) and lay["n_cols"] == N_ITEMS
        if tile_cols == 256:                                 # the heavy rows of W are dense blocks (a segment with a stored zero is not)
            di = lay["dense_idx"].cpu().numpy().reshape(lay["n_tiles"], N_ITEMS)
            assert lay["n_dense"] > 0
            W = c.W()
            for h in HEAVY_ROWS:
                seg = lambda t: W.data[W.indptr[h]:W.indptr[h + 1]][W.indices[W.indptr[h]:W.indptr[h + 1]] // TILE == t]
                for t in range(lay["n_tiles"]):             # (the 128 columns of the last tile are rarely full enough)
                    full = len(seg(t)) >= max(64, int(TILE / 3.0))
                    assert (di[t, h] >= 0) == bool(full and not (seg(t) == 0).any()), (h, t)
            assert (di[:2, list(HEAVY_ROWS)] >= 0).sum() >= (6 if name == "inf_times_stored_zero" else 8)
        for rows in (list(range(N_USERS)), ROW_LIST):
            for mode in (SPARSE, DENSE):
                for filt in (True, False):
                    for k in TOP_KS:
                        what = f"{name} f64={f64} tile={tile_cols} rows={len(rows)} mode={mode} filter={filt} k={k}"
                        got, n_rescored = d.run(rows, k, mode, filt)
                        assert d.eng.last_score_path == "tiled", (what, d.eng.last_score_path)
                        want, n_flag = expected(c, rows, k, mode, f64, filt)
                        print(what, "rescored", n_rescored, "expected", n_flag)
                        check_outputs(got, want, what, k)
                        assert n_rescored == n_flag, what
                        rescored_total += n_rescored
    if name == "plus_inf_ties":
        assert rescored_total > 0


def base_case(seed=7):
    """An undoctored set: `_base` alone."""
    _rng, Xv, Xm, Wv, Wm = _base(seed)
    return Case("base", *_csr(Xv, Xm), *_csr(Wv, Wm))


def with_rating(c, u, value):
    """`c` with the first rating of user u replaced."""
    xv = c.xv.copy()
    xv[int(c.xp[u])] = value
    return Case(c.name + "+rating", c.xp, c.xi, xv, c.wp, c.wi, c.wv)


def with_nan_first_ratings(c):
    """`c` with every user's first rating a NaN: the first-touch positions of everything listed lie behind a NaN rating."""
    xv = c.xv.copy()
    xv[c.xp[:-1][np.diff(c.xp) > 0]] = NAN_POS
    return Case(c.name + "+nan_first", c.xp, c.xi, xv, c.wp, c.wi, c.wv)


def with_weight(c, value):
    wv = c.wv.copy()
    wv[int(c.wp[HEAVY_ROWS[0]])] = value
    return Case(c.name + "+weight", c.xp, c.xi, c.xv, c.wp, c.wi, wv)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_default_settings_route_every_value_set_to_the_tiled_kernel(f64):
    rows = list(range(N_USERS))
    for name in VALUE_SETS:
        c = case(name)
        d = Dev(c, f64, forced_tiled=False)
        for mode, filt, k in ((SPARSE, True, 10), (DENSE, True, 10), (SPARSE, False, 63), (DENSE, False, 1)):
            what = f"{name} f64={f64} default settings mode={mode} filter={filt} k={k}"
            got, _n = d.run(rows, k, mode, filt)
            assert d.eng.last_score_path == "tiled", (what, d.eng.last_score_path)
            # (no fast form is even built of a W that holds a NaN or an infinity)
            assert ("fast" in d.eng._W) == bool(np.isfinite(c.wv).all()), what
            check_outputs(got, expected(c, rows, k, mode, f64, filt)[0], what, k)


def test_ordinary_data_keeps_its_fast_path_and_a_changed_value_switches_it():
    """The routing costs ordinary data nothing: an undoctored set reports a fast path and is the definition's.  One rating
    changed through set_interactions, or the weights replaced, and the same engine reports the tiled kernel -- the cached
    parts of the fact go with the ratings and the weights they describe -- and back."""
    rows = list(range(N_USERS))
    c = base_case()
    d = Dev(c, False, forced_tiled=False)

    def call(cc, fast):
        for mode, filt in ((SPARSE, True), (DENSE, True), (SPARSE, False)):
            got, _n = d.run(rows, 10, mode, filt)
            path = d.eng.last_score_path
            what = f"{cc.name} mode={mode} filter={filt} path={path}"
            assert (path in ("feature_rows", "segments")) if fast else (path == "tiled"), what
            want, _nf = expected(cc, rows, 10, mode, False, filt)
            msg = same(got[:3] + (None,) + got[4:], want, what)          # (a fast pass re-scores its own flagged rows: keys aside)
            assert not msg, msg
            assert not np.isnan(got[1]).any()

    call(c, fast=True)
    assert d.eng._X["rval_bound"] is not None and d.eng._W["w_absmax"] < 2.0
    for value in (NAN_POS, PINF, F32(3e38)):
        cx = with_rating(c, 11, value)
        d.set_x(cx)
        call(cx, fast=False)
        d.set_x(c)
        call(c, fast=True)
    for value in (NAN_POS, -PINF):
        cw = with_weight(c, value)
        d.set_w(cw)
        call(cw, fast=False)
        d.set_w(c)
        call(c, fast=True)
    # a batch that is not resident pays the fact per call: the same rows handed in as a host CSR batch
    for cc, fast in ((c, True), (with_rating(c, 11, NAN_POS), False)):
        ids, sc, cnt = d.eng.recommend_csr(cc.X(), top_k=10, filter_interacted=True, mode=SPARSE)
        assert (d.eng.last_score_path in ("feature_rows", "segments")) if fast else (d.eng.last_score_path == "tiled")
        want = definition(cc, rows, 10, SPARSE, False, True)
        msg = same((ids, sc, None, None, cnt), want, f"{cc.name} host batch")
        assert not msg, msg


def test_golden_fixture_keeps_its_fast_path():
    import os
    import torch
    from rtrec_amd.engine import SlimEngine
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    zm, zs = np.load(os.path.join(G, "models.npz")), np.load(os.path.join(G, "scoring.npz"))
    ld = lambda p: sp.csc_matrix((zm[f"{p}_data"], zm[f"{p}_indices"], zm[f"{p}_indptr"]), shape=tuple(zm[f"{p}_shape"]))
    X, W = ld("X2").tocsr(), ld("W2_k50")
    X.sort_indices(); W.sort_indices()
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(None, X, need_csc=False)
    eng.set_weights(W.astype(np.float32))
    ids, sc, cnt = eng.recommend_rows(zs["users"], top_k=10, filter_interacted=True, mode=SPARSE)
    assert eng.last_score_path in ("feature_rows", "segments"), eng.last_score_path
    assert np.array_equal(ids, zs["ids_f32_sparse_filter"]) and np.array_equal(bits(sc), bits(zs["scores_f32_sparse_filter"]))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_device_does_not_carry_the_defect(mutant):
    """The device's answer on the mutant's named set, at its named top_k, is the definition's and differs from the mutated
    definition's."""
    name, mode, f64, filt, top_ks = MUTANTS[mutant]
    c = case(name)
    if mutant == "nan_shifts_first_touch":
        # The device hands out first-touch keys only for the rows its exact-tie pass re-scored, and the named set has no
        # exact tie: its lists alone cannot tell the shifted keys.  The +inf ties behind a NaN first rating can.
        c = with_nan_first_ratings(case("plus_inf_ties"))
        rows = list(range(N_USERS))
        assert all(expected(c, rows, k, mode, f64, filt)[1] >= 5 for k in top_ks)
        assert all(same(expected(c, rows, k, mode, f64, filt)[0], expected(c, rows, k, mode, f64, filt, mutant=mutant)[0]) for k in top_ks)
    d = Dev(c, f64, forced_tiled=True)
    d.eng.tile_cols = 256
    rows = list(range(N_USERS))
    for k in top_ks:
        got, _n = d.run(rows, k, mode, filt)
        assert d.eng.last_score_path == "tiled"
        what = f"{mutant} on {name} k={k}"
        check_outputs(got, expected(c, rows, k, mode, f64, filt)[0], what, k)
        assert same(got, expected(c, rows, k, mode, f64, filt, mutant=mutant)[0], what), f"{what}: the device gives the mutant's answer"
