"""score_frows_kernel fills an EMPTY list by rank (every lane's best admissible sum takes its rank among the 64, the first
kk are the list) and hands only the sums that are not their lane's best to merge(); a partial list keeps the insertion
path.  The answers must be the oracle's: ids, counts and score bits.

Shapes: the smallest the kernel serves, as in test_gpu_fr_exit (6,000 items, 70 rows of W, 513-row batches), its
builders imported.  On top of that W a handful of RARE rows of W, each with weights on a few light columns only, and
users who rate nothing but such rows: what the first tile that scores anything for them holds is then known column by
column.  The layout sorts the columns of the rarest rows to the front, so a rare row's columns lie side by side in ONE
tile; the weights are handed out along the order the layout gives them (an aligned run of four = one lane
of a 256-column tile, two lanes of a 128-column one).  What each scenario must show in that tile (check_scenarios) is
checked against the host layout and the host model of the first fill before anything runs on the device."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from rtrec_amd.engine import SlimEngine
from rtrec_amd.layouts import build_feature_rows, fr_first_fill_model

from tests.test_gpu_fr_exit import bits, head_tail_w, users

pytestmark = pytest.mark.gpu

TOP_KS = (1, 10, 15)
N_USERS = 1000
COUNTS = (1, 2, 10, 11, 15, 16)          # kk and kk - 1 for every top_k


def rare_rows(W, feat, signed, seed):
    """Adds the rare rows to W.  Returns W, {name: item of the row}, the columns whose sum is zero for the "zero" user.  The layout orders the rows' runs of columns by the
    number of columns (rarest first), so the sizes below place them: [0, 64) the counted rows and a pad nobody rates,
    [64, 128) the three lane rows, from 128 the tie rows (or the signed ones), a second pad up to 256, and in [256, 512)
    the columns that complete a partial list -- no run straddles a tile of 128 or 256 columns."""
    rng = np.random.default_rng(seed)
    n_items = W.shape[0]
    light = np.setdiff1d(np.flatnonzero(np.diff(W.indptr) == 2), feat)       # light columns that are no row of W
    free = np.setdiff1d(np.flatnonzero(np.diff(W.tocsr().indptr) == 0), np.concatenate([feat, light]))
    free = free[free > 100]
    take = iter(rng.permutation(light))
    spec = {}

    def add(name, vals, share=None):
        own = np.sort([next(take) for _ in range(len(vals) - (0 if share is None else len(share)))])[::-1]
        spec[name] = (int(free[len(spec)]), (own if share is None else np.concatenate([share, own])).astype(np.int64), np.asarray(vals, dtype=np.float32))

    def distinct(n):
        return (0.01 + 0.001 * rng.permutation(n)).astype(np.float32)

    for n in COUNTS:                                                         # exactly n columns
        add(f"n{n}", distinct(n))
    add("pad9", distinct(9))
    for m, n in ((2, 20), (3, 21), (4, 23)):                                 # the top m values inside one aligned run of four
        v = distinct(n)
        v[8:8 + m] = 0.05 + 0.001 * np.arange(m)
        add(f"lane{m}", v)
    if not signed:
        v = distinct(24); v[[1, 9, 17]] = 0.05                               # equal scores in different lanes inside the top k
        add("tie_top", v)
        v = np.sort(distinct(25))[::-1].copy()                               # equal scores across k | k + 1 for k = 1, 10, 15
        for k in TOP_KS:
            v[k - 1:k + 2] = v[k - 1]
        add("tie_cut", v[rng.permutation(25)])
    else:
        v = distinct(30); v[5:] *= -1                                        # 5 positive, 25 negative sums
        add("neg", v)
        add("plus", distinct(32))                                            # plus + minus: twelve sums of exactly zero
    add("pad", distinct(66 if signed else 79))
    add("later", (0.0001 + 0.000001 * rng.permutation(256)).astype(np.float32))      # completes a partial list in later tiles
    if signed:                                                               # (the same 32 columns as "plus")
        add("minus", np.concatenate([-spec["plus"][2][:12], 0.5 * distinct(20)]), share=spec["plus"][1])

    def with_rows():
        r_ = np.concatenate([np.full(len(c), it) for it, c, _ in spec.values()])
        c_ = np.concatenate([c for _, c, _ in spec.values()])
        v_ = np.concatenate([v for _, _, v in spec.values()])
        W2 = sp.csc_matrix(W + sp.csc_matrix((v_, (r_, c_)), shape=(n_items, n_items), dtype=np.float32), dtype=np.float32)
        W2.sort_indices()
        return W2

    # Where a row's columns lie is a matter of the PATTERN alone: lay the pattern out, then hand every row's values out
    # along its run in layout order, a lane row's shifted so that its index 8 falls on a multiple of four
    pos = np.asarray(host_layout(with_rows(), 256)["fr_col_map"])
    for name, (item, cols, vals) in list(spec.items()):
        cols = cols[np.argsort(pos[cols])]
        assert len(cols) > 32 or (np.diff(pos[cols]) == 1).all()             # one run (the long rows span tiles)
        if name.startswith("lane"):
            vals = np.roll(vals, int(-pos[cols[0]] % 4))
        spec[name] = (item, cols, vals)
    if signed:
        spec["minus"] = (spec["minus"][0], spec["plus"][1], np.concatenate([-spec["plus"][2][:12], spec["minus"][2][12:]]))
    zero_cols = spec["plus"][1][:12] if signed else np.zeros(0, dtype=np.int64)
    return with_rows(), {k: v[0] for k, v in spec.items()}, zero_cols


def host_layout(W, tc):
    key = (id(W), tc)
    if key not in _layouts:
        cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
        col_map = np.full(W.shape[0], -1, dtype=np.int32)
        col_map[cols] = np.arange(len(cols), dtype=np.int32)
        _layouts[key] = (W, build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=tc))
    return _layouts[key][1]


_layouts = {}


def scenario_users(X, rows, signed):
    """Replaces every 13th user by a constructed one.  Returns X, {user: scenario name}."""
    plan = []
    for n in COUNTS:
        plan += [(f"n{n}", [rows[f"n{n}"]]), (f"n{n}+later", [rows[f"n{n}"], rows["later"]])]
    for name in ("lane2", "lane3", "lane4") + (() if signed else ("tie_top", "tie_cut")):
        plan += [(name, [rows[name]]), (name + "+later", [rows[name], rows["later"]])]
    plan += [("masked", [rows["n16"]])]      # (build() adds the ratings that mask the row's three best columns)
    if signed:
        plan += [("neg", [rows["neg"]]), ("neg+later", [rows["neg"], rows["later"]]), ("zero", [rows["plus"], rows["minus"]]),
                 ("zero+later", [rows["plus"], rows["minus"], rows["later"]])]
    plan += [("no_row", [3, 5]), ("empty", [])]
    X = X.tolil()
    who = {}
    for i, u in enumerate(range(6, N_USERS, 13)):
        name, items = plan[i % len(plan)]
        who[u] = name
        X[u, :] = 0
        for it in items:
            X[u, it] = 2.0
    return X, who


def build(signed):
    W, feat, _ = head_tail_w(seed=31 + signed, signed=bool(signed))
    W, rows, zero_cols = rare_rows(W, feat, signed, seed=33 + signed)
    X = users(N_USERS, W.shape[0], feat, seed=35 + signed, signed=bool(signed), avoid=tuple(rows.values()))
    X, who = scenario_users(X, rows, signed)
    # "masked": the three best columns of row n16 are interacted (their items are no rows of W)
    best3 = np.asarray(W[rows["n16"], :].todense()).ravel().argsort()[::-1][:3]
    for u, name in who.items():
        if name == "masked":
            for it in best3:
                X[u, int(it)] = 1.0
    X = sp.csr_matrix(X.tocsr(), dtype=np.float32)
    X.eliminate_zeros(); X.sort_indices()
    return W, X, who, zero_cols


def first_fill_facts(W, X, u, tc, kk, filt):
    """The first tile of the host layout that holds an admissible non-zero sum for user u, through the host model."""
    L = host_layout(W, tc)
    ids = np.asarray(L["fr_col_ids"])
    n_tiles = int(L["fr_n_tiles"])
    s = np.zeros(n_tiles * tc, dtype=np.float32)
    s[:len(ids)] = np.asarray((X[u] @ W.tocsr()).todense(), dtype=np.float32).ravel()[ids]
    adm = np.ones(n_tiles * tc, dtype=bool)
    if filt:
        adm[:len(ids)] = ~np.isin(ids, X[u].indices)
    ok = (adm & (s != 0)).reshape(n_tiles, tc)
    if not ok.any():
        return None
    t = int(np.flatnonzero(ok.any(axis=1))[0])
    m = fr_first_fill_model(s[t * tc:(t + 1) * tc], adm[t * tc:(t + 1) * tc], kk)
    m.update(tile=t, n_tile=int(ok[t].sum()), n_all=int(ok.sum()), raw_top=np.sort(s[t * tc:(t + 1) * tc])[::-1][:3])
    return m


def check_scenarios(W, X, who, tc, signed):
    """What the constructed users must show in their first scoring tile (host side: layout + model)."""
    by = {}
    for u, name in who.items():
        by.setdefault(name, u)
    for top_k in TOP_KS:
        kk = top_k + 1
        f = first_fill_facts(W, X, by[f"n{kk}"], tc, kk, True)
        assert f["n_tile"] == kk == f["n_all"] and f["values"][kk - 1] > -np.inf            # exactly kk columns
        f = first_fill_facts(W, X, by[f"n{kk - 1}+later"], tc, kk, True)
        assert f["n_tile"] == kk - 1 and f["n_all"] >= kk + 100 and f["values"][kk - 1] == -np.inf      # completed later
    for m in (2, 3, 4):                                                                      # extras: m of the best in one run of four
        f = first_fill_facts(W, X, by[f"lane{m}"], tc, 11, True)
        lanes = f["cols"][:m] // (tc // 64)
        assert f["n_inserted"] >= (m - 1 if tc == 256 else m // 2) and len(set(lanes.tolist())) == (1 if tc == 256 else (m + 1) // 2)
    if not signed:
        f = first_fill_facts(W, X, by["tie_top"], tc, 11, True)
        assert f["values"][0] == f["values"][1] == f["values"][2] > f["values"][3]
        assert len(set((f["cols"][:3] // (tc // 64)).tolist())) == 3                             # equal, in three lanes
        for top_k in TOP_KS:
            f = first_fill_facts(W, X, by["tie_cut"], tc, top_k + 1, True)
            assert f["n_tile"] == 25 and f["values"][top_k - 1] == f["values"][top_k]            # across k | k + 1
    f, g = first_fill_facts(W, X, by["masked"], tc, 11, True), first_fill_facts(W, X, by["masked"], tc, 11, False)
    assert f["n_tile"] == 13 and g["n_tile"] == 16 and f["values"][0] < g["raw_top"][2]      # the mask decides the maxima
    assert first_fill_facts(W, X, by["no_row"], tc, 11, True) is None and X[by["no_row"]].nnz == 2
    assert first_fill_facts(W, X, by["empty"], tc, 11, True) is None and X[by["empty"]].nnz == 0
    if signed:
        f = first_fill_facts(W, X, by["neg"], tc, 11, True)
        assert (f["values"][:5] > 0).all() and (f["values"][5:] < 0).all()
        f = first_fill_facts(W, X, by["zero"], tc, 11, True)
        assert f["n_tile"] == 20 and f["n_ranked"] <= 20                                     # twelve of the 32 sums are zero


class Case:
    """One W and X on the device, one engine per tile width; the oracle's answers are computed once per (rows, top_k,
    filter, mode) and shared by the tile widths and the users-per-wave forms."""

    def __init__(self, oracle, signed):
        self.oracle = oracle
        self.W, self.X, self.who, self.zero_cols = build(signed)
        self.Wr = self.W.tocsr()
        self.eng, self.ref = {}, {}
        for tc in (128, 256):
            check_scenarios(self.W, self.X, self.who, tc, signed)
            e = SlimEngine(device="cuda:0")
            e.FR_TILE_COLS = tc                       # the feature-row layout's tile width (128: the narrow kernels)
            e.set_interactions(None, self.X, need_csc=False)
            e.set_weights(self.W)
            self.eng[tc] = e

    def check(self, tc, uw, n_rows, top_k, filt, dense):
        rows = np.arange(n_rows)
        key = (n_rows, top_k, filt, dense)
        if key not in self.ref:
            self.ref[key] = self.oracle.recommend_batch(self.X[rows], self.Wr, top_k=top_k, filter_interacted=filt, dense=dense)
        o_ids, o_sc, o_cnt = self.ref[key]
        eng = self.eng[tc]
        eng.fr_users_per_wave = uw
        mode = _native.TOPK_DENSE if dense else _native.TOPK_SPARSE
        ids, sc, cnt = eng.recommend_rows(rows, top_k=top_k, filter_interacted=filt, mode=mode)
        assert eng.last_score_path.startswith("feature_rows"), eng.last_score_path
        assert int(eng._layout(True, top_k)["fr_host"]["fr_tile_cols"]) == tc
        assert np.array_equal(cnt, o_cnt)
        assert np.array_equal(ids, o_ids)
        assert np.array_equal(bits(sc), bits(o_sc))
        return ids, sc, cnt


_cases = {}


def get_case(oracle, signed):
    if signed not in _cases:
        _cases[signed] = Case(oracle, signed)
    return _cases[signed]


@pytest.mark.parametrize("uw", [2, 4, 8])
@pytest.mark.parametrize("tc", [128, 256])
@pytest.mark.parametrize("top_k", TOP_KS)
def test_first_fill_forms(oracle, top_k, tc, uw):
    """Every constructed user, filter on and off, SPARSE and DENSE mode."""
    c = get_case(oracle, 0)
    ids, sc, cnt = c.check(tc, uw, N_USERS, top_k, True, False)
    for u, name in c.who.items():                   # SPARSE mode: a user without a rated row of W has no list
        if name in ("no_row", "empty"):
            assert cnt[u] == 0 and (ids[u] == -1).all()
    c.check(tc, uw, 513, top_k, True, True)
    c.check(tc, uw, 513, top_k, False, False)
    c.check(tc, uw, 513, top_k, False, True)


@pytest.mark.parametrize("uw", [2, 4, 8])
@pytest.mark.parametrize("tc", [128, 256])
def test_first_fill_signed(oracle, tc, uw):
    """Signed W and ratings: negative sums in the lists, sums of exactly zero that must not compete."""
    c = get_case(oracle, 1)
    for top_k in (10, 15):
        ids, sc, cnt = c.check(tc, uw, N_USERS, top_k, True, False)
        for u, name in c.who.items():
            if name == "neg":
                assert cnt[u] == top_k and (sc[u, :5] > 0).all() and (sc[u, 5:] < 0).all()
            if name == "zero":            # none of the twelve columns whose sum is zero
                assert cnt[u] == top_k and not np.isin(ids[u], c.zero_cols).any()
    c.check(tc, uw, 513, 10, False, True)
    c.check(tc, uw, 513, 1, False, False)
