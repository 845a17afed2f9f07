"""score_frows_kernel ranks an EMPTY list's first fill over STRIDED groups (group g = register r of the lane 64 / REGS * r
below g) in every form but the two 8-user forms of 256-column tiles: <4,2,8> (65+ rows of W) still fills by insertion
and <4,1,8> (up to 64 rows) ranks lanes.  What merge() still gets are the sums above the new kk-th entry that are not
their group's largest.  The answers must be the oracle's: ids, counts, score bits.

Shapes: 6,000 items, 1,000 users, 513-row batches (the smallest the kernel serves, as in test_gpu_fr_exit, whose
builders are copied below), once with 40 + 18 rows of W (one 64-row word) and once with 70 + 18 (two).  On top of that W a
handful of RARE rows, each with weights on light columns only, and users who rate nothing but such rows: what their
first scoring tile holds is then known column by column.  The layout lays a rare row's columns side by side; the
short rows and two pads nobody rates add up to 512 columns, so that every 256-column row starts a tile of either width
(asserted).  Its values are handed out BY STRIDED GROUP of the tile width under test
(one W per width), and what each scenario must show in that tile is checked against the host layout and the host model
of the first fill (check_scenarios) before anything runs on the device."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from rtrec_amd import _native
from rtrec_amd.engine import SlimEngine
from rtrec_amd.layouts import build_feature_rows, fr_fill_group_columns, fr_first_fill_model

pytestmark = pytest.mark.gpu

TOP_KS = (1, 10, 15)
N_USERS = 1000
COUNTS = (1, 2, 10, 11, 15, 16)          # kk and kk - 1 for every top_k
N_FEATS = (40, 70)                       # + 18 rare rows: one and two 64-row words of W
BIG = 256


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def head_tail_w(n_items=6000, n_feat=70, n_head=500, seed=0, n_tail_rows=6):
    """`n_head` columns with a weight of 0.05-0.3 on ~95 % of the feature rows; every other column two weights of at most
    0.002 on two of `n_tail_rows` rows.  Returns W (csc), the feature items, the tail rows' items."""
    rng = np.random.default_rng(seed)
    feat = np.sort(rng.choice(n_items, n_feat, replace=False))
    cols = rng.permutation(n_items)
    r_, c_, v_ = [], [], []
    for j in cols[:n_head]:
        rows = feat[rng.random(n_feat) < 0.95]
        r_.append(rows); c_.append(np.full(len(rows), j)); v_.append(rng.uniform(0.05, 0.3, len(rows)).astype(np.float32))
    tail_rows = feat[rng.choice(n_feat, n_tail_rows, replace=False)]
    for j in cols[n_head:]:
        rows = rng.choice(tail_rows, 2, replace=False)
        r_.append(rows); c_.append(np.full(2, j)); v_.append(rng.uniform(0.0002, 0.002, 2).astype(np.float32))
    r_, c_, v_ = np.concatenate(r_), np.concatenate(c_), np.concatenate(v_).astype(np.float32)
    keep = r_ != c_
    W = sp.csc_matrix((v_[keep], (r_[keep], c_[keep])), shape=(n_items, n_items))
    W.sort_indices()
    return W, feat, tail_rows


def users(n_users, n_items, feat, seed=1, lo=1, hi=25, avoid=()):
    """Users with lo..hi-1 ratings (1-5) of feature items and up to 30 of other items; nobody rates an item of `avoid`."""
    rng = np.random.default_rng(seed)
    ok_feat = np.setdiff1d(feat, avoid)
    rows, cols, vals = [], [], []
    for u in range(n_users):
        own = rng.choice(ok_feat, int(rng.integers(lo, hi)), replace=False)
        other = np.setdiff1d(rng.choice(n_items, int(rng.integers(0, 30)), replace=False), avoid)
        its = np.unique(np.concatenate([own, other])).astype(np.int64)
        r = rng.integers(1, 6, len(its)).astype(np.float32)
        rows += [u] * len(its); cols += its.tolist()
        vals += r.tolist()
    X = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    return X


def host_layout(W, tc):
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    return build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=tc)


def group_of(local, tc):
    """Strided group of a tile-local column."""
    regs = tc // 64
    where = np.empty(tc, dtype=np.int64)
    where[fr_fill_group_columns(regs, True).ravel()] = np.repeat(np.arange(64), regs)
    return where[local]


def rare_rows(W, feat, tc, seed):
    """Adds the rare rows to W.  Returns W, {name: item of the row}, the columns whose sum is zero for the "zero" user."""
    rng = np.random.default_rng(seed)
    n_items = W.shape[0]
    light = np.setdiff1d(np.flatnonzero(np.diff(W.indptr) == 2), feat)       # light columns that are no row of W
    free = np.setdiff1d(np.flatnonzero(np.diff(W.tocsr().indptr) == 0), np.concatenate([feat, light]))
    free = free[free > 100]
    take = iter(rng.permutation(light))
    spec = {}

    def add(name, n, share=None):
        own = np.array([next(take) for _ in range(n)] if share is None else share, dtype=np.int64)
        spec[name] = [int(free[len(spec)]), own, None]

    for n in COUNTS:                                                         # exactly n columns
        add(f"n{n}", n)
    add("tie_cut", 25)
    add("neg", 30)
    add("plus", 32)
    add("run", 40)
    short = sum(COUNTS) + 25 + 30 + 32 + 40
    pad = 2 * BIG - short                                                    # two pads of different sizes, both above 40
    add("pad_a", pad // 2 - 7)
    add("pad_b", pad - (pad // 2 - 7))
    for name in ("share2", "share3", "share4", "tie_in"):
        add(name, BIG)
    add("later", 2 * BIG)                                                    # completes a partial list in later tiles
    add("minus", 32, share=spec["plus"][1])                                  # (the same 32 columns as "plus")

    def with_rows(fill):
        r_ = np.concatenate([np.full(len(c), it) for it, c, _ in spec.values()])
        c_ = np.concatenate([c for _, c, _ in spec.values()])
        v_ = np.concatenate([np.full(len(c), 1.0, np.float32) if fill else v for _, c, v in spec.values()])
        W2 = sp.csc_matrix(W + sp.csc_matrix((v_, (r_, c_)), shape=(n_items, n_items), dtype=np.float32), dtype=np.float32)
        W2.sort_indices()
        return W2

    def distinct(n, lo=0.01, step=0.0001):
        return (lo + step * rng.permutation(n)).astype(np.float32)

    # Where a row's columns lie is a matter of the PATTERN alone: lay the pattern out, then hand the values out by position
    pos = np.asarray(host_layout(with_rows(True), tc)["fr_col_map"])
    for name, (item, cols, _) in spec.items():
        cols = cols[np.argsort(pos[cols])]
        p = pos[cols]
        n = len(cols)
        assert n > 40 or (np.diff(p) == 1).all(), name                       # one run (the long rows span tiles)
        spec[name][1] = cols
        v = distinct(n)
        first = np.flatnonzero(p // tc == p[0] // tc)                        # the row's columns in its first tile
        grp = group_of(p[first] % tc, tc)
        if n == BIG:
            assert len(first) == tc, (name, p[0])                            # a whole tile of the row's own
            v[np.setdiff1d(np.arange(n), first)] *= 0.5                      # ... and the heavier of its tiles: visited first
            members = [first[grp == g] for g in range(64)]                   # tc // 64 columns of the run per group
        if name == "tie_cut":                                                # equal sums across k | k + 1 for k = 1, 10, 15
            v = np.sort(v)[::-1].copy()
            for k in TOP_KS:
                v[k - 1:k + 2] = v[k - 1]
            v = v[rng.permutation(n)]
        elif name == "later":                                                # the lightest tiles: visited behind all the others
            v = distinct(n, 0.0001, 0.000001)
        elif name == "neg":                                                  # 5 positive, 25 negative sums
            v[5:] *= -1
        elif name == "run":                                                  # 16 strong neighbours in the middle of the run
            v[12:28] = 0.05 + 0.001 * rng.permutation(16)
        elif name.startswith("share"):                                       # the top m sums in as few groups as the width allows
            m, chosen, g = int(name[5:]), [], 20
            while len(chosen) < m:
                chosen += members[g][:m - len(chosen)].tolist()
                g += 1
            v[chosen] = 0.05 + 0.001 * rng.permutation(m)
        elif name == "tie_in":                                               # equal sums inside one group and in two more groups
            v[members[7][:2]] = 0.05
            v[members[30][0]] = 0.05
            v[members[31][0]] = 0.05
        spec[name][2] = v.astype(np.float32)
    plus_v = spec["plus"][2]
    spec["minus"][2] = np.concatenate([-plus_v[:12], 0.5 * plus_v[12:]]).astype(np.float32)
    zero_cols = spec["plus"][1][:12]
    return with_rows(False), {k: v[0] for k, v in spec.items()}, zero_cols, {k: v[1] for k, v in spec.items()}


def scenario_users(X, rows):
    """Replaces every 13th user by a constructed one.  Returns X, {user: scenario name}."""
    plan = []
    for n in COUNTS:
        plan += [(f"n{n}", [rows[f"n{n}"]]), (f"n{n}+later", [rows[f"n{n}"], rows["later"]])]
    for name in ("run", "share2", "share3", "share4", "tie_in", "tie_cut", "neg"):
        plan += [(name, [rows[name]]), (name + "+later", [rows[name], rows["later"]])]
    plan += [("masked", [rows["share2"]]),   # (build() adds the rating that masks the row's best column)
             ("zero", [rows["plus"], rows["minus"]]), ("zero+later", [rows["plus"], rows["minus"], rows["later"]]),
             ("late_only", [rows["later"]]), ("no_row", [3, 5]), ("empty", [])]
    X = X.tolil()
    who = {}
    for i, u in enumerate(range(6, N_USERS, 13)):
        name, items = plan[i % len(plan)]
        who[u] = name
        X[u, :] = 0
        for it in items:
            X[u, it] = 2.0
    return X, who


def build(n_feat, tc):
    W, feat, _ = head_tail_w(n_feat=n_feat, n_head=2 * BIG, seed=41 + n_feat)      # (the head: two tiles of its own)
    W, rows, zero_cols, row_cols = rare_rows(W, feat, tc, seed=43 + n_feat)
    X = users(N_USERS, W.shape[0], feat, seed=45 + n_feat, avoid=tuple(rows.values()))
    X, who = scenario_users(X, rows)
    # "masked": the best column of row share2 is interacted (its item is no row of W): the group's second sum is ranked
    best = int(np.asarray(W[rows["share2"], :].todense()).ravel().argmax())
    # "late_only": the first tile of row "later" is interacted as a whole: the list fills from the tile behind it
    pos = np.asarray(host_layout(W, tc)["fr_col_map"])
    lc = row_cols["later"]
    first_later = lc[pos[lc] // tc == pos[lc[0]] // tc]
    for u, name in who.items():
        if name == "masked":
            X[u, best] = 1.0
        if name == "late_only":
            for it in first_later:
                X[u, int(it)] = 1.0
    X = sp.csr_matrix(X.tocsr(), dtype=np.float32)
    X.eliminate_zeros(); X.sort_indices()
    assert len(np.flatnonzero(np.diff(W.tocsr().indptr) > 0)) <= (64 if n_feat == 40 else 128)
    return W, X, who, zero_cols


def first_fill_facts(L, W, X, u, tc, kk, filt, strided=True):
    """The first tile of the host layout that holds an admissible non-zero sum for user u, through the host model."""
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
    m = fr_first_fill_model(s[t * tc:(t + 1) * tc], adm[t * tc:(t + 1) * tc], kk, strided=strided)
    raw = s[t * tc:(t + 1) * tc]
    m.update(tile=t, n_tile=int(ok[t].sum()), n_all=int(ok.sum()), raw_argmax=int(raw.argmax()), raw_nonzero=int((raw != 0).sum()),
             groups=group_of(np.maximum(m["cols"], 0), tc))
    return m


def check_scenarios(W, X, who, tc):
    """What the constructed users must show in their first scoring tile (host side: layout + model)."""
    L = host_layout(W, tc)
    regs = tc // 64
    by = {}
    for u, name in who.items():
        by.setdefault(name, u)

    def facts(name, kk=11, filt=True, strided=True):
        return first_fill_facts(L, W, X, by[name], tc, kk, filt, strided)

    for top_k in TOP_KS:
        kk = top_k + 1
        f = facts(f"n{kk}", kk)                     # exactly kk neighbouring columns: kk groups, nothing for merge()
        assert f["n_tile"] == kk == f["n_all"] == f["n_ranked"] and f["n_extras"] == 0 and f["values"][kk - 1] > -np.inf
        f = facts(f"n{kk - 1}+later", kk)           # fewer than kk groups hold a sum: completed from later tiles
        assert f["n_tile"] == kk - 1 == f["n_ranked"] and f["n_all"] >= kk + 100 and f["values"][kk - 1] == -np.inf
        f = facts("tie_cut", kk)
        assert f["n_tile"] == 25 and f["values"][top_k - 1] == f["values"][top_k]               # across k | k + 1
    f, fl = facts("run"), facts("run", strided=False)   # 16 strong neighbours: 16 groups; the lanes leave most of them to merge()
    assert f["n_extras"] == 0 and len(set(f["groups"].tolist())) == 11 and fl["n_extras"] >= 16 - 16 // regs - 1
    assert (f["values"] >= np.float32(0.1)).all() and np.array_equal(f["values"], fl["values"])
    for m in (2, 3, 4):                             # the m best sums in ceil(m / regs) groups: the rest of them are extras
        f = facts(f"share{m}")
        n_groups = -(-m // regs)
        assert len(set(f["groups"][:m].tolist())) == n_groups and f["n_inserted"] >= m - n_groups and (f["values"][:m] >= np.float32(0.1)).all()
    f = facts("tie_in")                             # four equal sums, two of them in one group
    assert (f["values"][:4] == f["values"][0]).all() and f["values"][4] < f["values"][0] and len(set(f["groups"][:4].tolist())) == 3
    f, g = facts("masked"), facts("masked", filt=False)      # the interacted column is its group's (and the tile's) largest sum
    assert f["n_tile"] == g["n_tile"] - 1 and g["cols"][0] == g["raw_argmax"] and g["raw_argmax"] not in f["cols"]
    assert group_of(g["raw_argmax"], tc) == f["groups"][0] and f["n_extras"] == g["n_extras"] - 1      # (the group's second sum: ranked now)
    f = facts("neg")
    assert (f["values"][:5] > 0).all() and (f["values"][5:] < 0).all()
    f = facts("zero")
    assert f["n_all"] == 20 and f["n_tile"] == f["raw_nonzero"]                                # twelve of the 32 sums are zero
    f, g = facts("late_only"), facts("late_only", filt=False)    # no admissible sum in the first tile the user scores in
    assert f["tile"] > g["tile"] and f["values"][10] > -np.inf
    assert facts("no_row") is None and X[by["no_row"]].nnz == 2
    assert facts("empty") is None and X[by["empty"]].nnz == 0


class Case:
    """One W and X on the device for one tile width; the oracle's answers are computed once per (rows, top_k, filter,
    mode) and shared by the users-per-wave forms."""

    def __init__(self, oracle, n_feat, tc):
        self.oracle, self.tc = oracle, tc
        self.W, self.X, self.who, self.zero_cols = build(n_feat, tc)
        check_scenarios(self.W, self.X, self.who, tc)
        self.Wr = self.W.tocsr()
        self.ref = {}
        self.eng = SlimEngine(device="cuda:0")
        self.eng.FR_TILE_COLS = tc                    # the feature-row layout's tile width (128: the narrow kernels)
        self.eng.set_interactions(None, self.X, need_csc=False)
        self.eng.set_weights(self.W)
        self.eng.rescored = torch.zeros(1, dtype=torch.int32, device="cuda:0")      # rows the exact-tie pass re-scored, per call

    def check(self, uw, n_rows, top_k, filt, dense):
        rows = np.arange(n_rows)
        key = (n_rows, top_k, filt, dense)
        if key not in self.ref:
            self.ref[key] = self.oracle.recommend_batch(self.X[rows], self.Wr, top_k=top_k, filter_interacted=filt, dense=dense)
        o_ids, o_sc, o_cnt = self.ref[key]
        eng = self.eng
        eng.fr_users_per_wave = uw
        mode = _native.TOPK_DENSE if dense else _native.TOPK_SPARSE
        ids, sc, cnt = eng.recommend_rows(rows, top_k=top_k, filter_interacted=filt, mode=mode)
        assert eng.last_score_path.startswith("feature_rows"), eng.last_score_path
        assert int(eng._layout(True, top_k)["fr_host"]["fr_tile_cols"]) == self.tc
        assert np.array_equal(cnt, o_cnt)
        assert np.array_equal(ids, o_ids)
        assert np.array_equal(bits(sc), bits(o_sc))
        return ids, sc, cnt, int(eng.rescored.item())


_cases = {}


def get_case(oracle, n_feat, tc):
    if (n_feat, tc) not in _cases:
        _cases[(n_feat, tc)] = Case(oracle, n_feat, tc)
    return _cases[(n_feat, tc)]


def run_forms(oracle, n_feat, tc, uw, top_k):
    c = get_case(oracle, n_feat, tc)
    ids, sc, cnt, n_rescored = c.check(uw, N_USERS, top_k, True, False)
    # equal sums across k | k + 1: every such row went through the exact-tie pass (and came back the oracle's, see check)
    assert n_rescored >= sum(name.startswith("tie_cut") for name in c.who.values()) > 0
    for u, name in c.who.items():
        if name in ("no_row", "empty"):             # SPARSE mode: a user without a rated row of W has no list
            assert cnt[u] == 0 and (ids[u] == -1).all()
        if name == "neg" and top_k >= 10:
            assert cnt[u] == top_k and (sc[u, :5] > 0).all() and (sc[u, 5:] < 0).all()
        if name == "zero":                          # none of the twelve columns whose sum is zero
            assert cnt[u] == min(top_k, 20) and not np.isin(ids[u], c.zero_cols).any()
    c.check(uw, 513, top_k, True, True)
    c.check(uw, 513, top_k, False, False)
    c.check(uw, 513, top_k, False, True)


@pytest.mark.parametrize("uw", [2, 4])
@pytest.mark.parametrize("tc", [128, 256])
@pytest.mark.parametrize("n_feat", N_FEATS)
@pytest.mark.parametrize("top_k", TOP_KS)
def test_fill_groups_forms(oracle, top_k, n_feat, tc, uw):
    """Every constructed user, filter on and off, SPARSE and DENSE mode, in the 2- and 4-user forms."""
    run_forms(oracle, n_feat, tc, uw, top_k)


@pytest.mark.parametrize("tc", [128, 256])
@pytest.mark.parametrize("n_feat", N_FEATS)
def test_eight_user_form(oracle, n_feat, tc):
    """The 8-user forms: <4,2,8> (70 + 18 rows, 256 columns) fills by insertion, <4,1,8> (40 + 18 rows) ranks lanes, <2,2,8> and
    <2,1,8> rank strided groups; the same answers."""
    run_forms(oracle, n_feat, tc, 8, 10)
