"""score_frows_kernel leaves a job once none of its users can open a tile that is still to come (streaming form: the
waves vote at the super-tile hand-over; resident form: each wave on its own).  The skipped work is work whose outcome
was "skip": ids, counts and score bits must equal the oracle's whatever the depth a job ends at.

Shapes.  The smallest W that streams and has a tail worth leaving: 6,000 items, 70 rows of W, two head tiles of 256
columns with ~66 stored rows each (a slice spans two or three 36 KiB super-tiles) and 22 tail tiles of at most 6 rows --
with fewer tail tiles the whole tail is one or two super-tiles and no job could end three short of the end, which case
(a) demands.  Batches of 513, 545 and 1,000 rows: the smallest the feature-row kernel serves, and no multiple of a job."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from rtrec_amd.engine import SlimEngine
from rtrec_amd.layouts import build_feature_rows, fr_exit_model

pytestmark = pytest.mark.gpu

TC = 256
BATCHES = (513, 545, 1000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host_layout(W):
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    return build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=TC)


def head_tail_w(n_items=6000, n_feat=70, n_head=500, seed=0, signed=False, n_tail_rows=6):
    """`n_head` columns with a weight of 0.05-0.3 on ~95 % of the feature rows; every other column two weights of at most
    0.002 on two of `n_tail_rows` rows.  Returns W (csc), the feature items, the tail rows' items."""
    rng = np.random.default_rng(seed)
    feat = np.sort(rng.choice(n_items, n_feat, replace=False))
    cols = rng.permutation(n_items)
    r_, c_, v_ = [], [], []
    for j in cols[:n_head]:
        rows = feat[rng.random(n_feat) < 0.95]
        v = rng.uniform(0.05, 0.3, len(rows)).astype(np.float32)
        r_.append(rows); c_.append(np.full(len(rows), j)); v_.append(np.where(rng.random(len(rows)) < 0.5, -v, v) if signed else v)
    tail_rows = feat[rng.choice(n_feat, n_tail_rows, replace=False)]
    for j in cols[n_head:]:
        rows = rng.choice(tail_rows, 2, replace=False)
        v = rng.uniform(0.0002, 0.002, 2).astype(np.float32)
        r_.append(rows); c_.append(np.full(2, j)); v_.append(-v if signed and rng.random() < 0.5 else v)
    r_, c_, v_ = np.concatenate(r_), np.concatenate(c_), np.concatenate(v_).astype(np.float32)
    keep = r_ != c_
    W = sp.csc_matrix((v_[keep], (r_[keep], c_[keep])), shape=(n_items, n_items))
    W.sort_indices()
    return W, feat, tail_rows


def users(n_users, n_items, feat, seed=1, lo=1, hi=25, signed=False, avoid=()):
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
        vals += (np.where(rng.random(len(its)) < 0.3, -r, r) if signed else r).tolist()
    X = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    return X


def set_row(X, u, items, ratings):
    X = X.tolil()
    X[u, :] = 0
    for i, r in zip(items, ratings):
        X[u, int(i)] = r
    X = X.tocsr().astype(np.float32)
    X.eliminate_zeros(); X.sort_indices()
    return X


class Case:
    """One W and X on the device; the oracle's answers are computed once per (rows, top_k, filter, mode) and shared by the
    three users-per-wave forms."""

    def __init__(self, oracle, W, X, resident=False):
        self.oracle, self.W, self.X, self.resident = oracle, W, X, resident
        self.Wr = W.tocsr()
        self.eng = SlimEngine(device="cuda:0", tile_cols=TC)
        self.eng.set_interactions(None, X, need_csc=False)
        self.eng.set_weights(W)
        self.ref = {}

    def check(self, uw, rows, top_k=10, filt=True, dense=False):
        rows = np.asarray(rows)
        key = (rows.tobytes(), top_k, filt, dense)
        if key not in self.ref:
            self.ref[key] = self.oracle.recommend_batch(self.X[rows], self.Wr, top_k=top_k, filter_interacted=filt, dense=dense)
        o_ids, o_sc, o_cnt = self.ref[key]
        self.eng.fr_users_per_wave = uw
        mode = _native.TOPK_DENSE if dense else _native.TOPK_SPARSE
        ids, sc, cnt = self.eng.recommend_rows(rows, top_k=top_k, filter_interacted=filt, mode=mode)
        assert self.eng.last_score_path.startswith("feature_rows"), self.eng.last_score_path
        lay = self.eng._layout(True, top_k)
        assert bool(lay["fr_host"]["fr_resident"]) == self.resident
        assert np.array_equal(cnt, o_cnt)
        assert np.array_equal(ids, o_ids)
        assert np.array_equal(bits(sc), bits(o_sc))
        return ids, sc, cnt


_cases = {}


def get_case(name, oracle):
    if name not in _cases:
        _cases[name] = BUILDERS[name](oracle)
    return _cases[name]


# ---------------------------------------------------------------------------------------------- the cases' models
def build_head_tail(oracle):
    W, feat, _ = head_tail_w()
    X = users(1000, W.shape[0], feat)
    c = Case(oracle, W, X)
    c.L = host_layout(W)
    c.model = fr_exit_model(c.L, W, X, 10)
    return c


def spike_model(where):
    """(b): one tail tile -- the partial last tile (`where` = "last"), or the middle one of the full tail tiles -- holds one
    column with weight 0.5 on a tail row that exactly one user rates.  The layout cuts tiles from the columns' row PATTERNS and
    orders the full tiles by their weight mass: the spike replaces a stored weight (same pattern, same tile), and for the
    middle tile the tile's other weights shrink so that its mass, hence its place in the order, stays what it was."""
    W, feat, tail_rows = head_tail_w(seed=5)
    L0 = host_layout(W)
    pos = np.asarray(L0["fr_col_map"])
    n_cols, n_tiles = len(L0["fr_col_ids"]), L0["fr_n_tiles"]
    tile_of_item = np.where(pos >= 0, pos // TC, -1)
    M = W.tolil()
    rows_of_tile = np.asarray(L0["fr_rows_of_tile"]).view(np.uint64).reshape(-1, 2)
    n_rows_t = np.array([bin(int(a)).count("1") + bin(int(b)).count("1") for a, b in rows_of_tile])
    tail_tiles = np.flatnonzero(n_rows_t <= 6)
    assert len(tail_tiles) >= 15 and n_cols % TC != 0
    t_star = n_tiles - 1 if where == "last" else int(tail_tiles[len(tail_tiles) // 2])
    Wc = W.tocsc()
    j_star = int(np.setdiff1d(np.flatnonzero(tile_of_item == t_star), feat)[0])
    r_star = int(Wc[:, j_star].indices[0])
    if where != "last":
        items = np.flatnonzero(tile_of_item == t_star)
        sub = abs(Wc[:, items])
        mass, n_w = float(sub.sum()), int(sub.nnz)
        scale = (mass - 0.5) / (mass - abs(float(Wc[r_star, j_star])))
        assert 0 < scale < 1
        for j in items:
            for r in Wc[:, j].indices:
                M[int(r), int(j)] = np.float32(M[int(r), int(j)] * scale)
    M[r_star, j_star] = np.float32(0.5)
    W2 = sp.csc_matrix(M.tocsc(), dtype=np.float32)
    W2.sort_indices()
    X = users(1000, W.shape[0], feat, seed=6, avoid=(r_star,))
    head_row = int(np.setdiff1d(feat, tail_rows)[0])
    u_star = 700
    X = set_row(X, u_star, [r_star, head_row], [5.0, 1.0])
    return W2, X, u_star, j_star, r_star


def build_spike(where):
    def build(oracle):
        W, X, u_star, j_star, _ = spike_model(where)
        c = Case(oracle, W, X)
        c.L = host_layout(W)
        c.model = fr_exit_model(c.L, W, X, 10)
        c.u_star, c.j_star = u_star, j_star
        return c
    return build


def build_one_heavy(oracle):
    W, feat, _ = head_tail_w(seed=7)
    X = users(1000, W.shape[0], feat, seed=8, lo=1, hi=3)
    for u in (17, 530, 999):                                    # one heavy user in a job of light ones
        X = set_row(X, u, feat, 5.0 - 0.25 * np.random.default_rng(u).random(len(feat)).astype(np.float32))
    return Case(oracle, W, X)


def build_never_fill(oracle):
    """Two rare rows of W: three columns hold a weight of the first, one column of the second.  Users who rate only such a
    row score fewer than top_k + 1 columns: their lists never fill and their jobs run to the end of W."""
    W, feat, _ = head_tail_w(seed=9)
    rare = np.setdiff1d(np.arange(W.shape[0]), feat)[[10, 2000]]
    M = W.tolil()
    for j, w in ((40, 0.001), (2500, 0.0015), (5100, 0.0008)):
        M[int(rare[0]), j] = np.float32(w)
    M[int(rare[1]), 3333] = np.float32(0.0012)
    W = sp.csc_matrix(M.tocsc(), dtype=np.float32)
    W.sort_indices()
    X = users(1000, W.shape[0], feat, seed=10, avoid=tuple(rare))
    for u in range(3, 1000, 37):
        X = set_row(X, u, [rare[u % 2], (u * 7) % 6000 if (u * 7) % 6000 not in feat else 1], [4.0, 2.0])
    X = set_row(X, 998, [rare[0], rare[1]], [1.0, 3.0])
    return Case(oracle, W, X)


def build_signed(oracle):
    """(e): signed W and ratings; and a rare row of W with 5 positive and 15 negative weights -- a user who rates only that
    row has a NEGATIVE (k+1)-th best: its list is full, yet the test with a bound can never close it."""
    W, feat, _ = head_tail_w(seed=11, signed=True)
    rare = int(np.setdiff1d(np.arange(W.shape[0]), feat)[77])
    M = W.tolil()
    for i, j in enumerate(range(100, 6000, 300)):
        M[rare, j if j != rare else j + 1] = np.float32((0.001 + 0.00003 * i) * (1 if i < 5 else -1))
    W = sp.csc_matrix(M.tocsc(), dtype=np.float32)
    W.sort_indices()
    X = users(1000, W.shape[0], feat, seed=12, signed=True, avoid=(rare,))
    for u in range(5, 1000, 41):
        X = set_row(X, u, [rare], [3.0])
    return Case(oracle, W, X)


def build_tall(oracle):
    """(f): 110 rows of W -- the first head tile stores 100+ rows, a slice of three or more super-tiles that every wave opens
    at its first fragment; the thresholds rise while it is swept."""
    W, feat, _ = head_tail_w(n_feat=110, n_head=300, seed=13)
    X = users(1000, W.shape[0], feat, seed=14, hi=40)
    c = Case(oracle, W, X)
    c.L = host_layout(W)
    return c


def build_empty_rows(oracle):
    W, feat, _ = head_tail_w(seed=15)
    X = users(1000, W.shape[0], feat, seed=16)
    nonfeat = np.setdiff1d(np.arange(W.shape[0]), feat)
    for u in range(980, 1000):                                  # the last job: empty rows, rows without a feature item
        X = set_row(X, u, [] if u % 2 else nonfeat[[u, u + 50]], [] if u % 2 else [3.0, 1.0])
    for u in (0, 511, 512, 544):
        X = set_row(X, u, [], [])
    return Case(oracle, W, X)


def build_resident(oracle):
    W, feat, _ = head_tail_w(n_items=800, n_feat=70, n_head=200, seed=17)
    X = users(1000, W.shape[0], feat, seed=18)
    c = Case(oracle, W, X, resident=True)
    c.L = host_layout(W)
    return c


def build_ties(oracle):
    """(i): every column a copy of one of 60 (a tenth of them head columns): exact ties inside the lists, at their thresholds,
    and between columns on either side of the point where a job leaves."""
    W, feat, _ = head_tail_w(seed=19)
    rng = np.random.default_rng(20)
    src = np.concatenate([np.flatnonzero(np.diff(W.indptr) > 20)[:6], np.flatnonzero(np.diff(W.indptr) == 2)[:54]])
    pick = np.where(rng.random(W.shape[0]) < 0.1, rng.choice(src[:6], W.shape[0]), rng.choice(src[6:], W.shape[0]))
    Wt = sp.csc_matrix(W[:, pick])
    Wt.sort_indices()
    X = users(1000, W.shape[0], feat, seed=21)
    return Case(oracle, Wt, X)


BUILDERS = {"head_tail": build_head_tail, "spike_last": build_spike("last"), "spike_middle": build_spike("middle"),
            "one_heavy": build_one_heavy, "never_fill": build_never_fill, "signed": build_signed, "tall": build_tall,
            "empty_rows": build_empty_rows, "resident": build_resident, "ties": build_ties}

UW = pytest.mark.parametrize("uw", [2, 4, 8])


# ---------------------------------------------------------------------------------------------------------- the tests
@UW
def test_a_heavy_head_light_tail(oracle, uw):
    """Precondition from the host model: no job needs the last three super-tiles -- the early path really runs."""
    c = get_case("head_tail", oracle)
    n_super = c.model["n_super"]
    assert c.L["fr_n_super"] == n_super >= 7
    assert int(c.model["depth_open"].max()) <= n_super - 3
    for n in BATCHES:
        c.check(uw, np.arange(n))
    c.check(uw, np.arange(1000), filt=False)


@UW
@pytest.mark.parametrize("where", ["last", "middle"])
def test_b_late_spike(oracle, uw, where):
    """The spike's column tops the list of the one user who rates its row: no job with that user may leave before it."""
    c = get_case("spike_" + where, oracle)
    m, u = c.model, c.u_star
    t_star = int(np.asarray(c.L["fr_col_map"])[c.j_star]) // TC
    s_star = int(m["last_super"][t_star])
    # (the suffix bound is a constant of W: the spike's 0.5 holds EVERY user with a rating open up to its tile; behind it
    # the bound drops to the tail's and the jobs leave)
    assert int(m["depth"][u]) >= s_star + 1 and int(m["depth"][m["l1"] > 0].min()) >= s_star + 1
    if where == "last":
        assert s_star == m["n_super"] - 1
    else:
        assert 4 <= s_star < m["n_super"] - 1 and int(m["depth_open"].max()) == s_star + 1
    for n in (1000, 713):
        ids, _, _ = c.check(uw, np.arange(n))
        assert ids[u, 0] == c.j_star


@UW
def test_c_one_heavy_user_in_a_job(oracle, uw):
    c = get_case("one_heavy", oracle)
    for n in BATCHES:
        c.check(uw, np.arange(n))


@UW
@pytest.mark.parametrize("top_k", [1, 10, 15])
def test_d_lists_that_never_fill(oracle, uw, top_k):
    c = get_case("never_fill", oracle)
    _, _, cnt = c.check(uw, np.arange(1000), top_k=top_k)
    assert (cnt[3::37] <= min(top_k, 3)).all() and cnt[998] <= min(top_k, 4)      # short lists, -1 / -inf behind them
    c.check(uw, np.arange(545), top_k=top_k, filt=False)


@UW
def test_e_signed_w(oracle, uw):
    c = get_case("signed", oracle)
    ids, sc, cnt = c.check(uw, np.arange(1000))
    assert (cnt[5::41] == 10).all() and (sc[5::41, 9] < 0).all()                 # negative scores in full lists
    c.check(uw, np.arange(513), top_k=15, filt=False)


@UW
def test_f_tall_tile_across_three_super_tiles(oracle, uw):
    c = get_case("tall", oracle)
    ft = np.asarray(c.L["fr_frag_tile"])
    assert c.L["fr_rows"] > 100 and (ft & 0xFFFFFF == 0).sum() >= 3 and int(np.asarray(c.L["fr_super_tile"])[3]) <= 3
    for n in (1000, 545):
        c.check(uw, np.arange(n))


@UW
def test_g_empty_rows_in_the_last_job(oracle, uw):
    """Empty rows and rows without a feature item, alone in the last job and scattered; a row id outside X never reaches
    the kernel (IndexError, like the reference's scipy indexing)."""
    c = get_case("empty_rows", oracle)
    for n in (1000, 545, 513):
        _, _, cnt = c.check(uw, np.arange(n))
    assert cnt[0] == 0 and cnt[512] == 0
    c.check(uw, np.concatenate([np.arange(600), np.arange(980, 1000)]))
    with pytest.raises(IndexError):
        c.eng.recommend_rows(np.array([5, 1000]), top_k=10)


@UW
def test_h_resident_form(oracle, uw):
    c = get_case("resident", oracle)
    assert c.L["fr_n_super"] == 1 and c.L["fr_n_tiles"] >= 3
    for n in BATCHES:
        c.check(uw, np.arange(n))
    c.check(uw, np.arange(1000), top_k=15, filt=False)


@UW
def test_i_ties_across_the_exit_point(oracle, uw):
    c = get_case("ties", oracle)
    for n in (1000, 513):
        for filt in (True, False):
            c.check(uw, np.arange(n), filt=filt)


@UW
def test_j_dense_mode_through_the_fast_pass(oracle, uw):
    c = get_case("head_tail", oracle)
    c.check(uw, np.arange(545), dense=True)
    c = get_case("never_fill", oracle)
    c.check(uw, np.arange(1000), dense=True)
    c = get_case("resident", oracle)
    c.check(uw, np.arange(513), dense=True)
