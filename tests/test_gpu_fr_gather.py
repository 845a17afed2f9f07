"""score_frows_kernel keeps the leading super-tiles of W resident in LDS (the head) and, behind them, every wave fetches
the rows it sweeps into a ring of its own (D = 4 LDS-DMA instructions of 1 KiB: four rows of a 256-column tile, eight of a
128-column one).  Wherever the head ends, and whatever the ring has to carry, ids, counts and score bits equal the
oracle's.

Shapes.  W is built from GROUPS of 256 columns that share one row pattern, so that the layout's tiles are exactly the
groups (it sorts the columns by pattern and cuts every 256 / 128): two heavy groups on nearly every feature row (the tall
tiles, visited first: 106 of 110 rows -- a slice of three or more fragments -- or 46 of 50), groups of D-1, D, D+1, 2D and
2D+1 = 3, 4, 5, 8, 9 rows (the ring's wrap-around; odd and even counts for the two-rows-per-instruction path of the
128-column tiles) and 17 two-row groups: 24 tiles of 256 columns, 6,144 columns, 110 rows (two ratings registers per
user) or 50 (one).  Users: the random users of tests/test_gpu_fr_exit.py, and SWEEPERS who rate every item but 15, one
in each of 15 tiles: with filter_interacted their lists never fill (top_k 15), so they open every tile, need every stored
row of it -- every step of the ring -- and show one score of every tile they were given.  Batches of 513, 545 and 1,000
rows: the smallest the feature-row kernel serves, and no multiple of a job.

A W of more than 64 narrow tiles that fits the head whole (FLAT below) gives the last boundary: a head of all but the
last super-tile, and a head of several super-tiles with nothing to gather.

Mutants these tests are meant to catch (csrc/score.hip): the counted vmcnt wait one too lax, the lgkmcnt wait before a
refill dropped, `in_head` off by one fragment."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native
from rtrec_amd.engine import SlimEngine
from rtrec_amd.layouts import build_feature_rows

from .test_gpu_fr_exit import bits, set_row, users

pytestmark = pytest.mark.gpu

RING = 4                                    # kFrRingDepth of csrc/score.hip
COUNTS = (RING - 1, RING, RING + 1, 2 * RING, 2 * RING + 1)
HEAD_MAX_KIB = 84                           # what 160 KiB leave beside 16 waves' rings, candidate buffers and tables
N_TAIL = 17
GROUP = 256
UW = pytest.mark.parametrize("uw", [2, 4, 8])


def grouped_w(n_feat, seed=0, spec=None):
    """W of groups of 256 columns, (rows, lowest, highest weight) each -- by default 2 + 5 + N_TAIL groups: two tall, the
    five ring counts, the two-row tail; the feature items hold no column of their own, so every column of a group has
    exactly the group's rows.  Returns W (csc), the feature items, per group its columns."""
    rng = np.random.default_rng(seed)
    if spec is None:
        spec = [(n_feat - 4, 0.05, 0.3)] * 2 + [(c, 0.0005, 0.002) for c in COUNTS] + [(2, 0.0002, 0.001)] * N_TAIL
    n_cols = GROUP * len(spec)
    n_items = n_cols + n_feat
    feat = np.sort(rng.choice(n_items, n_feat, replace=False))
    cols = rng.permutation(np.setdiff1d(np.arange(n_items), feat))
    pats, r_, c_, v_, groups = set(), [], [], [], []

    def add(group_cols, n_rows, lo, hi):
        while True:
            rows = np.sort(rng.choice(feat, n_rows, replace=False))
            if rows.tobytes() not in pats:
                break
        pats.add(rows.tobytes())
        for j in group_cols:
            r_.append(rows); c_.append(np.full(n_rows, j)); v_.append(rng.uniform(lo, hi, n_rows))
        groups.append(np.asarray(group_cols))

    for i, (n_rows, lo, hi) in enumerate(spec):
        add(cols[i * GROUP:(i + 1) * GROUP], n_rows, lo, hi)
    W = sp.csc_matrix((np.concatenate(v_).astype(np.float32), (np.concatenate(r_), np.concatenate(c_))), shape=(n_items, n_items))
    W.sort_indices()
    return W, feat, groups


def host_layout(W, tc):
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    return build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=tc)


def stored_rows(L):
    rt = np.asarray(L["fr_rows_of_tile"]).view(np.uint64).reshape(-1, 2)
    return np.array([bin(int(a)).count("1") + bin(int(b)).count("1") for a, b in rt])


def add_sweepers(X, groups, at, seed):
    """Users `at` rate every item except one column in each of 15 groups."""
    rng = np.random.default_rng(seed)
    n_items = X.shape[1]
    for i, u in enumerate(at):
        pick = (np.arange(15) + 3 * i) % len(groups)            # every sweeper another 15 tiles, the five ring tiles among them
        pick[:len(COUNTS)] = 2 + np.arange(len(COUNTS))
        leave = np.array([rng.choice(groups[g]) for g in np.unique(pick)])
        items = np.setdiff1d(np.arange(n_items), leave)
        X = set_row(X, u, items, rng.integers(1, 6, len(items)).astype(np.float32))
    return X


def head_cuts(L):
    """Head sizes in KiB by where they end: 0; between two tiles; inside a tile (its first fragment resident, the
    continuation gathered) -- None where the layout has no such cut inside HEAD_MAX_KIB.  The kernel cuts the head
    between super-tiles, so these are all the places a head can end at; "all but the last fragment" is therefore all but
    the last SUPER-TILE, and takes a W that fits the head whole: the flat cases below."""
    kb, st, ft = (np.asarray(L[k]) for k in ("fr_super_kb", "fr_super_tile", "fr_frag_tile"))
    first = lambda s: bool(ft[st[s]] & (1 << 24))
    inner = [s for s in range(1, L["fr_n_super"]) if kb[s] - kb[0] <= HEAD_MAX_KIB]
    between = [int(kb[s] - kb[0]) for s in inner if first(s)]
    inside = [int(kb[s] - kb[0]) for s in inner if not first(s)]
    return dict(none=0, between=between[-1] if between else None, inside=inside[0] if inside else None)


class Case:
    def __init__(self, oracle, W, X, tc=256):
        self.oracle, self.W, self.X, self.tc = oracle, W, X, tc
        self.Wr = W.tocsr()
        self.eng = SlimEngine(device="cuda:0", tile_cols=256)
        self.eng.FR_TILE_COLS = tc
        self.eng.set_interactions(None, X, need_csc=False)
        self.eng.set_weights(W)
        self.L = host_layout(W, tc)
        self.ref = {}

    def run(self, uw, rows, top_k=10, filt=True, dense=False, head=-1, row_ids=None):
        self.eng.fr_users_per_wave, self.eng.fr_head_kib = uw, head
        mode = _native.TOPK_DENSE if dense else _native.TOPK_SPARSE
        out = self.eng.recommend_rows(np.asarray(rows), top_k=top_k, filter_interacted=filt, mode=mode)
        assert self.eng.last_score_path.startswith("feature_rows"), self.eng.last_score_path
        assert self.eng._layout(True, top_k)["fr_tile_cols"] == self.tc
        return out

    def check(self, uw, rows, top_k=10, filt=True, dense=False, head=-1):
        rows = np.asarray(rows)
        key = (rows.tobytes(), top_k, filt, dense)
        if key not in self.ref:
            self.ref[key] = self.oracle.recommend_batch(self.X[rows], self.Wr, top_k=top_k, filter_interacted=filt, dense=dense)
        o_ids, o_sc, o_cnt = self.ref[key]
        ids, sc, cnt = self.run(uw, rows, top_k, filt, dense, head)
        assert np.array_equal(cnt, o_cnt)
        assert np.array_equal(ids, o_ids)
        assert np.array_equal(bits(sc), bits(o_sc))
        return ids, sc, cnt


SWEEPERS = (0, 3, 130, 512, 544, 777, 999)
_cases = {}


def get_case(name, oracle):
    if name not in _cases:
        n_feat, tc = {"tall": (110, 256), "narrow": (110, 128), "short": (50, 256), "short_narrow": (50, 128)}[name]
        W, feat, groups = grouped_w(n_feat, seed=n_feat)
        X = users(1000, W.shape[0], feat, seed=n_feat + 1, hi=min(40, n_feat))
        X = add_sweepers(X, groups, SWEEPERS, seed=n_feat + 2)
        X = set_row(X, 998, [], [])                                                       # no rating at all
        X = set_row(X, 17, np.setdiff1d(np.arange(W.shape[0]), feat)[:3], [1.0, 2.0, 3.0])  # no rating on any row of W
        X = set_row(X, 260, feat, 5.0 - 0.25 * np.random.default_rng(260).random(len(feat)).astype(np.float32))   # heavy among light
        c = Case(oracle, W, X, tc)
        c.feat, c.groups = feat, groups
        _cases[name] = c
    return _cases[name]


# W of MORE THAN 64 narrow tiles in less than the head's LDS: the layout builder keeps a W of up to 64 tiles in one super-tile
# (the all-resident form), a larger one it packs into super-tiles of 36 KiB, and here every one of them fits the head.
#   flat3: 2 tiles of 6 rows, 62 of one row, and LAST (the smallest weights) 2 tiles of 2D+1 = 9 rows: 79 KiB in three
#          super-tiles of 31, 33 and 2 fragments.  Head = all but the last super-tile: 64 resident fragments, then both 9-row
#          tiles through the ring (five instructions each, the last one half used).
#   flat2: 64 tiles of one row, last 2 tiles of D+1 = 5 rows: 70 KiB in two super-tiles, LESS than the 85 KiB the LDS
#          leaves, so the plan caps the head at W's size (n_super * 36 KiB).
FLAT = {"flat3": [(6, 0.05, 0.3)] + [(1, 0.0005, 0.002)] * 31 + [(2 * RING + 1, 0.00002, 0.0001)],
        "flat2": [(1, 0.05, 0.3)] + [(1, 0.0005, 0.002)] * 31 + [(RING + 1, 0.00002, 0.0001)]}
FLAT_SWEEPERS = (0, 130, 544, 999)


def get_flat(name, oracle):
    if name not in _cases:
        spec = FLAT[name]
        W, feat, groups = grouped_w(50, seed=len(name) + 50 * len(spec), spec=spec)
        X = users(1000, W.shape[0], feat, seed=77, hi=40)
        rng = np.random.default_rng(78)
        for i, u in enumerate(FLAT_SWEEPERS):                  # rate everything but one column in each of 15 groups, the last among them
            pick = np.unique(np.concatenate([[0, len(groups) - 1], (np.arange(13) * 2 + i + 1) % (len(groups) - 2) + 1]))
            leave = np.array([rng.choice(groups[g]) for g in pick])
            items = np.setdiff1d(np.arange(W.shape[0]), leave)
            X = set_row(X, u, items, rng.integers(1, 6, len(items)).astype(np.float32))
        X = set_row(X, 998, [], [])
        c = Case(oracle, W, X, 128)
        c.feat, c.groups = feat, groups
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", ["flat3", "flat2"])
def test_flat_layouts_fit_the_head(oracle, name):
    c = get_flat(name, oracle)
    L, n = c.L, stored_rows(c.L)
    kb, st = np.asarray(L["fr_super_kb"]), np.asarray(L["fr_super_tile"])
    assert L["fr_tile_cols"] == 128 and L["fr_n_tiles"] > 64 and L["fr_n_frags"] == L["fr_n_tiles"]
    assert L["fr_n_super"] == (3 if name == "flat3" else 2) and kb[-1] - kb[0] <= HEAD_MAX_KIB
    last = n[st[-2]:]                                           # a long resident run; the ring tiles end the last super-tile
    assert st[-2] >= 31 and last[-2:].tolist() == [FLAT[name][-1][0]] * 2 and (len(last) == 2) == (name == "flat3")
    assert (L["fr_n_super"] * (L["fr_buf_bytes"] >> 10) < HEAD_MAX_KIB) == (name == "flat2")


@UW
@pytest.mark.parametrize("name", ["flat3", "flat2"])
def test_head_of_all_but_the_last_super_tile(oracle, uw, name):
    """The head holds everything (several super-tiles, nothing gathered) or everything but the last super-tile (only its
    fragments go through the ring, straight after a long run of resident ones), or nothing: one answer, the oracle's."""
    c = get_flat(name, oracle)
    kb = np.asarray(c.L["fr_super_kb"])
    heads = [-1, int(kb[-2] - kb[0]), 0]
    outs = [c.check(uw, np.arange(1000), top_k=15, head=h) for h in heads]
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()
    cnt = outs[0][2]
    assert (cnt[list(FLAT_SWEEPERS)] >= 10).all() and (cnt[list(FLAT_SWEEPERS)] <= 15).all() and cnt[998] == 0


# ---------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", ["tall", "narrow", "short", "short_narrow"])
def test_layouts_are_what_the_cases_need(oracle, name):
    c = get_case(name, oracle)
    L, n = c.L, stored_rows(c.L)
    per_group = GROUP // c.tc
    assert L["fr_tile_cols"] == c.tc and L["fr_n_super"] >= 3
    assert (L["fr_rows"] > 64) == name.startswith(("tall", "narrow"))
    for k in COUNTS:                                            # pure tiles of D-1 .. 2D+1 stored rows, behind the tall ones
        assert (n == k).sum() >= per_group, (k, n.tolist())
    assert (n[:2 * per_group] == L["fr_rows"] - 4).all()
    cuts = head_cuts(L)
    assert cuts["inside"] is not None
    if name == "tall":                                          # tile 0: a slice of three or more fragments
        assert (np.asarray(L["fr_frag_tile"]) & 0xFFFFFF == 0).sum() >= 3
    if name == "short_narrow":
        assert cuts["between"] is not None


@UW
@pytest.mark.parametrize("name", ["tall", "narrow", "short", "short_narrow"])
def test_ring_wrap_and_head_boundaries(oracle, uw, name):
    """Sweepers need every stored row of every tile; the head ends nowhere, inside a tile, between two tiles, and where the
    LDS puts it: one answer, the oracle's."""
    c = get_case(name, oracle)
    cuts = head_cuts(c.L)
    heads = [-1, 0, cuts["inside"]] + ([cuts["between"]] if cuts["between"] is not None else [])
    outs = [c.check(uw, np.arange(1000), top_k=15, head=h) for h in heads]
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()
    cnt = outs[0][2]
    assert (cnt[list(SWEEPERS)] >= 10).all() and (cnt[list(SWEEPERS)] <= 15).all() and cnt[998] == 0 and cnt[17] == 0


@UW
@pytest.mark.parametrize("name", ["tall", "short_narrow"])
@pytest.mark.parametrize("top_k", [1, 10, 15])
def test_batches_filters_and_short_lists(oracle, uw, name, top_k):
    """545 rows: a last job with a single user at 8 users per wave (545 = 68 * 8 + 1); lists that never fill at top_k 15,
    fill at 1 and 10; filter off: the sweepers' lists fill at once."""
    c = get_case(name, oracle)
    inside = head_cuts(c.L)["inside"]
    c.check(uw, np.arange(545), top_k=top_k, head=inside)
    c.check(uw, np.arange(513), top_k=top_k, filt=False, head=0)


@UW
def test_row_ids_as_a_strict_subset(oracle, uw):
    c = get_case("tall", oracle)
    rows = np.concatenate([np.setdiff1d(np.arange(1000), np.arange(0, 1000, 3))[:542], [999, 777, 3]])    # 545 of the 1,000 rows, the last three out of order
    assert len(rows) == 545 and len(np.unique(rows)) == 545
    c.check(uw, rows, top_k=15, head=0)
    c.check(uw, rows[::-1].copy(), top_k=10)


@UW
def test_dense_mode_through_the_fast_pass(oracle, uw):
    c = get_case("short", oracle)
    c.check(uw, np.arange(545), dense=True, head=head_cuts(c.L)["inside"])


@UW
def test_two_launches_return_identical_bytes(oracle, uw):
    c = get_case("narrow", oracle)
    a = c.run(uw, np.arange(1000), top_k=15, head=0)
    b = c.run(uw, np.arange(1000), top_k=15, head=0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
