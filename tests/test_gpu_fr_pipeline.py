"""The job loop of score_frows_kernel: a wave's first job is its own number in the grid, every further one is claimed from
the queue at the end of the job before it; per job the wave follows the chain work order -> row id -> row pointers, takes
the first 128 entries of every user into registers and the rest in rounds of four or eight chunks, and the emit writes to
the row the chain went through.  Whatever job a wave runs, and however many: ids, counts and score bits equal the
oracle's, the three users-per-wave forms (which group the users differently, so that a stale register or a job taken one
too late does not coincide across them) return the same bytes, and so do two launches.  The file was written for a
pipelined form of the loop (next job's claim, extents and entries in flight under the current one; DESIGN 3.1, round 10:
measured slower, not kept) and asks of any job loop what it asked of that one.

Shapes.  W: 50 feature rows, 24 tiles of 256 columns (tests/test_gpu_fr_gather.py's `grouped_w`: several super-tiles, a
head and a ring).  The grid is capped at 256 workgroups of 16 waves, so a wave runs several jobs only from 4096 * uw rows
on: the steady-state batches hold 3 * 4096 * uw + 2048 * uw + 1 rows (waves run 3 or 4 jobs, the last job holds one user)
of short users (mean ~24 entries), with rows of every length at which the setup takes another path -- 0, 1, 63, 64,
65, 127, 128, 129 (the 128 entries held in registers), 320, 321 (one and two rounds of four chunks), 1,300 (the
eight-chunk rounds of the 2- and 4-user forms) -- scattered through them.  Small batches (513, 545, 1,000, 1,024 rows: no
work order, most waves get no job or one, the queue is claimed past its end) carry the same lengths in a cycle of eleven,
so that long and short users follow each other in consecutive jobs of a wave slot.

Mutants these tests are meant to catch (csrc/score.hip): a gap between the static first jobs and the claimed ones (count +
number of waves + 1: a job nobody runs), one job's entries or extents used for another (or kept for a shorter row), a
position past n_rows or a job past the end forming a row, the emit writing to another job's rows.  Not caught: an overlap
(count + number of waves - 1), where one job merely runs twice and writes the same bytes.  The static first job returns
the bytes its parent returned, so these tests guard the job loop; they do not tell the two kernels apart."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd import _native

from .test_gpu_fr_exit import bits
from .test_gpu_fr_gather import Case, grouped_w

pytestmark = pytest.mark.gpu

UW = pytest.mark.parametrize("uw", [2, 4, 8])
EDGE = (0, 1, 63, 64, 65, 127, 128, 129, 320, 321, 1300)
N_FEAT = 50
N_BIG = 3 * 4096 * 8 + 2048 * 8 + 1            # 114,689 rows: the steady state of the 8-user form
N_SAMPLE = 8192


def steady_rows(uw):
    return 3 * 4096 * uw + 2048 * uw + 1


def random_users(n_users, n_items, feat, edge_at, seed):
    """Users with ~24 distinct entries, about a third of them feature items; user edge_at[i] has exactly
    EDGE[i % len(EDGE)] entries, a third of them (at most all 50) feature items.  Ratings 1..5."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, 41, n_users)
    tot = int(lens.sum())
    rows = np.repeat(np.arange(n_users), lens)
    cols = np.where(rng.random(tot) < 0.35, feat[rng.integers(0, len(feat), tot)], rng.integers(0, n_items, tot))
    key = np.unique(rows.astype(np.int64) * n_items + cols)            # a user's items are distinct
    rows, cols = key // n_items, key % n_items
    keep = ~np.isin(rows, edge_at)
    rows, cols = rows[keep], cols[keep]
    e_rows, e_cols = [], []
    other = np.setdiff1d(np.arange(n_items), feat)
    for i, u in enumerate(edge_at):
        n = EDGE[i % len(EDGE)]
        n_f = min(len(feat), (n + 2) // 3)
        its = np.concatenate([rng.choice(feat, n_f, replace=False), rng.choice(other, n - n_f, replace=False)])
        e_rows.append(np.full(n, u)); e_cols.append(its)
    rows = np.concatenate([rows] + e_rows)
    cols = np.concatenate([cols] + e_cols)
    vals = rng.integers(1, 6, len(rows)).astype(np.float32)
    X = sp.csr_matrix((vals, (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    return X


_state = {}


def big_case(oracle):
    """One W, one X of 114,689 users on the device, shared by every test of this file."""
    if "big" not in _state:
        W, feat, groups = grouped_w(N_FEAT, seed=N_FEAT)
        rng = np.random.default_rng(5)
        # edge-length rows: the first 44 rows (every small batch sees the cycle four times), 11 * 40 scattered ones, and the
        # last rows of every steady-state batch (the one-user job)
        edge_at = np.unique(np.concatenate([np.arange(44), rng.choice(np.arange(44, N_BIG), 440, replace=False),
                                            [steady_rows(u) - 1 for u in (2, 4, 8)], [steady_rows(u) - 2 for u in (2, 4, 8)]]))
        X = random_users(N_BIG, W.shape[0], feat, edge_at, seed=6)
        c = Case(oracle, W, X, 256)
        c.edge_at = edge_at
        assert c.L["fr_n_super"] >= 3 and c.L["fr_n_tiles"] == 24 and c.L["fr_rows"] == N_FEAT
        nnz = np.diff(X.indptr)
        assert sorted(set(nnz[edge_at].tolist())) == sorted(EDGE) and 20 <= nnz.mean() <= 28
        _state["big"] = c
    return _state["big"]


def small_case(oracle):
    """1,024 users whose lengths run through EDGE in a cycle of eleven: with no work order job j of the strided deal holds the
    rows j, j + n_jobs, ...: in every user slot a long row is followed by a short one in the next job, and back."""
    if "small" not in _state:
        W, feat, groups = grouped_w(N_FEAT, seed=N_FEAT)
        X = random_users(1024, W.shape[0], feat, np.arange(1024), seed=7)
        c = Case(oracle, W, X, 256)
        nnz = np.diff(X.indptr)
        assert all(nnz[i] == EDGE[i % len(EDGE)] for i in range(1024))
        _state["small"] = c
    return _state["small"]


def to_np(out):
    return tuple(t.cpu().numpy().copy() for t in out)


def run_dev(c, uw, d_rows, n, top_k=10, filt=True):
    """A pass over a row tensor that stays on the device (bulk scoring): the engine gives such a row set the length order the
    first time and, for a layout of several super-tiles and 32,768+ rows, the pattern-grouped order (`consecutive`) from the
    second time on."""
    c.eng.fr_users_per_wave, c.eng.fr_head_kib = uw, -1
    out = to_np(c.eng.score_topk_device(None, n, top_k, filt, _native.TOPK_SPARSE, d_rows=d_rows))
    assert c.eng.last_score_path.startswith("feature_rows"), c.eng.last_score_path
    return out, bool(c.eng._order_grouped)


def oracle_on(c, rows, top_k=10, filt=True, dense=False):
    key = (np.asarray(rows).tobytes(), top_k, filt, dense)
    if key not in c.ref:
        c.ref[key] = c.oracle.recommend_batch(c.X[rows], c.Wr, top_k=top_k, filter_interacted=filt, dense=dense)
    return c.ref[key]


def assert_rows_equal_oracle(c, out, rows, at, top_k=10):
    """out[at] (positions of the batch) against the oracle's answers for the users rows[at]."""
    o_ids, o_sc, o_cnt = oracle_on(c, np.asarray(rows)[at], top_k)
    ids, sc, cnt = out
    assert np.array_equal(cnt[at], o_cnt)
    assert np.array_equal(ids[at], o_ids)
    assert np.array_equal(bits(sc[at]), bits(o_sc))


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def sample_of(c, n):
    """Every edge-length row of the first n, the batch's last rows, and a seeded sample of 8,192 rows."""
    rng = np.random.default_rng(n)
    at = np.concatenate([c.edge_at[c.edge_at < n], np.arange(n - 16, n), rng.choice(n, N_SAMPLE, replace=False)])
    return np.unique(at)


# ---------------------------------------------------------------------------------------------------------- the tests
@UW
def test_steady_state(oracle, uw):
    """3 or 4 jobs per wave, the last job one user.  First pass (length order, strided positions) and second pass
    (pattern-grouped, consecutive positions) of the same row tensor: the sample equals the oracle; every row is the same
    in both passes, in two launches and in the three forms."""
    c = big_case(oracle)
    n = steady_rows(uw)
    rows = np.arange(n, dtype=np.int32)
    d_rows = c.eng.be.to_dev(rows)
    c.eng._X.pop("_orders", None)
    first, g1 = run_dev(c, uw, d_rows, n)
    second, g2 = run_dev(c, uw, d_rows, n)
    third, g3 = run_dev(c, uw, d_rows, n)
    assert not g1 and g3 == g2 == (n >= c.eng.GROUPED_ORDER_MIN)
    at = sample_of(c, n)
    assert_rows_equal_oracle(c, first, rows, at)
    same_bytes(second, first)
    same_bytes(third, second)
    for other in (2, 4, 8):
        if other != uw:
            out, g = run_dev(c, other, d_rows, n)
            assert g == g2
            same_bytes(out, first)


def test_second_pass_is_the_grouped_one(oracle):
    """The 8-user batch is large enough for the pattern-grouped order (the smaller two run both passes in the length order)."""
    c = big_case(oracle)
    assert steady_rows(8) >= c.eng.GROUPED_ORDER_MIN and steady_rows(4) >= c.eng.GROUPED_ORDER_MIN > steady_rows(2)


@UW
@pytest.mark.parametrize("n", [513, 545, 1000, 1024])
def test_prefetch_boundaries_and_fewer_jobs_than_waves(oracle, uw, n):
    """No work order (fewer than 2,048 rows), fewer jobs than waves: most waves find their first job past the end, the
    others claim past it after one job; 1,024 rows are a whole number of jobs in every form, 513 and 545 end in a job of one user.  Every
    row is checked."""
    c = small_case(oracle)
    rows = np.arange(n)
    a = c.check(uw, rows)
    b = c.run(uw, rows)
    same_bytes(a, b)


@UW
def test_row_lengths_alternate_through_a_work_order(oracle, uw):
    """The same lengths with a work order (2,048+ rows: length order, strided positions): the users are the 1,024 of the
    small case taken three times over in a shuffled order, so every job mixes the long rows with the short ones."""
    c = small_case(oracle)
    rng = np.random.default_rng(11)
    rows = rng.permutation(np.tile(np.arange(1024), 3))[:2051]
    c.check(uw, rows)


@UW
def test_row_ids_a_strict_subset_with_repeats(oracle, uw):
    c = big_case(oracle)
    rng = np.random.default_rng(12)
    pool = np.concatenate([c.edge_at, rng.choice(N_BIG, 700, replace=False)])
    for n in (545, 4099):                              # without and with a work order
        rows = rng.choice(pool, n, replace=True)
        assert len(np.unique(rows)) < n
        c.check(uw, rows)
    n = steady_rows(2)                                 # several jobs per wave in the 2-user form
    rows = rng.choice(np.arange(0, N_BIG, 3), n, replace=True).astype(np.int32)
    d_rows = c.eng.be.to_dev(rows)
    out, _ = run_dev(c, uw, d_rows, n)
    at = np.unique(np.concatenate([np.arange(n - 16, n), rng.choice(n, N_SAMPLE, replace=False)]))
    assert_rows_equal_oracle(c, out, rows, at)
    again, _ = run_dev(c, uw, d_rows, n)
    same_bytes(again, out)


@UW
@pytest.mark.parametrize("top_k", [1, 10, 15])
def test_top_k_and_filter(oracle, uw, top_k):
    c = small_case(oracle)
    c.check(uw, np.arange(1000), top_k=top_k)
    c.check(uw, np.arange(545), top_k=top_k, filt=False)
    big = big_case(oracle)
    n = steady_rows(2)
    rows = np.arange(N_BIG - n, N_BIG, dtype=np.int32)
    d_rows = big.eng.be.to_dev(rows)
    for filt in (True, False):
        out, _ = run_dev(big, uw, d_rows, n, top_k=top_k, filt=filt)
        at = np.unique(np.concatenate([np.arange(n - 16, n), np.random.default_rng(top_k).choice(n, 2048, replace=False)]))
        o_ids, o_sc, o_cnt = oracle_on(big, rows[at], top_k, filt)
        assert np.array_equal(out[2][at], o_cnt) and np.array_equal(out[0][at], o_ids)
        assert np.array_equal(bits(out[1][at]), bits(o_sc))


@UW
def test_dense_mode_through_the_fast_pass(oracle, uw):
    c = small_case(oracle)
    c.check(uw, np.arange(1000), dense=True)
    c.check(uw, np.arange(545), dense=True, filt=False)
