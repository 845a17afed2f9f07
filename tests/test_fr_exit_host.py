"""Host model of score_frows_kernel's early exit (rtrec_amd.layouts.fr_exit_suffix_bound / fr_exit_model).

The kernel leaves a job once no user of it can open a tile that is still to come: the first-level tile test with
sfx[s + 1] = the largest frag_wtop from super-tile s + 1 on in place of a tile's own bound.  Two properties make that
exact: sfx dominates every later fragment's bound, and a user whose predicate has closed has no later column whose
float32 score beats its threshold."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.layouts import build_feature_rows, fr_exit_model, fr_exit_suffix_bound


def head_tail_w(n_items=3000, n_feat=70, n_head=520, seed=0, signed=False, tail_w=0.002):
    """A W that streams: `n_head` columns with a weight of 0.05-0.3 on nearly every feature row (tall head tiles), the other
    columns with one or two weights of at most `tail_w` on a handful of rows (flat tail tiles)."""
    rng = np.random.default_rng(seed)
    feat = np.sort(rng.choice(n_items, n_feat, replace=False))
    M = np.zeros((n_items, n_items), dtype=np.float32)
    cols = rng.permutation(n_items)
    for j in cols[:n_head]:
        rows = feat[rng.random(n_feat) < 0.95]
        v = rng.uniform(0.05, 0.3, len(rows)).astype(np.float32)
        M[rows, j] = np.where(rng.random(len(rows)) < 0.5, -v, v) if signed else v
    tail_rows = feat[rng.choice(n_feat, 6, replace=False)]
    for j in cols[n_head:]:
        rows = rng.choice(tail_rows, int(rng.integers(1, 3)), replace=False)
        v = rng.uniform(0.0002, tail_w, len(rows)).astype(np.float32)
        M[rows, j] = -v if signed and rng.random() < 0.5 else v
    np.fill_diagonal(M, 0)
    W = sp.csc_matrix(M)
    W.sort_indices()
    return W, feat


def users(n_users, n_items, feat, seed=1, signed=False):
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for u in range(n_users):
        own = rng.choice(feat, int(rng.integers(0, 25)), replace=False)
        other = rng.choice(n_items, int(rng.integers(0, 30)), replace=False)
        its = np.unique(np.concatenate([own, other]))
        rows += [u] * len(its)
        cols += its.tolist()
        r = rng.integers(1, 6, len(its)).astype(np.float32)
        vals += (np.where(rng.random(len(its)) < 0.3, -r, r) if signed else r).tolist()
    X = sp.csr_matrix((np.array(vals, np.float32), (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    return X


def layout(W, tc=256):
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    return build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=tc)


@pytest.fixture(scope="module", params=[(256, False), (128, False), (256, True)], ids=["tc256", "tc128", "tc256-signed"])
def case(request):
    tc, signed = request.param
    W, feat = head_tail_w(signed=signed, seed=3 if signed else 0)
    L = layout(W, tc)
    assert L is not None and L["fr_n_super"] >= 4                  # the W streams
    X = users(160, W.shape[0], feat, signed=signed)
    return W, L, X


def test_suffix_bound_is_non_increasing_and_dominates_every_later_fragment(case):
    _, L, _ = case
    sfx = fr_exit_suffix_bound(L)
    st = np.asarray(L["fr_super_tile"])
    tail = np.asarray(L["fr_w"])[int(L["fr_super_kb"][-1]) * 256:]
    assert sfx.dtype == np.float32 and sfx.shape == (L["fr_n_super"] + 1,)
    assert sfx[-1] == 0 and np.all(np.diff(sfx) <= 0)
    for s in range(L["fr_n_super"]):
        assert np.all(tail[st[s]:] <= sfx[s]) and sfx[s] == tail[st[s]:].max()
    # a tile's continuation fragments carry the tile's own bound: what holds a cut slice open holds its rest open
    ft = np.asarray(L["fr_frag_tile"]) & 0xFFFFFF
    for t in np.unique(ft):
        assert len(np.unique(tail[ft == t])) == 1


@pytest.mark.parametrize("top_k,filt", [(10, True), (10, False), (1, True), (15, True)])
def test_a_closed_user_has_no_later_column_above_its_threshold(case, top_k, filt):
    """Once the predicate has closed for a user at the hand-over that ends super-tile s, every column of a tile with a
    fragment behind s has |float32 score| <= the user's threshold there (scores summed in float32 in row order) -- and the
    predicate stays closed."""
    W, L, X = case
    M = fr_exit_model(L, W, X, top_k, filter_interacted=filt)
    tc = L["fr_tile_cols"]
    assert M["closed"].any() and not M["closed"][M["l1"] > 0, 0].all()
    for u in range(X.shape[0]):
        c = M["closed"][u]
        assert np.all(c[int(c.argmax()):]) or not c.any()          # monotone
        for s in np.flatnonzero(c):
            thr = M["thr_end"][u, s]
            for t in M["later_tiles"][s]:
                sc = M["scores"][u, t * tc:(t + 1) * tc]
                if M["l1"][u] == 0:
                    assert not sc.any()
                else:
                    assert thr >= 0 and np.all(np.abs(sc) <= thr)


def test_needed_depth_of_a_heavy_head_light_tail(case):
    """The head closes nearly every job well before the end of W; a user whose list never fills holds its job to the end."""
    W, L, X = case
    M = fr_exit_model(L, W, X, 10)
    n_super = M["n_super"]
    full = np.isfinite(M["thr_end"][:, -1])
    assert full.sum() > 100
    assert np.all(M["depth"] <= M["depth_open"]) and np.all(M["depth_open"] <= n_super)
    assert np.all(M["depth"][~full & (M["l1"] > 0)] == n_super)
    assert np.all(M["depth"][M["l1"] == 0] == 1)
