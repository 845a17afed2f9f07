"""The per-fragment first-level bound that the feature-row layout stores behind its super-tiles (fr_w tail):
1.0001 * max |w| over the fragment's tile, float32-rounded.  score_frows_kernel skips a tile for a wave when
(sum_f |x_uf|) * that value cannot beat any of its users' current (k+1)-th best scores, so it must bound every
float32 score a user can have in the tile."""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.layouts import FR_TILE_HEADER_BYTES, build_feature_rows, build_feature_rows_device


def _w(n_items, n_feat, seed, signed):
    rng = np.random.default_rng(seed)
    feat = np.sort(rng.choice(n_items, n_feat, replace=False))
    M = np.zeros((n_items, n_items), dtype=np.float32)
    for j in rng.choice(n_items, int(n_items * 0.8), replace=False):
        rows = feat[rng.random(n_feat) < rng.uniform(0.05, 0.6)]
        v = rng.uniform(0.01, 1.0, len(rows)).astype(np.float32)
        M[rows, j] = -v if signed and rng.random() < 0.5 else v
    np.fill_diagonal(M, 0)
    return sp.csc_matrix(M)


def _layout(W, tc):
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    return build_feature_rows(W, 0, W.shape[0], cols, col_map, tile_cols=tc)


def _tail(L):
    kb = np.asarray(L["fr_super_kb"])
    return np.asarray(L["fr_w"])[int(kb[-1]) * 256:]


def _tile_max(W, L):
    """max |w| over each tile of the layout, from W itself."""
    tc, n_tiles = L["fr_tile_cols"], L["fr_n_tiles"]
    A = abs(W).tocsc()
    colmax = np.asarray(A.max(axis=0).todense()).ravel().astype(np.float32)
    per_pos = colmax[np.asarray(L["fr_col_ids"])]
    out = np.zeros(n_tiles, dtype=np.float32)
    np.maximum.at(out, np.arange(len(per_pos)) // tc, per_pos)
    return out


@pytest.mark.parametrize("tc", [256, 128])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tail_is_the_rounded_up_tile_maximum(tc, seed):
    W = _w(900, 70 if seed != 2 else 40, seed, signed=seed == 3)
    L = _layout(W, tc)
    assert L is not None
    tail = _tail(L)
    ftile = np.asarray(L["fr_frag_tile"]) & 0xFFFFFF
    assert tail.shape == (L["fr_n_frags"],) and tail.dtype == np.float32
    want = (_tile_max(W, L) * np.float32(1.0001))[ftile]
    assert np.array_equal(tail.view(np.uint32), want.view(np.uint32))
    # ... and it is >= every entry of the tile's header (max |w| per row), strictly where that is positive
    wd = np.asarray(L["fr_w"])
    kb, off, sup = np.asarray(L["fr_super_kb"]), np.asarray(L["fr_tile_off"]), np.asarray(L["fr_super_tile"])
    for g in range(L["fr_n_frags"]):
        if not (L["fr_frag_tile"][g] >> 24) & 1:
            continue
        s = int(np.searchsorted(sup, g, side="right")) - 1
        h0 = int(kb[s]) * 256 + (int(off[g]) - FR_TILE_HEADER_BYTES) // 4
        hdr = wd[h0:h0 + 128]
        assert np.all(tail[g] >= hdr) and (hdr.max() == 0 or tail[g] > hdr.max())


@pytest.mark.parametrize("tc", [256, 128])
def test_first_level_bound_covers_every_float32_score(tc):
    """(sum_f |x_f|) * tail >= |every float32 score| of the tile, each score summed in float32 in row order, for
    random users (the kernel's order: rows of W ascending)."""
    W = _w(800, 60, 7, signed=True)
    L = _layout(W, tc)
    tail = _tail(L)
    fmap = np.asarray(L["fr_map"])
    F = np.flatnonzero(fmap >= 0)
    dense = W.tocsr()[F][:, np.asarray(L["fr_col_ids"])].toarray().astype(np.float32)    # R x n_cols, layout order
    first = np.asarray(L["fr_frag_tile"]) & (1 << 24) != 0
    wtop = np.zeros(L["fr_n_tiles"], dtype=np.float32)
    wtop[np.asarray(L["fr_frag_tile"])[first] & 0xFFFFFF] = tail[first]
    rng = np.random.default_rng(0)
    for _ in range(40):
        x = np.zeros(len(F), dtype=np.float32)
        own = rng.random(len(F)) < rng.uniform(0.05, 0.9)
        x[own] = rng.uniform(-5, 5, own.sum()).astype(np.float32)
        l1 = np.float32(0)
        for v in np.abs(x):
            l1 = np.float32(l1 + v)
        s = np.zeros(dense.shape[1], dtype=np.float32)
        for f in range(len(F)):
            s = (s + np.float32(x[f]) * dense[f]).astype(np.float32)
        for t in range(L["fr_n_tiles"]):
            b = np.float32(l1 * wtop[t])
            assert np.all(np.abs(s[t * tc:(t + 1) * tc]) <= b)


def test_device_builder_writes_the_same_tail():
    torch = pytest.importorskip("torch")
    W = _w(700, 50, 11, signed=True)
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(W.shape[0], -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    H = build_feature_rows(W, 0, 700, cols, col_map)
    coo = W.tocoo()
    o = np.lexsort((coo.row, coo.col))
    D = build_feature_rows_device(torch, torch.from_numpy(coo.row[o].astype(np.int64)), torch.from_numpy(coo.col[o].astype(np.int64)),
                                  torch.from_numpy(coo.data[o].astype(np.float32)), 700, 0, 700)
    assert np.array_equal(D["fr_w"].numpy().view(np.uint32), np.asarray(H["fr_w"]).view(np.uint32))
