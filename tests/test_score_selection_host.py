"""The tiled selection and the value routing of rtrec_slim_score_topk on the host, before any device run.

layouts.select_topk_model is a numpy model of select_topk (csrc/score.hip): admission, rank by count, the returned count,
branch by branch.  Here it is run tile by tile on the twelve value sets of tests/test_score_values_host.py, its per-tile lists
are merged like merge_topk_kernel merges them, and the result is held to the `definition` -- with the admission the kernel has
now (`key > -inf`).  With the admission it had before (`key != -inf`) the same model shows the defect the header used to name:
slots below the returned count that no lane wrote (test_old_admission_leaves_slots_unwritten prints the table).

Also here: score_plan.values_ordinary and the engine's evaluation of it at the boundary 2^127, and the layout builders' rule
that a row segment with a stored zero stays out of the dense blocks.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.layouts import build_tiled_w, build_tiled_w_device, select_topk_model
from tests.test_score_values_host import (DENSE, F32, F64, HEAVY_ROWS, N_ITEMS, N_USERS, SPARSE, TILE, TOP_KS, VALUE_SETS, case,
                                          cpu_engine, definition, same)

NO_NAN_INPUT_BUT_UNSAFE = ("plus_inf_ties", "inf_weight", "overflow_finite")    # reach the PREFILTER's -inf + inf


def tile_keys(c, u, mode, f64, filt):
    """(keys, aux, whole_tile) of row u over all columns, as the accumulators stand when select_topk runs: the sums of the
    definition; an own item (filter) holds -inf plus whatever was added to it (SPARSE: the PREFILTER writes -inf first, so
    an infinite or NaN product leaves a NaN; DENSE: -inf is written after the sums); SPARSE: an untouched column and a zero
    sum have the key -inf, aux is the first-touch position."""
    acc, ft, _order = c.sums(f64)[u]
    own = c.xi[int(c.xp[u]):int(c.xp[u + 1])]
    keys = acc.copy()
    ninf = keys.dtype.type(-np.inf)
    with np.errstate(invalid="ignore"):
        if mode == SPARSE:
            if filt:
                keys[own] = ninf + keys[own]
            keys[(ft < 0) | (keys == 0)] = ninf
        elif filt:
            keys[own] = ninf
    heavy = bool(np.isin(own, HEAVY_ROWS).any())          # a dense block ends the touched list: the whole tile is scanned
    return keys, ft, heavy


def model_lists(c, rows, top_k, mode, f64, filt, old_admission=False, first_pass=False):
    """The call's outputs from the model: per tile select_topk (kk = top_k + 1 in SPARSE mode, whose merge looks for ties;
    first-touch keys as in the exact-tie pass -- or none, the (score, id) compare of the FIRST pass, whose tie order is not the
    reference's), then the tiles' lists merged by (score, aux, id).  Also returns the (row, tile) jobs with an unwritten
    slot as (row, tile, returned count, unwritten slots, NaN keys the admission let in)."""
    kk = top_k + 1 if mode == SPARSE else top_k
    R = len(rows)
    ids = np.full((R, top_k), -1, np.int32)
    sc = np.full((R, top_k), -np.inf, F32)
    sc64 = np.full((R, top_k), -np.inf, F64) if f64 else None
    aux = np.zeros((R, top_k), np.uint32)
    cnt = np.zeros(R, np.int32)
    broken = []
    for r, u in enumerate(np.asarray(rows).tolist()):
        keys, ft, heavy = tile_keys(c, u, mode, f64, filt)
        cands = []
        for t0 in range(0, N_ITEMS, TILE):
            cols = np.arange(t0, min(t0 + TILE, N_ITEMS))
            whole = mode == DENSE or heavy
            if not whole:                                   # the touched list: touched columns and own items, first touch first
                own = c.xi[int(c.xp[u]):int(c.xp[u + 1])]
                listed = cols[(ft[cols] >= 0) | (np.isin(cols, own) & filt)]
                cols = listed[np.argsort(ft[listed], kind="stable")]
            if len(cols) == 0:
                continue
            m = select_topk_model(keys[cols], cols, ft[cols] if (mode == SPARSE and not first_pass) else None, kk, whole_tile=whole,
                                  old_admission=old_admission)
            if m["unwritten"]:
                broken.append((u, t0 // TILE, m["count"], len(m["unwritten"]), int(np.isnan(keys[cols]).sum())))
                continue
            cands += list(zip(m["slot_score"].tolist(), m["slot_aux"].tolist(), m["slot_id"].tolist()))
        if old_admission and any(np.isnan(s) for s, _a, _i in cands):
            continue                                        # (the merge's NaN precondition: nothing to model)
        cands.sort(reverse=True)
        n = min(len(cands), top_k)
        cnt[r] = n
        for k, (s, a, i) in enumerate(cands[:n]):
            ids[r, k], aux[r, k] = i, a if mode == SPARSE else 0
            with np.errstate(over="ignore"):
                sc[r, k] = F32(s)
            if f64:
                sc64[r, k] = s
    return (ids, sc, sc64, aux, cnt), broken


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", VALUE_SETS)
def test_selection_model_is_the_definition(name, f64):
    """Admission `key > -inf`: no slot below a returned count is unwritten, and lists, scores (bits), first-touch keys and
    counts are the definition's, SPARSE and DENSE, with and without the filter, at every top_k."""
    c = case(name)
    rows = list(range(N_USERS))
    for mode in (SPARSE, DENSE):
        for filt in (True, False):
            for k in TOP_KS:
                got, broken = model_lists(c, rows, k, mode, f64, filt)
                assert not broken, (name, mode, filt, k, broken[:3])
                msg = same(got, definition(c, rows, k, mode, f64, filt), f"{name} mode={mode} f64={f64} filter={filt} k={k}")
                assert not msg, msg
                assert not np.isnan(got[1]).any()
                if mode == SPARSE:                          # the first pass (no first-touch keys): the same columns, no hole
                    first, broken = model_lists(c, rows, k, mode, f64, filt, first_pass=True)
                    assert not broken and np.array_equal(first[4], got[4]), (name, filt, k, broken[:3])
                    assert np.array_equal(np.sort(first[1], axis=1).view(np.uint32), np.sort(got[1], axis=1).view(np.uint32))


def test_old_admission_leaves_slots_unwritten():
    """`key != -inf` lets a NaN accumulator in.  Where the lanes rank what they hold (a job that lists at most 64 columns),
    every compare with a NaN is false: in the first pass all NaN candidates and the true best take rank 0 and share one slot,
    with first-touch keys the order is no longer transitive and ranks collide as well -- and the function still returns
    min(n_have, kk): slots below the count that nobody wrote, which emit_result would have read as indices.  (A job with more
    than 64 columns goes through the threshold passes, whose `key >= tau` no NaN passes, so at this shape only the short
    rows show the hole; kk > 64 scans list NaN columns instead.)  Three sets have NaN accumulators WITHOUT a NaN input:
    -inf + inf on an own item, and inf - inf after an overflow.  The table is the "before" column of the change that
    repaired the admission; no device ever ran these sets with the old admission."""
    rows = list(range(N_USERS))
    table = {}
    for name in VALUE_SETS:
        c = case(name)
        holes = [len(model_lists(c, rows, 10, SPARSE, False, filt, old_admission=True, first_pass=fp)[1])
                 for filt, fp in ((True, True), (False, True), (True, False))]
        nan_rows = [sum(bool(np.isnan(tile_keys(c, u, SPARSE, False, filt)[0]).any()) for u in rows) for filt in (True, False)]
        wrong_200 = bool(same(model_lists(c, rows[:6], 200, SPARSE, False, True, old_admission=True)[0], definition(c, rows[:6], 200, SPARSE, False, True)))
        table[name] = (sum(holes), nan_rows, wrong_200)
    print("\n".join(f"{n:24s} jobs with an unwritten slot (top_k 10): {h:3d}   rows with a NaN accumulator (filter, no filter): {r}"
                    f"   top_k 200 wrong: {w}" for n, (h, r, w) in table.items()))
    assert table["all_nan"][0] >= 20 and table["nan_rating"][0] >= 1
    for name in VALUE_SETS:                                  # the hole needs an admitted NaN
        assert table[name][0] == 0 or max(table[name][1]) > 0
    for name in ("plus_inf_ties", "overflow_finite"):        # no NaN in X or W, yet NaN accumulators -- on own items only
        c = case(name)
        assert not np.isnan(c.xv).any() and not np.isnan(c.wv).any()
        assert table[name][1][0] > 0 and table[name][1][1] == 0
    assert table["overflow_cancel"][1] == [N_USERS, N_USERS] and np.isfinite(case("overflow_cancel").wv).all()
    assert table["minus_inf"] == (0, [0, 0], False) and table["inf_weight"][:2] == (0, [0, 0])
    # the new admission: none of it
    for name in ("all_nan", "nan_rating"):
        for filt, fp in ((True, True), (False, True), (True, False)):
            assert not model_lists(case(name), rows, 10, SPARSE, False, filt, first_pass=fp)[1]


def test_rank_by_count_writes_every_slot_without_a_nan():
    """The argument of DESIGN.md 3.5 on random keys: distinct columns and no NaN among the admitted keys -> the ranks of the
    held candidates are 0 .. n - 1, so every slot below min(n, kk) is written once.  Mass ties, +-inf and zeros included;
    every branch of the model (n <= 64, kk > 64, quad maxima, lane bests, list, bounded scans)."""
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(300):
        n = int(rng.choice([1, 5, 64, 65, 200, 256, 700]))
        kk = int(rng.choice([1, 2, 11, 16, 17, 64, 65, 201]))
        pool = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 1.0, 2.5, -3.0], F32)
        keys = rng.choice(pool, size=n) if trial % 2 else rng.normal(size=n).astype(F32)
        if trial % 3 == 0:
            keys[rng.random(n) < 0.3] = np.nan
        ids = rng.permutation(4096)[:n]
        aux = rng.integers(0, 4, n) if trial % 4 < 2 else None
        m = select_topk_model(keys, ids, aux, kk, whole_tile=bool(trial % 5 == 0))
        with np.errstate(invalid="ignore"):
            ok = keys > -np.inf
        want = sorted(zip(keys[ok].tolist(), (aux[ok] if aux is not None else np.zeros(ok.sum(), int)).tolist(), ids[ok].tolist()), reverse=True)[:kk]
        assert m["unwritten"] == [] and m["collisions"] == 0 and m["count"] == len(want)
        assert list(zip(m["slot_score"].tolist(), m["slot_aux"].tolist(), m["slot_id"].tolist())) == want
        seen.add((n <= 64, kk > 64, kk <= 16))
    assert len(seen) >= 5


# ---------------------------------------------------------------------------------------------- the value fact
def test_values_ordinary_at_the_boundary():
    from rtrec_amd.score_plan import VALUE_LIMIT, values_ordinary
    assert VALUE_LIMIT == 2.0 ** 127
    x, w = float(F32(2.0 ** 62)), float(F32(2.0 ** 63))
    assert not values_ordinary(4, x, w)                                          # 4 * 2^62 * 2^63 = 2^127 exactly
    assert values_ordinary(4, x, float(np.nextafter(F32(w), F32(0))))           # one float32 step below
    assert values_ordinary(3, x, w) and not values_ordinary(5, x, w)
    assert not values_ordinary(1, float("nan"), 1.0) and not values_ordinary(1, 1.0, float("nan"))
    assert not values_ordinary(1, float("inf"), 1.0) and not values_ordinary(1, 1.0, float("inf"))
    assert not values_ordinary(1, 0.0, float("inf"))                             # a stored zero rating times inf is a NaN
    assert values_ordinary(0, None, float("inf")) and values_ordinary(7, float("nan"), None)     # an empty side: no product
    assert values_ordinary(10 ** 6, 5.0, 1.0)


def _engine_with(xv_rows, wv):
    """An engine (CPU stand-in) holding X = rows of ratings on items 0.., W = one column of the weights `wv`."""
    import torch
    from rtrec_amd.backend import DeviceWeights
    from rtrec_amd.engine import SlimEngine
    from tests.cpu_backend import OracleBackend
    n_items = 8
    ptr = np.zeros(len(xv_rows) + 1, np.int32)
    np.cumsum([len(r) for r in xv_rows], out=ptr[1:])
    idx = np.concatenate([np.arange(len(r)) for r in xv_rows] + [np.empty(0, int)]).astype(np.int32)
    val = np.concatenate([np.asarray(r, F32) for r in xv_rows] + [np.empty(0, F32)]).astype(F32)
    eng = SlimEngine(backend=OracleBackend())
    eng.set_interactions(None, sp.csr_matrix((val, idx, ptr), shape=(len(xv_rows), n_items)), need_csc=False)
    wv = np.asarray(wv, F32)
    eng.set_weights(DeviceWeights(torch.arange(len(wv), dtype=torch.int64), torch.full((len(wv),), 7, dtype=torch.int64),
                                  torch.from_numpy(wv.copy()), n_items, False))
    return eng


def resident_ok(eng):
    return eng._values_ordinary((eng._X["rptr"], eng._X["rcol"], eng._X["rval"]))


def test_engine_evaluates_the_value_fact_and_caches_it():
    """The engine's reductions behind the fact: n_max from the longest row, NaN and inf propagate through max |.|, the
    rating part is cached for the resident X only, the weight part per weights; replacing either drops its cache."""
    import torch
    big_x, big_w = F32(2.0 ** 62), F32(2.0 ** 63)
    eng = _engine_with([[1.0], [big_x, 1.0, 1.0, 1.0]], [big_w, 1.0])
    xb = (eng._X["rptr"], eng._X["rcol"], eng._X["rval"])
    assert eng._x_bound(xb) == (4, float(big_x)) and eng._w_absmax() == float(big_w)
    assert not eng._values_ordinary(xb)                                          # exactly 2^127
    assert eng._X["rval_bound"] == (4, float(big_x)) and eng._W["w_absmax"] == float(big_w)
    below = _engine_with([[1.0], [big_x, 1.0, 1.0, 1.0]], [np.nextafter(big_w, F32(0)), 1.0])
    assert below._values_ordinary((below._X["rptr"], below._X["rcol"], below._X["rval"]))
    # a batch that is not resident: computed per call, nothing cached, the resident cache untouched
    other = (torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), torch.tensor([1.0, float("nan")]))
    assert not below._values_ordinary(other) and below._X["rval_bound"] == (4, float(big_x))
    assert below._values_ordinary((other[0], other[1], torch.tensor([1.0, 2.0])))
    # NaN rating, infinite weight, empty X, empty W
    assert not resident_ok(_engine_with([[1.0, np.nan]], [1.0]))
    assert not resident_ok(_engine_with([[1.0]], [np.inf]))
    assert not resident_ok(_engine_with([[0.0]], [-np.inf]))
    assert resident_ok(_engine_with([[], []], [np.inf]))
    assert resident_ok(_engine_with([[np.nan]], []))
    # new ratings / new weights: the caches go with the object they describe
    eng.set_interactions(None, sp.csr_matrix(np.ones((2, 8), F32)), need_csc=False)
    assert "rval_bound" not in eng._X and resident_ok(eng)                      # 8 * 1 * 2^63 now
    eng2 = _engine_with([[1.0]], [np.nan])
    assert not resident_ok(eng2)
    eng2.set_weights(eng.weights)
    assert "w_absmax" not in eng2._W and resident_ok(eng2)


# ---------------------------------------------------------------------------------------------- dense blocks and stored zeros
@pytest.mark.parametrize("name", ["inf_times_stored_zero", "inf_rating_mixed"])
def test_a_row_segment_with_a_stored_zero_stays_out_of_the_dense_blocks(name):
    """Both builders of the compacted layout: the heavy rows of W are dense blocks (every tile) -- except the (tile, row)
    segments that store a zero, which stay CSR, zero and all.  In a dense block a zero is therefore always padding."""
    import torch
    c = case(name)
    r, cc, v = c.w_coo_by_column()
    Wc = sp.csc_matrix((v, r, np.concatenate([[0], np.cumsum(np.bincount(cc, minlength=N_ITEMS))])), shape=(N_ITEMS, N_ITEMS))
    T = build_tiled_w(Wc, 0, N_ITEMS, TILE, compact=True, dense_fill=1.0 / 3.0)
    D = build_tiled_w_device(torch, torch.from_numpy(r), torch.from_numpy(cc), torch.from_numpy(v.copy()), N_ITEMS, 0, N_ITEMS, TILE,
                             compact=True, dense_fill=1.0 / 3.0)
    assert np.array_equal(D["dense_idx"].numpy(), T.dense_idx) and np.array_equal(bits_(D["dense_val"].numpy()), bits_(T.dense_val))
    assert np.array_equal(D["tile_ptr"].numpy(), T.tile_ptr) and np.array_equal(bits_(D["w_val"].numpy()), bits_(T.w_val))
    di = T.dense_idx.reshape(T.n_tiles, N_ITEMS)
    W = c.W()
    n_zero_segments = n_dense_rows = 0
    for h in HEAVY_ROWS:
        for t in range(T.n_tiles):
            seg = W.data[W.indptr[h]:W.indptr[h + 1]][(W.indices[W.indptr[h]:W.indptr[h + 1]] // TILE) == t]
            has_zero = bool((seg == 0).any())
            n_zero_segments += has_zero
            full = len(seg) >= max(64, int(TILE / 3.0))      # (the 128 columns of the last tile rarely are)
            n_dense_rows += int(di[t, h] >= 0)
            assert (di[t, h] >= 0) == (full and not has_zero), (h, t)
    assert n_zero_segments == (3 if name == "inf_times_stored_zero" else 0) and n_dense_rows >= (6 if n_zero_segments else 8)
    # every stored zero is still stored, in the CSR part
    assert int((T.w_val == 0).sum()) == int((c.wv == 0).sum())
    dense_rows = T.dense_val.reshape(-1, T.tile_cols)
    stored = np.zeros_like(dense_rows, dtype=bool)
    for t, h in zip(*np.nonzero(di >= 0)):
        cols = W.indices[W.indptr[h]:W.indptr[h + 1]]
        cols = cols[cols // TILE == t] % TILE
        stored[di[t, h], cols] = True
    assert np.array_equal(dense_rows != 0, stored)           # zero <=> not stored


def bits_(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
