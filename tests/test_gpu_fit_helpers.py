"""Direct tests of the fit-side helper kernels and of the segment-layout builder (models: tests/fit_helper_models.py, held to
the C oracle and the numpy specification by tests/test_fit_helpers_host.py):

  A  the one-pass X^T y of a small fit call, read from its own scratch (every non-zero sum, not only the selected ones);
  B  every fit kernel path with work slots that serve many targets each;
  C  column norms and the Gram matrix at the boundaries of their loops;
  D  csrc/seg_build.hip at the boundaries it branches on, array by array against the specification and through a decoder.
"""
import functools

import numpy as np
import pytest

from rtrec_amd import _native
from rtrec_amd.engine import SlimEngine, sklearn_seed
from rtrec_amd.fit_plan import FitKnobs
from rtrec_amd.synth import interaction_matrix
from tests import fit_helper_models as fm
from tests.fit_call_log import FIT_ENV, OpsLog

pytestmark = pytest.mark.gpu

bits = fm.f32_bits


@pytest.fixture
def fresh_engine():
    """An engine of its own: no scratch cached by an earlier test."""
    return SlimEngine(device="cuda:0")


@pytest.fixture
def clean_env(monkeypatch):
    for k in FIT_ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def assert_fit_equals_oracle(tg, items, coef, count, n_iter, ref, K):
    """Feature sets, coefficient bits and sweep counts, as tests/test_gpu_kernels.py::test_fit_columns_bit_exact compares."""
    ptr, idx, val, nit = ref
    assert np.array_equal(n_iter, nit), f"n_iter differs on {np.flatnonzero(n_iter != nit)[:10]}"
    assert np.array_equal(count, np.diff(ptr))
    for t in range(len(tg)):
        c = count[t]
        got_i, got_v = items[t, :c], coef[t, :c]
        if K is not None:   # kernel emits selection order, oracle ascending ids
            o = np.argsort(got_i, kind="stable")
            got_i, got_v = got_i[o], got_v[o]
        assert np.array_equal(got_i, idx[ptr[t]:ptr[t + 1]]), f"feature set differs for column {tg[t]}"
        assert np.array_equal(bits(got_v), bits(val[ptr[t]:ptr[t + 1]])), f"coefficient bits differ for column {tg[t]}"


# ------------------------------------------------------------------------------------------------ A: one-pass X^T y
@functools.lru_cache(maxsize=None)
def xty_expected(name):
    """(CSC, CSR, candidate lists, tmap, compacted rows) of a case, computed once."""
    case = fm.xty_case(name)
    Xc, Xr = fm.both_orientations(case.X)
    tmap, per_user = fm.xty_compact_model(Xr, case.targets)
    return Xc, Xr, fm.xty_lists(fm.xty_model(Xr, case.targets)), tmap, per_user


_xty_fits = {}


def xty_oracle_fit(oracle, name):
    if name not in _xty_fits:
        case = fm.xty_case(name)
        _xty_fits[name] = oracle.fit_columns(xty_expected(name)[0], case.targets, positive=case.positive, nn_feature_selection=case.K)
    return _xty_fits[name]


def run_and_check_xty(eng, oracle, name, col_order=None):
    """One launch of the latency kernel with the one-pass X^T y on `eng`, targets in the case's own order; then everything
    the three kernels left in the scratch against the models, and the launch's coefficients against the oracle."""
    case = fm.xty_case(name)
    Xc, Xr, lists, tmap_ref, per_user = xty_expected(name)
    be, torch = eng.be, eng.be.torch
    U, I = Xr.shape
    nnz, tg, n_t, K = int(Xr.nnz), case.targets, len(case.targets), case.K
    eng.set_interactions(Xc, Xr)
    X = eng._X
    X["sqn"] = be.empty((I,), torch.float32)
    be.column_sqnorms(I, X["cptr"], X["cval"], X["sqn"])
    if col_order is not None:
        X["col_order"] = be.to_dev(np.asarray(col_order, dtype=np.int32))
    cfg = _native.FitCfg(np.float32(0.1 * 0.1 * U), np.float32(0.1 * (1.0 - 0.1) * U), np.float32(1e-4), 100, sklearn_seed(43),
                         int(case.positive), K)
    cap = min(K, I)
    d = eng._launch_fit(tg, cfg, cap, min(n_t, 64), "main", FitKnobs(kernel=2), one_pass_xty=True)
    be.synchronize()
    assert be._xty_ws is not None
    ws = be._xty_ws.cpu().numpy()

    # the private layout, mirrored: a drift must fail here, not read garbage
    L = fm.xty_ws_mirror(U, I, nnz, n_t)
    assert L["total"] == int(be.lib.rtrec_slim_xty_workspace_bytes(U, I, nnz, n_t)) and 0 < L["total"] <= ws.size
    i32 = lambda k, n: ws[L[k]:L[k] + 4 * n].view(np.int32)
    f32 = lambda k, n: ws[L[k]:L[k] + 4 * n].view(np.float32)

    # xty_tmap_kernel
    tmap = i32("tmap", I)
    assert np.array_equal(tmap[tg], np.arange(n_t)) and np.array_equal(tmap, tmap_ref)

    # xty_compact_kernel: per user its entries restricted to the targets, stored order; disjoint slices that fill [0, cursor)
    ypos, ylen, cursor = i32("ypos", U), i32("ylen", U), i32("cursor", 2)
    assert np.array_equal(ylen, np.array([len(t) for t, _ in per_user]))
    total = int(ylen.sum())
    assert int(cursor[0]) == total and total <= nnz
    live = np.flatnonzero(ylen > 0)
    o = live[np.argsort(ypos[live], kind="stable")]
    assert np.all(ypos[o] >= 0) and np.array_equal(ypos[o], np.concatenate([[0], np.cumsum(ylen[o])[:-1]]))
    yt, yv = i32("yt", nnz), f32("yv", nnz)
    for u in live.tolist():
        t_ref, v_ref = per_user[u]
        assert np.array_equal(yt[ypos[u]:ypos[u] + ylen[u]], t_ref), f"user {u}"
        assert np.array_equal(bits(yv[ypos[u]:ypos[u] + ylen[u]]), bits(v_ref)), f"user {u}"

    # xty_batch_kernel: per target every non-zero sum, once (append order is not specified)
    cnt = i32("cand_cnt", n_t)
    cand_i, cand_s = i32("cand_i", n_t * I).reshape(n_t, I), f32("cand_s", n_t * I).reshape(n_t, I)
    assert np.array_equal(cnt, np.array([len(ids) for ids, _ in lists])), \
        f"candidate counts differ for targets {tg[np.flatnonzero(cnt != np.array([len(ids) for ids, _ in lists]))[:10]]}"
    for g in range(n_t):
        ids_ref, s_ref = lists[g]
        srt = np.argsort(cand_i[g, :cnt[g]], kind="stable")
        assert np.array_equal(cand_i[g, :cnt[g]][srt], ids_ref), f"candidate items differ for target {tg[g]}"
        assert np.array_equal(bits(cand_s[g, :cnt[g]][srt]), bits(s_ref)), f"X^T y bits differ for target {tg[g]}"

    # ... and what the fit kernel made of them (the scatter of the lists into its own scratch)
    out = [d[k].cpu().numpy() for k in ("items", "coef", "count", "niter")]
    assert_fit_equals_oracle(tg, *out, xty_oracle_fit(oracle, name), K)
    return lists, cnt


@pytest.mark.parametrize("name", fm.XTY_CASES)
def test_one_pass_xty_lists_equal_the_model(fresh_engine, oracle, name):
    """all_ascending: every item, sorted.  subset_shuffled: a strict subset in arbitrary order (tmap < 0 at work), an emptied
    target, a target with one user, users with more than 64 and more than 128 of the targets (the tail loop).  nt1 / nt64 /
    nt65: the lane tail of the flush loop.  cap2048: the most targets the pass takes.  signed: products of either sign, one
    sum that cancels to exactly zero and must be absent.  denormal: products and sums are denormal float32 -- the LDS float
    add must keep them as the reference's add does."""
    case = fm.xty_case(name)
    if name == "subset_shuffled":
        per_user = fm.targets_per_user(case.X, case.targets)
        assert np.count_nonzero(per_user > 64) > 0 and np.count_nonzero(per_user > 128) > 0
    lists, cnt = run_and_check_xty(fresh_engine, oracle, name)
    tg = list(case.targets)
    if name in ("subset_shuffled", "denormal"):
        assert cnt[tg.index(case.notes["empty"])] == 0
        assert cnt.sum() > 1000
    if name == "signed":
        g = tg.index(case.notes["target"])
        assert case.notes["feature"] not in lists[g][0] and cnt[g] > 0


@pytest.mark.parametrize("order", ["reversed", "permuted"])
def test_one_pass_xty_lists_do_not_depend_on_the_column_order(fresh_engine, oracle, order):
    I = fm.xty_case("subset_shuffled").X.shape[1]
    col_order = np.arange(I)[::-1] if order == "reversed" else np.random.default_rng(17).permutation(I)
    run_and_check_xty(fresh_engine, oracle, "subset_shuffled", col_order=col_order)
    assert np.array_equal(fresh_engine._X["col_order"].cpu().numpy(), col_order)


def test_one_pass_xty_on_a_reused_larger_scratch(fresh_engine, oracle):
    """300 targets, then one target on the same engine: the scratch is the larger one, and nothing of the first call shows."""
    run_and_check_xty(fresh_engine, oracle, "all_ascending")
    first = fresh_engine.be._xty_ws
    run_and_check_xty(fresh_engine, oracle, "nt1")
    assert fresh_engine.be._xty_ws is first
    assert first.numel() > 2 * fm.xty_ws_mirror(700, 300, int(fm.xty_case("nt1").X.nnz), 1)["total"]


# ------------------------------------------------------------------------------------------------ B: slot reuse
# name -> (K, positive, signed ratings, environment); the knobs as tests/test_gpu_kernels.py sets them
SLOT_PATHS = {
    "sw": (8, True, False, {"RTREC_AMD_FIT_MODE": "sw", "RTREC_AMD_XTY_BATCH": "0"}),
    "mw": (8, True, False, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_XTY_BATCH": "0"}),
    "mw-colwalk": (8, True, False, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_XTY_BATCH": "0", "RTREC_AMD_COLWALK_MIN": "1"}),
    "mw-xty": (8, True, False, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_XTY_BATCH": "force"}),
    "sw-screen": (8, True, False, {"RTREC_AMD_FIT_MODE": "sw", "RTREC_AMD_XTY_BATCH": "0", "RTREC_AMD_SCREEN_MIN": "1"}),
    "mw-screen": (8, True, False, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_XTY_BATCH": "0", "RTREC_AMD_SCREEN_MIN": "1"}),
    "gram-tracking": (8, True, False, {"RTREC_AMD_FIT_MODE": "sw", "RTREC_AMD_GRAM": "force", "RTREC_AMD_GRAM_ITEMS": "64"}),
    "every-item": (None, True, False, {}),
    "every-item-lane16": (None, True, False, {"RTREC_AMD_LANE_MAX": "16"}),
    "every-item-lane0": (None, True, False, {"RTREC_AMD_LANE_MAX": "0"}),
    "sw-spec-all": (8, True, False, {"RTREC_AMD_FIT_MODE": "sw", "RTREC_AMD_XTY_BATCH": "0", "RTREC_AMD_FOLD": "spec-all"}),
    "mw-spec-all": (8, True, False, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_XTY_BATCH": "0", "RTREC_AMD_FOLD": "spec-all"}),
    "sw-signed": (8, False, True, {"RTREC_AMD_FIT_MODE": "sw", "RTREC_AMD_SCREEN_MIN": "1"}),
    "mw-signed": (8, False, True, {"RTREC_AMD_FIT_MODE": "mw", "RTREC_AMD_SCREEN_MIN": "1", "RTREC_AMD_XTY_BATCH": "force"}),
}

_slot_fits = {}


def slot_oracle_fit(oracle, cols, K, positive, signed):
    key = (tuple(cols.tolist()), K, positive, signed)
    if key not in _slot_fits:
        _slot_fits[key] = oracle.fit_columns(fm.slot_matrix(signed)[0], cols, positive=positive, nn_feature_selection=K)
    return _slot_fits[key]


def logged_fit(eng, cols, n_slots, **kw):
    """eng.fit_columns behind an op log; every launch must have run with exactly `n_slots` slots and all of `cols` -- a
    cached scratch with more slots would be handed back as it is, and the test would prove nothing."""
    log = getattr(eng, "_test_log", None) or OpsLog(eng)
    eng._test_log = log
    before = len(log.calls)
    out = eng.fit_columns(cols, n_slots=n_slots, **kw)
    fits = [c for c in log.calls[before:] if c["op"] == "fit_columns"]
    assert len(fits) >= 1
    assert all(c["n_slots"] == n_slots and c["n_targets"] == len(cols) for c in fits), fits
    return out, fits


@pytest.mark.parametrize("n_slots", [1, 3])
@pytest.mark.parametrize("path", list(SLOT_PATHS))
def test_fit_paths_with_slots_that_serve_many_targets(fresh_engine, oracle, clean_env, path, n_slots):
    """200 targets on 1 and on 3 work slots: every slot's scratch (s, R, stash, touched, candidate arrays) is handed from
    target to target dozens of times, on every path of the fit kernels."""
    K, positive, signed, env = SLOT_PATHS[path]
    for k, v in env.items():
        clean_env.setenv(k, v)
    Xc, Xr = fm.slot_matrix(signed)
    fresh_engine.set_interactions(Xc, Xr)
    cols = np.arange(200)
    (tg, items, coef, count, n_iter), fits = logged_fit(fresh_engine, cols, n_slots, positive=positive, nn_feature_selection=K)
    assert np.array_equal(np.sort(tg), cols)
    if path == "gram-tracking":
        assert fresh_engine._X.get("gram") is not None and all(c["gram"] for c in fits)
    if path in ("mw-xty", "mw-signed"):
        assert all(c["xty_ws"] for c in fits)
    assert_fit_equals_oracle(tg, items, coef, count, n_iter, slot_oracle_fit(oracle, tg, K, positive, signed), K)


@pytest.mark.parametrize("mode", ["shuffle", "gram"])
def test_tolerance_modes_do_not_depend_on_the_slot_count(clean_env, mode):
    """mode="shuffle" / "gram": one slot for all 200 targets against one slot per target, bit for bit -- slots only decide who
    runs when.  (The one-slot-per-target run is held to the oracle by test_fit_tolerance_modes_track_the_exact_solution.)"""
    Xc, Xr = fm.slot_matrix()
    cols = np.arange(200)
    outs = []
    for n_slots in (1, 200):
        eng = SlimEngine(device="cuda:0")
        eng.set_interactions(Xc, Xr)
        out, fits = logged_fit(eng, cols, n_slots, nn_feature_selection=8, mode=mode)
        assert all(c["fast"] == {"shuffle": 1, "gram": 2}[mode] for c in fits)
        outs.append(out)
    (tg1, items1, coef1, count1, nit1), (tg2, items2, coef2, count2, nit2) = outs
    assert np.array_equal(tg1, tg2) and np.array_equal(count1, count2) and np.array_equal(nit1, nit2)
    for t in range(200):
        c = count1[t]
        assert np.array_equal(items1[t, :c], items2[t, :c]), f"column {tg1[t]}"
        assert np.array_equal(bits(coef1[t, :c]), bits(coef2[t, :c])), f"column {tg1[t]}"


@pytest.mark.parametrize("kernel", ["sw", "mw"])
def test_second_call_starts_from_the_scratch_the_first_left(fresh_engine, oracle, clean_env, kernel):
    clean_env.setenv("RTREC_AMD_FIT_MODE", kernel)
    clean_env.setenv("RTREC_AMD_XTY_BATCH", "0")
    Xc, Xr = fm.slot_matrix()
    fresh_engine.set_interactions(Xc, Xr)
    for cols in (np.arange(0, 100), np.arange(100, 200)):
        (tg, items, coef, count, n_iter), _ = logged_fit(fresh_engine, cols, 3, nn_feature_selection=8)
        assert_fit_equals_oracle(tg, items, coef, count, n_iter, slot_oracle_fit(oracle, tg, 8, True, False), 8)
    inits = [c for c in fresh_engine._test_log.calls if c["op"] == "fit_workspace_init"]
    assert len(inits) == 1 and inits[0]["n_slots"] == 3          # one scratch, initialised once, served both calls


# ------------------------------------------------------------------------------------------------ C: norms, Gram matrix
def test_column_sqnorms_chunks_stride_loop_and_value_edges():
    """Column lengths around the 64-entry chunk, 8,192 + 37 columns (the grid is capped at 8,192: the stride loop runs),
    squares that are denormal, that underflow, and a running sum that reaches inf -- against the left-to-right float32 fold."""
    import torch
    from rtrec_amd import ops  # noqa: F401
    cptr, cval = fm.sqnorm_case()
    ref = fm.sqnorm_model(cptr, cval)
    dev = torch.device("cuda:0")
    out = torch.full((len(cptr) - 1,), float("nan"), dtype=torch.float32, device=dev)
    torch.ops.rtrec_amd.column_sqnorms(torch.from_numpy(cptr).to(dev), torch.from_numpy(cval).to(dev), out)
    got = out.cpu().numpy()
    assert np.array_equal(bits(got), bits(ref)), f"columns {np.flatnonzero(bits(got) != bits(ref))[:10]}"


def device_gram(be, Xc, top):
    torch = be.torch
    U, I = Xc.shape
    P = len(top)
    p64 = -(-P // 64) * 64
    ws = be.empty((int(be.lib.rtrec_slim_gram_workspace_bytes(U, P)),), torch.uint8)
    G = torch.full((p64, p64), float("nan"), dtype=torch.float64, device=be.device)
    be.ops.gram_matrix(be.to_dev(Xc.indptr.astype(np.int32)), be.to_dev(Xc.indices.astype(np.int32)),
                       be.to_dev(Xc.data.astype(np.float32)), be.to_dev(np.asarray(top, dtype=np.int32)), ws, G, U, I)
    be.synchronize()
    return G.cpu().numpy()


@pytest.mark.parametrize("n_users", [1, 31, 32, 33, 4095, 4096, 4097, 8193])
def test_gram_matrix_is_exact_where_float64_is(engine, n_users):
    """Ratings that are multiples of 0.5: every float64 sum is exact in any order, so G == XP^T XP with `==` -- around the
    32-row slab and the 4,096-row chunk, for 1 .. 6 column tiles, items in an order that is neither sorted nor by popularity."""
    Xc = fm.gram_exact_matrix(n_users)
    cases = [(n_top, False) for n_top in (1, 63, 64, 65, 321)] + ([(65, True)] if n_users == 4097 else [])
    for n_top, repeat in cases:
        top = fm.gram_top_items(400, n_top, seed=n_top, repeat=repeat)
        G = device_gram(engine.be, Xc, top)
        XP = Xc[:, top].toarray().astype(np.float64)
        assert np.array_equal(G[:n_top, :n_top], XP.T @ XP), (n_top, repeat)
        assert not G[n_top:, :].any() and not G[:, n_top:].any(), (n_top, repeat)
        assert np.array_equal(G, G.T), (n_top, repeat)


def test_gram_matrix_keeps_the_headers_bound_on_float_ratings(engine):
    """include/rtrec_amd.h promises sums with a relative error of about n_users 2^-53.  For non-negative data that is
    |G - ref| <= g ref, g = n 2^-53 / (1 - n 2^-53), n = n_users, whatever the order of the additions; ref is the exactly
    rounded sum of the exact products (math.fsum)."""
    U = 9000
    Xc = fm.both_orientations(interaction_matrix(U, 700, 300000, seed=31))[0]
    top = fm.gram_top_items(700, 100, seed=9)
    G = device_gram(engine.be, Xc, top)
    ref = fm.gram_fsum(Xc[:, top].toarray())
    assert ref.min() >= 0 and np.count_nonzero(ref) > 5000
    assert np.all(np.abs(G[:100, :100] - ref) <= fm.gram_gamma(U) * ref)
    assert not G[100:, :].any() and not G[:, 100:].any() and np.array_equal(G, G.T)


# ------------------------------------------------------------------------------------------------ D: layout builder
@pytest.mark.parametrize("name", fm.SEG_CASES)
def test_native_layout_builder_at_its_boundaries(engine, name):
    """Constructed shards (tests/fit_helper_models.py: seg_case): segment lengths 64 / 65 and odd / even, 32,768 against
    32,769 columns, a single column, a single entry, a shard with gaps, a key_end that is a power of two, label orders with
    4,096 items, value edges of the bound.  The native arrays equal the specification's, and the decoder reads the shard
    back out of them."""
    from rtrec_amd.seg_layout import build_seg_layout, build_seg_layout_native
    case = fm.seg_case(name)
    be = engine.be
    ref = build_seg_layout(case.csc(), case.lo, case.hi, labels=case.labels)
    got = build_seg_layout_native(be, be.to_dev(case.rows), be.to_dev(case.cols), be.to_dev(case.vals), case.n_items, case.lo, case.hi,
                                  be.to_dev(case.labels))
    be.synchronize()
    assert got is not None
    for k in ("sg_T", "sg_n_tiles", "sg_rows", "sg_n_cols"):
        assert got[k] == ref[k], k
    assert got["sg_T"] == case.T
    n_rec, n_list = int(ref["sg_ent"].shape[0]), int(ref["sg_trow"].shape[0])
    host = {k: got[k] for k in ("sg_T", "sg_n_tiles", "sg_rows", "sg_n_cols")}
    for k in ("sg_info", "sg_ptr", "sg_bound", "sg_col_ids", "sg_trow_ptr", "sg_ent", "sg_trow"):
        host[k] = got[k].cpu().numpy()
    assert int(host["sg_ptr"][-1, -1]) == n_rec and int(host["sg_trow_ptr"][-1]) == n_list
    host["sg_ent"], host["sg_trow"] = host["sg_ent"][:n_rec], host["sg_trow"][:n_list]
    for k in ("sg_info", "sg_ptr", "sg_bound", "sg_col_ids", "sg_trow_ptr", "sg_ent", "sg_trow"):
        assert np.array_equal(host[k], np.asarray(ref[k])), k
    found = fm.decode_seg_layout(host, case)
    assert found["n_rec"] == n_rec and found["n_list"] == n_list
    for k, want in case.expect.items():
        assert found["segments"][k] == want, k
    for k, want in case.bounds.items():
        assert found["bounds"][k] == want, k
