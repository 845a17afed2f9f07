"""Tag features for the factor scorer (SLIM.attach_feature_factors, csrc/feature_repr.hip) without a GPU: the definition as a
plain-Python host model with an explicit float32 multiply, then add, and a vectorised one; the proof that the order and the
missing fma are observable (and that scipy's `csr @ table`, which the reference runs, is exactly this chain); the feature-row
builder against the reference's construction mirrored with the FeatureStore; validation; and the model / facade / serving layers
end to end through the CPU stand-in backend with `feature_repr` supplied by the host model.  The kernel is in
tests/test_gpu_feature_repr.py, which shares the checks of this file.

The definition (include/rtrec_amd_ext.h, "FEATURE REPRESENTATIONS"): job r takes row job_rows[r] of a CSR; per component c,
s = +0, then for the stored entries in storage order s = fl(s + fl(v * e[col][c])); entries whose column lies outside the table
are skipped; the bias is the same chain; a stacking layout adds the bias slot and a constant 1; a job without an entry in range
gets +0 everywhere (the constant included) and has = 0."""
import io

import numpy as np
import pytest
import scipy.sparse as sp

from rtrec_amd.engine import SlimEngine
from rtrec_amd.utils.factors import feature_rows, stack_bias
from rtrec_amd.utils.features import FeatureStore
from tests.test_blend_host import value_bits
from tests.test_factor_host import F32, FactorOracleBackend, bits, fitted_model, fma32, host_model_fast

PLAIN, USER, ITEM = 0, 1, 2


# ---------------------------------------------------------------------------------------------- the host models
def _job_span(ptr, n_f_rows, x, nnz):
    if 0 <= x < n_f_rows:
        return min(max(int(ptr[x]), 0), nnz), min(max(int(ptr[x + 1]), 0), nnz)
    return 0, 0


def _slots(layout, dim_e):
    """(bias slot, constant slot, first component slot, width)."""
    return {PLAIN: (-1, -1, 0, dim_e), USER: (0, 1, 2, dim_e + 2), ITEM: (1, 0, 2, dim_e + 2)}[layout]


def repr_plain(ptr, col, val, E, bias=None, layout=PLAIN, job_rows=None, n_jobs=None):
    """THE DEFINITION, one multiply and one add at a time: (out[n_jobs, width] float32, has[n_jobs] uint8)."""
    E = np.asarray(E, F32)
    n_features, dim_e = E.shape
    n_f_rows, nnz = len(ptr) - 1, len(col)
    n_jobs = (len(job_rows) if job_rows is not None else n_f_rows) if n_jobs is None else n_jobs
    b_slot, one_slot, first, width = _slots(layout, dim_e)
    out = np.zeros((n_jobs, width), F32)
    has = np.zeros(n_jobs, np.uint8)
    with np.errstate(all="ignore"):
        for r in range(n_jobs):
            lo, hi = _job_span(ptr, n_f_rows, int(job_rows[r]) if job_rows is not None else r, nnz)
            ks = [k for k in range(lo, hi) if 0 <= col[k] < n_features]
            has[r] = 1 if ks else 0
            for c in range(dim_e):
                s = F32(0.0)
                for k in ks:
                    prod = F32(F32(1.0 if val is None else val[k]) * E[col[k], c])       # rounded once ...
                    s = F32(s + prod)                                                    # ... and once more
                out[r, first + c] = s
            if b_slot >= 0:
                s = F32(0.0)
                for k in ks:
                    s = F32(s + F32(F32(1.0 if val is None else val[k]) * F32(bias[col[k]])))
                out[r, b_slot] = s
                out[r, one_slot] = 1.0 if ks else 0.0
    return out, has


def _padded(ptr, col, val, n_features, job_rows, n_jobs):
    """The in-range entries of every job as rectangular arrays (cols[n_jobs, L], vals, live), storage order kept."""
    n_f_rows, nnz = len(ptr) - 1, len(col)
    n_jobs = (len(job_rows) if job_rows is not None else n_f_rows) if n_jobs is None else n_jobs
    rows = []
    for r in range(n_jobs):
        lo, hi = _job_span(ptr, n_f_rows, int(job_rows[r]) if job_rows is not None else r, nnz)
        k = np.arange(lo, hi)
        rows.append(k[(np.asarray(col)[k] >= 0) & (np.asarray(col)[k] < n_features)] if hi > lo else k)
    L = max([len(k) for k in rows] + [1])
    cols = np.zeros((n_jobs, L), np.int64)
    vals = np.zeros((n_jobs, L), F32)
    live = np.zeros((n_jobs, L), bool)
    for r, k in enumerate(rows):
        cols[r, :len(k)], live[r, :len(k)] = np.asarray(col)[k], True
        vals[r, :len(k)] = 1.0 if val is None else np.asarray(val, F32)[k]
    return cols, vals, live


def repr_fast(ptr, col, val, E, bias=None, layout=PLAIN, job_rows=None, n_jobs=None, step=None, reverse=False):
    """repr_plain, vectorised over jobs and components: entry position by entry position, `step(s, v, e)` per entry (default:
    the float32 product, then the float32 sum).  `reverse` walks a row's entries backwards (for the proof that order shows)."""
    E = np.asarray(E, F32)
    n_features, dim_e = E.shape
    b_slot, one_slot, first, width = _slots(layout, dim_e)
    cols, vals, live = _padded(ptr, col, val, n_features, job_rows, n_jobs)
    if reverse:
        n = live.sum(1)
        idx = np.where(live, n[:, None] - 1 - np.arange(live.shape[1])[None, :], np.arange(live.shape[1])[None, :])
        cols, vals = np.take_along_axis(cols, idx, 1), np.take_along_axis(vals, idx, 1)
    step = step or (lambda s, v, e: (s + (v * e).astype(F32)).astype(F32))
    T = E if b_slot < 0 else np.concatenate([np.asarray(bias, F32).reshape(-1, 1), E], axis=1)
    if n_features == 0:
        T = np.zeros((1, T.shape[1]), F32)
    s = np.zeros((len(cols), T.shape[1]), F32)
    with np.errstate(all="ignore"):
        for k in range(cols.shape[1]):
            nxt = step(s, vals[:, k][:, None], T[np.minimum(cols[:, k], len(T) - 1)])
            s = np.where(live[:, k][:, None], nxt, s)
    has = live.any(1).astype(np.uint8)
    out = np.zeros((len(cols), width), F32)
    if b_slot < 0:
        out[:] = s
    else:
        out[:, b_slot], out[:, one_slot], out[:, first:] = s[:, 0], has.astype(F32), s[:, 1:]
    return out, has


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------- more slots than one trip of the grid
def grid_trip_case(layout, seed=31):
    """65,537 jobs x width 256 = 16,777,472 slots, 256 more than the kernel's 65,536 workgroups x 256 threads: the slots of the
    last job are second trips.  Four feature rows of 3, 0, 1 and 2 entries over a table of five features (PLAIN: dim_e 256, a
    stacking layout: dim_e 254), the job rows drawn per pattern from those four, -1 and 4 (no row); pattern 0 names the full row
    and pattern 384 -- job 65,536's -- the empty one.  (ptr, col, val, E, bias, job rows per pattern)."""
    from tests.test_factor_host import PATTERNS
    rng = np.random.default_rng(seed)
    dim_e = 256 if layout == PLAIN else 254
    ptr = np.array([0, 3, 3, 4, 6], np.int32)
    col = np.array([4, 0, 2, 1, 3, 3], np.int32)
    val = np.array([1.0, 2.0, 0.5, 3.0, 1.0, 1.0], F32)
    E = (rng.standard_normal((5, dim_e)).astype(F32) + F32(3.0) * np.sign(rng.standard_normal((5, dim_e))).astype(F32)).astype(F32)
    bias = (F32(2.0) + rng.random(5).astype(F32)).astype(F32)
    jobs = rng.choice(np.array([0, 1, 2, 3, -1, 4], np.int32), PATTERNS).astype(np.int32)
    jobs[0], jobs[384] = 0, 1
    return ptr, col, val, E, bias, jobs


@pytest.mark.parametrize("layout", [PLAIN, USER])
def test_grid_trip_case_is_the_definition_and_its_last_job_differs_from_the_first(layout):
    from tests.test_factor_host import GRID_CAP, PATTERNS, pattern_of
    ptr, col, val, E, bias, jobs = grid_trip_case(layout)
    want = repr_fast(ptr, col, val, E, bias, layout, jobs)
    plain = repr_plain(ptr, col, val, E, bias, layout, jobs[:40])
    assert same_bits(want[0][:40], plain[0]) and np.array_equal(want[1][:40], plain[1])
    n_jobs, width = GRID_CAP + 1, want[0].shape[1]
    assert width == 256 and n_jobs * width == GRID_CAP * 256 + 256 and pattern_of(n_jobs)[GRID_CAP] == 384 and len(jobs) == PATTERNS
    first, last = 0, pattern_of(n_jobs)[GRID_CAP]
    assert want[1][first] == 1 and want[1][last] == 0
    assert (want[0][first] != want[0][last]).all(), "job 65,536 differs from job 0 in every slot"
    assert set(want[1].tolist()) == {0, 1} and len({want[0][x].tobytes() for x in range(PATTERNS)}) == 4


# ---------------------------------------------------------------------------------------------- order and rounding
def adversarial_case(n_rows=300, n_features=50, dim=12, seed=5):
    """Feature rows of 1..12 entries (sorted distinct columns, values 1, 2 or 3) against a table whose ROWS span 2^-8 .. 2^8 in
    scale with full 24-bit mantissas: every add rounds, so the order, a fused step or a wider accumulator change bits."""
    rng = np.random.default_rng(seed)
    scale = F32(2.0) ** rng.integers(-8, 9, n_features).astype(F32)
    E = (rng.standard_normal((n_features, dim)).astype(F32) * scale[:, None]).astype(F32)
    bias = (rng.standard_normal(n_features).astype(F32) * scale).astype(F32)
    lens = rng.integers(1, 13, n_rows)
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int32)
    col = np.concatenate([np.sort(rng.choice(n_features, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.choice(np.array([1, 1, 1, 2, 3], F32), len(col)).astype(F32)
    return ptr, col, val, E, bias


def test_the_chain_is_scipys_product_and_order_fusion_and_width_show():
    ptr, col, val, E, bias = adversarial_case()
    plain, has = repr_plain(ptr, col, val, E)
    fast, has2 = repr_fast(ptr, col, val, E)
    A = sp.csr_matrix((val, col, ptr), shape=(len(ptr) - 1, len(E)))
    assert same_bits(plain, fast) and same_bits(plain, A @ E) and has.all() and has2.all()
    assert (A @ E).dtype == np.float32
    assert same_bits(repr_plain(ptr, col, val, E, bias, USER)[0][:, 0], A @ bias)              # csr_matvec: the bias chain
    fused = repr_fast(ptr, col, val, E, step=lambda s, v, e: fma32(v, e, s))[0]
    backwards = repr_fast(ptr, col, val, E, reverse=True)[0]
    wide = (sp.csr_matrix((val.astype(np.float64), col, ptr), shape=A.shape) @ E.astype(np.float64)).astype(F32)
    counts = {name: int((bits(x) != bits(plain)).sum()) for name, x in (("fused", fused), ("reversed", backwards), ("float64", wide))}
    print(f"of {plain.size} outputs differ from the unfused ordered float32 chain: {counts}")
    assert all(n > 0 for n in counts.values()), counts
    # a model that is wrong in one of these ways is caught by the comparison the GPU test makes
    for x in (fused, backwards, wide):
        assert not same_bits(x, plain)


def test_stacking_layouts_job_rows_and_skipped_columns():
    ptr, col, val, E, bias = adversarial_case(n_rows=40, n_features=20, dim=5, seed=8)
    col = col.copy()
    col[::7] = 20                     # beyond the table: skipped
    col[3::11] = -2                   # negative: skipped
    ptr = np.r_[ptr, ptr[-1]].astype(np.int32)          # row 40 is empty
    jobs = np.array([0, 40, -1, 41, 7, 7, 39, 1000, 2], np.int32)
    for layout in (PLAIN, USER, ITEM):
        for v in (val, None):
            want, has = repr_plain(ptr, col, v, E, bias, layout, jobs)
            got, has2 = repr_fast(ptr, col, v, E, bias, layout, jobs)
            assert same_bits(want, got) and np.array_equal(has, has2) and has.tolist() == [1, 0, 0, 0, 1, 1, 1, 0, 1]
            assert not want[has == 0].any() and same_bits(want[4], want[5])
    users, items = repr_plain(ptr, col, val, E, bias, USER)[0], repr_plain(ptr, col, val, E, bias, ITEM)[0]
    e, b = repr_plain(ptr, col, val, E)[0], repr_plain(ptr, col, val, E, bias, USER)[0][:, 0]
    P, Q = stack_bias(b[:40], e[:40], b[:40], e[:40])                      # utils/factors.stack_bias is the same stacking
    assert same_bits(users[:40], P) and same_bits(items[:40], Q) and not users[40].any() and not items[40].any()


def test_denormal_products_and_sums_are_kept():
    # every product and every partial sum below is a multiple of 2^-149 under 2^-126: exact as a denormal, zero if flushed
    E = np.array([[2.0 ** -70, 2.0 ** -75], [2.0 ** -72, 2.0 ** -78], [2.0 ** -130, 2.0 ** -149]], F32)
    ptr, col = np.array([0, 3, 5], np.int32), np.array([0, 1, 2, 0, 2], np.int32)
    val = np.array([2.0 ** -70, 2.0 ** -70, 1.0, 2.0 ** -60, 1.0], F32)
    plain, _ = repr_plain(ptr, col, val, E)
    fast, _ = repr_fast(ptr, col, val, E)
    A = sp.csr_matrix((val, col, ptr), shape=(2, 3))
    assert same_bits(plain, fast) and same_bits(plain, A @ E)
    exact = np.array([[2.0 ** -140 + 2.0 ** -142 + 2.0 ** -130, 2.0 ** -145 + 2.0 ** -148 + 2.0 ** -149],
                      [2.0 ** -130 + 2.0 ** -130, 2.0 ** -135 + 2.0 ** -149]])
    assert np.array_equal(plain.astype(np.float64), exact) and (plain > 0).all() and (plain < np.finfo(F32).tiny).all()
    flushed = repr_fast(ptr, col, val, E, step=lambda s, v, e: (s + np.where(abs((v * e).astype(F32)) < np.finfo(F32).tiny, F32(0), (v * e).astype(F32))).astype(F32))[0]
    assert not same_bits(flushed, plain), "the case does not tell a flushed product from a kept one"


# ---------------------------------------------------------------------------------------------- the feature-row builder
def canonical(M):
    M = sp.csr_matrix(M, dtype=np.float32)
    M.sum_duplicates()
    M.sort_indices()
    return M.indptr.tolist(), M.indices.tolist(), M.data.tolist(), M.shape


def reference_hot_rows(store, ids, users_tags, n_ident, ident_known=None):
    """rtrec/models/hybrid.py, _create_user_features(user_ids, users_tags, slice=True), with the project's FeatureStore:
    hstack((identity, build_user_features_matrix(ids, tags, num)))[ids]."""
    num = max(ids) + 1
    feats = store.build_user_features_matrix(list(ids), users_tags=users_tags, num_users=num)
    with_ident = [i for i in ids if ident_known is None or i in ident_known]
    identity = sp.csr_matrix((np.ones(len(with_ident), F32), (with_ident, with_ident)), dtype="float32", shape=(num, n_ident))
    M = identity if feats is None else sp.hstack((identity, feats), format="csr")
    return M[np.array(ids), :]


def reference_cold_rows(store, users_tags, n_ident, n_learned):
    """rtrec/models/hybrid.py, _cold_user_features: a zero identity block, then the learned tags of the request."""
    rows, cols, data = [], [], []
    for r, tags in enumerate(users_tags):
        for t in tags:
            tag_id = store.user_features.index(t)
            if tag_id < 0 or tag_id >= n_learned:
                continue
            rows.append(r), cols.append(tag_id), data.append(1)
    feats = sp.csr_matrix((data, (rows, cols)), shape=(len(users_tags), n_learned), dtype="float32")
    return sp.hstack((sp.csr_matrix((len(users_tags), n_ident), dtype="float32"), feats), format="csr")


def test_feature_rows_are_the_references_construction():
    store = FeatureStore()
    vocab = ["red", "blue", "green", "old", "new"]
    for t in vocab:                                         # the vocabulary in the order of the table's tag rows
        store.put_user_features(99, [t], append=True)
    store.clear_user_features([99])
    store.put_user_features(0, ["blue", "red"])
    store.put_user_features(2, ["new"])
    store.put_user_features(5, ["green", "green", "old"])   # (registered tags are a set)
    n_ident = 7
    tag_cols = {t: n_ident + j for j, t in enumerate(vocab)}
    n_cols = n_ident + len(vocab)
    registered = lambda e: [store.user_features[f] for f in store.user_feature_map.get(e, [])]
    ids = [5, 0, 3, 2, 6]
    # registered tags
    got = feature_rows(ids, [registered(e) for e in ids], tag_cols, n_cols)
    assert canonical(got) == canonical(reference_hot_rows(store, ids, None, n_ident))
    assert got.has_sorted_indices and got.dtype == np.float32 and got.indices.dtype == np.int32
    assert got[0].indices.tolist() == [5, n_ident + 2, n_ident + 3] and got[2].indices.tolist() == [3]
    # request tags replace the registered ones: an empty list, a tag named twice (value 2), tags nobody knows
    req = [["red"], [], ["new", "old", "new"], ["mystery", "blue"], ["mystery"]]
    got = feature_rows(ids, req, tag_cols, n_cols)
    assert canonical(got) == canonical(reference_hot_rows(store, ids, req, n_ident))
    assert got[1].indices.tolist() == [0] and got[2].data.tolist() == [1.0, 1.0, 2.0] and got[2].indices.tolist() == [3, n_ident + 3, n_ident + 4]
    assert got[4].indices.tolist() == [6]
    # the stored order is identity first, then ascending tag columns, whatever the order the tags were named in
    raw = feature_rows([4], [["new", "red", "old"]], tag_cols, n_cols)
    assert raw.indices.tolist() == [4, n_ident, n_ident + 3, n_ident + 4]
    # an entity without an identity row (it joined after the tables were trained): its tags alone
    got = feature_rows([5, -1, 2], [["old"], ["old", "red"], []], tag_cols, n_cols)
    assert canonical(got) == canonical(reference_hot_rows(store, [5, 6, 2], [["old"], ["old", "red"], []], n_ident, ident_known={5, 2}))
    # the cold form: a zero identity block plus the learned tags; a table that learned only the first three tags skips the rest
    cold = [["blue", "new"], [], ["green", "green"], ["mystery"]]
    got = feature_rows([-1] * 4, cold, tag_cols, n_cols)
    assert canonical(got) == canonical(reference_cold_rows(store, cold, n_ident, len(vocab)))
    few = {t: n_ident + j for j, t in enumerate(vocab[:3])}
    got = feature_rows([-1] * 4, cold, few, n_ident + 3)
    assert canonical(got) == canonical(reference_cold_rows(store, cold, n_ident, 3)) and got[0].indices.tolist() == [n_ident + 1]
    with pytest.raises(ValueError):
        feature_rows([0, 1], [[]], tag_cols, n_cols)
    with pytest.raises(ValueError):
        feature_rows([n_cols], [[]], tag_cols, n_cols)


def test_the_feature_store_counts_its_changes_outside_the_pickle():
    import pickle
    store = FeatureStore()
    blank = pickle.dumps(store)
    assert store.version == 0
    store.put_user_features(1, ["a"])
    store.put_item_features(1, ["b"])
    assert store.version == 2
    store.clear_user_features([1])
    store.clear_item_features()
    assert store.version == 4
    back = pickle.loads(pickle.dumps(store))
    assert back.version == 0 and "_version" not in back.__dict__ and list(back.user_features) == ["a"]
    assert pickle.dumps(FeatureStore()) == blank


# ---------------------------------------------------------------------------------------------- model / facade, end to end
class FeatureOracleBackend(FactorOracleBackend):
    """The CPU stand-in with feature_repr from the host model (TEST-ONLY, like its bases)."""

    def feature_repr(self, job_rows, f_csr, table, dim_e, bias, layout, n_jobs, out, row_stride, comp_stride, has):
        import torch
        ptr, col = f_csr[0].numpy(), f_csr[1].numpy()
        val = None if f_csr[2] is None else f_csr[2].numpy()
        got, h = repr_fast(ptr, col, val, table.numpy()[:, :dim_e], None if bias is None else bias.numpy(), layout,
                           None if job_rows is None else job_rows.numpy(), n_jobs)
        flat = out.view(-1)
        r, c = np.meshgrid(np.arange(n_jobs), np.arange(got.shape[1]), indexing="ij")
        flat[torch.from_numpy((r * row_stride + c * comp_stride).ravel())] = torch.from_numpy(got.ravel())
        if has is not None:
            has[:n_jobs] = torch.from_numpy(h)


def cpu_engine():
    return SlimEngine(backend=FeatureOracleBackend())


def feature_model(strings=False, cpu=True):
    """tests/test_factor_host.fitted_model, the CPU form with the stand-in that knows feature_repr."""
    if not cpu:
        return fitted_model(strings, cpu=False)
    from rtrec_amd.models.slim import SLIM
    from tests.test_rerank_host import _batch
    batch = _batch(strings)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.model._engine = cpu_engine()
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    return m, batch


U_TAGS = ["premium", "student", "night", "mobile", "lapsed", "new"]
I_TAGS = ["drama", "comedy", "short", "classic", "live"]


def seeded_tables(batch, dim_e=10, seed=21, strings=False, bias=True):
    """Seeded per-feature tables for the fixture: identity rows for all users but two and all items but three, one id on each
    side the model does not know, six user tags and five item tags; registrations to make before or after the attach."""
    rng = np.random.default_rng(seed)
    users = sorted({u for u, _, _, _ in batch}, key=str)
    items = sorted({i for _, i, _, _ in batch}, key=str)
    no_id_users, no_id_items = [users[5], users[17]], [items[2], items[30], items[31]]
    fu = [u for u in users if u not in no_id_users] + ["a stranger" if strings else 10 ** 8]
    fi = [i for i in items if i not in no_id_items] + ["never seen" if strings else 10 ** 7]
    fu = [fu[j] for j in rng.permutation(len(fu))]
    fi = [fi[j] for j in rng.permutation(len(fi))]
    t = dict(users=fu, items=fi, all_users=users, all_items=items, no_id_users=no_id_users, no_id_items=no_id_items,
             user_table=rng.standard_normal((len(fu) + len(U_TAGS), dim_e)).astype(F32),
             item_table=rng.standard_normal((len(fi) + len(I_TAGS), dim_e)).astype(F32),
             user_bias=(rng.standard_normal(len(fu) + len(U_TAGS)) * 0.3).astype(F32) if bias else None,
             item_bias=(rng.standard_normal(len(fi) + len(I_TAGS)) * 0.3).astype(F32) if bias else None)
    # users[5] has no identity row but a tag (a vector of its tag alone); users[17] has neither (no vector); items[30] likewise
    t["user_reg"] = [(users[0], ["premium", "night"]), (users[3], ["student"]), (users[5], ["mobile", "what is this"]),
                     (users[40], ["lapsed", "new", "premium", "student"]), (users[41], ["what is this"])]
    t["item_reg"] = [(items[0], ["drama"]), (items[1], ["comedy", "short"]), (items[2], ["classic"]), (items[30], ["unheard of"]),
                     (items[20], ["live", "drama", "short"])]
    return t


def attach_tables(m, t):
    return m.attach_feature_factors(t["users"], U_TAGS, t["user_table"], t["items"], I_TAGS, t["item_table"],
                                    user_bias=t["user_bias"], item_bias=t["item_bias"])


def host_vectors(m, t, side, entities, tags=None):
    """What the reference computes for `entities` (raw ids; None: an entity without identity): the feature rows by ITS
    construction (identity + FeatureStore matrix, mirrored above through an independent store in the table's tag order) times
    the table by the host model, stacked.  `tags`: one list per entity replacing the registered ones.  -> (vectors, has)."""
    ids_given, vocab = (t["users"], U_TAGS) if side == "user" else (t["items"], I_TAGS)
    table, bias = t[f"{side}_table"], t[f"{side}_bias"]
    known = m._known_user_id if side == "user" else m.item_ids.get_id
    store = m.feature_store._users if side == "user" else m.feature_store._items
    col_of_raw = {raw: j for j, raw in enumerate(ids_given)}
    rows = []
    for e, raw in enumerate(entities):
        cols = {}
        if raw is not None and raw in col_of_raw:
            cols[col_of_raw[raw]] = 1.0
        if tags is not None:
            named = tags[e]
        else:
            named = [store.vocab[f] for f in store.by_entity.get(known(raw), [])] if raw is not None else []
        for tg in named:
            if tg in vocab:
                c = len(ids_given) + vocab.index(tg)
                cols[c] = cols.get(c, 0.0) + 1.0
        rows.append(sorted(cols.items()))
    ptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    col = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], F32)
    layout = PLAIN if bias is None else (USER if side == "user" else ITEM)
    return repr_plain(ptr, col, val, table, bias, layout) if len(rows) <= 8 else repr_fast(ptr, col, val, table, bias, layout)


def with_host_vectors(m, t, call, user_tags_of=None):
    """`call()` on the same model with attach_factors fed the host-computed vectors of every known entity that has one
    (`user_tags_of`: {raw user: tags replacing the registered ones}); the feature tables are attached again afterwards."""
    users = [u for u in t["all_users"]]
    tags = None if user_tags_of is None else [user_tags_of.get(u, None) for u in users]
    if tags is not None:
        reg = m.feature_store._users
        tags = [tg if tg is not None else [reg.vocab[f] for f in reg.by_entity.get(m._known_user_id(u), [])] for u, tg in zip(users, tags)]
    P, pu = host_vectors(m, t, "user", users, tags)
    Q, qi = host_vectors(m, t, "item", t["all_items"])
    m.attach_factors([u for u, h in zip(users, pu) if h], P[pu != 0], [i for i, h in zip(t["all_items"], qi) if h], Q[qi != 0])
    try:
        return call()
    finally:
        attach_tables(m, t)


def same_lists(got, want, what=""):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype.kind == "f":
            assert np.array_equal(value_bits(g), value_bits(w)), what
        else:
            assert np.array_equal(g, w), what


def check_feature_api(m, batch, strings, make_engine=None):
    """The API checks shared with tests/test_gpu_feature_repr.py (there `m` runs on the device)."""
    from rtrec_amd.models.slim import SLIM
    t = seeded_tables(batch, strings=strings)
    for u, tags in t["user_reg"][:3]:
        m.register_user_feature(u, tags)
    for i, tags in t["item_reg"]:
        m.register_item_feature(i, tags)
    assert attach_tables(m, t) is m and m.has_factors() and m.has_feature_factors()
    cold = ["nobody", "no one"] if strings else [max(t["all_users"]) + 1000, max(t["all_users"]) + 1001]
    users = t["all_users"][:60] + cold[:1] + t["all_users"][60:] + cold[1:]
    hybrid_kw = dict(top_k=8, pool=12, similarity_weight_factor=0.5)
    factor = lambda **kw: m.recommend_factor_batch(users, top_k=9, as_arrays=True, **kw)
    hybrid = lambda **kw: m.recommend_hybrid_batch(users, as_arrays=True, **hybrid_kw, **kw)
    # 1. the registered tags: == attach_factors fed the host-computed stacked vectors
    got_f, got_h = factor(), hybrid()
    E = m.model.engine._F
    index, mask = E["index"].cpu().numpy(), E["mask"].cpu().numpy()
    assert sorted(np.flatnonzero(index < 0).tolist()) == [m._known_user_id(t["all_users"][17])]          # no identity row, no tag
    assert sorted(np.flatnonzero(mask == 0).tolist()) == sorted(m.item_ids.get_id(i) for i in (t["all_items"][30], t["all_items"][31]))
    assert tuple(E["qt"].shape) == (12, m.model.n_items_fitted) and tuple(E["p"].shape) == (m.model.engine.n_users, 12)
    same_lists(got_f, with_host_vectors(m, t, factor), "factor")
    same_lists(got_h, with_host_vectors(m, t, hybrid), "hybrid")
    same_lists(m.recommend_factor_batch(users, top_k=6, filter_interacted=False, candidate_items=t["all_items"][::3], as_arrays=True),
               with_host_vectors(m, t, lambda: m.recommend_factor_batch(users, top_k=6, filter_interacted=False,
                                                                        candidate_items=t["all_items"][::3], as_arrays=True)), "candidates")
    b17 = users.index(t["all_users"][17])
    assert m.recommend_factor_batch(users, top_k=9)[b17] == m.recommend_batch(cold[:1], top_k=9)[0]       # no vector: the cold-start list
    # 2. a tag registered (and one cleared) after the attach changes the next answer to the host model's
    for u, tags in t["user_reg"][3:]:
        m.register_user_feature(u, tags)
    m.clear_user_features([m._known_user_id(t["user_reg"][1][0])])
    m.register_item_feature(t["all_items"][31], ["live"])                                                 # this item gets a vector now
    new_f, new_h = factor(), hybrid()
    b40 = users.index(t["all_users"][40])
    assert not np.array_equal(bits(new_f[1][b40]), bits(got_f[1][b40])), "the registered tags did not reach the vectors"
    same_lists(new_f, with_host_vectors(m, t, factor), "factor after registering")
    same_lists(new_h, with_host_vectors(m, t, hybrid), "hybrid after registering")
    assert m.model.engine._F["mask"].cpu().numpy()[m.item_ids.get_id(t["all_items"][31])] == 1
    # 3. users_tags for known users replace the registered tags; one user twice with different tags in one batch
    ku = [t["all_users"][0], t["all_users"][40], t["all_users"][0], t["all_users"][5], t["all_users"][17], t["all_users"][9], t["all_users"][0]]
    kt = [["lapsed"], [], ["student", "student", "no such tag"], ["new"], [], ["night", "mobile"], ["premium", "night"]]
    got_f = m.recommend_factor_batch(ku, top_k=7, as_arrays=True, users_tags=kt)
    got_h = m.recommend_hybrid_batch(ku, as_arrays=True, users_tags=kt, **hybrid_kw)
    for b, (u, tg) in enumerate(zip(ku, kt)):
        want = with_host_vectors(m, t, lambda: m.recommend_factor_batch([u], top_k=7, as_arrays=True), {u: tg})
        same_lists([a[b:b + 1] for a in got_f], want, ("users_tags, factor", b))
        want = with_host_vectors(m, t, lambda: m.recommend_hybrid_batch([u], as_arrays=True, **hybrid_kw), {u: tg})
        same_lists([a[b:b + 1] for a in got_h], want, ("users_tags, hybrid", b))
    assert not np.array_equal(got_f[0][0], got_f[0][2]) or not np.array_equal(bits(got_f[1][0]), bits(got_f[1][2]))
    same_lists([a[6:7] for a in got_f], [a[:1] for a in m.recommend_factor_batch(ku[:1], top_k=7, as_arrays=True)], "the registered tags again")
    assert m.recommend_factor(ku[0], top_k=7, user_tags=kt[0]) == m.recommend_factor_batch(ku, top_k=7, users_tags=kt)[0]
    assert m.recommend_hybrid(ku[0], user_tags=kt[0], **hybrid_kw) == m.recommend_hybrid_batch(ku, users_tags=kt, **hybrid_kw)[0]
    # 4. unknown users: with tags the top-k of the tag-only vector, unfiltered; without (known) tags what they got before
    cu = [cold[0], t["all_users"][3], cold[1], cold[0], cold[1]]
    ct = [["night", "premium", "night"], ["new"], [], ["no such tag"], ["student"]]
    Q, qi = host_vectors(m, t, "item", t["all_items"])
    Qfull, qmask = np.zeros((m.model.n_items_fitted, Q.shape[1]), F32), np.zeros(m.model.n_items_fitted, np.uint8)
    for i, q, h in zip(t["all_items"], Q, qi):
        Qfull[m.item_ids.get_id(i)], qmask[m.item_ids.get_id(i)] = q, h
    ids, sc, cnt = m.recommend_factor_batch(cu, top_k=7, as_arrays=True, users_tags=ct)
    h_ids, h_val, h_src, h_cnt = m.recommend_hybrid_batch(cu, as_arrays=True, users_tags=ct, **hybrid_kw)
    cold_list = m.recommend_batch(cold[:1], top_k=7)[0]
    for b in (0, 4):
        vec, has = host_vectors(m, t, "user", [None], [ct[b]])
        assert has[0] == 1
        w_ids, w_sc, w_cnt = host_model_fast(vec, Qfull, 12, mask=qmask)                   # every item with a vector competes: no filter
        assert cnt[b] == 7 and np.array_equal(ids[b], w_ids[0, :7]) and np.array_equal(bits(sc[b]), bits(w_sc[0, :7])), b
        assert h_cnt[b] == 8 and np.array_equal(h_ids[b], w_ids[0, :8]) and np.array_equal(bits(h_val[b]), bits(w_sc[0, :8])), b
        assert (h_src[b] == 1).all()
    for b in (2, 3):                                                                       # no tag the table knows: as before
        assert [m.item_ids.get(int(i)) for i in ids[b, :cnt[b]]] == cold_list and (sc[b, :cnt[b]] == 0).all()
        assert h_cnt[b] == 0 and (h_ids[b] == -1).all()
    same_lists([a[1:2] for a in (ids, sc, cnt)],
               with_host_vectors(m, t, lambda: m.recommend_factor_batch(cu[1:2], top_k=7, as_arrays=True), {cu[1]: ct[1]}), "a known user among them")
    few = t["all_items"][::4]
    ids, sc, cnt = m.recommend_factor_batch(cu[:1], top_k=5, as_arrays=True, users_tags=ct[:1], candidate_items=few)
    allowed = np.zeros_like(qmask)
    allowed[[m.item_ids.get_id(i) for i in few]] = 1
    vec, _ = host_vectors(m, t, "user", [None], [ct[0]])
    w_ids, w_sc, _ = host_model_fast(vec, Qfull, 5, mask=qmask & allowed)
    assert np.array_equal(ids[0], w_ids[0]) and np.array_equal(bits(sc[0]), bits(w_sc[0]))
    plain_f = m.recommend_factor_batch(cu, top_k=7)                                         # no users_tags: unknown users as before
    assert plain_f[0] == plain_f[2] == cold_list and m.recommend_hybrid_batch(cu, **hybrid_kw)[0] == []
    # 5. the pickle carries the tables; the loaded model answers alike
    buf = io.BytesIO()
    m.save(buf)
    back = SLIM.loads(buf.getvalue())
    if make_engine is not None:
        back.model._engine = make_engine()
    assert back.has_feature_factors() and sorted(back._factors) == sorted(m._factors)
    for key in ("user_table", "item_table", "user_bias", "item_bias", "user_rows", "user_cols", "item_rows", "item_cols"):
        assert np.array_equal(back._factors[key], m._factors[key])
    same_lists(back.recommend_factor_batch(users, top_k=9, as_arrays=True), new_f, "after the pickle")
    same_lists(back.recommend_hybrid_batch(ku, as_arrays=True, users_tags=kt, **hybrid_kw), got_h, "after the pickle, users_tags")
    assert m.detach_factors() is m and not m.has_factors() and not m.has_feature_factors() and not m.model.engine.has_factors()
    return t, users


@pytest.mark.parametrize("strings", [False, True])
def test_feature_factors_end_to_end_on_the_cpu_stand_in(strings):
    from rtrec_amd.recommender import Recommender
    m, batch = feature_model(strings)
    t, users = check_feature_api(m, batch, strings, make_engine=cpu_engine)
    rec = Recommender(m)
    assert rec.attach_feature_factors(t["users"], U_TAGS, t["user_table"], t["items"], I_TAGS, t["item_table"],
                                      user_bias=t["user_bias"], item_bias=t["item_bias"]) is rec
    tags = [["night"]] * 4
    assert rec.recommend_factor_batch(users[:4], top_k=6, users_tags=tags) == m.recommend_factor_batch(users[:4], top_k=6, users_tags=tags)
    assert rec.recommend_hybrid_batch(users[:4], top_k=6, users_tags=tags) == m.recommend_hybrid_batch(users[:4], top_k=6, users_tags=tags)
    assert rec.recommend_factor(users[2], user_tags=["new"]) == m.recommend_factor(users[2], user_tags=["new"])
    assert rec.recommend_hybrid(users[2], top_k=6, user_tags=["new"]) == m.recommend_hybrid(users[2], top_k=6, user_tags=["new"])
    assert rec.recommend_hybrid(users[2], top_k=6) == m.recommend_hybrid(users[2], top_k=6)
    # tables without biases: the plain layout on both sides
    t2 = seeded_tables(batch, strings=strings, bias=False, dim_e=7)
    attach_tables(m, t2)
    got = m.recommend_factor_batch(users, top_k=5, as_arrays=True)
    assert m.model.engine._F["dim"] == 7
    same_lists(got, with_host_vectors(m, t2, lambda: m.recommend_factor_batch(users, top_k=5, as_arrays=True)), "no bias")


def check_engine_feature_factors(eng, n_items, seed=4):
    """set_feature_factors + factor_topk_rows == set_factors fed the host product of the same inputs: ids, counts, score bits;
    feature_vectors_device and brought vectors (cold jobs, jobs with a row, one row twice).  Shared with the GPU test."""
    from tests.test_factor_host import assert_same
    rng = np.random.default_rng(seed)
    n_users, dim_e, n_uf, n_if = eng.n_users, 6, 40, 30

    def rows_csr(n, n_f, empty):
        lens = rng.integers(1, 6, n)
        lens[empty] = 0
        col = np.concatenate([np.sort(rng.choice(n_f, k, replace=False)) for k in lens] + [np.zeros(0, np.int64)])
        return sp.csr_matrix((rng.choice(np.array([1, 1, 2], F32), len(col)), col.astype(np.int32), np.r_[0, np.cumsum(lens)].astype(np.int32)),
                             shape=(n, n_f))

    Fu, Fi = rows_csr(n_users, n_uf, [1, 7]), rows_csr(n_items, n_if, [0, 5, n_items - 1])
    Eu, Ei = rng.standard_normal((n_uf, dim_e)).astype(F32), rng.standard_normal((n_if, dim_e)).astype(F32)
    bu, bi = rng.standard_normal(n_uf).astype(F32), rng.standard_normal(n_if).astype(F32)
    rows = [0, 1, 3, n_users, -1, 7, 5, n_users - 1]
    for biases in ((bu, bi), (None, None)):
        eng.set_feature_factors(Fu, Eu, Fi, Ei, user_bias=biases[0], item_bias=biases[1])
        got = eng.factor_topk_rows(rows, top_k=9)
        got_open = eng.factor_topk_rows(rows, top_k=9, filter_interacted=False, item_splits=3)
        P, pu = repr_fast(Fu.indptr, Fu.indices, Fu.data, Eu, biases[0], USER if biases[0] is not None else PLAIN)
        Q, qi = repr_fast(Fi.indptr, Fi.indices, Fi.data, Ei, biases[1], ITEM if biases[1] is not None else PLAIN)
        assert same_bits(eng._F["p"].cpu().numpy(), P) and same_bits(eng._F["qt"].cpu().numpy().T, Q)
        assert pu.tolist() == (eng._F["index"].cpu().numpy() >= 0).astype(int).tolist() and qi.tolist() == eng._F["mask"].cpu().numpy().tolist()
        # ad-hoc rows against the kept tables, then scored as brought vectors
        ad = rows_csr(6, n_uf, [2])
        vec, has = eng.feature_vectors_device(ad, "user")
        V, vh = repr_fast(ad.indptr, ad.indices, ad.data, Eu, biases[0], USER if biases[0] is not None else PLAIN)
        assert same_bits(vec.cpu().numpy(), V) and has.cpu().numpy().tolist() == vh.tolist() == [1, 1, 0, 1, 1, 1]
        job_rows = [4, -1, 9, 4, n_users + 3, 4]                        # row 4 three times, two cold jobs, job 2 without a vector
        brought = eng.factor_topk_rows(job_rows, top_k=9, vectors=vec, vector_has=has)
        index = np.where(pu != 0, np.arange(n_users), -1)
        eng.set_factors(P, Q, user_index=index, item_mask=qi)
        assert_same(got, eng.factor_topk_rows(rows, top_k=9), "engine, filtered")
        assert_same(got_open, eng.factor_topk_rows(rows, top_k=9, filter_interacted=False), "engine, open")
        for j, x in enumerate(job_rows):
            if x == 4:                                                  # scored against row 4 of X with the brought vector
                P2 = P.copy()
                P2[4] = V[j]
                eng.set_factors(P2, Q, item_mask=qi)
                want = eng.factor_topk_rows([4], top_k=9)
            else:                                                       # a cold job: nothing filtered
                P2 = P.copy()
                P2[0] = V[j]
                eng.set_factors(P2, Q, user_index=np.where(np.arange(n_users) == 0, 0 if vh[j] else -1, -1), item_mask=qi)
                want = eng.factor_topk_rows([0], top_k=9, filter_interacted=False)
            assert_same([a[j:j + 1] for a in brought], want, ("brought", j))
        assert brought[2][2] == 0
    for bad in (lambda: eng.set_feature_factors(Fu, Eu, Fi, Ei, user_bias=bu), lambda: eng.set_feature_factors(Fu[:-1], Eu, Fi, Ei),
                lambda: eng.set_feature_factors(Fu, Eu, Fi[:-1], Ei), lambda: eng.set_feature_factors(Fu, Eu[:-1], Fi, Ei),
                lambda: eng.set_feature_factors(Fu, Eu, Fi, Ei[:, :-1]), lambda: eng.set_feature_factors(Fu, Eu.astype(np.float64) * 1.1, Fi, Ei),
                lambda: eng.set_feature_factors(Fu, Eu, Fi, Ei, user_bias=bu[:-1], item_bias=bi),
                lambda: eng.set_feature_factors(Fu, np.zeros((n_uf, 255), F32), Fi, np.zeros((n_if, 255), F32), user_bias=bu, item_bias=bi)):
        with pytest.raises(ValueError):
            bad()
    eng.clear_factors()
    with pytest.raises(RuntimeError, match="set_feature_factors"):
        eng.feature_vectors_device(Fu[:2], "user")


def test_engine_set_feature_factors_on_the_cpu_stand_in():
    m, batch = feature_model()
    m.recommend_batch([batch[0][0]])
    check_engine_feature_factors(m.model.engine, m.model.n_items_fitted)


# ---------------------------------------------------------------------------------------------- validation
def test_attach_feature_factors_and_users_tags_refuse_what_they_cannot_serve():
    from rtrec_amd.models.slim import SLIM
    m = SLIM()
    E = lambda n, d=4: np.ones((n, d), F32)
    ok = dict(users=[1, 2], user_tags=["a"], user_table=E(3), items=[5], item_tags=["x", "y"], item_table=E(3))
    assert m.attach_feature_factors(**ok) is m and m.has_feature_factors()
    for kw in (dict(user_table=E(2)), dict(item_table=E(4)), dict(item_table=E(3, 5)), dict(user_table=np.ones(3, F32)),
               dict(user_bias=np.ones(3, F32)), dict(item_bias=np.ones(3, F32)), dict(user_bias=np.ones(2, F32), item_bias=np.ones(3, F32)),
               dict(user_table=E(3, 255), item_table=E(3, 255), user_bias=np.ones(3, F32), item_bias=np.ones(3, F32)),
               dict(user_table=E(3, 257), item_table=E(3, 257)), dict(user_table=E(3, 0), item_table=E(3, 0)),
               dict(user_table=E(3).astype(np.float64) * 1.1)):
        with pytest.raises(ValueError):
            m.attach_feature_factors(**dict(ok, **kw))
    m.attach_feature_factors(**dict(ok, user_table=E(3, 254), item_table=E(3, 254), user_bias=np.ones(3), item_bias=np.ones(3)))   # the limit
    for call in (m.recommend_factor_batch, m.recommend_hybrid_batch):
        with pytest.raises(ValueError, match="one list of tags per user"):
            call([1, 2], users_tags=[["a"]])
        with pytest.raises(ValueError, match="LIST"):
            call([1, 2], users_tags=["a", "b"])
    with pytest.raises(ValueError, match="LIST"):
        m.recommend_factor(1, user_tags="a")
    m.detach_factors()
    for call in (m.recommend_factor_batch, m.recommend_hybrid_batch):
        with pytest.raises(ValueError, match="attach_feature_factors.*no factor model is attached"):
            call([1], users_tags=[["a"]])
    m.attach_factors([1], E(1), [5], E(1))
    for call in (m.recommend_factor_batch, m.recommend_hybrid_batch):
        with pytest.raises(ValueError, match="attach_feature_factors.*finished vector"):
            call([1], users_tags=[["a"]])
    with pytest.raises(ValueError, match="attach_feature_factors"):
        m.recommend_hybrid(1, user_tags=["a"])
    with pytest.raises(RuntimeError, match="fitted"):                  # without users_tags nothing changed
        m.recommend_factor_batch([1])


# ---------------------------------------------------------------------------------------------- serving
def check_serving(m, batch):
    from fastapi import FastAPI
    from fastapi.testclient import TestClient
    from rtrec_amd.serving.app import ModelGate, build_router
    t = seeded_tables(batch)
    app = FastAPI()
    app.include_router(build_router(ModelGate(m)))
    client = TestClient(app)
    ok = {"X-Token": "fake_secret_token"}
    user = t["all_users"][0]
    attach_tables(m, t)
    r = client.post("/recommend_hybrid", json={"user": user, "top_k": 6, "pool": 20, "user_tags": ["night", "student"]}, headers=ok)
    want = m.recommend_hybrid(user, top_k=6, pool=20, user_tags=["night", "student"])
    assert r.status_code == 200 and r.json() == {"user": user, "items": want} and len(want) == 6
    assert want != m.recommend_hybrid(user, top_k=6, pool=20, user_tags=["lapsed"]) or want != m.recommend_hybrid(user, top_k=6, pool=20)
    return client, ok, user


def test_recommend_hybrid_route_takes_user_tags():
    m, batch = feature_model()
    client, ok, user = check_serving(m, batch)
    r = client.post("/recommend_hybrid", json={"user": user, "top_k": 6}, headers=ok)
    assert r.status_code == 200 and r.json()["items"] == m.recommend_hybrid(user, top_k=6)
    stranger = max(u for u, _, _, _ in batch) + 77
    r = client.post("/recommend_hybrid", json={"user": stranger, "top_k": 4, "user_tags": ["premium"]}, headers=ok)
    assert r.status_code == 200 and len(r.json()["items"]) == 4
    f = m._factors
    m.attach_factors([user], np.ones((1, 3), F32), [batch[0][1]], np.ones((1, 3), F32))
    r = client.post("/recommend_hybrid", json={"user": user, "user_tags": ["night"]}, headers=ok)      # finished vectors: the shell's 500
    assert r.status_code == 500 and r.json() == {"detail": "Recommend hybrid failed"}
    m._factors = f


# ---------------------------------------------------------------------------------------------- registration
def test_feature_repr_is_declared_registered_and_exported():
    import ctypes
    import os
    import re
    import torch
    from rtrec_amd import _native, build, ops
    from rtrec_amd.backend import HipBackend
    from tests.test_diverse_host import ROOT, ext_declared_symbols
    assert "rtrec_feature_repr" in ext_declared_symbols() and ext_declared_symbols() == sorted(_native.EXT_EXPORTS)
    assert "rtrec_feature_repr" not in _native.EXPORTS and "feature_repr.hip" in build.SOURCES
    assert "feature_repr" in ops.EXT_OPS and "feature_repr" not in ops.OPS and ops.EXT_EXPORT_OF["feature_repr"] == "rtrec_feature_repr"
    header = open(os.path.join(ROOT, "include", "rtrec_amd_ext.h")).read()
    assert "FEATURE REPRESENTATIONS" in header and "never contracted" in header
    assert hasattr(ctypes.CDLL(build.LIB_PATH), "rtrec_feature_repr") and len(_native.load().rtrec_feature_repr.argtypes) == 18
    assert (_native.FEATURE_PLAIN, _native.FEATURE_USER, _native.FEATURE_ITEM) == (PLAIN, USER, ITEM)
    for name, value in (("PLAIN", 0), ("USER", 1), ("ITEM", 2)):
        assert re.search(rf"#define RTREC_FEATURE_{name} {value}\b", header)
    schema = str(torch.ops.rtrec_amd.feature_repr.default._schema)
    assert schema.startswith("rtrec_amd::feature_repr(") and schema.endswith("-> ()")
    assert re.search(r"Tensor\([a-z]!\) out\b", schema) and re.search(r"Tensor\([a-z]!\)\? has\b", schema), schema
    for arg in ("Tensor? job_rows", "Tensor f_ptr", "Tensor f_col", "Tensor? f_val", "Tensor e", "Tensor? bias", "int dim_e", "int layout",
                "int n_jobs", "int row_stride", "int comp_stride"):
        assert arg in schema, schema
    for name in ("set_feature_factors", "feature_vectors_device"):
        assert callable(getattr(SlimEngine, name))
    assert callable(getattr(HipBackend, "feature_repr"))
    src = open(os.path.join(ROOT, "rtrec_amd", "csrc", "feature_repr.hip")).read()
    assert "feature_repr_kernel" in src and "__fmul_rn" in src and "__fadd_rn" in src and "atomic" not in src.replace("no atomics", "")


def test_the_entry_point_checks_its_arguments_on_the_host():
    from rtrec_amd import _native
    fn = _native.load().rtrec_feature_repr
    one = 1                                                              # any non-NULL address: never dereferenced on these paths

    def args(n_jobs=4, jobs=None, n_f=4, ptr=one, col=one, val=None, nnz=9, e=one, es=12, n_feat=30, dim_e=12, bias=one, layout=1, out=one,
             rs=14, cs=1, has=None):
        return (n_jobs, jobs, n_f, ptr, col, val, nnz, e, es, n_feat, dim_e, bias, layout, out, rs, cs, has, None)

    for kw in (dict(layout=3), dict(layout=-1), dict(dim_e=0), dict(dim_e=255, es=255, rs=257), dict(dim_e=257, es=257, rs=257, layout=0)):
        assert fn(*args(**kw)) == -2, kw
    for kw in (dict(n_jobs=-1), dict(n_f=-1), dict(nnz=-1), dict(n_feat=-1), dict(es=11), dict(rs=13), dict(rs=14, cs=2), dict(rs=1, cs=3),
               dict(rs=0, cs=1), dict(rs=2, cs=2), dict(out=None), dict(ptr=None), dict(col=None), dict(e=None), dict(bias=None)):
        assert fn(*args(**kw)) == -1, kw
    assert fn(*args(n_jobs=0)) == 0 and fn(*args(n_jobs=0, ptr=None, col=None, e=None, bias=None, out=None)) == 0
    assert fn(*args(n_jobs=0, dim_e=254, es=254, rs=256)) == 0 and fn(*args(n_jobs=0, dim_e=256, es=256, rs=256, layout=0)) == 0
    assert fn(*args(n_jobs=0, rs=1, cs=0)) == 0                           # component-major: comp_stride >= n_jobs
