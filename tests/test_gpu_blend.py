"""Blended lists on the GPU (csrc/blend.hip, torch.ops.rtrec_amd.blend_lists, SLIM.recommend_blended_batch) against the host
models of tests/test_blend_host.py: ids, source and count with ==, values by their bits after adding +0.0f (the sign of a zero is
not part of the contract).  The output buffers are poisoned before every call (every slot must be written); both thread counts
per row (waves_per_row 1 and 4) are forced, and 0 (the library's choice) runs beside them."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_blend_host import (F32, FLT_MAX, _expected, assert_same, csr_of_rows, fixture, fixture_by_k, host_model,
                                   host_model_vectorised, random_contacts, random_lists, value_bits)
from tests.test_rerank_host import _batch

pytestmark = pytest.mark.gpu

WAVES = [1, 4, 0]
GRID_CAP = 65536                         # kListMaxGrid of csrc/list_stage.hip.h: workgroups per launch


def run_op(n_items, A, B, keep, weight_b=1.0, contacts=None, k=2.0, mnz=False, waves=0, ka=None, kb=None):
    """torch.ops.rtrec_amd.blend_lists on host arrays: A / B = (ids[n, >= ka], scores[n, >= ka], counts[n]); `contacts` as the host
    models take it (X csr, C csr or None, rows or None)."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to("cuda:0")        # (a copy: the shared fixture arrays are read-only)
    n = np.asarray(A[0]).shape[0]
    ka = np.asarray(A[0]).shape[1] if ka is None else ka
    kb = np.asarray(B[0]).shape[1] if kb is None else kb
    ids = torch.full((n, keep), 12345, dtype=torch.int32, device="cuda:0")                # poisoned: every slot must be written
    value = torch.full((n, keep), 7.0, dtype=torch.float32, device="cuda:0")
    source = torch.full((n, keep), -7, dtype=torch.int32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    rows = xp = xc = cp = cc = cv = None
    if contacts is not None:
        X, C = contacts["X"], contacts.get("C")
        xp, xc = up(X.indptr, np.int32), up(X.indices, np.int32)
        rows = None if contacts.get("rows") is None else up(contacts["rows"], np.int32)
        if C is not None:
            cp, cc, cv = up(C.indptr, np.int32), up(C.indices, np.int32), up(C.data, np.int32)
    torch.ops.rtrec_amd.blend_lists(n_items, up(A[0], np.int32), up(A[1], np.float32), up(A[2], np.int32), ka, up(B[0], np.int32),
                                    up(B[1], np.float32), up(B[2], np.int32), kb, keep, float(F32(weight_b)), contacts is not None, float(k),
                                    bool(mnz), rows, xp, xc, cp, cc, cv, waves, ids, value, source, count)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), value.cpu().numpy(), source.cpu().numpy(), count.cpu().numpy()


def cut(want, keep):
    """The host model's answer at a smaller keep: the head of the ranking."""
    return want[0][:, :keep], want[1][:, :keep], want[2][:, :keep], np.minimum(want[3], keep)


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def fixture_want():
    f = fixture()
    whole = f["A"][0].shape[1] + f["B"][0].shape[1]
    return f, whole, fixture_by_k(host_model_vectorised, whole), fixture_by_k(host_model_vectorised, whole, mnz=True)


@pytest.mark.parametrize("waves", WAVES)
def test_fixture_cases_equal_the_host_model_and_the_reference(fixture_want, waves):
    f, whole, want, want_mnz = fixture_want
    op = lambda n_items, A, B, keep, **kw: run_op(n_items, A, B, keep, waves=waves, **kw)
    got = fixture_by_k(op, whole)
    assert_same(got, want, f"fixture waves={waves}")
    for r, ref in enumerate(f["want"]):
        assert got[0][r, :got[3][r]].tolist() == ref, f"case {r}: not the reference's order"
    assert_same(fixture_by_k(op, 10), cut(want, 10), f"fixture top-10 waves={waves}")
    assert_same(fixture_by_k(op, whole, mnz=True), want_mnz, f"fixture mnz waves={waves}")


# ---------------------------------------------------------------------------------------------- every length
N_ITEMS = 64


@pytest.mark.parametrize("ka,kb", [(1, 1), (2, 1), (1, 2), (63, 64), (64, 65), (65, 63), (255, 256), (256, 257), (257, 255), (1024, 1),
                                   (1, 1024), (1024, 1024)])
def test_lists_of_every_length(ka, kb):
    """Eight rows of seeded lists over 64 items (ids repeat inside and across the lists): effective lengths 0, 1 and full on either
    side, a list cut by an invalid id and one cut by an invalid score, counts beyond the width, strides wider than the lists; keep
    1, a value between and ka + kb; a constant weight, contacts with and without counts, and mnz; all three wave settings."""
    rng = np.random.default_rng(1000 * ka + kb)
    n = 8
    ids_a, ids_b = rng.integers(0, N_ITEMS, (n, ka)).astype(np.int32), rng.integers(0, N_ITEMS, (n, kb)).astype(np.int32)
    sc_a = -np.sort(-rng.standard_normal((n, ka)).astype(F32), axis=1)
    sc_b = -np.sort(-(rng.random((n, kb)) * 50).astype(F32), axis=1)
    cnt_a, cnt_b = np.full(n, ka, np.int32), np.full(n, kb, np.int32)
    cnt_a[0], cnt_b[1], cnt_a[2], cnt_b[2], cnt_a[3], cnt_b[3] = 0, 0, 1, 1, ka + 5, -3
    ids_a[4, ka // 2], sc_b[5, kb // 2] = N_ITEMS, np.nan                 # cut at the first invalid position (position 0 at length 1)
    ids_b[6, kb - 1], sc_a[6, ka - 1] = -1, -FLT_MAX
    wide = lambda a, extra, fill: np.concatenate([a, np.full((n, extra), fill, a.dtype)], axis=1)
    A = (ids_a, sc_a, cnt_a)
    B = (ids_b, sc_b, cnt_b)
    A_wide = (wide(ids_a, 3, 1), wide(sc_a, 5, 9.0), cnt_a)               # valid-looking entries behind the list: never read
    B_wide = (wide(ids_b, 2, 2), wide(sc_b, 1, 9.0), cnt_b)
    con = random_contacts(rng, n, 5, N_ITEMS)
    whole = ka + kb
    for name, kw in (("constant", dict(weight_b=0.7)), ("contacts", dict(contacts=con, k=0.5)),
                     ("membership", dict(contacts=dict(con, C=None), k=2.0)), ("mnz", dict(weight_b=1.0, mnz=True))):
        want = host_model_vectorised(N_ITEMS, A, B, whole, **kw)
        if name == "constant":
            assert want[3][0] > 0 and want[3][1] > 0 and want[3][7] == len(set(ids_a[7].tolist()) | set(ids_b[7].tolist()))
        for keep in sorted({1, (whole + 1) // 2, whole}):
            for waves in WAVES:
                got = run_op(N_ITEMS, A_wide, B_wide, keep, waves=waves, ka=ka, kb=kb, **kw)
                assert_same(got, cut(want, keep), f"ka={ka} kb={kb} {name} keep={keep} waves={waves}")


def test_two_full_lists_of_distinct_items_fill_the_union():
    """ka = kb = 1024 over 4,096 items, no id twice inside a list: unions of up to 2,048 entries, ranked with many equal values
    (scores drawn from 16 levels)."""
    rng = np.random.default_rng(77)
    n, I = 3, 4096
    A = (np.stack([rng.permutation(I)[:1024] for _ in range(n)]).astype(np.int32), -np.sort(-rng.integers(0, 16, (n, 1024)).astype(F32), axis=1),
         np.full(n, 1024, np.int32))
    B = (np.stack([rng.permutation(I)[:1024] for _ in range(n)]).astype(np.int32), -np.sort(-rng.integers(0, 16, (n, 1024)).astype(F32), axis=1),
         np.full(n, 1024, np.int32))
    want = host_model_vectorised(I, A, B, 2048, weight_b=0.5)
    assert want[3].min() > 1700 and (np.diff(want[1][0, :want[3][0]]) == 0).sum() > 1000
    assert_same(host_model(I, tuple(a[:1] for a in A), tuple(b[:1] for b in B), 2048, weight_b=0.5), tuple(w[:1] for w in want), "host models")
    for waves in WAVES:
        assert_same(run_op(I, A, B, 2048, weight_b=0.5, waves=waves), want, f"full union waves={waves}")


# ---------------------------------------------------------------------------------------------- hand-written cases
def hand_inputs():
    d = np.float32(1e-45)
    X = csr_of_rows([[1, 2, 3]], 8)
    C = csr_of_rows([[2, 3, 5]], 8, [{2: 4, 3: 0, 5: 2}])
    con = lambda rows=None, C_=C: dict(X=X, C=C_, rows=rows)
    return [
        ("all equal", [3, 4, 1], [2, 2, 2], [5, 6], [7, 7], dict(weight_b=1.0)),
        ("one denormal apart", [1, 2], [2 * d, d], [2, 3], [d, 0.0], dict(weight_b=1.0)),
        ("denormal scores, mnz", [1, 2, 3], [3 * d, 2 * d, d], [3, 1], [2 * d, d], dict(weight_b=0.5, mnz=True)),
        ("duplicates: first position, last value", [1, 2, 1], [3, 2, 1], [5, 6, 5], [3, 2, 1], dict(weight_b=1.0)),
        ("separate roundings", [4, 2], [5, 1], [2, 4, 3], [7, 3, 1], dict(weight_b=0.3)),
        ("mnz", [4, 2], [5, 1], [2, 4, 3], [7, 3, 1], dict(weight_b=0.3, mnz=True)),
        ("contacts k=2", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(), k=2.0)),
        ("contacts k=0.5", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(), k=0.5)),
        ("contacts k=0", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(), k=0.0)),
        ("no count CSR", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(C_=None), k=2.0)),
        ("a row outside X", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(rows=[7]), k=2.0)),
        ("a negative row id", [0], [1.0], [1, 2, 3, 5, 6], [5, 5, 5, 5, 1], dict(contacts=con(rows=[-1]), k=2.0)),
        ("-0.0 ties with +0.0", [1, 2], [-0.0, 0.0], [3], [1.0], dict(weight_b=0.0)),
        ("an overflowing range: NaN is never listed", [1, 2, 3], [3e38, 0.0, -3e38], [3, 4], [3e38, -3e38], dict(weight_b=1.0)),
        ("cut by NaN", [1, 2, 3], [3, np.nan, 0.5], [5], [1.0], dict(weight_b=1.0)),
        ("cut by inf", [1, 2, 3], [np.inf, 2, 0.5], [5, 6], [1.0, -np.inf], dict(weight_b=1.0)),
        ("cut at -FLT_MAX, kept just above", [1, 2, 3], [3, np.nextafter(-FLT_MAX, F32(0)), -FLT_MAX], [5, 6], [1.0, -FLT_MAX], dict(weight_b=1.0)),
        ("two empty lists", [9], [1.0], [-1], [1.0], dict(weight_b=1.0)),
    ]


@pytest.mark.parametrize("waves", WAVES)
def test_hand_written_cases(waves):
    for name, a_ids, a_sc, b_ids, b_sc, kw in hand_inputs():
        A = (np.array([a_ids], np.int32), np.array([a_sc], F32), [len(a_ids)])
        B = (np.array([b_ids], np.int32), np.array([b_sc], F32), [len(b_ids)])
        keep = len(a_ids) + len(b_ids)
        want = host_model(8, A, B, keep, **kw)
        assert_same(run_op(8, A, B, keep, waves=waves, **kw), want, f"{name} waves={waves}")
    # what the cases are there for
    name, a_ids, a_sc, b_ids, b_sc, kw = hand_inputs()[1]
    want = host_model(8, (np.array([a_ids], np.int32), np.array([a_sc], F32), [2]), (np.array([b_ids], np.int32), np.array([b_sc], F32), [2]), 4, **kw)
    assert want[0][0].tolist() == [1, 2, 3, -1] and 0 < want[1][0, 0] < 1e-30 and want[1][0, 1] > 0


# ---------------------------------------------------------------------------------------------- contacts
@pytest.mark.parametrize("waves", WAVES)
def test_count_rows_of_0_1_and_200_entries(waves):
    """Over 256 items: row 0 of the count CSR is empty, row 1 holds one pair, row 2 holds 200; X's rows hold 0, 100 and 250 items.
    Every list row names one of them, a row beyond X, or a negative one."""
    rng = np.random.default_rng(9)
    I = 256
    own = [[], sorted(rng.permutation(I)[:100].tolist()), sorted(rng.permutation(I)[:250].tolist())]
    counted = [{}, {int(own[1][7]): 3}, {int(i): int(rng.integers(0, 9)) for i in rng.permutation(I)[:200]}]
    X, C = csr_of_rows(own, I), csr_of_rows([list(c) for c in counted], I, counted)
    assert np.diff(C.indptr).tolist() == [0, 1, 200]
    n = 40
    A, B = random_lists(rng, n, 12, 20, I)
    B[0][:, 0] = own[1][7]                                                # the one counted pair of row 1 is asked for
    rows = rng.integers(-1, 4, n)
    for con in (dict(X=X, C=C, rows=rows), dict(X=X, C=None, rows=rows), dict(X=X, C=C, rows=None)):
        for k in (2.0, 0.5):
            want = host_model_vectorised(I, A, B, 32, contacts=con, k=k)
            assert_same(run_op(I, A, B, 32, contacts=con, k=k, waves=waves), want, f"contacts k={k} waves={waves}")
    assert_same(host_model(I, A, B, 32, contacts=dict(X=X, C=C, rows=rows), k=0.5), host_model_vectorised(I, A, B, 32, contacts=dict(X=X, C=C, rows=rows), k=0.5), "host models")


# ---------------------------------------------------------------------------------------------- more rows than workgroups
def test_one_row_more_than_the_grid():
    rng = np.random.default_rng(65537)
    n, I = GRID_CAP + 1, 50
    A = (rng.integers(-1, I + 1, (n, 2)).astype(np.int32), rng.random((n, 2)).astype(F32), rng.integers(0, 3, n).astype(np.int32))
    B = (rng.integers(-1, I + 1, (n, 2)).astype(np.int32), rng.random((n, 2)).astype(F32), rng.integers(0, 3, n).astype(np.int32))
    want = host_model_vectorised(I, A, B, 3, weight_b=0.5)
    assert sorted(np.unique(want[3]).tolist()) == [0, 1, 2, 3] and want[3][-1] + want[3][GRID_CAP - 1] > 0
    assert_same(run_op(I, A, B, 3, weight_b=0.5), want, "65,537 rows")


# ---------------------------------------------------------------------------------------------- the API on the device
@pytest.mark.parametrize("strings", [False, True])
def test_recommend_blended_batch_equals_the_host_model_fed_with_recommend_batch(strings):
    from rtrec_amd import SLIM
    batch = _batch(strings)
    m = SLIM(min_value=0, max_value=15, nn_feature_selection=5)
    m.fit(batch, progress_bar=False)
    m.model.item_similarity = sp.csc_matrix(m.model.item_similarity, dtype=np.float32)
    rng = np.random.default_rng(8)
    known_users = sorted({u for u, _, _, _ in batch}, key=str)
    known_items = sorted({i for _, i, _, _ in batch}, key=str)
    cold = "nobody" if strings else max(known_users) + 1000
    unknown = "never seen" if strings else 10 ** 7
    users = known_users[:40] + [cold, known_users[3]]
    plain = m.recommend_batch(users, top_k=8)
    others, other_scores = [], []
    for b, u in enumerate(users):
        row = list(plain[b][:4]) + [known_items[j] for j in rng.permutation(len(known_items))[:6]] + [unknown]
        others.append([row[j] for j in rng.permutation(len(row))])
        other_scores.append((-np.sort(-rng.random(len(row)))).astype(F32).tolist())
    counts = [(u, plain[b][j], int(rng.integers(1, 5))) for b, u in enumerate(users[:40]) for j in range(0, len(plain[b]), 2)]
    for kw in (dict(top_k=8), dict(top_k=8, contact_counts=counts), dict(top_k=5, pool=12, contact_counts=counts, similarity_weight_factor=0.5),
               dict(top_k=8, weighting=0.6, mnz=True), dict(top_k=6, contact_counts=counts, filter_interacted=False)):
        want = _expected(m, users, others, other_scores, kw["top_k"], kw.get("pool", kw["top_k"]), kw.get("contact_counts"),
                         kw.get("similarity_weight_factor", 2.0), kw.get("weighting", "contacts"), kw.get("mnz", False),
                         kw.get("filter_interacted", True))
        assert m.recommend_blended_batch(users, others, other_scores, **kw) == [w[0] for w in want], kw
        ids, value, source, cnt = m.recommend_blended_batch(users, others, other_scores, as_arrays=True, **kw)
        for b, (w_ids, w_val, w_src) in enumerate(want):
            n = int(cnt[b])
            assert n == len(w_ids) and source[b, :n].tolist() == w_src and np.array_equal(value_bits(value[b, :n]), value_bits(w_val)), (kw, b)
    assert m.recommend_blended(users[2], others[2], other_scores[2], top_k=8, contact_counts=counts) == \
        m.recommend_blended_batch(users, others, other_scores, top_k=8, contact_counts=counts)[2]
    assert m.recommend_blended_batch(users, others, other_scores, top_k=8, contact_counts=counts) != m.recommend_blended_batch(users, others, other_scores, top_k=8)
    pairs = m.blend_batch(others[:5], other_scores[:5], [plain[b] for b in range(5)], [np.linspace(2, 1, len(plain[b])).tolist() for b in range(5)],
                          top_k=7, weight=0.8)
    assert all(len(p) == 7 and unknown not in [i for i, _ in p] for p in pairs)


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    op = torch.ops.rtrec_amd.blend_lists
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(ka=2, kb=3, keep=2, weight_b=1.0, contacts=False, k=2.0, waves=0, **kw):
        a = dict(a_ids=i32(3, ka), a_scores=f32(3, ka), a_counts=i32(3), b_ids=i32(3, kb), b_scores=f32(3, kb), b_counts=i32(3), rows=None,
                 xb_ptr=i32(5), xb_col=i32(4), cn_ptr=None, cn_col=None, cn_val=None, ids=i32(3, max(keep, 0)), value=f32(3, max(keep, 0)),
                 source=i32(3, max(keep, 0)), count=i32(3))
        a.update(kw)
        op(6, a["a_ids"], a["a_scores"], a["a_counts"], ka, a["b_ids"], a["b_scores"], a["b_counts"], kb, keep, weight_b, contacts, k, False,
           a["rows"], a["xb_ptr"], a["xb_col"], a["cn_ptr"], a["cn_col"], a["cn_val"], waves, a["ids"], a["value"], a["source"], a["count"])

    call()                                                               # the well-formed calls run
    call(ka=1024, kb=1024, keep=2048, waves=4)
    call(ka=1024, kb=1, keep=1, waves=1)
    call(contacts=True, rows=i32(3), cn_ptr=i32(5), cn_col=i32(2), cn_val=i32(2))
    call(contacts=True, k=0.0)
    call(xb_ptr=None, xb_col=None)                                       # a constant weight reads no X
    for kw in (dict(ka=0), dict(ka=1025), dict(kb=0), dict(kb=1025), dict(keep=0), dict(keep=6), dict(waves=2), dict(weight_b=-0.1),
               dict(weight_b=float("nan")), dict(k=-1.0), dict(k=float("nan"))):
        with pytest.raises(RuntimeError, match="must lie in|must be 0, 1 or 4"):
            call(**kw)
    bad = [dict(a_ids=torch.zeros((3, 2), dtype=torch.int64, device=dev)), dict(b_scores=torch.zeros((3, 3), dtype=torch.float64, device=dev)),
           dict(value=torch.zeros((3, 2), dtype=torch.float64, device=dev)), dict(source=torch.zeros((3, 2), dtype=torch.int64, device=dev)),
           dict(a_counts=torch.zeros(3, dtype=torch.int32)), dict(ids=torch.zeros((3, 2), dtype=torch.int32)), dict(a_ids=i32(3, 4)[:, ::2]),
           dict(a_ids=i32(3, 1)), dict(b_scores=f32(3, 2)), dict(b_ids=i32(2, 3)), dict(b_counts=i32(2)), dict(ids=i32(3, 3)), dict(count=i32(2)),
           dict(contacts=True, xb_ptr=None), dict(contacts=True, rows=i32(2)), dict(contacts=True, cn_ptr=i32(4), cn_col=i32(2), cn_val=i32(2)),
           dict(contacts=True, cn_ptr=i32(5), cn_col=i32(2), cn_val=i32(3)), dict(contacts=True, cn_ptr=i32(5)),
           dict(contacts=True, xb_col=torch.zeros(4, dtype=torch.int64, device=dev)),
           dict(contacts=True, cn_ptr=i32(5), cn_col=i32(2), cn_val=f32(2))]
    for kw in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            call(**kw)
    torch.cuda.synchronize()
