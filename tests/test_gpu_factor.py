"""The factor scorer on the GPU (csrc/factor_topk.hip, torch.ops.rtrec_amd.factor_topk, SLIM.recommend_factor_batch /
recommend_hybrid_batch) against the host models of tests/test_factor_host.py: ids and counts with ==, scores by their bits after
adding +0.0f (the sign of a zero is not part of the contract).  The output buffers are poisoned before every call (every slot must
be written).  The kernel computes a score with the f32-input MFMA; the rounding-order test is what says that this is the fmaf
chain of the contract, bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_factor_host import (CLASS_DIMS, F32, GRID_CAP, HYBRID_CASES, assert_same, check_factor_and_hybrid, class_edge_case, filter_case,
                                    fitted_model, host_model_fast, host_model_plain, host_scores, merge_trip_answer, merge_trip_case, operand_case,
                                    rounding_vectors, tiled)

pytestmark = pytest.mark.gpu


def run_op(P, Q, top_k, rows=None, p_index=None, n_x_rows=None, X=None, mask=None, filter_interacted=False, splits=0, pad=0, seed=0,
           pad_value=None):
    """torch.ops.rtrec_amd.factor_topk on host arrays, as the host models take them.  `pad` > 0: both strides are wider than the
    widths (and qt has rows beyond dim), with seeded values behind them, or `pad_value` in all three places (P's columns beyond
    dim, qt's rows beyond dim, qt's columns beyond n_items): a finite pad times a zero operand leaves a score as it is, a NaN
    does not."""
    import torch
    from rtrec_amd import ops  # noqa: F401  (registers torch.ops.rtrec_amd.*)
    P, Q = np.asarray(P, F32), np.asarray(Q, F32)
    dim, n_items = P.shape[1], len(Q)
    rng = np.random.default_rng(seed)
    behind = lambda *shape: rng.standard_normal(shape).astype(F32) * 100 if pad_value is None else np.full(shape, pad_value, F32)
    Pd = np.concatenate([P, behind(len(P), pad)], axis=1) if pad else P
    Qt = np.ascontiguousarray(Q.T)
    if pad:
        Qt = np.concatenate([Qt, behind(dim, pad)], axis=1)
        Qt = np.concatenate([Qt, behind(pad, n_items + pad)], axis=0)
    if dim == 0 or Qt.shape[1] == 0:
        Qt = np.zeros((max(dim, 1), max(Qt.shape[1], 1)), F32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda:0")
    n = len(P) if rows is None else len(rows)
    n_x_rows = (X.shape[0] if X is not None else len(P)) if n_x_rows is None else n_x_rows
    ids = torch.full((n, top_k), 12345, dtype=torch.int32, device="cuda:0")               # poisoned: every slot must be written
    scores = torch.full((n, top_k), 7.0, dtype=torch.float32, device="cuda:0")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    xp = xc = None
    if filter_interacted:
        xp, xc = up(X.indptr, np.int32), up(X.indices, np.int32)
    s_eff = splits if splits else 64
    ws = torch.empty((n * s_eff * (top_k * 8 + 4),), dtype=torch.uint8, device="cuda:0") if s_eff > 1 else None
    torch.ops.rtrec_amd.factor_topk(None if rows is None else up(rows, np.int32), None if p_index is None else up(p_index, np.int32),
                                    n_x_rows, up(Pd, np.float32), up(Qt, np.float32), n_items, dim,
                                    None if mask is None else up(np.asarray(mask) != 0, np.uint8), xp, xc, bool(filter_interacted), top_k,
                                    splits, ids, scores, count, ws)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


def cut(want, rows, top_k):
    """The host model's answer for the first `rows` jobs at a smaller top_k: the head of the ranking."""
    return want[0][:rows, :top_k], want[1][:rows, :top_k], np.minimum(want[2][:rows], top_k)


# ---------------------------------------------------------------------------------------------- 1. the operand map
def test_identity_vectors_against_an_asymmetric_integer_matrix():
    """A swapped row / column of the tile or a permuted k would show: P = unit vectors makes score(u, i) = Q[i, u % 32], and the
    transposed roles make it P[u, i % 32]; the integer matrix is not symmetric in any pair of its indices."""
    dim, n_items, n_users = 32, 40, 33
    i, c = np.meshgrid(np.arange(n_items), np.arange(dim), indexing="ij")
    Q = (i * 37 + c * 3 + (i * c) % 5 - 400).astype(F32)
    P = np.zeros((n_users, dim), F32)
    P[np.arange(n_users), np.arange(n_users) % dim] = 1
    got = run_op(P, Q, n_items, splits=1)
    assert_same(got, host_model_fast(P, Q, n_items), "P = I")
    for u in (0, 5, 31, 32):
        assert np.array_equal(np.sort(got[1][u]), np.sort(Q[:, u % dim])) and got[1][u, 0] == Q[:, u % dim].max()
    u, c = np.meshgrid(np.arange(n_users), np.arange(dim), indexing="ij")
    P2 = (u * 29 - c * 7 + (u * c) % 3).astype(F32)
    Q2 = np.zeros((n_items, dim), F32)
    Q2[np.arange(n_items), np.arange(n_items) % dim] = 1
    assert_same(run_op(P2, Q2, n_items, splits=1), host_model_fast(P2, Q2, n_items), "Q = I")
    assert_same(run_op(P2, Q2, n_items, splits=2), host_model_fast(P2, Q2, n_items), "Q = I, two chunks")


# ---------------------------------------------------------------------------------------------- 2. the rounding order
@pytest.mark.parametrize("dim", [1, 2, 3, 12, 13, 64, 255, 256] + CLASS_DIMS)
def test_scores_are_the_ascending_fmaf_chain_bit_for_bit(dim):
    """Decides between the MFMA and a VALU chain: every one of the 64 x 96 scores must carry the bits of
    fmaf(p[dim-1], q[dim-1], ... fmaf(p[0], q[0], +0)) on vectors where another order, an unfused multiply or a wider
    accumulator changes them (tests/test_factor_host.py shows that they do)."""
    P, Q = rounding_vectors(64, 96, dim, seed=dim)
    want = host_model_fast(P, Q, 96)
    got = run_op(P, Q, 96, splits=1)
    S = host_scores(P, Q)
    listed = np.zeros_like(S, dtype=bool)
    for r in range(64):
        listed[r, got[0][r, :got[2][r]]] = True
    print(f"dim {dim}: {int(listed.sum())} scores listed, {int(np.isnan(S).sum())} NaN")
    assert_same(got, want, f"dim {dim}")


# ---------------------------------------------------------------------------------------------- 3. every edge of the tiling
@pytest.fixture(scope="module")
def edge_vectors():
    rng = np.random.default_rng(33)
    return rng.standard_normal((130, 5)).astype(F32), rng.standard_normal((1000, 5)).astype(F32)


@pytest.mark.parametrize("n_items", [1, 31, 32, 33, 159, 160, 161, 511, 512, 513, 1000])
def test_every_edge_of_the_tiling(edge_vectors, n_items):
    """Catalogues around the tile (32) and around the chunk widths of 1,000 items cut in 7 (160) and in 2 (512); job counts
    around the block (32); every k-class, top_k beyond the catalogue included; every split count gives the same answer."""
    P, Q = edge_vectors[0], edge_vectors[1][:n_items]
    want = host_model_fast(P, Q, 128)
    for n_rows in (1, 31, 32, 33, 130):
        for top_k in (1, 10, 16, 17, 64, 65, 128):
            for splits in (0, 1, 2, 7):
                assert_same(run_op(P[:n_rows], Q, top_k, splits=splits), cut(want, n_rows, top_k), (n_items, n_rows, top_k, splits))


@pytest.mark.parametrize("dim", [17, 65])
def test_both_class_choices_change_in_one_call(dim):
    """200 items x 40 jobs one past a dim class (17 > 16, 65 > 64) at top_k one past a k class (17 > 16, 65 > 64), in one chunk
    and in three; the last component decides every list (tests/test_factor_host.py), so a rule that sends dim 17 to the 16-class
    or dim 65 to the 64-class shows in every job."""
    P, Q = class_edge_case(dim)
    want = host_model_fast(P, Q, 65)
    for top_k in (17, 65):
        for splits in (1, 3):
            assert_same(run_op(P, Q, top_k, splits=splits), cut(want, 40, top_k), (dim, top_k, splits))


# ---------------------------------------------------------------------------------------------- 3b. NaN behind dim and behind n_items
NAN_PAD = 32            # rows of qt behind dim: enough for every row a whole group of 16 k-steps could name (2 x 16 x 2 = 64 at dim 33)


@pytest.mark.parametrize("dim", [13, 33])
def test_nan_padding_is_never_read_into_a_score(dim):
    """The operand-map case and the filter / mask / rows case with NaN in P's columns beyond dim, in qt's rows beyond dim and in
    qt's columns beyond n_items: a load that misses its guard multiplies a finite pad by a zero operand and changes nothing, a
    NaN pad poisons the score.  Odd dims: the last k-step has a zero half.  The expected answer is the unpadded one."""
    P, Q, P2, Q2 = operand_case(dim)
    n_items = len(Q)
    nan = dict(pad=NAN_PAD, pad_value=np.nan)
    want = host_model_fast(P, Q, n_items)
    for splits in (1, 2):
        assert_same(run_op(P, Q, n_items, splits=splits, **nan), want, ("P = I", splits))
        assert_same(run_op(P2, Q2, n_items, splits=splits, **nan), host_model_fast(P2, Q2, n_items), ("Q = I", splits))
    P, Q, kw, _ = filter_case(dim)
    want = host_model_fast(P, Q, 10, **kw)
    few = np.zeros(len(Q), np.uint8)
    few[[3, 12, 77, 150, 299]] = 1
    want_few = host_model_fast(P, Q, 10, mask=few, **kw)
    for splits in (0, 1, 3):
        assert_same(run_op(P, Q, 10, splits=splits, **nan, **kw), want, ("filter", splits))
        assert_same(run_op(P, Q, 10, mask=few, splits=splits, **nan, **kw), want_few, ("filter and mask", splits))


# ---------------------------------------------------------------------------------------------- 3c. the merge's second trip
def test_the_merge_serves_more_jobs_than_its_grid():
    """65,536 + 40 jobs in two chunks: the merge kernel's grid is capped at 65,536 workgroups, so the last 40 jobs are second
    trips of the workgroups that served jobs 0 .. 39, and the two jobs of a workgroup differ in where their entries come from
    (tests/test_factor_host.py, merge_trip_case)."""
    case = merge_trip_case()
    want, _ = merge_trip_answer(case)
    n_rows = case["n_rows"]
    assert n_rows > GRID_CAP
    got = run_op(case["P"], case["Q"], case["top_k"], rows=case["rows"], p_index=case["p_index"], n_x_rows=case["n_x_rows"], mask=case["mask"],
                 splits=case["splits"])
    assert_same(got, tiled(want, n_rows), "merge, second trip")


# ---------------------------------------------------------------------------------------------- 4. ties
def test_thousands_of_tied_scores_go_to_the_lower_id():
    rng = np.random.default_rng(44)
    P = rng.integers(-1, 2, (40, 4)).astype(F32)
    Q = rng.integers(-1, 2, (3000, 4)).astype(F32)
    P[7] = 0                                                              # every score of this user is 0: ids 0 .. top_k-1
    want = host_model_fast(P, Q, 128)
    assert (want[0][7] == np.arange(128)).all() and (want[2] == 128).all()
    ties = sum(int((np.diff(want[1][r]) == 0).sum()) for r in range(40))
    assert ties > 3000
    for top_k, splits in ((128, 0), (128, 1), (128, 3), (10, 1), (10, 5)):
        assert_same(run_op(P, Q, top_k, splits=splits), cut(want, 40, top_k), (top_k, splits))


# ---------------------------------------------------------------------------------------------- 5. the threshold filter's worst case
@pytest.mark.parametrize("top_k", [10, 128])
def test_scores_that_rise_with_the_item_id_beat_the_threshold_every_time(top_k):
    """Every item beats everything before it, so no score is ever dropped in registers and the buffers compact all the way
    through the catalogue; the falling order (nothing after the first top_k survives) goes beside it."""
    n_items = 5000
    P = np.array([[1.0], [0.5], [3.0]], F32)
    rising = np.arange(n_items, dtype=F32)[:, None]
    for Q, name in ((rising, "rising"), (rising[::-1].copy(), "falling")):
        want = host_model_fast(P, Q, top_k)
        assert (want[0][0] == (np.arange(n_items - 1, n_items - 1 - top_k, -1) if name == "rising" else np.arange(top_k))).all()
        for splits in (1, 4):
            assert_same(run_op(P, Q, top_k, splits=splits), want, (name, top_k, splits))


def test_the_merge_fills_one_list_from_four_short_chunks():
    """One job, 97 items in four chunks of one tile (32, 32, 32 and 1 items), top_k 64: every partial list is shorter than top_k
    and the merge takes entries of all four; with a mask that admits 50 items the list ends in a
    -1 / -inf tail."""
    rng = np.random.default_rng(97)
    P = rng.standard_normal((1, 5)).astype(F32)
    Q = rng.standard_normal((97, 5)).astype(F32)
    Q[96] = 10 * P[0]                                                     # the last chunk's only item is the best of all
    mask = np.zeros(97, np.uint8)
    mask[rng.permutation(96)[:49]] = 1
    mask[96] = 1
    for m, n in ((None, 64), (mask, 50)):
        want = host_model_fast(P, Q, 64, mask=m)
        assert want[2][0] == n and want[0][0, 0] == 96 and set(want[0][0, :n] // 32) == {0, 1, 2, 3}
        assert (want[0][0, n:] == -1).all() and np.isneginf(want[1][0, n:]).all()
        assert_same(run_op(P, Q, 64, mask=m, splits=4), want, ("masked" if m is not None else "all", n))


# ---------------------------------------------------------------------------------------------- 6. filter, mask and rows
def test_filter_mask_rows_strides_and_specials():
    rng = np.random.default_rng(66)
    n_items, dim, n_x = 300, 7, 8
    P = rng.standard_normal((6, dim)).astype(F32)
    Q = rng.standard_normal((n_items, dim)).astype(F32)
    P[4, 2], P[5, 1] = np.inf, np.nan                    # vector 4 gives +-inf (and NaN against a 0), vector 5 only NaN
    Q[10, 2], Q[11, 2], Q[12, 0], Q[13, 3], Q[14, 2] = 0.0, -2.0, np.nan, np.inf, -np.inf
    p_index = np.array([0, 1, 2, 3, -1, 4, 5, 6])        # row 4 has no vector, row 7's index lies beyond P
    free = host_model_fast(P, Q, 40, rows=np.arange(n_x), p_index=p_index, n_x_rows=n_x)
    x_rows = [sorted(free[0][0, :30].tolist()),          # row 0: its 30 best items are all interacted
              list(range(n_items)),                      # row 1 stores every item
              [],                                        # row 2 is empty
              sorted(rng.choice(n_items, 50, replace=False).tolist()), [], sorted(rng.choice(n_items, 20, replace=False).tolist()), [3], []]
    X = sp.csr_matrix((np.ones(sum(map(len, x_rows)), F32), np.concatenate([np.array(r, np.int64) for r in x_rows]),
                       np.r_[0, np.cumsum([len(r) for r in x_rows])]), shape=(n_x, n_items))
    rows = [0, 1, 2, 3, 4, 5, 6, 7, -1, n_x, 0, 3]
    kw = dict(rows=rows, p_index=p_index, n_x_rows=n_x, X=X, filter_interacted=True)
    want = host_model_plain(P, Q, 10, **kw)
    assert_same(host_model_fast(P, Q, 10, **kw), want, "host models")
    assert want[2].tolist() == [10, 0, 10, 10, 0, 10, 0, 0, 0, 0, 10, 10]
    assert not set(want[0][0].tolist()) & set(x_rows[0]) and np.isposinf(want[1][5]).any()
    for splits in (0, 1, 3):
        for pad in (0, 5):
            assert_same(run_op(P, Q, 10, splits=splits, pad=pad, **kw), want, (splits, pad))
    few = np.zeros(n_items, np.uint8)
    few[[3, 12, 77, 150, 299]] = 1                       # five items, top_k 10; item 12 scores NaN for everyone, row 6 stores item 3
    want = host_model_plain(P, Q, 10, mask=few, **kw)
    assert want[2][0] <= 4 and want[2][2] == 4
    for splits in (0, 1, 3):
        assert_same(run_op(P, Q, 10, mask=few, splits=splits, pad=3, **kw), want, ("mask", splits))
    # the same without the filter: X is not read (no arrays are handed over)
    kw = dict(rows=rows, p_index=p_index, n_x_rows=n_x)
    assert_same(run_op(P, Q, 128, splits=2, **kw), host_model_fast(P, Q, 128, **kw), "no filter")
    # no p_index: row x has vector x, rows beyond P have none
    kw = dict(rows=[5, 6, 2, -1], n_x_rows=n_x, X=X, filter_interacted=True)
    want = host_model_plain(P, Q, 6, **kw)
    assert want[2].tolist() == [0, 0, 6, 0]
    assert_same(run_op(P, Q, 6, **kw), want, "no p_index")
    # an empty catalogue
    got = run_op(P, np.zeros((0, dim), F32), 4, splits=0)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all() and (got[2] == 0).all()


# ---------------------------------------------------------------------------------------------- 7. the API on the device
@pytest.mark.parametrize("strings", [False, True])
def test_recommend_factor_and_hybrid_batch_equal_the_host_path(strings):
    """All 150 users of the golden fixture model plus two cold ones, against the host path of tests/test_factor_host.py."""
    m, batch = fitted_model(strings, cpu=False)
    f, users = check_factor_and_hybrid(m, batch, strings, cases=(HYBRID_CASES[2], HYBRID_CASES[4], HYBRID_CASES[5]))
    assert len(users) == len(f["all_users"]) + 2 == 152
    eng = m.model.engine
    rows = np.arange(eng.n_users)
    base = eng.factor_topk_rows(rows, top_k=20)
    for splits in (1, 2, 9):
        assert_same(eng.factor_topk_rows(rows, top_k=20, item_splits=splits), base, splits)


# ---------------------------------------------------------------------------------------------- the op's own checks
def test_op_refuses_bad_ranges_and_mistyped_tensors():
    import torch
    from rtrec_amd import ops  # noqa: F401
    dev = "cuda:0"
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)

    def call(rows=None, pidx=None, n_x=4, p=None, qt=None, n_items=50, dim=6, mask=None, xp=None, xc=None, filt=False, top_k=5, splits=1,
             ids=None, scores=None, count=None, ws=None):
        p = f32(4, 6) if p is None else p
        qt = f32(6, 50) if qt is None else qt
        torch.ops.rtrec_amd.factor_topk(rows, pidx, n_x, p, qt, n_items, dim, mask, xp, xc, filt, top_k, splits,
                                        i32(2, top_k) if ids is None else ids, f32(2, top_k) if scores is None else scores,
                                        i32(2) if count is None else count, ws)

    call()
    for kw in (dict(dim=0), dict(dim=257), dict(top_k=0), dict(top_k=129), dict(splits=65), dict(splits=-1), dict(dim=7), dict(n_items=51),
               dict(p=f32(4, 6).double()), dict(qt=i32(6, 50)), dict(p=f32(4, 6).cpu()), dict(rows=i32(3)), dict(rows=i32(2).long()),
               dict(pidx=i32(5)), dict(mask=torch.zeros(49, dtype=torch.uint8, device=dev)), dict(mask=i32(50)), dict(filt=True),
               dict(filt=True, xp=i32(4), xc=i32(3)), dict(ids=i32(2, 4)), dict(scores=f32(2, 5).double()), dict(qt=f32(50, 6).t()),
               dict(splits=3, ws=None), dict(splits=3, ws=torch.zeros(10, dtype=torch.uint8, device=dev))):
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
