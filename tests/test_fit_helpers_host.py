"""The models of tests/fit_helper_models.py held to independent checks, on the CPU: the X^T y model against the C oracle on
every input of tests/test_gpu_fit_helpers.py, the preconditions those inputs were built for, the segment-layout decoder
against the numpy specification on every constructed shard, and the target cap of the one-pass X^T y scratch."""
import numpy as np
import pytest

from rtrec_amd import _native
from rtrec_amd.seg_layout import build_seg_layout
from tests import fit_helper_models as fm


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", fm.XTY_CASES)
def test_xty_model_equals_the_c_oracle(oracle, name):
    case = fm.xty_case(name)
    Xc, Xr = fm.both_orientations(case.X)
    assert np.array_equal(fm.f32_bits(Xr.data), fm.f32_bits(case.X.data))       # the case is already in canonical form
    assert len(np.unique(case.targets)) == len(case.targets)
    S = fm.xty_model(Xr, case.targets)
    D = Xr.toarray()
    for g, t in enumerate(case.targets.tolist()):
        ref = oracle.feature_scores(Xc, D[:, t], t)
        assert np.array_equal(fm.f32_bits(S[g]), fm.f32_bits(ref)), f"{name}: target {t}"
    lists = fm.xty_lists(S)
    assert all(np.all(np.diff(ids) > 0) and np.all(v != 0) for ids, v in lists)


def test_xty_inputs_meet_their_preconditions():
    all_asc, sub = fm.xty_case("all_ascending"), fm.xty_case("subset_shuffled")
    assert np.array_equal(all_asc.targets, np.arange(300))
    # a strict subset in an order that is not sorted; an emptied target, a target with one user
    assert len(sub.targets) == 200 and np.any(np.diff(sub.targets) < 0)
    nnz_col = np.diff(sub.X.tocsc().indptr)
    assert nnz_col[sub.notes["empty"]] == 0 and sub.notes["empty"] in sub.targets
    assert nnz_col[sub.notes["single"]] == 1 and sub.notes["single"] in sub.targets
    S = fm.xty_model(sub.X, sub.targets)
    assert not S[list(sub.targets).index(sub.notes["empty"])].any()
    # users with more than 64 / 128 of the call's targets: the kernel's tail loop runs for one and for two extra chunks
    per_user = fm.targets_per_user(sub.X, sub.targets)
    assert np.count_nonzero(per_user > 64) > 0 and np.count_nonzero(per_user > 128) > 0
    for name, n in (("nt1", 1), ("nt64", 64), ("nt65", 65), ("cap2048", 2048)):
        assert len(fm.xty_case(name).targets) == n
    cap = fm.xty_case("cap2048")
    assert cap.X.shape == (300, 2100) and 25000 < cap.X.nnz < 35000


def test_xty_signed_input_holds_a_sum_that_cancels_to_zero():
    case = fm.xty_case("signed")
    assert case.X.data.min() < 0 < case.X.data.max()
    t, f = case.notes["target"], case.notes["feature"]
    Xc = case.X.tocsc()
    assert np.array_equal(Xc[:, f].indices, Xc[:, t].indices) and Xc[:, f].nnz == 2     # the products exist ...
    S = fm.xty_model(case.X, case.targets)
    g = list(case.targets).index(t)
    assert S[g, f] == 0                                                                # ... and cancel
    ids, _ = fm.xty_lists(S)[g]
    assert f not in ids and len(ids) > 0


def test_xty_denormal_input_has_denormal_sums():
    case = fm.xty_case("denormal")
    S = fm.xty_model(case.X, case.targets)
    tiny = np.finfo(np.float32).tiny
    assert np.count_nonzero(S) > 1000
    assert np.all(np.abs(S) < tiny)                         # every sum is a denormal or zero
    same = fm.xty_model(fm.xty_case("subset_shuffled").X, case.targets)
    assert np.array_equal(S != 0, same != 0)                # nothing is lost to underflow


def test_xty_scratch_mirror_and_target_cap():
    lib = _native.load()
    for U, I, nnz, n_t in ((700, 300, 25000, 300), (700, 300, 25000, 1), (300, 2100, 30000, 2048), (1, 1, 1, 1), (64, 64, 63, 65)):
        assert fm.xty_ws_mirror(U, I, nnz, n_t)["total"] == int(lib.rtrec_slim_xty_workspace_bytes(U, I, nnz, n_t))
    assert fm.XTY_MAX_TARGETS == 2048
    assert int(lib.rtrec_slim_xty_workspace_bytes(300, 2100, 30000, 2048)) > 0
    assert int(lib.rtrec_slim_xty_workspace_bytes(300, 2100, 30000, 2049)) == 0


# ------------------------------------------------------------------------------------------------ C
def test_sqnorm_input_reaches_every_edge():
    cptr, cval = fm.sqnorm_case()
    lens = np.diff(cptr)
    assert tuple(lens[:len(fm.SQN_HEAD_LENGTHS)]) == fm.SQN_HEAD_LENGTHS and len(lens) == 8192 + 37
    assert lens[len(fm.SQN_HEAD_LENGTHS):].max() == 3 and lens[-37:].any()
    ref = fm.sqnorm_model(cptr, cval)
    tiny = np.finfo(np.float32).tiny
    assert np.isinf(ref[fm.SQN_INF_COLUMN]) and np.count_nonzero(np.isinf(ref)) == 1
    assert np.count_nonzero((ref > 0) & (ref < tiny)) > 10           # norms that are denormal
    assert np.count_nonzero((ref == 0) & (lens > 0)) > 10            # squares that underflow to zero
    ok = np.isfinite(ref)
    exact = np.array([np.sum(cval[cptr[c]:cptr[c + 1]].astype(np.float64) ** 2) for c in range(len(lens))])
    assert np.all(np.abs(ref[ok] - exact[ok]) <= 1e-4 * exact[ok] + 1e-44)


def test_gram_inputs_are_exact_in_float64():
    for n_users in (1, 33, 8193):
        X = fm.gram_exact_matrix(n_users)
        assert X.shape == (n_users, 400) and X.nnz > 0
        assert np.array_equal(X.data * 2, np.round(X.data * 2)) and X.data.min() >= 0.5 and X.data.max() <= 5.0
    top = fm.gram_top_items(400, 321, seed=4)
    assert len(np.unique(top)) == 321 and np.any(np.diff(top) < 0)
    pop = np.argsort(-np.diff(fm.gram_exact_matrix(8193).indptr), kind="stable")[:321]
    assert not np.array_equal(top, pop)
    rep = fm.gram_top_items(400, 65, seed=4, repeat=True)
    assert rep[-1] == rep[0] and len(np.unique(rep)) == 64
    XP = X[:, top[:40]].toarray().astype(np.float64)
    assert np.array_equal(fm.gram_fsum(XP), XP.T @ XP)
    assert 9000 * 2.0 ** -53 < fm.gram_gamma(9000) < 9001 * 2.0 ** -53


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("name", fm.SEG_CASES)
def test_layout_decoder_agrees_with_the_specification(name):
    case = fm.seg_case(name)
    ref = build_seg_layout(case.csc(), case.lo, case.hi, labels=case.labels)
    assert ref is not None and ref["sg_T"] == case.T
    found = fm.decode_seg_layout(ref, case)
    assert found["n_rec"] == ref["sg_ent"].shape[0] and found["n_list"] == ref["sg_trow"].shape[0]
    assert found["n_list"] == ref["sg_segments"]
    assert sum(d for _, d in found["segments"].values()) == ref["sg_dense_segments"]
    for k, want in case.expect.items():
        assert found["segments"][k] == want, (name, k)
    for k, want in case.bounds.items():
        assert found["bounds"][k] == want, (name, k)


def test_layout_inputs_meet_their_preconditions():
    lengths = fm.seg_case("lengths")
    assert lengths.n_items % 256 != 0 and lengths.cols.max() == lengths.n_items - 1
    got = {n for (_, t), (n, _) in lengths.expect.items() if t == 1}
    assert got == set(fm.SEG_LENGTHS)
    assert {n for (_, t), (n, _) in lengths.expect.items() if t == 3} == set(fm.SEG_LENGTHS) - {256}   # the last tile is 255 wide
    a, b = fm.seg_case("cols_32768"), fm.seg_case("cols_32769")
    assert len(np.unique(a.cols)) == 32768 and len(np.unique(b.cols)) == 32769 and a.n_items == b.n_items == 33000
    ref_b = build_seg_layout(b.csc(), b.lo, b.hi, labels=b.labels)
    assert ref_b["sg_dense_segments"] == 0 and not (ref_b["sg_ptr"] < 0).any()
    assert len(fm.seg_case("one_entry").vals) == 1 and len(np.unique(fm.seg_case("one_column").cols)) == 1
    gaps = fm.seg_case("shard_gaps")
    inside = (gaps.cols >= gaps.lo) & (gaps.cols < gaps.hi)
    assert len(np.unique(gaps.cols[inside])) < gaps.hi - gaps.lo
    assert set(gaps.rows[~inside]) - set(gaps.rows[inside]) == {40, 41}
    p2 = fm.seg_case("key_end_pow2")
    inside = (p2.cols >= p2.lo) & (p2.cols < p2.hi)
    R, n_cols = len(np.unique(p2.rows[inside])), len(np.unique(p2.cols[inside]))
    key_end = R * -(-n_cols // 256) * 256
    assert key_end == 2048 and key_end & (key_end - 1) == 0 and np.count_nonzero(~inside) > 0
    for name in ("labels_zero", "labels_reversed", "labels_top_on_lowest"):
        c = fm.seg_case(name)
        assert c.n_items == 4096 and len(np.unique(c.cols)) < 4096 and c.labels.max() <= 4095
    assert np.all(fm.seg_case("labels_top_on_lowest").labels[:10] == 4095)
    vals = fm.seg_case("values")
    bits = set(fm.f32_bits(vals.vals).tolist())
    assert {0x80000000, 0x7F7FFFFF, 0x3FC00000, 0x3FC00001, 0xBFC00001} <= bits
    assert any(0 < (b & 0x7FFFFFFF) < 0x00800000 for b in bits)
