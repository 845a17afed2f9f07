"""fit_sgd_kernel<1|2|4> (csrc/fit_sgd.hip) on the GPU, called directly through torch.ops.rtrec_amd.fit_sgd_epochs with hand-built
selections, against oracle.sgd on X[:, sel] -- weight bits and n_iter.  The cases, the builders of the kernel's inputs, the
Python statement of the kernel and the guards that show what each case is the witness of are in tests/test_sgd_host.py, where
the statement is proven equal to the oracle on every case without a GPU: a failure here points at the kernel, the driver or
the op wrapper.

Every case runs at blocks of 1, 3 and 16 epochs per call (the engine cuts max_iter into blocks of at most 16 and carries
sample_order, state, w, q, best_loss and no_improve across them): the answer must not depend on the block size."""
import numpy as np
import pytest

from tests.test_sgd_host import (BLOCKS, CASE_NAMES, POWER_T, bits32, epoch_blocks, fresh, get_case, kernel_inputs, native_schedule,
                                 oracle_answers)

pytestmark = pytest.mark.gpu

POISON = 1234.5
TAIL = 64


@pytest.fixture(scope="module", autouse=True)
def _ops():
    import rtrec_amd  # noqa: F401
    from rtrec_amd import ops  # noqa: F401  (registers and binds the ops)


def run_kernel(case, block, n_targets=None, stop_when_done=True):
    """The engine's driver around the solver, on hand-built inputs: per block of epochs the native schedule, the time-sorted
    copies of X in numpy, one fit_sgd_epochs call.  w and q start at zero, best_loss at +inf, no_improve and n_iter at 0.
    `n_targets`: the case's targets (and their selections) repeated in turn up to that many.  Returns (w[n, cap], q[n, cap], n_iter[n],
    per call: (unfinished as the kernel counted it, n_iter after the call, w after the call))."""
    import torch
    dev = "cuda:0"
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    U, I = case.X.shape
    n = len(case.targets) if n_targets is None else n_targets
    pick = np.arange(n) % len(case.targets)
    cap = case.cap
    d_cptr = to(case.X.indptr.astype(np.int32))
    d_t = to(case.targets[pick].astype(np.int32))
    d_sel = to(case.sel[pick].astype(np.int32))
    d_cnt = to(case.sel_count[pick].astype(np.int32))
    # state with a poisoned tail behind it: the kernel writes [n, cap] and nothing beyond
    w_buf = torch.full((n * cap + TAIL,), POISON, dtype=torch.float32, device=dev)
    q_buf = torch.full((n * cap + TAIL,), POISON, dtype=torch.float32, device=dev)
    d_w, d_q = w_buf[:n * cap].view(n, cap), q_buf[:n * cap].view(n, cap)
    d_w.zero_(); d_q.zero_()
    d_best = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
    d_noimp = torch.zeros(n, dtype=torch.int32, device=dev)
    d_niter = torch.zeros(n, dtype=torch.int32, device=dev)
    d_unf = torch.full((1,), 77, dtype=torch.int32, device=dev)
    order, state = fresh(U)
    nnz = int(case.X.nnz)
    calls = []
    for first, ne in epoch_blocks(case.max_iter, block):
        status, s = native_schedule(U, ne, case.seed, case.alpha, case.l1_ratio, case.eta0, POWER_T, order, state)
        assert status == 0
        order, state = s["sample_order"], s["state"]
        steps = ne * U
        tt, tv = kernel_inputs(case.X, s["time_of"][:ne])
        assert tt.shape == (ne, nnz) and int(tt.max()) < U
        torch.ops.rtrec_amd.fit_sgd_epochs(d_cptr, to(tt), to(tv), d_t, d_sel, d_cnt, U, I, nnz, cap, first, ne, case.max_iter,
                                           float(case.tol), to(s["eta"][:steps]), to(s["ws_before"][:steps]),
                                           to(s["ws_after"][:steps]), to(s["u_after"][:steps]), to(s["reset_cnt"][:steps + 1]),
                                           to(s["reset_mult"][:max(s["n_resets"], 1)]), d_w, d_q, d_best, d_noimp, d_niter, d_unf)
        torch.cuda.synchronize()
        calls.append((int(d_unf.item()), d_niter.cpu().numpy().copy(), d_w.cpu().numpy().copy()))
        if stop_when_done and calls[-1][0] == 0:
            break
    assert torch.all(w_buf[n * cap:] == POISON) and torch.all(q_buf[n * cap:] == POISON), "written beyond [n_targets, cap]"
    return d_w.cpu().numpy(), d_q.cpu().numpy(), d_niter.cpu().numpy(), calls


def check_against_oracle(case, w, q, nit, calls, w_ref, nit_ref, rows=None):
    rows = range(len(case.targets)) if rows is None else rows
    assert [int(nit[t]) for t in rows] == [int(nit_ref[t]) for t in rows], "n_iter differs from the oracle's"
    for t in rows:
        k = int(case.sel_count[t])
        if nit_ref[t] > 0:
            same = bits32(w[t, :k]) == bits32(w_ref[t, :k])
            assert np.all(same), (f"{case.name} target {t}: {int((~same).sum())} of {k} weights differ, first at position "
                                  f"{int(np.flatnonzero(~same)[0])}: {w[t, :k][~same][:4]} vs {w_ref[t, :k][~same][:4]}")
        assert np.all(bits32(w[t, k:]) == 0) and np.all(bits32(q[t, k:]) == 0), "positions from sel_count to cap must stay 0"
    # after every call: the kernel's count of unfinished targets, and a finished target's weights do not move any more
    for c, (unf, nit_c, w_c) in enumerate(calls):
        assert unf == int((nit_c == 0).sum()), f"call {c}: d_unfinished {unf}, targets with n_iter == 0: {int((nit_c == 0).sum())}"
        finished = np.flatnonzero(nit_c > 0)
        assert np.array_equal(nit_c[finished], nit[finished])
        assert np.array_equal(bits32(w_c[finished]), bits32(w[finished])), f"a target finished in call {c} moved afterwards"
    assert calls[-1][0] == 0


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_equals_the_oracle(name, block, oracle):
    """Every case family of tests/test_sgd_host.py (lane classes K = 1..256 with a full row, sel_count < cap, one lane at a
    time, gaps of 1 / 63 / 64 / 65 / 200 steps with resets on skipped steps, on sample steps and on a block's last step, the
    stop rule, divergence, the dloss clip, the target inside its own selection, empty columns): w bit for bit over the first
    sel_count positions, n_iter exactly (-1 for exactly the targets the oracle gives up on), zeros beyond sel_count, the
    kernel's unfinished count after every call, finished targets frozen."""
    case = get_case(name)
    w_ref, nit_ref = oracle_answers(name)
    w, q, nit, calls = run_kernel(case, block)
    check_against_oracle(case, w, q, nit, calls, w_ref, nit_ref)


def test_finished_targets_are_skipped_by_later_calls(oracle):
    """stops_mixed at one epoch per call, the calls going on to max_iter although some targets stopped at epoch 6: `n_iter !=
    0` must skip them (their weights, already multiplied by the final scale, stay as they are)."""
    case = get_case("stops_mixed")
    w_ref, nit_ref = oracle_answers("stops_mixed")
    for block in (1, 3):
        w, q, nit, calls = run_kernel(case, block, stop_when_done=False)
        assert len(calls) == len(list(epoch_blocks(case.max_iter, block)))
        check_against_oracle(case, w, q, nit, calls, w_ref, nit_ref)
        assert any(unf > 0 and (nit_c > 0).any() for unf, nit_c, _ in calls), "some targets finish while others run on"


def test_grid_stride_loop(oracle):
    """n_targets = 16384 + 70: the launch is capped at 16384 workgroups, the last 70 targets are a workgroup's second turn.
    The twelve columns of a 40 x 12 matrix repeated: every copy must give the bits of the first, the first twelve the oracle's."""
    case = get_case("grid")
    n0, n = len(case.targets), 16384 + 70
    w, q, nit, calls = run_kernel(case, 16, n_targets=n)
    assert w.shape == (n, case.cap) and len(calls) == 1 and calls[0][0] == 0
    w_ref, nit_ref = oracle_answers("grid")
    assert nit[:n0].tolist() == nit_ref.tolist()
    assert np.array_equal(bits32(w[:n0]), bits32(w_ref))
    first = np.arange(n) % n0
    assert np.array_equal(bits32(w), bits32(w[first])) and np.array_equal(nit, nit[first]), "a copy differs from the first"
    assert np.array_equal(bits32(q), bits32(q[first]))


def test_engine_names_the_first_diverged_column_and_is_block_invariant(oracle):
    """SlimEngine.fit_columns_sgd on the divergence case's matrix: the ValueError names the first column OF THE CALLER'S LIST
    whose weights left the finite range (the engine fits the longest columns first, here the two that converge); and on the
    stop case's matrix the answer does not depend on how many epochs one call of the solver gets."""
    from rtrec_amd.engine import SlimEngine
    case = get_case("diverge")
    X = case.X
    cfg = dict(alpha=case.alpha, l1_ratio=case.l1_ratio, eta0=case.eta0, max_iter=case.max_iter, nn_feature_selection=4)
    cols = np.array([12, 1, 13, 0])
    ref_iter = oracle.fit_columns_sgd(X, cols, **cfg)[3]
    assert ref_iter[0] > 0 and ref_iter[1] == -1 and ref_iter[2] > 0 and ref_iter[3] == -1
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(X, X.tocsr())
    with pytest.raises(ValueError, match=r"SGD fit of column 1\."):
        eng.fit_columns_sgd(cols, **cfg)
    tg, items, coef, count, n_iter = eng.fit_columns_sgd(cols[[0, 2]], **cfg)
    order = np.argsort(tg.cpu().numpy())
    assert np.asarray(n_iter)[order].tolist() == ref_iter[[0, 2]].tolist()

    case = get_case("stops_mixed")
    cfg = dict(alpha=case.alpha, l1_ratio=case.l1_ratio, eta0=case.eta0, max_iter=case.max_iter, tol=case.tol, nn_feature_selection=8)
    answers = []
    for block_bytes in (SlimEngine.SGD_EPOCH_BLOCK_BYTES, 8 * case.X.nnz, 3 * 8 * case.X.nnz):      # 16, 1 and 3 epochs per call
        eng = SlimEngine(device="cuda:0")
        eng.SGD_EPOCH_BLOCK_BYTES = block_bytes
        eng.set_interactions(case.X, case.X.tocsr())
        tg, items, coef, count, n_iter = eng.fit_columns_sgd(np.arange(10), **cfg)
        answers.append((tg.cpu().numpy(), items.cpu().numpy(), bits32(coef.cpu().numpy()), np.asarray(n_iter)))
    ptr, idx, val, nit = oracle.fit_columns_sgd(case.X, answers[0][0], **cfg)
    assert answers[0][3].tolist() == nit.tolist()
    for a in answers[1:]:
        for x, y in zip(a, answers[0]):
            assert np.array_equal(x, y), "the answer depends on the epochs per call"
