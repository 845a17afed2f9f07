"""optim="sgd" (csrc/fit_sgd.hip: rtrec_slim_sgd_schedule on the host, fit_sgd_kernel<F> on the device) without a GPU: a plain
Python statement of the host schedule and of the kernel's algorithm, the builders of the kernel's inputs and of the adversarial
cases, and the guards that show those cases decide something.  The kernel itself is in tests/test_gpu_sgd.py, which imports
the cases and the builders from here.

What is pinned here, on the CPU:
  * rtrec_slim_sgd_schedule equals schedule_model on every table, bit for bit, continues across calls, and refuses what it must;
  * kernel_model (the kernel's K-way merge over time-sorted columns, the skipping of samples that touch nothing, the schedule
    looked up at the next sample that matters, pending resets, the step's own reset, the epoch-end drain, the stop rule) equals
    oracle.sgd -- scikit-learn's sample-by-sample loop, tied to the real bits by tests/golden/sgd.json -- on EVERY case, at
    blocks of 1, 3 and 16 epochs: the builders, the schedule and the skipping argument are proven before any GPU run, so a
    failure on the GPU points at the kernel;
  * for each way the kernel could be subtly wrong (VARIANTS) at least one named case gives other bits or another n_iter.

Doubles are Python floats (IEEE binary64, one rounding per operation, like the kernel's __dadd_rn / __dmul_rn), floats are
numpy float32; pow is math.pow (libm, what the C routine calls) -- never np.power (tests/test_decay_host.py says why)."""
import ctypes as C
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import pytest
import scipy.sparse as sp

INF_T = 0x7FFFFFFF                 # kSgdInf
POWER_T = 0.25                     # SGDRegressor's default, what the engine passes
F32, F64 = np.float32, np.float64

# (alpha, l1_ratio, eta0)
PARAMS = {
    "default": (0.1, 0.1, 0.001),           # wscale never gets near 1e-6: no reset
    "frequent": (1.0, 0.0, 0.3),            # wscale falls below 1e-6 again and again
    "degenerate": (1.0, 0.0, 1.0),          # step 0: 1 - eta * alpha = 0 exactly -> c = 0, a reset with the factor 0.0f
    "all_zero": (20.0, 0.0, 1.0),           # arg <= 0 for the first 20^4 steps: EVERY step is a reset with the factor 0.0f
    "dense": (3.0, 0.0, 1.0),               # arg <= 0 for 81 steps, then c <= 0.73: every window of 64 steps holds a reset
    "no_scaling": (0.3, 1.0, 0.05),         # c == 1: wscale stays 1, only u grows
}


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- the host schedule
def rand_r(state: int):
    """sklearn/utils/_random.pxd our_rand_r: (new state, value)."""
    if state == 0:
        state = 1
    state ^= (state << 13) & 0xFFFFFFFF
    state ^= state >> 17
    state ^= (state << 5) & 0xFFFFFFFF
    return state, state % 2147483648


def schedule_model(n_samples, n_epochs, seed, alpha, l1_ratio, eta0, power_t, order, state):
    """rtrec_slim_sgd_schedule restated.  `order` (int list / array) and `state` = (wscale, u, t) are the values before the
    call; returns a dict of the tables plus "sample_order" and "state" after it."""
    order = [int(v) for v in order]
    wscale, u, t = (float(v) for v in state)
    n = n_samples
    time_of = np.empty((n_epochs, n), dtype=np.int32)
    eta, wsb, wsa, ua = ([0.0] * (n_epochs * n) for _ in range(4))
    rcnt = [0] * (n_epochs * n + 1)
    rmult = []
    g = 0
    for ep in range(n_epochs):
        s = int(seed) & 0xFFFFFFFF                      # the seed is passed by value: the same draws every epoch
        for i in range(n - 1):
            s, r = rand_r(s)
            j = i + r % (n - i)
            order[i], order[j] = order[j], order[i]
        time_of[ep, order] = np.arange(n, dtype=np.int32)
        for _ in range(n):
            e = eta0 / math.pow(t, power_t)
            eta[g], wsb[g], rcnt[g] = e, wscale, len(rmult)
            arg = 1.0 - ((1.0 - l1_ratio) * e * alpha)
            c = float(F32(arg if arg > 0.0 else 0.0))
            wscale *= c
            if wscale < 1e-6:
                rmult.append(F32(wscale))
                wscale = 1.0
            wsa[g] = wscale
            u += (l1_ratio * e * alpha)
            ua[g] = u
            t += 1.0
            g += 1
    rcnt[g] = len(rmult)
    return dict(time_of=time_of, eta=np.array(eta, F64), ws_before=np.array(wsb, F64), ws_after=np.array(wsa, F64),
                u_after=np.array(ua, F64), reset_cnt=np.array(rcnt, np.int32), reset_mult=np.array(rmult, F32),
                n_resets=len(rmult), sample_order=np.array(order, np.int32), state=np.array([wscale, u, t], F64))


def native_schedule(n_samples, n_epochs, seed, alpha, l1_ratio, eta0, power_t, order, state, reset_cap=None, null=None):
    """One rtrec_slim_sgd_schedule call on poisoned tables: (status, tables as schedule_model returns them).  `null` names
    one pointer argument to hand over as NULL."""
    from rtrec_amd import _native
    L = _native.load()
    steps = max(n_samples, 0) * max(n_epochs, 0)
    cap = steps + 1 if reset_cap is None else reset_cap
    a = dict(sample_order=np.array(order, dtype=np.int32), state=np.array(state, dtype=np.float64),
             time_of=np.full((max(n_epochs, 1), max(n_samples, 1)), -9, np.int32),
             eta=np.full(steps + 1, -9.0), ws_before=np.full(steps + 1, -9.0), ws_after=np.full(steps + 1, -9.0),
             u_after=np.full(steps + 1, -9.0), reset_cnt=np.full(steps + 2, -9, np.int32),
             reset_mult=np.full(max(cap, 0) + 2, -9.0, np.float32))
    n_res = C.c_int32(-9)
    hp = lambda k: None if k == null else C.c_void_p(a[k].ctypes.data)
    status = L.rtrec_slim_sgd_schedule(n_samples, n_epochs, int(seed) & 0xFFFFFFFF, float(alpha), float(l1_ratio), float(eta0),
                                       float(power_t), hp("sample_order"), hp("state"), hp("time_of"), hp("eta"), hp("ws_before"),
                                       hp("ws_after"), hp("u_after"), hp("reset_cnt"), hp("reset_mult"), int(cap),
                                       None if null == "n_resets" else C.byref(n_res))
    out = dict(a, n_resets=int(n_res.value), cap=cap, steps=steps)
    return int(status), out


def assert_schedule_equal(got, want, n_samples, n_epochs):
    """Every table of a native call against the model: integers exactly, doubles and floats by their bits; nothing is
    written beyond a table's end."""
    steps = n_samples * n_epochs
    assert got["n_resets"] == want["n_resets"]
    assert np.array_equal(got["time_of"][:n_epochs, :n_samples], want["time_of"])
    for k in ("eta", "ws_before", "ws_after", "u_after"):
        assert np.array_equal(bits64(got[k][:steps]), bits64(want[k])), k
        assert got[k][steps] == -9.0, f"{k} written beyond its end"
    assert np.array_equal(got["reset_cnt"][:steps + 1], want["reset_cnt"])
    assert got["reset_cnt"][steps + 1] == -9
    nr = want["n_resets"]
    assert np.array_equal(bits32(got["reset_mult"][:nr]), bits32(want["reset_mult"]))
    assert np.all(got["reset_mult"][nr:] == F32(-9.0)), "reset_mult written beyond n_resets"
    assert np.array_equal(got["sample_order"], want["sample_order"])
    assert np.array_equal(bits64(got["state"]), bits64(want["state"]))


def fresh(n):
    return np.arange(n, dtype=np.int32), np.array([1.0, 0.0, 1.0])


SCHEDULE_SEEDS = (0, 1, 2 ** 31 - 1, 1608637542)          # 0: our_rand_r turns the state 0 into 1; the last: sklearn_seed(43)


@pytest.mark.parametrize("pname", sorted(PARAMS))
@pytest.mark.parametrize("n_samples", [1, 2, 3, 64, 65, 400])
def test_schedule_equals_its_model(pname, n_samples):
    alpha, l1r, eta0 = PARAMS[pname]
    for n_epochs in (1, 5):
        for seed in (SCHEDULE_SEEDS if n_samples <= 65 else SCHEDULE_SEEDS[:3:2]):
            order, state = fresh(n_samples)
            want = schedule_model(n_samples, n_epochs, seed, alpha, l1r, eta0, POWER_T, order, state)
            status, got = native_schedule(n_samples, n_epochs, seed, alpha, l1r, eta0, POWER_T, order, state)
            assert status == 0
            assert_schedule_equal(got, want, n_samples, n_epochs)
            steps = n_samples * n_epochs
            assert sorted(want["sample_order"].tolist()) == list(range(n_samples))
            for ep in range(n_epochs):
                assert sorted(want["time_of"][ep].tolist()) == list(range(n_samples))
            if pname == "default":
                assert want["n_resets"] == 0 and np.all(want["ws_after"] > 0.5)
            elif pname == "no_scaling":
                assert want["n_resets"] == 0 and np.all(want["ws_after"] == 1.0) and np.all(np.diff(want["u_after"]) > 0)
            elif pname == "all_zero":
                assert want["n_resets"] == steps and np.all(want["reset_mult"] == 0.0) and np.all(want["ws_after"] == 1.0)
            elif pname == "degenerate":
                # 1 - eta0 / pow(1, .25) * alpha is exactly 0 at the first step only (t = 1); later steps reset every few steps
                assert want["reset_cnt"][1] == 1 and want["reset_mult"][0] == 0.0
                assert np.all(want["reset_mult"][1:] > 0)
            elif pname == "dense":
                r = want["reset_cnt"].astype(np.int64)
                assert steps < 64 or np.all(r[64:] - r[:-64] >= 1), "a reset in every window of 64 steps"
                assert want["reset_mult"][0] == 0.0 and (steps < 400 or np.any(want["reset_mult"] > 0))
            elif pname == "frequent":
                # measured, not assumed: with eta0 = 0.3 the scale needs about 60 steps for its first 1e-6 and ever more
                # later (eta falls with t^-1/4), so "one reset per 64 steps" holds at the start only -- the model's count
                # is what is asserted (exactly, above); here: resets do occur as soon as the run is long enough
                assert want["n_resets"] >= (1 if steps >= 128 else 0)
                if steps == 2000:
                    assert want["n_resets"] >= 8


def test_schedule_first_frequent_reset_is_within_the_first_window_sizes():
    """Where the 'frequent' set's resets fall (a 400-sample epoch): printed by the model, relied on by the gap cases."""
    alpha, l1r, eta0 = PARAMS["frequent"]
    m = schedule_model(400, 1, 7, alpha, l1r, eta0, POWER_T, *fresh(400))
    steps = np.flatnonzero(np.diff(m["reset_cnt"]))
    assert len(steps) >= 2 and steps[0] < 128, steps


@pytest.mark.parametrize("pname", ["default", "frequent", "degenerate"])
def test_schedule_continues_across_calls(pname):
    """One call for n epochs == calls of 1, 3 and n - 4 epochs chained through sample_order and state: reset_cnt restarts at 0
    in every call, reset_mult is the concatenation."""
    alpha, l1r, eta0 = PARAMS[pname]
    n_samples, n = 65, 9
    for seed in (0, 12345):
        order, state = fresh(n_samples)
        status, whole = native_schedule(n_samples, n, seed, alpha, l1r, eta0, POWER_T, order, state)
        assert status == 0
        parts, mults, first = [], [], 0
        for ne in (1, 3, n - 4):
            status, p = native_schedule(n_samples, ne, seed, alpha, l1r, eta0, POWER_T, order, state)
            assert status == 0
            assert_schedule_equal(p, schedule_model(n_samples, ne, seed, alpha, l1r, eta0, POWER_T, order, state), n_samples, ne)
            order, state = p["sample_order"], p["state"]
            s0, s1 = first * n_samples, (first + ne) * n_samples
            assert np.array_equal(p["time_of"][:ne], whole["time_of"][first:first + ne])
            for k in ("eta", "ws_before", "ws_after", "u_after"):
                assert np.array_equal(bits64(p[k][:s1 - s0]), bits64(whole[k][s0:s1])), k
            assert p["reset_cnt"][0] == 0
            assert np.array_equal(p["reset_cnt"][:s1 - s0 + 1], whole["reset_cnt"][s0:s1 + 1] - whole["reset_cnt"][s0])
            mults.append(p["reset_mult"][:p["n_resets"]])
            first += ne
        assert np.array_equal(order, whole["sample_order"]) and np.array_equal(bits64(state), bits64(whole["state"]))
        assert np.array_equal(bits32(np.concatenate(mults)), bits32(whole["reset_mult"][:whole["n_resets"]]))


def test_schedule_refusals():
    alpha, l1r, eta0 = PARAMS["frequent"]
    n_samples, n_epochs, seed = 400, 2, 3
    order, state = fresh(n_samples)
    count = schedule_model(n_samples, n_epochs, seed, alpha, l1r, eta0, POWER_T, order, state)["n_resets"]
    assert count >= 2
    status, got = native_schedule(n_samples, n_epochs, seed, alpha, l1r, eta0, POWER_T, order, state, reset_cap=count - 1)
    assert status == -3                                   # RTREC_ERR_WORKSPACE
    assert np.all(got["reset_mult"][count - 1:] == F32(-9.0)), "written beyond reset_cap"
    status, got = native_schedule(n_samples, n_epochs, seed, alpha, l1r, eta0, POWER_T, order, state, reset_cap=count)
    assert status == 0 and got["n_resets"] == count
    for ns, ne in ((0, 1), (-1, 1), (4, 0), (4, -2)):
        o, s = fresh(max(ns, 1))
        assert native_schedule(ns, ne, seed, alpha, l1r, eta0, POWER_T, o, s)[0] == -1          # RTREC_ERR_INVALID_ARG
    for name in ("sample_order", "state", "time_of", "eta", "ws_before", "ws_after", "u_after", "reset_cnt", "reset_mult", "n_resets"):
        o, s = fresh(4)
        status, got = native_schedule(4, 1, seed, alpha, l1r, eta0, POWER_T, o, s, null=name)
        assert status == -1, name
        assert np.all(got["eta"] == -9.0) and np.array_equal(got["sample_order"], o), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------- the kernel's inputs
def kernel_inputs(X_csc, epochs_time_of):
    """(ttime int32[ne, nnz], tval float32[ne, nnz]): per epoch the entries of every column of X ordered by their sample's
    time in that epoch (the engine: one device sort of (column, time) keys per epoch).  Asserts what the kernel relies on:
    inside a column the times ascend strictly, and the column's (time, value) multiset is the column's own."""
    ptr = np.asarray(X_csc.indptr, dtype=np.int64)
    rows = np.asarray(X_csc.indices, dtype=np.int64)
    vals = np.asarray(X_csc.data, dtype=np.float32)
    nnz = len(rows)
    col_of = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    ne = len(epochs_time_of)
    tt, tv = np.empty((ne, nnz), np.int32), np.empty((ne, nnz), np.float32)
    for e in range(ne):
        t = np.asarray(epochs_time_of[e], dtype=np.int64)[rows]
        perm = np.lexsort((t, col_of))
        tt[e], tv[e] = t[perm], vals[perm]
        assert np.array_equal(col_of[perm], col_of), "an entry left its column"
        inner = np.ones(nnz, bool)
        inner[ptr[1:-1][ptr[1:-1] < nnz]] = False
        if nnz:
            inner[0] = False
        assert np.all(np.diff(tt[e].astype(np.int64))[inner[1:]] > 0), "times must ascend strictly inside a column"
        back = np.lexsort((rows[perm], col_of))               # back to row order: the same entries, nothing lost or doubled
        assert np.array_equal(rows[perm][back], rows) and np.array_equal(bits32(tv[e][back]), bits32(vals))
    return tt, tv


# ---------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    X: sp.csc_matrix                  # U x I float32, sorted indices, no explicit zeros
    targets: np.ndarray               # [n_t] item column per target
    sel: np.ndarray                   # [n_t, cap] selected item columns, in selection order; beyond sel_count: padding
    sel_count: np.ndarray             # [n_t]
    cap: int
    alpha: float
    l1_ratio: float
    eta0: float
    tol: float
    max_iter: int
    seed: int
    note: dict = field(default_factory=dict)

    @property
    def U(self):
        return self.X.shape[0]


def signed_ratings(rng, shape, neg=0.3):
    """Float ratings in (0.5, 5], a share of them negative: weights of both signs reach both l1penalty branches."""
    v = rng.integers(1, 6, size=shape) * np.exp(-rng.random(shape) * 0.7)
    return (v * np.where(rng.random(shape) < neg, -1.0, 1.0)).astype(np.float32)


def random_dense(rng, U, I, density):
    return np.where(rng.random((U, I)) < density, signed_ratings(rng, (U, I)), 0).astype(np.float32)


def to_csc(D):
    X = sp.csc_matrix(np.asarray(D, dtype=np.float32))
    X.eliminate_zeros()
    X.sort_indices()
    return X


def epoch0_rows_by_time(U, seed):
    """row_at[t]: the sample visited at step t of epoch 0 (the shuffle does not depend on the parameters)."""
    m = schedule_model(U, 1, seed, 0.1, 0.1, 0.001, POWER_T, *fresh(U))
    return m["sample_order"].copy()


def make_case(name, D, targets, sel, sel_count, cap, pname, tol=1e-4, max_iter=6, seed=1608637542, **note):
    alpha, l1r, eta0 = PARAMS[pname] if isinstance(pname, str) else pname
    sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(len(targets), cap)
    return Case(name, to_csc(D), np.asarray(targets, np.int32), sel, np.asarray(sel_count, np.int32), int(cap), alpha, l1r, eta0,
                float(tol), int(max_iter), int(seed), note)


LANE_KS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
LANE_L2_KS = (65, 129, 193, 256)


def lane_case(K, l2_only=False):
    """130 x 260, cap = sel_count = K, a selection in random (not ascending) order, two targets (the second with the selection
    rotated).  Row r0 -- the LAST sample of epoch 0 -- stores every selected feature, y[r0] = 0:
      * positions pa < pb hold two identical columns with +3.25 / -3.25 in r0: their float products cancel EXACTLY;
      * every other feature's value in r0 is about 2^-60, so its product is below half an ulp of the cancelling pair's:
        what is summed before the second of the pair is absorbed and lost, what comes after survives -- which positions
        survive depends on the order of the summation, and whether the survivors round depends on the accumulator's type;
      * two probe features are stored in r0 alone: their weight is 0 until r0's update = -eta * p lands in them, so p's
        low bits become weight bits.  The probes keep them only without an L1 penalty (truncation clips 1e-24 to 0), hence
        the l2_only twin of the cases with more than one feature per lane."""
    rng = np.random.default_rng(1000 + K)
    U, I, seed = 130, 260, 1608637542
    D = random_dense(rng, U, I, 0.15)
    perm = rng.permutation(I)
    sel0, tg = perm[:K], perm[256:258]
    r0 = int(epoch0_rows_by_time(U, seed)[-1])
    D[r0, sel0] = (np.ldexp(1.0 + rng.random(K), -60) * np.where(rng.random(K) < 0.5, -1, 1)).astype(np.float32)
    D[r0, tg] = 0
    note = dict(r0=r0)
    if K >= 8:
        pa, pb = 5, K // 2 + 3
        yrows = np.flatnonzero(D[:, tg[0]])[:3]
        D[yrows, sel0[pa]] = 2.0                          # the pair's weight is non-zero when r0 comes
        D[:, sel0[pb]] = D[:, sel0[pa]]
        D[r0, sel0[pa]], D[r0, sel0[pb]] = 3.25, -3.25
        for probe in (K - 1, K // 3):
            D[:, sel0[probe]] = 0
            D[r0, sel0[probe]] = 1.0
        note.update(pa=pa, pb=pb, probes=(K - 1, K // 3))
    sel = np.stack([sel0, np.roll(sel0, K // 2)])
    pname = (0.05, 0.0, 0.01) if l2_only else (0.1, 0.1, 0.01)
    return make_case(f"lane_{K}" + ("_l2" if l2_only else ""), D, tg, sel, [K, K], K, pname, max_iter=4, seed=seed, **note)


def count_case(cap):
    """sel_count < cap, different counts in one call (cap 256: 0, 1, 64, 200; cap 128: 65, 127).  The padding beyond a count
    names a dense column that is NOT selected: a kernel that read it would give other bits."""
    rng = np.random.default_rng(2000 + cap)
    U, I = 130, 262
    D = random_dense(rng, U, I, 0.12)
    counts = [0, 1, 64, 200] if cap == 256 else [65, 127]
    perm = rng.permutation(I - 1)                           # column I - 1: the padding
    D[:, I - 1] = signed_ratings(rng, U)
    tg = perm[256:256 + len(counts)] if cap == 256 else perm[200:200 + len(counts)]
    sel = np.full((len(counts), cap), I - 1, np.int32)
    for t, c in enumerate(counts):
        sel[t, :c] = np.roll(perm[:cap], 7 * t)[:c]
    return make_case(f"count_{cap}", D, tg, sel, counts, cap, "default", max_iter=4)


LANE_ORDER = [63, 0, 15, 16, 31, 32, 47, 48]


def one_lane_case(K):
    """Every feature column stores exactly ONE entry, in a row of its own; the rows are laid along epoch 0's shuffle so that
    the feature whose turn it is walks the lanes 63, 0, 15, 16, 31, 32, 47, 48 and then the rest in a scrambled order (K = 256:
    four rounds, the register index f = pos / 64 changing from step to step as well).  Every third step is a row that stores
    only y; y is also stored in half of the feature rows (a weight only moves where y or p is non-zero)."""
    rng = np.random.default_rng(3000 + K)
    U = {64: 120, 256: 400}[K]
    seed = 99
    row_at = epoch0_rows_by_time(U, seed)
    rest = [l for l in rng.permutation(64).tolist() if l not in LANE_ORDER]
    lanes = LANE_ORDER + rest
    F = K // 64
    positions = [lane + 64 * ((idx + k) % F) for k in range(F) for idx, lane in enumerate(lanes)]
    assert sorted(positions) == list(range(K))
    I = K + 1
    D = np.zeros((U, I), np.float32)
    feat_cols = rng.permutation(K)                         # item column of position p
    tgt = K
    slot, walk = 0, []
    for n, p in enumerate(positions):
        if n % 2 == 0 and slot < U - (K - n):              # a y-only row in between, while rows are left
            D[row_at[slot], tgt] = signed_ratings(rng, 1)[0]
            slot += 1
        r = row_at[slot]
        slot += 1
        D[r, feat_cols[p]] = signed_ratings(rng, 1)[0]
        if n % 2 == 0 or n < 8:
            D[r, tgt] = signed_ratings(rng, 1)[0]
        walk.append((int(r), p))
    return make_case(f"one_lane_{K}", D, [tgt], feat_cols[None, :], [K], K, (0.1, 0.1, 0.05), max_iter=5, seed=seed, walk=walk,
                     positions=positions)


GAP_TIMES = (0, 1, 64, 128, 193, 393)                    # steps 1, 63, 64, 65 and 200 apart


def gap_case(pname):
    """U = 400, four targets with feature columns of their own, laid out in TIME (epoch 0's shuffle), not in row index:
      A  samples at steps 0, 1, 64, 128, 193, 393 of epoch 0 (1, 63, 64, 65, 200 apart; the first at step 0; the one at step 1
         stores only y; two store only features);
      B  one sample, at step U - 1 of epoch 0 (in later epochs wherever the shuffle puts it: one sample per epoch, so all the
         resets of an epoch lie between two samples);
      C  an empty target column whose three features are empty too: no sample at all, the drain alone walks the resets;
      D  samples ON the steps at which the schedule resets the weight scale in epoch 0 (and the step after the first)."""
    alpha, l1r, eta0 = PARAMS[pname]
    rng = np.random.default_rng(4000)
    U, seed, max_iter = 400, 7, 12
    row_at = epoch0_rows_by_time(U, seed)
    m = schedule_model(U, 1, seed, alpha, l1r, eta0, POWER_T, *fresh(U))
    resets = [int(s) for s in np.flatnonzero(np.diff(m["reset_cnt"])) if s not in GAP_TIMES and s + 1 not in GAP_TIMES and 1 < s < U - 2]
    d_times = ([resets[0], resets[0] + 1] + resets[1:3]) if resets else [50, 51, 300]
    d_times = sorted(set(d_times))
    I = 17
    D = np.zeros((U, I), np.float32)
    fa, fb, fc, fd = [4, 5, 6, 7, 8], [9, 10], [11, 12, 13], [14, 15, 16]
    for n, t in enumerate(GAP_TIMES):
        r = row_at[t]
        if n in (0, 1, 3, 5):
            D[r, 0] = signed_ratings(rng, 1)[0]
        if n != 1:
            pick = rng.permutation(5)[:rng.integers(1, 6)]
            D[r, np.array(fa)[pick]] = signed_ratings(rng, len(pick))
    D[row_at[0], fa] = signed_ratings(rng, 5)            # every feature of A moves at step 0
    D[row_at[U - 1], [1] + fb] = signed_ratings(rng, 3)
    for t in d_times:
        D[row_at[t], [3] + fd] = signed_ratings(rng, 4)
    sel = np.full((4, 5), 16, np.int32)
    cnt = [5, 2, 3, 3]
    for t, f in enumerate((fa, fb, fc, fd)):
        sel[t, :len(f)] = f
    sel[0, :5] = [7, 4, 8, 6, 5]
    return make_case(f"gap_{pname}", D, [0, 1, 2, 3], sel, cnt, 5, pname, max_iter=max_iter, seed=seed, d_times=d_times)


# found by reset_epoch_end_search() below: with the "frequent" set and this many samples a reset falls on the LAST step of
# epoch 5 (counting from 0), i.e. the last step of a block of 1 and of a block of 3 epochs and -- with max_iter = 6 -- of the run
RESET_END_U, RESET_END_EPOCH = 337, 5


def reset_epoch_end_search(max_epochs=6):
    alpha, l1r, eta0 = PARAMS["frequent"]
    for U in range(400, 60, -1):
        m = schedule_model(U, max_epochs, 1, alpha, l1r, eta0, POWER_T, *fresh(U))
        steps = np.flatnonzero(np.diff(m["reset_cnt"]))
        hit = [int(s) // U for s in steps if s % U == U - 1 and (s // U + 1) % 3 == 0]
        if hit:
            return U, hit[0]
    return None


def reset_end_case(extra_epochs):
    """A reset on the last step of an epoch that is the last of its block at every block size (1, 3, 16): with extra_epochs
    = 0 it is also the run's last step (the final reset_wscale follows at once), with 1 the next block starts from it."""
    U, ep = RESET_END_U, RESET_END_EPOCH
    rng = np.random.default_rng(5000)
    I, K = 24, 20
    D = random_dense(rng, U, I, 0.05)
    sel = np.stack([rng.permutation(np.delete(np.arange(I), t))[:K] for t in (0, 1, 2)])
    return make_case(f"reset_end_{extra_epochs}", D, [0, 1, 2], sel, [K] * 3, K, "frequent", tol=-np.inf,
                     max_iter=ep + 1 + extra_epochs, seed=1)


def stops_case(kind):
    """120 x 30, K = 8, ten targets.  mixed: tol = 1e-3 -- some targets stop by n_iter_no_change after epoch 6 or later, others run
    to max_iter = 20 (asserted on the oracle's answers); max1: max_iter = 1; tolnone: tol = -inf, nobody stops early."""
    rng = np.random.default_rng(6000)
    U, I, K = 120, 30, 8
    D = random_dense(rng, U, I, 0.2)
    D[:, :5] *= np.float32(0.02)                            # faint targets: their loss hardly moves -> they stop early
    tg = np.arange(10)
    sel = np.stack([rng.permutation(np.delete(np.arange(I), t))[:K] for t in tg])
    tol, max_iter = {"mixed": (1e-3, 20), "max1": (1e-4, 1), "tolnone": (-np.inf, 20)}[kind]
    return make_case(f"stops_{kind}", D, tg, sel, [K] * 10, K, (0.01, 0.1, 0.02), tol=tol, max_iter=max_iter)


def stop_rounding_case(seed):
    """The stop rule at its razor's edge, and the witness that a sample whose row holds only y must NOT be skipped.  alpha =
    50 with l1_ratio = 1: the truncated gradient clips every weight back to 0 within its own step, so p = 0 at every sample
    and the epoch's loss is sum(0.5 y^2) -- the same real number every epoch, but summed in the shuffle's order, so its last
    bits differ from epoch to epoch; with tol = 0 those bits alone decide `sumloss > best_loss`.  Leaving out the y-only
    rows shifts every epoch's loss by the same constant (invisible to any tolerance) but changes the rounding."""
    rng = np.random.default_rng(seed)
    U, I, K = 61, 8, 3
    D = np.zeros((U, I), np.float32)
    D[:, 0] = signed_ratings(rng, U)
    D[rng.permutation(U)[:20], 0] = 0
    for c in (1, 2, 3):
        rows = rng.permutation(U)[:12]
        D[rows, c] = signed_ratings(rng, 12)
    return make_case(f"stop_rounding_{seed}", D, [0], [[1, 2, 3]], [3], 3, (50.0, 1.0, 0.001), tol=0.0, max_iter=40, seed=seed)


def diverge_case():
    """eta0 = 0.3 on ratings of 1e17: the clip of dloss to 1e12 bounds an update, so a weight gets to about 1e29 and no further --
    but then the float products w * x overflow to +-inf, a row with products of both signs sums to NaN, and NaN goes through
    the clip into every weight of the row (the oracle returns -1 for targets 0..2; found by trying scales on the CPU: ratings
    of 40 or 1e6 only oscillate below the clip).  X^T y of these columns stays finite in float32, so the engine's own
    feature selection works on the same data.  The fourth target (column 12) is their neighbour in the same call: ordinary
    ratings in rows of their own, it converges -- and its columns are the longer ones, so the engine fits them FIRST."""
    rng = np.random.default_rng(7000)
    U, I, K = 80, 16, 4
    D = np.zeros((U, I), np.float32)
    D[:40, :8] = random_dense(rng, 40, 8, 0.5) * np.float32(1e17)
    D[40:, 8:] = random_dense(rng, 40, 8, 0.6)           # another block of rows: no sample in common with the columns above
    sel = np.array([[4, 5, 6, 7], [5, 6, 7, 4], [0, 4, 5, 6], [8, 9, 10, 11]])
    return make_case("diverge", D, [0, 1, 2, 12], sel, [K] * 4, K, (1e-4, 0.1, 0.3), max_iter=30)


def clip_case():
    """|p - y| > 1e12 with finite weights to the end: two ratings of 3e20 in the target column.  dloss is clipped to -1e12 at
    those samples, the update eta * 1e12 lands in the row's features (about 1e9: far inside float32), and the following
    samples pull the weights back.  Without the clip the update would be eta * 3e20 (variant "no_clip")."""
    rng = np.random.default_rng(8000)
    U, I, K = 60, 10, 5
    D = random_dense(rng, U, I, 0.3)
    rows = np.flatnonzero((D[:, 1:6] != 0).sum(axis=1) >= 2)[:2]
    D[rows, 0] = np.float32(3e20)
    return make_case("clip", D, [0], [[1, 2, 3, 4, 5]], [K], K, "default", max_iter=3, clip_rows=rows.tolist())


def self_case():
    """The target is one of its own selected features, at positions 0, 63, 64 and 255 (the oracle gets an empty column there:
    FeatureSelectionWrapper zeroes the target's column before the fit); target 4 is an empty column; target 5's three
    features are empty columns."""
    rng = np.random.default_rng(9000)
    U, I, K = 130, 270, 256
    D = random_dense(rng, U, I, 0.1)
    D[:, 260:] = 0
    tg = [10, 20, 30, 40, 265, 50]
    perm = rng.permutation(260)
    sel = np.full((6, K), 259, np.int32)
    cnt = [K, K, K, K, K, 3]
    for t, pos in enumerate((0, 63, 64, 255)):
        s = [c for c in np.roll(perm, 11 * t).tolist() if c != tg[t]][:K - 1]
        s.insert(pos, tg[t])
        sel[t] = s
    sel[4] = [c for c in perm.tolist()][:K]
    sel[5, :3] = [261, 262, 263]
    return make_case("self", D, tg, sel, cnt, K, (0.1, 0.1, 0.01), max_iter=4, self_pos=(0, 63, 64, 255))


def grid_case():
    """40 x 12, K = 3, max_iter = 3, every column a target: the GPU test repeats these twelve 16384 + 70 times over."""
    rng = np.random.default_rng(10000)
    U, I, K = 40, 12, 3
    D = random_dense(rng, U, I, 0.3)
    sel = np.stack([rng.permutation(np.delete(np.arange(I), t))[:K] for t in range(I)])
    return make_case("grid", D, np.arange(I), sel, [K] * I, K, (0.1, 0.1, 0.05), max_iter=3)


STOP_ROUNDING_SEEDS = (0,)

CASES = {}
for _K in LANE_KS:
    CASES[f"lane_{_K}"] = functools.partial(lane_case, _K)
for _K in LANE_L2_KS:
    CASES[f"lane_{_K}_l2"] = functools.partial(lane_case, _K, True)
for _cap in (256, 128):
    CASES[f"count_{_cap}"] = functools.partial(count_case, _cap)
for _K in (64, 256):
    CASES[f"one_lane_{_K}"] = functools.partial(one_lane_case, _K)
for _p in ("default", "frequent", "degenerate", "all_zero", "dense"):
    CASES[f"gap_{_p}"] = functools.partial(gap_case, _p)
for _e in (0, 1):
    CASES[f"reset_end_{_e}"] = functools.partial(reset_end_case, _e)
for _k in ("mixed", "max1", "tolnone"):
    CASES[f"stops_{_k}"] = functools.partial(stops_case, _k)
for _s in STOP_ROUNDING_SEEDS:
    CASES[f"stop_rounding_{_s}"] = functools.partial(stop_rounding_case, _s)
CASES.update(diverge=diverge_case, clip=clip_case, self=self_case, grid=grid_case)
CASE_NAMES = list(CASES)
BLOCKS = (1, 3, 16)


@functools.lru_cache(maxsize=None)
def get_case(name) -> Case:
    c = CASES[name]()
    assert c.name == name
    assert c.U <= 400 and c.max_iter <= 40 and 1 <= c.cap <= 256
    assert c.sel.shape == (len(c.targets), c.cap) and np.all((c.sel >= 0) & (c.sel < c.X.shape[1]))
    assert np.all((c.sel_count >= 0) & (c.sel_count <= c.cap))
    return c


def selected_csr(case: Case, t: int):
    """X[:, sel] of target t as the oracle takes it: CSR over the positions 0..sel_count-1, a row's entries stored in
    selection-position order, the target's own column (if selected) empty; and the dense y."""
    X, j, Kc = case.X, int(case.targets[t]), int(case.sel_count[t])
    rows, pos, vals = [], [], []
    for p in range(Kc):
        col = int(case.sel[t, p])
        if col == j:
            continue
        lo, hi = X.indptr[col], X.indptr[col + 1]
        rows.append(X.indices[lo:hi]); vals.append(X.data[lo:hi]); pos.append(np.full(hi - lo, p, np.int32))
    if rows:
        rows, pos, vals = np.concatenate(rows), np.concatenate(pos), np.concatenate(vals)
        o = np.lexsort((pos, rows))
        rows, pos, vals = rows[o], pos[o], vals[o]
    else:
        rows, pos, vals = np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    ptr = np.zeros(case.U + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=case.U), out=ptr[1:])
    R = sp.csr_matrix((vals.astype(np.float32), pos.astype(np.int32), ptr), shape=(case.U, max(Kc, 0)))
    y = np.zeros(case.U, np.float32)
    lo, hi = X.indptr[j], X.indptr[j + 1]
    y[X.indices[lo:hi]] = X.data[lo:hi]
    return R, y


@functools.lru_cache(maxsize=None)
def oracle_answers(name):
    """(w float32[n_t, cap] zero beyond sel_count, n_iter int[n_t]) of oracle.sgd, target by target."""
    from oracle import slim_oracle as so
    case = get_case(name)
    w = np.zeros((len(case.targets), case.cap), np.float32)
    nit = np.zeros(len(case.targets), np.int64)
    for t in range(len(case.targets)):
        R, y = selected_csr(case, t)
        wt, nit[t] = so.sgd(R, y, case.alpha, case.l1_ratio, case.eta0, POWER_T, case.tol, case.max_iter, case.seed)
        w[t, :len(wt)] = wt
    w.setflags(write=False); nit.setflags(write=False)
    return w, nit


# ---------------------------------------------------------------------------------------------- the kernel's algorithm
VARIANTS = ("lanes_outer", "f32_sum", "drop_pending", "own_reset_first", "skip_y_only", "eta_prev", "dead_192", "no_clip")


def epoch_blocks(max_iter, block):
    first = 0
    while first < max_iter:
        ne = min(block, max_iter - first)
        yield first, ne
        first += ne


@functools.lru_cache(maxsize=None)
def prepared(name, block):
    """Per block of epochs: (first_epoch, n_epochs, schedule tables, ttime, tval), the schedule chained through sample_order
    and state as the engine chains it (schedule_model: independent of the native routine)."""
    case = get_case(name)
    order, state = fresh(case.U)
    out = []
    for first, ne in epoch_blocks(case.max_iter, block):
        m = schedule_model(case.U, ne, case.seed, case.alpha, case.l1_ratio, case.eta0, POWER_T, order, state)
        order, state = m["sample_order"], m["state"]
        tt, tv = kernel_inputs(case.X, m["time_of"])
        out.append((first, ne, m, tt, tv))
    return out


def _mul_all(w, rm):
    with np.errstate(all="ignore"):
        return (F32(rm) * w).astype(F32)


def _run_block(case, t, first, ne, m, tt_all, tv_all, st, variant):
    """fit_sgd_kernel's body for one target and one block of epochs; st = dict(w, q, best, no_imp, n_iter) is updated."""
    U, cap = case.U, case.cap
    j, Kc = int(case.targets[t]), int(case.sel_count[t])
    F = 1 if cap <= 64 else 2 if cap <= 128 else 4
    cptr = case.X.indptr
    cols = case.sel[t, :Kc].astype(np.int64)
    live = cols != j
    if variant == "dead_192":
        live &= np.arange(Kc) < 192
    cb = np.where(live, cptr[cols], 0).astype(np.int64)
    ce = np.where(live, cptr[cols + 1], 0).astype(np.int64)
    yb, ye = int(cptr[j]), int(cptr[j + 1])
    w, q = st["w"], st["q"]
    eta_t, wsb_t, wsa_t, ua_t = (m[k].tolist() for k in ("eta", "ws_before", "ws_after", "u_after"))
    rcnt, rmult = m["reset_cnt"].tolist(), m["reset_mult"]
    nnz = tt_all.shape[1]
    done = 0
    for ep in range(ne):
        tt, tv = tt_all[ep], tv_all[ep]
        g0 = ep * U
        cur = cb.copy()
        yc = yb
        sumloss = 0.0
        ri = rcnt[g0]
        prev_g = None
        while True:
            open_ = cur < ce
            my_t = np.where(open_, tt[np.minimum(cur, nnz - 1)], INF_T) if Kc else np.zeros(0, np.int64)
            y_t = int(tt[yc]) if yc < ye else INF_T
            tmin = min(int(my_t.min()) if Kc else INF_T, y_t)
            if tmin == INF_T:
                break
            g = g0 + tmin
            rc = rcnt[g]
            while ri < rc:                                   # reset_wscale() of the skipped steps
                if variant != "drop_pending":
                    w = _mul_all(w, rmult[ri])
                ri += 1
            own = rcnt[g + 1] > rc
            if own and variant == "own_reset_first":
                w = _mul_all(w, rmult[ri])
                ri += 1
            part = np.flatnonzero(my_t == tmin)              # ascending position: f outer, lanes inner
            has_y = y_t == tmin
            if variant == "skip_y_only" and part.size == 0:
                if own and variant != "own_reset_first":
                    w = _mul_all(w, rmult[ri])
                    ri += 1
                yc += 1
                continue
            x = tv[cur[part]]
            with np.errstate(all="ignore"):
                prod = (w[part] * x).astype(F32)
                order = np.arange(part.size)
                if variant == "lanes_outer":
                    order = np.lexsort((part // 64, part % 64))
                if variant == "f32_sum":
                    acc = F32(0.0)
                    for v in prod[order]:
                        acc = F32(acc + v)
                    innerprod = float(acc)
                else:
                    innerprod = 0.0
                    for v in prod[order].astype(F64).tolist():
                        innerprod += v
                innerprod *= wsb_t[g]
                p = float(F32(innerprod))
                yv = float(tv[yc]) if has_y else 0.0
                eta = eta_t[prev_g] if (variant == "eta_prev" and prev_g is not None) else eta_t[g]
                d = p - yv
                sumloss += 0.5 * d * d
                dloss = d
                if variant != "no_clip":
                    if dloss < -1e12:
                        dloss = -1e12
                    elif dloss > 1e12:
                        dloss = 1e12
                update = -eta * dloss
                if own and variant != "own_reset_first":     # this step's w.scale() reset
                    w = _mul_all(w, rmult[ri])
                    ri += 1
                wsd, u = wsa_t[g], ua_t[g]
                if part.size:
                    if update != 0.0:
                        c, wsf = F32(update), F32(wsd)
                        step = float(F32(c / wsf))
                        w[part] = (w[part].astype(F64) + x.astype(F64) * step).astype(F32)
                    z = w[part].astype(F64)                   # l1penalty32
                    q64 = q[part].astype(F64)
                    sz = wsd * z
                    vp = z - (u + q64) / wsd
                    vn = z + (u - q64) / wsd
                    wn = np.where(sz > 0.0, np.where(vp > 0.0, vp, 0.0).astype(F32),
                                  np.where(sz < 0.0, np.where(vn < 0.0, vn, 0.0).astype(F32), w[part])).astype(F32)
                    w[part] = wn
                    q[part] = (q64 + wsd * (wn.astype(F64) - z)).astype(F32)
                    cur[part] += 1
            if has_y:
                yc += 1
            prev_g = g
        rc = rcnt[g0 + U]                                    # the epoch's remaining (skipped) steps
        while ri < rc:
            w = _mul_all(w, rmult[ri])
            ri += 1
        epoch = first + ep
        if not np.all(np.isfinite(w[:Kc])):
            done = -1
            break
        if sumloss > st["best"] - case.tol * float(U):
            st["no_imp"] += 1
        else:
            st["no_imp"] = 0
        if sumloss < st["best"]:
            st["best"] = sumloss
        if st["no_imp"] >= 5 or epoch == case.max_iter - 1:
            w = _mul_all(w, F32(wsa_t[g0 + U - 1]))          # w.reset_wscale()
            done = epoch + 1
            break
    st["w"], st["q"], st["n_iter"] = w, q, done


def kernel_model(name, block=16, variant=None, targets=None):
    """The kernel's algorithm over the whole run, `block` epochs per call with w, q, best_loss, no_improve and n_iter carried
    across the calls: (w[n_t, cap], n_iter[n_t], unfinished count after every call)."""
    assert variant is None or variant in VARIANTS
    case = get_case(name)
    n_t = len(case.targets)
    todo = range(n_t) if targets is None else targets
    sts = {t: dict(w=np.zeros(case.cap, F32), q=np.zeros(case.cap, F32), best=math.inf, no_imp=0, n_iter=0) for t in todo}
    unfinished = []
    for first, ne, m, tt, tv in prepared(name, block):
        for t in todo:
            if sts[t]["n_iter"] == 0:
                _run_block(case, t, first, ne, m, tt, tv, sts[t], variant)
        unfinished.append(sum(1 for t in todo if sts[t]["n_iter"] == 0))
        if unfinished[-1] == 0:
            break
    w = np.zeros((n_t, case.cap), F32)
    nit = np.zeros(n_t, np.int64)
    for t in todo:
        w[t], nit[t] = sts[t]["w"], sts[t]["n_iter"]
    return w, nit, unfinished


def same_answer(case, w, nit, w_ref, nit_ref, targets=None):
    """n_iter exactly; w bit for bit over the first sel_count positions of every target that did not diverge."""
    for t in (range(len(case.targets)) if targets is None else targets):
        if nit[t] != nit_ref[t]:
            return False
        k = int(case.sel_count[t])
        if nit_ref[t] > 0 and not np.array_equal(bits32(w[t, :k]), bits32(w_ref[t, :k])):
            return False
    return True


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_model_equals_the_oracle(name, block, oracle):
    case = get_case(name)
    w_ref, nit_ref = oracle_answers(name)
    w, nit, unfinished = kernel_model(name, block)
    assert nit.tolist() == nit_ref.tolist()
    for t in range(len(case.targets)):
        k = int(case.sel_count[t])
        if nit_ref[t] > 0:
            assert np.array_equal(bits32(w[t, :k]), bits32(w_ref[t, :k])), f"target {t}: weight bits differ"
        assert np.all(bits32(w[t, k:]) == 0)
    assert unfinished[-1] == 0 and all(a >= b for a, b in zip(unfinished, unfinished[1:]))


# ---------------------------------------------------------------------------------------------- the cases are what they claim
def relevant_times(case, t, time_of_e):
    """Sorted steps of one epoch at which target t has a sample that matters (a live feature or y stored in its row)."""
    X, j = case.X, int(case.targets[t])
    rows = [X.indices[X.indptr[j]:X.indptr[j + 1]]]
    for col in case.sel[t, :case.sel_count[t]].tolist():
        if col != j:
            rows.append(X.indices[X.indptr[col]:X.indptr[col + 1]])
    rows = np.unique(np.concatenate(rows))
    return np.sort(np.asarray(time_of_e)[rows])


def test_lane_cases_store_a_full_row_in_a_selection_that_does_not_ascend():
    for name in [n for n in CASE_NAMES if n.startswith("lane_")]:
        case = get_case(name)
        K = case.cap
        r0 = case.note["r0"]
        assert case.X.shape == (130, 260) and np.all(case.sel_count == K)
        for t in range(2):
            s = case.sel[t]
            assert len(set(s.tolist())) == K and case.targets[t] not in s
            assert K < 3 or np.any(np.diff(s) < 0)
            assert np.all(np.asarray(case.X[r0, s].todense()).ravel() != 0), "r0 stores every selected feature"
        m = prepared(name, 16)[0][2]
        assert m["time_of"][0][r0] == 129


def test_one_lane_cases_walk_the_lanes():
    """Replayed on the inputs the kernel gets: in epoch 0 the feature steps' minimum sits in ONE lane, in the order 63, 0, 15,
    16, 31, 32, 47, 48, then every other lane; at K = 256 the register index changes along the walk too."""
    for K in (64, 256):
        name = f"one_lane_{K}"
        case = get_case(name)
        first, ne, m, tt, tv = prepared(name, 16)[0]
        assert np.all(np.diff(case.X.indptr)[case.sel[0]] == 1), "one entry per feature column"
        t_of_pos = np.array([tt[0][case.X.indptr[c]] for c in case.sel[0]])
        order = np.argsort(t_of_pos)
        assert len(set(t_of_pos.tolist())) == K
        assert (order % 64)[:8].tolist() == LANE_ORDER
        assert sorted((order % 64)[:64].tolist()) == list(range(64))
        if K == 256:
            assert len(set((order // 64)[:8].tolist())) == 4
        rel = relevant_times(case, 0, m["time_of"][0])
        assert len(rel) > K + K // 4, "y has samples of its own between the feature steps"


def test_gap_cases_have_their_gaps_and_their_resets():
    for pname in ("default", "frequent", "degenerate", "all_zero", "dense"):
        name = f"gap_{pname}"
        case = get_case(name)
        m = prepared(name, 16)[0][2]
        U = case.U
        relA = relevant_times(case, 0, m["time_of"][0])
        assert relA.tolist() == list(GAP_TIMES) and np.diff(relA).tolist() == [1, 63, 64, 65, 200]
        assert relevant_times(case, 1, m["time_of"][0]).tolist() == [U - 1]
        assert case.X.indptr[3] == case.X.indptr[2] and np.all(np.diff(case.X.indptr)[[11, 12, 13]] == 0)   # C: nothing at all
        resets = np.flatnonzero(np.diff(m["reset_cnt"]))     # global steps with a reset
        if pname == "default":
            assert resets.size == 0
            continue
        on_skipped = on_sample = several = 0
        for t in (0, 1, 3):
            rel = np.concatenate([relevant_times(case, t, m["time_of"][ep]) + ep * U for ep in range(case.max_iter)])
            on_sample += int(np.isin(resets, rel).sum())
            on_skipped += int((~np.isin(resets, rel)).sum())
            # resets strictly between two consecutive samples (epoch borders included: the drain and the next epoch's first
            # sample share them out)
            between = np.searchsorted(resets, rel[1:], side="left") - np.searchsorted(resets, rel[:-1], side="right")
            several += int((between >= 2).sum())
        assert on_skipped >= 1 and on_sample >= 1 and several >= 1, (pname, on_skipped, on_sample, several)
        if pname == "all_zero":
            assert resets.size == U * case.max_iter and np.all(m["reset_mult"] == 0.0)
    # D sits on the reset steps of epoch 0
    case = get_case("gap_frequent")
    m = prepared("gap_frequent", 16)[0][2]
    resets0 = np.flatnonzero(np.diff(m["reset_cnt"][:case.U + 1]))
    relD = relevant_times(case, 3, m["time_of"][0])
    assert np.isin(relD, resets0).sum() >= 2 and resets0[0] in relD and resets0[0] + 1 in relD


def test_reset_end_cases_reset_on_the_last_step_of_a_block():
    assert reset_epoch_end_search() == (RESET_END_U, RESET_END_EPOCH)
    for extra in (0, 1):
        name = f"reset_end_{extra}"
        case = get_case(name)
        for block in BLOCKS:
            blocks = prepared(name, block)
            ends = [(first, ne, m) for first, ne, m, _, _ in blocks if first + ne == RESET_END_EPOCH + 1]
            if block == 16 and extra == 1:
                assert not ends                              # one block of 7 epochs: the control, the reset is inside it
                continue
            assert len(ends) == 1, "the epoch ends a block"
            first, ne, m = ends[0]
            assert m["reset_cnt"][ne * case.U] == m["reset_cnt"][ne * case.U - 1] + 1
            assert (first + ne == case.max_iter) == (extra == 0)


def test_stop_cases_stop_as_they_claim(oracle):
    _, nit = oracle_answers("stops_mixed")
    assert np.any((nit >= 6) & (nit <= 15)), nit            # stopped by n_iter_no_change inside the first block of 16
    assert np.any(nit == 20) and np.any((nit > 3) & (nit < 20)), nit
    assert oracle_answers("stops_max1")[1].tolist() == [1] * 10
    assert oracle_answers("stops_tolnone")[1].tolist() == [20] * 10
    w, nit = oracle_answers("diverge")
    assert nit.tolist()[:3] == [-1, -1, -1] and nit[3] > 0 and np.all(np.isfinite(w[3]))
    w, nit = oracle_answers("clip")
    assert nit[0] == 3 and np.all(np.isfinite(w[0])) and np.any(w[0] != 0)
    for s in STOP_ROUNDING_SEEDS:
        w, nit = oracle_answers(f"stop_rounding_{s}")
        assert 6 <= nit[0] < 40 and np.all(w[0] == 0)


def test_self_case_selects_the_target_itself():
    case = get_case("self")
    for t, pos in enumerate(case.note["self_pos"]):
        assert case.sel[t, pos] == case.targets[t] and len(set(case.sel[t].tolist())) == case.cap
        assert case.X.indptr[case.targets[t] + 1] > case.X.indptr[case.targets[t]]
    assert case.X.indptr[266] == case.X.indptr[265]
    assert np.all(np.diff(case.X.indptr)[case.sel[5, :3]] == 0)


# ---------------------------------------------------------------------------------------------- guards
# variant -> the named cases that are its witnesses: on each of them the variant must give other bits or another n_iter
WITNESSES = {
    "lanes_outer": ["lane_65_l2", "lane_129_l2", "lane_193_l2", "lane_256_l2"],
    "f32_sum": ["lane_64", "lane_129", "lane_256_l2", "count_256"],
    "drop_pending": ["gap_frequent", "gap_degenerate", "reset_end_1"],
    "own_reset_first": ["gap_dense", "gap_all_zero", "reset_end_0", "reset_end_1"],
    "skip_y_only": [f"stop_rounding_{s}" for s in STOP_ROUNDING_SEEDS],
    "eta_prev": ["gap_default", "one_lane_64", "one_lane_256"],
    "dead_192": ["lane_193", "lane_255", "lane_256", "self"],
    "no_clip": ["clip"],
}


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_guard_fires(variant, oracle):
    """A kernel that did what `variant` does would be caught: on every witness case the variant's answer differs from the
    oracle's (and the unmodified model's equals it: test_kernel_model_equals_the_oracle)."""
    for name in WITNESSES[variant]:
        case = get_case(name)
        w_ref, nit_ref = oracle_answers(name)
        w, nit, _ = kernel_model(name, 16, variant)
        assert not same_answer(case, w, nit, w_ref, nit_ref), f"{variant} changes nothing on {name}"


# ---------------------------------------------------------------------------------------------- the fuzzer's seed
FUZZ_SEED, FUZZ_N = 4, 40          # test_sgd_path_randomised_parity (tests/test_gpu_kernels.py)
FUZZ_COVER_N = 12                  # the seed is chosen on its first 12 draws; the later ones ride along


def test_fuzz_seed_draws_what_it_is_chosen_for():
    """tools/fuzz_fit.py draws its configurations on the host: seed 4 is the first whose 12 draws hold every one of these."""
    from tools.fuzz_fit import sgd_configs

    def covered(seed):
        cs = list(sgd_configs(FUZZ_COVER_N, seed))
        return (any(c["cfg"]["nn_feature_selection"] > 192 and c["I"] == 300 for c in cs),
                any(65 <= c["cfg"]["nn_feature_selection"] <= 128 for c in cs),
                any(c["tol"] is None for c in cs),
                any(c["negative"] and np.any(c["X"].data < 0) for c in cs),
                any(c["cfg"]["eta0"] == 0.3 and c["cfg"]["alpha"] == 1.0 for c in cs))
    assert all(covered(FUZZ_SEED))
    assert not any(all(covered(s)) for s in range(FUZZ_SEED))
    assert max(c["U"] * c["cfg"]["max_iter"] for c in sgd_configs(FUZZ_COVER_N, FUZZ_SEED)) == 2500 * 40
