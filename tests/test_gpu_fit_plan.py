"""The fit's host path asks the device for the same work as before it was split into a plan (rtrec_amd/fit_plan.py) and its
execution: every case of tests/fit_call_log.py is replayed on a fresh engine and its op log compared, entry for entry, with
tests/golden/fit_calls.json -- recorded by the same module at the commit the file names, i.e. BEFORE the change, never with
the code under test.  Cases 'bulk', 'bulk_pilot', 'latency' and 'allf_overflow' are also compared bit for bit with the CPU
oracle: the heavy-head split and the Gram pilot below workload size.
"""
import json
import os

import numpy as np
import pytest

from tests import fit_call_log as fcl

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "fit_calls.json")) as _f:
    GOLDEN = json.load(_f)

ORACLE_CASES = ("bulk", "bulk_pilot", "latency", "allf_overflow")
_oracle_fits = {}


def oracle_fit(oracle, shape, K, tg):
    """oracle.fit_columns of every column of the case's matrix in the engine's processing order, computed once per (matrix, K)."""
    if (shape, K) not in _oracle_fits:
        _oracle_fits[(shape, K)] = (tg.copy(), oracle.fit_columns(fcl.matrix(shape)[0], tg, nn_feature_selection=K))
    tg0, fit = _oracle_fits[(shape, K)]
    assert np.array_equal(tg0, tg)
    return fit


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_exact(oracle, name, out):
    shape, K = fcl.CASES[name][:2]
    tg, items, coef, count, n_iter = out
    ptr, idx, val, nit = oracle_fit(oracle, shape, K, tg)
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


def test_golden_names_its_commit_and_every_case():
    assert len(GOLDEN["recorded_at_commit"]) == 40
    assert set(GOLDEN["cases"]) == set(fcl.CASES)


def fits(calls):
    return [c for c in calls if c["op"] == "fit_columns"]


def check_bulk(calls, eng):
    """Not measured but derived (U = 4000, I = 2600: 163,978 entries, 87 columns with >= 256 users).  The call is a 'small
    call' (n <= 4096): the head takes min(4 x 256, 2600 - 2049, 87 columns with >= 2048 / 8 users) = 87 targets on the side
    stream with 87 slots; no pilot below 8 M entries, so MAX_SLOTS capped by n = 2600 slots, the main launch has the other
    2513 targets and as many slots; X is non-negative and n > 2048: Gram tracking with the default 512 items.  (The op's
    n_slots is that of the scratch the launch got: 87 rounded up to a power of two, 2513 likewise but not beyond `slots`.)"""
    st = eng.last_fit_stats
    assert (st["n_targets"], st["slots"], st["cap"], st["n_heavy"]) == (2600, 2600, 20, 87)
    assert [c["top_items"] for c in calls if c["op"] == "gram_matrix"] == [512]
    heavy, main = fits(calls)
    assert (heavy["n_targets"], heavy["n_slots"], heavy["default_stream"], heavy["xty_ws"]) == (87, 128, False, False)
    assert (main["n_targets"], main["n_slots"], main["default_stream"]) == (2513, 2600, True)
    assert heavy["gram"] and main["gram"] and heavy["gram_n"] == main["gram_n"] == 512 and heavy["fast"] == main["fast"] == 0
    assert [(ln.lo, ln.hi, ln.n_slots, ln.role, ln.one_pass_xty) for ln in st["plan"].launches] == [
        (0, 87, 87, "heavy", False), (87, 2600, 2513, "main", False)]
    assert st["plan"].use_gram and st["plan"].heavy_slots == 512


def check_bulk_pilot(calls, eng):
    from rtrec_amd import fit_plan
    pilot = fits(calls)[0]
    assert len(fits(calls)) == 3
    assert [c["op"] for c in calls[:3]] == ["fit_workspace_init", "fit_columns", "gram_matrix"]      # ahead of the Gram matrix, whose size it decides
    assert (pilot["n_targets"], pilot["n_slots"], pilot["max_iter"], pilot["xty_ws"], pilot["gram"]) == (64, 64, 1, False, False)
    density = eng._X["pilot_feature_density"]
    assert 0.0 < density <= 1.0
    assert eng.last_fit_stats["slots"] == min(fit_plan.fit_slots_for_density(density), 2600)
    assert not [k for k in eng._fit_ws if k[4] == "pilot"]      # its scratch is dropped after use


def check_overflow(calls, eng):
    first, refit = fits(calls)
    assert (first["cap"], refit["cap"]) == (8, 200) and 0 < refit["n_targets"] <= 200


def check_scratch_reuse(calls, eng):
    assert len([c for c in calls if c["op"] == "fit_workspace_init"]) == 1
    assert [(c["n_targets"], c["n_slots"]) for c in fits(calls)] == [(300, 300), (200, 300), (300, 300)]


def one_fit(**want):
    def check(calls, eng):
        (c,) = fits(calls)
        assert {k: c[k] for k in want} == want
    return check


def check_shuffle(calls, eng):
    one_fit(fast=1, gram=False, n_targets=2600, default_stream=True)(calls, eng)       # no head ...
    assert not [c for c in calls if c["op"] == "gram_matrix"]                           # ... and no Gram matrix


def check_gram_mode(calls, eng):
    assert len(fits(calls)) == 2 and all(c["fast"] == 2 and c["gram"] for c in fits(calls))      # Gram-form coordinate descent


def main_launch(**want):
    def check(calls, eng):
        heavy, main = fits(calls)
        assert not heavy["default_stream"] and {k: main[k] for k in want} == want
    return check


def heavy_launch(**want):
    def check(calls, eng):
        heavy, main = fits(calls)
        assert {k: heavy[k] for k in want} == want and heavy["n_targets"] + main["n_targets"] == 2600
    return check


# what each case is there for, asserted on the replayed log itself
CHECKS = {
    "bulk": check_bulk,
    "bulk_pilot": check_bulk_pilot,
    "bulk_shuffle": check_shuffle,
    "bulk_gram": check_gram_mode,
    "latency": one_fit(xty_ws=False, col_order=False, n_targets=800),        # too little traffic for the one pass to pay
    "latency_xty_force": one_fit(xty_ws=True, col_order=True),
    "latency_xty_off": one_fit(xty_ws=False),
    "repeated_target": one_fit(xty_ws=False, n_targets=4),
    "repeated_target_xty_force": one_fit(xty_ws=False, n_targets=4),
    "allf_overflow": check_overflow,
    "scratch_reuse": check_scratch_reuse,
    "bulk_n_slots_512": main_launch(n_slots=512),
    "bulk_env_slots_768": main_launch(n_slots=768),
    "bulk_heavy_min_rows_64": heavy_launch(n_targets=500, n_slots=512),      # 500 columns have >= 64 users; 2 x 256 heavy slots
    "bulk_heavy_off": one_fit(n_targets=2600, default_stream=True),
}


@pytest.mark.parametrize("name", list(fcl.CASES))
def test_fit_asks_the_device_for_the_same_work(name, oracle, monkeypatch):
    calls, outs, eng = fcl.run_case(name, monkeypatch)
    want = GOLDEN["cases"][name]
    for k, (got, exp) in enumerate(zip(calls, want["calls"])):
        assert got == exp, f"op call {k} differs"
    assert len(calls) == len(want["calls"]), [c["op"] for c in calls]
    stats = {k: int(eng.last_fit_stats[k]) for k in want["last_fit_stats"]}
    assert stats == want["last_fit_stats"]
    CHECKS[name](calls, eng)
    if name in ORACLE_CASES:
        assert_bit_exact(oracle, name, outs[-1])
