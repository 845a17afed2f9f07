"""What a fit asks the device to do, as data: a pass-through proxy in place of `engine.be.ops` that records the scalar view
of every fit_columns, fit_workspace_init and gram_matrix op call, and the cases tests/test_gpu_fit_plan.py replays.  TEST-ONLY.

Only the public API of SlimEngine and `be.ops` are used, so the same module records tests/golden/fit_calls.json at the commit
BEFORE a change of the fit's host path and replays it after:

    python -m tests.fit_call_log <parent hash> > tests/golden/fit_calls.json      (on the GPU, at that commit)
"""
from __future__ import annotations

import json
import sys
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

# argument names of torch.ops.rtrec_amd.fit_columns in schema order (csrc/torch_ops.cpp)
FIT_ARGS = ("cptr crow cval rptr rcol rval sqn targets n_users n_items l1_reg l2_reg tol max_iter seed positive top_features "
            "out_items out_coef out_count out_n_iter cap ws n_slots queue trace gram gram_index gram_n gram_rel_err fast kernel "
            "colwalk_min_rows screen_min lane_max xty_ws col_order fold").split()
FIT_SCALARS = ("cap", "n_slots", "fast", "kernel", "colwalk_min_rows", "screen_min", "lane_max", "fold", "max_iter", "top_features",
               "gram_n")
FIT_PRESENT = ("trace", "gram", "xty_ws", "col_order")

# every environment switch of the fit: a case starts with all of them unset
FIT_ENV = ["RTREC_AMD_FIT_SLOTS", "RTREC_AMD_FIT_SCRATCH_GIB", "RTREC_AMD_FIT_HEAVY", "RTREC_AMD_FIT_HEAVY_SLOTS",
           "RTREC_AMD_FIT_HEAVY_MIN_ROWS", "RTREC_AMD_ALLF_CAP", "RTREC_AMD_GRAM", "RTREC_AMD_GRAM_ITEMS", "RTREC_AMD_XTY_BATCH",
           "RTREC_AMD_FIT_MODE", "RTREC_AMD_COLWALK_MIN", "RTREC_AMD_SCREEN_MIN", "RTREC_AMD_LANE_MAX", "RTREC_AMD_FOLD",
           "RTREC_AMD_DEBUG_XTY"]


class OpsLog:
    """Stands where `be.ops` stood; every op passes through, the three of the fit leave an entry in `calls` first."""

    def __init__(self, engine):
        self._ops = engine.be.ops
        self._torch, self._device = engine.be.torch, engine.be.device
        self.calls: List[Dict[str, Any]] = []
        engine.be.ops = self

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def _default_stream(self) -> bool:
        cuda = self._torch.cuda
        return cuda.current_stream(self._device) == cuda.default_stream(self._device)

    def fit_columns(self, *args):
        a = dict(zip(FIT_ARGS, args))
        assert len(args) == len(FIT_ARGS)
        tg = a["targets"].cpu().numpy()
        e: Dict[str, Any] = {"op": "fit_columns", "n_targets": int(tg.shape[0]),
                             "first": int(tg[0]) if len(tg) else None, "last": int(tg[-1]) if len(tg) else None}
        e.update({k: int(a[k]) for k in FIT_SCALARS})
        e.update({k: a[k] is not None for k in FIT_PRESENT})
        e["default_stream"] = self._default_stream()
        self.calls.append(e)
        return self._ops.fit_columns(*args)

    def fit_workspace_init(self, ws, n_users, n_items, n_slots, top_features):
        self.calls.append({"op": "fit_workspace_init", "n_users": int(n_users), "n_items": int(n_items), "n_slots": int(n_slots),
                           "top_features": int(top_features)})
        return self._ops.fit_workspace_init(ws, n_users, n_items, n_slots, top_features)

    def gram_matrix(self, cptr, crow, cval, top_items, ws, gram, n_users, n_items):
        self.calls.append({"op": "gram_matrix", "n_users": int(n_users), "n_items": int(n_items), "top_items": int(top_items.size(0))})
        return self._ops.gram_matrix(cptr, crow, cval, top_items, ws, gram, n_users, n_items)


BULK = (4000, 2600, 200000)       # 163,978 entries, 87 columns with >= 256 users: the smallest-ish call with a heavy head
LATENCY = (3000, 800, 90000)
ALLF = (600, 200, 12000)
ALL = None                        # targets: every column

# name -> (matrix, K, environment, pilot forced, [(targets, keyword arguments of fit_columns), ...]); one fresh engine per case
CASES: Dict[str, Tuple[Tuple[int, int, int], Optional[int], Dict[str, str], bool, List[Tuple[Any, Dict[str, Any]]]]] = {
    "bulk": (BULK, 20, {}, False, [(ALL, {})]),
    "bulk_pilot": (BULK, 20, {}, True, [(ALL, {})]),
    "bulk_shuffle": (BULK, 20, {}, False, [(ALL, {"mode": "shuffle"})]),
    "bulk_gram": (BULK, 20, {}, False, [(ALL, {"mode": "gram"})]),
    "latency": (LATENCY, 50, {}, False, [(ALL, {})]),
    "latency_xty_force": (LATENCY, 50, {"RTREC_AMD_XTY_BATCH": "force"}, False, [(ALL, {})]),
    "latency_xty_off": (LATENCY, 50, {"RTREC_AMD_XTY_BATCH": "0"}, False, [(ALL, {})]),
    "repeated_target": (LATENCY, 50, {}, False, [([5, 9, 5, 700], {})]),
    "repeated_target_xty_force": (LATENCY, 50, {"RTREC_AMD_XTY_BATCH": "force"}, False, [([5, 9, 5, 700], {})]),
    "allf_overflow": (ALLF, None, {"RTREC_AMD_ALLF_CAP": "8"}, False, [(ALL, {})]),
    "scratch_reuse": (LATENCY, 50, {}, False, [(range(300), {}), (range(200), {}), (range(300), {})]),
    "bulk_n_slots_512": (BULK, 20, {}, False, [(ALL, {"n_slots": 512})]),
    "bulk_env_slots_768": (BULK, 20, {"RTREC_AMD_FIT_SLOTS": "768"}, False, [(ALL, {})]),
    "bulk_heavy_min_rows_64": (BULK, 20, {"RTREC_AMD_FIT_HEAVY_MIN_ROWS": "64"}, False, [(ALL, {})]),
    "bulk_heavy_off": (BULK, 20, {"RTREC_AMD_FIT_HEAVY": "0"}, False, [(ALL, {})]),
}

_matrices: Dict[Tuple[int, int, int], Any] = {}


def matrix(shape: Tuple[int, int, int]):
    """(CSC, CSR) of synth.interaction_matrix(U, I, draws, seed=31), built once per shape."""
    if shape not in _matrices:
        from rtrec_amd.synth import interaction_matrix
        X = interaction_matrix(*shape, seed=31)
        Xc = X.tocsc()
        Xc.sort_indices()
        _matrices[shape] = (Xc, X)
    return _matrices[shape]


def run_case(name: str, mp):
    """Runs one case on a fresh engine on cuda:0.  `mp` is a pytest.MonkeyPatch.  Returns (the op log, the results of the
    fit_columns calls, the engine)."""
    from rtrec_amd.engine import SlimEngine
    shape, K, env, pilot, calls = CASES[name]
    for k in FIT_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    if pilot:
        mp.setattr(SlimEngine, "GRAM_PILOT_MIN_NNZ", 0)
    Xc, X = matrix(shape)
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(Xc, X)
    log = OpsLog(eng)
    outs = []
    for targets, kw in calls:
        tg = np.arange(shape[1]) if targets is None else np.asarray(list(targets))
        outs.append(eng.fit_columns(tg, nn_feature_selection=K, **kw))
    return log.calls, outs, eng


def record(commit: str) -> Dict[str, Any]:
    import pytest
    out: Dict[str, Any] = {"recorded_at_commit": commit, "cases": {}}
    for name in CASES:
        with pytest.MonkeyPatch.context() as mp:
            calls, _, eng = run_case(name, mp)
            st = eng.last_fit_stats
            out["cases"][name] = {"calls": calls,
                                  "last_fit_stats": {k: int(st[k]) for k in ("n_targets", "slots", "cap", "n_heavy")}}
    return out


if __name__ == "__main__":
    json.dump(record(sys.argv[1]), sys.stdout, indent=1)
    print()
