#!/usr/bin/env python3
"""Recommender.evaluate over ALL users of a bench.py workload, host path against on_device=True.

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K); a seeded held-out frame names every user;
each path is called once untimed and then three times under the wall clock, frame preparation included.  The two dicts
must be equal.  Writes profiles/evaluate_<workload>.json with the build fingerprint.

    python tools/evaluate_bench.py --workload c3                    # both paths, the summary
    python tools/evaluate_bench.py --workload c3 --device-only 5    # only the device path, 5 calls: the run to put under
                                                                    # `rocprofv3 --kernel-trace --stats` for the kernel's own time
    python tools/evaluate_bench.py --kernel-stats <..._kernel_stats.csv>   # fold that run's figures into the summary

One process; every GPU step runs under its own time limit and nothing is started after a step that overran or failed."""
import argparse
import contextlib
import csv
import io
import json
import os
import re
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StepTimeout(RuntimeError):
    pass


@contextlib.contextmanager
def step(name: str, seconds: int):
    """One GPU step under its own limit: overrunning it raises out of the step (and ends the run)."""
    def on_alarm(signum, frame):
        raise StepTimeout(f"step '{name}' exceeded {seconds} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(seconds)
    t0 = time.perf_counter()
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
        print(f"[evaluate_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def held_out_frame(X, seed: int, per_user: int = 3):
    """Every user once with one of the 2,000 most popular items (so that lists hit), plus `per_user - 1` random rows per
    user on average (duplicated pairs included, as a real test frame has them), shuffled."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    U, I = X.shape
    pop = np.argsort(-np.bincount(X.indices, minlength=I))[:2000]
    users = np.concatenate([np.arange(U), rng.integers(0, U, U * (per_user - 1))])
    items = np.concatenate([pop[rng.integers(0, len(pop), U)], rng.integers(0, I, U * (per_user - 1))])
    order = rng.permutation(len(users))
    return pd.DataFrame({"user": users[order].astype(np.int64), "item": items[order].astype(np.int64)})


def kernel_stats(path: str) -> dict:
    """The rank_metrics_kernel row (and the scoring kernels beside it) of a rocprofv3 --kernel-trace --stats summary."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"(rank_metrics_kernel|score_\w+_kernel|fr_ties_kernel)", row.get("Name", ""))
            if m:
                out[m.group(1)] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                                   "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--size", type=int, default=10)
    ap.add_argument("--device-only", type=int, default=0, metavar="N", help="N calls of the device path and nothing else")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --device-only run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"evaluate_{args.workload}.json")
    if args.kernel_stats:
        res = json.load(open(out_path))
        res["kernel_trace"] = kernel_stats(args.kernel_stats)
        json.dump(res, open(out_path, "w"), indent=1)
        print(json.dumps(res["kernel_trace"]))
        return 0

    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, Recommender, build
    from rtrec_amd.synth import workload_matrix
    wl = WORKLOADS[args.workload]
    X = workload_matrix(wl)
    U, I = X.shape
    coo = X.tocoo()
    test = held_out_frame(X, seed=7)
    sink = io.StringIO()
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    rec = Recommender(SLIM(min_value=0, max_value=15, nn_feature_selection=wl["K"]))
    with step("fit", 600), contextlib.redirect_stdout(sink):
        rec.model.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64),
                                           1.7e9 + np.arange(coo.nnz, dtype=np.float64), coo.data.astype(np.float64))
        rec.model.bulk_fit(parallel=True, progress_bar=False)
        torch.cuda.synchronize()

    def timed(n: int, **kw):
        secs, last = [], None
        for _ in range(n):
            t0 = time.perf_counter()
            last = rec.evaluate(test, recommend_size=args.size, **kw)
            secs.append(time.perf_counter() - t0)
        return secs, last

    with step("device warm-up", 300):
        _, dev = timed(1, on_device=True)
    if args.device_only:
        with step("device", 300):
            secs, dev = timed(args.device_only, on_device=True)
        print(json.dumps({"device_s": secs, "scores": dev}))
        return 0
    with step("device", 300):
        dev_s, dev = timed(3, on_device=True)
    dev_path = getattr(rec.model.model.engine, "last_score_path", None)
    # where the device path's wall time goes: the frame -> CSR step alone (host, numpy), same columns
    from rtrec_amd.utils.metrics import ground_truth_csr
    same_id = lambda v: np.asarray(v, dtype=np.int64)
    prep_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        ground_truth_csr(test["user"].to_numpy(), test["item"].to_numpy(), same_id, same_id)
        prep_s.append(time.perf_counter() - t0)
    with step("host warm-up", 900):
        _, host = timed(1)
    with step("host", 1800):
        host_s, host = timed(3)
    same = list(dev) == list(host) and all(dev[k] == host[k] for k in host)
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz),
           "test_rows": int(len(test)), "test_users": int(test["user"].nunique()), "recommend_size": args.size,
           "host_s": host_s, "device_s": dev_s, "ground_truth_csr_s": prep_s, "device_faster_in_every_run": bool(max(dev_s) < min(host_s)),
           "speedup_min_over_max": min(host_s) / max(dev_s), "same_scores": bool(same), "scores": dev,
           "device_score_path": dev_path, "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
