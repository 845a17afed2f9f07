#!/usr/bin/env python3
"""What explanations cost: SLIM.explain_batch over ALL users of a bench.py workload (top-10, top_m = 3).

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Timed with device events on the engine's
stream, after one untimed call each:

  explain_launch_ms      eng.explain_device alone, on lists that are already resident (score_topk_device's output)
  score_launch_ms        eng.score_topk_device alone, the same rows (this build) -- the pass the explanation rides on
  explain_batch_ms       SLIM.explain_batch(users, as_arrays=True) end to end: scoring, explanation, five downloads
  host_model_s           the scipy-vectorised host model of tests/test_explain_host.py on the same lists (wall clock), whose
                         output the device's must equal (ids, contribution bits, support)

`--parent-bench FILE`: the JSON line of a `bench.py --workload W` run at the PARENT commit; its ms_per_step is recorded beside
the figures so that a reader sees what an explanation costs relative to the scoring step.  Writes
profiles/explain_<workload>.json with the build fingerprint.

    python tools/explain_bench.py --workload c3 --parent-bench parent_c3.json
    python tools/explain_bench.py --workload c3 --launch-only 20      # only the two launches: the run to put under
                                                                      # `rocprofv3 --kernel-trace --stats`

One process; every GPU step runs under its own time limit and nothing is started after a step that overran or failed."""
import argparse
import contextlib
import io
import json
import os
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
    """One step under its own limit: overrunning it raises out of the step (and ends the run)."""
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
        print(f"[explain_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--top-m", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--launch-only", type=int, default=0, metavar="N", help="N launches of scoring + explanation and nothing else")
    ap.add_argument("--parent-bench", default=None, help="file holding the JSON line of bench.py at the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"explain_{args.workload}.json")

    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.synth import workload_matrix
    from tests.test_explain_host import host_model_vectorised
    wl = WORKLOADS[args.workload]
    X = workload_matrix(wl)
    U, I = X.shape
    coo = X.tocoo()
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    model = SLIM(min_value=0, max_value=15, nn_feature_selection=wl["K"])
    with step("fit", 900), contextlib.redirect_stdout(io.StringIO()):
        model.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64),
                                       1.7e9 + np.arange(coo.nnz, dtype=np.float64), coo.data.astype(np.float64))
        model.bulk_fit(parallel=True, progress_bar=False)
        torch.cuda.synchronize()
    eng = model.model.engine
    users = np.arange(U, dtype=np.int64)
    k, m = args.top_k, args.top_m

    def timed(fn, n):
        """Device-event spans (ms) of n calls on the current stream."""
        out, last = [], None
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            last = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out, last

    with step("warm-up", 300):
        first = model.explain_batch(users, top_k=k, top_m=m, as_arrays=True)          # syncs W and X, builds the layouts
        d_rows = eng.be.to_dev(users.astype(np.int32))
        score = lambda: eng.score_topk_device(None, U, k, True, _native.TOPK_SPARSE, d_rows=d_rows)
        d_ids, _, d_cnt = score()
        d_ids, d_cnt = d_ids.contiguous(), d_cnt.contiguous()
        explain = lambda: eng.explain_device(d_rows, U, None, d_ids, d_cnt, m)
        explain()
        torch.cuda.synchronize()
    reps = args.launch_only or args.reps
    with step("launches", 300):
        score_ms, _ = timed(score, reps)
        explain_ms, dev = timed(explain, reps)
    if args.launch_only:
        print(json.dumps({"score_launch_ms": score_ms, "explain_launch_ms": explain_ms}))
        return 0
    with step("explain_batch", 600):
        e2e_ms, last = timed(lambda: model.explain_batch(users, top_k=k, top_m=m, as_arrays=True), max(3, args.reps // 2))
    ids, counts = d_ids.cpu().numpy(), d_cnt.cpu().numpy()
    got = tuple(t.cpu().numpy() for t in dev)
    Xs, W = model.interactions.to_csr(), model.model.item_similarity.tocsc()
    Xs.sort_indices(); W.sort_indices()
    with step("host model", 1800):
        t0 = time.perf_counter()
        want = host_model_vectorised(Xs, W, users, ids, counts, m, chunk=16384)
        host_s = time.perf_counter() - t0
    same = (np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            and np.array_equal(got[2], want[2]) and np.array_equal(last[0], ids) and np.array_equal(last[2], want[0])
            and np.array_equal(last[4], want[2]) and np.array_equal(first[2], want[0]))
    parent = None
    if args.parent_bench:
        for line in open(args.parent_bench):
            line = line.strip()
            if line.startswith("{") and "ms_per_step" in line:
                parent = json.loads(line)
    live = want[2][want[2] > 0]
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "w_nnz": int(W.nnz),
           "top_k": k, "top_m": m, "pairs": int(counts.sum()),
           "support": {"max": int(want[2].max()), "median": int(np.median(live)) if live.size else 0, "mean": float(live.mean()) if live.size else 0.0},
           "explain_launch_ms": explain_ms, "score_launch_ms": score_ms, "explain_batch_ms": e2e_ms, "host_model_s": host_s,
           "explain_launch_ms_median": float(np.median(explain_ms)), "score_launch_ms_median": float(np.median(score_ms)),
           "explain_batch_ms_median": float(np.median(e2e_ms)),
           "device_faster_than_host_model": bool(max(e2e_ms) < host_s * 1e3), "same_as_host_model": bool(same),
           "score_path": getattr(eng, "last_score_path", None),
           "parent_bench": None if parent is None else {"ms_per_step": parent.get("ms_per_step"), "users_per_sec": parent.get("value", parent.get("users_per_sec")),
                                                        "steps": parent.get("steps"), "build": parent.get("build")},
           "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
