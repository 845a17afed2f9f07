#!/usr/bin/env python3
"""What the audience of an item costs: SLIM.recommend_users_batch on a bench.py workload, all users resident.

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Query items: n_q of a fixed-seed permutation of
the catalogue, for n_q in 1, 64, 1024.  Timed with device events on the engine's stream, after `--warmup` untimed calls each
(`--reps` timed ones; medians are reported beside the raw spans):

  device_call_ms[n_q][top_n]  one eng.audience_device call, top_n in 10, 1024: its output and workspace allocations and the two
                              launches (audience_tile_kernel + audience_merge_kernel), results left in HBM.  At n_q = 1 this is
                              mostly launch and allocation; the kernels' own time comes from the rocprofv3 run below
  e2e_ms[n_q]                 SLIM.recommend_users_batch(items, top_n, as_arrays=True) end to end (top_n = --e2e-top-n)
  host_model_s[n_q]           the numpy host model of tests/test_audience_host.py on the same items (wall clock; n_q <= 64),
                              whose output the device's must equal (ids, score bits, counts, eligible)
  assembled_ms[n_q][top_n]    the route a caller can assemble from what exists: the candidates scoring of ALL users for the
                              same items with top_k = n_q (engine.score_topk_device(candidates=...)), a scatter of the (user,
                              item, score) lists into an items x users matrix and torch.topk over the users, on the device.
                              Its pieces are unchanged by the audience kernel, so timing them in the same build stands in for
                              the parent commit.  (torch.topk breaks ties its own way: the route is timed, not compared.)
  score_all_users_ms          for context: the plain top-10 scoring step of all users, this build
  products[n_q]               sum over the query items i and the rows j of W[:, i] of nnz(X[:, j]): the multiply-adds of the walk

Writes profiles/audience_<workload>.json with the build fingerprint.

    python tools/audience_bench.py --workload c3s
    python tools/audience_bench.py --workload c3s --launch-only 20    # only audience_device calls (largest n_q): the run to put
                                                                      # under `rocprofv3 --kernel-trace --stats`

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
        print(f"[audience_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-top-n", type=int, default=100)
    ap.add_argument("--launch-only", type=int, default=0, metavar="N", help="N audience_device calls at the largest n_q and nothing else")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"audience_{args.workload}.json")

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.synth import workload_matrix
    from tests.test_audience_host import host_model
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
    perm = np.random.default_rng(20251017).permutation(I)
    queries = {n: perm[:n].astype(np.int32) for n in (1, 64, 1024) if n <= I}

    def timed(fn, n):
        """Device-event spans (ms) of n calls on the current stream, after args.warmup untimed ones."""
        out, last = [], None
        for r in range(args.warmup + n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            last = fn()
            b.record()
            b.synchronize()
            if r >= args.warmup:
                out.append(a.elapsed_time(b))
        return out, last

    with step("warm-up", 300):
        first = model.recommend_users_batch(queries[1].tolist(), top_n=10, as_arrays=True)      # syncs W and X (both orientations)
        torch.cuda.synchronize()
    d_q = {n: eng.be.to_dev(q) for n, q in queries.items()}
    if args.launch_only:
        with step("launches", 300):
            n_big = max(queries)
            ms = {t: timed(lambda: eng.audience_device(d_q[n_big], n_big, t, True), args.launch_only)[0] for t in (10, 1024)}
        print(json.dumps({"n_q": n_big, "device_call_ms": ms}))
        return 0

    kernel, dev = {}, {}
    with step("kernel", 600):
        for n in queries:
            kernel[n] = {}
            for t in (10, 1024):
                kernel[n][t], out = timed(lambda: eng.audience_device(d_q[n], n, t, True), args.reps)
                dev[(n, t)] = tuple(x.cpu().numpy() for x in out)
    e2e = {}
    with step("recommend_users_batch", 600):
        for n, q in queries.items():
            items = q.tolist()
            e2e[n], _ = timed(lambda: model.recommend_users_batch(items, top_n=args.e2e_top_n, as_arrays=True), max(3, args.reps // 2))

    Xc, W = model.interactions.to_csc(), model.model.item_similarity.tocsc()
    Xc.sort_indices(); W.sort_indices()
    col_nnz = np.diff(Xc.indptr).astype(np.int64)
    work = np.asarray(sp.csc_matrix((np.ones(W.nnz, np.int64), W.indices, W.indptr), shape=W.shape).T @ col_nnz).ravel()
    host_s, same = {}, True
    with step("host model", 1800):
        for n, q in queries.items():
            if n > 64:
                continue
            t0 = time.perf_counter()
            want = host_model(Xc, W, q, 1024)
            host_s[n] = time.perf_counter() - t0
            for t in (10, 1024):
                g = dev[(n, t)]
                same &= bool(np.array_equal(g[0], want[0][:, :t]) and np.array_equal(g[1].view(np.uint32), want[1][:, :t].view(np.uint32))
                             and np.array_equal(g[2], np.minimum(want[2], t)) and np.array_equal(g[3], want[3]))
            if n == 1:
                same &= bool(np.array_equal(first[0], want[0][:, :10]) and np.array_equal(first[3], want[3]))

    # the route assembled from what exists: candidates scoring of all users, then a top-k over the users per item
    d_rows = eng.be.to_dev(np.arange(U, dtype=np.int32))
    assembled, assembled_path = {}, {}

    def assemble(n, t):
        q = queries[n]
        ids, sc, cnt = eng.score_topk_device(None, U, n, False, _native.TOPK_CANDIDATES, d_rows=d_rows, candidates=q)
        col = torch.full((I,), -1, dtype=torch.int64, device=ids.device)
        col[d_q[n].long()] = torch.arange(n, device=ids.device)
        live = torch.arange(n, device=ids.device)[None, :] < cnt[:, None]
        dense = torch.full((n, U), float("-inf"), dtype=torch.float32, device=ids.device)
        u_idx = torch.arange(U, device=ids.device)[:, None].expand(U, n)[live]
        dense[col[ids[live].long()], u_idx] = sc[live]
        return torch.topk(dense, min(t, U), dim=1)

    with step("assembled route", 900):
        for n in queries:
            assembled[n] = {}
            for t in (10, 1024):
                try:
                    assembled[n][t], _ = timed(lambda: assemble(n, t), max(3, args.reps // 2))
                except (ValueError, NotImplementedError) as e:      # a list length the existing scoring path does not serve
                    assembled[n][t] = []
                    assembled_path[n] = f"not served: {e}"
            assembled_path.setdefault(n, getattr(eng, "last_score_path", None))
    with step("plain scoring", 300):
        score_ms, _ = timed(lambda: eng.score_topk_device(None, U, 10, True, _native.TOPK_SPARSE, d_rows=d_rows), args.reps)

    med = lambda v: float(np.median(v)) if len(v) else None
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "w_nnz": int(W.nnz),
           "warmup_calls": args.warmup, "timed_calls": args.reps, "timing": "device events around each call, one stream, medians beside the raw spans",
           "e2e_top_n": args.e2e_top_n,
           "products": {str(n): int(work[q].sum()) for n, q in queries.items()},
           "device_call_ms": {str(n): {str(t): v for t, v in d.items()} for n, d in kernel.items()},
           "device_call_ms_median": {str(n): {str(t): med(v) for t, v in d.items()} for n, d in kernel.items()},
           "products_per_s": {str(n): {str(t): float(work[queries[n]].sum() / (med(v) * 1e-3)) for t, v in d.items()} for n, d in kernel.items()},
           "e2e_ms": {str(n): v for n, v in e2e.items()}, "e2e_ms_median": {str(n): med(v) for n, v in e2e.items()},
           "host_model_s": {str(n): v for n, v in host_s.items()},
           "assembled_ms": {str(n): {str(t): v for t, v in d.items()} for n, d in assembled.items()},
           "assembled_ms_median": {str(n): {str(t): med(v) for t, v in d.items()} for n, d in assembled.items()},
           "assembled_score_path": {str(n): p for n, p in assembled_path.items()},
           "device_call_faster_than_assembled": {str(n): {str(t): (None if not assembled[n][t] else bool(med(kernel[n][t]) < med(assembled[n][t]))) for t in (10, 1024)} for n in queries},
           "score_all_users_ms": score_ms, "score_all_users_ms_median": med(score_ms),
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
