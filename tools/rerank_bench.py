#!/usr/bin/env python3
"""What reranking per-user candidate lists costs: SLIM.rerank_batch / csrc/score_pairs.hip on a bench.py workload, all users
resident, every user with `--cands` (100) seeded candidates of its own, top_k = 10.

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Timed with device events on the engine's stream,
after `--warmup` untimed calls each (`--reps` timed ones; medians are reported beside the raw spans):

  device_call_ms[waves]       one eng.score_pairs_device call over all users (its output allocations and the one launch of
                              score_pairs_kernel, results left in HBM), waves_per_row = 1 and 4 ALTERNATING in one loop, so that
                              both see the same clocks and caches; `faster_waves_per_row` names the smaller median
  e2e_ms                      SLIM.rerank_batch(users, candidates, top_k, as_arrays=True) end to end (wall clock; the candidates
                              as one [B, k] integer array)
  host_model_s                the vectorised numpy host model of tests/test_rerank_host.py on the first `--host-users` users
                              (wall clock), whose output the device's must equal (score bits, support, order, count)
  per_user_recommend_batch    what the code without this kernel does for the same job: one recommend_batch([u],
                              candidate_items=c_u) per user, timed on a `--sample` (200) of the users and EXTRAPOLATED to all
  request_p50_ms              one user x `--request-cands` (500) candidates: rerank(u, c, top_k) against recommend(u,
                              candidate_items=c, top_k), p50 of `--reps` wall-clock calls each, and the device call of both
                              waves_per_row forms

Writes profiles/rerank_<workload>.json with the build fingerprint.

    python tools/rerank_bench.py --workload c3s

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
        print(f"[rerank_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--cands", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200, help="users of the one-call-per-user route (extrapolated to all)")
    ap.add_argument("--host-users", type=int, default=8192, help="users the host model is run and compared on")
    ap.add_argument("--request-cands", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"rerank_{args.workload}.json")

    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, build
    from rtrec_amd.synth import workload_matrix
    from tests.test_rerank_host import host_model_vectorised
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
    rng = np.random.default_rng(20251018)
    k, top_k = min(args.cands, I), min(args.top_k, args.cands, I)
    ids = rng.integers(0, I, (U, k)).astype(np.int32)
    counts = np.full(U, k, np.int32)
    users = np.arange(U, dtype=np.int64)

    def spans(fns, n):
        """Device-event spans (ms) of n rounds over the calls `fns` (name -> call), alternating, after args.warmup untimed rounds."""
        out, last = {name: [] for name in fns}, {}
        for r in range(args.warmup + n):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                last[name] = fn()
                b.record()
                b.synchronize()
                if r >= args.warmup:
                    out[name].append(a.elapsed_time(b))
        return out, last

    def wall(fn, n):
        out, last = [], None
        for r in range(args.warmup + n):
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            if r >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out, last

    with step("warm-up", 300):
        model.rerank_batch(users[:16], ids[:16], top_k=top_k, as_arrays=True)        # syncs W and X
        torch.cuda.synchronize()
    d_rows, d_ids, d_cnt = eng.be.to_dev(users.astype(np.int32)), eng.be.to_dev(ids), eng.be.to_dev(counts)
    with step("kernel", 600):
        kernel, last = spans({str(w): (lambda w=w: eng.score_pairs_device(d_rows, U, None, d_ids, d_cnt, top_k, False, waves_per_row=w))
                              for w in (1, 4)}, args.reps)
        dev = {w: tuple(t.cpu().numpy() for t in out) for w, out in last.items()}
    with step("rerank_batch", 900):
        e2e, arrays = wall(lambda: model.rerank_batch(users, ids, top_k=top_k, as_arrays=True), max(3, args.reps // 3))

    Xs, W = model.interactions.to_csr(), model.model.item_similarity.tocsc()
    Xs.sort_indices(); W.sort_indices()
    n_h = min(args.host_users, U)
    with step("host model", 1800):
        t0 = time.perf_counter()
        want = host_model_vectorised(Xs, W, users[:n_h], ids[:n_h], counts[:n_h], top_k, False)
        host_s = time.perf_counter() - t0
    same = True
    for w, g in dev.items():
        same &= bool(np.array_equal(g[0][:n_h].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(g[1][:n_h], want[1])
                     and np.array_equal(g[2][:n_h], want[2]) and np.array_equal(g[3][:n_h], want[3]))
    same &= bool(np.array_equal(arrays[0][:n_h], np.take_along_axis(ids[:n_h].astype(np.int64), want[2].astype(np.int64), axis=1))
                 and np.array_equal(arrays[2][:n_h], want[3]))

    sample = rng.permutation(U)[:min(args.sample, U)]
    with step("one call per user", 900):
        t0 = time.perf_counter()
        per_user = [model.recommend_batch([int(u)], candidate_items=ids[int(u)].tolist(), top_k=top_k) for u in sample.tolist()]
        torch.cuda.synchronize()
        per_user_s = time.perf_counter() - t0
    same &= all(row[0] == arrays[0][int(u), :len(row[0])].tolist() for u, row in zip(sample.tolist(), per_user))

    u0 = int(sample[0])
    c0 = rng.integers(0, I, min(args.request_cands, I)).tolist()
    d_u0, d_c0 = eng.be.to_dev(np.array([u0], np.int32)), eng.be.to_dev(np.asarray([c0], np.int32))
    d_n0 = eng.be.to_dev(np.array([len(c0)], np.int32))
    with step("request", 600):
        req_rerank, a = wall(lambda: model.rerank(u0, c0, top_k=top_k), args.reps * 3)
        req_recommend, b = wall(lambda: model.recommend(u0, candidate_items=c0, top_k=top_k), args.reps * 3)
        req_kernel, _ = spans({str(w): (lambda w=w: eng.score_pairs_device(d_u0, 1, None, d_c0, d_n0, top_k, False, waves_per_row=w))
                               for w in (1, 4)}, args.reps * 3)
    same &= a == b

    med = lambda v: float(np.median(v)) if len(v) else None
    pairs = int(U) * int(k)
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "w_nnz": int(W.nnz),
           "candidates_per_user": int(k), "top_k": int(top_k), "pairs": pairs, "warmup_calls": args.warmup, "timed_calls": args.reps,
           "timing": "device events around each call, one stream, the two waves_per_row forms alternating; wall clock where it says so",
           "device_call_ms": kernel, "device_call_ms_median": {w: med(v) for w, v in kernel.items()},
           "pairs_per_s": {w: pairs / (med(v) * 1e-3) for w, v in kernel.items()},
           "faster_waves_per_row": int(min(kernel, key=lambda w: med(kernel[w]))),
           "e2e_ms": e2e, "e2e_ms_median": med(e2e),
           "host_model_users": int(n_h), "host_model_s": host_s, "host_model_s_all_users_extrapolated": host_s * U / n_h,
           "per_user_recommend_batch": {"sample_users": int(len(sample)), "sample_s": per_user_s,
                                        "all_users_s_extrapolated": per_user_s * U / len(sample),
                                        "note": "one recommend_batch([u], candidate_items=c_u) per user; measured on the sample, EXTRAPOLATED to all users"},
           "request": {"candidates": len(c0), "rerank_ms": req_rerank, "rerank_p50_ms": med(req_rerank),
                       "recommend_ms": req_recommend, "recommend_p50_ms": med(req_recommend),
                       "device_call_ms_median": {w: med(v) for w, v in req_kernel.items()},
                       "faster_waves_per_row": int(min(req_kernel, key=lambda w: med(req_kernel[w])))},
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
