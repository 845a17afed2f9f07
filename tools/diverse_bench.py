#!/usr/bin/env python3
"""What diversified lists cost: SLIM.recommend_diverse_batch / csrc/diversify.hip on a bench.py workload, all users resident,
a pool of `--pool` (50) per user re-ranked to `--top-k` (10) at lambda = 1 - `--diversity` (0.7).

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Timed with device events on the engine's stream,
after `--warmup` untimed calls each (`--reps` timed ones; medians are reported beside the raw spans):

  device_call_ms[waves]       one eng.diversify_device call over all users' pools (its output allocations and the one launch of
                              diversify_lists_kernel, inputs and results in HBM), waves_per_row = 1 and 4 ALTERNATING in one
                              loop, so that both see the same clocks and caches; `faster_waves_per_row` names the smaller median
  scoring_ms / scoring_plus_diversify_ms
                              the top_k = pool scoring step the kernel follows (eng.score_topk_device), alone and with the
                              selection behind it, alternating
  e2e_ms                      SLIM.recommend_diverse_batch(users, as_arrays=True) end to end (wall clock), beside
                              recommend_batch(users, top_k, as_arrays=True)
  host_model_s                the vectorised numpy host model of tests/test_diverse_host.py on a SAMPLE of `--host-users` (200)
                              users (wall clock), whose output the device's must equal (order, count, value and penalty bits);
                              the all-users figure is an EXTRAPOLATION and marked as one
  request                     one user x a pool of `--request-pool` (500): the device call of both waves_per_row forms, and
                              recommend_diverse(u) p50 (wall clock)

Writes profiles/diverse_<workload>.json with the build fingerprint.

    python tools/diverse_bench.py --workload c3s

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
        print(f"[diverse_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--pool", type=int, default=50)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--diversity", type=float, default=0.3, help="lambda = 1 - diversity (0.3: lambda 0.7)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-users", type=int, default=200, help="users the host model is run and compared on (a sample)")
    ap.add_argument("--request-pool", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"diverse_{args.workload}.json")

    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.synth import workload_matrix
    from tests.test_diverse_host import host_model_vectorised
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
    pool, top_k = min(args.pool, I), min(args.top_k, args.pool, I)
    lam = np.float32(1.0 - args.diversity)
    users = np.arange(U, dtype=np.int64)
    mode = _native.TOPK_SPARSE

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
        model.recommend_diverse_batch(users[:16], top_k=top_k, pool=pool, diversity=args.diversity, as_arrays=True)   # syncs W and X
        torch.cuda.synchronize()
    d_rows = eng.be.to_dev(users.astype(np.int32))
    score = lambda k: eng.score_topk_device(None, U, k, True, mode, d_rows=d_rows)
    with step("pools", 300):
        d_ids, d_sc, d_cnt = score(pool)
        d_ids, d_sc, d_cnt = d_ids.contiguous(), d_sc.contiguous(), d_cnt.contiguous()
        torch.cuda.synchronize()
    with step("kernel", 600):
        kernel, last = spans({str(w): (lambda w=w: eng.diversify_device(d_ids, d_sc, d_cnt, top_k, lam, waves_per_row=w)) for w in (1, 4)},
                             args.reps)
        dev = {w: tuple(t.cpu().numpy() for t in out) for w, out in last.items()}

    def scored_and_diversified():
        i, s, c = score(pool)
        return eng.diversify_device(i, s, c, top_k, lam)

    with step("next to the scoring step", 600):
        beside, _ = spans({"scoring": lambda: score(pool), "scoring_plus_diversify": scored_and_diversified,
                           "scoring_top_k_only": lambda: score(top_k)}, args.reps)
    with step("recommend_diverse_batch", 900):
        n_e2e = max(3, args.reps // 3)
        e2e, arrays = wall(lambda: model.recommend_diverse_batch(users, top_k=top_k, pool=pool, diversity=args.diversity, as_arrays=True), n_e2e)
        e2e_plain, plain = wall(lambda: model.recommend_batch(users, top_k=top_k, as_arrays=True), n_e2e)

    W = model.model.item_similarity.tocsc()
    W.sort_indices()
    sample = np.sort(rng.permutation(U)[:min(args.host_users, U)])
    h_ids, h_sc, h_cnt = (t[eng.be.to_dev(sample)].cpu().numpy() for t in (d_ids, d_sc, d_cnt))
    with step("host model", 1800):
        t0 = time.perf_counter()
        want = host_model_vectorised(W, h_ids, h_sc, h_cnt, top_k, lam)
        host_s = time.perf_counter() - t0
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    same = True
    for w, g in dev.items():
        same &= bool(np.array_equal(g[0][sample], want[0]) and np.array_equal(u32(g[1][sample]), u32(want[1]))
                     and np.array_equal(u32(g[2][sample]), u32(want[2])) and np.array_equal(g[3][sample], want[3]))
    live = want[0] >= 0
    same &= bool(np.array_equal(arrays[0][sample], np.where(live, np.take_along_axis(h_ids.astype(np.int64), np.maximum(want[0], 0).astype(np.int64), axis=1), -1))
                 and np.array_equal(arrays[2][sample], want[3]))
    changed = int((dev["1"][0] != np.arange(top_k)[None, :]).any(axis=1).sum())

    u0 = int(sample[0])
    rp = min(args.request_pool, I, 1024)
    rp_served = rp                       # the widest pool the fused top-k kernels serve for this model, for the end-to-end call
    while rp_served > top_k and not eng.topk_supported(rp_served, mode):
        rp_served -= 1
    with step("request", 600):
        # the kernel's input: `rp` seeded items scored for the user (score_pairs serves lists of up to 1024), best first
        d_u0 = eng.be.to_dev(np.array([u0], np.int32))
        c0 = eng.be.to_dev(rng.permutation(I)[:rp].astype(np.int32)[None, :])
        r_cnt = eng.be.to_dev(np.array([rp], np.int32))
        sc0 = eng.score_pairs_device(d_u0, 1, None, c0, r_cnt, 0)[0]
        by_score = torch.argsort(sc0, dim=1, descending=True, stable=True)
        r_ids, r_sc = torch.gather(c0, 1, by_score).contiguous(), torch.gather(sc0, 1, by_score).contiguous()
        req_kernel, _ = spans({str(w): (lambda w=w: eng.diversify_device(r_ids, r_sc, r_cnt, top_k, lam, waves_per_row=w)) for w in (1, 4)},
                              args.reps * 3)
        req_e2e, _ = wall(lambda: model.recommend_diverse(u0, top_k=top_k, pool=rp_served, diversity=args.diversity), args.reps * 3)
        req_plain, _ = wall(lambda: model.recommend(u0, top_k=top_k), args.reps * 3)

    med = lambda v: float(np.median(v)) if len(v) else None
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "w_nnz": int(W.nnz),
           "w_longest_column": int(np.diff(W.indptr).max()), "pool": int(pool), "top_k": int(top_k), "lambda": float(lam),
           "lists_whose_top_k_changed": changed, "warmup_calls": args.warmup, "timed_calls": args.reps,
           "timing": "device events around each call, one stream, the compared forms alternating; wall clock where it says so",
           "device_call_ms": kernel, "device_call_ms_median": {w: med(v) for w, v in kernel.items()},
           "device_call_ms_min_max": {w: [float(min(v)), float(max(v))] for w, v in kernel.items()},
           "lists_per_s": {w: U / (med(v) * 1e-3) for w, v in kernel.items()},
           "faster_waves_per_row": int(min(kernel, key=lambda w: med(kernel[w]))),
           "next_to_scoring_ms": beside, "next_to_scoring_ms_median": {k: med(v) for k, v in beside.items()},
           "e2e_ms": e2e, "e2e_ms_median": med(e2e), "recommend_batch_e2e_ms": e2e_plain, "recommend_batch_e2e_ms_median": med(e2e_plain),
           "host_model": {"sample_users": int(len(sample)), "sample_s": host_s, "all_users_s_extrapolated": host_s * U / len(sample),
                          "note": "the vectorised numpy host model on a SAMPLE of the users; the all-users figure is an EXTRAPOLATION"},
           "request": {"pool": int(rp), "pool_note": "seeded items scored with score_pairs, best first", "recommend_diverse_pool": int(rp_served),
                       "device_call_ms": req_kernel, "device_call_ms_median": {w: med(v) for w, v in req_kernel.items()},
                       "faster_waves_per_row": int(min(req_kernel, key=lambda w: med(req_kernel[w]))),
                       "recommend_diverse_ms": req_e2e, "recommend_diverse_p50_ms": med(req_e2e),
                       "recommend_ms": req_plain, "recommend_p50_ms": med(req_plain)},
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
