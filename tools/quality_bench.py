#!/usr/bin/env python3
"""What measuring the lists costs: SLIM.recommend_quality / csrc/list_quality.hip on a bench.py workload, all users resident,
their top-`--top-k` (10) lists as the scoring kernels leave them and as the pool-`--pool` (50) diversify path leaves them at
lambda = 1 - `--diversity` (0.7).

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Timed with device events on the engine's stream,
after `--warmup` untimed calls each (`--reps` timed ones; medians are reported beside the raw spans):

  plain.device_call_ms        one eng.list_quality_device call over all users' top-k lists (its output allocations and the one
                              launch of list_quality_kernel, inputs and results in HBM) with the novelty table as the weight:
                              with `exposure` and one wave per row, the same with four waves, and one wave WITHOUT `exposure` (what
                              the atomics cost), ALTERNATING in one loop so that all see the same clocks and caches
  plain.next_to_scoring_ms    the top-k scoring step the kernel follows (eng.score_topk_device), alone and with the kernel behind it
  diverse.*                   the same after the diversify path (scoring a pool, the selection kernel, the gather)
  request                     one list of `--request-list` (500) seeded items: the device call with one and with four waves
  e2e_ms                      SLIM.recommend_quality(users) end to end (wall clock) at diversity 0 and at `--diversity`
  host_model_s                the vectorised numpy host model of tests/test_quality_host.py on a SAMPLE of `--host-users` (200)
                              users (wall clock), whose output the device's must equal (n, linked, sim_sum and weight_sum bits);
                              the all-users figure is an EXTRAPOLATION and marked as one

Only the position-owner mapping of csrc/list_quality.hip exists; no other mapping was built, so none is timed here.
Writes profiles/quality_<workload>.json with the build fingerprint.

    python tools/quality_bench.py --workload c3s

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
        print(f"[quality_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--pool", type=int, default=50)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--diversity", type=float, default=0.3, help="lambda = 1 - diversity (0.3: lambda 0.7)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-users", type=int, default=200, help="users the host model is run and compared on (a sample)")
    ap.add_argument("--request-list", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"quality_{args.workload}.json")

    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.synth import workload_matrix
    from rtrec_amd.utils.metrics import quality_summary
    from tests.test_quality_host import host_model_vectorised
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
    rng = np.random.default_rng(20251019)
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
        model.recommend_quality(users[:16], top_k=top_k, pool=pool, diversity=args.diversity)      # syncs W and X
        torch.cuda.synchronize()
    n_w = eng._whole_w("list_quality").n_items
    weight = eng.item_novelty_device()
    exposure = eng.be.zeros((n_w,), torch.int32)
    rows32 = users.astype(np.int32)
    d_rows = eng.be.to_dev(rows32)
    score = lambda k: eng.score_topk_device(None, U, k, True, mode, d_rows=d_rows)
    med = lambda v: float(np.median(v)) if len(v) else None
    W = model.model.item_similarity.tocsc()
    W.sort_indices()
    sample = np.sort(rng.permutation(U)[:min(args.host_users, U)])
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    h_weight = weight.cpu().numpy()
    same = True

    def measure(name, lists, make_lists):
        """The kernel on the device lists `lists` = (ids, counts), beside the step `make_lists` that produces them."""
        nonlocal same
        ids, cnt = lists[0].contiguous(), lists[1].contiguous()
        quality = lambda w, e: eng.list_quality_device(ids, cnt, weight, e, waves_per_row=w)
        with step(f"{name}: kernel", 600):
            kernel, last = spans({"exposure_1_wave": lambda: quality(1, exposure), "exposure_4_waves": lambda: quality(4, exposure),
                                  "no_exposure_1_wave": lambda: quality(1, None)}, args.reps)
            exposure.zero_()
            once = tuple(t.cpu().numpy() for t in quality(0, exposure))
            shown = exposure.cpu().numpy()
            dev = {k: tuple(t.cpu().numpy() for t in out) for k, out in last.items()}

        def made_and_measured():
            i, c = make_lists()
            return eng.list_quality_device(i.contiguous(), c.contiguous(), weight, exposure)

        with step(f"{name}: next to the step it follows", 600):
            beside, _ = spans({"lists": make_lists, "lists_plus_quality": made_and_measured}, args.reps)
        h_ids, h_cnt = (t[eng.be.to_dev(sample)].cpu().numpy() for t in (ids, cnt))
        with step(f"{name}: host model", 1800):
            t0 = time.perf_counter()
            want = host_model_vectorised(W, h_ids, h_cnt, h_weight)
            host_s = time.perf_counter() - t0
        for got in list(dev.values()) + [once]:
            same &= bool(np.array_equal(got[0][sample], want[0]) and np.array_equal(u32(got[1][sample]), u32(want[1]))
                         and np.array_equal(got[2][sample], want[2]) and np.array_equal(u32(got[3][sample]), u32(want[3])))
        same &= bool(int(shown.sum()) == int(once[0].sum()))
        summary = quality_summary(*once, shown)
        return {"device_call_ms": kernel, "device_call_ms_median": {k: med(v) for k, v in kernel.items()},
                "device_call_ms_min_max": {k: [float(min(v)), float(max(v))] for k, v in kernel.items()},
                "lists_per_s": {k: U / (med(v) * 1e-3) for k, v in kernel.items()},
                "next_to_lists_ms": beside, "next_to_lists_ms_median": {k: med(v) for k, v in beside.items()},
                "most_shown_item_count": int(shown.max()), "figures": summary,
                "host_model": {"sample_users": int(len(sample)), "sample_s": host_s, "all_users_s_extrapolated": host_s * U / len(sample),
                               "note": "the vectorised numpy host model on a SAMPLE of the users; the all-users figure is an EXTRAPOLATION"}}

    def top_lists():
        i, _, c = score(top_k)
        return i, c

    def diverse_lists():
        i, _, c, _, _ = model._diverse_device(rows32, top_k, pool, lam, True, mode)
        return i, c

    with step("lists", 300):
        plain_lists, div_lists = top_lists(), diverse_lists()
        torch.cuda.synchronize()
    plain = measure("plain", plain_lists, top_lists)
    diverse = measure("diverse", div_lists, diverse_lists)

    rl = min(args.request_list, I, 1024)
    with step("request", 600):
        r_ids = eng.be.to_dev(rng.permutation(I)[:rl].astype(np.int32)[None, :])
        r_cnt = eng.be.to_dev(np.array([rl], np.int32))
        req_kernel, req_last = spans({str(w): (lambda w=w: eng.list_quality_device(r_ids, r_cnt, weight, exposure, waves_per_row=w)) for w in (1, 4)},
                                     args.reps * 3)
        want = host_model_vectorised(W, r_ids.cpu().numpy(), r_cnt.cpu().numpy(), h_weight)
        for out in req_last.values():
            got = tuple(t.cpu().numpy() for t in out)
            same &= bool(np.array_equal(got[0], want[0]) and np.array_equal(u32(got[1]), u32(want[1])) and np.array_equal(got[2], want[2])
                         and np.array_equal(u32(got[3]), u32(want[3])))
    with step("recommend_quality", 900):
        n_e2e = max(3, args.reps // 3)
        e2e_plain, fig_plain = wall(lambda: model.recommend_quality(users, top_k=top_k), n_e2e)
        e2e_div, fig_div = wall(lambda: model.recommend_quality(users, top_k=top_k, pool=pool, diversity=args.diversity), n_e2e)
    same &= bool(fig_plain["intra_list_similarity"] == plain["figures"]["intra_list_similarity"] and fig_plain["gini"] == plain["figures"]["gini"]
                 and fig_div["intra_list_similarity"] == diverse["figures"]["intra_list_similarity"] and fig_div["gini"] == diverse["figures"]["gini"])

    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "w_nnz": int(W.nnz),
           "w_longest_column": int(np.diff(W.indptr).max()), "pool": int(pool), "top_k": int(top_k), "lambda": float(lam),
           "warmup_calls": args.warmup, "timed_calls": args.reps,
           "timing": "device events around each call, one stream, the compared forms alternating; wall clock where it says so",
           "mapping_variants": "none: only the position-owner form of csrc/list_quality.hip was built",
           "plain": plain, "diverse": diverse,
           "request": {"list": int(rl), "device_call_ms": req_kernel, "device_call_ms_median": {w: med(v) for w, v in req_kernel.items()},
                       "faster_waves_per_row": int(min(req_kernel, key=lambda w: med(req_kernel[w])))},
           "e2e_ms": {"diversity_0": e2e_plain, "diversity": e2e_div}, "e2e_ms_median": {"diversity_0": med(e2e_plain), "diversity": med(e2e_div)},
           "recommend_quality": {"diversity_0": fig_plain, "diversity": fig_div},
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
