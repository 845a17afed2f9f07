#!/usr/bin/env python3
"""What blended lists cost: SLIM.recommend_blended_batch / csrc/blend.hip on a bench.py workload, all users resident, a seeded
list A of `--list-a` (10) items per user blended with B = SLIM's own top-`--top-k` (10) list.

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  Timed with device events on the engine's stream,
after `--warmup` untimed calls each (`--reps` timed ones; medians are reported beside the raw spans):

  device_call_ms[form]        one eng.blend_device call over all users' lists (its output allocations and the one launch of
                              blend_lists_kernel, inputs and results in HBM): "contacts_w1" / "contacts_w4" = the reference's
                              weighting with waves_per_row 1 and 4, "constant_w1" = a constant weight (no lookup), ALTERNATING in
                              one loop, so that all see the same clocks and caches
  next_to_scoring_ms          the top_k scoring step the kernel follows (eng.score_topk_device), alone and with the blend behind it
  e2e_ms                      SLIM.recommend_blended_batch(users, A as two arrays, as_arrays=True) end to end (wall clock), beside
                              recommend_batch(users, top_k, as_arrays=True)
  host_model                  the vectorised numpy host model of tests/test_blend_host.py on a SAMPLE of `--host-users` (200) users
                              (wall clock), whose output the device's must equal (ids, source, count, value bits); the all-users
                              figure is an EXTRAPOLATION and marked as one

Writes profiles/blend_<workload>.json with the build fingerprint.

    python tools/blend_bench.py --workload c3s

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
        print(f"[blend_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--list-a", type=int, default=10)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--k", type=float, default=2.0, help="similarity_weight_factor")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-users", type=int, default=200, help="users the host model is run and compared on (a sample)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"blend_{args.workload}.json")

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.synth import workload_matrix
    from tests.test_blend_host import host_model_vectorised, value_bits
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
    rng = np.random.default_rng(20261019)
    top_k, la = min(args.top_k, I), min(args.list_a, I)
    users = np.arange(U, dtype=np.int64)
    mode = _native.TOPK_SPARSE
    # list A: per user `la` seeded items (drawn with replacement across the catalogue: a few repeat), scores descending.  No count
    # CSR: the contacts form looks every item of B up in the user's row of X, as the reference does without repeated contacts
    a_ids = rng.integers(0, I, (U, la)).astype(np.int32)
    a_sc = -np.sort(-rng.random((U, la)).astype(np.float32), axis=1)
    a_cnt = np.full(U, la, np.int32)

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
        model.recommend_blended_batch(users[:16], a_ids[:16].astype(np.int64), a_sc[:16], top_k=top_k, as_arrays=True)   # syncs W and X
        torch.cuda.synchronize()
    d_rows = eng.be.to_dev(users.astype(np.int32))
    score = lambda: eng.score_topk_device(None, U, top_k, True, mode, d_rows=d_rows)
    with step("lists", 300):
        b_ids, b_sc, b_cnt = score()
        b_ids, b_sc, b_cnt = b_ids.contiguous(), b_sc.to(torch.float32).contiguous(), b_cnt.contiguous()
        d_a = tuple(eng.be.to_dev(a) for a in (a_ids, a_sc, a_cnt))
        torch.cuda.synchronize()
    keep = min(top_k, la + top_k)
    blend = lambda waves, contacts, b=None: eng.blend_device(*d_a, *(b or (b_ids, b_sc, b_cnt)), keep, 1.0, contacts, args.k, False,
                                                              d_rows=d_rows, waves_per_row=waves)
    with step("kernel", 600):
        kernel, last = spans({"contacts_w1": lambda: blend(1, True), "contacts_w4": lambda: blend(4, True),
                              "constant_w1": lambda: blend(1, False)}, args.reps)
        dev = {name: tuple(t.cpu().numpy() for t in out) for name, out in last.items()}

    def scored_and_blended():
        i, s, c = score()
        return blend(0, True, (i, s.to(torch.float32), c))

    with step("next to the scoring step", 600):
        beside, _ = spans({"scoring": score, "scoring_plus_blend": scored_and_blended}, args.reps)
    with step("recommend_blended_batch", 900):
        n_e2e = max(3, args.reps // 3)
        a64 = a_ids.astype(np.int64)
        e2e, arrays = wall(lambda: model.recommend_blended_batch(users, a64, a_sc, top_k=top_k, similarity_weight_factor=args.k, as_arrays=True), n_e2e)
        e2e_plain, _ = wall(lambda: model.recommend_batch(users, top_k=top_k, as_arrays=True), n_e2e)

    sample = np.sort(rng.permutation(U)[:min(args.host_users, U)])
    h_b = tuple(t[eng.be.to_dev(sample)].cpu().numpy() for t in (b_ids, b_sc, b_cnt))
    h_a = (a_ids[sample], a_sc[sample], a_cnt[sample])
    Xr = sp.csr_matrix(X)
    Xr.sort_indices()
    con = dict(X=Xr[sample], C=None, rows=None)
    with step("host model", 1800):
        t0 = time.perf_counter()
        want = host_model_vectorised(I, h_a, h_b, keep, contacts=con, k=args.k)
        host_s = time.perf_counter() - t0
        want_const = host_model_vectorised(I, h_a, h_b, keep, weight_b=1.0)
    same = True
    for name, g in dev.items():
        w = want_const if name.startswith("constant") else want
        same &= bool(np.array_equal(g[0][sample], w[0]) and np.array_equal(value_bits(g[1][sample]), value_bits(w[1]))
                     and np.array_equal(g[2][sample], w[2]) and np.array_equal(g[3][sample], w[3]))
    same &= bool(np.array_equal(arrays[0][sample], want[0].astype(np.int64)) and np.array_equal(arrays[3][sample], want[3]))
    src = dev["constant_w1"][2]
    med = lambda v: float(np.median(v)) if len(v) else None
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "list_a": int(la),
           "list_b_top_k": int(top_k), "keep": int(keep), "similarity_weight_factor": args.k,
           "constant_weight_lists_showing_an_item_only_b_holds": int((src == 2).any(axis=1).sum()),
           "constant_weight_lists_showing_an_item_of_both": int((src == 3).any(axis=1).sum()),
           "warmup_calls": args.warmup, "timed_calls": args.reps,
           "timing": "device events around each call, one stream, the compared forms alternating; wall clock where it says so",
           "device_call_ms": kernel, "device_call_ms_median": {w: med(v) for w, v in kernel.items()},
           "device_call_ms_min_max": {w: [float(min(v)), float(max(v))] for w, v in kernel.items()},
           "lists_per_s": {w: U / (med(v) * 1e-3) for w, v in kernel.items()},
           "next_to_scoring_ms": beside, "next_to_scoring_ms_median": {k: med(v) for k, v in beside.items()},
           "e2e_ms": e2e, "e2e_ms_median": med(e2e), "recommend_batch_e2e_ms": e2e_plain, "recommend_batch_e2e_ms_median": med(e2e_plain),
           "e2e_note": "list A is handed over as two [B, K] integer arrays (the vectorised id check); lists of Python lists cost a loop per item",
           "host_model": {"sample_users": int(len(sample)), "sample_s": host_s, "all_users_s_extrapolated": host_s * U / len(sample),
                          "note": "the vectorised numpy host model on a SAMPLE of the users; the all-users figure is an EXTRAPOLATION"},
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("device_call_ms", "next_to_scoring_ms", "build")}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
