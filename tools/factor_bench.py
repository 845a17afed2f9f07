#!/usr/bin/env python3
"""What the factor scorer costs: csrc/factor_topk.hip / SlimEngine.factor_topk_device / SLIM.recommend_hybrid_batch on a bench.py
workload, all users resident, seeded normal vectors of `--dims` (12, 64) components, top_k in `--top-ks` (10, 100),
filter_interacted=True.

Timed with device events on the engine's stream, after `--warmup` untimed rounds (`--reps` timed ones; medians are reported
beside the raw spans).  Per (dim, top_k):

  kernel_ms                   HipBackend.factor_topk into buffers allocated before the loop: the launches alone
  device_call_ms              eng.factor_topk_device: the same plus its output allocations
  torch_baseline_ms           torch.matmul -> the interacted entries set to -inf -> torch.topk, in passes of one score block
                              (SlimEngine.RANKS_BLOCK_BYTES); the index tensors of the filter are built before the loop.  Same
                              process, INTERLEAVED with the two above round by round
  tflops                      2 * users * items * dim / kernel time, beside the 122 TF an untuned f32-MFMA GEMM of 4096^3 is
                              reported at: a reference point, not a target (this kernel also selects)
  request_ms                  one user, item_splits 0 (the library's choice: 64 chunks) against 1
  host                        numpy P @ Q.T + argpartition on a SAMPLE of `--host-users` (200) users (wall clock; the all-users
                              figure is an EXTRAPOLATION and marked as one), and the host model of tests/test_factor_host.py on the
                              same sample, which the device's lists must equal (ids, counts, score bits)

Then the model is fitted (bulk_fit, nn_feature_selection = the workload's K) and, for dim 12 and top_k 10:

  hybrid_e2e_ms               SLIM.recommend_hybrid_batch(users, as_arrays=True) end to end (wall clock), beside
                              recommend_blended_batch fed the same factor lists from the host, and recommend_batch

Writes profiles/factor_<workload>.json with the build fingerprint (once before the fit, once after).

    python tools/factor_bench.py --workload c3s

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
        print(f"[factor_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--dims", default="12,64")
    ap.add_argument("--top-ks", default="10,100")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-users", type=int, default=200, help="users the host model is run and compared on (a sample)")
    ap.add_argument("--no-fit", action="store_true", help="skip the fit and the hybrid end-to-end figures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"factor_{args.workload}.json")
    dims = [int(d) for d in args.dims.split(",")]
    top_ks = [int(k) for k in args.top_ks.split(",")]

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, build
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.synth import workload_matrix
    from tests.test_factor_host import bits, host_model_fast
    wl = WORKLOADS[args.workload]
    X = sp.csr_matrix(workload_matrix(wl))
    X.sort_indices()
    U, I = X.shape
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(None, X, need_csc=False)
    be = eng.be
    rng = np.random.default_rng(20261019)
    sample = np.sort(rng.permutation(U)[:min(args.host_users, U)])
    med = lambda v: float(np.median(v)) if len(v) else None

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

    # the torch baseline's passes: rows per score block, and the (row in block, column) indices of the interacted entries
    block_rows = max(1, SlimEngine.RANKS_BLOCK_BYTES // (4 * I))
    passes = []
    for lo in range(0, U, block_rows):
        hi = min(U, lo + block_rows)
        sub = X[lo:hi].tocoo()
        passes.append((lo, hi, be.to_dev(sub.row.astype(np.int64)), be.to_dev(sub.col.astype(np.int64))))
    d_rows = be.to_dev(np.arange(U, dtype=np.int32))
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "filter_interacted": True,
           "warmup_rounds": args.warmup, "timed_rounds": args.reps, "torch_baseline_rows_per_pass": int(block_rows),
           "timing": "device events around each call, one stream, the compared forms alternating round by round; wall clock where it says so",
           "mfma_gemm_reference_tflops": 122.0, "configs": [], "same_as_host_model": True, "build": build.fingerprint()}
    for dim in dims:
        P = rng.standard_normal((U, dim)).astype(np.float32)
        Q = rng.standard_normal((I, dim)).astype(np.float32)
        eng.set_factors(P, Q)
        F = eng._F
        with step(f"host model, dim {dim}", 900):
            t0 = time.perf_counter()
            want = host_model_fast(P[sample], Q, max(top_ks), X=X[sample], filter_interacted=True)
            host_model_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            S = P[sample] @ Q.T
            for a in range(len(sample)):
                S[a, X.indices[X.indptr[sample[a]]:X.indptr[sample[a] + 1]]] = -np.inf
            part = np.argpartition(-S, min(top_ks) - 1, axis=1)[:, :min(top_ks)]
            numpy_s = time.perf_counter() - t0
            del S, part
        for top_k in top_ks:
            ids = be.empty((U, top_k), torch.int32)
            sc = be.empty((U, top_k), torch.float32)
            cnt = be.zeros((U,), torch.int32)

            def kernel():
                be.factor_topk(d_rows, None, U, F["p"], F["qt"], I, dim, None, eng._x_csr(), True, top_k, ids, sc, cnt)
                return ids, sc, cnt

            def baseline():
                out_i, out_s = [], []
                for lo, hi, r_, c_ in passes:
                    s = torch.matmul(F["p"][lo:hi], F["qt"])
                    s[r_, c_] = float("-inf")
                    v, i = torch.topk(s, top_k, dim=1)
                    out_i.append(i)
                    out_s.append(v)
                return torch.cat(out_i), torch.cat(out_s)

            with step(f"dim {dim}, top_k {top_k}", 900):
                t, last = spans({"kernel": kernel, "device_call": lambda: eng.factor_topk_device(d_rows, U, top_k, True),
                                 "torch_baseline": baseline}, args.reps)
                one = be.to_dev(np.array([int(sample[0])], np.int32))
                req, _ = spans({"item_splits_0": lambda: eng.factor_topk_device(one, 1, top_k, True, item_splits=0),
                                "item_splits_1": lambda: eng.factor_topk_device(one, 1, top_k, True, item_splits=1)}, args.reps)
            at = be.to_dev(sample.astype(np.int64))
            same = True
            for name in ("kernel", "device_call"):
                g = tuple(x[at].cpu().numpy() for x in last[name])
                same &= bool(np.array_equal(g[0], want[0][:, :top_k]) and np.array_equal(bits(g[1]), bits(want[1][:, :top_k]))
                             and np.array_equal(g[2], np.minimum(want[2], top_k)))
            b_ids = last["torch_baseline"][0][at].cpu().numpy()
            res["same_as_host_model"] &= same
            flops = 2.0 * U * I * dim
            res["configs"].append({
                "dim": dim, "top_k": top_k, "same_as_host_model_on_the_sample": same,
                "torch_baseline_top_ids_equal_on_the_sample_rows": float((b_ids == want[0][:, :top_k]).all(axis=1).mean()),
                "kernel_ms": t["kernel"], "device_call_ms": t["device_call"], "torch_baseline_ms": t["torch_baseline"],
                "median_ms": {k: med(v) for k, v in t.items()}, "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
                "tflops_kernel": flops / (med(t["kernel"]) * 1e-3) / 1e12, "tflops_torch_baseline": flops / (med(t["torch_baseline"]) * 1e-3) / 1e12,
                "kernel_over_torch_baseline": med(t["kernel"]) / med(t["torch_baseline"]),
                "request_one_user_ms_median": {k: med(v) for k, v in req.items()},
                "host": {"sample_users": int(len(sample)), "numpy_matmul_argpartition_sample_s": numpy_s,
                         "numpy_all_users_s_extrapolated": numpy_s * U / len(sample), "host_model_sample_s": host_model_s,
                         "note": "numpy on a SAMPLE of the users at the smallest top_k; the all-users figure is an EXTRAPOLATION"}})
            print(json.dumps({k: v for k, v in res["configs"][-1].items() if not k.endswith("_ms") or k == "median_ms"}), flush=True)
            del ids, sc, cnt, last
        json.dump(res, open(out_path, "w"), indent=1)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    if args.no_fit:
        return 0 if res["same_as_host_model"] else 1

    # ---- end to end: the hybrid call of the model, dim = the first of --dims, top_k = the first of --top-ks
    dim, top_k = dims[0], top_ks[0]
    coo = X.tocoo()
    model = SLIM(min_value=0, max_value=15, nn_feature_selection=wl["K"])
    with step("fit", 900), contextlib.redirect_stdout(io.StringIO()):
        model.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64),
                                       1.7e9 + np.arange(coo.nnz, dtype=np.float64), coo.data.astype(np.float64))
        model.bulk_fit(parallel=True, progress_bar=False)
        torch.cuda.synchronize()
    users = np.arange(U, dtype=np.int64)
    P = rng.standard_normal((U, dim)).astype(np.float32)
    Q = rng.standard_normal((I, dim)).astype(np.float32)
    model.attach_factors(users.tolist(), P, np.arange(I).tolist(), Q)
    with step("warm-up", 300):
        model.recommend_hybrid_batch(users[:16], top_k=top_k, as_arrays=True)
        torch.cuda.synchronize()
    with step("recommend_hybrid_batch", 900):
        n_e2e = max(3, args.reps // 3)
        e2e, _ = wall(lambda: model.recommend_hybrid_batch(users, top_k=top_k, as_arrays=True), n_e2e)
        f_ids, f_sc, _ = model.recommend_factor_batch(users, top_k=top_k, as_arrays=True)
        e2e_brought, _ = wall(lambda: model.recommend_blended_batch(users, f_ids, f_sc, top_k=top_k, as_arrays=True), n_e2e)
        e2e_plain, _ = wall(lambda: model.recommend_batch(users, top_k=top_k, as_arrays=True), n_e2e)
    res["hybrid_e2e"] = {"dim": dim, "top_k": top_k, "recommend_hybrid_batch_ms": e2e, "recommend_hybrid_batch_ms_median": med(e2e),
                         "recommend_blended_batch_fed_the_same_lists_ms": e2e_brought,
                         "recommend_blended_batch_fed_the_same_lists_ms_median": med(e2e_brought),
                         "recommend_batch_ms": e2e_plain, "recommend_batch_ms_median": med(e2e_plain),
                         "note": "wall clock, as_arrays=True; the brought lists are two [B, K] integer arrays already in host memory, "
                                 "so what computed them is NOT in that figure"}
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res["hybrid_e2e"]))
    return 0 if res["same_as_host_model"] else 1


if __name__ == "__main__":
    try:
        sys.exit(main())
    except StepTimeout as e:            # an overrun is reported as one (124, timeout's status), so that a caller starts nothing after it
        print(f"[factor_bench] {e}", file=sys.stderr)
        sys.exit(124)
