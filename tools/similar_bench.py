#!/usr/bin/env python3
"""What the hybrid's similar_items costs: csrc/factor_similar.hip, csrc/similar_blend.hip, SlimEngine.similar_hybrid_device and
SLIM.similar_items_hybrid_batch on a bench.py workload -- the item-to-item table: ALL items as queries against all items,
seeded normal vectors of `--dims` (12, 64) components, top_k in `--top-ks` (10, 100).

Timed with device events on the engine's stream, after `--warmup` untimed rounds (`--reps` timed ones; medians are reported
beside the raw spans).  Per (dim, top_k):

  kernel_ms                   HipBackend.factor_similar_topk (write_cosine) into buffers allocated before the loop
  torch_baseline_ms           torch.matmul -> the division by the item norms -> the diagonal set to -inf -> torch.topk -> the
                              division of the k kept scores by the query norm, in passes of one score block
                              (SlimEngine.RANKS_BLOCK_BYTES).  Same process, INTERLEAVED with the kernel round by round
  request_ms                  one query item, item_splits 0 (the library's choice: 64 chunks) against 1
  host                        the vectorised host model of tests/test_similar_host.py on a SAMPLE of `--host-queries` (200)
                              queries, which the device's lists must equal (ids, counts, score bits); the norms of ALL items
                              must equal the host model's bits

Then the model is fitted (bulk_fit, nn_feature_selection = the workload's K) and, for the first dim and every top_k (pool = top_k):

  chain_ms                    SlimEngine.similar_hybrid_device: factor_similar_topk -> similar_topk -> similar_blend, nothing
                              downloaded in between (device events)
  blend_ms                    the blend kernel alone on the chain's two lists (device events); its baseline is the vectorised
                              host model on the sample, the all-queries figure an EXTRAPOLATION and marked as one
  hybrid_e2e_ms               SLIM.similar_items_hybrid_batch(all items, as_arrays=True) end to end (wall clock)

Writes profiles/similar_<workload>.json with the build fingerprint.

    python tools/similar_bench.py --workload c3s

One process; every GPU step runs under its own time limit and nothing is started after a step that overran or failed."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


from factor_bench import StepTimeout, step         # one step under its own limit: overrunning it raises out of the step and ends the run


def dump(res, path):
    """The profile as JSON with one top-level key per line and one line per entry of a top-level list."""
    one = lambda v: json.dumps(v) if not isinstance(v, list) else "[\n" + ",\n".join("  " + json.dumps(x) for x in v) + "\n ]"
    open(path, "w").write("{\n" + ",\n".join(f" {json.dumps(k)}: {one(v)}" for k, v in res.items()) + "\n}\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--dims", default="12,64")
    ap.add_argument("--top-ks", default="10,100")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=200, help="queries the host models are run and compared on (a sample)")
    ap.add_argument("--no-fit", action="store_true", help="skip the fit and with it the chain, blend and end-to-end figures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"similar_{args.workload}.json")
    dims = [int(d) for d in args.dims.split(",")]
    top_ks = [int(k) for k in args.top_ks.split(",")]

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, build
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.synth import workload_matrix
    from tests.test_factor_host import bits
    from tests.test_similar_host import dbits, host_blend, host_norms_fast, host_similar_fast
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
    sample = np.sort(rng.permutation(I)[:min(args.host_queries, I)])
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

    block_rows = max(1, SlimEngine.RANKS_BLOCK_BYTES // (4 * I))
    d_q = be.to_dev(np.arange(I, dtype=np.int32))
    at = be.to_dev(sample.astype(np.int64))
    res = {"workload": f"{args.workload}: {wl['desc']}", "n_queries": int(I), "n_items": int(I), "warmup_rounds": args.warmup,
           "timed_rounds": args.reps, "torch_baseline_rows_per_pass": int(block_rows),
           "timing": "device events around each call, one stream, the compared forms alternating round by round; wall clock where it says so",
           "configs": [], "same_as_host_model": True, "build": build.fingerprint()}
    vectors = {}
    for dim in dims:
        Q = rng.standard_normal((I, dim)).astype(np.float32)
        vectors[dim] = Q
        eng.set_factors(np.zeros((1, dim), np.float32), Q)
        F = eng._F
        norms = eng.item_norms_device(0)
        with step(f"host model, dim {dim}", 900):
            t0 = time.perf_counter()
            h_norms = host_norms_fast(Q)
            want = host_similar_fast(Q, h_norms, sample, max(top_ks), write_cosine=True)
            host_model_s = time.perf_counter() - t0
        norms_same = bool(np.array_equal(norms.cpu().numpy().view(np.int32), h_norms.view(np.int32)))
        res["same_as_host_model"] &= norms_same
        for top_k in top_ks:
            ids = be.empty((I, top_k), torch.int32)
            sc = be.empty((I, top_k), torch.float32)
            cnt = be.zeros((I,), torch.int32)

            def kernel():
                be.factor_similar_topk(d_q, None, None, F["qt"], I, dim, norms, None, top_k, True, ids, sc, cnt)
                return ids, sc, cnt

            def baseline():
                out_i, out_s = [], []
                for lo in range(0, I, block_rows):
                    hi = min(I, lo + block_rows)
                    s = torch.matmul(F["qt"][:, lo:hi].t(), F["qt"])
                    s /= norms[None, :]
                    s[torch.arange(hi - lo, device=s.device), torch.arange(lo, hi, device=s.device)] = float("-inf")
                    v, i = torch.topk(s, top_k, dim=1)
                    out_i.append(i)
                    out_s.append(v / norms[lo:hi, None])
                return torch.cat(out_i), torch.cat(out_s)

            with step(f"dim {dim}, top_k {top_k}", 900):
                t, last = spans({"kernel": kernel, "torch_baseline": baseline}, args.reps)
                one = [int(sample[0])]
                req, _ = spans({"item_splits_0": lambda: eng.similar_factor_device(one, top_k, 0, item_splits=0),
                                "item_splits_1": lambda: eng.similar_factor_device(one, top_k, 0, item_splits=1)}, args.reps)
            g = tuple(x[at].cpu().numpy() for x in last["kernel"])
            same = bool(np.array_equal(g[0], want[0][:, :top_k]) and np.array_equal(bits(g[1]), bits(want[1][:, :top_k]))
                        and np.array_equal(g[2], np.minimum(want[2], top_k)))
            b_ids = last["torch_baseline"][0][at].cpu().numpy()
            res["same_as_host_model"] &= same
            flops = 2.0 * I * I * dim
            res["configs"].append({
                "dim": dim, "top_k": top_k, "same_as_host_model_on_the_sample": same, "norms_equal_the_host_model_bit_for_bit": norms_same,
                "torch_baseline_top_ids_equal_on_the_sample_rows": float((b_ids == want[0][:, :top_k]).all(axis=1).mean()),
                "kernel_ms": t["kernel"], "torch_baseline_ms": t["torch_baseline"],
                "median_ms": {k: med(v) for k, v in t.items()}, "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
                "tflops_kernel": flops / (med(t["kernel"]) * 1e-3) / 1e12, "tflops_torch_baseline": flops / (med(t["torch_baseline"]) * 1e-3) / 1e12,
                "kernel_over_torch_baseline": med(t["kernel"]) / med(t["torch_baseline"]),
                "request_one_query_ms_median": {k: med(v) for k, v in req.items()},
                "host": {"sample_queries": int(len(sample)), "host_model_sample_s": host_model_s}})
            print(json.dumps({k: v for k, v in res["configs"][-1].items() if not k.endswith("_ms") or k == "median_ms"}), flush=True)
            del ids, sc, cnt, last
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        dump(res, out_path)
    if args.no_fit:
        return 0 if res["same_as_host_model"] else 1

    # ---- the chain, the blend alone and the model's call end to end: dim = the first of --dims, pool = top_k
    dim = dims[0]
    coo = X.tocoo()
    model = SLIM(min_value=0, max_value=15, nn_feature_selection=wl["K"])
    with step("fit", 900), contextlib.redirect_stdout(io.StringIO()):
        model.add_interactions_columns(coo.row.astype(np.int64), coo.col.astype(np.int64),
                                       1.7e9 + np.arange(coo.nnz, dtype=np.float64), coo.data.astype(np.float64))
        model.bulk_fit(parallel=True, progress_bar=False)
        torch.cuda.synchronize()
    items = np.arange(I, dtype=np.int64)
    item_list = items.tolist()
    model.attach_factors([0], np.zeros((1, dim), np.float32), items.tolist(), vectors[dim])
    with step("warm-up", 300):
        model.similar_items_hybrid_batch(items[:16].tolist(), top_k=top_ks[0], as_arrays=True)
        torch.cuda.synchronize()
    meng = model.model.engine
    res["hybrid"] = []
    for top_k in top_ks:
        with step(f"chain, top_k {top_k}", 900):
            a_ids, a_sc, a_cnt, a_div = meng.similar_factor_device(items, top_k, 0, write_cosine=False, want_div=True)
            b_ids, b_sc, b_cnt = meng.similar_items_device(items, top_k)
            d_ex = meng._up(items.astype(np.int32))
            t, last = spans({"chain": lambda: meng.similar_hybrid_device(items, top_k, top_k, 0),
                             "blend": lambda: meng.similar_blend_device(a_ids, a_sc, a_cnt, a_div, b_ids, b_sc, b_cnt, d_ex, top_k)}, args.reps)
            n_e2e = max(3, args.reps // 3)
            e2e, _ = wall(lambda: model.similar_items_hybrid_batch(item_list, top_k=top_k, as_arrays=True), n_e2e)
        dl = lambda x: x[at].cpu().numpy()
        t0 = time.perf_counter()
        want = host_blend(I, (dl(a_ids), dl(a_sc), dl(a_cnt)), (dl(b_ids), dl(b_sc), dl(b_cnt)), top_k, a_div=dl(a_div),
                          exclude=sample.astype(np.int32))
        host_blend_s = time.perf_counter() - t0
        same = True
        for name in ("chain", "blend"):
            g = tuple(dl(x) for x in last[name])
            same &= bool(np.array_equal(g[0], want[0]) and np.array_equal(dbits(g[1]), dbits(want[1])) and np.array_equal(g[2], want[2])
                         and np.array_equal(g[3], want[3]))
        res["same_as_host_model"] &= same
        res["hybrid"].append({
            "dim": dim, "top_k": top_k, "pool": top_k, "same_as_host_model_on_the_sample": same,
            "chain_ms": t["chain"], "blend_ms": t["blend"], "median_ms": {k: med(v) for k, v in t.items()},
            "similar_items_hybrid_batch_ms": e2e, "similar_items_hybrid_batch_ms_median": med(e2e),
            "rows_with_an_item_in_both_lists_on_the_sample": float((want[2] == 3).any(axis=1).mean()),
            "host_blend": {"sample_queries": int(len(sample)), "host_model_sample_s": host_blend_s,
                           "host_model_all_queries_s_EXTRAPOLATED": host_blend_s * I / len(sample),
                           "note": "the vectorised host model on a SAMPLE of the queries; the all-queries figure is an EXTRAPOLATION"},
            "note": "chain and blend by device events; the end-to-end figure is wall clock with as_arrays=True"})
        print(json.dumps({k: v for k, v in res["hybrid"][-1].items() if not k.endswith("_ms")}), flush=True)
        dump(res, out_path)
    res["build_after_fit"] = build.fingerprint()
    dump(res, out_path)
    return 0 if res["same_as_host_model"] else 1


if __name__ == "__main__":
    try:
        sys.exit(main())
    except StepTimeout as e:            # an overrun is reported as one (124, timeout's status), so that a caller starts nothing after it
        print(f"[similar_bench] {e}", file=sys.stderr)
        sys.exit(124)
