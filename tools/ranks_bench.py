#!/usr/bin/env python3
"""What exact catalogue ranks cost: Recommender.evaluate_catalogue / csrc/catalogue_ranks.hip on a bench.py workload, all users
resident, `--held-out` (3) seeded held-out items per user.

The model is fitted once (bulk_fit, nn_feature_selection = the workload's K).  The engine works through the users in passes of
one dense score block (SlimEngine.RANKS_BLOCK_BYTES); ONE such pass is timed with device events on the engine's stream, after
`--warmup` untimed rounds (`--reps` timed ones; medians are reported beside the raw spans), the three steps ALTERNATING in one
loop so that all see the same clocks and caches:

  pass.fill_ms        the score_rows launch that fills the block (eng.be.score_rows, the plain layout)
  pass.ranks_ms       one eng.catalogue_ranks_device call on the block (its four output allocations and the one launch of
                      catalogue_ranks_kernel; block, targets and results in HBM), and the GB/s of the block that implies
  pass.launch_ms      the op alone into outputs allocated beforehand (eng.be.catalogue_ranks): the launch of the kernel without
                      the allocations, and its GB/s
  pass.copy_ms        a device-to-device copy of the same block (torch's copy_), and its GB/s counted the same way (the bytes
                      READ): the yardstick for a streaming read.  A later decision to fuse scoring and counting (a per-workgroup
                      accumulator instead of the dense block) rests on these two figures; the fused variant is not built
  e2e_ms              Recommender.evaluate_catalogue(frame) end to end (wall clock): frame handling, every pass, the summary
  host_model_s        the vectorised numpy host model of tests/test_ranks_host.py on a SAMPLE of `--host-users` (200) users of the
                      timed block (wall clock; the sample's score rows are downloaded for it), whose output the device's must
                      equal (above, tied, competing with ==, score by its bits); the all-users figure is an EXTRAPOLATION and
                      marked as one, and leaves out what downloading all the rows would cost
Writes profiles/ranks_<workload>.json with the build fingerprint.

    python tools/ranks_bench.py --workload c3s

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
import scipy.sparse as sp

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
        print(f"[ranks_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--held-out", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-users", type=int, default=200, help="users the host model is run and compared on (a sample)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"ranks_{args.workload}.json")

    import pandas as pd
    import torch
    from bench import WORKLOADS
    from rtrec_amd import SLIM, _native, build
    from rtrec_amd.recommender import Recommender
    from rtrec_amd.synth import workload_matrix
    from tests.test_ranks_host import bits64, host_model_vectorised
    wl = WORKLOADS[args.workload]
    X = workload_matrix(wl).tocsr()
    X.sort_indices()
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
    h = args.held_out
    held = rng.integers(0, I, (U, h)).astype(np.int64)
    frame = pd.DataFrame({"user": np.repeat(np.arange(U, dtype=np.int64), h), "item": held.ravel()})
    rec = Recommender(model)
    mode = _native.TOPK_SPARSE
    med = lambda v: float(np.median(v)) if len(v) else None

    with step("warm-up", 300):
        model.rank_items_batch([0, 1], [[0, 1], [2]])                      # syncs W and X
        torch.cuda.synchronize()
    W = eng._W
    f64 = bool(W["acc_f64"])
    n_items = eng._whole_w("catalogue_ranks").n_items
    itemsize = 8 if f64 else 4
    rows_pass = int(max(1, min(U, eng.RANKS_BLOCK_BYTES // (n_items * itemsize))))
    block_bytes = rows_pass * n_items * itemsize
    lay = eng._catalogue_layout()
    xb = eng._x_csr()
    rows = np.arange(rows_pass, dtype=np.int32)
    d_rows = eng.be.to_dev(rows)
    block = eng.be.zeros((rows_pass, n_items), torch.float64 if f64 else torch.float32)
    other = torch.empty_like(block)
    tg_ptr = np.arange(rows_pass + 1, dtype=np.int64) * h
    tg_items = held[:rows_pass].ravel().astype(np.int32)
    d_ptr, d_items = eng.be.to_dev(tg_ptr), eng.be.to_dev(tg_items)

    fill = lambda: eng.be.score_rows(rows_pass, d_rows, xb, W["n_items"], 0, lay, f64, block)
    ranks = lambda: eng.catalogue_ranks_device(block, d_rows, d_ptr, d_items, True, mode, xb)
    outs = (eng.be.empty((len(tg_items),), torch.int32), eng.be.empty((len(tg_items),), torch.int32),
            eng.be.empty((len(tg_items),), torch.float64), eng.be.empty((rows_pass,), torch.int32))
    launch = lambda: eng.be.catalogue_ranks(n_items, block, d_rows, xb, True, mode, d_ptr, d_items, *outs)
    copy = lambda: other.copy_(block)
    fns = {"fill": fill, "ranks": ranks, "launch": launch, "copy": copy}
    spans, last = {name: [] for name in fns}, {}
    with step("one pass: fill, ranks, copy", 600):
        for r in range(args.warmup + args.reps):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                last[name] = fn()
                b.record()
                b.synchronize()
                if r >= args.warmup:
                    spans[name].append(a.elapsed_time(b))
        got = tuple(t.cpu().numpy() for t in last["ranks"])
        bare = tuple(t.cpu().numpy() for t in outs)
    gbs = lambda ms: block_bytes / (ms * 1e-3) / 1e9

    sample = np.sort(rng.permutation(rows_pass)[:min(args.host_users, rows_pass)])
    with step("host model", 1800):
        S = block[eng.be.to_dev(sample.astype(np.int64))].cpu().numpy()
        rptr, rcol = xb[0].cpu().numpy(), xb[1].cpu().numpy()              # own is what the RESIDENT X stores
        Xh = sp.csr_matrix((np.ones(len(rcol), np.float32), rcol, rptr), shape=(len(rptr) - 1, max(I, int(rcol.max()) + 1 if len(rcol) else 0)))
        s_ptr = np.arange(len(sample) + 1, dtype=np.int64) * h
        s_items = held[sample].ravel().astype(np.int32)
        t0 = time.perf_counter()
        want = host_model_vectorised(S, n_items, sample, Xh, True, mode, s_ptr, s_items)
        host_s = time.perf_counter() - t0
    pick = (sample[:, None] * h + np.arange(h)[None, :]).ravel()
    same_launch = all(np.array_equal(bits64(a) if a.dtype == np.float64 else a, bits64(b) if b.dtype == np.float64 else b)
                      for a, b in zip(bare, got))
    same = bool(np.array_equal(got[0][pick], want[0]) and np.array_equal(got[1][pick], want[1])
                and np.array_equal(bits64(got[2][pick]), bits64(want[2])) and np.array_equal(got[3][sample], want[3]))

    with step("evaluate_catalogue", 1200):
        e2e, figures = [], None
        for r in range(1 + max(3, args.reps // 3)):                         # (one untimed call first)
            t0 = time.perf_counter()
            figures = rec.evaluate_catalogue(frame)
            torch.cuda.synchronize()
            if r >= 1:
                e2e.append((time.perf_counter() - t0) * 1e3)
    # the end-to-end call and the timed pass must tell the same story about the block's users
    ptr_all, a_all, t_all, s_all, c_all = model.rank_items_batch(np.arange(rows_pass), [row.tolist() for row in held[:rows_pass]], as_arrays=True)
    same &= bool(np.array_equal(a_all, got[0]) and np.array_equal(t_all, got[1]) and np.array_equal(c_all, got[3])) and bool(same_launch)

    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz),
           "held_out_per_user": int(h), "scores": "float64" if f64 else "float32", "mode": "SPARSE",
           "what_is_timed": "ONE instantiation of the kernel: this score type, SPARSE mode, the 4-target form (3 targets a row); no "
                            "float64 and no 8-target timing exists",
           "never_listed_share_of_the_timed_pass": float((got[0] == -1).mean()),
           "warmup_calls": args.warmup, "timed_calls": args.reps,
           "timing": "device events around each call, one stream, the three steps alternating; wall clock where it says so",
           "pass": {"rows": int(rows_pass), "block_bytes": int(block_bytes), "passes_for_all_users": int(-(-U // rows_pass)),
                    "fill_ms": spans["fill"], "ranks_ms": spans["ranks"], "launch_ms": spans["launch"], "copy_ms": spans["copy"],
                    "launch_ms_median": med(spans["launch"]), "launch_block_GBps": gbs(med(spans["launch"])),
                    "fill_ms_median": med(spans["fill"]), "ranks_ms_median": med(spans["ranks"]), "copy_ms_median": med(spans["copy"]),
                    "ranks_ms_min_max": [float(min(spans["ranks"])), float(max(spans["ranks"]))],
                    "ranks_block_GBps": gbs(med(spans["ranks"])), "copy_block_read_GBps": gbs(med(spans["copy"])),
                    "note": "GB/s = the block's bytes over the median time: what the rank kernel reads, and what the copy reads "
                            "(the copy also writes as much); ranks_ms = the engine call (four output allocations + the launch), "
                            "launch_ms = the op into outputs allocated beforehand"},
           "e2e_ms": e2e, "e2e_ms_median": med(e2e), "evaluate_catalogue": figures,
           "host_model": {"sample_users": int(len(sample)), "sample_s": host_s, "all_users_s_extrapolated": host_s * U / len(sample),
                          "note": "the vectorised numpy host model on a SAMPLE of the users, score rows already on the host; the "
                                  "all-users figure is an EXTRAPOLATION"},
           "fused_variant": "not built: scoring and counting are two launches over a dense block",
           "same_as_host_model": bool(same), "build": build.fingerprint()}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
