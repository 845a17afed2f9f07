#!/usr/bin/env python3
"""What training the factor scorer costs: csrc/factor_gram.hip, csrc/factor_als.hip / SlimEngine.als_half_step / fit_factors on a
bench.py workload, X resident in both orientations, `--dims` (32, 64) components, regularization 0.01, alpha 1.

Timed with device events on the engine's stream, after `--warmup` untimed rounds (`--reps` timed ones; medians are reported
beside the raw spans).  Per dim:

  gram_ms                     HipBackend.factor_gram of the item vectors and of the user vectors: both launches of the one export
  user_half_step_ms           eng.als_half_step("user"): the Gram of the item vectors, then every row of X, the longest first
  item_half_step_ms           eng.als_half_step("item"): the Gram of the user vectors, then every column of X
                              (a round runs the user half-step, then the item half-step: the state moves on as in a fit)
  fit_factors_wall_s          one eng.fit_factors(iterations=15) end to end by wall clock, the upload of the seeded item vectors
                              and the install (transpose, norms) included
  status                      the status counts of the last half-step of each side
  mfma_lower_bound_ms         COMPUTED, not measured: sum over the rows of ceil(n_r / 2) * tiles * 64 cycles (n_r = the row's usable
                              entries; tiles = 1 up to dim 32, 3 up to 64), spread over the device's SIMDs at its clock: the time
                              the matrix cores need for the build alone if every SIMD were busy all the time
  host                        the vectorised host model of tests/test_als_host.py on a SAMPLE of `--host-rows` (200) rows per side
                              (wall clock; the all-rows figure is an EXTRAPOLATION and marked as one), which the device's rows
                              must equal bit for bit, status included

There is no other GPU implementation to compare with on this machine; nothing here is a speed-up claim.
Writes profiles/als_<workload>.json with the build fingerprint.

    python tools/als_bench.py --workload c3s

`--solver cg` measures the conjugate-gradient path instead (csrc/factor_als_cg.hip, the wide Gram kernel above 64 components) at
`--dims` (32, 64, 128, 256; `--dim` names one) with `--cg-steps` (3) steps, and writes profiles/als_cg_<workload>.json: the same
figures, the Cholesky half-steps interleaved round by round in the same process up to 64 components, fit_factors end to end for
both solvers with the float64 loss of both results, and the sampled rows of the first two half-steps against the host model
of tests/test_als_cg_host.py bit for bit (above 64 components the host model takes the device's Gram matrix, which
tests/test_gpu_als_cg.py compares on its own).

    python tools/als_bench.py --workload c3s --solver cg

One process; every GPU step runs under its own time limit and nothing is started after a step that overran or failed."""
import argparse
import contextlib
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
        print(f"[als_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--dims", default=None, help="comma-separated; default 32,64 (32,64,128,256 with --solver cg)")
    ap.add_argument("--dim", type=int, default=None, help="one dim instead of --dims")
    ap.add_argument("--solver", default="cholesky", choices=("cholesky", "cg"))
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=15)
    ap.add_argument("--host-rows", type=int, default=200, help="rows per side the host model is run and compared on (a sample)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="engine clock the computed bound assumes (the MI355X's peak, from its data sheet)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.solver == "cg":
        return main_cg(args)
    out_path = args.out or os.path.join(ROOT, "profiles", f"als_{args.workload}.json")
    dims = [args.dim] if args.dim else [int(d) for d in (args.dims or "32,64").split(",")]
    reg, alpha, seed = 0.01, 1.0, 0

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import build
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.synth import workload_matrix
    from tests.test_als_host import bits, gram_fast, solve_fast
    wl = WORKLOADS[args.workload]
    X = sp.csr_matrix(workload_matrix(wl), dtype=np.float32)
    X.sort_indices()
    Xt = sp.csr_matrix(X.T.tocsr(), dtype=np.float32)
    Xt.sort_indices()
    U, I = X.shape
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(X.tocsc(), X, need_csc=True)
    be = eng.be
    prop = torch.cuda.get_device_properties(0)
    simds = int(prop.multi_processor_count) * 4
    clock_hz = args.clock_ghz * 1e9
    rng = np.random.default_rng(20261020)
    samples = {"user": np.sort(rng.permutation(U)[:min(args.host_rows, U)]), "item": np.sort(rng.permutation(I)[:min(args.host_rows, I)])}
    sides = {"user": X, "item": Xt}
    med = lambda v: float(np.median(v)) if len(v) else None

    def event_span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz),
           "regularization": reg, "alpha": alpha, "seed": seed, "warmup_rounds": args.warmup, "timed_rounds": args.reps,
           "timing": "device events around each call, one stream; a round is the user half-step, then the item half-step; wall clock where it says so",
           "device": {"name": prop.name, "compute_units": int(prop.multi_processor_count), "simds": simds, "clock_hz_ASSUMED": clock_hz},
           "configs": [], "same_as_host_model": True, "build": build.fingerprint()}
    for dim in dims:
        tiles = 1 if dim <= 32 else 3
        Q0 = np.random.default_rng(seed).standard_normal((I, dim)).astype(np.float32) * np.float32(0.01)
        eng.als_begin(dim, reg, alpha, Q0)
        T = eng._als
        cfg = {"dim": dim, "tiles": tiles, "host": {}, "mfma_lower_bound_ms_COMPUTED": {}, "same_as_host_model_on_the_sample": {}}
        # ---- the in-run check: the first user half-step and the first item half-step against the host model on a sample
        for side in ("user", "item"):
            R, rows = sides[side], samples[side]
            with step(f"dim {dim}: {side} half-step and host model", 900):
                fixed = (T["Q"] if side == "user" else T["P"]).cpu().numpy()
                eng.als_half_step(side)
                torch.cuda.synchronize()
                got = (T["P"] if side == "user" else T["Q"]).cpu().numpy()[rows]
                got_status = T["status"][side].cpu().numpy()[rows]
                t0 = time.perf_counter()
                want = np.zeros((R.shape[0], dim), np.float32)
                want_status = solve_fast(R.indptr, R.indices, R.data, fixed, gram_fast(fixed, reg), alpha, want, rows)
                host_s = time.perf_counter() - t0
            same = bool(np.array_equal(got_status, want_status) and np.array_equal(bits(got), bits(want[rows])))
            res["same_as_host_model"] &= same
            cfg["same_as_host_model_on_the_sample"][side] = same
            cfg["host"][side] = {"sample_rows": int(len(rows)), "host_model_sample_s": host_s,
                                 "host_model_all_rows_s_EXTRAPOLATED": host_s * R.shape[0] / len(rows),
                                 "note": "the vectorised host model on a SAMPLE of the rows, its Gram matrix included; the all-rows "
                                         "figure is an EXTRAPOLATION"}
            usable = np.bincount(np.repeat(np.arange(R.shape[0]), np.diff(R.indptr)), weights=(alpha * R.data > 0),
                                 minlength=R.shape[0]).astype(np.int64)
            cycles = float((((usable + 1) // 2) * tiles * 64).sum())
            cfg["mfma_lower_bound_ms_COMPUTED"][side] = cycles / simds / clock_hz * 1e3
        # ---- timings
        gram = be.empty((dim, dim), torch.float32)
        t = {"gram_items": [], "gram_users": [], "user_half_step": [], "item_half_step": []}
        counts = {}
        with step(f"dim {dim}: timed rounds", 900):
            for r in range(args.warmup + args.reps):
                spans = {"gram_items": event_span(lambda: be.factor_gram(T["Q"], I, dim, reg, gram))[0],
                         "gram_users": event_span(lambda: be.factor_gram(T["P"], U, dim, reg, gram))[0]}
                spans["user_half_step"], counts["user"] = event_span(lambda: eng.als_half_step("user"))
                spans["item_half_step"], counts["item"] = event_span(lambda: eng.als_half_step("item"))
                if r >= args.warmup:
                    for k, v in spans.items():
                        t[k].append(v)
        with step(f"dim {dim}: fit_factors({args.iterations})", 900):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit_counts = eng.fit_factors(dim=dim, iterations=args.iterations, regularization=reg, alpha=alpha, seed=seed)
            torch.cuda.synchronize()
            fit_s = time.perf_counter() - t0
        cfg.update({"ms": t, "median_ms": {k: med(v) for k, v in t.items()},
                    "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
                    "status_of_the_last_timed_half_steps": {s: {str(k): v for k, v in c.items()} for s, c in counts.items()},
                    "fit_factors_iterations": args.iterations, "fit_factors_wall_s": fit_s,
                    "fit_factors_status": {s: {str(k): v for k, v in c.items()} for s, c in fit_counts.items()}})
        res["configs"].append(cfg)
        print(json.dumps({k: v for k, v in cfg.items() if k != "ms"}), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["same_as_host_model"] else 1


def implicit_loss(torch, X, P, Q, reg, alpha):
    """sum over ALL pairs of c (p - x . y)^2 + reg (|P|^2 + |Q|^2) in float64 on the device, c = 1 + alpha r and p = 1 on the stored
    positive entries, c = 1 and p = 0 elsewhere: the all-pairs part through the Gram matrix, sum_u x^T (Q^T Q) x, and the stored
    entries' correction c (1 - s)^2 - s^2 in chunks."""
    P, Q = torch.as_tensor(P, device="cuda").double(), torch.as_tensor(Q, device="cuda").double()
    total = float(((P @ (Q.T @ Q)) * P).sum()) + reg * float((P * P).sum() + (Q * Q).sum())
    coo = X.tocoo()
    keep = alpha * coo.data > 0
    rows, cols, vals = (torch.as_tensor(a[keep], device="cuda") for a in (coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float64)))
    for a in range(0, int(rows.numel()), 1 << 20):
        r, c, v = rows[a:a + (1 << 20)], cols[a:a + (1 << 20)], vals[a:a + (1 << 20)]
        sc = (P[r] * Q[c]).sum(dim=1)
        total += float(((1.0 + alpha * v) * (1.0 - sc) ** 2 - sc ** 2).sum())
    return total


def main_cg(args) -> int:
    out_path = args.out or os.path.join(ROOT, "profiles", f"als_cg_{args.workload}.json")
    dims = [args.dim] if args.dim else [int(d) for d in (args.dims or "32,64,128,256").split(",")]
    reg, alpha, seed, steps = 0.01, 1.0, 0, args.cg_steps

    import scipy.sparse as sp
    import torch
    from bench import WORKLOADS
    from rtrec_amd import build
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.synth import workload_matrix
    from tests.test_als_host import bits, gram_fast
    import tests.test_als_cg_host as cg_host
    from tests.test_als_cg_host import cg_fast
    cg_host.GROUP_ELEMENTS = 1 << 25            # (larger groups of jobs per vectorised step: fewer, larger numpy calls)
    wl = WORKLOADS[args.workload]
    X = sp.csr_matrix(workload_matrix(wl), dtype=np.float32)
    X.sort_indices()
    Xt = sp.csr_matrix(X.T.tocsr(), dtype=np.float32)
    Xt.sort_indices()
    U, I = X.shape
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    eng = SlimEngine(device="cuda:0")
    eng.set_interactions(X.tocsc(), X, need_csc=True)
    be = eng.be
    prop = torch.cuda.get_device_properties(0)
    rng = np.random.default_rng(20261020)
    samples = {"user": np.sort(rng.permutation(U)[:min(args.host_rows, U)]), "item": np.sort(rng.permutation(I)[:min(args.host_rows, I)])}
    sides = {"user": X, "item": Xt}
    med = lambda v: float(np.median(v)) if len(v) else None

    def event_span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def gram_call(dim):
        return be.factor_gram if dim <= SlimEngine.ALS_MAX_DIM else be.factor_gram_wide

    res = {"workload": f"{args.workload}: {wl['desc']}", "n_users": int(U), "n_items": int(I), "nnz": int(X.nnz), "solver": "cg",
           "cg_steps": steps, "regularization": reg, "alpha": alpha, "seed": seed, "warmup_rounds": args.warmup, "timed_rounds": args.reps,
           "timing": "device events around each call, one stream; a round is the CG user half-step, the CG item half-step and, up to 64 "
                     "components, the Cholesky user and item half-steps on a state of their own; wall clock where it says so",
           "device": {"name": prop.name, "compute_units": int(prop.multi_processor_count)},
           "configs": [], "same_as_host_model": True, "build": build.fingerprint()}
    for dim in dims:
        with_cholesky = dim <= SlimEngine.ALS_MAX_DIM
        Q0 = np.random.default_rng(seed).standard_normal((I, dim)).astype(np.float32) * np.float32(0.01)
        eng.als_begin(dim, reg, alpha, Q0, solver="cg", cg_steps=steps)
        T = eng._als
        cfg = {"dim": dim, "waves_per_job": 1 if dim <= 64 else 2 if dim <= 128 else 4, "host": {}, "same_as_host_model_on_the_sample": {}}
        # ---- the in-run check: the first user half-step (from zero) and the first item half-step (from the seeded vectors)
        for side in ("user", "item"):
            R, rows = sides[side], samples[side]
            with step(f"dim {dim}: {side} half-step and host model", 900):
                fixed = (T["Q"] if side == "user" else T["P"]).cpu().numpy()
                want = (T["P"] if side == "user" else T["Q"]).cpu().numpy().copy()
                want = np.concatenate([want, np.zeros((R.shape[0] - len(want), dim), np.float32)]) if len(want) < R.shape[0] else want
                eng.als_half_step(side)
                torch.cuda.synchronize()
                got = (T["P"] if side == "user" else T["Q"]).cpu().numpy()[rows]
                got_status = T["status"][side].cpu().numpy()[rows]
                t0 = time.perf_counter()
                if with_cholesky:
                    G = gram_fast(fixed, reg)
                else:
                    g = be.empty((dim, dim), torch.float32)
                    gram_call(dim)(be.to_dev(fixed), len(fixed), dim, reg, g)
                    G = g.cpu().numpy()
                want_status, _ = cg_fast(R.indptr, R.indices, R.data, fixed, G, alpha, want, rows, steps, True)
                host_s = time.perf_counter() - t0
            same = bool(np.array_equal(got_status, want_status) and np.array_equal(bits(got), bits(want[rows])))
            res["same_as_host_model"] &= same
            cfg["same_as_host_model_on_the_sample"][side] = same
            cfg["host"][side] = {"sample_rows": int(len(rows)), "host_model_sample_s": host_s,
                                 "gram": "host model" if with_cholesky else "the device's (compared bit for bit in tests/test_gpu_als_cg.py)"}
        # ---- timings
        T_cg = T
        T_ch = None
        if with_cholesky:
            eng.als_begin(dim, reg, alpha, Q0)
            T_ch = eng._als
            eng.als_half_step("user")
            eng.als_half_step("item")
        gram = be.empty((dim, dim), torch.float32)
        names = ["gram_items", "gram_users", "cg_user_half_step", "cg_item_half_step"] + (["cholesky_user_half_step", "cholesky_item_half_step"] if with_cholesky else [])
        t = {k: [] for k in names}
        counts = {}
        with step(f"dim {dim}: timed rounds", 900):
            for r in range(args.warmup + args.reps):
                eng._als = T_cg
                spans = {"gram_items": event_span(lambda: gram_call(dim)(T_cg["Q"], I, dim, reg, gram))[0],
                         "gram_users": event_span(lambda: gram_call(dim)(T_cg["P"], U, dim, reg, gram))[0]}
                spans["cg_user_half_step"], counts["user"] = event_span(lambda: eng.als_half_step("user"))
                spans["cg_item_half_step"], counts["item"] = event_span(lambda: eng.als_half_step("item"))
                if with_cholesky:
                    eng._als = T_ch
                    spans["cholesky_user_half_step"] = event_span(lambda: eng.als_half_step("user"))[0]
                    spans["cholesky_item_half_step"] = event_span(lambda: eng.als_half_step("item"))[0]
                if r >= args.warmup:
                    for k, v in spans.items():
                        t[k].append(v)
        fits = {}
        for solver in ("cg",) + (("cholesky",) if with_cholesky else ()):
            with step(f"dim {dim}: fit_factors({args.iterations}, {solver})", 900):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit_counts = eng.fit_factors(dim=dim, iterations=args.iterations, regularization=reg, alpha=alpha, seed=seed,
                                             solver=solver, cg_steps=steps)
                torch.cuda.synchronize()
                fit_s = time.perf_counter() - t0
                P, _, Q, _ = eng.als_vectors()
                fits[solver] = {"wall_s": fit_s, "loss_float64": implicit_loss(torch, X, P, Q, reg, alpha),
                                "status": {s_: {str(k): v for k, v in c.items()} for s_, c in fit_counts.items()}}
        cfg.update({"ms": t, "median_ms": {k: med(v) for k, v in t.items()},
                    "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
                    "status_of_the_last_timed_cg_half_steps": {s_: {str(k): v for k, v in c.items()} for s_, c in counts.items()},
                    "fit_factors_iterations": args.iterations, "fit_factors": fits,
                    "mat_bytes_from_l2_per_half_step_COMPUTED": {side: int(n) * (steps + 1) * dim * dim * 4 for side, n in (("user", U), ("item", I))}})
        res["configs"].append(cfg)
        print(json.dumps({k: v for k, v in cfg.items() if k != "ms"}), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)
    return 0 if res["same_as_host_model"] else 1


if __name__ == "__main__":
    try:
        sys.exit(main())
    except StepTimeout as e:            # an overrun is reported as one (124, timeout's status), so that a caller starts nothing after it
        print(f"[als_bench] {e}", file=sys.stderr)
        sys.exit(124)
