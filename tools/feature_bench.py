#!/usr/bin/env python3
"""What the representation kernel costs: csrc/feature_repr.hip on the shape of a bench.py workload -- every user and every item,
a feature row of the identity plus `--tags` (3) seeded tags from a vocabulary of `--vocab` (1,000), per-feature tables of
`--dims` (10, 62) components with biases (vectors of 12 and 64 slots).

Timed with device events on one stream after `--warmup` untimed rounds (`--reps` timed ones; medians beside the raw spans), the
compared forms INTERLEAVED round by round in one process.  A span holds `--inner` (20) back-to-back calls of one form and is
divided by that number: one launch takes tens of microseconds, too little for one pair of events.  Per dim_e:

  kernel_users_ms / kernel_items_ms   HipBackend.feature_repr into buffers allocated before the loop: the user launch (row-major
                                      output) and the item launch (component-major output, lanes of a job n_items floats apart);
                                      the one mapping that is built (one thread per slot)
  torch_users_ms / torch_items_ms     torch.sparse.mm on the same CSR against [bias | table], the stacked matrix assembled with
                                      torch.cat, and for the items the transpose to component-major (.t().contiguous())
  host_path_s                         what a caller had to do before: scipy `csr @ table` for both sides, utils.factors.stack_bias,
                                      SlimEngine.set_factors (host transpose and upload); wall clock, `--host-reps` rounds
  bytes                               what the kernel must move, computed from the shapes, and the rate that makes of the medians

The device results must equal the host model of tests/test_feature_repr_host.py bit for bit on a sample of `--sample` (200) rows
of each side, in the same run; the run fails otherwise.  Writes profiles/feature_<workload>.json with the build fingerprint.

    python tools/feature_bench.py --workload c3s

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
        print(f"[feature_bench] {name}: {time.perf_counter() - t0:.2f} s", file=sys.stderr, flush=True)


def feature_csr(n, vocab, tags, rng):
    """Identity column r plus `tags` distinct seeded tag columns n + t, ascending: the rows utils.factors.feature_rows builds."""
    import scipy.sparse as sp
    # (sorted draws from a range shortened by `tags`, spread by 0 .. tags-1: distinct and ascending without a shuffle per row)
    t = np.sort(rng.integers(0, vocab - tags + 1, (n, tags)), axis=1) + np.arange(tags)[None, :]
    col = np.concatenate([np.arange(n)[:, None], n + t], axis=1).astype(np.int32)
    ptr = (np.arange(n + 1, dtype=np.int64) * (tags + 1)).astype(np.int32)
    return sp.csr_matrix((np.ones(col.size, np.float32), col.ravel(), ptr), shape=(n, n + vocab))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3s")
    ap.add_argument("--dims", default="10,62", help="dim_e values; the vectors have two more slots (the stacked biases)")
    ap.add_argument("--tags", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls inside one timed span (a launch takes tens of microseconds)")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(ROOT, "profiles", f"feature_{args.workload}.json")

    import torch
    from bench import WORKLOADS
    from rtrec_amd import build
    from rtrec_amd._native import FEATURE_ITEM, FEATURE_USER
    from rtrec_amd.engine import SlimEngine
    from rtrec_amd.utils.factors import stack_bias
    from tests.test_feature_repr_host import ITEM, USER, repr_fast, same_bits
    wl = WORKLOADS[args.workload]
    U, I = int(wl["U"]), int(wl["I"])
    with step("start-up", 120):
        torch.zeros(1, device="cuda")
    eng = SlimEngine(device="cuda:0")
    be = eng.be
    rng = np.random.default_rng(20261019)
    med = lambda v: float(np.median(v)) if len(v) else None
    Fu, Fi = feature_csr(U, args.vocab, args.tags, rng), feature_csr(I, args.vocab, args.tags, rng)
    d_fu = (be.to_dev(Fu.indptr), be.to_dev(Fu.indices), None)                 # (all values are 1: d_f_val == NULL)
    d_fi = (be.to_dev(Fi.indptr), be.to_dev(Fi.indices), None)
    t_fu = torch.sparse_csr_tensor(d_fu[0], d_fu[1], torch.ones(Fu.nnz, dtype=torch.float32, device="cuda"), size=Fu.shape)
    t_fi = torch.sparse_csr_tensor(d_fi[0], d_fi[1], torch.ones(Fi.nnz, dtype=torch.float32, device="cuda"), size=Fi.shape)
    su, si = np.sort(rng.permutation(U)[:min(args.sample, U)]), np.sort(rng.permutation(I)[:min(args.sample, I)])

    def spans(fns, n):
        """Device-event spans (ms) of n rounds over the calls `fns` (name -> call), alternating, after args.warmup untimed rounds."""
        out, last = {name: [] for name in fns}, {}
        for r in range(args.warmup + n):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    last[name] = fn()
                b.record()
                b.synchronize()
                if r >= args.warmup:
                    out[name].append(a.elapsed_time(b) / args.inner)
        return out, last

    res = {"workload": f"{args.workload}: {wl['desc']} (its shape only: the feature rows are seeded here)", "n_users": U, "n_items": I,
           "tags_per_entity": args.tags, "tag_vocabulary": args.vocab, "entries_per_row": args.tags + 1, "biases": True,
           "warmup_rounds": args.warmup, "timed_rounds": args.reps, "calls_per_span": args.inner,
           "variants_built": ["plain: one thread per output slot (job = t / width, slot = t % width)"],
           "variants_not_built": ["transposing: a tile of 64 items staged in LDS and stored along the items"],
           "timing": "device events around each call, one stream, the compared forms alternating round by round; wall clock where it says so",
           "configs": [], "same_as_host_model": True, "build": build.fingerprint()}
    for dim_e in [int(d) for d in args.dims.split(",")]:
        dim = dim_e + 2
        Eu, Ei = rng.standard_normal((U + args.vocab, dim_e)).astype(np.float32), rng.standard_normal((I + args.vocab, dim_e)).astype(np.float32)
        bu, bi = rng.standard_normal(U + args.vocab).astype(np.float32), rng.standard_normal(I + args.vocab).astype(np.float32)
        d_eu, d_ei, d_bu, d_bi = be.to_dev(Eu), be.to_dev(Ei), be.to_dev(bu), be.to_dev(bi)
        d_tu, d_ti = torch.cat([d_bu[:, None], d_eu], dim=1).contiguous(), torch.cat([d_bi[:, None], d_ei], dim=1).contiguous()
        p, p_has = be.empty((U, dim), torch.float32), be.empty((U,), torch.uint8)
        qt, q_has = be.empty((dim, I), torch.float32), be.empty((I,), torch.uint8)
        ones_u, ones_i = torch.ones((U, 1), dtype=torch.float32, device="cuda"), torch.ones((I, 1), dtype=torch.float32, device="cuda")

        def kernel_users():
            be.feature_repr(None, d_fu, d_eu, dim_e, d_bu, FEATURE_USER, U, p, dim, 1, p_has)
            return p

        def kernel_items():
            be.feature_repr(None, d_fi, d_ei, dim_e, d_bi, FEATURE_ITEM, I, qt, 1, I, q_has)
            return qt

        def torch_users():
            s = torch.sparse.mm(t_fu, d_tu)
            return torch.cat([s[:, :1], ones_u, s[:, 1:]], dim=1)

        def torch_items():
            s = torch.sparse.mm(t_fi, d_ti)
            return torch.cat([ones_i, s], dim=1).t().contiguous()

        fns = {"kernel_users": kernel_users, "kernel_items": kernel_items}
        torch_error = None
        with step(f"torch.sparse.mm probe, dim_e {dim_e}", 300):
            try:
                torch_users(), torch_items()
                torch.cuda.synchronize()
                fns.update({"torch_users": torch_users, "torch_items": torch_items})
            except (RuntimeError, NotImplementedError) as e:            # (an operator this torch build lacks: recorded, not hidden)
                torch_error = f"{type(e).__name__}: {e}"[:300]
        with step(f"dim_e {dim_e}", 600):
            t, last = spans(fns, args.reps)
        # the same run's results against the host model on a sample of rows, bit for bit
        with step(f"host model, dim_e {dim_e}", 600):
            want_u = repr_fast(Fu.indptr, Fu.indices, None, Eu, bu, USER, su.astype(np.int32))
            want_i = repr_fast(Fi.indptr, Fi.indices, None, Ei, bi, ITEM, si.astype(np.int32))
            got_u = p[be.to_dev(su.astype(np.int64))].cpu().numpy()
            got_i = qt[:, be.to_dev(si.astype(np.int64))].cpu().numpy().T
            same = bool(same_bits(got_u, want_u[0]) and same_bits(got_i, want_i[0]) and bool(p_has.all()) and bool(q_has.all()))
            torch_diff = None
            if "torch_users" in last:
                torch_diff = {"users_max_abs": float((last["torch_users"][be.to_dev(su.astype(np.int64))].cpu().numpy() - want_u[0]).__abs__().max()),
                              "items_max_abs": float((last["torch_items"][:, be.to_dev(si.astype(np.int64))].cpu().numpy().T - want_i[0]).__abs__().max())}
        res["same_as_host_model"] &= same
        # the host path a caller had before: scipy products, stack_bias, set_factors (transpose + upload)
        host = []
        with step(f"host path, dim_e {dim_e}", 900):
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                P, Q = stack_bias(Fu @ bu, Fu @ Eu, Fi @ bi, Fi @ Ei)
                eng.set_factors(P, Q)
                torch.cuda.synchronize()
                host.append(time.perf_counter() - t0)
            same_host = bool(same_bits(P[su], want_u[0]) and same_bits(Q[si], want_i[0]))
            eng.clear_factors()
        bytes_users = Fu.nnz * (4 + 4 * (dim_e + 1)) + 4 * (U + 1) + 4 * U * dim + U
        bytes_items = Fi.nnz * (4 + 4 * (dim_e + 1)) + 4 * (I + 1) + 4 * I * dim + I
        cfg = {"dim_e": dim_e, "dim": dim, "same_as_host_model_on_the_sample": same, "scipy_host_path_same_as_host_model_on_the_sample": same_host,
               "spans_ms": t, "median_ms": {k: med(v) for k, v in t.items()}, "min_max_ms": {k: [float(min(v)), float(max(v))] for k, v in t.items()},
               "kernel_both_launches_median_ms": med(t["kernel_users"]) + med(t["kernel_items"]),
               "torch_both_median_ms": (med(t["torch_users"]) + med(t["torch_items"])) if "torch_users" in t else None,
               "torch_sparse_mm_error": torch_error, "torch_minus_host_model_on_the_sample": torch_diff,
               "host_path_s": host, "host_path_median_s": med(host),
               "bytes_needed": {"users": int(bytes_users), "items": int(bytes_items),
                                "note": "gathered table rows and bias once per entry, columns, offsets, the output and has; computed from the shapes"},
               "gb_per_s_at_the_median": {"users": bytes_users / (med(t["kernel_users"]) * 1e-3) / 1e9,
                                          "items": bytes_items / (med(t["kernel_items"]) * 1e-3) / 1e9}}
        res["configs"].append(cfg)
        print(json.dumps({k: v for k, v in cfg.items() if k not in ("spans_ms", "host_path_s")}), flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)
        del p, qt, d_eu, d_ei, d_tu, d_ti, last
    return 0 if res["same_as_host_model"] else 1


if __name__ == "__main__":
    try:
        sys.exit(main())
    except StepTimeout as e:            # an overrun is reported as one (124, timeout's status), so that a caller starts nothing after it
        print(f"[feature_bench] {e}", file=sys.stderr)
        sys.exit(124)
