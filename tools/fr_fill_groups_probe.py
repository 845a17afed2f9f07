"""What score_frows_kernel's first fill leaves for merge(), under the two groupings of a tile's columns (CPU only).

The first fill of an empty list ranks the 64 GROUP maxima of the tile and places the kk best; every other admissible sum
above the new kk-th entry (an "extra") goes through merge() one at a time.  Groups are either the lanes (a lane's REGS
consecutive columns: the kernel before round 12, and the 8-user form of 256-column tiles and up to 64 rows of W still) or
the strided groups of rtrec_amd.layouts.fr_fill_group_columns.  For a bench.py workload this script fits W with the C oracle, builds the
feature-row layout on the host, takes random users, and for each of them the first tile that holds an admissible non-zero
sum; it prints, per grouping, the extras per first fill (rtrec_amd.layouts.fr_first_fill_model) and how many of the
tile's true top-kk sums are not their group's maximum.

usage: python tools/fr_fill_groups_probe.py [--workload small] [--users 3000] [--top-k 10] [--tile-cols 256] [--threads 16]
(the c3 fit takes about five minutes on 16 cores, `small` seconds.)  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from oracle import slim_oracle as so
    from rtrec_amd.engine import merge_coefficients
    from rtrec_amd.layouts import build_feature_rows, fr_fill_group_columns, fr_first_fill_model
    from rtrec_amd.synth import workload_matrix

    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="small", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--tile-cols", type=int, default=256, choices=(128, 256))
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=12)
    args = ap.parse_args()
    wl = bench.WORKLOADS[args.workload]
    I, K, kk, tc = wl["I"], wl["K"], args.top_k + 1, args.tile_cols
    regs = tc // 64

    X = workload_matrix(wl, seed=20251003, float_ratings=True)
    Xc = X.tocsc()
    Xc.sort_indices()
    t0 = time.time()
    tg = np.arange(I)
    ptr, idx, val, _ = so.fit_columns(Xc, tg, nn_feature_selection=K, n_threads=args.threads)
    W = merge_coefficients(None, I, idx.astype(np.int64), np.repeat(tg, np.diff(ptr)), val).tocsc()
    W.sort_indices()
    fit_s = time.time() - t0
    cols = np.flatnonzero(np.diff(W.indptr) > 0).astype(np.int32)
    col_map = np.full(I, -1, dtype=np.int32)
    col_map[cols] = np.arange(len(cols), dtype=np.int32)
    L = build_feature_rows(W, 0, I, cols, col_map, tile_cols=tc)
    ids = np.asarray(L["fr_col_ids"])
    n_tiles = int(L["fr_n_tiles"])
    Wl = W.tocsr()[:, ids]                                     # columns in layout order

    rng = np.random.default_rng(args.seed)
    users = np.sort(rng.choice(X.shape[0], min(args.users, X.shape[0]), replace=False))
    gcols = {False: fr_fill_group_columns(regs, False), True: fr_fill_group_columns(regs, True)}
    tot = {g: dict(extras=0, inserted=0, top_not_max=0) for g in gcols}
    n_fills = 0
    for lo in range(0, len(users), 256):
        chunk = users[lo:lo + 256]
        S = np.zeros((len(chunk), n_tiles * tc), dtype=np.float32)
        S[:, :len(ids)] = np.asarray((X[chunk] @ Wl).todense(), dtype=np.float32)
        for i, u in enumerate(chunk):
            adm = np.ones(n_tiles * tc, dtype=bool)
            adm[:len(ids)] = ~np.isin(ids, X[u].indices)
            ok = (adm & (S[i] != 0)).reshape(n_tiles, tc)
            if not ok.any():
                continue
            t = int(np.flatnonzero(ok.any(axis=1))[0])
            s, a = S[i, t * tc:(t + 1) * tc], adm[t * tc:(t + 1) * tc]
            n_fills += 1
            vm = np.where(ok[t], s, -np.inf)
            top = np.argsort(-vm, kind="stable")[:min(kk, int(ok[t].sum()))]
            for strided, gc in gcols.items():
                m = fr_first_fill_model(s, a, kk, strided=strided)
                tot[strided]["extras"] += m["n_extras"]
                tot[strided]["inserted"] += m["n_inserted"]
                is_max = np.zeros(tc, dtype=bool)
                g_vm = vm[gc]
                best = regs - 1 - np.argmax(g_vm[:, ::-1], axis=1)
                is_max[gc[np.arange(64), best]] = g_vm.max(axis=1) > -np.inf
                tot[strided]["top_not_max"] += int((~is_max[top]).sum())
    n = max(n_fills, 1)
    out = {"workload": args.workload, "w_nnz": int(W.nnz), "w_rows": int(len(np.flatnonzero(np.diff(Wl.indptr) > 0))), "tile_cols": tc,
           "kk": kk, "users": int(len(users)), "first_fills": n_fills, "oracle_fit_seconds": round(fit_s, 1)}
    for strided, name in ((False, "lane_groups"), (True, "strided_groups")):
        out[name] = {"extras_per_fill": round(tot[strided]["extras"] / n, 2), "inserted_per_fill": round(tot[strided]["inserted"] / n, 2),
                     "top_kk_not_group_max_per_fill": round(tot[strided]["top_not_max"] / n, 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
