"""Where the waves of score_frows_kernel leave their jobs, and what they swept on the way.

Depth = the fragment at which a wave left its job (n_frags = it went to the end of W).  Beside the histogram the raw
phase counters of the -DSCORE_PROFILE build are printed: wave ticks per phase, `n_dense` = (wave, row) pairs swept and
`n_gather` = those of them that were fetched through the wave's row ring (the rows behind the resident head).
In score_frows_kernel the tile loop is split three ways: `dense` = the sweep and the tile tests, `select` = the candidate
block of users whose list is full, `sparse` = the candidate block of users whose kk-th entry is still empty (the first
fill).  `n_overflow` counts those first fills, `rowptr` the candidates they buffered or placed, `reset` those of them that
entered a list; `n_sparse_chunks` / `n_sparse_rows` count merge() rounds / insertions of every user.

usage: RTREC_AMD_LIB=<a -DSCORE_PROFILE build> python tools/fr_exit_depth.py [bench.py arguments]
Runs bench.py in this process, then reads the library's counters (rtrec_amd_fr_exit_depth, rtrec_amd_score_profile) and
prints one JSON line."""
import ctypes
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASES = ["jobs", "rowptr", "hdr", "group", "dense", "sparse", "select", "emit", "reset", "queue",
          "n_dense", "n_sparse_rows", "n_sparse_chunks", "n_overflow", "total", "n_gather"]


def main():
    path = os.environ.get("RTREC_AMD_LIB")
    if not path:
        sys.exit("RTREC_AMD_LIB must name a -DSCORE_PROFILE build of the library")
    sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
    sys.path.insert(0, ROOT)
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    except SystemExit as e:
        if e.code not in (None, 0):
            raise
    lib = ctypes.CDLL(path)                  # (loaded by the package by now: the same handle, the same counters)
    fn = getattr(lib, "rtrec_amd_fr_exit_depth", None)
    if fn is None:
        sys.exit(f"{path} is not a -DSCORE_PROFILE build")
    buf = (ctypes.c_uint32 * 257)()
    if fn(buf, 0) != 0:
        sys.exit("reading the counters failed")
    hist = {i: int(v) for i, v in enumerate(buf) if v}
    total = max(sum(hist.values()), 1)
    out = {"fr_exit_depth": {"jobs": total, "hist": hist, "share": {i: round(v / total, 4) for i, v in hist.items()}}}
    prof = getattr(lib, "rtrec_amd_score_profile", None)
    if prof is not None:                     # the timed steps' totals: bench.py reset them after its warm-up
        raw = (ctypes.c_uint64 * 16)()
        if prof(raw, 0) == 0:
            out["score_profile_raw"] = dict(zip(PHASES, [int(x) for x in raw]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
