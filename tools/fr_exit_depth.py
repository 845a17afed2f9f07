"""Histogram of the depth at which the jobs of score_frows_kernel end: super-tiles worked on (streaming form) or the
fragment at which a wave left (resident form; n_frags = it went to the end of W).

usage: RTREC_AMD_LIB=<a -DSCORE_PROFILE build> python tools/fr_exit_depth.py [bench.py arguments]
Runs bench.py in this process, then reads the library's counters (rtrec_amd_fr_exit_depth) and prints one JSON line."""
import ctypes
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    print(json.dumps({"fr_exit_depth": {"jobs": total, "hist": hist,
                                        "share": {i: round(v / total, 4) for i, v in hist.items()}}}), flush=True)


if __name__ == "__main__":
    main()
